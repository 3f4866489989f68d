"""Admission before verification on the CPU: the lane bodies of the admission kernels (csrc/admit_lanes.h, csrc/null_probe.h) compiled
for the host by tests/hostcheck/admit_check.cpp -- the decision function, the screen over a table built with the set's slot function,
the stable compaction, the gather / scatter index arithmetic and the framing compare -- against the Python model of
tests/admission_cases.py, which is itself held to hand-written expectations for the fixed lane mix.  The same bodies run on the GPU
in tests/test_gpu_admission.py."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

import admission_cases as ad
from conftest import ROOT, load_golden
from test_cbor import _variants


@pytest.fixture(scope="module")
def admit_check():
    return C.CDLL(ad.build_admit_check(os.path.join(ROOT, "tests", "hostcheck", "libadmit_check.so")))


def golden_records():
    g = load_golden("lifecycle_L128.json")
    return [bytes.fromhex(c["proof"]) for c in g["cases"][:2]], 128


def test_the_model_against_the_hand_written_lane_mix():
    ad.check_model_on_fixed_mix()


def test_status_and_counts_in_the_header():
    hd = open(os.path.join(ROOT, "include", "act_mi355x.h")).read()
    assert re.search(r"#define ACT_STATUS_WRONG_CHARGE 250\b", hd) and re.search(r"#define ACT_ADMIT_COUNTS 8\b", hd)
    taken = {int(v) for v in re.findall(r"#define ACT_STATUS_\w+ (\d+)", hd)}
    assert {251, 252, 253, 254, 255} <= taken and len(re.findall(r"#define ACT_STATUS_\w+ 250\b", hd)) == 1
    from act_amd import capi
    assert capi.STATUS_WRONG_CHARGE == 250 and len(capi.ADMIT_COUNTS) == 8 == len(ad.COUNTS) and tuple(capi.ADMIT_COUNTS) == ad.COUNTS
    for name in ("act_redeem_admit_batch", "act_redeem_cbor_admit_batch"):
        assert name in capi.EXPORTS and re.search(r"\bint %s\(" % name, hd)


def test_decision_and_screen(admit_check):
    ad.check_decision(admit_check)
    ad.check_screen(admit_check)


def test_compaction_is_stable(admit_check):
    ad.check_compaction(admit_check)


def test_gather_and_scatter(admit_check):
    ad.check_gather_scatter(admit_check)
    ad.check_patch(admit_check)


def test_framing_compare_against_the_template(admit_check):
    records, L = golden_records()
    ad.check_framing(admit_check, records, L, lambda rec: _variants("SpendProof", rec, L))


def test_density_seeds_fill_every_category():
    """what tests/test_gpu_admission.py asserts again on the GPU box before it compares anything"""
    n = ad.DENSITY_N
    for num, den in ((1, 8), (1, 2), (7, 8)):
        seed = ad.density_seed(num, den)
        for with_charges in (False, True):
            plan, tokens = ad.density_plan(n, num, den, seed, with_charges)
            cats, st, c = ad.plan_categories(plan, with_charges)
            assert all(16 * v >= n for v in cats.values()), (num, den, with_charges, cats)
            assert set(cats) == {"accepted", "spent_before", "rejected_by_verification", "in_batch_duplicate"} | ({"wrong_charge"} if with_charges else set())
            shed = c["spent_before"] + c["wrong_charge"]
            assert abs(shed / n - num / den) < 0.02 and tokens <= n
    for num, den, want in ((0, 1, 0), (1, 1, n)):
        plan, _ = ad.density_plan(n, num, den, ad.density_seed(num, den), True)
        _, _, c = ad.plan_categories(plan, True)
        assert c["spent_before"] + c["wrong_charge"] == want and c["verified"] == n - want


# the scalar-memory write instructions that this code base never uses, spelled in two halves so that this file does not hold them
FORBIDDEN = tuple("s" + "_" + stem for stem in ("store_dword", "buffer_store", "scratch_store", "atomic_", "buffer_atomic", "dcache_wb", "dcache_discard"))
NEW_SOURCES = ("anonymous-credit-tokens_amd/csrc/k_admit.hip", "anonymous-credit-tokens_amd/csrc/admit_lanes.h", "anonymous-credit-tokens_amd/csrc/admit.h",
               "anonymous-credit-tokens_amd/csrc/admit_impl.inc", "anonymous-credit-tokens_amd/csrc/null_probe.h", "tests/hostcheck/admit_check.cpp",
               "tests/admission_cases.py", "tests/test_gpu_admission.py", "tests/test_gpu_ring_finish.py", "tests/admission_sanitize_driver.py", "tools/admission_probe.py")


def test_new_sources_use_no_scalar_memory_writes():
    """the compaction has no atomic on a single counter either: its kernels use none at all"""
    for rel in NEW_SOURCES:
        src = open(os.path.join(ROOT, rel)).read().lower()
        for w in FORBIDDEN:
            assert w not in src, (rel, w)
    k = open(os.path.join(ROOT, NEW_SOURCES[0])).read()
    body = k[k.index("k_admit_count"):k.index("k_admit_rows")]
    assert "atomic" not in re.sub(r"//[^\n]*", "", body)


def test_admission_lane_bodies_under_asan_ubsan(tmp_path):
    libasan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(libasan) or not os.path.exists(libasan):
        pytest.skip("no libasan in this toolchain")
    so = ad.build_admit_check(str(tmp_path / "libadmit_check_asan.so"), sanitize=True)
    env = dict(os.environ, LD_PRELOAD=libasan, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "admission_sanitize_driver.py"), so], capture_output=True, text=True, env=env, timeout=1500)
    assert r.returncode == 0 and "ADMISSION SANITIZERS CLEAN" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-6000:]
