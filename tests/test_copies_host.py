"""Admission's copy stage on the CPU: the lane bodies of the copy kernels (csrc/copy_lanes.h) compiled for the host by
tests/hostcheck/copy_check.cpp -- the fingerprint, the leader table, the exact compare, the side array and the resolve pass -- and the
Python model of act_redeem_(cbor_)admit_unique_batch (tests/copies_cases.py), which is held to hand-written expectations for the
fixed lane mix and to the model of the existing admission loop everywhere else.  The same bodies run on the GPU in
tests/test_gpu_copies.py."""
import os
import re
import subprocess
import sys

import pytest

import admission_cases as ad
import copies_cases as cp
from conftest import ROOT


@pytest.fixture(scope="module")
def copy_check():
    return cp.load_copy_check(cp.build_copy_check(os.path.join(ROOT, "tests", "hostcheck", "libcopy_check.so")))


def test_the_model_against_the_hand_written_lane_mix():
    cp.check_model_on_fixed_mix()


def test_the_model_equals_the_admission_model_on_the_seeded_plans():
    cp.check_model_on_plans()


def test_plan_seeds_fill_every_category():
    """what tests/test_gpu_copies.py asserts again on the GPU box before it compares anything: with the chosen seeds accepted,
    rejected-by-verification, copies of valid leaders and copies of tampered leaders each hold at least 1/16 of the lanes"""
    n = cp.PLAN_N
    for num, den in ((1, 2), (7, 8)):
        assert cp.plan_seed(num, den) == cp.find_seed(n, num, den)
        for with_charges in (False, True):
            plan, tokens = cp.copy_plan(n, num, den, cp.plan_seed(num, den), with_charges)
            cats, c = cp.plan_categories(plan, with_charges)
            assert set(cats) == {"accepted", "rejected_by_verification", "copies_of_valid", "copies_of_tampered"}
            assert all(16 * v >= n for v in cats.values()), (num, den, with_charges, cats)
            cp.check_identities(c)
    plan, _ = cp.copy_plan(n, 0, 1, cp.plan_seed(0, 1), True)
    assert all(p.copy_of is None for p in plan)


def test_counts_and_prototypes_in_the_header():
    hd = open(os.path.join(ROOT, "include", "act_mi355x.h")).read()
    assert re.search(r"#define ACT_ADMIT_UNIQUE_COUNTS 9\b", hd) and re.search(r"#define ACT_ADMIT_COUNTS 8\b", hd)
    from act_amd import capi
    assert tuple(capi.ADMIT_UNIQUE_COUNTS) == cp.COUNTS and capi.ADMIT_UNIQUE_COUNTS[:8] == capi.ADMIT_COUNTS == ad.COUNTS
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", hd, flags=re.S))
    for new, old in (("act_redeem_admit_unique_batch", "act_redeem_admit_batch"), ("act_redeem_cbor_admit_unique_batch", "act_redeem_cbor_admit_batch")):
        assert new in capi.EXPORTS
        params = {name: re.search(r"\bint %s ?\(([^;]*?)\) ?;" % name, flat).group(1) for name in (new, old)}
        assert params[new] == params[old], new          # the same parameters
    rs = open(os.path.join(ROOT, "rust", "src", "mi355x.rs")).read()
    assert "fn act_redeem_admit_unique_batch(" in rs and "fn act_redeem_cbor_admit_unique_batch(" in rs and "pub fn unique(mut self, on: bool)" in rs


def test_fingerprint(copy_check):
    cp.check_fingerprint(copy_check)


def test_leader_table_against_a_dictionary(copy_check):
    cp.check_leader(copy_check)


def test_compare_is_exact(copy_check):
    cp.check_compare(copy_check)


def test_resolve_and_the_whole_stage(copy_check):
    cp.check_resolve(copy_check)
    cp.check_stage(copy_check)


def test_the_unit_is_in_both_libraries():
    mk = open(os.path.join(ROOT, "anonymous-credit-tokens_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, flags=re.M).group(1).split()
    assert "k_copies.hip" in srcs and "$(patsubst %.hip,fast_%.o,$(SRCS))" in mk
    hdrs = re.search(r"^HDRS := (.*)$", mk, flags=re.M).group(1).split()
    assert {"copy_lanes.h", "copies_impl.inc"} <= set(hdrs)


def test_copy_lane_bodies_under_asan_ubsan(tmp_path):
    libasan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(libasan) or not os.path.exists(libasan):
        pytest.skip("no libasan in this toolchain")
    so = cp.build_copy_check(str(tmp_path / "libcopy_check_asan.so"), sanitize=True)
    env = dict(os.environ, LD_PRELOAD=libasan, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "copies_sanitize_driver.py"), so], capture_output=True, text=True, env=env, timeout=1500)
    assert r.returncode == 0 and "COPIES SANITIZERS CLEAN" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-6000:]
