"""Reserve and settle on the CPU: the lane bodies of csrc/reserve_lanes.h compiled for the host by tests/hostcheck/reserve_check.cpp, a
stand-alone program with its own main -- run plain and under AddressSanitizer / UBSan with every buffer in a heap block of exactly its
size -- and the PREP lines it prints (settle's per-lane pass over t = 0, 1, s - 1, s, s + 1, s + l, 2^200 + 1, s = 0, key_index =
nkeys - 1, nkeys, 255, records at odd addresses, no amounts at all) against the definitions recomputed with oracle/pymodel.blake3
(tests/reserve_cases.py).  The same bodies run on the GPU in tests/test_gpu_reserve.py and tests/test_gpu_settle.py."""
import os
import re
import subprocess

import pytest

import reserve_cases as rc
from conftest import ELL, ROOT


def run_program(tmp_path, sanitized):
    exe = rc.build_program(str(tmp_path / ("reserve_check_asan" if sanitized else "reserve_check")), sanitized)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "RESERVE CHECK CLEAN" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-6000:]
    return r.stdout


@pytest.fixture(scope="module")
def plain_output(tmp_path_factory):
    return run_program(tmp_path_factory.mktemp("reserve_check"), False)


def test_lane_bodies_plain(plain_output):
    assert plain_output.count("PREP ") == 2 * 17      # seventeen cases, at an even and at an odd address


def test_lane_bodies_as_a_sanitized_stand_alone_program(tmp_path, plain_output):
    """exact-size heap blocks at even and odd addresses, the grid's tail lanes, n = 1, 65, 257 and 1025; nothing is preloaded.  The
    sanitized run computes what the plain run computes"""
    assert run_program(tmp_path, True) == plain_output


def test_settle_prep_lane_against_the_model(plain_output):
    rows = [ln.split() for ln in plain_output.splitlines() if ln.startswith("PREP ")]
    seen = set()
    for _, rec, kidx, t, nkeys, st, tr, tm, ta in rows:
        rec, kidx, nkeys, st = bytes.fromhex(rec), int(kidx), int(nkeys), int(st)
        tv = 0 if t == "-" else int.from_bytes(bytes.fromhex(t), "little")
        want = rc.prep(rec, kidx, tv, nkeys)
        assert (st, bytes.fromhex(tr), bytes.fromhex(tm), bytes.fromhex(ta)) == want, (rec.hex(), kidx, t)
        s = int.from_bytes(rec[64:], "little")
        label = None if t == "-" else "big" if tv == 2**200 + 1 else tv - s      # the amount relative to the record's s
        seen.add((label, s % ELL == 0, kidx - nkeys if kidx < 255 else 255, st))
    # the cases the issue names, each with the answer it must have
    S = 300
    for case in ((-S, False, -3, 0), (1 - S, False, -3, 0), (-1, False, -3, 0), (0, False, -3, 0), (1, False, -3, 249), (ELL, False, -2, 0), ("big", False, -1, 249),
                 (None, False, -3, 0), (0, True, -3, 0), (1, True, -3, 249), (ELL, True, -3, 0), (None, True, -3, 0),
                 (5 - S, False, -1, 0), (5 - S, False, 0, 248), (5 - S, False, 255, 248), (1, False, 0, 248)):
        assert case in seen, (case, sorted(map(str, seen)))


def test_the_model_against_hand_written_lanes():
    rc.check_model()


def test_statuses_counts_and_prototypes_in_the_header_the_bindings_and_the_rust_block():
    hd = open(os.path.join(ROOT, "include", "act_mi355x.h")).read()
    rs = open(os.path.join(ROOT, "rust", "src", "mi355x.rs")).read()
    lanes = open(os.path.join(ROOT, "anonymous-credit-tokens_amd", "csrc", "reserve_lanes.h")).read()
    assert re.search(r"#define ACT_RESERVE_COUNTS 11\b", hd) and re.search(r"#define ACT_SETTLE_COUNTS 7\b", hd)
    assert re.search(r"#define ACT_STATUS_NOT_RESERVED 248\b", hd) and re.search(r"#define ACT_STATUS_SETTLED_OTHER_AMOUNT 247\b", hd)
    from act_amd import capi
    assert (capi.STATUS_NOT_RESERVED, capi.STATUS_SETTLED_OTHER_AMOUNT, capi.RESERVATION_BYTES) == (rc.NOT_RESERVED, rc.SETTLED_OTHER_AMOUNT, 96)
    assert tuple(capi.RESERVE_COUNTS) == rc.RESERVE_COUNTS and len(rc.RESERVE_COUNTS) == 11 and tuple(capi.SETTLE_COUNTS) == rc.SETTLE_COUNTS and len(rc.SETTLE_COUNTS) == 7
    for name in ("act_redeem_reserve_batch", "act_redeem_cbor_reserve_batch", "act_redeem_settle_batch", "act_redeem_cbor_settle_batch"):
        assert name in capi.EXPORTS and re.search(r"\bint %s\(" % name, hd) and re.search(r"\bfn %s\(" % name, rs), name
    for label in (rc.LABEL_RES, rc.LABEL_SETTLED):
        assert label.rstrip(b"\0").decode() in hd and label.rstrip(b"\0").decode() in lanes
    assert "ACT_SETTLE_COUNTS: usize = 7" in rs and "ACT_RESERVE_COUNTS: usize = 11" in rs and "pub struct GpuReserve" in rs
