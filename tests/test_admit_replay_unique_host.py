"""The replay unique forms on the CPU: the serve pass (csrc/copy_lanes.h: copy_serve_lane / copy_serve_piece) compiled for the host by
tests/hostcheck/copy_serve_check.cpp -- every row of the header's table, row sizes 1, 16, 17, 128 and the framed Refund, bases 0 to 3
bytes past an aligned address, out_replayed null and not, 0, 1 and 4 096 copies behind a leader, every byte around the rows -- and the
Python model of act_redeem_(cbor_)admit_replay_unique_batch (tests/admit_replay_unique_cases.py), which is held to hand-written
expectations for the fixed lane mix and to the model of act_redeem_(cbor_)admit_replay_batch on the seeded plans.  The same bodies run
on the GPU in tests/test_gpu_admit_replay_unique.py."""
import ctypes as C
import os
import re
import subprocess

import pytest

import admit_replay_cases as ar
import admit_replay_unique_cases as aru
import copies_cases as cp
from conftest import ROOT


@pytest.fixture(scope="module")
def serve_check():
    return aru.load_serve_check(aru.build_serve_check(os.path.join(ROOT, "tests", "hostcheck", "libcopy_serve_check.so")))


# ---- 1. the model -------------------------------------------------------------------------------------------------------------------------------
def test_the_model_against_the_hand_written_lane_mix():
    aru.check_model_on_fixed_mix()
    # what the issue's table says in words
    st, rep, copy_of = aru.FIXED_EXPECT, aru.FIXED_REPLAYED, aru.FIXED_COPY_OF
    assert (st[0:3], rep[0:3], copy_of[0:3]) == ([0, 0, 0], [0, 1, 1], [None, 0, 0])                     # a. one fresh leader, two served copies
    assert (st[3:5], rep[3:5], copy_of[3:5]) == ([0, 0], [1, 1], [None, 3])                              # b. a retry candidate and its copy: served
    assert st[5:7] == [3, 3] and copy_of[5:7] == [None, None]                                            # c. shed by the screen, never copies
    assert st[7:9] == [7, 7] and copy_of[8] == 7                                                         # d. 7 and 7
    assert st[9:12] == [0, 3, 3] and copy_of[9:12] == [None, None, 10]                                   # e. the second proof loses behind verification, and so does its copy
    assert st[12:14] == [250, 250] and copy_of[12:14] == [None, None]                                    # f. neither is a copy
    assert st[14:16] == [0, 0] and rep[14:16] == [1, 1] and copy_of[14:16] == [None, None]               # g. verified and replayed, not copies
    assert aru.FIXED_COUNTS_RECORDS["foreign_spend"] == 2 and aru.FIXED_COUNTS_RECORDS["copies"] == 5 and aru.FIXED_COUNTS_RECORDS["copies_served"] == 3


def test_the_model_equals_the_admit_replay_model_on_the_seeded_plans():
    aru.check_model_on_plans()


def test_the_table_of_the_header():
    assert aru.serve(0, 2) == (0, 2, 1, True)
    for s in (255, 6, 7, aru.DOUBLE_SPEND, aru.UNDETERMINED, aru.RECORDED_UNSIGNED):
        assert aru.serve(s, 1) == (s, 1, 0, False)
    # where the admission unique forms say DOUBLE_SPEND, the replay unique forms serve or repeat
    assert cp.copy_status(0) == cp.copy_status(aru.RECORDED_UNSIGNED) == aru.DOUBLE_SPEND


# ---- 2. the plan seeds ----------------------------------------------------------------------------------------------------------------------------
def test_plan_seeds_fill_every_category():
    """what tests/test_gpu_admit_replay_unique.py asserts again on the GPU box before it compares anything"""
    n = aru.PLAN_N
    assert n == 8209
    for num, den in aru.FRACTIONS:
        assert aru.plan_seed(num, den) == aru.find_seed(n, num, den)
        for with_charges in (False, True):
            plan, tokens = aru.copy_plan(n, num, den, aru.plan_seed(num, den), with_charges)
            cats, ds, c = aru.plan_categories(plan, with_charges)
            print(num, den, with_charges, tokens, cats, ds)
            assert set(cats) == set(aru.CATEGORIES) and len(aru.CATEGORIES) == 5
            assert all(16 * v >= n for v in cats.values()) and ds >= 16, (num, den, with_charges, cats, ds)
            aru.check_identities(c)


# ---- 3. the serve pass ----------------------------------------------------------------------------------------------------------------------------
def test_the_wire_row_is_no_multiple_of_four():
    assert aru.refund_wire_bytes(8) == aru.refund_wire_bytes(128) == 141 and 141 % 4 == 1


def test_the_serve_pass_in_the_check_files_own_cases(serve_check):
    sizes = aru.serve_row_sizes()
    assert {1, 128, aru.refund_wire_bytes(8), aru.refund_wire_bytes(128)} <= set(sizes)
    assert serve_check.hc_copy_serve_checks((C.c_uint64 * len(sizes))(*sizes), len(sizes)) == 0


@pytest.mark.parametrize("pieces", [False, True])
def test_the_serve_pass_against_the_table_written_in_python(serve_check, pieces):
    for out_b in aru.serve_row_sizes():
        for base_off in range(4):
            for with_replayed in (False, True):
                aru.check_serve_against_the_table(serve_check, out_b, base_off, with_replayed, pieces, n=300 if out_b > 17 else 700)


def test_the_serve_pass_costs_no_field_operation(serve_check):
    """the figure the documents state beside the measured ratios: byte movement only"""
    before = serve_check.hc_copy_serve_field_ops()
    aru.check_serve_against_the_table(serve_check, 141, 1, True, False)
    aru.check_serve_against_the_table(serve_check, 128, 0, True, True)
    assert serve_check.hc_copy_serve_field_ops() == before == 0
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"serve pass[^.]*\*\*0 field operations per lane\*\*", design), "DESIGN.md section 4.9 does not state the count"


# ---- 4. sanitizers ----------------------------------------------------------------------------------------------------------------------------------
def test_the_serve_pass_as_a_sanitized_stand_alone_program(tmp_path):
    """copy_serve_check.cpp with its own main under AddressSanitizer and UBSan: exact-size heap arrays behind the guards, the grid's
    tail lanes, rows at every base offset, the load / store pieces at every address mod 16"""
    exe = aru.build_serve_program(str(tmp_path / "copy_serve_check_asan"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe] + [str(b) for b in aru.serve_row_sizes()], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "COPY SERVE CHECK CLEAN" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-6000:]


# ---- 5. header, binding, Rust -----------------------------------------------------------------------------------------------------------------------
def test_counts_and_prototypes_in_the_header():
    hd = open(os.path.join(ROOT, "include", "act_mi355x.h")).read()
    assert re.search(r"#define ACT_ADMIT_REPLAY_UNIQUE_COUNTS 13\b", hd) and re.search(r"#define ACT_ADMIT_REPLAY_COUNTS 11\b", hd)
    from act_amd import capi
    assert tuple(capi.ADMIT_REPLAY_UNIQUE_COUNTS) == aru.COUNTS and capi.ADMIT_REPLAY_UNIQUE_COUNTS[:11] == capi.ADMIT_REPLAY_COUNTS == ar.COUNTS
    assert capi.ADMIT_REPLAY_UNIQUE_COUNTS[11:] == ("copies", "copies_served")
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", hd, flags=re.S))
    for new, old in (("act_redeem_admit_replay_unique_batch", "act_redeem_admit_replay_batch"),
                     ("act_redeem_cbor_admit_replay_unique_batch", "act_redeem_cbor_admit_replay_batch")):
        assert new in capi.EXPORTS
        params = {name: re.search(r"\bint %s ?\(([^;]*?)\) ?;" % name, flat).group(1) for name in (new, old)}
        assert params[new] == params[old], new          # the same parameters
    for word in ("copies_served", "leader 0, fresh or replayed"):
        assert word in hd
    rs = open(os.path.join(ROOT, "rust", "src", "mi355x.rs")).read()
    assert "fn act_redeem_admit_replay_unique_batch(" in rs and "fn act_redeem_cbor_admit_replay_unique_batch(" in rs
    assert rs.count("pub fn unique(mut self, on: bool)") == 2         # Admission's and GpuReplay's
    assert "pub const ACT_ADMIT_REPLAY_UNIQUE_COUNTS: usize = 13;" in rs


def test_unique_without_admit_is_refused_by_the_python_layer():
    from act_amd import api
    ring = api.Keyring([api.PrivateKey(bytes(64))])
    for call in (ring.redeem_replay_batch, ring.redeem_replay_cbor_batch, ring.keys[0].redeem_replay_batch, ring.keys[0].redeem_replay_cbor_batch):
        with pytest.raises(ValueError, match="admit=True"):
            call(None, None, None, [], bytes(32), unique=True)
