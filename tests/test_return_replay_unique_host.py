"""The return replay unique forms on the CPU: the serve pass (csrc/copy_lanes.h: copy_serve_return_lane / copy_serve_return_piece)
compiled for the host by tests/hostcheck/copy_serve_return_check.cpp and held to the table of the header written in Python -- every row,
for a copy that names its leader's amount, that amount + l, and another amount; row sizes 1, 16, 17, 160 and the framed RefundReturn;
bases 0 to 3 bytes past an aligned address; every byte around the rows -- and the Python model of
act_redeem_(cbor_)return_replay_unique_batch (tests/return_replay_unique_cases.py), which is held to hand-written expectations and to
the model of act_redeem_(cbor_)return_replay_batch on the seeded plans.  The same bodies run on the GPU in
tests/test_gpu_return_replay_unique.py."""
import ctypes as C
import os
import re
import subprocess

import pytest

import admit_replay_unique_cases as aru
import return_replay_cases as rr
import return_replay_unique_cases as ru
from conftest import ROOT


@pytest.fixture(scope="module")
def check():
    return ru.load_check(ru.build_check(os.path.join(ROOT, "tests", "hostcheck", "libcopy_serve_return_check.so")))


# ---- 1. the table and the model ---------------------------------------------------------------------------------------------------------------
def test_the_table_of_the_header():
    for key in (0, 1, 255):
        assert ru.serve(0, key, True) == (0, key, 1, True)
        assert ru.serve(0, key, False) == (ru.DOUBLE_SPEND, key, 0, False)
        assert ru.serve(ru.RECORDED_UNSIGNED, key, False) == (ru.DOUBLE_SPEND, key, 0, False)
        assert ru.serve(ru.RECORDED_UNSIGNED, key, True)[:2] == (ru.RECORDED_UNSIGNED, key) and not ru.serve(ru.RECORDED_UNSIGNED, key, True)[3]
        for s in (255, 6, 7, ru.DOUBLE_SPEND, ru.UNDETERMINED):
            assert ru.serve(s, key, True) == ru.serve(s, key, False) == (s, key, 0, False)
    # with the leader's amount it is the table of the replay unique forms in status, key and record
    for s in (0, 255, 6, 7, ru.DOUBLE_SPEND, ru.UNDETERMINED, ru.RECORDED_UNSIGNED):
        a, b = ru.serve(s, 1, True), aru.serve(s, 1)
        assert (a[0], a[1], a[3]) == (b[0], b[1], b[3]) and (a[2] == b[2] or s == ru.RECORDED_UNSIGNED)


def test_the_model_against_hand_written_mixes_and_the_plain_model():
    rr.check_model()
    ru.check_model_on_fixed_mixes()


def test_the_model_equals_the_return_replay_model_on_the_seeded_plans():
    """the seeds are the smallest whose plans hold every kind of copy the table tells apart (what the GPU tests assert again)"""
    for n in ru.PLAN_SIZES:
        for num, den in ru.FRACTIONS:
            assert ru.plan_seed(n, num, den) == ru.find_seed(n, num, den)
    ru.check_model_on_plans()


def test_nothing_returned_is_the_model_of_the_replay_unique_forms():
    for num, den in aru.FRACTIONS:
        plan, _ = aru.copy_plan(600, num, den, aru.plan_seed(num, den), True)
        lanes, blobs, charges, spent, receipts = aru.plan_lanes(plan)
        want = aru.model(lanes, blobs, set(spent), set(receipts), charges)
        for returned in (None, [0] * 600, [rr.ELL] * 600):
            got = ru.model(lanes, blobs, set(spent), {(k, kp, 0) for k, kp in receipts}, charges, returned)
            assert got[:3] == want[:3] and got[4] == want[4]
            assert {k: v for k, v in got[3].items() if k not in ("return_too_big", "copies_other_amount")} == want[3]
            assert got[3]["return_too_big"] == got[3]["copies_other_amount"] == 0


# ---- 2. the serve pass ------------------------------------------------------------------------------------------------------------------------
def test_the_row_sizes_cover_whole_and_short_last_pieces():
    """the framed RefundReturn is 176 bytes, eleven whole pieces; 1 and 17 end in a short piece, and a row of 17 starts at every address mod 16"""
    assert ru.refund_return_wire_bytes(8) == ru.refund_return_wire_bytes(128) == 176
    assert ru.serve_row_sizes() == [1, 16, 17, 160, 176]


def test_the_amounts_compare_reduced(check):
    le = lambda v: v.to_bytes(32, "little")
    for t in (0, 1, 3, rr.ELL - 1):
        assert check.hc_same_amount(le(t), le(t)) == 1 and check.hc_same_amount(le(t), le(t + rr.ELL)) == 1 and check.hc_same_amount(le(t + rr.ELL), le(t)) == 1
        assert check.hc_same_amount(le(t), le((t + 1) % rr.ELL)) == 0 and check.hc_same_amount(le(t), le(t + (1 << 255))) == (1 if (1 << 255) % rr.ELL == 0 else 0)
    big = (1 << 256) - 1
    assert check.hc_same_amount(le(big), le(big % rr.ELL)) == 1


def test_the_serve_pass_in_the_check_files_own_cases(check):
    sizes = ru.serve_row_sizes()
    assert {1, 16, 17, 160, ru.refund_return_wire_bytes(8)} == set(sizes)
    assert check.hc_serve_return_checks((C.c_uint64 * len(sizes))(*sizes), len(sizes)) == 0


@pytest.mark.parametrize("pieces", [False, True])
def test_the_serve_pass_against_the_table_written_in_python(check, pieces):
    kinds = set()
    for out_b in ru.serve_row_sizes():
        for base_off in range(4):
            for with_replayed in (False, True):
                kinds |= ru.check_serve_against_the_table(check, out_b, base_off, with_replayed, pieces, n=300 if out_b > 17 else 700)
    # every row of the table was met with the leader's amount and with another one
    assert kinds == {(s, same) for s in (0, 255, 6, 7, ru.DOUBLE_SPEND, ru.UNDETERMINED, ru.RECORDED_UNSIGNED) for same in (True, False)}


def test_the_serve_pass_of_the_replay_unique_forms_answers_as_before(check):
    for out_b in (17, 128, 141):
        ru.check_serve_against_the_table(check, out_b, 1, True, False, n=300, plain=True)


def test_the_serve_pass_costs_no_field_operation(check):
    """the figure the documents state beside the measured ratios: byte movement and two scalar loads"""
    before = check.hc_serve_return_field_ops()
    ru.check_serve_against_the_table(check, ru.refund_return_wire_bytes(8), 1, True, False)
    ru.check_serve_against_the_table(check, 160, 0, True, True)
    assert check.hc_serve_return_field_ops() == before == 0
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"copy_serve_return[^.]*\*\*0 field operations per lane\*\*", design), "DESIGN.md section 4.10 does not state the count"


# ---- 3. sanitizers ------------------------------------------------------------------------------------------------------------------------------
def test_the_serve_pass_as_a_sanitized_stand_alone_program(tmp_path):
    """copy_serve_return_check.cpp with its own main under AddressSanitizer and UBSan: exact-size heap arrays (the amounts included),
    the grid's tail lanes, rows and amounts at every base offset"""
    exe = ru.build_program(str(tmp_path / "copy_serve_return_check_asan"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe] + [str(b) for b in ru.serve_row_sizes()], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "COPY SERVE RETURN CHECK CLEAN" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-6000:]


# ---- 4. header, binding, Rust ---------------------------------------------------------------------------------------------------------------------
def test_counts_and_prototypes_in_the_header():
    hd = open(os.path.join(ROOT, "include", "act_mi355x.h")).read()
    assert re.search(r"#define ACT_RETURN_REPLAY_UNIQUE_COUNTS 15\b", hd) and re.search(r"#define ACT_RETURN_REPLAY_COUNTS 12\b", hd)
    from act_amd import capi
    assert tuple(capi.RETURN_REPLAY_UNIQUE_COUNTS) == ru.COUNTS and capi.RETURN_REPLAY_UNIQUE_COUNTS[:12] == capi.RETURN_REPLAY_COUNTS == rr.COUNTS
    assert capi.RETURN_REPLAY_UNIQUE_COUNTS[12:] == ("copies", "copies_served", "copies_other_amount")
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", hd, flags=re.S))
    for new, old in (("act_redeem_return_replay_unique_batch", "act_redeem_return_replay_batch"),
                     ("act_redeem_cbor_return_replay_unique_batch", "act_redeem_cbor_return_replay_batch")):
        assert new in capi.EXPORTS
        params = {name: re.search(r"\bint %s ?\(([^;]*?)\) ?;" % name, flat).group(1) for name in (new, old)}
        assert params[new] == params[old], new          # the same parameters
    for word in ("copies_other_amount", "the receipt pins the leader's amount", "the conservative direction",
                 "NOT OFFERED, on purpose: the replay forms", "Also not offered here: the node-handle forms.", "h1 (e + x)^-1"):
        assert re.sub(r"\s+", " ", word) in re.sub(r"[\s*]+", " ", hd), word
    assert "the engine refuses the combination" not in hd
    # the engine's definitions take the header's parameters in the header's order
    src = open(os.path.join(ROOT, "anonymous-credit-tokens_amd", "csrc", "admit_replay_impl.inc")).read()
    types = lambda params: [re.sub(r"\s*\b\w+(\[\d+\])?$", r"\1", re.sub(r"\bctx\b", "c", p.strip())).replace(" ", "") for p in params.split(",")]
    for name in ("act_redeem_return_replay_unique_batch", "act_redeem_cbor_return_replay_unique_batch"):
        got = re.search(r'extern "C" int %s\(([^)]*)\)' % name, src).group(1)
        want = re.search(r"\bint %s ?\(([^;]*?)\) ?;" % name, flat).group(1)
        assert types(re.sub(r"\s+", " ", got)) == types(want), name
    rs = open(os.path.join(ROOT, "rust", "src", "mi355x.rs")).read()
    assert "fn act_redeem_return_replay_unique_batch(" in rs and "fn act_redeem_cbor_return_replay_unique_batch(" in rs
    assert "pub const ACT_RETURN_REPLAY_UNIQUE_COUNTS: usize = 15;" in rs and "copies_other_amount" in rs


def test_the_python_layer_has_methods_of_its_own_and_the_old_argument_pair_still_raises():
    from act_amd import api
    ring = api.Keyring([api.PrivateKey(bytes(64))])
    for owner in (ring, ring.keys[0]):
        assert callable(owner.redeem_return_replay_unique_batch) and callable(owner.redeem_return_replay_unique_cbor_batch)
    for call in (ring.redeem_replay_batch, ring.redeem_replay_cbor_batch, ring.keys[0].redeem_replay_batch, ring.keys[0].redeem_replay_cbor_batch):
        with pytest.raises(ValueError, match="redeem_return_replay_unique"):
            call(None, None, None, [], bytes(32), unique=True, returned=[])
