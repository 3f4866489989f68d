"""Admission for the replayable redemption on the CPU: the lane bodies of k_admit_replay.hip (csrc/admit_replay_lanes.h) compiled for the
host by tests/hostcheck/admit_replay_check.cpp -- Com_j -> Niels, Horner -> enc(K') -> tag, the decision, the key of the spent lanes'
compaction -- against oracle/pymodel, the verification lane bodies' own K' and the model of tests/admit_replay_cases.py.  The same
bodies run on the GPU in tests/test_gpu_admit_replay.py."""
import ctypes as C
import itertools
import os
import re
import subprocess

import pytest

import admission_cases as ad
import admit_replay_cases as ar
import pymodel
import replay_cases as rp
from conftest import ROOT, load_golden, shake
from test_spend_lanes_host import host_verify

# DESIGN.md section 4.9 quotes the screen's field multiplications + squarings per spent lane at L = 128 in these words
DESIGN_OPS = re.compile(r"\*\*([\d ]+) field operations per spent lane at L = 128\*\*")


@pytest.fixture(scope="module")
def arc():
    lib = C.CDLL(ar.build_check(os.path.join(ROOT, "tests", "hostcheck", "libadmit_replay_check.so")))
    lib.hc_ar_kprime.argtypes = [C.c_int, C.c_uint32, C.c_char_p, C.c_char_p, C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_void_p]
    return lib


def screen(arc, L, recs, kred, idx=None):
    """-> (enc(K') per candidate, tags, marks, (decode mul, decode sq, tag mul, tag sq))"""
    pb = 32 * (14 + 4 * L)
    n = len(recs) // pb
    kp, tag, mark = C.create_string_buffer(32 * n), C.create_string_buffer(32 * n), C.create_string_buffer(n)
    counts = (C.c_uint64 * 4)()
    ix = (C.c_uint32 * n)(*idx) if idx is not None else None
    assert arc.hc_ar_kprime(L, n, recs, kred, ix, kp, tag, mark, counts) == 1
    return kp.raw, tag.raw, mark.raw, tuple(counts)


def model_records(L, n, label):
    """records of the model: Com_j = r_j * B for scalars of the label, every other field bytes of the label"""
    pb = 32 * (14 + 4 * L)
    recs = bytearray(shake(label, pb * n))
    for c in range(n):
        for j in range(L):
            r = int.from_bytes(shake("%s-%d-%d" % (label, c, j), 32), "little") % pymodel.ELL
            recs[c * pb + 32 * (4 + j):c * pb + 32 * (5 + j)] = pymodel.ristretto_encode(pymodel.pt_mul(pymodel.BASEPOINT, r))
    return bytes(recs)


def test_the_model_against_hand_written_lanes():
    ar.check_model()


def test_kprime_and_tag_on_the_lifecycle_proofs(arc, hostcheck):
    g = load_golden("lifecycle_L128.json")
    L, cases = g["L"], [c for c in g["cases"] if c["status"] == 0]
    assert L == 128 and len(cases) >= 3
    recs = b"".join(bytes.fromhex(c["proof"]) for c in cases)
    pb, n = 32 * (14 + 4 * L), len(cases)
    kred = b"".join(rp.reduced(recs[pb * i:pb * i + 32]) for i in range(n))
    kp, tag, mark, _ = screen(arc, L, recs, kred)
    assert mark == bytes(n)
    st, vkp, _, _ = host_verify(hostcheck, bytes.fromhex(g["params"]), L, bytes.fromhex(g["sk"]), recs)
    assert st == bytes(n) and kp == vkp                              # the bytes k_spend_tail's lane body produces for the same proofs
    for i, c in enumerate(cases):
        rec = recs[pb * i:pb * i + pb]
        assert kp[32 * i:32 * i + 32] == ar.kprime(rec, L) == bytes.fromhex(c["kprime"]), i
        assert tag[32 * i:32 * i + 32] == rp.tag(rec[:32], kp[32 * i:32 * i + 32]), i
    # the nullifiers through an index, as the engine passes the screen's array and the spent lanes' numbers
    spread = b"".join(shake("pad%d" % i, 32) + kred[32 * i:32 * i + 32] for i in range(n))
    assert screen(arc, L, recs, spread, [2 * i + 1 for i in range(n)])[:3] == (kp, tag, mark)


@pytest.mark.parametrize("L,n", [(3, 5), (8, 67)])
def test_kprime_on_records_of_the_model_and_an_undecodable_com(arc, L, n):
    pb = 32 * (14 + 4 * L)
    recs = bytearray(model_records(L, n, "arc-L%d" % L))
    bad = n // 2
    recs[bad * pb + 32 * (4 + L - 1):bad * pb + 32 * (5 + L - 1)] = b"\xff" * 32
    recs = bytes(recs)
    kred = b"".join(rp.reduced(recs[pb * i:pb * i + 32]) for i in range(n))
    kp, tag, mark, _ = screen(arc, L, recs, kred)
    for i in range(n):
        rec = recs[pb * i:pb * i + pb]
        if i == bad:
            assert ar.kprime(rec, L) is None and (mark[i], kp[32 * i:32 * i + 32], tag[32 * i:32 * i + 32]) == (1, bytes(32), bytes(32))
            continue
        assert mark[i] == 0 and kp[32 * i:32 * i + 32] == ar.kprime(rec, L), i
        assert tag[32 * i:32 * i + 32] == rp.tag(rec[:32], kp[32 * i:32 * i + 32]), i


def test_the_decision_over_its_whole_domain(arc):
    out = C.create_string_buffer(2)
    for pre, spent, bad, found in itertools.product(range(256), (0, 1), (0, 1), (0, 1)):
        arc.hc_ar_decide(pre, spent, bad, found, out)
        assert tuple(out.raw) == ar.decide(pre, spent, bad, found), (pre, spent, bad, found)
    # a lane that is not spent is never touched; a spent lane never becomes anything but 0 (goes on to verification) or 3
    assert all(ar.decide(3, 1, b, f)[0] in (0, 3) for b in (0, 1) for f in (0, 1)) and ar.decide(3, 1, 0, 1) == (0, 1)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257])
def test_compaction_over_the_spent_lanes_and_the_decision_per_lane(arc, n):
    ac = C.CDLL(ad.build_admit_check(os.path.join(ROOT, "tests", "hostcheck", "libadmit_check.so")))
    for pat in ("all", "none", "mixed"):
        pre = bytes(3 if pat == "all" else 0 if pat == "none" else (3, 0, 250, 3, 254, 0, 3)[(i * i + i // 5) % 7] for i in range(n))
        key = C.create_string_buffer(n)
        arc.hc_ar_key_lanes(n, pre, key)
        assert key.raw == bytes(0 if p == 3 else 1 for p in pre)
        total, idx, pos = ad.host_compact(ac, key.raw)
        want = [i for i in range(n) if pre[i] == 3]
        assert total == len(want) and idx == want                   # stable: the spent lanes in lane order
        assert pos == [want.index(i) if pre[i] == 3 else 0xFFFFFFFF for i in range(n)]
        mark = bytes(1 if c % 5 == 4 else 0 for c in range(total)); found = bytes(1 if c % 2 == 0 else 0 for c in range(total))
        out = C.create_string_buffer(pre, n)
        arc.hc_ar_decide_lanes(n, (C.c_uint32 * n)(*pos), mark, found, out)
        for i in range(n):
            c = pos[i]
            assert out.raw[i] == (pre[i] if pre[i] != 3 else ar.decide(3, 1, mark[c], found[c])[0]), (n, pat, i)


def test_the_screens_cost_is_the_figure_in_the_design(arc):
    """field multiplications + squarings of the screen per spent lane at L = 128, counted by the host build; DESIGN 4.9 states the
    figure and its ratio to a verification's 485 560 (tests/test_keyring_host.py counts those the same way)"""
    g = load_golden("lifecycle_L128.json")
    rec = bytes.fromhex(next(c for c in g["cases"] if c["status"] == 0)["proof"])
    _, _, mark, (dm, ds, tm, ts) = screen(arc, 128, rec, rp.reduced(rec[:32]))
    total = dm + ds + tm + ts
    print("screen at L = 128: decode %d mul + %d sq, tag %d mul + %d sq = %d field operations; %.4f of 485 560" % (dm, ds, tm, ts, total, total / 485560))
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    m = DESIGN_OPS.search(design)
    assert m, "DESIGN.md section 4.9 does not state the count"
    assert int(m.group(1).replace(" ", "")) == total
    assert mark == b"\0" and (dm + ds) > 10 * (tm + ts)             # the decode is the bulk of the stage


def test_defines_and_bindings():
    hd = open(os.path.join(ROOT, "include", "act_mi355x.h")).read()
    assert re.search(r"#define ACT_ADMIT_REPLAY_COUNTS 11\b", hd)
    from act_amd import capi
    assert tuple(capi.ADMIT_REPLAY_COUNTS) == ar.COUNTS and len(ar.COUNTS) == 11
    for name in ("act_redeem_admit_replay_batch", "act_redeem_cbor_admit_replay_batch"):
        assert name in capi.EXPORTS and re.search(r"\bint %s\(" % name, hd)
    for word in ("foreign_spend", "retry_candidates", "double_spend_after", "unanswered"):
        assert word in hd


def test_lane_bodies_as_a_sanitized_stand_alone_program(tmp_path):
    """admit_replay_check.cpp with its own main under AddressSanitizer and UBSan: exact-size heap arrays, the grid's tail lanes, L = 3, 8
    and 128, an undecodable Com_j, K' against 2^j Com_j summed by another road, the decision over its whole domain"""
    exe = ar.build_program(str(tmp_path / "admit_replay_check_asan"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "ADMIT REPLAY CHECK CLEAN" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-6000:]
