"""Admission for the replayable redemption: the model and the builders that tests/test_admit_replay_host.py (lane bodies on the CPU)
and tests/test_gpu_admit_replay.py (the calls on the GPU) share.  Built on admission_cases (the screen's order) and replay_cases (the
tail: replay_cases.model runs over the lanes the screen lets through).

  model           the whole call over labelled lanes: a Python set for `set`, a set of (k, K') for `receipts`
  decide          the decision function of csrc/admit_replay_lanes.h, as the header states it
  kprime          enc(sum_j 2^j Com_j) of a SpendProof record, with oracle/pymodel
  build_check / build_program   tests/hostcheck/admit_replay_check.cpp as a library, and as a stand-alone sanitized program"""
import os
import subprocess
from collections import namedtuple

import pymodel
import replay_cases as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ELL = rp.ELL
KEY_NONE = 255
WRONG_CHARGE, DOUBLE_SPEND = 250, 3
COUNTS = ("lanes", "wire_rejected", "wrong_charge", "foreign_spend", "retry_candidates", "verified", "rejected_by_verification", "fresh", "replayed",
          "double_spend_after", "unanswered")

# k: the nullifier; kprime: the K' the proof commits to (any hashable); verdict / key: what verification says and the ring index it
# matches; s: the charge the proof carries; wire: the wire reader's code for the message (0 = well-shaped); com_ok: every Com_j decodes
Lane = namedtuple("Lane", "k kprime verdict key s wire com_ok", defaults=(0, 0, 0, 0, True))


def decide(pre, spent, undecodable, found):
    """(pre-status, spent, undecodable, found) -> (final pre-status, retry candidate)"""
    if not spent:
        return pre, 0
    if undecodable or not found:
        return DOUBLE_SPEND, 0
    return 0, 1


def model(lanes, spent: set, receipts: set, charges=None):
    """the call in lane order; mutates `spent` and `receipts` as the tail does -> (statuses, out_key, replayed, counts)"""
    before, had = frozenset(spent), frozenset(receipts)
    n = len(lanes)
    st, ok, rep = [None] * n, [KEY_NONE] * n, [0] * n
    c = dict.fromkeys(COUNTS, 0)
    c["lanes"] = n
    go = []
    for i, ln in enumerate(lanes):
        if ln.wire:                                                    # 1. the message fails structurally
            st[i] = ln.wire; c["wire_rejected"] += 1; continue
        if charges is not None and ln.s % ELL != charges[i] % ELL:     # 2. not the expected charge
            st[i] = WRONG_CHARGE; c["wrong_charge"] += 1; continue
        if ln.k in before:                                             # 3. spent when the call looks it up: ask the receipts
            pre, cand = decide(DOUBLE_SPEND, True, not ln.com_ok, (ln.k, ln.kprime) in had)
            if pre:
                st[i] = pre; c["foreign_spend"] += 1; continue
            c["retry_candidates"] += cand
        go.append(i)
    c["verified"] = len(go)                                            # 4. the replay call over what is left
    mst, mok, mrep, mc = rp.model([rp.Lane(lanes[i].k, lanes[i].kprime, lanes[i].verdict, lanes[i].key) for i in go], spent, receipts)
    for j, i in enumerate(go):
        st[i], ok[i], rep[i] = mst[j], mok[j], mrep[j]
    c.update(rejected_by_verification=mc["rejected_by_verification"], fresh=mc["fresh"], replayed=mc["replayed"], double_spend_after=mc["double_spend"],
             unanswered=mc["unanswered"])
    return st, ok, rep, c


# ---- the fixed mix, hand-written ------------------------------------------------------------------------------------------------------------
# tokens "sp*" were redeemed before the call with K' "A" (so `receipts` holds (sp*, "A")); every proof spends 2, a wrong-charge lane is asked 3
FIXED_MIX = [
    # name                                          lane                                   charge  status  key   replayed
    ("fresh",                                       Lane("t0", "A", 0, 0, 2),               2,      0,      0,    0),
    ("in-batch retry",                              Lane("t0", "A", 0, 0, 2),               2,      0,      0,    1),
    ("pre-spent retry",                             Lane("sp0", "A", 0, 1, 2),              2,      0,      1,    1),
    ("pre-spent, foreign K'",                       Lane("sp1", "B", 0, 0, 2),              2,      3,      255,  0),
    ("foreign and tampered",                        Lane("sp2", "B", 7, 255, 2),            2,      3,      255,  0),
    ("retry tampered outside k / Com",              Lane("sp3", "A", 7, 255, 2),            2,      7,      255,  0),
    ("spent, a Com_j that is no point",             Lane("sp4", "A", 255, 255, 2, 0, False), 2,     3,      255,  0),
    ("wrong charge on a spent lane",                Lane("sp0", "A", 0, 1, 2),              3,      250,    255,  0),
    ("fresh, other K' of an in-batch nullifier",    Lane("t0", "B", 0, 0, 2),               2,      3,      0,    0),
]
FIXED_SPENT = ("sp0", "sp1", "sp2", "sp3", "sp4")
FIXED_COUNTS = dict(lanes=9, wire_rejected=0, wrong_charge=1, foreign_spend=3, retry_candidates=2, verified=5, rejected_by_verification=1, fresh=1, replayed=2,
                    double_spend_after=1, unanswered=0)


def check_model():
    lanes, charges = [m[1] for m in FIXED_MIX], [m[2] for m in FIXED_MIX]
    spent, receipts = set(FIXED_SPENT), {(k, "A") for k in FIXED_SPENT}
    st, ok, rep, c = model(lanes, spent, receipts, charges)
    assert (st, ok, rep) == ([m[3] for m in FIXED_MIX], [m[4] for m in FIXED_MIX], [m[5] for m in FIXED_MIX]), (st, ok, rep)
    assert c == FIXED_COUNTS, c
    assert c["verified"] == c["lanes"] - c["wire_rejected"] - c["wrong_charge"] - c["foreign_spend"]
    assert spent == set(FIXED_SPENT) | {"t0"} and receipts == {(k, "A") for k in FIXED_SPENT} | {("t0", "A")}
    # with charge == NULL the accepted lanes, their keys and marks and both sets are the replay call's; only doubly bad lanes differ
    spent2, rec2 = set(FIXED_SPENT), {(k, "A") for k in FIXED_SPENT}
    spent3, rec3 = set(FIXED_SPENT), {(k, "A") for k in FIXED_SPENT}
    a = model(lanes, spent2, rec2, None)
    b = rp.model([rp.Lane(ln.k, ln.kprime, ln.verdict, ln.key) for ln in lanes], spent3, rec3)
    assert (spent2, rec2) == (spent3, rec3)
    differ = [i for i in range(len(lanes)) if (a[0][i], a[1][i], a[2][i]) != (b[0][i], b[1][i], b[2][i])]
    assert differ == [3, 4, 6] and [a[0][i] for i in differ] == [3, 3, 3] and [b[0][i] for i in differ] == [3, 7, 255]      # (lane 3: out_key only)
    assert a[0][7] == 0 and a[2][7] == 1                              # without the charge the wrong-charge lane is a retry


# ---- K' with the reference model -------------------------------------------------------------------------------------------------------------
def com_span(rec: bytes, L: int):
    return [rec[32 * (4 + j):32 * (5 + j)] for j in range(L)]


def kprime(rec: bytes, L: int):
    """enc(sum_j 2^j Com_j), or None where a Com_j is no canonical Ristretto encoding"""
    pts = [pymodel.ristretto_decode(b) for b in com_span(rec, L)]
    if any(p is None for p in pts):
        return None
    acc = pymodel.IDENTITY
    for p in reversed(pts):
        acc = pymodel.pt_add(pymodel.pt_double(acc), p)
    return pymodel.ristretto_encode(acc)


# ---- the host build of the lane bodies ------------------------------------------------------------------------------------------------------
def _build(out, extra):
    csrc = os.path.join(ROOT, "anonymous-credit-tokens_amd", "csrc")
    src = os.path.join(ROOT, "tests", "hostcheck", "admit_replay_check.cpp")
    deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".h", ".inc"))]
    if os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in deps):
        return out
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-Wno-psabi", *extra, "-o", out, src], check=True)
    return out


def build_check(out):
    """csrc/admit_replay_lanes.h compiled with g++ into a small library"""
    return _build(out, ["-O2", "-fPIC", "-shared"])


def build_program(out):
    """the same file with its own main, under AddressSanitizer and UBSan: a stand-alone program with the sanitizers' runtimes linked in,
    so that nothing has to be preloaded"""
    return _build(out, ["-O1", "-g", "-DADMIT_REPLAY_CHECK_MAIN", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer"])
