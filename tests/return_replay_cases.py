"""Replayable partial refunds ("the receipt pins t"): the definitions and the model that tests/test_return_replay_host.py
(lane bodies on the CPU) and tests/test_gpu_return_replay.py (the calls on the GPU) share.  Built on replay_cases (the v1 hashes),
admit_replay_cases (the screen's order) and refund_return_cases (t > s).

  tag_t / nonce_t   the two hashes of include/act_mi355x.h ("replayable partial refunds") for t^ != 0, with oracle/pymodel.blake3
  tag / nonce       the choice a lane makes: the v1 hash of replay_cases for t^ == 0, the _t hash otherwise
  model             the whole call over labelled lanes: a Python set for `set`, a set of (k, K', t^) for `receipts`
  build_check / build_program   tests/hostcheck/return_replay_check.cpp as a library, and as a stand-alone sanitized program"""
import os
import subprocess

import pymodel
import admit_replay_cases as ar
import replay_cases as rp

ROOT = rp.ROOT
ELL = rp.ELL
KEY_NONE = 255
WRONG_CHARGE, RETURN_TOO_BIG, DOUBLE_SPEND = 250, 249, 3
COUNTS = ar.COUNTS + ("return_too_big",)

LABEL_TAG_T = b"act-mi355x/receipt-t/v1".ljust(32, b"\0")
LABEL_NONCE_T = b"act-mi355x/refund-nonce-t/v1".ljust(32, b"\0")


def that(t) -> int:
    """t^ = t mod l, of an int or of 32 little-endian bytes"""
    return (int.from_bytes(t, "little") if isinstance(t, (bytes, bytearray)) else t) % ELL


def tag_t(k: bytes, kprime: bytes, t) -> bytes:
    msg = LABEL_TAG_T + rp.reduced(k) + kprime + that(t).to_bytes(32, "little")
    assert len(msg) == 128
    out = bytearray(pymodel.blake3(msg, 32))
    out[31] &= 0x0F
    return bytes(out)


def nonce_t(nonce_key: bytes, key: bytes, k: bytes, kprime: bytes, t) -> bytes:
    msg = LABEL_NONCE_T + nonce_key + key + rp.reduced(k) + kprime + that(t).to_bytes(32, "little")
    assert len(msg) == 224
    return pymodel.blake3(msg, 128)


def tag(k: bytes, kprime: bytes, t=0) -> bytes:
    return rp.tag(k, kprime) if that(t) == 0 else tag_t(k, kprime, t)


def nonce(nonce_key: bytes, key: bytes, k: bytes, kprime: bytes, t=0) -> bytes:
    return rp.nonce(nonce_key, key, k, kprime) if that(t) == 0 else nonce_t(nonce_key, key, k, kprime, t)


# ---- the whole call ---------------------------------------------------------------------------------------------------------------------
def model(lanes, spent: set, receipts: set, charges=None, returned=None):
    """admit_replay_cases.model with the amounts: `lanes` are ar.Lane, `receipts` holds (k, K', t^), returned[i] is an int (None: all
    zero).  The bound t^ <= s^ stands behind the charge rule and in front of both look-ups.  Mutates `spent` and `receipts`
    -> (statuses, out_key, replayed, counts)"""
    n = len(lanes)
    ts = [0] * n if returned is None else [that(t) for t in returned]
    st, ok, rep = [None] * n, [KEY_NONE] * n, [0] * n
    c = dict.fromkeys(COUNTS, 0)
    c["lanes"] = n
    # K' and t^ together are what a receipt is for: the calls without amounts run over lanes whose K' label carries the amount
    pinned = [ln._replace(kprime=(ln.kprime, ts[i])) for i, ln in enumerate(lanes)]
    shed = set()
    for i, ln in enumerate(lanes):
        if ln.wire:
            continue
        if charges is not None and ln.s % ELL != charges[i] % ELL:
            continue
        if ts[i] > ln.s % ELL:
            st[i] = RETURN_TOO_BIG; c["return_too_big"] += 1; shed.add(i)
    keep = [i for i in range(n) if i not in shed]
    inner_receipts = {(k, (kp, t)) for k, kp, t in receipts}
    mst, mok, mrep, mc = ar.model([pinned[i] for i in keep], spent, inner_receipts, None if charges is None else [charges[i] for i in keep])
    receipts.clear(); receipts.update((k, kp, t) for k, (kp, t) in inner_receipts)
    for j, i in enumerate(keep):
        st[i], ok[i], rep[i] = mst[j], mok[j], mrep[j]
    for name in ar.COUNTS:
        if name != "lanes":
            c[name] = mc[name]
    assert c["verified"] == c["lanes"] - c["wire_rejected"] - c["wrong_charge"] - c["return_too_big"] - c["foreign_spend"]
    return st, ok, rep, c


def check_model():
    """hand-written: [P t=5, P t=5, P t=6, P' t=5, P t=s+1], then the batch again.  P and P' share the nullifier; s = 7."""
    s = 7
    P, Q = ar.Lane(5, "A", 0, 0, s), ar.Lane(5, "B", 0, 1, s)
    lanes, returned = [P, P, P, Q, P], [5, 5, 6, 5, s + 1]
    spent, receipts = set(), set()
    st, ok, rep, c = model(lanes, spent, receipts, [s] * 5, returned)
    assert (st, ok, rep) == ([0, 0, 3, 3, 249], [0, 0, 0, 1, 255], [0, 1, 0, 0, 0]), (st, ok, rep)
    assert c == dict(lanes=5, wire_rejected=0, wrong_charge=0, foreign_spend=0, retry_candidates=0, verified=4, rejected_by_verification=0, fresh=1, replayed=1,
                     double_spend_after=2, unanswered=0, return_too_big=1), c
    assert spent == {5} and receipts == {(5, "A", 5)}                 # neither the other amount nor the other K' planted anything
    # again: the nullifier is spent when the call looks, so the screen decides -- the other amount and the other K' are shed unverified
    st, ok, rep, c = model(lanes, spent, receipts, [s] * 5, returned)
    assert (st, ok, rep) == ([0, 0, 3, 3, 249], [0, 0, 255, 255, 255], [1, 1, 0, 0, 0]), (st, ok, rep)
    assert c == dict(lanes=5, wire_rejected=0, wrong_charge=0, foreign_spend=2, retry_candidates=2, verified=2, rejected_by_verification=0, fresh=0, replayed=2,
                     double_spend_after=0, unanswered=0, return_too_big=1), c
    assert spent == {5} and receipts == {(5, "A", 5)}
    # t + l names the same amount; a wrong charge goes in front of the bound; nothing returned is the call without amounts
    assert model([P], spent, receipts, [s], [5 + ELL])[:3] == ([0], [0], [1])
    assert model([P], spent, receipts, [s + 1], [s + 1])[0] == [250]
    assert model([P], spent, receipts, None, None)[0] == [3] and model([P], spent, receipts, None, [0])[0] == [3]
    a = model([ar.Lane(9, "C", 0, 0, s)], set(), set(), None, None)
    b = ar.model([ar.Lane(9, "C", 0, 0, s)], set(), set(), None)
    assert a[:3] == b[:3] and {k: v for k, v in a[3].items() if k != "return_too_big"} == b[3]
    # the hashes: zero (also as l, and as None) is v1, everything else is not, and t and t + l are one amount
    k, kp, nk, key = bytes(range(32)), bytes(range(32, 64)), bytes(range(64, 96)), bytes(range(96, 160))
    assert tag(k, kp, 0) == tag(k, kp, ELL) == rp.tag(k, kp) and nonce(nk, key, k, kp, ELL) == rp.nonce(nk, key, k, kp)
    assert tag(k, kp, 1) == tag(k, kp, 1 + ELL) == tag_t(k, kp, 1) != rp.tag(k, kp) and tag(k, kp, 1)[31] & 0xF0 == 0
    assert nonce(nk, key, k, kp, 2) == nonce_t(nk, key, k, kp, (2 + ELL).to_bytes(32, "little")) != rp.nonce(nk, key, k, kp)
    assert len({tag(k, kp, t) for t in (0, 1, 2, s)}) == 4 and len({nonce(nk, key, k, kp, t)[:32] for t in (0, 1, 2, s)}) == 4


# ---- the host build of the lane bodies ------------------------------------------------------------------------------------------------------
def _build(out, extra):
    csrc = os.path.join(ROOT, "anonymous-credit-tokens_amd", "csrc")
    src = os.path.join(ROOT, "tests", "hostcheck", "return_replay_check.cpp")
    deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".h", ".inc"))]
    if os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in deps):
        return out
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-Wno-psabi", *extra, "-o", out, src], check=True)
    return out


def build_check(out):
    """csrc/return_replay_lanes.h compiled with g++ into a small library"""
    return _build(out, ["-O2", "-fPIC", "-shared"])


def build_program(out):
    """the same file with its own main, under AddressSanitizer and UBSan: a stand-alone program with the sanitizers' runtimes linked in,
    so that nothing has to be preloaded"""
    return _build(out, ["-O1", "-g", "-DRETURN_REPLAY_CHECK_MAIN", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer"])
