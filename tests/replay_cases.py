"""Replayable redemption: the definitions and the model that tests/test_replay_host.py (lane bodies on the CPU) and
tests/test_gpu_replay.py (the calls on the GPU) share.

  tag / nonce     the two hashes of include/act_mi355x.h ("replayable redemption"), recomputed with oracle/pymodel.blake3
  model           the whole call over labelled lanes: a Python set for `set`, a set of (k, K') for `receipts`
  build_replay_check / build_replay_program   tests/hostcheck/replay_check.cpp as a library, and as a stand-alone sanitized program"""
import os
import subprocess

import pymodel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ELL = 2**252 + 27742317777372353535851937790883648493
KEY_NONE = 255
DOUBLE_SPEND, UNDETERMINED, RECORDED_UNSIGNED = 3, 252, 251

LABEL_TAG = b"act-mi355x/receipt/v1".ljust(32, b"\0")
LABEL_NONCE = b"act-mi355x/refund-nonce/v1".ljust(32, b"\0")
COUNTS = ("lanes", "rejected_by_verification", "fresh", "replayed", "double_spend", "unanswered")


def reduced(k: bytes) -> bytes:
    return (int.from_bytes(k, "little") % ELL).to_bytes(32, "little")


def tag(k: bytes, kprime: bytes) -> bytes:
    """the receipt of nullifier k (32 bytes as on the wire, reduced here) spent for enc(K')"""
    assert len(k) == 32 and len(kprime) == 32
    t = bytearray(pymodel.blake3(LABEL_TAG + reduced(k) + kprime, 32))
    t[31] &= 0x0F
    return bytes(t)


def nonce(nonce_key: bytes, key: bytes, k: bytes, kprime: bytes) -> bytes:
    """the 128 nonce bytes of a lane signed with the 64-byte key record `key`"""
    assert len(nonce_key) == 32 and len(key) == 64 and len(k) == 32 and len(kprime) == 32
    return pymodel.blake3(LABEL_NONCE + nonce_key + key + reduced(k) + kprime, 128)


# ---- the whole call ---------------------------------------------------------------------------------------------------------------------
class Lane:
    """what a lane IS: its nullifier (an int, reduced), the K' it commits to (any hashable), the verification's verdict and matched key"""

    def __init__(self, k, kprime, verdict=0, key=0):
        self.k, self.kprime, self.verdict, self.key = k, kprime, verdict, key


def model(lanes, spent: set, receipts: set):
    """the replay calls in lane order; mutates `spent` (nullifiers) and `receipts` ((k, K') pairs)
    -> (statuses, out_key, replayed, counts)"""
    st, ok, rep = [], [], []
    for ln in lanes:
        if ln.verdict:
            st.append(ln.verdict); ok.append(KEY_NONE); rep.append(0)
            continue
        ok.append(ln.key)
        if ln.k not in spent:
            spent.add(ln.k); receipts.add((ln.k, ln.kprime))        # a receipt ONLY where k was fresh
            st.append(0); rep.append(0)
        elif (ln.k, ln.kprime) in receipts:
            st.append(0); rep.append(1)
        else:
            st.append(DOUBLE_SPEND); rep.append(0)
    return st, ok, rep, counts_of(st, rep)


def counts_of(st, rep):
    c = dict.fromkeys(COUNTS, 0)
    c["lanes"] = len(st)
    for s, r in zip(st, rep):
        if s == 0:
            c["replayed" if r else "fresh"] += 1
        elif s == DOUBLE_SPEND:
            c["double_spend"] += 1
        elif s in (UNDETERMINED, RECORDED_UNSIGNED):
            c["unanswered"] += 1
        else:
            c["rejected_by_verification"] += 1
    return c


def check_model():
    """the model against hand-written expectations: [P, P, P' (same k, other K'), tampered P, undecodable], then the batch again"""
    spent, receipts = set(), set()
    lanes = [Lane(5, "A"), Lane(5, "A"), Lane(5, "B"), Lane(5, "A", 7), Lane(6, "C", 255)]
    st, ok, rep, c = model(lanes, spent, receipts)
    assert (st, ok, rep) == ([0, 0, 3, 7, 255], [0, 0, 0, 255, 255], [0, 1, 0, 0, 0])
    assert c == dict(lanes=5, rejected_by_verification=2, fresh=1, replayed=1, double_spend=1, unanswered=0)
    assert spent == {5} and receipts == {(5, "A")}
    st, ok, rep, c = model(lanes, spent, receipts)
    assert (st, rep) == ([0, 0, 3, 7, 255], [1, 1, 0, 0, 0]) and c["fresh"] == 0 and c["replayed"] == 2
    assert spent == {5} and receipts == {(5, "A")}                  # a double spender plants nothing
    st, ok, rep, c = model([Lane(5, "B")], spent, receipts)
    assert st == [3] and receipts == {(5, "A")}


# ---- the host build of the lane bodies ------------------------------------------------------------------------------------------------------
def _build(out, extra):
    csrc = os.path.join(ROOT, "anonymous-credit-tokens_amd", "csrc")
    src = os.path.join(ROOT, "tests", "hostcheck", "replay_check.cpp")
    deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".h", ".inc"))]
    if os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in deps):
        return out
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-Wno-psabi", *extra, "-o", out, src], check=True)
    return out


def build_replay_check(out):
    """csrc/replay_lanes.h compiled with g++ into a small library"""
    return _build(out, ["-O2", "-fPIC", "-shared"])


def build_replay_program(out):
    """the same file with its own main, under AddressSanitizer and UBSan: a stand-alone program with the sanitizers'
    runtimes linked in, so that nothing has to be preloaded"""
    return _build(out, ["-O1", "-g", "-DREPLAY_CHECK_MAIN", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer"])
