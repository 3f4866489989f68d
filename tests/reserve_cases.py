"""Reserve and settle: the definitions and the model that tests/test_reserve_host.py (lane bodies on the CPU) and
tests/test_gpu_reserve.py / tests/test_gpu_settle.py (the calls on the GPU) share.  Built on admit_replay_cases (the screen's order and
the replay tail) and return_replay_cases (the amount tag and the derived nonces, reused as they are).

  tag_res / marker   the two hashes of include/act_mi355x.h ("reserve and settle"), with oracle/pymodel.blake3
  record / prep      the 96-byte reservation record; settle's per-lane pass over one (rules 1 and 2, the three tags), on bytes
  reserve            act_redeem_(cbor_)reserve_batch over labelled lanes: a Python set for `set`, a set of tuples for `receipts`
  settle             act_redeem_(cbor_)settle_batch over reservation tuples and the same receipts
  build_program      tests/hostcheck/reserve_check.cpp as a stand-alone program, plain or sanitized

The receipts hold three kinds of key: ("res", k, K', s^), ("mark", k, K') and ("amt", k, K', t^) -- the last is what
return_replay_cases.model keeps as (k, K', t^)."""
import os
import subprocess

import pymodel
import admit_replay_cases as ar
import replay_cases as rp
import return_replay_cases as rr

ROOT = rp.ROOT
ELL = rp.ELL
KEY_NONE = 255
DOUBLE_SPEND, RETURN_TOO_BIG, NOT_RESERVED, SETTLED_OTHER_AMOUNT = 3, 249, 248, 247
RESERVE_COUNTS = ar.COUNTS
SETTLE_COUNTS = ("lanes", "not_reserved", "return_too_big", "settled", "settled_again", "other_amount", "unanswered")

LABEL_RES = b"act-mi355x/reservation/v1".ljust(32, b"\0")
LABEL_SETTLED = b"act-mi355x/settled/v1".ljust(32, b"\0")

that = rr.that
tag = rr.tag          # the amount tag and the nonces are the replayable partial refunds' own
nonce = rr.nonce


def le(v: int) -> bytes:
    return v.to_bytes(32, "little")


def tag_res(k: bytes, kprime: bytes, s) -> bytes:
    msg = LABEL_RES + rp.reduced(k) + kprime + le(that(s))
    assert len(msg) == 128
    out = bytearray(pymodel.blake3(msg, 32))
    out[31] &= 0x0F
    return bytes(out)


def marker(k: bytes, kprime: bytes) -> bytes:
    msg = LABEL_SETTLED + rp.reduced(k) + kprime
    assert len(msg) == 96
    out = bytearray(pymodel.blake3(msg, 32))
    out[31] &= 0x0F
    return bytes(out)


def record(k: bytes, kprime: bytes, s) -> bytes:
    """k^ | enc(K') | s^"""
    return rp.reduced(k) + kprime + le(that(s))


def prep(rec: bytes, key_index: int, t, nkeys: int):
    """settle's pass over one record -> (status, tag_res, marker, amount tag); zero tags where the status is not 0"""
    k, kp, s = rec[:32], rec[32:64], rec[64:96]
    z = bytes(32)
    if key_index >= nkeys:
        return NOT_RESERVED, z, z, z
    if that(t) > that(s):
        return RETURN_TOO_BIG, z, z, z
    return 0, tag_res(k, kp, s), marker(k, kp), tag(k, kp, t)


# ---- the two calls over labelled lanes ------------------------------------------------------------------------------------------------------
def reserve(lanes, spent: set, receipts: set, charges=None):
    """act_redeem_(cbor_)reserve_batch: admit_replay_cases.model with the reservation where the receipt is -- `lanes` are ar.Lane, the
    receipts hold tuples (see the module's docstring).  Mutates `spent` and `receipts`
    -> (statuses, out_key, replayed, counts, records: (k, K', s^) for an accepted lane, None for every other)"""
    inner = {(e[1], ("res", e[2], e[3])) for e in receipts if e[0] == "res"}
    labelled = [ln._replace(kprime=("res", ln.kprime, ln.s % ELL)) for ln in lanes]
    st, ok, rep, c = ar.model(labelled, spent, inner, charges)
    receipts.update(("res", k, kp, s) for k, (_, kp, s) in inner)
    recs = [(ln.k, ln.kprime, ln.s % ELL) if st[i] == 0 else None for i, ln in enumerate(lanes)]
    return st, ok, rep, c, recs


def settle(reservations, key_index, amounts, receipts: set, nkeys: int):
    """act_redeem_(cbor_)settle_batch in lane order: reservations[i] = (k, K', s^) as reserve handed it out (or altered), amounts[i] an
    int (None: all zero).  Mutates `receipts` -> (statuses, settled_before, counts)"""
    n = len(reservations)
    ts = [0] * n if amounts is None else [that(t) for t in amounts]
    st, before = [None] * n, [0] * n
    c = dict.fromkeys(SETTLE_COUNTS, 0)
    c["lanes"] = n
    had = frozenset(receipts)
    for i, (k, kp, s) in enumerate(reservations):
        if key_index[i] >= nkeys:                                      # 1. the key index
            st[i] = NOT_RESERVED; c["not_reserved"] += 1; continue
        if ts[i] > s % ELL:                                            # 2. the amount against the record's own s
            st[i] = RETURN_TOO_BIG; c["return_too_big"] += 1; continue
        if ("res", k, kp, s % ELL) not in had:                         # 3. the reservation, as the receipts were when the call looked
            st[i] = NOT_RESERVED; c["not_reserved"] += 1; continue
        if ("mark", k, kp) not in receipts:                            # 4. the pin
            receipts.add(("mark", k, kp)); receipts.add(("amt", k, kp, ts[i]))
            st[i] = 0; c["settled"] += 1
        elif ("amt", k, kp, ts[i]) in receipts:
            st[i], before[i] = 0, 1; c["settled_again"] += 1
        else:
            st[i] = SETTLED_OTHER_AMOUNT; c["other_amount"] += 1
    return st, before, c


def check_model():
    """hand-written: reserve [P, P, Q, wrong charge], settle [R 5, R 5, R 6, altered, too big, bad index], then what the one-phase call sees"""
    s = 7
    P, Q, W = ar.Lane(5, "A", 0, 1, s), ar.Lane(5, "B", 0, 0, s), ar.Lane(6, "C", 0, 0, s)
    spent, receipts = set(), set()
    st, ok, rep, c, recs = reserve([P, P, Q, W], spent, receipts, [s, s, s, s + 1])
    assert (st, ok, rep) == ([0, 0, 3, 250], [1, 1, 0, 255], [0, 1, 0, 0]), (st, ok, rep)
    assert recs == [(5, "A", s), (5, "A", s), None, None]
    assert spent == {5} and receipts == {("res", 5, "A", s)}
    assert c == dict(lanes=4, wire_rejected=0, wrong_charge=1, foreign_spend=0, retry_candidates=0, verified=3, rejected_by_verification=0, fresh=1, replayed=1,
                     double_spend_after=1, unanswered=0), c
    # again: a retry candidate at the screen, the other K' shed unverified, the sets as they were
    st, ok, rep, c, recs = reserve([P, Q], spent, receipts, None)
    assert (st, ok, rep) == ([0, 3], [1, 255], [1, 0]) and c["retry_candidates"] == 1 and c["foreign_spend"] == 1 and c["verified"] == 1
    assert spent == {5} and receipts == {("res", 5, "A", s)}
    R = (5, "A", s)
    st, before, c = settle([R, R, R, (5, "A", s - 1), R, R], [1, 1, 1, 1, 1, 2], [5, 5 + ELL, 6, 5, s + 1, 5], receipts, 2)
    assert (st, before) == ([0, 0, 247, 248, 249, 248], [0, 1, 0, 0, 0, 0]), (st, before)
    assert c == dict(lanes=6, not_reserved=2, return_too_big=1, settled=1, settled_again=1, other_amount=1, unanswered=0), c
    assert receipts == {("res", 5, "A", s), ("mark", 5, "A"), ("amt", 5, "A", 5)}
    # settled: the one-phase call serves a retry with that t and refuses another; t = s cancels, t = 0 is an amount like any other
    amt = {(e[1], e[2], e[3]) for e in receipts if e[0] == "amt"}
    assert rr.model([P], set(spent), set(amt), None, [5])[:3] == ([0], [1], [1])
    assert rr.model([P], set(spent), set(amt), None, [4])[0] == [3]
    assert settle([R], [0], [0], receipts, 2)[0] == [247] and settle([R], [0], None, set(receipts), 2)[0] == [247]
    # an unsettled reservation is a foreign spend for the one-phase calls: their receipts' view holds no amount tag
    assert rr.model([W._replace(k=8)], {8}, set(), None, [0])[0] == [3]
    # the hashes: separated from the receipt tags and from one another, top nibble clear, k and s reduced
    k, kp = bytes(range(32)), bytes(range(32, 64))
    assert len({tag_res(k, kp, 0), tag_res(k, kp, 1), marker(k, kp), tag(k, kp, 0), tag(k, kp, 1)}) == 5
    assert tag_res(k, kp, 1) == tag_res(k, kp, 1 + ELL) and tag_res(k, kp, s)[31] & 0xF0 == 0 and marker(k, kp)[31] & 0xF0 == 0
    assert prep(record(k, kp, s), 0, s, 1)[0] == 0 and prep(record(k, kp, s), 0, s + 1, 1)[0] == 249 and prep(record(k, kp, s), 1, 0, 1)[0] == 248
    assert prep(record(k, kp, s), 0, s + ELL, 1) == (0, tag_res(k, kp, s), marker(k, kp), tag(k, kp, s))


# ---- the host build of the lane bodies ------------------------------------------------------------------------------------------------------
def build_program(out, sanitized: bool):
    """tests/hostcheck/reserve_check.cpp, a stand-alone program with its own main over csrc/reserve_lanes.h: plain, or under
    AddressSanitizer and UBSan with the sanitizers' runtimes linked in, so that nothing has to be preloaded"""
    src = os.path.join(ROOT, "tests", "hostcheck", "reserve_check.cpp")
    extra = ["-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if sanitized else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-Wno-psabi", *extra, "-o", out, src], check=True)
    return out
