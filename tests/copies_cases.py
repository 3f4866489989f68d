"""Shared by the tests of admission's copy stage (tests/test_copies_host.py, tests/test_gpu_copies.py, tools/copies_probe.py): the loop
of act_redeem_(cbor_)admit_unique_batch as a model over labels and input-byte identities; the fixed lane mix of the feature with
HAND-WRITTEN expectations; the seeded lane plans of the equality runs; and the host build of the copy lane bodies
(tests/hostcheck/copy_check.cpp) with its checks.  Not a test module."""
import ctypes as C
import os
import random
import subprocess
from collections import namedtuple

import admission_cases as ad

ROOT = ad.ROOT
KEY_NONE, DOUBLE_SPEND, WRONG_CHARGE = ad.KEY_NONE, ad.DOUBLE_SPEND, ad.WRONG_CHARGE
UNDETERMINED, RECORDED_UNSIGNED = 252, 251
COPY_NONE = 0xFFFFFFFF
COUNTS = ad.COUNTS + ("copies",)


def copy_status(leader_status):
    """the table of the header, written out: what a copy answers for each final status of its leader"""
    return {255: 255, 6: 6, 7: 7, DOUBLE_SPEND: DOUBLE_SPEND, UNDETERMINED: UNDETERMINED, 0: DOUBLE_SPEND, RECORDED_UNSIGNED: DOUBLE_SPEND}[leader_status]


def model(lanes, blobs, spent, charges=None):
    """The loop of the header with step 3a.  blobs[i]: the identity of lane i's input bytes (any hashable; equal iff the bytes are).
    -> (statuses, out_key, counts with copies, recorded, copy_of: the leader's lane or None)"""
    before = frozenset(spent)
    now = set(before)
    n = len(lanes)
    st, ok, rec, copy_of = [None] * n, [KEY_NONE] * n, [], [None] * n
    c = dict.fromkeys(COUNTS, 0)
    c["lanes"] = n
    leaders = {}
    for i, ln in enumerate(lanes):
        if ln.wire:
            st[i] = ln.wire; c["wire_rejected"] += 1; continue
        if charges is not None and ln.s % ad.ELL != charges[i] % ad.ELL:
            st[i] = WRONG_CHARGE; c["wrong_charge"] += 1; continue
        if ln.k in before:
            st[i] = DOUBLE_SPEND; c["spent_before"] += 1; continue
        if blobs[i] in leaders:                                        # 3a. the bytes of an earlier lane that passed steps 1-3
            copy_of[i] = leaders[blobs[i]]; c["copies"] += 1; continue
        leaders[blobs[i]] = i
        c["verified"] += 1
        if ln.verdict:
            st[i] = ln.verdict; c["rejected_by_verification"] += 1; continue
        ok[i] = ln.key
        if ln.k in now:
            st[i] = DOUBLE_SPEND; c["double_spend_after"] += 1; continue
        now.add(ln.k); rec.append((ln.k, ln.key))
        st[i] = 0; c["accepted"] += 1
    for i in range(n):
        if copy_of[i] is not None:
            st[i] = copy_status(st[copy_of[i]]); ok[i] = ok[copy_of[i]]
    return st, ok, c, rec, copy_of


def check_identities(c):
    assert c["verified"] == c["lanes"] - c["wire_rejected"] - c["wrong_charge"] - c["spent_before"] - c["copies"], c
    assert c["rejected_by_verification"] + c["double_spend_after"] + c["accepted"] == c["verified"], c


# ---- the fixed lane mix (the table of the feature), hand-written ------------------------------------------------------------------------
# (token, proof: which bytes -- lanes with one (token, proof) pair are byte-identical, verdict by construction, charge is the expected
# one).  "sp0" is recorded before the call; every proof spends ad.SPEND.  a / b are the two proofs of a token (one nullifier, different
# rng), x the tampered a, u the a with an undecodable A', i the a with A' = identity.
FIXED_MIX = [
    ("t0", "a", 0, True), ("t0", "a", 0, True), ("t0", "b", 0, True),
    ("t1", "x", 7, True), ("t1", "x", 7, True), ("t1", "a", 0, True), ("t1", "a", 0, True),
    ("sp0", "a", 0, True), ("sp0", "a", 0, True),
    ("t2", "u", 255, True), ("t2", "u", 255, True),
    ("t3", "a", 0, False), ("t3", "a", 0, True), ("t3", "a", 0, True),
    ("t4", "i", 6, True), ("t4", "i", 6, True),
]
# the wire form adds: a respelled message twice (the second is a copy); the canonical and the respelled message of one proof (both
# verified, the second is a double spend); one message without and with a trailing byte (not copies)
FIXED_WIRE_EXTRA = [
    ("t5", "a/respelled", 0, True), ("t5", "a/respelled", 0, True),
    ("t6", "a", 0, True), ("t6", "a/respelled", 0, True),
    ("t7", "a", 0, True), ("t7", "a/trailing", 0, True),
]
FIXED_TOKENS = ("t0", "t1", "t2", "t3", "t4", "t5", "t6", "t7", "sp0")
FIXED_SPENT = ("sp0",)
N_RECORD_LANES = 16
# written down by hand from the issue's table, not computed
FIXED_EXPECT = [0, 3, 3, 7, 7, 0, 3, 3, 3, 255, 255, 250, 0, 3, 6, 6] + [0, 3, 0, 3, 0, 3]
FIXED_KEYS = [0, 0, 0, 255, 255, 0, 0, 255, 255, 255, 255, 255, 0, 0, 255, 255] + [0, 0, 0, 0, 0, 0]      # out_key with a ring of one key
FIXED_COPY_OF = [None, 0, None, None, 3, None, 5, None, None, None, 9, None, None, 12, None, 14] + [None, 16, None, None, None, None]
FIXED_COUNTS_RECORDS = dict(lanes=16, wire_rejected=0, wrong_charge=1, spent_before=2, copies=6, verified=7, rejected_by_verification=3, double_spend_after=1, accepted=3)
FIXED_COUNTS_WIRE = dict(lanes=22, wire_rejected=0, wrong_charge=1, spent_before=2, copies=7, verified=12, rejected_by_verification=3, double_spend_after=3, accepted=6)


def fixed_lanes(wire):
    """-> (lanes, blobs, charges) of the fixed mix over token NAMES"""
    mix = FIXED_MIX + (FIXED_WIRE_EXTRA if wire else [])
    lanes = [ad.Lane(tok, ad.SPEND, verdict, 0, 0) for tok, _, verdict, _ in mix]
    blobs = [(tok, proof) for tok, proof, _, _ in mix]
    charges = [ad.SPEND if right else ad.EXPECTED_WRONG for _, _, _, right in mix]
    return lanes, blobs, charges


def check_model_on_fixed_mix():
    for wire in (False, True):
        lanes, blobs, charges = fixed_lanes(wire)
        n = len(lanes)
        st, ok, c, rec, copy_of = model(lanes, blobs, set(FIXED_SPENT), charges)
        assert st == FIXED_EXPECT[:n] and ok == FIXED_KEYS[:n] and copy_of == FIXED_COPY_OF[:n], (wire, st, ok, copy_of)
        assert c == (FIXED_COUNTS_WIRE if wire else FIXED_COUNTS_RECORDS), (wire, c)
        check_identities(c)
        # the theorem: everything but the counts is what the existing admission loop answers
        ast, aok, ac, arec = ad.model(lanes, set(FIXED_SPENT), charges)
        assert (st, ok, rec) == (ast, aok, arec), wire
        assert ac["verified"] == c["verified"] + c["copies"] and all(ac[k] == c[k] for k in ("lanes", "wire_rejected", "wrong_charge", "spent_before", "accepted"))


# ---- the seeded plans of the equality runs ------------------------------------------------------------------------------------------------
PLAN_N = 2 * 4096 + 17
FRACTIONS = ((0, 1), (1, 2), (7, 8))
# token: which token the lane spends; variant: which of its two proofs; tampered; spent: recorded before the call; wrong: the lane is
# asked the wrong charge (only with charges); copy_of: the earlier lane whose bytes this lane repeats, or None
PlanLane = namedtuple("PlanLane", "token variant tampered spent wrong copy_of")
# what a lane that is not a copy is, in turn: a fresh valid proof, a tampered one, the OTHER proof of the last valid token (verified, then
# a double spend), a replay of a recorded token, a valid proof that is asked the wrong charge.  At 7/8 one lane in eight is left for
# these, and accepted and rejected-by-verification can only both reach 1/16 of the lanes when they share that eighth between them.
CYCLE = ("v", "t", "v2", "s", "w", "v", "t")
CYCLE_7_8 = ("v", "t")


def copy_plan(n, num, den, seed, with_charges):
    r = random.Random(seed * 1000003 + num * 101 + den)
    cycle = CYCLE_7_8 if (num, den) == (7, 8) else CYCLE
    plan, bases, tok, turn, last_valid = [], [], 0, 0, None
    for i in range(n):
        if bases and r.random() * den < num:
            src = bases[r.randrange(len(bases))]
            p = plan[src]
            # the bytes of lane src; the charge belongs to the lane: now and then a copy is asked the wrong one, and a copy of a
            # wrong-charge lane is asked the right one
            wrong = with_charges and (r.random() < 1 / 16 if not p.wrong else r.random() < 1 / 2)
            plan.append(PlanLane(p.token, p.variant, p.tampered, p.spent, wrong, src))
            continue
        kind = cycle[turn % len(cycle)]; turn += 1
        if kind == "v2" and last_valid is not None:
            plan.append(PlanLane(last_valid, 1, False, False, False, None))
        else:
            plan.append(PlanLane(tok, 0, kind == "t", kind == "s", with_charges and kind == "w", None))
            if kind in ("v", "v2"):
                last_valid = tok
            tok += 1
        bases.append(i)
    return plan, tok


def plan_lanes(plan, nullifier=lambda t: t, verdict=lambda p: 7 if p.tampered else 0, key=lambda p: 0):
    """-> (model lanes, blobs, charges, spent set) of a plan"""
    lanes = [ad.Lane(nullifier(p.token), ad.SPEND, verdict(p), key(p), 0) for p in plan]
    blobs = [(p.token, p.variant, p.tampered) for p in plan]
    charges = [ad.SPEND + 1 if p.wrong else ad.SPEND for p in plan]
    spent = {nullifier(p.token) for p in plan if p.spent}
    return lanes, blobs, charges, spent


def plan_categories(plan, with_charges):
    lanes, blobs, charges, spent = plan_lanes(plan)
    st, ok, c, rec, copy_of = model(lanes, blobs, spent, charges if with_charges else None)
    cats = dict(accepted=c["accepted"], rejected_by_verification=c["rejected_by_verification"],
                copies_of_valid=sum(1 for i in range(len(plan)) if copy_of[i] is not None and st[copy_of[i]] == 0),
                copies_of_tampered=sum(1 for i in range(len(plan)) if copy_of[i] is not None and st[copy_of[i]] == 7))
    return cats, c


def plan_is_mixed_enough(n, num, den, seed):
    for with_charges in (False, True):
        plan, _ = copy_plan(n, num, den, seed, with_charges)
        cats, _ = plan_categories(plan, with_charges)
        if any(16 * v < n for v in cats.values()):
            return False
    return True


def find_seed(n, num, den, limit=200):
    for seed in range(1, limit):
        if plan_is_mixed_enough(n, num, den, seed):
            return seed
    raise AssertionError("no seed below %d gives every category 1/16 of the lanes at %d/%d" % (limit, num, den))


# chosen on the CPU (tests/test_copies_host.py asserts it): the smallest seed with which each of the four categories holds at least 1/16
# of the lanes, with and without charges
PLAN_SEEDS = {(0, 1): 1, (1, 2): 1, (7, 8): 1}


def plan_seed(num, den):
    return PLAN_SEEDS[(num, den)]


def check_model_on_plans():
    """the copy model against admission_cases.model, status for status, on every seeded plan; the identities of the counts"""
    for (num, den) in FRACTIONS:
        for with_charges in (False, True):
            plan, tokens = copy_plan(PLAN_N, num, den, plan_seed(num, den), with_charges)
            lanes, blobs, charges, spent = plan_lanes(plan)
            ch = charges if with_charges else None
            st, ok, c, rec, copy_of = model(lanes, blobs, spent, ch)
            ast, aok, ac, arec = ad.model(lanes, spent, ch)
            assert (st, ok, rec) == (ast, aok, arec), (num, den, with_charges)
            check_identities(c)
            assert ac["verified"] - c["verified"] == c["copies"] and tokens <= PLAN_N
            if num == 0:
                assert c["copies"] == 0
            else:
                # the plan repeats an earlier lane's bytes in num/den of the lanes; those whose bytes are shed (a replay, a wrong charge)
                # are counted there and not as copies
                repeats = sum(1 for p in plan if p.copy_of is not None)
                assert abs(repeats / PLAN_N - num / den) < 0.02 and 0 < c["copies"] <= repeats, (num, den, repeats, c)
                # a copy's leader is an earlier lane with the same bytes that is not a copy itself
                for i, l in enumerate(copy_of):
                    if l is not None:
                        assert l < i and blobs[l] == blobs[i] and copy_of[l] is None


# ---- host build of the lane bodies -------------------------------------------------------------------------------------------------------
def build_copy_check(out, sanitize=False):
    csrc = os.path.join(ROOT, "anonymous-credit-tokens_amd", "csrc")
    src = os.path.join(ROOT, "tests", "hostcheck", "copy_check.cpp")
    deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".h", ".inc"))]
    if os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in deps):
        return out
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-Wno-psabi", *flags, "-o", out, src], check=True)
    return out


def load_copy_check(path):
    cc = C.CDLL(path)
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    cc.hc_copy_fp.argtypes = [vp, u64, C.c_char_p]; cc.hc_copy_fp.restype = u64
    cc.hc_copy_fp_reversed.argtypes = [vp, u64, C.c_char_p]; cc.hc_copy_fp_reversed.restype = u64
    cc.hc_copy_fp_host.argtypes = [vp, u64, C.c_char_p]; cc.hc_copy_fp_host.restype = u64
    cc.hc_copy_fp_lanes.argtypes = [vp, vp, u64, vp, u32, C.c_char_p, vp]; cc.hc_copy_fp_lanes.restype = None
    cc.hc_copy_leaders.argtypes = [vp, u32, u32, vp, vp]; cc.hc_copy_leaders.restype = u32
    cc.hc_copy_equal.argtypes = [vp, vp, u64, vp, vp, u32, vp]; cc.hc_copy_equal.restype = None
    cc.hc_copy_mark.argtypes = [vp, vp, u32, vp, vp]; cc.hc_copy_mark.restype = None
    cc.hc_copy_resolve.argtypes = [vp, u32, vp, vp]; cc.hc_copy_resolve.restype = None
    return cc


SALT = bytes(range(16, 32))
FP_LENGTHS = (1, 15, 16, 17, 832, 1472, 18036)      # 832 / 1472: the records at L = 8 / 16 ... ; 18036: the SpendProof message at L = 128


def _u32(vals):
    return (C.c_uint32 * max(1, len(vals)))(*vals)


def _u64(vals):
    return (C.c_uint64 * max(1, len(vals)))(*vals)


def check_fingerprint(cc, lengths=FP_LENGTHS):
    """depends on every byte and on the length, never 0, the same at every source address mod 16, whatever order the partial values
    are added in, and keyed with the salt"""
    r = random.Random(17)
    for ln in lengths:
        data = bytes(r.randrange(256) for _ in range(ln))
        buf = C.create_string_buffer(ln + 64)
        base = C.addressof(buf)
        a0 = (-base) % 16
        seen = set()
        for off in range(16):
            C.memmove(base + a0 + off, data, ln)
            seen.add(cc.hc_copy_fp(base + a0 + off, ln, SALT))
        assert len(seen) == 1 and 0 not in seen, (ln, seen)
        fp = seen.pop()
        at = base + a0 + 15                                             # (the bytes are here after the last round)
        assert cc.hc_copy_fp_reversed(at, ln, SALT) == fp == cc.hc_copy_fp_host(at, ln, SALT)      # the host workers' walk: bit for bit
        assert cc.hc_copy_fp(at, ln, bytes(16)) != fp, "the salt does not enter"
        view = (C.c_ubyte * ln).from_address(at)
        for i in range(ln):                                             # every byte in turn, one bit and all bits
            for flip in (1, 0xFF) if ln <= 1472 else (1 << (i % 8),):
                view[i] ^= flip
                got = cc.hc_copy_fp(at, ln, SALT)
                view[i] ^= flip
                assert got != fp and got != 0, (ln, i, flip)
        assert cc.hc_copy_fp(at, ln, SALT) == fp
        # the length goes in: a zero-padded last piece is not the longer message that ends in zeros
        longer = C.create_string_buffer(data + bytes(16))
        for extra in (1, 15, 16):
            assert cc.hc_copy_fp(C.addressof(longer), ln + extra, SALT) != fp, (ln, extra)
        if ln > 1:
            assert cc.hc_copy_fp(at, ln - 1, SALT) != fp
    # two pieces that change places are another message
    two = bytes(range(32))
    b1, b2 = C.create_string_buffer(two), C.create_string_buffer(two[16:] + two[:16])
    assert cc.hc_copy_fp(C.addressof(b1), 32, SALT) != cc.hc_copy_fp(C.addressof(b2), 32, SALT)
    assert cc.hc_copy_fp(C.addressof(b1), 0, SALT) != 0


LEADER_NS = (0, 1, 63, 64, 65, 257, 70000)
CLASS_SHAPES = ("distinct", "equal", "pairs", "random")


def class_shape(name, n, seed=3):
    """-> the class of every lane (lanes of one class carry one fingerprint)"""
    r = random.Random(seed * 7919 + n)
    if name == "distinct":
        return list(range(n))
    if name == "equal":
        return [0] * n
    if name == "pairs":
        return [i // 2 for i in range(n)]
    out, cls = [], 0
    while len(out) < n:
        size = min(n - len(out), r.choice((1, 1, 1, 2, 3, 9, 70)))
        out += [cls] * size; cls += 1
    r.shuffle(out)
    return out


def want_leaders(fps):
    first = {}
    return [first.setdefault(f, j) for j, f in enumerate(fps)]


def host_leaders(cc, fps, cap=0, order=None):
    m = len(fps)
    leader = _u32([0] * m)
    used = cc.hc_copy_leaders(_u64(fps), m, cap, _u32(order) if order is not None else None, leader)
    return list(leader[:m]), used


def check_leader(cc, ns=LEADER_NS):
    """against a Python dictionary, every n and class shape; the claims in lane order, in reverse and shuffled give the same leaders;
    fingerprints that all start at ONE slot of the table (forced collisions of the slot function) are probed apart"""
    r = random.Random(23)
    for n in ns:
        for shape in CLASS_SHAPES:
            cls = class_shape(shape, n)
            fp_of = {}
            fps = [fp_of.setdefault(c, r.randrange(1, 1 << 64)) for c in cls]
            want = want_leaders(fps)
            orders = [None, list(range(n))[::-1]]
            if n <= 257:
                sh = list(range(n)); r.shuffle(sh); orders.append(sh)
            for order in orders:
                got, used = host_leaders(cc, fps, order=order)
                assert got == want and used == len(set(fps)), (n, shape, order is None)
            if n in (65, 257, 70000):
                # forced collisions: the upper word picks the slot -- every class starts at one slot and the table probes them apart
                crowd = {c: (0xABCD1234 << 32) | (c + 1) for c in set(cls)}
                fps2 = [crowd[c] for c in cls]
                got, used = host_leaders(cc, fps2)
                assert got == want_leaders(fps2) == want and used == len(crowd), (n, shape)
    # a table that is exactly full still answers (the engine's is at most half full)
    fps = [(7 << 32) | (i + 1) for i in range(8)]
    got, used = host_leaders(cc, fps + fps, cap=8)
    assert got == list(range(8)) * 2 and used == 8


def _spans(rows, lead_pad=0):
    """rows of uneven length behind lead_pad bytes -> (blob, offsets)"""
    offs = [lead_pad]
    for row in rows:
        offs.append(offs[-1] + len(row))
    return bytes(lead_pad) + b"".join(rows) + b"\0", offs


def host_equal(cc, blob, offs, row_bytes, idx, leader):
    m = len(idx)
    out = _u32([0] * m)
    cc.hc_copy_equal(blob, _u64(offs) if offs is not None else None, row_bytes, _u32(idx), _u32(leader), m, out)
    return list(out[:m])


def check_compare(cc):
    """a forced fingerprint collision (the leader array names lane 0 for everybody) never makes a copy of a lane that differs in the
    first byte only, in the last byte only, in one byte of the 16-byte tail or in length only"""
    r = random.Random(29)
    for ln in (37, 832, 18036):
        base = bytes(r.randrange(256) for _ in range(ln))
        def flip(i):
            b = bytearray(base); b[i] ^= 0x40
            return bytes(b)
        tail0 = (ln - 1) // 16 * 16
        rows = [base, base, flip(0), flip(ln - 1), flip(tail0), flip(max(0, tail0 - 1)), flip(ln // 2), base]
        n = len(rows)
        want = [COPY_NONE, 0, COPY_NONE, COPY_NONE, COPY_NONE, COPY_NONE, COPY_NONE, 0]
        leader = [0] * n
        # rows of one size (the records form), lanes 1:1 and through an index that skips lanes
        assert host_equal(cc, b"".join(rows) + b"\0", None, ln, list(range(n)), leader) == want, ln
        assert host_equal(cc, b"".join(rows) + b"\0", None, ln, [0, 2, 7], [0, 0, 0]) == [COPY_NONE, COPY_NONE, 0]
        # messages between offsets, starting at every address mod 16, with lanes that differ in LENGTH only
        for pad in range(16):
            rows2 = rows + [base[:-1], base + b"\0", base + base[-1:], b"", b""]
            blob, offs = _spans(rows2, pad)
            got = host_equal(cc, blob, offs, 0, list(range(len(rows2))), [0] * len(rows2))
            assert got == want + [COPY_NONE] * 5, (ln, pad, got)      # (the empty message is not a copy of lane 0 either)
        # a leader is an EARLIER lane: an array that names a later one or the lane itself makes no copy
        assert host_equal(cc, b"".join(rows) + b"\0", None, ln, list(range(n)), [1, 1, 2, 7, 7, 5, 6, 7]) == [COPY_NONE] * n
    blob, offs = _spans([b"", b"", b"x"])
    assert host_equal(cc, blob, offs, 0, [0, 1, 2], [0, 0, 0]) == [COPY_NONE, 0, COPY_NONE]


def check_resolve(cc):
    """every row of the status table; out_key follows the leader; lanes that are not copies keep what they have"""
    rows = [(255, 255, 255), (6, 255, 6), (7, 255, 7), (3, 2, 3), (UNDETERMINED, 1, UNDETERMINED), (0, 3, 3), (RECORDED_UNSIGNED, 0, 3)]
    for leader_status, leader_key, want in rows:
        assert cc.hc_copy_status(leader_status) == want == copy_status(leader_status)
    n = 300
    r = random.Random(37)
    status = bytearray(0x55 for _ in range(n + 1)); okey = bytearray(0x66 for _ in range(n + 1))
    lead = [COPY_NONE] * n
    want_st, want_ok = bytearray(status), bytearray(okey)
    for t, (ls, lk, want) in enumerate(rows):
        status[t], okey[t] = ls, lk
        want_st[t], want_ok[t] = ls, lk
    for i in range(len(rows), n):
        if r.random() < 0.6:
            lead[i] = r.randrange(len(rows))
            want_st[i], want_ok[i] = rows[lead[i]][2], rows[lead[i]][1]
    sb = (C.c_ubyte * (n + 1)).from_buffer(status); kb = (C.c_ubyte * (n + 1)).from_buffer(okey)
    cc.hc_copy_resolve(_u32(lead), n, sb, kb)
    del sb, kb
    assert status == want_st and okey == want_ok
    assert cc.hc_copy_mark_value() not in {s for s, _, _ in rows} | {250, 253, 254} and cc.hc_copy_mark_value() != 0


def host_stage(cc, blob, offs, row_bytes, pre):
    """the whole stage on the host as the engine strings it together: survivors of `pre`, fingerprints, leaders, compare, mark
    -> (pre2, lead per lane)"""
    n = len(pre)
    idx = [i for i in range(n) if pre[i] == 0]
    m = len(idx)
    fp = _u64([0] * m)
    cc.hc_copy_fp_lanes(blob, _u64(offs) if offs is not None else None, row_bytes, _u32(idx), m, SALT, fp)
    leader, _ = host_leaders(cc, list(fp[:m]))
    copy_of = host_equal(cc, blob, offs, row_bytes, idx, leader)
    pre2 = bytearray(pre) + b"\x77"; lead = _u32([COPY_NONE] * n + [0x77])
    pb = (C.c_ubyte * (n + 1)).from_buffer(pre2)
    cc.hc_copy_mark(_u32(idx), _u32(copy_of), m, pb, lead)
    del pb
    assert pre2[n] == 0x77 and lead[n] == 0x77
    return bytes(pre2[:n]), list(lead[:n]), list(fp[:m])


def check_stage(cc):
    """random short messages with many repeats and some shed lanes: the marked lanes and their leaders are the model's"""
    r = random.Random(43)
    mark = cc.hc_copy_mark_value()
    for n in (0, 1, 2, 63, 64, 65, 257, 1500):
        pool = [bytes(r.randrange(256) for _ in range(r.choice((0, 1, 15, 16, 17, 33, 70)))) for _ in range(max(1, n // 3))]
        pool += [p + b"\0" for p in pool[:5]] + [p[:-1] for p in pool[:5] if p]
        rows = [r.choice(pool) for _ in range(n)]
        pre = bytes(0 if r.random() < 0.7 else r.choice((3, 250, 254)) for _ in range(n))
        blob, offs = _spans(rows, 5)
        pre2, lead, fps = host_stage(cc, blob, offs, 0, pre)
        first, want_pre2, want_lead = {}, bytearray(pre), [COPY_NONE] * n
        for i in range(n):
            if pre[i] == 0:
                if rows[i] in first:
                    want_pre2[i] = mark; want_lead[i] = first[rows[i]]
                else:
                    first[rows[i]] = i
        assert pre2 == bytes(want_pre2) and lead == want_lead, n
        assert 0 not in fps
    # rows of one size
    rows = [bytes([r.randrange(3)]) * 40 for _ in range(200)]
    pre2, lead, _ = host_stage(cc, b"".join(rows) + b"\0", None, 40, bytes(200))
    assert [i for i in range(200) if pre2[i]] == [i for i in range(200) if rows[i] in rows[:i]] and all(l == COPY_NONE or rows[l] == rows[i] for i, l in enumerate(lead))


def check_all_lane_bodies(cc, quick=False):
    check_fingerprint(cc, (1, 15, 16, 17, 832) if quick else FP_LENGTHS)
    check_leader(cc, (0, 1, 63, 64, 65, 257) if quick else LEADER_NS)
    check_compare(cc)
    check_resolve(cc)
    check_stage(cc)
