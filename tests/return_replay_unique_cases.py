"""Shared by the tests of the return replay unique forms (tests/test_return_replay_unique_host.py, tests/test_gpu_return_replay_unique.py)
and tools/return_replay_unique_probe.py: the table of include/act_mi355x.h ("replayable partial refunds, unique forms") written out;
the loop of act_redeem_(cbor_)return_replay_unique_batch as a model over labels, input-byte identities and amounts, built on the models
of return_replay_cases (the screen with t^ <= s^, receipts as (k, K', t^)) and replay_cases (the tail); seeded lane plans whose repeats
name their source's amount or another one; and the host build of the serve pass (tests/hostcheck/copy_serve_return_check.cpp) as a
library and as a stand-alone sanitized program.  Not a test module."""
import ctypes as C
import os
import random
import subprocess
from collections import namedtuple

import admit_replay_cases as ar
import admit_replay_unique_cases as aru
import replay_cases as rp
import return_replay_cases as rr

ROOT = rr.ROOT
ELL = rr.ELL
KEY_NONE, DOUBLE_SPEND, WRONG_CHARGE, RETURN_TOO_BIG = rr.KEY_NONE, rr.DOUBLE_SPEND, rr.WRONG_CHARGE, rr.RETURN_TOO_BIG
UNDETERMINED, RECORDED_UNSIGNED = rp.UNDETERMINED, rp.RECORDED_UNSIGNED
COPY_NONE = aru.COPY_NONE
COUNTS = rr.COUNTS + ("copies", "copies_served", "copies_other_amount")


def serve(leader_status, leader_key, same):
    """the table of the header, written out: (status, out_key, replayed, takes the leader's record) of a copy whose amount is
    (same) or is not the leader's, both reduced mod l"""
    if leader_status == 0:
        return (0, leader_key, 1, True) if same else (DOUBLE_SPEND, leader_key, 0, False)
    if leader_status == RECORDED_UNSIGNED:
        # same amount: k is spent and the receipt is this lane's own -- the mark the plain call's tail sets before its signing step fails
        return (RECORDED_UNSIGNED, leader_key, 1, False) if same else (DOUBLE_SPEND, leader_key, 0, False)
    assert leader_status in (255, 6, 7, DOUBLE_SPEND, UNDETERMINED)
    return leader_status, leader_key, 0, False


def model(lanes, blobs, spent: set, receipts: set, charges=None, returned=None):
    """The loop of the header.  lanes: ar.Lane; blobs[i]: the identity of lane i's input bytes (equal iff the bytes are); receipts holds
    (k, K', t^); returned[i]: an int (None: all zero).  Mutates `spent` and `receipts` as the tail does.
    -> (statuses, out_key, replayed, counts, copy_of: the leader's lane or None)"""
    before, had = frozenset(spent), frozenset(receipts)
    n = len(lanes)
    ts = [0] * n if returned is None else [rr.that(t) for t in returned]
    st, ok, rep, copy_of = [None] * n, [KEY_NONE] * n, [0] * n, [None] * n
    c = dict.fromkeys(COUNTS, 0)
    c["lanes"] = n
    go, leaders = [], {}
    for i, ln in enumerate(lanes):
        if ln.wire:
            st[i] = ln.wire; c["wire_rejected"] += 1; continue
        if charges is not None and ln.s % ELL != charges[i] % ELL:
            st[i] = WRONG_CHARGE; c["wrong_charge"] += 1; continue
        if ts[i] > ln.s % ELL:
            st[i] = RETURN_TOO_BIG; c["return_too_big"] += 1; continue
        if ln.k in before:
            pre, cand = ar.decide(DOUBLE_SPEND, True, not ln.com_ok, (ln.k, ln.kprime, ts[i]) in had)
            if pre:
                st[i] = pre; c["foreign_spend"] += 1; continue
            c["retry_candidates"] += cand
        if blobs[i] in leaders:                                         # the bytes of an earlier lane that passed the screen, WHATEVER its amount
            copy_of[i] = leaders[blobs[i]]; c["copies"] += 1; continue
        leaders[blobs[i]] = i
        go.append(i)
    c["verified"] = len(go)
    inner = {(k, (kp, t)) for k, kp, t in receipts}
    mst, mok, mrep, mc = rp.model([rp.Lane(lanes[i].k, (lanes[i].kprime, ts[i]), lanes[i].verdict, lanes[i].key) for i in go], spent, inner)
    receipts.clear(); receipts.update((k, kp, t) for k, (kp, t) in inner)
    for j, i in enumerate(go):
        st[i], ok[i], rep[i] = mst[j], mok[j], mrep[j]
    c.update(rejected_by_verification=mc["rejected_by_verification"], fresh=mc["fresh"], replayed=mc["replayed"], double_spend_after=mc["double_spend"],
             unanswered=mc["unanswered"])
    for i in range(n):
        if copy_of[i] is not None:
            j = copy_of[i]
            st[i], ok[i], rep[i], _ = serve(st[j], ok[j], ts[i] == ts[j])
            c["copies_served"] += st[i] == 0
            c["copies_other_amount"] += ts[i] != ts[j]
    return st, ok, rep, c, copy_of


def check_identities(c):
    assert c["verified"] == c["lanes"] - c["wire_rejected"] - c["wrong_charge"] - c["return_too_big"] - c["foreign_spend"] - c["copies"], c
    assert c["rejected_by_verification"] + c["fresh"] + c["replayed"] + c["double_spend_after"] + c["unanswered"] == c["verified"], c
    assert c["copies_served"] <= c["copies"] and c["copies_other_amount"] <= c["copies"], c
    assert c["copies_served"] + c["copies_other_amount"] <= c["copies"], c      # a copy that names another amount is never answered 0


def check_count_relation(c, pc, st, copy_of):
    """c: the unique form's counts, pc: act_redeem_(cbor_)return_replay_batch's on the same batch, st: the (common) final statuses"""
    assert all(c[k] == pc[k] for k in ("lanes", "wire_rejected", "wrong_charge", "return_too_big", "foreign_spend", "retry_candidates", "fresh")), (c, pc)
    assert pc["verified"] - c["verified"] == c["copies"] == sum(1 for l in copy_of if l is not None), (c, pc)
    served = sum(1 for i, l in enumerate(copy_of) if l is not None and st[i] == 0)
    assert c["copies_served"] == served and pc["replayed"] - c["replayed"] == served, (c, pc)
    for name, codes in (("rejected_by_verification", (255, 6, 7)), ("double_spend_after", (DOUBLE_SPEND,)), ("unanswered", (UNDETERMINED, RECORDED_UNSIGNED))):
        assert pc[name] - c[name] == sum(1 for i, l in enumerate(copy_of) if l is not None and st[i] in codes), (name, c, pc)


def check_against_the_plain_form(lanes, blobs, spent, receipts, charges=None, returned=None):
    """the promise on the models: statuses, out_key, replay marks and both sets are those of return_replay_cases.model"""
    s1, r1, s2, r2 = set(spent), set(receipts), set(spent), set(receipts)
    st, ok, rep, c, copy_of = model(lanes, blobs, s1, r1, charges, returned)
    pst, pok, prep, pc = rr.model(lanes, s2, r2, charges, returned)
    assert (st, ok, rep) == (pst, pok, prep), (st, pst, ok, pok, rep, prep)
    assert (s1, r1) == (s2, r2)
    check_identities(c)
    check_count_relation(c, pc, st, copy_of)
    return st, ok, rep, c, copy_of


# ---- the fixed mixes, hand-written ----------------------------------------------------------------------------------------------------------
# P, Q: two proofs of token "a" (one nullifier, another K'); X: P tampered outside k and Com; R: the proof token "sp" was redeemed with
# before the call, for the amount 2; every proof spends S = 3.  (lane, blob, amount) -> hand-written (status, out_key, replayed, copy_of).
S = 3
_P, _Q, _X = ar.Lane("a", "A", 0, 0, S), ar.Lane("a", "B", 0, 0, S), ar.Lane("b", "A", 7, KEY_NONE, S)
_R, _Z = ar.Lane("sp", "A", 0, 1, S), ar.Lane("c", "A", 0, 1, S)
FIXED = {
    # the header's example and its mirror
    "t1 t1 t2": ([(_P, "P", 2), (_P, "P", 2), (_P, "P", 1)], [(0, 0, 0, None), (0, 0, 1, 0), (3, 0, 0, 0)]),
    "t1 t2 t2": ([(_P, "P", 2), (_P, "P", 1), (_P, "P", 1)], [(0, 0, 0, None), (3, 0, 0, 0), (3, 0, 0, 0)]),
    # t + l is t; t > s is shed by the screen and is neither leader nor copy: the NEXT lane leads
    "t + l": ([(_P, "P", 2), (_P, "P", 2 + ELL), (_P, "P", ELL)], [(0, 0, 0, None), (0, 0, 1, 0), (3, 0, 0, 0)]),
    "t > s first": ([(_P, "P", S + 1), (_P, "P", 2), (_P, "P", S + 1), (_P, "P", 2)], [(249, 255, 0, None), (0, 0, 0, None), (249, 255, 0, None), (0, 0, 1, 1)]),
    # a retry of an earlier call leads; a first lane that names another amount than the receipt's is shed, the next one leads
    "retry leads": ([(_R, "R", 2), (_R, "R", 2), (_R, "R", 2 + ELL)], [(0, 1, 1, None), (0, 1, 1, 0), (0, 1, 1, 0)]),
    "foreign first": ([(_R, "R", 1), (_R, "R", 2), (_R, "R", 2), (_R, "R", 1)], [(3, 255, 0, None), (0, 1, 1, None), (0, 1, 1, 1), (3, 255, 0, None)]),
    # an invalid leader hands its verdict on whatever the amounts; the other proof of a token loses behind verification, and so do its copies
    "invalid leader": ([(_X, "X", 1), (_X, "X", 1), (_X, "X", 2)], [(7, 255, 0, None), (7, 255, 0, 0), (7, 255, 0, 0)]),
    "second proof": ([(_P, "P", 1), (_Q, "Q", 1), (_Q, "Q", 1), (_Q, "Q", 2)], [(0, 0, 0, None), (3, 0, 0, None), (3, 0, 0, 1), (3, 0, 0, 1)]),
    # nothing returned at all, and zero against non-zero
    "zero": ([(_Z, "Z", 0), (_Z, "Z", ELL), (_Z, "Z", 1)], [(0, 1, 0, None), (0, 1, 1, 0), (3, 1, 0, 0)]),
}
FIXED_SPENT, FIXED_RECEIPTS = {"sp"}, {("sp", "A", 2)}


def check_model_on_fixed_mixes():
    for name, (mix, want) in FIXED.items():
        lanes, blobs, returned = [m[0] for m in mix], [m[1] for m in mix], [m[2] for m in mix]
        st, ok, rep, c, copy_of = check_against_the_plain_form(lanes, blobs, FIXED_SPENT, FIXED_RECEIPTS, [S] * len(mix), returned)
        assert list(zip(st, ok, rep, copy_of)) == want, (name, list(zip(st, ok, rep, copy_of)))
    c = model([m[0] for m in FIXED["t1 t2 t2"][0]], ["P"] * 3, set(), set(), None, [2, 1, 1])[3]
    assert (c["copies"], c["copies_served"], c["copies_other_amount"], c["verified"], c["fresh"]) == (2, 0, 2, 1, 1), c
    # the wire-only corner the header names: [A t1, A' t2, A' t1] with A' another spelling of A -- the plain call replays lane 2
    A, A2 = ar.Lane("w", "A", 0, 0, S), ar.Lane("w", "A", 0, 0, S)
    st = model([A, A2, A2], ["A", "A'", "A'"], set(), set(), None, [2, 1, 2])[0]
    pst = rr.model([A, A2, A2], set(), set(), None, [2, 1, 2])[0]
    assert (st, pst) == ([0, 3, 3], [0, 3, 0])


# ---- the seeded plans ---------------------------------------------------------------------------------------------------------------------
# token / variant / tampered / spent (redeemed before the call with variant 0 and the amount spent_t) / wrong charge / the amount the lane
# names / copy_of: the earlier lane whose bytes it repeats, or None
PlanLane = namedtuple("PlanLane", "token variant tampered spent wrong t copy_of")
# fresh valid, tampered, retry, the other proof of the last valid token (it spends no new token), a retry that names another amount (shed),
# a foreign K', a wrong charge, t > s: eight new tokens in ten lanes
CYCLE = ("v", "t", "r", "d", "v", "d", "f", "s", "w", "b")
AMOUNTS = (0, 1, 2, S)


def spent_amount(token):
    """what token `token` was redeemed for before the call"""
    return AMOUNTS[token % len(AMOUNTS)]


def copy_plan(n, num, den, seed, with_charges=True):
    """n lanes of which about num/den repeat the bytes of an earlier lane: two in three of those name their source's amount (now and then
    as t + l), the others another one (now and then one above s)"""
    r = random.Random(seed * 1000003 + num * 101 + den + n)
    plan, tok, turn, last_valid = [], 0, 0, None
    for i in range(n):
        if plan and r.random() * den < num:
            src = r.randrange(len(plan))
            while plan[src].copy_of is not None:                        # the amount is chosen against the FIRST lane with these bytes
                src = plan[src].copy_of
            p = plan[src]
            roll = r.random()
            if roll < 0.5:
                t = p.t
            elif roll < 0.66:
                t = p.t % ELL + ELL if p.t < ELL else p.t % ELL
            elif roll < 0.95:
                t = r.choice([a for a in AMOUNTS if a != p.t % ELL])
            else:
                t = S + 1
            plan.append(PlanLane(p.token, p.variant, p.tampered, p.spent, with_charges and r.random() < 1 / 16, t, src))
            continue
        kind = CYCLE[turn % len(CYCLE)]
        turn += 1
        if kind == "d" and last_valid is None:
            kind = "v"
        if kind == "d":
            plan.append(PlanLane(last_valid, 1, False, False, False, r.choice(AMOUNTS), None)); last_valid = None
            continue
        spent = kind in ("r", "f", "s")
        t = spent_amount(tok) if kind in ("r", "s") else AMOUNTS[(spent_amount(tok) + 1) % len(AMOUNTS)] if kind == "f" else S + 1 if kind == "b" else r.choice(AMOUNTS)
        plan.append(PlanLane(tok, 1 if kind == "s" else 0, kind == "t", spent, with_charges and kind == "w", t, None))
        if kind == "v":
            last_valid = tok
        tok += 1
    return plan, tok


def plan_lanes(plan, nullifier=lambda t: t, key=lambda p: p.token % 2):
    """-> (model lanes, blobs, charges, returned, spent set, receipts set) of a plan"""
    lanes = [ar.Lane(nullifier(p.token), (p.token, p.variant), 7 if p.tampered else 0, KEY_NONE if p.tampered else key(p), S) for p in plan]
    blobs = [(p.token, p.variant, p.tampered) for p in plan]
    charges = [S + 1 if p.wrong else S for p in plan]
    spent = {nullifier(p.token) for p in plan if p.spent}
    receipts = {(nullifier(p.token), (p.token, 0), spent_amount(p.token)) for p in plan if p.spent}
    return lanes, blobs, charges, [p.t for p in plan], spent, receipts


PLAN_SIZES = (65, 300)
FRACTIONS = ((0, 1), (1, 2), (7, 8))
# every kind of copy the table tells apart that a plan can hold (a leader ends 251 only when the signing step fails)
PLAN_KINDS = {(0, True), (0, False), (7, True), (7, False), (DOUBLE_SPEND, True), (DOUBLE_SPEND, False)}


def plan_is_mixed_enough(n, num, den, seed):
    """asserted on the MODEL's output, before anything runs on a GPU"""
    plan, _ = copy_plan(n, num, den, seed)
    lanes, blobs, charges, returned, spent, receipts = plan_lanes(plan)
    st, ok, rep, c, copy_of = model(lanes, blobs, set(spent), set(receipts), charges, returned)
    if num == 0:
        return c["copies"] == 0 and min(c[k] for k in ("return_too_big", "foreign_spend", "retry_candidates", "fresh", "wrong_charge", "replayed")) > 0
    ts = [rr.that(t) for t in returned]
    kinds = {(st[copy_of[i]], ts[i] == ts[copy_of[i]]) for i in range(n) if copy_of[i] is not None}
    served_of_retries = sum(1 for i in range(n) if copy_of[i] is not None and st[i] == 0 and rep[copy_of[i]] == 1)
    return (PLAN_KINDS <= kinds and 4 * c["copies"] >= n * num // den and c["copies_served"] >= 4 and c["copies_other_amount"] >= 4 and served_of_retries > 0
            and c["return_too_big"] > 0 and c["foreign_spend"] > 0 and any(copy_of[i] is not None and returned[i] >= ELL and st[i] == 0 for i in range(n)))


def find_seed(n, num, den, limit=400):
    for seed in range(1, limit):
        if plan_is_mixed_enough(n, num, den, seed):
            return seed
    raise AssertionError("no seed below %d fills every kind at %d lanes, %d/%d" % (limit, n, num, den))


# chosen on the CPU (tests/test_return_replay_unique_host.py asserts it): the smallest seed whose plan is mixed enough
PLAN_SEEDS = {(65, 0, 1): 1, (65, 1, 2): 7, (65, 7, 8): 2, (300, 0, 1): 1, (300, 1, 2): 1, (300, 7, 8): 1}


def plan_seed(n, num, den):
    return PLAN_SEEDS[(n, num, den)]


def check_model_on_plans():
    """the unique model against return_replay_cases.model, lane for lane and set for set, on every seeded plan"""
    for n in PLAN_SIZES:
        for num, den in FRACTIONS:
            assert plan_is_mixed_enough(n, num, den, plan_seed(n, num, den)), (n, num, den)
            plan, tokens = copy_plan(n, num, den, plan_seed(n, num, den))
            lanes, blobs, charges, returned, spent, receipts = plan_lanes(plan)
            st, ok, rep, c, copy_of = check_against_the_plain_form(lanes, blobs, spent, receipts, charges, returned)
            for i, l in enumerate(copy_of):                             # a copy's leader is an earlier lane with the same bytes that is no copy itself
                if l is not None:
                    assert l < i and blobs[l] == blobs[i] and copy_of[l] is None


# ---- host build of the serve pass -----------------------------------------------------------------------------------------------------------
def _build(out, extra):
    csrc = os.path.join(ROOT, "anonymous-credit-tokens_amd", "csrc")
    src = os.path.join(ROOT, "tests", "hostcheck", "copy_serve_return_check.cpp")
    deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".h", ".inc"))]
    if os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in deps):
        return out
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-Wno-psabi", *extra, "-o", out, src], check=True)
    return out


def build_check(out):
    """csrc/copy_lanes.h compiled with g++ into a small library"""
    return _build(out, ["-O2", "-fPIC", "-shared"])


def build_program(out):
    """the same file with its own main, under AddressSanitizer and UBSan: a stand-alone program with the sanitizers' runtimes linked in,
    so that nothing has to be preloaded"""
    return _build(out, ["-O1", "-g", "-DCOPY_SERVE_RETURN_CHECK_MAIN", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])


def load_check(path):
    sc = C.CDLL(path)
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    sc.hc_serve_return.argtypes = [vp, u32, u64, vp, vp, vp, vp, vp, C.c_int]; sc.hc_serve_return.restype = None
    sc.hc_serve_plain.argtypes = [vp, u32, u64, vp, vp, vp, vp]; sc.hc_serve_plain.restype = None
    sc.hc_same_amount.argtypes = [C.c_char_p, C.c_char_p]; sc.hc_same_amount.restype = C.c_int
    sc.hc_serve_return_checks.argtypes = [vp, u32]; sc.hc_serve_return_checks.restype = C.c_int
    sc.hc_serve_return_field_ops.argtypes = []; sc.hc_serve_return_field_ops.restype = u64
    return sc


def refund_return_wire_bytes(L):
    """act_cbor_size(ctx, ACT_CBOR_REFUND_RETURN): the framed RefundReturn (it does not depend on L)"""
    import refund_return_cases as rrc
    return len(rrc.cbor_encode(bytes(160)))


def serve_row_sizes():
    return sorted({1, 16, 17, 160, refund_return_wire_bytes(8)})


GUARD = 0xC3
FINALS = [(0, 0, 0), (0, 1, 1), (255, 255, 0), (6, 255, 0), (7, 255, 0), (DOUBLE_SPEND, 1, 0), (UNDETERMINED, 0, 0), (RECORDED_UNSIGNED, 1, 0), (RECORDED_UNSIGNED, 0, 1)]


def check_serve_against_the_table(sc, out_b, base_off, with_replayed, pieces, n=700, seed=5, plain=False):
    """hc_serve_return over random arrays held to serve() of this file: every byte of the output buffer (guards in front and behind), of
    status, out_key and out_replayed; rows of leaders and of lanes that are no copies stay as they are.  A copy names its leader's
    amount, that amount + l, or another one.  plain: hc_serve_plain (copy_serve_lane) held to admit_replay_unique_cases.serve, on the
    same arrays -- it answers as before"""
    r = random.Random(seed * 131 + out_b * 7 + base_off)
    lead, st, ok, rep, rows, ts = [], [], [], [], [], []
    for i in range(n):
        earlier = [j for j in range(i) if lead[j] == COPY_NONE]
        if earlier and r.random() < 0.6:
            l = r.choice(earlier)
            t = r.choice([ts[l], ts[l], (ts[l] + ELL) if ts[l] < ELL else ts[l] - ELL, (ts[l] + 1) % ELL, 0 if ts[l] % ELL else 1])
            lead.append(l); st.append(249); ok.append(KEY_NONE); rep.append(0); rows.append(bytes(out_b)); ts.append(t)
        else:
            s, k, m = r.choice(FINALS)
            lead.append(COPY_NONE); st.append(s); ok.append(k); rep.append(m); rows.append(bytes(r.randrange(1, 256) for _ in range(out_b)))
            ts.append(r.choice([0, 1, 2, 3, ELL, ELL + 2, ELL - 1, r.randrange(ELL)]))
    pad = 32
    buf = bytearray([GUARD]) * (pad + 16 + n * out_b + pad)
    raw = (C.c_ubyte * len(buf)).from_buffer(buf)
    at = pad + (-(C.addressof(raw) + pad)) % 16 + base_off
    buf[at:at + n * out_b] = b"".join(rows)
    sb, kb, rb = bytearray([GUARD] * pad + st + [GUARD] * pad), bytearray([GUARD] * pad + ok + [GUARD] * pad), bytearray([GUARD] * pad + rep + [GUARD] * pad)
    tb = bytearray(base_off) + bytearray(b"".join(t.to_bytes(32, "little") for t in ts))
    tb_before = bytes(tb)
    want_buf, want_s, want_k, want_r = bytearray(buf), bytearray(sb), bytearray(kb), bytearray(rb)
    for i in range(n):
        if lead[i] != COPY_NONE:
            l = lead[i]
            same = ts[i] % ELL == ts[l] % ELL
            want_s[pad + i], want_k[pad + i], mark, takes = aru.serve(st[l], ok[l]) if plain else serve(st[l], ok[l], same)
            if with_replayed:
                want_r[pad + i] = mark
            want_buf[at + i * out_b:at + (i + 1) * out_b] = rows[l] if takes else bytes(out_b)
    views = [(C.c_ubyte * len(b)).from_buffer(b) for b in (sb, kb, rb, tb)]
    args = [(C.c_uint32 * n)(*lead), n, out_b, C.addressof(views[0]) + pad, C.addressof(views[1]) + pad, C.addressof(raw) + at,
            C.addressof(views[2]) + pad if with_replayed else None]
    if plain:
        sc.hc_serve_plain(*args)
    else:
        sc.hc_serve_return(*args, C.addressof(views[3]) + base_off, 1 if pieces else 0)
    del raw, views
    assert buf == want_buf, (out_b, base_off, "output rows or their guards")
    assert (sb, kb, rb) == (want_s, want_k, want_r), (out_b, base_off, with_replayed)
    assert bytes(tb) == tb_before
    kinds = {(st[lead[i]], ts[i] % ELL == ts[lead[i]] % ELL) for i in range(n) if lead[i] != COPY_NONE}
    return kinds
