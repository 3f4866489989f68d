"""Shared by the tests of the replay unique forms (tests/test_admit_replay_unique_host.py, tests/test_gpu_admit_replay_unique.py,
tools/admit_replay_copies_probe.py): the loop of act_redeem_(cbor_)admit_replay_unique_batch as a model over labels and input-byte
identities, built on the models of admit_replay_cases (the screen and the receipts) and replay_cases (the tail); the fixed lane mix of
the feature with HAND-WRITTEN expectations; the seeded lane plans of the equality runs; and the host build of the serve pass
(tests/hostcheck/copy_serve_check.cpp) as a library and as a stand-alone sanitized program.  Not a test module."""
import ctypes as C
import os
import random
import subprocess
from collections import namedtuple

import admit_replay_cases as ar
import copies_cases as cp
import replay_cases as rp

ROOT = ar.ROOT
KEY_NONE, DOUBLE_SPEND, WRONG_CHARGE = ar.KEY_NONE, ar.DOUBLE_SPEND, ar.WRONG_CHARGE
UNDETERMINED, RECORDED_UNSIGNED = rp.UNDETERMINED, rp.RECORDED_UNSIGNED
COPY_NONE = cp.COPY_NONE
COUNTS = ar.COUNTS + ("copies", "copies_served")


def serve(leader_status, leader_key):
    """the table of the header, written out: (status, out_key, replayed, takes the leader's record) of a copy"""
    if leader_status == 0:
        return 0, leader_key, 1, True
    assert leader_status in (255, 6, 7, DOUBLE_SPEND, UNDETERMINED, RECORDED_UNSIGNED)
    return leader_status, leader_key, 0, False


def model(lanes, blobs, spent: set, receipts: set, charges=None):
    """The admit-replay loop of the header with the copy step.  blobs[i]: the identity of lane i's input bytes (any hashable; equal iff
    the bytes are).  Mutates `spent` and `receipts` as the tail does.
    -> (statuses, out_key, replayed, counts with copies and copies_served, copy_of: the leader's lane or None)"""
    before, had = frozenset(spent), frozenset(receipts)
    n = len(lanes)
    st, ok, rep, copy_of = [None] * n, [KEY_NONE] * n, [0] * n, [None] * n
    c = dict.fromkeys(COUNTS, 0)
    c["lanes"] = n
    go, leaders = [], {}
    for i, ln in enumerate(lanes):
        if ln.wire:
            st[i] = ln.wire; c["wire_rejected"] += 1; continue
        if charges is not None and ln.s % ar.ELL != charges[i] % ar.ELL:
            st[i] = WRONG_CHARGE; c["wrong_charge"] += 1; continue
        if ln.k in before:
            pre, cand = ar.decide(DOUBLE_SPEND, True, not ln.com_ok, (ln.k, ln.kprime) in had)
            if pre:
                st[i] = pre; c["foreign_spend"] += 1; continue
            c["retry_candidates"] += cand                               # (counted at the screen: a candidate that is a copy too)
        if blobs[i] in leaders:                                         # the bytes of an earlier lane that passed steps 1-3
            copy_of[i] = leaders[blobs[i]]; c["copies"] += 1; continue
        leaders[blobs[i]] = i
        go.append(i)
    c["verified"] = len(go)
    mst, mok, mrep, mc = rp.model([rp.Lane(lanes[i].k, lanes[i].kprime, lanes[i].verdict, lanes[i].key) for i in go], spent, receipts)
    for j, i in enumerate(go):
        st[i], ok[i], rep[i] = mst[j], mok[j], mrep[j]
    c.update(rejected_by_verification=mc["rejected_by_verification"], fresh=mc["fresh"], replayed=mc["replayed"], double_spend_after=mc["double_spend"],
             unanswered=mc["unanswered"])
    for i in range(n):
        if copy_of[i] is not None:
            st[i], ok[i], rep[i], served = serve(st[copy_of[i]], ok[copy_of[i]])
            c["copies_served"] += served
    return st, ok, rep, c, copy_of


def check_identities(c):
    assert c["verified"] == c["lanes"] - c["wire_rejected"] - c["wrong_charge"] - c["foreign_spend"] - c["copies"], c
    assert c["rejected_by_verification"] + c["fresh"] + c["replayed"] + c["double_spend_after"] + c["unanswered"] == c["verified"], c
    assert c["copies_served"] <= c["copies"], c


def check_against_the_plain_form(lanes, blobs, spent, receipts, charges=None):
    """the theorem on the models: statuses, out_key, replay marks and both sets are those of admit_replay_cases.model; the counts
    are related as the header says.  -> the unique model's output"""
    s1, r1, s2, r2 = set(spent), set(receipts), set(spent), set(receipts)
    st, ok, rep, c, copy_of = model(lanes, blobs, s1, r1, charges)
    pst, pok, prep, pc = ar.model(lanes, s2, r2, charges)
    assert (st, ok, rep) == (pst, pok, prep) and (s1, r1) == (s2, r2)
    check_identities(c)
    check_count_relation(c, pc, st, copy_of)
    return st, ok, rep, c, copy_of


def check_count_relation(c, pc, st, copy_of):
    """c: the unique form's counts, pc: the plain form's on the same batch, st: the (common) final statuses"""
    assert all(c[k] == pc[k] for k in ("lanes", "wire_rejected", "wrong_charge", "foreign_spend", "retry_candidates", "fresh")), (c, pc)
    assert pc["verified"] - c["verified"] == c["copies"] == sum(1 for l in copy_of if l is not None)
    served = sum(1 for i, l in enumerate(copy_of) if l is not None and st[i] == 0)
    assert c["copies_served"] == served and pc["replayed"] - c["replayed"] == served
    for name, codes in (("rejected_by_verification", (255, 6, 7)), ("double_spend_after", (DOUBLE_SPEND,)), ("unanswered", (UNDETERMINED, RECORDED_UNSIGNED))):
        assert pc[name] - c[name] == sum(1 for i, l in enumerate(copy_of) if l is not None and st[i] in codes), name


# ---- the fixed lane mix (the table of the feature), hand-written ------------------------------------------------------------------------
# (token, proof: which bytes -- lanes with one (token, proof) pair are byte-identical, verdict by construction, charge is the expected
# one).  a / b are the two proofs of a token (one nullifier, another K'), x the tampered a.  Tokens "sp*" were redeemed before the call
# with proof a, so `receipts` holds their (k, a).  Token NAMES map to tokens whose issuer key is ring index FIXED_OWNER[name].
FIXED_MIX = [
    ("t0", "a", 0, True), ("t0", "a", 0, True), ("t0", "a", 0, True),          # a. a fresh proof, then two copies of it
    ("sp0", "a", 0, True), ("sp0", "a", 0, True),                              # b. a retry candidate, then a copy
    ("sp1", "b", 0, True), ("sp1", "b", 0, True),                              # c. a foreign spend twice: shed by the screen, never copies
    ("t1", "x", 7, True), ("t1", "x", 7, True),                                # d. a tampered fresh proof and its copy
    ("t2", "a", 0, True), ("t2", "b", 0, True), ("t2", "b", 0, True),          # e. two proofs of one token, then a copy of the second
    ("t3", "a", 0, False), ("t3", "a", 0, False),                              # f. a wrong-charge lane twice
]
# g. wire only: a respelled copy of (a), and (a) with one trailing byte: other bytes, so both are verified -- and replayed
FIXED_WIRE_EXTRA = [("t0", "a/respelled", 0, True), ("t0", "a/trailing", 0, True)]
FIXED_TOKENS = ("t0", "t1", "t2", "t3", "sp0", "sp1")
FIXED_OWNER = dict(t0=0, t1=1, t2=0, t3=1, sp0=0, sp1=1)
FIXED_SPENT = ("sp0", "sp1")
N_RECORD_LANES = 14
SPEND, EXPECTED_WRONG = 3, 4
# written down by hand from the issue's table, not computed
FIXED_EXPECT = [0, 0, 0, 0, 0, 3, 3, 7, 7, 0, 3, 3, 250, 250] + [0, 0]
FIXED_KEYS = [0, 0, 0, 0, 0, 255, 255, 255, 255, 0, 0, 0, 255, 255] + [0, 0]
FIXED_REPLAYED = [0, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0] + [1, 1]
FIXED_COPY_OF = [None, 0, 0, None, 3, None, None, None, 7, None, None, 10, None, None] + [None, None]
FIXED_COUNTS_RECORDS = dict(lanes=14, wire_rejected=0, wrong_charge=2, foreign_spend=2, retry_candidates=2, verified=5, rejected_by_verification=1, fresh=2, replayed=1,
                            double_spend_after=1, unanswered=0, copies=5, copies_served=3)
FIXED_COUNTS_WIRE = dict(lanes=16, wire_rejected=0, wrong_charge=2, foreign_spend=2, retry_candidates=2, verified=7, rejected_by_verification=1, fresh=2, replayed=3,
                         double_spend_after=1, unanswered=0, copies=5, copies_served=3)


def fixed_lanes(wire):
    """-> (lanes, blobs, charges, spent, receipts) of the fixed mix over token NAMES"""
    mix = FIXED_MIX + (FIXED_WIRE_EXTRA if wire else [])
    # K' is that of proof a or b: the tampered byte of x and the spelling of a message are outside k and Com
    lanes = [ar.Lane(tok, (tok, "b" if proof[0] == "b" else "a"), verdict, KEY_NONE if verdict else FIXED_OWNER[tok], SPEND) for tok, proof, verdict, _ in mix]
    blobs = [(tok, proof) for tok, proof, _, _ in mix]
    charges = [SPEND if right else EXPECTED_WRONG for _, _, _, right in mix]
    return lanes, blobs, charges, set(FIXED_SPENT), {(k, (k, "a")) for k in FIXED_SPENT}


def check_model_on_fixed_mix():
    for wire in (False, True):
        lanes, blobs, charges, spent, receipts = fixed_lanes(wire)
        n = len(lanes)
        st, ok, rep, c, copy_of = check_against_the_plain_form(lanes, blobs, spent, receipts, charges)
        assert (st, ok, rep, copy_of) == (FIXED_EXPECT[:n], FIXED_KEYS[:n], FIXED_REPLAYED[:n], FIXED_COPY_OF[:n]), (wire, st, ok, rep, copy_of)
        assert c == (FIXED_COUNTS_WIRE if wire else FIXED_COUNTS_RECORDS), (wire, c)
    assert N_RECORD_LANES == len(FIXED_MIX)


# ---- the seeded plans of the equality runs ------------------------------------------------------------------------------------------------
PLAN_N = 2 * 4096 + 17
FRACTIONS = ((1, 2), (7, 8))
# token: which token the lane spends; variant: which of its two proofs; tampered; spent: the token was redeemed before the call with
# variant 0 (variant 0 is then a retry, variant 1 a foreign spend); wrong: the lane is asked the wrong charge (only with charges);
# copy_of: the earlier lane whose bytes this lane repeats, or None
PlanLane = namedtuple("PlanLane", "token variant tampered spent wrong copy_of")
# what a lane that repeats nobody's bytes is, in turn: v a fresh valid proof, t a tampered one, r a retry (spent, its own receipt), d the
# OTHER proof of the last valid token (verified, then a double spend behind verification), s a foreign spend, w a valid proof asked the
# wrong charge.  At 7/8 one lane in eight is left for these and fresh and rejected lanes must each be half of them, so retries and second
# proofs come only at the start -- their copies are many because a repeat picks the KIND of its source first (REPEAT_KINDS) and the lane second.
CYCLE = ("v", "t", "r", "d", "v", "t", "s", "w")
HEAD_7_8 = ("v", "t", "r", "d") * 6
CYCLE_7_8 = ("v", "t")
REPEAT_KINDS = ("v",) * 5 + ("r",) * 5 + ("t",) * 5 + ("d", "s")


def copy_plan(n, num, den, seed, with_charges):
    r = random.Random(seed * 1000003 + num * 101 + den)
    seven = (num, den) == (7, 8)
    plan, by_kind, tok, turn, last_valid = [], {}, 0, 0, None
    for i in range(n):
        if by_kind and r.random() * den < num:
            kind = r.choice(REPEAT_KINDS)
            if kind not in by_kind:
                kind = r.choice(sorted(by_kind))
            src = r.choice(by_kind[kind])
            p = plan[src]
            # the bytes of lane src; the charge belongs to the lane: now and then a repeat is asked the wrong one
            wrong = with_charges and (r.random() < 1 / 16 if not p.wrong else r.random() < 1 / 2)
            plan.append(PlanLane(p.token, p.variant, p.tampered, p.spent, wrong, src))
            continue
        kind = HEAD_7_8[turn] if seven and turn < len(HEAD_7_8) else (CYCLE_7_8 if seven else CYCLE)[turn % (2 if seven else len(CYCLE))]
        turn += 1
        if kind == "d" and last_valid is None:
            kind = "v"
        if kind == "d":
            plan.append(PlanLane(last_valid, 1, False, False, False, None)); last_valid = None
        else:
            plan.append(PlanLane(tok, 1 if kind == "s" else 0, kind == "t", kind in ("r", "s"), with_charges and kind == "w", None))
            if kind == "v":
                last_valid = tok
            tok += 1
        by_kind.setdefault(kind, []).append(i)
    return plan, tok


def plan_lanes(plan, nullifier=lambda t: t, key=lambda p: p.token % 2):
    """-> (model lanes, blobs, charges, spent set, receipts set) of a plan; token t was issued under ring index key(p)"""
    lanes = [ar.Lane(nullifier(p.token), (p.token, p.variant), 7 if p.tampered else 0, KEY_NONE if p.tampered else key(p), SPEND) for p in plan]
    blobs = [(p.token, p.variant, p.tampered) for p in plan]
    charges = [SPEND + 1 if p.wrong else SPEND for p in plan]
    spent = {nullifier(p.token) for p in plan if p.spent}
    receipts = {(nullifier(p.token), (p.token, 0)) for p in plan if p.spent}
    return lanes, blobs, charges, spent, receipts


CATEGORIES = ("served_copies_of_fresh", "served_copies_of_retries", "copies_of_rejected", "verified_fresh", "verified_rejected")
MIN_COPIES_OF_DOUBLE_SPENDS = 16


def categories_of(st, rep, copy_of):
    """from final statuses, replay marks and each copy's leader -> (the five shares' counts, copies of leaders that ended DOUBLE_SPEND
    behind verification)"""
    n = len(st)
    lead_ok = lambda i: copy_of[i] is not None and st[copy_of[i]] == 0
    cats = dict(served_copies_of_fresh=sum(1 for i in range(n) if lead_ok(i) and rep[copy_of[i]] == 0),
                served_copies_of_retries=sum(1 for i in range(n) if lead_ok(i) and rep[copy_of[i]] == 1),
                copies_of_rejected=sum(1 for i in range(n) if copy_of[i] is not None and st[copy_of[i]] in (255, 6, 7)),
                verified_fresh=sum(1 for i in range(n) if copy_of[i] is None and st[i] == 0 and rep[i] == 0),
                verified_rejected=sum(1 for i in range(n) if copy_of[i] is None and st[i] in (255, 6, 7)))
    return cats, sum(1 for i in range(n) if copy_of[i] is not None and st[copy_of[i]] == DOUBLE_SPEND)


def plan_categories(plan, with_charges):
    lanes, blobs, charges, spent, receipts = plan_lanes(plan)
    st, ok, rep, c, copy_of = model(lanes, blobs, spent, receipts, charges if with_charges else None)
    cats, ds = categories_of(st, rep, copy_of)
    return cats, ds, c


def categories_are_full(cats, ds, n):
    return all(16 * cats[k] >= n for k in CATEGORIES) and ds >= MIN_COPIES_OF_DOUBLE_SPENDS


def plan_is_mixed_enough(n, num, den, seed):
    for with_charges in (False, True):
        plan, _ = copy_plan(n, num, den, seed, with_charges)
        cats, ds, _ = plan_categories(plan, with_charges)
        if not categories_are_full(cats, ds, n):
            return False
    return True


def find_seed(n, num, den, limit=200):
    for seed in range(1, limit):
        if plan_is_mixed_enough(n, num, den, seed):
            return seed
    raise AssertionError("no seed below %d fills every category at %d/%d" % (limit, num, den))


# chosen on the CPU (tests/test_admit_replay_unique_host.py asserts it): the smallest seed with which each of the five categories holds
# at least 1/16 of the lanes and at least 16 lanes copy a leader that ends DOUBLE_SPEND behind verification, with and without charges
PLAN_SEEDS = {(1, 2): 1, (7, 8): 16}


def plan_seed(num, den):
    return PLAN_SEEDS[(num, den)]


def check_model_on_plans():
    """the unique model against admit_replay_cases.model, lane for lane and set for set, on every seeded plan"""
    for (num, den) in FRACTIONS:
        for with_charges in (False, True):
            plan, tokens = copy_plan(PLAN_N, num, den, plan_seed(num, den), with_charges)
            lanes, blobs, charges, spent, receipts = plan_lanes(plan)
            st, ok, rep, c, copy_of = check_against_the_plain_form(lanes, blobs, spent, receipts, charges if with_charges else None)
            repeats = sum(1 for p in plan if p.copy_of is not None)
            assert abs(repeats / PLAN_N - num / den) < 0.02 and 0 < c["copies"] <= repeats and tokens <= PLAN_N, (num, den, repeats, c)
            for i, l in enumerate(copy_of):                             # a copy's leader is an earlier lane with the same bytes that is no copy itself
                if l is not None:
                    assert l < i and blobs[l] == blobs[i] and copy_of[l] is None


# ---- host build of the serve pass -----------------------------------------------------------------------------------------------------------
def _build(out, extra):
    csrc = os.path.join(ROOT, "anonymous-credit-tokens_amd", "csrc")
    src = os.path.join(ROOT, "tests", "hostcheck", "copy_serve_check.cpp")
    deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".h", ".inc"))]
    if os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in deps):
        return out
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-Wno-psabi", *extra, "-o", out, src], check=True)
    return out


def build_serve_check(out):
    """csrc/copy_lanes.h compiled with g++ into a small library"""
    return _build(out, ["-O2", "-fPIC", "-shared"])


def build_serve_program(out):
    """the same file with its own main, under AddressSanitizer and UBSan: a stand-alone program with the sanitizers' runtimes linked in,
    so that nothing has to be preloaded"""
    return _build(out, ["-O1", "-g", "-DCOPY_SERVE_CHECK_MAIN", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer"])


def load_serve_check(path):
    sc = C.CDLL(path)
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    sc.hc_copy_serve.argtypes = [vp, u32, u64, vp, vp, vp, vp, C.c_int]; sc.hc_copy_serve.restype = None
    sc.hc_copy_serve_checks.argtypes = [vp, u32]; sc.hc_copy_serve_checks.restype = C.c_int
    sc.hc_copy_serve_field_ops.argtypes = []; sc.hc_copy_serve_field_ops.restype = u64
    return sc


def refund_wire_bytes(L):
    """act_cbor_size(ctx, ACT_CBOR_REFUND) at L, from the reference codec"""
    import pymodel
    return len(pymodel.cbor_encode("Refund", bytes(128), L))


def serve_row_sizes():
    return sorted({1, 16, 17, 128, refund_wire_bytes(8), refund_wire_bytes(128)})


GUARD = 0xC3


def check_serve_against_the_table(sc, out_b, base_off, with_replayed, pieces, n=700, seed=5):
    """hc_copy_serve over random arrays held to serve() of this file: every byte of the output buffer (guards in front and behind), of
    status, out_key and out_replayed"""
    r = random.Random(seed * 131 + out_b * 7 + base_off)
    finals = [(0, 0, 0), (0, 1, 1), (255, 255, 0), (6, 255, 0), (7, 255, 0), (DOUBLE_SPEND, 1, 0), (UNDETERMINED, 0, 0), (RECORDED_UNSIGNED, 1, 0)]
    lead, st, ok, rep, rows = [], [], [], [], []
    for i in range(n):
        earlier = [j for j in range(i) if lead[j] == COPY_NONE]
        if earlier and r.random() < 0.6:
            lead.append(r.choice(earlier)); st.append(249); ok.append(KEY_NONE); rep.append(0); rows.append(bytes(out_b))
        else:
            s, k, m = r.choice(finals)
            lead.append(COPY_NONE); st.append(s); ok.append(k); rep.append(m); rows.append(bytes(r.randrange(1, 256) for _ in range(out_b)))
    pad = 32
    buf = bytearray([GUARD]) * (pad + 16 + n * out_b + pad)
    raw = (C.c_ubyte * len(buf)).from_buffer(buf)
    at = pad + (-(C.addressof(raw) + pad)) % 16 + base_off
    buf[at:at + n * out_b] = b"".join(rows)
    sb, kb, rb = bytearray([GUARD] * pad + st + [GUARD] * pad), bytearray([GUARD] * pad + ok + [GUARD] * pad), bytearray([GUARD] * pad + rep + [GUARD] * pad)
    want_buf, want_s, want_k, want_r = bytearray(buf), bytearray(sb), bytearray(kb), bytearray(rb)
    for i in range(n):
        if lead[i] != COPY_NONE:
            l = lead[i]
            want_s[pad + i], want_k[pad + i], mark, takes = serve(st[l], ok[l])
            if with_replayed:
                want_r[pad + i] = mark
            want_buf[at + i * out_b:at + (i + 1) * out_b] = rows[l] if takes else bytes(out_b)
    views = [(C.c_ubyte * len(b)).from_buffer(b) for b in (sb, kb, rb)]
    sc.hc_copy_serve((C.c_uint32 * n)(*lead), n, out_b, C.addressof(views[0]) + pad, C.addressof(views[1]) + pad, C.addressof(raw) + at,
                     C.addressof(views[2]) + pad if with_replayed else None, 1 if pieces else 0)
    del raw, views
    assert buf == want_buf, (out_b, base_off, "output rows or their guards")
    assert (sb, kb, rb) == (want_s, want_k, want_r), (out_b, base_off, with_replayed)
