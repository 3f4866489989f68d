"""Shared by the tests of the two compositions partial refunds gained (tests/test_return_ring_host.py, tests/test_gpu_return_ring.py,
tests/test_gpu_return_unique.py).  Not a test module.

1. The client's RefundReturn check against a ring of issuer public keys.  Cases: the refund items of client_ring_cases.Pool (a proof
   and its PreRefund per key) signed as RefundReturn records by the model of refund_return_cases.py under ANY of the pool's keys with
   any t.  The model of the ring call is "the smallest ring index k for which refund_return_cases.to_credit_token_return(pre, params,
   pr, rec, w_k) succeeds"; where none does, the refusals in return_client_finish's order: 255 (an undecodable point: under every key),
   then 4 (no key's proof holds), then 8 (some ring key signed a t > s).
2. The return calls with the copy stage: copies_cases.model with rule 2b and ten counts, held to the model of the plain return loop."""
import ctypes as C
import os
import random
import struct
import subprocess

import admission_cases as ad
import client_ring_cases as cr
import copies_cases as cp
import pymodel as m
import refund_return_cases as rr

ROOT = cr.ROOT
ELL = cr.ELL
KEY_NONE = cr.KEY_NONE
RETURN_TOO_BIG = rr.STATUS_RETURN_TOO_BIG
RINGS = cr.RINGS


# ---- 1. the ring client ------------------------------------------------------------------------------------------------------------------
class ReturnPool:
    """RefundReturn items over the five proofs of a refund Pool.  items: [(name, prerefund, proof, 160-byte record)];
    cell(i, k) = (status, token) of the MODEL's one-key call on item i under keys[k]'s public key (k = 4: the stranger), computed when
    first asked for; table = all of them.  want: the names to sign (None: all) -- the pool at L = 128 signs the few items it uses."""

    def __init__(self, octx, h, L, tag, want=None):
        self.pool = pool = cr.Pool(octx, L, False, tag)
        self.L, self.keys, self.publics = L, pool.keys, pool.publics
        self.params = rr.params_of(h)
        self.sks = [rr.sk_of(k) for k in pool.keys]
        base = pool.items[:5]                                            # (name, prerefund, proof, refund) signed under keys 0..4
        self.parsed = [m.parse_spend_proof(it[2], L) for it in base]
        self.s = [pr.s for pr in self.parsed]
        items = []

        def sign(j, k, t, name):
            """proof j, signed under key k, returning t"""
            if want is not None and name not in want:
                return None
            e, alpha = rr.nonces_of(cr.shake("%s-%s-rr" % (tag, name), 128))
            rec = rr.refund_return(self.sks[k], self.params, self.parsed[j], t, e, alpha, verify=False)
            items.append((name, base[j][1], base[j][2], rec, j))
            return rec

        # every ring position and a key outside the ring, every t of the issue: s + 1 and l - 1 are VALIDLY signed amounts above s
        for k, kn in enumerate(("a", "b", "c", "d", "stranger")):
            s = self.s[k]
            for t, tn in ((0, "0"), (1, "1"), (s, "s"), (s + 1, "s+1"), (ELL - 1, "l-1")):
                sign(k, k, t, "%s/t=%s" % (kn, tn))
        by = {it[0]: i for i, it in enumerate(items)}
        off = 32 * (4 + L - 1)
        derived = (
            # t altered after signing: the proof fails whatever the new t says (4, not 8) -- to an amount that does not fit and to one that does
            ("b/altered to s+1", "b/t=1", lambda pre, proof, rec: (proof, rec[:128] + cr.scb(self.s[1] + 1)), True),
            ("c/altered to s", "c/t=s+1", lambda pre, proof, rec: (proof, rec[:128] + cr.scb(self.s[2])), True),
            # an undecodable A (255), also where t > s was signed: 255 comes first
            ("a/undecodable_A", "a/t=1", lambda pre, proof, rec: (proof, b"\xff" * 32 + rec[32:]), True),
            ("d/undecodable_A t=s+1", "d/t=s+1", lambda pre, proof, rec: (proof, b"\xff" * 32 + rec[32:]), True),
            # an undecodable Com_j: the model's parser refuses the proof as a whole -- 255 under every key
            ("a/undecodable_Com", "a/t=s", lambda pre, proof, rec: (proof[:off] + b"\xff" * 32 + proof[off + 32:], rec), False),
        )
        for name, src, make, parses in derived:
            if src in by:
                _, pre, proof, rec, j = items[by[src]]
                proof2, rec2 = make(pre, proof, rec)
                items.append((name, pre, proof2, rec2, j if parses else None))
        self.items = items
        self.names = [it[0] for it in items]
        self.by = {it[0]: i for i, it in enumerate(items)}
        self._memo = {}

    def cell(self, i, k):
        if (i, k) not in self._memo:
            self._memo[(i, k)] = self._one(self.items[i], k)
        return self._memo[(i, k)]

    @property
    def table(self):
        return [[self.cell(i, k) for k in range(5)] for i in range(len(self.items))]

    def _one(self, it, k):
        _, pre, proof, rec, j = it
        if j is None:
            return (255, bytes(160))
        try:
            return (0, rr.to_credit_token_return(rr.pre_of(pre), self.params, self.parsed[j], rec, self.sks[k].w).record())
        except m.ActError as err:
            return (err.code, bytes(160))

    def lanes(self, n, only=None):
        """item indices of a batch of n lanes: the items (or the subset `only`) over and over, so that the signing key rotates over the
        lanes and one wavefront holds every ring index and "no key" """
        src = list(range(len(self.items))) if only is None else list(only)
        return [src[i % len(src)] for i in range(n)]

    def zero_items(self):
        """the items whose t is 0: their first 128 bytes are plain Refunds"""
        return [i for i, it in enumerate(self.items) if it[3][128:] == bytes(32) and it[4] is not None]

    def inputs(self, idx):
        return b"".join(self.items[i][1] for i in idx), b"".join(self.items[i][2] for i in idx), b"".join(self.items[i][3] for i in idx)

    def ring_w(self, ring):
        return [self.publics[k] for k in ring]

    def expected(self, ring, idx):
        """(statuses, out_key, tokens): the smallest ring position whose one-key call accepts; otherwise 255 before 4 before 8"""
        memo = {}
        for i in set(idx):
            per = [self.cell(i, k) for k in ring]
            hit = [pos for pos, (st, _) in enumerate(per) if st == 0]
            if hit:
                memo[i] = (0, hit[0], per[hit[0]][1])
                continue
            sts = {st for st, _ in per}
            assert sts <= {m.ERR_UNDECODABLE, m.ERR_INVALID_REFUND_PROOF, m.ERR_AMOUNT_TOO_BIG}, sts
            if m.ERR_UNDECODABLE in sts:
                assert sts == {m.ERR_UNDECODABLE}
            st = m.ERR_UNDECODABLE if m.ERR_UNDECODABLE in sts else m.ERR_AMOUNT_TOO_BIG if m.ERR_AMOUNT_TOO_BIG in sts else m.ERR_INVALID_REFUND_PROOF
            memo[i] = (st, KEY_NONE, bytes(160))
        return bytes(memo[i][0] for i in idx), bytes(memo[i][1] for i in idx), b"".join(memo[i][2] for i in idx)


def build_return_ring_check(out, sanitize=False, main=False):
    """tests/hostcheck/return_ring_check.cpp -> a shared object, or (main=True) the stand-alone program that replays a case file"""
    csrc = os.path.join(ROOT, "anonymous-credit-tokens_amd", "csrc")
    hc = os.path.join(ROOT, "tests", "hostcheck")
    src = os.path.join(hc, "return_ring_check.cpp")
    deps = [src] + [os.path.join(hc, f) for f in ("hostcheck.cpp", "client_ring_check.cpp", "return_check.cpp")] + \
           [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".h", ".inc"))]
    if os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in deps):
        return out
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    kind = ["-DRETURN_RING_MAIN"] + (["-static-libasan", "-static-libubsan"] if sanitize else []) if main else ["-fPIC", "-shared"]
    subprocess.run(["g++", "-std=c++17", "-Wno-unknown-pragmas", "-Wno-psabi", *flags, *kind, "-o", out, src], check=True)
    return out


def host_ring_call(lib, h, rp, ring, idx):
    """-> (statuses, out_key, tokens, counts) of the host build over the lanes idx"""
    n, nk = len(idx), len(ring)
    pre, proofs, recs = rp.inputs(idx)
    st = C.create_string_buffer(n); ok = C.create_string_buffer(n); tok = C.create_string_buffer(160 * n)
    counts = (C.c_uint64 * 5)()
    assert lib.hc_return_ring(h, rp.L, b"".join(rp.ring_w(ring)), nk, n, pre, proofs, recs, tok, st, ok, counts) == 1
    return st.raw, ok.raw, tok.raw, list(counts)


def write_case_file(path, h, cases):
    """the case file of the stand-alone sanitizer program (return_ring_check.cpp main): cases = [(pool, ring, idx)] with the model's answers"""
    with open(path, "wb") as f:
        for rp, ring, idx in cases:
            pre, proofs, recs = rp.inputs(idx)
            st, ok, tok = rp.expected(ring, idx)
            f.write(struct.pack("<4I", 1, rp.L, len(ring), len(idx)))
            f.write(h + b"".join(rp.ring_w(ring)) + pre + proofs + recs + st + ok + tok)
        f.write(struct.pack("<I", 0))


# ---- 2. the return calls with the copy stage ---------------------------------------------------------------------------------------------
COUNTS_RETURN = ad.COUNTS + ("return_too_big",)
COUNTS_UNIQUE = COUNTS_RETURN + ("copies",)


def model_return(lanes, returned, spent, charges=None):
    """act_redeem_(cbor_)return_batch: admission_cases.model with rule 2b.  -> (statuses, out_key, counts, recorded [(k, key)],
    signed: {lane: t} of the lanes that get a record)"""
    before = frozenset(spent)
    now = set(before)
    st, ok, rec, signed = [], [], [], {}
    c = dict.fromkeys(COUNTS_RETURN, 0)
    c["lanes"] = len(lanes)
    for i, ln in enumerate(lanes):
        if ln.wire:
            st.append(ln.wire); ok.append(KEY_NONE); c["wire_rejected"] += 1; continue
        if charges is not None and ln.s % ELL != charges[i] % ELL:
            st.append(ad.WRONG_CHARGE); ok.append(KEY_NONE); c["wrong_charge"] += 1; continue
        if returned is not None and returned[i] % ELL > ln.s % ELL:           # 2b
            st.append(RETURN_TOO_BIG); ok.append(KEY_NONE); c["return_too_big"] += 1; continue
        if ln.k in before:
            st.append(ad.DOUBLE_SPEND); ok.append(KEY_NONE); c["spent_before"] += 1; continue
        c["verified"] += 1
        if ln.verdict:
            st.append(ln.verdict); ok.append(KEY_NONE); c["rejected_by_verification"] += 1; continue
        ok.append(ln.key)
        if ln.k in now:
            st.append(ad.DOUBLE_SPEND); c["double_spend_after"] += 1; continue
        now.add(ln.k); rec.append((ln.k, ln.key)); signed[i] = (returned[i] if returned is not None else 0) % ELL
        st.append(0); c["accepted"] += 1
    return st, ok, c, rec, signed


def model_unique(lanes, blobs, returned, spent, charges=None):
    """act_redeem_(cbor_)return_unique_batch: copies_cases.model with rule 2b and ten counts.  Equality is decided on blobs alone.
    -> (statuses, out_key, counts, recorded, signed, copy_of)"""
    before = frozenset(spent)
    now = set(before)
    n = len(lanes)
    st, ok, rec, copy_of, signed = [None] * n, [KEY_NONE] * n, [], [None] * n, {}
    c = dict.fromkeys(COUNTS_UNIQUE, 0)
    c["lanes"] = n
    leaders = {}
    for i, ln in enumerate(lanes):
        if ln.wire:
            st[i] = ln.wire; c["wire_rejected"] += 1; continue
        if charges is not None and ln.s % ELL != charges[i] % ELL:
            st[i] = ad.WRONG_CHARGE; c["wrong_charge"] += 1; continue
        if returned is not None and returned[i] % ELL > ln.s % ELL:           # 2b: shed, so neither a leader nor a copy
            st[i] = RETURN_TOO_BIG; c["return_too_big"] += 1; continue
        if ln.k in before:
            st[i] = ad.DOUBLE_SPEND; c["spent_before"] += 1; continue
        if blobs[i] in leaders:                                              # 3a
            copy_of[i] = leaders[blobs[i]]; c["copies"] += 1; continue
        leaders[blobs[i]] = i
        c["verified"] += 1
        if ln.verdict:
            st[i] = ln.verdict; c["rejected_by_verification"] += 1; continue
        ok[i] = ln.key
        if ln.k in now:
            st[i] = ad.DOUBLE_SPEND; c["double_spend_after"] += 1; continue
        now.add(ln.k); rec.append((ln.k, ln.key)); signed[i] = (returned[i] if returned is not None else 0) % ELL
        st[i] = 0; c["accepted"] += 1
    for i in range(n):
        if copy_of[i] is not None:
            st[i] = cp.copy_status(st[copy_of[i]]); ok[i] = ok[copy_of[i]]
    return st, ok, c, rec, signed, copy_of


def check_identities(c):
    assert c["verified"] == c["lanes"] - c["wire_rejected"] - c["wrong_charge"] - c["return_too_big"] - c["spent_before"] - c["copies"], c
    assert c["rejected_by_verification"] + c["double_spend_after"] + c["accepted"] == c["verified"], c


def check_same(lanes, blobs, returned, spent, charges):
    """the identity of the header on one batch: everything but the counts is what the plain return loop answers"""
    st, ok, c, rec, signed, copy_of = model_unique(lanes, blobs, returned, spent, charges)
    pst, pok, pc, prec, psigned = model_return(lanes, returned, spent, charges)
    assert (st, ok, rec, signed) == (pst, pok, prec, psigned)
    assert pc["verified"] == c["verified"] + c["copies"]
    assert all(pc[k] == c[k] for k in ("lanes", "wire_rejected", "wrong_charge", "return_too_big", "spent_before", "accepted"))
    check_identities(c)
    for i, l in enumerate(copy_of):
        if l is not None:
            assert l < i and blobs[l] == blobs[i] and copy_of[l] is None and i not in signed
    return st, ok, c, rec, signed, copy_of


# the fixed mixes of copies_cases (16 record lanes, 22 wire lanes; every proof spends ad.SPEND = 2) with the return lanes behind them:
# (token, proof bytes, t).  r0: a copy whose t differs from its leader's.  r1: a leader with t = s, a lane with the leader's bytes and
# t = s + 1 (shed at the screen: not a copy), and a copy with t = 0.
RETURN_LANES = [("r0", "a", 1), ("r0", "a", 2), ("r1", "a", ad.SPEND), ("r1", "a", ad.SPEND + 1), ("r1", "a", 0)]
RETURN_TOKENS = cp.FIXED_TOKENS + ("r0", "r1")
RETURN_EXPECT = [0, 3, 0, RETURN_TOO_BIG, 3]          # written down by hand
RETURN_KEYS = [0, 0, 0, 255, 0]
RETURN_COPY_OF = [None, 0, None, None, 2]             # relative to the first return lane
RETURN_SIGNED = {0: 1, 2: ad.SPEND}                   # relative lane -> the t its record carries


def fixed_returned(n_base):
    """the returned amounts of the lanes of the copies mix: amounts that fit, different from lane to lane"""
    return [i % (ad.SPEND + 1) for i in range(n_base)]


def fixed_lanes(wire):
    """-> (lanes, blobs, charges, returned, base) of the extended fixed mix over token NAMES; base = the first return lane"""
    lanes, blobs, charges = cp.fixed_lanes(wire)
    base = len(lanes)
    returned = fixed_returned(base)
    for tok, proof, t in RETURN_LANES:
        lanes.append(ad.Lane(tok, ad.SPEND, 0, 0, 0)); blobs.append((tok, proof)); charges.append(ad.SPEND); returned.append(t)
    return lanes, blobs, charges, returned, base


def fixed_expect(wire):
    """hand-written: (statuses, out_key, copy_of, counts) of the extended mix"""
    n0 = len(cp.FIXED_MIX) + (len(cp.FIXED_WIRE_EXTRA) if wire else 0)
    c = dict(cp.FIXED_COUNTS_WIRE if wire else cp.FIXED_COUNTS_RECORDS)
    c.update(lanes=c["lanes"] + 5, return_too_big=1, copies=c["copies"] + 2, verified=c["verified"] + 2, accepted=c["accepted"] + 2)
    copy_of = cp.FIXED_COPY_OF[:n0] + [None if x is None else n0 + x for x in RETURN_COPY_OF]
    return cp.FIXED_EXPECT[:n0] + RETURN_EXPECT, cp.FIXED_KEYS[:n0] + RETURN_KEYS, copy_of, c


def check_model_on_fixed_mix():
    for wire in (False, True):
        lanes, blobs, charges, returned, base = fixed_lanes(wire)
        st, ok, c, rec, signed, copy_of = check_same(lanes, blobs, returned, set(cp.FIXED_SPENT), charges)
        est, eok, ecopy, ec = fixed_expect(wire)
        assert (st, ok, copy_of) == (est, eok, ecopy), (wire, st, ok, copy_of)
        assert c == ec, (wire, c, ec)
        assert {i - base: t for i, t in signed.items() if i >= base} == RETURN_SIGNED
        # nothing returned: the model of the admission unique forms
        ust, uok, uc, urec, ucopy = cp.model(lanes, blobs, set(cp.FIXED_SPENT), charges)
        st0, ok0, c0, rec0, _, copy0 = model_unique(lanes, blobs, None, set(cp.FIXED_SPENT), charges)
        assert (st0, ok0, rec0, copy0) == (ust, uok, urec, ucopy) and {k: v for k, v in c0.items() if k != "return_too_big"} == uc and c0["return_too_big"] == 0


PLAN_NS = (65, 300)


def plan_returned(plan, seed):
    """an amount per lane of a copies plan: mostly one that fits (a copy's differs from its leader's as often as not), one lane in
    sixteen returns one credit too many"""
    r = random.Random(seed * 7919 + len(plan))
    return [ad.SPEND + 1 if r.random() < 1 / 16 else r.randrange(ad.SPEND + 1) for _ in plan]


def check_model_on_plans():
    for n in PLAN_NS:
        for num, den in cp.FRACTIONS:
            for with_charges in (False, True):
                plan, tokens = cp.copy_plan(n, num, den, cp.plan_seed(num, den), with_charges)
                lanes, blobs, charges, spent = cp.plan_lanes(plan)
                returned = plan_returned(plan, cp.plan_seed(num, den))
                st, ok, c, rec, signed, copy_of = check_same(lanes, blobs, returned, spent, charges if with_charges else None)
                assert tokens <= n and (c["copies"] == 0) == (num == 0 or not any(x is not None for x in copy_of))
                if num:
                    assert c["copies"] > 0 and c["return_too_big"] > 0
                    # copies whose amount differs from their leader's are there, and so are lanes with a leader's bytes that were shed
                    assert any(l is not None and returned[i] != returned[l] for i, l in enumerate(copy_of))
