"""Partial refunds on the GPU: act_redeem_return_batch / act_redeem_cbor_return_batch, act_refund_sign_return_keyring_batch
and act_refund_to_credit_token_return_batch through the C ABI.  With nothing returned they are held to act_redeem_(cbor_)admit_batch and
act_refund_to_credit_token_batch byte for byte; with t != 0 to the model of tests/refund_return_cases.py under the same nonces.  Proofs
come from the engine's prover at L = 8 (one case at L = 128).  Every step runs under a time limit of its own.

Sizes: 1 and 3 are tiny calls, 64 and 65 straddle the 64-lane kernels (and the client's one-launch form, which ends at 64), 300
straddles the 256-lane ones.  The client's third road (one lane per item, taken above 8 192 items) is walked with the A/B knobs."""
import numpy as np
import pytest

import pymodel as m
import refund_return_cases as rr
from conftest import ELL, shake, scb
from test_gpu_admission import Dev, _pairs, call_admit, step

pytestmark = pytest.mark.gpu

L = 8
CREDIT = 9
SIZES = (1, 3, 64, 65, 300)
N_MAX = 300


def spend_of(i):
    return 3 + i % 3


class World:
    """two keys; token i is issued under keys[i % 2] for CREDIT and has one proof that spends spend_of(i)"""

    def __init__(self, eng, tag, n, L=L):
        self.eng, self.pb, self.n, self.L = eng, eng.proof_bytes, n, L
        self.keys = [eng.private_key_random(shake("%s-sk%d" % (tag, i), 64)) for i in range(2)]
        pre = eng.pre_issuance_random(shake(tag + "-pre", 128 * n)); req = eng.request(pre, shake(tag + "-rq", 128 * n))
        tok = np.zeros((n, 160), np.uint8)
        for k in range(2):
            sel = list(range(k, n, 2))
            if not sel:
                continue
            rq = b"".join(req[128 * i:128 * i + 128] for i in sel); pr = b"".join(pre[64 * i:64 * i + 64] for i in sel)
            st, resp = eng.issue(self.keys[k], rq, scb(CREDIT) * len(sel), shake("%s-ir%d" % (tag, k), 128 * len(sel)))
            assert st == bytes(len(sel))
            st, t = eng.issuance_to_credit_token(pr, self.keys[k][32:], rq, resp)
            assert st == bytes(len(sel))
            tok[sel] = np.frombuffer(t, np.uint8).reshape(len(sel), 160)
        self.s = [spend_of(i) for i in range(n)]
        st, p, prer = eng.prove_spend_seeded(tok.tobytes(), b"".join(scb(s) for s in self.s), shake(tag + "-seed", 32))
        assert st == bytes(n)
        self.proofs = [p[self.pb * i:self.pb * i + self.pb] for i in range(n)]
        self.prer = [prer[96 * i:96 * i + 96] for i in range(n)]
        self.k = [self.proofs[i][:32] for i in range(n)]
        self._parsed = {}

    def parsed(self, i):
        if i not in self._parsed:
            self._parsed[i] = m.parse_spend_proof(self.proofs[i], self.L)
        return self._parsed[i]


_worlds = {}


def world(eng, tag, n, L=L):
    key = (id(eng), tag)
    if key not in _worlds:
        _worlds[key] = World(eng, tag, n, L)
    return _worlds[key]


def call_return(eng, mem, ns, ring, n, blob=None, msgs=None, charges=None, returned=None, rng=b"", rng_mode=0, sign_key=-1, key_epochs=None):
    """one return call in either memory kind and either form -> (statuses, out bytes, out_key, counts)"""
    from act_amd import capi
    wire = msgs is not None
    ob = eng.cbor_size("RefundReturn") if wire else 160
    if mem == "host":
        if wire:
            st, out, ok, c = eng.redeem_cbor_return(ns, ring, msgs, rng, rng_mode, sign_key, charges, returned, key_epochs)
            return st, b"".join(x if x else bytes(ob) for x in out), ok, c
        return eng.redeem_return(ns, ring, blob, rng, rng_mode, sign_key, charges, returned, key_epochs)
    d = Dev()
    src = d.up(b"".join(msgs) if wire else blob)
    offs = np.zeros(n + 1, np.uint64)
    if wire:
        offs[1:] = np.cumsum([len(x) for x in msgs], dtype=np.uint64)
    dc = d.up(charges) if charges is not None else None
    dt = d.up(returned) if returned is not None else None
    dr = None if isinstance(rng, capi.ReplayRng) else d.up(rng)
    out, st, ok = d.new(ob * n, 7), d.new(n, 99), d.new(n, 77)
    d.t.cuda.synchronize()
    p = dict(set=ns, charges=dc.data_ptr() if dc is not None else None, returned=dt.data_ptr() if dt is not None else None,
             rng=rng.ptr if dr is None else dr.data_ptr(), rng_mode=rng_mode, out=out.data_ptr(), status=st.data_ptr(), out_key=ok.data_ptr(),
             key_epochs=key_epochs, sign_key=sign_key)
    if wire:
        c = eng.return_ptr("redeem_cbor", ring, n, capi.MEM_DEVICE, cbor=src.data_ptr(), offsets=offs.ctypes.data, **p)
    else:
        c = eng.return_ptr("redeem", ring, n, capi.MEM_DEVICE, proofs=src.data_ptr(), **p)
    return d.down(st, n), d.down(out, ob * n), d.down(ok, n), c


def records_of(eng, wire, out, n):
    """the 160-byte records of a return call's output (wire: every signed message decoded as type 10; an unsigned slot is all zero)"""
    if not wire:
        return out
    ml = eng.cbor_size("RefundReturn")
    msgs = [out[ml * i:ml * i + ml] for i in range(n)]
    live = [i for i in range(n) if any(msgs[i])]
    recs = [bytes(160)] * n
    if live:
        st, dec = eng.cbor_decode("RefundReturn", [msgs[i] for i in live])
        assert st == bytes(len(live))
        for j, i in enumerate(live):
            recs[i] = dec[160 * j:160 * j + 160]
            assert msgs[i] == rr.cbor_encode(recs[i])          # canonical: the model's bytes
    return b"".join(recs)


def refunds_of(eng, wire, out, n):
    if not wire:
        return out
    ml = eng.cbor_size("Refund")
    msgs = [out[ml * i:ml * i + ml] for i in range(n)]
    live = [i for i in range(n) if any(msgs[i])]
    recs = [bytes(128)] * n
    if live:
        st, dec = eng.cbor_decode("Refund", [msgs[i] for i in live])
        assert st == bytes(len(live))
        for j, i in enumerate(live):
            recs[i] = dec[128 * j:128 * j + 128]
    return b"".join(recs)


def mixed_batch(w, n):
    """-> (records, charges, the nullifiers spent before): one tampered proof, one replayed nullifier and one wrong charge where n allows"""
    recs = [w.proofs[i] for i in range(n)]
    charges = [w.s[i] for i in range(n)]
    before = []
    if n >= 3:
        bad = bytearray(recs[0]); bad[w.pb - 32] ^= 1; recs[0] = bytes(bad)
        before = [w.k[1]]
        charges[2] += 1
    return recs, b"".join(scb(c) for c in charges), before


# ---- 4. the identity at t = 0 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_nothing_returned_is_the_admission_call(engine_factory, bench_params, n):
    from act_amd import capi
    eng = engine_factory(bench_params, L, max_batch=4096, transcript=capi.TRANSCRIPT_DEVICE)
    with step(240, "tokens and proofs"):
        w = world(eng, "rr-id", N_MAX)
    recs, charges, before = mixed_batch(w, n)
    rng = shake("rr-id-rng-%d" % n, 128 * n)
    combos = [(mem, wire, ring_idx, mode) for mem in ("host", "device") for wire in (False, True) for ring_idx in ((0,), (1, 0))
              for mode in (capi.RNG_SEQUENTIAL, capi.RNG_PER_LANE)]
    combos = [c for c in combos if c[0] == "host" or n in (65, 300)] + [("host", False, (1, 0), capi.RNG_CALLBACK)]
    for mem, wire, ring_idx, mode in combos:
        ring = [w.keys[k] for k in ring_idx]
        epochs = [100 + k for k in ring_idx] if len(ring_idx) > 1 else None
        kw = dict(msgs=eng.cbor_encode("SpendProof", b"".join(recs))) if wire else dict(blob=b"".join(recs))
        sets = [capi.NullifierSet(1000, salt=b"\x09" * 16) for _ in range(3)]
        for s in sets:
            if before:
                assert s.check_and_insert(b"".join(before)) == bytes(len(before))
        gens = [capi.ReplayRng(rng) for _ in range(3)] if mode == capi.RNG_CALLBACK else [rng] * 3
        with step(120, "n %d %s wire %d ring %s rng %d" % (n, mem, wire, ring_idx, mode)):
            rc, ast, aout, aok, ac = call_admit(eng, mem, sets[0], ring, n, charges=charges, rng=gens[0], rng_mode=mode, key_epochs=epochs, **kw)
            st0, out0, ok0, c0 = call_return(eng, mem, sets[1], ring, n, charges=charges, returned=None, rng=gens[1], rng_mode=mode, key_epochs=epochs, **kw)
            st1, out1, ok1, c1 = call_return(eng, mem, sets[2], ring, n, charges=charges, returned=bytes(32 * n), rng=gens[2], rng_mode=mode, key_epochs=epochs, **kw)
        what = (n, mem, wire, ring_idx, mode)
        assert st0 == st1 == ast and ok0 == ok1 == aok, what
        assert c0 == c1 and {k: v for k, v in c0.items() if k != "return_too_big"} == ac and c0["return_too_big"] == 0, what
        assert _pairs(sets[0]) == _pairs(sets[1]) == _pairs(sets[2]), what
        want = refunds_of(eng, wire, aout, n)
        for out in (out0, out1):
            got = records_of(eng, wire, out, n)
            for i in range(n):
                assert got[160 * i:160 * i + 128] == want[128 * i:128 * i + 128] and got[160 * i + 128:160 * i + 160] == bytes(32), (what, i)
                assert any(got[160 * i:160 * i + 160]) == (ast[i] == 0)
        if mode == capi.RNG_CALLBACK:
            assert gens[0].draws == gens[1].draws == gens[2].draws and gens[0].pos == gens[1].pos == gens[2].pos
        if n >= 3:
            assert (ast[0], ast[1], ast[2]) == (7, 3, 250), what
        if len(ring_idx) == 2:                                      # (under key 0 alone the tokens of key 1 do not verify)
            assert ac["accepted"] == (n - 3 if n >= 3 else n), what
        for s in sets:
            s.close()
    # the client: a record that returns nothing gives the token the existing call gives
    ring = [w.keys[1], w.keys[0]]
    ns = capi.NullifierSet(1000)
    with step(120, "client"):
        st, out, ok, _ = call_return(eng, "host", ns, ring, n, blob=b"".join(w.proofs[:n]), rng=rng, rng_mode=capi.RNG_PER_LANE, sign_key=1)
        assert st == bytes(n)
        pre, proofs = b"".join(w.prer[:n]), b"".join(w.proofs[:n])
        cst, tok = eng.refund_to_credit_token_return(pre, proofs, out, w.keys[0][32:])
        ost, otok = eng.refund_to_credit_token(pre, proofs, b"".join(out[160 * i:160 * i + 128] for i in range(n)), w.keys[0][32:])
    assert cst == ost == bytes(n) and tok == otok
    ns.close()
    assert eng.secret_residue() == 0


# ---- 5. t != 0 against the model ------------------------------------------------------------------------------------------------------------
def returned_cycle(w, n):
    return [(0, 1, w.s[i], w.s[i] - 1)[i % 4] for i in range(n)]


_model_records = {}


def model_records(w, h, n_max, rng, ts):
    """the model's records for lanes 0 .. n_max - 1 signed with key 0 under the lanes' own rng slices, computed once"""
    if id(w) not in _model_records:
        params, sk = rr.params_of(h), rr.sk_of(w.keys[0])
        _model_records[id(w)] = [rr.refund_return(sk, params, w.parsed(i), ts[i], *rr.nonces_of(rng[128 * i:128 * i + 128]), verify=False) for i in range(n_max)]
    return _model_records[id(w)]


@pytest.mark.parametrize("n", SIZES)
def test_returned_amounts_against_the_model(engine_factory, bench_params, n):
    from act_amd import capi
    eng = engine_factory(bench_params, L, max_batch=4096, transcript=capi.TRANSCRIPT_DEVICE)
    with step(240, "tokens and proofs"):
        w = world(eng, "rr-id", N_MAX)
    ts = returned_cycle(w, N_MAX)
    rng = shake("rr-model-rng", 128 * N_MAX)                     # per-lane slices: lane i signs with slice i at every n
    with step(300, "the model"):
        want = b"".join(model_records(w, bench_params, N_MAX, rng, ts)[:n])
    ring = [w.keys[1], w.keys[0]]
    blob, returned = b"".join(w.proofs[:n]), b"".join(scb(t) for t in ts[:n])
    charges = b"".join(scb(s) for s in w.s[:n])
    outs = {}
    for mem, wire in (("host", False), ("host", True), ("device", False), ("device", True)):
        if mem == "device" and n not in (3, 300):
            continue
        ns = capi.NullifierSet(1000)
        kw = dict(msgs=eng.cbor_encode("SpendProof", blob)) if wire else dict(blob=blob)
        with step(120, "n %d %s wire %d" % (n, mem, wire)):
            st, out, ok, c = call_return(eng, mem, ns, ring, n, charges=charges, returned=returned, rng=rng[:128 * n], rng_mode=capi.RNG_PER_LANE, sign_key=1,
                                         key_epochs=[7, 8], **kw)
        assert st == bytes(n) and list(ok) == [1 - i % 2 for i in range(n)] and c["accepted"] == n and c["return_too_big"] == 0
        assert sorted(e for _, e in _pairs(ns)) == sorted(7 + (1 - i % 2) for i in range(n))
        got = records_of(eng, wire, out, n)
        for i in range(n):
            assert got[160 * i:160 * i + 160] == want[160 * i:160 * i + 160], (n, mem, wire, i, ts[i])
        ns.close()
    # the client accepts them and holds c - s + t; the existing client refuses the first 128 bytes where t != 0
    pre, w0 = b"".join(w.prer[:n]), w.keys[0][32:]
    with step(120, "client"):
        cst, tok = eng.refund_to_credit_token_return(pre, blob, want, w0)
        ost, _ = eng.refund_to_credit_token(pre, blob, b"".join(want[160 * i:160 * i + 128] for i in range(n)), w0)
    assert cst == bytes(n)
    assert list(ost) == [4 if ts[i] else 0 for i in range(n)]
    bal = [CREDIT - w.s[i] + ts[i] for i in range(n)]
    for i in range(n):
        assert tok[160 * i + 128:160 * i + 160] == scb(bal[i]) and tok[160 * i:160 * i + 64] == want[160 * i:160 * i + 64]
    if n <= 3:
        params = rr.params_of(bench_params)
        for i in range(n):
            assert tok[160 * i:160 * i + 160] == rr.to_credit_token_return(rr.pre_of(w.prer[i]), params, w.parsed(i), want[160 * i:160 * i + 160],
                                                                           rr.sk_of(w.keys[0]).w).record()
    # ... and that balance is the balance the issuer signed: the new token spends ALL of it, under key 0, and is accepted
    with step(120, "spend again"):
        st, p2, _ = eng.prove_spend_seeded(tok, b"".join(scb(b) for b in bal), shake("rr-again-%d" % n, 32))
        assert st == bytes(n)
        ns = capi.NullifierSet(1000)
        st, out, ok, c = call_return(eng, "host", ns, [w.keys[0]], n, blob=p2, charges=b"".join(scb(b) for b in bal), returned=None,
                                     rng=shake("rr-again-rng", 128 * n), rng_mode=capi.RNG_SEQUENTIAL)
        assert st == bytes(n) and c["accepted"] == n
        # one credit more than the issuer signed does not verify
        if n == 3:
            st, p3, _ = eng.prove_spend_seeded(tok[:128] + scb(bal[0] + 1) + tok[160:], b"".join(scb(b) for b in bal), shake("rr-again-x", 32))
            vst, _ = eng.verify_spend_keyring([w.keys[0]], p3)
            assert vst[0] == 7 and vst[1:] == bytes(2)
        ns.close()
    assert eng.secret_residue() == 0


def test_returned_amounts_at_full_range_width(engine_factory, bench_params):
    """L = 128, n = 3: the client's Horner sum over 128 commitments under a returned amount"""
    from act_amd import capi
    eng = engine_factory(bench_params, 128, max_batch=16, transcript=capi.TRANSCRIPT_HOST)
    n = 3
    with step(240, "tokens and proofs"):
        w = world(eng, "rr-128", n, 128)
    ts = [w.s[0], 1, 0]
    rng = shake("rr-128-rng", 128 * n)
    ns = capi.NullifierSet(1000)
    blob = b"".join(w.proofs)
    with step(120, "redeem"):
        st, out, ok, c = call_return(eng, "host", ns, [w.keys[1], w.keys[0]], n, blob=blob, returned=b"".join(scb(t) for t in ts), rng=rng,
                                     rng_mode=capi.RNG_PER_LANE, sign_key=1)
    assert st == bytes(n) and c["accepted"] == n
    params, sk = rr.params_of(bench_params), rr.sk_of(w.keys[0])
    with step(300, "the model"):
        for i in range(n):
            assert out[160 * i:160 * i + 160] == rr.refund_return(sk, params, w.parsed(i), ts[i], *rr.nonces_of(rng[128 * i:128 * i + 128]), verify=False), i
    with step(120, "client"):
        cst, tok = eng.refund_to_credit_token_return(b"".join(w.prer), blob, out, w.keys[0][32:])
    assert cst == bytes(n) and [tok[160 * i + 128:160 * i + 160] for i in range(n)] == [scb(CREDIT - w.s[i] + ts[i]) for i in range(n)]
    ns.close()


# ---- 6. the screen ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem,wire", [("host", False), ("device", False), ("host", True), ("device", True)])
def test_the_screen_sheds_what_returns_too_much(engine_factory, bench_params, mem, wire):
    from act_amd import capi
    eng = engine_factory(bench_params, L, max_batch=4096, transcript=capi.TRANSCRIPT_DEVICE)
    with step(240, "tokens and proofs"):
        w = world(eng, "rr-id", N_MAX)
    n = 65
    ts = returned_cycle(w, n)
    big = {3: w.s[3] + 1, 10: w.s[10] + 1, 20: 1 << 128, 64: (1 << 200) + w.s[64]}      # one more than s, and at and beyond 2^128
    raw = [rr.le(big.get(i, ts[i])) for i in range(n)]
    raw[30] = rr.le(ELL + ts[30])                                  # an unreduced spelling of a fitting amount: accepted
    charges = [w.s[i] for i in range(n)]
    charges[10] += 1                                               # lane 10 fails both rules: the charge is the earlier one
    charges[11] += 1
    ring, epochs = [w.keys[1], w.keys[0]], [31, 32]
    recs = w.proofs[:n]
    msgs = eng.cbor_encode("SpendProof", b"".join(recs))
    rng = shake("rr-screen-rng", 128 * n)
    kw = lambda idx: dict(msgs=[msgs[i] for i in idx]) if wire else dict(blob=b"".join(recs[i] for i in idx))
    ns = capi.NullifierSet(1000)
    with step(120, "first call"):
        st, out, ok, c = call_return(eng, mem, ns, ring, n, charges=b"".join(scb(x) for x in charges), returned=b"".join(raw), rng=rng,
                                     rng_mode=capi.RNG_SEQUENTIAL, key_epochs=epochs, **kw(range(n)))
    shed = {3: 249, 20: 249, 64: 249, 10: 250, 11: 250}
    assert list(st) == [shed.get(i, 0) for i in range(n)]
    assert list(ok) == [255 if i in shed else 1 - i % 2 for i in range(n)]
    assert c == dict(lanes=n, wire_rejected=0, wrong_charge=2, spent_before=0, return_too_big=3, verified=n - 5, rejected_by_verification=0, double_spend_after=0,
                     accepted=n - 5)
    assert c["lanes"] == c["wire_rejected"] + c["wrong_charge"] + c["spent_before"] + c["return_too_big"] + c["verified"]
    assert c["verified"] == c["rejected_by_verification"] + c["double_spend_after"] + c["accepted"]
    assert ns.contains(b"".join(w.k[:n])) == bytes(0 if i in shed else 1 for i in range(n)) and len(ns) == n - 5
    got = records_of(eng, wire, out, n)
    for i in shed:
        assert got[160 * i:160 * i + 160] == bytes(160)
    # sequential slices went to the signed lanes only: the same call without the shed lanes signs the same bytes
    keep = [i for i in range(n) if i not in shed]
    ns2 = capi.NullifierSet(1000)
    with step(120, "the call without those lanes"):
        st2, out2, ok2, c2 = call_return(eng, mem, ns2, ring, len(keep), charges=b"".join(scb(charges[i]) for i in keep), returned=b"".join(raw[i] for i in keep),
                                         rng=rng, rng_mode=capi.RNG_SEQUENTIAL, key_epochs=epochs, **kw(keep))
    assert st2 == bytes(len(keep)) and c2["accepted"] == len(keep)
    got2 = records_of(eng, wire, out2, len(keep))
    assert b"".join(got[160 * i:160 * i + 160] for i in keep) == got2 and _pairs(ns) == _pairs(ns2)
    assert got[160 * 30 + 128:160 * 30 + 160] == scb(ts[30])        # the record holds the reduced t
    # a second call with amounts that fit (and the right charge) accepts the shed lanes
    idx = sorted(shed)
    with step(120, "second call"):
        st3, out3, ok3, c3 = call_return(eng, mem, ns, ring, len(idx), charges=b"".join(scb(w.s[i]) for i in idx), returned=b"".join(scb(w.s[i]) for i in idx),
                                         rng=shake("rr-screen-rng2", 128 * len(idx)), rng_mode=capi.RNG_SEQUENTIAL, key_epochs=epochs, **kw(idx))
    assert st3 == bytes(len(idx)) and c3["accepted"] == len(idx) and len(ns) == n
    got3 = records_of(eng, wire, out3, len(idx))
    assert [got3[160 * j + 128:160 * j + 160] for j in range(len(idx))] == [scb(w.s[i]) for i in idx]
    ns.close(); ns2.close()
    assert eng.secret_residue() == 0


def test_a_batch_in_which_every_lane_returns_too_much(engine_factory, bench_params):
    from act_amd import capi
    eng = engine_factory(bench_params, L, max_batch=4096, transcript=capi.TRANSCRIPT_DEVICE)
    with step(240, "tokens and proofs"):
        w = world(eng, "rr-id", N_MAX)
    n = 5
    ns = capi.NullifierSet(1000)
    g = capi.ReplayRng(shake("rr-all", 128 * n))
    st, out, ok, c = call_return(eng, "host", ns, [w.keys[0], w.keys[1]], n, blob=b"".join(w.proofs[:n]), returned=b"".join(scb(w.s[i] + 1 + i) for i in range(n)),
                                 rng=g, rng_mode=capi.RNG_CALLBACK)
    assert st == bytes([249] * n) and ok == bytes([255] * n) and out == bytes(160 * n) and len(ns) == 0 and g.draws == []
    assert c["return_too_big"] == n and c["verified"] == 0
    ns.close()


# ---- 7. the client's refusals, on each of its three roads -------------------------------------------------------------------------------------
@pytest.mark.parametrize("road", ["default", "no_fused_tiny", "no_wide_client"])
def test_the_client_refuses_altered_and_oversized_returns(engine_factory, bench_params, monkeypatch, road):
    """default: n = 3 and 64 take the one-launch form, 65 the four-role kernel and the finish kernel; no_fused_tiny: every n takes those
    two; no_wide_client: the one-lane-per-item kernel that calls above 8 192 items take"""
    from act_amd import capi
    if road != "default":
        monkeypatch.setenv("ACT_NO_FUSED_TINY", "1")               # (the one-launch form lives in the four-role kernel: without that kernel it is off too)
    if road == "no_wide_client":
        monkeypatch.setenv("ACT_NO_WIDE_CLIENT", "1")
    eng = engine_factory(bench_params, L, max_batch=4096, transcript=capi.TRANSCRIPT_DEVICE)
    try:
        with step(240, "tokens and proofs"):
            w = world(eng, "rr-id", N_MAX)
        for n in (3, 64, 65):
            keys = [w.keys[0], w.keys[1]]
            blob, pre = b"".join(w.proofs[:n]), b"".join(w.prer[:n])
            with step(120, "sign"):
                vst, vok, kp = eng.verify_spend_keyring(keys, blob, True)
                assert vst == bytes(n)
                # the sign-only call does not bound t: lane 1 returns one credit more than it spent
                ts = returned_cycle(w, n); ts[1] = w.s[1] + 1
                sst, recs = eng.refund_sign_return_keyring(keys, bytes(n), kp, vst, shake("rr-cl-%d" % n, 128 * n), b"".join(scb(t) for t in ts))
                assert sst == bytes(n)
            lanes = [recs[160 * i:160 * i + 160] for i in range(n)]
            lanes[0] = lanes[0][:128] + scb(ts[0] + 1)              # t altered after signing
            lanes[2] = lanes[2][:128] + scb(0)
            if n > 4:
                lanes[4] = b"\x01" + bytes(31) + lanes[4][32:]      # A is not a Ristretto encoding
            want = [4, 8, 4] + [0] * (n - 3)
            if n > 4:
                want[4] = 255
            with step(120, "client"):
                cst, tok = eng.refund_to_credit_token_return(pre, blob, b"".join(lanes), w.keys[0][32:])
            assert list(cst) == want, (road, n)
            for i in range(n):
                if want[i]:
                    assert tok[160 * i:160 * i + 160] == bytes(160)
                else:
                    assert tok[160 * i + 128:160 * i + 160] == scb(CREDIT - w.s[i] + ts[i]) and tok[160 * i + 64:160 * i + 128] == w.prer[i][32:64] + w.prer[i][:32]
            # under the other key nothing verifies
            cst, _ = eng.refund_to_credit_token_return(pre, blob, recs, w.keys[1][32:])
            assert cst == bytes([4] * n)
    finally:
        monkeypatch.undo()
        capi.forward_tuning_env()


# ---- 8. wire --------------------------------------------------------------------------------------------------------------------------------
SIZES_L128 = {"IssuanceRequest": 141, "IssuanceResponse": 176, "SpendProof": 18036, "Refund": 141, "PrivateKey": 71, "PublicKey": 34, "PreIssuance": 71,
              "CreditToken": 176, "PreRefund": 106}


def test_type_10_codec_and_reader(engine_factory, bench_params):
    from act_amd import capi
    e128 = engine_factory(bench_params, 128, max_batch=16)
    assert {t: e128.cbor_size(t) for t in SIZES_L128} == SIZES_L128 and e128.cbor_size("RefundReturn") == 176
    eng = engine_factory(bench_params, L, max_batch=4096, transcript=capi.TRANSCRIPT_DEVICE)
    assert eng.cbor_size("RefundReturn") == 176 == eng.cbor_size("Refund") + 35 and eng.lib.act_cbor_record_bytes(eng.ctx, 10) == 160
    assert eng.lib.act_cbor_size(eng.ctx, 11) == 0 and eng.lib.act_cbor_size(eng.ctx, 0) == 0
    with step(240, "tokens and proofs"):
        w = world(eng, "rr-id", N_MAX)
    n = 5
    ns = capi.NullifierSet(1000)
    st, out, ok, _ = call_return(eng, "host", ns, [w.keys[0], w.keys[1]], n, blob=b"".join(w.proofs[:n]), returned=b"".join(scb(w.s[i] - 1) for i in range(n)),
                                 rng=shake("rr-codec", 128 * n), rng_mode=capi.RNG_PER_LANE)
    assert st == bytes(n)
    recs = [out[160 * i:160 * i + 160] for i in range(n)]
    enc = eng.cbor_encode("RefundReturn", out)
    assert enc == [rr.cbor_encode(r) for r in recs] and all(len(x) == 176 for x in enc)
    assert eng.cbor_decode("RefundReturn", enc) == (bytes(n), out) and eng.cbor_read("RefundReturn", enc) == (bytes(n), out)
    cases = rr.respellings(recs[0])
    msgs = [c[1] for c in cases]
    want_st = bytes(c[2][0] for c in cases)                         # the codec's own codes: 0, 1 Ciborium, 2 InvalidStructure, 3 InvalidValue
    for fn in (eng.cbor_decode, eng.cbor_read):
        st, dec = fn("RefundReturn", msgs)
        assert st == want_st, fn
        assert dec == b"".join(c[2][1] for c in cases), fn
    ns.close()


# ---- 9. the Python interface ------------------------------------------------------------------------------------------------------------------
def test_python_api():
    """api.PrivateKey.refund_return / redeem_return_batch, api.Keyring, api.PreRefund.to_credit_token_return, api.RefundReturn"""
    from act_amd import api
    params = api.Params.new("test-org", "test-service", "test", "2024-01-01")
    rng = api.ByteStreamRng(shake("rr-api", 1 << 20))
    with step(240, "api round trip"):
        sk = api.PrivateKey.random(rng, params)
        pre = api.PreIssuance.random(rng, params)
        req = pre.request(params, rng)
        tok = pre.to_credit_token(params, sk.public(), req, sk.issue(params, req, 20, rng))
        proof, prer = tok.prove_spend(params, 5, rng)
        # the sign-only road: the bound is checked against the proof's own s, before the generator is touched
        before = rng.pos
        with pytest.raises(api.Error) as err:
            sk.refund_return(params, proof, 6, rng)
        assert err.value.code == 249 and err.value.name == "ReturnTooBig" and rng.pos == before
        rr1 = sk.refund_return(params, proof, 2, rng)
        assert isinstance(rr1, api.RefundReturn) and rr1.returned() == api.scalar(2) and rng.pos == before + 128
        assert api.RefundReturn.from_cbor(rr1.to_cbor(params), params) == rr1 and len(rr1.to_cbor(params)) == 176
        tok2 = prer.to_credit_token_return(params, proof, rr1, sk.public())
        assert tok2.credits() == api.scalar(20 - 5 + 2)
        with pytest.raises(api.Error) as err:
            prer.to_credit_token(params, proof, api.Refund(rr1.record[:128]), sk.public())
        assert err.value.code == 4
        with pytest.raises(api.Error) as err:
            prer.to_credit_token_return(params, proof, api.RefundReturn(rr1.record[:128] + api.scalar(3)), sk.public())
        assert err.value.code == 4
        # the redeem road
        db = api.NullifierDb(1000)
        res = sk.redeem_return_batch(params, db, [proof], rng, returned=[6], charges=[5])
        assert isinstance(res[0], api.Error) and res[0].code == 249 and len(db) == 0
        res = sk.redeem_return_batch(params, db, [proof, proof], rng, returned=[5, 0], charges=[5, 5])
        assert isinstance(res[0], api.RefundReturn) and res[0].returned() == api.scalar(5) and isinstance(res[1], api.Error) and res[1].code == 3 and len(db) == 1
        tok3 = prer.to_credit_token_return(params, proof, res[0], sk.public())
        assert tok3.credits() == api.scalar(20)
        ring = api.Keyring([sk], epochs=[9])
        proof3, prer3 = tok3.prove_spend(params, 20, rng)
        out, matched = ring.redeem_return_cbor_batch(params, db, [proof3.to_cbor(params)], rng, returned=[7], charges=[20])
        assert isinstance(out[0], bytes) and matched == [0] and db.epoch_len(9) == 1 and ring.last_admit_counts["return_too_big"] == 0
        tok4 = prer3.to_credit_token_return(params, proof3, api.RefundReturn.from_cbor(out[0], params), sk.public())
        assert tok4.credits() == api.scalar(7)
