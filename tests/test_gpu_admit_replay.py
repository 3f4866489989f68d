"""Admission for the replayable redemption on the GPU: act_redeem_admit_replay_batch / act_redeem_cbor_admit_replay_batch through the C
ABI against the model of tests/admit_replay_cases.py and against act_redeem_(cbor_)replay_batch on sets restored from the same
snapshots.  The tokens are those of tests/test_gpu_replay.py (its World: L = 8, 257 tokens, two proofs each with the same nullifier and
another K').  Every (transcripts, memory) pair, records and wire.  Every step runs under a time limit of its own.

Rates are measured by tools/admit_replay_probe.py; the tests here assert behaviour only."""
import numpy as np
import pytest

import admit_replay_cases as ar
import replay_cases as rp
from conftest import scb
from test_cbor import _variants
from test_gpu_replay import L, MODES, NONCE_KEY, SPEND, Dev, call_replay, keys_of, setup, step, _pairs

pytestmark = pytest.mark.gpu


def call_ar(eng, mem, ns, rs, ring, recs=None, msgs=None, charges=None, sign_key=-1, key_epochs=None, want_rc=0):
    """one call in either memory kind and either form -> (statuses, out: list of records or messages (b"" where not signed), out_key,
    replayed, counts).  Status bytes start as 99: a call that writes no status leaves them."""
    from act_amd import capi
    wire = msgs is not None
    n = len(msgs) if wire else len(recs)
    ob = eng.cbor_size("Refund") if wire else 128
    cc = b"".join(scb(c) for c in charges) if charges is not None else None
    if mem == "host":
        if wire:
            rc, st, out, ok, rep, c = eng.redeem_cbor_admit_replay(ns, rs, ring, msgs, NONCE_KEY, sign_key, key_epochs, cc, raw=True)
        else:
            rc, st, blob, ok, rep, c = eng.redeem_admit_replay(ns, rs, ring, b"".join(recs), NONCE_KEY, sign_key, key_epochs, cc, raw=True)
            out = [blob[128 * i:128 * i + 128] if st[i] == 0 else b"" for i in range(n)]
            assert all(st[i] == 0 or st[i] == 99 or not any(blob[128 * i:128 * i + 128]) for i in range(n)), "a failed lane's record is not zero"
    else:
        d = Dev()
        src = d.up(b"".join(msgs) if wire else b"".join(recs))
        dc = d.up(cc) if cc is not None else None
        offs = np.zeros(n + 1, np.uint64)
        if wire:
            offs[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
        o, s, k, r = d.new(ob * n, 7), d.new(n, 99), d.new(n, 77), d.new(n, 55)
        d.t.cuda.synchronize()
        p = dict(set=ns, receipts=rs, nonce_key=NONCE_KEY, out=o.data_ptr(), status=s.data_ptr(), out_key=k.data_ptr(), replayed=r.data_ptr(), key_epochs=key_epochs,
                 sign_key=sign_key, charges=dc.data_ptr() if dc is not None else None, raw=True)
        if wire:
            rc, c = eng.admit_replay_ptr("redeem_cbor", ring, n, capi.MEM_DEVICE, cbor=src.data_ptr(), offsets=offs.ctypes.data, **p)
        else:
            rc, c = eng.admit_replay_ptr("redeem", ring, n, capi.MEM_DEVICE, proofs=src.data_ptr(), **p)
        st, blob, ok, rep = d.down(s, n), d.down(o, ob * n), d.down(k, n), d.down(r, n)
        out = [blob[ob * i:ob * i + ob] if st[i] == 0 else b"" for i in range(n)]
        assert all(st[i] == 0 or st[i] == 99 or not any(blob[ob * i:ob * i + ob]) for i in range(n)), "a failed lane's slot is not zero"
    assert rc == want_rc, (rc, eng.lib.act_last_error(eng.ctx))
    return st, out, ok, rep, c


def lane(w, t, variant=0, how=None, s=SPEND):
    """the model's view of proof (t, variant) against the ring (key 0, key 1)"""
    if how == "bad com":
        return ar.Lane(w.k[t], (t, variant), 255, ar.KEY_NONE, s, 0, False)
    if how == "tampered":
        return ar.Lane(w.k[t], (t, variant), 7, ar.KEY_NONE, s)
    return ar.Lane(w.k[t], (t, variant), 0, w.owner[t], s)


def proof(w, t, variant=0, how=None):
    if how == "bad com":                                            # Com_0 is no point
        p = w.proofs[variant][t].copy()
        p[32 * 4:32 * 5] = 0xFF
        return p.tobytes()
    return w.proof(t, variant, how)                                 # "tampered": a byte of s_bar, outside k and Com


def against_model(got, lanes, spent, receipts, charges=None):
    st, out, ok, rep, c = got
    mst, mok, mrep, mc = ar.model(lanes, spent, receipts, charges)
    assert (list(st), list(ok), list(rep)) == (mst, mok, mrep)
    assert c == mc


def recorded(eng, mem, ring, w, tokens, key_epochs=None):
    """two fresh sets after one replay call that redeems variant 0 of `tokens` -> (set, receipts, the refunds of that call)"""
    from act_amd import capi
    ns, rs = capi.NullifierSet(2000), capi.NullifierSet(2000)
    got = call_replay(eng, mem, ns, rs, ring, recs=[w.proof(t) for t in tokens], key_epochs=key_epochs)
    assert got[0] == bytes(len(tokens))
    return ns, rs, got[1]


# the mixed batch: (token, variant, how).  Tokens 0..5 are redeemed (variant 0) before the call; a run of further lanes puts the batch
# over one workgroup of the compaction and mixes fresh lanes, retries and foreign spends
MIX = [(10, 0, None), (10, 0, None), (0, 0, None), (1, 1, None), (2, 1, "tampered"), (3, 0, "tampered"), (4, 0, "bad com"), (11, 0, "tampered"), (10, 1, None)]
MIX += [(t, 0, None) for t in range(20, 150)] + [(5, 0, None), (5, 1, None)] + [(t, 1, None) for t in range(150, 257)]
DOUBLY_BAD = (4, 6)                                                 # foreign and tampered; spent with a Com_j that is no point
PRE_SPENT = (0, 1, 2, 3, 4, 5) + tuple(range(100, 120)) + tuple(range(200, 257))      # retries inside the run of fresh lanes, then a run of foreign spends


# ---- 1. equivalence with the replay call ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,mem", MODES)
@pytest.mark.parametrize("wire", [False, True])
def test_equals_the_replay_call_on_every_lane_that_is_not_doubly_bad(engine_factory, bench_params, tmp_path, mode, mem, wire):
    capi, eng, w = setup(engine_factory, bench_params, mode)
    ring, epochs = w.keys, [31, 32]
    recs = [proof(w, t, v, how) for t, v, how in MIX]
    lanes = [lane(w, t, v, how) for t, v, how in MIX]
    kw = dict(msgs=eng.cbor_encode("SpendProof", b"".join(recs))) if wire else dict(recs=recs)
    with step(90, "the sets before the call"):
        ns, rs, _ = recorded(eng, mem, ring, w, PRE_SPENT, epochs)
        ns.save(str(tmp_path / "set.snap")); rs.save(str(tmp_path / "receipts.snap"))
        ns.close(); rs.close()
        sets = [(capi.NullifierSet.restore(str(tmp_path / "set.snap"), 2000), capi.NullifierSet.restore(str(tmp_path / "receipts.snap"), 2000)) for _ in range(2)]
    with step(90, "both calls"):
        new = call_ar(eng, mem, sets[0][0], sets[0][1], ring, key_epochs=epochs, **kw)
        old = call_replay(eng, mem, sets[1][0], sets[1][1], ring, key_epochs=epochs, **kw)
    spent, receipts = {w.k[t] for t in PRE_SPENT}, {(w.k[t], (t, 0)) for t in PRE_SPENT}
    before = frozenset(spent)
    against_model(new, lanes, spent, receipts)
    n = len(MIX)
    for i in range(n):
        if i in DOUBLY_BAD:
            assert (new[0][i], new[2][i], old[0][i]) == (3, 255, lanes[i].verdict), i
        elif new[0][i] == 3 and lanes[i].k in before:               # a foreign spend is shed unverified: ACT_KEY_NONE, where the replay call keeps the key it matched
            assert old[0][i] == 3 and new[1][i] == old[1][i] == b"" and new[3][i] == old[3][i] == 0 and (new[2][i], old[2][i]) == (255, w.owner[MIX[i][0]]), i
        else:
            assert (new[0][i], new[1][i], new[2][i], new[3][i]) == (old[0][i], old[1][i], old[2][i], old[3][i]), i
    assert _pairs(sets[0][0]) == _pairs(sets[1][0]) and _pairs(sets[0][1]) == _pairs(sets[1][1])
    c = new[4]
    assert c["verified"] == n - c["foreign_spend"] and c["fresh"] + c["replayed"] == sum(1 for s in new[0] if s == 0) and c["foreign_spend"] == 4 + 57
    for a, b in sets:
        a.close(); b.close()
    assert eng.secret_residue() == 0


# ---- 2. / 3. a retry is served, a foreign spend is not verified -- also over several windows --------------------------------------------------
@pytest.mark.parametrize("mode,mem", MODES)
@pytest.mark.parametrize("max_batch", [4096, 16])
def test_a_retry_is_served_and_a_foreign_spend_is_not_verified(engine_factory, bench_params, mode, mem, max_batch):
    capi, eng, w = setup(engine_factory, bench_params, mode)
    if max_batch != 4096:                                           # windows of 4 * 16 lanes: candidates and survivors each span several
        eng = engine_factory(bench_params, L, max_batch=max_batch, transcript=capi.TRANSCRIPT_HOST if mode == "host" else capi.TRANSCRIPT_DEVICE)
    n, ring = w.n, w.keys
    ns, rs = capi.NullifierSet(1000), capi.NullifierSet(1000)
    spent, receipts = set(), set()
    with step(90, "call 1: variant 0 of every token"):
        first = call_ar(eng, mem, ns, rs, ring, recs=[w.proof(t) for t in range(n)])
        against_model(first, [lane(w, t) for t in range(n)], spent, receipts)
        assert first[0] == bytes(n) and first[4]["fresh"] == n and first[4]["foreign_spend"] == 0 and (len(ns), len(rs)) == (n, n)
    before = (keys_of(ns), keys_of(rs))
    with step(90, "call 2: retries and foreign spends"):
        recs = [w.proof(t, t % 2) for t in range(n)]
        got = call_ar(eng, mem, ns, rs, ring, recs=recs)
        against_model(got, [lane(w, t, t % 2) for t in range(n)], spent, receipts)
        st, out, ok, rep, c = got
        retries, foreign = (n + 1) // 2, n // 2
        assert list(st) == [3 if t % 2 else 0 for t in range(n)] and list(rep) == [0 if t % 2 else 1 for t in range(n)]
        assert all(out[t] == first[1][t] and out[t] for t in range(0, n, 2))
        assert (c["foreign_spend"], c["retry_candidates"], c["verified"], c["replayed"], c["fresh"]) == (foreign, retries, retries, retries, 0)
        assert (keys_of(ns), keys_of(rs)) == before
    with step(90, "foreign spends only: no verification kernel"):
        eng.prof_enable(True); eng.prof_reset()
        got = call_ar(eng, mem, ns, rs, ring, recs=[w.proof(t, 1) for t in range(n)])
        prof = eng.prof()
        eng.prof_enable(False)
        assert got[0] == bytes([3]) * n and got[2] == b"\xff" * n and got[3] == bytes(n) and got[1] == [b""] * n
        assert got[4] == dict(lanes=n, wire_rejected=0, wrong_charge=0, foreign_spend=n, retry_candidates=0, verified=0, rejected_by_verification=0, fresh=0, replayed=0,
                              double_spend_after=0, unanswered=0)
        assert "k_spend_bits" not in prof and not any(k.startswith("k_spend") for k in prof), prof
        assert (keys_of(ns), keys_of(rs)) == before
    with step(90, "the same lanes through the replay call are verified: the hook sees the launches"):
        eng.prof_enable(True); eng.prof_reset()
        old = call_replay(eng, mem, ns, rs, ring, recs=[w.proof(t, 1) for t in range(n)])
        prof = eng.prof()
        eng.prof_enable(False)
        assert old[0] == bytes([3]) * n and prof["k_spend_bits"]["lanes"] == n * L
    ns.close(); rs.close()
    assert eng.secret_residue() == 0


# ---- 4. wire spellings -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,mem", MODES)
def test_respelled_retries_replay_and_respelled_foreign_spends_are_not_verified(engine_factory, bench_params, mode, mem):
    capi, eng, w = setup(engine_factory, bench_params, mode)
    n, ring = 67, w.keys
    canon = eng.cbor_encode("SpendProof", b"".join(w.proof(t) for t in range(n)))
    # every legal spelling of test_cbor._variants in turn, the canonical one among them; odd lanes are the OTHER proof of the token
    import pymodel
    msgs = []
    for t in range(n):
        rec = w.proof(t, t % 2)
        legal = [msg for msg, _ in _variants("SpendProof", rec, L) if pymodel.cbor_decode("SpendProof", msg, L) == (0, rec)]
        assert len(legal) >= 8
        msgs.append(legal[t % len(legal)])
    assert sum(1 for t in range(n) if msgs[t] != eng.cbor_encode("SpendProof", w.proof(t, t % 2))[0]) > n // 2
    try:
        for reader in (capi.WIRE_READER_DEVICE, capi.WIRE_READER_HOST):
            eng.set_wire_reader(reader)
            ns, rs = capi.NullifierSet(1000), capi.NullifierSet(1000)
            spent, receipts = set(), set()
            with step(90, "canonical, then respelled, reader %d" % reader):
                first = call_ar(eng, mem, ns, rs, ring, msgs=canon)
                against_model(first, [lane(w, t) for t in range(n)], spent, receipts)
                again = call_ar(eng, mem, ns, rs, ring, msgs=msgs)
                against_model(again, [lane(w, t, t % 2) for t in range(n)], spent, receipts)
                st, out, ok, rep, c = again
                assert list(st) == [3 if t % 2 else 0 for t in range(n)] and all(out[t] == first[1][t] and out[t] for t in range(0, n, 2))
                assert (c["foreign_spend"], c["verified"], c["replayed"]) == (n // 2, (n + 1) // 2, (n + 1) // 2) and (len(ns), len(rs)) == (n, n)
            ns.close(); rs.close()
    finally:
        eng.set_wire_reader(capi.WIRE_READER_DEVICE)
    assert eng.secret_residue() == 0


# ---- 5. charges ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,mem", MODES)
@pytest.mark.parametrize("wire", [False, True])
def test_a_wrong_charge_is_250_on_spent_and_fresh_lanes_and_leaves_no_trace(engine_factory, bench_params, mode, mem, wire):
    capi, eng, w = setup(engine_factory, bench_params, mode)
    ring = w.keys
    toks = [0, 1, 2, 3, 70, 71, 72, 73]                            # 0..3 are redeemed before the call
    recs = [w.proof(t) for t in toks]
    kw = dict(msgs=eng.cbor_encode("SpendProof", b"".join(recs))) if wire else dict(recs=recs)
    charges = [SPEND, SPEND + 1, SPEND, SPEND + 1, SPEND, SPEND + 1, SPEND, SPEND + 1]
    with step(90, "the sets before the call"):
        ns, rs, refunds = recorded(eng, mem, ring, w, (0, 1, 2, 3))
    spent, receipts = {w.k[t] for t in range(4)}, {(w.k[t], (t, 0)) for t in range(4)}
    with step(90, "every second lane at the wrong price"):
        got = call_ar(eng, mem, ns, rs, ring, charges=charges, **kw)
        against_model(got, [lane(w, t) for t in toks], spent, receipts, charges)
        assert list(got[0]) == [0, 250, 0, 250, 0, 250, 0, 250] and list(got[3]) == [1, 0, 1, 0, 0, 0, 0, 0] and got[4]["wrong_charge"] == 4
        assert (len(ns), len(rs)) == (6, 6)                         # tokens 71 and 73 left nothing in either set
    with step(90, "afterwards at the right price"):
        got = call_ar(eng, mem, ns, rs, ring, charges=[SPEND] * 8, **kw)
        against_model(got, [lane(w, t) for t in toks], spent, receipts, [SPEND] * 8)
        assert got[0] == bytes(8) and list(got[3]) == [1, 1, 1, 1, 1, 0, 1, 0] and (len(ns), len(rs)) == (8, 8)
        if not wire:
            assert got[1][:4] == refunds
    ns.close(); rs.close()
    assert eng.secret_residue() == 0


# ---- 6. refusals and epochs ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,mem", MODES)
def test_whole_call_refusals_and_the_matched_keys_epoch_in_both_sets(engine_factory, bench_params, mode, mem):
    capi, eng, w = setup(engine_factory, bench_params, mode)
    n, ring, epochs = 65, w.keys, [101, 102]
    recs = [w.proof(t) for t in range(n)]
    ns, small = capi.NullifierSet(1000), capi.NullifierSet(500)     # 1024 slots: room for 512 keys
    with step(90, "receipts == set, and a receipts set without room"):
        assert call_ar(eng, mem, ns, ns, ring, recs=recs, want_rc=1)[0] == bytes([99]) * n
        filler = b"".join(scb(1000 + i) for i in range(512 - n + 1))
        assert small.check_and_insert(filler) == bytes(512 - n + 1)
        st, out, ok, rep, c = call_ar(eng, mem, ns, small, ring, recs=recs, want_rc=1)
        assert st == bytes([99]) * n and (len(ns), len(small)) == (0, 512 - n + 1) and c["lanes"] == 0
        assert b"receipts" in eng.lib.act_last_error(eng.ctx)
    rs = capi.NullifierSet(1000)
    with step(90, "under epochs: both sets hold the matched key's epoch"):
        got = call_ar(eng, mem, ns, rs, ring, recs=recs, sign_key=0, key_epochs=epochs)
        assert got[0] == bytes(n) and got[4]["fresh"] == n
        kp = eng.verify_spend_keyring(ring, b"".join(recs), want_kprime=True)[2]
        assert _pairs(ns) == sorted((rp.reduced(recs[t][:32]), epochs[w.owner[t]]) for t in range(n))
        assert _pairs(rs) == sorted((rp.tag(recs[t][:32], kp[32 * t:32 * t + 32]), epochs[w.owner[t]]) for t in range(n))
    with step(90, "an epoch retired on one set only"):
        gone = sum(1 for t in range(n) if w.owner[t] == 1)
        assert rs.retire_epoch(102) == gone
        st = call_ar(eng, mem, ns, rs, ring, recs=recs, sign_key=0, key_epochs=epochs, want_rc=1)[0]
        assert st == bytes([99]) * n and (len(ns), len(rs)) == (n, n - gone)
    ns.close(); rs.close(); small.close()
    assert eng.secret_residue() == 0


# ---- 7. the Python layer ---------------------------------------------------------------------------------------------------------------------------
def test_the_python_api_with_admit_gives_what_the_capi_call_gives(engine_factory, bench_params):
    from act_amd import api
    capi, eng, w = setup(engine_factory, bench_params, "host")
    params = api.Params(bench_params)
    ring = api.Keyring([api.PrivateKey(k) for k in w.keys], epochs=[11, 12])
    toks = [(0, 0), (1, 1), (2, 0), (80, 0), (81, 0)]               # tokens 0..2 are redeemed before: a retry, a foreign spend, a retry, two fresh
    with step(120, "api and capi on sets with the same history"):
        dbs = [(api.NullifierDb(1 << 10), api.NullifierDb(1 << 10)) for _ in range(2)]
        for db, receipts in dbs:
            res, _, _ = ring.redeem_replay_batch(params, db, receipts, [api.SpendProof(w.proof(t), L) for t in range(3)], NONCE_KEY)
            assert all(isinstance(r, api.Refund) for r in res)
        proofs = [api.SpendProof(w.proof(t, v), L) for t, v in toks]
        res, keys, rep = ring.redeem_replay_batch(params, dbs[0][0], dbs[0][1], proofs, NONCE_KEY, admit=True, charges=[SPEND] * 5)
        st, out, ok, crep, c = eng.redeem_admit_replay(dbs[1][0].set, dbs[1][1].set, w.keys, b"".join(w.proof(t, v) for t, v in toks), NONCE_KEY, key_epochs=[11, 12],
                                                       charges=scb(SPEND) * 5)
        assert list(st) == [0, 3, 0, 0, 0] and [r.code if isinstance(r, api.Error) else 0 for r in res] == list(st)
        assert [r.record for r in res if isinstance(r, api.Refund)] == [out[128 * i:128 * i + 128] for i in range(5) if st[i] == 0]
        assert rep == [bool(b) for b in crep] == [True, False, True, False, False] and ring.last_replay_counts == c
        assert c["foreign_spend"] == 1 and c["verified"] == 4 and (len(dbs[0][0]), len(dbs[0][1])) == (5, 5)
        msgs = [p.to_cbor(params) for p in proofs]
        out2, _, rep2 = ring.redeem_replay_cbor_batch(params, dbs[0][0], dbs[0][1], msgs, NONCE_KEY, L, admit=True)
        assert rep2 == [True, False, True, True, True] and ring.last_replay_counts["foreign_spend"] == 1
        assert [o for o in out2 if isinstance(o, bytes)] == eng.cbor_encode("Refund", b"".join(out[128 * i:128 * i + 128] for i in range(5) if st[i] == 0))
        with pytest.raises(ValueError):
            ring.redeem_replay_batch(params, dbs[0][0], dbs[0][1], proofs, NONCE_KEY, charges=[SPEND] * 5)
