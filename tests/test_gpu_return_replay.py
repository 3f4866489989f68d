"""Replayable partial refunds on the GPU ("the receipt pins t"): act_redeem_return_replay_batch /
act_redeem_cbor_return_replay_batch / act_replay_derive_return_batch through the C ABI.  With nothing returned they are held to
act_redeem_(cbor_)admit_replay_batch on sets restored from the same snapshots; with t != 0 to the model of tests/refund_return_cases.py
under the nonces of tests/return_replay_cases.py, and the call as a whole to that file's model (receipts as (k, K', t^)).  The tokens are
those of tests/test_gpu_replay.py (its World: L = 8, 257 tokens that spend s = 3, two proofs each with the same nullifier and another K');
one case at L = 128.  Both memory kinds, records and wire, a ring of two keys.  Every step runs under a time limit of its own."""
import numpy as np
import pytest

import pymodel as m
import refund_return_cases as rrc
import return_replay_cases as rr
from conftest import ELL, scb, shake
from test_cbor import _variants
from test_gpu_admit_replay import MIX, PRE_SPENT, call_ar, lane, proof, recorded
from test_gpu_refund_return import records_of, refunds_of
from test_gpu_refund_return import world as world128
from test_gpu_replay import CREDIT, L, NONCE_KEY, SPEND, Dev, _pairs, call_replay, keys_of, setup, step

pytestmark = pytest.mark.gpu

MODES = [("host", "host"), ("device", "device")]                  # (transcripts, caller's memory): both of each
S = SPEND
NULL = "null"                                                       # returned = NULL, as opposed to an array of zeros


def call_rr(eng, mem, ns, rs, ring, recs=None, msgs=None, charges=None, returned=None, sign_key=-1, key_epochs=None, want_rc=0):
    """one call in either memory kind and either form; returned: a list of ints (unreduced values allowed) or NULL
    -> (statuses, out: list of records or messages (b"" where not signed), out_key, replayed, counts, the raw output bytes).
    Status bytes start as 99: a call that writes no status leaves them."""
    from act_amd import capi
    wire = msgs is not None
    n = len(msgs) if wire else len(recs)
    ob = eng.cbor_size("RefundReturn") if wire else 160
    cc = b"".join(scb(c) for c in charges) if charges is not None else None
    tt = None if returned is None or returned == NULL else b"".join(int(t).to_bytes(32, "little") for t in returned)
    if mem == "host":
        if wire:
            rc, st, out, ok, rep, c = eng.redeem_cbor_return_replay(ns, rs, ring, msgs, NONCE_KEY, sign_key, key_epochs, cc, tt, raw=True)
            blob = b"".join(x if x else bytes(ob) for x in out)
        else:
            rc, st, blob, ok, rep, c = eng.redeem_return_replay(ns, rs, ring, b"".join(recs), NONCE_KEY, sign_key, key_epochs, cc, tt, raw=True)
    else:
        d = Dev()
        src = d.up(b"".join(msgs) if wire else b"".join(recs))
        dc = d.up(cc) if cc is not None else None
        dt = d.up(tt) if tt is not None else None
        offs = np.zeros(n + 1, np.uint64)
        if wire:
            offs[1:] = np.cumsum([len(x) for x in msgs], dtype=np.uint64)
        o, s, k, r = d.new(ob * n, 7), d.new(n, 99), d.new(n, 77), d.new(n, 55)
        d.t.cuda.synchronize()
        p = dict(set=ns, receipts=rs, nonce_key=NONCE_KEY, out=o.data_ptr(), status=s.data_ptr(), out_key=k.data_ptr(), replayed=r.data_ptr(), key_epochs=key_epochs,
                 sign_key=sign_key, charges=dc.data_ptr() if dc is not None else None, returned=dt.data_ptr() if dt is not None else None, raw=True)
        if wire:
            rc, c = eng.return_replay_ptr("redeem_cbor", ring, n, capi.MEM_DEVICE, cbor=src.data_ptr(), offsets=offs.ctypes.data, **p)
        else:
            rc, c = eng.return_replay_ptr("redeem", ring, n, capi.MEM_DEVICE, proofs=src.data_ptr(), **p)
        st, blob, ok, rep = d.down(s, n), d.down(o, ob * n), d.down(k, n), d.down(r, n)
    assert rc == want_rc, (rc, eng.lib.act_last_error(eng.ctx))
    if rc == 0:
        assert all(st[i] == 0 or not any(blob[ob * i:ob * i + ob]) for i in range(n)), "a failed lane's slot is not zero"
        assert all(st[i] != 0 or any(blob[ob * i:ob * i + ob]) for i in range(n)), "an accepted lane's slot is zero"
    out = [blob[ob * i:ob * i + ob] if st[i] == 0 else b"" for i in range(n)]
    return st, out, ok, rep, c, blob


def records(eng, wire, got, n):
    """the 160-byte records of a call's output (wire: decoded as type 10, and canonical), zeros where not signed"""
    return records_of(eng, wire, got[5], n) if got[0] != bytes([99]) * n else bytes(160 * n)


def against_model(got, lanes, spent, receipts, charges=None, returned=None):
    mst, mok, mrep, mc = rr.model(lanes, spent, receipts, charges, None if returned in (None, NULL) else returned)
    assert (list(got[0]), list(got[2]), list(got[3])) == (mst, mok, mrep)
    assert got[4] == mc


_kprime = {}


def kprime_of(eng, w, t, variant=0):
    """enc(K') of proof (t, variant), by the engine's own verification"""
    if (id(w), t, variant) not in _kprime:
        st, ok, kp = eng.verify_spend_keyring(w.keys, w.proof(t, variant), want_kprime=True)
        assert st == b"\0"
        _kprime[(id(w), t, variant)] = kp
    return _kprime[(id(w), t, variant)]


_model_records = {}


def model_record(eng, w, h, t, amount, key):
    """refund_return_cases' model of the RefundReturn of token t's proof for `amount`, signed with ring key `key` under the derived nonces"""
    what = (id(w), t, amount % ELL, key)
    if what not in _model_records:
        rec = w.proof(t)
        non = rr.nonce(NONCE_KEY, w.keys[key], rec[:32], kprime_of(eng, w, t), amount)
        _model_records[what] = rrc.refund_return(rrc.sk_of(w.keys[key]), rrc.params_of(h), m.parse_spend_proof(rec, L), amount, *rrc.nonces_of(non), verify=False)
    return _model_records[what]


def snapshot(ns, rs, tmp_path, tag):
    a, b = str(tmp_path / (tag + "-set.snap")), str(tmp_path / (tag + "-receipts.snap"))
    ns.save(a); rs.save(b)
    return a, b


def restored(capi, snaps):
    return capi.NullifierSet.restore(snaps[0], 2000), capi.NullifierSet.restore(snaps[1], 2000)


# ---- 1. identity at nothing returned ------------------------------------------------------------------------------------------------------------
MIX257 = MIX + [(t, 0, None) for t in range(150, 150 + 257 - len(MIX))]      # one more than the compaction's workgroup of 256


@pytest.mark.parametrize("mode,mem", MODES)
@pytest.mark.parametrize("wire", [False, True])
def test_nothing_returned_is_the_admission_replay_call(engine_factory, bench_params, tmp_path, mode, mem, wire):
    capi, eng, w = setup(engine_factory, bench_params, mode)
    ring, epochs = w.keys, [31, 32]
    assert len(MIX257) == 257
    with step(90, "the sets before the calls"):
        ns, rs, _ = recorded(eng, mem, ring, w, PRE_SPENT, epochs)
        snaps = snapshot(ns, rs, tmp_path, "id")
        ns.close(); rs.close()
    for n in (1, 3, 64, 65, 257):
        recs = [proof(w, t, v, how) for t, v, how in MIX257[:n]]
        kw = dict(msgs=eng.cbor_encode("SpendProof", b"".join(recs))) if wire else dict(recs=recs)
        sets = [restored(capi, snaps) for _ in range(3)]
        with step(90, "n = %d: NULL, all zero, and the call without amounts" % n):
            null = call_rr(eng, mem, sets[0][0], sets[0][1], ring, key_epochs=epochs, returned=NULL, **kw)
            zero = call_rr(eng, mem, sets[1][0], sets[1][1], ring, key_epochs=epochs, returned=[0] * n, **kw)
            old = call_ar(eng, mem, sets[2][0], sets[2][1], ring, key_epochs=epochs, **kw)
        ob = eng.cbor_size("Refund") if wire else 128
        want = refunds_of(eng, wire, b"".join(x if x else bytes(ob) for x in old[1]), n)
        for got in (null, zero):
            assert (got[0], got[2], got[3]) == (old[0], old[2], old[3]), n
            assert {k: v for k, v in got[4].items() if k != "return_too_big"} == old[4] and got[4]["return_too_big"] == 0, n
            rec = records(eng, wire, got, n)
            for i in range(n):
                assert rec[160 * i:160 * i + 128] == want[128 * i:128 * i + 128] and rec[160 * i + 128:160 * i + 160] == bytes(32), (n, i)
        assert _pairs(sets[0][0]) == _pairs(sets[1][0]) == _pairs(sets[2][0]) and _pairs(sets[0][1]) == _pairs(sets[1][1]) == _pairs(sets[2][1]), n
        if n == 257:
            assert old[4]["foreign_spend"] > 0 and old[4]["retry_candidates"] > 0 and old[4]["fresh"] > 0 and old[4]["double_spend_after"] > 0
        for a, b in sets:
            a.close(); b.close()
    assert eng.secret_residue() == 0


# ---- 2. t != 0 against the model, and 3. the retry ------------------------------------------------------------------------------------------------
def amounts(n, shift=0):
    return [(1, S - 1, S)[(i + shift) % 3] for i in range(n)]


@pytest.mark.parametrize("mode,mem", MODES)
@pytest.mark.parametrize("wire", [False, True])
def test_returned_amounts_against_the_model_and_a_retry_gets_the_same_bytes(engine_factory, bench_params, tmp_path, mode, mem, wire):
    capi, eng, w = setup(engine_factory, bench_params, mode)
    n, ring, epochs = 6, w.keys, [41, 42]
    ts = amounts(n)
    recs = [w.proof(t) for t in range(n)]
    kw = dict(msgs=eng.cbor_encode("SpendProof", b"".join(recs))) if wire else dict(recs=recs)
    lanes = [lane(w, t) for t in range(n)]
    spent, receipts = set(), set()
    ns, rs = capi.NullifierSet(1000), capi.NullifierSet(1000)
    with step(60, "first call"):
        first = call_rr(eng, mem, ns, rs, ring, charges=[S] * n, returned=ts, key_epochs=epochs, **kw)
        against_model(first, lanes, spent, receipts, [S] * n, ts)
        assert first[0] == bytes(n) and first[3] == bytes(n) and first[4]["fresh"] == n
    with step(120, "the model's records, tags and nullifiers"):
        got = records(eng, wire, first, n)
        for t in range(n):
            assert got[160 * t:160 * t + 160] == model_record(eng, w, bench_params, t, ts[t], w.owner[t]), (t, ts[t])
        assert _pairs(rs) == sorted((rr.tag(recs[t][:32], kprime_of(eng, w, t), ts[t]), epochs[w.owner[t]]) for t in range(n))
        assert _pairs(ns) == sorted((rr.rp.reduced(recs[t][:32]), epochs[w.owner[t]]) for t in range(n))
    before = (_pairs(ns), _pairs(rs))
    with step(60, "the same batch again"):
        again = call_rr(eng, mem, ns, rs, ring, charges=[S] * n, returned=ts, key_epochs=epochs, **kw)
        against_model(again, lanes, spent, receipts, [S] * n, ts)
        assert again[0] == bytes(n) and again[3] == b"\1" * n and again[5] == first[5] and again[4]["retry_candidates"] == n
        assert (_pairs(ns), _pairs(rs)) == before and (len(ns), len(rs)) == (n, n)
    with step(90, "a second context, sets restored from snapshots"):
        snaps = snapshot(ns, rs, tmp_path, "retry")
        eng2 = engine_factory(bench_params, L, max_batch=2048, transcript=capi.TRANSCRIPT_HOST if mode == "host" else capi.TRANSCRIPT_DEVICE)
        assert eng2 is not eng
        ns2, rs2 = restored(capi, snaps)
        other = call_rr(eng2, mem, ns2, rs2, ring, charges=[S] * n, returned=ts, key_epochs=epochs, **kw)
        assert other[0] == bytes(n) and other[3] == b"\1" * n and other[5] == first[5] and (_pairs(ns2), _pairs(rs2)) == before
        ns2.close(); rs2.close()
        assert eng2.secret_residue() == 0
    if wire:
        legal = []
        for t in range(n):
            ok = [msg for msg, _ in _variants("SpendProof", recs[t], L) if m.cbor_decode("SpendProof", msg, L) == (0, recs[t]) and msg != kw["msgs"][t]]
            legal.append(ok[t % len(ok)])
        try:
            for reader in (capi.WIRE_READER_DEVICE, capi.WIRE_READER_HOST):
                eng.set_wire_reader(reader)
                with step(60, "the retry in another legal spelling, reader %d" % reader):
                    spelled = call_rr(eng, mem, ns, rs, ring, charges=[S] * n, returned=ts, key_epochs=epochs, msgs=legal)
                    assert spelled[0] == bytes(n) and spelled[3] == b"\1" * n and spelled[5] == first[5] and (_pairs(ns), _pairs(rs)) == before
        finally:
            eng.set_wire_reader(capi.WIRE_READER_DEVICE)
    ns.close(); rs.close()
    assert eng.secret_residue() == 0


@pytest.mark.parametrize("mode,mem", MODES)
def test_a_batch_over_several_workgroups_is_the_composition_of_derive_and_sign(engine_factory, bench_params, mode, mem):
    """n = 65 with shed lanes in between (so the amounts travel through the compaction): every record is
    act_refund_sign_return_keyring_batch over the nonces of act_replay_derive_return_batch, and those are the header's hashes"""
    capi, eng, w = setup(engine_factory, bench_params, mode)
    n, ring = 65, w.keys
    ts = amounts(n, 1)
    charges = [S + 1 if t % 9 == 4 else S for t in range(n)]       # every ninth lane is shed at the wrong price
    for t in range(7, n, 13):
        ts[t] = S + 1                                               # ... and a few for returning too much
    recs = [w.proof(t) for t in range(n)]
    shed = {t: 250 if charges[t] != S else 249 for t in range(n) if charges[t] != S or ts[t] > S}
    ns, rs = capi.NullifierSet(1000), capi.NullifierSet(1000)
    spent, receipts = set(), set()
    with step(60, "the call"):
        got = call_rr(eng, mem, ns, rs, ring, recs=recs, charges=charges, returned=ts)
        against_model(got, [lane(w, t) for t in range(n)], spent, receipts, charges, ts)
        assert list(got[0]) == [shed.get(t, 0) for t in range(n)] and got[4]["return_too_big"] == sum(1 for v in shed.values() if v == 249)
    with step(60, "derive and sign"):
        st, ok, kp = eng.verify_spend_keyring(ring, b"".join(recs), want_kprime=True)
        assert st == bytes(n)
        live = bytes(1 if t in shed else 0 for t in range(n))
        tt = b"".join(scb(v) for v in ts)
        tags, non = eng.replay_derive(ring, ok, NONCE_KEY, b"".join(r[:32] for r in recs), kp, live, returned=tt)
        sst, want = eng.refund_sign_return_keyring(ring, ok, kp, live, non, tt, capi.RNG_PER_LANE)
        for t in range(n):
            k, p = recs[t][:32], kp[32 * t:32 * t + 32]
            if t in shed:
                assert got[1][t] == b"" and tags[32 * t:32 * t + 32] == bytes(32) and non[128 * t:128 * t + 128] == bytes(128)
                continue
            assert tags[32 * t:32 * t + 32] == rr.tag(k, p, ts[t]) and non[128 * t:128 * t + 128] == rr.nonce(NONCE_KEY, ring[ok[t]], k, p, ts[t]), t
            assert sst[t] == 0 and got[1][t] == want[160 * t:160 * t + 160], t
        assert keys_of(rs) == sorted(tags[32 * t:32 * t + 32] for t in range(n) if t not in shed) and len(ns) == n - len(shed)
    ns.close(); rs.close()
    assert eng.secret_residue() == 0


# ---- 4. the pin ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,mem", MODES)
@pytest.mark.parametrize("wire", [False, True])
def test_the_receipt_pins_the_amount(engine_factory, bench_params, mode, mem, wire):
    capi, eng, w = setup(engine_factory, bench_params, mode)
    ring = w.keys
    toks = [0, 1, 2, 3]
    recs = [w.proof(t) for t in toks]
    form = lambda rs_: dict(msgs=eng.cbor_encode("SpendProof", b"".join(rs_))) if wire else dict(recs=rs_)
    ns, rs = capi.NullifierSet(1000), capi.NullifierSet(1000)
    t1 = [2, 2, 1, S]
    with step(60, "recorded with t1; tokens 4 and 5 by the call without amounts"):
        first = call_rr(eng, mem, ns, rs, ring, returned=t1, **form(recs))
        assert first[0] == bytes(4)
        plain = call_replay(eng, mem, ns, rs, ring, **form([w.proof(4), w.proof(5)]))
        assert plain[0] == bytes(2)
    before = (_pairs(ns), _pairs(rs))
    zero = dict.fromkeys(rr.COUNTS, 0)
    with step(60, "another amount, zero against non-zero and non-zero against zero included"):
        got = call_rr(eng, mem, ns, rs, ring, returned=[1, 0, 2, S - 1, 1, S], **form(recs + [w.proof(4), w.proof(5)]))
        assert got[0] == bytes([3]) * 6 and got[1] == [b""] * 6 and got[2] == b"\xff" * 6 and got[3] == bytes(6)
        assert got[4] == dict(zero, lanes=6, foreign_spend=6)      # shed in the screen: not in verified
        assert (_pairs(ns), _pairs(rs)) == before
        old = call_ar(eng, mem, ns, rs, ring, **form(recs))        # the calls without amounts name t = 0
        assert old[0] == bytes([3]) * 4 and (_pairs(ns), _pairs(rs)) == before
    with step(60, "t1 + l is t1; the spends of the call without amounts are served with t = 0"):
        got = call_rr(eng, mem, ns, rs, ring, returned=[t + ELL for t in t1] + [0, ELL], **form(recs + [w.proof(4), w.proof(5)]))
        assert got[0] == bytes(6) and got[3] == b"\1" * 6 and got[1][:4] == first[1] and got[4]["replayed"] == 6
        rec = records(eng, wire, got, 6)
        want = refunds_of(eng, wire, b"".join(plain[1]), 2)
        assert rec[160 * 4:160 * 4 + 128] == want[:128] and rec[160 * 5:160 * 5 + 128] == want[128:] and rec[160 * 4 + 128:160 * 5] == bytes(32)
        assert (_pairs(ns), _pairs(rs)) == before
    with step(60, "inside one batch: [P t1, P t1, P t2]"):
        p = w.proof(9)
        got = call_rr(eng, mem, ns, rs, ring, returned=[2, 2, 1], **form([p, p, p]))
        assert list(got[0]) == [0, 0, 3] and list(got[3]) == [0, 1, 0] and got[1][0] == got[1][1] and got[1][2] == b""
        assert (got[4]["fresh"], got[4]["replayed"], got[4]["double_spend_after"], got[4]["verified"]) == (1, 1, 1, 3)
        assert (len(ns), len(rs)) == (7, 7)
    ns.close(); rs.close()
    assert eng.secret_residue() == 0


# ---- 5. the screen ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,mem", MODES)
@pytest.mark.parametrize("wire", [False, True])
def test_too_much_is_249_in_front_of_the_look_up_and_leaves_no_trace(engine_factory, bench_params, mode, mem, wire):
    capi, eng, w = setup(engine_factory, bench_params, mode)
    ring = w.keys
    toks = [0, 1, 30, 31, 32, 33]                                   # 0 and 1 are spent before the call
    recs = [w.proof(t) for t in toks]
    kw = dict(msgs=eng.cbor_encode("SpendProof", b"".join(recs))) if wire else dict(recs=recs)
    ns, rs = capi.NullifierSet(1000), capi.NullifierSet(1000)
    with step(60, "the sets before the call"):
        assert call_rr(eng, mem, ns, rs, ring, returned=[1, 1], recs=recs[:2])[0] == bytes(2)
    before = (_pairs(ns), _pairs(rs))
    spent, receipts = {w.k[0], w.k[1]}, {(w.k[0], (0, 0), 1), (w.k[1], (1, 0), 1)}
    charges = [S, S + 1, S, S + 1, S, S]
    ts = [S + 1, S + 1, S + 1, S + 1, (1 << 200) + 1, S + ELL]      # lane 5: an unreduced spelling of an amount that fits
    with step(60, "t = s + 1 on spent and fresh lanes, with and without the wrong charge"):
        got = call_rr(eng, mem, ns, rs, ring, charges=charges, returned=ts, **kw)
        against_model(got, [lane(w, t) for t in toks], spent, receipts, charges, ts)
        assert list(got[0]) == [249, 250, 249, 250, 249, 0] and got[2][:5] == b"\xff" * 5 and got[1][:5] == [b""] * 5
        assert (got[4]["return_too_big"], got[4]["wrong_charge"], got[4]["foreign_spend"], got[4]["verified"], got[4]["fresh"]) == (3, 2, 0, 1, 1)
        assert ns.contains(b"".join(r[:32] for r in recs)) == bytes([1, 1, 0, 0, 0, 1]) and (len(ns), len(rs)) == (3, 3)
        assert [p for p in _pairs(ns) if p in before[0]] == before[0] and [p for p in _pairs(rs) if p in before[1]] == before[1]
    with step(60, "everything shed: nothing is verified, nothing is recorded"):
        got = call_rr(eng, mem, ns, rs, ring, returned=[S + 1] * 6, **kw)
        assert got[0] == bytes([249]) * 6 and got[4] == dict(dict.fromkeys(rr.COUNTS, 0), lanes=6, return_too_big=6) and (len(ns), len(rs)) == (3, 3)
    ns.close(); rs.close()
    assert eng.secret_residue() == 0


# ---- 6. nonce separation through the derive call ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["host", "device"])
def test_derive_separates_the_amounts_and_without_them_is_the_derive_call(engine_factory, bench_params, mem):
    capi, eng, w = setup(engine_factory, bench_params, "device")
    ring = w.keys
    rec = w.proof(0)
    kp = kprime_of(eng, w, 0)
    ts = [0, 1, 2, S]
    n = len(ts)
    kidx, nul, kps, st = bytes([1] * n), rec[:32] * n, kp * n, bytes(n)
    tt = b"".join(scb(t) for t in ts)

    def run(returned):
        """returned: bytes, NULL (the new symbol with a null pointer) or None (act_replay_derive_batch)"""
        if mem == "host":
            if returned == NULL:
                a = [np.frombuffer(x, np.uint8).copy() for x in (kidx, nul, kps, st)]
                tags, non = np.zeros(32 * n, np.uint8), np.zeros(128 * n, np.uint8)
                eng.replay_derive_ptr(ring, n, capi.MEM_HOST, NONCE_KEY, a[0].ctypes.data, a[1].ctypes.data, 32, a[2].ctypes.data, a[3].ctypes.data, tags.ctypes.data,
                                      non.ctypes.data, p_returned=0)
                return tags.tobytes(), non.tobytes()
            return eng.replay_derive(ring, kidx, NONCE_KEY, nul, kps, st, returned=returned)
        d = Dev()
        a = [d.up(x) for x in (kidx, nul, kps, st)]
        dt = d.up(returned) if isinstance(returned, bytes) else None
        tags, non = d.new(32 * n, 9), d.new(128 * n, 9)
        d.t.cuda.synchronize()
        eng.replay_derive_ptr(ring, n, capi.MEM_DEVICE, NONCE_KEY, a[0].data_ptr(), a[1].data_ptr(), 32, a[2].data_ptr(), a[3].data_ptr(), tags.data_ptr(), non.data_ptr(),
                              p_returned=None if returned is None else (dt.data_ptr() if dt is not None else 0))
        return d.down(tags, 32 * n), d.down(non, 128 * n)

    with step(60, "derive"):
        tags, non = run(tt)
        old, null = run(None), run(NULL)
    assert null == old and old[0] == rr.rp.tag(rec[:32], kp) * n and old[1] == rr.rp.nonce(NONCE_KEY, ring[1], rec[:32], kp) * n
    for i, t in enumerate(ts):
        assert tags[32 * i:32 * i + 32] == rr.tag(rec[:32], kp, t) and non[128 * i:128 * i + 128] == rr.nonce(NONCE_KEY, ring[1], rec[:32], kp, t), t
    assert len({tags[32 * i:32 * i + 32] for i in range(n)}) == n
    for q in range(4):
        assert len({non[128 * i + 32 * q:128 * i + 32 * q + 32] for i in range(n)}) == n, q
    assert eng.secret_residue() == 0


# ---- 7. the client accepts it -------------------------------------------------------------------------------------------------------------------------
def test_the_client_accepts_a_served_and_a_replayed_record_at_full_range_width(engine_factory, bench_params):
    from act_amd import capi
    eng = engine_factory(bench_params, 128, max_batch=16, transcript=capi.TRANSCRIPT_HOST)
    n = 3
    with step(240, "tokens and proofs"):
        w = world128(eng, "rr-128", n, 128)
    ts = [w.s[0], 1, 2]
    blob, ring = b"".join(w.proofs), [w.keys[1], w.keys[0]]
    ns, rs = capi.NullifierSet(1000), capi.NullifierSet(1000)
    with step(120, "served, then replayed"):
        tt = b"".join(scb(t) for t in ts)
        st, out, ok, rep, c = eng.redeem_return_replay(ns, rs, ring, blob, NONCE_KEY, sign_key=1, charges=b"".join(scb(s) for s in w.s), returned=tt)
        assert st == bytes(n) and rep == bytes(n) and c["fresh"] == n
        st2, out2, ok2, rep2, c2 = eng.redeem_return_replay(ns, rs, ring, blob, NONCE_KEY, sign_key=1, charges=b"".join(scb(s) for s in w.s), returned=tt)
        assert st2 == bytes(n) and rep2 == b"\1" * n and out2 == out and c2["replayed"] == n
    with step(120, "client"):
        pre = b"".join(w.prer)
        for o in (out, out2):
            cst, tok = eng.refund_to_credit_token_return(pre, blob, o, w.keys[0][32:])
            assert cst == bytes(n) and [tok[160 * i + 128:160 * i + 160] for i in range(n)] == [scb(CREDIT - w.s[i] + ts[i]) for i in range(n)]
        ost, _ = eng.refund_to_credit_token(pre, blob, b"".join(out[160 * i:160 * i + 128] for i in range(n)), w.keys[0][32:])
        assert ost == bytes([4]) * n                                # the plain client call refuses the first 128 bytes when t != 0
    ns.close(); rs.close()
    assert eng.secret_residue() == 0


# ---- 8. refusals and hygiene --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,mem", MODES)
def test_whole_call_refusals_and_a_failed_signature_step(engine_factory, bench_params, mode, mem):
    from act_amd import api
    capi, eng, w = setup(engine_factory, bench_params, mode)
    n, ring = 5, w.keys
    recs = [w.proof(t) for t in range(n)]
    ts = amounts(n)
    ns, small = capi.NullifierSet(1000), capi.NullifierSet(500)     # 1024 slots: room for 512 keys
    with step(60, "receipts == set, and a receipts set without room"):
        got = call_rr(eng, mem, ns, ns, ring, recs=recs, returned=ts, want_rc=1)
        assert got[0] == bytes([99]) * n and len(ns) == 0
        filler = b"".join(scb(1000 + i) for i in range(512 - n + 1))
        assert small.check_and_insert(filler) == bytes(512 - n + 1)
        got = call_rr(eng, mem, ns, small, ring, recs=recs, returned=ts, want_rc=1)
        assert got[0] == bytes([99]) * n and (len(ns), len(small)) == (0, 512 - n + 1) and got[4]["lanes"] == 0
        assert b"receipts" in eng.lib.act_last_error(eng.ctx)
    with step(60, "unique with returned amounts: refused before anything is looked at"):
        keyring = api.Keyring([api.PrivateKey(k) for k in ring])
        dbs = api.NullifierDb(1 << 10), api.NullifierDb(1 << 10)
        with pytest.raises(ValueError):
            keyring.redeem_replay_batch(api.Params(bench_params), dbs[0], dbs[1], [api.SpendProof(r, L) for r in recs], NONCE_KEY, unique=True, returned=ts)
        assert (len(dbs[0]), len(dbs[1])) == (0, 0)
    rs = capi.NullifierSet(1000)
    with step(60, "the signature step fails behind the recorded nullifiers"):
        assert eng.lib.act_debug_fail_next_signs(eng.ctx, 1) == 0
        got = call_rr(eng, mem, ns, rs, ring, recs=recs, returned=ts, want_rc=2)
        assert got[0] == bytes([251]) * n and got[1] == [b""] * n and (len(ns), len(rs)) == (n, n) and got[4]["unanswered"] == n
        assert eng.secret_residue() == 0
    with step(60, "a later retry with the same amounts is served; with other amounts it is not"):
        got = call_rr(eng, mem, ns, rs, ring, recs=recs, returned=amounts(n, 1))
        assert got[0] == bytes([3]) * n
        got = call_rr(eng, mem, ns, rs, ring, recs=recs, returned=ts)
        assert got[0] == bytes(n) and got[3] == b"\1" * n
        for t in range(n):
            assert got[1][t][128:160] == scb(ts[t])
        fresh_ns, fresh_rs = capi.NullifierSet(1000), capi.NullifierSet(1000)
        assert call_rr(eng, mem, fresh_ns, fresh_rs, ring, recs=recs, returned=ts)[5] == got[5]      # the bytes an undisturbed run gives
        fresh_ns.close(); fresh_rs.close()
    ns.close(); rs.close(); small.close()
    assert eng.secret_residue() == 0


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------------------------
def test_the_python_api_with_returned_gives_what_the_capi_call_gives(engine_factory, bench_params):
    from act_amd import api
    capi, eng, w = setup(engine_factory, bench_params, "host")
    params = api.Params(bench_params)
    ring = api.Keyring([api.PrivateKey(k) for k in w.keys], epochs=[11, 12])
    toks, ts = [0, 1, 2, 3], [1, S, S + 1, 2]
    with step(120, "api and capi on sets with the same history"):
        dbs = [(api.NullifierDb(1 << 10), api.NullifierDb(1 << 10)) for _ in range(2)]
        proofs = [api.SpendProof(w.proof(t), L) for t in toks]
        res, keys, rep = ring.redeem_replay_batch(params, dbs[0][0], dbs[0][1], proofs, NONCE_KEY, charges=[S] * 4, returned=ts)
        st, out, ok, crep, c = eng.redeem_return_replay(dbs[1][0].set, dbs[1][1].set, w.keys, b"".join(w.proof(t) for t in toks), NONCE_KEY, key_epochs=[11, 12],
                                                        charges=scb(S) * 4, returned=b"".join(scb(t) for t in ts))
        assert list(st) == [0, 0, 249, 0] and [r.code if isinstance(r, api.Error) else 0 for r in res] == list(st)
        assert [r.record for r in res if isinstance(r, api.RefundReturn)] == [out[160 * i:160 * i + 160] for i in range(4) if st[i] == 0]
        assert rep == [bool(b) for b in crep] == [False] * 4 and ring.last_replay_counts == c and c["return_too_big"] == 1
        msgs = [p.to_cbor(params) for p in proofs]
        out2, _, rep2 = ring.redeem_replay_cbor_batch(params, dbs[0][0], dbs[0][1], msgs, NONCE_KEY, L, returned=[1, S, S, 2])
        assert rep2 == [True, True, False, True] and ring.last_replay_counts["fresh"] == 1
        assert [o for i, o in enumerate(out2) if i != 2] == rrc_messages(eng, out, st)
        one = api.PrivateKey(w.keys[0]).redeem_replay_batch(params, api.NullifierDb(1 << 10), api.NullifierDb(1 << 10), proofs[:1], NONCE_KEY, returned=[1])
        assert isinstance(one[0][0], api.RefundReturn) and one[0][0].record == out[:160] and one[1] == [False]


def rrc_messages(eng, out, st):
    return [rrc.cbor_encode(out[160 * i:160 * i + 160]) for i in range(len(st)) if st[i] == 0]
