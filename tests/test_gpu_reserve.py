"""Reserve on the GPU: act_redeem_reserve_batch / act_redeem_cbor_reserve_batch through the C ABI.  Reserve is held to
act_redeem_(cbor_)admit_replay_batch without its signature on sets restored from snapshots -- statuses, out_key, out_replayed, counts
and the nullifier set -- and its receipts and records to the definitions of tests/reserve_cases.py.  The tokens are those of
tests/test_gpu_replay.py (its World: L = 8, 257 tokens that spend s = 3, two proofs each with the same nullifier and another K').  Both
transcript modes with both memory kinds, records and wire, a ring of two keys with epochs.  Every step runs under a time limit of its
own.  The settle half is tests/test_gpu_settle.py, which takes its helpers from here.

Rates are measured by tools/reserve_settle_probe.py; the tests here assert behaviour only."""
import numpy as np
import pytest

import pymodel as m
import reserve_cases as rc
from conftest import scb
from test_cbor import _variants
from test_gpu_admit_replay import PRE_SPENT, call_ar, lane, proof
from test_gpu_replay import L, NONCE_KEY, SPEND, Dev, _pairs, call_replay, setup, step
from test_gpu_return_replay import MIX257, restored, snapshot

pytestmark = pytest.mark.gpu

MODES = [("host", "host"), ("device", "device")]                  # (transcripts, caller's memory): both of each
S = SPEND


def call_reserve(eng, mem, ns, rs, ring, recs=None, msgs=None, charges=None, key_epochs=None, want_rc=0):
    """one reserve call in either memory kind and either form -> (statuses, records: 96 bytes or b"" where rejected, out_key, replayed,
    counts, the raw output bytes).  Status bytes start as 99: a call that writes no status leaves them."""
    from act_amd import capi
    wire = msgs is not None
    n = len(msgs) if wire else len(recs)
    cc = b"".join(scb(c) for c in charges) if charges is not None else None
    if mem == "host":
        rc_, st, blob, ok, rep, c = (eng.redeem_cbor_reserve(ns, rs, ring, msgs, key_epochs, cc, raw=True) if wire else
                                     eng.redeem_reserve(ns, rs, ring, b"".join(recs), key_epochs, cc, raw=True))
    else:
        d = Dev()
        src = d.up(b"".join(msgs) if wire else b"".join(recs))
        dc = d.up(cc) if cc is not None else None
        offs = np.zeros(n + 1, np.uint64)
        if wire:
            offs[1:] = np.cumsum([len(x) for x in msgs], dtype=np.uint64)
        o, s, k, r = d.new(96 * n, 7), d.new(n, 99), d.new(n, 77), d.new(n, 55)
        d.t.cuda.synchronize()
        p = dict(set=ns, receipts=rs, out=o.data_ptr(), status=s.data_ptr(), out_key=k.data_ptr(), replayed=r.data_ptr(), key_epochs=key_epochs,
                 charges=dc.data_ptr() if dc is not None else None, raw=True)
        if wire:
            rc_, c = eng.reserve_ptr("redeem_cbor", ring, n, capi.MEM_DEVICE, cbor=src.data_ptr(), offsets=offs.ctypes.data, **p)
        else:
            rc_, c = eng.reserve_ptr("redeem", ring, n, capi.MEM_DEVICE, proofs=src.data_ptr(), **p)
        st, blob, ok, rep = d.down(s, n), d.down(o, 96 * n), d.down(k, n), d.down(r, n)
    assert rc_ == want_rc, (rc_, eng.lib.act_last_error(eng.ctx))
    if rc_ == 0:
        assert all(st[i] == 0 or not any(blob[96 * i:96 * i + 96]) for i in range(n)), "a rejected lane's record is not zero"
    out = [blob[96 * i:96 * i + 96] if st[i] == 0 else b"" for i in range(n)]
    return st, out, ok, rep, c, blob


def call_settle(eng, mem, rs, ring, reservations, key_index, amounts=None, sign_key=-1, key_epochs=None, wire=False, nonce_key=NONCE_KEY, want_rc=0):
    """one settle call in either memory kind; reservations: a list of 96-byte records; amounts: a list of ints (unreduced values allowed)
    or None (a null pointer) -> (statuses, out: list of records or messages (b"" where not signed), settled_before, counts, raw output)"""
    from act_amd import capi
    n = len(reservations)
    ob = eng.cbor_size("RefundReturn") if wire else 160
    tt = None if amounts is None else b"".join(int(t).to_bytes(32, "little") for t in amounts)
    if mem == "host":
        rc_, st, out, sb, c = eng.redeem_settle(rs, ring, b"".join(reservations), bytes(key_index), nonce_key, tt, sign_key, key_epochs, cbor=wire, raw=True)
        blob = b"".join(x if x else bytes(ob) for x in out) if wire else out
    else:
        d = Dev()
        dr, dk = d.up(b"".join(reservations)), d.up(bytes(key_index))
        dt = d.up(tt) if tt is not None else None
        o, s, b = d.new(ob * n, 7), d.new(n, 99), d.new(n, 55)
        d.t.cuda.synchronize()
        rc_, c = eng.settle_ptr(ring, n, capi.MEM_DEVICE, receipts=rs, reservations=dr.data_ptr(), key_index=dk.data_ptr(), amounts=dt.data_ptr() if dt is not None else None,
                                nonce_key=nonce_key, out=o.data_ptr(), status=s.data_ptr(), settled_before=b.data_ptr(), key_epochs=key_epochs, sign_key=sign_key, cbor=wire,
                                raw=True)
        st, blob, sb = d.down(s, n), d.down(o, ob * n), d.down(b, n)
    assert rc_ == want_rc, (rc_, eng.lib.act_last_error(eng.ctx))
    if rc_ == 0:
        assert all(st[i] == 0 or not any(blob[ob * i:ob * i + ob]) for i in range(n)), "a failed lane's slot is not zero"
        assert all(st[i] != 0 or any(blob[ob * i:ob * i + ob]) for i in range(n)), "an accepted lane's slot is zero"
    out = [blob[ob * i:ob * i + ob] if st[i] == 0 else b"" for i in range(n)]
    return st, out, sb, c, blob


_kprimes = {}


def kprimes(eng, w):
    """enc(K') of every proof of the World, [variant][token], by the engine's own verification"""
    if id(w) not in _kprimes:
        out = []
        for v in range(2):
            st, ok, kp = eng.verify_spend_keyring(w.keys, b"".join(w.proof(t, v) for t in range(w.n)), want_kprime=True)
            assert st == bytes(w.n)
            out.append([kp[32 * t:32 * t + 32] for t in range(w.n)])
        _kprimes[id(w)] = out
    return _kprimes[id(w)]


def kbytes(w, t):
    return w.k[t].to_bytes(32, "little")


def model_receipts(eng, w, receipts, epochs):
    """the model's receipts (tests/reserve_cases.py) as the (key, epoch) pairs the set must hold; epochs None: epoch 0"""
    kp = kprimes(eng, w)
    tok = {w.k[t]: t for t in range(w.n)}
    out = []
    for e in receipts:
        t = tok[e[1]]
        p = kp[e[2][1]][t]
        key = rc.tag_res(kbytes(w, t), p, e[3]) if e[0] == "res" else rc.marker(kbytes(w, t), p) if e[0] == "mark" else rc.tag(kbytes(w, t), p, e[3])
        out.append((key, epochs[w.owner[t]] if epochs else 0))
    return sorted(out)


# ---- 1. reserve is the admit-replay call without the signature ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,mem", MODES)
@pytest.mark.parametrize("wire", [False, True])
def test_reserve_is_the_admit_replay_call_without_the_signature(engine_factory, bench_params, tmp_path, mode, mem, wire):
    capi, eng, w = setup(engine_factory, bench_params, mode)
    ring, epochs = w.keys, [31, 32]
    assert len(MIX257) == 257
    pre = [w.proof(t) for t in PRE_SPENT]
    with step(90, "the sets before the calls: the spends recorded by reserve itself, and by the admit-replay call"):
        ns, rs = capi.NullifierSet(2000), capi.NullifierSet(2000)
        got = call_reserve(eng, mem, ns, rs, ring, recs=pre, key_epochs=epochs)
        assert got[0] == bytes(len(pre)) and got[3] == bytes(len(pre))
        mine = snapshot(ns, rs, tmp_path, "reserve")
        ns.close(); rs.close()
        ns, rs = capi.NullifierSet(2000), capi.NullifierSet(2000)
        assert call_ar(eng, mem, ns, rs, ring, recs=pre, key_epochs=epochs)[0] == bytes(len(pre))
        theirs = snapshot(ns, rs, tmp_path, "admit-replay")
        ns.close(); rs.close()
    kp = kprimes(eng, w)
    for n in (1, 3, 64, 65, 257):
        recs = [proof(w, t, v, how) for t, v, how in MIX257[:n]]
        lanes = [lane(w, t, v, how) for t, v, how in MIX257[:n]]
        kw = dict(msgs=eng.cbor_encode("SpendProof", b"".join(recs))) if wire else dict(recs=recs)
        a, b = restored(capi, mine), restored(capi, theirs)
        with step(90, "n = %d: reserve, and the admit-replay call" % n):
            new = call_reserve(eng, mem, a[0], a[1], ring, key_epochs=epochs, **kw)
            old = call_ar(eng, mem, b[0], b[1], ring, key_epochs=epochs, **kw)
        assert (new[0], new[2], new[3], new[4]) == (old[0], old[2], old[3], old[4]), n
        assert _pairs(a[0]) == _pairs(b[0]), n
        spent, receipts = {w.k[t] for t in PRE_SPENT}, {("res", w.k[t], (t, 0), S) for t in PRE_SPENT}
        mst, mok, mrep, mc, mrecs = rc.reserve(lanes, spent, receipts)
        assert (list(new[0]), list(new[2]), list(new[3]), new[4]) == (mst, mok, mrep, mc), n
        assert _pairs(a[1]) == model_receipts(eng, w, receipts, epochs), n
        for i, (t, v, how) in enumerate(MIX257[:n]):
            assert new[1][i] == (rc.record(kbytes(w, t), kp[v][t], S) if mst[i] == 0 else b""), (n, i)
        if n == 257:
            assert old[4]["foreign_spend"] > 0 and old[4]["retry_candidates"] > 0 and old[4]["fresh"] > 0 and old[4]["double_spend_after"] > 0
        for x in a + b:
            x.close()
    assert eng.secret_residue() == 0


# ---- 3. retries of the SpendProof batch -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,mem", MODES)
@pytest.mark.parametrize("wire", [False, True])
def test_a_retried_batch_gets_its_records_again_and_changes_nothing(engine_factory, bench_params, tmp_path, mode, mem, wire):
    capi, eng, w = setup(engine_factory, bench_params, mode)
    n, ring, epochs = 6, w.keys, [41, 42]
    recs = [w.proof(t) for t in range(n)]
    kw = dict(msgs=eng.cbor_encode("SpendProof", b"".join(recs))) if wire else dict(recs=recs)
    ns, rs = capi.NullifierSet(1000), capi.NullifierSet(1000)
    with step(60, "first call"):
        first = call_reserve(eng, mem, ns, rs, ring, charges=[S] * n, key_epochs=epochs, **kw)
        assert first[0] == bytes(n) and first[3] == bytes(n) and first[4]["fresh"] == n and list(first[2]) == [w.owner[t] for t in range(n)]
    before = (_pairs(ns), _pairs(rs))
    with step(60, "the same batch again"):
        again = call_reserve(eng, mem, ns, rs, ring, charges=[S] * n, key_epochs=epochs, **kw)
        assert again[0] == bytes(n) and again[3] == b"\1" * n and again[5] == first[5] and again[2] == first[2] and again[4]["retry_candidates"] == n
        assert (_pairs(ns), _pairs(rs)) == before and (len(ns), len(rs)) == (n, n)
    with step(90, "a second context, sets restored from snapshots"):
        snaps = snapshot(ns, rs, tmp_path, "retry")
        eng2 = engine_factory(bench_params, L, max_batch=2048, transcript=capi.TRANSCRIPT_HOST if mode == "host" else capi.TRANSCRIPT_DEVICE)
        assert eng2 is not eng
        ns2, rs2 = restored(capi, snaps)
        other = call_reserve(eng2, mem, ns2, rs2, ring, charges=[S] * n, key_epochs=epochs, **kw)
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
                    spelled = call_reserve(eng, mem, ns, rs, ring, charges=[S] * n, key_epochs=epochs, msgs=legal)
                    assert spelled[0] == bytes(n) and spelled[3] == b"\1" * n and spelled[5] == first[5] and (_pairs(ns), _pairs(rs)) == before
        finally:
            eng.set_wire_reader(capi.WIRE_READER_DEVICE)
    with step(60, "the other proof of a reserved token, a wrong charge, and a spend recorded by a one-phase call"):
        assert call_replay(eng, mem, ns, rs, ring, recs=[w.proof(20)], key_epochs=epochs)[0] == b"\0"
        got = call_reserve(eng, mem, ns, rs, ring, recs=[w.proof(0, 1), w.proof(1), w.proof(20)], charges=[S, S + 1, S], key_epochs=epochs)
        assert list(got[0]) == [3, 250, 3] and got[2] == b"\xff" * 3 and got[3] == bytes(3) and got[4]["foreign_spend"] == 2 and got[4]["verified"] == 0
        assert (len(ns), len(rs)) == (n + 1, n + 1)
    ns.close(); rs.close()
    assert eng.secret_residue() == 0


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,mem", MODES)
def test_whole_call_refusals_leave_the_status_fill_and_the_sets(engine_factory, bench_params, mode, mem):
    capi, eng, w = setup(engine_factory, bench_params, mode)
    n, ring = 5, w.keys
    recs = [w.proof(t) for t in range(n)]
    ns, small = capi.NullifierSet(1000), capi.NullifierSet(500)     # 1024 slots: room for 512 keys
    with step(60, "receipts == set, and a receipts set without room for n"):
        got = call_reserve(eng, mem, ns, ns, ring, recs=recs, want_rc=1)
        assert got[0] == bytes([99]) * n and len(ns) == 0
        filler = b"".join(scb(1000 + i) for i in range(512 - n + 1))
        assert small.check_and_insert(filler) == bytes(512 - n + 1)
        got = call_reserve(eng, mem, ns, small, ring, recs=recs, want_rc=1)
        assert got[0] == bytes([99]) * n and (len(ns), len(small)) == (0, 512 - n + 1) and got[4]["lanes"] == 0
        assert b"receipts" in eng.lib.act_last_error(eng.ctx)
    with step(60, "a pending test hook for the signature step is not reserve's: nothing is signed here"):
        rs = capi.NullifierSet(1000)
        assert eng.lib.act_debug_fail_next_signs(eng.ctx, 1) == 0
        got = call_reserve(eng, mem, ns, rs, ring, recs=recs)
        assert got[0] == bytes(n) and (len(ns), len(rs)) == (n, n)
        assert eng.lib.act_debug_fail_next_signs(eng.ctx, 0) == 0
    ns.close(); rs.close(); small.close()
    assert eng.secret_residue() == 0
