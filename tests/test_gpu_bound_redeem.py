"""Request binding on the GPU, the redemption calls: act_redeem_(cbor_)return_replay_bound_batch and
act_redeem_(cbor_)reserve_bound_batch through the C ABI, and the Python layer over them.

What they are held to.  The binding enters the challenge hash and nothing else: K', the receipt tags and the derived nonces are functions
of the commitments, which a bound proof shares with the unbound proof made from the same token, charge and rng bytes.  So the model's
answer for a bound batch IS the unbound call's answer for the unbound twins of its lanes (a lane with a wrong binding: a tampered
twin), on sets with the same history -- statuses, output bytes, out_key, replay marks, counts and both sets, byte for byte.  Then
retries, the mismatch matrix around the compaction, the scenario of DESIGN 4.11 ("Why the pin"), reserve + settle, bind = NULL, and the
refusal of the unique form.  L = 8, both transcript modes with both memory kinds, records and wire.  Every step runs under a time limit
of its own."""
import numpy as np
import pytest

from conftest import scb, shake
from test_gpu_bound import SPEND, World, engine
from test_gpu_replay import NONCE_KEY, Dev, _pairs, step
from test_gpu_reserve import call_settle

pytestmark = pytest.mark.gpu

MODES = [("host", "host"), ("device", "device")]                  # (transcripts, caller's memory): both of each
L, N = 8, 140
S = SPEND
ABSENT = "absent"


def call(eng, mem, kind, ns, rs, ring, recs, wire, bind=ABSENT, charges=None, returned=None, key_epochs=None, want_rc=0, respell=()):
    """one return-replay (kind "rr") or reserve (kind "res") call in either memory kind and either form; bind: a list of 32-byte values,
    None (the bound call with NULL) or ABSENT (the call without the argument)
    -> (statuses, raw output bytes, out_key, replayed, counts).  Status bytes start as 99: a call that writes no status leaves them."""
    from act_amd import capi
    n = len(recs)
    msgs = eng.cbor_encode("SpendProof", b"".join(recs)) if wire else None
    for i in (respell if wire else ()):      # another legal CBOR spelling of the same record: the wire reader's road
        msgs[i] = respelled(recs[i], msgs[i], i)
    ob = 96 if kind == "res" else eng.cbor_size("RefundReturn") if wire else 160
    cc = b"".join(scb(c) for c in charges) if charges is not None else None
    tt = b"".join(scb(t) for t in returned) if returned is not None else None
    bb = b"".join(bind) if bind not in (ABSENT, None) else None
    kw = {} if bind == ABSENT else dict(bind=bb)
    if mem == "host":
        rows = msgs if wire else b"".join(recs)
        if kind == "res":
            rc, st, blob, ok, rep, c = (eng.redeem_cbor_reserve if wire else eng.redeem_reserve)(ns, rs, ring, rows, key_epochs, cc, raw=True, **kw)
        else:
            rc, st, out, ok, rep, c = (eng.redeem_cbor_return_replay if wire else eng.redeem_return_replay)(ns, rs, ring, rows, NONCE_KEY, -1, key_epochs, cc, tt, raw=True, **kw)
            blob = b"".join(x if x else bytes(ob) for x in out) if wire else out
    else:
        d = Dev()
        src = d.up(b"".join(msgs) if wire else b"".join(recs))
        dc, dt, db = (d.up(x) if x is not None else None for x in (cc, tt, bb))
        offs = np.zeros(n + 1, np.uint64)
        if wire:
            offs[1:] = np.cumsum([len(x) for x in msgs], dtype=np.uint64)
        o, s, k, r = d.new(ob * n, 7), d.new(n, 99), d.new(n, 77), d.new(n, 55)
        d.t.cuda.synchronize()
        p = dict(set=ns, receipts=rs, out=o.data_ptr(), status=s.data_ptr(), out_key=k.data_ptr(), replayed=r.data_ptr(), key_epochs=key_epochs,
                 charges=dc.data_ptr() if dc is not None else None, raw=True)
        if bind != ABSENT:
            p["bind"] = db.data_ptr() if db is not None else None
        p.update(dict(cbor=src.data_ptr(), offsets=offs.ctypes.data) if wire else dict(proofs=src.data_ptr()))
        if kind == "res":
            rc, c = eng.reserve_ptr("redeem_cbor" if wire else "redeem", ring, n, capi.MEM_DEVICE, **p)
        else:
            rc, c = eng.return_replay_ptr("redeem_cbor" if wire else "redeem", ring, n, capi.MEM_DEVICE, nonce_key=NONCE_KEY, sign_key=-1,
                                          returned=dt.data_ptr() if dt is not None else None, **p)
        st, blob, ok, rep = d.down(s, n), d.down(o, ob * n), d.down(k, n), d.down(r, n)
    assert rc == want_rc, (rc, eng.lib.act_last_error(eng.ctx))
    if rc == 0:
        assert all((st[i] == 0) == any(blob[ob * i:ob * i + ob]) for i in range(n)), "an accepted lane's slot is zero, or a failed lane's is not"
    return st, blob, ok, rep, c


def respelled(rec, canonical, pick):
    import pymodel as pm
    from test_cbor import _variants
    legal = [msg for msg, _ in _variants("SpendProof", rec, L) if pm.cbor_decode("SpendProof", msg, L) == (0, rec) and msg != canonical]
    return legal[pick % len(legal)]


class Lanes:
    """the World of tests/test_gpu_bound.py at L = 8 with a second proof per token (other rng bytes: the same nullifier, another K'),
    bound to the same binding, and the unbound twin of each"""

    def __init__(self, eng):
        self.w = w = World(eng, N, "bound-redeem")
        rng2 = shake("bound-redeem-pr2", eng.prove_rng_bytes * N)
        st, self.bound2, _ = eng.prove_spend(w.tok, w.s, rng2, bind=b"".join(w.binds))
        st2, self.plain2, _ = eng.prove_spend(w.tok, w.s, rng2)
        assert st == st2 == bytes(N)
        self.pb = w.pb

    def rec(self, t, bound=True, variant=0, tampered=False):
        blob = ((self.w.bound, self.bound2) if bound else (self.w.plain, self.plain2))[variant]
        p = bytearray(blob[self.pb * t:self.pb * (t + 1)])
        if tampered:
            p[self.pb - 32] ^= 1
        return bytes(p)


_lanes = {}


def setup(engine_factory, bench_params, mode):
    capi, eng = engine(engine_factory, bench_params, L, mode)
    if id(eng) not in _lanes:
        with step(120, "tokens and proofs"):
            _lanes[id(eng)] = Lanes(eng)
    return capi, eng, _lanes[id(eng)]


def sets(capi):
    return capi.NullifierSet(2000), capi.NullifierSet(2000)


def same(a, b):
    assert a[0] == b[0], ("statuses", [(i, x, y) for i, (x, y) in enumerate(zip(a[0], b[0])) if x != y])
    assert a[1] == b[1] and a[2] == b[2] and a[3] == b[3], "output bytes, out_key or replay marks"
    assert a[4] == b[4], ("counts", a[4], b[4])


# ---- 5. / 6. the mismatch matrix around the compaction, retries, the scenario of 4.11 -------------------------------------------------------
@pytest.mark.parametrize("mode,mem", MODES)
@pytest.mark.parametrize("wire", [False, True])
@pytest.mark.parametrize("kind", ["rr", "res"])
def test_a_bound_batch_is_answered_as_its_unbound_twins_and_every_survivor_meets_its_own_binding(engine_factory, bench_params, mode, mem, wire, kind):
    capi, eng, ln = setup(engine_factory, bench_params, mode)
    w, n = ln.w, 130
    epochs = [51, 52, 53]
    ring = w.ring3
    wrong_bind = {0, 63, 64, n - 1}                       # the first lane, both sides of the compaction's block of 64, the last lane
    wrong_charge = {1, 30, 62, 65, 100}
    foreign = {2, 31, 66, 101}                            # their nullifier is spent by the token's OTHER proof before the call
    binds = list(w.binds[:n])
    for i in wrong_bind:
        binds[i] = w.binds[(i + 1) % n]                   # another lane's binding
    charges = [S + 1 if i in wrong_charge else S for i in range(n)]
    ts = [(0, 1, S)[i % 3] for i in range(n)] if kind == "rr" else None
    a, b = sets(capi), sets(capi)
    pre = sorted(foreign)
    with step(60, "the foreign spends, recorded on both pairs of sets"):
        for (ns, rs), bound in ((a, True), (b, False)):
            got = call(eng, mem, kind, ns, rs, ring, [ln.rec(t, bound, 1) for t in pre], wire, bind=[w.binds[t] for t in pre] if bound else ABSENT,
                       returned=[0] * len(pre) if kind == "rr" else None, key_epochs=epochs)
            assert got[0] == bytes(len(pre))
    with step(90, "the bound batch, and its unbound twins through the call without a binding"):
        got = call(eng, mem, kind, a[0], a[1], ring, [ln.rec(t) for t in range(n)], wire, bind=binds, charges=charges, returned=ts, key_epochs=epochs)
        twin = call(eng, mem, kind, b[0], b[1], ring, [ln.rec(t, False, 0, tampered=t in wrong_bind) for t in range(n)], wire, charges=charges, returned=ts, key_epochs=epochs)
    want = [250 if i in wrong_charge else 3 if i in foreign else 7 if i in wrong_bind else 0 for i in range(n)]
    assert list(got[0]) == want and list(got[2]) == [255 if s else 2 for s in want] and got[3] == bytes(n)
    same(got, twin)
    assert got[4]["wrong_charge"] == 5 and got[4]["foreign_spend"] == 4 and got[4]["rejected_by_verification"] == 4 and got[4]["fresh"] == n - 13
    assert _pairs(a[0]) == _pairs(b[0]) and _pairs(a[1]) == _pairs(b[1])
    before = (_pairs(a[0]), _pairs(a[1]))
    served = [i for i in range(n) if want[i] == 0]
    with step(90, "a retry under the same bindings, then under other bindings"):
        again = call(eng, mem, kind, a[0], a[1], ring, [ln.rec(t) for t in range(n)], wire, bind=binds, charges=charges, returned=ts, key_epochs=epochs)
        assert list(again[0]) == want and again[1] == got[1] and again[2] == got[2]
        assert list(again[3]) == [1 if s == 0 else 0 for s in want] and (_pairs(a[0]), _pairs(a[1])) == before
        # DESIGN 4.11's scenario: the proof of a recorded spend presented beside another request is an invalid proof, not a replay
        moved = binds[1:] + binds[:1]
        other = call(eng, mem, kind, a[0], a[1], ring, [ln.rec(t) for t in served], wire, bind=[moved[t] for t in served], charges=[S] * len(served),
                     returned=[ts[t] for t in served] if ts else None, key_epochs=epochs)
        assert other[0] == b"\x07" * len(served) and other[2] == b"\xff" * len(served) and other[3] == bytes(len(served)) and not any(other[1])
        assert other[4]["retry_candidates"] == len(served) and other[4]["rejected_by_verification"] == len(served)
        assert (_pairs(a[0]), _pairs(a[1])) == before
        # ... and by the call without a binding, and an unbound proof by the bound call under the all-zero binding
        plain = call(eng, mem, kind, a[0], a[1], ring, [ln.rec(t) for t in served[:3]], wire, returned=[ts[t] for t in served[:3]] if ts else None, key_epochs=epochs)
        zero = call(eng, mem, kind, a[0], a[1], ring, [ln.rec(t, False) for t in served[:3]], wire, bind=[bytes(32)] * 3, returned=[ts[t] for t in served[:3]] if ts else None,
                    key_epochs=epochs)
        assert plain[0] == zero[0] == b"\x07" * 3 and (_pairs(a[0]), _pairs(a[1])) == before
    for x in a + b:
        x.close()
    assert eng.secret_residue() == 0


@pytest.mark.parametrize("mode,mem", MODES)
@pytest.mark.parametrize("wire", [False, True])
def test_reserve_and_settle_of_bound_proofs_is_the_bound_return_replay_call(engine_factory, bench_params, mode, mem, wire):
    capi, eng, ln = setup(engine_factory, bench_params, mode)
    w, n = ln.w, 65
    ring, epochs = w.ring3, [61, 62, 63]
    binds = list(w.binds[:n])
    binds[64] = w.binds[0]                                # one lane beside the wrong request
    ts = [(1, S - 1, S)[i % 3] for i in range(n)]
    recs = [ln.rec(t) for t in range(n)]
    a, b = sets(capi), sets(capi)
    with step(90, "reserve, settle, and the one-phase call"):
        res = call(eng, mem, "res", a[0], a[1], ring, recs, wire, bind=binds, charges=[S] * n, key_epochs=epochs)
        assert list(res[0]) == [0] * 64 + [7] and res[3] == bytes(n)
        two = call_settle(eng, mem, a[1], ring, [res[1][96 * i:96 * i + 96] for i in range(n)], res[2], ts, key_epochs=epochs, wire=wire)
        one = call(eng, mem, "rr", b[0], b[1], ring, recs, wire, bind=binds, charges=[S] * n, returned=ts, key_epochs=epochs)
    assert list(two[0]) == [0] * 64 + [248] and list(one[0]) == [0] * 64 + [7]
    assert two[4] == one[1] and res[2] == one[2]
    assert _pairs(a[0]) == _pairs(b[0])
    with step(60, "the client's retry after settlement is served by the bound one-phase call"):
        retry = call(eng, mem, "rr", a[0], a[1], ring, recs[:64], wire, bind=binds[:64], returned=ts[:64], key_epochs=epochs)
        ob = len(one[1]) // n
        assert retry[0] == bytes(64) and retry[3] == b"\1" * 64 and retry[1] == one[1][:ob * 64]
    for x in a + b:
        x.close()


# ---- 4. bind = NULL ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,mem", MODES)
@pytest.mark.parametrize("wire", [False, True])
@pytest.mark.parametrize("kind", ["rr", "res"])
def test_bind_null_is_the_call_it_extends(engine_factory, bench_params, mode, mem, wire, kind):
    """one mixed batch -- accepted, tampered, wrong charge, spent (a retry and a foreign spend) -- through the bound entry point with NULL
    and through the call it extends, on sets with the same history"""
    capi, eng, ln = setup(engine_factory, bench_params, mode)
    w, n = ln.w, 70
    ring, epochs = w.ring3, [71, 72, 73]
    recs = [ln.rec(t, False, tampered=t in (4, 64)) for t in range(n)]
    recs[7] = ln.rec(7)                                   # a bound proof: invalid for both
    charges = [S + 1 if t == 9 else S for t in range(n)]
    ts = [(0, 2, S + 1)[t % 3] if t != 0 else 1 for t in range(n)] if kind == "rr" else None
    a, b = sets(capi), sets(capi)
    with step(60, "history: a retry candidate and a foreign spend"):
        for ns, rs in (a, b):
            got = call(eng, mem, kind, ns, rs, ring, [ln.rec(0, False), ln.rec(1, False, 1)], wire, returned=[1, 0] if kind == "rr" else None, key_epochs=epochs)
            assert got[0] == bytes(2)
    with step(90, "NULL and the call without the argument"):
        null = call(eng, mem, kind, a[0], a[1], ring, recs, wire, bind=None, charges=charges, returned=ts, key_epochs=epochs)
        old = call(eng, mem, kind, b[0], b[1], ring, recs, wire, charges=charges, returned=ts, key_epochs=epochs)
    same(null, old)
    assert (old[0][0], old[3][0], old[0][1], old[0][4], old[0][7], old[0][9], old[0][64]) == (0, 1, 3, 7, 7, 250, 7)
    assert kind == "res" or old[0][2] == 249                  # t = s + 1
    assert _pairs(a[0]) == _pairs(b[0]) and _pairs(a[1]) == _pairs(b[1])
    with step(60, "nothing shed: the batch that goes straight to the replay implementation"):
        clean = [ln.rec(t, False) for t in range(100, 110)]
        null = call(eng, mem, kind, a[0], a[1], ring, clean, wire, bind=None, returned=[1] * 10 if kind == "rr" else None, key_epochs=epochs)
        old = call(eng, mem, kind, b[0], b[1], ring, clean, wire, returned=[1] * 10 if kind == "rr" else None, key_epochs=epochs)
        same(null, old)
        assert old[0] == bytes(10) and _pairs(a[0]) == _pairs(b[0]) and _pairs(a[1]) == _pairs(b[1])
    for x in a + b:
        x.close()


# ---- nothing shed, bound: the road that hands the caller's pointers to the replay implementation ---------------------------------------------------
@pytest.mark.parametrize("mode,mem", MODES)
@pytest.mark.parametrize("wire", [False, True])
def test_an_honest_bound_batch_and_the_host_reader(engine_factory, bench_params, mode, mem, wire):
    capi, eng, ln = setup(engine_factory, bench_params, mode)
    w, n = ln.w, 66
    ring = w.ring3
    recs, twins = [ln.rec(t) for t in range(n)], [ln.rec(t, False) for t in range(n)]
    for reader in ((capi.WIRE_READER_DEVICE, capi.WIRE_READER_HOST) if wire else (capi.WIRE_READER_DEVICE,)):
        a, b = sets(capi), sets(capi)
        try:
            eng.set_wire_reader(reader)
            with step(90, "every lane fresh and under its own binding"):
                got = call(eng, mem, "rr", a[0], a[1], ring, recs, wire, bind=w.binds[:n], charges=[S] * n, returned=[1] * n, respell=(3, 64, 65))
                twin = call(eng, mem, "rr", b[0], b[1], ring, twins, wire, charges=[S] * n, returned=[1] * n, respell=(3, 64, 65))
        finally:
            eng.set_wire_reader(capi.WIRE_READER_DEVICE)
        same(got, twin)
        assert got[0] == bytes(n) and got[2] == b"\2" * n and got[4]["fresh"] == n
        assert _pairs(a[0]) == _pairs(b[0]) and _pairs(a[1]) == _pairs(b[1])
        for x in a + b:
            x.close()


# ---- 7. no unique form ----------------------------------------------------------------------------------------------------------------------------
def test_the_bound_form_with_unique_is_refused_and_the_python_layer(engine_factory, bench_params):
    from act_amd import api
    capi, eng, ln = setup(engine_factory, bench_params, "host")
    w = ln.w
    ns, rs = sets(capi)
    with pytest.raises(capi.ActError):
        eng.redeem_return_replay(ns, rs, w.ring3, ln.rec(0), NONCE_KEY, unique=True, bind=w.binds[0])
    assert len(ns) == 0 and len(rs) == 0
    params = api.Params(bench_params)
    ring = api.Keyring([api.PrivateKey(k) for k in w.ring3])
    db, receipts = api.NullifierDb(1000), api.NullifierDb(1000)
    proofs = [api.SpendProof(ln.rec(t), L) for t in range(3)]
    with pytest.raises(ValueError):
        ring.redeem_replay_batch(params, db, receipts, proofs, NONCE_KEY, admit=True, unique=True, binds=w.binds[:3])
    with pytest.raises(ValueError):
        ring.redeem_replay_batch(params, db, receipts, proofs, NONCE_KEY, binds=w.binds[:3])
    with step(60, "the Python layer"):
        st, idx = ring.verify_spend_batch(params, proofs, binds=w.binds[:3])
        assert (st, idx) == (bytes(3), [2, 2, 2]) and ring.verify_spend_batch(params, proofs)[0] == b"\x07" * 3
        res, idx, rep = ring.redeem_replay_batch(params, db, receipts, proofs, NONCE_KEY, admit=True, returned=[1, 1, 1], binds=[w.binds[0], w.binds[0], w.binds[2]])
        assert isinstance(res[0], api.RefundReturn) and isinstance(res[1], api.Error) and isinstance(res[2], api.RefundReturn) and idx == [2, None, 2]
        res2, rep2 = ring.reserve_batch(params, db, receipts, [api.SpendProof(ln.rec(t), L) for t in (10, 11)], binds=[w.binds[10], w.binds[10]])
        assert isinstance(res2[0], api.Reservation) and isinstance(res2[1], api.Error) and rep2 == [False, False]
        tok = api.CreditToken(w.tok[:160])
        proof, _ = tok.prove_spend(params, SPEND, api.ByteStreamRng(w.rng[:eng.prove_rng_bytes]), nbits=L, bind=w.binds[0])
        assert proof.record == ln.rec(0)
    ns.close(); rs.close()
