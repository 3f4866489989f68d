"""The return calls with the copy stage, on the GPU: act_redeem_return_unique_batch / act_redeem_cbor_return_unique_batch through the C
ABI against hand-written expectations (the fixed mixes of tests/copies_cases.py with return lanes behind them), against the model of
tests/return_ring_cases.py and -- the identity of the header -- byte for byte against act_redeem_(cbor_)return_batch on the same batch
and an identical set: statuses, out_key, every output byte, the exported set with its epochs and the generator's draws, under all three
rng conventions, batches whose copies carry different t included.  L = 8; 21 / 27 lanes, 65 and 300."""
import numpy as np
import pytest

import admission_cases as ad
import copies_cases as cp
import return_ring_cases as rc
from conftest import shake, scb
from test_gpu_admission import Dev, World, step, _le, _mode, _pairs
from test_gpu_copies import call as call_admit_unique, pair_of_sets
from test_gpu_refund_return import records_of, refunds_of

pytestmark = pytest.mark.gpu

L, MAX_BATCH = 8, 1024
MEMS = [("host", "host"), ("host", "device"), ("device", "host"), ("device", "device")]


def call(eng, mem, ns, ring, n, unique, blob=None, msgs=None, charges=None, returned=None, rng=b"", rng_mode=0, sign_key=-1, key_epochs=None):
    """one return call, unique form or not, in either memory kind and either form -> (statuses, out bytes, out_key, counts)"""
    from act_amd import capi
    wire = msgs is not None
    ob = eng.cbor_size("RefundReturn") if wire else 160
    if mem == "host":
        if wire:
            st, out, ok, c = eng.redeem_cbor_return(ns, ring, msgs, rng, rng_mode, sign_key, charges, returned, key_epochs, unique=unique)
            return st, b"".join(x if x else bytes(ob) for x in out), ok, c
        return eng.redeem_return(ns, ring, blob, rng, rng_mode, sign_key, charges, returned, key_epochs, unique=unique)
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
             key_epochs=key_epochs, sign_key=sign_key, unique=unique)
    if wire:
        c = eng.return_ptr("redeem_cbor", ring, n, capi.MEM_DEVICE, cbor=src.data_ptr(), offsets=offs.ctypes.data, **p)
    else:
        c = eng.return_ptr("redeem", ring, n, capi.MEM_DEVICE, proofs=src.data_ptr(), **p)
    return d.down(st, n), d.down(out, ob * n), d.down(ok, n), c


_worlds = {}


def world(eng, tag, owners):
    if tag not in _worlds:
        _worlds[tag] = World(eng, tag, owners)
    return _worlds[tag]


def engine(engine_factory, bench_params, mode):
    from act_amd import capi
    return engine_factory(bench_params, L, max_batch=MAX_BATCH, transcript=_mode(capi, mode))


def gens(rng, rng_mode):
    from act_amd import capi
    return (capi.ReplayRng(rng), capi.ReplayRng(rng)) if rng_mode == capi.RNG_CALLBACK else (rng, rng)


def assert_same_answers(a, b, sa, sb, ga, gb, rng_mode):
    """check 1: (statuses, out, out_key) of the unique call and of the plain return call, the two sets with epochs, the two generators;
    only the counts differ"""
    from act_amd import capi
    assert a[0] == b[0] and a[2] == b[2], ("statuses / out_key differ", list(a[0]), list(b[0]))
    assert a[1] == b[1], "output bytes differ"
    assert _pairs(sa) == _pairs(sb) and len(sa) == len(sb)
    if rng_mode == capi.RNG_CALLBACK:
        assert ga.draws == gb.draws and ga.pos == gb.pos
    ca, cb = a[3], b[3]
    assert tuple(ca) == rc.COUNTS_UNIQUE and tuple(cb) == rc.COUNTS_RETURN
    assert all(ca[k] == cb[k] for k in ("lanes", "wire_rejected", "wrong_charge", "return_too_big", "spent_before", "accepted"))
    assert cb["verified"] - ca["verified"] == ca["copies"]
    rc.check_identities(ca)          # check 2: verified = lanes - wire_rejected - wrong_charge - return_too_big - spent_before - copies


# ---- the fixed mixes with return lanes -----------------------------------------------------------------------------------------------------
def fixed_mix(eng, w, wire):
    t = {name: i for i, name in enumerate(rc.RETURN_TOKENS)}
    how = {"a": (0, None), "b": (1, None), "x": (0, "tampered"), "u": (0, "undecodable"), "i": (0, "identity")}
    mix = [(tok, proof) for tok, proof, _, _ in cp.FIXED_MIX + (cp.FIXED_WIRE_EXTRA if wire else [])] + [(tok, proof) for tok, proof, _ in rc.RETURN_LANES]
    recs = [w.proof(t[tok], *how[proof.split("/")[0]]).tobytes() for tok, proof in mix]
    if not wire:
        return recs, None
    msgs = eng.cbor_encode("SpendProof", b"".join(recs))
    for i, (_, proof) in enumerate(mix):
        if proof.endswith("/respelled"):
            msgs[i] = ad.respelled(recs[i], L)
        elif proof.endswith("/trailing"):
            msgs[i] = msgs[i] + b"\0"
    return recs, msgs


@pytest.mark.parametrize("mode,mem", MEMS)
def test_fixed_lane_mix_hand_written(engine_factory, bench_params, mode, mem):
    from act_amd import capi
    rc.check_model_on_fixed_mix()
    eng = engine(engine_factory, bench_params, mode)
    with step(120, "tokens and proofs"):
        w = world(eng, "ru-fix", [0] * len(rc.RETURN_TOKENS))
    t = {name: i for i, name in enumerate(rc.RETURN_TOKENS)}
    for wire in (False, True):
        lanes, blobs, charges, returned, base = rc.fixed_lanes(wire)
        est, eok, ecopy, ec = rc.fixed_expect(wire)
        recs, msgs = fixed_mix(eng, w, wire)
        n = len(recs)
        assert n == len(lanes) == (27 if wire else 21)
        kw = dict(msgs=msgs) if wire else dict(blob=b"".join(recs))
        cc, tt = b"".join(scb(c) for c in charges), b"".join(scb(x) for x in returned)
        rng = shake("ru-fix-rng", 128 * n)
        for rng_mode in (capi.RNG_PER_LANE, capi.RNG_SEQUENTIAL, capi.RNG_CALLBACK):
            with step(60, "fixed mix, wire=%s rng=%d" % (wire, rng_mode)):
                sa, sb = pair_of_sets([w.k[t[name]] for name in cp.FIXED_SPENT])
                ga, gb = gens(rng, rng_mode)
                a = call(eng, mem, sa, [w.keys[0]], n, True, charges=cc, returned=tt, rng=ga, rng_mode=rng_mode, **kw)
                b = call(eng, mem, sb, [w.keys[0]], n, False, charges=cc, returned=tt, rng=gb, rng_mode=rng_mode, **kw)
            st, out, ok, c = a
            print("unique   ", list(st), c)
            assert list(st) == est and list(ok) == eok and c == ec, (wire, rng_mode)
            assert_same_answers(a, b, sa, sb, ga, gb, rng_mode)
            if rng_mode == capi.RNG_CALLBACK:
                assert ga.draws == [128 * c["accepted"]]               # a copy draws nothing
            got = records_of(eng, wire, out, n)
            for i in range(n):
                assert any(got[160 * i:160 * i + 160]) == (st[i] == 0), i      # a copy's record is all zero, whatever its leader got
                if st[i] == 0:
                    assert got[160 * i + 128:160 * i + 160] == scb(returned[i]), i      # every signed lane over its OWN t
            # the return lanes: the copy whose t differs and the copy with t = 0 are double spends of leaders signed over t = 1 and t = s;
            # the lane with its leader's bytes and t = s + 1 was shed at the screen
            assert [st[base + j] for j in range(5)] == [0, 3, 0, 249, 3] and [returned[base + j] for j in (0, 2)] == [1, ad.SPEND]
            if wire:      # a respelled copy is a leader of its own: verified, then a double spend from the set
                assert (st[18], st[19], ecopy[19]) == (0, 3, None) and c["double_spend_after"] == 3
            assert len(sa) == len(cp.FIXED_SPENT) + c["accepted"]
            sa.close(); sb.close()
        # check 3: returned == NULL -- the admission unique form's counts, and its records in the first 128 bytes
        with step(60, "nothing returned, wire=%s" % wire):
            sa, sb = pair_of_sets([w.k[t[name]] for name in cp.FIXED_SPENT])
            a = call(eng, mem, sa, [w.keys[0]], n, True, charges=cc, returned=None, rng=rng, rng_mode=capi.RNG_PER_LANE, **kw)
            rc_, ust, uout, uok, uc = call_admit_unique(eng, mem, sb, [w.keys[0]], n, True, charges=cc, rng=rng, rng_mode=capi.RNG_PER_LANE, **kw)
        assert rc_ == 0 and a[0] == ust and a[2] == uok and _pairs(sa) == _pairs(sb)
        assert [a[3][k] for k in ad.COUNTS] == [uc[k] for k in ad.COUNTS] and a[3]["copies"] == uc["copies"] and a[3]["return_too_big"] == 0
        got, want = records_of(eng, wire, a[1], n), refunds_of(eng, wire, uout, n)
        for i in range(n):
            assert got[160 * i:160 * i + 128] == want[128 * i:128 * i + 128] and got[160 * i + 128:160 * i + 160] == bytes(32), i
        sa.close(); sb.close()
    assert eng.secret_residue() == 0


# ---- the seeded plans ----------------------------------------------------------------------------------------------------------------------
N_TOKENS = 300
RING, EPOCHS = [1, 0], [101, 100]     # token t was issued under key t % 2: ring index 1 - t % 2


def plan_world(eng):
    w = world(eng, "ru-plan", [t % 2 for t in range(N_TOKENS)])
    if not hasattr(w, "rows"):
        tampered = w.proofs[0].copy(); tampered[:, w.pb - 32] ^= 1
        w.rows = {(0, False): w.proofs[0], (1, False): w.proofs[1], (0, True): tampered}
        ml = eng.cbor_size("SpendProof")
        enc = lambda arr: np.frombuffer(b"".join(eng.cbor_encode("SpendProof", arr.tobytes())), np.uint8).reshape(N_TOKENS, ml)
        w.wire_rows = {k: enc(v) for k, v in w.rows.items()}
    return w


@pytest.mark.parametrize("mode,mem,wire", [("host", "host", False), ("device", "device", False), ("host", "device", True), ("device", "host", True)])
def test_equal_to_the_plain_return_call(engine_factory, bench_params, mode, mem, wire):
    from act_amd import capi
    rc.check_model_on_plans()
    eng = engine(engine_factory, bench_params, mode)
    with step(300, "tokens and proofs"):
        w = plan_world(eng)
    for n in rc.PLAN_NS:
        rng = shake("ru-plan-rng", 128 * n)
        for num, den in cp.FRACTIONS:
            for rng_mode in (capi.RNG_CALLBACK, capi.RNG_SEQUENTIAL, capi.RNG_PER_LANE):
                with_charges = rng_mode != capi.RNG_SEQUENTIAL
                plan, tokens = cp.copy_plan(n, num, den, cp.plan_seed(num, den), with_charges)
                assert tokens <= N_TOKENS
                key_of = lambda p: RING.index(p.token % 2)
                lanes, blobs, charges, spent = cp.plan_lanes(plan, nullifier=lambda t: w.k[t], key=key_of)
                returned = rc.plan_returned(plan, cp.plan_seed(num, den))
                ch = charges if with_charges else None
                mst, mok, mc, mrec, msigned, mcopy = rc.model_unique(lanes, blobs, returned, spent, ch)
                src = w.wire_rows if wire else w.rows
                rows = np.stack([src[(p.variant, p.tampered)][p.token] for p in plan])
                kw = dict(msgs=[r.tobytes() for r in rows]) if wire else dict(blob=rows.tobytes())
                kw.update(charges=b"".join(scb(c) for c in charges) if with_charges else None, returned=b"".join(scb(x) for x in returned), rng_mode=rng_mode,
                          key_epochs=EPOCHS)
                ring = [w.keys[k] for k in RING]
                with step(120, "n %d copies %d/%d rng=%d" % (n, num, den, rng_mode)):
                    sa, sb = pair_of_sets(sorted(spent), epochs=(11, 12, 13), cap=3 * n + 64)
                    ga, gb = gens(rng, rng_mode)
                    a = call(eng, mem, sa, ring, n, True, rng=ga, **kw)
                    b = call(eng, mem, sb, ring, n, False, rng=gb, **kw)
                print("n %d copies %d/%d rng=%d:" % (n, num, den, rng_mode), a[3])
                assert_same_answers(a, b, sa, sb, ga, gb, rng_mode)
                if rng_mode == capi.RNG_CALLBACK:
                    assert ga.draws == ([128 * mc["accepted"]] if mc["accepted"] else [])
                # and the model: counts, every status, every key index, what was recorded under which epoch, every signed lane's own t
                assert a[3] == mc and a[3]["copies"] == sum(1 for x in mcopy if x is not None), (a[3], mc)
                assert list(a[0]) == mst and list(a[2]) == mok
                assert len(sa) == len(spent) + mc["accepted"]
                assert {(int.from_bytes(k, "little"), e) for k, e in _pairs(sa)} >= {(k, EPOCHS[key]) for k, key in mrec}
                got = records_of(eng, wire, a[1], n)
                for i in range(n):
                    assert any(got[160 * i:160 * i + 160]) == (i in msigned), i
                    if i in msigned:
                        assert got[160 * i + 128:160 * i + 160] == scb(msigned[i]), i
                sa.close(); sb.close()
    assert eng.secret_residue() == 0


# ---- one fresh proof sent 300 times with 300 different amounts ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mem,wire", [("device", False), ("host", False), ("device", True), ("host", True)])
def test_flood_of_one_proof_with_different_amounts(engine_factory, bench_params, mem, wire):
    """check 4: verified == 1, lane 0 is signed over its own t, 299 x DoubleSpendError.  The token holds 700 and spends 600 (the range
    proof is over the 100 that stay), so 300 different t <= s exist."""
    from act_amd import capi
    eng = engine(engine_factory, bench_params, "device")
    n, credit, spend = 300, 700, 600
    with step(120, "one token"):
        sk = eng.private_key_random(shake("ru-flood-sk", 64))
        pre = eng.pre_issuance_random(shake("ru-flood-pre", 128)); req = eng.request(pre, shake("ru-flood-rq", 128))
        st, resp = eng.issue(sk, req, scb(credit), shake("ru-flood-ir", 128))
        assert st == bytes(1)
        st, tok = eng.issuance_to_credit_token(pre, sk[32:], req, resp)
        assert st == bytes(1)
        st, proof, prer = eng.prove_spend_seeded(tok, scb(spend), shake("ru-flood-seed", 32))
        assert st == bytes(1)
    returned = [(7 * i + 5) % (spend + 1) for i in range(n)]
    assert len(set(returned)) == n and max(returned) <= spend
    row = eng.cbor_encode("SpendProof", proof)[0] if wire else proof
    kw = dict(msgs=[row] * n) if wire else dict(blob=row * n)
    with step(120, "flood"):
        sa, sb = pair_of_sets([], cap=1000)
        g = capi.ReplayRng(shake("ru-flood", 128 * 4))
        st, out, ok, c = call(eng, mem, sa, [sk], n, True, charges=scb(spend) * n, returned=b"".join(scb(x) for x in returned), rng=g, rng_mode=capi.RNG_CALLBACK, **kw)
    print("flood:", c)
    assert c == dict(lanes=n, wire_rejected=0, wrong_charge=0, spent_before=0, return_too_big=0, copies=n - 1, verified=1, rejected_by_verification=0,
                     double_spend_after=0, accepted=1)
    assert st == b"\0" + bytes([3]) * (n - 1) and ok == b"\0" * n and g.draws == [128] and len(sa) == 1
    got = records_of(eng, wire, out, n)
    assert got[128:160] == scb(returned[0]) and not any(got[160:])
    # the client holds what lane 0 was told
    cst, new = eng.refund_to_credit_token_return(prer, proof, got[:160], sk[32:])
    assert cst == bytes(1) and new[128:160] == scb(credit - spend + returned[0])
    sa.close(); sb.close()
    assert eng.secret_residue() == 0


def test_python_api_unique():
    """api.PrivateKey / api.Keyring: unique=True gives what unique=False gives on the same batch, copies with different amounts included"""
    from act_amd import api
    params = api.Params.new("test-org", "test-service", "test", "2024-01-01")
    with step(240, "api round trip"):
        rng = api.ByteStreamRng(shake("ru-api", 1 << 20))
        sk = api.PrivateKey.random(rng, params)
        proofs = []
        for spend in (5, 7):
            pre = api.PreIssuance.random(rng, params)
            req = pre.request(params, rng)
            tok = pre.to_credit_token(params, sk.public(), req, sk.issue(params, req, 20, rng))
            proofs.append(tok.prove_spend(params, spend, rng)[0])
        batch = [proofs[0], proofs[0], proofs[1], proofs[0], proofs[1], proofs[1]]
        charges = [5, 5, 8, 5, 7, 7]
        returned = [2, 4, 0, 6, 7, 1]          # lane 3: its leader's bytes and t > s -- shed, not a copy
        got = []
        for unique in (False, True):
            db = api.NullifierDb(1000)
            r = api.ByteStreamRng(shake("ru-api-sign", 1 << 16))
            res = sk.redeem_return_batch(params, db, batch, r, returned=returned, charges=charges, unique=unique)
            ring = api.Keyring([sk], epochs=[9])
            db2 = api.NullifierDb(1000)
            res2, matched = ring.redeem_return_cbor_batch(params, db2, [p.to_cbor(params) for p in batch], r, returned=returned, charges=charges, unique=unique)
            assert tuple(ring.last_return_counts) == (rc.COUNTS_UNIQUE if unique else rc.COUNTS_RETURN) and ring.last_return_counts is ring.last_admit_counts
            if unique:
                assert ring.last_return_counts["copies"] == 2 and ring.last_return_counts["verified"] == 2 and ring.last_return_counts["return_too_big"] == 1
            got.append(([x.record if isinstance(x, api.RefundReturn) else ("error", x.code, x.name) for x in res],
                        [x if isinstance(x, bytes) else ("error", x.code) for x in res2], matched, len(db), len(db2), db2.epoch_len(9)))
        assert got[0] == got[1]
        assert [x[1] if isinstance(x, tuple) else 0 for x in got[1][0]] == [0, 3, 250, 249, 0, 3] and got[1][2] == [0, 0, None, None, 0, 0]
        assert got[1][0][0][128:] == api.scalar(2) and got[1][0][4][128:] == api.scalar(7)
