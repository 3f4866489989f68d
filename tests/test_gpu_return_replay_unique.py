"""The return replay unique forms on the GPU: act_redeem_return_replay_unique_batch / act_redeem_cbor_return_replay_unique_batch through
the C ABI, held -- the promise of the header -- byte for byte to act_redeem_(cbor_)return_replay_batch on the same batch and identical
pairs of sets: rc, statuses, out_key, every output byte, every replay mark and both exported sets with their epochs; to the
hand-written expectations of tests/return_replay_unique_cases.py for the fixed mixes and to its model on the seeded plans (65 lanes, one
wavefront plus one, and 300, at copy shares 0, 1/2 and 7/8); and at amounts NULL and all zero to
act_redeem_(cbor_)admit_replay_unique_batch.  The tokens are those of tests/test_gpu_replay.py (its World: L = 8, 257 tokens that spend
s = 3, two proofs each with the same nullifier and another K').  Both memory kinds, records and wire.  Every step runs under a time
limit of its own."""
import numpy as np
import pytest

import admission_cases as ad
import return_replay_unique_cases as ru
from conftest import ELL, scb
from test_gpu_refund_return import records_of
from test_gpu_replay import CREDIT, L, NONCE_KEY, SPEND, Dev, _pairs, setup, step

pytestmark = pytest.mark.gpu

MODES = [("host", "host"), ("device", "device")]                  # (transcripts, caller's memory): both of each
S = SPEND
GUARD = 0xA5
NULL = "null"
assert S == ru.S


def call(eng, mem, ns, rs, ring, unique, recs=None, msgs=None, charges=None, returned=None, sign_key=-1, key_epochs=None, want_rc=0, lead_pad=0, out_pad=0):
    """one call, unique form or not, in either memory kind and either form; returned: a list of ints (unreduced values allowed), NULL or
    None (both: a null pointer) -> (rc, statuses, output bytes, out_key, replayed, counts).  Device memory: the first message starts
    lead_pad bytes and the output out_pad bytes into its allocation; the output allocation ends in 16 more bytes, and everything around
    the n rows must come back as it went in"""
    from act_amd import capi
    wire = msgs is not None
    n = len(msgs) if wire else len(recs)
    ob = eng.cbor_size("RefundReturn") if wire else 160
    cc = b"".join(scb(c) for c in charges) if charges is not None else None
    tt = None if returned is None or returned == NULL else b"".join(int(t).to_bytes(32, "little") for t in returned)
    if mem == "host":
        assert not lead_pad and not out_pad
        if wire:
            rc, st, out, ok, rep, c = eng.redeem_cbor_return_replay(ns, rs, ring, msgs, NONCE_KEY, sign_key, key_epochs, cc, tt, raw=True, unique=unique)
            out = b"".join(x if x else bytes(ob) for x in out)
        else:
            rc, st, out, ok, rep, c = eng.redeem_return_replay(ns, rs, ring, b"".join(recs), NONCE_KEY, sign_key, key_epochs, cc, tt, raw=True, unique=unique)
    else:
        d = Dev()
        src = d.up(bytes(lead_pad) + (b"".join(msgs) if wire else b"".join(recs)))
        dc = d.up(cc) if cc is not None else None
        dt = d.up(tt) if tt is not None else None
        offs = np.zeros(n + 1, np.uint64)
        if wire:
            offs[1:] = np.cumsum([len(x) for x in msgs], dtype=np.uint64)
        o, s, k, r = d.new(out_pad + ob * n + 16, GUARD), d.new(n, 99), d.new(n, 77), d.new(n, 55)
        d.t.cuda.synchronize()
        p = dict(set=ns, receipts=rs, nonce_key=NONCE_KEY, out=o.data_ptr() + out_pad, status=s.data_ptr(), out_key=k.data_ptr(), replayed=r.data_ptr(),
                 key_epochs=key_epochs, sign_key=sign_key, charges=dc.data_ptr() if dc is not None else None, returned=dt.data_ptr() if dt is not None else None,
                 raw=True, unique=unique)
        if wire:
            rc, c = eng.return_replay_ptr("redeem_cbor", ring, n, capi.MEM_DEVICE, cbor=src.data_ptr() + lead_pad, offsets=offs.ctypes.data, **p)
        else:
            rc, c = eng.return_replay_ptr("redeem", ring, n, capi.MEM_DEVICE, proofs=src.data_ptr() + lead_pad, **p)
        whole = d.down(o, out_pad + ob * n + 16)
        if rc != 1:
            assert whole[:out_pad] == bytes([GUARD]) * out_pad and whole[out_pad + ob * n:] == bytes([GUARD]) * 16, "bytes around the output rows were written"
        st, out, ok, rep = d.down(s, n), whole[out_pad:out_pad + ob * n], d.down(k, n), d.down(r, n)
    assert rc == want_rc, (rc, eng.lib.act_last_error(eng.ctx))
    if rc == 0:
        assert all((st[i] == 0) == any(out[ob * i:ob * i + ob]) for i in range(n)), "a failed lane's record is not zero, or an accepted lane's is"
    return rc, st, out, ok, rep, c


def twin_sets(eng, mem, ring, capi, recs, amounts, tmp_path, key_epochs=None, pairs=2, cap=2000):
    """`recs` redeemed for `amounts` by one return replay call; both sets saved once and restored -> identical (set, receipts) pairs"""
    ns, rs = capi.NullifierSet(cap), capi.NullifierSet(cap)
    if recs:
        got = call(eng, mem, ns, rs, ring, False, recs=recs, returned=amounts, key_epochs=key_epochs)
        assert got[1] == bytes(len(recs))
    ns.save(str(tmp_path / "set.snap")); rs.save(str(tmp_path / "receipts.snap"))
    ns.close(); rs.close()
    return [(capi.NullifierSet.restore(str(tmp_path / "set.snap"), cap), capi.NullifierSet.restore(str(tmp_path / "receipts.snap"), cap)) for _ in range(pairs)]


def close(sets):
    for s, r in sets:
        s.close(); r.close()


def assert_the_promise(a, b, sets, copy_of):
    """a: the unique call, b: act_redeem_(cbor_)return_replay_batch on the same batch; sets: the pair each of them ran on"""
    assert a[0] == b[0], "rc differs"
    assert a[1] == b[1], ("statuses differ", list(a[1]), list(b[1]))
    assert a[3] == b[3], ("out_key differs", list(a[3]), list(b[3]))
    assert a[2] == b[2], "output bytes differ"
    assert a[4] == b[4], ("replay marks differ", list(a[4]), list(b[4]))
    assert _pairs(sets[0][0]) == _pairs(sets[1][0]) and _pairs(sets[0][1]) == _pairs(sets[1][1]), "the sets differ"
    assert tuple(a[5]) == ru.COUNTS and tuple(b[5]) == ru.rr.COUNTS
    ru.check_identities(a[5])
    ru.check_count_relation(a[5], b[5], list(a[1]), copy_of)


# ---- 1. the fixed mixes: hand-written expectations, and the promise -------------------------------------------------------------------------
TOK = dict(P=(10, 0, None), Q=(10, 1, None), X=(11, 0, "tampered"), R=(1, 0, None), Z=(13, 0, None))      # 10: key 0; 1 and 13: key 1
SP_TOKEN, SP_AMOUNT = 1, 2


def mix_bytes(eng, w, mix, wire):
    recs = [w.proof(*TOK[blob]) for _, blob, _ in mix]
    return dict(msgs=eng.cbor_encode("SpendProof", b"".join(recs))) if wire else dict(recs=recs)


def run_mix(eng, capi, w, mem, wire, tmp_path, name, lead_pad=0, out_pad=0):
    mix, want = ru.FIXED[name]
    n = len(mix)
    assert all(w.owner[TOK[blob][0]] == lane.key for lane, blob, _ in mix if lane.verdict == 0)
    returned = [t for _, _, t in mix]
    kw = dict(mix_bytes(eng, w, mix, wire), charges=[S] * n, returned=returned, key_epochs=[7, 8], lead_pad=lead_pad, out_pad=out_pad)
    sets = twin_sets(eng, mem, w.keys, capi, [w.proof(SP_TOKEN)], [SP_AMOUNT], tmp_path, key_epochs=[7, 8])
    a = call(eng, mem, sets[0][0], sets[0][1], w.keys, True, **kw)
    b = call(eng, mem, sets[1][0], sets[1][1], w.keys, False, **kw)
    print(name, "unique", list(a[1]), list(a[3]), list(a[4]), a[5])
    assert [(a[1][i], a[3][i], a[4][i]) for i in range(n)] == [x[:3] for x in want], name
    copy_of = [x[3] for x in want]
    assert_the_promise(a, b, sets, copy_of)
    ob = len(a[2]) // n
    row = lambda i: a[2][ob * i:ob * i + ob]
    ts = [t % ELL for t in returned]
    for i, l in enumerate(copy_of):
        if l is not None:
            assert row(i) == (row(l) if a[1][i] == 0 else bytes(ob)), (name, i)
            assert (a[1][i] == 0) == (a[1][l] == 0 and ts[i] == ts[l]), (name, i)
    assert a[5]["copies"] == sum(1 for l in copy_of if l is not None)
    assert a[5]["copies_other_amount"] == sum(1 for i, l in enumerate(copy_of) if l is not None and ts[i] != ts[l])
    close(sets)
    return a


@pytest.mark.parametrize("mode,mem", MODES)
@pytest.mark.parametrize("wire", [False, True])
def test_fixed_mixes_hand_written_and_equal_to_the_return_replay_call(engine_factory, bench_params, tmp_path, mode, mem, wire):
    ru.check_model_on_fixed_mixes()
    capi, eng, w = setup(engine_factory, bench_params, mode)
    for name in ru.FIXED:
        with step(60, "%s, wire=%s" % (name, wire)):
            a = run_mix(eng, capi, w, mem, wire, tmp_path, name)
        if name == "t + l":                                         # the served copy's RefundReturn: the client takes it
            recs = records_of(eng, wire, a[2], 3)
            assert recs[160:320] == recs[:160] and recs[128:160] == scb(2)
            t = TOK["P"][0]
            cst, tok = eng.refund_to_credit_token_return(w.prerefunds[0][t].tobytes(), w.proof(t), recs[160:320], w.keys[w.owner[t]][32:])
            assert cst == b"\0" and tok[128:160] == scb(CREDIT - S + 2)
    assert eng.secret_residue() == 0


@pytest.mark.parametrize("mode,mem", MODES)
def test_two_spellings_of_one_message_are_not_copies(engine_factory, bench_params, tmp_path, mode, mem):
    capi, eng, w = setup(engine_factory, bench_params, mode)
    rec = w.proof(20)
    canon, other = eng.cbor_encode("SpendProof", rec)[0], ad.respelled(rec, L)
    assert canon != other
    msgs, returned = [canon, other, other, canon, other + b"\0"], [1, 1, 2, 1 + ELL, 1]
    with step(60, "canonical, respelled twice, canonical, trailing byte"):
        sets = twin_sets(eng, mem, w.keys, capi, [], [], tmp_path)
        a = call(eng, mem, sets[0][0], sets[0][1], w.keys, True, msgs=msgs, returned=returned)
        b = call(eng, mem, sets[1][0], sets[1][1], w.keys, False, msgs=msgs, returned=returned)
        # lane 1 is another spelling: verified, replayed; lane 2 copies lane 1 and names another amount; lane 3 copies lane 0; lane 4 is verified
        assert (list(a[1]), list(a[4])) == ([0, 0, 3, 0, 0], [0, 1, 0, 1, 1])
        assert_the_promise(a, b, sets, [None, None, 1, 0, None])
        assert (a[5]["verified"], a[5]["copies"], a[5]["copies_served"], a[5]["copies_other_amount"], a[5]["replayed"]) == (3, 2, 1, 1, 2)
        close(sets)
    assert eng.secret_residue() == 0


# ---- 2. a failed signature step: a 251 leader with a copy of each kind ----------------------------------------------------------------------------
@pytest.mark.parametrize("mode,mem", MODES)
def test_failed_signatures_are_answered_as_the_return_replay_call_answers_them(engine_factory, bench_params, tmp_path, mode, mem):
    capi, eng, w = setup(engine_factory, bench_params, mode)
    toks, returned = [30, 30, 30, 31, 30, 1, 1], [2, 2, 1, S, 2 + ELL, SP_AMOUNT, SP_AMOUNT]
    recs = [w.proof(t) for t in toks]
    copy_of = [None, 0, 0, None, 0, None, 5]
    with step(60, "the signature step fails behind the recorded nullifiers, in both calls"):
        sets = twin_sets(eng, mem, w.keys, capi, [w.proof(SP_TOKEN)], [SP_AMOUNT], tmp_path)
        assert eng.lib.act_debug_fail_next_signs(eng.ctx, 1) == 0
        a = call(eng, mem, sets[0][0], sets[0][1], w.keys, True, recs=recs, returned=returned, want_rc=2)
        assert eng.lib.act_debug_fail_next_signs(eng.ctx, 1) == 0
        b = call(eng, mem, sets[1][0], sets[1][1], w.keys, False, recs=recs, returned=returned, want_rc=2)
        # the fresh leader and the retry that leads: recorded, not signed; the same amount says the same, another amount is a double spend
        assert list(a[1]) == [251, 251, 3, 251, 251, 251, 251] and not any(a[2])
        assert_the_promise(a, b, sets, copy_of)
        assert (a[5]["unanswered"], a[5]["copies"], a[5]["copies_served"], a[5]["copies_other_amount"], a[5]["verified"]) == (3, 4, 0, 1, 3)
    with step(60, "the same lanes again: every lane that named the recorded amount is served"):
        a = call(eng, mem, sets[0][0], sets[0][1], w.keys, True, recs=recs, returned=returned)
        b = call(eng, mem, sets[1][0], sets[1][1], w.keys, False, recs=recs, returned=returned)
        assert list(a[1]) == [0, 0, 3, 0, 0, 0, 0] and list(a[4]) == [1, 1, 0, 1, 1, 1, 1]
        # lane 2 is shed by the screen now (k is spent, no receipt for its amount): neither leader nor copy
        assert_the_promise(a, b, sets, [None, 0, None, None, 0, None, 5])
        assert a[2][160:320] == a[2][:160] == a[2][640:800] and a[5]["foreign_spend"] == 1
        close(sets)
    assert eng.secret_residue() == 0


# ---- 3. a wire output base at an odd address -----------------------------------------------------------------------------------------------------
def test_wire_rows_one_byte_into_their_allocations(engine_factory, bench_params, tmp_path):
    capi, eng, w = setup(engine_factory, bench_params, "device")
    for name in ("t1 t1 t2", "retry leads"):
        with step(60, name):
            want = run_mix(eng, capi, w, "device", True, tmp_path, name)
            for pad in (1, 3):
                got = run_mix(eng, capi, w, "device", True, tmp_path, name, lead_pad=pad, out_pad=pad)      # (call() checks the bytes around the rows)
                assert got == want
    assert eng.secret_residue() == 0


# ---- 4. the promise and the model on the seeded plans --------------------------------------------------------------------------------------------
def plan_rows(eng, w, plan, wire):
    recs = [w.proof(p.token, p.variant, "tampered" if p.tampered else None) for p in plan]
    return dict(msgs=eng.cbor_encode("SpendProof", b"".join(recs))) if wire else dict(recs=recs)


@pytest.mark.parametrize("mode,mem,wire", [("host", "host", False), ("device", "device", False), ("host", "device", True), ("device", "host", True)])
@pytest.mark.parametrize("n", ru.PLAN_SIZES)
def test_equal_to_the_return_replay_call_on_the_seeded_plans(engine_factory, bench_params, tmp_path, mode, mem, wire, n):
    capi, eng, w = setup(engine_factory, bench_params, mode)
    ring, epochs = w.keys, [101, 100]
    for num, den in ru.FRACTIONS:
        seed = ru.plan_seed(n, num, den)
        assert ru.plan_is_mixed_enough(n, num, den, seed)           # asserted on the model's output before anything is compared
        plan, tokens = ru.copy_plan(n, num, den, seed)
        assert tokens <= w.n
        lanes, blobs, charges, returned, spent, receipts = ru.plan_lanes(plan, nullifier=lambda t: w.k[t], key=lambda p: w.owner[p.token])
        mst, mok, mrep, mc, mcopy = ru.model(lanes, blobs, set(spent), set(receipts), charges, returned)
        pre = sorted({p.token for p in plan if p.spent})
        kw = dict(plan_rows(eng, w, plan, wire), charges=charges, returned=returned, key_epochs=epochs, sign_key=-1 if num else 0)
        with step(120, "%d lanes, copies %d/%d" % (n, num, den)):
            sets = twin_sets(eng, mem, ring, capi, [w.proof(t) for t in pre], [ru.spent_amount(t) for t in pre], tmp_path, key_epochs=epochs)
            assert len(sets[0][0]) == len(sets[0][1]) == len(spent)
            a = call(eng, mem, sets[0][0], sets[0][1], ring, True, **kw)
            b = call(eng, mem, sets[1][0], sets[1][1], ring, False, **kw)
            print("%d lanes, copies %d/%d:" % (n, num, den), a[5])
            assert_the_promise(a, b, sets, mcopy)
            # and the model: every status, every key index, every replay mark, the counts
            assert (list(a[1]), list(a[3]), list(a[4])) == (mst, mok, mrep)
            assert a[5] == mc, (a[5], mc)
            assert len(sets[0][0]) == len(spent) + mc["fresh"] == len(sets[0][1])
            ob = len(a[2]) // n
            rows = np.frombuffer(a[2], np.uint8).reshape(n, ob)
            served = [i for i in range(n) if mcopy[i] is not None and mst[i] == 0]
            assert (rows[served] == rows[[mcopy[i] for i in served]]).all()      # (also part of the promise; said directly)
            close(sets)
    assert eng.secret_residue() == 0


# ---- 5. nothing returned: the replay unique forms ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,mem,wire", [("host", "host", False), ("device", "device", False), ("device", "device", True), ("host", "host", True)])
def test_nothing_returned_is_the_admit_replay_unique_call(engine_factory, bench_params, tmp_path, mode, mem, wire):
    from test_gpu_admit_replay_unique import call as call_aru
    capi, eng, w = setup(engine_factory, bench_params, mode)
    n, ring = 65, w.keys
    plan, _ = ru.copy_plan(n, 1, 2, ru.plan_seed(n, 1, 2))
    rows = plan_rows(eng, w, plan, wire)
    charges = [S + 1 if p.wrong else S for p in plan]
    pre = sorted({p.token for p in plan if p.spent})
    with step(120, "NULL, all zero (as 0 and as l), and the call without amounts"):
        sets = twin_sets(eng, mem, ring, capi, [w.proof(t) for t in pre], [0] * len(pre), tmp_path, pairs=4)
        null = call(eng, mem, sets[0][0], sets[0][1], ring, True, charges=charges, returned=NULL, **rows)
        zero = call(eng, mem, sets[1][0], sets[1][1], ring, True, charges=charges, returned=[0] * n, **rows)
        ells = call(eng, mem, sets[2][0], sets[2][1], ring, True, charges=charges, returned=[ELL] * n, **rows)
        old = call_aru(eng, mem, sets[3][0], sets[3][1], ring, True, charges=charges, **(dict(msgs=rows["msgs"]) if wire else dict(blob=b"".join(rows["recs"]))))
    from test_gpu_refund_return import refunds_of
    want = refunds_of(eng, wire, old[2], n)
    assert old[5]["copies"] > 8 and old[5]["copies_served"] > 2 and old[5]["foreign_spend"] > 0
    for got in (null, zero, ells):
        assert (got[0], got[1], got[3], got[4]) == (old[0], old[1], old[3], old[4])
        assert {k: v for k, v in got[5].items() if k not in ("return_too_big", "copies_other_amount")} == old[5]
        assert got[5]["return_too_big"] == got[5]["copies_other_amount"] == 0
        rec = records_of(eng, wire, got[2], n)
        for i in range(n):
            assert rec[160 * i:160 * i + 128] == want[128 * i:128 * i + 128] and rec[160 * i + 128:160 * i + 160] == bytes(32), i
    assert all(_pairs(sets[0][j]) == _pairs(sets[k][j]) for k in (1, 2, 3) for j in (0, 1))
    close(sets)
    assert eng.secret_residue() == 0


# ---- 6. refusals and the straight road ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["host", "device"])
def test_whole_call_refusals_write_nothing_and_a_batch_without_copies(engine_factory, bench_params, mem):
    capi, eng, w = setup(engine_factory, bench_params, "device")
    n, ring = 5, w.keys
    recs = [w.proof(40 + t) for t in range(n)]
    zero = dict.fromkeys(ru.COUNTS, 0)
    ns, rs = capi.NullifierSet(1000), capi.NullifierSet(1000)
    with step(60, "receipts == set; a sign_key outside the ring"):
        for bad in (dict(rs_=ns), dict(sign_key=4)):
            got = call(eng, mem, ns, bad.get("rs_", rs), ring, True, recs=recs, returned=[1] * n, sign_key=bad.get("sign_key", -1), want_rc=1)
            assert got[1] == bytes([99]) * n and got[5] == zero and (len(ns), len(rs)) == (0, 0)
    with step(60, "no copies, nothing shed"):
        got = call(eng, mem, ns, rs, ring, True, recs=recs, returned=[1, 2, 3, 0, 1])
        assert got[1] == bytes(n) and got[4] == bytes(n) and got[5] == dict(zero, lanes=n, verified=n, fresh=n) and (len(ns), len(rs)) == (n, n)
        again = call(eng, mem, ns, rs, ring, True, recs=recs, returned=[1, 2, 3, 0, 1])
        assert again[2] == got[2] and again[4] == b"\1" * n and again[5] == dict(zero, lanes=n, retry_candidates=n, verified=n, replayed=n)
    ns.close(); rs.close()
    assert eng.secret_residue() == 0


# ---- 7. the Python layer -------------------------------------------------------------------------------------------------------------------------------
def test_the_python_api_gives_what_the_capi_call_gives(engine_factory, bench_params):
    from act_amd import api
    capi, eng, w = setup(engine_factory, bench_params, "host")
    params = api.Params(bench_params)
    ring = api.Keyring([api.PrivateKey(k) for k in w.keys], epochs=[11, 12])
    toks, ts = [50, 50, 50, 51, 51, 52], [1, 1, 2, S, S + 1, 0]
    with step(120, "api and capi on fresh sets"):
        dbs = [(api.NullifierDb(1 << 10), api.NullifierDb(1 << 10)) for _ in range(2)]
        proofs = [api.SpendProof(w.proof(t), L) for t in toks]
        res, keys, rep = ring.redeem_return_replay_unique_batch(params, dbs[0][0], dbs[0][1], proofs, NONCE_KEY, returned=ts, charges=[S] * 6)
        st, out, ok, crep, c = eng.redeem_return_replay(dbs[1][0].set, dbs[1][1].set, w.keys, b"".join(w.proof(t) for t in toks), NONCE_KEY, key_epochs=[11, 12],
                                                        charges=scb(S) * 6, returned=b"".join(scb(t) for t in ts), unique=True)
        assert list(st) == [0, 0, 3, 0, 249, 0] and [r.code if isinstance(r, api.Error) else 0 for r in res] == list(st)
        assert [r.record for r in res if isinstance(r, api.RefundReturn)] == [out[160 * i:160 * i + 160] for i in range(6) if st[i] == 0]
        assert rep == [bool(x) for x in crep] == [False, True, False, False, False, False] and ring.last_replay_counts == c
        assert (c["copies"], c["copies_served"], c["copies_other_amount"], c["return_too_big"], c["verified"]) == (2, 1, 1, 1, 3) and len(c) == 15
        msgs = [p.to_cbor(params) for p in proofs]
        out2, _, rep2 = ring.redeem_return_replay_unique_cbor_batch(params, dbs[0][0], dbs[0][1], msgs, NONCE_KEY, L, returned=[1, 1, 1, S, S, 0])
        assert rep2 == [True] * 6 and ring.last_replay_counts["copies"] == 3 and out2[2] == out2[0] and out2[4] == out2[3]
        one, marks = ring.keys[0].redeem_return_replay_unique_batch(params, api.NullifierDb(1 << 10), api.NullifierDb(1 << 10), proofs[:2], NONCE_KEY, returned=[1, 1])
        assert one[0].record == one[1].record == out[:160] and marks == [False, True]
        with pytest.raises(ValueError):
            ring.redeem_replay_batch(params, dbs[0][0], dbs[0][1], proofs, NONCE_KEY, unique=True, returned=ts)
