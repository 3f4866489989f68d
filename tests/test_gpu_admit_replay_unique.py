"""The replay unique forms on the GPU: act_redeem_admit_replay_unique_batch / act_redeem_cbor_admit_replay_unique_batch through the C
ABI against hand-written expectations (the fixed lane mix), against the model of tests/admit_replay_unique_cases.py, and -- the theorem
of the header -- byte for byte against act_redeem_(cbor_)admit_replay_batch on the same batch and identical sets: rc, statuses,
out_key, every output byte, every replay mark and both exported sets with their epochs.  L = 8 and max_batch = 1024, so that the 8 209
lanes of the large runs cross the 4 096-lane gather windows and a copy's leader lies in an earlier window.  The tokens are those of
tests/test_gpu_replay.py (its World: two proofs per token with the same nullifier and another K', the prover's PreRefunds kept).  Every
step runs under a time limit of its own.

Rates are measured by tools/admit_replay_copies_probe.py; the tests here assert behaviour only."""
import numpy as np
import pytest

import admission_cases as ad
import admit_replay_unique_cases as aru
from conftest import scb
from test_gpu_replay import MODES, NONCE_KEY, SPEND, Dev, World, _pairs, call_replay, step

pytestmark = pytest.mark.gpu

L, MAX_BATCH = 8, 1024
N = aru.PLAN_N
N_TOKENS = 3700                       # every plan spends fewer (asserted below)
FLOOD = 4099
EPOCHS = [101, 100]
GUARD = 0xA5
assert SPEND == aru.SPEND


def engine(engine_factory, bench_params, mode):
    from act_amd import capi
    return engine_factory(bench_params, L, max_batch=MAX_BATCH, transcript=capi.TRANSCRIPT_HOST if mode == "host" else capi.TRANSCRIPT_DEVICE)


_world = []


def world(eng):
    """tokens and proofs are bytes that do not depend on the transcript mode: made once"""
    if not _world:
        with step(300, "tokens and proofs"):
            w = World(eng, N_TOKENS)
            tampered = w.proofs[0].copy(); tampered[:, w.pb - 32] ^= 1
            w.rows = {(0, False): w.proofs[0], (1, False): w.proofs[1], (0, True): tampered}
            ml = eng.cbor_size("SpendProof")
            enc = lambda arr: np.frombuffer(b"".join(eng.cbor_encode("SpendProof", arr.tobytes())), np.uint8).reshape(N_TOKENS, ml)
            w.wire_rows = {k: enc(v) for k, v in w.rows.items()}
            _world.append(w)
    return _world[0]


def call(eng, mem, ns, rs, ring, unique, blob=None, msgs=None, charges=None, sign_key=-1, key_epochs=None, want_rc=0, lead_pad=0, out_pad=0):
    """one call, unique form or not, in either memory kind and either form -> (rc, statuses, output bytes, out_key, replayed, counts).
    Device memory: the first message starts lead_pad bytes and the output out_pad bytes into its allocation; the output allocation
    ends in 16 more bytes, and everything around the n rows must come back as it went in"""
    from act_amd import capi
    wire = msgs is not None
    n = len(msgs) if wire else len(blob) // eng.proof_bytes
    ob = eng.cbor_size("Refund") if wire else 128
    cc = b"".join(scb(c) for c in charges) if charges is not None else None
    if mem == "host":
        assert not lead_pad and not out_pad
        if wire:
            rc, st, out, ok, rep, c = eng.redeem_cbor_admit_replay(ns, rs, ring, msgs, NONCE_KEY, sign_key, key_epochs, cc, raw=True, unique=unique)
            out = b"".join(m if m else bytes(ob) for m in out)
        else:
            rc, st, out, ok, rep, c = eng.redeem_admit_replay(ns, rs, ring, blob, NONCE_KEY, sign_key, key_epochs, cc, raw=True, unique=unique)
    else:
        d = Dev()
        src = d.up(bytes(lead_pad) + (b"".join(msgs) if wire else blob))
        dc = d.up(cc) if cc is not None else None
        offs = np.zeros(n + 1, np.uint64)
        if wire:
            offs[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
        o, s, k, r = d.new(out_pad + ob * n + 16, GUARD), d.new(n, 99), d.new(n, 77), d.new(n, 55)
        d.t.cuda.synchronize()
        p = dict(set=ns, receipts=rs, nonce_key=NONCE_KEY, out=o.data_ptr() + out_pad, status=s.data_ptr(), out_key=k.data_ptr(), replayed=r.data_ptr(),
                 key_epochs=key_epochs, sign_key=sign_key, charges=dc.data_ptr() if dc is not None else None, raw=True, unique=unique)
        if wire:
            rc, c = eng.admit_replay_ptr("redeem_cbor", ring, n, capi.MEM_DEVICE, cbor=src.data_ptr() + lead_pad, offsets=offs.ctypes.data, **p)
        else:
            rc, c = eng.admit_replay_ptr("redeem", ring, n, capi.MEM_DEVICE, proofs=src.data_ptr(), **p)
        whole = d.down(o, out_pad + ob * n + 16)
        assert whole[:out_pad] == bytes([GUARD]) * out_pad and whole[out_pad + ob * n:] == bytes([GUARD]) * 16, "bytes around the output rows were written"
        st, out, ok, rep = d.down(s, n), whole[out_pad:out_pad + ob * n], d.down(k, n), d.down(r, n)
    assert rc == want_rc, (rc, eng.lib.act_last_error(eng.ctx))
    if rc == 0:
        assert all(st[i] == 0 or not any(out[ob * i:ob * i + ob]) for i in range(n)), "a failed lane's record is not zero"
    return rc, st, out, ok, rep, c


def twin_sets(eng, mem, ring, w, tokens, tmp_path, key_epochs=None, cap=3 * N):
    """variant 0 of `tokens` redeemed by one replay call; both sets saved once and restored twice -> two identical (set, receipts) pairs"""
    from act_amd import capi
    ns, rs = capi.NullifierSet(cap), capi.NullifierSet(cap)
    if tokens:
        got = call_replay(eng, mem, ns, rs, ring, recs=[w.proof(t) for t in tokens], key_epochs=key_epochs)
        assert got[0] == bytes(len(tokens))
    ns.save(str(tmp_path / "set.snap")); rs.save(str(tmp_path / "receipts.snap"))
    ns.close(); rs.close()
    return [(capi.NullifierSet.restore(str(tmp_path / "set.snap"), cap), capi.NullifierSet.restore(str(tmp_path / "receipts.snap"), cap)) for _ in range(2)]


def assert_the_theorem(a, b, sets, copy_of):
    """a: the unique call, b: act_redeem_(cbor_)admit_replay_batch on the same batch; sets: the pair each of them ran on"""
    assert a[0] == b[0], "rc differs"
    assert a[1] == b[1] and a[3] == b[3], "statuses / out_key differ"
    assert a[2] == b[2], "output bytes differ"
    assert a[4] == b[4], "replay marks differ"
    assert _pairs(sets[0][0]) == _pairs(sets[1][0]) and _pairs(sets[0][1]) == _pairs(sets[1][1]), "the sets differ"
    assert set(a[5]) == set(aru.COUNTS) and set(b[5]) == set(aru.ar.COUNTS)
    aru.check_identities(a[5])
    aru.check_count_relation(a[5], b[5], list(a[1]), copy_of)


# ---- 6. the fixed lane mix: hand-written expectations ----------------------------------------------------------------------------------------
TOKEN_OF = {name: i for i, name in enumerate(aru.FIXED_TOKENS)}
HOW = {"a": (0, None), "b": (1, None), "x": (0, "tampered")}


def fixed_mix(eng, w, wire):
    assert all(w.owner[TOKEN_OF[name]] == aru.FIXED_OWNER[name] for name in aru.FIXED_TOKENS)
    mix = aru.FIXED_MIX + (aru.FIXED_WIRE_EXTRA if wire else [])
    recs = [w.proof(TOKEN_OF[tok], *HOW[proof.split("/")[0]]) for tok, proof, _, _ in mix]
    charges = [SPEND if right else aru.EXPECTED_WRONG for _, _, _, right in mix]
    if not wire:
        return recs, None, charges
    msgs = eng.cbor_encode("SpendProof", b"".join(recs))
    for i, (_, proof, _, _) in enumerate(mix):
        if proof.endswith("/respelled"):
            msgs[i] = ad.respelled(recs[i], L)
        elif proof.endswith("/trailing"):
            msgs[i] = msgs[i] + b"\0"
    assert msgs[14] != msgs[0] and msgs[15] != msgs[0] and msgs[1] == msgs[0]
    return recs, msgs, charges


def run_fixed_mix(eng, w, mem, wire, tmp_path, lead_pad=0, out_pad=0):
    recs, msgs, charges = fixed_mix(eng, w, wire)
    n = len(recs)
    kw = dict(msgs=msgs) if wire else dict(blob=b"".join(recs))
    sets = twin_sets(eng, mem, w.keys, w, [TOKEN_OF[name] for name in aru.FIXED_SPENT], tmp_path, cap=1000)
    a = call(eng, mem, sets[0][0], sets[0][1], w.keys, True, charges=charges, lead_pad=lead_pad, out_pad=out_pad, **kw)
    rc, st, out, ok, rep, c = a
    print("unique   ", list(st), list(rep), c)
    assert (list(st), list(ok), list(rep)) == (aru.FIXED_EXPECT[:n], aru.FIXED_KEYS[:n], aru.FIXED_REPLAYED[:n])
    assert c == (aru.FIXED_COUNTS_WIRE if wire else aru.FIXED_COUNTS_RECORDS)
    ob = len(out) // n
    row = lambda i: out[ob * i:ob * i + ob]
    for i in range(n):
        assert any(row(i)) == (st[i] == 0), i
        if aru.FIXED_COPY_OF[i] is not None:
            assert row(i) == row(aru.FIXED_COPY_OF[i]), i          # the leader's record, byte for byte -- or its all-zero one
    assert row(0) != row(3) and row(0) != row(9)
    if wire:
        assert row(14) == row(15) == row(0)                         # another spelling, a trailing byte: verified, replayed, the same Refund
    b = call(eng, mem, sets[1][0], sets[1][1], w.keys, False, charges=charges, lead_pad=lead_pad, out_pad=out_pad, **kw)
    assert_the_theorem(a, b, sets, aru.FIXED_COPY_OF[:n])
    assert len(sets[0][0]) == len(sets[0][1]) == len(aru.FIXED_SPENT) + c["fresh"]
    for s, r in sets:
        s.close(); r.close()
    return a


@pytest.mark.parametrize("mode,mem", MODES)
def test_fixed_lane_mix_hand_written(engine_factory, bench_params, tmp_path, mode, mem):
    aru.check_model_on_fixed_mix()
    eng = engine(engine_factory, bench_params, mode)
    w = world(eng)
    for wire in (False, True):
        with step(60, "fixed mix, wire=%s" % wire):
            run_fixed_mix(eng, w, mem, wire, tmp_path)
    assert eng.secret_residue() == 0


# ---- 7. the theorem on the seeded plans --------------------------------------------------------------------------------------------------------
# (copy share, with charges, sign_key): both shares with and without charges, sign_key matched and fixed
CASES = [(1, 2, False, -1), (1, 2, True, 0), (7, 8, False, 0), (7, 8, True, -1)]


@pytest.mark.parametrize("mode,mem,wire", [("host", "host", False), ("device", "device", False), ("host", "device", True), ("device", "host", True)])
def test_equal_to_the_admit_replay_call(engine_factory, bench_params, tmp_path, mode, mem, wire):
    eng = engine(engine_factory, bench_params, mode)
    w = world(eng)
    ring = w.keys                                                   # token t was issued under key t % 2
    for num, den, with_charges, sign_key in CASES:
        plan, tokens = aru.copy_plan(N, num, den, aru.plan_seed(num, den), with_charges)
        assert tokens <= N_TOKENS
        lanes, blobs, charges, spent, receipts = aru.plan_lanes(plan, nullifier=lambda t: w.k[t], key=lambda p: w.owner[p.token])
        ch = charges if with_charges else None
        mst, mok, mrep, mc, mcopy = aru.model(lanes, blobs, set(spent), set(receipts), ch)
        # asserted on the model's output before anything is compared (tests/test_admit_replay_unique_host.py chose the seeds)
        cats, ds = aru.categories_of(mst, mrep, mcopy)
        assert aru.categories_are_full(cats, ds, N), (num, den, with_charges, cats, ds)
        src = w.wire_rows if wire else w.rows
        rows = np.stack([src[(p.variant, p.tampered)][p.token] for p in plan])
        kw = dict(msgs=[r.tobytes() for r in rows]) if wire else dict(blob=rows.tobytes())
        kw.update(charges=ch, sign_key=sign_key, key_epochs=EPOCHS)
        with step(120, "copies %d/%d charges=%s sign_key=%d" % (num, den, with_charges, sign_key)):
            sets = twin_sets(eng, mem, ring, w, sorted({p.token for p in plan if p.spent}), tmp_path, key_epochs=EPOCHS)
            assert len(sets[0][0]) == len(sets[0][1]) == len(spent)
            a = call(eng, mem, sets[0][0], sets[0][1], ring, True, **kw)
            b = call(eng, mem, sets[1][0], sets[1][1], ring, False, **kw)
            print("copies %d/%d charges=%s sign_key=%d:" % (num, den, with_charges, sign_key), a[5])
            # the shares again, on what the GPU answered
            cats, ds = aru.categories_of(list(a[1]), list(a[4]), mcopy)
            assert aru.categories_are_full(cats, ds, N), (cats, ds)
            assert_the_theorem(a, b, sets, mcopy)
            # and the model: every status, every key index, every replay mark, the counts
            assert (list(a[1]), list(a[3]), list(a[4])) == (mst, mok, mrep)
            assert a[5] == mc, (a[5], mc)
            assert len(sets[0][0]) == len(spent) + mc["fresh"] == len(sets[0][1])
            ob = len(a[2]) // N
            lanes_of = np.frombuffer(a[2], np.uint8).reshape(N, ob)
            copies = [i for i in range(N) if mcopy[i] is not None]
            assert (lanes_of[copies] == lanes_of[[mcopy[i] for i in copies]]).all()      # (also part of the theorem; said directly)
            assert any(mcopy[i] // 4096 != i // 4096 for i in copies)                    # a leader in an earlier window
            for s, r in sets:
                s.close(); r.close()
    assert eng.secret_residue() == 0


# ---- 8. floods ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem,wire", [("device", False), ("host", False), ("device", True), ("host", True)])
def test_floods(engine_factory, bench_params, mem, wire):
    from act_amd import capi
    eng = engine(engine_factory, bench_params, "device")
    w = world(eng)
    ring, t = w.keys, 4                                             # token 4: key 0
    src = w.wire_rows if wire else w.rows
    zero = dict.fromkeys(aru.COUNTS, 0)
    row = src[(0, False)][t].tobytes()
    kw = dict(msgs=[row] * FLOOD) if wire else dict(blob=row * FLOOD)
    ns, rs = capi.NullifierSet(3 * FLOOD), capi.NullifierSet(3 * FLOOD)
    with step(60, "one fresh proof %d times" % FLOOD):
        eng.prof_enable(True); eng.prof_reset()
        rc, st, out, ok, rep, c = call(eng, mem, ns, rs, ring, True, **kw)
        prof = eng.prof()
        eng.prof_enable(False)
        assert c == dict(zero, lanes=FLOOD, verified=1, fresh=1, copies=FLOOD - 1, copies_served=FLOOD - 1)
        assert prof["k_spend_bits"]["lanes"] == L                   # one verification
        ob = len(out) // FLOOD
        first = out[:ob]
        assert st == bytes(FLOOD) and ok == bytes(FLOOD) and rep == b"\0" + b"\1" * (FLOOD - 1) and any(first) and out == first * FLOOD
        refund = eng.cbor_decode("Refund", [first])[1] if wire else first
        cst, _ = eng.refund_to_credit_token(w.prerefunds[0][t].tobytes(), w.proof(t), refund, ring[0][32:])
        assert cst == b"\0"                                         # PreRefund.to_credit_token accepts it: all 4 099 are these bytes
        assert (len(ns), len(rs)) == (1, 1)
    with step(60, "the same flood again: one already-served proof"):
        rc, st, out2, ok, rep, c = call(eng, mem, ns, rs, ring, True, **kw)
        assert c == dict(zero, lanes=FLOOD, retry_candidates=FLOOD, verified=1, replayed=1, copies=FLOOD - 1, copies_served=FLOOD - 1)
        assert st == bytes(FLOOD) and rep == b"\1" * FLOOD and out2 == out and (len(ns), len(rs)) == (1, 1)
    ns.close(); rs.close()
    row = src[(0, True)][t + 2].tobytes()
    kw = dict(msgs=[row] * FLOOD) if wire else dict(blob=row * FLOOD)
    ns, rs = capi.NullifierSet(3 * FLOOD), capi.NullifierSet(3 * FLOOD)
    with step(60, "one tampered proof %d times" % FLOOD):
        eng.prof_enable(True); eng.prof_reset()
        rc, st, out, ok, rep, c = call(eng, mem, ns, rs, ring, True, **kw)
        prof = eng.prof()
        eng.prof_enable(False)
        assert c == dict(zero, lanes=FLOOD, verified=1, rejected_by_verification=1, copies=FLOOD - 1)
        assert prof["k_spend_bits"]["lanes"] == L
        assert st == bytes([7]) * FLOOD and ok == b"\xff" * FLOOD and rep == bytes(FLOOD) and not any(out) and (len(ns), len(rs)) == (0, 0)
    ns.close(); rs.close()
    assert eng.secret_residue() == 0


# ---- 9. alignment on the device, wire form -------------------------------------------------------------------------------------------------------
def test_wire_rows_one_byte_into_their_allocations(engine_factory, bench_params, tmp_path):
    eng = engine(engine_factory, bench_params, "device")
    w = world(eng)
    with step(60, "aligned"):
        want = run_fixed_mix(eng, w, "device", True, tmp_path)
    with step(60, "messages and output 1 byte into their allocations"):
        got = run_fixed_mix(eng, w, "device", True, tmp_path, lead_pad=1, out_pad=1)      # (call() checks the bytes around the rows)
    assert got == want
    with step(60, "the flood's 4 098 row moves at an odd address"):
        from act_amd import capi
        row = w.wire_rows[(0, False)][9].tobytes()
        outs = []
        for pad in (0, 1, 3):
            ns, rs = capi.NullifierSet(3 * FLOOD), capi.NullifierSet(3 * FLOOD)
            outs.append(call(eng, "device", ns, rs, w.keys, True, msgs=[row] * FLOOD, lead_pad=pad, out_pad=pad))
            ns.close(); rs.close()
        assert outs[0] == outs[1] == outs[2] and outs[0][5]["copies_served"] == FLOOD - 1
    assert eng.secret_residue() == 0


# ---- 10. a failed signature step -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["host", "device"])
def test_failed_signatures_on_a_batch_with_copies(engine_factory, bench_params, mem):
    from act_amd import capi
    eng = engine(engine_factory, bench_params, "host")
    w = world(eng)
    ring = w.keys
    toks = [0, 1, 0, 2, 1, 1, 3, 2, 0]                             # lanes 2, 4, 5, 7, 8 repeat an earlier lane
    blob = b"".join(w.rows[(0, t == 3)][t].tobytes() for t in toks)      # token 3 is tampered
    zero = dict.fromkeys(aru.COUNTS, 0)
    ns, rs = capi.NullifierSet(1000), capi.NullifierSet(1000)
    with step(60, "the signature step fails behind the recorded nullifiers"):
        assert eng.lib.act_debug_fail_next_signs(eng.ctx, 1) == 0
        rc, st, out, ok, rep, c = call(eng, mem, ns, rs, ring, True, blob=blob, want_rc=2)
        # leaders: recorded, not signed; their copies say the same and are repaired by the same retry; the tampered lane as ever
        assert list(st) == [251, 251, 251, 251, 251, 251, 7, 251, 251] and list(ok) == [0, 1, 0, 0, 1, 1, 255, 0, 0]
        assert not any(out) and rep == bytes(9) and (len(ns), len(rs)) == (3, 3)
        assert c == dict(zero, lanes=9, verified=4, rejected_by_verification=1, unanswered=3, copies=5)
    with step(60, "the same lanes again: every one is served, one verification per proof"):
        rc, st, out, ok, rep, c = call(eng, mem, ns, rs, ring, True, blob=blob)
        assert list(st) == [0, 0, 0, 0, 0, 0, 7, 0, 0] and list(rep) == [1, 1, 1, 1, 1, 1, 0, 1, 1] and list(ok) == [0, 1, 0, 0, 1, 1, 255, 0, 0]
        assert c == dict(zero, lanes=9, retry_candidates=8, verified=4, rejected_by_verification=1, replayed=3, copies=5, copies_served=5)
        rows = [out[128 * i:128 * i + 128] for i in range(9)]
        assert rows[2] == rows[8] == rows[0] and rows[4] == rows[5] == rows[1] and rows[7] == rows[3] and len({rows[0], rows[1], rows[3]}) == 3
        for i in (0, 1, 3):
            t = toks[i]
            assert eng.refund_to_credit_token(w.prerefunds[0][t].tobytes(), w.proof(t), rows[i], ring[w.owner[t]][32:])[0] == b"\0"
        assert (len(ns), len(rs)) == (3, 3)
    with step(60, "refused calls write no counts"):
        rc, st, out, ok, rep, c = call(eng, mem, ns, rs, ring, True, blob=blob, sign_key=4, want_rc=1)
        assert c == zero and st == bytes([99]) * 9
        assert call(eng, mem, ns, ns, ring, True, blob=blob, want_rc=1)[5] == zero
    ns.close(); rs.close()
    assert eng.secret_residue() == 0


# ---- 11. the Python layer ------------------------------------------------------------------------------------------------------------------------
def test_the_python_api_with_unique_gives_what_the_capi_call_gives(engine_factory, bench_params):
    from act_amd import api
    eng = engine(engine_factory, bench_params, "host")
    w = world(eng)
    params = api.Params(bench_params)
    ring = api.Keyring([api.PrivateKey(k) for k in w.keys], epochs=[11, 12])
    # tokens 0..2 are redeemed before: a retry and its copy, a foreign spend twice, two fresh proofs and a copy, a copy at the wrong price
    toks = [(0, 0), (0, 0), (1, 1), (1, 1), (80, 0), (81, 0), (80, 0), (81, 0)]
    charges = [SPEND] * 7 + [SPEND + 1]
    with step(120, "api and capi on sets with the same history"):
        dbs = [(api.NullifierDb(1 << 10), api.NullifierDb(1 << 10)) for _ in range(2)]
        for db, receipts in dbs:
            res, _, _ = ring.redeem_replay_batch(params, db, receipts, [api.SpendProof(w.proof(t), L) for t in range(3)], NONCE_KEY)
            assert all(isinstance(r, api.Refund) for r in res)
        proofs = [api.SpendProof(w.proof(t, v), L) for t, v in toks]
        res, keys, rep = ring.redeem_replay_batch(params, dbs[0][0], dbs[0][1], proofs, NONCE_KEY, admit=True, charges=charges, unique=True)
        st, out, ok, crep, c = eng.redeem_admit_replay(dbs[1][0].set, dbs[1][1].set, w.keys, b"".join(w.proof(t, v) for t, v in toks), NONCE_KEY, key_epochs=[11, 12],
                                                       charges=b"".join(scb(x) for x in charges), unique=True)
        assert list(st) == [0, 0, 3, 3, 0, 0, 0, 250] and [r.code if isinstance(r, api.Error) else 0 for r in res] == list(st)
        assert [r.record for r in res if isinstance(r, api.Refund)] == [out[128 * i:128 * i + 128] for i in range(8) if st[i] == 0]
        assert rep == [bool(b) for b in crep] == [True, True, False, False, False, False, True, False] and ring.last_replay_counts == c
        assert keys == [0, 0, None, None, 0, 1, 0, None]
        assert len(c) == 13 and (c["copies"], c["copies_served"], c["verified"], c["foreign_spend"], c["wrong_charge"]) == (2, 2, 3, 2, 1)
        msgs = [p.to_cbor(params) for p in proofs]
        out2, _, rep2 = ring.redeem_replay_cbor_batch(params, dbs[0][0], dbs[0][1], msgs, NONCE_KEY, L, admit=True, unique=True)
        assert rep2 == [True, True, False, False, True, True, True, True] and ring.last_replay_counts["copies"] == 3
        assert [o for o in out2 if isinstance(o, bytes)] == eng.cbor_encode("Refund", b"".join(out[128 * i:128 * i + 128] for i in (0, 1, 4, 5, 6, 5)))
        for bad in (ring.redeem_replay_batch, ring.redeem_replay_cbor_batch):
            with pytest.raises(ValueError):
                bad(params, dbs[0][0], dbs[0][1], proofs if bad == ring.redeem_replay_batch else msgs, NONCE_KEY, unique=True)
