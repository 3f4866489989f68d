"""Admission's copy stage on the GPU: act_redeem_admit_unique_batch / act_redeem_cbor_admit_unique_batch through the C ABI against
hand-written expectations (the fixed lane mix), against the model of tests/copies_cases.py, and -- the theorem of the header -- byte
for byte against act_redeem_(cbor_)admit_batch on the same batch and an identical set: statuses, out_key, every output byte, the
exported set with its epochs and the generator's draws.  L = 8 and max_batch = 1024, so that the 8 209 lanes of the large runs cross
several gather windows and a copy's leader lies in an earlier window.  Every step runs under a time limit of its own.

Rates are measured by tools/copies_probe.py; the tests here assert behaviour only."""
import numpy as np
import pytest

import admission_cases as ad
import copies_cases as cp
from conftest import shake, scb
from test_gpu_admission import Dev, World, step, _le, _mode, _pairs

pytestmark = pytest.mark.gpu

L, MAX_BATCH = 8, 1024
MEMS = [("host", "host"), ("host", "device"), ("device", "host"), ("device", "device")]


def call(eng, mem, ns, ring, n, unique, blob=None, msgs=None, charges=None, rng=b"", rng_mode=0, sign_key=-1, key_epochs=None, raw=False, lead_pad=0):
    """one admission call, unique form or not, in either memory kind and either form -> (rc, statuses, out bytes, out_key, counts).
    lead_pad (device memory, wire): the first message starts lead_pad bytes into the caller's allocation"""
    from act_amd import capi
    wire = msgs is not None
    ob = eng.cbor_size("Refund") if wire else 128
    if mem == "host":
        if wire:
            rc, st, out, ok, c = eng.redeem_cbor_admit(ns, ring, msgs, rng, rng_mode, sign_key, charges, key_epochs, raw=True, unique=unique)
            out = b"".join(m if m else bytes(ob) for m in out)
        else:
            rc, st, out, ok, c = eng.redeem_admit(ns, ring, blob, rng, rng_mode, sign_key, charges, key_epochs, raw=True, unique=unique)
    else:
        d = Dev()
        src = d.up(bytes(lead_pad) + (b"".join(msgs) if wire else blob))
        offs = np.zeros(n + 1, np.uint64)
        if wire:
            offs[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
        dc = d.up(charges) if charges is not None else None
        dr = None if isinstance(rng, capi.ReplayRng) else d.up(rng)
        out, st, ok = d.new(ob * n, 7), d.new(n, 99), d.new(n, 77)
        d.t.cuda.synchronize()
        p = dict(set=ns, charges=dc.data_ptr() if dc is not None else None, rng=rng.ptr if dr is None else dr.data_ptr(), rng_mode=rng_mode, out=out.data_ptr(),
                 status=st.data_ptr(), out_key=ok.data_ptr(), key_epochs=key_epochs, sign_key=sign_key, raw=True, unique=unique)
        if wire:
            rc, c = eng.admit_ptr("redeem_cbor", ring, n, capi.MEM_DEVICE, cbor=src.data_ptr() + lead_pad, offsets=offs.ctypes.data, **p)
        else:
            rc, c = eng.admit_ptr("redeem", ring, n, capi.MEM_DEVICE, proofs=src.data_ptr(), **p)
        st, out, ok = d.down(st, n), d.down(out, ob * n), d.down(ok, n)
    if not raw:
        assert rc == 0, (rc, eng.lib.act_last_error(eng.ctx))
    return rc, st, out, ok, c


_worlds = {}


def world(eng, tag, owners):
    """tokens and proofs are bytes that do not depend on the transcript mode: made once per tag"""
    if tag not in _worlds:
        _worlds[tag] = World(eng, tag, owners)
    return _worlds[tag]


def engine(engine_factory, bench_params, mode):
    from act_amd import capi
    return engine_factory(bench_params, L, max_batch=MAX_BATCH, transcript=_mode(capi, mode))


def pair_of_sets(spent_keys, epochs=None, cap=1000, salt=b"\x07" * 16):
    """one export, two sets restored from it -> identical sets"""
    from act_amd import capi
    src = capi.NullifierSet(cap, salt=salt)
    if spent_keys:
        blob = b"".join(_le(k) for k in spent_keys)
        if epochs:
            assert src.check_and_insert(blob, epoch_index=bytes(i % len(epochs) for i in range(len(spent_keys))), epochs=list(epochs)) == bytes(len(spent_keys))
        else:
            assert src.check_and_insert(blob) == bytes(len(spent_keys))
    ekeys, eeps = src.export_epochs()
    src.close()
    out = []
    for _ in range(2):
        s = capi.NullifierSet(cap, salt=salt)
        if len(eeps):
            eps = sorted(set(int(e) for e in eeps))
            assert s.check_and_insert(ekeys, epoch_index=bytes(eps.index(int(e)) for e in eeps), epochs=eps) == bytes(len(eeps))
        out.append(s)
    return out


def assert_same_answers(a, b, sa, sb, ga=None, gb=None):
    """the theorem: (rc, statuses, out, out_key) of the unique call and of the existing one, the two sets, the two generators"""
    assert a[0] == b[0] and a[1] == b[1] and a[3] == b[3], "statuses / out_key differ"
    assert a[2] == b[2], "output bytes differ"
    assert _pairs(sa) == _pairs(sb) and len(sa) == len(sb)
    if ga is not None:
        assert ga.draws == gb.draws and ga.pos == gb.pos
    ca, cb = a[4], b[4]
    assert set(ca) == set(cp.COUNTS) and set(cb) == set(ad.COUNTS)
    assert all(ca[k] == cb[k] for k in ("lanes", "wire_rejected", "wrong_charge", "spent_before", "accepted")) and cb["verified"] - ca["verified"] == ca["copies"]
    cp.check_identities(ca)


# ---- 1. the fixed lane mix: hand-written expectations ----------------------------------------------------------------------------------------
def fixed_mix(eng, w, wire):
    t = {name: i for i, name in enumerate(cp.FIXED_TOKENS)}
    how = {"a": (0, None), "b": (1, None), "x": (0, "tampered"), "u": (0, "undecodable"), "i": (0, "identity")}
    mix = cp.FIXED_MIX + (cp.FIXED_WIRE_EXTRA if wire else [])
    recs = [w.proof(t[tok], *how[proof.split("/")[0]]).tobytes() for tok, proof, _, _ in mix]
    charges = b"".join(scb(ad.SPEND if right else ad.EXPECTED_WRONG) for _, _, _, right in mix)
    if not wire:
        return recs, None, charges
    msgs = eng.cbor_encode("SpendProof", b"".join(recs))
    for i, (_, proof, _, _) in enumerate(mix):
        if proof.endswith("/respelled"):
            msgs[i] = ad.respelled(recs[i], L)
        elif proof.endswith("/trailing"):
            msgs[i] = msgs[i] + b"\0"
    return recs, msgs, charges


def run_fixed_mix(eng, w, mem, wire, lead_pad=0):
    from act_amd import capi
    recs, msgs, charges = fixed_mix(eng, w, wire)
    n = len(recs)
    kw = dict(msgs=msgs) if wire else dict(blob=b"".join(recs))
    t = {name: i for i, name in enumerate(cp.FIXED_TOKENS)}
    sa, sb = pair_of_sets([w.k[t[name]] for name in cp.FIXED_SPENT])
    rng = shake("cp-fix-rng", 128 * n)
    a = call(eng, mem, sa, [w.keys[0]], n, True, charges=charges, rng=rng, rng_mode=capi.RNG_PER_LANE, lead_pad=lead_pad, **kw)
    rc, st, out, ok, c = a
    print("unique   ", list(st), c)
    assert list(st) == cp.FIXED_EXPECT[:n] and list(ok) == cp.FIXED_KEYS[:n]
    assert c == (cp.FIXED_COUNTS_WIRE if wire else cp.FIXED_COUNTS_RECORDS)
    ob = len(out) // n
    for i in range(n):
        assert any(out[ob * i:ob * i + ob]) == (st[i] == 0), i          # a copy's record is all zero, whatever its leader got
    # what the issue spells out for the records lanes: copies of accepted leaders carry the leader's matched index, copies of rejected
    # ones ACT_KEY_NONE; lane 2 (the token's other proof) is verified and a double spend; lane 12 leads because lane 11 was shed
    assert [ok[i] for i in (1, 6, 13)] == [ok[0], ok[5], ok[12]] == [0, 0, 0] and [ok[i] for i in (4, 10, 15)] == [255] * 3
    assert c["double_spend_after"] >= 1 and st[2] == 3 and ok[2] == 0 and st[11] == 250 and st[12] == 0
    b = call(eng, mem, sb, [w.keys[0]], n, False, charges=charges, rng=rng, rng_mode=capi.RNG_PER_LANE, lead_pad=lead_pad, **kw)
    assert_same_answers(a, b, sa, sb)
    assert len(sa) == len(cp.FIXED_SPENT) + c["accepted"]
    sa.close(); sb.close()


@pytest.mark.parametrize("mode,mem", MEMS)
def test_fixed_lane_mix_hand_written(engine_factory, bench_params, mode, mem):
    cp.check_model_on_fixed_mix()
    eng = engine(engine_factory, bench_params, mode)
    with step(120, "tokens and proofs"):
        w = world(eng, "cp-fix", [0] * len(cp.FIXED_TOKENS))
    for wire in (False, True):
        with step(60, "fixed mix, wire=%s" % wire):
            run_fixed_mix(eng, w, mem, wire)
    assert eng.secret_residue() == 0


# ---- 4. wire byte-alignment edges ------------------------------------------------------------------------------------------------------------
def test_wire_messages_at_every_offset_mod_16(engine_factory, bench_params):
    eng = engine(engine_factory, bench_params, "device")
    with step(120, "tokens and proofs"):
        w = world(eng, "cp-fix", [0] * len(cp.FIXED_TOKENS))
    with step(120, "sixteen offsets"):
        for pad in range(16):
            run_fixed_mix(eng, w, "device", True, lead_pad=pad)
    assert eng.secret_residue() == 0


# ---- 2. equal to the existing admission call -------------------------------------------------------------------------------------------------
N = cp.PLAN_N
N_TOKENS = 7100                       # every plan spends fewer (asserted below)
RING, EPOCHS = [1, 0], [101, 100]     # token t was issued under key t % 2: ring index 1 - t % 2


def plan_world(eng):
    w = world(eng, "cp-plan", [t % 2 for t in range(N_TOKENS)])
    if not hasattr(w, "rows"):
        tampered = w.proofs[0].copy(); tampered[:, w.pb - 32] ^= 1
        w.rows = {(0, False): w.proofs[0], (1, False): w.proofs[1], (0, True): tampered}
        ml = eng.cbor_size("SpendProof")
        enc = lambda arr: np.frombuffer(b"".join(eng.cbor_encode("SpendProof", arr.tobytes())), np.uint8).reshape(N_TOKENS, ml)
        w.wire_rows = {k: enc(v) for k, v in w.rows.items()}
    return w


def plan_case(w, num, den, with_charges, ring_idx):
    """-> (plan, model output, row selector) of one seeded plan under a ring"""
    plan, tokens = cp.copy_plan(N, num, den, cp.plan_seed(num, den), with_charges)
    assert tokens <= N_TOKENS
    key_of = lambda p: ring_idx.index(p.token % 2) if p.token % 2 in ring_idx else ad.KEY_NONE
    lanes, blobs, charges, spent = cp.plan_lanes(plan, nullifier=lambda t: w.k[t], verdict=lambda p: 7 if p.tampered or key_of(p) == ad.KEY_NONE else 0, key=key_of)
    return plan, lanes, blobs, charges, spent


@pytest.mark.parametrize("mode,mem,wire", [("host", "host", False), ("device", "device", False), ("host", "device", True), ("device", "host", True)])
def test_equal_to_the_existing_admission_call(engine_factory, bench_params, mode, mem, wire):
    from act_amd import capi
    eng = engine(engine_factory, bench_params, mode)
    with step(300, "tokens and proofs"):
        w = plan_world(eng)
    # asserted on the model's output before anything is compared (tests/test_copies_host.py chose the seeds)
    for num, den in ((1, 2), (7, 8)):
        for with_charges in (False, True):
            cats, _ = cp.plan_categories(cp.copy_plan(N, num, den, cp.plan_seed(num, den), with_charges)[0], with_charges)
            assert all(16 * v >= N for v in cats.values()), (num, den, with_charges, cats)
    cases = [(num, den, ch, capi.RNG_CALLBACK, RING, EPOCHS) for num, den in cp.FRACTIONS for ch in (False, True)]
    cases += [(1, 2, True, capi.RNG_SEQUENTIAL, RING, EPOCHS), (1, 2, True, capi.RNG_PER_LANE, RING, EPOCHS), (1, 2, False, capi.RNG_CALLBACK, [0], None)]
    rng = shake("cp-plan-rng", 128 * N)
    for num, den, with_charges, rng_mode, ring_idx, epochs in cases:
        plan, lanes, blobs, charges, spent = plan_case(w, num, den, with_charges, ring_idx)
        mst, mok, mc, mrec, mcopy = cp.model(lanes, blobs, spent, charges if with_charges else None)
        src = w.wire_rows if wire else w.rows
        rows = np.stack([src[(p.variant, p.tampered)][p.token] for p in plan])
        kw = dict(msgs=[r.tobytes() for r in rows]) if wire else dict(blob=rows.tobytes())
        kw.update(charges=b"".join(scb(c) for c in charges) if with_charges else None, rng_mode=rng_mode, key_epochs=epochs)
        ring = [w.keys[k] for k in ring_idx]
        with step(120, "copies %d/%d charges=%s rng=%d ring=%s" % (num, den, with_charges, rng_mode, ring_idx)):
            sa, sb = pair_of_sets(sorted(spent), epochs=(11, 12, 13), cap=3 * N)
            ga, gb = (capi.ReplayRng(rng), capi.ReplayRng(rng)) if rng_mode == capi.RNG_CALLBACK else (rng, rng)
            a = call(eng, mem, sa, ring, N, True, rng=ga, **kw)
            b = call(eng, mem, sb, ring, N, False, rng=gb, **kw)
            print("copies %d/%d charges=%s rng=%d ring=%s:" % (num, den, with_charges, rng_mode, ring_idx), a[4])
            if rng_mode == capi.RNG_CALLBACK:
                assert_same_answers(a, b, sa, sb, ga, gb)
                assert ga.draws == ([128 * mc["accepted"]] if mc["accepted"] else [])
            else:
                assert_same_answers(a, b, sa, sb)
            # and the model: the plan's count of copies, every status, every key index, what was recorded under which epoch
            assert a[4] == mc and a[4]["copies"] == sum(1 for x in mcopy if x is not None), (a[4], mc)
            assert list(a[1]) == mst and list(a[3]) == mok
            assert len(sa) == len(spent) + mc["accepted"]
            if epochs:
                assert {(int.from_bytes(k, "little"), e) for k, e in _pairs(sa)} >= {(k, epochs[key]) for k, key in mrec}
            if num:
                assert a[4]["copies"] > N // 4 and mc["accepted"] > 0
            sa.close(); sb.close()
    assert eng.secret_residue() == 0


# ---- 3. the flood ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem,wire", [("device", False), ("host", False), ("device", True), ("host", True)])
def test_flood_of_one_proof(engine_factory, bench_params, mem, wire):
    from act_amd import capi
    eng = engine(engine_factory, bench_params, "device")
    with step(300, "tokens and proofs"):
        w = plan_world(eng)
    a_key = [w.keys[0], w.keys[1]]
    already = [w.k[t] for t in (10, 11, 12)]
    for tampered in (False, True):
        row = (w.wire_rows if wire else w.rows)[(0, tampered)][4].tobytes()          # token 4: key 0
        kw = dict(msgs=[row] * N) if wire else dict(blob=row * N)
        with step(120, "flood, tampered=%s" % tampered):
            sa, sb = pair_of_sets(already, cap=3 * N)
            g = capi.ReplayRng(shake("cp-flood", 128 * 4))
            rc, st, out, ok, c = call(eng, mem, sa, a_key, N, True, rng=g, rng_mode=capi.RNG_CALLBACK, **kw)
            print("flood tampered=%s:" % tampered, c)
            ob = len(out) // N
            if tampered:
                assert c == dict(lanes=N, wire_rejected=0, wrong_charge=0, spent_before=0, copies=N - 1, verified=1, rejected_by_verification=1, double_spend_after=0, accepted=0)
                assert st == bytes([7]) * N and ok == b"\xff" * N and not any(out) and g.draws == [] and len(sa) == 3
            else:
                assert c == dict(lanes=N, wire_rejected=0, wrong_charge=0, spent_before=0, copies=N - 1, verified=1, rejected_by_verification=0, double_spend_after=0, accepted=1)
                assert st == b"\0" + bytes([3]) * (N - 1) and ok == b"\0" * N and any(out[:ob]) and not any(out[ob:]) and g.draws == [128] and len(sa) == 4
            assert sa.contains(_le(w.k[4])) == (b"\0" if tampered else b"\1")
            sa.close(); sb.close()
    assert eng.secret_residue() == 0


def test_leader_table_on_the_device(engine_factory, bench_params):
    """k_copy_claim / k_copy_leader over fingerprints made up here: the class shapes of the CPU test, forced collisions of the slot
    function, and every lane on one slot"""
    import random
    eng = engine(engine_factory, bench_params, "device")
    r = random.Random(53)
    with step(60, "leader tables"):
        for n in (1, 63, 64, 65, 257, 70000):
            for shape in cp.CLASS_SHAPES:
                cls = cp.class_shape(shape, n)
                fp_of = {}
                fps = [fp_of.setdefault(c, r.randrange(1, 1 << 64)) for c in cls]
                got, ms = eng.copy_leaders(fps)
                assert got == cp.want_leaders(fps), (n, shape)
                crowd = [(0xABCD1234 << 32) | (c + 1) for c in cls]      # one starting slot for every class
                got, _ = eng.copy_leaders(crowd)
                assert got == cp.want_leaders(crowd), (n, shape, "crowd")
        got, ms = eng.copy_leaders([0x1234567890ABCDEF] * (1 << 18))
        print("leader table, 2^18 lanes on one slot: %.3f ms" % ms)
        assert got == [0] * (1 << 18)
        assert eng.copy_leaders([]) == ([], 0.0)


# ---- 5. fast paths, hygiene, the failure contract ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem,wire", [("host", False), ("device", True)])
def test_fast_paths(engine_factory, bench_params, mem, wire):
    from act_amd import capi
    eng = engine(engine_factory, bench_params, "device")
    with step(300, "tokens and proofs"):
        w = plan_world(eng)
    n = 40
    ring = [w.keys[0], w.keys[1]]
    src = w.wire_rows if wire else w.rows
    rows = [src[(t % 2, False)][t].tobytes() for t in range(n)]
    rows[7] = src[(0, True)][7].tobytes()
    kw = dict(msgs=rows) if wire else dict(blob=b"".join(rows))
    rng = shake("cp-fast", 128 * n)
    with step(60, "all distinct, nothing shed: the redeem call's answers"):
        sa, sb = pair_of_sets([], cap=1000)
        rc, st, out, ok, c = call(eng, mem, sa, ring, n, True, rng=rng, rng_mode=capi.RNG_PER_LANE, **kw)
        if wire:
            pst, pout, pok = eng.redeem_cbor_keyring(sb, ring, rows, rng, capi.RNG_PER_LANE, -1, None)
            pout = b"".join(m if m else bytes(len(out) // n) for m in pout)
        else:
            pst, pout, pok = eng.redeem_keyring(sb, ring, b"".join(rows), rng, capi.RNG_PER_LANE, -1, key_epochs=None)
        assert (st, out, ok) == (pst, pout, pok) and list(st) == [7 if i == 7 else 0 for i in range(n)] and _pairs(sa) == _pairs(sb)
        assert c == dict(lanes=n, wire_rejected=0, wrong_charge=0, spent_before=0, copies=0, verified=n, rejected_by_verification=1, double_spend_after=0, accepted=n - 1)
        sa.close(); sb.close()
    with step(60, "everything shed (replays and wrong charges, repeated): no verification"):
        sa, sb = pair_of_sets([w.k[t] for t in range(0, n, 2)], cap=1000)
        rows2 = [rows[i // 2 * 2 if i % 4 < 2 else i] for i in range(n)]          # lanes 0,1 = row 0; 2,3 = rows 2,3; 4,5 = row 4 ...
        tok2 = [i // 2 * 2 if i % 4 < 2 else i for i in range(n)]
        charges = b"".join(scb(ad.SPEND + (1 if t % 2 else 0)) for t in tok2)      # odd tokens: wrong charge; even tokens: recorded
        kw2 = dict(msgs=rows2) if wire else dict(blob=b"".join(rows2))
        g = capi.ReplayRng(shake("cp-shed", 128 * n))
        eng.prof_enable(True); eng.prof_reset()
        rc, st, out, ok, c = call(eng, mem, sa, ring, n, True, charges=charges, rng=g, rng_mode=capi.RNG_CALLBACK, **kw2)
        prof = eng.prof()
        eng.prof_enable(False)
        assert list(st) == [250 if t % 2 else 3 for t in tok2] and ok == b"\xff" * n and not any(out)
        assert c == dict(lanes=n, wire_rejected=0, wrong_charge=sum(t % 2 for t in tok2), spent_before=sum(1 - t % 2 for t in tok2), copies=0, verified=0,
                         rejected_by_verification=0, double_spend_after=0, accepted=0)
        assert not any(k.startswith("k_spend") for k in prof), prof
        assert g.draws == [] and len(sa) == n // 2
        sa.close(); sb.close()
    assert eng.secret_residue() == 0


@pytest.mark.parametrize("mem", ["host", "device"])
def test_failed_signatures_on_a_batch_with_copies(engine_factory, bench_params, mem):
    from act_amd import capi
    eng = engine(engine_factory, bench_params, "host")
    with step(300, "tokens and proofs"):
        w = plan_world(eng)
    ring = [w.keys[0], w.keys[1]]
    toks = [0, 1, 0, 2, 1, 1, 3, 2, 0]                                             # lanes 2, 4, 5, 7, 8 repeat an earlier lane
    rows = [w.rows[(0, t == 3)][t].tobytes() for t in toks]                        # token 3 is tampered
    n = len(toks)
    rng = shake("cp-sign", 128 * n)
    with step(60, "the signature step fails behind the recorded nullifiers"):
        sa, sb = pair_of_sets([], cap=1000)
        assert eng.lib.act_debug_fail_next_signs(eng.ctx, 1) == 0
        rc, st, out, ok, c = call(eng, mem, sa, ring, n, True, blob=b"".join(rows), rng=rng, rng_mode=capi.RNG_PER_LANE, raw=True)
        assert rc != 0 and not any(out)
        # leaders: recorded, not signed; their copies: the nullifier IS recorded -- a double spend; the tampered lane as ever
        assert list(st) == [251, 251, 3, 251, 3, 3, 7, 3, 3] and list(ok) == [0, 1, 0, 0, 1, 1, 255, 0, 0]
        assert c["copies"] == 5 and c["verified"] == 4 and len(sa) == 3
        # the same batch, signatures working, on the twin set
        rc, st, out, ok, c = call(eng, mem, sb, ring, n, True, blob=b"".join(rows), rng=rng, rng_mode=capi.RNG_PER_LANE)
        assert list(st) == [0, 0, 3, 0, 3, 3, 7, 3, 3] and c["accepted"] == 3 and _pairs(sa) == _pairs(sb)
        sa.close(); sb.close()
    with step(60, "refused calls write no counts"):
        s1, s2 = pair_of_sets([], cap=1000)
        rc, st, out, ok, c = call(eng, mem, s1, ring, n, True, blob=b"".join(rows), rng=rng, rng_mode=capi.RNG_PER_LANE, raw=True, sign_key=4)
        assert rc == 1 and len(s1) == 0 and c == dict.fromkeys(cp.COUNTS, 0)
        rc, st, out, ok, c = call(eng, "host", s1, ring, 0, True, blob=b"", rng=rng, rng_mode=capi.RNG_PER_LANE)
        assert rc == 0 and c["lanes"] == 0
        s1.close(); s2.close()
    assert eng.secret_residue() == 0


def test_python_api_unique():
    """api.PrivateKey / api.Keyring: unique=True gives what unique=False gives on the same batch"""
    from act_amd import api
    params = api.Params.new("test-org", "test-service", "test", "2024-01-01")
    with step(240, "api round trip"):
        rng = api.ByteStreamRng(shake("cp-api", 1 << 20))
        sk = api.PrivateKey.random(rng, params)
        proofs = []
        for spend in (5, 7):
            pre = api.PreIssuance.random(rng, params)
            req = pre.request(params, rng)
            tok = pre.to_credit_token(params, sk.public(), req, sk.issue(params, req, 20, rng))
            proofs.append(tok.prove_spend(params, spend, rng)[0])
        batch = [proofs[0], proofs[0], proofs[1], proofs[0], proofs[1]]
        charges = [5, 5, 8, 5, 7]
        got = []
        for unique in (False, True):
            db = api.NullifierDb(1000)
            r = api.ByteStreamRng(shake("cp-api-sign", 1 << 16))
            res = sk.redeem_admit_batch(params, db, batch, r, charges=charges, unique=unique)
            ring = api.Keyring([sk], epochs=[9])
            db2 = api.NullifierDb(1000)
            res2, matched = ring.redeem_admit_cbor_batch(params, db2, [p.to_cbor(params) for p in batch], r, charges=charges, unique=unique)
            assert ("copies" in ring.last_admit_counts) == unique
            if unique:
                assert ring.last_admit_counts["copies"] == 2 and ring.last_admit_counts["verified"] == 2
            got.append(([x.record if isinstance(x, api.Refund) else ("error", x.code, x.name) for x in res],
                        [x if isinstance(x, bytes) else ("error", x.code) for x in res2], matched, len(db), len(db2), db2.epoch_len(9)))
        assert got[0] == got[1]
        assert [x[1] if isinstance(x, tuple) else 0 for x in got[1][0]] == [0, 3, 250, 3, 0] and got[1][2] == [0, 0, None, 0, 0]
