"""Nullifier epochs on the GPU: every recorded nullifier carries the epoch of the issuer key it was spent under, the ring redemption
calls record the matched key's epoch, and act_nullifier_set_retire_epoch removes one epoch's nullifiers and refuses it from then on.
The model is a Python dict reduced scalar -> epoch (the reference tests' NullifierDb, src/tests.rs:29-50, with the epoch of the first
recorder beside every key); the existing calls are the reference wherever the contract is "nothing existing moved"."""
import random

import numpy as np
import pytest

import keyring_cases as kr
from conftest import ELL, shake

pytestmark = pytest.mark.gpu

UNDETERMINED = 2          # ACT_NULLIFIER_UNDETERMINED
ERR_ARG = 1               # ACT_ERR_ARG


def _le(v: int) -> bytes:
    return v.to_bytes(32, "little")


def _batch(r, pool, n):
    """n keys drawn from `pool` (repeats likely), about one in eight spelled k + l where that still fits 256 bits"""
    out = []
    for _ in range(n):
        v = pool[r.randrange(len(pool))]
        out.append(v + ELL if r.random() < 0.125 and v + ELL < 2**256 else v)
    return out


def _model_step(model, vals, mask, eidx, table):
    """the sequential loop: a masked lane answers 0 and records nothing; the epoch of the first recorder sticks"""
    ans = []
    for v, m, e in zip(vals, mask, eidx):
        if m:
            ans.append(0); continue
        k = v % ELL
        ans.append(1 if k in model else 0)
        model.setdefault(k, table[e])
    return bytes(ans)


def _keyset(blob: bytes) -> set:
    return {blob[i:i + 32] for i in range(0, len(blob), 32)}


def _pairs(keys: bytes, epochs) -> dict:
    ks = [int.from_bytes(keys[i:i + 32], "little") for i in range(0, len(keys), 32)]
    assert len(ks) == len(epochs) and len(set(ks)) == len(ks), "a key exported twice"
    assert all(k < ELL for k in ks), "an exported key is not reduced"
    return dict(zip(ks, (int(e) for e in epochs)))


def _export_epochs_dev(s, max_keys):
    import torch
    from act_amd import capi
    dk = torch.zeros(32 * max_keys, dtype=torch.uint8, device="cuda"); de = torch.zeros(max_keys, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    cur, keys, eps = 0, [], []
    while cur != capi.EXPORT_DONE:
        cur, got = s.export_epochs_dev(cur, max_keys, dk.data_ptr(), de.data_ptr())
        keys.append(dk[:32 * got].cpu().numpy().tobytes()); eps.append(de[:got].cpu().numpy().astype(np.uint32))
    return b"".join(keys), np.concatenate(eps)


def _check_against_model(s, model, table, unused=777):
    assert len(s) == len(model)
    for e in table:
        assert s.epoch_len(e) == sum(1 for v in model.values() if v == e), e
    assert s.epoch_len(unused) == 0
    for mk in (1 << 20, 777):
        assert _pairs(*s.export_epochs(mk)) == model, mk
        assert _pairs(*_export_epochs_dev(s, mk)) == model, mk
    plain = s.export()
    assert {int.from_bytes(plain[i:i + 32], "little") for i in range(0, len(plain), 32)} == set(model) and len(plain) == 32 * len(model)


def _insert_dev(s, blob, mask, eidx, table, raw=False):
    import torch
    n = len(blob) // 32
    up = lambda b: torch.from_numpy(np.frombuffer(bytes(b) + b"\0", np.uint8).copy()).cuda()
    dk, dm, de = up(blob), up(mask), up(eidx)
    out = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = s.check_and_insert_epoch_dev(n, dk.data_ptr(), 32, dm.data_ptr(), de.data_ptr(), table, out.data_ptr(), raw=True)
    return rc, out.cpu().numpy().tobytes()


def test_epoch_insert_count_and_export_equal_the_model():
    from act_amd import capi
    r = random.Random(11)
    pool = [r.randrange(ELL) for _ in range(9000)]
    table = [5, 0, (1 << 24) - 1]
    s = capi.NullifierSet(20000, salt=bytes(range(16)))
    model = {}
    for b, n in enumerate((1, 5000, 37, 2500, 640, 4096, 3)):
        vals = _batch(r, pool, n)
        mask = bytes(1 if r.random() < 0.2 else 0 for _ in range(n))
        eidx = bytes(r.randrange(3) for _ in range(n))
        blob = b"".join(_le(v) for v in vals)
        want = _model_step(model, vals, mask, eidx, table)
        if b % 2:
            rc, got = _insert_dev(s, blob, mask, eidx, table)
            assert rc == 0
        else:
            got = s.check_and_insert(blob, skip_mask=mask, epoch_index=eidx, epochs=table)
        assert got == want, b
        _check_against_model(s, model, table)
        probe = vals + [r.randrange(ELL) for _ in range(50)]
        assert s.contains(b"".join(_le(v) for v in probe)) == bytes(1 if v % ELL in model else 0 for v in probe)
    probe = pool[:3000] + [r.randrange(ELL) for _ in range(100)]
    assert s.contains(b"".join(_le(v) for v in probe)) == bytes(1 if v in model else 0 for v in probe)
    assert len({e for e in model.values()}) == 3
    # a lane whose index names no table entry: undetermined, not recorded, and it does not shadow a later lane with the same key
    fresh = [r.randrange(ELL) for _ in range(6)]
    vals = [fresh[0], fresh[0], fresh[1], pool[0], fresh[2], fresh[2]]
    eidx = bytes([3, 1, 255, 7, 0, 2]); mask = bytes(6)
    want = bytes([2, 0, 2, 2, 0, 1])
    for dev in (False, True):
        twin = capi.NullifierSet(20000, salt=bytes(range(16)))
        twin.check_and_insert(b"".join(_le(k) for k in model if model[k] == 5), epochs=[5])
        n0 = len(twin)
        blob = b"".join(_le(v) for v in vals)
        rc, got = _insert_dev(twin, blob, mask, eidx, table) if dev else twin.check_and_insert(blob, skip_mask=mask, epoch_index=eidx, epochs=table, raw=True)
        assert (rc, got) == (ERR_ARG, want), dev
        assert len(twin) == n0 + 2 and twin.contains(blob) == bytes([1, 1, 0, int(model.get(pool[0] % ELL) == 5), 1, 1])
        got = _pairs(*twin.export_epochs())
        assert got[fresh[0]] == 0 and got[fresh[2]] == 5
        # the next call is an ordinary one again
        assert twin.check_and_insert(_le(fresh[1]), epochs=[9]) == b"\0" and twin.epoch_len(9) == 1
        twin.close()
    s.close()


def test_reserve_keeps_epochs_and_the_existing_call_is_the_zero_table():
    from act_amd import capi
    r = random.Random(12)
    pool = [r.randrange(ELL) for _ in range(4000)]
    table = [0, 3, 70000]
    s = capi.NullifierSet(4000, salt=b"\x21" * 16)
    model = {}
    for n in (1500, 1500):
        vals = _batch(r, pool, n); eidx = bytes(r.randrange(3) for _ in range(n))
        assert s.check_and_insert(b"".join(_le(v) for v in vals), epoch_index=eidx, epochs=table) == _model_step(model, vals, bytes(n), eidx, table)
    s.reserve(8 * 4000)
    _check_against_model(s, model, table)
    # the existing call on the same set: epoch 0, and never a change of a recorded epoch
    vals = _batch(r, pool, 800) + [r.randrange(ELL) for _ in range(200)]
    assert s.check_and_insert(b"".join(_le(v) for v in vals)) == _model_step(model, vals, bytes(1000), bytes(1000), [0])
    _check_against_model(s, model, table)
    s.close()
    # table {0} / no indices against the existing call, twin sets with one salt: the same answers, the same table
    a, b, c = (capi.NullifierSet(3000, salt=b"\x22" * 16) for _ in range(3))
    for n in (1, 900, 1200):
        vals = _batch(r, pool, n); blob = b"".join(_le(v) for v in vals); mask = bytes(1 if r.random() < 0.1 else 0 for _ in range(n))
        want = a.check_and_insert(blob, skip_mask=mask)
        assert b.check_and_insert(blob, skip_mask=mask, epochs=[0]) == want
        assert _insert_dev(c, blob, mask, bytes(n), [0]) == (0, want)
    # (which of two keys that meet in one probe chain inside a batch takes the earlier slot is not fixed, so contents are compared)
    want = _pairs(*a.export_epochs())
    assert len(want) == len(a) and not any(want.values())
    for t in (b, c):
        assert _pairs(*t.export_epochs()) == want and len(t) == len(a)
    assert _keyset(a.export()) == _keyset(b.export()) == _keyset(c.export()) == {_le(k) for k in want}
    for t in (a, b, c):
        t.close()


def test_retire_epoch():
    from act_amd import capi
    r = random.Random(13)
    pool = [r.randrange(ELL) for _ in range(5000)]
    table = [0, 8, 9]
    s = capi.NullifierSet(6000, salt=b"\x31" * 16)
    model = {}
    for n in (2000, 2000):
        vals = _batch(r, pool, n); eidx = bytes(r.randrange(3) for _ in range(n))
        assert s.check_and_insert(b"".join(_le(v) for v in vals), epoch_index=eidx, epochs=table) == _model_step(model, vals, bytes(n), eidx, table)
    cur, _, _ = s.export_epochs_step(0, 100)
    cur_plain, _ = s.export_step(0, 100)
    for bad in (0, 1 << 24):
        with pytest.raises(capi.ActError):
            s.retire_epoch(bad)
    assert len(s) == len(model) and s.retired_epochs() == []
    gone = [k for k, e in model.items() if e == 8]
    kept = [k for k, e in model.items() if e != 8]
    assert gone and s.retire_epoch(8) == len(gone)
    model = {k: e for k, e in model.items() if e != 8}
    assert len(s) == len(model) and s.epoch_len(8) == 0 and s.retired_epochs() == [8]
    assert s.contains(b"".join(_le(k) for k in gone)) == bytes(len(gone))
    assert s.contains(b"".join(_le(k) for k in kept)) == b"\1" * len(kept)
    assert s.retire_epoch(8) == 0 and s.retired_epochs() == [8] and len(s) == len(model)
    # cursors taken before the retirement are refused by either export call; a fresh one walks the new table
    for step, c in ((s.export_epochs_step, cur), (s.export_step, cur), (s.export_epochs_step, cur_plain), (s.export_step, cur_plain)):
        with pytest.raises(capi.ActError, match="restart from 0"):
            step(c, 100)
    _check_against_model(s, model, [0, 9])
    # an insert whose table names the retired epoch is refused whole, host and device memory
    vals = [r.randrange(ELL) for _ in range(50)]; blob = b"".join(_le(v) for v in vals)
    mask = bytes(1 if i % 7 == 0 else 0 for i in range(50)); eidx = bytes(i % 2 for i in range(50))      # no lane even uses the retired entry
    want = bytes(0 if m else UNDETERMINED for m in mask)
    assert s.check_and_insert(blob, skip_mask=mask, epoch_index=eidx, epochs=[0, 9, 8], raw=True) == (ERR_ARG, want)
    assert _insert_dev(s, blob, mask, eidx, [0, 9, 8]) == (ERR_ARG, want)
    assert s.check_and_insert(blob, skip_mask=mask, epochs=[1 << 24], raw=True) == (ERR_ARG, want)
    assert "EPOCH_MAX" in s.lib.act_nullifier_set_last_error(s.h).decode()
    assert len(s) == len(model) and s.contains(blob) == bytes(50)
    # a removed key under a live epoch is fresh -- once -- and len keeps counting from what is left
    again = gone[:40]
    assert s.check_and_insert(b"".join(_le(k) for k in again), epochs=[9]) == bytes(40)
    assert s.check_and_insert(b"".join(_le(k) for k in again)) == b"\1" * 40
    model.update({k: 9 for k in again})
    # an epoch without keys: nothing removed, the refusal armed, the table (and a cursor into it) untouched
    cur, _, _ = s.export_epochs_step(0, 64)
    assert s.retire_epoch(4242) == 0 and s.retired_epochs() == [8, 4242]
    s.export_epochs_step(cur, 64)
    with pytest.raises(capi.ActError):
        s.check_and_insert(_le(1), epochs=[4242])
    _check_against_model(s, model, [0, 9])
    # retirement and growth together
    s.reserve(30000)
    assert s.retire_epoch(9) == sum(1 for e in model.values() if e == 9)
    model = {k: e for k, e in model.items() if e == 0}
    _check_against_model(s, model, [0])
    assert s.retired_epochs() == [8, 9, 4242]
    s.close()


def _two_key_lanes(octx, tag):
    """tokens issued under a and b; lane 4 under a stranger's key, lane 5 tampered, lane 0 and lane 1 submitted twice"""
    keys = kr.make_keys(octx, tag)
    a, b = keys[0], keys[1]
    lanes = [kr.spend_under(octx, (a, b, a, b, keys[4], a, b, a)[i], "%s-%d" % (tag, i))[0] for i in range(8)]
    t = bytearray(lanes[5]); t[33] ^= 1; lanes[5] = bytes(t)
    lanes += [lanes[0], lanes[1]]
    return a, b, lanes


def _want_epochs(lanes, st, ok, key_epochs):
    """accepted lanes: the epoch of the key they MATCHED; every other lane recorded nothing"""
    want = {}
    for p, s, k in zip(lanes, st, ok):
        if s == 0:
            want[int.from_bytes(p[:32], "little") % ELL] = key_epochs[k]
    return want


@pytest.mark.parametrize("mode", ["host", "device"])
def test_ring_redemption_records_the_matched_keys_epoch(engine_factory, oracle, bench_params, mode):
    import torch
    from act_amd import capi
    L = 8
    eng = engine_factory(bench_params, L, max_batch=16, transcript=capi.TRANSCRIPT_HOST if mode == "host" else capi.TRANSCRIPT_DEVICE)
    octx = oracle.ctx(bench_params, L)
    a, b, lanes = _two_key_lanes(octx, "gne-rd")
    ring, key_epochs = [b, a], (7, 9)
    blob = b"".join(lanes); n = len(lanes)
    rng = shake("gne-rd-rng", 128 * n)
    up = lambda x: torch.from_numpy(np.frombuffer(x + b"\0", np.uint8).copy()).cuda()
    for sign_key in (capi.SIGN_MATCHED, 0):
        ref, ns = capi.NullifierSet(1000, salt=b"r" * 16), capi.NullifierSet(1000, salt=b"r" * 16)
        want = eng.redeem_keyring(ref, ring, blob, rng, capi.RNG_SEQUENTIAL, sign_key)
        assert list(want[0]) == [0, 0, 0, 0, 7, 7, 0, 0, 3, 3] and list(want[2]) == [1, 0, 1, 0, 255, 255, 0, 1, 1, 0]
        assert eng.redeem_keyring(ns, ring, blob, rng, capi.RNG_SEQUENTIAL, sign_key, key_epochs=key_epochs) == want
        epochs_want = _want_epochs(lanes, want[0], want[2], key_epochs)
        assert len(epochs_want) == 6 and _pairs(*ns.export_epochs()) == epochs_want
        assert _keyset(ns.export()) == _keyset(ref.export()) and not ref.export_epochs()[1].any()
        assert ns.epoch_len(7) == 3 and ns.epoch_len(9) == 3 and ns.epoch_len(0) == 0
        # everything again: double spends, nothing recorded, no epoch changed (the ring the other way round would name other epochs)
        st, rf, ok = eng.redeem_keyring(ns, ring, blob, rng, capi.RNG_SEQUENTIAL, sign_key, key_epochs=(9, 7))
        assert st == bytes(3 if v == 0 else v for v in want[0]) and not any(rf) and ok == want[2]
        assert _pairs(*ns.export_epochs()) == epochs_want
        ns.close()
        # device memory
        ns = capi.NullifierSet(1000, salt=b"r" * 16)
        dp, dr = up(blob), up(rng)
        out, st, ok = (torch.full((m,), f, dtype=torch.uint8, device="cuda") for m, f in ((128 * n, 7), (n, 99), (n, 77)))
        torch.cuda.synchronize()
        eng.keyring_ptr("redeem", ring, n, capi.MEM_DEVICE, set=ns, sign_key=sign_key, key_epochs=key_epochs, proofs=dp.data_ptr(), rng=dr.data_ptr(),
                        rng_mode=capi.RNG_SEQUENTIAL, out=out.data_ptr(), status=st.data_ptr(), out_key=ok.data_ptr())
        assert tuple(t.cpu().numpy().tobytes() for t in (st, out, ok)) == want
        assert _pairs(*ns.export_epochs()) == epochs_want
        ns.close(); ref.close()
    # the CBOR form: host and device memory against the existing call
    msgs = eng.cbor_encode("SpendProof", blob)
    ref, ns = capi.NullifierSet(1000), capi.NullifierSet(1000)
    want = eng.redeem_cbor_keyring(ref, ring, msgs, rng, capi.RNG_SEQUENTIAL)
    assert eng.redeem_cbor_keyring(ns, ring, msgs, rng, capi.RNG_SEQUENTIAL, key_epochs=key_epochs) == want
    assert _pairs(*ns.export_epochs()) == _want_epochs(lanes, want[0], want[2], key_epochs)
    ns.close()
    ns = capi.NullifierSet(1000)
    ml, rl = eng.cbor_size("SpendProof"), eng.cbor_size("Refund")
    assert all(len(m) == ml for m in msgs)                          # offsets NULL: message i at cbor + i * act_cbor_size
    dm, dr = up(b"".join(msgs)), up(rng)
    out, st, ok = (torch.full((m,), f, dtype=torch.uint8, device="cuda") for m, f in ((rl * n, 7), (n, 99), (n, 77)))
    torch.cuda.synchronize()
    eng.keyring_ptr("redeem_cbor", ring, n, capi.MEM_DEVICE, set=ns, key_epochs=key_epochs, cbor=dm.data_ptr(), rng=dr.data_ptr(), rng_mode=capi.RNG_SEQUENTIAL,
                    out=out.data_ptr(), status=st.data_ptr(), out_key=ok.data_ptr())
    ob = out.cpu().numpy().tobytes()
    assert (st.cpu().numpy().tobytes(), [ob[rl * i:rl * i + rl] if want[0][i] == 0 else b"" for i in range(n)], ok.cpu().numpy().tobytes()) == want
    assert _pairs(*ns.export_epochs()) == _want_epochs(lanes, want[0], want[2], key_epochs)
    # a retired epoch (or one above the maximum) in key_epochs fails the call before any status is written
    ns.retire_epoch(7)
    for bad in ((7, 9), (9, 1 << 24)):
        n0 = len(ns)
        rc, st, rf, ok = eng.redeem_keyring(ns, ring, blob, rng, capi.RNG_SEQUENTIAL, raw=True, key_epochs=bad)
        assert rc == ERR_ARG and st == bytes(n) and rf == b"\7" * (128 * n) and len(ns) == n0
        with pytest.raises(capi.ActError):
            eng.redeem_cbor_keyring(ns, ring, msgs, rng, capi.RNG_SEQUENTIAL, key_epochs=bad)
    # the epoch of key a retired, key a out of the ring: the ring call with the live epoch goes on
    st, rf, ok = eng.redeem_keyring(ns, [a], blob, rng, capi.RNG_SEQUENTIAL, key_epochs=(9,))
    assert list(st) == [3, 7, 3, 7, 7, 7, 7, 3, 3, 7]
    ns.close(); ref.close()
    assert eng.secret_residue() == 0


def test_ring_redemption_with_epochs_over_a_node(engine_factory, oracle, bench_params):
    from act_amd import capi
    L = 8
    eng = engine_factory(bench_params, L, max_batch=16, transcript=capi.TRANSCRIPT_DEVICE)
    octx = oracle.ctx(bench_params, L)
    a, b, lanes = _two_key_lanes(octx, "gne-rd")
    ring, key_epochs = [b, a], (7, 9)
    blob = b"".join(lanes); n = len(lanes)
    rng = shake("gne-node-rng", 128 * n)
    node = capi.Node(bench_params, L, devices=(0, 0), max_batch=7, transcript=capi.TRANSCRIPT_DEVICE)
    ref, nn = capi.NodeNullifierSet(4000, devices=(0, 0)), capi.NodeNullifierSet(4000, devices=(0, 0))
    try:
        for sign_key in (capi.SIGN_MATCHED, 1):
            want = node.redeem_keyring(ref, ring, blob, rng, capi.RNG_SEQUENTIAL, sign_key)
            assert node.redeem_keyring(nn, ring, blob, rng, capi.RNG_SEQUENTIAL, sign_key, key_epochs=key_epochs) == want
            if sign_key == capi.SIGN_MATCHED:
                first = want
                assert list(want[0]) == [0, 0, 0, 0, 7, 7, 0, 0, 3, 3]
        epochs_want = _want_epochs(lanes, first[0], first[2], key_epochs)
        for mk in (1 << 20, 2):                                         # the node cursor covers both parts
            assert _pairs(*nn.export_epochs(mk)) == epochs_want, mk
        assert nn.epoch_len(7) == nn.epoch_len(9) == 3 and len(nn) == 6 and not ref.export_epochs()[1].any()
        msgs = eng.cbor_encode("SpendProof", blob)
        ref2, nn2 = capi.NodeNullifierSet(4000, devices=(0, 0)), capi.NodeNullifierSet(4000, devices=(0, 0))
        want = node.redeem_cbor_keyring(ref2, ring, msgs, capi.ReplayRng(rng), capi.RNG_CALLBACK)
        assert node.redeem_cbor_keyring(nn2, ring, msgs, capi.ReplayRng(rng), capi.RNG_CALLBACK, key_epochs=key_epochs) == want
        assert _pairs(*nn2.export_epochs()) == epochs_want
        ref2.close(); nn2.close()
        # node retirement, the refusal, and the node form of the insert
        assert nn.retire_epoch(9) == 3 and nn.retired_epochs() == [9] and len(nn) == 3 and nn.retire_epoch(9) == 0
        rc, st, rf, ok = node.redeem_keyring(nn, ring, blob, rng, capi.RNG_SEQUENTIAL, raw=True, key_epochs=key_epochs)
        assert rc == ERR_ARG and st == bytes(n) and rf == b"\7" * (128 * n) and len(nn) == 3
        r = random.Random(14)
        vals = [r.randrange(ELL) for _ in range(300)]; eidx = bytes(i % 3 for i in range(300))
        assert nn.check_and_insert(b"".join(_le(v) for v in vals), epoch_index=eidx, epochs=[0, 7, 11]) == bytes(300)
        assert (nn.epoch_len(0), nn.epoch_len(7), nn.epoch_len(11)) == (100, 103, 100)
        got = _pairs(*nn.export_epochs(50))
        assert all(got[v] == [0, 7, 11][i % 3] for i, v in enumerate(vals))
    finally:
        ref.close(); nn.close(); node.close()


def test_rotation_through_the_api(tmp_path):
    """ring [new, old] with epochs; spends of both; the old key leaves the ring and its epoch is retired"""
    from act_amd import api, nullifier_snapshot
    params = api.Params.new("test-org", "test-service", "test", "2024-01-01")
    rng = api.ByteStreamRng(shake("gne-api", 1 << 20))
    old, new = api.PrivateKey.random(rng, params), api.PrivateKey.random(rng, params)
    toks = []
    for sk in (old, new, old, new, old):
        pre = api.PreIssuance.random(rng, params); req = pre.request(params, rng)
        toks.append(pre.to_credit_token(params, sk.public(), req, sk.issue(params, req, 20, rng)))
    proofs = [t.prove_spend(params, 5, rng)[0] for t in toks]
    db = api.NullifierDb(1000)
    plain = str(tmp_path / "plain.snap")
    ring = api.Keyring([new, old], epochs=[2, 1])
    refunds, idx = ring.redeem_batch(params, db, proofs[:4], rng)
    assert idx == [1, 0, 1, 0] and all(isinstance(x, api.Refund) for x in refunds)
    out, idx = ring.redeem_cbor_batch(params, db, [proofs[4].to_cbor(params)], rng)
    assert idx == [1] and isinstance(out[0], bytes)
    assert (len(db), db.epoch_len(1), db.epoch_len(2), db.retired()) == (5, 3, 2, [])
    # the old key leaves the ring for good; its epoch is retired
    ring = api.Keyring([new], epochs=[2])
    assert db.retire(1) == 3 and len(db) == 2 and db.retired() == [1]
    res, idx = ring.redeem_batch(params, db, proofs, rng)
    assert [x.name for x in res] == ["InvalidClientSpendProof", "DoubleSpendError"] * 2 + ["InvalidClientSpendProof"] and len(db) == 2
    assert db.spend(proofs[1].nullifier(), epoch=2) is False and db.spend_batch([bytes([9]) * 31 + b"\0"], epoch=2) == [True]
    with pytest.raises(Exception):
        db.spend(bytes([8]) * 31 + b"\0", epoch=1)
    # save -> restore keeps epochs, counts and the retired list
    p = str(tmp_path / "db.snap")
    assert db.save(p) == 3 and open(p, "rb").read(8) == nullifier_snapshot.MAGIC_V2
    db2 = api.NullifierDb.restore(p, capacity=1000)
    assert (len(db2), db2.epoch_len(2), db2.epoch_len(1), db2.retired()) == (3, 3, 0, [1])
    assert db2.set.export_epochs()[0] != b"" and _pairs(*db2.set.export_epochs()) == _pairs(*db.set.export_epochs())
    with pytest.raises(Exception):
        db2.spend(bytes([8]) * 31 + b"\0", epoch=1)
    res, _ = ring.redeem_batch(params, db2, proofs[:2], rng)
    assert [x.name for x in res] == ["InvalidClientSpendProof", "DoubleSpendError"]
    # a set that never saw an epoch still saves v1 bytes
    db3 = api.NullifierDb(1000)
    nul = [p_.nullifier() for p_ in proofs]
    assert db3.spend_batch(nul) == [True] * 5
    assert db3.save(plain) == 5 and open(plain, "rb").read() == nullifier_snapshot.encode(b"".join(nul))
    assert len(api.NullifierDb.restore(plain, capacity=1000)) == 5


def test_a_million_keys_over_four_epochs():
    import torch
    from act_amd import capi
    n = 1 << 20
    g = np.random.default_rng(15)
    raw = g.integers(0, 256, size=(n, 32), dtype=np.uint8)
    raw[:, 31] &= 0x0F                                              # below 2^252 < l: every key already reduced, all distinct w.h.p.
    assert len(np.unique(raw.view("S32").reshape(-1))) == n
    eidx = g.integers(0, 4, size=n, dtype=np.uint8)
    table = [0, 100, 200, 300]
    s = capi.NullifierSet(n, salt=b"m" * 16)
    d_keys, d_eidx = torch.from_numpy(raw.reshape(-1)).cuda(), torch.from_numpy(eidx).cuda()
    d_out = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s.check_and_insert_epoch_dev(n, d_keys.data_ptr(), 32, 0, d_eidx.data_ptr(), table, d_out.data_ptr())
    assert int(d_out.sum().item()) == 0 and len(s) == n
    counts = [int((d_eidx == k).sum().item()) for k in range(4)]
    assert [s.epoch_len(e) for e in table] == counts
    assert s.retire_epoch(200) == counts[2] and len(s) == n - counts[2]
    assert [s.epoch_len(e) for e in table] == [counts[0], counts[1], 0, counts[3]]
    s.contains_dev(n, d_keys.data_ptr(), 32, d_out.data_ptr())
    assert torch.equal(d_out, (d_eidx != 2).to(torch.uint8))
    # what is left carries its epoch; the next insert counts on from what is left
    dk = torch.zeros(32 * n, dtype=torch.uint8, device="cuda"); de = torch.zeros(n, dtype=torch.int32, device="cuda")
    cur, got = s.export_epochs_dev(0, 1 << 22, dk.data_ptr(), de.data_ptr())
    assert cur == capi.EXPORT_DONE and got == n - counts[2]
    assert torch.bincount(de[:got], minlength=301)[[0, 100, 200, 300]].tolist() == [counts[0], counts[1], 0, counts[3]]
    m = 1 << 17
    back = int((d_eidx[:m] == 2).sum().item())
    s.check_and_insert_epoch_dev(m, d_keys.data_ptr(), 32, 0, 0, [300], d_out.data_ptr())
    assert torch.equal(d_out[:m], (d_eidx[:m] != 2).to(torch.uint8))
    assert len(s) == n - counts[2] + back and s.epoch_len(300) == counts[3] + back
    s.close()
