"""Growth, export, read-only look-up and snapshots of the GPU nullifier set (act_nullifier_set_reserve / _export / contains_batch and
their node forms; anonymous-credit-tokens_amd/nullifier_snapshot.py), against a Python set of reduced scalars -- the reference tests'
NullifierDb (src/tests.rs:29-50) -- and through the product path: a restarted issuer must still refuse every token redeemed before."""
import random

import numpy as np
import pytest

from conftest import ELL, shake, scb

pytestmark = pytest.mark.gpu


def _le(v: int) -> bytes:
    return v.to_bytes(32, "little")


def _keys_of(blob: bytes):
    return [blob[i:i + 32] for i in range(0, len(blob), 32)]


def _batch(r, pool, n):
    """n keys drawn from `pool` (repeats likely), about one in eight spelled k + l where that still fits 256 bits"""
    out = []
    for _ in range(n):
        v = pool[r.randrange(len(pool))]
        out.append(v + ELL if r.random() < 0.125 and v + ELL < 2**256 else v)
    return out


def _model_step(model, vals):
    ans = []
    for v in vals:
        k = v % ELL
        ans.append(1 if k in model else 0)
        model.add(k)
    return bytes(ans)


def _fill(s, model, r, pool, batches, n):
    for _ in range(batches):
        vals = _batch(r, pool, n)
        assert s.check_and_insert(b"".join(_le(v) for v in vals)) == _model_step(model, vals)


def _as_set(blob: bytes):
    keys = _keys_of(blob)
    vals = [int.from_bytes(k, "little") for k in keys]
    assert len(set(keys)) == len(keys), "a key exported twice"
    assert all(v < ELL for v in vals), "an exported key is not reduced"
    return set(vals)


def _export_dev(s, max_keys):
    import torch
    from act_amd import capi
    buf = torch.zeros(32 * max_keys, dtype=torch.uint8, device="cuda")
    cur, parts = 0, []
    while cur != capi.EXPORT_DONE:
        cur, got = s.export_dev(cur, max_keys, buf.data_ptr())
        parts.append(buf[:32 * got].cpu().numpy().tobytes())
    return b"".join(parts)


def test_export_equals_the_model():
    from act_amd import capi
    r = random.Random(1)
    pool = [r.randrange(ELL) for _ in range(1500)]
    s = capi.NullifierSet(3000, salt=bytes(range(16)))
    model = set()
    _fill(s, model, r, pool, 4, 500)
    assert len(s) == len(model)
    for mk in (1, 3, 1000, 1 << 20):
        assert _as_set(s.export(mk)) == model, mk
        assert _as_set(_export_dev(s, mk)) == model, mk
    # a device buffer that is not 16-byte aligned goes through the staging buffer
    import torch
    buf = torch.zeros(32 * 4000 + 8, dtype=torch.uint8, device="cuda")
    cur, got = s.export_dev(0, 4000, buf.data_ptr() + 8)
    assert cur != capi.EXPORT_DONE or got == len(model)
    part = _as_set(buf[8:8 + 32 * got].cpu().numpy().tobytes())
    assert part <= model
    s.close()


def test_contains_equals_the_model_and_changes_nothing(engine_factory, bench_params):
    from act_amd import capi
    r = random.Random(2)
    pool = [r.randrange(ELL) for _ in range(2000)]
    s = capi.NullifierSet(5000)
    model = set()
    _fill(s, model, r, pool[:1000], 3, 400)
    n0 = len(s)
    probe = pool[800:1200] + [v + ELL for v in pool[900:950] if v + ELL < 2**256] + [r.randrange(ELL) for _ in range(50)]
    want = bytes(1 if v % ELL in model else 0 for v in probe)
    assert s.contains(b"".join(_le(v) for v in probe)) == want
    # the stride of SpendProof records: the `k` field read straight out of them
    eng = engine_factory(bench_params, 8, max_batch=64)
    pb = eng.proof_bytes
    recs = b"".join(_le(v) + bytes(r.randrange(256) for _ in range(pb - 32)) for v in probe)
    assert s.contains(recs, stride=pb) == want
    assert len(s) == n0 and _as_set(s.export()) == model
    # device memory
    import torch
    d_keys = torch.from_numpy(np.frombuffer(recs, np.uint8).copy()).cuda()
    d_out = torch.full((len(probe),), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s.contains_dev(len(probe), d_keys.data_ptr(), pb, d_out.data_ptr())
    assert d_out.cpu().numpy().tobytes() == want
    # later check-and-insert answers are those of a set that was never queried
    _fill(s, model, r, pool, 2, 300)
    assert len(s) == len(model)
    s.close()


def test_growth_after_a_refused_batch():
    from act_amd import capi
    r = random.Random(3)
    pool = [r.randrange(ELL) for _ in range(6000)]
    s = capi.NullifierSet(1000, salt=b"\x07" * 16)               # 2048 slots: room for 1024 keys
    model = set()
    _fill(s, model, r, pool[:900], 2, 450)
    n0 = len(s)
    vals = _batch(r, pool[900:], 600)
    mask = bytes(1 if i % 9 == 0 else 0 for i in range(len(vals)))
    with pytest.raises(capi.ActError):
        s.check_and_insert(b"".join(_le(v) for v in vals), skip_mask=mask)
    out = np.zeros(len(vals), np.uint8)
    keys = np.frombuffer(b"".join(_le(v) for v in vals), np.uint8); m = np.frombuffer(mask, np.uint8)
    rc = s.lib.act_nullifier_check_and_insert_batch(s.h, len(vals), capi.MEM_HOST, keys.ctypes.data, 32, m.ctypes.data, out.ctypes.data)
    assert rc == 1 and list(out) == [0 if m else capi_undetermined() for m in mask] and len(s) == n0
    before = _as_set(s.export())
    cur, _ = s.export_step(0, 100)                                  # a cursor in the middle of the old table
    s.reserve(5000)
    assert len(s) == n0 and _as_set(s.export()) == before == model
    with pytest.raises(capi.ActError, match="stale"):
        s.export_step(cur, 100)
    # the same batch again: exactly the sequential model's answers
    keep = [v for v, m in zip(vals, mask) if not m]
    want = _model_step(model, keep)
    got = s.check_and_insert(b"".join(_le(v) for v in vals), skip_mask=mask)
    assert bytes(b for b, m in zip(got, mask) if not m) == want and all(got[i] == 0 for i in range(len(vals)) if mask[i])
    assert len(s) == len(model) and _as_set(s.export()) == model
    # a smaller capacity is a no-op (a cursor stays valid); more than 2^30 is refused and changes nothing
    cur, _ = s.export_step(0, 100)
    s.reserve(10)
    s.reserve(5000)
    s.export_step(cur, 100)
    with pytest.raises(capi.ActError):
        s.reserve((1 << 30) + 1)
    assert len(s) == len(model) and _as_set(s.export()) == model
    _fill(s, model, r, pool, 2, 500)
    s.close()


def capi_undetermined():
    return 2                                                        # ACT_NULLIFIER_UNDETERMINED


def test_round_trip_across_salt_and_size(tmp_path):
    from act_amd import capi
    r = random.Random(4)
    pool = [r.randrange(ELL) for _ in range(4000)]
    a = capi.NullifierSet(3000, salt=b"a" * 16)
    model = set()
    _fill(a, model, r, pool[:2500], 5, 400)
    p = str(tmp_path / "a.snap")
    assert a.save(p) == len(model)
    b = capi.NullifierSet.restore(p, capacity=10000, salt=b"b" * 16)
    assert len(b) == len(model)
    assert b.contains(b"".join(_le(v) for v in sorted(model))) == b"\1" * len(model)
    for _ in range(3):
        blob = b"".join(_le(v) for v in _batch(r, pool, 300))
        assert a.check_and_insert(blob) == b.check_and_insert(blob)
    b2 = str(tmp_path / "b.snap")
    b.save(b2); a.save(p)
    assert open(p, "rb").read() == open(b2, "rb").read()            # two sets with one content: byte-identical snapshots
    a.close(); b.close()


def _proofs(eng, sk, n, tag):
    pre = eng.pre_issuance_random(shake(tag + "-pre", 128 * n)); req = eng.request(pre, shake(tag + "-rq", 128 * n))
    st, resp = eng.issue(sk, req, b"".join(scb(30 + i) for i in range(n)), shake(tag + "-ir", 128 * n))
    st, tok = eng.issuance_to_credit_token(pre, sk[32:], req, resp)
    st, proofs, _ = eng.prove_spend(tok, b"".join(scb(i % 20) for i in range(n)), shake(tag + "-pr", eng.prove_rng_bytes * n))
    assert st == bytes(n)
    return proofs


def test_restart_through_the_product_path(engine_factory, bench_params, tmp_path):
    from act_amd import api, capi
    eng = engine_factory(bench_params, 8, max_batch=64)
    sk = eng.private_key_random(shake("ns-sk", 64))
    n = 10
    proofs = _proofs(eng, sk, n, "ns-a")
    a = capi.NullifierSet(100)
    st, _ = eng.redeem(a, sk, proofs, shake("ns-r1", 128 * n))
    assert st == bytes(n) and len(a) == n
    p = str(tmp_path / "issuer.snap")
    a.save(p); a.close()
    b = capi.NullifierSet.restore(p, capacity=100)
    st, rf = eng.redeem(b, sk, proofs, shake("ns-r2", 128 * n))
    assert list(st) == [3] * n and rf == bytes(128 * n)             # ACT_STATUS_DOUBLE_SPEND on every lane after the restart
    fresh = _proofs(eng, sk, 4, "ns-b")
    st, _ = eng.redeem(b, sk, fresh, shake("ns-r3", 128 * 4))
    assert st == bytes(4) and len(b) == n + 4
    b.close()
    # the API mirror: NullifierDb.save / restore + PrivateKey.redeem_batch
    params = api.Params.new("test-org", "test-service", "test", "2024-01-01")
    rng = api.OsRng()
    ask = api.PrivateKey.random(rng, params)
    toks = []
    for _ in range(3):
        pre = api.PreIssuance.random(rng, params); req = pre.request(params, rng)
        toks.append(pre.to_credit_token(params, ask.public(), req, ask.issue(params, req, 20, rng)))
    spends = [t.prove_spend(params, 5, rng)[0] for t in toks]
    db = api.NullifierDb(1 << 10)
    assert all(isinstance(x, api.Refund) for x in ask.redeem_batch(params, db, spends, rng))
    q = str(tmp_path / "db.snap")
    assert db.save(q) == 3
    db2 = api.NullifierDb.restore(q, capacity=1 << 10)
    res = ask.redeem_batch(params, db2, spends, rng)
    assert all(isinstance(x, api.Error) and x.name == "DoubleSpendError" for x in res)
    db2.reserve(1 << 12)
    assert len(db2) == 3 and db2.spend_batch([sp.nullifier() for sp in spends]) == [False] * 3


def test_node_form(tmp_path):
    from act_amd import capi
    r = random.Random(6)
    pool = [r.randrange(ELL) for _ in range(3000)]
    a = capi.NodeNullifierSet(4000, devices=(0, 0))
    model = set()
    _fill(a, model, r, pool[:2000], 4, 500)
    for mk in (7, 1000, 1 << 20):                                   # the cursor covers both parts
        assert _as_set(a.export(mk)) == model, mk
    p = str(tmp_path / "node.snap")
    assert a.save(p) == len(model)
    b = capi.NodeNullifierSet.restore(p, 2000, devices=(0, 0, 0))
    c = capi.NullifierSet.restore(p, capacity=8000)
    assert len(b) == len(c) == len(model)
    probe = b"".join(_le(v) for v in pool[1500:2500])
    want = bytes(1 if v in model else 0 for v in pool[1500:2500])
    assert a.contains(probe) == b.contains(probe) == c.contains(probe) == want
    for _ in range(3):
        blob = b"".join(_le(v) for v in _batch(r, pool, 400))
        assert a.check_and_insert(blob) == b.check_and_insert(blob) == c.check_and_insert(blob)
    # node reserve: every part grows, nothing is lost, a cursor inside a grown part is refused
    cur, _ = b.export_step(0, 10)
    n0 = len(b)
    b.reserve(20000)
    assert len(b) == n0 and _as_set(b.export()) == _as_set(c.export())
    with pytest.raises(capi.ActError):
        b.export_step(cur, 10)
    for s in (a, b, c):
        s.close()


def test_four_million_keys():
    import torch
    from act_amd import capi
    n = 1 << 22
    g = np.random.default_rng(7)
    raw = g.integers(0, 256, size=(n, 32), dtype=np.uint8)
    raw[:, 31] &= 0x0F                                              # below 2^252 < l: every key already reduced, all distinct w.h.p.
    s = capi.NullifierSet(n, salt=b"s" * 16)
    d_keys = torch.from_numpy(raw.reshape(-1)).cuda()
    d_out = torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s.check_and_insert_dev(n, d_keys.data_ptr(), 32, 0, d_out.data_ptr())
    assert int(d_out.sum().item()) == 0 and len(s) == n
    exported = _export_dev(s, 1 << 23)
    assert len(exported) == 32 * n
    ex = np.frombuffer(exported, np.uint8).reshape(n, 32)
    assert np.array_equal(np.unique(ex.view("S32").reshape(-1)), np.unique(raw.view("S32").reshape(-1)))
    s.close()
    b = capi.NullifierSet(1024)
    from act_amd import nullifier_snapshot
    nullifier_snapshot.restore_into(b, exported)
    assert len(b) == n
    b.contains_dev(n, d_keys.data_ptr(), 32, d_out.data_ptr())
    assert int(d_out.sum().item()) == n
    b.close()


def test_node_restore_reserves_each_devices_share_and_grows_a_full_one(tmp_path):
    from act_amd import capi
    r = random.Random(8)
    vals = [r.randrange(ELL) for _ in range(6000)]
    blob = b"".join(_le(v) for v in vals)
    s = capi.NodeNullifierSet(1000, devices=(0, 0))              # 2048 slots per device: room for 1024 keys each
    with pytest.raises(capi.ActError):
        s.check_and_insert(blob)                                 # each device's bucket is refused, nothing recorded
    assert len(s) == 0
    assert s.check_and_insert_growing(blob) == bytes(len(vals))  # grown twice, the refused lanes resubmitted
    assert len(s) == len(vals) and s.capacity_per_device >= 3000 and _as_set(s.export()) == set(vals)
    p = str(tmp_path / "n.snap")
    s.save(p); s.close()
    b = capi.NodeNullifierSet.restore(p, devices=(0, 0, 0))
    assert len(b) == len(vals) and b.capacity_per_device < len(vals)      # about a third of the keys per device, not all of them
    assert b.contains(blob) == b"\1" * len(vals)
    assert b.check_and_insert(blob[:3200] + _le(vals[0] + ELL)) == b"\1" * 101
    b.close()


def test_sharded_save_and_restore_on_the_hip_shard(tmp_path):
    import os
    import socket
    import torch
    import torch.distributed as dist
    from act_amd.sharded_nullifier import ShardedNullifierSet
    from act_amd import nullifier_snapshot
    sock = socket.socket(); sock.bind(("127.0.0.1", 0)); port = sock.getsockname()[1]; sock.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        a = ShardedNullifierSet(10_000, device=0)
        empty = a.save(str(tmp_path / "empty-{rank}.bin"))            # an empty shard still writes a (0-key) snapshot
        assert nullifier_snapshot.read(empty) == b""
        r = random.Random(9)
        vals = [r.randrange(ELL) for _ in range(3000)]
        keys = torch.tensor([list(_le(v)) for v in vals], dtype=torch.uint8).cuda()
        assert int(a.check_and_insert(keys).sum().item()) == 0
        path = a.save(str(tmp_path / "shard-{rank}.bin"))
        b = ShardedNullifierSet(100, device=0)
        b.restore([path, empty])
        assert len(b) == len(vals)
        assert b.contains(keys).cpu().tolist() == [1] * len(vals)
        assert int(b.check_and_insert(keys[:10]).sum().item()) == 10
        a.close(); b.close()
    finally:
        dist.destroy_process_group()
