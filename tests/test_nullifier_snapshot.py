"""Nullifier snapshots (anonymous-credit-tokens_amd/nullifier_snapshot.py) and the sharded set's save / restore / contains, without a
GPU: the v1 encoding pinned byte for byte, every damaged file refused before anything is inserted, and two gloo ranks that save their
shards and restore them into a fresh two-rank set (from the per-rank files and from one combined file) against the sequential model
of the reference tests' NullifierDb."""
import hashlib
import os
import random
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import act_amd  # noqa: E402,F401
from act_amd import nullifier_snapshot as snap  # noqa: E402

ELL = snap.ELL


def _le(v: int) -> bytes:
    return v.to_bytes(32, "little")


def _by_hand(values) -> bytes:
    """the v1 layout written out independently of the module: reduce, de-duplicate, sort by the little-endian bytes"""
    body = b"".join(sorted({_le(v % ELL) for v in values}))
    head = b"ACTNULS1" + (len(body) // 32).to_bytes(8, "little")
    return head + body + hashlib.sha256(head + body).digest()


FIXED = [0, 1, 5, 7, 5, ELL - 1, ELL, ELL + 5, 2**256 - 1, 2**200 + 3, 2**252 + 9]


def test_v1_encoding_is_pinned():
    keys = b"".join(_le(v) for v in FIXED)
    data = snap.encode(keys)
    assert data == _by_hand(FIXED)
    assert hashlib.sha256(data).hexdigest() == "129f170cc9b90d9d880917cc1b6a25ffa7ebadb8ba5bb4959fce212087707eef"
    # k and k + l (5 / l + 5, 0 / l) collapse to one entry each; 5 given twice is saved once
    assert int.from_bytes(data[8:16], "little") == len({v % ELL for v in FIXED}) == 8


def test_rust_binding_pins_the_same_encoding():
    """rust/src/mi355x.rs writes the format itself (GpuNullifierStore::save); its unit test encodes the same fixture and must
    expect the same digest as the pin above"""
    rs = open(os.path.join(ROOT, "rust", "src", "mi355x.rs")).read()
    test = rs[rs.index("fn encoding_matches_the_python_pin"):]
    assert "129f170cc9b90d9d880917cc1b6a25ffa7ebadb8ba5bb4959fce212087707eef" in test[:2000]


def test_round_trip(tmp_path):
    r = random.Random(5)
    vals = [r.randrange(2**256) for _ in range(3000)] + [r.randrange(ELL) for _ in range(3000)]
    vals += [v + ELL for v in vals[3000:3100]]                       # aliases of keys already in the list
    keys = b"".join(_le(v) for v in vals)
    p = str(tmp_path / "s.bin")
    assert snap.write(p, keys) == len({v % ELL for v in vals})
    got = snap.read(p)
    assert {int.from_bytes(got[i:i + 32], "little") for i in range(0, len(got), 32)} == {v % ELL for v in vals}
    # two saves of the same set are byte-identical, whatever order and spelling the keys came in
    shuffled = vals[:]; r.shuffle(shuffled)
    assert snap.encode(b"".join(_le(v) for v in shuffled)) == open(p, "rb").read()
    assert snap.read(str(tmp_path / "s.bin")) == got
    assert snap.decode(snap.encode(b"")) == b""


def _reseal(head_and_body: bytes) -> bytes:
    return head_and_body + hashlib.sha256(head_and_body).digest()


def _damaged():
    good = _by_hand([3, 10, 99, 2**100])
    n = 4
    body = good[16:16 + 32 * n]
    keys = [body[32 * i:32 * i + 32] for i in range(n)]
    head = lambda c: b"ACTNULS1" + c.to_bytes(8, "little")
    return {
        "bad magic": b"ACTNULS2" + good[8:],
        "truncated": good[:-1],
        "trailing bytes": good + b"\0",
        "wrong count": _reseal(head(n + 1) + body),
        "wrong checksum": good[:-1] + bytes([good[-1] ^ 1]),
        "key not below l": _reseal(head(n) + b"".join(keys[:3]) + _le(ELL + 1)),
        "key equal to l": _reseal(head(n) + b"".join(keys[:3]) + _le(ELL)),
        "out of order": _reseal(head(n) + keys[1] + keys[0] + keys[2] + keys[3]),
        "repeated key": _reseal(head(n) + keys[0] + keys[1] + keys[1] + keys[3]),
        "empty file": b"",
    }


class _Recorder:
    """stand-in for a nullifier set: records every call that would change it"""

    def __init__(self):
        self.calls = []

    def __len__(self):
        return 0

    def reserve(self, c):
        self.calls.append(("reserve", c))

    def check_and_insert(self, keys, stride=32, skip_mask=None):
        self.calls.append(("insert", len(keys)))
        return bytes(len(keys) // 32)


@pytest.mark.parametrize("case", sorted(_damaged()))
def test_damaged_snapshot_is_refused_before_any_insert(tmp_path, case):
    p = str(tmp_path / "bad.bin")
    open(p, "wb").write(_damaged()[case])
    target = _Recorder()
    with pytest.raises(snap.SnapshotError):
        snap.restore_file(target, p)
    assert target.calls == []


def test_intact_snapshot_restores_through_check_and_insert(tmp_path):
    p = str(tmp_path / "ok.bin")
    vals = list(range(1, 2500))
    snap.write(p, b"".join(_le(v) for v in vals))
    target = _Recorder()
    assert snap.restore_file(target, p, chunk=1000) == len(vals)
    assert target.calls == [("reserve", len(vals)), ("insert", 32 * 1000), ("insert", 32 * 1000), ("insert", 32 * 499)]


# ---- the sharded set on two gloo ranks --------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _key(i: int) -> int:
    """key id -> scalar; odd ids above 1000 are spelled k + l on the wire (the same nullifier as id - 1000)"""
    base = int.from_bytes(hashlib.shake_256(b"snap%d" % (i % 1000)).digest(32), "little") % ELL
    return base + ELL if i >= 1000 and base + ELL < 2**256 else base


def _batch(seed: int, rank: int, n: int):
    r = random.Random(seed * 7 + rank)
    return [r.randrange(400) + (1000 if r.random() < 0.1 else 0) for _ in range(n)]


class _DictShardX:
    """Test-only local shard with the extended protocol: check-and-insert, contains, export (keys arrive reduced)."""

    def __init__(self):
        self.db = set()
        self.reserved = []

    def check_and_insert_tensor(self, keys):
        out = torch.zeros(keys.shape[0], dtype=torch.uint8)
        for i in range(keys.shape[0]):
            k = bytes(keys[i].tolist())
            if k in self.db:
                out[i] = 1
            else:
                self.db.add(k)
        return out

    def contains_tensor(self, keys):
        return torch.tensor([1 if bytes(keys[i].tolist()) in self.db else 0 for i in range(keys.shape[0])], dtype=torch.uint8)

    def export_tensor(self):
        rows = sorted(self.db)
        return torch.tensor([list(k) for k in rows], dtype=torch.uint8).reshape(len(rows), 32)

    def reserve(self, c):
        self.reserved.append(c)

    def __len__(self):
        return len(self.db)


def _tensor(ids):
    return torch.tensor([list(_le(_key(i))) for i in ids], dtype=torch.uint8).reshape(len(ids), 32)


def _sequential(db, per_rank):
    out = []
    for ids in per_rank:
        row = []
        for i in ids:
            k = _key(i) % ELL
            row.append(1 if k in db else 0)
            db.add(k)
        out.append(row)
    return out


def _worker(rank, world, port, tmp, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from act_amd.sharded_nullifier import ShardedNullifierSet
    try:
        a = ShardedNullifierSet(0, local_set=_DictShardX())
        for rnd in range(3):
            a.check_and_insert(_tensor(_batch(rnd, rank, [50, 300, 120][rnd])))
        path = a.save(os.path.join(tmp, "shard-{rank}-of-{world}.bin"))
        dist.barrier()
        if rank == 0:                                                       # one combined file of both shards
            both = snap.read(os.path.join(tmp, "shard-0-of-2.bin")) + snap.read(os.path.join(tmp, "shard-1-of-2.bin"))
            snap.write(os.path.join(tmp, "combined.bin"), both)
        dist.barrier()
        res = {"saved": path}
        for name, paths in (("per_rank", [os.path.join(tmp, "shard-%d-of-2.bin" % r) for r in range(world)]),
                            ("combined", [os.path.join(tmp, "combined.bin")])):
            shard = _DictShardX()
            b = ShardedNullifierSet(0, local_set=shard)
            b.restore(paths, chunk=64)
            own_ok = all(int.from_bytes(k[:8], "little") % (1 << 63) % world == rank for k in shard.db)
            restored = sorted(shard.db)
            probe = list(range(0, 500, 3)) + [1001, 1003, 1399]
            found = b.contains(_tensor(probe)).tolist()
            later = [b.check_and_insert(_tensor(_batch(10 + rnd, rank, [40, 200][rnd]))).tolist() for rnd in range(2)]
            res[name] = (own_ok, restored, found, later, shard.reserved)
        # a damaged file read by one rank stops every rank before anything is inserted
        open(os.path.join(tmp, "broken.bin"), "wb").write(b"ACTNULS1" + bytes(8))
        shard = _DictShardX()
        c = ShardedNullifierSet(0, local_set=shard)
        try:
            c.restore([os.path.join(tmp, "combined.bin"), os.path.join(tmp, "broken.bin")])
            res["damaged"] = "accepted"
        except snap.SnapshotError:
            res["damaged"] = len(shard.db)
        q.put((rank, res))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_two_rank_save_and_restore_match_the_sequential_set(tmp_path):
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, str(tmp_path), q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(world):
        rank, got = q.get(timeout=300)
        res[rank] = got
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    db = set()
    for rnd in range(3):
        _sequential(db, [_batch(rnd, r, [50, 300, 120][rnd]) for r in range(world)])
    saved = db.copy()
    probe = list(range(0, 500, 3)) + [1001, 1003, 1399]
    for name in ("per_rank", "combined"):
        model = saved.copy()
        later = [_sequential(model, [_batch(10 + rnd, r, [40, 200][rnd]) for r in range(world)]) for rnd in range(2)]
        held = set()
        for rank in range(world):
            own_ok, keys, found, got_later, reserved = res[rank][name]
            assert own_ok, (name, rank)
            held |= {int.from_bytes(k, "little") for k in keys}
            assert found == [1 if _key(i) % ELL in saved else 0 for i in probe], (name, rank)
            for rnd in range(2):
                assert got_later[rnd] == later[rnd][rank], (name, rank, rnd)
            assert reserved and reserved[0] >= 1
        assert held == saved, name
    assert res[0]["damaged"] == 0 and res[1]["damaged"] == 0
