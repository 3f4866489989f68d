"""Snapshot format v2 of the nullifier set (anonymous-credit-tokens_amd/nullifier_snapshot.py): keys with their epochs and the retired
epochs.  v2 is written only when there is something v1 cannot say; the reader takes both; every refusal rule is exercised on a valid
file that was corrupted and re-sealed, so that the rule and not the checksum fires."""
import hashlib
import random

import numpy as np
import pytest

from conftest import ELL

from act_amd import nullifier_snapshot as snap


def _le(v: int) -> bytes:
    return v.to_bytes(32, "little")


def _sample(seed=1, n=200):
    r = random.Random(seed)
    vals = sorted({r.randrange(ELL) for _ in range(n)}, key=lambda v: _le(v))
    epochs = [r.choice((0, 3, 3, 70000, (1 << 24) - 1)) for _ in vals]
    return vals, epochs


def _reseal(body: bytes) -> bytes:
    return body + hashlib.sha256(body).digest()


def _valid():
    vals, epochs = _sample()
    data = snap.encode_epochs(b"".join(_le(v) for v in vals), epochs, [9, 5])
    assert data[:8] == b"ACTNULS2"
    return vals, epochs, data


def test_round_trip():
    vals, epochs, data = _valid()
    n = len(vals)
    assert len(data) == 24 + 36 * n + 4 * 2 + 32
    assert int.from_bytes(data[8:16], "little") == n and int.from_bytes(data[16:24], "little") == 2
    keys, ep, retired = snap.decode_epochs(data)
    assert keys == b"".join(_le(v) for v in vals) and list(ep) == epochs and retired == [5, 9]
    # the writer reduces, sorts and de-duplicates (k and k + l are one key), carrying every key's epoch
    order = list(range(n)); random.Random(2).shuffle(order)
    spelled = [vals[i] + ELL if vals[i] + ELL < 2**256 and i % 3 == 0 else vals[i] for i in order]
    blob = b"".join(_le(v) for v in spelled) + _le(vals[order[0]])
    assert snap.encode_epochs(blob, [epochs[i] for i in order] + [epochs[order[0]]], (9, 5, 9)) == data
    with pytest.raises(ValueError):
        snap.encode_epochs(_le(vals[0]) + _le(vals[0]), [1, 2])     # one nullifier under two epochs
    with pytest.raises(ValueError):
        snap.encode_epochs(_le(vals[0]), [4], [4])                  # a key under a retired epoch
    with pytest.raises(ValueError):
        snap.encode_epochs(_le(vals[0]), [1 << 24])
    with pytest.raises(ValueError):
        snap.encode_epochs(_le(vals[0]), [1], [0])
    # only a retired list, no keys; only keys of one non-zero epoch
    assert snap.decode_epochs(snap.encode_epochs(b"", [], [7]))[2] == [7]
    k, e, r = snap.decode_epochs(snap.encode_epochs(_le(5), [6]))
    assert (k, list(e), r) == (_le(5), [6], [])


def test_a_set_without_epochs_encodes_to_v1_bytes(tmp_path):
    vals, _ = _sample(3)
    blob = b"".join(_le(v) for v in reversed(vals)) + _le(vals[0] + ELL)
    assert snap.encode_epochs(blob, [0] * (len(vals) + 1), ()) == snap.encode(blob)
    p = str(tmp_path / "s.snap")
    assert snap.write_epochs(p, blob, np.zeros(len(vals) + 1, np.uint32)) == len(vals)
    assert open(p, "rb").read() == snap.encode(blob) and snap.read(p) == snap.canonical(blob)


def test_the_new_reader_reads_v1(tmp_path):
    vals, _ = _sample(4)
    blob = b"".join(_le(v) for v in vals)
    keys, ep, retired = snap.decode_epochs(snap.encode(blob))
    assert keys == blob and list(ep) == [0] * len(vals) and retired == []
    p = str(tmp_path / "v1.snap")
    snap.write(p, blob)
    assert snap.read_epochs(p)[0] == blob
    # ... and refuses what v1 refuses
    bad = bytearray(snap.encode(blob)); bad[20] ^= 1
    with pytest.raises(snap.SnapshotError, match="checksum"):
        snap.decode_epochs(bytes(bad))
    with pytest.raises(snap.SnapshotError, match="magic"):
        snap.decode_epochs(b"ACTNULS3" + bytes(40))
    # the v1 reader does not take a v2 file for a v1 file
    with pytest.raises(snap.SnapshotError):
        snap.decode(_valid()[2])


def test_refuses_a_checksum_mismatch_and_a_wrong_length():
    _, _, data = _valid()
    for at in (9, 30, len(data) - 40, len(data) - 1):
        bad = bytearray(data); bad[at] ^= 0x10
        with pytest.raises(snap.SnapshotError):
            snap.decode_epochs(bytes(bad))
    bad = bytearray(data); bad[30] ^= 0x10
    with pytest.raises(snap.SnapshotError, match="checksum"):
        snap.decode_epochs(bytes(bad))
    for cut in (data[:-1], data + b"\0", data[:40], _reseal(data[:-32] + bytes(4))):
        with pytest.raises(snap.SnapshotError, match="length|shorter"):
            snap.decode_epochs(cut)


def _parts(data):
    n, r = int.from_bytes(data[8:16], "little"), int.from_bytes(data[16:24], "little")
    return n, r, 24, 24 + 32 * n, 24 + 36 * n


def test_refuses_a_key_that_is_not_reduced():
    _, _, data = _valid()
    n, r, k0, e0, r0 = _parts(data)
    body = bytearray(data[:-32]); body[k0 + 32 * (n - 1):k0 + 32 * n] = _le(ELL)
    with pytest.raises(snap.SnapshotError, match="reduced"):
        snap.decode_epochs(_reseal(bytes(body)))


def test_refuses_keys_out_of_order_or_repeated():
    _, _, data = _valid()
    n, r, k0, e0, r0 = _parts(data)
    body = bytearray(data[:-32])
    body[k0:k0 + 64] = body[k0 + 32:k0 + 64] + body[k0:k0 + 32]
    with pytest.raises(snap.SnapshotError, match="order"):
        snap.decode_epochs(_reseal(bytes(body)))
    body = bytearray(data[:-32]); body[k0 + 32:k0 + 64] = body[k0:k0 + 32]
    with pytest.raises(snap.SnapshotError, match="repeated"):
        snap.decode_epochs(_reseal(bytes(body)))


def test_refuses_an_epoch_out_of_range():
    _, _, data = _valid()
    n, r, k0, e0, r0 = _parts(data)
    body = bytearray(data[:-32]); body[e0 + 4 * 7:e0 + 4 * 8] = (1 << 24).to_bytes(4, "little")
    with pytest.raises(snap.SnapshotError, match="epoch of key 7"):
        snap.decode_epochs(_reseal(bytes(body)))


@pytest.mark.parametrize("retired,what", [((9, 5), "order"), ((5, 5), "repeated"), ((0, 5), "range"), ((5, 1 << 24), "range")])
def test_refuses_a_bad_retired_list(retired, what):
    _, _, data = _valid()
    n, r, k0, e0, r0 = _parts(data)
    body = bytearray(data[:-32]); body[r0:r0 + 8] = b"".join(e.to_bytes(4, "little") for e in retired)
    with pytest.raises(snap.SnapshotError, match=what):
        snap.decode_epochs(_reseal(bytes(body)))


def test_refuses_a_key_under_a_retired_epoch():
    vals, epochs, data = _valid()
    n, r, k0, e0, r0 = _parts(data)
    at = epochs.index(3)
    body = bytearray(data[:-32]); body[e0 + 4 * at:e0 + 4 * at + 4] = (5).to_bytes(4, "little")
    with pytest.raises(snap.SnapshotError, match="key %d is recorded under a retired epoch" % at):
        snap.decode_epochs(_reseal(bytes(body)))


class _ModelSet:
    """what restore_epochs_into needs of a set"""

    def __init__(self):
        self.keys, self.retired, self.reserved = {}, [], 0

    def __len__(self):
        return len(self.keys)

    def reserve(self, n):
        self.reserved = max(self.reserved, n)

    def check_and_insert(self, blob, epochs=None):
        e = epochs[0] if epochs else 0
        assert e not in self.retired
        out = []
        for i in range(0, len(blob), 32):
            out.append(1 if blob[i:i + 32] in self.keys else 0)
            self.keys.setdefault(blob[i:i + 32], e)
        return bytes(out)

    def retire_epoch(self, e):
        assert e not in self.keys.values()
        self.retired.append(e)
        return 0


def test_restore_inserts_by_epoch_then_retires(tmp_path):
    vals, epochs, data = _valid()
    p = str(tmp_path / "v2.snap")
    with open(p, "wb") as f:
        f.write(data)
    keys, ep, retired = snap.read_epochs(p)
    t = _ModelSet()
    snap.restore_epochs_into(t, keys, ep, retired, chunk=64)
    assert t.keys == {_le(v): e for v, e in zip(vals, epochs)} and t.retired == [5, 9] and t.reserved >= len(vals)
    # a v1 file restores as all-epoch-0
    t = _ModelSet()
    snap.restore_epochs_into(t, *snap.decode_epochs(snap.encode(keys)))
    assert set(t.keys.values()) == {0} and len(t) == len(vals) and t.retired == []
