"""Snapshot files of a nullifier set: what an issuer saves at shutdown and loads at start ("restart and growth").

Format v1, versioned and self-checking:

    0        8 B    magic b"ACTNULS1"
    8        8 B    count n, u64 little-endian
    16       32n B  keys: reduced scalars (< l), strictly ascending in memcmp order
    16+32n   32 B   SHA-256 of bytes [0, 16+32n)

Format v2 carries the epoch of every key and the set's retired epochs (include/act_mi355x.h "Epochs").  It is written ONLY when a set
holds a non-zero epoch or a retired epoch; any other set saves the v1 bytes above.  `decode_epochs` / `read_epochs` accept both.

    0          8 B   magic b"ACTNULS2"
    8          8 B   n  (u64 LE)  keys
    16         8 B   r  (u64 LE)  retired epochs
    24         32n   keys: reduced scalars, strictly ascending in memcmp order          (as v1)
    24+32n     4n    epochs: u32 LE, epochs[i] belongs to keys[i], each <= 2^24 - 1
    24+36n     4r    retired epochs: u32 LE, strictly ascending, each in 1 .. 2^24 - 1
    24+36n+4r  32 B  SHA-256 of everything before

The v2 reader refuses everything v1 refuses plus: an epoch out of range, a retired list out of order / repeated / containing 0, a
key whose epoch is in the retired list.  (ShardedNullifierSet keeps v1.)

The writer reduces, sorts and de-duplicates, so two saves of the same set are byte-identical.  The reader refuses a wrong magic,
a length that disagrees with the count, a checksum mismatch, a key not below l and keys out of order or repeated.  `restore_into`
validates the whole file before it inserts anything: a damaged snapshot that loaded partly would silently re-enable double
spends.  Pure Python + numpy; the sets themselves are the HIP tables behind capi.NullifierSet / NodeNullifierSet.
"""
import hashlib
import os

import numpy as np

MAGIC = b"ACTNULS1"
MAGIC_V2 = b"ACTNULS2"
EPOCH_MAX = (1 << 24) - 1
ELL = 2**252 + 27742317777372353535851937790883648493
_ELL_BE = np.frombuffer(ELL.to_bytes(32, "big"), dtype="S32")[0]


class SnapshotError(ValueError):
    """The file is not an intact nullifier snapshot."""


def _rows(keys) -> np.ndarray:
    a = np.frombuffer(bytes(keys), dtype=np.uint8) if isinstance(keys, (bytes, bytearray, memoryview)) else np.ascontiguousarray(keys, dtype=np.uint8)
    if a.size % 32:
        raise ValueError(f"keys: {a.size} bytes is not a whole number of 32-byte nullifiers")
    return a.reshape(-1, 32)


def _not_below_l(rows: np.ndarray) -> np.ndarray:
    """[n,32] little-endian rows -> [n] bool, value >= l (compared big-endian, as bytes)"""
    return np.ascontiguousarray(rows[:, ::-1]).view("S32").reshape(-1) >= _ELL_BE


def canonical(keys) -> bytes:
    """32-byte nullifiers (any representative) -> their reduced scalars, sorted in memcmp order, each once"""
    rows = _rows(keys).copy()
    for i in np.nonzero(_not_below_l(rows))[0]:
        rows[i] = np.frombuffer((int.from_bytes(rows[i].tobytes(), "little") % ELL).to_bytes(32, "little"), np.uint8)
    return np.unique(rows.view("S32").reshape(-1)).tobytes() if rows.shape[0] else b""


def encode(keys) -> bytes:
    body = canonical(keys)
    head = MAGIC + (len(body) // 32).to_bytes(8, "little")
    return head + body + hashlib.sha256(head + body).digest()


def decode(data: bytes) -> bytes:
    """a whole snapshot -> its keys (n*32 bytes), or SnapshotError"""
    data = bytes(data)
    if len(data) < 48 or data[:8] != MAGIC:
        raise SnapshotError("not a nullifier snapshot (bad magic or shorter than header + checksum)")
    n = int.from_bytes(data[8:16], "little")
    if len(data) != 16 + 32 * n + 32:
        raise SnapshotError(f"length {len(data)} disagrees with count {n} (expected {16 + 32 * n + 32}): truncated or trailing bytes")
    if hashlib.sha256(data[:16 + 32 * n]).digest() != data[16 + 32 * n:]:
        raise SnapshotError("checksum mismatch")
    body = data[16:16 + 32 * n]
    rows = _rows(body)
    if n and _not_below_l(rows).any():
        raise SnapshotError(f"key {int(np.nonzero(_not_below_l(rows))[0][0])} is not a reduced scalar (>= l)")
    s = rows.view("S32").reshape(-1)
    if n > 1 and not (s[1:] > s[:-1]).all():
        raise SnapshotError(f"keys out of order or repeated at index {int(np.nonzero(~(s[1:] > s[:-1]))[0][0]) + 1}")
    return body


def write(path: str, keys) -> int:
    """keys -> file at `path` (written beside it, then renamed into place); returns the number of keys saved"""
    data = encode(keys)
    tmp = f"{path}.tmp{os.getpid()}"
    with open(tmp, "wb") as f:
        f.write(data)
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, path)
    return (len(data) - 48) // 32


def read(path: str) -> bytes:
    with open(path, "rb") as f:
        return decode(f.read())


def restore_file(target, path: str, chunk: int = 1 << 20) -> int:
    """read + validate the whole file, then restore_into; returns the number of keys in the snapshot"""
    keys = read(path)
    restore_into(target, keys, chunk)
    return len(keys) // 32


def restore_into(target, keys: bytes, chunk: int = 1 << 20) -> None:
    """validated keys -> `target` (anything with reserve / check_and_insert / len): reserved first for what it holds plus the
    snapshot, then fed through check-and-insert in chunks, so any salt, capacity or device count takes the snapshot.  A target
    spread over devices says what to reserve per device (restore_capacity) and may insert through check_and_insert_growing."""
    n = len(keys) // 32
    per = getattr(target, "restore_capacity", None)
    target.reserve(per(n) if per else len(target) + n)
    insert = getattr(target, "check_and_insert_growing", target.check_and_insert)
    for i in range(0, n, chunk):
        insert(keys[32 * i:32 * min(n, i + chunk)])


# ---- format v2: keys with epochs, and the retired epochs ---------------------------------------------------------------------------
def canonical_epochs(keys, epochs):
    """32-byte nullifiers (any representative) with their epochs -> (reduced scalars sorted in memcmp order, each once; their epochs)"""
    rows = _rows(keys).copy()
    ep = np.ascontiguousarray(epochs, dtype=np.uint32).reshape(-1)
    if len(ep) != rows.shape[0]:
        raise ValueError(f"{len(ep)} epochs for {rows.shape[0]} keys")
    for i in np.nonzero(_not_below_l(rows))[0]:
        rows[i] = np.frombuffer((int.from_bytes(rows[i].tobytes(), "little") % ELL).to_bytes(32, "little"), np.uint8)
    if not rows.shape[0]:
        return b"", ep
    s = rows.view("S32").reshape(-1)
    order = np.argsort(s, kind="stable")
    s, ep = s[order], ep[order]
    first = np.ones(len(s), bool); first[1:] = s[1:] != s[:-1]
    group = np.cumsum(first) - 1
    if (ep != ep[first][group]).any():
        raise ValueError("one nullifier under two epochs")
    return s[first].tobytes(), np.ascontiguousarray(ep[first])


def encode_epochs(keys, epochs, retired=()) -> bytes:
    """v2 bytes -- or the v1 bytes of encode(keys) when every epoch is 0 and nothing is retired"""
    body, ep = canonical_epochs(keys, epochs)
    ret = np.unique(np.asarray(list(retired), dtype=np.uint64))
    if (ep > EPOCH_MAX).any() or (len(ret) and (ret[0] == 0 or ret[-1] > EPOCH_MAX)):
        raise ValueError("an epoch above 2^24 - 1, or a retired epoch 0")
    if np.isin(ep, ret).any():
        raise ValueError("a key under a retired epoch")
    if not ep.any() and not len(ret):
        return encode(body)
    n = len(body) // 32
    data = MAGIC_V2 + n.to_bytes(8, "little") + len(ret).to_bytes(8, "little") + body + ep.astype("<u4").tobytes() + ret.astype("<u4").tobytes()
    return data + hashlib.sha256(data).digest()


def decode_epochs(data: bytes):
    """a whole snapshot of either version -> (keys bytes, epochs uint32 array, retired epochs list), or SnapshotError"""
    data = bytes(data)
    if data[:8] != MAGIC_V2:
        keys = decode(data)
        return keys, np.zeros(len(keys) // 32, np.uint32), []
    if len(data) < 56:
        raise SnapshotError("not a nullifier snapshot (shorter than header + checksum)")
    n, r = int.from_bytes(data[8:16], "little"), int.from_bytes(data[16:24], "little")
    end = 24 + 36 * n + 4 * r
    if len(data) != end + 32:
        raise SnapshotError(f"length {len(data)} disagrees with counts {n} / {r} (expected {end + 32}): truncated or trailing bytes")
    if hashlib.sha256(data[:end]).digest() != data[end:]:
        raise SnapshotError("checksum mismatch")
    body = data[24:24 + 32 * n]
    rows = _rows(body)
    if n and _not_below_l(rows).any():
        raise SnapshotError(f"key {int(np.nonzero(_not_below_l(rows))[0][0])} is not a reduced scalar (>= l)")
    s = rows.view("S32").reshape(-1)
    if n > 1 and not (s[1:] > s[:-1]).all():
        raise SnapshotError(f"keys out of order or repeated at index {int(np.nonzero(~(s[1:] > s[:-1]))[0][0]) + 1}")
    ep = np.frombuffer(data, "<u4", n, 24 + 32 * n).astype(np.uint32)
    ret = np.frombuffer(data, "<u4", r, 24 + 36 * n).astype(np.uint32)
    if (ep > EPOCH_MAX).any():
        raise SnapshotError(f"epoch of key {int(np.nonzero(ep > EPOCH_MAX)[0][0])} is above 2^24 - 1")
    if r and (ret[0] == 0 or (ret > EPOCH_MAX).any()):
        raise SnapshotError("retired epoch out of range (0, or above 2^24 - 1)")
    if r > 1 and not (ret[1:] > ret[:-1]).all():
        raise SnapshotError("retired epochs out of order or repeated")
    if np.isin(ep, ret).any():
        raise SnapshotError(f"key {int(np.nonzero(np.isin(ep, ret))[0][0])} is recorded under a retired epoch")
    return body, ep, [int(e) for e in ret]


def write_epochs(path: str, keys, epochs, retired=()) -> int:
    """as write(); v1 bytes when the set never saw an epoch"""
    data = encode_epochs(keys, epochs, retired)
    tmp = f"{path}.tmp{os.getpid()}"
    with open(tmp, "wb") as f:
        f.write(data)
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, path)
    return int.from_bytes(data[8:16], "little")


def read_epochs(path: str):
    with open(path, "rb") as f:
        return decode_epochs(f.read())


def restore_epochs_into(target, keys: bytes, epochs, retired=(), chunk: int = 1 << 20) -> None:
    """validated keys, epochs and retired list -> `target`: reserved as restore_into reserves, the keys inserted grouped by epoch
    through the epoch insert, then the listed epochs retired (they hold no keys, so nothing is removed: it re-arms the refusal)."""
    n = len(keys) // 32
    epochs = np.asarray(epochs, dtype=np.uint32)
    per = getattr(target, "restore_capacity", None)
    target.reserve(per(n) if per else len(target) + n)
    rows = _rows(keys)
    growing = getattr(target, "check_and_insert_growing", None)
    for e in np.unique(epochs):
        sub = np.ascontiguousarray(rows[epochs == e]).tobytes()
        for i in range(0, len(sub) // 32, chunk):
            part = sub[32 * i:32 * (i + chunk)]
            if growing:
                growing(part, epoch=int(e))
            elif e:
                target.check_and_insert(part, epochs=[int(e)])
            else:
                target.check_and_insert(part)
    for e in retired:
        target.retire_epoch(int(e))
