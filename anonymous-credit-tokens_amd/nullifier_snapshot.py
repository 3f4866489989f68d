"""Snapshot files of a nullifier set: what an issuer saves at shutdown and loads at start ("restart and growth").

Format v1, versioned and self-checking:

    0        8 B    magic b"ACTNULS1"
    8        8 B    count n, u64 little-endian
    16       32n B  keys: reduced scalars (< l), strictly ascending in memcmp order
    16+32n   32 B   SHA-256 of bytes [0, 16+32n)

The writer reduces, sorts and de-duplicates, so two saves of the same set are byte-identical.  The reader refuses a wrong magic,
a length that disagrees with the count, a checksum mismatch, a key not below l and keys out of order or repeated.  `restore_into`
validates the whole file before it inserts anything: a damaged snapshot that loaded partly would silently re-enable double
spends.  Pure Python + numpy; the sets themselves are the HIP tables behind capi.NullifierSet / NodeNullifierSet.
"""
import hashlib
import os

import numpy as np

MAGIC = b"ACTNULS1"
ELL = 2**252 + 27742317777372353535851937790883648493
_ELL_BE = np.frombuffer(ELL.to_bytes(32, "big"), dtype="S32")[0]


class SnapshotError(ValueError):
    """The file is not an intact v1 nullifier snapshot."""


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
