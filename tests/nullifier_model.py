"""Shared by the tests that pin the nullifier set's slot function and probe loops (tests/test_nullifier_hash_host.py): SipHash restated from the paper (Aumasson, Bernstein: "SipHash: a fast short-input PRF",
section 3) in plain integers, a numpy form of SipHash-1-3 over 32-byte keys for searching, the search for keys that start at a
chosen slot of the persistent table and of the batch table, and the order-independent model of a linear-probing table.  Nothing here
reads the product's code.  Not a test module."""
import numpy as np

ELL = 2**252 + 27742317777372353535851937790883648493
M64 = (1 << 64) - 1
BLOCK = 1 << 20          # candidates hashed at a time by aim()
LIMIT = 1 << 24          # candidates after which aim() gives up


def _rotl(x, b):
    return ((x << b) | (x >> (64 - b))) & M64


def _sipround(v):
    v0, v1, v2, v3 = v
    v0 = (v0 + v1) & M64; v1 = _rotl(v1, 13); v1 ^= v0; v0 = _rotl(v0, 32)
    v2 = (v2 + v3) & M64; v3 = _rotl(v3, 16); v3 ^= v2
    v0 = (v0 + v3) & M64; v3 = _rotl(v3, 21); v3 ^= v0
    v2 = (v2 + v1) & M64; v1 = _rotl(v1, 17); v1 ^= v2; v2 = _rotl(v2, 32)
    return [v0, v1, v2, v3]


def siphash(key16: bytes, msg: bytes, c: int, d: int) -> int:
    """SipHash-c-d of msg under the 16-byte key: c rounds per 8-byte word, d rounds of finalisation, 64-bit result"""
    assert len(key16) == 16
    k0, k1 = int.from_bytes(key16[:8], "little"), int.from_bytes(key16[8:], "little")
    v = [k0 ^ 0x736f6d6570736575, k1 ^ 0x646f72616e646f6d, k0 ^ 0x6c7967656e657261, k1 ^ 0x7465646279746573]
    n = len(msg)
    whole = n - n % 8
    # the message as little-endian words; the last one holds the remaining bytes and, in its top byte, the length mod 256
    words = [int.from_bytes(msg[i:i + 8], "little") for i in range(0, whole, 8)]
    words.append(int.from_bytes(msg[whole:], "little") | (n & 0xFF) << 56)
    for m in words:
        v[3] ^= m
        for _ in range(c):
            v = _sipround(v)
        v[0] ^= m
    v[2] ^= 0xFF
    for _ in range(d):
        v = _sipround(v)
    return v[0] ^ v[1] ^ v[2] ^ v[3]


def key_hash(k: int, salt16: bytes) -> int:
    """the slot hash of the set's key k (a reduced scalar): SipHash-1-3 of its 32 little-endian bytes under the salt"""
    assert 0 <= k < ELL
    return siphash(salt16, k.to_bytes(32, "little"), 1, 3)


def start_slot(k: int, salt16: bytes, cap: int) -> int:
    """where the probe sequence of key k starts in a persistent table of cap slots: the HIGH half of the hash"""
    return (key_hash(k, salt16) >> 32) & (cap - 1)


def batch_slot(k: int, salt16: bytes, batch_cap: int) -> int:
    """... and in the batch table of one call: the LOW half"""
    return key_hash(k, salt16) & (batch_cap - 1)


def sip13_keys(words: np.ndarray, salt16: bytes) -> np.ndarray:
    """SipHash-1-3 of N 32-byte keys, words: (N, 4) uint64 (little-endian words of each key) -> (N,) uint64"""
    words = np.ascontiguousarray(words, dtype=np.uint64)
    assert words.ndim == 2 and words.shape[1] == 4 and len(salt16) == 16
    u = np.uint64
    k0, k1 = u(int.from_bytes(salt16[:8], "little")), u(int.from_bytes(salt16[8:], "little"))
    n = len(words)
    v0 = np.full(n, k0 ^ u(0x736f6d6570736575)); v1 = np.full(n, k1 ^ u(0x646f72616e646f6d))
    v2 = np.full(n, k0 ^ u(0x6c7967656e657261)); v3 = np.full(n, k1 ^ u(0x7465646279746573))
    rot = lambda x, b: (x << u(b)) | (x >> u(64 - b))

    def rnd(v0, v1, v2, v3):
        v0 = v0 + v1; v1 = rot(v1, 13) ^ v0; v0 = rot(v0, 32)
        v2 = v2 + v3; v3 = rot(v3, 16) ^ v2
        v0 = v0 + v3; v3 = rot(v3, 21) ^ v0
        v2 = v2 + v1; v1 = rot(v1, 17) ^ v2; v2 = rot(v2, 32)
        return v0, v1, v2, v3

    with np.errstate(over="ignore"):
        for m in [words[:, i] for i in range(4)] + [np.full(n, u(32 << 56))]:
            v3 = v3 ^ m
            v0, v1, v2, v3 = rnd(v0, v1, v2, v3)
            v0 = v0 ^ m
        v2 = v2 ^ u(0xFF)
        for _ in range(3):
            v0, v1, v2, v3 = rnd(v0, v1, v2, v3)
    return v0 ^ v1 ^ v2 ^ v3


def words_to_int(row) -> int:
    return sum(int(x) << (64 * i) for i, x in enumerate(row))


def int_to_words(ks) -> np.ndarray:
    return np.array([[(k >> (64 * i)) & M64 for i in range(4)] for k in ks], dtype=np.uint64).reshape(len(ks), 4)


_blocks = {}


def _block(salt16: bytes, rng_seed: int, b: int):
    """block b of the candidates of (salt, seed): 2^20 scalars below 2^252 and their hashes; hashed once per process"""
    key = (bytes(salt16), rng_seed, b)
    if key not in _blocks:
        w = np.random.default_rng([rng_seed, b]).integers(0, 1 << 64, size=(BLOCK, 4), dtype=np.uint64)
        w[:, 3] &= np.uint64((1 << 60) - 1)             # 3 * 64 + 60 = 252 bits: below l, so already reduced
        _blocks[key] = (w, sip13_keys(w, salt16))
    return _blocks[key]


def aim(salt, cap, slot, count, *, batch_cap=None, batch_slots=None, rng_seed):
    """`count` distinct reduced scalars whose probe sequence starts at `slot` of a persistent table of `cap` slots (slot None: anywhere)
    and, where batch_cap is given, at one of `batch_slots` of a batch table of batch_cap slots.  The same (salt, seed) walks the same
    candidates, so a larger request for the same slots returns the smaller one's keys first."""
    assert cap & (cap - 1) == 0 and (slot is None or 0 <= slot < cap) and (batch_cap is None) == (batch_slots is None)
    out = []
    for b in range(LIMIT // BLOCK):
        w, h = _block(salt, rng_seed, b)
        hit = np.ones(BLOCK, bool) if slot is None else ((h >> np.uint64(32)) & np.uint64(cap - 1)) == np.uint64(slot)
        if batch_cap is not None:
            assert batch_cap & (batch_cap - 1) == 0
            hit &= np.isin(h & np.uint64(batch_cap - 1), np.array(sorted(batch_slots), dtype=np.uint64))
        idx = np.flatnonzero(hit)[:count - len(out)]
        out += [words_to_int(w[i]) for i in idx]
        if len(out) >= count:
            assert len(set(out)) == count and all(k < ELL for k in out)
            return out
    raise AssertionError("aim: %d of %d keys after 2^24 candidates (slot %r of %d, batch slots %r of %r)" % (len(out), count, slot, cap, batch_slots, batch_cap))


class LinearTable:
    """A table of `cap` slots under linear probing without deletion.  insert() places keys one at a time, each at the first free slot
    from its start -- for a sequence of single inserts that IS the table.  For keys that arrive together, which key takes which slot
    of a run depends on who came first, but the SET of occupied slots does not (a key starting at s fills the first free slot at or
    after s, and the union of the filled slots is the same for every order), and every key lies between its start and the first
    empty slot behind it: occupied() and run_of() are what a concurrent batch is compared with."""

    def __init__(self, cap, salt=None):
        assert cap & (cap - 1) == 0
        self.cap, self.salt = cap, salt
        self.at = {}           # slot -> key
        self.start = {}        # key -> start slot
        self.slot = {}         # key -> slot (sequential placement)

    def insert(self, key, start=None):
        """-> the slot of `key` (placed now or earlier)"""
        if key in self.slot:
            return self.slot[key]
        assert len(self.at) < self.cap
        s = start_slot(key, self.salt, self.cap) if start is None else start
        self.start[key] = s
        while s in self.at:
            s = (s + 1) & (self.cap - 1)
        self.at[s] = key; self.slot[key] = s
        return s

    def occupied(self):
        return set(self.at)

    def run_of(self, key, start=None):
        """the slots from the key's start up to (not including) the first empty slot; the key need not be in the table"""
        s = self.start[key] if key in self.start else (start_slot(key, self.salt, self.cap) if start is None else start)
        run = []
        while s in self.at and len(run) < self.cap:
            run.append(s); s = (s + 1) & (self.cap - 1)
        return run
