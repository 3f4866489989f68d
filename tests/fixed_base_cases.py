"""Scalars for the fixed-base products (msm.h fixed_base_acc over k_build_table's tables) at any window width w in 4..24, shared by
the host test (tests/test_fixed_base_widths_host.py) and the device tests (tests/test_gpu_fixed_base_widths.py).

Two sets.  The EDGE set does not depend on w: 0, the smallest and largest canonical scalars, every single bit 2^k (which puts a bit
in every digit position of every window whatever the width), 2^252 +- 1 around the top bit, one non-canonical value and a few
random ones.  Its expected encodings come from the Python model.  The WINDOW set depends on w: scalars e * 2^(w * pos) -- one
table entry each -- over every entry of every window (w <= 8) or the entries at a window's edges plus seeded (pos, e) pairs (w > 8),
the largest top digit a canonical scalar can have, and strings of all-ones windows.  Its expected encodings come from the C oracle.
Where the two sets meet, both references are asked and must agree (Expected.window)."""
import hashlib

ELL = 2**252 + 27742317777372353535851937790883648493
N_RANDOM_PAIRS = 1024            # seeded (pos, e) pairs per width above 8 bits


def _shake(label: str, n: int) -> bytes:
    return hashlib.shake_256(label.encode()).digest(n)


def windows(w: int) -> int:
    return -(-253 // w)


def edge_scalars() -> list:
    """As 32-byte strings: the one non-canonical value (2^256 - 1) has to reach the loader unreduced."""
    v = [0, 1, 2, ELL - 1, ELL - 2, (1 << 252) - 1, 1 << 252] + [1 << k for k in range(253)] + [(1 << 256) - 1]
    v += [int.from_bytes(_shake("fixed-base-edge-%d" % i, 64), "little") % ELL for i in range(8)]
    return [x.to_bytes(32, "little") for x in v]


def window_scalars(w: int, pairs: int = N_RANDOM_PAIRS) -> list:
    """Canonical scalars (ints below l), each value once, in a fixed order."""
    nw, full = windows(w), (1 << w) - 1
    top_shift = w * (nw - 1)
    top_digit = (ELL - 1) >> top_shift                      # the largest digit the top window of a canonical scalar holds
    out = []
    if w <= 8:
        out += [e << (w * pos) for pos in range(nw) for e in range(1 << w)]
    else:
        out += [e << (w * pos) for pos in range(nw) for e in (1, 2, 1 << (w - 1), full - 1, full)]
        rnd = _shake("fixed-base-pairs-w%d" % w, 8 * pairs)
        for i in range(pairs):
            pos = int.from_bytes(rnd[8 * i:8 * i + 4], "little") % nw
            e = int.from_bytes(rnd[8 * i + 4:8 * i + 8], "little") & full
            out.append(e << (w * pos))
    out.append(top_digit << top_shift)
    low = (1 << top_shift) - 1                              # every window below the top one all-ones ...
    out.append(low + (top_digit << top_shift) if low + (top_digit << top_shift) < ELL else low + ((top_digit - 1) << top_shift))
    for phase in (0, 1):                                    # all-ones and zero windows in turn
        v = 0
        for pos in range(phase, nw, 2):
            d = full if pos < nw - 1 else min(full, top_digit - 1)
            v += d << (w * pos)
        out.append(v)
    seen, uniq = set(), []
    for x in out:
        if x < ELL and x not in seen:
            seen.add(x); uniq.append(x)
    return uniq


def digits(v: int, w: int) -> list:
    """The table entries fixed_base_acc reads for v: digit pos = bits [w pos, w pos + w) of v."""
    return [(v >> (w * pos)) & ((1 << w) - 1) for pos in range(windows(w))]


class Expected:
    """Expected encodings of s * B for one base B (a 32-byte encoding; None = the generator): the edge set through the Python model,
    computed once, everything else through the C oracle; a scalar both know is asked of both."""

    def __init__(self, oracle, base_enc=None):
        import pymodel as m
        self.m, self.oracle, self.base_enc = m, oracle, base_enc
        self.pt = m.BASEPOINT if base_enc is None else m.ristretto_decode(base_enc)
        self.edge = edge_scalars()
        self.edge_want = [m.ristretto_encode(m.pt_mul(self.pt, int.from_bytes(s, "little") % ELL)) for s in self.edge]
        self.by_value = {int.from_bytes(s, "little"): e for s, e in zip(self.edge, self.edge_want)}
        assert self.edge_want[0] == bytes(32)                # 0 * B: the identity

    def oracle_mul(self, v: int) -> bytes:
        s = v.to_bytes(32, "little")
        return self.oracle.mul_base(s) if self.base_enc is None else self.oracle.mul(self.base_enc, s)

    def window(self, w: int, pairs: int = N_RANDOM_PAIRS):
        """(scalars as bytes, expected encodings) of width w's window set"""
        vals = window_scalars(w, pairs)
        want = []
        for v in vals:
            e = self.oracle_mul(v)
            if v in self.by_value:
                assert e == self.by_value[v], ("the two references disagree", hex(v))
            want.append(e)
        return [v.to_bytes(32, "little") for v in vals], want

    def lanes(self, w: int, pairs: int = N_RANDOM_PAIRS):
        """edge set + window set of width w: (scalar bytes, concatenated; expected encodings, concatenated; the scalars as a list)"""
        ws, ww = self.window(w, pairs)
        sc = self.edge + ws
        return b"".join(sc), b"".join(self.edge_want + ww), sc


# ---- protocol level: SpendProof records whose scalars are chosen ------------------------------------------------------------------
def crafted_spend_proofs(proof: bytes, L: int, pats: list) -> list:
    """One record per pattern from one honest proof (tests/test_gpu_parity.py test_crafted_scalars_reproduce_the_oracle_transcript):
    gamma = pats[n], gamma0_j and z_j0 walk through pats.  Invalid by construction; what the verifier recomputes is in the transcript."""
    scb = lambda v: (v % ELL).to_bytes(32, "little")
    N = len(pats)
    recs = []
    for n, v in enumerate(pats):
        t = bytearray(proof)
        t[32 * (4 + L):32 * (5 + L)] = scb(v)                                           # gamma
        for j in range(L):
            w = pats[(n + j) % N]
            t[32 * (12 + L + j):32 * (13 + L + j)] = scb(w)                             # gamma0_j
            t[32 * (12 + 2 * L + 2 * j):32 * (13 + 2 * L + 2 * j)] = scb(pats[(n + 2 * j + 1) % N])       # z_j0
        recs.append(bytes(t))
    nc = bytearray(recs[3]); nc[32 * (4 + L):32 * (5 + L)] = ((1 << 253) - 1).to_bytes(32, "little"); recs[3] = bytes(nc)   # gamma >= l
    return recs


def protocol_scalars(w: int) -> list:
    """What the fixed-base products of a protocol call are aimed at, at width w: the ends of the scalar range, the lone top bit, the
    top window's largest digit, the all-ones strings, and both edge entries of a few windows (bottom, middle, last full one)."""
    nw, full = windows(w), (1 << w) - 1
    ws = window_scalars(w, 0)
    v = [0, 1, ELL - 1, ELL - 2, 1 << 252, (1 << 252) - 1] + ws[-4:]
    for pos in sorted({0, 1, nw // 2, nw - 2}):
        v += [full << (w * pos), 1 << (w * pos), (1 << (w - 1)) << (w * pos)]
    return [x for x in v if x < ELL]


def steer_fixed_base_fields(recs: list, L: int, vals: list) -> list:
    """The same records with the scalars that feed fixed-base products (spend_lanes.h: k, c_bar, r_bar, w00, w01, z_j1, k_bar, s_bar)
    set so that the PRODUCT's scalar -- after the verifier's own arithmetic on the field -- is a value of `vals`:
      h2 gets -gamma k, h1 gets -c_bar - gamma s (the tail kernel's product; A2's takes c_bar as it is), the range kernel works on halves (w00 / 2, w01 / 2, z_j1 / 2); r_bar, k_bar and
      s_bar go in as they are."""
    import pymodel as m
    scb = lambda v: (v % ELL).to_bytes(32, "little")
    get = lambda t, f: int.from_bytes(t[32 * f:32 * f + 32], "little") % ELL
    out = []
    M = len(vals)
    for n, rec in enumerate(recs):
        t = bytearray(rec)
        put = lambda f, v: t.__setitem__(slice(32 * f, 32 * f + 32), scb(v))
        pick = lambda i: vals[(7 * n + i) % M]
        gamma, s = get(t, 4 + L), get(t, 1)
        put(0, -pick(0) * m.sc_inv(gamma) if gamma else pick(0))                         # k: h2 gets -gamma k
        put(8 + L, -(pick(1) + gamma * s))                                               # c_bar: h1 gets -c_bar - gamma s
        put(9 + L, pick(2))                                                              # r_bar
        put(10 + L, 2 * pick(3)); put(11 + L, 2 * pick(4))                               # w00, w01 (halved)
        put(12 + 4 * L, pick(5)); put(13 + 4 * L, pick(6))                               # k_bar, s_bar
        for j in range(L):
            put(12 + 2 * L + 2 * j + 1, 2 * vals[(7 * n + 11 * j + 5) % M])              # z_j1 (halved)
        out.append(bytes(t))
    return out
