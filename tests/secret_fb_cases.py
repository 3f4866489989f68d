"""Scalars for the products of SECRET scalars (msm.h fixed_base_acc_mf, chain_ct, chain_ct_quarter), shared by the host tests
(tests/test_secret_fb_cases_host.py, tests/test_hostcheck.py) and the device test (tests/test_gpu_secret_products.py).  Importable
without a GPU and without the library.

FIXED-BASE LANES.  fixed_base_acc_mf recodes a scalar into 37 signed 7-bit digits and, per window, picks entry |digit| of 64 on the
matrix cores: the one-hot operand is built per lane, the table operand's rows are loaded by all 64 lanes, the result changes lane
halves twice.  So a look-up can be wrong for one (window, entry) -- a byte of the table image in the wrong slot -- or for one lane, and
a case has to put a chosen digit into a chosen window IN a chosen lane.  The family is fixed_base_cases.edge_scalars() followed by
fixed_base_cases.window_scalars(7), 4 846 scalars.  They reach all 4 610 (window, signed digit) pairs a canonical scalar can produce:
every digit -64 .. 63 in windows 0 .. 35, and 0 and 1 in window 36 (which holds bit 252 alone).  The other 126 pairs -- entries
2 .. 64 of the top window, in either sign -- are read by no scalar below l, so nothing can test them through the product.  In list
order the window set puts digit i mod 128 into the lane i mod 64 it started from, two entries per lane; the family is therefore the
list under all 64 ROTATIONS -- rotation r pads the front with r zero scalars, so scalar i runs in lane (i + r) mod 64 -- and every
reachable pair then meets every lane, both lane halves and both one-hot operands.  Expected encodings are computed once (the Python
model for the edge set, the C oracle for the rest, both where they meet: fixed_base_cases.Expected) and rotated with the scalars:
0 * B encodes as 32 zero bytes.

MIXED WAVEFRONTS.  4 096 seeded scalars: every lane of a wavefront holds its own digit in every window (almost surely all different
from its neighbours' and non-zero), where the window set keeps 63 of 64 lanes' other windows at digit 0.

CHAIN LANES.  chain_points() x chain_scalars(): the recoding corners of the radix-4 chain (next_digit4's carry) for the whole chain
of 127 steps and for each of chain_ct_quarter's four 33-step pieces, whose last step exists for the carry alone.

mf_digits() restates the recoding on Python integers.  It DESCRIBES what a case aims at (coverage, failure messages); no expected
value comes from it."""
import fixed_base_cases as fb
from fixed_base_cases import ELL, _shake

MF_WBITS, MF_WINDOWS, MF_ENTRIES = 7, 37, 64          # msm.h MF_WBITS / MF_WINDOWS / MF_ENTRIES at ACT_MF_KSTEPS = 2
N_MIXED = 4096
N_CHAIN_RANDOM = 256


def mf_digits(s: int) -> list:
    """signed digit w of s, w = 0 .. 36: add the bias sum_w 64 * 2^(7 w), take 7-bit groups, subtract 64 from each"""
    t = s + sum(64 << (MF_WBITS * w) for w in range(MF_WINDOWS))
    return [((t >> (MF_WBITS * w)) & 127) - 64 for w in range(MF_WINDOWS)]


def fixed_scalars() -> list:
    """The fixed-base family in list order, as 32-byte strings (one of them, 2^256 - 1, not canonical: the loader reduces it)."""
    return fb.edge_scalars() + [v.to_bytes(32, "little") for v in fb.window_scalars(MF_WBITS)]


def value(s: bytes) -> int:
    """the scalar the product sees: reduced mod l on load"""
    return int.from_bytes(s, "little") % ELL


def rotate(scalars: bytes, want: bytes, r: int, pad_to: int = 64):
    """Rotation r of a lane list: r zero scalars in front (scalar i moves to lane (i + r) mod 64), zero scalars behind up to a
    multiple of pad_to, so that rotations can follow one another in one call without moving each other's lanes.  Expected
    encodings move with the scalars; a zero scalar's is 32 zero bytes."""
    n = len(scalars) // 32
    tail = -(r + n) % pad_to
    return bytes(32 * r) + scalars + bytes(32 * tail), bytes(32 * r) + want + bytes(32 * tail)


def mixed_scalars() -> list:
    return [(int.from_bytes(_shake("secret-fb-mixed-%d" % i, 64), "little") % ELL).to_bytes(32, "little") for i in range(N_MIXED)]


# ---- chains ---------------------------------------------------------------------------------------------------------------------------
def quarter_scalars() -> list:
    """Quarter q of the scalar all ones, the others zero: piece q of chain_ct_quarter is 2^64 - 1, whose 32 radix-4 digits are all 3,
    so the carry runs through all of them and the piece's 33rd step adds it.  The top quarter of a canonical scalar is at most
    (l - 1) >> 192 = 2^60, so there the all-ones value is 2^60 - 1 (the carry ends at step 31; no canonical scalar has a top piece
    that needs step 33)."""
    assert (ELL - 1) >> 192 == 1 << 60
    return [((1 << 64) - 1) << (64 * q) for q in range(3)] + [((1 << 60) - 1) << 192]


def chain_scalars() -> list:
    """32-byte strings.  Part 1: the fixed-base edge set; the radix-4 digit strings 1111.., 2222.., 3333.. (0x55.., 0xAA.., 0xFF..)
    cut to 252 bits; the quarter scalars.  Part 2: 2^(64 q) +- 1 around each piece's boundary, l - 1, l - 2, seeded random ones."""
    low252 = (1 << 252) - 1
    v = [int(c * 64, 16) & low252 for c in "5af"] + quarter_scalars()
    v += [(1 << (64 * q)) + d for q in range(4) for d in (-1, 1)] + [ELL - 1, ELL - 2]
    v += [int.from_bytes(_shake("secret-chain-%d" % i, 64), "little") % ELL for i in range(N_CHAIN_RANDOM)]
    assert all(0 <= x < ELL for x in v)
    return fb.edge_scalars() + [x.to_bytes(32, "little") for x in v]


def next_digit4(s: int, carry: int):
    """msm.h next_digit4 on integers: (digit in {0, 1, 2, -1, 0}, the scalar shifted down two bits, the new carry)"""
    v = (s & 3) + carry
    return (v if v < 3 else v - 4), s >> 2, int(v >= 3)


def chain_points(prim: dict, h: bytes) -> list:
    """prim = tests/golden/sodium_primitives.json, h = the context's Params (h1 | h2 | h3).  The first 64 points of libsodium's
    scalarmult records, the generator, the three h, the all-zero encoding (the identity) and two encodings that do not decode."""
    pts = [bytes.fromhex(x["point"]) for x in prim["scalarmult"][:64]]
    import pymodel as m
    gen = m.ristretto_encode(m.BASEPOINT)
    bad = [bytes.fromhex(x["bytes"]) for x in prim["decode_validity"] if not x["valid"]][:2]
    assert len(pts) == 64 and len(bad) == 2
    return pts + [gen, h[0:32], h[32:64], h[64:96], bytes(32)] + bad


def chain_lanes(prim: dict, h: bytes):
    """(points, scalars, scalars2, n_golden) as lists of 32-byte strings, lane by lane: libsodium's own (point, scalar) pairs for the 64
    golden points first, then every chain scalar on three points each (strides 1, 5, 11 through the point list, so every special
    scalar meets decodable points and every point -- the identity and the undecodable ones included -- meets many scalars).
    scalars2[i] is the scalar half the list further on: the second scalar of chain_ct<2>."""
    P, S = chain_points(prim, h), chain_scalars()
    pts = [bytes.fromhex(x["point"]) for x in prim["scalarmult"][:64]]
    scs = [bytes.fromhex(x["scalar"]) for x in prim["scalarmult"][:64]]
    for a, b in ((1, 0), (5, 1), (11, 2)):
        for k, s in enumerate(S):
            pts.append(P[(a * k + b) % len(P)]); scs.append(s)
    n = len(scs)
    return pts, scs, [scs[(i + n // 2) % n] for i in range(n)], 64
