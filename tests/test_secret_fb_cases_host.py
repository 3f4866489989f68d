"""What tests/secret_fb_cases.py promises about its families, checked without a GPU: the device test (tests/test_gpu_secret_products.py)
compares bytes, and only this file says that those bytes were aimed at every table entry the matrix-core look-up can be asked for,
from every lane, and at the carry of every chain piece."""
import secret_fb_cases as sf
from conftest import ELL


def reachable_pairs() -> set:
    """Every (window w, signed digit d) some canonical scalar has, worked out WITHOUT the recoding: the smallest non-negative scalar
    with digit d in window w is d * 2^(7 w), plus 2^(7 (w + 1)) -- a one in the next window -- when d is negative; a negative digit in
    the top window has no next window to borrow from.  The pair is reachable iff that scalar lies below l."""
    out = set()
    for w in range(sf.MF_WINDOWS):
        for d in range(-64, 64):
            v = d << (7 * w)
            if d < 0 and w < sf.MF_WINDOWS - 1:
                v += 1 << (7 * (w + 1))
            if 0 <= v < ELL:
                out.add((w, d))
    return out


def test_digits_resum_to_the_scalar():
    fam = sf.fixed_scalars() + sf.mixed_scalars() + sf.chain_scalars()
    assert len(sf.fixed_scalars()) == 4846 and len(sf.mixed_scalars()) == sf.N_MIXED
    for s in fam:
        v = sf.value(s)
        d = sf.mf_digits(v)
        assert len(d) == sf.MF_WINDOWS and all(-64 <= x <= 63 for x in d), s.hex()
        assert sum(x << (7 * w) for w, x in enumerate(d)) == v, s.hex()
        assert max(abs(x) for x in d) <= sf.MF_ENTRIES


def test_the_family_covers_exactly_the_reachable_pairs():
    want = reachable_pairs()
    assert len(want) == 4610
    assert want == {(w, d) for w in range(36) for d in range(-64, 64)} | {(36, 0), (36, 1)}
    got = {(w, d) for s in sf.fixed_scalars() for w, d in enumerate(sf.mf_digits(sf.value(s)))}
    assert not (want - got), sorted(want - got)[:8]
    assert not (got - want), sorted(got - want)[:8]
    # the 126 pairs nothing reaches: entries 2 .. 64 of the top window, in either sign (-1 and 2 .. 63 as digits, -64 .. -2)
    assert 37 * 128 - len(want) == 126
    # entry 64 exists as the digit -64 alone, and the family has it in every window below the top one
    assert {w for (w, d) in got if d == -64} == set(range(36))


def test_every_reachable_pair_meets_every_lane_over_the_rotations():
    fam = [sf.mf_digits(sf.value(s)) for s in sf.fixed_scalars()]
    at = {}                                     # pair -> bit mask of the lanes (i mod 64) that hold it in rotation 0
    for i, ds in enumerate(fam):
        for w, d in enumerate(ds):
            at[(w, d)] = at.get((w, d), 0) | 1 << (i % 64)
    full = (1 << 64) - 1
    rot = lambda m, r: ((m << r) | (m >> (64 - r))) & full          # lane (i + r) mod 64
    # unrotated, no non-zero digit of the windows' own entries is seen from all lanes: the rotations are the point
    assert all(m != full for (w, d), m in at.items() if d not in (0, 1))
    for pair, m in at.items():
        seen = 0
        for r in range(64):
            seen |= rot(m, r)
        assert seen == full, pair
    # and rotate() puts scalar i of rotation r at lane (i + r) mod 64, whole wavefronts each, zeros around it
    sc = b"".join(sf.fixed_scalars()[:130]); want = bytes(range(1, 131)) * 32
    for r in (0, 1, 37, 63):
        s2, w2 = sf.rotate(sc, want[:len(sc)], r)
        assert len(s2) == len(w2) and len(s2) % (64 * 32) == 0
        assert s2[32 * r:32 * r + len(sc)] == sc and w2[32 * r:32 * r + len(sc)] == want[:len(sc)]
        assert not any(s2[:32 * r]) and not any(s2[32 * r + len(sc):]) and not any(w2[:32 * r]) and not any(w2[32 * r + len(sc):])


def test_mixed_wavefronts_fill_every_window_of_every_lane():
    """per wavefront of 64 and window below the top one: at most a few zero digits, many different entries, both signs"""
    ds = [sf.mf_digits(sf.value(s)) for s in sf.mixed_scalars()]
    for lo in range(0, len(ds), 64):
        for w in range(36):
            col = [d[w] for d in ds[lo:lo + 64]]
            assert len({abs(x) for x in col}) >= 24 and col.count(0) <= 4 and min(col) < 0 < max(col), (lo, w)


def test_quarter_scalars_end_on_the_carry():
    """chain_ct_quarter gives piece q (64 bits) 33 steps: 32 digits and the recoding's carry.  For the all-ones pieces the carry is
    still 1 when step 33 begins and that step's digit is +1 -- from the carry alone, the piece's bits are used up.  The top piece of
    a canonical scalar has 61 bits; its all-ones value 2^60 - 1 hands the carry to step 31, and steps 32, 33 add nothing."""
    qs = sf.quarter_scalars()
    assert len(qs) == 4 and all(v < ELL for v in qs)
    for q, v in enumerate(qs):
        piece = (v >> (64 * q)) & ((1 << 64) - 1)
        assert v == piece << (64 * q) and piece == ((1 << 64) - 1 if q < 3 else (1 << 60) - 1)
        carry, digits, carries_in = 0, [], []
        for step in range(33):
            carries_in.append(carry)
            d, piece, carry = sf.next_digit4(piece, carry)
            digits.append(d)
        assert piece == 0 and carry == 0                      # 33 steps use the piece up
        last = 33 if q < 3 else 31                            # the step that takes the carry
        assert carries_in[last - 1] == 1 and digits[last - 1] == 1 and digits[0] == -1
        assert all(d == 0 for d in digits[1:last - 1]) and all(d == 0 for d in digits[last:])
        assert sum(d << (2 * i) for i, d in enumerate(digits)) == (v >> (64 * q))
    # the whole-chain walk of the same scalars: 127 steps, nothing left over
    for s in sf.chain_scalars():
        v, carry, acc = sf.value(s), 0, 0
        x = v
        for step in range(127):
            d, x, carry = sf.next_digit4(x, carry)
            acc += d << (2 * step)
        assert x == 0 and carry == 0 and acc == v, s.hex()
