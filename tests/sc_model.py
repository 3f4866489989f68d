"""Big-integer restatement of csrc/sc25519.h, statement for statement: the three-stage fold of sc_reduce512, sc_from_words, the
Montgomery product scm_mul on its exact limbs and the two limb conversions of sc_invert.  Word arrays of the header are integers here,
cut to the width of the array that holds them, so a value the header's comments promise to fit and that does not fit goes wrong here
as it would there -- and every such promise is asserted on the way (ModelViolation).  The model returns the intermediates, so the
tests can say which road a case took (how many conditional subtractions, how large h1 and h2 were).

Nothing here is the expected value of a test by itself: tests/test_sc_edges_host.py holds the model to plain `% ELL` arithmetic
first, and the host and device builds to the model after that."""
from collections import namedtuple

C = 27742317777372353535851937790883648493           # l - 2^252, 125 bits
ELL = 2**252 + C
W256 = (1 << 256) - 1
L_WORDS = (0x5cf5d3ed, 0x5812631a, 0xa2f79cd6, 0x14def9de, 0, 0, 0, 0x10000000)          # sc_l_word
assert sum(w << (32 * i) for i, w in enumerate(L_WORDS)) == ELL


class ModelViolation(AssertionError):
    """A bound that a comment of sc25519.h promises does not hold for this input."""


def promise(ok, what, *values):
    if not ok:
        raise ModelViolation(what + ": " + ", ".join(hex(v) for v in values))


def words(x, n):
    """x as an array of n 32-bit words holds it"""
    return x & ((1 << (32 * n)) - 1)


def split252(x, n):
    """bn_split252<N>: lo = x mod 2^252 in 8 words, hi = x >> 252 in N - 7 words"""
    return x & ((1 << 252) - 1), words(x >> 252, n - 7)


def cond_sub_l(r, times):
    """sc_cond_sub_l on r < 2^256: (r after at most `times` subtractions of l, how many were taken).  bn_sub's borrow out of eight
    words is r < l."""
    promise(0 <= r <= W256, "sc_cond_sub_l takes eight words", r)
    taken = 0
    for _ in range(times):
        d = (r - ELL) & W256
        if r >= ELL:                                  # no borrow
            r, taken = d, taken + 1
    return r, taken


Fold = namedtuple("Fold", "r lo0 h0 y1 lo1 h1 y2 lo2 h2 y3 A B subs")


def reduce512(x, times=4):
    """sc_reduce512 on sixteen words.  `times` is the argument of the final sc_cond_sub_l (4 in the header)."""
    promise(0 <= x < 1 << 512, "sc_reduce512 takes sixteen words", x)
    lo0, h0 = split252(x, 16)
    promise(h0 < 1 << 260, "h0 < 2^260", h0)
    y1 = words(h0 * C, 13)                            # bn_mul<9, 4>
    promise(h0 * C < 1 << 385, "y1 < 2^385", h0 * C)
    lo1, h1 = split252(y1, 13)
    promise(h1 < 1 << 133, "h1 < 2^133", h1)
    y2 = words(h1 * C, 10)                            # bn_mul<6, 4>
    promise(h1 * C < 1 << 258, "y2 < 2^258", h1 * C)
    lo2, h2 = split252(y2, 10)
    promise(h2 < 1 << 6, "h2 < 2^6", h2)
    y3 = words(h2 * C, 7)                             # bn_mul<3, 4>, seven words written and y3[7] = 0
    promise(h2 * C < 1 << 131, "y3 < 2^131", h2 * C)
    l2 = words(ELL + ELL, 8)
    A = words(lo0 + lo2, 8)
    promise(A + l2 < 1 << 256, "A < 2^256", A + l2)
    A = words(A + l2, 8)
    B = words(lo1 + y3, 8)
    promise(A >= B, "A >= B", A, B)
    r, subs = cond_sub_l(words(A - B, 8), times)
    return Fold(r, lo0, h0, y1, lo1, h1, y2, lo2, h2, y3, A, B, subs)


def from_words(w):
    """sc_from_words on eight words: (result, 1 if the conditional subtraction was taken else 0)"""
    promise(0 <= w <= W256, "sc_from_words takes eight words", w)
    q = w >> 252
    lo = w & ((1 << 252) - 1)
    qc = words(q * C, 5)                              # bn_mul<1, 4>
    r = words(lo + ELL, 8)
    r = words(r - qc, 8)
    return cond_sub_l(r, 1)


def add(a, b):
    """sc_add on raw words: (result, subtraction taken)"""
    return cond_sub_l(words(a + b, 8), 1)


def sub(a, b):
    """sc_sub on raw words: (result, subtraction taken)"""
    return cond_sub_l(words(words(a + ELL, 8) - b, 8), 1)


def neg(a):
    return sub(0, a)


def half(a):
    """sc_half: the sum a + (l if a is odd) is formed in eight words and shifted"""
    return words(a + (ELL if a & 1 else 0), 8) >> 1


def mul(a, b):
    """sc_mul: the Fold of the 512-bit product"""
    return reduce512(words(a * b, 16))


def muladd(a, b, c):
    """sc_muladd: (result, the product's Fold, sc_add's subtraction taken)"""
    f = mul(a, b)
    r, taken = add(f.r, c)
    return r, f, taken


# ---- the Montgomery arithmetic inside sc_invert: ten limbs of 26 bits, R = 2^260 -------------------------------------------------
SCM_LIMBS = 10
SCM_MASK = (1 << 26) - 1
NPRIME = 0x2547e1b
SCM_L = (0x0f5d3ed, 0x098c697, 0x1cd6581, 0x37a8bde, 0x014def9, 0, 0, 0, 0, 0x0040000)          # scm_l
R = 1 << 260
R1 = (0x321e6ed, 0x3d22f59, 0x067e45a, 0x0eead6b, 0x335e51b, 0x3fffffa, 0x3ffffff, 0x3ffffff, 0x3ffffff, 0x003ffff)
R2 = (0x152d13b, 0x274997a, 0x1bea69f, 0x358f1c5, 0x3687604, 0x16f9972, 0x33d217f, 0x0f73bb1, 0x37c309a, 0x0025046)
U64 = (1 << 64) - 1
U32 = (1 << 32) - 1


def limbs_val(limbs):
    return sum(v << (26 * i) for i, v in enumerate(limbs))


def val_limbs(x):
    """x < 2^260 in ten 26-bit limbs"""
    assert 0 <= x < R
    return [(x >> (26 * i)) & SCM_MASK for i in range(SCM_LIMBS)]


assert limbs_val(SCM_L) == ELL and limbs_val(R1) == R % ELL and limbs_val(R2) == R * R % ELL and (ELL * NPRIME + 1) % (1 << 26) == 0

peak_column = [0]          # the largest 64-bit column any scm_mul of this process has held


def scm_mul(a, b, lazy_bound=True, scm_l=SCM_L):
    """scm_mul on exact limbs (lists of ten values below 2^32): the ten result limbs.  Every column is held to its 64 bits, the top
    limb to its 26; with lazy_bound and operands below 2 l the result is held below 2 l."""
    col = [0] * (2 * SCM_LIMBS)

    def acc(k, v):
        col[k] += v
        promise(col[k] <= U64, "scm_mul column %d < 2^64" % k, col[k])
        peak_column[0] = max(peak_column[0], col[k])

    for i in range(SCM_LIMBS):
        for j in range(SCM_LIMBS):
            acc(i + j, a[i] * b[j])
    for i in range(SCM_LIMBS):
        m = (((col[i] & U32) * NPRIME) & U32) & SCM_MASK
        for j in range(SCM_LIMBS):
            if j < 5 or j == 9:
                acc(i + j, m * scm_l[j])
        promise(col[i] & SCM_MASK == 0, "the low 26 bits of column %d are zero after its step" % i, col[i])
        acc(i + 1, col[i] >> 26)
    out = [0] * SCM_LIMBS
    for k in range(SCM_LIMBS, 2 * SCM_LIMBS - 1):
        acc(k + 1, col[k] >> 26)
        out[k - SCM_LIMBS] = col[k] & U32 & SCM_MASK
    out[SCM_LIMBS - 1] = col[2 * SCM_LIMBS - 1] & U32
    promise(col[2 * SCM_LIMBS - 1] < 1 << 26, "top output limb < 2^26", col[2 * SCM_LIMBS - 1])
    if lazy_bound and limbs_val(a) < 2 * ELL and limbs_val(b) < 2 * ELL:
        promise(limbs_val(out) < 2 * ELL, "operands below 2 l give a result below 2 l", limbs_val(a), limbs_val(b), limbs_val(out))
    return out


M_FULL = (-pow(ELL, -1, R)) % R


def scm_mul_value(a, b):
    """The integer scm_mul returns for operands of 26-bit limbs with the values a, b: (a b + m l) / R with the one m < R that makes
    the division exact -- what the ten interleaved steps add up to (test_sc_edges_host.py holds the two forms together)."""
    t = a * b
    m = t * M_FULL % R
    return (t + m * ELL) >> 260


def to_limbs26(a):
    """sc_invert's 8 x 32 bits -> 10 x 26 bits, on the eight words of a"""
    w = [(a >> (32 * i)) & U32 for i in range(8)]
    al = []
    for i in range(SCM_LIMBS):
        bit = 26 * i
        k, sh = bit >> 5, bit & 31
        v = w[k] >> sh
        if sh > 6 and k + 1 < 8:
            v |= (w[k + 1] << (32 - sh)) & U32
        al.append(v & SCM_MASK)
    return al


def to_words32(o):
    """sc_invert's 10 x 26 bits -> 8 x 32 bits: the integer of the eight words"""
    r = 0
    for w in range(8):
        bit = 32 * w
        i, sh = bit // 26, bit % 26
        v = o[i] >> sh
        if i + 1 < SCM_LIMBS:
            v |= (o[i + 1] << (26 - sh)) & U32
        if sh > 20 and i + 2 < SCM_LIMBS:
            v |= (o[i + 2] << (52 - sh)) & U32
        r |= (v & U32) << bit
    return r


Invert = namedtuple("Invert", "r before_sub subs peak")          # peak: the largest Montgomery value on the way


def invert(a, exact_limbs=False):
    """sc_invert on eight raw words.  exact_limbs runs every one of the 328 products limb by limb (columns checked); otherwise they run
    on values (scm_mul_value, the same integers) and the bound `below 2 l` is checked on each."""
    if exact_limbs:
        prod = scm_mul
    else:
        def prod(x, y):
            v = scm_mul_value(limbs_val(x), limbs_val(y))
            promise(v < 2 * ELL, "operands below 2 l give a result below 2 l", limbs_val(x), limbs_val(y), v)
            return val_limbs(v)
    promise(0 <= a < 2 * ELL, "sc_invert's Montgomery products take operands below 2 l", a)
    al = to_limbs26(a)
    promise(limbs_val(al) == a, "the 26-bit limbs hold the operand", a, limbs_val(al))
    am = prod(al, list(R2))
    acc = list(R1)
    peak = 0
    e = ELL - 2
    for i in range(252, -1, -1):
        acc = prod(acc, acc)
        if (e >> i) & 1:
            acc = prod(acc, am)
        peak = max(peak, limbs_val(acc))
    o = prod(acc, [1] + [0] * 9)
    before = to_words32(o)
    promise(before == limbs_val(o), "the eight words hold the result", limbs_val(o), before)
    r, subs = cond_sub_l(before, 1)
    return Invert(r, before, subs, peak)
