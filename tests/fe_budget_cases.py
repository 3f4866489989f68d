"""Operands at the top of the limb-size classes of csrc/fe25519.h (its header comment), shared by the host tests of the field code
(test_hostcheck.py), the model of the generated device code (test_fe_asm_host.py) and the device test (test_gpu_fe_forms.py).

An element is nine limbs, limb i at bit POS[i] with WID[i] bits; its size phi is max_i limb_i / 2^WID[i]."""

P = 2**255 - 19
POS = [-(-85 * i // 3) for i in range(10)]
WID = [POS[i + 1] - POS[i] for i in range(9)]

# what fe_mul / fe_sq / fe_carry may leave in a limb ("tight": limb 1 takes the folded top carry)
tight_max = [(1 << w) + ((1 << 12) if i == 1 else 0) for i, w in enumerate(WID)]

# sizes (phi, gamma) of the two operands of a product: phi * gamma up to the 12.5 the header allows, every operand below phi = 7.5
pairs = [(1, 1), (2, 2), (3, 3), (4, 3), (3, 4), (6, 2), (2, 6), (7.4, 1.68), (1.68, 7.4), (5, 2.5), (3.5, 3.5)]

# the size pairs the range kernel's own calls have (ge25519.h writes them beside each call): ct * cx of the doubling, ge_add_ded
range_kernel_pairs = [(3, 4), (4, 3), (3, 3), (2, 3), (3, 2)]


def val(limbs):
    return sum(l << POS[i] for i, l in enumerate(limbs))


def operand(phi, kind, r):
    """Nine limbs of size phi: every limb at its top ("max"), every other one there and the rest at a third ("alt"), or drawn from
    the upper half of the range with the random.Random `r` (any other kind)."""
    top = [min(int(phi * (1 << w)), (1 << 32) - 1) for w in WID]
    if kind == "max":
        return top
    if kind == "alt":
        return [t if i % 2 else t // 3 for i, t in enumerate(top)]
    return [r.randrange(t // 2, t + 1) for t in top]


# ---- case lists of the field-form tests (test_fe_asm_host.py on the model, test_gpu_fe_forms.py on the device) --------------------
KINDS = ("max", "alt", "rnd", "rnd")
# fe_sqda_sq(f, a, fb) with f tight: the largest sizes of a and fb (in 1/256) at which the one-statement form overflows no column,
# wraps no register and returns the right tight limbs; found by the model (test_fe_asm_host.py searches again and compares) and
# recorded in the comment above fe_sqda_sq in fe25519.h
SQDA_A_MAX_256, SQDA_FB_MAX_256 = 2047, 915
# ... where the sum 2 f^2 + a is formed limb by limb and carried by fe_carry (every other build), a is held to 7.4 - 2: fe_carry is
# tested up to 7.4 (test_hostcheck.py)
SQDA_A_MAX_CARRY = 5.4


def mul_cases():
    """(f, g) for fe_mul: the budget's size pairs and the range kernel's own, every kind."""
    import random
    r = random.Random(11)
    return [(operand(pa, k, r), operand(pb, k, r)) for pa, pb in pairs + range_kernel_pairs for k in KINDS]


def sq_cases():
    import random
    r = random.Random(12)
    return [(operand(phi, k, r),) for phi in (1, 2, 3, 3.5) for k in KINDS]


def mul2_cases():
    """(f, g, fb, gb) for fe_mul2: the two halves take different size pairs AND different kinds, so a register that the two
    interleaved streams share by mistake changes a result."""
    import random
    r = random.Random(13)
    sizes = pairs + range_kernel_pairs
    out = []
    for i, (pa, pb) in enumerate(sizes):
        qa, qb = sizes[(i + 5) % len(sizes)]
        for ka, kb in (("max", "alt"), ("alt", "max"), ("rnd", "max"), ("alt", "rnd")):
            out.append((operand(pa, ka, r), operand(pb, ka, r), operand(qa, kb, r), operand(qb, kb, r)))
    return out


def sq2_cases():
    import random
    r = random.Random(14)
    phis = (1, 2, 3, 3.5)
    return [(operand(pa, ka, r), operand(pb, kb, r)) for pa in phis for pb in phis for ka, kb in (("max", "alt"), ("alt", "max"), ("rnd", "max"), ("alt", "rnd"))]


def sqda_cases(a_sizes=(2, SQDA_A_MAX_256 / 256), fb_sizes=(1, 2, 3, 3.5, SQDA_FB_MAX_256 / 256)):
    """(f, a, fb) for fe_sqda_sq: f at tight_max (and below it), a at tight_max and at each of a_sizes, fb at each of fb_sizes."""
    import random
    r = random.Random(15)
    fs = [list(tight_max), operand(1, "alt", r), operand(1, "rnd", r)]
    as_ = [list(tight_max)] + [operand(phi, k, r) for phi in a_sizes for k in ("max", "alt", "rnd")]
    out = []
    for i, f in enumerate(fs):
        for j, a in enumerate(as_):
            for n, phi in enumerate(fb_sizes):
                out.append((f, a, operand(phi, ("alt", "max", "rnd")[(i + j + n) % 3], r)))
    return out


def carry_cases():
    import random
    r = random.Random(16)
    return [operand(phi, k, r) for phi in (1, 2, 5, 6, 7.4) for k in ("max", "alt", "rnd")]


# the limb-wise offsets of fe_sub / fe_neg (2p), fe_sub3 (3p), fe_sub4 (4p): k * (2^w - 1), less 18 k in limb 0
def offset(k):
    return [k * ((1 << w) - 1 - (18 if i == 0 else 0)) for i, w in enumerate(WID)]


def sub_cases(k):
    """(f, g) for the subtraction with offset k p: the subtrahend g equal to the offset limb-wise, zero, and random below the
    offset (never above it: fe_limb_sub's rule), f at sizes 1 and 4."""
    import random
    r = random.Random(17 + k)
    off = offset(k)
    gs = [list(off), [0] * 9] + [[r.randrange(0, o + 1) for o in off] for _ in range(4)] + [[o - (i % 2) for i, o in enumerate(off)], [o if i % 3 else 0 for i, o in enumerate(off)]]
    return [(operand(phi, kind, r), g) for g in gs for phi in (1, 4) for kind in ("max", "rnd")]
