"""Operands at the edges of the scalar arithmetic mod l (csrc/sc25519.h), one seeded and deterministic list per operation, shared by
the host test (test_sc_edges_host.py: model, host build, rejected edits) and the device test (test_gpu_sc_edges.py).  All values are
Python integers; the lists aim at 2^252 and l, at word and limb boundaries, at every number of final subtractions the fold of
sc_reduce512 can take, and at the lazy bound (operands below 2 l) of the Montgomery product.  The searches below look at the MODEL
(tests/sc_model.py) to decide which cases to keep, never at the code under test."""
import functools
import json
import os
import random

import sc_model as sm
from sc_model import C, ELL

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sodium_primitives.json")
MIN_PER_COUNT = 8                  # cases per reachable number of final subtractions (1, 2, 3)


@functools.lru_cache(maxsize=None)
def sodium():
    with open(GOLDEN) as f:
        g = json.load(f)
    return {k: g[k] for k in ("sc_ring", "sc_reduce32", "sc_reduce_wide")}


def le_int(hexstr):
    return int.from_bytes(bytes.fromhex(hexstr), "little")


@functools.lru_cache(maxsize=None)
def wide_cases():
    """512-bit inputs of sc_reduce512 (LOAD_WIDE)."""
    r = random.Random(2521)
    top = (2**512 - 1) // ELL * ELL                     # the largest multiple of l below 2^512
    xs = [0, 1, ELL - 1, ELL, ELL + 1, 2 * ELL - 1, 2 * ELL + 1, 2**252 - 1, 2**252, 2**252 + 1, 2**256 - 1, 2**256, 2**512 - 1]
    xs += [2**k for k in range(512)] + [2**k - 1 for k in range(1, 513)]
    xs += [k * ELL + d for k in range(1, 41) for d in (-1, 0, 1)]
    xs += [top - 1, top, top + 1, (ELL - 1) ** 2, (ELL - 1) ** 2 + (ELL - 1)]
    # (h0 << 252) + lo0: the fold's A - B is lo0 + 2 l + lo2 - lo1 - y3, so the two ends of lo0 steer the number of subtractions
    for h0 in [1, 2**130, 2**259, 2**260 - 1] + [r.getrandbits(260) for _ in range(28)]:
        xs += [(h0 << 252) + lo0 for lo0 in (0, 2**252 - 1)]
    xs += [r.getrandbits(512) for _ in range(64)]
    return tuple(xs)


@functools.lru_cache(maxsize=None)
def scalar_list():
    """The operands of add, sub, neg and half (all canonical): 0, 1, 2, the top of the range, the halves, 2^252 - 1, c = l - 2^252
    and its neighbours, a set bit and a run of ones at every word boundary, and runs of ones below a high bit (a carry or a borrow
    that starts at word 0 runs through w words)."""
    xs = [0, 1, 2, ELL - 1, ELL - 2, (ELL - 1) // 2, (ELL + 1) // 2, 2**252 - 1, C, C - 1, C + 1]
    xs += [2 ** (32 * w) for w in range(1, 8)] + [2 ** (32 * w) - 1 for w in range(1, 8)]
    xs += [2**248 + 2 ** (32 * w) - 1 for w in range(1, 8)]
    assert all(0 <= x < ELL for x in xs) and len(set(xs)) == len(xs)
    return tuple(xs)


@functools.lru_cache(maxsize=None)
def pair_cases():
    """(a, b) for sc_add and sc_sub: all ordered pairs of scalar_list()."""
    return tuple((a, b) for a in scalar_list() for b in scalar_list())


@functools.lru_cache(maxsize=None)
def half_cases():
    """a for sc_half and sc_neg: scalar_list() (odd and even), and its members' neighbours of the other parity."""
    xs = list(scalar_list()) + [x ^ 1 for x in scalar_list() if x ^ 1 < ELL and x ^ 1 not in scalar_list()]
    return tuple(xs)


@functools.lru_cache(maxsize=None)
def aimed_products():
    """{number of final subtractions: [(a, b), ...]} with a, b < l, MIN_PER_COUNT pairs for each of 1, 2 and 3: a seeded search on the
    model.  Random products take three subtractions about once in 1 400 draws."""
    r = random.Random(2522)
    found = {1: [], 2: [], 3: []}
    draws = 0
    while any(len(v) < MIN_PER_COUNT for v in found.values()):
        a, b = r.randrange(ELL), r.randrange(ELL)
        draws += 1
        assert draws < 200000, "the search for aimed products does not end"
        k = sm.mul(a, b).subs
        if len(found[k]) < MIN_PER_COUNT:
            found[k].append((a, b))
    return found


@functools.lru_cache(maxsize=None)
def random_products():
    r = random.Random(2523)
    return tuple((r.randrange(ELL), r.randrange(ELL)) for _ in range(64))


@functools.lru_cache(maxsize=None)
def mul_cases():
    """(a, b) for sc_mul: the pairs of the add / sub list, the aimed pairs (1, 2, 3 final subtractions), 64 random pairs."""
    return pair_cases() + tuple(p for k in (1, 2, 3) for p in aimed_products()[k]) + random_products()


@functools.lru_cache(maxsize=None)
def muladd_cases():
    """(a, b, c) for sc_muladd: the aimed and the random products and a slice of the named pairs, each with addends that put
    sc_add's sum at l - 1 (nothing subtracted), at l (subtracted, result 0) and at the far ends."""
    prods = tuple(p for k in (1, 2, 3) for p in aimed_products()[k]) + random_products() + pair_cases()[::37]
    out = []
    for a, b in prods:
        p = a * b % ELL
        out += [(a, b, c % ELL) for c in (ELL - 1 - p, ELL - p, 0, ELL - 1)]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def reduce32_cases():
    """256-bit inputs of sc_from_words (LOAD_SC): for every top nibble q the values of lo on both sides of q c (where the conditional
    subtraction flips) and at both ends, the multiples of l below 2^256 and their neighbours, 2^256 - 1."""
    xs = []
    for q in range(16):
        xs += [(q << 252) + lo for lo in (0, q * C - 1, q * C, q * C + 1, 2**252 - 1) if lo >= 0]
    xs += [k * ELL + d for k in range(1, 16) for d in (-1, 0, 1)] + [2**256 - 1]
    assert all(0 <= x < 2**256 for x in xs)
    return tuple(xs)


@functools.lru_cache(maxsize=None)
def invert_cases():
    """a < l for sc_invert: small and large values, every power of two, one 26-bit limb of the Montgomery form all ones at each of its
    ten positions (the top limb: the 18 bits a value below 2^252 has there), one 32-bit word all ones at each of the eight positions
    (reduced mod l), every a of libsodium's sc_ring records, 64 random values."""
    r = random.Random(2524)
    xs = [0, 1, 2, 3, ELL - 1, ELL - 2, (ELL + 1) // 2]
    xs += [2**k for k in range(253)]
    xs += [((1 << min(26, 252 - 26 * i)) - 1) << (26 * i) for i in range(10)]
    xs += [(0xffffffff << (32 * w)) % ELL for w in range(8)]
    xs += [le_int(v["a"]) for v in sodium()["sc_ring"]]
    xs += [r.randrange(ELL) for _ in range(64)]
    assert all(0 <= x < ELL for x in xs)
    return tuple(xs)


@functools.lru_cache(maxsize=None)
def scm_named():
    """Values below 2 l for scm_mul: 0, 1, around l, the top of the lazy range, R and R^2 mod l, and nine low limbs at 2^26 - 1 under
    the largest top limb that keeps the value below 2 l."""
    full = (((2 * ELL) >> 234) - 1 << 234) + 2**234 - 1
    xs = [0, 1, ELL - 1, ELL, ELL + 1, 2 * ELL - 1, sm.R % ELL, sm.R * sm.R % ELL, full]
    assert all(0 <= x < 2 * ELL for x in xs) and sm.val_limbs(full)[:9] == [sm.SCM_MASK] * 9 and full + 2**234 >= 2 * ELL
    return tuple(xs)


@functools.lru_cache(maxsize=None)
def scm_cases():
    """(a, b) as values below 2 l (ten 26-bit limbs each: sc_model.val_limbs): all pairs of scm_named(), 64 random operands with each
    other and with the named ones."""
    r = random.Random(2525)
    rnd = [r.randrange(2 * ELL) for _ in range(64)]
    named = scm_named()
    out = [(a, b) for a in named for b in named]
    out += [(rnd[i], rnd[(i + 1) % 64]) for i in range(64)]
    out += [(rnd[i], named[i % len(named)]) if i % 2 else (named[i % len(named)], rnd[i]) for i in range(64)]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def equal_cases():
    """(a, b) for sc_equal: equal pairs, and pairs that differ in exactly one bit, the lowest and the highest of every word."""
    base = list(scalar_list()) + [2**256 - 1]
    out = [(a, a) for a in base]
    for i, a in enumerate(base):
        for w in range(8):
            out.append((a, a ^ (1 << (32 * w + (31 if (i + w) % 2 else 0)))))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def is_zero_cases():
    """a for sc_is_zero: 0, one bit at either end of every word, l, 2^256 - 1, the add / sub list."""
    return (0,) + tuple(1 << (32 * w + b) for w in range(8) for b in (0, 31)) + (ELL, 2**256 - 1) + scalar_list()


# ---- the lists by operation, and what the model returns for them ---------------------------------------------------------------------
OPS = ("load_wide", "load_sc", "add", "sub", "neg", "half", "mul", "muladd", "invert", "scm_mul", "equal", "is_zero")


@functools.lru_cache(maxsize=None)
def cases(op):
    """Operand tuples (integers) of an operation, in the order of the hook's arrays."""
    one = lambda xs: tuple((x,) for x in xs)
    return {"load_wide": lambda: one(wide_cases()), "load_sc": lambda: one(reduce32_cases()), "add": pair_cases, "sub": pair_cases,
            "neg": lambda: one(half_cases()), "half": lambda: one(half_cases()), "mul": mul_cases, "muladd": muladd_cases,
            "invert": lambda: one(invert_cases()), "scm_mul": scm_cases, "equal": equal_cases, "is_zero": lambda: one(is_zero_cases())}[op]()


@functools.lru_cache(maxsize=None)
def model(op):
    """What the model returns for every case of the operation: a list of (result, detail).  result: an integer, for scm_mul the ten
    limbs.  detail: the Fold, the subtraction count or None.  Computed once; the device test reads it too."""
    out = []
    for c in cases(op):
        if op == "load_wide":
            f = sm.reduce512(*c); out.append((f.r, f))
        elif op == "load_sc":
            out.append(sm.from_words(*c))
        elif op in ("add", "sub", "neg"):
            out.append(getattr(sm, op)(*c))
        elif op == "half":
            out.append((sm.half(*c), None))
        elif op == "mul":
            f = sm.mul(*c); out.append((f.r, f))
        elif op == "muladd":
            r, f, taken = sm.muladd(*c); out.append((r, (f, taken)))
        elif op == "invert":
            v = sm.invert(*c); out.append((v.r, v))
        elif op == "scm_mul":
            out.append((sm.scm_mul(sm.val_limbs(c[0]), sm.val_limbs(c[1])), None))
        elif op == "equal":
            out.append((int(c[0] == c[1]), None))
        else:
            out.append((int(c[0] == 0), None))
    return out


def ragged(cases, chunk=512, block=256):
    """The list repeated from its start until it is longer than a chunk of the test's context and no whole number of blocks: a call
    then crosses a chunk boundary and ends in a ragged block."""
    out = list(cases)
    i = 0
    while len(out) <= chunk or len(out) % block == 0:
        out.append(cases[i % len(cases)])
        i += 1
    return out
