"""The device forms of the field arithmetic (csrc/fe25519.h, fe25519_gen.inc) on the GPU, one operation per lane on raw limbs
(act_debug_fe_batch, csrc/k_debug_fe.hip), at the top of the limb-size classes -- in BOTH builds of the field code: the per-column
form every kernel but one runs (act_cz* / act_c* asm helpers, fe_limb_sub's v_sad_u32) and the one-statement form of the range
kernel's translation unit (ACT_FE_*_ONE_ASM on v232..v254).  Protocol runs reach these with limbs of typical size only.

Expected values never come from the code under test: big integers mod p; limb for limb the CPU model of the generated code
(tests/fe_asm_model.py: the hardware thereby checks the model) for the one-statement products; limb for limb the host build
(tests/hostcheck) for the per-column products and, in both builds, for fe_carry, fe_sub, fe_sub3, fe_sub4 and fe_neg.  The case
lists are those of tests/test_fe_asm_host.py (tests/fe_budget_cases.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

import fe_asm_model as am
import fe_budget_cases as fc
from fe_budget_cases import P, tight_max, val

pytestmark = pytest.mark.gpu

L_SMALL, MAX_BATCH = 8, 512
FILL = 0xA5A5A5A5
BUILDS = [pytest.param(0, id="per-column"), pytest.param(1, id="pair")]
PRODUCTS = ("mul", "sq", "mul2", "sq2", "sqda_sq")
MACRO = {"mul": "ACT_FE_MUL_ONE_ASM", "sq": "ACT_FE_SQ_ONE_ASM", "mul2": "ACT_FE_MUL2_ONE_ASM", "sq2": "ACT_FE_SQ2_ONE_ASM", "sqda_sq": "ACT_FE_SQDA_SQ_ONE_ASM"}
SUB_K = {"sub": 2, "sub3": 3, "sub4": 4}


@pytest.fixture(scope="module")
def eng(oracle):
    from act_amd import capi
    e = capi.Engine(oracle.params_new("fe-forms", "svc", "env", "v1"), L_SMALL, max_batch=MAX_BATCH)
    try:
        yield e
    finally:
        e.close()


@functools.lru_cache(maxsize=None)
def cases(op, pair):
    """Operand tuples in the order (f, g, fb, gb_or_a) of the entry point (None where the operation names none)."""
    if op == "mul":
        return [(f, g, None, None) for f, g in fc.mul_cases()]
    if op == "sq":
        return [(f, None, None, None) for f, in fc.sq_cases()]
    if op == "mul2":
        return [(f, g, fb, gb) for f, g, fb, gb in fc.mul2_cases()]
    if op == "sq2":
        return [(f, None, fb, None) for f, fb in fc.sq2_cases()]
    if op == "sqda_sq":
        # the one-statement form at the sizes the model found for it; the other form at what its carry pass and squaring take
        cs = fc.sqda_cases() if pair else fc.sqda_cases(a_sizes=(2, fc.SQDA_A_MAX_CARRY), fb_sizes=(1, 2, 3, 3.5))
        return [(f, None, fb, a) for f, a, fb in cs]
    if op == "carry":
        return [(f, None, None, None) for f in fc.carry_cases()]
    if op in SUB_K:
        return [(f, g, None, None) for f, g in fc.sub_cases(SUB_K[op])]
    if op == "neg":
        return [(g, None, None, None) for _, g in fc.sub_cases(2)]
    raise KeyError(op)


def big_integer_values(op, c):
    """(value of h, value of hb or None); for the subtractions the exact integer, for the rest a value mod p."""
    f, g, fb, ga = (None if x is None else val(x) for x in c)
    if op in SUB_K:
        return f - g + val(fc.offset(SUB_K[op])), None
    if op == "neg":
        return val(fc.offset(2)) - f, None
    if op == "mul":
        return f * g, None
    if op == "mul2":
        return f * g, fb * ga
    if op == "sq2":
        return f * f, fb * fb
    if op == "sqda_sq":
        return 2 * f * f + ga, fb * fb
    return {"sq": f * f, "carry": f}[op], None


@functools.lru_cache(maxsize=None)
def model_limbs(op):
    """What the one-statement form must return, limb for limb: the CPU model of csrc/fe25519_gen.inc."""
    text = am.source()
    out = []
    for f, g, fb, ga in cases(op, 1):
        kw = {"f": f}
        if g is not None:
            kw["g"] = g
        if fb is not None:
            kw["fb"] = fb
        if ga is not None:
            kw["a" if op == "sqda_sq" else "gb"] = ga
        r = am.run_macro(text, MACRO[op], **kw).results
        out.append((r["h"], r.get("hb")))
    return out


def host_limbs(hc, op, c):
    """What the per-column form (and either build's fe_carry / fe_sub* / fe_neg) must return: the host build of the same headers."""
    arr = lambda x: (C.c_uint32 * 9)(*x)
    f, g, fb, ga = c
    h, hb, out = (C.c_uint32 * 9)(), (C.c_uint32 * 9)(), C.create_string_buffer(32)
    if op == "mul":
        hc.hc_fe_mul_out_limbs(arr(f), arr(g), h)
    elif op == "sq":
        hc.hc_fe_sq_out_limbs(arr(f), h)
    elif op == "mul2":
        hc.hc_fe_mul_out_limbs(arr(f), arr(g), h); hc.hc_fe_mul_out_limbs(arr(fb), arr(ga), hb)
    elif op == "sq2":
        hc.hc_fe_sq_out_limbs(arr(f), h); hc.hc_fe_sq_out_limbs(arr(fb), hb)
    elif op == "sqda_sq":
        hc.hc_fe_sqda_sq_out_limbs(arr(f), arr(ga), arr(fb), h, hb)
    elif op == "carry":
        hc.hc_fe_carry_limbs(arr(f), h, out)
    elif op in SUB_K:
        assert hc.hc_fe_sub_out_limbs(SUB_K[op], arr(f), arr(g), h) == 1
    else:
        hc.hc_fe_neg_out_limbs(arr(f), h)
    return list(h), (list(hb) if op in ("mul2", "sq2", "sqda_sq") else None)


def run(eng, pair, op, cs):
    n = len(cs)
    cols = [None if cs[0][k] is None else np.array([c[k] for c in cs], np.uint32).reshape(-1) for k in range(4)]
    h, hb = eng.debug_fe(pair, op, n, *cols, fill=FILL)
    lanes = (n + 255) // 256 * 256
    assert h.size == 9 * lanes and (hb is None or hb.size == 9 * lanes)
    # lanes from n on: the buffer went to the device and back, and the kernel's guard left them alone
    assert (h[9 * n:] == FILL).all() and (hb is None or (hb[9 * n:] == FILL).all()), (op, pair, n)
    got = lambda a, i: [int(x) for x in a[9 * i:9 * i + 9]]
    return [(got(h, i), None if hb is None else got(hb, i)) for i in range(n)]


def check_lane(hc, pair, op, c, got, model):
    for name, g, want in zip(("h", "hb"), got, big_integer_values(op, c)):
        if want is None:
            assert g is None
            continue
        if op in SUB_K or op == "neg":
            assert val(g) == want, (op, pair, name, c, g)                 # no limb wrapped: the exact integer f - g + k p
        assert val(g) % P == want % P, (op, pair, name, c, g)
        if op in PRODUCTS or op == "carry":
            assert all(l <= t for l, t in zip(g, tight_max)), (op, pair, name, c, g)
    if pair and op in PRODUCTS:
        assert got == model, (op, "the device and the model of the one-statement form differ", c, got, model)
    else:
        assert got == host_limbs(hc, op, c), (op, pair, "the device and the host build differ", c, got)


@pytest.mark.parametrize("op", PRODUCTS + ("carry", "sub", "sub3", "sub4", "neg"))
@pytest.mark.parametrize("pair", BUILDS)
def test_field_operation_at_the_limb_budget(eng, hostcheck, pair, op):
    """Every case of the operation's list in one launch: right value, tight limbs where the operation promises them, exact limbs
    against the model (one-statement products) or the host build (everything else)."""
    cs = cases(op, pair)
    models = model_limbs(op) if pair and op in PRODUCTS else [None] * len(cs)
    assert len(cs) % 256 and len(models) == len(cs)
    for c, got, model in zip(cs, run(eng, pair, op, cs), models):
        check_lane(hostcheck, pair, op, c, got, model)


@pytest.mark.parametrize("n", [1, 63, 65, 600])
@pytest.mark.parametrize("pair", BUILDS)
def test_batch_sizes_and_the_lanes_beyond(eng, hostcheck, pair, n):
    """One lane, one short of a wave, one past it, and more than a chunk of the context (two launches, the second a partial block):
    every lane right, every lane from n on as the caller filled it (run() asserts that)."""
    for op in ("mul2", "sub3"):
        base = cases(op, pair)
        cs = [base[(7 * i + n) % len(base)] for i in range(n)]
        models = model_limbs(op) if pair and op in PRODUCTS else None
        for i, (c, got) in enumerate(zip(cs, run(eng, pair, op, cs))):
            check_lane(hostcheck, pair, op, c, got, models[(7 * i + n) % len(base)] if models else None)


def test_arguments_are_checked(eng):
    from act_amd import capi
    f = np.zeros(9, np.uint32)
    with pytest.raises(capi.ActError):
        eng.debug_fe(0, "mul", 1, f)                       # g missing
    with pytest.raises(capi.ActError):
        eng.debug_fe(1, "sqda_sq", 1, f, None, f, None)    # a missing
    h = np.zeros(9 * 256, np.uint32)
    assert eng.lib.act_debug_fe_batch(eng.ctx, 0, len(eng.FE_OPS), 1, f.ctypes.data, None, None, None, h.ctypes.data, None) != 0
    assert eng.lib.act_debug_fe_batch(eng.ctx, 0, -1, 1, f.ctypes.data, None, None, None, h.ctypes.data, None) != 0
