"""The generated device code of the field products (csrc/fe25519_gen.inc), executed by a CPU model (tests/fe_asm_model.py) at the
limb budget.  The host build that test_hostcheck.py drives compiles the #else branch of that file and none of the one-statement
products; the device branches are otherwise reached only through whole protocol runs, whose limbs sit at typical sizes.

  * the five ACT_FE_*_ONE_ASM statements (the range kernel's translation unit runs them and nothing else does): raw limbs against
    big integers mod p, every output limb tight, no column past 2^64, every fixed register written before it is read and on the
    clobber list -- on operands at the top of their size classes, the two halves of a pair statement of different kinds;
  * fe_sqda_sq's preconditions on `a` and `fb`, searched by the model and held against what fe25519.h records;
  * every per-column helper act_cz* / act_c*: the device branch's template against the host branch's C expression;
  * a self-check: edits of the text that the model or its comparison must reject.
No GPU and no build: the model reads the source."""
import os
import random
import re

import pytest

import fe_asm_model as am
import fe_budget_cases as fc
from fe_budget_cases import P, tight_max, val

TEXT = am.source()


def tight(limbs):
    return all(l <= t for l, t in zip(limbs, tight_max))


def check(text, name, want, **operands):
    """Run macro `name` of `text`; want = {result variable: value mod p}.  Raises (ModelError, AssertionError) when anything is off."""
    rep = am.run_macro(text, name, **operands)
    assert set(rep.results) == set(want), (name, sorted(rep.results))
    for k, w in want.items():
        assert val(rep.results[k]) % P == w % P, (name, k, operands, rep.results[k])
        assert tight(rep.results[k]), (name, k, operands, rep.results[k])
    assert rep.max_column < 1 << 64 and not rep.wraps
    return rep


def check_mul(text, f, g):
    return check(text, "ACT_FE_MUL_ONE_ASM", {"h": val(f) * val(g)}, f=f, g=g)


def check_sq(text, f):
    return check(text, "ACT_FE_SQ_ONE_ASM", {"h": val(f) ** 2}, f=f)


def check_mul2(text, f, g, fb, gb):
    return check(text, "ACT_FE_MUL2_ONE_ASM", {"h": val(f) * val(g), "hb": val(fb) * val(gb)}, f=f, g=g, fb=fb, gb=gb)


def check_sq2(text, f, fb):
    return check(text, "ACT_FE_SQ2_ONE_ASM", {"h": val(f) ** 2, "hb": val(fb) ** 2}, f=f, fb=fb)


def check_sqda(text, f, a, fb):
    return check(text, "ACT_FE_SQDA_SQ_ONE_ASM", {"h": 2 * val(f) ** 2 + val(a), "hb": val(fb) ** 2}, f=f, a=a, fb=fb)


CHECKS = {"ACT_FE_MUL_ONE_ASM": (check_mul, fc.mul_cases), "ACT_FE_SQ_ONE_ASM": (check_sq, fc.sq_cases), "ACT_FE_MUL2_ONE_ASM": (check_mul2, fc.mul2_cases),
          "ACT_FE_SQ2_ONE_ASM": (check_sq2, fc.sq2_cases), "ACT_FE_SQDA_SQ_ONE_ASM": (check_sqda, fc.sqda_cases)}


def check_all(text, name):
    fn, cases = CHECKS[name]
    reps = [fn(text, *c) for c in cases()]
    return max(r.max_column for r in reps), reps[0].instructions


@pytest.mark.parametrize("name", am.ONE_ASM_MACROS)
def test_one_statement_product_at_the_limb_budget(name):
    """Right value, tight limbs, no overflow, clean register use -- on every case of the list, which holds operands with EVERY limb at
    the top of its class (the budget's size pairs, the range kernel's own 3 x 4, 4 x 3, 3 x 3, 2 x 3, 3 x 2) and, for the pair
    statements, halves of different kinds."""
    col, n = check_all(TEXT, name)
    print("%s: %d instructions, largest column 2^%.3f" % (name, n, __import__("math").log2(col)))
    assert 85 <= n <= 250 and col >= 1 << 63, (n, col)      # the cases do reach the top bit of a column


def test_pair_cases_give_the_halves_different_operands():
    for f, g, fb, gb in fc.mul2_cases():
        assert f != fb and g != gb
    for f, fb in fc.sq2_cases():
        assert f != fb


def _sqda_ok(a256, fb256):
    try:
        for kind in ("max", "alt"):
            check_sqda(TEXT, list(tight_max), fc.operand(a256 / 256, kind, None), fc.operand(fb256 / 256, kind, None))
        return True
    except (am.ModelError, AssertionError):
        return False


def test_sqda_sq_preconditions_are_the_recorded_ones():
    """With f at tight_max: the largest size of fb, then of a beside it (in 1/256; an element stays below 8 in any case), that the
    statement takes.  fe_budget_cases.py holds the two numbers for the case lists, fe25519.h records them above fe_sqda_sq."""
    def largest(ok):
        lo, hi = 256, 8 * 256            # ok(lo), not ok(hi): 8 is not a size an element has
        assert ok(lo)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if ok(mid) else (lo, mid)
        return lo
    fb_max = largest(lambda k: _sqda_ok(256, k))
    a_max = largest(lambda k: k < 8 * 256 and _sqda_ok(k, fb_max))
    print("fe_sqda_sq with f tight: a up to %d/256 = %.4f, fb up to %d/256 = %.4f" % (a_max, a_max / 256, fb_max, fb_max / 256))
    assert (a_max, fb_max) == (fc.SQDA_A_MAX_256, fc.SQDA_FB_MAX_256)
    assert all(_sqda_ok(a, fb_max) for a in range(256, a_max + 1, 64)) and all(_sqda_ok(a_max, k) for k in range(256, fb_max + 1, 16))      # and everything below
    assert not _sqda_ok(a_max, fb_max + 1)
    hdr = open(os.path.join(os.path.dirname(am.GEN_INC), "fe25519.h")).read()
    m = re.search(r"^// r = 2 f\^2 \+ a carried ONCE.*?^ACT_HD void fe_sqda_sq", hdr, re.S | re.M)
    assert m and "phi(a) <= %d/256" % a_max in m.group(0) and "phi(fb) <= %d/256" % fb_max in m.group(0), m and m.group(0)


# ---- per-column helpers: the device branch against the host branch ---------------------------------------------------------------
def helper_inputs(h, r):
    """Column-sized arguments: 29- and 30-bit limbs (a 28-bit limb doubled, a loose limb), the first argument of a helper that starts
    from a carry up to 32 bits ((uint32_t)(h >> 32), (uint32_t)h), the accumulator up to the 36 bits that l >> 28 leaves."""
    n = len(h.params) - 1
    top = [[(1 << 30) - 1] * n, [(1 << 29) - 1] * n, [((1 << 30) - 1) if i % 2 else (1 << 29) for i in range(n)]]
    rnd = [[r.randrange(1 << 28, 1 << 30) for _ in range(n)] for _ in range(6)]
    out = []
    for args in top + rnd:
        for x0 in (args[0], (1 << 32) - 1, r.randrange(1 << 31, 1 << 32)):
            for acc in (0, (1 << 36) - 1, r.randrange(1 << 35, 1 << 36)):
                out.append((acc, [x0] + args[1:]))
    return out


def compare_helpers(text):
    dev, host = am.helpers(text)
    assert set(dev) == set(host), set(dev) ^ set(host)
    assert len(dev) >= 20
    r = random.Random(21)
    for name in sorted(dev):
        assert [t for t, _ in dev[name].params] == [t for t, _ in host[name].params], name
        for acc, args in helper_inputs(dev[name], r):
            d = am.run_helper(dev[name], acc, args)
            assert d.results["acc"] == am.eval_host_helper(host[name], acc, args), (name, acc, args)
            assert d.instructions == (len(args) + 1) // 2, name


def test_every_per_column_helper_agrees_with_its_host_twin():
    compare_helpers(TEXT)


# ---- the self-check --------------------------------------------------------------------------------------------------------------
def in_macro(text, name, edit):
    """`text` with `edit` applied to the body of macro `name` only; the edit must change something."""
    m = re.search(r"^#define %s \\\n(?:.*\\\n)*.*\n" % name, text, re.M)
    body = edit(m.group(0))
    assert body != m.group(0), (name, "the edit found nothing to change")
    return text[:m.start()] + body + text[m.end():]


def rejected(text, name):
    try:
        check_all(text, name)
    except (am.ModelError, AssertionError):
        return True
    return False


def nth(pattern, repl, n):
    """An edit: the n-th match of `pattern` replaced."""
    def edit(body):
        ms = list(re.finditer(pattern, body))
        if len(ms) <= n:
            return body
        return body[:ms[n].start()] + ms[n].expand(repl) + body[ms[n].end():]
    return edit


PAIR_MACROS = ("ACT_FE_MUL2_ONE_ASM", "ACT_FE_SQ2_ONE_ASM", "ACT_FE_SQDA_SQ_ONE_ASM")
EDITS = {
    "a carry shift of 28 becomes 29": [nth(r"(v_lshrrev_b64 v\[\d+:\d+\]), 28,", r"\1, 29,", k) for k in (0, 3)],
    "the top column's shift of 28 becomes 29": [nth(r"(v_alignbit_b32 v\d+, v\d+, v\d+), 28", r"\1, 29", 0), nth(r"(v_lshrrev_b32 v\d+), 28,", r"\1, 29,", 0)],
    "the last carry's shift of 29 becomes 28": [nth(r"(v_alignbit_b32 v\d+, v\d+, v\d+), 29", r"\1, 28", 0)],
    "a fold by 19 becomes one by 18": [nth(r"(v_mad_u64_u32 v\[\d+:\d+\], vcc, v\d+), 19,", r"\1, 18,", k) for k in (0, 5)] + [nth(r"(v_mul_u32_u24 v\d+), 19,", r"\1, 18,", 0)],
    "304 becomes 303": [nth(r'"s"\(304u\)', '"s"(303u)', 0)],
    "a register leaves the clobber list": [nth(r'"v250", ', "", 0), nth(r'"v254", ', "", 0)],
    "vcc leaves the clobber list": [nth(r', "vcc"\)', ")", 0)],
    "a multiply-accumulate is deleted": [nth(r' *"v_mad_u64_u32 [^\n]*%\[[^\n]*\n', "", k) for k in (0, 17, 40)],
}
# (fe_sqda_sq's two streams end one after the other, not interleaved: there a shared temporary of the tail would be harmless)
INTERLEAVED_TAIL_EDITS = {"the two streams share a temporary": [lambda b: b.replace("v242", "v254"), lambda b: b.replace("v241", "v253")]}
PAIR_EDITS = {
    "the two streams share an accumulator": [lambda b: b.replace("v[238:239]", "v[250:251]").replace("v238", "v250").replace("v239", "v251")],
    "a register of the second stream leaves the clobber list": [nth(r'"v236", ', "", 0)],
}


@pytest.mark.parametrize("name", am.ONE_ASM_MACROS)
def test_the_model_rejects_edited_statements(name):
    assert not rejected(TEXT, name)
    edits = dict(EDITS, **(PAIR_EDITS if name in PAIR_MACROS else {}), **(INTERLEAVED_TAIL_EDITS if name in PAIR_MACROS[:2] else {}))
    for what, es in edits.items():
        for k, e in enumerate(es):
            assert rejected(in_macro(TEXT, name, e), name), (name, what, k, "was accepted")


def test_the_model_rejects_edited_helpers():
    """The same for the per-column helpers: an edit of the device branch alone no longer agrees with the host branch."""
    m = re.search(r"^#if defined\(__HIP_DEVICE_COMPILE__\)\n.*?^#else\n", TEXT, re.S | re.M)
    for what, pat, repl in (("a fold by 19 becomes 18", r"(act_c9_i19at0\(.*?v_mad_u64_u32 %0, vcc, %1), 19,", r"\1, 18,"),
                            ("a factor of 16 becomes 8", r"(act_cz7_i16at0\(.*?v_mad_u64_u32 %0, vcc, %1), 16,", r"\1, 8,"),
                            ("a term is dropped", r"(act_cz8\(.*?)v_mad_u64_u32 %0, vcc, %15, %16, %0", r"\1v_mad_u64_u32 %0, vcc, %13, %14, %0"),
                            ("operands change places", r"(act_c4_i19at0\(.*?)%4, %5, %0", r"\1%4, %3, %0"),
                            ("the carry is forgotten", r"(act_c10_sat0\(.*?v_mad_u64_u32 %0, vcc, %1, %2), %0", r"\1, 0"),
                            ("a helper goes missing on the device", r"static __device__ __forceinline__ void act_cz4\([^\n]*\n", "")):
        dev = re.sub(pat, repl, m.group(0), count=1, flags=re.S)
        assert dev != m.group(0), what
        with pytest.raises((am.ModelError, AssertionError)):
            compare_helpers(TEXT[:m.start()] + dev + TEXT[m.end():])


def test_the_model_does_not_guess():
    with pytest.raises(am.ModelError, match="v_mul_hi_u32"):
        am.run_macro(in_macro(TEXT, "ACT_FE_SQ_ONE_ASM", nth(r"v_and_b32 v252", "v_mul_hi_u32 v252", 0)), "ACT_FE_SQ_ONE_ASM", f=list(tight_max))
    with pytest.raises(am.ModelError, match="before this statement wrote it"):
        am.run_macro(in_macro(TEXT, "ACT_FE_SQ_ONE_ASM", nth(r' *"v_mad_u64_u32 v\[244:245\], vcc, %\[f1_2\], %\[f8_2\], 0[^\n]*\n', "", 0)), "ACT_FE_SQ_ONE_ASM", f=list(tight_max))
    with pytest.raises(am.ModelError, match="overflows 2\\^64"):
        am.run_macro(TEXT, "ACT_FE_MUL_ONE_ASM", f=fc.operand(4, "max", None), g=fc.operand(4, "max", None))
    with pytest.raises(am.ModelError, match="wraps 32 bits"):
        am.run_macro(TEXT, "ACT_FE_SQ_ONE_ASM", f=fc.operand(4.1, "max", None))
    with pytest.raises(am.ModelError, match="no inline constant"):
        am.run_macro(in_macro(TEXT, "ACT_FE_MUL_ONE_ASM", nth(r"%\[c304\]", "304", 0)), "ACT_FE_MUL_ONE_ASM", f=list(tight_max), g=list(tight_max))


def test_the_model_and_the_host_build_return_the_same_limbs(hostcheck):
    """fe_mul / fe_sq: the one-statement form (model) and the per-column form (host build) carry alike, so their raw limbs agree --
    which ties the model to code the host tests own."""
    import ctypes as C
    arr = lambda x: (C.c_uint32 * 9)(*x)
    for f, g in fc.mul_cases():
        lo = (C.c_uint32 * 9)()
        hostcheck.hc_fe_mul_out_limbs(arr(f), arr(g), lo)
        assert list(lo) == am.run_macro(TEXT, "ACT_FE_MUL_ONE_ASM", f=f, g=g).results["h"], (f, g)
    for f, in fc.sq_cases():
        lo = (C.c_uint32 * 9)()
        hostcheck.hc_fe_sq_out_limbs(arr(f), lo)
        assert list(lo) == am.run_macro(TEXT, "ACT_FE_SQ_ONE_ASM", f=f).results["h"], f
