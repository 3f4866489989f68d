"""The scalar arithmetic mod l (csrc/sc25519.h) at its edges, without a GPU: the big-integer model of the header (tests/sc_model.py)
against plain `% ELL` arithmetic on every case list of tests/sc_edge_cases.py, what those lists cover (stated on the model alone),
the host build of the header (tests/hostcheck, raw operands) against the model byte for byte -- scm_mul limb for limb -- and against
libsodium's records, and five wrong versions of the header that the lists must tell from the right one.
tests/test_gpu_sc_edges.py sends the same lists through the device build."""
import ctypes as C
import math
import os
import shutil
import subprocess

import pytest

import sc_edge_cases as ec
import sc_model as sm
from conftest import ROOT
from sc_edge_cases import OPS, cases, model
from sc_model import ELL

le32 = lambda x: x.to_bytes(32, "little")


def plain(op, c):
    """The same operation in plain arithmetic mod l (scm_mul: mod l and below 2 l)."""
    if op in ("load_wide", "load_sc"):
        return c[0] % ELL
    if op == "invert":
        return pow(c[0], ELL - 2, ELL)
    return {"add": lambda a, b: a + b, "sub": lambda a, b: a - b, "neg": lambda a: -a, "half": lambda a: a * (ELL + 1) // 2,
            "mul": lambda a, b: a * b, "muladd": lambda a, b, c_: a * b + c_}[op](*c) % ELL


@pytest.mark.parametrize("op", [o for o in OPS if o not in ("equal", "is_zero")])
def test_model_equals_plain_arithmetic(op):
    """... and raises on no case: every bound the header's comments promise holds on every list."""
    for c, (r, _) in zip(cases(op), model(op)):
        if op == "scm_mul":
            v = sm.limbs_val(r)
            assert v * sm.R % ELL == c[0] * c[1] % ELL and v < 2 * ELL and all(x <= sm.SCM_MASK for x in r), c
            assert v == sm.scm_mul_value(*c), c                    # the value form sc_model.invert runs on
        else:
            assert r == plain(op, c), (op, c)
    if op == "invert":
        # the whole exponentiation limb by limb (every column of its 328 products held to 64 bits) where single limbs and words matter
        for a in ec.invert_cases()[:7] + ec.invert_cases()[7 + 253:7 + 253 + 18]:
            assert sm.invert(a, exact_limbs=True).r == pow(a, ELL - 2, ELL), a


def test_the_lists_cover_what_they_aim_at(capsys):
    wide = [f for _, f in model("load_wide")]
    count = lambda folds: {k: sum(f.subs == k for f in folds) for k in range(5)}
    cw = count(wide)
    assert all(cw[k] >= ec.MIN_PER_COUNT for k in (1, 2, 3)) and cw[0] == cw[4] == 0, cw
    assert max(f.h2 for f in wide) == 27 and wide[ec.wide_cases().index(2**512 - 1)].h2 == 27
    assert any(f.h1 >= 1 << 132 for f in wide)
    assert {0, 1, ELL - 1} <= {f.r for f in wide}
    prods = [f for _, f in model("mul")]
    cp = count(prods)
    assert all(cp[k] >= ec.MIN_PER_COUNT for k in (1, 2, 3)) and cp[0] == cp[4] == 0, cp
    cm = count([f for _, (f, _) in model("muladd")])
    assert all(cm[k] >= ec.MIN_PER_COUNT for k in (1, 2, 3)) and cm[0] == cm[4] == 0, cm
    # sc_from_words: for every top nibble but 0 a case that subtracts l and one that does not (q = 0 always subtracts)
    for q in range(16):
        taken = {t for (x,), (_, t) in zip(cases("load_sc"), model("load_sc")) if x >> 252 == q}
        assert taken == ({1} if q == 0 else {0, 1}), (q, taken)
    # every other conditional subtraction: both outcomes
    for op in ("add", "sub", "neg"):
        assert {t for _, t in model(op)} == {0, 1}, op
    assert {t for _, (_, t) in model("muladd")} == {0, 1}
    assert {r for r, _ in model("equal")} == {0, 1} and {r for r, _ in model("is_zero")} == {0, 1}
    assert {c[0] & 1 for c in cases("half")} == {0, 1}
    # sc_invert's final subtraction: recorded, nothing required of it
    inv = [v for _, v in model("invert")]
    taken = sum(v.subs for v in inv)
    with capsys.disabled():
        print("\nsc_reduce512 final subtractions: wide", cw, "products", cp)
        print("sc_invert: final subtraction taken in %d of %d cases; largest value before it l - %d; largest Montgomery value on the way %.6f l; "
              "largest scm_mul column of this run 2^%.2f" % (taken, len(inv), ELL - max(v.before_sub for v in inv), max(v.peak for v in inv) / ELL, math.log2(max(1, sm.peak_column[0]))))


def host_result(hc, op, c):
    """What the host build of sc25519.h returns on the raw operands: an integer, for scm_mul ten limbs."""
    o = C.create_string_buffer(32)
    if op == "load_wide":
        hc.hc_sc_reduce_wide(c[0].to_bytes(64, "little"), o)
    elif op == "scm_mul":
        arr = lambda v: (C.c_uint32 * 10)(*sm.val_limbs(v))
        out = (C.c_uint32 * 10)()
        hc.hc_scm_mul(arr(c[0]), arr(c[1]), out)
        return list(out)
    elif op == "equal":
        return hc.hc_sc_equal(le32(c[0]), le32(c[1]))
    elif op == "is_zero":
        return hc.hc_sc_is_zero(le32(c[0]))
    else:
        fn = {"load_sc": "hc_sc_from_bytes", "add": "hc_sc_add", "sub": "hc_sc_sub_raw", "neg": "hc_sc_neg_raw", "half": "hc_sc_half_raw", "mul": "hc_sc_mul",
              "muladd": "hc_sc_muladd_raw", "invert": "hc_sc_invert_raw"}[op]
        getattr(hc, fn)(*[le32(x) for x in c], o)
    return int.from_bytes(o.raw, "little")


def mismatches(hc, ops=OPS):
    """{op: indices of the cases on which this build of the header differs from the model}"""
    bad = {}
    for op in ops:
        idx = [i for i, (c, (want, _)) in enumerate(zip(cases(op), model(op))) if host_result(hc, op, c) != want]
        if idx:
            bad[op] = idx
    return bad


def test_host_build_equals_the_model(hostcheck):
    assert mismatches(hostcheck) == {}


def test_host_build_equals_libsodium(hostcheck):
    """Third-party expected values on the raw-operand entries: crypto_core_ristretto255_scalar_* records of libsodium 1.0.18."""
    hc, g = hostcheck, ec.sodium()
    for v in g["sc_reduce32"]:
        assert host_result(hc, "load_sc", (ec.le_int(v["in"]),)) == ec.le_int(v["out"])
    for v in g["sc_reduce_wide"]:
        assert host_result(hc, "load_wide", (ec.le_int(v["in"]),)) == ec.le_int(v["out"])
    for v in g["sc_ring"]:
        a, b = ec.le_int(v["a"]), ec.le_int(v["b"])
        assert a < ELL and b < ELL
        for op, c, key in (("add", (a, b), "add"), ("sub", (a, b), "sub"), ("mul", (a, b), "mul"), ("neg", (a,), "neg_a"), ("invert", (a,), "inv_a")):
            assert host_result(hc, op, c) == ec.le_int(v[key]), (op, v)


# ---- rejected edits: five wrong versions of sc25519.h, built with the host compiler from a copy of the sources ------------------------
MUTANTS = {
    "two final subtractions in sc_reduce512": ("sc_cond_sub_l(A, 4);", "sc_cond_sub_l(A, 2);"),
    "c without its top word in sc_from_words": ("bn_mul<1, 4>(qc, &q, c); ", "c[3] = 0u; bn_mul<1, 4>(qc, &q, c); "),
    "sc_half adds l to even values too": ("(sc_l_word(i) & odd)", "sc_l_word(i)"),
    "sh > 8 in sc_invert's 32 -> 26 conversion": ("if (sh > 6 && w + 1 < 8)", "if (sh > 8 && w + 1 < 8)"),
    "a limb of scm_l off by one": ("0x37a8bdeu, 0x014def9u, 0u, 0u, 0u, 0u, 0x0040000u}", "0x37a8bdfu, 0x014def9u, 0u, 0u, 0u, 0u, 0x0040000u}"),
}


def build_mutants(tmp):
    """One copy of csrc's headers and of hostcheck.cpp per mutant, the edit applied to its sc25519.h, all five compiled at once."""
    csrc = os.path.join(ROOT, "anonymous-credit-tokens_amd", "csrc")
    procs = {}
    for k, (name, (old, new)) in enumerate(MUTANTS.items()):
        d = os.path.join(str(tmp), "m%d" % k)
        os.makedirs(os.path.join(d, "anonymous-credit-tokens_amd", "csrc"))
        os.makedirs(os.path.join(d, "tests", "hostcheck"))
        for f in os.listdir(csrc):
            if f.endswith((".h", ".inc")):
                shutil.copy(os.path.join(csrc, f), os.path.join(d, "anonymous-credit-tokens_amd", "csrc", f))
        src = os.path.join(d, "tests", "hostcheck", "hostcheck.cpp")
        shutil.copy(os.path.join(ROOT, "tests", "hostcheck", "hostcheck.cpp"), src)
        hdr = os.path.join(d, "anonymous-credit-tokens_amd", "csrc", "sc25519.h")
        text = open(hdr).read()
        assert text.count(old) == 1, (name, "the text this edit replaces is no longer in sc25519.h exactly once")
        with open(hdr, "w") as f:
            f.write(text.replace(old, new))
        out = os.path.join(d, "libhostcheck_mutant.so")
        procs[name] = (out, subprocess.Popen(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", out, src]))
    libs = {}
    for name, (out, p) in procs.items():
        assert p.wait() == 0, name
        libs[name] = C.CDLL(out)
    return libs


def test_rejected_edits_fail_a_case(tmp_path, capsys):
    """Each wrong header gives wrong bytes on at least one case of the lists (and the first, the point of the aimed products, on every
    product that takes three subtractions)."""
    libs = build_mutants(tmp_path)
    report = []
    for name, lib in libs.items():
        bad = mismatches(lib)
        assert bad, name + ": no case of any list tells this header from the right one"
        report.append("%s: %s" % (name, ", ".join("%s %d of %d" % (op, len(i), len(cases(op))) for op, i in bad.items())))
    bad = mismatches(libs["two final subtractions in sc_reduce512"], ("mul",))["mul"]
    three = [i for i, (_, f) in enumerate(model("mul")) if f.subs == 3]
    assert bad == three and len(three) >= ec.MIN_PER_COUNT
    first_random = len(cases("mul")) - len(ec.random_products())
    report.append("two final subtractions: %d products fail, %d of them among the 64 random ones" % (len(bad), sum(i >= first_random for i in bad)))
    with capsys.disabled():
        print("\n" + "\n".join(report))
