"""The scalar arithmetic mod l (csrc/sc25519.h) on the GPU, one operation per lane (act_debug_sc_batch, csrc/k_debug_sc.hip), on the
case lists of tests/sc_edge_cases.py: 2^252 and l, word and limb boundaries, every number of final subtractions the fold of
sc_reduce512 can take (products that take three are one in 1 400 among random ones), both sides of q c in from_bytes_mod_order, the
lazy bound of the Montgomery product inside the inversion.  Protocol runs reach this code with random scalars only.

Expected values never come from the code under test: the big-integer model of the header (tests/sc_model.py, held to plain `% ELL`
arithmetic by tests/test_sc_edges_host.py), every byte of every lane -- scm_mul limb for limb -- and libsodium's records where they
exist.  Everything is bit-exact.  Every call is longer than a chunk of the context and ends in a ragged block; what the operation does
not write (the rest of a lane's record, the lanes from n on) must come back as it went in."""
import numpy as np
import pytest

import sc_edge_cases as ec
import sc_model as sm
from sc_edge_cases import OPS, cases, model

pytestmark = pytest.mark.gpu

L_SMALL, MAX_BATCH = 8, 512
FILL = 0xA5A5A5A5
JUNK = 0xC3                                            # operand bytes an operation must not read
WORDS = 16                                             # words of a lane's record
IN_BYTES = {"load_wide": 64, "load_sc": 32, "scm_mul": 40}                   # every other operation: 32
OUT_WORDS = {"scm_mul": 10, "equal": 1, "is_zero": 1}                        # every other operation: 8


@pytest.fixture(scope="module")
def eng(oracle):
    from act_amd import capi
    e = capi.Engine(oracle.params_new("sc-edges", "svc", "env", "v1"), L_SMALL, max_batch=MAX_BATCH)
    try:
        yield e
    finally:
        e.close()


def records(op, values):
    """One operand array: a 64-byte record per lane, the operand at its start and JUNK behind it."""
    k = IN_BYTES.get(op, 32)
    if op == "scm_mul":
        enc = lambda v: np.array(sm.val_limbs(v), "<u4").tobytes()
    else:
        enc = lambda v: v.to_bytes(k, "little")
    return np.frombuffer(b"".join(enc(v) + bytes([JUNK]) * (4 * WORDS - k) for v in values), "<u4")


def run(eng, op, cs):
    """The cases through the hook in one call: per lane the result (an integer, for scm_mul ten limbs), after the checks on everything
    the operation must leave alone."""
    n = len(cs)
    r = eng.debug_sc(op, n, *[records(op, [c[k] for c in cs]) for k in range(len(cs[0]))], fill=FILL)
    lanes = (n + 255) // 256 * 256
    assert r.size == WORDS * lanes
    r = r.reshape(lanes, WORDS)
    k = OUT_WORDS.get(op, 8)
    assert (r[n:] == FILL).all(), (op, n, "a lane from n on was written")
    assert (r[:n, k:] == FILL).all(), (op, n, "words of a record behind the result were written")
    if op == "scm_mul":
        return [[int(x) for x in row[:k]] for row in r[:n]]
    return [int.from_bytes(row[:k].astype("<u4").tobytes(), "little") for row in r[:n]]


@pytest.mark.parametrize("op", OPS)
def test_operation_on_its_edge_cases(eng, op):
    """The whole list of the operation in one call (repeated from its start where it is shorter than a chunk and a block more)."""
    cs = ec.ragged(cases(op), MAX_BATCH)
    want = [w for w, _ in model(op)]
    assert len(cs) > MAX_BATCH and len(cs) % 256
    got = run(eng, op, cs)
    bad = [i for i in range(len(cs)) if got[i] != want[i % len(want)]]
    assert not bad, (op, "wrong cases (indices into the list, the first 32)", sorted({i % len(want) for i in bad})[:32], "of", len(want),
                     "the first", [hex(v) for v in cs[bad[0]]], got[bad[0]], want[bad[0] % len(want)])


def test_libsodium_records(eng):
    """crypto_core_ristretto255_scalar_reduce / _add / _sub / _mul / _negate / _invert of libsodium 1.0.18 on the same entry."""
    g = ec.sodium()
    le = ec.le_int
    for op, key in (("load_sc", "sc_reduce32"), ("load_wide", "sc_reduce_wide")):
        assert run(eng, op, [(le(v["in"]),) for v in g[key]]) == [le(v["out"]) for v in g[key]], op
    ring = g["sc_ring"]
    for op, key in (("add", "add"), ("sub", "sub"), ("mul", "mul")):
        assert run(eng, op, [(le(v["a"]), le(v["b"])) for v in ring]) == [le(v[key]) for v in ring], op
    for op, key in (("neg", "neg_a"), ("invert", "inv_a")):
        assert run(eng, op, [(le(v["a"]),) for v in ring]) == [le(v[key]) for v in ring], op


@pytest.mark.parametrize("n", [1, 63, 65, 256])
def test_batch_sizes_and_the_lanes_beyond(eng, n):
    """One lane, one short of a wave, one past it, one whole block: every lane right, everything else as the caller filled it."""
    for op in ("muladd", "load_wide", "scm_mul"):
        base, want = cases(op), [w for w, _ in model(op)]
        pick = [(7 * i + n) % len(base) for i in range(n)]
        assert run(eng, op, [base[k] for k in pick]) == [want[k] for k in pick], (op, n)


def test_arguments_are_checked(eng):
    from act_amd import capi
    a = np.zeros(WORDS, np.uint32)
    with pytest.raises(capi.ActError):
        eng.debug_sc("add", 1, a)                          # b missing
    with pytest.raises(capi.ActError):
        eng.debug_sc("muladd", 1, a, a)                    # c missing
    with pytest.raises(capi.ActError):
        eng.debug_sc("scm_mul", 1, a)                      # b missing
    r = np.zeros(WORDS * 256, np.uint32)
    ERR_ARG = eng.lib.act_debug_sc_batch(None, 0, 1, a.ctypes.data, None, None, r.ctypes.data)
    assert ERR_ARG != 0
    for op in (len(eng.SC_OPS), -1):
        assert eng.lib.act_debug_sc_batch(eng.ctx, op, 1, a.ctypes.data, a.ctypes.data, a.ctypes.data, r.ctypes.data) == ERR_ARG
    assert eng.lib.act_debug_sc_batch(eng.ctx, eng.SC_OPS.index("neg"), 1, None, None, None, r.ctypes.data) == ERR_ARG
    assert eng.lib.act_debug_sc_batch(eng.ctx, eng.SC_OPS.index("neg"), 1, a.ctypes.data, None, None, None) == ERR_ARG
    assert not r.any()
