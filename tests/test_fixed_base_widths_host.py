"""The fixed-base product at every window width the host build can afford (4..11 bits), on the CPU: the table filled by the lane
body of k_build_table (msm.h fb_table_entry, the function the kernel calls) and read by fixed_base_acc, both at a RUN-TIME width as
on the device (the entries the scalars read; every one of them at 4..8 bits), against the Python model and the C oracle -- for the generator and for one Params point, on the edge set and each
width's window set (tests/fixed_base_cases.py).  Byte for byte, every lane.  (tests/test_gpu_fixed_base_widths.py runs the same
sets on the device at 4..24 bits.)"""
import ctypes as C

import pytest

import fixed_base_cases as fb

HOST_WIDTHS = list(range(4, 12))


@pytest.fixture(scope="module")
def expected(oracle, bench_params):
    """per base: the edge set's encodings (Python model), computed once"""
    return {"g": fb.Expected(oracle, None), "h1": fb.Expected(oracle, bench_params[:32])}


@pytest.fixture(scope="module")
def hc_fixed_base_w(hostcheck):
    fn = hostcheck.hc_fixed_base_w
    fn.argtypes = [C.c_char_p, C.c_int, C.c_size_t, C.c_char_p, C.c_char_p]
    return fn


def test_the_scalar_sets_are_what_they_claim():
    """Every scalar is canonical (or the one deliberate exception), fb_next_digit's decomposition -- digit pos = bits [w pos, w pos + w)
    -- rebuilds it exactly at all 21 widths, and the window set reaches what it is there for: every entry of every window at
    w <= 8, both edge entries of every window above, the top window's largest digit, and the lone top bit 2^252."""
    edge = [int.from_bytes(s, "little") for s in fb.edge_scalars()]
    assert sum(v >= fb.ELL for v in edge) == 1 and len(edge) == 7 + 253 + 1 + 8      # (1, 2 and 2^252 come twice: as named edges and as single bits)
    for w in range(4, 25):
        nw, full = fb.windows(w), (1 << w) - 1
        assert (nw - 1) * w < 253 <= nw * w
        vals = fb.window_scalars(w)
        assert len(set(vals)) == len(vals) and all(0 <= v < fb.ELL for v in vals)
        hit = set()
        for v in vals + [e % fb.ELL for e in edge]:
            d = fb.digits(v, w)
            assert sum(x << (w * pos) for pos, x in enumerate(d)) == v, (w, hex(v))
            hit.update((pos, x) for pos, x in enumerate(d) if x)
        top = (fb.ELL - 1) >> (w * (nw - 1))
        assert (nw - 1, top) in hit and (nw - 1, 1) in hit
        for pos in range(nw - 1):
            want = range(1, full + 1) if w <= 8 else (1, 2, 1 << (w - 1), full - 1, full)
            assert all((pos, e) in hit for e in want), (w, pos)
        if w <= 8:
            assert all((nw - 1, e) in hit for e in range(1, top + 1)), w
            assert len(vals) <= 8192 + 4
        # every bit of a digit in every window: the single-bit scalars
        assert all((k // w, 1 << (k % w)) in hit for k in range(253)), w


@pytest.mark.parametrize("base", ["g", "h1"])
@pytest.mark.parametrize("w", HOST_WIDTHS)
def test_host_fixed_base_product_at_width(hc_fixed_base_w, expected, base, w):
    ex = expected[base]
    scalars, want, lanes = ex.lanes(w)
    n = len(lanes)
    pt = ex.base_enc if ex.base_enc is not None else ex.m.ristretto_encode(ex.m.BASEPOINT)
    out = C.create_string_buffer(32 * n)
    assert hc_fixed_base_w(pt, w, n, scalars, out) == 1
    got = out.raw
    bad = [i for i in range(n) if got[32 * i:32 * i + 32] != want[32 * i:32 * i + 32]]
    assert not bad, (w, base, len(bad), [(i, lanes[i].hex(), fb.digits(int.from_bytes(lanes[i], "little") % fb.ELL, w)) for i in bad[:4]])


def test_host_fixed_base_refuses_what_the_abi_refuses(hc_fixed_base_w, expected):
    pt = expected["h1"].base_enc
    out = C.create_string_buffer(32)
    assert hc_fixed_base_w(pt, 3, 1, bytes(32), out) == 0 and hc_fixed_base_w(pt, 25, 1, bytes(32), out) == 0
