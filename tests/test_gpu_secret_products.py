"""The products of SECRET scalars on the device, one product per lane, against references that share nothing with them.

In the default build every fixed-base product of a secret scalar -- key generation, the signing nonces, request, all of prove_spend --
is msm.h fixed_base_acc_mf: 37 signed 7-bit digits, entry |digit| of a 64-entry window picked with two chained
v_mfma_i32_32x32x32_i8 on a one-hot operand, from a table image whose byte scatter k_build_table_mf wrote.  None of it exists on the
host, and protocol calls with random scalars meet a given (window, entry, lane) about once in 300 000 products.  Here
act_debug_fixed_base_mf_batch (csrc/k_debug_secret.hip) runs that product over the context's own image, and tests/secret_fb_cases.py
aims it: every (window, digit) pair a canonical scalar can produce -- 4 610; entries 2 .. 64 of the top window are read by no scalar
below l and stay untested -- from every one of the 64 lanes, in blocks of 64 threads (k_keygen, the per-proof kernels) and of 256
(k_prove_bits).  act_debug_chain_ct_batch does the same for the address-free chains chain_ct<1>, chain_ct<2> and the four
chain_ct_quarter pieces.  Expected bytes: the Python model, the C oracle, libsodium's recorded answers.  Everything is byte-exact.

Params and the engine are this file's own; max_batch is a multiple of 64, so that lane i of a call is lane i mod 64 of a wavefront."""
import pytest

import fixed_base_cases as fb
import secret_fb_cases as sf
from conftest import load_golden

pytestmark = pytest.mark.gpu

L_SMALL, MAX_BATCH = 8, 8192
ROTATIONS_256 = (0, 37)
hx = bytes.fromhex


@pytest.fixture(scope="module")
def mine(oracle):
    return oracle.params_new("secret-products", "svc", "env", "v1")


@pytest.fixture(scope="module")
def eng(mine):
    from act_amd import capi
    assert MAX_BATCH % 64 == 0
    e = capi.Engine(mine, L_SMALL, max_batch=MAX_BATCH)
    try:
        yield e
    finally:
        e.close()


@pytest.fixture(scope="module")
def family(oracle, mine):
    """per base g, h1, h2, h3: (scalars, expected encodings, the scalars as a list) of the fixed-base family, computed once: the edge
    set through the Python model, the window set through the C oracle, both where they meet"""
    out = []
    for b in range(4):
        sc, want, lanes = fb.Expected(oracle, None if b == 0 else mine[32 * (b - 1):32 * b]).lanes(sf.MF_WBITS)
        assert lanes == sf.fixed_scalars() and len(lanes) == 4846
        out.append((sc, want, lanes))
    return out


@pytest.fixture(scope="module")
def mixed(oracle, mine):
    """per base: (scalars, expected encodings from the C oracle) of the mixed wavefronts"""
    scs = sf.mixed_scalars()
    mul = lambda b, s: oracle.mul_base(s) if b == 0 else oracle.mul(mine[32 * (b - 1):32 * b], s)
    return [(b"".join(scs), b"".join(mul(b, s) for s in scs)) for b in range(4)]


def _rotations(sc: bytes, want: bytes, rots, pad_to: int):
    """the rotations one after the other, each padded to whole blocks: (scalars, expected, [(rotation, first lane, lanes)])"""
    s_all, w_all, spans = [], [], []
    at = 0
    for r in rots:
        s, w = sf.rotate(sc, want, r, pad_to)
        s_all.append(s); w_all.append(w); spans.append((r, at, len(s) // 32)); at += len(s) // 32
    return b"".join(s_all), b"".join(w_all), spans


def _check_rotations(eng, base, fam, rots, block_threads):
    sc, want, lanes = fam
    s_all, w_all, spans = _rotations(sc, want, rots, block_threads)
    assert len(s_all) // 32 > MAX_BATCH                                # several chunks: lane arithmetic must survive the chunking
    got = eng.debug_fixed_base_mf(base, s_all, block_threads)
    assert len(got) == len(w_all)
    if got == w_all:
        return
    bad = []
    for r, at, n in spans:
        for i in range(n):
            k = at + i
            if got[32 * k:32 * k + 32] != w_all[32 * k:32 * k + 32]:
                s = s_all[32 * k:32 * k + 32]
                bad.append((r, k % 64, s.hex(), sf.mf_digits(sf.value(s))))
    assert not bad, (base, block_threads, len(bad), bad[:4])


@pytest.mark.parametrize("base", range(4))
def test_every_entry_from_every_lane(eng, family, base):
    """64 rotations x 4 846 lanes in blocks of 64 threads: every reachable (window, digit) pair, looked up from every lane"""
    _check_rotations(eng, base, family[base], range(64), 64)


@pytest.mark.parametrize("base", range(4))
def test_every_entry_in_blocks_of_256(eng, family, base):
    """the same product as k_prove_bits launches it -- four wavefronts per block, lane = threadIdx.x & 63 -- over rotations 0 and 37"""
    _check_rotations(eng, base, family[base], ROTATIONS_256, 256)


@pytest.mark.parametrize("base", range(4))
def test_mixed_wavefronts(eng, mixed, base):
    """4 096 seeded scalars: every lane of a wavefront holds a digit of its own in every window; the generator's also on libsodium's
    known answers"""
    sc, want = mixed[base]
    for bt in (64, 256):
        got = eng.debug_fixed_base_mf(base, sc, bt)
        bad = [i for i in range(len(sc) // 32) if got[32 * i:32 * i + 32] != want[32 * i:32 * i + 32]]
        assert not bad, (base, bt, len(bad), [(i % 64, sc[32 * i:32 * i + 32].hex(), sf.mf_digits(sf.value(sc[32 * i:32 * i + 32]))) for i in bad[:4]])
    if base == 0:
        v = load_golden("sodium_primitives.json")["scalarmult_base"]
        for bt in (64, 256):
            out = eng.debug_fixed_base_mf(0, b"".join(hx(x["scalar"]) for x in v), bt)
            assert [out[32 * i:32 * i + 32].hex() for i in range(len(v))] == [x["out"] for x in v], bt


def test_ragged_ends(eng, mixed):
    """A last wavefront that is not full: the lanes past n run the product with the scalar 0 -- the table operand needs their rows --
    and write nothing; what the caller holds past record n comes back as it was."""
    for base in range(4):
        sc, want = mixed[base]
        for bt in (64, 256):
            for n in (1, 63, 64, 65, 127):
                got = eng.debug_fixed_base_mf(base, sc[-32 * n:], bt, out_lanes=n + 256, fill=0xA5)
                assert got[:32 * n] == want[-32 * n:], (base, bt, n)
                assert got[32 * n:] == b"\xa5" * (32 * 256), (base, bt, n)


def test_public_road_agrees(eng, family):
    """The window set once through the public call that runs the same product, PrivateKey::random (k_keygen: one live lane, 63 that
    take the scalar 0): rng = s | 0^32 reduces to s itself."""
    sc, want, lanes = family[0]
    first = len(fb.edge_scalars())
    assert len(lanes) - first > 4500
    bad = []
    for i in range(first, len(lanes)):
        sk = eng.private_key_random(lanes[i] + bytes(32))
        if sk[:32] != lanes[i] or sk[32:] != want[32 * i:32 * i + 32]:
            bad.append((lanes[i].hex(), sf.mf_digits(sf.value(lanes[i]))))
    assert not bad, (len(bad), bad[:4])


@pytest.fixture(scope="module")
def chains(eng, oracle, mine):
    """the chain lanes, their expected encodings (the C oracle; None where the point does not decode) and what the device answered:
    the three modes of act_debug_chain_ct_batch and the bucket chain of act_debug_scalarmult_batch, each run once"""
    prim = load_golden("sodium_primitives.json")
    pts, scs, scs2, n_golden = sf.chain_lanes(prim, mine)
    undecodable = set(sf.chain_points(prim, mine)[-2:])
    red = lambda s: sf.value(s).to_bytes(32, "little")
    want = [None if p in undecodable else oracle.mul(p, red(s)) for p, s in zip(pts, scs)]
    want2 = [None if p in undecodable else oracle.mul(p, red(s)) for p, s in zip(pts, scs2)]
    for i in range(n_golden):                                          # libsodium's own answers for its (point, scalar) pairs
        assert want[i].hex() == prim["scalarmult"][i]["out"]
    P, S, S2 = b"".join(pts), b"".join(scs), b"".join(scs2)
    return {"pts": pts, "scs": scs, "scs2": scs2, "want": want, "want2": want2, "n_golden": n_golden, "golden": prim["scalarmult"][:n_golden],
            0: eng.debug_chain_ct(0, P, S), 1: eng.debug_chain_ct(1, P, S), 2: eng.debug_chain_ct(2, P, S, S2), "buckets": eng.debug_scalarmult(P, S)}


@pytest.mark.parametrize("mode", range(3))
def test_ct_chains(chains, mode):
    """chain_ct<1>, the sum of the four chain_ct_quarter pieces, chain_ct<2>: against the C oracle and libsodium, and byte for byte
    against each other and the bucket chain.  A point that does not decode: status 255, zero records."""
    c = chains
    n = len(c["pts"])
    assert n > 1500 and any(w is None for w in c["want"]) and any(p == bytes(32) for p in c["pts"])
    st, out = c[mode][0], c[mode][1]
    rec = lambda b, i: b[32 * i:32 * i + 32]
    bad = [i for i in range(n) if rec(out, i) != (c["want"][i] or bytes(32)) or st[i] != (0 if c["want"][i] else 255)]
    assert not bad, (mode, len(bad), [(c["pts"][i].hex(), c["scs"][i].hex(), st[i]) for i in bad[:4]])
    for i in range(c["n_golden"]):
        assert rec(out, i).hex() == c["golden"][i]["out"], (mode, i)
    if mode == 2:
        out2 = c[2][2]
        bad = [i for i in range(n) if rec(out2, i) != (c["want2"][i] or bytes(32))]
        assert not bad, (mode, len(bad), [(c["pts"][i].hex(), c["scs2"][i].hex()) for i in bad[:4]])
    # the three forms and the bucket chain agree with each other
    assert c[0][:2] == c[1][:2] == c[2][:2] == c["buckets"]


def test_bad_arguments(eng):
    from act_amd import capi
    one, gen = (1).to_bytes(32, "little"), load_golden("sodium_primitives.json")["scalarmult"][0]["point"]
    for base, bt in ((4, 64), (-1, 64), (0, 128), (0, 0)):
        with pytest.raises(capi.ActError):
            eng.debug_fixed_base_mf(base, one, bt)
    for mode in (3, -1):
        with pytest.raises(capi.ActError):
            eng.debug_chain_ct(mode, hx(gen), one, one)
    with pytest.raises(capi.ActError):
        eng.debug_chain_ct(2, hx(gen), one)                            # chain_ct<2> without its second scalar
    assert eng.debug_fixed_base_mf(0, b"") == b"" and eng.debug_chain_ct(0, b"", b"") == (b"", b"")
