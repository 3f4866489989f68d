"""Fixed-base tables at every window width the ABI accepts (act_ctx_set_fixed_base_bits: 4..24 bits), on the device.  The width is a
run-time parameter of the table builder (k_build_table), of the product (msm.h fb_windows / fb_next_digit / fixed_base_acc) and of
the table cache; it decides the number of windows, whether the top window is full (11, 23), whether it holds the single bit 2^252
(4, 6, 7, 9, 12, 14, 18, 21) and where digits straddle 32-bit words.  One product per lane (act_debug_fixed_base_batch) on chosen
scalars (tests/fixed_base_cases.py) against the Python model and the C oracle, byte for byte, for all four bases; then the protocol
calls -- verifier, issuer, client, and the fast build's prover -- at non-default widths against the oracle.

Params and engines are this file's own: a changed width must not reach the session's cached engines."""

import pytest

import fixed_base_cases as fb
from conftest import ELL, load_golden, shake, scb

pytestmark = pytest.mark.gpu

L_SMALL, MAX_BATCH = 8, 512
PROTOCOL_WIDTHS = [4, 11, 13, 23, 24]


@pytest.fixture(scope="module")
def mine(oracle):
    return oracle.params_new("fixed-base-widths", "svc", "env", "v1")


@pytest.fixture(scope="module")
def expected(oracle, mine):
    """per base g, h1, h2, h3: the edge set's encodings from the Python model, computed once"""
    return [fb.Expected(oracle, None)] + [fb.Expected(oracle, mine[32 * b:32 * b + 32]) for b in range(3)]


@pytest.fixture(scope="module")
def eng(mine):
    from act_amd import capi
    e = capi.Engine(mine, L_SMALL, max_batch=MAX_BATCH)
    try:
        yield e
    finally:
        e.close()


def _set_width(eng, base, w):
    """A width above 20 bits may be refused for memory, and only for that; the refusal is a skip that says which table it was."""
    from act_amd import capi
    try:
        eng.set_fixed_base_bits(base, w)
    except capi.ActError as e:
        if w > 20 and "not enough free device memory" in str(e):
            pytest.skip("no room on this device for the %d-bit table of base %d" % (w, base))
        raise


def _restore(eng):
    for b in range(4):
        if eng.fixed_base_bits()[b] != 16:
            eng.set_fixed_base_bits(b, 16)


def _check_lanes(eng, ex, base, w):
    scalars, want, lanes = ex.lanes(w)
    got = eng.debug_fixed_base(base, scalars)           # more than max_batch lanes: ragged chunks
    assert len(lanes) > MAX_BATCH and len(lanes) % MAX_BATCH and len(got) == len(want)
    bad = [i for i in range(len(lanes)) if got[32 * i:32 * i + 32] != want[32 * i:32 * i + 32]]
    assert not bad, (w, base, len(bad), [(i, lanes[i].hex(), fb.digits(int.from_bytes(lanes[i], "little") % ELL, w)) for i in bad[:4]])


def _check_a_handful_at_16(eng, ex, base):
    assert eng.fixed_base_bits()[base] == 16
    pick = [0, 3, 6, 7 + 252, 7 + 253, len(ex.edge) - 1]      # 0, l - 1, 2^252 (twice: as an edge and as a bit), 2^256 - 1, a random one
    assert eng.debug_fixed_base(base, b"".join(ex.edge[i] for i in pick)) == b"".join(ex.edge_want[i] for i in pick)


@pytest.mark.parametrize("w", range(4, 21))
def test_fixed_base_product_at_width(eng, expected, w):
    """All four bases at w bits: the edge set and w's window set through the table of that width; the generator's also against
    libsodium's known answers.  Back at 16 bits the same context gives the same bytes."""
    from act_amd import capi
    try:
        for b in range(4):
            eng.set_fixed_base_bits(b, w)
        assert eng.fixed_base_bits() == [w] * 4
        for b in range(4):
            _check_lanes(eng, expected[b], b, w)
        v = load_golden("sodium_primitives.json")["scalarmult_base"]
        out = eng.debug_fixed_base(0, b"".join(bytes.fromhex(x["scalar"]) for x in v))
        assert [out[32 * i:32 * i + 32].hex() for i in range(len(v))] == [x["out"] for x in v]
        with pytest.raises(capi.ActError):
            eng.debug_fixed_base(4, bytes(32))
        with pytest.raises(capi.ActError):
            eng.debug_fixed_base(-1, bytes(32))
    finally:
        _restore(eng)
    for b in range(4):
        _check_a_handful_at_16(eng, expected[b], b)


@pytest.mark.parametrize("base", range(4))
@pytest.mark.parametrize("w", range(21, 25))
def test_fixed_base_product_at_wide_width(eng, expected, w, base):
    """One base at a time (a 24-bit table is 23.6 GB), restored to 16 bits before the next."""
    try:
        _set_width(eng, base, w)
        assert eng.fixed_base_bits() == [w if b == base else 16 for b in range(4)]
        _check_lanes(eng, expected[base], base, w)
    finally:
        _restore(eng)
    _check_a_handful_at_16(eng, expected[base], base)


def _engine_at_width(mine, L, w):
    """An engine of the caller's own (to be closed by it) with all four bases at w bits, or h1 and h3 -- the range kernel's bases, the
    ones bench.py widens -- above 20."""
    from act_amd import capi
    e = capi.Engine(mine, L, max_batch=MAX_BATCH)
    try:
        for b in ((0, 1, 2, 3) if w <= 20 else (1, 3)):
            _set_width(e, b, w)
        assert e.fixed_base_bits() == ([w] * 4 if w <= 20 else [16, w, 16, w])
    except BaseException:
        e.close()
        raise
    return e


@pytest.mark.parametrize("L", [64, L_SMALL])
@pytest.mark.parametrize("w", PROTOCOL_WIDTHS)
def test_crafted_scalars_reproduce_the_oracle_transcript_at_width(oracle, mine, w, L):
    """test_gpu_parity.py's crafted proofs (gamma, gamma0_j, z_j0 on recoding corner cases), here with the scalars of EVERY fixed-base
    product of the verifier steered as well -- k, c_bar, r_bar, w00, w01, z_j1, k_bar, s_bar onto the ends of the scalar range, the
    top window's largest digit and window-edge entries of width w -- through both schedules.  Every commitment the verifier recomputes
    is in the transcript, which must equal the oracle's byte for byte."""
    octx = oracle.ctx(mine, L)
    pats = [0, 1, 3, 7, ELL - 1, ELL - 3, (1 << 252) - 1, 1 << 252] + [int(c * 63, 16) % ELL for c in "37bf5"]
    pats += [2 * x % ELL for x in [int(("%x" % d) * 63, 16) for d in range(1, 9)] + [int("08" * 31, 16), sum(1 << i for i in range(0, 252, 3)),
                                                                                   sum(3 << i for i in range(0, 249, 3))]]
    N = len(pats)
    eng = _engine_at_width(mine, L, w)
    try:
        sk = octx.private_key_random(shake("fbw-pk", 64))
        pre = octx.pre_issuance_random(shake("fbw-pre", 128))
        req = eng.request(pre, shake("fbw-rq", 128))
        st, resp = eng.issue(sk, req, scb(1000), shake("fbw-ir", 128))
        st, tok = eng.issuance_to_credit_token(pre, sk[32:], req, resp)
        st, proof, _ = eng.prove_spend(tok, scb(321), shake("fbw-pr", octx.prove_rng_bytes))
        assert st == b"\0" and proof == octx.prove_spend(tok, scb(321), shake("fbw-pr", octx.prove_rng_bytes))[1]
        recs = fb.steer_fixed_base_fields(fb.crafted_spend_proofs(proof, L, pats), L, fb.protocol_scalars(w))
        batch = b"".join(recs)
        want = [octx.verify_spend(sk, r, True) for r in recs]
        for small_max in (8192, 0):          # the small-batch schedule, then the pipelined one
            eng.set_small_batch_max(small_max)
            st, kp = eng.verify_spend(sk, batch, True)
            trs = eng.last_spend_transcripts(N)
            for i in range(N):
                so, kpo, tro = want[i]
                assert so == st[i] and so != 0, (w, small_max, i)
                assert trs[i] == tro, (w, small_max, i)
    finally:
        eng.close()


def issuer_scalars(w):
    """Amounts c and nonces e of the issuer test: the whole edge set (as canonical scalars) and width w's protocol set."""
    return [int.from_bytes(x, "little") % ELL for x in fb.edge_scalars()] + fb.protocol_scalars(w)


@pytest.mark.parametrize("w", PROTOCOL_WIDTHS)
def test_issuer_and_client_at_width(oracle, mine, w):
    """The issuer's c h1 (k_sign.hip) and the client's e G (k_client.hip) on chosen scalars at width w: lane i's amount c is value i of
    the edge set followed by the width's protocol set, and the issuer's nonce e (the wide reduction of the first 64 rng bytes) is
    steered onto the same list, half a turn on, so every value is once a c and once an e.  Responses must equal the oracle's through
    the one-kernel path (calls of at most 64 lanes) and the multi-launch path; the client must accept every one and build the oracle's
    token."""
    octx = oracle.ctx(mine, L_SMALL)
    vals = issuer_scalars(w)
    n = len(vals)
    eng = _engine_at_width(mine, L_SMALL, w)
    try:
        sk = octx.private_key_random(shake("fbw-i-pk", 64))
        pre = b"".join(octx.pre_issuance_random(shake("fbw-i-pre-%d" % i, 128)) for i in range(n))
        rq = shake("fbw-i-rq", 128 * n)
        req = eng.request(pre, rq)
        assert req == octx.request_batch(pre, rq, 8)
        cam = b"".join(scb(v) for v in vals)
        irng = b"".join(scb(vals[(i + n // 2) % n]) + bytes(32) + shake("fbw-i-ir-%d" % i, 64) for i in range(n))
        sto, respo = octx.issue_batch(sk, req, cam, irng, 8)
        assert sto == bytes(n) and all(respo[160 * i + 32:160 * i + 64] == irng[128 * i:128 * i + 32] for i in range(n))      # e is where it was aimed
        try:
            for tiny, step in ((1, 64), (0, n)):
                eng.set_tiny_calls(tiny)
                st, resp, tok = b"", b"", b""
                for lo in range(0, n, step):
                    hi = min(n, lo + step)
                    s1, r1 = eng.issue(sk, req[128 * lo:128 * hi], cam[32 * lo:32 * hi], irng[128 * lo:128 * hi])
                    assert s1 == sto[lo:hi] and r1 == respo[160 * lo:160 * hi], (w, tiny, lo)
                    s2, t1 = eng.issuance_to_credit_token(pre[64 * lo:64 * hi], sk[32:], req[128 * lo:128 * hi], r1)
                    assert s2 == bytes(hi - lo), (w, tiny, lo, list(s2))
                    resp += r1; tok += t1
                for i in range(n):
                    so, to = octx.issuance_to_credit_token(pre[64 * i:64 * i + 64], sk[32:], req[128 * i:128 * i + 128], resp[160 * i:160 * i + 160])
                    assert so == 0 and to == tok[160 * i:160 * i + 160], (w, tiny, i)
        finally:
            eng.set_tiny_calls(1)
    finally:
        eng.close()


@pytest.mark.parametrize("w", [4, 11])
def test_prove_spend_at_width(oracle, mine, w):
    """The prover of the fast build (libact_mi355x_fast.so) reads the tables this width applies to; the default build's does not
    (matrix-core look-ups) and must not care.  tests/test_gpu_fast_option.py runs this under the fast build."""
    octx = oracle.ctx(mine, L_SMALL)
    n = 3
    eng = _engine_at_width(mine, L_SMALL, w)
    try:
        sk = octx.private_key_random(shake("fbw-p-pk", 64))
        pre = eng.pre_issuance_random(shake("fbw-p-pre", 128 * n)); req = eng.request(pre, shake("fbw-p-rq", 128 * n))
        assert req == octx.request_batch(pre, shake("fbw-p-rq", 128 * n), 1)
        st, resp = eng.issue(sk, req, scb(200) * n, shake("fbw-p-ir", 128 * n))
        st, tok = eng.issuance_to_credit_token(pre, sk[32:], req, resp)
        assert st == bytes(n)
        s_b, rng = scb(0) + scb(77) + scb(200), shake("fbw-p-pr", octx.prove_rng_bytes * n)
        st, proofs, prer = eng.prove_spend(tok, s_b, rng)
        assert st == bytes(n) and (proofs, prer) == octx.prove_spend_batch(tok, s_b, rng, 1)
        assert eng.verify_spend(sk, proofs) == bytes(n)
    finally:
        eng.close()
