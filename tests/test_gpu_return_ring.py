"""Key rotation and partial refunds together, on the GPU: act_refund_to_credit_token_return_keyring_batch through the C ABI against the
model of tests/return_ring_cases.py (refund_return_cases.to_credit_token_return once per ring key, the smallest accepting index being
the expected out_key) -- never against the library itself, except where the contract IS "the bytes of another call": nkeys == 1 is
act_refund_to_credit_token_return_batch, t == 0 everywhere is act_refund_to_credit_token_keyring_batch on the first 128 bytes.

L = 8; n = 1, 3, 64, 65 and 300 cross one wavefront and one 256-thread block in both the (key, item) grid of the candidate and hash
kernels and the item grid of the finish; one case at L = 128.  Both transcript modes, host and device memory.  The lanes walk the pool
over and over, so one wavefront holds every ring index, "no key" and every refusal."""
import numpy as np
import pytest

import return_ring_cases as rc
from conftest import shake
from test_gpu_admission import Dev, step

pytestmark = pytest.mark.gpu

L = 8
SIZES = (1, 3, 64, 65, 300)
NONE = rc.KEY_NONE
_pools = {}


def _pool(oracle, h, L=L, want=None):
    """the items and the model's per-key answers, computed once per L and shared"""
    if L not in _pools:
        _pools[L] = rc.ReturnPool(oracle.ctx(h, L), h, L, "grr-%d" % L, want)
    return _pools[L]


def _engine(engine_factory, h, mode, L=L, max_batch=4096):
    from act_amd import capi
    return engine_factory(h, L, max_batch=max_batch, transcript=capi.TRANSCRIPT_HOST if mode == "host" else capi.TRANSCRIPT_DEVICE)


def _call(eng, mem, pool, ring, idx):
    pre, proofs, recs = pool.inputs(idx)
    publics = pool.ring_w(ring)
    n = len(idx)
    if mem == "host":
        return eng.refund_to_credit_token_return_ring(pre, proofs, recs, publics)
    from act_amd import capi
    d = Dev(); ins = [d.up(x) for x in (pre, proofs, recs)]; tok, st, ok = d.new(160 * n, 7), d.new(n, 99), d.new(n, 77)
    d.t.cuda.synchronize()
    eng.client_ring_ptr("refund_return", publics, n, capi.MEM_DEVICE, pre=ins[0].data_ptr(), proofs=ins[1].data_ptr(), refund=ins[2].data_ptr(),
                        out=tok.data_ptr(), status=st.data_ptr(), out_key=ok.data_ptr())
    return d.down(st, n), d.down(tok, 160 * n), d.down(ok, n)


def _check(eng, mem, pool, ring, idx):
    st, tok, ok = _call(eng, mem, pool, ring, idx)
    est, ekey, etok = pool.expected(ring, idx)
    assert (st, ok) == (est, ekey), (ring, len(idx), list(st[:40]), list(ok[:40]), list(est[:40]), list(ekey[:40]))
    assert tok == etok, (ring, len(idx))
    return st, ok


MODES = [("host", "host"), ("host", "device"), ("device", "host"), ("device", "device")]


# ---- 3, 4. t != 0 against the model, every refusal and their order -------------------------------------------------------------------------
@pytest.mark.parametrize("mode,mem", MODES)
def test_ring_parity_against_the_model(engine_factory, oracle, bench_params, mode, mem):
    pool = _pool(oracle, bench_params)
    eng = _engine(engine_factory, bench_params, mode)
    with step(240, "ring calls"):
        for n in SIZES if mem == "host" else (3, 65, 300):
            for ring in rc.RINGS:
                _check(eng, mem, pool, ring, pool.lanes(n))
        # spelled out once: ring a, b, c, d over one pass of the pool
        st, ok = _check(eng, mem, pool, [0, 1, 2, 3], list(range(len(pool.items))))
    got = dict(zip(pool.names, zip(st, ok)))
    for k, kn in enumerate(("a", "b", "c", "d")):
        assert [got["%s/t=%s" % (kn, tn)] for tn in ("0", "1", "s", "s+1", "l-1")] == [(0, k)] * 3 + [(8, NONE)] * 2, kn
    assert {got["stranger/t=%s" % tn] for tn in ("0", "1", "s", "s+1", "l-1")} == {(4, NONE)}      # also where t > s: no ring key signed it
    assert got["b/altered to s+1"] == (4, NONE) == got["c/altered to s"]                            # an altered t: 4, not 8
    assert got["a/undecodable_A"] == got["d/undecodable_A t=s+1"] == got["a/undecodable_Com"] == (255, NONE)
    assert eng.secret_residue() == 0                            # after calls with rejected lanes


def test_three_chunks(engine_factory, oracle, bench_params):
    """n = 2 * max_batch + 37 on an engine with a small max_batch: the chunk loop, both memory kinds"""
    pool = _pool(oracle, bench_params)
    small = _engine(engine_factory, bench_params, "device", max_batch=16)
    with step(120, "three chunks"):
        for mem in ("host", "device"):
            for ring in ([0], [1, 0, 2], [0, 1, 2, 3], [3, 2]):
                _check(small, mem, pool, ring, pool.lanes(2 * 16 + 37))
    assert small.secret_residue() == 0


# ---- 1. nkeys == 1 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["host", "device"])
def test_one_key_ring_is_the_one_key_return_call(engine_factory, oracle, bench_params, mode):
    """byte for byte the outputs of act_refund_to_credit_token_return_batch under that key, for every key, accepted or not; n = 3 takes
    the one-launch road there and the chunked launches here"""
    pool = _pool(oracle, bench_params)
    eng = _engine(engine_factory, bench_params, mode)
    with step(120, "one-key rings"):
        for n in (3, 70):
            idx = pool.lanes(n) if n > 3 else [pool.by["b/t=s"], pool.by["b/t=s+1"], pool.by["a/undecodable_A"]]
            pre, proofs, recs = pool.inputs(idx)
            for k in range(5):
                one = eng.refund_to_credit_token_return(pre, proofs, recs, pool.publics[k])
                st, tok, ok = _call(eng, "host", pool, [k], idx)
                assert (st, tok) == one, (n, k)
                assert ok == bytes(0 if s == 0 else NONE for s in st)
                assert (st, ok, tok) == pool.expected([k], idx)
            st, tok, ok = _call(eng, "device", pool, [1], idx)
            assert (st, tok) == eng.refund_to_credit_token_return(pre, proofs, recs, pool.publics[1])


# ---- 2. t == 0 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["host", "device"])
def test_nothing_returned_is_the_refund_ring(engine_factory, oracle, bench_params, mode):
    """status, token and out_key of act_refund_to_credit_token_keyring_batch on the first 128 bytes of each record"""
    pool = _pool(oracle, bench_params)
    eng = _engine(engine_factory, bench_params, mode)
    zero = pool.zero_items()
    assert len(zero) == 5
    with step(120, "t = 0"):
        for n in (1, 65, 300):
            idx = pool.lanes(n, only=zero)
            pre, proofs, recs = pool.inputs(idx)
            refunds = b"".join(recs[160 * i:160 * i + 128] for i in range(n))
            for ring in rc.RINGS:
                want = eng.refund_to_credit_token_ring(pre, proofs, refunds, pool.ring_w(ring))
                assert _call(eng, "host", pool, ring, idx) == want, (n, ring)
            assert _call(eng, "device", pool, [1, 0, 3], idx) == eng.refund_to_credit_token_ring(pre, proofs, refunds, pool.ring_w([1, 0, 3])), n


# ---- L = 128 ----------------------------------------------------------------------------------------------------------------------------------
def test_full_width_proofs(engine_factory, oracle, bench_params):
    """L = 128, n = 3: the Horner sum over 128 commitments with t h1 in X_A, s read from a 16.8 KB proof record"""
    names = ("d/t=s", "b/t=s+1", "stranger/t=1")
    pool = _pool(oracle, bench_params, 128, want=set(names))
    eng = _engine(engine_factory, bench_params, "device", 128, max_batch=16)
    idx = [pool.by[x] for x in names]
    with step(240, "L = 128"):
        for mem in ("host", "device"):
            st, ok = _check(eng, mem, pool, [0, 1, 2, 3], idx)
            assert (list(st), list(ok)) == ([0, 8, 4], [3, NONE, NONE])
        st, ok = _check(eng, "host", pool, [3, 1], idx)
        assert (list(st), list(ok)) == ([0, 8, 4], [0, NONE, NONE])


# ---- 5, 6. the ring's arguments and the table cache ---------------------------------------------------------------------------------------------
def test_ring_arguments_and_table_cache(engine_factory, oracle, bench_params):
    """nkeys out of range or a ring entry that is not a canonical encoding fails the call with ACT_ERR_ARG and writes nothing; consecutive
    calls with different rings on one context follow the ring's bytes"""
    pool = _pool(oracle, bench_params)
    eng = _engine(engine_factory, bench_params, "device")
    idx = [pool.by["a/t=1"], pool.by["b/t=s"], pool.by["c/t=s+1"], pool.by["d/t=0"]]
    pre, proofs, recs = pool.inputs(idx)
    n = len(idx)
    good = pool.ring_w([0, 1])
    want = pool.expected([0, 1], idx)
    with step(120, "ring arguments"):
        for publics in ([], pool.ring_w([0, 1, 2, 3, 4]), [good[0], b"\xff" * 32], [b"\xff" * 32, good[1]], [good[0], good[1], shake("grr-not-a-point", 31) + b"\x80"]):
            rc_, st, tok, ok = eng.refund_to_credit_token_return_ring(pre, proofs, recs, publics, raw=True)
            assert rc_ == 1, len(publics)
            assert st == bytes(n) and tok == bytes(160 * n) and ok == bytes(n)
            assert eng.refund_to_credit_token_return_ring(pre, proofs, recs, good) == (want[0], want[2], want[1])
        for ring in ([0, 1], [0, 2], [0, 1], [1, 1], [1, 0], [3, 2, 1, 0], [0, 3]):
            _check(eng, "host", pool, ring, idx)
        # the plain refund ring shares the cache: alternate the two calls over rings that differ in their later entries
        zero = pool.lanes(6, only=pool.zero_items())
        zpre, zproofs, zrecs = pool.inputs(zero)
        refunds = b"".join(zrecs[160 * i:160 * i + 128] for i in range(len(zero)))
        for ring in ([0, 1], [0, 3, 2], [2, 0]):
            plain = eng.refund_to_credit_token_ring(zpre, zproofs, refunds, pool.ring_w(ring))
            _check(eng, "host", pool, ring[::-1], idx)
            assert _call(eng, "host", pool, ring, zero) == plain, ring


# ---- 7. end to end ------------------------------------------------------------------------------------------------------------------------------
def test_api_round_trip():
    """Keyring.redeem_return_batch(sign_with=1) moves the client onto ring key 1 without telling it and returns credits;
    to_credit_token_return_ring finds index 1 among the published keys, and the token's next proof, of its whole balance, verifies"""
    from act_amd import api
    params = api.Params.new("test-org", "test-service", "test", "2024-01-01")
    rng = api.ByteStreamRng(shake("grr-api", 1 << 20))
    with step(240, "api round trip"):
        a, b = api.PrivateKey.random(rng, params), api.PrivateKey.random(rng, params)
        ring = api.Keyring([a, b])
        publics = [ring.public(0), ring.public(1)]
        pre = api.PreIssuance.random(rng, params); req = pre.request(params, rng)
        tok = pre.to_credit_token(params, a.public(), req, a.issue(params, req, 20, rng))
        proof, prerefund = tok.prove_spend(params, 5, rng)
        db = api.NullifierDb(1000)
        res, matched = ring.redeem_return_batch(params, db, [proof], rng, returned=[3], charges=[5], sign_with=1)
        assert matched == [0] and isinstance(res[0], api.RefundReturn) and ring.last_return_counts["accepted"] == 1
        new, idx = prerefund.to_credit_token_return_ring(params, proof, res[0], publics)
        assert idx == 1 and new == prerefund.to_credit_token_return(params, proof, res[0], b.public())
        assert api.scalar_to_u128(new.credits()) == 20 - 5 + 3
        assert prerefund.to_credit_token_return_ring(params, proof, res[0], [b.public(), a.public()])[1] == 0
        with pytest.raises(api.Error) as ex:
            prerefund.to_credit_token_return_ring(params, proof, res[0], [a.public()])
        assert ex.value.code == 4
        with pytest.raises(api.Error) as ex:
            prerefund.to_credit_token_return_ring(params, proof, api.RefundReturn(res[0].record[:128] + api.scalar(4)), publics)
        assert ex.value.code == 4
        # the new token spends ALL of its balance, and the proof verifies under the key the client was moved onto
        proof2, _ = new.prove_spend(params, 18, rng)
        st, matched2 = ring.verify_spend_batch(params, [proof2])
        assert (st, matched2) == (bytes(1), [1])
