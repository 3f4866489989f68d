"""The client's side of key rotation on the GPU: act_issuance_to_credit_token_keyring_batch / act_refund_to_credit_token_keyring_batch
through the C ABI against the C oracle called once per ring key (oracle.issuance_to_credit_token / .refund_to_credit_token under w_k, the
smallest accepting index being the expected out_key) -- never against the library itself, except where the contract IS "the bytes of
the one-key call" (nkeys == 1).  Both transcript modes, host and device memory, rings of 1..4, lanes that alternate over the signing
keys with the rejection cases among them, and an engine with a small max_batch so that n = 2 * max_batch + 37 spans three chunks."""
import numpy as np
import pytest

import client_ring_cases as cr
from conftest import shake

pytestmark = pytest.mark.gpu

MB = 16
RINGS = ([0], [0, 1], [1, 0, 2], [0, 1, 2, 3], [0, 0, 1], [3, 2])
_pools = {}


def _pool(oracle, h, L, issuance):
    """the items and the per-key oracle table, computed once per (L, kind) and shared"""
    key = (L, issuance)
    if key not in _pools:
        _pools[key] = cr.Pool(oracle.ctx(h, L), L, issuance, "gcr-%d-%d" % (L, issuance))
    return _pools[key]


class _Dev:
    """the calls from device memory (torch tensors as the caller's HBM)"""

    def __init__(self):
        import torch
        self.t = torch

    def up(self, b):
        return self.t.from_numpy(np.frombuffer(b + b"\0", np.uint8).copy()).cuda()

    def new(self, n, fill):
        return self.t.full((max(1, n),), fill, dtype=self.t.uint8, device="cuda")

    def down(self, t, n):
        return t.cpu().numpy().tobytes()[:n]


def _call(eng, mem, pool, ring, idx):
    pre, mid, resp = pool.inputs(idx)
    publics = pool.ring_w(ring)
    n = len(idx)
    if mem == "host":
        if pool.issuance:
            return eng.issuance_to_credit_token_ring(pre, publics, mid, resp)
        return eng.refund_to_credit_token_ring(pre, mid, resp, publics)
    from act_amd import capi
    d = _Dev(); ins = [d.up(x) for x in (pre, mid, resp)]; tok, st, ok = d.new(160 * n, 7), d.new(n, 99), d.new(n, 77)
    d.t.cuda.synchronize()
    if pool.issuance:
        eng.client_ring_ptr("issuance", publics, n, capi.MEM_DEVICE, pre=ins[0].data_ptr(), req=ins[1].data_ptr(), resp=ins[2].data_ptr(),
                            out=tok.data_ptr(), status=st.data_ptr(), out_key=ok.data_ptr())
    else:
        eng.client_ring_ptr("refund", publics, n, capi.MEM_DEVICE, pre=ins[0].data_ptr(), proofs=ins[1].data_ptr(), refund=ins[2].data_ptr(),
                            out=tok.data_ptr(), status=st.data_ptr(), out_key=ok.data_ptr())
    return d.down(st, n), d.down(tok, 160 * n), d.down(ok, n)


def _check(eng, mem, pool, ring, n):
    idx = pool.lanes(n)
    st, tok, ok = _call(eng, mem, pool, ring, idx)
    est, ekey, etok = pool.expected(ring, idx)
    assert (st, ok) == (est, ekey), (ring, n, list(st[:16]), list(ok[:16]), list(est[:16]), list(ekey[:16]))
    assert tok == etok, (ring, n)
    return st, ok


@pytest.mark.parametrize("issuance", [True, False], ids=["issuance", "refund"])
@pytest.mark.parametrize("mode,mem", [("host", "host"), ("host", "device"), ("device", "host"), ("device", "device")])
def test_ring_parity_through_the_c_abi(engine_factory, oracle, bench_params, issuance, mode, mem):
    from act_amd import capi
    L = 8
    tr = capi.TRANSCRIPT_HOST if mode == "host" else capi.TRANSCRIPT_DEVICE
    pool = _pool(oracle, bench_params, L, issuance)
    eng = engine_factory(bench_params, L, transcript=tr)
    for n in (1, 63, 64, 65):
        for ring in RINGS:
            _check(eng, mem, pool, ring, n)
    # the table is what the feature says it is, spelled out once: ring a, b, c, d over one pass of the pool
    st, ok = _check(eng, mem, pool, [0, 1, 2, 3], len(pool.items))
    bad = 2 if issuance else 4
    assert list(zip(st, ok)) == [(0, 0), (0, 1), (0, 2), (0, 3), (bad, 255), (bad, 255), (255, 255), (255, 255)]
    assert eng.secret_residue() == 0                            # after calls with rejected lanes
    # three chunks: n = 2 * max_batch + 37 on an engine with a small max_batch
    small = engine_factory(bench_params, L, max_batch=MB, transcript=tr)
    for ring in RINGS:
        _check(small, mem, pool, ring, 2 * MB + 37)
    assert small.secret_residue() == 0


@pytest.mark.parametrize("mode", ["host", "device"])
def test_issuance_across_the_wide_kernel_limit(engine_factory, oracle, bench_params, mode):
    """n = 8193 in ONE chunk: phase A takes k_client_a instead of the role-block kernel (CLIENT_WIDE_MAX = 8192)"""
    from act_amd import capi
    pool = _pool(oracle, bench_params, 8, True)
    eng = engine_factory(bench_params, 8, max_batch=16384, transcript=capi.TRANSCRIPT_HOST if mode == "host" else capi.TRANSCRIPT_DEVICE)
    _check(eng, "host", pool, [1, 0, 3, 2], 8193)
    _check(eng, "device", pool, [2, 3], 8192)


@pytest.mark.parametrize("issuance", [True, False], ids=["issuance", "refund"])
def test_full_width_proofs(engine_factory, oracle, bench_params, issuance):
    """L = 128, n = 5"""
    from act_amd import capi
    pool = _pool(oracle, bench_params, 128, issuance)
    eng = engine_factory(bench_params, 128, max_batch=MB, transcript=capi.TRANSCRIPT_DEVICE)
    idx = [3, 1, 7, 4, 0]                                        # d, b, the undecodable Com_j / K, the stranger, a
    for ring in ([0, 1, 2, 3], [3, 1]):
        st, tok, ok = _call(eng, "host", pool, ring, idx)
        assert (st, ok, tok) == pool.expected(ring, idx), ring
    st, tok, ok = _call(eng, "device", pool, [0, 1, 2, 3], idx)
    assert (st, ok, tok) == pool.expected([0, 1, 2, 3], idx)
    assert list(ok) == [3, 1, 255, 255, 0]


@pytest.mark.parametrize("issuance", [True, False], ids=["issuance", "refund"])
def test_one_key_ring_is_the_one_key_entry_point(engine_factory, oracle, bench_params, issuance):
    """nkeys == 1: byte for byte the outputs of act_*_to_credit_token_batch under that key, for every key, accepted or not"""
    from act_amd import capi
    pool = _pool(oracle, bench_params, 8, issuance)
    for tr in (capi.TRANSCRIPT_HOST, capi.TRANSCRIPT_DEVICE):
        eng = engine_factory(bench_params, 8, transcript=tr)
        idx = pool.lanes(70)
        pre, mid, resp = pool.inputs(idx)
        for k in range(5):
            w = pool.publics[k]
            one = eng.issuance_to_credit_token(pre, w, mid, resp) if issuance else eng.refund_to_credit_token(pre, mid, resp, w)
            st, tok, ok = _call(eng, "host", pool, [k], idx)
            assert (st, tok) == one
            assert ok == bytes(0 if s == 0 else 255 for s in st)


def test_ring_arguments(engine_factory, oracle, bench_params):
    """nkeys out of range or a ring entry that does not decode fails the call with ACT_ERR_ARG and writes nothing; the one-key call's
    cached key and the ring's cached tables survive it"""
    from act_amd import capi
    pool = _pool(oracle, bench_params, 8, True)
    eng = engine_factory(bench_params, 8, transcript=capi.TRANSCRIPT_DEVICE)
    idx = [0, 1]
    pre, mid, resp = pool.inputs(idx)
    good = pool.ring_w([0, 1])
    want = pool.expected([0, 1], idx)
    for publics in ([], pool.ring_w([0, 1, 2, 3, 4]), [good[0], b"\xff" * 32], [b"\xff" * 32, good[1]], [good[0], good[1], shake("gcr-not-a-point", 31) + b"\x80"]):
        rc, st, tok, ok = eng.issuance_to_credit_token_ring(pre, publics, mid, resp, raw=True)
        assert rc == 1, len(publics)
        assert st == bytes(2) and tok == bytes(320) and ok == bytes(2)
        assert eng.issuance_to_credit_token_ring(pre, good, mid, resp) == (want[0], want[2], want[1])
    # a ring whose later entries change between calls: the tables follow the bytes
    for ring in ([0, 1], [0, 2], [0, 1], [1, 1], [1, 0]):
        st, tok, ok = _call(eng, "host", pool, ring, idx)
        assert (st, ok, tok) == pool.expected(ring, idx), ring


def test_client_ring_api_round_trip():
    """Keyring.refund_batch(sign_with=1) on the server moves the clients onto ring key 1 without telling them; to_credit_token_ring on
    the client finds index 1 among the published keys, and the resulting token spends."""
    from act_amd import api
    params = api.Params.new("test-org", "test-service", "test", "2024-01-01")
    rng = api.ByteStreamRng(shake("gcr-api", 1 << 20))
    a, b = api.PrivateKey.random(rng, params), api.PrivateKey.random(rng, params)
    ring = api.Keyring([a, b])
    publics = [ring.public(0), ring.public(1)]
    pre = api.PreIssuance.random(rng, params); req = pre.request(params, rng)
    resp = a.issue(params, req, 20, rng)
    tok, idx = pre.to_credit_token_ring(params, publics, req, resp)
    assert idx == 0 and tok == pre.to_credit_token(params, a.public(), req, resp)
    assert pre.to_credit_token_ring(params, [b.public(), a.public()], req, resp)[1] == 1
    with pytest.raises(api.Error) as ex:
        pre.to_credit_token_ring(params, [b.public()], req, resp)
    assert ex.value.code == 2
    proof, prerefund = tok.prove_spend(params, 5, rng)
    refunds, matched = ring.refund_batch(params, [proof], rng, sign_with=1)
    assert matched == [0] and isinstance(refunds[0], api.Refund)
    new, idx = prerefund.to_credit_token_ring(params, proof, refunds[0], publics)
    assert idx == 1 and new == prerefund.to_credit_token(params, proof, refunds[0], b.public())
    with pytest.raises(api.Error) as ex:
        prerefund.to_credit_token_ring(params, proof, refunds[0], [a.public()])
    assert ex.value.code == 4
    # the new token spends, and its proof verifies under the key the client was moved onto
    proof2, _ = new.prove_spend(params, 7, rng)
    st, matched2 = ring.verify_spend_batch(params, [proof2])
    assert (st, matched2) == (bytes(1), [1])
    assert api.scalar_to_u128(new.credits()) == 15
