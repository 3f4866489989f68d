"""Key rotation on the GPU: act_*_keyring_batch through the C ABI against the C oracle called once per candidate key
(oracle.verify_spend(sk_k, ...), .refund(sk_k, ...), .refund_to_credit_token(..., w)) -- never against the library itself, except
where the contract IS "the bytes of the one-key call" (nkeys == 1, a named sign_key, framing).  Both transcript modes, host and device
memory, an engine with a small max_batch so that n = 2 * max_batch + 37 spans three chunks."""
import numpy as np
import pytest

import keyring_cases as kr
from conftest import ELL, shake, scb

pytestmark = pytest.mark.gpu

MB = 16
N = 2 * MB + 37


def _keys_and_lanes(eng, octx, L, tag):
    """the lane mix of the issue (oracle-made) followed by library-made proofs under a, b, c and the stranger, N lanes in all"""
    keys = kr.make_keys(octx, tag)
    mix = kr.lane_mix(octx, keys, tag)
    proofs = [p for _, p, _ in mix]; prer = [r for _, _, r in mix]; names = [n for n, _, _ in mix]
    more = N - len(mix)
    owners = [keys[(0, 1, 2, 4, 1, 0, 2)[i % 7]] for i in range(more)]
    pre = eng.pre_issuance_random(shake(tag + "-gpre", 128 * more)); req = eng.request(pre, shake(tag + "-grq", 128 * more))
    resp = b"".join(eng.issue(owners[i], req[128 * i:128 * i + 128], scb(40 + i), shake("%s-gir%d" % (tag, i), 128))[1] for i in range(more))
    tok = b"".join(eng.issuance_to_credit_token(pre[64 * i:64 * i + 64], owners[i][32:], req[128 * i:128 * i + 128], resp[160 * i:160 * i + 160])[1] for i in range(more))
    st, pr, prr = eng.prove_spend(tok, b"".join(scb(i % 9) for i in range(more)), shake(tag + "-gpr", eng.prove_rng_bytes * more))
    assert st == bytes(more)
    pb = eng.proof_bytes
    proofs += [pr[pb * i:pb * i + pb] for i in range(more)]; prer += [prr[96 * i:96 * i + 96] for i in range(more)]
    return keys, names, proofs, prer


def _oracle_table(octx, keys, proofs):
    """status / K' of every proof under every key: the oracle loop, 16 threads"""
    blob = b"".join(proofs)
    per_key = [octx.verify_spend_batch(sk, blob, 16) for sk in keys]
    kp = [next((octx.verify_spend(keys[k], p)[1] for k in range(len(keys)) if per_key[k][i] == 0), bytes(32)) for i, p in enumerate(proofs)]
    return per_key, kp


def _want(per_key, kp, ring_idx, n):
    st, ok, k = [], [], []
    for i in range(n):
        m = next((j for j, ki in enumerate(ring_idx) if per_key[ki][i] == 0), None)
        if m is not None:
            st.append(0); ok.append(m); k.append(kp[i])
        else:
            s = {per_key[ki][i] for ki in ring_idx}
            assert len(s) == 1
            st.append(s.pop()); ok.append(255); k.append(bytes(32))
    return bytes(st), bytes(ok), b"".join(k)


class _Dev:
    """the ring calls from device memory (torch tensors as the caller's HBM)"""

    def __init__(self):
        import torch
        self.t = torch

    def up(self, b):
        return self.t.from_numpy(np.frombuffer(b + b"\0", np.uint8).copy()).cuda()

    def new(self, n, fill):
        return self.t.full((max(1, n),), fill, dtype=self.t.uint8, device="cuda")

    def down(self, t, n):
        return t.cpu().numpy().tobytes()[:n]


def _verify(eng, mem, ring, blob, n):
    if mem == "host":
        return eng.verify_spend_keyring(ring, blob, True)
    from act_amd import capi
    d = _Dev(); dp = d.up(blob); st, ok, kp = d.new(n, 99), d.new(n, 77), d.new(32 * n, 7)
    d.t.cuda.synchronize()
    eng.keyring_ptr("verify", ring, n, capi.MEM_DEVICE, proofs=dp.data_ptr(), status=st.data_ptr(), out_key=ok.data_ptr(), kprime=kp.data_ptr())
    return d.down(st, n), d.down(ok, n), d.down(kp, 32 * n)


def _sign(eng, mem, ring, kidx, kp, st_in, rng, mode):
    n = len(st_in)
    if mem == "host":
        return eng.refund_sign_keyring(ring, kidx, kp, st_in, rng, mode)
    from act_amd import capi
    d = _Dev(); ins = [d.up(x) for x in (kidx, kp, st_in, rng)]; out, st = d.new(128 * n, 7), d.new(n, 99)
    d.t.cuda.synchronize()
    eng.keyring_ptr("sign", ring, n, capi.MEM_DEVICE, key_index=ins[0].data_ptr(), kprime=ins[1].data_ptr(), status_in=ins[2].data_ptr(), rng=ins[3].data_ptr(),
                    rng_mode=mode, out=out.data_ptr(), status=st.data_ptr())
    return d.down(st, n), d.down(out, 128 * n)


@pytest.mark.parametrize("L,mode,mem", [(8, "host", "host"), (8, "host", "device"), (8, "device", "host"), (8, "device", "device"),
                                         (128, "host", "host"), (128, "device", "device"), (64, "device", "host")])
def test_ring_parity_through_the_c_abi(engine_factory, oracle, bench_params, L, mode, mem):
    from act_amd import capi
    eng = engine_factory(bench_params, L, max_batch=MB, transcript=capi.TRANSCRIPT_HOST if mode == "host" else capi.TRANSCRIPT_DEVICE)
    octx = oracle.ctx(bench_params, L)
    keys, names, proofs, prer = _keys_and_lanes(eng, octx, L, "gkr-%d" % L)
    a, b, c, d, e = keys
    blob = b"".join(proofs)
    per_key, kp_all = _oracle_table(octx, keys, proofs)
    assert [per_key[0][i] for i in range(8)] == [0, 7, 7, 7, 7, 7, 6, 255] and per_key[1][1] == 0 and per_key[2][2] == 0 and per_key[4][3] == 0
    rng = shake("gkr-rng-%d" % L, 128 * N)
    for ring_idx in ([0], [0, 1], [1, 0], [0, 1, 2, 3]):
        ring = [keys[i] for i in ring_idx]
        want_st, want_ok, want_kp = _want(per_key, kp_all, ring_idx, N)
        st, ok, kp = _verify(eng, mem, ring, blob, N)
        print("ring", ring_idx, "accepted", st.count(0), "of", N, "per key", [ok.count(k) for k in range(len(ring))])
        assert (st, ok, kp) == (want_st, want_ok, want_kp), ring_idx
        # ACT_SIGN_MATCHED: byte for byte PrivateKey::refund of the matched key over the lane's slice
        for rmode in (capi.RNG_PER_LANE, capi.RNG_SEQUENTIAL):
            st2, rf = _sign(eng, mem, ring, ok, kp, st, rng, rmode)
            assert st2 == want_st
            cur = 0
            for i in range(N):
                if want_st[i]:
                    assert rf[128 * i:128 * i + 128] == bytes(128); continue
                slot = i if rmode == capi.RNG_PER_LANE else cur
                cur += 1
                assert octx.refund(ring[want_ok[i]], proofs[i], rng[128 * slot:128 * slot + 128]) == (0, rf[128 * i:128 * i + 128]), (ring_idx, rmode, i)
        # a named key: the bytes of act_refund_sign_batch under it; the refund verifies under w[sign_key] and under no other ring key
        sk_i = len(ring) - 1
        st3, rf3 = _sign(eng, mem, ring, bytes([sk_i]) * N, kp, st, rng, capi.RNG_SEQUENTIAL)
        assert (st3, rf3) == eng.refund_sign(ring[sk_i], kp, st, rng, capi.RNG_SEQUENTIAL)
        for i in [j for j in range(N) if want_st[j] == 0][:6]:
            for k, sk in enumerate(ring):
                got = octx.refund_to_credit_token(prer[i], proofs[i], rf3[128 * i:128 * i + 128], sk[32:])[0]
                assert (got == 0) == (k == sk_i), (ring_idx, i, k, got)
        # an index outside the ring is the lane's verdict: 255, zero record, no slice consumed
        acc = [i for i in range(N) if want_st[i] == 0]
        bad = bytearray(ok); bad[acc[1]] = 200; bad[acc[4]] = len(ring)
        st4, rf4 = _sign(eng, mem, ring, bytes(bad), kp, st, rng, capi.RNG_SEQUENTIAL)
        cur = 0
        for i in range(N):
            if want_st[i] or i in (acc[1], acc[4]):
                assert st4[i] == (want_st[i] or 255) and rf4[128 * i:128 * i + 128] == bytes(128); continue
            assert st4[i] == 0 and octx.refund(ring[want_ok[i]], proofs[i], rng[128 * cur:128 * cur + 128])[1] == rf4[128 * i:128 * i + 128]
            cur += 1
    # nkeys == 1: verify + sign give the bytes of act_refund_batch
    st, ok, kp = _verify(eng, mem, [a], blob, N)
    assert _sign(eng, mem, [a], ok, kp, st, rng, capi.RNG_SEQUENTIAL) == eng.refund(a, blob, rng, capi.RNG_SEQUENTIAL)
    assert (st, kp) == eng.verify_spend(a, blob, True)
    # n = 0 and n = 1
    assert _verify(eng, mem, [b, a], b"", 0) == (b"", b"", b"")
    assert _verify(eng, mem, [b, a], proofs[0], 1) == (b"\0", b"\1", kp_all[0])
    assert _sign(eng, mem, [b, a], b"\1", kp_all[0], b"\0", rng, capi.RNG_PER_LANE) == (b"\0", octx.refund(a, proofs[0], rng[:128])[1])
    assert eng.secret_residue() == 0


def _redeem_lanes(eng, octx, L, tag):
    keys = kr.make_keys(octx, tag)
    a, b = keys[0], keys[1]
    lanes = [kr.spend_under(octx, (a, b, a, b, keys[4], a, b, a)[i], "%s-%d" % (tag, i))[0] for i in range(8)]
    t = bytearray(lanes[5]); t[33] ^= 1; lanes[5] = bytes(t)                   # tampered
    lanes += [lanes[0], lanes[1]]                                             # repeats inside the batch
    return keys, lanes


def _ring_loop(eng, octx, ring, sign_key, proofs, rng, spent):
    """the sequential loop of a server that tries its keys in ring order.  Signing with the matched key is the oracle's refund; a
    refund signed with ANOTHER key is something PrivateKey::refund cannot produce: there the contract is the bytes of the existing
    act_refund_sign_batch under keys[sign_key] over the oracle's K' and verdicts."""
    from act_amd import capi
    st_out, rf_out, ok_out, kp_out, cur = [], [], [], [], 0
    for p in proofs:
        st, m, kp = kr.oracle_ring_verdict(octx, ring, p)
        k = int.from_bytes(p[:32], "little") % ELL
        if st == 0 and k in spent:
            st = 3
        ok_out.append(m); kp_out.append(kp)
        if st:
            st_out.append(st); rf_out.append(bytes(128)); continue
        spent.add(k)
        s2, rf = octx.refund(ring[m], p, rng[128 * cur:128 * cur + 128]); cur += 1
        assert s2 == 0
        st_out.append(0); rf_out.append(rf)
    if sign_key >= 0:
        st2, rf2 = eng.refund_sign(ring[sign_key], b"".join(kp_out), bytes(st_out), rng, capi.RNG_SEQUENTIAL)
        assert st2 == bytes(st_out)
        return bytes(st_out), rf2, bytes(ok_out), cur
    return bytes(st_out), b"".join(rf_out), bytes(ok_out), cur


@pytest.mark.parametrize("mode", ["host", "device"])
def test_ring_redeem(engine_factory, oracle, bench_params, mode):
    from act_amd import capi
    L = 8
    eng = engine_factory(bench_params, L, max_batch=MB, transcript=capi.TRANSCRIPT_HOST if mode == "host" else capi.TRANSCRIPT_DEVICE)
    octx = oracle.ctx(bench_params, L)
    keys, lanes = _redeem_lanes(eng, octx, L, "gkr-rd")
    a, b = keys[0], keys[1]
    blob = b"".join(lanes); n = len(lanes)
    rng = shake("gkr-rd-rng", 128 * n)
    for sign_key in (-1, 0):
        want = _ring_loop(eng, octx, [b, a], sign_key, lanes, rng, set())
        assert list(want[0]) == [0, 0, 0, 0, 7, 7, 0, 0, 3, 3] and list(want[2]) == [1, 0, 1, 0, 255, 255, 0, 1, 1, 0]
        ns = capi.NullifierSet(1000)
        assert eng.redeem_keyring(ns, [b, a], blob, rng, capi.RNG_SEQUENTIAL, sign_key) == want[:3]
        assert len(ns) == 6
        # everything again: double spends keep the index they matched
        st, rf, ok = eng.redeem_keyring(ns, [b, a], blob, rng, capi.RNG_SEQUENTIAL, sign_key)
        assert st == bytes(3 if v == 0 else v for v in want[0]) and not any(rf) and ok == want[2]
        ns.close()
        # the generator itself (ACT_RNG_CALLBACK): drawn once, for the signed lanes
        ns = capi.NullifierSet(1000)
        g = capi.ReplayRng(rng)
        assert eng.redeem_keyring(ns, [b, a], blob, g, capi.RNG_CALLBACK, sign_key) == want[:3]
        ns.close()
        # device memory
        d = _Dev(); ns = capi.NullifierSet(1000)
        dp, dr = d.up(blob), d.up(rng); out, st, ok = d.new(128 * n, 7), d.new(n, 99), d.new(n, 77)
        d.t.cuda.synchronize()
        eng.keyring_ptr("redeem", [b, a], n, capi.MEM_DEVICE, set=ns, sign_key=sign_key, proofs=dp.data_ptr(), rng=dr.data_ptr(), rng_mode=capi.RNG_SEQUENTIAL,
                        out=out.data_ptr(), status=st.data_ptr(), out_key=ok.data_ptr())
        assert (d.down(st, n), d.down(out, 128 * n), d.down(ok, n)) == want[:3]
        ns.close()
    # across entry points: redeemed once under key a through the one-key call, then through the ring -- and the other way round
    ns = capi.NullifierSet(1000)
    assert eng.redeem(ns, a, lanes[0], rng, capi.RNG_SEQUENTIAL)[0] == b"\0"
    st, rf, ok = eng.redeem_keyring(ns, [b, a], lanes[0] + lanes[1], rng, capi.RNG_SEQUENTIAL)
    assert (st, ok) == (b"\3\0", b"\1\0") and rf[:128] == bytes(128) and rf[128:] == octx.refund(b, lanes[1], rng[:128])[1]
    assert eng.redeem(ns, b, lanes[1], rng, capi.RNG_SEQUENTIAL) == (b"\3", bytes(128))
    ns.close()
    # nkeys == 1: the bytes of act_redeem_batch
    ns1, ns2 = capi.NullifierSet(1000), capi.NullifierSet(1000)
    one = eng.redeem(ns1, a, blob, rng, capi.RNG_SEQUENTIAL)
    assert eng.redeem_keyring(ns2, [a], blob, rng, capi.RNG_SEQUENTIAL)[:2] == one and len(ns1) == len(ns2)
    ns1.close(); ns2.close()
    # the signature step fails after the nullifiers were recorded: RECORDED_UNSIGNED exactly on the lanes the one-key call marks
    marks = []
    for ring_call in (False, True):
        ns = capi.NullifierSet(1000)
        assert eng.lib.act_debug_fail_next_signs(eng.ctx, 1) == 0
        if ring_call:
            rc, st, rf, ok = eng.redeem_keyring(ns, [a], blob, rng, capi.RNG_SEQUENTIAL, raw=True)
        else:
            stb = np.zeros(n, np.uint8); out = np.full(128 * n, 7, np.uint8)
            args = [np.frombuffer(x, np.uint8) for x in (a, blob, rng)]
            rc = eng.lib.act_redeem_batch(eng.ctx, ns.h, n, capi.MEM_HOST, args[0].ctypes.data, args[1].ctypes.data, args[2].ctypes.data, capi.RNG_SEQUENTIAL,
                                          out.ctypes.data, stb.ctypes.data)
            st, rf = stb.tobytes(), out.tobytes()
        assert rc != 0 and not any(rf) and st.count(251) == len(ns) > 0
        marks.append(st)
        ns.close()
    assert marks[0] == marks[1]
    assert eng.secret_residue() == 0


def test_ring_redeem_on_wire_bytes(engine_factory, oracle, bench_params):
    from act_amd import capi
    L = 8
    eng = engine_factory(bench_params, L, max_batch=MB, transcript=capi.TRANSCRIPT_DEVICE)
    octx = oracle.ctx(bench_params, L)
    keys, lanes = _redeem_lanes(eng, octx, L, "gkr-rd")
    a, b = keys[0], keys[1]
    rng = shake("gkr-w-rng", 128 * 32)
    msgs = eng.cbor_encode("SpendProof", b"".join(lanes))
    # wire form = record form + framing
    ns1, ns2 = capi.NullifierSet(1000), capi.NullifierSet(1000)
    st, rf, ok = eng.redeem_keyring(ns1, [b, a], b"".join(lanes), rng, capi.RNG_SEQUENTIAL)
    stw, out, okw = eng.redeem_cbor_keyring(ns2, [b, a], msgs, rng, capi.RNG_SEQUENTIAL)
    framed = eng.cbor_encode("Refund", rf)
    assert (stw, okw) == (st, ok) and out == [framed[i] if st[i] == 0 else b"" for i in range(len(lanes))]
    ns1.close(); ns2.close()
    # malformed, structurally wrong, non-canonical-but-valid and invalid-value messages: the statuses act_redeem_cbor_batch gives
    odd = list(msgs[:6])
    odd[1] = odd[1][:-5]                                        # truncated
    odd[2] = b"\x83\x01\x02\x03"                                # not a map
    odd[3] = b"\xff" + odd[3][1:]                               # a break where the map should start
    pos = odd[4].find(lanes[4][64:96]); v = bytearray(odd[4]); v[pos:pos + 32] = b"\xff" * 32; odd[4] = bytes(v)      # A' not canonical: InvalidValue
    odd.append(b"")
    nsa, nsb, nsr = capi.NullifierSet(1000), capi.NullifierSet(1000), capi.NullifierSet(1000)
    one_a = eng.redeem_cbor(nsa, a, odd, rng, capi.RNG_PER_LANE)
    one_b = eng.redeem_cbor(nsb, b, odd, rng, capi.RNG_PER_LANE)
    stw, out, okw = eng.redeem_cbor_keyring(nsr, [b, a], odd, rng, capi.RNG_PER_LANE)
    print("wire statuses", list(stw), "one-key a", list(one_a[0]), "one-key b", list(one_b[0]))
    for i in range(len(odd)):
        if one_a[0][i] in (253, 254, 255):
            assert stw[i] == one_a[0][i] == one_b[0][i] and okw[i] == 255 and out[i] == b""
        else:
            want = (0, 1, one_a[1][i]) if one_a[0][i] == 0 else (0, 0, one_b[1][i]) if one_b[0][i] == 0 else (7, 255, b"")
            assert (stw[i], okw[i], out[i]) == want, i
    assert any(s in (253, 254) for s in stw) and 255 in stw
    # nkeys == 1 on wire bytes: the bytes of act_redeem_cbor_batch
    ns1, ns2 = capi.NullifierSet(1000), capi.NullifierSet(1000)
    assert eng.redeem_cbor_keyring(ns2, [a], odd, rng, capi.RNG_SEQUENTIAL)[:2] == eng.redeem_cbor(ns1, a, odd, rng, capi.RNG_SEQUENTIAL)
    for s in (nsa, nsb, nsr, ns1, ns2):
        s.close()
    assert eng.secret_residue() == 0


@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)])
def test_ring_over_a_node(engine_factory, oracle, bench_params, devices):
    from act_amd import capi
    L = 8
    eng = engine_factory(bench_params, L, max_batch=MB, transcript=capi.TRANSCRIPT_DEVICE)
    octx = oracle.ctx(bench_params, L)
    keys, names, proofs, prer = _keys_and_lanes(eng, octx, L, "gkr-8")
    ring = [keys[1], keys[0], keys[2]]
    blob = b"".join(proofs)
    rng = shake("gkr-node-rng", 128 * N)
    node = capi.Node(bench_params, L, devices=devices, max_batch=7, transcript=capi.TRANSCRIPT_DEVICE)
    ns, nn = capi.NullifierSet(4000), capi.NodeNullifierSet(4000, devices=(0, 0))
    try:
        st, ok, kp = eng.verify_spend_keyring(ring, blob, True)
        assert node.verify_spend_keyring(ring, blob, True) == (st, ok, kp)
        for rmode in (capi.RNG_PER_LANE, capi.RNG_SEQUENTIAL):
            assert node.refund_sign_keyring(ring, ok, kp, st, rng, rmode) == eng.refund_sign_keyring(ring, ok, kp, st, rng, rmode)
        two = blob + proofs[0] + proofs[1]
        want = eng.redeem_keyring(ns, ring, two, rng, capi.RNG_SEQUENTIAL, 2)
        assert node.redeem_keyring(nn, ring, two, rng, capi.RNG_SEQUENTIAL, 2) == want and len(nn) == len(ns)
        assert want[0][-2:] == b"\3\3" and want[2][-2:] == want[2][:2] == b"\1\0"
        msgs = eng.cbor_encode("SpendProof", blob)
        msgs[3] = msgs[3][:-2]; msgs[9] = b"\x83\x01\x02\x03"
        ns2, nn2 = capi.NullifierSet(4000), capi.NodeNullifierSet(4000, devices=(0, 0))
        assert node.redeem_cbor_keyring(nn2, ring, msgs, capi.ReplayRng(rng), capi.RNG_CALLBACK) == eng.redeem_cbor_keyring(ns2, ring, msgs, capi.ReplayRng(rng), capi.RNG_CALLBACK)
        ns2.close(); nn2.close()
    finally:
        ns.close(); nn.close(); node.close()


def test_ring_hygiene(engine_factory, oracle, bench_params):
    from act_amd import capi
    L = 8
    eng = engine_factory(bench_params, L, max_batch=MB, transcript=capi.TRANSCRIPT_HOST)
    octx = oracle.ctx(bench_params, L)
    keys = kr.make_keys(octx, "gkr-hy")
    a, b = keys[0], keys[1]
    pa, pb_ = kr.spend_under(octx, a, "gkr-hy-a")[0], kr.spend_under(octx, b, "gkr-hy-b")[0]
    assert eng.verify_spend(a, pa + pb_) == b"\0\7"                    # the one-key call caches key a
    assert eng.verify_spend_keyring([b, a], pa + pb_) == (b"\0\0", b"\1\0")
    # rejected rings: a w that is not a canonical encoding, nkeys out of range -- nothing of them stays, the cached keys stay usable
    badw = b[:32] + b"\xff" * 32
    with pytest.raises(capi.ActError):
        eng.verify_spend_keyring([a, badw], pa + pb_)
    for ring in ([], [a] * 5):
        st = np.zeros(2, np.uint8); ok = np.zeros(2, np.uint8); pr = np.frombuffer(pa + pb_, np.uint8); kb = np.frombuffer(b"".join(ring) + b"\0", np.uint8)
        assert eng.lib.act_verify_spend_keyring_batch(eng.ctx, 2, capi.MEM_HOST, kb.ctypes.data, len(ring), pr.ctypes.data, st.ctypes.data, ok.ctypes.data, None) == 1
    ns = capi.NullifierSet(100)
    for sign_key in (-2, 2):
        assert eng.redeem_keyring(ns, [b, a], pa + pb_, shake("hy", 256), capi.RNG_PER_LANE, sign_key, raw=True)[0] == 1
    assert len(ns) == 0
    assert eng.verify_spend(a, pa + pb_) == b"\0\7"
    assert eng.verify_spend_keyring([b, a], pa + pb_) == (b"\0\0", b"\1\0")
    st, rf, ok = eng.redeem_keyring(ns, [b, a], pa + pb_, shake("hy", 256), capi.RNG_PER_LANE)
    assert st == b"\0\0" and rf[:128] == octx.refund(a, pa, shake("hy", 256)[:128])[1]
    ns.close()
    assert eng.secret_residue() == 0


def test_keyring_api_round_trip():
    """issue under a and b, spend, redeem the wire messages against the ring [b, a] signing with b (the new key), client
    to_credit_token under the key index returned, second spend of the new token."""
    from act_amd import api
    params = api.Params.new("test-org", "test-service", "test", "2024-01-01")
    rng = api.ByteStreamRng(shake("gkr-api", 1 << 20))
    a, b = api.PrivateKey.random(rng, params), api.PrivateKey.random(rng, params)
    ring = api.Keyring([b, a])
    toks = []
    for sk in (a, b, a):
        pre = api.PreIssuance.random(rng, params); req = pre.request(params, rng)
        toks.append(pre.to_credit_token(params, sk.public(), req, sk.issue(params, req, 20, rng)))
    spends = [t.prove_spend(params, 5, rng) for t in toks]
    proofs = [p for p, _ in spends]
    assert ring.verify_spend_batch(params, proofs) == (bytes(3), [1, 0, 1])
    db = api.NullifierDb(1000)
    out, idx = ring.redeem_cbor_batch(params, db, [p.to_cbor(params) for p in proofs], rng, sign_with=0)
    assert idx == [1, 0, 1] and all(isinstance(m, bytes) for m in out)
    new = [spends[i][1].to_credit_token(params, proofs[i], api.Refund.from_cbor(out[i], params), ring.public(0)) for i in range(3)]
    with pytest.raises(api.Error):
        spends[0][1].to_credit_token(params, proofs[0], api.Refund.from_cbor(out[0], params), ring.public(1))
    # the second spend: every client is on key b now; the old proofs are double spends
    again = [t.prove_spend(params, 7, rng) for t in new]
    refunds, idx2 = ring.redeem_batch(params, db, [p for p, _ in again] + [proofs[0]], rng)
    assert idx2 == [0, 0, 0, 1] and isinstance(refunds[3], api.Error) and refunds[3].code == 3
    for i in range(3):
        assert api.scalar_to_u128(again[i][1].to_credit_token(params, again[i][0], refunds[i], ring.public(idx2[i])).credits()) == 8
    res, idx3 = ring.refund_batch(params, [p for p, _ in again], rng, sign_with=None)
    assert idx3 == [0, 0, 0] and all(isinstance(r, api.Refund) for r in res)
