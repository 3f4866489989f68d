"""Issuance on wire bytes (act_issue_cbor_batch, act_issue_check_cbor_batch, act_issue_sign_cbor_batch and their node forms): the
issuer's other endpoint as a server built on the crate runs it --

    let req  = IssuanceRequest::from_cbor(&msg)?;                       // src/cbor.rs:118-148
    let resp = private_key.issue(&params, &req, c, &mut rng)?;          // src/lib.rs:621-663
    resp.to_cbor()                                                      // src/cbor.rs:162-175

-- as one call over a batch, compared lane by lane with that loop restated: the Python model's from_cbor, the C oracle's issue fed the
rng slice the sequential loop would have handed it, the Python model's to_cbor.  Canonical messages, every spelling of
tests/test_cbor.py's _variants, tampered proofs, an undecodable K, trailing bytes, every rng convention, host and device memory, both
transcript modes, several chunks, the tiny road and its fallback, more than one settle window, the halves, the node handle."""
import ctypes as C

import numpy as np
import pytest

import pymodel as m
from conftest import shake, scb
from test_cbor import _variants

pytestmark = pytest.mark.gpu

WIRE = {1: 254, 2: 253, 3: 255}       # CborError::{Ciborium, InvalidStructure, InvalidValue} as lane statuses
RESP = 176                            # act_cbor_size(ctx, ACT_CBOR_ISSUANCE_RESPONSE)


def _requests(eng, n, tag):
    pre = eng.pre_issuance_random(shake(tag + "-pre", 128 * n))
    return eng.request(pre, shake(tag + "-rq", 128 * n))


def _messages(eng, n, tag):
    req = _requests(eng, n, tag)
    recs = [bytearray(req[128 * i:128 * i + 128]) for i in range(n)]
    recs[2][32] ^= 1                                    # gamma            -> 1
    recs[3][64] ^= 1                                    # k_bar            -> 1
    recs[4][0:32] = b"\xff" * 32                        # K undecodable    -> 255 (CborError::InvalidValue)
    r = int.from_bytes(recs[6][96:128], "little") + m.ELL
    recs[6][96:128] = r.to_bytes(32, "little")          # r_bar + l on the wire: from_cbor reduces it -> accepted
    msgs = [bytes(x) for x in _encode(eng, b"".join(bytes(x) for x in recs))]
    msgs[5] = msgs[5] + b"\x00\x07\xff"                 # bytes after the first item are not read
    for i in (0, 1):                                    # every spelling, canonical or not, broken or not, of two valid requests
        msgs += [v for v, _ in _variants("IssuanceRequest", bytes(recs[i]), 128)]
    return msgs


def _encode(eng, recs):
    return eng.cbor_encode("IssuanceRequest", recs)


def _loop(octx, sk, msgs, cs, stream, per_lane=False):
    """the server loop, one generator (or lane i's own slice): statuses, IssuanceResponse messages, bytes drawn, from_cbor's requests"""
    st, out, reqs, cur = [], [], [], 0
    for i, msg in enumerate(msgs):
        es, rec = m.cbor_decode("IssuanceRequest", msg, 128)
        if es:
            st.append(WIRE[es]); out.append(b""); reqs.append(bytes(128)); continue
        rng = stream[128 * i:128 * i + 128] if per_lane else stream[128 * cur:128 * cur + 128]
        v, resp = octx.issue(sk, rec, cs[32 * i:32 * i + 32], rng)
        if v:
            st.append(v); out.append(b""); reqs.append(bytes(128)); continue
        cur += 1
        st.append(0); out.append(m.cbor_encode("IssuanceResponse", resp, 128)); reqs.append(bytes(rec))
    return bytes(st), out, 128 * cur, b"".join(reqs)


def _amounts(n, tag):
    return b"".join(scb(int.from_bytes(shake("%s-c%d" % (tag, i), 16), "little")) for i in range(n))


def _raw_issue(eng, sk, msgs, cs, rng_ptr, rng_mode, offsets=True):
    """act_issue_cbor_batch with its return code, statuses and every output byte (slots of failed lanes included)"""
    from act_amd import capi
    n = len(msgs)
    blob = np.frombuffer(b"".join(msgs) + b"\0", np.uint8)
    offs = np.zeros(n + 1, np.uint64); offs[1:] = np.cumsum([len(x) for x in msgs], dtype=np.uint64)
    cc = np.frombuffer(cs, np.uint8)
    st = np.full(n, 99, np.uint8); out = np.full(RESP * n, 7, np.uint8); sk_a = np.frombuffer(sk, np.uint8)
    rc = eng.lib.act_issue_cbor_batch(eng.ctx, n, capi.MEM_HOST, sk_a.ctypes.data, blob.ctypes.data, offs.ctypes.data if offsets else None,
                                      cc.ctypes.data, rng_ptr, rng_mode, out.ctypes.data, st.ctypes.data)
    return rc, st.tobytes(), out.tobytes()


def _flat(out):
    return b"".join(x if x else bytes(RESP) for x in out)


@pytest.mark.parametrize("max_batch", [4, 64])
def test_issue_on_wire_bytes_equals_the_server_loop(engine_factory, oracle, bench_params, max_batch):
    from act_amd import capi
    eng = engine_factory(bench_params, 8, max_batch=max_batch)          # (issuance does not depend on L; 4: many chunks)
    sk = eng.private_key_random(shake("iw-sk", 64))
    octx = oracle.ctx(bench_params, 8)
    n = 12
    msgs = _messages(eng, n, "iw")
    N = len(msgs)
    cs = _amounts(N, "iw")
    stream = shake("iw-rng", 128 * N)
    want_st, want_out, drawn, want_req = _loop(octx, sk, msgs, cs, stream)
    want_pl = _loop(octx, sk, msgs, cs, stream, per_lane=True)
    assert {0, 1, 253, 254, 255}.issubset(set(want_st)) and want_st.count(0) > n
    assert eng.cbor_size("IssuanceResponse") == RESP and all(len(x) in (0, RESP) for x in want_out)
    for mode in (capi.TRANSCRIPT_HOST, capi.TRANSCRIPT_DEVICE):
        eng.set_transcript_mode(mode)
        # the generator itself: drawn once, after every verdict, exactly what the loop drew
        g = capi.ReplayRng(stream)
        st, out = eng.issue_cbor(sk, msgs, cs, g, capi.RNG_CALLBACK)
        assert st == want_st, [(i, st[i], want_st[i]) for i in range(N) if st[i] != want_st[i]]
        assert out == want_out and g.draws == [drawn] and g.pos == drawn
        assert eng.secret_residue() == 0
        # the same bytes pre-drawn, and lane i's own slice
        assert eng.issue_cbor(sk, msgs, cs, stream, capi.RNG_SEQUENTIAL) == (want_st, want_out)
        assert eng.secret_residue() == 0
        assert eng.issue_cbor(sk, msgs, cs, stream, capi.RNG_PER_LANE) == want_pl[:2]
        assert eng.secret_residue() == 0
        # every slot of a lane that was not signed is zero (raw call: the binding's b"" hides the slot)
        rc, st, flat = _raw_issue(eng, sk, msgs, cs, np.frombuffer(stream, np.uint8).ctypes.data, capi.RNG_SEQUENTIAL)
        assert rc == 0 and st == want_st and flat == _flat(want_out)
        # offsets = NULL: canonical-size messages back to back
        canon = [x for x in msgs[:n] if len(x) == 141]
        cw = _loop(octx, sk, canon, cs, stream)
        rc, st, flat = _raw_issue(eng, sk, canon, cs[:32 * len(canon)], np.frombuffer(stream, np.uint8).ctypes.data, capi.RNG_SEQUENTIAL, offsets=False)
        assert rc == 0 and (st, flat) == (cw[0], _flat(cw[1]))
        # one message per call, and a few with per-lane slices: the tiny road (unframed on the host, one kernel); a non-canonical message
        # among them sends the whole call down the general path
        for i in (0, 2, 4, 5, n + 3, N - 1):
            assert eng.issue_cbor(sk, [msgs[i]], cs[32 * i:32 * i + 32], stream[:128], capi.RNG_SEQUENTIAL) == \
                _loop(octx, sk, [msgs[i]], cs[32 * i:32 * i + 32], stream)[:2], i
        k = min(4, max_batch)
        assert eng.issue_cbor(sk, msgs[:k], cs[:32 * k], stream[:128 * k], capi.RNG_PER_LANE) == _loop(octx, sk, msgs[:k], cs, stream, per_lane=True)[:2]
        mixed = [msgs[1], msgs[n + 4], msgs[0], msgs[6]]
        mc = cs[32:64] + cs[32 * (n + 4):32 * (n + 5)] + cs[:32] + cs[192:224]
        assert eng.issue_cbor(sk, mixed, mc, stream[:512], capi.RNG_PER_LANE) == _loop(octx, sk, mixed, mc, stream, per_lane=True)[:2]
        # the halves: verdict + the request as from_cbor returns it, then sign + frame
        stv, req = eng.issue_check_cbor(msgs)
        assert stv == want_st and req == want_req
        assert eng.issue_sign_cbor(sk, req, cs, stv, stream, capi.RNG_SEQUENTIAL) == (want_st, want_out)
        g = capi.ReplayRng(stream)
        assert eng.issue_sign_cbor(sk, req, cs, stv, g, capi.RNG_CALLBACK) == (want_st, want_out) and g.draws == [drawn]
        assert eng.secret_residue() == 0
        # the three-call composition on canonical input gives the same bytes
        cst, crec = eng.cbor_decode("IssuanceRequest", canon)
        ist, iresp = eng.issue(sk, crec, cs[:32 * len(canon)], stream, capi.RNG_SEQUENTIAL)
        enc = eng.cbor_encode("IssuanceResponse", iresp)
        comp = [enc[i] if ist[i] == 0 and cst[i] == 0 else b"" for i in range(len(canon))]
        assert eng.issue_cbor(sk, canon, cs[:32 * len(canon)], stream, capi.RNG_SEQUENTIAL) == (bytes(WIRE[a] if a else b for a, b in zip(cst, ist)), comp)
    # a generator that fails: ACT_ERR_RNG, nothing signed, every slot zero
    g = capi.ReplayRng(stream[:drawn - 1])
    rc, st, flat = _raw_issue(eng, sk, msgs, cs, g.ptr, capi.RNG_CALLBACK)
    assert rc == 5 and flat == bytes(RESP * N) and st == want_st and g.pos == 0
    assert eng.secret_residue() == 0
    assert eng.issue_cbor(sk, [], b"", stream) == (b"", [])


def test_issue_on_wire_bytes_in_device_memory(engine_factory, oracle, bench_params):
    import torch
    from act_amd import capi
    eng = engine_factory(bench_params, 8, max_batch=4)
    sk = eng.private_key_random(shake("iwd-sk", 64))
    octx = oracle.ctx(bench_params, 8)
    msgs = _messages(eng, 10, "iwd")
    N = len(msgs)
    cs = _amounts(N, "iwd")
    stream = shake("iwd-rng", 128 * N)
    want_st, want_out, drawn, want_req = _loop(octx, sk, msgs, cs, stream)
    want_pl = _loop(octx, sk, msgs, cs, stream, per_lane=True)
    blob = b"".join(msgs)
    offs = np.zeros(N + 1, np.uint64); offs[1:] = np.cumsum([len(x) for x in msgs], dtype=np.uint64)
    d = lambda b: torch.from_numpy(np.frombuffer(b, np.uint8).copy()).cuda()
    d_blob, d_rng, d_c = d(blob + b"\0"), d(stream), d(cs)
    d_st = torch.full((N,), 99, dtype=torch.uint8, device="cuda"); d_out = torch.full((RESP * N,), 9, dtype=torch.uint8, device="cuda")
    host = lambda t: t.cpu().numpy().tobytes()
    for mode in (capi.TRANSCRIPT_HOST, capi.TRANSCRIPT_DEVICE):
        eng.set_transcript_mode(mode)
        for rng_mode, rng_ptr, want in ((capi.RNG_SEQUENTIAL, d_rng.data_ptr(), (want_st, want_out)), (capi.RNG_PER_LANE, d_rng.data_ptr(), want_pl[:2])):
            d_st.fill_(99); d_out.fill_(9); torch.cuda.synchronize()
            eng.issue_cbor_ptr(sk, N, capi.MEM_DEVICE, d_blob.data_ptr(), offs.ctypes.data, d_c.data_ptr(), rng_ptr, rng_mode, d_out.data_ptr(), d_st.data_ptr())
            assert (host(d_st), host(d_out)) == (want[0], _flat(want[1])), rng_mode
            assert eng.secret_residue() == 0
        g = capi.ReplayRng(stream)
        d_st.fill_(99); d_out.fill_(9); torch.cuda.synchronize()
        eng.issue_cbor_ptr(sk, N, capi.MEM_DEVICE, d_blob.data_ptr(), offs.ctypes.data, d_c.data_ptr(), g.ptr, capi.RNG_CALLBACK, d_out.data_ptr(), d_st.data_ptr())
        assert (host(d_st), host(d_out)) == (want_st, _flat(want_out)) and g.draws == [drawn]
        # the halves in device memory
        d_req = torch.full((128 * N,), 5, dtype=torch.uint8, device="cuda"); d_st2 = torch.full((N,), 99, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        eng.issue_check_cbor_ptr(N, capi.MEM_DEVICE, d_blob.data_ptr(), offs.ctypes.data, d_st2.data_ptr(), d_req.data_ptr())
        assert host(d_st2) == want_st and host(d_req) == want_req
        d_out.fill_(9); torch.cuda.synchronize()
        eng.issue_sign_cbor_ptr(sk, N, capi.MEM_DEVICE, d_req.data_ptr(), d_c.data_ptr(), d_st2.data_ptr(), d_rng.data_ptr(), capi.RNG_SEQUENTIAL,
                                d_out.data_ptr(), d_st.data_ptr())
        assert (host(d_st), host(d_out)) == (want_st, _flat(want_out))
    # canonical messages back to back, offsets = NULL
    canon = [x for x in msgs[:10] if len(x) == 141]
    cw = _loop(octx, sk, canon, cs, stream)
    d_cb = d(b"".join(canon))
    d_st.fill_(99); d_out.fill_(9); torch.cuda.synchronize()
    eng.issue_cbor_ptr(sk, len(canon), capi.MEM_DEVICE, d_cb.data_ptr(), 0, d_c.data_ptr(), d_rng.data_ptr(), capi.RNG_SEQUENTIAL, d_out.data_ptr(), d_st.data_ptr())
    assert host(d_st)[:len(canon)] == cw[0] and host(d_out)[:RESP * len(canon)] == _flat(cw[1])
    assert eng.secret_residue() == 0


def test_settle_windows_and_sparse_non_canonical_requests(engine_factory, oracle, bench_params):
    """More non-canonical messages than one settle window (4 096), and two far apart in a device-memory batch."""
    import torch
    from act_amd import capi
    eng = engine_factory(bench_params, 8, max_batch=4096)
    sk = eng.private_key_random(shake("isw-sk", 64))
    octx = oracle.ctx(bench_params, 8)
    n = 6000
    canon = _encode(eng, _requests(eng, n, "isw"))
    loose = [b"\xbf" + c[1:] + b"\xff" for c in canon]                 # indefinite-length map: same content, not canonical
    cs = _amounts(n, "isw")
    stream = shake("isw-rng", 128 * n)
    eng.set_transcript_mode(capi.TRANSCRIPT_DEVICE)
    st_c, out_c = eng.issue_cbor(sk, canon, cs, stream, capi.RNG_PER_LANE)
    assert st_c == bytes(n)
    for i in (0, 1, 4095, 4096, n - 1):                                 # the canonical path against the loop, a few lanes
        assert [out_c[i]] == _loop(octx, sk, [canon[i]], cs[32 * i:32 * i + 32], stream[128 * i:128 * i + 128])[1], i
    # every message non-canonical: two settle windows, the same responses (per-lane slices: the same bytes per lane)
    assert eng.issue_cbor(sk, loose, cs, stream, capi.RNG_PER_LANE) == (st_c, out_c)
    assert eng.issue_cbor(sk, loose, cs, stream, capi.RNG_SEQUENTIAL) == eng.issue_cbor(sk, canon, cs, stream, capi.RNG_SEQUENTIAL)
    stv, req = eng.issue_check_cbor(loose)
    assert (stv, req) == eng.issue_check_cbor(canon)
    # device memory, two non-canonical messages at the two ends
    msgs = list(canon); msgs[0] = loose[0]; msgs[n - 1] = loose[n - 1]
    blob = b"".join(msgs)
    offs = np.zeros(n + 1, np.uint64); offs[1:] = np.cumsum([len(x) for x in msgs], dtype=np.uint64)
    d = lambda b: torch.from_numpy(np.frombuffer(b, np.uint8).copy()).cuda()
    d_blob, d_rng, d_c = d(blob), d(stream), d(cs)
    d_st = torch.full((n,), 99, dtype=torch.uint8, device="cuda"); d_out = torch.full((RESP * n,), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eng.issue_cbor_ptr(sk, n, capi.MEM_DEVICE, d_blob.data_ptr(), offs.ctypes.data, d_c.data_ptr(), d_rng.data_ptr(), capi.RNG_PER_LANE, d_out.data_ptr(), d_st.data_ptr())
    assert d_st.cpu().numpy().tobytes() == st_c and d_out.cpu().numpy().tobytes() == b"".join(out_c)
    assert eng.secret_residue() == 0


@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)])
def test_issue_wire_calls_through_the_node(oracle, bench_params, devices):
    from act_amd import capi
    eng_msgs = capi.Engine(bench_params, 8, device=0, max_batch=64)
    try:
        sk = eng_msgs.private_key_random(shake("iwn-sk", 64))
        msgs = _messages(eng_msgs, 11, "iwn")
    finally:
        eng_msgs.close()
    octx = oracle.ctx(bench_params, 8)
    N = len(msgs)
    cs = _amounts(N, "iwn")
    stream = shake("iwn-rng", 128 * N)
    want_st, want_out, drawn, want_req = _loop(octx, sk, msgs, cs, stream)
    want_pl = _loop(octx, sk, msgs, cs, stream, per_lane=True)
    node = capi.Node(bench_params, 8, devices=devices, max_batch=3)
    try:
        for mode in (capi.TRANSCRIPT_HOST, capi.TRANSCRIPT_DEVICE):
            node.set_transcript_mode(mode)
            g = capi.ReplayRng(stream)
            assert node.issue_cbor(sk, msgs, cs, g, capi.RNG_CALLBACK) == (want_st, want_out) and g.draws == [drawn]
            assert node.issue_cbor(sk, msgs, cs, stream, capi.RNG_SEQUENTIAL) == (want_st, want_out)
            assert node.issue_cbor(sk, msgs, cs, stream, capi.RNG_PER_LANE) == want_pl[:2]
            stv, req = node.issue_check_cbor(msgs)
            assert (stv, req) == (want_st, want_req)
            g = capi.ReplayRng(stream)
            assert node.issue_sign_cbor(sk, req, cs, stv, g, capi.RNG_CALLBACK) == (want_st, want_out) and g.pos == drawn
        for i in (0, 1, 4, N - 1):
            assert node.issue_cbor(sk, [msgs[i]], cs[32 * i:32 * i + 32], stream[:128], capi.RNG_SEQUENTIAL) == \
                _loop(octx, sk, [msgs[i]], cs[32 * i:32 * i + 32], stream)[:2]
        g = capi.ReplayRng(stream[:drawn - 1])
        with pytest.raises(capi.ActError):
            node.issue_cbor(sk, msgs, cs, g, capi.RNG_CALLBACK)
        for k in range(len(devices)):
            n_res = C.c_size_t(0)
            assert node.lib.act_debug_secret_residue(node.lib.act_node_ctx(node.nd, k), C.byref(n_res)) == 0 and n_res.value == 0
    finally:
        node.close()


def test_issue_cbor_batch_through_the_api_mirror(bench_params):
    import act_amd
    from act_amd.api import ByteStreamRng, CborError, Error
    params = act_amd.Params(bench_params)
    e = params.engine(128)
    sk = act_amd.PrivateKey(e.private_key_random(shake("iwa-sk", 64)))
    msgs = _messages(e, 8, "iwa")[:10]
    cs = [5 + i for i in range(len(msgs))]
    rng = ByteStreamRng(shake("iwa-rng", 128 * len(msgs)))
    res = sk.issue_cbor_batch(params, msgs, cs, rng)
    st, out = e.issue_cbor(sk.record, msgs, b"".join(scb(c) for c in cs), shake("iwa-rng", 128 * len(msgs)), 1)
    for i, r in enumerate(res):
        if st[i] == 0:
            assert r == out[i]
        else:
            assert isinstance(r, CborError if st[i] in (253, 254, 255) else Error)
    assert rng.pos == 128 * st.count(0)
