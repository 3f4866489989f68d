"""Respelled IssuanceRequest messages are read on the GPU (csrc/issue_wire_lanes.h, k_issue_wire_flag, k_cbor_read_raw,
k_issue_a_wire_read): act_issue_check_cbor_batch and act_issue_cbor_batch under both reader settings (act_ctx_set_wire_reader) against
each other and against the server loop restated (tests/test_gpu_issue_wire.py), from host and device memory, under every rng
convention; where the messages were read (act_ctx_wire_stats, act_prof_*); a failing generator; the node.

Shapes: L = 8 (issuance does not depend on L), (max_batch, n) = (4, 11): three chunks alternating over both slots, the last one ragged
(3), and 11 > max_batch keeps the call off the tiny road; (256, 200): one chunk of four waves whose last wave has 8 lanes."""
import ctypes as C

import numpy as np
import pytest

import pymodel as m
from conftest import shake
from test_gpu_issue_wire import RESP, _amounts, _encode, _flat, _loop, _raw_issue, _requests

pytestmark = pytest.mark.gpu

SHAPES = [(4, 11), (256, 200)]
BAD_PT = b"\x01" + bytes(31)
bstr = lambda b: b"\x58\x20" + b


def _ents(rec):
    return [(k + 1, bstr(rec[32 * k:32 * k + 32])) for k in range(4)]


def _body(es):
    return b"".join(m._cbor_head(0, k) + v for k, v in es)


def _tamper(rec):
    r = bytearray(rec); r[32] ^= 1                              # gamma: the proof of knowledge fails -> status 1
    return bytes(r)


def _unreduced(rec):
    r = int.from_bytes(rec[96:128], "little") + m.ELL           # r_bar + l on the wire: from_cbor reduces it
    return rec[:96] + r.to_bytes(32, "little")


# acceptable spellings that are not the canonical bytes
RESPELL = {
    "indefinite": lambda r: b"\xbf" + _body(_ents(r)) + b"\xff",
    "reversed": lambda r: b"\xa4" + _body(_ents(r)[::-1]),
    "chunked": lambda r: b"\xa4\x01\x5f\x50" + r[:16] + b"\x50" + r[16:32] + b"\xff" + _body(_ents(r)[1:]),
    "key1801": lambda r: b"\xa4\x18\x01" + _ents(r)[0][1] + _body(_ents(r)[1:]),
    "unknown": lambda r: b"\xa5\x18\x63\x81\x00" + _body(_ents(r)),
    "swapped": lambda r: b"\xa4" + _body([_ents(r)[i] for i in (1, 0, 2, 3)]),      # two keys swapped: the canonical length
}
# lane i of a mixed batch is PATTERN[i % 13] of request i: (spelling or None for the canonical encoding, change to the record)
PATTERN = [("indefinite", None), (None, None), (None, _tamper), ("reversed", None), ("chunked", None), ("truncated", None), ("key1801", _tamper),
           ("indefinite", lambda r: b"\xff" * 32 + r[32:]), ("shape", None), ("double", None), ("unknown", None), (None, lambda r: b"\xff" * 32 + r[32:]),
           ("swapped", _unreduced)]
RESPELLED_IN_PATTERN = {0, 3, 4, 6, 7, 10, 12}                 # (6: status 1, 7: an undecodable K in a regular message -- both READ)


def _message(eng, rec, spelling):
    if spelling is None:
        return _encode(eng, rec)[0]
    if spelling == "truncated":
        return _encode(eng, rec)[0][:-1]                        # -> 254
    if spelling == "shape":
        return b"\xa4\x01\x01" + _body(_ents(rec)[1:])          # an integer where K's byte string belongs -> 253
    if spelling == "double":                                    # an invalid point AND a short scalar behind it: the point is met first -> 255
        return b"\xa4\x01" + bstr(BAD_PT) + b"\x02\x58\x1f" + bytes(31) + _body(_ents(rec)[2:])
    return RESPELL[spelling](rec)


def _batches(eng, n, tag):
    """the mixed batch, one that is entirely respelled, one that is entirely canonical"""
    req = _requests(eng, n, tag)
    recs = [req[128 * i:128 * i + 128] for i in range(n)]
    mixed = []
    for i, rec in enumerate(recs):
        sp, change = PATTERN[i % 13]
        mixed.append(_message(eng, change(rec) if change else rec, sp))
    names = sorted(RESPELL)
    respelled = [RESPELL[names[i % len(names)]](_tamper(rec) if i % 7 == 5 else rec) for i, rec in enumerate(recs)]
    canon = [_encode(eng, _tamper(rec) if i % 7 == 5 else rec)[0] for i, rec in enumerate(recs)]
    return mixed, respelled, canon


def _respelled_lanes(n):
    return [i for i in range(n) if i % 13 in RESPELLED_IN_PATTERN]


def _each_reader(eng, fn):
    """fn() under the device reader (the default), then under the host reader; the default is restored"""
    from act_amd import capi
    try:
        eng.set_wire_reader(capi.WIRE_READER_DEVICE); dev = fn()
        eng.set_wire_reader(capi.WIRE_READER_HOST); host = fn()
    finally:
        eng.set_wire_reader(capi.WIRE_READER_DEVICE)
    return dev, host


def _all_calls(eng, sk, msgs, cs, stream, with_offsets=True):
    """every issuance wire call over one batch, from host and from device memory: a dict of results, raw bytes throughout"""
    import torch
    from act_amd import capi
    n = len(msgs)
    blob = b"".join(msgs)
    offs = np.zeros(n + 1, np.uint64); offs[1:] = np.cumsum([len(x) for x in msgs], dtype=np.uint64)
    p_offs = offs.ctypes.data if with_offsets else 0
    h_blob = np.frombuffer(blob + b"\0", np.uint8); h_c = np.frombuffer(cs, np.uint8); h_rng = np.frombuffer(stream, np.uint8)
    d = lambda a: torch.from_numpy(a.copy()).cuda()
    d_blob, d_c, d_rng = d(h_blob), d(h_c), d(h_rng)
    out = {}
    for mem, name in ((capi.MEM_HOST, "host"), (capi.MEM_DEVICE, "hbm")):
        dev = mem == capi.MEM_DEVICE
        if dev:
            st = torch.full((n,), 99, dtype=torch.uint8, device="cuda"); req = torch.full((128 * n,), 5, dtype=torch.uint8, device="cuda")
            resp = torch.full((RESP * n,), 9, dtype=torch.uint8, device="cuda"); torch.cuda.synchronize()
            ptr = lambda t: t.data_ptr(); back = lambda t: t.cpu().numpy().tobytes()
            p_blob, p_c, p_rng = d_blob.data_ptr(), d_c.data_ptr(), d_rng.data_ptr()
        else:
            st = np.full(n, 99, np.uint8); req = np.full(128 * n, 5, np.uint8); resp = np.full(RESP * n, 9, np.uint8)
            ptr = lambda a: a.ctypes.data; back = lambda a: a.tobytes()
            p_blob, p_c, p_rng = h_blob.ctypes.data, h_c.ctypes.data, h_rng.ctypes.data
        eng.issue_check_cbor_ptr(n, mem, p_blob, p_offs, ptr(st), ptr(req))
        out[name, "check"] = (back(st), back(req))
        assert eng.secret_residue() == 0
        for mode, label in ((capi.RNG_PER_LANE, "per_lane"), (capi.RNG_SEQUENTIAL, "sequential")):
            st[:] = 99; resp[:] = 9
            if dev:
                torch.cuda.synchronize()
            eng.issue_cbor_ptr(sk, n, mem, p_blob, p_offs, p_c, p_rng, mode, ptr(resp), ptr(st))
            out[name, label] = (back(st), back(resp))
            assert eng.secret_residue() == 0
        g = capi.ReplayRng(stream)
        st[:] = 99; resp[:] = 9
        if dev:
            torch.cuda.synchronize()
        eng.issue_cbor_ptr(sk, n, mem, p_blob, p_offs, p_c, g.ptr, capi.RNG_CALLBACK, ptr(resp), ptr(st))
        out[name, "callback"] = (back(st), back(resp), list(g.draws), g.pos)
        assert eng.secret_residue() == 0
    return out


def _expect(octx, sk, msgs, cs, stream):
    st, resp, drawn, req = _loop(octx, sk, msgs, cs, stream)
    st_pl, resp_pl, _, _ = _loop(octx, sk, msgs, cs, stream, per_lane=True)
    want = {}
    for name in ("host", "hbm"):
        want[name, "check"] = (st, req)
        want[name, "per_lane"] = (st_pl, _flat(resp_pl))
        want[name, "sequential"] = (st, _flat(resp))
        want[name, "callback"] = (st, _flat(resp), [drawn], drawn)      # one draw, after every verdict, of exactly 128 k bytes
    return want


@pytest.mark.parametrize("max_batch,n", SHAPES)
def test_both_readers_equal_the_server_loop(engine_factory, oracle, bench_params, max_batch, n):
    from act_amd import capi
    eng = engine_factory(bench_params, 8, max_batch=max_batch)
    sk = eng.private_key_random(shake("iwr-sk", 64))
    octx = oracle.ctx(bench_params, 8)
    tag = "iwr%d" % n
    cs = _amounts(n, tag)
    stream = shake(tag + "-rng", 128 * n)
    mixed, respelled, canon = _batches(eng, n, tag)
    # respelled lanes at lane 0, at the last lane of a chunk, at the first lane of the next chunk and at the last lane of the call
    marks = {0, n - 1} | ({max_batch - 1, max_batch} if n > max_batch else set())
    assert marks <= set(_respelled_lanes(n)) and all(not mixed[i].startswith(canon[i][:4]) for i in marks)
    assert all(len(x) == 141 for x in canon) and all(a[:4] != b[:4] for a, b in zip(respelled, canon))
    for mode in ((capi.TRANSCRIPT_HOST, capi.TRANSCRIPT_DEVICE) if n < 64 else (capi.TRANSCRIPT_DEVICE,)):
        eng.set_transcript_mode(mode)
        for name, msgs in (("mixed", mixed), ("respelled", respelled), ("canonical", canon)):
            want = _expect(octx, sk, msgs, cs, stream)
            if name == "mixed":
                assert {0, 1, 253, 254, 255} <= set(want["host", "check"][0]) and want["host", "check"][0].count(0) >= n // 3
                assert all(want["host", "check"][0][i] == 0 for i in marks)
            else:
                assert set(want["host", "check"][0]) == {0, 1}
            dev, host = _each_reader(eng, lambda: _all_calls(eng, sk, msgs, cs, stream))
            for key in want:
                assert dev[key] == host[key], (name, key, "device reader against host reader")
                assert dev[key] == want[key], (name, key, [i for i in range(n) if dev[key][0][i] != want[key][0][i]])
        # offsets == NULL: messages of the canonical length back to back, every third one with two keys swapped
        same = [RESPELL["swapped"](_decode(m_)) if i % 3 == 0 else m_ for i, m_ in enumerate(canon)]
        assert all(len(x) == 141 for x in same) and same[0] != canon[0]
        want = _expect(octx, sk, same, cs, stream)
        dev, host = _each_reader(eng, lambda: _all_calls(eng, sk, same, cs, stream, with_offsets=False))
        for key in want:
            assert dev[key] == host[key] == want[key], ("no offsets", key)
    assert eng.secret_residue() == 0


def _decode(msg):
    es, rec = m.cbor_decode("IssuanceRequest", msg, 8)
    assert es == 0
    # (from_cbor's record: a tampered gamma stays tampered; the scalars of a request the engine made are reduced already)
    return rec


@pytest.mark.parametrize("max_batch,n", SHAPES)
def test_where_the_messages_were_read(engine_factory, bench_params, max_batch, n):
    """FAILS ON THE PARENT COMMIT: there the issuance calls count nothing and read every respelled message on the host."""
    from act_amd import capi
    eng = engine_factory(bench_params, 8, max_batch=max_batch, transcript=capi.TRANSCRIPT_DEVICE)
    sk = eng.private_key_random(shake("iwr-sk", 64))
    tag = "iws%d" % n
    cs = _amounts(n, tag)
    stream = shake(tag + "-rng", 128 * n)
    _, respelled, canon = _batches(eng, n, tag)
    msgs = [respelled[i] if i % 3 != 1 else canon[i] for i in range(n)]
    r = sum(1 for i in range(n) if i % 3 != 1); c = n - r
    calls = {"check": lambda: eng.issue_check_cbor(msgs), "per_lane": lambda: eng.issue_cbor(sk, msgs, cs, stream, capi.RNG_PER_LANE),
             "sequential": lambda: eng.issue_cbor(sk, msgs, cs, stream, capi.RNG_SEQUENTIAL), "callback": lambda: eng.issue_cbor(sk, msgs, cs, capi.ReplayRng(stream), capi.RNG_CALLBACK)}
    chunks = (n + max_batch - 1) // max_batch
    try:
        eng.prof_enable(True)
        for name, call in calls.items():
            assert eng.wire_stats(reset=True) is not None      # (the default setting: nothing is set here)
            eng.prof_reset()
            res_d = call()
            prof = eng.prof()
            assert eng.wire_stats(reset=True) == {"seen": r + c, "canonical": c, "read_on_device": r, "read_by_host": 0}, name
            for k in ("k_issue_wire_flag", "k_cbor_read_raw", "k_cbor_read_raw(validate)", "k_issue_a_wire"):
                assert prof[k]["launches"] == chunks and prof[k]["lanes"] == n, (name, k, prof.get(k))
            eng.set_wire_reader(capi.WIRE_READER_HOST)
            eng.prof_reset()
            res_h = call()
            prof = eng.prof()
            assert eng.wire_stats(reset=True) == {"seen": r + c, "canonical": c, "read_on_device": 0, "read_by_host": r}, name
            assert "k_cbor_read_raw" not in prof and "k_issue_wire_flag" not in prof and prof["k_issue_a_wire"]["launches"] == chunks
            eng.set_wire_reader(capi.WIRE_READER_DEVICE)
            assert res_d == res_h and set(res_d[0]) == {0, 1}
    finally:
        eng.prof_enable(False)
        eng.set_wire_reader(capi.WIRE_READER_DEVICE)
    assert eng.secret_residue() == 0


def test_a_failing_generator_signs_nothing(engine_factory, oracle, bench_params):
    from act_amd import capi
    max_batch, n = SHAPES[0]
    eng = engine_factory(bench_params, 8, max_batch=max_batch, transcript=capi.TRANSCRIPT_DEVICE)
    sk = eng.private_key_random(shake("iwr-sk", 64))
    octx = oracle.ctx(bench_params, 8)
    cs = _amounts(n, "iwf")
    stream = shake("iwf-rng", 128 * n)
    mixed, _, _ = _batches(eng, n, "iwf")
    want_st, _, drawn, _ = _loop(octx, sk, mixed, cs, stream)
    accepted_respelled = [i for i in _respelled_lanes(n) if want_st[i] == 0]
    assert len(accepted_respelled) >= 3 and drawn == 128 * want_st.count(0)
    eng.wire_stats(reset=True)
    g = capi.ReplayRng(stream[:drawn - 1])
    rc, st, flat = _raw_issue(eng, sk, mixed, cs, g.ptr, capi.RNG_CALLBACK)
    assert rc == 5 and st == want_st and flat == bytes(RESP * n) and g.pos == 0      # ACT_ERR_RNG: the check half's statuses, every slot zero
    assert eng.wire_stats(reset=True)["read_by_host"] == 0
    assert eng.secret_residue() == 0


def test_through_the_node(engine_factory, oracle, bench_params):
    from act_amd import capi
    max_batch, n = SHAPES[0]
    eng = engine_factory(bench_params, 8, max_batch=max_batch, transcript=capi.TRANSCRIPT_DEVICE)
    sk = eng.private_key_random(shake("iwr-sk", 64))
    octx = oracle.ctx(bench_params, 8)
    cs = _amounts(n, "iwn2")
    stream = shake("iwn2-rng", 128 * n)
    mixed, _, _ = _batches(eng, n, "iwn2")
    want_st, want_out, drawn, want_req = _loop(octx, sk, mixed, cs, stream)
    want_pl = _loop(octx, sk, mixed, cs, stream, per_lane=True)
    one = (eng.issue_check_cbor(mixed), eng.issue_cbor(sk, mixed, cs, stream, capi.RNG_SEQUENTIAL), eng.issue_cbor(sk, mixed, cs, stream, capi.RNG_PER_LANE))
    assert one == ((want_st, want_req), (want_st, want_out), want_pl[:2])
    node = capi.Node(bench_params, 8, devices=(0, 0), max_batch=3, transcript=capi.TRANSCRIPT_DEVICE)
    try:
        for where in (capi.WIRE_READER_DEVICE, capi.WIRE_READER_HOST):
            assert node.lib.act_node_set_wire_reader(node.nd, where) == 0
            for k in range(2):
                out = (C.c_uint64 * 4)()
                assert node.lib.act_ctx_wire_stats(node.lib.act_node_ctx(node.nd, k), C.cast(out, C.c_void_p), 1) == 0
            g = capi.ReplayRng(stream)
            got = (node.issue_check_cbor(mixed), node.issue_cbor(sk, mixed, cs, stream, capi.RNG_SEQUENTIAL), node.issue_cbor(sk, mixed, cs, stream, capi.RNG_PER_LANE))
            assert got == one, where
            assert node.issue_cbor(sk, mixed, cs, g, capi.RNG_CALLBACK) == (want_st, want_out) and g.draws == [drawn]
            seen = [0, 0, 0, 0]
            for k in range(2):
                out = (C.c_uint64 * 4)()
                assert node.lib.act_ctx_wire_stats(node.lib.act_node_ctx(node.nd, k), C.cast(out, C.c_void_p), 1) == 0
                seen = [a + int(b) for a, b in zip(seen, out)]
                n_res = C.c_size_t(0)
                assert node.lib.act_debug_secret_residue(node.lib.act_node_ctx(node.nd, k), C.byref(n_res)) == 0 and n_res.value == 0
            assert seen[0] == 4 * n and seen[1] < seen[0] and (seen[3] == 0) == (where == capi.WIRE_READER_DEVICE) and (seen[2] == 0) == (where == capi.WIRE_READER_HOST)
    finally:
        node.close()
