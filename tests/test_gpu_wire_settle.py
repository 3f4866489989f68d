"""The host reader's settle window (csrc/wire_window.h, wire_window_read in cbor_impl.inc) through its three callers -- the spend
calls, the admission screen and the issuance calls -- on device-memory batches whose flagged messages lie FAR APART: lanes 0 and
n - 1 respelled, n chosen so that the bytes between them just exceed 2^20 + 2 * (the flagged bytes), which is where a window gathers
one copy per message instead of one copy of the span, and where 2 lanes over a span of n make the lane patch sparse (issuance; the
spend settle patches the span of its lanes, and every unflagged lane between them must come back as it was).  Beside each
such batch the same one with two messages from_cbor refuses next to lane 0: a truncated map (254) and an invalid point that a
duplicate key keeps out of the record (255, which only cbor_settle_codes can tell; the reader itself reads a full record).

ACT_WIRE_READER_HOST is held to ACT_WIRE_READER_DEVICE on every output byte, and both to the answers for the few distinct messages:
the server loop restated (tests/test_gpu_wire.py, tests/test_gpu_issue_wire.py) and the oracle.  L = 8; every other lane of a batch
is one canonical message repeated, so an unflagged lane that a patch disturbs shows in the whole-array comparison."""
import numpy as np
import pytest

import keyring_cases as kr
import pymodel as m
from conftest import shake, scb
from test_gpu_issue_wire import RESP, _loop as _issue_loop, _requests
from test_gpu_issue_wire_reader import RESPELL
from test_gpu_wire import WIRE, _loop
from test_gpu_wire_reader import _both, _irregular, _respellings

pytestmark = pytest.mark.gpu

L = 8
REFUSED = [(), ("truncated", "hidden")]


def _far_apart(first, last, refused, canon):
    """[first, *refused, canon ... canon, last] with the fewest canonical messages that put the window on the per-message road"""
    flagged = len(first) + len(last) + sum(len(x) for x in refused)
    fill = (2**20 + 2 * flagged - flagged) // len(canon) + 1      # span = flagged + fill * len(canon) > 2 * flagged + 2^20
    msgs = [first] + list(refused) + [canon] * fill + [last]
    span = sum(len(x) for x in msgs)
    assert span > 2 * flagged + 2**20 >= span - len(canon)        # one canonical message fewer and the window is one span copy
    assert len(msgs) > 2 * (2 + len(refused)) + 64                # and the lanes are sparse by the patch rule
    return msgs


def _dev(msgs):
    import torch
    offs = np.zeros(len(msgs) + 1, np.uint64); offs[1:] = np.cumsum([len(x) for x in msgs], dtype=np.uint64)
    return torch.from_numpy(np.frombuffer(b"".join(msgs) + b"\0", np.uint8).copy()).cuda(), offs


def _fill(n, v):
    import torch
    return torch.full((n,), v, dtype=torch.uint8, device="cuda")


def _back(*ts):
    return tuple(t.cpu().numpy().tobytes() for t in ts)


@pytest.fixture(scope="module")
def spend(engine_factory, oracle, bench_params):
    """one valid proof under key b of the ring (a, b): its canonical message, two respellings, the two refused spellings"""
    from act_amd import capi
    eng = engine_factory(bench_params, L, max_batch=256, transcript=capi.TRANSCRIPT_DEVICE)
    octx = oracle.ctx(bench_params, L)
    a, b = kr.make_keys(octx, "wst", 2)
    rec = kr.spend_under(octx, b, "wst-p")[0]
    canon = eng.cbor_encode("SpendProof", rec)[0]
    assert len(canon) == eng.cbor_size("SpendProof")
    sp = _respellings(rec, L)
    refused = {"truncated": canon[:-1], "hidden": _irregular(rec, L)[0]}
    assert [m.cbor_decode("SpendProof", x, L)[0] for x in (refused["truncated"], refused["hidden"])] == [1, 3]
    return eng, octx, (a, b), rec, canon, (sp[0], sp[1]), refused


def _spend_batch(spend, which):
    eng, octx, ring, rec, canon, (first, last), refused = spend
    msgs = _far_apart(first, last, [refused[w] for w in which], canon)
    assert 500 < len(msgs) < 800
    return msgs, 2 + len(which)


@pytest.mark.parametrize("which", REFUSED, ids=["two-respelled", "with-refused"])
def test_spend_settle_far_apart_one_key(spend, which):
    from act_amd import capi
    eng, octx, (a, b), rec, canon, _, refused = spend
    eng.set_transcript_mode(capi.TRANSCRIPT_DEVICE)
    msgs, flagged = _spend_batch(spend, which)
    n = len(msgs)
    d_blob, offs = _dev(msgs)
    ps, ks = capi._in(b, 64)

    def call():
        import torch
        d_st, d_kp, d_nul = _fill(n, 99), _fill(32 * n, 9), _fill(32 * n, 9); torch.cuda.synchronize()
        eng._ck(eng.lib.act_verify_spend_cbor_keys_batch(eng.ctx, n, capi.MEM_DEVICE, ps, d_blob.data_ptr(), offs.ctypes.data, d_st.data_ptr(), d_kp.data_ptr(), d_nul.data_ptr()))
        return _back(d_st, d_kp, d_nul)
    dv, hv, sd, sh = _both(eng, call)
    assert sd == {"seen": n, "canonical": n - flagged, "read_on_device": flagged, "read_by_host": 0}
    assert sh == {"seen": n, "canonical": n - flagged, "read_on_device": 0, "read_by_host": flagged}
    # what every lane must hold: the oracle's K' and the record's k for a message that reads; the hidden invalid point keeps its k
    vst, kprime = octx.verify_spend(b, rec)
    assert vst == 0
    lanes = {"ok": (0, kprime, rec[:32]), "truncated": (254, bytes(32), bytes(32)), "hidden": (255, bytes(32), rec[:32])}
    names = ["ok"] + list(which) + ["ok"] * (n - 1 - len(which))
    want = tuple(b"".join(lanes[x][f] if f else bytes([lanes[x][0]]) for x in names) for f in range(3))
    assert hv == want and dv == want
    # ... and the server loop restated, on the distinct messages
    small = [msgs[0]] + [refused[w] for w in which] + [canon, msgs[-1]]
    assert _loop(octx, b, L, small, shake("wst-rng", 128 * len(small)))[0] == bytes([0] + [lanes[w][0] for w in which] + [0, 0])
    assert eng.secret_residue() == 0


@pytest.mark.parametrize("which", REFUSED, ids=["two-respelled", "with-refused"])
def test_spend_settle_far_apart_ring_and_admission(spend, which):
    """the ring's verification (out_key patched beside the statuses) through act_redeem_cbor_keyring_batch, and the same batch through
    act_redeem_cbor_admit_batch against an empty set: every lane carries the same nullifier, so lane 0 is signed and the others that
    read are double spends -- after verification for the ring call, and for the admission call too (the screen looks up the set, which is empty)"""
    import torch
    from act_amd import capi
    eng, octx, (a, b), rec, canon, _, refused = spend
    eng.set_transcript_mode(capi.TRANSCRIPT_DEVICE)
    msgs, flagged = _spend_batch(spend, which)
    n = len(msgs)
    d_blob, offs = _dev(msgs)
    rng = shake("wst-ring-rng", 128 * n)
    d_rng = torch.from_numpy(np.frombuffer(rng, np.uint8).copy()).cuda()
    ml = eng.cbor_size("Refund")

    def run(fn):
        ns = capi.NullifierSet(4 * n)
        try:
            d_st, d_ok, d_out = _fill(n, 99), _fill(n, 99), _fill(ml * n, 9); torch.cuda.synchronize()
            p = dict(set=ns, cbor=d_blob.data_ptr(), offsets=offs.ctypes.data, rng=d_rng.data_ptr(), rng_mode=capi.RNG_PER_LANE, out=d_out.data_ptr(),
                     status=d_st.data_ptr(), out_key=d_ok.data_ptr())
            counts = eng.admit_ptr("redeem_cbor", [a, b], n, capi.MEM_DEVICE, **p) if fn == "admit" else eng.keyring_ptr("redeem_cbor", [a, b], n, capi.MEM_DEVICE, **p)
            return _back(d_st, d_ok, d_out), counts, len(ns)
        finally:
            ns.close()
    wire = {"truncated": 254, "hidden": 255}
    want_st = bytes([0] + [wire[w] for w in which] + [3] * (n - 1 - len(which)))
    want_ok = bytes([1] + [255] * len(which) + [1] * (n - 1 - len(which)))      # (a double spend keeps the key it matched)
    s2, rf = octx.refund(b, rec, rng[:128])
    assert s2 == 0
    want_out = m.cbor_encode("Refund", rf, L) + bytes(ml * (n - 1))
    for fn in ("ring", "admit"):
        dv, hv, sd, sh = _both(eng, lambda: run(fn))
        assert dv == hv, fn
        assert dv[0] == (want_st, want_ok, want_out) and dv[2] == 1, fn
        assert sd["read_by_host"] == 0 and sd["read_on_device"] == sh["read_by_host"] > 0 and sh["read_on_device"] == 0, fn
        if fn == "admit":      # nothing is shed but what the reader refused
            assert dv[1]["lanes"] == n and dv[1]["wire_rejected"] == len(which) and dv[1]["spent_before"] == 0 and dv[1]["accepted"] == 1, dv[1]
    assert eng.secret_residue() == 0


@pytest.mark.parametrize("which", REFUSED, ids=["two-respelled", "with-refused"])
def test_issuance_settle_far_apart(engine_factory, oracle, bench_params, which):
    import torch
    from act_amd import capi
    eng = engine_factory(bench_params, L, max_batch=4096, transcript=capi.TRANSCRIPT_DEVICE)
    octx = oracle.ctx(bench_params, L)
    sk = eng.private_key_random(shake("wsi-sk", 64))
    rec = _requests(eng, 1, "wsi")
    canon = eng.cbor_encode("IssuanceRequest", rec)[0]
    assert len(canon) == 141
    es = [(k + 1, b"\x58\x20" + rec[32 * k:32 * k + 32]) for k in range(4)]
    body = b"".join(m._cbor_head(0, k) + v for k, v in es)
    refused = {"truncated": canon[:-1], "hidden": b"\xa5\x01\x58\x20\x01" + bytes(31) + body}
    assert [m.cbor_decode("IssuanceRequest", refused[w], 128)[0] for w in ("truncated", "hidden")] == [1, 3]
    msgs = _far_apart(RESPELL["indefinite"](rec), RESPELL["reversed"](rec), [refused[w] for w in which], canon)
    n, flagged = len(msgs), 2 + len(which)
    assert 7000 < n < 8000
    cs = scb(77) * n
    stream = shake("wsi-rng", 128 * n)
    d_blob, offs = _dev(msgs)
    d_c, d_rng = (torch.from_numpy(np.frombuffer(x, np.uint8).copy()).cuda() for x in (cs, stream))

    def calls():
        d_st, d_req, d_resp = _fill(n, 99), _fill(128 * n, 5), _fill(RESP * n, 9); torch.cuda.synchronize()
        eng.issue_check_cbor_ptr(n, capi.MEM_DEVICE, d_blob.data_ptr(), offs.ctypes.data, d_st.data_ptr(), d_req.data_ptr())
        check = _back(d_st, d_req)
        d_st[:] = 99; torch.cuda.synchronize()
        eng.issue_cbor_ptr(sk, n, capi.MEM_DEVICE, d_blob.data_ptr(), offs.ctypes.data, d_c.data_ptr(), d_rng.data_ptr(), capi.RNG_PER_LANE, d_resp.data_ptr(), d_st.data_ptr())
        return check, _back(d_st, d_resp)
    dv, hv, sd, sh = _both(eng, calls)
    assert sd == {"seen": 2 * n, "canonical": 2 * (n - flagged), "read_on_device": 2 * flagged, "read_by_host": 0}
    assert sh == {"seen": 2 * n, "canonical": 2 * (n - flagged), "read_on_device": 0, "read_by_host": 2 * flagged}
    # every lane that reads carries the same request: what the all-canonical batch answers, lane by lane its own rng slice
    st_c, out_c = eng.issue_cbor(sk, [canon] * n, cs, stream, capi.RNG_PER_LANE)
    assert st_c == bytes(n)
    wire = {"truncated": 254, "hidden": 255}
    bad = range(1, 1 + len(which))
    want_st = bytes([0] + [wire[w] for w in which] + [0] * (n - 1 - len(which)))
    want_req = b"".join(bytes(128) if i in bad else rec for i in range(n))
    want_resp = b"".join(bytes(RESP) if i in bad else out_c[i] for i in range(n))
    assert hv == ((want_st, want_req), (want_st, want_resp))
    assert dv == hv
    # the server loop restated on the small lanes (lane i signs with slice i)
    for i in (0, 1, 2, 3, n - 1):
        st, out, _, req = _issue_loop(octx, sk, [msgs[i]], cs[32 * i:32 * i + 32], stream[128 * i:128 * i + 128])
        assert (st[0], out[0] or bytes(RESP), req) == (want_st[i], want_resp[RESP * i:RESP * i + RESP], want_req[128 * i:128 * i + 128]), i
    assert eng.secret_residue() == 0
