"""Request binding on the CPU: the prover's and the ring verifier's lane bodies with a binding, compiled for the host by
tests/hostcheck/bound_check.cpp, against the big-integer model of tests/bound_cases.py; the ring's patched re-hash at the bound length
(csrc/blake3_hd.h in the lane body, csrc/host_pool.cpp act_host_hash_ring_many as the engine calls it) against a whole-message BLAKE3;
and bind = NULL through the same bodies against the existing ones.  The same bodies run on the GPU in tests/test_gpu_bound.py.

Why these L (bytes(L) = 424 + 120 L): 5 -- unbound is exactly one chunk (1 024 bytes, the root itself), bound is two, so chunk 0 of the
ring's re-hash gains its first path sibling; 10 -- bound is 1 664 bytes, a whole number of 64-byte blocks; 22 -- 3 064 -> 3 104 crosses
the three-to-four chunk boundary; 128 -- the product's size."""
import ctypes as C
import os

import numpy as np
import pytest

import pymodel as pm

import bound_cases as bc
from conftest import ROOT


@pytest.fixture(scope="module")
def check():
    lib = C.CDLL(bc.build_check(os.path.join(ROOT, "tests", "hostcheck", "libbound_check.so")))
    lib.hc_bound_transcript_bytes.restype = C.c_uint32
    lib.hc_bound_transcript_stride.restype = C.c_uint32
    return lib


@pytest.fixture(scope="module")
def engine_lib():
    from act_amd import capi
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    lib = capi.load()
    lib.act_host_hash_ring_many.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_size_t, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.act_host_hash_ring_many.restype = None
    return lib


def prove(check, c, bind):
    L = c["L"]
    tb = check.hc_bound_transcript_bytes(L, 1 if bind is not None else 0)
    proof = C.create_string_buffer(32 * (14 + 4 * L)); prer = C.create_string_buffer(96); st = C.create_string_buffer(1); tr = C.create_string_buffer(tb)
    assert check.hc_bound_prove(c["h"], L, 1, c["tok_rec"], bc.scb(c["s"]), c["rng"], bind, proof, prer, st, tr) == 1
    assert st.raw == b"\0"
    return proof.raw, prer.raw, tr.raw


def ring_verify(check, c, ring, proofs, bind):
    L = c["L"]
    n, nk = len(proofs) // (32 * (14 + 4 * L)), len(ring)
    stride = check.hc_bound_transcript_stride(L, 1 if bind is not None else 0)
    st = C.create_string_buffer(n); ok = C.create_string_buffer(n); kp = C.create_string_buffer(32 * n); tr = C.create_string_buffer(stride * n + 64)
    cand = C.create_string_buffer(max(1, 32 * n * (nk - 1))); xofs = C.create_string_buffer(64 * n * nk)
    assert check.hc_bound_ring_verify(c["h"], L, b"".join(ring), nk, n, proofs, bind, st, ok, kp, tr, cand, xofs) == 1
    return st.raw, ok.raw, kp.raw, tr.raw, cand.raw, xofs.raw, stride


def strangers(count):
    """ring keys the proofs were NOT made under (the proof's own key goes last)"""
    return [pm.PrivateKey.random(pm.ByteRng(bc.shake("bound-stranger-%d" % i, 64))).record() for i in range(count)]


@pytest.mark.parametrize("L", bc.LS)
def test_a_bound_lane_writes_the_models_transcript_and_finds_its_challenge(check, L):
    """1. the prover's body: proof bytes and PreRefund are the model's, the transcript is transcript_preimage(...) + _lp(bind); the
    verifier's body under the same binding: the same pre-image, status 0, the model's K'"""
    c = bc.case(L)
    proof, prer, tr = prove(check, c, c["bind"])
    assert len(tr) == bc.tr_bytes(L, True) == bc.tr_bytes(L) + 40
    assert proof == c["proof_rec"] and prer == c["prerefund"]
    assert proof[32 * (4 + L):32 * (5 + L)] == pm.sc_bytes(c["gamma"])
    items = bc.spend_items(c["params"], c["sk"].x, c["proof"])
    want = pm.transcript_preimage(c["params"], b"spend", items) + bc.lp(c["bind"])
    assert tr == want
    assert pm.sc_from_wide(pm.blake3(tr, 64)) == c["gamma"]
    st, ok, kp, vtr, _, xofs, stride = ring_verify(check, c, [c["sk_rec"]], proof, c["bind"])
    assert (st, ok) == (b"\0", b"\0") and vtr[:len(want)] == want
    assert kp == pm.E(pm.spend_verify_challenge(c["sk"].x, c["params"], c["proof"])[1])
    assert xofs == pm.blake3(want, 64)
    # the same proof under a binding with one bit flipped, under the all-zero binding, and unbound: a tampered proof's status
    flipped = bytes([c["bind"][0] ^ 1]) + c["bind"][1:]
    for other in (flipped, bytes(32), None):
        st, ok, kp, _, _, _, _ = ring_verify(check, c, [c["sk_rec"]], proof, other)
        assert (st, ok, kp) == (b"\x07", b"\xff", bytes(32)), other
    # an unbound proof under the all-zero binding
    st, ok, _, _, _, _, _ = ring_verify(check, c, [c["sk_rec"]], c["plain_rec"], bytes(32))
    assert (st, ok) == (b"\x07", b"\xff")


@pytest.mark.parametrize("nkeys", [1, 3])
@pytest.mark.parametrize("L", bc.LS)
def test_ring_rehash_at_the_bound_length_is_the_whole_message_hash(check, engine_lib, L, nkeys):
    """2. rings of 1 and 3 keys, the proof under the LAST key: act_host_hash_ring_many at the bound length (what the host-transcript mode
    calls) and ring_hash_lane (the device mode's body) against pymodel.blake3 of every key's patched transcript"""
    c = bc.case(L)
    ring = strangers(nkeys - 1) + [c["sk_rec"]]
    n = 17                                          # one group of sixteen through the SIMD routines and one message through the scalar one
    binds = [bc.shake("bound-rehash-%d-%d" % (L, i), 32) for i in range(n)]
    binds[3] = c["bind"]
    proofs = c["proof_rec"] * n
    st, ok, _, tr, cand, xofs, stride = ring_verify(check, c, ring, proofs, b"".join(binds))
    assert [i for i in range(n) if st[i] == 0] == [3] and ok[3] == nkeys - 1 and all(ok[i] == 255 for i in range(n) if i != 3)
    length, a1, extra = bc.tr_bytes(L, True), 184 + 40 * 3 + 8, nkeys - 1
    assert stride == bc.tr_stride(L, True)
    msgs = np.frombuffer(tr, np.uint8).copy(); cd = np.frombuffer(cand, np.uint8).copy(); out = np.zeros(n * nkeys * 16, np.uint32)
    engine_lib.act_host_hash_ring_many(msgs.ctypes.data, stride, length, n, 2, nkeys, a1, cd.ctypes.data, out.ctypes.data)
    got = out.tobytes()
    for i in range(n):
        msg = tr[i * stride:i * stride + length]
        assert msg[-40:] == bc.lp(binds[i])
        for k in range(nkeys):
            patched = msg if k == 0 else msg[:a1] + cand[32 * (i * extra + k - 1):][:32] + msg[a1 + 32:]
            want = pm.blake3(patched, 64)
            at = 64 * (i * nkeys + k)
            assert got[at:at + 64] == want, (L, nkeys, i, k, "act_host_hash_ring_many")
            assert xofs[at:at + 64] == want, (L, nkeys, i, k, "ring_hash_lane")
    assert pm.sc_from_wide(got[64 * (3 * nkeys + nkeys - 1):][:64]) == c["gamma"]


@pytest.mark.parametrize("L", bc.LS)
def test_bind_null_through_the_new_bodies_is_the_existing_output(check, hostcheck, L):
    """3. bind = NULL: the prover's and the verifier's bodies give the bytes hostcheck.cpp's existing entry points give"""
    c = bc.case(L)
    pb, tb = 32 * (14 + 4 * L), bc.tr_bytes(L)
    proof, prer, tr = prove(check, c, None)
    old_p = C.create_string_buffer(pb); old_r = C.create_string_buffer(96); old_s = C.create_string_buffer(1)
    assert hostcheck.hc_prove_spend(c["h"], L, 1, c["tok_rec"], bc.scb(c["s"]), c["rng"], old_p, old_r, old_s, None) == 1
    assert (proof, prer) == (old_p.raw, old_r.raw) and proof == c["plain_rec"] and len(tr) == tb
    for rec in (proof, c["proof_rec"]):             # an accepted lane and a rejected one
        st, ok, kp, vtr, _, xofs, stride = ring_verify(check, c, [c["sk_rec"]], rec, None)
        otr = C.create_string_buffer(tb); ost = C.create_string_buffer(1); okp = C.create_string_buffer(32)
        assert hostcheck.hc_spend_verify(c["h"], L, c["sk_rec"], 1, rec, otr, ost, okp, None) == 1
        assert stride == bc.tr_stride(L) and vtr[:tb] == otr.raw and (st, kp) == (ost.raw, okp.raw)
        assert xofs == pm.blake3(otr.raw, 64)
    items = bc.spend_items(c["params"], c["sk"].x, pm.parse_spend_proof(proof, L))
    assert tr == pm.transcript_preimage(c["params"], b"spend", items)
