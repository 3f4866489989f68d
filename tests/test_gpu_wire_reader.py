"""The wire reader on the GPU (csrc/cbor_lanes.h, k_cbor_read.hip): a message that is not byte for byte the canonical template is
read by a kernel in its chunk's own stream and verified once, in the pipeline.  act_cbor_read_batch against act_cbor_decode_batch;
every wire-level spend call under both reader settings (act_ctx_set_wire_reader) against each other and against the server loop
restated (tests/test_gpu_wire.py); batches in which every message is respelled; irregular messages (duplicate keys, over-long
arrays) whose first failure in wire order only the validating pass can tell; the admission screen; act_ctx_wire_stats."""
import numpy as np
import pytest

import keyring_cases as kr
import pymodel as m
from conftest import shake, scb
from test_cbor import _variants
from test_cbor_read_host import _entries as _ents
from test_gpu_cbor_verify import _proofs
from test_gpu_wire import WIRE, _loop, _messages

pytestmark = pytest.mark.gpu

BAD_PT = b"\x58\x20\x01" + bytes(31)


def _both(eng, fn):
    """fn() under the device reader and under the host reader -> (device result, host result, stats of each); the default is restored"""
    from act_amd import capi
    res = []
    try:
        for where in (capi.WIRE_READER_DEVICE, capi.WIRE_READER_HOST):
            eng.set_wire_reader(where)
            eng.wire_stats(reset=True)
            r = fn()
            res.append((r, eng.wire_stats(reset=True)))
    finally:
        eng.set_wire_reader(capi.WIRE_READER_DEVICE)
    return res[0][0], res[1][0], res[0][1], res[1][1]


def _body(es):
    return b"".join(m._cbor_head(0, k) + v for k, v in es)


_ACCEPTABLE = {}


def _respellings(rec, L):
    """acceptable spellings of one record that are not the canonical bytes: every spelling of _variants that from_cbor accepts (the
    model decides) and that does not begin with the canonical message, then six written here -- _variants has no indefinite-length
    array inside an indefinite-length map and no duplicate of a POINT key with a valid value, which is what forces the validating pass"""
    enc = m.cbor_encode("SpendProof", rec, L)
    vs = [v for v, _ in _variants("SpendProof", rec, L)]
    if L not in _ACCEPTABLE:      # which entries of _variants those are does not depend on the record: the model is asked once per L
        same = (0, m.cbor_decode("SpendProof", enc, L)[1])      # accepted, and the same record (a valid proof's scalars are reduced already)
        _ACCEPTABLE[L] = [i for i, v in enumerate(vs) if not v.startswith(enc) and m.cbor_decode("SpendProof", v, L) == same]
    from_variants = [vs[i] for i in _ACCEPTABLE[L]]
    assert len(from_variants) >= 8 and not any(v.startswith(enc) for v in from_variants)
    return from_variants + [w for w in _written_respellings(rec, L) if w not in from_variants]


def _written_respellings(rec, L):
    es = _ents(rec, L); n = len(es)
    hd = lambda k: m._cbor_head(5, k)
    com = dict(es)[5]; ch = len(m._cbor_head(4, L))
    indef_arrays = [(k, (b"\x9f" + v[ch:] + b"\xff") if k in (5, 14, 15) else v) for k, v in es]
    return [b"\xbf" + _body(indef_arrays) + b"\xff",                          # indefinite map with indefinite arrays
            hd(n) + _body(es[::-1]),                                           # reversed key order
            hd(n + 1) + m._cbor_head(0, 3) + dict(es)[4] + _body(es),          # a duplicate key over a point: the last one wins, the validating pass runs
            hd(n + 1) + b"\x18\x63\x81\x00" + _body(es),                       # one unknown key
            hd(n) + b"\x18\x01" + es[0][1] + _body(es[1:]),                    # a key spelt 18 01
            hd(n) + m._cbor_head(0, es[0][0]) + b"\x5f\x50" + rec[:16] + b"\x50" + rec[16:32] + b"\xff" + _body(es[1:])]      # a chunked byte string


def test_cbor_read_equals_cbor_decode(engine_factory, bench_params, monkeypatch):
    import torch
    from act_amd import capi
    L = 8
    eng = engine_factory(bench_params, L, max_batch=6)
    sk = eng.private_key_random(shake("rd-sk", 64))
    pre = eng.pre_issuance_random(shake("rd-pre", 128 * 2)); req = eng.request(pre, shake("rd-rq", 128 * 2))
    st, resp = eng.issue(sk, req, scb(77) * 2, shake("rd-ir", 128 * 2))
    st, tok = eng.issuance_to_credit_token(pre, sk[32:], req, resp)
    st, proofs, prer = eng.prove_spend(tok, scb(7) * 2, shake("rd-pr", eng.prove_rng_bytes * 2))
    st, rf = eng.refund(sk, proofs, shake("rd-rr", 128 * 2))
    sk2 = eng.private_key_random(shake("rd-sk2", 64))
    recs = {"IssuanceRequest": req, "IssuanceResponse": resp, "SpendProof": proofs, "Refund": rf, "PrivateKey": sk + sk2, "PublicKey": sk[32:] + sk2[32:],
            "PreIssuance": pre, "CreditToken": tok, "PreRefund": prer}
    for chunk in (None, "3"):
        if chunk:
            monkeypatch.setenv("ACT_CBOR_CHUNK_MSGS", chunk)
            capi.forward_tuning_env()
        for t, blob in recs.items():
            rb = len(blob) // 2
            msgs = [v for i in range(2) for v, _ in _variants(t, blob[rb * i:rb * i + rb], L)]
            want = eng.cbor_decode(t, msgs)
            assert set(want[0]) >= {0, 1, 2}
            got = eng.cbor_read(t, msgs)
            assert got[0] == want[0], (t, chunk, [(i, got[0][i], want[0][i]) for i in range(len(msgs)) if got[0][i] != want[0][i]])
            assert got[1] == want[1], (t, chunk)
            # device memory
            n = len(msgs)
            offs = np.zeros(n + 1, np.uint64); offs[1:] = np.cumsum([len(x) for x in msgs], dtype=np.uint64)
            d_blob = torch.from_numpy(np.frombuffer(b"".join(msgs) + b"\0", np.uint8).copy()).cuda()
            d_out = torch.full((rb * n,), 9, dtype=torch.uint8, device="cuda"); d_st = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            eng._ck(eng.lib.act_cbor_read_batch(eng.ctx, capi.CBOR_TYPES[t], n, capi.MEM_DEVICE, d_blob.data_ptr(), offs.ctypes.data, d_out.data_ptr(), d_st.data_ptr()))
            assert d_st.cpu().numpy().tobytes() == want[0] and d_out.cpu().numpy().tobytes() == want[1], (t, chunk, "device")
    monkeypatch.delenv("ACT_CBOR_CHUNK_MSGS"); capi.forward_tuning_env()
    # canonical fixed-size messages without offsets
    canon = eng.cbor_encode("SpendProof", proofs)
    n = 2; p0, k0 = capi._in(b"".join(canon)); out = np.zeros(eng.proof_bytes * n, np.uint8); st = np.ones(n, np.uint8)
    eng._ck(eng.lib.act_cbor_read_batch(eng.ctx, capi.CBOR_TYPES["SpendProof"], n, capi.MEM_HOST, p0, None, out.ctypes.data, st.ctypes.data))
    assert st.tobytes() == bytes(2) and out.tobytes() == proofs
    assert eng.secret_residue() == 0


@pytest.mark.parametrize("L,max_batch", [(8, 3), (8, 6), (128, 6)])
def test_spend_wire_calls_under_both_readers_equal_the_server_loop(engine_factory, oracle, bench_params, L, max_batch):
    import torch
    from act_amd import capi
    eng = engine_factory(bench_params, L, max_batch=max_batch)
    sk = eng.private_key_random(shake("wrd-sk", 64))
    octx = oracle.ctx(bench_params, L)
    n = 13 if L == 8 else 8
    msgs = _messages(eng, sk, L, n, "wrd%d" % L)
    if L == 128:      # the same mix, thinned: the restated loop decodes every point of every message in Python
        msgs = msgs[:n] + msgs[n::3]
    N = len(msgs)
    stream = shake("wrd-rng", 128 * N)
    want_st, want_out, drawn = _loop(octx, sk, L, msgs, stream)
    assert {0, 6, 7, 253, 254, 255}.issubset(set(want_st))
    db = set()
    r_st, r_out, r_drawn = _loop(octx, sk, L, msgs, stream, db)
    ml = eng.cbor_size("Refund")
    for mode in ((capi.TRANSCRIPT_HOST, capi.TRANSCRIPT_DEVICE) if L == 8 else (capi.TRANSCRIPT_DEVICE,)):
        eng.set_transcript_mode(mode)
        dv, hv, sd, sh = _both(eng, lambda: eng.verify_spend_cbor_keys(sk, msgs))
        assert dv == hv and dv[0] == want_st
        assert sd["read_by_host"] == 0 and sd["read_on_device"] == sh["read_by_host"] > 10 and sd["seen"] == N and sd["canonical"] == N - sd["read_on_device"]
        for i, msg in enumerate(msgs if L == 8 else []):
            es, rec = m.cbor_decode("SpendProof", msg, L)
            kp, nul = dv[1][32 * i:32 * i + 32], dv[2][32 * i:32 * i + 32]
            if es == 0:       # the nullifier as it stood on the wire names the record's scalar
                assert int.from_bytes(nul, "little") % m.ELL == int.from_bytes(rec[:32], "little") % m.ELL, i
            elif es != 3:     # a message that does not read has neither (one that reads but holds an undecodable point still has its k)
                assert kp == bytes(32) and nul == bytes(32), (i, es)
            assert (kp != bytes(32)) == (want_st[i] == 0), i

        def refunds():
            g = capi.ReplayRng(stream)
            a = eng.refund_cbor(sk, msgs, g, capi.RNG_CALLBACK)
            return a, g.draws, eng.refund_cbor(sk, msgs, stream, capi.RNG_SEQUENTIAL)
        dv, hv, _, _ = _both(eng, refunds)
        assert dv == hv and dv[0] == (want_st, want_out) and dv[1] == [drawn] and dv[2] == (want_st, want_out)

        def redeems():
            ns = capi.NullifierSet(4 * N)
            g = capi.ReplayRng(stream)
            a = eng.redeem_cbor(ns, sk, msgs, g, capi.RNG_CALLBACK)
            keys = ns.export_epochs()
            ns.close()
            return a, g.pos, sorted(keys[0][i:i + 32] for i in range(0, len(keys[0]), 32))
        dv, hv, sd, _ = _both(eng, redeems)
        assert dv == hv and dv[0] == (r_st, r_out) and dv[1] == r_drawn and len(dv[2]) == len(db) and sd["read_by_host"] == 0
    # device memory: the settle kernel instead of the host patch
    eng.set_transcript_mode(capi.TRANSCRIPT_DEVICE)
    blob = b"".join(msgs)
    offs = np.zeros(N + 1, np.uint64); offs[1:] = np.cumsum([len(x) for x in msgs], dtype=np.uint64)
    d_blob = torch.from_numpy(np.frombuffer(blob + b"\0", np.uint8).copy()).cuda()
    ps, ks = capi._in(sk, 64)

    def device_keys():
        d_st = torch.full((N,), 99, dtype=torch.uint8, device="cuda"); d_kp = torch.full((32 * N,), 9, dtype=torch.uint8, device="cuda")
        d_nul = torch.full((32 * N,), 9, dtype=torch.uint8, device="cuda"); torch.cuda.synchronize()
        eng._ck(eng.lib.act_verify_spend_cbor_keys_batch(eng.ctx, N, capi.MEM_DEVICE, ps, d_blob.data_ptr(), offs.ctypes.data, d_st.data_ptr(), d_kp.data_ptr(), d_nul.data_ptr()))
        return d_st.cpu().numpy().tobytes(), d_kp.cpu().numpy().tobytes(), d_nul.cpu().numpy().tobytes()
    dv, hv, sd, _ = _both(eng, device_keys)
    assert dv == hv == eng.verify_spend_cbor_keys(sk, msgs) and sd["read_by_host"] == 0
    assert eng.secret_residue() == 0


def test_ring_forms_with_epochs_under_both_readers(engine_factory, oracle, bench_params):
    """The ring calls that take wire bytes are act_redeem_cbor_keyring_batch and its epochs form (there is no ring verify or ring refund
    on wire bytes in the interface); both go through ring_verify_locked -> wire_unframe_chunk, the one place where the reader runs.
    Its own message mix: _messages makes its proofs under ONE key."""
    from act_amd import capi
    L = 8
    eng = engine_factory(bench_params, L, max_batch=3, transcript=capi.TRANSCRIPT_DEVICE)
    octx = oracle.ctx(bench_params, L)
    keys = kr.make_keys(octx, "wrr")
    a, b = keys[0], keys[1]
    ring, key_epochs = [a, b], (7, 9)
    recs = [kr.spend_under(octx, sk, "wrr-%d" % i)[0] for i, sk in enumerate((a, b, a, b, keys[4], b, a))]
    t = bytearray(recs[5]); t[33] ^= 1; recs[5] = bytes(t)
    canon = eng.cbor_encode("SpendProof", b"".join(recs))
    msgs = []
    for i, rec in enumerate(recs):
        sp = _respellings(rec, L)
        msgs += [canon[i], sp[i % len(sp)]] if i % 2 else [sp[i % len(sp)], canon[i]]      # every proof twice: the second one is a double spend
    msgs += [v for v, _ in _variants("SpendProof", recs[6], L)][6:]
    N = len(msgs)
    stream = shake("wrr-rng", 128 * N)
    # the server loop over a ring: from_cbor, the first key whose refund accepts, the nullifier store with the matched key's epoch
    st, out, okey, cur, db = [], [], [], 0, {}
    for msg in msgs:
        es, rec = m.cbor_decode("SpendProof", msg, L)
        if es:
            st.append(WIRE[es]); out.append(b""); okey.append(255); continue
        v, k, _ = kr.oracle_ring_verdict(octx, ring, rec)
        if v:
            st.append(v); out.append(b""); okey.append(255); continue
        okey.append(k)
        nul = int.from_bytes(rec[:32], "little") % m.ELL
        if nul in db:
            st.append(3); out.append(b""); continue
        db[nul] = key_epochs[k]
        s2, rf = octx.refund(ring[k], rec, stream[128 * cur:128 * cur + 128]); cur += 1
        assert s2 == 0
        st.append(0); out.append(m.cbor_encode("Refund", rf, L))
    assert {0, 3, 7, 253, 254, 255} <= set(st) and {0, 1} <= set(okey)

    def redeem():
        ns = capi.NullifierSet(4 * N)
        g = capi.ReplayRng(stream)
        r = eng.redeem_cbor_keyring(ns, ring, msgs, g, capi.RNG_CALLBACK, key_epochs=key_epochs)
        keys_b, eps = ns.export_epochs()
        ns.close()
        return r, g.pos, {int.from_bytes(keys_b[32 * i:32 * i + 32], "little"): int(e) for i, e in enumerate(eps)}
    dv, hv, sd, sh = _both(eng, redeem)
    assert dv == hv and sd["read_by_host"] == 0 and sd["read_on_device"] == sh["read_by_host"] > 10

    def redeem_plain():      # the form without epochs, host transcripts, pre-drawn sequential bytes
        eng.set_transcript_mode(capi.TRANSCRIPT_HOST)
        ns = capi.NullifierSet(4 * N)
        try:
            return eng.redeem_cbor_keyring(ns, ring, msgs, stream, capi.RNG_SEQUENTIAL), len(ns)
        finally:
            ns.close(); eng.set_transcript_mode(capi.TRANSCRIPT_DEVICE)
    pv, phv, _, _ = _both(eng, redeem_plain)
    assert pv == phv == (dv[0], len(db))
    got_st, got_out, got_key = dv[0]
    assert got_st == bytes(st) and got_out == out and dv[1] == 128 * cur and dv[2] == db
    assert all(got_key[i] == okey[i] for i in range(N) if st[i] in (0, 253, 254, 255, 7, 6))      # (a double spend keeps the key it matched)
    assert eng.secret_residue() == 0


def test_a_batch_of_respelled_messages_is_read_on_the_device(engine_factory, bench_params):
    from act_amd import capi
    L, n = 8, 300
    eng = engine_factory(bench_params, L, max_batch=6, transcript=capi.TRANSCRIPT_DEVICE)
    sk = eng.private_key_random(shake("rsp-sk", 64))
    proofs = _proofs(eng, sk, 12, "rsp")
    pb = eng.proof_bytes
    recs = [bytearray(proofs[pb * i:pb * i + pb]) for i in range(12)]
    recs[5][32] ^= 1                                                    # one tampered among them
    canon = eng.cbor_encode("SpendProof", b"".join(bytes(r) for r in recs))
    sp = [_respellings(bytes(r), L) for r in recs]
    assert len({len(x) for x in sp}) == 1 and len(sp[0]) >= 10 and all(len(set(x)) == len(x) for x in sp)
    msgs = [sp[i % 12][(i + i // 12) % len(sp[0])] for i in range(n)]      # every spelling occurs, of every proof
    want = eng.verify_spend_cbor(sk, [canon[i % 12] for i in range(n)], True)
    assert set(want[0]) == {0, 7} and want[0].count(7) == n // 12
    dv, hv, sd, sh = _both(eng, lambda: eng.verify_spend_cbor(sk, msgs, True))
    assert dv == want and hv == want
    assert sd == {"seen": n, "canonical": 0, "read_on_device": n, "read_by_host": 0}
    assert sh == {"seen": n, "canonical": 0, "read_on_device": 0, "read_by_host": n}
    assert eng.secret_residue() == 0


def _irregular(rec, L):
    """messages whose code depends on points that are not in the record, or on the order of two faults"""
    es = _ents(rec, L); n = len(es)
    hd = lambda k: m._cbor_head(5, k)
    sub = lambda k2, v2, src=es: [(k, v) if k != k2 else (k2, v2) for k, v in src]
    com = dict(es)[5]; ch = len(m._cbor_head(4, L))
    bad_com = com[:ch] + com[ch:ch + 34 * (L - 1)] + BAD_PT
    z = dict(es)[15]
    z3 = z[:ch] + b"\x83" + z[ch + 1:ch + 69] + b"\x58\x20" + bytes(32) + z[ch + 69:]
    return [hd(n + 1) + m._cbor_head(0, 3) + BAD_PT + _body(es),                       # invalid point under a key that a later duplicate overwrites
            hd(n + 1) + _body(es) + m._cbor_head(0, 3) + BAD_PT,                       # ... and the other way round
            hd(n + 1) + m._cbor_head(0, 3) + dict(es)[4] + _body(es),                  # a duplicate that is valid: accepted, the last one wins
            hd(n) + _body(sub(5, m._cbor_head(4, L + 1) + com[ch:] + BAD_PT)),         # over-long Com whose extra element is invalid
            hd(n) + _body(sub(5, m._cbor_head(4, L + 1) + com[ch:] + com[ch:ch + 34])),      # over-long Com, all valid
            hd(n) + _body(sub(15, z3, sub(5, bad_com))),                               # invalid Com element in front of a 3-element z pair
            hd(n) + _body(sub(15, z3, sub(5, bad_com))[::-1])]                         # ... and behind it


def test_irregular_messages_through_the_pipeline(engine_factory, bench_params):
    import torch
    from act_amd import capi
    L = 8
    eng = engine_factory(bench_params, L, max_batch=6, transcript=capi.TRANSCRIPT_DEVICE)
    sk = eng.private_key_random(shake("irr-sk", 64))
    proofs = _proofs(eng, sk, 4, "irr")
    pb = eng.proof_bytes
    canon = eng.cbor_encode("SpendProof", proofs)
    irr = _irregular(proofs[:pb], L)
    model = [m.cbor_decode("SpendProof", x, L)[0] for x in irr]
    assert model == [3, 3, 0, 3, 2, 3, 2]
    want = bytes(WIRE.get(c, 0) for c in model)
    msgs = [canon[1]] + irr + [canon[2]]
    dv, hv, sd, _ = _both(eng, lambda: eng.verify_spend_cbor_keys(sk, msgs))
    assert dv == hv and dv[0] == bytes(1) + want + bytes(1) and sd["read_on_device"] == len(irr)
    assert eng.cbor_read("SpendProof", irr)[0] == bytes(model) == eng.cbor_decode("SpendProof", irr)[0]
    # as the only flagged messages at lanes 0 and n - 1 of a device-memory batch
    n = 300
    ps, ks = capi._in(sk, 64)
    # the nullifier of a refused message is zero, except where every field READ and the invalid point is one that never reaches the
    # record (the first two): there it is handed out as it stood on the wire, as for a regular message with an undecodable point
    keeps = {0, 1, 2}
    for fi, li in ((0, 4), (6, 1), (3, 2), (5, 5)):
        first, last = irr[fi], irr[li]
        batch = [first] + [canon[i % 4] for i in range(1, n - 1)] + [last]
        offs = np.zeros(n + 1, np.uint64); offs[1:] = np.cumsum([len(x) for x in batch], dtype=np.uint64)
        d_blob = torch.from_numpy(np.frombuffer(b"".join(batch) + b"\0", np.uint8).copy()).cuda()

        def call():
            d_st = torch.full((n,), 99, dtype=torch.uint8, device="cuda"); d_kp = torch.full((32 * n,), 9, dtype=torch.uint8, device="cuda")
            d_nul = torch.full((32 * n,), 9, dtype=torch.uint8, device="cuda"); torch.cuda.synchronize()
            eng._ck(eng.lib.act_verify_spend_cbor_keys_batch(eng.ctx, n, capi.MEM_DEVICE, ps, d_blob.data_ptr(), offs.ctypes.data, d_st.data_ptr(), d_kp.data_ptr(), d_nul.data_ptr()))
            return d_st.cpu().numpy().tobytes(), d_kp.cpu().numpy().tobytes(), d_nul.cpu().numpy().tobytes()
        dv, hv, sd, sh = _both(eng, call)
        assert dv == hv
        st, kp, nul = dv
        w0, w1 = WIRE.get(model[fi], 0), WIRE.get(model[li], 0)
        assert st == bytes([w0]) + bytes(n - 2) + bytes([w1])
        for lane, w, idx in ((0, w0, fi), (n - 1, w1, li)):
            assert (kp[32 * lane:32 * lane + 32] == bytes(32)) == (w != 0) and (nul[32 * lane:32 * lane + 32] != bytes(32)) == (idx in keeps), (fi, li, lane)
        assert sd == {"seen": n, "canonical": n - 2, "read_on_device": 2, "read_by_host": 0} and sh["read_by_host"] == 2
    assert eng.secret_residue() == 0


@pytest.mark.parametrize("unique", [False, True])
def test_admission_reads_respelled_messages_on_the_device(engine_factory, bench_params, unique):
    import torch
    from act_amd import capi
    L = 8
    eng = engine_factory(bench_params, L, max_batch=6, transcript=capi.TRANSCRIPT_DEVICE)
    sk = eng.private_key_random(shake("adr-sk", 64))
    n0 = 10
    proofs = _proofs(eng, sk, n0, "adr")
    pb = eng.proof_bytes
    recs = [proofs[pb * i:pb * i + pb] for i in range(n0)]
    canon = eng.cbor_encode("SpendProof", proofs)
    sp = [_respellings(r, L) for r in recs]
    spent = 4                                                           # proofs 0..3 are in the set before the batch arrives
    k = len(sp[0])
    batch = [sp[i][(3 * i) % k] for i in range(spent)]                  # respelled replays
    batch += [sp[i][(3 * i + 1) % k] for i in range(spent, n0)] + [canon[spent]]      # fresh ones respelled; one of them again, canonical
    batch += _irregular(recs[9], L)[:2] + [b"\xbf" + canon[8][1:], sp[0][1], sp[8][0]]      # refused by the reader; a replay; an in-batch repeat
    assert len(set(batch)) == len(batch)
    N = len(batch)
    rng = shake("adr-rng", 128 * N)
    blob = b"".join(batch)
    offs = np.zeros(N + 1, np.uint64); offs[1:] = np.cumsum([len(x) for x in batch], dtype=np.uint64)
    d_blob = torch.from_numpy(np.frombuffer(blob + b"\0", np.uint8).copy()).cuda()
    d_rng = torch.from_numpy(np.frombuffer(rng, np.uint8).copy()).cuda()
    ml = eng.cbor_size("Refund")

    def host_call():
        ns = capi.NullifierSet(1000)
        assert eng.redeem_cbor(ns, sk, canon[:spent], rng[:128 * spent], capi.RNG_SEQUENTIAL)[0] == bytes(spent)
        r = eng.redeem_cbor_admit(ns, [sk], batch, rng, capi.RNG_SEQUENTIAL, unique=unique)
        size = len(ns); ns.close()
        return r, size

    def device_call():
        ns = capi.NullifierSet(1000)
        assert eng.redeem_cbor(ns, sk, canon[:spent], rng[:128 * spent], capi.RNG_SEQUENTIAL)[0] == bytes(spent)
        d_st = torch.full((N,), 99, dtype=torch.uint8, device="cuda"); d_ok = torch.full((N,), 99, dtype=torch.uint8, device="cuda")
        d_out = torch.full((ml * N,), 9, dtype=torch.uint8, device="cuda"); torch.cuda.synchronize()
        counts = eng.admit_ptr("redeem_cbor", [sk], N, capi.MEM_DEVICE, set=ns, cbor=d_blob.data_ptr(), offsets=offs.ctypes.data, rng=d_rng.data_ptr(),
                               rng_mode=capi.RNG_SEQUENTIAL, out=d_out.data_ptr(), status=d_st.data_ptr(), out_key=d_ok.data_ptr(), unique=unique)
        size = len(ns); ns.close()
        return (d_st.cpu().numpy().tobytes(), d_out.cpu().numpy().tobytes(), d_ok.cpu().numpy().tobytes(), counts), size

    for call in (host_call, device_call):
        dv, hv, sd, sh = _both(eng, call)
        assert dv == hv, call.__name__
        (st, out, ok, counts), size = dv
        fresh = n0 - spent
        assert st[:spent] == bytes([3] * spent) and st[spent:n0] == bytes(fresh) and st[n0] == 3
        assert st[n0 + 1:] == bytes([255, 255, 254, 3, 3]) and size == n0
        # the respelled replays are shed by the screen: they are not among the verified
        assert counts["spent_before"] == spent + 1 and counts["wire_rejected"] == 3 and counts["lanes"] == N
        assert counts["verified"] == N - counts["spent_before"] - counts["wire_rejected"] - counts.get("copies", 0) and counts["accepted"] == fresh
        assert sd["read_by_host"] == 0 and sd["read_on_device"] > 0 and sh["read_on_device"] == 0 and sh["read_by_host"] == sd["read_on_device"]
    assert eng.secret_residue() == 0
