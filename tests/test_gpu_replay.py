"""Replayable redemption on the GPU: act_redeem_replay_batch / act_redeem_cbor_replay_batch / act_replay_derive_batch through the C ABI
against the model of tests/replay_cases.py (a Python set for `set`, a set of (k, K') for `receipts`) and against the definitions of
the header recomputed with oracle/pymodel.blake3.  Tokens are made as tests/test_gpu_admission.py makes them: two proofs per token
with the same nullifier and different randomness.  Both transcript modes, host and device memory, records and wire.  Every step runs
under a time limit of its own.

Rates are measured by tools/replay_probe.py; the tests here assert behaviour only."""
import contextlib
import signal

import numpy as np
import pytest

import admission_cases as ad
import replay_cases as rp
from conftest import ELL, shake, scb

pytestmark = pytest.mark.gpu

L = 8
N_TOKENS = 257
SPEND, CREDIT = 3, 9
NONCE_KEY = shake("replay-nonce-key", 32)
MODES = [("host", "host"), ("host", "device"), ("device", "host"), ("device", "device")]      # (transcripts, caller's memory)


@contextlib.contextmanager
def step(seconds, what):
    def late(signum, frame):
        raise TimeoutError("step '%s' took more than %d s" % (what, seconds))
    old = signal.signal(signal.SIGALRM, late)
    signal.alarm(seconds)
    try:
        yield
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


class World:
    """two issuer keys; token t is issued under keys[t % 2] for CREDIT and has two proofs that spend SPEND: the same nullifier,
    different randomness, so a different K'.  The prover's PreRefunds are kept: a refund must convert into the next token."""

    def __init__(self, eng, n=N_TOKENS):
        self.eng, self.pb, self.n = eng, eng.proof_bytes, n
        self.keys = [eng.private_key_random(shake("rp-sk%d" % i, 64)) for i in range(2)]
        self.owner = [t % 2 for t in range(n)]
        pre = eng.pre_issuance_random(shake("rp-pre", 128 * n)); req = eng.request(pre, shake("rp-rq", 128 * n))
        tok = np.zeros((n, 160), np.uint8)
        for k in range(2):
            sel = [i for i in range(n) if self.owner[i] == k]
            rq = b"".join(req[128 * i:128 * i + 128] for i in sel); pr = b"".join(pre[64 * i:64 * i + 64] for i in sel)
            st, resp = eng.issue(self.keys[k], rq, scb(CREDIT) * len(sel), shake("rp-ir%d" % k, 128 * len(sel)))
            assert st == bytes(len(sel))
            st, t = eng.issuance_to_credit_token(pr, self.keys[k][32:], rq, resp)
            assert st == bytes(len(sel))
            tok[sel] = np.frombuffer(t, np.uint8).reshape(len(sel), 160)
        self.proofs, self.prerefunds = [], []
        for v in range(2):
            st, p, pr = eng.prove_spend_seeded(tok.tobytes(), scb(SPEND) * n, shake("rp-seed%d" % v, 32))
            assert st == bytes(n)
            self.proofs.append(np.frombuffer(p, np.uint8).reshape(n, self.pb).copy())
            self.prerefunds.append(np.frombuffer(pr, np.uint8).reshape(n, 96).copy())
        assert (self.proofs[0][:, :32] == self.proofs[1][:, :32]).all() and not (self.proofs[0] == self.proofs[1]).all(axis=1).any()
        self.k = [int.from_bytes(self.proofs[0][i, :32].tobytes(), "little") % ELL for i in range(n)]
        assert len(set(self.k)) == n

    def proof(self, t, variant=0, how=None):
        p = self.proofs[variant][t].copy()
        if how == "tampered":
            p[self.pb - 32] ^= 1
        elif how == "undecodable":
            p[64:96] = 0xFF
        return p.tobytes()

    def lane(self, t, variant=0, how=None, ring=(0, 1)):
        """the model's view of proof (t, variant) against a ring of key numbers"""
        if how == "undecodable":
            return rp.Lane(self.k[t], (t, variant), 255, rp.KEY_NONE)
        if how == "tampered" or self.owner[t] not in ring:
            return rp.Lane(self.k[t], (t, variant), 7, rp.KEY_NONE)
        return rp.Lane(self.k[t], (t, variant), 0, list(ring).index(self.owner[t]))


_world = {}


def world(eng):
    if id(eng) not in _world:
        with step(120, "tokens and proofs"):
            _world[id(eng)] = World(eng)
    return _world[id(eng)]


def setup(engine_factory, bench_params, mode):
    from act_amd import capi
    eng = engine_factory(bench_params, L, max_batch=4096, transcript=capi.TRANSCRIPT_HOST if mode == "host" else capi.TRANSCRIPT_DEVICE)
    return capi, eng, world(eng)


class Dev:
    """device-memory callers: torch tensors as the caller's HBM"""

    def __init__(self):
        import torch
        self.t = torch

    def up(self, b):
        return self.t.from_numpy(np.frombuffer(bytes(b) + b"\0", np.uint8).copy()).cuda()

    def new(self, n, fill):
        return self.t.full((max(1, n),), fill, dtype=self.t.uint8, device="cuda")

    def down(self, t, n):
        return t.cpu().numpy().tobytes()[:n]


def call_replay(eng, mem, ns, rs, ring, recs=None, msgs=None, sign_key=-1, key_epochs=None, nonce_key=NONCE_KEY, want_rc=0):
    """one replay call in either memory kind and either form -> (statuses, out: list of records or messages (b"" where not signed),
    out_key, replayed, counts).  Status bytes start as 99: a call that writes no status leaves them."""
    from act_amd import capi
    wire = msgs is not None
    n = len(msgs) if wire else len(recs)
    ob = eng.cbor_size("Refund") if wire else 128
    if mem == "host":
        if wire:
            rc, st, out, ok, rep, c = eng.redeem_cbor_replay(ns, rs, ring, msgs, nonce_key, sign_key, key_epochs, raw=True)
        else:
            rc, st, blob, ok, rep, c = eng.redeem_replay(ns, rs, ring, b"".join(recs), nonce_key, sign_key, key_epochs, raw=True)
            out = [blob[128 * i:128 * i + 128] if st[i] == 0 else b"" for i in range(n)]
            assert all(st[i] == 0 or st[i] == 99 or not any(blob[128 * i:128 * i + 128]) for i in range(n)), "a failed lane's record is not zero"
    else:
        d = Dev()
        src = d.up(b"".join(msgs) if wire else b"".join(recs))
        offs = np.zeros(n + 1, np.uint64)
        if wire:
            offs[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
        o, s, k, r = d.new(ob * n, 7), d.new(n, 99), d.new(n, 77), d.new(n, 55)
        d.t.cuda.synchronize()
        p = dict(set=ns, receipts=rs, nonce_key=nonce_key, out=o.data_ptr(), status=s.data_ptr(), out_key=k.data_ptr(), replayed=r.data_ptr(), key_epochs=key_epochs,
                 sign_key=sign_key, raw=True)
        if wire:
            rc, c = eng.replay_ptr("redeem_cbor", ring, n, capi.MEM_DEVICE, cbor=src.data_ptr(), offsets=offs.ctypes.data, **p)
        else:
            rc, c = eng.replay_ptr("redeem", ring, n, capi.MEM_DEVICE, proofs=src.data_ptr(), **p)
        st, blob, ok, rep = d.down(s, n), d.down(o, ob * n), d.down(k, n), d.down(r, n)
        out = [blob[ob * i:ob * i + ob] if st[i] == 0 else b"" for i in range(n)]
        assert all(st[i] == 0 or st[i] == 99 or not any(blob[ob * i:ob * i + ob]) for i in range(n)), "a failed lane's slot is not zero"
    assert rc == want_rc, (rc, eng.lib.act_last_error(eng.ctx))
    return st, out, ok, rep, c


def keys_of(s):
    """the set's keys, sorted (one export: its order is unspecified and may differ from call to call)"""
    blob = s.export()
    return sorted(blob[i:i + 32] for i in range(0, len(blob), 32))


def against_model(got, lanes, spent, receipts):
    st, out, ok, rep, c = got
    mst, mok, mrep, mc = rp.model(lanes, spent, receipts)
    assert (list(st), list(ok), list(rep), c) == (mst, mok, mrep, mc)


def expected_refunds(eng, ring, recs, kidx):
    """the definition: act_refund_sign_keyring_batch over out_kprime of act_verify_spend_keyring_batch with the nonces of the header,
    recomputed with pymodel.blake3 -> (records, nonces, kprime)"""
    from act_amd import capi
    n = len(recs)
    st, ok, kp = eng.verify_spend_keyring(ring, b"".join(recs), want_kprime=True)
    assert st == bytes(n)
    non = b"".join(rp.nonce(NONCE_KEY, ring[kidx[i]], recs[i][:32], kp[32 * i:32 * i + 32]) for i in range(n))
    st, ref = eng.refund_sign_keyring(ring, bytes(kidx), kp, bytes(n), non, capi.RNG_PER_LANE)
    assert st == bytes(n)
    return [ref[128 * i:128 * i + 128] for i in range(n)], non, kp


# ---- retry and bytes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65, 257])
@pytest.mark.parametrize("mode,mem,wire", [("host", "host", False), ("device", "device", False), ("device", "host", True), ("host", "device", True)])
def test_a_retried_batch_gets_its_refunds_again(engine_factory, bench_params, mode, mem, wire, n):
    capi, eng, w = setup(engine_factory, bench_params, mode)
    ring = w.keys
    recs = [w.proof(t) for t in range(n)]
    kw = dict(msgs=eng.cbor_encode("SpendProof", b"".join(recs))) if wire else dict(recs=recs)
    lanes = [w.lane(t) for t in range(n)]
    spent, receipts = set(), set()
    ns, rs = capi.NullifierSet(1000), capi.NullifierSet(1000)
    with step(60, "first call"):
        first = call_replay(eng, mem, ns, rs, ring, **kw)
        against_model(first, lanes, spent, receipts)
        assert first[0] == bytes(n) and first[3] == bytes(n) and first[4]["fresh"] == n and (len(ns), len(rs)) == (n, n)
    with step(60, "the same batch again"):
        again = call_replay(eng, mem, ns, rs, ring, **kw)
        against_model(again, lanes, spent, receipts)
        assert again[0] == bytes(n) and again[3] == b"\1" * n and again[4]["replayed"] == n
        assert again[1] == first[1] and (len(ns), len(rs)) == (n, n)
    with step(60, "the definition"):
        kidx = [w.owner[t] for t in range(n)]                       # ACT_SIGN_MATCHED: the ring is (key 0, key 1)
        want, non, kp = expected_refunds(eng, ring, recs, kidx)
        got = first[1]
        if wire:
            dst, dec = eng.cbor_decode("Refund", got)
            assert dst == bytes(n)
            got = [dec[128 * i:128 * i + 128] for i in range(n)]
        assert got == want
        tags, dn = eng.replay_derive(ring, bytes(kidx), NONCE_KEY, b"".join(r[:32] for r in recs), kp, bytes(n))
        assert dn == non and tags == b"".join(rp.tag(recs[i][:32], kp[32 * i:32 * i + 32]) for i in range(n))
        assert keys_of(rs) == sorted(tags[32 * i:32 * i + 32] for i in range(n))
        for k in range(2):                                          # every refund converts into the holder's next token
            sel = [t for t in range(n) if w.owner[t] == k]
            if sel:
                cst, _ = eng.refund_to_credit_token(b"".join(w.prerefunds[0][t].tobytes() for t in sel), b"".join(recs[t] for t in sel),
                                                    b"".join(got[t] for t in sel), ring[k][32:])
                assert cst == bytes(len(sel))
    with step(60, "the existing call on the same set"):
        pst, pout, pok = eng.redeem_keyring(ns, ring, b"".join(recs), shake("rp-plain", 128 * n), capi.RNG_PER_LANE, key_epochs=[0, 0])
        assert pst == bytes([3]) * n and not any(pout) and len(ns) == n
    ns.close(); rs.close()
    assert eng.secret_residue() == 0


def test_derive_in_device_memory_and_lanes_that_take_no_part(engine_factory, bench_params):
    capi, eng, w = setup(engine_factory, bench_params, "device")
    n = 257
    recs = b"".join(w.proof(t) for t in range(n))
    kp, st = shake("rp-derive-kp", 32 * n), bytes(7 if i % 5 == 3 else 0 for i in range(n))
    kidx = bytes(255 if i % 7 == 6 else i % 2 for i in range(n))
    d = Dev()
    with step(60, "derive"):
        src, dkp, dst, dki, tags, non = d.up(recs), d.up(kp), d.up(st), d.up(kidx), d.new(32 * n, 9), d.new(128 * n, 9)
        d.t.cuda.synchronize()
        eng.replay_derive_ptr(w.keys, n, capi.MEM_DEVICE, NONCE_KEY, dki.data_ptr(), src.data_ptr(), w.pb, dkp.data_ptr(), dst.data_ptr(), tags.data_ptr(), non.data_ptr())
        tags, non = d.down(tags, 32 * n), d.down(non, 128 * n)
        htags, hnon = eng.replay_derive(w.keys, kidx, NONCE_KEY, recs, kp, st, stride=w.pb)
    assert (tags, non) == (htags, hnon)
    for i in range(n):
        k, p = recs[w.pb * i:w.pb * i + 32], kp[32 * i:32 * i + 32]
        live = st[i] == 0 and kidx[i] < 2
        assert tags[32 * i:32 * i + 32] == (rp.tag(k, p) if live else bytes(32)), i
        assert non[128 * i:128 * i + 128] == (rp.nonce(NONCE_KEY, w.keys[kidx[i]], k, p) if live else bytes(128)), i
    assert eng.secret_residue() == 0


# ---- a real double spend ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,mem", MODES)
def test_the_other_proof_of_a_redeemed_token_is_a_double_spend(engine_factory, bench_params, mode, mem):
    capi, eng, w = setup(engine_factory, bench_params, mode)
    n = 65
    ring, spent, receipts = w.keys, set(), set()
    ns, rs = capi.NullifierSet(1000), capi.NullifierSet(1000)
    v0, v1 = [w.proof(t, 0) for t in range(n)], [w.proof(t, 1) for t in range(n)]
    with step(60, "variant 0, then variant 1"):
        first = call_replay(eng, mem, ns, rs, ring, recs=v0)
        against_model(first, [w.lane(t, 0) for t in range(n)], spent, receipts)
        before = keys_of(rs)
        other = call_replay(eng, mem, ns, rs, ring, recs=v1)
        against_model(other, [w.lane(t, 1) for t in range(n)], spent, receipts)
        assert other[0] == bytes([3]) * n and other[1] == [b""] * n and other[3] == bytes(n) and other[4]["double_spend"] == n
        assert list(other[2]) == [w.owner[t] for t in range(n)]     # a double spend keeps the key it matched
        assert (len(ns), len(rs)) == (n, n) and keys_of(rs) == before
    with step(60, "afterwards, both in one batch"):
        mixed = call_replay(eng, mem, ns, rs, ring, recs=v0 + v1)
        against_model(mixed, [w.lane(t, 0) for t in range(n)] + [w.lane(t, 1) for t in range(n)], spent, receipts)
        assert mixed[0] == bytes(n) + bytes([3]) * n and mixed[3] == b"\1" * n + bytes(n) and mixed[1][:n] == first[1]
        assert (len(ns), len(rs)) == (n, n)
    ns.close(); rs.close()
    assert eng.secret_residue() == 0


# ---- one batch with everything in it ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,mem", MODES)
@pytest.mark.parametrize("wire", [False, True])
def test_one_batch_fresh_replay_double_spend_tampered_undecodable(engine_factory, bench_params, mode, mem, wire):
    capi, eng, w = setup(engine_factory, bench_params, mode)
    t = 4
    recs = [w.proof(t), w.proof(t), w.proof(t, 1), w.proof(t, 0, "tampered"), w.proof(t + 1, 0, "undecodable")]
    lanes = [w.lane(t), w.lane(t), w.lane(t, 1), w.lane(t, 0, "tampered"), w.lane(t + 1, 0, "undecodable")]
    kw = dict(msgs=eng.cbor_encode("SpendProof", b"".join(recs))) if wire else dict(recs=recs)
    spent, receipts = set(), set()
    ns, rs = capi.NullifierSet(1000), capi.NullifierSet(1000)
    with step(60, "the batch"):
        got = call_replay(eng, mem, ns, rs, w.keys, **kw)
        against_model(got, lanes, spent, receipts)
        st, out, ok, rep, c = got
        assert list(st) == [0, 0, 3, 7, 255] and list(rep) == [0, 1, 0, 0, 0] and out[1] == out[0] and out[0]
        assert (len(ns), len(rs)) == (1, 1) and rs.export() == rp.tag(recs[0][:32], eng.verify_spend_keyring(w.keys, recs[0], want_kprime=True)[2])
        assert c == dict(lanes=5, rejected_by_verification=2, fresh=1, replayed=1, double_spend=1, unanswered=0)
    ns.close(); rs.close()
    assert eng.secret_residue() == 0


# ---- wire: another spelling of a redeemed message ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,mem", [("host", "device"), ("device", "host")])
def test_a_respelled_retry_gets_the_identical_refund_message(engine_factory, bench_params, mode, mem):
    capi, eng, w = setup(engine_factory, bench_params, mode)
    n = 65
    recs = [w.proof(t) for t in range(n)]
    canon = eng.cbor_encode("SpendProof", b"".join(recs))
    other = [ad.respelled(r, L) for r in recs]
    assert all(a != b for a, b in zip(canon, other))
    try:
        for reader in (capi.WIRE_READER_DEVICE, capi.WIRE_READER_HOST):
            eng.set_wire_reader(reader)
            ns, rs = capi.NullifierSet(1000), capi.NullifierSet(1000)
            spent, receipts = set(), set()
            with step(60, "canonical, then respelled, reader %d" % reader):
                first = call_replay(eng, mem, ns, rs, w.keys, msgs=canon)
                against_model(first, [w.lane(t) for t in range(n)], spent, receipts)
                again = call_replay(eng, mem, ns, rs, w.keys, msgs=other)
                against_model(again, [w.lane(t) for t in range(n)], spent, receipts)
                assert again[3] == b"\1" * n and again[1] == first[1] and all(first[1]) and (len(ns), len(rs)) == (n, n)
            ns.close(); rs.close()
    finally:
        eng.set_wire_reader(capi.WIRE_READER_DEVICE)
    assert eng.secret_residue() == 0


# ---- a ring of two keys ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,mem", MODES)
def test_ring_of_two_matched_key_and_a_moved_sign_key(engine_factory, bench_params, mode, mem):
    capi, eng, w = setup(engine_factory, bench_params, mode)
    n = 65
    ring, recs, lanes = w.keys, [w.proof(t) for t in range(n)], [w.lane(t) for t in range(n)]
    spent, receipts = set(), set()
    ns, rs = capi.NullifierSet(1000), capi.NullifierSet(1000)
    with step(60, "matched key, twice"):
        first = call_replay(eng, mem, ns, rs, ring, recs=recs, sign_key=capi.SIGN_MATCHED)
        against_model(first, lanes, spent, receipts)
        again = call_replay(eng, mem, ns, rs, ring, recs=recs, sign_key=capi.SIGN_MATCHED)
        against_model(again, lanes, spent, receipts)
        assert again[1] == first[1] and again[3] == b"\1" * n
    with step(60, "the retry signed with key 1"):
        moved = call_replay(eng, mem, ns, rs, ring, recs=recs, sign_key=1)
        against_model(moved, lanes, spent, receipts)
        assert moved[0] == bytes(n) and moved[3] == b"\1" * n and list(moved[2]) == [w.owner[t] for t in range(n)]
        # a token of key 0 is now signed with another key: other nonces, another signature; a token of key 1 was signed with key 1 before
        assert all((moved[1][t] != first[1][t]) == (w.owner[t] == 0) for t in range(n))
        assert moved[1] == expected_refunds(eng, ring, recs, [1] * n)[0]
        pre, blob, ref = b"".join(w.prerefunds[0][t].tobytes() for t in range(n)), b"".join(recs), b"".join(moved[1])
        assert eng.refund_to_credit_token(pre, blob, ref, ring[1][32:])[0] == bytes(n)
        assert all(eng.refund_to_credit_token(pre, blob, ref, ring[0][32:])[0])                  # under w[1] only: w[0] accepts none of them
    ns.close(); rs.close()
    assert eng.secret_residue() == 0


# ---- epochs ---------------------------------------------------------------------------------------------------------------------------------------
def _pairs(s):
    keys, eps = s.export_epochs()
    return sorted((keys[32 * i:32 * i + 32], int(eps[i])) for i in range(len(eps)))


@pytest.mark.parametrize("mode,mem", [("host", "host"), ("device", "device")])
def test_receipts_carry_the_matched_keys_epoch_and_retire_with_it(engine_factory, bench_params, mode, mem):
    capi, eng, w = setup(engine_factory, bench_params, mode)
    n = 65
    ring, epochs, recs = w.keys, [101, 102], [w.proof(t) for t in range(n)]
    ns, rs = capi.NullifierSet(1000), capi.NullifierSet(1000)
    spent, receipts = set(), set()
    with step(60, "redeem under epochs, sign with key 0"):
        got = call_replay(eng, mem, ns, rs, ring, recs=recs, sign_key=0, key_epochs=epochs)
        against_model(got, [w.lane(t) for t in range(n)], spent, receipts)
        kp = eng.verify_spend_keyring(ring, b"".join(recs), want_kprime=True)[2]
        assert _pairs(ns) == sorted((rp.reduced(recs[t][:32]), epochs[w.owner[t]]) for t in range(n))      # the key it MATCHED, not the key it is signed with
        assert _pairs(rs) == sorted((rp.tag(recs[t][:32], kp[32 * t:32 * t + 32]), epochs[w.owner[t]]) for t in range(n))
    with step(60, "retire key 1 on both sets"):
        gone = sum(1 for t in range(n) if w.owner[t] == 1)
        assert ns.retire_epoch(102) == gone and rs.retire_epoch(102) == gone and (len(ns), len(rs)) == (n - gone, n - gone)
        rc_st = call_replay(eng, mem, ns, rs, ring, recs=recs, sign_key=0, key_epochs=epochs, want_rc=1)      # a retired epoch: refused as a whole by either set
        assert rc_st[0] == bytes([99]) * n and (len(ns), len(rs)) == (n - gone, n - gone)
    ns.close(); rs.close()
    assert eng.secret_residue() == 0


# ---- the failure contract ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,mem,wire", [("host", "host", False), ("device", "device", False), ("host", "device", True), ("device", "host", True)])
def test_recorded_unsigned_is_repaired_by_calling_again(engine_factory, bench_params, mode, mem, wire):
    capi, eng, w = setup(engine_factory, bench_params, mode)
    n = 65
    recs = [w.proof(t, 0, "tampered" if t == 7 else None) for t in range(n)]
    lanes = [w.lane(t, 0, "tampered" if t == 7 else None) for t in range(n)]
    kw = dict(msgs=eng.cbor_encode("SpendProof", b"".join(recs))) if wire else dict(recs=recs)
    ns, rs = capi.NullifierSet(1000), capi.NullifierSet(1000)
    with step(60, "a signature step that fails"):
        assert eng.lib.act_debug_fail_next_signs(eng.ctx, 1) == 0
        st, out, ok, rep, c = call_replay(eng, mem, ns, rs, w.keys, want_rc=2, **kw)
        assert list(st) == [7 if t == 7 else 251 for t in range(n)] and out == [b""] * n and (len(ns), len(rs)) == (n - 1, n - 1)
        assert c == dict(lanes=n, rejected_by_verification=1, fresh=0, replayed=0, double_spend=0, unanswered=n - 1)
        assert eng.secret_residue() == 0
    with step(60, "the same call again, and an undisturbed run"):
        spent, receipts = {ln.k for ln in lanes if not ln.verdict}, {(ln.k, ln.kprime) for ln in lanes if not ln.verdict}
        again = call_replay(eng, mem, ns, rs, w.keys, **kw)
        against_model(again, lanes, spent, receipts)
        assert list(again[3]) == [0 if t == 7 else 1 for t in range(n)]
        ns2, rs2 = capi.NullifierSet(1000), capi.NullifierSet(1000)
        clean = call_replay(eng, mem, ns2, rs2, w.keys, **kw)
        assert again[1] == clean[1] and clean[3] == bytes(n)
        ns2.close(); rs2.close()
    ns.close(); rs.close()
    assert eng.secret_residue() == 0


@pytest.mark.parametrize("mem", ["host", "device"])
def test_whole_call_refusals_write_nothing(engine_factory, bench_params, mem):
    capi, eng, w = setup(engine_factory, bench_params, "device")
    n = 65
    recs = [w.proof(t) for t in range(n)]
    ns, small = capi.NullifierSet(1000), capi.NullifierSet(500)     # 1024 slots: room for 512 keys
    with step(60, "a receipts set without room"):
        filler = b"".join(scb(1000 + i) for i in range(512 - n + 1))
        assert small.check_and_insert(filler) == bytes(512 - n + 1)
        st, out, ok, rep, c = call_replay(eng, mem, ns, small, w.keys, recs=recs, want_rc=1)
        assert st == bytes([99]) * n and (len(ns), len(small)) == (0, 512 - n + 1) and c["lanes"] == 0
        assert b"receipts" in eng.lib.act_last_error(eng.ctx)
        assert eng.secret_residue() == 0
    with step(60, "the other refusals"):
        class Null:
            h = None
        for rs, key in ((Null, NONCE_KEY), (ns, NONCE_KEY), (small, None)):
            if key is None and mem == "device":
                continue                                            # (the pointer helper wants the key's bytes; the host form passes NULL)
            if key is None:
                p0 = np.frombuffer(b"".join(recs), np.uint8); o = np.zeros(128 * n, np.uint8); s = np.full(n, 99, np.uint8); k = np.zeros(n, np.uint8)
                rc = eng.lib.act_redeem_replay_batch(eng.ctx, ns.h, small.h, n, capi.MEM_HOST, b"".join(w.keys), 2, None, -1, p0.ctypes.data, None, o.ctypes.data,
                                                     s.ctypes.data, k.ctypes.data, None, None)
                assert rc == 1 and s.tobytes() == bytes([99]) * n
            else:
                st = call_replay(eng, mem, ns, rs, w.keys, recs=recs, nonce_key=key, want_rc=1)[0]
                assert st == bytes([99]) * n
        assert len(ns) == 0
    with step(60, "one more key of room is enough"):
        small2 = capi.NullifierSet(500)
        assert small2.check_and_insert(filler[32:]) == bytes(512 - n)
        got = call_replay(eng, mem, ns, small2, w.keys, recs=recs)
        assert got[0] == bytes(n) and (len(ns), len(small2)) == (n, 512)
        small2.close()
    ns.close(); small.close()
    assert eng.secret_residue() == 0


# ---- restart: both sets saved and restored, another context ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,mem", [("host", "host"), ("device", "device")])
def test_a_retry_after_a_restart_replays_byte_identically(engine_factory, bench_params, tmp_path, mode, mem):
    capi, eng, w = setup(engine_factory, bench_params, mode)
    n = 65
    recs, epochs = [w.proof(t) for t in range(n)], [7, 8]
    ns, rs = capi.NullifierSet(1000), capi.NullifierSet(1000)
    with step(60, "redeem and save"):
        first = call_replay(eng, mem, ns, rs, w.keys, recs=recs, key_epochs=epochs)
        ns.save(str(tmp_path / "set.snap")); rs.save(str(tmp_path / "receipts.snap"))
        ns.close(); rs.close()
    with step(120, "a new context, both sets restored"):
        eng2 = capi.Engine(bench_params, L, max_batch=256)
        eng2.set_transcript_mode(capi.TRANSCRIPT_HOST if mode == "host" else capi.TRANSCRIPT_DEVICE)
        ns2, rs2 = capi.NullifierSet.restore(str(tmp_path / "set.snap"), 1000), capi.NullifierSet.restore(str(tmp_path / "receipts.snap"), 1000)
        again = call_replay(eng2, mem, ns2, rs2, w.keys, recs=recs, key_epochs=epochs)
        assert again[0] == bytes(n) and again[3] == b"\1" * n and again[1] == first[1] and again[4]["replayed"] == n
        assert eng2.secret_residue() == 0
        ns2.close(); rs2.close(); eng2.close()


# ---- the Python API --------------------------------------------------------------------------------------------------------------------------------
def test_the_python_api_hands_a_retry_its_refund_again(engine_factory, bench_params):
    from act_amd import api
    capi, eng, w = setup(engine_factory, bench_params, "host")
    params = api.Params(bench_params)
    ring = api.Keyring([api.PrivateKey(k) for k in w.keys], epochs=[11, 12])
    db, receipts = api.NullifierDb(1 << 10), api.NullifierDb(1 << 10)
    proofs = [api.SpendProof(w.proof(t), L) for t in range(5)] + [api.SpendProof(w.proof(0, 1), L)]
    with step(120, "ring, records and wire"):
        res, keys, rep = ring.redeem_replay_batch(params, db, receipts, proofs, NONCE_KEY)
        assert [isinstance(r, api.Refund) for r in res] == [True] * 5 + [False] and res[5].code == 3
        assert keys == [w.owner[t] for t in range(5)] + [0] and rep == [False] * 6 and (len(db), len(receipts)) == (5, 5)
        assert ring.last_replay_counts == dict(lanes=6, rejected_by_verification=0, fresh=5, replayed=0, double_spend=1, unanswered=0)
        res2, keys2, rep2 = ring.redeem_replay_batch(params, db, receipts, proofs, NONCE_KEY)
        assert [r.record for r in res2[:5]] == [r.record for r in res[:5]] and rep2 == [True] * 5 + [False] and res2[5].code == 3
        msgs = [p.to_cbor(params) for p in proofs[:5]]
        out, keys3, rep3 = ring.redeem_replay_cbor_batch(params, db, receipts, msgs, NONCE_KEY, L)
        assert out == eng.cbor_encode("Refund", b"".join(r.record for r in res[:5])) and rep3 == [True] * 5 and (len(db), len(receipts)) == (5, 5)
    with step(120, "one key"):
        sk = api.PrivateKey(w.keys[0])
        db1, receipts1 = api.NullifierDb(1 << 10), api.NullifierDb(1 << 10)
        mine = [api.SpendProof(w.proof(t), L) for t in (0, 2, 4)]
        first, rep = sk.redeem_replay_batch(params, db1, receipts1, mine, NONCE_KEY)
        again, rep2 = sk.redeem_replay_batch(params, db1, receipts1, mine, NONCE_KEY)
        assert [r.record for r in again] == [r.record for r in first] and (rep, rep2) == ([False] * 3, [True] * 3)
        assert [r.record for r in first] == [res[t].record for t in (0, 2, 4)]       # a ring of one signs what the ring signed with the matched key
