"""Request binding on the GPU: act_prove_spend_bound_batch and act_verify_spend_keyring_bound_batch through the C ABI.
Proof bytes against the committed fixture and the big-integer model of tests/bound_cases.py; the challenge recomputed from the engine's
own unbound pre-image with oracle/pymodel.blake3; round trips and refusals over both transcript modes, both memory kinds, rings of one
and three keys; bind = NULL against the calls the new ones extend; a call that spend_schedule cuts into chunks.  The redemption calls
are in tests/test_gpu_bound_redeem.py.  Every step runs under a time limit of its own."""
import json
import os

import numpy as np
import pytest

import pymodel as pm

import bound_cases as bc
from conftest import GOLDEN, scb, shake
from test_gpu_replay import Dev, step

pytestmark = pytest.mark.gpu

MODES = [("host", "host"), ("host", "device"), ("device", "host"), ("device", "device")]      # (transcripts, caller's memory)
CREDIT, SPEND = 9, 2


def engine(engine_factory, h, L, mode, max_batch=4096):
    from act_amd import capi
    return capi, engine_factory(h, L, max_batch=max_batch, transcript=capi.TRANSCRIPT_HOST if mode == "host" else capi.TRANSCRIPT_DEVICE)


def prove(eng, mem, tok, s, rng, bind="absent"):
    """prove_spend in either memory kind; bind: n * 32 bytes, None (the bound call with NULL) or "absent" (act_prove_spend_batch)"""
    from act_amd import capi
    n = len(tok) // 160
    if mem == "host":
        return eng.prove_spend(tok, s, rng) if bind == "absent" else eng.prove_spend(tok, s, rng, bind=bind)
    d = Dev()
    dt, ds, dr = d.up(tok), d.up(s), d.up(rng)
    db = d.up(bind) if bind not in ("absent", None) else None
    o, pr, st = d.new(eng.proof_bytes * n, 7), d.new(96 * n, 7), d.new(n, 99)
    d.t.cuda.synchronize()
    if bind == "absent":
        eng._ck(eng.lib.act_prove_spend_batch(eng.ctx, n, capi.MEM_DEVICE, dt.data_ptr(), ds.data_ptr(), dr.data_ptr(), o.data_ptr(), pr.data_ptr(), st.data_ptr()))
    else:
        eng._ck(eng.lib.act_prove_spend_bound_batch(eng.ctx, n, capi.MEM_DEVICE, dt.data_ptr(), ds.data_ptr(), dr.data_ptr(), db.data_ptr() if db is not None else None,
                                                    o.data_ptr(), pr.data_ptr(), st.data_ptr()))
    return d.down(st, n), d.down(o, eng.proof_bytes * n), d.down(pr, 96 * n)


def verify(eng, mem, ring, proofs, bind="absent"):
    """the ring verification in either memory kind -> (statuses, out_key, enc(K'))"""
    from act_amd import capi
    n = len(proofs) // eng.proof_bytes
    if mem == "host":
        return eng.verify_spend_keyring(ring, proofs, True) if bind == "absent" else eng.verify_spend_keyring(ring, proofs, True, bind=bind)
    d = Dev()
    dp = d.up(proofs)
    db = d.up(bind) if bind not in ("absent", None) else None
    st, ok, kp = d.new(n, 99), d.new(n, 77), d.new(32 * n, 7)
    d.t.cuda.synchronize()
    p = dict(proofs=dp.data_ptr(), status=st.data_ptr(), out_key=ok.data_ptr(), kprime=kp.data_ptr())
    if bind != "absent":
        p["bind"] = db.data_ptr() if db is not None else None
    eng.keyring_ptr("verify", ring, n, capi.MEM_DEVICE, **p)
    return d.down(st, n), d.down(ok, n), d.down(kp, 32 * n)


class World:
    """n tokens under one issuer key (the LAST key of the ring of three), their rng bytes and bindings, and per token the bound proof,
    the unbound proof from the same rng bytes (same commitments, so the same K') and enc(K')"""

    def __init__(self, eng, n, tag):
        self.eng, self.n, self.pb = eng, n, eng.proof_bytes
        self.own = eng.private_key_random(shake(tag + "-own", 64))
        self.ring3 = [eng.private_key_random(shake(tag + "-other%d" % i, 64)) for i in range(2)] + [self.own]
        pre = eng.pre_issuance_random(shake(tag + "-pre", 128 * n)); req = eng.request(pre, shake(tag + "-rq", 128 * n))
        st, resp = eng.issue(self.own, req, scb(CREDIT) * n, shake(tag + "-ir", 128 * n))
        assert st == bytes(n)
        st, self.tok = eng.issuance_to_credit_token(pre, self.own[32:], req, resp)
        assert st == bytes(n)
        self.s = scb(SPEND) * n
        self.rng = shake(tag + "-pr", eng.prove_rng_bytes * n)
        self.binds = [shake(tag + "-bind%d" % i, 32) for i in range(n)]
        st, self.bound, self.prer = eng.prove_spend(self.tok, self.s, self.rng, bind=b"".join(self.binds))
        assert st == bytes(n)
        st, self.plain, prer = eng.prove_spend(self.tok, self.s, self.rng)
        assert st == bytes(n) and prer == self.prer
        st, ok, self.kprime = eng.verify_spend_keyring([self.own], self.plain, True)
        assert st == bytes(n) and ok == bytes(n)

    def proofs(self, n, bound=True):
        return (self.bound if bound else self.plain)[:self.pb * n]


_worlds = {}


def world(eng, L, n):
    if (id(eng), n) not in _worlds:
        with step(120, "tokens and proofs"):
            _worlds[(id(eng), n)] = World(eng, n, "bound-gpu-%d" % L)
    return _worlds[(id(eng), n)]


# ---- 1. the model and the fixture -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,mem", MODES)
@pytest.mark.parametrize("L", [5, 10, 22])
def test_bound_proofs_are_the_models_bytes(engine_factory, mode, mem, L):
    c = bc.case(L, "bound-fixture") if L == bc.FIXTURE_L else bc.case(L)
    capi, eng = engine(engine_factory, c["h"], L, mode)
    with step(30, "prove, bound and unbound"):
        st, proof, prer = prove(eng, mem, c["tok_rec"], scb(c["s"]), c["rng"], c["bind"])
        st0, plain, prer0 = prove(eng, mem, c["tok_rec"], scb(c["s"]), c["rng"])
    assert (st, st0) == (b"\0", b"\0")
    assert proof == c["proof_rec"] and prer == c["prerefund"] and plain == c["plain_rec"] and prer0 == prer
    if L == bc.FIXTURE_L:
        with open(os.path.join(GOLDEN, "bound_spend.json")) as f:
            fx = json.load(f)
        assert (c["h"].hex(), c["tok_rec"].hex(), c["rng"].hex(), c["bind"].hex()) == (fx["params"], fx["token"], fx["rng"], fx["binding"])
        assert proof.hex() == fx["proof"] and prer.hex() == fx["prerefund"] and proof[32 * (4 + L):32 * (5 + L)].hex() == fx["gamma"]
    with step(30, "verify"):
        assert verify(eng, mem, [c["sk_rec"]], proof, c["bind"])[:2] == (b"\0", b"\0")
        assert verify(eng, mem, [c["sk_rec"]], proof)[:2] == (b"\x07", b"\xff")
    assert eng.secret_residue() == 0


# ---- 2. the pre-image, independently ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["host", "device"])
def test_the_challenge_is_the_hash_of_the_unbound_preimage_and_the_binding(engine_factory, bench_params, mode):
    """L = 128, n = 3.  A plain ring verification of the bound proofs rejects them and leaves their unbound pre-images; each, followed by
    _lp(bind) and hashed with pymodel.blake3, reduces to the proof's gamma"""
    L, n = 128, 3
    capi, eng = engine(engine_factory, bench_params, L, mode)
    w = world(eng, L, 65)
    proofs = w.proofs(n)
    with step(30, "plain verify and its transcripts"):
        st, ok, _ = eng.verify_spend_keyring([w.own], proofs, True)
        trs = eng.last_spend_transcripts(n)
    assert st == b"\x07" * n and len(trs) == n and len(trs[0]) == bc.tr_bytes(L)
    for i in range(n):
        gamma = proofs[w.pb * i + 32 * (4 + L):][:32]
        assert pm.sc_bytes(pm.sc_from_wide(pm.blake3(trs[i] + bc.lp(w.binds[i]), 64))) == gamma, i
        assert pm.sc_bytes(pm.sc_from_wide(pm.blake3(trs[i], 64))) != gamma


# ---- 3. round trip and refusals ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,mem", MODES)
@pytest.mark.parametrize("L", [5, 10, 22, 128])
def test_round_trip_and_refusals(engine_factory, bench_params, mode, mem, L):
    capi, eng = engine(engine_factory, bench_params, L, mode)
    sizes = (1, 3, 64, 65, 257) if L == 5 else (1, 3, 64, 65)
    w = world(eng, L, sizes[-1])
    for ring in ([w.own], w.ring3):
        last = len(ring) - 1
        for n in sizes:
            proofs, binds = w.proofs(n), w.binds[:n]
            flipped = [bytes([b[0] ^ (1 << (i % 8))]) + b[1:] for i, b in enumerate(binds)]
            others = binds[1:] + [w.binds[n % w.n] if n < w.n else shake("bound-gpu-spare", 32)]      # every lane under another lane's binding
            with step(60, "L = %d, %d keys, n = %d" % (L, len(ring), n)):
                good = verify(eng, mem, ring, proofs, b"".join(binds))
                bad = [verify(eng, mem, ring, proofs, b"".join(flipped)), verify(eng, mem, ring, proofs, b"".join(others)), verify(eng, mem, ring, proofs)]
                zero = verify(eng, mem, ring, w.proofs(n, bound=False), bytes(32 * n))
                plain = verify(eng, mem, ring, w.proofs(n, bound=False))
            assert good == (bytes(n), bytes([last]) * n, w.kprime[:32 * n]), (len(ring), n)
            for got in bad + [zero]:
                assert got == (b"\x07" * n, b"\xff" * n, bytes(32 * n)), (len(ring), n)
            assert plain == good
    assert eng.secret_residue() == 0


# ---- 4. bind = NULL ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,mem", MODES)
def test_bind_null_is_the_call_it_extends(engine_factory, bench_params, mode, mem):
    L, n = 10, 65
    capi, eng = engine(engine_factory, bench_params, L, mode)
    w = world(eng, L, n)
    with step(60, "prove"):
        assert prove(eng, mem, w.tok, w.s, w.rng, None) == prove(eng, mem, w.tok, w.s, w.rng) == (bytes(n), w.plain, w.prer)
    mixed = bytearray(w.plain)
    mixed[w.pb * 3 + 33] ^= 1                                    # a tampered charge
    mixed[w.pb * 64 + 64:w.pb * 64 + 96] = b"\xff" * 32        # an undecodable A'
    mixed[w.pb * 7:w.pb * 8] = w.bound[w.pb * 7:w.pb * 8]        # a bound proof: invalid for both
    for ring in ([w.own], w.ring3):
        with step(60, "verify"):
            a, b = verify(eng, mem, ring, bytes(mixed), None), verify(eng, mem, ring, bytes(mixed))
        assert a == b and [i for i in range(n) if a[0][i]] == [3, 7, 64] and (a[0][3], a[0][7], a[0][64]) == (7, 7, 255)
        with step(30, "the transcripts of an unbound call stay what they were"):
            verify(eng, mem, ring, bytes(mixed[:w.pb * 2]), None); t_new = eng.last_spend_transcripts(2)
            verify(eng, mem, ring, bytes(mixed[:w.pb * 2])); t_old = eng.last_spend_transcripts(2)
        assert t_new == t_old and len(t_new[0]) == bc.tr_bytes(L)


# ---- 8. a chunk boundary ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,mem", MODES)
def test_wrong_bindings_on_both_sides_of_a_chunk_boundary(engine_factory, bench_params, mode, mem):
    """a context of 64 records per launch: 150 proofs are three chunks on the two workspaces; the last lane of the first chunk and the
    first lane of the second carry wrong bindings, and every other lane its own"""
    L, n, B = 5, 150, 64
    capi, eng = engine(engine_factory, bench_params, L, mode, max_batch=B)
    w = world(eng, L, n)
    binds = list(w.binds)
    binds[B - 1], binds[B] = w.binds[B], w.binds[B - 1]
    for ring in ([w.own], w.ring3):
        with step(60, "verify"):
            st, ok, kp = verify(eng, mem, ring, w.proofs(n), b"".join(binds))
        want = [7 if i in (B - 1, B) else 0 for i in range(n)]
        assert list(st) == want and list(ok) == [255 if s else len(ring) - 1 for s in want]
        assert kp == b"".join(bytes(32) if want[i] else w.kprime[32 * i:32 * i + 32] for i in range(n))
    with step(60, "prove across the same boundary"):
        assert prove(eng, mem, w.tok, w.s, w.rng, b"".join(w.binds)) == (bytes(n), w.bound, w.prer)
