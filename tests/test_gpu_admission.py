"""Admission before verification on the GPU: act_redeem_admit_batch / act_redeem_cbor_admit_batch through the C ABI against the model of
tests/admission_cases.py (labels by construction, a Python set) and against the existing act_redeem_(cbor_)keyring_epochs_batch where
the contract is "the same bytes".  Proofs come from the engine's prover, which the existing tests pin to the oracle.  Both transcript
modes, host and device memory, records and wire.  Every step runs under a time limit of its own.

Rates are measured by tools/admission_probe.py; the tests here assert behaviour only."""
import contextlib
import itertools
import random
import signal

import numpy as np
import pytest

import admission_cases as ad
from conftest import ELL, shake, scb

pytestmark = pytest.mark.gpu


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


def _mode(capi, name):
    return capi.TRANSCRIPT_HOST if name == "host" else capi.TRANSCRIPT_DEVICE


class World:
    """keys and tokens made by the engine: token t is issued under keys[owner[t]] for CREDIT and has two proofs that spend SPEND
    (the same nullifier, different rng)"""
    CREDIT = 9

    def __init__(self, eng, tag, owners, n_keys=4):
        self.eng, self.pb = eng, eng.proof_bytes
        self.keys = [eng.private_key_random(shake("%s-sk%d" % (tag, i), 64)) for i in range(n_keys)]
        n = len(owners)
        self.owners = list(owners)
        pre = eng.pre_issuance_random(shake(tag + "-pre", 128 * n)); req = eng.request(pre, shake(tag + "-rq", 128 * n))
        tok = np.zeros((n, 160), np.uint8)
        for k in range(n_keys):
            sel = [i for i in range(n) if owners[i] == k]
            if not sel:
                continue
            rq = b"".join(req[128 * i:128 * i + 128] for i in sel); pr = b"".join(pre[64 * i:64 * i + 64] for i in sel)
            st, resp = eng.issue(self.keys[k], rq, scb(self.CREDIT) * len(sel), shake("%s-ir%d" % (tag, k), 128 * len(sel)))
            assert st == bytes(len(sel))
            st, t = eng.issuance_to_credit_token(pr, self.keys[k][32:], rq, resp)
            assert st == bytes(len(sel))
            tok[sel] = np.frombuffer(t, np.uint8).reshape(len(sel), 160)
        self.proofs = []
        for v in range(2):
            st, p, _ = eng.prove_spend_seeded(tok.tobytes(), scb(ad.SPEND) * n, shake("%s-seed%d" % (tag, v), 32))
            assert st == bytes(n)
            self.proofs.append(np.frombuffer(p, np.uint8).reshape(n, self.pb).copy())
        assert (self.proofs[0][:, :64] == self.proofs[1][:, :64]).all() and not (self.proofs[0] == self.proofs[1]).all(axis=1).any()
        self.k = [int.from_bytes(self.proofs[0][i, :32].tobytes(), "little") % ELL for i in range(n)]
        assert len(set(self.k)) == n

    def proof(self, t, variant=0, how=None):
        p = self.proofs[variant][t].copy()
        if how == "tampered":
            p[self.pb - 32] ^= 1                        # the last response scalar: the challenge no longer matches
        elif how == "undecodable":
            p[64:96] = 0xFF                             # A' is not a canonical encoding
        elif how == "identity":
            p[64:96] = 0
        return p

    def key_of(self, t, ring_idx):
        """the ring index token t verifies under, or None"""
        return ring_idx.index(self.owners[t]) if self.owners[t] in ring_idx else None


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


def call_admit(eng, mem, ns, ring, n, blob=None, msgs=None, charges=None, rng=b"", rng_mode=0, sign_key=-1, key_epochs=None, raw=False):
    """one admission call in either memory kind and either form -> (rc, statuses, out bytes, out_key, counts)"""
    from act_amd import capi
    wire = msgs is not None
    ob = eng.cbor_size("Refund") if wire else 128
    if mem == "host":
        if wire:
            rc, st, out, ok, c = eng.redeem_cbor_admit(ns, ring, msgs, rng, rng_mode, sign_key, charges, key_epochs, raw=True)
            out = b"".join(m if m else bytes(ob) for m in out)
        else:
            rc, st, out, ok, c = eng.redeem_admit(ns, ring, blob, rng, rng_mode, sign_key, charges, key_epochs, raw=True)
    else:
        d = Dev()
        src = d.up(b"".join(msgs) if wire else blob)
        offs = np.zeros(n + 1, np.uint64)
        if wire:
            offs[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
        dc = d.up(charges) if charges is not None else None
        dr = None if isinstance(rng, capi.ReplayRng) else d.up(rng)
        out, st, ok = d.new(ob * n, 7), d.new(n, 99), d.new(n, 77)
        d.t.cuda.synchronize()
        p = dict(set=ns, charges=dc.data_ptr() if dc is not None else None, rng=rng.ptr if dr is None else dr.data_ptr(), rng_mode=rng_mode, out=out.data_ptr(),
                 status=st.data_ptr(), out_key=ok.data_ptr(), key_epochs=key_epochs, sign_key=sign_key, raw=True)
        if wire:
            rc, c = eng.admit_ptr("redeem_cbor", ring, n, capi.MEM_DEVICE, cbor=src.data_ptr(), offsets=offs.ctypes.data, **p)
        else:
            rc, c = eng.admit_ptr("redeem", ring, n, capi.MEM_DEVICE, proofs=src.data_ptr(), **p)
        st, out, ok = d.down(st, n), d.down(out, ob * n), d.down(ok, n)
    if not raw:
        assert rc == 0, (rc, eng.lib.act_last_error(eng.ctx))
    return rc, st, out, ok, c


def call_plain(eng, mem, ns, ring, n, blob=None, msgs=None, rng=b"", rng_mode=0, sign_key=-1, key_epochs=None):
    """act_redeem_(cbor_)keyring_epochs_batch, the existing call -> (statuses, out bytes, out_key)"""
    from act_amd import capi
    wire = msgs is not None
    ob = eng.cbor_size("Refund") if wire else 128
    if mem == "host":
        if wire:
            st, out, ok = eng.redeem_cbor_keyring(ns, ring, msgs, rng, rng_mode, sign_key, key_epochs)
            return st, b"".join(m if m else bytes(ob) for m in out), ok
        return eng.redeem_keyring(ns, ring, blob, rng, rng_mode, sign_key, key_epochs=key_epochs)
    d = Dev()
    src = d.up(b"".join(msgs) if wire else blob)
    offs = np.zeros(n + 1, np.uint64)
    if wire:
        offs[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
    dr = None if isinstance(rng, capi.ReplayRng) else d.up(rng)
    out, st, ok = d.new(ob * n, 7), d.new(n, 99), d.new(n, 77)
    d.t.cuda.synchronize()
    p = dict(set=ns, rng=rng.ptr if dr is None else dr.data_ptr(), rng_mode=rng_mode, out=out.data_ptr(), status=st.data_ptr(), out_key=ok.data_ptr(),
             key_epochs=key_epochs, sign_key=sign_key)
    if wire:
        eng.keyring_ptr("redeem_cbor", ring, n, capi.MEM_DEVICE, cbor=src.data_ptr(), offsets=offs.ctypes.data, **p)
    else:
        eng.keyring_ptr("redeem", ring, n, capi.MEM_DEVICE, proofs=src.data_ptr(), **p)
    return d.down(st, n), d.down(out, ob * n), d.down(ok, n)


def _le(v):
    return v.to_bytes(32, "little")


def _pairs(ns):
    keys, eps = ns.export_epochs()
    return sorted((keys[32 * i:32 * i + 32], int(eps[i])) for i in range(len(eps)))


_worlds = {}


def world(eng, tag, owners):
    key = (id(eng), tag)
    if key not in _worlds:
        _worlds[key] = World(eng, tag, owners)
    return _worlds[key]


# ---- 1. the fixed lane mix: exact codes ---------------------------------------------------------------------------------------------------
TOKENS = ("t0", "t1", "t2", "t3", "t4", "t5", "t6", "t7", "sp0", "sp1", "sp2", "sp3", "sp4")
HOW = {7: "tampered", 255: "undecodable", 6: "identity", 0: None}


def fixed_mix(eng, w, L):
    """-> (record lanes, wire messages, charges) of ad.FIXED_MIX"""
    t = {name: i for i, name in enumerate(TOKENS)}
    seen, recs = {}, []
    for name, tok, verdict, right, code, canon in ad.FIXED_MIX:
        v = seen.get(tok, 0) if tok.startswith("t") else 0          # the second lane of a shared fresh nullifier is the token's other proof
        seen[tok] = v + 1
        recs.append(w.proof(t[tok], v, HOW[verdict]).tobytes())
    msgs = eng.cbor_encode("SpendProof", b"".join(recs))
    msgs[12] = ad.respelled(recs[12], L)
    msgs[13] = msgs[13][:-1]
    msgs[14] = b"\x83\x01\x02\x03"
    msgs[15] = ad.invalid_point_then_fault(recs[15], L)
    charges = b"".join(scb(ad.SPEND if right else ad.EXPECTED_WRONG) for _, _, _, right, _, _ in ad.FIXED_MIX)
    return recs, msgs, charges


@pytest.mark.parametrize("mode,mem", [("host", "host"), ("host", "device"), ("device", "host"), ("device", "device")])
def test_fixed_lane_mix_exact_codes(engine_factory, bench_params, mode, mem):
    from act_amd import capi
    ad.check_model_on_fixed_mix()
    L = 8
    eng = engine_factory(bench_params, L, max_batch=16, transcript=_mode(capi, mode))
    with step(120, "tokens and proofs"):
        w = world(eng, "adm-fix", [0] * len(TOKENS))
        recs, msgs, charges = fixed_mix(eng, w, L)
    a = w.keys[0]
    t = {name: i for i, name in enumerate(TOKENS)}
    spent = b"".join(_le(w.k[t[name]]) for name in ad.FIXED_SPENT)
    rng = shake("adm-fix-rng", 128 * 16)
    for wire in (False, True):
        n = 16 if wire else ad.N_RECORD_LANES
        want = ad.FIXED_EXPECT[:n]
        kw = dict(msgs=msgs[:n]) if wire else dict(blob=b"".join(recs[:n]))
        with step(120, "fixed mix, wire=%s" % wire):
            ns, twin = capi.NullifierSet(1000, salt=bytes(16)), capi.NullifierSet(1000, salt=bytes(16))
            assert ns.check_and_insert(spent) == bytes(5) and twin.check_and_insert(spent) == bytes(5)
            rc, st, out, ok, c = call_admit(eng, mem, ns, [a], n, charges=charges[:32 * n], rng=rng, rng_mode=capi.RNG_PER_LANE, **kw)
            print("admission", list(st), c)
            assert list(st) == want
            assert c == (ad.FIXED_COUNTS_WIRE if wire else ad.FIXED_COUNTS_RECORDS)
            assert c["verified"] == c["lanes"] - c["wire_rejected"] - c["wrong_charge"] - c["spent_before"]
            ob = len(out) // n
            for i in range(n):
                assert any(out[ob * i:ob * i + ob]) == (st[i] == 0) and ok[i] == (0 if i in (0, 8, 9, 10) else 255), i
            # the plain redeem call on a twin set: its codes, and the accepted lanes' bytes (per-lane rng: the ORIGINAL lane's slice)
            pst, pout, pok = call_plain(eng, mem, twin, [a], n, rng=rng, rng_mode=capi.RNG_PER_LANE, **kw)
            print("plain    ", list(pst))
            assert list(pst) == ad.FIXED_EXPECT_PLAIN[:n]
            for i in range(n):
                if st[i] == 0:
                    assert pst[i] == 0 and out[ob * i:ob * i + ob] == pout[ob * i:ob * i + ob], i
            # a wrong-charge lane left no trace and is redeemed by a second call that asks the right price
            k2 = _le(w.k[t["t2"]])
            assert ns.contains(k2) == b"\0" and len(ns) == 5 + 3
            kw1 = dict(msgs=[msgs[5]]) if wire else dict(blob=recs[5])
            rc, st1, out1, ok1, c1 = call_admit(eng, mem, ns, [a], 1, charges=scb(ad.SPEND), rng=rng, rng_mode=capi.RNG_PER_LANE, **kw1)
            assert (st1, ok1) == (b"\0", b"\0") and any(out1) and c1["accepted"] == 1 and ns.contains(k2) == b"\1"
            ns.close(); twin.close()
    assert eng.secret_residue() == 0


# ---- 2. charge == NULL: byte for byte the existing call -----------------------------------------------------------------------------------
EQ_N = 150
_r = random.Random(5)
EQ_OWNERS = [_r.randrange(4) for _ in range(EQ_N)]      # the issuer key of every token


def eq_lanes(w):
    plan, tokens = ad.density_plan(EQ_N, 1, 2, 7, False)
    recs = [w.proof(p.token, p.variant, "tampered" if p.tampered else None).tobytes() for p in plan]
    return plan, recs


@pytest.mark.parametrize("mode,mem,wire", [("host", "host", False), ("device", "device", False), ("device", "host", True), ("host", "device", True)])
def test_equal_to_the_existing_call_without_charges(engine_factory, bench_params, mode, mem, wire):
    from act_amd import capi
    L = 8
    eng = engine_factory(bench_params, L, max_batch=16, transcript=_mode(capi, mode))
    with step(180, "tokens and proofs"):
        w = world(eng, "adm-eq", EQ_OWNERS)
        plan, recs = eq_lanes(w)
        msgs = eng.cbor_encode("SpendProof", b"".join(recs)) if wire else None
        if wire:                                                    # some other legal spellings among them, one of them a replay
            for i in (3, 40, 77):
                msgs[i] = ad.respelled(recs[i], L)
            i = next(i for i, p in enumerate(plan) if p.spent)
            msgs[i] = ad.respelled(recs[i], L)
    n = EQ_N
    kw = dict(msgs=msgs) if wire else dict(blob=b"".join(recs))
    spent_tokens = sorted({p.token for p in plan if p.spent})
    # one export, two sets restored from it
    with step(60, "the source set"):
        src = capi.NullifierSet(4000, salt=b"\x07" * 16)
        blob = b"".join(_le(w.k[t]) for t in spent_tokens)
        assert src.check_and_insert(blob, epoch_index=bytes(i % 3 for i in range(len(spent_tokens))), epochs=[11, 12, 13]) == bytes(len(spent_tokens))
        ekeys, eeps = src.export_epochs()
        src.close()

    def restored():
        s = capi.NullifierSet(4000, salt=b"\x07" * 16)
        eps = sorted(set(int(e) for e in eeps))
        assert s.check_and_insert(ekeys, epoch_index=bytes(eps.index(int(e)) for e in eeps), epochs=eps) == bytes(len(eeps))
        return s
    rng = shake("adm-eq-rng", 128 * n)
    rings = ([0], [1, 0], [3, 2, 1, 0])
    for ring_idx, sign_key, rng_mode in itertools.product(rings, (-1, 0), (capi.RNG_PER_LANE, capi.RNG_SEQUENTIAL, capi.RNG_CALLBACK)):
        ring = [w.keys[k] for k in ring_idx]
        epochs = [100 + k for k in ring_idx]
        with step(120, "ring %s sign %d rng %d" % (ring_idx, sign_key, rng_mode)):
            sa, sb = restored(), restored()
            ga, gb = (capi.ReplayRng(rng), capi.ReplayRng(rng)) if rng_mode == capi.RNG_CALLBACK else (rng, rng)
            rc, st, out, ok, c = call_admit(eng, mem, sa, ring, n, rng=ga, rng_mode=rng_mode, sign_key=sign_key, key_epochs=epochs, **kw)
            pst, pout, pok = call_plain(eng, mem, sb, ring, n, rng=gb, rng_mode=rng_mode, sign_key=sign_key, key_epochs=epochs, **kw)
            # the model: a lane verifies iff it is not tampered and its token's key is in the ring
            lanes = [ad.Lane(w.k[p.token], ad.SPEND, 7 if p.tampered or w.key_of(p.token, ring_idx) is None else 0,
                             w.key_of(p.token, ring_idx) if w.key_of(p.token, ring_idx) is not None else 255) for p in plan]
            mst, mok, mc, mrec = ad.model(lanes, {w.k[t] for t in spent_tokens})
            assert list(st) == mst and list(ok) == mok and c == mc, (ring_idx, sign_key, rng_mode)
            assert c["verified"] == n - c["spent_before"] and c["spent_before"] == sum(1 for p in plan if p.spent)
            ob = len(out) // n
            before = {w.k[t] for t in spent_tokens}
            for i in range(n):
                if st[i] != pst[i]:
                    assert lanes[i].k in before and st[i] == 3, (i, st[i], pst[i])
                if st[i] == 0 or pst[i] == 0:
                    assert st[i] == pst[i] == 0 and ok[i] == pok[i] and out[ob * i:ob * i + ob] == pout[ob * i:ob * i + ob], (i, ring_idx, sign_key, rng_mode)
                else:
                    assert not any(out[ob * i:ob * i + ob]), i
                if lanes[i].k not in before:
                    assert (st[i], ok[i]) == (pst[i], pok[i]), i
            assert _pairs(sa) == _pairs(sb) and len(sa) == len(spent_tokens) + c["accepted"] and c["accepted"] > 0 and c["double_spend_after"] > 0
            assert {(int.from_bytes(k, "little"), e) for k, e in _pairs(sa)} >= {(k, epochs[key]) for k, key in mrec}
            if rng_mode == capi.RNG_CALLBACK:
                assert ga.draws == gb.draws == ([128 * c["accepted"]] if c["accepted"] else []) and ga.pos == gb.pos
            sa.close(); sb.close()
    assert eng.secret_residue() == 0


# ---- 3. work is skipped ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem,wire", [("host", False), ("device", False), ("host", True), ("device", True)])
def test_a_batch_that_is_shed_completely_runs_no_verification(engine_factory, bench_params, mem, wire):
    from act_amd import capi
    L = 8
    eng = engine_factory(bench_params, L, max_batch=16, transcript=capi.TRANSCRIPT_DEVICE)
    with step(120, "tokens and proofs"):
        w = world(eng, "adm-eq", EQ_OWNERS)
    n = 40
    recs = [w.proof(t, t % 2, "tampered" if t % 3 == 0 else None).tobytes() for t in range(n)]
    charges = b"".join(scb(ad.SPEND + (1 if t % 2 else 0)) for t in range(n))        # odd lanes: wrong charge; even lanes: replays
    kw = dict(msgs=eng.cbor_encode("SpendProof", b"".join(recs))) if wire else dict(blob=b"".join(recs))
    ns = capi.NullifierSet(1000)
    assert ns.check_and_insert(b"".join(_le(w.k[t]) for t in range(0, n, 2))) == bytes(n // 2)
    g = capi.ReplayRng(shake("adm-shed", 128 * n))
    with step(60, "the shed batch"):
        eng.prof_enable(True); eng.prof_reset()
        rc, st, out, ok, c = call_admit(eng, mem, ns, [w.keys[0], w.keys[1]], n, charges=charges, rng=g, rng_mode=capi.RNG_CALLBACK, **kw)
        prof = eng.prof()
        eng.prof_enable(False)
    assert list(st) == [250 if t % 2 else 3 for t in range(n)] and ok == b"\xff" * n and not any(out)
    assert c == dict(lanes=n, wire_rejected=0, wrong_charge=n // 2, spent_before=n // 2, verified=0, rejected_by_verification=0, double_spend_after=0, accepted=0)
    assert "k_spend_bits" not in prof and not any(k.startswith("k_spend") for k in prof), prof
    assert g.draws == [] and len(ns) == n // 2
    # the same lanes without charges and with an empty set are verified: the hook sees the launches
    ns2 = capi.NullifierSet(1000)
    with step(60, "the same batch, nothing shed"):
        eng.prof_enable(True); eng.prof_reset()
        rc, st, out, ok, c = call_admit(eng, mem, ns2, [w.keys[0], w.keys[1]], n, rng=g, rng_mode=capi.RNG_CALLBACK, **kw)
        prof = eng.prof()
        eng.prof_enable(False)
    assert c["verified"] == n and prof["k_spend_bits"]["launches"] >= 1 and prof["k_spend_bits"]["lanes"] == n * L
    ns.close(); ns2.close()
    assert eng.secret_residue() == 0


# ---- 4. sizes and densities -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,mem,wire", [("host", "host", False), ("device", "device", False), ("host", "device", True), ("device", "host", True)])
def test_sizes_and_densities(engine_factory, bench_params, mode, mem, wire):
    from act_amd import capi
    L, n = 8, ad.DENSITY_N
    eng = engine_factory(bench_params, L, max_batch=4096, transcript=_mode(capi, mode))
    with step(300, "tokens and proofs"):
        w = world(eng, "adm-den", [0] * n)
        tampered = w.proofs[0].copy(); tampered[:, w.pb - 32] ^= 1
        wire_of = None
        if wire:
            ml = eng.cbor_size("SpendProof")
            enc = lambda arr: np.frombuffer(b"".join(eng.cbor_encode("SpendProof", arr.tobytes())), np.uint8).reshape(n, ml)
            wire_of = {(0, False): enc(w.proofs[0]), (1, False): enc(w.proofs[1]), (0, True): enc(tampered)}
    rec_of = {(0, False): w.proofs[0], (1, False): w.proofs[1], (0, True): tampered}
    a = w.keys[0]
    for (num, den), with_charges in itertools.product(ad.DENSITIES + ad.EXTRA_DENSITIES, (False, True)):
        plan, tokens = ad.density_plan(n, num, den, ad.density_seed(num, den), with_charges)
        cats, mst0, mc0 = ad.plan_categories(plan, with_charges)
        if (num, den) in ((1, 8), (1, 2), (7, 8)):                  # asserted on the model's output before anything is compared
            assert all(16 * v >= n for v in cats.values()), (num, den, with_charges, cats)
        lanes, charges, spent = ad.plan_lanes(plan, nullifier=lambda t: w.k[t])
        mst, mok, mc, mrec = ad.model(lanes, spent, charges if with_charges else None)
        assert mst == mst0 and mc == mc0
        src = wire_of if wire else rec_of
        rows = np.stack([src[(p.variant, p.tampered)][p.token] for p in plan])
        kw = dict(msgs=[r.tobytes() for r in rows]) if wire else dict(blob=rows.tobytes())
        cb = b"".join(scb(c) for c in charges) if with_charges else None
        with step(240, "density %d/%d charges=%s" % (num, den, with_charges)):
            ns = capi.NullifierSet(3 * n, salt=b"\x05" * 16)
            if spent:
                assert ns.check_and_insert(b"".join(_le(k) for k in sorted(spent))) == bytes(len(spent))
            g = capi.ReplayRng(shake("adm-den-rng", 128 * n))
            rc, st, out, ok, c = call_admit(eng, mem, ns, [a], n, charges=cb, rng=g, rng_mode=capi.RNG_CALLBACK, **kw)
            print("density %d/%d charges=%s:" % (num, den, with_charges), c)
            assert c == mc and list(st) == mst and list(ok) == mok, (num, den, with_charges)
            assert c["verified"] == n - c["wire_rejected"] - c["wrong_charge"] - c["spent_before"]
            ob = len(out) // n
            signed = np.frombuffer(out, np.uint8).reshape(n, ob).any(axis=1)
            assert (signed == (np.frombuffer(st, np.uint8) == 0)).all()
            assert g.draws == ([128 * mc["accepted"]] if mc["accepted"] else []) and len(ns) == len(spent) + mc["accepted"]
            keys = ns.export()
            assert {int.from_bytes(keys[32 * i:32 * i + 32], "little") for i in range(len(ns))} == spent | {k for k, _ in mrec}
            ns.close()
    assert eng.secret_residue() == 0


# ---- 5. hygiene and the failure contract ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["host", "device"])
def test_hygiene_and_failed_signatures(engine_factory, bench_params, mem):
    from act_amd import capi
    L = 8
    eng = engine_factory(bench_params, L, max_batch=16, transcript=capi.TRANSCRIPT_HOST)
    with step(120, "tokens and proofs"):
        w = world(eng, "adm-eq", EQ_OWNERS)
        plan, recs = eq_lanes(w)
    n = EQ_N
    ring_idx = [1, 0, 3, 2]
    ring = [w.keys[k] for k in ring_idx]
    blob = b"".join(recs)
    spent = {w.k[p.token] for p in plan if p.spent}
    rng = shake("adm-hy-rng", 128 * n)
    lanes = [ad.Lane(w.k[p.token], ad.SPEND, 7 if p.tampered else 0, w.key_of(p.token, ring_idx)) for p in plan]
    mst, mok, mc, mrec = ad.model(lanes, spent)

    def fresh():
        s = capi.NullifierSet(4000)
        assert s.check_and_insert(b"".join(_le(k) for k in sorted(spent))) == bytes(len(spent))
        return s
    with step(120, "accepted, per-lane rng"):
        ns = fresh()
        rc, st, out, ok, c = call_admit(eng, mem, ns, ring, n, blob=blob, rng=rng, rng_mode=capi.RNG_PER_LANE)
        assert list(st) == mst and c == mc and eng.secret_residue() == 0
        ns.close()
    with step(120, "the signature step fails behind the recorded nullifiers"):
        marks = []
        for admit in (True, False):
            ns = fresh()
            assert eng.lib.act_debug_fail_next_signs(eng.ctx, 1) == 0
            if admit:
                rc, st, out, ok, c = call_admit(eng, mem, ns, ring, n, blob=blob, rng=rng, rng_mode=capi.RNG_PER_LANE, raw=True)
            else:
                rc, st, out, ok = eng.redeem_keyring(ns, ring, blob, rng, capi.RNG_PER_LANE, raw=True)
            assert rc != 0 and not any(out) and st.count(251) == len(ns) - len(spent) == mc["accepted"]
            marks.append(st)
            ns.close()
            assert eng.secret_residue() == 0
        assert [i for i, s in enumerate(marks[0]) if s == 251] == [i for i, s in enumerate(marks[1]) if s == 251] == [i for i, s in enumerate(mst) if s == 0]
        assert all(a == b or (lanes[i].k in spent and a == 3) for i, (a, b) in enumerate(zip(marks[0], marks[1])))
    with step(120, "refused calls"):
        ns = fresh()
        for bad in (dict(sign_key=4), dict(key_epochs=[1, 2, 3, 1 << 24])):
            rc, st, out, ok, c = call_admit(eng, mem, ns, ring, n, blob=blob, rng=rng, rng_mode=capi.RNG_PER_LANE, raw=True, **bad)
            assert rc == 1 and len(ns) == len(spent) and c["lanes"] == 0
        assert eng.secret_residue() == 0
        # n == 0 is an empty call
        rc, st, out, ok, c = call_admit(eng, "host", ns, ring, 0, blob=b"", rng=rng, rng_mode=capi.RNG_PER_LANE)
        assert rc == 0 and c["lanes"] == 0
        ns.close()


def test_python_api():
    """api.PrivateKey / api.Keyring: the admission methods beside their redeem twins"""
    import act_amd
    from act_amd import api
    params = api.Params.new("test-org", "test-service", "test", "2024-01-01")
    rng = api.ByteStreamRng(shake("adm-api", 1 << 20))
    with step(240, "api round trip"):
        sk = api.PrivateKey.random(rng, params)
        pre = api.PreIssuance.random(rng, params)
        req = pre.request(params, rng)
        tok = pre.to_credit_token(params, sk.public(), req, sk.issue(params, req, 20, rng))
        proof, prer = tok.prove_spend(params, 5, rng)
        db = api.NullifierDb(1000)
        res = sk.redeem_admit_batch(params, db, [proof], rng, charges=[6])
        assert isinstance(res[0], api.Error) and res[0].code == 250 and res[0].name == "WrongCharge" and len(db) == 0
        res = sk.redeem_admit_batch(params, db, [proof, proof], rng, charges=[5, 5])
        assert isinstance(res[0], api.Refund) and isinstance(res[1], api.Error) and res[1].code == 3 and len(db) == 1
        tok2 = prer.to_credit_token(params, proof, res[0], sk.public())
        ring = api.Keyring([sk], epochs=[9])
        res, matched = ring.redeem_admit_cbor_batch(params, db, [proof.to_cbor(params)], rng, charges=[5])
        assert isinstance(res[0], api.Error) and res[0].code == 3 and matched == [None] and ring.last_admit_counts["verified"] == 0
        proof2, _ = tok2.prove_spend(params, 1, rng)
        res, matched = ring.redeem_admit_cbor_batch(params, db, [proof2.to_cbor(params)], rng, charges=[1])
        assert isinstance(res[0], bytes) and matched == [0] and db.epoch_len(9) == 1
    assert act_amd is not None


def test_two_threads_on_one_context(engine_factory, bench_params):
    """A context may be shared between host threads: two threads in act_redeem_admit_batch on ONE engine, device memory and per-lane
    rng (the survivors' slices are gathered into a buffer of the context's), each on a set of its own -- every call's bytes are those
    of the same call made alone."""
    import threading
    from act_amd import capi
    L = 8
    eng = engine_factory(bench_params, L, max_batch=16, transcript=capi.TRANSCRIPT_DEVICE)
    with step(120, "tokens and proofs"):
        w = world(eng, "adm-eq", EQ_OWNERS)
        plan, recs = eq_lanes(w)
    ring = [w.keys[k] for k in (1, 0, 3, 2)]
    spent = sorted({w.k[p.token] for p in plan if p.spent})
    jobs = []
    for t in range(2):                                  # two different batches: lanes [0, 110) and [40, 150), different rng
        lo, hi = (0, 110) if t == 0 else (40, EQ_N)
        jobs.append((b"".join(recs[lo:hi]), hi - lo, shake("adm-thr-rng%d" % t, 128 * (hi - lo))))

    def one(job):
        blob, n, rng = job
        ns = capi.NullifierSet(4000)
        assert ns.check_and_insert(b"".join(_le(k) for k in spent)) == bytes(len(spent))
        res = call_admit(eng, "device", ns, ring, n, blob=blob, rng=rng, rng_mode=capi.RNG_PER_LANE)
        ns.close()
        return res
    with step(120, "alone"):
        alone = [one(j) for j in jobs]
        assert all(r[4]["accepted"] > 0 and 0 < r[4]["verified"] < r[4]["lanes"] for r in alone)
    with step(240, "together"):
        for rnd in range(6):
            got, errs = [None, None], []

            def run(i):
                try:
                    got[i] = one(jobs[i])
                except BaseException as e:      # noqa: BLE001
                    errs.append(e)
            th = [threading.Thread(target=run, args=(i,)) for i in range(2)]
            for x in th:
                x.start()
            for x in th:
                x.join()
            assert not errs, errs
            assert got == alone, rnd
    assert eng.secret_residue() == 0
