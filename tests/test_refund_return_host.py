"""Partial refunds on the CPU: the model of tests/refund_return_cases.py against itself and against oracle/pymodel.py at
t = 0; the lane bodies the feature adds (csrc/return_lanes.h, the screen of csrc/admit_lanes.h), compiled for the host by
tests/hostcheck/return_check.cpp and judged by the model; CBOR type 10 through the host reader and the device reader's lane body.
The same bodies run on the GPU in tests/test_gpu_refund_return.py."""
import ctypes as C
import os
import re
import struct
import subprocess

import pytest

import pymodel as m
import refund_return_cases as rr
from conftest import ROOT, load_golden, shake

L = 8
S = 5          # what the proofs below spend
CREDIT = 9


@pytest.fixture(scope="module")
def world():
    """one key, one token of CREDIT, one proof that spends S at L = 8 -- all by the model"""
    params = m.Params.new("refund-return", "host", "test", "1")
    sk = m.PrivateKey.random(m.ByteRng(shake("rrh-sk", 64)))
    pre = m.PreIssuance.random(m.ByteRng(shake("rrh-pre", 128)))
    req = m.request(pre, params, m.ByteRng(shake("rrh-rq", 128)))
    resp = m.issue(sk, params, req, CREDIT, m.ByteRng(shake("rrh-ir", 128)))
    tok = m.issuance_to_credit_token(pre, params, sk.w, req, resp)
    proof, prer = m.prove_spend(tok, params, S, m.ByteRng(shake("rrh-pr", 64 * (4 * L + 12))), L)
    return params, sk, proof, prer


@pytest.fixture(scope="module")
def return_check():
    return C.CDLL(rr.build_return_check(os.path.join(ROOT, "tests", "hostcheck", "libreturn_check.so")))


# ---- 1. the model against itself ------------------------------------------------------------------------------------------------------------
def test_the_model_against_itself_and_against_pymodel_at_zero(world):
    params, sk, proof, prer = world
    rng = shake("rrh-rr", 128)
    e, alpha = rr.nonces_of(rng)
    for t in (0, 1, S):
        rec = rr.refund_return(sk, params, proof, t, e, alpha)
        assert len(rec) == 160 and rec[128:] == m.sc_bytes(t)
        tok = rr.to_credit_token_return(prer, params, proof, rec, sk.w)
        assert tok.c == (CREDIT - S + t) % m.ELL and (tok.k, tok.r) == (prer.k, prer.r)
        if t == 0:
            old = m.refund(sk, params, proof, m.ByteRng(rng))
            assert rec[:128] == old.record() and rec[128:] == bytes(32)
            assert tok.record() == m.refund_to_credit_token(prer, params, proof, old, sk.w).record()
        else:
            # the existing client must refuse the first 128 bytes: they are a signature over another X_A
            f = [rec[32 * i:32 * i + 32] for i in range(4)]
            as_refund = m.Refund(m.ristretto_decode(f[0]), *(int.from_bytes(x, "little") for x in f[1:]))
            with pytest.raises(m.ActError) as err:
                m.refund_to_credit_token(prer, params, proof, as_refund, sk.w)
            assert err.value.code == m.ERR_INVALID_REFUND_PROOF
        # t altered after signing: the proof fails whatever the new t is
        for other in (t + 1, 0 if t else 2):
            with pytest.raises(m.ActError) as err:
                rr.to_credit_token_return(prer, params, proof, rec[:128] + m.sc_bytes(other), sk.w)
            assert err.value.code == m.ERR_INVALID_REFUND_PROOF
    # a validly signed t > s is an amount the client could never prove in range
    with pytest.raises(m.ActError) as err:
        rr.to_credit_token_return(prer, params, proof, rr.refund_return(sk, params, proof, S + 1, e, alpha), sk.w)
    assert err.value.code == m.ERR_AMOUNT_TOO_BIG
    # the balance the client holds is the balance the issuer signed: X_A = g + h1 (c - s + t) + h2 k* + h3 r*
    t = 3
    want = m.pt_add(m.pt_add(m.pt_add(m.G, m.pt_mul(params.h1, CREDIT - S + t)), m.pt_mul(params.h2, prer.k)), m.pt_mul(params.h3, prer.r))
    assert m.pt_eq(rr.x_a_of(params, proof, t), want)


def test_status_counts_and_prototypes_in_the_header():
    hd = open(os.path.join(ROOT, "include", "act_mi355x.h")).read()
    assert re.search(r"#define ACT_STATUS_RETURN_TOO_BIG 249\b", hd) and re.search(r"#define ACT_REDEEM_RETURN_COUNTS 9\b", hd)
    assert re.search(r"#define ACT_CBOR_REFUND_RETURN 10\b", hd)
    taken = [int(v) for v in re.findall(r"#define ACT_STATUS_\w+ (\d+)", hd)]
    assert taken.count(249) == 1 and len(taken) == len(set(taken))
    from act_amd import capi
    assert capi.STATUS_RETURN_TOO_BIG == 249 == rr.STATUS_RETURN_TOO_BIG and capi.REDEEM_RETURN_COUNTS == capi.ADMIT_COUNTS + ("return_too_big",)
    assert capi.CBOR_TYPES["RefundReturn"] == 10 == rr.CBOR_TYPE
    for name in ("act_refund_sign_return_keyring_batch", "act_redeem_return_batch", "act_redeem_cbor_return_batch", "act_refund_to_credit_token_return_batch"):
        assert name in capi.EXPORTS and re.search(r"\bint %s\(" % name, hd)
    # the replay forms take no returned amounts, and the header says why
    for proto in re.findall(r"\bint (act_\w*replay\w*)\(([^;]*)\);", hd):
        assert "returned" not in proto[1], proto[0]
    assert "NOT OFFERED, on purpose" in hd and "h1 (e + x)^-1" in hd


# ---- 2. the lane bodies ---------------------------------------------------------------------------------------------------------------------
def test_compare(return_check):
    for name, t, s in rr.COMPARE_CASES:
        tb, sb = rr.le(t), rr.le(s)
        assert bool(return_check.hc_return_exceeds(tb, sb)) == rr.exceeds(tb, sb) == ((t % m.ELL) > (s % m.ELL)), name
    import random
    r = random.Random(249)
    for _ in range(2000):
        s = r.getrandbits(r.choice((8, 64, 128, 200, 253, 256)))
        t = r.choice((s, s + 1, max(0, s - 1), s ^ (1 << r.randrange(256)), r.getrandbits(256))) % (1 << 256)
        assert bool(return_check.hc_return_exceeds(rr.le(t), rr.le(s))) == ((t % m.ELL) > (s % m.ELL)), (t, s)


def test_decision_order(return_check):
    """wire code, then the charge, then the returned amount, then the look-up -- which is made for no lane that an earlier rule sheds"""
    probed = C.c_int(0)
    for code in (0, 253, 254, 255):
        for cg in (0, 1):
            for ce in (0, 1):
                for rg in (0, 1):
                    for rf in (0, 1):
                        for found in (0, 1):
                            got = return_check.hc_return_decide(code, cg, ce, rg, rf, found, C.byref(probed))
                            want = code if code else 250 if (cg and not ce) else 249 if (rg and not rf) else 3 if found else 0
                            assert got == want and bool(probed.value) == (want in (0, 3)), (code, cg, ce, rg, rf, found)


def test_screen(return_check):
    """the screen's lane body over records with k, s: charge and returned amount in one pass, nothing returned = the admission screen"""
    cases = [(t, s) for _, t, s in rr.COMPARE_CASES]
    n = len(cases) + 3
    ks = bytearray()
    for i, (t, s) in enumerate(cases):
        ks += rr.le(1000 + i) + rr.le(s)
    for i in range(3):
        ks += rr.le(5000 + i) + rr.le(7)
    returned = b"".join(rr.le(t) for t, _ in cases) + rr.le(8) + rr.le(7) + rr.le(8)
    charge = b"".join(rr.le(s) for _, s in cases) + rr.le(7) + rr.le(6) + rr.le(6)      # the last two: wrong charge (and, the last, t > s as well)
    cap = 64
    tab_keys = (C.c_uint32 * (8 * cap))(); tab_state = (C.c_uint32 * cap)()
    pre = C.create_string_buffer(n + 256); kred = C.create_string_buffer(32 * n + 32 * 256)
    return_check.hc_return_screen(n, 64, bytes(ks), charge, returned, None, tab_keys, tab_state, cap, bytes(16), pre, kred)
    want = [249 if (t % m.ELL) > (s % m.ELL) else 0 for t, s in cases] + [249, 250, 250]
    assert list(pre.raw[:n]) == want
    assert kred.raw[:32 * n] == b"".join(rr.le(int.from_bytes(ks[64 * i:64 * i + 32], "little") % m.ELL) for i in range(n))
    # without charges the last lanes are judged by the returned amount alone; without returned amounts nothing is 249
    return_check.hc_return_screen(n, 64, bytes(ks), None, returned, None, tab_keys, tab_state, cap, bytes(16), pre, kred)
    assert list(pre.raw[:n]) == want[:-3] + [249, 0, 249]
    return_check.hc_return_screen(n, 64, bytes(ks), charge, None, None, tab_keys, tab_state, cap, bytes(16), pre, kred)
    assert list(pre.raw[:n]) == [0] * len(cases) + [0, 250, 250]


def test_sign_and_client_bodies_against_the_model(return_check, world):
    params, sk, proof, prer = world
    h, skb, pb, preb = params.encoded(), sk.record(), proof.record(), prer.record()
    kprime = m.ristretto_encode(rr.k_prime_of(proof))
    e, alpha = rr.nonces_of(shake("rrh-body", 128))
    recs = {}
    for t in (0, 1, S - 1, S, S + 1, m.ELL + 2):      # the last: an unreduced t + l given for t = 2
        rec, counts = rr.host_sign(return_check, h, skb, kprime, rr.le(t), e, alpha)
        assert rec == rr.refund_return(sk, params, proof, t, e, alpha, verify=(t == 0)), t
        recs[t] = rec
        # what the feature adds per signed lane: one fixed-base product on h1 and one point addition.  Restated for the product's
        # 16-bit table of h1 (16 windows; this build: counts[3] windows of 6 bits, 7 multiplications per mixed addition)
        added = counts[0] + counts[1] - counts[2] * (counts[3] - 16) * 7
        print("t = %d: return_xa costs %d fe_mul + %d fe_sq here, %d field operations at the product's table width" % (t, counts[0], counts[1], added))
        assert counts[2] == 1 and added == 16 * 7 + 9, (counts, added)      # 16 mixed additions of 7 multiplications and one full addition of 9
        assert added < 0.001 * 485560
    assert recs[0][:128] == m.refund(sk, params, proof, m.ByteRng(shake("rrh-body", 128))).record()
    lanes = [recs[0], recs[1], recs[S], recs[S + 1], recs[1][:128] + rr.le(2), recs[S][:128] + rr.le(0), bytes(32) + recs[1][32:], b"\x01" + bytes(31) + recs[1][32:]]
    n = len(lanes)
    st, tok = rr.host_client(return_check, h, L, m.ristretto_encode(sk.w), preb * n, pb * n, b"".join(lanes))
    assert list(st) == [0, 0, 0, 8, 4, 4, 4, 255]
    for i, rec in enumerate(lanes):
        if st[i] == 0:
            assert tok[160 * i:160 * i + 160] == rr.to_credit_token_return(prer, params, proof, rec, sk.w).record()
            assert tok[160 * i + 128:160 * i + 160] == rr.le(CREDIT - S + int.from_bytes(rec[128:], "little"))
        else:
            assert tok[160 * i:160 * i + 160] == bytes(160)
    # an unreduced t on the wire: the client reduces it like every scalar
    st, tok = rr.host_client(return_check, h, L, m.ristretto_encode(sk.w), preb, pb, recs[1][:128] + rr.le(m.ELL + 1))
    assert list(st) == [0] and tok[128:160] == rr.le(CREDIT - S + 1)


def test_lane_bodies_under_asan_ubsan_as_a_program_of_their_own(tmp_path):
    """a stand-alone program with its own main, built with the sanitizers and run directly"""
    exe = rr.build_return_check(str(tmp_path / "return_check_asan"), sanitize=True, main=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0 and "RETURN SANITIZERS CLEAN" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


# ---- 3. CBOR type 10 --------------------------------------------------------------------------------------------------------------------------
SIZES_L128 = {"IssuanceRequest": 141, "IssuanceResponse": 176, "SpendProof": 18036, "Refund": 141, "PrivateKey": 71, "PublicKey": 34, "PreIssuance": 71,
              "CreditToken": 176, "PreRefund": 106}      # act_cbor_size of types 1-9 at L = 128, as before this type existed


def test_sizes_of_the_nine_types_in_the_model():
    g = load_golden("lifecycle_L128.json")
    c = g["cases"][0]
    recs = {"IssuanceRequest": c["request"], "IssuanceResponse": c["response"], "SpendProof": c["proof"], "Refund": c["refund"], "PrivateKey": g["sk"],
            "PublicKey": g["sk"][64:], "PreIssuance": c["pre"], "CreditToken": c["token"], "PreRefund": c["prerefund"]}
    assert {t: len(m.cbor_encode(t, bytes.fromhex(hx))) for t, hx in recs.items()} == SIZES_L128


def test_type_10_round_trip_and_respellings_through_both_readers(world, tmp_path):
    """tests/hostcheck/cbor_read_check.cpp: the host reader (cbor_read_message + settle + fix) and the device reader's lane body on a
    corpus of type-10 messages, both against the model"""
    from test_cbor_read_host import build_check
    params, sk, proof, prer = world
    e, alpha = rr.nonces_of(shake("rrh-cbor", 128))
    rec = rr.refund_return(sk, params, proof, 3, e, alpha, verify=False)
    enc = rr.cbor_encode(rec)
    assert len(enc) == 176 == len(m.cbor_encode("Refund", rec[:128])) + 35 and enc[0] == 0xA5 and enc[141:144] == b"\x05\x58\x20" and enc[144:] == rec[128:]
    assert enc[1:141] == m.cbor_encode("Refund", rec[:128])[1:]      # keys spelled and ordered as Refund's, then key 5
    assert rr.cbor_decode(enc) == (0, rec)
    cases = rr.respellings(rec)
    corpus = tmp_path / "corpus.bin"; out = tmp_path / "out.bin"
    with open(corpus, "wb") as f:
        for _, msg, _ in cases:
            f.write(struct.pack("<III", rr.CBOR_TYPE, L, len(msg)) + msg)
    exe = build_check(str(tmp_path / "cbor_read_check"))
    r = subprocess.run([exe, str(corpus), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "%d messages, 0 mismatches" % len(cases) in r.stdout, (r.stdout, r.stderr[-2000:])
    blob = open(out, "rb").read()
    assert len(blob) == len(cases) * 164
    for i, (name, _, (code, want)) in enumerate(cases):
        row = blob[164 * i:164 * i + 164]
        assert (row[0], row[1], row[2]) == (code, code, 0) and row[4:] == want, name
