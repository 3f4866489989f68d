"""Request binding: the model and the helpers that tests/test_bound_model.py, tests/test_bound_host.py (lane bodies on the
CPU) and tests/test_gpu_bound*.py (the calls on the GPU) share.  Not a test module.

  bound(bind)       oracle/pymodel.py resolves transcript_challenge as a module global at call time; inside this context manager a "spend"
                    transcript gets the binding as one more item behind C, so pymodel.prove_spend, spend_verify_challenge and refund
                    ARE the model of the bound form.  Every other label is untouched.
  case(L, tag)      one token made by the model (request, issue, to_credit_token), a charge, rng bytes and a binding, with the bound and
                    the unbound proof the model makes from them
  fixture()         case(5, ...) as the JSON of tests/golden/bound_spend.json
  build_check(out)  tests/hostcheck/bound_check.cpp (+ csrc/host_hash.cpp) as a library"""
import contextlib
import hashlib
import os
import subprocess

import pymodel as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ELL = pm.ELL
FIXTURE_L = 5
LS = (5, 10, 22, 128)      # bytes(L) = 424 + 120 L: 1024 -> 1064 (one chunk -> two), 1664 (a full last block), 3064 -> 3104 (three chunks -> four), the product's size


def shake(label, n):
    return hashlib.shake_256(label.encode()).digest(n)


def scb(v):
    return (v % ELL).to_bytes(32, "little")


def lp(b):
    return pm._lp(b)


def tr_bytes(L, bound=False):
    return 184 + 40 * (6 + 3 * L + (1 if bound else 0))


def tr_stride(L, bound=False):
    return (tr_bytes(L, bound) + 15) & ~15


@contextlib.contextmanager
def bound(bind):
    """pymodel with `bind` (32 bytes) appended to the items of every "spend" transcript"""
    assert len(bind) == 32
    plain = pm.transcript_challenge

    def with_binding(params, label, items):
        return plain(params, label, list(items) + [bytes(bind)] if label == b"spend" else items)
    pm.transcript_challenge = with_binding
    try:
        yield
    finally:
        pm.transcript_challenge = plain


def spend_items(params, sk_x, proof):
    """the items of the "spend" transcript as the verifier under sk_x recomputes them (the unbound ones)"""
    seen = []
    plain = pm.transcript_challenge

    def spy(params_, label, items):
        seen.append(list(items))
        return plain(params_, label, items)
    pm.transcript_challenge = spy
    try:
        pm.spend_verify_challenge(sk_x, params, proof)
    finally:
        pm.transcript_challenge = plain
    return seen[0]


_cases = {}


def case(L, tag="bound", credit=9, spend=2):
    """-> dict: params (pymodel), h, sk (pymodel), sk_rec, tok (pymodel), tok_rec, s, rng, bind, proof / proof_rec / prerefund (bound),
    plain_rec (the unbound proof from the same inputs), gamma (the bound proof's challenge)"""
    key = (L, tag, credit, spend)
    if key in _cases:
        return _cases[key]
    params = pm.Params.new("bound-org", "bound-service", "bound-env", "2025-01-01")
    sk = pm.PrivateKey.random(pm.ByteRng(shake(tag + "-sk", 64)))
    pre = pm.PreIssuance.random(pm.ByteRng(shake(tag + "-pre-%d" % L, 128)))
    req = pm.request(pre, params, pm.ByteRng(shake(tag + "-rq-%d" % L, 128)))
    resp = pm.issue(sk, params, req, credit, pm.ByteRng(shake(tag + "-ir-%d" % L, 128)))
    tok = pm.issuance_to_credit_token(pre, params, sk.w, req, resp)
    rng = shake(tag + "-pr-%d" % L, 64 * (4 * L + 12))
    bind = shake(tag + "-bind-%d" % L, 32)
    with bound(bind):
        proof, prer = pm.prove_spend(tok, params, spend, pm.ByteRng(rng), L)
        g, _ = pm.spend_verify_challenge(sk.x, params, proof)
        assert g == proof.gamma                                     # the model's verifier accepts its prover's bound proof ...
    assert pm.spend_verify_challenge(sk.x, params, proof)[0] != proof.gamma      # ... and the crate's refund does not
    plain, _ = pm.prove_spend(tok, params, spend, pm.ByteRng(rng), L)
    c = dict(L=L, params=params, h=params.encoded(), sk=sk, sk_rec=sk.record(), tok=tok, tok_rec=tok.record(), s=spend, rng=rng, bind=bind, proof=proof,
             proof_rec=proof.record(), prerefund=prer.record(), plain_rec=plain.record(), gamma=proof.gamma)
    _cases[key] = c
    return c


def fixture():
    """what tests/golden/bound_spend.json holds: hex strings and small integers only"""
    c = case(FIXTURE_L, "bound-fixture")
    return {"about": "request binding (DESIGN 4.12): one bound spend proof by the big-integer model (tests/bound_cases.py over oracle/pymodel.py)",
            "L": c["L"], "params": c["h"].hex(), "key": c["sk_rec"].hex(), "token": c["tok_rec"].hex(), "s": c["s"], "rng": c["rng"].hex(),
            "binding": c["bind"].hex(), "proof": c["proof_rec"].hex(), "prerefund": c["prerefund"].hex(), "gamma": pm.sc_bytes(c["gamma"]).hex()}


def build_check(out):
    """tests/hostcheck/bound_check.cpp + csrc/host_hash.cpp (-DACT_B3_COUNT, as keyring_check.cpp wants it) -> a shared object"""
    csrc = os.path.join(ROOT, "anonymous-credit-tokens_amd", "csrc")
    hc = os.path.join(ROOT, "tests", "hostcheck")
    src = os.path.join(hc, "bound_check.cpp")
    deps = [src, os.path.join(hc, "keyring_check.cpp"), os.path.join(hc, "hostcheck.cpp")] + [os.path.join(csrc, f) for f in os.listdir(csrc)
                                                                                          if f.endswith((".h", ".inc", "host_hash.cpp"))]
    if os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in deps):
        return out
    hh = out + ".host_hash.o"
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-Wno-psabi", "-DACT_B3_COUNT", "-c", "-o", hh, os.path.join(csrc, "host_hash.cpp")], check=True)
    subprocess.run(["g++", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-Wno-psabi", "-O2", "-o", out, src, hh], check=True)
    os.remove(hh)
    return out
