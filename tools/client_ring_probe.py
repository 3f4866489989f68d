"""The client's side of key rotation: what to_credit_token against a ring of issuer public keys costs beside the one-key call and
beside what a client does without it -- one full one-key pass per published key over the items the previous pass rejected.

One MI355X, 2^log2 distinct items made on the device and resident in HBM, device transcripts, L = 128.  Per kind (refund, issuance)
and ring size nk in {2, 4}, two mixes of signing keys:
    last     every item signed under the LAST ring key (the worst case for the pass-per-key client: nk full passes)
    spread   item i signed under ring key i % nk
and three ways to turn the batch into tokens, alternating, `--reps` times each:
    a   act_*_to_credit_token_batch under ONE key (its time does not depend on which items it accepts: the untouched baseline)
    b   act_*_to_credit_token_keyring_batch against the ring
    c   nk one-key passes: pass j runs under ring key j over the items every earlier pass rejected, gathered into a dense batch
        on the device (torch index_select), statuses read back in between -- what a client does today
Reported per cell: every repetition's seconds, the median items/s of a, b, c, the ratios of those rates b/a and b/c (rate_b_over_a, rate_b_over_c), and every way's
run-to-run spread (max - min over median).  No pass mark: the figures go into DESIGN.md 4.6.

    python tools/client_ring_probe.py [--out profiles/client_ring_probe.json] [--reps 3] [--log2 18]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 128
CHUNK = 65536


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "client_ring_probe.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--log2", type=int, default=18)
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    import numpy as np
    import torch
    import act_amd  # noqa: F401
    from act_amd import capi
    N = 1 << args.log2
    sh = lambda tag, n: hashlib.shake_256(tag.encode()).digest(n)
    h = capi.params_new("bench-org", "bench-service", "bench-env", "2024-01-01", device=0)
    eng = capi.Engine(h, L, device=0, transcript=capi.TRANSCRIPT_DEVICE)
    lib, ctx = eng.lib, eng.ctx
    PB = eng.proof_bytes
    keys = [eng.private_key_random(sh("crp-sk-%d" % i, 64)) for i in range(4)]
    g = torch.Generator(device="cuda"); g.manual_seed(20240611)
    rnd = lambda *shape: torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)
    buf = lambda m, w: torch.empty((m, w), dtype=torch.uint8, device="cuda")
    ck = lambda rc: eng._ck(rc)

    def make(signers, refund):
        """N items, item i signed under signers[i % len(signers)]: (pre, mid, resp) as [N, w] tensors in HBM (mid = IssuanceRequest
        or SpendProof).  Made by the engine itself with device pointers, a dense chunk per signer at a time, then interleaved."""
        nk_, per = len(signers), N // len(signers)
        outs = (buf(N, 96 if refund else 64), buf(N, PB if refund else 128), buf(N, 128 if refund else 160))
        views = [o.view(per, nk_, o.shape[1]) for o in outs]                   # item i = (i // nk_, i % nk_)
        for j, sk in enumerate(signers):
            for off in range(0, per, CHUNK):
                m = min(CHUNK, per - off)
                pre, req, resp, st = buf(m, 64), buf(m, 128), buf(m, 160), torch.empty(m, dtype=torch.uint8, device="cuda")
                amount = torch.zeros((m, 32), dtype=torch.uint8, device="cuda"); amount[:, 0] = 200
                r0, r1, r2 = rnd(m, 128), rnd(m, 128), rnd(m, 128)
                torch.cuda.synchronize()          # the engine works on its own streams
                eng.pre_issuance_random_dev(m, r0.data_ptr(), pre.data_ptr())
                eng.request_dev(m, pre.data_ptr(), r1.data_ptr(), req.data_ptr())
                eng.issue_dev(sk, m, req.data_ptr(), amount.data_ptr(), r2.data_ptr(), capi.RNG_PER_LANE, resp.data_ptr(), st.data_ptr())
                assert int(st.sum()) == 0
                item = (pre, req, resp)
                if refund:
                    tok, charge = buf(m, 160), torch.zeros((m, 32), dtype=torch.uint8, device="cuda")
                    charge[:, 0] = 7
                    proof, prer, rf = buf(m, PB), buf(m, 96), buf(m, 128)
                    r3, r4 = rnd(m, eng.prove_rng_bytes), rnd(m, 128)
                    torch.cuda.synchronize()
                    eng.issuance_to_credit_token_dev(m, pre.data_ptr(), sk[32:], req.data_ptr(), resp.data_ptr(), tok.data_ptr(), st.data_ptr())
                    assert int(st.sum()) == 0
                    eng.prove_spend_dev(m, tok.data_ptr(), charge.data_ptr(), r3.data_ptr(), proof.data_ptr(), prer.data_ptr(), st.data_ptr())
                    assert int(st.sum()) == 0
                    eng.refund_dev(sk, m, proof.data_ptr(), r4.data_ptr(), capi.RNG_PER_LANE, rf.data_ptr(), st.data_ptr())
                    assert int(st.sum()) == 0
                    del r3
                    item = (prer, proof, rf)
                for v, t in zip(views, item):
                    v[off:off + m, j, :] = t                                      # a strided copy of at most CHUNK rows
        torch.cuda.synchronize()                  # the copies run on torch's stream, the engine reads on its own
        return outs

    def one_key(refund, w, n, pre, mid, resp, tok, st):
        pw, keep = capi._in(w, 32)
        if refund:
            ck(lib.act_refund_to_credit_token_batch(ctx, n, capi.MEM_DEVICE, pre.data_ptr(), mid.data_ptr(), resp.data_ptr(), pw, tok.data_ptr(), st.data_ptr()))
        else:
            ck(lib.act_issuance_to_credit_token_batch(ctx, n, capi.MEM_DEVICE, pre.data_ptr(), pw, mid.data_ptr(), resp.data_ptr(), tok.data_ptr(), st.data_ptr()))

    def ring_call(refund, publics, n, pre, mid, resp, tok, st, ok):
        if refund:
            eng.client_ring_ptr("refund", publics, n, capi.MEM_DEVICE, pre=pre.data_ptr(), proofs=mid.data_ptr(), refund=resp.data_ptr(),
                                out=tok.data_ptr(), status=st.data_ptr(), out_key=ok.data_ptr())
        else:
            eng.client_ring_ptr("issuance", publics, n, capi.MEM_DEVICE, pre=pre.data_ptr(), req=mid.data_ptr(), resp=resp.data_ptr(),
                                out=tok.data_ptr(), status=st.data_ptr(), out_key=ok.data_ptr())

    def passes(refund, publics, pre, mid, resp, tok, st):
        """way c; returns how many items ended up accepted"""
        left = None                                  # indices of the items still without a token (None = all)
        done = 0
        for w in publics:
            if left is None:
                p, m_, r, n = pre, mid, resp, N
            else:
                n = int(left.numel())
                if n == 0:
                    break
                p, m_, r = pre.index_select(0, left), mid.index_select(0, left), resp.index_select(0, left)
            t, s = tok[:n], st[:n]
            torch.cuda.synchronize()
            one_key(refund, w, n, p, m_, r, t, s)
            rej = torch.nonzero(s != 0).flatten()
            done += n - int(rej.numel())
            left = rej if left is None else left.index_select(0, rej)
        torch.cuda.synchronize()
        return done

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    report = {"items": N, "L": L, "reps": args.reps, "device": torch.cuda.get_device_name(0), "transcripts": "device", "cells": []}
    for refund in (True, False):
        sets = {}
        for nk, mix in ((2, "last"), (4, "last"), (2, "spread"), (4, "spread")):
            signers = tuple(range(nk)) if mix == "spread" else (3,)
            if signers not in sets:
                sets.clear()                          # one set in HBM at a time
                torch.cuda.empty_cache()
                sets[signers] = make([keys[i] for i in signers], refund)
            pre, mid, resp = sets[signers]
            ring = list(range(nk)) if mix == "spread" else [0, 1, 2, 3][:nk - 1] + [3]
            publics = [keys[i][32:] for i in ring]
            tok, st, ok = buf(N, 160), torch.empty(N, dtype=torch.uint8, device="cuda"), torch.empty(N, dtype=torch.uint8, device="cuda")
            # warm-up and the answers: every item accepted by b and by c, under the key it was signed with
            ring_call(refund, publics, N, pre, mid, resp, tok, st, ok)
            assert int(st.sum()) == 0, (nk, mix, int((st != 0).sum()), torch.nonzero(st != 0).flatten()[:8].tolist())
            want = (torch.arange(N, device="cuda") % nk).to(torch.uint8) if mix == "spread" else torch.full((N,), nk - 1, dtype=torch.uint8, device="cuda")
            assert bool((ok == want).all())
            assert passes(refund, publics, pre, mid, resp, tok, st) == N
            one_key(refund, publics[-1], N, pre, mid, resp, tok, st)
            secs = {"a": [], "b": [], "c": []}
            for _ in range(args.reps):
                secs["a"].append(timed(lambda: one_key(refund, publics[-1], N, pre, mid, resp, tok, st))[0])
                secs["b"].append(timed(lambda: ring_call(refund, publics, N, pre, mid, resp, tok, st, ok))[0])
                secs["c"].append(timed(lambda: passes(refund, publics, pre, mid, resp, tok, st))[0])
            med = {k: statistics.median(v) for k, v in secs.items()}
            cell = {"kind": "refund" if refund else "issuance", "nkeys": nk, "mix": mix, "seconds": secs,
                    "items_per_s": {k: N / med[k] for k in med}, "rate_b_over_a": med["a"] / med["b"], "rate_b_over_c": med["c"] / med["b"],
                    "spread": {k: (max(v) - min(v)) / med[k] for k, v in secs.items()}}
            report["cells"].append(cell)
            print(json.dumps(cell), flush=True)
            del tok, st, ok
        sets.clear()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
