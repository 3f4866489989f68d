"""Partial refunds with key rotation and with the copy stage: what the two compositions cost beside the calls they are made of, in one
process, alternating (tools/README.md).  The methods of tools/client_ring_probe.py and tools/refund_return_probe.py.

One MI355X, L = 128, 2^log2 distinct items made on the device and resident in HBM, device transcripts, `--reps` interleaved repetitions.
--baseline-tree names a checkout of the commit to compare against, with its library built; its binding is loaded beside this one under
another module name and gets a context of its own.  Without the option the baseline is this tree's own library (and the result says so).

"ring": the client.  Every item is signed under the LAST ring key; rings of 1, 2 and 4 keys.
    base    act_refund_to_credit_token_keyring_batch of the BASELINE library on plain Refunds (t = 0)
    zero    act_refund_to_credit_token_return_keyring_batch on those Refunds with 32 zero bytes appended
    all     the same call on RefundReturn records that return t = s
    passes  (rings of 2 and 4) nk one-key passes of act_refund_to_credit_token_return_batch, pass j under ring key j over the items every
            earlier pass rejected, gathered into a dense batch on the device -- what a client does without the ring call
  The new call adds one fixed-base product on h1 per item to the baseline (121 of 47 289 counted field operations): its time should lie
  inside the baseline's own run-to-run spread plus one per cent.  Reported per ring size, not asserted.
"unique": the server.  act_redeem_return_unique_batch against the BASELINE library's act_redeem_return_batch on batches in which a share
  of 0, 1/2 and 7/8 of the lanes repeat the bytes of an earlier lane (their returned amounts differ), t = s elsewhere, ring of one key,
  sequential rng, empty sets; from HBM, and (a quarter of the lanes) from host memory.  The band is stated for share 0 from HBM only.
Writes profiles/client_ring_return_probe.json (or --out).

    python tools/client_ring_return_probe.py [--baseline-tree DIR] [--out f] [--log2 18] [--reps 5]
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import act_amd  # noqa: E402,F401
from act_amd import capi  # noqa: E402
from refund_return_probe import load_tree  # noqa: E402

L = 128
CHUNK = 65536


def stats(t, base):
    med = {k: statistics.median(v) for k, v in t.items()}
    spread = (max(t[base]) - min(t[base])) / med[base]
    band = 1.0 + spread + 0.01
    return {"seconds": t, "median_s": med, "baseline_spread": spread, "band": band,
            "spread": {k: (max(v) - min(v)) / med[k] for k, v in t.items()},
            "ratio_to_base": {k: med[k] / med[base] for k in t if k != base},
            "inside_band": {k: med[k] / med[base] <= band for k in t if k != base}}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "client_ring_return_probe.json"))
    ap.add_argument("--baseline-tree", default=None)
    ap.add_argument("--log2", type=int, default=18)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    N, REPS = 1 << a.log2, a.reps
    sh = lambda tag, n: hashlib.shake_256(tag.encode()).digest(n)
    h = capi.params_new("bench-org", "bench-service", "bench-env", "2024-01-01", device=0)
    eng = capi.Engine(h, L, device=0, transcript=capi.TRANSCRIPT_DEVICE)
    bcapi = load_tree(a.baseline_tree, "act_baseline") if a.baseline_tree else capi
    beng = bcapi.Engine(h, L, device=0, transcript=bcapi.TRANSCRIPT_DEVICE) if a.baseline_tree else eng
    lib, ctx, PB = eng.lib, eng.ctx, eng.proof_bytes
    keys = [eng.private_key_random(sh("crrp-sk-%d" % i, 64)) for i in range(4)]
    sk = keys[3]                                                    # every item is signed under the last ring key
    g = torch.Generator(device="cuda"); g.manual_seed(20241020)
    rnd = lambda *shape: torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)
    buf = lambda m, w: torch.empty((m, w), dtype=torch.uint8, device="cuda")
    u8 = lambda m: torch.empty(m, dtype=torch.uint8, device="cuda")
    key_arr = np.frombuffer(sk, np.uint8); ep = np.array([1], np.uint32)

    # ---- the items: PreRefund, SpendProof (s = 7 of 200), Refund (t = 0) and RefundReturn (t = s), all under keys[3] ----------------------
    t0 = time.perf_counter()
    prer, proofs, rf, rr = buf(N, 96), buf(N, PB), buf(N, 128), buf(N, 160)
    for off in range(0, N, CHUNK):
        m = min(CHUNK, N - off)
        pre, req, resp, tok, st, ok = buf(m, 64), buf(m, 128), buf(m, 160), buf(m, 160), u8(m), u8(m)
        amount = torch.zeros((m, 32), dtype=torch.uint8, device="cuda"); amount[:, 0] = 200
        charge = torch.zeros((m, 32), dtype=torch.uint8, device="cuda"); charge[:, 0] = 7
        r0, r1, r2, r3, r4, r5 = rnd(m, 128), rnd(m, 128), rnd(m, 128), rnd(m, eng.prove_rng_bytes), rnd(m, 128), rnd(m, 128)
        torch.cuda.synchronize()                                    # the engine works on its own streams
        eng.pre_issuance_random_dev(m, r0.data_ptr(), pre.data_ptr())
        eng.request_dev(m, pre.data_ptr(), r1.data_ptr(), req.data_ptr())
        eng.issue_dev(sk, m, req.data_ptr(), amount.data_ptr(), r2.data_ptr(), capi.RNG_PER_LANE, resp.data_ptr(), st.data_ptr())
        assert int(st.sum()) == 0
        eng.issuance_to_credit_token_dev(m, pre.data_ptr(), sk[32:], req.data_ptr(), resp.data_ptr(), tok.data_ptr(), st.data_ptr())
        assert int(st.sum()) == 0
        eng.prove_spend_dev(m, tok.data_ptr(), charge.data_ptr(), r3.data_ptr(), proofs[off:off + m].data_ptr(), prer[off:off + m].data_ptr(), st.data_ptr())
        assert int(st.sum()) == 0
        eng.refund_dev(sk, m, proofs[off:off + m].data_ptr(), r4.data_ptr(), capi.RNG_PER_LANE, rf[off:off + m].data_ptr(), st.data_ptr())
        assert int(st.sum()) == 0
        ns = capi.NullifierSet(2 * m)
        c = eng.return_ptr("redeem", [sk], m, capi.MEM_DEVICE, set=ns, proofs=proofs[off:off + m].data_ptr(), returned=charge.data_ptr(), rng=r5.data_ptr(),
                           rng_mode=capi.RNG_PER_LANE, out=rr[off:off + m].data_ptr(), status=st.data_ptr(), out_key=ok.data_ptr())
        assert c["accepted"] == m
        ns.close()
        del r3
    rz = torch.cat([rf, torch.zeros((N, 32), dtype=torch.uint8, device="cuda")], dim=1).contiguous()
    torch.cuda.synchronize()
    print("made %d items in %.1f s" % (N, time.perf_counter() - t0), flush=True)

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t, r

    tok, st, ok = buf(N, 160), u8(N), u8(N)

    def base_ring(publics):
        beng.client_ring_ptr("refund", publics, N, bcapi.MEM_DEVICE, pre=prer.data_ptr(), proofs=proofs.data_ptr(), refund=rf.data_ptr(), out=tok.data_ptr(),
                             status=st.data_ptr(), out_key=ok.data_ptr())

    def new_ring(publics, recs):
        eng.client_ring_ptr("refund_return", publics, N, capi.MEM_DEVICE, pre=prer.data_ptr(), proofs=proofs.data_ptr(), refund=recs.data_ptr(), out=tok.data_ptr(),
                            status=st.data_ptr(), out_key=ok.data_ptr())

    def passes(publics):
        left, done = None, 0
        for w in publics:
            if left is None:
                p, m_, r, n = prer, proofs, rr, N
            else:
                n = int(left.numel())
                if n == 0:
                    break
                p, m_, r = prer.index_select(0, left), proofs.index_select(0, left), rr.index_select(0, left)
            t_, s_ = tok[:n], st[:n]
            torch.cuda.synchronize()
            pw, keep = capi._in(w, 32)
            eng._ck(lib.act_refund_to_credit_token_return_batch(ctx, n, capi.MEM_DEVICE, p.data_ptr(), m_.data_ptr(), r.data_ptr(), pw, t_.data_ptr(), s_.data_ptr()))
            rej = torch.nonzero(s_ != 0).flatten()
            done += n - int(rej.numel())
            left = rej if left is None else left.index_select(0, rej)
        torch.cuda.synchronize()
        return done

    report = {"tool": "tools/client_ring_return_probe.py", "device": torch.cuda.get_device_name(0), "L": L, "items": N, "reps": REPS, "transcripts": "device",
              "baseline": "the library under --baseline-tree" if a.baseline_tree else "THIS library (no --baseline-tree given)", "ring": [], "unique": []}
    for nk in (1, 2, 4):
        publics = [keys[i][32:] for i in [0, 1, 2][:nk - 1] + [3]]
        ways = {"base": lambda: base_ring(publics), "zero": lambda: new_ring(publics, rz), "all": lambda: new_ring(publics, rr)}
        if nk > 1:
            ways["passes"] = lambda: passes(publics)
        for name, fn in ways.items():                               # warm-up and the answers: every item accepted under the last key
            r = fn()
            assert int(st.sum()) == 0 and (name == "passes" and r == N or bool((ok == nk - 1).all())), (nk, name)
        t = {k: [] for k in ways}
        for _ in range(REPS):
            for name, fn in ways.items():                           # alternating: drift of the box hits all alike
                t[name].append(timed(fn)[0])
        cell = dict(nkeys=nk, **stats(t, "base"))
        cell["items_per_s"] = {k: N / v for k, v in cell["median_s"].items()}
        if nk > 1:
            cell["rate_all_over_passes"] = cell["median_s"]["passes"] / cell["median_s"]["all"]
        report["ring"].append(cell)
        print(json.dumps({k: cell[k] for k in cell if k != "seconds"}), flush=True)
    del rz, rf, tok

    # ---- the unique return form ---------------------------------------------------------------------------------------------------------------
    rng = torch.randint(0, 256, (N * 128,), dtype=torch.uint8, device="cuda")
    out = torch.empty(N * 160, dtype=torch.uint8, device="cuda")
    cnt = (C.c_uint64 * len(capi.REDEEM_RETURN_UNIQUE_COUNTS))()

    def redeem(unique, n, mem, src, ret, rngp, outp, stp, okp):
        c_, e = (capi, eng) if unique else (bcapi, beng)
        s = c_.NullifierSet(2 * n)
        fn = e.lib.act_redeem_return_unique_batch if unique else e.lib.act_redeem_return_batch
        t = time.perf_counter()
        rc = fn(e.ctx, s.h, n, mem, key_arr.ctypes.data, 1, ep.ctypes.data, c_.SIGN_MATCHED, src, None, ret, rngp, c_.RNG_SEQUENTIAL, outp, stp, okp, cnt)
        dt = time.perf_counter() - t
        if rc:
            raise RuntimeError("rc %d %s" % (rc, e.lib.act_last_error(e.ctx).decode()))
        got = (int(cnt[7]), len(s))
        s.close()
        return dt, got

    for num, den in ((0, 1), (1, 2), (7, 8)):
        r = random.Random(1009 * num + den)
        idx, firsts = [], []
        for i in range(N):
            if firsts and r.random() * den < num:
                idx.append(firsts[r.randrange(len(firsts))])
            else:
                idx.append(i); firsts.append(i)
        sel = torch.from_numpy(np.array(idx, np.int64)).cuda()
        lanes = proofs.index_select(0, sel) if num else proofs
        ret = lanes[:, 32:64].contiguous()                          # t = s ...
        if num:
            ret[torch.from_numpy(np.array([i for i in range(N) if idx[i] != i], np.int64)).cuda(), 0] = 3      # ... and another amount on every repeat
        torch.cuda.synchronize()
        for where, n in (("hbm", N), ("host", N // 4)):
            if where == "hbm":
                args = (n, capi.MEM_DEVICE, lanes.data_ptr(), ret.data_ptr(), rng.data_ptr(), out.data_ptr(), st.data_ptr(), ok.data_ptr())
            else:
                hl, hr, hg = lanes[:n].cpu().numpy(), ret[:n].cpu().numpy(), rng[:128 * n].cpu().numpy()
                ho, hs, hk = np.empty(160 * n, np.uint8), np.empty(n, np.uint8), np.empty(n, np.uint8)
                args = (n, capi.MEM_HOST, hl.ctypes.data, hr.ctypes.data, hg.ctypes.data, ho.ctypes.data, hs.ctypes.data, hk.ctypes.data)
            want = len(set(idx[:n]))
            for unique in (False, True):                            # warm-up and the answers: every leader accepted, every repeat a double spend
                _, got = redeem(unique, *args)
                assert got == (want, want), (num, den, where, unique, got, want)
            t = {"base": [], "unique": []}
            for _ in range(REPS):
                t["base"].append(redeem(False, *args)[0])
                t["unique"].append(redeem(True, *args)[0])
            cell = dict(copy_share="%d/%d" % (num, den), memory=where, lanes=n, distinct=want, **stats(t, "base"))
            cell["lanes_per_s"] = {k: n / v for k, v in cell["median_s"].items()}
            cell["gated"] = (num == 0 and where == "hbm")
            report["unique"].append(cell)
            print(json.dumps({k: cell[k] for k in cell if k != "seconds"}), flush=True)
        del lanes, ret, sel
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print("wrote", a.out)
    eng.close()
    if beng is not eng:
        beng.close()


if __name__ == "__main__":
    main()
