"""Request binding: what the bound calls cost against the parent commit's unbound calls, in one process, alternating (the
shape of tools/return_replay_probe.py).

One MI355X, L = 128, 2^18 distinct tokens; per token an unbound and a bound proof from the same rng bytes, both resident in HBM; device
transcripts, the context's default max_batch, a ring of one key.  Per repetition, one after the other:
    (base_verify)   act_verify_spend_keyring_batch of the BASELINE library over the unbound proofs -- --baseline-tree names a checkout of
                    the commit to compare against, with its library built; its binding is loaded beside this one under another module name
                    and gets a context of its own.  Without the option the baseline is this tree's own call (and the result says so).
    (verify)        (a) this library's act_verify_spend_keyring_batch over the same proofs: the guard on the stride and workspace change
    (bound_verify)  (b) act_verify_spend_keyring_bound_batch over the bound proofs and their bindings
    (base_redeem)   the baseline's act_redeem_return_replay_batch over the unbound proofs, t = s, on fresh sets of 4 n slots
    (bound_redeem)  (c) act_redeem_return_replay_bound_batch over the bound proofs, the same amounts, on fresh sets
Judged as the other probes judge theirs: the ratio of medians, the baseline's own run-to-run spread (max - min over median), and whether
the ratio lies inside 1 + spread + 1 %.  (a) is the figure with a threshold; (b) and (c) are REPORTED whatever they are.  Every call's
statuses are checked (all accepted); nothing is asserted about rates.  Writes profiles/bound_probe.json (or --out).

    python tools/bound_probe.py [--baseline-tree DIR] [--out f] [--log2 18] [--reps 5]
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import act_amd  # noqa: E402,F401
from act_amd import capi  # noqa: E402
from return_replay_probe import load_tree  # noqa: E402


def make_proofs(eng, torch, sk, n, L, chunk=65536):
    """n distinct tokens made on the device, and per token the unbound and the bound proof from the same rng bytes
    -> (unbound [n, PB], bound [n, PB], binds [n, 32]) uint8 cuda tensors; credits uniform in [0, 2^L), charges in [0, c]"""
    import random
    r = random.Random(20250101)
    PB = eng.proof_bytes
    cs = [r.getrandbits(L) for _ in range(n)]
    ss = [r.randrange(c + 1) for c in cs]
    c_host = np.frombuffer(b"".join(c.to_bytes(32, "little") for c in cs), np.uint8).reshape(n, 32)
    s_host = np.frombuffer(b"".join(s.to_bytes(32, "little") for s in ss), np.uint8).reshape(n, 32)
    g = torch.Generator(device="cuda"); g.manual_seed(20250101)
    rnd = lambda *shape: torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)
    buf = lambda m, w: torch.empty((m, w), dtype=torch.uint8, device="cuda")
    plain, bound, binds = buf(n, PB), buf(n, PB), rnd(n, 32)
    for off in range(0, n, chunk):
        m = min(chunk, n - off)
        d_c = torch.from_numpy(c_host[off:off + m].copy()).cuda(); d_s = torch.from_numpy(s_host[off:off + m].copy()).cuda()
        r_pre, r_rq, r_ir, r_pr = rnd(m, 128), rnd(m, 128), rnd(m, 128), rnd(m, eng.prove_rng_bytes)
        pre, req, resp, tok, prer = buf(m, 64), buf(m, 128), buf(m, 160), buf(m, 160), buf(m, 96)
        st = torch.empty(m, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        eng.pre_issuance_random_dev(m, r_pre.data_ptr(), pre.data_ptr())
        eng.request_dev(m, pre.data_ptr(), r_rq.data_ptr(), req.data_ptr())
        eng.issue_dev(sk, m, req.data_ptr(), d_c.data_ptr(), r_ir.data_ptr(), capi.RNG_PER_LANE, resp.data_ptr(), st.data_ptr())
        assert int(st.sum()) == 0
        eng.issuance_to_credit_token_dev(m, pre.data_ptr(), sk[32:], req.data_ptr(), resp.data_ptr(), tok.data_ptr(), st.data_ptr())
        assert int(st.sum()) == 0
        eng.prove_spend_dev(m, tok.data_ptr(), d_s.data_ptr(), r_pr.data_ptr(), plain[off:off + m].data_ptr(), prer.data_ptr(), st.data_ptr())
        assert int(st.sum()) == 0
        eng._ck(eng.lib.act_prove_spend_bound_batch(eng.ctx, m, capi.MEM_DEVICE, tok.data_ptr(), d_s.data_ptr(), r_pr.data_ptr(), binds[off:off + m].data_ptr(),
                                                    bound[off:off + m].data_ptr(), prer.data_ptr(), st.data_ptr()))
        assert int(st.sum()) == 0
        del r_pr
    return plain, bound, binds


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bound_probe.json"))
    ap.add_argument("--baseline-tree", default=None)
    ap.add_argument("--log2", type=int, default=18)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    N, L, REPS = 1 << a.log2, 128, a.reps
    sh = lambda tag, n: hashlib.shake_256(tag.encode()).digest(n)
    h = capi.params_new("bench-org", "bench-service", "bench-env", "2024-01-01", device=0)
    eng = capi.Engine(h, L, device=0, transcript=capi.TRANSCRIPT_DEVICE)
    sk = eng.private_key_random(sh("bp-sk", 64))
    bcapi = load_tree(a.baseline_tree, "act_baseline") if a.baseline_tree else capi
    beng = bcapi.Engine(h, L, device=0, transcript=bcapi.TRANSCRIPT_DEVICE) if a.baseline_tree else eng
    t0 = time.perf_counter()
    plain, bound, binds = make_proofs(eng, torch, sk, N, L)
    print("made 2 x %d proofs in %.1f s" % (N, time.perf_counter() - t0), flush=True)
    amounts = plain[:, 32:64].contiguous()                       # t = s: the largest amount the bound lets through
    key = np.frombuffer(sk, np.uint8); ep = np.array([1], np.uint32); nonce_key = np.frombuffer(sh("bp-nonce-key", 32), np.uint8)
    out = torch.empty(N * 160, dtype=torch.uint8, device="cuda")
    st, ok, rp, kp = (torch.empty(N * w, dtype=torch.uint8, device="cuda") for w in (1, 1, 1, 32))
    cnt = (C.c_uint64 * len(capi.RETURN_REPLAY_COUNTS))()
    torch.cuda.synchronize()

    def accepted(what):
        assert int(st.sum()) == 0 and int(ok.sum()) == 0, what + ": a lane was not accepted"

    def verify(what):
        e = beng if what == "base_verify" else eng
        t = time.perf_counter()
        if what == "bound_verify":
            rc = e.lib.act_verify_spend_keyring_bound_batch(e.ctx, N, capi.MEM_DEVICE, key.ctypes.data, 1, bound.data_ptr(), binds.data_ptr(), st.data_ptr(), ok.data_ptr(), kp.data_ptr())
        else:
            rc = e.lib.act_verify_spend_keyring_batch(e.ctx, N, capi.MEM_DEVICE, key.ctypes.data, 1, plain.data_ptr(), st.data_ptr(), ok.data_ptr(), kp.data_ptr())
        dt = time.perf_counter() - t
        if rc:
            raise RuntimeError("%s: rc %d %s" % (what, rc, e.lib.act_last_error(e.ctx).decode()))
        accepted(what)
        return dt

    def redeem(what):
        base = what == "base_redeem"
        cp, e = (bcapi, beng) if base else (capi, eng)
        s, r = cp.NullifierSet(4 * N), cp.NullifierSet(4 * N)
        head = [e.ctx, s.h, r.h, N, capi.MEM_DEVICE, key.ctypes.data, 1, ep.ctypes.data, cp.SIGN_MATCHED]
        tail = [None, amounts.data_ptr(), nonce_key.ctypes.data, out.data_ptr(), st.data_ptr(), ok.data_ptr(), rp.data_ptr(), cnt]
        t = time.perf_counter()
        if base:
            rc = e.lib.act_redeem_return_replay_batch(*(head + [plain.data_ptr()] + tail))
        else:
            rc = e.lib.act_redeem_return_replay_bound_batch(*(head + [bound.data_ptr(), binds.data_ptr()] + tail))
        dt = time.perf_counter() - t
        if rc:
            raise RuntimeError("%s: rc %d %s" % (what, rc, e.lib.act_last_error(e.ctx).decode()))
        accepted(what)
        assert (len(s), len(r)) == (N, N), (what, list(cnt))
        s.close(); r.close()
        return dt

    calls = {"base_verify": verify, "verify": verify, "bound_verify": verify, "base_redeem": redeem, "bound_redeem": redeem}
    for what, fn in calls.items():                              # warm-up: side buffers, code objects
        fn(what)
    t = {what: [] for what in calls}
    for _ in range(REPS):
        for what, fn in calls.items():                          # alternating: drift of the box hits all alike
            t[what].append(fn(what))
    med = {k: statistics.median(v) for k, v in t.items()}
    spread = {k: (max(t[k]) - min(t[k])) / med[k] for k in ("base_verify", "base_redeem")}
    pairs = {"verify": "base_verify", "bound_verify": "base_verify", "bound_redeem": "base_redeem"}
    res = {"tool": "tools/bound_probe.py", "device": torch.cuda.get_device_name(0), "L": L, "lanes": N, "reps": REPS, "transcripts": "device", "memory": "device",
           "baseline": "the calls of " + ("the library under --baseline-tree" if a.baseline_tree else "THIS library (no --baseline-tree given)"),
           "seconds": t, "median_s": med, "lanes_per_s": {k: N / v for k, v in med.items()}, "baseline_spread": spread,
           "band": {k: 1.0 + spread[b] + 0.01 for k, b in pairs.items()},
           "ratio_to_base": {k: med[k] / med[b] for k, b in pairs.items()},
           "inside_band": {k: med[k] / med[b] <= 1.0 + spread[b] + 0.01 for k, b in pairs.items()},
           "transcript_bytes": {"unbound": eng.transcript_bytes, "bound": eng.transcript_bytes + 40}}
    print(json.dumps({k: res[k] for k in ("median_s", "baseline_spread", "band", "ratio_to_base", "inside_band")}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    eng.close()
    if beng is not eng:
        beng.close()


if __name__ == "__main__":
    main()
