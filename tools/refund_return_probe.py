"""Partial refunds: what the returned amounts cost an honest batch, against act_redeem_admit_batch, in one process, alternating
(tools/README.md).

One MI355X, L = 128, 2^18 distinct proofs resident in HBM, records, device transcripts, the context's default max_batch, ring of one
key, sequential rng, charge == NULL, empty sets.  Per repetition, one after the other:
    (base)    act_redeem_admit_batch of the BASELINE library -- --baseline-tree names a checkout of the commit to compare against, with
              its library built; its binding is loaded beside this one under another module name and gets a context of its own.
              Without the option the baseline is this tree's own act_redeem_admit_batch (and the result says so).
    (zero)    act_redeem_return_batch with returned = n zero scalars
    (null)    act_redeem_return_batch with returned = NULL
    (all)     act_redeem_return_batch with t = s on every lane
Reported: the raw times, the medians, the ratios median(x) / median(base), the baseline's own run-to-run spread (max - min over
median) and whether each ratio lies inside 1 + spread + 1 %.  Nothing is asserted: a ratio outside the band is reported as measured.
Writes profiles/refund_return_probe.json (or --out).

    python tools/refund_return_probe.py [--baseline-tree DIR] [--out f] [--log2 18] [--reps 5]
"""
import argparse
import ctypes as C
import hashlib
import importlib
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import act_amd  # noqa: E402,F401
from act_amd import capi  # noqa: E402
import bench  # noqa: E402


def load_tree(path, name):
    """the binding of another checkout under the module name `name` (its capi finds the library beside itself)"""
    d = os.path.join(os.path.abspath(path), "anonymous-credit-tokens_amd")
    spec = importlib.util.spec_from_file_location(name, os.path.join(d, "__init__.py"), submodule_search_locations=[d])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return importlib.import_module(name + ".capi")


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refund_return_probe.json"))
    ap.add_argument("--baseline-tree", default=None)
    ap.add_argument("--log2", type=int, default=18)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    N, L, REPS = 1 << a.log2, 128, a.reps
    sh = lambda tag, n: hashlib.shake_256(tag.encode()).digest(n)
    h = capi.params_new("bench-org", "bench-service", "bench-env", "2024-01-01", device=0)
    eng = capi.Engine(h, L, device=0, transcript=capi.TRANSCRIPT_DEVICE)
    sk = eng.private_key_random(sh("rrp-sk", 64))
    bcapi = load_tree(a.baseline_tree, "act_baseline") if a.baseline_tree else capi
    beng = bcapi.Engine(h, L, device=0, transcript=bcapi.TRANSCRIPT_DEVICE) if a.baseline_tree else eng
    t0 = time.perf_counter()
    proofs = bench.make_distinct_proofs_on_device(eng, capi, torch, np, sk, N, L, seed=67)[0]
    print("made %d proofs in %.1f s" % (N, time.perf_counter() - t0), flush=True)
    spent = proofs[:, 32:64].contiguous()                          # s of every lane: returning all of it is the largest t the screen lets through
    zeros = torch.zeros(N * 32, dtype=torch.uint8, device="cuda")
    rng = torch.randint(0, 256, (N * 128,), dtype=torch.uint8, device="cuda")
    out = torch.empty(N * 160, dtype=torch.uint8, device="cuda")
    st = torch.empty(N, dtype=torch.uint8, device="cuda"); ok = torch.empty(N, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    key = np.frombuffer(sk, np.uint8); ep = np.array([1], np.uint32)
    cnt = (C.c_uint64 * len(capi.REDEEM_RETURN_COUNTS))()
    returned = {"zero": zeros.data_ptr(), "null": None, "all": spent.data_ptr()}

    def run(what):
        if what == "base":
            s = bcapi.NullifierSet(2 * N)
            fn, e = beng.lib.act_redeem_admit_batch, beng
            args = [e.ctx, s.h, N, bcapi.MEM_DEVICE, key.ctypes.data, 1, ep.ctypes.data, bcapi.SIGN_MATCHED, proofs.data_ptr(), None,
                    rng.data_ptr(), bcapi.RNG_SEQUENTIAL, out.data_ptr(), st.data_ptr(), ok.data_ptr(), cnt]
        else:
            s = capi.NullifierSet(2 * N)
            fn, e = eng.lib.act_redeem_return_batch, eng
            args = [e.ctx, s.h, N, capi.MEM_DEVICE, key.ctypes.data, 1, ep.ctypes.data, capi.SIGN_MATCHED, proofs.data_ptr(), None, returned[what],
                    rng.data_ptr(), capi.RNG_SEQUENTIAL, out.data_ptr(), st.data_ptr(), ok.data_ptr(), cnt]
        t = time.perf_counter()
        rc = fn(*args)
        dt = time.perf_counter() - t
        if rc:
            raise RuntimeError("%s: rc %d %s" % (what, rc, e.lib.act_last_error(e.ctx).decode()))
        assert int(cnt[7]) == N and len(s) == N, (what, list(cnt))          # every lane accepted
        s.close()
        return dt

    kinds = ("base", "zero", "null", "all")
    for what in kinds:                                              # warm-up: side buffers, staging, code objects
        run(what)
    t = {k: [] for k in kinds}
    for _ in range(REPS):
        for what in kinds:                                          # alternating: drift of the box hits all alike
            t[what].append(run(what))
    med = {k: statistics.median(v) for k, v in t.items()}
    spread = (max(t["base"]) - min(t["base"])) / med["base"]
    band = 1.0 + spread + 0.01
    res = {"tool": "tools/refund_return_probe.py", "device": torch.cuda.get_device_name(0), "L": L, "lanes": N, "reps": REPS, "transcripts": "device",
           "baseline": "act_redeem_admit_batch of " + ("the library under --baseline-tree" if a.baseline_tree else "THIS library (no --baseline-tree given)"),
           "seconds": t, "median_s": med, "lanes_per_s": {k: N / v for k, v in med.items()}, "baseline_spread": spread, "band": band,
           "ratio_to_base": {k: med[k] / med["base"] for k in kinds if k != "base"},
           "inside_band": {k: med[k] / med["base"] <= band for k in kinds if k != "base"}}
    print(json.dumps({k: res[k] for k in ("median_s", "baseline_spread", "band", "ratio_to_base", "inside_band")}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    eng.close()
    if beng is not eng:
        beng.close()


if __name__ == "__main__":
    main()
