"""Replayable partial refunds: what the returned amounts cost an honest batch and a batch of retries, against the parent commit's
act_redeem_(cbor_)admit_replay_batch, in one process, alternating (tools/README.md; the shape of tools/refund_return_probe.py).

One MI355X, L = 128, 2^18 distinct proofs resident in HBM, records and wire (canonical messages of one size), device transcripts, the
context's default max_batch, ring of one key with an epoch, charge == NULL, fresh sets of 4 n slots per timed pair.  Per repetition and
form, one after the other, each a first call on empty sets and then THE SAME batch again on the same sets (every lane a retry):
    (base)    act_redeem_(cbor_)admit_replay_batch of the BASELINE library -- --baseline-tree names a checkout of the commit to compare
              against, with its library built; its binding is loaded beside this one under another module name and gets a context of its
              own.  Without the option the baseline is this tree's own call (and the result says so).
    (null)    act_redeem_(cbor_)return_replay_batch with returned = NULL
    (zero)    ... with returned = n zero scalars
    (all)     ... with t = s on every lane; its second call is (all_retry), judged against (base_retry)
Reported: the raw times, the medians, the ratios median(x) / median(base) (all_retry: / median(base_retry)), the baseline's own
run-to-run spread (max - min over median) of the figure each ratio is judged against, and whether each ratio lies inside
1 + spread + 1 %.  Nothing is asserted about rates: a ratio outside the band is reported as measured.  Every retry is checked byte for
byte against its first call.  Writes profiles/return_replay_probe.json (or --out).

    python tools/return_replay_probe.py [--baseline-tree DIR] [--out f] [--log2 18] [--reps 5]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "return_replay_probe.json"))
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
    proofs = bench.make_distinct_proofs_on_device(eng, capi, torch, np, sk, N, L, seed=73)[0]
    print("made %d proofs in %.1f s" % (N, time.perf_counter() - t0), flush=True)
    PB, ML = eng.proof_bytes, eng.cbor_size("SpendProof")
    OB = {"records": {"base": 128, "new": 160}, "wire": {"base": eng.cbor_size("Refund"), "new": eng.cbor_size("RefundReturn")}}
    view = proofs.view(N, PB)
    spent = view[:, 32:64].contiguous()                            # s of every lane: returning all of it is the largest t the screen lets through
    zeros = torch.zeros(N * 32, dtype=torch.uint8, device="cuda")
    wire = torch.empty((N, ML), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eng._ck(eng.lib.act_cbor_encode_batch(eng.ctx, capi.CBOR_TYPES["SpendProof"], N, capi.MEM_DEVICE, view.data_ptr(), wire.data_ptr()))
    src = {"records": view.data_ptr(), "wire": wire.data_ptr()}
    ob_max = max(OB["wire"]["new"], 160)
    out = torch.empty(N * ob_max, dtype=torch.uint8, device="cuda"); keep = torch.empty(N * ob_max, dtype=torch.uint8, device="cuda")
    st = torch.empty(N, dtype=torch.uint8, device="cuda"); ok = torch.empty(N, dtype=torch.uint8, device="cuda"); rp = torch.empty(N, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    key = np.frombuffer(sk, np.uint8); ep = np.array([1], np.uint32); nonce_key = np.frombuffer(sh("rrp-nonce-key", 32), np.uint8)
    cnt = (C.c_uint64 * len(capi.RETURN_REPLAY_COUNTS))()
    returned = {"null": None, "zero": zeros.data_ptr(), "all": spent.data_ptr()}

    def pair(form, what):
        """a first call on empty sets, then the same batch again -> (seconds of the first call, seconds of the retry)"""
        base = what == "base"
        cp, e = (bcapi, beng) if base else (capi, eng)
        s, r = cp.NullifierSet(4 * N), cp.NullifierSet(4 * N)
        head = [e.ctx, s.h, r.h, N, cp.MEM_DEVICE, key.ctypes.data, 1, ep.ctypes.data, cp.SIGN_MATCHED, src[form]] + ([None] if form == "wire" else []) + [None]
        if base:
            fn = e.lib.act_redeem_cbor_admit_replay_batch if form == "wire" else e.lib.act_redeem_admit_replay_batch
        else:
            fn = e.lib.act_redeem_cbor_return_replay_batch if form == "wire" else e.lib.act_redeem_return_replay_batch
            head.append(returned[what])
        args = head + [nonce_key.ctypes.data, out.data_ptr(), st.data_ptr(), ok.data_ptr(), rp.data_ptr(), cnt]
        dts = []
        nbytes = N * OB[form]["base" if base else "new"]
        for turn in range(2):
            t = time.perf_counter()
            rc = fn(*args)
            dts.append(time.perf_counter() - t)
            if rc:
                raise RuntimeError("%s %s: rc %d %s" % (form, what, rc, e.lib.act_last_error(e.ctx).decode()))
            assert int(cnt[7 + turn]) == N and (len(s), len(r)) == (N, N), (form, what, turn, list(cnt))      # every lane fresh, then every lane replayed
            if turn == 0:
                keep[:nbytes].copy_(out[:nbytes])
            else:
                assert bool(torch.equal(out[:nbytes], keep[:nbytes])), "a retried batch did not get its refunds again"
        s.close(); r.close()
        return dts

    kinds = ("base", "null", "zero", "all")
    forms = ("records", "wire")
    for form in forms:
        for what in kinds:                                          # warm-up: side buffers, staging, code objects
            pair(form, what)
    t = {form: {k: [] for k in kinds + ("base_retry", "all_retry")} for form in forms}
    for _ in range(REPS):
        for form in forms:
            for what in kinds:                                      # alternating: drift of the box hits all alike
                first, again = pair(form, what)
                t[form][what].append(first)
                if what in ("base", "all"):
                    t[form][what + "_retry"].append(again)
    res = {"tool": "tools/return_replay_probe.py", "device": torch.cuda.get_device_name(0), "L": L, "lanes": N, "reps": REPS, "transcripts": "device",
           "baseline": "act_redeem_(cbor_)admit_replay_batch of " + ("the library under --baseline-tree" if a.baseline_tree else "THIS library (no --baseline-tree given)"),
           "forms": {}}
    for form in forms:
        med = {k: statistics.median(v) for k, v in t[form].items()}
        spread = {k: (max(t[form][k]) - min(t[form][k])) / med[k] for k in ("base", "base_retry")}
        against = {"null": "base", "zero": "base", "all": "base", "all_retry": "base_retry"}
        row = {"seconds": t[form], "median_s": med, "lanes_per_s": {k: N / v for k, v in med.items()}, "baseline_spread": spread,
               "band": {k: 1.0 + spread[b] + 0.01 for k, b in against.items()},
               "ratio_to_base": {k: med[k] / med[b] for k, b in against.items()},
               "inside_band": {k: med[k] / med[b] <= 1.0 + spread[b] + 0.01 for k, b in against.items()}}
        res["forms"][form] = row
        print(json.dumps({"form": form, **{k: row[k] for k in ("median_s", "baseline_spread", "band", "ratio_to_base", "inside_band")}}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    eng.close()
    if beng is not eng:
        beng.close()


if __name__ == "__main__":
    main()
