"""Key rotation: what a ring of issuer keys costs, against the one-key call and against what a caller does without it, in one
process, alternating (tools/README.md).

One MI355X, L = 128, 2^18 distinct proofs resident in HBM, the context's default max_batch (65 536), host and device transcripts.
Two workloads per ring size:
    last     every proof issued under the LAST ring key (worst case: every candidate is computed, none matches early)
    split    the proofs split evenly over the ring's keys (a rotation's steady state)
Three paths, run one after the other in every repetition; the table shows the median rate in proofs/s:
    (a) one-key   act_verify_spend_batch under one key -- unchanged code, the parent commit's rate
    (b) ring      act_verify_spend_keyring_batch with nkeys = 1, 2, 4
    (c) passes    what a caller does today: nkeys one-key passes, each over the lanes the previous pass rejected (the rejected lanes
                  are gathered on the device between the passes; that gather is inside the timing, it is part of the method)
To be read against (a) and (c): (b) has to beat (c), and the field-operation count (tests/test_keyring_host.py) predicts
(b)/(a) ~ 1 - 0.01 (nkeys - 1) at worst.  One extra, untimed pair of runs per mode collects the per-kernel times (act_prof_get) and the
host hashing time (act_ctx_host_hash_stats) of (a) and of (b) at nkeys = 2, so that a shortfall can be attributed to a stage.
Writes profiles/keyring_probe.txt (or the path given as the first argument).

    python tools/keyring_probe.py [out.txt] [log2_proofs]
"""
import ctypes as C
import hashlib
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


def main():
    import torch
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "keyring_probe.txt")
    N = 1 << (int(sys.argv[2]) if len(sys.argv) > 2 else 18)
    L, REPS = 128, 3
    sh = lambda tag, n: hashlib.shake_256(tag.encode()).digest(n)
    h = capi.params_new("bench-org", "bench-service", "bench-env", "2024-01-01", device=0)
    eng = capi.Engine(h, L, device=0, transcript=capi.TRANSCRIPT_DEVICE)
    lib, ctx = eng.lib, eng.ctx
    PB = eng.proof_bytes
    keys = [eng.private_key_random(sh("krp-sk-%d" % i, 64)) for i in range(4)]
    A, B, Cc, D = keys
    t0 = time.perf_counter()
    made = {}

    def proofs_under(k, n):
        if (k, n) not in made:
            made[(k, n)] = bench.make_distinct_proofs_on_device(eng, capi, torch, np, keys[k], n, L, seed=100 + k)[0]
        return made[(k, n)]
    last = proofs_under(0, N)                                                   # every proof under A: rings end in A
    split = {1: last,
             2: torch.cat([last[:N // 2], proofs_under(1, N // 2)]),
             4: torch.cat([last[:N // 4], proofs_under(1, N // 2)[:N // 4], proofs_under(2, N // 4), proofs_under(3, N // 4)])}
    rings = {"last": {1: [A], 2: [B, A], 4: [B, Cc, D, A]}, "split": {1: [A], 2: [A, B], 4: [A, B, Cc, D]}}
    data = {"last": {1: last, 2: last, 4: last}, "split": split}
    print("made %d proofs under 4 keys in %.1f s" % (sum(v.shape[0] for v in made.values()), time.perf_counter() - t0), flush=True)
    st = torch.zeros(N, dtype=torch.uint8, device="cuda"); ok = torch.zeros(N, dtype=torch.uint8, device="cuda")
    st2 = torch.zeros(N, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def ck(rc, what):
        if rc:
            raise RuntimeError("%s: %s %s" % (what, capi._ERRS.get(rc, rc), lib.act_last_error(ctx).decode()))

    def keyp(ring):
        a = np.frombuffer(b"".join(ring), np.uint8)
        return a, a.ctypes.data

    def one_key(proofs, sk):
        k, p = keyp([sk])
        ck(lib.act_verify_spend_batch(ctx, proofs.shape[0], capi.MEM_DEVICE, p, proofs.data_ptr(), st.data_ptr(), None), "one-key")

    def ring_call(proofs, ring):
        k, p = keyp(ring)
        ck(lib.act_verify_spend_keyring_batch(ctx, proofs.shape[0], capi.MEM_DEVICE, p, len(ring), proofs.data_ptr(), st.data_ptr(), ok.data_ptr(), None), "ring")

    def passes(proofs, ring):
        """nkeys one-key passes; pass i takes the lanes pass i-1 rejected.  Returns accepted lanes."""
        cur, accepted = proofs, 0
        for i, sk in enumerate(ring):
            m = cur.shape[0]
            if m == 0:
                break
            k, p = keyp([sk])
            ck(lib.act_verify_spend_batch(ctx, m, capi.MEM_DEVICE, p, cur.data_ptr(), st2.data_ptr(), None), "pass")
            rej = torch.nonzero(st2[:m] == 7).flatten()
            accepted += m - rej.numel()
            if i + 1 < len(ring) and rej.numel():
                cur = cur.index_select(0, rej); torch.cuda.synchronize()
            else:
                cur = cur[:0]
        return accepted

    def timed(fn):
        t = time.perf_counter(); fn(); return time.perf_counter() - t

    def stage_times(fn):
        """per-kernel milliseconds and the host hashing seconds of one untimed run"""
        eng.prof_enable(True); eng.prof_reset()
        w, hs, by = C.c_double(0), C.c_double(0), C.c_uint64(0)
        lib.act_ctx_host_hash_stats(ctx, None, None, None, 1)
        fn()
        lib.act_ctx_host_hash_stats(ctx, C.byref(w), C.byref(hs), C.byref(by), 1)
        pr = {k: v for k, v in eng.prof().items()}
        eng.prof_enable(False)
        return pr, hs.value, w.value

    rows, stages = [], []
    for mode, mname in ((capi.TRANSCRIPT_HOST, "host"), (capi.TRANSCRIPT_DEVICE, "device")):
        eng.set_transcript_mode(mode)
        for wl in ("last", "split"):
            paths = [("a", lambda: one_key(data[wl][1], A))]
            for nk in (1, 2, 4):
                paths.append(("b%d" % nk, lambda nk=nk: ring_call(data[wl][nk], rings[wl][nk])))
            for nk in (2, 4):
                paths.append(("c%d" % nk, lambda nk=nk: passes(data[wl][nk], rings[wl][nk])))
            for name, fn in paths:                                     # warm-up: side buffers, staging, code objects
                fn()
            # every lane verifies, under the key it was issued under
            for nk in (1, 2, 4):
                ring_call(data[wl][nk], rings[wl][nk]); torch.cuda.synchronize()
                assert int(st.count_nonzero()) == 0, "a valid proof was rejected"
                want = (nk - 1) if wl == "last" else None
                hist = torch.bincount(ok.to(torch.int64), minlength=4).tolist()
                assert hist[:nk] == ([0] * (nk - 1) + [N] if want is not None else [N // nk] * nk), (wl, nk, hist)
                assert passes(data[wl][nk], rings[wl][nk]) == N
            t = {name: [] for name, _ in paths}
            for _ in range(REPS):
                for name, fn in paths:                                 # alternating: drift of the box hits all paths alike
                    t[name].append(timed(fn))
            med = {name: N / statistics.median(v) for name, v in t.items()}
            spread = {name: (max(v) - min(v)) / statistics.median(v) for name, v in t.items()}
            rows.append((mname, wl, med, spread))
            print(mname, wl, {k: round(v) for k, v in med.items()}, flush=True)
        pa = stage_times(lambda: one_key(last, A))
        pb = stage_times(lambda: ring_call(last, rings["last"][2]))
        stages.append((mname, pa, pb))

    lines = ["# tools/keyring_probe.py: spend verification against a ring of issuer keys, proofs/s (median of %d alternating repetitions)" % REPS,
             "# one MI355X, L = 128, %d distinct proofs resident in HBM, max_batch 65536, 16-bit fixed-base windows" % N,
             "# (a) act_verify_spend_batch, one key   (b) act_verify_spend_keyring_batch, nkeys = 1 / 2 / 4   (c) nkeys one-key passes over the rejected lanes",
             "# workload last: every proof under the LAST ring key; split: proofs split evenly over the ring's keys",
             "%-7s %-6s %10s %10s %10s %10s %10s %10s | %7s %7s %7s | %9s %9s | %s" % ("transcr", "load", "(a)", "(b) 1", "(b) 2", "(b) 4", "(c) 2", "(c) 4",
                                                                                      "b1/a", "b2/a", "b4/a", "b2/c2", "b4/c4", "max spread")]
    for mname, wl, med, spread in rows:
        lines.append("%-7s %-6s %10.0f %10.0f %10.0f %10.0f %10.0f %10.0f | %7.3f %7.3f %7.3f | %9.3f %9.3f | %.1f %%" % (
            mname, wl, med["a"], med["b1"], med["b2"], med["b4"], med["c2"], med["c4"], med["b1"] / med["a"], med["b2"] / med["a"], med["b4"] / med["a"],
            med["b2"] / med["c2"], med["b4"] / med["c4"], 100 * max(spread.values())))
    lines.append("# stages of one untimed run over the `last` workload with event timing on (ms summed over launches; the two slots' kernels overlap):")
    for mname, (pa, ha, wa), (pb, hb, wb) in stages:
        names = [k for k in pb if pb[k]["ms"] > 0 or (k in pa and pa[k]["ms"] > 0)]
        lines.append("#   %s transcripts: host hashing %.3f s one-key, %.3f s ring nkeys=2 (waited for the device %.3f / %.3f s)" % (mname, ha, hb, wa, wb))
        for k in names:
            lines.append("#     %-24s one-key %9.1f ms   ring nkeys=2 %9.1f ms" % (k, pa.get(k, {"ms": 0})["ms"], pb[k]["ms"]))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    eng.close()


if __name__ == "__main__":
    main()
