"""Admission before verification: what the screen costs an honest batch and what it spares a batch of replays, against the existing
redeem call, in one process, alternating (tools/README.md).

One MI355X, L = 128, 2^18 distinct proofs resident in HBM, records and wire (canonical CBOR messages), device transcripts, the
context's default max_batch.  The nullifier set is preloaded so that a fraction f of the batch replays, f in {0, 1/2, 7/8, 1}.  Per f
and form, three repetitions of
    (new)   act_redeem_admit_batch / act_redeem_cbor_admit_batch, charge == NULL
    (base)  act_redeem_keyring_epochs_batch / act_redeem_cbor_keyring_epochs_batch -- existing code, the baseline
run alternately, each on a set freshly restored from one export (the restore is outside the timing), ring of one key, sequential
rng.  Reported: median lanes/s of both, new / base, the bound 1 / (1 - f), the baseline's own run-to-run spread (max - min over
median), and the counts the new call returned.  Then the one-item latency in host memory beside act_redeem_batch's.
Writes profiles/admission_probe.json (or --out).

    python tools/admission_probe.py [--out f] [--log2 18] [--reps 3]
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
import act_amd  # noqa: E402,F401
from act_amd import capi  # noqa: E402
import bench  # noqa: E402


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "admission_probe.json"))
    ap.add_argument("--log2", type=int, default=18)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    N, L, REPS = 1 << a.log2, 128, a.reps
    sh = lambda tag, n: hashlib.shake_256(tag.encode()).digest(n)
    h = capi.params_new("bench-org", "bench-service", "bench-env", "2024-01-01", device=0)
    eng = capi.Engine(h, L, device=0, transcript=capi.TRANSCRIPT_DEVICE)
    lib, ctx = eng.lib, eng.ctx
    sk = eng.private_key_random(sh("adp-sk", 64))
    t0 = time.perf_counter()
    proofs = bench.make_distinct_proofs_on_device(eng, capi, torch, np, sk, N, L, seed=61)[0]
    PB, ML, RB = eng.proof_bytes, eng.cbor_size("SpendProof"), eng.cbor_size("Refund")
    wire = torch.empty(N * ML, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eng._ck(lib.act_cbor_encode_batch(ctx, capi.CBOR_TYPES["SpendProof"], N, capi.MEM_DEVICE, proofs.data_ptr(), wire.data_ptr()))
    print("made %d proofs and their messages in %.1f s" % (N, time.perf_counter() - t0), flush=True)
    nul = proofs[:, :32].contiguous()
    rng = torch.randint(0, 256, (N * 128,), dtype=torch.uint8, device="cuda")
    out = torch.empty(N * max(128, RB), dtype=torch.uint8, device="cuda")
    st = torch.empty(N, dtype=torch.uint8, device="cuda"); ok = torch.empty(N, dtype=torch.uint8, device="cuda"); sp = torch.empty(N, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    key = np.frombuffer(sk, np.uint8); ep = np.array([1], np.uint32)
    cnt = (C.c_uint64 * len(capi.ADMIT_COUNTS))()

    def restored(replay):
        s = capi.NullifierSet(2 * N)
        if replay.numel():
            keys = nul.index_select(0, replay).contiguous(); torch.cuda.synchronize()
            s.check_and_insert_dev(replay.numel(), keys.data_ptr(), 32, 0, sp.data_ptr())
        return s

    def run(new, form, s):
        args = [ctx, s.h, N, capi.MEM_DEVICE, key.ctypes.data, 1, ep.ctypes.data, capi.SIGN_MATCHED]
        args += [proofs.data_ptr()] if form == "records" else [wire.data_ptr(), None]
        if new:
            args.append(None)
        args += [rng.data_ptr(), capi.RNG_SEQUENTIAL, out.data_ptr(), st.data_ptr(), ok.data_ptr()]
        if new:
            args.append(cnt)
        fn = {(True, "records"): lib.act_redeem_admit_batch, (True, "wire"): lib.act_redeem_cbor_admit_batch,
              (False, "records"): lib.act_redeem_keyring_epochs_batch, (False, "wire"): lib.act_redeem_cbor_keyring_epochs_batch}[(new, form)]
        t = time.perf_counter()
        rc = fn(*args)
        dt = time.perf_counter() - t
        if rc:
            raise RuntimeError("%s: rc %d %s" % (fn.__name__, rc, lib.act_last_error(ctx).decode()))
        return dt

    rows = []
    for form in ("records", "wire"):
        for num, den in ((0, 1), (1, 2), (7, 8), (1, 1)):
            lane = torch.arange(N, device="cuda")
            replay = lane[(lane % den) < num] if num else lane[:0]
            f = replay.numel() / N
            for new in (True, False):                                   # warm-up: side buffers, staging, code objects
                s = restored(replay); run(new, form, s); s.close()
            t = {True: [], False: []}
            counts = None
            for _ in range(REPS):
                for new in (True, False):                               # alternating: drift of the box hits both alike
                    s = restored(replay)
                    t[new].append(run(new, form, s))
                    if new:
                        counts = dict(zip(capi.ADMIT_COUNTS, (int(v) for v in cnt)))
                        assert counts["spent_before"] == replay.numel() and counts["accepted"] == N - replay.numel(), counts
                    assert len(s) == N
                    s.close()
            med = {k: statistics.median(v) for k, v in t.items()}
            row = {"form": form, "f": f, "lanes": N, "new_lanes_per_s": N / med[True], "base_lanes_per_s": N / med[False], "ratio": med[False] / med[True],
                   "bound": (1 / (1 - f)) if f < 1 else None, "new_s": t[True], "base_s": t[False],
                   "base_spread": (max(t[False]) - min(t[False])) / med[False], "new_spread": (max(t[True]) - min(t[True])) / med[True], "counts": counts}
            rows.append(row)
            print(json.dumps({k: row[k] for k in ("form", "f", "new_lanes_per_s", "base_lanes_per_s", "ratio", "bound", "base_spread")}), flush=True)
    # one item at a time, host memory: the admission call beside act_redeem_batch (distinct proofs, empty sets)
    K = 48
    host = proofs[:2 * K].cpu().numpy()
    r1 = sh("adp-one", 128)
    lat = {"admit": [], "redeem": []}
    sa, sb = capi.NullifierSet(4096), capi.NullifierSet(4096)
    for i in range(K):
        p = host[i].tobytes(); q = host[K + i].tobytes()
        t = time.perf_counter(); eng.redeem_admit(sa, [sk], p, r1, capi.RNG_PER_LANE); lat["admit"].append(time.perf_counter() - t)
        t = time.perf_counter(); eng.redeem(sb, sk, q, r1, capi.RNG_PER_LANE); lat["redeem"].append(time.perf_counter() - t)
    sa.close(); sb.close()
    one = {k: {"median_ms": 1e3 * statistics.median(v[8:]), "min_ms": 1e3 * min(v[8:])} for k, v in lat.items()}
    print("one item, host memory:", one, flush=True)
    res = {"tool": "tools/admission_probe.py", "device": torch.cuda.get_device_name(0), "L": L, "lanes": N, "reps": REPS, "transcripts": "device",
           "rows": rows, "one_item_host_ms": one}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
