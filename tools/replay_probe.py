"""Replayable redemption: what the derived nonces and the receipts set cost an honest batch, and what a batch of retries costs.  A/B
against the PARENT commit's build on one box (tools/README.md; the protocol of tools/copies_probe.py).

The parent tree (a checkout of the parent commit with its library built) and this tree are measured by child processes, alternating,
`--reps` times each (a child imports the package of the tree it is given, so each build runs behind its own binding).  Per child, on
one MI355X: L = 128, 2^log2 distinct valid proofs made on the device, device transcripts, a ring of one key with an epoch, empty sets
of 2 n slots per cell.  Cells: records and wire (canonical messages of one size), the batch in HBM and in host memory.  Per cell one
warm-up call on sets of its own, then
    parent     act_redeem_(cbor_)keyring_epochs_batch, per-lane rng bytes                -- the baseline: an honest batch
    this tree  act_redeem_(cbor_)replay_batch on empty sets (honest: every lane fresh), then THE SAME BATCH AGAIN on the same sets
               (every lane a replay, checked byte for byte against the first call's output)
Reported per cell: the times of every repetition, median lanes/s, both ratios to the baseline, the baseline's own run-to-run spread
(max - min over median).  No pass mark: the figures go into DESIGN 4.8.

    python tools/replay_probe.py --parent DIR [--out profiles/replay_probe.json] [--reps 3] [--log2 18] [--no-host]
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(root, log2, with_host):
    sys.path.insert(0, root)
    os.chdir(root)
    import numpy as np
    import torch
    import act_amd  # noqa: F401
    from act_amd import capi
    import bench
    N, L = 1 << log2, 128
    sh = lambda tag, n: hashlib.shake_256(tag.encode()).digest(n)
    replay = "act_redeem_replay_batch" in capi.EXPORTS
    h = capi.params_new("bench-org", "bench-service", "bench-env", "2024-01-01", device=0)
    eng = capi.Engine(h, L, device=0, transcript=capi.TRANSCRIPT_DEVICE)
    lib, ctx = eng.lib, eng.ctx
    sk = eng.private_key_random(sh("rpp-sk", 64))
    t0 = time.perf_counter()
    proofs = bench.make_distinct_proofs_on_device(eng, capi, torch, np, sk, N, L, seed=67)[0]
    ML, RB = eng.cbor_size("SpendProof"), eng.cbor_size("Refund")
    wire = torch.empty((N, ML), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eng._ck(lib.act_cbor_encode_batch(ctx, capi.CBOR_TYPES["SpendProof"], N, capi.MEM_DEVICE, proofs.data_ptr(), wire.data_ptr()))
    made_s = time.perf_counter() - t0
    rng = torch.randint(0, 256, (N * 128,), dtype=torch.uint8, device="cuda")
    ob = max(128, RB)
    out = torch.empty(N * ob, dtype=torch.uint8, device="cuda"); keep = torch.empty(N * ob, dtype=torch.uint8, device="cuda")
    st = torch.empty(N, dtype=torch.uint8, device="cuda"); ok = torch.empty(N, dtype=torch.uint8, device="cuda"); rp = torch.empty(N, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    h_rng = rng.cpu().numpy(); h_out = np.empty(N * ob, np.uint8); h_keep = np.empty(N * ob, np.uint8)
    h_st = np.empty(N, np.uint8); h_ok = np.empty(N, np.uint8); h_rp = np.empty(N, np.uint8)
    key = np.frombuffer(sk, np.uint8); ep = np.array([1], np.uint32); nonce_key = np.frombuffer(sh("rpp-nonce-key", 32), np.uint8)
    cnt = (C.c_uint64 * 6)()

    def call(form, dev, src_ptr, s, r):
        mem = capi.MEM_DEVICE if dev else capi.MEM_HOST
        o, s_, k_, r_ = (out.data_ptr(), st.data_ptr(), ok.data_ptr(), rp.data_ptr()) if dev else (h_out.ctypes.data, h_st.ctypes.data, h_ok.ctypes.data, h_rp.ctypes.data)
        if replay:
            head = [ctx, s.h, r.h, N, mem, key.ctypes.data, 1, ep.ctypes.data, capi.SIGN_MATCHED, src_ptr] + ([None] if form == "wire" else [])
            fn = lib.act_redeem_cbor_replay_batch if form == "wire" else lib.act_redeem_replay_batch
            args = head + [nonce_key.ctypes.data, o, s_, k_, r_, cnt]
        else:
            head = [ctx, s.h, N, mem, key.ctypes.data, 1, ep.ctypes.data, capi.SIGN_MATCHED, src_ptr] + ([None] if form == "wire" else [])
            fn = lib.act_redeem_cbor_keyring_epochs_batch if form == "wire" else lib.act_redeem_keyring_epochs_batch
            args = head + [rng.data_ptr() if dev else h_rng.ctypes.data, capi.RNG_PER_LANE, o, s_, k_]
        t = time.perf_counter()
        rc = fn(*args)
        dt = time.perf_counter() - t
        if rc:
            raise RuntimeError("%s %s: rc %d %s" % (form, "hbm" if dev else "host", rc, lib.act_last_error(ctx).decode()))
        return dt

    def accepted(dev):
        return int((st == 0).sum().item()) if dev else int((h_st == 0).sum())

    cells = []
    for form, table in (("records", proofs), ("wire", wire)):
        for mem in ("hbm", "host") if with_host else ("hbm",):
            dev = mem == "hbm"
            host = table.cpu().numpy() if not dev else None
            ptr = table.data_ptr() if dev else host.ctypes.data
            s, r = capi.NullifierSet(2 * N), capi.NullifierSet(2 * N)
            call(form, dev, ptr, s, r)                                  # warm-up: side buffers, staging, code objects
            s.close(); r.close()
            s, r = capi.NullifierSet(2 * N), capi.NullifierSet(2 * N)
            cell = {"form": form, "mem": mem, "honest_s": call(form, dev, ptr, s, r)}
            assert accepted(dev) == N == len(s), (accepted(dev), len(s))
            if replay:
                counts = dict(zip(capi.REPLAY_COUNTS, (int(v) for v in cnt)))
                assert counts["fresh"] == N and len(r) == N, counts
                if dev:
                    keep.copy_(out)
                else:
                    h_keep[:] = h_out
                cell["replay_s"] = call(form, dev, ptr, s, r)
                counts = dict(zip(capi.REPLAY_COUNTS, (int(v) for v in cnt)))
                assert counts["replayed"] == N and (len(s), len(r)) == (N, N), counts
                same = bool(torch.equal(out, keep)) if dev else bool((h_out == h_keep).all())
                assert same, "a retried batch did not get its refunds again"
                cell["replay_counts"] = counts
            s.close(); r.close()
            cells.append(cell)
            del host
    res = {"root": root, "replay": replay, "lanes": N, "made_proofs_s": made_s, "cells": cells, "device": torch.cuda.get_device_name(0)}
    eng.close()
    print("CHILD " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a checkout of the parent commit with its library built")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "replay_probe.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--log2", type=int, default=18)
    ap.add_argument("--no-host", action="store_true", help="leave the host-memory cells out")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(os.path.abspath(a.child), a.log2, not a.no_host)
    if not a.parent:
        ap.error("--parent DIR is required")
    runs = {"parent": [], "this": []}
    for rep in range(a.reps):
        for name, root in (("parent", os.path.abspath(a.parent)), ("this", HERE)):      # alternating: drift of the box hits both alike
            cmd = [sys.executable, os.path.abspath(__file__), "--child", root, "--log2", str(a.log2)] + (["--no-host"] if a.no_host else [])
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("CHILD ")]
            if r.returncode != 0 or not line:                           # nothing more is started on the device behind a failed child
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit("the %s child failed (exit %d)" % (name, r.returncode))
            runs[name].append(json.loads(line[0][6:]))
            print("rep %d %s: %s" % (rep, name, [("%.3f" % c["honest_s"], "%.3f" % c.get("replay_s", 0)) for c in runs[name][-1]["cells"]]), flush=True)
    assert not runs["parent"][0]["replay"] and runs["this"][0]["replay"]
    rows = []
    n = runs["this"][0]["lanes"]
    for k, cell in enumerate(runs["this"][0]["cells"]):
        honest = [r["cells"][k]["honest_s"] for r in runs["this"]]; again = [r["cells"][k]["replay_s"] for r in runs["this"]]
        base = [r["cells"][k]["honest_s"] for r in runs["parent"]]
        mh, ma, mb = statistics.median(honest), statistics.median(again), statistics.median(base)
        row = {"form": cell["form"], "mem": cell["mem"], "lanes": n, "base_lanes_per_s": n / mb, "honest_lanes_per_s": n / mh, "replay_lanes_per_s": n / ma,
               "honest_ratio": mb / mh, "replay_ratio": mb / ma, "base_spread": (max(base) - min(base)) / mb, "honest_spread": (max(honest) - min(honest)) / mh,
               "base_s": base, "honest_s": honest, "replay_s": again}
        rows.append(row)
        print(json.dumps({k2: row[k2] for k2 in ("form", "mem", "base_lanes_per_s", "honest_lanes_per_s", "replay_lanes_per_s", "honest_ratio", "replay_ratio", "base_spread")}), flush=True)
    res = {"tool": "tools/replay_probe.py", "device": runs["this"][0]["device"], "L": 128, "lanes": n, "reps": a.reps, "transcripts": "device",
           "baseline": "act_redeem_(cbor_)keyring_epochs_batch of the parent commit's build, an honest batch, per-lane rng bytes", "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
