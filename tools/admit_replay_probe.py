"""Admission for the replayable redemption: what the screen costs an honest batch, and what it saves on retries and foreign spends.  A/B
against the PARENT commit's build on one box (tools/README.md; the protocol of tools/replay_probe.py).

The parent tree (a checkout of the parent commit with its library built) and this tree are measured by child processes, alternating,
`--reps` times each (a child imports the package of the tree it is given, so each build runs behind its own binding).  Per child, on
one MI355X: L = 128, 2^log2 distinct valid proofs made on the device, device transcripts, a ring of one key with an epoch, sets of
4 n slots per cell.  Cells: records and wire (canonical messages of one size), the batch in HBM and in host memory.  Per cell one
warm-up call of every mix on sets of its own, then four mixes, each timed as ONE call:
    honest        every lane fresh, empty sets
    retries       the same batch again on the same sets: every lane a retry (checked byte for byte against the first call's output)
    foreign       every lane has a spent nullifier and another K': the recorded proofs with Com_0 taken from the next lane (a valid point,
                  so K' and the tag differ; the proof no longer verifies, which costs the baseline the same verification)
    half foreign  even lanes retries, odd lanes foreign
    parent     act_redeem_(cbor_)replay_batch                 -- the baseline: every spent lane is verified
    this tree  act_redeem_(cbor_)admit_replay_batch, charge == NULL
Reported per cell and mix: the times of every repetition, median lanes/s, the ratio to the baseline, the baseline's own run-to-run
spread (max - min over median), and this tree's counts.  No pass mark: the figures go into DESIGN 4.9.

    python tools/admit_replay_probe.py --parent DIR [--out profiles/admit_replay_probe.json] [--reps 3] [--log2 18] [--no-host]
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
MIXES = ("honest", "retries", "foreign", "half_foreign")


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
    admit = "act_redeem_admit_replay_batch" in capi.EXPORTS
    h = capi.params_new("bench-org", "bench-service", "bench-env", "2024-01-01", device=0)
    eng = capi.Engine(h, L, device=0, transcript=capi.TRANSCRIPT_DEVICE)
    lib, ctx = eng.lib, eng.ctx
    sk = eng.private_key_random(sh("arp-sk", 64))
    t0 = time.perf_counter()
    proofs = bench.make_distinct_proofs_on_device(eng, capi, torch, np, sk, N, L, seed=71)[0]
    PB, ML, RB = eng.proof_bytes, eng.cbor_size("SpendProof"), eng.cbor_size("Refund")
    # foreign spends: Com_0 (record field 4) of the next lane; half foreign: that on the odd lanes only
    view = proofs.view(N, PB)
    foreign = view.clone(); foreign[:, 128:160] = torch.roll(view[:, 128:160], 1, 0)
    half = view.clone(); half[1::2] = foreign[1::2]
    tables = {"records": {"honest": view, "retries": view, "foreign": foreign, "half_foreign": half}, "wire": {}}
    for name in ("honest", "foreign", "half_foreign"):
        wire = torch.empty((N, ML), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        eng._ck(lib.act_cbor_encode_batch(ctx, capi.CBOR_TYPES["SpendProof"], N, capi.MEM_DEVICE, tables["records"][name].data_ptr(), wire.data_ptr()))
        tables["wire"][name] = wire
    tables["wire"]["retries"] = tables["wire"]["honest"]
    made_s = time.perf_counter() - t0
    ob = max(128, RB)
    out = torch.empty(N * ob, dtype=torch.uint8, device="cuda"); keep = torch.empty(N * ob, dtype=torch.uint8, device="cuda")
    st = torch.empty(N, dtype=torch.uint8, device="cuda"); ok = torch.empty(N, dtype=torch.uint8, device="cuda"); rp = torch.empty(N, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    h_out = np.empty(N * ob, np.uint8); h_keep = np.empty(N * ob, np.uint8)
    h_st = np.empty(N, np.uint8); h_ok = np.empty(N, np.uint8); h_rp = np.empty(N, np.uint8)
    key = np.frombuffer(sk, np.uint8); ep = np.array([1], np.uint32); nonce_key = np.frombuffer(sh("arp-nonce-key", 32), np.uint8)
    cnt = (C.c_uint64 * (11 if admit else 6))()
    names = capi.ADMIT_REPLAY_COUNTS if admit else capi.REPLAY_COUNTS

    def call(form, dev, src_ptr, s, r):
        mem = capi.MEM_DEVICE if dev else capi.MEM_HOST
        o, s_, k_, r_ = (out.data_ptr(), st.data_ptr(), ok.data_ptr(), rp.data_ptr()) if dev else (h_out.ctypes.data, h_st.ctypes.data, h_ok.ctypes.data, h_rp.ctypes.data)
        head = [ctx, s.h, r.h, N, mem, key.ctypes.data, 1, ep.ctypes.data, capi.SIGN_MATCHED, src_ptr] + ([None] if form == "wire" else [])
        if admit:
            fn = lib.act_redeem_cbor_admit_replay_batch if form == "wire" else lib.act_redeem_admit_replay_batch
            head.append(None)                                           # charge == NULL
        else:
            fn = lib.act_redeem_cbor_replay_batch if form == "wire" else lib.act_redeem_replay_batch
        t = time.perf_counter()
        rc = fn(*(head + [nonce_key.ctypes.data, o, s_, k_, r_, cnt]))
        dt = time.perf_counter() - t
        if rc:
            raise RuntimeError("%s %s: rc %d %s" % (form, "hbm" if dev else "host", rc, lib.act_last_error(ctx).decode()))
        return dt, dict(zip(names, (int(v) for v in cnt)))

    def statuses(dev):
        return st.cpu().numpy() if dev else h_st

    cells = []
    for form in ("records", "wire"):
        for mem in ("hbm", "host") if with_host else ("hbm",):
            dev = mem == "hbm"
            held = {name: (t if dev else t.cpu().numpy()) for name, t in tables[form].items() if name != "retries"}
            held["retries"] = held["honest"]
            ptr = {name: (t.data_ptr() if dev else t.ctypes.data) for name, t in held.items()}
            s, r = capi.NullifierSet(4 * N), capi.NullifierSet(4 * N)
            # warm-up on sets of its own, every mix once: side buffers, staging, code objects, and the allocations of the roads that only
            # a batch with spent lanes takes (their times are kept: what a first call costs)
            warm = {m: call(form, dev, ptr[m], s, r)[0] for m in MIXES}
            s.close(); r.close()
            s, r = capi.NullifierSet(4 * N), capi.NullifierSet(4 * N)
            cell = {"form": form, "mem": mem, "s": {}, "counts": {}, "warmup_s": warm}
            cell["s"]["honest"], cell["counts"]["honest"] = call(form, dev, ptr["honest"], s, r)
            assert int((statuses(dev) == 0).sum()) == N == len(s) == len(r)
            if dev:
                keep.copy_(out)
            else:
                h_keep[:] = h_out
            cell["s"]["retries"], cell["counts"]["retries"] = call(form, dev, ptr["retries"], s, r)
            assert cell["counts"]["retries"]["replayed"] == N and (len(s), len(r)) == (N, N), cell["counts"]["retries"]
            assert bool(torch.equal(out, keep)) if dev else bool((h_out == h_keep).all()), "a retried batch did not get its refunds again"
            cell["s"]["foreign"], cell["counts"]["foreign"] = call(form, dev, ptr["foreign"], s, r)
            got = statuses(dev)
            assert int((got == 0).sum()) == 0 and (len(s), len(r)) == (N, N)
            if admit:
                assert int((got == 3).sum()) == N and cell["counts"]["foreign"]["foreign_spend"] == N and cell["counts"]["foreign"]["verified"] == 0
            cell["s"]["half_foreign"], cell["counts"]["half_foreign"] = call(form, dev, ptr["half_foreign"], s, r)
            got = statuses(dev)
            assert int((got[0::2] == 0).sum()) == N // 2 and int((got[1::2] == 0).sum()) == 0 and (len(s), len(r)) == (N, N)
            s.close(); r.close()
            cells.append(cell)
            del held, ptr
    res = {"root": root, "admit": admit, "lanes": N, "made_proofs_s": made_s, "cells": cells, "device": torch.cuda.get_device_name(0)}
    eng.close()
    print("CHILD " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a checkout of the parent commit with its library built")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "admit_replay_probe.json"))
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
            print("rep %d %s: %s" % (rep, name, [["%.3f" % c["s"][m] for m in MIXES] for c in runs[name][-1]["cells"]]), flush=True)
    assert not runs["parent"][0]["admit"] and runs["this"][0]["admit"]
    rows = []
    n = runs["this"][0]["lanes"]
    for k, cell in enumerate(runs["this"][0]["cells"]):
        row = {"form": cell["form"], "mem": cell["mem"], "lanes": n, "mixes": {}}
        for m in MIXES:
            new = [r["cells"][k]["s"][m] for r in runs["this"]]; base = [r["cells"][k]["s"][m] for r in runs["parent"]]
            mn, mb = statistics.median(new), statistics.median(base)
            row["mixes"][m] = {"base_lanes_per_s": n / mb, "lanes_per_s": n / mn, "ratio": mb / mn, "base_spread": (max(base) - min(base)) / mb,
                               "spread": (max(new) - min(new)) / mn, "base_s": base, "s": new, "warmup_s": [r["cells"][k]["warmup_s"][m] for r in runs["this"]],
                               "counts": cell["counts"][m]}
            print(json.dumps({"form": row["form"], "mem": row["mem"], "mix": m, **{k2: row["mixes"][m][k2] for k2 in ("base_lanes_per_s", "lanes_per_s", "ratio", "base_spread")}}), flush=True)
        rows.append(row)
    res = {"tool": "tools/admit_replay_probe.py", "device": runs["this"][0]["device"], "L": 128, "lanes": n, "reps": a.reps, "transcripts": "device",
           "baseline": "act_redeem_(cbor_)replay_batch of the parent commit's build on the same batch and sets", "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
