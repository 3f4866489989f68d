"""Admission, unique forms: what the copy stage costs a batch without copies and what it spares a batch with them.  A/B against the
PARENT commit's build on one box (tools/README.md).

The parent tree (a checkout of the parent commit with its library built: `git worktree add DIR HEAD~; make -C
DIR/anonymous-credit-tokens_amd/csrc`) and this tree are measured by child processes, alternating, `--reps` times each (a child imports
the package of the tree it is given, so each build runs behind its own binding).  Per child, on one MI355X: L = 128, 2^log2 distinct
valid proofs made on the device, device transcripts, a ring of one key, sequential rng, an empty set of 2 n slots per call.  A batch
with copy fraction f repeats, in a seeded fraction f of its lanes, the bytes of an earlier lane that is not itself a repeat; the flood
is one proof n times.  Cells: records and wire (canonical messages of one size), the batch in HBM and in host memory (where the
fingerprint and the compare run on the host workers), f in {0, 1/2, 7/8, flood}.  Per cell one warm-up and one timed call of
    parent     act_redeem_admit_batch / act_redeem_cbor_admit_batch         -- the baseline: verifies every lane
    this tree  act_redeem_admit_unique_batch / act_redeem_cbor_admit_unique_batch
Reported per cell: the times of every repetition, median lanes/s of both, ratio, the bound 1 / (1 - f), the baseline's own run-to-run
spread (max - min over median), the counts.  Also the leader table alone over n equal fingerprints (every lane on one slot).
No pass mark: the figures go into DESIGN 4.7.

    python tools/copies_probe.py --parent DIR [--out profiles/admission_copies_probe.json] [--reps 3] [--log2 18] [--no-host]
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
FRACTIONS = ((0, 1), (1, 2), (7, 8), (1, 1))      # (1, 1): the flood


def copy_sources(torch, n, num, den, seed=71):
    """src[i] = the lane whose bytes lane i carries: itself, or an earlier lane that carries its own (seeded; lane 0 is its own)"""
    lane = torch.arange(n, device="cuda")
    if (num, den) == (1, 1):
        return torch.zeros_like(lane)
    if num == 0:
        return lane
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    own = torch.rand(n, device="cuda", generator=g) * den >= num
    own[0] = True
    before = torch.cumsum(own.to(torch.int64), 0) - own.to(torch.int64)          # own lanes below lane i
    owners = lane[own]
    pick = (torch.rand(n, device="cuda", generator=g) * before.clamp(min=1).to(torch.float64)).to(torch.int64).clamp(max=owners.numel() - 1)
    pick = torch.minimum(pick, (before - 1).clamp(min=0))
    return torch.where(own, lane, owners[pick])


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
    unique = "act_redeem_admit_unique_batch" in capi.EXPORTS
    names = capi.ADMIT_UNIQUE_COUNTS if unique else capi.ADMIT_COUNTS
    h = capi.params_new("bench-org", "bench-service", "bench-env", "2024-01-01", device=0)
    eng = capi.Engine(h, L, device=0, transcript=capi.TRANSCRIPT_DEVICE)
    lib, ctx = eng.lib, eng.ctx
    sk = eng.private_key_random(sh("cpp-sk", 64))
    t0 = time.perf_counter()
    proofs = bench.make_distinct_proofs_on_device(eng, capi, torch, np, sk, N, L, seed=67)[0]
    PB, ML, RB = eng.proof_bytes, eng.cbor_size("SpendProof"), eng.cbor_size("Refund")
    wire = torch.empty((N, ML), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eng._ck(lib.act_cbor_encode_batch(ctx, capi.CBOR_TYPES["SpendProof"], N, capi.MEM_DEVICE, proofs.data_ptr(), wire.data_ptr()))
    made_s = time.perf_counter() - t0
    rng = torch.randint(0, 256, (N * 128,), dtype=torch.uint8, device="cuda")
    out = torch.empty(N * max(128, RB), dtype=torch.uint8, device="cuda")
    st = torch.empty(N, dtype=torch.uint8, device="cuda"); ok = torch.empty(N, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    h_rng = rng.cpu().numpy(); h_out = np.empty(N * max(128, RB), np.uint8); h_st = np.empty(N, np.uint8); h_ok = np.empty(N, np.uint8)
    key = np.frombuffer(sk, np.uint8); ep = np.array([1], np.uint32)
    cnt = (C.c_uint64 * len(names))()
    fn = {("records", True): "act_redeem_admit_unique_batch", ("wire", True): "act_redeem_cbor_admit_unique_batch",
          ("records", False): "act_redeem_admit_batch", ("wire", False): "act_redeem_cbor_admit_batch"}

    def run(form, mem, src_ptr):
        s = capi.NullifierSet(2 * N)
        dev = mem == "hbm"
        args = [ctx, s.h, N, capi.MEM_DEVICE if dev else capi.MEM_HOST, key.ctypes.data, 1, ep.ctypes.data, capi.SIGN_MATCHED, src_ptr]
        if form == "wire":
            args.append(None)                                           # messages of one size: no offsets
        args += [None, rng.data_ptr() if dev else h_rng.ctypes.data, capi.RNG_SEQUENTIAL, out.data_ptr() if dev else h_out.ctypes.data,
                 st.data_ptr() if dev else h_st.ctypes.data, ok.data_ptr() if dev else h_ok.ctypes.data, cnt]
        call = getattr(lib, fn[(form, unique)])
        t = time.perf_counter()
        rc = call(*args)
        dt = time.perf_counter() - t
        if rc:
            raise RuntimeError("%s: rc %d %s" % (fn[(form, unique)], rc, lib.act_last_error(ctx).decode()))
        counts = dict(zip(names, (int(v) for v in cnt)))
        size = len(s)
        s.close()
        return dt, counts, size

    cells = []
    for num, den in FRACTIONS:
        src = copy_sources(torch, N, num, den)
        distinct = int((src == torch.arange(N, device="cuda")).sum().item())
        for form, table in (("records", proofs), ("wire", wire)):
            batch = table.index_select(0, src).contiguous()
            torch.cuda.synchronize()
            for mem in ("hbm", "host") if with_host else ("hbm",):
                host = batch.cpu().numpy() if mem == "host" else None
                ptr = batch.data_ptr() if mem == "hbm" else host.ctypes.data
                run(form, mem, ptr)                                     # warm-up: side buffers, staging, code objects
                dt, counts, size = run(form, mem, ptr)
                assert counts["accepted"] == distinct == size and counts["lanes"] == N, (counts, distinct, size)
                if unique:
                    assert counts["copies"] == N - distinct and counts["verified"] == distinct, counts
                else:
                    assert counts["verified"] == N and counts["double_spend_after"] == N - distinct, counts
                cells.append({"form": form, "mem": mem, "f": (N - distinct) / N, "flood": (num, den) == (1, 1), "seconds": dt, "counts": counts})
                del host
            del batch
    res = {"root": root, "unique": unique, "lanes": N, "made_proofs_s": made_s, "cells": cells, "device": torch.cuda.get_device_name(0)}
    if unique:
        res["flood_leader_table_ms"] = [eng.copy_leaders(np.full(N, 0x1234567890ABCDEF, np.uint64))[1] for _ in range(4)][1:]
    eng.close()
    print("CHILD " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a checkout of the parent commit with its library built")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "admission_copies_probe.json"))
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
            print("rep %d %s: %s" % (rep, name, ["%.3f" % c["seconds"] for c in runs[name][-1]["cells"]]), flush=True)
    assert not runs["parent"][0]["unique"] and runs["this"][0]["unique"]
    rows = []
    n = runs["this"][0]["lanes"]
    for k, cell in enumerate(runs["this"][0]["cells"]):
        new = [r["cells"][k]["seconds"] for r in runs["this"]]; base = [r["cells"][k]["seconds"] for r in runs["parent"]]
        mn, mb = statistics.median(new), statistics.median(base)
        f = cell["f"]
        row = {"form": cell["form"], "mem": cell["mem"], "f": f, "flood": cell["flood"], "lanes": n, "unique_lanes_per_s": n / mn, "base_lanes_per_s": n / mb,
               "ratio": mb / mn, "bound": 1 / (1 - f), "unique_s": new, "base_s": base, "base_spread": (max(base) - min(base)) / mb,
               "unique_spread": (max(new) - min(new)) / mn, "counts": cell["counts"], "base_counts": runs["parent"][0]["cells"][k]["counts"]}
        rows.append(row)
        print(json.dumps({k2: row[k2] for k2 in ("form", "mem", "f", "unique_lanes_per_s", "base_lanes_per_s", "ratio", "bound", "base_spread")}), flush=True)
    res = {"tool": "tools/copies_probe.py", "device": runs["this"][0]["device"], "L": 128, "lanes": n, "reps": a.reps, "transcripts": "device",
           "baseline": "act_redeem_(cbor_)admit_batch of the parent commit's build", "rows": rows,
           "flood_leader_table_ms": [ms for r in runs["this"] for ms in r["flood_leader_table_ms"]]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
