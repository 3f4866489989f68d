"""The wire reader: what a batch of respelled SpendProof messages costs, read on the GPU in the pipeline (this tree) and on the old
road (the PARENT commit's build: flagged messages verified as zero records, parsed serially on the calling thread behind the
pipeline, verified a second time).  A/B on one box (tools/README.md), the shape of tools/copies_probe.py.

The parent tree (a checkout of the parent commit with its library built: `git worktree add DIR HEAD~; make -C
DIR/anonymous-credit-tokens_amd/csrc`) and this tree are measured by child processes, alternating, `--reps` times each.  Per child, on
one MI355X: L = 128, 2^log2 distinct valid proofs made on the device, device transcripts.  A batch with share f of respelled messages
carries one of three spellings in the lanes i with i % den < num:
    indefinite   an indefinite-length map whose three arrays are indefinite-length too
    reversed     the seventeen entries in reversed key order
    duplicate    key 3 (A') twice, the first time with another valid point: the last one wins; forces the validating pass
Messages lie at one stride (the longest spelling; a canonical message is followed by padding, which from_cbor does not read), f = 0
is the canonical batch back to back without offsets.  Cells: act_verify_spend_cbor_batch and act_redeem_cbor_admit_batch (a ring of one
key, sequential rng, an empty set of 2 n slots per call), the batch in HBM and in host memory, f in {0, 1/64, 1/2, 1} per spelling.
One warm-up call per (call, memory) at f = 0, then one timed call per cell.
Reported per cell: every repetition's seconds, median messages/s of both builds, parent / this, this build's rate against its own
f = 0 rate (the bound), both builds' run-to-run spread (max - min over median).  This tree also reports, per spelling at f = 1 from
HBM, the reader kernels' time per chunk (plain and validating pass, from the engine's launch events: act_prof_get) beside that
chunk's k_spend_bits, and act_ctx_wire_stats.  No pass mark: the figures go into DESIGN 4.4.

    python tools/wire_reader_probe.py --parent DIR [--out profiles/wire_reader_probe.json] [--reps 3] [--log2 18] [--no-host]
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
FRACTIONS = ((1, 64), (1, 2), (1, 1))
SPELLINGS = ("indefinite", "reversed", "duplicate")
SPEC = [(1, 0), (2, 0), (3, 0), (4, 0), (5, 1), (6, 0), (7, 0), (8, 0), (9, 0), (10, 0), (11, 0), (12, 0), (13, 0), (14, 1), (15, 2), (16, 0), (17, 0)]      # (key, shape)


def spellings(L):
    """per spelling: (source column of every output byte or -1, constant byte where the source is -1) over the canonical message"""
    ah = 1 if L < 24 else 2 if L < 256 else 3
    pos, ents = 1, []                                   # [key col, value start, value end, shape]
    for key, shape in SPEC:
        k = pos; pos += 1
        v0 = pos
        pos += 34 if shape == 0 else ah + 34 * L if shape == 1 else ah + 69 * L
        ents.append((k, v0, pos, shape))
    ml = pos
    src = lambda a, b: [(c, 0) for c in range(a, b)]
    const = lambda v: [(-1, v)]
    out = {}
    ind = const(0xBF)
    for k, v0, v1, shape in ents:
        ind += src(k, k + 1) + (src(v0, v1) if shape == 0 else const(0x9F) + src(v0 + ah, v1) + const(0xFF))
    out["indefinite"] = ind + const(0xFF)
    rev = src(0, 1)
    for k, v0, v1, shape in ents[::-1]:
        rev += src(k, v1)
    out["reversed"] = rev
    out["duplicate"] = const(0xA0 | 18) + const(0x03) + src(ents[3][1], ents[3][2]) + src(1, ml)
    return ml, out


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
    has_reader = "act_ctx_set_wire_reader" in capi.EXPORTS
    h = capi.params_new("bench-org", "bench-service", "bench-env", "2024-01-01", device=0)
    eng = capi.Engine(h, L, device=0, transcript=capi.TRANSCRIPT_DEVICE)
    lib, ctx = eng.lib, eng.ctx
    sk = eng.private_key_random(sh("wrp-sk", 64))
    proofs = bench.make_distinct_proofs_on_device(eng, capi, torch, np, sk, N, L, seed=83)[0]
    ML, RB = eng.cbor_size("SpendProof"), eng.cbor_size("Refund")
    wire = torch.empty((N, ML), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eng._ck(lib.act_cbor_encode_batch(ctx, capi.CBOR_TYPES["SpendProof"], N, capi.MEM_DEVICE, proofs.data_ptr(), wire.data_ptr()))
    del proofs
    ml, maps = spellings(L)
    assert ml == ML
    S = max(len(v) for v in maps.values())
    offs = (np.arange(N + 1, dtype=np.uint64) * np.uint64(S))
    rng = torch.randint(0, 256, (N * 128,), dtype=torch.uint8, device="cuda")
    out = torch.empty(N * RB, dtype=torch.uint8, device="cuda")
    st = torch.empty(N, dtype=torch.uint8, device="cuda"); ok = torch.empty(N, dtype=torch.uint8, device="cuda"); kp = torch.empty(N * 32, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    h_rng = rng.cpu().numpy(); h_out = np.empty(N * RB, np.uint8); h_st = np.empty(N, np.uint8); h_ok = np.empty(N, np.uint8); h_kp = np.empty(N * 32, np.uint8)
    key = np.frombuffer(sk, np.uint8); ep = np.array([1], np.uint32)
    cnt = (C.c_uint64 * len(capi.ADMIT_COUNTS))()

    def run(call, mem, ptr, with_offsets):
        dev = mem == "hbm"
        o = offs.ctypes.data if with_offsets else None
        if call == "verify":
            t = time.perf_counter()
            rc = lib.act_verify_spend_cbor_batch(ctx, N, capi.MEM_DEVICE if dev else capi.MEM_HOST, key.ctypes.data, ptr, o, st.data_ptr() if dev else h_st.ctypes.data,
                                                 kp.data_ptr() if dev else h_kp.ctypes.data)
            dt = time.perf_counter() - t
        else:
            s = capi.NullifierSet(2 * N)
            t = time.perf_counter()
            rc = lib.act_redeem_cbor_admit_batch(ctx, s.h, N, capi.MEM_DEVICE if dev else capi.MEM_HOST, key.ctypes.data, 1, ep.ctypes.data, capi.SIGN_MATCHED, ptr, o, None,
                                                 rng.data_ptr() if dev else h_rng.ctypes.data, capi.RNG_SEQUENTIAL, out.data_ptr() if dev else h_out.ctypes.data,
                                                 st.data_ptr() if dev else h_st.ctypes.data, ok.data_ptr() if dev else h_ok.ctypes.data, cnt)
            dt = time.perf_counter() - t
            s.close()
        if rc:
            raise RuntimeError("%s: rc %d %s" % (call, rc, lib.act_last_error(ctx).decode()))
        accepted = int((st == 0).sum().item()) if dev else int((h_st == 0).sum())
        assert accepted == N, (call, mem, accepted)                      # every message is a valid proof, whatever its spelling
        return dt

    mems = ("hbm", "host") if with_host else ("hbm",)
    cells = []

    def measure(spelling, num, den, batch, with_offsets):
        torch.cuda.synchronize()
        for mem in mems:
            host = batch.cpu().numpy() if mem == "host" else None
            ptr = batch.data_ptr() if mem == "hbm" else host.ctypes.data
            for call in ("verify", "admit"):
                if spelling is None:
                    run(call, mem, ptr, with_offsets)                   # warm-up: side buffers, staging, code objects
                cells.append({"call": call, "mem": mem, "spelling": spelling, "f": num / den, "seconds": run(call, mem, ptr, with_offsets)})
            del host

    measure(None, 0, 1, wire, False)
    kernels = {}
    lane = torch.arange(N, device="cuda")
    for name in SPELLINGS:
        cols = maps[name]
        idx = torch.tensor([max(c, 0) for c, _ in cols], dtype=torch.int64, device="cuda")
        cmask = torch.tensor([c < 0 for c, _ in cols], dtype=torch.bool, device="cuda")
        cval = torch.tensor([v for _, v in cols], dtype=torch.uint8, device="cuda")
        for num, den in FRACTIONS:
            rows = lane[(lane % den) < num]
            batch = torch.zeros((N, S), dtype=torch.uint8, device="cuda")
            batch[:, :ML] = wire
            for r0 in range(0, rows.numel(), 1 << 14):                   # in pieces: the gather's temporaries stay small
                r = rows[r0:r0 + (1 << 14)]
                resp = wire.index_select(0, r).index_select(1, idx)
                resp[:, cmask] = cval[cmask]
                batch[r, :len(cols)] = resp
                if len(cols) < S:
                    batch[r, len(cols):] = 0
            measure(name, num, den, batch, True)
            if (num, den) == (1, 1) and has_reader:                      # the reader kernels per chunk beside the range kernel, and the counters
                eng.wire_stats(reset=True)
                lib.act_prof_enable(ctx, 1); lib.act_prof_reset(ctx)
                run("verify", "hbm", batch.data_ptr(), True)
                per = {}
                for i in range(lib.act_prof_kernel_count(ctx)):
                    nm = lib.act_prof_kernel_name(ctx, i).decode()
                    if nm in ("k_cbor_read_raw", "k_cbor_read_raw(validate)", "k_spend_bits"):
                        ms = C.c_double(0); la = C.c_uint64(0); ln = C.c_uint64(0)
                        lib.act_prof_get(ctx, i, C.byref(ms), C.byref(la), C.byref(ln))
                        per[nm] = {"ms_total": ms.value, "launches": int(la.value), "ms_per_chunk": ms.value / max(1, int(la.value)), "messages": int(ln.value)}
                lib.act_prof_enable(ctx, 0)
                kernels[name] = {"kernels": per, "wire_stats": eng.wire_stats(reset=True)}
            del batch
    res = {"root": root, "has_reader": has_reader, "lanes": N, "cells": cells, "kernels": kernels, "stride": S, "canonical_bytes": ML,
           "device": torch.cuda.get_device_name(0)}
    eng.close()
    print("CHILD " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a checkout of the parent commit with its library built")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "wire_reader_probe.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--log2", type=int, default=18)
    ap.add_argument("--no-host", action="store_true", help="leave the host-memory cells out")
    ap.add_argument("--child-timeout", type=int, default=900)
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
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("CHILD ")]
            if r.returncode != 0 or not line:                           # nothing more is started on the device behind a failed child
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit("the %s child failed (exit %d)" % (name, r.returncode))
            runs[name].append(json.loads(line[0][6:]))
            print("rep %d %s: %s" % (rep, name, ["%.3f" % c["seconds"] for c in runs[name][-1]["cells"]]), flush=True)
    assert not runs["parent"][0]["has_reader"] and runs["this"][0]["has_reader"]
    n = runs["this"][0]["lanes"]
    rows, own_f0 = [], {}
    for k, cell in enumerate(runs["this"][0]["cells"]):
        new = [r["cells"][k]["seconds"] for r in runs["this"]]; base = [r["cells"][k]["seconds"] for r in runs["parent"]]
        mn, mb = statistics.median(new), statistics.median(base)
        if cell["spelling"] is None:
            own_f0[(cell["call"], cell["mem"])] = mn
        row = {"call": cell["call"], "mem": cell["mem"], "spelling": cell["spelling"], "f": cell["f"], "messages": n, "this_per_s": n / mn, "parent_per_s": n / mb,
               "parent_over_this": mb / mn, "this_rate_over_own_f0": own_f0[(cell["call"], cell["mem"])] / mn, "this_s": new, "parent_s": base,
               "this_spread": (max(new) - min(new)) / mn, "parent_spread": (max(base) - min(base)) / mb}
        rows.append(row)
        print(json.dumps({k2: row[k2] for k2 in ("call", "mem", "spelling", "f", "this_per_s", "parent_per_s", "parent_over_this", "this_rate_over_own_f0", "parent_spread")}), flush=True)
    res = {"tool": "tools/wire_reader_probe.py", "device": runs["this"][0]["device"], "L": 128, "messages": n, "reps": a.reps, "transcripts": "device",
           "stride": runs["this"][0]["stride"], "canonical_bytes": runs["this"][0]["canonical_bytes"],
           "baseline": "the parent commit's build: host reader behind the pipeline, second verification", "rows": rows,
           "reader_kernels_f1_hbm": [r["kernels"] for r in runs["this"]]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
