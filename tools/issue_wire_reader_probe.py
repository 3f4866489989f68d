"""The issuance wire reader: what a batch of respelled IssuanceRequest messages costs, read on the GPU in the pipeline (this tree) and
on the old road (the PARENT commit's build: flagged messages settled on the calling thread behind the pipeline -- per message a
blocking copy of its bytes, and for a device-memory caller two more for its amount and its rng slice).  A/B on one box
(tools/README.md), the shape of tools/wire_reader_probe.py.

The parent tree (a checkout of the parent commit with its library built: `git worktree add DIR HEAD~; make -C
DIR/anonymous-credit-tokens_amd/csrc`) and this tree are measured by child processes, alternating, `--reps` times each.  Per child, on
one MI355X: 2^log2 distinct valid requests made on the device, device transcripts.  A batch with share f of respelled messages carries
one of three spellings in the lanes i with i % den < num:
    indefinite   an indefinite-length map
    reordered    the four entries in reversed key order
    chunked      K as a chunked byte string of two 16-byte chunks
Messages lie at one stride (the longest spelling; a canonical message is followed by padding, which from_cbor does not read), f = 0
is the canonical batch back to back without offsets.  Cells: act_issue_cbor_batch with ACT_RNG_PER_LANE and with ACT_RNG_SEQUENTIAL,
the batch in HBM and in host memory, f in {0, 1/64, 1/2, 1} per spelling.  One warm-up call per (mode, memory) at f = 0, then one
timed call per cell.  The respelled cells may use fewer messages than the f = 0 cells (--log2-respelled: the parent's road takes
three blocking copies per message, which at 2^20 messages is minutes per cell); every row names its own count.
Reported per cell: every repetition's seconds, median messages/s of both builds, parent / this, this build's rate against its own
f = 0 rate, both builds' run-to-run spread (max - min over median).  This tree also reports, at f = 0 and per spelling at f = 1 from
HBM, the time per chunk of the flag and reader kernels beside k_issue_a_wire (from the engine's launch events: act_prof_get), and
act_ctx_wire_stats.  No pass mark: the figures go into DESIGN 4.4.

    python tools/issue_wire_reader_probe.py --parent DIR [--out profiles/issue_wire_reader_probe.json] [--reps 3] [--log2 20] [--log2-respelled K] [--no-host]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRACTIONS = ((1, 64), (1, 2), (1, 1))
SPELLINGS = ("indefinite", "reordered", "chunked")
ML = 141                                                  # the canonical IssuanceRequest: a4, then four times  key | 58 20 | 32 bytes
KERNELS = ("k_issue_wire_flag", "k_cbor_read_raw", "k_cbor_read_raw(validate)", "k_issue_a_wire")


def spellings():
    """per spelling: (source column of every output byte or -1, constant byte where the source is -1) over the canonical message"""
    ents = [(1 + 35 * k, 2 + 35 * k, 36 + 35 * k) for k in range(4)]      # key column, value columns [v0, v1)
    src = lambda a, b: [(c, 0) for c in range(a, b)]
    const = lambda *vs: [(-1, v) for v in vs]
    out = {"indefinite": const(0xBF) + src(1, ML) + const(0xFF)}
    rev = src(0, 1)
    for k, v0, v1 in ents[::-1]:
        rev += src(k, v1)
    out["reordered"] = rev
    k, v0, v1 = ents[0]
    out["chunked"] = src(0, 2) + const(0x5F, 0x50) + src(v0 + 2, v0 + 18) + const(0x50) + src(v0 + 18, v1) + const(0xFF) + src(v1, ML)
    return out


def child(root, log2, log2r, with_host):
    sys.path.insert(0, root)
    os.chdir(root)
    import numpy as np
    import torch
    import act_amd  # noqa: F401
    from act_amd import capi
    N, NR = 1 << log2, 1 << log2r
    has_reader = "k_issue_wire_flag" in open(os.path.join(root, "anonymous-credit-tokens_amd", "csrc", "engine.hip")).read()
    h = capi.params_new("bench-org", "bench-service", "bench-env", "2024-01-01", device=0)
    eng = capi.Engine(h, 8, device=0, transcript=capi.TRANSCRIPT_DEVICE)      # (issuance does not depend on L)
    lib, ctx = eng.lib, eng.ctx
    g = torch.Generator(device="cuda"); g.manual_seed(89)
    rnd = lambda n: torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)
    sk = eng.private_key_random(bytes(rnd(64).cpu().numpy()))
    pre = torch.empty(N * 64, dtype=torch.uint8, device="cuda"); req = torch.empty(N * 128, dtype=torch.uint8, device="cuda")
    r0, r1 = rnd(N * 128), rnd(N * 128)
    torch.cuda.synchronize()
    eng.pre_issuance_random_dev(N, r0.data_ptr(), pre.data_ptr())
    eng.request_dev(N, pre.data_ptr(), r1.data_ptr(), req.data_ptr())
    assert eng.cbor_size("IssuanceRequest") == ML
    RB = eng.cbor_size("IssuanceResponse")
    wire = torch.empty((N, ML), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eng._ck(lib.act_cbor_encode_batch(ctx, capi.CBOR_TYPES["IssuanceRequest"], N, capi.MEM_DEVICE, req.data_ptr(), wire.data_ptr()))
    del pre, req, r0, r1
    maps = spellings()
    S = max(len(v) for v in maps.values())
    offs = (np.arange(N + 1, dtype=np.uint64) * np.uint64(S))
    rng = rnd(N * 128); cam = torch.zeros(N * 32, dtype=torch.uint8, device="cuda"); cam[::32] = 7
    out = torch.empty(N * RB, dtype=torch.uint8, device="cuda"); st = torch.empty(N, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    h_rng = rng.cpu().numpy(); h_cam = cam.cpu().numpy(); h_out = np.empty(N * RB, np.uint8); h_st = np.empty(N, np.uint8)
    key = np.frombuffer(sk, np.uint8)
    MODES = (("per_lane", capi.RNG_PER_LANE), ("sequential", capi.RNG_SEQUENTIAL))

    def run(mode, mem, ptr, n, with_offsets):
        dev = mem == "hbm"
        t = time.perf_counter()
        rc = lib.act_issue_cbor_batch(ctx, n, capi.MEM_DEVICE if dev else capi.MEM_HOST, key.ctypes.data, ptr, offs.ctypes.data if with_offsets else None,
                                      cam.data_ptr() if dev else h_cam.ctypes.data, rng.data_ptr() if dev else h_rng.ctypes.data, mode,
                                      out.data_ptr() if dev else h_out.ctypes.data, st.data_ptr() if dev else h_st.ctypes.data)
        dt = time.perf_counter() - t
        if rc:
            raise RuntimeError("rc %d %s" % (rc, lib.act_last_error(ctx).decode()))
        accepted = int((st[:n] == 0).sum().item()) if dev else int((h_st[:n] == 0).sum())
        assert accepted == n, (mode, mem, accepted)                      # every message is a valid request, whatever its spelling
        return dt

    mems = ("hbm", "host") if with_host else ("hbm",)
    cells = []

    def measure(spelling, num, den, batch, n, with_offsets):
        torch.cuda.synchronize()
        for mem in mems:
            host = batch.cpu().numpy() if mem == "host" else None
            ptr = batch.data_ptr() if mem == "hbm" else host.ctypes.data
            for name, mode in MODES:
                if spelling is None:
                    run(mode, mem, ptr, n, with_offsets)                # warm-up: side buffers, staging, code objects
                cells.append({"mode": name, "mem": mem, "spelling": spelling, "f": num / den, "messages": n, "seconds": run(mode, mem, ptr, n, with_offsets)})
            del host

    def profile(batch, n, with_offsets):
        eng.wire_stats(reset=True)
        lib.act_prof_enable(ctx, 1); lib.act_prof_reset(ctx)
        run(capi.RNG_PER_LANE, "hbm", batch.data_ptr(), n, with_offsets)
        per = {}
        for i in range(lib.act_prof_kernel_count(ctx)):
            nm = lib.act_prof_kernel_name(ctx, i).decode()
            if nm in KERNELS:
                ms = C.c_double(0); la = C.c_uint64(0); ln = C.c_uint64(0)
                lib.act_prof_get(ctx, i, C.byref(ms), C.byref(la), C.byref(ln))
                if la.value:
                    per[nm] = {"ms_total": ms.value, "launches": int(la.value), "ms_per_chunk": ms.value / int(la.value), "messages": int(ln.value)}
        lib.act_prof_enable(ctx, 0)
        return {"kernels": per, "wire_stats": eng.wire_stats(reset=True)}

    measure(None, 0, 1, wire, N, False)
    kernels = {"canonical": profile(wire, N, False)}
    lane = torch.arange(NR, device="cuda")
    for name in SPELLINGS:
        cols = maps[name]
        idx = torch.tensor([max(c, 0) for c, _ in cols], dtype=torch.int64, device="cuda")
        cmask = torch.tensor([c < 0 for c, _ in cols], dtype=torch.bool, device="cuda")
        cval = torch.tensor([v for _, v in cols], dtype=torch.uint8, device="cuda")
        for num, den in FRACTIONS:
            rows = lane[(lane % den) < num]
            batch = torch.zeros((NR, S), dtype=torch.uint8, device="cuda")
            batch[:, :ML] = wire[:NR]
            for q0 in range(0, rows.numel(), 1 << 16):                   # in pieces: the gather's temporaries stay small
                q = rows[q0:q0 + (1 << 16)]
                resp = wire.index_select(0, q).index_select(1, idx)
                resp[:, cmask] = cval[cmask]
                batch[q, :len(cols)] = resp
                if len(cols) < S:
                    batch[q, len(cols):] = 0
            measure(name, num, den, batch, NR, True)
            if (num, den) == (1, 1):
                kernels[name] = profile(batch, NR, True)
            del batch
    res = {"root": root, "has_reader": has_reader, "cells": cells, "kernels": kernels, "stride": S, "canonical_bytes": ML, "max_batch": int(eng.max_batch) if hasattr(eng, "max_batch") else None,
           "device": torch.cuda.get_device_name(0)}
    eng.close()
    print("CHILD " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a checkout of the parent commit with its library built")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "issue_wire_reader_probe.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--log2", type=int, default=20)
    ap.add_argument("--log2-respelled", type=int, default=None, help="messages of the respelled cells (default: --log2)")
    ap.add_argument("--no-host", action="store_true", help="leave the host-memory cells out")
    ap.add_argument("--child-timeout", type=int, default=900)
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    log2r = a.log2 if a.log2_respelled is None else min(a.log2, a.log2_respelled)
    if a.child:
        return child(os.path.abspath(a.child), a.log2, log2r, not a.no_host)
    if not a.parent:
        ap.error("--parent DIR is required")
    runs = {"parent": [], "this": []}
    for rep in range(a.reps):
        for name, root in (("parent", os.path.abspath(a.parent)), ("this", HERE)):      # alternating: drift of the box hits both alike
            cmd = [sys.executable, os.path.abspath(__file__), "--child", root, "--log2", str(a.log2), "--log2-respelled", str(log2r)] + (["--no-host"] if a.no_host else [])
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("CHILD ")]
            if r.returncode != 0 or not line:                           # nothing more is started on the device behind a failed child
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit("the %s child failed (exit %d)" % (name, r.returncode))
            runs[name].append(json.loads(line[0][6:]))
            print("rep %d %s: %s" % (rep, name, ["%.4f" % c["seconds"] for c in runs[name][-1]["cells"]]), flush=True)
    assert not runs["parent"][0]["has_reader"] and runs["this"][0]["has_reader"]
    rows, own_f0 = [], {}
    for k, cell in enumerate(runs["this"][0]["cells"]):
        new = [r["cells"][k]["seconds"] for r in runs["this"]]; base = [r["cells"][k]["seconds"] for r in runs["parent"]]
        mn, mb, n = statistics.median(new), statistics.median(base), cell["messages"]
        if cell["spelling"] is None:
            own_f0[(cell["mode"], cell["mem"])] = n / mn
        row = {"mode": cell["mode"], "mem": cell["mem"], "spelling": cell["spelling"], "f": cell["f"], "messages": n, "this_per_s": n / mn, "parent_per_s": n / mb,
               "parent_over_this": mb / mn, "this_rate_over_own_f0": (n / mn) / own_f0[(cell["mode"], cell["mem"])], "this_s": new, "parent_s": base,
               "this_spread": (max(new) - min(new)) / mn, "parent_spread": (max(base) - min(base)) / mb}
        rows.append(row)
        print(json.dumps({k2: row[k2] for k2 in ("mode", "mem", "spelling", "f", "messages", "this_per_s", "parent_per_s", "parent_over_this", "this_spread", "parent_spread")}), flush=True)
    res = {"tool": "tools/issue_wire_reader_probe.py", "device": runs["this"][0]["device"], "reps": a.reps, "transcripts": "device",
           "messages_f0": 1 << a.log2, "messages_respelled": 1 << log2r, "stride": runs["this"][0]["stride"], "canonical_bytes": ML,
           "step_a": "a separate flag kernel (k_issue_wire_flag) in front of the two reader kernels; k_issue_a_wire_read takes lanes by flag and code",
           "baseline": "the parent commit's build: flagged messages settled by the host reader behind the pipeline", "rows": rows,
           "kernels_per_chunk_hbm": [r["kernels"] for r in runs["this"]]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
