"""Issuance on wire bytes against its alternatives, in one process, alternating (tools/README.md).

Messages per second at 1, 64, 4 096, 65 536 and 2^20 messages, host and device memory, for three paths over the same canonical
IssuanceRequest messages and ACT_RNG_PER_LANE bytes:
    wire      act_issue_cbor_batch                                                       (one call)
    compose   act_cbor_decode_batch(IssuanceRequest) -> act_issue_batch -> act_cbor_encode_batch(IssuanceResponse)
    records   act_issue_batch on the records the first two start from                    (the engine's figure; no CBOR)
Each repetition runs the three paths one after the other; the table shows the median rate.  Device transcripts, L = 128, the context's
default max_batch (65 536).  Writes profiles/issue_wire_probe.txt (or the path given as the first argument).

    python tools/issue_wire_probe.py [out.txt]
"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import act_amd  # noqa: E402
from act_amd import capi  # noqa: E402

SIZES = (1, 64, 4096, 65536, 1 << 20)


def reps_for(n):
    return 40 if n <= 64 else 12 if n <= 4096 else 6 if n <= 65536 else 3


def main():
    import hashlib
    import torch
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "issue_wire_probe.txt")
    sh = lambda tag, n: hashlib.shake_256(tag.encode()).digest(n)
    h = capi.params_new("bench-org", "bench-service", "bench-env", "2024-01-01", device=0)
    eng = capi.Engine(h, 128, device=0, transcript=capi.TRANSCRIPT_DEVICE)
    lib, ctx = eng.lib, eng.ctx
    sk = np.frombuffer(eng.private_key_random(sh("iwp-sk", 64)), np.uint8)
    nmax = max(SIZES)
    req = eng.request(eng.pre_issuance_random(sh("iwp-pre", 128 * nmax)), sh("iwp-rq", 128 * nmax))
    rq = np.frombuffer(req, np.uint8)
    ml, rl = eng.cbor_size("IssuanceRequest"), eng.cbor_size("IssuanceResponse")
    # the canonical messages (framed by the codec itself), amounts, per-lane rng
    wire = np.zeros(ml * nmax, np.uint8)
    assert lib.act_cbor_encode_batch(ctx, 1, nmax, capi.MEM_HOST, rq.ctypes.data, wire.ctypes.data) == 0
    camt = np.frombuffer(b"".join((i + 1).to_bytes(32, "little") for i in range(nmax)), np.uint8)
    rng = np.frombuffer(sh("iwp-rng", 128 * nmax), np.uint8)
    H = dict(wire=wire, req=rq, c=camt, rng=rng, out=np.zeros(rl * nmax, np.uint8), rec=np.zeros(128 * nmax, np.uint8),
             resp=np.zeros(160 * nmax, np.uint8), st=np.zeros(nmax, np.uint8), st2=np.zeros(nmax, np.uint8))
    D = {k: torch.from_numpy(v.copy()).cuda() for k, v in H.items()}
    torch.cuda.synchronize()
    P = {"host": {k: v.ctypes.data for k, v in H.items()}, "device": {k: v.data_ptr() for k, v in D.items()}}
    MEM = {"host": capi.MEM_HOST, "device": capi.MEM_DEVICE}

    def ck(rc, what):
        if rc:
            raise RuntimeError("%s: %s %s" % (what, capi._ERRS.get(rc, rc), lib.act_last_error(ctx).decode()))

    def run(path, mk, n):
        p, mem = P[mk], MEM[mk]
        if path == "wire":
            ck(lib.act_issue_cbor_batch(ctx, n, mem, sk.ctypes.data, p["wire"], None, p["c"], p["rng"], capi.RNG_PER_LANE, p["out"], p["st"]), path)
        elif path == "compose":
            ck(lib.act_cbor_decode_batch(ctx, 1, n, mem, p["wire"], None, p["rec"], p["st2"]), "decode")
            ck(lib.act_issue_batch(ctx, n, mem, sk.ctypes.data, p["rec"], p["c"], p["rng"], capi.RNG_PER_LANE, p["resp"], p["st"]), "issue")
            ck(lib.act_cbor_encode_batch(ctx, 2, n, mem, p["resp"], p["out"]), "encode")
        else:
            ck(lib.act_issue_batch(ctx, n, mem, sk.ctypes.data, p["req"], p["c"], p["rng"], capi.RNG_PER_LANE, p["resp"], p["st"]), path)

    paths = ("wire", "compose", "records")
    rows = []
    for n in SIZES:
        for mk in ("host", "device"):
            for path in paths:                                       # warm-up: staging buffers, code objects
                run(path, mk, n)
            t = {path: [] for path in paths}
            for _ in range(reps_for(n)):
                for path in paths:                                   # alternating: drift of the box hits all three alike
                    t0 = time.perf_counter(); run(path, mk, n); t[path].append(time.perf_counter() - t0)
            if mk == "device":
                torch.cuda.synchronize()
            st = (D["st"][:n].cpu().numpy() if mk == "device" else H["st"][:n])
            assert not st.any(), "a canonical request was rejected"
            med = {path: n / statistics.median(t[path]) for path in paths}
            rows.append((n, mk, med))
            print("%8d %-6s " % (n, mk) + "  ".join("%s %12.0f/s" % (pth, med[pth]) for pth in paths), flush=True)
    # the wire call's output = the composition's output
    run("wire", "host", 4096); a = H["out"][:rl * 4096].copy(); run("compose", "host", 4096)
    assert (a == H["out"][:rl * 4096]).all()
    lines = ["# tools/issue_wire_probe.py: IssuanceRequest CBOR in -> IssuanceResponse CBOR out, messages/s (median of alternating repetitions)",
             "# wire = act_issue_cbor_batch; compose = act_cbor_decode_batch -> act_issue_batch -> act_cbor_encode_batch; records = act_issue_batch",
             "# L = 128, device transcripts, max_batch 65536, ACT_RNG_PER_LANE, canonical messages; wire == compose byte for byte (checked at 4096)",
             "%10s %-6s %14s %14s %14s %10s %10s" % ("messages", "memory", "wire", "compose", "records", "wire/rec", "wire/comp")]
    for n, mk, med in rows:
        lines.append("%10d %-6s %14.0f %14.0f %14.0f %10.3f %10.3f" % (n, mk, med["wire"], med["compose"], med["records"],
                                                                      med["wire"] / med["records"], med["wire"] / med["compose"]))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    eng.close()


if __name__ == "__main__":
    main()
