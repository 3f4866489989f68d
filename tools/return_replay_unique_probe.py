"""Replayable partial refunds, unique forms: what the copy stage costs a batch without copies and what it spares a batch of resends,
against the parent commit's act_redeem_(cbor_)return_replay_batch, in one process, alternating (tools/README.md; the shape of
tools/return_replay_probe.py).

One MI355X, L = 128, 2^18 lanes resident in HBM, records and wire (canonical messages of one size), device transcripts, the context's
default max_batch, ring of one key with an epoch, charge == NULL, t = s on every leader, fresh sets of 4 n slots per timed call.  Four
batches of n lanes each:
    share_0          n distinct proofs                                            (THE GATE: the copy stage finds nothing)
    share_1_2        every proof sent twice, the resend names the leader's amount (n / 2 served copies)
    share_7_8        every proof sent eight times, the same                       (7 n / 8 served copies)
    share_1_2_other  every proof sent twice, the resend names t = 0, not s        (n / 2 copies answered DOUBLE_SPEND)
Per repetition, form and batch, one after the other on the SAME batch:
    (base)    act_redeem_(cbor_)return_replay_batch of the BASELINE library -- --baseline-tree names a checkout of the commit to compare
              against, with its library built; its binding is loaded beside this one under another module name and gets a context of its
              own.  Without the option the baseline is this tree's own call (and the result says so).
    (unique)  act_redeem_(cbor_)return_replay_unique_batch of this library
Both calls must give the same statuses, replay marks and output bytes (checked once per form and batch, outside the timed region).
Reported: the raw times, the medians, the ratio median(unique) / median(base) and its inverse, the baseline's own run-to-run spread
(max - min over median), and for share_0 whether the ratio lies inside 1 + spread + 1 %.  The copy shares are reported, not gated.
--host-log2 (default 16; 0 = skip): the same four batches from HOST memory at that many lanes, three repetitions, reported only.
Writes profiles/return_replay_unique_probe.json (or --out).

    python tools/return_replay_unique_probe.py [--baseline-tree DIR] [--out f] [--log2 18] [--reps 5] [--host-log2 16]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import act_amd  # noqa: E402,F401
from act_amd import capi  # noqa: E402
import bench  # noqa: E402
from return_replay_probe import load_tree  # noqa: E402

BATCHES = (("share_0", 1, False), ("share_1_2", 2, False), ("share_7_8", 8, False), ("share_1_2_other", 2, True))      # (name, times each proof is sent, resends name t = 0)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "return_replay_unique_probe.json"))
    ap.add_argument("--baseline-tree", default=None)
    ap.add_argument("--log2", type=int, default=18)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-log2", type=int, default=16)
    a = ap.parse_args()
    N, L, REPS = 1 << a.log2, 128, a.reps
    NH = min(N, 1 << a.host_log2) if a.host_log2 else 0
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
    OB = {"records": 160, "wire": eng.cbor_size("RefundReturn")}
    view = proofs.view(N, PB)
    wire = torch.empty((N, ML), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eng._ck(eng.lib.act_cbor_encode_batch(eng.ctx, capi.CBOR_TYPES["SpendProof"], N, capi.MEM_DEVICE, view.data_ptr(), wire.data_ptr()))
    rows = {"records": view, "wire": wire}
    key = np.frombuffer(sk, np.uint8); ep = np.array([1], np.uint32); nonce_key = np.frombuffer(sh("rrp-nonce-key", 32), np.uint8)
    ucnt = (C.c_uint64 * len(capi.RETURN_REPLAY_UNIQUE_COUNTS))()
    bcnt = (C.c_uint64 * len(capi.RETURN_REPLAY_COUNTS))()

    def probe(mem, n, reps, take):
        """take(form, src, other) -> (batch pointer, amounts pointer, keep-alive) in `mem` memory; the outputs are this function's"""
        dev = mem == capi.MEM_DEVICE
        if dev:
            mk = lambda size: torch.empty(size, dtype=torch.uint8, device="cuda")
            ptr = lambda x: x.data_ptr()
            same = lambda x, y: bool(torch.equal(x, y))
        else:
            mk = lambda size: np.empty(size, np.uint8)
            ptr = lambda x: x.ctypes.data
            same = lambda x, y: bool((x == y).all())
        ob_max = max(OB.values())
        outs = {w: (mk(n * ob_max), mk(n), mk(n), mk(n)) for w in ("base", "unique")}
        res = {}
        for form in ("records", "wire"):
            res[form] = {}
            for name, times, other in BATCHES:
                src = np.arange(n, dtype=np.int64) // times
                batch, amounts, alive = take(form, src, other)

                def one(what):
                    base = what == "base"
                    cp, e = (bcapi, beng) if base else (capi, eng)
                    s, r = cp.NullifierSet(4 * n), cp.NullifierSet(4 * n)
                    o, st, ok, rp = outs[what]
                    fn = ((e.lib.act_redeem_cbor_return_replay_batch if form == "wire" else e.lib.act_redeem_return_replay_batch) if base else
                          (e.lib.act_redeem_cbor_return_replay_unique_batch if form == "wire" else e.lib.act_redeem_return_replay_unique_batch))
                    args = [e.ctx, s.h, r.h, n, mem, key.ctypes.data, 1, ep.ctypes.data, cp.SIGN_MATCHED, batch] + ([None] if form == "wire" else []) + \
                           [None, amounts, nonce_key.ctypes.data, ptr(o), ptr(st), ptr(ok), ptr(rp), bcnt if base else ucnt]
                    if dev:
                        torch.cuda.synchronize()
                    t = time.perf_counter()
                    rc = fn(*args)
                    dt = time.perf_counter() - t
                    if rc:
                        raise RuntimeError("%s %s %s: rc %d %s" % (form, name, what, rc, e.lib.act_last_error(e.ctx).decode()))
                    assert (len(s), len(r)) == (n // times, n // times), (form, name, what, len(s), len(r))
                    s.close(); r.close()
                    if not base:
                        c = dict(zip(capi.RETURN_REPLAY_UNIQUE_COUNTS, (int(v) for v in ucnt)))
                        copies = n - n // times
                        assert (c["verified"], c["fresh"], c["copies"]) == (n // times, n // times, copies), (form, name, c)
                        assert (c["copies_served"], c["copies_other_amount"]) == ((0, copies) if other else (copies, 0)), (form, name, c)
                    return dt

                one("base"); one("unique")                          # warm-up: side buffers, staging, code objects -- and the equality check
                nb = n * OB[form]
                for k in range(4):
                    x, y = outs["base"][k], outs["unique"][k]
                    assert same(x[:nb] if k == 0 else x, y[:nb] if k == 0 else y), (form, name, "the two calls differ in output %d" % k)
                res[form][name] = {"base": [], "unique": []}
                print("checked %s %s at %d lanes" % (form, name, n), flush=True)
            for _ in range(reps):                                   # alternating: drift of the box hits all alike
                for name, times, other in BATCHES:
                    src = np.arange(n, dtype=np.int64) // times
                    batch, amounts, alive = take(form, src, other)
                    for what in ("base", "unique"):
                        res[form][name][what].append(one(what))
        return res

    def take_device(form, src, other):
        idx = torch.from_numpy(src).cuda()
        b = rows[form].index_select(0, idx).contiguous()
        t = view[:, 32:64].index_select(0, idx).contiguous()
        if other:
            t[1::2] = 0                                             # the resend names nothing returned
        torch.cuda.synchronize()
        return b.data_ptr(), t.data_ptr(), (b, t, idx)

    def summary(t, n, gate):
        out = {}
        for form, per in t.items():
            out[form] = {}
            for name, v in per.items():
                med = {k: statistics.median(x) for k, x in v.items()}
                spread = (max(v["base"]) - min(v["base"])) / med["base"]
                row = {"seconds": v, "median_s": med, "lanes_per_s": {k: n / x for k, x in med.items()}, "baseline_spread": spread,
                       "ratio_to_base": med["unique"] / med["base"], "times_faster": med["base"] / med["unique"]}
                if gate and name == "share_0":
                    row["band"] = 1.0 + spread + 0.01
                    row["inside_band"] = row["ratio_to_base"] <= row["band"]
                out[form][name] = row
                print(json.dumps({"lanes": n, "form": form, "batch": name, **{k: row[k] for k in row if k != "seconds"}}), flush=True)
        return out

    res = {"tool": "tools/return_replay_unique_probe.py", "device": torch.cuda.get_device_name(0), "L": L, "lanes": N, "reps": REPS, "transcripts": "device",
           "baseline": "act_redeem_(cbor_)return_replay_batch of " + ("the library under --baseline-tree" if a.baseline_tree else "THIS library (no --baseline-tree given)"),
           "gate": "share_0: ratio_to_base <= 1 + baseline_spread + 0.01; every other figure is reported, not gated"}
    res["hbm"] = summary(probe(capi.MEM_DEVICE, N, REPS, take_device), N, True)
    if NH:
        host = {"records": view[:NH].cpu().numpy(), "wire": wire[:NH].cpu().numpy()}
        amounts = np.ascontiguousarray(host["records"][:, 32:64])

        def take_host(form, src, other):
            b = np.ascontiguousarray(host[form][src])
            t = np.ascontiguousarray(amounts[src])
            if other:
                t[1::2] = 0
            return b.ctypes.data, t.ctypes.data, (b, t)

        res["host_memory"] = {"lanes": NH, "reps": 3, **summary(probe(capi.MEM_HOST, NH, 3, take_host), NH, False)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    eng.close()
    if beng is not eng:
        beng.close()


if __name__ == "__main__":
    main()
