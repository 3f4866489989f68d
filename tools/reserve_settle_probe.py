"""Reserve and settle: what the two calls cost against the parent commit's calls, in one process, alternating (tools/README.md; the shape
of tools/return_replay_probe.py).

One MI355X, L = 128, 2^18 distinct proofs resident in HBM (and one smaller size from host memory, --host-log2), records and wire
(canonical messages of one size), device transcripts, the context's default max_batch, ring of one key with an epoch, charge == NULL,
fresh sets of 4 n slots per timed group.  Per repetition, memory kind and form, one after the other:
    (base)          act_redeem_(cbor_)admit_replay_batch of the BASELINE library -- --baseline-tree names a checkout of the commit to
                    compare against, with its library built; its binding is loaded beside this one under another module name and gets
                    a context of its own.  Without the option the baseline is this tree's own call (and the result says so).
    (reserve)       act_redeem_(cbor_)reserve_batch on empty sets: the honest batch
    (*_retry)       the same batch again on the same sets: every lane a retry
    (*_foreign)     the same batch on sets whose nullifier set holds every k and whose receipts hold nothing: every lane shed by the screen
    (compose)       records only: the baseline's act_replay_derive_return_batch + act_refund_sign_return_keyring_batch over the lanes of
                    the reservation records (t = s on every lane)
    (settle)        act_redeem_settle_batch over the same records and amounts: the three receipts steps on top of what (compose) does
    (settle_again)  the same call again: every lane settled before
Reserve does strictly less than the baseline's call, so each of its three figures is judged as the other probes judge theirs: the ratio
median(reserve) / median(base), the baseline's own run-to-run spread (max - min over median), and whether the ratio lies inside
1 + spread + 1 %.  For settle the ratio to (compose) is REPORTED; no threshold is fixed in advance.  Every retry is checked byte for byte
against its first call.  Nothing is asserted about rates.  Writes profiles/reserve_settle_probe.json (or --out).

    python tools/reserve_settle_probe.py [--baseline-tree DIR] [--out f] [--log2 18] [--host-log2 14] [--reps 5]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import act_amd  # noqa: E402,F401
from act_amd import capi  # noqa: E402
import bench  # noqa: E402
from return_replay_probe import load_tree  # noqa: E402


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reserve_settle_probe.json"))
    ap.add_argument("--baseline-tree", default=None)
    ap.add_argument("--log2", type=int, default=18)
    ap.add_argument("--host-log2", type=int, default=14)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    NMAX, L, REPS = 1 << a.log2, 128, a.reps
    sh = lambda tag, n: hashlib.shake_256(tag.encode()).digest(n)
    h = capi.params_new("bench-org", "bench-service", "bench-env", "2024-01-01", device=0)
    eng = capi.Engine(h, L, device=0, transcript=capi.TRANSCRIPT_DEVICE)
    sk = eng.private_key_random(sh("rsp-sk", 64))
    bcapi = load_tree(a.baseline_tree, "act_baseline") if a.baseline_tree else capi
    beng = bcapi.Engine(h, L, device=0, transcript=bcapi.TRANSCRIPT_DEVICE) if a.baseline_tree else eng
    t0 = time.perf_counter()
    proofs = bench.make_distinct_proofs_on_device(eng, capi, torch, np, sk, NMAX, L, seed=79)[0]
    print("made %d proofs in %.1f s" % (NMAX, time.perf_counter() - t0), flush=True)
    PB, ML = eng.proof_bytes, eng.cbor_size("SpendProof")
    view = proofs.view(NMAX, PB)
    wire = torch.empty((NMAX, ML), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eng._ck(eng.lib.act_cbor_encode_batch(eng.ctx, capi.CBOR_TYPES["SpendProof"], NMAX, capi.MEM_DEVICE, view.data_ptr(), wire.data_ptr()))
    OB = {"records": 128, "wire": eng.cbor_size("Refund")}
    key = np.frombuffer(sk, np.uint8); ep = np.array([1], np.uint32); nonce_key = np.frombuffer(sh("rsp-nonce-key", 32), np.uint8)
    rcnt = (C.c_uint64 * len(capi.RESERVE_COUNTS))(); scnt = (C.c_uint64 * len(capi.SETTLE_COUNTS))()

    def measure(mem_name, N):
        dev = mem_name == "device"
        mem = capi.MEM_DEVICE if dev else capi.MEM_HOST

        class Buf:      # n bytes in the caller's kind of memory, with its address
            def __init__(self, n, src=None):
                if dev:
                    self.t = torch.empty(max(1, n), dtype=torch.uint8, device="cuda") if src is None else src
                    self.p = self.t.data_ptr()
                else:
                    self.t = np.empty(max(1, n), np.uint8) if src is None else np.ascontiguousarray(src.cpu().numpy())
                    self.p = self.t.ctypes.data

            def bytes(self, n):
                return self.t[:n].cpu().numpy().tobytes() if dev else self.t[:n].tobytes()

        src = {"records": Buf(0, view[:N].contiguous().view(-1)), "wire": Buf(0, wire[:N].contiguous().view(-1))}
        nul = view[:N, :32].contiguous().cpu().numpy().tobytes()
        amounts = Buf(0, view[:N, 32:64].contiguous().view(-1))      # t = s: the largest amount the bound lets through
        out, st, ok, rp = Buf(N * max(160, OB["wire"])), Buf(N), Buf(N), Buf(N)
        tags, non, zero_st, kp = Buf(N * 32), Buf(N * 128), Buf(N), Buf(N * 32)
        if dev:
            zero_st.t.zero_(); torch.cuda.synchronize()
        else:
            zero_st.t[:] = 0

        def redeem(form, what, s, r):
            """one call of (base) or (reserve) on the sets given -> seconds"""
            base = what == "base"
            cp, e = (bcapi, beng) if base else (capi, eng)
            head = [e.ctx, s.h, r.h, N, mem, key.ctypes.data, 1, ep.ctypes.data] + ([cp.SIGN_MATCHED] if base else []) + [src[form].p] + ([None] if form == "wire" else []) + [None]
            if base:
                fn = e.lib.act_redeem_cbor_admit_replay_batch if form == "wire" else e.lib.act_redeem_admit_replay_batch
                args = head + [nonce_key.ctypes.data, out.p, st.p, ok.p, rp.p, rcnt]
            else:
                fn = e.lib.act_redeem_cbor_reserve_batch if form == "wire" else e.lib.act_redeem_reserve_batch
                args = head + [out.p, st.p, ok.p, rp.p, rcnt]
            t = time.perf_counter()
            rc = fn(*args)
            dt = time.perf_counter() - t
            if rc:
                raise RuntimeError("%s %s: rc %d %s" % (form, what, rc, e.lib.act_last_error(e.ctx).decode()))
            return dt

        def group(form, what):
            """honest, retry and foreign batch of one call -> three times; the sets are built and dropped here"""
            cp = bcapi if what == "base" else capi
            nb = N * (OB[form] if what == "base" else 96)
            s, r = cp.NullifierSet(4 * N), cp.NullifierSet(4 * N)
            first = redeem(form, what, s, r)
            assert int(rcnt[7]) == N and (len(s), len(r)) == (N, N), (form, what, list(rcnt))      # every lane fresh
            keep = out.bytes(nb)
            again = redeem(form, what, s, r)
            assert int(rcnt[8]) == N and out.bytes(nb) == keep, "a retried batch did not get its answers again"
            s.close(); r.close()
            s, r = cp.NullifierSet(4 * N), cp.NullifierSet(4 * N)
            assert s.check_and_insert(nul) == bytes(N)
            foreign = redeem(form, what, s, r)
            assert int(rcnt[3]) == N and int(rcnt[5]) == 0 and len(r) == 0, (form, what, list(rcnt))      # every lane shed unverified
            s.close(); r.close()
            return first, again, foreign

        def settle_group():
            """compose (baseline), settle and settle again over the same reservation records -> three times"""
            s, r = capi.NullifierSet(4 * N), capi.NullifierSet(8 * N)
            redeem("records", "reserve", s, r)
            recs = Buf(N * 96)
            if dev:
                recs.t.copy_(out.t[:N * 96]); kp.t.view(N, 32).copy_(recs.t.view(N, 96)[:, 32:64]); torch.cuda.synchronize()
            else:
                recs.t[:] = out.t[:N * 96]; kp.t.reshape(N, 32)[:] = recs.t.reshape(N, 96)[:, 32:64]
            kidx = Buf(N)
            if dev:
                kidx.t.copy_(ok.t[:N]); torch.cuda.synchronize()
            else:
                kidx.t[:] = ok.t[:N]
            t = time.perf_counter()
            rc = beng.lib.act_replay_derive_return_batch(beng.ctx, N, mem, key.ctypes.data, 1, kidx.p, nonce_key.ctypes.data, recs.p, 96, kp.p, zero_st.p, amounts.p, tags.p, non.p)
            rc = rc or beng.lib.act_refund_sign_return_keyring_batch(beng.ctx, N, mem, key.ctypes.data, 1, kidx.p, kp.p, zero_st.p, non.p, bcapi.RNG_PER_LANE, amounts.p, out.p, st.p)
            compose = time.perf_counter() - t
            if rc:
                raise RuntimeError("compose: rc %d %s" % (rc, beng.lib.act_last_error(beng.ctx).decode()))
            want = out.bytes(N * 160)
            (non.t.zero_(), torch.cuda.synchronize()) if dev else non.t.fill(0)
            dts = []
            for turn in range(2):
                t = time.perf_counter()
                rc = eng.lib.act_redeem_settle_batch(eng.ctx, r.h, N, mem, key.ctypes.data, 1, ep.ctypes.data, capi.SIGN_MATCHED, recs.p, kidx.p, amounts.p, nonce_key.ctypes.data,
                                                     out.p, st.p, rp.p, scnt)
                dts.append(time.perf_counter() - t)
                if rc:
                    raise RuntimeError("settle: rc %d %s" % (rc, eng.lib.act_last_error(eng.ctx).decode()))
                assert int(scnt[3 + turn]) == N and out.bytes(N * 160) == want, (turn, list(scnt))      # settled, then settled again; the composition's bytes
            s.close(); r.close()
            return compose, dts[0], dts[1]

        forms, kinds = ("records", "wire"), ("base", "reserve")
        for form in forms:                                              # warm-up: side buffers, staging, code objects
            for what in kinds:
                group(form, what)
        settle_group()
        names = ("", "_retry", "_foreign")
        t = {form: {k + x: [] for k in kinds for x in names} for form in forms}
        ts = {"compose": [], "settle": [], "settle_again": []}
        for _ in range(REPS):
            for form in forms:
                for what in kinds:                                      # alternating: drift of the box hits all alike
                    for x, v in zip(names, group(form, what)):
                        t[form][what + x].append(v)
            for k, v in zip(("compose", "settle", "settle_again"), settle_group()):
                ts[k].append(v)
        res = {"lanes": N, "forms": {}}
        for form in forms:
            med = {k: statistics.median(v) for k, v in t[form].items()}
            spread = {x: (max(t[form]["base" + x]) - min(t[form]["base" + x])) / med["base" + x] for x in names}
            row = {"seconds": t[form], "median_s": med, "lanes_per_s": {k: N / v for k, v in med.items()}, "baseline_spread": {"base" + x: spread[x] for x in names},
                   "band": {"reserve" + x: 1.0 + spread[x] + 0.01 for x in names},
                   "ratio_to_base": {"reserve" + x: med["reserve" + x] / med["base" + x] for x in names},
                   "inside_band": {"reserve" + x: med["reserve" + x] / med["base" + x] <= 1.0 + spread[x] + 0.01 for x in names}}
            res["forms"][form] = row
            print(json.dumps({"memory": mem_name, "form": form, **{k: row[k] for k in ("median_s", "baseline_spread", "band", "ratio_to_base", "inside_band")}}), flush=True)
        med = {k: statistics.median(v) for k, v in ts.items()}
        spread = (max(ts["compose"]) - min(ts["compose"])) / med["compose"]
        res["settle"] = {"seconds": ts, "median_s": med, "lanes_per_s": {k: N / v for k, v in med.items()}, "compose_spread": spread, "band": 1.0 + spread + 0.01,
                         "ratio_to_compose": {k: med[k] / med["compose"] for k in ("settle", "settle_again")},
                         "inside_band": {k: med[k] / med["compose"] <= 1.0 + spread + 0.01 for k in ("settle", "settle_again")}}
        print(json.dumps({"memory": mem_name, "settle": {k: res["settle"][k] for k in ("median_s", "compose_spread", "ratio_to_compose", "inside_band")}}), flush=True)
        return res

    res = {"tool": "tools/reserve_settle_probe.py", "device": torch.cuda.get_device_name(0), "L": L, "reps": REPS, "transcripts": "device",
           "baseline": "the calls of " + ("the library under --baseline-tree" if a.baseline_tree else "THIS library (no --baseline-tree given)"),
           "device_memory": measure("device", NMAX), "host_memory": measure("host", min(NMAX, 1 << a.host_log2))}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    eng.close()
    if beng is not eng:
        beng.close()


if __name__ == "__main__":
    main()
