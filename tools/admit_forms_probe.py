"""The admission family after its engine was rewritten as a call record and stages: is a call as fast as the parent commit's?  One
process, one MI355X, the parent's library loaded beside this one, alternating (tools/README.md; the shape of tools/return_replay_probe.py).

L = 128, 2^18 lanes resident in HBM, records and wire (canonical messages of one size), device transcripts, the context's default
max_batch, a ring of one key with an epoch, charge == NULL, fresh sets of 4 n slots per timed call.  THE SAME call on both sides:
    (admit)            act_redeem_(cbor_)admit_batch on distinct proofs, per-lane rng bytes in HBM
    (admit_unique2)    act_redeem_(cbor_)admit_unique_batch, every proof twice (lane i and lane i + n / 2)
    (rru)              act_redeem_(cbor_)return_replay_unique_batch on distinct proofs, t = s on every lane
    (rru2)             ... every proof twice, the copy naming its leader's amount
and the same four from HOST memory at 2^16 lanes, reported only.  Per repetition every row runs on both libraries, one behind the other, and
which of the two goes first alternates (with one library on both sides, the second call of a pair was up to 18 % slower on the host rows with copies);
before the timed repetitions each row's statuses, out_key, replay marks, counts and output bytes are compared between the two
libraries once.  Reported: the raw times, the medians, median(this) / median(baseline), the baseline's own run-to-run spread (max - min
over median) and whether the ratio lies inside 1 + spread + 1 % (the HBM rows: the gate; host rows: reported).  Writes
profiles/admit_forms_probe.json (or --out); exit status 1 if an HBM row lies outside its band.

    python tools/admit_forms_probe.py --baseline-tree DIR [--out f] [--log2 18] [--host-log2 16] [--reps 5]

DIR: a checkout of the commit to compare against, with its library built; its binding is loaded under another module name and gets a
context of its own.  Without the option the baseline is this tree's own library (and the result says so)."""
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
from tools.return_replay_probe import load_tree  # noqa: E402

ROWS = ("admit", "admit_unique2", "rru", "rru2")


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "admit_forms_probe.json"))
    ap.add_argument("--baseline-tree", default=None)
    ap.add_argument("--log2", type=int, default=18)
    ap.add_argument("--host-log2", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    N, NH, L, REPS = 1 << a.log2, 1 << a.host_log2, 128, a.reps
    sh = lambda tag, n: hashlib.shake_256(tag.encode()).digest(n)
    h = capi.params_new("bench-org", "bench-service", "bench-env", "2024-01-01", device=0)
    eng = capi.Engine(h, L, device=0, transcript=capi.TRANSCRIPT_DEVICE)
    sk = eng.private_key_random(sh("afp-sk", 64))
    bcapi = load_tree(a.baseline_tree, "act_baseline") if a.baseline_tree else capi
    beng = bcapi.Engine(h, L, device=0, transcript=bcapi.TRANSCRIPT_DEVICE) if a.baseline_tree else eng
    t0 = time.perf_counter()
    proofs = bench.make_distinct_proofs_on_device(eng, capi, torch, np, sk, N, L, seed=79)[0]
    print("made %d proofs in %.1f s" % (N, time.perf_counter() - t0), flush=True)
    PB, ML = eng.proof_bytes, eng.cbor_size("SpendProof")
    view = proofs.view(N, PB)
    twice = torch.cat([view[:N // 2], view[:N // 2]]).contiguous()              # lane i + N / 2 has the bytes of lane i
    key = np.frombuffer(sk, np.uint8); ep = np.array([1], np.uint32); nonce_key = np.frombuffer(sh("afp-nonce-key", 32), np.uint8)

    def encode(recs):
        w = torch.empty((recs.shape[0], ML), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        eng._ck(eng.lib.act_cbor_encode_batch(eng.ctx, capi.CBOR_TYPES["SpendProof"], recs.shape[0], capi.MEM_DEVICE, recs.data_ptr(), w.data_ptr()))
        return w

    class Where:
        """the inputs and outputs of n lanes in one kind of memory"""

        def __init__(self, mem, n):
            self.mem, self.n = mem, n
            place = (lambda t: t.contiguous()) if mem == capi.MEM_DEVICE else (lambda t: t.cpu().contiguous())
            new = lambda size: torch.empty(size, dtype=torch.uint8, device="cuda" if mem == capi.MEM_DEVICE else "cpu")
            d, t = view[:n], torch.cat([view[:n // 2], view[:n // 2]]).contiguous() if n != N else twice
            self.src = {("records", False): place(d), ("records", True): place(t), ("wire", False): place(encode(d)), ("wire", True): place(encode(t))}
            self.spent = {False: place(d[:, 32:64]), True: place(t[:, 32:64])}      # s of every lane: the largest t the screen lets through
            g = torch.Generator(device="cpu"); g.manual_seed(7907)
            self.rng = place(torch.randint(0, 256, (n * 128,), dtype=torch.uint8, generator=g).cuda())
            ob = max(160, eng.cbor_size("RefundReturn"))
            self.out, self.st, self.ok, self.rp = new(n * ob), new(n), new(n), new(n)
            torch.cuda.synchronize()

    def call(cp, e, w, row, form):
        """one call on fresh sets -> (seconds, what it answered)"""
        n, double = w.n, row.endswith("2")
        s, r = cp.NullifierSet(4 * n), cp.NullifierSet(4 * n)
        head = [n, w.mem, key.ctypes.data, 1, ep.ctypes.data, cp.SIGN_MATCHED, w.src[form, double].data_ptr()] + ([None] if form == "wire" else []) + [None]
        stem = {"admit": "admit", "admit_unique2": "admit_unique", "rru": "return_replay_unique", "rru2": "return_replay_unique"}[row]
        fn = getattr(e.lib, "act_redeem_%s%s_batch" % ("cbor_" if form == "wire" else "", stem))
        if row.startswith("rru"):
            cnt = (C.c_uint64 * len(cp.RETURN_REPLAY_UNIQUE_COUNTS))()
            args = [e.ctx, s.h, r.h] + head + [w.spent[double].data_ptr(), nonce_key.ctypes.data, w.out.data_ptr(), w.st.data_ptr(), w.ok.data_ptr(), w.rp.data_ptr(), cnt]
            ob = e.cbor_size("RefundReturn") if form == "wire" else 160
        else:
            cnt = (C.c_uint64 * len(cp.ADMIT_UNIQUE_COUNTS if double else cp.ADMIT_COUNTS))()
            args = [e.ctx, s.h] + head + [w.rng.data_ptr(), cp.RNG_PER_LANE, w.out.data_ptr(), w.st.data_ptr(), w.ok.data_ptr(), cnt]
            ob = e.cbor_size("Refund") if form == "wire" else 128
            w.rp.zero_()
        t = time.perf_counter()
        rc = fn(*args)
        dt = time.perf_counter() - t
        if rc:
            raise RuntimeError("%s %s: rc %d %s" % (row, form, rc, e.lib.act_last_error(e.ctx).decode()))
        assert len(s) == (n // 2 if double else n), (row, form, len(s), list(cnt))          # every distinct proof recorded once
        digest = hashlib.sha256(w.out[:n * ob].cpu().numpy().tobytes() + w.st.cpu().numpy().tobytes() + w.ok.cpu().numpy().tobytes() + w.rp.cpu().numpy().tobytes())
        s.close(); r.close()
        return dt, (list(cnt), digest.hexdigest())

    sides = (("base", bcapi, beng), ("this", capi, eng))
    res = {"tool": "tools/admit_forms_probe.py", "device": torch.cuda.get_device_name(0), "L": L, "reps": REPS, "transcripts": "device",
           "baseline": "the library under --baseline-tree" if a.baseline_tree else "THIS library (no --baseline-tree given)", "memory": {}}
    outside = []
    for label, mem, n, reps in (("hbm", capi.MEM_DEVICE, N, REPS), ("host", capi.MEM_HOST, NH, REPS)):
        w = Where(mem, n)
        rows = {}
        for form in ("records", "wire"):
            for row in ROWS:                                        # warm-up (side buffers, staging, code objects) and the one comparison of outputs
                got = {side: call(cp, e, w, row, form)[1] for side, cp, e in sides}
                assert got["base"] == got["this"], ("the two libraries answer differently", label, form, row, got)
            t = {row: {side: [] for side, _, _ in sides} for row in ROWS}
            for rep in range(reps):
                for row in ROWS:                                    # alternating: drift of the box hits both alike; who goes first alternates too
                    for side, cp, e in (sides if rep % 2 == 0 else sides[::-1]):
                        t[row][side].append(call(cp, e, w, row, form)[0])
            for row in ROWS:
                med = {side: statistics.median(v) for side, v in t[row].items()}
                spread = (max(t[row]["base"]) - min(t[row]["base"])) / med["base"]
                ratio = med["this"] / med["base"]
                rows["%s/%s" % (form, row)] = {"seconds": t[row], "median_s": med, "lanes_per_s": {k: n / v for k, v in med.items()}, "baseline_spread": spread,
                                               "band": 1.0 + spread + 0.01, "ratio_to_base": ratio, "inside_band": ratio <= 1.0 + spread + 0.01}
                print(json.dumps({"memory": label, "row": "%s/%s" % (form, row), "median_s": med, "baseline_spread": spread, "ratio_to_base": ratio,
                                  "inside_band": ratio <= 1.0 + spread + 0.01}), flush=True)
                if label == "hbm" and ratio > 1.0 + spread + 0.01:
                    outside.append("%s/%s" % (form, row))
        res["memory"][label] = {"lanes": n, "gated": label == "hbm", "rows": rows}
    res["hbm_rows_outside_their_band"] = outside
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    eng.close()
    if beng is not eng:
        beng.close()
    return 1 if outside else 0


if __name__ == "__main__":
    sys.exit(main())
