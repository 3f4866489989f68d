"""Admission for the replayable redemption, unique forms: what the copy step costs a batch without copies and what it spares a batch of
resent proofs.  A/B against the PARENT commit's build on one box (tools/README.md; the protocols of tools/copies_probe.py and
tools/admit_replay_probe.py).

The parent tree (a checkout of the parent commit with its library built) and this tree are each measured by ONE child process that
imports the package of the tree it is given, so each build runs behind its own binding.  Both children make the same 2^log2 distinct
valid proofs on the device once (L = 128, device transcripts, a ring of one key with an epoch) and then take turns: the driver tells
the parent's child to run a cell's mixes once, then this tree's, `--reps` times -- interleaved, so drift of the box hits both alike.
Cells: records and wire (canonical messages of one size), the batch in HBM and in host memory (where the fingerprint and the compare
run on the host workers).  Mixes, each timed as ONE call on sets of 4 n slots:
    none      2^log2 distinct fresh proofs, empty sets                         -- the honest batch: the one condition below
    twice     every proof twice (lane i carries proof i mod n/2: a copy's leader lies n/2 lanes back), empty sets
    eight     every proof eight times (i mod n/8), empty sets
    flood     one fresh proof n times, empty sets
    served    the same proof n times again on the flood's sets: every lane a retry candidate
    parent     act_redeem_(cbor_)admit_replay_batch, charge == NULL           -- the baseline: verifies and signs every lane
    this tree  act_redeem_(cbor_)admit_replay_unique_batch, charge == NULL
Before anything is timed every mix is called once on sets of its own, and the two children's outputs of that call (statuses, out_key,
replay marks, every output byte) are compared by hash: the theorem of the header at 2^log2 lanes.
Reported per cell and mix: the times of every repetition, median lanes/s of both, the ratio, the baseline's own run-to-run spread
(max - min over median), this tree's counts.  The one condition: from HBM the mix without copies may cost no more than the baseline's
spread plus one per cent (`condition_met`).  For host memory the copy share at which the two forms cost the same is interpolated between
the mixes on either side of it.  This tree's child also reports act_prof_get of one more HBM call without copies.

    python tools/admit_replay_copies_probe.py --parent DIR [--out profiles/admit_replay_copies_probe.json] [--reps 5] [--log2 18] [--no-host]
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import select
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIXES = ("none", "twice", "eight", "flood", "served")
SHARE = {"none": 0.0, "twice": 0.5, "eight": 0.875}


def child(root, log2):
    sys.path.insert(0, root)
    os.chdir(root)
    import numpy as np
    import torch
    import act_amd  # noqa: F401
    from act_amd import capi
    import bench
    N, L = 1 << log2, 128
    sh = lambda tag, n: hashlib.shake_256(tag.encode()).digest(n)
    unique = "act_redeem_admit_replay_unique_batch" in capi.EXPORTS
    say = lambda d: print("CHILD " + json.dumps(d), flush=True)
    h = capi.params_new("bench-org", "bench-service", "bench-env", "2024-01-01", device=0)
    eng = capi.Engine(h, L, device=0, transcript=capi.TRANSCRIPT_DEVICE)
    lib, ctx = eng.lib, eng.ctx
    sk = eng.private_key_random(sh("arcp-sk", 64))
    t0 = time.perf_counter()
    proofs = bench.make_distinct_proofs_on_device(eng, capi, torch, np, sk, N, L, seed=73)[0]
    PB, ML, RB = eng.proof_bytes, eng.cbor_size("SpendProof"), eng.cbor_size("Refund")
    view = proofs.view(N, PB)
    lane = torch.arange(N, device="cuda")
    pick = {"none": lane, "twice": lane % (N // 2), "eight": lane % (N // 8), "flood": torch.full_like(lane, N - 1)}
    ob = max(128, RB)
    out = torch.empty(N * ob, dtype=torch.uint8, device="cuda")
    st = torch.empty(N, dtype=torch.uint8, device="cuda"); ok = torch.empty(N, dtype=torch.uint8, device="cuda"); rp = torch.empty(N, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    h_out = np.empty(N * ob, np.uint8); h_st = np.empty(N, np.uint8); h_ok = np.empty(N, np.uint8); h_rp = np.empty(N, np.uint8)
    key = np.frombuffer(sk, np.uint8); ep = np.array([1], np.uint32); nonce_key = np.frombuffer(sh("arcp-nonce-key", 32), np.uint8)
    names = capi.ADMIT_REPLAY_UNIQUE_COUNTS if unique else capi.ADMIT_REPLAY_COUNTS
    cnt = (C.c_uint64 * len(names))()
    say({"ready": True, "unique": unique, "lanes": N, "made_proofs_s": time.perf_counter() - t0, "device": torch.cuda.get_device_name(0)})

    state = {}

    def call(form, dev, src_ptr, s, r):
        mem = capi.MEM_DEVICE if dev else capi.MEM_HOST
        o, s_, k_, r_ = (out.data_ptr(), st.data_ptr(), ok.data_ptr(), rp.data_ptr()) if dev else (h_out.ctypes.data, h_st.ctypes.data, h_ok.ctypes.data, h_rp.ctypes.data)
        head = [ctx, s.h, r.h, N, mem, key.ctypes.data, 1, ep.ctypes.data, capi.SIGN_MATCHED, src_ptr] + ([None] if form == "wire" else []) + [None]      # charge == NULL
        if unique:
            fn = lib.act_redeem_cbor_admit_replay_unique_batch if form == "wire" else lib.act_redeem_admit_replay_unique_batch
        else:
            fn = lib.act_redeem_cbor_admit_replay_batch if form == "wire" else lib.act_redeem_admit_replay_batch
        t = time.perf_counter()
        rc = fn(*(head + [nonce_key.ctypes.data, o, s_, k_, r_, cnt]))
        dt = time.perf_counter() - t
        if rc:
            raise RuntimeError("%s %s: rc %d %s" % (form, "hbm" if dev else "host", rc, lib.act_last_error(ctx).decode()))
        return dt, dict(zip(names, (int(v) for v in cnt)))

    def digest(form, dev):
        """statuses, out_key, replay marks and the n output rows of the last call"""
        rows = RB if form == "wire" else 128
        parts = (st.cpu().numpy(), ok.cpu().numpy(), rp.cpu().numpy(), out[:N * rows].cpu().numpy()) if dev else (h_st, h_ok, h_rp, h_out[:N * rows])
        hh = hashlib.sha256()
        for p in parts:
            hh.update(p.tobytes())
        return hh.hexdigest(), int((parts[0] == 0).sum())

    def run_mixes(form, dev, ptr, check):
        res = {"s": {}, "counts": {}, "sha256": {}, "accepted": {}}
        s = r = None
        for m in MIXES:
            if m != "served":                                           # (served: the flood's sets)
                if s is not None:
                    s.close(); r.close()
                s, r = capi.NullifierSet(4 * N), capi.NullifierSet(4 * N)
            res["s"][m], res["counts"][m] = call(form, dev, ptr["flood" if m == "served" else m], s, r)
            if check:
                res["sha256"][m], res["accepted"][m] = digest(form, dev)
                assert res["accepted"][m] == N, (m, res["accepted"][m])
                assert (len(s), len(r)) == ({"none": N, "twice": N // 2, "eight": N // 8}.get(m, 1),) * 2, (m, len(s), len(r))
        s.close(); r.close()
        return res

    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == "quit":
            break
        if cmd[0] == "cell":                                            # the cell's tables, then every mix once on sets of its own
            form, dev = cmd[1], cmd[2] == "hbm"
            state.clear()
            torch.cuda.empty_cache()
            held = {}
            for m, idx in pick.items():
                t = view if m == "none" else view[idx]
                if form == "wire":
                    wire = torch.empty((N, ML), dtype=torch.uint8, device="cuda")
                    torch.cuda.synchronize()
                    eng._ck(lib.act_cbor_encode_batch(ctx, capi.CBOR_TYPES["SpendProof"], N, capi.MEM_DEVICE, t.data_ptr(), wire.data_ptr()))
                    t = wire
                held[m] = t if dev else t.cpu().numpy()
                torch.cuda.synchronize()
            ptr = {m: (t.data_ptr() if dev else t.ctypes.data) for m, t in held.items()}
            state.update(form=form, dev=dev, held=held, ptr=ptr)
            say({"warmup": run_mixes(form, dev, ptr, True)})
        elif cmd[0] == "rep":
            say({"rep": run_mixes(state["form"], state["dev"], state["ptr"], False)})
        elif cmd[0] == "prof":                                          # one more call without copies, the kernel timers on
            eng.prof_enable(True); eng.prof_reset()
            s, r = capi.NullifierSet(4 * N), capi.NullifierSet(4 * N)
            dt, _ = call(state["form"], state["dev"], state["ptr"]["none"], s, r)
            prof = eng.prof()
            eng.prof_enable(False)
            s.close(); r.close()
            say({"prof": {"s": dt, "kernels": prof}})
    eng.close()


class Child:
    def __init__(self, name, root, log2):
        self.name = name
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", root, "--log2", str(log2)], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                  bufsize=0)
        self.buf = b""

    def tell(self, line):
        self.p.stdin.write((line + "\n").encode()); self.p.stdin.flush()

    def hear(self, seconds):
        """the child's next CHILD line, or None when it ends or stays silent for `seconds`"""
        deadline = time.monotonic() + seconds
        while True:
            while b"\n" in self.buf:
                line, self.buf = self.buf.split(b"\n", 1)
                if line.startswith(b"CHILD "):
                    return json.loads(line[6:].decode())
            left = deadline - time.monotonic()
            if left <= 0 or not select.select([self.p.stdout], [], [], left)[0]:
                return None
            more = os.read(self.p.stdout.fileno(), 1 << 16)
            if not more:
                return None
            self.buf += more

    def end(self):
        try:
            self.tell("quit")
            self.p.wait(timeout=60)
        except Exception:
            self.p.kill()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a checkout of the parent commit with its library built")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "admit_replay_copies_probe.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--log2", type=int, default=18)
    ap.add_argument("--no-host", action="store_true", help="leave the host-memory cells out")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(os.path.abspath(a.child), a.log2)
    if not a.parent:
        ap.error("--parent DIR is required")
    if a.reps < 5:
        ap.error("the median is taken over at least five repetitions")
    kids = [Child("parent", os.path.abspath(a.parent), a.log2), Child("this", HERE, a.log2)]

    def ask(kid, line, seconds):
        if line:
            kid.tell(line)
        got = kid.hear(seconds)
        if got is None:                                                 # nothing more is started on the device behind a failed child
            for k in kids:
                k.p.kill()
            raise SystemExit("the %s child failed or fell silent behind '%s'" % (kid.name, line))
        return got

    ready = [ask(k, "", 900) for k in kids]
    assert not ready[0]["unique"] and ready[1]["unique"]
    n = ready[1]["lanes"]
    print("proofs made in %.1f s / %.1f s" % (ready[0]["made_proofs_s"], ready[1]["made_proofs_s"]), flush=True)
    rows = []
    for form in ("records", "wire"):
        for mem in ("hbm",) if a.no_host else ("hbm", "host"):
            warm = [ask(k, "cell %s %s" % (form, mem), 900)["warmup"] for k in kids]
            equal = {m: warm[0]["sha256"][m] == warm[1]["sha256"][m] for m in MIXES}
            print("%s %s: outputs equal to the baseline's: %s" % (form, mem, equal), flush=True)
            times = {"parent": {m: [] for m in MIXES}, "this": {m: [] for m in MIXES}}
            for rep in range(a.reps):
                for k in kids:                                          # interleaved
                    got = ask(k, "rep", 600)["rep"]
                    for m in MIXES:
                        times[k.name][m].append(got["s"][m])
                print("%s %s rep %d: %s" % (form, mem, rep, {k: ["%.3f" % times[k][m][-1] for m in MIXES] for k in times}), flush=True)
            row = {"form": form, "mem": mem, "lanes": n, "mixes": {}}
            for m in MIXES:
                base, new = times["parent"][m], times["this"][m]
                mb, mn = statistics.median(base), statistics.median(new)
                row["mixes"][m] = {"base_lanes_per_s": n / mb, "lanes_per_s": n / mn, "ratio": mb / mn, "base_spread": (max(base) - min(base)) / mb,
                                   "spread": (max(new) - min(new)) / mn, "base_s": base, "s": new, "warmup_s": [w["s"][m] for w in warm],
                                   "outputs_equal_to_baseline": equal[m], "counts": warm[1]["counts"][m], "base_counts": warm[0]["counts"][m]}
                print(json.dumps({"form": form, "mem": mem, "mix": m, **{k2: row["mixes"][m][k2] for k2 in ("base_lanes_per_s", "lanes_per_s", "ratio", "base_spread")}}), flush=True)
            none = row["mixes"]["none"]
            if mem == "hbm":
                none["bound"] = 1 - (none["base_spread"] + 0.01)
                none["condition_met"] = none["ratio"] >= none["bound"]
                row["prof_none"] = ask(kids[1], "prof", 600)["prof"]
            else:                                                       # the copy share at which the two forms cost the same, between its neighbours
                pts = [(SHARE[m], row["mixes"][m]["ratio"]) for m in ("none", "twice", "eight")]
                row["crossover_copy_share"] = next((f0 + (1 - r0) * (f1 - f0) / (r1 - r0) for (f0, r0), (f1, r1) in zip(pts, pts[1:]) if r0 < 1 <= r1),
                                                   0.0 if pts[0][1] >= 1 else None)
            rows.append(row)
    for k in kids:
        k.end()
    res = {"tool": "tools/admit_replay_copies_probe.py", "device": ready[1]["device"], "L": 128, "lanes": n, "reps": a.reps, "transcripts": "device",
           "baseline": "act_redeem_(cbor_)admit_replay_batch of the parent commit's build on the same batch and sets, interleaved", "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
