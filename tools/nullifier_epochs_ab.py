"""Nullifier epochs: did the existing set calls or the ring redemption get slower?  A/B against the PARENT commit's build on one box.

The parent tree (a checkout of the parent commit with its library built: `git worktree add DIR HEAD~; make -C DIR/anonymous-credit-tokens_amd/csrc`)
and this tree are measured by child processes, alternating, `--reps` times each (a child imports the package of the tree it is given,
so each build runs behind its own binding).  Per child, on one MI355X:
    set        a set of 2^24 recorded keys; 2^22-key batches from device memory, half recorded, half not:
               check_and_insert (existing call, on a fresh set of the same size), contains, and -- this tree only -- the epoch insert
               of the same batch with a random index over a table of four epochs
    redeem     2^log2 distinct proofs (L = 128) resident in HBM, half under each key of a ring of two, per-lane rng in HBM, a fresh set
               per call: act_redeem_keyring_batch, and -- this tree only -- act_redeem_keyring_epochs_batch
Every timed call follows a warm-up of the same shape; host clock around calls that end in a device synchronise.
The bar: this tree's medians stay within the spread the parent's own repetitions show, doubled (recorded as `holds`).

    python tools/nullifier_epochs_ab.py --parent DIR [--out profiles/nullifier_epochs_probe.json] [--reps 3] [--redeem-log2 18]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(root, redeem_log2):
    sys.path.insert(0, root)
    os.chdir(root)
    import numpy as np
    import torch
    import act_amd  # noqa: F401
    from act_amd import capi
    if redeem_log2:
        import bench                                                 # the tree's own, before this tree's tools directory joins the path
    sys.path.insert(0, os.path.join(HERE, "tools"))
    from nullifier_store_probe import fill, keys_on_device, timed
    has_epochs = hasattr(capi.NullifierSet, "check_and_insert_epoch_dev")
    res = {"root": root, "has_epochs": has_epochs}
    n, m = 1 << 24, 1 << 22
    s, keys = fill(capi, torch, n, 1024)
    q = torch.cat([keys[:m // 2], keys_on_device(torch, m - m // 2, 31)])
    found = torch.zeros(m, dtype=torch.uint8, device="cuda")
    eidx = torch.randint(0, 4, (m,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s.contains_dev(m, q.data_ptr(), 32, found.data_ptr())
    t, _ = timed(torch, lambda: s.contains_dev(m, q.data_ptr(), 32, found.data_ptr()))
    assert int(found.sum().item()) == m // 2
    res["contains_keys_per_s"] = m / t
    s.close()
    calls = [("check_and_insert", lambda s2: s2.check_and_insert_dev(m, q.data_ptr(), 32, 0, found.data_ptr()))]
    if has_epochs:
        calls.append(("epoch_insert", lambda s2: s2.check_and_insert_epoch_dev(m, q.data_ptr(), 32, 0, eidx.data_ptr(), [0, 5, 6, 7], found.data_ptr())))
    for name, fn in calls:
        for rep in range(2):                                          # the first is the warm-up
            s2 = capi.NullifierSet(n, device=0)
            t, _ = timed(torch, lambda: fn(s2))
            assert len(s2) == m
            s2.close()
        res[name + "_keys_per_s"] = m / t
    del keys, q, found
    if redeem_log2:
        import hashlib
        N, L = 1 << redeem_log2, 128
        sh = lambda tag, k: hashlib.shake_256(tag.encode()).digest(k)
        h = capi.params_new("bench-org", "bench-service", "bench-env", "2024-01-01", device=0)
        eng = capi.Engine(h, L, device=0, transcript=capi.TRANSCRIPT_DEVICE)
        A, B = (eng.private_key_random(sh("nep-sk-%d" % i, 64)) for i in range(2))
        proofs = torch.cat([bench.make_distinct_proofs_on_device(eng, capi, torch, np, sk, N // 2, L, seed=200 + i)[0] for i, sk in enumerate((A, B))])
        rng = torch.randint(0, 256, (N, 128), dtype=torch.uint8, device="cuda")
        out = torch.zeros(128 * N, dtype=torch.uint8, device="cuda"); st = torch.zeros(N, dtype=torch.uint8, device="cuda"); ok = torch.zeros(N, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        forms = [("redeem_keyring", {})] + ([("redeem_keyring_epochs", {"key_epochs": (7, 9)})] if has_epochs else [])
        for name, extra in forms:
            for rep in range(2):
                ns = capi.NullifierSet(N, device=0)
                t, _ = timed(torch, lambda: eng.keyring_ptr("redeem", [B, A], N, capi.MEM_DEVICE, set=ns, proofs=proofs.data_ptr(), rng=rng.data_ptr(),
                                                            rng_mode=capi.RNG_PER_LANE, out=out.data_ptr(), status=st.data_ptr(), out_key=ok.data_ptr(), **extra))
                assert int(st.count_nonzero()) == 0 and len(ns) == N
                if extra:
                    assert ns.epoch_len(7) == ns.epoch_len(9) == N // 2
                ns.close()
            res[name + "_proofs_per_s"] = N / t
        eng.close()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a checkout of the parent commit with its library built")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "nullifier_epochs_probe.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--redeem-log2", type=int, default=18)
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(os.path.abspath(a.child), a.redeem_log2)
    if not a.parent:
        raise SystemExit("--parent DIR: the A/B needs the parent commit's build")
    runs = {"parent": [], "this": []}
    for rep in range(a.reps):
        for name, root in (("parent", os.path.abspath(a.parent)), ("this", HERE)):      # alternating: drift of the box hits both builds alike
            t0 = time.perf_counter()
            env = {k: v for k, v in os.environ.items() if k != "ACT_LIB_PATH"}
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, "--redeem-log2", str(a.redeem_log2)], env=env, capture_output=True,
                               text=True, timeout=600)
            line = next((l for l in p.stdout.splitlines() if l.startswith("RESULT ")), None)
            if p.returncode or line is None:
                raise SystemExit("child for %s failed (%d):\n%s\n%s" % (name, p.returncode, p.stdout[-2000:], p.stderr[-4000:]))
            runs[name].append(json.loads(line[7:]))
            print("rep %d %s %.0f s: %s" % (rep, name, time.perf_counter() - t0, line[7:]), flush=True)
    assert not runs["parent"][0]["has_epochs"] and runs["this"][0]["has_epochs"], "--parent is not a build of the parent commit"
    med = lambda rs, k: statistics.median(r[k] for r in rs)
    spread = lambda rs, k: (max(r[k] for r in rs) - min(r[k] for r in rs)) / med(rs, k)
    out = {"reps": a.reps, "parent": {}, "this": {}, "checks": {}}
    for name in runs:
        for k in runs[name][0]:
            if k.endswith("_per_s"):
                out[name][k] = {"median": med(runs[name], k), "spread": spread(runs[name], k), "all": [r[k] for r in runs[name]]}
    # (metric of this tree, the parent's metric it is held against)
    pairs = [("check_and_insert_keys_per_s",) * 2, ("contains_keys_per_s",) * 2, ("epoch_insert_keys_per_s", "check_and_insert_keys_per_s")]
    if a.redeem_log2:
        pairs += [("redeem_keyring_proofs_per_s",) * 2, ("redeem_keyring_epochs_proofs_per_s", "redeem_keyring_proofs_per_s")]
    for mine, ref in pairs:
        margin = 2 * out["parent"][ref]["spread"]
        ratio = out["this"][mine]["median"] / out["parent"][ref]["median"]
        out["checks"][mine] = {"against_parent": ref, "ratio": ratio, "margin": margin, "holds": ratio >= 1 - margin}
    import torch
    out["device"] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out["checks"], indent=1))


if __name__ == "__main__":
    main()
