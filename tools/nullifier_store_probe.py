"""Nullifier-set growth, export and read-only look-up on one GPU: keys/s for export (to host and to device memory), for contains
with check-and-insert beside it, and seconds per reserve (a rehash into a table twice as large) at 2^24 and 2^26 recorded keys.
Epochs: the epoch insert beside check-and-insert (same batch, a random index over a table of four epochs), and on a set whose keys
are spread over four epochs the seconds of one epoch_len and of retire_epoch of one epoch in four (a rehash into a table of the same size).
Host clock around calls that end in a device synchronise; every timed call is preceded by a warm-up of the same shape.

    python tools/nullifier_store_probe.py [--out profiles/nullifier_store_probe.json] [--sizes 24,26]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def keys_on_device(torch, n, seed, chunk=1 << 22):
    """n random canonical scalars (below 2^252 < l, distinct with overwhelming probability), drawn 2^22 rows at a time: one draw
    of 2^31 bytes or more repeats itself"""
    k = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
    g = torch.Generator(device="cuda")
    for i in range(0, n, chunk):
        g.manual_seed(seed * 4096 + i // chunk)
        m = min(chunk, n - i)
        k[i:i + m] = torch.randint(0, 256, (m, 32), dtype=torch.uint8, device="cuda", generator=g)
    k[:, 31] &= 0x0F
    torch.cuda.synchronize()                                  # the set works on a stream of its own: the keys must have landed
    return k


def timed(torch, fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, r


def fill(capi, torch, n, seed, chunk=1 << 22, keys=None, epochs=None):
    """a set of n recorded keys; `epochs` (a table): every key under a random entry of it, the per-key indices returned as well"""
    s = capi.NullifierSet(n, device=0, salt=seed.to_bytes(16, "little"))
    out = torch.zeros(chunk, dtype=torch.uint8, device="cuda")
    keys = keys_on_device(torch, n, seed) if keys is None else keys
    eidx = None
    if epochs:
        g = torch.Generator(device="cuda"); g.manual_seed(seed)
        eidx = torch.randint(0, len(epochs), (n,), dtype=torch.uint8, device="cuda", generator=g)
        torch.cuda.synchronize()
    for i in range(0, n, chunk):
        m = min(chunk, n - i)
        if epochs:
            s.check_and_insert_epoch_dev(m, keys[i:i + m].data_ptr(), 32, 0, eidx[i:i + m].data_ptr(), epochs, out.data_ptr())
        else:
            s.check_and_insert_dev(m, keys[i:i + m].data_ptr(), 32, 0, out.data_ptr())
    torch.cuda.synchronize()
    assert len(s) == n, (len(s), n)
    return (s, keys, eidx) if epochs else (s, keys)


def export_dev_all(capi, s, buf, max_keys):
    cur, total = 0, 0
    while cur != capi.EXPORT_DONE:
        cur, got = s.export_dev(cur, max_keys, buf.data_ptr())
        total += got
    return total


def probe(lg, capi, torch):
    n = 1 << lg
    res = {"recorded_keys": n}
    s, keys = fill(capi, torch, n, 1000 + lg)
    slots = 1 << (2 * n - 1).bit_length()
    res["table_slots"] = slots
    # export to device memory: one call over the whole table (the buffer has room for every slot)
    buf = torch.empty(32 * slots, dtype=torch.uint8, device="cuda")
    export_dev_all(capi, s, buf, slots)
    t, got = timed(torch, lambda: export_dev_all(capi, s, buf, slots))
    assert got == n
    res["export_device"] = {"seconds": t, "keys_per_s": n / t, "max_keys": slots}
    del buf
    # export to host memory through the binding (2^21-slot staging windows, pageable numpy destination)
    s.export(1 << 21)
    t, blob = timed(torch, lambda: s.export(1 << 21))
    assert len(blob) == 32 * n
    res["export_host"] = {"seconds": t, "keys_per_s": n / t, "max_keys": 1 << 21}
    del blob
    # contains vs check-and-insert, 2^22 keys from device memory: half recorded, half not
    m = min(n, 1 << 22)
    q = torch.cat([keys[:m // 2], keys_on_device(torch, m - m // 2, 7 + lg)])
    found = torch.zeros(m, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s.contains_dev(m, q.data_ptr(), 32, found.data_ptr())
    t, _ = timed(torch, lambda: s.contains_dev(m, q.data_ptr(), 32, found.data_ptr()))
    assert int(found.sum().item()) == m // 2
    res["contains"] = {"keys": m, "seconds": t, "keys_per_s": m / t}
    # check-and-insert of the same shape on a fresh set of the same size (warm-up call on another fresh set)
    for rep in range(2):
        s2 = capi.NullifierSet(n, device=0)
        t, _ = timed(torch, lambda: s2.check_and_insert_dev(m, q.data_ptr(), 32, 0, found.data_ptr()))
        s2.close()
    res["check_and_insert"] = {"keys": m, "seconds": t, "keys_per_s": m / t}
    # the epoch insert of the same batch: a random index per lane over a table of four epochs
    table = [0, 11, 12, 13]
    qidx = torch.randint(0, 4, (m,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for rep in range(2):
        s2 = capi.NullifierSet(n, device=0)
        t, _ = timed(torch, lambda: s2.check_and_insert_epoch_dev(m, q.data_ptr(), 32, 0, qidx.data_ptr(), table, found.data_ptr()))
        s2.close()
    res["check_and_insert_epoch"] = {"keys": m, "seconds": t, "keys_per_s": m / t}
    # reserve: a rehash of all n keys into a table twice as large (the first reserve of a process is warmed on a small set)
    w = capi.NullifierSet(1024); w.check_and_insert(bytes(32)); w.reserve(4096); w.close()
    t, _ = timed(torch, lambda: s.reserve(2 * n))
    assert len(s) == n
    moved = slots * 4 + n * 32 + (2 * slots) * 4 * 2 + n * 32          # old states + old keys read, new states cleared + CAS, new keys written
    res["reserve"] = {"seconds": t, "new_table_slots": 2 * slots, "approx_hbm_bytes": moved}
    s.contains_dev(m, q.data_ptr(), 32, found.data_ptr())
    assert int(found.sum().item()) == m // 2
    s.close()
    # epoch_len and retire_epoch on a set of n keys spread over four epochs (the first retirement of a process is warmed on a small set)
    s, _, eidx = fill(capi, torch, n, 2000 + lg, keys=keys, epochs=table)
    want = int((eidx == 2).sum().item())
    s.epoch_len(12)
    t, got = timed(torch, lambda: s.epoch_len(12))
    assert got == want
    res["epoch_len"] = {"seconds": t, "slots_per_s": slots / t, "state_bytes": 4 * slots}
    w = capi.NullifierSet(1024); w.check_and_insert(bytes(32), epochs=[3]); w.retire_epoch(3); w.close()
    t, removed = timed(torch, lambda: s.retire_epoch(12))
    assert removed == want and len(s) == n - want
    moved = slots * 4 * 2 + (n - want) * 32 + slots * 4 * 2 + (n - want) * 32      # states counted and read, kept keys read; new states cleared + CAS, keys written
    res["retire_epoch"] = {"seconds": t, "removed": removed, "of": n, "table_slots": slots, "approx_hbm_bytes": moved}
    s.contains_dev(m, q.data_ptr(), 32, found.data_ptr())
    assert int(found.sum().item()) == int((eidx[:m // 2] != 2).sum().item())
    s.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nullifier_store_probe.json"))
    ap.add_argument("--sizes", default="24,26", help="log2 of the recorded key counts")
    a = ap.parse_args()
    import torch
    from act_amd import capi
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this probe measures the device and has no CPU path")
    out = {"device": torch.cuda.get_device_name(0), "runs": [probe(int(x), capi, torch) for x in a.sizes.split(",")]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
