"""The admission family pinned to a recorded run: every act_redeem_(cbor_)*_batch entry point that ends in the admission body or in the
replay tail, called through the C ABI itself (no binding method in between) on fixed batches, and everything a caller can see kept:
rc, statuses, out_key, replay marks and counts verbatim, SHA-256 of the output bytes (guard bytes included) and of each set's sorted
exported (key, epoch) pairs.  tests/test_gpu_admit_forms_pinned.py replays the matrix against the built library and compares it with
tests/golden/admit_forms_L8.json, which this file records from ANOTHER checkout (the commit the refactor started from):

    python tests/admit_forms_cases.py --record --tree DIR --commit SHA [--out tests/golden/admit_forms_L8.json]

DIR: a checkout of that commit with its library built, loaded under another module name (as tools/return_replay_probe.py loads its
baseline).  The world is tests/test_gpu_replay.py's (L = 8, 257 tokens, two keys, two proofs per token, fixed seeds); the calls run on
an engine with max_batch = 16, so a verification window is 64 lanes."""
import argparse
import ctypes as C
import hashlib
import importlib
import importlib.util
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, os.path.join(ROOT, "oracle"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

L, MAX_BATCH = 8, 16
S = 3                                            # test_gpu_replay.SPEND
EPOCHS = [7, 8]
SALT_SET, SALT_RECEIPTS = bytes(range(16)), bytes(range(16, 32))
CAP = 4096
GUARD, GUARD_LEN = 0xA5, 16
PRE_SPENT = list(range(200, 230))                # redeemed before every case, token t for the amount t % 3
shake = lambda label, n: hashlib.shake_256(label.encode()).digest(n)
NONCE_KEY = shake("replay-nonce-key", 32)
scalar = lambda v: int(v).to_bytes(32, "little")

# name -> (symbol stem, has receipts / nonce_key / replayed, takes charges, takes returned, name of the capi count tuple, record row)
FORMS = {
    "admit": ("admit", False, True, False, "ADMIT_COUNTS", 128),
    "admit_unique": ("admit_unique", False, True, False, "ADMIT_UNIQUE_COUNTS", 128),
    "return": ("return", False, True, True, "REDEEM_RETURN_COUNTS", 160),
    "return_unique": ("return_unique", False, True, True, "REDEEM_RETURN_UNIQUE_COUNTS", 160),
    "replay": ("replay", True, False, False, "REPLAY_COUNTS", 128),
    "admit_replay": ("admit_replay", True, True, False, "ADMIT_REPLAY_COUNTS", 128),
    "admit_replay_unique": ("admit_replay_unique", True, True, False, "ADMIT_REPLAY_UNIQUE_COUNTS", 128),
    "return_replay": ("return_replay", True, True, True, "RETURN_REPLAY_COUNTS", 160),
    "return_replay_unique": ("return_replay_unique", True, True, True, "RETURN_REPLAY_UNIQUE_COUNTS", 160),
}
BATCHES = ("n0", "n1", "valid70", "shed70", "mix300")


def load_tree(path, name):
    """the binding of another checkout under the module name `name` (its capi finds the library beside itself)"""
    d = os.path.join(os.path.abspath(path), "anonymous-credit-tokens_amd")
    spec = importlib.util.spec_from_file_location(name, os.path.join(d, "__init__.py"), submodule_search_locations=[d])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return importlib.import_module(name + ".capi")


# ---- the batches ----------------------------------------------------------------------------------------------------------------------------
def _mix():
    """300 lanes as (token, variant, how, charge, t, spelling), in a fixed order that interleaves the kinds"""
    lanes = []
    add = lambda toks, variant=0, how=None, charge=S, t=None, spell=None: lanes.extend(
        (k, variant, how, charge, (k % 4) if t is None else t(k), spell) for k in toks)
    add(range(0, 120))                                                     # fresh and valid
    add(range(0, 20))                                                      # byte-identical copies, the same t
    add(range(20, 30), t=lambda k: (k + 1) % 4)                            # copies that name another amount
    add(range(30, 45), variant=1)                                          # the same nullifier with the other K'
    add(range(200, 230), t=lambda k: k % 3)                                # retries with the t they were redeemed for
    add(range(200, 210), t=lambda k: k % 3)                                # ... and copies of those retries
    add(range(210, 220), t=lambda k: (k + 1) % 3)                          # retries with another t
    add(range(220, 230), variant=1)                                        # spent, and another proof: no receipt is theirs
    add(range(120, 135), charge=S + 1)                                     # wrong charges
    add(range(135, 145), t=lambda k: S + 1)                                # t > s
    add(range(145, 160), how="tampered")
    add(range(145, 150), how="tampered")                                   # copies of a rejected leader
    add(range(160, 170), how="undecodable")
    add(range(160, 163), how="undecodable")
    add(range(170, 176), spell="respelled")                                # wire: other spellings of valid proofs (records: valid lanes)
    add(range(176, 186))
    add(range(186, 187), spell="unreadable")                               # wire: one message that does not read
    assert len(lanes) == 300
    order = sorted(range(300), key=lambda i: shake("admit-forms-mix-%d" % i, 8))
    return [lanes[i] for i in order]


def batch_lanes(name):
    if name == "n0":
        return []
    if name == "n1":
        return [(0, 0, None, S, 1, None)]
    if name == "valid70":
        return [(k, 0, None, S, k % 4, None) for k in range(70)]
    if name == "shed70":                         # spent with no receipt of their own, or wrongly charged: shed by every screen
        return [(k, 1, None, S, 0, None) for k in PRE_SPENT] + [(k, 0, None, S + 1, 0, None) for k in range(40)]
    return _mix()


def batch_bytes(eng, world, name, wire):
    """-> (rows: records or messages, charges, amounts, every message canonical)"""
    import admission_cases as ad
    lanes = batch_lanes(name)
    recs = [world.proof(k, v, how) for k, v, how, _, _, _ in lanes]
    charges, amounts = [c for _, _, _, c, _, _ in lanes], [t for _, _, _, _, t, _ in lanes]
    if not wire:
        return recs, charges, amounts, True
    msgs = eng.cbor_encode("SpendProof", b"".join(recs)) if recs else []
    canonical = True
    for i, lane in enumerate(lanes):
        if lane[5] == "respelled":
            msgs[i] = ad.respelled(recs[i], L); canonical = False
        elif lane[5] == "unreadable":
            msgs[i] = msgs[i][:-5]; canonical = False
    return msgs, charges, amounts, canonical


# ---- memory of either kind ------------------------------------------------------------------------------------------------------------------
class Host:
    def up(self, b):
        a = np.frombuffer(bytes(b) + b"\0", np.uint8).copy()
        return a, a.ctypes.data

    def new(self, n, fill):
        a = np.full(n + 2 * GUARD_LEN, GUARD, np.uint8); a[GUARD_LEN:GUARD_LEN + n] = fill
        return a, a.ctypes.data + GUARD_LEN

    def down(self, a):
        return a.tobytes()

    def sync(self):
        pass


class Device:
    def __init__(self):
        import torch
        self.t = torch

    def up(self, b):
        a = self.t.from_numpy(np.frombuffer(bytes(b) + b"\0", np.uint8).copy()).cuda()
        return a, a.data_ptr()

    def new(self, n, fill):
        h = np.full(n + 2 * GUARD_LEN, GUARD, np.uint8); h[GUARD_LEN:GUARD_LEN + n] = fill
        a = self.t.from_numpy(h).cuda()
        return a, a.data_ptr() + GUARD_LEN

    def down(self, a):
        return a.cpu().numpy().tobytes()

    def sync(self):
        self.t.cuda.synchronize()


# ---- the state every case starts from ---------------------------------------------------------------------------------------------------
class Rig:
    """two engines of one binding (the world's, and the max_batch = 16 one the calls run on), the world, and a snapshot of the two sets
    after PRE_SPENT was redeemed by one act_redeem_return_replay_batch"""

    def __init__(self, capi, tmp_dir, make_engine=None):
        from test_gpu_replay import World
        self.capi, self.tmp = capi, tmp_dir
        h = capi.params_new("bench-org", "bench-service", "bench-env", "2024-01-01", device=0)
        make = make_engine or (lambda h_, L_, max_batch: capi.Engine(h_, L_, device=0, max_batch=max_batch))
        self.world = World(make(h, L, max_batch=4096))
        self.eng = make(h, L, max_batch=MAX_BATCH)
        self.keys = np.frombuffer(b"".join(self.world.keys), np.uint8).copy()
        self.epochs = np.array(EPOCHS, np.uint32)
        self.nonce = np.frombuffer(NONCE_KEY, np.uint8).copy()
        self._bytes = {}
        ns, rs = self.sets(fresh=True)
        recs = b"".join(self.world.proof(k) for k in PRE_SPENT)
        self.eng.set_transcript_mode(capi.TRANSCRIPT_HOST)
        st = self.eng.redeem_return_replay(ns, rs, self.world.keys, recs, NONCE_KEY, key_epochs=EPOCHS, returned=b"".join(scalar(k % 3) for k in PRE_SPENT))[0]
        assert st == bytes(len(PRE_SPENT))
        ns.save(os.path.join(tmp_dir, "set.snap")); rs.save(os.path.join(tmp_dir, "receipts.snap"))
        ns.close(); rs.close()

    def sets(self, fresh=False):
        c = self.capi
        if fresh:
            return c.NullifierSet(CAP, salt=SALT_SET), c.NullifierSet(CAP, salt=SALT_RECEIPTS)
        return (c.NullifierSet.restore(os.path.join(self.tmp, "set.snap"), CAP, salt=SALT_SET),
                c.NullifierSet.restore(os.path.join(self.tmp, "receipts.snap"), CAP, salt=SALT_RECEIPTS))

    def batch(self, name, wire):
        if (name, wire) not in self._bytes:
            self._bytes[name, wire] = batch_bytes(self.eng, self.world, name, wire)
        return self._bytes[name, wire]


def pairs_digest(s):
    keys, eps = s.export_epochs()
    rows = sorted((keys[32 * i:32 * i + 32], int(eps[i])) for i in range(len(eps)))
    return hashlib.sha256(b"".join(k + e.to_bytes(4, "little") for k, e in rows)).hexdigest()


def variants(rig, form, wire, mem):
    """the cases of one (form, wire, memory kind): (case id, batch, offsets given, wire reader)"""
    capi = rig.capi
    out = []
    for name in BATCHES:
        out.append((name, True, capi.WIRE_READER_DEVICE))
        if wire and rig.batch(name, True)[3]:
            out.append((name, False, capi.WIRE_READER_DEVICE))
        if wire and name == "mix300":
            out.append((name, True, capi.WIRE_READER_HOST))
    tag = lambda name, offs, reader: "%s/%s/%s/%s%s%s" % (form, "wire" if wire else "records", mem, name, "" if offs or not wire else "/no-offsets",
                                                       "/host-reader" if reader == capi.WIRE_READER_HOST else "")
    return [(tag(*v),) + v for v in out]


def run_case(rig, form, wire, mem, name, offsets_given, reader):
    """one call on restored sets -> what the fixture keeps of it"""
    capi, eng = rig.capi, rig.eng
    stem, replay, has_charge, has_returned, counts_name, row = FORMS[form]
    rows, charges, amounts, _ = rig.batch(name, wire)
    n = len(rows)
    ob = eng.cbor_size("RefundReturn" if has_returned else "Refund") if wire else row
    m = Device() if mem == "device" else Host()
    eng.set_transcript_mode(capi.TRANSCRIPT_DEVICE if mem == "device" else capi.TRANSCRIPT_HOST)
    eng.set_wire_reader(reader)
    ns, rs = rig.sets()
    keep = []

    def up(b):
        a, p = m.up(b); keep.append(a)
        return p
    src = up(b"".join(rows))
    offs = np.zeros(n + 1, np.uint64)
    if wire:
        offs[1:] = np.cumsum([len(x) for x in rows], dtype=np.uint64)
    o, po = m.new(ob * n, 7); s, ps = m.new(n, 99); k, pk = m.new(n, 77); r, pr = m.new(n, 55)
    cnt = (C.c_uint64 * len(getattr(capi, counts_name)))()
    args = [eng.ctx, ns.h] + ([rs.h] if replay else []) + [n, capi.MEM_DEVICE if mem == "device" else capi.MEM_HOST, rig.keys.ctypes.data, 2, rig.epochs.ctypes.data,
                                                          capi.SIGN_MATCHED, src]
    if wire:
        args.append(offs.ctypes.data if offsets_given else None)
    if has_charge:
        args.append(up(b"".join(scalar(c) for c in charges)))
    if has_returned:
        args.append(up(b"".join(scalar(t) for t in amounts)))
    if replay:
        args += [rig.nonce.ctypes.data, po, ps, pk, pr, cnt]
    else:
        args += [up(shake("admit-forms-rng", 128 * n)), capi.RNG_PER_LANE, po, ps, pk, cnt]
    m.sync()
    rc = getattr(eng.lib, "act_redeem_%s%s_batch" % ("cbor_" if wire else "", stem))(*args)
    m.sync()
    got = {"rc": int(rc), "status": m.down(s).hex(), "out_key": m.down(k).hex(), "replayed": m.down(r).hex() if replay else None,
           "counts": [int(v) for v in cnt], "out_sha256": hashlib.sha256(m.down(o)).hexdigest(), "set_sha256": pairs_digest(ns),
           "receipts_sha256": pairs_digest(rs) if replay else None}
    eng.set_wire_reader(capi.WIRE_READER_DEVICE)
    ns.close(); rs.close()
    return got


def matrix():
    return [(form, wire, mem) for form in FORMS for wire in (False, True) for mem in ("host", "device")]


# ---- the fixture: arrays are kept once in a pool, a case names them by number ------------------------------------------------------------
ARRAYS = ("status", "out_key", "replayed")


def pack(cases, commit):
    pool, where = [], {}
    for got in cases.values():
        for a in ARRAYS:
            if got[a] is not None:
                if got[a] not in where:
                    where[got[a]] = len(pool); pool.append(got[a])
                got[a] = where[got[a]]
    return {"recorded_from": commit, "L": L, "max_batch": MAX_BATCH, "guard": "%d bytes of 0x%02X on either side of every output array" % (GUARD_LEN, GUARD),
            "pool": pool, "cases": cases}


def unpack(fixture):
    pool = fixture["pool"]
    return {cid: dict(got, **{a: pool[got[a]] for a in ARRAYS if got[a] is not None}) for cid, got in fixture["cases"].items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", action="store_true", required=True)
    ap.add_argument("--tree", required=True)
    ap.add_argument("--commit", required=True)
    ap.add_argument("--out", default=os.path.join(HERE, "golden", "admit_forms_L8.json"))
    a = ap.parse_args()
    capi = load_tree(a.tree, "act_recorded")
    cases = {}
    with tempfile.TemporaryDirectory() as tmp:
        rig = Rig(capi, tmp)
        for form, wire, mem in matrix():
            for cid, name, offs, reader in variants(rig, form, wire, mem):
                cases[cid] = run_case(rig, form, wire, mem, name, offs, reader)
                print(cid, cases[cid]["rc"], cases[cid]["counts"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(pack(cases, a.commit), f, separators=(",", ":"))
        f.write("\n")
    print("recorded %d cases from %s -> %s" % (len(cases), a.commit, a.out))


if __name__ == "__main__":
    main()
