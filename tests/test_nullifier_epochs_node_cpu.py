"""Nullifier epochs over a node without a device: csrc/node.cpp + csrc/node_keyring.cpp + csrc/node_epochs.cpp linked against the
TEST-ONLY stand-ins (tests/node_mock, and tests/node_mock_epochs/node_mock_epochs.cpp which keeps the epochs beside node_mock.cpp's
key sets).  Answers and epochs must land on the right lanes whatever the routing, a lane with a bad index is undetermined while the
others are served, a retirement that fails on one device leaves the rest valid and a repeat completes it, epoch_len sums over the
devices and the node cursor of export_epochs covers all parts.  The same code over real sets is tests/test_gpu_nullifier_epochs.py.

(The stand-in keeps its epochs in a table keyed by the set's address, so the sets of this module are never destroyed.)"""
import ctypes as C
import os
import random
import subprocess

import pytest

from conftest import ELL, ROOT
from test_node_dispatch_cpu import PB, make_node, records

DONE = 2**64 - 1
u32, u64, sz = C.c_uint32, C.c_uint64, C.c_size_t


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("node_mock_epochs") / "libnode_mock_epochs.so")
    csrc = os.path.join(ROOT, "anonymous-credit-tokens_amd", "csrc")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-pthread", "-o", out, os.path.join(csrc, "node.cpp"),
                    os.path.join(csrc, "node_keyring.cpp"), os.path.join(csrc, "node_epochs.cpp"),
                    os.path.join(ROOT, "tests", "node_mock_epochs", "node_mock_epochs.cpp"), os.path.join(ROOT, "tests", "node_mock", "node_mock_keyring.cpp")], check=True)
    l = C.CDLL(out)
    l.act_node_ctx.restype = C.c_void_p
    l.act_node_ctx.argtypes = [C.c_void_p, C.c_int]
    l.act_mock_lanes.restype = C.c_size_t
    l.act_mock_lanes.argtypes = [C.c_void_p]
    l.act_node_nullifier_set_len.restype = C.c_size_t
    l.act_node_nullifier_set_last_error.restype = C.c_char_p
    return l


def new_set(lib, ndev, cap=100000, salt=b"0123456789abcdef"):
    ns = C.c_void_p()
    devs = (C.c_int * ndev)(*range(ndev))
    assert lib.act_node_nullifier_set_create(devs, ndev, sz(cap), salt, C.byref(ns)) == 0
    return ns


def insert(lib, ns, vals, mask, eidx, table):
    n = len(vals)
    keys = b"".join(v.to_bytes(32, "little") for v in vals)
    out = C.create_string_buffer(max(1, n))
    tab = (u32 * len(table))(*table)
    rc = lib.act_node_nullifier_check_and_insert_epoch_batch(ns, sz(n), keys, sz(32), mask, eidx, tab, len(table), out)
    return rc, out.raw[:n]


def epoch_len(lib, ns, e):
    c = u64(0)
    assert lib.act_node_nullifier_set_epoch_len(ns, u32(e), C.byref(c)) == 0
    return c.value


def retired(lib, ns):
    n = sz(0)
    assert lib.act_node_nullifier_set_retired_epochs(ns, None, sz(0), C.byref(n)) == 0
    buf = (u32 * max(1, n.value))()
    assert lib.act_node_nullifier_set_retired_epochs(ns, buf, sz(n.value), C.byref(n)) == 0
    return list(buf[:n.value])


def export(lib, ns, max_keys):
    cur, pairs = u64(0), {}
    keys = C.create_string_buffer(32 * max_keys); eps = (u32 * max_keys)(); got = sz(0)
    while cur.value != DONE:
        assert lib.act_node_nullifier_set_export_epochs(ns, C.byref(cur), sz(max_keys), keys, eps, C.byref(got)) == 0
        for i in range(got.value):
            k = int.from_bytes(keys.raw[32 * i:32 * i + 32], "little")
            assert k not in pairs, "a key exported twice"
            pairs[k] = eps[i]
    return pairs


def model_step(model, vals, mask, eidx, table):
    ans = []
    for i, v in enumerate(vals):
        if mask and mask[i]:
            ans.append(0); continue
        e = eidx[i] if eidx else 0
        if e >= len(table):
            ans.append(2); continue
        k = v % ELL
        ans.append(1 if k in model else 0)
        model.setdefault(k, table[e])
    return bytes(ans)


@pytest.mark.parametrize("ndev", [1, 2, 3, 8])
def test_answers_and_epochs_land_on_the_right_lanes(lib, ndev):
    r = random.Random(100 + ndev)
    pool = [r.randrange(ELL) for _ in range(3000)]
    table = [4, 0, 90000]
    ns = new_set(lib, ndev)
    model = {}
    for n in (1, 700, 9000, 33):
        vals = [pool[r.randrange(len(pool))] for _ in range(n)]
        vals = [v + ELL if r.random() < 0.125 and v + ELL < 2**256 else v for v in vals]
        mask = bytes(1 if r.random() < 0.2 else 0 for _ in range(n))
        eidx = bytes(r.randrange(3) for _ in range(n))
        want = model_step(model, vals, mask, eidx, table)
        assert insert(lib, ns, vals, mask, eidx, table) == (0, want), n
        assert lib.act_node_nullifier_set_len(ns) == len(model)
        for e in table + [5]:
            assert epoch_len(lib, ns, e) == sum(1 for v in model.values() if v == e)
    for mk in (7, 1000, 1 << 16):                                   # the node cursor covers every part
        assert export(lib, ns, mk) == model, mk
    # no indices: every lane under table[0]; the existing call records epoch 0 on the same set
    vals = [r.randrange(ELL) for _ in range(500)]
    assert insert(lib, ns, vals, None, None, [77]) == (0, model_step(model, vals, None, None, [77]))
    keys = b"".join(v.to_bytes(32, "little") for v in vals[:100] + pool[:100])
    out = C.create_string_buffer(200)
    assert lib.act_node_nullifier_check_and_insert_batch(ns, sz(200), keys, sz(32), None, out) == 0
    assert out.raw == model_step(model, vals[:100] + pool[:100], None, None, [0])
    assert export(lib, ns, 5000) == model and epoch_len(lib, ns, 77) == 500


def test_a_bad_index_is_undetermined_and_the_others_are_served(lib):
    r = random.Random(7)
    ns = new_set(lib, 3)
    vals = [r.randrange(ELL) for _ in range(600)]
    vals[300:310] = vals[290:300]                                   # repeats: a bad-index lane does not shadow the repeat behind it
    eidx = bytes(255 if i % 10 == 5 else 3 if i % 10 == 7 else i % 3 for i in range(600))
    mask = bytes(1 if i % 50 == 0 else 0 for i in range(600))
    table = [1, 2, 3]
    model = {}
    want = model_step(model, vals, mask, eidx, table)
    assert want.count(2) > 100 and want.count(1) > 0
    rc, got = insert(lib, ns, vals, mask, eidx, table)
    assert rc == 1 and got == want
    assert b"index" in lib.act_node_nullifier_set_last_error(ns)
    assert export(lib, ns, 1000) == model and lib.act_node_nullifier_set_len(ns) == len(model)
    # a table entry above the maximum: the whole call is refused, nothing recorded
    rc, got = insert(lib, ns, vals, mask, eidx, [1, 2, 1 << 24])
    assert rc == 1 and got == bytes(0 if m else 2 for m in mask) and export(lib, ns, 1000) == model
    # bad arguments
    tab = (u32 * 1)(0)
    assert lib.act_node_nullifier_check_and_insert_epoch_batch(ns, sz(1), bytes(32), sz(32), None, None, tab, 0, C.create_string_buffer(1)) == 1
    assert lib.act_node_nullifier_check_and_insert_epoch_batch(ns, sz(1), bytes(32), sz(32), None, None, None, 1, C.create_string_buffer(1)) == 1


def test_retire_with_one_device_failing_then_a_repeat(lib):
    r = random.Random(8)
    ndev = 4
    ns = new_set(lib, ndev)
    vals = [r.randrange(ELL) for _ in range(4000)]
    eidx = bytes(i % 3 for i in range(4000))
    model = {}
    assert insert(lib, ns, vals, None, eidx, [0, 6, 7])[0] == 0
    model_step(model, vals, None, eidx, [0, 6, 7])
    per_epoch = 4000 // 3
    removed = u64(99)
    for bad in (0, 1 << 24):
        assert lib.act_node_nullifier_set_retire_epoch(ns, u32(bad), C.byref(removed)) == 1 and removed.value == 0
    assert export(lib, ns, 5000) == model and retired(lib, ns) == []
    lib.act_mock_epochs_fail(2, 1)
    try:
        rc = lib.act_node_nullifier_set_retire_epoch(ns, u32(6), C.byref(removed))
        assert rc == 2 and b"device 2" in lib.act_node_nullifier_set_last_error(ns)
        first = removed.value
        assert 0 < first < per_epoch
        # every set is valid: the failed device still holds its keys of the epoch, the others have dropped theirs
        left = export(lib, ns, 5000)
        assert len(left) == 4000 - first and all(model[k] == e for k, e in left.items())
        assert sum(1 for e in left.values() if e == 6) == per_epoch - first == epoch_len(lib, ns, 6)
        assert retired(lib, ns) == []                               # not retired for the node until every device has
        # ... but an insert naming it is refused already
        rc, got = insert(lib, ns, [1, 2, 3], None, None, [6])
        assert rc == 1 and got == b"\2\2\2" and b"retired" in lib.act_node_nullifier_set_last_error(ns)
    finally:
        lib.act_mock_epochs_fail(-1, 0)
    assert lib.act_node_nullifier_set_retire_epoch(ns, u32(6), C.byref(removed)) == 0 and removed.value == per_epoch - first
    assert retired(lib, ns) == [6] and epoch_len(lib, ns, 6) == 0
    model = {k: e for k, e in model.items() if e != 6}
    assert export(lib, ns, 5000) == model and lib.act_node_nullifier_set_len(ns) == len(model)
    assert lib.act_node_nullifier_set_retire_epoch(ns, u32(6), C.byref(removed)) == 0 and removed.value == 0
    assert lib.act_node_nullifier_set_retire_epoch(ns, u32(3), None) == 0 and retired(lib, ns) == [3, 6]
    n = sz(0); one = (u32 * 1)()
    assert lib.act_node_nullifier_set_retired_epochs(ns, one, sz(1), C.byref(n)) == 0 and (n.value, one[0]) == (2, 3)
    # a removed key under a live epoch is fresh again
    gone = [v for i, v in enumerate(vals) if i % 3 == 1][:50]
    assert insert(lib, ns, gone, None, None, [7]) == (0, bytes(50))
    # one device of the insert failing: its lanes undetermined, the others final
    lib.act_mock_epochs_fail(1, 2)
    try:
        fresh = [r.randrange(ELL) for _ in range(400)]
        rc, got = insert(lib, ns, fresh, None, bytes(400), [7])
        assert rc == 2 and set(got) == {0, 2} and 0 < got.count(2) < 400
    finally:
        lib.act_mock_epochs_fail(-1, 0)
    rc, again = insert(lib, ns, fresh, None, bytes(400), [7])
    assert rc == 0 and again == bytes(1 if g == 0 else 0 for g in got)


def ring(nkeys):
    return b"".join(bytes([0x40 + k]) + bytes(63) for k in range(nkeys))


@pytest.mark.parametrize("ndev", [1, 3])
def test_node_ring_redemption_records_the_matched_epoch(lib, ndev):
    nd = make_node(lib, ndev)
    n, nkeys = 500, 3
    keys = ring(nkeys)
    key_epochs = (u32 * nkeys)(11, 12, 13)
    proofs = bytearray(records(n, PB, 5 * ndev))
    r = random.Random(3)
    for i in range(n):                                              # distinct nullifiers below l, some lanes repeated
        proofs[PB * i + 9:PB * i + 32] = bytes(r.randrange(256) for _ in range(22)) + b"\0"
    proofs[PB * 400:PB * 420] = proofs[PB * 100:PB * 120]
    proofs = bytes(proofs)
    rng = records(n, 128, 9)
    ref, ns = new_set(lib, 2), new_set(lib, 2)
    outs = []
    for epochs in (False, True):
        out, st, ok = C.create_string_buffer(128 * n), C.create_string_buffer(n), C.create_string_buffer(n)
        if epochs:
            rc = lib.act_node_redeem_keyring_epochs_batch(nd, ns, sz(n), keys, nkeys, key_epochs, -1, proofs, rng, 1, out, st, ok)
        else:
            rc = lib.act_node_redeem_keyring_batch(nd, ref, sz(n), keys, nkeys, -1, proofs, rng, 1, out, st, ok)
        assert rc == 0
        outs.append((out.raw, st.raw, ok.raw))
    assert outs[0] == outs[1]                                       # statuses, refunds, out_key: the existing call's
    st, ok = outs[0][1], outs[0][2]
    assert st.count(b"\3") > 0 and st.count(b"\7") > 0
    want = {}
    for i in range(n):
        if st[i] == 0:
            want[int.from_bytes(proofs[PB * i:PB * i + 32], "little") % ELL] = (11, 12, 13)[ok[i]]
    assert export(lib, ns, 1000) == want and set(export(lib, ref, 1000).values()) == {0}
    # the wire form
    msgs = b"".join(b"\0\0\0" + proofs[PB * i:PB * i + PB] for i in range(n))
    ref2, ns2 = new_set(lib, 2), new_set(lib, 2)
    wire = []
    for epochs in (False, True):
        out, st2, ok2 = C.create_string_buffer(129 * n), C.create_string_buffer(n), C.create_string_buffer(n)
        if epochs:
            rc = lib.act_node_redeem_cbor_keyring_epochs_batch(nd, ns2, sz(n), keys, nkeys, key_epochs, 1, msgs, None, rng, 1, out, st2, ok2)
        else:
            rc = lib.act_node_redeem_cbor_keyring_batch(nd, ref2, sz(n), keys, nkeys, 1, msgs, None, rng, 1, out, st2, ok2)
        assert rc == 0
        wire.append((out.raw, st2.raw, ok2.raw))
    assert wire[0] == wire[1] and wire[0][1:] == (st, ok)
    assert export(lib, ns2, 1000) == want                           # the matched key's epoch, not the signing key's
    # a retired epoch, or one above the maximum, fails the call before anything is verified or written
    assert lib.act_node_nullifier_set_retire_epoch(ns, u32(12), None) == 0
    lanes0 = lib.act_mock_lanes(lib.act_node_ctx(nd, 0))
    for bad in ((11, 12, 13), (11, 1 << 24, 13)):
        out, st3, ok3 = C.create_string_buffer(b"\7" * (128 * n)), C.create_string_buffer(b"\7" * n), C.create_string_buffer(b"\7" * n)
        assert lib.act_node_redeem_keyring_epochs_batch(nd, ns, sz(n), keys, nkeys, (u32 * 3)(*bad), -1, proofs, rng, 1, out, st3, ok3) == 1
        assert st3.raw[:n] == b"\7" * n and ok3.raw[:n] == b"\7" * n and out.raw[:128 * n] == b"\7" * (128 * n)
    assert lib.act_mock_lanes(lib.act_node_ctx(nd, 0)) == lanes0       # no verification work was started
    assert lib.act_node_redeem_keyring_epochs_batch(nd, ns, sz(n), keys, nkeys, None, -1, proofs, rng, 1, out, st3, ok3) == 1
