"""The nullifier set's slot function on the CPU.  The set's design (csrc/nullifier_impl.inc) rests on the slots coming from
SipHash-1-3 of the reduced key under the set's 128-bit salt; the other nullifier tests compare answers with a Python set, which any
function of the key passes.  Here the model of tests/nullifier_model.py is first held to the SipHash paper's own values, then the host
build of null_load_key + null_hash (tests/hostcheck/admit_check.cpp: hc_null_hash) is held to the model, and the admission screen's
read-only probe walks a chain of keys aimed at one slot through the table's wrap."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import admission_cases as ad
import nullifier_model as nm
from conftest import ELL, ROOT


@pytest.fixture(scope="module")
def admit_check():
    lib = C.CDLL(ad.build_admit_check(os.path.join(ROOT, "tests", "hostcheck", "libadmit_check.so")))
    lib.hc_null_hash.restype = C.c_uint64
    lib.hc_null_hash.argtypes = [C.c_char_p, C.c_char_p]
    return lib


def edge_values(r, n_random):
    """raw 256-bit values: the edges of the reduction and n_random scalars, each also spelled k + l where that fits 256 bits"""
    vals = [0, 1, ELL - 1, ELL, ELL + 1, 2**252, 2**256 - 1]
    for _ in range(n_random):
        k = r.randrange(ELL)
        vals.append(k)
        if k + ELL < 2**256:
            vals.append(k + ELL)
    return vals


def test_the_model_reproduces_the_published_siphash_2_4_values():
    """SipHash-2-4 under the key 00 01 .. 0f of the messages 00 01 .. (n-1): the reference implementation's vectors for n = 0 and 1
    and the paper's worked example (Appendix A) for n = 15.  c and d are loop counts in the model, so 1-3 is the same code."""
    key = bytes(range(16))
    assert nm.siphash(key, b"", 2, 4) == 0x726fdb47dd0e0e31
    assert nm.siphash(key, bytes(range(1)), 2, 4) == 0x74f839c593dc67fd
    assert nm.siphash(key, bytes(range(15)), 2, 4) == 0xa129ca6149be45e5
    # the round counts matter to the model
    assert len({nm.siphash(key, bytes(range(15)), c, d) for c, d in ((2, 4), (1, 3), (1, 4), (2, 3))}) == 4


def test_the_vectorised_hash_equals_the_model_lane_for_lane():
    r = random.Random(11)
    for salt in (bytes(range(16)), bytes(16), b"\xff" * 16, bytes(r.randrange(256) for _ in range(16))):
        ks = [0, 1, ELL - 1, 2**252 - 1, 2**252, (1 << 64) - 1, 1 << 64, 1 << 128, 1 << 192] + [r.randrange(ELL) for _ in range(300)]
        got = nm.sip13_keys(nm.int_to_words(ks), salt)
        assert [int(x) for x in got] == [nm.siphash(salt, k.to_bytes(32, "little"), 1, 3) for k in ks]


def test_aimed_keys_start_where_they_were_aimed():
    salt = bytes(range(16))
    ks = nm.aim(salt, 1024, 1021, 40, rng_seed=5)
    assert len(set(ks)) == 40 and all(k < 2**252 for k in ks)
    assert all(nm.start_slot(k, salt, 1024) == 1021 for k in ks)
    assert nm.aim(salt, 1024, 1021, 10, rng_seed=5) == ks[:10]
    both = nm.aim(salt, 1024, 7, 4, batch_cap=1024, batch_slots=range(1016, 1024), rng_seed=5)
    assert all(nm.start_slot(k, salt, 1024) == 7 and nm.batch_slot(k, salt, 1024) >= 1016 for k in both) and len(set(both)) == 4
    anywhere = nm.aim(salt, 1024, None, 30, batch_cap=1024, batch_slots=[1023], rng_seed=5)
    assert all(nm.batch_slot(k, salt, 1024) == 1023 for k in anywhere) and len({nm.start_slot(k, salt, 1024) for k in anywhere}) > 10


def test_the_linear_table_is_order_independent_in_its_occupied_slots():
    r = random.Random(3)
    starts = {k: r.choice((5, 6, 7, 60, 61, 62, 63, r.randrange(64))) for k in range(40)}
    want = None
    for trial in range(20):
        order = list(starts); r.shuffle(order)
        t = nm.LinearTable(64)
        for k in order:
            t.insert(k, starts[k])
        assert want is None or t.occupied() == want
        want = t.occupied()
        assert all(t.slot[k] in t.run_of(k) for k in starts) and sorted(t.at.values()) == sorted(starts)
    assert {0, 1, 2} <= want and 63 in want             # the pile at the end went through the wrap
    assert nm.LinearTable(64).run_of(99, start=3) == []


def test_the_host_build_of_the_slot_hash_is_siphash_1_3_of_the_reduced_key(admit_check):
    r = random.Random(2024)
    salts = [bytes(16), b"\xff" * 16, bytes(range(16))]
    checked = 0
    for v in edge_values(r, 40):
        for salt in salts:
            want = nm.siphash(salt, (v % ELL).to_bytes(32, "little"), 1, 3)
            assert admit_check.hc_null_hash(v.to_bytes(32, "little"), salt) == want, (hex(v), salt.hex())
            checked += 1
    for i in range(10000):
        salt = bytes(r.randrange(256) for _ in range(16))
        v = r.randrange(2**256) if i % 2 else r.randrange(ELL)
        assert admit_check.hc_null_hash(v.to_bytes(32, "little"), salt) == nm.siphash(salt, (v % ELL).to_bytes(32, "little"), 1, 3), (hex(v), salt.hex())
    # k and k + l are one key
    k = r.randrange(2**252)
    assert admit_check.hc_null_hash(k.to_bytes(32, "little"), salts[2]) == admit_check.hc_null_hash((k + ELL).to_bytes(32, "little"), salts[2])
    # the key is read byte by byte where it is not 4-byte aligned (a record field at an odd offset)
    buf = C.create_string_buffer(b"\x5a" + k.to_bytes(32, "little") + b"\x5a")
    unaligned = C.cast(C.addressof(buf) + 1, C.c_char_p)
    assert admit_check.hc_null_hash(unaligned, salts[2]) == nm.key_hash(k, salts[2])
    assert checked >= (7 + 40) * 3


def test_every_bit_of_the_salt_and_of_the_key_reaches_the_hash(admit_check):
    """a hash that drops a word of the key or half of the salt passes every set-against-set test; here each of the 128 + 253 input
    bits, flipped alone, changes the result -- and changes it to what the model says"""
    r = random.Random(77)
    for trial in range(4):
        salt = bytes(r.randrange(256) for _ in range(16))
        k = r.randrange(2**252) if trial else 0
        base = admit_check.hc_null_hash(k.to_bytes(32, "little"), salt)
        assert base == nm.key_hash(k, salt)
        s = int.from_bytes(salt, "little")
        for bit in range(128):
            s2 = (s ^ 1 << bit).to_bytes(16, "little")
            got = admit_check.hc_null_hash(k.to_bytes(32, "little"), s2)
            assert got != base and got == nm.key_hash(k, s2), ("salt bit", bit)
        for bit in range(253):
            k2 = k ^ 1 << bit
            if k2 >= ELL:                   # bit 252 on top of a random key: not a reduced key (the key 0 of the first pass takes that bit)
                continue
            got = admit_check.hc_null_hash(k2.to_bytes(32, "little"), salt)
            assert got != base and got == nm.key_hash(k2, salt), ("key bit", bit)
    # bit 252 on its own: 2^252 is a reduced key (l is a little larger)
    assert admit_check.hc_null_hash((1 << 252).to_bytes(32, "little"), bytes(16)) == nm.key_hash(1 << 252, bytes(16)) != nm.key_hash(0, bytes(16))


def test_the_host_screen_walks_an_aimed_chain_through_the_wrap(admit_check):
    """70 keys aimed at slot cap - 3 of a 1024-slot table fill cap - 3 .. cap - 1 and 0 .. 66: longer than a wavefront, through the
    wrap.  The screen answers 3 for exactly those 70; 70 more keys aimed at the same slot, never inserted, walk the whole chain and
    stop at the empty slot behind it."""
    cap, salt = 1024, bytes(range(16, 32))
    aimed = nm.aim(salt, cap, cap - 3, 140, rng_seed=9)
    chain, absent = aimed[:70], aimed[70:]
    tk, ts = (C.c_uint32 * (cap * 8))(), (C.c_uint32 * cap)()
    model = nm.LinearTable(cap, salt)
    for k in chain:
        assert admit_check.hc_admit_table_insert(tk, ts, cap, salt, k.to_bytes(32, "little"), 7) == 1
        model.insert(k)
    want_slots = {(cap - 3 + i) % cap for i in range(70)}
    assert model.occupied() == want_slots
    assert {t for t in range(cap) if ts[t]} == want_slots and all(ts[t] == (7 << 8 | 2) for t in want_slots)
    # the host table holds key i at the slot the sequential model gives it
    for k in chain:
        t = model.slot[k]
        assert bytes(np.frombuffer(tk, np.uint32)[8 * t:8 * t + 8].tobytes()) == k.to_bytes(32, "little")
    r = random.Random(5)
    lanes = [(k, True) for k in chain] + [(k, False) for k in absent]
    order = list(range(140)); r.shuffle(order)
    for spelled in (False, True):
        vals = [lanes[i][0] + (ELL if spelled and i % 8 == 0 else 0) for i in range(140)]
        for perm in (list(range(140)), order):
            blob = b"".join(vals[i].to_bytes(32, "little") for i in perm) + b"\0"
            pre = C.create_string_buffer(b"\x55" * 141); kred = C.create_string_buffer(32 * 140 + 1)
            admit_check.hc_admit_screen(140, 32, blob, None, None, tk, ts, cap, salt, pre, kred)
            assert list(pre.raw[:140]) == [3 if lanes[i][1] else 0 for i in perm] and pre.raw[140:141] == b"\x55"
            assert kred.raw[:32 * 140] == b"".join(lanes[i][0].to_bytes(32, "little") for i in perm)
    # the first 70 lanes in lane order, as the issue states it
    blob = b"".join(k.to_bytes(32, "little") for k, _ in lanes) + b"\0"
    admit_check.hc_admit_screen(140, 32, blob, None, None, tk, ts, cap, salt, pre, kred)
    assert pre.raw[:70] == b"\x03" * 70 and pre.raw[70:140] == bytes(70)
