"""Replayable redemption on the CPU: the lane bodies of the replay kernels (csrc/replay_lanes.h) compiled for the host by
tests/hostcheck/replay_check.cpp -- the receipt tag, the derived refund nonce, the resolve step -- against the definitions of
include/act_mi355x.h recomputed with oracle/pymodel.blake3 (tests/replay_cases.py).  The same bodies run on the GPU in
tests/test_gpu_replay.py."""
import ctypes as C
import itertools
import os
import re
import subprocess

import pytest

import replay_cases as rp
from conftest import ELL, ROOT, shake


@pytest.fixture(scope="module")
def replay_check():
    return C.CDLL(rp.build_replay_check(os.path.join(ROOT, "tests", "hostcheck", "libreplay_check.so")))


def derive(rc, nul, kp, st, kidx, keys, nonce_key, stride=32):
    n = len(st)
    tags, non = C.create_string_buffer(32 * n), C.create_string_buffer(128 * n)
    rc.hc_replay_tags(n, stride, nul, kp, st, None, 0, tags)
    rc.hc_replay_nonces(n, stride, nul, kp, st, kidx, b"".join(keys), len(keys), nonce_key, non)
    return tags.raw, non.raw


INPUTS = [("random", None), ("zeros", 0x00), ("ones", 0xFF)]


@pytest.mark.parametrize("name,fill", INPUTS)
def test_tags_and_nonces_against_blake3(replay_check, name, fill):
    n = 67                                                      # one past a wavefront, some lanes rejected, some without a ring key
    gen = (lambda label, m: shake("replay-" + label, m)) if fill is None else (lambda label, m: bytes([fill]) * m)
    nul, kp, nonce_key = gen("k", 32 * n), gen("kp", 32 * n), gen("nk", 32)
    keys = [gen("key%d" % j, 64) for j in range(3)]
    st = bytes(7 if i % 5 == 3 else 0 for i in range(n))
    kidx = bytes(255 if i % 7 == 6 else i % 3 for i in range(n))
    tags, non = derive(replay_check, nul, kp, st, kidx, keys, nonce_key)
    for i in range(n):
        k, p = nul[32 * i:32 * i + 32], kp[32 * i:32 * i + 32]
        t, x = tags[32 * i:32 * i + 32], non[128 * i:128 * i + 128]
        if st[i]:
            assert t == bytes(32) and x == bytes(128), i
            continue
        assert t == rp.tag(k, p) and t[31] & 0xF0 == 0, i
        assert int.from_bytes(t, "little") < 2**252 < ELL       # the receipts set's own reduction is the identity
        assert x == (rp.nonce(nonce_key, keys[kidx[i]], k, p) if kidx[i] < 3 else bytes(128)), i


def test_the_nonce_halves_are_xof_blocks_0_and_1(replay_check):
    nul, kp, nonce_key, key = shake("h-k", 32), shake("h-kp", 32), shake("h-nk", 32), shake("h-key", 64)
    _, non = derive(replay_check, nul, kp, b"\0", b"\0", [key], nonce_key)
    import pymodel
    msg = rp.LABEL_NONCE + nonce_key + key + rp.reduced(nul) + kp
    assert len(msg) == 192 and len(rp.LABEL_TAG + rp.reduced(nul) + kp) == 96
    assert non[:64] == pymodel.blake3(msg, 64) and non == pymodel.blake3(msg, 128) and non[:64] != non[64:]


def test_k_and_k_plus_l_are_one_nullifier(replay_check):
    k = int.from_bytes(shake("red-k", 32), "little") % 2**252
    kp, nonce_key, key = shake("red-kp", 32), shake("red-nk", 32), shake("red-key", 64)
    a = derive(replay_check, k.to_bytes(32, "little"), kp, b"\0", b"\0", [key], nonce_key)
    b = derive(replay_check, (k + ELL).to_bytes(32, "little"), kp, b"\0", b"\0", [key], nonce_key)
    assert a == b and a[0] == rp.tag((k % ELL).to_bytes(32, "little"), kp)
    # each input matters: another K', another signing key, another nonce key
    other_kp = bytes([kp[0] ^ 1]) + kp[1:]
    c = derive(replay_check, k.to_bytes(32, "little"), other_kp, b"\0", b"\0", [key], nonce_key)
    assert c[0] != a[0] and c[1] != a[1]
    d = derive(replay_check, k.to_bytes(32, "little"), kp, b"\0", b"\1", [key, shake("red-key2", 64)], nonce_key)
    assert d[0] == a[0] and d[1] != a[1]                        # the tag does not depend on the key the lane is signed with
    e = derive(replay_check, k.to_bytes(32, "little"), kp, b"\0", b"\0", [key], shake("red-nk2", 32))
    assert e[0] == a[0] and e[1] != a[1]


def test_strided_nullifiers_as_in_a_record(replay_check):
    """records form: k is the first field of a SpendProof record, the lanes a record apart"""
    n, stride = 5, 32 * 46
    blob = shake("stride", stride * (n - 1) + 32)
    kp, nonce_key, key = shake("stride-kp", 32 * n), shake("stride-nk", 32), shake("stride-key", 64)
    tags, non = derive(replay_check, blob, kp, bytes(n), bytes(n), [key], nonce_key, stride=stride)
    for i in range(n):
        k = blob[stride * i:stride * i + 32]
        assert tags[32 * i:32 * i + 32] == rp.tag(k, kp[32 * i:32 * i + 32])
        assert non[128 * i:128 * i + 128] == rp.nonce(nonce_key, key, k, kp[32 * i:32 * i + 32])


def test_resolve_truth_table(replay_check):
    out = C.create_string_buffer(3)
    for verdict, spent, found in itertools.product((0, 1, 6, 7, 253, 254, 255), (0, 1, 2), (0, 1)):
        replay_check.hc_replay_resolve(verdict, spent, found, out)
        skip, sp, replayed = out.raw
        ok = verdict == 0
        assert skip == (0 if ok and spent == 0 else 1)          # a receipt only where k was fresh: a double spender plants nothing
        assert replayed == (1 if ok and spent == 1 and found else 0)
        want_sp = 0 if not ok or spent == 0 or replayed else spent
        assert sp == want_sp, (verdict, spent, found)
    # over lanes, in the two passes of the call: skip[] in front of the receipts insert, sp[] and replayed[] behind the look-up
    n = 257
    st = bytes(7 if i % 4 == 1 else 0 for i in range(n)); spent = bytes(i % 3 for i in range(n)); found = bytes((i // 3) % 2 for i in range(n))
    skip, sp, rep = (C.create_string_buffer(b"\x09" * n, n) for _ in range(3))
    replay_check.hc_replay_resolve_lanes(n, st, spent, None, skip, sp, rep)
    assert sp.raw == b"\x09" * n and rep.raw == b"\x09" * n
    assert skip.raw == bytes(0 if st[i] == 0 and spent[i] == 0 else 1 for i in range(n))
    replay_check.hc_replay_resolve_lanes(n, st, spent, found, skip, sp, rep)
    for i in range(n):
        replay_check.hc_replay_resolve(st[i], spent[i], found[i], out)
        assert (sp.raw[i], rep.raw[i]) == (out.raw[1], out.raw[2]), i


def test_the_model_against_hand_written_lanes():
    rp.check_model()


def test_counts_and_prototypes_in_the_header():
    hd = open(os.path.join(ROOT, "include", "act_mi355x.h")).read()
    assert re.search(r"#define ACT_REPLAY_COUNTS 6\b", hd)
    from act_amd import capi
    assert tuple(capi.REPLAY_COUNTS) == rp.COUNTS and len(rp.COUNTS) == 6
    for name in ("act_redeem_replay_batch", "act_redeem_cbor_replay_batch", "act_replay_derive_batch"):
        assert name in capi.EXPORTS and re.search(r"\bint %s\(" % name, hd)
    assert rp.LABEL_TAG.rstrip(b"\0").decode() in hd and rp.LABEL_NONCE.rstrip(b"\0").decode() in hd


def test_lane_bodies_as_a_sanitized_stand_alone_program(tmp_path):
    """replay_check.cpp with its own main under AddressSanitizer and UBSan: exact-size heap arrays at odd offsets, the grid's tail lanes,
    n = 1, 65 and 257, against blake3_hd.h's general hash over the assembled message"""
    exe = rp.build_replay_program(str(tmp_path / "replay_check_asan"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "REPLAY CHECK CLEAN" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-6000:]
