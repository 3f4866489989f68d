"""Replayable partial refunds on the CPU: the lane bodies of csrc/return_replay_lanes.h compiled for the host by
tests/hostcheck/return_replay_check.cpp -- the receipt tag and the derived nonce with the lane's returned amount, the candidate's tag
of the admission stage -- against the definitions of include/act_mi355x.h recomputed with oracle/pymodel.blake3
(tests/return_replay_cases.py).  The same bodies run on the GPU in tests/test_gpu_return_replay.py."""
import ctypes as C
import os
import re
import subprocess

import pytest

import admit_replay_cases as ar
import replay_cases as rp
import return_replay_cases as rr
from conftest import ELL, ROOT, shake

S = 5                                                           # the charge the amounts below are drawn around
AMOUNTS = [0, 1, S, ELL - 1, 1 + ELL, ELL, S + ELL, 2]          # t = 0, 1, s, l - 1; t + l given unreduced; t = l (that is t^ = 0)


@pytest.fixture(scope="module")
def check():
    return C.CDLL(rr.build_check(os.path.join(ROOT, "tests", "hostcheck", "libreturn_replay_check.so")))


def le(v):
    return v.to_bytes(32, "little")


def odd(b):
    """the same bytes at an odd address -> (pointer, keep-alive)"""
    buf = C.create_string_buffer(len(b) + 1)
    C.memmove(C.addressof(buf) + 1, b, len(b))
    return C.c_void_p(C.addressof(buf) + 1), buf


def derive(lib, nul, kp, st, kidx, keys, nonce_key, t, stride=32, v1=0, shifted=False):
    n = len(st)
    tags, non = C.create_string_buffer(32 * n + 1), C.create_string_buffer(128 * n + 1)
    off = 1 if shifted else 0
    keep = []
    def arg(b):
        if b is None or not shifted:
            return b
        p, k = odd(b); keep.append(k)
        return p
    pt, pn = C.c_void_p(C.addressof(tags) + off), C.c_void_p(C.addressof(non) + off)
    lib.hc_rr_tags(n, stride, arg(nul), arg(kp), st, None, 0, arg(t), v1, pt)
    lib.hc_rr_nonces(n, stride, arg(nul), arg(kp), st, kidx, b"".join(keys), len(keys), nonce_key, arg(t), v1, pn)
    return tags.raw[off:off + 32 * n], non.raw[off:off + 128 * n]


@pytest.mark.parametrize("shifted", [False, True], ids=["aligned", "odd addresses"])
def test_tags_and_nonces_against_blake3(check, shifted):
    n = 67                                                      # one past a wavefront, some lanes rejected, some without a ring key
    nul, kp, nonce_key = shake("rr-k", 32 * n), shake("rr-kp", 32 * n), shake("rr-nk", 32)
    keys = [shake("rr-key%d" % j, 64) for j in range(3)]
    st = bytes(7 if i % 5 == 3 else 0 for i in range(n))
    kidx = bytes(255 if i % 7 == 6 else i % 3 for i in range(n))
    ts = [AMOUNTS[i % len(AMOUNTS)] for i in range(n)]
    t = b"".join(le(v) for v in ts)
    tags, non = derive(check, nul, kp, st, kidx, keys, nonce_key, t, shifted=shifted)
    old_tags, old_non = derive(check, nul, kp, st, kidx, keys, nonce_key, None, v1=1, shifted=shifted)
    for i in range(n):
        k, p = nul[32 * i:32 * i + 32], kp[32 * i:32 * i + 32]
        g, x = tags[32 * i:32 * i + 32], non[128 * i:128 * i + 128]
        if st[i]:
            assert g == bytes(32) and x == bytes(128), i       # dead lanes give zeros
            continue
        assert g == rr.tag(k, p, ts[i]) and g[31] & 0xF0 == 0, i
        assert x == (rr.nonce(nonce_key, keys[kidx[i]], k, p, ts[i]) if kidx[i] < 3 else bytes(128)), i
        if ts[i] % ELL == 0:                                    # t = 0 and t = l: the v1 functions byte for byte
            assert g == old_tags[32 * i:32 * i + 32] == rp.tag(k, p) and x == old_non[128 * i:128 * i + 128], i
        else:
            assert g == rr.tag_t(k, p, ts[i] % ELL) != rp.tag(k, p), i
    # no amounts at all is every amount zero
    assert derive(check, nul, kp, st, kidx, keys, nonce_key, None, shifted=shifted) == (old_tags, old_non)


def test_the_messages_have_the_stated_lengths_and_t_plus_l_is_t(check):
    import pymodel
    nul, kp, nonce_key, key = shake("rr-h-k", 32), shake("rr-h-kp", 32), shake("rr-h-nk", 32), shake("rr-h-key", 64)
    for t in (1, S, ELL - 1):
        a = derive(check, nul, kp, b"\0", b"\0", [key], nonce_key, le(t))
        b = derive(check, nul, kp, b"\0", b"\0", [key], nonce_key, le(t + ELL)) if t + ELL < 2**256 else a
        msg = rr.LABEL_NONCE_T + nonce_key + key + rp.reduced(nul) + kp + le(t)
        assert len(msg) == 224 and len(rr.LABEL_TAG_T + rp.reduced(nul) + kp + le(t)) == 128
        assert a == b and a[1] == pymodel.blake3(msg, 128) and a[1][:64] == pymodel.blake3(msg, 64) and a[1][:64] != a[1][64:]
    # for one (key, k, K') the amounts 0, 1, 2, s give four different tags, and nonces that differ in every 32-byte quarter
    outs = [derive(check, nul, kp, b"\0", b"\0", [key], nonce_key, le(t)) for t in (0, 1, 2, S)]
    assert len({o[0] for o in outs}) == 4
    for q in range(4):
        assert len({o[1][32 * q:32 * q + 32] for o in outs}) == 4, q


def test_compressions_per_lane_are_counted_not_assumed(check):
    """2 for either tag, 4 for the v1 nonces and 5 for nonce_t; the hashes add no field operation"""
    c = (C.c_uint64 * 3)()
    for t, want in ((0, (2, 4)), (ELL, (2, 4)), (1, (2, 5)), (S, (2, 5)), (ELL - 1, (2, 5)), (1 + ELL, (2, 5))):
        check.hc_rr_lane_counts(le(t), c)
        assert (c[0], c[1]) == want and c[2] == 0, (t, list(c))


@pytest.mark.parametrize("L,n", [(3, 1), (8, 5), (8, 65)])
def test_the_candidate_tag_lane_over_a_gathered_index(check, L, n):
    """candidate c's nullifier AND amount lie at idx[c] of the call's arrays; enc(K') by oracle/pymodel; the amount changes the tag and
    nothing else, at the cost of no field operation beyond the lane without amounts"""
    import pymodel
    pb = 32 * (14 + 4 * L)
    recs = bytearray(shake("rr-kp-recs%d" % L, pb * n))
    for c in range(n):
        for j in range(L):
            recs[c * pb + 32 * (4 + j):c * pb + 32 * (5 + j)] = pymodel.ristretto_encode(pymodel.pt_mul(pymodel.G, 3 + 5 * c + j))
    bad = n // 2 if n > 1 else None
    if bad is not None:
        recs[bad * pb + 32 * 4:bad * pb + 32 * 5] = b"\xff" * 32
    recs = bytes(recs)
    m = 2 * n + 1
    kred = b"".join(le(int.from_bytes(shake("rr-kred%d" % i, 32), "little") % ELL) for i in range(m))
    ts = [AMOUNTS[(i * 3 + 1) % len(AMOUNTS)] for i in range(m)]
    idx = (C.c_uint32 * n)(*[2 * c + 1 for c in range(n)])
    pt, keep = odd(b"".join(le(v) for v in ts))
    for with_t in (True, False):
        kp, tag, mark = C.create_string_buffer(32 * n), C.create_string_buffer(32 * n), C.create_string_buffer(n)
        counts = (C.c_uint64 * 4)()
        assert check.hc_rr_kprime(L, n, recs, kred, idx, pt if with_t else None, kp, tag, mark, counts) == 1
        good = n - (1 if bad is not None else 0)
        assert counts[0] == counts[2] and counts[1] == counts[3] == 2 * good
        for c in range(n):
            if c == bad:
                assert mark.raw[c] == 1 and kp.raw[32 * c:32 * c + 32] == bytes(32) == tag.raw[32 * c:32 * c + 32]
                continue
            want_kp = ar.kprime(recs[c * pb:(c + 1) * pb], L)
            assert mark.raw[c] == 0 and kp.raw[32 * c:32 * c + 32] == want_kp
            i = 2 * c + 1
            assert tag.raw[32 * c:32 * c + 32] == rr.tag(kred[32 * i:32 * i + 32], want_kp, ts[i] if with_t else 0), (c, with_t)


def test_the_model_against_hand_written_lanes():
    rr.check_model()


def test_counts_and_prototypes_in_the_header_the_bindings_and_the_rust_block():
    hd = open(os.path.join(ROOT, "include", "act_mi355x.h")).read()
    rs = open(os.path.join(ROOT, "rust", "src", "mi355x.rs")).read()
    assert re.search(r"#define ACT_RETURN_REPLAY_COUNTS 12\b", hd)
    from act_amd import capi
    assert tuple(capi.RETURN_REPLAY_COUNTS) == rr.COUNTS and len(rr.COUNTS) == 12 and rr.COUNTS[:11] == tuple(capi.ADMIT_REPLAY_COUNTS)
    for name in ("act_redeem_return_replay_batch", "act_redeem_cbor_return_replay_batch", "act_replay_derive_return_batch"):
        assert name in capi.EXPORTS and re.search(r"\bint %s\(" % name, hd) and re.search(r"\bfn %s\(" % name, rs), name
    assert rr.LABEL_TAG_T.rstrip(b"\0").decode() in hd and rr.LABEL_NONCE_T.rstrip(b"\0").decode() in hd
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "Not offered: the replay forms" not in design


def test_lane_bodies_as_a_sanitized_stand_alone_program(tmp_path):
    """return_replay_check.cpp with its own main under AddressSanitizer and UBSan: exact-size heap arrays at odd offsets, the grid's tail
    lanes, n = 1, 65 and 257, against blake3_hd.h's general hash over the assembled message; nothing is preloaded"""
    exe = rr.build_program(str(tmp_path / "return_replay_check_asan"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "RETURN REPLAY CHECK CLEAN" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-6000:]
