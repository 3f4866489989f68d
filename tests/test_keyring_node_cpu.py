"""Key rotation over a node without a device: csrc/node.cpp + csrc/node_keyring.cpp linked against the TEST-ONLY stand-ins of
tests/node_mock (node_mock.cpp + node_mock_keyring.cpp).  out_key, statuses and outputs must land at the right offsets whatever the
number of devices, ACT_RNG_SEQUENTIAL must stay exact across pieces, and a failing generator must sign nothing.  The same dispatcher
over real contexts is tests/test_gpu_keyring.py."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT
from test_node_dispatch_cpu import PB, _Replay, make_node, records

ML, RL = PB + 3, 129


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("node_mock_keyring") / "libnode_mock_keyring.so")
    csrc = os.path.join(ROOT, "anonymous-credit-tokens_amd", "csrc")
    mock = os.path.join(ROOT, "tests", "node_mock")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-pthread", "-o", out, os.path.join(csrc, "node.cpp"),
                    os.path.join(csrc, "node_keyring.cpp"), os.path.join(mock, "node_mock.cpp"), os.path.join(mock, "node_mock_keyring.cpp")], check=True)
    l = C.CDLL(out)
    l.act_node_ctx.restype = C.c_void_p
    l.act_node_ctx.argtypes = [C.c_void_p, C.c_int]
    l.act_mock_lanes.restype = C.c_size_t
    l.act_mock_lanes.argtypes = [C.c_void_p]
    l.act_node_nullifier_set_len.restype = C.c_size_t
    return l


def ring(nkeys):
    return b"".join(bytes([0x40 + k]) + bytes(63) for k in range(nkeys))


def bufs(n, *recs):
    return [C.create_string_buffer(max(1, r * n)) for r in recs]


def expect_signed(recs, keys, kidx, status_in, rng, mode, nkeys):
    """the mock's refund of every lane, slices handed out as the sequential loop would"""
    n = len(status_in); out, st, cur = [], [], 0
    for i in range(n):
        s = status_in[i]
        if s == 0 and kidx[i] >= nkeys:
            s = 255
        st.append(s)
        if s:
            out.append(bytes(128)); continue
        slot = i if mode == 0 else cur
        cur += 1
        out.append(recs[PB * i:PB * i + 8] + rng[128 * slot:128 * slot + 100] + bytes(18) + bytes([keys[64 * kidx[i]], kidx[i]]))
    return bytes(st), b"".join(out), cur


@pytest.mark.parametrize("ndev", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [0, 1, 5, 23, 1000])
def test_ring_calls_land_at_the_right_offsets(lib, ndev, n):
    nd = make_node(lib, ndev)
    nkeys = 1 + (n + ndev) % 4
    keys = ring(nkeys)
    proofs = records(n, PB, 31 * ndev + n)
    rng = records(n, 128, 9)
    verdict = bytes(7 if proofs[PB * i] & 1 else 0 for i in range(n))
    match = bytes(255 if verdict[i] else proofs[PB * i + 8] % nkeys for i in range(n))
    st, ok, kp = bufs(n, 1, 1, 32)
    assert lib.act_node_verify_spend_keyring_batch(nd, C.c_size_t(n), keys, nkeys, proofs, st, ok, kp) == 0
    assert st.raw[:n] == verdict and ok.raw[:n] == match
    for i in range(n):
        assert kp.raw[32 * i:32 * i + 8] == (bytes(8) if verdict[i] else proofs[PB * i:PB * i + 8])
    # the sign half with an index per lane, every seventh one outside the ring: not signed, no slice consumed
    kidx = bytes(200 if i % 7 == 3 else (i * 5) % nkeys for i in range(n))
    for mode in (0, 1):
        out, st2 = bufs(n, 128, 1)
        assert lib.act_node_refund_sign_keyring_batch(nd, C.c_size_t(n), keys, nkeys, kidx, kp.raw, verdict, rng + b"\0", mode, out, st2) == 0
        want = expect_signed(proofs, keys, kidx, verdict, rng, mode, nkeys)
        assert (st2.raw[:n], out.raw[:128 * n]) == want[:2], mode
    # redeem: records and wire bytes, matched key and a named key, the generator itself
    devs = (C.c_int * 2)(0, 1)
    msgs = b"".join(b"\xa1\x01\x58" + proofs[PB * i:PB * (i + 1)] for i in range(n))
    for wire in (False, True):
        for sign_key in (-1, nkeys - 1):
            ns = C.c_void_p()
            assert lib.act_node_nullifier_set_create(devs, 2, C.c_size_t(10 * n + 16), None, C.byref(ns)) == 0
            kidx = bytes(sign_key if sign_key >= 0 else (match[i] if match[i] != 255 else 0) for i in range(n))
            want = expect_signed(proofs, keys, kidx, verdict, rng, 1, nkeys)
            g = _Replay(rng[:128 * want[2]])
            rec = RL if wire else 128
            out, st3, ok3 = bufs(n, rec, 1, 1)
            if wire:
                rc = lib.act_node_redeem_cbor_keyring_batch(nd, ns, C.c_size_t(n), keys, nkeys, sign_key, msgs + b"\0", None, g.ptr, 2, out, st3, ok3)
            else:
                rc = lib.act_node_redeem_keyring_batch(nd, ns, C.c_size_t(n), keys, nkeys, sign_key, proofs + b"\0", g.ptr, 2, out, st3, ok3)
            assert rc == 0 and st3.raw[:n] == want[0] and ok3.raw[:n] == match
            assert g.draws == ([128 * want[2]] if want[2] else [])
            for i in range(n):
                got = out.raw[rec * i:rec * (i + 1)]
                w = want[1][128 * i:128 * i + 128]
                assert got == ((b"\xa4" + w if want[0][i] == 0 else bytes(RL)) if wire else w), (wire, sign_key, i)
            assert lib.act_node_nullifier_set_len(ns) == want[2]
            # everything again: every accepted lane is a double spend now, keeps the index it matched, nothing is drawn
            g2 = _Replay(rng)
            if wire:
                rc = lib.act_node_redeem_cbor_keyring_batch(nd, ns, C.c_size_t(n), keys, nkeys, sign_key, msgs + b"\0", None, g2.ptr, 2, out, st3, ok3)
            else:
                rc = lib.act_node_redeem_keyring_batch(nd, ns, C.c_size_t(n), keys, nkeys, sign_key, proofs + b"\0", g2.ptr, 2, out, st3, ok3)
            assert rc == 0 and st3.raw[:n] == bytes(3 if v == 0 else v for v in verdict) and ok3.raw[:n] == match
            assert out.raw[:rec * n] == bytes(rec * n) and g2.draws == []
            lib.act_node_nullifier_set_destroy(ns)
    if n >= ndev:
        lanes = [lib.act_mock_lanes(lib.act_node_ctx(nd, k)) for k in range(ndev)]
        assert min(lanes) > 0
    lib.act_node_destroy(nd)


def test_ring_arguments_and_malformed_messages(lib):
    nd = make_node(lib, 3)
    n = 40
    proofs = records(n, PB, 5)
    st, ok, kp = bufs(n, 1, 1, 32)
    for keys, nkeys in ((ring(1), 0), (ring(4), 5), (None, 2)):
        assert lib.act_node_verify_spend_keyring_batch(nd, C.c_size_t(n), keys, nkeys, proofs, st, ok, kp) == 1
        assert lib.act_node_verify_spend_keyring_batch(nd, C.c_size_t(0), keys, nkeys, proofs, st, ok, kp) == 1
    devs = (C.c_int * 2)(0, 1)
    ns = C.c_void_p()
    assert lib.act_node_nullifier_set_create(devs, 2, C.c_size_t(1000), None, C.byref(ns)) == 0
    out, st3, ok3 = bufs(n, 128, 1, 1)
    for sign_key in (-2, 2, 7):
        assert lib.act_node_redeem_keyring_batch(nd, ns, C.c_size_t(n), ring(2), 2, sign_key, proofs, records(n, 128, 1), 1, out, st3, ok3) == 1
    assert lib.act_node_nullifier_set_len(ns) == 0
    # wire: messages of several lengths at absolute offsets, every fifth one malformed -> from_cbor's status, no key, no nullifier, no slice
    body = [(b"\xff" if i % 5 == 2 else b"\xa1") + b"\x01\x58" + proofs[PB * i:PB * (i + 1)] + bytes(i % 3) for i in range(n)]
    offs = (C.c_uint64 * (n + 1))(); pos = 0
    for i, m in enumerate(body):
        offs[i] = pos; pos += len(m)
    offs[n] = pos
    keys = ring(3)
    verdict = bytes(254 if i % 5 == 2 else (7 if proofs[PB * i] & 1 else 0) for i in range(n))
    match = bytes(255 if verdict[i] else proofs[PB * i + 8] % 3 for i in range(n))
    rng = records(n, 128, 2)
    want = expect_signed(proofs, keys, bytes(m if m != 255 else 0 for m in match), verdict, rng, 1, 3)
    out, st4, ok4 = bufs(n, RL, 1, 1)
    assert lib.act_node_redeem_cbor_keyring_batch(nd, ns, C.c_size_t(n), keys, 3, -1, b"".join(body) + b"\0", offs, rng, 1, out, st4, ok4) == 0
    assert st4.raw[:n] == want[0] and ok4.raw[:n] == match and lib.act_node_nullifier_set_len(ns) == want[2]
    for i in range(n):
        assert out.raw[RL * i:RL * (i + 1)] == (b"\xa4" + want[1][128 * i:128 * i + 128] if want[0][i] == 0 else bytes(RL))
    lib.act_node_nullifier_set_destroy(ns)
    lib.act_node_destroy(nd)


def test_a_failing_generator_or_gpu_signs_nothing(lib):
    nd = make_node(lib, 3)
    n = 50
    keys = ring(2)
    proofs = records(n, PB, 77)
    verdict = bytes(7 if proofs[PB * i] & 1 else 0 for i in range(n))
    match = bytes(255 if verdict[i] else proofs[PB * i + 8] % 2 for i in range(n))
    acc = verdict.count(0)
    devs = (C.c_int * 2)(0, 1)
    ns = C.c_void_p()
    assert lib.act_node_nullifier_set_create(devs, 2, C.c_size_t(1000), None, C.byref(ns)) == 0
    short = _Replay(records(n, 128, 5)[:128 * acc - 1])            # one byte too few: draw() returns 1 and writes nothing
    out, st, ok = bufs(n, 128, 1, 1)
    assert lib.act_node_redeem_keyring_batch(nd, ns, C.c_size_t(n), keys, 2, -1, proofs, short.ptr, 2, out, st, ok) == 5
    assert short.draws == [] and out.raw[:128 * n] == bytes(128 * n)
    assert st.raw[:n] == bytes(251 if v == 0 else v for v in verdict) and ok.raw[:n] == match      # recorded, unsigned: the refund is owed
    assert lib.act_node_nullifier_set_len(ns) == acc
    lib.act_node_nullifier_set_destroy(ns)
    # one GPU fails while signing: the lanes of ITS pieces that were to be signed are recorded-unsigned, all others are finished
    ns = C.c_void_p()
    assert lib.act_node_nullifier_set_create(devs, 2, C.c_size_t(1000), None, C.byref(ns)) == 0
    lib.act_mock_keyring_fail(1)
    rng = records(n, 128, 6)
    rc = lib.act_node_redeem_keyring_batch(nd, ns, C.c_size_t(n), keys, 2, -1, proofs, rng, 0, out, st, ok)
    lib.act_mock_keyring_fail(-1)
    assert rc == 2 and ok.raw[:n] == match
    unsigned = [i for i in range(n) if st.raw[i] == 251]
    assert unsigned and all(verdict[i] == 0 and out.raw[128 * i:128 * i + 128] == bytes(128) for i in unsigned)
    done = [i for i in range(n) if st.raw[i] == 0]
    assert done and all(out.raw[128 * i:128 * i + 8] == proofs[PB * i:PB * i + 8] and out.raw[128 * i + 127] == match[i] for i in done)
    assert sorted(unsigned + done) == [i for i in range(n) if verdict[i] == 0]
    lib.act_node_nullifier_set_destroy(ns)
    lib.act_node_destroy(nd)


@pytest.mark.parametrize("fault", ["nullifier device", "signing device", "generator"])
def test_one_key_and_a_ring_of_one_finish_a_failed_redemption_alike(lib, fault):
    """The steps behind verification are the same for act_node_redeem_batch and act_node_redeem_keyring_batch: under the same fault,
    on fresh sets, the two calls agree on every status byte, on which output slots are all zero, on the set's length and on whether
    the call failed.  (n = 40 with a stream generator: the general path of the one-key call, not its road for a few items.)"""
    ndev, n, bad = 3, 40, 1
    nd = make_node(lib, ndev)
    devs = (C.c_int * ndev)(*range(ndev))
    proofs = bytearray(records(n, PB, 123))
    for i in range(n):                                             # the mocks reject an odd first byte: every third lane
        proofs[PB * i] = (proofs[PB * i] & 0xfe) | (i % 3 == 1)
    proofs = bytes(proofs)
    verdict = bytes(7 if i % 3 == 1 else 0 for i in range(n))
    acc = verdict.count(0)
    rng = records(n, 128, 124)
    keys = ring(1)
    got = {}
    for form in ("one key", "ring"):
        ns = C.c_void_p()
        assert lib.act_node_nullifier_set_create(devs, ndev, C.c_size_t(1000), b"0123456789abcdef", C.byref(ns)) == 0
        short = _Replay(rng[:128 * acc - 1])                       # one byte too few: draw() returns non-zero and writes nothing
        src, mode = (short.ptr, 2) if fault == "generator" else (rng, 1)
        lib.act_mock_fail(bad if fault == "nullifier device" else -1, bad if fault == "signing device" else -1)
        lib.act_mock_keyring_fail(bad if fault == "signing device" else -1)
        out, st, ok = bufs(n, 128, 1, 1)
        if form == "one key":
            rc = lib.act_node_redeem_batch(nd, ns, C.c_size_t(n), bytes(64), proofs, src, mode, out, st)
        else:
            rc = lib.act_node_redeem_keyring_batch(nd, ns, C.c_size_t(n), keys, 1, -1, proofs, src, mode, out, st, ok)
            assert ok.raw[:n] == bytes(255 if v else 0 for v in verdict)
        lib.act_mock_fail(-1, -1)
        lib.act_mock_keyring_fail(-1)
        status, refunds = st.raw[:n], [out.raw[128 * i:128 * (i + 1)] for i in range(n)]
        # every signed lane against its own mock's rule, every other slot all zero.  The slices are the sequential loop's: a lane that
        # was to be signed has its slice whether or not its device then failed (251), a lane the store could not answer has none (252)
        checked = bytes(0 if s == 251 else s for s in status)
        want = expect_signed(proofs, keys, bytes(n), checked, rng, 1, 1)
        cur = 0
        for i in range(n):
            if status[i]:
                assert refunds[i] == bytes(128), (form, i)
            elif form == "ring":
                assert refunds[i] == want[1][128 * i:128 * (i + 1)], (form, i)
            else:
                assert refunds[i][:8] == proofs[PB * i:PB * i + 8] and refunds[i][8:16] == rng[128 * cur:128 * cur + 8], (form, i)
            cur += checked[i] == 0
        assert short.draws == []
        got[form] = (status, [r == bytes(128) for r in refunds], lib.act_node_nullifier_set_len(ns), rc != 0)
        lib.act_node_nullifier_set_destroy(ns)
    lib.act_node_destroy(nd)
    assert got["one key"] == got["ring"]
    status, _, recorded, failed = got["ring"]
    assert failed and all(status[i] == 7 for i in range(n) if verdict[i])
    accepted = [status[i] for i in range(n) if verdict[i] == 0]
    if fault == "nullifier device":        # the lost device's lanes are undetermined and not recorded, every other lane is finished
        assert set(accepted) == {0, 252} and recorded == accepted.count(0)
    elif fault == "signing device":        # the accepted lanes of the failed device's piece are recorded and unsigned
        a, b = n * bad // ndev, n * (bad + 1) // ndev
        assert status == bytes(v if v else (251 if a <= i < b else 0) for i, v in enumerate(verdict)) and recorded == acc
    else:                                  # nothing was drawn: every accepted lane is recorded and unsigned
        assert status == bytes(v if v else 251 for v in verdict) and recorded == acc
