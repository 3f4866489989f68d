"""Key rotation and partial refunds together, on the CPU: the ring form of the client's RefundReturn check
(csrc/client_ring_return_lanes.h, with the candidate and hash lanes of csrc/client_ring_lanes.h at the 160-byte stride) compiled for
the host by tests/hostcheck/return_ring_check.cpp and judged by the model of tests/return_ring_cases.py; the model of the return calls'
unique forms against the model of the plain return loop.  The same bodies run on the GPU in tests/test_gpu_return_ring.py."""
import ctypes as C
import os
import re
import subprocess

import pytest

import client_ring_cases as cr
import return_ring_cases as rc
from conftest import ROOT

L_SMALL = 8


@pytest.fixture(scope="module")
def ring_check():
    lib = C.CDLL(rc.build_return_ring_check(os.path.join(ROOT, "tests", "hostcheck", "libreturn_ring_check.so")))
    lib.hc_client_ring_resp_stride.restype = C.c_uint32
    return lib


@pytest.fixture(scope="module")
def pool(oracle, bench_params):
    return rc.ReturnPool(oracle.ctx(bench_params, L_SMALL), bench_params, L_SMALL, "rrh")


def test_the_pool_is_what_the_issue_lists(pool):
    """the model's one-key answers, spelled out: which key accepts what, 8 only for a validly signed t > s, 4 for an altered t"""
    for k, kn in enumerate(("a", "b", "c", "d", "stranger")):
        for tn, want in (("0", 0), ("1", 0), ("s", 0), ("s+1", 8), ("l-1", 8)):
            row = pool.table[pool.by["%s/t=%s" % (kn, tn)]]
            assert [st for st, _ in row] == [want if j == k else 4 for j in range(5)], (kn, tn)
    assert {st for st, _ in pool.table[pool.by["b/altered to s+1"]]} == {4} == {st for st, _ in pool.table[pool.by["c/altered to s"]]}
    for name in ("a/undecodable_A", "d/undecodable_A t=s+1", "a/undecodable_Com"):
        assert {st for st, _ in pool.table[pool.by[name]]} == {255}, name
    # the token of an accepted item holds m + t
    i = pool.by["b/t=s"]
    pre = pool.items[i][1]
    assert pool.table[i][1][1][128:] == cr.scb(int.from_bytes(pre[64:96], "little") + pool.s[1])


def test_record_stride_is_a_function_of_label_and_with_t(ring_check):
    assert [ring_check.hc_client_ring_resp_stride(i, t) for i, t in ((1, 0), (1, 1), (0, 0), (0, 1))] == [160, 160, 128, 160]


def test_ring_lane_bodies_against_the_model(ring_check, pool, bench_params):
    idx = pool.lanes(len(pool.items) + 3)
    for ring in rc.RINGS:
        st, ok, tok, _ = rc.host_ring_call(ring_check, bench_params, pool, ring, idx)
        est, ekey, etok = pool.expected(ring, idx)
        assert (st, ok) == (est, ekey), (ring, pool.names, list(st), list(ok), list(est), list(ekey))
        assert tok == etok, ring
    # spelled out once: ring a, b, c, d
    st, ok, tok, _ = rc.host_ring_call(ring_check, bench_params, pool, [0, 1, 2, 3], list(range(len(pool.items))))
    got = dict(zip(pool.names, zip(st, ok)))
    none = cr.KEY_NONE
    for k, kn in enumerate(("a", "b", "c", "d")):
        for tn in ("0", "1", "s"):
            assert got["%s/t=%s" % (kn, tn)] == (0, k)
        for tn in ("s+1", "l-1"):
            assert got["%s/t=%s" % (kn, tn)] == (8, none)          # validly signed under a ring key, more than was spent
    for tn in ("0", "1", "s", "s+1", "l-1"):
        assert got["stranger/t=%s" % tn] == (4, none)               # also where t > s: no ring key signed it
    assert got["b/altered to s+1"] == (4, none) and got["c/altered to s"] == (4, none)      # 4, not 8
    assert got["a/undecodable_A"] == got["d/undecodable_A t=s+1"] == got["a/undecodable_Com"] == (255, none)
    for i, name in enumerate(pool.names):
        assert (tok[160 * i:160 * i + 160] == bytes(160)) == (got[name][0] != 0), name
    # a ring without the signer: 4 whatever t is; a duplicated entry: the first one wins
    st, ok, _, _ = rc.host_ring_call(ring_check, bench_params, pool, [2, 3], [pool.by["a/t=s+1"], pool.by["a/t=1"]])
    assert (list(st), list(ok)) == ([4, 4], [none, none])
    st, ok, _, _ = rc.host_ring_call(ring_check, bench_params, pool, [3, 0, 3, 0], [pool.by["a/t=s"], pool.by["d/t=1"], pool.by["a/t=l-1"]])
    assert (list(st), list(ok)) == ([0, 0, 8], [1, 0, none])


def test_one_key_ring_is_the_one_key_call(ring_check, pool, bench_params):
    """nkeys == 1 against the host build of the one-key return client (hc_return_client), byte for byte"""
    import refund_return_cases as rr
    idx = list(range(len(pool.items)))
    pre, proofs, recs = pool.inputs(idx)
    for k in range(5):
        st, ok, tok, _ = rc.host_ring_call(ring_check, bench_params, pool, [k], idx)
        ost, otok = rr.host_client(ring_check, bench_params, L_SMALL, pool.publics[k], pre, proofs, recs)
        assert (st, tok) == (ost, otok), k
        assert list(st) == [pool.table[i][k][0] for i in idx]
        assert list(ok) == [0 if s == 0 else cr.KEY_NONE for s in st]


def test_nothing_returned_is_the_refund_ring(ring_check, pool, bench_params):
    """t == 0 in every record against the host build of the plain refund ring on the first 128 bytes"""
    idx = pool.zero_items()
    assert len(idx) == 5
    pre, proofs, recs = pool.inputs(idx)
    refunds = b"".join(recs[160 * i:160 * i + 128] for i in range(len(idx)))
    n = len(idx)
    for ring in rc.RINGS:
        st, ok, tok, _ = rc.host_ring_call(ring_check, bench_params, pool, ring, idx)
        pst = C.create_string_buffer(n); pok = C.create_string_buffer(n); ptok = C.create_string_buffer(160 * n)
        assert ring_check.hc_client_ring(bench_params, L_SMALL, 0, b"".join(pool.ring_w(ring)), len(ring), n, pre, None, proofs, refunds, ptok, pst, pok, None, None) == 1
        assert (st, ok, tok) == (pst.raw, pok.raw, ptok.raw), ring


PRODUCT_G_WINDOWS, MADD_OPS = 16, 7      # as tests/test_client_ring_host.py restates its counts for the product's 16-bit table of g


def test_an_extra_key_costs_what_it_costs_a_plain_refund(ring_check, pool, bench_params):
    """A derived equality, not a measurement: t h1 belongs to phase A and does not depend on w, so
    cost(ring of k, return) - cost(ring of 1, return) == (k - 1) x the per-key cost of the plain refund ring, for k = 2 and 4 --
    counted the way tests/test_client_ring_host.py counts, on one item under both calls."""
    ring4 = [0, 1, 2, 3]
    for name in ("d/t=0", "d/t=s", "d/t=s+1"):
        i = pool.by[name]
        pre, proofs, recs = pool.inputs([i])
        st1, _, _, c1 = rc.host_ring_call(ring_check, bench_params, pool, ring4[:1], [i])
        assert c1[1] == 0 and c1[3] == 0
        # the plain refund ring over the first 128 bytes: the same e, gamma, z, so the same candidates and hashes
        plain = {}
        for nk in (2, 4):
            counts = (C.c_uint64 * 5)()
            st = C.create_string_buffer(1); ok = C.create_string_buffer(1); tok = C.create_string_buffer(160); cand = C.create_string_buffer(64 * 3)
            assert ring_check.hc_client_ring(bench_params, L_SMALL, 0, b"".join(pool.ring_w(ring4[:nk])), nk, 1, pre, None, proofs, recs[:128], tok, st, ok, cand, counts) == 1
            plain[nk] = counts[1]
        per_key = plain[2]
        assert plain[4] == 3 * per_key
        for nk in (2, 4):
            st, ok, _, c = rc.host_ring_call(ring_check, bench_params, pool, ring4[:nk], [i])
            total, total1 = c[0] + c[1], c1[0] + c1[1]
            assert total - total1 == (nk - 1) * per_key, (name, nk, total, total1, per_key)
            assert c[0] == c1[0], "the one-key body's count depends on the ring"
            # two products on g and one on w_k per extra key -- and none on h1, whose counter the ring tables share (CLIENT_RING_TAB_ID)
            assert (c[2], c[3]) == (2 * (nk - 1), nk - 1)
            if nk == 4:
                assert (st[0], ok[0]) == ((8, cr.KEY_NONE) if name.endswith("s+1") else (0, 3))
        restated = per_key - 2 * (c1[4] - PRODUCT_G_WINDOWS) * MADD_OPS
        print("%s: +%d field operations per extra key as built, %d with 16-bit g" % (name, per_key, restated))
        assert restated == 1023          # the figure of client_ring_lanes.h


def test_ring_lane_bodies_under_asan_ubsan(tmp_path, pool, bench_params):
    """The same bodies in a stand-alone program with its own main, built with -fsanitize=address,undefined and run as a child process;
    the buffers of a case have exactly the sizes the call is given."""
    exe = rc.build_return_ring_check(str(tmp_path / "return_ring_check_asan"), sanitize=True, main=True)
    idx = list(range(len(pool.items)))
    cases = [(pool, ring, idx) for ring in ([0], [1, 0], [0, 0, 1], [0, 1, 2, 3])] + [(pool, [3, 2, 1, 0], [pool.by["a/t=l-1"]])]
    path = str(tmp_path / "cases.bin")
    rc.write_case_file(path, bench_params, cases)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, path], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0 and "RETURN RING SANITIZERS CLEAN (%d cases)" % len(cases) in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-6000:]


# ---- the return calls' unique forms: the model ------------------------------------------------------------------------------------------
def test_unique_return_model_equals_the_plain_return_loop():
    rc.check_model_on_fixed_mix()
    rc.check_model_on_plans()


def test_counts_and_prototypes_in_the_header():
    hd = open(os.path.join(ROOT, "include", "act_mi355x.h")).read()
    assert re.search(r"#define ACT_REDEEM_RETURN_UNIQUE_COUNTS 10\b", hd) and re.search(r"#define ACT_REDEEM_RETURN_COUNTS 9\b", hd)
    from act_amd import capi
    assert capi.REDEEM_RETURN_UNIQUE_COUNTS == capi.REDEEM_RETURN_COUNTS + ("copies",) == rc.COUNTS_UNIQUE and len(rc.COUNTS_UNIQUE) == 10
    for name in ("act_refund_to_credit_token_return_keyring_batch", "act_redeem_return_unique_batch", "act_redeem_cbor_return_unique_batch"):
        assert name in capi.EXPORTS and re.search(r"\bint %s\(" % name, hd)
    # the replay forms still take no returned amounts; what is not offered is the node forms and the replay forms
    for proto in re.findall(r"\bint (act_\w*replay\w*)\(([^;]*)\);", hd):
        assert "returned" not in proto[1], proto[0]
    assert not re.search(r"\bint act_node_\w*return\w*\(", hd)
    assert "NOT OFFERED, on purpose: the replay forms" in hd and "Also not offered here: the node-handle forms." in hd
    assert "the client ring verifier and the unique forms" not in hd
