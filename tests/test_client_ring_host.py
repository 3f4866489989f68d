"""The client's side of key rotation on the CPU: the ring lane bodies (csrc/client_ring_lanes.h) compiled for the host by
tests/hostcheck/client_ring_check.cpp and judged by the C oracle called once per ring key (oracle_c.py issuance_to_credit_token /
refund_to_credit_token), the smallest accepting index being the expected out_key.  The same bodies run on the GPU in
tests/test_gpu_client_ring.py."""
import ctypes as C
import os
import subprocess

import pytest

import client_ring_cases as cr
from conftest import ROOT

L_SMALL = 8


@pytest.fixture(scope="module")
def ring_check():
    return C.CDLL(cr.build_client_ring_check(os.path.join(ROOT, "tests", "hostcheck", "libclient_ring_check.so")))


@pytest.fixture(scope="module")
def pools(oracle, bench_params):
    octx = oracle.ctx(bench_params, L_SMALL)
    return {True: cr.Pool(octx, L_SMALL, True, "crh-iss"), False: cr.Pool(octx, L_SMALL, False, "crh-ref")}


@pytest.mark.parametrize("issuance", [True, False], ids=["issuance", "refund"])
def test_ring_lane_bodies_against_the_oracle(ring_check, pools, bench_params, issuance):
    """Items signed under each of four keys (and a fifth that is in no ring), rings of 1..4 keys: statuses, out_key and token bytes are
    the oracle's; a key outside the ring, a tampered gamma, an undecodable A, an undecodable Com_j (refund) / K (issuance) and a
    duplicated ring entry behave as the header says."""
    pool = pools[issuance]
    idx = pool.lanes(len(pool.items) + 3)
    bad, none = (2, 4)[0 if issuance else 1], cr.KEY_NONE
    for ring in cr.RINGS:
        st, ok, tok, cand, _ = cr.host_ring_call(ring_check, bench_params, pool, ring, idx)
        est, ekey, etok = pool.expected(ring, idx)
        assert (st, ok) == (est, ekey), (ring, pool.names, list(st), list(ok))
        assert tok == etok, ring
    # the table is what the feature says it is, spelled out once: ring a, b, c, d
    st, ok, tok, _, _ = cr.host_ring_call(ring_check, bench_params, pool, [0, 1, 2, 3], list(range(len(pool.items))))
    got = dict(zip(pool.names, zip(st, ok)))
    assert got == {"a": (0, 0), "b": (0, 1), "c": (0, 2), "d": (0, 3), "stranger": (bad, none), "tampered": (bad, none), "undecodable_A": (255, none),
                   ("undecodable_K" if issuance else "undecodable_Com"): (255, none)}, got
    for i, name in enumerate(pool.names):
        if got[name][0]:
            assert tok[160 * i:160 * i + 160] == bytes(160), name
    # a duplicated entry: the first one wins;   a ring without the signer: rejected, not 255
    st, ok, _, _, _ = cr.host_ring_call(ring_check, bench_params, pool, [3, 0, 3, 0], [0, 3])
    assert (list(st), list(ok)) == ([0, 0], [1, 0])
    st, ok, _, _, _ = cr.host_ring_call(ring_check, bench_params, pool, [2, 3], [0])
    assert (list(st), list(ok)) == ([bad], [none])


@pytest.mark.parametrize("issuance", [True, False], ids=["issuance", "refund"])
def test_one_key_ring_is_the_one_key_call(ring_check, pools, bench_params, issuance):
    pool = pools[issuance]
    idx = list(range(len(pool.items)))
    for k in range(5):
        st, ok, tok, _, _ = cr.host_ring_call(ring_check, bench_params, pool, [k], idx)
        assert list(st) == [pool.table[i][k][0] for i in idx]
        assert tok == b"".join(pool.table[i][k][1] for i in idx)
        assert list(ok) == [0 if pool.table[i][k][0] == 0 else cr.KEY_NONE for i in idx]


def test_candidates_are_the_transcript_elements_of_the_other_keys(ring_check, pools, bench_params):
    """enc(X_g,k) | enc(Y_g,k) of ring position k >= 1 are what phase A itself writes when key k is ring key 0: the candidate of
    (item, k) in ring [0, k] makes the ring call accept exactly the items the one-key call under k accepts (checked above), and the
    candidates do not depend on what else is in the ring."""
    pool = pools[False]
    idx = [0, 1, 2]
    _, _, _, c01, _ = cr.host_ring_call(ring_check, bench_params, pool, [0, 1], idx)
    _, _, _, c201, _ = cr.host_ring_call(ring_check, bench_params, pool, [2, 0, 1], idx)
    for i in range(len(idx)):
        assert c01[64 * i:64 * i + 64] == c201[64 * (2 * i + 1):64 * (2 * i + 1) + 64]


def test_patched_single_chunk_hash(ring_check, oracle):
    """b3_chunk_xof64_patched2 == BLAKE3 of the patched message, for replaced payloads at every byte residue and for lengths on both
    sides of the block boundaries (the prefixes are 185 / 186 bytes long: the X_g and Y_g slots are not word aligned)."""
    for length in (313, 425, 426, 448, 465, 466, 511, 512):      # 425 / 426 and 465 / 466 are the refund and respond transcripts
        for r in (80, 81, 82, 83, 32, 150):                     # the second payload ends the message, as Y_g does; the first lies r bytes before it
            off_b = length - 32
            off_a = off_b - r
            msg = cr.shake("crh-b3-%d-%d" % (length, r), length)
            ra, rb = cr.shake("crh-ra-%d-%d" % (length, r), 32), cr.shake("crh-rb-%d-%d" % (length, r), 32)
            out = C.create_string_buffer(64)
            ring_check.hc_client_ring_patched_hash(msg, length, off_a, ra, off_b, rb, out)
            patched = bytearray(msg); patched[off_a:off_a + 32] = ra; patched[off_b:off_b + 32] = rb
            assert out.raw == oracle.blake3(bytes(patched), 64), (length, off_a, off_b)


def test_finish_body_over_its_whole_domain(ring_check):
    """match mask x flags, for rings of 1..4 and both labels: the smallest matching index, 255 before 2 / 4, zeroed tokens"""
    for issuance in (True, False):
        for nkeys in (1, 2, 3, 4):
            d = cr.finish_domain(issuance, nkeys, "crh-fin")
            assert d["n"] == 4 << nkeys
            st, ok, tok = cr.run_finish_domain(ring_check, issuance, nkeys, d)
            assert (st, ok) == (d["status"], d["out_key"]), (issuance, nkeys)
            assert tok == d["tokens"], (issuance, nkeys)


# fixed_base_acc on g: this build's tables have 6-bit windows (43 mixed additions), the product's 16-bit ones (16); a mixed addition
# is 7 field multiplications (hostcheck.cpp says the same of its own counts)
PRODUCT_G_WINDOWS, MADD_OPS = 16, 7


def test_an_extra_key_costs_less_than_one_variable_base_product(ring_check, oracle, bench_params):
    """Field multiplications + squarings as tests/hostcheck counts them: what an extra ring key adds to an item must not exceed ONE
    chain_b<1> product on a random base and scalar -- the least any per-key variable-base form would pay.  Counted AS BUILT HERE
    (6-bit windows on g: the harder case) and restated for the product's 16-bit table of g; printed with the share of the one-key
    body, for issuance and for refund at L = 128 (DESIGN.md 4.6 quotes these figures)."""
    pt = oracle.mul_base(cr.scb(int.from_bytes(cr.shake("crh-cost-pt", 40), "little")))
    s = cr.scb(int.from_bytes(cr.shake("crh-cost-s", 40), "little"))
    out = C.create_string_buffer(32); n_ops = C.c_uint64(0)
    assert ring_check.hc_chain_b1_ops(pt, s, out, C.byref(n_ops)) == 1
    assert out.raw == oracle.mul(pt, s)
    chain = n_ops.value
    assert 2000 < chain < 3500, chain
    octx = oracle.ctx(bench_params, 128)
    for issuance in (True, False):
        pool = cr.Pool(octx, 128, issuance, "crh-cost-%d" % issuance)
        base = None
        for nk in (1, 2, 3, 4):
            st, ok, _, _, c = cr.host_ring_call(ring_check, bench_params, pool, [0, 1, 2, 3][:nk], [3])
            assert (st[0], ok[0]) == ((0, 3) if nk == 4 else ((2 if issuance else 4), cr.KEY_NONE))
            one_key, extra, on_g, on_w, host_windows = c
            base = one_key if base is None else base
            assert one_key == base, "the one-key body's count depends on the ring"
            if nk == 1:
                assert extra == 0
                continue
            assert (on_g, on_w) == (2 * (nk - 1), nk - 1)
            per_key = extra / (nk - 1)
            restated = per_key - 2 * (host_windows - PRODUCT_G_WINDOWS) * MADD_OPS
            # the one-key body restated the same way: two products on g (and one on h1 for issuance)
            one_key_product = one_key - (3 if issuance else 2) * (host_windows - PRODUCT_G_WINDOWS) * MADD_OPS
            print("%s nkeys=%d: +%d field operations per extra key as built, %d with 16-bit g = %.3f of one chain_b<1> (%d) = %.2f %% of the one-key body (%d)"
                  % ("issuance" if issuance else "refund L=128", nk, per_key, restated, restated / chain, chain, 100.0 * restated / one_key_product, one_key_product))
            assert per_key <= chain, (issuance, nk, per_key, chain)
            assert restated <= chain


def test_ring_lane_bodies_under_asan_ubsan(tmp_path, pools, bench_params):
    """The same bodies in a stand-alone program built with -fsanitize=address,undefined, replaying the lifecycle cases and the finish
    domain from a file with the oracle's answers in it; run as a child process in the inherited environment.  The sanitizer runtimes are linked
    statically into the program, so it needs nothing preloaded and starts beside whatever the environment preloads."""
    exe = cr.build_client_ring_check(str(tmp_path / "client_ring_check_asan"), sanitize=True, main=True)
    ring_cases = []
    for issuance in (True, False):
        pool = pools[issuance]
        idx = list(range(len(pool.items)))
        for ring in ([0], [1, 0], [0, 0, 1], [0, 1, 2, 3]):
            ring_cases.append((pool, ring, idx))
    finish_cases = [(iss, nk, cr.finish_domain(iss, nk, "crh-fin")) for iss in (True, False) for nk in (1, 2, 3, 4)]
    path = str(tmp_path / "cases.bin")
    cr.write_case_file(path, bench_params, ring_cases, finish_cases)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, path], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0 and "CLIENT RING SANITIZERS CLEAN (%d cases)" % (len(ring_cases) + len(finish_cases)) in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-6000:]
