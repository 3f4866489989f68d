"""Key rotation on the CPU: the ring kernels' lane bodies (csrc/keyring_lanes.h) and the incremental challenge hash (csrc/blake3_hd.h
b3_xof64_patched, csrc/host_hash.cpp), compiled for the host by tests/hostcheck/keyring_check.cpp and judged by the C oracle called
once per candidate key.  The same bodies run on the GPU in tests/test_gpu_keyring.py."""
import ctypes as C
import os
import subprocess
import sys

import pytest

import keyring_cases as kr
from conftest import ROOT
from test_spend_lanes_host import op_counts


@pytest.fixture(scope="module")
def keyring_check():
    return C.CDLL(kr.build_keyring_check(os.path.join(ROOT, "tests", "hostcheck", "libkeyring_check.so")))


def test_ring_lane_bodies_against_the_oracle(keyring_check, oracle, bench_params):
    kr.check_lane_bodies(keyring_check, oracle, bench_params)


def test_an_extra_key_costs_under_one_percent_of_the_field_work(keyring_check, oracle, bench_params):
    """(operations with nkeys keys - operations with one) <= 1 % of the one-key total per extra key at L = 128: per extra key one
    chain_ct on A' (127 steps of 2 doublings, 2 ge_to_cached, 1 ge_add_cached), two decodings, one encoding, against ~453 k."""
    L = 128
    octx = oracle.ctx(bench_params, L)
    keys = kr.make_keys(octx, "kr-work")
    proof, _ = kr.spend_under(octx, keys[3], "kr-work-p")
    pb = octx.proof_bytes
    tb = 184 + 40 * (6 + 3 * L)
    tr = C.create_string_buffer(tb); st = C.create_string_buffer(1); kp = C.create_string_buffer(32)
    counts = (C.c_uint64 * 25)()
    assert keyring_check.hc_spend_verify(bench_params, L, keys[0], 1, proof, tr, st, kp, counts) == 1
    raw_mul = sum(counts[6 * k] for k in range(4)); raw_sq = sum(counts[6 * k + 1] for k in range(4))
    per_kernel = op_counts(list(counts), 1)
    total = sum(v["fe_mul"] + v["fe_sq"] for v in per_kernel.values())
    assert 400e3 < total < 500e3, total
    for nk in (1, 2, 3, 4):
        stt, ok, _, _, c = kr.host_ring_verify(keyring_check, bench_params, L, keys[:nk], proof)
        assert (c[0], c[1]) == (raw_mul, raw_sq), "the one-key kernels' count changed"
        extra = c[2] + c[3]
        print("nkeys=%d: +%d field operations = %.3f %% of %d per extra key" % (nk, extra, 100.0 * extra / max(1, nk - 1) / total, total))
        assert extra <= 0.01 * total * (nk - 1), (nk, extra, total)
        if nk == 1:
            assert extra == 0
        assert (stt[0], ok[0]) == ((0, 3) if nk == 4 else (7, 255))
        assert c[4] <= (nk - 1) * (16 + 4 + 1)


def test_incremental_challenge_hash(keyring_check, oracle):
    kr.check_incremental_hash(keyring_check, oracle)


def test_ring_lane_bodies_under_asan_ubsan(tmp_path):
    libasan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(libasan) or not os.path.exists(libasan):
        pytest.skip("no libasan in this toolchain")
    so = kr.build_keyring_check(str(tmp_path / "libkeyring_check_asan.so"), sanitize=True)
    env = dict(os.environ, LD_PRELOAD=libasan, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "keyring_sanitize_driver.py"), so], capture_output=True, text=True, env=env, timeout=1500)
    assert r.returncode == 0 and "KEYRING SANITIZERS CLEAN" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-6000:]
