"""Node-level dispatch (include/act_mi355x.h act_node_*): a batch cut into contiguous shards over several contexts must
give byte-for-byte what one context gives -- in particular with ACT_RNG_SEQUENTIAL, where a lane's rng slice depends on
how many lanes in front of it (on other shards too) were accepted (/root/reference/src/lib.rs:638-643, 842-846).  A box
of the test pool has one GPU, so the "devices" are several contexts on device 0: the dispatcher, its threads, the slicing
and the two-phase sequential path are exactly those of a multi-GPU node; and bench.py's N > 1 path is driven with two
ranks sharing device 0 through its gloo hook."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT, shake, scb

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)])
@pytest.mark.parametrize("mode", [0, 1])
def test_node_equals_single_context(engine_factory, bench_params, devices, mode):
    from act_amd import capi
    L, N = 8, 23
    eng = engine_factory(bench_params, L, max_batch=5, transcript=mode)
    node = capi.Node(bench_params, L, devices=devices, max_batch=5, transcript=mode)
    assert node.device_count() == len(devices)
    sk = eng.private_key_random(shake("node-sk", 64))
    pre = eng.pre_issuance_random(shake("node-pre", 128 * N))
    rq = shake("node-rq", 128 * N)
    req = eng.request(pre, rq)
    assert node.request(pre, rq) == req
    bad = bytearray(req)
    bad[128 * 1 + 70] ^= 1; bad[128 * 9 + 40] ^= 1; bad[128 * 10 + 3] ^= 0x08; bad[128 * 22 + 100] ^= 1      # rejected lanes on every shard
    bad = bytes(bad)
    cam = b"".join(scb(200 + i) for i in range(N))
    irng = shake("node-ir", 128 * N)
    for rng_mode in (capi.RNG_PER_LANE, capi.RNG_SEQUENTIAL):
        want = eng.issue(sk, bad, cam, irng, rng_mode)
        assert node.issue(sk, bad, cam, irng, rng_mode) == want, rng_mode
        assert {0, 1} <= set(want[0])
    st, resp = eng.issue(sk, req, cam, irng)
    st, tok = eng.issuance_to_credit_token(pre, sk[32:], req, resp)
    assert node.issuance_to_credit_token(pre, sk[32:], req, resp) == (st, tok)
    s_b = b"".join(scb(3 * i) for i in range(N))
    prng = shake("node-pr", eng.prove_rng_bytes * N)
    want = eng.prove_spend(tok, s_b, prng)
    assert node.prove_spend(tok, s_b, prng) == want
    proofs, prer = bytearray(want[1]), want[2]
    pb = eng.proof_bytes
    proofs[pb * 0 + 33] ^= 2; proofs[pb * 7 + 64:pb * 7 + 96] = bytes(32); proofs[pb * 8 + 32 * 5 + 1] ^= 0x40
    proofs[pb * 15 + 32 * (4 + L) + 2] ^= 1; proofs[pb * 22 + 33] ^= 1
    proofs = bytes(proofs)
    assert node.verify_spend(sk, proofs, True) == eng.verify_spend(sk, proofs, True)
    rrng = shake("node-rr", 128 * N)
    for rng_mode in (capi.RNG_PER_LANE, capi.RNG_SEQUENTIAL):
        want = eng.refund(sk, proofs, rrng, rng_mode)
        got = node.refund(sk, proofs, rrng, rng_mode)
        assert got == want, rng_mode
        assert {0, 6, 7} <= set(want[0])
    # the halves through the node handle: check, draw exactly 128 bytes per accepted lane, sign -- what the Rust binding does
    st, kp = node.verify_spend(sk, proofs, True)
    accepted = sum(1 for v in st if v == 0)
    assert node.refund_sign(sk, kp, st, rrng[:128 * accepted]) == eng.refund(sk, proofs, rrng, capi.RNG_SEQUENTIAL)
    st = node.issue_check(bad)
    accepted = sum(1 for v in st if v == 0)
    assert node.issue_sign(sk, bad, cam, st, irng[:128 * accepted]) == eng.issue(sk, bad, cam, irng, capi.RNG_SEQUENTIAL)
    st, rf = eng.refund(sk, proofs, rrng)
    assert node.refund_to_credit_token(prer, proofs, rf, sk[32:]) == eng.refund_to_credit_token(prer, proofs, rf, sk[32:])
    # fewer lanes than shards, and an empty batch
    assert node.refund(sk, proofs[:pb], rrng[:128], capi.RNG_SEQUENTIAL) == eng.refund(sk, proofs[:pb], rrng[:128], capi.RNG_SEQUENTIAL)
    assert node.verify_spend(sk, b"") == b""
    node.close()


def test_check_then_sign_equals_one_call(engine_factory, bench_params):
    """act_issue_check_batch + act_issue_sign_batch / act_verify_spend_batch + act_refund_sign_batch = the one-call forms."""
    import ctypes as C
    import numpy as np
    from act_amd import capi
    L, N = 8, 11
    eng = engine_factory(bench_params, L, max_batch=4)
    lib = eng.lib
    sk = eng.private_key_random(shake("cs-sk", 64))
    pre = eng.pre_issuance_random(shake("cs-pre", 128 * N)); req = bytearray(eng.request(pre, shake("cs-rq", 128 * N)))
    req[128 * 2 + 70] ^= 1; req = bytes(req)
    cam = scb(77) * N; irng = shake("cs-ir", 128 * N)
    buf = lambda b: np.frombuffer(b, np.uint8).copy()
    for rng_mode in (0, 1):
        want = eng.issue(sk, req, cam, irng, rng_mode)
        st = np.zeros(N, np.uint8); out = np.zeros(160 * N, np.uint8); st2 = np.zeros(N, np.uint8)
        a = [buf(x) for x in (sk, req, cam, irng)]
        assert lib.act_issue_check_batch(eng.ctx, N, 0, a[1].ctypes.data, st.ctypes.data) == 0
        assert lib.act_issue_sign_batch(eng.ctx, N, 0, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, st.ctypes.data, a[3].ctypes.data, rng_mode,
                                        out.ctypes.data, st2.ctypes.data) == 0
        assert (st2.tobytes(), out.tobytes()) == want
    st, resp = eng.issue(sk, eng.request(pre, shake("cs-rq", 128 * N)), cam, irng)
    st, tok = eng.issuance_to_credit_token(pre, sk[32:], eng.request(pre, shake("cs-rq", 128 * N)), resp)
    st, proofs, _ = eng.prove_spend(tok, scb(5) * N, shake("cs-pr", eng.prove_rng_bytes * N))
    proofs = bytearray(proofs); proofs[eng.proof_bytes * 4 + 33] ^= 1; proofs = bytes(proofs)
    rrng = shake("cs-rr", 128 * N)
    for rng_mode in (0, 1):
        want = eng.refund(sk, proofs, rrng, rng_mode)
        st, kp = eng.verify_spend(sk, proofs, True)
        a = [buf(x) for x in (sk, kp, st, rrng)]
        out = np.zeros(128 * N, np.uint8); st2 = np.zeros(N, np.uint8)
        assert lib.act_refund_sign_batch(eng.ctx, N, 0, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data, rng_mode,
                                         out.ctypes.data, st2.ctypes.data) == 0
        assert (st2.tobytes(), out.tobytes()) == want


def test_bench_two_ranks_on_one_device():
    """`python bench.py --gpus 2` run DIRECTLY, the way the driver runs it: the bench must start its two ranks itself (round 3
    parsed --gpus and never read it: an 8-GPU driver run would have measured one GPU), every rank must see WORLD_SIZE == --gpus,
    `value` must be weak scaling (independent proofs sharded over the ranks, every rank its own batch: per-GPU work fixed) with the
    strong figure (ONE batch cut over the whole node) alongside, and rank 0 must also time the product's own multi-GPU path (one process, one act_node handle over both devices).
    Two gloo ranks that both drive device 0 through the bench's --dist-backend / --force-device hooks (RCCL refuses two ranks on
    one device)."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("WORLD_SIZE", None); env.pop("RANK", None); env.pop("LOCAL_RANK", None)
    args = ["--gpus", "2", "--steps", "2", "--warmup", "1", "--batch-log2", "12", "--max-batch", "1024", "--distinct", "256",
            "--dist-backend", "gloo", "--force-device", "0"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args + ["--full"], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]                       # ONE line, relayed from rank 0
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["scaling"] == "weak" and d["cpu_baseline"] is None
    assert d["config"]["batch_per_gpu"] == 4096 and d["config"]["batch_total"] == 8192
    assert d["config"]["transcript"] == "host BLAKE3 (src/transcript.rs)" and "resident in HBM" in d["config"]["workload"]
    assert d["value"] == d["weak"]["value"]
    assert abs(d["value"] - 2 * 4096 * 2 / (d["ms_per_step"] * 2 / 1e3)) < 1e-6 * d["value"]      # whole-job aggregate over both ranks
    s, w = d["strong"], d["weak"]
    assert s["batch_total"] == 4096 and s["batch_per_gpu"] == 2048 and s["scaling"] == "strong"
    assert w["batch_per_gpu"] == 4096 and abs(w["value"] - 2 * 4096 * 2 / (w["ms_per_step"] * 2 / 1e3)) < 1e-6 * w["value"]
    assert d["roofline"]["avg_launch_ms"] * d["roofline"]["launches_per_step"] <= d["ms_per_step"] * 1.001
    assert d["roofline"]["bound"] == "valu-int-mad" and 0 < d["roofline"]["frac"] < 1 and d["roofline"]["hbm"]["bound"] == "hbm"
    nm = d["node_multi"]
    assert "error" not in nm, nm
    assert nm["devices"] == [0, 0] and nm["proofs"] == 4096 and nm["value"] > 0 and nm["host_pool"]["threads_created"] <= nm["host_pool"]["pool_size"]
    # under a launcher (the other way the driver may start it), --scaling strong swaps which of the two is `value`
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29671",
           os.path.join(ROOT, "bench.py")] + args + ["--scaling", "strong", "--no-node-multi", "--full"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["config"]["batch_per_gpu"] == 2048 and d["config"]["batch_total"] == 4096
    assert d["value"] == d["strong"]["value"] and d["weak"]["batch_per_gpu"] == 4096 and "node_multi" not in d
    assert abs(d["value"] - 4096 * 2 / (d["ms_per_step"] * 2 / 1e3)) < 1e-6 * d["value"]
    # RCCL that cannot come up (here: two ranks on ONE device, which it refuses) must not cost the measurement: the barrier and the
    # reduction of the ranks' times fall back to gloo -- the data path has no collective -- and the line says which carried them
    args_rccl = [a for a in args if a not in ("--dist-backend", "gloo")] + ["--no-node-multi"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args_rccl, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert d["n_gpus"] == 2 and d["value"] > 0 and d["config"]["dist_backend"].startswith("gloo (RCCL failed to initialise)")
    # a launcher whose world size disagrees with --gpus is refused: the line would claim GPUs that were not measured
    bad = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1", "--master-port", "29672",
           os.path.join(ROOT, "bench.py")] + args
    r = subprocess.run(bad, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode != 0 and "WORLD_SIZE" in (r.stderr + r.stdout)


def test_eight_contexts_on_one_pool_do_not_oversubscribe(engine_factory, bench_params):
    """a node handle over 8 contexts in host-transcript mode used to start 8 x all-CPUs threads per hash piece.
    With the process-wide pool (csrc/host_pool.cpp) the process creates its workers once, statuses are identical, and what the
    HOST side costs does not grow with the number of contexts: on the one GPU of a test box eight contexts contend for the device
    (16 streams on its hardware queues) in either transcript mode, so the host side is isolated as the ratio host-transcripts /
    device-transcripts at 8 contexts against the same ratio at 2."""
    import time
    import numpy as np
    from act_amd import capi
    L, n = 128, 1 << 18          # 2^15 proofs = 8 chunks per context at 8 contexts: steady state, not pipeline fill and drain
    eng = engine_factory(bench_params, L, max_batch=4096, transcript=capi.TRANSCRIPT_DEVICE)
    sk = eng.private_key_random(shake("np-sk", 64))
    base = 64
    pre = eng.pre_issuance_random(shake("np-pre", 128 * base)); req = eng.request(pre, shake("np-rq", 128 * base))
    st, resp = eng.issue(sk, req, b"".join(scb(100 + i) for i in range(base)), shake("np-ir", 128 * base))
    st, tok = eng.issuance_to_credit_token(pre, sk[32:], req, resp)
    st, proofs, _ = eng.prove_spend(tok, b"".join(scb(i) for i in range(base)), shake("np-pr", eng.prove_rng_bytes * base))
    assert st == bytes(base)
    batch = np.frombuffer(proofs * (n // base), np.uint8).copy()
    batch[eng.proof_bytes * 5 + 33] ^= 1
    want = bytes(7 if i == 5 else 0 for i in range(n))
    rates = {}
    for ndev in (2, 8):
        node = capi.Node(bench_params, L, devices=(0,) * ndev, max_batch=4096, transcript=capi.TRANSCRIPT_HOST)
        node.set_balance(False, 0)          # equal static shares: this test isolates the host side; contexts that share ONE GPU have no speed differences to balance
        try:
            stn = np.zeros(n, np.uint8)
            for mode in (capi.TRANSCRIPT_HOST, capi.TRANSCRIPT_DEVICE):
                node.set_transcript_mode(mode)
                node.verify_spend_ptr(sk, n, batch.ctypes.data, stn.ctypes.data)           # warm-up: staging buffers, pinned transcripts, the pool
                created = capi.host_pool_stats()["threads_created"]
                best = 1e9
                for _ in range(3):
                    t0 = time.perf_counter(); node.verify_spend_ptr(sk, n, batch.ctypes.data, stn.ctypes.data); best = min(best, time.perf_counter() - t0)
                assert stn.tobytes() == want
                assert capi.host_pool_stats()["threads_created"] == created <= capi.host_usable_cpus()
                rates[ndev, mode] = n / best
        finally:
            node.close()
    H, D = capi.TRANSCRIPT_HOST, capi.TRANSCRIPT_DEVICE
    print("verifies/s (contexts, transcript mode):", rates)
    # (box to box the two ratios move by a few per cent each: 0.976 / 0.988, 0.947 / 1.012 measured; the thread-creation assertions
    # above are the functional guard)
    assert rates[8, H] / rates[8, D] > 0.90 * rates[2, H] / rates[2, D], rates


def test_bench_rccl_path_with_one_rank(tmp_path):
    """bench.py's RCCL calls (init_process_group("nccl", device_id=...), barrier, all_reduce MAX of the timing, destroy) on the one GPU a
    test box has: one rank under torch.distributed.run with --force-dist.  The two-rank test above uses gloo because RCCL refuses two
    ranks on one device; this one makes sure the nccl branch itself runs."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1", "--master-port", "29673",
           os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch-log2", "12", "--max-batch", "1024",
           "--force-dist", "--no-extras", "--no-cpu-baseline", "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["config"]["distinct_proofs_per_gpu"] == 4096 and d["value"] > 0
    # a plain run times exactly --steps steps and measures nothing beside `value`
    assert d["steps"] == 2 and abs(d["value"] - 4096 * 2 / (d["ms_per_step"] * 2 / 1e3)) < 1e-6 * d["value"]
    assert "roofline" not in d and "host_memory_path" not in d and "extra" not in d and d["cpu_baseline"] is None
    # --dump-outputs: the statuses of the last timed step, the bench's tamper pattern (1 lane in 1024 from lane 513: 7, 6, ...)
    import numpy as np
    st = np.load(os.path.join(str(tmp_path), "statuses.npy"))
    want = np.zeros(4096, np.float32); want[513::2048] = 7; want[1537::2048] = 6
    assert st.dtype == np.float32 and st.shape == (4096,) and np.array_equal(st, want)


def test_single_item_refunds_from_many_threads_on_a_node_handle(engine_factory, bench_params):
    """The Rust binding's `PrivateKey::refund` (rust/src/mi355x.rs): act_node_verify_spend_batch over ONE proof, then -- with 128
    bytes drawn only if it verified -- act_node_refund_sign_batch (ACT_RNG_SEQUENTIAL), on the one node handle every thread of a
    server shares.  Such calls queue on the handle; every thread must get exactly the refund (or the rejection) it gets alone."""
    import threading
    from act_amd import capi
    L, D = 8, 40
    eng = engine_factory(bench_params, L, max_batch=256, transcript=capi.TRANSCRIPT_DEVICE)
    sk = eng.private_key_random(shake("nm-sk", 64))
    pre = eng.pre_issuance_random(shake("nm-pre", 128 * D)); req = eng.request(pre, shake("nm-rq", 128 * D))
    st, resp = eng.issue(sk, req, b"".join(scb(70 + i) for i in range(D)), shake("nm-ir", 128 * D))
    st, tok = eng.issuance_to_credit_token(pre, sk[32:], req, resp)
    st, proofs, _ = eng.prove_spend(tok, b"".join(scb(i % 30) for i in range(D)), shake("nm-pr", eng.prove_rng_bytes * D))
    assert st == bytes(D)
    pb = eng.proof_bytes
    items = []
    for i in range(D):
        p = bytearray(proofs[pb * i:pb * (i + 1)])
        if i % 5 == 0:
            p[40] ^= 1                                   # rejected: no rng drawn, no refund
        items.append(bytes(p))
    node = capi.Node(bench_params, L, devices=(0, 0), max_batch=256, transcript=capi.TRANSCRIPT_DEVICE)

    def refund_one(i):
        stv, kp = node.verify_spend(sk, items[i], True)
        rng = shake("nm-r%d" % i, 128) if stv[0] == 0 else b"\0"   # the binding draws after the verdict: nothing for a rejected proof (a non-null pointer to no bytes)
        st2, rf = node.refund_sign(sk, kp, stv, rng, capi.RNG_SEQUENTIAL)
        return stv, st2, rf
    try:
        alone = [refund_one(i) for i in range(D)]
        merged = [None] * D

        def work(t):
            try:
                for i in range(t, D, 8):
                    merged[i] = refund_one(i)
            except BaseException as e:
                merged[t] = e
        th = [threading.Thread(target=work, args=(t,)) for t in range(8)]
        for x in th:
            x.start()
        for x in th:
            x.join()
    finally:
        node.close()
    for i in range(D):
        assert not isinstance(merged[i], BaseException), merged[i]
        assert merged[i] == alone[i], i
        assert alone[i][0][0] == (7 if i % 5 == 0 else 0) and (alone[i][2] == bytes(128)) == (i % 5 == 0)


def test_single_item_issues_from_many_threads_on_a_node_handle(engine_factory, bench_params, oracle):
    """The Rust binding's `PrivateKey::issue`: act_node_issue_check_batch over ONE request, then act_node_issue_sign_batch
    (ACT_RNG_SEQUENTIAL, 128 bytes drawn only if the request verified), from eight threads that share a node handle."""
    import threading
    from act_amd import capi
    L, D = 8, 32
    eng = engine_factory(bench_params, L, max_batch=256, transcript=capi.TRANSCRIPT_DEVICE)
    sk = eng.private_key_random(shake("ni-sk", 64))
    pre = eng.pre_issuance_random(shake("ni-pre", 128 * D)); reqs = eng.request(pre, shake("ni-rq", 128 * D))
    items = []
    for i in range(D):
        r = bytearray(reqs[128 * i:128 * (i + 1)])
        if i % 6 == 0:
            r[70] ^= 1                                   # k_bar tampered: InvalidIssuanceRequestProof, nothing drawn, nothing signed
        items.append(bytes(r))
    node = capi.Node(bench_params, L, devices=(0, 0), max_batch=256, transcript=capi.TRANSCRIPT_DEVICE)

    def issue_one(i):
        stc = node.issue_check(items[i])
        rng = shake("ni-r%d" % i, 128) if stc[0] == 0 else b"\0"
        st2, resp = node.issue_sign(sk, items[i], scb(10 + i), stc, rng, capi.RNG_SEQUENTIAL)
        return stc, st2, resp
    try:
        alone = [issue_one(i) for i in range(D)]
        merged = [None] * D

        def work(t):
            try:
                for i in range(t, D, 8):
                    merged[i] = issue_one(i)
            except BaseException as e:
                merged[t] = e
        th = [threading.Thread(target=work, args=(t,)) for t in range(8)]
        for x in th:
            x.start()
        for x in th:
            x.join()
    finally:
        node.close()
    octx = oracle.ctx(bench_params, L)
    for i in range(D):
        assert not isinstance(merged[i], BaseException), merged[i]
        assert merged[i] == alone[i], i
        so, resp = octx.issue(sk, items[i], scb(10 + i), shake("ni-r%d" % i, 128))
        assert alone[i][1][0] == so == (1 if i % 6 == 0 else 0) and alone[i][2] == resp


def test_slow_context_is_relieved_and_bytes_do_not_change(engine_factory, bench_params):
    """Load balance of the node dispatcher on real contexts: three contexts, one of them made slower by the test
    hook.  In the first call the others take the tail pieces; the weights that call leaves behind give the slow context a
    smaller head in the second; statuses, K' and (ACT_RNG_SEQUENTIAL, cut into pieces) refunds equal one context's."""
    from act_amd import capi
    L, distinct, reps = 8, 4096, 48
    n = distinct * reps
    eng = engine_factory(bench_params, L, max_batch=16384)
    sk = eng.private_key_random(shake("lb-sk", 64))
    pre = eng.pre_issuance_random(shake("lb-pre", 128 * distinct)); req = eng.request(pre, shake("lb-rq", 128 * distinct))
    st, resp = eng.issue(sk, req, b"".join(scb(1000 + i) for i in range(distinct)), shake("lb-ir", 128 * distinct))
    st, tok = eng.issuance_to_credit_token(pre, sk[32:], req, resp)
    st, proofs, _ = eng.prove_spend(tok, b"".join(scb(i % 200) for i in range(distinct)), shake("lb-pr", eng.prove_rng_bytes * distinct))
    assert st == bytes(distinct)
    pb = eng.proof_bytes
    tampered = bytearray(proofs)
    for i in range(0, distinct, 97):
        tampered[pb * i + 33] ^= 1
    batch = bytes(tampered) * reps
    rng = shake("lb-rr", 128 * distinct) * reps
    want_v = eng.verify_spend(sk, batch, True)
    want_r = eng.refund(sk, batch, rng, capi.RNG_SEQUENTIAL)
    node = capi.Node(bench_params, L, devices=(0, 0, 0), max_batch=16384)
    try:
        node.lib.act_debug_set_slowdown(node.ctx_handle(1), 1000)      # 1 us per lane on top of context 1's calls
        assert node.verify_spend(sk, batch, True) == want_v
        s1, b1 = node.device_stats(), node.balance_state()
        assert sum(d["lanes"] for d in s1) == n and abs(b1["tail_fraction"] - 1 / 16) < 0.01 and b1["spread"] > 0.2, (s1, b1)
        assert s1[1]["calls"] == 1 and s1[0]["calls"] + s1[2]["calls"] == 2 + 3, s1           # the three tail pieces went to the fast contexts
        assert s1[1]["weight"] < 0.9 < s1[0]["weight"], s1
        assert node.refund(sk, batch, rng, capi.RNG_SEQUENTIAL) == want_r                       # verify pass + sign pass, both cut by the weights
        assert node.verify_spend(sk, batch, True) == want_v
        s2 = node.device_stats()
        assert s2[1]["lanes"] < 0.9 * s2[0]["lanes"] and sum(d["lanes"] for d in s2) == n, s2
        node.set_balance(False, 0)
        assert node.verify_spend(sk, batch) == want_v[0]
        assert [d["lanes"] for d in node.device_stats()] == [n // 3] * 3
    finally:
        node.close()
