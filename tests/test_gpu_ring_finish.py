"""The end of a ring call whose LAST chunk runs on the second slot: the wipe of slot 0's shared staging areas (the ring's decoded keys,
the CBOR layout tables) must wait for both slots' streams.  Before it did, act_redeem_keyring_batch in device memory with per-lane rng
now and then signed the last chunk's refunds with x = 0 (z, sometimes gamma, differed from the host-memory call's bytes)."""
import numpy as np
import pytest

from conftest import shake, scb

pytestmark = pytest.mark.gpu

MB = 16
N = 9 * MB + 6          # ten chunks: the last one (six lanes) runs on slot 1


def test_ring_redeem_in_device_memory_equals_host_memory_every_time(engine_factory, bench_params):
    import torch
    from act_amd import capi
    L = 8
    eng = engine_factory(bench_params, L, max_batch=MB, transcript=capi.TRANSCRIPT_DEVICE)
    keys = [eng.private_key_random(shake("rf-sk%d" % i, 64)) for i in range(2)]
    pre = eng.pre_issuance_random(shake("rf-pre", 128 * N)); req = eng.request(pre, shake("rf-rq", 128 * N))
    st, resp = eng.issue(keys[1], req, scb(9) * N, shake("rf-ir", 128 * N))
    st, tok = eng.issuance_to_credit_token(pre, keys[1][32:], req, resp)
    st, proofs, _ = eng.prove_spend_seeded(tok, scb(2) * N, shake("rf-seed", 32))
    assert st == bytes(N)
    ring = [keys[0], keys[1]]                           # every proof matches ring key 1: x of the matched key is not ring[0].x
    rng = shake("rf-rng", 128 * N)
    ns = capi.NullifierSet(4 * N)
    want = eng.redeem_keyring(ns, ring, proofs, rng, capi.RNG_PER_LANE)
    ns.close()
    assert want[0] == bytes(N) and want[2] == b"\1" * N
    up = lambda b: torch.from_numpy(np.frombuffer(b + b"\0", np.uint8).copy()).cuda()
    dp, dr = up(proofs), up(rng)
    for rnd in range(12):
        ns = capi.NullifierSet(4 * N)
        out = torch.full((128 * N,), 7, dtype=torch.uint8, device="cuda"); dst = torch.full((N,), 9, dtype=torch.uint8, device="cuda")
        dok = torch.full((N,), 9, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        eng.keyring_ptr("redeem", ring, N, capi.MEM_DEVICE, set=ns, proofs=dp.data_ptr(), rng=dr.data_ptr(), rng_mode=capi.RNG_PER_LANE, out=out.data_ptr(),
                        status=dst.data_ptr(), out_key=dok.data_ptr())
        got = (dst.cpu().numpy().tobytes(), out.cpu().numpy().tobytes(), dok.cpu().numpy().tobytes())
        ns.close()
        bad = [i for i in range(N) if got[1][128 * i:128 * i + 128] != want[1][128 * i:128 * i + 128]]
        assert got[0] == want[0] and got[2] == want[2] and not bad, (rnd, bad)
