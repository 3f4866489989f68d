"""Shared by the key-ring tests (tests/test_keyring_*.py, tests/test_gpu_keyring*.py): the lane mix of the issue, what the C oracle
-- called once per candidate key -- says about every lane, and the host build of the ring lane bodies (tests/hostcheck/
keyring_check.cpp).  Not a test module."""
import ctypes as C
import hashlib
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ELL = 2**252 + 27742317777372353535851937790883648493
KEY_NONE = 255


def shake(label, n):
    return hashlib.shake_256(label.encode()).digest(n)


def scb(v):
    return (v % ELL).to_bytes(32, "little")


def make_keys(octx, tag, count=5):
    """a, b, c, d (ring material) and e (a stranger)."""
    return [octx.private_key_random(shake("%s-sk-%d" % (tag, i), 64)) for i in range(count)]


def spend_under(octx, sk, tag, credit=9, spend=2):
    pre = octx.pre_issuance_random(shake(tag + "-pre", 128))
    req = octx.request(pre, shake(tag + "-rq", 128))
    st, resp = octx.issue(sk, req, scb(credit), shake(tag + "-ir", 128))
    assert st == 0
    st, tok = octx.issuance_to_credit_token(pre, sk[32:], req, resp)
    assert st == 0
    st, proof, prerefund = octx.prove_spend(tok, scb(spend), shake(tag + "-pr", octx.prove_rng_bytes))
    assert st == 0
    return proof, prerefund


def lane_mix(octx, keys, tag):
    """Proofs under a, b, c (tokens issued under three different keys), one under a key outside every ring (e), a tampered lane,
    A' = identity, an undecodable A'.  Returns [(name, proof, prerefund)]."""
    a, b, c, d, e = keys
    lanes = []
    for name, sk in (("a", a), ("b", b), ("c", c), ("stranger", e), ("a2", a), ("b2", b)):
        proof, prer = spend_under(octx, sk, "%s-%s" % (tag, name))
        lanes.append((name, proof, prer))
    t = bytearray(lanes[4][1]); t[33] ^= 1                      # the charge s
    lanes[4] = ("tampered", bytes(t), lanes[4][2])
    t = bytearray(lanes[5][1]); t[64:96] = bytes(32)            # A' = identity
    lanes.append(("identity", bytes(t), lanes[5][2]))
    t = bytearray(lanes[5][1]); t[64:96] = b"\xff" * 32         # not a canonical encoding
    lanes.append(("undecodable", bytes(t), lanes[5][2]))
    return lanes


def oracle_ring_verdict(octx, ring, proof):
    """(status, out_key, K') by the contract: the smallest k whose PrivateKey::refund accepts; 255 / 6 are the same under every key."""
    per_key = [octx.verify_spend(sk, proof) for sk in ring]
    for k, (st, kp) in enumerate(per_key):
        if st == 0:
            return 0, k, kp
    sts = {st for st, _ in per_key}
    if sts == {7}:
        return 7, KEY_NONE, bytes(32)
    assert len(sts) == 1 and sts <= {6, 255}, sts               # decoding and the identity check do not depend on the key
    return sts.pop(), KEY_NONE, bytes(32)


def build_keyring_check(out, sanitize=False):
    """tests/hostcheck/keyring_check.cpp + csrc/host_hash.cpp (-DACT_B3_COUNT) -> a shared object of its own.  host_hash.cpp is built
    without the sanitizer (its target_clones resolvers run before the sanitizer runtime exists)."""
    csrc = os.path.join(ROOT, "anonymous-credit-tokens_amd", "csrc")
    src = os.path.join(ROOT, "tests", "hostcheck", "keyring_check.cpp")
    deps = [src, os.path.join(ROOT, "tests", "hostcheck", "hostcheck.cpp")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".h", ".inc", "host_hash.cpp"))]
    if os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in deps):
        return out
    hh = out + ".host_hash.o"
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-Wno-psabi", "-DACT_B3_COUNT", "-c", "-o", hh, os.path.join(csrc, "host_hash.cpp")], check=True)
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-Wno-psabi", *flags, "-o", out, src, hh], check=True)
    os.remove(hh)
    return out


def host_ring_verify(kc, h, L, ring, proofs):
    pb = 32 * (14 + 4 * L)
    n = len(proofs) // pb
    nk = len(ring)
    st = C.create_string_buffer(n); ok = C.create_string_buffer(n); kp = C.create_string_buffer(32 * n)
    cand = C.create_string_buffer(max(1, 32 * n * (nk - 1)))
    counts = (C.c_uint64 * 5)()
    assert kc.hc_ring_verify(h, L, b"".join(ring), nk, n, proofs, st, ok, kp, cand, counts) == 1
    return st.raw, ok.raw, kp.raw, cand.raw, list(counts)


def check_lane_bodies(kc, oracle, h, Ls=(3, 64, 128)):
    """Check 1 of the feature: the ring lane bodies against the oracle, every ring of the issue over the whole lane mix."""
    for L in Ls:
        octx = oracle.ctx(h, L)
        keys = make_keys(octx, "kr-%d" % L)
        a, b, c, d, e = keys
        lanes = lane_mix(octx, keys, "kr-%d" % L)
        proofs = b"".join(p for _, p, _ in lanes)
        a1 = 184 + 40 * 3 + 8
        for ring in ([a], [a, b], [b, a], [a, b, c, d]):
            st, ok, kp, cand, _ = host_ring_verify(kc, h, L, ring, proofs)
            for i, (name, proof, _) in enumerate(lanes):
                est, ekey, ekp = oracle_ring_verdict(octx, ring, proof)
                assert (st[i], ok[i], kp[32 * i:32 * i + 32]) == (est, ekey, ekp), (L, len(ring), name)
                if est in (0, 7):          # candidate k = the A1 element of the transcript the oracle builds under sk_k
                    for k in range(1, len(ring)):
                        tro = octx.verify_spend(ring[k], proof, True)[2]
                        got = cand[32 * (i * (len(ring) - 1) + k - 1):][:32]
                        assert got == tro[a1:a1 + 32], (L, len(ring), name, k)
        names = [n for n, _, _ in lanes]
        st, ok, _, _, _ = host_ring_verify(kc, h, L, [a, b, c, d], proofs)
        assert dict(zip(names, zip(st, ok))) == {"a": (0, 0), "b": (0, 1), "c": (0, 2), "stranger": (7, 255), "tampered": (7, 255), "b2": (0, 1),
                                                "identity": (6, 255), "undecodable": (255, 255)}


def check_incremental_hash(kc, oracle, Ls=(3, 5, 6, 30, 64, 100, 128)):
    """Check 3: scalar and 16-lane incremental routines == oracle.blake3 of the patched message, within the compression bound."""
    for L in Ls:
        length = 184 + 40 * (6 + 3 * L)
        chunks = (length + 1023) // 1024
        for t in range(3):
            msg = shake("kr-b3-%d-%d" % (L, t), length)
            rep = shake("kr-b3-rep-%d-%d" % (L, t), 32)
            off = 184 + 40 * 3 + 8
            plain = C.create_string_buffer(64); sca = C.create_string_buffer(64); x16 = C.create_string_buffer(64)
            comp = (C.c_uint64 * 2)()
            assert kc.hc_blake3_patched(msg, length, off, rep, plain, sca, x16, comp) == 1
            patched = msg[:off] + rep + msg[off + 32:]
            assert plain.raw == oracle.blake3(msg, 64), L
            assert sca.raw == oracle.blake3(patched, 64), L
            assert x16.raw == oracle.blake3(patched, 64), L
            bound = 16 + (chunks - 1).bit_length() + 1
            assert 0 < comp[0] <= bound and 0 < comp[1] <= bound, (L, list(comp), bound)
