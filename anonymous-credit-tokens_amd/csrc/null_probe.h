// null_probe.h — the key and slot functions of the nullifier set (nullifier_impl.inc says what the table is): how a 32-byte nullifier
// becomes the set's key, where its probe sequence starts, and the read-only probe.  Shared by the set's own kernels (engine.hip) and
// by the admission screen (k_admit.hip, admit_lanes.h); compiles under g++ like the other lane headers.
#pragma once
#include "kernels.h"

struct NullSalt { uint32_t w[4]; };

// the set's key of a nullifier: the scalar, reduced mod l (Scalar::from_bytes_mod_order)
ACT_HD void null_load_key(uint32_t w[8], const uint8_t* p) {
  uint32_t r[8];
  if ((reinterpret_cast<uintptr_t>(p) & 3u) == 0) { const uint32_t* q = reinterpret_cast<const uint32_t*>(p); for (int i = 0; i < 8; i++) r[i] = q[i]; }
  else for (int i = 0; i < 8; i++) r[i] = (uint32_t)p[4 * i] | (uint32_t)p[4 * i + 1] << 8 | (uint32_t)p[4 * i + 2] << 16 | (uint32_t)p[4 * i + 3] << 24;
  const act::sc k = act::sc_from_words(r);
  for (int i = 0; i < 8; i++) w[i] = k.v[i];
}
// SipHash-1-3 (one compression round per 8-byte block, three finalisation rounds) of the 32-byte key under salt[0..3]
ACT_HD uint64_t null_hash(const uint32_t w[8], const uint32_t salt[4]) {
  const uint64_t k0 = (uint64_t)salt[0] | (uint64_t)salt[1] << 32, k1 = (uint64_t)salt[2] | (uint64_t)salt[3] << 32;
  uint64_t v0 = k0 ^ 0x736f6d6570736575ull, v1 = k1 ^ 0x646f72616e646f6dull, v2 = k0 ^ 0x6c7967656e657261ull, v3 = k1 ^ 0x7465646279746573ull;
  auto rotl = [](uint64_t x, int b) { return (x << b) | (x >> (64 - b)); };
  auto round = [&]() {
    v0 += v1; v1 = rotl(v1, 13); v1 ^= v0; v0 = rotl(v0, 32);
    v2 += v3; v3 = rotl(v3, 16); v3 ^= v2;
    v0 += v3; v3 = rotl(v3, 21); v3 ^= v0;
    v2 += v1; v1 = rotl(v1, 17); v1 ^= v2; v2 = rotl(v2, 32);
  };
  for (int i = 0; i < 4; i++) { const uint64_t m = (uint64_t)w[2 * i] | (uint64_t)w[2 * i + 1] << 32; v3 ^= m; round(); v0 ^= m; }
  const uint64_t last = (uint64_t)32 << 56;                                // length byte, no tail bytes
  v3 ^= last; round(); v0 ^= last;
  v2 ^= 0xff; round(); round(); round();
  return v0 ^ v1 ^ v2 ^ v3;
}
ACT_HD bool null_eq(const uint32_t a[8], const uint32_t b[8]) { uint32_t d = 0; for (int i = 0; i < 8; i++) d |= a[i] ^ b[i]; return d == 0; }

// Read-only look-up of the reduced key w: probes from the persistent table's start slot until the key (found) or an empty slot
// (absent); no write to the set.  The caller holds the set's lock, so no slot is being written.
ACT_HD bool null_probe_contains(const uint32_t w[8], const uint32_t* tab_keys, const uint32_t* tab_state, uint32_t tab_cap, const uint32_t salt[4]) {
  uint32_t o[8];
  uint32_t t = (uint32_t)(null_hash(w, salt) >> 32) & (tab_cap - 1);
  for (uint32_t probes = 0; probes < tab_cap; probes++) {
    const uint32_t st = tab_state[t];
    if (st == 0u) return false;
    if ((st & 0xFFu) == 2u) {
      const uint32_t* src = tab_keys + (size_t)t * 8;
      for (int k = 0; k < 8; k++) o[k] = src[k];
      if (null_eq(w, o)) return true;
    }
    t = (t + 1) & (tab_cap - 1);
  }
  return false;
}
