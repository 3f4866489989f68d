// return_replay_lanes.h — the per-lane bodies of the replayable partial refunds (kernels in k_return_replay.hip, engine side
// in replay_impl.inc and admit_replay_impl.inc), as functions that also compile under g++ (tests/hostcheck/return_replay_check.cpp runs,
// counts and sanitizes them; the replay_lanes.h pattern).
//
// A replay form may return t <= s credits once t is part of BOTH the receipt's tag and the nonce derivation: the receipt then pins the
// amount a spend was answered with, and two different amounts for one (key, k, K') never share the nonce e.  Write t^ = t mod l.
//   t^ == 0   the tag and the nonces are the v1 hashes of replay_lanes.h (replay_tag, replay_nonce), bit for bit
//   t^ != 0   tag_t   = BLAKE3(LABEL_TAG_T | k | enc(K') | t^)[0:32], top nibble cleared                      (128-byte message, 2 blocks)
//             nonce_t = BLAKE3-XOF(LABEL_NONCE_T | nonce_key | key | k | enc(K') | t^, 128)                    (224-byte message, 4 blocks)
// t is public (it travels in the RefundReturn), so the branch on t^ == 0 is a branch on public data.
//   return_replay_tag_lane    lane = item        replay_tag_lane with the lane's t (ReplayDeriveArgs::t; null: every t = 0)
//   return_replay_nonce_lane  lane = item        replay_nonce_lane likewise
//   kprime_tag_return_lane    lane = candidate   kprime_tag_lane with the candidate's t, gathered by the same idx as its reduced nullifier
// Nothing is restated: the v1 hashes, the loads and the point arithmetic are those of replay_lanes.h and admit_replay_lanes.h.
#pragma once
#include "admit_replay_lanes.h"

namespace act {

// word i of a domain label of the _t hashes, zero-padded to 32 bytes
ACT_HD uint32_t return_replay_label_word(bool nonce, int i) {
  constexpr char TAG[33] = "act-mi355x/receipt-t/v1";
  constexpr char NONCE[33] = "act-mi355x/refund-nonce-t/v1";
  uint32_t w = 0;
  for (int b = 0; b < 4; b++) w |= (uint32_t)(uint8_t)(nonce ? NONCE[4 * i + b] : TAG[4 * i + b]) << (8 * b);
  return w;
}
ACT_HD bool return_replay_zero(const uint32_t t[8]) { uint32_t d = 0; for (int i = 0; i < 8; i++) d |= t[i]; return d == 0; }

// ---- the two hashes, t reduced and not zero ---------------------------------------------------------------------------------------------
ACT_HD void replay_tag_t(uint32_t tag[8], const uint32_t k[8], const uint32_t kp[8], const uint32_t t[8]) {
  uint32_t m[16], cv[8], o[16];
  for (int i = 0; i < 8; i++) { m[i] = return_replay_label_word(false, i); m[8 + i] = k[i]; cv[i] = b3_iv(i); }
  b3_compress(o, cv, m, 0u, 0u, 64u, B3_CHUNK_START);
  for (int i = 0; i < 8; i++) { cv[i] = o[i]; m[i] = kp[i]; m[8 + i] = t[i]; }
  b3_compress(o, cv, m, 0u, 0u, 64u, B3_CHUNK_END | B3_ROOT);
  for (int i = 0; i < 8; i++) tag[i] = o[i];
  tag[7] &= 0x0FFFFFFFu;
}
// out[0..16) = output block 0 of the root, out[16..32) = output block 1, as replay_nonce
ACT_HD void replay_nonce_t(uint32_t out[32], const uint32_t nonce_key[8], const uint32_t key[16], const uint32_t k[8], const uint32_t kp[8], const uint32_t t[8]) {
  uint32_t m[16], cv[8], o[16];
  for (int i = 0; i < 8; i++) { m[i] = return_replay_label_word(true, i); m[8 + i] = nonce_key[i]; cv[i] = b3_iv(i); }
  b3_compress(o, cv, m, 0u, 0u, 64u, B3_CHUNK_START);
  for (int i = 0; i < 8; i++) cv[i] = o[i];
  for (int i = 0; i < 16; i++) m[i] = key[i];
  b3_compress(o, cv, m, 0u, 0u, 64u, 0u);
  for (int i = 0; i < 8; i++) { cv[i] = o[i]; m[i] = k[i]; m[8 + i] = kp[i]; }
  b3_compress(o, cv, m, 0u, 0u, 64u, 0u);
  for (int i = 0; i < 8; i++) { cv[i] = o[i]; m[i] = t[i]; m[8 + i] = 0; }
  b3_compress(out, cv, m, 0u, 0u, 32u, B3_CHUNK_END | B3_ROOT);
  b3_compress(out + 16, cv, m, 1u, 0u, 32u, B3_CHUNK_END | B3_ROOT);
}
// v1 or _t by t^ == 0
ACT_HD void return_replay_tag(uint32_t tag[8], const uint32_t k[8], const uint32_t kp[8], const uint32_t t[8]) {
  if (return_replay_zero(t)) replay_tag(tag, k, kp); else replay_tag_t(tag, k, kp, t);
}
ACT_HD void return_replay_nonce(uint32_t out[32], const uint32_t nonce_key[8], const uint32_t key[16], const uint32_t k[8], const uint32_t kp[8], const uint32_t t[8]) {
  if (return_replay_zero(t)) replay_nonce(out, nonce_key, key, k, kp); else replay_nonce_t(out, nonce_key, key, k, kp, t);
}
// lane i's t^: 32 bytes at any alignment, reduced as the screen reduces them (null_load_key); a.t null: zero
ACT_HD void return_replay_load_t(uint32_t t[8], const uint8_t* base, size_t i) {
  if (base) null_load_key(t, base + i * 32);
  else for (int j = 0; j < 8; j++) t[j] = 0;
}

// ---- tag and nonce per lane: replay_tag_lane / replay_nonce_lane with the lane's t -------------------------------------------------------
ACT_HD void return_replay_tag_lane(const ReplayDeriveArgs& a, uint32_t i) {
  if (i >= a.n) return;
  uint32_t tg[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (replay_lane_live(a, i)) {      // (a dead lane's t is never read)
    uint32_t k[8], kp[8], t[8];
    null_load_key(k, a.nul + (size_t)i * a.stride);
    replay_load32(kp, a.kp + (size_t)i * 32);
    return_replay_load_t(t, a.t, i);
    return_replay_tag(tg, k, kp, t);
  }
  store32_bytes(a.out + (size_t)i * 32, tg);
}
ACT_HD void return_replay_nonce_lane(const ReplayDeriveArgs& a, uint32_t i) {
  if (i >= a.n) return;
  uint32_t o[32];
  for (int j = 0; j < 32; j++) o[j] = 0;
  if (replay_lane_live(a, i)) {
    uint32_t k[8], kp[8], nk[8], key[16], t[8];
    const uint32_t* s = reinterpret_cast<const uint32_t*>(a.secrets);
    const uint32_t j = a.kidx[i];
    for (int w = 0; w < 8; w++) nk[w] = s[w];
    for (int w = 0; w < 16; w++) key[w] = s[8 + 16 * j + w];
    null_load_key(k, a.nul + (size_t)i * a.stride);
    replay_load32(kp, a.kp + (size_t)i * 32);
    return_replay_load_t(t, a.t, i);
    return_replay_nonce(o, nk, key, k, kp, t);
  }
  uint8_t* dst = a.out + (size_t)i * 128;
  for (int q = 0; q < 4; q++) store32_bytes(dst + 32 * q, o + 8 * q);
}

// ---- the candidate's tag in the admission stage: kprime_tag_lane with the candidate's t ---------------------------------------------------
ACT_HD void kprime_tag_return_lane(const KprimeArgs& a, uint32_t c) {
  if (c >= a.s.n) return;
  uint32_t enc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tg[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const bool bad = (a.s.flags[c] & FLAG_UNDECODABLE) != 0;
  if (!bad) {
    uint32_t k[8], t[8];
    const size_t at = a.idx ? a.idx[c] : c;
    ristretto_encode(enc, spend_tail_horner(a.s, c, 0, a.s.P.L, 0));
    null_load_key(k, a.kred + at * 32);
    return_replay_load_t(t, a.t, at);
    return_replay_tag(tg, k, enc, t);
  }
  store32_bytes(a.kp + (size_t)c * 32, enc);
  store32_bytes(a.tag + (size_t)c * 32, tg);
  a.mark[c] = bad ? 1 : 0;
}

#if defined(__HIPCC__)
// launchers (k_return_replay.hip): one lane per thread; 256 per workgroup for the two derive kernels, 64 for the candidates' tags
void launch_return_replay_tag(const ReplayDeriveArgs& a, hipStream_t s);
void launch_return_replay_nonce(const ReplayDeriveArgs& a, hipStream_t s);
void launch_kprime_tag_return(const KprimeArgs& a, hipStream_t s);
#endif

}  // namespace act
