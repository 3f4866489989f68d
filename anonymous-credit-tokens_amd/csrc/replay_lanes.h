// replay_lanes.h — the per-lane bodies of the replayable redemption (k_replay.hip; engine side in replay_impl.inc), as functions that
// also compile under g++ (tests/hostcheck/replay_check.cpp runs and sanitizes them; the copy_lanes.h / admit_lanes.h pattern).
//
// A refund becomes replayable without being stored: its 128 nonce bytes are a keyed function of what is signed, and a
// second nullifier set (the receipts) remembers for WHICH enc(K') a nullifier was recorded.
//   replay_tag_lane      lane = item   tag   = BLAKE3(LABEL_TAG | k | enc(K'))[0:32], top nibble cleared        (96-byte message)
//   replay_nonce_lane    lane = item   nonce = BLAKE3-XOF(LABEL_NONCE | nonce_key | key | k | enc(K'), 128)     (192-byte message)
//   replay_resolve_lane  lane = item   (verdict, the set's answer, the receipts' answer) -> what the redemption tail merges
// k is the nullifier reduced mod l (the set's key, null_probe.h); key is the 64-byte record x | enc(w) the lane is signed with.  All
// inputs have fixed length, so nothing is length-prefixed; both messages are one chunk, hashed block by block from registers.
#pragma once
#include "kernels.h"
#include "null_probe.h"

namespace act {

constexpr uint32_t REPLAY_SECRET_BYTES = 32 + 64 * 4;                     // nonce_key, then the ring's records (ACT_KEYRING_MAX of them)

// word i of a domain label, zero-padded to 32 bytes
ACT_HD uint32_t replay_label_word(bool nonce, int i) {
  constexpr char TAG[33] = "act-mi355x/receipt/v1";
  constexpr char NONCE[33] = "act-mi355x/refund-nonce/v1";
  uint32_t w = 0;
  for (int b = 0; b < 4; b++) w |= (uint32_t)(uint8_t)(nonce ? NONCE[4 * i + b] : TAG[4 * i + b]) << (8 * b);
  return w;
}
// 32 bytes at any alignment, not reduced (enc(K') is a point encoding)
ACT_HD void replay_load32(uint32_t w[8], const uint8_t* p) {
  if ((reinterpret_cast<uintptr_t>(p) & 3u) == 0) { const uint32_t* q = reinterpret_cast<const uint32_t*>(p); for (int i = 0; i < 8; i++) w[i] = q[i]; }
  else for (int i = 0; i < 8; i++) w[i] = (uint32_t)p[4 * i] | (uint32_t)p[4 * i + 1] << 8 | (uint32_t)p[4 * i + 2] << 16 | (uint32_t)p[4 * i + 3] << 24;
}

// ---- the two hashes -------------------------------------------------------------------------------------------------------------------
// byte 31 &= 0x0F: the tag is below 2^252 < l, so the receipts set's own reduction of its keys is the identity
ACT_HD void replay_tag(uint32_t tag[8], const uint32_t k[8], const uint32_t kp[8]) {
  uint32_t m[16], cv[8], o[16];
  for (int i = 0; i < 8; i++) { m[i] = replay_label_word(false, i); m[8 + i] = k[i]; cv[i] = b3_iv(i); }
  b3_compress(o, cv, m, 0u, 0u, 64u, B3_CHUNK_START);
  for (int i = 0; i < 8; i++) { cv[i] = o[i]; m[i] = kp[i]; m[8 + i] = 0; }
  b3_compress(o, cv, m, 0u, 0u, 32u, B3_CHUNK_END | B3_ROOT);
  for (int i = 0; i < 8; i++) tag[i] = o[i];
  tag[7] &= 0x0FFFFFFFu;
}
// out[0..16) = output block 0 of the root, out[16..32) = output block 1 (the root compression again with counter 1, as k_xof_expand)
ACT_HD void replay_nonce(uint32_t out[32], const uint32_t nonce_key[8], const uint32_t key[16], const uint32_t k[8], const uint32_t kp[8]) {
  uint32_t m[16], cv[8], o[16];
  for (int i = 0; i < 8; i++) { m[i] = replay_label_word(true, i); m[8 + i] = nonce_key[i]; cv[i] = b3_iv(i); }
  b3_compress(o, cv, m, 0u, 0u, 64u, B3_CHUNK_START);
  for (int i = 0; i < 8; i++) cv[i] = o[i];
  for (int i = 0; i < 16; i++) m[i] = key[i];
  b3_compress(o, cv, m, 0u, 0u, 64u, 0u);
  for (int i = 0; i < 8; i++) { cv[i] = o[i]; m[i] = k[i]; m[8 + i] = kp[i]; }
  b3_compress(out, cv, m, 0u, 0u, 64u, B3_CHUNK_END | B3_ROOT);
  b3_compress(out + 16, cv, m, 1u, 0u, 64u, B3_CHUNK_END | B3_ROOT);
}

// ---- tag and nonce per lane -----------------------------------------------------------------------------------------------------------
// A lane takes part when its status byte is 0 and (kidx given) its key index is below nkeys; every other lane gets zeros.
struct ReplayDeriveArgs {
  uint32_t n, stride, nkeys;          // nullifier i at nul + i * stride (32 bytes: the `k` field of a SpendProof record, or a dense array)
  const uint8_t* nul; const uint8_t* kp;      // kp: n * 32, enc(K')
  const uint8_t* st;                  // n status bytes
  const uint8_t* kidx;                // n key indices: nullable for the tag (it does not depend on the key), required for the nonce
  const uint8_t* secrets;             // the nonce: REPLAY_SECRET_BYTES, 4-byte aligned -- nonce_key | nkeys records of 64 bytes
  uint8_t* out;                       // n * 32 tags or n * 128 nonces, any alignment
  const uint8_t* t;                   // the return forms (return_replay_lanes.h) only: nullable, n returned amounts of 32 bytes at any alignment
};
ACT_HD bool replay_lane_live(const ReplayDeriveArgs& a, uint32_t i) { return a.st[i] == 0 && (!a.kidx || a.kidx[i] < a.nkeys); }

ACT_HD void replay_tag_lane(const ReplayDeriveArgs& a, uint32_t i) {
  if (i >= a.n) return;
  uint32_t t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (replay_lane_live(a, i)) {
    uint32_t k[8], kp[8];
    null_load_key(k, a.nul + (size_t)i * a.stride);
    replay_load32(kp, a.kp + (size_t)i * 32);
    replay_tag(t, k, kp);
  }
  store32_bytes(a.out + (size_t)i * 32, t);
}
ACT_HD void replay_nonce_lane(const ReplayDeriveArgs& a, uint32_t i) {
  if (i >= a.n) return;
  uint32_t o[32];
  for (int j = 0; j < 32; j++) o[j] = 0;
  if (replay_lane_live(a, i)) {
    uint32_t k[8], kp[8], nk[8], key[16];
    const uint32_t* s = reinterpret_cast<const uint32_t*>(a.secrets);
    const uint32_t j = a.kidx[i];
    for (int w = 0; w < 8; w++) nk[w] = s[w];
    for (int w = 0; w < 16; w++) key[w] = s[8 + 16 * j + w];
    null_load_key(k, a.nul + (size_t)i * a.stride);
    replay_load32(kp, a.kp + (size_t)i * 32);
    replay_nonce(o, nk, key, k, kp);
  }
  uint8_t* dst = a.out + (size_t)i * 128;
  for (int q = 0; q < 4; q++) store32_bytes(dst + 32 * q, o + 8 * q);
}

// ---- what the two sets' answers make of a verified lane ---------------------------------------------------------------------------------
// verdict: the verification's status; spent: the nullifier set's answer for k (0 fresh and now recorded, 1 spent, 2 = ACT_NULLIFIER_
// UNDETERMINED); found: the receipts set holds the lane's tag.
//   skip      the mask of the receipts insert: a receipt is written ONLY for a lane whose k was fresh -- a double spender must not be
//             able to plant the tag of its second K' and collect on a later retry.  Does not depend on `found`.
//   sp        what redeem_tail's merge reads: 0 for fresh AND replayed lanes (both are signed), 1 for a double spend, 2 undetermined
//   replayed  1: k was spent for this very K' -- the lane is signed again and, the nonces being derived, gets the same refund
struct ReplayResolved { uint8_t skip, sp, replayed; };
ACT_HD ReplayResolved replay_resolve(uint8_t verdict, uint8_t spent, uint8_t found) {
  ReplayResolved r{1, 0, 0};
  if (verdict != 0) return r;
  if (spent == 0) { r.skip = 0; return r; }
  if (spent == 1 && found) { r.replayed = 1; return r; }
  r.sp = spent;
  return r;
}
struct ReplayResolveArgs {
  uint32_t n;
  const uint8_t* st; const uint8_t* spent;
  const uint8_t* found;               // null: the pass in front of the receipts insert, which writes skip[]; else the pass behind the look-up
  uint8_t* skip; uint8_t* sp; uint8_t* replayed;
};
ACT_HD void replay_resolve_lane(const ReplayResolveArgs& a, uint32_t i) {
  if (i >= a.n) return;
  const ReplayResolved r = replay_resolve(a.st[i], a.spent[i], a.found ? a.found[i] : (uint8_t)0);
  if (!a.found) { a.skip[i] = r.skip; return; }
  a.sp[i] = r.sp; a.replayed[i] = r.replayed;
}

#if defined(__HIPCC__)
// launchers (k_replay.hip): one lane per thread, 256 per workgroup
void launch_replay_tag(const ReplayDeriveArgs& a, hipStream_t s);
void launch_replay_nonce(const ReplayDeriveArgs& a, hipStream_t s);
void launch_replay_resolve(const ReplayResolveArgs& a, hipStream_t s);
#endif

}  // namespace act
