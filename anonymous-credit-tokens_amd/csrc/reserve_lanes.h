// reserve_lanes.h — the per-lane bodies of reserve and settle (kernels in k_reserve.hip, engine side in reserve_impl.inc), as
// functions that also compile under g++ (tests/hostcheck/reserve_check.cpp runs and sanitizes them; the return_replay_lanes.h pattern).
//
// A metered service records a spend of s now and signs the partial refund t <= s when the work is done.  Between the two calls stands a
// reservation record of 96 public bytes, k^ | enc(K') | s^ (k^, s^: nullifier and charge reduced mod l), and three keys in the receipts:
//   tag_res = BLAKE3(LABEL_RES | k^ | enc(K') | s^)[0:32], top nibble cleared          (128-byte message, 2 blocks: the shape of replay_tag_t)
//   marker  = BLAKE3(LABEL_SETTLED | k^ | enc(K'))[0:32], top nibble cleared           (96-byte message: the shape of replay_tag)
//   the amount tag of (k^, enc(K'), t^): return_replay_tag itself, as the nonces are return_replay_nonce's
//   reserve_sred_lane        lane = item        s^ of every lane, as the screen reduces it, into a dense array beside the reduced nullifiers
//   kprime_tag_reserve_lane  lane = candidate   kprime_tag_return_lane with tag_res: the candidate's s^ gathered by the same idx as its k^
//   reserve_tag_lane         lane = item        tag_res of the tail's lanes (ReplayDeriveArgs::t carries s here)
//   reserve_emit_lane        lane = item        the 96-byte record of an accepted lane, zeros for every other
//   settle_prep_lane         lane = item        one pass over a reservation: the three reductions, the key-index rule, t^ > s^, the three tags
//   settle_found_lane / settle_merge_lane       what the receipts' answers make of a lane
// Nothing is restated: reductions, loads and the hashes' compression are those of null_probe.h, replay_lanes.h and return_replay_lanes.h.
#pragma once
#include "return_replay_lanes.h"

namespace act {

constexpr uint8_t SETTLE_NOT_RESERVED = 248;          // ACT_STATUS_NOT_RESERVED
constexpr uint8_t SETTLE_OTHER_AMOUNT = 247;          // ACT_STATUS_SETTLED_OTHER_AMOUNT
constexpr uint32_t RESERVATION_BYTES = 96;

// word i of a domain label of the two hashes, zero-padded to 32 bytes
ACT_HD uint32_t reserve_label_word(bool marker, int i) {
  constexpr char RES[33] = "act-mi355x/reservation/v1";
  constexpr char SETTLED[33] = "act-mi355x/settled/v1";
  uint32_t w = 0;
  for (int b = 0; b < 4; b++) w |= (uint32_t)(uint8_t)(marker ? SETTLED[4 * i + b] : RES[4 * i + b]) << (8 * b);
  return w;
}

// ---- the two hashes -------------------------------------------------------------------------------------------------------------------
ACT_HD void reserve_tag(uint32_t tag[8], const uint32_t k[8], const uint32_t kp[8], const uint32_t s[8]) {
  uint32_t m[16], cv[8], o[16];
  for (int i = 0; i < 8; i++) { m[i] = reserve_label_word(false, i); m[8 + i] = k[i]; cv[i] = b3_iv(i); }
  b3_compress(o, cv, m, 0u, 0u, 64u, B3_CHUNK_START);
  for (int i = 0; i < 8; i++) { cv[i] = o[i]; m[i] = kp[i]; m[8 + i] = s[i]; }
  b3_compress(o, cv, m, 0u, 0u, 64u, B3_CHUNK_END | B3_ROOT);
  for (int i = 0; i < 8; i++) tag[i] = o[i];
  tag[7] &= 0x0FFFFFFFu;
}
ACT_HD void settle_marker(uint32_t tag[8], const uint32_t k[8], const uint32_t kp[8]) {
  uint32_t m[16], cv[8], o[16];
  for (int i = 0; i < 8; i++) { m[i] = reserve_label_word(true, i); m[8 + i] = k[i]; cv[i] = b3_iv(i); }
  b3_compress(o, cv, m, 0u, 0u, 64u, B3_CHUNK_START);
  for (int i = 0; i < 8; i++) { cv[i] = o[i]; m[i] = kp[i]; m[8 + i] = 0; }
  b3_compress(o, cv, m, 0u, 0u, 32u, B3_CHUNK_END | B3_ROOT);
  for (int i = 0; i < 8; i++) tag[i] = o[i];
  tag[7] &= 0x0FFFFFFFu;
}

// ---- reserve --------------------------------------------------------------------------------------------------------------------------
// s of item i in the 32 bytes behind its k (AdmitScreenArgs::ks / stride), reduced into sred + i * 32 (the engine's own allocation)
struct ReserveSredArgs { uint32_t n, stride; const uint8_t* ks; uint8_t* sred; };
ACT_HD void reserve_sred_lane(const ReserveSredArgs& a, uint32_t i) {
  if (i >= a.n) return;
  uint32_t s[8];
  null_load_key(s, a.ks + (size_t)i * a.stride + 32);
  store32_bytes(a.sred + (size_t)i * 32, s);
}

// the candidate's tag in the admission stage: KprimeArgs::t carries the charges, candidate c's at t + idx[c] * 32
ACT_HD void kprime_tag_reserve_lane(const KprimeArgs& a, uint32_t c) {
  if (c >= a.s.n) return;
  uint32_t enc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tg[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const bool bad = (a.s.flags[c] & FLAG_UNDECODABLE) != 0;
  if (!bad) {
    uint32_t k[8], s[8];
    const size_t at = a.idx ? a.idx[c] : c;
    ristretto_encode(enc, spend_tail_horner(a.s, c, 0, a.s.P.L, 0));
    null_load_key(k, a.kred + at * 32);
    null_load_key(s, a.t + at * 32);
    reserve_tag(tg, k, enc, s);
  }
  store32_bytes(a.kp + (size_t)c * 32, enc);
  store32_bytes(a.tag + (size_t)c * 32, tg);
  a.mark[c] = bad ? 1 : 0;
}

// the tail's tag: a.t carries the charges lane for lane (never null here)
ACT_HD void reserve_tag_lane(const ReplayDeriveArgs& a, uint32_t i) {
  if (i >= a.n) return;
  uint32_t tg[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (replay_lane_live(a, i)) {
    uint32_t k[8], kp[8], s[8];
    null_load_key(k, a.nul + (size_t)i * a.stride);
    replay_load32(kp, a.kp + (size_t)i * 32);
    null_load_key(s, a.t + (size_t)i * 32);
    reserve_tag(tg, k, kp, s);
  }
  store32_bytes(a.out + (size_t)i * 32, tg);
}

// the record of a lane whose merged status is 0, zeros for every other; the lane's status goes out with it
struct ReserveEmitArgs {
  uint32_t n, stride;                 // nullifier i at nul + i * stride
  const uint8_t* nul; const uint8_t* kp; const uint8_t* s;      // kp, s: n * 32 each
  const uint8_t* st;                  // n merged statuses
  uint8_t* out; uint8_t* status;      // n * 96 at any alignment, n
};
ACT_HD void reserve_emit_lane(const ReserveEmitArgs& a, uint32_t i) {
  if (i >= a.n) return;
  uint32_t k[8] = {0, 0, 0, 0, 0, 0, 0, 0}, kp[8] = {0, 0, 0, 0, 0, 0, 0, 0}, s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const uint8_t st = a.st[i];
  if (st == 0) {
    null_load_key(k, a.nul + (size_t)i * a.stride);
    replay_load32(kp, a.kp + (size_t)i * 32);
    null_load_key(s, a.s + (size_t)i * 32);
  }
  uint8_t* dst = a.out + (size_t)i * RESERVATION_BYTES;
  store32_bytes(dst, k); store32_bytes(dst + 32, kp); store32_bytes(dst + 64, s);
  a.status[i] = st;
}

// ---- settle ---------------------------------------------------------------------------------------------------------------------------
// One pass per reservation.  The order of the rules: the key index (SETTLE_NOT_RESERVED), then t^ > s^ with s^ from the record
// (RETURN_TOO_BIG); a lane that fails either gets zero tags and its record is not hashed.  All inputs are public.
struct SettlePrepArgs {
  uint32_t n, nkeys;
  const uint8_t* rec;                 // n * 96 at any alignment: k | enc(K') | s
  const uint8_t* kidx;                // n key indices, as reserve left them in out_key
  const uint8_t* t;                   // nullable (every amount zero): n * 32 at any alignment
  uint8_t* tag_res; uint8_t* marker; uint8_t* tag_amt;      // n * 32 each
  uint8_t* kp;                        // nullable: n * 32, enc(K') as a dense array for the nonce derivation and the signing step
  uint8_t* st;                        // n
};
ACT_HD uint8_t settle_prep_status(uint8_t kidx, uint32_t nkeys, const uint32_t t[8], const uint32_t s[8]) {
  if (kidx >= nkeys) return SETTLE_NOT_RESERVED;
  if (return_exceeds(t, s)) return RETURN_TOO_BIG;
  return 0;
}
ACT_HD void settle_prep_lane(const SettlePrepArgs& a, uint32_t i) {
  if (i >= a.n) return;
  const uint8_t* rec = a.rec + (size_t)i * RESERVATION_BYTES;
  uint32_t k[8], kp[8], s[8], t[8], tr[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tm[8] = {0, 0, 0, 0, 0, 0, 0, 0}, ta[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  null_load_key(k, rec);
  replay_load32(kp, rec + 32);
  null_load_key(s, rec + 64);
  return_replay_load_t(t, a.t, i);
  const uint8_t st = settle_prep_status(a.kidx[i], a.nkeys, t, s);
  if (st == 0) { reserve_tag(tr, k, kp, s); settle_marker(tm, k, kp); return_replay_tag(ta, k, kp, t); }
  store32_bytes(a.tag_res + (size_t)i * 32, tr);
  store32_bytes(a.marker + (size_t)i * 32, tm);
  store32_bytes(a.tag_amt + (size_t)i * 32, ta);
  if (a.kp) store32_bytes(a.kp + (size_t)i * 32, kp);
  a.st[i] = st;
}

// the reservation's look-up: a lane that passed the rules and whose tag_res the receipts do not hold was never reserved
struct SettleFoundArgs { uint32_t n; const uint8_t* found; uint8_t* st; };
ACT_HD void settle_found_lane(const SettleFoundArgs& a, uint32_t i) {
  if (i >= a.n) return;
  if (a.st[i] == 0 && !a.found[i]) a.st[i] = SETTLE_NOT_RESERVED;
}

// behind replay_resolve over (status, the marker's answer, the amount tag's answer): sp = 1 is a reservation settled with another amount
ACT_HD uint8_t settle_merge(uint8_t st, uint8_t sp) {
  if (st) return st;
  if (sp == 1) return SETTLE_OTHER_AMOUNT;
  return sp ? (uint8_t)252 : (uint8_t)0;      // ACT_STATUS_NULLIFIER_UNDETERMINED: the receipts could not answer for the marker
}
struct SettleMergeArgs { uint32_t n; const uint8_t* sp; uint8_t* st; };
ACT_HD void settle_merge_lane(const SettleMergeArgs& a, uint32_t i) {
  if (i >= a.n) return;
  a.st[i] = settle_merge(a.st[i], a.sp[i]);
}

#if defined(__HIPCC__)
// launchers (k_reserve.hip): one lane per thread; 256 per workgroup, 64 for the candidates' tags
void launch_reserve_sred(const ReserveSredArgs& a, hipStream_t s);
void launch_kprime_tag_reserve(const KprimeArgs& a, hipStream_t s);
void launch_reserve_tag(const ReplayDeriveArgs& a, hipStream_t s);
void launch_reserve_emit(const ReserveEmitArgs& a, hipStream_t s);
void launch_settle_prep(const SettlePrepArgs& a, hipStream_t s);
void launch_settle_found(const SettleFoundArgs& a, hipStream_t s);
void launch_settle_merge(const SettleMergeArgs& a, hipStream_t s);
#endif

}  // namespace act
