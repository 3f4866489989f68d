// return_lanes.h — partial refunds: the per-lane pieces the RefundReturn path adds to the screen, the signing phase and the
// client verifier, as functions that also compile under g++ (tests/hostcheck/return_check.cpp runs and counts them).
//
// The issuer reserved s credits and returns t <= s of them: it signs X_A = g + K' + t h1 instead of g + K' (src/lib.rs:848), where
// K' = sum 2^j Com_j commits to c - s, so the client's next token holds c - s + t.  Both parties know t -- it travels in the record --
// so, like the amount c of an issuance, its digits may address a table: t h1 is an ADDRESSED fixed-base product on both sides.
//   return_exceeds       t > s as 256-bit integers, both reduced mod l: the screen's rule (ACT_STATUS_RETURN_TOO_BIG) and the client's (8)
//   return_xa            X_A + t h1: one fixed-base product on h1 and one point addition
//   return_client_finish the client's phase B over a 160-byte record: challenge == gamma, t <= s, token balance (m + t) mod l
#pragma once
#include "kernels.h"

namespace act {

constexpr uint8_t RETURN_TOO_BIG = 249;         // ACT_STATUS_RETURN_TOO_BIG

// t > s, both canonical (below l < 2^253): from the top word down, the first word that differs decides.  Public values on both sides.
ACT_HD bool return_exceeds(const uint32_t t[8], const uint32_t s[8]) {
  bool gt = false, decided = false;
  for (int i = 7; i >= 0; i--) {
    const bool ne = t[i] != s[i];
    if (!decided && ne) gt = t[i] > s[i];
    decided = decided || ne;
  }
  return gt;
}
// the same on two scalars as they lie in memory (32 little-endian bytes each, any value below 2^256: reduced here)
ACT_HD bool return_exceeds_bytes(const uint8_t* t, const uint8_t* s) {
  const sc tv = load_sc(t), sv = load_sc(s);
  return return_exceeds(tv.v, sv.v);
}

// X_A of a RefundReturn from the X_A of a Refund (g + K'): + t h1.  t = 0 adds the identity: the same group element, so the same bytes.
ACT_HD ge return_xa(const DevParams& P, const ge& xa, const sc& t) {
  return ge_add(xa, fixed_base_acc(ge_identity(), P.tab[BASE_H1], t));
}

// The client's phase B over RefundReturn records (k_client_b's part; a.resp has 160-byte records A | e | gamma | z | t, a.proofs the
// spend proofs whose field 1 is s).  The order of the refusals: an undecodable point, then the proof (InvalidRefundProof, 4), then the
// bound -- a record that was altered after signing fails its proof whatever its t says, and only a VALIDLY signed t > s is reported as
// an amount the client could never prove in range (AmountTooBigError, 8).
ACT_HD void return_client_finish(const ClientArgs& a, uint32_t p, const uint32_t w[16]) {
  const uint8_t* resp = a.resp + (size_t)p * 160;
  const sc gamma = load_sc(resp + 64), t = load_sc(resp + 128);
  const sc s = load_sc(a.proofs + (size_t)p * ProofLayout{a.P.L}.bytes() + 32);
  uint8_t stt = 0;
  if (a.flags[p] & FLAG_UNDECODABLE) stt = 255;
  else if (!sc_equal(sc_from_wide_words(w), gamma)) stt = 4;      // InvalidRefundProof
  else if (return_exceeds(t.v, s.v)) stt = 8;                     // AmountTooBigError
  a.status[p] = stt;
  uint8_t* out = a.out_token + (size_t)p * 160;
  if (stt) { for (int i = 0; i < 160; i += 32) zero8(out + i); return; }
  const uint8_t* pre = a.pre + (size_t)p * 96;                    // r | k | m
  uint32_t enc[8];
  load8(enc, resp); store8(out, enc);
  store_sc(out + 32, load_sc(resp + 32));
  store_sc(out + 64, load_sc(pre + 32));
  store_sc(out + 96, load_sc(pre));
  store_sc(out + 128, sc_add(load_sc(pre + 64), t));              // c - s + t
}

}  // namespace act
