// client_ring_return_lanes.h — key rotation and partial refunds together on the client: the ring form of phase B over
// 160-byte RefundReturn records, as a function that also compiles under g++ (tests/hostcheck/return_ring_check.cpp runs, counts and
// sanitizes it).
//
// A RefundReturn (A | e | gamma | z | t) names no key, like a Refund.  t enters the check through X_A = g + K' + t h1 alone
// (return_lanes.h return_xa), and X_A does not depend on the issuer's key: phase A runs once under ring key 0 with ClientArgs::with_t,
// and per extra key an item costs exactly what a plain refund costs -- client_ring_cand_lane and client_ring_hash_lane
// (client_ring_lanes.h), which read e, gamma and z at the record stride client_ring_resp_stride(label, with_t) gives.  What differs is
// the finish: the token holds (m + t) mod l, and behind the proof stands the bound t <= s.
#pragma once
#include "client_ring_lanes.h"
#include "return_lanes.h"

namespace act {

// client_ring_finish_lane and return_client_finish in one, in the latter's order of refusals: an undecodable point (255), then the
// proof under EVERY ring key (InvalidRefundProof, 4), then the bound -- only a t that some ring key validly signed can be reported as
// t > s (AmountTooBigError, 8; s: field 1 of the lane's proof record).  A rejected lane gets an all-zero token and KEY_NONE.
ACT_HD void client_ring_return_finish_lane(const ClientRingArgs& r, uint32_t p) {
  const ClientArgs& a = r.c;
  const uint8_t* resp = a.resp + (size_t)p * client_ring_resp_stride(LABEL_REFUND, 1);
  const sc gamma = load_sc(resp + 64), t = load_sc(resp + 128);
  const sc s = load_sc(a.proofs + (size_t)p * ProofLayout{a.P.L}.bytes() + 32);
  const uint32_t match = client_ring_match(r, p, gamma);
  uint8_t stt = 0;
  if (a.flags[p] & FLAG_UNDECODABLE) stt = 255;
  else if (match == KEY_NONE) stt = 4;                            // InvalidRefundProof under every ring key
  else if (return_exceeds(t.v, s.v)) stt = 8;                     // AmountTooBigError
  a.status[p] = stt;
  r.out_key[p] = stt == 0 ? (uint8_t)match : KEY_NONE;
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

#if defined(__HIPCC__)
void launch_client_ring_return_finish(const ClientRingArgs& r, hipStream_t s);
#endif

}  // namespace act
