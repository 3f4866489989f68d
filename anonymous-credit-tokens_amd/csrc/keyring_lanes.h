// keyring_lanes.h — the per-lane bodies of the key-ring kernels (k_keyring.hip), as functions that also compile under g++
// (tests/hostcheck/keyring_check.cpp runs, counts and sanitizes them; the spend_lanes.h pattern).
//
// A SpendProof names no issuer key, and the issuer's x enters verification in ONE place: A1 = (e_bar - x gamma) A' + r2_bar B_bar
// (spend_lanes.h spend_prep_role_a, src/lib.rs:791-795).  While an issuer rotates its key a batch is therefore
// verified ONCE -- every kernel of spend_lanes.h under ring key 0, unchanged -- and per additional candidate key k a proof costs
//   ring_cand_lane    lane = (proof, k)   A1_k = A1_0 + ((x_0 - x_k) gamma) A', encoded into a side buffer: one chain_ct on A'
//   (b3_xof64_patched, blake3_hd.h)       the challenge hash of the transcript with A1 replaced: chunk 0 and its ancestors only
//   ring_finish_lane  lane = proof        nkeys challenges against gamma, the first match wins -> status, out_key
// No digit of any x_k selects an address or a branch (chain_ct); ring entries are only ever chosen by PUBLIC indices.
#pragma once
#include "spend_lanes.h"
#include "keyring.h"

namespace act {

// A1_k from what k_spend_prep left in the transcript.  decode(enc(A1_0)) is another representative of A1_0's Ristretto class, and the
// encoding of a sum does not depend on the representatives.  A proof whose A' does not decode is rejected by its flags whatever
// lands here.
ACT_HD void ring_cand_lane(const RingArgs& r, uint32_t gid) {
  const uint32_t extra = r.nkeys - 1u;
  const uint32_t p = gid / extra, k = gid % extra + 1u;
  if (p >= r.s.n) return;
  const SpendArgs& a = r.s;
  const ProofLayout pl{a.P.L};
  const SpendTranscript st{a.P.L};
  const uint8_t* rec = a.proofs + (size_t)p * pl.bytes();
  const uint8_t* el = a.tr + (size_t)p * a.tr_stride + 184;
  uint32_t wa[8], w1[8];
  load8(wa, rec + 32 * pl.a_prime());
  load8(w1, el + 40 * st.el_a1() + 8);
  ge A, A1;
  (void)ristretto_decode(A, wa);
  (void)ristretto_decode(A1, w1);
  const sc gamma = load_sc(rec + 32 * pl.gamma());
  ge acc[1] = {A1};
  sc sa[1] = {sc_mul(sc_sub(r.ring[0].x, r.ring[k].x), gamma)};
  chain_ct<1>(acc, A, sa);                                  // the scalar depends on two issuer keys: address-free (msm.h)
  uint32_t enc[8];
  ristretto_encode(enc, acc[0]);
  store8(r.cand + ((size_t)p * extra + (k - 1u)) * 32, enc);
}

// the hash of transcript p under ring key k >= 1 (device-transcript mode; the host mode runs b3_xof64_patched on its workers)
ACT_HD void ring_hash_lane(const RingArgs& r, uint32_t gid) {
  const uint32_t extra = r.nkeys - 1u;
  const uint32_t p = gid / extra, k = gid % extra + 1u;
  if (p >= r.s.n) return;
  const SpendTranscript st{r.s.P.L, r.s.bind != nullptr};      // a bound call hashes the bound length
  uint32_t rep[8], o[16];
  load8(rep, r.cand + ((size_t)p * extra + (k - 1u)) * 32);
  b3_xof64_patched(o, reinterpret_cast<const uint32_t*>(r.s.tr + (size_t)p * r.s.tr_stride), (uint32_t)st.bytes(),
                   r.sib + (size_t)p * B3_MAX_SIBLINGS * 8, ring_a1_offset(r.s.P.L) / 4u, rep);
  uint32_t* q = r.xofs + ((size_t)p * r.nkeys + k) * 16;
  for (int i = 0; i < 16; i++) q[i] = o[i];
}

// spend_finish_lane over a ring: the smallest k whose challenge equals gamma
ACT_HD void ring_finish_lane(const RingArgs& r, uint32_t p) {
  const SpendArgs& a = r.s;
  const ProofLayout pl{a.P.L};
  const sc gamma = load_sc(a.proofs + (size_t)p * pl.bytes() + 32 * pl.gamma());
  uint32_t match = KEY_NONE;
  for (uint32_t k = r.nkeys; k-- > 0;) {
    uint32_t w[16];
    for (int i = 0; i < 16; i++) w[i] = r.xofs[((size_t)p * r.nkeys + k) * 16 + i];
    if (sc_equal(sc_from_wide_words(w), gamma)) match = k;                     // src/transcript.rs:149-154, lib.rs:842-844
  }
  const uint32_t f = a.flags[p];
  uint8_t stt = 0;
  if (f & FLAG_UNDECODABLE) stt = 255;
  else if (f & FLAG_IDENTITY) stt = 6;                                        // Error::IdentityPointError
  else if (match == KEY_NONE) stt = 7;                                        // Error::InvalidClientSpendProof under every ring key
  a.status[p] = stt;
  r.out_key[p] = stt == 0 ? (uint8_t)match : KEY_NONE;
  if (a.kprime_enc && stt != 0) zero8(a.kprime_enc + (size_t)p * 32);
}

}  // namespace act
