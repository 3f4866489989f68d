// keyring.h — argument blocks and launchers of the key-ring kernels (k_keyring.hip; lane bodies in keyring_lanes.h, engine side in
// keyring_impl.inc): one batch of spend proofs verified and refunded against an ordered ring of up to four issuer keys.
#pragma once
#include "kernels.h"

namespace act {

constexpr int KEYRING_MAX = 4;            // ACT_KEYRING_MAX
constexpr uint8_t KEY_NONE = 255;         // ACT_KEY_NONE

struct RingArgs {
  SpendArgs s;               // the chunk's one-key arguments (s.K = ring key 0; s.xof is not read here)
  const DevKey* ring;        // nkeys entries (device memory, wiped with the call's other secrets)
  uint32_t nkeys;
  uint8_t* cand;             // n * (nkeys - 1) * 32: enc(A1_k), k = 1 .. nkeys - 1
  uint32_t* sib;             // n * B3_MAX_SIBLINGS * 8: chunk 0's path siblings of every transcript hash
  uint32_t* xofs;            // n * nkeys * 16: XOF words of the transcript under key k
  uint8_t* out_key;          // n
};

// byte offset of the A1 payload inside a "spend" transcript: prefix (184) | k | A' | B_bar | A1 ..., 8 bytes of length in front
ACT_HDC inline uint32_t ring_a1_offset(int L) { return 184u + 40u * (uint32_t)SpendTranscript{L}.el_a1() + 8u; }

// sign with a per-lane key (k_sign.hip ring instantiations of k_sign_a / k_sign_b): lane p signs with ring[key_index[p]]
struct SignRingArgs {
  SignArgs s;                // s.K is not read
  const DevKey* ring;
  const uint8_t* key_index;  // n: below nkeys on every lane whose status is 0 (launch_ring_index_check has seen to it)
  uint32_t nkeys;
};

#if defined(__HIPCC__)
void launch_ring_cand(const RingArgs& r, hipStream_t s);          // candidates A1_k, k >= 1
void launch_ring_hash_full(const RingArgs& r, hipStream_t s);     // device transcripts: the whole hash (key 0), chunk 0's path siblings kept
void launch_ring_hash(const RingArgs& r, hipStream_t s);          // device transcripts: the patched hashes, k >= 1
void launch_ring_finish(const RingArgs& r, hipStream_t s);
// status[p] == 0 and key_index[p] >= nkeys -> status[p] = 255 (the lane is not signed)
void launch_ring_index_check(uint8_t* status, const uint8_t* key_index, uint32_t nkeys, uint32_t n, hipStream_t s);
// key_index[p] = sign_key >= 0 ? sign_key : out_key[p]   (ACT_SIGN_MATCHED = -1)
void launch_ring_resolve_index(uint8_t* key_index, const uint8_t* out_key, int sign_key, uint32_t n, hipStream_t s);
void launch_sign_a_ring(const SignRingArgs& a, hipStream_t s);
void launch_sign_b_ring(const SignRingArgs& a, hipStream_t s);
#endif

}  // namespace act
