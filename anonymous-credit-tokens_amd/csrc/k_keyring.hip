// k_keyring.hip — key rotation: the kernels a ring of issuer keys adds to spend verification (lane bodies in keyring_lanes.h, which
// says what they compute and why it costs under 1 % of a verification per extra key).  The one-key kernels are not touched: a ring
// call runs them under ring key 0 and these behind them.
#include "keyring_lanes.h"

namespace act {

__global__ void __launch_bounds__(64, 2) k_ring_cand(RingArgs r) { ring_cand_lane(r, blockIdx.x * 64 + threadIdx.x); }

// Transcript::challenge's hash as k_hash_xof computes it, lane = message, leaving the siblings of chunk 0's path behind
__global__ void __launch_bounds__(64) k_ring_hash_full(RingArgs r) {
  const uint32_t p = blockIdx.x * 64 + threadIdx.x;
  if (p >= r.s.n) return;
  const SpendTranscript st{r.s.P.L, r.s.bind != nullptr};      // a bound call hashes the bound length
  const uint32_t* msg = reinterpret_cast<const uint32_t*>(r.s.tr + (size_t)p * r.s.tr_stride);
  const uint32_t len = (uint32_t)st.bytes();
  uint32_t* sib = r.sib + (size_t)p * B3_MAX_SIBLINGS * 8;
  uint32_t o[16];
  b3_hash_xof64_sib(o, msg, len, [&](uint32_t c, uint32_t* cv) { b3_chunk_cv(cv, msg, len, c); },
                    [&](int level, const uint32_t* cv) { for (int i = 0; i < 8; i++) sib[level * 8 + i] = cv[i]; });
  uint4* q = reinterpret_cast<uint4*>(r.xofs + (size_t)p * r.nkeys * 16);
  q[0] = make_uint4(o[0], o[1], o[2], o[3]); q[1] = make_uint4(o[4], o[5], o[6], o[7]);
  q[2] = make_uint4(o[8], o[9], o[10], o[11]); q[3] = make_uint4(o[12], o[13], o[14], o[15]);
}
__global__ void __launch_bounds__(64) k_ring_hash(RingArgs r) { ring_hash_lane(r, blockIdx.x * 64 + threadIdx.x); }

__global__ void __launch_bounds__(256) k_ring_finish(RingArgs r) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p < r.s.n) ring_finish_lane(r, p);
}

__global__ void __launch_bounds__(256) k_ring_index_check(uint8_t* status, const uint8_t* key_index, uint32_t nkeys, uint32_t n) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p < n && status[p] == 0 && key_index[p] >= nkeys) status[p] = 255;
}
__global__ void __launch_bounds__(256) k_ring_resolve_index(uint8_t* key_index, const uint8_t* out_key, int sign_key, uint32_t n) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p < n) key_index[p] = sign_key >= 0 ? (uint8_t)sign_key : out_key[p];
}

static unsigned ring_extra_blocks(const RingArgs& r) { return (unsigned)(((size_t)r.s.n * (r.nkeys - 1u) + 63) / 64); }
void launch_ring_cand(const RingArgs& r, hipStream_t s) { if (r.s.n && r.nkeys > 1) hipLaunchKernelGGL(k_ring_cand, dim3(ring_extra_blocks(r)), dim3(64), 0, s, r); }
void launch_ring_hash_full(const RingArgs& r, hipStream_t s) { if (r.s.n) hipLaunchKernelGGL(k_ring_hash_full, dim3((r.s.n + 63) / 64), dim3(64), 0, s, r); }
void launch_ring_hash(const RingArgs& r, hipStream_t s) { if (r.s.n && r.nkeys > 1) hipLaunchKernelGGL(k_ring_hash, dim3(ring_extra_blocks(r)), dim3(64), 0, s, r); }
void launch_ring_finish(const RingArgs& r, hipStream_t s) { if (r.s.n) hipLaunchKernelGGL(k_ring_finish, dim3((r.s.n + 255) / 256), dim3(256), 0, s, r); }
void launch_ring_index_check(uint8_t* status, const uint8_t* key_index, uint32_t nkeys, uint32_t n, hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_ring_index_check, dim3((n + 255) / 256), dim3(256), 0, s, status, key_index, nkeys, n);
}
void launch_ring_resolve_index(uint8_t* key_index, const uint8_t* out_key, int sign_key, uint32_t n, hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_ring_resolve_index, dim3((n + 255) / 256), dim3(256), 0, s, key_index, out_key, sign_key, n);
}

}  // namespace act
