// k_client_ring.hip — key rotation on the client: the kernels a ring of issuer PUBLIC keys adds to the two to_credit_token verifiers
// (lane bodies in client_ring_lanes.h, which says what they compute and what an extra key costs).  The one-key kernels of k_client.hip
// are not touched: a ring call runs phase A under ring key 0 and these behind it.  k_client_ring_return_finish is the finish over
// RefundReturn records (client_ring_return_lanes.h): the candidate and hash kernels serve both, at the record stride with_t selects.
#include "client_ring_return_lanes.h"

namespace act {

__global__ void __launch_bounds__(64) k_client_ring_cand(ClientRingArgs r) { client_ring_cand_lane(r, blockIdx.x * 64 + threadIdx.x); }
__global__ void __launch_bounds__(64) k_client_ring_hash(ClientRingArgs r) { client_ring_hash_lane(r, blockIdx.x * 64 + threadIdx.x); }
__global__ void __launch_bounds__(256) k_client_ring_finish(ClientRingArgs r) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p < r.c.n) client_ring_finish_lane(r, p);
}
__global__ void __launch_bounds__(256) k_client_ring_return_finish(ClientRingArgs r) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p < r.c.n) client_ring_return_finish_lane(r, p);
}

static unsigned client_ring_extra_blocks(const ClientRingArgs& r) { return (unsigned)(((size_t)r.c.n * (r.nkeys - 1u) + 63) / 64); }
void launch_client_ring_cand(const ClientRingArgs& r, hipStream_t s) {
  if (r.c.n && r.nkeys > 1) hipLaunchKernelGGL(k_client_ring_cand, dim3(client_ring_extra_blocks(r)), dim3(64), 0, s, r);
}
void launch_client_ring_hash(const ClientRingArgs& r, hipStream_t s) {
  if (r.c.n && r.nkeys > 1) hipLaunchKernelGGL(k_client_ring_hash, dim3(client_ring_extra_blocks(r)), dim3(64), 0, s, r);
}
void launch_client_ring_finish(const ClientRingArgs& r, hipStream_t s) {
  if (r.c.n) hipLaunchKernelGGL(k_client_ring_finish, dim3((r.c.n + 255) / 256), dim3(256), 0, s, r);
}
void launch_client_ring_return_finish(const ClientRingArgs& r, hipStream_t s) {
  if (r.c.n) hipLaunchKernelGGL(k_client_ring_return_finish, dim3((r.c.n + 255) / 256), dim3(256), 0, s, r);
}

}  // namespace act
