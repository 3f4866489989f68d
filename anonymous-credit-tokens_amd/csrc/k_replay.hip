// k_replay.hip — the replayable redemption's kernels (lane bodies in replay_lanes.h, which says what they compute; engine side in
// replay_impl.inc).  Nothing here is on the verification path: two short hashes and one truth table per lane beside a verification.
#include "replay_lanes.h"

namespace act {

__global__ void __launch_bounds__(256) k_replay_tag(ReplayDeriveArgs a) { replay_tag_lane(a, blockIdx.x * 256 + threadIdx.x); }
__global__ void __launch_bounds__(256) k_replay_nonce(ReplayDeriveArgs a) { replay_nonce_lane(a, blockIdx.x * 256 + threadIdx.x); }
__global__ void __launch_bounds__(256) k_replay_resolve(ReplayResolveArgs a) { replay_resolve_lane(a, blockIdx.x * 256 + threadIdx.x); }

static unsigned replay_grid(uint32_t n) { return (n + 255u) / 256u; }

void launch_replay_tag(const ReplayDeriveArgs& a, hipStream_t s) { if (a.n) hipLaunchKernelGGL(k_replay_tag, dim3(replay_grid(a.n)), dim3(256), 0, s, a); }
void launch_replay_nonce(const ReplayDeriveArgs& a, hipStream_t s) { if (a.n) hipLaunchKernelGGL(k_replay_nonce, dim3(replay_grid(a.n)), dim3(256), 0, s, a); }
void launch_replay_resolve(const ReplayResolveArgs& a, hipStream_t s) { if (a.n) hipLaunchKernelGGL(k_replay_resolve, dim3(replay_grid(a.n)), dim3(256), 0, s, a); }

}  // namespace act
