// k_return_replay.hip — the kernels of the replayable partial refunds (lane bodies in return_replay_lanes.h, which says what they compute;
// engine side in replay_impl.inc and admit_replay_impl.inc).  The kernels of k_replay.hip and k_admit_replay.hip with the lane's returned
// amount in the hashes; those files' own kernels are not touched and serve every call that takes no amounts.
#include "return_replay_lanes.h"

namespace act {

__global__ void __launch_bounds__(256) k_return_replay_tag(ReplayDeriveArgs a) { return_replay_tag_lane(a, blockIdx.x * 256 + threadIdx.x); }
__global__ void __launch_bounds__(256) k_return_replay_nonce(ReplayDeriveArgs a) { return_replay_nonce_lane(a, blockIdx.x * 256 + threadIdx.x); }
__global__ void __launch_bounds__(64, 2) k_kprime_tag_return(KprimeArgs a) { kprime_tag_return_lane(a, blockIdx.x * 64 + threadIdx.x); }

void launch_return_replay_tag(const ReplayDeriveArgs& a, hipStream_t s) { if (a.n) hipLaunchKernelGGL(k_return_replay_tag, dim3((a.n + 255u) / 256u), dim3(256), 0, s, a); }
void launch_return_replay_nonce(const ReplayDeriveArgs& a, hipStream_t s) { if (a.n) hipLaunchKernelGGL(k_return_replay_nonce, dim3((a.n + 255u) / 256u), dim3(256), 0, s, a); }
void launch_kprime_tag_return(const KprimeArgs& a, hipStream_t s) { if (a.s.n) hipLaunchKernelGGL(k_kprime_tag_return, dim3((a.s.n + 63u) / 64u), dim3(64), 0, s, a); }

}  // namespace act
