// k_admit_replay.hip — the kernels of the admission stage of the replayable redemption (lane bodies in admit_replay_lanes.h, which says
// what they compute; engine side in admit_replay_impl.inc).  Nothing here is on the verification path: the range kernel, the spend
// kernels and the chunk schedule are not touched.  The decode is the bulk of the stage (L lanes per candidate, one inverse square root
// each, perfectly lane-parallel); the tag kernel is one Horner run, one encoding and two hash blocks per candidate.
#include "admit_replay_lanes.h"

namespace act {

__global__ void __launch_bounds__(256) k_admit_replay_key(AdmitReplayKeyArgs a) { admit_replay_key_lane(a, blockIdx.x * 256 + threadIdx.x); }
__global__ void __launch_bounds__(64, 2) k_kprime_decode(KprimeArgs a) { kprime_decode_lane(a, blockIdx.x * 64 + threadIdx.x); }
__global__ void __launch_bounds__(64, 2) k_kprime_tag(KprimeArgs a) { kprime_tag_lane(a, blockIdx.x * 64 + threadIdx.x); }
__global__ void __launch_bounds__(256) k_admit_replay_decide(AdmitReplayDecideArgs a) { admit_replay_decide_lane(a, blockIdx.x * 256 + threadIdx.x); }

void launch_admit_replay_key(const AdmitReplayKeyArgs& a, hipStream_t s) { if (a.n) hipLaunchKernelGGL(k_admit_replay_key, dim3((a.n + 255u) / 256u), dim3(256), 0, s, a); }
void launch_kprime_decode(const KprimeArgs& a, hipStream_t s) {
  if (!a.s.n) return;
  const size_t lanes = (size_t)a.s.n * a.s.P.L;
  hipLaunchKernelGGL(k_kprime_decode, dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, s, a);
}
void launch_kprime_tag(const KprimeArgs& a, hipStream_t s) { if (a.s.n) hipLaunchKernelGGL(k_kprime_tag, dim3((a.s.n + 63u) / 64u), dim3(64), 0, s, a); }
void launch_admit_replay_decide(const AdmitReplayDecideArgs& a, hipStream_t s) { if (a.n) hipLaunchKernelGGL(k_admit_replay_decide, dim3((a.n + 255u) / 256u), dim3(256), 0, s, a); }

}  // namespace act
