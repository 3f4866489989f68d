// k_reserve.hip — the kernels of reserve and settle (lane bodies in reserve_lanes.h, which says what they compute; engine side in
// reserve_impl.inc, replay_impl.inc and admit_impl.inc).  One lane per thread; the kernels of k_replay.hip, k_admit_replay.hip and
// k_return_replay.hip are not touched and serve every other call.
#include "reserve_lanes.h"

namespace act {

__global__ void __launch_bounds__(256) k_reserve_sred(ReserveSredArgs a) { reserve_sred_lane(a, blockIdx.x * 256 + threadIdx.x); }
__global__ void __launch_bounds__(64, 2) k_kprime_tag_reserve(KprimeArgs a) { kprime_tag_reserve_lane(a, blockIdx.x * 64 + threadIdx.x); }
__global__ void __launch_bounds__(256) k_reserve_tag(ReplayDeriveArgs a) { reserve_tag_lane(a, blockIdx.x * 256 + threadIdx.x); }
__global__ void __launch_bounds__(256) k_reserve_emit(ReserveEmitArgs a) { reserve_emit_lane(a, blockIdx.x * 256 + threadIdx.x); }
__global__ void __launch_bounds__(256) k_settle_prep(SettlePrepArgs a) { settle_prep_lane(a, blockIdx.x * 256 + threadIdx.x); }
__global__ void __launch_bounds__(256) k_settle_found(SettleFoundArgs a) { settle_found_lane(a, blockIdx.x * 256 + threadIdx.x); }
__global__ void __launch_bounds__(256) k_settle_merge(SettleMergeArgs a) { settle_merge_lane(a, blockIdx.x * 256 + threadIdx.x); }

void launch_reserve_sred(const ReserveSredArgs& a, hipStream_t s) { if (a.n) hipLaunchKernelGGL(k_reserve_sred, dim3((a.n + 255u) / 256u), dim3(256), 0, s, a); }
void launch_kprime_tag_reserve(const KprimeArgs& a, hipStream_t s) { if (a.s.n) hipLaunchKernelGGL(k_kprime_tag_reserve, dim3((a.s.n + 63u) / 64u), dim3(64), 0, s, a); }
void launch_reserve_tag(const ReplayDeriveArgs& a, hipStream_t s) { if (a.n) hipLaunchKernelGGL(k_reserve_tag, dim3((a.n + 255u) / 256u), dim3(256), 0, s, a); }
void launch_reserve_emit(const ReserveEmitArgs& a, hipStream_t s) { if (a.n) hipLaunchKernelGGL(k_reserve_emit, dim3((a.n + 255u) / 256u), dim3(256), 0, s, a); }
void launch_settle_prep(const SettlePrepArgs& a, hipStream_t s) { if (a.n) hipLaunchKernelGGL(k_settle_prep, dim3((a.n + 255u) / 256u), dim3(256), 0, s, a); }
void launch_settle_found(const SettleFoundArgs& a, hipStream_t s) { if (a.n) hipLaunchKernelGGL(k_settle_found, dim3((a.n + 255u) / 256u), dim3(256), 0, s, a); }
void launch_settle_merge(const SettleMergeArgs& a, hipStream_t s) { if (a.n) hipLaunchKernelGGL(k_settle_merge, dim3((a.n + 255u) / 256u), dim3(256), 0, s, a); }

}  // namespace act
