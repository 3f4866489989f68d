// admit.h — launchers of the admission kernels (k_admit.hip; argument blocks and lane bodies in admit_lanes.h, engine side in
// admit_impl.inc).
#pragma once
#include "admit_lanes.h"

namespace act {

#if defined(__HIPCC__)
void launch_admit_wire(const AdmitWireArgs& a, hipStream_t s);          // framing compare, k and s out; flags must be zero before
void launch_admit_screen(const AdmitScreenArgs& a, hipStream_t s);
// idx[0 .. *total) = the lanes with pre == 0 in lane order, pos[i] = a lane's place in idx or ADMIT_SHED; blk: (n + 255) / 256 words
void launch_admit_compact(const uint8_t* pre, uint32_t n, uint32_t* blk, uint32_t* idx, uint32_t* pos, uint32_t* total, hipStream_t s);
void launch_admit_rows(const AdmitRowsArgs& a, hipStream_t s);
void launch_admit_msgs(const AdmitMsgsArgs& a, hipStream_t s);
void launch_admit_scatter(const AdmitScatterArgs& a, hipStream_t s);
void launch_admit_patch(const AdmitPatchArgs& a, hipStream_t s);
#endif

}  // namespace act
