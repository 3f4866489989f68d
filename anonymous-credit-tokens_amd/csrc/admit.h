// admit.h — launchers of the admission kernels (k_admit.hip; argument blocks and lane bodies in admit_lanes.h, engine side in
// admit_impl.inc) and of the copy stage behind the screen (k_copies.hip; copy_lanes.h; copies_impl.inc).
#pragma once
#include "admit_lanes.h"
#include "copy_lanes.h"

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
// the copy stage, over the m survivors of the screen in their compact order
void launch_copy_fp(const CopyFpArgs& a, hipStream_t s);                // fp[j]: one wavefront per survivor
void launch_copy_leaders(const CopyTableArgs& a, hipStream_t s);        // tab_fp zero and tab_j all-ones before; leader[j] = the smallest j with fp[j]
void launch_copy_equal(const CopyEqualArgs& a, hipStream_t s);          // copy_of[j] = leader[j] when every byte is equal, else COPY_NONE
void launch_copy_mark(const CopyMarkArgs& a, hipStream_t s);            // pre2 = a copy of pre and lead all-ones before
void launch_copy_resolve(const CopyResolveArgs& a, hipStream_t s);      // behind launch_admit_scatter on the same stream
void launch_copy_serve(const CopyServeArgs& a, hipStream_t s);          // the replay unique forms: behind BOTH scatters (rows and replay marks)
void launch_copy_serve_return(const CopyServeReturnArgs& a, hipStream_t s);      // the return replay unique forms: the same place, with the amounts
#endif

}  // namespace act
