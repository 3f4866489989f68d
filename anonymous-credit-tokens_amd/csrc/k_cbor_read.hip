// k_cbor_read.hip — the general RFC 8949 reader on the GPU (lane bodies in cbor_lanes.h, which says what they compute and why they
// terminate; engine side in cbor_impl.inc and admit_impl.inc).  A message that is not byte for byte the canonical template is read
// here, in its chunk's own stream between the unframing kernel and the verification kernels, instead of on the host behind the
// pipeline.  Nothing here is on the verification path itself: the range kernel, the spend kernels and the chunk schedule are not touched.
//
// Shape: ONE THREAD PER MESSAGE.  A lane reads a few bytes per head and moves each 32-byte payload as two byte-aligned 16-byte
// accesses; the lanes of a wave sit in 64 different messages, so these reads do not coalesce.  A SpendProof at L = 128 is 18 KB and
// about 650 heads -- small beside the 39.9 M multiply-accumulates of its verification.  A flagged message costs its whole wave the
// walk; waves without one return at once.  Workgroups of one wave are a choice without a measurement behind it (there is no
// barrier, so waves retire independently at any size).  The frame stack of cbor_skip (1 KiB per lane) lives in scratch memory, so
// every dispatch of these kernels asks for scratch -- also the dispatches of a canonical batch, whose lanes all return at once.
// What that costs per dispatch is NOT MEASURED: tools/wire_reader_probe.py (f = 0 against the parent build) is the measurement.
#include "cbor_lanes.h"

namespace act {

template <bool VALIDATE>
__global__ void __launch_bounds__(64) k_cbor_read_raw(CborReadArgs a) {
  uint32_t st[CBOR_MAX_DEPTH];
  cbor_read_message_lane<VALIDATE>(a, blockIdx.x * 64 + threadIdx.x, st);
}
__global__ void __launch_bounds__(256) k_cbor_read_fix(CborFixArgs a) { cbor_fix_field_lane(a, (uint64_t)blockIdx.x * 256 + threadIdx.x); }
__global__ void __launch_bounds__(256) k_cbor_read_zero(CborFixArgs a) { cbor_zero_failed_lane(a, (uint64_t)blockIdx.x * 256 + threadIdx.x); }
__global__ void __launch_bounds__(256) k_cbor_read_settle(CborSettleArgs a) { cbor_settle_lane(a, blockIdx.x * 256 + threadIdx.x); }
__global__ void __launch_bounds__(256) k_cbor_wire_code(CborCodeArgs a) { cbor_wire_code_lane(a, blockIdx.x * 256 + threadIdx.x); }

void launch_cbor_read(const CborReadArgs& a, bool validate, hipStream_t s) {
  if (!a.n) return;
  const dim3 grid((a.n + 63) / 64), block(64);
  if (validate) hipLaunchKernelGGL(k_cbor_read_raw<true>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(k_cbor_read_raw<false>, grid, block, 0, s, a);
}
void launch_cbor_fix(const CborFixArgs& a, hipStream_t s) {
  if (!a.n || !a.n_fields) return;
  const dim3 grid((unsigned)(((uint64_t)a.n * a.n_fields + 255) / 256)), block(256);
  hipLaunchKernelGGL(k_cbor_read_fix, grid, block, 0, s, a);
  hipLaunchKernelGGL(k_cbor_read_zero, grid, block, 0, s, a);
}
void launch_cbor_settle(const CborSettleArgs& a, hipStream_t s) { if (a.n) hipLaunchKernelGGL(k_cbor_read_settle, dim3((a.n + 255) / 256), dim3(256), 0, s, a); }
void launch_cbor_wire_code(const CborCodeArgs& a, hipStream_t s) { if (a.n) hipLaunchKernelGGL(k_cbor_wire_code, dim3((a.n + 255) / 256), dim3(256), 0, s, a); }

}  // namespace act
