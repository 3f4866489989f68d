// k_copies.hip — the copy stage of admission: byte-identical proofs of one batch are verified once (act_redeem_admit_unique_batch /
// act_redeem_cbor_admit_unique_batch; lane bodies in copy_lanes.h, which says what they compute; engine side in copies_impl.inc), and
// the serve pass of act_redeem_(cbor_)admit_replay_unique_batch, where a copy gets its leader's refund, and that of
// act_redeem_(cbor_)return_replay_unique_batch, where it gets it only if it names its leader's amount.
// Nothing here is on the verification path.
#include "copy_lanes.h"
#include "admit.h"

namespace act {

constexpr uint32_t COPY_WAVES = 4;      // survivors per workgroup of the two byte-touching kernels: one wavefront each

// the 64 values of a wavefront, summed: every lane ends with the total (butterfly over __shfl_xor, the two halves of a 64-bit word
// travel as two 32-bit shuffles)
__device__ __forceinline__ uint64_t copy_wave_sum(uint64_t v) {
  for (int o = 32; o; o >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o);
    v += (uint64_t)hi << 32 | lo;
  }
  return v;
}

// One wavefront per survivor: a record is 16.8 KB at L = 128, and 64 threads reading consecutive 16-byte pieces make every load of
// the wavefront one contiguous KiB.  Messages start at any byte, so the loads are byte-aligned ones (copy_load16).
__global__ void __launch_bounds__(64 * COPY_WAVES) k_copy_fp(CopyFpArgs a) {
  const uint32_t j = blockIdx.x * COPY_WAVES + (threadIdx.x >> 6), t = threadIdx.x & 63u;
  if (j >= a.m) return;                                       // (uniform per wavefront)
  const uint32_t lane = a.idx[j];
  const uint64_t len = copy_len(a.span, lane);
  const uint64_t sum = copy_wave_sum(copy_fp_partial(a.span.src + copy_beg(a.span, lane), len, t, a.salt.w));
  if (t == 0) a.fp[j] = copy_fp_finish(sum, len, a.salt.w);
}

__global__ void __launch_bounds__(256) k_copy_claim(CopyTableArgs a) { copy_claim_lane(a, blockIdx.x * 256 + threadIdx.x); }
__global__ void __launch_bounds__(256) k_copy_leader(CopyTableArgs a) { copy_leader_lane(a, blockIdx.x * 256 + threadIdx.x); }

__global__ void __launch_bounds__(64 * COPY_WAVES) k_copy_equal(CopyEqualArgs a) {
  const uint32_t j = blockIdx.x * COPY_WAVES + (threadIdx.x >> 6), t = threadIdx.x & 63u;
  if (j >= a.m) return;                                       // (uniform per wavefront)
  const uint8_t *x = nullptr, *y = nullptr; uint64_t len = 0;
  bool same = copy_equal_ranges(a, j, &x, &y, &len);          // (uniform per wavefront)
  if (same) same = __ballot(!copy_equal_partial(x, y, len, t)) == 0ull;
  if (t == 0) a.copy_of[j] = same ? a.leader[j] : COPY_NONE;
}

__global__ void __launch_bounds__(256) k_copy_mark(CopyMarkArgs a) { copy_mark_lane(a, blockIdx.x * 256 + threadIdx.x); }
__global__ void __launch_bounds__(256) k_copy_resolve(CopyResolveArgs a) { copy_resolve_lane(a, blockIdx.x * 256 + threadIdx.x); }

// The replay unique forms: one thread per 16-byte piece of an item's output row, so the threads of a copy read consecutive pieces of
// its leader's row and write consecutive pieces of its own.  Rows of leaders are read, rows of copies are written, a leader is never a
// copy: no thread reads what another writes.  The caller's full-size arrays (a leader may lie in an earlier gather window).
__global__ void __launch_bounds__(256) k_copy_serve(CopyServeArgs a, uint32_t pieces) {
  const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t i = p / pieces;
  if (i < a.n) copy_serve_piece(a, (uint32_t)i, (uint32_t)(p % pieces));
}

// The return replay unique forms: k_copy_serve's shape and mapping, and per thread two 32-byte amounts more -- the copy's and its
// leader's, in the caller's array.  The threads of a row load the same 64 bytes (the copy's amount is one line, the leader's another:
// broadcasts within the row's threads) and reach the same verdict, so a row is written whole or zeroed whole.
__global__ void __launch_bounds__(256) k_copy_serve_return(CopyServeReturnArgs a, uint32_t pieces) {
  const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t i = p / pieces;
  if (i < a.v.n) copy_serve_return_piece(a, (uint32_t)i, (uint32_t)(p % pieces));
}

static unsigned copy_grid(uint64_t lanes, uint32_t per_block) { return (unsigned)((lanes + per_block - 1) / per_block); }

void launch_copy_fp(const CopyFpArgs& a, hipStream_t s) { if (a.m) hipLaunchKernelGGL(k_copy_fp, dim3(copy_grid(a.m, COPY_WAVES)), dim3(64 * COPY_WAVES), 0, s, a); }
void launch_copy_leaders(const CopyTableArgs& a, hipStream_t s) {
  if (!a.m) return;
  hipLaunchKernelGGL(k_copy_claim, dim3(copy_grid(a.m, 256)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_copy_leader, dim3(copy_grid(a.m, 256)), dim3(256), 0, s, a);
}
void launch_copy_equal(const CopyEqualArgs& a, hipStream_t s) { if (a.m) hipLaunchKernelGGL(k_copy_equal, dim3(copy_grid(a.m, COPY_WAVES)), dim3(64 * COPY_WAVES), 0, s, a); }
void launch_copy_mark(const CopyMarkArgs& a, hipStream_t s) { if (a.m) hipLaunchKernelGGL(k_copy_mark, dim3(copy_grid(a.m, 256)), dim3(256), 0, s, a); }
void launch_copy_resolve(const CopyResolveArgs& a, hipStream_t s) { if (a.n) hipLaunchKernelGGL(k_copy_resolve, dim3(copy_grid(a.n, 256)), dim3(256), 0, s, a); }
void launch_copy_serve(const CopyServeArgs& a, hipStream_t s) {
  const uint32_t pieces = admit_pieces(a.out_b);
  if (a.n && pieces) hipLaunchKernelGGL(k_copy_serve, dim3(copy_grid((uint64_t)a.n * pieces, 256)), dim3(256), 0, s, a, pieces);
}
void launch_copy_serve_return(const CopyServeReturnArgs& a, hipStream_t s) {
  const uint32_t pieces = admit_pieces(a.v.out_b);
  if (a.v.n && pieces) hipLaunchKernelGGL(k_copy_serve_return, dim3(copy_grid((uint64_t)a.v.n * pieces, 256)), dim3(256), 0, s, a, pieces);
}

}  // namespace act
