// k_admit.hip — admission before verification: the kernels in front of act_redeem_admit_batch / act_redeem_cbor_admit_batch (lane
// bodies in admit_lanes.h, which says what they compute; engine side in admit_impl.inc).  Nothing here is on the verification path:
// the range kernel, the spend kernels and the chunk schedule are not touched.
#include "admit_lanes.h"
#include "admit.h"

namespace act {

__global__ void __launch_bounds__(256) k_admit_wire(AdmitWireArgs a) {
  const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (uint64_t)a.n * a.n_fields) return;
  const uint32_t m = (uint32_t)(gid / a.n_fields), f = (uint32_t)(gid % a.n_fields);
  if (!admit_wire_piece(a, m, f)) atomicOr(reinterpret_cast<unsigned int*>(a.flags + (m & ~3u)), 0x80u << (8 * (m & 3u)));
}

__global__ void __launch_bounds__(256) k_admit_screen(AdmitScreenArgs a) { admit_screen_lane(a, blockIdx.x * 256 + threadIdx.x); }

// Stable compaction of the lanes with pre[i] == 0, three launches.  No atomic anywhere: every wave's survivors are counted with one
// 64-bit ballot, a workgroup's four counts meet in LDS, the workgroup counts are scanned by one workgroup, and the write pass
// recomputes the ballots -- a survivor's place is (workgroups below) + (waves below) + (lanes below), which is its rank in lane order.
__global__ void __launch_bounds__(ADMIT_BLOCK) k_admit_count(const uint8_t* pre, uint32_t n, uint32_t* blk) {
  __shared__ uint32_t wc[ADMIT_BLOCK / 64];
  const uint32_t i = blockIdx.x * ADMIT_BLOCK + threadIdx.x;
  const unsigned long long mask = __ballot(i < n && admit_keep(pre[i < n ? i : 0]));
  if ((threadIdx.x & 63u) == 0) wc[threadIdx.x >> 6] = (uint32_t)__popcll(mask);
  __syncthreads();
  if (threadIdx.x == 0) blk[blockIdx.x] = admit_wave_base(wc, ADMIT_BLOCK / 64);
}
__global__ void __launch_bounds__(ADMIT_BLOCK) k_admit_scan(uint32_t* blk, uint32_t nb, uint32_t* total) {
  __shared__ uint32_t sums[ADMIT_BLOCK];
  const uint32_t t = threadIdx.x, seg = admit_scan_seg(nb, ADMIT_BLOCK);
  sums[t] = admit_scan_sum(blk, nb, seg, t);
  __syncthreads();
  if (t == 0) { uint32_t run = 0; for (uint32_t j = 0; j < ADMIT_BLOCK; j++) { const uint32_t v = sums[j]; sums[j] = run; run += v; } *total = run; }
  __syncthreads();
  admit_scan_write(blk, nb, seg, t, sums[t]);
}
__global__ void __launch_bounds__(ADMIT_BLOCK) k_admit_write(const uint8_t* pre, uint32_t n, const uint32_t* blk, uint32_t* idx, uint32_t* pos) {
  __shared__ uint32_t wc[ADMIT_BLOCK / 64];
  const uint32_t i = blockIdx.x * ADMIT_BLOCK + threadIdx.x;
  const bool keep = i < n && admit_keep(pre[i < n ? i : 0]);
  const unsigned long long mask = __ballot(keep);
  if ((threadIdx.x & 63u) == 0) wc[threadIdx.x >> 6] = (uint32_t)__popcll(mask);
  __syncthreads();
  if (i >= n) return;
  if (!keep) { pos[i] = ADMIT_SHED; return; }
  const uint32_t at = blk[blockIdx.x] + admit_wave_base(wc, threadIdx.x >> 6) + admit_rank(mask, threadIdx.x & 63u);
  idx[at] = i; pos[i] = at;                                   // at < (survivors in all) <= n: idx and pos hold n entries each
}

__global__ void __launch_bounds__(256) k_admit_rows(AdmitRowsArgs a) { admit_rows_piece(a, (uint64_t)blockIdx.x * 256 + threadIdx.x); }
__global__ void __launch_bounds__(256) k_admit_msgs(AdmitMsgsArgs a) { admit_msgs_piece(a, (uint64_t)blockIdx.x * 256 + threadIdx.x); }
__global__ void __launch_bounds__(256) k_admit_scatter(AdmitScatterArgs a) { admit_scatter_piece(a, (uint64_t)blockIdx.x * 256 + threadIdx.x); }
__global__ void __launch_bounds__(256) k_admit_patch(AdmitPatchArgs a) { admit_patch_piece(a, blockIdx.x * 256 + threadIdx.x); }

static unsigned admit_grid(uint64_t lanes) { return (unsigned)((lanes + 255) / 256); }

void launch_admit_wire(const AdmitWireArgs& a, hipStream_t s) { if (a.n) hipLaunchKernelGGL(k_admit_wire, dim3(admit_grid((uint64_t)a.n * a.n_fields)), dim3(256), 0, s, a); }
void launch_admit_screen(const AdmitScreenArgs& a, hipStream_t s) { if (a.n) hipLaunchKernelGGL(k_admit_screen, dim3(admit_grid(a.n)), dim3(256), 0, s, a); }
void launch_admit_compact(const uint8_t* pre, uint32_t n, uint32_t* blk, uint32_t* idx, uint32_t* pos, uint32_t* total, hipStream_t s) {
  if (!n) return;
  const uint32_t nb = (n + ADMIT_BLOCK - 1) / ADMIT_BLOCK;
  hipLaunchKernelGGL(k_admit_count, dim3(nb), dim3(ADMIT_BLOCK), 0, s, pre, n, blk);
  hipLaunchKernelGGL(k_admit_scan, dim3(1), dim3(ADMIT_BLOCK), 0, s, blk, nb, total);
  hipLaunchKernelGGL(k_admit_write, dim3(nb), dim3(ADMIT_BLOCK), 0, s, pre, n, blk, idx, pos);
}
void launch_admit_rows(const AdmitRowsArgs& a, hipStream_t s) { if (a.m && a.row_bytes) hipLaunchKernelGGL(k_admit_rows, dim3(admit_grid((uint64_t)a.m * admit_pieces(a.row_bytes))), dim3(256), 0, s, a); }
void launch_admit_msgs(const AdmitMsgsArgs& a, hipStream_t s) { if (a.m && a.max_pieces) hipLaunchKernelGGL(k_admit_msgs, dim3(admit_grid((uint64_t)a.m * a.max_pieces)), dim3(256), 0, s, a); }
void launch_admit_scatter(const AdmitScatterArgs& a, hipStream_t s) { if (a.n) hipLaunchKernelGGL(k_admit_scatter, dim3(admit_grid((uint64_t)a.n * admit_pieces(a.out_bytes))), dim3(256), 0, s, a); }
void launch_admit_patch(const AdmitPatchArgs& a, hipStream_t s) { if (a.count) hipLaunchKernelGGL(k_admit_patch, dim3(admit_grid((uint64_t)a.count * 4)), dim3(256), 0, s, a); }

}  // namespace act
