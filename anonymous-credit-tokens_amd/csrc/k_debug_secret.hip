// k_debug_secret.hip -- test hooks for the products of SECRET scalars (msm.h "secret scalars"), one product per lane, so that a chosen
// scalar can aim at one entry of one window of the matrix-core look-up from one lane, or at one digit of the address-free chains
// (tests/test_gpu_secret_products.py):
//   act_debug_fixed_base_mf_batch   fixed_base_acc_mf over the context's own table image (k_build_table_mf), in blocks of 64 threads
//                                   (k_keygen, the per-proof kernels) or 256 (k_prove_bits)
//   act_debug_chain_ct_batch        chain_ct<1>, the four chain_ct_quarter pieces added up, chain_ct<2>
// with the production load_sc, ristretto_decode and ristretto_encode around them.  Never on the product's path.
#include "kernels.h"

namespace act {

// out[i] = enc(s_i * B), B's image at tab_mf.  Launched in whole blocks.  A lane from n on takes the scalar 0, runs the product WITH
// its wavefront and returns only after it, as k_keygen does: the look-up's table operand has its rows loaded by all 64 lanes of the
// wavefront (msm.h mf_select), so a lane that left before the product would leave the live lanes garbage rows to multiply with.
template <int BT>
__global__ void __launch_bounds__(BT, BT == 256 ? 2 : 1) k_debug_fixed_base_mf(const uint8_t* tab_mf, const uint8_t* scs, uint32_t n, uint8_t* out) {
  const uint32_t i = blockIdx.x * BT + threadIdx.x;
  const sc s = i < n ? load_sc(scs + (size_t)i * 32) : sc_zero();
  const ge r = fixed_base_acc_mf(ge_identity(), tab_mf, s);        // every lane of the wavefront
  if (i >= n) return;
  uint32_t e[8]; ristretto_encode(e, r);
  store8(out + (size_t)i * 32, e);
}
void launch_debug_fixed_base_mf(const uint8_t* tab_mf, int block_threads, const uint8_t* scs, uint32_t n, uint8_t* out, hipStream_t s) {
  if (!n) return;
  if (block_threads == 256) hipLaunchKernelGGL(k_debug_fixed_base_mf<256>, dim3((n + 255) / 256), dim3(256), 0, s, tab_mf, scs, n, out);
  else hipLaunchKernelGGL(k_debug_fixed_base_mf<64>, dim3((n + 63) / 64), dim3(64), 0, s, tab_mf, scs, n, out);
}

// lane i decodes P_i (status 255 and zero records if it does not decode, as k_debug_scalarmult answers) and writes
//   mode 0   out = enc(s_i P_i)                     chain_ct<1> from the identity
//   mode 1   out = enc(sum_q chain_ct_quarter(P_i, s_i, q))      the four pieces of the single-item calls, added with ge_add
//   mode 2   out = enc(s_i P_i), out2 = enc(s2_i P_i)            chain_ct<2>: two scalars on one doubling chain
// Nothing here is shared between lanes, so a lane from n on leaves at once.
__global__ void __launch_bounds__(64, 2) k_debug_chain_ct(int mode, const uint8_t* pts, const uint8_t* scs, const uint8_t* scs2, uint32_t n, uint8_t* out, uint8_t* out2, uint8_t* status) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t w[8]; load8(w, pts + (size_t)i * 32);
  ge p; const bool ok = ristretto_decode(p, w);
  const sc s0 = load_sc(scs + (size_t)i * 32);
  ge acc[2] = {ge_identity(), ge_identity()};
  if (mode == 0) {
    sc s[1] = {s0};
    chain_ct<1>(acc, p, s);
  } else if (mode == 1) {
    acc[0] = chain_ct_quarter(p, s0, 0);
    for (int q = 1; q < 4; q++) acc[0] = ge_add(acc[0], chain_ct_quarter(p, s0, q));
  } else {
    sc s[2] = {s0, load_sc(scs2 + (size_t)i * 32)};
    chain_ct<2>(acc, p, s);
  }
  uint32_t e[8]; ristretto_encode(e, acc[0]);
  if (ok) store8(out + (size_t)i * 32, e); else zero8(out + (size_t)i * 32);
  if (mode == 2) {
    ristretto_encode(e, acc[1]);
    if (ok) store8(out2 + (size_t)i * 32, e); else zero8(out2 + (size_t)i * 32);
  }
  status[i] = ok ? 0 : 255;
}
void launch_debug_chain_ct(int mode, const uint8_t* pts, const uint8_t* scs, const uint8_t* scs2, uint32_t n, uint8_t* out, uint8_t* out2, uint8_t* status, hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_debug_chain_ct, dim3((n + 63) / 64), dim3(64), 0, s, mode, pts, scs, scs2, n, out, out2, status);
}

}  // namespace act
