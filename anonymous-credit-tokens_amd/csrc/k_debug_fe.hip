// k_debug_fe.hip -- test hook (act_debug_fe_batch): ONE field operation per lane on raw 9-limb operands, so that the device forms of
// fe25519.h can be driven to the top of their limb-size classes one call at a time (tests/test_gpu_fe_forms.py).  Built twice:
// as it stands, with the flags of every other unit (per-column products: the act_cz* / act_c* helpers, fe_limb_sub's v_sad_u32), and
// through k_debug_fe_pair.hip with the range kernel's flags (Makefile BITSFLAGS: the one-statement products ACT_FE_*_ONE_ASM, which
// name the registers v232..v254 -- hence launch bounds that leave a lane all 256, as k_spend_bits has).  Never on the product's path.
#include "kernels.h"

namespace act {

#if defined(ACT_DEBUG_FE_PAIR)
#define K_DEBUG_FE k_debug_fe_pair
#define LAUNCH_DEBUG_FE launch_debug_fe_pair
#else
#define K_DEBUG_FE k_debug_fe
#define LAUNCH_DEBUG_FE launch_debug_fe
#endif

static __device__ __forceinline__ fe dfe_load(const uint32_t* p, uint32_t i) {
  fe r; for (int k = 0; k < FE_LIMBS; k++) r.v[k] = p[(size_t)i * FE_LIMBS + k]; return r;
}
static __device__ __forceinline__ void dfe_store(uint32_t* p, uint32_t i, const fe& x) {
  for (int k = 0; k < FE_LIMBS; k++) p[(size_t)i * FE_LIMBS + k] = x.v[k];
}

// lane i: operands f[i], g[i], fb[i], ga[i] (the second product's g, or fe_sqda_sq's addend a) -> h[i], hb[i]; an operation reads and
// writes only the arrays it names
__global__ void __launch_bounds__(256, 2) K_DEBUG_FE(int op, uint32_t n, const uint32_t* f, const uint32_t* g, const uint32_t* fb, const uint32_t* ga, uint32_t* h, uint32_t* hb) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const fe x = dfe_load(f, i);
  fe r, rb;
  switch (op) {
    case DFE_MUL: dfe_store(h, i, fe_mul(x, dfe_load(g, i))); break;
    case DFE_SQ: dfe_store(h, i, fe_sq(x)); break;
    case DFE_MUL2: fe_mul2(r, rb, x, dfe_load(g, i), dfe_load(fb, i), dfe_load(ga, i)); dfe_store(h, i, r); dfe_store(hb, i, rb); break;
    case DFE_SQ2: fe_sq2(r, rb, x, dfe_load(fb, i)); dfe_store(h, i, r); dfe_store(hb, i, rb); break;
    case DFE_SQDA_SQ: fe_sqda_sq(r, rb, x, dfe_load(ga, i), dfe_load(fb, i)); dfe_store(h, i, r); dfe_store(hb, i, rb); break;
    case DFE_CARRY: dfe_store(h, i, fe_carry(x)); break;
    case DFE_SUB: dfe_store(h, i, fe_sub(x, dfe_load(g, i))); break;
    case DFE_SUB3: dfe_store(h, i, fe_sub3(x, dfe_load(g, i))); break;
    case DFE_SUB4: dfe_store(h, i, fe_sub4(x, dfe_load(g, i))); break;
    case DFE_NEG: dfe_store(h, i, fe_neg(x)); break;
    default: break;
  }
}
void LAUNCH_DEBUG_FE(int op, uint32_t n, const uint32_t* f, const uint32_t* g, const uint32_t* fb, const uint32_t* ga, uint32_t* h, uint32_t* hb, hipStream_t s) {
  if (n) hipLaunchKernelGGL(K_DEBUG_FE, dim3((n + 255) / 256), dim3(256), 0, s, op, n, f, g, fb, ga, h, hb);
}

}  // namespace act
