// k_debug_sc.hip -- test hook (act_debug_sc_batch): ONE operation of the scalar arithmetic mod l (sc25519.h) per lane, so that the
// device build of the three-stage fold, of from_bytes_mod_order, of the carry and borrow chains and of the Montgomery product inside
// sc_invert can be driven to their edges one call at a time (tests/test_gpu_sc_edges.py, case lists in tests/sc_edge_cases.py).
// Protocol runs reach them with random scalars only.  A lane owns one record of DSC_WORDS words in each array an operation names:
//   LOAD_SC, LOAD_WIDE        32 / 64 operand BYTES at the start of a's record, through the production load_sc / load_wide; the result
//                             leaves through store_sc
//   ADD ... INVERT            raw 8-word operands (nothing reduces them on the way in: the test chooses what is canonical)
//   SCM_MUL                   raw 10-limb operands and result (scm_mul: 26-bit limbs, Montgomery form, lazily reduced)
//   EQUAL, IS_ZERO            result word 0 or 1
// An operation writes the words of its result and no other word of r.  Never on the product's path.
#include "kernels.h"

namespace act {

static __device__ __forceinline__ sc dsc_load(const uint32_t* p, uint32_t i) {
  sc r; for (int k = 0; k < 8; k++) r.v[k] = p[(size_t)i * DSC_WORDS + k]; return r;
}
static __device__ __forceinline__ void dsc_store(uint32_t* p, uint32_t i, const sc& x) {
  for (int k = 0; k < 8; k++) p[(size_t)i * DSC_WORDS + k] = x.v[k];
}

__global__ void __launch_bounds__(256) k_debug_sc(int op, uint32_t n, const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* r) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint8_t* ab = reinterpret_cast<const uint8_t*>(a + (size_t)i * DSC_WORDS);      // records are 64 bytes: aligned for load8 / store8
  uint8_t* rb = reinterpret_cast<uint8_t*>(r + (size_t)i * DSC_WORDS);
  switch (op) {
    case DSC_LOAD_SC: store_sc(rb, load_sc(ab)); break;
    case DSC_LOAD_WIDE: store_sc(rb, load_wide(ab)); break;
    case DSC_ADD: dsc_store(r, i, sc_add(dsc_load(a, i), dsc_load(b, i))); break;
    case DSC_SUB: dsc_store(r, i, sc_sub(dsc_load(a, i), dsc_load(b, i))); break;
    case DSC_NEG: dsc_store(r, i, sc_neg(dsc_load(a, i))); break;
    case DSC_HALF: dsc_store(r, i, sc_half(dsc_load(a, i))); break;
    case DSC_MUL: dsc_store(r, i, sc_mul(dsc_load(a, i), dsc_load(b, i))); break;
    case DSC_MULADD: dsc_store(r, i, sc_muladd(dsc_load(a, i), dsc_load(b, i), dsc_load(c, i))); break;
    case DSC_INVERT: dsc_store(r, i, sc_invert(dsc_load(a, i))); break;
    case DSC_SCM_MUL: {
      uint32_t x[SCM_LIMBS], y[SCM_LIMBS], o[SCM_LIMBS];
      for (int k = 0; k < SCM_LIMBS; k++) { x[k] = a[(size_t)i * DSC_WORDS + k]; y[k] = b[(size_t)i * DSC_WORDS + k]; }
      scm_mul(o, x, y);
      for (int k = 0; k < SCM_LIMBS; k++) r[(size_t)i * DSC_WORDS + k] = o[k];
      break;
    }
    case DSC_EQUAL: r[(size_t)i * DSC_WORDS] = sc_equal(dsc_load(a, i), dsc_load(b, i)) ? 1u : 0u; break;
    case DSC_IS_ZERO: r[(size_t)i * DSC_WORDS] = sc_is_zero(dsc_load(a, i)) ? 1u : 0u; break;
    default: break;
  }
}
void launch_debug_sc(int op, uint32_t n, const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* r, hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_debug_sc, dim3((n + 255) / 256), dim3(256), 0, s, op, n, a, b, c, r);
}

}  // namespace act
