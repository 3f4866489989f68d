// admit_check.cpp — TEST-ONLY host build of the admission lane bodies (csrc/admit_lanes.h, csrc/null_probe.h): the decision, the screen
// over a table this file builds with the set's own slot function, the framing compare, the stable compaction as the three kernels
// of k_admit.hip run it (workgroups of 256 lanes, waves of 64, one scanning workgroup), and the gather / scatter pieces.  Built by
// tests/admission_cases.py; never linked into libact_mi355x.so.
#include <cstring>
#include <vector>
#include "../../anonymous-credit-tokens_amd/csrc/admit_lanes.h"

using namespace act;

extern "C" {

int hc_admit_decide(int wire_code, int charge_given, int charge_equal, int found, int* probed) {
  *probed = 0;
  return admit_decide((uint8_t)wire_code, charge_given != 0, charge_equal != 0, [&]() { *probed = 1; return found != 0; });
}

// the set's slot hash of a 32-byte nullifier under a 16-byte salt, as the kernels compute it: reduce, then hash (both table starts come from it)
uint64_t hc_null_hash(const uint8_t key[32], const uint8_t salt[16]) {
  uint32_t w[8], s[4]; null_load_key(w, key); memcpy(s, salt, 16);
  return null_hash(w, s);
}

// a committed slot for `key` (reduced here, as the set reduces it) under `epoch`: the set's slot function, linear probing.  0 = table full
int hc_admit_table_insert(uint32_t* tab_keys, uint32_t* tab_state, uint32_t tab_cap, const uint8_t salt[16], const uint8_t key[32], uint32_t epoch) {
  uint32_t w[8], s[4]; null_load_key(w, key); memcpy(s, salt, 16);
  uint32_t t = (uint32_t)(null_hash(w, s) >> 32) & (tab_cap - 1);
  for (uint32_t p = 0; p < tab_cap; p++, t = (t + 1) & (tab_cap - 1)) {
    if ((tab_state[t] & 0xFFu) == 2u) { if (null_eq(w, tab_keys + (size_t)t * 8)) return 1; continue; }
    memcpy(tab_keys + (size_t)t * 8, w, 32); tab_state[t] = epoch << 8 | 2u;
    return 1;
  }
  return 0;
}

void hc_admit_screen(uint32_t n, uint32_t stride, const uint8_t* ks, const uint8_t* charge, const uint8_t* wire_code, const uint32_t* tab_keys,
                     const uint32_t* tab_state, uint32_t tab_cap, const uint8_t salt[16], uint8_t* pre, uint8_t* kred) {
  AdmitScreenArgs a{};
  a.n = n; a.stride = stride; a.ks = ks; a.charge = charge; a.wire_code = wire_code; a.tab_keys = tab_keys; a.tab_state = tab_state; a.tab_cap = tab_cap;
  memcpy(a.salt.w, salt, 16); a.pre = pre; a.kred = kred;
  for (uint32_t i = 0; i < ((n + 255) / 256) * 256; i++) admit_screen_lane(a, i);      // the grid's tail lanes too
}

// flags[m] = 0x80 unless every field's framing is the template's; ks as the kernel leaves it
void hc_admit_wire(uint32_t n, uint32_t n_fields, uint32_t msg_len, const uint8_t* cbor, const uint64_t* offsets, const uint8_t* tmpl, const uint32_t* pay_off,
                   uint8_t* ks, uint8_t* flags) {
  AdmitWireArgs a{n, n_fields, msg_len, cbor, offsets, tmpl, pay_off, ks, flags};
  for (uint32_t m = 0; m < n; m++) for (uint32_t f = 0; f < n_fields; f++) if (!admit_wire_piece(a, m, f)) flags[m] |= 0x80;
}

// k_admit_count -> k_admit_scan -> k_admit_write, lane for lane: blk (nb words), idx and pos (n words each).  Returns the survivors.
uint32_t hc_admit_compact(const uint8_t* pre, uint32_t n, uint32_t* blk, uint32_t* idx, uint32_t* pos) {
  const uint32_t nb = (n + ADMIT_BLOCK - 1) / ADMIT_BLOCK, waves = ADMIT_BLOCK / 64;
  auto masks = [&](uint32_t b, uint64_t mask[ADMIT_BLOCK / 64], uint32_t wc[ADMIT_BLOCK / 64]) {
    for (uint32_t w = 0; w < waves; w++) {
      mask[w] = 0;
      for (uint32_t l = 0; l < 64; l++) { const uint32_t i = b * ADMIT_BLOCK + w * 64 + l; if (i < n && admit_keep(pre[i])) mask[w] |= 1ull << l; }
      wc[w] = (uint32_t)__builtin_popcountll(mask[w]);
    }
  };
  uint64_t mask[ADMIT_BLOCK / 64]; uint32_t wc[ADMIT_BLOCK / 64];
  for (uint32_t b = 0; b < nb; b++) { masks(b, mask, wc); blk[b] = admit_wave_base(wc, waves); }
  uint32_t sums[ADMIT_BLOCK], total = 0;
  const uint32_t seg = admit_scan_seg(nb, ADMIT_BLOCK);
  for (uint32_t t = 0; t < ADMIT_BLOCK; t++) sums[t] = admit_scan_sum(blk, nb, seg, t);
  for (uint32_t t = 0; t < ADMIT_BLOCK; t++) { const uint32_t v = sums[t]; sums[t] = total; total += v; }
  for (uint32_t t = 0; t < ADMIT_BLOCK; t++) admit_scan_write(blk, nb, seg, t, sums[t]);
  for (uint32_t b = 0; b < nb; b++) {
    masks(b, mask, wc);
    for (uint32_t t = 0; t < ADMIT_BLOCK; t++) {
      const uint32_t i = b * ADMIT_BLOCK + t, w = t >> 6, l = t & 63u;
      if (i >= n) continue;
      if (!(mask[w] >> l & 1)) { pos[i] = ADMIT_SHED; continue; }
      const uint32_t at = blk[b] + admit_wave_base(wc, w) + admit_rank(mask[w], l);
      idx[at] = i; pos[i] = at;
    }
  }
  return total;
}

void hc_admit_rows(uint8_t* dst, const uint8_t* src, const uint32_t* idx, uint32_t m, uint64_t row_bytes) {
  AdmitRowsArgs a{dst, src, idx, m, row_bytes};
  const uint64_t lanes = ((uint64_t)m * admit_pieces(row_bytes) + 255) / 256 * 256;
  for (uint64_t p = 0; p < lanes; p++) admit_rows_piece(a, p);
}
void hc_admit_msgs(uint8_t* dst, const uint64_t* dst_off, const uint8_t* src, const uint64_t* src_beg, uint32_t m, uint32_t max_pieces) {
  AdmitMsgsArgs a{dst, dst_off, src, src_beg, m, max_pieces};
  const uint64_t lanes = ((uint64_t)m * max_pieces + 255) / 256 * 256;
  for (uint64_t p = 0; p < lanes; p++) admit_msgs_piece(a, p);
}
void hc_admit_scatter(uint32_t n, uint64_t out_bytes, const uint32_t* pos, const uint8_t* pre, const uint8_t* c_status, const uint8_t* c_key, const uint8_t* c_out,
                      uint8_t* status, uint8_t* out_key, uint8_t* out) {
  AdmitScatterArgs a{n, out_bytes, pos, pre, c_status, c_key, c_out, status, out_key, out};
  const uint64_t lanes = ((uint64_t)n * admit_pieces(out_bytes) + 255) / 256 * 256;
  for (uint64_t p = 0; p < lanes; p++) admit_scatter_piece(a, p);
}
void hc_admit_patch(uint8_t* ks, const uint32_t* which, const uint8_t* patch, uint32_t count) {
  AdmitPatchArgs a{ks, which, patch, count};
  for (uint32_t p = 0; p < (count * 4 + 255) / 256 * 256; p++) admit_patch_piece(a, p);
}

}  // extern "C"
