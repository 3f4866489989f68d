// copy_check.cpp — TEST-ONLY host build of the lane bodies of admission's copy stage (csrc/copy_lanes.h): the fingerprint as a
// wavefront computes it (64 partial sums, added), the leader table over fingerprints the caller supplies (so that collisions can be
// forced) with the claims made in any order, the exact compare, the side array of the second compaction and the resolve pass.
// Built by tests/copies_cases.py; never linked into libact_mi355x.so.
#include <cstring>
#include <vector>
#include "../../anonymous-credit-tokens_amd/csrc/copy_lanes.h"

using namespace act;

extern "C" {

// one range, as k_copy_fp's wavefront: thread t's partial for t = 0 .. 63, summed, finished with the length
uint64_t hc_copy_fp(const uint8_t* p, uint64_t len, const uint8_t salt[16]) {
  uint32_t s[4]; memcpy(s, salt, 16);
  uint64_t sum = 0;
  for (uint32_t t = 0; t < 64; t++) sum += copy_fp_partial(p, len, t, s);
  return copy_fp_finish(sum, len, s);
}
// the same with the 64 partial values added in another order (the reduction is commutative)
uint64_t hc_copy_fp_reversed(const uint8_t* p, uint64_t len, const uint8_t salt[16]) {
  uint32_t s[4]; memcpy(s, salt, 16);
  uint64_t sum = 0;
  for (uint32_t t = 64; t-- > 0;) sum += copy_fp_partial(p, len, t, s);
  return copy_fp_finish(sum, len, s);
}
// and as a host worker computes it: one thread, the pieces in order
uint64_t hc_copy_fp_host(const uint8_t* p, uint64_t len, const uint8_t salt[16]) {
  uint32_t s[4]; memcpy(s, salt, 16);
  return copy_fp_finish(copy_fp_sum(p, len, s), len, s);
}
// the compare as a host worker runs it
int hc_copy_equal_all(const uint8_t* x, const uint8_t* y, uint64_t len) { return copy_equal_all(x, y, len); }
// fp[j] of survivor idx[j], as the kernel addresses it (offsets nullable: rows of row_bytes)
void hc_copy_fp_lanes(const uint8_t* src, const uint64_t* offsets, uint64_t row_bytes, const uint32_t* idx, uint32_t m, const uint8_t salt[16], uint64_t* fp) {
  const CopySpan span{src, offsets, row_bytes};
  for (uint32_t j = 0; j < m; j++) fp[j] = hc_copy_fp(src + copy_beg(span, idx[j]), copy_len(span, idx[j]), salt);
}

// k_copy_claim for every j in the order `order` gives (nullable: 0, 1, ...), then k_copy_leader; the grid's tail lanes too.
// cap = 0: the engine's choice (the power of two >= 2 m, at least 4).  Returns the slots in use.
uint32_t hc_copy_leaders(const uint64_t* fp, uint32_t m, uint32_t cap, const uint32_t* order, uint32_t* leader) {
  if (!cap) { cap = 4; while (cap < 2 * (uint64_t)m) cap <<= 1; }
  std::vector<uint64_t> tab_fp(cap, 0); std::vector<uint32_t> tab_j(cap, COPY_NONE), slot(m ? m : 1, COPY_NONE);
  CopyTableArgs a{fp, m, tab_fp.data(), tab_j.data(), cap, slot.data(), leader};
  for (uint32_t k = 0; k < m; k++) copy_claim_lane(a, order ? order[k] : k);
  for (uint32_t j = m; j < (m + 255) / 256 * 256; j++) copy_claim_lane(a, j);
  for (uint32_t j = 0; j < (m + 255) / 256 * 256; j++) copy_leader_lane(a, j);
  uint32_t used = 0;
  for (uint32_t t = 0; t < cap; t++) used += tab_fp[t] != 0;
  return used;
}

// k_copy_equal: copy_of[j] = leader[j] when the two ranges are equal in length and in every byte
void hc_copy_equal(const uint8_t* src, const uint64_t* offsets, uint64_t row_bytes, const uint32_t* idx, const uint32_t* leader, uint32_t m, uint32_t* copy_of) {
  CopyEqualArgs a{{src, offsets, row_bytes}, idx, leader, m, copy_of};
  for (uint32_t j = 0; j < m; j++) {
    const uint8_t *x = nullptr, *y = nullptr; uint64_t len = 0;
    bool same = copy_equal_ranges(a, j, &x, &y, &len);
    if (same) {
      uint64_t ballot = 0;
      for (uint32_t t = 0; t < 64; t++) if (!copy_equal_partial(x, y, len, t)) ballot |= 1ull << t;
      same = ballot == 0;
      if (copy_equal_all(x, y, len) != same) { copy_of[j] = 0xBAD0BAD0u; continue; }      // the host workers' walk must agree with the wavefront's
    }
    copy_of[j] = same ? leader[j] : COPY_NONE;
  }
}

void hc_copy_mark(const uint32_t* idx, const uint32_t* copy_of, uint32_t m, uint8_t* pre2, uint32_t* lead) {
  CopyMarkArgs a{idx, copy_of, m, pre2, lead};
  for (uint32_t j = 0; j < (m + 255) / 256 * 256; j++) copy_mark_lane(a, j);
}
void hc_copy_resolve(const uint32_t* lead, uint32_t n, uint8_t* status, uint8_t* out_key) {
  CopyResolveArgs a{lead, n, status, out_key};
  for (uint32_t i = 0; i < (n + 255) / 256 * 256; i++) copy_resolve_lane(a, i);
}
int hc_copy_status(int leader_status) { return copy_status((uint8_t)leader_status); }
int hc_copy_mark_value() { return COPY_MARK; }

}  // extern "C"
