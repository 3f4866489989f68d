// admit_replay_check.cpp — TEST-ONLY host build of the lane bodies of the admission stage of the replayable redemption
// (csrc/admit_replay_lanes.h): the key of the spent lanes' compaction, Com_j -> Niels, Horner -> enc(K') -> tag, and the decision, as
// the kernels of k_admit_replay.hip run them (one lane per thread, the grid's tail lanes included).  Built by
// tests/admit_replay_cases.py as a small library for tests/test_admit_replay_host.py; with -DADMIT_REPLAY_CHECK_MAIN it is a
// stand-alone program that checks the same bodies itself (K' by another road: 2^j Com_j by j doublings each) and is run under the
// sanitizers.  The build counts field multiplications and squarings (ACT_FE_BOUNDS), as tests/hostcheck/hostcheck.cpp does.
// Never linked into libact_mi355x.so.
#include <cstdio>
#include <cstring>
#include <vector>
#define ACT_FE_BOUNDS 1
#include "../../anonymous-credit-tokens_amd/csrc/admit_replay_lanes.h"

namespace act { fe_bounds_t fe_bounds = {0, 0, 0, 0, 0, 0}; fe_counts_t fe_counts = {0, 0, {0, 0, 0, 0}}; }
using namespace act;

namespace {
uint32_t grid_lanes(uint64_t n, uint32_t block) { return (uint32_t)(((n + block - 1) / block) * block); }
}  // namespace

extern "C" {

// out[0..2) = final pre-status, candidate
void hc_ar_decide(int pre, int spent, int undecodable, int found, uint8_t out[2]) {
  const AdmitReplayDecision d = admit_replay_decide((uint8_t)pre, spent != 0, undecodable != 0, found != 0);
  out[0] = d.pre; out[1] = d.candidate;
}
void hc_ar_key_lanes(uint32_t n, const uint8_t* pre, uint8_t* key) {
  const AdmitReplayKeyArgs a{n, pre, key};
  for (uint32_t i = 0; i < grid_lanes(n, 256); i++) admit_replay_key_lane(a, i);
}
void hc_ar_decide_lanes(uint32_t n, const uint32_t* pos, const uint8_t* mark, const uint8_t* found, uint8_t* pre) {
  const AdmitReplayDecideArgs a{n, pos, mark, found, pre};
  for (uint32_t i = 0; i < grid_lanes(n, 256); i++) admit_replay_decide_lane(a, i);
}
// n gathered records of 32 * (14 + 4 L) bytes; kred / idx as KprimeArgs has them; counts (nullable): fe_mul and fe_sq of the decode
// lanes, then of the tag lanes, summed over the n candidates
int hc_ar_kprime(int L, uint32_t n, const uint8_t* recs, const uint8_t* kred, const uint32_t* idx, uint8_t* kp, uint8_t* tag, uint8_t* mark, uint64_t counts[4]) {
  if (L < 1 || L > 128) return 0;
  std::vector<uint32_t> coords((size_t)n * L * NIELS_WORDS), flags(n, 0);      // exact sizes: a lane that strays is the sanitizer's to find
  KprimeArgs a{};
  a.s.P.L = L; a.s.proofs = recs; a.s.n = n; a.s.coords = coords.data(); a.s.flags = flags.data();
  a.kred = kred; a.idx = idx; a.kp = kp; a.tag = tag; a.mark = mark;
  fe_counts = fe_counts_t{0, 0, {0, 0, 0, 0}};
  for (uint32_t g = 0; g < grid_lanes((uint64_t)n * L, 64); g++) kprime_decode_lane(a, g);
  if (counts) { counts[0] = fe_counts.mul; counts[1] = fe_counts.sq; }
  fe_counts = fe_counts_t{0, 0, {0, 0, 0, 0}};
  for (uint32_t c = 0; c < grid_lanes(n, 64); c++) kprime_tag_lane(a, c);
  if (counts) { counts[2] = fe_counts.mul; counts[3] = fe_counts.sq; }
  fe_counts = fe_counts_t{0, 0, {0, 0, 0, 0}};
  return 1;
}

}  // extern "C"

#if defined(ADMIT_REPLAY_CHECK_MAIN)
namespace {
int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { failures++; fprintf(stderr, "admit_replay_check: line %d: %s\n", __LINE__, #cond); } } while (0)

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint8_t next_byte() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint8_t)(rng_state >> 24); }

void check_decision() {
  for (int pre = 0; pre < 256; pre++) for (int spent = 0; spent < 2; spent++) for (int bad = 0; bad < 2; bad++) for (int found = 0; found < 2; found++) {
    uint8_t r[2]; hc_ar_decide(pre, spent, bad, found, r);
    if (!spent) { EXPECT(r[0] == pre && r[1] == 0); continue; }
    const bool cand = !bad && found;
    EXPECT(r[0] == (cand ? 0 : 3) && r[1] == (cand ? 1 : 0));
  }
  for (uint32_t n : {1u, 63u, 64u, 65u, 256u, 257u}) {
    std::vector<uint8_t> pre(n), key(n, 9), mark, found;
    std::vector<uint32_t> pos(n);
    uint32_t ns = 0;
    for (uint32_t i = 0; i < n; i++) { pre[i] = (i % 3 == 0) ? 3 : (i % 7 == 1) ? 250 : (i % 11 == 2) ? 254 : 0; pos[i] = pre[i] == 3 ? ns++ : 0xFFFFFFFFu; }
    mark.resize(ns); found.resize(ns);
    for (uint32_t c = 0; c < ns; c++) { mark[c] = (c % 5 == 4); found[c] = (c % 2 == 0); }
    hc_ar_key_lanes(n, pre.data(), key.data());
    for (uint32_t i = 0; i < n; i++) EXPECT(key[i] == (pre[i] == 3 ? 0 : 1));
    std::vector<uint8_t> out = pre;
    hc_ar_decide_lanes(n, pos.data(), mark.data(), found.data(), out.data());
    for (uint32_t i = 0; i < n; i++) {
      if (pre[i] != 3) { EXPECT(out[i] == pre[i]); continue; }
      const uint32_t c = pos[i];
      EXPECT(out[i] == ((!mark[c] && found[c]) ? 0 : 3));
    }
  }
}

// n records at L with Com_j = (a few) * B; candidate `bad_at` (if < n) has one Com_j of 0xFF bytes.  K' by another road.
void check_kprime(int L, uint32_t n, uint32_t bad_at, bool with_idx) {
  const ProofLayout pl{L};
  const size_t pb = pl.bytes();
  std::vector<uint8_t> recs(n * pb), kred((size_t)(with_idx ? 2 * n : n) * 32), kp(n * 32, 0xAA), tag(n * 32, 0xAA), mark(n, 0xAA);
  std::vector<uint32_t> idx(n);
  for (auto& b : recs) b = next_byte();
  for (auto& b : kred) b = next_byte();
  for (uint32_t c = 0; c < n; c++) idx[c] = 2 * c + 1;
  std::vector<ge> pts((size_t)n * L);
  ge q = ge_basepoint();
  for (uint32_t c = 0; c < n; c++) for (int j = 0; j < L; j++) {
    for (int t = 0; t < 1 + (next_byte() & 3); t++) q = ge_add(ge_double(q), ge_basepoint());
    pts[(size_t)c * L + j] = q;
    uint32_t enc[8]; ristretto_encode(enc, q);
    store32_bytes(recs.data() + c * pb + 32 * pl.com(j), enc);
  }
  if (bad_at < n) memset(recs.data() + bad_at * pb + 32 * pl.com(L / 2), 0xFF, 32);
  uint64_t counts[4];
  EXPECT(hc_ar_kprime(L, n, recs.data(), kred.data(), with_idx ? idx.data() : nullptr, kp.data(), tag.data(), mark.data(), counts) == 1);
  const uint8_t zero[32] = {0};
  for (uint32_t c = 0; c < n; c++) {
    if (c == bad_at) { EXPECT(mark[c] == 1 && !memcmp(kp.data() + 32 * c, zero, 32) && !memcmp(tag.data() + 32 * c, zero, 32)); continue; }
    ge sum = ge_identity();
    for (int j = 0; j < L; j++) { ge t = pts[(size_t)c * L + j]; for (int d = 0; d < j; d++) t = ge_double(t); sum = ge_add(sum, t); }
    uint32_t enc[8], k[8], want[8];
    ristretto_encode(enc, sum);
    uint8_t eb[32], tb[32]; store32_bytes(eb, enc);
    EXPECT(mark[c] == 0 && !memcmp(kp.data() + 32 * c, eb, 32));
    null_load_key(k, kred.data() + (size_t)(with_idx ? idx[c] : c) * 32);
    replay_tag(want, k, enc); store32_bytes(tb, want);
    EXPECT(!memcmp(tag.data() + 32 * c, tb, 32) && (tag[32 * c + 31] & 0xF0) == 0);
  }
}
}  // namespace

int main() {
  check_decision();
  for (int L : {3, 8}) for (uint32_t n : {1u, 65u}) { check_kprime(L, n, n, false); check_kprime(L, n, n / 2, true); }
  check_kprime(128, 2, 1, true);
  if (failures) { fprintf(stderr, "admit_replay_check: %d failures\n", failures); return 1; }
  puts("ADMIT REPLAY CHECK CLEAN");
  return 0;
}
#endif
