// return_replay_check.cpp — TEST-ONLY host build of the lane bodies of the replayable partial refunds (csrc/return_replay_lanes.h): the
// receipt tag and the derived nonce with the lane's returned amount, and the candidate's tag of the admission stage, as the kernels of
// k_return_replay.hip run them (one lane per thread, the grid's tail lanes included).  Built by tests/return_replay_cases.py as a small
// library for tests/test_return_replay_host.py; with -DRETURN_REPLAY_CHECK_MAIN it is a stand-alone program that checks the same bodies
// itself (against blake3_hd.h's general hash over the assembled message) and is run under the sanitizers.  The build counts BLAKE3
// compressions (ACT_B3_COUNT) and field multiplications and squarings (ACT_FE_BOUNDS).  Never linked into libact_mi355x.so.
#include <cstdio>
#include <cstring>
#include <vector>
#define ACT_FE_BOUNDS 1
#define ACT_B3_COUNT 1
#include "../../anonymous-credit-tokens_amd/csrc/return_replay_lanes.h"

namespace act { fe_bounds_t fe_bounds = {0, 0, 0, 0, 0, 0}; fe_counts_t fe_counts = {0, 0, {0, 0, 0, 0}}; uint64_t b3_compress_count = 0; }
using namespace act;

namespace {
// nonce_key | ring records where the lane body wants them: 4-byte aligned
struct Secrets {
  uint32_t w[REPLAY_SECRET_BYTES / 4];
  Secrets(const uint8_t nonce_key[32], const uint8_t* keys, uint32_t nkeys) { memset(w, 0, sizeof(w)); memcpy(w, nonce_key, 32); memcpy(w + 8, keys, (size_t)nkeys * 64); }
};
uint32_t grid_lanes(uint64_t n, uint32_t block) { return (uint32_t)(((n + block - 1) / block) * block); }
void reset_counts() { fe_counts = fe_counts_t{0, 0, {0, 0, 0, 0}}; b3_compress_count = 0; }
}  // namespace

extern "C" {

// t: nullable (every amount zero).  v1 != 0: the lane bodies of replay_lanes.h, which take no amount
void hc_rr_tags(uint32_t n, uint32_t stride, const uint8_t* nul, const uint8_t* kp, const uint8_t* st, const uint8_t* kidx, uint32_t nkeys, const uint8_t* t, int v1,
                uint8_t* out) {
  ReplayDeriveArgs a{}; a.n = n; a.stride = stride; a.nkeys = nkeys; a.nul = nul; a.kp = kp; a.st = st; a.kidx = kidx; a.out = out; a.t = t;
  for (uint32_t i = 0; i < grid_lanes(n, 256); i++) { if (v1) replay_tag_lane(a, i); else return_replay_tag_lane(a, i); }
}
void hc_rr_nonces(uint32_t n, uint32_t stride, const uint8_t* nul, const uint8_t* kp, const uint8_t* st, const uint8_t* kidx, const uint8_t* keys, uint32_t nkeys,
                  const uint8_t nonce_key[32], const uint8_t* t, int v1, uint8_t* out) {
  const Secrets sec(nonce_key, keys, nkeys);
  ReplayDeriveArgs a{}; a.n = n; a.stride = stride; a.nkeys = nkeys; a.nul = nul; a.kp = kp; a.st = st; a.kidx = kidx; a.t = t;
  a.secrets = reinterpret_cast<const uint8_t*>(sec.w); a.out = out;
  for (uint32_t i = 0; i < grid_lanes(n, 256); i++) { if (v1) replay_nonce_lane(a, i); else return_replay_nonce_lane(a, i); }
}
// One live lane with the amount t (32 bytes): counts[0], [1] = BLAKE3 compressions of the tag lane and of the nonce lane, counted, not
// assumed; counts[2] = fe_mul + fe_sq of both lanes together (the hashes add no field operation)
void hc_rr_lane_counts(const uint8_t t[32], uint64_t counts[3]) {
  uint8_t nul[32], kp[32], keys[64], nonce_key[32], tag[32], non[128];
  for (int i = 0; i < 32; i++) { nul[i] = (uint8_t)(i + 1); kp[i] = (uint8_t)(3 * i + 7); nonce_key[i] = (uint8_t)(5 * i + 2); }
  nul[31] &= 0x0F;
  for (int i = 0; i < 64; i++) keys[i] = (uint8_t)(7 * i + 1);
  const uint8_t st = 0, kidx = 0;
  const Secrets sec(nonce_key, keys, 1);
  ReplayDeriveArgs a{}; a.n = 1; a.stride = 32; a.nkeys = 1; a.nul = nul; a.kp = kp; a.st = &st; a.kidx = &kidx; a.t = t;
  a.secrets = reinterpret_cast<const uint8_t*>(sec.w);
  reset_counts();
  a.out = tag; return_replay_tag_lane(a, 0);
  counts[0] = b3_compress_count; b3_compress_count = 0;
  a.out = non; return_replay_nonce_lane(a, 0);
  counts[1] = b3_compress_count;
  counts[2] = fe_counts.mul + fe_counts.sq;
  reset_counts();
}
// n gathered records of 32 * (14 + 4 L) bytes; kred / idx / t as KprimeArgs has them (t nullable).  counts (nullable): fe_mul + fe_sq
// and BLAKE3 compressions of the n tag lanes of admit_replay_lanes.h (no amount), then of the n tag lanes with the amounts
int hc_rr_kprime(int L, uint32_t n, const uint8_t* recs, const uint8_t* kred, const uint32_t* idx, const uint8_t* t, uint8_t* kp, uint8_t* tag, uint8_t* mark,
                 uint64_t counts[4]) {
  if (L < 1 || L > 128) return 0;
  std::vector<uint32_t> coords((size_t)n * L * NIELS_WORDS), flags(n, 0);      // exact sizes: a lane that strays is the sanitizer's to find
  KprimeArgs a{};
  a.s.P.L = L; a.s.proofs = recs; a.s.n = n; a.s.coords = coords.data(); a.s.flags = flags.data();
  a.kred = kred; a.idx = idx; a.kp = kp; a.tag = tag; a.mark = mark; a.t = t;
  for (uint32_t g = 0; g < grid_lanes((uint64_t)n * L, 64); g++) kprime_decode_lane(a, g);
  reset_counts();
  for (uint32_t c = 0; c < grid_lanes(n, 64); c++) kprime_tag_lane(a, c);
  if (counts) { counts[0] = fe_counts.mul + fe_counts.sq; counts[1] = b3_compress_count; }
  reset_counts();
  for (uint32_t c = 0; c < grid_lanes(n, 64); c++) kprime_tag_return_lane(a, c);
  if (counts) { counts[2] = fe_counts.mul + fe_counts.sq; counts[3] = b3_compress_count; }
  reset_counts();
  return 1;
}

}  // extern "C"

#if defined(RETURN_REPLAY_CHECK_MAIN)
namespace {
int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { failures++; fprintf(stderr, "return_replay_check: line %d: %s\n", __LINE__, #cond); } } while (0)

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint8_t next_byte() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint8_t)(rng_state >> 24); }

// l = 2^252 + 27742317777372353535851937790883648493, little-endian
const uint8_t ELL[32] = {0xed, 0xd3, 0xf5, 0x5c, 0x1a, 0x63, 0x12, 0x58, 0xd6, 0x9c, 0xf7, 0xa2, 0xde, 0xf9, 0xde, 0x14, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0x10};
void add_ell(uint8_t out[32], const uint8_t in[32]) {
  unsigned carry = 0;
  for (int i = 0; i < 32; i++) { const unsigned s = in[i] + ELL[i] + carry; out[i] = (uint8_t)s; carry = s >> 8; }
}
void small(uint8_t out[32], uint8_t v) { memset(out, 0, 32); out[0] = v; }
void ell_minus_1(uint8_t out[32]) { memcpy(out, ELL, 32); out[0] -= 1; }

// the same hashes by another road: the message assembled in memory, k and t reduced, through the general b3_hash_xof64.  The amount is
// not zero after reduction.
void reference_t(const uint8_t k_raw[32], const uint8_t kp[32], const uint8_t key[64], const uint8_t nonce_key[32], const uint8_t t_raw[32], uint8_t tag[32],
                 uint8_t block0[64]) {
  uint32_t kw[8], tw[8]; null_load_key(kw, k_raw); null_load_key(tw, t_raw);
  uint32_t msg[56], o[16];
  uint8_t* m = reinterpret_cast<uint8_t*>(msg);
  memset(msg, 0, sizeof(msg)); memcpy(m, "act-mi355x/receipt-t/v1", 23); memcpy(m + 32, kw, 32); memcpy(m + 64, kp, 32); memcpy(m + 96, tw, 32);
  b3_hash_xof64(o, msg, 128);
  memcpy(tag, o, 32); tag[31] &= 0x0F;
  memset(msg, 0, sizeof(msg)); memcpy(m, "act-mi355x/refund-nonce-t/v1", 28); memcpy(m + 32, nonce_key, 32); memcpy(m + 64, key, 64); memcpy(m + 128, kw, 32);
  memcpy(m + 160, kp, 32); memcpy(m + 192, tw, 32);
  b3_hash_xof64(o, msg, 224);
  memcpy(block0, o, 64);
}

// lane i's amount: 0, 1, s (= 5), l - 1, 1 + l (unreduced), l (reduces to 0), in turn
void amount(uint8_t out[32], uint32_t i) {
  uint8_t one[32];
  switch (i % 6) {
    case 0: small(out, 0); break;
    case 1: small(out, 1); break;
    case 2: small(out, 5); break;
    case 3: ell_minus_1(out); break;
    case 4: small(one, 1); add_ell(out, one); break;
    default: memcpy(out, ELL, 32); break;
  }
}
bool amount_is_zero(uint32_t i) { return i % 6 == 0 || i % 6 == 5; }

void check_derive(uint32_t n, uint32_t stride, uint32_t shift) {
  const uint32_t nkeys = 3;
  // exact-size heap blocks, the arrays at an odd byte offset when shift is odd: a read or write past an array is the sanitizer's to find
  std::vector<uint8_t> nul_b((size_t)(n - 1) * stride + 32 + shift), kp_b((size_t)n * 32 + shift), t_b((size_t)n * 32 + shift), st(n), kidx(n), keys(nkeys * 64),
      tags_b((size_t)n * 32 + shift), non_b((size_t)n * 128 + shift), tags1((size_t)n * 32), non1((size_t)n * 128);
  uint8_t nonce_key[32];
  uint8_t *nul = nul_b.data() + shift, *kp = kp_b.data() + shift, *t = t_b.data() + shift, *tags = tags_b.data() + shift, *non = non_b.data() + shift;
  for (auto& b : nul_b) b = next_byte();
  for (auto& b : kp_b) b = next_byte();
  for (auto& b : keys) b = next_byte();
  for (auto& b : nonce_key) b = next_byte();
  for (uint32_t i = 0; i < n; i++) { st[i] = (i % 5 == 3) ? 7 : 0; kidx[i] = (uint8_t)((i % 7 == 6) ? 255 : i % nkeys); amount(t + 32 * i, i); }
  memset(tags_b.data(), 0xAA, tags_b.size()); memset(non_b.data(), 0xAA, non_b.size());
  hc_rr_tags(n, stride, nul, kp, st.data(), nullptr, 0, t, 0, tags);
  hc_rr_nonces(n, stride, nul, kp, st.data(), kidx.data(), keys.data(), nkeys, nonce_key, t, 0, non);
  hc_rr_tags(n, stride, nul, kp, st.data(), nullptr, 0, nullptr, 1, tags1.data());
  hc_rr_nonces(n, stride, nul, kp, st.data(), kidx.data(), keys.data(), nkeys, nonce_key, nullptr, 1, non1.data());
  const uint8_t zero[128] = {0};
  for (uint32_t i = 0; i < n; i++) {
    if (st[i]) { EXPECT(!memcmp(tags + 32 * i, zero, 32)); EXPECT(!memcmp(non + 128 * i, zero, 128)); continue; }      // dead lanes give zeros
    const bool keyed = kidx[i] < nkeys;
    if (!keyed) EXPECT(!memcmp(non + 128 * i, zero, 128));
    if (amount_is_zero(i)) {      // t^ = 0 (also given as l): the v1 functions byte for byte
      EXPECT(!memcmp(tags + 32 * i, tags1.data() + 32 * i, 32));
      EXPECT(!memcmp(non + 128 * i, non1.data() + 128 * i, 128));
      continue;
    }
    uint8_t tag[32], b0[64];
    reference_t(nul + (size_t)i * stride, kp + (size_t)i * 32, keys.data() + 64 * (keyed ? kidx[i] : 0), nonce_key, t + 32 * i, tag, b0);
    EXPECT(!memcmp(tags + 32 * i, tag, 32));
    EXPECT((tags[32 * i + 31] & 0xF0) == 0);
    EXPECT(memcmp(tags + 32 * i, tags1.data() + 32 * i, 32) != 0);
    if (!keyed) continue;
    EXPECT(!memcmp(non + 128 * i, b0, 64));
    EXPECT(memcmp(non + 128 * i, non + 128 * i + 64, 64) != 0);      // output block 1 is not block 0 again
    EXPECT(memcmp(non + 128 * i, non1.data() + 128 * i, 64) != 0 && memcmp(non + 128 * i + 64, non1.data() + 128 * i + 64, 64) != 0);
  }
  // a null amount array is every amount zero
  hc_rr_tags(n, stride, nul, kp, st.data(), nullptr, 0, nullptr, 0, tags);
  hc_rr_nonces(n, stride, nul, kp, st.data(), kidx.data(), keys.data(), nkeys, nonce_key, nullptr, 0, non);
  EXPECT(!memcmp(tags, tags1.data(), (size_t)n * 32) && !memcmp(non, non1.data(), (size_t)n * 128));
}

void check_reduction_and_counts() {
  uint8_t k[32], kp[32], keys[64], nonce_key[32], t1[32], t1l[32];
  for (auto& b : k) b = next_byte();
  for (auto& b : kp) b = next_byte();
  for (auto& b : keys) b = next_byte();
  for (auto& b : nonce_key) b = next_byte();
  small(t1, 5); add_ell(t1l, t1);
  const uint8_t st = 0, kidx = 0;
  uint8_t a[32], b[32], na[128], nb[128];
  hc_rr_tags(1, 32, k, kp, &st, nullptr, 0, t1, 0, a); hc_rr_tags(1, 32, k, kp, &st, nullptr, 0, t1l, 0, b);
  hc_rr_nonces(1, 32, k, kp, &st, &kidx, keys, 1, nonce_key, t1, 0, na); hc_rr_nonces(1, 32, k, kp, &st, &kidx, keys, 1, nonce_key, t1l, 0, nb);
  EXPECT(!memcmp(a, b, 32) && !memcmp(na, nb, 128));      // t and t + l are one amount
  small(t1l, 6);
  hc_rr_tags(1, 32, k, kp, &st, nullptr, 0, t1l, 0, b); hc_rr_nonces(1, 32, k, kp, &st, &kidx, keys, 1, nonce_key, t1l, 0, nb);
  EXPECT(memcmp(a, b, 32) != 0);
  for (int q = 0; q < 4; q++) EXPECT(memcmp(na + 32 * q, nb + 32 * q, 32) != 0);      // every quarter of the nonces differs
  // compressions per lane, counted: 2 for either tag, 4 for the v1 nonces, 5 for nonce_t; no field operation
  uint64_t c[3];
  uint8_t t[32];
  small(t, 0); hc_rr_lane_counts(t, c); EXPECT(c[0] == 2 && c[1] == 4 && c[2] == 0);
  memcpy(t, ELL, 32); hc_rr_lane_counts(t, c); EXPECT(c[0] == 2 && c[1] == 4 && c[2] == 0);
  small(t, 1); hc_rr_lane_counts(t, c); EXPECT(c[0] == 2 && c[1] == 5 && c[2] == 0);
  ell_minus_1(t); hc_rr_lane_counts(t, c); EXPECT(c[0] == 2 && c[1] == 5 && c[2] == 0);
}

// n records at L with Com_j = (a few) * B; candidate `bad_at` (if < n) has one Com_j of 0xFF bytes; candidate c's nullifier and amount
// lie at idx[c] = 2 c + 1 of arrays of 2 n entries.  K' by another road.
void check_kprime(int L, uint32_t n, uint32_t bad_at, bool with_t) {
  const ProofLayout pl{L};
  const size_t pb = pl.bytes();
  std::vector<uint8_t> recs(n * pb), kred((size_t)2 * n * 32), t((size_t)2 * n * 32 + 1), kp(n * 32, 0xAA), tag(n * 32, 0xAA), mark(n, 0xAA);
  uint8_t* tp = t.data() + 1;      // the amounts at an odd address
  std::vector<uint32_t> idx(n);
  for (auto& b : recs) b = next_byte();
  for (auto& b : kred) b = next_byte();
  for (uint32_t c = 0; c < n; c++) { idx[c] = 2 * c + 1; amount(tp + 32 * (size_t)(2 * c), c + 1); amount(tp + 32 * (size_t)(2 * c + 1), c); }
  std::vector<ge> pts((size_t)n * L);
  ge q = ge_basepoint();
  for (uint32_t c = 0; c < n; c++) for (int j = 0; j < L; j++) {
    for (int d = 0; d < 1 + (next_byte() & 3); d++) q = ge_add(ge_double(q), ge_basepoint());
    pts[(size_t)c * L + j] = q;
    uint32_t enc[8]; ristretto_encode(enc, q);
    store32_bytes(recs.data() + c * pb + 32 * pl.com(j), enc);
  }
  if (bad_at < n) memset(recs.data() + bad_at * pb + 32 * pl.com(L / 2), 0xFF, 32);
  uint64_t counts[4];
  EXPECT(hc_rr_kprime(L, n, recs.data(), kred.data(), idx.data(), with_t ? tp : nullptr, kp.data(), tag.data(), mark.data(), counts) == 1);
  const uint32_t good = n - (bad_at < n ? 1 : 0);
  EXPECT(counts[0] == counts[2]);                              // no added field operation
  EXPECT(counts[1] == 2 * (uint64_t)good && counts[3] == 2 * (uint64_t)good);      // two compressions for either tag
  const uint8_t zero[32] = {0};
  for (uint32_t c = 0; c < n; c++) {
    if (c == bad_at) { EXPECT(mark[c] == 1 && !memcmp(kp.data() + 32 * c, zero, 32) && !memcmp(tag.data() + 32 * c, zero, 32)); continue; }
    ge sum = ge_identity();
    for (int j = 0; j < L; j++) { ge p = pts[(size_t)c * L + j]; for (int d = 0; d < j; d++) p = ge_double(p); sum = ge_add(sum, p); }
    uint32_t enc[8], k[8], tw[8] = {0, 0, 0, 0, 0, 0, 0, 0}, want[8];
    ristretto_encode(enc, sum);
    uint8_t eb[32], tb[32]; store32_bytes(eb, enc);
    EXPECT(mark[c] == 0 && !memcmp(kp.data() + 32 * c, eb, 32));
    null_load_key(k, kred.data() + (size_t)idx[c] * 32);
    if (with_t) null_load_key(tw, tp + (size_t)idx[c] * 32);
    if (!with_t || amount_is_zero(c)) replay_tag(want, k, enc); else replay_tag_t(want, k, enc, tw);
    store32_bytes(tb, want);
    EXPECT(!memcmp(tag.data() + 32 * c, tb, 32) && (tag[32 * c + 31] & 0xF0) == 0);
  }
}
}  // namespace

int main() {
  for (uint32_t n : {1u, 65u, 257u}) for (uint32_t stride : {32u, 32u * 46u}) for (uint32_t shift : {0u, 1u}) check_derive(n, stride, shift);
  check_reduction_and_counts();
  for (int L : {3, 8}) for (uint32_t n : {1u, 65u}) { check_kprime(L, n, n, true); check_kprime(L, n, n / 2, true); check_kprime(L, n, n, false); }
  if (failures) { fprintf(stderr, "return_replay_check: %d failures\n", failures); return 1; }
  puts("RETURN REPLAY CHECK CLEAN");
  return 0;
}
#endif
