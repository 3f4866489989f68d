// reserve_check.cpp — TEST-ONLY stand-alone host program over the lane bodies of reserve and settle (csrc/reserve_lanes.h), as the
// kernels of k_reserve.hip run them (one lane per thread, the grid's tail lanes included).  tests/test_reserve_host.py builds it plain and
// under AddressSanitizer / UBSan and runs both: every buffer is a heap block of exactly its size, so a lane that strays is the
// sanitizer's to find.  reserve_tag and settle_marker are checked against blake3_hd.h's general hash over the spelled-out message;
// settle_prep_lane against rules written out here -- and, through the PREP lines it prints, against tests/reserve_cases.py.
// Never linked into libact_mi355x.so.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>
#define ACT_FE_BOUNDS 1
#define ACT_B3_COUNT 1
#include "../../anonymous-credit-tokens_amd/csrc/reserve_lanes.h"

namespace act { fe_bounds_t fe_bounds = {0, 0, 0, 0, 0, 0}; fe_counts_t fe_counts = {0, 0, {0, 0, 0, 0}}; uint64_t b3_compress_count = 0; }
using namespace act;

namespace {
int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { failures++; fprintf(stderr, "reserve_check: line %d: %s\n", __LINE__, #cond); } } while (0)

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint8_t next_byte() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint8_t)(rng_state >> 24); }
uint32_t grid_lanes(uint64_t n, uint32_t block) { return (uint32_t)(((n + block - 1) / block) * block); }

// a heap block of exactly `bytes` bytes behind `shift` unused ones: data() is at an odd address when shift is odd
struct Block {
  std::unique_ptr<uint8_t[]> p; size_t shift;
  Block(size_t bytes, size_t shift_, int fill = -1) : p(new uint8_t[bytes + shift_]), shift(shift_) {
    for (size_t i = 0; i < bytes + shift; i++) p[i] = fill < 0 ? next_byte() : (uint8_t)fill;
  }
  uint8_t* data() { return p.get() + shift; }
};

// l = 2^252 + 27742317777372353535851937790883648493, little-endian
const uint8_t ELL[32] = {0xed, 0xd3, 0xf5, 0x5c, 0x1a, 0x63, 0x12, 0x58, 0xd6, 0x9c, 0xf7, 0xa2, 0xde, 0xf9, 0xde, 0x14, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0x10};
void add_ell(uint8_t out[32], const uint8_t in[32]) {
  unsigned carry = 0;
  for (int i = 0; i < 32; i++) { const unsigned s = in[i] + ELL[i] + carry; out[i] = (uint8_t)s; carry = s >> 8; }
}
void small(uint8_t out[32], uint32_t v) { memset(out, 0, 32); out[0] = (uint8_t)v; out[1] = (uint8_t)(v >> 8); }
void hex(const uint8_t* b, size_t n) { for (size_t i = 0; i < n; i++) printf("%02x", b[i]); }

// the two hashes by another road: the message assembled in memory, k and s reduced, through the general b3_hash_xof64
void reference_res(const uint8_t k_raw[32], const uint8_t kp[32], const uint8_t s_raw[32], uint8_t tag[32]) {
  uint32_t kw[8], sw[8], msg[32], o[16];
  null_load_key(kw, k_raw); null_load_key(sw, s_raw);
  uint8_t* m = reinterpret_cast<uint8_t*>(msg);
  memset(msg, 0, sizeof(msg)); memcpy(m, "act-mi355x/reservation/v1", 25); memcpy(m + 32, kw, 32); memcpy(m + 64, kp, 32); memcpy(m + 96, sw, 32);
  b3_hash_xof64(o, msg, 128);
  memcpy(tag, o, 32); tag[31] &= 0x0F;
}
void reference_marker(const uint8_t k_raw[32], const uint8_t kp[32], uint8_t tag[32]) {
  uint32_t kw[8], msg[24], o[16];
  null_load_key(kw, k_raw);
  uint8_t* m = reinterpret_cast<uint8_t*>(msg);
  memset(msg, 0, sizeof(msg)); memcpy(m, "act-mi355x/settled/v1", 21); memcpy(m + 32, kw, 32); memcpy(m + 64, kp, 32);
  b3_hash_xof64(o, msg, 96);
  memcpy(tag, o, 32); tag[31] &= 0x0F;
}
void reference_amount(const uint8_t k_raw[32], const uint8_t kp[32], const uint8_t t_raw[32], uint8_t tag[32]) {
  uint32_t kw[8], kpw[8], tw[8], o[8];
  null_load_key(kw, k_raw); replay_load32(kpw, kp); null_load_key(tw, t_raw);
  return_replay_tag(o, kw, kpw, tw);      // (checked against BLAKE3 by return_replay_check.cpp)
  store32_bytes(tag, o);
}

void check_hashes() {
  uint32_t k[8], kp[8], s[8], a[8], b[8];
  uint8_t kb[32], kpb[32], sb[32], want[32], got[32];
  for (int round = 0; round < 4; round++) {
    for (int i = 0; i < 32; i++) { kb[i] = next_byte(); kpb[i] = next_byte(); sb[i] = round == 3 ? 0 : next_byte(); }
    null_load_key(k, kb); replay_load32(kp, kpb); null_load_key(s, sb);
    b3_compress_count = 0;
    reserve_tag(a, k, kp, s);
    EXPECT(b3_compress_count == 2);      // 128 bytes: two blocks
    store32_bytes(got, a); reference_res(kb, kpb, sb, want);
    EXPECT(!memcmp(got, want, 32) && (got[31] & 0xF0) == 0);
    b3_compress_count = 0;
    settle_marker(b, k, kp);
    EXPECT(b3_compress_count == 2);      // 96 bytes: two blocks, the second half full
    store32_bytes(got, b); reference_marker(kb, kpb, want);
    EXPECT(!memcmp(got, want, 32) && (got[31] & 0xF0) == 0);
    EXPECT(memcmp(a, b, 32) != 0);
    uint32_t v1[8], z[8] = {0, 0, 0, 0, 0, 0, 0, 0}, amt[8];
    replay_tag(v1, k, kp); return_replay_tag(amt, k, kp, s);
    EXPECT(memcmp(a, v1, 32) != 0 && memcmp(b, v1, 32) != 0 && memcmp(a, amt, 32) != 0);      // separated from the receipt tags, also at s = 0
    reserve_tag(amt, k, kp, z);
    EXPECT((round == 3) == !memcmp(a, amt, 32));
    // every input bit changes the output
    for (int w = 0; w < 24; w++) for (int bit = 0; bit < 32; bit++) {
      uint32_t k2[8], kp2[8], s2[8], o[8];
      memcpy(k2, k, 32); memcpy(kp2, kp, 32); memcpy(s2, s, 32);
      (w < 8 ? k2 : w < 16 ? kp2 : s2)[w % 8] ^= 1u << bit;
      reserve_tag(o, k2, kp2, s2);
      EXPECT(memcmp(o, a, 32) != 0);
      if (w < 16) { settle_marker(o, k2, kp2); EXPECT(memcmp(o, b, 32) != 0); }
    }
  }
}

// One settle_prep_lane case over exact-size blocks; rec / t at odd addresses when shift is odd.  Prints the PREP line the Python
// model reads and checks the rules written out here.
void prep_case(const uint8_t rec_in[96], uint8_t kidx_in, const uint8_t* t_in, uint32_t nkeys, size_t shift) {
  Block rec(96, shift), t(32, shift), tr(32, shift, 0xAA), tm(32, shift, 0xAA), ta(32, shift, 0xAA), kp(32, shift, 0xAA), st(1, 0, 0xAA), kidx(1, 0);
  memcpy(rec.data(), rec_in, 96); if (t_in) memcpy(t.data(), t_in, 32);
  kidx.data()[0] = kidx_in;
  SettlePrepArgs a{1, nkeys, rec.data(), kidx.data(), t_in ? t.data() : nullptr, tr.data(), tm.data(), ta.data(), kp.data(), st.data()};
  for (uint32_t i = 0; i < grid_lanes(1, 256); i++) settle_prep_lane(a, i);
  const uint8_t zero[32] = {0};
  uint8_t tz[32]; memset(tz, 0, 32);
  const uint8_t* tv = t_in ? t_in : tz;
  const bool too_big = return_exceeds_bytes(tv, rec_in + 64);
  const uint8_t want = kidx_in >= nkeys ? 248 : too_big ? 249 : 0;
  EXPECT(st.data()[0] == want);
  EXPECT(!memcmp(kp.data(), rec_in + 32, 32));
  if (want) EXPECT(!memcmp(tr.data(), zero, 32) && !memcmp(tm.data(), zero, 32) && !memcmp(ta.data(), zero, 32));
  else {
    uint8_t w[32];
    reference_res(rec_in, rec_in + 32, rec_in + 64, w); EXPECT(!memcmp(tr.data(), w, 32));
    reference_marker(rec_in, rec_in + 32, w); EXPECT(!memcmp(tm.data(), w, 32));
    reference_amount(rec_in, rec_in + 32, tv, w); EXPECT(!memcmp(ta.data(), w, 32));
  }
  printf("PREP "); hex(rec_in, 96); printf(" %u ", (unsigned)kidx_in);
  if (t_in) hex(t_in, 32); else printf("-");
  printf(" %u %u ", nkeys, (unsigned)st.data()[0]); hex(tr.data(), 32); printf(" "); hex(tm.data(), 32); printf(" "); hex(ta.data(), 32); printf("\n");
}

void check_prep() {
  const uint32_t nkeys = 3, S = 300;
  uint8_t rec[96], t[32], s[32], one[32];
  for (size_t shift : {(size_t)0, (size_t)1}) {
    for (int i = 0; i < 64; i++) rec[i] = next_byte();
    // s = 300: t = 0, 1, s - 1, s, s + 1, s + l, 2^200 + 1; then no amounts at all
    small(s, S); memcpy(rec + 64, s, 32);
    for (uint32_t v : {0u, 1u, S - 1, S, S + 1}) { small(t, v); prep_case(rec, 0, t, nkeys, shift); }
    add_ell(t, s); prep_case(rec, 1, t, nkeys, shift);
    small(t, 1); t[25] = 1; prep_case(rec, 2, t, nkeys, shift);
    prep_case(rec, 0, nullptr, nkeys, shift);
    // the record's own k and s unreduced: k + l, s + l are the same reservation
    uint8_t rec2[96]; memcpy(rec2, rec, 96); rec2[31] &= 0x0F; add_ell(rec2, rec2); add_ell(rec2 + 64, s);
    small(t, S); prep_case(rec2, 0, t, nkeys, shift);
    // s = 0: t = 0 passes, t = 1 does not, t = l is t = 0
    small(s, 0); memcpy(rec + 64, s, 32);
    small(t, 0); prep_case(rec, 0, t, nkeys, shift);
    small(one, 1); prep_case(rec, 0, one, nkeys, shift);
    prep_case(rec, 0, ELL, nkeys, shift);
    prep_case(rec, 0, nullptr, nkeys, shift);
    // the key index: nkeys - 1, nkeys, 255; the index rule stands in front of the amount's
    small(s, S); memcpy(rec + 64, s, 32); small(t, 5);
    for (uint32_t kx : {nkeys - 1, nkeys, 255u}) prep_case(rec, (uint8_t)kx, t, nkeys, shift);
    small(t, S + 1); prep_case(rec, (uint8_t)nkeys, t, nkeys, shift);
  }
  // a batch: 257 lanes over exact-size arrays, the grid's tail lanes included, amounts null and given
  const uint32_t n = 257;
  for (size_t shift : {(size_t)0, (size_t)1}) for (int with_t = 0; with_t < 2; with_t++) {
    Block recs((size_t)n * 96, shift), ts((size_t)n * 32, shift), kidx(n, 0), tr((size_t)n * 32, shift, 0xAA), tm((size_t)n * 32, shift, 0xAA), ta((size_t)n * 32, shift, 0xAA),
        st(n, 0, 0xAA);
    for (uint32_t i = 0; i < n; i++) {
      kidx.data()[i] = (uint8_t)(i % 5 == 4 ? 200 : i % nkeys);
      small(recs.data() + 96 * (size_t)i + 64, 10); small(ts.data() + 32 * (size_t)i, i % 13);      // t = 11, 12 exceed s = 10
    }
    SettlePrepArgs a{n, nkeys, recs.data(), kidx.data(), with_t ? ts.data() : nullptr, tr.data(), tm.data(), ta.data(), nullptr, st.data()};
    for (uint32_t i = 0; i < grid_lanes(n, 256); i++) settle_prep_lane(a, i);
    for (uint32_t i = 0; i < n; i++) {
      const uint8_t want = kidx.data()[i] >= nkeys ? 248 : (with_t && i % 13 > 10) ? 249 : 0;
      EXPECT(st.data()[i] == want);
      uint8_t w[32] = {0};
      if (!want) reference_res(recs.data() + 96 * (size_t)i, recs.data() + 96 * (size_t)i + 32, recs.data() + 96 * (size_t)i + 64, w);
      EXPECT(!memcmp(tr.data() + 32 * (size_t)i, w, 32));
    }
  }
}

void check_found_and_merge() {
  for (int st = 0; st < 256; st++) for (int found = 0; found < 2; found++) {
    uint8_t s = (uint8_t)st, f = (uint8_t)found;
    SettleFoundArgs a{1, &f, &s};
    settle_found_lane(a, 0); settle_found_lane(a, 1);
    EXPECT(s == (st == 0 && !found ? 248 : st));
  }
  // (status, the marker's answer, the amount tag's answer) through replay_resolve and settle_merge
  struct { uint8_t st, spent, found, want, before, skip; } rows[] = {
    {0, 0, 0, 0, 0, 0}, {0, 0, 1, 0, 0, 0}, {0, 1, 1, 0, 1, 1}, {0, 1, 0, 247, 0, 1}, {0, 2, 0, 252, 0, 1}, {248, 0, 0, 248, 0, 1}, {249, 1, 1, 249, 0, 1}};
  for (auto& r : rows) {
    uint8_t st = r.st, skip = 9, sp = 9, before = 9;
    ReplayResolveArgs ra{1, &st, &r.spent, nullptr, &skip, &sp, &before};
    replay_resolve_lane(ra, 0);
    EXPECT(skip == r.skip);
    ra.found = &r.found; replay_resolve_lane(ra, 0);
    SettleMergeArgs ma{1, &sp, &st};
    settle_merge_lane(ma, 0); settle_merge_lane(ma, 1);
    EXPECT(st == r.want && before == r.before);
  }
}

void check_tag_and_emit(uint32_t n, uint32_t stride, size_t shift) {
  Block nul((size_t)(n - 1) * stride + 32, shift), kp((size_t)n * 32, shift), s((size_t)n * 32, shift), st(n, 0), tags((size_t)n * 32, shift, 0xAA), out((size_t)n * 96, shift, 0xAA),
      status(n, 0, 0xAA), sred((size_t)n * 32, 0, 0xAA);
  for (uint32_t i = 0; i < n; i++) st.data()[i] = (uint8_t)(i % 4 == 3 ? i % 256 : 0);      // every non-zero status somewhere at n = 1025
  if (n > 1) memcpy(s.data() + 32, ELL, 32);      // lane 1: s = l, that is s^ = 0
  ReplayDeriveArgs ta{}; ta.n = n; ta.stride = stride; ta.nul = nul.data(); ta.kp = kp.data(); ta.st = st.data(); ta.out = tags.data(); ta.t = s.data();
  for (uint32_t i = 0; i < grid_lanes(n, 256); i++) reserve_tag_lane(ta, i);
  ReserveEmitArgs ea{n, stride, nul.data(), kp.data(), s.data(), st.data(), out.data(), status.data()};
  for (uint32_t i = 0; i < grid_lanes(n, 256); i++) reserve_emit_lane(ea, i);
  // s^ beside k^: the charge is the 32 bytes behind the nullifier (stride >= 64 only)
  if (stride >= 64) {
    ReserveSredArgs sa{n, stride, nul.data(), sred.data()};
    Block ks((size_t)(n - 1) * stride + 64, shift);
    sa.ks = ks.data();
    for (uint32_t i = 0; i < grid_lanes(n, 256); i++) reserve_sred_lane(sa, i);
    for (uint32_t i = 0; i < n; i++) { uint32_t w[8]; uint8_t b[32]; null_load_key(w, ks.data() + (size_t)i * stride + 32); store32_bytes(b, w); EXPECT(!memcmp(sred.data() + 32 * (size_t)i, b, 32)); }
  }
  const uint8_t zero[96] = {0};
  for (uint32_t i = 0; i < n; i++) {
    EXPECT(status.data()[i] == st.data()[i]);
    if (st.data()[i]) { EXPECT(!memcmp(tags.data() + 32 * (size_t)i, zero, 32) && !memcmp(out.data() + 96 * (size_t)i, zero, 96)); continue; }
    uint8_t w[32], rec[96]; uint32_t kw[8], sw[8];
    reference_res(nul.data() + (size_t)i * stride, kp.data() + 32 * (size_t)i, s.data() + 32 * (size_t)i, w);
    EXPECT(!memcmp(tags.data() + 32 * (size_t)i, w, 32));
    null_load_key(kw, nul.data() + (size_t)i * stride); null_load_key(sw, s.data() + 32 * (size_t)i);
    store32_bytes(rec, kw); memcpy(rec + 32, kp.data() + 32 * (size_t)i, 32); store32_bytes(rec + 64, sw);
    EXPECT(!memcmp(out.data() + 96 * (size_t)i, rec, 96));
    if (i == 1) EXPECT(!memcmp(rec + 64, zero, 32));
  }
}

// reserve_emit_lane writes zeros for EVERY non-zero status, and the record for 0; the output row at an odd address
void check_emit_every_status() {
  for (int v = 0; v < 256; v++) {
    Block nul(32, 1), kp(32, 1), s(32, 1), out(96, 1, 0xAA), st(1, 0), status(1, 0, 0xAA);
    st.data()[0] = (uint8_t)v;
    ReserveEmitArgs ea{1, 32, nul.data(), kp.data(), s.data(), st.data(), out.data(), status.data()};
    for (uint32_t i = 0; i < 256; i++) reserve_emit_lane(ea, i);
    const uint8_t zero[96] = {0};
    EXPECT(status.data()[0] == (uint8_t)v);
    EXPECT((v != 0) == !memcmp(out.data(), zero, 96));
    if (v == 0) EXPECT(!memcmp(out.data() + 32, kp.data(), 32));
  }
}

// n records at L with Com_j = (a few) * B; candidate `bad_at` (if < n) has one Com_j of 0xFF bytes; candidate c's nullifier and charge
// lie at idx[c] = 2 c + 1 of arrays of 2 n entries.  K' by another road.
void check_kprime(int L, uint32_t n, uint32_t bad_at) {
  const ProofLayout pl{L};
  const size_t pb = pl.bytes();
  Block recs(n * pb, 0), kred((size_t)2 * n * 32, 0), sred((size_t)2 * n * 32, 1), kp(n * 32, 0, 0xAA), tag(n * 32, 0, 0xAA), mark(n, 0, 0xAA);
  std::vector<uint32_t> idx(n), coords((size_t)n * L * NIELS_WORDS), flags(n, 0);
  for (uint32_t c = 0; c < n; c++) idx[c] = 2 * c + 1;
  std::vector<ge> pts((size_t)n * L);
  ge q = ge_basepoint();
  for (uint32_t c = 0; c < n; c++) for (int j = 0; j < L; j++) {
    for (int d = 0; d < 1 + (next_byte() & 3); d++) q = ge_add(ge_double(q), ge_basepoint());
    pts[(size_t)c * L + j] = q;
    uint32_t enc[8]; ristretto_encode(enc, q);
    store32_bytes(recs.data() + c * pb + 32 * pl.com(j), enc);
  }
  if (bad_at < n) memset(recs.data() + bad_at * pb + 32 * pl.com(L / 2), 0xFF, 32);
  KprimeArgs a{};
  a.s.P.L = L; a.s.proofs = recs.data(); a.s.n = n; a.s.coords = coords.data(); a.s.flags = flags.data();
  a.kred = kred.data(); a.idx = idx.data(); a.kp = kp.data(); a.tag = tag.data(); a.mark = mark.data(); a.t = sred.data();
  for (uint32_t g = 0; g < grid_lanes((uint64_t)n * L, 64); g++) kprime_decode_lane(a, g);
  for (uint32_t c = 0; c < grid_lanes(n, 64); c++) kprime_tag_reserve_lane(a, c);
  const uint8_t zero[32] = {0};
  for (uint32_t c = 0; c < n; c++) {
    if (c == bad_at) { EXPECT(mark.data()[c] == 1 && !memcmp(kp.data() + 32 * c, zero, 32) && !memcmp(tag.data() + 32 * c, zero, 32)); continue; }
    ge sum = ge_identity();
    for (int j = 0; j < L; j++) { ge p = pts[(size_t)c * L + j]; for (int d = 0; d < j; d++) p = ge_double(p); sum = ge_add(sum, p); }
    uint32_t enc[8];
    ristretto_encode(enc, sum);
    uint8_t eb[32], w[32]; store32_bytes(eb, enc);
    EXPECT(mark.data()[c] == 0 && !memcmp(kp.data() + 32 * c, eb, 32));
    reference_res(kred.data() + (size_t)idx[c] * 32, eb, sred.data() + (size_t)idx[c] * 32, w);
    EXPECT(!memcmp(tag.data() + 32 * c, w, 32));
  }
}
}  // namespace

int main() {
  check_hashes();
  check_prep();
  check_found_and_merge();
  check_emit_every_status();
  for (uint32_t n : {1u, 65u, 1025u}) for (uint32_t stride : {32u, 32u * 46u}) for (size_t shift : {(size_t)0, (size_t)1}) check_tag_and_emit(n, stride, shift);
  for (uint32_t n : {1u, 65u}) { check_kprime(3, n, n); check_kprime(3, n, n / 2); }
  if (failures) { fprintf(stderr, "reserve_check: %d failures\n", failures); return 1; }
  puts("RESERVE CHECK CLEAN");
  return 0;
}
