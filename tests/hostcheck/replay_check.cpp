// replay_check.cpp — TEST-ONLY host build of the replay lane bodies (csrc/replay_lanes.h): the receipt tag, the derived refund nonce
// and the resolve step, as the kernels of k_replay.hip run them (one lane per thread, the grid's tail lanes included).  Built by
// tests/replay_cases.py as a small library for tests/test_replay_host.py; with -DREPLAY_CHECK_MAIN it is a stand-alone program that
// checks the same bodies itself (against blake3_hd.h's general hash over the assembled message) and is run under the sanitizers.
// Never linked into libact_mi355x.so.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../anonymous-credit-tokens_amd/csrc/replay_lanes.h"

using namespace act;

namespace {
// nonce_key | ring records where the lane body wants them: 4-byte aligned
struct Secrets {
  uint32_t w[REPLAY_SECRET_BYTES / 4];
  Secrets(const uint8_t nonce_key[32], const uint8_t* keys, uint32_t nkeys) { memset(w, 0, sizeof(w)); memcpy(w, nonce_key, 32); memcpy(w + 8, keys, (size_t)nkeys * 64); }
};
uint32_t grid_lanes(uint32_t n) { return ((n + 255) / 256) * 256; }
}  // namespace

extern "C" {

void hc_replay_tags(uint32_t n, uint32_t stride, const uint8_t* nul, const uint8_t* kp, const uint8_t* st, const uint8_t* kidx, uint32_t nkeys, uint8_t* out) {
  ReplayDeriveArgs a{}; a.n = n; a.stride = stride; a.nkeys = nkeys; a.nul = nul; a.kp = kp; a.st = st; a.kidx = kidx; a.out = out;
  for (uint32_t i = 0; i < grid_lanes(n); i++) replay_tag_lane(a, i);
}
void hc_replay_nonces(uint32_t n, uint32_t stride, const uint8_t* nul, const uint8_t* kp, const uint8_t* st, const uint8_t* kidx, const uint8_t* keys, uint32_t nkeys,
                      const uint8_t nonce_key[32], uint8_t* out) {
  const Secrets sec(nonce_key, keys, nkeys);
  ReplayDeriveArgs a{}; a.n = n; a.stride = stride; a.nkeys = nkeys; a.nul = nul; a.kp = kp; a.st = st; a.kidx = kidx;
  a.secrets = reinterpret_cast<const uint8_t*>(sec.w); a.out = out;
  for (uint32_t i = 0; i < grid_lanes(n); i++) replay_nonce_lane(a, i);
}
// out[0..3) = skip, sp, replayed
void hc_replay_resolve(int verdict, int spent, int found, uint8_t out[3]) {
  const ReplayResolved r = replay_resolve((uint8_t)verdict, (uint8_t)spent, (uint8_t)found);
  out[0] = r.skip; out[1] = r.sp; out[2] = r.replayed;
}
// found == NULL: the pass in front of the receipts insert (skip[] only)
void hc_replay_resolve_lanes(uint32_t n, const uint8_t* st, const uint8_t* spent, const uint8_t* found, uint8_t* skip, uint8_t* sp, uint8_t* replayed) {
  const ReplayResolveArgs a{n, st, spent, found, skip, sp, replayed};
  for (uint32_t i = 0; i < grid_lanes(n); i++) replay_resolve_lane(a, i);
}

}  // extern "C"

#if defined(REPLAY_CHECK_MAIN)
namespace {
int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { failures++; fprintf(stderr, "replay_check: line %d: %s\n", __LINE__, #cond); } } while (0)

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint8_t next_byte() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint8_t)(rng_state >> 24); }

// the same hashes by another road: the message assembled in memory, reduced k included, through the general b3_hash_xof64
void reference(const uint8_t k_raw[32], const uint8_t kp[32], const uint8_t key[64], const uint8_t nonce_key[32], uint8_t tag[32], uint8_t block0[64]) {
  uint32_t kw[8]; null_load_key(kw, k_raw);
  uint32_t msg[48], o[16];
  uint8_t* m = reinterpret_cast<uint8_t*>(msg);
  memset(msg, 0, sizeof(msg)); memcpy(m, "act-mi355x/receipt/v1", 21); memcpy(m + 32, kw, 32); memcpy(m + 64, kp, 32);
  b3_hash_xof64(o, msg, 96);
  memcpy(tag, o, 32); tag[31] &= 0x0F;
  memset(msg, 0, sizeof(msg)); memcpy(m, "act-mi355x/refund-nonce/v1", 26); memcpy(m + 32, nonce_key, 32); memcpy(m + 64, key, 64); memcpy(m + 128, kw, 32); memcpy(m + 160, kp, 32);
  b3_hash_xof64(o, msg, 192);
  memcpy(block0, o, 64);
}

void check_derive(uint32_t n, uint32_t stride, uint32_t shift, int fill) {
  const uint32_t nkeys = 3;
  // exact-size heap blocks, the arrays at an odd byte offset when shift is odd: a read or write past an array is the sanitizer's to find
  std::vector<uint8_t> nul_b((size_t)(n - 1) * stride + 32 + shift), kp_b((size_t)n * 32 + shift), st(n), kidx(n), keys(nkeys * 64), tags_b((size_t)n * 32 + shift), non_b((size_t)n * 128 + shift);
  uint8_t nonce_key[32];
  uint8_t *nul = nul_b.data() + shift, *kp = kp_b.data() + shift, *tags = tags_b.data() + shift, *non = non_b.data() + shift;
  auto gen = [&]() -> uint8_t { return fill < 0 ? next_byte() : (uint8_t)fill; };
  for (auto& b : nul_b) b = gen();
  for (auto& b : kp_b) b = gen();
  for (auto& b : keys) b = gen();
  for (auto& b : nonce_key) b = gen();
  for (uint32_t i = 0; i < n; i++) { st[i] = (i % 5 == 3) ? 7 : 0; kidx[i] = (uint8_t)((i % 7 == 6) ? 255 : i % nkeys); }
  memset(tags_b.data(), 0xAA, tags_b.size()); memset(non_b.data(), 0xAA, non_b.size());
  hc_replay_tags(n, stride, nul, kp, st.data(), nullptr, 0, tags);
  hc_replay_nonces(n, stride, nul, kp, st.data(), kidx.data(), keys.data(), nkeys, nonce_key, non);
  const uint8_t zero[128] = {0};
  for (uint32_t i = 0; i < n; i++) {
    uint8_t tag[32], b0[64];
    const uint8_t* key = keys.data() + 64 * (kidx[i] < nkeys ? kidx[i] : 0);
    reference(nul + (size_t)i * stride, kp + (size_t)i * 32, key, nonce_key, tag, b0);
    if (st[i]) { EXPECT(!memcmp(tags + 32 * i, zero, 32)); EXPECT(!memcmp(non + 128 * i, zero, 128)); continue; }
    EXPECT(!memcmp(tags + 32 * i, tag, 32));
    EXPECT((tags[32 * i + 31] & 0xF0) == 0);
    if (kidx[i] >= nkeys) { EXPECT(!memcmp(non + 128 * i, zero, 128)); continue; }
    EXPECT(!memcmp(non + 128 * i, b0, 64));
    EXPECT(memcmp(non + 128 * i, non + 128 * i + 64, 64) != 0);      // output block 1 is not block 0 again
  }
  // with key indices the tag takes part only where the index names a ring key
  hc_replay_tags(n, stride, nul, kp, st.data(), kidx.data(), nkeys, tags);
  for (uint32_t i = 0; i < n; i++) if (st[i] == 0 && kidx[i] >= nkeys) EXPECT(!memcmp(tags + 32 * i, zero, 32));
}

void check_reduction() {
  // l = 2^252 + 27742317777372353535851937790883648493, little-endian; k and k + l are one nullifier
  const uint8_t ell[32] = {0xed, 0xd3, 0xf5, 0x5c, 0x1a, 0x63, 0x12, 0x58, 0xd6, 0x9c, 0xf7, 0xa2, 0xde, 0xf9, 0xde, 0x14, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0x10};
  uint8_t k[32], kl[32], kp[32], keys[64], nonce_key[32];
  for (auto& b : k) b = next_byte();
  k[31] &= 0x0F;
  unsigned carry = 0;
  for (int i = 0; i < 32; i++) { const unsigned s = k[i] + ell[i] + carry; kl[i] = (uint8_t)s; carry = s >> 8; }
  EXPECT(carry == 0);
  for (auto& b : kp) b = next_byte();
  for (auto& b : keys) b = next_byte();
  for (auto& b : nonce_key) b = next_byte();
  const uint8_t st = 0, kidx = 0;
  uint8_t t0[32], t1[32], n0[128], n1[128];
  hc_replay_tags(1, 32, k, kp, &st, nullptr, 0, t0); hc_replay_tags(1, 32, kl, kp, &st, nullptr, 0, t1);
  hc_replay_nonces(1, 32, k, kp, &st, &kidx, keys, 1, nonce_key, n0); hc_replay_nonces(1, 32, kl, kp, &st, &kidx, keys, 1, nonce_key, n1);
  EXPECT(!memcmp(t0, t1, 32) && !memcmp(n0, n1, 128));
  kp[0] ^= 1;      // another K': another tag, other nonces
  hc_replay_tags(1, 32, k, kp, &st, nullptr, 0, t1); hc_replay_nonces(1, 32, k, kp, &st, &kidx, keys, 1, nonce_key, n1);
  EXPECT(memcmp(t0, t1, 32) != 0 && memcmp(n0, n1, 64) != 0 && memcmp(n0 + 64, n1 + 64, 64) != 0);
}

void check_resolve() {
  for (int verdict : {0, 6, 7, 255}) for (int spent = 0; spent < 3; spent++) for (int found = 0; found < 2; found++) {
    uint8_t r[3]; hc_replay_resolve(verdict, spent, found, r);
    const bool ok = verdict == 0;
    EXPECT(r[0] == ((ok && spent == 0) ? 0 : 1));                                          // a receipt only where k was fresh
    EXPECT(r[1] == (!ok ? 0 : spent == 0 ? 0 : spent == 1 ? (found ? 0 : 1) : 2));
    EXPECT(r[2] == ((ok && spent == 1 && found) ? 1 : 0));
  }
  const uint32_t n = 257;
  std::vector<uint8_t> st(n), spent(n), found(n), skip(n, 9), sp(n, 9), rep(n, 9);
  for (uint32_t i = 0; i < n; i++) { st[i] = (i % 4 == 1) ? 7 : 0; spent[i] = (uint8_t)(i % 3); found[i] = (uint8_t)((i / 3) % 2); }
  hc_replay_resolve_lanes(n, st.data(), spent.data(), nullptr, skip.data(), sp.data(), rep.data());
  for (uint32_t i = 0; i < n; i++) EXPECT(sp[i] == 9 && rep[i] == 9 && skip[i] == ((st[i] == 0 && spent[i] == 0) ? 0 : 1));
  hc_replay_resolve_lanes(n, st.data(), spent.data(), found.data(), skip.data(), sp.data(), rep.data());
  for (uint32_t i = 0; i < n; i++) { uint8_t r[3]; hc_replay_resolve(st[i], spent[i], found[i], r); EXPECT(sp[i] == r[1] && rep[i] == r[2]); }
}
}  // namespace

int main() {
  for (uint32_t n : {1u, 65u, 257u}) for (uint32_t stride : {32u, 32u * 46u}) for (uint32_t shift : {0u, 1u}) check_derive(n, stride, shift, -1);
  check_derive(5, 32, 0, 0x00);
  check_derive(5, 32, 1, 0xFF);
  check_reduction();
  check_resolve();
  if (failures) { fprintf(stderr, "replay_check: %d failures\n", failures); return 1; }
  puts("REPLAY CHECK CLEAN");
  return 0;
}
#endif
