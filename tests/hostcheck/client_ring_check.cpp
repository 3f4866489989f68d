// client_ring_check.cpp — TEST-ONLY host build of the client-ring lane bodies (csrc/client_ring_lanes.h), on top of everything
// hostcheck.cpp offers (its tables, its hc_* functions: this unit is hostcheck.cpp plus the client ring).  Built by
// tests/client_ring_cases.py as a shared object for tests/test_client_ring_host.py and, with -DCLIENT_RING_MAIN, as a stand-alone
// program that replays a case file under the sanitizers; never linked into libact_mi355x.so.
//
// Phase A of ring key 0 is a __global__ kernel (k_client.hip k_client_decode_com / k_client_a) with no host-compilable lane body; the
// two functions below restate it statement by statement so that the ring bodies find the transcripts, flags and XOF words they find
// on the device.  The kernels themselves are judged on the GPU (tests/test_gpu_client_ring.py).
#include "hostcheck.cpp"
#include "../../anonymous-credit-tokens_amd/csrc/client_ring_lanes.h"
#include <cstdio>
#include <map>
#include <string>

namespace {

void host_client_decode_com(const ClientArgs& a, uint32_t p, uint32_t j) {
  const int L = a.P.L;
  const ProofLayout pl{L};
  uint32_t wc[8]; load8(wc, a.proofs + (size_t)p * pl.bytes() + 32 * pl.com(j));
  ge C;
  if (!ristretto_decode(C, wc)) a.flags[p] |= FLAG_UNDECODABLE;
  niels_store(a.coords + ((size_t)p * L + j) * NIELS_WORDS, niels_from_affine(C));
}
void host_client_a(const ClientArgs& a, uint32_t p) {
  const int L = a.P.L;
  const bool issuance = a.label == LABEL_RESPOND;
  const uint8_t* resp = a.resp + (size_t)p * (issuance ? 160 : 128);
  uint32_t flags = issuance ? 0u : a.flags[p];
  uint32_t wa[8]; load8(wa, resp);
  ge A; if (!ristretto_decode(A, wa)) flags |= FLAG_UNDECODABLE;
  sc e = load_sc(resp + 32), gamma = load_sc(resp + 64), z = load_sc(resp + 96);
  ge xa; sc c = sc_zero();
  if (issuance) {
    uint32_t wk[8]; load8(wk, a.req + (size_t)p * 128);
    ge K; if (!ristretto_decode(K, wk)) flags |= FLAG_UNDECODABLE;
    c = load_sc(resp + 128);
    xa = ge_add(fixed_base_acc(ge_basepoint(), a.P.tab[BASE_H1], c), K);
  } else {
    ge kp = ge_identity();
    for (int j = L - 1; j >= 0; j--) { kp = ge_double(kp); kp = ge_madd(kp, niels_load(a.coords + ((size_t)p * L + j) * NIELS_WORDS)); }
    xa = ge_add(kp, ge_basepoint());
  }
  sc ng = sc_neg(gamma);
  ge xg = ge_add(fixed_base_acc(ge_identity(), a.P.tab[BASE_G], e), a.w);
  ge acc[2];
  acc[0] = ge_identity();
  acc[1] = fixed_base_acc(ge_identity(), a.P.tab[BASE_G], sc_sub(z, sc_mul(gamma, e)));
  uint32_t* bk = a.pbk + (size_t)p * 2 * BUCKET_WORDS;
  sc s1[1] = {z}; chain_b<1>(acc, A, s1, bk);
  sc s2[1] = {ng}; chain_b<1>(acc, xa, s2, bk);
  ge yg[1] = {acc[1]}; chain_b<1>(yg, a.w, s2, bk);
  uint8_t* tr = a.trs + (size_t)p * SMALL_TR_STRIDE;
  tr_put_prefix(tr, a.P, a.label);
  uint8_t* el = tr + a.P.prefix_len[a.label];
  if (issuance) { tr_put_bytes(el, c.v); el += 40; }
  tr_put_bytes(el, e.v); el += 40;
  uint32_t enc[8];
  tr_put_bytes(el, wa); el += 40;
  ristretto_encode(enc, xa); tr_put_bytes(el, enc); el += 40;
  ristretto_encode(enc, xg); tr_put_bytes(el, enc); el += 40;
  ristretto_encode(enc, acc[0]); tr_put_bytes(el, enc); el += 40;
  ristretto_encode(enc, yg[0]); tr_put_bytes(el, enc);
  a.flags[p] = flags;
}

// the table of a ring key at CLIENT_RING_WBITS, entry by entry with the lane body of k_build_table (msm.h fb_table_entry), kept per key
std::map<std::string, std::vector<uint32_t>> g_ring_tabs;
const uint32_t* ring_table(const uint8_t w_enc[32]) {
  const std::string key((const char*)w_enc, 32);
  auto it = g_ring_tabs.find(key);
  if (it != g_ring_tabs.end()) return it->second.data();
  uint32_t w[8]; ld(w, w_enc);
  ge b; if (!ristretto_decode(b, w)) return nullptr;
  std::vector<uint32_t>& tab = g_ring_tabs[key];
  tab.assign(fb_table_words(CLIENT_RING_WBITS), 0u);
  const uint32_t lanes = fb_windows(CLIENT_RING_WBITS) << CLIENT_RING_WBITS;
  for (uint32_t gid = 0; gid < lanes; gid++) niels_store(&tab[(size_t)gid * NIELS_WORDS], fb_table_entry(b, CLIENT_RING_WBITS, gid));
  return tab.data();
}
void fill_params(DevParams& P, const uint8_t* h, int L) {
  for (int b = 0; b < 4; b++) P.tab[b] = FbTab{g_tabs.tab[b].data(), (uint32_t)FB_WBITS, (uint32_t)b};
  P.half_h1 = nullptr; P.L = L;
  static const char* const labels[4] = {"request", "respond", "spend", "refund"};
  static const char version[] = "curve25519-ristretto anonymous-credits v1.0";
  for (int l = 0; l < 4; l++) {
    std::vector<uint8_t> p; put_lp(p, (const uint8_t*)version, sizeof(version) - 1);
    put_lp(p, h, 32); put_lp(p, h + 32, 32); put_lp(p, h + 64, 32); put_lp(p, (const uint8_t*)labels[l], strlen(labels[l]));
    P.prefix_len[l] = (uint32_t)p.size(); p.resize(PREFIX_WORDS * 4, 0); memcpy(P.prefix[l], p.data(), PREFIX_WORDS * 4);
  }
}
uint64_t ops() { return fe_counts.mul + fe_counts.sq; }

}  // namespace

// One ring call over n items, lane by lane, in the order the engine launches the kernels: decode_com (refund), phase A under ring key
// 0, BLAKE3 of key 0's transcripts, candidates, their patched hashes, ring finish.  issuance != 0: pre n*64, req n*128, resp n*160;
// else pre n*96, proofs, resp n*128.  out_cand: n * (nkeys - 1) * 64.
//   counts[0] = fe_mul + fe_sq of the one-key body (decode_com + phase A)     counts[1] = of everything the ring adds
//   counts[2], [3] = fixed_base_acc calls on g / on the ring tables in the ring's part     counts[4] = this build's window count of g
extern "C" int hc_client_ring(const uint8_t* h, int L, int issuance, const uint8_t* ring_w, uint32_t nkeys, uint32_t n, const uint8_t* pre,
                              const uint8_t* req, const uint8_t* proofs, const uint8_t* resp, uint8_t* out_token, uint8_t* out_status,
                              uint8_t* out_key, uint8_t* out_cand, uint64_t* counts) {
  if (L < 1 || L > 128 || nkeys < 1 || nkeys > (uint32_t)KEYRING_MAX || !build_tables(h)) return 0;
  const uint32_t extra = nkeys - 1u;
  std::vector<uint32_t> tabw((size_t)(extra ? extra : 1u) * fb_table_words(CLIENT_RING_WBITS));
  for (uint32_t k = 1; k < nkeys; k++) {
    const uint32_t* t = ring_table(ring_w + 32 * k);
    if (!t) return 0;
    memcpy(&tabw[(size_t)(k - 1) * fb_table_words(CLIENT_RING_WBITS)], t, fb_table_words(CLIENT_RING_WBITS) * 4);
  }
  ClientRingArgs r{};
  ClientArgs& a = r.c;
  fill_params(a.P, h, L);
  { uint32_t w[8]; ld(w, ring_w); if (!ristretto_decode(a.w, w)) return 0; }
  std::vector<uint32_t> coords((size_t)n * L * NIELS_WORDS), flags(n, 0u), xof((size_t)n * 16), pbk((size_t)n * PREP_BUCKET_SETS * BUCKET_WORDS),
      xofs((size_t)n * (extra ? extra : 1u) * 16);
  std::vector<uint8_t> trs((size_t)n * SMALL_TR_STRIDE, 0), cand((size_t)n * (extra ? extra : 1u) * 64, 0);
  a.n = n; a.label = issuance ? LABEL_RESPOND : LABEL_REFUND; a.pre = pre; a.req = req; a.resp = resp; a.proofs = proofs;
  a.coords = coords.data(); a.trs = trs.data(); a.flags = flags.data(); a.xof = xof.data(); a.out_token = out_token; a.status = out_status; a.pbk = pbk.data();
  r.tabw = tabw.data(); r.nkeys = nkeys; r.cand = cand.data(); r.xofs = xofs.data(); r.out_key = out_key;
  fe_counts = fe_counts_t{0, 0, {0, 0, 0, 0}};
  if (!issuance) for (uint32_t p = 0; p < n; p++) for (uint32_t j = 0; j < (uint32_t)L; j++) host_client_decode_com(a, p, j);
  for (uint32_t p = 0; p < n; p++) host_client_a(a, p);
  uint64_t c[5] = {ops(), 0, 0, 0, (uint64_t)FB_WINDOWS};
  for (uint32_t p = 0; p < n; p++)
    b3_hash_xof64(&xof[(size_t)p * 16], reinterpret_cast<const uint32_t*>(trs.data() + (size_t)p * SMALL_TR_STRIDE), client_ring_tr_len(a.P, a.label));
  fe_counts = fe_counts_t{0, 0, {0, 0, 0, 0}};
  for (uint32_t g = 0; g < n * extra; g++) client_ring_cand_lane(r, g);
  for (uint32_t g = 0; g < n * extra; g++) client_ring_hash_lane(r, g);
  for (uint32_t p = 0; p < n; p++) client_ring_finish_lane(r, p);
  c[1] = ops(); c[2] = fe_counts.fixed_base[BASE_G]; c[3] = fe_counts.fixed_base[CLIENT_RING_TAB_ID];
  if (extra && out_cand) memcpy(out_cand, cand.data(), (size_t)n * extra * 64);
  if (counts) memcpy(counts, c, sizeof(c));
  return 1;
}

// the finish body alone on arrays the caller made up: n lanes, flags n words, xof0 n * 16 words, xofs n * (nkeys - 1) * 16 words
extern "C" void hc_client_ring_finish(int issuance, uint32_t nkeys, uint32_t n, const uint8_t* pre, const uint8_t* resp, const uint32_t* flags,
                                      const uint32_t* xof0, const uint32_t* xofs, uint8_t* out_token, uint8_t* out_status, uint8_t* out_key) {
  ClientRingArgs r{};
  ClientArgs& a = r.c;
  a.n = n; a.label = issuance ? LABEL_RESPOND : LABEL_REFUND; a.pre = pre; a.resp = resp; a.flags = const_cast<uint32_t*>(flags); a.xof = xof0;
  a.out_token = out_token; a.status = out_status;
  r.nkeys = nkeys; r.xofs = const_cast<uint32_t*>(xofs); r.out_key = out_key;
  for (uint32_t p = 0; p < n; p++) client_ring_finish_lane(r, p);
}

// BLAKE3 of `msg` (at most one chunk) with the 32 bytes at byte offsets off_a and off_b replaced, by the ring's routine
extern "C" void hc_client_ring_patched_hash(const uint8_t* msg, uint32_t len, uint32_t off_a, const uint8_t* rep_a, uint32_t off_b, const uint8_t* rep_b, uint8_t* out) {
  std::vector<uint32_t> w((len + 3) / 4 + 1, 0u); if (len) memcpy(w.data(), msg, len);
  uint32_t ra[8], rb[8], o[16]; memcpy(ra, rep_a, 32); memcpy(rb, rep_b, 32);
  b3_chunk_xof64_patched2(o, w.data(), len, b3_patch_make(off_a, ra), b3_patch_make(off_b, rb));
  memcpy(out, o, 64);
}

// fe_mul + fe_sq of ONE chain_b<1> product s * pt (the yardstick of the counted-cost test); out = its encoding
extern "C" int hc_chain_b1_ops(const uint8_t* pt, const uint8_t* s, uint8_t* out, uint64_t* n_ops) {
  uint32_t w[8], r[8]; ld(w, pt); ge p; if (!ristretto_decode(p, w)) return 0;
  ge acc[1] = {ge_identity()}; sc sv[1] = {sc_in(s)};
  std::vector<uint32_t> bk(BUCKET_WORDS);
  fe_counts = fe_counts_t{0, 0, {0, 0, 0, 0}};
  chain_b<1>(acc, p, sv, bk.data());
  *n_ops = ops();
  ristretto_encode(r, acc[0]); st(out, r);
  return 1;
}

#if defined(CLIENT_RING_MAIN)
// Stand-alone replay of a case file written by tests/client_ring_cases.py write_case_file (little-endian u32 fields):
//   kind 1: L, issuance, nkeys, n, then h[96], ring_w, pre, req (issuance) or proofs, resp, expected status, out_key, tokens
//   kind 2: issuance, nkeys, n, then pre, resp, flags, xof0, xofs, expected status, out_key, tokens          kind 0: end
static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static bool rd_vec(FILE* f, std::vector<uint8_t>& v, size_t n) { v.assign(n + 1, 0); return rd(f, v.data(), n); }
int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s CASEFILE\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int cases = 0;
  for (;;) {
    uint32_t kind = 0;
    if (!rd(f, &kind, 4)) { fprintf(stderr, "truncated case file\n"); return 2; }
    if (kind == 0) break;
    std::vector<uint8_t> pre, req, proofs, resp, est, ekey, etok;
    if (kind == 1) {
      uint32_t hd[4]; uint8_t h[96];
      if (!rd(f, hd, 16) || !rd(f, h, 96)) return 2;
      const uint32_t L = hd[0], iss = hd[1], nkeys = hd[2], n = hd[3];
      std::vector<uint8_t> ring;
      const size_t pb = ProofLayout{(int)L}.bytes();
      if (!rd_vec(f, ring, 32 * nkeys) || !rd_vec(f, pre, (size_t)n * (iss ? 64 : 96)) || !rd_vec(f, iss ? req : proofs, (size_t)n * (iss ? 128 : pb)) ||
          !rd_vec(f, resp, (size_t)n * (iss ? 160 : 128)) || !rd_vec(f, est, n) || !rd_vec(f, ekey, n) || !rd_vec(f, etok, (size_t)n * 160)) return 2;
      std::vector<uint8_t> tok((size_t)n * 160), stt(n), okey(n), cand((size_t)n * 3 * 64);
      if (!hc_client_ring(h, (int)L, (int)iss, ring.data(), nkeys, n, pre.data(), req.data(), proofs.data(), resp.data(), tok.data(), stt.data(), okey.data(), cand.data(), nullptr)) {
        fprintf(stderr, "case %d: hc_client_ring refused its input\n", cases); return 1;
      }
      if (memcmp(stt.data(), est.data(), n) || memcmp(okey.data(), ekey.data(), n) || memcmp(tok.data(), etok.data(), (size_t)n * 160)) {
        fprintf(stderr, "case %d (L=%u issuance=%u nkeys=%u): outputs differ from the recorded oracle answers\n", cases, L, iss, nkeys); return 1;
      }
    } else if (kind == 2) {
      uint32_t hd[3];
      if (!rd(f, hd, 12)) return 2;
      const uint32_t iss = hd[0], nkeys = hd[1], n = hd[2], extra = nkeys - 1u;
      std::vector<uint8_t> fl, x0, xs;
      if (!rd_vec(f, pre, (size_t)n * (iss ? 64 : 96)) || !rd_vec(f, resp, (size_t)n * (iss ? 160 : 128)) || !rd_vec(f, fl, (size_t)n * 4) || !rd_vec(f, x0, (size_t)n * 64) ||
          !rd_vec(f, xs, (size_t)n * extra * 64) || !rd_vec(f, est, n) || !rd_vec(f, ekey, n) || !rd_vec(f, etok, (size_t)n * 160)) return 2;
      std::vector<uint32_t> flw(n + 1), x0w((size_t)n * 16 + 1), xsw((size_t)n * extra * 16 + 1);
      memcpy(flw.data(), fl.data(), (size_t)n * 4); memcpy(x0w.data(), x0.data(), (size_t)n * 64); memcpy(xsw.data(), xs.data(), (size_t)n * extra * 64);
      std::vector<uint8_t> tok((size_t)n * 160), stt(n), okey(n);
      hc_client_ring_finish((int)iss, nkeys, n, pre.data(), resp.data(), flw.data(), x0w.data(), xsw.data(), tok.data(), stt.data(), okey.data());
      if (memcmp(stt.data(), est.data(), n) || memcmp(okey.data(), ekey.data(), n) || memcmp(tok.data(), etok.data(), (size_t)n * 160)) {
        fprintf(stderr, "case %d (finish domain, issuance=%u nkeys=%u): outputs differ\n", cases, iss, nkeys); return 1;
      }
    } else { fprintf(stderr, "unknown case kind %u\n", kind); return 2; }
    cases++;
  }
  fclose(f);
  g_ring_tabs.clear();
  printf("CLIENT RING SANITIZERS CLEAN (%d cases)\n", cases);
  return 0;
}
#endif
