// return_ring_check.cpp — TEST-ONLY host build of the ring form of the client's RefundReturn check (csrc/client_ring_return_lanes.h),
// on top of everything return_check.cpp and client_ring_check.cpp offer (tables, transcript prefixes, the client's decode pass, phase A
// with t h1 in X_A, the ring tables).  Built by tests/return_ring_cases.py as a shared object for tests/test_return_ring_host.py and,
// with -DRETURN_RING_MAIN, as a stand-alone program that replays a case file under the sanitizers; never linked into libact_mi355x.so.
//
// What runs here are the REAL lane bodies: client_ring_cand_lane and client_ring_hash_lane over 160-byte records (ClientArgs::with_t
// picks the stride) and client_ring_return_finish_lane.  Phase A is restated (host_client_a_return, return_check.cpp).  The kernels
// themselves are judged on the GPU (tests/test_gpu_return_ring.py).
#include "return_check.cpp"
#include "../../anonymous-credit-tokens_amd/csrc/client_ring_return_lanes.h"

// One ring call over n RefundReturn records, lane by lane, in the order the engine launches the kernels: decode_com, phase A under ring
// key 0 with return_xa, BLAKE3 of key 0's transcripts, candidates, their patched hashes, the return finish.  pre n*96, proofs, resp n*160.
//   counts[0] = fe_mul + fe_sq of the one-key body (decode_com + phase A)     counts[1] = of everything the ring adds
//   counts[2], [3] = fixed_base_acc calls on g / on the ring tables in the ring's part     counts[4] = this build's window count of g
// (counts[3] is the counter of table id CLIENT_RING_TAB_ID, which h1 shares: it equals nkeys - 1 only if the ring's part has NO product
// on h1 -- t h1 belongs to phase A)
extern "C" int hc_return_ring(const uint8_t* h, int L, const uint8_t* ring_w, uint32_t nkeys, uint32_t n, const uint8_t* pre, const uint8_t* proofs,
                              const uint8_t* resp, uint8_t* out_token, uint8_t* out_status, uint8_t* out_key, uint64_t* counts) {
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
  std::vector<uint8_t> trs((size_t)n * SMALL_TR_STRIDE + 64, 0), cand((size_t)n * (extra ? extra : 1u) * 64, 0);
  a.n = n; a.label = LABEL_REFUND; a.pre = pre; a.resp = resp; a.proofs = proofs; a.with_t = 1;
  a.coords = coords.data(); a.trs = trs.data(); a.flags = flags.data(); a.xof = xof.data(); a.out_token = out_token; a.status = out_status; a.pbk = pbk.data();
  r.tabw = tabw.data(); r.nkeys = nkeys; r.cand = cand.data(); r.xofs = xofs.data(); r.out_key = out_key;
  fe_counts = fe_counts_t{0, 0, {0, 0, 0, 0}};
  for (uint32_t p = 0; p < n; p++) for (uint32_t j = 0; j < (uint32_t)L; j++) host_client_decode_com(a, p, j);
  for (uint32_t p = 0; p < n; p++) host_client_a_return(a, p);
  uint64_t c[5] = {ops(), 0, 0, 0, (uint64_t)FB_WINDOWS};
  for (uint32_t p = 0; p < n; p++)
    b3_hash_xof64(&xof[(size_t)p * 16], reinterpret_cast<const uint32_t*>(trs.data() + (size_t)p * SMALL_TR_STRIDE), client_ring_tr_len(a.P, a.label));
  fe_counts = fe_counts_t{0, 0, {0, 0, 0, 0}};
  for (uint32_t g = 0; g < n * extra; g++) client_ring_cand_lane(r, g);
  for (uint32_t g = 0; g < n * extra; g++) client_ring_hash_lane(r, g);
  for (uint32_t p = 0; p < n; p++) client_ring_return_finish_lane(r, p);
  c[1] = ops(); c[2] = fe_counts.fixed_base[BASE_G]; c[3] = fe_counts.fixed_base[CLIENT_RING_TAB_ID];
  if (counts) memcpy(counts, c, sizeof(c));
  return 1;
}

// the record stride the ring lanes use, as the one function that decides it
extern "C" uint32_t hc_client_ring_resp_stride(int issuance, int with_t) { return client_ring_resp_stride(issuance ? LABEL_RESPOND : LABEL_REFUND, with_t); }

#if defined(RETURN_RING_MAIN)
// Stand-alone replay of a case file written by tests/return_ring_cases.py write_case_file (little-endian u32 fields):
//   kind 1: L, nkeys, n, then h[96], ring_w, pre, proofs, resp (n * 160), expected status, out_key, tokens          kind 0: end
static bool rr_rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static bool rr_vec(FILE* f, std::vector<uint8_t>& v, size_t n) { v.assign(n, 0); return rr_rd(f, v.data(), n); }      // exact sizes: a read past a record is the sanitizer's to find
int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s CASEFILE\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int cases = 0;
  for (;;) {
    uint32_t kind = 0;
    if (!rr_rd(f, &kind, 4)) { fprintf(stderr, "truncated case file\n"); return 2; }
    if (kind == 0) break;
    if (kind != 1) { fprintf(stderr, "unknown case kind %u\n", kind); return 2; }
    uint32_t hd[3]; uint8_t h[96];
    if (!rr_rd(f, hd, 12) || !rr_rd(f, h, 96)) return 2;
    const uint32_t L = hd[0], nkeys = hd[1], n = hd[2];
    if (L < 1 || L > 128 || nkeys < 1 || nkeys > (uint32_t)KEYRING_MAX) return 2;
    const size_t pb = ProofLayout{(int)L}.bytes();
    std::vector<uint8_t> ring, pre, proofs, resp, est, ekey, etok;
    if (!rr_vec(f, ring, 32 * nkeys) || !rr_vec(f, pre, (size_t)n * 96) || !rr_vec(f, proofs, (size_t)n * pb) || !rr_vec(f, resp, (size_t)n * 160) ||
        !rr_vec(f, est, n) || !rr_vec(f, ekey, n) || !rr_vec(f, etok, (size_t)n * 160)) return 2;
    std::vector<uint8_t> tok((size_t)n * 160), stt(n), okey(n);
    if (!hc_return_ring(h, (int)L, ring.data(), nkeys, n, pre.data(), proofs.data(), resp.data(), tok.data(), stt.data(), okey.data(), nullptr)) {
      fprintf(stderr, "case %d: hc_return_ring refused its input\n", cases); return 1;
    }
    if (memcmp(stt.data(), est.data(), n) || memcmp(okey.data(), ekey.data(), n) || memcmp(tok.data(), etok.data(), (size_t)n * 160)) {
      fprintf(stderr, "case %d (L=%u nkeys=%u): outputs differ from the model's answers\n", cases, L, nkeys); return 1;
    }
    cases++;
  }
  fclose(f);
  g_ring_tabs.clear();
  printf("RETURN RING SANITIZERS CLEAN (%d cases)\n", cases);
  return 0;
}
#endif
