// return_check.cpp — TEST-ONLY host build of what partial refunds add to the lane bodies (csrc/return_lanes.h, and the screen of
// csrc/admit_lanes.h with its `returned` array), on top of everything hostcheck.cpp and client_ring_check.cpp offer (tables, transcript
// prefixes, the client's decode pass).  Built by tests/refund_return_cases.py as a shared object for tests/test_refund_return_host.py
// and, with -DRETURN_MAIN, as a stand-alone program for the sanitizers; never linked into libact_mi355x.so.
//
// The signing phases and the client's phase A are __global__ kernels (k_sign.hip, k_client.hip) with no host-compilable lane body: the
// functions below restate them statement by statement AROUND the real bodies -- return_exceeds, return_xa, return_client_finish,
// admit_decide_return, admit_screen_lane -- so that those are judged by the model.  The kernels themselves are judged on the GPU
// (tests/test_gpu_refund_return.py).
#include "client_ring_check.cpp"
#include "../../anonymous-credit-tokens_amd/csrc/admit_lanes.h"
#include "../../anonymous-credit-tokens_amd/csrc/return_lanes.h"

namespace {

// k_client_a for a RefundReturn lane (with_t): host_client_a of client_ring_check.cpp with the one statement the feature adds
void host_client_a_return(const ClientArgs& a, uint32_t p) {
  const int L = a.P.L;
  const uint8_t* resp = a.resp + (size_t)p * 160;
  uint32_t flags = a.flags[p];
  uint32_t wa[8]; load8(wa, resp);
  ge A; if (!ristretto_decode(A, wa)) flags |= FLAG_UNDECODABLE;
  sc e = load_sc(resp + 32), gamma = load_sc(resp + 64), z = load_sc(resp + 96);
  ge kp = ge_identity();
  for (int j = L - 1; j >= 0; j--) { kp = ge_double(kp); kp = ge_madd(kp, niels_load(a.coords + ((size_t)p * L + j) * NIELS_WORDS)); }
  ge xa = ge_add(kp, ge_basepoint());
  xa = return_xa(a.P, xa, load_sc(resp + 128));
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
  tr_put_bytes(el, e.v); el += 40;
  uint32_t enc[8];
  tr_put_bytes(el, wa); el += 40;
  ristretto_encode(enc, xa); tr_put_bytes(el, enc); el += 40;
  ristretto_encode(enc, xg); tr_put_bytes(el, enc); el += 40;
  ristretto_encode(enc, acc[0]); tr_put_bytes(el, enc); el += 40;
  ristretto_encode(enc, yg[0]); tr_put_bytes(el, enc);
  a.flags[p] = flags;
}

}  // namespace

extern "C" {

// t > s on two 32-byte little-endian values, each reduced mod l first (return_lanes.h)
int hc_return_exceeds(const uint8_t* t, const uint8_t* s) { return return_exceeds_bytes(t, s) ? 1 : 0; }

int hc_return_decide(int wire_code, int charge_given, int charge_equal, int return_given, int return_fits, int found, int* probed) {
  *probed = 0;
  return admit_decide_return((uint8_t)wire_code, charge_given != 0, charge_equal != 0, return_given != 0, return_fits != 0, [&]() { *probed = 1; return found != 0; });
}

// the screen with the returned amounts: hc_admit_screen of admit_check.cpp plus `returned` (nullable)
void hc_return_screen(uint32_t n, uint32_t stride, const uint8_t* ks, const uint8_t* charge, const uint8_t* returned, const uint8_t* wire_code,
                      const uint32_t* tab_keys, const uint32_t* tab_state, uint32_t tab_cap, const uint8_t salt[16], uint8_t* pre, uint8_t* kred) {
  AdmitScreenArgs a{};
  a.n = n; a.stride = stride; a.ks = ks; a.charge = charge; a.returned = returned; a.wire_code = wire_code; a.tab_keys = tab_keys; a.tab_state = tab_state;
  a.tab_cap = tab_cap; memcpy(a.salt.w, salt, 16); a.pre = pre; a.kred = kred;
  for (uint32_t i = 0; i < ((n + 255) / 256) * 256; i++) admit_screen_lane(a, i);      // the grid's tail lanes too
}

// One RefundReturn signature from enc(K'), t and the two nonces (reduced scalars), as k_sign_xa -> k_sign_a_ring -> BLAKE3 -> k_sign_b_ring
// compute it: X_A = return_xa(g + K', t), A = (e + x)^-1 X_A, the "refund" transcript, z.  out: 160 bytes.
//   counts[0], [1] = fe_mul, fe_sq of return_xa alone (what the feature adds per signed lane)    counts[2] = its fixed-base products on h1
//   counts[3] = this build's window count
int hc_return_sign(const uint8_t* h, const uint8_t* sk, const uint8_t* kprime, const uint8_t* t, const uint8_t* e_in, const uint8_t* alpha_in, uint8_t* out,
                   uint64_t* counts) {
  if (!build_tables(h)) return 0;
  DevParams P; fill_params(P, h, 8);
  uint32_t w[8]; ld(w, kprime);
  ge K; if (!ristretto_decode(K, w)) return 0;
  ld(w, sk + 32);
  ge W; if (!ristretto_decode(W, w)) return 0;
  const sc x = sc_in(sk), e = sc_in(e_in), alpha = sc_in(alpha_in), tv = load_sc(t);
  ge xa = ge_add(K, ge_basepoint());
  fe_counts = fe_counts_t{0, 0, {0, 0, 0, 0}};
  xa = return_xa(P, xa, tv);
  if (counts) { counts[0] = fe_counts.mul; counts[1] = fe_counts.sq; counts[2] = fe_counts.fixed_base[BASE_H1]; counts[3] = (uint64_t)FB_WINDOWS; }
  const sc inv = sc_invert(sc_add(e, x));
  std::vector<uint32_t> bk(2 * BUCKET_WORDS);
  ge a1[1] = {ge_identity()}; sc s1[1] = {inv}; chain_b<1>(a1, xa, s1, bk.data());                       // A
  ge a2[1] = {ge_identity()}; sc s2[1] = {sc_mul(alpha, inv)}; chain_b<1>(a2, xa, s2, bk.data());        // Y_A = alpha A
  const ge xg = ge_add(fixed_base_acc(ge_identity(), P.tab[BASE_G], e), W);
  const ge yg = fixed_base_acc(ge_identity(), P.tab[BASE_G], alpha);
  std::vector<uint8_t> tr(SMALL_TR_STRIDE + 64, 0);
  tr_put_prefix(tr.data(), P, LABEL_REFUND);
  uint8_t* el = tr.data() + P.prefix_len[LABEL_REFUND];
  uint32_t enc[8], enc_a[8];
  tr_put_bytes(el, e.v); el += 40;
  ristretto_encode(enc_a, a1[0]); tr_put_bytes(el, enc_a); el += 40;
  ristretto_encode(enc, xa); tr_put_bytes(el, enc); el += 40;
  ristretto_encode(enc, xg); tr_put_bytes(el, enc); el += 40;
  ristretto_encode(enc, a2[0]); tr_put_bytes(el, enc); el += 40;
  ristretto_encode(enc, yg); tr_put_bytes(el, enc);
  uint32_t xof[16];
  b3_hash_xof64(xof, reinterpret_cast<const uint32_t*>(tr.data()), P.prefix_len[LABEL_REFUND] + 40u * 6u);
  const sc gamma = sc_from_wide_words(xof);
  const sc z = sc_muladd(gamma, sc_add(x, e), alpha);
  store8(out, enc_a); store_sc(out + 32, e); store_sc(out + 64, gamma); store_sc(out + 96, z); store_sc(out + 128, tv);
  return 1;
}

// The client's call over n RefundReturn records, lane by lane, in the order the engine launches the kernels: decode_com, phase A with
// return_xa, BLAKE3, return_client_finish.  pre n*96, proofs, resp n*160; out_token n*160, out_status n.
int hc_return_client(const uint8_t* h, int L, const uint8_t* w_enc, uint32_t n, const uint8_t* pre, const uint8_t* proofs, const uint8_t* resp,
                     uint8_t* out_token, uint8_t* out_status) {
  if (L < 1 || L > 128 || !build_tables(h)) return 0;
  ClientArgs a{};
  fill_params(a.P, h, L);
  { uint32_t w[8]; ld(w, w_enc); if (!ristretto_decode(a.w, w)) return 0; }
  std::vector<uint32_t> coords((size_t)n * L * NIELS_WORDS), flags(n, 0u), xof((size_t)n * 16), pbk((size_t)n * PREP_BUCKET_SETS * BUCKET_WORDS);
  std::vector<uint8_t> trs((size_t)n * SMALL_TR_STRIDE + 64, 0);
  a.n = n; a.label = LABEL_REFUND; a.pre = pre; a.resp = resp; a.proofs = proofs; a.with_t = 1;
  a.coords = coords.data(); a.trs = trs.data(); a.flags = flags.data(); a.xof = xof.data(); a.out_token = out_token; a.status = out_status; a.pbk = pbk.data();
  for (uint32_t p = 0; p < n; p++) for (uint32_t j = 0; j < (uint32_t)L; j++) host_client_decode_com(a, p, j);
  for (uint32_t p = 0; p < n; p++) host_client_a_return(a, p);
  for (uint32_t p = 0; p < n; p++) {
    b3_hash_xof64(&xof[(size_t)p * 16], reinterpret_cast<const uint32_t*>(trs.data() + (size_t)p * SMALL_TR_STRIDE), client_ring_tr_len(a.P, a.label));
    return_client_finish(a, p, &xof[(size_t)p * 16]);
  }
  return 1;
}

}  // extern "C"

#if defined(RETURN_MAIN)
// Stand-alone run for the sanitizers: the compare on its edge cases, the decision table, and sign -> client round trips through the
// bodies above under made-up Params (three points of the form i * g) for t = 0, 1, s and s + 1, each also with t altered after signing.
int main() {
  uint8_t s[32] = {0}, t[32] = {0};
  s[0] = 5; t[0] = 5;
  if (hc_return_exceeds(t, s)) return 1;
  t[0] = 6; if (!hc_return_exceeds(t, s)) return 1;
  t[0] = 5; t[20] = 1; if (!hc_return_exceeds(t, s)) return 1;
  int probed = 0;
  if (hc_return_decide(0, 1, 1, 1, 0, 1, &probed) != RETURN_TOO_BIG || probed) return 1;
  if (hc_return_decide(0, 1, 0, 1, 0, 1, &probed) != ADMIT_WRONG_CHARGE || probed) return 1;
  // made-up Params and key: h_b = (7 + b) g, x = 11, w = x g; the "proof" is a zero record of L = 1 whose Com_0 = 5 g and s = 5
  auto mul_g = [](uint8_t v, uint8_t* out32) {
    uint32_t r[8], gw[8]; uint8_t sv[32] = {0}; sv[0] = v;
    ld(gw, kGen); ge g; if (!ristretto_decode(g, gw)) return false;
    ge acc[1] = {ge_identity()}; sc one[1] = {sc_in(sv)}; std::vector<uint32_t> bk(BUCKET_WORDS);
    chain_b<1>(acc, g, one, bk.data());
    ristretto_encode(r, acc[0]); st(out32, r);
    return true;
  };
  uint8_t h[96], sk[64] = {0}, com[32];
  for (int b = 0; b < 3; b++) if (!mul_g((uint8_t)(7 + b), h + 32 * b)) return 1;
  sk[0] = 11; if (!mul_g(11, sk + 32) || !mul_g(5, com)) return 1;
  const ProofLayout pl{1};
  std::vector<uint8_t> proof(pl.bytes(), 0), pre(96, 0);
  proof[32] = 5; memcpy(proof.data() + 32 * pl.com(0), com, 32);
  pre[0] = 1; pre[32] = 2; pre[64] = 9;                             // r | k | m
  uint8_t e[32] = {0}, alpha[32] = {0}; e[0] = 3; e[9] = 0x55; alpha[0] = 4; alpha[17] = 0x77;
  const uint8_t want_status[4] = {0, 0, 0, 8};                       // t = 0, 1, s, s + 1 (validly signed, then refused by the client)
  const uint8_t ts[4] = {0, 1, 5, 6};
  for (int c = 0; c < 4; c++) {
    uint8_t tt[32] = {0}, rec[160], tok[160], stt = 99; uint64_t counts[4];
    tt[0] = ts[c];
    if (!hc_return_sign(h, sk, com, tt, e, alpha, rec, counts)) return 1;
    if (!hc_return_client(h, 1, sk + 32, 1, pre.data(), proof.data(), rec, tok, &stt)) return 1;
    if (stt != want_status[c]) { fprintf(stderr, "t = %d: status %d, expected %d\n", ts[c], stt, want_status[c]); return 1; }
    if (stt == 0 && tok[128] != 9 + ts[c]) { fprintf(stderr, "t = %d: balance %d\n", ts[c], tok[128]); return 1; }
    rec[128] ^= 1;                                                  // t altered after signing: the proof fails
    if (!hc_return_client(h, 1, sk + 32, 1, pre.data(), proof.data(), rec, tok, &stt) || stt != 4) { fprintf(stderr, "t = %d altered: status %d\n", ts[c], stt); return 1; }
  }
  g_ring_tabs.clear();
  printf("RETURN SANITIZERS CLEAN\n");
  return 0;
}
#endif
