// bound_check.cpp — TEST-ONLY host build of the lane bodies with a request binding: the prover's and the ring verifier's
// bodies exactly as hostcheck.cpp / keyring_check.cpp run them, with SpendArgs::bind / ProveArgs::bind set (or null: the unbound
// call through the same code) and the transcripts, candidates and challenge hashes handed out.  This unit is keyring_check.cpp plus
// the binding; built by tests/bound_cases.py, never linked into libact_mi355x.so.
#include "keyring_check.cpp"

namespace {
void bound_params(DevParams& P, const uint8_t* h, int L) {
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
}  // namespace

extern "C" uint32_t hc_bound_transcript_bytes(int L, int bound) { return (uint32_t)SpendTranscript{L, bound}.bytes(); }
extern "C" uint32_t hc_bound_transcript_stride(int L, int bound) { return (uint32_t)SpendTranscript{L, bound}.stride(); }

// prove_spend for n tokens as the prover kernels run it (hc_prove_spend), under bind (n * 32 bytes, or null: unbound).
// out_transcripts: n pre-images of hc_bound_transcript_bytes(L, bind != null) bytes, back to back
extern "C" int hc_bound_prove(const uint8_t* h, int L, uint32_t n, const uint8_t* tok, const uint8_t* s_amount, const uint8_t* rng, const uint8_t* bind,
                              uint8_t* out_proofs, uint8_t* out_prerefund, uint8_t* out_status, uint8_t* out_transcripts) {
  if (L < 1 || L > 128 || !build_tables(h)) return 0;
  ProveArgs a{};
  bound_params(a.P, h, L);
  std::vector<uint32_t> half_h1((size_t)2 * NIELS_WORDS, 0u);
  {
    niels_store(half_h1.data(), ge_niels_identity());
    sc one = sc_zero(); one.v[0] = 1;
    ge hp = fixed_base_acc(ge_identity(), a.P.tab[BASE_H1], sc_half(one));
    fe zi = fe_invert(hp.Z); ge af; af.X = fe_mul(hp.X, zi); af.Y = fe_mul(hp.Y, zi); af.Z = fe_one(); af.T = fe_mul(af.X, af.Y);
    niels_store(half_h1.data() + NIELS_WORDS, niels_from_affine(af));
  }
  a.P.half_h1 = half_h1.data();
  const SpendTranscript st{L, bind != nullptr};
  std::vector<uint8_t> tr((size_t)n * st.stride(), 0), status(n, 0);
  std::vector<uint32_t> d3((size_t)n * 3 * GE_WORDS), half((size_t)n * (L < 2 ? 2 : L) * BUCKET_WORDS), state((size_t)n * 24, 0), flags(n, 0), xof((size_t)n * 16);
  a.n = n; a.tok = tok; a.s = s_amount; a.rng = rng; a.tr = tr.data(); a.tr_stride = (uint32_t)st.stride(); a.d3 = d3.data(); a.half = half.data();
  a.state = state.data(); a.flags = flags.data(); a.xof = xof.data(); a.proof = out_proofs; a.prerefund = out_prerefund; a.status = status.data();
  a.bind = bind;
  HostFb fb{a.P};
  for (uint32_t p = 0; p < n; p++) prove_head_lane(a, p, fb);
  for (uint32_t g = 0; g < n * (uint32_t)L; g++) prove_bits_lane(a, g, fb);
  for (uint64_t q0 = 0; q0 < (uint64_t)n * L * 3; q0 += PROVE_ENC_BATCH) prove_enc_lane(a, q0);
  for (uint32_t p = 0; p < n; p++) prove_tail_lane(a, p, fb);
  for (uint32_t p = 0; p < n; p++) b3_hash_xof64(&xof[(size_t)p * 16], reinterpret_cast<const uint32_t*>(tr.data() + (size_t)p * st.stride()), (uint32_t)st.bytes());
  for (uint32_t g = 0; g < n * (uint32_t)L; g++) prove_resp_lane(a, g);
  memcpy(out_status, status.data(), n);
  for (uint32_t p = 0; p < n; p++) memcpy(out_transcripts + (size_t)p * st.bytes(), tr.data() + (size_t)p * st.stride(), st.bytes());
  return 1;
}

// hc_ring_verify under bind (n * 32 bytes, or null: unbound).  out_transcripts: n pre-images as written under ring key 0, at stride
// hc_bound_transcript_stride (what act_host_hash_ring_many takes); out_cand: n * (nkeys - 1) candidates; out_xofs: n * nkeys * 64 bytes,
// the device-mode hashes (the full hash keeping chunk 0's siblings, then ring_hash_lane per extra key)
extern "C" int hc_bound_ring_verify(const uint8_t* h, int L, const uint8_t* keys, uint32_t nkeys, uint32_t n, const uint8_t* proofs, const uint8_t* bind,
                                    uint8_t* out_status, uint8_t* out_key, uint8_t* out_kprime, uint8_t* out_transcripts, uint8_t* out_cand, uint8_t* out_xofs) {
  if (L < 1 || L > 128 || nkeys < 1 || nkeys > (uint32_t)KEYRING_MAX || !build_tables(h)) return 0;
  RingArgs r{};
  SpendArgs& a = r.s;
  bound_params(a.P, h, L);
  std::vector<DevKey> ring(nkeys);
  for (uint32_t k = 0; k < nkeys; k++) {
    uint32_t w[8]; ld(w, keys + 64 * k); ring[k].x = sc_from_words(w);
    ld(w, keys + 64 * k + 32); if (!ristretto_decode(ring[k].w, w)) return 0;
  }
  a.K = ring[0];
  const SpendTranscript st{L, bind != nullptr};
  const uint32_t extra = nkeys - 1u;
  std::vector<uint8_t> tr((size_t)n * st.stride(), 0), status(n, 0), kp((size_t)n * 32, 0), cand((size_t)n * extra * 32 + 1, 0), okey(n, 0);
  std::vector<uint32_t> coords((size_t)n * L * NIELS_WORDS), d01((size_t)n * 2 * GE_WORDS), buckets((size_t)n * (L < PREP_BUCKET_SETS ? PREP_BUCKET_SETS : L) * BUCKET_WORDS),
      xa((size_t)n * GE_WORDS), flags(n, 0), naf((size_t)n * NAF_WORDS), dig((size_t)n * L * 8), sib((size_t)n * B3_MAX_SIBLINGS * 8, 0), xofs((size_t)n * nkeys * 16);
  a.proofs = proofs; a.n = n; a.tr = tr.data(); a.tr_stride = (uint32_t)st.stride(); a.coords = coords.data(); a.d01 = d01.data();
  a.buckets = buckets.data(); a.xa = xa.data(); a.flags = flags.data(); a.status = status.data(); a.kprime_enc = kp.data(); a.naf = naf.data(); a.dig = dig.data(); a.pbk = buckets.data();
  a.bind = bind;
  r.ring = ring.data(); r.nkeys = nkeys; r.cand = cand.data(); r.sib = sib.data(); r.xofs = xofs.data(); r.out_key = okey.data();
  for (uint32_t p = 0; p < n; p++) spend_prep_lane(a, p);
  for (uint32_t g = 0; g < n * (uint32_t)L; g++) { if (L % 64 == 0) spend_bits_lane<true>(a, g, nullptr); else spend_bits_lane<false>(a, g, nullptr); }
  for (uint64_t q0 = 0; q0 < (uint64_t)n * L * 2; q0 += ENC_BATCH) spend_enc_lane(a, q0);
  for (uint32_t p = 0; p < n; p++) spend_tail_lane(a, p);
  for (uint32_t p = 0; p < n; p++) {      // k_ring_hash_full's body
    const uint32_t* msg = reinterpret_cast<const uint32_t*>(tr.data() + (size_t)p * st.stride());
    b3_hash_xof64_sib(&xofs[(size_t)p * nkeys * 16], msg, (uint32_t)st.bytes(), [&](uint32_t ch, uint32_t* cv) { b3_chunk_cv(cv, msg, (uint32_t)st.bytes(), ch); },
                      [&](int l, const uint32_t* cv) { memcpy(&sib[((size_t)p * B3_MAX_SIBLINGS + l) * 8], cv, 32); });
  }
  for (uint32_t g = 0; g < n * extra; g++) ring_cand_lane(r, g);
  for (uint32_t g = 0; g < n * extra; g++) ring_hash_lane(r, g);
  for (uint32_t p = 0; p < n; p++) ring_finish_lane(r, p);
  memcpy(out_status, status.data(), n); memcpy(out_key, okey.data(), n); memcpy(out_kprime, kp.data(), (size_t)n * 32);
  memcpy(out_transcripts, tr.data(), tr.size());
  if (extra) memcpy(out_cand, cand.data(), (size_t)n * extra * 32);
  memcpy(out_xofs, xofs.data(), xofs.size() * 4);
  return 1;
}
