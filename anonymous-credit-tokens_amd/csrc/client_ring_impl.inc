// client_ring_impl.inc — included by engine.hip inside its extern "C" block, behind client_impl.inc: the client's side of key rotation.
//   act_issuance_to_credit_token_keyring_batch    PreIssuance::to_credit_token against a ring of issuer public keys
//   act_refund_to_credit_token_keyring_batch      PreRefund::to_credit_token against the same
//   act_refund_to_credit_token_return_keyring_batch   the same over RefundReturn records (DESIGN 4.10): phase A with t h1 in X_A, the
//                                                 candidates and hashes at the 160-byte stride, k_client_ring_return_finish behind them
// Neither message names the key it was signed with, and w enters the check only through X_g and Y_g (client_ring_lanes.h).  A ring
// call is therefore client_batch's schedule -- same chunks, same staging and wiping of the secret `pre` records, same host / device
// memory handling -- with phase A run ONCE under ring key 0 (fused = 0) and per chunk: the candidates X_g,k / Y_g,k of the other keys
// (k_client_ring_cand), their challenge hashes (k_client_ring_hash, in the kernel in both transcript modes) and the ring form of phase B
// (k_client_ring_finish).  In the host-transcript mode the two ring kernels run while the host hashes key 0's transcripts.
// There is NO tiny or fused road for rings: always the chunked launches, whatever n (as the server's ring calls).
//
// Side data, all of it public: per ring key k >= 1 a fixed-base table of w_k (1 MiB at CLIENT_RING_WBITS = 8), cached per ring position on
// the key's 32 bytes like w_cached and rebuilt when they change; per lane of a slot 192 B of candidate encodings, 192 B of XOF blocks
// and an index byte.  Allocated by a context's FIRST client-ring call and freed with it: a context that never makes one keeps its footprint.
struct ClientRingWs {
  uint8_t* d_cand[2] = {nullptr, nullptr};  uint32_t* d_xofs[2] = {nullptr, nullptr};  uint8_t* d_okey[2] = {nullptr, nullptr};
  uint32_t* d_tabw = nullptr;               // KEYRING_MAX - 1 tables, back to back
  uint32_t* d_ext = nullptr;                // a decoded base on its way to launch_build_table
  uint8_t tab_key[KEYRING_MAX - 1][32] = {}; bool tab_valid[KEYRING_MAX - 1] = {};
};

static void client_ring_ws_free(act_ctx* c) {
  ClientRingWs* w = c->client_ring_ws;
  if (!w) return;
  for (int s = 0; s < 2; s++) { void* dev[] = {w->d_cand[s], w->d_xofs[s], w->d_okey[s]}; for (void* p : dev) if (p) (void)hipFree(p); }
  if (w->d_tabw) (void)hipFree(w->d_tabw);
  if (w->d_ext) (void)hipFree(w->d_ext);
  delete w;
  c->client_ring_ws = nullptr;
}
static int client_ring_ws_alloc(act_ctx* c, ClientRingWs* w) {
  const size_t B = c->max_batch;
  for (int s = 0; s < 2; s++) {
    HIPCK(c, hipMalloc(&w->d_cand[s], B * (KEYRING_MAX - 1) * 64));
    HIPCK(c, hipMalloc(&w->d_xofs[s], B * (KEYRING_MAX - 1) * 64));
    HIPCK(c, hipMalloc(&w->d_okey[s], B));
  }
  HIPCK(c, hipMalloc(&w->d_tabw, (KEYRING_MAX - 1) * fb_table_words(CLIENT_RING_WBITS) * 4));
  HIPCK(c, hipMalloc(&w->d_ext, GE_WORDS * 4));
  return ACT_OK;
}
static int client_ring_ws_get(act_ctx* c) {
  if (c->client_ring_ws) return ACT_OK;
  // the set becomes the context's only when it is COMPLETE: after a failed allocation the next call allocates again instead of
  // launching kernels on null buffers
  ClientRingWs* w = c->client_ring_ws = new ClientRingWs();
  const int rc = client_ring_ws_alloc(c, w);
  if (rc) client_ring_ws_free(c);
  return rc;
}
// Checks the whole ring on the host BEFORE anything is launched (nothing of a rejected ring replaces what is cached), makes ring key 0 the
// context's cached public key and builds the tables of the entries whose bytes changed.
static int client_ring_set(act_ctx* c, const uint8_t* ring_w, uint32_t nkeys) {
  ge pts[KEYRING_MAX];
  for (uint32_t k = 0; k < nkeys; k++) {
    uint32_t w[8]; memcpy(w, ring_w + 32 * k, 32);
    if (!ristretto_decode(pts[k], w)) { c->err = "client key ring: an entry is not a canonical Ristretto encoding"; return ACT_ERR_ARG; }
  }
  int rc = set_pubkey(c, ring_w); if (rc) return rc;
  if ((rc = client_ring_ws_get(c))) return rc;
  ClientRingWs* ws = c->client_ring_ws;
  Slot& s0 = c->slots[0];
  for (uint32_t k = 1; k < nkeys; k++) {
    if (ws->tab_valid[k - 1] && memcmp(ws->tab_key[k - 1], ring_w + 32 * k, 32) == 0) continue;
    ws->tab_valid[k - 1] = false;
    uint32_t ext[GE_WORDS]; ge_store(ext, pts[k]);
    HIPCK(c, hipMemcpyAsync(ws->d_ext, ext, sizeof(ext), hipMemcpyHostToDevice, s0.stream));
    launch_build_table(ws->d_ext, ws->d_tabw + (size_t)(k - 1) * fb_table_words(CLIENT_RING_WBITS), CLIENT_RING_WBITS, s0.stream);
    HIPCK(c, hipStreamSynchronize(s0.stream));      // `ext` is a stack buffer, d_ext is reused, and the other slot's stream reads the table too
    memcpy(ws->tab_key[k - 1], ring_w + 32 * k, 32); ws->tab_valid[k - 1] = true;
  }
  return ACT_OK;
}

static int client_ring_batch(act_ctx* c, size_t n, int mem, int label, const uint8_t* pre, const uint8_t* ring_w, uint32_t nkeys, const uint8_t* req,
                             const uint8_t* resp, const uint8_t* proofs, uint8_t* out_token, uint8_t* status, uint8_t* out_key, bool with_t = false) {
  Call call(c, n);
  HIPCK(c, hipSetDevice(c->device));
  int rc = client_ring_set(c, ring_w, nkeys); if (rc) return rc;
  ClientRingWs* ws = c->client_ring_ws;
  const bool issuance = label == LABEL_RESPOND;
  const uint32_t extra = nkeys - 1u;
  const size_t pre_b = issuance ? 64 : 96, resp_b = client_ring_resp_stride(label, with_t), pb = ProofLayout{c->L}.bytes();
  // client_batch's chunk schedule: host-memory refund calls in quarters that alternate between the two slots, everything else on one slot
  size_t chunk = std::min(c->max_batch, std::max<size_t>(16384, (n / 4 + 1023) / 1024 * 1024));
  const bool taper_off = tune(T_NO_TAPER) != 0;
  const uint8_t* proofs_view = (!issuance && mem == ACT_MEM_HOST) ? mapped_view(c, proofs, n * pb) : nullptr;
  const bool two_slots = mem == ACT_MEM_HOST && !issuance && !proofs_view && c->depth > 1 && n > chunk && !taper_off;
  if (!two_slots) chunk = c->max_batch;
  const uint32_t len = client_ring_tr_len(c->P, label);
  size_t k = 0;
  for (size_t off = 0; off < n; off += chunk, k++) {
    const size_t s = two_slots ? (k & 1) : 0;
    Slot& sl = c->slots[s];
    if (two_slots) HIPCK(c, hipStreamSynchronize(sl.stream));      // the chunk before last has left this slot's staging areas
    uint32_t m = (uint32_t)std::min(chunk, n - off);
    sl.d_trs_dirty = std::max(sl.d_trs_dirty, (size_t)m);
    ClientRingArgs r{}; r.tabw = ws->d_tabw; r.nkeys = nkeys; r.cand = ws->d_cand[s]; r.xofs = ws->d_xofs[s]; r.out_key = ws->d_okey[s];
    ClientArgs& a = r.c;
    a.P = c->P; a.w = c->w_pub; a.n = m; a.label = label; a.coords = sl.d_coords; a.trs = sl.d_trs; a.flags = sl.d_flags; a.pbk = sl.d_buckets;
    a.xof = sl.d_xof; a.status = sl.d_status; a.with_t = with_t ? 1 : 0;
    if (two_slots && (rc = copy_chain_wait(c, sl, false))) return rc;
    if ((rc = dev_in(c, sl, 0, mem, pre + off * pre_b, (size_t)m * pre_b, &a.pre))) return rc;
    if ((rc = dev_in(c, sl, 1, mem, resp + off * resp_b, (size_t)m * resp_b, &a.resp))) return rc;
    if (issuance) { if ((rc = dev_in(c, sl, 3, mem, req + off * 128, (size_t)m * 128, &a.req))) return rc; }
    else if (proofs_view) a.proofs = proofs_view + off * pb;
    else { if ((rc = dev_in(c, sl, 3, mem, proofs + off * pb, (size_t)m * pb, &a.proofs))) return rc; }
    if (two_slots && (rc = copy_chain_record(c, sl, false))) return rc;
    if ((rc = dev_out_begin(c, sl, 2, mem, out_token + off * 160, (size_t)m * 160, &a.out_token))) return rc;
    HIPCK(c, hipMemsetAsync(sl.d_flags, 0, (size_t)m * 4, sl.stream));      // the kernels OR their flags in
    if (!issuance) {
      if ((rc = prof_launch(c, sl, PK_CLIENT, (uint64_t)m * c->L, [&] { launch_client_decode_com(a, sl.stream); }))) return rc;
    }
    a.group_counter = group_counters(c, sl);
    a.fused = 0;
    if ((rc = prof_launch(c, sl, PK_CLIENT, m, [&] { launch_client_a(a, sl.stream); }))) return rc;      // phase A under ring key 0
    if ((rc = hash_begin(c, sl, PK_HASH_SMALL, sl.d_trs, SMALL_TR_STRIDE, len, m))) return rc;
    if (extra) {
      if ((rc = prof_launch(c, sl, PK_CLIENT, (uint64_t)m * extra, [&] { launch_client_ring_cand(r, sl.stream); }))) return rc;
      if ((rc = prof_launch(c, sl, PK_CLIENT, (uint64_t)m * extra, [&] { launch_client_ring_hash(r, sl.stream); }))) return rc;
    }
    if ((rc = hash_end(c, sl, SMALL_TR_STRIDE, len, m))) return rc;
    if ((rc = prof_launch(c, sl, PK_CLIENT, m, [&] { if (with_t) launch_client_ring_return_finish(r, sl.stream); else launch_client_ring_finish(r, sl.stream); }))) return rc;
    if ((rc = dev_out_end(c, sl, mem, out_token + off * 160, a.out_token, (size_t)m * 160))) return rc;
    HIPCK(c, hipMemcpyAsync(out_key + off, ws->d_okey[s], m, mem == ACT_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, sl.stream));
    if ((rc = copy_status_out(c, sl, mem, status + off, m))) return rc;
    if (!two_slots && (rc = sync_all(c))) return rc;
  }
  return call.finish();      // waits for both streams
}
int act_issuance_to_credit_token_keyring_batch(act_ctx* c, size_t n, int mem, const uint8_t* pre, const uint8_t* ring_w, uint32_t nkeys,
                                               const uint8_t* req, const uint8_t* resp, uint8_t* out_token, uint8_t* status, uint8_t* out_key) {
  if (!c || !ring_w || nkeys < 1 || nkeys > ACT_KEYRING_MAX || (n && (!pre || !req || !resp || !out_token || !status || !out_key))) return ACT_ERR_ARG;
  return client_ring_batch(c, n, mem, LABEL_RESPOND, pre, ring_w, nkeys, req, resp, nullptr, out_token, status, out_key);
}
int act_refund_to_credit_token_keyring_batch(act_ctx* c, size_t n, int mem, const uint8_t* prerefund, const uint8_t* proof, const uint8_t* refund,
                                             const uint8_t* ring_w, uint32_t nkeys, uint8_t* out_token, uint8_t* status, uint8_t* out_key) {
  if (!c || !ring_w || nkeys < 1 || nkeys > ACT_KEYRING_MAX || (n && (!prerefund || !proof || !refund || !out_token || !status || !out_key))) return ACT_ERR_ARG;
  return client_ring_batch(c, n, mem, LABEL_REFUND, prerefund, ring_w, nkeys, nullptr, refund, proof, out_token, status, out_key);
}
// PreRefund::to_credit_token over RefundReturn records against a ring (client_ring_return_lanes.h): X_A = g + K' + t h1 does not depend
// on the key, so the per-extra-key work is that of the call above; status 8 only for a t > s that some ring key validly signed
int act_refund_to_credit_token_return_keyring_batch(act_ctx* c, size_t n, int mem, const uint8_t* prerefund, const uint8_t* proof, const uint8_t* refund_return,
                                                    const uint8_t* ring_w, uint32_t nkeys, uint8_t* out_token, uint8_t* status, uint8_t* out_key) {
  if (!c || !ring_w || nkeys < 1 || nkeys > ACT_KEYRING_MAX || (n && (!prerefund || !proof || !refund_return || !out_token || !status || !out_key))) return ACT_ERR_ARG;
  return client_ring_batch(c, n, mem, LABEL_REFUND, prerefund, ring_w, nkeys, nullptr, refund_return, proof, out_token, status, out_key, true);
}
