// client_impl.inc -- the client's side of the path behind the C ABI (included by engine.hip, inside its extern "C" block):
//   act_prove_spend_batch / _seeded_batch            CreditToken::prove_spend        /root/reference/src/lib.rs:972-1152
//   act_issuance_to_credit_token_batch               PreIssuance::to_credit_token    src/lib.rs:528-562
//   act_refund_to_credit_token_batch                 PreRefund::to_credit_token      src/lib.rs:1217-1253
// and the copy chaining both use for host-memory callers.
// rng: the caller's bytes, or (seed != nullptr) expanded on the device from a 32-byte seed: lane i draws from the BLAKE3 XOF of
// seed | u64_le(first_lane + i) (k_misc.hip k_xof_expand) -- 33 536 bytes per proof that then never cross PCIe
static int prove_spend_impl(act_ctx* c, size_t n, int mem, const uint8_t* token, const uint8_t* s, const uint8_t* rng, const uint8_t* seed,
                            uint64_t first_lane, uint8_t* out_proof, uint8_t* out_prerefund, uint8_t* status, const uint8_t* bind = nullptr) {
  Call call(c, n);
  HIPCK(c, hipSetDevice(c->device));
  const size_t pb = ProofLayout{c->L}.bytes(), rb = act_prove_rng_bytes(c);
  // bind (DESIGN 4.12, request binding): n * 32 bytes in `mem` memory or null; the head kernel writes a lane's bytes as its transcript's
  // last element and the hash takes the bound length
  const SpendTranscript st{c->L, bind != nullptr};
  // Chunk schedule: full-size chunks; a host-memory caller's LAST chunk is cut in two (11/16 + 5/16) -- its 16.8 KB per proof leave
  // after everything is computed (19 ms of a 76 ms call over 65 536 proofs), and the first part's copy out fits under the second
  // part's kernels (a proof takes ~0.3 us to leave, ~0.9 us to make)
  std::vector<std::pair<size_t, size_t>> sched;          // (offset, lanes)
  for (size_t off = 0; off < n; off += c->max_batch) sched.emplace_back(off, std::min(c->max_batch, n - off));
  const bool taper_off = tune(T_NO_TAPER) != 0;
  if (mem == ACT_MEM_HOST && !sched.empty() && sched.back().second >= 8192 && !taper_off) {
    const size_t off = sched.back().first, l = sched.back().second, t = (l * 5 / 16 + 1023) / 1024 * 1024;
    sched.back() = {off, l - t}; sched.emplace_back(off + l - t, t);
  }
  const size_t nchunks = sched.size();
  ProveArgs args[2]; uint32_t ms[2] = {0, 0}; size_t offs[2] = {0, 0};
  // two-slot pipeline like spend_batch: head/bits/tail + hash start of chunk i+1 are enqueued before chunk i is finished
  const size_t depth = (size_t)c->depth;
  auto stage1 = [&](size_t i) -> int {
    Slot& sl = c->slots[i % depth]; ProveArgs& a = args[i % depth];
    size_t off = sched[i].first; uint32_t m = (uint32_t)sched[i].second;
    ms[i % depth] = m; offs[i % depth] = off;
    a = ProveArgs{}; a.P = c->P; a.n = m; a.tr = sl.d_tr; a.tr_stride = (uint32_t)st.stride(); a.d3 = sl.d_d01; a.half = sl.d_buckets; a.state = sl.d_state;
    a.flags = sl.d_flags; a.xof = sl.d_xof; a.status = sl.d_status; a.group_counter = group_counters(c, sl);
    int rc;
    if ((rc = dev_in(c, sl, 0, mem, token + off * 160, (size_t)m * 160, &a.tok))) return rc;
    if ((rc = dev_in(c, sl, 1, mem, s + off * 32, (size_t)m * 32, &a.s))) return rc;
    if (bind && (rc = dev_in(c, sl, 5, mem, bind + off * 32, (size_t)m * 32, &a.bind))) return rc;
    if (!seed) { if ((rc = dev_in(c, sl, 3, mem, rng + off * rb, (size_t)m * rb, &a.rng))) return rc; }
    else {
      // 48 bytes past the lanes' bytes hold the seed (read by the expansion kernel on this stream)
      if ((rc = stage_reserve(c, sl, 3, (size_t)m * rb + 48))) return rc;
      uint8_t* d_seed = sl.d_stage[3] + (size_t)m * rb;
      HIPCK(c, hipMemcpyAsync(d_seed, seed, 32, hipMemcpyHostToDevice, sl.stream));
      launch_xof_expand(reinterpret_cast<const uint32_t*>(d_seed), first_lane + off, m, (uint32_t)(rb / 64), sl.d_stage[3], sl.stream);
      a.rng = sl.d_stage[3];
    }
    if ((rc = dev_out_begin(c, sl, 2, mem, out_proof + off * pb, (size_t)m * pb, &a.proof))) return rc;
    if ((rc = dev_out_begin(c, sl, 4, mem, out_prerefund + off * 96, (size_t)m * 96, &a.prerefund))) return rc;
    // A call of one short chunk is latency: k_prove_tail (C and r*: functions of the generator bytes alone) then runs on the OTHER
    // slot's stream beside head / bits / enc instead of behind them (0.5 ms of a 3.6 ms single-item prove_spend)
    const bool side = nchunks == 1 && depth > 1 && m <= 8192;
    Slot& other = c->slots[(i + 1) % depth];
    if (side) {
      if ((rc = copy_chain_record(c, sl, false))) return rc;                       // inputs and generator bytes are in place
      HIPCK(c, hipStreamWaitEvent(other.stream, sl.cp_in_ev, 0));
      if ((rc = prof_launch_on(c, sl, other.stream, PK_PROVE_TAIL, m, [&] { launch_prove_tail(a, other.stream); }))) return rc;
      if ((rc = copy_chain_record(c, other, true))) return rc;
    }
    if ((rc = prof_launch(c, sl, PK_PROVE_HEAD, m, [&] { launch_prove_head(a, sl.stream); }))) return rc;
    if ((rc = prof_launch(c, sl, PK_PROVE_BITS, (uint64_t)m * c->L, [&] { launch_prove_bits(a, sl.stream); }))) return rc;
    if ((rc = prof_launch(c, sl, PK_PROVE_ENC, (uint64_t)m * c->L * 3, [&] { launch_prove_enc(a, sl.stream); }))) return rc;
    if (side) HIPCK(c, hipStreamWaitEvent(sl.stream, other.cp_out_ev, 0));
    else if ((rc = prof_launch(c, sl, PK_PROVE_TAIL, m, [&] { launch_prove_tail(a, sl.stream); }))) return rc;
    return hash_begin(c, sl, PK_HASH_SPEND, sl.d_tr, (uint32_t)st.stride(), (uint32_t)st.bytes(), m);
  };
  auto stage2 = [&](size_t i) -> int {
    Slot& sl = c->slots[i % depth]; ProveArgs& a = args[i % depth];
    uint32_t m = ms[i % depth]; size_t off = offs[i % depth];
    int rc;
    if ((rc = hash_end(c, sl, (uint32_t)st.stride(), (uint32_t)st.bytes(), m))) return rc;
    if ((rc = prof_launch(c, sl, PK_PROVE_RESP, (uint64_t)m * c->L, [&] { launch_prove_resp(a, sl.stream); }))) return rc;
    if ((rc = dev_out_end(c, sl, mem, out_proof + off * pb, a.proof, (size_t)m * pb))) return rc;
    if ((rc = dev_out_end(c, sl, mem, out_prerefund + off * 96, a.prerefund, (size_t)m * 96))) return rc;
    return copy_status_out(c, sl, mem, status + off, m);
  };
  int rc;
  for (size_t i = 0; i < nchunks; i++) {
    if (i >= depth) { HIPCK(c, hipStreamSynchronize(c->slots[i % depth].stream)); }
    if ((rc = stage1(i))) return rc;
    if (i + 1 >= depth && (rc = stage2(i + 1 - depth))) return rc;
  }
  for (size_t i = nchunks >= depth ? nchunks - depth + 1 : 0; i < nchunks; i++) if ((rc = stage2(i))) return rc;
  return call.finish();
}
int act_prove_spend_batch(act_ctx* c, size_t n, int mem, const uint8_t* token, const uint8_t* s, const uint8_t* rng,
                          uint8_t* out_proof, uint8_t* out_prerefund, uint8_t* status) {
  if (!c || (n && (!token || !s || !rng || !out_proof || !out_prerefund || !status))) return ACT_ERR_ARG;
  return prove_spend_impl(c, n, mem, token, s, rng, nullptr, 0, out_proof, out_prerefund, status);
}
// request binding (DESIGN 4.12): prove_spend with n * 32 bytes of associated data in the challenge hash; bind == NULL is act_prove_spend_batch
int act_prove_spend_bound_batch(act_ctx* c, size_t n, int mem, const uint8_t* token, const uint8_t* s, const uint8_t* rng, const uint8_t* bind,
                                uint8_t* out_proof, uint8_t* out_prerefund, uint8_t* status) {
  if (!c || (n && (!token || !s || !rng || !out_proof || !out_prerefund || !status))) return ACT_ERR_ARG;
  return prove_spend_impl(c, n, mem, token, s, rng, nullptr, 0, out_proof, out_prerefund, status, bind);
}
int act_prove_spend_seeded_batch(act_ctx* c, size_t n, int mem, const uint8_t* token, const uint8_t* s, const uint8_t seed[32], uint64_t first_lane,
                                 uint8_t* out_proof, uint8_t* out_prerefund, uint8_t* status) {
  if (!c || !seed || (n && (!token || !s || !out_proof || !out_prerefund || !status))) return ACT_ERR_ARG;
  return prove_spend_impl(c, n, mem, token, s, nullptr, seed, first_lane, out_proof, out_prerefund, status);
}

// Two slots that each copy in, compute, copy out fall into step when left alone: both copy in at once (sharing the link), then both
// compute, then both copy out, and nothing overlaps (docs/history/profiles/r04_codec_trace.txt).  Chaining the copies of one direction across
// the two streams keeps them in anti-phase: chunk k + 1 copies in while chunk k computes.
// the chunk on `sl` is about to copy in (out = false) or out (out = true): after the other slot's copy of the same direction
static int copy_chain_wait(act_ctx* c, Slot& sl, bool out) {
  Slot& other = c->slots[&sl == &c->slots[0] ? 1 : 0];
  hipEvent_t ev = out ? other.cp_out_ev : other.cp_in_ev;
  if (ev) HIPCK(c, hipStreamWaitEvent(sl.stream, ev, 0));
  return ACT_OK;
}
static int copy_chain_record(act_ctx* c, Slot& sl, bool out) {
  hipEvent_t& ev = out ? sl.cp_out_ev : sl.cp_in_ev;
  if (!ev) HIPCK(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  HIPCK(c, hipEventRecord(ev, sl.stream));
  return ACT_OK;
}

static int client_batch(act_ctx* c, size_t n, int mem, int label, const uint8_t* pre, const uint8_t w[32], const uint8_t* req,
                        const uint8_t* resp, const uint8_t* proofs, uint8_t* out_token, uint8_t* status, bool with_t = false) {
  Call call(c, n);
  HIPCK(c, hipSetDevice(c->device));
  int rc = set_pubkey(c, w); if (rc) return rc;
  const bool issuance = label == LABEL_RESPOND;
  const size_t pre_b = issuance ? 64 : 96, resp_b = (issuance || with_t) ? 160 : 128, pb = ProofLayout{c->L}.bytes();
  // Host-memory callers: the refund check reads every proof (16.8 KB per lane over PCIe against ~0.2 us of kernels), so the call is
  // cut into quarters that alternate between the two slots -- a chunk's kernels and copy out run under the next chunk's copy in.
  // Device-memory callers: one slot, full-size chunks.
  size_t chunk = std::min(c->max_batch, std::max<size_t>(16384, (n / 4 + 1023) / 1024 * 1024));      // (below 16 384 lanes the kernels no longer fill the chip)
  // (issuance: 352 B per lane, nothing to hide)
  const bool taper_off = tune(T_NO_TAPER) != 0;
  const uint8_t* proofs_view = (!issuance && mem == ACT_MEM_HOST) ? mapped_view(c, proofs, n * pb) : nullptr;      // pinned: the SpendProofs (public, 16.8 KB each) are read in place
  const bool two_slots = mem == ACT_MEM_HOST && !issuance && !proofs_view && c->depth > 1 && n > chunk && !taper_off;
  if (!two_slots) chunk = c->max_batch;
  size_t k = 0;
  for (size_t off = 0; off < n; off += chunk, k++) {
    Slot& sl = c->slots[two_slots ? (k & 1) : 0];
    if (two_slots) HIPCK(c, hipStreamSynchronize(sl.stream));      // the chunk before last has left this slot's staging areas
    uint32_t m = (uint32_t)std::min(chunk, n - off);
    sl.d_trs_dirty = std::max(sl.d_trs_dirty, (size_t)m);
    ClientArgs a{}; a.P = c->P; a.w = c->w_pub; a.n = m; a.label = label; a.coords = sl.d_coords; a.trs = sl.d_trs; a.flags = sl.d_flags; a.pbk = sl.d_buckets;
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
    a.fused = (m <= TINY_MAX && tiny_enabled(c)) ? 1 : 0;          // tiny calls: phase A, the hash and phase B in one launch (k_client.hip)
    if ((rc = prof_launch(c, sl, PK_CLIENT, m, [&] { launch_client_a(a, sl.stream); }))) return rc;
    if (!a.fused) {
      uint32_t len = c->P.prefix_len[label] + 40u * (issuance ? 7u : 6u);
      if ((rc = hash_step(c, sl, PK_HASH_SMALL, sl.d_trs, SMALL_TR_STRIDE, len, m))) return rc;
      if ((rc = prof_launch(c, sl, PK_CLIENT, m, [&] { launch_client_b(a, sl.stream); }))) return rc;
    }
    if ((rc = dev_out_end(c, sl, mem, out_token + off * 160, a.out_token, (size_t)m * 160))) return rc;
    if ((rc = copy_status_out(c, sl, mem, status + off, m))) return rc;
    if (!two_slots && (rc = sync_all(c))) return rc;
  }
  return call.finish();      // waits for both streams
}
int act_issuance_to_credit_token_batch(act_ctx* c, size_t n, int mem, const uint8_t* pre, const uint8_t w[32], const uint8_t* req,
                                       const uint8_t* resp, uint8_t* out_token, uint8_t* status) {
  if (!c || !w || (n && (!pre || !req || !resp || !out_token || !status))) return ACT_ERR_ARG;
  return client_batch(c, n, mem, LABEL_RESPOND, pre, w, req, resp, nullptr, out_token, status);
}
int act_refund_to_credit_token_batch(act_ctx* c, size_t n, int mem, const uint8_t* prerefund, const uint8_t* proof, const uint8_t* refund,
                                     const uint8_t w[32], uint8_t* out_token, uint8_t* status) {
  if (!c || !w || (n && (!prerefund || !proof || !refund || !out_token || !status))) return ACT_ERR_ARG;
  return client_batch(c, n, mem, LABEL_REFUND, prerefund, w, nullptr, refund, proof, out_token, status);
}
// PreRefund::to_credit_token over RefundReturn records (DESIGN 4.10): the proof is checked over X_A = g + K' + t h1 and the token holds
// (m + t) mod l; a validly signed t > s (s: field 1 of the lane's proof) is ACT_STATUS_AMOUNT_TOO_BIG.  The same chunking, kernels and
// roads by n as the call above -- the kernels take the record's fifth field into X_A and the finish (return_lanes.h)
int act_refund_to_credit_token_return_batch(act_ctx* c, size_t n, int mem, const uint8_t* prerefund, const uint8_t* proof, const uint8_t* refund_return,
                                            const uint8_t w[32], uint8_t* out_token, uint8_t* status) {
  if (!c || !w || (n && (!prerefund || !proof || !refund_return || !out_token || !status))) return ACT_ERR_ARG;
  return client_batch(c, n, mem, LABEL_REFUND, prerefund, w, nullptr, refund_return, proof, out_token, status, true);
}
