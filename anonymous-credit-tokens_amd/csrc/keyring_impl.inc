// keyring_impl.inc — included by engine.hip inside its extern "C" block: key rotation.  One batch of spend proofs verified against an
// ordered ring of up to ACT_KEYRING_MAX issuer keys, and refunds signed with a key chosen per lane.
//
// A SpendProof carries no key identifier, and the issuer's x enters verification only through A1 (keyring_lanes.h).  A ring call
// therefore runs the one-key kernels ONCE, under ring key 0 -- the chunked two-slot schedule of spend_batch_locked, same chunk sizes,
// same staggering -- and adds per chunk: the candidates A1_k of the other keys (k_ring_cand), their challenge hashes from chunk 0 of
// the transcript and the siblings of its path (device: k_ring_hash_full / k_ring_hash; host: act_host_hash_ring_many on the worker pool,
// for which only the candidates travel to the host beside the transcripts), and the ring form of the status kernel.
//
// Side buffers per lane of a slot: 96 B of candidates, 256 B of siblings, 256 B of XOF blocks, 2 index bytes (610 B; twice that per lane
// of max_batch for the two slots, plus 352 B per lane pinned on the host), allocated by a context's FIRST ring call and freed with it: a
// context that never sees a ring keeps the one-key footprint.  The decoded ring itself is staged in slot 0's stage 9 for the call and
// wiped by finish_call like every staged secret; the host copy of the last ring (decoded points, for calls that repeat it) dies with
// the context, as the cached one-key `key` does.
struct RingWs {
  uint8_t* d_cand[2] = {nullptr, nullptr};  uint32_t* d_sib[2] = {nullptr, nullptr};  uint32_t* d_xofs[2] = {nullptr, nullptr};
  uint8_t* d_okey[2] = {nullptr, nullptr};  uint8_t* d_kidx[2] = {nullptr, nullptr};
  uint8_t* h_cand[2] = {nullptr, nullptr};  uint32_t* h_xofs[2] = {nullptr, nullptr};      // pinned (host-transcript mode)
  uint8_t keys_cached[KEYRING_MAX * 64] = {}; uint32_t nkeys_cached = 0; DevKey ring[KEYRING_MAX] = {};
};

struct RingSel { const uint8_t* keys; int nkeys; uint8_t* out_key; const uint8_t* bind = nullptr; };      // a ring in place of `sk` (cbor_impl.inc verify_spend_cbor_impl); bind: the lanes' request bindings in the call's kind of memory, or null

extern "C" void act_host_hash_ring_many(const uint8_t* msgs, size_t stride, uint32_t len, size_t n, int max_threads, uint32_t nkeys, uint32_t rep_off,
                                        const uint8_t* cand, uint32_t* xofs);      // host_pool.cpp

static void ring_ws_free(act_ctx* c) {
  RingWs* w = c->ring_ws;
  if (!w) return;
  for (int s = 0; s < 2; s++) {
    void* dev[] = {w->d_cand[s], w->d_sib[s], w->d_xofs[s], w->d_okey[s], w->d_kidx[s]};
    for (void* p : dev) if (p) (void)hipFree(p);
    if (w->h_cand[s]) (void)hipHostFree(w->h_cand[s]);
    if (w->h_xofs[s]) (void)hipHostFree(w->h_xofs[s]);
  }
  wipe_host(reinterpret_cast<uint8_t*>(w->keys_cached), sizeof(w->keys_cached));
  wipe_host(reinterpret_cast<uint8_t*>(w->ring), sizeof(w->ring));
  delete w;
  c->ring_ws = nullptr;
}
static int ring_ws_get(act_ctx* c) {
  if (c->ring_ws) return ACT_OK;
  RingWs* w = c->ring_ws = new RingWs();      // (a failed allocation below leaves a partial set: freed with the context)
  const size_t B = c->max_batch;
  for (int s = 0; s < 2; s++) {
    HIPCK(c, hipMalloc(&w->d_cand[s], B * (KEYRING_MAX - 1) * 32));
    HIPCK(c, hipMalloc(&w->d_sib[s], B * B3_MAX_SIBLINGS * 32));
    HIPCK(c, hipMalloc(&w->d_xofs[s], B * KEYRING_MAX * 64));
    HIPCK(c, hipMalloc(&w->d_okey[s], B));
    HIPCK(c, hipMalloc(&w->d_kidx[s], B));
    HIPCK(c, hipHostMalloc(&w->h_cand[s], B * (KEYRING_MAX - 1) * 32, hipHostMallocDefault));
    HIPCK(c, hipHostMalloc(&w->h_xofs[s], B * KEYRING_MAX * 64, hipHostMallocDefault));
  }
  return ACT_OK;
}
// Decodes the ring (set_key's rule: nothing of a rejected ring replaces what is cached) and stages it on the device for this call.
static int ring_set(act_ctx* c, const uint8_t* keys, int nkeys, const DevKey** d_ring) {
  if (!keys || nkeys < 1 || nkeys > KEYRING_MAX) { c->err = "key ring: nkeys must be 1 .. ACT_KEYRING_MAX and keys non-null"; return ACT_ERR_ARG; }
  int rc = ring_ws_get(c); if (rc) return rc;
  RingWs* w = c->ring_ws;
  if (!(w->nkeys_cached == (uint32_t)nkeys && ct_equal(w->keys_cached, keys, (size_t)nkeys * 64))) {
    DevKey tmp[KEYRING_MAX];
    for (int k = 0; k < nkeys; k++) {
      uint32_t x[8]; memcpy(x, keys + 64 * k, 32);
      tmp[k].x = sc_from_words(x);
      if ((rc = decode_one(c, keys + 64 * k + 32, &tmp[k].w))) { wipe_host(reinterpret_cast<uint8_t*>(tmp), sizeof(tmp)); return rc; }
    }
    w->nkeys_cached = 0;
    for (int k = 0; k < nkeys; k++) w->ring[k] = tmp[k];
    memcpy(w->keys_cached, keys, (size_t)nkeys * 64); w->nkeys_cached = (uint32_t)nkeys;
    wipe_host(reinterpret_cast<uint8_t*>(tmp), sizeof(tmp));
  }
  Slot& s0 = c->slots[0];
  if ((rc = stage_reserve(c, s0, 9, sizeof(DevKey) * KEYRING_MAX))) return rc;
  HIPCK(c, hipMemcpyAsync(s0.d_stage[9], w->ring, sizeof(DevKey) * (size_t)nkeys, hipMemcpyHostToDevice, s0.stream));
  HIPCK(c, hipStreamSynchronize(s0.stream));      // the other slot's stream reads it too
  *d_ring = reinterpret_cast<const DevKey*>(s0.d_stage[9]);
  return ACT_OK;
}

// spend_batch_locked's pipeline with the ring steps in it.  The caller holds the context (Call) and has staged the ring (ring_set).
// bind (DESIGN 4.12, request binding): n * 32 bytes in `mem` memory or null.  Each chunk brings its 32 m bytes in the way it brings its
// proofs in, the prep kernel writes them as the transcript's last element, and every hash of the call takes the bound length.
static int ring_verify_locked(act_ctx* c, size_t n, int mem, const DevKey* d_ring, int nkeys, const uint8_t* proof, uint8_t* status, uint8_t* out_key,
                              uint8_t* out_kprime, const WireSrc* wire = nullptr, const uint8_t* bind = nullptr) {
  RingWs* w = c->ring_ws;
  const SpendTranscript st{c->L, bind != nullptr};
  const size_t pb = ProofLayout{c->L}.bytes();
  const uint32_t extra = (uint32_t)nkeys - 1u, stride = (uint32_t)st.stride(), len = (uint32_t)st.bytes();
  const uint8_t* proof_view = (mem == ACT_MEM_HOST && !wire) ? mapped_view(c, proof, n * pb) : nullptr;
  const bool in_host = mem == ACT_MEM_HOST && !proof_view;
  const uint8_t* bind_view = (bind && mem == ACT_MEM_HOST) ? mapped_view(c, bind, n * 32) : nullptr;
  bool stagger = false;
  const std::vector<std::pair<size_t, size_t>> sched = spend_schedule(c, n, in_host, &stagger);
  const size_t nchunks = sched.size(), depth = (size_t)c->depth;
  SpendChunk chunks[2]; RingArgs rings[2];
  c->last_bits_ev = nullptr; c->last_bits_sig = nullptr;
  for (Slot& sl : c->slots) if (sl.bits_sig) { *(volatile uint32_t*)sl.bits_sig = 0; sl.bits_wgs = 0; }
  auto stage1 = [&](size_t i) -> int {
    const size_t s = i % depth;
    Slot& sl = c->slots[s]; SpendChunk& ch = chunks[s]; RingArgs& r = rings[s];
    ch = SpendChunk{}; ch.off = sched[i].first; ch.m = (uint32_t)sched[i].second; ch.stagger = stagger;
    int rc;
    if (wire) { if ((rc = wire_unframe_chunk(c, sl, *wire, mem, ch.off, ch.m, &ch.d_proofs))) return rc; }
    else if (proof_view) ch.d_proofs = proof_view + ch.off * pb;
    else if ((rc = dev_in(c, sl, 0, mem, proof + ch.off * pb, (size_t)ch.m * pb, &ch.d_proofs))) return rc;
    if (bind_view) ch.d_bind = bind_view + ch.off * 32;
    else if (bind && (rc = dev_in(c, sl, 5, mem, bind + ch.off * 32, (size_t)ch.m * 32, &ch.d_bind))) return rc;
    if (out_kprime && (rc = dev_out_begin(c, sl, 2, mem, out_kprime + ch.off * 32, (size_t)ch.m * 32, &ch.d_kprime))) return rc;
    if ((rc = spend_stage1_kernels(c, sl, ch, w->ring[0]))) return rc;
    r = RingArgs{}; r.s = ch.a; r.ring = d_ring; r.nkeys = (uint32_t)nkeys;
    r.cand = w->d_cand[s]; r.sib = w->d_sib[s]; r.xofs = w->d_xofs[s]; r.out_key = w->d_okey[s];
    if (extra && (rc = prof_launch(c, sl, PK_RING_CAND, (uint64_t)ch.m * extra, [&] { launch_ring_cand(r, sl.stream); }))) return rc;
    if (c->tr_mode == ACT_TRANSCRIPT_DEVICE) {
      if ((rc = prof_launch(c, sl, PK_HASH_SPEND, ch.m, [&] { launch_ring_hash_full(r, sl.stream); }))) return rc;
      if (extra && (rc = prof_launch(c, sl, PK_RING_HASH, (uint64_t)ch.m * extra, [&] { launch_ring_hash(r, sl.stream); }))) return rc;
    } else {
      // the candidates go first: every piece event of hash_begin then covers them
      if (extra) HIPCK(c, hipMemcpyAsync(w->h_cand[s], w->d_cand[s], (size_t)ch.m * extra * 32, hipMemcpyDeviceToHost, sl.stream));
      if ((rc = hash_begin(c, sl, PK_HASH_SPEND, sl.d_tr, stride, len, ch.m))) return rc;
    }
    sl.last_spend_lanes = ch.m;
    return ACT_OK;
  };
  auto stage2 = [&](size_t i) -> int {
    const size_t s = i % depth;
    Slot& sl = c->slots[s]; SpendChunk& ch = chunks[s]; RingArgs& r = rings[s];
    int rc;
    if (c->tr_mode == ACT_TRANSCRIPT_HOST) {
      auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
      const int pieces = hash_pieces(ch.m);
      for (int k = 0; k < pieces; k++) {
        const size_t i0 = (size_t)ch.m * k / pieces, i1 = (size_t)ch.m * (k + 1) / pieces;
        const double t0 = now();
        HIPCK(c, hipEventSynchronize(sl.h_ev[k]));
        const double t1 = now();
        if (i1 > i0) act_host_hash_ring_many(sl.h_tr + i0 * stride, stride, len, i1 - i0, c->host_threads, (uint32_t)nkeys, ring_a1_offset(c->L),
                                             w->h_cand[s] + i0 * extra * 32, w->h_xofs[s] + i0 * (size_t)nkeys * 16);
        const double t2 = now();
        c->host_wait_s += t1 - t0; c->host_hash_s += t2 - t1; c->host_hash_bytes += (uint64_t)(i1 - i0) * len;
      }
      HIPCK(c, hipMemcpyAsync(w->d_xofs[s], w->h_xofs[s], (size_t)ch.m * nkeys * 64, hipMemcpyHostToDevice, sl.stream));
    }
    if ((rc = prof_launch(c, sl, PK_RING_FINISH, ch.m, [&] { launch_ring_finish(r, sl.stream); }))) return rc;
    if (out_kprime && (rc = dev_out_end(c, sl, mem, out_kprime + ch.off * 32, ch.d_kprime, (size_t)ch.m * 32))) return rc;
    c->last_spend_slot = (int)s;
    HIPCK(c, hipMemcpyAsync(out_key + ch.off, w->d_okey[s], ch.m, mem == ACT_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, sl.stream));
    return copy_status_out(c, sl, mem, status + ch.off, ch.m);
  };
  int rc;
  for (size_t i = 0; i < nchunks; i++) {
    if (i >= depth) { HIPCK(c, hipStreamSynchronize(c->slots[i % depth].stream)); }
    if ((rc = stage1(i))) return rc;
    if (i + 1 >= depth && (rc = stage2(i + 1 - depth))) return rc;
  }
  for (size_t i = nchunks >= depth ? nchunks - depth + 1 : 0; i < nchunks; i++) if ((rc = stage2(i))) return rc;
  return sync_all(c);
}

// request binding (DESIGN 4.12): the ring call with n * 32 bytes of associated data in the challenge hash; bind == NULL is the ring call
int act_verify_spend_keyring_bound_batch(act_ctx* c, size_t n, int mem, const uint8_t* keys, int nkeys, const uint8_t* proof, const uint8_t* bind,
                                         uint8_t* status, uint8_t* out_key, uint8_t* out_kprime) {
  if (!c || !keys || nkeys < 1 || nkeys > ACT_KEYRING_MAX || (n && (!proof || !status || !out_key))) return ACT_ERR_ARG;
  if (n >= ((size_t)1 << 32)) return ACT_ERR_ARG;
  Call call(c, n);
  HIPCK(c, hipSetDevice(c->device));
  const DevKey* d_ring = nullptr;
  int rc = ring_set(c, keys, nkeys, &d_ring); if (rc) return rc;
  if ((rc = ring_verify_locked(c, n, mem, d_ring, nkeys, proof, status, out_key, out_kprime, nullptr, bind))) return rc;
  return call.finish();
}
int act_verify_spend_keyring_batch(act_ctx* c, size_t n, int mem, const uint8_t* keys, int nkeys, const uint8_t* proof, uint8_t* status,
                                   uint8_t* out_key, uint8_t* out_kprime) {
  return act_verify_spend_keyring_bound_batch(c, n, mem, keys, nkeys, proof, nullptr, status, out_key, out_kprime);
}

// act_refund_sign_batch with the key chosen per lane: a lane whose status_in is 0 and whose key_index is not below nkeys is not signed
// (status 255, zero record, no rng slice) -- the array may live in device memory, so that is the lane's verdict, not the call's.
// with_t (act_refund_sign_return_keyring_batch, DESIGN 4.10): X_A = g + K' + t h1 and 160-byte RefundReturn records; returned = n
// scalars in `mem` memory, or null (every t = 0: no product on h1 at all).  frame (with_t only; the wire form of the return calls):
// out_refund takes n ACT_CBOR_REFUND_RETURN messages framed by phase B (k_sign_b_frame_ring), all zero where not signed, instead of records
static int refund_return_frame_prepare(act_ctx* c, FrameOut* fo);      // keyring_redeem_impl.inc, behind the codec
static int refund_sign_keyring_impl(act_ctx* c, size_t n, int mem, const uint8_t* keys, int nkeys, const uint8_t* key_index, const uint8_t* kprime,
                                    const uint8_t* status_in, const uint8_t* rng, int rng_mode, uint8_t* out_refund, uint8_t* status, bool with_t,
                                    const uint8_t* returned, bool frame = false) {
  size_t rec = with_t ? 160 : 128;
  if (frame && !with_t) return ACT_ERR_ARG;
  if (!c || !keys || nkeys < 1 || nkeys > ACT_KEYRING_MAX || (n && (!key_index || !kprime || !status_in || !rng || !out_refund || !status))) return ACT_ERR_ARG;
  if (rng_mode != ACT_RNG_PER_LANE && rng_mode != ACT_RNG_SEQUENTIAL) return ACT_ERR_ARG;
  Call call(c, n);
  HIPCK(c, hipSetDevice(c->device));
  const DevKey* d_ring = nullptr;
  int rc = ring_set(c, keys, nkeys, &d_ring); if (rc) return rc;
  RingWs* w = c->ring_ws;
  FrameOut fo{nullptr, nullptr, 0};
  if (frame) { if ((rc = refund_return_frame_prepare(c, &fo))) return rc; rec = fo.len; }
  const hipMemcpyKind in_kind = mem == ACT_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  size_t cursor = 0, chunk = 0;
  for (size_t off = 0; off < n; off += c->max_batch, chunk++) {
    const size_t s = chunk % c->depth;
    Slot& sl = c->slots[s];
    if (chunk >= (size_t)c->depth) { HIPCK(c, hipStreamSynchronize(sl.stream)); if ((rc = prof_collect(c, sl))) return rc; }
    const uint32_t m = (uint32_t)std::min(c->max_batch, n - off);
    SignXaArgs x{}; x.P = c->P; x.n = m; x.point_stride = 32; x.xa = sl.d_xa; x.status = sl.d_status;
    if ((rc = dev_in(c, sl, 0, mem, kprime + off * 32, (size_t)m * 32, &x.point))) return rc;
    if (returned && (rc = dev_in(c, sl, 1, mem, returned + off * 32, (size_t)m * 32, &x.t_amount))) return rc;
    HIPCK(c, hipMemcpyAsync(sl.d_status, status_in + off, m, in_kind, sl.stream));
    HIPCK(c, hipMemcpyAsync(w->d_kidx[s], key_index + off, m, in_kind, sl.stream));
    uint8_t* d_out;
    if ((rc = dev_out_begin(c, sl, 2, mem, out_refund + off * rec, (size_t)m * rec, &d_out))) return rc;
    launch_ring_index_check(sl.d_status, w->d_kidx[s], (uint32_t)nkeys, m, sl.stream);
    launch_sign_xa(x, sl.stream);
    const uint8_t* d_rng;
    if ((rc = prepare_rng_slots(c, sl, m, off, mem, rng, rng_mode, &cursor, &d_rng))) return rc;
    sl.d_trs_dirty = std::max(sl.d_trs_dirty, (size_t)m);
    SignRingArgs g{}; g.ring = d_ring; g.key_index = w->d_kidx[s]; g.nkeys = (uint32_t)nkeys;
    SignArgs& a = g.s; a.P = c->P; a.n = m; a.label = LABEL_REFUND; a.xa = sl.d_xa; a.status = sl.d_status; a.rng_slot = sl.d_slot;
    a.rng = d_rng; a.trs = sl.d_trs; a.state = sl.d_state; a.xof = sl.d_xof; a.out = d_out; a.pbk = sl.d_buckets;
    a.with_t = with_t ? 1 : 0; a.t_amount = x.t_amount;
    if (frame) { a.frame = fo.tmpl; a.frame_off = fo.off; a.frame_len = fo.len; }
    if ((rc = prof_launch(c, sl, PK_SIGN_A, m, [&] { launch_sign_a_ring(g, sl.stream); }))) return rc;
    if ((rc = hash_step(c, sl, PK_HASH_SMALL, sl.d_trs, SMALL_TR_STRIDE, c->P.prefix_len[LABEL_REFUND] + 40u * 6u, m))) return rc;
    if ((rc = prof_launch(c, sl, frame ? PK_SIGN_B_FRAME : PK_SIGN_B, m, [&] { launch_sign_b_ring(g, sl.stream); }))) return rc;
    if ((rc = dev_out_end(c, sl, mem, out_refund + off * rec, d_out, (size_t)m * rec))) return rc;
    if ((rc = copy_status_out(c, sl, mem, status + off, m))) return rc;
  }
  return call.finish();
}
int act_refund_sign_keyring_batch(act_ctx* c, size_t n, int mem, const uint8_t* keys, int nkeys, const uint8_t* key_index, const uint8_t* kprime,
                                  const uint8_t* status_in, const uint8_t* rng, int rng_mode, uint8_t* out_refund, uint8_t* status) {
  return refund_sign_keyring_impl(c, n, mem, keys, nkeys, key_index, kprime, status_in, rng, rng_mode, out_refund, status, false, nullptr);
}
// the same signature over X_A = g + K' + t h1 (DESIGN 4.10).  This call does not see s: the bound t <= s is the caller's
int act_refund_sign_return_keyring_batch(act_ctx* c, size_t n, int mem, const uint8_t* keys, int nkeys, const uint8_t* key_index, const uint8_t* kprime,
                                         const uint8_t* status_in, const uint8_t* rng, int rng_mode, const uint8_t* returned, uint8_t* out_refund_return,
                                         uint8_t* status) {
  return refund_sign_keyring_impl(c, n, mem, keys, nkeys, key_index, kprime, status_in, rng, rng_mode, out_refund_return, status, true, returned);
}
