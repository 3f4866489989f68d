// admit_replay_impl.inc — included by engine.hip behind replay_impl.inc: admission for the replayable redemption (DESIGN 4.9; kernels in
// k_admit_replay.hip, lane bodies in admit_replay_lanes.h).  act_redeem_(cbor_)admit_replay_batch are redeem_admit (admit_impl.inc)
// with one stage between its screen and its compaction, and the replay tail (replay_impl.inc) where the admission calls have the ring
// redeem tail:
//   a. compaction    the lanes the screen found spent, in lane order                            [k_admit_replay_key, k_admit_count / _scan / _write]
//   b. windows       ADMIT_WINDOW_BATCHES * max_batch spent lanes at a time: their records (records callers: gathered; host memory:
//                    the Com span alone crosses the link) or their messages turned into records (k_cbor_unframe_raw, then the
//                    configured reader over the spellings it flags), Com_j -> Niels, Horner -> enc(K') -> tag    [k_kprime_decode, k_kprime_tag]
//   c. look-up       the tags in `receipts`, read only
//   d. decision      tag found: a retry candidate, pre-status 0 -- verified like a fresh lane; otherwise (or a Com_j that is no point)
//                    the lane stays ACT_STATUS_DOUBLE_SPEND, unverified                          [k_admit_replay_decide]
// The stage never accepts anything: every refund is behind a full verification, the check-and-insert and the receipts look-up of the
// tail.  All of its buffers hold public data (proof bytes, points, tags, lane numbers).
namespace {

struct AdmitComJob { uint8_t* dst; const uint8_t* src; const uint32_t* idx; size_t pb, at, span; };

}  // namespace

static int admit_replay_stage(act_ctx* c, act_nullifier_set* receipts, const AdmitReplayStage& g, size_t* candidates) {
  const size_t n = g.n; hipStream_t stream = g.stream; int rc;
  const int L = c->L; const ProofLayout pl{L}; const size_t pb = pl.bytes();
  ADCK(c, hipSetDevice(c->device));
  // ---- a. the spent lanes in lane order (the compaction's arrays are free until the survivors' compaction) ------------------------------
  DevTmp d_key(c);
  if ((rc = d_key.alloc(n))) return rc;
  uint32_t ns32 = 0;
  {
    AdmitReplayKeyArgs ka{(uint32_t)n, g.d_pre, d_key.p};
    launch_admit_replay_key(ka, stream);
    launch_admit_compact(d_key.p, (uint32_t)n, g.d_blk, g.d_idx, g.d_pos, g.d_total, stream);
    ADCK(c, hipGetLastError());
    ADCK(c, hipMemcpyAsync(&ns32, g.d_total, 4, hipMemcpyDeviceToHost, stream));
    ADCK(c, hipStreamSynchronize(stream));
  }
  const size_t ns = ns32;
  if (ns > n) { c->err = "admission: the compaction counted more spent lanes than lanes"; return ACT_ERR_HIP; }
  if (ns == 0) return ACT_OK;      // nothing is spent: the screen's answers stand
  std::vector<uint32_t> h_sidx(ns);
  ADCK(c, hipMemcpy(h_sidx.data(), g.d_idx, ns * 4, hipMemcpyDeviceToHost));

  // per spent lane: enc(K'), the tag, the mark of an undecodable Com_j, the receipts' answer
  DevTmp d_res(c);
  if ((rc = d_res.alloc(ns * 66))) return rc;
  uint8_t *d_kp = d_res.p, *d_tag = d_kp + ns * 32, *d_mark = d_tag + ns * 32, *d_found = d_mark + ns;
  ADCK(c, hipMemsetAsync(d_res.p, 0, ns * 66, stream));

  // ---- b. a window at a time: records, Niels coordinates (L * NIELS_WORDS words per lane) and flag words ----------------------------------
  const size_t W = std::max<size_t>(1, ADMIT_WINDOW_BATCHES * c->max_batch), wmax = std::min(W, ns);
  const size_t coord_bytes = wmax * (size_t)L * NIELS_WORDS * 4;
  DevTmp d_rec(c), d_co(c);
  if ((rc = d_rec.alloc(wmax * pb)) || (rc = d_co.alloc(coord_bytes + wmax * 4))) return rc;
  uint32_t* const d_coords = reinterpret_cast<uint32_t*>(d_co.p); uint32_t* const d_flags = reinterpret_cast<uint32_t*>(d_co.p + coord_bytes);

  // wire callers: the codec's layout, the window's messages (host-memory callers) with their offsets, the framing flags and the reader's codes
  const CborType* T = cbor_type(ACT_CBOR_SPEND_PROOF);
  CborLayout lay; if (g.wire) lay = cbor_layout(*T, L);
  const size_t ml = lay.tmpl.size(), nf = lay.pay_off.size(), fcap = (wmax + 3) & ~(size_t)3;
  DevTmp d_lay(c), d_wf(c), d_msg(c), d_off(c);
  size_t msg_cap = 0;
  uint32_t* d_pay = nullptr; uint8_t *d_kind = nullptr, *d_tmpl = nullptr;
  if (g.wire) {
    if ((rc = d_lay.alloc(nf * 5 + ml)) || (rc = d_wf.alloc(3 * fcap))) return rc;
    d_pay = reinterpret_cast<uint32_t*>(d_lay.p); d_kind = d_lay.p + nf * 4; d_tmpl = d_kind + nf;
    ADCK(c, hipMemcpyAsync(d_pay, lay.pay_off.data(), nf * 4, hipMemcpyHostToDevice, stream));
    ADCK(c, hipMemcpyAsync(d_kind, lay.kind.data(), nf, hipMemcpyHostToDevice, stream));
    ADCK(c, hipMemcpyAsync(d_tmpl, lay.tmpl.data(), ml, hipMemcpyHostToDevice, stream));
    if (!g.dev && g.offsets && (rc = d_off.alloc((wmax + 1) * 8))) return rc;
  }
  AdmitGather gather(c, stream, g.dev, g.wire ? g.cbor : g.proof, g.wire ? ml : pb, (g.wire && g.offsets) ? g.ext : nullptr);
  std::unique_ptr<uint8_t[]> h_com;      // records in host memory: the windows' Com spans (not zero-filled: every byte is written)
  const size_t com_at = 32 * (size_t)pl.com(0), com_span = 32 * (size_t)L;
  std::vector<uint8_t> h_flags; std::vector<size_t> which, local; WireWindow win;

  for (size_t w0 = 0; w0 < ns; w0 += W) {
    const size_t w = std::min(W, ns - w0);
    const uint32_t* h_idx = h_sidx.data() + w0;
    if (!g.wire && g.dev) {
      AdmitRowsArgs ra{d_rec.p, g.proof, g.d_idx + w0, (uint32_t)w, pb};
      launch_admit_rows(ra, stream);
    } else if (!g.wire) {      // only the Com span crosses the link
      if (!h_com) h_com.reset(new uint8_t[wmax * com_span]);
      AdmitComJob job{h_com.get(), g.proof, h_idx, pb, com_at, com_span};
      act_host_parallel_for(w, 16, 0, [](void* p, size_t i0, size_t i1) {
        const AdmitComJob& j = *static_cast<const AdmitComJob*>(p);
        for (size_t k = i0; k < i1; k++) memcpy(j.dst + k * j.span, j.src + (size_t)j.idx[k] * j.pb + j.at, j.span);
      }, &job);
      ADCK(c, hipMemcpy2DAsync(d_rec.p + com_at, pb, h_com.get(), com_span, com_span, w, hipMemcpyHostToDevice, stream));
    } else {
      // the window's messages in device memory, then records: the canonical ones by the unframing kernel, every other spelling by the
      // reader the context is set to (all of them have read before: the screen has their k and s from the same reader)
      if ((rc = gather.run(g.d_idx + w0, h_idx, w))) return rc;
      const uint8_t* d_in = gather.data(); const uint64_t* d_offsets = gather.dev_offsets();
      if (!g.dev) {
        const size_t bytes = g.offsets ? (size_t)gather.dst_off[w] : w * ml;
        if (bytes > msg_cap) { if ((rc = AdmitGather::regrow(c, d_msg, bytes))) return rc; msg_cap = bytes; }
        ADCK(c, hipMemcpyAsync(d_msg.p, gather.data(), bytes, hipMemcpyHostToDevice, stream));
        if (g.offsets) { ADCK(c, hipMemcpyAsync(d_off.p, gather.dst_off.data(), (w + 1) * 8, hipMemcpyHostToDevice, stream)); d_offsets = reinterpret_cast<const uint64_t*>(d_off.p); }
        d_in = d_msg.p;
      }
      ADCK(c, hipMemsetAsync(d_wf.p, 0, 3 * fcap, stream));
      CborArgs ua{}; ua.n = (uint32_t)w; ua.n_fields = (uint32_t)nf; ua.msg_len = (uint32_t)ml; ua.pay_off = d_pay; ua.kind = d_kind; ua.tmpl = d_tmpl;
      ua.in = d_in; ua.out = d_rec.p; ua.offsets = d_offsets; ua.status = d_wf.p;
      hipLaunchKernelGGL(k_cbor_unframe_raw, dim3((unsigned)((w * nf + 255) / 256)), dim3(256), 0, stream, ua, 0u);
      if (g.dev_reader) {
        CborReadArgs ra{};
        ra.T = *T; ra.L = L; ra.n = (uint32_t)w; ra.first = 0; ra.msg_len = (uint32_t)ml; ra.in = d_in; ra.offsets = d_offsets;
        ra.flags = d_wf.p; ra.rec = d_rec.p; ra.rec_stride = pb; ra.keep_fields = (uint32_t)nf; ra.code = d_wf.p + fcap; ra.info = d_wf.p + 2 * fcap;
        launch_cbor_read(ra, false, stream);
        ADCK(c, hipGetLastError());
      } else {
        ADCK(c, hipGetLastError());
        h_flags.resize(w);
        ADCK(c, hipMemcpyAsync(h_flags.data(), d_wf.p, w, hipMemcpyDeviceToHost, stream));
        ADCK(c, hipStreamSynchronize(stream));
        which.clear(); local.clear();
        for (size_t k = 0; k < w; k++) if (h_flags[k] & 0x80) { which.push_back(h_idx[k]); local.push_back(k); }
        for (size_t q0 = 0; q0 < which.size(); q0 += WIRE_SETTLE_WINDOW) {
          const size_t cnt = std::min(which.size(), q0 + WIRE_SETTLE_WINDOW) - q0;
          if ((rc = wire_window_read(c, stream, *T, *g.ext, g.dev, which.data() + q0, cnt, pb, win))) return rc;
          for (size_t k = 0; k < cnt; k++)      // (a message that does not read leaves an all-zero record, whose tag no receipt holds)
            ADCK(c, hipMemcpyAsync(d_rec.p + local[q0 + k] * pb, win.recs.data() + k * pb, pb, hipMemcpyHostToDevice, stream));
          ADCK(c, hipStreamSynchronize(stream));      // win is reused by the next window
        }
      }
    }
    ADCK(c, hipMemsetAsync(d_flags, 0, w * 4, stream));
    KprimeArgs ka{};
    ka.s.P.L = L; ka.s.proofs = d_rec.p; ka.s.n = (uint32_t)w; ka.s.coords = d_coords; ka.s.flags = d_flags;
    ka.kred = g.d_kred; ka.idx = g.d_idx + w0; ka.kp = d_kp + w0 * 32; ka.tag = d_tag + w0 * 32; ka.mark = d_mark + w0; ka.t = g.d_t;
    launch_kprime_decode(ka, stream);
    if (g.reserve) launch_kprime_tag_reserve(ka, stream);      // (the reserve form: tag_res, the candidate's s^ where the return form has its t)
    else if (ka.t) launch_kprime_tag_return(ka, stream); else launch_kprime_tag(ka, stream);      // (the candidate's t, by the same idx as its nullifier)
    ADCK(c, hipGetLastError());
    ADCK(c, hipStreamSynchronize(stream));      // the window's buffers are reused
  }

  // ---- c. the receipts, read only, and d. the decision -------------------------------------------------------------------------------------
  if ((rc = act_nullifier_contains_batch(receipts, ns, ACT_MEM_DEVICE, d_tag, 32, d_found))) {
    c->err = std::string("admission: receipts set: ") + act_nullifier_set_last_error(receipts);
    return rc;
  }
  AdmitReplayDecideArgs da{(uint32_t)n, g.d_pos, d_mark, d_found, g.d_pre};
  launch_admit_replay_decide(da, stream);
  ADCK(c, hipGetLastError());
  std::vector<uint8_t> mf(2 * ns);
  ADCK(c, hipMemcpyAsync(mf.data(), d_mark, 2 * ns, hipMemcpyDeviceToHost, stream));
  ADCK(c, hipStreamSynchronize(stream));
  *candidates = 0;
  for (size_t k = 0; k < ns; k++) *candidates += admit_replay_decide(ACT_STATUS_DOUBLE_SPEND, true, mf[k] != 0, mf[ns + k] != 0).candidate;
  return ACT_OK;
}

extern "C" int act_redeem_admit_replay_batch(act_ctx* c, act_nullifier_set* set, act_nullifier_set* receipts, size_t n, int mem, const uint8_t* keys, int nkeys,
                                             const uint32_t* key_epochs, int sign_key, const uint8_t* proof, const uint8_t* charge, const uint8_t nonce_key[32],
                                             uint8_t* out_refund, uint8_t* status, uint8_t* out_key, uint8_t* out_replayed, uint64_t* out_counts) {
  if (n && !proof) return ACT_ERR_ARG;
  return redeem_admit(AdmitCall(c, set, n, mem).ring(keys, nkeys, key_epochs, sign_key).records(proof).charged(charge).replays(receipts, nonce_key, out_replayed)
                          .answers(out_refund, status, out_key, out_counts));
}
extern "C" int act_redeem_cbor_admit_replay_batch(act_ctx* c, act_nullifier_set* set, act_nullifier_set* receipts, size_t n, int mem, const uint8_t* keys, int nkeys,
                                                  const uint32_t* key_epochs, int sign_key, const uint8_t* cbor, const uint64_t* offsets, const uint8_t* charge,
                                                  const uint8_t nonce_key[32], uint8_t* out_refund_cbor, uint8_t* status, uint8_t* out_key, uint8_t* out_replayed,
                                                  uint64_t* out_counts) {
  if (n && !cbor) return ACT_ERR_ARG;
  return redeem_admit(AdmitCall(c, set, n, mem).ring(keys, nkeys, key_epochs, sign_key).messages(cbor, offsets).charged(charge).replays(receipts, nonce_key, out_replayed)
                          .answers(out_refund_cbor, status, out_key, out_counts));
}

// the unique forms: the copy stage of the admission unique forms (copies_impl.inc) behind this screen, and copies SERVED from their
// leader's answer (copy_serve_lane; out_counts: ACT_ADMIT_REPLAY_UNIQUE_COUNTS values)
extern "C" int act_redeem_admit_replay_unique_batch(act_ctx* c, act_nullifier_set* set, act_nullifier_set* receipts, size_t n, int mem, const uint8_t* keys, int nkeys,
                                                    const uint32_t* key_epochs, int sign_key, const uint8_t* proof, const uint8_t* charge, const uint8_t nonce_key[32],
                                                    uint8_t* out_refund, uint8_t* status, uint8_t* out_key, uint8_t* out_replayed, uint64_t* out_counts) {
  if (n && !proof) return ACT_ERR_ARG;
  return redeem_admit(AdmitCall(c, set, n, mem).ring(keys, nkeys, key_epochs, sign_key).records(proof).charged(charge).replays(receipts, nonce_key, out_replayed)
                          .uniquely().answers(out_refund, status, out_key, out_counts));
}
extern "C" int act_redeem_cbor_admit_replay_unique_batch(act_ctx* c, act_nullifier_set* set, act_nullifier_set* receipts, size_t n, int mem, const uint8_t* keys,
                                                         int nkeys, const uint32_t* key_epochs, int sign_key, const uint8_t* cbor, const uint64_t* offsets,
                                                         const uint8_t* charge, const uint8_t nonce_key[32], uint8_t* out_refund_cbor, uint8_t* status, uint8_t* out_key,
                                                         uint8_t* out_replayed, uint64_t* out_counts) {
  if (n && !cbor) return ACT_ERR_ARG;
  return redeem_admit(AdmitCall(c, set, n, mem).ring(keys, nkeys, key_epochs, sign_key).messages(cbor, offsets).charged(charge).replays(receipts, nonce_key, out_replayed)
                          .uniquely().answers(out_refund_cbor, status, out_key, out_counts));
}

// ---- replayable partial refunds (DESIGN 4.10): the admission replay calls with the amounts t the issuer returns ----------------------------
// The screen's rule t <= s (ACT_STATUS_RETURN_TOO_BIG) behind the charge and in front of both look-ups; the receipt's tag and the derived
// nonces take t^ = t mod l (return_replay_lanes.h: t^ = 0 is the v1 hash, so `returned` null or all zero is act_redeem_(cbor_)admit_
// replay_batch with RefundReturn outputs); the signing step is the return calls'.  out_counts: ACT_RETURN_REPLAY_COUNTS values.
extern "C" int act_redeem_return_replay_batch(act_ctx* c, act_nullifier_set* set, act_nullifier_set* receipts, size_t n, int mem, const uint8_t* keys, int nkeys,
                                              const uint32_t* key_epochs, int sign_key, const uint8_t* proof, const uint8_t* charge, const uint8_t* returned,
                                              const uint8_t nonce_key[32], uint8_t* out_refund_return, uint8_t* status, uint8_t* out_key, uint8_t* out_replayed,
                                              uint64_t* out_counts) {
  return redeem_admit(AdmitCall(c, set, n, mem).ring(keys, nkeys, key_epochs, sign_key).records(proof).charged(charge).returns(returned)
                          .replays(receipts, nonce_key, out_replayed).answers(out_refund_return, status, out_key, out_counts));
}
extern "C" int act_redeem_cbor_return_replay_batch(act_ctx* c, act_nullifier_set* set, act_nullifier_set* receipts, size_t n, int mem, const uint8_t* keys, int nkeys,
                                                   const uint32_t* key_epochs, int sign_key, const uint8_t* cbor, const uint64_t* offsets, const uint8_t* charge,
                                                   const uint8_t* returned, const uint8_t nonce_key[32], uint8_t* out_refund_return_cbor, uint8_t* status,
                                                   uint8_t* out_key, uint8_t* out_replayed, uint64_t* out_counts) {
  return redeem_admit(AdmitCall(c, set, n, mem).ring(keys, nkeys, key_epochs, sign_key).messages(cbor, offsets).charged(charge).returns(returned)
                          .replays(receipts, nonce_key, out_replayed).answers(out_refund_return_cbor, status, out_key, out_counts));
}

// request binding (DESIGN 4.12): the two calls above with n * 32 bytes of associated data, which enter the challenge hash of every lane
// that is verified and nothing else -- tags, nonces and both sets are those of the unbound call.  bind == NULL is the call above
extern "C" int act_redeem_return_replay_bound_batch(act_ctx* c, act_nullifier_set* set, act_nullifier_set* receipts, size_t n, int mem, const uint8_t* keys, int nkeys,
                                                    const uint32_t* key_epochs, int sign_key, const uint8_t* proof, const uint8_t* bind, const uint8_t* charge,
                                                    const uint8_t* returned, const uint8_t nonce_key[32], uint8_t* out_refund_return, uint8_t* status, uint8_t* out_key,
                                                    uint8_t* out_replayed, uint64_t* out_counts) {
  return redeem_admit(AdmitCall(c, set, n, mem).ring(keys, nkeys, key_epochs, sign_key).records(proof).bound(bind).charged(charge).returns(returned)
                          .replays(receipts, nonce_key, out_replayed).answers(out_refund_return, status, out_key, out_counts));
}
extern "C" int act_redeem_cbor_return_replay_bound_batch(act_ctx* c, act_nullifier_set* set, act_nullifier_set* receipts, size_t n, int mem, const uint8_t* keys,
                                                         int nkeys, const uint32_t* key_epochs, int sign_key, const uint8_t* cbor, const uint64_t* offsets,
                                                         const uint8_t* bind, const uint8_t* charge, const uint8_t* returned, const uint8_t nonce_key[32],
                                                         uint8_t* out_refund_return_cbor, uint8_t* status, uint8_t* out_key, uint8_t* out_replayed, uint64_t* out_counts) {
  return redeem_admit(AdmitCall(c, set, n, mem).ring(keys, nkeys, key_epochs, sign_key).messages(cbor, offsets).bound(bind).charged(charge).returns(returned)
                          .replays(receipts, nonce_key, out_replayed).answers(out_refund_return_cbor, status, out_key, out_counts));
}

// The unique forms of the two calls above: the copy stage of the admit-replay unique forms behind this screen, equality decided on the
// proof bytes ALONE (t takes no part, as in act_redeem_(cbor_)return_unique_batch), the amounts of the verified lanes gathered by v_idx --
// a copy's t never reaches a tag, a nonce or a signature -- and behind the tail a copy answered from its leader's final status and from
// whether it names its leader's amount (copy_serve_return_lane).  out_counts: ACT_RETURN_REPLAY_UNIQUE_COUNTS values.
extern "C" int act_redeem_return_replay_unique_batch(act_ctx* c, act_nullifier_set* set, act_nullifier_set* receipts, size_t n, int mem, const uint8_t* keys, int nkeys,
                                                     const uint32_t* key_epochs, int sign_key, const uint8_t* proof, const uint8_t* charge, const uint8_t* returned,
                                                     const uint8_t nonce_key[32], uint8_t* out_refund_return, uint8_t* status, uint8_t* out_key, uint8_t* out_replayed,
                                                     uint64_t* out_counts) {
  return redeem_admit(AdmitCall(c, set, n, mem).ring(keys, nkeys, key_epochs, sign_key).records(proof).charged(charge).returns(returned)
                          .replays(receipts, nonce_key, out_replayed).uniquely().answers(out_refund_return, status, out_key, out_counts));
}
extern "C" int act_redeem_cbor_return_replay_unique_batch(act_ctx* c, act_nullifier_set* set, act_nullifier_set* receipts, size_t n, int mem, const uint8_t* keys,
                                                          int nkeys, const uint32_t* key_epochs, int sign_key, const uint8_t* cbor, const uint64_t* offsets,
                                                          const uint8_t* charge, const uint8_t* returned, const uint8_t nonce_key[32], uint8_t* out_refund_return_cbor,
                                                          uint8_t* status, uint8_t* out_key, uint8_t* out_replayed, uint64_t* out_counts) {
  return redeem_admit(AdmitCall(c, set, n, mem).ring(keys, nkeys, key_epochs, sign_key).messages(cbor, offsets).charged(charge).returns(returned)
                          .replays(receipts, nonce_key, out_replayed).uniquely().answers(out_refund_return_cbor, status, out_key, out_counts));
}
