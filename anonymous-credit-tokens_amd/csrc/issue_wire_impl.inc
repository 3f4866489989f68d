// issue_wire_impl.inc — wire bytes in, wire bytes out for issuance (include/act_mi355x.h act_issue_*cbor_batch), included by engine.hip
// after cbor_impl.inc.  Lane i is one iteration of the issuer's loop
//     IssuanceRequest::from_cbor(msg_i)          src/cbor.rs:118-148
//       .and_then(|r| sk.issue(params, &r, c_i, rng))   src/lib.rs:621-663
//       .map(|resp| resp.to_cbor())              src/cbor.rs:162-175
// without an IssuanceRequest, a RistrettoPoint or an IssuanceResponse on the host.  A chunk is ONE pipeline: k_issue_a_wire reads the
// canonical messages in place (unframing, K decoded once, the records from_cbor returns left in the slot's staging for k_issue_check and
// the signature), the transcript hash, k_issue_check, and -- for the whole endpoint -- the signature, whose phase B frames the
// IssuanceResponse messages (k_sign_b_frame).  What is not byte-for-byte canonical:
//   ACT_WIRE_READER_DEVICE (the default): k_issue_wire_flag marks it, k_cbor_read_raw reads it into the slot's records in the chunk's own
//     stream, k_issue_a_wire_read takes the record up and the lane is checked, signed and framed beside its canonical neighbours;
//     k_issue_check gives a message the reader refused its wire status (lane bodies: issue_wire_lanes.h).  Nothing is left for the end
//     of the call but counting the flags for act_ctx_wire_stats.
//   ACT_WIRE_READER_HOST: k_issue_a_wire flags it, and it is settled after the pipeline has drained, in windows of WIRE_SETTLE_WINDOW,
//     through the window of the spend path (wire_window_read in cbor_impl.inc over wire_window.h: gather, cbor_read_message,
//     cbor_settle_codes), then one small act_issue_check_batch.

namespace {

// the call's two message layouts on the device: IssuanceRequest in slot 0's layout area, IssuanceResponse in slot 1's
struct IssueWire { const uint8_t* cbor = nullptr; const uint64_t* offsets = nullptr; size_t ml = 0; CborDev req, resp; };
int issue_wire_prepare(act_ctx* c, IssueWire& w, bool want_req, bool want_resp) {
  int rc;
  if (want_req && (rc = cbor_dev_prepare(c, c->slots[0], ACT_CBOR_ISSUANCE_REQUEST, &w.req))) return rc;
  if (want_resp && (rc = cbor_dev_prepare(c, c->slots[1], ACT_CBOR_ISSUANCE_RESPONSE, &w.resp))) return rc;
  w.ml = w.req.lay.tmpl.size();
  return ACT_OK;
}

// out_req: the record of an accepted lane, zero for any other (16 bytes per thread; the caller's pointer may have any alignment)
__global__ void __launch_bounds__(256) k_issue_req_out(const uint8_t* rec, const uint8_t* status, uint8_t* out, uint32_t n) {
  const uint32_t gid = blockIdx.x * 256 + threadIdx.x;
  if (gid >= n * 8) return;
  const uint4 v = status[gid / 8] == 0 ? reinterpret_cast<const uint4*>(rec)[gid] : make_uint4(0, 0, 0, 0);
  __builtin_memcpy(out + (size_t)gid * 16, &v, 16);
}

// Check (and with `sign` -- ACT_RNG_PER_LANE only, where no slice depends on another lane's verdict -- sign and frame) every canonical
// message; chunks of max_batch alternate between the two slots as in issue_batch_impl.  dev_reader: every flagged message is read in
// front of phase A and goes through the same kernels.  Otherwise a flagged message leaves with status 255, a zero record and a zero
// slot.  The caller holds the context (Call).
int issue_wire_pipeline(act_ctx* c, size_t n, int mem, const IssueWire& w, const uint8_t* camt, const uint8_t* rng, bool sign, bool dev_reader,
                        uint8_t* out_resp, uint8_t* status, uint8_t* out_req) {
  const size_t rl = w.resp.lay.tmpl.size();
  const FrameOut fo{w.resp.tmpl, w.resp.pay_off, (uint32_t)rl};
  size_t cursor = 0, chunk = 0; int rc;
  for (size_t off = 0; off < n; off += c->max_batch, chunk++) {
    Slot& sl = c->slots[chunk % c->depth];
    if (chunk >= (size_t)c->depth) { HIPCK(c, hipStreamSynchronize(sl.stream)); if ((rc = prof_collect(c, sl))) return rc; }
    const uint32_t m = (uint32_t)std::min(c->max_batch, n - off);
    sl.d_trs_dirty = std::max(sl.d_trs_dirty, (size_t)m);
    IssueArgs a{}; a.P = c->P; a.n = m; a.trs = sl.d_trs; a.xa = sl.d_xa; a.flags = sl.d_flags; a.xof = sl.d_xof; a.status = sl.d_status; a.pbk = sl.d_buckets;
    // the chunk's bytes, staged (as wire_unframe_chunk does: 16-byte loads at 141-byte strides make poor reads over the link), offsets relative
    const size_t beg = w.offsets ? (size_t)w.offsets[off] : off * w.ml, end = w.offsets ? (size_t)w.offsets[off + m] : (off + m) * w.ml;
    if ((rc = dev_in(c, sl, 0, mem, w.cbor + beg, end - beg, &a.wire))) return rc;
    if (w.offsets) {
      sl.h_rel.resize((size_t)m + 1);                          // lives in the slot: the copy below is asynchronous
      for (size_t i = 0; i <= m; i++) sl.h_rel[i] = w.offsets[off + i] - beg;
      if ((rc = stage_reserve(c, sl, 7, ((size_t)m + 1) * 8))) return rc;
      a.wire_off = reinterpret_cast<const uint64_t*>(sl.d_stage[7]);
      HIPCK(c, hipMemcpyAsync(sl.d_stage[7], sl.h_rel.data(), ((size_t)m + 1) * 8, hipMemcpyHostToDevice, sl.stream));
    }
    if ((rc = stage_reserve(c, sl, 6, (size_t)m * 128))) return rc;
    a.rec_out = sl.d_stage[6]; a.req = a.rec_out;
    a.tmpl = w.req.tmpl; a.pay_off = w.req.pay_off; a.msg_len = (uint32_t)w.ml; a.wire_flags = c->d_wire_flags; a.first = (uint32_t)off;
    if (sign && (rc = dev_in(c, sl, 1, mem, camt + off * 32, (size_t)m * 32, &a.c_amount))) return rc;      // (null: no X_A)
    if (dev_reader) {
      // flag pass, plain pass, validating pass (a lane of either reader kernel returns at once unless its message is flagged), then phase A
      act::IssueWireFlagArgs fa{m, (uint32_t)off, (uint32_t)w.ml, a.wire, a.wire_off, a.tmpl, a.pay_off, c->d_wire_flags};
      if ((rc = prof_launch(c, sl, PK_ISSUE_WIRE_FLAG, m, [&] { launch_issue_wire_flag(fa, sl.stream); }))) return rc;
      CborReadArgs ra{};
      ra.T = *cbor_type(ACT_CBOR_ISSUANCE_REQUEST); ra.L = c->L; ra.n = m; ra.first = (uint32_t)off; ra.msg_len = (uint32_t)w.ml; ra.in = a.wire; ra.offsets = a.wire_off;
      ra.flags = c->d_wire_flags; ra.rec = a.rec_out; ra.rec_stride = 128; ra.keep_fields = 4; ra.code = c->d_wire_codes; ra.info = c->d_wire_codes + c->d_wire_codes_cap;
      if ((rc = prof_launch(c, sl, PK_CBOR_READ, m, [&] { launch_cbor_read(ra, false, sl.stream); }))) return rc;
      if ((rc = prof_launch(c, sl, PK_CBOR_READ_VALIDATE, m, [&] { launch_cbor_read(ra, true, sl.stream); }))) return rc;
      a.wire_code = c->d_wire_codes;
      if ((rc = prof_launch(c, sl, PK_ISSUE_A_WIRE, m, [&] { launch_issue_a_wire_read(a, sl.stream); }))) return rc;
    } else if ((rc = prof_launch(c, sl, PK_ISSUE_A_WIRE, m, [&] { launch_issue_a_wire(a, sl.stream); }))) return rc;
    if ((rc = hash_step(c, sl, PK_HASH_SMALL, sl.d_trs, SMALL_TR_STRIDE, c->P.prefix_len[LABEL_REQUEST] + 80, m))) return rc;
    if ((rc = prof_launch(c, sl, PK_ISSUE_CHECK, m, [&] { launch_issue_check(a, sl.stream); }))) return rc;
    if (out_req) {
      uint8_t* d_req;
      if ((rc = dev_out_begin(c, sl, 4, mem, out_req + off * 128, (size_t)m * 128, &d_req))) return rc;
      hipLaunchKernelGGL(k_issue_req_out, dim3((m * 8 + 255) / 256), dim3(256), 0, sl.stream, a.rec_out, sl.d_status, d_req, m);
      if ((rc = dev_out_end(c, sl, mem, out_req + off * 128, d_req, (size_t)m * 128))) return rc;
    }
    if (sign) {
      uint8_t* d_out; const uint8_t* d_rng;
      if ((rc = dev_out_begin(c, sl, 2, mem, out_resp + off * rl, (size_t)m * rl, &d_out))) return rc;
      if ((rc = prepare_rng_slots(c, sl, m, off, mem, rng, ACT_RNG_PER_LANE, &cursor, &d_rng))) return rc;
      if ((rc = sign_phase(c, sl, m, LABEL_RESPOND, d_rng, a.c_amount, d_out, &fo))) return rc;
      if ((rc = dev_out_end(c, sl, mem, out_resp + off * rl, d_out, (size_t)m * rl))) return rc;
    }
    if ((rc = copy_status_out(c, sl, mem, status + off, m))) return rc;
  }
  return sync_all(c);
}

// The signature half from records (what act_issue_sign_batch does, sign_only_batch in engine.hip) with phase B framing the messages.
// The caller holds the context; rng is bytes (ACT_RNG_CALLBACK resolved by the caller).
int issue_sign_frame_locked(act_ctx* c, size_t n, int mem, const IssueWire& w, const uint8_t* req, const uint8_t* camt, const uint8_t* status_in,
                            const uint8_t* rng, int rng_mode, uint8_t* out_resp, uint8_t* status) {
  const size_t rl = w.resp.lay.tmpl.size();
  const FrameOut fo{w.resp.tmpl, w.resp.pay_off, (uint32_t)rl};
  size_t cursor = 0, chunk = 0; int rc;
  for (size_t off = 0; off < n; off += c->max_batch, chunk++) {
    Slot& sl = c->slots[chunk % c->depth];
    if (chunk >= (size_t)c->depth) { HIPCK(c, hipStreamSynchronize(sl.stream)); if ((rc = prof_collect(c, sl))) return rc; }
    const uint32_t m = (uint32_t)std::min(c->max_batch, n - off);
    SignXaArgs x{}; x.P = c->P; x.n = m; x.point_stride = 128; x.xa = sl.d_xa; x.status = sl.d_status;
    if ((rc = dev_in(c, sl, 0, mem, req + off * 128, (size_t)m * 128, &x.point))) return rc;
    if ((rc = dev_in(c, sl, 1, mem, camt + off * 32, (size_t)m * 32, &x.c_amount))) return rc;
    HIPCK(c, hipMemcpyAsync(sl.d_status, status_in + off, m, mem == ACT_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, sl.stream));
    uint8_t* d_out; const uint8_t* d_rng;
    if ((rc = dev_out_begin(c, sl, 2, mem, out_resp + off * rl, (size_t)m * rl, &d_out))) return rc;
    launch_sign_xa(x, sl.stream);
    if ((rc = prepare_rng_slots(c, sl, m, off, mem, rng, rng_mode, &cursor, &d_rng))) return rc;
    if ((rc = sign_phase(c, sl, m, LABEL_RESPOND, d_rng, x.c_amount, d_out, &fo))) return rc;
    if ((rc = dev_out_end(c, sl, mem, out_resp + off * rl, d_out, (size_t)m * rl))) return rc;
    if ((rc = copy_status_out(c, sl, mem, status + off, m))) return rc;
  }
  return sync_all(c);
}

// issue_wire_settle runs between calls, with no lock held (its small calls take the context themselves): the locking forms of the
// window and of the lane patch (wire_window_read, wire_patch_lanes: cbor_impl.inc).  They are defined here, behind the spend path,
// which runs with the context held and must not see them.
int window_read_locked(act_ctx* c, const CborType& T, const WireExtent& x, int mem, const size_t* which, size_t cnt, WireWindow& w) {
  std::lock_guard<std::mutex> lk(c->mu);
  HIPCK(c, hipSetDevice(c->device));
  return wire_window_read(c, c->slots[0].stream, T, x, mem == ACT_MEM_DEVICE, which, cnt, 128, w);
}
int patch_lanes(act_ctx* c, int mem, uint8_t* base, size_t stride, const size_t* lanes, size_t cnt, const uint8_t* vals) {
  std::lock_guard<std::mutex> lk(c->mu);
  HIPCK(c, hipSetDevice(c->device));
  return wire_patch_lanes(c, mem, base, stride, lanes, cnt, vals);
}
// `bytes` of caller memory at p (host or device) into dst
int read_caller(act_ctx* c, int mem, const uint8_t* p, size_t bytes, uint8_t* dst) {
  if (!bytes) return ACT_OK;
  if (mem == ACT_MEM_HOST) { memcpy(dst, p, bytes); return ACT_OK; }
  std::lock_guard<std::mutex> lk(c->mu);
  HIPCK(c, hipSetDevice(c->device));
  HIPCK(c, hipMemcpy(dst, p, bytes, hipMemcpyDeviceToHost));
  return ACT_OK;
}

// Settling the messages the pipeline flagged, after it has drained (no lock held: the small calls take it themselves).  A window is
// read by the spend path's window (its own messages only, the codes ordered as from_cbor does); here the records that read are checked
// in one small act_issue_check_batch and the window's lanes of status / out_req patched.  With `sk` (the whole endpoint,
// ACT_RNG_PER_LANE) the accepted ones are also signed from their own rng slices and framed into out_resp.
int issue_wire_settle(act_ctx* c, int mem, const IssueWire& w, const std::vector<size_t>& which, const uint8_t sk[64], const uint8_t* camt,
                      const uint8_t* rng, uint8_t* out_resp, uint8_t* status, uint8_t* out_req) {
  const CborType* T = cbor_type(ACT_CBOR_ISSUANCE_REQUEST);
  const CborLayout rlay = cbor_layout(*cbor_type(ACT_CBOR_ISSUANCE_RESPONSE), c->L);
  const size_t rl = rlay.tmpl.size();
  const WireExtent x{w.cbor, w.offsets, w.ml};
  WireWindow win;
  int rc;
  for (size_t w0 = 0; w0 < which.size(); w0 += WIRE_SETTLE_WINDOW) {
    const size_t cnt = std::min(which.size(), w0 + WIRE_SETTLE_WINDOW) - w0;
    const size_t* lanes = which.data() + w0;
    if ((rc = window_read_locked(c, *T, x, mem, lanes, cnt, win))) return rc;
    std::vector<uint8_t>& recs = win.recs;
    std::vector<uint8_t> good_recs; std::vector<size_t> good;
    for (size_t k = 0; k < cnt; k++) {
      if (win.codes[k] != CBOR_OK) continue;
      for (int f = 1; f < 4; f++) store_sc(recs.data() + k * 128 + 32 * f, load_sc(recs.data() + k * 128 + 32 * f));      // decode_scalar
      good.push_back(k);
      good_recs.insert(good_recs.end(), recs.data() + k * 128, recs.data() + (k + 1) * 128);
    }
    std::vector<uint8_t> verdict(win.status), st(good.size()), resp(cnt * rl, 0);
    if (!good.empty()) {
      if ((rc = act_issue_check_batch(c, good.size(), ACT_MEM_HOST, good_recs.data(), st.data()))) return rc;
      for (size_t g = 0; g < good.size(); g++) verdict[good[g]] = st[g];
      if (sk) {
        // the accepted ones: their amounts and (per-lane) rng slices, signed as records, framed here
        std::vector<size_t> acc;
        for (size_t g = 0; g < good.size(); g++) if (st[g] == 0) acc.push_back(g);
        if (!acc.empty()) {
          act::DrawnRng slices;                                   // (a container that wipes itself: the slices are signing-nonce seeds)
          std::vector<uint8_t> r2(acc.size() * 128), cam(acc.size() * 32), st_in(acc.size(), 0), st2(acc.size()), rec2(acc.size() * 160);
          slices.buf.assign(acc.size() * 128, 0);
          for (size_t j = 0; j < acc.size(); j++) {
            const size_t k = good[acc[j]], i = lanes[k];
            memcpy(r2.data() + j * 128, recs.data() + k * 128, 128);
            if ((rc = read_caller(c, mem, camt + i * 32, 32, cam.data() + j * 32))) return rc;
            if ((rc = read_caller(c, mem, rng + i * 128, 128, slices.buf.data() + j * 128))) return rc;
          }
          rc = act_issue_sign_batch(c, acc.size(), ACT_MEM_HOST, sk, r2.data(), cam.data(), st_in.data(), slices.buf.data(), ACT_RNG_PER_LANE, rec2.data(), st2.data());
          if (rc) return rc;
          for (size_t j = 0; j < acc.size(); j++) {
            const size_t k = good[acc[j]];
            verdict[k] = st2[j];
            if (st2[j]) continue;
            uint8_t* dst = resp.data() + k * rl;
            memcpy(dst, rlay.tmpl.data(), rl);
            for (size_t f = 0; f < rlay.pay_off.size(); f++) memcpy(dst + rlay.pay_off[f], rec2.data() + j * 160 + 32 * f, 32);
          }
        }
      }
    }
    for (size_t k = 0; k < cnt; k++) if (verdict[k]) { memset(recs.data() + k * 128, 0, 128); memset(resp.data() + k * rl, 0, rl); }
    if ((rc = patch_lanes(c, mem, status, 1, lanes, cnt, verdict.data()))) return rc;
    if (out_req && (rc = patch_lanes(c, mem, out_req, 128, lanes, cnt, recs.data()))) return rc;
    if (sk && (rc = patch_lanes(c, mem, out_resp, rl, lanes, cnt, resp.data()))) return rc;
  }
  return ACT_OK;
}

// the lanes whose wire flag says "not canonical" (read back after the pipeline; the caller holds the context)
int flagged_lanes(act_ctx* c, size_t n, std::vector<size_t>& which) {
  std::vector<uint8_t> flags(n);
  HIPCK(c, hipMemcpy(flags.data(), c->d_wire_flags, n, hipMemcpyDeviceToHost));
  which.clear();
  for (size_t i = 0; i < n; i++) if (flags[i] & 0x80) which.push_back(i);
  return ACT_OK;
}

// how many lanes the flag pass marked (the device reader's road: only the count is wanted, for act_ctx_wire_stats)
int flagged_count(act_ctx* c, size_t n, size_t* count) {
  std::vector<uint8_t> flags(n);
  HIPCK(c, hipMemcpy(flags.data(), c->d_wire_flags, n, hipMemcpyDeviceToHost));
  size_t k = 0;
  for (size_t i = 0; i < n; i++) k += flags[i] >> 7;
  *count = k;
  return ACT_OK;
}

int check_offsets(size_t n, const uint64_t* offsets) {
  if (n >= ((size_t)1 << 32)) return ACT_ERR_ARG;
  if (offsets) for (size_t i = 0; i < n; i++) if (offsets[i + 1] < offsets[i]) return ACT_ERR_ARG;     // message i = [offsets[i], offsets[i+1])
  return ACT_OK;
}

// the check half (and, with sk and ACT_RNG_PER_LANE bytes, the whole endpoint in one pipeline).  Device reader: the pipeline is the whole
// call.  Host reader: the flagged lanes are settled behind it.
int issue_wire_run(act_ctx* c, size_t n, int mem, const uint8_t sk[64], const uint8_t* cbor, const uint64_t* offsets, const uint8_t* camt,
                   const uint8_t* rng, uint8_t* out_resp, uint8_t* status, uint8_t* out_req) {
  IssueWire w; w.cbor = cbor; w.offsets = offsets;
  std::vector<size_t> which;
  {
    Call call(c, n);
    HIPCK(c, hipSetDevice(c->device));
    int rc;
    const bool dev_reader = c->wire_reader.load() == ACT_WIRE_READER_DEVICE;
    if (sk && (rc = set_key(c, sk))) return rc;
    if ((rc = issue_wire_prepare(c, w, true, sk != nullptr))) return rc;
    if (dev_reader && (rc = wire_codes_reserve(c, n))) return rc;
    if ((rc = wire_flags_reserve(c, n))) return rc;
    if ((rc = issue_wire_pipeline(c, n, mem, w, camt, rng, sk != nullptr, dev_reader, out_resp, status, out_req))) return rc;
    if (dev_reader) {
      size_t read = 0;
      if ((rc = flagged_count(c, n, &read))) return rc;
      c->wire_stats[0] += n; c->wire_stats[1] += n - read; c->wire_stats[2] += read;
      return call.finish();
    }
    if ((rc = flagged_lanes(c, n, which))) return rc;
    c->wire_stats[0] += n; c->wire_stats[1] += n - which.size(); c->wire_stats[3] += which.size();
    if ((rc = call.finish())) return rc;
  }
  return issue_wire_settle(c, mem, w, which, sk, camt, rng, out_resp, status, out_req);
}

// the sign half: rng resolved (ACT_RNG_CALLBACK: one draw for the accepted lanes), then the framed signature
int issue_sign_cbor_impl(act_ctx* c, size_t n, int mem, const uint8_t sk[64], const uint8_t* req, const uint8_t* camt, const uint8_t* status_in,
                         const uint8_t* rng, int rng_mode, uint8_t* out_resp_cbor, uint8_t* status) {
  const size_t rl = act_cbor_size(c, ACT_CBOR_ISSUANCE_RESPONSE);
  ResolvedRng rr(c);
  int rc = rr.resolve(c, mem, status_in, n, rng, rng_mode);
  if (rc) {
    if (rc == ACT_ERR_RNG) {                                      // nothing signed: every slot zero
      if (mem == ACT_MEM_HOST) memset(out_resp_cbor, 0, n * rl);
      else { std::lock_guard<std::mutex> lk(c->mu); HIPCK(c, hipSetDevice(c->device)); HIPCK(c, hipMemset(out_resp_cbor, 0, n * rl)); }
      c->err = "ACT_RNG_CALLBACK: the caller's generator failed; nothing was signed";
    }
    return rc;
  }
  Call call(c, n);
  HIPCK(c, hipSetDevice(c->device));
  if ((rc = set_key(c, sk))) return rc;
  IssueWire w;
  if ((rc = issue_wire_prepare(c, w, false, true))) return rc;
  if ((rc = issue_sign_frame_locked(c, n, mem, w, req, camt, status_in, rng, rng_mode, out_resp_cbor, status))) return rc;
  return call.finish();
}

// The tiny road (host memory, at most TINY_MAX messages, per-lane rng or one message): unframed here -- template compare and payload copy;
// the kernel decodes K and reduces the scalars --, then act_issue_batch's one-kernel form (issue_tiny: k_sign_fused<true>), framed here.
// TINY_NEEDS_GENERAL_PATH when a message is not the canonical encoding: nothing has been written.
int issue_cbor_tiny(act_ctx* c, size_t n, const uint8_t sk[64], const uint8_t* cbor, const uint64_t* offsets, const uint8_t* camt,
                    const uint8_t* rng, int rng_mode, uint8_t* out_resp_cbor, uint8_t* status) {
  const CborLayout q = cbor_layout(*cbor_type(ACT_CBOR_ISSUANCE_REQUEST), c->L);
  const size_t ml = q.tmpl.size();
  std::vector<uint8_t> recs(n * 128), resp(n * 160), st(n);
  for (size_t i = 0; i < n; i++) {
    const size_t beg = offsets ? (size_t)offsets[i] : i * ml, end = offsets ? (size_t)offsets[i + 1] : beg + ml;
    if (end - beg < ml) return TINY_NEEDS_GENERAL_PATH;
    const uint8_t* src = cbor + beg;
    for (size_t f = 0, prev = 0; f < q.pay_off.size(); prev = q.pay_off[f] + 32, f++) {
      if (memcmp(src + prev, q.tmpl.data() + prev, q.pay_off[f] - prev)) return TINY_NEEDS_GENERAL_PATH;
      memcpy(recs.data() + i * 128 + 32 * f, src + q.pay_off[f], 32);
    }
  }
  const int rc = act_issue_batch(c, n, ACT_MEM_HOST, sk, recs.data(), camt, rng, rng_mode, resp.data(), st.data());
  if (rc) return rc;
  cbor_frame_refunds_host(cbor_layout(*cbor_type(ACT_CBOR_ISSUANCE_RESPONSE), c->L), n, resp.data(), st.data(), out_resp_cbor);
  memcpy(status, st.data(), n);
  c->wire_stats[0] += n; c->wire_stats[1] += n;                  // (every message of a call that ends here is canonical)
  return ACT_OK;
}

}  // namespace

extern "C" {

int act_issue_check_cbor_batch(act_ctx* c, size_t n, int mem, const uint8_t* cbor, const uint64_t* offsets, uint8_t* status, uint8_t* out_req) {
  if (!c || (n && (!cbor || !status))) return ACT_ERR_ARG;
  if (check_offsets(n, offsets)) return ACT_ERR_ARG;
  if (n == 0) return ACT_OK;
  return issue_wire_run(c, n, mem, nullptr, cbor, offsets, nullptr, nullptr, nullptr, status, out_req);
}

int act_issue_sign_cbor_batch(act_ctx* c, size_t n, int mem, const uint8_t sk[64], const uint8_t* req, const uint8_t* camt, const uint8_t* status_in,
                              const uint8_t* rng, int rng_mode, uint8_t* out_resp_cbor, uint8_t* status) {
  if (!c || !sk || !rng || (n && (!req || !camt || !status_in || !out_resp_cbor || !status))) return ACT_ERR_ARG;
  if (rng_mode != ACT_RNG_PER_LANE && rng_mode != ACT_RNG_SEQUENTIAL && rng_mode != ACT_RNG_CALLBACK) return ACT_ERR_ARG;
  if (n == 0) return ACT_OK;
  return issue_sign_cbor_impl(c, n, mem, sk, req, camt, status_in, rng, rng_mode, out_resp_cbor, status);
}

int act_issue_cbor_batch(act_ctx* c, size_t n, int mem, const uint8_t sk[64], const uint8_t* cbor, const uint64_t* offsets, const uint8_t* camt,
                         const uint8_t* rng, int rng_mode, uint8_t* out_resp_cbor, uint8_t* status) {
  if (!c || !sk || !rng || (n && (!cbor || !camt || !out_resp_cbor || !status))) return ACT_ERR_ARG;
  if (rng_mode != ACT_RNG_PER_LANE && rng_mode != ACT_RNG_SEQUENTIAL && rng_mode != ACT_RNG_CALLBACK) return ACT_ERR_ARG;
  if (check_offsets(n, offsets)) return ACT_ERR_ARG;
  if (n == 0) return ACT_OK;
  if (mem == ACT_MEM_HOST && n <= TINY_MAX && n <= c->max_batch && tiny_enabled(c) && (rng_mode == ACT_RNG_PER_LANE || (rng_mode == ACT_RNG_SEQUENTIAL && n == 1))) {
    const int rc = issue_cbor_tiny(c, n, sk, cbor, offsets, camt, rng, rng_mode, out_resp_cbor, status);
    if (rc != TINY_NEEDS_GENERAL_PATH) return rc;
  }
  // per-lane slices depend on no verdict: one pipeline signs as it checks
  if (rng_mode == ACT_RNG_PER_LANE) return issue_wire_run(c, n, mem, sk, cbor, offsets, camt, rng, out_resp_cbor, status, nullptr);
  // SEQUENTIAL / CALLBACK: a lane's slice is the number of accepted lanes in front of it, so every verdict -- the settled ones included --
  // is known before anything is signed: the check half with the records kept, then the sign half
  std::vector<uint8_t> h_req, h_st; DevTmp d(c);
  uint8_t *req, *st;
  int rc;
  if (mem == ACT_MEM_DEVICE) { if ((rc = d.alloc(n * 129))) return rc; req = d.p; st = d.p + n * 128; }
  else { h_req.resize(n * 128); h_st.resize(n); req = h_req.data(); st = h_st.data(); }
  if ((rc = issue_wire_run(c, n, mem, nullptr, cbor, offsets, nullptr, nullptr, nullptr, st, req))) return rc;
  rc = issue_sign_cbor_impl(c, n, mem, sk, req, camt, st, rng, rng_mode, out_resp_cbor, status);
  if (rc == ACT_ERR_RNG) {                                        // the verdicts stand; nothing was signed
    if (mem == ACT_MEM_HOST) memcpy(status, st, n);
    else { std::lock_guard<std::mutex> lk(c->mu); HIPCK(c, hipSetDevice(c->device)); HIPCK(c, hipMemcpy(status, st, n, hipMemcpyDeviceToDevice)); }
    c->err = "ACT_RNG_CALLBACK: the caller's generator failed; nothing was signed";
  }
  return rc;
}

}  // extern "C"
