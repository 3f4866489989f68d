// reserve_impl.inc — included by engine.hip behind admit_replay_impl.inc: reserve and settle (DESIGN 4.11; kernels in k_reserve.hip, lane
// bodies in reserve_lanes.h).  A metered service records a spend of s, does the work, and signs the partial refund t <= s afterwards.
//   reserve   act_redeem_(cbor_)reserve_batch: the admit-replay driver (redeem_admit, AdmitCall::reserves) with tag_res where the receipt's
//             tag is and with the replay tail's signature half switched off (replay_tail's `res`): screen, candidate stage, verification,
//             check-and-insert of k, tag_res into the receipts, and where the tail signs the 96-byte reservation records are written.
//             Nothing secret beyond the ring is staged.
//   settle    act_redeem_(cbor_)settle_batch, over ONE set (the receipts), whose lock every step takes once for itself:
//               prep          per lane the three reductions, the key-index rule, t^ > s^, tag_res / marker / amount tag   [k_settle_prep]
//               reservation   tag_res looked up, read only; absent: ACT_STATUS_NOT_RESERVED                               [k_settle_found]
//               the pin       check-and-insert of the marker under the matched key's epoch; the amount tag recorded where the marker was
//                             fresh, looked up where it was spent (replay_resolve, with the marker where the nullifier is); a spent marker
//                             without this amount's tag: ACT_STATUS_SETTLED_OTHER_AMOUNT                                  [k_settle_merge]
//               signature     the key each lane is signed with, the derived nonces of (nonce_key, key, k^, enc(K'), t^) in the context's
//                             replay buffer, the ring signing step with amounts (ring_sign_step)
// Device-memory callers: kernels; host-memory callers: the same lane bodies on the host workers.  The replay buffer is wiped on every exit.
namespace {

struct ReserveTagJob { ReplayDeriveArgs a; };
struct ReserveEmitJob { ReserveEmitArgs a; };
struct SettlePrepJob { SettlePrepArgs a; };

void settle_counts_of(uint64_t* out_counts, size_t n, const uint8_t* status, const uint8_t* before) {
  uint64_t k[ACT_SETTLE_COUNTS] = {n, 0, 0, 0, 0, 0, 0};      // lanes, not_reserved, return_too_big, settled, settled_again, other_amount, unanswered
  for (size_t i = 0; i < n; i++) {
    const uint8_t s = status[i];
    if (s == 0) k[before[i] ? 4 : 3]++;
    else if (s == ACT_STATUS_NOT_RESERVED) k[1]++;
    else if (s == ACT_STATUS_RETURN_TOO_BIG) k[2]++;
    else if (s == ACT_STATUS_SETTLED_OTHER_AMOUNT) k[5]++;
    else k[6]++;
  }
  memcpy(out_counts, k, sizeof(k));
}

}  // namespace

// ---- reserve: what replay_tail calls where the replay forms derive their tag and sign -------------------------------------------------
static void reserve_tags_host(const ReplayDeriveArgs& a) {
  ReserveTagJob job{a};
  act_host_parallel_for(a.n, 256, 0, [](void* p, size_t i0, size_t i1) {
    const ReplayDeriveArgs& a = static_cast<ReserveTagJob*>(p)->a;
    for (size_t i = i0; i < i1; i++) reserve_tag_lane(a, (uint32_t)i);
  }, &job);
}
static int reserve_emit(act_ctx* c, hipStream_t stream, size_t n, int mem, const uint8_t* k_at, size_t k_stride, const uint8_t* kp, const uint8_t* s, const uint8_t* st,
                        uint8_t* out, uint8_t* status) {
  ReserveEmitJob job{ReserveEmitArgs{(uint32_t)n, (uint32_t)k_stride, k_at, kp, s, st, out, status}};
  if (mem == ACT_MEM_DEVICE) {
    RPCK(c, hipSetDevice(c->device));
    launch_reserve_emit(job.a, stream);
    RPCK(c, hipGetLastError());
    RPCK(c, hipStreamSynchronize(stream));
    return ACT_OK;
  }
  act_host_parallel_for(n, 256, 0, [](void* p, size_t i0, size_t i1) {
    const ReserveEmitArgs& a = static_cast<ReserveEmitJob*>(p)->a;
    for (size_t i = i0; i < i1; i++) reserve_emit_lane(a, (uint32_t)i);
  }, &job);
  return ACT_OK;
}

extern "C" int act_redeem_reserve_batch(act_ctx* c, act_nullifier_set* set, act_nullifier_set* receipts, size_t n, int mem, const uint8_t* keys, int nkeys,
                                        const uint32_t* key_epochs, const uint8_t* proof, const uint8_t* charge, uint8_t* out_reservation, uint8_t* status,
                                        uint8_t* out_key, uint8_t* out_replayed, uint64_t* out_counts) {
  if (n && !proof) return ACT_ERR_ARG;
  return redeem_admit(AdmitCall(c, set, n, mem).ring(keys, nkeys, key_epochs, ACT_SIGN_MATCHED).records(proof).charged(charge).reserves(receipts, out_replayed)
                          .answers(out_reservation, status, out_key, out_counts));
}
extern "C" int act_redeem_cbor_reserve_batch(act_ctx* c, act_nullifier_set* set, act_nullifier_set* receipts, size_t n, int mem, const uint8_t* keys, int nkeys,
                                             const uint32_t* key_epochs, const uint8_t* cbor, const uint64_t* offsets, const uint8_t* charge, uint8_t* out_reservation,
                                             uint8_t* status, uint8_t* out_key, uint8_t* out_replayed, uint64_t* out_counts) {
  if (n && !cbor) return ACT_ERR_ARG;
  return redeem_admit(AdmitCall(c, set, n, mem).ring(keys, nkeys, key_epochs, ACT_SIGN_MATCHED).messages(cbor, offsets).charged(charge).reserves(receipts, out_replayed)
                          .answers(out_reservation, status, out_key, out_counts));
}

// request binding (DESIGN 4.12): reserve with n * 32 bytes of associated data in every verified lane's challenge hash; bind == NULL is the
// call above.  A recorded reservation's proof resent under another binding is an invalid proof, not a replay.  Settle takes no binding
extern "C" int act_redeem_reserve_bound_batch(act_ctx* c, act_nullifier_set* set, act_nullifier_set* receipts, size_t n, int mem, const uint8_t* keys, int nkeys,
                                              const uint32_t* key_epochs, const uint8_t* proof, const uint8_t* bind, const uint8_t* charge, uint8_t* out_reservation,
                                              uint8_t* status, uint8_t* out_key, uint8_t* out_replayed, uint64_t* out_counts) {
  if (n && !proof) return ACT_ERR_ARG;
  return redeem_admit(AdmitCall(c, set, n, mem).ring(keys, nkeys, key_epochs, ACT_SIGN_MATCHED).records(proof).bound(bind).charged(charge).reserves(receipts, out_replayed)
                          .answers(out_reservation, status, out_key, out_counts));
}
extern "C" int act_redeem_cbor_reserve_bound_batch(act_ctx* c, act_nullifier_set* set, act_nullifier_set* receipts, size_t n, int mem, const uint8_t* keys, int nkeys,
                                                   const uint32_t* key_epochs, const uint8_t* cbor, const uint64_t* offsets, const uint8_t* bind, const uint8_t* charge,
                                                   uint8_t* out_reservation, uint8_t* status, uint8_t* out_key, uint8_t* out_replayed, uint64_t* out_counts) {
  if (n && !cbor) return ACT_ERR_ARG;
  return redeem_admit(AdmitCall(c, set, n, mem).ring(keys, nkeys, key_epochs, ACT_SIGN_MATCHED).messages(cbor, offsets).bound(bind).charged(charge).reserves(receipts, out_replayed)
                          .answers(out_reservation, status, out_key, out_counts));
}

// ---- settle -----------------------------------------------------------------------------------------------------------------------------
// Everything settle refuses as a whole: replay_refused's rules against ONE set, under one hold of its lock, with room for 2 n keys
static int settle_refused(act_ctx* c, act_nullifier_set* receipts, size_t n, int mem, const uint8_t* keys, int nkeys, const uint32_t* key_epochs, int sign_key,
                          const uint8_t* reservation, const uint8_t* key_index, const uint8_t* nonce_key, const uint8_t* out, const uint8_t* status) {
  if (!c || !receipts || !keys || !nonce_key || nkeys < 1 || nkeys > ACT_KEYRING_MAX || (mem != ACT_MEM_HOST && mem != ACT_MEM_DEVICE) || n > ((size_t)1 << 30)) return ACT_ERR_ARG;
  if (sign_key != ACT_SIGN_MATCHED && (sign_key < 0 || sign_key >= nkeys)) return ACT_ERR_ARG;
  if (n && (!reservation || !key_index || !out || !status)) return ACT_ERR_ARG;
  if (receipts->device != c->device) { c->err = "act_redeem_settle_batch: the receipts set lives on another device"; return ACT_ERR_ARG; }
  std::lock_guard<std::mutex> lk(receipts->mu);
  if (key_epochs) {
    const std::string why = null_epochs_refused(receipts, key_epochs, nkeys);
    if (!why.empty()) { c->err = "act_redeem_settle_batch: the receipts set: " + why; return ACT_ERR_ARG; }
  }
  if (receipts->len + 2 * n > receipts->tab_cap / 2) {
    c->err = "act_redeem_settle_batch: the receipts set has no room for " + std::to_string(2 * n) + " more keys (act_nullifier_set_reserve)";
    return ACT_ERR_ARG;
  }
  return ACT_OK;
}

static int redeem_settle_impl(act_ctx* c, act_nullifier_set* receipts, size_t n, int mem, const uint8_t* keys, int nkeys, const uint32_t* key_epochs, int sign_key,
                              const uint8_t* reservation, const uint8_t* key_index, const uint8_t* amounts, const uint8_t* nonce_key, bool wire, uint8_t* out,
                              uint8_t* status, uint8_t* out_settled_before, uint64_t* out_counts) {
  if (out_counts) memset(out_counts, 0, sizeof(uint64_t) * ACT_SETTLE_COUNTS);
  if (int bad = settle_refused(c, receipts, n, mem, keys, nkeys, key_epochs, sign_key, reservation, key_index, nonce_key, out, status)) return bad;
  // a ring whose w does not decode fails the call before anything is recorded (the empty ring call, as in the admission calls)
  static const uint8_t derived = 0;
  if (int bad = redeem_keyring_impl(c, receipts, 0, mem, keys, nkeys, key_epochs, sign_key, nullptr, nullptr, nullptr, &derived, ACT_RNG_PER_LANE, nullptr, nullptr, nullptr)) return bad;
  if (n == 0) return ACT_OK;
  // one replay call at a time per context: the staged secrets and the derived nonces live in the context's own buffer (d_replay)
  std::lock_guard<std::mutex> replay(c->replay_mu);
  const bool dev = mem == ACT_MEM_DEVICE;
  const RedeemReturn ret{amounts};
  const size_t out_b = redeem_out_bytes(c, wire, &ret);
  // the three tags and enc(K') as dense arrays; statuses, the receipts' answers, masks, the signing keys, the marks
  const size_t per_lane = 4 * 32 + 9;
  std::vector<uint8_t> h; DevTmp d(c);
  uint8_t* base; int rc;
  if (dev) { if ((rc = d.alloc(n * per_lane))) return rc; base = d.p; }
  else { h.resize(n * per_lane); base = h.data(); }
  uint8_t *tag_res = base, *marker = tag_res + n * 32, *tag_amt = marker + n * 32, *kp = tag_amt + n * 32, *st = kp + n * 32, *found = st + n, *spent = found + n,
          *skip = spent + n, *sp = skip + n, *r_ans = sp + n, *found_amt = r_ans + n, *kidx = found_amt + n,
          *before = out_settled_before ? out_settled_before : kidx + n;

  ReplaySecretsDev sec_dev(c); ReplaySecretsHost sec_host;
  const uint8_t* secrets;
  if (dev) { if ((rc = sec_dev.stage(n * 128, nonce_key, keys, nkeys))) return rc; secrets = c->d_replay; }
  else { sec_host.stage(n * 128, nonce_key, keys, nkeys); secrets = sec_host.p.get(); }
  uint8_t* const nonces = const_cast<uint8_t*>(secrets) + REPLAY_NONCE_OFF;

  hipStream_t stream = receipts->stream;
  // ---- prep: rules 1 and 2 and the tags, then the reservation's look-up (read only) ------------------------------------------------------------------
  SettlePrepJob pj{SettlePrepArgs{(uint32_t)n, (uint32_t)nkeys, reservation, key_index, amounts, tag_res, marker, tag_amt, kp, st}};
  if (dev) {
    RPCK(c, hipSetDevice(c->device));
    launch_settle_prep(pj.a, stream);
    RPCK(c, hipGetLastError());
    RPCK(c, hipMemsetAsync(found, 0, n, stream)); RPCK(c, hipMemsetAsync(found_amt, 0, n, stream)); RPCK(c, hipMemsetAsync(before, 0, n, stream));
    RPCK(c, hipStreamSynchronize(stream));
  } else {
    act_host_parallel_for(n, 256, 0, [](void* p, size_t i0, size_t i1) {
      const SettlePrepArgs& a = static_cast<SettlePrepJob*>(p)->a;
      for (size_t i = i0; i < i1; i++) settle_prep_lane(a, (uint32_t)i);
    }, &pj);
    memset(found, 0, n); memset(found_amt, 0, n); memset(before, 0, n);
  }
  if ((rc = act_nullifier_contains_batch(receipts, n, mem, tag_res, 32, found))) {      // nothing recorded, status untouched
    c->err = std::string("act_redeem_settle_batch: receipts set: ") + act_nullifier_set_last_error(receipts);
    return rc;
  }
  const SettleFoundArgs fa{(uint32_t)n, found, st};
  if (dev) { launch_settle_found(fa, stream); RPCK(c, hipGetLastError()); RPCK(c, hipStreamSynchronize(stream)); }
  else for (size_t i = 0; i < n; i++) settle_found_lane(fa, (uint32_t)i);

  // a step failed as a whole: every lane that was to be answered says `what`, the others their status, and there is no output
  auto give_up = [&](uint8_t what, void (*k_mark)(uint8_t*, const uint8_t*, uint32_t)) {
    if (!dev) { for (size_t i = 0; i < n; i++) status[i] = st[i] ? st[i] : what; memset(out, 0, n * out_b); return; }
    std::lock_guard<std::mutex> lk(c->mu);
    (void)hipSetDevice(c->device);
    hipLaunchKernelGGL(k_mark, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, status, st, (uint32_t)n);
    (void)hipMemsetAsync(out, 0, n * out_b, nullptr);
    if (hipDeviceSynchronize() != hipSuccess) (void)hipGetLastError();
  };
  auto counts = [&] {      // status[] is complete from here on, whatever fails
    if (!out_counts) return;
    std::vector<uint8_t> hs;
    const uint8_t *s = status, *b = before;
    if (dev) {
      hs.resize(2 * n);
      std::lock_guard<std::mutex> lk(c->mu);
      if (hipSetDevice(c->device) != hipSuccess || hipMemcpy(hs.data(), status, n, hipMemcpyDeviceToHost) != hipSuccess ||
          hipMemcpy(hs.data() + n, before, n, hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return; }
      s = hs.data(); b = hs.data() + n;
    }
    settle_counts_of(out_counts, n, s, b);
  };

  // ---- the pin: the marker where the replay tail has the nullifier, the amount tag where it has the receipt -----------------------------------------
  int rc_mark = ACT_OK, rc_amt = ACT_OK; std::string pin_err;
  const int rc_pin = [&]() -> int {
    rc_mark = key_epochs ? act_nullifier_check_and_insert_epoch_batch(receipts, n, mem, marker, 32, st, key_index, key_epochs, nkeys, spent)
                         : act_nullifier_check_and_insert_batch(receipts, n, mem, marker, 32, st, spent);
    if (rc_mark) pin_err = std::string("receipts set: ") + act_nullifier_set_last_error(receipts);
    if (rc_mark == ACT_ERR_HIP) return rc_mark;
    ReplayResolveArgs ra{(uint32_t)n, st, spent, nullptr, skip, sp, before};
    if (dev) { launch_replay_resolve(ra, stream); RPCK(c, hipGetLastError()); RPCK(c, hipStreamSynchronize(stream)); }
    else for (size_t i = 0; i < n; i++) replay_resolve_lane(ra, (uint32_t)i);
    // the amount tag of every lane whose marker was fresh, under the marker's epoch; the answer is ignored (a tag that is there is harmless)
    rc_amt = key_epochs ? act_nullifier_check_and_insert_epoch_batch(receipts, n, mem, tag_amt, 32, skip, key_index, key_epochs, nkeys, r_ans)
                        : act_nullifier_check_and_insert_batch(receipts, n, mem, tag_amt, 32, skip, r_ans);
    // the others: is this the amount the reservation was settled with?  (Behind the insert: a lane settled by an earlier lane of this batch finds that lane's tag.)
    const int rc_found = act_nullifier_contains_batch(receipts, n, mem, tag_amt, 32, found_amt);
    if (!rc_amt) rc_amt = rc_found;
    if (rc_amt && pin_err.empty()) pin_err = std::string("receipts set: ") + act_nullifier_set_last_error(receipts);
    ra.found = found_amt;
    const SettleMergeArgs ma{(uint32_t)n, sp, st};
    if (dev) {
      launch_replay_resolve(ra, stream); launch_settle_merge(ma, stream);
      RPCK(c, hipGetLastError()); RPCK(c, hipStreamSynchronize(stream));
    } else for (size_t i = 0; i < n; i++) { replay_resolve_lane(ra, (uint32_t)i); settle_merge_lane(ma, (uint32_t)i); }
    return ACT_OK;
  }();
  if (rc_pin) {      // the device itself failed: no answer can be trusted, nothing is signed
    if (!pin_err.empty()) c->err = pin_err + " (every reserved lane is undetermined)";
    give_up(ACT_STATUS_NULLIFIER_UNDETERMINED, k_mark_undetermined_status);
    counts();
    return rc_pin;
  }

  // ---- the signature: the key every lane is signed with, its derived nonces, the ring signing step with amounts ---------------------------------------
  ReplayDeriveArgs na{}; na.n = (uint32_t)n; na.stride = RESERVATION_BYTES; na.nkeys = (uint32_t)nkeys; na.nul = reservation; na.kp = kp; na.st = st; na.kidx = kidx;
  na.secrets = secrets; na.out = nonces; na.t = amounts;
  int rc_sign = ACT_OK;
  if (dev) {
    std::lock_guard<std::mutex> lk(c->mu);
    (void)hipSetDevice(c->device);
    ring_sign_index(mem, kidx, key_index, sign_key, n);
    replay_derive_dev(na, true, nullptr);
    if (hipDeviceSynchronize() != hipSuccess) { c->err = "act_redeem_settle_batch: the nonce derivation failed"; (void)hipGetLastError(); rc_sign = ACT_ERR_HIP; }
  } else { ring_sign_index(mem, kidx, key_index, sign_key, n); replay_derive_host(na, true); }
  const bool fail_sign = c->debug_fail_signs.load() > 0 && c->debug_fail_signs.fetch_sub(1) > 0;      // error-path test hook (act_debug_fail_next_signs)
  if (!rc_sign) {
    if (fail_sign) { rc_sign = ACT_ERR_HIP; c->err = "act_debug_fail_next_signs: simulated failure of the signature step"; }
    else rc_sign = ring_sign_step(c, n, mem, keys, nkeys, wire, kidx, kp, st, nonces, ACT_RNG_PER_LANE, out, status, &ret);
  }
  if (rc_sign) {      // marker and amount tag ARE recorded: the refunds are owed, and the same call again hands them out
    give_up(ACT_STATUS_RECORDED_UNSIGNED, k_mark_recorded_unsigned);
    counts();
    return rc_sign;
  }
  counts();
  if (rc_mark || rc_amt) { c->err = pin_err + " (every signed refund was handed out; lanes the set could not answer are undetermined)"; return rc_mark ? rc_mark : rc_amt; }
  return ACT_OK;
}

extern "C" int act_redeem_settle_batch(act_ctx* c, act_nullifier_set* receipts, size_t n, int mem, const uint8_t* keys, int nkeys, const uint32_t* key_epochs, int sign_key,
                                       const uint8_t* reservation, const uint8_t* key_index, const uint8_t* amounts, const uint8_t nonce_key[32],
                                       uint8_t* out_refund_return, uint8_t* status, uint8_t* out_settled_before, uint64_t* out_counts) {
  return redeem_settle_impl(c, receipts, n, mem, keys, nkeys, key_epochs, sign_key, reservation, key_index, amounts, nonce_key, false, out_refund_return, status,
                            out_settled_before, out_counts);
}
extern "C" int act_redeem_cbor_settle_batch(act_ctx* c, act_nullifier_set* receipts, size_t n, int mem, const uint8_t* keys, int nkeys, const uint32_t* key_epochs,
                                            int sign_key, const uint8_t* reservation, const uint8_t* key_index, const uint8_t* amounts, const uint8_t nonce_key[32],
                                            uint8_t* out_refund_return_cbor, uint8_t* status, uint8_t* out_settled_before, uint64_t* out_counts) {
  return redeem_settle_impl(c, receipts, n, mem, keys, nkeys, key_epochs, sign_key, reservation, key_index, amounts, nonce_key, true, out_refund_return_cbor, status,
                            out_settled_before, out_counts);
}
