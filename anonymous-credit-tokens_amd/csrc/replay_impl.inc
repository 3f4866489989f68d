// replay_impl.inc — included by engine.hip behind keyring_redeem_impl.inc: replayable redemption (DESIGN 4.8; kernels in k_replay.hip,
// lane bodies in replay_lanes.h).  act_redeem_replay_batch / act_redeem_cbor_replay_batch are redeem_tail_ring's shape with their own
// steps handed to redeem_tail:
//   null step      check-and-insert of k into `set`; the tag of every verified lane; a receipt for the lanes whose k was fresh; a
//                  read-only look-up of the others' tags in `receipts` -> sp = 0 for fresh AND replayed lanes, 1 for a double spend
//   beside_merge   the key every lane is signed with, then the derived nonces of the lanes that are signed, into a buffer that the
//                  signing call reads as ACT_RNG_PER_LANE bytes in `mem` memory
//   sign step      the ring calls' own (ring_sign_step)
// Device-memory callers: kernels, the secrets in the context's d_replay; host-memory callers: the same lane bodies on the host workers
// into a host buffer.  Both are wiped on every exit.
namespace {

#define RPCK(c, expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { (c)->err = std::string("replay: ") + #expr + ": " + hipGetErrorString(e_); (void)hipGetLastError(); return ACT_ERR_HIP; } } while (0)

constexpr size_t REPLAY_NONCE_OFF = 512;      // d_replay: nonce_key | ring records (REPLAY_SECRET_BYTES), then the nonces, 128 bytes a lane

// the context's secret buffer of a device-memory replay call, wiped on every exit
struct ReplaySecretsDev {
  act_ctx* c; size_t dirty = 0;
  explicit ReplaySecretsDev(act_ctx* c_) : c(c_) {}
  int stage(size_t nonce_bytes, const uint8_t* nonce_key, const uint8_t* keys, int nkeys) {
    const size_t bytes = REPLAY_NONCE_OFF + nonce_bytes;
    std::lock_guard<std::mutex> lk(c->mu);
    RPCK(c, hipSetDevice(c->device));
    if (bytes > c->d_replay_cap) {
      if (c->d_replay) { RPCK(c, hipFree(c->d_replay)); c->d_replay = nullptr; c->d_replay_cap = 0; }      // (wiped when its call ended)
      RPCK(c, hipMalloc(&c->d_replay, bytes)); c->d_replay_cap = bytes;
      RPCK(c, hipMemset(c->d_replay, 0, bytes));
    }
    dirty = bytes;
    RPCK(c, hipMemcpy(c->d_replay, nonce_key, 32, hipMemcpyHostToDevice));
    RPCK(c, hipMemcpy(c->d_replay + 32, keys, (size_t)nkeys * 64, hipMemcpyHostToDevice));
    RPCK(c, hipDeviceSynchronize());      // (memset and copies run on the null stream; the kernels that read the buffer may not wait for that stream)
    return ACT_OK;
  }
  ~ReplaySecretsDev() { if (dirty && c->d_replay) { (void)hipSetDevice(c->device); if (hipMemset(c->d_replay, 0, dirty) != hipSuccess || hipDeviceSynchronize() != hipSuccess) (void)hipGetLastError(); } }
};

struct ReplayDeriveJob { ReplayDeriveArgs a; };
// the lane bodies on the host workers (host-memory callers)
void replay_derive_host(const ReplayDeriveArgs& a, bool nonce) {
  ReplayDeriveJob job{a};
  if (a.t && nonce) act_host_parallel_for(a.n, 256, 0, [](void* p, size_t i0, size_t i1) {      // the return forms: the lane's t in both hashes
    const ReplayDeriveArgs& a = static_cast<ReplayDeriveJob*>(p)->a;
    for (size_t i = i0; i < i1; i++) return_replay_nonce_lane(a, (uint32_t)i);
  }, &job);
  else if (a.t) act_host_parallel_for(a.n, 256, 0, [](void* p, size_t i0, size_t i1) {
    const ReplayDeriveArgs& a = static_cast<ReplayDeriveJob*>(p)->a;
    for (size_t i = i0; i < i1; i++) return_replay_tag_lane(a, (uint32_t)i);
  }, &job);
  else if (nonce) act_host_parallel_for(a.n, 256, 0, [](void* p, size_t i0, size_t i1) {
    const ReplayDeriveArgs& a = static_cast<ReplayDeriveJob*>(p)->a;
    for (size_t i = i0; i < i1; i++) replay_nonce_lane(a, (uint32_t)i);
  }, &job);
  else act_host_parallel_for(a.n, 256, 0, [](void* p, size_t i0, size_t i1) {
    const ReplayDeriveArgs& a = static_cast<ReplayDeriveJob*>(p)->a;
    for (size_t i = i0; i < i1; i++) replay_tag_lane(a, (uint32_t)i);
  }, &job);
}
// the kernels of k_replay.hip, or with amounts (a.t) those of k_return_replay.hip
void replay_derive_dev(const ReplayDeriveArgs& a, bool nonce, hipStream_t s) {
  if (a.t) { if (nonce) launch_return_replay_nonce(a, s); else launch_return_replay_tag(a, s); }
  else if (nonce) launch_replay_nonce(a, s); else launch_replay_tag(a, s);
}
// The same buffer for host-memory callers: nonce_key | ring records where the host lane body reads them (4-byte aligned: the
// allocation's own), then the nonces.  Not zero-filled (the lane body writes all 128 bytes of every lane) and wiped with
// explicit_bzero, not wipe_host's byte loop: 32 MB at 2^18 lanes (filled and wiped bytewise, records from host memory ran at 0.952
// of the plain call; so, 0.970: profiles/replay_probe.json).
struct ReplaySecretsHost {
  std::unique_ptr<uint8_t[]> p; size_t bytes = 0;
  void stage(size_t nonce_bytes, const uint8_t* nonce_key, const uint8_t* keys, int nkeys) {
    bytes = REPLAY_NONCE_OFF + nonce_bytes;
    p.reset(new uint8_t[bytes]);
    memset(p.get(), 0, REPLAY_NONCE_OFF);
    memcpy(p.get(), nonce_key, 32); memcpy(p.get() + 32, keys, (size_t)nkeys * 64);
  }
  ~ReplaySecretsHost() { if (p) explicit_bzero(p.get(), bytes); }
};

void replay_counts_of(uint64_t* out_counts, size_t n, const uint8_t* status, const uint8_t* replayed) {
  uint64_t k[ACT_REPLAY_COUNTS] = {n, 0, 0, 0, 0, 0};
  for (size_t i = 0; i < n; i++) {
    const uint8_t s = status[i];
    if (s == 0) k[replayed[i] ? 3 : 2]++;
    else if (s == ACT_STATUS_DOUBLE_SPEND) k[4]++;
    else if (s == ACT_STATUS_NULLIFIER_UNDETERMINED || s == ACT_STATUS_RECORDED_UNSIGNED) k[5]++;
    else k[1]++;
  }
  memcpy(out_counts, k, sizeof(k));
}

}  // namespace

// Everything the replay calls refuse as a whole on top of the ring redeem call's refusals: the receipts handle, nonce_key, the epoch table
// against the receipts set, and the receipts' room for n more keys.  (Also in front of the admission form, admit_replay_impl.inc.)
static int replay_refused(act_ctx* c, act_nullifier_set* set, act_nullifier_set* receipts, const uint8_t* nonce_key, size_t n, const uint32_t* key_epochs, int nkeys) {
  if (!receipts || !nonce_key || receipts == set) return ACT_ERR_ARG;
  if (receipts->device != c->device) { c->err = "act_redeem_replay_batch: the receipts set lives on another device"; return ACT_ERR_ARG; }
  std::lock_guard<std::mutex> lk(receipts->mu);
  if (key_epochs) {
    const std::string why = null_epochs_refused(receipts, key_epochs, nkeys);
    if (!why.empty()) { c->err = "act_redeem_replay_batch: the receipts set: " + why; return ACT_ERR_ARG; }
  }
  if (receipts->len + n > receipts->tab_cap / 2) {
    c->err = "act_redeem_replay_batch: the receipts set has no room for " + std::to_string(n) + " more keys (act_nullifier_set_reserve)";
    return ACT_ERR_ARG;
  }
  return ACT_OK;
}

// The replay tail: everything behind the verification, over dense arrays in `mem` memory -- the nullifiers at k_at + i * k_stride, enc(K')
// kp, the verdicts st (merged in place), the matched keys out_key.  Tags, both set steps, resolve, derived nonces, the sign step and the
// counts (ACT_REPLAY_COUNTS values, nullable).  The replay calls end in it over the caller's lanes, the admission form over its
// survivors.  The caller holds replay_mu.  began (nullable): set once nothing in front of the tail proper can fail any more -- a return
// with it unset has recorded nothing and written no status.  ret (act_redeem_(cbor_)return_replay_batch, DESIGN 4.10): the returned amounts
// lane for lane with the tail's arrays (ret->t null: every t = 0) -- they enter the tags, the nonces and the signing step, and the
// outputs are RefundReturn records or messages.  res (act_redeem_(cbor_)reserve_batch, DESIGN 4.11): the tail without its signature half --
// the receipt's tag is tag_res over the charges res->s (lane for lane with the tail's arrays), no secret is staged, no nonce derived, and
// where the sign step stands the 96-byte reservation records are written (reserve_impl.inc).
static int replay_tail(act_ctx* c, act_nullifier_set* set, act_nullifier_set* receipts, size_t n, int mem, const uint8_t* keys, int nkeys, const uint32_t* key_epochs,
                       int sign_key, bool wire, const uint8_t* k_at, size_t k_stride, const uint8_t* kp, uint8_t* st, const uint8_t* nonce_key, uint8_t* out,
                       uint8_t* status, uint8_t* out_key, uint8_t* out_replayed, uint64_t* out_counts, bool* began, const RedeemReturn* ret, const ReplayReserve* res) {
  const bool dev = mem == ACT_MEM_DEVICE;
  const uint8_t* const t = res ? res->s : ret ? ret->t : nullptr;
  // tags; merged answers, key indices, the two sets' answers, the receipts mask and its answers, the replay marks
  const size_t per_lane = 32 + 7;
  std::vector<uint8_t> h; DevTmp d(c);
  uint8_t* base; int rc;
  if (dev) { if ((rc = d.alloc(n * per_lane))) return rc; base = d.p; }
  else { h.resize(n * per_lane); base = h.data(); }
  uint8_t *tag = base, *sp = base + n * 32, *kidx = sp + n, *spent = kidx + n, *found = spent + n, *skip = found + n, *r_ans = skip + n,
          *repl = out_replayed ? out_replayed : r_ans + n;

  ReplaySecretsDev sec_dev(c); ReplaySecretsHost sec_host;
  static uint8_t unsigned_stand_in = 0;      // res: where the nonces stand (never read: nothing is signed)
  const uint8_t* secrets = nullptr; uint8_t* nonces = &unsigned_stand_in;
  if (!res) {
    if (dev) { if ((rc = sec_dev.stage(n * 128, nonce_key, keys, nkeys))) return rc; secrets = c->d_replay; }
    else { sec_host.stage(n * 128, nonce_key, keys, nkeys); secrets = sec_host.p.get(); }
    nonces = const_cast<uint8_t*>(secrets) + REPLAY_NONCE_OFF;
  }

  hipStream_t stream = set->stream;
  int rc_receipts = ACT_OK; std::string receipts_err;
  if (began) *began = true;      // from here on status[] is complete on return, whatever fails
  const int rc_tail = redeem_tail_sized(c, set, n, mem, res ? (size_t)RESERVATION_BYTES : redeem_out_bytes(c, wire, ret), st, sp, nonces, ACT_RNG_PER_LANE, out, status,
    [&](const uint8_t* mask, uint8_t* sp_out) -> int {
      // the tags first: they depend on the verification alone, and behind the insert of k nothing but the receipts may fail
      ReplayDeriveArgs ta{}; ta.n = (uint32_t)n; ta.stride = (uint32_t)k_stride; ta.nul = k_at; ta.kp = kp; ta.st = mask; ta.out = tag; ta.t = t;
      if (dev) {
        RPCK(c, hipSetDevice(c->device));
        if (res) launch_reserve_tag(ta, stream); else replay_derive_dev(ta, false, stream);
        RPCK(c, hipGetLastError());
        RPCK(c, hipMemsetAsync(found, 0, n, stream)); RPCK(c, hipMemsetAsync(repl, 0, n, stream));
        RPCK(c, hipStreamSynchronize(stream));
      } else { if (res) reserve_tags_host(ta); else replay_derive_host(ta, false); memset(found, 0, n); memset(repl, 0, n); }
      const int rc_set = key_epochs ? act_nullifier_check_and_insert_epoch_batch(set, n, mem, k_at, k_stride, mask, out_key, key_epochs, nkeys, spent)
                                    : act_nullifier_check_and_insert_batch(set, n, mem, k_at, k_stride, mask, spent);
      if (rc_set == ACT_ERR_HIP) return rc_set;      // no answer can be trusted: redeem_tail gives every verified lane up as undetermined
      ReplayResolveArgs ra{(uint32_t)n, mask, spent, nullptr, skip, sp_out, repl};
      if (dev) { launch_replay_resolve(ra, stream); RPCK(c, hipGetLastError()); RPCK(c, hipStreamSynchronize(stream)); }
      else for (size_t i = 0; i < n; i++) replay_resolve_lane(ra, (uint32_t)i);
      // a receipt for every lane whose k was fresh, under the epoch k was recorded under; the answer is ignored (a tag that is there is harmless)
      rc_receipts = key_epochs ? act_nullifier_check_and_insert_epoch_batch(receipts, n, mem, tag, 32, skip, out_key, key_epochs, nkeys, r_ans)
                               : act_nullifier_check_and_insert_batch(receipts, n, mem, tag, 32, skip, r_ans);
      // the others: is this the spend that was recorded?  (Behind the insert: a lane spent by an earlier lane of this batch finds that lane's receipt.)
      const int rc_found = act_nullifier_contains_batch(receipts, n, mem, tag, 32, found);
      if (!rc_receipts) rc_receipts = rc_found;
      if (rc_receipts) receipts_err = act_nullifier_set_last_error(receipts);
      ra.found = found;
      if (dev) { launch_replay_resolve(ra, stream); RPCK(c, hipGetLastError()); RPCK(c, hipStreamSynchronize(stream)); }
      else for (size_t i = 0; i < n; i++) replay_resolve_lane(ra, (uint32_t)i);
      return rc_set;
    },
    [&] {      // st is merged by now: the nonces of exactly the lanes that are signed, under the key each is signed with
      if (res) return;
      ring_sign_index(mem, kidx, out_key, sign_key, n);
      ReplayDeriveArgs na{}; na.n = (uint32_t)n; na.stride = (uint32_t)k_stride; na.nkeys = (uint32_t)nkeys; na.nul = k_at; na.kp = kp; na.st = st; na.kidx = kidx;
      na.secrets = secrets; na.out = nonces; na.t = t;
      if (dev) replay_derive_dev(na, true, nullptr); else replay_derive_host(na, true);
    },
    [&](const uint8_t* verdict, const uint8_t* r, int r_mode, uint8_t* o, uint8_t* o_st) {
      if (res) return reserve_emit(c, stream, n, mem, k_at, k_stride, kp, res->s, verdict, o, o_st);
      return ring_sign_step(c, n, mem, keys, nkeys, wire, kidx, kp, verdict, r, r_mode, o, o_st, ret);
    }, !res);
  if (out_counts) {      // status[] is complete behind the tail, whatever it returned
    std::vector<uint8_t> hs;
    const uint8_t *s = status, *r = repl;
    bool ok = true;
    if (dev) {
      hs.resize(2 * n);
      std::lock_guard<std::mutex> lk(c->mu);
      ok = hipSetDevice(c->device) == hipSuccess && hipMemcpy(hs.data(), status, n, hipMemcpyDeviceToHost) == hipSuccess &&
           hipMemcpy(hs.data() + n, repl, n, hipMemcpyDeviceToHost) == hipSuccess;
      if (!ok) (void)hipGetLastError();
      s = hs.data(); r = hs.data() + n;
    }
    if (ok) replay_counts_of(out_counts, n, s, r);
  }
  if (rc_tail) return rc_tail;
  if (rc_receipts && res) { c->err = "receipts set: " + receipts_err + " (every record was handed out; a fresh lane of this batch may not settle and its retry may be refused)"; return rc_receipts; }
  if (rc_receipts) { c->err = "receipts set: " + receipts_err + " (every refund was handed out; a retry of this batch's fresh lanes may be refused)"; return rc_receipts; }
  return ACT_OK;
}

// the verification and the tail over the caller's lanes; the caller has made the whole-call refusals and holds replay_mu
static int redeem_replay_locked(act_ctx* c, act_nullifier_set* set, act_nullifier_set* receipts, size_t n, int mem, const uint8_t* keys, int nkeys,
                                const uint32_t* key_epochs, int sign_key, const uint8_t* proof, const uint8_t* cbor, const uint64_t* offsets, const uint8_t* nonce_key,
                                uint8_t* out, uint8_t* status, uint8_t* out_key, uint8_t* out_replayed, uint64_t* out_counts, const RedeemReturn* ret,
                                const ReplayReserve* res, const uint8_t* bind) {
  const bool wire = cbor != nullptr, dev = mem == ACT_MEM_DEVICE;
  const size_t pb = act_spend_proof_bytes(c);
  // K', the verdicts and (wire form) the nullifiers
  const size_t per_lane = 32 + 1 + (wire ? 32 : 0);
  std::vector<uint8_t> h; DevTmp d(c);
  uint8_t* base; int rc;
  if (dev) { if ((rc = d.alloc(n * per_lane))) return rc; base = d.p; }
  else { h.resize(n * per_lane); base = h.data(); }
  uint8_t *kp = base, *nul = base + n * 32, *st = base + n * (per_lane - 1);
  // bind (DESIGN 4.12): the lanes' request bindings or null; they gate the verification and nothing behind it
  if (wire) { RingSel sel{keys, nkeys, out_key, bind}; rc = verify_spend_cbor_impl(c, n, mem, nullptr, cbor, offsets, st, kp, nul, &sel); }
  else rc = act_verify_spend_keyring_bound_batch(c, n, mem, keys, nkeys, proof, bind, st, out_key, kp);
  if (rc) return rc;
  return replay_tail(c, set, receipts, n, mem, keys, nkeys, key_epochs, sign_key, wire, wire ? nul : proof, wire ? 32 : pb, kp, st, nonce_key, out, status, out_key,
                     out_replayed, out_counts, nullptr, ret, res);
}

static int redeem_replay_impl(act_ctx* c, act_nullifier_set* set, act_nullifier_set* receipts, size_t n, int mem, const uint8_t* keys, int nkeys,
                              const uint32_t* key_epochs, int sign_key, const uint8_t* proof, const uint8_t* cbor, const uint64_t* offsets, const uint8_t* nonce_key,
                              uint8_t* out, uint8_t* status, uint8_t* out_key, uint8_t* out_replayed, uint64_t* out_counts) {
  if (out_counts) memset(out_counts, 0, sizeof(uint64_t) * ACT_REPLAY_COUNTS);
  if (!c || (mem != ACT_MEM_HOST && mem != ACT_MEM_DEVICE) || n > ((size_t)1 << 30)) return ACT_ERR_ARG;
  // everything the ring redeem call refuses as a whole, in the same words (the nonces stand where its rng stands), then this call's own
  static const uint8_t derived = 0;
  if (int bad = redeem_keyring_refused(c, set, n, keys, nkeys, key_epochs, sign_key, proof, cbor, &derived, ACT_RNG_PER_LANE, out, status, out_key)) return bad;
  if (int bad = replay_refused(c, set, receipts, nonce_key, n, key_epochs, nkeys)) return bad;
  if (n == 0) return redeem_keyring_impl(c, set, 0, mem, keys, nkeys, key_epochs, sign_key, nullptr, nullptr, nullptr, &derived, ACT_RNG_PER_LANE, nullptr, nullptr, nullptr);
  // one replay call at a time per context: the staged secrets and the derived nonces live in the context's own buffer (d_replay)
  std::lock_guard<std::mutex> replay(c->replay_mu);
  return redeem_replay_locked(c, set, receipts, n, mem, keys, nkeys, key_epochs, sign_key, proof, cbor, offsets, nonce_key, out, status, out_key, out_replayed, out_counts,
                              nullptr, nullptr);
}

extern "C" int act_redeem_replay_batch(act_ctx* c, act_nullifier_set* set, act_nullifier_set* receipts, size_t n, int mem, const uint8_t* keys, int nkeys,
                                       const uint32_t* key_epochs, int sign_key, const uint8_t* proof, const uint8_t nonce_key[32], uint8_t* out_refund,
                                       uint8_t* status, uint8_t* out_key, uint8_t* out_replayed, uint64_t* out_counts) {
  if (n && !proof) return ACT_ERR_ARG;
  return redeem_replay_impl(c, set, receipts, n, mem, keys, nkeys, key_epochs, sign_key, proof, nullptr, nullptr, nonce_key, out_refund, status, out_key, out_replayed,
                            out_counts);
}
extern "C" int act_redeem_cbor_replay_batch(act_ctx* c, act_nullifier_set* set, act_nullifier_set* receipts, size_t n, int mem, const uint8_t* keys, int nkeys,
                                            const uint32_t* key_epochs, int sign_key, const uint8_t* cbor, const uint64_t* offsets, const uint8_t nonce_key[32],
                                            uint8_t* out_refund_cbor, uint8_t* status, uint8_t* out_key, uint8_t* out_replayed, uint64_t* out_counts) {
  if (n && !cbor) return ACT_ERR_ARG;
  static const uint8_t none = 0;
  return redeem_replay_impl(c, set, receipts, n, mem, keys, nkeys, key_epochs, sign_key, nullptr, cbor ? cbor : &none, offsets, nonce_key, out_refund_cbor, status,
                            out_key, out_replayed, out_counts);
}

// the building block of both derive calls; returned (act_replay_derive_return_batch): n amounts in `mem` memory, null: act_replay_derive_batch
static int replay_derive_impl(act_ctx* c, size_t n, int mem, const uint8_t* keys, int nkeys, const uint8_t* key_index, const uint8_t* nonce_key,
                              const uint8_t* nullifiers, size_t stride, const uint8_t* kprime, const uint8_t* status_in, const uint8_t* returned, uint8_t* out_tags,
                              uint8_t* out_nonces) {
  if (!c || !keys || !nonce_key || nkeys < 1 || nkeys > ACT_KEYRING_MAX || (mem != ACT_MEM_HOST && mem != ACT_MEM_DEVICE)) return ACT_ERR_ARG;
  if (n > ((size_t)1 << 30) || stride < 32 || stride > 0xFFFFFFFFu || (n && (!key_index || !nullifiers || !kprime || !status_in))) return ACT_ERR_ARG;
  if (n == 0 || (!out_tags && !out_nonces)) return ACT_OK;
  std::lock_guard<std::mutex> replay(c->replay_mu);
  ReplayDeriveArgs a{}; a.n = (uint32_t)n; a.stride = (uint32_t)stride; a.nkeys = (uint32_t)nkeys; a.nul = nullifiers; a.kp = kprime; a.st = status_in; a.kidx = key_index;
  a.t = returned;
  if (mem == ACT_MEM_HOST) {
    ReplaySecretsHost sec;
    sec.stage(0, nonce_key, keys, nkeys);
    a.secrets = sec.p.get();
    if (out_tags) { a.out = out_tags; replay_derive_host(a, false); }
    if (out_nonces) { a.out = out_nonces; replay_derive_host(a, true); }
    return ACT_OK;
  }
  ReplaySecretsDev sec(c);
  if (int rc = sec.stage(0, nonce_key, keys, nkeys)) return rc;
  a.secrets = c->d_replay;
  std::lock_guard<std::mutex> lk(c->mu);
  RPCK(c, hipSetDevice(c->device));
  hipStream_t stream = c->slots[0].stream;
  if (out_tags) { a.out = out_tags; replay_derive_dev(a, false, stream); }
  if (out_nonces) { a.out = out_nonces; replay_derive_dev(a, true, stream); }
  RPCK(c, hipGetLastError());
  RPCK(c, hipStreamSynchronize(stream));
  return ACT_OK;
}
extern "C" int act_replay_derive_batch(act_ctx* c, size_t n, int mem, const uint8_t* keys, int nkeys, const uint8_t* key_index, const uint8_t nonce_key[32],
                                       const uint8_t* nullifiers, size_t stride, const uint8_t* kprime, const uint8_t* status_in, uint8_t* out_tags,
                                       uint8_t* out_nonces) {
  return replay_derive_impl(c, n, mem, keys, nkeys, key_index, nonce_key, nullifiers, stride, kprime, status_in, nullptr, out_tags, out_nonces);
}
extern "C" int act_replay_derive_return_batch(act_ctx* c, size_t n, int mem, const uint8_t* keys, int nkeys, const uint8_t* key_index, const uint8_t nonce_key[32],
                                              const uint8_t* nullifiers, size_t stride, const uint8_t* kprime, const uint8_t* status_in, const uint8_t* returned,
                                              uint8_t* out_tags, uint8_t* out_nonces) {
  return replay_derive_impl(c, n, mem, keys, nkeys, key_index, nonce_key, nullifiers, stride, kprime, status_in, returned, out_tags, out_nonces);
}
