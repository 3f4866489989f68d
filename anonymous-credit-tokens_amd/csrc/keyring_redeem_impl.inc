// keyring_redeem_impl.inc — included by engine.hip after nullifier_impl.inc: the redemption step against a ring of issuer keys.
// Ring verification, then redeem_tail (nullifier_impl.inc: the body every redeem entry point ends in, with its failure contract) over
// the ring's steps: each lane is signed with the key `sign_key` names.  Membership in the nullifier set does not depend on the key.  No tiny form.
// key_epochs (nullable, host memory, nkeys values): an accepted lane's nullifier is recorded under the epoch of the key it MATCHED --
// out_key, as the ring verification leaves it, is the epoch index of the insert.
// Arrays of n lanes in `mem` memory: st = the verdicts, out_key = the matched ring indices, kp = enc(K'), the nullifiers at
// nul + i * nul_stride; sp and kidx are scratch of n bytes each.  The admission calls (admit_impl.inc) hand it the survivors' compact arrays.
// the signatures of a ring redemption, each lane with ring key kidx[i], framed as Refund messages for the wire form (redeem_tail's sign_step)
// The return calls (act_redeem_(cbor_)return_batch, DESIGN 4.10): the amounts t the signing step adds to X_A as t h1.  t: n scalars in
// the call's kind of memory, lane for lane with the tail's arrays, or null (every t = 0).  The outputs are RefundReturn records (160
// bytes) or messages (ACT_CBOR_REFUND_RETURN).  A null RedeemReturn* everywhere below: the Refund forms, as they were.
struct RedeemReturn { const uint8_t* t; };
static size_t redeem_out_bytes(const act_ctx* c, bool wire, const RedeemReturn* ret) {
  return wire ? act_cbor_size(c, ret ? ACT_CBOR_REFUND_RETURN : ACT_CBOR_REFUND) : (ret ? (size_t)160 : (size_t)128);
}
// the RefundReturn layout on the device for phase B's framing (refund_sign_keyring_impl, keyring_impl.inc; the caller holds the context):
// slot 1's layout area, as the issuance wire calls keep their response layout
extern "C" {
static int refund_return_frame_prepare(act_ctx* c, FrameOut* fo) {
  CborDev d;
  if (int rc = cbor_dev_prepare(c, c->slots[1], ACT_CBOR_REFUND_RETURN, &d)) return rc;
  *fo = FrameOut{d.tmpl, d.pay_off, (uint32_t)d.lay.tmpl.size()};
  return ACT_OK;
}
}
static int ring_sign_step(act_ctx* c, size_t n, int mem, const uint8_t* keys, int nkeys, bool wire, const uint8_t* kidx, const uint8_t* kp, const uint8_t* verdict,
                          const uint8_t* r, int r_mode, uint8_t* o, uint8_t* o_st, const RedeemReturn* ret = nullptr) {
  // the return calls: records, or (wire) messages framed on the device by the lane that signed, as issuance frames its responses
  if (ret) return refund_sign_keyring_impl(c, n, mem, keys, nkeys, kidx, kp, verdict, r, r_mode, o, o_st, true, ret->t, wire);
  if (!wire) return act_refund_sign_keyring_batch(c, n, mem, keys, nkeys, kidx, kp, verdict, r, r_mode, o, o_st);
  int rc_sign;
  if (mem == ACT_MEM_HOST) {      // framed as act_refund_sign_cbor_batch frames: on the host workers, where the signatures landed
    std::vector<uint8_t> rec(n * 128);
    rc_sign = act_refund_sign_keyring_batch(c, n, mem, keys, nkeys, kidx, kp, verdict, r, r_mode, rec.data(), o_st);
    if (!rc_sign) cbor_frame_refunds_host(cbor_layout(*cbor_type(ACT_CBOR_REFUND), c->L), n, rec.data(), o_st, o);
    return rc_sign;
  }
  DevTmp rec(c);
  rc_sign = rec.alloc(n * 128);
  if (!rc_sign) rc_sign = act_refund_sign_keyring_batch(c, n, mem, keys, nkeys, kidx, kp, verdict, r, r_mode, rec.p, o_st);
  if (!rc_sign) rc_sign = act_cbor_encode_batch(c, ACT_CBOR_REFUND, n, mem, rec.p, o);
  if (!rc_sign) {
    std::lock_guard<std::mutex> lk(c->mu);
    (void)hipSetDevice(c->device);
    const uint32_t out_b = (uint32_t)act_cbor_size(c, ACT_CBOR_REFUND);
    hipLaunchKernelGGL(k_cbor_zero_failed, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->slots[0].stream, o, out_b, o_st, (uint32_t)n);
    if (hipStreamSynchronize(c->slots[0].stream) != hipSuccess) { (void)hipGetLastError(); c->err = "k_cbor_zero_failed failed"; rc_sign = ACT_ERR_HIP; }
  }
  return rc_sign;
}
// the key every lane is signed with (out_key keeps what the lane matched): redeem_tail's beside_merge of the ring calls
static void ring_sign_index(int mem, uint8_t* kidx, const uint8_t* out_key, int sign_key, size_t n) {
  if (mem == ACT_MEM_DEVICE) launch_ring_resolve_index(kidx, out_key, sign_key, (uint32_t)n, nullptr);
  else for (size_t i = 0; i < n; i++) kidx[i] = sign_key >= 0 ? (uint8_t)sign_key : out_key[i];
}
static int redeem_tail_ring(act_ctx* c, act_nullifier_set* set, size_t n, int mem, const uint8_t* keys, int nkeys, const uint32_t* key_epochs, int sign_key, bool wire,
                            const uint8_t* nul, size_t nul_stride, const uint8_t* kp, uint8_t* st, uint8_t* sp, uint8_t* kidx, const uint8_t* rng, int rng_mode,
                            uint8_t* out, uint8_t* status, uint8_t* out_key, const RedeemReturn* ret = nullptr) {
  return redeem_tail_sized(c, set, n, mem, redeem_out_bytes(c, wire, ret), st, sp, rng, rng_mode, out, status,
    [&](const uint8_t* mask, uint8_t* spent) {
      return key_epochs ? act_nullifier_check_and_insert_epoch_batch(set, n, mem, nul, nul_stride, mask, out_key, key_epochs, nkeys, spent)
                        : act_nullifier_check_and_insert_batch(set, n, mem, nul, nul_stride, mask, spent);
    },
    [&] { ring_sign_index(mem, kidx, out_key, sign_key, n); },
    [&](const uint8_t* verdict, const uint8_t* r, int r_mode, uint8_t* o, uint8_t* o_st) {
      return ring_sign_step(c, n, mem, keys, nkeys, wire, kidx, kp, verdict, r, r_mode, o, o_st, ret);
    });
}

// what the ring redeem calls refuse as a whole before any GPU work (no status written, nothing recorded): shared with admit_impl.inc
static int redeem_keyring_refused(act_ctx* c, act_nullifier_set* set, size_t n, const uint8_t* keys, int nkeys, const uint32_t* key_epochs, int sign_key, const uint8_t* proof,
                                  const uint8_t* cbor, const uint8_t* rng, int rng_mode, const uint8_t* out, const uint8_t* status, const uint8_t* out_key) {
  if (!c || !set || !keys || !rng || nkeys < 1 || nkeys > ACT_KEYRING_MAX || (n && ((!proof && !cbor) || !out || !status || !out_key))) return ACT_ERR_ARG;
  if (sign_key != ACT_SIGN_MATCHED && (sign_key < 0 || sign_key >= nkeys)) return ACT_ERR_ARG;
  if (rng_mode != ACT_RNG_PER_LANE && rng_mode != ACT_RNG_SEQUENTIAL && rng_mode != ACT_RNG_CALLBACK) return ACT_ERR_ARG;
  if (set->device != c->device) { c->err = "act_redeem_keyring_batch: the nullifier set lives on another device"; return ACT_ERR_ARG; }
  if (key_epochs) {      // refused before any verification work: nothing recorded, nothing signed, no status written
    std::string why;
    { std::lock_guard<std::mutex> lk(set->mu); why = null_epochs_refused(set, key_epochs, nkeys); }
    if (!why.empty()) { c->err = "act_redeem_keyring_epochs_batch: " + why; return ACT_ERR_ARG; }
  }
  return ACT_OK;
}

static int redeem_keyring_impl(act_ctx* c, act_nullifier_set* set, size_t n, int mem, const uint8_t* keys, int nkeys, const uint32_t* key_epochs, int sign_key, const uint8_t* proof,
                               const uint8_t* cbor, const uint64_t* offsets, const uint8_t* rng, int rng_mode, uint8_t* out, uint8_t* status, uint8_t* out_key,
                               const RedeemReturn* ret = nullptr) {
  const bool wire = cbor != nullptr;
  if (int bad = redeem_keyring_refused(c, set, n, keys, nkeys, key_epochs, sign_key, proof, cbor, rng, rng_mode, out, status, out_key)) return bad;
  if (n == 0) {      // a bad ring fails the call whatever n
    Call call(c, 0);
    HIPCK(c, hipSetDevice(c->device));
    const DevKey* d_ring = nullptr;
    int rc0 = ring_set(c, keys, nkeys, &d_ring);
    return rc0 ? rc0 : call.finish();
  }
  const size_t pb = act_spend_proof_bytes(c);
  // K', verdicts, look-up answers, key indices and (wire form) the nullifiers beside the caller's arrays
  const size_t per_lane = 35 + (wire ? 32 : 0);
  std::vector<uint8_t> h; DevTmp d(c);
  uint8_t* base; int rc;
  if (mem == ACT_MEM_DEVICE) { if ((rc = d.alloc(n * per_lane))) return rc; base = d.p; }
  else { h.resize(n * per_lane); base = h.data(); }
  uint8_t *kp = base, *nul = base + n * 32, *st = base + n * (per_lane - 3), *sp = st + n, *kidx = sp + n;
  if (wire) { RingSel sel{keys, nkeys, out_key}; rc = verify_spend_cbor_impl(c, n, mem, nullptr, cbor, offsets, st, kp, nul, &sel); }
  else rc = act_verify_spend_keyring_batch(c, n, mem, keys, nkeys, proof, st, out_key, kp);
  if (rc) return rc;
  return redeem_tail_ring(c, set, n, mem, keys, nkeys, key_epochs, sign_key, wire, wire ? nul : proof, wire ? 32 : pb, kp, st, sp, kidx, rng, rng_mode, out, status, out_key, ret);
}

extern "C" int act_redeem_keyring_batch(act_ctx* c, act_nullifier_set* set, size_t n, int mem, const uint8_t* keys, int nkeys, int sign_key, const uint8_t* proof,
                                        const uint8_t* rng, int rng_mode, uint8_t* out_refund, uint8_t* status, uint8_t* out_key) {
  if (n && !proof) return ACT_ERR_ARG;
  return redeem_keyring_impl(c, set, n, mem, keys, nkeys, nullptr, sign_key, proof, nullptr, nullptr, rng, rng_mode, out_refund, status, out_key);
}
extern "C" int act_redeem_cbor_keyring_batch(act_ctx* c, act_nullifier_set* set, size_t n, int mem, const uint8_t* keys, int nkeys, int sign_key,
                                             const uint8_t* cbor, const uint64_t* offsets, const uint8_t* rng, int rng_mode, uint8_t* out_refund_cbor,
                                             uint8_t* status, uint8_t* out_key) {
  if (n && !cbor) return ACT_ERR_ARG;
  static const uint8_t none = 0;
  return redeem_keyring_impl(c, set, n, mem, keys, nkeys, nullptr, sign_key, nullptr, cbor ? cbor : &none, offsets, rng, rng_mode, out_refund_cbor, status, out_key);
}
extern "C" int act_redeem_keyring_epochs_batch(act_ctx* c, act_nullifier_set* set, size_t n, int mem, const uint8_t* keys, int nkeys, const uint32_t* key_epochs,
                                               int sign_key, const uint8_t* proof, const uint8_t* rng, int rng_mode, uint8_t* out_refund, uint8_t* status, uint8_t* out_key) {
  if (!key_epochs || (n && !proof)) return ACT_ERR_ARG;
  return redeem_keyring_impl(c, set, n, mem, keys, nkeys, key_epochs, sign_key, proof, nullptr, nullptr, rng, rng_mode, out_refund, status, out_key);
}
extern "C" int act_redeem_cbor_keyring_epochs_batch(act_ctx* c, act_nullifier_set* set, size_t n, int mem, const uint8_t* keys, int nkeys, const uint32_t* key_epochs,
                                                    int sign_key, const uint8_t* cbor, const uint64_t* offsets, const uint8_t* rng, int rng_mode,
                                                    uint8_t* out_refund_cbor, uint8_t* status, uint8_t* out_key) {
  if (!key_epochs || (n && !cbor)) return ACT_ERR_ARG;
  static const uint8_t none = 0;
  return redeem_keyring_impl(c, set, n, mem, keys, nkeys, key_epochs, sign_key, nullptr, cbor ? cbor : &none, offsets, rng, rng_mode, out_refund_cbor, status, out_key);
}
