// admit_impl.inc — included by engine.hip after keyring_redeem_impl.inc: admission before verification (DESIGN 4.7; kernels in
// k_admit.hip, lane bodies in admit_lanes.h).  act_redeem_admit_batch / act_redeem_cbor_admit_batch are the ring redeem calls with a
// screen in front: per lane the charge is compared with the expected one and the nullifier is looked up (read only) BEFORE the proof
// is verified, and only the lanes that pass go through verification -> check-and-insert -> sign.
//   1. screen        k and s of every lane (records: fields 0 and 1; wire: the payloads of a canonical message, and of any other
//                    spelling what the wire reader's reduced form gives -- cbor_lanes.h with keep_fields = 2, as a kernel for
//                    device-memory callers and on the host workers for host-memory callers; under ACT_WIRE_READER_HOST the host
//                    reader's record, in windows of WIRE_SETTLE_WINDOW: wire_window_read, cbor_impl.inc) -> pre-status, reduced k [k_admit_screen]
//   2. compaction    the survivors' lane numbers in lane order                                  [k_admit_count / _scan / _write]
//   3. verification  of the survivors only, their records / messages gathered ADMIT_WINDOW_BATCHES * max_batch at a time
//   4. once per call check-and-insert and signing over the compact 32-byte arrays (redeem_tail_ring, keyring_redeem_impl.inc): one rng draw per call
//   5. scatter       statuses, out_key and refunds back to their lanes; shed lanes get all-zero records           [k_admit_scatter]
// Nothing is shed (m == n): the caller's pointers go straight to redeem_keyring_impl; everything is shed: no verification kernel runs.
// The decision that RECORDS is still the check-and-insert behind verification; the look-up of step 1 only spares work.
// act_redeem_(cbor_)admit_unique_batch add the copy stage between steps 2 and 3 (copies_impl.inc, included behind this file): a
// survivor whose input bytes are those of an earlier survivor is not verified and takes its answer from that lane      [k_copies.hip]
// act_redeem_(cbor_)admit_replay_batch (admit_replay_impl.inc, included behind replay_impl.inc; DESIGN 4.9) add a stage between steps 1
// and 2 -- a spent lane whose receipt is this proof's own is a retry candidate and survives -- and end in the replay tail, not the ring's
// act_redeem_(cbor_)return_replay_batch are that form with the returned amounts of the return calls (ret && rp, DESIGN 4.10): t <= s is the
// screen's rule, a candidate's tag and every tag and nonce of the tail take the lane's t, and the outputs are RefundReturns.
// act_redeem_(cbor_)admit_replay_unique_batch are both at once (unique && rp): the copy stage runs over fresh lanes and retry candidates
// alike, and behind the scatters a copy is SERVED -- it takes its leader's refund -- where the unique forms above resolve it  [k_copy_serve]
// act_redeem_(cbor_)return_replay_unique_batch are all three (ret && rp && unique): equality is decided on the proof bytes alone, the amounts
// of the verified lanes are gathered by v_idx, and a copy is served only if it names its leader's amount                 [k_copy_serve_return]
namespace {

constexpr size_t ADMIT_WINDOW_BATCHES = 4;       // survivors gathered and verified at a time, in units of max_batch
constexpr size_t ADMIT_WIRE_LAUNCH = (size_t)1 << 20;      // messages per launch of the framing compare

#define ADCK(c, expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { (c)->err = std::string("admission: ") + #expr + ": " + hipGetErrorString(e_); (void)hipGetLastError(); return ACT_ERR_HIP; } } while (0)

// the per-lane rng slices of the survivors (ACT_RNG_PER_LANE, device-memory callers): the context's own buffer, wiped on every exit
struct AdmitRngDev {
  act_ctx* c; size_t dirty = 0;
  explicit AdmitRngDev(act_ctx* c_) : c(c_) {}
  int reserve(size_t bytes) {
    std::lock_guard<std::mutex> lk(c->mu);
    ADCK(c, hipSetDevice(c->device));
    if (bytes > c->d_admit_rng_cap) {
      if (c->d_admit_rng) { ADCK(c, hipFree(c->d_admit_rng)); c->d_admit_rng = nullptr; c->d_admit_rng_cap = 0; }      // (wiped when its call ended)
      ADCK(c, hipMalloc(&c->d_admit_rng, bytes)); c->d_admit_rng_cap = bytes;
      ADCK(c, hipMemset(c->d_admit_rng, 0, bytes));
      ADCK(c, hipDeviceSynchronize());      // (the memset runs on the null stream; the gather that fills the buffer does not wait for that stream)
    }
    dirty = bytes;
    return ACT_OK;
  }
  ~AdmitRngDev() { if (dirty && c->d_admit_rng) { (void)hipSetDevice(c->device); if (hipMemset(c->d_admit_rng, 0, dirty) != hipSuccess || hipDeviceSynchronize() != hipSuccess) (void)hipGetLastError(); } }
};
struct AdmitHostWipe { std::vector<uint8_t>& v; ~AdmitHostWipe() { if (!v.empty()) wipe_host(v.data(), v.size()); } };

// n bytes in the caller's kind of memory
struct AdmitArr {
  std::vector<uint8_t> h; DevTmp d; uint8_t* p = nullptr;
  explicit AdmitArr(act_ctx* c) : d(c) {}
  int alloc(int mem, size_t bytes) {
    if (mem == ACT_MEM_DEVICE) { int rc = d.alloc(bytes); if (rc) return rc; p = d.p; hipError_t e = hipMemset(p, 0, bytes ? bytes : 1); if (e == hipSuccess) e = hipDeviceSynchronize(); if (e != hipSuccess) { (void)hipGetLastError(); return ACT_ERR_HIP; } }
    else { h.assign(bytes ? bytes : 1, 0); p = h.data(); }
    return ACT_OK;
  }
};

struct AdmitWireJob { AdmitWireArgs a; };
struct AdmitReadJob { CborReadArgs a; };
struct AdmitRowsJob { uint8_t* dst; const uint8_t* src; const uint32_t* idx; size_t row; };
struct AdmitMsgsJob { uint8_t* dst; const uint64_t* dst_off; const uint8_t* src; const uint64_t* src_beg; };

// One window of lanes gathered into the caller's kind of memory (step 3's survivors; the spent lanes of the replay form,
// admit_replay_impl.inc): records or canonical-size messages as rows of one size, messages between monotone offsets with offsets of
// their own.  d_idx: the window's lane numbers in device memory (device-memory callers); h_idx: the same on the host.
struct AdmitGather {
  act_ctx* c; hipStream_t stream; bool dev; const uint8_t* src; size_t row; const WireExtent* ext;      // ext: messages between offsets, else rows
  DevTmp gd, d_moff; std::unique_ptr<uint8_t[]> gh; size_t g_cap = 0, moff_cap = 0;      // (host: not zero-filled -- the gather writes every byte that is read)
  std::vector<uint64_t> dst_off, src_beg;
  AdmitGather(act_ctx* c_, hipStream_t s, bool dev_, const uint8_t* src_, size_t row_, const WireExtent* ext_) : c(c_), stream(s), dev(dev_), src(src_), row(row_), ext(ext_), gd(c_), d_moff(c_) {}
  const uint8_t* data() const { return dev ? gd.p : gh.get(); }
  const uint64_t* offsets() const { return ext ? dst_off.data() : nullptr; }
  const uint64_t* dev_offsets() const { return (ext && dev) ? reinterpret_cast<const uint64_t*>(d_moff.p) + moff_cap : nullptr; }      // the same in device memory (device-memory callers)
  static int regrow(act_ctx* c, DevTmp& t, size_t bytes) {
    if (t.p) { std::lock_guard<std::mutex> lk(c->mu); ADCK(c, hipFree(t.p)); t.p = nullptr; t.bytes = 0; }
    return t.alloc(bytes);
  }
  int reserve(size_t bytes) {      // the gather buffer, in the caller's kind of memory
    if (bytes <= g_cap) return ACT_OK;
    if (dev) { if (int r = regrow(c, gd, bytes)) return r; }
    else gh.reset(new uint8_t[bytes ? bytes : 1]);
    g_cap = bytes;
    return ACT_OK;
  }
  int run(const uint32_t* d_idx, const uint32_t* h_idx, size_t w) {
    int rc;
    if (!ext) {      // rows of one size
      if ((rc = reserve(w * row))) return rc;
      if (dev) {
        AdmitRowsArgs ra{gd.p, src, d_idx, (uint32_t)w, row};
        launch_admit_rows(ra, stream);
        ADCK(c, hipGetLastError());
        ADCK(c, hipStreamSynchronize(stream));
      } else {
        AdmitRowsJob job{gh.get(), src, h_idx, row};
        act_host_parallel_for(w, 16, 0, [](void* p, size_t i0, size_t i1) {
          const AdmitRowsJob& j = *static_cast<const AdmitRowsJob*>(p);
          for (size_t k = i0; k < i1; k++) memcpy(j.dst + k * j.row, j.src + (size_t)j.idx[k] * j.row, j.row);
        }, &job);
      }
      return ACT_OK;
    }
    // messages between monotone offsets, gathered with offsets of their own
    dst_off.assign(w + 1, 0); src_beg.assign(w, 0);
    size_t longest = 0;
    for (size_t k = 0; k < w; k++) {
      const size_t i = h_idx[k], len = ext->end(i) - ext->beg(i);
      src_beg[k] = ext->beg(i); dst_off[k + 1] = dst_off[k] + len; longest = std::max(longest, len);
    }
    if ((rc = reserve((size_t)dst_off[w]))) return rc;
    if (dev) {      // a window's source starts and destination offsets
      if (w > moff_cap) { if ((rc = regrow(c, d_moff, (2 * w + 1) * 8))) return rc; moff_cap = w; }
      uint64_t* d_src = reinterpret_cast<uint64_t*>(d_moff.p); uint64_t* d_dst = d_src + moff_cap;
      ADCK(c, hipMemcpyAsync(d_src, src_beg.data(), w * 8, hipMemcpyHostToDevice, stream));
      ADCK(c, hipMemcpyAsync(d_dst, dst_off.data(), (w + 1) * 8, hipMemcpyHostToDevice, stream));
      AdmitMsgsArgs ma{gd.p, d_dst, src, d_src, (uint32_t)w, admit_pieces(longest)};
      launch_admit_msgs(ma, stream);
      ADCK(c, hipGetLastError());
      ADCK(c, hipStreamSynchronize(stream));
    } else {
      AdmitMsgsJob job{gh.get(), dst_off.data(), src, src_beg.data()};
      act_host_parallel_for(w, 16, 0, [](void* p, size_t i0, size_t i1) {
        const AdmitMsgsJob& j = *static_cast<const AdmitMsgsJob*>(p);
        for (size_t k = i0; k < i1; k++) memcpy(j.dst + j.dst_off[k], j.src + j.src_beg[k], (size_t)(j.dst_off[k + 1] - j.dst_off[k]));
      }, &job);
    }
    return ACT_OK;
  }
};

// ret (the return calls): a ninth value, the lanes whose returned amount exceeded their charge (ACT_REDEEM_RETURN_COUNTS); their
// unique forms keep a tenth, the copies, which the caller fills in (ACT_REDEEM_RETURN_UNIQUE_COUNTS)
void admit_counts_of(uint64_t* out_counts, size_t n, const uint8_t* pre, size_t m, const uint8_t* cst, bool ret = false) {
  if (!out_counts) return;
  uint64_t k[ACT_REDEEM_RETURN_COUNTS] = {n, 0, 0, 0, m, 0, 0, 0, 0};
  for (size_t i = 0; i < n; i++) {
    const uint8_t p = pre[i];
    if (p == ACT_STATUS_WRONG_CHARGE) k[2]++; else if (p == ACT_STATUS_DOUBLE_SPEND) k[3]++; else if (ret && p == ACT_STATUS_RETURN_TOO_BIG) k[8]++; else if (p) k[1]++;
  }
  for (size_t j = 0; j < m; j++) {
    const uint8_t s = cst[j];
    if (s == 0) k[7]++; else if (s == ACT_STATUS_DOUBLE_SPEND) k[6]++;
    else if (s != ACT_STATUS_NULLIFIER_UNDETERMINED && s != ACT_STATUS_RECORDED_UNSIGNED) k[5]++;
  }
  memcpy(out_counts, k, sizeof(uint64_t) * (ret ? ACT_REDEEM_RETURN_COUNTS : ACT_ADMIT_COUNTS));
}

// the copy stage of the unique forms (copies_impl.inc): what it leaves for the rest of the call.  copies == 0: nothing below is used
struct AdmitCopies {
  act_ctx* c; DevTmp d;
  size_t copies = 0, m2 = 0;                                  // m2 = the lanes that are verified
  uint8_t* d_pre2 = nullptr; uint32_t *d_lead = nullptr, *d_idx2 = nullptr, *d_pos2 = nullptr;      // n entries each, in d
  explicit AdmitCopies(act_ctx* c_) : c(c_), d(c_) {}
  // span: the survivors' bytes in the caller's kind of memory (offsets in the same kind); h_idx: host-memory callers only
  int run(hipStream_t stream, bool dev, size_t n, size_t m, const CopySpan& span, const uint8_t* d_pre, const uint32_t* d_idx, const uint32_t* h_idx,
          const uint32_t salt[4]);
};

// the replay form (act_redeem_(cbor_)admit_replay_batch, DESIGN 4.9; admit_replay_impl.inc, included behind replay_impl.inc): what it
// hands to redeem_admit_impl and what its stage between the screen and the compaction leaves
struct AdmitReplay {
  act_nullifier_set* receipts; const uint8_t* nonce_key; uint8_t* out_replayed; uint64_t* out_counts;
  size_t candidates = 0;              // spent lanes whose tag the receipts hold: verified like fresh lanes
};
// the stage's view of the call: the screen's arrays and, as scratch until the survivors' compaction overwrites them, the compaction's
struct AdmitReplayStage {
  hipStream_t stream; size_t n; bool dev, wire, dev_reader; const uint8_t* proof; const uint8_t* cbor; const WireExtent* ext; bool offsets;
  uint8_t* d_pre; const uint8_t* d_kred; uint32_t *d_blk, *d_idx, *d_pos, *d_total;
  const uint8_t* d_t;                 // the return form: the n returned amounts in device memory, as the screen read them (null: every t = 0)
};

}  // namespace

static int admit_replay_stage(act_ctx* c, AdmitReplay& rp, const AdmitReplayStage& g);
static void admit_replay_counts_of(uint64_t* out_counts, size_t n, const uint8_t* pre, size_t candidates, size_t m, const uint64_t* tail_counts, bool ret = false);
static int replay_refused(act_ctx* c, act_nullifier_set* set, act_nullifier_set* receipts, const uint8_t* nonce_key, size_t n, const uint32_t* key_epochs, int nkeys);
static int replay_tail(act_ctx* c, act_nullifier_set* set, act_nullifier_set* receipts, size_t n, int mem, const uint8_t* keys, int nkeys, const uint32_t* key_epochs,
                       int sign_key, bool wire, const uint8_t* k_at, size_t k_stride, const uint8_t* kp, uint8_t* st, const uint8_t* nonce_key, uint8_t* out,
                       uint8_t* status, uint8_t* out_key, uint8_t* out_replayed, uint64_t* out_counts, bool* began = nullptr, const RedeemReturn* ret = nullptr);
static int redeem_replay_locked(act_ctx* c, act_nullifier_set* set, act_nullifier_set* receipts, size_t n, int mem, const uint8_t* keys, int nkeys,
                                const uint32_t* key_epochs, int sign_key, const uint8_t* proof, const uint8_t* cbor, const uint64_t* offsets, const uint8_t* nonce_key,
                                uint8_t* out, uint8_t* status, uint8_t* out_key, uint8_t* out_replayed, uint64_t* out_counts, const RedeemReturn* ret = nullptr);

// rp (the replay form): rng / rng_mode are the derived nonces' stand-in (one byte, ACT_RNG_PER_LANE) and out_counts is null -- the
// form's own counts are rp->out_counts
static int redeem_admit_impl(act_ctx* c, act_nullifier_set* set, size_t n, int mem, const uint8_t* keys, int nkeys, const uint32_t* key_epochs, int sign_key,
                             const uint8_t* proof, const uint8_t* cbor, const uint64_t* offsets, const uint8_t* charge, const uint8_t* rng, int rng_mode,
                             uint8_t* out, uint8_t* status, uint8_t* out_key, uint64_t* out_counts, bool unique = false, AdmitReplay* rp = nullptr,
                             const RedeemReturn* ret = nullptr) {      // ret (the return calls, DESIGN 4.10); ret && rp: the return replay forms
  const bool wire = cbor != nullptr, dev = mem == ACT_MEM_DEVICE;
  if (out_counts) memset(out_counts, 0, sizeof(uint64_t) * (ret ? (unique ? ACT_REDEEM_RETURN_UNIQUE_COUNTS : ACT_REDEEM_RETURN_COUNTS) : unique ? ACT_ADMIT_UNIQUE_COUNTS : ACT_ADMIT_COUNTS));
  if (rp && rp->out_counts) memset(rp->out_counts, 0, sizeof(uint64_t) * (ret ? (unique ? ACT_RETURN_REPLAY_UNIQUE_COUNTS : ACT_RETURN_REPLAY_COUNTS) : unique ? ACT_ADMIT_REPLAY_UNIQUE_COUNTS : ACT_ADMIT_REPLAY_COUNTS));
  if (!c || (mem != ACT_MEM_HOST && mem != ACT_MEM_DEVICE) || n > ((size_t)1 << 30)) return ACT_ERR_ARG;
  if (n && ((!proof && !cbor) || !out || !status || !out_key)) return ACT_ERR_ARG;
  if (wire && offsets) for (size_t i = 0; i < n; i++) if (offsets[i + 1] < offsets[i]) return ACT_ERR_ARG;
  // everything the redeem call refuses as a whole (null handles, ring size, sign_key, rng convention, device, epochs) is refused here in
  // the same words and before anything is looked at -- host checks only; a ring whose w does not decode fails the verification step
  // (or, for a batch that is shed completely, the empty ring call below) before anything is written
  int rc = redeem_keyring_refused(c, set, 0, keys, nkeys, key_epochs, sign_key, nullptr, nullptr, rng, rng_mode, nullptr, nullptr, nullptr);
  if (rc) return rc;
  if (rp && (rc = replay_refused(c, set, rp->receipts, rp->nonce_key, n, key_epochs, nkeys))) return rc;
  if (n == 0) return redeem_keyring_impl(c, set, 0, mem, keys, nkeys, key_epochs, sign_key, nullptr, nullptr, nullptr, rng, rng_mode, nullptr, nullptr, nullptr);
  // one admission call at a time per context: the gathered rng slices live in the context's own buffer (d_admit_rng)
  std::lock_guard<std::mutex> admission(c->admit_mu);
  std::unique_lock<std::mutex> replay;      // the replay form: the staged secrets and the derived nonces of its tail (d_replay)
  if (rp) replay = std::unique_lock<std::mutex>(c->replay_mu);
  const size_t pb = act_spend_proof_bytes(c), out_b = redeem_out_bytes(c, wire, ret);
  const CborType* T = cbor_type(ACT_CBOR_SPEND_PROOF);
  CborLayout lay; if (wire) lay = cbor_layout(*T, c->L);
  const size_t ml = lay.tmpl.size(), nf = lay.pay_off.size();
  const WireExtent ext{cbor, offsets, ml};      // where message i lies (wire callers)
  hipStream_t stream = set->stream;

  // ---- the stage's own device memory (public data: lane numbers, codes, nullifiers, charges) -------------------------------------------
  const size_t nb = (n + ADMIT_BLOCK - 1) / ADMIT_BLOCK, fcap = (n + 3) & ~(size_t)3;
  size_t need = 0;
  auto take = [&](size_t bytes) { const size_t at = need; need += (bytes + 15) & ~(size_t)15; return at; };
  const size_t o_pre = take(n), o_kred = take(n * 32), o_idx = take(n * 4), o_pos = take(n * 4), o_blk = take(nb * 4), o_total = take(4);
  const bool own_ks = wire || !dev;
  const size_t o_ks = own_ks ? take(n * 64) : 0, o_charge = (charge && !dev) ? take(n * 32) : 0;
  const uint8_t* const t_in = ret ? ret->t : nullptr;      // the returned amounts, n scalars in the caller's kind of memory (null: all zero)
  const size_t o_ret = (t_in && !dev) ? take(n * 32) : 0;
  const size_t o_code = wire ? take(n) : 0, o_flags = (wire && dev) ? take(fcap) : 0, o_off = (wire && dev && offsets) ? take((n + 1) * 8) : 0;
  const size_t o_tmpl = (wire && dev) ? take(ml) : 0, o_pay = (wire && dev) ? take(nf * 4) : 0;
  const size_t o_pwhich = wire ? take(WIRE_SETTLE_WINDOW * 4) : 0, o_patch = wire ? take(WIRE_SETTLE_WINDOW * 64) : 0;
  const bool dev_reader = wire && c->wire_reader.load() == ACT_WIRE_READER_DEVICE;
  const size_t o_rcode = (dev_reader && dev) ? take(2 * n) : 0;      // the device reader's codes, then its infos
  DevTmp d(c);
  if ((rc = d.alloc(need))) return rc;
  ADCK(c, hipSetDevice(c->device));
  uint8_t* const d_pre = d.p + o_pre; uint8_t* const d_kred = d.p + o_kred;
  uint32_t* const d_idx = reinterpret_cast<uint32_t*>(d.p + o_idx); uint32_t* const d_pos = reinterpret_cast<uint32_t*>(d.p + o_pos);
  uint32_t* const d_blk = reinterpret_cast<uint32_t*>(d.p + o_blk); uint32_t* const d_total = reinterpret_cast<uint32_t*>(d.p + o_total);
  uint8_t* const d_ks = d.p + o_ks;

  // ---- step 1: where k and s are ------------------------------------------------------------------------------------------------------
  AdmitScreenArgs sa{};
  sa.n = (uint32_t)n; sa.pre = d_pre; sa.kred = d_kred;
  std::vector<uint8_t> h_code;
  if (!wire) {
    if (dev) { sa.ks = proof; sa.stride = (uint32_t)pb; }
    else { ADCK(c, hipMemcpy2DAsync(d_ks, 64, proof, pb, 64, n, hipMemcpyHostToDevice, stream)); sa.ks = d_ks; sa.stride = 64; }      // the 64-byte fields only
  } else {
    std::vector<uint8_t> flags(fcap, 0), h_ks;
    if (dev) {
      uint8_t* d_flags = d.p + o_flags;
      ADCK(c, hipMemsetAsync(d_flags, 0, fcap, stream));
      ADCK(c, hipMemcpyAsync(d.p + o_tmpl, lay.tmpl.data(), ml, hipMemcpyHostToDevice, stream));
      ADCK(c, hipMemcpyAsync(d.p + o_pay, lay.pay_off.data(), nf * 4, hipMemcpyHostToDevice, stream));
      if (offsets) ADCK(c, hipMemcpyAsync(d.p + o_off, offsets, (n + 1) * 8, hipMemcpyHostToDevice, stream));
      for (size_t off = 0; off < n; off += ADMIT_WIRE_LAUNCH) {      // (off is a multiple of 4: the flag words of two launches do not overlap)
        AdmitWireArgs a{};
        a.n = (uint32_t)std::min(ADMIT_WIRE_LAUNCH, n - off); a.n_fields = (uint32_t)nf; a.msg_len = (uint32_t)ml;
        a.cbor = offsets ? cbor : cbor + off * ml; a.offsets = offsets ? reinterpret_cast<const uint64_t*>(d.p + o_off) + off : nullptr;
        a.tmpl = d.p + o_tmpl; a.pay_off = reinterpret_cast<const uint32_t*>(d.p + o_pay); a.ks = d_ks + off * 64; a.flags = d_flags + off;
        launch_admit_wire(a, stream);
      }
      if (dev_reader) {      // every other spelling: the reader's reduced form over the flagged messages, k and s into d_ks, the codes for the screen
        ADCK(c, hipMemsetAsync(d.p + o_rcode, 0, 2 * n, stream));
        CborReadArgs ra{};
        ra.T = *T; ra.L = c->L; ra.n = (uint32_t)n; ra.first = 0; ra.msg_len = (uint32_t)ml; ra.in = cbor; ra.offsets = offsets ? reinterpret_cast<const uint64_t*>(d.p + o_off) : nullptr;
        ra.flags = d_flags; ra.rec = d_ks; ra.rec_stride = 64; ra.keep_fields = 2; ra.code = d.p + o_rcode; ra.info = d.p + o_rcode + n;
        launch_cbor_read(ra, false, stream);
        launch_cbor_read(ra, true, stream);
        CborCodeArgs ca{(uint32_t)n, ra.code, ra.info, d.p + o_code};
        launch_cbor_wire_code(ca, stream);
      }
      ADCK(c, hipGetLastError());
      ADCK(c, hipMemcpyAsync(flags.data(), d_flags, fcap, hipMemcpyDeviceToHost, stream));
      ADCK(c, hipStreamSynchronize(stream));
    } else {      // host memory: the same lane body on the host workers, 64 bytes per message cross the link
      h_ks.assign(n * 64, 0);
      AdmitWireJob job{};
      job.a.n = (uint32_t)n; job.a.n_fields = (uint32_t)nf; job.a.msg_len = (uint32_t)ml; job.a.cbor = cbor; job.a.offsets = offsets;
      job.a.tmpl = lay.tmpl.data(); job.a.pay_off = lay.pay_off.data(); job.a.ks = h_ks.data(); job.a.flags = flags.data();
      act_host_parallel_for(n, 256, 0, [](void* p, size_t i0, size_t i1) {
        const AdmitWireArgs& a = static_cast<AdmitWireJob*>(p)->a;
        for (size_t m = i0; m < i1; m++) {
          bool canon = true;
          for (uint32_t f = 0; f < a.n_fields && canon; f++) canon = admit_wire_piece(a, (uint32_t)m, f);
          a.flags[m] = canon ? 0 : 0x80;
        }
      }, &job);
      h_code.assign(n, 0);
      if (dev_reader) {      // the reader's lane body on the host workers, both passes of a message one behind the other
        std::vector<uint8_t> rinfo(n, 0);
        AdmitReadJob rj{};
        rj.a.T = *T; rj.a.L = c->L; rj.a.n = (uint32_t)n; rj.a.first = 0; rj.a.msg_len = (uint32_t)ml; rj.a.in = cbor; rj.a.offsets = offsets;
        rj.a.flags = flags.data(); rj.a.rec = h_ks.data(); rj.a.rec_stride = 64; rj.a.keep_fields = 2; rj.a.code = h_code.data(); rj.a.info = rinfo.data();
        act_host_parallel_for(n, 64, 0, [](void* p, size_t i0, size_t i1) {
          const CborReadArgs& a = static_cast<AdmitReadJob*>(p)->a;
          uint32_t st[CBOR_MAX_DEPTH];
          for (size_t m = i0; m < i1; m++) {
            cbor_read_message_lane<false>(a, (uint32_t)m, st);
            cbor_read_message_lane<true>(a, (uint32_t)m, st);
            a.code[m] = cbor_code_status(a.code[m]);      // (an unflagged message keeps its 0)
          }
        }, &rj);
      }
      ADCK(c, hipMemcpyAsync(d_ks, h_ks.data(), n * 64, hipMemcpyHostToDevice, stream));
      ADCK(c, hipStreamSynchronize(stream));
    }
    // every other spelling: the general reader, a window at a time (wire_window_read).  A message that reads yields the record, and so
    // k and s; one that does not takes the status act_redeem_cbor_* gives it (the first error in wire order: cbor_settle_codes)
    if (h_code.size() != n) h_code.assign(n, 0);
    std::vector<size_t> which;
    for (size_t i = 0; i < n; i++) if (flags[i] & 0x80) which.push_back(i);
    c->wire_stats[0] += n; c->wire_stats[1] += n - which.size(); c->wire_stats[dev_reader ? 2 : 3] += which.size();
    if (dev_reader) which.clear();      // read already: the serial window loop below is the road of ACT_WIRE_READER_HOST
    WireWindow win; std::vector<uint8_t> patch; std::vector<uint32_t> pwhich;
    for (size_t w0 = 0; w0 < which.size(); w0 += WIRE_SETTLE_WINDOW) {
      const size_t cnt = std::min(which.size(), w0 + WIRE_SETTLE_WINDOW) - w0;
      const size_t* lanes = which.data() + w0;
      if ((rc = wire_window_read(c, stream, *T, ext, dev, lanes, cnt, pb, win))) return rc;
      patch.clear(); pwhich.clear();
      for (size_t k = 0; k < cnt; k++) {
        if (win.codes[k] != CBOR_OK) { h_code[lanes[k]] = win.status[k]; continue; }
        patch.insert(patch.end(), win.recs.data() + k * pb, win.recs.data() + k * pb + 64);      // k and s: the record's first two fields
        pwhich.push_back((uint32_t)lanes[k]);
      }
      if (const size_t np = pwhich.size()) {
        ADCK(c, hipMemcpyAsync(d.p + o_pwhich, pwhich.data(), np * 4, hipMemcpyHostToDevice, stream));
        ADCK(c, hipMemcpyAsync(d.p + o_patch, patch.data(), np * 64, hipMemcpyHostToDevice, stream));
        AdmitPatchArgs pa{d_ks, reinterpret_cast<const uint32_t*>(d.p + o_pwhich), d.p + o_patch, (uint32_t)np};
        launch_admit_patch(pa, stream);
        ADCK(c, hipGetLastError());
        ADCK(c, hipStreamSynchronize(stream));      // pwhich / patch are reused by the next window
      }
    }
    if (!(dev_reader && dev)) ADCK(c, hipMemcpyAsync(d.p + o_code, h_code.data(), n, hipMemcpyHostToDevice, stream));
    sa.ks = d_ks; sa.stride = 64; sa.wire_code = d.p + o_code;
  }
  if (charge) {
    if (dev) sa.charge = charge;
    else { ADCK(c, hipMemcpyAsync(d.p + o_charge, charge, n * 32, hipMemcpyHostToDevice, stream)); sa.charge = d.p + o_charge; }
  }
  if (t_in) {      // t <= s is the screen's rule, in the pass that compares the charge
    if (dev) sa.returned = t_in;
    else { ADCK(c, hipMemcpyAsync(d.p + o_ret, t_in, n * 32, hipMemcpyHostToDevice, stream)); sa.returned = d.p + o_ret; }
  }

  // ---- steps 1 and 2: the screen (the set's lock is held while its table is read) and the compaction ----------------------------------
  uint32_t m32 = 0;
  std::vector<uint8_t> h_pre(n);
  {
    std::lock_guard<std::mutex> lk(set->mu);
    sa.tab_keys = set->tab_keys; sa.tab_state = set->tab_state; sa.tab_cap = set->tab_cap; memcpy(sa.salt.w, set->salt, 16);
    launch_admit_screen(sa, stream);
    if (!rp) launch_admit_compact(d_pre, (uint32_t)n, d_blk, d_idx, d_pos, d_total, stream);
    ADCK(c, hipGetLastError());
    if (!rp) {
      ADCK(c, hipMemcpyAsync(&m32, d_total, 4, hipMemcpyDeviceToHost, stream));
      ADCK(c, hipMemcpyAsync(h_pre.data(), d_pre, n, hipMemcpyDeviceToHost, stream));
    }
    ADCK(c, hipStreamSynchronize(stream));
  }
  if (rp) {      // the spent lanes: retry candidates go on, the others stay double spends; then the compaction over what that leaves
    const AdmitReplayStage g{stream, n, dev, wire, dev_reader, proof, cbor, &ext, offsets != nullptr, d_pre, d_kred, d_blk, d_idx, d_pos, d_total, sa.returned};
    if ((rc = admit_replay_stage(c, *rp, g))) return rc;
    launch_admit_compact(d_pre, (uint32_t)n, d_blk, d_idx, d_pos, d_total, stream);
    ADCK(c, hipGetLastError());
    ADCK(c, hipMemcpyAsync(&m32, d_total, 4, hipMemcpyDeviceToHost, stream));
    ADCK(c, hipMemcpyAsync(h_pre.data(), d_pre, n, hipMemcpyDeviceToHost, stream));
    ADCK(c, hipStreamSynchronize(stream));
  }
  const size_t m = m32;
  if (m > n) { c->err = "admission: the compaction counted more survivors than lanes"; return ACT_ERR_HIP; }

  // ---- step 3a (the unique forms): a survivor with the bytes of an earlier survivor is a copy and is not verified -----------------------
  // mv lanes are verified: v_idx / v_pos / v_pre are the screen's arrays, or the copy stage's when it found copies
  AdmitCopies cp(c);
  std::vector<uint32_t> h_idx, h_lead;
  const uint8_t* v_pre = d_pre; const uint32_t *v_idx = d_idx, *v_pos = d_pos; size_t mv = m;
  if (unique && m >= 2) {
    if (!dev) { h_idx.resize(m); ADCK(c, hipMemcpy(h_idx.data(), d_idx, m * 4, hipMemcpyDeviceToHost)); }
    CopySpan span{wire ? cbor : proof, nullptr, wire ? ml : pb};
    if (wire && offsets) span.offsets = dev ? reinterpret_cast<const uint64_t*>(d.p + o_off) : offsets;
    uint32_t salt[4];
    { std::lock_guard<std::mutex> lk(set->mu); memcpy(salt, set->salt, 16); }
    if ((rc = cp.run(stream, dev, n, m, span, d_pre, d_idx, h_idx.data(), salt))) return rc;
    if (cp.copies) {
      v_pre = cp.d_pre2; v_idx = cp.d_idx2; v_pos = cp.d_pos2; mv = cp.m2;
      if (!dev) { h_lead.resize(n); ADCK(c, hipMemcpy(h_lead.data(), cp.d_lead, n * 4, hipMemcpyDeviceToHost)); }
    }
  }

  // ---- nothing shed: the honest batch pays the screen and nothing else ------------------------------------------------------------------
  if (mv == n && rp) {
    uint64_t tc[ACT_REPLAY_COUNTS] = {0, 0, 0, 0, 0, 0};
    rc = redeem_replay_locked(c, set, rp->receipts, n, mem, keys, nkeys, key_epochs, sign_key, proof, cbor, offsets, rp->nonce_key, out, status, out_key, rp->out_replayed,
                              rp->out_counts ? tc : nullptr, ret);      // (the caller's `returned`, lane for lane)
    if (rp->out_counts && tc[0] == n) admit_replay_counts_of(rp->out_counts, n, h_pre.data(), rp->candidates, n, tc, ret != nullptr);      // (tc[0] == 0: the call ended before its tail)
    return rc;
  }
  if (mv == n) {
    rc = redeem_keyring_impl(c, set, n, mem, keys, nkeys, key_epochs, sign_key, proof, cbor, offsets, rng, rng_mode, out, status, out_key, ret);
    if (out_counts && (rc == ACT_OK || rc == ACT_ERR_ARG)) {      // (ACT_ERR_ARG: the nullifier step refused lanes; status[] is complete)
      std::vector<uint8_t> hs;
      const uint8_t* s = status;
      if (dev) { hs.resize(n); if (hipMemcpy(hs.data(), status, n, hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return rc; } s = hs.data(); }
      admit_counts_of(out_counts, n, h_pre.data(), n, s, ret != nullptr);      // (copies: 0)
    }
    return rc;
  }
  // ---- everything shed: no verification, nothing recorded, no rng drawn -----------------------------------------------------------------
  if (mv == 0) {
    if ((rc = redeem_keyring_impl(c, set, 0, mem, keys, nkeys, key_epochs, sign_key, nullptr, nullptr, nullptr, rng, rng_mode, nullptr, nullptr, nullptr))) return rc;      // a bad ring fails the call whatever is shed
    if (dev) {
      ADCK(c, hipMemcpyAsync(status, d_pre, n, hipMemcpyDeviceToDevice, stream));
      ADCK(c, hipMemsetAsync(out_key, ACT_KEY_NONE, n, stream));
      ADCK(c, hipMemsetAsync(out, 0, n * out_b, stream));
      if (rp && rp->out_replayed) ADCK(c, hipMemsetAsync(rp->out_replayed, 0, n, stream));
      ADCK(c, hipStreamSynchronize(stream));
    } else { memcpy(status, h_pre.data(), n); memset(out_key, ACT_KEY_NONE, n); memset(out, 0, n * out_b); if (rp && rp->out_replayed) memset(rp->out_replayed, 0, n); }
    admit_counts_of(out_counts, n, h_pre.data(), 0, nullptr, ret != nullptr);
    if (rp && rp->out_counts) admit_replay_counts_of(rp->out_counts, n, h_pre.data(), 0, 0, nullptr, ret != nullptr);
    return ACT_OK;
  }

  // ---- step 3: the survivors, a window at a time -------------------------------------------------------------------------------------------
  std::vector<uint32_t> h_pos;
  h_idx.resize(mv);
  ADCK(c, hipMemcpy(h_idx.data(), v_idx, mv * 4, hipMemcpyDeviceToHost));
  if (!dev) { h_pos.resize(n); ADCK(c, hipMemcpy(h_pos.data(), v_pos, n * 4, hipMemcpyDeviceToHost)); }
  // compact arrays in the caller's kind of memory: K' | nullifiers | verdicts | look-up answers | key indices | matched keys | statuses
  AdmitArr arr(c), cout(c);
  const size_t arr_lane = rp ? 70 : 69;
  if ((rc = arr.alloc(mem, mv * arr_lane + (t_in ? mv * 32 + 32 : 0)))) { c->err = "admission: compact arrays"; return rc; }
  if ((rc = cout.alloc(mem, mv * out_b))) { c->err = "admission: compact output"; return rc; }
  uint8_t *kp = arr.p, *knul = kp + mv * 32, *st = knul + mv * 32, *sp = st + mv, *kidx = sp + mv, *okey = kidx + mv, *cst = okey + mv,
          *crepl = cst + mv;      // (the replay form: the survivors' replay marks)
  // a survivor's status that the tail leaves unwritten (it returns early only on a device failure BEHIND check-and-insert) must never
  // read as accepted: recorded, not signed
  if (dev) { ADCK(c, hipMemset(cst, ACT_STATUS_RECORDED_UNSIGNED, mv)); ADCK(c, hipDeviceSynchronize()); } else memset(cst, ACT_STATUS_RECORDED_UNSIGNED, mv);
  {      // the reduced nullifiers of the survivors, as the screen left them
    DevTmp g(c); uint8_t* dst = knul;
    if (!dev) { if ((rc = g.alloc(mv * 32))) return rc; dst = g.p; }
    AdmitRowsArgs ra{dst, d_kred, v_idx, (uint32_t)mv, 32};
    launch_admit_rows(ra, stream);
    ADCK(c, hipGetLastError());
    if (!dev) ADCK(c, hipMemcpyAsync(knul, g.p, mv * 32, hipMemcpyDeviceToHost, stream));
    ADCK(c, hipStreamSynchronize(stream));
  }
  // the per-lane rng slices follow their lanes (secret: staged in the context's own buffer or a host vector, wiped on every exit)
  AdmitRngDev rng_dev(c); std::vector<uint8_t> rng_host; AdmitHostWipe rng_wipe{rng_host};
  const uint8_t* c_rng = rng;
  if (rng_mode == ACT_RNG_PER_LANE && !rp) {
    if (dev) {
      if ((rc = rng_dev.reserve(mv * 128))) return rc;
      AdmitRowsArgs ra{c->d_admit_rng, rng, v_idx, (uint32_t)mv, 128};
      launch_admit_rows(ra, stream);
      ADCK(c, hipGetLastError());
      ADCK(c, hipStreamSynchronize(stream));
      c_rng = c->d_admit_rng;
    } else {
      rng_host.resize(mv * 128);
      for (size_t j = 0; j < mv; j++) memcpy(rng_host.data() + j * 128, rng + (size_t)h_idx[j] * 128, 128);
      c_rng = rng_host.data();
    }
  }
  // the returned amounts follow their lanes too (public; the compact copy lies behind the other compact arrays, 32-byte aligned).  Like
  // the rng slices they are gathered by v_idx: in the unique forms the amounts of the lanes that are verified -- a copy's t is never read
  RedeemReturn cret{nullptr};
  if (t_in) {
    uint8_t* ct = arr.p + ((mv * arr_lane + 31) & ~(size_t)31);
    if (dev) {
      AdmitRowsArgs ra{ct, t_in, v_idx, (uint32_t)mv, 32};
      launch_admit_rows(ra, stream);
      ADCK(c, hipGetLastError());
      ADCK(c, hipStreamSynchronize(stream));
    } else for (size_t j = 0; j < mv; j++) memcpy(ct + j * 32, t_in + (size_t)h_idx[j] * 32, 32);
    cret.t = ct;
  }
  const size_t W = std::max<size_t>(1, ADMIT_WINDOW_BATCHES * c->max_batch);
  AdmitGather gather(c, stream, dev, wire ? cbor : proof, wire ? ml : pb, (wire && offsets) ? &ext : nullptr);
  for (size_t w0 = 0; w0 < mv; w0 += W) {
    const size_t w = std::min(W, mv - w0);
    if ((rc = gather.run(v_idx + w0, h_idx.data() + w0, w))) return rc;
    const uint8_t* g = gather.data();
    if (wire) { RingSel sel{keys, nkeys, okey + w0}; rc = verify_spend_cbor_impl(c, w, mem, nullptr, g, gather.offsets(), st + w0, kp + w0 * 32, nullptr, &sel); }
    else rc = act_verify_spend_keyring_batch(c, w, mem, keys, nkeys, g, st + w0, okey + w0, kp + w0 * 32);
    if (rc) return rc;            // as in the redeem calls: nothing recorded, status untouched
  }

  // ---- step 4: once per call, over the compact arrays ---------------------------------------------------------------------------------------
  uint64_t tc[ACT_REPLAY_COUNTS] = {0, 0, 0, 0, 0, 0};
  bool began = false;
  const int rc_tail = rp ? replay_tail(c, set, rp->receipts, mv, mem, keys, nkeys, key_epochs, sign_key, wire, knul, 32, kp, st, rp->nonce_key, cout.p, cst, okey, crepl, tc, &began, ret ? &cret : nullptr)
                         : redeem_tail_ring(c, set, mv, mem, keys, nkeys, key_epochs, sign_key, wire, knul, 32, kp, st, sp, kidx, c_rng, rng_mode, cout.p, cst, okey, ret ? &cret : nullptr);

  if (rp && rc_tail && !began) return rc_tail;      // staging its buffers failed: as a failed verification -- nothing recorded, status untouched
  // ---- step 5: the answers back to their lanes (also behind a failure of step 4: status[] is complete on return) ----------------------------
  std::vector<uint8_t> h_cst, h_fin, h_t;      // h_fin, h_t: the final statuses and the amounts of a device-memory caller (the replay unique forms' copy counts)
  if (dev) {
    AdmitScatterArgs sc{}; sc.n = (uint32_t)n; sc.out_bytes = out_b; sc.pos = v_pos; sc.pre = v_pre; sc.c_status = cst; sc.c_key = okey; sc.c_out = cout.p;
    sc.status = status; sc.out_key = out_key; sc.out = out;
    launch_admit_scatter(sc, stream);
    if (cp.copies && !rp) { CopyResolveArgs ra{cp.d_lead, (uint32_t)n, status, out_key}; launch_copy_resolve(ra, stream); }      // COPY_MARK leaves status[] here
    if (rp && rp->out_replayed) {      // the replay marks ride the same scatter as one-byte records (a shed lane: 0)
      AdmitScatterArgs sr = sc; sr.out_bytes = 1; sr.c_out = crepl; sr.out = rp->out_replayed;
      launch_admit_scatter(sr, stream);
    }
    // the replay unique forms: behind both scatters the rows of leaders are final; a copy takes its leader's whole answer
    // (with amounts: only if it names its leader's -- a copy's t is read here and nowhere else)
    if (cp.copies && rp) {
      const CopyServeArgs va{cp.d_lead, (uint32_t)n, out_b, status, out_key, out, rp->out_replayed};
      if (ret) { CopyServeReturnArgs vr{va, t_in}; launch_copy_serve_return(vr, stream); } else launch_copy_serve(va, stream);
    }
    ADCK(c, hipGetLastError());
    if (out_counts) { h_cst.resize(mv); ADCK(c, hipMemcpyAsync(h_cst.data(), cst, mv, hipMemcpyDeviceToHost, stream)); }
    if (cp.copies && rp && rp->out_counts) {      // copies_served is counted on the final statuses
      h_lead.resize(n); h_fin.resize(n);
      ADCK(c, hipMemcpyAsync(h_lead.data(), cp.d_lead, n * 4, hipMemcpyDeviceToHost, stream));
      ADCK(c, hipMemcpyAsync(h_fin.data(), status, n, hipMemcpyDeviceToHost, stream));
      if (t_in) { h_t.resize(n * 32); ADCK(c, hipMemcpyAsync(h_t.data(), t_in, n * 32, hipMemcpyDeviceToHost, stream)); }
    }
    ADCK(c, hipStreamSynchronize(stream));
  } else {
    for (size_t i = 0; i < n; i++) {
      const uint32_t j = h_pos[i];
      if (j == ADMIT_SHED) { status[i] = h_pre[i]; out_key[i] = ACT_KEY_NONE; memset(out + i * out_b, 0, out_b); }
      else { status[i] = cst[j]; out_key[i] = okey[j]; memcpy(out + i * out_b, cout.p + (size_t)j * out_b, out_b); }
      if (rp && rp->out_replayed) rp->out_replayed[i] = j == ADMIT_SHED ? 0 : crepl[j];
    }
    if (cp.copies && !rp) { CopyResolveArgs ra{h_lead.data(), (uint32_t)n, status, out_key}; for (size_t i = 0; i < n; i++) copy_resolve_lane(ra, (uint32_t)i); }
    if (cp.copies && rp && ret) { CopyServeReturnArgs vr{{h_lead.data(), (uint32_t)n, out_b, status, out_key, out, rp->out_replayed}, t_in}; for (size_t i = 0; i < n; i++) copy_serve_return_lane(vr, (uint32_t)i); }
    else if (cp.copies && rp) { CopyServeArgs va{h_lead.data(), (uint32_t)n, out_b, status, out_key, out, rp->out_replayed}; for (size_t i = 0; i < n; i++) copy_serve_lane(va, (uint32_t)i); }
  }
  admit_counts_of(out_counts, n, h_pre.data(), mv, dev ? h_cst.data() : cst, ret != nullptr);
  if (rp && rp->out_counts && tc[0] == mv) admit_replay_counts_of(rp->out_counts, n, h_pre.data(), rp->candidates, mv, tc, ret != nullptr);
  if (out_counts && unique) out_counts[ret ? ACT_REDEEM_RETURN_COUNTS : ACT_ADMIT_COUNTS] = cp.copies;
  if (rp && rp->out_counts && unique && cp.copies && tc[0] == mv) {      // copies, then the copies whose leader ended 0
    const uint8_t* fin = dev ? h_fin.data() : status;
    uint64_t served = 0, other = 0;
    for (size_t i = 0; i < n; i++) served += h_lead[i] != COPY_NONE && fin[i] == 0;
    uint64_t* const at = rp->out_counts + (ret ? ACT_RETURN_REPLAY_COUNTS : ACT_ADMIT_REPLAY_COUNTS);
    at[0] = cp.copies; at[1] = served;
    if (ret) {      // the return form: then the copies that name another amount than their leader (no amounts: none does)
      const uint8_t* t = dev ? h_t.data() : t_in;
      if (t_in) for (size_t i = 0; i < n; i++) other += h_lead[i] != COPY_NONE && !copy_same_amount(t + i * 32, t + (size_t)h_lead[i] * 32);
      at[2] = other;
    }
  }
  return rc_tail;
}

extern "C" int act_redeem_admit_batch(act_ctx* c, act_nullifier_set* set, size_t n, int mem, const uint8_t* keys, int nkeys, const uint32_t* key_epochs, int sign_key,
                                      const uint8_t* proof, const uint8_t* charge, const uint8_t* rng, int rng_mode, uint8_t* out_refund, uint8_t* status,
                                      uint8_t* out_key, uint64_t* out_counts) {
  if (n && !proof) return ACT_ERR_ARG;
  return redeem_admit_impl(c, set, n, mem, keys, nkeys, key_epochs, sign_key, proof, nullptr, nullptr, charge, rng, rng_mode, out_refund, status, out_key, out_counts);
}
extern "C" int act_redeem_cbor_admit_batch(act_ctx* c, act_nullifier_set* set, size_t n, int mem, const uint8_t* keys, int nkeys, const uint32_t* key_epochs, int sign_key,
                                           const uint8_t* cbor, const uint64_t* offsets, const uint8_t* charge, const uint8_t* rng, int rng_mode,
                                           uint8_t* out_refund_cbor, uint8_t* status, uint8_t* out_key, uint64_t* out_counts) {
  if (n && !cbor) return ACT_ERR_ARG;
  static const uint8_t none = 0;
  return redeem_admit_impl(c, set, n, mem, keys, nkeys, key_epochs, sign_key, nullptr, cbor ? cbor : &none, offsets, charge, rng, rng_mode, out_refund_cbor, status,
                           out_key, out_counts);
}
extern "C" int act_redeem_admit_unique_batch(act_ctx* c, act_nullifier_set* set, size_t n, int mem, const uint8_t* keys, int nkeys, const uint32_t* key_epochs,
                                             int sign_key, const uint8_t* proof, const uint8_t* charge, const uint8_t* rng, int rng_mode, uint8_t* out_refund,
                                             uint8_t* status, uint8_t* out_key, uint64_t* out_counts) {
  if (n && !proof) return ACT_ERR_ARG;
  return redeem_admit_impl(c, set, n, mem, keys, nkeys, key_epochs, sign_key, proof, nullptr, nullptr, charge, rng, rng_mode, out_refund, status, out_key, out_counts,
                           true);
}
extern "C" int act_redeem_cbor_admit_unique_batch(act_ctx* c, act_nullifier_set* set, size_t n, int mem, const uint8_t* keys, int nkeys, const uint32_t* key_epochs,
                                                  int sign_key, const uint8_t* cbor, const uint64_t* offsets, const uint8_t* charge, const uint8_t* rng, int rng_mode,
                                                  uint8_t* out_refund_cbor, uint8_t* status, uint8_t* out_key, uint64_t* out_counts) {
  if (n && !cbor) return ACT_ERR_ARG;
  static const uint8_t none = 0;
  return redeem_admit_impl(c, set, n, mem, keys, nkeys, key_epochs, sign_key, nullptr, cbor ? cbor : &none, offsets, charge, rng, rng_mode, out_refund_cbor, status,
                           out_key, out_counts, true);
}

// ---- partial refunds (DESIGN 4.10): the admission calls with the amounts t the issuer returns ---------------------------------------------
// The admission loop with one more rule in the screen (t_i > s_i -> ACT_STATUS_RETURN_TOO_BIG, behind the charge and in front of the
// look-up) and a signing step over X_A = g + K' + t h1; 160-byte RefundReturn records or ACT_CBOR_REFUND_RETURN messages.  Drawn nonces
// here; the replay form with amounts is act_redeem_(cbor_)return_replay_batch (admit_replay_impl.inc), where t enters the receipt's tag
// and the nonce derivation -- with e derived from (nonce_key, key, k, enc(K')) alone, two signatures with one e over X_A that differ by
// a multiple of h1 would give h1 (e + x)^-1 away.
extern "C" int act_redeem_return_batch(act_ctx* c, act_nullifier_set* set, size_t n, int mem, const uint8_t* keys, int nkeys, const uint32_t* key_epochs, int sign_key,
                                       const uint8_t* proof, const uint8_t* charge, const uint8_t* returned, const uint8_t* rng, int rng_mode,
                                       uint8_t* out_refund_return, uint8_t* status, uint8_t* out_key, uint64_t* out_counts) {
  if (n && !proof) { if (out_counts) memset(out_counts, 0, sizeof(uint64_t) * ACT_REDEEM_RETURN_COUNTS); return ACT_ERR_ARG; }
  const RedeemReturn ret{returned};
  return redeem_admit_impl(c, set, n, mem, keys, nkeys, key_epochs, sign_key, proof, nullptr, nullptr, charge, rng, rng_mode, out_refund_return, status, out_key,
                           out_counts, false, nullptr, &ret);
}
extern "C" int act_redeem_cbor_return_batch(act_ctx* c, act_nullifier_set* set, size_t n, int mem, const uint8_t* keys, int nkeys, const uint32_t* key_epochs,
                                            int sign_key, const uint8_t* cbor, const uint64_t* offsets, const uint8_t* charge, const uint8_t* returned,
                                            const uint8_t* rng, int rng_mode, uint8_t* out_refund_return_cbor, uint8_t* status, uint8_t* out_key,
                                            uint64_t* out_counts) {
  if (n && !cbor) { if (out_counts) memset(out_counts, 0, sizeof(uint64_t) * ACT_REDEEM_RETURN_COUNTS); return ACT_ERR_ARG; }
  static const uint8_t none = 0;
  const RedeemReturn ret{returned};
  return redeem_admit_impl(c, set, n, mem, keys, nkeys, key_epochs, sign_key, nullptr, cbor ? cbor : &none, offsets, charge, rng, rng_mode, out_refund_return_cbor,
                           status, out_key, out_counts, false, nullptr, &ret);
}

// The return calls with the copy stage of the unique forms in its usual place, behind the screen and in front of verification.  Equality
// is decided on the proof bytes alone: t takes no part in it, because what a lane that passed the screen is answered depends on t only if
// it is the lane that is signed, and that lane is the leader -- in act_redeem_(cbor_)return_batch lanes that share a fresh nullifier are
// all verified and the first valid one in lane order wins, whatever the others' t.  A lane the screen sheds (t > s among the reasons) is
// neither a leader nor a copy.  out_counts: ACT_REDEEM_RETURN_UNIQUE_COUNTS values.
extern "C" int act_redeem_return_unique_batch(act_ctx* c, act_nullifier_set* set, size_t n, int mem, const uint8_t* keys, int nkeys, const uint32_t* key_epochs,
                                              int sign_key, const uint8_t* proof, const uint8_t* charge, const uint8_t* returned, const uint8_t* rng, int rng_mode,
                                              uint8_t* out_refund_return, uint8_t* status, uint8_t* out_key, uint64_t* out_counts) {
  if (n && !proof) { if (out_counts) memset(out_counts, 0, sizeof(uint64_t) * ACT_REDEEM_RETURN_UNIQUE_COUNTS); return ACT_ERR_ARG; }
  const RedeemReturn ret{returned};
  return redeem_admit_impl(c, set, n, mem, keys, nkeys, key_epochs, sign_key, proof, nullptr, nullptr, charge, rng, rng_mode, out_refund_return, status, out_key,
                           out_counts, true, nullptr, &ret);
}
extern "C" int act_redeem_cbor_return_unique_batch(act_ctx* c, act_nullifier_set* set, size_t n, int mem, const uint8_t* keys, int nkeys, const uint32_t* key_epochs,
                                                   int sign_key, const uint8_t* cbor, const uint64_t* offsets, const uint8_t* charge, const uint8_t* returned,
                                                   const uint8_t* rng, int rng_mode, uint8_t* out_refund_return_cbor, uint8_t* status, uint8_t* out_key,
                                                   uint64_t* out_counts) {
  if (n && !cbor) { if (out_counts) memset(out_counts, 0, sizeof(uint64_t) * ACT_REDEEM_RETURN_UNIQUE_COUNTS); return ACT_ERR_ARG; }
  static const uint8_t none = 0;
  const RedeemReturn ret{returned};
  return redeem_admit_impl(c, set, n, mem, keys, nkeys, key_epochs, sign_key, nullptr, cbor ? cbor : &none, offsets, charge, rng, rng_mode, out_refund_return_cbor,
                           status, out_key, out_counts, true, nullptr, &ret);
}
