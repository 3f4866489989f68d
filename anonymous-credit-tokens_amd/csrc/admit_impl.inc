// admit_impl.inc — included by engine.hip after keyring_redeem_impl.inc: admission before verification (DESIGN 4.7; kernels in
// k_admit.hip, lane bodies in admit_lanes.h).  act_redeem_admit_batch / act_redeem_cbor_admit_batch are the ring redeem calls with a
// screen in front: per lane the charge is compared with the expected one and the nullifier is looked up (read only) BEFORE the proof
// is verified, and only the lanes that pass go through verification -> check-and-insert -> sign.
// Every entry point of the family fills one AdmitCall -- the ring, the input, the prices, the rng or the replay part, the outputs and the
// form (unique: the copy stage, copies_impl.inc [k_copies.hip]; replay: receipts and the replay tail, admit_replay_impl.inc, DESIGN 4.9;
// ret: returned amounts and RefundReturn outputs, DESIGN 4.10; reserve: the replay form without its signature half and with 96-byte
// reservation records out, reserve_impl.inc, DESIGN 4.11) -- and calls redeem_admit, which runs the stages of AdmitState in order:
//   refusals         admit_refused: everything refused as a whole, before anything is looked at; n == 0 is the empty ring call
//   locate_ks        k and s of every lane (records: fields 0 and 1; wire, wire_ks: the payloads of a canonical message, and of any other
//                    spelling what the wire reader's reduced form gives -- cbor_lanes.h with keep_fields = 2, as a kernel for
//                    device-memory callers and on the host workers for host-memory callers; under ACT_WIRE_READER_HOST the host
//                    reader's record, in windows of WIRE_SETTLE_WINDOW: wire_window_read, cbor_impl.inc); the charges and amounts
//   screen           pre-status and reduced k [k_admit_screen]; replay: the stage that lets a spent lane whose receipt is this proof's own
//                    survive as a retry candidate (with amounts: the tag takes the lane's t); then the survivors' lane numbers in lane
//                    order                                                                          [k_admit_count / _scan / _write]
//   copy_stage       unique: a survivor whose input bytes are those of an earlier survivor is not verified (with amounts: equality is
//                    decided on the proof bytes alone); leaves the arrays of the lanes that ARE verified in cp.v
//   nothing_shed     every lane is verified: the caller's pointers go straight to redeem_keyring_impl (replay: redeem_replay_locked)
//   everything_shed  no verification kernel runs, nothing is recorded, no rng is drawn
//   compact_inputs   the compact 32-byte arrays; the nullifiers, rng slices and amounts of the verified lanes   [gather_verified, k_admit_rows]
//   verify_windows   the verified lanes' records / messages gathered ADMIT_WINDOW_BATCHES * max_batch at a time
//   tail             once per call check-and-insert and signing over the compact arrays (redeem_tail_ring, keyring_redeem_impl.inc: one
//                    rng draw per call; replay: replay_tail, every tag and nonce takes the lane's t)
//   scatter          statuses, out_key and refunds back to their lanes; shed lanes get all-zero records           [k_admit_scatter]
//                    a copy is resolved [k_copy_resolve] or, in the replay forms, SERVED its leader's refund -- with amounts only if it
//                    names its leader's                                                             [k_copy_serve, k_copy_serve_return]
//   counts           admit_counts (admit_counts.h), from host arrays
// The decision that RECORDS is still the check-and-insert behind verification; the look-up of the screen only spares work.
#include "admit_counts.h"
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

// One window of lanes gathered into the caller's kind of memory (the verified lanes' windows; the spent lanes of the replay form,
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

// the lanes that are verified, in lane order: m lane numbers idx[], every lane's place among them pos[] (ADMIT_SHED: none) and the
// pre-statuses they were compacted from -- all in device memory
struct AdmitVerified { const uint8_t* pre; const uint32_t *idx, *pos; size_t m; };

// the copy stage of the unique forms (copies_impl.inc): what it leaves for the rest of the call.  copies == 0: v is what pass() was given
struct AdmitCopies {
  act_ctx* c; DevTmp d;
  AdmitVerified v{nullptr, nullptr, nullptr, 0};
  size_t copies = 0, m2 = 0;                                  // m2 = the lanes that are verified
  uint8_t* d_pre2 = nullptr; uint32_t *d_lead = nullptr, *d_idx2 = nullptr, *d_pos2 = nullptr;      // n entries each, in d
  explicit AdmitCopies(act_ctx* c_) : c(c_), d(c_) {}
  void pass(const AdmitVerified& survivors) { v = survivors; }      // no stage, or no copies: the screen's survivors are verified
  // over the survivors passed; span: their bytes in the caller's kind of memory (offsets in the same kind); h_idx: host-memory callers only
  int run(hipStream_t stream, bool dev, size_t n, const CopySpan& span, const uint32_t* h_idx, const uint32_t salt[4]);
};

// One call of the family, filled once by its entry point.  rng / rng_mode of a replay form are the derived nonces' stand-in (one byte,
// ACT_RNG_PER_LANE); out_counts is the FORM's array (admit_counts_len(form) values).
struct AdmitCall {
  act_ctx* c; act_nullifier_set* set; size_t n; int mem;
  const uint8_t* keys = nullptr; int nkeys = 0; const uint32_t* key_epochs = nullptr; int sign_key = 0;      // the ring
  const uint8_t* proof = nullptr; const uint8_t* cbor = nullptr; const uint64_t* offsets = nullptr;          // records, or messages
  const uint8_t* charge = nullptr; const uint8_t* returned = nullptr;      // expected charges; form.ret: the amounts t, n scalars (null: all zero)
  const uint8_t* rng = nullptr; int rng_mode = 0;
  uint8_t *out = nullptr, *status = nullptr, *out_key = nullptr; uint64_t* out_counts = nullptr;
  AdmitForm form{false, false, false};
  act_nullifier_set* receipts = nullptr; const uint8_t* nonce_key = nullptr; uint8_t* out_replayed = nullptr;      // form.replay
  RedeemReturn amounts{nullptr};

  AdmitCall(act_ctx* c_, act_nullifier_set* set_, size_t n_, int mem_) : c(c_), set(set_), n(n_), mem(mem_) {}
  AdmitCall& ring(const uint8_t* k, int nk, const uint32_t* epochs, int sign) { keys = k; nkeys = nk; key_epochs = epochs; sign_key = sign; return *this; }
  AdmitCall& records(const uint8_t* p) { proof = p; return *this; }
  AdmitCall& messages(const uint8_t* m, const uint64_t* offs) {      // (an empty wire call may pass no bytes at all; a null pointer with lanes is refused)
    static const uint8_t none = 0;
    cbor = (m || n) ? m : &none; offsets = offs; return *this;
  }
  AdmitCall& charged(const uint8_t* s) { charge = s; return *this; }
  AdmitCall& returns(const uint8_t* t) { form.ret = true; returned = t; amounts.t = t; return *this; }
  AdmitCall& draws(const uint8_t* r, int mode) { rng = r; rng_mode = mode; return *this; }
  AdmitCall& replays(act_nullifier_set* rs, const uint8_t* key, uint8_t* marks) {
    static const uint8_t derived = 0;      // the nonces stand where the admission calls' rng stands
    form.replay = true; receipts = rs; nonce_key = key; out_replayed = marks; return draws(&derived, ACT_RNG_PER_LANE);
  }
  // act_redeem_(cbor_)reserve_batch (DESIGN 4.11): the replay form without its signature half -- no sign_key, no nonce_key, 96-byte records out
  bool reserve = false;
  AdmitCall& reserves(act_nullifier_set* rs, uint8_t* marks) {
    static const uint8_t unsigned_key[32] = {0};      // where replay_refused wants a nonce_key: never staged, never hashed
    reserve = true; return replays(rs, unsigned_key, marks);
  }
  AdmitCall& uniquely() { form.unique = true; return *this; }
  // request binding (DESIGN 4.12): n * 32 bytes in `mem` memory that enter every verified lane's challenge hash.  Only the verification
  // step sees them: the screen, the candidate stage, the tags, the nonces and both sets do not.  Null: the unbound call
  const uint8_t* bind = nullptr;
  AdmitCall& bound(const uint8_t* b) { bind = b; return *this; }
  AdmitCall& answers(uint8_t* o, uint8_t* st, uint8_t* key, uint64_t* counts) { out = o; status = st; out_key = key; out_counts = counts; return *this; }

  bool wire() const { return cbor != nullptr; }
  bool dev() const { return mem == ACT_MEM_DEVICE; }
  bool replay() const { return form.replay; }
  const RedeemReturn* ret() const { return form.ret ? &amounts : nullptr; }      // as the tails and the ring redeem take it
  const uint8_t* input() const { return wire() ? cbor : proof; }
};

// the replay stage's view of the call (admit_replay_impl.inc): the screen's arrays and, as scratch until the survivors' compaction
// overwrites them, the compaction's
struct AdmitReplayStage {
  hipStream_t stream; size_t n; bool dev, wire, dev_reader; const uint8_t* proof; const uint8_t* cbor; const WireExtent* ext; bool offsets;
  uint8_t* d_pre; const uint8_t* d_kred; uint32_t *d_blk, *d_idx, *d_pos, *d_total;
  const uint8_t* d_t;                 // the return form: the n returned amounts in device memory, as the screen read them (null: every t = 0)
  bool reserve;                       // the reserve form: d_t holds the n reduced charges s^ and the tag is tag_res (reserve_lanes.h)
};

}  // namespace

// the reserve form of the replay tail (reserve_impl.inc): the charges lane for lane with the tail's arrays, in the call's kind of memory
struct ReplayReserve { const uint8_t* s; };
static void reserve_tags_host(const ReplayDeriveArgs& a);
static int reserve_emit(act_ctx* c, hipStream_t stream, size_t n, int mem, const uint8_t* k_at, size_t k_stride, const uint8_t* kp, const uint8_t* s, const uint8_t* st,
                        uint8_t* out, uint8_t* status);

// candidates: the spent lanes whose tag the receipts hold -- verified like fresh lanes
static int admit_replay_stage(act_ctx* c, act_nullifier_set* receipts, const AdmitReplayStage& g, size_t* candidates);
static int replay_refused(act_ctx* c, act_nullifier_set* set, act_nullifier_set* receipts, const uint8_t* nonce_key, size_t n, const uint32_t* key_epochs, int nkeys);
static int replay_tail(act_ctx* c, act_nullifier_set* set, act_nullifier_set* receipts, size_t n, int mem, const uint8_t* keys, int nkeys, const uint32_t* key_epochs,
                       int sign_key, bool wire, const uint8_t* k_at, size_t k_stride, const uint8_t* kp, uint8_t* st, const uint8_t* nonce_key, uint8_t* out,
                       uint8_t* status, uint8_t* out_key, uint8_t* out_replayed, uint64_t* out_counts, bool* began = nullptr, const RedeemReturn* ret = nullptr,
                       const ReplayReserve* res = nullptr);
static int redeem_replay_locked(act_ctx* c, act_nullifier_set* set, act_nullifier_set* receipts, size_t n, int mem, const uint8_t* keys, int nkeys,
                                const uint32_t* key_epochs, int sign_key, const uint8_t* proof, const uint8_t* cbor, const uint64_t* offsets, const uint8_t* nonce_key,
                                uint8_t* out, uint8_t* status, uint8_t* out_key, uint8_t* out_replayed, uint64_t* out_counts, const RedeemReturn* ret = nullptr,
                                const ReplayReserve* res = nullptr, const uint8_t* bind = nullptr);

namespace {

// What one call owns between its stages: the shape of its input, the stage's device scratch (one slab, public data: lane numbers,
// codes, nullifiers, charges) with its host mirrors, and the compact arrays of the verified lanes.  Built under the call's locks;
// the wiped rng buffers go with it on every exit.
struct AdmitState {
  const AdmitCall& a; act_ctx* const c; const size_t n; const bool wire, dev, rp; const RedeemReturn* const ret; const hipStream_t stream;
  const size_t pb, out_b; const CborType* const T; CborLayout lay; size_t ml, nf; const WireExtent ext; const bool dev_reader;
  // the slab: the screen's and the compaction's arrays, and where the wire branch keeps its own
  DevTmp d; size_t fcap = 0, o_charge = 0, o_ret = 0, o_code = 0, o_flags = 0, o_off = 0, o_tmpl = 0, o_pay = 0, o_pwhich = 0, o_patch = 0, o_rcode = 0;
  uint8_t *d_pre = nullptr, *d_kred = nullptr, *d_ks = nullptr; uint32_t *d_idx = nullptr, *d_pos = nullptr, *d_blk = nullptr, *d_total = nullptr;
  AdmitScreenArgs sa{};
  std::vector<uint8_t> h_pre;              // every lane's final pre-status
  size_t m = 0, candidates = 0;            // the screen's survivors; replay: the retry candidates among them
  AdmitCopies cp;                          // cp.v: the lanes that are verified (mv of them)
  std::vector<uint32_t> h_sidx, h_lead;    // host-memory callers of the unique forms: the survivors' lane numbers; with copies, every lane's leader
  std::vector<uint32_t> h_vidx, h_pos;     // the verified lanes' numbers; host-memory callers: every lane's place among them
  // the compact arrays in the caller's kind of memory: K' | nullifiers | verdicts | look-up answers | key indices | matched keys | statuses (| replay marks) (| amounts)
  AdmitArr arr, cout;
  uint8_t *kp = nullptr, *knul = nullptr, *st = nullptr, *sp = nullptr, *kidx = nullptr, *okey = nullptr, *cst = nullptr, *crepl = nullptr;
  AdmitRngDev rng_dev; std::vector<uint8_t> rng_host; AdmitHostWipe rng_wipe{rng_host};      // the verified lanes' rng slices (secret): wiped on every exit
  const uint8_t* c_rng; RedeemReturn cret{nullptr};
  const uint8_t* c_bind = nullptr;      // a bound call: the verified lanes' request bindings, behind the other compact arrays
  uint8_t* d_sred = nullptr; std::vector<uint8_t> h_sred; ReplayReserve cres{nullptr};      // the reserve form: every lane's s^ (device; host copy), the verified lanes'
  uint64_t tc[ACT_REPLAY_COUNTS] = {0, 0, 0, 0, 0, 0};      // replay: the tail's counts
  std::vector<uint8_t> h_cst, h_fin, h_t;  // device-memory callers, for the counts: compact statuses; the replay unique forms' final statuses and amounts

  explicit AdmitState(const AdmitCall& a_)
      : a(a_), c(a_.c), n(a_.n), wire(a_.wire()), dev(a_.dev()), rp(a_.replay()), ret(a_.ret()), stream(a_.set->stream), pb(act_spend_proof_bytes(a_.c)),
        out_b(a_.reserve ? (size_t)RESERVATION_BYTES : redeem_out_bytes(a_.c, a_.wire(), a_.ret())), T(cbor_type(ACT_CBOR_SPEND_PROOF)), lay(a_.wire() ? cbor_layout(*T, a_.c->L) : CborLayout()),
        ml(lay.tmpl.size()), nf(lay.pay_off.size()), ext{a_.cbor, a_.offsets, ml}, dev_reader(a_.wire() && a_.c->wire_reader.load() == ACT_WIRE_READER_DEVICE),
        d(a_.c), cp(a_.c), arr(a_.c), cout(a_.c), rng_dev(a_.c), c_rng(a_.rng) {}

  size_t mv() const { return cp.v.m; }
  const uint64_t* d_offsets() const { return reinterpret_cast<const uint64_t*>(d.p + o_off); }      // wire with offsets, device-memory callers

  int reserve() {
    const size_t nb = (n + ADMIT_BLOCK - 1) / ADMIT_BLOCK;
    fcap = (n + 3) & ~(size_t)3;
    size_t need = 0;
    auto take = [&](size_t bytes) { const size_t at = need; need += (bytes + 15) & ~(size_t)15; return at; };
    const size_t o_pre = take(n), o_kred = take(n * 32), o_idx = take(n * 4), o_pos = take(n * 4), o_blk = take(nb * 4), o_total = take(4);
    const size_t o_ks = (wire || !dev) ? take(n * 64) : 0;
    o_charge = (a.charge && !dev) ? take(n * 32) : 0; o_ret = (a.returned && !dev) ? take(n * 32) : 0;
    o_code = wire ? take(n) : 0; o_flags = (wire && dev) ? take(fcap) : 0; o_off = (wire && dev && a.offsets) ? take((n + 1) * 8) : 0;
    o_tmpl = (wire && dev) ? take(ml) : 0; o_pay = (wire && dev) ? take(nf * 4) : 0;
    o_pwhich = wire ? take(WIRE_SETTLE_WINDOW * 4) : 0; o_patch = wire ? take(WIRE_SETTLE_WINDOW * 64) : 0;
    o_rcode = (dev_reader && dev) ? take(2 * n) : 0;      // the device reader's codes, then its infos
    const size_t o_sred = a.reserve ? take(n * 32) : 0;
    if (int rc = d.alloc(need)) return rc;
    ADCK(c, hipSetDevice(c->device));
    d_pre = d.p + o_pre; d_kred = d.p + o_kred; d_ks = d.p + o_ks; d_sred = a.reserve ? d.p + o_sred : nullptr;
    d_idx = reinterpret_cast<uint32_t*>(d.p + o_idx); d_pos = reinterpret_cast<uint32_t*>(d.p + o_pos);
    d_blk = reinterpret_cast<uint32_t*>(d.p + o_blk); d_total = reinterpret_cast<uint32_t*>(d.p + o_total);
    return ACT_OK;
  }

  // ---- where k and s are ------------------------------------------------------------------------------------------------------------------
  int locate_ks() {
    sa.n = (uint32_t)n; sa.pre = d_pre; sa.kred = d_kred;
    if (wire) {
      if (int rc = wire_ks()) return rc;
      sa.ks = d_ks; sa.stride = 64; sa.wire_code = d.p + o_code;
    } else if (dev) { sa.ks = a.proof; sa.stride = (uint32_t)pb; }
    else { ADCK(c, hipMemcpy2DAsync(d_ks, 64, a.proof, pb, 64, n, hipMemcpyHostToDevice, stream)); sa.ks = d_ks; sa.stride = 64; }      // the 64-byte fields only
    if (a.charge) {
      if (dev) sa.charge = a.charge;
      else { ADCK(c, hipMemcpyAsync(d.p + o_charge, a.charge, n * 32, hipMemcpyHostToDevice, stream)); sa.charge = d.p + o_charge; }
    }
    if (a.returned) {      // t <= s is the screen's rule, in the pass that compares the charge
      if (dev) sa.returned = a.returned;
      else { ADCK(c, hipMemcpyAsync(d.p + o_ret, a.returned, n * 32, hipMemcpyHostToDevice, stream)); sa.returned = d.p + o_ret; }
    }
    return ACT_OK;
  }

  // device memory: the framing compare as a kernel, then the device reader over what it flags -> d_ks, the codes, flags on the host
  int wire_frames_dev(std::vector<uint8_t>& flags) {
    uint8_t* d_flags = d.p + o_flags;
    ADCK(c, hipMemsetAsync(d_flags, 0, fcap, stream));
    ADCK(c, hipMemcpyAsync(d.p + o_tmpl, lay.tmpl.data(), ml, hipMemcpyHostToDevice, stream));
    ADCK(c, hipMemcpyAsync(d.p + o_pay, lay.pay_off.data(), nf * 4, hipMemcpyHostToDevice, stream));
    if (a.offsets) ADCK(c, hipMemcpyAsync(d.p + o_off, a.offsets, (n + 1) * 8, hipMemcpyHostToDevice, stream));
    for (size_t off = 0; off < n; off += ADMIT_WIRE_LAUNCH) {      // (off is a multiple of 4: the flag words of two launches do not overlap)
      AdmitWireArgs w{};
      w.n = (uint32_t)std::min(ADMIT_WIRE_LAUNCH, n - off); w.n_fields = (uint32_t)nf; w.msg_len = (uint32_t)ml;
      w.cbor = a.offsets ? a.cbor : a.cbor + off * ml; w.offsets = a.offsets ? d_offsets() + off : nullptr;
      w.tmpl = d.p + o_tmpl; w.pay_off = reinterpret_cast<const uint32_t*>(d.p + o_pay); w.ks = d_ks + off * 64; w.flags = d_flags + off;
      launch_admit_wire(w, stream);
    }
    if (dev_reader) {      // every other spelling: the reader's reduced form over the flagged messages, k and s into d_ks, the codes for the screen
      ADCK(c, hipMemsetAsync(d.p + o_rcode, 0, 2 * n, stream));
      CborReadArgs ra{};
      ra.T = *T; ra.L = c->L; ra.n = (uint32_t)n; ra.first = 0; ra.msg_len = (uint32_t)ml; ra.in = a.cbor; ra.offsets = a.offsets ? d_offsets() : nullptr;
      ra.flags = d_flags; ra.rec = d_ks; ra.rec_stride = 64; ra.keep_fields = 2; ra.code = d.p + o_rcode; ra.info = d.p + o_rcode + n;
      launch_cbor_read(ra, false, stream);
      launch_cbor_read(ra, true, stream);
      CborCodeArgs ca{(uint32_t)n, ra.code, ra.info, d.p + o_code};
      launch_cbor_wire_code(ca, stream);
    }
    ADCK(c, hipGetLastError());
    ADCK(c, hipMemcpyAsync(flags.data(), d_flags, fcap, hipMemcpyDeviceToHost, stream));
    ADCK(c, hipStreamSynchronize(stream));
    return ACT_OK;
  }
  // host memory: the same lane bodies on the host workers, 64 bytes per message cross the link
  int wire_frames_host(std::vector<uint8_t>& flags, std::vector<uint8_t>& h_code) {
    std::vector<uint8_t> h_ks(n * 64, 0);
    AdmitWireJob job{};
    job.a.n = (uint32_t)n; job.a.n_fields = (uint32_t)nf; job.a.msg_len = (uint32_t)ml; job.a.cbor = a.cbor; job.a.offsets = a.offsets;
    job.a.tmpl = lay.tmpl.data(); job.a.pay_off = lay.pay_off.data(); job.a.ks = h_ks.data(); job.a.flags = flags.data();
    act_host_parallel_for(n, 256, 0, [](void* p, size_t i0, size_t i1) {
      const AdmitWireArgs& w = static_cast<AdmitWireJob*>(p)->a;
      for (size_t m = i0; m < i1; m++) {
        bool canon = true;
        for (uint32_t f = 0; f < w.n_fields && canon; f++) canon = admit_wire_piece(w, (uint32_t)m, f);
        w.flags[m] = canon ? 0 : 0x80;
      }
    }, &job);
    if (dev_reader) {      // the reader's lane body on the host workers, both passes of a message one behind the other
      std::vector<uint8_t> rinfo(n, 0);
      AdmitReadJob rj{};
      rj.a.T = *T; rj.a.L = c->L; rj.a.n = (uint32_t)n; rj.a.first = 0; rj.a.msg_len = (uint32_t)ml; rj.a.in = a.cbor; rj.a.offsets = a.offsets;
      rj.a.flags = flags.data(); rj.a.rec = h_ks.data(); rj.a.rec_stride = 64; rj.a.keep_fields = 2; rj.a.code = h_code.data(); rj.a.info = rinfo.data();
      act_host_parallel_for(n, 64, 0, [](void* p, size_t i0, size_t i1) {
        const CborReadArgs& r = static_cast<AdmitReadJob*>(p)->a;
        uint32_t stack[CBOR_MAX_DEPTH];
        for (size_t m = i0; m < i1; m++) {
          cbor_read_message_lane<false>(r, (uint32_t)m, stack);
          cbor_read_message_lane<true>(r, (uint32_t)m, stack);
          r.code[m] = cbor_code_status(r.code[m]);      // (an unflagged message keeps its 0)
        }
      }, &rj);
    }
    ADCK(c, hipMemcpyAsync(d_ks, h_ks.data(), n * 64, hipMemcpyHostToDevice, stream));
    ADCK(c, hipStreamSynchronize(stream));
    return ACT_OK;
  }
  // wire: k and s of every message into d_ks, every message's code into the slab
  int wire_ks() {
    std::vector<uint8_t> flags(fcap, 0), h_code(n, 0);
    if (int rc = dev ? wire_frames_dev(flags) : wire_frames_host(flags, h_code)) return rc;
    // every other spelling: the general reader, a window at a time (wire_window_read).  A message that reads yields the record, and so
    // k and s; one that does not takes the status act_redeem_cbor_* gives it (the first error in wire order: cbor_settle_codes)
    std::vector<size_t> which;
    for (size_t i = 0; i < n; i++) if (flags[i] & 0x80) which.push_back(i);
    c->wire_stats[0] += n; c->wire_stats[1] += n - which.size(); c->wire_stats[dev_reader ? 2 : 3] += which.size();
    if (dev_reader) which.clear();      // read already: the serial window loop below is the road of ACT_WIRE_READER_HOST
    WireWindow win; std::vector<uint8_t> patch; std::vector<uint32_t> pwhich;
    for (size_t w0 = 0; w0 < which.size(); w0 += WIRE_SETTLE_WINDOW) {
      const size_t cnt = std::min(which.size(), w0 + WIRE_SETTLE_WINDOW) - w0;
      const size_t* lanes = which.data() + w0;
      if (int rc = wire_window_read(c, stream, *T, ext, dev, lanes, cnt, pb, win)) return rc;
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
    return ACT_OK;
  }

  // ---- the screen (the set's lock is held while its table is read), the replay stage, the compaction --------------------------------------------
  int screen() {
    uint32_t m32 = 0;
    h_pre.resize(n);
    std::unique_lock<std::mutex> lk(a.set->mu);
    sa.tab_keys = a.set->tab_keys; sa.tab_state = a.set->tab_state; sa.tab_cap = a.set->tab_cap; memcpy(sa.salt.w, a.set->salt, 16);
    launch_admit_screen(sa, stream);
    if (a.reserve) { ReserveSredArgs ra{(uint32_t)n, sa.stride, sa.ks, d_sred}; launch_reserve_sred(ra, stream); }      // s^ beside k^, for the tags and the records
    if (rp) {      // the spent lanes: retry candidates go on, the others stay double spends; the compaction is over what that leaves
      ADCK(c, hipGetLastError());
      ADCK(c, hipStreamSynchronize(stream));
      lk.unlock();
      const AdmitReplayStage g{stream, n, dev, wire, dev_reader, a.proof, a.cbor, &ext, a.offsets != nullptr, d_pre, d_kred, d_blk, d_idx, d_pos, d_total, a.reserve ? d_sred : sa.returned, a.reserve};
      if (int rc = admit_replay_stage(c, a.receipts, g, &candidates)) return rc;
    }
    launch_admit_compact(d_pre, (uint32_t)n, d_blk, d_idx, d_pos, d_total, stream);
    ADCK(c, hipGetLastError());
    ADCK(c, hipMemcpyAsync(&m32, d_total, 4, hipMemcpyDeviceToHost, stream));
    ADCK(c, hipMemcpyAsync(h_pre.data(), d_pre, n, hipMemcpyDeviceToHost, stream));
    ADCK(c, hipStreamSynchronize(stream));
    m = m32;
    if (m > n) { c->err = "admission: the compaction counted more survivors than lanes"; return ACT_ERR_HIP; }
    return ACT_OK;
  }

  // ---- the unique forms: a survivor with the bytes of an earlier survivor is a copy and is not verified ------------------------------------------
  int copy_stage() {
    cp.pass({d_pre, d_idx, d_pos, m});
    if (!a.form.unique || m < 2) return ACT_OK;
    if (!dev) { h_sidx.resize(m); ADCK(c, hipMemcpy(h_sidx.data(), d_idx, m * 4, hipMemcpyDeviceToHost)); }
    CopySpan span{a.input(), nullptr, wire ? ml : pb};
    if (wire && a.offsets) span.offsets = dev ? d_offsets() : a.offsets;
    uint32_t salt[4];
    { std::lock_guard<std::mutex> lk(a.set->mu); memcpy(salt, a.set->salt, 16); }
    if (int rc = cp.run(stream, dev, n, span, h_sidx.data(), salt)) return rc;
    if (cp.copies && !dev) { h_lead.resize(n); ADCK(c, hipMemcpy(h_lead.data(), cp.d_lead, n * 4, hipMemcpyDeviceToHost)); }
    return ACT_OK;
  }

  // ---- nothing shed: the honest batch pays the screen and nothing else; replay: the replay call itself ---------------------------------------------
  int nothing_shed() {
    if (rp) {
      if (a.reserve) {      // every lane's s^ in the caller's kind of memory, lane for lane
        cres.s = d_sred;
        if (!dev) { h_sred.resize(n * 32); ADCK(c, hipMemcpy(h_sred.data(), d_sred, n * 32, hipMemcpyDeviceToHost)); cres.s = h_sred.data(); }
      }
      const int rc = redeem_replay_locked(c, a.set, a.receipts, n, a.mem, a.keys, a.nkeys, a.key_epochs, a.sign_key, a.proof, a.cbor, a.offsets, a.nonce_key, a.out, a.status,
                                          a.out_key, a.out_replayed, a.out_counts ? tc : nullptr, ret, a.reserve ? &cres : nullptr, a.bind);      // (the caller's `returned` and bindings, lane for lane)
      counts(nullptr, tc);      // (tc[0] == 0: the call ended before its tail, and the counts stay zero)
      return rc;
    }
    const int rc = redeem_keyring_impl(c, a.set, n, a.mem, a.keys, a.nkeys, a.key_epochs, a.sign_key, a.proof, a.cbor, a.offsets, a.rng, a.rng_mode, a.out, a.status, a.out_key, ret);
    if (a.out_counts && (rc == ACT_OK || rc == ACT_ERR_ARG)) {      // (ACT_ERR_ARG: the nullifier step refused lanes; status[] is complete)
      const uint8_t* s = a.status;
      if (dev) { h_cst.resize(n); if (hipMemcpy(h_cst.data(), a.status, n, hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return rc; } s = h_cst.data(); }
      counts(s, nullptr);
    }
    return rc;
  }
  // ---- everything shed: no verification, nothing recorded, no rng drawn; replay: no mark either -----------------------------------------------------
  int everything_shed() {
    if (int rc = redeem_keyring_impl(c, a.set, 0, a.mem, a.keys, a.nkeys, a.key_epochs, a.sign_key, nullptr, nullptr, nullptr, a.rng, a.rng_mode, nullptr, nullptr, nullptr)) return rc;      // a bad ring fails the call whatever is shed
    if (dev) {
      ADCK(c, hipMemcpyAsync(a.status, d_pre, n, hipMemcpyDeviceToDevice, stream));
      ADCK(c, hipMemsetAsync(a.out_key, ACT_KEY_NONE, n, stream));
      ADCK(c, hipMemsetAsync(a.out, 0, n * out_b, stream));
      if (a.out_replayed) ADCK(c, hipMemsetAsync(a.out_replayed, 0, n, stream));
      ADCK(c, hipStreamSynchronize(stream));
    } else { memcpy(a.status, h_pre.data(), n); memset(a.out_key, ACT_KEY_NONE, n); memset(a.out, 0, n * out_b); if (a.out_replayed) memset(a.out_replayed, 0, n); }
    counts(nullptr, nullptr);
    return ACT_OK;
  }

  // ---- the compact inputs of the verified lanes ------------------------------------------------------------------------------------------------------
  // mv() rows of `row` bytes gathered by the verified lanes' numbers into dst, which lies in the caller's kind of memory; src lies there
  // too, or (src_dev) in device memory whatever the caller's kind
  int gather_verified(uint8_t* dst, const uint8_t* src, bool src_dev, size_t row) {
    if (!src_dev) { for (size_t j = 0; j < mv(); j++) memcpy(dst + j * row, src + (size_t)h_vidx[j] * row, row); return ACT_OK; }
    DevTmp g(c); uint8_t* to = dst;
    if (!dev) { if (int rc = g.alloc(mv() * row)) return rc; to = g.p; }
    AdmitRowsArgs ra{to, src, cp.v.idx, (uint32_t)mv(), row};
    launch_admit_rows(ra, stream);
    ADCK(c, hipGetLastError());
    if (!dev) ADCK(c, hipMemcpyAsync(dst, g.p, mv() * row, hipMemcpyDeviceToHost, stream));
    ADCK(c, hipStreamSynchronize(stream));
    return ACT_OK;
  }
  int compact_inputs() {
    const size_t mv = this->mv();
    int rc;
    h_vidx.resize(mv);
    ADCK(c, hipMemcpy(h_vidx.data(), cp.v.idx, mv * 4, hipMemcpyDeviceToHost));
    if (!dev) { h_pos.resize(n); ADCK(c, hipMemcpy(h_pos.data(), cp.v.pos, n * 4, hipMemcpyDeviceToHost)); }
    const size_t arr_lane = rp ? 70 : 69;
    const size_t o_bind = ((mv * arr_lane + 31) & ~(size_t)31) + ((a.returned || a.reserve) ? mv * 32 : 0);      // (a 32-byte boundary: the amounts or charges in front are whole rows)
    if ((rc = arr.alloc(a.mem, mv * arr_lane + ((a.returned || a.reserve) ? mv * 32 + 32 : 0) + (a.bind ? mv * 32 + 32 : 0)))) { c->err = "admission: compact arrays"; return rc; }
    if ((rc = cout.alloc(a.mem, mv * out_b))) { c->err = "admission: compact output"; return rc; }
    kp = arr.p; knul = kp + mv * 32; st = knul + mv * 32; sp = st + mv; kidx = sp + mv; okey = kidx + mv; cst = okey + mv;
    crepl = cst + mv;      // (the replay form: the verified lanes' replay marks)
    // a status that the tail leaves unwritten (it returns early only on a device failure BEHIND check-and-insert) must never read as
    // accepted: recorded, not signed
    if (dev) { ADCK(c, hipMemset(cst, ACT_STATUS_RECORDED_UNSIGNED, mv)); ADCK(c, hipDeviceSynchronize()); } else memset(cst, ACT_STATUS_RECORDED_UNSIGNED, mv);
    if ((rc = gather_verified(knul, d_kred, true, 32))) return rc;      // the reduced nullifiers, as the screen left them
    // the per-lane rng slices follow their lanes (secret: staged in the context's own buffer or a host vector, wiped on every exit)
    if (a.rng_mode == ACT_RNG_PER_LANE && !rp) {
      if (dev) { if ((rc = rng_dev.reserve(mv * 128))) return rc; c_rng = c->d_admit_rng; }
      else { rng_host.resize(mv * 128); c_rng = rng_host.data(); }
      if ((rc = gather_verified(const_cast<uint8_t*>(c_rng), a.rng, dev, 128))) return rc;
    }
    // the returned amounts follow their lanes too (public; the compact copy lies behind the other compact arrays, 32-byte aligned): in
    // the unique forms the amounts of the lanes that are verified -- a copy's t is never read here
    if (a.returned) {
      uint8_t* ct = arr.p + ((mv * arr_lane + 31) & ~(size_t)31);
      if ((rc = gather_verified(ct, a.returned, dev, 32))) return rc;
      cret.t = ct;
    }
    if (a.reserve) {      // the reserve form: the verified lanes' s^ in the same place (it takes no amounts)
      uint8_t* cs = arr.p + ((mv * arr_lane + 31) & ~(size_t)31);
      if ((rc = gather_verified(cs, d_sred, true, 32))) return rc;
      cres.s = cs;
    }
    // the request bindings follow their lanes too, by the same row gather: survivor j is verified under the binding of lane v_idx[j]
    if (a.bind) {
      uint8_t* cb = arr.p + o_bind;
      if ((rc = gather_verified(cb, a.bind, dev, 32))) return rc;
      c_bind = cb;
    }
    return ACT_OK;
  }

  // ---- verification, a window at a time ------------------------------------------------------------------------------------------------------------------
  int verify_windows() {
    const size_t W = std::max<size_t>(1, ADMIT_WINDOW_BATCHES * c->max_batch);
    AdmitGather gather(c, stream, dev, a.input(), wire ? ml : pb, (wire && a.offsets) ? &ext : nullptr);
    for (size_t w0 = 0; w0 < mv(); w0 += W) {
      const size_t w = std::min(W, mv() - w0);
      int rc = gather.run(cp.v.idx + w0, h_vidx.data() + w0, w);
      if (rc) return rc;
      const uint8_t* g = gather.data();
      const uint8_t* wb = c_bind ? c_bind + w0 * 32 : nullptr;
      if (wire) { RingSel sel{a.keys, a.nkeys, okey + w0, wb}; rc = verify_spend_cbor_impl(c, w, a.mem, nullptr, g, gather.offsets(), st + w0, kp + w0 * 32, nullptr, &sel); }
      else rc = act_verify_spend_keyring_bound_batch(c, w, a.mem, a.keys, a.nkeys, g, wb, st + w0, okey + w0, kp + w0 * 32);
      if (rc) return rc;            // as in the redeem calls: nothing recorded, status untouched
    }
    return ACT_OK;
  }

  // ---- once per call, over the compact arrays.  *answer: the lanes are owed their answers whatever the tail returns ---------------------------------------
  int tail(bool* answer) {
    const RedeemReturn* const t = ret ? &cret : nullptr;
    if (!rp) {
      *answer = true;
      return redeem_tail_ring(c, a.set, mv(), a.mem, a.keys, a.nkeys, a.key_epochs, a.sign_key, wire, knul, 32, kp, st, sp, kidx, c_rng, a.rng_mode, cout.p, cst, okey, t);
    }
    bool began = false;
    const int rc = replay_tail(c, a.set, a.receipts, mv(), a.mem, a.keys, a.nkeys, a.key_epochs, a.sign_key, wire, knul, 32, kp, st, a.nonce_key, cout.p, cst, okey, crepl, tc, &began, t, a.reserve ? &cres : nullptr);
    *answer = !rc || began;      // staging its buffers failed: as a failed verification -- nothing recorded, status untouched
    return rc;
  }

  // ---- the answers back to their lanes (also behind a failure of the tail: status[] is complete on return) ----------------------------------------------
  // a copy: resolved from its leader's final status, or (replay) served its leader's whole answer -- with amounts only if it names its
  // leader's: a copy's t is read here and nowhere else
  int scatter() {
    const bool serve = cp.copies && rp, resolve = cp.copies && !rp;
    if (dev) {
      AdmitScatterArgs sc{}; sc.n = (uint32_t)n; sc.out_bytes = out_b; sc.pos = cp.v.pos; sc.pre = cp.v.pre; sc.c_status = cst; sc.c_key = okey; sc.c_out = cout.p;
      sc.status = a.status; sc.out_key = a.out_key; sc.out = a.out;
      launch_admit_scatter(sc, stream);
      if (resolve) { CopyResolveArgs ra{cp.d_lead, (uint32_t)n, a.status, a.out_key}; launch_copy_resolve(ra, stream); }      // COPY_MARK leaves status[] here
      if (rp && a.out_replayed) {      // the replay marks ride the same scatter as one-byte records (a shed lane: 0)
        AdmitScatterArgs sr = sc; sr.out_bytes = 1; sr.c_out = crepl; sr.out = a.out_replayed;
        launch_admit_scatter(sr, stream);
      }
      if (serve) {      // behind both scatters the rows of leaders are final
        const CopyServeArgs va{cp.d_lead, (uint32_t)n, out_b, a.status, a.out_key, a.out, a.out_replayed};
        if (ret) { CopyServeReturnArgs vr{va, a.returned}; launch_copy_serve_return(vr, stream); } else launch_copy_serve(va, stream);
      }
      ADCK(c, hipGetLastError());
      if (a.out_counts && !rp) { h_cst.resize(mv()); ADCK(c, hipMemcpyAsync(h_cst.data(), cst, mv(), hipMemcpyDeviceToHost, stream)); }
      if (serve && a.out_counts) {      // copies_served is counted on the final statuses
        h_lead.resize(n); h_fin.resize(n);
        ADCK(c, hipMemcpyAsync(h_lead.data(), cp.d_lead, n * 4, hipMemcpyDeviceToHost, stream));
        ADCK(c, hipMemcpyAsync(h_fin.data(), a.status, n, hipMemcpyDeviceToHost, stream));
        if (a.returned) { h_t.resize(n * 32); ADCK(c, hipMemcpyAsync(h_t.data(), a.returned, n * 32, hipMemcpyDeviceToHost, stream)); }
      }
      ADCK(c, hipStreamSynchronize(stream));
    } else {
      for (size_t i = 0; i < n; i++) {
        const uint32_t j = h_pos[i];
        if (j == ADMIT_SHED) { a.status[i] = h_pre[i]; a.out_key[i] = ACT_KEY_NONE; memset(a.out + i * out_b, 0, out_b); }
        else { a.status[i] = cst[j]; a.out_key[i] = okey[j]; memcpy(a.out + i * out_b, cout.p + (size_t)j * out_b, out_b); }
        if (rp && a.out_replayed) a.out_replayed[i] = j == ADMIT_SHED ? 0 : crepl[j];
      }
      if (resolve) { CopyResolveArgs ra{h_lead.data(), (uint32_t)n, a.status, a.out_key}; for (size_t i = 0; i < n; i++) copy_resolve_lane(ra, (uint32_t)i); }
      const CopyServeArgs va{h_lead.data(), (uint32_t)n, out_b, a.status, a.out_key, a.out, a.out_replayed};
      if (serve && ret) { CopyServeReturnArgs vr{va, a.returned}; for (size_t i = 0; i < n; i++) copy_serve_return_lane(vr, (uint32_t)i); }
      else if (serve) for (size_t i = 0; i < n; i++) copy_serve_lane(va, (uint32_t)i);
    }
    return ACT_OK;
  }

  // ---- the counts.  cst: the verified lanes' statuses on the host (the forms without replay); tail: the replay tail's counts (null: no lane verified)
  void counts(const uint8_t* cst_host, const uint64_t* tail_counts) {
    if (!a.out_counts) return;
    const AdmitCountsIn in{n, h_pre.data(), mv(), cst_host, candidates, tail_counts, cp.copies, h_lead.data(), dev ? h_fin.data() : a.status,
                           !a.returned ? nullptr : dev ? h_t.data() : a.returned};
    admit_counts(a.form, in, a.out_counts);
  }
};

// everything the call refuses as a whole, before anything is looked at -- host checks only; a ring whose w does not decode fails the
// verification step (or, for a batch that is shed completely, the empty ring call) before anything is written
int admit_refused(const AdmitCall& a) {
  if (!a.c || (a.mem != ACT_MEM_HOST && a.mem != ACT_MEM_DEVICE) || a.n > ((size_t)1 << 30)) return ACT_ERR_ARG;
  if (a.n && ((!a.proof && !a.cbor) || !a.out || !a.status || !a.out_key)) return ACT_ERR_ARG;
  if (a.wire() && a.offsets) for (size_t i = 0; i < a.n; i++) if (a.offsets[i + 1] < a.offsets[i]) return ACT_ERR_ARG;
  if (a.bind && a.form.unique) { a.c->err = "admission: a bound call has no unique form"; return ACT_ERR_ARG; }      // (equality of proof bytes says nothing about two lanes' bindings)
  // what the redeem call refuses (null handles, ring size, sign_key, rng convention, device, epochs), in the same words
  if (int rc = redeem_keyring_refused(a.c, a.set, 0, a.keys, a.nkeys, a.key_epochs, a.sign_key, nullptr, nullptr, a.rng, a.rng_mode, nullptr, nullptr, nullptr)) return rc;
  return a.replay() ? replay_refused(a.c, a.set, a.receipts, a.nonce_key, a.n, a.key_epochs, a.nkeys) : ACT_OK;
}

int redeem_admit(const AdmitCall& a) {
  if (a.out_counts) memset(a.out_counts, 0, sizeof(uint64_t) * admit_counts_len(a.form));
  int rc = admit_refused(a);
  if (rc) return rc;
  if (a.n == 0) return redeem_keyring_impl(a.c, a.set, 0, a.mem, a.keys, a.nkeys, a.key_epochs, a.sign_key, nullptr, nullptr, nullptr, a.rng, a.rng_mode, nullptr, nullptr, nullptr);
  // one admission call at a time per context: the gathered rng slices live in the context's own buffer (d_admit_rng)
  std::lock_guard<std::mutex> admission(a.c->admit_mu);
  std::unique_lock<std::mutex> replay;      // the replay form: the staged secrets and the derived nonces of its tail (d_replay)
  if (a.replay()) replay = std::unique_lock<std::mutex>(a.c->replay_mu);
  AdmitState s(a);
  if ((rc = s.reserve()) || (rc = s.locate_ks()) || (rc = s.screen()) || (rc = s.copy_stage())) return rc;
  if (s.mv() == a.n) return s.nothing_shed();
  if (s.mv() == 0) return s.everything_shed();
  if ((rc = s.compact_inputs()) || (rc = s.verify_windows())) return rc;
  bool answer = false;
  const int rc_tail = s.tail(&answer);
  if (!answer) return rc_tail;
  if ((rc = s.scatter())) return rc;
  s.counts(s.dev ? s.h_cst.data() : s.cst, s.rp ? s.tc : nullptr);
  return rc_tail;
}

}  // namespace

extern "C" int act_redeem_admit_batch(act_ctx* c, act_nullifier_set* set, size_t n, int mem, const uint8_t* keys, int nkeys, const uint32_t* key_epochs, int sign_key,
                                      const uint8_t* proof, const uint8_t* charge, const uint8_t* rng, int rng_mode, uint8_t* out_refund, uint8_t* status,
                                      uint8_t* out_key, uint64_t* out_counts) {
  if (n && !proof) return ACT_ERR_ARG;
  return redeem_admit(AdmitCall(c, set, n, mem).ring(keys, nkeys, key_epochs, sign_key).records(proof).charged(charge).draws(rng, rng_mode)
                          .answers(out_refund, status, out_key, out_counts));
}
extern "C" int act_redeem_cbor_admit_batch(act_ctx* c, act_nullifier_set* set, size_t n, int mem, const uint8_t* keys, int nkeys, const uint32_t* key_epochs, int sign_key,
                                           const uint8_t* cbor, const uint64_t* offsets, const uint8_t* charge, const uint8_t* rng, int rng_mode,
                                           uint8_t* out_refund_cbor, uint8_t* status, uint8_t* out_key, uint64_t* out_counts) {
  if (n && !cbor) return ACT_ERR_ARG;
  return redeem_admit(AdmitCall(c, set, n, mem).ring(keys, nkeys, key_epochs, sign_key).messages(cbor, offsets).charged(charge).draws(rng, rng_mode)
                          .answers(out_refund_cbor, status, out_key, out_counts));
}
extern "C" int act_redeem_admit_unique_batch(act_ctx* c, act_nullifier_set* set, size_t n, int mem, const uint8_t* keys, int nkeys, const uint32_t* key_epochs,
                                             int sign_key, const uint8_t* proof, const uint8_t* charge, const uint8_t* rng, int rng_mode, uint8_t* out_refund,
                                             uint8_t* status, uint8_t* out_key, uint64_t* out_counts) {
  if (n && !proof) return ACT_ERR_ARG;
  return redeem_admit(AdmitCall(c, set, n, mem).ring(keys, nkeys, key_epochs, sign_key).records(proof).charged(charge).draws(rng, rng_mode).uniquely()
                          .answers(out_refund, status, out_key, out_counts));
}
extern "C" int act_redeem_cbor_admit_unique_batch(act_ctx* c, act_nullifier_set* set, size_t n, int mem, const uint8_t* keys, int nkeys, const uint32_t* key_epochs,
                                                  int sign_key, const uint8_t* cbor, const uint64_t* offsets, const uint8_t* charge, const uint8_t* rng, int rng_mode,
                                                  uint8_t* out_refund_cbor, uint8_t* status, uint8_t* out_key, uint64_t* out_counts) {
  if (n && !cbor) return ACT_ERR_ARG;
  return redeem_admit(AdmitCall(c, set, n, mem).ring(keys, nkeys, key_epochs, sign_key).messages(cbor, offsets).charged(charge).draws(rng, rng_mode).uniquely()
                          .answers(out_refund_cbor, status, out_key, out_counts));
}

// ---- partial refunds (DESIGN 4.10): the admission calls with the amounts t the issuer returns ---------------------------------------------
// The admission loop with one more rule in the screen (t_i > s_i -> ACT_STATUS_RETURN_TOO_BIG, behind the charge and in front of the
// look-up) and a signing step over X_A = g + K' + t h1; 160-byte RefundReturn records or ACT_CBOR_REFUND_RETURN messages.  Drawn nonces
// here; the replay form with amounts is act_redeem_(cbor_)return_replay_batch (admit_replay_impl.inc), where t enters the receipt's tag
// and the nonce derivation -- with e derived from (nonce_key, key, k, enc(K')) alone, two signatures with one e over X_A that differ by
// a multiple of h1 would give h1 (e + x)^-1 away.  (Lanes without an input pointer: redeem_admit zeroes the counts, then refuses.)
extern "C" int act_redeem_return_batch(act_ctx* c, act_nullifier_set* set, size_t n, int mem, const uint8_t* keys, int nkeys, const uint32_t* key_epochs, int sign_key,
                                       const uint8_t* proof, const uint8_t* charge, const uint8_t* returned, const uint8_t* rng, int rng_mode,
                                       uint8_t* out_refund_return, uint8_t* status, uint8_t* out_key, uint64_t* out_counts) {
  return redeem_admit(AdmitCall(c, set, n, mem).ring(keys, nkeys, key_epochs, sign_key).records(proof).charged(charge).returns(returned).draws(rng, rng_mode)
                          .answers(out_refund_return, status, out_key, out_counts));
}
extern "C" int act_redeem_cbor_return_batch(act_ctx* c, act_nullifier_set* set, size_t n, int mem, const uint8_t* keys, int nkeys, const uint32_t* key_epochs,
                                            int sign_key, const uint8_t* cbor, const uint64_t* offsets, const uint8_t* charge, const uint8_t* returned,
                                            const uint8_t* rng, int rng_mode, uint8_t* out_refund_return_cbor, uint8_t* status, uint8_t* out_key,
                                            uint64_t* out_counts) {
  return redeem_admit(AdmitCall(c, set, n, mem).ring(keys, nkeys, key_epochs, sign_key).messages(cbor, offsets).charged(charge).returns(returned).draws(rng, rng_mode)
                          .answers(out_refund_return_cbor, status, out_key, out_counts));
}

// The return calls with the copy stage of the unique forms in its usual place, behind the screen and in front of verification.  Equality
// is decided on the proof bytes alone: t takes no part in it, because what a lane that passed the screen is answered depends on t only if
// it is the lane that is signed, and that lane is the leader -- in act_redeem_(cbor_)return_batch lanes that share a fresh nullifier are
// all verified and the first valid one in lane order wins, whatever the others' t.  A lane the screen sheds (t > s among the reasons) is
// neither a leader nor a copy.  out_counts: ACT_REDEEM_RETURN_UNIQUE_COUNTS values.
extern "C" int act_redeem_return_unique_batch(act_ctx* c, act_nullifier_set* set, size_t n, int mem, const uint8_t* keys, int nkeys, const uint32_t* key_epochs,
                                              int sign_key, const uint8_t* proof, const uint8_t* charge, const uint8_t* returned, const uint8_t* rng, int rng_mode,
                                              uint8_t* out_refund_return, uint8_t* status, uint8_t* out_key, uint64_t* out_counts) {
  return redeem_admit(AdmitCall(c, set, n, mem).ring(keys, nkeys, key_epochs, sign_key).records(proof).charged(charge).returns(returned).draws(rng, rng_mode).uniquely()
                          .answers(out_refund_return, status, out_key, out_counts));
}
extern "C" int act_redeem_cbor_return_unique_batch(act_ctx* c, act_nullifier_set* set, size_t n, int mem, const uint8_t* keys, int nkeys, const uint32_t* key_epochs,
                                                   int sign_key, const uint8_t* cbor, const uint64_t* offsets, const uint8_t* charge, const uint8_t* returned,
                                                   const uint8_t* rng, int rng_mode, uint8_t* out_refund_return_cbor, uint8_t* status, uint8_t* out_key,
                                                   uint64_t* out_counts) {
  return redeem_admit(AdmitCall(c, set, n, mem).ring(keys, nkeys, key_epochs, sign_key).messages(cbor, offsets).charged(charge).returns(returned).draws(rng, rng_mode)
                          .uniquely().answers(out_refund_return_cbor, status, out_key, out_counts));
}
