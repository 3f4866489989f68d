// nullifier_impl.inc — GPU nullifier set (SURVEY.md section 8f "next" #4), included by engine.hip.
//
// The reference leaves double-spend detection to the caller (/root/reference/src/lib.rs:741-745); its tests
// and example use `HashSet<Scalar>` with "if is_spent(k) reject else insert(k)" per spend, in order
// (src/tests.rs:29-50, examples/act.rs:10-30).  act_nullifier_check_and_insert_batch gives a batch exactly
// that sequential meaning: lane i is reported spent iff its nullifier is already in the set OR equals the
// nullifier of an earlier unmasked lane j < i of the same batch; every fresh nullifier is inserted once.
//
// Two phases, no spin waits, no same-key write races:
//   1. intra-batch: a scratch open-addressing table of LANE INDICES (keys are read from the immutable input by
//      index).  Lanes with equal keys walk the same probe sequence and meet in one slot; atomicMin keeps the
//      smallest lane there (k_null_claim); a second pass marks every lane that is not its slot's winner as a
//      duplicate (k_null_resolve).
//   2. persistent table (32-byte key + state word per slot): only the winners look up / insert, so all keys in
//      flight are distinct — a lane that meets a slot being written by another lane knows it holds a different key
//      and just probes on.  A slot is only ever given back by act_nullifier_set_retire_epoch, which builds a new table.
// The state word of a slot: low 8 bits 0 empty / 1 being written / 2 committed; high 24 bits the EPOCH the key was recorded under
// (the caller's name for the issuer key the token was spent under; 0 = untagged, what every call without epochs records, so an
// untagged slot keeps the bit pattern 2).  Membership ignores the epoch; it is metadata for counting, export and retirement.
// Keys are the nullifier SCALARS, not their bytes: every key is reduced mod l as it is loaded (the reference's set is a
// `HashSet<Scalar>` and a Rust Scalar is always canonical, src/cbor.rs:85), so a raw record carrying k + l -- which the
// verifier accepts, because it reduces k too -- is the same key as k.
// Slots come from SipHash-1-3 of the reduced key under a 128-bit per-set key (`salt`; drawn from the OS when the caller
// passes none): clients choose their nullifiers, and without the key they cannot aim them at one probe chain.  The batch
// table starts at the low half of the 64-bit hash, the persistent table at the high half.

#include "null_probe.h"      // null_load_key, null_hash, null_eq, NullSalt, null_probe_contains
#include "merge_spent.h"     // merge_spent

namespace {

struct NullArgs {
  uint32_t n; uint32_t stride;              // nullifier i at keys + i*stride (32 bytes, e.g. the `k` field of a SpendProof record)
  const uint8_t* keys; const uint8_t* mask; // mask: nullable; lanes with mask[i] != 0 are skipped (e.g. rejected proofs)
  uint32_t* batch_tab; uint32_t batch_cap;  // power of two, >= 2n, filled with 0xFFFFFFFF
  uint32_t* tab_keys; uint32_t* tab_state; uint32_t tab_cap;   // persistent table; state 0 empty, 1 being written, 2 committed
  uint32_t salt[4];
  uint8_t* spent; uint32_t* counters;       // counters[0] = inserted count, counters[1] = table-full flag, counters[2] = bad-epoch-index flag
  const uint8_t* eidx; const uint32_t* etab; uint32_t n_epochs;   // eidx nullable: lane i commits (etab[eidx[i]] << 8 | 2); etab in device memory
  uint32_t commit0;                         // the state word every lane commits when eidx is null
};
// a lane whose epoch index names no table entry is left out of the batch altogether (as if masked) and answered undetermined
__device__ __forceinline__ bool null_bad_index(const NullArgs& a, uint32_t i) { return a.eidx && a.eidx[i] >= a.n_epochs; }

__global__ void __launch_bounds__(256) k_null_claim(NullArgs a) {
  uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n || (a.mask && a.mask[i]) || null_bad_index(a, i)) return;
  uint32_t w[8], o[8]; null_load_key(w, a.keys + (size_t)i * a.stride);
  uint32_t s = (uint32_t)null_hash(w, a.salt) & (a.batch_cap - 1);
  for (;;) {
    uint32_t v = atomicCAS(a.batch_tab + s, 0xFFFFFFFFu, i);
    if (v == 0xFFFFFFFFu) return;                                        // claimed an empty slot
    null_load_key(o, a.keys + (size_t)v * a.stride);
    if (null_eq(w, o)) { atomicMin(a.batch_tab + s, i); return; }        // same nullifier: the smallest lane wins
    s = (s + 1) & (a.batch_cap - 1);
  }
}
__global__ void __launch_bounds__(256) k_null_resolve(NullArgs a) {
  uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  if (a.mask && a.mask[i]) { a.spent[i] = 0; return; }
  if (null_bad_index(a, i)) { atomicExch(a.counters + 2, 1u); a.spent[i] = ACT_NULLIFIER_UNDETERMINED; return; }
  uint32_t w[8], o[8]; null_load_key(w, a.keys + (size_t)i * a.stride);
  uint32_t s = (uint32_t)null_hash(w, a.salt) & (a.batch_cap - 1);
  for (;;) {                                                             // find this key's slot (it exists)
    uint32_t v = a.batch_tab[s];
    if (v == 0xFFFFFFFFu) { a.spent[i] = 0; return; }                    // only reachable if the caller mutated the keys mid-call
    null_load_key(o, a.keys + (size_t)v * a.stride);
    if (null_eq(w, o)) { if (v != i) { a.spent[i] = 1; return; } break; }   // an earlier lane of this batch spends it first
    s = (s + 1) & (a.batch_cap - 1);
  }
  // winner: look up / insert in the persistent table
  uint32_t t = (uint32_t)(null_hash(w, a.salt) >> 32) & (a.tab_cap - 1);   // the other half of the hash starts the big table
  const uint32_t commit = a.eidx ? (a.etab[a.eidx[i]] << 8 | 2u) : a.commit0;
  for (uint32_t probes = 0; probes < a.tab_cap; probes++) {
    uint32_t st = atomicCAS(a.tab_state + t, 0u, 1u);
    if (st == 0u) {                                                      // empty: ours
      uint32_t* dst = a.tab_keys + (size_t)t * 8;
      for (int k = 0; k < 8; k++) dst[k] = w[k];
      __threadfence();
      atomicExch(a.tab_state + t, commit);
      atomicAdd(a.counters, 1u);
      a.spent[i] = 0; return;
    }
    if ((st & 0xFFu) == 2u) {                                            // committed by an earlier batch (this batch's keys are all distinct)
      const uint32_t* src = a.tab_keys + (size_t)t * 8;
      for (int k = 0; k < 8; k++) o[k] = src[k];
      if (null_eq(w, o)) { a.spent[i] = 1; return; }
    }
    t = (t + 1) & (a.tab_cap - 1);                                       // st == 1: another lane's (different) key is landing here
  }
  atomicExch(a.counters + 1, 1u);                                        // table full: this lane is neither found nor recorded
  a.spent[i] = ACT_NULLIFIER_UNDETERMINED;
}
// a call that fails before it has looked anything up still answers every lane: undetermined (nothing was recorded)
__global__ void __launch_bounds__(256) k_null_mark_undetermined(uint8_t* spent, const uint8_t* mask, uint32_t n) {
  uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) spent[i] = (mask && mask[i]) ? 0 : ACT_NULLIFIER_UNDETERMINED;
}

// ---- export, rehash, read-only look-up (not on the redemption path: simple, bandwidth-shaped) ------------------------------
// Committed slots of [begin, begin + count) -> out[*], dense, order unspecified.  One thread per slot: the state words are read
// coalesced, every wave compacts its committed lanes with a ballot and takes its output range with ONE atomicAdd on counter[0];
// a key moves as two 16-byte loads and two 16-byte stores (slots are 32-byte aligned, `out` is 16-byte aligned).  out_ep (nullable):
// the epoch of key `at` beside it.
__global__ void __launch_bounds__(256) k_null_export(const uint32_t* tab_keys, const uint32_t* tab_state, uint32_t begin, uint32_t count,
                                                     uint4* out, uint32_t* out_ep, uint32_t* counter) {
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  const uint32_t st = j < count ? tab_state[begin + j] : 0u;
  const bool live = (st & 0xFFu) == 2u;
  const unsigned long long m = __ballot(live);
  if (m == 0) return;
  const uint32_t lane = __lane_id(), first = (uint32_t)__ffsll((long long)m) - 1;
  uint32_t base = 0;
  if (lane == first) base = atomicAdd(counter, (uint32_t)__popcll(m));
  base = __shfl(base, (int)first);
  if (!live) return;
  const uint32_t at = base + (uint32_t)__popcll(m & ((1ull << lane) - 1));   // committed lanes below this one in the wave
  const uint4* src = reinterpret_cast<const uint4*>(tab_keys + (size_t)(begin + j) * 8);
  const uint4 lo = src[0], hi = src[1];
  out[(size_t)at * 2] = lo; out[(size_t)at * 2 + 1] = hi;
  if (out_ep) out_ep[at] = st >> 8;
}
// counter[0] += the slots of the table whose state word is `want` (a committed slot of one epoch): the state words only, 4 bytes per
// slot, read 16 bytes per lane in a grid-stride loop (cap is a multiple of 1024), summed over the wave, ONE atomic per wave of the
// grid -- a few thousand in all, where one atomic per 64 slots on the one counter would serialise (6 ms for 2^25 slots).
__global__ void __launch_bounds__(256) k_null_count_state(const uint4* tab_state4, uint32_t cap4, uint32_t want, uint32_t* counter) {
  uint32_t mine = 0;
  for (uint32_t j = blockIdx.x * 256 + threadIdx.x; j < cap4; j += gridDim.x * 256) {
    const uint4 v = tab_state4[j];
    mine += (v.x == want) + (v.y == want) + (v.z == want) + (v.w == want);
  }
  for (int off = 32; off; off >>= 1) mine += __shfl_down(mine, off);
  if (__lane_id() == 0 && mine) atomicAdd(counter, mine);
}
// Every committed slot of the old table into the new one (same salt, same slot function, masked to the new capacity).  The keys are
// known distinct, so a slot is claimed by a compare-and-swap 0 -> its old state word (committed, epoch carried over) and no key is
// compared; nothing reads the new table before the kernel has finished.  `drop`: the state word of the slots that are left behind
// (the committed slots of a retired epoch); 0 = none.  counter[0] += keys placed (one atomic per wave), counter[1] = 1 if a key
// found no slot.
__global__ void __launch_bounds__(256) k_null_rehash(const uint32_t* old_keys, const uint32_t* old_state, uint32_t old_cap, uint32_t* new_keys,
                                                     uint32_t* new_state, uint32_t new_cap, NullSalt salt, uint32_t drop, uint32_t* counter) {
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  bool placed = false;
  const uint32_t st = j < old_cap ? old_state[j] : 0u;
  if ((st & 0xFFu) == 2u && st != drop) {
    const uint4* src = reinterpret_cast<const uint4*>(old_keys + (size_t)j * 8);
    const uint4 lo = src[0], hi = src[1];
    const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    uint32_t t = (uint32_t)(null_hash(w, salt.w) >> 32) & (new_cap - 1);
    for (uint32_t probes = 0; probes < new_cap; probes++) {
      if (atomicCAS(new_state + t, 0u, st) == 0u) {
        uint4* dst = reinterpret_cast<uint4*>(new_keys + (size_t)t * 8);
        dst[0] = lo; dst[1] = hi;
        placed = true;
        break;
      }
      t = (t + 1) & (new_cap - 1);
    }
    if (!placed) atomicExch(counter + 1, 1u);
  }
  const unsigned long long m = __ballot(placed);
  if (m && __lane_id() == (uint32_t)__ffsll((long long)m) - 1) atomicAdd(counter, (uint32_t)__popcll(m));
}
// Read-only look-up: found[i] = 1 iff the reduced key i is committed.  Probes from the persistent table's start slot until the key
// (found) or an empty slot (absent); no batch table, no write to the set.  The caller holds the set's lock, so no slot is being written.
__global__ void __launch_bounds__(256) k_null_contains(const uint8_t* keys, uint32_t n, uint32_t stride, const uint32_t* tab_keys,
                                                       const uint32_t* tab_state, uint32_t tab_cap, NullSalt salt, uint8_t* found) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint32_t w[8]; null_load_key(w, keys + (size_t)i * stride);
  const uint8_t f = null_probe_contains(w, tab_keys, tab_state, tab_cap, salt.w) ? 1 : 0;
  found[i] = f;
}

}  // namespace

struct act_nullifier_set {
  int device = 0; hipStream_t stream = nullptr;
  uint32_t *tab_keys = nullptr, *tab_state = nullptr, *batch_tab = nullptr, *counters = nullptr;
  uint32_t tab_cap = 0, batch_cap = 0; uint32_t salt[4]{};
  uint8_t *d_keys = nullptr, *d_mask = nullptr, *d_spent = nullptr, *d_eidx = nullptr; size_t stage_cap = 0;
  uint8_t* d_xout = nullptr; size_t xout_cap = 0; uint32_t* aux = nullptr;   // export staging (host output), export / rehash counters
  uint32_t* d_xep = nullptr; size_t xep_cap = 0;                              // export staging of the epochs
  uint32_t* d_etab = nullptr; uint32_t h_etab[256]{};                         // the epoch table of the call in flight (device copy, its host source)
  std::vector<uint32_t> retired;  // ascending; an insert that names one of them is refused
  uint32_t gen = 0;               // table instance: counts the retirements that removed a key (export cursors carry it)
  size_t len = 0; std::string err;
  std::mutex mu;                  // check_and_insert holds it: a set shared between host threads serves them one at a time
};

#define NSCK(s, expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { (s)->err = std::string(#expr) + ": " + hipGetErrorString(e_); (void)hipGetLastError(); return ACT_ERR_HIP; } } while (0)

extern "C" {

int act_nullifier_set_create(int device, size_t capacity, const uint8_t salt[16], act_nullifier_set** out) {
  if (!out || capacity == 0 || capacity > ((size_t)1 << 30)) return ACT_ERR_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return ACT_ERR_NO_DEVICE;
  if (device < 0 || device >= ndev) return ACT_ERR_ARG;
  act_nullifier_set* s = new act_nullifier_set();
  *out = s; s->device = device;
  uint32_t cap = 1024; while (cap < 2 * capacity) cap <<= 1;             // load factor <= 1/2
  s->tab_cap = cap;
  if (salt) memcpy(s->salt, salt, 16);
  else if (getrandom(s->salt, 16, 0) != 16) { s->err = "getrandom failed"; return ACT_ERR_ARG; }   // never a public constant
  NSCK(s, hipSetDevice(device));
  NSCK(s, hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
  NSCK(s, hipMalloc(&s->tab_keys, (size_t)cap * 32)); NSCK(s, hipMalloc(&s->tab_state, (size_t)cap * 4)); NSCK(s, hipMalloc(&s->counters, 16));
  NSCK(s, hipMemsetAsync(s->tab_state, 0, (size_t)cap * 4, s->stream)); NSCK(s, hipMemsetAsync(s->counters, 0, 16, s->stream));
  NSCK(s, hipStreamSynchronize(s->stream));
  return ACT_OK;
}
void act_nullifier_set_destroy(act_nullifier_set* s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  void* ptrs[] = {s->tab_keys, s->tab_state, s->batch_tab, s->counters, s->d_keys, s->d_mask, s->d_spent, s->d_eidx, s->d_xout, s->aux, s->d_xep, s->d_etab};
  for (void* p : ptrs) if (p) (void)hipFree(p);
  if (s->stream) (void)hipStreamDestroy(s->stream);
  delete s;
}
size_t act_nullifier_set_len(const act_nullifier_set* s) { return s ? s->len : 0; }
const char* act_nullifier_set_last_error(const act_nullifier_set* s) {
  if (!s) return "null set";
  thread_local std::string mine;
  { std::lock_guard<std::mutex> lk(const_cast<act_nullifier_set*>(s)->mu); mine = s->err; }
  return mine.c_str();
}

}  // extern "C"

namespace {
// the staging buffers of the host-memory calls: keys, mask, answers and epoch indices of n lanes
int null_stage(act_nullifier_set* s, size_t n) {
  if (n <= s->stage_cap) return ACT_OK;
  for (uint8_t** p : {&s->d_keys, &s->d_mask, &s->d_spent, &s->d_eidx}) if (*p) { NSCK(s, hipFree(*p)); *p = nullptr; }
  s->stage_cap = 0;
  NSCK(s, hipMalloc(&s->d_keys, n * 32)); NSCK(s, hipMalloc(&s->d_mask, n)); NSCK(s, hipMalloc(&s->d_spent, n)); NSCK(s, hipMalloc(&s->d_eidx, n));
  s->stage_cap = n;
  return ACT_OK;
}
// "" if every epoch of the table may be recorded under, else why not.  Caller holds s->mu.
std::string null_epochs_refused(const act_nullifier_set* s, const uint32_t* tab, int n_epochs) {
  for (int k = 0; k < n_epochs; k++) {
    if (tab[k] > ACT_NULLIFIER_EPOCH_MAX) return "epoch " + std::to_string(tab[k]) + " is above ACT_NULLIFIER_EPOCH_MAX";
    if (std::binary_search(s->retired.begin(), s->retired.end(), tab[k])) return "epoch " + std::to_string(tab[k]) + " has been retired";
  }
  return std::string();
}
// One body for act_nullifier_check_and_insert_batch (table {0}, no indices) and act_nullifier_check_and_insert_epoch_batch.
int null_insert_impl(act_nullifier_set* s, size_t n, int mem, const uint8_t* nullifiers, size_t stride, const uint8_t* skip_mask, const uint8_t* epoch_index,
                     const uint32_t* epoch_table, int n_epochs, uint8_t* out_spent) {
  if (!s || (n && (!nullifiers || !out_spent)) || stride < 32 || n > ((size_t)1 << 30) || !epoch_table || n_epochs < 1 || n_epochs > 255) return ACT_ERR_ARG;
  std::lock_guard<std::mutex> lock(s->mu);
  // a call that is refused as a whole records nothing: every unmasked lane is ACT_NULLIFIER_UNDETERMINED
  auto refuse = [&](const std::string& why) {
    s->err = why;
    if (n == 0) return ACT_ERR_ARG;
    if (mem == ACT_MEM_HOST) { for (size_t i = 0; i < n; i++) out_spent[i] = (skip_mask && skip_mask[i]) ? 0 : ACT_NULLIFIER_UNDETERMINED; }
    else if (hipSetDevice(s->device) == hipSuccess) {
      hipLaunchKernelGGL(k_null_mark_undetermined, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, out_spent, skip_mask, (uint32_t)n);
      if (hipStreamSynchronize(s->stream) != hipSuccess) (void)hipGetLastError();
    }
    return ACT_ERR_ARG;
  };
  const std::string bad_epoch = null_epochs_refused(s, epoch_table, n_epochs);
  if (!bad_epoch.empty()) return refuse("nullifier set: " + bad_epoch);
  if (n == 0) return ACT_OK;
  NSCK(s, hipSetDevice(s->device));
  // (resubmit to this set after act_nullifier_set_reserve)
  if (s->len + n > s->tab_cap / 2) return refuse("nullifier set capacity exceeded");
  uint32_t bcap = 1024; while (bcap < 2 * n) bcap <<= 1;
  if (bcap > s->batch_cap) { if (s->batch_tab) NSCK(s, hipFree(s->batch_tab)); s->batch_tab = nullptr; NSCK(s, hipMalloc(&s->batch_tab, (size_t)bcap * 4)); s->batch_cap = bcap; }
  NSCK(s, hipMemsetAsync(s->batch_tab, 0xFF, (size_t)bcap * 4, s->stream));
  NullArgs a{}; a.n = (uint32_t)n; a.batch_tab = s->batch_tab; a.batch_cap = bcap; a.tab_keys = s->tab_keys; a.tab_state = s->tab_state;
  a.tab_cap = s->tab_cap; memcpy(a.salt, s->salt, 16); a.counters = s->counters;
  a.commit0 = epoch_table[0] << 8 | 2u; a.n_epochs = (uint32_t)n_epochs;
  if (epoch_index) {
    if (!s->d_etab) NSCK(s, hipMalloc(&s->d_etab, sizeof(s->h_etab)));
    memcpy(s->h_etab, epoch_table, (size_t)n_epochs * 4);
    NSCK(s, hipMemcpyAsync(s->d_etab, s->h_etab, (size_t)n_epochs * 4, hipMemcpyHostToDevice, s->stream));
    a.etab = s->d_etab;
  }
  if (mem == ACT_MEM_DEVICE) { a.keys = nullifiers; a.stride = (uint32_t)stride; a.mask = skip_mask; a.spent = out_spent; a.eidx = epoch_index; }
  else {
    if (int rc = null_stage(s, n)) return rc;
    NSCK(s, hipMemcpy2DAsync(s->d_keys, 32, nullifiers, stride, 32, n, hipMemcpyHostToDevice, s->stream));   // gather the 32-byte fields
    if (skip_mask) NSCK(s, hipMemcpyAsync(s->d_mask, skip_mask, n, hipMemcpyHostToDevice, s->stream));
    if (epoch_index) NSCK(s, hipMemcpyAsync(s->d_eidx, epoch_index, n, hipMemcpyHostToDevice, s->stream));
    a.keys = s->d_keys; a.stride = 32; a.mask = skip_mask ? s->d_mask : nullptr; a.spent = s->d_spent; a.eidx = epoch_index ? s->d_eidx : nullptr;
  }
  hipLaunchKernelGGL(k_null_claim, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, a);
  hipLaunchKernelGGL(k_null_resolve, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, a);
  uint32_t cnt[3];
  NSCK(s, hipMemcpyAsync(cnt, s->counters, 12, hipMemcpyDeviceToHost, s->stream));
  if (mem == ACT_MEM_HOST) NSCK(s, hipMemcpyAsync(out_spent, s->d_spent, n, hipMemcpyDeviceToHost, s->stream));
  NSCK(s, hipStreamSynchronize(s->stream));
  s->len = cnt[0];
  if (cnt[1] || cnt[2]) {                                      // [1] cannot happen below the load factor checked above; answered per lane all the same
    s->err = cnt[1] ? "nullifier table full: the lanes reported ACT_NULLIFIER_UNDETERMINED were neither found nor recorded"
                    : "epoch index not below n_epochs: the lanes reported ACT_NULLIFIER_UNDETERMINED were neither looked up nor recorded";
    NSCK(s, hipMemsetAsync(s->counters + 1, 0, 8, s->stream)); NSCK(s, hipStreamSynchronize(s->stream));
    return ACT_ERR_ARG;
  }
  return ACT_OK;
}
}  // namespace

extern "C" {

int act_nullifier_check_and_insert_batch(act_nullifier_set* s, size_t n, int mem, const uint8_t* nullifiers, size_t stride,
                                         const uint8_t* skip_mask, uint8_t* out_spent) {
  static const uint32_t untagged = 0;
  return null_insert_impl(s, n, mem, nullifiers, stride, skip_mask, nullptr, &untagged, 1, out_spent);
}
int act_nullifier_check_and_insert_epoch_batch(act_nullifier_set* s, size_t n, int mem, const uint8_t* nullifiers, size_t stride, const uint8_t* skip_mask,
                                               const uint8_t* epoch_index, const uint32_t* epoch_table, int n_epochs, uint8_t* out_spent) {
  return null_insert_impl(s, n, mem, nullifiers, stride, skip_mask, epoch_index, epoch_table, n_epochs, out_spent);
}

// Growth: a new table sized by the rule of act_nullifier_set_create, every committed key rehashed into it on the device, then the
// old one freed.  Any failure before the swap frees the new table and leaves the set exactly as it was.
int act_nullifier_set_reserve(act_nullifier_set* s, size_t capacity) {
  if (!s) return ACT_ERR_ARG;
  std::lock_guard<std::mutex> lock(s->mu);
  if (capacity > ((size_t)1 << 30)) { s->err = "act_nullifier_set_reserve: capacity above 2^30"; return ACT_ERR_ARG; }
  uint32_t cap = 1024; while (cap < 2 * capacity) cap <<= 1;
  if (cap <= s->tab_cap) return ACT_OK;                                   // never shrinks; already large enough
  NSCK(s, hipSetDevice(s->device));
  uint32_t *nk = nullptr, *ns = nullptr;
  auto fail = [&](const std::string& what, hipError_t e) {
    s->err = "act_nullifier_set_reserve: " + what + (e != hipSuccess ? std::string(": ") + hipGetErrorString(e) : std::string());
    (void)hipGetLastError();
    if (nk) (void)hipFree(nk);
    if (ns) (void)hipFree(ns);
    return ACT_ERR_HIP;
  };
  hipError_t e;
  if (!s->aux && (e = hipMalloc(&s->aux, 8)) != hipSuccess) { s->aux = nullptr; return fail("hipMalloc(counters)", e); }
  if ((e = hipMalloc(&nk, (size_t)cap * 32)) != hipSuccess) { nk = nullptr; return fail("hipMalloc(new table keys)", e); }
  if ((e = hipMalloc(&ns, (size_t)cap * 4)) != hipSuccess) { ns = nullptr; return fail("hipMalloc(new table states)", e); }
  if ((e = hipMemsetAsync(ns, 0, (size_t)cap * 4, s->stream)) != hipSuccess) return fail("hipMemsetAsync", e);
  if ((e = hipMemsetAsync(s->aux, 0, 8, s->stream)) != hipSuccess) return fail("hipMemsetAsync", e);
  NullSalt salt; memcpy(salt.w, s->salt, 16);
  hipLaunchKernelGGL(k_null_rehash, dim3((s->tab_cap + 255) / 256), dim3(256), 0, s->stream, s->tab_keys, s->tab_state, s->tab_cap, nk, ns, cap, salt, 0u, s->aux);
  if ((e = hipGetLastError()) != hipSuccess) return fail("k_null_rehash launch", e);
  uint32_t cnt[2] = {0, 0};
  if ((e = hipMemcpyAsync(cnt, s->aux, 8, hipMemcpyDeviceToHost, s->stream)) != hipSuccess) return fail("hipMemcpyAsync", e);
  if ((e = hipStreamSynchronize(s->stream)) != hipSuccess) return fail("k_null_rehash", e);
  if (cnt[1] || cnt[0] != s->len)
    return fail("rehash placed " + std::to_string(cnt[0]) + " of " + std::to_string(s->len) + " keys; the old table is kept", hipSuccess);
  (void)hipFree(s->tab_keys); (void)hipFree(s->tab_state);
  s->tab_keys = nk; s->tab_state = ns; s->tab_cap = cap;
  return ACT_OK;
}

// Export cursor: 0 = start; ACT_NULLIFIER_EXPORT_DONE = finished; otherwise table instance << 37 | log2(table slots) << 32 | next
// slot.  A reserve that changes anything changes the table size and a retirement that removes a key counts the instance up (14 bits,
// so a cursor kept across 16384 such retirements could be taken for a fresh one), so the two name the table a cursor walks.  Below 2^51.
}  // extern "C"
namespace {
int null_export_impl(act_nullifier_set* s, uint64_t* cursor, size_t max_keys, int mem, uint8_t* out_keys, uint32_t* out_epochs, bool epochs, size_t* n_out) {
  if (!s || !cursor || !n_out || !max_keys || !out_keys || (epochs && !out_epochs) || (mem != ACT_MEM_HOST && mem != ACT_MEM_DEVICE)) return ACT_ERR_ARG;
  std::lock_guard<std::mutex> lock(s->mu);
  *n_out = 0;
  if (*cursor == ACT_NULLIFIER_EXPORT_DONE) return ACT_OK;
  const uint64_t tag = (uint64_t)(s->gen & 0x3FFFu) << 5 | (uint32_t)__builtin_ctz(s->tab_cap);
  uint64_t slot = 0;
  if (*cursor != 0) {
    slot = *cursor & 0xFFFFFFFFull;
    if ((*cursor >> 32) != tag || slot >= s->tab_cap) {
      s->err = "act_nullifier_set_export: stale or foreign cursor (the set was reserved or an epoch retired since it was taken): restart from 0";
      return ACT_ERR_ARG;
    }
  }
  size_t window = std::min<size_t>(max_keys, s->tab_cap - slot);          // one slot holds at most one key: never more than max_keys
  const bool stage = mem == ACT_MEM_HOST || (reinterpret_cast<uintptr_t>(out_keys) & 15u) || (epochs && (reinterpret_cast<uintptr_t>(out_epochs) & 3u));
  if (stage) window = std::min<size_t>(window, (size_t)1 << 21);         // staging of at most 64 MB (+ 8 MB of epochs)
  NSCK(s, hipSetDevice(s->device));
  if (!s->aux) NSCK(s, hipMalloc(&s->aux, 8));
  if (stage && window > s->xout_cap) {
    if (s->d_xout) { NSCK(s, hipFree(s->d_xout)); s->d_xout = nullptr; s->xout_cap = 0; }
    NSCK(s, hipMalloc(&s->d_xout, window * 32)); s->xout_cap = window;
  }
  if (stage && epochs && window > s->xep_cap) {
    if (s->d_xep) { NSCK(s, hipFree(s->d_xep)); s->d_xep = nullptr; s->xep_cap = 0; }
    NSCK(s, hipMalloc(&s->d_xep, window * 4)); s->xep_cap = window;
  }
  uint8_t* dst = stage ? s->d_xout : out_keys;
  uint32_t* dst_ep = !epochs ? nullptr : stage ? s->d_xep : out_epochs;
  NSCK(s, hipMemsetAsync(s->aux, 0, 4, s->stream));
  hipLaunchKernelGGL(k_null_export, dim3((unsigned)((window + 255) / 256)), dim3(256), 0, s->stream, s->tab_keys, s->tab_state, (uint32_t)slot,
                     (uint32_t)window, reinterpret_cast<uint4*>(dst), dst_ep, s->aux);
  NSCK(s, hipGetLastError());
  uint32_t got = 0;
  NSCK(s, hipMemcpyAsync(&got, s->aux, 4, hipMemcpyDeviceToHost, s->stream));
  NSCK(s, hipStreamSynchronize(s->stream));
  if (stage && got) {
    const hipMemcpyKind kind = mem == ACT_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    NSCK(s, hipMemcpyAsync(out_keys, s->d_xout, (size_t)got * 32, kind, s->stream));
    if (epochs) NSCK(s, hipMemcpyAsync(out_epochs, s->d_xep, (size_t)got * 4, kind, s->stream));
    NSCK(s, hipStreamSynchronize(s->stream));
  }
  const uint64_t next = slot + window;
  *cursor = next >= s->tab_cap ? ACT_NULLIFIER_EXPORT_DONE : (tag << 32 | next);
  *n_out = got;
  return ACT_OK;
}
// the committed slots of one epoch, counted on the device.  Caller holds s->mu and has set the device.
int null_count_epoch(act_nullifier_set* s, uint32_t epoch, uint64_t* out) {
  if (!s->aux) NSCK(s, hipMalloc(&s->aux, 8));
  NSCK(s, hipMemsetAsync(s->aux, 0, 4, s->stream));
  const uint32_t cap4 = s->tab_cap / 4;
  hipLaunchKernelGGL(k_null_count_state, dim3(std::min<uint32_t>((cap4 + 255) / 256, 4096u)), dim3(256), 0, s->stream, reinterpret_cast<const uint4*>(s->tab_state), cap4,
                     epoch << 8 | 2u, s->aux);
  NSCK(s, hipGetLastError());
  uint32_t got = 0;
  NSCK(s, hipMemcpyAsync(&got, s->aux, 4, hipMemcpyDeviceToHost, s->stream));
  NSCK(s, hipStreamSynchronize(s->stream));
  *out = got;
  return ACT_OK;
}
}  // namespace
extern "C" {
int act_nullifier_set_export(act_nullifier_set* s, uint64_t* cursor, size_t max_keys, int mem, uint8_t* out_keys, size_t* n_out) {
  return null_export_impl(s, cursor, max_keys, mem, out_keys, nullptr, false, n_out);
}
int act_nullifier_set_export_epochs(act_nullifier_set* s, uint64_t* cursor, size_t max_keys, int mem, uint8_t* out_keys, uint32_t* out_epochs, size_t* n_out) {
  return null_export_impl(s, cursor, max_keys, mem, out_keys, out_epochs, true, n_out);
}

int act_nullifier_set_epoch_len(act_nullifier_set* s, uint32_t epoch, uint64_t* out_count) {
  if (!s || !out_count) return ACT_ERR_ARG;
  *out_count = 0;
  if (epoch > ACT_NULLIFIER_EPOCH_MAX) return ACT_OK;                     // no such epoch: nothing is recorded under it
  std::lock_guard<std::mutex> lock(s->mu);
  NSCK(s, hipSetDevice(s->device));
  return null_count_epoch(s, epoch, out_count);
}

// Retirement: built like reserve.  A second table of the same capacity takes every committed slot of another epoch (state word and
// all), the tables are swapped, the old one freed.  Any failure before the swap frees the new table, leaves the set exactly as it
// was and does not mark the epoch retired.
int act_nullifier_set_retire_epoch(act_nullifier_set* s, uint32_t epoch, uint64_t* out_removed) {
  if (!s) return ACT_ERR_ARG;
  if (out_removed) *out_removed = 0;
  std::lock_guard<std::mutex> lock(s->mu);
  if (epoch == 0 || epoch > ACT_NULLIFIER_EPOCH_MAX) { s->err = "act_nullifier_set_retire_epoch: epoch 0 (untagged) and epochs above ACT_NULLIFIER_EPOCH_MAX cannot be retired"; return ACT_ERR_ARG; }
  const auto at = std::lower_bound(s->retired.begin(), s->retired.end(), epoch);
  if (at != s->retired.end() && *at == epoch) return ACT_OK;              // already retired: nothing of it is left
  NSCK(s, hipSetDevice(s->device));
  uint64_t gone = 0;
  if (int rc = null_count_epoch(s, epoch, &gone)) return rc;
  if (gone == 0) { s->retired.insert(at, epoch); return ACT_OK; }         // nothing to remove: only the refusal is armed
  const uint32_t cap = s->tab_cap;
  uint32_t *nk = nullptr, *ns = nullptr;
  auto fail = [&](const std::string& what, hipError_t e) {
    s->err = "act_nullifier_set_retire_epoch: " + what + (e != hipSuccess ? std::string(": ") + hipGetErrorString(e) : std::string());
    (void)hipGetLastError();
    if (nk) (void)hipFree(nk);
    if (ns) (void)hipFree(ns);
    return ACT_ERR_HIP;
  };
  hipError_t e;
  if ((e = hipMalloc(&nk, (size_t)cap * 32)) != hipSuccess) { nk = nullptr; return fail("hipMalloc(new table keys)", e); }
  if ((e = hipMalloc(&ns, (size_t)cap * 4)) != hipSuccess) { ns = nullptr; return fail("hipMalloc(new table states)", e); }
  if ((e = hipMemsetAsync(ns, 0, (size_t)cap * 4, s->stream)) != hipSuccess) return fail("hipMemsetAsync", e);
  if ((e = hipMemsetAsync(s->aux, 0, 8, s->stream)) != hipSuccess) return fail("hipMemsetAsync", e);
  NullSalt salt; memcpy(salt.w, s->salt, 16);
  hipLaunchKernelGGL(k_null_rehash, dim3((cap + 255) / 256), dim3(256), 0, s->stream, s->tab_keys, s->tab_state, cap, nk, ns, cap, salt, epoch << 8 | 2u, s->aux);
  if ((e = hipGetLastError()) != hipSuccess) return fail("k_null_rehash launch", e);
  uint32_t cnt[2] = {0, 0};
  if ((e = hipMemcpyAsync(cnt, s->aux, 8, hipMemcpyDeviceToHost, s->stream)) != hipSuccess) return fail("hipMemcpyAsync", e);
  if ((e = hipStreamSynchronize(s->stream)) != hipSuccess) return fail("k_null_rehash", e);
  if (cnt[1] || (uint64_t)cnt[0] + gone != s->len)
    return fail("rehash placed " + std::to_string(cnt[0]) + " of " + std::to_string(s->len) + " - " + std::to_string(gone) + " keys; the old table is kept", hipSuccess);
  // the device-side insert counter is cumulative and is read back as len after every insert: it must hold what is left
  if ((e = hipMemcpyAsync(s->counters, cnt, 4, hipMemcpyHostToDevice, s->stream)) != hipSuccess) return fail("hipMemcpyAsync(counter)", e);
  if ((e = hipStreamSynchronize(s->stream)) != hipSuccess) return fail("hipMemcpyAsync(counter)", e);
  (void)hipFree(s->tab_keys); (void)hipFree(s->tab_state);
  s->tab_keys = nk; s->tab_state = ns; s->len = cnt[0]; s->gen++;
  s->retired.insert(at, epoch);
  if (out_removed) *out_removed = gone;
  return ACT_OK;
}

int act_nullifier_set_retired_epochs(act_nullifier_set* s, uint32_t* out_epochs, size_t max_epochs, size_t* n_out) {
  if (!s || !n_out || (max_epochs && !out_epochs)) return ACT_ERR_ARG;
  std::lock_guard<std::mutex> lock(s->mu);
  *n_out = s->retired.size();
  for (size_t i = 0; i < std::min(max_epochs, s->retired.size()); i++) out_epochs[i] = s->retired[i];
  return ACT_OK;
}

int act_nullifier_contains_batch(act_nullifier_set* s, size_t n, int mem, const uint8_t* nullifiers, size_t stride, uint8_t* out_found) {
  if (!s || (n && (!nullifiers || !out_found)) || stride < 32 || n > ((size_t)1 << 30) || (mem != ACT_MEM_HOST && mem != ACT_MEM_DEVICE)) return ACT_ERR_ARG;
  if (n == 0) return ACT_OK;
  std::lock_guard<std::mutex> lock(s->mu);
  NSCK(s, hipSetDevice(s->device));
  const uint8_t* keys = nullifiers; uint8_t* found = out_found; size_t kstride = stride;
  if (mem == ACT_MEM_HOST) {
    if (int rc = null_stage(s, n)) return rc;
    NSCK(s, hipMemcpy2DAsync(s->d_keys, 32, nullifiers, stride, 32, n, hipMemcpyHostToDevice, s->stream));
    keys = s->d_keys; found = s->d_spent; kstride = 32;
  }
  NullSalt salt; memcpy(salt.w, s->salt, 16);
  hipLaunchKernelGGL(k_null_contains, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, keys, (uint32_t)n, (uint32_t)kstride, s->tab_keys,
                     s->tab_state, s->tab_cap, salt, found);
  NSCK(s, hipGetLastError());
  if (mem == ACT_MEM_HOST) NSCK(s, hipMemcpyAsync(out_found, s->d_spent, n, hipMemcpyDeviceToHost, s->stream));
  NSCK(s, hipStreamSynchronize(s->stream));
  return ACT_OK;
}

}  // extern "C"

// ---- the issuer's whole redemption step ------------------------------------------------------------------------------------
// What a server does with a batch of spends (examples/act.rs:62-73, the NullifierDb loops of src/tests.rs): verify the proof, look
// the nullifier up, record it, sign the refund -- as one call whose result is that of the loop
//     for i in 0..n:  refund(proof_i)'s checks fail            -> status_i = that error, nothing recorded, no rng drawn
//                     nullifier_i already recorded (or spent by an earlier accepted lane of this batch)
//                                                               -> status_i = DoubleSpendError (3), no rng drawn
//                     otherwise record it, sign                 -> status_i = 0, Refund_i (128 rng bytes drawn)
// Verification comes first so that a proof that does not verify cannot burn a nullifier.  (The crate's example marks the nullifier
// before it calls refund and unwraps: for valid proofs the two orders give the same result; for invalid ones the example panics.)
// Composed from the public entry points above: verify -> check-and-insert with the verdicts as skip mask -> sign the rest.
namespace {
__global__ void __launch_bounds__(256) k_merge_double_spend(uint8_t* status, const uint8_t* spent, uint32_t n) {
  uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) status[i] = merge_spent(status[i], spent[i]);
}
// the signature step failed after the nullifiers were recorded: lanes that were to be signed say so
__global__ void __launch_bounds__(256) k_mark_recorded_unsigned(uint8_t* status, const uint8_t* verdict, uint32_t n) {
  uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) status[i] = verdict[i] == 0 ? (uint8_t)ACT_STATUS_RECORDED_UNSIGNED : verdict[i];
}
}  // namespace

// Failure semantics (include/act_mi355x.h): a failure of the nullifier step or of the signature step after verification never
// loses what has already been decided -- status[] is written for every lane before the error code is returned:
//   verification failed            -> nothing recorded, status untouched, error
//   nullifier step failed          -> lanes it answered are finished as usual (signed or DoubleSpend), lanes it could not answer
//                                     get ACT_STATUS_NULLIFIER_UNDETERMINED (not recorded, not signed: safe to resubmit), error
//   signature step failed          -> lanes whose nullifier was just recorded get ACT_STATUS_RECORDED_UNSIGNED (their refund is
//                                     owed: re-run act_verify_spend_batch(out_kprime) + act_refund_sign_batch on them, never
//                                     redeem them again), all other lanes their verdict, error
// One body for records in / records out (act_redeem_batch) and wire bytes in / wire bytes out (act_redeem_cbor_batch): they differ in
// the verification call (which also says where the nullifiers are) and in the signing call (which frames its output or does not).
namespace {
__global__ void __launch_bounds__(256) k_mark_undetermined_status(uint8_t* status, const uint8_t* verdict, uint32_t n) {
  uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) status[i] = verdict[i] ? verdict[i] : (uint8_t)ACT_STATUS_NULLIFIER_UNDETERMINED;
}
}  // namespace

// Everything behind verification, ONCE for every redeem entry point (one key here; ring, epochs and admission: keyring_redeem_impl.inc),
// over arrays of n lanes in `mem` memory: st = the verdicts, sp = scratch for the store's answers.  What differs is handed in:
//   null_step(skip_mask = st, out_spent = sp) -> rc     the plain check-and-insert or the epoch insert
//   beside_merge()                                      the caller's share of the merge's pass: in device memory it runs under c->mu and
//                                                       may launch on the null stream, in front of the merge's synchronisation
//   sign_step(st, rng, rng_mode, out, status) -> rc     the signatures, rng already resolved, framed or not as the call's output is
// out_b: the bytes of one output slot (a Refund record or message; a RefundReturn's for the return calls, DESIGN 4.10)
template <class NullStep, class BesideMerge, class SignStep>
static int redeem_tail_sized(act_ctx* c, act_nullifier_set* set, size_t n, int mem, size_t out_b, uint8_t* st, uint8_t* sp, const uint8_t* rng, int rng_mode,
                             uint8_t* out, uint8_t* status, NullStep null_step, BesideMerge beside_merge, SignStep sign_step, bool signs = true) {
  // signs == false (act_redeem_(cbor_)reserve_batch, reserve_impl.inc): the last step signs nothing -- the test hook below is not for it,
  // and if it fails there is no refund owed: its lanes read as not answered, and the same call again is served as a retry
  const int rc_null = null_step(st, sp);
  // a step failed as a whole: every lane that verified says `what`, the others their verdict, and there is no output.  (Device memory:
  // best effort on a device that may just have failed a call -- the header promises a status for every lane.)
  auto give_up = [&](uint8_t what, void (*k_mark)(uint8_t*, const uint8_t*, uint32_t)) {
    if (mem == ACT_MEM_HOST) { for (size_t i = 0; i < n; i++) status[i] = st[i] ? st[i] : what; memset(out, 0, n * out_b); return; }
    std::lock_guard<std::mutex> lk(c->mu);
    (void)hipSetDevice(c->device);
    hipLaunchKernelGGL(k_mark, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, status, st, (uint32_t)n);
    (void)hipMemsetAsync(out, 0, n * out_b, nullptr);
    if (hipDeviceSynchronize() != hipSuccess) (void)hipGetLastError();
  };
  std::string null_err;
  if (rc_null) {
    null_err = std::string("nullifier set: ") + act_nullifier_set_last_error(set);
    if (rc_null == ACT_ERR_HIP) {           // the device itself failed: no per-lane answer can be trusted; nothing is signed
      c->err = null_err + " (every verified lane is undetermined)";
      give_up(ACT_STATUS_NULLIFIER_UNDETERMINED, k_mark_undetermined_status);
      return rc_null;
    }
  }
  if (mem == ACT_MEM_DEVICE) {
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(k_merge_double_spend, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, st, sp, (uint32_t)n);
    beside_merge();
    if (hipDeviceSynchronize() != hipSuccess) { c->err = "k_merge_double_spend failed"; (void)hipGetLastError(); return ACT_ERR_HIP; }
  } else {
    for (size_t i = 0; i < n; i++) st[i] = merge_spent(st[i], sp[i]);
    beside_merge();
  }
  // the generator is touched only now, for the lanes that are signed (the reference draws e, alpha after its checks, src/lib.rs:842-852)
  ResolvedRng rr(c);
  int rc_sign = rr.resolve(c, mem, st, n, rng, rng_mode);
  const bool fail_sign = signs && c->debug_fail_signs.load() > 0 && c->debug_fail_signs.fetch_sub(1) > 0;      // error-path test hook (act_debug_fail_next_signs)
  if (!rc_sign) {
    if (fail_sign) { rc_sign = ACT_ERR_HIP; c->err = "act_debug_fail_next_signs: simulated failure of the signature step"; }
    else rc_sign = sign_step(st, rng, rng_mode, out, status);
  }
  if (rc_sign && !signs) { give_up(ACT_STATUS_NULLIFIER_UNDETERMINED, k_mark_undetermined_status); return rc_sign; }
  if (rc_sign) { give_up(ACT_STATUS_RECORDED_UNSIGNED, k_mark_recorded_unsigned); return rc_sign; }      // the nullifiers ARE recorded: the refunds are owed
  if (rc_null) c->err = null_err;
  return rc_null;
}

template <class NullStep, class BesideMerge, class SignStep>
static int redeem_tail(act_ctx* c, act_nullifier_set* set, size_t n, int mem, bool wire, uint8_t* st, uint8_t* sp, const uint8_t* rng, int rng_mode,
                       uint8_t* out, uint8_t* status, NullStep null_step, BesideMerge beside_merge, SignStep sign_step) {
  return redeem_tail_sized(c, set, n, mem, wire ? act_cbor_size(c, ACT_CBOR_REFUND) : (size_t)128, st, sp, rng, rng_mode, out, status, null_step, beside_merge, sign_step);
}

static int redeem_impl(act_ctx* c, act_nullifier_set* set, size_t n, int mem, const uint8_t sk[64], const uint8_t* proof, const uint8_t* cbor,
                       const uint64_t* offsets, const uint8_t* rng, int rng_mode, uint8_t* out, uint8_t* status) {
  const bool wire = cbor != nullptr;
  if (!c || !set || !sk || !rng || (n && ((!proof && !cbor) || !out || !status))) return ACT_ERR_ARG;
  if (rng_mode != ACT_RNG_PER_LANE && rng_mode != ACT_RNG_SEQUENTIAL && rng_mode != ACT_RNG_CALLBACK) return ACT_ERR_ARG;
  if (set->device != c->device) { c->err = "act_redeem_batch: the nullifier set lives on another device"; return ACT_ERR_ARG; }
  if (n == 0) return ACT_OK;
  const size_t pb = act_spend_proof_bytes(c), out_b = wire ? act_cbor_size(c, ACT_CBOR_REFUND) : 128;
  // A few items whose rng slices do not depend on the verdicts (per-lane bytes, or one item with its 128 bytes): the refund as ONE call
  // with the signature computed beside the verification (small_impl.inc), THEN the nullifier step, and a lane's refund is handed out
  // only if it verified and its nullifier was fresh -- the same answers as verify -> look-up -> sign (a double spend's signature is
  // dropped unseen), 2.2 ms for one item instead of 3.1.  A signature can then no longer fail behind a recorded nullifier; the test
  // hook for that contract (act_debug_fail_next_signs) keeps the general path.
  if (tiny_refund_applies(c, n, mem, rng_mode) && c->debug_fail_signs.load() == 0) {
    std::vector<uint8_t> rec, st, nul(wire ? n * 32 : 0), sp(n);
    int rc = wire ? refund_cbor_tiny_records(c, n, sk, cbor, offsets, rng, rng_mode, rec, st, nul.data())
                  : (rec.assign(n * 128, 0), st.assign(n, 0), act_refund_batch(c, n, ACT_MEM_HOST, sk, proof, rng, rng_mode, rec.data(), st.data()));
    if (rc != TINY_NEEDS_GENERAL_PATH) {      // (records form: any error of act_refund_batch is the call's error -- no public code means "try the other path")
      if (rc) return rc;
      const int rc_null = act_nullifier_check_and_insert_batch(set, n, ACT_MEM_HOST, wire ? nul.data() : proof, wire ? 32 : pb, st.data(), sp.data());
      if (rc_null == ACT_ERR_HIP) {
        c->err = std::string("nullifier set: ") + act_nullifier_set_last_error(set) + " (every verified lane is undetermined)";
        for (size_t i = 0; i < n; i++) status[i] = st[i] ? st[i] : (uint8_t)ACT_STATUS_NULLIFIER_UNDETERMINED;
        memset(out, 0, n * out_b);
        wipe_host(rec.data(), rec.size());
        return rc_null;
      }
      for (size_t i = 0; i < n; i++) { st[i] = merge_spent(st[i], sp[i]); if (st[i]) memset(rec.data() + 128 * i, 0, 128); }
      if (wire) cbor_frame_refunds_host(cbor_layout(*cbor_type(ACT_CBOR_REFUND), c->L), n, rec.data(), st.data(), out);
      else memcpy(out, rec.data(), n * 128);
      memcpy(status, st.data(), n);
      wipe_host(rec.data(), rec.size());       // (a double spend's refund existed here for a moment: it goes nowhere, not even back to the allocator)
      if (rc_null) c->err = std::string("nullifier set: ") + act_nullifier_set_last_error(set);
      return rc_null;
    }
  }
  // K', verdicts, look-up answers and (wire form) the nullifiers: 32 + 1 + 1 (+ 32) bytes per lane beside the caller's arrays
  const size_t per_lane = 34 + (wire ? 32 : 0);
  std::vector<uint8_t> h; DevTmp d(c);
  uint8_t* base; int rc;
  if (mem == ACT_MEM_DEVICE) { if ((rc = d.alloc(n * per_lane))) return rc; base = d.p; }
  else { h.resize(n * per_lane); base = h.data(); }
  uint8_t *kp = base, *nul = base + n * 32, *st = base + n * (per_lane - 2), *sp = st + n;
  rc = wire ? verify_spend_cbor_impl(c, n, mem, sk, cbor, offsets, st, kp, nul) : act_verify_spend_batch(c, n, mem, sk, proof, st, kp);
  if (rc) return rc;
  return redeem_tail(c, set, n, mem, wire, st, sp, rng, rng_mode, out, status,
                     [&](const uint8_t* mask, uint8_t* spent) {      // records: `k` is the first field of a SpendProof record; wire: the fields the verification call gathered
                       return act_nullifier_check_and_insert_batch(set, n, mem, wire ? nul : proof, wire ? 32 : pb, mask, spent);
                     },
                     [] {},
                     [&](const uint8_t* verdict, const uint8_t* r, int r_mode, uint8_t* o, uint8_t* o_st) {
                       return wire ? act_refund_sign_cbor_batch(c, n, mem, sk, kp, verdict, r, r_mode, o, o_st) : act_refund_sign_batch(c, n, mem, sk, kp, verdict, r, r_mode, o, o_st);
                     });
}

extern "C" int act_redeem_batch(act_ctx* c, act_nullifier_set* set, size_t n, int mem, const uint8_t sk[64], const uint8_t* proof, const uint8_t* rng,
                                int rng_mode, uint8_t* out_refund, uint8_t* status) {
  if (n && !proof) return ACT_ERR_ARG;
  return redeem_impl(c, set, n, mem, sk, proof, nullptr, nullptr, rng, rng_mode, out_refund, status);
}
extern "C" int act_redeem_cbor_batch(act_ctx* c, act_nullifier_set* set, size_t n, int mem, const uint8_t sk[64], const uint8_t* cbor, const uint64_t* offsets,
                                     const uint8_t* rng, int rng_mode, uint8_t* out_refund_cbor, uint8_t* status) {
  if (n && !cbor) return ACT_ERR_ARG;
  static const uint8_t none = 0;           // (n == 0: redeem_impl tells the forms apart by the pointer)
  return redeem_impl(c, set, n, mem, sk, nullptr, cbor ? cbor : &none, offsets, rng, rng_mode, out_refund_cbor, status);
}
// Test hook (tests/test_gpu_redeem.py): the signature step of the next `count` redeem calls on this context fails after the nullifiers
// have been recorded -- the one failure the RECORDED_UNSIGNED contract exists for, which no input can provoke.  Needs the handle;
// nothing in the environment reaches it.
extern "C" int act_debug_fail_next_signs(act_ctx* c, int count) {
  if (!c || count < 0) return ACT_ERR_ARG;
  c->debug_fail_signs.store(count);
  return ACT_OK;
}
