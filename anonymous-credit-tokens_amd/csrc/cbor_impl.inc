// cbor_impl.inc — batch CBOR codec for the nine wire/state types of /root/reference/src/cbor.rs
// (SURVEY.md section 8f "next" #3), included by engine.hip.
//
// Encoding (to_cbor, src/cbor.rs:104-115, 162-175, 236-274, 421-433, 476-486, 522-526, 545-555, 595-608,
// 655-666) is deterministic: a definite-length map with keys 1..n in order, every scalar/point a 32-byte
// byte string (58 20 ..), SpendProof's Com / gamma0 as arrays of L byte strings and z as an array of L
// two-element arrays; PublicKey is a bare byte string.  One GPU lane per 32-byte field frames
// (k_cbor_frame) or unframes (k_cbor_unframe) it: the canonical message is a fixed template with the
// payloads at fixed offsets.  k_cbor_unframe also reduces scalars mod l (decode_scalar =
// from_bytes_mod_order, src/cbor.rs:80-91) and rejects invalid Ristretto encodings (decode_point,
// src/cbor.rs:59-78).
//
// Decoding (from_cbor) must accept what ciborium accepts, not only what to_cbor emits: any well-formed
// CBOR item (RFC 8949) whose top level is a map; integer keys select fields, unknown keys and non-matching
// value shapes are ignored, a later duplicate key overwrites an earlier one, errors surface in map order,
// trailing bytes after the first item are not read.  Messages that are not byte-for-byte canonical take
// the host reader below (cbor_read_message); canonical ones never leave the GPU.  The wire calls that settle such messages after their
// pipeline (ACT_WIRE_READER_HOST: spend, admission, issuance) do it through one window: wire_window.h and wire_window_read below.

#include "cbor_reader.h"      // CborType, cbor_type(), CborReader, cbor_read_message: the host reader, shared with tests/hostcheck
#include "wire_window.h"      // one window of the host reader's road (ACT_WIRE_READER_HOST): gather plan, parse step, lane-patch plan

namespace {

// canonical layout of one message type: template bytes + payload offset and kind of every record field
struct CborLayout { std::vector<uint8_t> tmpl; std::vector<uint32_t> pay_off; std::vector<uint8_t> kind; std::vector<int> entry_first_field; };

void cbor_put_head(std::vector<uint8_t>& v, int major, uint32_t n) {
  if (n < 24) v.push_back((uint8_t)(major << 5 | n));
  else if (n < 256) { v.push_back((uint8_t)(major << 5 | 24)); v.push_back((uint8_t)n); }
  else { v.push_back((uint8_t)(major << 5 | 25)); v.push_back((uint8_t)(n >> 8)); v.push_back((uint8_t)n); }
}
CborLayout cbor_layout(const CborType& T, int L) {
  CborLayout lay;
  auto bstr32 = [&](int kind) { cbor_put_head(lay.tmpl, 2, 32); lay.pay_off.push_back((uint32_t)lay.tmpl.size()); lay.kind.push_back((uint8_t)kind); lay.tmpl.insert(lay.tmpl.end(), 32, 0); };
  if (T.bare) { lay.entry_first_field.push_back(0); bstr32(T.e[0].kind); return lay; }
  cbor_put_head(lay.tmpl, 5, (uint32_t)T.n_entries);
  for (int i = 0; i < T.n_entries; i++) {
    cbor_put_head(lay.tmpl, 0, (uint32_t)T.e[i].key);
    lay.entry_first_field.push_back((int)lay.pay_off.size());
    if (T.e[i].shape == 0) bstr32(T.e[i].kind);
    else if (T.e[i].shape == 1) { cbor_put_head(lay.tmpl, 4, (uint32_t)L); for (int j = 0; j < L; j++) bstr32(T.e[i].kind); }
    else { cbor_put_head(lay.tmpl, 4, (uint32_t)L); for (int j = 0; j < L; j++) { cbor_put_head(lay.tmpl, 4, 2); bstr32(T.e[i].kind); bstr32(T.e[i].kind); } }
  }
  return lay;
}

// ---- GPU framing kernels: lane = (message, record field) -------------------------------------------------
struct CborArgs {
  uint32_t n, n_fields, msg_len;         // msg_len = canonical length
  const uint32_t* pay_off;               // n_fields
  const uint8_t* kind;                   // n_fields: CBOR_S / CBOR_P
  const uint8_t* tmpl;                   // msg_len canonical template
  const uint8_t* in; uint8_t* out;       // encode: records -> cbor ; decode: cbor -> records
  const uint64_t* offsets;               // decode: n+1 message offsets (null = fixed stride msg_len)
  uint8_t* status;                       // decode: per message; also the "is canonical" flag while in flight
};

// A payload is 32 bytes at a byte offset that is whatever the framing in front of it adds up to (a SpendProof's fields start at
// offsets of every residue mod 4).  gfx950 takes byte-aligned dwordx4 accesses to global memory (the compiler emits them for a
// 16-byte memcpy), so a payload moves as two of those, not as 32 byte accesses: 15 M -> see profiles/ for what that gave.
__device__ __forceinline__ void cbor_load32(uint32_t w[8], const uint8_t* p) {
  uint4 a, b;
  __builtin_memcpy(&a, p, 16); __builtin_memcpy(&b, p + 16, 16);
  w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
}
__device__ __forceinline__ void cbor_store32(uint8_t* p, const uint32_t w[8]) {
  const uint4 a = make_uint4(w[0], w[1], w[2], w[3]), b = make_uint4(w[4], w[5], w[6], w[7]);
  __builtin_memcpy(p, &a, 16); __builtin_memcpy(p + 16, &b, 16);
}

__global__ void __launch_bounds__(256) k_cbor_frame(CborArgs a) {
  uint32_t gid = blockIdx.x * 256 + threadIdx.x;
  if (gid >= a.n * a.n_fields) return;
  uint32_t m = gid / a.n_fields, f = gid % a.n_fields;
  uint32_t off = a.pay_off[f], prev_end = f ? a.pay_off[f - 1] + 32 : 0;
  uint8_t* dst = a.out + (size_t)m * a.msg_len;
  for (uint32_t i = prev_end; i < off; i++) dst[i] = a.tmpl[i];               // the framing bytes in front of this payload
  uint32_t w[8];
  cbor_load32(w, a.in + ((size_t)m * a.n_fields + f) * 32);
  cbor_store32(dst + off, w);
}
// status codes written: 0 canonical and valid, CBOR_ERR_VALUE invalid point, 0x80 = not canonical (host reader needed)
__global__ void __launch_bounds__(256) k_cbor_unframe(CborArgs a) {
  uint32_t gid = blockIdx.x * 256 + threadIdx.x;
  if (gid >= a.n * a.n_fields) return;
  uint32_t m = gid / a.n_fields, f = gid % a.n_fields;
  uint64_t beg = a.offsets ? a.offsets[m] : (uint64_t)m * a.msg_len, end = a.offsets ? a.offsets[m + 1] : beg + a.msg_len;
  // ciborium reads one item and ignores trailing bytes: a canonical prefix is enough
  if (end - beg < a.msg_len) { atomicOr(reinterpret_cast<unsigned int*>(a.status + (m & ~3u)), 0x80u << (8 * (m & 3u))); return; }
  const uint8_t* src = a.in + beg;
  uint32_t off = a.pay_off[f], prev_end = f ? a.pay_off[f - 1] + 32 : 0;
  bool canon = true;
  for (uint32_t i = prev_end; i < off; i++) canon = canon && (src[i] == a.tmpl[i]);
  if (!canon) { atomicOr(reinterpret_cast<unsigned int*>(a.status + (m & ~3u)), 0x80u << (8 * (m & 3u))); return; }
  uint32_t w[8];
  cbor_load32(w, src + off);
  if (a.kind[f] == CBOR_S) { sc s = sc_from_words(w); for (int i = 0; i < 8; i++) w[i] = s.v[i]; }      // from_bytes_mod_order
  else { ge p; if (!ristretto_decode(p, w)) atomicOr(reinterpret_cast<unsigned int*>(a.status + (m & ~3u)), (unsigned)CBOR_ERR_VALUE << (8 * (m & 3u))); }
  cbor_store32(a.out + ((size_t)m * a.n_fields + f) * 32, w);
}
// second pass for messages that went through the host reader: reduce scalars / validate points of given records
__global__ void __launch_bounds__(256) k_cbor_fix_records(uint32_t n, uint32_t n_fields, const uint8_t* kind, const uint32_t* which, uint8_t* records, uint8_t* status) {
  uint32_t gid = blockIdx.x * 256 + threadIdx.x;
  if (gid >= n * n_fields) return;
  uint32_t m = which[gid / n_fields], f = gid % n_fields;
  uint8_t* rec = records + ((size_t)m * n_fields + f) * 32;
  uint32_t w[8];
  for (int i = 0; i < 8; i++) w[i] = (uint32_t)rec[4 * i] | (uint32_t)rec[4 * i + 1] << 8 | (uint32_t)rec[4 * i + 2] << 16 | (uint32_t)rec[4 * i + 3] << 24;
  if (kind[f] == CBOR_S) {
    sc s = sc_from_words(w);
    for (int i = 0; i < 8; i++) { rec[4 * i] = (uint8_t)s.v[i]; rec[4 * i + 1] = (uint8_t)(s.v[i] >> 8); rec[4 * i + 2] = (uint8_t)(s.v[i] >> 16); rec[4 * i + 3] = (uint8_t)(s.v[i] >> 24); }
  } else { ge p; if (!ristretto_decode(p, w)) atomicOr(reinterpret_cast<unsigned int*>(status + (m & ~3u)), (unsigned)CBOR_ERR_VALUE << (8 * (m & 3u))); }
}

// loose point values (the reader's CborCand::pts of several messages back to back): bad[i] = 1 when value i is not a canonical
// Ristretto encoding (decode_point's InvalidValue, src/cbor.rs:62-77)
__global__ void __launch_bounds__(256) k_cbor_check_points(uint32_t n, const uint8_t* pts, uint8_t* bad) {
  uint32_t gid = blockIdx.x * 256 + threadIdx.x;
  if (gid >= n) return;
  uint32_t w[8];
  cbor_load32(w, pts + (size_t)gid * 32);
  ge p;
  bad[gid] = ristretto_decode(p, w) ? 0 : 1;
}

// Unframing for the fused wire-to-verdict path (act_verify_spend_cbor_batch): the canonical check and the payload copy of
// k_cbor_unframe WITHOUT scalar reduction and point validation -- the verification kernels reduce every scalar they load and decode
// every point anyway (an undecodable one becomes status 255 there), so a point is decoded once, not once here and once there.
// flags[first + m] |= 0x80 for a message that is not byte-for-byte canonical (its record is zero-filled: it is re-read on the host).
__global__ void __launch_bounds__(256) k_cbor_unframe_raw(CborArgs a, uint32_t first) {
  uint32_t gid = blockIdx.x * 256 + threadIdx.x;
  if (gid >= a.n * a.n_fields) return;
  uint32_t m = gid / a.n_fields, f = gid % a.n_fields;
  uint64_t beg = a.offsets ? a.offsets[m] : (uint64_t)m * a.msg_len, end = a.offsets ? a.offsets[m + 1] : beg + a.msg_len;
  const uint32_t gm = first + m;
  uint4* dst = reinterpret_cast<uint4*>(a.out + ((size_t)m * a.n_fields + f) * 32);
  bool canon = end - beg >= a.msg_len;                        // ciborium reads one item and ignores trailing bytes: a canonical prefix is enough
  const uint8_t* src = a.in + beg;
  uint32_t off = a.pay_off[f], prev_end = f ? a.pay_off[f - 1] + 32 : 0;
  if (canon) for (uint32_t i = prev_end; i < off; i++) canon = canon && (src[i] == a.tmpl[i]);
  if (!canon) {
    atomicOr(reinterpret_cast<unsigned int*>(a.status + (gm & ~3u)), 0x80u << (8 * (gm & 3u)));
    dst[0] = make_uint4(0, 0, 0, 0); dst[1] = make_uint4(0, 0, 0, 0);
    return;
  }
  uint32_t w[8];
  cbor_load32(w, src + off);
  dst[0] = make_uint4(w[0], w[1], w[2], w[3]); dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

struct CborDev { uint32_t* pay_off = nullptr; uint8_t* kind = nullptr; uint8_t* tmpl = nullptr; CborLayout lay; };
int cbor_dev_prepare(act_ctx* c, Slot& sl, int type, CborDev* d) {
  const CborType* T = cbor_type(type);
  d->lay = cbor_layout(*T, c->L);
  size_t nf = d->lay.pay_off.size(), tl = d->lay.tmpl.size();
  // a staging area of its own: set_key / set_pubkey decode keys through area 5 while a wire-bytes call holds this layout
  int rc = stage_reserve(c, sl, 8, nf * 5 + tl + 64); if (rc) return rc;
  uint8_t* base = sl.d_stage[8];
  d->pay_off = reinterpret_cast<uint32_t*>(base); d->kind = base + nf * 4; d->tmpl = d->kind + nf;
  HIPCK(c, hipMemcpyAsync(d->pay_off, d->lay.pay_off.data(), nf * 4, hipMemcpyHostToDevice, sl.stream));
  HIPCK(c, hipMemcpyAsync(d->kind, d->lay.kind.data(), nf, hipMemcpyHostToDevice, sl.stream));
  HIPCK(c, hipMemcpyAsync(d->tmpl, d->lay.tmpl.data(), tl, hipMemcpyHostToDevice, sl.stream));
  HIPCK(c, hipStreamSynchronize(sl.stream));   // the layout vectors are about to be reused by the caller
  return ACT_OK;
}

// The codes of messages that went through the host reader, as from_cbor orders them.  codes[k] = the reader's result for message k,
// cands[k] = its point values.  A message whose reader stopped at a structural fault with points in front of it, or whose points
// are not all in its record (duplicate keys, over-long arrays), has those points validated here -- rare, adversarial spellings; one
// small kernel per call -- and reports CBOR_ERR_VALUE when one of them is invalid: that decode_point ran, and returned, first.
// (Public data: plain device allocations, freed before returning.)
int cbor_settle_codes(act_ctx* c, hipStream_t stream, std::vector<int>& codes, const std::vector<CborCand>& cands) {
  std::vector<uint8_t> pts; std::vector<uint32_t> owner;
  for (size_t k = 0; k < codes.size(); k++) {
    const bool need = (codes[k] == CBOR_ERR_STRUCTURE && !cands[k].pts.empty()) || (codes[k] == CBOR_OK && cands[k].irregular);
    if (!need) continue;
    pts.insert(pts.end(), cands[k].pts.begin(), cands[k].pts.end());
    owner.insert(owner.end(), cands[k].pts.size() / 32, (uint32_t)k);
  }
  if (owner.empty()) return ACT_OK;
  if (owner.size() >= ((size_t)1 << 32)) return ACT_ERR_ARG;
  uint8_t *d_pts = nullptr, *d_bad = nullptr;
  std::vector<uint8_t> bad(owner.size());
  hipError_t he = hipMalloc(&d_pts, pts.size());
  if (he == hipSuccess) he = hipMalloc(&d_bad, owner.size());
  if (he == hipSuccess) he = hipMemcpyAsync(d_pts, pts.data(), pts.size(), hipMemcpyHostToDevice, stream);
  if (he == hipSuccess) {
    hipLaunchKernelGGL(k_cbor_check_points, dim3((unsigned)((owner.size() + 255) / 256)), dim3(256), 0, stream, (uint32_t)owner.size(), d_pts, d_bad);
    he = hipMemcpyAsync(bad.data(), d_bad, owner.size(), hipMemcpyDeviceToHost, stream);
  }
  if (he == hipSuccess) he = hipStreamSynchronize(stream);
  if (d_pts) (void)hipFree(d_pts);
  if (d_bad) (void)hipFree(d_bad);
  HIPCK(c, he);
  for (size_t i = 0; i < owner.size(); i++) if (bad[i]) codes[owner[i]] = CBOR_ERR_VALUE;
  return ACT_OK;
}

// One window of the host reader's road, for its three settles (verify_spend_cbor_impl below, issue_wire_settle, the admission
// screen): the flagged messages which[0..cnt) are brought to the host (device-memory callers; wire_window.h has the rule), read by
// cbor_read_message, and their codes ordered as from_cbor orders them (cbor_settle_codes).  It leaves codes[k], status[k] -- the
// lane status of a message that is refused, 0 for one that reads -- and the raw record recs[k * rb ...] of every message that READ,
// all zero otherwise; a record can have read and still be refused (CBOR_ERR_VALUE from a point that never reaches it).
// Nothing here or in wire_patch_lanes takes the context's lock: the spend settle runs inside its call, which holds it (the admission
// screen is serialised by the context's admission lock); issue_wire_settle runs between calls and takes it around each of the two
// (issue_wire_impl.inc).
struct WireWindow { WireGather g; std::vector<uint8_t> bytes, recs, status; std::vector<int> codes; std::vector<CborCand> cands; };
int wire_window_read(act_ctx* c, hipStream_t stream, const CborType& T, const WireExtent& x, bool dev, const size_t* which, size_t cnt, size_t rb, WireWindow& w) {
  if (dev) {
    wire_gather_plan(x, which, cnt, w.g);
    w.bytes.resize(w.g.bytes);
    const int rc = wire_gather_run(w.g, w.bytes.data(), [&](uint8_t* dst, size_t src, size_t len) -> int { HIPCK(c, hipMemcpy(dst, x.cbor + src, len, hipMemcpyDeviceToHost)); return ACT_OK; });
    if (rc) return rc;
  }
  wire_window_parse(T, c->L, x, which, cnt, dev ? w.bytes.data() : nullptr, w.g.at, rb, w.recs, w.codes, w.cands);
  // the first error in wire order, as from_cbor reports it: an invalid point in front of a structural fault, or in a value that a
  // duplicate key or an over-long array keeps out of the record, is InvalidValue (status 255)
  if (const int rc = cbor_settle_codes(c, stream, w.codes, w.cands)) return rc;
  w.status.resize(cnt);
  for (size_t k = 0; k < cnt; k++) w.status[k] = act::cbor_code_status((uint8_t)w.codes[k]);
  return ACT_OK;
}
// lanes[0..cnt) of a caller's array (host or device memory; null: nothing to do) take vals[k * stride ...]
int wire_patch_lanes(act_ctx* c, int mem, uint8_t* base, size_t stride, const size_t* lanes, size_t cnt, const uint8_t* vals, bool span_only = false) {
  if (!base) return ACT_OK;
  if (mem == ACT_MEM_HOST) { for (size_t k = 0; k < cnt; k++) memcpy(base + lanes[k] * stride, vals + k * stride, stride); return ACT_OK; }
  return wire_patch_run(lanes, cnt, stride, vals,
    [&](uint8_t* dst, size_t off, size_t len) -> int { HIPCK(c, hipMemcpy(dst, base + off, len, hipMemcpyDeviceToHost)); return ACT_OK; },
    [&](size_t off, const uint8_t* src, size_t len) -> int { HIPCK(c, hipMemcpy(base + off, src, len, hipMemcpyHostToDevice)); return ACT_OK; }, span_only);
}

// one flag byte per message of a wire-bytes call, accumulated with 32-bit atomics, zero when this returns (slot 0's stream has drained:
// the other slot's stream reads the flags, and the layout, too)
int wire_flags_reserve(act_ctx* c, size_t n) {
  const size_t fcap = (n + 3) & ~(size_t)3;
  if (fcap > c->d_wire_flags_cap) {
    if (c->d_wire_flags) HIPCK(c, hipFree(c->d_wire_flags));
    c->d_wire_flags = nullptr; c->d_wire_flags_cap = 0;
    HIPCK(c, hipMalloc(&c->d_wire_flags, fcap)); c->d_wire_flags_cap = fcap;
  }
  HIPCK(c, hipMemsetAsync(c->d_wire_flags, 0, fcap, c->slots[0].stream));
  HIPCK(c, hipStreamSynchronize(c->slots[0].stream));
  return ACT_OK;
}
// the device reader's code and info bytes, one each per message of the call, zero (CBOR_OK) until a reader kernel writes them (the
// memset is on slot 0's stream: wire_flags_reserve, called next, waits for it)
int wire_codes_reserve(act_ctx* c, size_t n) {
  const size_t fcap = (n + 3) & ~(size_t)3;
  if (fcap > c->d_wire_codes_cap) {
    if (c->d_wire_codes) HIPCK(c, hipFree(c->d_wire_codes));
    c->d_wire_codes = nullptr; c->d_wire_codes_cap = 0;
    HIPCK(c, hipMalloc(&c->d_wire_codes, 2 * fcap)); c->d_wire_codes_cap = fcap;
  }
  HIPCK(c, hipMemsetAsync(c->d_wire_codes, 0, 2 * c->d_wire_codes_cap, c->slots[0].stream));
  return ACT_OK;
}

}  // namespace

extern "C" {

size_t act_cbor_size(const act_ctx* c, int type) {
  const CborType* T = cbor_type(type);
  return (c && T) ? cbor_layout(*T, c->L).tmpl.size() : 0;
}
size_t act_cbor_record_bytes(const act_ctx* c, int type) {
  const CborType* T = cbor_type(type);
  return (c && T) ? 32 * cbor_layout(*T, c->L).pay_off.size() : 0;
}

// Host-memory callers: a chunk's bytes cross PCIe twice (in, out) around a kernel that is short next to either copy, so the chunks
// alternate between the context's two slots (own stream, own staging areas each): chunk k's copy in runs while chunk k-1's copy
// out is still on the other link direction.  Left to themselves the two streams fall into step (both copy in, then both copy out,
// each pair sharing one direction), so the copies of one direction are chained: chunk k's copy in waits for chunk k-1's, its copy
// out for chunk k-1's (events across the two streams).  Device-memory callers: one stream, large chunks, no copies.
constexpr size_t CBOR_HOST_CHUNK_BYTES = (size_t)128 << 20;
// messages per chunk; the cbor_chunk_msgs knob (act_tuning_set, read per call) lets the tests cut small batches into many chunks
static size_t cbor_chunk_msgs(int mem, size_t nf, size_t ml) {
  { const long v = tune(T_CBOR_CHUNK_MSGS); if (v > 0) return (size_t)v; }
  size_t chunk = std::max<size_t>(1, ((size_t)1 << 24) / nf);
  if (mem == ACT_MEM_HOST) chunk = std::max<size_t>(1, std::min(chunk, CBOR_HOST_CHUNK_BYTES / ml));
  return chunk;
}

int act_cbor_encode_batch(act_ctx* c, int type, size_t n, int mem, const uint8_t* records, uint8_t* out_cbor) {
  const CborType* T = cbor_type(type);
  if (!c || !T || (n && (!records || !out_cbor))) return ACT_ERR_ARG;
  Call call(c, 0);          // serialises the context's callers; wipes the staging copies (PrivateKey, CreditToken ... records) on every exit
  HIPCK(c, hipSetDevice(c->device));
  CborDev d; int rc = cbor_dev_prepare(c, c->slots[0], type, &d); if (rc) return rc;
  const size_t nf = d.lay.pay_off.size(), ml = d.lay.tmpl.size();
  const size_t chunk = cbor_chunk_msgs(mem, nf, ml);
  size_t k = 0;
  for (size_t off = 0; off < n; off += chunk, k++) {
    Slot& sl = c->slots[mem == ACT_MEM_HOST ? (k & 1) : 0];
    HIPCK(c, hipStreamSynchronize(sl.stream));               // the chunk before last has left this slot's staging areas
    uint32_t m = (uint32_t)std::min(chunk, n - off);
    CborArgs a{}; a.n = m; a.n_fields = (uint32_t)nf; a.msg_len = (uint32_t)ml; a.pay_off = d.pay_off; a.kind = d.kind; a.tmpl = d.tmpl;
    const bool host = mem == ACT_MEM_HOST;
    if (host && (rc = copy_chain_wait(c, sl, false))) return rc;
    if ((rc = dev_in(c, sl, 0, mem, records + off * nf * 32, (size_t)m * nf * 32, &a.in))) return rc;
    if (host && (rc = copy_chain_record(c, sl, false))) return rc;
    if ((rc = dev_out_begin(c, sl, 2, mem, out_cbor + off * ml, (size_t)m * ml, &a.out))) return rc;
    hipLaunchKernelGGL(k_cbor_frame, dim3((unsigned)(((size_t)m * nf + 255) / 256)), dim3(256), 0, sl.stream, a);
    if (host && (rc = copy_chain_wait(c, sl, true))) return rc;
    if ((rc = dev_out_end(c, sl, mem, out_cbor + off * ml, a.out, (size_t)m * ml))) return rc;
    if (host && (rc = copy_chain_record(c, sl, true))) return rc;
  }
  return call.finish();                                      // waits for both streams
}

namespace {
// one chunk of a decode call between its two halves: submitted (copy in, unframe, statuses on their way back) ... completed
// (host reader for what was not canonical, failed records zeroed, records and statuses on their way out)
struct CborDecChunk {
  Slot* sl = nullptr; size_t off = 0, m = 0, byte_beg = 0, byte_end = 0;
  const uint8_t* d_in = nullptr; uint8_t* d_out = nullptr; uint8_t* d_status = nullptr;
  std::vector<uint64_t> rel; uint8_t* st = nullptr;       // st: the slot's pinned status buffer (the copy back must not block the host)
};
}  // namespace

int act_cbor_decode_batch(act_ctx* c, int type, size_t n, int mem, const uint8_t* cbor, const uint64_t* offsets, uint8_t* out_records,
                          uint8_t* status) {
  const CborType* T = cbor_type(type);
  if (!c || !T || (n && (!cbor || !out_records || !status))) return ACT_ERR_ARG;
  if (offsets) for (size_t i = 0; i < n; i++) if (offsets[i + 1] < offsets[i]) return ACT_ERR_ARG;     // message i = [offsets[i], offsets[i+1])
  CborDecChunk chunks[2];   // declared before `call`: on an early return its destructor waits for the streams while the copies' host buffers still exist
  Call call(c, 0);          // serialises the context's callers; wipes the staging copies (PrivateKey, CreditToken ... records) on every exit
  HIPCK(c, hipSetDevice(c->device));
  CborDev d; int rc = cbor_dev_prepare(c, c->slots[0], type, &d); if (rc) return rc;
  const size_t nf = d.lay.pay_off.size(), ml = d.lay.tmpl.size(), rb = nf * 32;
  const size_t chunk = cbor_chunk_msgs(mem, nf, ml);

  auto submit = [&](CborDecChunk& ch, Slot& sl, size_t off) -> int {
    HIPCK(c, hipStreamSynchronize(sl.stream));               // the chunk before last has left this slot's staging areas
    ch.sl = &sl; ch.off = off; ch.m = std::min(chunk, n - off);
    const size_t m = ch.m;
    ch.byte_beg = offsets ? (size_t)offsets[off] : off * ml; ch.byte_end = offsets ? (size_t)offsets[off + m] : (off + m) * ml;
    uint64_t* d_offsets = nullptr;
    int rc2;
    if (mem == ACT_MEM_HOST && (rc2 = copy_chain_wait(c, sl, false))) return rc2;
    if ((rc2 = dev_in(c, sl, 0, mem, cbor + ch.byte_beg, ch.byte_end - ch.byte_beg, &ch.d_in))) return rc2;
    if (mem == ACT_MEM_HOST && (rc2 = copy_chain_record(c, sl, false))) return rc2;
    if ((rc2 = dev_out_begin(c, sl, 2, mem, out_records + off * rb, m * rb, &ch.d_out))) return rc2;
    // statuses are accumulated with 32-bit atomics: always in an internal, 4-byte-padded buffer
    if ((rc2 = stage_reserve(c, sl, 4, (m + 3) & ~(size_t)3))) return rc2;
    ch.d_status = sl.d_stage[4];
    HIPCK(c, hipMemsetAsync(ch.d_status, 0, (m + 3) & ~(size_t)3, sl.stream));
    ch.rel.clear();
    if (offsets) {
      ch.rel.resize(m + 1);
      for (size_t i = 0; i <= m; i++) ch.rel[i] = offsets[off + i] - ch.byte_beg;
      if ((rc2 = stage_reserve(c, sl, 1, (m + 1) * 8))) return rc2;
      d_offsets = reinterpret_cast<uint64_t*>(sl.d_stage[1]);
      HIPCK(c, hipMemcpyAsync(d_offsets, ch.rel.data(), (m + 1) * 8, hipMemcpyHostToDevice, sl.stream));
    }
    CborArgs a{}; a.n = (uint32_t)m; a.n_fields = (uint32_t)nf; a.msg_len = (uint32_t)ml; a.pay_off = d.pay_off; a.kind = d.kind; a.tmpl = d.tmpl;
    a.in = ch.d_in; a.out = ch.d_out; a.offsets = d_offsets; a.status = ch.d_status;
    hipLaunchKernelGGL(k_cbor_unframe, dim3((unsigned)((m * nf + 255) / 256)), dim3(256), 0, sl.stream, a);
    if (m > sl.h_cst_cap) {
      if (sl.h_cst) HIPCK(c, hipHostFree(sl.h_cst));
      sl.h_cst = nullptr; sl.h_cst_cap = 0;
      HIPCK(c, hipHostMalloc(&sl.h_cst, m, hipHostMallocDefault)); sl.h_cst_cap = m;
    }
    ch.st = sl.h_cst;
    HIPCK(c, hipMemcpyAsync(ch.st, ch.d_status, m, hipMemcpyDeviceToHost, sl.stream));
    return ACT_OK;
  };
  auto complete = [&](CborDecChunk& ch) -> int {
    Slot& sl = *ch.sl; const size_t m = ch.m, off = ch.off;
    uint8_t* st = ch.st;
    HIPCK(c, hipStreamSynchronize(sl.stream));
    // non-canonical messages: general reader on the host, then the same scalar-reduction / point-validation pass on the GPU
    std::vector<uint32_t> which;
    for (size_t i = 0; i < m; i++) if (st[i] & 0x80) which.push_back((uint32_t)i);
    if (!which.empty()) {
      std::vector<uint8_t> host_msgs;
      const uint8_t* hsrc = cbor + ch.byte_beg;
      if (mem == ACT_MEM_DEVICE) { host_msgs.resize(ch.byte_end - ch.byte_beg); HIPCK(c, hipMemcpy(host_msgs.data(), cbor + ch.byte_beg, ch.byte_end - ch.byte_beg, hipMemcpyDeviceToHost)); hsrc = host_msgs.data(); }
      std::vector<uint8_t> recs(which.size() * rb, 0);
      std::vector<uint32_t> good;
      std::vector<int> codes(which.size()); std::vector<CborCand> cands(which.size());
      for (size_t k = 0; k < which.size(); k++) {
        uint32_t i = which[k];
        size_t beg = offsets ? (size_t)ch.rel[i] : (size_t)i * ml, end = offsets ? (size_t)ch.rel[i + 1] : beg + ml;
        codes[k] = cbor_read_message(*T, c->L, hsrc + beg, end - beg, recs.data() + k * rb, &cands[k]);
      }
      { int rc3 = cbor_settle_codes(c, sl.stream, codes, cands); if (rc3) return rc3; }     // the first error in wire order, as from_cbor reports it
      for (size_t k = 0; k < which.size(); k++) {
        uint32_t i = which[k];
        st[i] = (uint8_t)codes[k];
        if (codes[k] == CBOR_OK) good.push_back(i); else memset(recs.data() + k * rb, 0, rb);
      }
      for (size_t k = 0; k < which.size(); k++)
        HIPCK(c, hipMemcpyAsync(ch.d_out + (size_t)which[k] * rb, recs.data() + k * rb, rb, hipMemcpyHostToDevice, sl.stream));
      HIPCK(c, hipMemcpyAsync(ch.d_status, st, m, hipMemcpyHostToDevice, sl.stream));
      if (!good.empty()) {
        int rc2 = stage_reserve(c, sl, 3, good.size() * 4); if (rc2) return rc2;
        HIPCK(c, hipMemcpyAsync(sl.d_stage[3], good.data(), good.size() * 4, hipMemcpyHostToDevice, sl.stream));
        hipLaunchKernelGGL(k_cbor_fix_records, dim3((unsigned)((good.size() * nf + 255) / 256)), dim3(256), 0, sl.stream, (uint32_t)good.size(),
                           (uint32_t)nf, d.kind, reinterpret_cast<const uint32_t*>(sl.d_stage[3]), ch.d_out, ch.d_status);
      }
      HIPCK(c, hipMemcpyAsync(st, ch.d_status, m, hipMemcpyDeviceToHost, sl.stream));
      HIPCK(c, hipStreamSynchronize(sl.stream));              // recs / good / st are read by the copies above
    }
    // the record of a failed message is all zero, like every failed lane of this ABI
    for (size_t i = 0; i < m; i++) if (st[i]) HIPCK(c, hipMemsetAsync(ch.d_out + i * rb, 0, rb, sl.stream));
    int rc2;
    if (mem == ACT_MEM_HOST && (rc2 = copy_chain_wait(c, sl, true))) return rc2;
    if ((rc2 = dev_out_end(c, sl, mem, out_records + off * rb, ch.d_out, m * rb))) return rc2;
    if (mem == ACT_MEM_HOST && (rc2 = copy_chain_record(c, sl, true))) return rc2;
    HIPCK(c, hipMemcpyAsync(status + off, ch.d_status, m, mem == ACT_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, sl.stream));
    return ACT_OK;
  };

  size_t k = 0;
  for (size_t off = 0; off < n; off += chunk, k++) {
    const size_t s = mem == ACT_MEM_HOST ? (k & 1) : 0;
    // host memory: this chunk's copy in and kernel are queued first (nothing in `submit` waits for them), then the chunk before is
    // completed on the other slot's stream -- statuses read, what was not canonical settled, its copy out started beside them.
    // (Queued the other way round the two copies ran one after the other: docs/history/profiles/r04_codec_trace.txt.)
    if (mem != ACT_MEM_HOST && k) { if ((rc = complete(chunks[0]))) return rc; }       // one slot: finish the chunk before starting the next
    if ((rc = submit(chunks[s], c->slots[s], off))) return rc;
    if (mem == ACT_MEM_HOST && k) { if ((rc = complete(chunks[s ^ 1]))) return rc; }
  }
  if (k) { if ((rc = complete(chunks[mem == ACT_MEM_HOST ? ((k - 1) & 1) : 0]))) return rc; }
  return call.finish();                                      // waits for both streams
}

// act_cbor_decode_batch's contract with every message going through the device reader: no canonical short cut, no host reader.
// Per chunk, on the chunk's stream: the plain pass into the caller's records, the validating pass over the messages it names, then
// per (message, field) the scalar reduction / point validation that k_cbor_unframe does, and zeros over what failed.  Nothing here
// waits for the host, so the chunks of a host-memory caller alternate between the two slots like those of act_cbor_encode_batch.
int act_cbor_read_batch(act_ctx* c, int type, size_t n, int mem, const uint8_t* cbor, const uint64_t* offsets, uint8_t* out_records,
                        uint8_t* status) {
  const CborType* T = cbor_type(type);
  if (!c || !T || (n && (!cbor || !out_records || !status))) return ACT_ERR_ARG;
  if (offsets) for (size_t i = 0; i < n; i++) if (offsets[i + 1] < offsets[i]) return ACT_ERR_ARG;     // message i = [offsets[i], offsets[i+1])
  std::vector<uint64_t> rel[2];   // declared before `call`: on an early return its destructor waits for the streams while the copies' host buffers still exist
  Call call(c, 0);
  HIPCK(c, hipSetDevice(c->device));
  CborDev d; int rc = cbor_dev_prepare(c, c->slots[0], type, &d); if (rc) return rc;
  const size_t nf = d.lay.pay_off.size(), ml = d.lay.tmpl.size(), rb = nf * 32;
  const size_t chunk = std::min(cbor_chunk_msgs(mem, nf, ml), (size_t)1 << 30);
  const bool host = mem == ACT_MEM_HOST;
  size_t k = 0;
  for (size_t off = 0; off < n; off += chunk, k++) {
    Slot& sl = c->slots[host ? (k & 1) : 0];
    HIPCK(c, hipStreamSynchronize(sl.stream));               // the chunk before last has left this slot's staging areas
    const size_t m = std::min(chunk, n - off), pad = (m + 3) & ~(size_t)3;
    const size_t byte_beg = offsets ? (size_t)offsets[off] : off * ml, byte_end = offsets ? (size_t)offsets[off + m] : (off + m) * ml;
    CborReadArgs ra{};
    ra.T = *T; ra.L = c->L; ra.n = (uint32_t)m; ra.first = 0; ra.msg_len = (uint32_t)ml; ra.rec_stride = rb; ra.keep_fields = (uint32_t)nf;
    if (host && (rc = copy_chain_wait(c, sl, false))) return rc;
    if ((rc = dev_in(c, sl, 0, mem, cbor + byte_beg, byte_end - byte_beg, &ra.in))) return rc;
    if (offsets) {
      std::vector<uint64_t>& r = rel[host ? (k & 1) : 0];
      r.resize(m + 1);
      for (size_t i = 0; i <= m; i++) r[i] = offsets[off + i] - byte_beg;
      if ((rc = stage_reserve(c, sl, 1, (m + 1) * 8))) return rc;
      HIPCK(c, hipMemcpyAsync(sl.d_stage[1], r.data(), (m + 1) * 8, hipMemcpyHostToDevice, sl.stream));
      ra.offsets = reinterpret_cast<const uint64_t*>(sl.d_stage[1]);
    }
    if (host && (rc = copy_chain_record(c, sl, false))) return rc;
    if ((rc = dev_out_begin(c, sl, 2, mem, out_records + off * rb, m * rb, &ra.rec))) return rc;
    if ((rc = stage_reserve(c, sl, 4, 2 * pad))) return rc;      // codes (padded: 32-bit OR in the field pass), then infos
    ra.code = sl.d_stage[4]; ra.info = sl.d_stage[4] + pad;
    HIPCK(c, hipMemsetAsync(sl.d_stage[4], 0, 2 * pad, sl.stream));
    launch_cbor_read(ra, false, sl.stream);
    launch_cbor_read(ra, true, sl.stream);
    CborFixArgs fa{(uint32_t)m, (uint32_t)nf, d.kind, ra.rec, ra.code};
    launch_cbor_fix(fa, sl.stream);
    HIPCK(c, hipGetLastError());
    if (host && (rc = copy_chain_wait(c, sl, true))) return rc;
    if ((rc = dev_out_end(c, sl, mem, out_records + off * rb, ra.rec, m * rb))) return rc;
    if (host && (rc = copy_chain_record(c, sl, true))) return rc;
    HIPCK(c, hipMemcpyAsync(status + off, ra.code, m, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, sl.stream));
  }
  return call.finish();                                      // waits for both streams
}

int act_ctx_set_wire_reader(act_ctx* c, int where) {
  if (!c || (where != ACT_WIRE_READER_HOST && where != ACT_WIRE_READER_DEVICE)) return ACT_ERR_ARG;
  c->wire_reader.store(where);
  return ACT_OK;
}
// (here and not in node.cpp: it needs nothing of the node but its contexts, and the reader is this file's)
int act_node_set_wire_reader(act_node* nd, int reader) {
  if (!nd) return ACT_ERR_ARG;
  for (int k = 0; k < act_node_device_count(nd); k++) { const int rc = act_ctx_set_wire_reader(act_node_ctx(nd, k), reader); if (rc) return rc; }
  return ACT_OK;
}
int act_ctx_wire_stats(act_ctx* c, uint64_t out[4], int reset) {
  if (!c || !out) return ACT_ERR_ARG;
  for (int i = 0; i < 4; i++) out[i] = reset ? c->wire_stats[i].exchange(0) : c->wire_stats[i].load();
  return ACT_OK;
}


// ---- wire bytes in, verdict out -----------------------------------------------------------------------------------------
// SpendProof::from_cbor (src/cbor.rs:236-408) followed by PrivateKey::refund up to the challenge check (src/lib.rs:787-844) as ONE
// pass: every chunk's messages are unframed into raw records on the chunk's own stream in front of its verification kernels, and
// each of the 130 points of a proof is decoded exactly once (by the kernel that needs it).  Messages that are not the canonical
// encoding are flagged by the unframing kernel, verified as all-zero records for the moment, and settled after the pipeline has
// drained: the general reader on the host (cbor_read_message), then a second, small verification call for those that parse.
// That is the road of ACT_WIRE_READER_HOST.  Under ACT_WIRE_READER_DEVICE (the default) the flagged messages are read by
// k_cbor_read_raw between the unframing kernel and the verification kernels of their own chunk: every spelling is verified once,
// in the pipeline, and what is left for the end of the call is to give the messages the reader refused their wire status.
static int wire_unframe_chunk(act_ctx* c, Slot& sl, const WireSrc& w, int mem, size_t off, uint32_t m, const uint8_t** d_records) {
  const ProofLayout pl{c->L};
  const size_t nf = pl.bytes() / 32;
  const size_t byte_beg = w.offsets ? (size_t)w.offsets[off] : off * w.msg_len, byte_end = w.offsets ? (size_t)w.offsets[off + m] : (off + m) * w.msg_len;
  const uint8_t* d_in; int rc;
  // (wire bytes are always staged, pinned or not: the unframing kernel's 32-byte moves at 35-byte strides make poor reads over the
  // link -- measured 456 k messages/s reading pinned memory in place against 486 k staged, docs/history/profiles/r05_k_bench.json / r05_i -- unlike
  // the record kernels' 2 KiB-contiguous loads, which do read pinned memory in place: engine.hip mapped_view)
  if ((rc = dev_in(c, sl, 0, mem, w.cbor + byte_beg, byte_end - byte_beg, &d_in))) return rc;
  uint64_t* d_offsets = nullptr;
  if (w.offsets) {
    sl.h_rel.resize((size_t)m + 1);                          // lives in the slot: the copy below is asynchronous
    for (size_t i = 0; i <= m; i++) sl.h_rel[i] = w.offsets[off + i] - byte_beg;
    if ((rc = stage_reserve(c, sl, 7, ((size_t)m + 1) * 8))) return rc;
    d_offsets = reinterpret_cast<uint64_t*>(sl.d_stage[7]);
    HIPCK(c, hipMemcpyAsync(d_offsets, sl.h_rel.data(), ((size_t)m + 1) * 8, hipMemcpyHostToDevice, sl.stream));
  }
  if ((rc = stage_reserve(c, sl, 6, (size_t)m * pl.bytes()))) return rc;
  sl.d_stage_dirty[6] = std::max(sl.d_stage_dirty[6], (size_t)m * pl.bytes());
  CborDev& d = *reinterpret_cast<CborDev*>(c->wire_layout);
  CborArgs a{}; a.n = m; a.n_fields = (uint32_t)nf; a.msg_len = (uint32_t)w.msg_len; a.pay_off = d.pay_off; a.kind = d.kind; a.tmpl = d.tmpl;
  a.in = d_in; a.out = sl.d_stage[6]; a.offsets = d_offsets; a.status = c->d_wire_flags;
  hipLaunchKernelGGL(k_cbor_unframe_raw, dim3((unsigned)(((size_t)m * nf + 255) / 256)), dim3(256), 0, sl.stream, a, (uint32_t)off);
  // the device reader: every flagged message of the chunk is read from the staged bytes into the record the unframing kernel would
  // have filled, on the same stream and without a word to the host -- first the plain pass, then the validating pass over the
  // messages the plain pass names (cbor_lanes.h); a lane of either returns at once unless its message is flagged
  if (c->wire_read_code) {
    CborReadArgs ra{};
    ra.T = *cbor_type(ACT_CBOR_SPEND_PROOF); ra.L = c->L; ra.n = m; ra.first = (uint32_t)off; ra.msg_len = (uint32_t)w.msg_len; ra.in = d_in; ra.offsets = d_offsets;
    ra.flags = c->d_wire_flags; ra.rec = sl.d_stage[6]; ra.rec_stride = pl.bytes(); ra.keep_fields = (uint32_t)nf; ra.keep_k_on_value = 1; ra.code = c->wire_read_code; ra.info = c->wire_read_info;
    if ((rc = prof_launch(c, sl, PK_CBOR_READ, m, [&] { launch_cbor_read(ra, false, sl.stream); }))) return rc;
    if ((rc = prof_launch(c, sl, PK_CBOR_READ_VALIDATE, m, [&] { launch_cbor_read(ra, true, sl.stream); }))) return rc;
  }
  // the nullifier `k` is the first field of the record (src/cbor.rs:250): 32 bytes per proof to the caller's array
  if (w.out_nullifier)
    HIPCK(c, hipMemcpy2DAsync(w.out_nullifier + off * 32, 32, sl.d_stage[6], pl.bytes(), 32, m, mem == ACT_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, sl.stream));
  *d_records = sl.d_stage[6];
  return ACT_OK;
}

// Settling the messages that were not byte-for-byte canonical (ACT_WIRE_READER_HOST): in windows of at most WIRE_SETTLE_WINDOW, each
// read by wire_window_read above; here the window's records that read are verified in one small call and the caller's arrays patched
// over the window's lanes -- the host never holds more than one window of records, whatever the batch looks like.
// `ring` (keyring_impl.inc): the same pass against a ring of issuer keys instead of sk -- ring_verify_locked in place of
// spend_batch_locked, and ring->out_key patched beside the statuses
static int verify_spend_cbor_impl(act_ctx* c, size_t n, int mem, const uint8_t sk[64], const uint8_t* cbor, const uint64_t* offsets,
                                  uint8_t* status, uint8_t* out_kprime, uint8_t* out_nullifier, const RingSel* ring = nullptr) {
  if (!c || (!sk && !ring) || (n && (!cbor || !status))) return ACT_ERR_ARG;
  if (n >= ((size_t)1 << 32)) return ACT_ERR_ARG;
  if (offsets) for (size_t i = 0; i < n; i++) if (offsets[i + 1] < offsets[i]) return ACT_ERR_ARG;     // message i = [offsets[i], offsets[i+1])
  Call call(c, n);
  HIPCK(c, hipSetDevice(c->device));
  if (!n) return call.finish();
  const CborType* T = cbor_type(ACT_CBOR_SPEND_PROOF);
  Slot& s0 = c->slots[0];
  CborDev d; int rc = cbor_dev_prepare(c, s0, ACT_CBOR_SPEND_PROOF, &d); if (rc) return rc;
  c->wire_layout = &d;
  const size_t ml = d.lay.tmpl.size(), pb = ProofLayout{c->L}.bytes();
  const bool dev_reader = c->wire_reader.load() == ACT_WIRE_READER_DEVICE;
  if (dev_reader && (rc = wire_codes_reserve(c, n))) return rc;
  if ((rc = wire_flags_reserve(c, n))) return rc;             // (waits for both memsets: the other slot's stream reads the layout and the flags too)
  WireSrc w{cbor, offsets, ml, out_nullifier};
  const DevKey* d_ring = nullptr;
  if (ring && (rc = ring_set(c, ring->keys, ring->nkeys, &d_ring))) { c->wire_layout = nullptr; return rc; }
  if (dev_reader) { c->wire_read_code = c->d_wire_codes; c->wire_read_info = c->d_wire_codes + c->d_wire_codes_cap; }
  rc = ring ? ring_verify_locked(c, n, mem, d_ring, ring->nkeys, nullptr, status, ring->out_key, out_kprime, &w, ring->bind)
            : spend_batch_locked(c, n, mem, sk, nullptr, false, nullptr, ACT_RNG_PER_LANE, nullptr, status, out_kprime, &w);
  c->wire_layout = nullptr; c->wire_read_code = c->wire_read_info = nullptr;
  if (rc) return rc;
  if (dev_reader) {
    // every message has been verified once, in the pipeline.  A message the reader refused was verified as the all-zero record the
    // reader left: it takes its wire status, all-zero K' and nullifier and ACT_KEY_NONE -- what the settle loop below patches in
    std::vector<uint8_t> ci(c->d_wire_codes_cap + n);      // codes and infos lie in one buffer: one copy
    HIPCK(c, hipMemcpy(ci.data(), c->d_wire_codes, ci.size(), hipMemcpyDeviceToHost));
    const uint8_t *code = ci.data(), *info = ci.data() + c->d_wire_codes_cap;
    size_t read = 0, refused = 0;
    for (size_t i = 0; i < n; i++) if (info[i] & act::CBOR_INFO_DEVICE) { read++; refused += code[i] != CBOR_OK; }
    if (refused && mem == ACT_MEM_DEVICE) {
      CborSettleArgs sa{(uint32_t)n, c->d_wire_codes, c->d_wire_codes + c->d_wire_codes_cap, status, out_kprime, out_nullifier, ring ? ring->out_key : nullptr};
      launch_cbor_settle(sa, s0.stream);
      HIPCK(c, hipGetLastError());
      HIPCK(c, hipStreamSynchronize(s0.stream));
    } else if (refused) {
      for (size_t i = 0; i < n; i++) {
        if (!(info[i] & act::CBOR_INFO_DEVICE) || code[i] == CBOR_OK) continue;
        status[i] = act::cbor_code_status(code[i]);
        if (out_kprime) memset(out_kprime + i * 32, 0, 32);
        if (out_nullifier && !(info[i] & act::CBOR_INFO_KEPT_K)) memset(out_nullifier + i * 32, 0, 32);
        if (ring) ring->out_key[i] = (uint8_t)ACT_KEY_NONE;
      }
    }
    c->wire_stats[0] += n; c->wire_stats[1] += n - read; c->wire_stats[2] += read;
    return call.finish();
  }
  std::vector<uint8_t> flags(n);
  HIPCK(c, hipMemcpy(flags.data(), c->d_wire_flags, n, hipMemcpyDeviceToHost));
  std::vector<size_t> which;
  for (size_t i = 0; i < n; i++) if (flags[i] & 0x80) which.push_back(i);
  c->wire_stats[0] += n; c->wire_stats[1] += n - which.size(); c->wire_stats[3] += which.size();
  const WireExtent x{cbor, offsets, ml};
  WireWindow win;
  std::vector<uint8_t> st2, kp2, ok2, verdict, kprime, nul, key, bind2;      // bind2: a bound ring call's bindings of the window's records (DESIGN 4.12)
  std::vector<size_t> good;
  for (size_t w0 = 0; w0 < which.size(); w0 += WIRE_SETTLE_WINDOW) {
    const size_t cnt = std::min(which.size(), w0 + WIRE_SETTLE_WINDOW) - w0;
    const size_t* lanes = which.data() + w0;
    if ((rc = wire_window_read(c, s0.stream, *T, x, mem == ACT_MEM_DEVICE, lanes, cnt, pb, win))) return rc;
    // a refused message: its wire status, all-zero K' and ACT_KEY_NONE, and its `k` (the record's first field) as it stood on the wire
    // if every field read; then the records of the messages that read move to the front, one behind the other, for the small call
    verdict = win.status; kprime.assign(cnt * 32, 0); key.assign(cnt, (uint8_t)ACT_KEY_NONE); nul.resize(cnt * 32); good.clear();
    for (size_t k = 0; k < cnt; k++) {
      memcpy(nul.data() + k * 32, win.recs.data() + k * pb, 32);
      if (win.codes[k] != CBOR_OK) continue;
      if (good.size() != k) memcpy(win.recs.data() + good.size() * pb, win.recs.data() + k * pb, pb);
      good.push_back(k);
    }
    if (!good.empty()) {
      st2.assign(good.size(), 0); ok2.assign(good.size(), (uint8_t)ACT_KEY_NONE);
      if (out_kprime) kp2.assign(good.size() * 32, 0);
      if (ring && ring->bind) {      // the bindings follow their records into the small call
        bind2.resize(good.size() * 32);
        for (size_t g = 0; g < good.size(); g++) {
          const uint8_t* from = ring->bind + lanes[good[g]] * 32;
          if (mem == ACT_MEM_DEVICE) HIPCK(c, hipMemcpy(bind2.data() + g * 32, from, 32, hipMemcpyDeviceToHost)); else memcpy(bind2.data() + g * 32, from, 32);
        }
      }
      rc = ring ? ring_verify_locked(c, good.size(), ACT_MEM_HOST, d_ring, ring->nkeys, win.recs.data(), st2.data(), ok2.data(), out_kprime ? kp2.data() : nullptr, nullptr,
                                     ring->bind ? bind2.data() : nullptr)
                : spend_batch_locked(c, good.size(), ACT_MEM_HOST, sk, win.recs.data(), false, nullptr, ACT_RNG_PER_LANE, nullptr, st2.data(), out_kprime ? kp2.data() : nullptr);
      if (rc) return rc;
      for (size_t g = 0; g < good.size(); g++) {
        const size_t k = good[g];
        if ((verdict[k] = st2[g])) continue;
        if (out_kprime) memcpy(kprime.data() + k * 32, kp2.data() + g * 32, 32);
        key[k] = ok2[g];
      }
    }
    // (the span of the window's lanes, read once and written back once, as before: with one message in 64 respelled the lane-by-lane
    // road of the issuance settle measured 27 % slower here -- 512 blocking copies of 1 to 32 bytes in place of four of the span)
    if ((rc = wire_patch_lanes(c, mem, status, 1, lanes, cnt, verdict.data(), true))) return rc;
    if ((rc = wire_patch_lanes(c, mem, out_kprime, 32, lanes, cnt, kprime.data(), true))) return rc;
    if ((rc = wire_patch_lanes(c, mem, out_nullifier, 32, lanes, cnt, nul.data(), true))) return rc;
    if ((rc = wire_patch_lanes(c, mem, ring ? ring->out_key : nullptr, 1, lanes, cnt, key.data(), true))) return rc;
  }
  return call.finish();
}

int act_verify_spend_cbor_batch(act_ctx* c, size_t n, int mem, const uint8_t sk[64], const uint8_t* cbor, const uint64_t* offsets,
                                uint8_t* status, uint8_t* out_kprime) {
  return verify_spend_cbor_impl(c, n, mem, sk, cbor, offsets, status, out_kprime, nullptr);
}
int act_verify_spend_cbor_keys_batch(act_ctx* c, size_t n, int mem, const uint8_t sk[64], const uint8_t* cbor, const uint64_t* offsets,
                                     uint8_t* status, uint8_t* out_kprime, uint8_t* out_nullifier) {
  return verify_spend_cbor_impl(c, n, mem, sk, cbor, offsets, status, out_kprime, out_nullifier);
}

}  // extern "C"

// ---- wire bytes in, wire bytes out ------------------------------------------------------------------------------------------
// Refund::to_cbor (src/cbor.rs:421-433) is a 141-byte template around four 32-byte payloads.  Host-memory callers get it written where
// the signatures landed -- on the host workers, 128 payload bytes per lane, nothing crosses PCIe a second time; device-memory callers
// through the framing kernel.  A lane that was not signed gets an all-zero slot.
namespace {
struct FrameJob { const CborLayout* lay; const uint8_t* rec; const uint8_t* status; uint8_t* out; };
void cbor_frame_refunds_host(const CborLayout& lay, size_t n, const uint8_t* rec, const uint8_t* status, uint8_t* out) {
  FrameJob j{&lay, rec, status, out};
  act_host_parallel_for(n, 4096, 0, [](void* p, size_t i0, size_t i1) {
    const FrameJob& j = *static_cast<const FrameJob*>(p);
    const size_t ml = j.lay->tmpl.size(), nf = j.lay->pay_off.size();
    for (size_t i = i0; i < i1; i++) {
      uint8_t* dst = j.out + i * ml;
      if (j.status[i]) { memset(dst, 0, ml); continue; }
      memcpy(dst, j.lay->tmpl.data(), ml);
      for (size_t f = 0; f < nf; f++) memcpy(dst + j.lay->pay_off[f], j.rec + (i * nf + f) * 32, 32);
    }
  }, &j);
}
__global__ void __launch_bounds__(256) k_cbor_zero_failed(uint8_t* out, uint32_t ml, const uint8_t* status, uint32_t n) {
  uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n || status[i] == 0) return;
  for (uint32_t b = 0; b < ml; b++) out[(size_t)i * ml + b] = 0;
}
// device temporaries of the composed calls (wiped before they go back to the allocator: K' and refunds are not secrets, rng is)
struct DevTmp {
  act_ctx* c; uint8_t* p = nullptr; size_t bytes = 0;
  explicit DevTmp(act_ctx* c_) : c(c_) {}
  int alloc(size_t b) {
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCK(c, hipSetDevice(c->device));
    HIPCK(c, hipMalloc(&p, b ? b : 1)); bytes = b;
    return ACT_OK;
  }
  ~DevTmp() { if (p) { (void)hipSetDevice(c->device); if (bytes) (void)hipMemset(p, 0, bytes); (void)hipFree(p); } }
};
// number of lanes with status 0 (host or device array)
int count_accepted(act_ctx* c, int mem, const uint8_t* st, size_t n, size_t* out) {
  std::vector<uint8_t> h;
  if (mem == ACT_MEM_DEVICE) {
    h.resize(n);
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCK(c, hipSetDevice(c->device));
    HIPCK(c, hipMemcpy(h.data(), st, n, hipMemcpyDeviceToHost));
    st = h.data();
  }
  size_t a = 0;
  for (size_t i = 0; i < n; i++) a += st[i] == 0;
  *out = a;
  return ACT_OK;
}
// ACT_RNG_CALLBACK -> drawn bytes where the signing call can read them (host vector, or a device copy for device-memory callers)
struct ResolvedRng {
  act::DrawnRng drawn; DevTmp dev;
  explicit ResolvedRng(act_ctx* c) : dev(c) {}
  int resolve(act_ctx* c, int mem, const uint8_t* st, size_t n, const uint8_t*& rng, int& mode) {
    if (mode != ACT_RNG_CALLBACK) return (mode == ACT_RNG_PER_LANE || mode == ACT_RNG_SEQUENTIAL) ? ACT_OK : ACT_ERR_ARG;
    size_t acc = 0; int rc = count_accepted(c, mem, st, n, &acc); if (rc) return rc;
    if ((rc = drawn.resolve(rng, mode, acc))) return rc;
    if (mem == ACT_MEM_DEVICE) {
      if ((rc = dev.alloc(drawn.buf.size()))) return rc;
      std::lock_guard<std::mutex> lk(c->mu);
      HIPCK(c, hipMemcpy(dev.p, drawn.buf.data(), drawn.buf.size(), hipMemcpyHostToDevice));
      rng = dev.p;
    }
    return ACT_OK;
  }
};
}  // namespace

extern "C" {

int act_refund_sign_cbor_batch(act_ctx* c, size_t n, int mem, const uint8_t sk[64], const uint8_t* kprime, const uint8_t* status_in,
                               const uint8_t* rng, int rng_mode, uint8_t* out_refund_cbor, uint8_t* status) {
  if (!c || !sk || !rng || (n && (!kprime || !status_in || !out_refund_cbor || !status))) return ACT_ERR_ARG;
  if (n == 0) return ACT_OK;
  ResolvedRng rr(c);
  int rc = rr.resolve(c, mem, status_in, n, rng, rng_mode); if (rc) return rc;
  const CborLayout lay = cbor_layout(*cbor_type(ACT_CBOR_REFUND), c->L);
  if (mem == ACT_MEM_HOST) {
    std::vector<uint8_t> rec(n * 128);
    if ((rc = act_refund_sign_batch(c, n, mem, sk, kprime, status_in, rng, rng_mode, rec.data(), status))) return rc;
    cbor_frame_refunds_host(lay, n, rec.data(), status, out_refund_cbor);
    return ACT_OK;
  }
  DevTmp rec(c);
  if ((rc = rec.alloc(n * 128))) return rc;
  if ((rc = act_refund_sign_batch(c, n, mem, sk, kprime, status_in, rng, rng_mode, rec.p, status))) return rc;
  if ((rc = act_cbor_encode_batch(c, ACT_CBOR_REFUND, n, mem, rec.p, out_refund_cbor))) return rc;
  std::lock_guard<std::mutex> lk(c->mu);
  HIPCK(c, hipSetDevice(c->device));
  hipLaunchKernelGGL(k_cbor_zero_failed, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->slots[0].stream, out_refund_cbor, (uint32_t)lay.tmpl.size(), status, (uint32_t)n);
  HIPCK(c, hipStreamSynchronize(c->slots[0].stream));
  return ACT_OK;
}

// A tiny wire-level refund whose rng slices do not depend on the verdicts (ACT_RNG_PER_LANE bytes, or one message with its 128 bytes):
// unframing, verification and the signature BESIDE it (small_impl.inc) as one call, then the framing of the Refund messages on the
// host -- 2.2 ms for one message instead of 3.1 through verify -> sign.  Returns TINY_NEEDS_GENERAL_PATH (a private, negative value
// that no public ACT_ERR_* code can equal) when a message turned out not to be the canonical encoding (the unframing kernel flags it):
// nothing has been written, the caller takes the general path with its host reader.
// (the core hands back raw Refund records, verdicts and, if asked, the nullifiers as they stood on the wire: act_redeem_cbor_batch's
// tiny form puts the nullifier store between this and the framing)
constexpr int TINY_NEEDS_GENERAL_PATH = -1;
static int refund_cbor_tiny_records(act_ctx* c, size_t n, const uint8_t sk[64], const uint8_t* cbor, const uint64_t* offsets, const uint8_t* rng, int rng_mode,
                                    std::vector<uint8_t>& rec, std::vector<uint8_t>& st, uint8_t* out_nullifier) {
  if (offsets) for (size_t i = 0; i < n; i++) if (offsets[i + 1] < offsets[i]) return ACT_ERR_ARG;
  rec.assign(n * 128, 0); st.assign(n, 0);
  std::vector<uint8_t> flags(n);
  {
    Call call(c, n);
    HIPCK(c, hipSetDevice(c->device));
    Slot& s0 = c->slots[0];
    CborDev d; int rc = cbor_dev_prepare(c, s0, ACT_CBOR_SPEND_PROOF, &d); if (rc) return rc;
    c->wire_layout = &d;
    if ((rc = wire_flags_reserve(c, n))) return rc;
    WireSrc w{cbor, offsets, d.lay.tmpl.size(), out_nullifier};
    rc = spend_batch_locked(c, n, ACT_MEM_HOST, sk, nullptr, true, rng, rng_mode, rec.data(), st.data(), nullptr, &w);
    c->wire_layout = nullptr;
    if (rc) return rc;
    HIPCK(c, hipMemcpy(flags.data(), c->d_wire_flags, n, hipMemcpyDeviceToHost));
    if ((rc = call.finish())) return rc;
  }
  for (size_t i = 0; i < n; i++) if (flags[i] & 0x80) return TINY_NEEDS_GENERAL_PATH;
  return ACT_OK;
}
static bool tiny_refund_applies(const act_ctx* c, size_t n, int mem, int rng_mode) {
  return mem == ACT_MEM_HOST && n <= TINY_MAX && n <= c->max_batch && n <= c->small_max.load() && tiny_enabled(c) &&
         (rng_mode == ACT_RNG_PER_LANE || (rng_mode == ACT_RNG_SEQUENTIAL && n == 1));
}
int act_refund_cbor_keys_batch(act_ctx* c, size_t n, int mem, const uint8_t sk[64], const uint8_t* cbor, const uint64_t* offsets,
                               const uint8_t* rng, int rng_mode, uint8_t* out_refund_cbor, uint8_t* status, uint8_t* out_nullifier) {
  if (!c || !sk || !rng || (n && (!cbor || !out_refund_cbor || !status))) return ACT_ERR_ARG;
  if (rng_mode != ACT_RNG_PER_LANE && rng_mode != ACT_RNG_SEQUENTIAL && rng_mode != ACT_RNG_CALLBACK) return ACT_ERR_ARG;
  if (n == 0) return ACT_OK;
  if (tiny_refund_applies(c, n, mem, rng_mode)) {
    std::vector<uint8_t> rec, st;
    const int rc = refund_cbor_tiny_records(c, n, sk, cbor, offsets, rng, rng_mode, rec, st, out_nullifier);
    if (rc == ACT_OK) {
      cbor_frame_refunds_host(cbor_layout(*cbor_type(ACT_CBOR_REFUND), c->L), n, rec.data(), st.data(), out_refund_cbor);
      memcpy(status, st.data(), n);
    }
    if (rc != TINY_NEEDS_GENERAL_PATH) return rc;
  }
  std::vector<uint8_t> h; DevTmp d(c);
  uint8_t* kp; uint8_t* st; int rc;
  if (mem == ACT_MEM_DEVICE) { if ((rc = d.alloc(n * 33))) return rc; kp = d.p; st = d.p + n * 32; }
  else { h.resize(n * 33); kp = h.data(); st = h.data() + n * 32; }
  if ((rc = verify_spend_cbor_impl(c, n, mem, sk, cbor, offsets, st, kp, out_nullifier))) return rc;
  return act_refund_sign_cbor_batch(c, n, mem, sk, kp, st, rng, rng_mode, out_refund_cbor, status);
}
int act_refund_cbor_batch(act_ctx* c, size_t n, int mem, const uint8_t sk[64], const uint8_t* cbor, const uint64_t* offsets,
                          const uint8_t* rng, int rng_mode, uint8_t* out_refund_cbor, uint8_t* status) {
  return act_refund_cbor_keys_batch(c, n, mem, sk, cbor, offsets, rng, rng_mode, out_refund_cbor, status, nullptr);
}

}  // extern "C"
