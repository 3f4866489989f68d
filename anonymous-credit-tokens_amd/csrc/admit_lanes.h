// admit_lanes.h — the per-lane bodies of the admission kernels (k_admit.hip), as functions that also compile under g++
// (tests/hostcheck/admit_check.cpp runs and sanitizes them; the spend_lanes.h / keyring_lanes.h pattern).
//
// Admission stands in front of verification: a lane whose charge is not the expected one, or whose nullifier the set
// already holds, is answered without the 39.9 M multiply-accumulates of a verification.  Per lane the screen costs two scalar
// reductions, one comparison and one read-only probe of the set; the survivors are compacted IN LANE ORDER (the first valid lane of
// a fresh nullifier wins, and the sequential rng convention hands slices out in lane order) and only they are verified.
//   admit_wire_piece    lane = (message, field)   framing bytes against the codec's template; fields 0 and 1 (k, s) copied out
//   admit_screen_lane   lane = item               reduce k and s, compare s with the charge, probe the set -> pre-status, reduced k
//   admit_rank ...      lane = item               stable compaction: 64-bit ballot + popcount in the wave, block counts, a scan, the write
//   admit_*_piece       lane = 16-byte piece      gather of the survivors' records / messages / rng slices, scatter of the answers
#pragma once
#include "kernels.h"
#include "null_probe.h"
#include "return_lanes.h"

namespace act {

constexpr uint8_t ADMIT_WRONG_CHARGE = 250;     // ACT_STATUS_WRONG_CHARGE
constexpr uint8_t ADMIT_DOUBLE_SPEND = 3;       // ACT_STATUS_DOUBLE_SPEND
constexpr uint8_t ADMIT_RETURN_TOO_BIG = RETURN_TOO_BIG;      // ACT_STATUS_RETURN_TOO_BIG (return_lanes.h)
constexpr uint32_t ADMIT_SHED = 0xFFFFFFFFu;    // pos[] of a lane that is not verified
constexpr uint32_t ADMIT_BLOCK = 256;           // lanes per workgroup of the compaction kernels (four waves)

// ---- the decision, in the order of the issue's loop ---------------------------------------------------------------------------------
// wire_code: what the wire reader said about the message (0 = well-shaped); charge_given / charge_equal: step 2; the probe is only
// made (found() is only called) for a lane that has passed steps 1 and 2 -- a lane with the wrong charge is not looked up.
// return_given / return_fits (act_redeem_(cbor_)return_batch): the returned amount t against the lane's own s, in the same
// pass and behind the charge -- a lane that fails both rules has the wrong charge, the earlier rule
template <class Probe>
ACT_HD uint8_t admit_decide_return(uint8_t wire_code, bool charge_given, bool charge_equal, bool return_given, bool return_fits, Probe&& found) {
  if (wire_code) return wire_code;
  if (charge_given && !charge_equal) return ADMIT_WRONG_CHARGE;
  if (return_given && !return_fits) return ADMIT_RETURN_TOO_BIG;
  if (found()) return ADMIT_DOUBLE_SPEND;
  return 0;
}
template <class Probe>
ACT_HD uint8_t admit_decide(uint8_t wire_code, bool charge_given, bool charge_equal, Probe&& found) {
  return admit_decide_return(wire_code, charge_given, charge_equal, false, true, found);
}

struct AdmitScreenArgs {
  uint32_t n, stride;                 // k of item i at ks + i * stride, s in the 32 bytes behind it (fields 0 and 1 of a SpendProof record)
  const uint8_t* ks;
  const uint8_t* charge;              // nullable: n scalars like s
  const uint8_t* wire_code;           // nullable: n codes of the wire reader (non-zero: the message is rejected as it stands)
  const uint32_t* tab_keys; const uint32_t* tab_state; uint32_t tab_cap; NullSalt salt;      // the set's persistent table (read only)
  uint8_t* pre;                       // n: 0 = goes on to verification, else the lane's final status
  uint8_t* kred;                      // n * 32: k reduced mod l (the set's key), all zero for a lane the wire reader rejected
  const uint8_t* returned;            // nullable: n scalars like s, the amounts t the issuer returns (t > s, both reduced: ADMIT_RETURN_TOO_BIG)
};

ACT_HD void admit_screen_lane(const AdmitScreenArgs& a, uint32_t i) {
  if (i >= a.n) return;
  const uint8_t code = a.wire_code ? a.wire_code[i] : (uint8_t)0;
  uint32_t k[8] = {0, 0, 0, 0, 0, 0, 0, 0}, s[8], want[8];
  bool eq = true, fits = true;
  if (!code) {
    null_load_key(k, a.ks + (size_t)i * a.stride);
    if (a.charge || a.returned) null_load_key(s, a.ks + (size_t)i * a.stride + 32);
    if (a.charge) { null_load_key(want, a.charge + (size_t)i * 32); eq = null_eq(s, want); }
    if (a.returned) { null_load_key(want, a.returned + (size_t)i * 32); fits = !return_exceeds(want, s); }
  }
  a.pre[i] = admit_decide_return(code, a.charge != nullptr, eq, a.returned != nullptr, fits, [&]() { return null_probe_contains(k, a.tab_keys, a.tab_state, a.tab_cap, a.salt.w); });
  uint32_t* dst = reinterpret_cast<uint32_t*>(a.kred + (size_t)i * 32);      // kred is the engine's own allocation: 4-byte aligned
  for (int j = 0; j < 8; j++) dst[j] = k[j];
}

// ---- wire form: the framing of a canonical message against the codec's template -----------------------------------------------------
struct AdmitWireArgs {
  uint32_t n, n_fields, msg_len;      // msg_len = canonical length
  const uint8_t* cbor; const uint64_t* offsets;      // offsets nullable: message m = [m * msg_len, (m + 1) * msg_len)
  const uint8_t* tmpl; const uint32_t* pay_off;      // the canonical template and every field's payload offset in it (cbor_layout)
  uint8_t* ks;                        // n * 64: the payloads of fields 0 and 1, raw
  uint8_t* flags;                     // n, rounded up to a multiple of 4: 0x80 = not byte-for-byte canonical (the host reader settles it)
};
// the framing bytes in front of field f (and, for the last field, nothing behind it: the template ends with a payload).  true = as
// the template has them.  Fields 0 and 1 are copied to ks whether or not the rest of the message is canonical: a message that is
// not is read again by the host reader, which overwrites them.
ACT_HD bool admit_wire_piece(const AdmitWireArgs& a, uint32_t m, uint32_t f) {
  const uint64_t beg = a.offsets ? a.offsets[m] : (uint64_t)m * a.msg_len, end = a.offsets ? a.offsets[m + 1] : beg + a.msg_len;
  if (end - beg < a.msg_len) return false;                    // (a canonical prefix is enough: one item is read, trailing bytes are not)
  const uint8_t* src = a.cbor + beg;
  const uint32_t off = a.pay_off[f], prev_end = f ? a.pay_off[f - 1] + 32 : 0;
  bool canon = true;
  for (uint32_t i = prev_end; i < off; i++) canon = canon && (src[i] == a.tmpl[i]);
  if (f < 2) { uint8_t* d = a.ks + (size_t)m * 64 + 32 * f; for (int i = 0; i < 32; i++) d[i] = src[off + i]; }
  return canon;
}

// ---- stable compaction --------------------------------------------------------------------------------------------------------------
ACT_HD bool admit_keep(uint8_t pre) { return pre == 0; }
// survivors below `lane` in a wave whose survivors are `mask`
ACT_HD uint32_t admit_rank(uint64_t mask, uint32_t lane) { return (uint32_t)__builtin_popcountll(mask & ((1ull << lane) - 1ull)); }
// survivors in the waves below wave w of a workgroup (wave_count[] = popcount of each wave's mask)
ACT_HD uint32_t admit_wave_base(const uint32_t wave_count[ADMIT_BLOCK / 64], uint32_t w) { uint32_t b = 0; for (uint32_t j = 0; j < w; j++) b += wave_count[j]; return b; }
// The scan of the workgroup counts by ONE workgroup of `threads`: thread t owns the segment [t * seg, (t + 1) * seg) of blk[0 .. nb),
// sums it, the sums are scanned, and the thread rewrites its segment as exclusive prefixes starting from its own.
ACT_HD uint32_t admit_scan_seg(uint32_t nb, uint32_t threads) { return (nb + threads - 1) / threads; }
ACT_HD uint32_t admit_scan_sum(const uint32_t* blk, uint32_t nb, uint32_t seg, uint32_t t) {
  uint32_t s = 0;
  for (uint64_t j = (uint64_t)t * seg; j < (uint64_t)(t + 1) * seg && j < nb; j++) s += blk[j];
  return s;
}
ACT_HD void admit_scan_write(uint32_t* blk, uint32_t nb, uint32_t seg, uint32_t t, uint32_t start) {
  for (uint64_t j = (uint64_t)t * seg; j < (uint64_t)(t + 1) * seg && j < nb; j++) { const uint32_t v = blk[j]; blk[j] = start; start += v; }
}

// ---- gather and scatter: 16-byte pieces ---------------------------------------------------------------------------------------------
ACT_HD void admit_move16(uint8_t* dst, const uint8_t* src, uint32_t bytes) {
  if (bytes == 16) { uint32_t t[4]; __builtin_memcpy(t, src, 16); __builtin_memcpy(dst, t, 16); }
  else for (uint32_t i = 0; i < bytes; i++) dst[i] = src[i];
}
ACT_HD void admit_zero16(uint8_t* dst, uint32_t bytes) {
  if (bytes == 16) { const uint32_t z[4] = {0, 0, 0, 0}; __builtin_memcpy(dst, z, 16); }
  else for (uint32_t i = 0; i < bytes; i++) dst[i] = 0;
}
ACT_HD uint32_t admit_pieces(uint64_t bytes) { return (uint32_t)((bytes + 15) / 16); }
ACT_HD uint32_t admit_piece_bytes(uint64_t row_bytes, uint32_t q) { const uint64_t left = row_bytes - (uint64_t)q * 16; return left < 16 ? (uint32_t)left : 16u; }

// rows of one size (records, rng slices): dst row j = src row idx[j], j < m.  Piece p = (row p / pieces, piece p % pieces).
struct AdmitRowsArgs { uint8_t* dst; const uint8_t* src; const uint32_t* idx; uint32_t m; uint64_t row_bytes; };
ACT_HD void admit_rows_piece(const AdmitRowsArgs& a, uint64_t p) {
  const uint32_t pieces = admit_pieces(a.row_bytes);
  const uint64_t j = p / pieces; const uint32_t q = (uint32_t)(p % pieces);
  if (j >= a.m) return;
  admit_move16(a.dst + j * a.row_bytes + (uint64_t)q * 16, a.src + (uint64_t)a.idx[j] * a.row_bytes + (uint64_t)q * 16, admit_piece_bytes(a.row_bytes, q));
}
// messages (contiguous bytes between monotone offsets): dst message j = [dst_off[j], dst_off[j + 1]) = the bytes at src + src_beg[j]
struct AdmitMsgsArgs { uint8_t* dst; const uint64_t* dst_off; const uint8_t* src; const uint64_t* src_beg; uint32_t m; uint32_t max_pieces; };
ACT_HD void admit_msgs_piece(const AdmitMsgsArgs& a, uint64_t p) {
  const uint64_t j = p / a.max_pieces; const uint32_t q = (uint32_t)(p % a.max_pieces);
  if (j >= a.m) return;
  const uint64_t len = a.dst_off[j + 1] - a.dst_off[j];
  if ((uint64_t)q * 16 >= len) return;
  admit_move16(a.dst + a.dst_off[j] + (uint64_t)q * 16, a.src + a.src_beg[j] + (uint64_t)q * 16, admit_piece_bytes(len, q));
}
// the answers back to their lanes: a verified lane takes its compact status, key index and output record, a shed lane its
// pre-status, ACT_KEY_NONE and an all-zero record
struct AdmitScatterArgs {
  uint32_t n; uint64_t out_bytes;     // per lane: 128 (Refund record) or the Refund message's length
  const uint32_t* pos; const uint8_t* pre;
  const uint8_t* c_status; const uint8_t* c_key; const uint8_t* c_out;      // compact, m entries
  uint8_t* status; uint8_t* out_key; uint8_t* out;
};
ACT_HD void admit_scatter_piece(const AdmitScatterArgs& a, uint64_t p) {
  const uint32_t pieces = admit_pieces(a.out_bytes);
  const uint64_t i = p / pieces; const uint32_t q = (uint32_t)(p % pieces);
  if (i >= a.n) return;
  const uint32_t j = a.pos[i];
  if (q == 0) { a.status[i] = j == ADMIT_SHED ? a.pre[i] : a.c_status[j]; a.out_key[i] = j == ADMIT_SHED ? (uint8_t)255 : a.c_key[j]; }
  uint8_t* dst = a.out + i * a.out_bytes + (uint64_t)q * 16;
  const uint32_t bytes = admit_piece_bytes(a.out_bytes, q);
  if (j == ADMIT_SHED) admit_zero16(dst, bytes);
  else admit_move16(dst, a.c_out + (uint64_t)j * a.out_bytes + (uint64_t)q * 16, bytes);
}
// the reader's records of the messages that were not canonical, over what admit_wire_piece left: ks[which[t]] = patch[t]
struct AdmitPatchArgs { uint8_t* ks; const uint32_t* which; const uint8_t* patch; uint32_t count; };
ACT_HD void admit_patch_piece(const AdmitPatchArgs& a, uint32_t p) {
  const uint32_t t = p / 4, q = p % 4;
  if (t >= a.count) return;
  admit_move16(a.ks + (size_t)a.which[t] * 64 + q * 16, a.patch + (size_t)t * 64 + q * 16, 16);
}

}  // namespace act
