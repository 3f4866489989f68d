// copy_lanes.h — the per-lane bodies of the copy stage of admission (k_copies.hip), as functions that also compile under
// g++ (tests/hostcheck/copy_check.cpp runs and sanitizes them; the admit_lanes.h / keyring_lanes.h / spend_lanes.h pattern).
//
// act_redeem_(cbor_)admit_unique_batch verify byte-identical proofs of one batch once.  The stage runs over the SURVIVORS of the
// screen in their compact order (j = a survivor's place in idx[], which is lane order: the smallest j is the smallest lane):
//   copy_fp_*          lane = wavefront per survivor   64-bit keyed fingerprint of the input bytes: thread t mixes the 16-byte pieces
//                                                      t, t + 64, ... with their index, the 64 partial values are ADDED (commutative)
//   copy_claim_lane    lane = survivor                 open addressing over (fp, j): compare-and-swap on fp, then min on j
//   copy_leader_lane   lane = survivor                 leader[j] = the smallest j with this fingerprint
//   copy_equal_*       lane = wavefront per survivor   the exact compare with the leader's bytes: copy_of[j] = leader[j] only when
//                                                      the lengths and EVERY byte are equal -- a fingerprint collision costs a
//                                                      verification and never changes an answer
//   copy_mark_lane     lane = survivor                 the side array of the second compaction and every copy's leader LANE
//   copy_resolve_lane  lane = item                     a copy's status and out_key from its leader's final ones
//   copy_serve_lane    lane = item                     the replay unique forms: a copy's status, out_key, replay mark and output row
//                                                      from its leader's final ones (copy_serve_piece: one 16-byte piece of the row)
//   copy_serve_return_lane  lane = item                the return replay unique forms: the same from the leader's final status AND
//                                                      whether the copy names the leader's amount (copy_serve_return_piece)
// Nothing here is secret: proofs, fingerprints, lane numbers, amounts, statuses and refunds are public.
#pragma once
#include "admit_lanes.h"

namespace act {

constexpr uint32_t COPY_NONE = 0xFFFFFFFFu;       // copy_of[] / lead[] of a lane that is not a copy; lane word of an unclaimed slot
constexpr uint8_t COPY_MARK = 249;                // a copy in the side array the second compaction reads: any non-zero byte would do.  (The
                                                  // return calls' RETURN_TOO_BIG has this value: a copy is told from a shed lane by lead[] alone.)
constexpr uint8_t COPY_RECORDED_UNSIGNED = 251;   // ACT_STATUS_RECORDED_UNSIGNED

// ---- where a survivor's input bytes are ---------------------------------------------------------------------------------------------
// records: lane i = [i * row_bytes, (i + 1) * row_bytes); wire: [offsets[i], offsets[i + 1]), or rows of row_bytes without offsets
struct CopySpan { const uint8_t* src; const uint64_t* offsets; uint64_t row_bytes; };
ACT_HD uint64_t copy_beg(const CopySpan& s, uint32_t lane) { return s.offsets ? s.offsets[lane] : (uint64_t)lane * s.row_bytes; }
ACT_HD uint64_t copy_len(const CopySpan& s, uint32_t lane) { return s.offsets ? s.offsets[lane + 1] - s.offsets[lane] : s.row_bytes; }

// ---- the fingerprint ----------------------------------------------------------------------------------------------------------------
// 16 bytes at any address (a short last piece zero-padded) as two little-endian words
ACT_HD void copy_load16(uint64_t w[2], const uint8_t* p, uint32_t bytes) {
  uint32_t t[4] = {0, 0, 0, 0};
  if (bytes == 16) __builtin_memcpy(t, p, 16);
  else for (uint32_t i = 0; i < bytes; i++) t[i >> 2] |= (uint32_t)p[i] << (8 * (i & 3u));
  w[0] = (uint64_t)t[0] | (uint64_t)t[1] << 32; w[1] = (uint64_t)t[2] | (uint64_t)t[3] << 32;
}
// SipHash rounds (null_hash's) over the two words of a piece, the state keyed with the set's salt and the piece's index: one
// compression round per word, two closing rounds.  A client who does not know the salt cannot choose pieces whose values cancel.
ACT_HD uint64_t copy_mix(uint64_t a, uint64_t b, uint64_t q, const uint32_t salt[4]) {
  const uint64_t k0 = (uint64_t)salt[0] | (uint64_t)salt[1] << 32, k1 = (uint64_t)salt[2] | (uint64_t)salt[3] << 32;
  uint64_t v0 = k0 ^ 0x736f6d6570736575ull, v1 = k1 ^ 0x646f72616e646f6dull ^ q, v2 = k0 ^ 0x6c7967656e657261ull, v3 = k1 ^ 0x7465646279746573ull ^ (q * 0x9e3779b97f4a7c15ull);
  auto rotl = [](uint64_t x, int s) { return (x << s) | (x >> (64 - s)); };
  auto round = [&]() {
    v0 += v1; v1 = rotl(v1, 13); v1 ^= v0; v0 = rotl(v0, 32);
    v2 += v3; v3 = rotl(v3, 16); v3 ^= v2;
    v0 += v3; v3 = rotl(v3, 21); v3 ^= v0;
    v2 += v1; v1 = rotl(v1, 17); v1 ^= v2; v2 = rotl(v2, 32);
  };
  v3 ^= a; round(); v0 ^= a;
  v3 ^= b; round(); v0 ^= b;
  v2 ^= 0xff; round(); round();
  return v0 ^ v1 ^ v2 ^ v3;
}
// thread t of 64: the sum of its pieces' values
ACT_HD uint64_t copy_fp_partial(const uint8_t* p, uint64_t len, uint32_t t, const uint32_t salt[4]) {
  const uint64_t pieces = (len + 15) / 16;
  uint64_t sum = 0, w[2];
  for (uint64_t q = t; q < pieces; q += 64) {
    copy_load16(w, p + q * 16, admit_piece_bytes(len, (uint32_t)q));
    sum += copy_mix(w[0], w[1], q, salt);
  }
  return sum;
}
// the same sum by ONE thread walking the pieces in order (the host workers: a sequential read; addition is commutative, so this is the
// wavefront's total bit for bit)
ACT_HD uint64_t copy_fp_sum(const uint8_t* p, uint64_t len, const uint32_t salt[4]) {
  const uint64_t pieces = (len + 15) / 16;
  uint64_t sum = 0, w[2];
  for (uint64_t q = 0; q < pieces; q++) {
    copy_load16(w, p + q * 16, admit_piece_bytes(len, (uint32_t)q));
    sum += copy_mix(w[0], w[1], q, salt);
  }
  return sum;
}
// the sum of the 64 partial values and the length -> the fingerprint; never 0 (0 is the empty slot of the leader table)
ACT_HD uint64_t copy_fp_finish(uint64_t sum, uint64_t len, const uint32_t salt[4]) {
  const uint64_t f = copy_mix(sum, len, ~(uint64_t)0, salt);
  return f ? f : 1;
}

struct CopyFpArgs { CopySpan span; const uint32_t* idx; uint32_t m; NullSalt salt; uint64_t* fp; };      // fp[j], j < m: survivor idx[j]

// ---- the leader table ---------------------------------------------------------------------------------------------------------------
// tab_fp: cap words, zero before; tab_j: cap words, COPY_NONE before; cap a power of two >= 2 m.  After copy_claim_lane has run for
// every j (in any order, concurrently on the device) the slot of a fingerprint holds the smallest j that carries it.
struct CopyTableArgs { const uint64_t* fp; uint32_t m; uint64_t* tab_fp; uint32_t* tab_j; uint32_t cap; uint32_t* slot; uint32_t* leader; };

ACT_HD uint32_t copy_slot0(uint64_t fp, uint32_t cap) { return (uint32_t)(fp >> 32) & (cap - 1); }
ACT_HD void copy_claim_lane(const CopyTableArgs& a, uint32_t j) {
  if (j >= a.m) return;
  const uint64_t h = a.fp[j];
  uint32_t t = copy_slot0(h, a.cap);
  for (uint32_t probes = 0; probes < a.cap; probes++, t = (t + 1) & (a.cap - 1)) {
#if defined(__HIP_DEVICE_COMPILE__)
    // a plain look first: in a flood (every lane of the batch on ONE slot) all but the first arrivals find the slot claimed and a
    // smaller j in it, and issue no atomic at all.  Both words only ever move one way (0 -> fp, j downwards), so a stale look costs
    // an atomic and never an answer.
    unsigned long long* slot_fp = reinterpret_cast<unsigned long long*>(a.tab_fp + t);
    unsigned long long seen = __hip_atomic_load(slot_fp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (seen == 0) { seen = atomicCAS(slot_fp, 0ull, (unsigned long long)h); if (seen == 0) seen = h; }      // (0: this lane claimed it)
    if (seen != h) continue;
    if (__hip_atomic_load(a.tab_j + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > j) atomicMin(a.tab_j + t, j);
#else
    if (a.tab_fp[t] == 0) a.tab_fp[t] = h;
    if (a.tab_fp[t] != h) continue;
    if (a.tab_j[t] > j) a.tab_j[t] = j;
#endif
    a.slot[j] = t;
    return;
  }
  a.slot[j] = COPY_NONE;      // (cap >= 2 m: not reached)
}
ACT_HD void copy_leader_lane(const CopyTableArgs& a, uint32_t j) {
  if (j >= a.m) return;
  const uint32_t t = a.slot[j];
  a.leader[j] = t == COPY_NONE ? j : a.tab_j[t];
}

// ---- the exact compare --------------------------------------------------------------------------------------------------------------
// thread t of 64: are the pieces t, t + 64, ... of the two ranges equal (16-byte loads at any address, the short last piece byte-wise)
ACT_HD bool copy_equal_partial(const uint8_t* x, const uint8_t* y, uint64_t len, uint32_t t) {
  const uint64_t pieces = (len + 15) / 16;
  uint64_t d = 0, a[2], b[2];
  for (uint64_t q = t; q < pieces; q += 64) {
    const uint32_t bytes = admit_piece_bytes(len, (uint32_t)q);
    copy_load16(a, x + q * 16, bytes); copy_load16(b, y + q * 16, bytes);
    d |= (a[0] ^ b[0]) | (a[1] ^ b[1]);
  }
  return d == 0;
}
// all pieces by ONE thread in order (the host workers), stopping at the first difference
ACT_HD bool copy_equal_all(const uint8_t* x, const uint8_t* y, uint64_t len) {
  const uint64_t pieces = (len + 15) / 16;
  uint64_t a[2], b[2];
  for (uint64_t q = 0; q < pieces; q++) {
    const uint32_t bytes = admit_piece_bytes(len, (uint32_t)q);
    copy_load16(a, x + q * 16, bytes); copy_load16(b, y + q * 16, bytes);
    if ((a[0] ^ b[0]) | (a[1] ^ b[1])) return false;
  }
  return true;
}
struct CopyEqualArgs { CopySpan span; const uint32_t* idx; const uint32_t* leader; uint32_t m; uint32_t* copy_of; };      // copy_of[j] = leader[j] or COPY_NONE
// the ranges of survivor j and of its leader, or false when j leads itself or the lengths differ (no byte is looked at)
ACT_HD bool copy_equal_ranges(const CopyEqualArgs& a, uint32_t j, const uint8_t** x, const uint8_t** y, uint64_t* len) {
  const uint32_t l = a.leader[j];
  if (l >= j) return false;                                   // (a leader is never behind its lane)
  const uint32_t li = a.idx[l], ji = a.idx[j];
  *len = copy_len(a.span, ji);
  if (copy_len(a.span, li) != *len) return false;
  *x = a.span.src + copy_beg(a.span, ji); *y = a.span.src + copy_beg(a.span, li);
  return true;
}

// ---- the side array of the second compaction ----------------------------------------------------------------------------------------
// pre2 = the screen's pre-status with COPY_MARK on every copy (pre2 starts as a copy of pre); lead[lane] = the leader's LANE of a copy
// (lead starts as COPY_NONE everywhere)
struct CopyMarkArgs { const uint32_t* idx; const uint32_t* copy_of; uint32_t m; uint8_t* pre2; uint32_t* lead; };
ACT_HD void copy_mark_lane(const CopyMarkArgs& a, uint32_t j) {
  if (j >= a.m) return;
  const uint32_t l = a.copy_of[j];
  if (l == COPY_NONE) return;
  a.pre2[a.idx[j]] = COPY_MARK; a.lead[a.idx[j]] = a.idx[l];
}

// ---- a copy's answer ----------------------------------------------------------------------------------------------------------------
// the table of the header: a rejected, double-spent or undetermined leader hands its status on; an accepted one (signed or not) has
// recorded the nullifier, and its copy is a double spend
ACT_HD uint8_t copy_status(uint8_t leader_status) { return (leader_status == 0 || leader_status == COPY_RECORDED_UNSIGNED) ? ADMIT_DOUBLE_SPEND : leader_status; }
struct CopyResolveArgs { const uint32_t* lead; uint32_t n; uint8_t* status; uint8_t* out_key; };
ACT_HD void copy_resolve_lane(const CopyResolveArgs& a, uint32_t i) {
  if (i >= a.n) return;
  const uint32_t l = a.lead[i];
  if (l == COPY_NONE) return;                                 // leaders are never copies: status[l] is final, one pass suffices
  a.status[i] = copy_status(a.status[l]); a.out_key[i] = a.out_key[l];
}

// ---- a copy's answer under replay semantics (act_redeem_(cbor_)admit_replay_unique_batch) ----------------------------------------------
// the table of the header: a leader that ends 0 (fresh or replayed) hands its output record on byte for byte and its copy is a replay;
// every other leader hands its status on and the copy's record stays all-zero.  Rows start at out + i * out_b at ANY byte address (the
// framed Refund is not a multiple of 4 long and the caller's base is free), so a row moves in byte-aligned pieces: copy_load16's
// counterpart for stores, and no row pointer is ever cast to a wider type.
ACT_HD void copy_store16(uint8_t* p, const uint64_t w[2], uint32_t bytes) {
  const uint32_t t[4] = {(uint32_t)w[0], (uint32_t)(w[0] >> 32), (uint32_t)w[1], (uint32_t)(w[1] >> 32)};
  if (bytes == 16) __builtin_memcpy(p, t, 16);
  else for (uint32_t i = 0; i < bytes; i++) p[i] = (uint8_t)(t[i >> 2] >> (8 * (i & 3u)));
}
// out_replayed: nullable.  Reads rows of leaders only and writes rows of copies only (a leader is never a copy): any order, no atomics
struct CopyServeArgs { const uint32_t* lead; uint32_t n; uint64_t out_b; uint8_t* status; uint8_t* out_key; uint8_t* out; uint8_t* out_replayed; };
// piece q of lane i's row (the device runs one thread per piece; piece 0 also writes the lane's three bytes)
ACT_HD void copy_serve_piece(const CopyServeArgs& a, uint32_t i, uint32_t q) {
  if (i >= a.n) return;
  const uint32_t l = a.lead[i];
  if (l == COPY_NONE) return;
  const uint8_t s = a.status[l];                              // (a leader's: final, and no lane of this pass writes it)
  if (q == 0) { a.status[i] = s; a.out_key[i] = a.out_key[l]; if (a.out_replayed) a.out_replayed[i] = s == 0 ? 1 : 0; }
  const uint32_t bytes = admit_piece_bytes(a.out_b, q);
  uint64_t w[2] = {0, 0};
  if (s == 0) copy_load16(w, a.out + (uint64_t)l * a.out_b + (uint64_t)q * 16, bytes);
  copy_store16(a.out + (uint64_t)i * a.out_b + (uint64_t)q * 16, w, bytes);
}
ACT_HD void copy_serve_lane(const CopyServeArgs& a, uint32_t i) {
  const uint32_t pieces = admit_pieces(a.out_b);
  for (uint32_t q = 0; q < pieces; q++) copy_serve_piece(a, i, q);
}

// ---- a copy's answer when lanes name returned amounts (act_redeem_(cbor_)return_replay_unique_batch) ---------------------------
// Equality is decided on the proof bytes alone, so a copy may name another amount than its leader -- and the receipt pins the LEADER's.
// The table of the header, from the leader's final status s and same = (t^_i == t^_l), both reduced mod l as return_exceeds_bytes
// reduces them (t and t + l are one amount):
//   s == 0, same            status 0, replay mark 1, the leader's RefundReturn byte for byte
//   s == 0 or 251, other    ACT_STATUS_DOUBLE_SPEND, a zero record, mark 0
//   s == 251, same          251, a zero record, mark 1: k is spent and the leader's receipt is this lane's own, which is what
//                           act_redeem_(cbor_)return_replay_batch's tail marks before its signing step fails
//   anything else           s, a zero record, mark 0
// out_key is the leader's in every row (the key the shared bytes verified under; ACT_KEY_NONE where they did not verify).
struct CopyServed { uint8_t status, replayed; bool row; };
ACT_HD CopyServed copy_serve_return_verdict(uint8_t s, bool same) {
  if (s == 0) return same ? CopyServed{0, 1, true} : CopyServed{ADMIT_DOUBLE_SPEND, 0, false};
  if (s == COPY_RECORDED_UNSIGNED) return same ? CopyServed{COPY_RECORDED_UNSIGNED, 1, false} : CopyServed{ADMIT_DOUBLE_SPEND, 0, false};
  return CopyServed{s, 0, false};
}
// two amounts as they lie in memory name one t^ (32 little-endian bytes each at any address, any value below 2^256; the screen's
// load, whose reduction is return_exceeds_bytes')
ACT_HD bool copy_same_amount(const uint8_t* x, const uint8_t* y) {
  uint32_t a[8], b[8];
  null_load_key(a, x); null_load_key(b, y);
  return null_eq(a, b);
}
// amounts: n scalars in the memory the arrays of `v` lie in; null: every t^ is 0, so every copy names its leader's amount
struct CopyServeReturnArgs { CopyServeArgs v; const uint8_t* amounts; };
// piece q of lane i's row.  Every thread of a row reads the same leader status and the same two amounts, so all reach one verdict;
// piece 0 also writes the lane's three bytes.  Reads rows, statuses and keys of leaders only, writes those of copies only.
ACT_HD void copy_serve_return_piece(const CopyServeReturnArgs& r, uint32_t i, uint32_t q) {
  const CopyServeArgs& a = r.v;
  if (i >= a.n) return;
  const uint32_t l = a.lead[i];
  if (l == COPY_NONE) return;
  const CopyServed c = copy_serve_return_verdict(a.status[l], !r.amounts || copy_same_amount(r.amounts + (uint64_t)i * 32, r.amounts + (uint64_t)l * 32));
  if (q == 0) { a.status[i] = c.status; a.out_key[i] = a.out_key[l]; if (a.out_replayed) a.out_replayed[i] = c.replayed; }
  const uint32_t bytes = admit_piece_bytes(a.out_b, q);
  uint64_t w[2] = {0, 0};
  if (c.row) copy_load16(w, a.out + (uint64_t)l * a.out_b + (uint64_t)q * 16, bytes);
  copy_store16(a.out + (uint64_t)i * a.out_b + (uint64_t)q * 16, w, bytes);
}
ACT_HD void copy_serve_return_lane(const CopyServeReturnArgs& r, uint32_t i) {
  const uint32_t pieces = admit_pieces(r.v.out_b);
  for (uint32_t q = 0; q < pieces; q++) copy_serve_return_piece(r, i, q);
}

}  // namespace act
