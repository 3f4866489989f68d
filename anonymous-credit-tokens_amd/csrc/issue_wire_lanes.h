// issue_wire_lanes.h — the issuance side of the wire reader as lane bodies (kernels in k_sign.hip; the cbor_lanes.h / admit_lanes.h
// pattern: the same functions compile under g++, where tests/hostcheck/issue_wire_read_check.cpp runs the whole device road of one
// IssuanceRequest message beside its specification).
//
// Under ACT_WIRE_READER_DEVICE a chunk of act_issue_cbor_batch / act_issue_check_cbor_batch is, on the chunk's own stream,
//     k_issue_wire_flag        issue_wire_flag_lane     the 13 framing bytes against the template -> wire_flags[first + p]
//     k_cbor_read_raw<false>   cbor_read_message_lane   flagged messages only: record (128 bytes, as on the wire), code, info
//     k_cbor_read_raw<true>                             ... the ones whose first failure in wire order needs the points decoded
//     k_issue_a_wire_read      issue_wire_take_lane     a flagged lane takes its four fields from the record the reader left
//     k_issue_check            issue_wire_status        a refused lane's status is its wire status
// The specification is the host road (issue_wire_impl.inc issue_wire_settle): cbor_read_message, cbor_settle_codes, decode_scalar
// on gamma / k_bar / r_bar, 254 / 253 / 255 for a message that does not read.
#pragma once
#include "cbor_lanes.h"

namespace act {

// (a) the flag pass.  ciborium reads one item and ignores trailing bytes: a canonical prefix is enough (issue_a_lane<1> in k_sign.hip
// does the same comparison for the host road).  pay_off: the offsets of the four payloads in the canonical message `tmpl`.
struct IssueWireFlagArgs {
  uint32_t n, first;                  // message p of this launch is message first + p of the call
  uint32_t msg_len;                   // the canonical length; offsets == null: message p = [p * msg_len, (p + 1) * msg_len)
  const uint8_t* wire; const uint64_t* wire_off;
  const uint8_t* tmpl; const uint32_t* pay_off;
  uint8_t* flags;                     // flags[first + p] = 0x80: not the canonical encoding
};
ACT_HD bool issue_wire_canonical(const uint8_t* src, uint64_t len, const uint8_t* tmpl, const uint32_t* pay_off, uint32_t msg_len) {
  bool canon = len >= msg_len;
  for (uint32_t f = 0, prev = 0; canon && f < 4; prev = pay_off[f] + 32, f++)
    for (uint32_t i = prev; i < pay_off[f]; i++) canon = canon && src[i] == tmpl[i];
  return canon;
}
ACT_HD void issue_wire_flag_lane(const IssueWireFlagArgs& a, uint32_t p) {
  if (p >= a.n) return;
  const uint64_t beg = a.wire_off ? a.wire_off[p] : (uint64_t)p * a.msg_len, end = a.wire_off ? a.wire_off[p + 1] : beg + a.msg_len;
  a.flags[a.first + p] = issue_wire_canonical(a.wire + beg, end - beg, a.tmpl, a.pay_off, a.msg_len) ? 0 : 0x80;
}

// (c) a canonical lane: the four payloads where the template has them, byte-aligned 16-byte loads; K as it stands, the scalars reduced
ACT_HD void issue_wire_take_canonical(const uint8_t* src, const uint32_t* pay_off, uint8_t* rec, uint32_t wk[8], sc& gamma, sc& k_bar, sc& r_bar) {
  uint32_t w[8];
  load32_bytes(wk, src + pay_off[0]); store8(rec, wk);
  load32_bytes(w, src + pay_off[1]); gamma = sc_from_words(w); store_sc(rec + 32, gamma);
  load32_bytes(w, src + pay_off[2]); k_bar = sc_from_words(w); store_sc(rec + 64, k_bar);
  load32_bytes(w, src + pay_off[3]); r_bar = sc_from_words(w); store_sc(rec + 96, r_bar);
}
// the take-up of a flagged lane: rec is the 128-byte record the reader wrote (K | gamma | k_bar | r_bar as they stood on the
// wire) or zeroed.  CBOR_OK: K's bytes and the three scalars REDUCED (decode_scalar, src/cbor.rs: Scalar::from_bytes_mod_order) --
// the record handed to k_issue_check, to the signature and to out_req is the one from_cbor returns, so the reduced scalars are
// written back.  Any other code: a zero record, false (the lane is FLAG_UNDECODABLE and does no further work).
ACT_HD bool issue_wire_take_lane(uint8_t* rec, uint8_t code, uint32_t wk[8], sc& gamma, sc& k_bar, sc& r_bar) {
  if (code != CBOR_OK) { for (int i = 0; i < 128; i += 32) zero8(rec + i); return false; }
  load8(wk, rec);
  gamma = load_sc(rec + 32); store_sc(rec + 32, gamma);
  k_bar = load_sc(rec + 64); store_sc(rec + 64, k_bar);
  r_bar = load_sc(rec + 96); store_sc(rec + 96, r_bar);
  return true;
}

// (d) the status of a lane whose message the reader refused: CborError::{Ciborium, InvalidStructure, InvalidValue} as 254 / 253 / 255,
// over whatever the check made of its zero record.  code = CBOR_OK (every canonical lane: the call's code bytes start out zero) keeps stt.
ACT_HD uint8_t issue_wire_status(uint8_t stt, uint8_t code) { return code != CBOR_OK ? cbor_code_status(code) : stt; }

#if defined(__HIPCC__)
void launch_issue_wire_flag(const IssueWireFlagArgs& a, hipStream_t s);
#endif

}  // namespace act
