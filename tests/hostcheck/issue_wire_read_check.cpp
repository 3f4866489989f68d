// issue_wire_read_check.cpp — TEST-ONLY host program: the device road of one IssuanceRequest message (csrc/issue_wire_lanes.h over
// csrc/cbor_lanes.h: flag lane, plain pass, validating pass, take-up, status override) beside its specification, the host road
// (csrc/cbor_reader.h cbor_read_message, the ordering of cbor_settle_codes with the points validated here, decode_scalar), on a
// corpus file.  Built and run by tests/test_issue_wire_read_host.py, plain and under ASan + UBSan; never linked into libact_mi355x.so.
//
//   issue_wire_read_check CORPUS OUT
// CORPUS:  u32 L | u32 ml | ml bytes canonical template | 4 x u32 payload offsets, then messages back to back: u32 len | len bytes.
// OUT: per message  u8 spec flag | u8 lane flag | u8 spec status | u8 lane status | u8 mismatch bits | u8 spec code of cbor_read_message
// alone | u8 spec code after the ordering step | u8 lane info, then the specification's 128-byte record as out_req hands it out (the
// record from_cbor returns, all zero unless the status is 0).
// The status is the one the READ gives: 254 / 253 / 255 for a message that does not read, 255 for a K that does not decode, else 0
// (the proof check that follows is not a matter of reading).
// mismatch bits: 1 flag, 2 status, 4 record as phase A leaves it in staging, 8 record as handed out, 16 code.
// Every message and every record lives in a heap block of exactly its size, so that a sanitizer sees any access beyond it.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>
#include "../../anonymous-credit-tokens_amd/csrc/issue_wire_lanes.h"

using namespace act;

static bool point_ok(const uint8_t* p) { uint32_t w[8]; memcpy(w, p, 32); ge P; return ristretto_decode(P, w); }

struct Verdict { uint8_t flag, status, plain, code, info; uint8_t staged[128], out[128]; };

// the specification: issue_cbor_tiny's template compare for the flag; issue_wire_settle for the rest
static Verdict spec(const CborType& T, int L, const uint8_t* msg, size_t len, const std::vector<uint8_t>& tmpl, const uint32_t pay_off[4]) {
  Verdict v{};
  bool canon = len >= tmpl.size();
  for (size_t f = 0, prev = 0; canon && f < 4; prev = pay_off[f] + 32, f++) if (memcmp(msg + prev, tmpl.data() + prev, pay_off[f] - prev)) canon = false;
  v.flag = canon ? 0 : 0x80;
  CborCand cc;
  int code = cbor_read_message(T, L, msg, len, v.staged, &cc);
  v.plain = (uint8_t)code;
  const bool need = (code == CBOR_ERR_STRUCTURE && !cc.pts.empty()) || (code == CBOR_OK && cc.irregular);
  if (need) for (size_t i = 0; i + 32 <= cc.pts.size(); i += 32) if (!point_ok(cc.pts.data() + i)) { code = CBOR_ERR_VALUE; break; }
  v.code = (uint8_t)code;
  if (code != CBOR_OK) memset(v.staged, 0, 128);
  else for (int f = 1; f < 4; f++) { uint32_t w[8]; memcpy(w, v.staged + 32 * f, 32); const sc s = sc_from_words(w); memcpy(v.staged + 32 * f, s.v, 32); }      // decode_scalar
  v.status = code == CBOR_ERR_PARSE ? 254 : code == CBOR_ERR_STRUCTURE ? 253 : code == CBOR_ERR_VALUE ? 255 : point_ok(v.staged) ? 0 : 255;
  if (v.status == 0) memcpy(v.out, v.staged, 128);
  return v;
}

// the device road, one message as a launch of one lane
static Verdict lanes(const CborType& T, int L, const uint8_t* msg, size_t len, const std::vector<uint8_t>& tmpl, const uint32_t pay_off[4]) {
  Verdict v{};
  const uint64_t off[2] = {0, (uint64_t)len};
  uint8_t flag = 0x55, code = 0, info = 0;                    // (the call's code and info bytes start out zero; the flag pass writes every flag)
  IssueWireFlagArgs fa{1, 0, (uint32_t)tmpl.size(), msg, off, tmpl.data(), pay_off, &flag};
  issue_wire_flag_lane(fa, 0);
  v.flag = flag;
  std::unique_ptr<uint8_t[]> rec(new uint8_t[128]);
  memset(rec.get(), 0xA5, 128);                               // the road must write or zero every field itself
  std::unique_ptr<uint32_t[]> st(new uint32_t[CBOR_MAX_DEPTH]);
  CborReadArgs ra{};
  ra.T = T; ra.L = L; ra.n = 1; ra.first = 0; ra.msg_len = (uint32_t)tmpl.size(); ra.in = msg; ra.offsets = off; ra.flags = &flag;
  ra.rec = rec.get(); ra.rec_stride = 128; ra.keep_fields = 4; ra.code = &code; ra.info = &info;
  cbor_read_message_lane<false>(ra, 0, st.get());
  v.plain = code;
  cbor_read_message_lane<true>(ra, 0, st.get());
  v.code = code; v.info = info;
  uint32_t wk[8]; sc gamma, k_bar, r_bar;
  bool live = true;
  if (flag & 0x80) live = issue_wire_take_lane(rec.get(), code, wk, gamma, k_bar, r_bar);
  else issue_wire_take_canonical(msg, pay_off, rec.get(), wk, gamma, k_bar, r_bar);
  uint8_t stt = 255;                                          // FLAG_UNDECODABLE as k_issue_check reports it
  if (live) { ge K; stt = ristretto_decode(K, wk) ? 0 : 255; }
  v.status = issue_wire_status(stt, code);
  memcpy(v.staged, rec.get(), 128);
  if (v.status == 0) memcpy(v.out, rec.get(), 128);           // k_issue_req_out
  return v;
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: issue_wire_read_check CORPUS OUT\n"); return 2; }
  FILE* in = fopen(argv[1], "rb"); FILE* out = fopen(argv[2], "wb");
  if (!in || !out) { fprintf(stderr, "cannot open files\n"); return 2; }
  uint32_t hd[2], pay_off[4];
  if (fread(hd, 4, 2, in) != 2 || hd[0] < 1 || hd[0] > 4096 || hd[1] < 4 * 33 || hd[1] > 4096) { fprintf(stderr, "bad corpus header\n"); return 2; }
  const int L = (int)hd[0];
  std::vector<uint8_t> tmpl(hd[1]);
  if (fread(tmpl.data(), 1, tmpl.size(), in) != tmpl.size() || fread(pay_off, 4, 4, in) != 4) { fprintf(stderr, "short corpus header\n"); return 2; }
  for (int f = 0; f < 4; f++) if (pay_off[f] + 32 > tmpl.size() || (f && pay_off[f] < pay_off[f - 1] + 32)) { fprintf(stderr, "bad payload offsets\n"); return 2; }
  const CborType* T = cbor_type(1);                           // ACT_CBOR_ISSUANCE_REQUEST
  if (!T || cbor_field_count(*T, L) != 4) { fprintf(stderr, "no IssuanceRequest type\n"); return 2; }
  size_t count = 0, bad = 0;
  for (;;) {
    uint32_t len;
    if (fread(&len, 4, 1, in) != 1) break;
    std::unique_ptr<uint8_t[]> msg(new uint8_t[len]);
    if (len && fread(msg.get(), 1, len, in) != len) { fprintf(stderr, "short corpus\n"); return 2; }
    const Verdict s = spec(*T, L, msg.get(), len, tmpl, pay_off), l = lanes(*T, L, msg.get(), len, tmpl, pay_off);
    uint8_t mis = 0;
    if (s.flag != l.flag) mis |= 1;
    if (s.status != l.status) mis |= 2;
    if (memcmp(s.staged, l.staged, 128)) mis |= 4;
    if (memcmp(s.out, l.out, 128)) mis |= 8;
    if (s.code != l.code) mis |= 16;
    const uint8_t o[8] = {s.flag, l.flag, s.status, l.status, mis, s.plain, s.code, l.info};
    fwrite(o, 1, 8, out); fwrite(s.out, 1, 128, out);
    if (mis) { bad++; if (bad <= 10) fprintf(stderr, "message %zu (%u bytes): flag %u/%u status %u/%u code %u/%u mismatch %u\n", count, len, s.flag, l.flag, s.status, l.status, s.code, l.code, mis); }
    count++;
  }
  fclose(in); fclose(out);
  printf("ISSUE WIRE READ CHECK: %zu messages, %zu mismatches\n", count, bad);
  return bad ? 1 : 0;
}
