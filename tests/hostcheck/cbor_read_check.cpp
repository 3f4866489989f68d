// cbor_read_check.cpp — TEST-ONLY host program: the device reader's lane body (csrc/cbor_lanes.h) against its specification, the host
// reader (csrc/cbor_reader.h: cbor_read_message, then what cbor_settle_codes does with its candidates), on a corpus file.  Built and
// run by tests/test_cbor_read_host.py, plain and under ASan + UBSan; never linked into libact_mi355x.so.
//
//   cbor_read_check CORPUS OUT
// CORPUS: messages back to back, each  u32 type | u32 L | u32 len | len bytes  (little endian).
// OUT: per message  u8 host code | u8 lane code | u8 mismatch bits | u8 info | record (32 * fields bytes: the host reader's, scalars
// reduced, all zero when the code is not 0) -- the codes are final: CBOR_ERR_VALUE includes a record point that does not decode.
// mismatch bits: 1 code, 2 raw record, 4 final record, 8 keep_fields = 2 differs from the full read, 16 validation demanded differently,
// 32 the wire nullifier of the spend path (the two kernel lane bodies with keep_k_on_value) is not the one the host road hands out.
// Every message and every record lives in a heap block of exactly its size, so that a sanitizer sees any access beyond it.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>
#include "../../anonymous-credit-tokens_amd/csrc/cbor_lanes.h"

using namespace act;

static bool point_ok(const uint8_t* p) { uint32_t w[8]; memcpy(w, p, 32); ge P; return ristretto_decode(P, w); }

// the specification: cbor_read_message, then cbor_settle_codes with the point check on the host.  rec: zero on failure.
static int host_read(const CborType& T, int L, const uint8_t* msg, size_t len, uint8_t* rec, size_t rb, bool* wanted_validation) {
  CborCand cc;
  memset(rec, 0, rb);
  int code = cbor_read_message(T, L, msg, len, rec, &cc);
  const bool need = (code == CBOR_ERR_STRUCTURE && !cc.pts.empty()) || (code == CBOR_OK && cc.irregular);
  *wanted_validation = need;
  if (need) for (size_t i = 0; i + 32 <= cc.pts.size(); i += 32) if (!point_ok(cc.pts.data() + i)) { code = CBOR_ERR_VALUE; break; }
  if (code != CBOR_OK) memset(rec, 0, rb);
  return code;
}
static int lane_read(const CborType& T, int L, const uint8_t* msg, size_t len, uint8_t* rec, uint32_t keep, uint8_t* info_out, bool* wanted_validation) {
  std::unique_ptr<uint32_t[]> st(new uint32_t[CBOR_MAX_DEPTH]);
  uint8_t info = 0;
  int code = cbor_read_lane<false>(T, L, msg, len, rec, keep, st.get(), &info);
  *wanted_validation = cbor_needs_validation(code, info);
  if (*wanted_validation) code = cbor_read_lane<true>(T, L, msg, len, rec, keep, st.get(), nullptr);
  *info_out = info;
  return code;
}
// scalars reduced, record points validated: act_cbor_decode_batch's second pass, written out plainly for the host reader's record
static int host_fix(const CborType& T, int L, int code, uint8_t* rec, size_t nf) {
  if (code != CBOR_OK) return code;
  std::vector<uint8_t> kind;
  if (T.bare) kind.push_back((uint8_t)T.e[0].kind);
  else for (int i = 0; i < T.n_entries; i++) kind.insert(kind.end(), T.e[i].shape == 0 ? 1 : T.e[i].shape == 1 ? L : 2 * L, (uint8_t)T.e[i].kind);
  for (size_t f = 0; f < nf; f++) {
    if (kind[f] == CBOR_S) { uint32_t w[8]; memcpy(w, rec + 32 * f, 32); const sc s = sc_from_words(w); memcpy(rec + 32 * f, s.v, 32); }
    else if (!point_ok(rec + 32 * f)) code = CBOR_ERR_VALUE;
  }
  if (code != CBOR_OK) memset(rec, 0, nf * 32);
  return code;
}
// the same through the lane bodies of k_cbor_read_fix / k_cbor_read_zero (one message: its code byte in a padded word)
static int lane_fix(const CborType& T, int L, int code, uint8_t* rec, size_t nf) {
  std::vector<uint8_t> kind;
  if (T.bare) kind.push_back((uint8_t)T.e[0].kind);
  else for (int i = 0; i < T.n_entries; i++) kind.insert(kind.end(), T.e[i].shape == 0 ? 1 : T.e[i].shape == 1 ? L : 2 * L, (uint8_t)T.e[i].kind);
  alignas(4) uint8_t cw[4] = {(uint8_t)code, 0, 0, 0};
  CborFixArgs a{1, (uint32_t)nf, kind.data(), rec, cw};
  for (uint64_t g = 0; g < (nf + 255) / 256 * 256; g++) cbor_fix_field_lane(a, g);
  for (uint64_t g = 0; g < (nf + 255) / 256 * 256; g++) cbor_zero_failed_lane(a, g);
  return cw[0];
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: cbor_read_check CORPUS OUT\n"); return 2; }
  FILE* in = fopen(argv[1], "rb"); FILE* out = fopen(argv[2], "wb");
  if (!in || !out) { fprintf(stderr, "cannot open files\n"); return 2; }
  size_t count = 0, bad = 0;
  for (;;) {
    uint32_t hd[3];
    if (fread(hd, 4, 3, in) != 3) break;
    const CborType* T = cbor_type((int)hd[0]);
    const int L = (int)hd[1]; const size_t len = hd[2];
    if (!T || L < 1 || L > 4096) { fprintf(stderr, "bad corpus header at message %zu\n", count); return 2; }
    std::unique_ptr<uint8_t[]> msg(new uint8_t[len]);
    if (len && fread(msg.get(), 1, len, in) != len) { fprintf(stderr, "short corpus\n"); return 2; }
    const size_t nf = cbor_field_count(*T, L), rb = nf * 32;
    std::unique_ptr<uint8_t[]> hrec(new uint8_t[rb]), lrec(new uint8_t[rb]);
    memset(lrec.get(), 0xA5, rb);                             // the lane must write or zero every field itself
    bool hv = false, lv = false, kv = false; uint8_t info = 0, kinfo = 0;
    int hc = host_read(*T, L, msg.get(), len, hrec.get(), rb, &hv);
    int lc = lane_read(*T, L, msg.get(), len, lrec.get(), (uint32_t)nf, &info, &lv);
    uint8_t mis = 0;
    if (hc != lc) mis |= 1;
    if (memcmp(hrec.get(), lrec.get(), rb)) mis |= 2;
    if (hv != lv) mis |= 16;
    // the reduced form: fields 0 and 1 only, in a block of exactly that size
    const size_t kf = nf < 2 ? nf : 2;
    std::unique_ptr<uint8_t[]> krec(new uint8_t[kf * 32]);
    memset(krec.get(), 0xA5, kf * 32);
    const int kc = lane_read(*T, L, msg.get(), len, krec.get(), 2, &kinfo, &kv);
    if (kc != lc || kinfo != info || memcmp(krec.get(), lrec.get(), kf * 32)) mis |= 8;
    if (hd[0] == 3) {                                         // SpendProof: the nullifier act_verify_spend_cbor_keys_batch returns for a flagged message
      // host road (verify_spend_cbor_impl): field 0 of the reader's record when cbor_read_message itself returned CBOR_OK, else zero
      std::unique_ptr<uint8_t[]> r0(new uint8_t[rb]); memset(r0.get(), 0, rb);
      CborCand cc0; uint8_t want[32] = {0};
      if (cbor_read_message(*T, L, msg.get(), len, r0.get(), &cc0) == CBOR_OK) memcpy(want, r0.get(), 32);
      std::unique_ptr<uint8_t[]> r1(new uint8_t[rb]); memset(r1.get(), 0xA5, rb);
      std::unique_ptr<uint32_t[]> st(new uint32_t[CBOR_MAX_DEPTH]);
      uint8_t code1 = 0, info1 = 0, flag = 0x80;
      CborReadArgs a{}; a.T = *T; a.L = L; a.n = 1; a.msg_len = (uint32_t)len; a.in = msg.get(); a.flags = &flag; a.rec = r1.get(); a.rec_stride = rb;
      a.keep_fields = (uint32_t)nf; a.keep_k_on_value = 1; a.code = &code1; a.info = &info1;
      cbor_read_message_lane<false>(a, 0, st.get()); cbor_read_message_lane<true>(a, 0, st.get());
      uint8_t got[32]; memcpy(got, r1.get(), 32);
      if (code1 != CBOR_OK && !(info1 & CBOR_INFO_KEPT_K)) memset(got, 0, 32);      // what the settle step does
      if (memcmp(got, want, 32) || code1 != lc) mis |= 32;
      if (code1 != CBOR_OK) for (size_t b = 32; b < rb; b++) if (r1[b]) mis |= 32;      // everything behind field 0 is zero
    }
    hc = host_fix(*T, L, hc, hrec.get(), nf);
    lc = lane_fix(*T, L, lc, lrec.get(), nf);
    if (hc != lc) mis |= 1;
    if (memcmp(hrec.get(), lrec.get(), rb)) mis |= 4;
    const uint8_t o[4] = {(uint8_t)hc, (uint8_t)lc, mis, info};
    fwrite(o, 1, 4, out); fwrite(hrec.get(), 1, rb, out);
    if (mis) { bad++; if (bad <= 10) fprintf(stderr, "message %zu (type %u, L %d, %zu bytes): host %d lane %d mismatch %u\n", count, hd[0], L, len, hc, lc, mis); }
    count++;
  }
  fclose(in); fclose(out);
  printf("CBOR READ CHECK: %zu messages, %zu mismatches\n", count, bad);
  return bad ? 1 : 0;
}
