// cbor_lanes.h — the general RFC 8949 reader as a lane body: one message per lane, no recursion, no allocation (kernels in
// k_cbor_read.hip; the spend_lanes.h / admit_lanes.h pattern: the same functions compile under g++, where
// tests/hostcheck/cbor_read_check.cpp holds them to the host reader on every input).
//
// The specification is cbor_read_message followed by cbor_settle_codes (cbor_reader.h, cbor_impl.inc): the code and the record of
// cbor_read_lane are theirs on every input.  What differs is the form.
//   * CborReader::skip() recurses; cbor_skip() walks an explicit stack of 32-bit frames, one per open container: the items (a map:
//     keys and values) it still has to yield, or a mark for an indefinite one.  skip() refuses the item at nesting depth 257, so the
//     stack holds 256 frames.  A definite count that exceeds the bytes left is refused before the frame is pushed (as skip() does),
//     and a message is at most CBOR_MAX_LEN bytes, so a count -- twice the pair count for a map -- is below the three marks.
//   * std::vector becomes a 32-byte buffer and a length: only a byte string of exactly 32 bytes is ever looked at.
//   * CborCand becomes two bits (CBOR_INFO_IRREGULAR, CBOR_INFO_POINTS) and a second instantiation: cbor_read_lane<true> calls
//     ristretto_decode where decode_point would run and returns CBOR_ERR_VALUE at the first invalid point -- the first failure in
//     wire order, without a candidate list.  Only messages that cbor_needs_validation() names are walked that second time; a regular
//     message that reads cleanly has its points decoded by whoever consumes the record.
//   * keep_fields: only record fields with an index below it are written (admission wants k and s: keep_fields = 2).
// A message that fails leaves its first min(keep_fields, fields) record fields all zero.
#pragma once
#include "kernels.h"
#include "cbor_reader.h"

namespace act {

constexpr uint32_t CBOR_MAX_DEPTH = 256;                      // CborReader::skip(): `++depth > 256`
constexpr uint32_t CBOR_MAX_LEN = 0x7FFFFFFFu;                // bytes of one message that a lane looks at
constexpr uint32_t CBOR_FRAME_ARRAY = 0xFFFFFFFFu;            // indefinite array: an element or the break comes next
constexpr uint32_t CBOR_FRAME_MAP_KEY = 0xFFFFFFFEu;          // indefinite map: a key or the break comes next
constexpr uint32_t CBOR_FRAME_MAP_VALUE = 0xFFFFFFFDu;        // indefinite map: a value comes next (a break here is a stray break)
constexpr uint8_t CBOR_INFO_IRREGULAR = 1, CBOR_INFO_POINTS = 2, CBOR_INFO_KEPT_K = 4, CBOR_INFO_DEVICE = 0x80;      // the per-message info byte

// the cursor of one lane; st = CBOR_MAX_DEPTH words of the lane's own for cbor_skip
struct CborCur { const uint8_t* p; uint32_t n, pos; uint32_t* st; };

ACT_HD bool cborl_head(CborCur& r, int& major, uint64_t& val, bool& indefinite) {
  if (r.pos >= r.n) return false;
  const uint8_t b = r.p[r.pos++]; major = b >> 5; const int ai = b & 31; indefinite = false;
  if (ai < 24) { val = (uint64_t)ai; return true; }
  if (ai == 31) { if (major == 0 || major == 1 || major == 6) return false; indefinite = true; val = 0; return true; }
  if (ai > 27) return false;
  const uint32_t len = 1u << (ai - 24);
  if (len > r.n - r.pos) return false;
  val = 0; for (uint32_t i = 0; i < len; i++) val = val << 8 | r.p[r.pos++];
  return true;
}
ACT_HD bool cborl_is_break(const CborCur& r) { return r.pos < r.n && r.p[r.pos] == 0xFF; }
// CborReader::utf8_ok.  Every turn of the loop moves i forward by at least one byte, and i < len <= bytes left.
ACT_HD bool cborl_utf8_ok(const uint8_t* s, uint32_t len) {
  uint32_t i = 0;
  while (i < len) {
    const uint8_t b = s[i];
    uint32_t need, cp;
    if (b < 0x80) { i++; continue; }
    else if ((b & 0xE0) == 0xC0) { need = 1; cp = b & 0x1F; }
    else if ((b & 0xF0) == 0xE0) { need = 2; cp = b & 0x0F; }
    else if ((b & 0xF8) == 0xF0) { need = 3; cp = b & 0x07; }
    else return false;
    if (len - i <= need) return false;
    for (uint32_t k = 1; k <= need; k++) { const uint8_t c = s[i + k]; if ((c & 0xC0) != 0x80) return false; cp = (cp << 6) | (c & 0x3F); }
    if ((need == 1 && cp < 0x80) || (need == 2 && cp < 0x800) || (need == 3 && cp < 0x10000) || cp > 0x10FFFF || (cp >= 0xD800 && cp <= 0xDFFF)) return false;
    i += need + 1;
  }
  return true;
}
// CborReader::string_body.  w (nullable) receives the bytes of a string of exactly 32 bytes, *total its length whatever it is.
// The chunk loop: every turn reads a head (at least one byte) or the break, then returns or goes on behind the chunk's payload,
// which lies inside the message -- it cannot run more often than the message has bytes.
ACT_HD bool cborl_string(CborCur& r, int major, uint64_t val, bool indefinite, uint32_t* w, uint32_t* total) {
  if (!indefinite) {
    if (val > (uint64_t)(r.n - r.pos)) return false;
    if (major == 3 && !cborl_utf8_ok(r.p + r.pos, (uint32_t)val)) return false;
    if (w && val == 32) load32_bytes(w, r.p + r.pos);
    *total = (uint32_t)val; r.pos += (uint32_t)val; return true;
  }
  uint8_t buf[32]; uint32_t got = 0;
  for (;;) {
    if (r.pos >= r.n) return false;
    if (cborl_is_break(r)) { r.pos++; break; }
    int m2; uint64_t v2; bool ind2;
    if (!cborl_head(r, m2, v2, ind2) || m2 != major || ind2) return false;
    if (v2 > (uint64_t)(r.n - r.pos)) return false;
    if (major == 3 && !cborl_utf8_ok(r.p + r.pos, (uint32_t)v2)) return false;
    if (w) for (uint32_t i = 0; i < (uint32_t)v2 && got + i < 32; i++) buf[got + i] = r.p[r.pos + i];
    got += (uint32_t)v2; r.pos += (uint32_t)v2;      // (the chunks lie one behind the other inside the message: got <= n)
  }
  if (w && got == 32) for (int i = 0; i < 8; i++) w[i] = (uint32_t)buf[4 * i] | (uint32_t)buf[4 * i + 1] << 8 | (uint32_t)buf[4 * i + 2] << 16 | (uint32_t)buf[4 * i + 3] << 24;
  *total = got;
  return true;
}

// CborReader::skip(): one complete data item, nesting counted from the item itself (every skip() call of the host reader starts
// at depth 0 too: the probe's reader and the walking reader are fresh, and a nested value is skipped by a call of its own).
//
// TERMINATION.  One turn of the outer loop does one of three things: (a) it consumes the break of the indefinite container on top
// of the stack (one byte), (b) it reads the head of an item (at least one byte; cborl_head returns false without one), or (c) it
// returns.  So the loop runs at most n times, n <= CBOR_MAX_LEN being the length of the message -- never a number that a length
// field names: a definite container's count is only ever counted DOWN, one per item read, and every item read is a turn that has
// consumed a byte.  The inner `while` pops one frame per turn or leaves, and there are at most CBOR_MAX_DEPTH frames.
ACT_HD bool cbor_skip(CborCur& r) {
  uint32_t sp = 0;                                            // open containers: the next item is at depth sp + 1
  for (;;) {
    bool complete = false;
    if (sp && (r.st[sp - 1] == CBOR_FRAME_ARRAY || r.st[sp - 1] == CBOR_FRAME_MAP_KEY)) {
      if (r.pos >= r.n) return false;
      if (r.p[r.pos] == 0xFF) { r.pos++; sp--; complete = true; }
    }
    if (!complete) {
      if (sp >= CBOR_MAX_DEPTH) return false;                 // `++depth > 256`
      int major; uint64_t val; bool ind;
      if (!cborl_head(r, major, val, ind)) return false;
      switch (major) {
        case 0: case 1: complete = true; break;
        case 2: case 3: { uint32_t total; if (!cborl_string(r, major, val, ind, nullptr, &total)) return false; complete = true; break; }
        case 4: case 5:
          if (ind) r.st[sp++] = major == 5 ? CBOR_FRAME_MAP_KEY : CBOR_FRAME_ARRAY;
          else {
            if (val > (uint64_t)(r.n - r.pos)) return false;  // refused before it is walked: the frame below fits 32 bits
            if (val == 0) complete = true; else r.st[sp++] = (uint32_t)val * (major == 5 ? 2u : 1u);
          }
          break;
        case 6: r.st[sp++] = 1; break;                        // a tag: one item follows
        default: if (ind) return false; complete = true; break;      // 7: a stray break; floats / simple values carry no further bytes
      }
    }
    while (complete) {                                        // the item just finished belongs to the container on top
      if (sp == 0) return true;
      const uint32_t top = r.st[sp - 1];
      if (top == CBOR_FRAME_ARRAY) break;
      if (top == CBOR_FRAME_MAP_KEY) { r.st[sp - 1] = CBOR_FRAME_MAP_VALUE; break; }
      if (top == CBOR_FRAME_MAP_VALUE) { r.st[sp - 1] = CBOR_FRAME_MAP_KEY; break; }
      if (top > 1) { r.st[sp - 1] = top - 1; break; }
      sp--;                                                   // its last item: the container is complete in turn
    }
  }
}

// cbor_read_bstr32: the value at the cursor as a 32-byte byte string -> w
ACT_HD int cborl_bstr32(CborCur& r, uint32_t w[8]) {
  const uint32_t save = r.pos; int major; uint64_t val; bool ind;
  if (!cborl_head(r, major, val, ind)) return CBOR_ERR_PARSE;
  if (major != 2) { r.pos = save; return cbor_skip(r) ? CBOR_ERR_STRUCTURE : CBOR_ERR_PARSE; }
  uint32_t total = 0;
  if (!cborl_string(r, 2, val, ind, w, &total)) return CBOR_ERR_PARSE;
  return total == 32 ? CBOR_OK : CBOR_ERR_STRUCTURE;
}
// cbor_read_array.  Both loops read or skip one element per turn, and an element is at least one byte of the message (a turn that
// finds none returns CBOR_ERR_PARSE): `val` bounds nothing, the bytes left do.
template <class F>
ACT_HD int cborl_array(CborCur& r, uint32_t count, bool* was_array, F&& elem) {
  const uint32_t save = r.pos; int major; uint64_t val; bool ind;
  if (!cborl_head(r, major, val, ind)) return CBOR_ERR_PARSE;
  if (major != 4) { r.pos = save; *was_array = false; return cbor_skip(r) ? CBOR_OK : CBOR_ERR_PARSE; }
  *was_array = true;
  uint32_t got = 0; int first_err = CBOR_OK;
  auto one = [&]() -> bool {
    const uint32_t s2 = r.pos;
    if (first_err == CBOR_OK) { const int e = elem(got); if (e == CBOR_ERR_PARSE) return false; if (e != CBOR_OK) first_err = e; }
    else { r.pos = s2; if (!cbor_skip(r)) return false; }
    got++; return true;
  };
  if (ind) { for (;;) { if (r.pos >= r.n) return CBOR_ERR_PARSE; if (cborl_is_break(r)) { r.pos++; break; } if (!one()) return CBOR_ERR_PARSE; } }
  else { if (val > (uint64_t)(r.n - r.pos)) return CBOR_ERR_PARSE; for (uint64_t i = 0; i < val; i++) if (!one()) return CBOR_ERR_PARSE; }
  if (first_err != CBOR_OK) return first_err;
  return got == count ? CBOR_OK : CBOR_ERR_STRUCTURE;
}

ACT_HD uint32_t cbor_field_count(const CborType& T, int L) {
  if (T.bare) return 1;
  uint32_t nf = 0;
  for (int i = 0; i < T.n_entries; i++) nf += T.e[i].shape == 0 ? 1u : T.e[i].shape == 1 ? (uint32_t)L : 2u * (uint32_t)L;
  return nf;
}
// which messages the validating instantiation has to walk: exactly the two cases of cbor_settle_codes
ACT_HD bool cbor_needs_validation(int code, uint8_t info) {
  return (code == CBOR_ERR_STRUCTURE && (info & CBOR_INFO_POINTS)) || (code == CBOR_OK && (info & CBOR_INFO_IRREGULAR));
}

// cbor_read_message.  VALIDATE = false: the record fields below keep_fields are written as they stand on the wire (scalars not
// reduced, points not decoded), *info takes CBOR_INFO_IRREGULAR / CBOR_INFO_POINTS.  VALIDATE = true: nothing is written on the way,
// every point value is decoded where it is read and the first invalid one ends the walk with CBOR_ERR_VALUE.  Either way a result
// other than CBOR_OK zeroes the record fields below keep_fields.  st: CBOR_MAX_DEPTH words.
// The map loop: every turn reads the head of a key (at least one byte) or returns; `remaining` only ends it earlier.
template <bool VALIDATE>
ACT_HD int cbor_read_walk(const CborType& T, int L, CborCur& r, uint8_t* rec, uint32_t keep_fields, uint8_t* info) {
  auto put = [&](uint32_t field, const uint32_t w[8]) { if (!VALIDATE && field < keep_fields) store32_bytes(rec + (size_t)field * 32, w); };
  auto bad_point = [&](const uint32_t w[8]) { if (!VALIDATE) return false; ge P; return !ristretto_decode(P, w); };
  if (T.bare) {                                               // PublicKey: a bare byte string, never irregular
    uint32_t w[8];
    const int e = cborl_bstr32(r, w);
    if (e == CBOR_OK) { if (T.e[0].kind == CBOR_P && bad_point(w)) return CBOR_ERR_VALUE; put(0, w); }
    return e;
  }
  { CborCur probe = r; if (!cbor_skip(probe)) return CBOR_ERR_PARSE; }      // the complete first item is parsed before anything is looked at
  int major; uint64_t val; bool ind;
  if (!cborl_head(r, major, val, ind)) return CBOR_ERR_PARSE;
  if (major != 5) return CBOR_ERR_STRUCTURE;
  uint32_t present = 0;
  uint64_t remaining = val;
  for (;;) {
    if (ind) { if (cborl_is_break(r)) break; } else if (remaining-- == 0) break;
    const uint32_t save = r.pos; int km; uint64_t kv; bool kind_;
    if (!cborl_head(r, km, kv, kind_)) return CBOR_ERR_PARSE;
    int ent = -1;
    if (km == 0) { for (int i = 0; i < T.n_entries; i++) if ((uint64_t)T.e[i].key == kv) ent = i; }
    else { r.pos = save; if (!cbor_skip(r)) return CBOR_ERR_PARSE; }
    if (ent < 0) { if (!cbor_skip(r)) return CBOR_ERR_PARSE; continue; }
    uint32_t first = 0;
    for (int i = 0; i < ent; i++) first += T.e[i].shape == 0 ? 1u : T.e[i].shape == 1 ? (uint32_t)L : 2u * (uint32_t)L;
    const bool is_point = T.e[ent].kind == CBOR_P, seen = (present >> ent & 1u) != 0;
    if (T.e[ent].shape == 0) {
      uint32_t w[8];
      const int e = cborl_bstr32(r, w); if (e) return e;
      if (is_point) { *info |= CBOR_INFO_POINTS; if (seen) *info |= CBOR_INFO_IRREGULAR; if (bad_point(w)) return CBOR_ERR_VALUE; }
      put(first, w);
      present |= 1u << ent;
    } else {
      bool was_array = true; int e;
      if (T.e[ent].shape == 1) e = cborl_array(r, (uint32_t)L, &was_array, [&](uint32_t j) {
        uint32_t w[8];
        const int be = cborl_bstr32(r, w);
        if (be != CBOR_OK) return be;
        if (is_point) { *info |= CBOR_INFO_POINTS; if (j >= (uint32_t)L || seen) *info |= CBOR_INFO_IRREGULAR; if (bad_point(w)) return (int)CBOR_ERR_VALUE; }
        if (j < (uint32_t)L) put(first + j, w);               // the elements beyond L of an over-long array are read, and never stored
        return (int)CBOR_OK;
      });
      else e = cborl_array(r, (uint32_t)L, &was_array, [&](uint32_t j) {
        bool pair_arr = true; uint32_t tw[2][8];
        const int pe = cborl_array(r, 2, &pair_arr, [&](uint32_t k) {
          uint32_t w[8];
          const int be = cborl_bstr32(r, w);
          if (be == CBOR_OK && k < 2) for (int i = 0; i < 8; i++) tw[k][i] = w[i];
          return be;
        });
        if (!pair_arr) return (int)CBOR_ERR_STRUCTURE;
        if (pe) return pe;
        if (j < (uint32_t)L) { put(first + 2 * j, tw[0]); put(first + 2 * j + 1, tw[1]); }
        return (int)CBOR_OK;
      });
      if (e) return e;
      if (was_array) present |= 1u << ent;
    }
  }
  for (int i = 0; i < T.n_entries; i++) if (!(present >> i & 1u)) return CBOR_ERR_STRUCTURE;      // missing fields are reported last
  return CBOR_OK;
}
template <bool VALIDATE>
ACT_HD int cbor_read_lane(const CborType& T, int L, const uint8_t* msg, uint64_t len, uint8_t* rec, uint32_t keep_fields, uint32_t* st, uint8_t* info,
                          uint32_t zero_from = 0) {
  CborCur r{msg, len > CBOR_MAX_LEN ? CBOR_MAX_LEN : (uint32_t)len, 0, st};
  uint8_t bits = 0;
  const int code = cbor_read_walk<VALIDATE>(T, L, r, rec, keep_fields, &bits);
  if (code != CBOR_OK) {
    const uint32_t nf = cbor_field_count(T, L), z = keep_fields < nf ? keep_fields : nf;
    const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t f = zero_from; f < z; f++) store32_bytes(rec + (size_t)f * 32, zero);
  }
  if (info) *info = bits;
  return code;
}

// ---- argument blocks of the kernels (k_cbor_read.hip) and of the host workers that run the same bodies ------------------------------
struct CborReadArgs {
  CborType T; int L;
  uint32_t n, first;                  // message m of this launch is message first + m of the call: flags / code / info are per call
  uint32_t msg_len;                   // offsets == null: message m = [m * msg_len, (m + 1) * msg_len)
  const uint8_t* in; const uint64_t* offsets;
  const uint8_t* flags;               // nullable: only the messages whose byte has 0x80 set are read (the unframing kernel flagged them)
  uint8_t* rec; uint64_t rec_stride;  // message m's record at rec + m * rec_stride
  uint32_t keep_fields;
  // spend wire path: a message that READ (every field in its record) and whose validating pass then finds an invalid point among the
  // values that are not in the record keeps field 0, the nullifier as it stood on the wire, and is marked CBOR_INFO_KEPT_K -- the
  // host road hands that nullifier out beside status 255, as it does for a regular message with an undecodable point
  uint32_t keep_k_on_value;
  uint8_t* code;                      // CBOR_OK / CBOR_ERR_*
  uint8_t* info;                      // CBOR_INFO_*; CBOR_INFO_DEVICE marks a message this reader has read
};
// the plain pass (VALIDATE = false) and, behind it, the validating pass over the messages the plain pass names
template <bool VALIDATE>
ACT_HD void cbor_read_message_lane(const CborReadArgs& a, uint32_t m, uint32_t* st) {
  if (m >= a.n) return;
  const uint32_t gm = a.first + m;
  if (a.flags && !(a.flags[gm] & 0x80)) return;
  const uint64_t beg = a.offsets ? a.offsets[m] : (uint64_t)m * a.msg_len, end = a.offsets ? a.offsets[m + 1] : beg + a.msg_len;
  uint8_t* rec = a.rec + (uint64_t)m * a.rec_stride;
  if (!VALIDATE) {
    uint8_t info = 0;
    a.code[gm] = (uint8_t)cbor_read_lane<false>(a.T, a.L, a.in + beg, end - beg, rec, a.keep_fields, st, &info);
    a.info[gm] = info | CBOR_INFO_DEVICE;
  } else {
    if (!cbor_needs_validation(a.code[gm], a.info[gm])) return;
    const bool keep_k = a.keep_k_on_value && a.code[gm] == CBOR_OK;
    const int code = cbor_read_lane<true>(a.T, a.L, a.in + beg, end - beg, rec, a.keep_fields, st, nullptr, keep_k ? 1u : 0u);
    a.code[gm] = (uint8_t)code;
    if (keep_k && code != CBOR_OK) a.info[gm] |= CBOR_INFO_KEPT_K;
  }
}

// behind the reader for act_cbor_read_batch: lane = (message, field) of a message that read cleanly -- scalars reduced mod l, points
// validated (CBOR_ERR_VALUE into the message's code byte, 32-bit OR: `code` is padded to a multiple of 4), as k_cbor_unframe does
struct CborFixArgs { uint32_t n, n_fields; const uint8_t* kind; uint8_t* rec; uint8_t* code; };
ACT_HD void cbor_fix_field_lane(const CborFixArgs& a, uint64_t gid) {
  if (gid >= (uint64_t)a.n * a.n_fields) return;
  const uint32_t m = (uint32_t)(gid / a.n_fields), f = (uint32_t)(gid % a.n_fields);
  const uint8_t c = a.code[m];
  if (c == CBOR_ERR_PARSE || c == CBOR_ERR_STRUCTURE) return;      // (CBOR_ERR_VALUE may be another lane of this message speaking: carry on)
  uint8_t* p = a.rec + ((size_t)m * a.n_fields + f) * 32;
  uint32_t w[8];
  load32_bytes(w, p);
  if (a.kind[f] == CBOR_S) { const sc s = sc_from_words(w); store32_bytes(p, s.v); }
  else { ge P; if (!ristretto_decode(P, w)) ACT_FLAG_OR(reinterpret_cast<unsigned int*>(a.code + (m & ~3u)), (unsigned)CBOR_ERR_VALUE << (8 * (m & 3u))); }
}
ACT_HD void cbor_zero_failed_lane(const CborFixArgs& a, uint64_t gid) {
  if (gid >= (uint64_t)a.n * a.n_fields) return;
  const uint32_t m = (uint32_t)(gid / a.n_fields), f = (uint32_t)(gid % a.n_fields);
  if (a.code[m] == CBOR_OK) return;
  const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  store32_bytes(a.rec + ((size_t)m * a.n_fields + f) * 32, zero);
}

// the wire status of a message with a code: what the settle loop of the host road patches in (ACT_STATUS_CBOR_MALFORMED 254,
// ACT_STATUS_CBOR_STRUCTURE 253, ACT_STATUS_UNDECODABLE 255)
ACT_HD uint8_t cbor_code_status(uint8_t code) { return code == CBOR_ERR_PARSE ? 254 : code == CBOR_ERR_STRUCTURE ? 253 : code == CBOR_ERR_VALUE ? 255 : 0; }
// behind the pipeline (device-memory callers): a message the reader refused takes its wire status, all-zero K' and nullifier
// (CBOR_INFO_KEPT_K: the nullifier stays) and ACT_KEY_NONE -- over whatever the verification of its all-zero record wrote.  Nullable: out_kprime, out_nullifier, out_key.
struct CborSettleArgs { uint32_t n; const uint8_t* code; const uint8_t* info; uint8_t* status; uint8_t* out_kprime; uint8_t* out_nullifier; uint8_t* out_key; };
ACT_HD void cbor_settle_lane(const CborSettleArgs& a, uint32_t m) {
  if (m >= a.n || !(a.info[m] & CBOR_INFO_DEVICE) || a.code[m] == CBOR_OK) return;
  a.status[m] = cbor_code_status(a.code[m]);
  if (a.out_kprime) for (int i = 0; i < 32; i++) a.out_kprime[(size_t)m * 32 + i] = 0;
  if (a.out_nullifier && !(a.info[m] & CBOR_INFO_KEPT_K)) for (int i = 0; i < 32; i++) a.out_nullifier[(size_t)m * 32 + i] = 0;
  if (a.out_key) a.out_key[m] = 255;
}
// admission: wire_code[m] for the screen (0 = goes on)
struct CborCodeArgs { uint32_t n; const uint8_t* code; const uint8_t* info; uint8_t* wire_code; };
ACT_HD void cbor_wire_code_lane(const CborCodeArgs& a, uint32_t m) {
  if (m >= a.n) return;
  a.wire_code[m] = (a.info[m] & CBOR_INFO_DEVICE) ? cbor_code_status(a.code[m]) : (uint8_t)0;
}

#if defined(__HIPCC__)
void launch_cbor_read(const CborReadArgs& a, bool validate, hipStream_t s);       // one lane per message
void launch_cbor_fix(const CborFixArgs& a, hipStream_t s);                         // cbor_fix_field_lane, then cbor_zero_failed_lane
void launch_cbor_settle(const CborSettleArgs& a, hipStream_t s);
void launch_cbor_wire_code(const CborCodeArgs& a, hipStream_t s);
#endif

}  // namespace act
