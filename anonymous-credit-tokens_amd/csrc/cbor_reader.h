// cbor_reader.h — the general RFC 8949 reader of the codec as plain C++ (no HIP): the nine message types of src/cbor.rs as a table and
// cbor_read_message, which mirrors from_cbor on every input ciborium accepts or refuses.  It is the SPECIFICATION of the device reader
// (cbor_lanes.h: the same reader as a lane body without recursion or allocation; tests/hostcheck/cbor_read_check.cpp compiles both
// and compares code and record on every input) and the reader of the calls that still parse on the host: act_cbor_decode_batch, the
// issuance wire calls, and the spend wire path under ACT_WIRE_READER_HOST.  Included by cbor_impl.inc (engine.hip) and by cbor_lanes.h.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>

enum { CBOR_S = 0, CBOR_P = 1 };                 // field kinds
enum { CBOR_OK = 0, CBOR_ERR_PARSE = 1, CBOR_ERR_STRUCTURE = 2, CBOR_ERR_VALUE = 3 };

struct CborEntry { int key; int kind; int shape; };   // shape: 0 single, 1 array[L], 2 array[L] of pairs
struct CborType { int n_entries; CborEntry e[17]; bool bare; };

inline const CborType* cbor_type(int t) {
  static const CborType T[11] = {
    {0, {}, false},
    /* 1 IssuanceRequest  */ {4, {{1, CBOR_P, 0}, {2, CBOR_S, 0}, {3, CBOR_S, 0}, {4, CBOR_S, 0}}, false},
    /* 2 IssuanceResponse */ {5, {{1, CBOR_P, 0}, {2, CBOR_S, 0}, {3, CBOR_S, 0}, {4, CBOR_S, 0}, {5, CBOR_S, 0}}, false},
    /* 3 SpendProof       */ {17, {{1, CBOR_S, 0}, {2, CBOR_S, 0}, {3, CBOR_P, 0}, {4, CBOR_P, 0}, {5, CBOR_P, 1}, {6, CBOR_S, 0}, {7, CBOR_S, 0},
                                   {8, CBOR_S, 0}, {9, CBOR_S, 0}, {10, CBOR_S, 0}, {11, CBOR_S, 0}, {12, CBOR_S, 0}, {13, CBOR_S, 0}, {14, CBOR_S, 1},
                                   {15, CBOR_S, 2}, {16, CBOR_S, 0}, {17, CBOR_S, 0}}, false},
    /* 4 Refund           */ {4, {{1, CBOR_P, 0}, {2, CBOR_S, 0}, {3, CBOR_S, 0}, {4, CBOR_S, 0}}, false},
    /* 5 PrivateKey       */ {2, {{1, CBOR_S, 0}, {2, CBOR_P, 0}}, false},
    /* 6 PublicKey        */ {1, {{0, CBOR_P, 0}}, true},
    /* 7 PreIssuance      */ {2, {{1, CBOR_S, 0}, {2, CBOR_S, 0}}, false},
    /* 8 CreditToken      */ {5, {{1, CBOR_P, 0}, {2, CBOR_S, 0}, {3, CBOR_S, 0}, {4, CBOR_S, 0}, {5, CBOR_S, 0}}, false},
    /* 9 PreRefund        */ {3, {{1, CBOR_S, 0}, {2, CBOR_S, 0}, {3, CBOR_S, 0}}, false},
    /* 10 RefundReturn: Refund's map with a fifth entry, key 5 -> the returned amount t (not a type of src/cbor.rs) */
                             {5, {{1, CBOR_P, 0}, {2, CBOR_S, 0}, {3, CBOR_S, 0}, {4, CBOR_S, 0}, {5, CBOR_S, 0}}, false},
  };
  return (t >= 1 && t <= 10) ? &T[t] : nullptr;
}

// ---- general RFC 8949 reader (host) ----------------------------------------------------------------------
struct CborReader {
  const uint8_t* p; size_t n, pos; int depth;
  bool head(int& major, uint64_t& val, bool& indefinite) {
    if (pos >= n) return false;
    uint8_t b = p[pos++]; major = b >> 5; int ai = b & 31; indefinite = false;
    if (ai < 24) { val = (uint64_t)ai; return true; }
    if (ai == 31) { if (major == 0 || major == 1 || major == 6) return false; indefinite = true; val = 0; return true; }
    if (ai > 27) return false;
    int len = 1 << (ai - 24);
    if (pos + (size_t)len > n) return false;
    val = 0; for (int i = 0; i < len; i++) val = val << 8 | p[pos++];
    return true;
  }
  bool is_break() const { return pos < n && p[pos] == 0xFF; }
  // well-formed UTF-8 (RFC 3629: no overlongs, no surrogates, <= U+10FFFF): ciborium rejects text strings that are not
  static bool utf8_ok(const uint8_t* s, size_t len) {
    size_t i = 0;
    while (i < len) {
      const uint8_t b = s[i];
      size_t need; uint32_t cp;
      if (b < 0x80) { i++; continue; }
      else if ((b & 0xE0) == 0xC0) { need = 1; cp = b & 0x1F; }
      else if ((b & 0xF0) == 0xE0) { need = 2; cp = b & 0x0F; }
      else if ((b & 0xF8) == 0xF0) { need = 3; cp = b & 0x07; }
      else return false;
      if (len - i <= need) return false;                        // truncated sequence
      for (size_t k = 1; k <= need; k++) { const uint8_t c = s[i + k]; if ((c & 0xC0) != 0x80) return false; cp = (cp << 6) | (c & 0x3F); }
      if ((need == 1 && cp < 0x80) || (need == 2 && cp < 0x800) || (need == 3 && cp < 0x10000) || cp > 0x10FFFF || (cp >= 0xD800 && cp <= 0xDFFF)) return false;
      i += need + 1;
    }
    return true;
  }
  // reads a (possibly chunked) byte/text string into out (if non-null)
  bool string_body(int major, uint64_t val, bool indefinite, std::vector<uint8_t>* out) {
    if (!indefinite) {
      if (val > n - pos) return false;
      if (major == 3 && !utf8_ok(p + pos, (size_t)val)) return false;
      if (out) out->insert(out->end(), p + pos, p + pos + val);
      pos += (size_t)val; return true;
    }
    for (;;) {
      if (pos >= n) return false;
      if (is_break()) { pos++; return true; }
      int m2; uint64_t v2; bool ind2;
      if (!head(m2, v2, ind2) || m2 != major || ind2) return false;
      if (v2 > n - pos) return false;
      if (major == 3 && !utf8_ok(p + pos, (size_t)v2)) return false;      // every chunk of a text string is valid UTF-8 on its own
      if (out) out->insert(out->end(), p + pos, p + pos + v2);
      pos += (size_t)v2;
    }
  }
  bool skip() {                                   // one complete data item
    if (++depth > 256) return false;
    int major; uint64_t val; bool ind;
    if (!head(major, val, ind)) return false;
    bool ok = true;
    switch (major) {
      case 0: case 1: break;
      case 2: case 3: ok = string_body(major, val, ind, nullptr); break;
      case 4: case 5: {
        uint64_t items = major == 5 ? 2 : 1;
        if (ind) { for (;;) { if (pos >= n) { ok = false; break; } if (is_break()) { pos++; break; } for (uint64_t k = 0; k < items && ok; k++) ok = skip(); if (!ok) break; } }
        else { if (val > (n - pos)) { ok = false; break; } for (uint64_t i = 0; i < val * items && ok; i++) ok = skip(); }
        break;
      }
      case 6: ok = skip(); break;
      case 7: if (ind) ok = false; break;         // a stray break; floats / simple values carry no further bytes
    }
    depth--;
    return ok;
  }
};

// value at the reader = 32-byte byte string?  0 yes (copied to out), 2 structural mismatch, 1 malformed
inline int cbor_read_bstr32(CborReader& r, uint8_t out[32]) {
  size_t save = r.pos; int major; uint64_t val; bool ind;
  if (!r.head(major, val, ind)) return CBOR_ERR_PARSE;
  if (major != 2) { r.pos = save; return r.skip() ? CBOR_ERR_STRUCTURE : CBOR_ERR_PARSE; }
  std::vector<uint8_t> b;
  if (!r.string_body(2, val, ind, &b)) return CBOR_ERR_PARSE;
  if (b.size() != 32) return CBOR_ERR_STRUCTURE;                               // "expected 32-byte array"
  memcpy(out, b.data(), 32);
  return CBOR_OK;
}
// array of `count` elements read by `elem`; ciborium parses the whole value before the codec looks at it, so a
// malformed tail is a parse error even if the shape is already wrong
template <class F>
int cbor_read_array(CborReader& r, size_t count, bool* was_array, F&& elem) {
  size_t save = r.pos; int major; uint64_t val; bool ind;
  if (!r.head(major, val, ind)) return CBOR_ERR_PARSE;
  if (major != 4) { r.pos = save; *was_array = false; return r.skip() ? CBOR_OK : CBOR_ERR_PARSE; }   // not an array: field silently absent
  *was_array = true;
  // every element is decoded, in order, BEFORE the length is looked at (src/cbor.rs:307-319: collect::<Result<Vec<_>, _>>()? and only
  // then `len() == L`): `elem` also sees the indices >= count of an over-long array (it must not store those) until one fails
  size_t got = 0; int first_err = CBOR_OK;
  auto one = [&]() -> bool {
    size_t s2 = r.pos;
    if (first_err == CBOR_OK) { int e = elem(got); if (e == CBOR_ERR_PARSE) return false; if (e != CBOR_OK) first_err = e; }
    else { r.pos = s2; if (!r.skip()) return false; }
    got++; return true;
  };
  if (ind) { for (;;) { if (r.pos >= r.n) return CBOR_ERR_PARSE; if (r.is_break()) { r.pos++; break; } if (!one()) return CBOR_ERR_PARSE; } }
  else { if (val > r.n - r.pos) return CBOR_ERR_PARSE; for (uint64_t i = 0; i < val; i++) if (!one()) return CBOR_ERR_PARSE; }
  if (first_err != CBOR_OK) return first_err;
  return got == count ? CBOR_OK : CBOR_ERR_STRUCTURE;                        // "... array wrong size"
}

// from_cbor returns the FIRST failure in wire order (src/cbor.rs:276-388: `?` inside `for (key, val) in map`), and a point is
// validated where it is read (decode_point, :62-77).  The reader does not validate points (the GPU does), so it hands back what
// the order depends on: `pts` = every point value read, in wire order, up to the reader's own return -- including values a later
// duplicate key overwrites and the elements beyond L of an over-long array, which never reach the record -- and `irregular` = some
// of them are not in the record.  The caller has the GPU validate `pts` when the reader stopped at a structural fault (an invalid
// point in front of it is what the crate reports: InvalidValue) or when `irregular` (cbor_settle_codes below).
struct CborCand { std::vector<uint8_t> pts; bool irregular = false; };

// one message -> raw record (fields left unreduced / unvalidated: the GPU pass does that).  Mirrors from_cbor.
inline int cbor_read_message(const CborType& T, int L, const uint8_t* msg, size_t len, uint8_t* rec, CborCand* cc = nullptr) {
  CborReader r{msg, len, 0, 0};
  if (T.bare) return cbor_read_bstr32(r, rec);                                  // PublicKey (src/cbor.rs:529-534)
  // ciborium::from_reader parses the complete first item before the codec inspects it
  { CborReader probe{msg, len, 0, 0}; if (!probe.skip()) return CBOR_ERR_PARSE; }
  int major; uint64_t val; bool ind;
  if (!r.head(major, val, ind)) return CBOR_ERR_PARSE;
  if (major != 5) return CBOR_ERR_STRUCTURE;                                    // "expected CBOR map"
  std::vector<int> first(T.n_entries); int nf = 0;
  for (int i = 0; i < T.n_entries; i++) { first[i] = nf; nf += T.e[i].shape == 0 ? 1 : T.e[i].shape == 1 ? L : 2 * L; }
  std::vector<uint8_t> present(T.n_entries, 0);
  uint64_t remaining = val;
  for (;;) {
    if (ind) { if (r.is_break()) break; } else if (remaining-- == 0) break;
    // key: only (unsigned) integers can match; everything else is skipped
    size_t save = r.pos; int km; uint64_t kv; bool kind_;
    if (!r.head(km, kv, kind_)) return CBOR_ERR_PARSE;
    int ent = -1;
    if (km == 0) { for (int i = 0; i < T.n_entries; i++) if ((uint64_t)T.e[i].key == kv) ent = i; }
    else { r.pos = save; if (!r.skip()) return CBOR_ERR_PARSE; }
    if (ent < 0) { if (!r.skip()) return CBOR_ERR_PARSE; continue; }
    uint8_t* dst = rec + 32 * (size_t)first[ent];
    int e;
    const bool is_point = T.e[ent].kind == CBOR_P;
    if (T.e[ent].shape == 0) {
      e = cbor_read_bstr32(r, dst); if (e) return e;
      if (is_point && cc) { cc->pts.insert(cc->pts.end(), dst, dst + 32); if (present[ent]) cc->irregular = true; }
      present[ent] = 1;
    } else {
      bool was_array = true;
      if (T.e[ent].shape == 1) e = cbor_read_array(r, (size_t)L, &was_array, [&](size_t j) {
        uint8_t over[32];
        uint8_t* d = j < (size_t)L ? dst + 32 * j : over;
        const int be = cbor_read_bstr32(r, d);
        if (be == CBOR_OK && is_point && cc) { cc->pts.insert(cc->pts.end(), d, d + 32); if (j >= (size_t)L || present[ent]) cc->irregular = true; }
        return be;
      });
      else e = cbor_read_array(r, (size_t)L, &was_array, [&](size_t j) {
        // z pair: an array of exactly two byte strings (src/cbor.rs:351-367; the pair's length is looked at before its elements)
        bool pair_arr = true; uint8_t tmp[64], over[32];
        int pe = cbor_read_array(r, 2, &pair_arr, [&](size_t k) { return cbor_read_bstr32(r, k < 2 ? tmp + 32 * k : over); });
        if (!pair_arr) return (int)CBOR_ERR_STRUCTURE;                          // "expected array for z pair"
        if (pe) return pe;                                                      // "z pair wrong size" / bad element
        if (j < (size_t)L) memcpy(dst + 64 * j, tmp, 64);
        return (int)CBOR_OK;
      });
      if (e) return e;
      if (was_array) present[ent] = 1;
    }
  }
  for (int i = 0; i < T.n_entries; i++) if (!present[i]) return CBOR_ERR_STRUCTURE;   // "missing field i"
  return CBOR_OK;
}
