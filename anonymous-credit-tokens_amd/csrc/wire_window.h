// wire_window.h — one window of the host reader's road (ACT_WIRE_READER_HOST) as plain C++ (no HIP), beside cbor_reader.h: what the
// spend, admission and issuance settles share and what touches no GPU.  A window is at most WIRE_SETTLE_WINDOW flagged messages
// which[0..cnt), in lane order: the gather plan says which bytes to bring to the host, wire_window_parse reads them with
// cbor_read_message, and the lane-patch plan says how a caller's array is rewritten over the window's lanes.  The copies themselves
// are the caller's: hipMemcpy in the engine (cbor_impl.inc: wire_window_read, wire_patch_lanes), memcpy in
// tests/hostcheck/wire_window_check.cpp.  Nothing here locks or knows a context.
#pragma once
#include "cbor_reader.h"

// Untrusted clients choose the encoding, so there can be two flagged messages at the ends of a 2^20-message batch or a million of
// them: they are settled in windows, and the host never holds more than one window of bytes and records.
constexpr size_t WIRE_SETTLE_WINDOW = 4096;

// where message i lies in the caller's bytes: offsets[i] .. offsets[i + 1], or a fixed length ml without a table
struct WireExtent {
  const uint8_t* cbor; const uint64_t* offsets; size_t ml;
  size_t beg(size_t i) const { return offsets ? (size_t)offsets[i] : i * ml; }
  size_t end(size_t i) const { return offsets ? (size_t)offsets[i + 1] : (i + 1) * ml; }
};

// The window's bytes on the host: one copy of the span that holds the messages when they lie close together (span <= 2 * sum of their
// lengths + 2^20), one copy per message when they do not.  at[k] = where message which[k] starts among the `bytes` gathered.
struct WireCopy { size_t src, len, dst; };            // src: offset in the caller's bytes; dst: offset in the gathered ones
struct WireGather { std::vector<WireCopy> copies; std::vector<size_t> at; size_t bytes = 0; };
inline void wire_gather_plan(const WireExtent& x, const size_t* which, size_t cnt, WireGather& g) {
  g.copies.clear(); g.at.assign(cnt, 0); g.bytes = 0;
  if (!cnt) return;
  size_t sum = 0;
  for (size_t k = 0; k < cnt; k++) sum += x.end(which[k]) - x.beg(which[k]);
  const size_t span_beg = x.beg(which[0]), span_end = x.end(which[cnt - 1]);      // offsets are monotone (every call checks)
  if (span_end - span_beg <= 2 * sum + ((size_t)1 << 20)) {
    g.bytes = span_end - span_beg;
    g.copies.push_back({span_beg, g.bytes, 0});
    for (size_t k = 0; k < cnt; k++) g.at[k] = x.beg(which[k]) - span_beg;
  } else {
    for (size_t k = 0; k < cnt; k++) {
      const size_t b = x.beg(which[k]), l = x.end(which[k]) - b;
      g.copies.push_back({b, l, g.bytes});
      g.at[k] = g.bytes; g.bytes += l;
    }
  }
}
// copy(dst, src offset, len) -> 0 or the error that ends the gather; dst has g.bytes bytes
template <class Copy>
int wire_gather_run(const WireGather& g, uint8_t* dst, Copy&& copy) {
  for (const WireCopy& cp : g.copies) if (cp.len) { const int rc = copy(dst + cp.dst, cp.src, cp.len); if (rc) return rc; }
  return 0;
}

// Message which[k] -> codes[k], cands[k] and the raw record recs[k * rb ...]; a record that did not read is left all zero.  `bytes`:
// the gathered bytes (with at[]), or null for a caller whose messages are host memory and are read where they lie.
inline void wire_window_parse(const CborType& T, int L, const WireExtent& x, const size_t* which, size_t cnt, const uint8_t* bytes, const std::vector<size_t>& at,
                              size_t rb, std::vector<uint8_t>& recs, std::vector<int>& codes, std::vector<CborCand>& cands) {
  recs.assign(cnt * rb, 0); codes.assign(cnt, CBOR_OK); cands.assign(cnt, CborCand{});
  for (size_t k = 0; k < cnt; k++) {
    const size_t beg = x.beg(which[k]), end = x.end(which[k]);
    codes[k] = cbor_read_message(T, L, bytes ? bytes + at[k] : x.cbor + beg, end - beg, recs.data() + k * rb, &cands[k]);
    if (codes[k] != CBOR_OK) memset(recs.data() + k * rb, 0, rb);
  }
}

// Lanes lanes[0..cnt) (ascending) of a caller's array of `stride`-byte entries take vals[k * stride ...]: a dense window
// (span <= 2 * cnt + 64 lanes) as one read-modify-write of its lane span, a sparse one (two messages at the two ends of a large
// batch) lane by lane.  rd(dst, byte offset, len) and wr(byte offset, src, len) -> 0 or the error that ends the patch.
// span_only: the span whatever the lanes (the spend settle: see verify_spend_cbor_impl).
template <class Rd, class Wr>
int wire_patch_run(const size_t* lanes, size_t cnt, size_t stride, const uint8_t* vals, Rd&& rd, Wr&& wr, bool span_only = false) {
  if (!cnt) return 0;
  const size_t first = lanes[0], span = lanes[cnt - 1] - first + 1;
  if (span_only || span <= 2 * cnt + 64) {
    std::vector<uint8_t> h(span * stride);
    if (const int rc = rd(h.data(), first * stride, h.size())) return rc;
    for (size_t k = 0; k < cnt; k++) memcpy(h.data() + (lanes[k] - first) * stride, vals + k * stride, stride);
    return wr(first * stride, h.data(), h.size());
  }
  for (size_t k = 0; k < cnt; k++) if (const int rc = wr(lanes[k] * stride, vals + k * stride, stride)) return rc;
  return 0;
}
