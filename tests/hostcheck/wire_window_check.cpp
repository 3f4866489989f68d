// wire_window_check.cpp — TEST-ONLY host program: the settle window of the host reader's road (csrc/wire_window.h over
// csrc/cbor_reader.h) with memcpy as the copier, out of a "device" buffer allocated at exactly the batch's size, so that a sanitizer
// sees any copy beyond it.  Built and run by tests/test_wire_window_host.py, plain and under ASan + UBSan; never linked into
// libact_mi355x.so.
//
//   wire_window_check [CORPUS]
// (a) the gather plan over synthetic offset tables, (b) the lane patch, (c) with CORPUS (u32 L, then IssuanceRequest messages back to
// back: u32 len | len bytes | u8 code the model expects) the parse step and the status of a code.
#include <cstdio>
#include <cstring>
#include <memory>
#include <numeric>
#include <vector>
#include "../../anonymous-credit-tokens_amd/csrc/wire_window.h"
#include "../../anonymous-credit-tokens_amd/csrc/cbor_lanes.h"          // act::cbor_code_status (the lane headers compile under g++)
#include "../../include/act_mi355x.h"

static size_t failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; fprintf(stderr, "FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

// ---- (a) ----------------------------------------------------------------------------------------------------------------------------
// a batch of messages of the given lengths whose byte j is a function of j, the flagged lanes `which`, in windows: every gathered
// message equals its source bytes, no copy reads outside [beg(first), end(last)), and the copy count is what the rule says
static void gather_case(const char* name, const std::vector<size_t>& len, bool table, const std::vector<size_t>& which, const std::vector<int>& want_copies) {
  const size_t n = len.size();
  std::vector<uint64_t> offs(n + 1, 0);
  for (size_t i = 0; i < n; i++) offs[i + 1] = offs[i] + len[i];
  const size_t total = (size_t)offs[n];
  std::unique_ptr<uint8_t[]> dev(new uint8_t[total ? total : 1]);
  for (size_t j = 0; j < total; j++) dev[j] = (uint8_t)(j * 131 + (j >> 8) * 7 + 3);
  const WireExtent x{dev.get(), table ? offs.data() : nullptr, table ? 0 : len[0]};
  size_t windows = 0;
  for (size_t w0 = 0; w0 < which.size(); w0 += WIRE_SETTLE_WINDOW, windows++) {
    const size_t cnt = std::min(which.size(), w0 + WIRE_SETTLE_WINDOW) - w0;
    const size_t* w = which.data() + w0;
    WireGather g;
    wire_gather_plan(x, w, cnt, g);
    CHECK(g.at.size() == cnt, "%s", name);
    size_t sum = 0;
    for (size_t k = 0; k < cnt; k++) sum += len[w[k]];
    const size_t span_beg = (size_t)offs[w[0]], span_end = (size_t)offs[w[cnt - 1] + 1];
    const bool one = span_end - span_beg <= 2 * sum + ((size_t)1 << 20);
    CHECK(g.copies.size() == (one ? 1 : cnt), "%s: %zu copies for %zu messages", name, g.copies.size(), cnt);
    if (windows < want_copies.size()) CHECK((int)g.copies.size() == want_copies[windows], "%s: window %zu has %zu copies, the case expects %d", name, windows, g.copies.size(), want_copies[windows]);
    CHECK(g.bytes == (one ? span_end - span_beg : sum), "%s: %zu bytes gathered", name, g.bytes);
    std::unique_ptr<uint8_t[]> host(new uint8_t[g.bytes ? g.bytes : 1]);
    const int rc = wire_gather_run(g, host.get(), [&](uint8_t* dst, size_t src, size_t l) -> int {
      CHECK(src >= span_beg && src + l <= span_end, "%s: a copy of [%zu, %zu) leaves the window's span [%zu, %zu)", name, src, src + l, span_beg, span_end);
      CHECK(dst >= host.get() && dst + l <= host.get() + g.bytes, "%s: a copy lands outside the gathered bytes", name);
      memcpy(dst, dev.get() + src, l);
      return 0;
    });
    CHECK(rc == 0, "%s", name);
    for (size_t k = 0; k < cnt; k++) {
      CHECK(g.at[k] + len[w[k]] <= g.bytes, "%s: message %zu lies outside the gathered bytes", name, w[k]);
      CHECK(x.end(w[k]) - x.beg(w[k]) == len[w[k]] && x.beg(w[k]) == (size_t)offs[w[k]], "%s: extent of message %zu", name, w[k]);
      CHECK(memcmp(host.get() + g.at[k], dev.get() + offs[w[k]], len[w[k]]) == 0, "%s: message %zu differs from its source", name, w[k]);
    }
  }
  CHECK(windows == (which.size() + WIRE_SETTLE_WINDOW - 1) / WIRE_SETTLE_WINDOW, "%s", name);
  // a copier that fails ends the gather with its code
  WireGather g;
  wire_gather_plan(x, which.data(), std::min(which.size(), WIRE_SETTLE_WINDOW), g);
  if (g.bytes) { std::vector<uint8_t> h(g.bytes); CHECK(wire_gather_run(g, h.data(), [](uint8_t*, size_t, size_t) { return -7; }) == -7, "%s", name); }
}

static void gather_cases() {
  std::vector<size_t> all4097(4097); std::iota(all4097.begin(), all4097.end(), 0);
  gather_case("adjacent", std::vector<size_t>(10, 141), true, {3, 4, 5}, {1});
  gather_case("adjacent, fixed length", std::vector<size_t>(10, 141), false, {0, 1, 9}, {1});
  // two flagged messages of 100 bytes: span = 200 + between; one copy up to between == 2 * 200 + 2^20 - 200
  const size_t edge = 200 + ((size_t)1 << 20);
  gather_case("span == 2 * sum + 2^20", {100, edge, 100}, true, {0, 2}, {1});
  gather_case("span == 2 * sum + 2^20 + 1", {100, edge + 1, 100}, true, {0, 2}, {2});
  gather_case("fixed length, far apart", std::vector<size_t>(7600, 141), false, {0, 7599}, {2});
  gather_case("fixed length, a window of 4096", std::vector<size_t>(4096, 35), false, std::vector<size_t>(all4097.begin(), all4097.begin() + 4096), {1});
  gather_case("4097 flagged: two windows", std::vector<size_t>(4097, 35), true, all4097, {1, 1});
  gather_case("zero-length messages", {0, 5, 0, 0, 9, 0}, true, {0, 2, 3, 5}, {1});
  gather_case("zero-length messages, far apart", {0, edge, 0, 3}, true, {0, 2, 3}, {3});
  gather_case("nothing but zero-length messages", {0, 0, 0}, true, {0, 1, 2}, {1});
}

// ---- (b) ----------------------------------------------------------------------------------------------------------------------------
static void patch_case(const char* name, size_t n, size_t stride, const std::vector<size_t>& lanes, bool want_dense, bool span_only = false) {
  std::unique_ptr<uint8_t[]> dev(new uint8_t[n * stride]), before(new uint8_t[n * stride]);
  for (size_t j = 0; j < n * stride; j++) before[j] = dev[j] = (uint8_t)(j * 29 + 1);
  std::vector<uint8_t> vals(lanes.size() * stride);
  for (size_t j = 0; j < vals.size(); j++) vals[j] = (uint8_t)(0x80 ^ (j * 53));
  size_t reads = 0, writes = 0, moved = 0;
  const int rc = wire_patch_run(lanes.data(), lanes.size(), stride, vals.data(),
    [&](uint8_t* dst, size_t off, size_t l) -> int { CHECK(off + l <= n * stride, "%s: read beyond the array", name); memcpy(dst, dev.get() + off, l); reads++; moved += l; return 0; },
    [&](size_t off, const uint8_t* src, size_t l) -> int { CHECK(off + l <= n * stride, "%s: write beyond the array", name); memcpy(dev.get() + off, src, l); writes++; moved += l; return 0; }, span_only);
  CHECK(rc == 0, "%s", name);
  const size_t span = lanes.back() - lanes.front() + 1;
  CHECK(span_only || (span <= 2 * lanes.size() + 64) == want_dense, "%s: the case is on the other side of the rule", name);
  if (want_dense) CHECK(reads == 1 && writes == 1 && moved == 2 * span * stride, "%s: %zu reads, %zu writes, %zu bytes", name, reads, writes, moved);
  else CHECK(reads == 0 && writes == lanes.size() && moved == lanes.size() * stride, "%s: %zu reads, %zu writes, %zu bytes", name, reads, writes, moved);
  size_t k = 0;
  for (size_t i = 0; i < n; i++) {
    const bool mine = k < lanes.size() && lanes[k] == i;
    CHECK(memcmp(dev.get() + i * stride, mine ? vals.data() + k * stride : before.get() + i * stride, stride) == 0, "%s: lane %zu %s", name, i, mine ? "was not patched" : "was disturbed");
    if (mine) k++;
  }
  // a failing copier ends the patch with its code
  CHECK(wire_patch_run(lanes.data(), lanes.size(), stride, vals.data(), [](uint8_t*, size_t, size_t) { return -5; }, [](size_t, const uint8_t*, size_t) { return -5; }) == -5, "%s", name);
}

static void patch_cases() {
  for (size_t stride : {(size_t)1, (size_t)32, (size_t)128, (size_t)141}) {
    patch_case("dense, every lane", 9, stride, {0, 1, 2, 3, 4, 5, 6, 7, 8}, true);
    patch_case("dense, one lane", 5, stride, {3}, true);
    patch_case("dense with gaps", 40, stride, {1, 7, 8, 30, 38}, true);
    patch_case("span just under 2 * lanes + 64", 80, stride, {5, 6, 72}, true);
    patch_case("span == 2 * lanes + 64", 80, stride, {5, 6, 74}, true);
    patch_case("span == 2 * lanes + 64 + 1", 80, stride, {5, 6, 75}, false);
    patch_case("two lanes at the ends", 700, stride, {0, 699}, false);
    patch_case("two lanes at the ends, the span asked for", 700, stride, {0, 699}, true, true);
  }
  CHECK(wire_patch_run(nullptr, 0, 32, nullptr, [](uint8_t*, size_t, size_t) { return -1; }, [](size_t, const uint8_t*, size_t) { return -1; }) == 0, "an empty window copies nothing");
}

// ---- (c) ----------------------------------------------------------------------------------------------------------------------------
static int parse_cases(const char* path) {
  FILE* in = fopen(path, "rb");
  uint32_t L32;
  if (!in || fread(&L32, 4, 1, in) != 1 || L32 < 1 || L32 > 4096) { fprintf(stderr, "cannot read the corpus\n"); return 2; }
  std::vector<uint8_t> blob, want; std::vector<uint64_t> offs(1, 0);
  for (;;) {
    uint32_t len; uint8_t code;
    if (fread(&len, 4, 1, in) != 1) break;
    const size_t at = blob.size();
    blob.resize(at + len);
    if ((len && fread(blob.data() + at, 1, len, in) != len) || fread(&code, 1, 1, in) != 1) { fprintf(stderr, "short corpus\n"); return 2; }
    want.push_back(code); offs.push_back(blob.size());
  }
  fclose(in);
  const size_t n = want.size(), rb = 128;
  const CborType* T = cbor_type(1);                           // ACT_CBOR_ISSUANCE_REQUEST
  std::unique_ptr<uint8_t[]> dev(new uint8_t[blob.size() ? blob.size() : 1]);
  memcpy(dev.get(), blob.data(), blob.size());
  const WireExtent x{dev.get(), offs.data(), 0};
  std::vector<size_t> which(n); std::iota(which.begin(), which.end(), 0);
  size_t seen[4] = {0, 0, 0, 0};
  for (int gathered = 0; gathered < 2; gathered++) {         // a device-memory caller's window, then a host-memory caller's (read in place)
    WireGather g; std::vector<uint8_t> recs; std::vector<int> codes; std::vector<CborCand> cands;
    wire_gather_plan(x, which.data(), n, g);
    std::unique_ptr<uint8_t[]> host(new uint8_t[g.bytes ? g.bytes : 1]);
    wire_gather_run(g, host.get(), [&](uint8_t* dst, size_t src, size_t l) -> int { memcpy(dst, dev.get() + src, l); return 0; });
    wire_window_parse(*T, (int)L32, x, which.data(), n, gathered ? host.get() : nullptr, g.at, rb, recs, codes, cands);
    CHECK(recs.size() == n * rb && codes.size() == n && cands.size() == n, "the window's arrays");
    for (size_t k = 0; k < n; k++) {
      // the reader's own code: the model's, except that an invalid point is for the GPU to find (cbor_settle_codes) -- the model's 3
      // is a message that reads (0) or one that stopped at a structural fault behind the point (2)
      uint8_t alone[128]; memset(alone, 0, 128);
      const int spec = cbor_read_message(*T, (int)L32, blob.data() + offs[k], (size_t)(offs[k + 1] - offs[k]), alone);
      CHECK(codes[k] == spec, "message %zu: code %d, the reader alone says %d", k, codes[k], spec);
      CHECK(want[k] == 3 ? (codes[k] == CBOR_OK || codes[k] == CBOR_ERR_STRUCTURE) : codes[k] == (int)want[k], "message %zu: code %d, the model says %u", k, codes[k], want[k]);
      bool zero = true;
      for (size_t j = 0; j < rb; j++) zero = zero && recs[k * rb + j] == 0;
      if (codes[k] != CBOR_OK) CHECK(zero, "message %zu failed (%d) and left a record that is not zero", k, codes[k]);
      else CHECK(memcmp(recs.data() + k * rb, alone, rb) == 0 && !zero, "message %zu: record", k);
      if (!gathered) seen[codes[k] & 3]++;
    }
  }
  CHECK(seen[CBOR_OK] && seen[CBOR_ERR_PARSE] && seen[CBOR_ERR_STRUCTURE], "the corpus holds %zu / %zu / %zu messages of the three codes", seen[0], seen[1], seen[2]);
  printf("parsed %zu messages: %zu read, %zu malformed, %zu of another structure\n", n, seen[0], seen[1], seen[2]);
  return 0;
}

int main(int argc, char** argv) {
  gather_cases();
  patch_cases();
  // the status of a code: one spelling for the device road and the host road
  CHECK(act::cbor_code_status(CBOR_OK) == 0 && act::cbor_code_status(CBOR_ERR_PARSE) == 254 && act::cbor_code_status(CBOR_ERR_STRUCTURE) == 253 && act::cbor_code_status(CBOR_ERR_VALUE) == 255, "code -> status");
  CHECK(ACT_STATUS_UNDECODABLE == 255 && ACT_STATUS_CBOR_MALFORMED == 254 && ACT_STATUS_CBOR_STRUCTURE == 253, "the statuses of the interface");
  CHECK(WIRE_SETTLE_WINDOW == 4096, "the window");
  if (argc > 1) { const int rc = parse_cases(argv[1]); if (rc) return rc; }
  printf("WIRE WINDOW CHECK: %zu failures\n", failures);
  return failures ? 1 : 0;
}
