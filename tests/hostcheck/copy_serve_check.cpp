// copy_serve_check.cpp — TEST-ONLY host build of the serve pass of the replay unique forms (csrc/copy_lanes.h: copy_serve_lane, and
// copy_serve_piece as k_copy_serve runs it, one thread per 16-byte piece, the grid's tail included) beside the resolve pass of the
// admission unique forms, which must answer as before.  Built by tests/admit_replay_unique_cases.py as a small library for
// tests/test_admit_replay_unique_host.py; with -DCOPY_SERVE_CHECK_MAIN it is a stand-alone program that runs the same checks
// (hc_copy_serve_checks) and is run under the sanitizers.  The build counts field multiplications and squarings (ACT_FE_BOUNDS): the
// serve pass must not add one.  Never linked into libact_mi355x.so.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define ACT_FE_BOUNDS 1
#include "../../anonymous-credit-tokens_amd/csrc/copy_lanes.h"

namespace act { fe_bounds_t fe_bounds = {0, 0, 0, 0, 0, 0}; fe_counts_t fe_counts = {0, 0, {0, 0, 0, 0}}; }
using namespace act;

namespace {

int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { failures++; if (failures < 20) fprintf(stderr, "copy_serve_check: line %d: %s\n", __LINE__, #cond); } } while (0)

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint8_t next_byte() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint8_t)(rng_state >> 24); }

constexpr size_t GUARD = 64;
constexpr uint8_t GUARD_BYTE = 0xC3;

// the table of the header, row by row: the leader's final status and key, and what a copy of it must say
struct Row { uint8_t status, key, replayed; };      // replayed: the LEADER's mark (0 fresh, 1 replayed)
const Row ROWS[] = {{0, 2, 0}, {0, 1, 1}, {255, 255, 0}, {6, 255, 0}, {7, 255, 0}, {3, 3, 0}, {252, 0, 0}, {251, 1, 0}};
constexpr uint32_t N_ROWS = sizeof(ROWS) / sizeof(ROWS[0]);

// One array: per table row a leader, a bystander that is not a copy, then `copies` copies of the leader with a bystander after every
// seventh -- so rows that must stay as they are lie in front of, between and behind the rows that are written, and every byte of the
// buffer (its guards in front and behind included) has an expected value.  base_off: the output base is that many bytes past an
// aligned address.  pieces: run copy_serve_piece for every (lane, piece) of the launch grid in REVERSE order in place of copy_serve_lane.
void serve_case(uint64_t out_b, uint32_t base_off, bool with_replayed, uint32_t copies, bool pieces) {
  std::vector<uint32_t> lead; std::vector<uint8_t> status, okey, rep;
  for (uint32_t r = 0; r < N_ROWS; r++) {
    const uint32_t leader = (uint32_t)lead.size();
    auto lane = [&](uint32_t l, uint8_t s, uint8_t k, uint8_t m) { lead.push_back(l); status.push_back(s); okey.push_back(k); rep.push_back(m); };
    lane(COPY_NONE, ROWS[r].status, ROWS[r].key, ROWS[r].replayed);
    lane(COPY_NONE, (uint8_t)(r % 2 ? 7 : 0), (uint8_t)(r % 3), (uint8_t)(r % 2 ? 0 : 1));
    for (uint32_t c = 0; c < copies; c++) {
      lane(leader, COPY_MARK, 255, 0);      // as the scatters leave a copy
      if (c % 7 == 6) lane(COPY_NONE, 250, 255, 0);
    }
  }
  const uint32_t n = (uint32_t)lead.size();
  // exact sizes behind the guards: a lane that strays further is the sanitizer's to find
  std::vector<uint8_t> buf(GUARD + 16 + (size_t)n * out_b + GUARD, GUARD_BYTE);
  const size_t at = GUARD + ((16 - (size_t)(reinterpret_cast<uintptr_t>(buf.data()) + GUARD) % 16) % 16) + base_off;
  uint8_t* out = buf.data() + at;
  for (uint32_t i = 0; i < n; i++) for (uint64_t b = 0; b < out_b; b++) out[(size_t)i * out_b + b] = lead[i] == COPY_NONE ? (uint8_t)(next_byte() | 1) : 0;
  std::vector<uint8_t> st(GUARD, GUARD_BYTE), ok(GUARD, GUARD_BYTE), rp(GUARD, GUARD_BYTE);
  st.insert(st.end(), status.begin(), status.end()); ok.insert(ok.end(), okey.begin(), okey.end()); rp.insert(rp.end(), rep.begin(), rep.end());
  st.insert(st.end(), GUARD, GUARD_BYTE); ok.insert(ok.end(), GUARD, GUARD_BYTE); rp.insert(rp.end(), GUARD, GUARD_BYTE);

  // what must come out, written the plain way
  std::vector<uint8_t> want_buf = buf, want_st = st, want_ok = ok, want_rp = rp;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t l = lead[i];
    if (l == COPY_NONE) continue;
    want_st[GUARD + i] = status[l]; want_ok[GUARD + i] = okey[l]; want_rp[GUARD + i] = status[l] == 0 ? 1 : 0;
    if (status[l] == 0) memcpy(want_buf.data() + at + (size_t)i * out_b, want_buf.data() + at + (size_t)l * out_b, out_b);
    else memset(want_buf.data() + at + (size_t)i * out_b, 0, out_b);
  }

  const CopyServeArgs a{lead.data(), n, out_b, st.data() + GUARD, ok.data() + GUARD, out, with_replayed ? rp.data() + GUARD : nullptr};
  const fe_counts_t before = fe_counts;
  if (!pieces) for (uint32_t i = 0; i < (n + 255) / 256 * 256; i++) copy_serve_lane(a, i);
  else {
    const uint32_t per = admit_pieces(out_b);
    const uint64_t grid = ((uint64_t)n * per + 255) / 256 * 256;
    for (uint64_t p = grid; p-- > 0;) { const uint64_t i = p / per; if (i < n) copy_serve_piece(a, (uint32_t)i, (uint32_t)(p % per)); }
  }
  EXPECT(fe_counts.mul == before.mul && fe_counts.sq == before.sq && fe_counts.sqadd == before.sqadd);
  EXPECT(buf == want_buf);
  EXPECT(st == want_st && ok == want_ok);
  EXPECT(rp == (with_replayed ? want_rp : [&] { std::vector<uint8_t> v(GUARD, GUARD_BYTE); v.insert(v.end(), rep.begin(), rep.end()); v.insert(v.end(), GUARD, GUARD_BYTE); return v; }()));
  // a served copy carries a record, every other copy none
  for (uint32_t i = 0; i < n; i++) if (lead[i] != COPY_NONE) {
    bool any = false;
    for (uint64_t b = 0; b < out_b; b++) any |= out[(size_t)i * out_b + b] != 0;
    EXPECT(any == (status[lead[i]] == 0));
  }
}

// the resolve pass of the admission unique forms answers as it did
void resolve_unchanged() {
  const uint8_t want[N_ROWS] = {3, 3, 255, 6, 7, 3, 252, 3};
  std::vector<uint32_t> lead; std::vector<uint8_t> st, ok;
  for (uint32_t r = 0; r < N_ROWS; r++) { lead.push_back(COPY_NONE); st.push_back(ROWS[r].status); ok.push_back(ROWS[r].key); }
  for (uint32_t r = 0; r < N_ROWS; r++) for (int c = 0; c < 3; c++) { lead.push_back(r); st.push_back(COPY_MARK); ok.push_back(255); }
  lead.push_back(COPY_NONE); st.push_back(250); ok.push_back(255);
  const uint32_t n = (uint32_t)lead.size();
  CopyResolveArgs a{lead.data(), n, st.data(), ok.data()};
  for (uint32_t i = 0; i < (n + 255) / 256 * 256; i++) copy_resolve_lane(a, i);
  for (uint32_t r = 0; r < N_ROWS; r++) {
    EXPECT(copy_status(ROWS[r].status) == want[r] && st[r] == ROWS[r].status && ok[r] == ROWS[r].key);
    for (int c = 0; c < 3; c++) EXPECT(st[N_ROWS + 3 * r + c] == want[r] && ok[N_ROWS + 3 * r + c] == ROWS[r].key);
  }
  EXPECT(st[n - 1] == 250 && ok[n - 1] == 255);
}

// 16 bytes and every shorter piece at every address mod 16: what copy_store16 writes is what copy_load16 read, and nothing else
void store_is_the_counterpart_of_load() {
  std::vector<uint8_t> src(80), dst(80);
  for (uint32_t off = 0; off < 16; off++) for (uint32_t bytes = 0; bytes <= 16; bytes++) {
    for (auto& b : src) b = next_byte();
    std::fill(dst.begin(), dst.end(), GUARD_BYTE);
    uint64_t w[2];
    copy_load16(w, src.data() + 16 + off, bytes);
    copy_store16(dst.data() + 32 + (15 - off), w, bytes);
    for (uint32_t b = 0; b < 80; b++) {
      const uint32_t k = b - (32 + 15 - off);
      EXPECT(dst[b] == (k < bytes ? src[16 + off + k] : GUARD_BYTE));
    }
  }
}

}  // namespace

extern "C" {

// the serve pass over the caller's arrays: lane by lane (the host-memory callers' loop) or piece by piece over the launch grid
void hc_copy_serve(const uint32_t* lead, uint32_t n, uint64_t out_b, uint8_t* status, uint8_t* out_key, uint8_t* out, uint8_t* out_replayed, int pieces) {
  const CopyServeArgs a{lead, n, out_b, status, out_key, out, out_replayed};
  if (!pieces) { for (uint32_t i = 0; i < (n + 255) / 256 * 256; i++) copy_serve_lane(a, i); return; }
  const uint32_t per = admit_pieces(out_b);
  const uint64_t grid = ((uint64_t)n * per + 255) / 256 * 256;
  for (uint64_t p = 0; p < grid; p++) { const uint64_t i = p / per; if (i < n) copy_serve_piece(a, (uint32_t)i, (uint32_t)(p % per)); }
}
// field multiplications + squarings the build has counted so far (the serve pass adds none)
uint64_t hc_copy_serve_field_ops() { return fe_counts.mul + fe_counts.sq + fe_counts.sqadd; }

// every row of the table; out_b in the list given; base pointers 0 .. 3 bytes past an aligned address; out_replayed null and not;
// 0, 1 and 4 096 copies behind a leader; both walks.  -> the number of failed expectations
int hc_copy_serve_checks(const uint64_t* out_bs, uint32_t count) {
  failures = 0;
  store_is_the_counterpart_of_load();
  resolve_unchanged();
  for (uint32_t k = 0; k < count; k++)
    for (uint32_t off = 0; off < 4; off++)
      for (int with_replayed = 0; with_replayed < 2; with_replayed++)
        for (uint32_t copies : {0u, 1u, 4096u}) {
          if (copies == 4096u && (off & 1u) != (uint32_t)with_replayed) continue;      // the long runs: every offset, out_replayed null on the even ones
          serve_case(out_bs[k], off, with_replayed != 0, copies, false);
          serve_case(out_bs[k], off, with_replayed != 0, copies, true);
        }
  return failures;
}

}  // extern "C"

#if defined(COPY_SERVE_CHECK_MAIN)
// arguments: the row sizes (default: 1, 16, 17, 128 and 141, the framed Refund)
int main(int argc, char** argv) {
  std::vector<uint64_t> out_bs;
  for (int i = 1; i < argc; i++) out_bs.push_back(strtoull(argv[i], nullptr, 10));
  if (out_bs.empty()) out_bs = {1, 16, 17, 128, 141};
  const int bad = hc_copy_serve_checks(out_bs.data(), (uint32_t)out_bs.size());
  if (bad || hc_copy_serve_field_ops()) { fprintf(stderr, "copy_serve_check: %d failures, %llu field operations\n", bad, (unsigned long long)hc_copy_serve_field_ops()); return 1; }
  puts("COPY SERVE CHECK CLEAN");
  return 0;
}
#endif
