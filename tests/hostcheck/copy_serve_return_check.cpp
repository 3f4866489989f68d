// copy_serve_return_check.cpp — TEST-ONLY host build of the serve pass of the return replay unique forms (csrc/copy_lanes.h:
// copy_serve_return_lane, and copy_serve_return_piece as k_copy_serve_return runs it, one thread per 16-byte piece, the grid's tail
// included) beside the serve pass of the replay unique forms (copy_serve_lane), which must answer as before.  Built by
// tests/return_replay_unique_cases.py as a small library for tests/test_return_replay_unique_host.py; with
// -DCOPY_SERVE_RETURN_CHECK_MAIN it is a stand-alone program that runs the same checks (hc_serve_return_checks) and is run under the
// sanitizers.  The build counts field multiplications and squarings (ACT_FE_BOUNDS): the serve pass must not add one.  Never linked
// into libact_mi355x.so.
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
#define EXPECT(cond) do { if (!(cond)) { failures++; if (failures < 20) fprintf(stderr, "copy_serve_return_check: line %d: %s\n", __LINE__, #cond); } } while (0)

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint8_t next_byte() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint8_t)(rng_state >> 24); }

constexpr size_t GUARD = 64;
constexpr uint8_t GUARD_BYTE = 0xC3;

// l, the group order, little-endian
const uint8_t ELL[32] = {0xed, 0xd3, 0xf5, 0x5c, 0x1a, 0x63, 0x12, 0x58, 0xd6, 0x9c, 0xf7, 0xa2, 0xde, 0xf9, 0xde, 0x14,
                         0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0x10};
// v, or v + l, as 32 little-endian bytes
void amount(uint8_t out[32], uint32_t v, bool plus_l) {
  memset(out, 0, 32);
  for (int b = 0; b < 4; b++) out[b] = (uint8_t)(v >> (8 * b));
  if (!plus_l) return;
  uint32_t carry = 0;
  for (int b = 0; b < 32; b++) { const uint32_t s = (uint32_t)out[b] + ELL[b] + carry; out[b] = (uint8_t)s; carry = s >> 8; }
}

// the table of the header, written out a second time the plain way: what a copy of a leader that ended `s` says
struct Want { uint8_t status, replayed; bool row; };
Want want_of(uint8_t s, bool same) {
  if (s == 0 && same) return {0, 1, true};
  if ((s == 0 || s == 251) && !same) return {3, 0, false};
  if (s == 251) return {251, 1, false};
  return {s, 0, false};
}

// the leader's final status and key, and its replay mark (0 fresh, 1 replayed)
struct Row { uint8_t status, key, replayed; };
const Row ROWS[] = {{0, 2, 0}, {0, 1, 1}, {255, 255, 0}, {6, 255, 0}, {7, 255, 0}, {3, 3, 0}, {252, 0, 0}, {251, 1, 0}, {251, 0, 1}};
constexpr uint32_t N_ROWS = sizeof(ROWS) / sizeof(ROWS[0]);

// One array: per table row a leader with amount 5 + r, a bystander that is not a copy, then `copies` copies of the leader with a
// bystander after every seventh.  Copy c names the leader's amount (c % 3 == 0), the leader's amount + l (1) or another amount (2).
// Every byte of the buffer (its guards in front and behind included) has an expected value.  base_off: the output base is that many
// bytes past an aligned address, and the amounts lie base_off bytes past one too.  pieces: copy_serve_return_piece for every
// (lane, piece) of the launch grid in REVERSE order in place of copy_serve_return_lane.  no_amounts: a null amounts array (every t = 0).
void serve_case(uint64_t out_b, uint32_t base_off, bool with_replayed, uint32_t copies, bool pieces, bool no_amounts) {
  std::vector<uint32_t> lead; std::vector<uint8_t> status, okey, rep, same, amt;
  uint8_t t[32];
  for (uint32_t r = 0; r < N_ROWS; r++) {
    const uint32_t leader = (uint32_t)lead.size();
    auto lane = [&](uint32_t l, uint8_t s, uint8_t k, uint8_t m, uint32_t v, bool plus_l, bool sm) {
      lead.push_back(l); status.push_back(s); okey.push_back(k); rep.push_back(m); same.push_back(sm || no_amounts);
      amount(t, v, plus_l); amt.insert(amt.end(), t, t + 32);
    };
    lane(COPY_NONE, ROWS[r].status, ROWS[r].key, ROWS[r].replayed, 5 + r, r % 2 == 1, true);      // (every other leader names t + l itself)
    lane(COPY_NONE, (uint8_t)(r % 2 ? 7 : 0), (uint8_t)(r % 3), (uint8_t)(r % 2 ? 0 : 1), 77, false, true);
    for (uint32_t c = 0; c < copies; c++) {
      const uint32_t kind = c % 3;
      lane(leader, COPY_MARK, 255, 0, kind == 2 ? 4 + r : 5 + r, kind == 1, kind != 2);      // as the scatters leave a copy
      if (c % 7 == 6) lane(COPY_NONE, 250, 255, 0, 1, false, true);
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
  // exact size behind base_off bytes (the allocator's blocks are 16-byte aligned): a read past the last amount is the sanitizer's to find
  const size_t tat = base_off;
  std::vector<uint8_t> tbuf(tat + (size_t)n * 32, GUARD_BYTE);
  memcpy(tbuf.data() + tat, amt.data(), (size_t)n * 32);
  const std::vector<uint8_t> tbuf_before = tbuf;

  // what must come out, written the plain way
  std::vector<uint8_t> want_buf = buf, want_st = st, want_ok = ok, want_rp = rp;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t l = lead[i];
    if (l == COPY_NONE) continue;
    const Want w = want_of(status[l], same[i] != 0);
    want_st[GUARD + i] = w.status; want_ok[GUARD + i] = okey[l]; want_rp[GUARD + i] = w.replayed;
    if (w.row) memcpy(want_buf.data() + at + (size_t)i * out_b, want_buf.data() + at + (size_t)l * out_b, out_b);
    else memset(want_buf.data() + at + (size_t)i * out_b, 0, out_b);
  }

  const CopyServeReturnArgs a{{lead.data(), n, out_b, st.data() + GUARD, ok.data() + GUARD, out, with_replayed ? rp.data() + GUARD : nullptr},
                              no_amounts ? nullptr : tbuf.data() + tat};
  const fe_counts_t before = fe_counts;
  if (!pieces) for (uint32_t i = 0; i < (n + 255) / 256 * 256; i++) copy_serve_return_lane(a, i);
  else {
    const uint32_t per = admit_pieces(out_b);
    const uint64_t grid = ((uint64_t)n * per + 255) / 256 * 256;
    for (uint64_t p = grid; p-- > 0;) { const uint64_t i = p / per; if (i < n) copy_serve_return_piece(a, (uint32_t)i, (uint32_t)(p % per)); }
  }
  EXPECT(fe_counts.mul == before.mul && fe_counts.sq == before.sq && fe_counts.sqadd == before.sqadd);
  EXPECT(buf == want_buf);
  EXPECT(st == want_st && ok == want_ok);
  EXPECT(tbuf == tbuf_before);
  EXPECT(rp == (with_replayed ? want_rp : [&] { std::vector<uint8_t> v(GUARD, GUARD_BYTE); v.insert(v.end(), rep.begin(), rep.end()); v.insert(v.end(), GUARD, GUARD_BYTE); return v; }()));
  // a served copy carries a record, every other copy none
  for (uint32_t i = 0; i < n; i++) if (lead[i] != COPY_NONE) {
    bool any = false;
    for (uint64_t b = 0; b < out_b; b++) any |= out[(size_t)i * out_b + b] != 0;
    EXPECT(any == (status[lead[i]] == 0 && same[i]));
  }
}

// the verdicts one by one, and the amounts' comparison: t against t, t + l, t + 1, 0 against l, and the top bits
void verdicts_and_amounts() {
  for (uint32_t s = 0; s < 256; s++) for (int same = 0; same < 2; same++) {
    const CopyServed c = copy_serve_return_verdict((uint8_t)s, same != 0);
    const Want w = want_of((uint8_t)s, same != 0);
    EXPECT(c.status == w.status && c.replayed == w.replayed && c.row == w.row);
  }
  uint8_t buf[3][40];
  for (uint32_t off = 0; off < 4; off++) {      // any address
    uint8_t *x = buf[0] + off, *y = buf[1] + off, *z = buf[2] + off;
    amount(x, 9, false); amount(y, 9, true); amount(z, 10, false);
    EXPECT(copy_same_amount(x, x) && copy_same_amount(x, y) && copy_same_amount(y, x) && !copy_same_amount(x, z) && !copy_same_amount(y, z));
    amount(x, 0, false); amount(y, 0, true);
    EXPECT(copy_same_amount(x, y) && !copy_same_amount(y, z));
    amount(x, 3, false); memcpy(y, x, 32); y[31] = 0x80;      // 3 + 2^255 is another amount
    EXPECT(!copy_same_amount(x, y));
  }
}

// the serve pass of the replay unique forms answers as it did: the leader's status whatever it is, the mark 1 only behind a 0
void serve_unchanged() {
  std::vector<uint32_t> lead; std::vector<uint8_t> st, ok, rp;
  for (uint32_t r = 0; r < N_ROWS; r++) { lead.push_back(COPY_NONE); st.push_back(ROWS[r].status); ok.push_back(ROWS[r].key); rp.push_back(ROWS[r].replayed); }
  for (uint32_t r = 0; r < N_ROWS; r++) for (int c = 0; c < 3; c++) { lead.push_back(r); st.push_back(COPY_MARK); ok.push_back(255); rp.push_back(0); }
  const uint32_t n = (uint32_t)lead.size();
  const uint64_t out_b = 17;
  std::vector<uint8_t> out((size_t)n * out_b, 0);
  for (uint32_t r = 0; r < N_ROWS; r++) for (uint64_t b = 0; b < out_b; b++) out[r * out_b + b] = (uint8_t)(next_byte() | 1);
  const CopyServeArgs a{lead.data(), n, out_b, st.data(), ok.data(), out.data(), rp.data()};
  for (uint32_t i = 0; i < (n + 255) / 256 * 256; i++) copy_serve_lane(a, i);
  for (uint32_t r = 0; r < N_ROWS; r++) for (int c = 0; c < 3; c++) {
    const uint32_t i = N_ROWS + 3 * r + c;
    EXPECT(st[i] == ROWS[r].status && ok[i] == ROWS[r].key && rp[i] == (ROWS[r].status == 0 ? 1 : 0));
    bool equal = true, zero = true;
    for (uint64_t b = 0; b < out_b; b++) { equal &= out[i * out_b + b] == out[r * out_b + b]; zero &= out[i * out_b + b] == 0; }
    EXPECT(ROWS[r].status == 0 ? equal : zero);
  }
  for (uint32_t r = 0; r < N_ROWS; r++) EXPECT(st[r] == ROWS[r].status && ok[r] == ROWS[r].key && rp[r] == ROWS[r].replayed);
}

}  // namespace

extern "C" {

// the serve pass over the caller's arrays: lane by lane (the host-memory callers' loop) or piece by piece over the launch grid
void hc_serve_return(const uint32_t* lead, uint32_t n, uint64_t out_b, uint8_t* status, uint8_t* out_key, uint8_t* out, uint8_t* out_replayed, const uint8_t* amounts,
                     int pieces) {
  const CopyServeReturnArgs a{{lead, n, out_b, status, out_key, out, out_replayed}, amounts};
  if (!pieces) { for (uint32_t i = 0; i < (n + 255) / 256 * 256; i++) copy_serve_return_lane(a, i); return; }
  const uint32_t per = admit_pieces(out_b);
  const uint64_t grid = ((uint64_t)n * per + 255) / 256 * 256;
  for (uint64_t p = 0; p < grid; p++) { const uint64_t i = p / per; if (i < n) copy_serve_return_piece(a, (uint32_t)i, (uint32_t)(p % per)); }
}
// the serve pass of the replay unique forms, lane by lane
void hc_serve_plain(const uint32_t* lead, uint32_t n, uint64_t out_b, uint8_t* status, uint8_t* out_key, uint8_t* out, uint8_t* out_replayed) {
  const CopyServeArgs a{lead, n, out_b, status, out_key, out, out_replayed};
  for (uint32_t i = 0; i < (n + 255) / 256 * 256; i++) copy_serve_lane(a, i);
}
int hc_same_amount(const uint8_t* x, const uint8_t* y) { return copy_same_amount(x, y) ? 1 : 0; }
// field multiplications + squarings the build has counted so far (the serve pass adds none)
uint64_t hc_serve_return_field_ops() { return fe_counts.mul + fe_counts.sq + fe_counts.sqadd; }

// every row of the table with copies of all three kinds; out_b in the list given; base pointers 0 .. 3 bytes past an aligned address;
// out_replayed null and not; 0, 1, 3 and 4 096 copies behind a leader; both walks; with and without an amounts array
// -> the number of failed expectations
int hc_serve_return_checks(const uint64_t* out_bs, uint32_t count) {
  failures = 0;
  verdicts_and_amounts();
  serve_unchanged();
  for (uint32_t k = 0; k < count; k++)
    for (uint32_t off = 0; off < 4; off++)
      for (int with_replayed = 0; with_replayed < 2; with_replayed++)
        for (uint32_t copies : {0u, 1u, 3u, 4096u}) {
          if (copies == 4096u && (off & 1u) != (uint32_t)with_replayed) continue;      // the long runs: every offset, out_replayed null on the even ones
          serve_case(out_bs[k], off, with_replayed != 0, copies, false, false);
          serve_case(out_bs[k], off, with_replayed != 0, copies, true, false);
          if (copies == 3u) serve_case(out_bs[k], off, with_replayed != 0, copies, off % 2 == 0, true);
        }
  return failures;
}

}  // extern "C"

#if defined(COPY_SERVE_RETURN_CHECK_MAIN)
// arguments: the row sizes (default: 1, 16, 17, 160 and 176, the framed RefundReturn)
int main(int argc, char** argv) {
  std::vector<uint64_t> out_bs;
  for (int i = 1; i < argc; i++) out_bs.push_back(strtoull(argv[i], nullptr, 10));
  if (out_bs.empty()) out_bs = {1, 16, 17, 160, 176};
  const int bad = hc_serve_return_checks(out_bs.data(), (uint32_t)out_bs.size());
  if (bad || hc_serve_return_field_ops()) { fprintf(stderr, "copy_serve_return_check: %d failures, %llu field operations\n", bad, (unsigned long long)hc_serve_return_field_ops()); return 1; }
  puts("COPY SERVE RETURN CHECK CLEAN");
  return 0;
}
#endif
