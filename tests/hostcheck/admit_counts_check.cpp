// admit_counts_check.cpp — TEST-ONLY stand-alone program over csrc/admit_counts.h (tests/test_admit_counts_host.py builds it with g++,
// once more under ASan + UBSan, and runs it).  Every expectation below is written by hand from what include/act_mi355x.h says each
// count means, for all eight forms; every input array lives in a heap block of exactly its size.  Prints the eight lengths for the
// Python side, then "ADMIT COUNTS CHECK: <failures> failures".
#include <cstdio>
#include <initializer_list>
#include <vector>
#include "../../anonymous-credit-tokens_amd/csrc/admit_counts.h"

using namespace act;

static int failures = 0;
static const uint8_t WRONG = ACT_STATUS_WRONG_CHARGE, SPENT = ACT_STATUS_DOUBLE_SPEND, BIG = ACT_STATUS_RETURN_TOO_BIG, WIRE = 254, WIRE2 = 253, REJ = 7,
                     UNDET = ACT_STATUS_NULLIFIER_UNDETERMINED, UNSIGNED = ACT_STATUS_RECORDED_UNSIGNED;
static const uint32_t NONE = COPY_NONE;

static const AdmitForm ADMIT{false, false, false}, ADMIT_U{true, false, false}, RETURN{false, false, true}, RETURN_U{true, false, true},
                       REPLAY{false, true, false}, REPLAY_U{true, true, false}, RET_REPLAY{false, true, true}, RET_REPLAY_U{true, true, true};

struct Batch {
  std::vector<uint8_t> pre, cst, fin, amounts; std::vector<uint32_t> lead; std::vector<uint64_t> tc;
  size_t mv = 0, candidates = 0, copies = 0;
};

static void expect(const char* what, const AdmitForm& f, const Batch& b, std::initializer_list<uint64_t> want) {
  AdmitCountsIn in{b.pre.size(), b.pre.empty() ? nullptr : b.pre.data(), b.mv, b.cst.empty() ? nullptr : b.cst.data(), b.candidates,
                   b.tc.empty() ? nullptr : b.tc.data(), b.copies, b.lead.empty() ? nullptr : b.lead.data(), b.fin.empty() ? nullptr : b.fin.data(),
                   b.amounts.empty() ? nullptr : b.amounts.data()};
  std::vector<uint64_t> got(admit_counts_len(f), 0xEEEE);      // (a block of exactly the form's length: a write past it is the sanitizer's)
  admit_counts(f, in, got.data());
  const std::vector<uint64_t> w(want);
  if (got != w) {
    failures++;
    printf("FAIL %s (unique %d replay %d ret %d): got", what, f.unique, f.replay, f.ret);
    for (uint64_t v : got) printf(" %llu", (unsigned long long)v);
    printf(", want");
    for (uint64_t v : w) printf(" %llu", (unsigned long long)v);
    printf("\n");
  }
}

static std::vector<uint8_t> amounts_of(std::initializer_list<int> ts) {      // t < 256 as 32 little-endian bytes; -2: the scalar l + 2
  static const uint8_t ell[32] = {0xed, 0xd3, 0xf5, 0x5c, 0x1a, 0x63, 0x12, 0x58, 0xd6, 0x9c, 0xf7, 0xa2, 0xde, 0xf9, 0xde, 0x14, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0x10};
  std::vector<uint8_t> out;
  for (int t : ts) {
    uint8_t row[32] = {0};
    if (t == -2) { memcpy(row, ell, 32); row[0] += 2; } else row[0] = (uint8_t)t;
    out.insert(out.end(), row, row + 32);
  }
  return out;
}

int main() {
  printf("LEN admit %zu\nLEN admit_unique %zu\nLEN return %zu\nLEN return_unique %zu\n", admit_counts_len(ADMIT), admit_counts_len(ADMIT_U), admit_counts_len(RETURN), admit_counts_len(RETURN_U));
  printf("LEN admit_replay %zu\nLEN admit_replay_unique %zu\nLEN return_replay %zu\nLEN return_replay_unique %zu\n", admit_counts_len(REPLAY), admit_counts_len(REPLAY_U),
         admit_counts_len(RET_REPLAY), admit_counts_len(RET_REPLAY_U));

  // ---- the empty batch ---------------------------------------------------------------------------------------------------------------
  const Batch none;
  expect("empty", ADMIT, none, {0, 0, 0, 0, 0, 0, 0, 0});
  expect("empty", ADMIT_U, none, {0, 0, 0, 0, 0, 0, 0, 0, 0});
  expect("empty", RETURN, none, {0, 0, 0, 0, 0, 0, 0, 0, 0});
  expect("empty", RETURN_U, none, {0, 0, 0, 0, 0, 0, 0, 0, 0, 0});
  expect("empty", REPLAY, none, {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0});
  expect("empty", REPLAY_U, none, {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0});
  expect("empty", RET_REPLAY, none, {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0});
  expect("empty", RET_REPLAY_U, none, {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0});

  // ---- everything shed: a wrong charge, two spent lanes, two messages that do not read (the return forms: one of them t > s) -----------
  Batch shed; shed.pre = {WRONG, SPENT, WIRE, WIRE2, SPENT};
  Batch shed_t = shed; shed_t.pre[3] = BIG;
  //                              lanes wire wrong spent verified rej dsa acc
  expect("all shed", ADMIT, shed, {5, 2, 1, 2, 0, 0, 0, 0});
  expect("all shed", ADMIT_U, shed, {5, 2, 1, 2, 0, 0, 0, 0, 0});
  expect("all shed", RETURN, shed_t, {5, 1, 1, 2, 0, 0, 0, 0, 1});
  expect("all shed", RETURN_U, shed_t, {5, 1, 1, 2, 0, 0, 0, 0, 1, 0});
  //                               lanes wire wrong foreign cand verified rej fresh replayed dsa unanswered
  expect("all shed", REPLAY, shed, {5, 2, 1, 2, 0, 0, 0, 0, 0, 0, 0});
  expect("all shed", REPLAY_U, shed, {5, 2, 1, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0});
  expect("all shed", RET_REPLAY, shed_t, {5, 1, 1, 2, 0, 0, 0, 0, 0, 0, 0, 1});
  expect("all shed", RET_REPLAY_U, shed_t, {5, 1, 1, 2, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0});

  // ---- nothing shed: two accepted, one rejected by verification, one found spent by the check-and-insert ------------------------------------
  Batch all; all.pre = {0, 0, 0, 0}; all.mv = 4; all.cst = {0, 0, REJ, SPENT};
  all.candidates = 1; all.tc = {4, 1, 1, 1, 1, 0};      // the replay tail over the same lanes: one rejected, one fresh, one replayed, one double spend
  expect("none shed", ADMIT, all, {4, 0, 0, 0, 4, 1, 1, 2});
  expect("none shed", ADMIT_U, all, {4, 0, 0, 0, 4, 1, 1, 2, 0});
  expect("none shed", RETURN, all, {4, 0, 0, 0, 4, 1, 1, 2, 0});
  expect("none shed", RETURN_U, all, {4, 0, 0, 0, 4, 1, 1, 2, 0, 0});
  expect("none shed", REPLAY, all, {4, 0, 0, 0, 1, 4, 1, 1, 1, 1, 0});
  expect("none shed", REPLAY_U, all, {4, 0, 0, 0, 1, 4, 1, 1, 1, 1, 0, 0, 0});
  expect("none shed", RET_REPLAY, all, {4, 0, 0, 0, 1, 4, 1, 1, 1, 1, 0, 0});
  expect("none shed", RET_REPLAY_U, all, {4, 0, 0, 0, 1, 4, 1, 1, 1, 1, 0, 0, 0, 0, 0});

  // ---- a mix, forms without copies: lanes 2 (wrong charge) and 5 (spent) are shed, six are verified --------------------------------------
  Batch mix; mix.pre = {0, 0, WRONG, 0, 0, SPENT, 0, 0}; mix.mv = 6; mix.cst = {0, 0, REJ, REJ, SPENT, UNSIGNED};
  mix.candidates = 2; mix.tc = {6, 2, 1, 1, 1, 1};
  expect("mix", ADMIT, mix, {8, 0, 1, 1, 6, 2, 1, 2});              // (the unsigned lane is in none of the last three)
  expect("mix", RETURN, mix, {8, 0, 1, 1, 6, 2, 1, 2, 0});
  expect("mix", REPLAY, mix, {8, 0, 1, 1, 2, 6, 2, 1, 1, 1, 1});
  expect("mix", RET_REPLAY, mix, {8, 0, 1, 1, 2, 6, 2, 1, 1, 1, 1, 0});
  Batch undet = mix; undet.cst[0] = UNDET;
  expect("mix, one undetermined", ADMIT, undet, {8, 0, 1, 1, 6, 2, 1, 1});

  // ---- the same lanes in the unique forms: lane 1 copies lane 0 (accepted: served), lane 4 copies lane 3 (rejected: a copy behind a
  // non-zero leader), lane 6 copies lane 0 and names another amount (answered DOUBLE_SPEND); lanes 0, 3 and 7 are verified ------------------
  Batch u; u.pre = mix.pre; u.mv = 3; u.cst = {0, REJ, UNSIGNED}; u.copies = 3;
  u.lead = {NONE, 0, NONE, NONE, 3, NONE, 0, NONE}; u.fin = {0, 0, WRONG, REJ, REJ, SPENT, SPENT, UNSIGNED};
  u.candidates = 0; u.tc = {3, 1, 1, 0, 0, 1};
  u.amounts = amounts_of({2, -2, 0, 0, 0, 0, 1, 3});      // lane 1 names l + 2: the amount of lane 0; lane 6 names 1
  expect("mix with copies", ADMIT_U, u, {8, 0, 1, 1, 3, 1, 0, 1, 3});
  expect("mix with copies", RETURN_U, u, {8, 0, 1, 1, 3, 1, 0, 1, 0, 3});
  expect("mix with copies", REPLAY_U, u, {8, 0, 1, 1, 0, 3, 1, 1, 0, 0, 1, 3, 1});
  expect("mix with copies", RET_REPLAY_U, u, {8, 0, 1, 1, 0, 3, 1, 1, 0, 0, 1, 0, 3, 1, 1});
  Batch u_null = u; u_null.amounts.clear();             // amounts null: every t is 0, no copy names another amount
  expect("mix with copies, amounts null", RET_REPLAY_U, u_null, {8, 0, 1, 1, 0, 3, 1, 1, 0, 0, 1, 0, 3, 1, 0});
  Batch u_big = u; u_big.pre[5] = BIG; u_big.fin[5] = BIG;
  expect("mix with copies, t > s", RET_REPLAY_U, u_big, {8, 0, 1, 0, 0, 3, 1, 1, 0, 0, 1, 1, 3, 1, 1});
  expect("mix with copies, t > s", RETURN_U, u_big, {8, 0, 1, 0, 3, 1, 0, 1, 1, 3});

  // ---- the replay tail ended before it ran over the verified lanes (tc[0] != mv): the replay forms report zeros ------------------------------
  Batch early = u; early.tc = {0, 0, 0, 0, 0, 0};
  expect("tail did not run", REPLAY_U, early, {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0});
  expect("tail did not run", RET_REPLAY_U, early, {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0});
  Batch early2 = mix; early2.tc = {5, 2, 1, 1, 1, 0};
  expect("tail did not run", REPLAY, early2, {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0});
  expect("tail did not run", RET_REPLAY, early2, {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0});
  expect("tail counts are not read without replay", ADMIT, early2, {8, 0, 1, 1, 6, 2, 1, 2});

  printf("ADMIT COUNTS CHECK: %d failures\n", failures);
  return failures ? 1 : 0;
}
