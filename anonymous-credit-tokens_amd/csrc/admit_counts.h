// admit_counts.h — the out_counts of the admission family as plain C++ (no GPU runtime), beside wire_window.h: which of the eight count
// arrays of include/act_mi355x.h a form fills, and every value in it, from host arrays alone.  The engine (admit_impl.inc) brings the
// arrays to the host and calls admit_counts once per exit; tests/hostcheck/admit_counts_check.cpp calls it under g++.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include "../../include/act_mi355x.h"
#include "copy_lanes.h"

namespace act {

// unique: the copy stage; replay: receipts and the replay tail; ret: returned amounts (RefundReturn outputs)
struct AdmitForm { bool unique, replay, ret; };

inline size_t admit_counts_len(const AdmitForm& f) {
  static constexpr size_t len[2][2][2] = {      // [replay][ret][unique]
    {{ACT_ADMIT_COUNTS, ACT_ADMIT_UNIQUE_COUNTS}, {ACT_REDEEM_RETURN_COUNTS, ACT_REDEEM_RETURN_UNIQUE_COUNTS}},
    {{ACT_ADMIT_REPLAY_COUNTS, ACT_ADMIT_REPLAY_UNIQUE_COUNTS}, {ACT_RETURN_REPLAY_COUNTS, ACT_RETURN_REPLAY_UNIQUE_COUNTS}}};
  return len[f.replay][f.ret][f.unique];
}

// What a call knows when it ends.  Nothing shed: mv = n; everything shed: mv = 0 and cst / tc null.
struct AdmitCountsIn {
  size_t n; const uint8_t* pre;                  // the lanes and their final pre-statuses (0: verified, or a copy of a verified lane)
  size_t mv; const uint8_t* cst;                 // the verified lanes; their statuses in compact order (read by the forms without replay)
  size_t candidates; const uint64_t* tc;         // replay: the retry candidates; the tail's ACT_REPLAY_COUNTS over the mv lanes
  size_t copies;                                 // unique: the lanes that were not verified because an earlier lane has their bytes
  const uint32_t* lead; const uint8_t* fin;      // replay && unique && copies: every lane's leader (COPY_NONE: none), the final statuses
  const uint8_t* amounts;                        // ... && ret: the n returned amounts (null: every copy names its leader's)
};

// out: admit_counts_len(f) values.  A replay form whose tail did not run over all mv lanes (tc[0] != mv) reports zeros.
inline void admit_counts(const AdmitForm& f, const AdmitCountsIn& in, uint64_t* out) {
  const size_t len = admit_counts_len(f), base = admit_counts_len({false, f.replay, f.ret});
  memset(out, 0, sizeof(uint64_t) * len);
  if (f.replay && in.tc && in.tc[0] != in.mv) return;
  const size_t too_big = f.replay ? ACT_ADMIT_REPLAY_COUNTS : ACT_ADMIT_COUNTS;      // where the return forms count t > s
  out[0] = in.n;
  for (size_t i = 0; i < in.n; i++) {            // wire_rejected, wrong_charge, spent_before / foreign_spend
    const uint8_t p = in.pre[i];
    if (p == ACT_STATUS_WRONG_CHARGE) out[2]++; else if (p == ACT_STATUS_DOUBLE_SPEND) out[3]++; else if (f.ret && p == ACT_STATUS_RETURN_TOO_BIG) out[too_big]++; else if (p) out[1]++;
  }
  if (f.replay) {
    out[4] = in.candidates; out[5] = in.mv;
    if (in.tc) for (int j = 0; j < 5; j++) out[6 + j] = in.tc[1 + j];      // rejected_by_verification, fresh, replayed, double_spend_after, unanswered
  } else {
    out[4] = in.mv;
    for (size_t j = 0; j < in.mv; j++) {         // rejected_by_verification, double_spend_after, accepted
      const uint8_t s = in.cst[j];
      if (s == 0) out[7]++; else if (s == ACT_STATUS_DOUBLE_SPEND) out[6]++;
      else if (s != ACT_STATUS_NULLIFIER_UNDETERMINED && s != ACT_STATUS_RECORDED_UNSIGNED) out[5]++;
    }
  }
  if (!f.unique) return;
  out[base] = in.copies;
  if (!f.replay || !in.copies) return;
  for (size_t i = 0; i < in.n; i++) {            // copies_served, and the copies that name another amount than their leader
    if (in.lead[i] == COPY_NONE) continue;
    out[base + 1] += in.fin[i] == 0;
    if (f.ret && in.amounts) out[base + 2] += !copy_same_amount(in.amounts + i * 32, in.amounts + (size_t)in.lead[i] * 32);
  }
}

}  // namespace act
