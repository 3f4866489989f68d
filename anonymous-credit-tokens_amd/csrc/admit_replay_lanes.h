// admit_replay_lanes.h — the per-lane bodies of the admission stage of the replayable redemption (k_admit_replay.hip; engine side in
// admit_replay_impl.inc), as functions that also compile under g++ (tests/hostcheck/admit_replay_check.cpp runs and sanitizes them;
// the admit_lanes.h / replay_lanes.h pattern).
//
// A lane whose nullifier is spent is a retry or a double spend, and the receipts can tell which without a verification:
// the receipt's tag needs k and enc(K'), and K' = sum_j 2^j Com_j is a function of the proof's bytes alone.
//   admit_replay_key_lane     lane = item             the key of the spent lanes' compaction (0 = spent at the screen)
//   kprime_decode_lane        lane = (candidate, j)   Com_j -> affine Niels: spend_coords_lane itself, over the gathered records
//   kprime_tag_lane           lane = candidate        Horner (spend_tail_horner) -> enc(K') -> tag (replay_tag); a mark where a Com_j failed
//   admit_replay_decide_lane  lane = item             (pre-status, spent, undecodable, found) -> final pre-status
// Nothing is restated: the point arithmetic is spend_lanes.h's, the hash replay_lanes.h's.  The stage never accepts anything -- a
// candidate goes on to verification like a fresh lane.
#pragma once
#include "spend_lanes.h"
#include "admit_lanes.h"
#include "replay_lanes.h"

namespace act {

// ---- the decision ---------------------------------------------------------------------------------------------------------------------
// pre: the screen's answer (admit_decide); spent: the screen found k in the set (then pre is ADMIT_DOUBLE_SPEND); undecodable: a Com_j
// of the lane is no point; found: the receipts hold the lane's tag.  Only a spent lane is touched: it is a retry candidate (pre-status
// 0: verified like a fresh lane) when its tag is there, and stays a double spend otherwise.
struct AdmitReplayDecision { uint8_t pre; uint8_t candidate; };
ACT_HD AdmitReplayDecision admit_replay_decide(uint8_t pre, bool spent, bool undecodable, bool found) {
  if (!spent) return AdmitReplayDecision{pre, 0};
  if (undecodable || !found) return AdmitReplayDecision{ADMIT_DOUBLE_SPEND, 0};
  return AdmitReplayDecision{0, 1};
}
ACT_HD bool admit_replay_spent(uint8_t pre) { return pre == ADMIT_DOUBLE_SPEND; }      // (the wire reader's codes are 253 / 254 / 255)

// the compaction of admit_lanes.h keeps the lanes whose byte is 0
struct AdmitReplayKeyArgs { uint32_t n; const uint8_t* pre; uint8_t* key; };
ACT_HD void admit_replay_key_lane(const AdmitReplayKeyArgs& a, uint32_t i) {
  if (i >= a.n) return;
  a.key[i] = admit_replay_spent(a.pre[i]) ? 0 : 1;
}

// pos: the lane's place among the spent lanes (ADMIT_SHED: not spent); mark / found: per spent lane
struct AdmitReplayDecideArgs { uint32_t n; const uint32_t* pos; const uint8_t* mark; const uint8_t* found; uint8_t* pre; };
ACT_HD void admit_replay_decide_lane(const AdmitReplayDecideArgs& a, uint32_t i) {
  if (i >= a.n) return;
  const uint32_t c = a.pos[i];
  const bool spent = c != ADMIT_SHED;
  a.pre[i] = admit_replay_decide(a.pre[i], spent, spent && a.mark[c] != 0, spent && a.found[c] != 0).pre;
}

// ---- enc(K') and the tag of a candidate ---------------------------------------------------------------------------------------------------
// s: P.L, proofs (the window's gathered records), n, coords (n * L * NIELS_WORDS words) and flags (n words, zero before the decode) are
// used, nothing else -- no key, no transcript, no table.
struct KprimeArgs {
  SpendArgs s;
  const uint8_t* kred; const uint32_t* idx;      // candidate c's reduced nullifier at kred + idx[c] * 32 (idx null: kred + c * 32)
  uint8_t* kp; uint8_t* tag; uint8_t* mark;      // n * 32, n * 32, n: enc(K'), the tag, 1 where a Com_j did not decode (then both are zero)
  const uint8_t* t;                              // the return form (return_replay_lanes.h) only: candidate c's returned amount at t + idx[c] * 32, nullable
};
ACT_HD void kprime_decode_lane(const KprimeArgs& a, uint32_t gid) { spend_coords_lane(a.s, gid); }
ACT_HD void kprime_tag_lane(const KprimeArgs& a, uint32_t c) {
  if (c >= a.s.n) return;
  uint32_t enc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const bool bad = (a.s.flags[c] & FLAG_UNDECODABLE) != 0;
  if (!bad) {
    uint32_t k[8];
    ristretto_encode(enc, spend_tail_horner(a.s, c, 0, a.s.P.L, 0));
    null_load_key(k, a.kred + (size_t)(a.idx ? a.idx[c] : c) * 32);
    replay_tag(t, k, enc);
  }
  store32_bytes(a.kp + (size_t)c * 32, enc);
  store32_bytes(a.tag + (size_t)c * 32, t);
  a.mark[c] = bad ? 1 : 0;
}

#if defined(__HIPCC__)
// launchers (k_admit_replay.hip)
void launch_admit_replay_key(const AdmitReplayKeyArgs& a, hipStream_t s);
void launch_kprime_decode(const KprimeArgs& a, hipStream_t s);      // 64 lanes per workgroup, as k_spend_coords
void launch_kprime_tag(const KprimeArgs& a, hipStream_t s);
void launch_admit_replay_decide(const AdmitReplayDecideArgs& a, hipStream_t s);
#endif

}  // namespace act
