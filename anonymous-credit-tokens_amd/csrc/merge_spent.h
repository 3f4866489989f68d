// merge_spent.h -- what a lane's verdict and the nullifier store's answer make of the lane: the one definition behind the engine's
// host loops, its k_merge_double_spend (nullifier_impl.inc) and the node forms (node.cpp).
#pragma once
#include <cstdint>
#include "../../include/act_mi355x.h"
#ifdef __HIPCC__
#define ACT_MERGE_HD __host__ __device__
#else
#define ACT_MERGE_HD
#endif

// verdict 0 + spent 1 -> DoubleSpendError; verdict 0 + undetermined -> ACT_STATUS_NULLIFIER_UNDETERMINED (neither recorded nor signed)
ACT_MERGE_HD inline uint8_t merge_spent(uint8_t verdict, uint8_t spent) {
  if (verdict != 0 || spent == 0) return verdict;
  return spent == 1 ? (uint8_t)ACT_STATUS_DOUBLE_SPEND : (uint8_t)ACT_STATUS_NULLIFIER_UNDETERMINED;
}
