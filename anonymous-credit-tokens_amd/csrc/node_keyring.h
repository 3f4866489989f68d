// node_keyring.h -- the body of the node-level ring redemption (node_keyring.cpp), shared with node_epochs.cpp.
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include "../../include/act_mi355x.h"

namespace act_node_keyring {
// the nullifier step of a redemption: (set, n, nullifiers, stride, skip_mask = the verdicts, out_key, out_spent) -> rc
using NullStep = std::function<int(act_node_nullifier_set*, size_t, const uint8_t*, size_t, const uint8_t*, const uint8_t*, uint8_t*)>;
// records (proof) or wire bytes (cbor + offsets) in; null_step nullable = act_node_nullifier_check_and_insert_batch
int redeem(act_node* nd, act_node_nullifier_set* set, size_t n, const uint8_t* keys, int nkeys, int sign_key, const uint8_t* proof, const uint8_t* cbor,
           const uint64_t* offsets, const uint8_t* rng, int rng_mode, uint8_t* out, uint8_t* status, uint8_t* out_key, const NullStep* null_step);
}  // namespace act_node_keyring
