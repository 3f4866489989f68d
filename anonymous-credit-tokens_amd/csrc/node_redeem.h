// node_redeem.h -- what the node files share: node.cpp's dispatcher as the translation units beside it see it (node_keyring.cpp,
// node_issue_wire.cpp), and the one body every node-level redeem call ends in (redeem_tail, defined in node.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <vector>
#include "../../include/act_mi355x.h"

namespace act_node_dispatch {
struct Piece { size_t k, off, m; int rc; };       // lanes [off, off + m) ran (or were to run: k == SIZE_MAX) on context k with result rc
// The handle's dispatcher (weights, tail) under the handle's lock: fn(context, off, m) per piece.  `pieces` (optional) receives what
// ran where and how it ended, and -- with k == SIZE_MAX -- whatever nobody ran because every context had failed.
int run_pieces(act_node* nd, size_t n, const std::function<int(act_ctx*, size_t, size_t)>& fn, std::vector<Piece>* pieces = nullptr);

inline const uint8_t* at(const uint8_t* p, size_t off, size_t rec) { return p ? p + off * rec : nullptr; }
inline uint8_t* at(uint8_t* p, size_t off, size_t rec) { return p ? p + off * rec : nullptr; }
inline size_t count_zero(const uint8_t* st, size_t n) { size_t a = 0; for (size_t i = 0; i < n; i++) a += st[i] == 0; return a; }

// Everything behind verification, for the one-key, ring and epoch forms alike: the node-level nullifier set over the whole batch in
// lane order with the verdicts as skip mask, the store's answers merged into `verdict`, the caller's generator touched only now and
// only for the lanes that are signed, the signatures over the pieces.  Failures never lose a decision (act_redeem_batch's contract):
// a device of the set that fails leaves ITS lanes ACT_STATUS_NULLIFIER_UNDETERMINED (not recorded, not signed); a GPU that fails
// while signing leaves the lanes of ITS pieces that were to be signed ACT_STATUS_RECORDED_UNSIGNED (recorded, refund owed), a failing
// generator all of them, their output slots (out_rec bytes each) zero; every other lane is finished and the error code is returned.
//   null_step(skip_mask = verdict, out_spent) -> rc
//   sign_step(verdict, rng, rng_mode, pieces) -> rc      rng already resolved to bytes; writes out / status; `pieces` as run_pieces
//                                                        fills it.  Called WITHOUT the handle's lock: run_pieces takes it itself.
using NullFn = std::function<int(const uint8_t*, uint8_t*)>;
using SignFn = std::function<int(const uint8_t*, const uint8_t*, int, std::vector<Piece>*)>;
int redeem_tail(act_node* nd, act_node_nullifier_set* set, size_t n, size_t out_rec, uint8_t* verdict, const uint8_t* rng, int rng_mode, uint8_t* out, uint8_t* status,
                const NullFn& null_step, const SignFn& sign_step);
}  // namespace act_node_dispatch
