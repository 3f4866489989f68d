// node_epochs.cpp -- nullifier epochs over the GPUs of a node (include/act_mi355x.h act_node_nullifier_*epoch*, act_node_redeem_*_epochs_batch).
// A translation unit of its own, like node_nullifier.cpp: the CPU test builds link node.cpp and node_keyring.cpp against stand-ins
// that have only the single-GPU calls those two use.  Routing is node.cpp's (bucket_by_owner); the ring redemption is
// node_keyring.cpp's body with the nullifier step handed in.
#include <algorithm>
#include <cstring>
#include <iterator>
#include <string>
#include "node_keyring.h"
#include "node_nullifier.h"

using act_node_null::bucket_by_owner;
using act_node_null::kCursorShift;
using act_node_null::per_device;

namespace {
std::string device_err(act_node_nullifier_set* ns, size_t p) { return "device " + std::to_string(ns->devices[p]) + ": " + act_nullifier_set_last_error(ns->sets[p]); }
void add_err(act_node_nullifier_set* ns, size_t p) { ns->err += (ns->err.empty() ? "" : "; ") + device_err(ns, p); }

// the epochs device p has retired, ascending
int retired_of(act_node_nullifier_set* ns, size_t p, std::vector<uint32_t>& out) {
  size_t have = 0;
  int rc = act_nullifier_set_retired_epochs(ns->sets[p], nullptr, 0, &have);
  out.assign(have, 0);
  if (!rc && have) rc = act_nullifier_set_retired_epochs(ns->sets[p], out.data(), have, &have);
  if (!rc) out.resize(std::min(out.size(), have));
  return rc;
}
// "" if every epoch of the table may be recorded under on every device, else why not (an epoch ANY device has retired is refused: a
// retirement that stopped half way must not let keys of that epoch back in).  Caller holds ns->mu.
std::string epochs_refused(act_node_nullifier_set* ns, const uint32_t* tab, int n_epochs) {
  for (int k = 0; k < n_epochs; k++) if (tab[k] > ACT_NULLIFIER_EPOCH_MAX) return "epoch " + std::to_string(tab[k]) + " is above ACT_NULLIFIER_EPOCH_MAX";
  std::vector<uint32_t> r;
  for (size_t p = 0; p < ns->sets.size(); p++) {
    if (retired_of(ns, p, r)) return device_err(ns, p);
    for (int k = 0; k < n_epochs; k++)
      if (std::binary_search(r.begin(), r.end(), tab[k])) return "epoch " + std::to_string(tab[k]) + " has been retired (device " + std::to_string(ns->devices[p]) + ")";
  }
  return std::string();
}

int insert_epochs(act_node_nullifier_set* ns, size_t n, const uint8_t* nullifiers, size_t stride, const uint8_t* skip_mask, const uint8_t* epoch_index,
                  const uint32_t* epoch_table, int n_epochs, uint8_t* out_spent) {
  if (!ns || (n && (!nullifiers || !out_spent)) || stride < 32 || !epoch_table || n_epochs < 1 || n_epochs > 255) return ACT_ERR_ARG;
  std::lock_guard<std::mutex> lock(ns->mu);
  const std::string why = epochs_refused(ns, epoch_table, n_epochs);
  if (!why.empty()) {      // refused as a whole: nothing recorded, every unmasked lane undetermined
    ns->err = "nullifier set: " + why;
    for (size_t i = 0; i < n; i++) out_spent[i] = (skip_mask && skip_mask[i]) ? 0 : ACT_NULLIFIER_UNDETERMINED;
    return ACT_ERR_ARG;
  }
  const size_t parts = ns->sets.size();
  bucket_by_owner(ns, n, nullifiers, stride, skip_mask, out_spent);
  std::vector<std::vector<uint8_t>> eidx(epoch_index ? parts : 0);      // the bucket's lanes' epoch indices, in the bucket's order
  for (size_t p = 0; p < eidx.size(); p++) {
    const auto& b = ns->buckets[p];
    eidx[p].resize(b.count);
    for (size_t j = 0; j < b.count; j++) eidx[p][j] = epoch_index[b.lanes[j]];
  }
  std::vector<int> rc = per_device(ns, [&](size_t p, act_node_nullifier_set::Bucket& b) {
    return act_nullifier_check_and_insert_epoch_batch(ns->sets[p], b.count, ACT_MEM_HOST, b.keys.data(), 32, nullptr, epoch_index ? eidx[p].data() : nullptr,
                                                      epoch_table, n_epochs, b.spent.data());
  });
  // As in act_node_nullifier_check_and_insert_batch: the devices that answered have answered for good.  ACT_ERR_ARG from a device is
  // an answer too -- it has written every lane (undetermined where it refused: no room for the bucket, or an index outside the table).
  int first_rc = ACT_OK;
  ns->err.clear();
  for (size_t p = 0; p < parts; p++) {
    const auto& b = ns->buckets[p];
    if (rc[p]) { if (!first_rc) first_rc = rc[p]; add_err(ns, p); }
    const bool answered = rc[p] == ACT_OK || rc[p] == ACT_ERR_ARG;
    for (size_t j = 0; j < b.count; j++) out_spent[b.lanes[j]] = answered ? b.spent[j] : (uint8_t)ACT_NULLIFIER_UNDETERMINED;
  }
  return first_rc;
}

int redeem_epochs(act_node* nd, act_node_nullifier_set* set, size_t n, const uint8_t* keys, int nkeys, const uint32_t* key_epochs, int sign_key,
                  const uint8_t* proof, const uint8_t* cbor, const uint64_t* offsets, const uint8_t* rng, int rng_mode, uint8_t* out, uint8_t* status, uint8_t* out_key) {
  if (!nd || !set || !keys || !key_epochs || nkeys < 1 || nkeys > ACT_KEYRING_MAX) return ACT_ERR_ARG;
  {      // refused before any verification work: nothing recorded, nothing signed, no status written
    std::lock_guard<std::mutex> lock(set->mu);
    const std::string why = epochs_refused(set, key_epochs, nkeys);
    if (!why.empty()) { set->err = "act_node_redeem_keyring_epochs_batch: " + why; return ACT_ERR_ARG; }
  }
  // out_key, as the ring verification leaves it, is the epoch index: the epoch of the key the proof matched
  const act_node_keyring::NullStep step = [&](act_node_nullifier_set* s, size_t m, const uint8_t* nul, size_t stride, const uint8_t* mask, const uint8_t* matched,
                                              uint8_t* spent) { return insert_epochs(s, m, nul, stride, mask, matched, key_epochs, nkeys, spent); };
  return act_node_keyring::redeem(nd, set, n, keys, nkeys, sign_key, proof, cbor, offsets, rng, rng_mode, out, status, out_key, &step);
}
}  // namespace

extern "C" {

int act_node_nullifier_check_and_insert_epoch_batch(act_node_nullifier_set* ns, size_t n, const uint8_t* nullifiers, size_t stride, const uint8_t* skip_mask,
                                                    const uint8_t* epoch_index, const uint32_t* epoch_table, int n_epochs, uint8_t* out_spent) {
  return insert_epochs(ns, n, nullifiers, stride, skip_mask, epoch_index, epoch_table, n_epochs, out_spent);
}

int act_node_nullifier_set_epoch_len(act_node_nullifier_set* ns, uint32_t epoch, uint64_t* out_count) {
  if (!ns || !out_count) return ACT_ERR_ARG;
  std::lock_guard<std::mutex> lock(ns->mu);
  *out_count = 0;
  for (size_t p = 0; p < ns->sets.size(); p++) {
    uint64_t c = 0;
    const int rc = act_nullifier_set_epoch_len(ns->sets[p], epoch, &c);
    if (rc) { ns->err = device_err(ns, p); *out_count = 0; return rc; }
    *out_count += c;
  }
  return ACT_OK;
}

int act_node_nullifier_set_retire_epoch(act_node_nullifier_set* ns, uint32_t epoch, uint64_t* out_removed) {
  if (!ns) return ACT_ERR_ARG;
  std::lock_guard<std::mutex> lock(ns->mu);
  if (out_removed) *out_removed = 0;
  int first_rc = ACT_OK;
  ns->err.clear();
  for (size_t p = 0; p < ns->sets.size(); p++) {  // one device after the other: a failure leaves every set valid, some already retired;
    uint64_t gone = 0;                            // the call is idempotent per device, so a repeat finishes the job
    const int rc = act_nullifier_set_retire_epoch(ns->sets[p], epoch, &gone);
    if (rc) { if (!first_rc) first_rc = rc; add_err(ns, p); }
    else if (out_removed) *out_removed += gone;
  }
  return first_rc;
}

int act_node_nullifier_set_retired_epochs(act_node_nullifier_set* ns, uint32_t* out_epochs, size_t max_epochs, size_t* n_out) {
  if (!ns || !n_out || (max_epochs && !out_epochs)) return ACT_ERR_ARG;
  std::lock_guard<std::mutex> lock(ns->mu);
  *n_out = 0;
  std::vector<uint32_t> all, r, both;      // retired for the node = retired on every device
  for (size_t p = 0; p < ns->sets.size(); p++) {
    const int rc = retired_of(ns, p, r);
    if (rc) { ns->err = device_err(ns, p); return rc; }
    if (p == 0) { all = r; continue; }
    both.clear();
    std::set_intersection(all.begin(), all.end(), r.begin(), r.end(), std::back_inserter(both));
    all.swap(both);
  }
  *n_out = all.size();
  for (size_t i = 0; i < std::min(max_epochs, all.size()); i++) out_epochs[i] = all[i];
  return ACT_OK;
}

// The cursor of act_node_nullifier_set_export (node_nullifier.cpp): either call may continue the other's.
int act_node_nullifier_set_export_epochs(act_node_nullifier_set* ns, uint64_t* cursor, size_t max_keys, uint8_t* out_keys, uint32_t* out_epochs, size_t* n_out) {
  if (!ns || !cursor || !n_out || !max_keys || !out_keys || !out_epochs) return ACT_ERR_ARG;
  std::lock_guard<std::mutex> lock(ns->mu);
  *n_out = 0;
  if (*cursor == ACT_NULLIFIER_EXPORT_DONE) return ACT_OK;
  const uint64_t part = *cursor >> kCursorShift;
  if (part >= ns->sets.size()) { ns->err = "act_node_nullifier_set_export_epochs: foreign cursor"; return ACT_ERR_ARG; }
  uint64_t inner = *cursor & ((1ull << kCursorShift) - 1);
  const int rc = act_nullifier_set_export_epochs(ns->sets[part], &inner, max_keys, ACT_MEM_HOST, out_keys, out_epochs, n_out);
  if (rc) { ns->err = device_err(ns, part); return rc; }
  if (inner != ACT_NULLIFIER_EXPORT_DONE) *cursor = part << kCursorShift | inner;
  else *cursor = part + 1 < ns->sets.size() ? (part + 1) << kCursorShift : ACT_NULLIFIER_EXPORT_DONE;
  return ACT_OK;
}

int act_node_redeem_keyring_epochs_batch(act_node* nd, act_node_nullifier_set* set, size_t n, const uint8_t* keys, int nkeys, const uint32_t* key_epochs, int sign_key,
                                         const uint8_t* proof, const uint8_t* rng, int rng_mode, uint8_t* out_refund, uint8_t* status, uint8_t* out_key) {
  if (n && !proof) return ACT_ERR_ARG;
  return redeem_epochs(nd, set, n, keys, nkeys, key_epochs, sign_key, proof, nullptr, nullptr, rng, rng_mode, out_refund, status, out_key);
}
int act_node_redeem_cbor_keyring_epochs_batch(act_node* nd, act_node_nullifier_set* set, size_t n, const uint8_t* keys, int nkeys, const uint32_t* key_epochs,
                                              int sign_key, const uint8_t* cbor, const uint64_t* offsets, const uint8_t* rng, int rng_mode, uint8_t* out_refund_cbor,
                                              uint8_t* status, uint8_t* out_key) {
  if (n && !cbor) return ACT_ERR_ARG;
  static const uint8_t none = 0;
  return redeem_epochs(nd, set, n, keys, nkeys, key_epochs, sign_key, nullptr, cbor ? cbor : &none, offsets, rng, rng_mode, out_refund_cbor, status, out_key);
}

}  // extern "C"
