// node_nullifier.cpp -- growth, export and read-only look-up of the node-level nullifier set (include/act_mi355x.h; the set itself,
// its routing and check-and-insert: node.cpp).
#include <cstring>
#include "node_nullifier.h"

using act_node_null::bucket_by_owner;
using act_node_null::per_device;

extern "C" {
int act_node_nullifier_contains_batch(act_node_nullifier_set* ns, size_t n, const uint8_t* nullifiers, size_t stride, uint8_t* out_found) {
  if (!ns || (n && (!nullifiers || !out_found)) || stride < 32) return ACT_ERR_ARG;
  std::lock_guard<std::mutex> lock(ns->mu);
  bucket_by_owner(ns, n, nullifiers, stride, nullptr, out_found);
  std::vector<int> rc = per_device(ns, [&](size_t p, act_node_nullifier_set::Bucket& b) {
    return act_nullifier_contains_batch(ns->sets[p], b.count, ACT_MEM_HOST, b.keys.data(), 32, b.spent.data());
  });
  int first_rc = ACT_OK;
  ns->err.clear();
  for (size_t p = 0; p < ns->sets.size(); p++) {
    if (rc[p]) {                                   // this device's lanes stay 0 (not known); the call fails
      if (!first_rc) first_rc = rc[p];
      ns->err += (ns->err.empty() ? "device " : "; device ") + std::to_string(ns->devices[p]) + ": " + act_nullifier_set_last_error(ns->sets[p]);
      continue;
    }
    for (size_t j = 0; j < ns->buckets[p].count; j++) out_found[ns->buckets[p].lanes[j]] = ns->buckets[p].spent[j];
  }
  return first_rc;
}

int act_node_nullifier_set_reserve(act_node_nullifier_set* ns, size_t capacity_per_device) {
  if (!ns) return ACT_ERR_ARG;
  std::lock_guard<std::mutex> lock(ns->mu);
  int first_rc = ACT_OK;
  ns->err.clear();
  for (size_t p = 0; p < ns->sets.size(); p++) {  // one device after the other: a failure leaves every set valid, the earlier ones grown
    const int rc = act_nullifier_set_reserve(ns->sets[p], capacity_per_device);
    if (rc) {
      if (!first_rc) first_rc = rc;
      ns->err += (ns->err.empty() ? "device " : "; device ") + std::to_string(ns->devices[p]) + ": " + act_nullifier_set_last_error(ns->sets[p]);
    }
  }
  return first_rc;
}

// Node cursor: device index << kCursorShift | that device's set cursor (node_nullifier.h); the device's own cursor check refuses one
// that stopped inside a set that has been grown, or has had an epoch retired, since.
int act_node_nullifier_set_export(act_node_nullifier_set* ns, uint64_t* cursor, size_t max_keys, uint8_t* out_keys, size_t* n_out) {
  if (!ns || !cursor || !n_out || !max_keys || !out_keys) return ACT_ERR_ARG;
  std::lock_guard<std::mutex> lock(ns->mu);
  *n_out = 0;
  if (*cursor == ACT_NULLIFIER_EXPORT_DONE) return ACT_OK;
  const uint64_t part = *cursor >> act_node_null::kCursorShift;
  if (part >= ns->sets.size()) { ns->err = "act_node_nullifier_set_export: foreign cursor"; return ACT_ERR_ARG; }
  uint64_t inner = *cursor & ((1ull << act_node_null::kCursorShift) - 1);
  const int rc = act_nullifier_set_export(ns->sets[part], &inner, max_keys, ACT_MEM_HOST, out_keys, n_out);
  if (rc) { ns->err = "device " + std::to_string(ns->devices[part]) + ": " + act_nullifier_set_last_error(ns->sets[part]); return rc; }
  if (inner != ACT_NULLIFIER_EXPORT_DONE) *cursor = part << act_node_null::kCursorShift | inner;
  else *cursor = part + 1 < ns->sets.size() ? (part + 1) << act_node_null::kCursorShift : ACT_NULLIFIER_EXPORT_DONE;
  return ACT_OK;
}
}  // extern "C"
