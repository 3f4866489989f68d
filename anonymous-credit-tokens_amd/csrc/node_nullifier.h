// node_nullifier.h -- the node-level nullifier set's state and routing helpers, shared by node.cpp (create, check-and-insert) and
// node_nullifier.cpp (reserve, export, contains).  The CPU test builds link node.cpp against a mock engine that has only the
// single-GPU calls node.cpp itself uses, so the calls that need more of the engine live in their own translation unit.
#pragma once
#include <cstdint>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "../../include/act_mi355x.h"

// The node-level set (design: node.cpp, "the double-spend set over the GPUs of a node").
struct act_node_nullifier_set {
  std::vector<act_nullifier_set*> sets;
  std::vector<int> devices;
  uint64_t route_key[2] = {0, 0};
  std::string err;
  std::mutex mu;
  // routing scratch, kept between calls (under mu) and only ever grown: a fresh 32 MB of key buckets per million-key call would
  // be page-faulted in by one thread every time
  struct Bucket { std::vector<uint32_t> lanes; std::vector<uint8_t> keys, spent; size_t count = 0; };
  std::vector<Bucket> buckets;
  std::vector<uint16_t> owner;
  std::vector<size_t> place;
};


namespace act_node_null {
// Node export cursor: device index << kCursorShift | that device's set cursor (which is below 2^51 until it is
// ACT_NULLIFIER_EXPORT_DONE; at most 4096 devices, so a node cursor never reaches ACT_NULLIFIER_EXPORT_DONE by itself).
constexpr int kCursorShift = 51;
// The keys of a call bucketed by owner (ns->buckets, lane order kept inside every bucket); out[i] = 0 for every lane.  Caller holds ns->mu.
void bucket_by_owner(act_node_nullifier_set* ns, size_t n, const uint8_t* nullifiers, size_t stride, const uint8_t* skip_mask, uint8_t* out);
// every device's bucket through `call` on its own thread, in parallel; rc per device
template <class F>
std::vector<int> per_device(act_node_nullifier_set* ns, F call) {
  const size_t parts = ns->sets.size();
  std::vector<int> rc(parts, ACT_OK);
  std::vector<std::thread> th;
  auto work = [&](size_t p) { if (ns->buckets[p].count) rc[p] = call(p, ns->buckets[p]); };
  for (size_t p = 1; p < parts; p++) th.emplace_back(work, p);
  work(0);
  for (auto& t : th) t.join();
  return rc;
}
}  // namespace act_node_null
