// node_mock_epochs.cpp — TEST-ONLY stand-ins for the single-GPU epoch calls that csrc/node_epochs.cpp uses, on top of node_mock.cpp
// (included, so that this file sees its act_nullifier_set and its failure switch): tests/test_nullifier_epochs_node_cpu.py links
// node.cpp + node_keyring.cpp + node_epochs.cpp + this file + node_mock_keyring.cpp.
//
// The epochs live beside the existing stand-in's key set: per set, reduced key -> epoch for every key recorded under a non-zero epoch,
// and the retired list.  act_mock_epochs_fail(device, what): the set on `device` fails its next calls of kind `what` (1 = retire,
// 2 = insert) with ACT_ERR_HIP and changes nothing; -1 = none.
#include "../node_mock/node_mock.cpp"

namespace {
struct Side { std::map<std::vector<uint8_t>, uint32_t> epoch; std::set<uint32_t> retired; };
std::map<const act_nullifier_set*, Side> g_side;
std::mutex g_side_mu;
int g_fail_epoch_device = -1, g_fail_epoch_what = 0;

Side& side(const act_nullifier_set* s) { std::lock_guard<std::mutex> lk(g_side_mu); return g_side[s]; }
std::vector<uint8_t> reduced(const uint8_t* k) {
  static const uint64_t Lw[4] = {0x5812631a5cf5d3edull, 0x14def9dea2f79cd6ull, 0, 0x1000000000000000ull};
  uint64_t v[4]; memcpy(v, k, 32);
  for (;;) {
    uint64_t t[4]; unsigned __int128 b = 0;
    for (int j = 0; j < 4; j++) { unsigned __int128 d = (unsigned __int128)v[j] - Lw[j] - (uint64_t)b; t[j] = (uint64_t)d; b = (d >> 64) & 1; }
    if (b) break;
    memcpy(v, t, 32);
  }
  std::vector<uint8_t> key(32); memcpy(key.data(), v, 32);
  return key;
}
}  // namespace

extern "C" {
void act_mock_epochs_fail(int device, int what) { g_fail_epoch_device = device; g_fail_epoch_what = what; }

int act_nullifier_check_and_insert_epoch_batch(act_nullifier_set* s, size_t n, int, const uint8_t* k, size_t stride, const uint8_t* mask, const uint8_t* eidx,
                                               const uint32_t* tab, int n_epochs, uint8_t* spent) {
  if (!tab || n_epochs < 1 || n_epochs > 255) return ACT_ERR_ARG;
  if (s->device == g_fail_null_device || (s->device == g_fail_epoch_device && g_fail_epoch_what == 2)) { s->err = "mock: device lost"; return ACT_ERR_HIP; }
  Side& sd = side(s);
  bool refused = false;
  for (int e = 0; e < n_epochs; e++) refused |= tab[e] > ACT_NULLIFIER_EPOCH_MAX || sd.retired.count(tab[e]);
  if (refused) {
    s->err = "mock: epoch refused";
    for (size_t i = 0; i < n; i++) spent[i] = (mask && mask[i]) ? 0 : ACT_NULLIFIER_UNDETERMINED;
    return ACT_ERR_ARG;
  }
  bool bad = false;
  for (size_t i = 0; i < n; i++) {
    if (mask && mask[i]) { spent[i] = 0; continue; }
    const uint8_t ix = eidx ? eidx[i] : 0;
    if (ix >= n_epochs) { spent[i] = ACT_NULLIFIER_UNDETERMINED; bad = true; continue; }
    const std::vector<uint8_t> key = reduced(k + i * stride);
    spent[i] = !s->keys.insert(key).second;
    if (!spent[i] && tab[ix]) sd.epoch[key] = tab[ix];
  }
  if (bad) s->err = "mock: epoch index not below n_epochs";
  return bad ? ACT_ERR_ARG : ACT_OK;
}

int act_nullifier_set_epoch_len(act_nullifier_set* s, uint32_t epoch, uint64_t* out) {
  Side& sd = side(s);
  uint64_t c = 0;
  if (epoch == 0) c = s->keys.size() - sd.epoch.size();
  else for (const auto& kv : sd.epoch) c += kv.second == epoch;
  *out = c;
  return ACT_OK;
}

int act_nullifier_set_retire_epoch(act_nullifier_set* s, uint32_t epoch, uint64_t* out_removed) {
  if (out_removed) *out_removed = 0;
  if (epoch == 0 || epoch > ACT_NULLIFIER_EPOCH_MAX) { s->err = "mock: epoch cannot be retired"; return ACT_ERR_ARG; }
  if (s->device == g_fail_epoch_device && g_fail_epoch_what == 1) { s->err = "mock: no memory for the new table"; return ACT_ERR_HIP; }
  Side& sd = side(s);
  uint64_t gone = 0;
  for (auto it = sd.epoch.begin(); it != sd.epoch.end();) {
    if (it->second == epoch) { s->keys.erase(it->first); it = sd.epoch.erase(it); gone++; }
    else ++it;
  }
  sd.retired.insert(epoch);
  if (out_removed) *out_removed = gone;
  return ACT_OK;
}

int act_nullifier_set_retired_epochs(act_nullifier_set* s, uint32_t* out, size_t max_epochs, size_t* n_out) {
  Side& sd = side(s);
  *n_out = sd.retired.size();
  size_t i = 0;
  for (uint32_t e : sd.retired) { if (i >= max_epochs) break; out[i++] = e; }
  return ACT_OK;
}

// cursor: 0 = start, otherwise 1 + the number of keys already written (std::set order), DONE after the last
int act_nullifier_set_export_epochs(act_nullifier_set* s, uint64_t* cursor, size_t max_keys, int, uint8_t* out_keys, uint32_t* out_epochs, size_t* n_out) {
  *n_out = 0;
  if (*cursor == ACT_NULLIFIER_EXPORT_DONE) return ACT_OK;
  Side& sd = side(s);
  const size_t from = *cursor ? (size_t)*cursor - 1 : 0;
  if (from > s->keys.size()) { s->err = "mock: foreign cursor"; return ACT_ERR_ARG; }
  auto it = s->keys.begin();
  std::advance(it, from);
  size_t got = 0;
  for (; it != s->keys.end() && got < max_keys; ++it, ++got) {
    memcpy(out_keys + 32 * got, it->data(), 32);
    const auto e = sd.epoch.find(*it);
    out_epochs[got] = e == sd.epoch.end() ? 0 : e->second;
  }
  *n_out = got;
  *cursor = it == s->keys.end() ? ACT_NULLIFIER_EXPORT_DONE : from + got + 1;
  return ACT_OK;
}
}  // extern "C"
