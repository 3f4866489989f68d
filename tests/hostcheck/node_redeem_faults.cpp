// node_redeem_faults.cpp -- the failure contract of the node-level redeem calls as a stand-alone program for the host sanitizers:
// csrc/node.cpp, node_keyring.cpp and node_epochs.cpp over the TEST-ONLY mocks, no device.  3 devices, 40 records of which every third
// is rejected, and in turn a nullifier device that fails, a signing device that fails, a generator that fails; each through the
// one-key call, a ring of one and the same ring with an epoch.  The three forms must agree on every status byte, on which output slots
// are all zero, on the set's length and on whether the call failed.  Exit status 0 = they do.
//   g++ -std=c++17 -O1 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined -o node_redeem_faults
//       tests/hostcheck/node_redeem_faults.cpp anonymous-credit-tokens_amd/csrc/node.cpp anonymous-credit-tokens_amd/csrc/node_keyring.cpp
//       anonymous-credit-tokens_amd/csrc/node_epochs.cpp tests/node_mock_epochs/node_mock_epochs.cpp tests/node_mock/node_mock_keyring.cpp
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../include/act_mi355x.h"

extern "C" void act_mock_fail(int null_device, int sign_device);
extern "C" void act_mock_keyring_fail(int sign_device);

namespace {
constexpr size_t N = 40, PB = 64;      // (node_mock.cpp's proof record)
struct Got { std::vector<uint8_t> status, zero; size_t len; bool failed; };
bool operator==(const Got& a, const Got& b) { return a.status == b.status && a.zero == b.zero && a.len == b.len && a.failed == b.failed; }
int refuse(void*, uint8_t*, size_t) { return 1; }

Got run(act_node* nd, int form, int fault, const uint8_t* proofs, const uint8_t* rng) {
  const int devs[3] = {0, 1, 2};
  act_node_nullifier_set* ns = nullptr;
  if (act_node_nullifier_set_create(devs, 3, 1000, (const uint8_t*)"0123456789abcdef", &ns)) { std::puts("set_create failed"); std::exit(2); }
  act_mock_fail(fault == 0 ? 1 : -1, fault == 1 ? 1 : -1);
  act_mock_keyring_fail(fault == 1 ? 1 : -1);
  const act_rng_source bad{refuse, nullptr};
  const uint8_t* src = fault == 2 ? (const uint8_t*)&bad : rng;
  const int mode = fault == 2 ? ACT_RNG_CALLBACK : ACT_RNG_SEQUENTIAL;
  uint8_t sk[64] = {0}, key[64] = {0x40};
  const uint32_t epoch[1] = {5};
  std::vector<uint8_t> out(128 * N, 7), st(N, 99), ok(N, 99);
  int rc;
  if (form == 0) rc = act_node_redeem_batch(nd, ns, N, sk, proofs, src, mode, out.data(), st.data());
  else if (form == 1) rc = act_node_redeem_keyring_batch(nd, ns, N, key, 1, ACT_SIGN_MATCHED, proofs, src, mode, out.data(), st.data(), ok.data());
  else rc = act_node_redeem_keyring_epochs_batch(nd, ns, N, key, 1, epoch, ACT_SIGN_MATCHED, proofs, src, mode, out.data(), st.data(), ok.data());
  act_mock_fail(-1, -1);
  act_mock_keyring_fail(-1);
  Got g{st, std::vector<uint8_t>(N), act_node_nullifier_set_len(ns), rc != 0};
  const std::vector<uint8_t> none(128, 0);
  for (size_t i = 0; i < N; i++) g.zero[i] = memcmp(out.data() + 128 * i, none.data(), 128) == 0;
  act_node_nullifier_set_destroy(ns);
  return g;
}
}  // namespace

int main() {
  const int devs[3] = {0, 1, 2};
  const uint8_t h[96] = {0};
  act_node* nd = nullptr;
  if (act_node_create(h, 128, devs, 3, 0, &nd)) { std::puts("node_create failed"); return 2; }
  std::vector<uint8_t> proofs(PB * N), rng(128 * N + 1);
  for (size_t i = 0; i < proofs.size(); i++) proofs[i] = (uint8_t)(i * 131 + i / PB);
  for (size_t i = 0; i < N; i++) { proofs[PB * i] = (uint8_t)((proofs[PB * i] & 0xfe) | (i % 3 == 1)); memcpy(&proofs[PB * i + 1], &i, 7); }
  for (size_t i = 0; i < rng.size(); i++) rng[i] = (uint8_t)(i * 29 + 3);
  int bad = 0;
  for (int fault = 0; fault < 3; fault++) {
    const Got one = run(nd, 0, fault, proofs.data(), rng.data());
    size_t marked = 0;
    for (size_t i = 0; i < N; i++) {
      marked += one.status[i] == (fault == 0 ? ACT_STATUS_NULLIFIER_UNDETERMINED : ACT_STATUS_RECORDED_UNSIGNED);
      if ((one.status[i] != 0) != (one.zero[i] != 0) || (i % 3 == 1 && one.status[i] != 7)) { std::printf("fault %d lane %zu: status %d\n", fault, i, one.status[i]); bad = 1; }
    }
    if (!one.failed || !marked) { std::printf("fault %d: rc %d, %zu lanes marked\n", fault, (int)one.failed, marked); bad = 1; }
    for (int form = 1; form < 3; form++)
      if (!(run(nd, form, fault, proofs.data(), rng.data()) == one)) { std::printf("fault %d: form %d differs from the one-key call\n", fault, form); bad = 1; }
    std::printf("fault %d: %zu lanes marked, set length %zu\n", fault, marked, one.len);
  }
  act_node_destroy(nd);
  return bad;
}
