// node_mock_keyring.cpp — TEST-ONLY stand-ins for the single-GPU key-ring entry points that csrc/node_keyring.cpp calls (and the two
// codec calls its wire form uses), beside node_mock.cpp: tests/test_keyring_node_cpu.py links node.cpp + node_keyring.cpp + both mocks.
//
// Mock semantics (node_mock.cpp's, extended): a lane is ACCEPTED iff the first byte of its record is even (status 7 otherwise); an
// accepted lane MATCHES ring key (record byte 8) % nkeys; its K' carries the record's 8-byte tag; a signed lane's refund = tag | the
// first bytes of the rng slice it was handed, with byte 127 = the key index it was signed with and byte 126 = first byte of that ring
// key.  A wire message = 3 framing bytes + the record; framing byte 0 == 0xff makes it malformed (the codec's status 1, a wire call's 254).
#include <atomic>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/act_mi355x.h"

struct act_ctx { int device; int L; std::atomic<size_t> lanes{0}; std::string err; std::atomic<unsigned> ns_per_lane{0}; };     // node_mock.cpp's
static const size_t kPB = 64;
static int g_fail_ring_sign_device = -1;

extern "C" {
void act_mock_keyring_fail(int sign_device) { g_fail_ring_sign_device = sign_device; }

int act_verify_spend_keyring_batch(act_ctx* c, size_t n, int, const uint8_t* keys, int nkeys, const uint8_t* proof, uint8_t* status, uint8_t* out_key, uint8_t* kp) {
  if (!keys || nkeys < 1 || nkeys > ACT_KEYRING_MAX) return ACT_ERR_ARG;
  c->lanes += n;
  for (size_t i = 0; i < n; i++) {
    const uint8_t* r = proof + kPB * i;
    status[i] = (r[0] & 1) ? 7 : 0;
    out_key[i] = status[i] ? ACT_KEY_NONE : (uint8_t)(r[8] % nkeys);
    if (kp) { memset(kp + 32 * i, 0, 32); if (!status[i]) memcpy(kp + 32 * i, r, 8); }
  }
  return ACT_OK;
}
int act_refund_sign_keyring_batch(act_ctx* c, size_t n, int, const uint8_t* keys, int nkeys, const uint8_t* key_index, const uint8_t* kprime,
                                  const uint8_t* status_in, const uint8_t* rng, int mode, uint8_t* out, uint8_t* status) {
  if (!keys || nkeys < 1 || nkeys > ACT_KEYRING_MAX) return ACT_ERR_ARG;
  if (c->device == g_fail_ring_sign_device) { c->err = "mock: ring signature step failed"; return ACT_ERR_HIP; }
  c->lanes += n; size_t cur = 0;
  for (size_t i = 0; i < n; i++) {
    uint8_t st = status_in[i];
    if (st == 0 && key_index[i] >= nkeys) st = 255;
    status[i] = st;
    memset(out + 128 * i, 0, 128);
    if (st) continue;
    const uint8_t* slice = rng + 128 * (mode == ACT_RNG_PER_LANE ? i : cur++);
    memcpy(out + 128 * i, kprime + 32 * i, 8); memcpy(out + 128 * i + 8, slice, 100);
    out[128 * i + 127] = key_index[i]; out[128 * i + 126] = keys[64 * key_index[i]];
  }
  return ACT_OK;
}
size_t act_cbor_record_bytes(const act_ctx*, int) { return kPB; }
int act_cbor_decode_batch(act_ctx* c, int, size_t n, int, const uint8_t* cbor, const uint64_t* offsets, uint8_t* out_records, uint8_t* status) {
  c->lanes += n;
  for (size_t i = 0; i < n; i++) {
    const uint8_t* m = cbor + (offsets ? offsets[i] : i * (kPB + 3));
    status[i] = m[0] == 0xff ? 1 : 0;                      // the codec's numbering: 1 = CborError::Ciborium
    if (status[i]) memset(out_records + kPB * i, 0, kPB); else memcpy(out_records + kPB * i, m + 3, kPB);
  }
  return ACT_OK;
}
int act_cbor_encode_batch(act_ctx* c, int, size_t n, int, const uint8_t* records, uint8_t* out) {
  c->lanes += n;
  for (size_t i = 0; i < n; i++) { out[129 * i] = 0xa4; memcpy(out + 129 * i + 1, records + 128 * i, 128); }
  return ACT_OK;
}
}  // extern "C"
