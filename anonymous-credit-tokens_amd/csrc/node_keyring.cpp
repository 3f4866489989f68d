// node_keyring.cpp -- key rotation over the GPUs of a node (include/act_mi355x.h act_node_*_keyring_batch).  A translation unit of its
// own, like node_nullifier.cpp and node_issue_wire.cpp: the CPU test builds link node.cpp against a mock engine that has only the
// single-GPU calls node.cpp itself uses.  The pieces are cut by node.cpp's dispatcher (act_node_dispatch::run_pieces: weights, tail,
// the handle's lock); out_key is cut per piece like status.
//
// Redemption: ring verification of every piece, then the body node.cpp's node_redeem ends in too (act_node_dispatch::redeem_tail,
// node_redeem.h): the NODE-level nullifier set over the whole batch in lane order (verdicts as skip mask; the set does not depend on
// the key), then the signatures, here with the per-lane key index -- check -> count -> sign, so that ACT_RNG_SEQUENTIAL /
// ACT_RNG_CALLBACK hand out one stream exactly as the sequential loop would.  The wire form reads the messages with act_cbor_decode_batch (its statuses are from_cbor's, the ones act_redeem_cbor_batch
// reports, in the codec's own numbering), block by block so that the host never holds more than a block of records, and frames with act_cbor_encode_batch.
#include <algorithm>
#include <cstring>
#include <functional>
#include <string>
#include <vector>
#include "../../include/act_mi355x.h"
#include "node_keyring.h"
#include "node_redeem.h"

namespace {
using namespace act_node_dispatch;      // run_pieces, Piece, at (node_redeem.h)
bool ring_ok(const uint8_t* keys, int nkeys) { return keys && nkeys >= 1 && nkeys <= ACT_KEYRING_MAX; }

// The sign half over the pieces.  rng is bytes.  A lane counts for the stream iff it is signed: status_in 0 AND key_index below nkeys.
// `pieces` (nullable): as run_pieces fills it.
int sign_pieces(act_node* nd, size_t n, const uint8_t* keys, int nkeys, const uint8_t* key_index, const uint8_t* kprime, const uint8_t* status_in,
                const uint8_t* rng, int rng_mode, uint8_t* out_refund, uint8_t* status, std::vector<Piece>* pieces) {
  const std::vector<uint8_t> checked(status_in, status_in + n), kidx(key_index, key_index + n);
  std::vector<size_t> before(n + 1, 0);
  for (size_t i = 0; i < n; i++) before[i + 1] = before[i] + (checked[i] == 0 && kidx[i] < nkeys);
  return run_pieces(nd, n, [&](act_ctx* ctx, size_t off, size_t m) {
    return act_refund_sign_keyring_batch(ctx, m, ACT_MEM_HOST, keys, nkeys, kidx.data() + off, at(kprime, off, 32), checked.data() + off,
                                         rng + (rng_mode == ACT_RNG_PER_LANE ? off : before[off]) * 128, rng_mode, at(out_refund, off, 128), status + off);
  }, pieces);
}

constexpr size_t WIRE_BLOCK = (size_t)1 << 16;      // messages decoded into host records at a time (1.1 GB at L = 128)
}  // namespace

// null_step (nullable): the nullifier step when it is not the plain check-and-insert (node_epochs.cpp records the matched key's epoch:
// it is handed out_key beside the verdicts).  A parameter and not a call, so that this file needs nothing of the engine's epoch calls.
int act_node_keyring::redeem(act_node* nd, act_node_nullifier_set* set, size_t n, const uint8_t* keys, int nkeys, int sign_key, const uint8_t* proof,
                             const uint8_t* cbor, const uint64_t* offsets, const uint8_t* rng, int rng_mode, uint8_t* out, uint8_t* status, uint8_t* out_key,
                             const NullStep* null_step) {
  const bool wire = cbor != nullptr;
  if (!nd || !set || !rng || !ring_ok(keys, nkeys) || (n && ((!proof && !cbor) || !out || !status || !out_key))) return ACT_ERR_ARG;
  if (sign_key != ACT_SIGN_MATCHED && (sign_key < 0 || sign_key >= nkeys)) return ACT_ERR_ARG;
  if (rng_mode != ACT_RNG_PER_LANE && rng_mode != ACT_RNG_SEQUENTIAL && rng_mode != ACT_RNG_CALLBACK) return ACT_ERR_ARG;
  act_ctx* c0 = act_node_ctx(nd, 0);
  if (n == 0) return act_verify_spend_keyring_batch(c0, 0, ACT_MEM_HOST, keys, nkeys, nullptr, nullptr, nullptr, nullptr);      // a bad ring fails the call whatever n
  const size_t pb = act_spend_proof_bytes(c0), out_rec = wire ? act_cbor_size(c0, ACT_CBOR_REFUND) : 128;
  std::vector<uint8_t> kprime(n * 32), verdict(n), nul(wire ? n * 32 : 0);
  int rc;
  if (!wire) {
    rc = run_pieces(nd, n, [&](act_ctx* ctx, size_t off, size_t m) {
      return act_verify_spend_keyring_batch(ctx, m, ACT_MEM_HOST, keys, nkeys, at(proof, off, pb), verdict.data() + off, out_key + off, kprime.data() + off * 32);
    });
    if (rc) return rc;
  } else {
    const size_t ml = act_cbor_size(c0, ACT_CBOR_SPEND_PROOF);
    std::vector<uint8_t> recs(std::min(n, WIRE_BLOCK) * pb), wst(std::min(n, WIRE_BLOCK));
    for (size_t b0 = 0; b0 < n; b0 += WIRE_BLOCK) {
      const size_t bn = std::min(WIRE_BLOCK, n - b0);
      rc = run_pieces(nd, bn, [&](act_ctx* ctx, size_t off, size_t m) {      // offsets are absolute into `cbor`: every piece gets the same base
        return act_cbor_decode_batch(ctx, ACT_CBOR_SPEND_PROOF, m, ACT_MEM_HOST, offsets ? cbor : cbor + (b0 + off) * ml, offsets ? offsets + b0 + off : nullptr,
                                     recs.data() + off * pb, wst.data() + off);
      });
      if (rc) return rc;
      for (size_t i = 0; i < bn; i++) if (wst[i]) memset(recs.data() + i * pb, 0, pb);
      rc = run_pieces(nd, bn, [&](act_ctx* ctx, size_t off, size_t m) {
        return act_verify_spend_keyring_batch(ctx, m, ACT_MEM_HOST, keys, nkeys, recs.data() + off * pb, verdict.data() + b0 + off, out_key + b0 + off,
                                              kprime.data() + (b0 + off) * 32);
      });
      if (rc) return rc;
      for (size_t i = 0; i < bn; i++) {
        if (wst[i]) {      // from_cbor's error comes first: the codec's 1 / 2 / 3 (Ciborium, InvalidStructure, InvalidValue) as the wire calls' lane statuses
          verdict[b0 + i] = wst[i] == 1 ? ACT_STATUS_CBOR_MALFORMED : wst[i] == 2 ? ACT_STATUS_CBOR_STRUCTURE : ACT_STATUS_UNDECODABLE;
          out_key[b0 + i] = ACT_KEY_NONE; memset(kprime.data() + (b0 + i) * 32, 0, 32);
        }
        else memcpy(nul.data() + (b0 + i) * 32, recs.data() + i * pb, 32);                                                                // `k` is the record's first field
      }
    }
  }
  const uint8_t* nullifiers = wire ? nul.data() : proof;
  const size_t stride = wire ? 32 : pb;
  return act_node_dispatch::redeem_tail(nd, set, n, out_rec, verdict.data(), rng, rng_mode, out, status,
    [&](const uint8_t* mask, uint8_t* spent) {
      return null_step ? (*null_step)(set, n, nullifiers, stride, mask, out_key, spent) : act_node_nullifier_check_and_insert_batch(set, n, nullifiers, stride, mask, spent);
    },
    [&](const uint8_t* checked, const uint8_t* r, int r_mode, std::vector<Piece>* pieces) {
      std::vector<uint8_t> kidx(n), rec(wire ? n * 128 : 0);
      for (size_t i = 0; i < n; i++) kidx[i] = sign_key >= 0 ? (uint8_t)sign_key : out_key[i];
      int rc_sign = sign_pieces(nd, n, keys, nkeys, kidx.data(), kprime.data(), checked, r, r_mode, wire ? rec.data() : out, status, pieces);
      if (rc_sign || !wire) return rc_sign;
      rc_sign = run_pieces(nd, n, [&](act_ctx* ctx, size_t off, size_t m) {
        return act_cbor_encode_batch(ctx, ACT_CBOR_REFUND, m, ACT_MEM_HOST, rec.data() + off * 128, out + off * out_rec);
      });
      if (rc_sign) pieces->push_back({(size_t)-1, 0, n, rc_sign});      // no lane has its message: every signature is owed
      else for (size_t i = 0; i < n; i++) if (status[i]) memset(out + i * out_rec, 0, out_rec);      // an unsigned lane's slot is all zero
      return rc_sign;
    });
}
using act_node_keyring::redeem;

extern "C" {

int act_node_verify_spend_keyring_batch(act_node* nd, size_t n, const uint8_t* keys, int nkeys, const uint8_t* proof, uint8_t* status, uint8_t* out_key,
                                        uint8_t* out_kprime) {
  if (!nd || !ring_ok(keys, nkeys) || (n && (!proof || !status || !out_key))) return ACT_ERR_ARG;
  act_ctx* c0 = act_node_ctx(nd, 0);
  if (n == 0) return act_verify_spend_keyring_batch(c0, 0, ACT_MEM_HOST, keys, nkeys, nullptr, nullptr, nullptr, nullptr);
  const size_t pb = act_spend_proof_bytes(c0);
  return run_pieces(nd, n, [&](act_ctx* ctx, size_t off, size_t m) {
    return act_verify_spend_keyring_batch(ctx, m, ACT_MEM_HOST, keys, nkeys, at(proof, off, pb), status + off, out_key + off, at(out_kprime, off, 32));
  });
}

int act_node_refund_sign_keyring_batch(act_node* nd, size_t n, const uint8_t* keys, int nkeys, const uint8_t* key_index, const uint8_t* kprime,
                                       const uint8_t* status_in, const uint8_t* rng, int rng_mode, uint8_t* out_refund, uint8_t* status) {
  if (!nd || !ring_ok(keys, nkeys) || (n && (!key_index || !kprime || !status_in || !rng || !out_refund || !status))) return ACT_ERR_ARG;
  if (rng_mode != ACT_RNG_PER_LANE && rng_mode != ACT_RNG_SEQUENTIAL) return ACT_ERR_ARG;
  if (n == 0) return act_refund_sign_keyring_batch(act_node_ctx(nd, 0), 0, ACT_MEM_HOST, keys, nkeys, nullptr, nullptr, nullptr, nullptr, rng_mode, nullptr, nullptr);
  return sign_pieces(nd, n, keys, nkeys, key_index, kprime, status_in, rng, rng_mode, out_refund, status, nullptr);
}

int act_node_redeem_keyring_batch(act_node* nd, act_node_nullifier_set* set, size_t n, const uint8_t* keys, int nkeys, int sign_key, const uint8_t* proof,
                                  const uint8_t* rng, int rng_mode, uint8_t* out_refund, uint8_t* status, uint8_t* out_key) {
  if (n && !proof) return ACT_ERR_ARG;
  return redeem(nd, set, n, keys, nkeys, sign_key, proof, nullptr, nullptr, rng, rng_mode, out_refund, status, out_key, nullptr);
}
int act_node_redeem_cbor_keyring_batch(act_node* nd, act_node_nullifier_set* set, size_t n, const uint8_t* keys, int nkeys, int sign_key, const uint8_t* cbor,
                                       const uint64_t* offsets, const uint8_t* rng, int rng_mode, uint8_t* out_refund_cbor, uint8_t* status, uint8_t* out_key) {
  if (n && !cbor) return ACT_ERR_ARG;
  static const uint8_t none = 0;
  return redeem(nd, set, n, keys, nkeys, sign_key, nullptr, cbor ? cbor : &none, offsets, rng, rng_mode, out_refund_cbor, status, out_key, nullptr);
}

}  // extern "C"
