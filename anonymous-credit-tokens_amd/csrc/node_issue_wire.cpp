// node_issue_wire.cpp -- issuance on wire bytes over the GPUs of a node (include/act_mi355x.h act_node_issue_*cbor_batch).  A translation
// unit of its own, like node_nullifier.cpp: the CPU test builds link node.cpp against a mock engine that has only the single-GPU calls
// node.cpp itself uses.  The pieces are cut by node.cpp's dispatcher (act_node_dispatch::run_pieces: weights, tail, the handle's lock).
#include <cstring>
#include <functional>
#include <vector>
#include "../../include/act_mi355x.h"
#include "node_redeem.h"      // run_pieces, at, count_zero
#include "rng_source.h"

namespace {
using namespace act_node_dispatch;
// accepted lanes in front of every lane (ACT_RNG_SEQUENTIAL across pieces: a piece signs from its own offset into the stream)
std::vector<size_t> accepted_before(const uint8_t* st, size_t n) {
  std::vector<size_t> a(n + 1, 0);
  for (size_t i = 0; i < n; i++) a[i + 1] = a[i] + (st[i] == 0);
  return a;
}
// the sign half over the pieces; rng is bytes (ACT_RNG_CALLBACK already drawn once for the accepted lanes of all pieces)
int issue_sign_cbor_pieces(act_node* nd, size_t n, const uint8_t sk[64], const uint8_t* req, const uint8_t* c, const uint8_t* status_in,
                           const uint8_t* rng, int rng_mode, uint8_t* out_resp_cbor, uint8_t* status) {
  const std::vector<uint8_t> checked(status_in, status_in + n);
  const std::vector<size_t> before = accepted_before(checked.data(), n);
  const size_t rl = act_cbor_size(act_node_ctx(nd, 0), ACT_CBOR_ISSUANCE_RESPONSE);
  return run_pieces(nd, n, [&](act_ctx* ctx, size_t off, size_t m) {
    return act_issue_sign_cbor_batch(ctx, m, ACT_MEM_HOST, sk, at(req, off, 128), at(c, off, 32), checked.data() + off,
                                     rng + (rng_mode == ACT_RNG_PER_LANE ? off : before[off]) * 128, rng_mode, at(out_resp_cbor, off, rl), status + off);
  });
}
}  // namespace

extern "C" {

// a piece takes messages [off, off + m) (offsets absolute into `cbor`, as for the spend messages)
int act_node_issue_check_cbor_batch(act_node* nd, size_t n, const uint8_t* cbor, const uint64_t* offsets, uint8_t* status, uint8_t* out_req) {
  if (!nd || (n && (!cbor || !status))) return ACT_ERR_ARG;
  const size_t ml = act_cbor_size(act_node_ctx(nd, 0), ACT_CBOR_ISSUANCE_REQUEST);
  return run_pieces(nd, n, [&](act_ctx* ctx, size_t off, size_t m) {
    return act_issue_check_cbor_batch(ctx, m, ACT_MEM_HOST, offsets ? cbor : cbor + off * ml, offsets ? offsets + off : nullptr, status + off,
                                      at(out_req, off, 128));
  });
}
int act_node_issue_sign_cbor_batch(act_node* nd, size_t n, const uint8_t sk[64], const uint8_t* req, const uint8_t* c, const uint8_t* status_in,
                                   const uint8_t* rng, int rng_mode, uint8_t* out_resp_cbor, uint8_t* status) {
  if (!nd || !sk || !rng || (n && (!req || !c || !status_in || !out_resp_cbor || !status))) return ACT_ERR_ARG;
  if (rng_mode != ACT_RNG_PER_LANE && rng_mode != ACT_RNG_SEQUENTIAL && rng_mode != ACT_RNG_CALLBACK) return ACT_ERR_ARG;
  act::DrawnRng drawn;
  const int rc = drawn.resolve(rng, rng_mode, rng_mode == ACT_RNG_CALLBACK ? count_zero(status_in, n) : 0);
  if (rc) { if (n) memset(out_resp_cbor, 0, n * act_cbor_size(act_node_ctx(nd, 0), ACT_CBOR_ISSUANCE_RESPONSE)); return rc; }
  return issue_sign_cbor_pieces(nd, n, sk, req, c, status_in, rng, rng_mode, out_resp_cbor, status);
}
// The whole endpoint.  ACT_RNG_PER_LANE (or one GPU): every piece runs the whole call.  SEQUENTIAL / CALLBACK: every piece is checked
// first, the accepted lanes in front of each piece are counted, the generator drawn once, then every piece signs and frames
// (act_node_issue_batch's two phases).
int act_node_issue_cbor_batch(act_node* nd, size_t n, const uint8_t sk[64], const uint8_t* cbor, const uint64_t* offsets, const uint8_t* c,
                              const uint8_t* rng, int rng_mode, uint8_t* out_resp_cbor, uint8_t* status) {
  if (!nd || !sk || !rng || (n && (!cbor || !c || !out_resp_cbor || !status))) return ACT_ERR_ARG;
  if (rng_mode != ACT_RNG_PER_LANE && rng_mode != ACT_RNG_SEQUENTIAL && rng_mode != ACT_RNG_CALLBACK) return ACT_ERR_ARG;
  if (n == 0) return ACT_OK;
  act_ctx* c0 = act_node_ctx(nd, 0);
  const size_t ml = act_cbor_size(c0, ACT_CBOR_ISSUANCE_REQUEST), rl = act_cbor_size(c0, ACT_CBOR_ISSUANCE_RESPONSE);
  if (rng_mode == ACT_RNG_PER_LANE || act_node_device_count(nd) == 1)
    return run_pieces(nd, n, [&](act_ctx* ctx, size_t off, size_t m) {
      return act_issue_cbor_batch(ctx, m, ACT_MEM_HOST, sk, offsets ? cbor : cbor + off * ml, offsets ? offsets + off : nullptr, at(c, off, 32),
                                  rng_mode == ACT_RNG_PER_LANE ? at(rng, off, 128) : rng, rng_mode, at(out_resp_cbor, off, rl), status + off);
    });
  std::vector<uint8_t> req(n * 128), verdict(n);
  int rc = act_node_issue_check_cbor_batch(nd, n, cbor, offsets, verdict.data(), req.data());
  if (rc) return rc;
  act::DrawnRng drawn;
  if ((rc = drawn.resolve(rng, rng_mode, rng_mode == ACT_RNG_CALLBACK ? count_zero(verdict.data(), n) : 0))) {
    memcpy(status, verdict.data(), n); memset(out_resp_cbor, 0, n * rl);      // the verdicts stand; nothing was signed
    return rc;
  }
  return issue_sign_cbor_pieces(nd, n, sk, req.data(), c, verdict.data(), rng, rng_mode, out_resp_cbor, status);
}

}  // extern "C"
