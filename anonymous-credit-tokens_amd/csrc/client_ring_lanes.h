// client_ring_lanes.h — the client's side of key rotation: the per-lane bodies of k_client_ring.hip, as functions that also compile
// under g++ (tests/hostcheck/client_ring_check.cpp runs, counts and sanitizes them; the keyring_lanes.h pattern).
//
// Neither an IssuanceResponse nor a Refund names the key it was signed with, and in both client verifiers (k_client.hip) the issuer's
// public key w enters in TWO places only:  X_g = e g + w  and  Y_g = (z - gamma e) g - gamma w.  A, X_A, Y_A, the Com_j decodings,
// the Horner sum and the chains on A and X_A are the same under every key.  A ring call therefore runs phase A ONCE, under ring key
// 0 -- k_client_a / k_client_a_wide, unchanged -- and per additional key k an item costs
//   client_ring_cand_lane    lane = (k, item)   X_g,k and Y_g,k computed DIRECTLY from e, gamma, z and tables, both encoded into a
//                                               side buffer: two fixed-base products on g, one on w_k's own table, one mixed addition
//   client_ring_hash_lane    lane = (k, item)   the challenge hash of the item's transcript with the X_g and Y_g payloads replaced
//                                               (one BLAKE3 chunk: the transcripts are under 512 bytes)
//   client_ring_finish_lane  lane = item        nkeys challenges against gamma, the smallest index wins -> status, out_key, token
// (RefundReturn records, ClientArgs::with_t: the same two per-key lanes at the 160-byte stride and the finish of client_ring_return_lanes.h)
// Direct, not as a difference to key 0: X_g,0 and Y_g,0 exist only as encodings in the transcript, and decoding the two costs more
// (two square roots, ~530 field operations) than the two products on g that the direct form adds (32 mixed additions, 224).  It
// also makes the candidates independent of phase A.  gamma and w are public, so gamma w_k is an ADDRESSED fixed-base product like
// every product of the one-key verifier.  w_k's table is 8 bits wide: 32 mixed additions per product, 1 MiB per key (L2 resident),
// built in one short launch whenever the ring changes; at 12 bits it would save 10 of the candidate's 65 additions for 11 MiB.
// Counted cost per extra key (tests/test_client_ring_host.py, restated for the product's 16-bit table of g): 65 mixed additions and
// two encodings, 1 023 field multiplications + squarings -- 0.40 of ONE chain_b<1> product (2 538), the least a variable-base form
// would pay; 10.6 % of the one-key issuance body (9 666) and 2.2 % of the one-key refund body at L = 128 (47 289).
#pragma once
#include "kernels.h"
#include "keyring.h"      // KEYRING_MAX, KEY_NONE

namespace act {

constexpr uint32_t CLIENT_RING_WBITS = 8;       // window width of a ring key's table
constexpr uint32_t CLIENT_RING_TAB_ID = 1;      // FbTab::id of those tables (host-side operation counting only: not g's slot)

struct ClientRingArgs {
  ClientArgs c;              // the chunk's one-key arguments (c.w = ring key 0; c.xof = the XOF words of the transcripts as phase A left them)
  const uint32_t* tabw;      // nkeys - 1 fixed-base tables of CLIENT_RING_WBITS bits, back to back: w_1, w_2, ... (public)
  uint32_t nkeys;
  uint8_t* cand;             // n * (nkeys - 1) * 64: enc(X_g,k) | enc(Y_g,k), k = 1 .. nkeys - 1
  uint32_t* xofs;            // n * (nkeys - 1) * 16: XOF words of the transcript under key k >= 1
  uint8_t* out_key;          // n
};

ACT_HD FbTab client_ring_table(const ClientRingArgs& r, uint32_t k) {
  return FbTab{r.tabw + (size_t)(k - 1u) * fb_table_words(CLIENT_RING_WBITS), CLIENT_RING_WBITS, CLIENT_RING_TAB_ID};
}
// byte offset of the X_g payload inside a "respond" / "refund" transcript: prefix | [c] | e | A | X_A | X_g | Y_A | Y_g, 40 bytes per
// element, 8 bytes of length in front of every payload (k_client.hip).  Y_g's payload lies 80 bytes further and ends the message.
ACT_HD uint32_t client_ring_xg_offset(const DevParams& P, int label) {
  return P.prefix_len[label] + (label == LABEL_RESPOND ? 40u : 0u) + 40u * 3u + 8u;
}
ACT_HD uint32_t client_ring_tr_len(const DevParams& P, int label) { return P.prefix_len[label] + 40u * (label == LABEL_RESPOND ? 7u : 6u); }
// bytes per answer record: IssuanceResponse 160, Refund 128, RefundReturn (with_t: A | e | gamma | z | t) 160.  The one place the ring
// lanes take their stride from; e, gamma and z lie at 32, 64 and 96 in all three.
ACT_HD uint32_t client_ring_resp_stride(int label, int with_t) { return (label == LABEL_RESPOND || with_t) ? 160u : 128u; }

// X_g,k = e g + w_k and Y_g,k = (z - gamma e) g - gamma w_k (src/lib.rs:537, :541 / :1232, :1234), encoded.  w_k itself is entry 1 of
// window 0 of its table.  An item whose A or Com_j does not decode is rejected by its flags whatever lands here.
ACT_HD void client_ring_cand_lane(const ClientRingArgs& r, uint32_t gid) {
  const uint32_t extra = r.nkeys - 1u;
  if (gid >= r.c.n * extra) return;
  const uint32_t p = gid % r.c.n, k = gid / r.c.n + 1u;      // key-major: the lanes of a wavefront walk ONE ring table
  const ClientArgs& a = r.c;
  const uint8_t* resp = a.resp + (size_t)p * client_ring_resp_stride(a.label, a.with_t);
  const sc e = load_sc(resp + 32), gamma = load_sc(resp + 64), z = load_sc(resp + 96);
  const FbTab tw = client_ring_table(r, k);
  const ge xg = ge_madd(fixed_base_acc(ge_identity(), a.P.tab[BASE_G], e), niels_load(tw.p + NIELS_WORDS));
  const ge yg = fixed_base_acc(fixed_base_acc(ge_identity(), a.P.tab[BASE_G], sc_sub(z, sc_mul(gamma, e))), tw, sc_neg(gamma));
  uint8_t* out = r.cand + ((size_t)p * extra + (k - 1u)) * 64;
  uint32_t enc[8];
  ristretto_encode(enc, xg); store8(out, enc);
  ristretto_encode(enc, yg); store8(out + 32, enc);
}

// ---- one BLAKE3 chunk with 32-byte payloads replaced at ANY byte offset (the prefixes are 185 / 186 bytes long) ---------------------
// The payload as the (up to nine) message words it touches: word `word + j` becomes (old & ~m[j]) | v[j].  Static indices only.
struct b3_patch { uint32_t word; uint32_t v[9], m[9]; };
ACT_HD b3_patch b3_patch_make(uint32_t byte_off, const uint32_t rep[8]) {
  b3_patch q;
  q.word = byte_off >> 2;
  const uint32_t sh = 8u * (byte_off & 3u);
  for (int j = 0; j < 9; j++) {
    const uint32_t lo = j < 8 ? rep[j] : 0u, hi = j > 0 ? rep[j - 1] : 0u;
    q.v[j] = sh ? ((lo << sh) | (hi >> (32u - sh))) : lo;
    q.m[j] = j == 0 ? (0xffffffffu << sh) : j == 8 ? (sh ? ~(0xffffffffu << sh) : 0u) : 0xffffffffu;
  }
  return q;
}
ACT_HD void b3_patch_apply(uint32_t m[16], uint32_t block_word, const b3_patch& q) {
  if (block_word + 16u <= q.word || q.word + 9u <= block_word) return;
  for (int i = 0; i < 16; i++) {
    const uint32_t d = block_word + (uint32_t)i - q.word;
    for (int j = 0; j < 9; j++) if (d == (uint32_t)j) m[i] = (m[i] & ~q.m[j]) | (q.v[j] & q.m[j]);
  }
}
// b3_hash_xof64 (blake3_hd.h) of a message of at most one chunk (len <= 1024) with the two patches applied: the same block walk --
// every block but the last compressed into the chaining value, the last one as the root -- with the replaced words put in on the way
ACT_HD void b3_chunk_xof64_patched2(uint32_t out[16], const uint32_t* msg, uint32_t len, const b3_patch& qa, const b3_patch& qb) {
  const uint32_t nblocks = len ? (len + 63u) >> 6 : 1u;
  uint32_t cv[8], m[16], o[16];
  for (int i = 0; i < 8; i++) cv[i] = b3_iv(i);
  uint32_t blen = 0, fl = 0;
  for (uint32_t b = 0; b < nblocks; b++) {
    blen = b3_load_block(m, msg, len, b * 64u);
    b3_patch_apply(m, b * 16u, qa);
    b3_patch_apply(m, b * 16u, qb);
    fl = (b == 0 ? B3_CHUNK_START : 0u) | (b == nblocks - 1 ? B3_CHUNK_END : 0u);
    if (b + 1 < nblocks) { b3_compress(o, cv, m, 0u, 0u, 64u, fl); for (int i = 0; i < 8; i++) cv[i] = o[i]; }
  }
  b3_compress(out, cv, m, 0u, 0u, blen, fl | B3_ROOT);
}

// the challenge of item p under ring key k >= 1: phase A's transcript with the candidate's two encodings in the X_g and Y_g slots
// (in the kernel in BOTH transcript modes, as the fused tiny calls hash: one chunk, the same bytes either way)
ACT_HD void client_ring_hash_lane(const ClientRingArgs& r, uint32_t gid) {
  const uint32_t extra = r.nkeys - 1u;
  if (gid >= r.c.n * extra) return;
  const uint32_t p = gid % r.c.n, k = gid / r.c.n + 1u;
  const ClientArgs& a = r.c;
  const uint8_t* cand = r.cand + ((size_t)p * extra + (k - 1u)) * 64;
  uint32_t rx[8], ry[8], o[16];
  load8(rx, cand); load8(ry, cand + 32);
  const uint32_t off = client_ring_xg_offset(a.P, a.label);
  b3_chunk_xof64_patched2(o, reinterpret_cast<const uint32_t*>(a.trs + (size_t)p * SMALL_TR_STRIDE), client_ring_tr_len(a.P, a.label),
                          b3_patch_make(off, rx), b3_patch_make(off + 80u, ry));
  uint32_t* q = r.xofs + ((size_t)p * extra + (k - 1u)) * 16;
  for (int i = 0; i < 16; i++) q[i] = o[i];
}

// the smallest ring index whose challenge for item p equals gamma (counting down, so that the smallest index is kept), or KEY_NONE
ACT_HD uint32_t client_ring_match(const ClientRingArgs& r, uint32_t p, const sc& gamma) {
  const uint32_t extra = r.nkeys - 1u;
  uint32_t match = KEY_NONE;
  for (uint32_t k = r.nkeys; k-- > 0;) {
    const uint32_t* q = k ? r.xofs + ((size_t)p * extra + (k - 1u)) * 16 : r.c.xof + (size_t)p * 16;
    uint32_t w[16];
    for (int i = 0; i < 16; i++) w[i] = q[i];
    if (sc_equal(sc_from_wide_words(w), gamma)) match = k;
  }
  return match;
}

// k_client_b over a ring: the smallest k whose challenge equals gamma.  The token (:554-560 / :1246-1252) does not depend on the key.
ACT_HD void client_ring_finish_lane(const ClientRingArgs& r, uint32_t p) {
  const ClientArgs& a = r.c;
  const bool issuance = a.label == LABEL_RESPOND;
  const uint8_t* resp = a.resp + (size_t)p * client_ring_resp_stride(a.label, a.with_t);
  const sc gamma = load_sc(resp + 64);
  const uint32_t match = client_ring_match(r, p, gamma);
  uint8_t stt = 0;
  if (a.flags[p] & FLAG_UNDECODABLE) stt = 255;
  else if (match == KEY_NONE) stt = issuance ? 2 : 4;       // InvalidIssuanceResponseProof / InvalidRefundProof under every ring key
  a.status[p] = stt;
  r.out_key[p] = stt == 0 ? (uint8_t)match : KEY_NONE;
  uint8_t* out = a.out_token + (size_t)p * 160;
  if (stt) { for (int i = 0; i < 160; i += 32) zero8(out + i); return; }
  const uint8_t* pre = a.pre + (size_t)p * (issuance ? 64 : 96);      // pre record is r | k (| m)
  uint32_t t[8];
  load8(t, resp); store8(out, t);
  store_sc(out + 32, load_sc(resp + 32));
  store_sc(out + 64, load_sc(pre + 32));
  store_sc(out + 96, load_sc(pre));
  store_sc(out + 128, issuance ? load_sc(resp + 128) : load_sc(pre + 64));
}

#if defined(__HIPCC__)
void launch_client_ring_cand(const ClientRingArgs& r, hipStream_t s);
void launch_client_ring_hash(const ClientRingArgs& r, hipStream_t s);
void launch_client_ring_finish(const ClientRingArgs& r, hipStream_t s);
#endif

}  // namespace act
