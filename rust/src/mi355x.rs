//! src/mi355x.rs — MI355X batch engine behind the crate's own API (feature `mi355x`).
//!
//! UNCOMPILED in the authoring environment (no Rust toolchain there; rust/README.md).  Binds `libact_mi355x.so`
//! (C ABI: include/act_mi355x.h).  Every `*_batch` method equals the loop
//! `items.iter().map(|x| x.method(params, .., &mut rng))` byte for byte, including the state `rng` is left in:
//! lane i of a batch is one call of the method, raw records are the structs' fields in CBOR key order
//! (src/cbor.rs:105-110, 163-169, 250-268, 422-427, 546-549, 596-602, 656-660), every `Scalar::random` is one 64-byte
//! `fill_bytes`, and issue / refund draw only for accepted lanes (src/lib.rs:638-643, 842-846).
//!
//! The existing single-call signatures are kept (bottom of this file): with the feature on they are batches of one.
use crate::{
    CreditToken, Error, IssuanceRequest, IssuanceResponse, Params, PreIssuance, PreRefund, PrivateKey, PublicKey, Refund,
    SpendProof, L,
};
use curve25519_dalek::{ristretto::CompressedRistretto, RistrettoPoint, Scalar};
use rand_core::CryptoRngCore;
use std::ffi::CStr;
use std::os::raw::{c_char, c_int, c_void};
use std::sync::OnceLock;

#[repr(C)]
pub struct ActNode {
    _private: [u8; 0],
}
#[repr(C)]
pub struct ActNodeNullifierSet {
    _private: [u8; 0],
}
/// One-GPU handles (`act_ctx`, `act_nullifier_set`): what the admission calls take.
#[repr(C)]
pub struct ActCtx {
    _private: [u8; 0],
}
#[repr(C)]
pub struct ActNullifierSet {
    _private: [u8; 0],
}
/// `act_rng_source` (include/act_mi355x.h): the caller's generator handed to the library, which draws 128 bytes per lane it signs --
/// once, after every verdict is known -- so the generator ends where a sequential loop over `refund` would have left it.
#[repr(C)]
pub struct ActRngSource {
    draw: unsafe extern "C" fn(rng_ctx: *mut c_void, dst: *mut u8, len: usize) -> c_int,
    rng_ctx: *mut c_void,
}
const ACT_RNG_SEQUENTIAL: c_int = 1;
const ACT_RNG_CALLBACK: c_int = 2;
const REFUND_CBOR_BYTES: usize = 141; // act_cbor_size(ctx, ACT_CBOR_REFUND): A4, then four times (key, 58 20, 32 bytes)
const ISSUANCE_RESPONSE_CBOR_BYTES: usize = 176; // act_cbor_size(ctx, ACT_CBOR_ISSUANCE_RESPONSE): A5, then five times (key, 58 20, 32 bytes)
const PROOF_FIELDS: usize = 14 + 4 * L;
const PROOF_BYTES: usize = 32 * PROOF_FIELDS; // 16 832
const PROVE_RNG_BYTES: usize = 64 * (4 * L + 12); // 33 536: draw order of src/lib.rs:978-1058

// one declaration per entry point used, prototypes as in include/act_mi355x.h
extern "C" {
    fn act_node_create(h: *const u8, l: c_int, devices: *const c_int, n_devices: c_int, max_batch: usize, out: *mut *mut ActNode) -> c_int;
    fn act_node_destroy(node: *mut ActNode);
    // where messages that are not the canonical encoding are read (1 = on the GPU, the default; 0 = the host reader): declared for
    // deployments that want the fallback, called nowhere in this binding
    fn act_node_set_wire_reader(node: *mut ActNode, reader: c_int) -> c_int;
    fn act_node_last_error(node: *const ActNode) -> *const c_char;
    fn act_node_request_batch(node: *mut ActNode, n: usize, pre: *const u8, rng: *const u8, out_req: *mut u8) -> c_int;
    fn act_node_issue_check_batch(node: *mut ActNode, n: usize, req: *const u8, status: *mut u8) -> c_int;
    fn act_node_issue_sign_batch(node: *mut ActNode, n: usize, sk: *const u8, req: *const u8, c: *const u8, status_in: *const u8,
                                 rng: *const u8, rng_mode: c_int, out_resp: *mut u8, status: *mut u8) -> c_int;
    fn act_node_issuance_to_credit_token_batch(node: *mut ActNode, n: usize, pre: *const u8, w: *const u8, req: *const u8,
                                               resp: *const u8, out_token: *mut u8, status: *mut u8) -> c_int;
    fn act_node_prove_spend_batch(node: *mut ActNode, n: usize, token: *const u8, s: *const u8, rng: *const u8,
                                  out_proof: *mut u8, out_prerefund: *mut u8, status: *mut u8) -> c_int;
    fn act_node_prove_spend_seeded_batch(node: *mut ActNode, n: usize, token: *const u8, s: *const u8, seed: *const u8, first_lane: u64,
                                         out_proof: *mut u8, out_prerefund: *mut u8, status: *mut u8) -> c_int;
    fn act_node_verify_spend_batch(node: *mut ActNode, n: usize, sk: *const u8, proof: *const u8, status: *mut u8, out_kprime: *mut u8) -> c_int;
    fn act_node_issue_batch(node: *mut ActNode, n: usize, sk: *const u8, req: *const u8, c: *const u8, rng: *const u8, rng_mode: c_int,
                            out_resp: *mut u8, status: *mut u8) -> c_int;
    fn act_node_refund_batch(node: *mut ActNode, n: usize, sk: *const u8, proof: *const u8, rng: *const u8, rng_mode: c_int,
                             out_refund: *mut u8, status: *mut u8) -> c_int;
    fn act_node_refund_sign_batch(node: *mut ActNode, n: usize, sk: *const u8, kprime: *const u8, status_in: *const u8,
                                  rng: *const u8, rng_mode: c_int, out_refund: *mut u8, status: *mut u8) -> c_int;
    fn act_node_refund_to_credit_token_batch(node: *mut ActNode, n: usize, prerefund: *const u8, proof: *const u8, refund: *const u8,
                                             w: *const u8, out_token: *mut u8, status: *mut u8) -> c_int;
    // the same two against a ring of issuer public keys (one GPU; `PublicRing` below)
    fn act_issuance_to_credit_token_keyring_batch(ctx: *mut ActCtx, n: usize, mem: c_int, pre: *const u8, ring_w: *const u8, nkeys: u32,
                                                  req: *const u8, resp: *const u8, out_token: *mut u8, status: *mut u8, out_key: *mut u8) -> c_int;
    fn act_refund_to_credit_token_keyring_batch(ctx: *mut ActCtx, n: usize, mem: c_int, prerefund: *const u8, proof: *const u8, refund: *const u8,
                                                ring_w: *const u8, nkeys: u32, out_token: *mut u8, status: *mut u8, out_key: *mut u8) -> c_int;
    // wire bytes in, wire bytes out (src/cbor.rs:276-408, src/lib.rs:781-869, src/cbor.rs:421-433) and the redemption step
    // (examples/act.rs:62-73); `rng` with ACT_RNG_CALLBACK points to an ActRngSource
    fn act_node_verify_spend_cbor_batch(node: *mut ActNode, n: usize, sk: *const u8, cbor: *const u8, offsets: *const u64,
                                        status: *mut u8, out_kprime: *mut u8) -> c_int;
    fn act_node_refund_cbor_batch(node: *mut ActNode, n: usize, sk: *const u8, cbor: *const u8, offsets: *const u64,
                                  rng: *const u8, rng_mode: c_int, out_refund_cbor: *mut u8, status: *mut u8) -> c_int;
    // issuance on wire bytes (src/cbor.rs:118-148, src/lib.rs:621-663, src/cbor.rs:162-175)
    fn act_node_issue_check_cbor_batch(node: *mut ActNode, n: usize, cbor: *const u8, offsets: *const u64, status: *mut u8,
                                       out_req: *mut u8) -> c_int;
    fn act_node_issue_sign_cbor_batch(node: *mut ActNode, n: usize, sk: *const u8, req: *const u8, c: *const u8, status_in: *const u8,
                                      rng: *const u8, rng_mode: c_int, out_resp_cbor: *mut u8, status: *mut u8) -> c_int;
    fn act_node_issue_cbor_batch(node: *mut ActNode, n: usize, sk: *const u8, cbor: *const u8, offsets: *const u64, c: *const u8,
                                 rng: *const u8, rng_mode: c_int, out_resp_cbor: *mut u8, status: *mut u8) -> c_int;
    fn act_node_redeem_batch(node: *mut ActNode, set: *mut ActNodeNullifierSet, n: usize, sk: *const u8, proof: *const u8,
                             rng: *const u8, rng_mode: c_int, out_refund: *mut u8, status: *mut u8) -> c_int;
    fn act_node_redeem_cbor_batch(node: *mut ActNode, set: *mut ActNodeNullifierSet, n: usize, sk: *const u8, cbor: *const u8,
                                  offsets: *const u64, rng: *const u8, rng_mode: c_int, out_refund_cbor: *mut u8, status: *mut u8) -> c_int;
    fn act_node_redeem_keyring_batch(node: *mut ActNode, set: *mut ActNodeNullifierSet, n: usize, keys: *const u8, nkeys: c_int, sign_key: c_int,
                                     proof: *const u8, rng: *const u8, rng_mode: c_int, out_refund: *mut u8, status: *mut u8, out_key: *mut u8) -> c_int;
    fn act_node_redeem_cbor_keyring_batch(node: *mut ActNode, set: *mut ActNodeNullifierSet, n: usize, keys: *const u8, nkeys: c_int, sign_key: c_int,
                                          cbor: *const u8, offsets: *const u64, rng: *const u8, rng_mode: c_int, out_refund_cbor: *mut u8,
                                          status: *mut u8, out_key: *mut u8) -> c_int;
    fn act_node_nullifier_set_create(devices: *const c_int, n_devices: c_int, capacity_per_device: usize, salt: *const u8,
                                     out: *mut *mut ActNodeNullifierSet) -> c_int;
    fn act_node_nullifier_set_destroy(set: *mut ActNodeNullifierSet);
    fn act_node_nullifier_set_len(set: *const ActNodeNullifierSet) -> usize;
    fn act_node_nullifier_set_last_error(set: *const ActNodeNullifierSet) -> *const c_char;
    fn act_node_nullifier_check_and_insert_batch(set: *mut ActNodeNullifierSet, n: usize, nullifiers: *const u8, stride: usize, skip_mask: *const u8,
                                                 out_spent: *mut u8) -> c_int;
    fn act_node_nullifier_set_reserve(set: *mut ActNodeNullifierSet, capacity_per_device: usize) -> c_int;
    fn act_node_nullifier_set_export(set: *mut ActNodeNullifierSet, cursor: *mut u64, max_keys: usize, out_keys: *mut u8, n_out: *mut usize) -> c_int;
    fn act_node_nullifier_contains_batch(set: *mut ActNodeNullifierSet, n: usize, nullifiers: *const u8, stride: usize, out_found: *mut u8) -> c_int;
    fn act_node_nullifier_check_and_insert_epoch_batch(set: *mut ActNodeNullifierSet, n: usize, nullifiers: *const u8, stride: usize, skip_mask: *const u8,
                                                       epoch_index: *const u8, epoch_table: *const u32, n_epochs: c_int, out_spent: *mut u8) -> c_int;
    fn act_node_nullifier_set_epoch_len(set: *mut ActNodeNullifierSet, epoch: u32, out_count: *mut u64) -> c_int;
    fn act_node_nullifier_set_retire_epoch(set: *mut ActNodeNullifierSet, epoch: u32, out_removed: *mut u64) -> c_int;
    fn act_node_nullifier_set_retired_epochs(set: *mut ActNodeNullifierSet, out_epochs: *mut u32, max_epochs: usize, n_out: *mut usize) -> c_int;
    fn act_node_nullifier_set_export_epochs(set: *mut ActNodeNullifierSet, cursor: *mut u64, max_keys: usize, out_keys: *mut u8, out_epochs: *mut u32,
                                            n_out: *mut usize) -> c_int;
    fn act_node_redeem_keyring_epochs_batch(node: *mut ActNode, set: *mut ActNodeNullifierSet, n: usize, keys: *const u8, nkeys: c_int, key_epochs: *const u32,
                                            sign_key: c_int, proof: *const u8, rng: *const u8, rng_mode: c_int, out_refund: *mut u8, status: *mut u8,
                                            out_key: *mut u8) -> c_int;
    fn act_node_redeem_cbor_keyring_epochs_batch(node: *mut ActNode, set: *mut ActNodeNullifierSet, n: usize, keys: *const u8, nkeys: c_int,
                                                 key_epochs: *const u32, sign_key: c_int, cbor: *const u8, offsets: *const u64, rng: *const u8, rng_mode: c_int,
                                                 out_refund_cbor: *mut u8, status: *mut u8, out_key: *mut u8) -> c_int;
    fn act_redeem_admit_batch(ctx: *mut ActCtx, set: *mut ActNullifierSet, n: usize, mem: c_int, keys: *const u8, nkeys: c_int, key_epochs: *const u32,
                              sign_key: c_int, proof: *const u8, charge: *const u8, rng: *const u8, rng_mode: c_int, out_refund: *mut u8, status: *mut u8,
                              out_key: *mut u8, out_counts: *mut u64) -> c_int;
    fn act_redeem_cbor_admit_batch(ctx: *mut ActCtx, set: *mut ActNullifierSet, n: usize, mem: c_int, keys: *const u8, nkeys: c_int, key_epochs: *const u32,
                                   sign_key: c_int, cbor: *const u8, offsets: *const u64, charge: *const u8, rng: *const u8, rng_mode: c_int,
                                   out_refund_cbor: *mut u8, status: *mut u8, out_key: *mut u8, out_counts: *mut u64) -> c_int;
    fn act_redeem_admit_unique_batch(ctx: *mut ActCtx, set: *mut ActNullifierSet, n: usize, mem: c_int, keys: *const u8, nkeys: c_int, key_epochs: *const u32,
                                     sign_key: c_int, proof: *const u8, charge: *const u8, rng: *const u8, rng_mode: c_int, out_refund: *mut u8, status: *mut u8,
                                     out_key: *mut u8, out_counts: *mut u64) -> c_int;
    fn act_redeem_cbor_admit_unique_batch(ctx: *mut ActCtx, set: *mut ActNullifierSet, n: usize, mem: c_int, keys: *const u8, nkeys: c_int, key_epochs: *const u32,
                                          sign_key: c_int, cbor: *const u8, offsets: *const u64, charge: *const u8, rng: *const u8, rng_mode: c_int,
                                          out_refund_cbor: *mut u8, status: *mut u8, out_key: *mut u8, out_counts: *mut u64) -> c_int;
    fn act_redeem_replay_batch(ctx: *mut ActCtx, set: *mut ActNullifierSet, receipts: *mut ActNullifierSet, n: usize, mem: c_int, keys: *const u8, nkeys: c_int,
                               key_epochs: *const u32, sign_key: c_int, proof: *const u8, nonce_key: *const u8, out_refund: *mut u8, status: *mut u8,
                               out_key: *mut u8, out_replayed: *mut u8, out_counts: *mut u64) -> c_int;
    fn act_redeem_cbor_replay_batch(ctx: *mut ActCtx, set: *mut ActNullifierSet, receipts: *mut ActNullifierSet, n: usize, mem: c_int, keys: *const u8, nkeys: c_int,
                                    key_epochs: *const u32, sign_key: c_int, cbor: *const u8, offsets: *const u64, nonce_key: *const u8, out_refund_cbor: *mut u8,
                                    status: *mut u8, out_key: *mut u8, out_replayed: *mut u8, out_counts: *mut u64) -> c_int;
    fn act_replay_derive_batch(ctx: *mut ActCtx, n: usize, mem: c_int, keys: *const u8, nkeys: c_int, key_index: *const u8, nonce_key: *const u8,
                               nullifiers: *const u8, stride: usize, kprime: *const u8, status_in: *const u8, out_tags: *mut u8, out_nonces: *mut u8) -> c_int;
    fn act_redeem_admit_replay_batch(ctx: *mut ActCtx, set: *mut ActNullifierSet, receipts: *mut ActNullifierSet, n: usize, mem: c_int, keys: *const u8, nkeys: c_int,
                                     key_epochs: *const u32, sign_key: c_int, proof: *const u8, charge: *const u8, nonce_key: *const u8, out_refund: *mut u8,
                                     status: *mut u8, out_key: *mut u8, out_replayed: *mut u8, out_counts: *mut u64) -> c_int;
    fn act_redeem_cbor_admit_replay_batch(ctx: *mut ActCtx, set: *mut ActNullifierSet, receipts: *mut ActNullifierSet, n: usize, mem: c_int, keys: *const u8,
                                          nkeys: c_int, key_epochs: *const u32, sign_key: c_int, cbor: *const u8, offsets: *const u64, charge: *const u8,
                                          nonce_key: *const u8, out_refund_cbor: *mut u8, status: *mut u8, out_key: *mut u8, out_replayed: *mut u8,
                                          out_counts: *mut u64) -> c_int;
    fn act_redeem_admit_replay_unique_batch(ctx: *mut ActCtx, set: *mut ActNullifierSet, receipts: *mut ActNullifierSet, n: usize, mem: c_int, keys: *const u8,
                                            nkeys: c_int, key_epochs: *const u32, sign_key: c_int, proof: *const u8, charge: *const u8, nonce_key: *const u8,
                                            out_refund: *mut u8, status: *mut u8, out_key: *mut u8, out_replayed: *mut u8, out_counts: *mut u64) -> c_int;
    fn act_redeem_cbor_admit_replay_unique_batch(ctx: *mut ActCtx, set: *mut ActNullifierSet, receipts: *mut ActNullifierSet, n: usize, mem: c_int, keys: *const u8,
                                                 nkeys: c_int, key_epochs: *const u32, sign_key: c_int, cbor: *const u8, offsets: *const u64, charge: *const u8,
                                                 nonce_key: *const u8, out_refund_cbor: *mut u8, status: *mut u8, out_key: *mut u8, out_replayed: *mut u8,
                                                 out_counts: *mut u64) -> c_int;
    fn act_node_device_stats(node: *mut ActNode, k: c_int, weight: *mut f64, last_lanes: *mut u64, last_seconds: *mut f64, last_calls: *mut u64) -> c_int;
    fn act_refund_sign_return_keyring_batch(ctx: *mut ActCtx, n: usize, mem: c_int, keys: *const u8, nkeys: c_int, key_index: *const u8, kprime: *const u8,
                                            status_in: *const u8, rng: *const u8, rng_mode: c_int, returned: *const u8, out_refund_return: *mut u8,
                                            status: *mut u8) -> c_int;
    fn act_redeem_return_batch(ctx: *mut ActCtx, set: *mut ActNullifierSet, n: usize, mem: c_int, keys: *const u8, nkeys: c_int, key_epochs: *const u32,
                               sign_key: c_int, proof: *const u8, charge: *const u8, returned: *const u8, rng: *const u8, rng_mode: c_int,
                               out_refund_return: *mut u8, status: *mut u8, out_key: *mut u8, out_counts: *mut u64) -> c_int;
    fn act_redeem_cbor_return_batch(ctx: *mut ActCtx, set: *mut ActNullifierSet, n: usize, mem: c_int, keys: *const u8, nkeys: c_int, key_epochs: *const u32,
                                    sign_key: c_int, cbor: *const u8, offsets: *const u64, charge: *const u8, returned: *const u8, rng: *const u8,
                                    rng_mode: c_int, out_refund_return_cbor: *mut u8, status: *mut u8, out_key: *mut u8, out_counts: *mut u64) -> c_int;
    fn act_refund_to_credit_token_return_batch(ctx: *mut ActCtx, n: usize, mem: c_int, prerefund: *const u8, proof: *const u8, refund_return: *const u8,
                                               w: *const u8, out_token: *mut u8, status: *mut u8) -> c_int;
    // ... against a ring of issuer public keys, and the return calls with byte-identical proofs of one batch verified once
    fn act_refund_to_credit_token_return_keyring_batch(ctx: *mut ActCtx, n: usize, mem: c_int, prerefund: *const u8, proof: *const u8, refund_return: *const u8,
                                                       ring_w: *const u8, nkeys: u32, out_token: *mut u8, status: *mut u8, out_key: *mut u8) -> c_int;
    fn act_redeem_return_unique_batch(ctx: *mut ActCtx, set: *mut ActNullifierSet, n: usize, mem: c_int, keys: *const u8, nkeys: c_int, key_epochs: *const u32,
                                      sign_key: c_int, proof: *const u8, charge: *const u8, returned: *const u8, rng: *const u8, rng_mode: c_int,
                                      out_refund_return: *mut u8, status: *mut u8, out_key: *mut u8, out_counts: *mut u64) -> c_int;
    fn act_redeem_cbor_return_unique_batch(ctx: *mut ActCtx, set: *mut ActNullifierSet, n: usize, mem: c_int, keys: *const u8, nkeys: c_int, key_epochs: *const u32,
                                           sign_key: c_int, cbor: *const u8, offsets: *const u64, charge: *const u8, returned: *const u8, rng: *const u8,
                                           rng_mode: c_int, out_refund_return_cbor: *mut u8, status: *mut u8, out_key: *mut u8, out_counts: *mut u64) -> c_int;
    fn act_redeem_return_replay_batch(ctx: *mut ActCtx, set: *mut ActNullifierSet, receipts: *mut ActNullifierSet, n: usize, mem: c_int, keys: *const u8, nkeys: c_int,
                                      key_epochs: *const u32, sign_key: c_int, proof: *const u8, charge: *const u8, amounts: *const u8, nonce_key: *const u8,
                                      out_refund_return: *mut u8, status: *mut u8, out_key: *mut u8, out_replayed: *mut u8, out_counts: *mut u64) -> c_int;
    fn act_redeem_cbor_return_replay_batch(ctx: *mut ActCtx, set: *mut ActNullifierSet, receipts: *mut ActNullifierSet, n: usize, mem: c_int, keys: *const u8,
                                           nkeys: c_int, key_epochs: *const u32, sign_key: c_int, cbor: *const u8, offsets: *const u64, charge: *const u8,
                                           amounts: *const u8, nonce_key: *const u8, out_refund_return_cbor: *mut u8, status: *mut u8, out_key: *mut u8,
                                           out_replayed: *mut u8, out_counts: *mut u64) -> c_int;
    fn act_replay_derive_return_batch(ctx: *mut ActCtx, n: usize, mem: c_int, keys: *const u8, nkeys: c_int, key_index: *const u8, nonce_key: *const u8,
                                      nullifiers: *const u8, stride: usize, kprime: *const u8, status_in: *const u8, amounts: *const u8, out_tags: *mut u8,
                                      out_nonces: *mut u8) -> c_int;
    fn act_redeem_return_replay_unique_batch(ctx: *mut ActCtx, set: *mut ActNullifierSet, receipts: *mut ActNullifierSet, n: usize, mem: c_int, keys: *const u8,
                                             nkeys: c_int, key_epochs: *const u32, sign_key: c_int, proof: *const u8, charge: *const u8, amounts: *const u8,
                                             nonce_key: *const u8, out_refund_return: *mut u8, status: *mut u8, out_key: *mut u8, out_replayed: *mut u8,
                                             out_counts: *mut u64) -> c_int;
    fn act_redeem_cbor_return_replay_unique_batch(ctx: *mut ActCtx, set: *mut ActNullifierSet, receipts: *mut ActNullifierSet, n: usize, mem: c_int, keys: *const u8,
                                                  nkeys: c_int, key_epochs: *const u32, sign_key: c_int, cbor: *const u8, offsets: *const u64, charge: *const u8,
                                                  amounts: *const u8, nonce_key: *const u8, out_refund_return_cbor: *mut u8, status: *mut u8, out_key: *mut u8,
                                                  out_replayed: *mut u8, out_counts: *mut u64) -> c_int;
    // reserve and settle: record a spend now, sign its partial refund later
    fn act_redeem_reserve_batch(ctx: *mut ActCtx, set: *mut ActNullifierSet, receipts: *mut ActNullifierSet, n: usize, mem: c_int, keys: *const u8, nkeys: c_int,
                                key_epochs: *const u32, proof: *const u8, charge: *const u8, out_reservation: *mut u8, status: *mut u8, out_key: *mut u8,
                                out_replayed: *mut u8, out_counts: *mut u64) -> c_int;
    fn act_redeem_cbor_reserve_batch(ctx: *mut ActCtx, set: *mut ActNullifierSet, receipts: *mut ActNullifierSet, n: usize, mem: c_int, keys: *const u8, nkeys: c_int,
                                     key_epochs: *const u32, cbor: *const u8, offsets: *const u64, charge: *const u8, out_reservation: *mut u8, status: *mut u8,
                                     out_key: *mut u8, out_replayed: *mut u8, out_counts: *mut u64) -> c_int;
    fn act_redeem_settle_batch(ctx: *mut ActCtx, receipts: *mut ActNullifierSet, n: usize, mem: c_int, keys: *const u8, nkeys: c_int, key_epochs: *const u32,
                               sign_key: c_int, reservation: *const u8, key_index: *const u8, amounts: *const u8, nonce_key: *const u8, out_refund_return: *mut u8,
                               status: *mut u8, out_settled_before: *mut u8, out_counts: *mut u64) -> c_int;
    fn act_redeem_cbor_settle_batch(ctx: *mut ActCtx, receipts: *mut ActNullifierSet, n: usize, mem: c_int, keys: *const u8, nkeys: c_int, key_epochs: *const u32,
                                    sign_key: c_int, reservation: *const u8, key_index: *const u8, amounts: *const u8, nonce_key: *const u8,
                                    out_refund_return_cbor: *mut u8, status: *mut u8, out_settled_before: *mut u8, out_counts: *mut u64) -> c_int;
    // request binding: 32 caller bytes per lane enter the spend challenge (bind null: the call each extends)
    fn act_prove_spend_bound_batch(ctx: *mut ActCtx, n: usize, mem: c_int, token: *const u8, s: *const u8, rng: *const u8, bind: *const u8,
                                   out_proof: *mut u8, out_prerefund: *mut u8, status: *mut u8) -> c_int;
    fn act_verify_spend_keyring_bound_batch(ctx: *mut ActCtx, n: usize, mem: c_int, keys: *const u8, nkeys: c_int, proof: *const u8, bind: *const u8,
                                            status: *mut u8, out_key: *mut u8, out_kprime: *mut u8) -> c_int;
    fn act_redeem_return_replay_bound_batch(ctx: *mut ActCtx, set: *mut ActNullifierSet, receipts: *mut ActNullifierSet, n: usize, mem: c_int, keys: *const u8,
                                            nkeys: c_int, key_epochs: *const u32, sign_key: c_int, proof: *const u8, bind: *const u8, charge: *const u8,
                                            amounts: *const u8, nonce_key: *const u8, out_refund_return: *mut u8, status: *mut u8, out_key: *mut u8,
                                            out_replayed: *mut u8, out_counts: *mut u64) -> c_int;
    fn act_redeem_cbor_return_replay_bound_batch(ctx: *mut ActCtx, set: *mut ActNullifierSet, receipts: *mut ActNullifierSet, n: usize, mem: c_int, keys: *const u8,
                                                 nkeys: c_int, key_epochs: *const u32, sign_key: c_int, cbor: *const u8, offsets: *const u64, bind: *const u8,
                                                 charge: *const u8, amounts: *const u8, nonce_key: *const u8, out_refund_return_cbor: *mut u8, status: *mut u8,
                                                 out_key: *mut u8, out_replayed: *mut u8, out_counts: *mut u64) -> c_int;
    fn act_redeem_reserve_bound_batch(ctx: *mut ActCtx, set: *mut ActNullifierSet, receipts: *mut ActNullifierSet, n: usize, mem: c_int, keys: *const u8, nkeys: c_int,
                                      key_epochs: *const u32, proof: *const u8, bind: *const u8, charge: *const u8, out_reservation: *mut u8, status: *mut u8,
                                      out_key: *mut u8, out_replayed: *mut u8, out_counts: *mut u64) -> c_int;
    fn act_redeem_cbor_reserve_bound_batch(ctx: *mut ActCtx, set: *mut ActNullifierSet, receipts: *mut ActNullifierSet, n: usize, mem: c_int, keys: *const u8,
                                           nkeys: c_int, key_epochs: *const u32, cbor: *const u8, offsets: *const u64, bind: *const u8, charge: *const u8,
                                           out_reservation: *mut u8, status: *mut u8, out_key: *mut u8, out_replayed: *mut u8, out_counts: *mut u64) -> c_int;
    // test hook: one field operation per lane on raw 9-limb operands, in the per-column or the range kernel's build of the field code
    fn act_debug_fe_batch(ctx: *mut ActCtx, pair_build: c_int, op: c_int, n: usize, f: *const u32, g: *const u32, fb: *const u32, gb_or_a: *const u32,
                          h: *mut u32, hb: *mut u32) -> c_int;
    // test hook: one operation of the scalar arithmetic mod l per lane, on records of 16 words
    fn act_debug_sc_batch(ctx: *mut ActCtx, op: c_int, n: usize, a: *const u32, b: *const u32, c: *const u32, r: *mut u32) -> c_int;
    // test hooks: one product of a secret scalar per lane -- the matrix-core look-up over the context's table image, the address-free chains
    fn act_debug_fixed_base_mf_batch(ctx: *mut ActCtx, base: c_int, block_threads: c_int, n: usize, mem: c_int, scalars: *const u8, out: *mut u8) -> c_int;
    fn act_debug_chain_ct_batch(ctx: *mut ActCtx, mode: c_int, n: usize, mem: c_int, points: *const u8, scalars: *const u8, scalars2: *const u8,
                                out: *mut u8, out2: *mut u8, status: *mut u8) -> c_int;
}

/// ACT_MI355X_DEVICES = "0,1,2,3,4,5,6,7" (default: device 0)
fn devices_from_env() -> Vec<c_int> {
    std::env::var("ACT_MI355X_DEVICES").map(|s| s.split(',').filter_map(|d| d.trim().parse().ok()).collect()).unwrap_or_else(|_| vec![0])
}

/// All GPUs of the node behind one handle (contiguous pieces, load-balanced, no collective).
///
/// How `Params` (src/lib.rs:222-229, `#[derive(Clone)]`) carries it: add the field
/// `#[cfg(feature = "mi355x")] gpu: GpuSlot` and nothing else -- `GpuSlot` below is `Clone` (a clone starts EMPTY and builds its own
/// handle on first use, so `#[derive(Clone)]` on `Params` keeps compiling and clones never share engine state), `Default`, `Send`
/// and `Sync`.
///
/// Threads: safe Rust may call `request` / `issue` / `refund` on one `&Params` from many threads at once.  The library serialises
/// them itself -- every `act_node_*_batch` call takes the node handle's lock and every context entry point the context's
/// (include/act_mi355x.h, "A node handle ... may be shared between host threads") -- so concurrent callers are served one after
/// the other and never observe each other's staging buffers, cached key or error string.  That is why `Gpu` may be `Sync`; the
/// guarantee lives in the library, not in a promise by the caller.
pub struct Gpu(*mut ActNode);
// SAFETY: the handle is only ever passed to act_node_* entry points.  Calls that are cut over the GPUs take the node's lock
// (csrc/node.cpp `node_lock`); the few-item calls that go to one context are serialised by that context's lock -- either way no two
// threads are ever inside the same context's buffers.  act_node_destroy runs from Drop, i.e. with exclusive access.  The error text is safe too: act_node_last_error copies the
// CALLING thread's own last failure on the handle (kept per thread by the library) into a buffer of that thread, valid until it asks
// again, so `check` below neither reads a string another thread's failing call is rewriting nor reports another thread's error.
unsafe impl Send for Gpu {}
unsafe impl Sync for Gpu {}
impl Drop for Gpu {
    fn drop(&mut self) {
        unsafe { act_node_destroy(self.0) }
    }
}

/// The `Params` field: a lazily built `Gpu` that does not get in the way of `#[derive(Clone)]`.
#[derive(Default)]
pub struct GpuSlot(OnceLock<Gpu>);
impl Clone for GpuSlot {
    fn clone(&self) -> Self {
        GpuSlot(OnceLock::new()) // a cloned Params builds its own node handle on first use
    }
}
impl std::fmt::Debug for GpuSlot {
    fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result {
        f.write_str(if self.0.get().is_some() { "GpuSlot(ready)" } else { "GpuSlot(empty)" })
    }
}

impl Gpu {
    fn new(params: &Params) -> Gpu {
        let mut h = [0u8; 96]; // enc(h1) | enc(h2) | enc(h3), as Transcript::new hashes them (src/transcript.rs:64-66)
        h[..32].copy_from_slice(params.h1.basepoint().compress().as_bytes());
        h[32..64].copy_from_slice(params.h2.basepoint().compress().as_bytes());
        h[64..].copy_from_slice(params.h3.basepoint().compress().as_bytes());
        let devices = devices_from_env();
        // The library never touches the process environment.  A service with many HIP streams exports GPU_MAX_HW_QUEUES=8 before its
        // first HIP call; the engine measures whether its two pipeline streams overlap either way.
        // ACT_MI355X_MAX_BATCH: records per internal launch.  Unset = the library default, 65 536: 27 GB of workspace per GPU
        // + 0.5 GB of tables, and nothing else: wider fixed-base windows (+47 GB, +3 % verifies/s) are asked for explicitly with
        // act_node_set_fixed_base_bits (include/act_mi355x.h).  A service that only ever sees small batches sets e.g. 4096 (1.7 GB).
        let max_batch: usize = std::env::var("ACT_MI355X_MAX_BATCH").ok().and_then(|s| s.parse().ok()).unwrap_or(0);
        let mut node = std::ptr::null_mut();
        let rc = unsafe { act_node_create(h.as_ptr(), L as c_int, devices.as_ptr(), devices.len() as c_int, max_batch, &mut node) };
        if rc != 0 {
            let msg = if node.is_null() { String::new() } else { unsafe { CStr::from_ptr(act_node_last_error(node)) }.to_string_lossy().into_owned() };
            panic!("act_node_create failed ({rc}): {msg}"); // infrastructure failure, not a protocol error
        }
        Gpu(node)
    }
    fn check(&self, rc: c_int) {
        if rc != 0 {
            let msg = unsafe { CStr::from_ptr(act_node_last_error(self.0)) }.to_string_lossy().into_owned();
            panic!("MI355X engine failure ({rc}): {msg}");
        }
    }
}

impl Params {
    pub(crate) fn gpu(&self) -> &Gpu {
        self.gpu.0.get_or_init(|| Gpu::new(self))
    }
}

fn status_to_error(s: u8) -> Error {
    match s {
        // 1 + discriminant, src/lib.rs:102-112
        1 => Error::InvalidIssuanceRequestProof,
        2 => Error::InvalidIssuanceResponseProof,
        3 => Error::DoubleSpendError,
        4 => Error::InvalidRefundProof,
        5 => Error::InvalidRefundResponseProof,
        6 => Error::IdentityPointError,
        7 => Error::InvalidClientSpendProof,
        8 => Error::AmountTooBigError,
        _ => Error::ScalarOutOfRangeError, // 255 cannot occur: every point of a Rust struct is a valid RistrettoPoint
    }
}

// ---- record marshalling ------------------------------------------------------------------------------------------
fn put_s(out: &mut Vec<u8>, s: &Scalar) {
    out.extend_from_slice(s.as_bytes());
}
fn put_p(out: &mut Vec<u8>, p: &RistrettoPoint) {
    out.extend_from_slice(p.compress().as_bytes());
}
fn get_s(rec: &[u8], field: usize) -> Scalar {
    // the engine writes canonical scalars
    Scalar::from_canonical_bytes(rec[32 * field..32 * field + 32].try_into().unwrap()).unwrap()
}
fn get_p(rec: &[u8], field: usize) -> RistrettoPoint {
    CompressedRistretto::from_slice(&rec[32 * field..32 * field + 32]).unwrap().decompress().expect("engine wrote a valid point")
}
/// `count` x `Scalar::random` worth of bytes, drawn exactly as dalek draws them: one 64-byte `fill_bytes` each.
fn draw(rng: &mut impl CryptoRngCore, count: usize) -> Vec<u8> {
    let mut buf = vec![0u8; 64 * count];
    for chunk in buf.chunks_exact_mut(64) {
        rng.fill_bytes(chunk);
    }
    buf
}

// Marshalling is the expensive part of the struct-level batch API: a `RistrettoPoint` becomes 32 bytes by `compress()` (one inverse
// square root, ~4 us on one core) and comes back by `decompress()` (another).  A SpendProof holds 130 points: ~0.5 ms of compress per
// proof = ~2 000 proofs/s per core in front of an engine that verifies ~514 000/s per GPU (INTEGRATION.md section 6 has the measured
// figures).  So records are written and read on `std::thread::scope` workers, one slice of the batch each; a server that can should
// use the wire-level calls further down (`refund_cbor_batch`), where no point is ever built on the host.
fn workers_for(items: usize) -> usize {
    let cpus = std::thread::available_parallelism().map(|n| n.get()).unwrap_or(1);
    cpus.min(items / 8).max(1) // fewer than 8 items per worker is not worth a thread
}
/// `rec_bytes` per item, written by `write(item, out)` (which appends exactly `rec_bytes`), on scoped worker threads.
fn marshal<T: Sync>(items: &[T], rec_bytes: usize, write: impl Fn(&T, &mut Vec<u8>) + Sync) -> Vec<u8> {
    let n = items.len();
    let workers = workers_for(n);
    if workers == 1 {
        let mut out = Vec::with_capacity(n * rec_bytes);
        items.iter().for_each(|it| write(it, &mut out));
        return out;
    }
    let per = (n + workers - 1) / workers;
    let parts: Vec<Vec<u8>> = std::thread::scope(|sc| {
        let handles: Vec<_> = items
            .chunks(per)
            .map(|chunk| {
                let write = &write;
                sc.spawn(move || {
                    let mut out = Vec::with_capacity(chunk.len() * rec_bytes);
                    chunk.iter().for_each(|it| write(it, &mut out));
                    out
                })
            })
            .collect();
        handles.into_iter().map(|h| h.join().expect("marshalling worker")).collect()
    });
    let mut out = Vec::with_capacity(n * rec_bytes);
    parts.iter().for_each(|p| out.extend_from_slice(p));
    out
}
/// The reverse: `n` results from `rec_bytes`-sized records + statuses, `read(record)` on scoped worker threads.
fn unmarshal<T: Send>(records: &[u8], rec_bytes: usize, status: &[u8], read: impl Fn(&[u8]) -> T + Sync) -> Vec<Result<T, Error>> {
    let n = status.len();
    let one = |i: usize| if status[i] == 0 { Ok(read(&records[rec_bytes * i..rec_bytes * (i + 1)])) } else { Err(status_to_error(status[i])) };
    let workers = workers_for(n);
    if workers == 1 {
        return (0..n).map(one).collect();
    }
    let per = (n + workers - 1) / workers;
    let parts: Vec<Vec<Result<T, Error>>> = std::thread::scope(|sc| {
        let handles: Vec<_> = (0..n)
            .step_by(per)
            .map(|lo| {
                let one = &one;
                sc.spawn(move || (lo..(lo + per).min(n)).map(one).collect::<Vec<_>>())
            })
            .collect();
        handles.into_iter().map(|h| h.join().expect("unmarshalling worker")).collect()
    });
    parts.into_iter().flatten().collect()
}

impl PrivateKey {
    fn record(&self) -> [u8; 64] {
        // x | w (src/cbor.rs:477-480)
        let mut r = [0u8; 64];
        r[..32].copy_from_slice(self.x.as_bytes());
        r[32..].copy_from_slice(self.public.w.compress().as_bytes());
        r
    }
}
impl IssuanceRequest {
    fn write_record(&self, out: &mut Vec<u8>) {
        // K | gamma | k_bar | r_bar (src/cbor.rs:105-110)
        put_p(out, &self.big_k);
        put_s(out, &self.gamma);
        put_s(out, &self.k_bar);
        put_s(out, &self.r_bar);
    }
    fn from_record(r: &[u8]) -> Self {
        IssuanceRequest { big_k: get_p(r, 0), gamma: get_s(r, 1), k_bar: get_s(r, 2), r_bar: get_s(r, 3) }
    }
}
impl IssuanceResponse {
    fn write_record(&self, out: &mut Vec<u8>) {
        // A | e | gamma | z | c (src/cbor.rs:163-169)
        put_p(out, &self.a);
        for s in [&self.e, &self.gamma, &self.z, &self.c] {
            put_s(out, s);
        }
    }
    fn from_record(r: &[u8]) -> Self {
        IssuanceResponse { a: get_p(r, 0), e: get_s(r, 1), gamma: get_s(r, 2), z: get_s(r, 3), c: get_s(r, 4) }
    }
}
impl CreditToken {
    fn write_record(&self, out: &mut Vec<u8>) {
        // a | e | k | r | c (src/cbor.rs:596-602)
        put_p(out, &self.a);
        for s in [&self.e, &self.k, &self.r, &self.c] {
            put_s(out, s);
        }
    }
    fn from_record(r: &[u8]) -> Self {
        CreditToken { a: get_p(r, 0), e: get_s(r, 1), k: get_s(r, 2), r: get_s(r, 3), c: get_s(r, 4) }
    }
}
impl SpendProof {
    /// k | s | A' | B_bar | Com[L] | gamma | e_bar | r2_bar | r3_bar | c_bar | r_bar | w00 | w01 | gamma0[L] | z[L][2] | k_bar | s_bar
    /// (src/cbor.rs:250-268)
    fn write_record(&self, out: &mut Vec<u8>) {
        put_s(out, &self.k);
        put_s(out, &self.s);
        put_p(out, &self.a_prime);
        put_p(out, &self.b_bar);
        self.com.iter().for_each(|c| put_p(out, c));
        for s in [&self.gamma, &self.e_bar, &self.r2_bar, &self.r3_bar, &self.c_bar, &self.r_bar, &self.w00, &self.w01] {
            put_s(out, s);
        }
        self.gamma0.iter().for_each(|g| put_s(out, g));
        self.z.iter().for_each(|z| {
            put_s(out, &z[0]);
            put_s(out, &z[1]);
        });
        put_s(out, &self.k_bar);
        put_s(out, &self.s_bar);
    }
    fn from_record(r: &[u8]) -> Self {
        let mut com = [RistrettoPoint::default(); L];
        let mut gamma0 = [Scalar::ZERO; L];
        let mut z = [[Scalar::ZERO; 2]; L];
        for j in 0..L {
            com[j] = get_p(r, 4 + j);
            gamma0[j] = get_s(r, 12 + L + j);
            z[j] = [get_s(r, 12 + 2 * L + 2 * j), get_s(r, 13 + 2 * L + 2 * j)];
        }
        SpendProof {
            k: get_s(r, 0), s: get_s(r, 1), a_prime: get_p(r, 2), b_bar: get_p(r, 3), com,
            gamma: get_s(r, 4 + L), e_bar: get_s(r, 5 + L), r2_bar: get_s(r, 6 + L), r3_bar: get_s(r, 7 + L),
            c_bar: get_s(r, 8 + L), r_bar: get_s(r, 9 + L), w00: get_s(r, 10 + L), w01: get_s(r, 11 + L),
            gamma0, z, k_bar: get_s(r, 12 + 4 * L), s_bar: get_s(r, 13 + 4 * L),
        }
    }
}
impl Refund {
    fn write_record(&self, out: &mut Vec<u8>) {
        // A* | e | gamma | z (src/cbor.rs:422-427)
        put_p(out, &self.a);
        for s in [&self.e, &self.gamma, &self.z] {
            put_s(out, s);
        }
    }
    fn from_record(r: &[u8]) -> Self {
        Refund { a: get_p(r, 0), e: get_s(r, 1), gamma: get_s(r, 2), z: get_s(r, 3) }
    }
}

// ---- the batch siblings ----------------------------------------------------------------------------------------------
impl PreIssuance {
    /// Batch sibling of `request` (src/lib.rs:463-487): lane i draws k', r' (2 x 64 bytes), in lane order.
    pub fn request_batch(pres: &[PreIssuance], params: &Params, mut rng: impl CryptoRngCore) -> Vec<IssuanceRequest> {
        let n = pres.len();
        let mut rec = Vec::with_capacity(64 * n);
        for p in pres {
            put_s(&mut rec, &p.r); // r | k (src/cbor.rs:546-549)
            put_s(&mut rec, &p.k);
        }
        let rng_bytes = draw(&mut rng, 2 * n);
        let mut out = vec![0u8; 128 * n];
        let gpu = params.gpu();
        gpu.check(unsafe { act_node_request_batch(gpu.0, n, rec.as_ptr(), rng_bytes.as_ptr(), out.as_mut_ptr()) });
        out.chunks_exact(128).map(IssuanceRequest::from_record).collect()
    }

    /// Batch sibling of `to_credit_token` (src/lib.rs:528-562).
    pub fn to_credit_token_batch(pres: &[PreIssuance], params: &Params, public: &PublicKey, requests: &[IssuanceRequest],
                                 responses: &[IssuanceResponse]) -> Vec<Result<CreditToken, Error>> {
        let n = pres.len();
        assert!(requests.len() == n && responses.len() == n);
        let (mut pre, mut req, mut resp) = (Vec::with_capacity(64 * n), Vec::with_capacity(128 * n), Vec::with_capacity(160 * n));
        for i in 0..n {
            put_s(&mut pre, &pres[i].r);
            put_s(&mut pre, &pres[i].k);
            requests[i].write_record(&mut req);
            responses[i].write_record(&mut resp);
        }
        let w = public.w.compress();
        let (mut out, mut status) = (vec![0u8; 160 * n], vec![0u8; n]);
        let gpu = params.gpu();
        gpu.check(unsafe {
            act_node_issuance_to_credit_token_batch(gpu.0, n, pre.as_ptr(), w.as_bytes().as_ptr(), req.as_ptr(), resp.as_ptr(), out.as_mut_ptr(), status.as_mut_ptr())
        });
        (0..n).map(|i| if status[i] == 0 { Ok(CreditToken::from_record(&out[160 * i..160 * i + 160])) } else { Err(status_to_error(status[i])) }).collect()
    }
}

impl PrivateKey {
    /// Batch sibling of `issue` (src/lib.rs:621-663).  e, alpha are drawn only for lanes whose PoK verified, in lane order.
    pub fn issue_batch(&self, params: &Params, requests: &[IssuanceRequest], amounts: &[Scalar], mut rng: impl CryptoRngCore)
        -> Vec<Result<IssuanceResponse, Error>> {
        let n = requests.len();
        assert_eq!(amounts.len(), n);
        let (mut req, mut c) = (Vec::with_capacity(128 * n), Vec::with_capacity(32 * n));
        requests.iter().for_each(|r| r.write_record(&mut req));
        amounts.iter().for_each(|a| put_s(&mut c, a));
        let sk = self.record();
        let gpu = params.gpu();
        let mut checked = vec![0u8; n];
        gpu.check(unsafe { act_node_issue_check_batch(gpu.0, n, req.as_ptr(), checked.as_mut_ptr()) }); // :629-640
        let accepted = checked.iter().filter(|&&s| s == 0).count();
        let rng_bytes = draw(&mut rng, 2 * accepted); // :643, :649 -- exactly what the sequential loop would have drawn
        let (mut out, mut status) = (vec![0u8; 160 * n], vec![0u8; n]);
        gpu.check(unsafe {
            act_node_issue_sign_batch(gpu.0, n, sk.as_ptr(), req.as_ptr(), c.as_ptr(), checked.as_ptr(), rng_bytes.as_ptr(), ACT_RNG_SEQUENTIAL,
                                      out.as_mut_ptr(), status.as_mut_ptr())
        });
        (0..n).map(|i| if status[i] == 0 { Ok(IssuanceResponse::from_record(&out[160 * i..160 * i + 160])) } else { Err(status_to_error(status[i])) }).collect()
    }

    /// Batch sibling of `refund` (src/lib.rs:781-869): verification (:787-844) on the GPUs, then e, alpha for the accepted
    /// lanes only (:846, :852), then the BBS signature on K' (:848-868).
    pub fn refund_batch(&self, params: &Params, proofs: &[SpendProof], mut rng: impl CryptoRngCore) -> Vec<Result<Refund, Error>> {
        let n = proofs.len();
        let rec = marshal(proofs, PROOF_BYTES, |p, out| p.write_record(out)); // 130 compress() per proof: on all cores
        let sk = self.record();
        let gpu = params.gpu();
        let (mut checked, mut kprime) = (vec![0u8; n], vec![0u8; 32 * n]);
        gpu.check(unsafe { act_node_verify_spend_batch(gpu.0, n, sk.as_ptr(), rec.as_ptr(), checked.as_mut_ptr(), kprime.as_mut_ptr()) });
        let accepted = checked.iter().filter(|&&s| s == 0).count();
        let rng_bytes = draw(&mut rng, 2 * accepted);
        let (mut out, mut status) = (vec![0u8; 128 * n], vec![0u8; n]);
        gpu.check(unsafe {
            act_node_refund_sign_batch(gpu.0, n, sk.as_ptr(), kprime.as_ptr(), checked.as_ptr(), rng_bytes.as_ptr(), ACT_RNG_SEQUENTIAL,
                                       out.as_mut_ptr(), status.as_mut_ptr())
        });
        unmarshal(&out, 128, &status, Refund::from_record)
    }
}

impl CreditToken {
    /// Batch sibling of `prove_spend` (src/lib.rs:972-1152): lane i draws its 4L + 12 scalars in the order of :978-1058.
    pub fn prove_spend_batch(tokens: &[CreditToken], params: &Params, charges: &[Scalar], mut rng: impl CryptoRngCore)
        -> Vec<(SpendProof, PreRefund)> {
        let n = tokens.len();
        assert_eq!(charges.len(), n);
        let tok = marshal(tokens, 160, |t, out| t.write_record(out));
        let mut s = Vec::with_capacity(32 * n);
        charges.iter().for_each(|c| put_s(&mut s, c));
        let rng_bytes = draw(&mut rng, (4 * L + 12) * n);
        debug_assert_eq!(rng_bytes.len(), PROVE_RNG_BYTES * n);
        let (mut proofs, mut prer, mut status) = (vec![0u8; PROOF_BYTES * n], vec![0u8; 96 * n], vec![0u8; n]);
        let gpu = params.gpu();
        gpu.check(unsafe {
            act_node_prove_spend_batch(gpu.0, n, tok.as_ptr(), s.as_ptr(), rng_bytes.as_ptr(), proofs.as_mut_ptr(), prer.as_mut_ptr(), status.as_mut_ptr())
        });
        proofs_out(&proofs, &prer)
    }
}

/// `prove_spend_batch` under request bindings on ONE GPU (include/act_mi355x.h "request binding"): `binds[i]`, 32 bytes that both sides
/// derive from the request spend i pays for, enter proof i's challenge.  The issuer verifies under the same bytes
/// (`verify_spend_keyring_bound`, `GpuReplay::bound`, `GpuReserve::reserve_bound_batch`).  A bound proof has the layout of a
/// `SpendProof` and is NOT one: the crate's `refund` and every unbound call reject it.  Draw order and bytes are those of
/// `prove_spend_batch`; only the challenge differs.
/// # Safety
/// `ctx` is a live handle (`act_ctx_create` / `act_node_ctx`) made with `params` and L = 128.
pub unsafe fn prove_spend_bound(ctx: *mut ActCtx, tokens: &[CreditToken], charges: &[Scalar], binds: &[[u8; 32]], mut rng: impl CryptoRngCore)
    -> Result<Vec<(SpendProof, PreRefund)>, c_int> {
    let n = tokens.len();
    assert!(charges.len() == n && binds.len() == n);
    let tok = marshal(tokens, 160, |t, out| t.write_record(out));
    let mut s = Vec::with_capacity(32 * n);
    charges.iter().for_each(|c| put_s(&mut s, c));
    let bind: Vec<u8> = binds.iter().flat_map(|b| b.iter().copied()).collect();
    let rng_bytes = draw(&mut rng, (4 * L + 12) * n);
    let (mut proofs, mut prer, mut status) = (vec![0u8; PROOF_BYTES * n], vec![0u8; 96 * n], vec![0u8; n]);
    let rc = act_prove_spend_bound_batch(ctx, n, 0, tok.as_ptr(), s.as_ptr(), rng_bytes.as_ptr(), bind.as_ptr(), proofs.as_mut_ptr(), prer.as_mut_ptr(),
                                         status.as_mut_ptr());
    if rc != 0 { return Err(rc); }
    Ok(proofs_out(&proofs, &prer))
}
/// The ring verification under request bindings on ONE GPU: `proofs` = n records of `PROOF_BYTES`, `binds` = n values of 32 bytes.
/// -> (rc, statuses, matched ring indices, enc(K') per lane).
/// # Safety
/// `ctx` is a live handle and outlives the call.
pub unsafe fn verify_spend_keyring_bound(ctx: *mut ActCtx, keys: &[u8], proofs: &[u8], binds: &[u8]) -> (c_int, Vec<u8>, Vec<u8>, Vec<u8>) {
    let (n, nkeys) = (proofs.len() / PROOF_BYTES, keys.len() / 64);
    assert!(proofs.len() == n * PROOF_BYTES && binds.len() == 32 * n);
    let (mut status, mut out_key, mut kprime) = (vec![0u8; n + 1], vec![ACT_KEY_NONE; n + 1], vec![0u8; 32 * n + 1]);
    let rc = act_verify_spend_keyring_bound_batch(ctx, n, 0, keys.as_ptr(), nkeys as c_int, proofs.as_ptr(), binds.as_ptr(), status.as_mut_ptr(), out_key.as_mut_ptr(),
                                                  kprime.as_mut_ptr());
    status.truncate(n); out_key.truncate(n); kprime.truncate(32 * n);
    (rc, status, out_key, kprime)
}

/// (proof records, PreRefund records) -> structs; 130 `decompress()` per proof, on scoped worker threads
fn proofs_out(proofs: &[u8], prer: &[u8]) -> Vec<(SpendProof, PreRefund)> {
    let n = prer.len() / 96;
    let zeros = vec![0u8; n]; // prove_spend has no failing lanes: every status is Ok
    let ps = unmarshal(proofs, PROOF_BYTES, &zeros, SpendProof::from_record);
    ps.into_iter()
        .enumerate()
        .map(|(i, p)| {
            let r = &prer[96 * i..96 * i + 96]; // r | k | m (src/cbor.rs:656-660)
            (p.unwrap_or_else(|_| unreachable!()), PreRefund { r: get_s(r, 0), k: get_s(r, 1), m: get_s(r, 2) })
        })
        .collect()
}

/// The generator `prove_spend_seeded_batch` gives lane `lane`: the BLAKE3 XOF of `seed | lane.to_le_bytes()`, read sequentially.
/// `tokens[i].prove_spend(params, charges[i], XofRng::new(&seed, first_lane + i as u64))` is the CPU twin of lane i.
pub struct XofRng(blake3::OutputReader);
impl XofRng {
    pub fn new(seed: &[u8; 32], lane: u64) -> Self {
        let mut h = blake3::Hasher::new();
        h.update(seed);
        h.update(&lane.to_le_bytes());
        XofRng(h.finalize_xof())
    }
}
impl rand_core::RngCore for XofRng {
    fn next_u32(&mut self) -> u32 { let mut b = [0u8; 4]; self.0.fill(&mut b); u32::from_le_bytes(b) }
    fn next_u64(&mut self) -> u64 { let mut b = [0u8; 8]; self.0.fill(&mut b); u64::from_le_bytes(b) }
    fn fill_bytes(&mut self, dest: &mut [u8]) { self.0.fill(dest) }
    fn try_fill_bytes(&mut self, dest: &mut [u8]) -> Result<(), rand_core::Error> { self.0.fill(dest); Ok(()) }
}
impl rand_core::CryptoRng for XofRng {}

impl CreditToken {
    /// `prove_spend_batch` with seeded generators: the 33 536 rng bytes per proof are expanded in HBM (k_xof_expand) instead of being
    /// drawn on the host and copied over PCIe.  `seed` is a secret of the prover; a (seed, lane) pair must never be used twice.
    pub fn prove_spend_seeded_batch(tokens: &[CreditToken], params: &Params, charges: &[Scalar], seed: &[u8; 32], first_lane: u64)
        -> Vec<(SpendProof, PreRefund)> {
        let n = tokens.len();
        assert_eq!(charges.len(), n);
        let tok = marshal(tokens, 160, |t, out| t.write_record(out));
        let mut s = Vec::with_capacity(32 * n);
        charges.iter().for_each(|c| put_s(&mut s, c));
        let (mut proofs, mut prer, mut status) = (vec![0u8; PROOF_BYTES * n], vec![0u8; 96 * n], vec![0u8; n]);
        let gpu = params.gpu();
        gpu.check(unsafe {
            act_node_prove_spend_seeded_batch(gpu.0, n, tok.as_ptr(), s.as_ptr(), seed.as_ptr(), first_lane, proofs.as_mut_ptr(), prer.as_mut_ptr(), status.as_mut_ptr())
        });
        proofs_out(&proofs, &prer)
    }
}

impl PreRefund {
    /// Batch sibling of `to_credit_token` (src/lib.rs:1217-1253).
    pub fn to_credit_token_batch(pres: &[PreRefund], params: &Params, proofs: &[SpendProof], refunds: &[Refund], public_key: &PublicKey)
        -> Vec<Result<CreditToken, Error>> {
        let n = pres.len();
        assert!(proofs.len() == n && refunds.len() == n);
        let (mut pre, mut rf) = (Vec::with_capacity(96 * n), Vec::with_capacity(128 * n));
        for i in 0..n {
            put_s(&mut pre, &pres[i].r);
            put_s(&mut pre, &pres[i].k);
            put_s(&mut pre, &pres[i].m);
            refunds[i].write_record(&mut rf);
        }
        let rec = marshal(proofs, PROOF_BYTES, |p, out| p.write_record(out));
        let w = public_key.w.compress();
        let (mut out, mut status) = (vec![0u8; 160 * n], vec![0u8; n]);
        let gpu = params.gpu();
        gpu.check(unsafe {
            act_node_refund_to_credit_token_batch(gpu.0, n, pre.as_ptr(), rec.as_ptr(), rf.as_ptr(), w.as_bytes().as_ptr(), out.as_mut_ptr(), status.as_mut_ptr())
        });
        (0..n).map(|i| if status[i] == 0 { Ok(CreditToken::from_record(&out[160 * i..160 * i + 160])) } else { Err(status_to_error(status[i])) }).collect()
    }
}

// ---- wire bytes in, wire bytes out ---------------------------------------------------------------------------------------
// A server does not receive `SpendProof`s, it receives bytes.  The loop it runs today --
//     let proof = SpendProof::from_cbor(&msg)?;  let refund = key.refund(&params, &proof, &mut rng)?;  refund.to_cbor()
// (src/cbor.rs:276-408, src/lib.rs:781-869, src/cbor.rs:421-433) -- builds 130 RistrettoPoints per message on the host only to
// have them compressed again for the GPU.  These calls hand the bytes over as they came: no point, no scalar, no `SpendProof` and
// no `Refund` ever exists on the host; message i in, message i out.

/// What a lane of a wire-level call can come back with instead of bytes.
#[derive(Debug, PartialEq)]
pub enum WireError {
    /// `CborError::Ciborium`: not well-formed CBOR
    Malformed,
    /// `CborError::InvalidStructure`: not a map, a field missing, wrong shape or length
    InvalidStructure,
    /// `CborError::InvalidValue`: a point that is not a canonical Ristretto encoding
    InvalidValue,
    /// the message decoded; `refund` (or the nullifier store: `DoubleSpendError`) rejected it
    Protocol(Error),
    /// redeem only, and only together with an engine failure: verified, but the nullifier store could not answer -- NOT recorded,
    /// NOT signed, safe to resubmit (include/act_mi355x.h ACT_STATUS_NULLIFIER_UNDETERMINED)
    NullifierUndetermined,
    /// redeem only, and only together with an engine failure: the nullifier IS recorded and the signature step failed -- the refund
    /// is owed: sign it (`refund`), never redeem it again (ACT_STATUS_RECORDED_UNSIGNED)
    RecordedUnsigned,
}
fn status_to_wire_error(s: u8) -> WireError {
    match s {
        254 => WireError::Malformed,
        253 => WireError::InvalidStructure,
        255 => WireError::InvalidValue,
        252 => WireError::NullifierUndetermined,
        251 => WireError::RecordedUnsigned,
        other => WireError::Protocol(status_to_error(other)),
    }
}

/// The caller's generator as the library's draw callback.  dalek draws a `Scalar::random` with one `fill_bytes(&mut [u8; 64])`;
/// so does this, 64 bytes at a time, so that generators that are not plain byte streams still see the calls they would have seen.
/// Returns 0 = all `len` bytes written; a generator that can fail reports it through `try_fill_bytes` and the library then signs
/// nothing (ACT_ERR_RNG).  (A panic inside the generator cannot unwind through the C frames: the process aborts.)
unsafe extern "C" fn draw_trampoline<R: CryptoRngCore>(rng_ctx: *mut c_void, dst: *mut u8, len: usize) -> c_int {
    let rng = &mut *(rng_ctx as *mut R);
    let buf = std::slice::from_raw_parts_mut(dst, len);
    for chunk in buf.chunks_mut(64) {
        if rng.try_fill_bytes(chunk).is_err() {
            return 1;
        }
    }
    0
}
fn rng_source<R: CryptoRngCore>(rng: &mut R) -> ActRngSource {
    ActRngSource { draw: draw_trampoline::<R>, rng_ctx: rng as *mut R as *mut c_void }
}

/// `msgs` gathered into one buffer + offsets (what the C ABI takes).  The copy is 18 KB per message at memcpy speed; a server that
/// already holds its messages in one buffer calls the `*_blob` forms and skips it.
fn gather(msgs: &[&[u8]]) -> (Vec<u8>, Vec<u64>) {
    let total: usize = msgs.iter().map(|m| m.len()).sum();
    let mut offsets = Vec::with_capacity(msgs.len() + 1);
    let mut blob = Vec::with_capacity(total + 1);
    offsets.push(0u64);
    for m in msgs {
        blob.extend_from_slice(m);
        offsets.push(blob.len() as u64);
    }
    blob.push(0); // never an empty allocation: the library wants a non-null pointer
    (blob, offsets)
}
fn refund_messages(out: &[u8], status: &[u8]) -> Vec<Result<Vec<u8>, WireError>> {
    status
        .iter()
        .enumerate()
        .map(|(i, &s)| if s == 0 { Ok(out[REFUND_CBOR_BYTES * i..REFUND_CBOR_BYTES * (i + 1)].to_vec()) } else { Err(status_to_wire_error(s)) })
        .collect()
}

fn issuance_messages(out: &[u8], status: &[u8]) -> Vec<Result<Vec<u8>, WireError>> {
    const M: usize = ISSUANCE_RESPONSE_CBOR_BYTES;
    status.iter().enumerate().map(|(i, &s)| if s == 0 { Ok(out[M * i..M * (i + 1)].to_vec()) } else { Err(status_to_wire_error(s)) }).collect()
}

impl PrivateKey {
    /// `msgs.iter().map(|m| SpendProof::from_cbor(m).map(|p| self.refund(params, &p, &mut rng)).map(|r| r.to_cbor()))` as ONE call:
    /// CBOR `SpendProof` messages in, CBOR `Refund` messages out, byte for byte what that loop returns, `rng` left where it leaves
    /// it (e, alpha are drawn for accepted lanes only, in lane order, after all verdicts: src/lib.rs:842-852).
    pub fn refund_cbor_batch(&self, params: &Params, msgs: &[&[u8]], rng: impl CryptoRngCore) -> Vec<Result<Vec<u8>, WireError>> {
        let (blob, offsets) = gather(msgs);
        self.refund_cbor_blob(params, &blob, &offsets, rng)
    }
    /// The same over messages that already lie in one buffer: message i = `blob[offsets[i]..offsets[i + 1]]`.
    pub fn refund_cbor_blob(&self, params: &Params, blob: &[u8], offsets: &[u64], mut rng: impl CryptoRngCore) -> Vec<Result<Vec<u8>, WireError>> {
        assert!(!offsets.is_empty() && *offsets.last().unwrap() as usize <= blob.len());
        let n = offsets.len() - 1;
        let sk = self.record();
        let gpu = params.gpu();
        let src = rng_source(&mut rng);
        let (mut out, mut status) = (vec![0u8; REFUND_CBOR_BYTES * n + 1], vec![0u8; n + 1]);
        gpu.check(unsafe {
            act_node_refund_cbor_batch(gpu.0, n, sk.as_ptr(), blob.as_ptr(), offsets.as_ptr(), &src as *const ActRngSource as *const u8,
                                       ACT_RNG_CALLBACK, out.as_mut_ptr(), status.as_mut_ptr())
        });
        refund_messages(&out, &status[..n])
    }
    /// `msgs.iter().zip(amounts).map(|(m, c)| IssuanceRequest::from_cbor(m).map(|r| self.issue(params, &r, *c, &mut rng)).map(|r| r.to_cbor()))`
    /// as ONE call: CBOR `IssuanceRequest` messages in, CBOR `IssuanceResponse` messages out, byte for byte what that loop returns,
    /// `rng` left where it leaves it (e, alpha are drawn for accepted lanes only, in lane order, after all verdicts: src/lib.rs:638-643).
    pub fn issue_cbor_batch(&self, params: &Params, msgs: &[&[u8]], amounts: &[Scalar], rng: impl CryptoRngCore) -> Vec<Result<Vec<u8>, WireError>> {
        let (blob, offsets) = gather(msgs);
        self.issue_cbor_blob(params, &blob, &offsets, amounts, rng)
    }
    /// The same over messages that already lie in one buffer: message i = `blob[offsets[i]..offsets[i + 1]]`.
    pub fn issue_cbor_blob(&self, params: &Params, blob: &[u8], offsets: &[u64], amounts: &[Scalar], mut rng: impl CryptoRngCore)
        -> Vec<Result<Vec<u8>, WireError>> {
        assert!(!offsets.is_empty() && *offsets.last().unwrap() as usize <= blob.len());
        let n = offsets.len() - 1;
        assert_eq!(amounts.len(), n);
        let mut cb = Vec::with_capacity(32 * n + 1);
        for c in amounts {
            put_s(&mut cb, c);
        }
        cb.push(0);
        let sk = self.record();
        let gpu = params.gpu();
        let src = rng_source(&mut rng);
        let (mut out, mut status) = (vec![0u8; ISSUANCE_RESPONSE_CBOR_BYTES * n + 1], vec![0u8; n + 1]);
        gpu.check(unsafe {
            act_node_issue_cbor_batch(gpu.0, n, sk.as_ptr(), blob.as_ptr(), offsets.as_ptr(), cb.as_ptr(), &src as *const ActRngSource as *const u8,
                                      ACT_RNG_CALLBACK, out.as_mut_ptr(), status.as_mut_ptr())
        });
        issuance_messages(&out, &status[..n])
    }
    /// Verdicts only (`refund` up to the challenge check, src/lib.rs:787-844) for CBOR `SpendProof` messages.
    pub fn verify_spend_cbor_batch(&self, params: &Params, msgs: &[&[u8]]) -> Vec<Result<(), WireError>> {
        let (blob, offsets) = gather(msgs);
        let n = msgs.len();
        let sk = self.record();
        let gpu = params.gpu();
        let mut status = vec![0u8; n + 1];
        gpu.check(unsafe { act_node_verify_spend_cbor_batch(gpu.0, n, sk.as_ptr(), blob.as_ptr(), offsets.as_ptr(), status.as_mut_ptr(), std::ptr::null_mut()) });
        status[..n].iter().map(|&s| if s == 0 { Ok(()) } else { Err(status_to_wire_error(s)) }).collect()
    }
}

// ---- the redemption step (examples/act.rs:62-73) ------------------------------------------------------------------------------
/// The double-spend database the crate leaves to the caller (src/lib.rs:741-745; `HashSet<Scalar>` in src/tests.rs:29-50 and
/// examples/act.rs:10-30) as a hash set in the HBM of the node's GPUs: one set per GPU, a nullifier owned by exactly one of them.
pub struct GpuNullifierStore(*mut ActNodeNullifierSet);
// SAFETY: every entry point that takes the set locks it (csrc/node.cpp act_node_nullifier_check_and_insert_batch); destroy runs from Drop.
unsafe impl Send for GpuNullifierStore {}
unsafe impl Sync for GpuNullifierStore {}
impl Drop for GpuNullifierStore {
    fn drop(&mut self) {
        unsafe { act_node_nullifier_set_destroy(self.0) }
    }
}
impl GpuNullifierStore {
    /// `capacity_per_device`: nullifiers each GPU's share must be able to hold (32 bytes + 4 per slot, load factor 1/2).
    pub fn new(capacity_per_device: usize) -> Self {
        let devices = devices_from_env();
        let mut set = std::ptr::null_mut();
        // salt = null: the routing and slot hashes are keyed with 16 bytes from the OS -- clients choose their nullifiers
        let rc = unsafe { act_node_nullifier_set_create(devices.as_ptr(), devices.len() as c_int, capacity_per_device, std::ptr::null(), &mut set) };
        if rc != 0 {
            let msg = if set.is_null() { String::new() } else { unsafe { CStr::from_ptr(act_node_nullifier_set_last_error(set)) }.to_string_lossy().into_owned() };
            panic!("act_node_nullifier_set_create failed ({rc}): {msg}");
        }
        GpuNullifierStore(set)
    }
    pub fn len(&self) -> usize {
        unsafe { act_node_nullifier_set_len(self.0) }
    }
    pub fn is_empty(&self) -> bool {
        self.len() == 0
    }
    fn check(&self, rc: c_int) -> Result<(), String> {
        if rc == 0 { Ok(()) } else { Err(format!("nullifier store ({rc}): {}", unsafe { CStr::from_ptr(act_node_nullifier_set_last_error(self.0)) }.to_string_lossy())) }
    }
    /// Grow every GPU's share so that `capacity_per_device` nullifiers fit; recorded ones are rehashed on the GPU, never lost.
    pub fn reserve(&self, capacity_per_device: usize) -> Result<(), String> {
        self.check(unsafe { act_node_nullifier_set_reserve(self.0, capacity_per_device) })
    }
    /// How many nullifiers are recorded under `epoch` (the caller's name for an issuer key; `Keyring::with_epochs`).
    pub fn epoch_len(&self, epoch: u32) -> Result<u64, String> {
        let mut count = 0u64;
        self.check(unsafe { act_node_nullifier_set_epoch_len(self.0, epoch, &mut count) })?;
        Ok(count)
    }
    /// Remove every nullifier recorded under `epoch` and refuse the epoch from then on; returns how many were removed.  ONLY once the
    /// epoch's key has been removed from every ring of every server that shares this store and will never be put back: from then on no
    /// proof under that key verifies, so its nullifiers are never consulted again; retiring earlier re-enables double spends of that
    /// key's tokens.  GPU after GPU: after an error some have retired, every set is valid, and a repeat of the call finishes the job.
    pub fn retire_epoch(&self, epoch: u32) -> Result<u64, String> {
        let mut removed = 0u64;
        self.check(unsafe { act_node_nullifier_set_retire_epoch(self.0, epoch, &mut removed) })?;
        Ok(removed)
    }
    /// Read-only: is each nullifier recorded?  For audit and status queries -- a spend decision is `redeem_*_batch`, which records.
    pub fn contains(&self, nullifiers: &[Scalar]) -> Result<Vec<bool>, String> {
        let keys: Vec<u8> = nullifiers.iter().flat_map(|k| k.to_bytes()).collect();
        let mut found = vec![0u8; nullifiers.len() + 1];
        self.check(unsafe { act_node_nullifier_contains_batch(self.0, nullifiers.len(), keys.as_ptr(), 32, found.as_mut_ptr()) })?;
        Ok(found[..nullifiers.len()].iter().map(|&f| f != 0).collect())
    }
    /// Every recorded nullifier, reduced, in unspecified order.
    fn export(&self) -> Result<Vec<[u8; 32]>, String> {
        const MAX: usize = 1 << 20;
        let (mut cursor, mut keys, mut buf) = (0u64, Vec::new(), vec![0u8; 32 * MAX]);
        while cursor != u64::MAX {
            let mut got = 0usize;
            self.check(unsafe { act_node_nullifier_set_export(self.0, &mut cursor, MAX, buf.as_mut_ptr(), &mut got) })?;
            keys.extend(buf[..32 * got].chunks_exact(32).map(|c| <[u8; 32]>::try_from(c).unwrap()));
        }
        Ok(keys)
    }
    /// Snapshot v1 (anonymous-credit-tokens_amd/nullifier_snapshot.py; encoding: `snapshot_encode`).  A point-in-time copy: log
    /// what is recorded after it ("restart and growth").
    pub fn save(&self, path: &std::path::Path) -> std::io::Result<usize> {
        let keys = self.export().map_err(std::io::Error::other)?;
        let data = snapshot_encode(keys);
        let tmp = path.with_extension("tmp");
        std::fs::write(&tmp, &data)?;
        std::fs::rename(&tmp, path)?;
        Ok((data.len() - 48) / 32)
    }
    /// A new store (devices from ACT_MI355X_DEVICES) holding a snapshot's keys; the file is validated as a whole before anything
    /// is inserted.  Every device is reserved for its expected share (owners are a keyed hash); a device that still runs full is
    /// grown and only its lanes -- refused, not recorded -- are resubmitted.
    pub fn restore(path: &std::path::Path, capacity_per_device: usize) -> std::io::Result<Self> {
        let data = std::fs::read(path)?;
        let body = snapshot_decode(&data).map_err(|m| std::io::Error::new(std::io::ErrorKind::InvalidData, format!("nullifier snapshot: {m}")))?;
        let per = (body.len() / 32).div_ceil(devices_from_env().len().max(1));
        let mut cap = capacity_per_device.max(per + per / 8 + 4 * per.isqrt() + 1024);
        let store = GpuNullifierStore::new(cap);
        for chunk in body.chunks(32 << 20) {
            let mut lanes = chunk.to_vec();
            loop {
                let m = lanes.len() / 32;
                let mut spent = vec![0u8; m + 1];
                let rc = unsafe { act_node_nullifier_check_and_insert_batch(store.0, m, lanes.as_ptr(), 32, std::ptr::null(), spent.as_mut_ptr()) };
                if rc == 0 { break; }
                // ACT_NULLIFIER_UNDETERMINED (2): the lanes of a device that refused its bucket; every other lane is final
                let left: Vec<u8> = lanes.chunks_exact(32).zip(&spent[..m]).filter(|(_, s)| **s == 2).flat_map(|(k, _)| k.iter().copied()).collect();
                if rc != 1 || left.is_empty() || cap >= 1 << 30 { store.check(rc).map_err(std::io::Error::other)?; }
                cap = (2 * cap).min(1 << 30);
                store.reserve(cap).map_err(std::io::Error::other)?;
                lanes = left;
            }
        }
        Ok(store)
    }
}

/// Snapshot v1: "ACTNULS1", count u64 LE, the keys reduced mod l, de-duplicated and strictly ascending (memcmp), SHA-256 of all
/// bytes before it -- byte for byte what nullifier_snapshot.py writes (`snapshot_tests` pins the same fixture as the Python test).
fn snapshot_encode(mut keys: Vec<[u8; 32]>) -> Vec<u8> {
    for k in keys.iter_mut() { *k = Scalar::from_bytes_mod_order(*k).to_bytes(); }
    keys.sort_unstable();
    keys.dedup();
    let mut data = b"ACTNULS1".to_vec();
    data.extend_from_slice(&(keys.len() as u64).to_le_bytes());
    for k in &keys { data.extend_from_slice(k); }
    let digest = sha256(&data);
    data.extend_from_slice(&digest);
    data
}
/// The keys of an intact v1 snapshot (n*32 bytes), or what is wrong with it: magic, length vs count, checksum, a key not
/// reduced, keys out of order or repeated.
fn snapshot_decode(data: &[u8]) -> Result<&[u8], &'static str> {
    if data.len() < 48 || &data[..8] != b"ACTNULS1" { return Err("bad magic"); }
    let n = u64::from_le_bytes(data[8..16].try_into().unwrap()) as usize;
    if n > (data.len() - 48) / 32 || data.len() != 48 + 32 * n { return Err("length disagrees with count"); }
    if sha256(&data[..16 + 32 * n])[..] != data[16 + 32 * n..] { return Err("checksum mismatch"); }
    let body = &data[16..16 + 32 * n];
    for (i, k) in body.chunks_exact(32).enumerate() {
        if bool::from(Scalar::from_canonical_bytes(<[u8; 32]>::try_from(k).unwrap()).is_none()) { return Err("key not reduced"); }
        if i > 0 && body[32 * (i - 1)..32 * i] >= *k { return Err("keys out of order or repeated"); }
    }
    Ok(body)
}

/// SHA-256 (FIPS 180-4) for the snapshot checksum; the crate has no SHA-2 dependency to lean on.
fn sha256(msg: &[u8]) -> [u8; 32] {
    const K: [u32; 64] = [
        0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3,
        0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
        0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13,
        0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
        0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
        0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2,
    ];
    let mut h: [u32; 8] = [0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19];
    let mut m = msg.to_vec();
    m.push(0x80);
    while m.len() % 64 != 56 { m.push(0); }
    m.extend_from_slice(&((msg.len() as u64) * 8).to_be_bytes());
    for block in m.chunks_exact(64) {
        let mut w = [0u32; 64];
        for t in 0..16 { w[t] = u32::from_be_bytes(block[4 * t..4 * t + 4].try_into().unwrap()); }
        for t in 16..64 {
            let s0 = w[t - 15].rotate_right(7) ^ w[t - 15].rotate_right(18) ^ (w[t - 15] >> 3);
            let s1 = w[t - 2].rotate_right(17) ^ w[t - 2].rotate_right(19) ^ (w[t - 2] >> 10);
            w[t] = w[t - 16].wrapping_add(s0).wrapping_add(w[t - 7]).wrapping_add(s1);
        }
        let [mut a, mut b, mut c, mut d, mut e, mut f, mut g, mut hh] = h;
        for t in 0..64 {
            let t1 = hh.wrapping_add(e.rotate_right(6) ^ e.rotate_right(11) ^ e.rotate_right(25)).wrapping_add((e & f) ^ (!e & g)).wrapping_add(K[t]).wrapping_add(w[t]);
            let t2 = (a.rotate_right(2) ^ a.rotate_right(13) ^ a.rotate_right(22)).wrapping_add((a & b) ^ (a & c) ^ (b & c));
            hh = g; g = f; f = e; e = d.wrapping_add(t1); d = c; c = b; b = a; a = t1.wrapping_add(t2);
        }
        for (x, y) in h.iter_mut().zip([a, b, c, d, e, f, g, hh]) { *x = x.wrapping_add(y); }
    }
    let mut out = [0u8; 32];
    for i in 0..8 { out[4 * i..4 * i + 4].copy_from_slice(&h[i].to_be_bytes()); }
    out
}

#[cfg(test)]
mod snapshot_tests {
    use super::*;
    fn hex(b: &[u8]) -> String { b.iter().map(|x| format!("{x:02x}")).collect() }
    #[test]
    fn sha256_fips_vectors() {
        assert_eq!(hex(&sha256(b"abc")), "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad");
        assert_eq!(hex(&sha256(b"")), "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855");
    }
    /// tests/test_nullifier_snapshot.py::test_v1_encoding_is_pinned: 0, 1, 5, 7, 5, l - 1, l, l + 5, 2^256 - 1, 2^200 + 3, 2^252 + 9
    #[test]
    fn encoding_matches_the_python_pin() {
        let small = |v: u8| { let mut k = [0u8; 32]; k[0] = v; k };
        let l: [u8; 32] = [0xed, 0xd3, 0xf5, 0x5c, 0x1a, 0x63, 0x12, 0x58, 0xd6, 0x9c, 0xf7, 0xa2, 0xde, 0xf9, 0xde, 0x14,
                           0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0x10];
        let (mut lm1, mut lp5, mut b200, mut b252) = (l, l, small(3), small(9));
        lm1[0] = 0xec; lp5[0] = 0xf2; b200[25] = 1; b252[31] = 0x10;
        let keys = vec![small(0), small(1), small(5), small(7), small(5), lm1, l, lp5, [0xff; 32], b200, b252];
        let data = snapshot_encode(keys);
        assert_eq!(hex(&sha256(&data)), "129f170cc9b90d9d880917cc1b6a25ffa7ebadb8ba5bb4959fce212087707eef");
        assert_eq!(snapshot_decode(&data).unwrap().len(), 32 * 8);
        let mut bad = data.clone(); *bad.last_mut().unwrap() ^= 1;
        assert_eq!(snapshot_decode(&bad), Err("checksum mismatch"));
        assert_eq!(snapshot_decode(&data[..data.len() - 1]), Err("length disagrees with count"));
    }
}

/// Outcome of a redeem call.  `engine_failure` is set when a GPU or the store failed AFTER verification: every lane still has its
/// decision (`WireError::NullifierUndetermined` / `RecordedUnsigned` name the lanes that were left over) -- nothing is lost, nothing
/// may be blindly resubmitted (include/act_mi355x.h, act_redeem_batch).
pub struct Redeemed<T> {
    pub lanes: Vec<Result<T, WireError>>,
    pub engine_failure: Option<String>,
}

impl PrivateKey {
    /// The server loop of examples/act.rs:62-73 over a batch of wire messages --
    ///     from_cbor -> refund's checks -> `if store.is_used(k) { DoubleSpendError } else { store.mark_used(k) }` -> sign -> to_cbor
    /// -- with the meaning of that loop run in lane order (a nullifier repeated inside the batch is a double spend from its second
    /// occurrence on; a proof that does not verify cannot burn a nullifier) and `rng` drawn for exactly the lanes that are signed.
    pub fn redeem_cbor_batch(&self, params: &Params, store: &GpuNullifierStore, msgs: &[&[u8]], mut rng: impl CryptoRngCore) -> Redeemed<Vec<u8>> {
        let (blob, offsets) = gather(msgs);
        let n = msgs.len();
        let sk = self.record();
        let gpu = params.gpu();
        let src = rng_source(&mut rng);
        let (mut out, mut status) = (vec![0u8; REFUND_CBOR_BYTES * n + 1], vec![0u8; n + 1]);
        let rc = unsafe {
            act_node_redeem_cbor_batch(gpu.0, store.0, n, sk.as_ptr(), blob.as_ptr(), offsets.as_ptr(), &src as *const ActRngSource as *const u8,
                                       ACT_RNG_CALLBACK, out.as_mut_ptr(), status.as_mut_ptr())
        };
        let engine_failure = if rc != 0 { Some(unsafe { CStr::from_ptr(act_node_last_error(gpu.0)) }.to_string_lossy().into_owned()) } else { None };
        Redeemed { lanes: refund_messages(&out, &status[..n]), engine_failure }
    }
    /// The same over `SpendProof`s (marshalled on all cores: 130 `compress()` per proof).
    pub fn redeem_batch(&self, params: &Params, store: &GpuNullifierStore, proofs: &[SpendProof], mut rng: impl CryptoRngCore) -> Redeemed<Refund> {
        let n = proofs.len();
        let rec = marshal(proofs, PROOF_BYTES, |p, out| p.write_record(out));
        let sk = self.record();
        let gpu = params.gpu();
        let src = rng_source(&mut rng);
        let (mut out, mut status) = (vec![0u8; 128 * n + 1], vec![0u8; n + 1]);
        let rc = unsafe {
            act_node_redeem_batch(gpu.0, store.0, n, sk.as_ptr(), rec.as_ptr(), &src as *const ActRngSource as *const u8, ACT_RNG_CALLBACK,
                                  out.as_mut_ptr(), status.as_mut_ptr())
        };
        let engine_failure = if rc != 0 { Some(unsafe { CStr::from_ptr(act_node_last_error(gpu.0)) }.to_string_lossy().into_owned()) } else { None };
        let lanes = (0..n).map(|i| if status[i] == 0 { Ok(Refund::from_record(&out[128 * i..128 * i + 128])) } else { Err(status_to_wire_error(status[i])) }).collect();
        Redeemed { lanes, engine_failure }
    }
}

/// Key rotation: an ordered ring of up to four issuer keys (the caller's order of preference) that one batch is redeemed against.
/// A `SpendProof` names no key: every proof is verified once, `matched[i]` says which ring key lane i verified under (`None` where
/// no ring key accepts it; a double spend keeps the index it matched), and the refund is signed with the matched key
/// (`sign_with = None`) or with ring key `sign_with = Some(i)` -- which moves the client onto that key with its next token (the
/// client then calls `to_credit_token` with `ring.public(i)`).  The nullifier store is shared by all keys; `Params` must be the
/// ones every ring key issued under.  With epochs (`with_epochs`: one `u32` up to 2^24 - 1 per key, the caller's stable name for it) an
/// accepted nullifier is recorded under the epoch of the key its proof matched, so that `GpuNullifierStore::retire_epoch` can drop a
/// key's nullifiers once the key has left every ring for good.
pub struct Keyring<'a>(pub &'a [PrivateKey], pub Option<&'a [u32]>);
pub const ACT_KEYRING_MAX: usize = 4;
const ACT_KEY_NONE: u8 = 255;
const ACT_SIGN_MATCHED: c_int = -1;
/// `lanes` as `Redeemed`, plus the ring index per lane.
pub struct RingRedeemed<T> {
    pub redeemed: Redeemed<T>,
    pub matched: Vec<Option<usize>>,
}

impl<'a> Keyring<'a> {
    pub fn new(keys: &'a [PrivateKey]) -> Self {
        Keyring(keys, None)
    }
    pub fn with_epochs(keys: &'a [PrivateKey], epochs: &'a [u32]) -> Self {
        assert!(keys.len() == epochs.len(), "one epoch per ring key");
        Keyring(keys, Some(epochs))
    }
    pub fn public(&self, i: usize) -> &PublicKey {
        self.0[i].public()
    }
    fn records(&self) -> Vec<u8> {
        assert!(!self.0.is_empty() && self.0.len() <= ACT_KEYRING_MAX, "a key ring holds 1 ..= ACT_KEYRING_MAX keys");
        self.0.iter().flat_map(|k| k.record().to_vec()).collect()
    }
    fn sign_key(&self, sign_with: Option<usize>) -> c_int {
        match sign_with {
            None => ACT_SIGN_MATCHED,
            Some(i) => { assert!(i < self.0.len(), "sign_with is not a ring index"); i as c_int }
        }
    }
    fn matched(out_key: &[u8]) -> Vec<Option<usize>> {
        out_key.iter().map(|&k| if k == ACT_KEY_NONE { None } else { Some(k as usize) }).collect()
    }
    /// `PrivateKey::redeem_cbor_batch` against the ring.
    pub fn redeem_cbor_batch(&self, params: &Params, store: &GpuNullifierStore, msgs: &[&[u8]], sign_with: Option<usize>, mut rng: impl CryptoRngCore)
        -> RingRedeemed<Vec<u8>> {
        let (blob, offsets) = gather(msgs);
        let n = msgs.len();
        let (keys, sign_key) = (self.records(), self.sign_key(sign_with));
        let gpu = params.gpu();
        let src = rng_source(&mut rng);
        let (mut out, mut status, mut out_key) = (vec![0u8; REFUND_CBOR_BYTES * n + 1], vec![0u8; n + 1], vec![ACT_KEY_NONE; n + 1]);
        let rc = unsafe {
            match self.1 {
                Some(ep) => act_node_redeem_cbor_keyring_epochs_batch(gpu.0, store.0, n, keys.as_ptr(), self.0.len() as c_int, ep.as_ptr(), sign_key, blob.as_ptr(),
                                                                      offsets.as_ptr(), &src as *const ActRngSource as *const u8, ACT_RNG_CALLBACK, out.as_mut_ptr(),
                                                                      status.as_mut_ptr(), out_key.as_mut_ptr()),
                None => act_node_redeem_cbor_keyring_batch(gpu.0, store.0, n, keys.as_ptr(), self.0.len() as c_int, sign_key, blob.as_ptr(), offsets.as_ptr(),
                                                           &src as *const ActRngSource as *const u8, ACT_RNG_CALLBACK, out.as_mut_ptr(), status.as_mut_ptr(), out_key.as_mut_ptr()),
            }
        };
        let engine_failure = if rc != 0 { Some(unsafe { CStr::from_ptr(act_node_last_error(gpu.0)) }.to_string_lossy().into_owned()) } else { None };
        RingRedeemed { redeemed: Redeemed { lanes: refund_messages(&out, &status[..n]), engine_failure }, matched: Self::matched(&out_key[..n]) }
    }
    /// `PrivateKey::redeem_batch` against the ring.
    pub fn redeem_batch(&self, params: &Params, store: &GpuNullifierStore, proofs: &[SpendProof], sign_with: Option<usize>, mut rng: impl CryptoRngCore)
        -> RingRedeemed<Refund> {
        let n = proofs.len();
        let rec = marshal(proofs, PROOF_BYTES, |p, out| p.write_record(out));
        let (keys, sign_key) = (self.records(), self.sign_key(sign_with));
        let gpu = params.gpu();
        let src = rng_source(&mut rng);
        let (mut out, mut status, mut out_key) = (vec![0u8; 128 * n + 1], vec![0u8; n + 1], vec![ACT_KEY_NONE; n + 1]);
        let rc = unsafe {
            match self.1 {
                Some(ep) => act_node_redeem_keyring_epochs_batch(gpu.0, store.0, n, keys.as_ptr(), self.0.len() as c_int, ep.as_ptr(), sign_key, rec.as_ptr(),
                                                                 &src as *const ActRngSource as *const u8, ACT_RNG_CALLBACK, out.as_mut_ptr(), status.as_mut_ptr(),
                                                                 out_key.as_mut_ptr()),
                None => act_node_redeem_keyring_batch(gpu.0, store.0, n, keys.as_ptr(), self.0.len() as c_int, sign_key, rec.as_ptr(), &src as *const ActRngSource as *const u8,
                                                      ACT_RNG_CALLBACK, out.as_mut_ptr(), status.as_mut_ptr(), out_key.as_mut_ptr()),
            }
        };
        let engine_failure = if rc != 0 { Some(unsafe { CStr::from_ptr(act_node_last_error(gpu.0)) }.to_string_lossy().into_owned()) } else { None };
        let lanes = (0..n).map(|i| if status[i] == 0 { Ok(Refund::from_record(&out[128 * i..128 * i + 128])) } else { Err(status_to_wire_error(status[i])) }).collect();
        RingRedeemed { redeemed: Redeemed { lanes, engine_failure }, matched: Self::matched(&out_key[..n]) }
    }
}

/// `ACT_STATUS_WRONG_CHARGE`: the admission calls only -- `s` is not the expected charge; not verified, not recorded, not signed.
pub const ACT_STATUS_WRONG_CHARGE: u8 = 250;
pub const ACT_ADMIT_COUNTS: usize = 8;
pub const ACT_ADMIT_UNIQUE_COUNTS: usize = 9;
/// statuses, outputs (128-byte Refund records or `REFUND_CBOR_BYTES` messages, all zero where not signed), matched ring keys, and
/// lanes / wire_rejected / wrong_charge / spent_before / verified / rejected_by_verification / double_spend_after / accepted
pub struct Admitted {
    pub rc: c_int,
    pub status: Vec<u8>,
    pub out: Vec<u8>,
    pub out_key: Vec<u8>,
    pub counts: [u64; ACT_ADMIT_COUNTS],
    /// the unique forms only: lanes with the bytes of an earlier lane of the batch, answered from that lane without being verified
    /// (`counts[4]`, verified, is smaller by exactly this)
    pub copies: u64,
}
/// Admission before verification on ONE GPU (include/act_mi355x.h "admission before verification"): the ring redeem calls with a screen
/// in front -- a proof whose charge `s` is not the expected one is answered `ACT_STATUS_WRONG_CHARGE` and a proof whose nullifier the
/// set already holds `DoubleSpendError`, both WITHOUT being verified.  Thin: bytes in, bytes out, the statuses as the header lists them.
/// The node-level forms do not exist yet; node callers compose `act_node_nullifier_contains_batch` in front of their redeem call.
pub struct GpuAdmission {
    ctx: *mut ActCtx,
    set: *mut ActNullifierSet,
    unique: bool,
}
impl GpuAdmission {
    /// # Safety
    /// `ctx` and `set` are live handles on one device (`act_ctx_create` / `act_node_ctx`, `act_nullifier_set_create`) and outlive `self`.
    pub unsafe fn from_raw(ctx: *mut ActCtx, set: *mut ActNullifierSet) -> Self {
        GpuAdmission { ctx, set, unique: false }
    }
    /// `true`: the calls go to `act_redeem_admit_unique_batch` / `act_redeem_cbor_admit_unique_batch` -- byte-identical proofs of one
    /// batch are verified once.  Statuses, `out_key`, output bytes, what is recorded and what is drawn stay the same; `copies` is filled.
    pub fn unique(mut self, on: bool) -> Self {
        self.unique = on;
        self
    }
    /// `keys`: nkeys records of 64 bytes; `proofs`: n records of `PROOF_BYTES`; `charges`: n scalars of 32 bytes, or None.
    pub fn redeem_admit_batch(&self, keys: &[u8], key_epochs: Option<&[u32]>, sign_with: Option<usize>, proofs: &[u8], charges: Option<&[u8]>,
                              mut rng: impl CryptoRngCore) -> Admitted {
        let (n, nkeys) = (proofs.len() / PROOF_BYTES, keys.len() / 64);
        assert!(proofs.len() == n * PROOF_BYTES && charges.map_or(true, |c| c.len() == 32 * n) && key_epochs.map_or(true, |e| e.len() == nkeys));
        let src = rng_source(&mut rng);
        let mut r = Admitted { rc: 0, status: vec![0u8; n + 1], out: vec![0u8; 128 * n + 1], out_key: vec![ACT_KEY_NONE; n + 1], counts: [0; ACT_ADMIT_COUNTS], copies: 0 };
        let mut counts = [0u64; ACT_ADMIT_UNIQUE_COUNTS];
        let call = if self.unique { act_redeem_admit_unique_batch } else { act_redeem_admit_batch };
        r.rc = unsafe {
            call(self.ctx, self.set, n, 0, keys.as_ptr(), nkeys as c_int, key_epochs.map_or(std::ptr::null(), |e| e.as_ptr()),
                                   sign_with.map_or(ACT_SIGN_MATCHED, |i| i as c_int), proofs.as_ptr(), charges.map_or(std::ptr::null(), |c| c.as_ptr()),
                                   &src as *const ActRngSource as *const u8, ACT_RNG_CALLBACK, r.out.as_mut_ptr(), r.status.as_mut_ptr(), r.out_key.as_mut_ptr(),
                                   counts.as_mut_ptr())
        };
        r.counts.copy_from_slice(&counts[..ACT_ADMIT_COUNTS]); r.copies = counts[ACT_ADMIT_COUNTS];
        r.status.truncate(n); r.out.truncate(128 * n); r.out_key.truncate(n);
        r
    }
    /// The same on wire bytes: CBOR SpendProof messages in, CBOR Refund messages out.
    pub fn redeem_cbor_admit_batch(&self, keys: &[u8], key_epochs: Option<&[u32]>, sign_with: Option<usize>, msgs: &[&[u8]], charges: Option<&[u8]>,
                                   mut rng: impl CryptoRngCore) -> Admitted {
        let (blob, offsets) = gather(msgs);
        let (n, nkeys) = (msgs.len(), keys.len() / 64);
        assert!(charges.map_or(true, |c| c.len() == 32 * n) && key_epochs.map_or(true, |e| e.len() == nkeys));
        let src = rng_source(&mut rng);
        let mut r = Admitted { rc: 0, status: vec![0u8; n + 1], out: vec![0u8; REFUND_CBOR_BYTES * n + 1], out_key: vec![ACT_KEY_NONE; n + 1], counts: [0; ACT_ADMIT_COUNTS], copies: 0 };
        let mut counts = [0u64; ACT_ADMIT_UNIQUE_COUNTS];
        let call = if self.unique { act_redeem_cbor_admit_unique_batch } else { act_redeem_cbor_admit_batch };
        r.rc = unsafe {
            call(self.ctx, self.set, n, 0, keys.as_ptr(), nkeys as c_int, key_epochs.map_or(std::ptr::null(), |e| e.as_ptr()),
                                        sign_with.map_or(ACT_SIGN_MATCHED, |i| i as c_int), blob.as_ptr(), offsets.as_ptr(),
                                        charges.map_or(std::ptr::null(), |c| c.as_ptr()), &src as *const ActRngSource as *const u8, ACT_RNG_CALLBACK,
                                        r.out.as_mut_ptr(), r.status.as_mut_ptr(), r.out_key.as_mut_ptr(), counts.as_mut_ptr())
        };
        r.counts.copy_from_slice(&counts[..ACT_ADMIT_COUNTS]); r.copies = counts[ACT_ADMIT_COUNTS];
        r.status.truncate(n); r.out.truncate(REFUND_CBOR_BYTES * n); r.out_key.truncate(n);
        r
    }
}

/// `ACT_STATUS_RETURN_TOO_BIG`: the return calls only -- the returned amount `t` exceeds the charge `s`; not looked up, not verified,
/// not recorded, not signed.
pub const ACT_STATUS_RETURN_TOO_BIG: u8 = 249;
pub const ACT_REDEEM_RETURN_COUNTS: usize = 9;
/// the nine above, then copies (`GpuReturn::unique(true)`)
pub const ACT_REDEEM_RETURN_UNIQUE_COUNTS: usize = 10;
/// a RefundReturn on the wire (`ACT_CBOR_REFUND_RETURN`): the Refund map with a fifth entry, key 5 -> t
pub const REFUND_RETURN_CBOR_BYTES: usize = REFUND_CBOR_BYTES + 35;
/// statuses, outputs (160-byte RefundReturn records `A | e | gamma | z | t` or `REFUND_RETURN_CBOR_BYTES` messages, all zero where not
/// signed), matched ring keys, the eight admission counts, `return_too_big` and (`GpuReturn::unique(true)`; 0 otherwise) `copies`
pub struct Returned {
    pub rc: c_int,
    pub status: Vec<u8>,
    pub out: Vec<u8>,
    pub out_key: Vec<u8>,
    pub counts: [u64; ACT_ADMIT_COUNTS],
    pub return_too_big: u64,
    pub copies: u64,
}
/// Partial refunds on ONE GPU (include/act_mi355x.h "partial refunds"): the admission calls with the amounts `t <= s` the issuer gives
/// back -- every accepted lane is signed over `X_A = g + K' + t h1`, so the client's next token holds `c - s + t`.  A lane with
/// `t > s` is answered `ACT_STATUS_RETURN_TOO_BIG` without being looked up or verified.  A sibling of `GpuAdmission`, not a mode of
/// the replay types: drawn nonces here.  The retry-safe form is `GpuReplay::returned`, where `t` enters the receipt tag and the nonces.
pub struct GpuReturn {
    ctx: *mut ActCtx,
    set: *mut ActNullifierSet,
    unique: bool,
}
impl GpuReturn {
    /// # Safety
    /// `ctx` and `set` are live handles on one device and outlive `self`.
    pub unsafe fn from_raw(ctx: *mut ActCtx, set: *mut ActNullifierSet) -> Self {
        GpuReturn { ctx, set, unique: false }
    }
    /// `true`: the calls go to `act_redeem_return_unique_batch` / `act_redeem_cbor_return_unique_batch` -- a proof with the bytes of an
    /// earlier proof of the batch is not verified, whatever its `t`: the first one is signed over its own `t` and the others are double
    /// spends, as they are without this.  The same statuses, outputs and recorded nullifiers; `Returned::copies` counts them.
    pub fn unique(mut self, enabled: bool) -> Self {
        self.unique = enabled;
        self
    }
    /// `returned`: n scalars of 32 bytes (None: every t is 0); the other arguments as `GpuAdmission::redeem_admit_batch`.
    pub fn redeem_return_batch(&self, keys: &[u8], key_epochs: Option<&[u32]>, sign_with: Option<usize>, proofs: &[u8], charges: Option<&[u8]>,
                               returned: Option<&[u8]>, mut rng: impl CryptoRngCore) -> Returned {
        let (n, nkeys) = (proofs.len() / PROOF_BYTES, keys.len() / 64);
        assert!(proofs.len() == n * PROOF_BYTES && charges.map_or(true, |c| c.len() == 32 * n) && returned.map_or(true, |t| t.len() == 32 * n) &&
                key_epochs.map_or(true, |e| e.len() == nkeys));
        let src = rng_source(&mut rng);
        let mut r = Returned { rc: 0, status: vec![0u8; n + 1], out: vec![0u8; 160 * n + 1], out_key: vec![ACT_KEY_NONE; n + 1], counts: [0; ACT_ADMIT_COUNTS], return_too_big: 0, copies: 0 };
        let mut counts = [0u64; ACT_REDEEM_RETURN_UNIQUE_COUNTS];
        let call = if self.unique { act_redeem_return_unique_batch } else { act_redeem_return_batch };
        r.rc = unsafe {
            call(self.ctx, self.set, n, 0, keys.as_ptr(), nkeys as c_int, key_epochs.map_or(std::ptr::null(), |e| e.as_ptr()),
                 sign_with.map_or(ACT_SIGN_MATCHED, |i| i as c_int), proofs.as_ptr(), charges.map_or(std::ptr::null(), |c| c.as_ptr()),
                 returned.map_or(std::ptr::null(), |t| t.as_ptr()), &src as *const ActRngSource as *const u8, ACT_RNG_CALLBACK,
                 r.out.as_mut_ptr(), r.status.as_mut_ptr(), r.out_key.as_mut_ptr(), counts.as_mut_ptr())
        };
        r.counts.copy_from_slice(&counts[..ACT_ADMIT_COUNTS]); r.return_too_big = counts[ACT_ADMIT_COUNTS]; r.copies = counts[ACT_REDEEM_RETURN_COUNTS];
        r.status.truncate(n); r.out.truncate(160 * n); r.out_key.truncate(n);
        r
    }
    /// The same on wire bytes: CBOR SpendProof messages in, CBOR RefundReturn messages out.
    pub fn redeem_cbor_return_batch(&self, keys: &[u8], key_epochs: Option<&[u32]>, sign_with: Option<usize>, msgs: &[&[u8]], charges: Option<&[u8]>,
                                    returned: Option<&[u8]>, mut rng: impl CryptoRngCore) -> Returned {
        let (blob, offsets) = gather(msgs);
        let (n, nkeys) = (msgs.len(), keys.len() / 64);
        assert!(charges.map_or(true, |c| c.len() == 32 * n) && returned.map_or(true, |t| t.len() == 32 * n) && key_epochs.map_or(true, |e| e.len() == nkeys));
        let src = rng_source(&mut rng);
        let mut r = Returned { rc: 0, status: vec![0u8; n + 1], out: vec![0u8; REFUND_RETURN_CBOR_BYTES * n + 1], out_key: vec![ACT_KEY_NONE; n + 1], counts: [0; ACT_ADMIT_COUNTS], return_too_big: 0, copies: 0 };
        let mut counts = [0u64; ACT_REDEEM_RETURN_UNIQUE_COUNTS];
        let call = if self.unique { act_redeem_cbor_return_unique_batch } else { act_redeem_cbor_return_batch };
        r.rc = unsafe {
            call(self.ctx, self.set, n, 0, keys.as_ptr(), nkeys as c_int, key_epochs.map_or(std::ptr::null(), |e| e.as_ptr()),
                 sign_with.map_or(ACT_SIGN_MATCHED, |i| i as c_int), blob.as_ptr(), offsets.as_ptr(),
                 charges.map_or(std::ptr::null(), |c| c.as_ptr()), returned.map_or(std::ptr::null(), |t| t.as_ptr()),
                 &src as *const ActRngSource as *const u8, ACT_RNG_CALLBACK, r.out.as_mut_ptr(), r.status.as_mut_ptr(),
                 r.out_key.as_mut_ptr(), counts.as_mut_ptr())
        };
        r.counts.copy_from_slice(&counts[..ACT_ADMIT_COUNTS]); r.return_too_big = counts[ACT_ADMIT_COUNTS]; r.copies = counts[ACT_REDEEM_RETURN_COUNTS];
        r.status.truncate(n); r.out.truncate(REFUND_RETURN_CBOR_BYTES * n); r.out_key.truncate(n);
        r
    }
    /// The sign-only call: `kprime` and `status_in` as `act_verify_spend_keyring_batch` left them.  It does not see `s`: the CALLER
    /// bounds `returned[i] <= s_i`.  -> (rc, statuses, 160-byte records)
    pub fn refund_sign_return(&self, keys: &[u8], key_index: &[u8], kprime: &[u8], status_in: &[u8], returned: Option<&[u8]>, rng_slices: &[u8]) -> (c_int, Vec<u8>, Vec<u8>) {
        let n = status_in.len();
        assert!(key_index.len() == n && kprime.len() == 32 * n && returned.map_or(true, |t| t.len() == 32 * n));
        let (mut status, mut out) = (vec![0u8; n + 1], vec![0u8; 160 * n + 1]);
        let rc = unsafe {
            act_refund_sign_return_keyring_batch(self.ctx, n, 0, keys.as_ptr(), (keys.len() / 64) as c_int, key_index.as_ptr(), kprime.as_ptr(), status_in.as_ptr(),
                                                 rng_slices.as_ptr(), ACT_RNG_SEQUENTIAL, returned.map_or(std::ptr::null(), |t| t.as_ptr()), out.as_mut_ptr(),
                                                 status.as_mut_ptr())
        };
        status.truncate(n); out.truncate(160 * n);
        (rc, status, out)
    }
    /// The client's side: `PreRefund::to_credit_token` over RefundReturn records.  -> (rc, statuses, 160-byte CreditToken records whose
    /// balance is `m + t`); 4 = the proof over `g + K' + t h1` fails, 8 = a validly signed `t > s`.
    pub fn refund_to_credit_token_return(&self, prerefund: &[u8], proofs: &[u8], refund_return: &[u8], w: &[u8; 32]) -> (c_int, Vec<u8>, Vec<u8>) {
        let n = prerefund.len() / 96;
        assert!(prerefund.len() == 96 * n && proofs.len() == PROOF_BYTES * n && refund_return.len() == 160 * n);
        let (mut status, mut tokens) = (vec![0u8; n + 1], vec![0u8; 160 * n + 1]);
        let rc = unsafe {
            act_refund_to_credit_token_return_batch(self.ctx, n, 0, prerefund.as_ptr(), proofs.as_ptr(), refund_return.as_ptr(), w.as_ptr(), tokens.as_mut_ptr(),
                                                    status.as_mut_ptr())
        };
        status.truncate(n); tokens.truncate(160 * n);
        (rc, status, tokens)
    }
}

/// What the `PublicRing` calls return: statuses (those of the one-key call: 255 undecodable, 2 / 4 no ring key verifies), 160-byte
/// CreditToken records (all zero where rejected) and per lane the smallest ring index that verified (`ACT_KEY_NONE` where none did).
pub struct RingTokens {
    pub rc: c_int,
    pub status: Vec<u8>,
    pub tokens: Vec<u8>,
    pub out_key: Vec<u8>,
}
/// The client's side of key rotation on ONE GPU (include/act_mi355x.h "key rotation, the client's side"): `to_credit_token` against
/// the issuer's PUBLISHED keys, in the caller's order of preference.  Neither an `IssuanceResponse` nor a `Refund` names its key, and
/// a key identifier sent beside one would be a tag chosen by the server; here every item is verified once and an extra key costs
/// about 0.4 of one scalar multiplication.  Thin: bytes in, bytes out.
pub struct PublicRing {
    ctx: *mut ActCtx,
    ring_w: Vec<u8>,
}
impl PublicRing {
    /// # Safety
    /// `ctx` is a live handle (`act_ctx_create` / `act_node_ctx`) and outlives `self`.
    pub unsafe fn from_raw(ctx: *mut ActCtx, publics: &[PublicKey]) -> Self {
        assert!(!publics.is_empty() && publics.len() <= ACT_KEYRING_MAX, "a key ring holds 1 ..= ACT_KEYRING_MAX keys");
        let mut ring_w = Vec::with_capacity(32 * publics.len());
        for p in publics {
            ring_w.extend_from_slice(p.w.compress().as_bytes());
        }
        PublicRing { ctx, ring_w }
    }
    fn empty(n: usize) -> RingTokens {
        RingTokens { rc: 0, status: vec![0u8; n], tokens: vec![0u8; 160 * n], out_key: vec![ACT_KEY_NONE; n] }
    }
    /// `pre`: n records r | k (64 bytes); `req`: n IssuanceRequest records (128); `resp`: n IssuanceResponse records (160).
    pub fn issuance_to_credit_token_batch(&self, pre: &[u8], req: &[u8], resp: &[u8]) -> RingTokens {
        let n = pre.len() / 64;
        assert!(pre.len() == 64 * n && req.len() == 128 * n && resp.len() == 160 * n);
        let mut r = Self::empty(n);
        r.rc = unsafe {
            act_issuance_to_credit_token_keyring_batch(self.ctx, n, 0, pre.as_ptr(), self.ring_w.as_ptr(), (self.ring_w.len() / 32) as u32, req.as_ptr(),
                                                       resp.as_ptr(), r.tokens.as_mut_ptr(), r.status.as_mut_ptr(), r.out_key.as_mut_ptr())
        };
        r
    }
    /// `prerefund`: n records r | k | m (96 bytes); `proofs`: n SpendProof records (`PROOF_BYTES`); `refunds`: n Refund records (128).
    pub fn refund_to_credit_token_batch(&self, prerefund: &[u8], proofs: &[u8], refunds: &[u8]) -> RingTokens {
        let n = prerefund.len() / 96;
        assert!(prerefund.len() == 96 * n && proofs.len() == PROOF_BYTES * n && refunds.len() == 128 * n);
        let mut r = Self::empty(n);
        r.rc = unsafe {
            act_refund_to_credit_token_keyring_batch(self.ctx, n, 0, prerefund.as_ptr(), proofs.as_ptr(), refunds.as_ptr(), self.ring_w.as_ptr(),
                                                     (self.ring_w.len() / 32) as u32, r.tokens.as_mut_ptr(), r.status.as_mut_ptr(), r.out_key.as_mut_ptr())
        };
        r
    }
    /// The same over RefundReturn records (160 bytes, `A | e | gamma | z | t`): the tokens hold `m + t`; status 4 where no ring key's
    /// proof over `g + K' + t h1` holds, 8 for a `t > s` that a ring key validly signed.
    pub fn refund_return_to_credit_token(&self, prerefund: &[u8], proofs: &[u8], refund_returns: &[u8]) -> RingTokens {
        let n = prerefund.len() / 96;
        assert!(prerefund.len() == 96 * n && proofs.len() == PROOF_BYTES * n && refund_returns.len() == 160 * n);
        let mut r = Self::empty(n);
        r.rc = unsafe {
            act_refund_to_credit_token_return_keyring_batch(self.ctx, n, 0, prerefund.as_ptr(), proofs.as_ptr(), refund_returns.as_ptr(), self.ring_w.as_ptr(),
                                                            (self.ring_w.len() / 32) as u32, r.tokens.as_mut_ptr(), r.status.as_mut_ptr(), r.out_key.as_mut_ptr())
        };
        r
    }
}

pub const ACT_REPLAY_COUNTS: usize = 6;
/// lanes / wire_rejected / wrong_charge / foreign_spend / retry_candidates / verified / rejected_by_verification / fresh / replayed /
/// double_spend_after / unanswered (`GpuReplay::admit(true)`)
pub const ACT_ADMIT_REPLAY_COUNTS: usize = 11;
/// the eleven above, then copies / copies_served (`GpuReplay::unique(true)`)
pub const ACT_ADMIT_REPLAY_UNIQUE_COUNTS: usize = 13;
/// the eleven of `ACT_ADMIT_REPLAY_COUNTS`, then return_too_big (`GpuReplay::returned(Some(..))`)
pub const ACT_RETURN_REPLAY_COUNTS: usize = 12;
/// the twelve above, then copies / copies_served / copies_other_amount (`GpuReplay::returned(Some(..))` with `unique(true)`)
pub const ACT_RETURN_REPLAY_UNIQUE_COUNTS: usize = 15;
/// statuses, outputs (128-byte Refund records or `REFUND_CBOR_BYTES` messages, all zero where not signed), matched ring keys, the
/// replay marks, and lanes / rejected_by_verification / fresh / replayed / double_spend / unanswered
pub struct Replayed {
    pub rc: c_int,
    pub status: Vec<u8>,
    pub out: Vec<u8>,
    pub out_key: Vec<u8>,
    pub replayed: Vec<u8>,
    pub counts: [u64; ACT_REPLAY_COUNTS],
    /// all zero unless the call went through the admission screen (`GpuReplay::admit(true)`); then `counts` is its tail's view:
    /// lanes, rejected_by_verification, fresh, replayed, double_spend_after, unanswered
    pub admit_counts: [u64; ACT_ADMIT_REPLAY_COUNTS],
    /// all zero unless the call ran the unique form (`GpuReplay::unique(true)`): copies (lanes with the bytes of an earlier lane, not
    /// verified) and copies_served (those whose leader ended 0); `admit_counts` then counts verified lanes only
    pub copy_counts: [u64; 2],
    /// 0 unless the call took returned amounts (`GpuReplay::returned`): the lanes whose amount exceeded their charge.  `out` then holds
    /// 160-byte RefundReturn records or `REFUND_RETURN_CBOR_BYTES` messages
    pub return_too_big: u64,
    /// 0 unless the call took returned amounts AND ran the unique form: the copies that named another amount than their leader (behind
    /// an accepted leader they are `DoubleSpendError`: the receipt pins the leader's amount)
    pub copies_other_amount: u64,
}
impl Replayed {
    fn take_return_counts(&mut self, t: &[u64; ACT_RETURN_REPLAY_COUNTS]) {
        self.admit_counts.copy_from_slice(&t[..ACT_ADMIT_REPLAY_COUNTS]);
        self.return_too_big = t[ACT_ADMIT_REPLAY_COUNTS];
    }
    fn take_return_unique_counts(&mut self, v: &[u64; ACT_RETURN_REPLAY_UNIQUE_COUNTS]) {
        self.admit_counts.copy_from_slice(&v[..ACT_ADMIT_REPLAY_COUNTS]);
        self.return_too_big = v[ACT_ADMIT_REPLAY_COUNTS];
        self.copy_counts = [v[ACT_RETURN_REPLAY_COUNTS], v[ACT_RETURN_REPLAY_COUNTS + 1]];
        self.copies_other_amount = v[ACT_RETURN_REPLAY_COUNTS + 2];
    }
    fn take_unique_counts(&mut self, u: &[u64; ACT_ADMIT_REPLAY_UNIQUE_COUNTS]) {
        self.admit_counts.copy_from_slice(&u[..ACT_ADMIT_REPLAY_COUNTS]);
        self.copy_counts = [u[ACT_ADMIT_REPLAY_COUNTS], u[ACT_ADMIT_REPLAY_COUNTS + 1]];
    }
    fn take_admit_counts(&mut self) {
        let a = self.admit_counts;
        self.counts = [a[0], a[6], a[7], a[8], a[9], a[10]];
    }
}
/// Replayable redemption on ONE GPU (include/act_mi355x.h "replayable redemption"): the ring redeem calls without a generator -- the
/// nonces are derived from `nonce_key`, the signing key, the nullifier and K' -- and with a second set, the receipts, that records for
/// which K' a nullifier was spent.  A `SpendProof` that is sent again gets the same `Refund`, byte for byte, instead of
/// `DoubleSpendError`; another proof for the same nullifier is refused as before.  Retire an epoch on BOTH sets.  Thin: bytes in, bytes
/// out.  The node-level forms do not exist yet; node callers compose `derive` with their verify, set and sign calls.
pub struct GpuReplay {
    ctx: *mut ActCtx,
    set: *mut ActNullifierSet,
    receipts: *mut ActNullifierSet,
    nonce_key: [u8; 32],
    admit: bool,
    unique: bool,
    charges: Option<Vec<u8>>,
    returned: Option<Vec<u8>>,
    binds: Option<Vec<u8>>,
}
impl GpuReplay {
    /// # Safety
    /// `ctx`, `set` and `receipts` are live handles on one device, `set != receipts`, and all three outlive `self`.
    pub unsafe fn from_raw(ctx: *mut ActCtx, set: *mut ActNullifierSet, receipts: *mut ActNullifierSet, nonce_key: [u8; 32]) -> Self {
        GpuReplay { ctx, set, receipts, nonce_key, admit: false, unique: false, charges: None, returned: None, binds: None }
    }
    /// `true`: the calls go through the admission screen (include/act_mi355x.h "admission for the replayable redemption") -- a spent
    /// nullifier whose receipt is not this proof's is `DoubleSpendError` without being verified; a retry is verified and served.
    pub fn admit(mut self, on: bool) -> Self { self.admit = on; self }
    /// `true` (with `admit(true)`; nothing without it): the unique forms (include/act_mi355x.h "admission for the replayable redemption,
    /// unique forms") -- a lane with the bytes of an earlier lane of the batch is not verified and gets that lane's answer, its `Refund`
    /// included.  Statuses, outputs and both sets end as without it; `Replayed::copy_counts` says how many lanes were spared.
    pub fn unique(mut self, on: bool) -> Self { self.unique = on; self }
    /// What each request of the next calls costs: n scalars of 32 bytes, compared with `SpendProof.s` by the screen (implies nothing
    /// without `admit(true)`); `None`: no comparison.
    pub fn charges(mut self, charges: Option<Vec<u8>>) -> Self { self.charges = charges; self }
    /// The amounts the issuer gives back with the next calls (include/act_mi355x.h "replayable partial refunds"): n scalars of 32 bytes,
    /// `t <= s` per lane (`ACT_STATUS_RETURN_TOO_BIG` otherwise).  `Some`: the calls go to `act_redeem_(cbor_)return_replay_batch` -- the
    /// admission screen is implied, the outputs are RefundReturns, and the receipt PINS the amount: a retry with the same amount gets
    /// the same bytes, with another amount `DoubleSpendError`.  Derive the amount from the request, or remember it.  Together with
    /// `unique(true)` the calls go to `act_redeem_(cbor_)return_replay_unique_batch` ("replayable partial refunds, unique forms"): a
    /// lane with the bytes of an earlier lane is not verified whatever amount it names, and gets that lane's RefundReturn only if it
    /// names that lane's amount (`Replayed::copies_other_amount` counts the others).  `None`: the calls without amounts.
    pub fn returned(mut self, returned: Option<Vec<u8>>) -> Self { self.returned = returned; self }
    /// Request bindings for the next calls (include/act_mi355x.h "request binding"): n values of 32 bytes, typically a hash of the
    /// request each spend pays for.  `Some`: the calls go to `act_redeem_(cbor_)return_replay_bound_batch` -- the admission screen is
    /// implied, the outputs are RefundReturns (over 0 without `returned`), and lane i verifies only if its proof was made with the same
    /// 32 bytes (`prove_spend_bound`).  The binding enters neither the receipt nor the nonces.  There is no unique form: with
    /// `unique(true)` the calls panic.  `None`: the unbound calls.
    pub fn bound(mut self, binds: Option<Vec<u8>>) -> Self { self.binds = binds; self }
    fn bind_ptr(&self, n: usize) -> *const u8 {
        self.binds.as_ref().map_or(std::ptr::null(), |b| { assert!(b.len() == 32 * n); b.as_ptr() })
    }
    fn returned_ptr(&self, n: usize) -> *const u8 {
        self.returned.as_ref().map_or(std::ptr::null(), |t| { assert!(t.len() == 32 * n); t.as_ptr() })
    }
    fn charge_ptr(&self, n: usize) -> *const u8 {
        self.charges.as_ref().map_or(std::ptr::null(), |c| { assert!(c.len() == 32 * n); c.as_ptr() })
    }
    /// `keys`: nkeys records of 64 bytes; `proofs`: n records of `PROOF_BYTES`.
    pub fn redeem_replay_batch(&self, keys: &[u8], key_epochs: Option<&[u32]>, sign_with: Option<usize>, proofs: &[u8]) -> Replayed {
        let (n, nkeys) = (proofs.len() / PROOF_BYTES, keys.len() / 64);
        assert!(proofs.len() == n * PROOF_BYTES && key_epochs.map_or(true, |e| e.len() == nkeys));
        assert!(!(self.binds.is_some() && self.unique), "request binding: the bound calls have no unique form");
        let with_t = self.returned.is_some() || self.binds.is_some();
        let rec = if with_t { 160 } else { 128 };
        let mut r = Replayed { rc: 0, status: vec![0u8; n + 1], out: vec![0u8; rec * n + 1], out_key: vec![ACT_KEY_NONE; n + 1], replayed: vec![0u8; n + 1], counts: [0; ACT_REPLAY_COUNTS],
                               admit_counts: [0; ACT_ADMIT_REPLAY_COUNTS], copy_counts: [0; 2], return_too_big: 0, copies_other_amount: 0 };
        let mut u = [0u64; ACT_ADMIT_REPLAY_UNIQUE_COUNTS];
        let mut t = [0u64; ACT_RETURN_REPLAY_COUNTS];
        let mut v = [0u64; ACT_RETURN_REPLAY_UNIQUE_COUNTS];
        r.rc = if self.binds.is_some() { unsafe {
            act_redeem_return_replay_bound_batch(self.ctx, self.set, self.receipts, n, 0, keys.as_ptr(), nkeys as c_int, key_epochs.map_or(std::ptr::null(), |e| e.as_ptr()),
                                                 sign_with.map_or(ACT_SIGN_MATCHED, |i| i as c_int), proofs.as_ptr(), self.bind_ptr(n), self.charge_ptr(n), self.returned_ptr(n),
                                                 self.nonce_key.as_ptr(), r.out.as_mut_ptr(), r.status.as_mut_ptr(), r.out_key.as_mut_ptr(), r.replayed.as_mut_ptr(),
                                                 t.as_mut_ptr())
        } } else if self.returned.is_some() && self.unique { unsafe {
            act_redeem_return_replay_unique_batch(self.ctx, self.set, self.receipts, n, 0, keys.as_ptr(), nkeys as c_int, key_epochs.map_or(std::ptr::null(), |e| e.as_ptr()),
                                                  sign_with.map_or(ACT_SIGN_MATCHED, |i| i as c_int), proofs.as_ptr(), self.charge_ptr(n), self.returned_ptr(n),
                                                  self.nonce_key.as_ptr(), r.out.as_mut_ptr(), r.status.as_mut_ptr(), r.out_key.as_mut_ptr(), r.replayed.as_mut_ptr(),
                                                  v.as_mut_ptr())
        } } else if self.returned.is_some() { unsafe {
            act_redeem_return_replay_batch(self.ctx, self.set, self.receipts, n, 0, keys.as_ptr(), nkeys as c_int, key_epochs.map_or(std::ptr::null(), |e| e.as_ptr()),
                                           sign_with.map_or(ACT_SIGN_MATCHED, |i| i as c_int), proofs.as_ptr(), self.charge_ptr(n), self.returned_ptr(n),
                                           self.nonce_key.as_ptr(), r.out.as_mut_ptr(), r.status.as_mut_ptr(), r.out_key.as_mut_ptr(), r.replayed.as_mut_ptr(), t.as_mut_ptr())
        } } else if self.admit && self.unique { unsafe {
            act_redeem_admit_replay_unique_batch(self.ctx, self.set, self.receipts, n, 0, keys.as_ptr(), nkeys as c_int, key_epochs.map_or(std::ptr::null(), |e| e.as_ptr()),
                                                 sign_with.map_or(ACT_SIGN_MATCHED, |i| i as c_int), proofs.as_ptr(), self.charge_ptr(n), self.nonce_key.as_ptr(),
                                                 r.out.as_mut_ptr(), r.status.as_mut_ptr(), r.out_key.as_mut_ptr(), r.replayed.as_mut_ptr(), u.as_mut_ptr())
        } } else if self.admit { unsafe {
            act_redeem_admit_replay_batch(self.ctx, self.set, self.receipts, n, 0, keys.as_ptr(), nkeys as c_int, key_epochs.map_or(std::ptr::null(), |e| e.as_ptr()),
                                          sign_with.map_or(ACT_SIGN_MATCHED, |i| i as c_int), proofs.as_ptr(), self.charge_ptr(n), self.nonce_key.as_ptr(),
                                          r.out.as_mut_ptr(), r.status.as_mut_ptr(), r.out_key.as_mut_ptr(), r.replayed.as_mut_ptr(), r.admit_counts.as_mut_ptr())
        } } else { unsafe {
            act_redeem_replay_batch(self.ctx, self.set, self.receipts, n, 0, keys.as_ptr(), nkeys as c_int, key_epochs.map_or(std::ptr::null(), |e| e.as_ptr()),
                                    sign_with.map_or(ACT_SIGN_MATCHED, |i| i as c_int), proofs.as_ptr(), self.nonce_key.as_ptr(), r.out.as_mut_ptr(),
                                    r.status.as_mut_ptr(), r.out_key.as_mut_ptr(), r.replayed.as_mut_ptr(), r.counts.as_mut_ptr())
        } };
        if self.returned.is_some() && self.unique { r.take_return_unique_counts(&v); }
        else if with_t { r.take_return_counts(&t); }
        else if self.admit && self.unique { r.take_unique_counts(&u); }
        if self.admit || with_t { r.take_admit_counts(); }
        r.status.truncate(n); r.out.truncate(rec * n); r.out_key.truncate(n); r.replayed.truncate(n);
        r
    }
    /// The same on wire bytes: CBOR SpendProof messages in (a retry may be another spelling of the same proof), CBOR Refund messages out.
    pub fn redeem_cbor_replay_batch(&self, keys: &[u8], key_epochs: Option<&[u32]>, sign_with: Option<usize>, msgs: &[&[u8]]) -> Replayed {
        let (blob, offsets) = gather(msgs);
        let (n, nkeys) = (msgs.len(), keys.len() / 64);
        assert!(key_epochs.map_or(true, |e| e.len() == nkeys));
        assert!(!(self.binds.is_some() && self.unique), "request binding: the bound calls have no unique form");
        let with_t = self.returned.is_some() || self.binds.is_some();
        let rec = if with_t { REFUND_RETURN_CBOR_BYTES } else { REFUND_CBOR_BYTES };
        let mut r = Replayed { rc: 0, status: vec![0u8; n + 1], out: vec![0u8; rec * n + 1], out_key: vec![ACT_KEY_NONE; n + 1], replayed: vec![0u8; n + 1],
                               counts: [0; ACT_REPLAY_COUNTS], admit_counts: [0; ACT_ADMIT_REPLAY_COUNTS], copy_counts: [0; 2], return_too_big: 0, copies_other_amount: 0 };
        let mut u = [0u64; ACT_ADMIT_REPLAY_UNIQUE_COUNTS];
        let mut t = [0u64; ACT_RETURN_REPLAY_COUNTS];
        let mut v = [0u64; ACT_RETURN_REPLAY_UNIQUE_COUNTS];
        r.rc = if self.binds.is_some() { unsafe {
            act_redeem_cbor_return_replay_bound_batch(self.ctx, self.set, self.receipts, n, 0, keys.as_ptr(), nkeys as c_int, key_epochs.map_or(std::ptr::null(), |e| e.as_ptr()),
                                                      sign_with.map_or(ACT_SIGN_MATCHED, |i| i as c_int), blob.as_ptr(), offsets.as_ptr(), self.bind_ptr(n), self.charge_ptr(n),
                                                      self.returned_ptr(n), self.nonce_key.as_ptr(), r.out.as_mut_ptr(), r.status.as_mut_ptr(), r.out_key.as_mut_ptr(),
                                                      r.replayed.as_mut_ptr(), t.as_mut_ptr())
        } } else if self.returned.is_some() && self.unique { unsafe {
            act_redeem_cbor_return_replay_unique_batch(self.ctx, self.set, self.receipts, n, 0, keys.as_ptr(), nkeys as c_int, key_epochs.map_or(std::ptr::null(), |e| e.as_ptr()),
                                                       sign_with.map_or(ACT_SIGN_MATCHED, |i| i as c_int), blob.as_ptr(), offsets.as_ptr(), self.charge_ptr(n),
                                                       self.returned_ptr(n), self.nonce_key.as_ptr(), r.out.as_mut_ptr(), r.status.as_mut_ptr(), r.out_key.as_mut_ptr(),
                                                       r.replayed.as_mut_ptr(), v.as_mut_ptr())
        } } else if self.returned.is_some() { unsafe {
            act_redeem_cbor_return_replay_batch(self.ctx, self.set, self.receipts, n, 0, keys.as_ptr(), nkeys as c_int, key_epochs.map_or(std::ptr::null(), |e| e.as_ptr()),
                                                sign_with.map_or(ACT_SIGN_MATCHED, |i| i as c_int), blob.as_ptr(), offsets.as_ptr(), self.charge_ptr(n), self.returned_ptr(n),
                                                self.nonce_key.as_ptr(), r.out.as_mut_ptr(), r.status.as_mut_ptr(), r.out_key.as_mut_ptr(), r.replayed.as_mut_ptr(),
                                                t.as_mut_ptr())
        } } else if self.admit && self.unique { unsafe {
            act_redeem_cbor_admit_replay_unique_batch(self.ctx, self.set, self.receipts, n, 0, keys.as_ptr(), nkeys as c_int, key_epochs.map_or(std::ptr::null(), |e| e.as_ptr()),
                                                      sign_with.map_or(ACT_SIGN_MATCHED, |i| i as c_int), blob.as_ptr(), offsets.as_ptr(), self.charge_ptr(n),
                                                      self.nonce_key.as_ptr(), r.out.as_mut_ptr(), r.status.as_mut_ptr(), r.out_key.as_mut_ptr(), r.replayed.as_mut_ptr(),
                                                      u.as_mut_ptr())
        } } else if self.admit { unsafe {
            act_redeem_cbor_admit_replay_batch(self.ctx, self.set, self.receipts, n, 0, keys.as_ptr(), nkeys as c_int, key_epochs.map_or(std::ptr::null(), |e| e.as_ptr()),
                                               sign_with.map_or(ACT_SIGN_MATCHED, |i| i as c_int), blob.as_ptr(), offsets.as_ptr(), self.charge_ptr(n),
                                               self.nonce_key.as_ptr(), r.out.as_mut_ptr(), r.status.as_mut_ptr(), r.out_key.as_mut_ptr(), r.replayed.as_mut_ptr(),
                                               r.admit_counts.as_mut_ptr())
        } } else { unsafe {
            act_redeem_cbor_replay_batch(self.ctx, self.set, self.receipts, n, 0, keys.as_ptr(), nkeys as c_int, key_epochs.map_or(std::ptr::null(), |e| e.as_ptr()),
                                         sign_with.map_or(ACT_SIGN_MATCHED, |i| i as c_int), blob.as_ptr(), offsets.as_ptr(), self.nonce_key.as_ptr(),
                                         r.out.as_mut_ptr(), r.status.as_mut_ptr(), r.out_key.as_mut_ptr(), r.replayed.as_mut_ptr(), r.counts.as_mut_ptr())
        } };
        if self.returned.is_some() && self.unique { r.take_return_unique_counts(&v); }
        else if with_t { r.take_return_counts(&t); }
        else if self.admit && self.unique { r.take_unique_counts(&u); }
        if self.admit || with_t { r.take_admit_counts(); }
        r.status.truncate(n); r.out.truncate(rec * n); r.out_key.truncate(n); r.replayed.truncate(n);
        r
    }
    /// The building block: per lane with `status_in[i] == 0` and `key_index[i] < nkeys` the 32-byte receipt tag and the 128 nonce
    /// bytes (`ACT_RNG_PER_LANE` slices for the sign call); zeros elsewhere.  `nullifiers`: n dense 32-byte values.  -> (rc, tags, nonces)
    pub fn derive(&self, keys: &[u8], key_index: &[u8], nullifiers: &[u8], kprime: &[u8], status_in: &[u8]) -> (c_int, Vec<u8>, Vec<u8>) {
        let n = status_in.len();
        assert!(key_index.len() == n && nullifiers.len() == 32 * n && kprime.len() == 32 * n);
        let (mut tags, mut nonces) = (vec![0u8; 32 * n + 1], vec![0u8; 128 * n + 1]);
        let rc = if self.returned.is_some() { unsafe {      // the hashes take the lanes' amounts
            act_replay_derive_return_batch(self.ctx, n, 0, keys.as_ptr(), (keys.len() / 64) as c_int, key_index.as_ptr(), self.nonce_key.as_ptr(), nullifiers.as_ptr(), 32,
                                           kprime.as_ptr(), status_in.as_ptr(), self.returned_ptr(n), tags.as_mut_ptr(), nonces.as_mut_ptr())
        } } else { unsafe {
            act_replay_derive_batch(self.ctx, n, 0, keys.as_ptr(), (keys.len() / 64) as c_int, key_index.as_ptr(), self.nonce_key.as_ptr(), nullifiers.as_ptr(), 32,
                                    kprime.as_ptr(), status_in.as_ptr(), tags.as_mut_ptr(), nonces.as_mut_ptr())
        } };
        tags.truncate(32 * n); nonces.truncate(128 * n);
        (rc, tags, nonces)
    }
}

/// the eleven of `ACT_ADMIT_REPLAY_COUNTS` in their order (`GpuReserve::reserve_batch`)
pub const ACT_RESERVE_COUNTS: usize = 11;
/// lanes / not_reserved / return_too_big / settled / settled_again / other_amount / unanswered (`GpuReserve::settle_batch`)
pub const ACT_SETTLE_COUNTS: usize = 7;
pub const ACT_STATUS_NOT_RESERVED: u8 = 248;
pub const ACT_STATUS_SETTLED_OTHER_AMOUNT: u8 = 247;
/// k^ | enc(K') | s^: what a service keeps per job, with the matched ring index (97 bytes) and, once known, t
pub const RESERVATION_BYTES: usize = 96;
/// statuses, 96-byte reservation records (all zero where rejected), matched ring keys, the replay marks and the counts
pub struct Reserved {
    pub rc: c_int,
    pub status: Vec<u8>,
    pub reservation: Vec<u8>,
    pub out_key: Vec<u8>,
    pub replayed: Vec<u8>,
    pub counts: [u64; ACT_RESERVE_COUNTS],
}
/// statuses, outputs (160-byte RefundReturn records or `REFUND_RETURN_CBOR_BYTES` messages, all zero where not signed), the
/// settled-before marks and the counts
pub struct Settled {
    pub rc: c_int,
    pub status: Vec<u8>,
    pub out: Vec<u8>,
    pub settled_before: Vec<u8>,
    pub counts: [u64; ACT_SETTLE_COUNTS],
}
/// Reserve and settle on ONE GPU (include/act_mi355x.h "reserve and settle"): a metered service records a spend of s with
/// `reserve_batch`, does the work, and signs the partial refund t <= s with `settle_batch`.  `Reserved::replayed[i] == 1` obliges the
/// service to find the job it already started for that nullifier, never to start a second one; settling one reservation again with the
/// same amount gives the same bytes, with another amount `ACT_STATUS_SETTLED_OTHER_AMOUNT`.  Thin: bytes in, bytes out.
pub struct GpuReserve {
    ctx: *mut ActCtx,
    set: *mut ActNullifierSet,
    receipts: *mut ActNullifierSet,
    nonce_key: [u8; 32],
}
impl GpuReserve {
    /// # Safety
    /// `ctx`, `set` and `receipts` are live handles on one device, `set != receipts`, and all three outlive `self`.
    pub unsafe fn from_raw(ctx: *mut ActCtx, set: *mut ActNullifierSet, receipts: *mut ActNullifierSet, nonce_key: [u8; 32]) -> Self {
        GpuReserve { ctx, set, receipts, nonce_key }
    }
    fn reserved(n: usize) -> Reserved {
        Reserved { rc: 0, status: vec![0u8; n + 1], reservation: vec![0u8; RESERVATION_BYTES * n + 1], out_key: vec![ACT_KEY_NONE; n + 1], replayed: vec![0u8; n + 1],
                   counts: [0; ACT_RESERVE_COUNTS] }
    }
    /// `keys`: nkeys records of 64 bytes; `proofs`: n records of `PROOF_BYTES`; `charges`: n scalars of 32 bytes or `None`.
    pub fn reserve_batch(&self, keys: &[u8], key_epochs: Option<&[u32]>, proofs: &[u8], charges: Option<&[u8]>) -> Reserved {
        let (n, nkeys) = (proofs.len() / PROOF_BYTES, keys.len() / 64);
        assert!(proofs.len() == n * PROOF_BYTES && key_epochs.map_or(true, |e| e.len() == nkeys) && charges.map_or(true, |c| c.len() == 32 * n));
        let mut r = Self::reserved(n);
        r.rc = unsafe {
            act_redeem_reserve_batch(self.ctx, self.set, self.receipts, n, 0, keys.as_ptr(), nkeys as c_int, key_epochs.map_or(std::ptr::null(), |e| e.as_ptr()),
                                     proofs.as_ptr(), charges.map_or(std::ptr::null(), |c| c.as_ptr()), r.reservation.as_mut_ptr(), r.status.as_mut_ptr(),
                                     r.out_key.as_mut_ptr(), r.replayed.as_mut_ptr(), r.counts.as_mut_ptr())
        };
        r.status.truncate(n); r.reservation.truncate(RESERVATION_BYTES * n); r.out_key.truncate(n); r.replayed.truncate(n);
        r
    }
    /// `reserve_batch` under request bindings (include/act_mi355x.h "request binding"): `binds` = n values of 32 bytes; lane i verifies
    /// only if its proof was made with binds[i], so a recorded reservation's proof resent beside another request is an invalid proof,
    /// not `replayed[i] == 1`.  Settle takes no binding.
    pub fn reserve_bound_batch(&self, keys: &[u8], key_epochs: Option<&[u32]>, proofs: &[u8], binds: &[u8], charges: Option<&[u8]>) -> Reserved {
        let (n, nkeys) = (proofs.len() / PROOF_BYTES, keys.len() / 64);
        assert!(proofs.len() == n * PROOF_BYTES && binds.len() == 32 * n && key_epochs.map_or(true, |e| e.len() == nkeys) && charges.map_or(true, |c| c.len() == 32 * n));
        let mut r = Self::reserved(n);
        r.rc = unsafe {
            act_redeem_reserve_bound_batch(self.ctx, self.set, self.receipts, n, 0, keys.as_ptr(), nkeys as c_int, key_epochs.map_or(std::ptr::null(), |e| e.as_ptr()),
                                           proofs.as_ptr(), binds.as_ptr(), charges.map_or(std::ptr::null(), |c| c.as_ptr()), r.reservation.as_mut_ptr(),
                                           r.status.as_mut_ptr(), r.out_key.as_mut_ptr(), r.replayed.as_mut_ptr(), r.counts.as_mut_ptr())
        };
        r.status.truncate(n); r.reservation.truncate(RESERVATION_BYTES * n); r.out_key.truncate(n); r.replayed.truncate(n);
        r
    }
    /// The same on wire bytes.
    pub fn reserve_cbor_bound_batch(&self, keys: &[u8], key_epochs: Option<&[u32]>, msgs: &[&[u8]], binds: &[u8], charges: Option<&[u8]>) -> Reserved {
        let (blob, offsets) = gather(msgs);
        let (n, nkeys) = (msgs.len(), keys.len() / 64);
        assert!(binds.len() == 32 * n && key_epochs.map_or(true, |e| e.len() == nkeys) && charges.map_or(true, |c| c.len() == 32 * n));
        let mut r = Self::reserved(n);
        r.rc = unsafe {
            act_redeem_cbor_reserve_bound_batch(self.ctx, self.set, self.receipts, n, 0, keys.as_ptr(), nkeys as c_int, key_epochs.map_or(std::ptr::null(), |e| e.as_ptr()),
                                                blob.as_ptr(), offsets.as_ptr(), binds.as_ptr(), charges.map_or(std::ptr::null(), |c| c.as_ptr()),
                                                r.reservation.as_mut_ptr(), r.status.as_mut_ptr(), r.out_key.as_mut_ptr(), r.replayed.as_mut_ptr(), r.counts.as_mut_ptr())
        };
        r.status.truncate(n); r.reservation.truncate(RESERVATION_BYTES * n); r.out_key.truncate(n); r.replayed.truncate(n);
        r
    }
    /// The same on wire bytes: CBOR SpendProof messages in (a retry may be another spelling of the same proof).
    pub fn reserve_cbor_batch(&self, keys: &[u8], key_epochs: Option<&[u32]>, msgs: &[&[u8]], charges: Option<&[u8]>) -> Reserved {
        let (blob, offsets) = gather(msgs);
        let (n, nkeys) = (msgs.len(), keys.len() / 64);
        assert!(key_epochs.map_or(true, |e| e.len() == nkeys) && charges.map_or(true, |c| c.len() == 32 * n));
        let mut r = Self::reserved(n);
        r.rc = unsafe {
            act_redeem_cbor_reserve_batch(self.ctx, self.set, self.receipts, n, 0, keys.as_ptr(), nkeys as c_int, key_epochs.map_or(std::ptr::null(), |e| e.as_ptr()),
                                          blob.as_ptr(), offsets.as_ptr(), charges.map_or(std::ptr::null(), |c| c.as_ptr()), r.reservation.as_mut_ptr(),
                                          r.status.as_mut_ptr(), r.out_key.as_mut_ptr(), r.replayed.as_mut_ptr(), r.counts.as_mut_ptr())
        };
        r.status.truncate(n); r.reservation.truncate(RESERVATION_BYTES * n); r.out_key.truncate(n); r.replayed.truncate(n);
        r
    }
    /// `reservations`: n records of `RESERVATION_BYTES`; `key_index`: what reserve left in `out_key`; `amounts`: n scalars of 32 bytes
    /// (`None`: every t = 0); `cbor`: CBOR RefundReturn messages out instead of 160-byte records.
    pub fn settle_batch(&self, keys: &[u8], key_epochs: Option<&[u32]>, sign_with: Option<usize>, reservations: &[u8], key_index: &[u8], amounts: Option<&[u8]>,
                        cbor: bool) -> Settled {
        let (n, nkeys) = (key_index.len(), keys.len() / 64);
        assert!(reservations.len() == RESERVATION_BYTES * n && key_epochs.map_or(true, |e| e.len() == nkeys) && amounts.map_or(true, |t| t.len() == 32 * n));
        let rec = if cbor { REFUND_RETURN_CBOR_BYTES } else { 160 };
        let mut r = Settled { rc: 0, status: vec![0u8; n + 1], out: vec![0u8; rec * n + 1], settled_before: vec![0u8; n + 1], counts: [0; ACT_SETTLE_COUNTS] };
        r.rc = if cbor { unsafe {
            act_redeem_cbor_settle_batch(self.ctx, self.receipts, n, 0, keys.as_ptr(), nkeys as c_int, key_epochs.map_or(std::ptr::null(), |e| e.as_ptr()),
                                         sign_with.map_or(ACT_SIGN_MATCHED, |i| i as c_int), reservations.as_ptr(), key_index.as_ptr(),
                                         amounts.map_or(std::ptr::null(), |t| t.as_ptr()), self.nonce_key.as_ptr(), r.out.as_mut_ptr(), r.status.as_mut_ptr(),
                                         r.settled_before.as_mut_ptr(), r.counts.as_mut_ptr())
        } } else { unsafe {
            act_redeem_settle_batch(self.ctx, self.receipts, n, 0, keys.as_ptr(), nkeys as c_int, key_epochs.map_or(std::ptr::null(), |e| e.as_ptr()),
                                    sign_with.map_or(ACT_SIGN_MATCHED, |i| i as c_int), reservations.as_ptr(), key_index.as_ptr(),
                                    amounts.map_or(std::ptr::null(), |t| t.as_ptr()), self.nonce_key.as_ptr(), r.out.as_mut_ptr(), r.status.as_mut_ptr(),
                                    r.settled_before.as_mut_ptr(), r.counts.as_mut_ptr())
        } };
        r.status.truncate(n); r.out.truncate(rec * n); r.settled_before.truncate(n);
        r
    }
}

/// What the node dispatcher knows about its GPUs (load balance: include/act_mi355x.h "Load balance"): per device its weight
/// (relative speed, mean 1) and the lanes / seconds / calls of the most recent cut call.
pub fn gpu_device_stats(params: &Params) -> Vec<(f64, u64, f64, u64)> {
    let gpu = params.gpu();
    let mut out = Vec::new();
    let mut k = 0;
    loop {
        let (mut w, mut lanes, mut secs, mut calls) = (0f64, 0u64, 0f64, 0u64);
        if unsafe { act_node_device_stats(gpu.0, k, &mut w, &mut lanes, &mut secs, &mut calls) } != 0 {
            break;
        }
        out.push((w, lanes, secs, calls));
        k += 1;
    }
    out
}

// ---- the kept single-call signatures: batches of one ------------------------------------------------------------------
// In src/lib.rs the six existing method bodies become `#[cfg(not(feature = "mi355x"))]`; these take their place otherwise: with the
// feature on, nothing of the protocol runs on the CPU.  One item per call is latency, not throughput, and a GPU's latency is a
// dependent chain on a few lanes (docs/history/profiles/r04_single_item_latency.txt; the C port on one core of the same box in brackets):
//     request 0.59 ms (0.05)    issue 2.7 (0.25)    PreIssuance::to_credit_token 2.3 (0.21)
//     prove_spend 3.1 (15.5)    refund 3.5 (17.3)   PreRefund::to_credit_token 3.0 (5.0)
// The `*_batch` siblings are where the rates are (24 M issues/s, 112 M requests/s, 520 k refunds/s).
#[cfg(feature = "mi355x")]
impl PreIssuance {
    pub fn request(&self, params: &Params, rng: impl CryptoRngCore) -> IssuanceRequest {
        // src/lib.rs:463
        Self::request_batch(std::slice::from_ref(self), params, rng).pop().unwrap()
    }
    pub fn to_credit_token(&self, params: &Params, public: &PublicKey, request: &IssuanceRequest, response: &IssuanceResponse)
        -> Result<CreditToken, Error> {
        // src/lib.rs:528-534
        Self::to_credit_token_batch(std::slice::from_ref(self), params, public, std::slice::from_ref(request), std::slice::from_ref(response)).pop().unwrap()
    }
}
#[cfg(feature = "mi355x")]
impl PrivateKey {
    pub fn issue(&self, params: &Params, request: &IssuanceRequest, c: Scalar, rng: impl CryptoRngCore) -> Result<IssuanceResponse, Error> {
        // src/lib.rs:621-627
        self.issue_batch(params, std::slice::from_ref(request), &[c], rng).pop().unwrap()
    }
    pub fn refund(&self, params: &Params, spend_proof: &SpendProof, rng: impl CryptoRngCore) -> Result<Refund, Error> {
        // src/lib.rs:781-786
        self.refund_batch(params, std::slice::from_ref(spend_proof), rng).pop().unwrap()
    }
}
#[cfg(feature = "mi355x")]
impl CreditToken {
    pub fn prove_spend(&self, params: &Params, s: Scalar, rng: impl CryptoRngCore) -> (SpendProof, PreRefund) {
        // src/lib.rs:972-977
        Self::prove_spend_batch(std::slice::from_ref(self), params, &[s], rng).pop().unwrap()
    }
}
#[cfg(feature = "mi355x")]
impl PreRefund {
    pub fn to_credit_token(&self, params: &Params, spend_proof: &SpendProof, refund: &Refund, public_key: &PublicKey) -> Result<CreditToken, Error> {
        // src/lib.rs:1217-1223
        Self::to_credit_token_batch(std::slice::from_ref(self), params, std::slice::from_ref(spend_proof), std::slice::from_ref(refund), public_key).pop().unwrap()
    }
}

// ---- one library call per item, with nonce bytes the CALLER has already drawn ----------------------------------------------------
// NOT part of the drop-in surface, and deliberately not methods that take a generator.  `PrivateKey::issue` / `refund` above keep the
// crate's contract exactly -- e and alpha are drawn only after the checks have passed (src/lib.rs:638-643, 842-846), so a rejected
// item leaves the caller's generator untouched -- and pay for it with two library calls (check, then sign).  The functions below are
// ONE call: the signature is computed BESIDE the check (issue 1.25 ms instead of ~2.0, refund 1.95 instead of ~2.8, a wire-level
// redemption 2.1 instead of 3.2), which is only possible if the 128 bytes that seed (e, alpha) exist before the verdict does.  They
// therefore take the BYTES, not a generator: there is no generator state here that could disagree with the crate's, and what
// happens to the bytes of a rejected item is the caller's explicit decision (they were read by the GPU and wiped there; never use
// them again).  A caller whose generator is the operating system's loses nothing; a caller that replays a deterministic stream and
// must match the crate's draws byte for byte stays with the methods above.
#[cfg(feature = "mi355x")]
pub mod predrawn {
    use super::*;

    /// 128 bytes from `rng`, drawn as two `Scalar::random` would draw them (two 64-byte `fill_bytes`).
    pub fn nonce_bytes(mut rng: impl CryptoRngCore) -> [u8; 128] {
        let v = draw(&mut rng, 2);
        let mut out = [0u8; 128];
        out.copy_from_slice(&v);
        out
    }
    /// `sk.refund(params, proof, rng)` for an rng whose next 128 bytes are `nonces` -- if the proof verifies.  If it does not, the
    /// result is the same `Err`, and `nonces` have been spent on nothing.
    pub fn refund(sk: &PrivateKey, params: &Params, spend_proof: &SpendProof, nonces: &[u8; 128]) -> Result<Refund, Error> {
        let mut rec = Vec::with_capacity(PROOF_BYTES);
        spend_proof.write_record(&mut rec);
        let (skr, gpu) = (sk.record(), params.gpu());
        let (mut out, mut status) = ([0u8; 128], [0u8; 1]);
        gpu.check(unsafe { act_node_refund_batch(gpu.0, 1, skr.as_ptr(), rec.as_ptr(), nonces.as_ptr(), ACT_RNG_SEQUENTIAL, out.as_mut_ptr(), status.as_mut_ptr()) });
        if status[0] == 0 { Ok(Refund::from_record(&out)) } else { Err(status_to_error(status[0])) }
    }
    /// `sk.issue(params, request, c, rng)` for an rng whose next 128 bytes are `nonces`, the signature beside the request's proof of
    /// knowledge (src/lib.rs:629-660).
    pub fn issue(sk: &PrivateKey, params: &Params, request: &IssuanceRequest, c: Scalar, nonces: &[u8; 128]) -> Result<IssuanceResponse, Error> {
        let (mut req, mut cb) = (Vec::with_capacity(128), Vec::with_capacity(32));
        request.write_record(&mut req);
        put_s(&mut cb, &c);
        let (skr, gpu) = (sk.record(), params.gpu());
        let (mut out, mut status) = ([0u8; 160], [0u8; 1]);
        gpu.check(unsafe { act_node_issue_batch(gpu.0, 1, skr.as_ptr(), req.as_ptr(), cb.as_ptr(), nonces.as_ptr(), ACT_RNG_SEQUENTIAL, out.as_mut_ptr(), status.as_mut_ptr()) });
        if status[0] == 0 { Ok(IssuanceResponse::from_record(&out)) } else { Err(status_to_error(status[0])) }
    }
    /// One CBOR `SpendProof` message in, one CBOR `Refund` message out: unframing, verification and the signature beside it.
    pub fn refund_cbor(sk: &PrivateKey, params: &Params, msg: &[u8], nonces: &[u8; 128]) -> Result<Vec<u8>, WireError> {
        let offsets = [0u64, msg.len() as u64];
        let (skr, gpu) = (sk.record(), params.gpu());
        let (mut out, mut status) = (vec![0u8; REFUND_CBOR_BYTES + 1], vec![0u8; 2]);
        gpu.check(unsafe {
            act_node_refund_cbor_batch(gpu.0, 1, skr.as_ptr(), msg.as_ptr(), offsets.as_ptr(), nonces.as_ptr(), ACT_RNG_SEQUENTIAL, out.as_mut_ptr(), status.as_mut_ptr())
        });
        refund_messages(&out, &status[..1]).pop().unwrap()
    }
    /// One CBOR `IssuanceRequest` message in, one CBOR `IssuanceResponse` message out: unframing, the proof-of-knowledge check and the
    /// signature beside it (src/lib.rs:629-660).  A rejected message has spent `nonces` on nothing.
    pub fn issue_cbor(sk: &PrivateKey, params: &Params, msg: &[u8], c: Scalar, nonces: &[u8; 128]) -> Result<Vec<u8>, WireError> {
        let offsets = [0u64, msg.len() as u64];
        let mut cb = Vec::with_capacity(32);
        put_s(&mut cb, &c);
        let (skr, gpu) = (sk.record(), params.gpu());
        let (mut out, mut status) = (vec![0u8; ISSUANCE_RESPONSE_CBOR_BYTES + 1], vec![0u8; 2]);
        gpu.check(unsafe {
            act_node_issue_cbor_batch(gpu.0, 1, skr.as_ptr(), msg.as_ptr(), offsets.as_ptr(), cb.as_ptr(), nonces.as_ptr(), ACT_RNG_SEQUENTIAL,
                                      out.as_mut_ptr(), status.as_mut_ptr())
        });
        issuance_messages(&out, &status[..1]).pop().unwrap()
    }
    /// The whole redemption step for one message: the refund is computed first (one call), THEN the store decides whether it is handed
    /// out; a rejected message or a double spend has spent `nonces` on nothing.
    pub fn redeem_cbor(sk: &PrivateKey, params: &Params, store: &GpuNullifierStore, msg: &[u8], nonces: &[u8; 128]) -> Redeemed<Vec<u8>> {
        let offsets = [0u64, msg.len() as u64];
        let (skr, gpu) = (sk.record(), params.gpu());
        let (mut out, mut status) = (vec![0u8; REFUND_CBOR_BYTES + 1], vec![0u8; 2]);
        let rc = unsafe {
            act_node_redeem_cbor_batch(gpu.0, store.0, 1, skr.as_ptr(), msg.as_ptr(), offsets.as_ptr(), nonces.as_ptr(), ACT_RNG_SEQUENTIAL, out.as_mut_ptr(), status.as_mut_ptr())
        };
        let engine_failure = if rc != 0 { Some(unsafe { CStr::from_ptr(act_node_last_error(gpu.0)) }.to_string_lossy().into_owned()) } else { None };
        Redeemed { lanes: refund_messages(&out, &status[..1]), engine_failure }
    }
}
