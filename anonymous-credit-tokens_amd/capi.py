"""ctypes binding of libact_mi355x.so (C ABI: include/act_mi355x.h).  Host side only moves bytes."""
from __future__ import annotations

import ctypes as C
import math
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ACT_LIB_PATH") or os.path.join(_HERE, "libact_mi355x.so")   # override: tuning A/B runs only

MEM_HOST, MEM_DEVICE = 0, 1
RNG_PER_LANE, RNG_SEQUENTIAL, RNG_CALLBACK = 0, 1, 2
TRANSCRIPT_HOST, TRANSCRIPT_DEVICE = 0, 1
WIRE_READER_HOST, WIRE_READER_DEVICE = 0, 1      # act_ctx_set_wire_reader: where a message that is not the canonical encoding is read
WIRE_STATS = ("seen", "canonical", "read_on_device", "read_by_host")
KEYRING_MAX, KEY_NONE, SIGN_MATCHED = 4, 255, -1      # act_*_keyring_batch: ring size, "no ring key matched", "sign with the matched key"
STATUS_WRONG_CHARGE = 250                             # act_redeem_*admit_batch: s is not the expected charge
ADMIT_COUNTS = ("lanes", "wire_rejected", "wrong_charge", "spent_before", "verified", "rejected_by_verification", "double_spend_after", "accepted")
STATUS_RETURN_TOO_BIG = 249                           # act_redeem_*return_batch: the returned amount t exceeds the charge s
REDEEM_RETURN_COUNTS = ADMIT_COUNTS + ("return_too_big",)      # act_redeem_*return_batch
REDEEM_RETURN_UNIQUE_COUNTS = REDEEM_RETURN_COUNTS + ("copies",)      # act_redeem_*return_unique_batch
ADMIT_UNIQUE_COUNTS = ADMIT_COUNTS + ("copies",)      # act_redeem_*admit_unique_batch: lanes with the bytes of an earlier lane, not verified
REPLAY_COUNTS = ("lanes", "rejected_by_verification", "fresh", "replayed", "double_spend", "unanswered")      # act_redeem_*replay_batch
ADMIT_REPLAY_COUNTS = ("lanes", "wire_rejected", "wrong_charge", "foreign_spend", "retry_candidates", "verified", "rejected_by_verification", "fresh", "replayed",
                       "double_spend_after", "unanswered")      # act_redeem_*admit_replay_batch
ADMIT_REPLAY_UNIQUE_COUNTS = ADMIT_REPLAY_COUNTS + ("copies", "copies_served")      # act_redeem_*admit_replay_unique_batch: copies, and those whose leader ended 0
RETURN_REPLAY_COUNTS = ADMIT_REPLAY_COUNTS + ("return_too_big",)      # act_redeem_*return_replay_batch
# act_redeem_*return_replay_unique_batch: copies, those answered 0, and those that name another amount than their leader
RETURN_REPLAY_UNIQUE_COUNTS = RETURN_REPLAY_COUNTS + ("copies", "copies_served", "copies_other_amount")
# reserve and settle (act_redeem_*reserve_batch / act_redeem_*settle_batch): record a spend now, sign its partial refund later
STATUS_NOT_RESERVED, STATUS_SETTLED_OTHER_AMOUNT = 248, 247
RESERVATION_BYTES = 96                                # k^ | enc(K') | s^
RESERVE_COUNTS = ADMIT_REPLAY_COUNTS
SETTLE_COUNTS = ("lanes", "not_reserved", "return_too_big", "settled", "settled_again", "other_amount", "unanswered")
_ERRS = {1: "ACT_ERR_ARG", 2: "ACT_ERR_HIP", 3: "ACT_ERR_PARAMS", 4: "ACT_ERR_NO_DEVICE", 5: "ACT_ERR_RNG"}

EXPORTS = [
    "act_params_new", "act_params_random", "act_ctx_create", "act_ctx_destroy", "act_ctx_set_transcript_mode",
    "act_ctx_set_host_threads", "act_host_usable_cpus", "act_host_hash_many", "act_host_parallel_for", "act_host_pool_stats", "act_ctx_streams_overlap", "act_ctx_set_pipeline_depth", "act_ctx_set_small_batch_max", "act_ctx_set_fixed_base_bits", "act_node_set_fixed_base_bits", "act_tuning_set", "act_build_has_ct_secret_tables", "act_ctx_fixed_base_bits", "act_last_error", "act_spend_proof_bytes", "act_prove_rng_bytes",
    "act_spend_transcript_bytes", "act_private_key_random", "act_pre_issuance_random_batch", "act_request_batch",
    "act_issue_batch", "act_issuance_to_credit_token_batch", "act_prove_spend_batch", "act_prove_spend_seeded_batch", "act_node_prove_spend_seeded_batch", "act_verify_spend_batch",
    "act_refund_batch", "act_refund_to_credit_token_batch", "act_debug_last_spend_transcripts", "act_debug_scalarmult_batch", "act_debug_fixed_base_batch", "act_debug_fe_batch", "act_debug_sc_batch", "act_debug_fixed_base_mf_batch", "act_debug_chain_ct_batch", "act_debug_secret_residue", "act_prof_enable",
    "act_prof_reset", "act_prof_kernel_count", "act_prof_kernel_name", "act_prof_get", "act_prof_get_busy", "act_ubench_mad_u64_u32", "act_ubench_random_read", "act_ubench_table_read",
    "act_cbor_size", "act_cbor_record_bytes", "act_cbor_encode_batch", "act_cbor_decode_batch", "act_cbor_read_batch", "act_ctx_set_wire_reader", "act_ctx_wire_stats", "act_node_set_wire_reader", "act_verify_spend_cbor_batch",
    "act_node_verify_spend_cbor_batch", "act_redeem_batch", "act_node_redeem_batch",
    "act_nullifier_set_create", "act_nullifier_set_destroy", "act_nullifier_set_len", "act_nullifier_set_last_error",
    "act_nullifier_check_and_insert_batch", "act_nullifier_set_reserve", "act_nullifier_set_export", "act_nullifier_contains_batch",
    "act_issue_check_batch", "act_issue_sign_batch", "act_refund_sign_batch",
    "act_node_create", "act_node_destroy", "act_node_device_count", "act_node_ctx", "act_node_last_error", "act_node_set_transcript_mode",
    "act_node_set_host_threads", "act_node_request_batch", "act_node_issue_batch", "act_node_issuance_to_credit_token_batch",
    "act_node_prove_spend_batch", "act_node_verify_spend_batch", "act_node_refund_batch", "act_node_refund_to_credit_token_batch",
    "act_node_issue_check_batch", "act_node_issue_sign_batch", "act_node_refund_sign_batch",
    "act_node_nullifier_set_create", "act_node_nullifier_set_destroy", "act_node_nullifier_set_len", "act_node_nullifier_set_last_error",
    "act_node_nullifier_check_and_insert_batch", "act_node_nullifier_set_reserve", "act_node_nullifier_set_export", "act_node_nullifier_contains_batch",
    "act_verify_spend_cbor_keys_batch", "act_node_verify_spend_cbor_keys_batch", "act_refund_sign_cbor_batch", "act_refund_cbor_batch", "act_refund_cbor_keys_batch",
    "act_node_refund_sign_cbor_batch", "act_node_refund_cbor_batch", "act_redeem_cbor_batch", "act_node_redeem_cbor_batch",
    "act_verify_spend_keyring_batch", "act_refund_sign_keyring_batch", "act_redeem_keyring_batch", "act_redeem_cbor_keyring_batch",
    "act_node_verify_spend_keyring_batch", "act_node_refund_sign_keyring_batch", "act_node_redeem_keyring_batch", "act_node_redeem_cbor_keyring_batch",
    "act_nullifier_check_and_insert_epoch_batch", "act_nullifier_set_epoch_len", "act_nullifier_set_retire_epoch", "act_nullifier_set_retired_epochs",
    "act_nullifier_set_export_epochs", "act_redeem_keyring_epochs_batch", "act_redeem_cbor_keyring_epochs_batch",
    "act_node_nullifier_check_and_insert_epoch_batch", "act_node_nullifier_set_epoch_len", "act_node_nullifier_set_retire_epoch",
    "act_node_nullifier_set_retired_epochs", "act_node_nullifier_set_export_epochs", "act_node_redeem_keyring_epochs_batch",
    "act_node_redeem_cbor_keyring_epochs_batch",
    "act_redeem_admit_batch", "act_redeem_cbor_admit_batch", "act_redeem_admit_unique_batch", "act_redeem_cbor_admit_unique_batch", "act_debug_copy_leaders",
    "act_redeem_replay_batch", "act_redeem_cbor_replay_batch", "act_replay_derive_batch",
    "act_redeem_admit_replay_batch", "act_redeem_cbor_admit_replay_batch", "act_redeem_admit_replay_unique_batch", "act_redeem_cbor_admit_replay_unique_batch",
    "act_issuance_to_credit_token_keyring_batch", "act_refund_to_credit_token_keyring_batch",
    "act_issue_check_cbor_batch", "act_issue_sign_cbor_batch", "act_issue_cbor_batch",
    "act_node_issue_check_cbor_batch", "act_node_issue_sign_cbor_batch", "act_node_issue_cbor_batch",
    "act_refund_sign_return_keyring_batch", "act_redeem_return_batch", "act_redeem_cbor_return_batch", "act_refund_to_credit_token_return_batch",
    "act_refund_to_credit_token_return_keyring_batch", "act_redeem_return_unique_batch", "act_redeem_cbor_return_unique_batch",
    "act_redeem_return_replay_batch", "act_redeem_cbor_return_replay_batch", "act_replay_derive_return_batch",
    "act_redeem_return_replay_unique_batch", "act_redeem_cbor_return_replay_unique_batch",
    "act_redeem_reserve_batch", "act_redeem_cbor_reserve_batch", "act_redeem_settle_batch", "act_redeem_cbor_settle_batch",
    "act_prove_spend_bound_batch", "act_verify_spend_keyring_bound_batch", "act_redeem_return_replay_bound_batch", "act_redeem_cbor_return_replay_bound_batch",
    "act_redeem_reserve_bound_batch", "act_redeem_cbor_reserve_bound_batch",
    "act_ctx_host_hash_stats", "act_ctx_set_tiny_calls", "act_node_set_balance", "act_node_device_stats", "act_node_balance_state", "act_debug_set_slowdown", "act_debug_fail_next_signs",
]
CBOR_TYPES = {"IssuanceRequest": 1, "IssuanceResponse": 2, "SpendProof": 3, "Refund": 4, "PrivateKey": 5, "PublicKey": 6,
              "PreIssuance": 7, "CreditToken": 8, "PreRefund": 9, "RefundReturn": 10}


class ActError(RuntimeError):
    pass


_UNBOUND = object()      # request binding: "no bind argument" (the unbound call); bind=None is the bound call with a NULL pointer


def build(jobs: int = 8) -> str:
    """Compile every HIP source for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    # `all` = libact_mi355x.so, address-free for every secret (the reference's constant-time posture); `fast` =
    # libact_mi355x_fast.so, the same library with scalar-addressed tables for the CLIENT's secrets (prover, request)
    subprocess.run(["make", "-C", os.path.join(_HERE, "csrc"), f"-j{jobs}", "-s", "all", "fast"], check=True)
    return LIB_PATH


_lib = None


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ActError(f"{LIB_PATH} is missing: build it with act_amd.build() / make -C anonymous-credit-tokens_amd/csrc "
                       "(the HIP engine is the only implementation; there is no CPU fallback)")
    # PyTorch ships its own libamdhip64; if this library initialises HIP first (binding /opt/rocm's copy) a later
    # `import torch` in the same process reports "No HIP GPUs are available".  Loading torch's runtime first makes
    # both use one copy, whichever order the caller imports things in.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    vp, sz, i32, u8p = C.c_void_p, C.c_size_t, C.c_int, C.c_void_p
    lib.act_params_new.argtypes = [i32, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, u8p]
    lib.act_params_random.argtypes = [i32, u8p, u8p]
    lib.act_ctx_create.argtypes = [u8p, i32, i32, sz, C.POINTER(vp)]
    lib.act_ctx_destroy.argtypes = [vp]
    lib.act_ctx_destroy.restype = None
    lib.act_ctx_set_transcript_mode.argtypes = [vp, i32]
    lib.act_ctx_set_host_threads.argtypes = [vp, i32]
    lib.act_ctx_set_pipeline_depth.argtypes = [vp, i32]
    lib.act_ctx_set_small_batch_max.argtypes = [vp, sz]
    lib.act_ctx_set_fixed_base_bits.argtypes = [vp, i32, i32]
    lib.act_node_set_fixed_base_bits.argtypes = [vp, i32, i32]
    lib.act_tuning_set.argtypes = [C.c_char_p, C.c_int64]
    lib.act_host_usable_cpus.argtypes = []
    lib.act_host_hash_many.argtypes = [u8p, sz, C.c_uint32, sz, i32, u8p]
    lib.act_host_hash_many.restype = None
    lib.act_host_parallel_for.argtypes = [C.c_size_t, C.c_size_t, C.c_int, C.CFUNCTYPE(None, C.c_void_p, C.c_size_t, C.c_size_t), C.c_void_p]
    lib.act_host_parallel_for.restype = None
    lib.act_host_pool_stats.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
    lib.act_host_pool_stats.restype = None
    lib.act_ctx_streams_overlap.argtypes = [vp]
    lib.act_build_has_ct_secret_tables.argtypes = []
    lib.act_ctx_fixed_base_bits.argtypes = [vp, i32]
    lib.act_last_error.argtypes = [vp]
    lib.act_last_error.restype = C.c_char_p
    for f in ("act_spend_proof_bytes", "act_prove_rng_bytes", "act_spend_transcript_bytes"):
        getattr(lib, f).argtypes = [vp]
        getattr(lib, f).restype = sz
    lib.act_private_key_random.argtypes = [vp, u8p, u8p]
    lib.act_pre_issuance_random_batch.argtypes = [vp, sz, i32, u8p, u8p]
    lib.act_request_batch.argtypes = [vp, sz, i32, u8p, u8p, u8p]
    lib.act_issue_batch.argtypes = [vp, sz, i32, u8p, u8p, u8p, u8p, i32, u8p, u8p]
    lib.act_issuance_to_credit_token_batch.argtypes = [vp, sz, i32, u8p, u8p, u8p, u8p, u8p, u8p]
    lib.act_prove_spend_batch.argtypes = [vp, sz, i32, u8p, u8p, u8p, u8p, u8p, u8p]
    lib.act_prove_spend_seeded_batch.argtypes = [vp, sz, i32, u8p, u8p, u8p, C.c_uint64, u8p, u8p, u8p]
    lib.act_node_prove_spend_seeded_batch.argtypes = [vp, sz, u8p, u8p, u8p, C.c_uint64, u8p, u8p, u8p]
    lib.act_verify_spend_batch.argtypes = [vp, sz, i32, u8p, u8p, u8p, u8p]
    lib.act_refund_batch.argtypes = [vp, sz, i32, u8p, u8p, u8p, i32, u8p, u8p]
    lib.act_refund_to_credit_token_batch.argtypes = [vp, sz, i32, u8p, u8p, u8p, u8p, u8p, u8p]
    lib.act_issuance_to_credit_token_keyring_batch.argtypes = [vp, sz, i32, u8p, u8p, C.c_uint32, u8p, u8p, u8p, u8p, u8p]
    lib.act_refund_to_credit_token_keyring_batch.argtypes = [vp, sz, i32, u8p, u8p, u8p, u8p, C.c_uint32, u8p, u8p, u8p]
    lib.act_debug_last_spend_transcripts.argtypes = [vp, sz, u8p, C.POINTER(sz)]
    lib.act_debug_scalarmult_batch.argtypes = [vp, sz, i32, u8p, u8p, u8p, u8p]
    lib.act_debug_fixed_base_batch.argtypes = [vp, i32, sz, i32, u8p, u8p]
    lib.act_debug_fe_batch.argtypes = [vp, i32, i32, sz, u8p, u8p, u8p, u8p, u8p, u8p]
    lib.act_debug_sc_batch.argtypes = [vp, i32, sz, u8p, u8p, u8p, u8p]
    lib.act_debug_fixed_base_mf_batch.argtypes = [vp, i32, i32, sz, i32, u8p, u8p]
    lib.act_debug_chain_ct_batch.argtypes = [vp, i32, sz, i32, u8p, u8p, u8p, u8p, u8p, u8p]
    lib.act_debug_secret_residue.argtypes = [vp, C.POINTER(sz)]
    for f in ("act_cbor_size", "act_cbor_record_bytes"):
        getattr(lib, f).argtypes = [vp, i32]
        getattr(lib, f).restype = sz
    lib.act_cbor_encode_batch.argtypes = [vp, i32, sz, i32, u8p, u8p]
    lib.act_cbor_decode_batch.argtypes = [vp, i32, sz, i32, u8p, vp, u8p, u8p]
    lib.act_cbor_read_batch.argtypes = [vp, i32, sz, i32, u8p, vp, u8p, u8p]
    lib.act_ctx_set_wire_reader.argtypes = [vp, i32]
    lib.act_ctx_wire_stats.argtypes = [vp, vp, i32]
    lib.act_node_set_wire_reader.argtypes = [vp, i32]
    lib.act_verify_spend_cbor_batch.argtypes = [vp, sz, i32, u8p, u8p, vp, u8p, u8p]
    lib.act_node_verify_spend_cbor_batch.argtypes = [vp, sz, u8p, u8p, vp, u8p, u8p]
    lib.act_redeem_batch.argtypes = [vp, vp, sz, i32, u8p, u8p, u8p, i32, u8p, u8p]
    lib.act_node_redeem_batch.argtypes = [vp, vp, sz, u8p, u8p, u8p, i32, u8p, u8p]
    lib.act_nullifier_set_create.argtypes = [i32, sz, u8p, C.POINTER(vp)]
    lib.act_nullifier_set_destroy.argtypes = [vp]
    lib.act_nullifier_set_destroy.restype = None
    lib.act_nullifier_set_len.argtypes = [vp]
    lib.act_nullifier_set_len.restype = sz
    lib.act_nullifier_set_last_error.argtypes = [vp]
    lib.act_nullifier_set_last_error.restype = C.c_char_p
    lib.act_nullifier_check_and_insert_batch.argtypes = [vp, sz, i32, u8p, sz, u8p, u8p]
    lib.act_nullifier_set_reserve.argtypes = [vp, sz]
    lib.act_nullifier_set_export.argtypes = [vp, C.POINTER(C.c_uint64), sz, i32, u8p, C.POINTER(C.c_size_t)]
    lib.act_nullifier_contains_batch.argtypes = [vp, sz, i32, u8p, sz, u8p]
    lib.act_prof_enable.argtypes = [vp, i32]
    lib.act_prof_reset.argtypes = [vp]
    lib.act_prof_kernel_count.argtypes = [vp]
    lib.act_prof_kernel_name.argtypes = [vp, i32]
    lib.act_prof_kernel_name.restype = C.c_char_p
    lib.act_prof_get.argtypes = [vp, i32, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.act_prof_get_busy.argtypes = [vp, i32, C.POINTER(C.c_double)]
    lib.act_ubench_mad_u64_u32.argtypes = [i32, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.act_ubench_random_read.argtypes = [i32, sz, i32, i32, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.act_ubench_table_read.argtypes = [vp, i32, i32, i32, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.act_issue_check_batch.argtypes = [vp, sz, i32, u8p, u8p]
    lib.act_issue_sign_batch.argtypes = [vp, sz, i32, u8p, u8p, u8p, u8p, u8p, i32, u8p, u8p]
    lib.act_refund_sign_batch.argtypes = [vp, sz, i32, u8p, u8p, u8p, u8p, i32, u8p, u8p]
    lib.act_node_create.argtypes = [u8p, i32, C.POINTER(C.c_int), i32, sz, C.POINTER(vp)]
    lib.act_node_destroy.argtypes = [vp]
    lib.act_node_destroy.restype = None
    lib.act_node_device_count.argtypes = [vp]
    lib.act_node_ctx.argtypes = [vp, i32]
    lib.act_node_ctx.restype = vp
    lib.act_node_last_error.argtypes = [vp]
    lib.act_node_last_error.restype = C.c_char_p
    lib.act_node_set_transcript_mode.argtypes = [vp, i32]
    lib.act_node_set_host_threads.argtypes = [vp, i32]
    lib.act_node_request_batch.argtypes = [vp, sz, u8p, u8p, u8p]
    lib.act_node_issue_batch.argtypes = [vp, sz, u8p, u8p, u8p, u8p, i32, u8p, u8p]
    lib.act_node_issuance_to_credit_token_batch.argtypes = [vp, sz, u8p, u8p, u8p, u8p, u8p, u8p]
    lib.act_node_prove_spend_batch.argtypes = [vp, sz, u8p, u8p, u8p, u8p, u8p, u8p]
    lib.act_node_verify_spend_batch.argtypes = [vp, sz, u8p, u8p, u8p, u8p]
    lib.act_node_refund_batch.argtypes = [vp, sz, u8p, u8p, u8p, i32, u8p, u8p]
    lib.act_node_refund_to_credit_token_batch.argtypes = [vp, sz, u8p, u8p, u8p, u8p, u8p, u8p]
    lib.act_node_issue_check_batch.argtypes = [vp, sz, u8p, u8p]
    lib.act_node_issue_sign_batch.argtypes = [vp, sz, u8p, u8p, u8p, u8p, u8p, i32, u8p, u8p]
    lib.act_node_refund_sign_batch.argtypes = [vp, sz, u8p, u8p, u8p, u8p, i32, u8p, u8p]
    lib.act_node_nullifier_set_create.argtypes = [C.POINTER(C.c_int), i32, sz, u8p, C.POINTER(vp)]
    lib.act_node_nullifier_set_destroy.argtypes = [vp]
    lib.act_node_nullifier_set_destroy.restype = None
    lib.act_node_nullifier_set_len.argtypes = [vp]
    lib.act_node_nullifier_set_len.restype = sz
    lib.act_node_nullifier_set_last_error.argtypes = [vp]
    lib.act_node_nullifier_set_last_error.restype = C.c_char_p
    lib.act_node_nullifier_check_and_insert_batch.argtypes = [vp, sz, u8p, sz, u8p, u8p]
    lib.act_node_nullifier_set_reserve.argtypes = [vp, sz]
    lib.act_node_nullifier_set_export.argtypes = [vp, C.POINTER(C.c_uint64), sz, u8p, C.POINTER(C.c_size_t)]
    lib.act_node_nullifier_contains_batch.argtypes = [vp, sz, u8p, sz, u8p]
    lib.act_verify_spend_cbor_keys_batch.argtypes = [vp, sz, i32, u8p, u8p, vp, u8p, u8p, u8p]
    lib.act_node_verify_spend_cbor_keys_batch.argtypes = [vp, sz, u8p, u8p, vp, u8p, u8p, u8p]
    lib.act_refund_sign_cbor_batch.argtypes = [vp, sz, i32, u8p, u8p, u8p, u8p, i32, u8p, u8p]
    lib.act_refund_cbor_batch.argtypes = [vp, sz, i32, u8p, u8p, vp, u8p, i32, u8p, u8p]
    lib.act_refund_cbor_keys_batch.argtypes = [vp, sz, i32, u8p, u8p, vp, u8p, i32, u8p, u8p, u8p]
    lib.act_node_refund_sign_cbor_batch.argtypes = [vp, sz, u8p, u8p, u8p, u8p, i32, u8p, u8p]
    lib.act_node_refund_cbor_batch.argtypes = [vp, sz, u8p, u8p, vp, u8p, i32, u8p, u8p]
    lib.act_redeem_cbor_batch.argtypes = [vp, vp, sz, i32, u8p, u8p, vp, u8p, i32, u8p, u8p]
    # key rotation: a ring of issuer keys (keys = nkeys x 64 bytes)
    lib.act_verify_spend_keyring_batch.argtypes = [vp, sz, i32, u8p, i32, u8p, u8p, u8p, u8p]
    lib.act_refund_sign_keyring_batch.argtypes = [vp, sz, i32, u8p, i32, u8p, u8p, u8p, u8p, i32, u8p, u8p]
    lib.act_redeem_keyring_batch.argtypes = [vp, vp, sz, i32, u8p, i32, i32, u8p, u8p, i32, u8p, u8p, u8p]
    lib.act_redeem_cbor_keyring_batch.argtypes = [vp, vp, sz, i32, u8p, i32, i32, u8p, vp, u8p, i32, u8p, u8p, u8p]
    lib.act_node_verify_spend_keyring_batch.argtypes = [vp, sz, u8p, i32, u8p, u8p, u8p, u8p]
    lib.act_node_refund_sign_keyring_batch.argtypes = [vp, sz, u8p, i32, u8p, u8p, u8p, u8p, i32, u8p, u8p]
    lib.act_node_redeem_keyring_batch.argtypes = [vp, vp, sz, u8p, i32, i32, u8p, u8p, i32, u8p, u8p, u8p]
    lib.act_node_redeem_cbor_keyring_batch.argtypes = [vp, vp, sz, u8p, i32, i32, u8p, vp, u8p, i32, u8p, u8p, u8p]
    u32p, u64p, szp = C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_size_t)
    lib.act_nullifier_check_and_insert_epoch_batch.argtypes = [vp, sz, i32, u8p, sz, u8p, u8p, u32p, i32, u8p]
    lib.act_nullifier_set_epoch_len.argtypes = [vp, C.c_uint32, u64p]
    lib.act_nullifier_set_retire_epoch.argtypes = [vp, C.c_uint32, u64p]
    lib.act_nullifier_set_retired_epochs.argtypes = [vp, u32p, sz, szp]
    lib.act_nullifier_set_export_epochs.argtypes = [vp, u64p, sz, i32, u8p, vp, szp]
    lib.act_redeem_keyring_epochs_batch.argtypes = [vp, vp, sz, i32, u8p, i32, u32p, i32, u8p, u8p, i32, u8p, u8p, u8p]
    lib.act_redeem_cbor_keyring_epochs_batch.argtypes = [vp, vp, sz, i32, u8p, i32, u32p, i32, u8p, vp, u8p, i32, u8p, u8p, u8p]
    lib.act_node_nullifier_check_and_insert_epoch_batch.argtypes = [vp, sz, u8p, sz, u8p, u8p, u32p, i32, u8p]
    lib.act_node_nullifier_set_epoch_len.argtypes = [vp, C.c_uint32, u64p]
    lib.act_node_nullifier_set_retire_epoch.argtypes = [vp, C.c_uint32, u64p]
    lib.act_node_nullifier_set_retired_epochs.argtypes = [vp, u32p, sz, szp]
    lib.act_node_nullifier_set_export_epochs.argtypes = [vp, u64p, sz, u8p, vp, szp]
    lib.act_node_redeem_keyring_epochs_batch.argtypes = [vp, vp, sz, u8p, i32, u32p, i32, u8p, u8p, i32, u8p, u8p, u8p]
    lib.act_node_redeem_cbor_keyring_epochs_batch.argtypes = [vp, vp, sz, u8p, i32, u32p, i32, u8p, vp, u8p, i32, u8p, u8p, u8p]
    lib.act_node_redeem_cbor_batch.argtypes = [vp, vp, sz, u8p, u8p, vp, u8p, i32, u8p, u8p]
    # admission before verification: the expected charge and the spent nullifiers first (out_counts: ACT_ADMIT_COUNTS values, host)
    lib.act_redeem_admit_batch.argtypes = [vp, vp, sz, i32, u8p, i32, u32p, i32, u8p, u8p, u8p, i32, u8p, u8p, u8p, u64p]
    lib.act_redeem_cbor_admit_batch.argtypes = [vp, vp, sz, i32, u8p, i32, u32p, i32, u8p, vp, u8p, u8p, i32, u8p, u8p, u8p, u64p]
    # the unique forms: byte-identical proofs of one batch are verified once (out_counts: ACT_ADMIT_UNIQUE_COUNTS values)
    lib.act_redeem_admit_unique_batch.argtypes = lib.act_redeem_admit_batch.argtypes
    lib.act_redeem_cbor_admit_unique_batch.argtypes = lib.act_redeem_cbor_admit_batch.argtypes
    lib.act_debug_copy_leaders.argtypes = [vp, sz, u64p, vp, C.POINTER(C.c_double)]
    # replayable redemption: derived nonces and a receipts set (out_counts: ACT_REPLAY_COUNTS values, host)
    lib.act_redeem_replay_batch.argtypes = [vp, vp, vp, sz, i32, u8p, i32, u32p, i32, u8p, u8p, u8p, u8p, u8p, u8p, u64p]
    lib.act_redeem_cbor_replay_batch.argtypes = [vp, vp, vp, sz, i32, u8p, i32, u32p, i32, u8p, vp, u8p, u8p, u8p, u8p, u8p, u64p]
    lib.act_replay_derive_batch.argtypes = [vp, sz, i32, u8p, i32, u8p, u8p, u8p, sz, u8p, u8p, u8p, u8p]
    # its admission form: the screen asks the receipts before anything is verified (out_counts: ACT_ADMIT_REPLAY_COUNTS values, host)
    lib.act_redeem_admit_replay_batch.argtypes = [vp, vp, vp, sz, i32, u8p, i32, u32p, i32, u8p, u8p, u8p, u8p, u8p, u8p, u8p, u64p]
    lib.act_redeem_cbor_admit_replay_batch.argtypes = [vp, vp, vp, sz, i32, u8p, i32, u32p, i32, u8p, vp, u8p, u8p, u8p, u8p, u8p, u8p, u64p]
    # its unique forms: byte-identical proofs of one batch are verified and signed once (out_counts: ACT_ADMIT_REPLAY_UNIQUE_COUNTS values)
    lib.act_redeem_admit_replay_unique_batch.argtypes = lib.act_redeem_admit_replay_batch.argtypes
    lib.act_redeem_cbor_admit_replay_unique_batch.argtypes = lib.act_redeem_cbor_admit_replay_batch.argtypes
    # partial refunds: the admission calls with the returned amounts t (out_counts: ACT_REDEEM_RETURN_COUNTS values), the sign-only call, the client's
    lib.act_refund_sign_return_keyring_batch.argtypes = [vp, sz, i32, u8p, i32, u8p, u8p, u8p, u8p, i32, u8p, u8p, u8p]
    lib.act_redeem_return_batch.argtypes = [vp, vp, sz, i32, u8p, i32, u32p, i32, u8p, u8p, u8p, u8p, i32, u8p, u8p, u8p, u64p]
    lib.act_redeem_cbor_return_batch.argtypes = [vp, vp, sz, i32, u8p, i32, u32p, i32, u8p, vp, u8p, u8p, u8p, i32, u8p, u8p, u8p, u64p]
    lib.act_refund_to_credit_token_return_batch.argtypes = [vp, sz, i32, u8p, u8p, u8p, u8p, u8p, u8p]
    # ... against a ring of public keys, and the return calls' unique forms (out_counts: ACT_REDEEM_RETURN_UNIQUE_COUNTS values)
    lib.act_refund_to_credit_token_return_keyring_batch.argtypes = lib.act_refund_to_credit_token_keyring_batch.argtypes
    lib.act_redeem_return_unique_batch.argtypes = lib.act_redeem_return_batch.argtypes
    lib.act_redeem_cbor_return_unique_batch.argtypes = lib.act_redeem_cbor_return_batch.argtypes
    # replayable partial refunds: the admission replay calls with `returned` behind `charge` (out_counts: ACT_RETURN_REPLAY_COUNTS values)
    lib.act_redeem_return_replay_batch.argtypes = [vp, vp, vp, sz, i32, u8p, i32, u32p, i32, u8p, u8p, u8p, u8p, u8p, u8p, u8p, u8p, u64p]
    lib.act_redeem_cbor_return_replay_batch.argtypes = [vp, vp, vp, sz, i32, u8p, i32, u32p, i32, u8p, vp, u8p, u8p, u8p, u8p, u8p, u8p, u8p, u64p]
    # their unique forms: a copy is served only if it names its leader's amount (out_counts: ACT_RETURN_REPLAY_UNIQUE_COUNTS values)
    lib.act_redeem_return_replay_unique_batch.argtypes = lib.act_redeem_return_replay_batch.argtypes
    lib.act_redeem_cbor_return_replay_unique_batch.argtypes = lib.act_redeem_cbor_return_replay_batch.argtypes
    # reserve and settle: the admit-replay call without sign_key / nonce_key, 96-byte reservation records out (ACT_RESERVE_COUNTS values);
    # reservation records, key indices and amounts in, RefundReturn records or messages out (ACT_SETTLE_COUNTS values)
    lib.act_redeem_reserve_batch.argtypes = [vp, vp, vp, sz, i32, u8p, i32, u32p, u8p, u8p, u8p, u8p, u8p, u8p, u64p]
    lib.act_redeem_cbor_reserve_batch.argtypes = [vp, vp, vp, sz, i32, u8p, i32, u32p, u8p, vp, u8p, u8p, u8p, u8p, u8p, u64p]
    # request binding: the signature of the call each extends, with bind directly behind the proof or message arguments
    lib.act_prove_spend_bound_batch.argtypes = [vp, sz, i32, u8p, u8p, u8p, u8p, u8p, u8p, u8p]
    lib.act_verify_spend_keyring_bound_batch.argtypes = [vp, sz, i32, u8p, i32, u8p, u8p, u8p, u8p, u8p]
    lib.act_redeem_return_replay_bound_batch.argtypes = [vp, vp, vp, sz, i32, u8p, i32, u32p, i32, u8p, u8p, u8p, u8p, u8p, u8p, u8p, u8p, u8p, u64p]
    lib.act_redeem_cbor_return_replay_bound_batch.argtypes = [vp, vp, vp, sz, i32, u8p, i32, u32p, i32, u8p, vp, u8p, u8p, u8p, u8p, u8p, u8p, u8p, u8p, u64p]
    lib.act_redeem_reserve_bound_batch.argtypes = [vp, vp, vp, sz, i32, u8p, i32, u32p, u8p, u8p, u8p, u8p, u8p, u8p, u8p, u64p]
    lib.act_redeem_cbor_reserve_bound_batch.argtypes = [vp, vp, vp, sz, i32, u8p, i32, u32p, u8p, vp, u8p, u8p, u8p, u8p, u8p, u8p, u64p]
    lib.act_redeem_settle_batch.argtypes = [vp, vp, sz, i32, u8p, i32, u32p, i32, u8p, u8p, u8p, u8p, u8p, u8p, u8p, u64p]
    lib.act_redeem_cbor_settle_batch.argtypes = lib.act_redeem_settle_batch.argtypes
    lib.act_replay_derive_return_batch.argtypes = [vp, sz, i32, u8p, i32, u8p, u8p, u8p, sz, u8p, u8p, u8p, u8p, u8p]
    lib.act_issue_check_cbor_batch.argtypes = [vp, sz, i32, u8p, vp, u8p, u8p]
    lib.act_issue_sign_cbor_batch.argtypes = [vp, sz, i32, u8p, u8p, u8p, u8p, u8p, i32, u8p, u8p]
    lib.act_issue_cbor_batch.argtypes = [vp, sz, i32, u8p, u8p, vp, u8p, u8p, i32, u8p, u8p]
    lib.act_node_issue_check_cbor_batch.argtypes = [vp, sz, u8p, vp, u8p, u8p]
    lib.act_node_issue_sign_cbor_batch.argtypes = [vp, sz, u8p, u8p, u8p, u8p, u8p, i32, u8p, u8p]
    lib.act_node_issue_cbor_batch.argtypes = [vp, sz, u8p, u8p, vp, u8p, u8p, i32, u8p, u8p]
    lib.act_ctx_host_hash_stats.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint64), i32]
    lib.act_ctx_set_tiny_calls.argtypes = [vp, i32]
    lib.act_node_set_balance.argtypes = [vp, i32, i32]
    lib.act_node_device_stats.argtypes = [vp, i32, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    lib.act_node_balance_state.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.act_debug_set_slowdown.argtypes = [vp, C.c_uint32]
    lib.act_debug_fail_next_signs.argtypes = [vp, i32]
    _lib = lib
    forward_tuning_env(lib)
    return lib


# The library reads no ACT_* tuning variable itself (act_tuning_set is the only way in): tools/, tests/ and bench.py keep their
# environment-variable interface HERE, in the binding they all go through.  ACT_<NAME>=v -> act_tuning_set("<name>", v).
TUNING_ENV = ("NO_MAPPED_READS", "NO_STREAM_PROBE", "NO_FUSED_TINY", "NO_TAPER", "NO_WIDE_CLIENT", "NO_WIDE_PROVE", "NO_WIDE_SIGN", "NO_LDS_ISOLATION",
              "SMALL_NORMAL_PRIO", "SMALL_TRACE", "SMALL_IN_FLIGHT", "SMALL_SUB", "STAGGER", "HARD_STAGGER", "HOST_CHUNK", "CBOR_CHUNK_MSGS", "UBENCH_ITERS")


def forward_tuning_env(lib=None):
    """(also callable later: a test that changes ACT_CBOR_CHUNK_MSGS between calls re-forwards)"""
    lib = lib or load()
    defaults = {"STAGGER": -1, "SMALL_IN_FLIGHT": 2}
    for name in TUNING_ENV:
        v = os.environ.get("ACT_" + name)
        try:
            val = defaults.get(name, 0) if v is None else (int(v) if v.strip() else 1)
        except ValueError:
            val = 1
        lib.act_tuning_set(name.lower().encode(), val)


RNG_DRAW_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)


def rng_trampoline(fill):
    """act_rng_draw_fn around `fill(n) -> n bytes`.  ctypes swallows an exception raised inside a callback (it prints it and returns
    garbage), so the trampoline catches everything itself, checks the length, and reports failure as the ABI says: non-zero -- the
    library then signs nothing (ACT_ERR_RNG).  The exception is kept in `.error` of the returned callback's holder list."""
    err = []

    def draw(_ctx, dst, n):
        try:
            data = fill(n)
            if len(data) != n:
                raise ValueError("generator returned %d bytes, %d asked" % (len(data), n))
            C.memmove(dst, bytes(data), n)
            return 0
        except BaseException as e:      # noqa: BLE001 -- nothing may propagate into C
            err.append(e)
            return 1
    cb = RNG_DRAW_FN(draw)
    cb.errors = err
    return cb


class RngSource(C.Structure):
    """act_rng_source (ACT_RNG_CALLBACK): the library draws 128 bytes per SIGNED lane through `draw`, once, after the verdicts."""
    _fields_ = [("draw", RNG_DRAW_FN), ("rng_ctx", C.c_void_p)]


class ReplayRng:
    """A generator that hands out a fixed byte string (what tests/parity.rs feeds the crate); `pos` = bytes consumed so far."""

    def __init__(self, data: bytes):
        self.data, self.pos, self.draws = bytes(data), 0, []

        def fill(n):
            if self.pos + n > len(self.data):
                raise ValueError("generator exhausted")
            out = self.data[self.pos:self.pos + n]
            self.pos += n
            self.draws.append(n)
            return out
        self._cb = rng_trampoline(fill)
        self.source = RngSource(self._cb, None)

    @property
    def ptr(self):
        return C.addressof(self.source)


def _msgs(messages):
    """list of byte strings -> (blob pointer, keep-alive, offsets array)"""
    n = len(messages)
    offs = np.zeros(n + 1, np.uint64); offs[1:] = np.cumsum([len(m) for m in messages], dtype=np.uint64)
    p, keep = _in(b"".join(messages) + b"\0")
    return p, keep, offs


def _rng_arg(rng):
    """bytes -> pointer; ReplayRng -> pointer to its act_rng_source (rng_mode must then be RNG_CALLBACK)"""
    if isinstance(rng, ReplayRng):
        return rng.ptr, rng
    return _in(rng)


def _in(x, nbytes=None):
    """bytes / numpy uint8 -> (ctypes pointer value, keep-alive object)."""
    if x is None:
        return None, None
    a = np.frombuffer(x, dtype=np.uint8) if isinstance(x, (bytes, bytearray, memoryview)) else np.ascontiguousarray(x, dtype=np.uint8)
    if nbytes is not None and a.size != nbytes:
        raise ValueError(f"expected {nbytes} bytes, got {a.size}")
    return a.ctypes.data, a


def params_new(org: str, svc: str, dep: str, ver: str, device: int = 0) -> bytes:
    out = np.zeros(96, np.uint8)
    rc = load().act_params_new(device, org.encode(), svc.encode(), dep.encode(), ver.encode(), out.ctypes.data)
    if rc:
        raise ActError(f"act_params_new failed: {_ERRS.get(rc, rc)}")
    return out.tobytes()


def params_random(rng: bytes, device: int = 0) -> bytes:
    out = np.zeros(96, np.uint8)
    p, keep = _in(rng, 192)
    rc = load().act_params_random(device, p, out.ctypes.data)
    if rc:
        raise ActError(f"act_params_random failed: {_ERRS.get(rc, rc)}")
    return out.tobytes()


def host_usable_cpus() -> int:
    return load().act_host_usable_cpus()


def host_pool_stats() -> dict:
    j, t, n = C.c_uint64(0), C.c_uint64(0), C.c_int(0)
    load().act_host_pool_stats(C.byref(j), C.byref(t), C.byref(n))
    return {"jobs": j.value, "threads_created": t.value, "pool_size": n.value}


def host_hash_many(msgs, stride: int, length: int, n: int, max_threads: int = 0) -> bytes:
    """BLAKE3 XOF (64 B) of n messages at `stride` through the process-wide worker pool (pure host code)."""
    out = np.zeros(64 * n, np.uint8)
    p, keep = _in(msgs)
    load().act_host_hash_many(p, stride, length, n, max_threads, out.ctypes.data)
    return out.tobytes()


def ubench_mad(device: int = 0):
    """(lane-MADs per second, probe ms) of the v_mad_u64_u32 roofline probe."""
    r, ms = C.c_double(0), C.c_double(0)
    rc = load().act_ubench_mad_u64_u32(device, C.byref(r), C.byref(ms))
    if rc:
        raise ActError(f"act_ubench_mad_u64_u32 failed: {_ERRS.get(rc, rc)}")
    return r.value, ms.value


def ubench_random_read(device: int = 0, gib: int = 0, waves_per_simd: int = 0, in_flight: int = 0):
    """(GB/s of 128-byte random reads, probe ms): the memory-side roofline of the scalar-addressed fixed-base tables."""
    r, ms = C.c_double(0), C.c_double(0)
    rc = load().act_ubench_random_read(device, gib, waves_per_simd, in_flight, C.byref(r), C.byref(ms))
    if rc:
        raise ActError(f"act_ubench_random_read failed: {_ERRS.get(rc, rc)}")
    return r.value, ms.value


class Engine:
    """One context: Params (enc(h1)|enc(h2)|enc(h3)) + range width L + one GPU.
    Host-memory methods take/return bytes; the *_dev methods take raw device pointers (ints)."""

    def __init__(self, h: bytes, L: int = 128, device: int = 0, max_batch: int = 0,
                 transcript: int = TRANSCRIPT_HOST, host_threads: int = 0):
        self.lib = load()
        self.h, self.L, self.device = bytes(h), L, device
        ctx = C.c_void_p()
        p, keep = _in(h, 96)
        rc = self.lib.act_ctx_create(p, L, device, max_batch, C.byref(ctx))
        if rc:
            msg = self.lib.act_last_error(ctx).decode() if ctx else ""
            if ctx:
                self.lib.act_ctx_destroy(ctx)
            raise ActError(f"act_ctx_create failed: {_ERRS.get(rc, rc)} {msg}")
        self.ctx = ctx
        forward_tuning_env(self.lib)       # ACT_* measurement knobs as they stand now (tests change them between engines)
        wide = os.environ.get("ACT_FB_WIDE_BITS")          # tools' A/B interface of rounds 3-5; the library itself no longer looks
        if wide and wide.isdigit() and int(wide) != 16:
            for b in ((0, 1, 2, 3) if os.environ.get("ACT_FB_ALL_WIDE") else (1, 3)):
                self.lib.act_ctx_set_fixed_base_bits(ctx, b, int(wide))
        self.proof_bytes = self.lib.act_spend_proof_bytes(ctx)
        self.prove_rng_bytes = self.lib.act_prove_rng_bytes(ctx)
        self.transcript_bytes = self.lib.act_spend_transcript_bytes(ctx)
        self.set_transcript_mode(transcript)
        if host_threads:
            self._ck(self.lib.act_ctx_set_host_threads(ctx, host_threads))

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.act_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc:
            raise ActError(f"{_ERRS.get(rc, rc)}: {self.lib.act_last_error(self.ctx).decode()}")

    def set_transcript_mode(self, mode: int):
        self._ck(self.lib.act_ctx_set_transcript_mode(self.ctx, mode))

    def fixed_base_bits(self):
        """Window widths of the g, h1, h2, h3 tables of this context."""
        return [self.lib.act_ctx_fixed_base_bits(self.ctx, b) for b in range(4)]

    def set_pipeline_depth(self, depth: int):
        self._ck(self.lib.act_ctx_set_pipeline_depth(self.ctx, depth))

    def set_host_threads(self, n: int):
        self._ck(self.lib.act_ctx_set_host_threads(self.ctx, n))

    def ubench_table_read(self, base: int, waves_per_simd: int = 0, in_flight: int = 0):
        """(GB/s, ms) of random 128-byte reads over this context's own table of base 0..3 (g, h1, h2, h3)."""
        r, ms = C.c_double(0), C.c_double(0)
        self._ck(self.lib.act_ubench_table_read(self.ctx, base, waves_per_simd, in_flight, C.byref(r), C.byref(ms)))
        return r.value, ms.value

    def set_fixed_base_bits(self, base: int, bits: int):
        """Window width of the table of base 0..3 (g, h1, h2, h3); act_ctx_create leaves all four at 16 bits."""
        self._ck(self.lib.act_ctx_set_fixed_base_bits(self.ctx, base, bits))

    def set_wide_range_tables(self, bits: int = 24) -> bool:
        """24-bit windows for h1 and h3, the range kernel's bases (+47 GB, +3 % verifies/s): what a GPU that serves nothing else asks
        for.  Returns False (tables unchanged) when the device has not the room."""
        try:
            self.set_fixed_base_bits(1, bits); self.set_fixed_base_bits(3, bits)
            return True
        except ActError:
            for b in (1, 3):
                if self.lib.act_ctx_fixed_base_bits(self.ctx, b) != 16:
                    self.lib.act_ctx_set_fixed_base_bits(self.ctx, b, 16)
            return False

    def set_small_batch_max(self, n: int):
        """Calls of at most n proofs take the small-batch (latency) schedule; 0 = never."""
        self._ck(self.lib.act_ctx_set_small_batch_max(self.ctx, n))

    def streams_overlap(self) -> int:
        """1 = the two pipeline streams run side by side, 0 = they share a hardware queue, -1 = not measured."""
        return self.lib.act_ctx_streams_overlap(self.ctx)

    # ---- host-memory batch calls ----------------------------------------------------------------
    def private_key_random(self, rng: bytes) -> bytes:
        out = np.zeros(64, np.uint8); p, k = _in(rng, 64)
        self._ck(self.lib.act_private_key_random(self.ctx, p, out.ctypes.data)); return out.tobytes()

    def pre_issuance_random(self, rng: bytes) -> bytes:
        n = len(rng) // 128; out = np.zeros(64 * n, np.uint8); p, k = _in(rng, 128 * n)
        self._ck(self.lib.act_pre_issuance_random_batch(self.ctx, n, MEM_HOST, p, out.ctypes.data)); return out.tobytes()

    def request(self, pre: bytes, rng: bytes) -> bytes:
        n = len(pre) // 64; out = np.zeros(128 * n, np.uint8)
        p0, k0 = _in(pre, 64 * n); p1, k1 = _in(rng, 128 * n)
        self._ck(self.lib.act_request_batch(self.ctx, n, MEM_HOST, p0, p1, out.ctypes.data)); return out.tobytes()

    def issue(self, sk: bytes, req: bytes, c: bytes, rng: bytes, rng_mode: int = RNG_PER_LANE):
        n = len(req) // 128; out = np.zeros(160 * n, np.uint8); st = np.zeros(n, np.uint8)
        ps, ks = _in(sk, 64); p0, k0 = _in(req, 128 * n); p1, k1 = _in(c, 32 * n); p2, k2 = _in(rng)
        self._ck(self.lib.act_issue_batch(self.ctx, n, MEM_HOST, ps, p0, p1, p2, rng_mode, out.ctypes.data, st.ctypes.data))
        return st.tobytes(), out.tobytes()

    def issuance_to_credit_token(self, pre: bytes, w: bytes, req: bytes, resp: bytes):
        n = len(pre) // 64; out = np.zeros(160 * n, np.uint8); st = np.zeros(n, np.uint8)
        p0, k0 = _in(pre, 64 * n); pw, kw = _in(w, 32); p1, k1 = _in(req, 128 * n); p2, k2 = _in(resp, 160 * n)
        self._ck(self.lib.act_issuance_to_credit_token_batch(self.ctx, n, MEM_HOST, p0, pw, p1, p2, out.ctypes.data, st.ctypes.data))
        return st.tobytes(), out.tobytes()

    def prove_spend(self, tok: bytes, s: bytes, rng: bytes, bind=_UNBOUND):
        """bind given (32 bytes a lane, or None: NULL): act_prove_spend_bound_batch -- the bytes enter each proof's challenge hash"""
        n = len(tok) // 160; out = np.zeros(self.proof_bytes * n, np.uint8); pr = np.zeros(96 * n, np.uint8); st = np.zeros(n, np.uint8)
        p0, k0 = _in(tok, 160 * n); p1, k1 = _in(s, 32 * n); p2, k2 = _in(rng, self.prove_rng_bytes * n)
        if bind is _UNBOUND:
            self._ck(self.lib.act_prove_spend_batch(self.ctx, n, MEM_HOST, p0, p1, p2, out.ctypes.data, pr.ctypes.data, st.ctypes.data))
        else:
            pb, kb = _in(bind, 32 * n) if bind is not None else (None, None)
            self._ck(self.lib.act_prove_spend_bound_batch(self.ctx, n, MEM_HOST, p0, p1, p2, pb, out.ctypes.data, pr.ctypes.data, st.ctypes.data))
        return st.tobytes(), out.tobytes(), pr.tobytes()

    def prove_spend_seeded(self, tok: bytes, s: bytes, seed: bytes, first_lane: int = 0):
        """prove_spend with lane i's rng = BLAKE3-XOF(seed | u64_le(first_lane + i)), expanded on the device."""
        n = len(tok) // 160; out = np.zeros(self.proof_bytes * n, np.uint8); pr = np.zeros(96 * n, np.uint8); st = np.zeros(n, np.uint8)
        p0, k0 = _in(tok, 160 * n); p1, k1 = _in(s, 32 * n); p2, k2 = _in(seed, 32)
        self._ck(self.lib.act_prove_spend_seeded_batch(self.ctx, n, MEM_HOST, p0, p1, p2, first_lane, out.ctypes.data, pr.ctypes.data, st.ctypes.data))
        return st.tobytes(), out.tobytes(), pr.tobytes()

    def verify_spend(self, sk: bytes, proofs: bytes, want_kprime: bool = False):
        n = len(proofs) // self.proof_bytes; st = np.zeros(n, np.uint8)
        kp = np.zeros(32 * n, np.uint8) if want_kprime else None
        ps, ks = _in(sk, 64); p0, k0 = _in(proofs, self.proof_bytes * n)
        self._ck(self.lib.act_verify_spend_batch(self.ctx, n, MEM_HOST, ps, p0, st.ctypes.data, kp.ctypes.data if want_kprime else None))
        return (st.tobytes(), kp.tobytes()) if want_kprime else st.tobytes()

    def refund(self, sk: bytes, proofs: bytes, rng: bytes, rng_mode: int = RNG_PER_LANE):
        n = len(proofs) // self.proof_bytes; out = np.zeros(128 * n, np.uint8); st = np.zeros(n, np.uint8)
        ps, ks = _in(sk, 64); p0, k0 = _in(proofs, self.proof_bytes * n); p1, k1 = _in(rng)
        self._ck(self.lib.act_refund_batch(self.ctx, n, MEM_HOST, ps, p0, p1, rng_mode, out.ctypes.data, st.ctypes.data))
        return st.tobytes(), out.tobytes()

    def refund_to_credit_token(self, prerefund: bytes, proofs: bytes, refund: bytes, w: bytes):
        n = len(prerefund) // 96; out = np.zeros(160 * n, np.uint8); st = np.zeros(n, np.uint8)
        p0, k0 = _in(prerefund, 96 * n); p1, k1 = _in(proofs, self.proof_bytes * n); p2, k2 = _in(refund, 128 * n); pw, kw = _in(w, 32)
        self._ck(self.lib.act_refund_to_credit_token_batch(self.ctx, n, MEM_HOST, p0, p1, p2, pw, out.ctypes.data, st.ctypes.data))
        return st.tobytes(), out.tobytes()

    def last_spend_transcripts(self, max_lanes: int) -> list:
        out = np.zeros(max_lanes * self.transcript_bytes, np.uint8); n = C.c_size_t(0)
        self._ck(self.lib.act_debug_last_spend_transcripts(self.ctx, max_lanes, out.ctypes.data, C.byref(n)))
        b = out.tobytes()
        return [b[i * self.transcript_bytes:(i + 1) * self.transcript_bytes] for i in range(n.value)]

    def secret_residue(self) -> int:
        n = C.c_size_t(0)
        self._ck(self.lib.act_debug_secret_residue(self.ctx, C.byref(n))); return n.value

    def debug_scalarmult(self, points: bytes, scalars: bytes):
        n = len(points) // 32; out = np.zeros(32 * n, np.uint8); st = np.zeros(n, np.uint8)
        p0, k0 = _in(points, 32 * n); p1, k1 = _in(scalars, 32 * n)
        self._ck(self.lib.act_debug_scalarmult_batch(self.ctx, n, MEM_HOST, p0, p1, out.ctypes.data, st.ctypes.data))
        return st.tobytes(), out.tobytes()

    def debug_fixed_base(self, base: int, scalars: bytes) -> bytes:
        """enc(s_i * B) for the fixed base 0..3 (g, h1, h2, h3) through this context's table of B at its current window width."""
        n = len(scalars) // 32; out = np.zeros(32 * n, np.uint8)
        p0, k0 = _in(scalars, 32 * n)
        self._ck(self.lib.act_debug_fixed_base_batch(self.ctx, base, n, MEM_HOST, p0, out.ctypes.data))
        return out.tobytes()

    def debug_fixed_base_mf(self, base: int, scalars: bytes, block_threads: int = 64, out_lanes: int = 0, fill: int = 0) -> bytes:
        """enc(s_i * B) for the fixed base 0..3 through the product of secret scalars (act_debug_fixed_base_mf_batch: the matrix-core
        look-up over this context's table image), in blocks of 64 or 256 threads.  The result holds max(n, out_lanes) records, pre-filled
        with `fill`: what lies past record n must come back as it went in."""
        n = len(scalars) // 32; out = np.full(32 * max(n, out_lanes), fill, np.uint8)
        p0, k0 = _in(scalars, 32 * n)
        self._ck(self.lib.act_debug_fixed_base_mf_batch(self.ctx, base, block_threads, n, MEM_HOST, p0, out.ctypes.data))
        return out.tobytes()

    def debug_chain_ct(self, mode: int, points: bytes, scalars: bytes, scalars2: bytes = None):
        """The address-free chains, one per lane (act_debug_chain_ct_batch): mode 0 chain_ct<1>, 1 the four chain_ct_quarter pieces
        added, 2 chain_ct<2> with (scalars, scalars2).  Returns (status, out), in mode 2 (status, out, out2)."""
        n = len(points) // 32; out = np.zeros(32 * n, np.uint8); st = np.zeros(n, np.uint8)
        out2 = np.zeros(32 * n, np.uint8) if scalars2 is not None else None
        p0, k0 = _in(points, 32 * n); p1, k1 = _in(scalars, 32 * n); p2, k2 = _in(scalars2, 32 * n)
        self._ck(self.lib.act_debug_chain_ct_batch(self.ctx, mode, n, MEM_HOST, p0, p1, p2, out.ctypes.data, None if out2 is None else out2.ctypes.data, st.ctypes.data))
        return (st.tobytes(), out.tobytes()) if out2 is None else (st.tobytes(), out.tobytes(), out2.tobytes())

    FE_OPS = ("mul", "sq", "mul2", "sq2", "sqda_sq", "carry", "sub", "sub3", "sub4", "neg")

    def debug_fe(self, pair_build: bool, op: str, n: int, f, g=None, fb=None, gb_or_a=None, fill: int = 0):
        """One field operation per lane on raw limbs (act_debug_fe_batch).  f, g, fb, gb_or_a: uint32 arrays of 9 n limbs (those the
        operation names).  Returns (h, hb) as uint32 arrays of 9 * (n rounded up to 256) limbs pre-filled with `fill`; hb is None for
        the operations with one result."""
        lanes = (n + 255) // 256 * 256
        two = op in ("mul2", "sq2", "sqda_sq")
        ins = [None if a is None else np.ascontiguousarray(a, np.uint32) for a in (f, g, fb, gb_or_a)]
        assert all(a is None or a.size == 9 * n for a in ins)
        h = np.full(9 * lanes, fill, np.uint32); hb = np.full(9 * lanes, fill, np.uint32) if two else None
        self._ck(self.lib.act_debug_fe_batch(self.ctx, int(bool(pair_build)), self.FE_OPS.index(op), n, *[None if a is None else a.ctypes.data for a in ins],
                                             h.ctypes.data, None if hb is None else hb.ctypes.data))
        return h, hb

    SC_OPS = ("load_sc", "load_wide", "add", "sub", "neg", "half", "mul", "muladd", "invert", "scm_mul", "equal", "is_zero")
    SC_WORDS = 16

    def debug_sc(self, op: str, n: int, a, b=None, c=None, fill: int = 0):
        """One operation of the scalar arithmetic mod l per lane (act_debug_sc_batch).  a, b, c: uint32 arrays of 16 n words, a record of
        16 words per lane (those the operation names; "load_sc" / "load_wide" read 32 / 64 bytes at the start of a's record).  Returns r
        as a uint32 array of 16 * (n rounded up to 256) words pre-filled with `fill`."""
        lanes = (n + 255) // 256 * 256
        ins = [None if x is None else np.ascontiguousarray(x, np.uint32) for x in (a, b, c)]
        assert all(x is None or x.size == self.SC_WORDS * n for x in ins)
        r = np.full(self.SC_WORDS * lanes, fill, np.uint32)
        self._ck(self.lib.act_debug_sc_batch(self.ctx, self.SC_OPS.index(op), n, *[None if x is None else x.ctypes.data for x in ins], r.ctypes.data))
        return r

    # ---- CBOR wire codec (src/cbor.rs) -----------------------------------------------------------------
    def cbor_size(self, type_name: str) -> int:
        return self.lib.act_cbor_size(self.ctx, CBOR_TYPES[type_name])

    def cbor_encode(self, type_name: str, records: bytes) -> list:
        t = CBOR_TYPES[type_name]; rb = self.lib.act_cbor_record_bytes(self.ctx, t); ml = self.lib.act_cbor_size(self.ctx, t)
        n = len(records) // rb; out = np.zeros(ml * n, np.uint8); p0, k0 = _in(records, rb * n)
        self._ck(self.lib.act_cbor_encode_batch(self.ctx, t, n, MEM_HOST, p0, out.ctypes.data))
        b = out.tobytes()
        return [b[i * ml:(i + 1) * ml] for i in range(n)]

    def cbor_decode(self, type_name: str, messages: list):
        """messages: list of byte strings (any lengths).  Returns (status bytes, records bytes)."""
        t = CBOR_TYPES[type_name]; rb = self.lib.act_cbor_record_bytes(self.ctx, t); n = len(messages)
        offs = np.zeros(n + 1, np.uint64); offs[1:] = np.cumsum([len(m) for m in messages], dtype=np.uint64)
        blob = b"".join(messages) + b"\0"
        out = np.zeros(rb * n, np.uint8); st = np.zeros(n, np.uint8); p0, k0 = _in(blob)
        self._ck(self.lib.act_cbor_decode_batch(self.ctx, t, n, MEM_HOST, p0, offs.ctypes.data, out.ctypes.data, st.ctypes.data))
        return st.tobytes(), out.tobytes()

    def cbor_read(self, type_name: str, messages: list):
        """cbor_decode with every message read by the general reader on the GPU (act_cbor_read_batch): (status bytes, records bytes)."""
        t = CBOR_TYPES[type_name]; rb = self.lib.act_cbor_record_bytes(self.ctx, t); n = len(messages)
        offs = np.zeros(n + 1, np.uint64); offs[1:] = np.cumsum([len(m) for m in messages], dtype=np.uint64)
        blob = b"".join(messages) + b"\0"
        out = np.zeros(rb * n, np.uint8); st = np.zeros(n, np.uint8); p0, k0 = _in(blob)
        self._ck(self.lib.act_cbor_read_batch(self.ctx, t, n, MEM_HOST, p0, offs.ctypes.data, out.ctypes.data, st.ctypes.data))
        return st.tobytes(), out.tobytes()

    def set_wire_reader(self, where: int):
        """WIRE_READER_DEVICE (default) or WIRE_READER_HOST: where the spend wire calls, the admission screen and the issuance wire calls
        read a message that is not the canonical encoding"""
        self._ck(self.lib.act_ctx_set_wire_reader(self.ctx, where))

    def wire_stats(self, reset: bool = False) -> dict:
        out = (C.c_uint64 * 4)()
        self._ck(self.lib.act_ctx_wire_stats(self.ctx, C.cast(out, C.c_void_p), 1 if reset else 0))
        return dict(zip(WIRE_STATS, (int(v) for v in out)))

    def redeem(self, nullifier_set, sk: bytes, proofs: bytes, rng: bytes, rng_mode: int = RNG_PER_LANE):
        """verify -> nullifier check-and-insert -> sign: statuses (3 = DoubleSpendError) and refunds."""
        n = len(proofs) // self.proof_bytes; out = np.zeros(128 * n, np.uint8); st = np.zeros(n, np.uint8)
        ps, ks = _in(sk, 64); p0, k0 = _in(proofs, self.proof_bytes * n); p1, k1 = _rng_arg(rng)
        self._ck(self.lib.act_redeem_batch(self.ctx, nullifier_set.h, n, MEM_HOST, ps, p0, p1, rng_mode, out.ctypes.data, st.ctypes.data))
        return st.tobytes(), out.tobytes()

    # the halves of issue / refund around the point where the crate draws its rng (src/lib.rs:643, 846): check, then sign what was accepted
    def issue_check(self, req: bytes) -> bytes:
        n = len(req) // 128; st = np.zeros(n, np.uint8); p0, k0 = _in(req, 128 * n)
        self._ck(self.lib.act_issue_check_batch(self.ctx, n, MEM_HOST, p0, st.ctypes.data)); return st.tobytes()

    def issue_sign(self, sk: bytes, req: bytes, c: bytes, status_in: bytes, rng: bytes, rng_mode: int = RNG_SEQUENTIAL):
        n = len(status_in); out = np.zeros(160 * n, np.uint8); st = np.zeros(n, np.uint8)
        ps, ks = _in(sk, 64); p0, k0 = _in(req, 128 * n); p1, k1 = _in(c, 32 * n); p2, k2 = _in(status_in, n); p3, k3 = _in(rng)
        self._ck(self.lib.act_issue_sign_batch(self.ctx, n, MEM_HOST, ps, p0, p1, p2, p3, rng_mode, out.ctypes.data, st.ctypes.data))
        return st.tobytes(), out.tobytes()

    def refund_sign(self, sk: bytes, kprime: bytes, status_in: bytes, rng: bytes, rng_mode: int = RNG_SEQUENTIAL):
        n = len(status_in); out = np.zeros(128 * n, np.uint8); st = np.zeros(n, np.uint8)
        ps, ks = _in(sk, 64); p0, k0 = _in(kprime, 32 * n); p1, k1 = _in(status_in, n); p2, k2 = _in(rng)
        self._ck(self.lib.act_refund_sign_batch(self.ctx, n, MEM_HOST, ps, p0, p1, p2, rng_mode, out.ctypes.data, st.ctypes.data))
        return st.tobytes(), out.tobytes()

    def redeem_dev(self, nullifier_set, sk: bytes, n: int, d_proofs: int, d_rng: int, rng_mode: int, d_out: int, d_status: int):
        ps, ks = _in(sk, 64)
        self._ck(self.lib.act_redeem_batch(self.ctx, nullifier_set.h, n, MEM_DEVICE, ps, d_proofs, d_rng, rng_mode, d_out, d_status))

    def verify_spend_cbor(self, sk: bytes, messages: list, want_kprime: bool = False):
        """CBOR SpendProof messages (byte strings of any length) -> statuses: from_cbor + refund's verification in one pass."""
        n = len(messages)
        offs = np.zeros(n + 1, np.uint64); offs[1:] = np.cumsum([len(m) for m in messages], dtype=np.uint64)
        blob = b"".join(messages) + b"\0"
        st = np.zeros(n, np.uint8); kp = np.zeros(32 * n, np.uint8) if want_kprime else None
        ps, ks = _in(sk, 64); p0, k0 = _in(blob)
        self._ck(self.lib.act_verify_spend_cbor_batch(self.ctx, n, MEM_HOST, ps, p0, offs.ctypes.data, st.ctypes.data, kp.ctypes.data if want_kprime else None))
        return (st.tobytes(), kp.tobytes()) if want_kprime else st.tobytes()

    def verify_spend_cbor_ptr(self, sk: bytes, n: int, mem: int, p_cbor: int, p_offsets: int, p_status: int, p_kprime: int = 0):
        ps, ks = _in(sk, 64)
        self._ck(self.lib.act_verify_spend_cbor_batch(self.ctx, n, mem, ps, p_cbor, p_offsets or None, p_status, p_kprime or None))

    def verify_spend_cbor_keys(self, sk: bytes, messages: list):
        """-> (statuses, enc(K') per message, nullifier `k` per message as it stood on the wire)"""
        n = len(messages); p0, k0, offs = _msgs(messages)
        st = np.zeros(n, np.uint8); kp = np.zeros(32 * n, np.uint8); nul = np.zeros(32 * n, np.uint8); ps, ks = _in(sk, 64)
        self._ck(self.lib.act_verify_spend_cbor_keys_batch(self.ctx, n, MEM_HOST, ps, p0, offs.ctypes.data, st.ctypes.data, kp.ctypes.data, nul.ctypes.data))
        return st.tobytes(), kp.tobytes(), nul.tobytes()

    def refund_cbor(self, sk: bytes, messages: list, rng, rng_mode: int = RNG_PER_LANE):
        """CBOR SpendProof messages in -> (statuses, list of CBOR Refund messages; b"" for a lane that was not signed)"""
        n = len(messages); p0, k0, offs = _msgs(messages); ml = self.cbor_size("Refund")
        st = np.zeros(n, np.uint8); out = np.zeros(ml * n, np.uint8); ps, ks = _in(sk, 64); pr, kr = _rng_arg(rng)
        self._ck(self.lib.act_refund_cbor_batch(self.ctx, n, MEM_HOST, ps, p0, offs.ctypes.data, pr, rng_mode, out.ctypes.data, st.ctypes.data))
        b = out.tobytes()
        assert all(st[i] == 0 or not out[i * ml:(i + 1) * ml].any() for i in range(n)), "a failed lane's slot is not zero"
        return st.tobytes(), [b[i * ml:(i + 1) * ml] if st[i] == 0 else b"" for i in range(n)]

    def refund_sign_cbor(self, sk: bytes, kprime: bytes, status_in: bytes, rng, rng_mode: int = RNG_SEQUENTIAL):
        n = len(status_in); ml = self.cbor_size("Refund"); st = np.zeros(n, np.uint8); out = np.zeros(ml * n, np.uint8)
        ps, ks = _in(sk, 64); p0, k0 = _in(kprime, 32 * n); p1, k1 = _in(status_in, n); pr, kr = _rng_arg(rng)
        self._ck(self.lib.act_refund_sign_cbor_batch(self.ctx, n, MEM_HOST, ps, p0, p1, pr, rng_mode, out.ctypes.data, st.ctypes.data))
        b = out.tobytes()
        return st.tobytes(), [b[i * ml:(i + 1) * ml] if st[i] == 0 else b"" for i in range(n)]

    def redeem_cbor(self, nullifier_set, sk: bytes, messages: list, rng, rng_mode: int = RNG_SEQUENTIAL, raw: bool = False):
        """wire bytes -> verify -> nullifier check-and-insert -> sign -> wire bytes.  raw=True: (rc, statuses, out bytes), no exception."""
        n = len(messages); p0, k0, offs = _msgs(messages); ml = self.cbor_size("Refund")
        st = np.zeros(n, np.uint8); out = np.full(ml * n, 7 if raw else 0, np.uint8); ps, ks = _in(sk, 64); pr, kr = _rng_arg(rng)
        rc = self.lib.act_redeem_cbor_batch(self.ctx, nullifier_set.h, n, MEM_HOST, ps, p0, offs.ctypes.data, pr, rng_mode, out.ctypes.data, st.ctypes.data)
        if raw:
            return rc, st.tobytes(), out.tobytes()
        self._ck(rc)
        b = out.tobytes()
        return st.tobytes(), [b[i * ml:(i + 1) * ml] if st[i] == 0 else b"" for i in range(n)]

    def wire_ptr(self, fn: str, sk: bytes, n: int, mem: int, p_cbor: int, p_offsets: int, p_rng: int, rng_mode: int, p_out: int, p_status: int, nullifier_set=None):
        """act_refund_cbor_batch / act_redeem_cbor_batch on raw pointers of either kind (device-memory callers)"""
        ps, ks = _in(sk, 64)
        if fn == "refund":
            self._ck(self.lib.act_refund_cbor_batch(self.ctx, n, mem, ps, p_cbor, p_offsets or None, p_rng, rng_mode, p_out, p_status))
        else:
            self._ck(self.lib.act_redeem_cbor_batch(self.ctx, nullifier_set.h, n, mem, ps, p_cbor, p_offsets or None, p_rng, rng_mode, p_out, p_status))

    # ---- key rotation: one batch against an ordered ring of issuer keys (act_*_keyring_batch; keys = list of 64-byte sk) ----------
    def verify_spend_keyring(self, keys, proofs: bytes, want_kprime: bool = False, bind=_UNBOUND):
        """-> (statuses, out_key bytes: the ring index every accepted lane verified under, KEY_NONE elsewhere[, enc(K')]).  bind given
        (32 bytes a lane, or None: NULL): act_verify_spend_keyring_bound_batch"""
        n = len(proofs) // self.proof_bytes; st = np.zeros(n, np.uint8); ok = np.zeros(n, np.uint8)
        kp = np.zeros(32 * n, np.uint8) if want_kprime else None
        pk, kk = _in(b"".join(keys)); p0, k0 = _in(proofs, self.proof_bytes * n)
        if bind is _UNBOUND:
            self._ck(self.lib.act_verify_spend_keyring_batch(self.ctx, n, MEM_HOST, pk, len(keys), p0, st.ctypes.data, ok.ctypes.data, kp.ctypes.data if want_kprime else None))
        else:
            pb, kb = _in(bind, 32 * n) if bind is not None else (None, None)
            self._ck(self.lib.act_verify_spend_keyring_bound_batch(self.ctx, n, MEM_HOST, pk, len(keys), p0, pb, st.ctypes.data, ok.ctypes.data,
                                                                   kp.ctypes.data if want_kprime else None))
        return (st.tobytes(), ok.tobytes(), kp.tobytes()) if want_kprime else (st.tobytes(), ok.tobytes())

    def refund_sign_keyring(self, keys, key_index: bytes, kprime: bytes, status_in: bytes, rng: bytes, rng_mode: int = RNG_SEQUENTIAL):
        n = len(status_in); out = np.zeros(128 * n, np.uint8); st = np.zeros(n, np.uint8)
        pk, kk = _in(b"".join(keys)); pi, ki = _in(key_index, n); p0, k0 = _in(kprime, 32 * n); p1, k1 = _in(status_in, n); p2, k2 = _in(rng)
        self._ck(self.lib.act_refund_sign_keyring_batch(self.ctx, n, MEM_HOST, pk, len(keys), pi, p0, p1, p2, rng_mode, out.ctypes.data, st.ctypes.data))
        return st.tobytes(), out.tobytes()

    def redeem_keyring(self, nullifier_set, keys, proofs: bytes, rng, rng_mode: int = RNG_PER_LANE, sign_key: int = SIGN_MATCHED, raw: bool = False,
                       key_epochs=None):
        """-> (statuses, refunds, out_key).  raw=True: (rc, statuses, refunds, out_key), no exception.  key_epochs: one epoch per ring
        key; an accepted lane's nullifier is recorded under the epoch of the key it matched (act_redeem_keyring_epochs_batch)."""
        n = len(proofs) // self.proof_bytes; out = np.full(128 * n, 7 if raw else 0, np.uint8); st = np.zeros(n, np.uint8); ok = np.zeros(n, np.uint8)
        pk, kk = _in(b"".join(keys)); p0, k0 = _in(proofs, self.proof_bytes * n); p1, k1 = _rng_arg(rng)
        if key_epochs is not None:
            ke = _epoch_table(key_epochs, len(keys))
            rc = self.lib.act_redeem_keyring_epochs_batch(self.ctx, nullifier_set.h, n, MEM_HOST, pk, len(keys), ke.ctypes.data, sign_key, p0, p1, rng_mode,
                                                          out.ctypes.data, st.ctypes.data, ok.ctypes.data)
        else:
            rc = self.lib.act_redeem_keyring_batch(self.ctx, nullifier_set.h, n, MEM_HOST, pk, len(keys), sign_key, p0, p1, rng_mode, out.ctypes.data, st.ctypes.data, ok.ctypes.data)
        if raw:
            return rc, st.tobytes(), out.tobytes(), ok.tobytes()
        self._ck(rc)
        return st.tobytes(), out.tobytes(), ok.tobytes()

    def redeem_cbor_keyring(self, nullifier_set, keys, messages: list, rng, rng_mode: int = RNG_SEQUENTIAL, sign_key: int = SIGN_MATCHED, key_epochs=None):
        """wire bytes in, wire bytes out -> (statuses, list of CBOR Refund messages (b"" where not signed), out_key)"""
        n = len(messages); p0, k0, offs = _msgs(messages); ml = self.cbor_size("Refund")
        st = np.zeros(n, np.uint8); ok = np.zeros(n, np.uint8); out = np.zeros(ml * n, np.uint8); pk, kk = _in(b"".join(keys)); pr, kr = _rng_arg(rng)
        if key_epochs is not None:
            ke = _epoch_table(key_epochs, len(keys))
            self._ck(self.lib.act_redeem_cbor_keyring_epochs_batch(self.ctx, nullifier_set.h, n, MEM_HOST, pk, len(keys), ke.ctypes.data, sign_key, p0, offs.ctypes.data,
                                                                   pr, rng_mode, out.ctypes.data, st.ctypes.data, ok.ctypes.data))
        else:
            self._ck(self.lib.act_redeem_cbor_keyring_batch(self.ctx, nullifier_set.h, n, MEM_HOST, pk, len(keys), sign_key, p0, offs.ctypes.data, pr, rng_mode,
                                                            out.ctypes.data, st.ctypes.data, ok.ctypes.data))
        b = out.tobytes()
        assert all(st[i] == 0 or not out[i * ml:(i + 1) * ml].any() for i in range(n)), "a failed lane's slot is not zero"
        return st.tobytes(), [b[i * ml:(i + 1) * ml] if st[i] == 0 else b"" for i in range(n)], ok.tobytes()

    # ---- key rotation, the client's side: to_credit_token against a ring of issuer PUBLIC keys (publics = list of 32-byte w) ----------
    def issuance_to_credit_token_ring(self, pre: bytes, publics, req: bytes, resp: bytes, raw: bool = False):
        """-> (statuses, tokens, out_key bytes: the smallest ring index every accepted lane verifies under, KEY_NONE elsewhere).
        raw=True: (rc, statuses, tokens, out_key), no exception."""
        n = len(pre) // 64; out = np.zeros(160 * n, np.uint8); st = np.zeros(n, np.uint8); ok = np.zeros(n, np.uint8)
        p0, k0 = _in(pre, 64 * n); pw, kw = _in(b"".join(publics)); p1, k1 = _in(req, 128 * n); p2, k2 = _in(resp, 160 * n)
        rc = self.lib.act_issuance_to_credit_token_keyring_batch(self.ctx, n, MEM_HOST, p0, pw, len(publics), p1, p2, out.ctypes.data, st.ctypes.data, ok.ctypes.data)
        if raw:
            return rc, st.tobytes(), out.tobytes(), ok.tobytes()
        self._ck(rc)
        return st.tobytes(), out.tobytes(), ok.tobytes()

    def refund_to_credit_token_ring(self, prerefund: bytes, proofs: bytes, refund: bytes, publics, raw: bool = False):
        n = len(prerefund) // 96; out = np.zeros(160 * n, np.uint8); st = np.zeros(n, np.uint8); ok = np.zeros(n, np.uint8)
        p0, k0 = _in(prerefund, 96 * n); p1, k1 = _in(proofs, self.proof_bytes * n); p2, k2 = _in(refund, 128 * n); pw, kw = _in(b"".join(publics))
        rc = self.lib.act_refund_to_credit_token_keyring_batch(self.ctx, n, MEM_HOST, p0, p1, p2, pw, len(publics), out.ctypes.data, st.ctypes.data, ok.ctypes.data)
        if raw:
            return rc, st.tobytes(), out.tobytes(), ok.tobytes()
        self._ck(rc)
        return st.tobytes(), out.tobytes(), ok.tobytes()

    def client_ring_ptr(self, fn: str, publics, n: int, mem: int, **p):
        """the same on raw pointers of either kind (device-memory callers): fn = issuance / refund / refund_return (p["refund"]: the
        160-byte RefundReturn records); the ring itself is host bytes"""
        pw, kw = _in(b"".join(publics)); nk = len(publics)
        if fn == "refund_return":
            self._ck(self.lib.act_refund_to_credit_token_return_keyring_batch(self.ctx, n, mem, p["pre"], p["proofs"], p["refund"], pw, nk, p["out"], p["status"], p["out_key"]))
        elif fn == "issuance":
            self._ck(self.lib.act_issuance_to_credit_token_keyring_batch(self.ctx, n, mem, p["pre"], pw, nk, p["req"], p["resp"], p["out"], p["status"], p["out_key"]))
        else:
            self._ck(self.lib.act_refund_to_credit_token_keyring_batch(self.ctx, n, mem, p["pre"], p["proofs"], p["refund"], pw, nk, p["out"], p["status"], p["out_key"]))

    def keyring_ptr(self, fn: str, keys, n: int, mem: int, **p):
        """the ring calls on raw pointers of either kind (device-memory callers): fn = verify / sign / redeem / redeem_cbor"""
        pk, kk = _in(b"".join(keys)); nk = len(keys)
        if fn == "verify" and "bind" in p:      # request binding (0 / None: NULL)
            self._ck(self.lib.act_verify_spend_keyring_bound_batch(self.ctx, n, mem, pk, nk, p["proofs"], p["bind"] or None, p["status"], p["out_key"], p.get("kprime") or None))
        elif fn == "verify":
            self._ck(self.lib.act_verify_spend_keyring_batch(self.ctx, n, mem, pk, nk, p["proofs"], p["status"], p["out_key"], p.get("kprime") or None))
        elif fn == "sign":
            self._ck(self.lib.act_refund_sign_keyring_batch(self.ctx, n, mem, pk, nk, p["key_index"], p["kprime"], p["status_in"], p["rng"], p["rng_mode"], p["out"], p["status"]))
        elif fn in ("redeem", "redeem_cbor") and p.get("key_epochs") is not None:
            ke = _epoch_table(p["key_epochs"], nk)
            if fn == "redeem":
                self._ck(self.lib.act_redeem_keyring_epochs_batch(self.ctx, p["set"].h, n, mem, pk, nk, ke.ctypes.data, p.get("sign_key", SIGN_MATCHED), p["proofs"],
                                                                  p["rng"], p["rng_mode"], p["out"], p["status"], p["out_key"]))
            else:
                self._ck(self.lib.act_redeem_cbor_keyring_epochs_batch(self.ctx, p["set"].h, n, mem, pk, nk, ke.ctypes.data, p.get("sign_key", SIGN_MATCHED), p["cbor"],
                                                                       p.get("offsets") or None, p["rng"], p["rng_mode"], p["out"], p["status"], p["out_key"]))
        elif fn == "redeem":
            self._ck(self.lib.act_redeem_keyring_batch(self.ctx, p["set"].h, n, mem, pk, nk, p.get("sign_key", SIGN_MATCHED), p["proofs"], p["rng"], p["rng_mode"],
                                                       p["out"], p["status"], p["out_key"]))
        else:
            self._ck(self.lib.act_redeem_cbor_keyring_batch(self.ctx, p["set"].h, n, mem, pk, nk, p.get("sign_key", SIGN_MATCHED), p["cbor"], p.get("offsets") or None,
                                                            p["rng"], p["rng_mode"], p["out"], p["status"], p["out_key"]))

    # ---- the admission family: five kinds of call, each on records and on wire bytes, plain and (but `replay`) unique -----------------
    # kind -> (C symbol stem, count names, count names of the unique form, record row, CBOR type of the output, takes charges, takes
    # returned, tail: receipts / nonce_key / replayed where True, rng / rng_mode where False, the _ptr form honours raw)
    _FAMILY = {"admit": ("admit", ADMIT_COUNTS, ADMIT_UNIQUE_COUNTS, 128, "Refund", True, False, False, True),
               "return": ("return", REDEEM_RETURN_COUNTS, REDEEM_RETURN_UNIQUE_COUNTS, 160, "RefundReturn", True, True, False, False),
               "replay": ("replay", REPLAY_COUNTS, REPLAY_COUNTS, 128, "Refund", False, False, True, True),
               "admit_replay": ("admit_replay", ADMIT_REPLAY_COUNTS, ADMIT_REPLAY_UNIQUE_COUNTS, 128, "Refund", True, False, True, True),
               "return_replay": ("return_replay", RETURN_REPLAY_COUNTS, RETURN_REPLAY_UNIQUE_COUNTS, 160, "RefundReturn", True, True, True, True)}

    def _family_ptr(self, kind: str, fn: str, keys, n: int, mem: int, p: dict, raw: bool = None):
        """one call of the family on raw pointers of either kind, its arguments in the header's order.  -> counts dict, or (rc, counts)
        with raw; raw=None: what p asks for, where the kind's _ptr method honours it"""
        stem, names, unique_names, _, _, has_charges, has_returned, replay, honours_raw = self._FAMILY[kind]
        raw = (honours_raw and bool(p.get("raw"))) if raw is None else raw; unique = kind != "replay" and bool(p.get("unique")); wire = fn != "redeem"
        bound = "bind" in p      # request binding: p["bind"] = n * 32 bytes behind the proofs or messages (0 / None: NULL)
        if bound and (kind != "return_replay" or unique):
            raise ActError("request binding: only the return-replay and reserve calls have a bound form, and it has no unique form")
        pk, kk = _in(b"".join(keys)); nk = len(keys)
        ke = _epoch_table(p["key_epochs"], nk) if p.get("key_epochs") is not None else None
        names = unique_names if unique else names
        cnt = (C.c_uint64 * len(names))()
        args = [self.ctx, p["set"].h] + ([p["receipts"].h] if replay else []) + [n, mem, pk, nk, ke.ctypes.data if ke is not None else None, p.get("sign_key", SIGN_MATCHED)]
        args += [p["cbor"], p.get("offsets") or None] if wire else [p["proofs"]]
        args += [p["bind"] or None] if bound else []
        args += ([p.get("charges") or None] if has_charges else []) + ([p.get("returned") or None] if has_returned else [])
        if replay:
            pn, kn = _in(p["nonce_key"], 32)
            args += [pn, p["out"], p["status"], p["out_key"], p.get("replayed") or None, cnt]
        else:
            args += [p["rng"], p["rng_mode"], p["out"], p["status"], p["out_key"], cnt]
        rc = getattr(self.lib, "act_redeem_%s%s%s_batch" % ("cbor_" if wire else "", stem, "_unique" if unique else "_bound" if bound else ""))(*args)
        if not raw:
            self._ck(rc)
        counts = dict(zip(names, (int(v) for v in cnt)))
        return (rc, counts) if raw else counts

    def _family_host(self, kind: str, nullifier_set, keys, rows, tail: dict, sign_key, key_epochs, charges, returned, raw: bool, unique: bool, bind=_UNBOUND):
        """one call of the family from host memory; rows: records (bytes) or messages (a list).  -> (statuses, records | list of messages
        (b"" where not signed), out_key, [replayed,] counts dict); raw=True: (rc, ...), no exception.  bind given (32 bytes a lane, or
        None: NULL): the kind's bound call"""
        _, _, _, row, cbor_type, _, _, replay, _ = self._FAMILY[kind]
        wire = isinstance(rows, (list, tuple))
        if wire:
            n = len(rows); p0, k0, offs = _msgs(rows); ob = self.cbor_size(cbor_type)
            p = dict(cbor=p0, offsets=offs.ctypes.data)
        else:
            n = len(rows) // self.proof_bytes; p0, k0 = _in(rows, self.proof_bytes * n); ob = row
            p = dict(proofs=p0)
        out = np.full(ob * n, 7 if raw and not wire else 0, np.uint8)      # (records under raw: a call that writes nothing leaves the 7s)
        st = np.full(n, 99 if raw and replay else 0, np.uint8); ok = np.zeros(n, np.uint8); rp = np.zeros(n, np.uint8)
        pc, kc = _in(charges, 32 * n) if charges is not None else (None, None)
        pt, kt = _in(returned, 32 * n) if returned is not None else (None, None)
        if replay:
            p.update(receipts=tail["receipts"], nonce_key=tail["nonce_key"], replayed=rp.ctypes.data)
        else:
            pr, kr = _rng_arg(tail["rng"])
            p.update(rng=pr, rng_mode=tail["rng_mode"])
        p.update(set=nullifier_set, sign_key=sign_key, key_epochs=key_epochs, charges=pc, returned=pt, out=out.ctypes.data, status=st.ctypes.data, out_key=ok.ctypes.data,
                 unique=unique)
        if bind is not _UNBOUND:
            pb, kb = _in(bind, 32 * n) if bind is not None else (None, None)
            p.update(bind=pb)
        rc, counts = self._family_ptr(kind, "redeem_cbor" if wire else "redeem", keys, n, MEM_HOST, p, raw=True)
        b = out.tobytes()
        res = (st.tobytes(), [b[i * ob:(i + 1) * ob] if st[i] == 0 else b"" for i in range(n)] if wire else b, ok.tobytes()) + ((rp.tobytes(),) if replay else ()) + (counts,)
        if raw:
            return (rc,) + res
        self._ck(rc)
        assert not wire or all(st[i] == 0 or not out[i * ob:(i + 1) * ob].any() for i in range(n)), "a failed lane's slot is not zero"
        return res

    # ---- admission before verification (act_redeem_admit_batch / act_redeem_cbor_admit_batch) ---------------------------------------
    def redeem_admit(self, nullifier_set, keys, proofs: bytes, rng, rng_mode: int = RNG_PER_LANE, sign_key: int = SIGN_MATCHED, charges: bytes = None,
                     key_epochs=None, raw: bool = False, unique: bool = False):
        """redeem_keyring with the admission stage in front: a lane whose charge s is not charges[i] (STATUS_WRONG_CHARGE) or whose
        nullifier is already in the set (3) is answered without being verified.  -> (statuses, refunds, out_key, counts dict);
        raw=True: (rc, statuses, refunds, out_key, counts), no exception.  unique=True: act_redeem_admit_unique_batch -- a lane with
        the bytes of an earlier lane is not verified either; the same answers, and counts gains "copies"."""
        return self._family_host("admit", nullifier_set, keys, proofs, dict(rng=rng, rng_mode=rng_mode), sign_key, key_epochs, charges, None, raw, unique)

    def redeem_cbor_admit(self, nullifier_set, keys, messages: list, rng, rng_mode: int = RNG_SEQUENTIAL, sign_key: int = SIGN_MATCHED, charges: bytes = None,
                          key_epochs=None, raw: bool = False, unique: bool = False):
        """wire bytes in, wire bytes out -> (statuses, list of CBOR Refund messages (b"" where not signed), out_key, counts dict);
        unique=True: act_redeem_cbor_admit_unique_batch (a copy has the same length and the same bytes as an earlier message)"""
        return self._family_host("admit", nullifier_set, keys, list(messages), dict(rng=rng, rng_mode=rng_mode), sign_key, key_epochs, charges, None, raw, unique)

    def admit_ptr(self, fn: str, keys, n: int, mem: int, **p):
        """the admission calls on raw pointers of either kind: fn = redeem / redeem_cbor; p: set, proofs | cbor (+ offsets), charges,
        rng, rng_mode, out, status, out_key, key_epochs, sign_key, unique (the act_redeem_*admit_unique_batch forms).  -> counts dict"""
        return self._family_ptr("admit", fn, keys, n, mem, p)

    # ---- partial refunds (act_redeem_return_batch / act_redeem_cbor_return_batch and the two calls around them) ---------------------
    def refund_sign_return_keyring(self, keys, key_index: bytes, kprime: bytes, status_in: bytes, rng: bytes, returned: bytes = None,
                                   rng_mode: int = RNG_SEQUENTIAL):
        """refund_sign_keyring over X_A = g + K' + t h1 -> (statuses, 160-byte RefundReturn records).  The call does not see s: the
        caller bounds t."""
        n = len(status_in); out = np.zeros(160 * n, np.uint8); st = np.zeros(n, np.uint8)
        pk, kk = _in(b"".join(keys)); pi, ki = _in(key_index, n); p0, k0 = _in(kprime, 32 * n); p1, k1 = _in(status_in, n); p2, k2 = _in(rng)
        pt, kt = _in(returned, 32 * n) if returned is not None else (None, None)
        self._ck(self.lib.act_refund_sign_return_keyring_batch(self.ctx, n, MEM_HOST, pk, len(keys), pi, p0, p1, p2, rng_mode, pt, out.ctypes.data, st.ctypes.data))
        return st.tobytes(), out.tobytes()

    def redeem_return(self, nullifier_set, keys, proofs: bytes, rng, rng_mode: int = RNG_PER_LANE, sign_key: int = SIGN_MATCHED, charges: bytes = None,
                      returned: bytes = None, key_epochs=None, raw: bool = False, unique: bool = False):
        """redeem_admit with the amounts the issuer returns: a lane with t > s is STATUS_RETURN_TOO_BIG (not looked up, not verified,
        not recorded, not signed); the others are signed over X_A = g + K' + t h1.  -> (statuses, 160-byte RefundReturn records,
        out_key, counts dict); raw=True: (rc, ...), no exception.  unique=True: act_redeem_return_unique_batch -- a lane with the proof
        bytes of an earlier lane (whatever its t) is not verified; the same answers, and counts gains "copies"."""
        return self._family_host("return", nullifier_set, keys, proofs, dict(rng=rng, rng_mode=rng_mode), sign_key, key_epochs, charges, returned, raw, unique)

    def redeem_cbor_return(self, nullifier_set, keys, messages: list, rng, rng_mode: int = RNG_SEQUENTIAL, sign_key: int = SIGN_MATCHED, charges: bytes = None,
                           returned: bytes = None, key_epochs=None, raw: bool = False, unique: bool = False):
        """wire bytes in, wire bytes out -> (statuses, list of CBOR RefundReturn messages (b"" where not signed), out_key, counts dict);
        unique=True: act_redeem_cbor_return_unique_batch (a copy has the same length and the same bytes as an earlier message)"""
        return self._family_host("return", nullifier_set, keys, list(messages), dict(rng=rng, rng_mode=rng_mode), sign_key, key_epochs, charges, returned, raw, unique)

    def return_ptr(self, fn: str, keys, n: int, mem: int, **p):
        """the return calls on raw pointers of either kind: fn = redeem / redeem_cbor; p as admit_ptr's plus returned (unique: the
        act_redeem_*return_unique_batch forms).  -> counts dict"""
        return self._family_ptr("return", fn, keys, n, mem, p)

    def refund_to_credit_token_return(self, prerefund: bytes, proofs: bytes, refund_return: bytes, w: bytes):
        """refund_to_credit_token over 160-byte RefundReturn records -> (statuses, tokens with balance m + t); t > s is status 8"""
        n = len(prerefund) // 96; out = np.zeros(160 * n, np.uint8); st = np.zeros(n, np.uint8)
        p0, k0 = _in(prerefund, 96 * n); p1, k1 = _in(proofs, self.proof_bytes * n); p2, k2 = _in(refund_return, 160 * n); pw, kw = _in(w, 32)
        self._ck(self.lib.act_refund_to_credit_token_return_batch(self.ctx, n, MEM_HOST, p0, p1, p2, pw, out.ctypes.data, st.ctypes.data))
        return st.tobytes(), out.tobytes()

    def refund_to_credit_token_return_ring(self, prerefund: bytes, proofs: bytes, refund_return: bytes, publics, raw: bool = False):
        """refund_to_credit_token_return against a ring of issuer public keys -> (statuses, tokens, out_key bytes: the smallest ring
        index every accepted lane verifies under, KEY_NONE elsewhere).  raw=True: (rc, statuses, tokens, out_key), no exception."""
        n = len(prerefund) // 96; out = np.zeros(160 * n, np.uint8); st = np.zeros(n, np.uint8); ok = np.zeros(n, np.uint8)
        p0, k0 = _in(prerefund, 96 * n); p1, k1 = _in(proofs, self.proof_bytes * n); p2, k2 = _in(refund_return, 160 * n); pw, kw = _in(b"".join(publics))
        rc = self.lib.act_refund_to_credit_token_return_keyring_batch(self.ctx, n, MEM_HOST, p0, p1, p2, pw, len(publics), out.ctypes.data, st.ctypes.data, ok.ctypes.data)
        if raw:
            return rc, st.tobytes(), out.tobytes(), ok.tobytes()
        self._ck(rc)
        return st.tobytes(), out.tobytes(), ok.tobytes()

    # ---- replayable redemption (act_redeem_replay_batch / act_redeem_cbor_replay_batch / act_replay_derive_batch) -------------------
    def redeem_replay(self, nullifier_set, receipts, keys, proofs: bytes, nonce_key: bytes, sign_key: int = SIGN_MATCHED, key_epochs=None, raw: bool = False):
        """redeem_keyring with derived nonces and a receipts set: a retried proof gets its refund again, byte for byte.
        -> (statuses, refunds, out_key, replayed, counts dict); raw=True: (rc, ...), no exception"""
        return self._family_host("replay", nullifier_set, keys, proofs, dict(receipts=receipts, nonce_key=nonce_key), sign_key, key_epochs, None, None, raw, False)

    def redeem_cbor_replay(self, nullifier_set, receipts, keys, messages: list, nonce_key: bytes, sign_key: int = SIGN_MATCHED, key_epochs=None, raw: bool = False):
        """wire bytes in, wire bytes out -> (statuses, list of CBOR Refund messages (b"" where not signed), out_key, replayed, counts dict)"""
        return self._family_host("replay", nullifier_set, keys, list(messages), dict(receipts=receipts, nonce_key=nonce_key), sign_key, key_epochs, None, None, raw, False)

    def replay_ptr(self, fn: str, keys, n: int, mem: int, **p):
        """the replay calls on raw pointers of either kind: fn = redeem / redeem_cbor; p: set, receipts, proofs | cbor (+ offsets), nonce_key,
        out, status, out_key, replayed, key_epochs, sign_key, raw.  -> counts dict, or (rc, counts) with raw"""
        return self._family_ptr("replay", fn, keys, n, mem, p)

    # ---- admission for the replayable redemption (act_redeem_admit_replay_batch / act_redeem_cbor_admit_replay_batch) ----------------
    def redeem_admit_replay(self, nullifier_set, receipts, keys, proofs: bytes, nonce_key: bytes, sign_key: int = SIGN_MATCHED, key_epochs=None, charges: bytes = None,
                            raw: bool = False, unique: bool = False):
        """redeem_replay with the admission screen in front: a wrong charge (STATUS_WRONG_CHARGE) and a spent nullifier whose receipt is
        not this proof's (STATUS_DOUBLE_SPEND) are answered unverified; a retry is verified and served.
        -> (statuses, refunds, out_key, replayed, counts dict); raw=True: (rc, ...), no exception.  unique=True:
        act_redeem_admit_replay_unique_batch -- a lane with the bytes of an earlier lane is not verified and takes that lane's answer"""
        return self._family_host("admit_replay", nullifier_set, keys, proofs, dict(receipts=receipts, nonce_key=nonce_key), sign_key, key_epochs, charges, None, raw, unique)

    def redeem_cbor_admit_replay(self, nullifier_set, receipts, keys, messages: list, nonce_key: bytes, sign_key: int = SIGN_MATCHED, key_epochs=None,
                                 charges: bytes = None, raw: bool = False, unique: bool = False):
        """wire bytes in, wire bytes out -> (statuses, list of CBOR Refund messages (b"" where not signed), out_key, replayed, counts dict)
        unique=True: act_redeem_cbor_admit_replay_unique_batch (a copy has the same length and the same bytes as an earlier message)"""
        return self._family_host("admit_replay", nullifier_set, keys, list(messages), dict(receipts=receipts, nonce_key=nonce_key), sign_key, key_epochs, charges, None, raw, unique)

    def admit_replay_ptr(self, fn: str, keys, n: int, mem: int, **p):
        """the two calls on raw pointers of either kind: fn = redeem / redeem_cbor; p: set, receipts, proofs | cbor (+ offsets), charges, nonce_key,
        out, status, out_key, replayed, key_epochs, sign_key, raw, unique (the act_redeem_*admit_replay_unique_batch forms).
        -> counts dict, or (rc, counts) with raw"""
        return self._family_ptr("admit_replay", fn, keys, n, mem, p)

    # ---- replayable partial refunds (act_redeem_return_replay_batch / act_redeem_cbor_return_replay_batch / act_replay_derive_return_batch)
    def redeem_return_replay(self, nullifier_set, receipts, keys, proofs: bytes, nonce_key: bytes, sign_key: int = SIGN_MATCHED, key_epochs=None, charges: bytes = None,
                             returned: bytes = None, raw: bool = False, unique: bool = False, bind=_UNBOUND):
        """redeem_admit_replay with the amounts the issuer returns: t > s is STATUS_RETURN_TOO_BIG in the screen; the receipt pins t, so
        a retry with the same t is served byte for byte and one with another t is STATUS_DOUBLE_SPEND.
        -> (statuses, 160-byte RefundReturn records, out_key, replayed, counts dict); raw=True: (rc, ...), no exception
        unique=True: act_redeem_return_replay_unique_batch -- a lane with the bytes of an earlier lane is not verified; it takes that
        lane's answer if it names that lane's amount and is STATUS_DOUBLE_SPEND behind an accepted leader if it names another"""
        return self._family_host("return_replay", nullifier_set, keys, proofs, dict(receipts=receipts, nonce_key=nonce_key), sign_key, key_epochs, charges, returned, raw, unique,
                                 bind)

    def redeem_cbor_return_replay(self, nullifier_set, receipts, keys, messages: list, nonce_key: bytes, sign_key: int = SIGN_MATCHED, key_epochs=None,
                                  charges: bytes = None, returned: bytes = None, raw: bool = False, unique: bool = False, bind=_UNBOUND):
        """wire bytes in, wire bytes out -> (statuses, list of CBOR RefundReturn messages (b"" where not signed), out_key, replayed, counts dict)
        unique=True: act_redeem_cbor_return_replay_unique_batch (a copy has the same length and the same bytes as an earlier message)"""
        return self._family_host("return_replay", nullifier_set, keys, list(messages), dict(receipts=receipts, nonce_key=nonce_key), sign_key, key_epochs, charges, returned, raw, unique,
                                 bind)

    def return_replay_ptr(self, fn: str, keys, n: int, mem: int, **p):
        """the two calls on raw pointers of either kind: fn = redeem / redeem_cbor; p as admit_replay_ptr's plus returned (unique: the
        act_redeem_*return_replay_unique_batch forms).  -> counts dict, or (rc, counts) with raw"""
        return self._family_ptr("return_replay", fn, keys, n, mem, p)

    def replay_derive(self, keys, key_index: bytes, nonce_key: bytes, nullifiers: bytes, kprime: bytes, status_in: bytes, stride: int = 32, returned: bytes = None):
        """-> (tags: 32 bytes a lane, nonces: 128 bytes a lane) of the lanes with status_in 0 and key_index < len(keys); zeros elsewhere.
        returned (32 bytes a lane): act_replay_derive_return_batch -- the hashes take the lane's amount"""
        n = len(status_in); tags = np.zeros(32 * n, np.uint8); non = np.zeros(128 * n, np.uint8)
        pk, kk = _in(b"".join(keys)); pi, ki = _in(key_index, n); pn, kn = _in(nonce_key, 32); p0, k0 = _in(nullifiers); p1, k1 = _in(kprime, 32 * n); p2, k2 = _in(status_in, n)
        if returned is None:
            self._ck(self.lib.act_replay_derive_batch(self.ctx, n, MEM_HOST, pk, len(keys), pi, pn, p0, stride, p1, p2, tags.ctypes.data, non.ctypes.data))
        else:
            pt, kt = _in(returned, 32 * n)
            self._ck(self.lib.act_replay_derive_return_batch(self.ctx, n, MEM_HOST, pk, len(keys), pi, pn, p0, stride, p1, p2, pt, tags.ctypes.data, non.ctypes.data))
        return tags.tobytes(), non.tobytes()

    def replay_derive_ptr(self, keys, n: int, mem: int, nonce_key: bytes, p_key_index: int, p_nullifiers: int, stride: int, p_kprime: int, p_status_in: int,
                          p_tags: int = 0, p_nonces: int = 0, p_returned: int = None):
        """p_returned given (0: NULL): act_replay_derive_return_batch"""
        pk, kk = _in(b"".join(keys)); pn, kn = _in(nonce_key, 32)
        if p_returned is None:
            self._ck(self.lib.act_replay_derive_batch(self.ctx, n, mem, pk, len(keys), p_key_index, pn, p_nullifiers, stride, p_kprime, p_status_in, p_tags or None, p_nonces or None))
        else:
            self._ck(self.lib.act_replay_derive_return_batch(self.ctx, n, mem, pk, len(keys), p_key_index, pn, p_nullifiers, stride, p_kprime, p_status_in, p_returned or None,
                                                             p_tags or None, p_nonces or None))

    # ---- reserve and settle (act_redeem_reserve_batch / act_redeem_cbor_reserve_batch / act_redeem_settle_batch / act_redeem_cbor_settle_batch)
    def reserve_ptr(self, fn: str, keys, n: int, mem: int, **p):
        """the reserve calls on raw pointers of either kind: fn = redeem / redeem_cbor; p: set, receipts, proofs | cbor (+ offsets), charges,
        out (96 bytes a lane), status, out_key, replayed, key_epochs, raw.  -> counts dict, or (rc, counts) with raw"""
        wire = fn != "redeem"; nk = len(keys); pk, kk = _in(b"".join(keys))
        ke = _epoch_table(p["key_epochs"], nk) if p.get("key_epochs") is not None else None
        cnt = (C.c_uint64 * len(RESERVE_COUNTS))()
        args = [self.ctx, p["set"].h, p["receipts"].h if p["receipts"] is not None else None, n, mem, pk, nk, ke.ctypes.data if ke is not None else None]
        args += [p["cbor"], p.get("offsets") or None] if wire else [p["proofs"]]
        bound = "bind" in p      # request binding (0 / None: NULL): the bound calls
        args += [p["bind"] or None] if bound else []
        args += [p.get("charges") or None, p["out"], p["status"], p["out_key"], p.get("replayed") or None, cnt]
        rc = getattr(self.lib, "act_redeem_%sreserve%s_batch" % ("cbor_" if wire else "", "_bound" if bound else ""))(*args)
        counts = dict(zip(RESERVE_COUNTS, (int(v) for v in cnt)))
        if p.get("raw"):
            return rc, counts
        self._ck(rc)
        return counts

    def _reserve_host(self, nullifier_set, receipts, keys, rows, key_epochs, charges, raw: bool, bind=_UNBOUND):
        wire = isinstance(rows, (list, tuple))
        if wire:
            n = len(rows); p0, k0, offs = _msgs(rows); p = dict(cbor=p0, offsets=offs.ctypes.data)
        else:
            n = len(rows) // self.proof_bytes; p0, k0 = _in(rows, self.proof_bytes * n); p = dict(proofs=p0)
        if bind is not _UNBOUND:
            pb, kb = _in(bind, 32 * n) if bind is not None else (None, None)
            p.update(bind=pb)
        out = np.full(RESERVATION_BYTES * n, 7 if raw else 0, np.uint8); st = np.full(n, 99 if raw else 0, np.uint8); ok = np.zeros(n, np.uint8); rp = np.zeros(n, np.uint8)
        pc, kc = _in(charges, 32 * n) if charges is not None else (None, None)
        rc, counts = self.reserve_ptr("redeem_cbor" if wire else "redeem", keys, n, MEM_HOST, set=nullifier_set, receipts=receipts, key_epochs=key_epochs, charges=pc,
                                      out=out.ctypes.data, status=st.ctypes.data, out_key=ok.ctypes.data, replayed=rp.ctypes.data, raw=True, **p)
        res = (st.tobytes(), out.tobytes(), ok.tobytes(), rp.tobytes(), counts)
        if raw:
            return (rc,) + res
        self._ck(rc)
        return res

    def redeem_reserve(self, nullifier_set, receipts, keys, proofs: bytes, key_epochs=None, charges: bytes = None, raw: bool = False, bind=_UNBOUND):
        """redeem_admit_replay WITHOUT the signature: screen, verify, record k and a reservation tag.  -> (statuses, 96-byte reservation
        records k^ | enc(K') | s^ (zero where rejected), out_key, replayed, counts dict); raw=True: (rc, ...), no exception"""
        return self._reserve_host(nullifier_set, receipts, keys, proofs, key_epochs, charges, raw, bind)

    def redeem_cbor_reserve(self, nullifier_set, receipts, keys, messages: list, key_epochs=None, charges: bytes = None, raw: bool = False, bind=_UNBOUND):
        """SpendProof messages in -> what redeem_reserve returns (the reservation record has no wire type)"""
        return self._reserve_host(nullifier_set, receipts, keys, list(messages), key_epochs, charges, raw, bind)

    def settle_ptr(self, keys, n: int, mem: int, **p):
        """the settle calls on raw pointers of either kind; p: receipts, reservations (96 bytes a lane), key_index, amounts (0: all zero),
        nonce_key, out, status, settled_before, key_epochs, sign_key, cbor (the wire form), raw.  -> counts dict, or (rc, counts) with raw"""
        nk = len(keys); pk, kk = _in(b"".join(keys))
        ke = _epoch_table(p["key_epochs"], nk) if p.get("key_epochs") is not None else None
        pn, kn = _in(p["nonce_key"], 32) if p.get("nonce_key") is not None else (None, None)
        cnt = (C.c_uint64 * len(SETTLE_COUNTS))()
        fn = self.lib.act_redeem_cbor_settle_batch if p.get("cbor") else self.lib.act_redeem_settle_batch
        rc = fn(self.ctx, p["receipts"].h if p["receipts"] is not None else None, n, mem, pk, nk, ke.ctypes.data if ke is not None else None, p.get("sign_key", SIGN_MATCHED),
                p["reservations"], p["key_index"], p.get("amounts") or None, pn, p["out"], p["status"], p.get("settled_before") or None, cnt)
        counts = dict(zip(SETTLE_COUNTS, (int(v) for v in cnt)))
        if p.get("raw"):
            return rc, counts
        self._ck(rc)
        return counts

    def redeem_settle(self, receipts, keys, reservations: bytes, key_index: bytes, nonce_key: bytes, amounts: bytes = None, sign_key: int = SIGN_MATCHED, key_epochs=None,
                      cbor: bool = False, raw: bool = False):
        """reservation records and amounts t <= s in, RefundReturn out: the reservation is looked up, the amount pinned, the refund signed
        with derived nonces -- the same reservation with the same amount again gives the same bytes.  -> (statuses, 160-byte records |
        (cbor=True) list of RefundReturn messages (b"" where not signed), settled_before, counts dict); raw=True: (rc, ...), no exception"""
        n = len(key_index); ob = self.cbor_size("RefundReturn") if cbor else 160
        out = np.full(ob * n, 7 if raw and not cbor else 0, np.uint8); st = np.full(n, 99 if raw else 0, np.uint8); sb = np.zeros(n, np.uint8)
        p0, k0 = _in(reservations, RESERVATION_BYTES * n); p1, k1 = _in(key_index, n)
        pt, kt = _in(amounts, 32 * n) if amounts is not None else (None, None)
        rc, counts = self.settle_ptr(keys, n, MEM_HOST, receipts=receipts, reservations=p0, key_index=p1, amounts=pt, nonce_key=nonce_key, out=out.ctypes.data,
                                     status=st.ctypes.data, settled_before=sb.ctypes.data, key_epochs=key_epochs, sign_key=sign_key, cbor=cbor, raw=True)
        b = out.tobytes()
        res = (st.tobytes(), [b[i * ob:(i + 1) * ob] if st[i] == 0 else b"" for i in range(n)] if cbor else b, sb.tobytes(), counts)
        if raw:
            return (rc,) + res
        self._ck(rc)
        assert not cbor or all(st[i] == 0 or not out[i * ob:(i + 1) * ob].any() for i in range(n)), "a failed lane's slot is not zero"
        return res

    def copy_leaders(self, fps):
        """act_debug_copy_leaders: the leader table of the unique admission forms over made-up fingerprints -> (leaders, milliseconds)"""
        m = len(fps); a = np.asarray(fps, np.uint64); out = np.zeros(max(1, m), np.uint32); ms = C.c_double(0)
        self._ck(self.lib.act_debug_copy_leaders(self.ctx, m, a.ctypes.data_as(C.POINTER(C.c_uint64)), out.ctypes.data, C.byref(ms)))
        return out[:m].tolist(), ms.value

    # ---- issuance on wire bytes (act_issue_*cbor_batch): IssuanceRequest messages in, IssuanceResponse messages out ----------------
    def issue_cbor(self, sk: bytes, messages: list, c: bytes, rng, rng_mode: int = RNG_PER_LANE):
        """CBOR IssuanceRequest messages (byte strings of any length) -> (statuses, list of CBOR IssuanceResponse messages; b"" for a lane
        that was not signed)"""
        n = len(messages); p0, k0, offs = _msgs(messages); ml = self.cbor_size("IssuanceResponse")
        st = np.zeros(n, np.uint8); out = np.zeros(ml * n, np.uint8); ps, ks = _in(sk, 64); p1, k1 = _in(c, 32 * n); pr, kr = _rng_arg(rng)
        self._ck(self.lib.act_issue_cbor_batch(self.ctx, n, MEM_HOST, ps, p0, offs.ctypes.data, p1, pr, rng_mode, out.ctypes.data, st.ctypes.data))
        b = out.tobytes()
        assert all(st[i] == 0 or not out[i * ml:(i + 1) * ml].any() for i in range(n)), "a failed lane's slot is not zero"
        return st.tobytes(), [b[i * ml:(i + 1) * ml] if st[i] == 0 else b"" for i in range(n)]

    def issue_check_cbor(self, messages: list):
        """-> (statuses, requests as from_cbor returns them: n*128 bytes, zero where the status is not 0)"""
        n = len(messages); p0, k0, offs = _msgs(messages)
        st = np.zeros(n, np.uint8); req = np.zeros(128 * n, np.uint8)
        self._ck(self.lib.act_issue_check_cbor_batch(self.ctx, n, MEM_HOST, p0, offs.ctypes.data, st.ctypes.data, req.ctypes.data))
        return st.tobytes(), req.tobytes()

    def issue_sign_cbor(self, sk: bytes, req: bytes, c: bytes, status_in: bytes, rng, rng_mode: int = RNG_SEQUENTIAL):
        n = len(status_in); ml = self.cbor_size("IssuanceResponse"); st = np.zeros(n, np.uint8); out = np.zeros(ml * n, np.uint8)
        ps, ks = _in(sk, 64); p0, k0 = _in(req, 128 * n); p1, k1 = _in(c, 32 * n); p2, k2 = _in(status_in, n); pr, kr = _rng_arg(rng)
        self._ck(self.lib.act_issue_sign_cbor_batch(self.ctx, n, MEM_HOST, ps, p0, p1, p2, pr, rng_mode, out.ctypes.data, st.ctypes.data))
        b = out.tobytes()
        return st.tobytes(), [b[i * ml:(i + 1) * ml] if st[i] == 0 else b"" for i in range(n)]

    def issue_cbor_ptr(self, sk: bytes, n: int, mem: int, p_cbor: int, p_offsets: int, p_c: int, p_rng: int, rng_mode: int, p_out: int, p_status: int):
        """act_issue_cbor_batch on raw pointers of either kind (device-memory callers); p_offsets: host memory or 0"""
        ps, ks = _in(sk, 64)
        self._ck(self.lib.act_issue_cbor_batch(self.ctx, n, mem, ps, p_cbor, p_offsets or None, p_c, p_rng, rng_mode, p_out, p_status))

    def issue_check_cbor_ptr(self, n: int, mem: int, p_cbor: int, p_offsets: int, p_status: int, p_req: int = 0):
        self._ck(self.lib.act_issue_check_cbor_batch(self.ctx, n, mem, p_cbor, p_offsets or None, p_status, p_req or None))

    def issue_sign_cbor_ptr(self, sk: bytes, n: int, mem: int, p_req: int, p_c: int, p_status_in: int, p_rng: int, rng_mode: int, p_out: int, p_status: int):
        ps, ks = _in(sk, 64)
        self._ck(self.lib.act_issue_sign_cbor_batch(self.ctx, n, mem, ps, p_req, p_c, p_status_in, p_rng, rng_mode, p_out, p_status))

    def host_hash_stats(self, reset: bool = False) -> dict:
        """host-transcript mode: seconds the calling thread waited for transcripts / hashed them, bytes hashed, since the last reset"""
        w, hs, b = C.c_double(0), C.c_double(0), C.c_uint64(0)
        self._ck(self.lib.act_ctx_host_hash_stats(self.ctx, C.byref(w), C.byref(hs), C.byref(b), 1 if reset else 0))
        return {"wait_s": w.value, "hash_s": hs.value, "bytes": b.value}

    def set_tiny_calls(self, on: bool):
        """calls of at most 64 lanes as one kernel with the transcript hashed in it (default) or the multi-launch paths"""
        self._ck(self.lib.act_ctx_set_tiny_calls(self.ctx, 1 if on else 0))

    def set_slowdown(self, ns_per_lane: int):
        self._ck(self.lib.act_debug_set_slowdown(self.ctx, ns_per_lane))

    # ---- device-memory batch calls (raw device pointers) -----------------------------------------
    def verify_spend_dev(self, sk: bytes, n: int, d_proofs: int, d_status: int, d_kprime: int = 0):
        ps, ks = _in(sk, 64)
        self._ck(self.lib.act_verify_spend_batch(self.ctx, n, MEM_DEVICE, ps, d_proofs, d_status, d_kprime or None))

    def verify_spend_ptr(self, sk: bytes, n: int, mem: int, p_proofs: int, p_status: int, p_kprime: int = 0):
        """Raw pointers of either kind (mem = MEM_HOST for e.g. pinned host buffers, MEM_DEVICE for HBM)."""
        ps, ks = _in(sk, 64)
        self._ck(self.lib.act_verify_spend_batch(self.ctx, n, mem, ps, p_proofs, p_status, p_kprime or None))

    def refund_dev(self, sk: bytes, n: int, d_proofs: int, d_rng: int, rng_mode: int, d_out: int, d_status: int):
        ps, ks = _in(sk, 64)
        self._ck(self.lib.act_refund_batch(self.ctx, n, MEM_DEVICE, ps, d_proofs, d_rng, rng_mode, d_out, d_status))

    def prove_spend_dev(self, n: int, d_tok: int, d_s: int, d_rng: int, d_proof: int, d_prerefund: int, d_status: int):
        self._ck(self.lib.act_prove_spend_batch(self.ctx, n, MEM_DEVICE, d_tok, d_s, d_rng, d_proof, d_prerefund, d_status))

    def issue_dev(self, sk: bytes, n: int, d_req: int, d_c: int, d_rng: int, rng_mode: int, d_out: int, d_status: int):
        ps, ks = _in(sk, 64)
        self._ck(self.lib.act_issue_batch(self.ctx, n, MEM_DEVICE, ps, d_req, d_c, d_rng, rng_mode, d_out, d_status))

    def request_dev(self, n: int, d_pre: int, d_rng: int, d_out: int):
        self._ck(self.lib.act_request_batch(self.ctx, n, MEM_DEVICE, d_pre, d_rng, d_out))

    def pre_issuance_random_dev(self, n: int, d_rng: int, d_out: int):
        self._ck(self.lib.act_pre_issuance_random_batch(self.ctx, n, MEM_DEVICE, d_rng, d_out))

    def issuance_to_credit_token_dev(self, n: int, d_pre: int, w: bytes, d_req: int, d_resp: int, d_tok: int, d_status: int):
        pw, kw = _in(w, 32)
        self._ck(self.lib.act_issuance_to_credit_token_batch(self.ctx, n, MEM_DEVICE, d_pre, pw, d_req, d_resp, d_tok, d_status))

    # ---- profiling ---------------------------------------------------------------------------------
    def prof_enable(self, on: bool = True):
        self._ck(self.lib.act_prof_enable(self.ctx, 1 if on else 0))

    def prof_reset(self):
        self._ck(self.lib.act_prof_reset(self.ctx))

    def prof(self) -> dict:
        out = {}
        for i in range(self.lib.act_prof_kernel_count(self.ctx)):
            ms, la, ln = C.c_double(0), C.c_uint64(0), C.c_uint64(0)
            self._ck(self.lib.act_prof_get(self.ctx, i, C.byref(ms), C.byref(la), C.byref(ln)))
            if la.value:
                busy = C.c_double(0)
                self._ck(self.lib.act_prof_get_busy(self.ctx, i, C.byref(busy)))
                out[self.lib.act_prof_kernel_name(self.ctx, i).decode()] = {"ms": ms.value, "busy_ms": busy.value, "launches": la.value, "lanes": ln.value}
        return out


class Node:
    """The GPUs of one node behind one handle (act_node_*): contiguous shards, one context and host thread per entry of
    `devices`, outputs in the matching slices; ACT_RNG_SEQUENTIAL exact across shards.  Host memory (bytes) only."""

    def __init__(self, h: bytes, L: int = 128, devices=(0,), max_batch: int = 0, transcript: int = TRANSCRIPT_HOST):
        self.lib = load()
        self.L = L
        nd = C.c_void_p()
        p, keep = _in(h, 96)
        devs = (C.c_int * len(devices))(*devices)
        rc = self.lib.act_node_create(p, L, devs, len(devices), max_batch, C.byref(nd))
        if rc:
            msg = self.lib.act_node_last_error(nd).decode() if nd else ""
            if nd:
                self.lib.act_node_destroy(nd)
            raise ActError(f"act_node_create failed: {_ERRS.get(rc, rc)} {msg}")
        self.nd = nd
        c0 = self.lib.act_node_ctx(nd, 0)
        self.proof_bytes = self.lib.act_spend_proof_bytes(c0)
        self.prove_rng_bytes = self.lib.act_prove_rng_bytes(c0)
        self._ck(self.lib.act_node_set_transcript_mode(nd, transcript))

    def close(self):
        if getattr(self, "nd", None):
            self.lib.act_node_destroy(self.nd)
            self.nd = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc:
            raise ActError(f"{_ERRS.get(rc, rc)}: {self.lib.act_node_last_error(self.nd).decode()}")

    def device_count(self) -> int:
        return self.lib.act_node_device_count(self.nd)

    def set_transcript_mode(self, mode: int):
        self._ck(self.lib.act_node_set_transcript_mode(self.nd, mode))

    def set_host_threads(self, per_gpu: int):
        self._ck(self.lib.act_node_set_host_threads(self.nd, per_gpu))

    def set_fixed_base_bits(self, base: int, bits: int):
        self._ck(self.lib.act_node_set_fixed_base_bits(self.nd, base, bits))

    def streams_overlap(self) -> list:
        return [self.lib.act_ctx_streams_overlap(self.lib.act_node_ctx(self.nd, k)) for k in range(self.device_count())]

    def request(self, pre: bytes, rng: bytes) -> bytes:
        n = len(pre) // 64; out = np.zeros(128 * n, np.uint8)
        p0, k0 = _in(pre, 64 * n); p1, k1 = _in(rng, 128 * n)
        self._ck(self.lib.act_node_request_batch(self.nd, n, p0, p1, out.ctypes.data)); return out.tobytes()

    def issue(self, sk: bytes, req: bytes, c: bytes, rng: bytes, rng_mode: int = RNG_PER_LANE):
        n = len(req) // 128; out = np.zeros(160 * n, np.uint8); st = np.zeros(n, np.uint8)
        ps, ks = _in(sk, 64); p0, k0 = _in(req, 128 * n); p1, k1 = _in(c, 32 * n); p2, k2 = _in(rng)
        self._ck(self.lib.act_node_issue_batch(self.nd, n, ps, p0, p1, p2, rng_mode, out.ctypes.data, st.ctypes.data))
        return st.tobytes(), out.tobytes()

    def issuance_to_credit_token(self, pre: bytes, w: bytes, req: bytes, resp: bytes):
        n = len(pre) // 64; out = np.zeros(160 * n, np.uint8); st = np.zeros(n, np.uint8)
        p0, k0 = _in(pre, 64 * n); pw, kw = _in(w, 32); p1, k1 = _in(req, 128 * n); p2, k2 = _in(resp, 160 * n)
        self._ck(self.lib.act_node_issuance_to_credit_token_batch(self.nd, n, p0, pw, p1, p2, out.ctypes.data, st.ctypes.data))
        return st.tobytes(), out.tobytes()

    def prove_spend(self, tok: bytes, s: bytes, rng: bytes):
        n = len(tok) // 160; out = np.zeros(self.proof_bytes * n, np.uint8); pr = np.zeros(96 * n, np.uint8); st = np.zeros(n, np.uint8)
        p0, k0 = _in(tok, 160 * n); p1, k1 = _in(s, 32 * n); p2, k2 = _in(rng, self.prove_rng_bytes * n)
        self._ck(self.lib.act_node_prove_spend_batch(self.nd, n, p0, p1, p2, out.ctypes.data, pr.ctypes.data, st.ctypes.data))
        return st.tobytes(), out.tobytes(), pr.tobytes()

    def prove_spend_seeded(self, tok: bytes, s: bytes, seed: bytes, first_lane: int = 0):
        n = len(tok) // 160; out = np.zeros(self.proof_bytes * n, np.uint8); pr = np.zeros(96 * n, np.uint8); st = np.zeros(n, np.uint8)
        p0, k0 = _in(tok, 160 * n); p1, k1 = _in(s, 32 * n); p2, k2 = _in(seed, 32)
        self._ck(self.lib.act_node_prove_spend_seeded_batch(self.nd, n, p0, p1, p2, first_lane, out.ctypes.data, pr.ctypes.data, st.ctypes.data))
        return st.tobytes(), out.tobytes(), pr.tobytes()

    def verify_spend(self, sk: bytes, proofs: bytes, want_kprime: bool = False):
        n = len(proofs) // self.proof_bytes; st = np.zeros(n, np.uint8)
        kp = np.zeros(32 * n, np.uint8) if want_kprime else None
        ps, ks = _in(sk, 64); p0, k0 = _in(proofs, self.proof_bytes * n)
        self._ck(self.lib.act_node_verify_spend_batch(self.nd, n, ps, p0, st.ctypes.data, kp.ctypes.data if want_kprime else None))
        return (st.tobytes(), kp.tobytes()) if want_kprime else st.tobytes()

    def verify_spend_ptr(self, sk: bytes, n: int, p_proofs: int, p_status: int, p_kprime: int = 0):
        """Raw HOST pointers (pageable or pinned): the call a Rust caller's slices turn into."""
        ps, ks = _in(sk, 64)
        self._ck(self.lib.act_node_verify_spend_batch(self.nd, n, ps, p_proofs, p_status, p_kprime or None))

    def refund(self, sk: bytes, proofs: bytes, rng: bytes, rng_mode: int = RNG_PER_LANE):
        n = len(proofs) // self.proof_bytes; out = np.zeros(128 * n, np.uint8); st = np.zeros(n, np.uint8)
        ps, ks = _in(sk, 64); p0, k0 = _in(proofs, self.proof_bytes * n); p1, k1 = _in(rng)
        self._ck(self.lib.act_node_refund_batch(self.nd, n, ps, p0, p1, rng_mode, out.ctypes.data, st.ctypes.data))
        return st.tobytes(), out.tobytes()

    def redeem(self, nullifier_set, sk: bytes, proofs: bytes, rng: bytes, rng_mode: int = RNG_SEQUENTIAL):
        n = len(proofs) // self.proof_bytes; out = np.zeros(128 * n, np.uint8); st = np.zeros(n, np.uint8)
        ps, ks = _in(sk, 64); p0, k0 = _in(proofs, self.proof_bytes * n); p1, k1 = _rng_arg(rng)
        self._ck(self.lib.act_node_redeem_batch(self.nd, nullifier_set.h, n, ps, p0, p1, rng_mode, out.ctypes.data, st.ctypes.data))
        return st.tobytes(), out.tobytes()

    def refund_sign(self, sk: bytes, kprime: bytes, status_in: bytes, rng: bytes, rng_mode: int = RNG_SEQUENTIAL):
        n = len(status_in); out = np.zeros(128 * n, np.uint8); st = np.zeros(n, np.uint8)
        ps, ks = _in(sk, 64); p0, k0 = _in(kprime, 32 * n); p1, k1 = _in(status_in, n); p2, k2 = _in(rng)
        self._ck(self.lib.act_node_refund_sign_batch(self.nd, n, ps, p0, p1, p2, rng_mode, out.ctypes.data, st.ctypes.data))
        return st.tobytes(), out.tobytes()

    def issue_check(self, req: bytes) -> bytes:
        n = len(req) // 128; st = np.zeros(n, np.uint8); p0, k0 = _in(req, 128 * n)
        self._ck(self.lib.act_node_issue_check_batch(self.nd, n, p0, st.ctypes.data)); return st.tobytes()

    def issue_sign(self, sk: bytes, req: bytes, c: bytes, status_in: bytes, rng: bytes, rng_mode: int = RNG_SEQUENTIAL):
        n = len(status_in); out = np.zeros(160 * n, np.uint8); st = np.zeros(n, np.uint8)
        ps, ks = _in(sk, 64); p0, k0 = _in(req, 128 * n); p1, k1 = _in(c, 32 * n); p2, k2 = _in(status_in, n); p3, k3 = _in(rng)
        self._ck(self.lib.act_node_issue_sign_batch(self.nd, n, ps, p0, p1, p2, p3, rng_mode, out.ctypes.data, st.ctypes.data))
        return st.tobytes(), out.tobytes()

    def refund_to_credit_token(self, prerefund: bytes, proofs: bytes, refund: bytes, w: bytes):
        n = len(prerefund) // 96; out = np.zeros(160 * n, np.uint8); st = np.zeros(n, np.uint8)
        p0, k0 = _in(prerefund, 96 * n); p1, k1 = _in(proofs, self.proof_bytes * n); p2, k2 = _in(refund, 128 * n); pw, kw = _in(w, 32)
        self._ck(self.lib.act_node_refund_to_credit_token_batch(self.nd, n, p0, p1, p2, pw, out.ctypes.data, st.ctypes.data))
        return st.tobytes(), out.tobytes()


    def _wire(self, messages):
        p0, k0, offs = _msgs(messages)
        return p0, k0, offs, self.lib.act_cbor_size(self.lib.act_node_ctx(self.nd, 0), CBOR_TYPES["Refund"])

    def verify_spend_cbor_keys(self, sk: bytes, messages: list):
        n = len(messages); p0, k0, offs = _msgs(messages)
        st = np.zeros(n, np.uint8); kp = np.zeros(32 * n, np.uint8); nul = np.zeros(32 * n, np.uint8); ps, ks = _in(sk, 64)
        self._ck(self.lib.act_node_verify_spend_cbor_keys_batch(self.nd, n, ps, p0, offs.ctypes.data, st.ctypes.data, kp.ctypes.data, nul.ctypes.data))
        return st.tobytes(), kp.tobytes(), nul.tobytes()

    def refund_cbor(self, sk: bytes, messages: list, rng, rng_mode: int = RNG_SEQUENTIAL):
        n = len(messages); p0, k0, offs, ml = self._wire(messages)
        st = np.zeros(n, np.uint8); out = np.zeros(ml * n, np.uint8); ps, ks = _in(sk, 64); pr, kr = _rng_arg(rng)
        self._ck(self.lib.act_node_refund_cbor_batch(self.nd, n, ps, p0, offs.ctypes.data, pr, rng_mode, out.ctypes.data, st.ctypes.data))
        b = out.tobytes()
        return st.tobytes(), [b[i * ml:(i + 1) * ml] if st[i] == 0 else b"" for i in range(n)]

    def refund_sign_cbor(self, sk: bytes, kprime: bytes, status_in: bytes, rng, rng_mode: int = RNG_SEQUENTIAL):
        n = len(status_in); ml = self.lib.act_cbor_size(self.lib.act_node_ctx(self.nd, 0), CBOR_TYPES["Refund"])
        st = np.zeros(n, np.uint8); out = np.zeros(ml * n, np.uint8)
        ps, ks = _in(sk, 64); p0, k0 = _in(kprime, 32 * n); p1, k1 = _in(status_in, n); pr, kr = _rng_arg(rng)
        self._ck(self.lib.act_node_refund_sign_cbor_batch(self.nd, n, ps, p0, p1, pr, rng_mode, out.ctypes.data, st.ctypes.data))
        b = out.tobytes()
        return st.tobytes(), [b[i * ml:(i + 1) * ml] if st[i] == 0 else b"" for i in range(n)]

    def redeem_cbor(self, nullifier_set, sk: bytes, messages: list, rng, rng_mode: int = RNG_SEQUENTIAL):
        n = len(messages); p0, k0, offs, ml = self._wire(messages)
        st = np.zeros(n, np.uint8); out = np.zeros(ml * n, np.uint8); ps, ks = _in(sk, 64); pr, kr = _rng_arg(rng)
        self._ck(self.lib.act_node_redeem_cbor_batch(self.nd, nullifier_set.h, n, ps, p0, offs.ctypes.data, pr, rng_mode, out.ctypes.data, st.ctypes.data))
        b = out.tobytes()
        return st.tobytes(), [b[i * ml:(i + 1) * ml] if st[i] == 0 else b"" for i in range(n)]

    # ---- key rotation over the node's GPUs (act_node_*_keyring_batch) ---------------------------------------------------------
    def verify_spend_keyring(self, keys, proofs: bytes, want_kprime: bool = False):
        n = len(proofs) // self.proof_bytes; st = np.zeros(n, np.uint8); ok = np.zeros(n, np.uint8)
        kp = np.zeros(32 * n, np.uint8) if want_kprime else None
        pk, kk = _in(b"".join(keys)); p0, k0 = _in(proofs, self.proof_bytes * n)
        self._ck(self.lib.act_node_verify_spend_keyring_batch(self.nd, n, pk, len(keys), p0, st.ctypes.data, ok.ctypes.data, kp.ctypes.data if want_kprime else None))
        return (st.tobytes(), ok.tobytes(), kp.tobytes()) if want_kprime else (st.tobytes(), ok.tobytes())

    def refund_sign_keyring(self, keys, key_index: bytes, kprime: bytes, status_in: bytes, rng: bytes, rng_mode: int = RNG_SEQUENTIAL):
        n = len(status_in); out = np.zeros(128 * n, np.uint8); st = np.zeros(n, np.uint8)
        pk, kk = _in(b"".join(keys)); pi, ki = _in(key_index, n); p0, k0 = _in(kprime, 32 * n); p1, k1 = _in(status_in, n); p2, k2 = _in(rng)
        self._ck(self.lib.act_node_refund_sign_keyring_batch(self.nd, n, pk, len(keys), pi, p0, p1, p2, rng_mode, out.ctypes.data, st.ctypes.data))
        return st.tobytes(), out.tobytes()

    def redeem_keyring(self, nullifier_set, keys, proofs: bytes, rng, rng_mode: int = RNG_SEQUENTIAL, sign_key: int = SIGN_MATCHED, raw: bool = False,
                       key_epochs=None):
        n = len(proofs) // self.proof_bytes; out = np.full(128 * n, 7 if raw else 0, np.uint8); st = np.zeros(n, np.uint8); ok = np.zeros(n, np.uint8)
        pk, kk = _in(b"".join(keys)); p0, k0 = _in(proofs, self.proof_bytes * n); p1, k1 = _rng_arg(rng)
        if key_epochs is not None:
            ke = _epoch_table(key_epochs, len(keys))
            rc = self.lib.act_node_redeem_keyring_epochs_batch(self.nd, nullifier_set.h, n, pk, len(keys), ke.ctypes.data, sign_key, p0, p1, rng_mode,
                                                               out.ctypes.data, st.ctypes.data, ok.ctypes.data)
        else:
            rc = self.lib.act_node_redeem_keyring_batch(self.nd, nullifier_set.h, n, pk, len(keys), sign_key, p0, p1, rng_mode, out.ctypes.data, st.ctypes.data, ok.ctypes.data)
        if raw:
            return rc, st.tobytes(), out.tobytes(), ok.tobytes()
        self._ck(rc)
        return st.tobytes(), out.tobytes(), ok.tobytes()

    def redeem_cbor_keyring(self, nullifier_set, keys, messages: list, rng, rng_mode: int = RNG_SEQUENTIAL, sign_key: int = SIGN_MATCHED, key_epochs=None):
        n = len(messages); p0, k0, offs, ml = self._wire(messages)
        st = np.zeros(n, np.uint8); ok = np.zeros(n, np.uint8); out = np.zeros(ml * n, np.uint8); pk, kk = _in(b"".join(keys)); pr, kr = _rng_arg(rng)
        if key_epochs is not None:
            ke = _epoch_table(key_epochs, len(keys))
            self._ck(self.lib.act_node_redeem_cbor_keyring_epochs_batch(self.nd, nullifier_set.h, n, pk, len(keys), ke.ctypes.data, sign_key, p0, offs.ctypes.data,
                                                                        pr, rng_mode, out.ctypes.data, st.ctypes.data, ok.ctypes.data))
        else:
            self._ck(self.lib.act_node_redeem_cbor_keyring_batch(self.nd, nullifier_set.h, n, pk, len(keys), sign_key, p0, offs.ctypes.data, pr, rng_mode,
                                                                 out.ctypes.data, st.ctypes.data, ok.ctypes.data))
        b = out.tobytes()
        return st.tobytes(), [b[i * ml:(i + 1) * ml] if st[i] == 0 else b"" for i in range(n)], ok.tobytes()

    def issue_cbor(self, sk: bytes, messages: list, c: bytes, rng, rng_mode: int = RNG_SEQUENTIAL):
        n = len(messages); p0, k0, offs = _msgs(messages)
        ml = self.lib.act_cbor_size(self.lib.act_node_ctx(self.nd, 0), CBOR_TYPES["IssuanceResponse"])
        st = np.zeros(n, np.uint8); out = np.zeros(ml * n, np.uint8); ps, ks = _in(sk, 64); p1, k1 = _in(c, 32 * n); pr, kr = _rng_arg(rng)
        self._ck(self.lib.act_node_issue_cbor_batch(self.nd, n, ps, p0, offs.ctypes.data, p1, pr, rng_mode, out.ctypes.data, st.ctypes.data))
        b = out.tobytes()
        return st.tobytes(), [b[i * ml:(i + 1) * ml] if st[i] == 0 else b"" for i in range(n)]

    def issue_check_cbor(self, messages: list):
        n = len(messages); p0, k0, offs = _msgs(messages)
        st = np.zeros(n, np.uint8); req = np.zeros(128 * n, np.uint8)
        self._ck(self.lib.act_node_issue_check_cbor_batch(self.nd, n, p0, offs.ctypes.data, st.ctypes.data, req.ctypes.data))
        return st.tobytes(), req.tobytes()

    def issue_sign_cbor(self, sk: bytes, req: bytes, c: bytes, status_in: bytes, rng, rng_mode: int = RNG_SEQUENTIAL):
        n = len(status_in); ml = self.lib.act_cbor_size(self.lib.act_node_ctx(self.nd, 0), CBOR_TYPES["IssuanceResponse"])
        st = np.zeros(n, np.uint8); out = np.zeros(ml * n, np.uint8)
        ps, ks = _in(sk, 64); p0, k0 = _in(req, 128 * n); p1, k1 = _in(c, 32 * n); p2, k2 = _in(status_in, n); pr, kr = _rng_arg(rng)
        self._ck(self.lib.act_node_issue_sign_cbor_batch(self.nd, n, ps, p0, p1, p2, pr, rng_mode, out.ctypes.data, st.ctypes.data))
        b = out.tobytes()
        return st.tobytes(), [b[i * ml:(i + 1) * ml] if st[i] == 0 else b"" for i in range(n)]

    def set_balance(self, weighted: bool = True, tail_64ths: int = -1):
        self._ck(self.lib.act_node_set_balance(self.nd, 1 if weighted else 0, tail_64ths))

    def device_stats(self) -> list:
        """per context: weight (relative speed, mean 1) and what the most recent cut call gave it"""
        out = []
        for k in range(self.device_count()):
            w, s = C.c_double(0), C.c_double(0); la, ca = C.c_uint64(0), C.c_uint64(0)
            self._ck(self.lib.act_node_device_stats(self.nd, k, C.byref(w), C.byref(la), C.byref(s), C.byref(ca)))
            out.append({"weight": w.value, "lanes": la.value, "seconds": s.value, "calls": ca.value})
        return out

    def balance_state(self) -> dict:
        sp, tf = C.c_double(0), C.c_double(0)
        self._ck(self.lib.act_node_balance_state(self.nd, C.byref(sp), C.byref(tf)))
        return {"spread": sp.value, "tail_fraction": tf.value}

    def ctx_handle(self, k: int):
        return self.lib.act_node_ctx(self.nd, k)


class NullifierSet:
    """GPU double-spend set with the sequential meaning of the reference tests' NullifierDb (src/tests.rs:29-50)."""

    def __init__(self, capacity: int, device: int = 0, salt: bytes = None):
        self.lib = load()
        h = C.c_void_p()
        p, keep = _in(salt, 16) if salt else (None, None)
        rc = self.lib.act_nullifier_set_create(device, capacity, p, C.byref(h))
        if rc:
            raise ActError(f"act_nullifier_set_create failed: {_ERRS.get(rc, rc)}")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.act_nullifier_set_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return self.lib.act_nullifier_set_len(self.h)

    def _ck(self, rc):
        if rc:
            raise ActError(f"{_ERRS.get(rc, rc)}: {self.lib.act_nullifier_set_last_error(self.h).decode()}")

    def check_and_insert(self, nullifiers: bytes, stride: int = 32, skip_mask: bytes = None, epoch_index: bytes = None, epochs=None, raw: bool = False):
        """epochs (a list of 1 .. 255 epochs) / epoch_index (one byte per lane, an index into it; None = every lane epochs[0]): a fresh
        lane is recorded under epochs[epoch_index[i]] (act_nullifier_check_and_insert_epoch_batch); neither = untagged, the existing
        call.  raw=True: (rc, answers), no exception (a lane with an index outside the table is answered 2 beside the others)."""
        n = (len(nullifiers) + stride - 32) // stride if nullifiers else 0
        out = np.zeros(n, np.uint8)
        p0, k0 = _in(nullifiers); pm, km = _in(skip_mask, n) if skip_mask is not None else (None, None)
        if epochs is None and epoch_index is None:
            rc = self.lib.act_nullifier_check_and_insert_batch(self.h, n, MEM_HOST, p0, stride, pm, out.ctypes.data)
        else:
            tab = _epoch_table(epochs if epochs is not None else [0]); pe, ke = _in(epoch_index, n) if epoch_index is not None else (None, None)
            rc = self.lib.act_nullifier_check_and_insert_epoch_batch(self.h, n, MEM_HOST, p0, stride, pm, pe, tab.ctypes.data, len(tab), out.ctypes.data)
        if raw:
            return rc, out.tobytes()
        self._ck(rc)
        return out.tobytes()

    def check_and_insert_dev(self, n: int, d_nullifiers: int, stride: int, d_skip_mask: int, d_out_spent: int):
        self._ck(self.lib.act_nullifier_check_and_insert_batch(self.h, n, MEM_DEVICE, d_nullifiers, stride, d_skip_mask or None, d_out_spent))

    def check_and_insert_epoch_dev(self, n: int, d_nullifiers: int, stride: int, d_skip_mask: int, d_epoch_index: int, epochs, d_out_spent: int, raw: bool = False):
        """device pointers; `epochs` is the (host) table"""
        tab = _epoch_table(epochs)
        rc = self.lib.act_nullifier_check_and_insert_epoch_batch(self.h, n, MEM_DEVICE, d_nullifiers, stride, d_skip_mask or None, d_epoch_index or None,
                                                                 tab.ctypes.data, len(tab), d_out_spent)
        if raw:
            return rc
        self._ck(rc)

    # ---- epochs: count, retire, list, export with epochs (include/act_mi355x.h "Epochs") ----
    def epoch_len(self, epoch: int) -> int:
        c = C.c_uint64(0)
        self._ck(self.lib.act_nullifier_set_epoch_len(self.h, epoch, C.byref(c)))
        return c.value

    def retire_epoch(self, epoch: int) -> int:
        """remove every nullifier recorded under `epoch` and refuse the epoch from then on -> how many were removed.  Only for a key that
        has left every ring of every server sharing the set, for good."""
        c = C.c_uint64(0)
        self._ck(self.lib.act_nullifier_set_retire_epoch(self.h, epoch, C.byref(c)))
        return c.value

    def retired_epochs(self) -> list:
        return _retired_list(lambda p, m, n: self._ck(self.lib.act_nullifier_set_retired_epochs(self.h, p, m, n)))

    def export_epochs_step(self, cursor: int, max_keys: int):
        """one export call into host memory -> (next cursor, keys bytes, epochs as a uint32 array)"""
        out = np.empty(32 * max_keys, np.uint8); ep = np.empty(max_keys, np.uint32); cur = C.c_uint64(cursor); got = C.c_size_t(0)
        self._ck(self.lib.act_nullifier_set_export_epochs(self.h, C.byref(cur), max_keys, MEM_HOST, out.ctypes.data, ep.ctypes.data, C.byref(got)))
        return cur.value, out[:32 * got.value].tobytes(), ep[:got.value].copy()

    def export_epochs_dev(self, cursor: int, max_keys: int, d_out_keys: int, d_out_epochs: int):
        cur = C.c_uint64(cursor); got = C.c_size_t(0)
        self._ck(self.lib.act_nullifier_set_export_epochs(self.h, C.byref(cur), max_keys, MEM_DEVICE, d_out_keys, d_out_epochs, C.byref(got)))
        return cur.value, got.value

    def export_epochs(self, max_keys: int = 1 << 20):
        """every recorded nullifier with its epoch -> (keys bytes, uint32 array), unspecified order"""
        return _export_epochs_loop(self.export_epochs_step, max_keys)

    # ---- growth, export, read-only look-up, snapshots (include/act_mi355x.h; nullifier_snapshot.py) ----
    def reserve(self, capacity: int):
        """grow so that `capacity` nullifiers fit (keys rehashed on the device; never shrinks)"""
        self._ck(self.lib.act_nullifier_set_reserve(self.h, capacity))

    def contains(self, nullifiers: bytes, stride: int = 32) -> bytes:
        """read-only: 1 per recorded nullifier, else 0.  Audit and status queries only -- a spend decision is check_and_insert."""
        n = (len(nullifiers) + stride - 32) // stride if nullifiers else 0
        out = np.zeros(n, np.uint8); p0, k0 = _in(nullifiers)
        self._ck(self.lib.act_nullifier_contains_batch(self.h, n, MEM_HOST, p0, stride, out.ctypes.data))
        return out.tobytes()

    def contains_dev(self, n: int, d_nullifiers: int, stride: int, d_out_found: int):
        self._ck(self.lib.act_nullifier_contains_batch(self.h, n, MEM_DEVICE, d_nullifiers, stride, d_out_found))

    def export_step(self, cursor: int, max_keys: int, out: np.ndarray = None):
        """one export call into host memory (`out`: a reusable uint8 buffer of at least 32*max_keys bytes): -> (next cursor, keys bytes)"""
        out = _export_buffer(out, max_keys); cur = C.c_uint64(cursor); got = C.c_size_t(0)
        self._ck(self.lib.act_nullifier_set_export(self.h, C.byref(cur), max_keys, MEM_HOST, out.ctypes.data, C.byref(got)))
        return cur.value, out[:32 * got.value].tobytes()

    def export_dev(self, cursor: int, max_keys: int, d_out_keys: int):
        """one export call into device memory (room for max_keys keys at d_out_keys): -> (next cursor, keys written)"""
        cur = C.c_uint64(cursor); got = C.c_size_t(0)
        self._ck(self.lib.act_nullifier_set_export(self.h, C.byref(cur), max_keys, MEM_DEVICE, d_out_keys, C.byref(got)))
        return cur.value, got.value

    def export(self, max_keys: int = 1 << 20) -> bytes:
        """every recorded nullifier (reduced, 32 bytes each, unspecified order)"""
        return _export_loop(self.export_step, max_keys)

    def save(self, path: str) -> int:
        """format v2 when the set holds a non-zero epoch or a retired epoch, else today's v1 bytes (nullifier_snapshot.py)"""
        from . import nullifier_snapshot
        keys, epochs = self.export_epochs()
        return nullifier_snapshot.write_epochs(path, keys, epochs, self.retired_epochs())

    @classmethod
    def restore(cls, path: str, capacity: int = None, device: int = 0, salt: bytes = None) -> "NullifierSet":
        """a new set holding the snapshot's keys, their epochs and its retired list (validated as a whole before anything is inserted)"""
        from . import nullifier_snapshot
        keys, epochs, retired = nullifier_snapshot.read_epochs(path)
        s = cls(max(capacity or 0, len(keys) // 32, 1), device=device, salt=salt)
        nullifier_snapshot.restore_epochs_into(s, keys, epochs, retired)
        return s


class NodeNullifierSet:
    """The double-spend set over the GPUs of a node (act_node_nullifier_*): host-side routing by owner, one set per device."""

    def __init__(self, capacity_per_device: int, devices=(0,), salt: bytes = None):
        self.lib = load()
        h = C.c_void_p()
        devs = (C.c_int * len(devices))(*devices)
        p, keep = _in(salt, 16) if salt else (None, None)
        rc = self.lib.act_node_nullifier_set_create(devs, len(devices), capacity_per_device, p, C.byref(h))
        if rc:
            msg = self.lib.act_node_nullifier_set_last_error(h).decode() if h else ""
            if h:
                self.lib.act_node_nullifier_set_destroy(h)
            raise ActError(f"act_node_nullifier_set_create failed: {_ERRS.get(rc, rc)} {msg}")
        self.h = h
        self.n_devices = len(devices)
        self.capacity_per_device = capacity_per_device    # what every device was created or reserved for (reserve only grows it)

    def close(self):
        if getattr(self, "h", None):
            self.lib.act_node_nullifier_set_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return self.lib.act_node_nullifier_set_len(self.h)

    def check_and_insert(self, nullifiers: bytes, stride: int = 32, skip_mask: bytes = None, epoch_index: bytes = None, epochs=None, raw: bool = False):
        n = (len(nullifiers) + stride - 32) // stride if nullifiers else 0
        out = np.zeros(n, np.uint8)
        p0, k0 = _in(nullifiers); pm, km = _in(skip_mask, n) if skip_mask is not None else (None, None)
        if epochs is None and epoch_index is None:
            rc = self.lib.act_node_nullifier_check_and_insert_batch(self.h, n, p0, stride, pm, out.ctypes.data)
        else:
            tab = _epoch_table(epochs if epochs is not None else [0]); pe, ke = _in(epoch_index, n) if epoch_index is not None else (None, None)
            rc = self.lib.act_node_nullifier_check_and_insert_epoch_batch(self.h, n, p0, stride, pm, pe, tab.ctypes.data, len(tab), out.ctypes.data)
        if raw:
            return rc, out.tobytes()
        if rc:
            raise ActError(f"{_ERRS.get(rc, rc)}: {self.lib.act_node_nullifier_set_last_error(self.h).decode()}")
        return out.tobytes()

    def _ck(self, rc):
        if rc:
            raise ActError(f"{_ERRS.get(rc, rc)}: {self.lib.act_node_nullifier_set_last_error(self.h).decode()}")

    def reserve(self, capacity_per_device: int):
        self._ck(self.lib.act_node_nullifier_set_reserve(self.h, capacity_per_device))
        self.capacity_per_device = max(self.capacity_per_device, capacity_per_device)

    def restore_capacity(self, n: int) -> int:
        """per-device capacity for what the set holds plus n more keys.  Owners are a keyed hash, so a device receives about
        1/devices of them; the margin (1/8 + 4 standard deviations + 1024) makes a device that still runs full rare, and
        check_and_insert_growing grows it when it happens."""
        per = -(-(len(self) + n) // self.n_devices)
        return per + per // 8 + 4 * math.isqrt(per) + 1024

    def check_and_insert_growing(self, nullifiers: bytes, epoch: int = 0) -> bytes:
        """check_and_insert of 32-byte keys that, when a device refuses its bucket for capacity (its lanes come back
        ACT_NULLIFIER_UNDETERMINED, nothing of them recorded; the other devices' answers are final), doubles the per-device
        capacity and resubmits exactly those lanes.  Restore's path: no device count or key spread can make it fail."""
        n = len(nullifiers) // 32
        keys = np.frombuffer(nullifiers, np.uint8).reshape(n, 32)
        answer, lanes = np.zeros(n, np.uint8), np.arange(n)
        while True:
            sub = np.ascontiguousarray(keys[lanes]); out = np.zeros(len(lanes), np.uint8)
            if epoch:
                tab = _epoch_table([epoch])
                rc = self.lib.act_node_nullifier_check_and_insert_epoch_batch(self.h, len(lanes), sub.ctypes.data, 32, None, None, tab.ctypes.data, 1, out.ctypes.data)
            else:
                rc = self.lib.act_node_nullifier_check_and_insert_batch(self.h, len(lanes), sub.ctypes.data, 32, None, out.ctypes.data)
            answer[lanes] = out
            undetermined = out == 2                         # ACT_NULLIFIER_UNDETERMINED
            if rc == 0:
                return answer.tobytes()
            if rc != 1 or not undetermined.any() or self.capacity_per_device >= 1 << 30:
                self._ck(rc)
            self.reserve(min(1 << 30, 2 * self.capacity_per_device))
            lanes = lanes[undetermined]

    def contains(self, nullifiers: bytes, stride: int = 32) -> bytes:
        n = (len(nullifiers) + stride - 32) // stride if nullifiers else 0
        out = np.zeros(n, np.uint8); p0, k0 = _in(nullifiers)
        self._ck(self.lib.act_node_nullifier_contains_batch(self.h, n, p0, stride, out.ctypes.data))
        return out.tobytes()

    def export_step(self, cursor: int, max_keys: int, out: np.ndarray = None):
        out = _export_buffer(out, max_keys); cur = C.c_uint64(cursor); got = C.c_size_t(0)
        self._ck(self.lib.act_node_nullifier_set_export(self.h, C.byref(cur), max_keys, out.ctypes.data, C.byref(got)))
        return cur.value, out[:32 * got.value].tobytes()

    def export(self, max_keys: int = 1 << 20) -> bytes:
        return _export_loop(self.export_step, max_keys)

    def epoch_len(self, epoch: int) -> int:
        c = C.c_uint64(0)
        self._ck(self.lib.act_node_nullifier_set_epoch_len(self.h, epoch, C.byref(c)))
        return c.value

    def retire_epoch(self, epoch: int) -> int:
        """device after device; if one fails the others have retired and a repeat of the call finishes the job"""
        c = C.c_uint64(0)
        self._ck(self.lib.act_node_nullifier_set_retire_epoch(self.h, epoch, C.byref(c)))
        return c.value

    def retired_epochs(self) -> list:
        """the epochs every device has retired"""
        return _retired_list(lambda p, m, n: self._ck(self.lib.act_node_nullifier_set_retired_epochs(self.h, p, m, n)))

    def export_epochs_step(self, cursor: int, max_keys: int):
        out = np.empty(32 * max_keys, np.uint8); ep = np.empty(max_keys, np.uint32); cur = C.c_uint64(cursor); got = C.c_size_t(0)
        self._ck(self.lib.act_node_nullifier_set_export_epochs(self.h, C.byref(cur), max_keys, out.ctypes.data, ep.ctypes.data, C.byref(got)))
        return cur.value, out[:32 * got.value].tobytes(), ep[:got.value].copy()

    def export_epochs(self, max_keys: int = 1 << 20):
        return _export_epochs_loop(self.export_epochs_step, max_keys)

    def save(self, path: str) -> int:
        from . import nullifier_snapshot
        keys, epochs = self.export_epochs()
        return nullifier_snapshot.write_epochs(path, keys, epochs, self.retired_epochs())

    @classmethod
    def restore(cls, path: str, capacity_per_device: int = None, devices=(0,), salt: bytes = None) -> "NodeNullifierSet":
        """a new node set holding the snapshot's keys, epochs and retired list; every device is reserved for its expected share
        (restore_capacity)"""
        from . import nullifier_snapshot
        keys, epochs, retired = nullifier_snapshot.read_epochs(path)
        s = cls(max(capacity_per_device or 0, 1), devices=devices, salt=salt)
        nullifier_snapshot.restore_epochs_into(s, keys, epochs, retired)
        return s


EXPORT_DONE = 2**64 - 1      # ACT_NULLIFIER_EXPORT_DONE


def _export_buffer(out, max_keys: int) -> np.ndarray:
    if out is None:
        return np.empty(32 * max_keys, np.uint8)
    if out.dtype != np.uint8 or not out.flags.c_contiguous or out.size < 32 * max_keys:
        raise ValueError(f"export buffer: need a contiguous uint8 array of at least {32 * max_keys} bytes")
    return out


def _export_loop(step, max_keys: int) -> bytes:
    cur, parts, buf = 0, [], np.empty(32 * max_keys, np.uint8)      # one staging buffer for the whole loop
    while cur != EXPORT_DONE:
        cur, b = step(cur, max_keys, buf)
        parts.append(b)
    return b"".join(parts)


EPOCH_MAX = 0xFFFFFF         # ACT_NULLIFIER_EPOCH_MAX


def _epoch_table(epochs, want_len: int = None) -> np.ndarray:
    tab = np.ascontiguousarray(list(epochs), dtype=np.uint32)
    if not 1 <= len(tab) <= 255 or (want_len is not None and len(tab) != want_len):
        raise ValueError(f"epochs: {len(tab)} entries" + (f", expected {want_len}" if want_len is not None else ", expected 1 .. 255"))
    return tab


def _retired_list(call) -> list:
    n = C.c_size_t(0)
    call(None, 0, C.byref(n))
    while True:
        buf = np.zeros(max(1, n.value), np.uint32); room = len(buf)
        call(buf.ctypes.data, room, C.byref(n))
        if n.value <= room:
            return [int(e) for e in buf[:n.value]]


def _export_epochs_loop(step, max_keys: int):
    cur, keys, eps = 0, [], []
    while cur != EXPORT_DONE:
        cur, b, e = step(cur, max_keys)
        keys.append(b); eps.append(e)
    return b"".join(keys), (np.concatenate(eps) if eps else np.zeros(0, np.uint32))
