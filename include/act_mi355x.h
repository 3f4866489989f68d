/* act_mi355x.h — C ABI of libact_mi355x.so: the MI355X (gfx950) batch engine for the sigma-protocol
 * hot path of anonymous-credit-tokens v0.2.1.
 *
 * The reference crate has no FFI of its own; the drop-in boundary is its public Rust API
 * (/root/reference/src/lib.rs).  Each *_batch entry point below is what a `mod mi355x` inside the
 * crate binds for the corresponding method (INTEGRATION.md shows the Rust side), lane i of a batch
 * being one call of the method:
 *
 *   act_params_new                      <-> Params::new                  src/lib.rs:291-315
 *   act_request_batch                   <-> PreIssuance::request         src/lib.rs:463-487
 *   act_issue_batch                     <-> PrivateKey::issue            src/lib.rs:621-663
 *   act_prove_spend_batch               <-> CreditToken::prove_spend     src/lib.rs:972-1152
 *   act_refund_batch                    <-> PrivateKey::refund           src/lib.rs:781-869
 *   act_verify_spend_batch              <-> PrivateKey::refund up to the challenge check (:787-844)
 *   act_issuance_to_credit_token_batch  <-> PreIssuance::to_credit_token src/lib.rs:528-562
 *   act_refund_to_credit_token_batch    <-> PreRefund::to_credit_token   src/lib.rs:1217-1253
 *
 * Records are the crate's structs as consecutive 32-byte fields in CBOR key order
 * (src/cbor.rs:105-110, 163-169, 250-268, 422-427, 477-480, 546-549, 596-602, 656-660) with the CBOR
 * framing stripped; scalars little-endian (Scalar::as_bytes), points compressed Ristretto:
 *   PrivateKey        x | w                                                              64 B
 *   PreIssuance       r | k                                                              64 B
 *   IssuanceRequest   K | gamma | k_bar | r_bar                                         128 B
 *   IssuanceResponse  A | e | gamma | z | c                                             160 B
 *   CreditToken       a | e | k | r | c                                                 160 B
 *   SpendProof        k | s | A' | B_bar | Com[L] | gamma | e_bar | r2_bar | r3_bar | c_bar | r_bar |
 *                     w00 | w01 | gamma0[L] | z[L][2] | k_bar | s_bar                 32*(14+4L) B
 *   PreRefund         r | k | m                                                          96 B
 *   Refund            A* | e | gamma | z                                               128 B
 *
 * RNG: where the crate takes `impl CryptoRngCore`, the ABI takes the bytes that generator would
 * have produced; every Scalar::random is one 64-byte draw reduced mod l (draw order per function:
 * src/lib.rs:468-469, 643/649, 846/852, 978-1058).  issue/refund draw only for accepted lanes
 * (src/lib.rs:638-643, 842-846): ACT_RNG_PER_LANE gives lane i the slice rng[128*i..], and
 * ACT_RNG_SEQUENTIAL hands consecutive 128-byte slices to the accepted lanes in lane order — the
 * byte-for-byte equivalent of a sequential loop sharing one generator.
 *
 * Errors: the function result reports infrastructure failures only.  Per-lane results are
 * status[i] = 0 for Ok, else 1 + the discriminant of the crate's `Error` (src/lib.rs:102-112);
 * 255 = a point field that is not a canonical Ristretto encoding (the crate rejects those while
 * decoding, src/cbor.rs:62-77, before any of these methods can run).  The output record of a
 * failed lane is all zero.  Scalar fields are reduced mod l on input (src/cbor.rs:85).
 *
 * Memory: every bulk pointer of one call is either host memory (ACT_MEM_HOST) or memory of the
 * context's GPU (ACT_MEM_DEVICE); `sk` is always host memory.  The engine works on its own HIP streams:
 * device-memory inputs must be complete (the producing stream synchronised) before a call, and outputs are
 * complete when the call returns.  A context is bound to one GPU and owns its streams and workspace; every batch entry
 * point takes the context's lock, so a context shared between host threads serves them one at a time; different contexts
 * (e.g. one per GPU) run concurrently (batches shard across GPUs with no collective).  Contexts of one process on the
 * same GPU with the same Params share one set of fixed-base tables.
 * Host memory may be pageable or pinned.  Spend-proof RECORDS (public inputs) that lie in pinned memory (hipHostMalloc /
 * hipHostRegister under the context's device) are read by the kernels in place over the link -- no staging copy in front of the
 * first kernel; a caller must therefore not write to them while the call runs.  Everything else (wire bytes included), and pageable
 * memory, is staged through the context's own buffers, which are wiped when the call ends.
 * There is no CPU fallback: without a HIP device every entry point fails.
 */
#ifndef ACT_MI355X_H
#define ACT_MI355X_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ======== SURVEY.md 8 rows a7 + b: result codes, memory kinds, rng conventions, per-lane statuses (records: the comment above) ==== */
#define ACT_OK 0
#define ACT_ERR_ARG 1        /* null pointer, bad L, bad mode */
#define ACT_ERR_HIP 2        /* a HIP runtime call failed; act_last_error() has the text */
#define ACT_ERR_PARAMS 3     /* h1/h2/h3 or the public key is not a canonical Ristretto encoding */
#define ACT_ERR_NO_DEVICE 4
#define ACT_ERR_RNG 5        /* ACT_RNG_CALLBACK: the caller's draw() reported a failure; nothing was signed with the bytes */

#define ACT_MEM_HOST 0
#define ACT_MEM_DEVICE 1

#define ACT_RNG_PER_LANE 0
#define ACT_RNG_SEQUENTIAL 1
/* The crate's `impl CryptoRngCore` itself, for the calls that say they take it (the wire-level and redeem entry points below): `rng`
 * points to an act_rng_source instead of bytes.  The library calls draw(rng_ctx, dst, 128 * k) ONCE per call, from the calling
 * thread, after every verdict is known, k = the number of lanes that will be signed -- the generator is advanced by exactly what a
 * sequential loop over refund() would have drawn (src/lib.rs:842-852: e, alpha only after the checks), and the slices go to the
 * signed lanes in lane order like ACT_RNG_SEQUENTIAL.  The drawn bytes are wiped before the call returns.
 * draw returns 0 when it has written all `len` bytes and non-zero when it could not (generator exhausted, an exception in a
 * language binding's trampoline ...): the call then fails with ACT_ERR_RNG and signs NOTHING -- a signature made with e = alpha = 0
 * would give the issuer's key away (z = gamma * x).  Lanes that were to be signed are reported as after a failed signature step
 * (redeem: ACT_STATUS_RECORDED_UNSIGNED, their nullifiers are recorded; the other calls: no output records). */
#define ACT_RNG_CALLBACK 2
typedef int (*act_rng_draw_fn)(void *rng_ctx, uint8_t *dst, size_t len);
typedef struct act_rng_source { act_rng_draw_fn draw; void *rng_ctx; } act_rng_source;

#define ACT_TRANSCRIPT_HOST 0    /* BLAKE3 of every transcript on host threads (src/transcript.rs stays on the host) */
#define ACT_TRANSCRIPT_DEVICE 1  /* the same bytes hashed by the device BLAKE3 kernel; no D2H/H2D inside a batch */

/* per-lane status = 1 + discriminant of reference `Error`, src/lib.rs:102-112 */
#define ACT_STATUS_OK 0
#define ACT_STATUS_INVALID_ISSUANCE_REQUEST_PROOF 1
#define ACT_STATUS_INVALID_ISSUANCE_RESPONSE_PROOF 2
#define ACT_STATUS_DOUBLE_SPEND 3
#define ACT_STATUS_INVALID_REFUND_PROOF 4
#define ACT_STATUS_INVALID_REFUND_RESPONSE_PROOF 5
#define ACT_STATUS_IDENTITY_POINT 6
#define ACT_STATUS_INVALID_CLIENT_SPEND_PROOF 7
#define ACT_STATUS_AMOUNT_TOO_BIG 8
#define ACT_STATUS_SCALAR_OUT_OF_RANGE 9
#define ACT_STATUS_UNDECODABLE 255
/* act_redeem_batch / act_node_redeem_batch only, and only together with a non-zero function result (see there) */
#define ACT_STATUS_NULLIFIER_UNDETERMINED 252   /* verified; the nullifier step could not answer: NOT recorded, NOT signed -- resubmit */
#define ACT_STATUS_RECORDED_UNSIGNED 251        /* verified, nullifier recorded, the signature step failed: the refund is owed -- sign, never redeem again */

/* ======== row a6: Params::new / Params::random ================================================================================== */
typedef struct act_ctx act_ctx;

/* Params::new (src/lib.rs:291-315): out_h = enc(h1) | enc(h2) | enc(h3).  Runs on `device`. */
int act_params_new(int device, const char *organization, const char *service, const char *deployment_id,
                   const char *version, uint8_t out_h[96]);
/* Params::random (src/lib.rs:259-265): rng = 192 bytes (three RistrettoPoint::random draws). */
int act_params_random(int device, const uint8_t rng[192], uint8_t out_h[96]);

/* ======== row b: the context (one GPU), row a5: where the transcript is hashed, and the context's knobs ========================= */
/* A context = Params (h1,h2,h3 with their device-resident fixed-base tables, cf. the three
 * RistrettoBasepointTables of src/lib.rs:222-229) + the range-proof width L (src/lib.rs:116; 128 is the
 * crate's value, 1..128 accepted) + one GPU.  max_batch bounds the records per internal launch and thereby the workspace.
 * What a context costs in HBM at L = 128:
 *     workspace      about 200 KB per record of max_batch per pipeline slot, two slots:  max_batch 65536 -> 27 GB, 16384 -> 6.8 GB,
 *                    4096 -> 1.7 GB; staging buffers of host-memory callers grow on demand on top (up to ~7 GB for a 65536-lane
 *                    prover chunk)
 *     tables         0.5 GB (16-bit windows for g, h1, h2, h3 + the matrix-core images), shared by all contexts of the process on
 *                    that GPU with the same Params
 * and nothing else, whatever the device has free: wider fixed-base windows are asked for (act_ctx_set_fixed_base_bits below).
 * 0 = default = 65536, from which size on the throughput of every entry point is flat; 16384 costs about 5 % of the verify rate and
 * two thirds of the issue/request rate.  Batches of any length are accepted and processed in such chunks.  max_batch > 2^22 is
 * refused (ACT_ERR_ARG).  On failure *out still receives a context whose only use is act_last_error() and act_ctx_destroy(). */
int act_ctx_create(const uint8_t h[96], int L, int device, size_t max_batch, act_ctx **out);
void act_ctx_destroy(act_ctx *ctx);
int act_ctx_set_transcript_mode(act_ctx *ctx, int mode);    /* default ACT_TRANSCRIPT_HOST */
/* Host BLAKE3 workers of the host-transcript mode.  All contexts of a process share ONE pool of act_host_usable_cpus() workers,
 * started on the first hashing call (never, if only device transcripts are used).  A call takes its fair share of it -- pool size /
 * (contexts hashing at that moment) -- so the 8 contexts of a node handle get an eighth each when they all hash and the whole pool
 * when they hash alone; nthreads > 0 caps the share of this context, 0 = no cap.  ACT_NUMA=1 pins worker k to the k-th CPU of the
 * process's affinity mask. */
int act_ctx_set_host_threads(act_ctx *ctx, int nthreads);
/* Telemetry of the host-transcript mode on this context since the last reset: seconds its calling thread spent waiting for
 * transcript pieces to arrive from the device, seconds it spent hashing them (with its share of the pool), bytes hashed.  hash_s over
 * the wall time of the calls = how close the host side is to being the bottleneck (bench.py reports it per rank at N > 1). */
int act_ctx_host_hash_stats(act_ctx *ctx, double *wait_s, double *hash_s, uint64_t *bytes, int reset);
int act_host_usable_cpus(void);                             /* CPUs the process may use (affinity mask, cgroup quota) = pool size */
/* The pool's hashing entry point (what the host-transcript mode calls; pure host code, usable and tested without a GPU):
 * xof[16*i ..] = first 64 XOF bytes of BLAKE3(msgs + i*stride, len), i < n; max_threads as nthreads above. */
void act_host_hash_many(const uint8_t *msgs, size_t stride, uint32_t len, size_t n, int max_threads, uint32_t *xof);
/* fn(ctx, i0, i1) over [0, n) in items of `grain` indices on the same workers, in any order, the caller among them; returns when
 * all have run.  (What act_node_nullifier_check_and_insert_batch routes keys to their owning GPU with; max_threads as above.) */
typedef void (*act_host_range_fn)(void *ctx, size_t i0, size_t i1);
void act_host_parallel_for(size_t n, size_t grain, int max_threads, act_host_range_fn fn, void *ctx);
/* diagnostics: hashing calls served, worker threads ever created by this process (constant after the first call), pool size */
void act_host_pool_stats(uint64_t *jobs, uint64_t *threads_created, int *pool_size);
/* A context pipelines two chunks on two HIP streams.  The HIP runtime maps a process's streams onto GPU_MAX_HW_QUEUES hardware
 * queues per device and priority (default 4): in a process with many streams both may land on one queue and the chunks then run
 * one after the other (measured: 415 k instead of 466 k verifies/s from host memory).  act_ctx_create measures this (two idle
 * wavefronts, 0.3 ms) and, if they share a queue, moves the second stream to another priority class, which has its own queues.
 * 1 = the streams run side by side, 0 = they still share a queue (set GPU_MAX_HW_QUEUES=8 in the embedding process before HIP
 * initialises: INTEGRATION.md), -1 = not measured.  The library never edits the process environment and, apart from the diagnostics
 * ACT_TRACE / ACT_TIMELINE_FILE and the worker pinning ACT_NUMA, never reads it. */
int act_ctx_streams_overlap(const act_ctx *ctx);
/* chunks in flight per call: 2 (default; chunk i+1's kernels overlap chunk i's low-occupancy head / tail kernels and, in
 * host-transcript mode, its host hashing) or 1 (strictly one after the other: profiling runs whose per-kernel durations
 * must not overlap) */
int act_ctx_set_pipeline_depth(act_ctx *ctx, int depth);
/* The crate's entry points take ONE proof per call (src/lib.rs:781-786).  Verify / refund calls of at most `n` proofs (default
 * 8192, and 16384 while the context hashes its transcripts on the device; 0 = never) run the small-batch schedule: one chunk, the per-proof kernels next to the range kernel on streams of their own (five in all) instead of
 * in front of and behind it -- the same lane code and bytes, 2-3 x shorter for one proof and ~1.5 x the rate at 4 096 proofs; larger
 * calls pipeline 65 536-proof chunks as before (one lane per proof is the faster form once a launch fills the chip).
 * Threads with a context each may make such calls at the same time; two of them run on a device at once, the others wait their
 * turn inside the call (more active streams than that and the driver time-slices the process's queues: INTEGRATION.md). */
int act_ctx_set_small_batch_max(act_ctx *ctx, size_t n);
/* Tiny calls -- at most 64 lanes, the crate's own one-item call shape (src/lib.rs:463, 528, 621, 781, 1217).  Their answer time is a
 * dependent chain plus fixed cost, so act_request_batch, act_issue_batch (ACT_RNG_PER_LANE, or one lane), the signing half of every
 * issue / refund call and the two to_credit_token calls run such a call as ONE kernel: the independent pieces of the method on
 * separate workgroups (a signature's two variable-base products cut into quarters), the block that arrives last assembling the
 * transcript, hashing it -- these transcripts are a single BLAKE3 chunk; the routine is the one ACT_TRANSCRIPT_DEVICE runs, so the
 * bytes are those of either transcript mode -- and finishing the record; inputs cross PCIe in one copy from a pinned buffer, which
 * the kernel zeroes itself.  One item, MI355X: request 0.27 ms (was 0.58), issue 1.15 (2.7), PreIssuance::to_credit_token 1.1 (2.3),
 * PreRefund::to_credit_token 1.5 (3.0), refund 2.0 (3.7), prove_spend 2.0 (3.2): profiles/r05_single_item_latency.txt.
 * act_ctx_set_tiny_calls(ctx, 0) keeps the multi-launch paths, whose transcripts follow
 * the context's transcript mode -- a deployment that wants every hash on the host, whatever the call size (same bytes either way;
 * tests/test_gpu_tiny.py compares). */
int act_ctx_set_tiny_calls(act_ctx *ctx, int on);           /* default 1 */
/* Secrets and memory addresses.  The reference is constant-time in its table accesses (`subtle`, src/lib.rs:98, 1025-1118;
 * dalek's table scans).  libact_mi355x.so (the default build, for which this returns 1) matches that for EVERY secret: the issuer's
 * private key and signing nonces, and the client's tokens, blinding factors and prover rng, never select a memory address --
 * variable-base products run a register-only chain that executes every digit addition, and fixed-base products pick their table
 * entries on the matrix cores: selected = Table x onehot(digits), one v_mfma_i32_32x32x32_i8 per 32 bytes x 32 lanes x 32 entries,
 * so a window holds 64 entries (37 per product) with no entry ever addressed by a digit (csrc/msm.h fixed_base_acc_mf).
 * libact_mi355x_fast.so (make fast; returns 0) differs only for the CLIENT's secrets (act_prove_spend_*, act_request_batch): they go
 * through scalar-addressed 16- / 24-bit tables and Pippenger buckets -- the instruction stream still does not depend on them, the
 * memory-access pattern does.  Same bytes either way.  Measured on one MI355X (docs/history/profiles/r04_*_other_configs_1gpu*.json): default
 * vs fast build prove_spend 0.48 x (1.16 M/s vs 2.40 M/s; round 3's masked scan: 0.26 x), request 0.55 x, a whole lifecycle
 * 0.85 x; every issuer-side call -- verify, refund, issue, redeem -- is the same code in both.  A client that owns its GPU may load
 * the fast build; an issuer gains nothing from it. */
int act_build_has_ct_secret_tables(void);
/* Window width in bits of the fixed-base table of base 0..3 = g, h1, h2, h3 in this context (a product costs ceil(253 / bits) table
 * additions).  16 after act_ctx_create (128 MiB per base), always.  act_ctx_set_fixed_base_bits(ctx, base, bits), bits in 4..24,
 * builds the table of that width now (or shares it with the process's other contexts on the device) and releases the old one; the
 * range kernel's bases are h1 (1) and h3 (3): 24 bits on both is +47 GB (23.6 GB each, built in about 2 s) for +3 % verifies/s --
 * worth it on a GPU that serves nothing else, and only the caller knows that.  Refused (ACT_ERR_HIP, width unchanged) when the
 * device has not the table's size + 16 GB free.  Not while another thread has a call on the context in flight with results that
 * matter for timing: it takes the context's lock like a batch call. */
int act_ctx_fixed_base_bits(const act_ctx *ctx, int base);
int act_ctx_set_fixed_base_bits(act_ctx *ctx, int base, int bits);
/* Text of the CALLING THREAD's last failure on this handle (of the handle's most recent failure if this thread has had none): a
 * handle is shared between threads, and a caller whose small call was merged into another thread's launch gets that launch's text.
 * Every *_last_error function copies the text into a buffer of the calling thread, valid until that thread asks again. */
const char *act_last_error(const act_ctx *ctx);
size_t act_spend_proof_bytes(const act_ctx *ctx);           /* 32*(14+4L) */
size_t act_prove_rng_bytes(const act_ctx *ctx);             /* 64*(4L+12) */
size_t act_spend_transcript_bytes(const act_ctx *ctx);      /* pre-image of the "spend" challenge */

/* ======== rows a1 - a4 and f1: request, issue, prove_spend, refund (and its verification half), the two client verifiers -- lane i = one call of the method ==== */
/* PrivateKey::random (src/lib.rs:188-194): rng 64 B -> x | w.  PreIssuance::random (:432-437): rng 128 B -> r | k. */
int act_private_key_random(act_ctx *ctx, const uint8_t rng[64], uint8_t out_sk[64]);
int act_pre_issuance_random_batch(act_ctx *ctx, size_t n, int mem, const uint8_t *rng, uint8_t *out_pre);

/* PreIssuance::request: pre n*64, rng n*128 -> req n*128 */
int act_request_batch(act_ctx *ctx, size_t n, int mem, const uint8_t *pre, const uint8_t *rng, uint8_t *out_req);
/* PrivateKey::issue: req n*128, c n*32, rng (n or #accepted)*128 -> resp n*160, status n.  The rng argument is BYTES: this call
 * never touches a generator, so it cannot advance one for a rejected item.  ACT_RNG_SEQUENTIAL with n == 1: the buffer must hold its
 * 128 bytes WHATEVER the verdict -- a one-lane call computes the signature beside the check and reads the slice first (the bytes of
 * a rejected lane are wiped with the call and go nowhere).  A caller that draws from a generator and must leave it where the crate
 * leaves it (src/lib.rs:638-643: e, alpha only after the check) uses the two halves below, as the Rust binding's `issue` does; the
 * binding offers the one-call form only as a free function over explicit bytes (rust/src/mi355x.rs `predrawn::issue`). */
int act_issue_batch(act_ctx *ctx, size_t n, int mem, const uint8_t sk[64], const uint8_t *req, const uint8_t *c,
                    const uint8_t *rng, int rng_mode, uint8_t *out_resp, uint8_t *status);
/* PreIssuance::to_credit_token: pre n*64, w 32 (host), req n*128, resp n*160 -> token n*160, status n */
int act_issuance_to_credit_token_batch(act_ctx *ctx, size_t n, int mem, const uint8_t *pre, const uint8_t w[32],
                                       const uint8_t *req, const uint8_t *resp, uint8_t *out_token, uint8_t *status);
/* CreditToken::prove_spend: token n*160, s n*32, rng n*act_prove_rng_bytes -> proof n*act_spend_proof_bytes, prerefund n*96 */
int act_prove_spend_batch(act_ctx *ctx, size_t n, int mem, const uint8_t *token, const uint8_t *s, const uint8_t *rng,
                          uint8_t *out_proof, uint8_t *out_prerefund, uint8_t *status);
/* The same with the generator SEEDED instead of spelled out: lane i draws from the BLAKE3 XOF of seed | u64_le(first_lane + i),
 * read sequentially by every Scalar::random -- on the crate's side `prove_spend(params, s, XofRng(seed, lane))` with an RngCore over
 * blake3::Hasher::new().update(seed).update(&lane.to_le_bytes()).finalize_xof().  The 64 (4L + 12) = 33 536 rng bytes per proof are
 * expanded in HBM and never cross PCIe (streaming 2^16 lifecycles per call from host memory: 200 k -> see DESIGN.md section 6).  The
 * seed is a secret of the prover like the rng bytes are; one seed must never serve the same lane number twice. */
int act_prove_spend_seeded_batch(act_ctx *ctx, size_t n, int mem, const uint8_t *token, const uint8_t *s, const uint8_t seed[32],
                                 uint64_t first_lane, uint8_t *out_proof, uint8_t *out_prerefund, uint8_t *status);
/* spend-proof verification only (src/lib.rs:787-844): proof -> status n; out_kprime (nullable) n*32 = enc(K') */
int act_verify_spend_batch(act_ctx *ctx, size_t n, int mem, const uint8_t sk[64], const uint8_t *proof,
                           uint8_t *status, uint8_t *out_kprime);
/* PrivateKey::refund: proof, rng (n or #accepted)*128 -> refund n*128, status n.  As for act_issue_batch: a one-lane ACT_RNG_SEQUENTIAL
 * call needs its 128 bytes present whatever the verdict (the signature is computed beside the verification); generator-exact callers
 * use act_verify_spend_batch + act_refund_sign_batch (src/lib.rs:842-846), or the wire-level calls with ACT_RNG_CALLBACK. */
int act_refund_batch(act_ctx *ctx, size_t n, int mem, const uint8_t sk[64], const uint8_t *proof, const uint8_t *rng,
                     int rng_mode, uint8_t *out_refund, uint8_t *status);
/* PreRefund::to_credit_token: prerefund n*96, proof, refund n*128, w 32 (host) -> token n*160, status n */
int act_refund_to_credit_token_batch(act_ctx *ctx, size_t n, int mem, const uint8_t *prerefund, const uint8_t *proof,
                                     const uint8_t *refund, const uint8_t w[32], uint8_t *out_token, uint8_t *status);

/* The two halves of issue / refund as separate calls, for callers that must see every verdict before any rng is assigned
 * (the node dispatcher below; a caller with its own admission step between check and signature):
 *   act_issue_check_batch   the PoK check alone (src/lib.rs:629-640): req n*128 -> status n
 *   act_issue_sign_batch    the BBS signature (:643-660) for lanes with status_in == 0: X_A = g + c h1 + K from the request
 *   act_refund_sign_batch   the BBS signature (:846-868) for lanes with status_in == 0: X_A = g + K', kprime n*32 as returned
 *                           by act_verify_spend_batch
 * rng / rng_mode as in act_issue_batch; check + sign with the same rng gives the bytes of the one-call form. */
int act_issue_check_batch(act_ctx *ctx, size_t n, int mem, const uint8_t *req, uint8_t *status);
int act_issue_sign_batch(act_ctx *ctx, size_t n, int mem, const uint8_t sk[64], const uint8_t *req, const uint8_t *c,
                         const uint8_t *status_in, const uint8_t *rng, int rng_mode, uint8_t *out_resp, uint8_t *status);
int act_refund_sign_batch(act_ctx *ctx, size_t n, int mem, const uint8_t sk[64], const uint8_t *kprime, const uint8_t *status_in,
                          const uint8_t *rng, int rng_mode, uint8_t *out_refund, uint8_t *status);

/* ======== row e: the GPUs of one node behind one handle (no collective) ========================================================= */
/* Node-level dispatch: the GPUs of one node behind one handle.  act_node_create builds one context per
 * entry of devices[] (the same device may be listed more than once: each entry is its own context, stream set and
 * workspace).  Every act_node_*_batch call cuts its batch into contiguous pieces (one per context, shard k = lanes
 * [n*k/N, n*(k+1)/N), for batches below 16384 lanes per GPU; see "Load balance" below for larger ones), runs every piece on a
 * context from that context's own host thread through the single-GPU entry point of the same
 * name, and writes outputs into the matching slices of the caller's arrays: no collective, no peer traffic.  All bulk
 * pointers are host memory.  ACT_RNG_SEQUENTIAL stays exact across shards -- the bytes of one sequential loop over one
 * generator (src/lib.rs:638-643, 842-846 draw only for accepted lanes): all shards are checked first, the host counts
 * the accepted lanes in front of every shard, then all shards sign from their offsets into the stream; refund carries
 * only enc(K') between the two phases.  ACT_RNG_PER_LANE needs no such barrier and is one pass.  A node handle (like a
 * context) may be shared between host threads: every *_batch call takes the handle's lock, so concurrent callers are
 * served one after the other.  act_node_create builds the contexts concurrently (one thread per entry); entries that name
 * the same device share that device's fixed-base tables. */
typedef struct act_node act_node;
int act_node_create(const uint8_t h[96], int L, const int *devices, int n_devices, size_t max_batch, act_node **out);
void act_node_destroy(act_node *node);
int act_node_device_count(const act_node *node);
act_ctx *act_node_ctx(act_node *node, int k);                  /* context k, e.g. for act_ctx_set_* / act_prof_* */
const char *act_node_last_error(const act_node *node);
int act_node_set_transcript_mode(act_node *node, int mode);
int act_node_set_host_threads(act_node *node, int per_gpu);    /* host BLAKE3 workers of every context */
int act_node_set_wire_reader(act_node *node, int reader);      /* act_ctx_set_wire_reader on every context */
int act_node_set_fixed_base_bits(act_node *node, int base, int bits);   /* act_ctx_set_fixed_base_bits on every context */
/* Load balance.  The GPUs of a node are not equally fast (clocks differ by several percent between devices and move with
 * temperature) and a call ends when its slowest GPU does, so the cut is not n/N: (1) every throughput-sized call -- at least
 * 16384 lanes per GPU -- measures what each context did with its piece and the next call cuts in proportion (weights: relative
 * speed, mean 1); (2) the last part of such a batch is not assigned in advance but handed out in small pieces (>= 4096 lanes) to
 * whichever GPU asks next, its size following the finish-time spread the previous calls showed: a sixteenth of the batch while
 * nothing is known, nothing once the GPUs finish together (a tail costs a few small calls).  Neither changes a byte of the output:
 * a lane's result depends on its inputs and its rng slice, never on the GPU that computed it.
 *   act_node_set_balance     weighted = 0 turns (1) off (equal cut); tail_64ths = -1 adaptive (default), 0 = no tail, k = k/64 of the batch
 *   act_node_device_stats    context k: its weight, and lanes / seconds / calls it was given in the most recent cut call
 *   act_node_balance_state   finish-time spread of the heads (running average, relative to their mean; < 0 = not measured yet) and the
 *                            fraction of the last call that went through the tail */
int act_node_set_balance(act_node *node, int weighted, int tail_64ths);
int act_node_device_stats(act_node *node, int k, double *weight, uint64_t *last_lanes, double *last_seconds, uint64_t *last_calls);
int act_node_balance_state(act_node *node, double *spread, double *tail_fraction);
int act_node_request_batch(act_node *node, size_t n, const uint8_t *pre, const uint8_t *rng, uint8_t *out_req);
int act_node_issue_batch(act_node *node, size_t n, const uint8_t sk[64], const uint8_t *req, const uint8_t *c, const uint8_t *rng,
                         int rng_mode, uint8_t *out_resp, uint8_t *status);
int act_node_issuance_to_credit_token_batch(act_node *node, size_t n, const uint8_t *pre, const uint8_t w[32], const uint8_t *req,
                                            const uint8_t *resp, uint8_t *out_token, uint8_t *status);
/* the halves on their own (cf. act_issue_check_batch ...): a caller that draws its rng between check and signature -- the
 * Rust binding advances the caller's generator by exactly 128 bytes per accepted lane, as the sequential loop would */
int act_node_issue_check_batch(act_node *node, size_t n, const uint8_t *req, uint8_t *status);
int act_node_issue_sign_batch(act_node *node, size_t n, const uint8_t sk[64], const uint8_t *req, const uint8_t *c,
                              const uint8_t *status_in, const uint8_t *rng, int rng_mode, uint8_t *out_resp, uint8_t *status);
int act_node_refund_sign_batch(act_node *node, size_t n, const uint8_t sk[64], const uint8_t *kprime, const uint8_t *status_in,
                               const uint8_t *rng, int rng_mode, uint8_t *out_refund, uint8_t *status);
int act_node_prove_spend_batch(act_node *node, size_t n, const uint8_t *token, const uint8_t *s, const uint8_t *rng,
                               uint8_t *out_proof, uint8_t *out_prerefund, uint8_t *status);
int act_node_prove_spend_seeded_batch(act_node *node, size_t n, const uint8_t *token, const uint8_t *s, const uint8_t seed[32],
                                      uint64_t first_lane, uint8_t *out_proof, uint8_t *out_prerefund, uint8_t *status);
int act_node_verify_spend_batch(act_node *node, size_t n, const uint8_t sk[64], const uint8_t *proof, uint8_t *status,
                                uint8_t *out_kprime);
int act_node_refund_batch(act_node *node, size_t n, const uint8_t sk[64], const uint8_t *proof, const uint8_t *rng, int rng_mode,
                          uint8_t *out_refund, uint8_t *status);
int act_node_refund_to_credit_token_batch(act_node *node, size_t n, const uint8_t *prerefund, const uint8_t *proof,
                                          const uint8_t *refund, const uint8_t w[32], uint8_t *out_token, uint8_t *status);

/* ======== row f3: wire bytes -- the batch CBOR codec, wire -> verdict, wire -> wire ============================================= */
/* Batch CBOR codec (src/cbor.rs: to_cbor / from_cbor of the nine wire and state types; deterministic RFC 8949
 * encoding, int-keyed maps, 32-byte byte strings).  `type` selects the struct; records are the raw layouts above.
 * Encoding writes n canonical messages of act_cbor_size(ctx, type) bytes each, back to back.  Decoding takes n
 * messages delimited by offsets[0..n] (byte offsets into `cbor`, host memory; NULL = n canonical-size messages back to
 * back) and accepts whatever ciborium accepts (any well-formed CBOR map; unknown keys ignored; the last duplicate
 * wins; bytes after the first item ignored).  Scalars come out reduced mod l (decode_scalar, src/cbor.rs:80-91).
 * status[i]: 0 ok, 1 malformed CBOR (CborError::Ciborium), 2 CborError::InvalidStructure, 3 CborError::InvalidValue
 * (a point that is not a canonical Ristretto encoding, src/cbor.rs:59-78); the record of a failed message is zero.
 * The code is from_cbor's code, also for a message that is wrong in several ways: the whole item is parsed first (1), then the
 * first failure in WIRE order of the map's entries decides (src/cbor.rs:276-388: an invalid point in front of a mis-shaped
 * field is 3, behind it 2; array elements, those of an over-long array included, are decoded before the length is checked;
 * a value a later duplicate key overwrites still has to decode), and missing fields come last (:390-407).
 * Canonical messages are framed / unframed on the GPU (one lane per 32-byte field); others take a host reader, which hands the
 * points whose position matters to a validation kernel.
 * act_cbor_read_batch has the same contract -- all nine types, scalars reduced, points validated, the first failure in wire order,
 * a zero record for a failed message -- with EVERY message read by the general RFC 8949 reader on the GPU (one lane per message,
 * csrc/cbor_lanes.h): no canonical short cut and no host reader.  It is the reader the spend wire calls below run for messages that
 * are not the canonical encoding, exposed on its own; chunked and staged like the decode call. */
#define ACT_CBOR_ISSUANCE_REQUEST 1
#define ACT_CBOR_ISSUANCE_RESPONSE 2
#define ACT_CBOR_SPEND_PROOF 3
#define ACT_CBOR_REFUND 4
#define ACT_CBOR_PRIVATE_KEY 5
#define ACT_CBOR_PUBLIC_KEY 6
#define ACT_CBOR_PRE_ISSUANCE 7
#define ACT_CBOR_CREDIT_TOKEN 8
#define ACT_CBOR_PRE_REFUND 9
#define ACT_CBOR_REFUND_RETURN 10   /* the Refund map with one more entry, key 5 -> t (partial refunds, below); record A | e | gamma | z | t, 160 bytes */
size_t act_cbor_size(const act_ctx *ctx, int type);
size_t act_cbor_record_bytes(const act_ctx *ctx, int type);
int act_cbor_encode_batch(act_ctx *ctx, int type, size_t n, int mem, const uint8_t *records, uint8_t *out_cbor);
int act_cbor_decode_batch(act_ctx *ctx, int type, size_t n, int mem, const uint8_t *cbor, const uint64_t *offsets,
                          uint8_t *out_records, uint8_t *status);
int act_cbor_read_batch(act_ctx *ctx, int type, size_t n, int mem, const uint8_t *cbor, const uint64_t *offsets,
                        uint8_t *out_records, uint8_t *status);

/* Wire bytes in, verdict out: SpendProof::from_cbor (src/cbor.rs:236-408) + PrivateKey::refund up to the challenge check
 * (src/lib.rs:787-844) as ONE pass over n CBOR messages (delimited like act_cbor_decode_batch's: offsets[0..n] in host memory, or
 * NULL for canonical-size messages back to back).  Every chunk is unframed on the GPU in front of its verification kernels, and
 * each of a proof's 130 points is decoded once -- act_cbor_decode_batch followed by act_verify_spend_batch decodes them twice and
 * moves the records through the caller's memory in between.  status[i]: 0 / 6 / 7 as act_verify_spend_batch;
 * 255 = a point that is not a canonical Ristretto encoding (from_cbor's CborError::InvalidValue);
 * ACT_STATUS_CBOR_MALFORMED = not well-formed CBOR (CborError::Ciborium); ACT_STATUS_CBOR_STRUCTURE = CborError::InvalidStructure
 * (not a map, missing field, wrong shape or length).  The status is the one from_cbor followed by refund gives, also for a message
 * that is wrong in several ways (the first failure in wire order, as described at act_cbor_decode_batch).  A message that is not
 * the canonical encoding -- an indefinite-length map, another key order, an unknown key, a chunked byte string ... -- is read by the
 * general reader ON THE GPU, in its chunk's own stream between the unframing kernel and the verification kernels, and verified
 * once, in the pipeline, like every other message; the same holds for every wire-level spend call below (refund, redeem, the ring
 * and epoch forms) and for the admission screen.  out_kprime (nullable) as in act_verify_spend_batch.
 *
 * act_ctx_set_wire_reader chooses where such messages are read: ACT_WIRE_READER_DEVICE (the default) as described;
 * ACT_WIRE_READER_HOST keeps the earlier road -- flagged messages verified as all-zero records, then read on the calling thread
 * behind the pipeline and verified a second time -- as a fallback and as the baseline of comparisons.  The answers are the same.
 * The setting also governs act_issue_check_cbor_batch and act_issue_cbor_batch (below).
 * act_ctx_wire_stats: messages seen, canonical, read on the device, read by the host reader -- counted on the spend wire path, in
 * the admission screen and by the issuance wire calls (once per message and call) since the last reset.  The counters count READS, not distinct messages: an admission call counts every
 * message once in its screen (where the reduced form, k and s, is read) and every survivor of the screen once more in the
 * verification behind it, which reads the whole record. */
#define ACT_STATUS_CBOR_MALFORMED 254
#define ACT_STATUS_CBOR_STRUCTURE 253
#define ACT_WIRE_READER_HOST 0
#define ACT_WIRE_READER_DEVICE 1
int act_ctx_set_wire_reader(act_ctx *ctx, int where);
int act_ctx_wire_stats(act_ctx *ctx, uint64_t out[4], int reset);
int act_verify_spend_cbor_batch(act_ctx *ctx, size_t n, int mem, const uint8_t sk[64], const uint8_t *cbor, const uint64_t *offsets,
                                uint8_t *status, uint8_t *out_kprime);
int act_node_verify_spend_cbor_batch(act_node *node, size_t n, const uint8_t sk[64], const uint8_t *cbor, const uint64_t *offsets,
                                     uint8_t *status, uint8_t *out_kprime);
/* The same, also returning what the rest of a redemption needs: out_nullifier (nullable) n*32 = the `k` field of every message as it
 * stood on the wire (unreduced; the nullifier sets reduce mod l themselves), zero for a message that did not parse. */
int act_verify_spend_cbor_keys_batch(act_ctx *ctx, size_t n, int mem, const uint8_t sk[64], const uint8_t *cbor, const uint64_t *offsets,
                                     uint8_t *status, uint8_t *out_kprime, uint8_t *out_nullifier);
int act_node_verify_spend_cbor_keys_batch(act_node *node, size_t n, const uint8_t sk[64], const uint8_t *cbor, const uint64_t *offsets,
                                          uint8_t *status, uint8_t *out_kprime, uint8_t *out_nullifier);

/* Wire bytes in, wire bytes out: what a server does with the bytes a client sent (SpendProof::from_cbor, src/cbor.rs:276-408;
 * PrivateKey::refund, src/lib.rs:781-869; Refund::to_cbor, src/cbor.rs:421-433) without a SpendProof, a RistrettoPoint or a Refund
 * ever existing on the host.  Message i in, message i out: out_refund_cbor holds n slots of act_cbor_size(ctx, ACT_CBOR_REFUND)
 * bytes (141), the canonical Refund message of an accepted lane, all zero for any other lane.
 *   act_refund_sign_cbor_batch   act_refund_sign_batch + framing: the BBS signature for lanes with status_in == 0 from enc(K')
 *   act_refund_cbor_batch        act_verify_spend_cbor_batch, then the above; status as act_verify_spend_cbor_batch
 * rng / rng_mode: ACT_RNG_PER_LANE, ACT_RNG_SEQUENTIAL (both halves see every verdict before a slice is assigned, so SEQUENTIAL is the
 * sequential loop's byte stream) or ACT_RNG_CALLBACK.  The node forms cut the batch over the GPUs like every act_node_* call. */
int act_refund_sign_cbor_batch(act_ctx *ctx, size_t n, int mem, const uint8_t sk[64], const uint8_t *kprime, const uint8_t *status_in,
                               const uint8_t *rng, int rng_mode, uint8_t *out_refund_cbor, uint8_t *status);
int act_refund_cbor_batch(act_ctx *ctx, size_t n, int mem, const uint8_t sk[64], const uint8_t *cbor, const uint64_t *offsets,
                          const uint8_t *rng, int rng_mode, uint8_t *out_refund_cbor, uint8_t *status);
/* ... and the nullifier `k` of every message as it stood on the wire (n*32; zero for a message that did not parse), as
 * act_verify_spend_cbor_keys_batch returns it: for a caller that keeps the double-spend store itself and decides AFTER the refund was
 * computed whether to hand it out (what act_node_redeem_cbor_batch does with a few messages: refund in one call, then the store). */
int act_refund_cbor_keys_batch(act_ctx *ctx, size_t n, int mem, const uint8_t sk[64], const uint8_t *cbor, const uint64_t *offsets,
                               const uint8_t *rng, int rng_mode, uint8_t *out_refund_cbor, uint8_t *status, uint8_t *out_nullifier);
int act_node_refund_sign_cbor_batch(act_node *node, size_t n, const uint8_t sk[64], const uint8_t *kprime, const uint8_t *status_in,
                                    const uint8_t *rng, int rng_mode, uint8_t *out_refund_cbor, uint8_t *status);
int act_node_refund_cbor_batch(act_node *node, size_t n, const uint8_t sk[64], const uint8_t *cbor, const uint64_t *offsets,
                               const uint8_t *rng, int rng_mode, uint8_t *out_refund_cbor, uint8_t *status);

/* The issuer's other endpoint on wire bytes: IssuanceRequest::from_cbor (src/cbor.rs:118-148), PrivateKey::issue (src/lib.rs:621-663)
 * and IssuanceResponse::to_cbor (src/cbor.rs:162-175) without an IssuanceRequest, a RistrettoPoint or an IssuanceResponse ever existing on
 * the host.  Messages are delimited as for act_verify_spend_cbor_batch (offsets[0..n] in host memory, or NULL for canonical-size
 * messages back to back; bytes after the first item are ignored); c is n*32 scalars as for act_issue_batch.  Message i in, message i
 * out: out_resp_cbor holds n slots of act_cbor_size(ctx, ACT_CBOR_ISSUANCE_RESPONSE) bytes (176), the canonical IssuanceResponse
 * message of an accepted lane, all zero for any other lane.  status[i]: 0; ACT_STATUS_INVALID_ISSUANCE_REQUEST_PROOF; 255 = K is not a
 * canonical Ristretto encoding (CborError::InvalidValue); ACT_STATUS_CBOR_MALFORMED; ACT_STATUS_CBOR_STRUCTURE -- from_cbor's code for
 * a message that is wrong in several ways (as described at act_cbor_decode_batch).  Canonical messages are unframed by the issue kernel
 * itself (the message is read once, K decoded once) and the responses framed by the signing kernel.  Any other encoding -- an
 * indefinite-length map, another key order, an unknown key, a chunked byte string ... -- is read by the general reader ON THE GPU, in
 * its chunk's own stream in front of the issue kernel, and then checked, signed and framed in the same pipeline as its canonical
 * neighbours (act_ctx_set_wire_reader: ACT_WIRE_READER_HOST keeps the earlier road, the host reader behind the pipeline and one small
 * act_issue_check_batch / act_issue_sign_batch call per window, as a fallback and as the baseline of comparisons; same answers).
 *   act_issue_check_cbor_batch   from_cbor + the PoK check of issue (src/lib.rs:629-640): status, and out_req (nullable, n*128) = the
 *                                request as from_cbor returns it (K as on the wire, scalars reduced mod l), zero where status != 0 --
 *                                for a server that decides c after the verdicts
 *   act_issue_sign_cbor_batch    act_issue_sign_batch for the lanes with status_in == 0, framed as IssuanceResponse messages
 *   act_issue_cbor_batch         the whole endpoint: from_cbor -> issue -> to_cbor
 * rng / rng_mode: ACT_RNG_PER_LANE (lane i: rng + 128 i), ACT_RNG_SEQUENTIAL (consecutive slices to the accepted lanes in lane order)
 * or ACT_RNG_CALLBACK (one draw of 128 x accepted bytes after every verdict is known; a failing draw: ACT_ERR_RNG, nothing signed, every
 * slot zero).  The node forms cut the batch over the GPUs like every act_node_* call. */
int act_issue_check_cbor_batch(act_ctx *ctx, size_t n, int mem, const uint8_t *cbor, const uint64_t *offsets,
                               uint8_t *status, uint8_t *out_req);
int act_issue_sign_cbor_batch(act_ctx *ctx, size_t n, int mem, const uint8_t sk[64], const uint8_t *req, const uint8_t *c,
                              const uint8_t *status_in, const uint8_t *rng, int rng_mode, uint8_t *out_resp_cbor, uint8_t *status);
int act_issue_cbor_batch(act_ctx *ctx, size_t n, int mem, const uint8_t sk[64], const uint8_t *cbor, const uint64_t *offsets,
                         const uint8_t *c, const uint8_t *rng, int rng_mode, uint8_t *out_resp_cbor, uint8_t *status);
int act_node_issue_check_cbor_batch(act_node *node, size_t n, const uint8_t *cbor, const uint64_t *offsets, uint8_t *status,
                                    uint8_t *out_req);
int act_node_issue_sign_cbor_batch(act_node *node, size_t n, const uint8_t sk[64], const uint8_t *req, const uint8_t *c,
                                   const uint8_t *status_in, const uint8_t *rng, int rng_mode, uint8_t *out_resp_cbor, uint8_t *status);
int act_node_issue_cbor_batch(act_node *node, size_t n, const uint8_t sk[64], const uint8_t *cbor, const uint64_t *offsets,
                              const uint8_t *c, const uint8_t *rng, int rng_mode, uint8_t *out_resp_cbor, uint8_t *status);

/* ======== row f4: the nullifier set and the issuer's whole redemption step ====================================================== */
/* Nullifier set: the double-spend database the crate leaves to the caller (src/lib.rs:741-745; `HashSet<Scalar>` with
 * "is_spent? reject : insert" per spend in src/tests.rs:29-50, examples/act.rs:10-30), as a hash set in one GPU's HBM.
 * act_nullifier_check_and_insert_batch has the meaning of that loop run over the batch in lane order: out_spent[i] = 1
 * iff nullifier i is already in the set or equals the nullifier of an earlier lane of this batch; fresh nullifiers are
 * inserted.  Nullifier i is the 32 bytes at nullifiers + i*stride (stride = act_spend_proof_bytes reads the `k` field
 * straight out of SpendProof records).  skip_mask (nullable): lanes with a non-zero byte (e.g. the status of a rejected
 * proof) are neither checked nor inserted and report 0.  Keys are compared as scalars: every nullifier is reduced mod l
 * on input (k and k + l are the same key, as in the reference's HashSet<Scalar>).  capacity = the number of nullifiers
 * the set must hold; `salt` (16 bytes) keys the SipHash-1-3 slot hash; NULL = 16 bytes from the OS (getrandom).  Multi-GPU deployments shard the key space (owner = low 64 bits mod N): one
 * set per GPU behind an all-to-all of the keys, anonymous-credit-tokens_amd/sharded_nullifier.py. */
typedef struct act_nullifier_set act_nullifier_set;
int act_nullifier_set_create(int device, size_t capacity, const uint8_t salt[16], act_nullifier_set **out);
void act_nullifier_set_destroy(act_nullifier_set *set);
size_t act_nullifier_set_len(const act_nullifier_set *set);
const char *act_nullifier_set_last_error(const act_nullifier_set *set);
int act_nullifier_check_and_insert_batch(act_nullifier_set *set, size_t n, int mem, const uint8_t *nullifiers, size_t stride,
                                         const uint8_t *skip_mask, uint8_t *out_spent);

/* Growth, export and read-only look-up (restart and growth: INTEGRATION.md; the snapshot file format:
 * anonymous-credit-tokens_amd/nullifier_snapshot.py).
 * act_nullifier_set_reserve: afterwards the set can hold `capacity` nullifiers (the sizing rule of act_nullifier_set_create).  It
 *   never shrinks: a capacity at or below the current one returns ACT_OK and changes nothing.  capacity > 2^30 returns ACT_ERR_ARG,
 *   set unchanged.  If the new table cannot be allocated (or the rehash does not place every key) the call returns ACT_ERR_HIP and
 *   the set keeps its old table, fully usable.  Otherwise every recorded key is rehashed into the new table on the device under the
 *   set's own salt; len does not change; the set's lock is held for the whole call.  Export cursors taken before a reserve that
 *   grew the set are stale: the next export call refuses them with ACT_ERR_ARG and a last_error text.
 * act_nullifier_set_export: *cursor = 0 on the first call, opaque in between, ACT_NULLIFIER_EXPORT_DONE once every key has been
 *   written.  One call writes at most max_keys (>= 1) keys to out_keys and sets *n_out, which may be 0 even when the cursor moved.
 *   Keys are the reduced scalars, 32 bytes each, in unspecified order.  cursor and n_out are host pointers; `mem` says where
 *   out_keys is.  A loop of calls from 0 to DONE yields every key recorded before its first call exactly once, and may also yield
 *   keys recorded during the loop (slots never move between reserves).
 * act_nullifier_contains_batch: out_found[i] = 1 if nullifier i (compared as a scalar: k and k + l are one key) is recorded, else
 *   0; the set is never modified.  Nullifier i is the 32 bytes at nullifiers + i*stride, as in check-and-insert.  For audit and
 *   status queries only: NOT a substitute for check-and-insert in a spend decision -- a look-up that does not record lets the same
 *   nullifier pass two concurrent callers. */
#define ACT_NULLIFIER_EXPORT_DONE UINT64_MAX
int act_nullifier_set_reserve(act_nullifier_set *set, size_t capacity);
int act_nullifier_set_export(act_nullifier_set *set, uint64_t *cursor, size_t max_keys, int mem, uint8_t *out_keys, size_t *n_out);
int act_nullifier_contains_batch(act_nullifier_set *set, size_t n, int mem, const uint8_t *nullifiers, size_t stride,
                                 uint8_t *out_found);

/* Epochs: every recorded nullifier carries the epoch of the issuer key it was spent under, and a key that has left every ring for
 * good can have its nullifiers removed (the rule for when that is safe: INTEGRATION.md section 8).  An epoch is a uint32_t the caller
 * chooses per issuer key, 0 ... ACT_NULLIFIER_EPOCH_MAX; 0 is "untagged", what every call without epochs records, and can never be
 * retired.  Membership ignores the epoch: a nullifier recorded under any live epoch is a double spend for every later spend; the
 * epoch of the first recorder sticks.  The epoch lives in the high 24 bits of the slot's state word: a slot stays 36 bytes.
 * act_nullifier_check_and_insert_epoch_batch: act_nullifier_check_and_insert_batch where a fresh lane i is recorded under
 *   epoch_table[epoch_index[i]].  epoch_table: HOST memory, 1 <= n_epochs <= 255.  epoch_index: n bytes in `mem` memory (e.g. the out_key
 *   array of a ring verification), or NULL = every lane uses epoch_table[0].  A table entry above ACT_NULLIFIER_EPOCH_MAX or naming a
 *   retired epoch refuses the whole call as a batch without room is refused: ACT_ERR_ARG, nothing recorded, every unmasked lane
 *   ACT_NULLIFIER_UNDETERMINED.  An unmasked lane whose index is not below n_epochs is neither looked up nor recorded and reports
 *   ACT_NULLIFIER_UNDETERMINED; the other lanes are served; the call returns ACT_ERR_ARG.  Table {0} with NULL indices is the existing call.
 * act_nullifier_set_epoch_len: *out_count = the nullifiers recorded under `epoch` (0 for an unknown or retired one); one pass over
 *   the state words on the device.
 * act_nullifier_set_retire_epoch: removes every nullifier of `epoch` (*out_removed, nullable, = how many), gives their slots back and
 *   refuses the epoch from then on.  epoch 0 or above the maximum: ACT_ERR_ARG, set unchanged.  Retiring a retired epoch, or one without
 *   keys, is ACT_OK with 0 removed (and the epoch is remembered).  Built like reserve -- a second table of the same capacity, swapped in
 *   when every other key has been placed; on any failure (ACT_ERR_HIP) the set is exactly as it was and the epoch is NOT retired.  len
 *   drops by *out_removed; capacity does not change; the set's lock is held for the whole call; export cursors taken before a
 *   retirement that removed a key are stale.
 * act_nullifier_set_retired_epochs: the retired epochs, ascending, at most max_epochs of them; *n_out = how many there are.  Host pointers.
 * act_nullifier_set_export_epochs: act_nullifier_set_export with out_epochs[i] (in `mem` memory) the epoch of out_keys[32 i ...]; the two
 *   calls share one cursor space. */
#define ACT_NULLIFIER_EPOCH_MAX 0xFFFFFFu
int act_nullifier_check_and_insert_epoch_batch(act_nullifier_set *set, size_t n, int mem, const uint8_t *nullifiers, size_t stride,
                                               const uint8_t *skip_mask, const uint8_t *epoch_index, const uint32_t *epoch_table,
                                               int n_epochs, uint8_t *out_spent);
int act_nullifier_set_epoch_len(act_nullifier_set *set, uint32_t epoch, uint64_t *out_count);
int act_nullifier_set_retire_epoch(act_nullifier_set *set, uint32_t epoch, uint64_t *out_removed);
int act_nullifier_set_retired_epochs(act_nullifier_set *set, uint32_t *out_epochs, size_t max_epochs, size_t *n_out);
int act_nullifier_set_export_epochs(act_nullifier_set *set, uint64_t *cursor, size_t max_keys, int mem, uint8_t *out_keys,
                                    uint32_t *out_epochs, size_t *n_out);

/* The same set spread over the GPUs of a node: one set per entry of devices[], a nullifier owned by exactly one of them
 * (keyed hash of the reduced scalar), so a batch keeps the sequential meaning above in lane order.  The host buckets the
 * keys by owner (stable), every GPU checks-and-inserts its bucket from its own thread, answers are scattered back:
 * 33 bytes per spend over PCIe, no peer traffic.  Host memory only.  `salt` (16 bytes) keys the routing (SipHash-1-3 of the
 * reduced scalar, so that clients, who choose their nullifiers, cannot aim them at one GPU); NULL = 16 bytes from the OS
 * (getrandom), and creation fails if that fails.  A handle may be shared between host threads (calls are serialised).
 * Failure of one device: the other devices have checked and inserted their keys all the same, so the call fills in their
 * answers (final), marks the lanes owned by the failed device ACT_NULLIFIER_UNDETERMINED in out_spent, and returns the error;
 * only the undetermined lanes may be resubmitted -- a blind retry of the whole batch would report the honest spends that
 * were already inserted as double spends.  The single-GPU form answers the same way: a batch the set has no room for is refused as
 * a whole (nothing recorded, every unmasked lane ACT_NULLIFIER_UNDETERMINED; resubmit to this set after act_nullifier_set_reserve). */
#define ACT_NULLIFIER_UNDETERMINED 2
typedef struct act_node_nullifier_set act_node_nullifier_set;
int act_node_nullifier_set_create(const int *devices, int n_devices, size_t capacity_per_device, const uint8_t salt[16],
                                  act_node_nullifier_set **out);
void act_node_nullifier_set_destroy(act_node_nullifier_set *set);
size_t act_node_nullifier_set_len(const act_node_nullifier_set *set);
const char *act_node_nullifier_set_last_error(const act_node_nullifier_set *set);
int act_node_nullifier_check_and_insert_batch(act_node_nullifier_set *set, size_t n, const uint8_t *nullifiers, size_t stride,
                                              const uint8_t *skip_mask, uint8_t *out_spent);
/* Node forms of reserve / export / contains (meanings above).  reserve: every device's set is reserved to capacity_per_device; if
 * one fails, the error names it, every set stays valid and some may already have grown.  export: host memory only; the cursor
 * walks the devices in turn (a cursor is refused when the device it stopped inside has been grown since).  contains: the keys
 * are routed by owner exactly as in check-and-insert and the answers scattered back. */
int act_node_nullifier_set_reserve(act_node_nullifier_set *set, size_t capacity_per_device);
int act_node_nullifier_set_export(act_node_nullifier_set *set, uint64_t *cursor, size_t max_keys, uint8_t *out_keys, size_t *n_out);
int act_node_nullifier_contains_batch(act_node_nullifier_set *set, size_t n, const uint8_t *nullifiers, size_t stride,
                                      uint8_t *out_found);
/* Node forms of the epoch calls (host memory).  check-and-insert: routed by owner as above, the lanes' epoch indices with them.
 * epoch_len: the sum over the devices.  retire_epoch: device after device; a failure names the device, leaves every set valid and some
 * already retired, and a repeat of the call finishes the job.  retired_epochs: the epochs EVERY device has retired (an insert naming an
 * epoch that any device has retired is refused all the same).  export_epochs shares the cursor space of act_node_nullifier_set_export. */
int act_node_nullifier_check_and_insert_epoch_batch(act_node_nullifier_set *set, size_t n, const uint8_t *nullifiers, size_t stride,
                                                    const uint8_t *skip_mask, const uint8_t *epoch_index, const uint32_t *epoch_table,
                                                    int n_epochs, uint8_t *out_spent);
int act_node_nullifier_set_epoch_len(act_node_nullifier_set *set, uint32_t epoch, uint64_t *out_count);
int act_node_nullifier_set_retire_epoch(act_node_nullifier_set *set, uint32_t epoch, uint64_t *out_removed);
int act_node_nullifier_set_retired_epochs(act_node_nullifier_set *set, uint32_t *out_epochs, size_t max_epochs, size_t *n_out);
int act_node_nullifier_set_export_epochs(act_node_nullifier_set *set, uint64_t *cursor, size_t max_keys, uint8_t *out_keys,
                                         uint32_t *out_epochs, size_t *n_out);

/* The issuer's whole redemption step -- verify, look the nullifier up, record it, sign the refund (examples/act.rs:62-73; the
 * NullifierDb loops of src/tests.rs) -- as one call with the result of the loop
 *     for i in 0..n:  refund(proof_i)'s checks fail (src/lib.rs:787-844)  -> status[i] = that error; nothing recorded, no rng drawn
 *                     nullifier_i already in the set, or spent by an earlier accepted lane of this batch
 *                                                                        -> status[i] = ACT_STATUS_DOUBLE_SPEND; no rng drawn
 *                     otherwise: recorded, signed (src/lib.rs:846-868)    -> status[i] = 0, out_refund[i]
 * Verification comes first, so a proof that does not verify cannot burn a nullifier (the crate's example marks the nullifier
 * before calling refund and unwraps: same result for valid proofs).  rng / rng_mode as in act_refund_batch: ACT_RNG_SEQUENTIAL hands
 * consecutive 128-byte slices to the lanes that are SIGNED.  The set must live on the context's device.  The node form runs the
 * verification and the signatures on all GPUs and the look-up through the node-level set.  The three steps take their handles'
 * locks one after the other: concurrent callers interleave between steps, never inside one.
 * Failures: a non-zero result never hides a decision already taken -- status[] is complete when the call returns.
 *   verification failed (a HIP error)   nothing recorded, nothing signed; status[] not written.
 *   the nullifier step failed           lanes it answered are finished as usual (0 + refund, or ACT_STATUS_DOUBLE_SPEND); lanes it could
 *                                       not answer -- the set was too small for the batch, or (node form) their owner GPU failed -- get
 *                                       ACT_STATUS_NULLIFIER_UNDETERMINED: not recorded, not signed, safe to resubmit.
 *   the signature step failed           nullifiers ARE recorded; the lanes that were to be signed (node form: those of the failing GPU's
 *                                       shard) get ACT_STATUS_RECORDED_UNSIGNED and a zero record.  Their refund is owed: call
 *                                       act_verify_spend_batch(out_kprime) and act_refund_sign_batch on exactly those lanes.  Redeeming them
 *                                       again would report DoubleSpendError and the client would lose its credits.
 * A few items at a time (host memory, at most 64, rng slices that do not depend on the verdicts: ACT_RNG_PER_LANE bytes, or ONE item
 * with its 128 bytes): the refunds are computed FIRST -- one call, the signature beside the verification -- and the store then decides
 * which of them are handed out (2.1 ms for one item instead of 3.2).  Same statuses, refunds and store; the third failure above cannot
 * occur on this road (nothing is signed behind a recorded nullifier). */
int act_redeem_batch(act_ctx *ctx, act_nullifier_set *set, size_t n, int mem, const uint8_t sk[64], const uint8_t *proof,
                     const uint8_t *rng, int rng_mode, uint8_t *out_refund, uint8_t *status);
int act_node_redeem_batch(act_node *node, act_node_nullifier_set *set, size_t n, const uint8_t sk[64], const uint8_t *proof,
                          const uint8_t *rng, int rng_mode, uint8_t *out_refund, uint8_t *status);
/* The redemption step on wire bytes: act_redeem_batch with CBOR SpendProof messages in (as act_verify_spend_cbor_batch) and CBOR Refund
 * messages out (as act_refund_cbor_batch) -- the loop of examples/act.rs:62-73 for a server that holds bytes.  status[i] additionally
 * takes the wire codes 255 / ACT_STATUS_CBOR_MALFORMED / ACT_STATUS_CBOR_STRUCTURE; failure semantics as above.
 * All four redeem entry points accept ACT_RNG_CALLBACK: the draw happens after the nullifier step, for the lanes that are signed. */
int act_redeem_cbor_batch(act_ctx *ctx, act_nullifier_set *set, size_t n, int mem, const uint8_t sk[64], const uint8_t *cbor,
                          const uint64_t *offsets, const uint8_t *rng, int rng_mode, uint8_t *out_refund_cbor, uint8_t *status);
int act_node_redeem_cbor_batch(act_node *node, act_node_nullifier_set *set, size_t n, const uint8_t sk[64], const uint8_t *cbor,
                               const uint64_t *offsets, const uint8_t *rng, int rng_mode, uint8_t *out_refund_cbor, uint8_t *status);

/* ======== key rotation: one batch against a ring of issuer keys ========================================================================
 * A SpendProof carries no key identifier.  While an issuer rotates its key -- the old key live until its tokens are spent or expired,
 * the new one for everything issued since -- these calls verify every proof ONCE and say per lane WHICH key it verified under, for
 * under 1 % of a verification per extra key, instead of one pass per key over the lanes the previous pass rejected.
 *   keys      nkeys records of 64 bytes (x | enc(w), the `sk` layout), 1 <= nkeys <= ACT_KEYRING_MAX, in the caller's order of preference.
 *             nkeys out of range or a null ring: ACT_ERR_ARG; a w that is not a canonical encoding: ACT_ERR_PARAMS.  Nothing of a
 *             rejected ring is kept, and no ring call touches the key the one-key calls have cached.
 *   out_key   per lane: the SMALLEST ring index k whose PrivateKey::refund accepts the proof (status 0); ACT_KEY_NONE on every other
 *             lane (255 / ACT_STATUS_IDENTITY_POINT, which do not depend on the key, and ACT_STATUS_INVALID_CLIENT_SPEND_PROOF = no
 *             ring key accepts it).  Output records of rejected lanes are all zero, as in the one-key calls.  In the redeem calls a
 *             lane that verified and is then found ACT_STATUS_DOUBLE_SPEND / NULLIFIER_UNDETERMINED / RECORDED_UNSIGNED keeps the
 *             index it matched.
 *   sign_key  ACT_SIGN_MATCHED: lane p's refund is signed with ring key out_key[p] -- byte for byte PrivateKey::refund of that key over
 *             the lane's rng slice; 0 <= sign_key < nkeys: every accepted lane is signed with that one key, which moves the client onto
 *             it with its next token (the refund verifies under w[sign_key] only).  Anything else: ACT_ERR_ARG.
 *   key_index (act_refund_sign_keyring_batch) the index per lane, in `mem` memory: a lane with status_in 0 whose index is not below nkeys
 *             is not signed -- status 255, zero record, no rng slice consumed.
 * rng conventions are those of the one-key call of the same name (ACT_RNG_CALLBACK in the redeem calls only); the generator is touched
 * after every verdict (and nullifier answer) is known.  nkeys == 1 gives the bytes of the one-key call.  The nullifier set does not
 * depend on the key: a nullifier spent under the old key stays spent (until that key's epoch is retired, below).  Always the pipelined chunk schedule, whatever n. */
#define ACT_KEYRING_MAX 4
#define ACT_KEY_NONE 255
#define ACT_SIGN_MATCHED (-1)
int act_verify_spend_keyring_batch(act_ctx *ctx, size_t n, int mem, const uint8_t *keys, int nkeys, const uint8_t *proof, uint8_t *status,
                                   uint8_t *out_key, uint8_t *out_kprime /* nullable */);
int act_refund_sign_keyring_batch(act_ctx *ctx, size_t n, int mem, const uint8_t *keys, int nkeys, const uint8_t *key_index, const uint8_t *kprime,
                                  const uint8_t *status_in, const uint8_t *rng, int rng_mode, uint8_t *out_refund, uint8_t *status);
int act_redeem_keyring_batch(act_ctx *ctx, act_nullifier_set *set, size_t n, int mem, const uint8_t *keys, int nkeys, int sign_key,
                             const uint8_t *proof, const uint8_t *rng, int rng_mode, uint8_t *out_refund, uint8_t *status, uint8_t *out_key);
int act_redeem_cbor_keyring_batch(act_ctx *ctx, act_nullifier_set *set, size_t n, int mem, const uint8_t *keys, int nkeys, int sign_key,
                                  const uint8_t *cbor, const uint64_t *offsets, const uint8_t *rng, int rng_mode, uint8_t *out_refund_cbor,
                                  uint8_t *status, uint8_t *out_key);
/* The same over the GPUs of a node (host memory; out_key is cut per piece like status; ACT_RNG_SEQUENTIAL stays exact across pieces). */
int act_node_verify_spend_keyring_batch(act_node *node, size_t n, const uint8_t *keys, int nkeys, const uint8_t *proof, uint8_t *status,
                                        uint8_t *out_key, uint8_t *out_kprime /* nullable */);
int act_node_refund_sign_keyring_batch(act_node *node, size_t n, const uint8_t *keys, int nkeys, const uint8_t *key_index, const uint8_t *kprime,
                                       const uint8_t *status_in, const uint8_t *rng, int rng_mode, uint8_t *out_refund, uint8_t *status);
int act_node_redeem_keyring_batch(act_node *node, act_node_nullifier_set *set, size_t n, const uint8_t *keys, int nkeys, int sign_key,
                                  const uint8_t *proof, const uint8_t *rng, int rng_mode, uint8_t *out_refund, uint8_t *status, uint8_t *out_key);
int act_node_redeem_cbor_keyring_batch(act_node *node, act_node_nullifier_set *set, size_t n, const uint8_t *keys, int nkeys, int sign_key,
                                       const uint8_t *cbor, const uint64_t *offsets, const uint8_t *rng, int rng_mode, uint8_t *out_refund_cbor,
                                       uint8_t *status, uint8_t *out_key);
/* The ring redemption calls with epochs: key_epochs = nkeys values in HOST memory, key_epochs[k] the epoch of ring key k.  Everything
 * the calls above return is byte for byte the same; an accepted lane's nullifier is recorded under the epoch of the key its proof
 * MATCHED (key_epochs[out_key[i]]), never the key it is signed with: the nullifier belongs to the token being spent.  An epoch above
 * ACT_NULLIFIER_EPOCH_MAX or a retired one fails the call with ACT_ERR_ARG before any verification: nothing recorded, nothing
 * signed, status[] not written. */
int act_redeem_keyring_epochs_batch(act_ctx *ctx, act_nullifier_set *set, size_t n, int mem, const uint8_t *keys, int nkeys,
                                    const uint32_t *key_epochs, int sign_key, const uint8_t *proof, const uint8_t *rng, int rng_mode,
                                    uint8_t *out_refund, uint8_t *status, uint8_t *out_key);
int act_redeem_cbor_keyring_epochs_batch(act_ctx *ctx, act_nullifier_set *set, size_t n, int mem, const uint8_t *keys, int nkeys,
                                         const uint32_t *key_epochs, int sign_key, const uint8_t *cbor, const uint64_t *offsets,
                                         const uint8_t *rng, int rng_mode, uint8_t *out_refund_cbor, uint8_t *status, uint8_t *out_key);
int act_node_redeem_keyring_epochs_batch(act_node *node, act_node_nullifier_set *set, size_t n, const uint8_t *keys, int nkeys,
                                         const uint32_t *key_epochs, int sign_key, const uint8_t *proof, const uint8_t *rng, int rng_mode,
                                         uint8_t *out_refund, uint8_t *status, uint8_t *out_key);
int act_node_redeem_cbor_keyring_epochs_batch(act_node *node, act_node_nullifier_set *set, size_t n, const uint8_t *keys, int nkeys,
                                              const uint32_t *key_epochs, int sign_key, const uint8_t *cbor, const uint64_t *offsets,
                                              const uint8_t *rng, int rng_mode, uint8_t *out_refund_cbor, uint8_t *status, uint8_t *out_key);

/* ======== key rotation, the client's side: to_credit_token against a ring of issuer PUBLIC keys ========================================
 * Neither an IssuanceResponse nor a Refund names the key it was signed with, and with sign_key the server moves a client onto a new key
 * with its next refund.  These two calls verify every item ONCE and say per lane under WHICH published key it verified: w enters the
 * client's check only through X_g and Y_g, so an extra key costs two fixed-base products on g, one on an 8-bit table of w_k, a mixed
 * addition, two encodings and one single-chunk BLAKE3 per item (0.4 of one variable-base product) instead of a whole verification -- and no key identifier, which
 * would be a tagging channel chosen by the server, has to travel beside the message.
 *   ring_w    nkeys encodings of 32 bytes, 1 <= nkeys <= ACT_KEYRING_MAX, in the caller's order of preference; always HOST memory, like w
 *             in the one-key calls.  nkeys out of range, a null ring or an entry that is not a canonical encoding: ACT_ERR_ARG before
 *             anything is launched.  Duplicate entries are legal: the first one wins.
 *   out_key   per lane: the SMALLEST ring index under which the one-key call accepts the item; ACT_KEY_NONE on every lane whose status
 *             is not 0.
 *   status, out_token   those of the one-key call under that key: 255 = undecodable, whatever the ring; 2 (issuance) / 4 (refund) = no
 *             ring key verifies; a rejected lane's token is all zero.
 * nkeys == 1 gives the bytes of the one-key call.  The secret pre records are staged and wiped as there; the ring's tables and side
 * buffers (public data) are allocated by a context's first call of this kind.  There is no tiny or fused road for rings: always the
 * chunked launches, whatever n. */
int act_issuance_to_credit_token_keyring_batch(act_ctx *ctx, size_t n, int mem, const uint8_t *pre, const uint8_t *ring_w, uint32_t nkeys,
                                               const uint8_t *req, const uint8_t *resp, uint8_t *out_token, uint8_t *status,
                                               uint8_t *out_key);
int act_refund_to_credit_token_keyring_batch(act_ctx *ctx, size_t n, int mem, const uint8_t *prerefund, const uint8_t *proof,
                                             const uint8_t *refund, const uint8_t *ring_w, uint32_t nkeys, uint8_t *out_token,
                                             uint8_t *status, uint8_t *out_key);

/* ======== admission before verification: the expected charge and the spent nullifiers first ========
 * The redeem calls above verify, then look up and record, then sign: a replayed proof costs a whole verification before the set
 * answers DoubleSpendError, and nothing compares SpendProof.s with what the request costs.  These two calls put an admission stage in
 * front.  They are the superset forms (ring and epoch parameters); nkeys == 1 with key_epochs == NULL is the one-key call.  In lane
 * order:
 *     for i in 0..n:
 *       1. wire form only: the message fails structurally -> exactly the code act_redeem_cbor_* gives (ACT_STATUS_CBOR_MALFORMED /
 *          ACT_STATUS_CBOR_STRUCTURE, and 255 where an invalid point stands in front of the fault in wire order).  A well-shaped
 *          message, its points not yet validated, goes on.  Every legal spelling is read, not only the canonical one.
 *       2. charge != NULL and s_i != charge_i (both reduced mod l)      -> ACT_STATUS_WRONG_CHARGE: not looked up, not verified, not
 *          recorded, not signed; no trace in the set -- the token can be redeemed later at the right price
 *       3. k_i (reduced) is in the set when the call looks it up         -> ACT_STATUS_DOUBLE_SPEND, NOT verified
 *       4. otherwise exactly act_redeem_(cbor_)keyring_epochs_batch: verification (255 / 6 / 7, out_key), check-and-insert (in the
 *          set, or spent by an earlier ACCEPTED lane of this batch -> ACT_STATUS_DOUBLE_SPEND), recorded under the matched key's
 *          epoch (untagged without key_epochs), signed
 * charge: nullable; n scalars of 32 bytes in `mem` memory, laid out like SpendProof.s.
 * What stays the same: with charge == NULL the accepted lanes, their refund bytes, their out_key, the nullifiers recorded with their
 * epochs and what is drawn from the generator are byte for byte those of act_redeem_(cbor_)keyring_epochs_batch on an identical set --
 * ACT_RNG_SEQUENTIAL slices go to the signed lanes in lane order, ACT_RNG_CALLBACK makes one draw of 128 x accepted bytes per call,
 * ACT_RNG_PER_LANE uses the ORIGINAL lane's slice.
 * What may differ: only the rejection code of a lane that is rejected for more than one reason.  A spent nullifier with a tampered or
 * undecodable proof reports ACT_STATUS_DOUBLE_SPEND here and 7 / 255 there; a lane shed in steps 1-3 has out_key = ACT_KEY_NONE and an
 * all-zero output record.
 * Lanes that share a FRESH nullifier cannot be shed up front (the first VALID one wins): all of them are verified, as in the redeem calls.
 * The look-up of step 3 is read-only.  The decision that records is still the check-and-insert behind verification: a nullifier that a
 * concurrent caller records in between is caught there.
 * Failure semantics are those of act_redeem_* (ACT_STATUS_NULLIFIER_UNDETERMINED / ACT_STATUS_RECORDED_UNSIGNED, status[] complete on
 * return).  A HIP failure in the admission stage itself: nothing recorded, nothing signed, status[] not written.
 * out_counts: nullable, HOST memory, ACT_ADMIT_COUNTS values: lanes, wire_rejected (step 1), wrong_charge, spent_before (step 3),
 * verified (= lanes - wire_rejected - wrong_charge - spent_before: the lanes that cost a verification), rejected_by_verification,
 * double_spend_after (step 4's check-and-insert), accepted. */
#define ACT_STATUS_WRONG_CHARGE 250   /* admission: s != the expected charge; not verified, not recorded, not signed */
#define ACT_ADMIT_COUNTS 8
int act_redeem_admit_batch(act_ctx *ctx, act_nullifier_set *set, size_t n, int mem, const uint8_t *keys, int nkeys,
                           const uint32_t *key_epochs /* nullable */, int sign_key, const uint8_t *proof, const uint8_t *charge /* nullable */,
                           const uint8_t *rng, int rng_mode, uint8_t *out_refund, uint8_t *status, uint8_t *out_key,
                           uint64_t *out_counts /* nullable, host */);
int act_redeem_cbor_admit_batch(act_ctx *ctx, act_nullifier_set *set, size_t n, int mem, const uint8_t *keys, int nkeys,
                                const uint32_t *key_epochs /* nullable */, int sign_key, const uint8_t *cbor, const uint64_t *offsets,
                                const uint8_t *charge /* nullable */, const uint8_t *rng, int rng_mode, uint8_t *out_refund_cbor,
                                uint8_t *status, uint8_t *out_key, uint64_t *out_counts /* nullable, host */);

/* ======== admission, unique forms: byte-identical proofs of one batch are verified once ========
 * The two calls above verify every lane that shares a FRESH nullifier, because any of them may be the first valid one.  Lanes with
 * IDENTICAL input bytes have the same verdict and the same matched key by definition, so one verification answers all of them.  These
 * two calls run the admission loop above with one more step between step 3 and step 4:
 *       3a. lane i has passed steps 1-3, and an earlier lane j < i that has also passed them has the same input bytes -> lane i is a
 *           COPY and is not verified.  Its leader is the smallest such j; a leader is never itself a copy.
 *           Records form: the input bytes are the whole act_spend_proof_bytes record.  Wire form: the message's bytes
 *           [offsets[i], offsets[i + 1]), the same length and the same content -- two different spellings of one proof, or one message
 *           with and without a trailing byte, are NOT copies of each other (both are verified, as above).
 * After the call's single check-and-insert and signing pass a copy is answered from its leader's FINAL status:
 *       leader 255 / 6 / 7, ACT_STATUS_DOUBLE_SPEND, ACT_STATUS_NULLIFIER_UNDETERMINED   -> the same status
 *       leader 0 or ACT_STATUS_RECORDED_UNSIGNED (its nullifier is recorded)           -> ACT_STATUS_DOUBLE_SPEND
 * and in every case out_key[i] = out_key[j] (a verified lane that is then a double spend keeps the index it matched), an all-zero
 * output record, and no rng slice: copies never sign, so ACT_RNG_SEQUENTIAL slices and the one ACT_RNG_CALLBACK draw are unchanged.
 * What stays the same: every status, every out_key, every output byte, the nullifiers recorded with their epochs and what is drawn
 * from the generator (all three conventions) are byte for byte those of act_redeem_(cbor_)admit_batch on the same batch and an
 * identical set.  (Not promised where lanes end ACT_STATUS_NULLIFIER_UNDETERMINED: a set too small for the batch.)
 * What differs: only out_counts.  ACT_ADMIT_UNIQUE_COUNTS values: the eight above, then copies.  verified = lanes - wire_rejected -
 * wrong_charge - spent_before - copies; rejected_by_verification, double_spend_after and accepted count VERIFIED lanes only (their
 * sum is verified when nothing is undetermined or unsigned).
 * Equality is decided on the bytes themselves: a 64-bit fingerprint keyed with the set's salt only finds candidates, and a collision
 * costs a verification and never changes an answer.  Whole-call refusals, failure semantics and the hygiene contract are those of the
 * two calls above; nothing secret is staged (proofs, fingerprints and lane numbers are public).  A batch without copies in which
 * nothing is shed still goes straight to the redeem call; a batch in which nothing survives still launches no verification kernel. */
#define ACT_ADMIT_UNIQUE_COUNTS 9
int act_redeem_admit_unique_batch(act_ctx *ctx, act_nullifier_set *set, size_t n, int mem, const uint8_t *keys, int nkeys,
                                  const uint32_t *key_epochs /* nullable */, int sign_key, const uint8_t *proof, const uint8_t *charge /* nullable */,
                                  const uint8_t *rng, int rng_mode, uint8_t *out_refund, uint8_t *status, uint8_t *out_key,
                                  uint64_t *out_counts /* nullable, host */);
int act_redeem_cbor_admit_unique_batch(act_ctx *ctx, act_nullifier_set *set, size_t n, int mem, const uint8_t *keys, int nkeys,
                                       const uint32_t *key_epochs /* nullable */, int sign_key, const uint8_t *cbor, const uint64_t *offsets,
                                       const uint8_t *charge /* nullable */, const uint8_t *rng, int rng_mode, uint8_t *out_refund_cbor,
                                       uint8_t *status, uint8_t *out_key, uint64_t *out_counts /* nullable, host */);

/* ======== replayable redemption: a retried SpendProof gets its Refund again ========
 * The redeem calls above record the nullifier and then sign; the refund exists only in the call's output buffer.  A client whose
 * response was lost resends the same SpendProof, gets DoubleSpendError and loses its remaining credits.  These two calls are
 * act_redeem_(cbor_)keyring_epochs_batch (key_epochs nullable; nkeys == 1 is the one-key call) made retry-safe without storing a refund:
 *   derived nonces  the lane's 128 nonce bytes are not drawn from a generator (there is no rng / rng_mode) but derived from the
 *                   issuer's `nonce_key`, the key the lane is SIGNED with, the nullifier and enc(K'): signing the same spend again
 *                   gives the same refund byte for byte, a different spend gets independent nonces.
 *   receipts        a second, ordinary act_nullifier_set records one 32-byte tag per recorded nullifier: WHICH K' it was spent for.
 * Exact definitions (BLAKE3, default mode; every input has a fixed length, so nothing is length-prefixed; k_i = the lane's
 * nullifier reduced mod l, 32 bytes little-endian; key_j = the 64-byte record x | enc(w) of the key lane i is signed with):
 *     tag_i   = BLAKE3("act-mi355x/receipt/v1" zero-padded to 32 bytes | k_i | enc(K'_i))[0:32] with byte 31 &= 0x0F
 *     nonce_i = BLAKE3-XOF("act-mi355x/refund-nonce/v1" zero-padded to 32 bytes | nonce_key | key_j | k_i | enc(K'_i), 128 bytes)
 * The refund of lane i is byte for byte act_refund_sign_keyring_batch over enc(K'_i) with nonce_i as its ACT_RNG_PER_LANE slice.
 * In lane order:
 *     1. verification exactly as in the ring redeem call, records or wire (every legal spelling, read as act_ctx_set_wire_reader
 *        says; 255 / 6 / 7 and the CBOR codes unchanged; out_key unchanged)
 *     2. check-and-insert of k into `set`, under the matched key's epoch when key_epochs is given
 *     3. k was fresh: the lane's tag is recorded in `receipts` under the same epoch (ONLY then: a double spender cannot plant a tag)
 *     4. k was spent -- before the call or by an earlier lane of this batch -- and the tag is in `receipts`: this is the very spend
 *        that was recorded, a REPLAY: status 0, out_replayed[i] = 1, signed again.  Tag absent: another spend of the same token,
 *        ACT_STATUS_DOUBLE_SPEND and a zero record as in the redeem calls (the lane keeps the out_key it matched).
 *     5. fresh and replayed lanes are signed with nonce_i, by ring key sign_key or the matched key (ACT_SIGN_MATCHED); the wire form
 *        frames Refund messages.
 * Why this is safe: the refund depends only on K', and K' commits to the new nullifier k*, to r* and to c - s.  Handing the same
 * refund out twice gives the holder ONE token with nullifier k*, which can be spent once.  A second proof for the same k with another
 * K' -- the actual double spend -- has another tag and is refused.  A replay is verified again: it costs what a double spend costs.
 * What follows:
 *   - a retry after the original call returned gets the identical refund bytes as long as the signing key and nonce_key are the same
 *     -- also on another context, after export / restore of BOTH sets, and when the retry is another CBOR spelling of the same proof.
 *   - if sign_key has moved in between, the retry gets a different refund, valid under the new key for the same K'; likewise a
 *     rotated nonce_key gives a different, still valid refund.  (Either way the client holds one K' and can finish one of them.)
 *   - a retry that races its original call may still see ACT_STATUS_DOUBLE_SPEND once (k recorded, receipt not yet).
 *   - failures are those of act_redeem_*: ACT_STATUS_NULLIFIER_UNDETERMINED lanes are not recorded and get no receipt; after a failed
 *     signature step lanes say ACT_STATUS_RECORDED_UNSIGNED, and their repair is now TO CALL THIS CALL AGAIN with the same lanes (the
 *     receipt was written before signing).  A failure of the receipts step after k was recorded never withholds a refund: the lanes
 *     are signed, the call returns the receipts set's error with its text, and only the retry of those lanes is lost.
 *   - retire an epoch on BOTH sets.  The existing act_redeem_* calls, and a set that never sees one of these calls, are unchanged.
 * Refused as a whole before any GPU work (nothing verified, nothing recorded, status[] not written), ACT_ERR_ARG: everything the ring
 * redeem calls refuse; receipts NULL, the same handle as set, or on another device; nonce_key NULL; an epoch table either set
 * refuses; a receipts set that cannot take n more keys by the set's own room rule (len + n > slots / 2: act_nullifier_set_reserve it).
 * out_replayed: nullable, n bytes in `mem` memory.  out_counts: nullable, HOST memory, ACT_REPLAY_COUNTS values: lanes,
 * rejected_by_verification, fresh (recorded and signed), replayed, double_spend, unanswered (UNDETERMINED or RECORDED_UNSIGNED).
 * One replay call runs at a time per context; nonce_key, the ring and the derived nonces are staged in buffers of the context that
 * are wiped on every exit.  Always the pipelined chunk schedule, whatever n. */
#define ACT_REPLAY_COUNTS 6
int act_redeem_replay_batch(act_ctx *ctx, act_nullifier_set *set, act_nullifier_set *receipts, size_t n, int mem, const uint8_t *keys, int nkeys,
                            const uint32_t *key_epochs /* nullable */, int sign_key, const uint8_t *proof, const uint8_t nonce_key[32],
                            uint8_t *out_refund, uint8_t *status, uint8_t *out_key, uint8_t *out_replayed /* nullable */,
                            uint64_t *out_counts /* nullable, host */);
int act_redeem_cbor_replay_batch(act_ctx *ctx, act_nullifier_set *set, act_nullifier_set *receipts, size_t n, int mem, const uint8_t *keys, int nkeys,
                                 const uint32_t *key_epochs /* nullable */, int sign_key, const uint8_t *cbor, const uint64_t *offsets,
                                 const uint8_t nonce_key[32], uint8_t *out_refund_cbor, uint8_t *status, uint8_t *out_key,
                                 uint8_t *out_replayed /* nullable */, uint64_t *out_counts /* nullable, host */);
/* The building block of the two calls above, for callers that compose the same thing from act_node_verify_spend_keyring_batch, two
 * node-level sets and act_node_refund_sign_keyring_batch: out_tags[i] (32 bytes) and out_nonces[i] (128 bytes) of every lane with
 * status_in[i] == 0 and key_index[i] < nkeys (the key the lane is to be SIGNED with); every other lane gets zeros.  nullifiers:
 * lane i at nullifiers + i * stride (stride >= 32; reduced here).  All arrays in `mem` memory; keys and nonce_key in host memory. */
int act_replay_derive_batch(act_ctx *ctx, size_t n, int mem, const uint8_t *keys, int nkeys, const uint8_t *key_index,
                            const uint8_t nonce_key[32], const uint8_t *nullifiers, size_t stride, const uint8_t *kprime,
                            const uint8_t *status_in, uint8_t *out_tags /* nullable */, uint8_t *out_nonces /* nullable */);

/* ======== admission for the replayable redemption: retries are recognised BEFORE they are verified ========
 * Behind the admission calls an honest retry is ACT_STATUS_DOUBLE_SPEND; behind the replay calls every lane whose nullifier is spent is
 * verified at full price before the receipts can say whether it is a retry.  These two calls are act_redeem_(cbor_)replay_batch with
 * the admission screen in front, and the screen asks the receipts: tag_i (defined above) needs only k_i and enc(K'_i), and
 * K'_i = sum_j 2^j Com_j is a function of the proof's bytes alone -- L point decodings, one Horner run and one encoding; no key, no
 * transcript, no range kernel.  In lane order:
 *     for i in 0..n:
 *       1. wire form only: the message fails structurally -> exactly the code act_redeem_cbor_* gives, under either
 *          act_ctx_set_wire_reader setting, for every legal spelling
 *       2. charge != NULL and s_i != charge_i (both reduced mod l)      -> ACT_STATUS_WRONG_CHARGE: not looked up, not verified, no
 *          trace in either set
 *       3. k_i (reduced) is in `set` when the call looks it up: enc(K'_i) is computed from the lane's Com_j, tag_i from it, and tag_i is
 *          looked up in `receipts`, read only
 *          3a. a Com_j does not decode, or the tag is absent            -> ACT_STATUS_DOUBLE_SPEND, NOT verified, ACT_KEY_NONE and an
 *              all-zero record
 *          3b. the tag is present: the lane is a retry CANDIDATE and goes on
 *       4. every remaining lane, fresh or candidate: exactly act_redeem_(cbor_)replay_batch over those lanes in lane order --
 *          verification, check-and-insert under the matched key's epoch, a receipt only where k was fresh, a replay where the tag is
 *          found, derived nonces, signing, out_replayed
 * Why 3a is safe: a receipt for k is written only by the lane that found k fresh.  k was spent before this call's look-up, so no lane
 * of this batch can write one: a lane whose k is in the set and whose tag is not in `receipts` can only end 3 / 6 / 7 / 255 in the
 * replay call, never 0.  The screen never accepts anything: every refund is still behind a full verification, the check-and-insert
 * and the receipts look-up of step 4.
 * What stays the same: with charge == NULL every accepted lane and its refund bytes, out_key, out_replayed and the keys and epochs
 * both sets hold afterwards are byte for byte those of act_redeem_(cbor_)replay_batch on the same batch and identical sets.
 * What may differ: only the rejection code of a lane rejected for more than one reason -- a foreign spend (step 3a) that is also
 * tampered or undecodable reports ACT_STATUS_DOUBLE_SPEND here and 7 / 255 there; a lane shed in steps 1-3 has out_key = ACT_KEY_NONE.
 * A retry that races its original call may see ACT_STATUS_DOUBLE_SPEND once: both look-ups of step 3 are read-only, and the race the
 * replay calls document (k recorded, receipt not yet) also exists at the screen.
 * Refused as a whole: everything the admission calls and the replay calls refuse, the receipts' room rule computed with n included.
 * Failure semantics (ACT_STATUS_NULLIFIER_UNDETERMINED / ACT_STATUS_RECORDED_UNSIGNED, status[] complete on return, a receipts
 * failure never withholds a refund) are those of the replay calls; a HIP failure inside the screen leaves nothing recorded, nothing
 * signed and status[] not written.  A batch in which nothing is shed goes straight to the replay implementation with the caller's
 * pointers; a batch in which nothing survives launches no verification kernel.  One call at a time per context (the admission calls'
 * lock, then the replay calls').
 * out_counts: nullable, HOST memory, ACT_ADMIT_REPLAY_COUNTS values: lanes, wire_rejected (step 1), wrong_charge (step 2),
 * foreign_spend (step 3a), retry_candidates (step 3b), verified (= lanes - wire_rejected - wrong_charge - foreign_spend),
 * rejected_by_verification, fresh (recorded and signed), replayed (signed again from a found receipt), double_spend_after (step 4's
 * check-and-insert), unanswered (UNDETERMINED or RECORDED_UNSIGNED). */
#define ACT_ADMIT_REPLAY_COUNTS 11
int act_redeem_admit_replay_batch(act_ctx *ctx, act_nullifier_set *set, act_nullifier_set *receipts, size_t n, int mem, const uint8_t *keys, int nkeys,
                                  const uint32_t *key_epochs /* nullable */, int sign_key, const uint8_t *proof, const uint8_t *charge /* nullable */,
                                  const uint8_t nonce_key[32], uint8_t *out_refund, uint8_t *status, uint8_t *out_key,
                                  uint8_t *out_replayed /* nullable */, uint64_t *out_counts /* nullable, host */);
int act_redeem_cbor_admit_replay_batch(act_ctx *ctx, act_nullifier_set *set, act_nullifier_set *receipts, size_t n, int mem, const uint8_t *keys, int nkeys,
                                       const uint32_t *key_epochs /* nullable */, int sign_key, const uint8_t *cbor, const uint64_t *offsets,
                                       const uint8_t *charge /* nullable */, const uint8_t nonce_key[32], uint8_t *out_refund_cbor, uint8_t *status,
                                       uint8_t *out_key, uint8_t *out_replayed /* nullable */, uint64_t *out_counts /* nullable, host */);

/* ======== admission for the replayable redemption, unique forms: copies in one batch are verified and signed once ========
 * A client whose response was lost resends the same SpendProof, and resends it several times while the server is slow -- which is when
 * batches are largest.  Byte-identical copies of one proof inside one batch are the normal load behind the two calls above, and they
 * answer them the expensive way: every copy passes the screen (fresh, or a retry candidate), is verified in full and is signed again
 * with the derived nonces, for the same bytes n times.  The admission unique forms cannot stand in: they answer the copy of an accepted
 * leader ACT_STATUS_DOUBLE_SPEND.  These two calls run the admit-replay loop above with one more step between step 3 and step 4, which
 * is step 3a of the admission unique forms unchanged:
 *       3c. lane i has passed steps 1-3, as a fresh lane or as a retry candidate, and an earlier lane j < i that has also passed them
 *           has the same input bytes -> lane i is a COPY and is not verified.  Its leader is the smallest such j; a leader is never
 *           itself a copy.  Records form: the whole act_spend_proof_bytes record.  Wire form: the bytes [offsets[i], offsets[i + 1]),
 *           the same length and the same content -- two different spellings of one proof, or one message with and without a trailing
 *           byte, are NOT copies of each other (both are verified, as above).
 * After the call's single replay tail a copy is answered from its leader's FINAL answer:
 *       leader 0, fresh or replayed                                   -> status 0, out_replayed[i] = 1, out_key[i] = out_key[j] and the
 *                                                                        leader's output record byte for byte (128 bytes; wire form:
 *                                                                        the framed Refund message)
 *       leader 255 / 6 / 7, ACT_STATUS_DOUBLE_SPEND,
 *       ACT_STATUS_NULLIFIER_UNDETERMINED, ACT_STATUS_RECORDED_UNSIGNED -> the same status, out_key[i] = out_key[j], an all-zero record,
 *                                                                        out_replayed[i] = 0
 * What stays the same: every status, every out_key, every output byte, every out_replayed byte and the keys and epochs both sets hold
 * afterwards are byte for byte those of act_redeem_(cbor_)admit_replay_batch on the same batch and identical sets.  Why: there a later
 * copy of a fresh leader finds k spent by an earlier lane of the batch and its own tag in `receipts`, so it is a replay; nonce_i depends
 * only on nonce_key, the signing key, k and enc(K'), so it is signed into the same refund.  A copy of a rejected lane has the same
 * verdict by definition; a copy of a lane that lost k to another proof has the same tag and loses too.  (Not promised where lanes end
 * ACT_STATUS_NULLIFIER_UNDETERMINED: a set too small for the batch.)
 * What differs: only out_counts.  ACT_ADMIT_REPLAY_UNIQUE_COUNTS values: the eleven above, then copies, then copies_served (the copies
 * whose leader ended 0).  verified = lanes - wire_rejected - wrong_charge - foreign_spend - copies; rejected_by_verification, fresh,
 * replayed, double_spend_after and unanswered count VERIFIED lanes only.
 * Equality is decided on the bytes themselves, as in the admission unique forms.  Whole-call refusals, locks, failure semantics (a copy
 * of an ACT_STATUS_RECORDED_UNSIGNED leader says the same and is repaired by the same retry) and the hygiene contract are those of the
 * two calls above; nothing staged by the new step is secret (refunds are output).  Output rows may start at any byte address.  A batch
 * without copies in which nothing is shed still goes straight to the replay implementation with the caller's pointers; a batch in
 * which nothing survives still launches no verification kernel. */
#define ACT_ADMIT_REPLAY_UNIQUE_COUNTS 13
int act_redeem_admit_replay_unique_batch(act_ctx *ctx, act_nullifier_set *set, act_nullifier_set *receipts, size_t n, int mem, const uint8_t *keys, int nkeys,
                                         const uint32_t *key_epochs /* nullable */, int sign_key, const uint8_t *proof, const uint8_t *charge /* nullable */,
                                         const uint8_t nonce_key[32], uint8_t *out_refund, uint8_t *status, uint8_t *out_key,
                                         uint8_t *out_replayed /* nullable */, uint64_t *out_counts /* nullable, host */);
int act_redeem_cbor_admit_replay_unique_batch(act_ctx *ctx, act_nullifier_set *set, act_nullifier_set *receipts, size_t n, int mem, const uint8_t *keys, int nkeys,
                                              const uint32_t *key_epochs /* nullable */, int sign_key, const uint8_t *cbor, const uint64_t *offsets,
                                              const uint8_t *charge /* nullable */, const uint8_t nonce_key[32], uint8_t *out_refund_cbor, uint8_t *status,
                                              uint8_t *out_key, uint8_t *out_replayed /* nullable */, uint64_t *out_counts /* nullable, host */);

/* ======== row d and test infrastructure: debug hooks, measurement knobs, kernel timing, roofline probes (nothing here is on the product's path) ==== */
/* Debug / test hook: the exact "spend" transcript pre-images of the last act_verify_spend_batch /
 * act_refund_batch chunk (n_last * act_spend_transcript_bytes, copied to host memory). */
int act_debug_last_spend_transcripts(act_ctx *ctx, size_t max_lanes, uint8_t *out, size_t *n_copied);

/* Debug / test hook: number of non-zero bytes left in the context's secret-bearing device buffers -- the staging copies of
 * host inputs (tokens, PreIssuance, rng), the signer's nonces, the prover's r3 / r* / k* terms and the per-proof Pippenger
 * buckets -- all of which every entry point clears before it returns (the crate's ZeroizeOnDrop, src/lib.rs:160,362,393). */
int act_debug_secret_residue(act_ctx *ctx, size_t *nonzero_bytes);
/* Debug / test hook: every batch call on this context additionally sleeps ns_per_lane nanoseconds per lane while it holds the
 * context: a GPU that is slower than its neighbours, for the load-balance tests of the node dispatcher.  0 = off. */
int act_debug_set_slowdown(act_ctx *ctx, uint32_t ns_per_lane);
/* Debug / test hook: the signature step of the next `count` act_redeem_batch / act_redeem_cbor_batch calls on this context fails after
 * the nullifiers have been recorded (the failure ACT_STATUS_RECORDED_UNSIGNED exists for; no input can provoke it). */
int act_debug_fail_next_signs(act_ctx *ctx, int count);
/* Debug / test hook: the leader table of the unique admission forms alone, on the device, over m fingerprints the caller makes up
 * (HOST memory, none of them 0): out_leader[j] = the smallest index that carries fp[j].  out_ms (nullable): the time of the table's
 * two launches -- every lane on one slot is the contention case. */
int act_debug_copy_leaders(act_ctx *ctx, size_t m, const uint64_t *fp, uint32_t *out_leader, double *out_ms);
/* Debug / test hook: out[i] = enc(scalars[i] * points[i]) (`RistrettoPoint * Scalar`, e.g. src/lib.rs:791) computed by the
 * engine's production variable-base chain, decode and encode; status[i] = 255 and a zero record when points[i] is not a
 * canonical encoding.  Exists so that third-party known answers can be replayed on the device one operation at a time
 * (tests/golden/sodium_primitives.json). */
int act_debug_scalarmult_batch(act_ctx *ctx, size_t n, int mem, const uint8_t *points, const uint8_t *scalars, uint8_t *out,
                               uint8_t *status);
/* Debug / test hook: out[i] = enc(scalars[i] * B) for the fixed base B = `base` 0..3 (g, h1, h2, h3) (`&table * &scalar`, e.g.
 * src/lib.rs:224-228), computed by the engine's production fixed-base product on the table and window width the context holds for
 * that base at the time of the call (act_ctx_set_fixed_base_bits), and the production encode.  Scalars are 32 bytes each and are
 * reduced mod l on load.  Exists so that every window and entry of a table of any width can be aimed at with a chosen scalar.
 * ACT_ERR_ARG for a base outside 0..3. */
int act_debug_fixed_base_batch(act_ctx *ctx, int base, size_t n, int mem, const uint8_t *scalars, uint8_t *out);
/* Debug / test hook: ONE operation of the device's field arithmetic (csrc/fe25519.h) per lane, on raw limbs.  An element is nine
 * uint32_t limbs (limb i at bit ceil(85 i / 3)), lane i's at [9 i, 9 i + 9); nothing is reduced or checked on the way in or out, so
 * operands may sit anywhere in their limb-size class.  op: 0 h = f * g, 1 h = f^2, 2 h = f * g and hb = fb * gb_or_a, 3 h = f^2 and
 * hb = fb^2, 4 fe_sqda_sq: h = 2 f^2 + gb_or_a carried once and hb = fb^2, 5 h = fe_carry(f), 6 / 7 / 8 h = f - g + 2p / 3p / 4p
 * (fe_sub, fe_sub3, fe_sub4: g at most the offset limb-wise), 9 h = 2p - f (fe_neg).  pair_build 0 runs the per-column form of the
 * products that every kernel but one is built with, 1 the one-statement form of the range kernel's translation unit.  An array an
 * operation does not name may be NULL.  HOST memory only.  h (and hb, where written) must hold n rounded up to a multiple of 256
 * lanes: the lanes from n on make the round trip through device memory and come back as the caller filled them.  ACT_ERR_ARG for an
 * op outside 0..9 or a missing array. */
int act_debug_fe_batch(act_ctx *ctx, int pair_build, int op, size_t n, const uint32_t *f, const uint32_t *g, const uint32_t *fb,
                       const uint32_t *gb_or_a, uint32_t *h, uint32_t *hb);
/* Debug / test hook: ONE operation of the device's scalar arithmetic mod l (csrc/sc25519.h) per lane.  Lane i owns a record of 16
 * uint32_t words, [16 i, 16 i + 16), in every array the operation names.  op: 0 r = from_bytes_mod_order of the 32 BYTES at the start
 * of a's record and 1 r = from_bytes_mod_order_wide of its 64 bytes, both through the production loads and store; on raw 8-word
 * operands, which nothing reduces on the way in: 2 r = a + b, 3 r = a - b, 4 r = -a, 5 r = a / 2, 6 r = a b, 7 r = a b + c,
 * 8 r = 1 / a (0 for 0); 9 the Montgomery product inside the inversion on raw operands of ten 26-bit limbs, ten limbs out; 10 / 11
 * word 0 of r = 1 if a = b / a = 0 as words, else 0.  An array an operation does not name may be NULL.  HOST memory only.  r must
 * hold n rounded up to a multiple of 256 records: every word the operation does not write, in the records from n on too, makes the
 * round trip through device memory and comes back as the caller filled it.  ACT_ERR_ARG for an op outside 0..11 or a missing array. */
int act_debug_sc_batch(act_ctx *ctx, int op, size_t n, const uint32_t *a, const uint32_t *b, const uint32_t *c, uint32_t *r);
/* Debug / test hook: out[i] = enc(scalars[i] * B) for the fixed base B = 0..3 (g, h1, h2, h3) through the product every SECRET scalar
 * takes in the default build: 37 signed 7-bit digits, entry |digit| of a 64-entry window picked on the matrix cores from this context's
 * table image of B.  One product per lane, in blocks of block_threads = 64 or 256 threads (both shapes exist in the library), chunked
 * by the context's max_batch: with max_batch a multiple of 64, scalar i runs in lane i mod 64 of its wavefront.  32-byte scalars,
 * reduced mod l on load.  ACT_ERR_ARG for a base outside 0..3 or any other block_threads. */
int act_debug_fixed_base_mf_batch(act_ctx *ctx, int base, int block_threads, size_t n, int mem, const uint8_t *scalars, uint8_t *out);
/* Debug / test hook: the address-free variable-base chains of secret scalars, one per lane.  mode 0: out[i] = enc(scalars[i] *
 * points[i]) by the one-scalar chain; mode 1: the same product as the sum of its four 64-bit quarters (the single-item calls' form);
 * mode 2: out[i] as in mode 0 and out2[i] = enc(scalars2[i] * points[i]), both on one doubling chain.  scalars2 and out2 may be NULL
 * in modes 0 and 1.  status[i] = 0, or 255 with zero records where points[i] does not decode.  ACT_ERR_ARG for any other mode. */
int act_debug_chain_ct_batch(act_ctx *ctx, int mode, size_t n, int mem, const uint8_t *points, const uint8_t *scalars,
                             const uint8_t *scalars2, uint8_t *out, uint8_t *out2, uint8_t *status);

/* Measurement hook: A/B switches and size overrides of tools/ and tests/ (csrc/kernels.h TuneKey: "no_mapped_reads", "no_fused_tiny",
 * "no_taper", "no_wide_sign", "no_wide_prove", "no_wide_client", "no_lds_isolation", "no_stream_probe", "small_sub", "small_in_flight",
 * "small_normal_prio", "small_trace", "stagger", "host_chunk", "cbor_chunk_msgs", "ubench_iters").  Process-wide; none of them changes a
 * byte of any result.  A deployment never calls this; the library reads no environment variable in its place. */
int act_tuning_set(const char *name, int64_t value);

/* Kernel timing (HIP events on the context's own stream, which torch.cuda.Event cannot see):
 * enable, run batches, then read per-kernel totals.  names: act_prof_kernel_name(i), i < act_prof_kernel_count(). */
int act_prof_enable(act_ctx *ctx, int on);
int act_prof_reset(act_ctx *ctx);
int act_prof_kernel_count(const act_ctx *ctx);
const char *act_prof_kernel_name(const act_ctx *ctx, int i);
int act_prof_get(act_ctx *ctx, int i, double *ms_total, uint64_t *launches, uint64_t *lanes);
/* ms during which at least one launch of kernel i was executing (union of the launch intervals; launches of two chunks
 * in flight overlap, so ms_total of act_prof_get can exceed the wall time) */
int act_prof_get_busy(act_ctx *ctx, int i, double *ms_busy);
/* ALU roofline probe: rate of the 64-bit multiply-accumulate (v_mad_u64_u32) the field arithmetic is made of, with every
 * SIMD of `device` saturated by register-resident dependency chains.  lane_mads_per_s is summed over lanes; ms = probe time. */
int act_ubench_mad_u64_u32(int device, double *lane_mads_per_s, double *ms);
/* Memory-side roofline probe of the scalar-addressed fixed-base tables: every lane reads pseudo-random 128-byte lines (seven 16-byte
 * loads each, as an affine-Niels table entry is read) of a `gib` GiB buffer (0 = 16) allocated for the probe, `in_flight` (1, 2 or 4;
 * 0 = 2) entries at a time, with `waves_per_simd` (0 = 2, the occupancy of the kernels that do these look-ups) wavefronts per SIMD.
 * gbytes_per_s counts 128 bytes per read. */
int act_ubench_random_read(int device, size_t gib, int waves_per_simd, int in_flight, double *gbytes_per_s, double *ms);
/* The same probe over the context's own fixed-base table of base 0..3 (g, h1, h2, h3; the largest power-of-two prefix of it): the
 * product's look-ups in the product's memory with nothing else running. */
int act_ubench_table_read(act_ctx *ctx, int base, int waves_per_simd, int in_flight, double *gbytes_per_s, double *ms);

/* ======== partial refunds: the issuer returns t <= s unused credits with the Refund ========
 * Every redeem call above charges a token exactly s credits: refund signs X_A = g + K', and K' = sum 2^j Com_j commits to c - s.  A
 * metered service reserves s, does the work, and the work costs s - t.  These calls sign X_A = g + K' + t h1 instead; the client, who
 * reads t from the response, checks the same proof (label "refund", the same six transcript items: t is bound through X_A) over that
 * X_A and holds a token for c - s + t.  Both parties know t; like the amount c of an issuance it may address a table.
 *
 * RefundReturn record, 160 bytes: A | e | gamma | z | t.  The first 128 bytes are laid out as a Refund, t is a reduced scalar; a
 * rejected lane's record is all zero.  On the wire it is ACT_CBOR_REFUND_RETURN: the Refund map with a fifth entry, key 5 -> t.
 * returned: nullable (NULL = every t is 0); n scalars of 32 bytes in `mem` memory, laid out like SpendProof.s; reduced mod l on reading.
 *
 * act_refund_sign_return_keyring_batch is act_refund_sign_keyring_batch over X_A = g + K' + t h1 for the lanes with status_in == 0,
 * writing 160-byte records (nkeys == 1 is the one-key call).  IT DOES NOT SEE s: whoever calls it bounds t_i <= s_i, or signs a balance
 * the client never had.  (The client call below refuses such a record, but an issuer must not rely on its clients for its own books.)
 *
 * act_redeem_return_batch / act_redeem_cbor_return_batch are act_redeem_(cbor_)admit_batch with `returned`: the admission loop with one
 * more rule in step 2, checked in the screen's pass behind the charge and before any look-up:
 *       2b. t_i > s_i (both reduced mod l, compared as integers)  -> ACT_STATUS_RETURN_TOO_BIG: not looked up, not verified, not
 *           recorded, not signed; a zero record, ACT_KEY_NONE, no rng slice.  A lane that also has the wrong charge reports
 *           ACT_STATUS_WRONG_CHARGE, the earlier rule.
 * Every other lane goes through the redemption tail of the admission calls, whose signing step adds t h1, and gets a RefundReturn
 * record (wire form: an ACT_CBOR_REFUND_RETURN message of act_cbor_size bytes, all zero where not signed).
 * out_counts: nullable, host, ACT_REDEEM_RETURN_COUNTS values: the eight of ACT_ADMIT_COUNTS, then return_too_big; verified excludes
 * those lanes too.
 * With returned all zero (or NULL): statuses, out_key, the recorded nullifiers with their epochs, out_counts[0..8) and what is drawn
 * from the generator are byte for byte those of act_redeem_(cbor_)admit_batch on an identical set; the first 128 bytes of every record
 * equal that call's and bytes 128..160 are zero.
 *
 * act_refund_to_credit_token_return_batch is act_refund_to_credit_token_batch over n * 160 RefundReturn records: the proof over
 * X_A = g + K' + t h1 (ACT_STATUS_INVALID_REFUND_PROOF when it fails -- a record whose t was altered after signing fails it), then
 * t > s, s from the lane's proof record -> ACT_STATUS_AMOUNT_TOO_BIG (a balance above what the client had can never be proven in
 * range: better to learn it now), else the token A | e | k | r | (m + t) mod l.
 *
 * NOT OFFERED, on purpose: the replay forms of the sections above (act_redeem_(cbor_)replay_batch, act_redeem_(cbor_)admit_replay_batch
 * and their unique forms) take no `returned`.  They derive e and alpha from (nonce_key, key, k, enc(K')) alone, so a retry with another
 * t would be signed with the SAME e over an X_A that differs by (t1 - t2) h1: the two A values differ by (t1 - t2) (e + x)^-1 h1, which
 * hands out h1 (e + x)^-1 -- and with it anyone raises the balance of a token signed under that e.  The calls here use drawn nonces.
 * The replay form WITH amounts is a pair of calls of its own, act_redeem_(cbor_)return_replay_batch below ("replayable partial
 * refunds"), where t is bound into BOTH the receipt tag and the nonce derivation.  Also not offered here: the node-handle forms.
 * A service that learns t only from the work takes act_redeem_(cbor_)reserve_batch and act_redeem_(cbor_)settle_batch ("reserve and
 * settle", at the end of this file): the spend is recorded first and t is named when the refund is signed.
 *
 * act_refund_to_credit_token_return_keyring_batch is act_refund_to_credit_token_keyring_batch over n * 160 RefundReturn records: a
 * RefundReturn names no key either.  The same chunk schedule, staging and wiping of `pre`, ring checks (an entry that is not a canonical
 * encoding: ACT_ERR_ARG, nothing written), table cache and out_key contract -- the smallest ring index the item verifies under,
 * ACT_KEY_NONE where status != 0.  t h1 does not depend on the key: X_A = g + K' + t h1 is computed once, under ring key 0, and an extra
 * key costs what it costs a plain Refund.  The refusals in order: an undecodable point -> 255; no ring key's challenge equals gamma ->
 * ACT_STATUS_INVALID_REFUND_PROOF; a t > s that a ring key validly signed -> ACT_STATUS_AMOUNT_TOO_BIG; otherwise the token
 * A | e | k | r | (m + t) mod l.  A rejected lane's token is all zero.  No tiny or fused road, like every ring call.
 * With nkeys == 1: status and token bytes are those of act_refund_to_credit_token_return_batch, out_key is 0 where accepted.
 * With t == 0 in every record: status, token and out_key are those of act_refund_to_credit_token_keyring_batch on the first 128 bytes
 * of each record.
 *
 * act_redeem_return_unique_batch / act_redeem_cbor_return_unique_batch are the two return calls with step 3a of the admission unique
 * forms in its usual place, behind the screen and in front of verification.  The screen does not change (wire code, wrong charge,
 * t > s, spent before), and a lane shed by any of its rules is never a leader and never a copy.  Equality is decided on the proof bytes
 * alone (record or message): t takes no part in it.  What a lane that passed the screen is answered depends on its t only if it is the
 * lane that is signed, and that lane is the leader: in act_redeem_(cbor_)return_batch lanes that share a fresh nullifier are all
 * verified and the first valid one in lane order wins, whatever the others' t.  So a copy takes the answer of the admission unique
 * forms from its leader's final status -- ACT_STATUS_DOUBLE_SPEND behind a leader that ended 0 or ACT_STATUS_RECORDED_UNSIGNED, the
 * leader's own status otherwise -- a zero record and the leader's out_key, and draws no rng.
 * Statuses, out_key, output bytes, the recorded nullifiers with their epochs and the bytes drawn under all three rng conventions are
 * those of act_redeem_(cbor_)return_batch on an identical set, batches whose copies carry different t included; only the counts differ.
 * out_counts: nullable, host, ACT_REDEEM_RETURN_UNIQUE_COUNTS values: the eight of ACT_ADMIT_COUNTS, then return_too_big, then copies;
 * verified = lanes - wire_rejected - wrong_charge - return_too_big - spent_before - copies. */
#define ACT_STATUS_RETURN_TOO_BIG 249   /* t > s: not looked up, not verified, not recorded, not signed */
#define ACT_REDEEM_RETURN_COUNTS 9
#define ACT_REDEEM_RETURN_UNIQUE_COUNTS 10
int act_refund_sign_return_keyring_batch(act_ctx *ctx, size_t n, int mem, const uint8_t *keys, int nkeys, const uint8_t *key_index,
                                         const uint8_t *kprime, const uint8_t *status_in, const uint8_t *rng, int rng_mode,
                                         const uint8_t *returned /* nullable */, uint8_t *out_refund_return, uint8_t *status);
int act_redeem_return_batch(act_ctx *ctx, act_nullifier_set *set, size_t n, int mem, const uint8_t *keys, int nkeys,
                            const uint32_t *key_epochs /* nullable */, int sign_key, const uint8_t *proof, const uint8_t *charge /* nullable */,
                            const uint8_t *returned /* nullable */, const uint8_t *rng, int rng_mode, uint8_t *out_refund_return,
                            uint8_t *status, uint8_t *out_key, uint64_t *out_counts /* nullable, host */);
int act_redeem_cbor_return_batch(act_ctx *ctx, act_nullifier_set *set, size_t n, int mem, const uint8_t *keys, int nkeys,
                                 const uint32_t *key_epochs /* nullable */, int sign_key, const uint8_t *cbor, const uint64_t *offsets,
                                 const uint8_t *charge /* nullable */, const uint8_t *returned /* nullable */, const uint8_t *rng, int rng_mode,
                                 uint8_t *out_refund_return_cbor, uint8_t *status, uint8_t *out_key, uint64_t *out_counts /* nullable, host */);
int act_refund_to_credit_token_return_batch(act_ctx *ctx, size_t n, int mem, const uint8_t *prerefund, const uint8_t *proof,
                                            const uint8_t *refund_return, const uint8_t w[32], uint8_t *out_token, uint8_t *status);
int act_refund_to_credit_token_return_keyring_batch(act_ctx *ctx, size_t n, int mem, const uint8_t *prerefund, const uint8_t *proof,
                                                    const uint8_t *refund_return, const uint8_t *ring_w, uint32_t nkeys, uint8_t *out_token,
                                                    uint8_t *status, uint8_t *out_key);
int act_redeem_return_unique_batch(act_ctx *ctx, act_nullifier_set *set, size_t n, int mem, const uint8_t *keys, int nkeys,
                                   const uint32_t *key_epochs /* nullable */, int sign_key, const uint8_t *proof, const uint8_t *charge /* nullable */,
                                   const uint8_t *returned /* nullable */, const uint8_t *rng, int rng_mode, uint8_t *out_refund_return,
                                   uint8_t *status, uint8_t *out_key, uint64_t *out_counts /* nullable, host */);
int act_redeem_cbor_return_unique_batch(act_ctx *ctx, act_nullifier_set *set, size_t n, int mem, const uint8_t *keys, int nkeys,
                                        const uint32_t *key_epochs /* nullable */, int sign_key, const uint8_t *cbor, const uint64_t *offsets,
                                        const uint8_t *charge /* nullable */, const uint8_t *returned /* nullable */, const uint8_t *rng, int rng_mode,
                                        uint8_t *out_refund_return_cbor, uint8_t *status, uint8_t *out_key, uint64_t *out_counts /* nullable, host */);

/* ======== replayable partial refunds: the receipt pins t, the nonces take it ========
 * act_redeem_return_replay_batch / act_redeem_cbor_return_replay_batch are act_redeem_(cbor_)admit_replay_batch with `returned` (the
 * `amounts` argument of the prototypes below: n scalars in `mem` memory behind `charge`, nullable: all zero): a metered service that reserves s and gives t <= s back stays
 * retry-safe.  Write t^ = t mod l.  The outputs are RefundReturn records of 160 bytes (wire form: ACT_CBOR_REFUND_RETURN messages of
 * act_cbor_size bytes) ALWAYS, all zero where not signed.
 *
 * The two hashes of the replayable redemption with an amount:
 *       t^ == 0   the tag and the nonces are the v1 hashes above ("act-mi355x/receipt/v1", "act-mi355x/refund-nonce/v1"), bit for bit
 *       t^ != 0   tag   = BLAKE3("act-mi355x/receipt-t/v1" padded to 32 | k | enc(K') | t^)[0:32], top nibble cleared      (128 bytes)
 *                 nonce = BLAKE3-XOF("act-mi355x/refund-nonce-t/v1" padded to 32 | nonce_key | key | k | enc(K') | t^, 128)  (224 bytes)
 * t is public (it travels in the record), so which hash a lane takes is public too.  Under any history of the two sets, rollbacks from
 * snapshots included, two different t^ for one (key, k, K') never share an e.
 *
 * Per lane, in this order:
 *   1. the wire reader's code (wire form), 2. the charge (ACT_STATUS_WRONG_CHARGE) -- as act_redeem_(cbor_)admit_replay_batch.
 *   2b. t^ > s^ (both reduced mod l, compared as integers) -> ACT_STATUS_RETURN_TOO_BIG: behind the charge rule and in front of BOTH
 *       look-ups; not verified, not recorded, not signed, a zero record, ACT_KEY_NONE.  A lane that also has the wrong charge reports
 *       ACT_STATUS_WRONG_CHARGE.  A shed lane leaves no trace in either set.
 *   3. k is looked up.  A spent lane is a retry candidate only if `receipts` holds the tag of (k, enc(K'), t^): THE RECEIPT PINS THE
 *      AMOUNT.  A retry that names the t^ the spend was recorded with is verified and signed again, and its RefundReturn is byte for
 *      byte the one handed out before (out_replayed = 1).  A retry that names ANOTHER amount is ACT_STATUS_DOUBLE_SPEND, shed
 *      unverified (counted as foreign_spend, not in verified; zero record, ACT_KEY_NONE), and both sets stay as they were.
 *   4. verification, then the replay tail over the lanes that are left: check-and-insert of k; a receipt (k, enc(K'), t^) ONLY where
 *      k was fresh; the others are looked up -- found: replayed, else ACT_STATUS_DOUBLE_SPEND (so inside one batch [P t1, P t1, P t2]
 *      ends 0 / 0 replayed / 3); the nonces of (nonce_key, key, k, enc(K'), t^); the signature over X_A = g + K' + t h1.
 * This is on purpose: a SpendProof is not bound to a request.  The pinned t^ is what keeps a client from replaying an expensive spend
 * beside a cheap request and collecting a larger refund.  THE CALLER'S CONTRACT: a service must derive t deterministically from the
 * request, or remember it -- a retry answered with another t is refused, not re-priced.
 *
 * With returned all zero (or NULL): statuses, out_key, out_replayed, both sets with their epochs, out_counts[0..11) and the first 128
 * bytes of every record are those of act_redeem_(cbor_)admit_replay_batch on identical sets, and bytes 128..160 are zero (wire form:
 * the type 10 framing of the same fields).  A spend recorded by act_redeem_(cbor_)(admit_)replay_batch is served here with t = 0, and
 * retried here with t != 0 it is a double spend; a spend recorded here with t != 0 is a double spend for the calls without amounts.
 *
 * out_counts: nullable, host, ACT_RETURN_REPLAY_COUNTS values: the eleven of ACT_ADMIT_REPLAY_COUNTS in their order, then
 * return_too_big; verified = lanes - wire_rejected - wrong_charge - return_too_big - foreign_spend.
 * Refused as a whole (nothing written, nothing recorded): everything act_redeem_(cbor_)admit_replay_batch refuses -- receipts == set,
 * a receipts set without room for n more keys, epoch tables that do not fit both sets, a bad ring.  The failure contract is that
 * call's: after ACT_STATUS_RECORDED_UNSIGNED a later retry with the same t is served.
 * The unique forms are act_redeem_(cbor_)return_replay_unique_batch below ("replayable partial refunds, unique forms"): a copy that
 * names another t than its leader is not served the leader's row, it is refused.  Still not offered: node-handle forms; tiny or fused
 * roads; a `returned` argument on the screenless act_redeem_(cbor_)replay_batch -- the bound t <= s lives in the screen.  A service
 * that cannot know t when the spend is recorded: act_redeem_(cbor_)reserve_batch / act_redeem_(cbor_)settle_batch ("reserve and settle").
 *
 * act_replay_derive_return_batch is act_replay_derive_batch plus `returned` (nullable: that call): the tags and nonces above for
 * callers that compose the feature over the node-level calls with act_refund_sign_return_keyring_batch -- which is how it reaches
 * several GPUs.  A lane that does not take part (status_in != 0, key_index >= nkeys) gets zeros and its amount is not read. */
#define ACT_RETURN_REPLAY_COUNTS 12
int act_redeem_return_replay_batch(act_ctx *ctx, act_nullifier_set *set, act_nullifier_set *receipts, size_t n, int mem, const uint8_t *keys, int nkeys,
                                   const uint32_t *key_epochs /* nullable */, int sign_key, const uint8_t *proof, const uint8_t *charge /* nullable */,
                                   const uint8_t *amounts /* t; nullable: all zero */, const uint8_t nonce_key[32], uint8_t *out_refund_return,
                                   uint8_t *status, uint8_t *out_key, uint8_t *out_replayed /* nullable */, uint64_t *out_counts /* nullable, host */);
int act_redeem_cbor_return_replay_batch(act_ctx *ctx, act_nullifier_set *set, act_nullifier_set *receipts, size_t n, int mem, const uint8_t *keys, int nkeys,
                                        const uint32_t *key_epochs /* nullable */, int sign_key, const uint8_t *cbor, const uint64_t *offsets,
                                        const uint8_t *charge /* nullable */, const uint8_t *amounts /* t; nullable: all zero */, const uint8_t nonce_key[32],
                                        uint8_t *out_refund_return_cbor, uint8_t *status, uint8_t *out_key, uint8_t *out_replayed /* nullable */,
                                        uint64_t *out_counts /* nullable, host */);
int act_replay_derive_return_batch(act_ctx *ctx, size_t n, int mem, const uint8_t *keys, int nkeys, const uint8_t *key_index,
                                   const uint8_t nonce_key[32], const uint8_t *nullifiers, size_t stride, const uint8_t *kprime,
                                   const uint8_t *status_in, const uint8_t *amounts /* t; nullable */, uint8_t *out_tags /* nullable */,
                                   uint8_t *out_nonces /* nullable */);

/* ======== replayable partial refunds, unique forms: a copy answers to its own t ========
 * act_redeem_return_replay_unique_batch / act_redeem_cbor_return_replay_unique_batch are the two return replay calls above with step
 * 3c of the admit-replay unique forms unchanged, behind the screen (wire code, charge, t^ > s^ -> 249, both look-ups with the tag of
 * (k, enc(K'), t^)) and in front of verification.  Equality is decided on the proof bytes ALONE, as in act_redeem_(cbor_)return_
 * unique_batch: a lane that repeats the bytes of an earlier lane that passed the screen is a copy and is not verified, whatever amount
 * it names.  A lane the screen sheds (t^ > s^ and a spent k whose receipt names another amount among the reasons) is neither a leader
 * nor a copy.  The amounts of the VERIFIED lanes follow their lanes into the tail; a copy's t never reaches a tag, a nonce or a
 * signature.  Behind the call's single replay tail a copy i with leader j is answered from the leader's FINAL status and from whether
 * t^_i == t^_j (both reduced mod l, so t and t + l are one amount):
 *       leader's final status                     t^_i == t^_j   the copy's answer
 *       0 (fresh or replayed)                     yes            status 0, out_replayed[i] = 1, the leader's RefundReturn byte for byte
 *                                                                (160 bytes; wire form: the framed ACT_CBOR_REFUND_RETURN message)
 *       0 or ACT_STATUS_RECORDED_UNSIGNED         no             ACT_STATUS_DOUBLE_SPEND, a zero record, out_replayed[i] = 0: the receipt
 *                                                                pins the leader's amount
 *       ACT_STATUS_RECORDED_UNSIGNED              yes            ACT_STATUS_RECORDED_UNSIGNED, a zero record, out_replayed[i] = 1 (k is
 *                                                                spent and the receipt is this lane's own: what the tail of the calls
 *                                                                above marks before its signing step fails); repaired by the same retry
 *       anything else (255 / 6 / 7, DOUBLE_SPEND,
 *       ACT_STATUS_NULLIFIER_UNDETERMINED)        either         the leader's status, a zero record, out_replayed[i] = 0
 * out_key[i] = out_key[j] in every row: the key the shared bytes verified under, ACT_KEY_NONE where they did not verify -- which is
 * what the calls above report for a verified lane that their tail refuses.
 * THE PROMISE: on any batch and identical pairs of sets every status, every out_key, every output byte, every out_replayed byte and the
 * keys and epochs both sets hold afterwards are byte for byte those of act_redeem_(cbor_)return_replay_batch; only the counts differ.
 * Why: there a later copy with the leader's t^ finds k spent and its own tag in `receipts` and is signed with the same derived nonces;
 * a later copy with another t^ finds k spent and no tag for its amount ([P t1, P t1, P t2] -> 0 / 0 replayed / 3 in both).
 * Not promised:
 *   - lanes that end ACT_STATUS_NULLIFIER_UNDETERMINED (a set too small for the batch), as in the other unique forms;
 *   - a `receipts` set that holds tags for TWO amounts of one (k, enc(K')) -- only rolling `set` back from a snapshot while keeping
 *     `receipts` produces that.  There the calls above serve a copy that names the second amount and these refuse it
 *     (ACT_STATUS_DOUBLE_SPEND): the conservative direction;
 *   - wire form only: a copy of a leader that ended ACT_STATUS_DOUBLE_SPEND BECAUSE OF ITS AMOUNT -- the leader is another spelling of
 *     a message an earlier lane of the batch was served for with t1, names t2 and loses; its byte-identical copy that names t1 takes
 *     the leader's status here and is replayed by the calls above.  Again the conservative direction; sent alone it is served.
 * With amounts NULL or all zero: the first 128 bytes of every record, statuses, out_key, both sets, out_counts[0..11), copies and
 * copies_served are those of act_redeem_(cbor_)admit_replay_unique_batch, and return_too_big and copies_other_amount are 0;
 * out_replayed differs in one place, the copy of an ACT_STATUS_RECORDED_UNSIGNED leader (1 here, as in the calls above; 0 there).
 * out_counts: nullable, host, ACT_RETURN_REPLAY_UNIQUE_COUNTS values: the twelve of ACT_RETURN_REPLAY_COUNTS in their order, then
 * copies, copies_served (the copies answered 0) and copies_other_amount (the copies whose t^ differs from their leader's, whatever they
 * were answered).  verified = lanes - wire_rejected - wrong_charge - return_too_big - foreign_spend - copies; the tail's five counts
 * are over VERIFIED lanes only.
 * Whole-call refusals, locks, failure semantics and the hygiene contract are those of the calls above; nothing the serve step reads is
 * secret (amounts, statuses and refunds are public).  Output rows may start at any byte address.  A batch without copies in which
 * nothing is shed still goes straight to the replay implementation with the caller's pointers.  Still not offered: node-handle forms,
 * tiny or fused roads. */
#define ACT_RETURN_REPLAY_UNIQUE_COUNTS 15
int act_redeem_return_replay_unique_batch(act_ctx *ctx, act_nullifier_set *set, act_nullifier_set *receipts, size_t n, int mem, const uint8_t *keys, int nkeys,
                                          const uint32_t *key_epochs /* nullable */, int sign_key, const uint8_t *proof, const uint8_t *charge /* nullable */,
                                          const uint8_t *amounts /* t; nullable: all zero */, const uint8_t nonce_key[32], uint8_t *out_refund_return,
                                          uint8_t *status, uint8_t *out_key, uint8_t *out_replayed /* nullable */, uint64_t *out_counts /* nullable, host */);
int act_redeem_cbor_return_replay_unique_batch(act_ctx *ctx, act_nullifier_set *set, act_nullifier_set *receipts, size_t n, int mem, const uint8_t *keys, int nkeys,
                                               const uint32_t *key_epochs /* nullable */, int sign_key, const uint8_t *cbor, const uint64_t *offsets,
                                               const uint8_t *charge /* nullable */, const uint8_t *amounts /* t; nullable: all zero */, const uint8_t nonce_key[32],
                                               uint8_t *out_refund_return_cbor, uint8_t *status, uint8_t *out_key, uint8_t *out_replayed /* nullable */,
                                               uint64_t *out_counts /* nullable, host */);

/* ======== reserve and settle: record a spend now, sign its partial refund later ========
 * "A metered service reserves s, does the work, and the work costs s - t" in that order.  Every call above that records a nullifier
 * also signs in the same call, so t must be known before the spend is recorded.  act_redeem_reserve_batch / act_redeem_cbor_reserve_
 * batch are act_redeem_(cbor_)admit_replay_batch WITHOUT the signature: they screen, verify, record k and hand back a reservation
 * record.  act_redeem_settle_batch / act_redeem_cbor_settle_batch take reservation records and amounts t <= s, check that the
 * reservation is in the receipts, PIN the amount and sign a RefundReturn with the derived nonces of the replayable partial refunds.
 * Settling one reservation with the same amount again gives the same bytes.
 *
 * Definitions.  Write k^ = k mod l, s^ = s mod l, t^ = t mod l; enc(K') is the encoding the verification computes.
 *   reservation record   96 bytes, public: k^ | enc(K') | s^.  A rejected lane's record is all zero.  The matched ring index is
 *                        out_key[i], as in every ring call; it is not part of the record (a service stores 97 bytes and, later, t).
 *   reservation tag      tag_res = BLAKE3("act-mi355x/reservation/v1" padded to 32 | k^ | enc(K') | s^)[0:32], top nibble cleared
 *                        (128 bytes, two blocks).  s^ is in the tag so that settle's bound t <= s rests on what was reserved, not on
 *                        what the caller kept.
 *   settlement marker    BLAKE3("act-mi355x/settled/v1" padded to 32 | k^ | enc(K'))[0:32], top nibble cleared (96 bytes).
 *   amount tag, nonces   exactly act_replay_derive_return_batch's tag and nonces for (nonce_key, key_j, k^, enc(K'), t^), key_j the
 *                        key the lane is signed with: the v1 hashes at t^ = 0, the "-t" hashes otherwise.
 *
 * RESERVE, per lane and in this order (no sign_key, no nonce_key, no rng: nothing secret beyond the ring is staged):
 *   1. the wire reader's code (wire form) and the charge (ACT_STATUS_WRONG_CHARGE): as act_redeem_(cbor_)admit_replay_batch.
 *   2. k is already in `set`: enc(K') from the lane's Com_j, tag_res with the lane's s^, looked up in `receipts` (read only).  A lane
 *      with an undecodable Com_j or an absent tag is ACT_STATUS_DOUBLE_SPEND: not verified, ACT_KEY_NONE, a zero record.  A lane whose
 *      tag is there is a retry candidate.
 *   3. every remaining lane is verified against the ring.
 *   4. k is checked and inserted under the matched key's epoch; tag_res is recorded in `receipts` under the same epoch ONLY where k was
 *      fresh; where k was spent tag_res is looked up -- found: status 0 and out_replayed = 1, absent: ACT_STATUS_DOUBLE_SPEND.
 *   5. accepted lanes, fresh or replayed, get their record.  A retry gets the bytes of the first time: the record is a function of the proof.
 * What out_replayed = 1 obliges the service to do: the spend was reserved before -- look the job up by k^, never start a second one.
 * Failure contract: the replay calls' without its signature half.  ACT_STATUS_NULLIFIER_UNDETERMINED exists (also behind a device
 * failure of the last step: the same call again is then served as a retry); ACT_STATUS_RECORDED_UNSIGNED cannot occur.  A receipts
 * failure behind a recorded k returns the receipts set's error with status[] complete.  Whole-call refusals and locks are those of
 * act_redeem_(cbor_)admit_replay_batch (receipts == set, a receipts set without room for n more keys, epoch tables, a bad ring); one
 * call runs at a time per context.  out_counts: nullable, host, ACT_RESERVE_COUNTS values -- the eleven of ACT_ADMIT_REPLAY_COUNTS
 * in their order.
 *
 * SETTLE, per lane and in this order (key_index[i] is what reserve wrote to out_key[i]):
 *   1. key_index[i] >= nkeys -> ACT_STATUS_NOT_RESERVED; nothing is touched.
 *   2. t^ > s^ as integers, s^ from the record -> ACT_STATUS_RETURN_TOO_BIG: in front of every look-up, no trace.
 *   3. tag_res(k^, enc(K'), s^) is not in `receipts` (read only) -> ACT_STATUS_NOT_RESERVED: a record the caller altered, a spend
 *      recorded by any one-phase call, an epoch that was retired.
 *   4. THE PIN: the marker is checked and inserted into `receipts` under key_epochs[key_index[i]].  Fresh: the amount tag is recorded
 *      under the same epoch, out_settled_before = 0.  Spent before the call or by an earlier lane of the batch: the amount tag is
 *      looked up -- found: status 0, out_settled_before = 1 and the same bytes as before; absent: ACT_STATUS_SETTLED_OTHER_AMOUNT and a
 *      zero record.  So [R t1, R t1, R t2] ends 0 / 0 (settled before) / 247.
 *   5. the nonces of (nonce_key, key_j, k^, enc(K'), t^) and the signature over X_A = g + K' + t h1, by the ring signing step with
 *      amounts; key_j = sign_key, or key_index[i] for ACT_SIGN_MATCHED.  160-byte RefundReturn records (wire form: ACT_CBOR_REFUND_RETURN
 *      messages), all zero where not signed.
 * Why the pin: a SpendProof is not bound to a request.  A client can resend an expensive spend beside a cheap request; reserve answers
 * out_replayed = 1, and a service that nevertheless starts a second job and settles it with a larger t is stopped at the second
 * settlement.  t is in the nonces, so two amounts never share an e whatever the sets' history.
 * Failure contract: marker and amount tag are written before signing.  A failed signature step leaves ACT_STATUS_RECORDED_UNSIGNED;
 * the repair is the same call again with the same amounts.  A lane the receipts could not answer for is
 * ACT_STATUS_NULLIFIER_UNDETERMINED (nothing recorded for it: resubmit).
 * Refused as a whole (nothing written, nothing recorded): a NULL receipts handle or nonce_key, receipts with len + 2 n > slots / 2,
 * an epoch table that does not fit the receipts, a bad ring.
 * Races: two settlements of ONE reservation that race may see ACT_STATUS_SETTLED_OTHER_AMOUNT once -- the marker is recorded and the
 * amount tag not yet -- as two racing retries of one spend may see one ACT_STATUS_DOUBLE_SPEND in the replay calls; the same call
 * again is served.
 * out_counts: nullable, host, ACT_SETTLE_COUNTS values: lanes, not_reserved, return_too_big, settled, settled_again, other_amount,
 * unanswered (ACT_STATUS_NULLIFIER_UNDETERMINED and ACT_STATUS_RECORDED_UNSIGNED).
 * Hygiene: nonce_key, the ring and the derived nonces live in the context's replay buffer and are wiped on every exit;
 * act_debug_secret_residue stays 0.
 *
 * What follows from the definitions:
 *   - Settle equals the one-phase call.  After reserve and settle with t every output byte, status, out_key and the contents of `set`
 *     with their epochs are those of act_redeem_(cbor_)return_replay_batch on the same batch and amounts (identical empty sets;
 *     ACT_SIGN_MATCHED or the same sign_key).  Only the receipts differ: tag_res, the marker and the amount tag instead of the
 *     amount tag alone.  Two kinds of lane are answered under another name or leave more behind: a lane reserve shed (wrong charge, wire
 *     code) has no reservation, so settling its zero record with ACT_KEY_NONE is ACT_STATUS_NOT_RESERVED; and a lane with t^ > s^ is
 *     ACT_STATUS_RETURN_TOO_BIG on both roads, but reserve, which never sees t, HAS recorded its k -- the reservation stays open until it
 *     is settled with an amount that fits, and then the sets agree again.
 *   - A later client retry is served by the one-phase call: after settlement `receipts` holds the amount tag (k, K', t^), so
 *     act_redeem_(cbor_)return_replay_batch with that t serves the same RefundReturn (out_replayed = 1); with another t it is a
 *     double spend.
 *   - Unsettled reservations are closed to the one-phase calls: for every other redeem call such a spend is a foreign spend,
 *     ACT_STATUS_DOUBLE_SPEND, shed by the screen where there is one.
 *   - t = s cancels a reservation: the client gets its whole balance back.
 *   - Retire an epoch on both sets, as before: all three new keys carry the matched key's epoch.
 * Not offered: unique forms, node-handle forms, tiny or fused roads, a listing of unsettled reservations, a wire type for the
 * reservation record (it never goes to a client). */
#define ACT_STATUS_NOT_RESERVED 248           /* settle: no such reservation in the receipts (or key_index >= nkeys); nothing recorded, nothing signed */
#define ACT_STATUS_SETTLED_OTHER_AMOUNT 247   /* settle: the reservation was settled with another amount; nothing recorded, nothing signed */
#define ACT_RESERVE_COUNTS 11
#define ACT_SETTLE_COUNTS 7
int act_redeem_reserve_batch(act_ctx *ctx, act_nullifier_set *set, act_nullifier_set *receipts, size_t n, int mem, const uint8_t *keys, int nkeys,
                             const uint32_t *key_epochs /* nullable */, const uint8_t *proof, const uint8_t *charge /* nullable */,
                             uint8_t *out_reservation, uint8_t *status, uint8_t *out_key, uint8_t *out_replayed /* nullable */,
                             uint64_t *out_counts /* nullable, host */);
int act_redeem_cbor_reserve_batch(act_ctx *ctx, act_nullifier_set *set, act_nullifier_set *receipts, size_t n, int mem, const uint8_t *keys, int nkeys,
                                  const uint32_t *key_epochs /* nullable */, const uint8_t *cbor, const uint64_t *offsets,
                                  const uint8_t *charge /* nullable */, uint8_t *out_reservation, uint8_t *status, uint8_t *out_key,
                                  uint8_t *out_replayed /* nullable */, uint64_t *out_counts /* nullable, host */);
int act_redeem_settle_batch(act_ctx *ctx, act_nullifier_set *receipts, size_t n, int mem, const uint8_t *keys, int nkeys,
                            const uint32_t *key_epochs /* nullable */, int sign_key, const uint8_t *reservation, const uint8_t *key_index,
                            const uint8_t *amounts /* t; nullable: all zero */, const uint8_t nonce_key[32], uint8_t *out_refund_return,
                            uint8_t *status, uint8_t *out_settled_before /* nullable */, uint64_t *out_counts /* nullable, host */);
int act_redeem_cbor_settle_batch(act_ctx *ctx, act_nullifier_set *receipts, size_t n, int mem, const uint8_t *keys, int nkeys,
                                 const uint32_t *key_epochs /* nullable */, int sign_key, const uint8_t *reservation, const uint8_t *key_index,
                                 const uint8_t *amounts /* t; nullable: all zero */, const uint8_t nonce_key[32], uint8_t *out_refund_return_cbor,
                                 uint8_t *status, uint8_t *out_settled_before /* nullable */, uint64_t *out_counts /* nullable, host */);

/* ======== request binding: 32 caller bytes enter the spend challenge ========
 * A SpendProof is a bearer instrument: nothing in it says which request it pays for, so whoever sees it before the issuer does can
 * present it beside a request of their own.  The calls below take associated data for the proof's Fiat-Shamir challenge: `bind`, n * 32
 * bytes in `mem` memory beside the proofs, typically a hash of the request.  The library hashes nothing for the caller, and the binding
 * is never sent inside the proof: both sides derive it from the request.
 * The construction: the "spend" transcript followed by one more Transcript::update(bind_i) -- the 8-byte big-endian length 00..20 and
 * the 32 bytes, appended behind the last existing element C -- hashed and reduced as before.  The unbound pre-image is a strict prefix
 * of the bound one and no element moves; an unbound L-bit transcript has 6 + 3 L items and a bound one 7 + 3 L, so the two never
 * coincide.  An all-zero binding is a binding: such a proof is not an unbound proof.
 * A BOUND PROOF IS NOT A CRATE SpendProof: the crate's PrivateKey::refund rejects it, as every unbound call here does.  It has the
 * record layout, size and CBOR type of a SpendProof.
 * bind == NULL makes each call below the call it extends, byte for byte.  Each has the signature of that call with `bind` directly
 * behind the proof or message arguments.  A lane whose binding is not the one its proof was made with gets the status a tampered
 * proof gets (7, or the ring call's ACT_KEY_NONE): nothing is recorded, signed or reserved for it.
 * What the binding does not enter: the screen, the retry-candidate stage, the receipt tags, the derived nonces and both sets.  The
 * same proof served again under the same binding gives the same refund bytes with out_replayed = 1; under another binding it is an
 * invalid proof and both sets stay as they are.  For reserve this closes what "Why the pin" describes above: a recorded reservation's
 * proof resent beside another request no longer answers out_replayed = 1.  Settle takes no binding: it never sees a proof.
 * Not offered: node-handle forms, unique forms (ACT_ERR_ARG; equal proof bytes say nothing about two lanes' bindings), the one-key
 * calls with their small-batch and tiny roads (a ring of one key is the bound one-key call), act_prove_spend_seeded_batch, a wire
 * field.  act_debug_last_spend_transcripts reports unbound pre-images and is meaningful after an unbound call only. */
int act_prove_spend_bound_batch(act_ctx *ctx, size_t n, int mem, const uint8_t *token, const uint8_t *s, const uint8_t *rng,
                                const uint8_t *bind /* n*32; nullable */, uint8_t *out_proof, uint8_t *out_prerefund, uint8_t *status);
int act_verify_spend_keyring_bound_batch(act_ctx *ctx, size_t n, int mem, const uint8_t *keys, int nkeys, const uint8_t *proof,
                                         const uint8_t *bind /* n*32; nullable */, uint8_t *status, uint8_t *out_key, uint8_t *out_kprime /* nullable */);
int act_redeem_return_replay_bound_batch(act_ctx *ctx, act_nullifier_set *set, act_nullifier_set *receipts, size_t n, int mem, const uint8_t *keys, int nkeys,
                                         const uint32_t *key_epochs /* nullable */, int sign_key, const uint8_t *proof, const uint8_t *bind /* n*32; nullable */,
                                         const uint8_t *charge /* nullable */, const uint8_t *amounts /* t; nullable: all zero */, const uint8_t nonce_key[32],
                                         uint8_t *out_refund_return, uint8_t *status, uint8_t *out_key, uint8_t *out_replayed /* nullable */,
                                         uint64_t *out_counts /* nullable, host */);
int act_redeem_cbor_return_replay_bound_batch(act_ctx *ctx, act_nullifier_set *set, act_nullifier_set *receipts, size_t n, int mem, const uint8_t *keys, int nkeys,
                                              const uint32_t *key_epochs /* nullable */, int sign_key, const uint8_t *cbor, const uint64_t *offsets,
                                              const uint8_t *bind /* n*32; nullable */, const uint8_t *charge /* nullable */,
                                              const uint8_t *amounts /* t; nullable: all zero */, const uint8_t nonce_key[32], uint8_t *out_refund_return_cbor,
                                              uint8_t *status, uint8_t *out_key, uint8_t *out_replayed /* nullable */, uint64_t *out_counts /* nullable, host */);
int act_redeem_reserve_bound_batch(act_ctx *ctx, act_nullifier_set *set, act_nullifier_set *receipts, size_t n, int mem, const uint8_t *keys, int nkeys,
                                   const uint32_t *key_epochs /* nullable */, const uint8_t *proof, const uint8_t *bind /* n*32; nullable */,
                                   const uint8_t *charge /* nullable */, uint8_t *out_reservation, uint8_t *status, uint8_t *out_key,
                                   uint8_t *out_replayed /* nullable */, uint64_t *out_counts /* nullable, host */);
int act_redeem_cbor_reserve_bound_batch(act_ctx *ctx, act_nullifier_set *set, act_nullifier_set *receipts, size_t n, int mem, const uint8_t *keys, int nkeys,
                                        const uint32_t *key_epochs /* nullable */, const uint8_t *cbor, const uint64_t *offsets,
                                        const uint8_t *bind /* n*32; nullable */, const uint8_t *charge /* nullable */, uint8_t *out_reservation,
                                        uint8_t *status, uint8_t *out_key, uint8_t *out_replayed /* nullable */, uint64_t *out_counts /* nullable, host */);

#ifdef __cplusplus
}
#endif
#endif
