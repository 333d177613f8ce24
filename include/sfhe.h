/*
 * sfhe.h -- C ABI of the MI355X CKKS rank-sort engine (drop-in boundary).
 *
 * The reference (oksuman/sorting-fhe) is C++ calling OpenFHE 1.1.4; it has
 * no FFI of its own.  Its hot path is DirectSort<N>::sort and the lbcrypto
 * calls beneath it.  Every entry point below replaces
 * one of those reference interfaces (cited per function), with plain
 * pointers, sizes and int status codes so any FFI (ctypes, cgo, JNI, N-API)
 * can bind it.  C++ callers can instead use the lbcrypto-compatible headers
 * in sorting-fhe_amd/csrc/core and csrc/algo, which wrap the same engine.
 *
 * Conventions: functions return SFHE_OK (0) or a negative SFHE_E* code;
 * sfhe_last_error() gives the message (thread-local).  Objects returned
 * through out-pointers are owned by the caller and released with the
 * matching *_free / *_destroy.  A context and everything created from it
 * must be used from one thread at a time (calls are internally serialised).
 */
#ifndef SFHE_H
#define SFHE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SFHE_ABI_VERSION 3  /* bumped when a declaration or struct below changes */
/* (sfhe_decrypt_batch and sfhe_decode_counts were added at version 3: additions
 * only, no existing declaration changed, so the version stays; likewise
 * sfhe_encrypt_batch and sfhe_sample_counts, and sfhe_sorter_sort_stable,
 * sfhe_sorter_rank_stable and sfhe_tie_counts, and sfhe_const_term_counts, and
 * the record sort: SFHE_MAX_COLUMNS, sfhe_sorter_place_many,
 * sfhe_sorter_sort_records, sfhe_sorter_records_graph_nodes, sfhe_place_counts,
 * and the selection: sfhe_select_params, sfhe_sorter_select_ranked,
 * sfhe_sorter_select, sfhe_eval_rotate_fold, sfhe_select_counts, and the
 * record selection: sfhe_sorter_select_many, sfhe_sorter_select_records,
 * sfhe_eval_rotate_fold_many, sfhe_select_cols_counts, and the ordering by
 * several keys: SFHE_LEX_KEYS, sfhe_lex_sort_depth, sfhe_sorter_rank_lex,
 * sfhe_sorter_sort_records_lex, sfhe_sorter_select_records_lex,
 * sfhe_eval_lex_step, sfhe_lex_counts, and the sum of two products:
 * sfhe_eval_mult_sum2, sfhe_dot_counts, and the sum of n products:
 * sfhe_eval_mult_sum, sfhe_eval_mult_sum_many, sfhe_sumn_counts,
 * sfhe_sumn_batch_counts, sfhe_ct_relabel_scale, and the grouping by a key:
 * sfhe_group_params, sfhe_sorter_group, sfhe_eval_gate_sum_many,
 * sfhe_group_counts, and the window sums: SFHE_FRAME_*, sfhe_window_params,
 * sfhe_sorter_window, sfhe_eval_weight_sum_many, sfhe_window_counts, and the
 * join of two tables: sfhe_join_params, sfhe_sorter_join, sfhe_eval_gate_or,
 * sfhe_join_counts) */

#define SFHE_OK 0
#define SFHE_EINVAL (-1)   /* bad argument */
#define SFHE_ESCHEME (-2)  /* CKKS error: depth exhausted, missing key, ... */
#define SFHE_EDEVICE (-3)  /* device / backend failure */
#define SFHE_ENOTIMPL (-4) /* valid request, not implemented */

typedef struct sfhe_ctx sfhe_ctx;
typedef struct sfhe_ct sfhe_ct;
typedef struct sfhe_sorter sfhe_sorter;

/* Scaling techniques (lbcrypto::ScalingTechnique values).  FLEXIBLEAUTOEXT,
 * OpenFHE's default and therefore the reference's (it never calls
 * SetScalingTechnique), forms fresh encryptions modulo Q*q_ext and rescales
 * by q_ext; FLEXIBLEAUTO encrypts directly modulo Q. */
#define SFHE_FLEXIBLEAUTO 2
#define SFHE_FLEXIBLEAUTOEXT 3

/* Security levels (lbcrypto::SecurityLevel). */
#define SFHE_HESTD_128_CLASSIC 0
#define SFHE_HESTD_NOTSET 3

/* CCParams<CryptoContextCKKSRNS> (GenCryptoContext inputs; reference
 * tests/DirectSortTest.cpp:29-37, sort_algo.h:87-201). */
typedef struct {
    uint32_t mult_depth;
    uint32_t scaling_mod_size;  /* bits of the scaling primes (e.g. 40) */
    uint32_t first_mod_size;    /* bits of q_0 (default 60) */
    uint32_t batch_size;        /* default slot count; 0 = n/2 */
    uint32_t ring_dim;          /* 0 = smallest secure */
    int32_t security_level;     /* SFHE_HESTD_* */
    uint32_t num_large_digits;  /* HYBRID dnum; 0 = default (3) */
    int32_t device;             /* HIP device ordinal */
    uint64_t seed;              /* deterministic key / noise sampling */
    int32_t scaling_technique;  /* SFHE_FLEXIBLEAUTO[EXT]; 0 = FLEXIBLEAUTOEXT */
} sfhe_params;

int sfhe_abi_version(void);
const char* sfhe_last_error(void);
/* "hip-gfx950" for the product library. */
const char* sfhe_backend(void);
void sfhe_params_default(sfhe_params* p);

/* ---- context and keys ---------------------------------------------------
 * Replaces GenCryptoContext + Enable(...) + KeyGen + EvalMultKeyGen
 * (DirectSortTest.cpp:39-54) and EvalRotateKeyGen (:52). */
int sfhe_context_create(const sfhe_params* p, sfhe_ctx** out);
void sfhe_context_destroy(sfhe_ctx* c);
int sfhe_keygen(sfhe_ctx* c);
int sfhe_rotate_keygen(sfhe_ctx* c, const int32_t* idx, size_t count);
/* ring_dim, mult_depth, #Q primes, #P primes, dnum (any pointer may be NULL) */
int sfhe_context_info(sfhe_ctx* c, uint32_t* ring_dim, uint32_t* mult_depth, uint32_t* num_q,
                      uint32_t* num_p, uint32_t* dnum);
/* prime table [q_0..q_L, p_0..p_{K-1}] (+ q_ext under FLEXIBLEAUTOEXT) */
int sfhe_context_primes(sfhe_ctx* c, uint64_t* out, size_t cap, size_t* count);
/* Cache of encoded constant plaintexts (sort masks) across calls; default on. */
int sfhe_set_plaintext_cache(sfhe_ctx* c, int on);
/* Suppress the reference's stdout prints inside sort() (default off). */
int sfhe_set_quiet(sfhe_ctx* c, int quiet);
/* Block until queued device work is done; reports asynchronous errors. */
int sfhe_sync(sfhe_ctx* c);
/* counts[9]: keyswitch, rescale, tensor, ptmult, constmult, add, automorph,
 * ntt_limbs, wsum_terms; bytes: algorithmic HBM bytes (SURVEY §8(d) model). */
int sfhe_op_stats(sfhe_ctx* c, uint64_t* counts, double* bytes, int reset);
/* Bootstrap shapes (input level, iterations, precision) replayed from a
 * captured hipGraph so far (the first call of a shape runs eagerly, the
 * second is captured). */
int sfhe_bootstrap_graphs(sfhe_ctx* c, uint64_t* count);
/* Plaintext encodings done on the device (sfp_encode) and on the host since
 * the last sfhe_op_stats reset. */
int sfhe_encode_counts(sfhe_ctx* c, uint64_t* device, uint64_t* host);
/* Ciphertexts whose decryption was decoded on the device (sfp_decode_batch)
 * and on the host since the last sfhe_op_stats reset (SFHE_DEV_DECODE=0, read
 * per call, decodes on the host; the results are bit-identical). */
int sfhe_decode_counts(sfhe_ctx* c, uint64_t* device, uint64_t* host);
/* Tie terms of the stable rank (one per batch of sfhe_sorter_rank_stable)
 * whose tensor ran as one fused launch (sfp_tie_tensor) and as the composed
 * generic prims since the last sfhe_op_stats reset (SFHE_TIE_FUSED=0, read
 * per call, composes; the results are bit-identical). */
int sfhe_tie_counts(sfhe_ctx* c, uint64_t* fused, uint64_t* composed);
/* Constant terms c*x at a level (one-input weighted sums: the sign
 * polynomials' coefficient terms) since the last sfhe_op_stats reset: issued
 * inside a multi-term launch (sfp_const_terms_rescale), as one fused constant
 * rescale, and as a weighted sum followed by a rescale (SFHE_CONST_TERMS=0,
 * read per call, composes; the results are bit-identical). */
int sfhe_const_term_counts(sfhe_ctx* c, uint64_t* merged, uint64_t* single, uint64_t* composed);
/* since the last sfhe_op_stats reset: indicators evaluated for a multi-column placement, columns they
 * served, giant-step sums issued through sfp_mac_plain2_cols, and through the per-column path
 * (SFHE_PLACE_COLS=0, read per call, takes the per-column path; the results are bit-identical) */
int sfhe_place_counts(sfhe_ctx* c, uint64_t* hits, uint64_t* columns, uint64_t* fused, uint64_t* composed);
/* Since the last sfhe_op_stats reset: indicator batches the selections ran, and
 * sfhe_eval_rotate_fold calls (the selections' included) whose inner products
 * were one launch / were composed of the generic primitives. */
int sfhe_select_counts(sfhe_ctx* c, uint64_t* batches, uint64_t* fold_fused, uint64_t* fold_composed);
/* Since the last sfhe_op_stats reset: columns the multi-column selections
 * served, launches sfhe_eval_rotate_fold_many issued through
 * sfp_ks_inner_aut_sum_cols, and columns it passed to sfhe_eval_rotate_fold's
 * path (SFHE_SELECT_COLS=0, read per call, takes the latter; the results are
 * bit-identical). */
int sfhe_select_cols_counts(sfhe_ctx* c, uint64_t* columns, uint64_t* fused, uint64_t* composed);
/* Small polynomials (an encryption's v, e0, e1; the keys' errors and secret)
 * sampled on the device (sfp_sample_small) and on the host since the last
 * sfhe_op_stats reset (SFHE_DEV_SAMPLE=0, read per call, samples on the host;
 * the residues are identical). */
int sfhe_sample_counts(sfhe_ctx* c, uint64_t* device, uint64_t* host);
/* Device memory held by the context's buffer pool (live and free blocks). */
int sfhe_pool_bytes(sfhe_ctx* c, uint64_t* bytes);
/* Engine contexts alive in this process (diagnostics: after every
 * sfhe_context_destroy of a process's contexts it is back to 0). */
int sfhe_live_contexts(void);
/* Live kernel timing (bench roofline; no reference counterpart): kernel
 * families SFHE_KFAM_*; every `period`-th launch of the family is bracketed
 * by HIP events on the context's stream (period 0 = off; resets counters).
 * _read synchronises and returns launches seen, launches timed, their summed
 * duration (ms) and summed algorithmic bytes (prims.h defines the model). */
#define SFHE_KFAM_NTT 0
#define SFHE_KFAM_CONV 1
#define SFHE_KFAM_KSINNER 2
#define SFHE_KFAM_NTTKS 3   /* k_ntt_ks: ModUp's ROW pass fused with the key inner product */
#define SFHE_KFAM_OTHER 4   /* (graph timing only) every kernel of no family above */
#define SFHE_KFAM_ALL 5     /* (graph timing only) every kernel */
int sfhe_kernel_timing(sfhe_ctx* c, uint32_t family, uint32_t period);
int sfhe_kernel_timing_read(sfhe_ctx* c, uint32_t family, uint64_t* launches, uint64_t* timed,
                            double* ms, double* bytes);
/* on != 0: all of the context's lanes (streams) issue on one stream, so timed
 * launches run alone, as under rocprofv3 (bench profiling leg; slower). */
int sfhe_serialize_lanes(sfhe_ctx* c, int on);
/* Stacked launches so far (no reference counterpart; prims.h sfp_stack_*):
 * the sort's two batches issue their identical ops as one launch each --
 * `merged` such pairs, `single` launches issued alone inside stacked regions. */
int sfhe_stack_stats(sfhe_ctx* c, uint64_t* merged, uint64_t* single);
/* Collective statistics of a sharded context (no reference counterpart; the
 * reference has no distributed code): sfhe_comm_stats_reset zeroes them
 * (timed != 0: every eager collective is also timed with events on its
 * stream); sfhe_comm_stats returns the collectives this rank issued since,
 * the bytes it received through them and their summed duration in ms. */
int sfhe_comm_stats_reset(sfhe_ctx* c, int timed);
int sfhe_comm_stats(sfhe_ctx* c, uint64_t* calls, double* bytes, double* ms);

/* ---- encryption ------------------------------------------------------------
 * Replaces Encryption::encryptInput (encryption.cpp:5-12, MakeCKKSPacked-
 * Plaintext + Encrypt) and DebugEncryption::getPlaintext / Decrypt
 * (:14-33).  slots = 0 uses the batch size; level > 0 encrypts lower. */
int sfhe_encrypt(sfhe_ctx* c, const double* values, size_t len, uint32_t slots, uint32_t level,
                 sfhe_ct** out);
/* `count` inputs encrypted in one call: input k is the lens[k] values at
 * values + k * stride (lens[k] <= stride), packed into `slots` slots (0: the
 * batch size) at level levels[k] (levels NULL: level 0).  outs[k] equals what
 * sfhe_encrypt gives when called on each input in order. */
int sfhe_encrypt_batch(sfhe_ctx* c, const double* values, size_t stride, const size_t* lens, size_t count,
                       uint32_t slots, const uint32_t* levels, sfhe_ct** outs);
/* writes min(cap, slots) real parts; *len = slots */
int sfhe_decrypt(sfhe_ctx* c, const sfhe_ct* ct, double* out, size_t cap, size_t* len);
/* `count` ciphertexts (any mix of levels and slot counts) decrypted with one
 * device synchronisation: the real parts of ciphertext k go to out + k * stride
 * (at most `stride` values each), lens[k] = its slot count (lens may be NULL).
 * The values equal sfhe_decrypt's on each ciphertext. */
int sfhe_decrypt_batch(sfhe_ctx* c, const sfhe_ct* const* cts, size_t count, double* out, size_t stride,
                       size_t* lens);
void sfhe_ct_free(sfhe_ct* ct);
int sfhe_ct_clone(const sfhe_ct* ct, sfhe_ct** out);
/* Ciphertext::GetLevel / GetSlots / limb count */
int sfhe_ct_info(const sfhe_ct* ct, uint32_t* level, uint32_t* slots, uint32_t* limbs);
/* Ciphertext::SetSlots (metadata only) */
int sfhe_ct_set_slots(sfhe_ct* ct, uint32_t slots);
/* raw residues [c0 limbs][c1 limbs] (evaluation domain), 2*limbs*n words */
int sfhe_ct_download(sfhe_ctx* c, const sfhe_ct* ct, uint64_t* out, size_t cap_words);

/* ---- evaluation (CryptoContextImpl::Eval*, as called on the hot path) ---- */
int sfhe_eval_add(sfhe_ctx* c, const sfhe_ct* a, const sfhe_ct* b, sfhe_ct** out);
int sfhe_eval_sub(sfhe_ctx* c, const sfhe_ct* a, const sfhe_ct* b, sfhe_ct** out);
int sfhe_eval_add_const(sfhe_ctx* c, const sfhe_ct* a, double k, sfhe_ct** out);
int sfhe_eval_mult_const(sfhe_ctx* c, const sfhe_ct* a, double k, sfhe_ct** out);
/* EvalMult(ct, pt): pt = encode(values, slots) at a's level */
int sfhe_eval_mult_plain(sfhe_ctx* c, const sfhe_ct* a, const double* values, size_t len,
                         uint32_t slots, sfhe_ct** out);
/* EvalMultAndRelinearize / EvalMult(ct, ct) (sign.cpp:23-33) */
int sfhe_eval_mult(sfhe_ctx* c, const sfhe_ct* a, const sfhe_ct* b, sfhe_ct** out);
/* EvalRotate (rotation.h:224) */
int sfhe_eval_rotate(sfhe_ctx* c, const sfhe_ct* a, int32_t r, sfhe_ct** out);
/* sum_k EvalRotate(a[k], r[k]) with one shared ModDown (engine extension:
 * output aggregation of the giant steps of vecRotsOpt / blindRotationOptN,
 * src/sort_algo.h:342-364, 561-584, which sum individually rotated terms) */
int sfhe_eval_rotate_sum(sfhe_ctx* c, const sfhe_ct* const* a, const int32_t* r, size_t count, sfhe_ct** out);
/* sum_{k < count} EvalRotate(a, k * stride), 2 <= count <= 8 (engine extension,
 * no reference counterpart): the rotations of ONE ciphertext share its ModUp
 * and one ModDown, and on the device their key inner products are one launch
 * (SFHE_SELECT_FOLD=0, read per call: one permutation and one accumulating
 * inner product per term -- the same residues).  Term 0 is `a` itself; a term
 * whose amount is a multiple of a's slot count is added as it is; any other
 * amount needs its rotation key (SFHE_ESCHEME; the message names the amount).
 * count outside [2, 8]: SFHE_EINVAL. */
int sfhe_eval_rotate_fold(sfhe_ctx* c, const sfhe_ct* a, int32_t stride, uint32_t count, sfhe_ct** out);
/* outs[i] = sfhe_eval_rotate_fold(cts[i], stride, count), residue for residue,
 * for ncts >= 1 ciphertexts at one level and slot count (else SFHE_ESCHEME):
 * on the device the inner products of up to 16 of them are tiles of columns
 * that read each rotation-key word once (SFHE_SELECT_COLS=0, read per call,
 * or more than 16: sfhe_eval_rotate_fold per ciphertext).  ncts = 0, a NULL
 * entry, count outside [2, 8]: SFHE_EINVAL. */
int sfhe_eval_rotate_fold_many(sfhe_ctx* c, const sfhe_ct* const* cts, size_t ncts, int32_t stride, uint32_t count,
                               sfhe_ct** outs);
/* CKKS bootstrapping (OpenFHE's EvalBootstrapSetup + EvalBootstrapKeyGen and
 * EvalBootstrap, as src/k-way/EvalUtils.cpp:57-86 and src/sort_algo.h:1437
 * call them): setup for ciphertexts of `slots` slots with the level budget
 * {budget_c2s, budget_s2c} (and its rotation / conjugation keys); depth =
 * the level a bootstrapped ciphertext comes out at; iterations 2 with
 * precision p = meta-bootstrapping. */
int sfhe_bootstrap_setup(sfhe_ctx* c, uint32_t budget_c2s, uint32_t budget_s2c, uint32_t slots);
int sfhe_bootstrap_depth(sfhe_ctx* c, uint32_t budget_c2s, uint32_t budget_s2c, uint32_t slots, uint32_t* depth);
int sfhe_bootstrap(sfhe_ctx* c, const sfhe_ct* a, uint32_t iterations, uint32_t precision, sfhe_ct** out);
/* EvalChebyshevSeriesPS (sort_algo.h:727-728, sign.cpp:76); c0/2 convention */
int sfhe_eval_chebyshev(sfhe_ctx* c, const sfhe_ct* x, const double* coeffs, size_t count,
                        double a, double b, sfhe_ct** out);

/* ---- hot path ----------------------------------------------------------------
 * sign(x, cc, CompositeSign, SignConfig(CompositeSignConfig(n, dg, df)))
 * (sign.cpp:635-651; n in {3, 4}). */
int sfhe_sign(sfhe_ctx* c, const sfhe_ct* x, int n, int dg, int df, sfhe_ct** out);
/* Comparison::compare (comparison.cpp:4-22): (sign(a-b)+1)/2 */
int sfhe_compare(sfhe_ctx* c, const sfhe_ct* a, const sfhe_ct* b, int n, int dg, int df,
                 sfhe_ct** out);
/* DirectSort<N>::getSizeParameters (sort_algo.h:87-201): depth and rotation
 * keys: the reference table for N in {4, 8, ..., 2048} (sorters: N <= 1024). */
int sfhe_direct_sort_params(uint32_t N, uint32_t* mult_depth, int32_t* rotations, size_t cap,
                            size_t* count);
/* Doubled-sinc Chebyshev table (generated_doubled_sinc_coeffs.h). */
int sfhe_doubled_sinc_coeffs(uint32_t N, double* out, size_t cap, size_t* count);
/* DirectSort<N> construction (sort_algo.h:74-81; encrypts the zero cache).
 * debug != 0 uses DebugEncryption, so sort() runs the reference's three
 * PRINT_PT decrypts ("as-test" timing); 0 = plain Encryption ("pure"). */
int sfhe_sorter_create(sfhe_ctx* c, uint32_t N, int debug, sfhe_sorter** out);
/* The same with the rotation-key list the DirectSort<N> constructor receives
 * (sort_algo.h:74-81, its rotIndices argument: the amounts RotationComposer
 * uses as single steps); NULL / 0 = the getSizeParameters list.  The context
 * must hold keys for them (sfhe_keygen's rotation list). */
int sfhe_sorter_create_rot(sfhe_ctx* c, uint32_t N, int debug, const int32_t* rotations, size_t nrot,
                           sfhe_sorter** out);
void sfhe_sorter_destroy(sfhe_sorter* s);
/* DirectSort<N>::sort (sort_algo.h:752-774).  Sets the input's slots to
 * the partition size as the reference does (sort_algo.h:711). */
int sfhe_sorter_sort(sfhe_sorter* s, sfhe_ct* in, int n, int dg, int df, sfhe_ct** out);
/* DirectSort<N>::constructRank (sort_algo.h:368-506) */
int sfhe_sorter_rank(sfhe_sorter* s, const sfhe_ct* in, int n, int dg, int df, sfhe_ct** out);
/* DirectSort<N>::rotationIndexCheckN (sort_algo.h:658-750) */
int sfhe_sorter_place(sfhe_sorter* s, const sfhe_ct* rank, sfhe_ct* in, sfhe_ct** out);
/* Engine extensions (additions at ABI 3): the tie-aware stable rank sort.
 * sfhe_sorter_rank_stable gives #{j : x_j < x_r} + #{j < r : x_j = x_r}, so
 * inputs with duplicate values sort and equal values keep their input order
 * (place(rank_stable(keys), payload) orders records by key).  Inputs must be
 * equal or at least the sign configuration's resolution apart (1/N for the
 * default configurations).  The rank consumes one level more than
 * sfhe_sorter_rank: a context needs mult_depth = sfhe_direct_sort_params'
 * depth + 1; with less, both return SFHE_ESCHEME and the message names the
 * depth needed. */
int sfhe_sorter_sort_stable(sfhe_sorter* s, sfhe_ct* in, int n, int dg, int df, sfhe_ct** out);
int sfhe_sorter_rank_stable(sfhe_sorter* s, const sfhe_ct* in, int n, int dg, int df, sfhe_ct** out);
/* Engine extensions (additions at ABI 3): records -- several payload columns
 * placed by ONE rank.  The placement's indicator depends on the rank alone,
 * so it is evaluated once per batch for all columns; only the linear tail
 * runs per column.  outs[i] holds exactly the residues of
 * sfhe_sorter_place(rank, cols[i]).  Every column must be at one level and is
 * left at the partition's slot count, as sfhe_sorter_place leaves its input.
 * Payload values must lie in [-1, 1]: the placement error scales with |value|.
 * count = 0, count > SFHE_MAX_COLUMNS or a NULL entry: SFHE_EINVAL (one
 * column is allowed). */
#define SFHE_MAX_COLUMNS 8
int sfhe_sorter_place_many(sfhe_sorter* s, const sfhe_ct* rank, sfhe_ct* const* cols, size_t count,
                           sfhe_ct** outs);
/* rank (stable != 0: sfhe_sorter_rank_stable, else sfhe_sorter_rank) of the
 * keys, then one placement of the keys and the `count` columns: *keys_out the
 * sorted keys, outs[i] column i in the keys' order (stable: equal keys keep
 * their input order).  count = 0 sorts the keys alone (cols / outs may be
 * NULL).  stable = 1 needs mult_depth = sfhe_direct_sort_params' depth + 1;
 * with less it returns SFHE_ESCHEME and the message names the depth needed.
 * Captured like sfhe_sorter_sort, in a graph of its own: first call of a
 * shape (levels, slots, column count, stable, sign configuration) eager,
 * second captured, later ones replayed. */
int sfhe_sorter_sort_records(sfhe_sorter* s, sfhe_ct* keys, sfhe_ct* const* cols, size_t count, int stable,
                             int n, int dg, int df, sfhe_ct** keys_out, sfhe_ct** outs);
/* Engine extensions (additions at ABI 3): selection by rank -- order
 * statistics (minimum, maximum, median, quantiles, the k smallest) without
 * the full placement.  `targets` holds `count` distinct ranks in [0, N), 1 <=
 * count <= N; *out is an N-slot ciphertext whose slot i < count holds the
 * element of rank targets[i] (0 = the smallest) and whose other slots hold 0
 * up to noise, at the level sfhe_sorter_place leaves.  The indicator runs
 * ceil(count / Psel) batches, Psel = min(nextpow2(count), P), instead of the
 * placement's N / P.  Duplicate targets, a target >= N, count = 0 or count >
 * N: SFHE_EINVAL.  A missing rotation key of the in-partition folds or too
 * little depth: SFHE_ESCHEME, and the message names the amount or the depth.
 * Always eager (never captured).
 * sfhe_select_params: sfhe_direct_sort_params' depth and its rotation list
 * united with the folds' amounts {s, 2s, 3s : s = 4^i < N} (sorted, no
 * repeats); create the sorter with that list (sfhe_sorter_create_rot).
 * sfhe_sorter_select_ranked selects `in` by a rank computed before
 * (sfhe_sorter_rank / _rank_stable of `in` or of a key column: records);
 * sfhe_sorter_select computes the rank of `in` first (stable != 0: the stable
 * rank, which needs depth + 1 and selects correctly among duplicate values). */
int sfhe_select_params(uint32_t N, uint32_t* mult_depth, int32_t* rotations, size_t cap, size_t* count);
int sfhe_sorter_select_ranked(sfhe_sorter* s, const sfhe_ct* rank, const sfhe_ct* in, const uint32_t* targets,
                              size_t count, sfhe_ct** out);
int sfhe_sorter_select(sfhe_sorter* s, const sfhe_ct* in, const uint32_t* targets, size_t count, int stable, int n,
                       int dg, int df, sfhe_ct** out);
/* Engine extensions (additions at ABI 3): selection of records -- ORDER BY key
 * LIMIT k over rows.  sfhe_sorter_select_many: outs[i] holds the residues of
 * sfhe_sorter_select_ranked(rank, cols[i], targets), 1 <= ncols <=
 * SFHE_MAX_COLUMNS columns at one level (else SFHE_ESCHEME); the indicator of
 * a batch is evaluated once for all columns.  sfhe_sorter_select_records
 * computes the (stable != 0: stable) rank of `keys` first and selects the keys
 * and 0 <= ncols <= SFHE_MAX_COLUMNS payload columns by it: *keys_out is
 * sfhe_sorter_select's result, outs[i] column i's rows in the same order.
 * Targets, depth and rotation keys as sfhe_sorter_select_ranked; a NULL entry
 * or a column count out of range: SFHE_EINVAL.  Always eager. */
int sfhe_sorter_select_many(sfhe_sorter* s, const sfhe_ct* rank, const sfhe_ct* const* cols, size_t ncols,
                            const uint32_t* targets, size_t count, sfhe_ct** outs);
int sfhe_sorter_select_records(sfhe_sorter* s, const sfhe_ct* keys, const sfhe_ct* const* cols, size_t ncols,
                               const uint32_t* targets, size_t count, int stable, int n, int dg, int df,
                               sfhe_ct** keys_out, sfhe_ct** outs);
/* Engine extensions (additions at ABI 3): ordering by several keys -- ORDER BY
 * a, b [DESC], ... over rows.  `keys` holds 1 <= nkeys <= SFHE_LEX_KEYS key
 * columns at one level and slot count, keys[0] the most significant;
 * descending[i] != 0 orders by key i descending (descending = NULL: every key
 * ascending).  Rows equal on every key keep their input order.  Per key, two
 * values must be equal or at least the sign configuration's resolution apart
 * (1/N for the defaults).
 * sfhe_lex_sort_depth: the mult_depth the record sort by nkeys keys needs, the
 * stable sort's (sfhe_direct_sort_params' depth + 1 for the default
 * configuration) + nkeys - 1.
 * sfhe_sorter_rank_lex: the rank of every row in that order, nkeys - 1 levels
 * below sfhe_sorter_rank_stable; with one ascending key exactly its residues.
 * sfhe_sorter_sort_records_lex: that rank, then one placement of the keys and
 * the ncols payload columns: keys_out[i] is key column i and outs[j] column j
 * in sorted order.  sfhe_sorter_select_records_lex: that rank, then the rows of
 * the target ranks (as sfhe_sorter_select_records; rotation keys from
 * sfhe_select_params).  nkeys + ncols may be at most 1 + SFHE_MAX_COLUMNS.
 * A key count or column count out of range or a NULL entry: SFHE_EINVAL; keys
 * at different levels or too little depth: SFHE_ESCHEME, and the message
 * names the depth needed.  Always eager. */
#define SFHE_LEX_KEYS 4
int sfhe_lex_sort_depth(uint32_t N, int n, int dg, int df, uint32_t nkeys, uint32_t* mult_depth);
int sfhe_sorter_rank_lex(sfhe_sorter* s, const sfhe_ct* const* keys, size_t nkeys, const int* descending, int n,
                         int dg, int df, sfhe_ct** out);
int sfhe_sorter_sort_records_lex(sfhe_sorter* s, sfhe_ct* const* keys, size_t nkeys, const int* descending,
                                 sfhe_ct* const* cols, size_t ncols, int n, int dg, int df, sfhe_ct** keys_out,
                                 sfhe_ct** outs);
int sfhe_sorter_select_records_lex(sfhe_sorter* s, const sfhe_ct* const* keys, size_t nkeys, const int* descending,
                                   const sfhe_ct* const* cols, size_t ncols, const uint32_t* targets, size_t count,
                                   int n, int dg, int df, sfhe_ct** keys_out, sfhe_ct** outs);
/* v + (1 - q) (.) u, relinearised, one level below u (one relinearisation,
 * one rescale): the lexicographic rank's Horner step.  v and q may have more
 * limbs than u (a numerically lower level).  sfhe_lex_counts: such steps whose
 * tensor ran as one fused launch (sfp_lex_tensor) and as the composed generic
 * prims since the last sfhe_op_stats reset (SFHE_LEX_FUSED=0, read per call,
 * composes; the results are bit-identical). */
int sfhe_eval_lex_step(sfhe_ctx* c, const sfhe_ct* v, const sfhe_ct* q, const sfhe_ct* u, sfhe_ct** out);
int sfhe_lex_counts(sfhe_ctx* c, uint64_t* fused, uint64_t* composed);
/* Rescale(Relin(a (x) b + a2 (x) b2)) + r, one level below the operands: the
 * sum of two products with one relinearisation, ModDown and rescale (the sign
 * polynomials' paired products).  The four operands at one level (a product
 * among them is settled first); r: null, or a ciphertext at the result's level.
 * sfhe_dot_counts: such sums that ran as one fused launch chain
 * (sfp_mult2_relin_rescale_add) and as the composed generic prims since the
 * last sfhe_op_stats reset (SFHE_MULT_SUM2_FUSED=0, read per call, composes;
 * the results are bit-identical).  SFHE_SIGN_DOT=0 (read per call) keeps the
 * sign polynomials on two separate products. */
int sfhe_eval_mult_sum2(sfhe_ctx* c, const sfhe_ct* a, const sfhe_ct* b, const sfhe_ct* a2, const sfhe_ct* b2,
                        const sfhe_ct* r, sfhe_ct** out);
int sfhe_dot_counts(sfhe_ctx* c, uint64_t* fused, uint64_t* composed);
/* Rescale(Relin(sum_i a[i] (x) b[i])) + r for 1 <= n <= 8 terms, one level below
 * the operands: sfhe_eval_mult_sum2's contract with n pairs (all 2n operands
 * at one level, equal product scales; r: null, or a ciphertext at the result's
 * level).  The Chebyshev evaluator's remainder chains run through it
 * (SFHE_PS_DOT=0, read per call, keeps one product per node).
 * sfhe_sumn_counts: such sums that ran as one fused launch chain
 * (sfp_multn_relin_rescale_add) and as the composed generic prims since the
 * last sfhe_op_stats reset (SFHE_MULT_SUM_FUSED=0, read per call, composes;
 * the results are bit-identical); sfhe_eval_mult_sum2's are not included. */
int sfhe_eval_mult_sum(sfhe_ctx* c, const sfhe_ct* const* a, const sfhe_ct* const* b, size_t n, const sfhe_ct* r,
                       sfhe_ct** out);
int sfhe_sumn_counts(sfhe_ctx* c, uint64_t* fused, uint64_t* composed);
/* nops independent sfhe_eval_mult_sum ops in one call (EvalMultSumMany): op o
 * has counts[o] terms, the terms of all ops laid end to end in a / b; r: null,
 * or nops addends (null entries allowed); out: nops handles.  Consecutive ops
 * of one level and one term count go out as one batch, ops of different term
 * counts never share one; each result equals the op issued alone.
 * sfhe_sumn_batch_counts: such runs issued, and remainder chains of the
 * Chebyshev evaluator that fell outside the op's conditions and ran as
 * separate products, since the last sfhe_op_stats reset. */
int sfhe_eval_mult_sum_many(sfhe_ctx* c, const sfhe_ct* const* a, const sfhe_ct* const* b, const size_t* counts,
                            size_t nops, const sfhe_ct* const* r, sfhe_ct** out);
int sfhe_sumn_batch_counts(sfhe_ctx* c, uint64_t* batches, uint64_t* fallbacks);
/* A copy of ct whose scale label is multiplied by factor (the rows are not
 * touched): for testing how the evaluator treats operands of unequal scales. */
int sfhe_ct_relabel_scale(const sfhe_ct* ct, double factor, sfhe_ct** out);
/* Engine extensions (additions at ABI 3): grouping rows by an encrypted key --
 * COUNT(*), SUM(col) and ROW_NUMBER() OVER (PARTITION BY key), every result in
 * the rows' input order.  `keys` and the 0 <= ncols <= SFHE_MAX_COLUMNS payload
 * columns sit at one level and slot count.  *count: slot r holds the number of
 * rows whose key equals row r's (row r included).  *index (want_index != 0;
 * else set to NULL and `index` may be NULL): slot r holds the number of rows
 * before r with r's key, so the first row of every group holds 0.  sums_out[c]:
 * slot r holds the sum of column c over the rows with r's key.  *count is one
 * level above the others, which end at the context's sfhe_group_params depth.
 * Two keys must be equal or at least the sign configuration's resolution apart
 * (1/N for the defaults).  No placement is evaluated: the depth is the stable
 * rank's.
 * sfhe_group_params: the mult_depth of sfhe_sorter_group with N's default sign
 * configuration, and the rotation amounts it uses (the rank's: baby steps,
 * giant steps, batch offsets and partition folds in the layout of ring 2^17; at
 * a smaller ring the entry uses a subset of them or composes its own from
 * them).  cap / count as sfhe_direct_sort_params.
 * A column count out of range, a NULL entry or columns at another level or slot
 * count than the key: SFHE_EINVAL; too little depth: SFHE_ESCHEME, the message
 * naming the depth needed, before anything is computed.  Always eager. */
int sfhe_group_params(uint32_t N, uint32_t* mult_depth, int32_t* rotations, size_t cap, size_t* count);
int sfhe_sorter_group(sfhe_sorter* s, const sfhe_ct* keys, const sfhe_ct* const* cols, size_t ncols, int want_index,
                      int n, int dg, int df, sfhe_ct** count, sfhe_ct** index, sfhe_ct** sums_out);
/* outs[c] = sum_b (1 - q[b]) (.) u[c * nq + b], relinearised once per column,
 * one level below q: the grouping's gated column sums.  The nq >= 1 gates sit
 * at one level and scale; an operand may have more limbs than the gates (a
 * numerically lower level), a column's operands share one scale; 0 <= ncols <=
 * SFHE_MAX_COLUMNS.  A NULL entry, gates at different levels, an operand at a
 * numerically higher level than the gates or a count out of range: SFHE_EINVAL.
 * sfhe_group_counts: such calls whose tensors ran as fused launches
 * (sfp_gate_tensor_cols) and as the composed generic prims since the last
 * sfhe_op_stats reset (SFHE_GROUP_FUSED=0, read per call, composes; the results
 * are bit-identical). */
int sfhe_eval_gate_sum_many(sfhe_ctx* c, const sfhe_ct* const* q, size_t nq, const sfhe_ct* const* u, size_t ncols,
                            sfhe_ct** outs);
int sfhe_group_counts(sfhe_ctx* c, uint64_t* fused, uint64_t* composed);
/* Engine extensions (additions at ABI 3): aggregates over an ordered frame --
 * SUM(col) OVER (ORDER BY key) with ROW_NUMBER(), RANK() and CUME_DIST() --
 * every result in the rows' input order, with no placement.  `keys` and the
 * 0 <= ncols <= SFHE_MAX_COLUMNS payload columns (values in [-1, 1]) sit at one
 * level and slot count.  Row j is in row r's frame where
 *   SFHE_FRAME_ROWS   (key_j, j) <= (key_r, r): ROWS UNBOUNDED PRECEDING ..
 *                     CURRENT ROW in stable order
 *   SFHE_FRAME_RANGE  key_j <= key_r: SQL's default frame, peers included
 *   SFHE_FRAME_BELOW  key_j < key_r
 * sums_out[c]: slot r holds column c's sum over row r's frame.  *count
 * (want_count != 0; else set to NULL and `count` may be NULL): slot r holds the
 * number of rows in the frame -- ROW_NUMBER() under rows, N CUME_DIST() under
 * range, RANK() - 1 under below.  *count is one level above the sums, which
 * end at the context's sfhe_window_params depth: the stable rank's plus one.
 * Two keys must be equal or at least the sign configuration's resolution apart
 * (1/N for the defaults).
 * sfhe_window_params: the mult_depth of sfhe_sorter_window with N's default
 * sign configuration and the rotation amounts it uses: sfhe_group_params'.
 * An unknown frame, a column count out of range, a NULL entry or columns at
 * another level or slot count than the key: SFHE_EINVAL; too little depth:
 * SFHE_ESCHEME, the message naming the depth needed, before anything is
 * computed.  Always eager. */
#define SFHE_FRAME_ROWS 0
#define SFHE_FRAME_RANGE 1
#define SFHE_FRAME_BELOW 2
int sfhe_window_params(uint32_t N, uint32_t* mult_depth, int32_t* rotations, size_t cap, size_t* count);
int sfhe_sorter_window(sfhe_sorter* s, const sfhe_ct* keys, const sfhe_ct* const* cols, size_t ncols, int frame,
                       int want_count, int n, int dg, int df, sfhe_ct** count, sfhe_ct** sums_out);
/* outs[c] = sum_b (weights[b] + v[b]) (.) u[c * nv + b], relinearised once per
 * column, one level below v: the window sums' weighted column sums.  The nv >= 1
 * gates sit at one level and scale; weights[b] holds `len` doubles, encoded as
 * sfhe_eval_mult_plain encodes its values but at v's scale, so the sum with
 * v[b] is exact; an operand may have more limbs than the gates (a numerically
 * lower level), a column's operands share one scale; 0 <= ncols <=
 * SFHE_MAX_COLUMNS.  A NULL entry, gates at different levels, an operand at a
 * numerically higher level than the gates or a count out of range: SFHE_EINVAL.
 * sfhe_window_counts: such calls whose tensors ran as fused launches
 * (sfp_weight_tensor_cols) and as the composed generic prims since the last
 * sfhe_op_stats reset (SFHE_WINDOW_FUSED=0, read per call, composes; the
 * results are bit-identical). */
int sfhe_eval_weight_sum_many(sfhe_ctx* c, const sfhe_ct* const* v, size_t nv, const double* const* weights,
                              size_t len, uint32_t slots, const sfhe_ct* const* u, size_t ncols, sfhe_ct** outs);
int sfhe_window_counts(sfhe_ctx* c, uint64_t* fused, uint64_t* composed);
/* Engine extensions (additions at ABI 3): the join of two encrypted tables on
 * 1 <= nkeys <= 4 keys -- SELECT a.*, COUNT(b.*), SUM(b.col) FROM a LEFT JOIN b
 * ON a.k1 = b.k1 [AND a.k2 = b.k2 ...] -- every result in table A's input order.
 * keys_a[k], keys_b[k] and the 0 <= ncols <= SFHE_MAX_COLUMNS columns of table B
 * sit at one level and slot count.  *count: slot r holds the number of rows of B
 * that agree with A's row r on every key.  sums_out[c]: slot r holds the sum of
 * cols_b[c] over those rows.  *count is one level above the sums, which end at
 * the context's sfhe_join_params depth: the grouping's plus ceil(log2 nkeys).
 * Preconditions: per key, any A value and any B value are equal or at least the
 * sign configuration's resolution apart (1/N for the defaults) and their
 * difference lies in the sign's domain (the keys are in the sort's input
 * range); both tables occupy N rows: a shorter B is padded with a key no A row
 * takes, A's padded rows are ignored by the client.  With unique B keys *count
 * is the 0/1 semi-join flag (1 - *count the anti-join flag) and a sum is the
 * looked-up value; a table joined with itself is GROUP BY k1, ..., km.
 * sfhe_join_params: the mult_depth of sfhe_sorter_join on nkeys keys with N's
 * default sign configuration and the rotation amounts it uses
 * (sfhe_group_params': the rank's).  cap / count as sfhe_direct_sort_params.
 * A key or column count out of range, a NULL entry or inputs at different
 * levels or slot counts: SFHE_EINVAL; too little depth: SFHE_ESCHEME, the
 * message naming the depth needed, before anything is computed.  Always eager. */
int sfhe_join_params(uint32_t N, uint32_t nkeys, uint32_t* mult_depth, int32_t* rotations, size_t cap,
                     size_t* count);
int sfhe_sorter_join(sfhe_sorter* s, const sfhe_ct* const* keys_a, const sfhe_ct* const* keys_b, size_t nkeys,
                     const sfhe_ct* const* cols_b, size_t ncols, int n, int dg, int df, sfhe_ct** count,
                     sfhe_ct** sums_out);
/* *out = a + b - a (.) b (the OR of two 0/1 gates), relinearised once, one level
 * below the lower operand; the operands keep their own scales and may sit at
 * different levels (the one with more limbs is read over the other's).  A NULL
 * argument or different slot counts: SFHE_EINVAL.
 * sfhe_join_counts: such calls whose tensor ran as the one fused launch
 * (sfp_or_tensor) and as the composed generic prims since the last sfhe_op_stats
 * reset (SFHE_JOIN_FUSED=0, read per call, composes; the results are
 * bit-identical). */
int sfhe_eval_gate_or(sfhe_ctx* c, const sfhe_ct* a, const sfhe_ct* b, sfhe_ct** out);
int sfhe_join_counts(sfhe_ctx* c, uint64_t* fused, uint64_t* composed);
/* nodes of the captured record sort (0 while none); sfhe_sorter_graph_nodes
 * keeps reporting the plain / stable sort's graph */
int sfhe_sorter_records_graph_nodes(const sfhe_sorter* s, uint64_t* nodes);
/* Kernel / dependency nodes of the sorter's captured sort graph (engine
 * extension, no reference counterpart): sort() runs its first call of a shape
 * eagerly, captures the second into a hipGraph and replays it from then on
 * (SFHE_GRAPH=0 keeps every sort eager; debug sorters never capture).
 * 0 while no graph exists. */
int sfhe_sorter_graph_nodes(const sfhe_sorter* s, uint64_t* nodes);
/* Roofline measurement (engine extension): the NTT kernel nodes of the
 * sorter's captured sort graph re-instantiated alone, in captured order, and
 * replayed `reps` times, timed with HIP events: *ms per replay (= the NTT
 * kernel time of one sort), *launches, *bytes (algorithmic: 16 B per
 * coefficient per pass).  SFHE_EINVAL-class error when no graph exists. */
int sfhe_sorter_graph_ntt_time(sfhe_sorter* s, int reps, double* ms, uint64_t* launches, double* bytes);
/* The same for any family SFHE_KFAM_* (OTHER: the kernels of no family, ALL:
 * every kernel node -- the sort's kernel time without lane overlap); *bytes:
 * the algorithmic bytes of the family's kernels for NTT, CONV and NTTKS
 * (sources read and targets written once), 0 for the others. */
int sfhe_sorter_graph_family_time(sfhe_sorter* s, uint32_t family, int reps, double* ms, uint64_t* launches,
                                  double* bytes);
/* DirectSort<N>::sort_hybrid1 (sort_algo.h:1213-1229): constructRank, then
 * rotationIndexCheckHybrid1 (:1067-1209, MEHP24 indicatorAdv placement,
 * mehp24_utils.cpp:166-174, :246-261).  Needs ring dimension >= 2 N^2 for
 * N <= 256 and the DirectSortH1Test keys (sfhe_hybrid1_params). */
int sfhe_sorter_sort_hybrid1(sfhe_sorter* s, sfhe_ct* in, int n, int dg, int df, sfhe_ct** out);
/* Depth and rotation keys of tests/DirectSortH1Test.cpp:36-117 for N
 * (the reference keeps them in the test; ring 2^17, HEStd_128_classic). */
int sfhe_hybrid1_params(uint32_t N, uint32_t* mult_depth, int32_t* rotations, size_t cap, size_t* count);

/* DirectSort<N>::sort_hybrid (variant 0; sort_algo.h:1049-1062) and
 * sort_hybrid2 (variant 2; :1376-1389): constructRank, then the MEHP24 matrix
 * placement on rank / N with the scaled-sinc Chebyshev indicator (hybrid2;
 * hybrid below N = 256) or the composite-sign indicator |d| < 1/2N (hybrid at
 * N >= 256: CompositeSign(3,4,2) at 256, (3,5,2) above; rotationIndexCheck-
 * Hybrid :894-1047, -Hybrid2 :1233-1374).  Needs 2 N^2 <= the ring
 * dimension for N <= 256 and the keys of sfhe_hybrid_params. */
int sfhe_sorter_sort_hybrid(sfhe_sorter* s, sfhe_ct* in, int variant, int n, int dg, int df, sfhe_ct** out);
/* the DirectSortHTest (variant 0, tests/DirectSortHTest.cpp:29-100) and
 * DirectSortH2Test (variant 2, tests/DirectSortH2Test.cpp:39-108) depth and
 * rotation keys at ring 2^17 */
int sfhe_hybrid_params(uint32_t N, int variant, uint32_t* mult_depth, int32_t* rotations, size_t cap,
                       size_t* count);
/* DirectSort<N>::rotationIndexCheck2N (sort_algo.h:587-656): placement over
 * 2N-slot blocks with the scaled sinc (rank from sfhe_sorter_rank). */
int sfhe_sorter_place_2n(sfhe_sorter* s, const sfhe_ct* rank, sfhe_ct* in, sfhe_ct** out);
/* BitonicSort<N>::sort (sort_algo.h:1421-1486): the compare-and-swap network
 * over the sorter's N slots with EvalBootstrap(ct, 2, 20) whenever the level
 * passes 29 -- needs sfhe_bootstrap_setup for N slots and the +-2^i keys the
 * sorter was created with; input values in [0, 255]. */
int sfhe_sorter_sort_bitonic(sfhe_sorter* s, sfhe_ct* in, int n, int dg, int df, sfhe_ct** out);

/* Serialized I/O (src/sort.h:31-102, src/main.cpp:9-44: the FHERMA-style file
 * set).  sfhe_save writes <dir>/cc.bin, pub.bin, mult.bin, rot.bin and, if the
 * context holds it, sk.bin; sfhe_load reads them back into a new context
 * (sk.bin optional).  Records are this engine's (magic, version, kind, context
 * fingerprint), not OpenFHE's cereal layout. */
int sfhe_save(sfhe_ctx* c, const char* dir);
int sfhe_load(const char* dir, sfhe_ctx** out);
int sfhe_ct_save(sfhe_ctx* c, const sfhe_ct* ct, const char* path);
int sfhe_ct_load(sfhe_ctx* c, const char* path, sfhe_ct** out);

/* k-way sorting network: KWayAdapter<N>::sort = kwaySort::Sorter::sorter
 * (src/kway_adapter.h:66-72, src/k-way/Sorter.cpp:284-404) over k^M = the
 * ciphertext's first slots, k in {2, 3, 5}; comparisons CompositeSign(n, dg,
 * df) with lazy bootstrapping against mult_depth (SignConfig(cfg, multDepth),
 * tests/k-way/KWaySort2Test.cpp:157 -- note that test passes (3, d_f, d_g));
 * needs sfhe_bootstrap_setup for the ciphertext's slots. */
int sfhe_kway_sort(sfhe_ctx* c, const sfhe_ct* in, int k, int M, int n, int dg, int df, uint32_t mult_depth,
                   sfhe_ct** out);
/* A persistent KWayAdapter<N> (N = k^M; k = 2: N = 4 .. 1024, k = 3: 9 .. 729,
 * k = 5: 25 .. 625): the reference's adapter object (kway_adapter.h:23-35),
 * whose sorts after the first reuse the encoded masks and bootstrapping
 * diagonals. */
typedef struct sfhe_kway sfhe_kway;
int sfhe_kway_create(sfhe_ctx* c, uint32_t N, int k, int M, sfhe_kway** out);
int sfhe_kway_run(sfhe_kway* s, const sfhe_ct* in, int n, int dg, int df, uint32_t mult_depth, sfhe_ct** out);
void sfhe_kway_destroy(sfhe_kway* s);
/* Nodes of the handle's captured sort graph (0: none yet).  The first sort of
 * a shape runs eagerly, the second is captured whole -- stages and the
 * bootstraps between them -- and later sorts replay it (SFHE_GRAPH=0: eager). */
int sfhe_kway_graph_nodes(const sfhe_kway* s, uint64_t* nodes);
/* The captured k-way sort's kernels of one family (SFHE_KFAM_*) replayed
 * alone, summed over its chain of graphs: ms per sort, launches, and their
 * algorithmic bytes (NTT, conversion and k_ntt_ks families; 0 for others).
 * No reference counterpart (bench attribution of BASELINE config 4). */
int sfhe_kway_graph_family_time(sfhe_kway* s, uint32_t family, int reps, double* ms, uint64_t* launches,
                                double* bytes);
/* KWayAdapter<N>::getSizeParameters (kway_adapter.h:41-64): batch (next power
 * of two >= N), depth 40, first modulus 60 / scale 59 bits, level budget
 * {4,4} (N <= 128) or {5,5}, the +-2^i rotation keys below N. */
int sfhe_kway_params(uint32_t N, uint32_t* batch, uint32_t* mult_depth, uint32_t* budget_c2s, uint32_t* budget_s2c,
                     int32_t* rotations, size_t cap, size_t* count);

/* Decomposer<N>::decompose (rotation.h:54-102); algo 0 NAF, 1 BNAF, 2 BINARY.
 * N in {4..1024}; writes (value, stepSize) pairs. */
int sfhe_decompose(uint32_t N, const int32_t* keys, size_t nkeys, int32_t rotation, int32_t wrapN,
                   int algo, int32_t* values, int32_t* steps, size_t cap, size_t* count);

/* ---- limb sharding (no reference counterpart: the reference
 * runs one process on one device) -------------------------------------------
 * One process per GPU; rank r of W holds the RNS limbs q_i / p_k with
 * i % W == r / k % W == r of every ciphertext level with more than the
 * replicated-tail limb count (SFHE_SHARD_TAIL, default 16; below it every
 * rank holds and computes every limb, without exchanges).  Key generation
 * and encryption run on every limb (setup) and every rank keeps whole
 * switching keys; evaluation runs on the local limbs only, with three
 * exchanges: the ModUp input (all-gather of the coefficient-form Q limbs),
 * the ModDown P limbs (all-gather) and a rescale's dropped limb (broadcast by
 * its owner), plus one all-gather where a ciphertext enters the tail.
 * Decryption and sfhe_ct_download all-gather the limbs.  Every rank makes
 * the same calls in the same order (they are collective); results are
 * bit-identical to the unsharded context.  Call once per context, after
 * sfhe_context_create and before sfhe_keygen, with the same params and seed
 * on every rank.  RCCL-sharded sorts are captured into hipGraphs with their
 * collectives; a one-rank RCCL communicator takes the sharded path too. */
/* 128-byte RCCL unique id (one rank; shared out of band).  SFHE_ENOTIMPL on
 * a backend without RCCL (the CPU oracle). */
int sfhe_comm_uid(uint8_t uid[128]);
/* RCCL communicator over xGMI (the product path). */
int sfhe_shard_rccl(sfhe_ctx* c, int rank, int world, const uint8_t uid[128]);
/* Host-memory collectives supplied by the caller (tests; any transport):
 * allgather writes world blocks of `bytes`, rank-major, into recv. */
typedef void (*sfhe_allgather_fn)(void* user, const void* send, void* recv, size_t bytes);
typedef void (*sfhe_bcast_fn)(void* user, void* buf, size_t bytes, int root);
int sfhe_shard_host(sfhe_ctx* c, int rank, int world, sfhe_allgather_fn ag, sfhe_bcast_fn bc,
                    void* user);
/* The replicated-tail limb count of a sharded context (0: unsharded). */
int sfhe_shard_tail(const sfhe_ctx* c, uint32_t* limbs);
/* Rows per digit part of this rank's switching keys: num_q + num_p for whole
 * keys; a sharded rank of world > 1 keeps only its slice (the replicated
 * tail's Q rows, its own dealt Q rows, the P rows; SFHE_KEY_SLICE=0: whole). */
int sfhe_key_rows(const sfhe_ctx* c, uint32_t* rows);

/* ---- batch groups (no reference counterpart) ------------------------------
 * DirectSort's rank and placement phases each run B independent batches
 * (reference src/sort_algo.h:438-492, 713-742, the OpenMP batch loop).  With
 * G batch groups, the ranks form G groups of W/G (each group limb-sharded
 * over its own communicator, or one unsharded rank); group g runs the
 * batches b with b % G == g and every part is all-gathered over a second
 * communicator joining the ranks that hold the same rows in different groups
 * (in-group rank r of every group).  Every rank ends with the same,
 * bit-identical result as the unsplit sort.  B not a multiple of G: every
 * group runs every batch; one group (groups == 1) runs every batch and
 * still routes each part through the communicator (single-GPU validation of
 * the collective).  Call before sfhe_keygen, with the same params and
 * seed on every rank; the calls are collective like the sharded ones. */
int sfhe_groups_rccl(sfhe_ctx* c, int group, int groups, const uint8_t uid[128]);
int sfhe_groups_host(sfhe_ctx* c, int group, int groups, sfhe_allgather_fn ag, void* user);
int sfhe_groups(const sfhe_ctx* c, int* group, int* groups);

#ifdef __cplusplus
}
#endif
#endif /* SFHE_H */
