// RNS polynomial primitive layer (L1 in SURVEY.md §1).
//
// Two implementations exist and are bit-for-bit interchangeable:
//   * csrc/hip/prims_hip.hip  -- the product: hand-written gfx950 kernels;
//   * oracle/prims_ref.c      -- the CPU oracle (test infrastructure only).
// The host CKKS layer (csrc/core/*.cpp) is compiled against this interface
// once per backend.  The product library never contains the oracle.
//
// Data layout (HBM): a polynomial with L limbs is L contiguous rows of n u64
// residues, limb-major: limb i at base + i*n.  A ciphertext is two such
// polynomials back to back (c0 rows, then c1 rows).  Limb i of a polynomial
// uses prime index  i < split ? i : pbase + (i - split)  in the context's
// prime table [q_0 .. q_L, p_0 .. p_{K-1}] (the "limb map").
//
// Every primitive is enqueued on the backend's stream; the host observes
// results only through sfp_d2h (which synchronises).
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SFP_MAX_LIMBS 96
#define SFP_MAX_WSUM 80

typedef struct sfp_dev sfp_dev;

typedef struct {
    uint32_t count;   // number of limbs
    uint32_t split;   // limbs [0, split) -> primes base, base + stride, ...
    uint32_t pbase;   // limbs [split, count) -> primes pbase, pbase + stride, ...
    uint32_t base;    // (0 unless addressing a run that starts mid-table)
    uint32_t stride;  // prime step between consecutive limbs; 0 or 1 = contiguous.
                      // A limb-sharded rank r of W holds primes r, r + W, ...
} sfp_limbs;

static inline uint32_t sfp_prime_of(sfp_limbs m, uint32_t i) {
    const uint32_t st = m.stride ? m.stride : 1;
    return i < m.split ? m.base + i * st : m.pbase + (i - m.split) * st;
}

// Tables the host computes once per context (identical for both backends).
typedef struct {
    uint32_t logn;
    uint32_t nprimes;       // L+1+K
    const uint64_t* primes; // nprimes
    // per prime, n entries each (bit-reversed psi powers, OpenFHE/SEAL layout)
    const uint64_t* psi_rev;        // [nprimes][n]
    const uint64_t* psi_rev_shoup;  // [nprimes][n]
    const uint64_t* ipsi_rev;       // [nprimes][n]
    const uint64_t* ipsi_rev_shoup; // [nprimes][n]
    const uint64_t* n_inv;          // [nprimes]
    const uint64_t* n_inv_shoup;    // [nprimes]
} sfp_tables;

// Base-conversion table for fast basis extension from a source set S of
// primes to a target set T (Halevi-Polyakov-Shoup / OpenFHE "PartQlHat"):
//   y_i  = x_i * shat_inv[i] mod s_i                 (i in S)
//   out_t = sum_i y_i * shat_mod[i][t] mod t          (t in T)
// where shat = prod(S) / s_i.  Lives in backend memory (sfp_upload_conv).
typedef struct sfp_conv sfp_conv;

// ---- lifetime / memory --------------------------------------------------
sfp_dev* sfp_create(int device, const sfp_tables* t);
void sfp_destroy(sfp_dev* d);
const char* sfp_backend_name(void);
void* sfp_alloc(sfp_dev* d, size_t bytes);
void sfp_free(sfp_dev* d, void* p);
void sfp_h2d(sfp_dev* d, void* dst, const void* src, size_t bytes);
void sfp_d2h(sfp_dev* d, void* dst, const void* src, size_t bytes);
void sfp_d2d(sfp_dev* d, void* dst, const void* src, size_t bytes);
void sfp_zero(sfp_dev* d, void* dst, size_t bytes);
void sfp_sync(sfp_dev* d);
// Returns 0 if no asynchronous error is pending; otherwise an error string.
const char* sfp_last_error(sfp_dev* d);

// ---- NTT ----------------------------------------------------------------
// In-place negacyclic NTT of every limb (forward: coefficient -> evaluation
// at psi^(2*brev(k)+1); inverse includes the 1/n factor).
void sfp_ntt(sfp_dev* d, uint64_t* p, sfp_limbs m, int inverse);

// ---- elementwise ----------------------------------------------------------
void sfp_add(sfp_dev* d, uint64_t* out, const uint64_t* a, const uint64_t* b, sfp_limbs m);
void sfp_sub(sfp_dev* d, uint64_t* out, const uint64_t* a, const uint64_t* b, sfp_limbs m);
void sfp_neg(sfp_dev* d, uint64_t* out, const uint64_t* a, sfp_limbs m);
void sfp_mul(sfp_dev* d, uint64_t* out, const uint64_t* a, const uint64_t* b, sfp_limbs m);
// out = a * b + c  (pointwise)
void sfp_mul_add(sfp_dev* d, uint64_t* out, const uint64_t* a, const uint64_t* b,
                 const uint64_t* c, sfp_limbs m);
// out[i] = a[i] * k[limb] (k: host array of m.count residues)
void sfp_mul_const(sfp_dev* d, uint64_t* out, const uint64_t* a, const uint64_t* k,
                   sfp_limbs m);
// out[i] = a[i] + k[limb]
void sfp_add_const(sfp_dev* d, uint64_t* out, const uint64_t* a, const uint64_t* k,
                   sfp_limbs m);
// Ciphertext tensor: d0 = a0 b0, d1 = a0 b1 + a1 b0, d2 = a1 b1
void sfp_tensor(sfp_dev* d, uint64_t* d0, uint64_t* d1, uint64_t* d2, const uint64_t* a0,
                const uint64_t* a1, const uint64_t* b0, const uint64_t* b1, sfp_limbs m);
// out = sum_j ins[j] * k[j][limb]  (+ k0[limb] if k0 != NULL), j < nin <= SFP_MAX_WSUM.
// ins: host array of device pointers; k: host array nin x m.count.
void sfp_lin_wsum(sfp_dev* d, uint64_t* out, const uint64_t* const* ins, const uint64_t* k,
                  uint32_t nin, sfp_limbs m);
// Several weighted sums of the same ciphertext inputs in one pass (the
// Chebyshev leaves): for o < nout, p in {0, 1}:
//   out + o*out_stride + p*poly_stride  =  sum_j in_p[j] * k[o][j][limb]
// in0/in1: host arrays of nin device pointers (c0 / c1 of each input),
// nin <= SFP_MAX_WSUM; k: host array nout x nin x m.count.
void sfp_lin_wsum_multi(sfp_dev* d, uint64_t* out, size_t out_stride, size_t poly_stride,
                        const uint64_t* const* in0, const uint64_t* const* in1, uint32_t nin,
                        const uint64_t* k, uint32_t nout, sfp_limbs m);

// out = sum_j a[j] * b[j]  (pointwise products summed, nin <= SFP_MAX_WSUM).
// a, b: host arrays of device pointers.
void sfp_mac_plain(sfp_dev* d, uint64_t* out, const uint64_t* const* a, const uint64_t* const* b,
                   uint32_t nin, sfp_limbs m);
// Both polynomials of a ciphertext sum at once (each plaintext read once):
// out0 = sum_j a0[j] * b[j], out1 = sum_j a1[j] * b[j]  (nin <= SFP_MAX_WSUM).
void sfp_mac_plain2(sfp_dev* d, uint64_t* out0, uint64_t* out1, const uint64_t* const* a0,
                    const uint64_t* const* a1, const uint64_t* const* b, uint32_t nin, sfp_limbs m);
// ng such sums over the SAME ciphertexts (a0, a1) with their own plaintexts
// b[g * nin + j]: out0[g] / out1[g], g < ng <= SFP_MAC_MULTI_G, nin <=
// SFP_MAC_MULTI_N -- the giant steps of one baby-step set, each ciphertext
// row read once for all of them.  The same residues as ng sfp_mac_plain2
// calls.  Returns 0, or -1 (shape unsupported: the caller runs those calls).
#define SFP_MAC_MULTI_G 8
#define SFP_MAC_MULTI_N 32
int sfp_mac_plain2_multi(sfp_dev* d, uint64_t* const* out0, uint64_t* const* out1, const uint64_t* const* a0,
                         const uint64_t* const* a1, const uint64_t* const* b, uint32_t nin, uint32_t ng,
                         sfp_limbs m);

// ---- automorphism ----------------------------------------------------------
// out = sigma_g(in) in the evaluation domain (g odd, < 2n); out != in.
void sfp_automorph(sfp_dev* d, uint64_t* out, const uint64_t* in, uint32_t galois, sfp_limbs m);

// ---- rescale ------------------------------------------------------------------
// in: ell limbs (evaluation domain, limb map identity); out: ell-1 limbs,
//   out_i = (in_i - [in_last]_{q_i}) * q_last^{-1} mod q_i   (in_last taken in
//   coefficient domain with the rounding offset floor(q_last/2)).
// qlinv: host array ell-1 of q_last^{-1} mod q_i.  npoly polynomials (stride
// in_stride / out_stride u64) are processed.
void sfp_rescale(sfp_dev* d, uint64_t* out, const uint64_t* in, uint32_t ell, const uint64_t* qlinv,
                 uint32_t npoly, size_t in_stride, size_t out_stride);
// Same, but the dropped (last) row is modulo prime index drop_prime instead of
// ell-1 (rows 0..ell-2 stay primes 0..ell-2): the extended-modulus
// encryption's division by q_ext.
void sfp_rescale_ext(sfp_dev* d, uint64_t* out, const uint64_t* in, uint32_t ell,
                     uint32_t drop_prime, const uint64_t* qlinv, uint32_t npoly, size_t in_stride,
                     size_t out_stride);

// Rescale of a product, fused (the product is never written out):
//   sfp_mul_const_rescale: out = Rescale(in * k_i), k = host array of ell
//                          per-row residues (EvalMult(ct, double), level adjust)
//   sfp_mul_rescale:       out = Rescale(in (.) m), m = ell plaintext rows
//                          shared by the npoly polys (EvalMult(ct, pt))
// Bit-identical to sfp_mul_const / sfp_mul followed by sfp_rescale.
void sfp_mul_const_rescale(sfp_dev* d, uint64_t* out, const uint64_t* in, const uint64_t* k,
                           uint32_t ell, const uint64_t* qlinv, uint32_t npoly, size_t in_stride,
                           size_t out_stride);
void sfp_mul_rescale(sfp_dev* d, uint64_t* out, const uint64_t* in, const uint64_t* m, uint32_t ell,
                     const uint64_t* qlinv, uint32_t npoly, size_t in_stride, size_t out_stride);

// ---- basis conversion / key switching ----------------------------------------
// Upload a conversion table: ns source primes (prime indices src_idx), nt
// target primes (dst_idx) written to output rows dst_row[t] (NULL: row t);
// shat_inv[ns], shat_mod[ns][nt].
sfp_conv* sfp_upload_conv(sfp_dev* d, uint32_t ns, const uint32_t* src_idx, uint32_t nt,
                          const uint32_t* dst_idx, const uint32_t* dst_row,
                          const uint64_t* shat_inv, const uint64_t* shat_mod);
void sfp_free_conv(sfp_dev* d, sfp_conv* c);
// Fast base conversion in the COEFFICIENT domain: src has ns rows; target t
// is written to dst row dst_row[t].
void sfp_conv_apply(sfp_dev* d, uint64_t* dst, const uint64_t* src, const sfp_conv* c);
// Centred conversion (source values taken in (-s_i/2, s_i/2], as ModDown)
// to the first nt_use targets only.
void sfp_conv_apply_centered(sfp_dev* d, uint64_t* dst, const uint64_t* src, const sfp_conv* c,
                             uint32_t nt_use);

// Hybrid key-switch ModUp of every digit (evaluation domain in and out).
//   in   : ell limbs (limb map identity), evaluation domain.
//   ext  : beta = ceil(ell/alpha) extended polys of ell+K rows each (stride
//          (ell+K)*n; row t < ell is prime t, row ell+k is prime Lq+k).  Rows
//          of digit j's own range [j*alpha, min((j+1)*alpha, ell)) are copies
//          of `in`; all others are NTT(Conv_j(INTT(in[digit j]))), with
//          convs[j] writing rows by its dst_row table.
//   scratch: ell*n words.
void sfp_modup(sfp_dev* d, uint64_t* ext, const uint64_t* in, uint32_t ell, uint32_t K,
               uint32_t Lq, uint32_t alpha, const sfp_conv* const* convs, uint64_t* scratch);

// ModUp fused with the key inner product (one key switch's ModUp + inner
// product without the extended digits' round trip through HBM): the same
// acc0 / acc1 as sfp_modup followed by sfp_ks_inner_fold (fold0 != NULL),
// sfp_ks_inner_acc (accum) or sfp_ks_inner -- except that the rows
// t >= inv_from (the P rows: ell; with the dropped q row: ell - 1; UINT32_MAX:
// none) leave after the first (ROW) pass of ModDown's inverse NTT, so the
// ModDown that follows is called with row_done = 1.  ext: beta * (ell+K) * n
// words of scratch (the COL-pass intermediate), scr: ell * n words.  Returns
// -1 (and does nothing) where the backend has no fused form -- rings of one
// NTT tile, SFHE_KS_FUSE=0, the oracle -- and the caller runs the unfused prims.
int sfp_modup_inner(sfp_dev* d, uint64_t* acc0, uint64_t* acc1, const uint64_t* in, uint32_t ell, uint32_t K,
                    uint32_t Lq, uint32_t alpha, const sfp_conv* const* convs, const uint64_t* key,
                    const uint64_t* fold0, const uint64_t* fold1, uint64_t fold_k, int accum, uint32_t inv_from,
                    uint64_t* ext, uint64_t* scratch);
// sfp_modup_inner in two halves (the same launches): phases 1 = the ModUp
// (INTT of `in` into scratch, the digits' conversions and forward COL pass
// into ext), 2 = the fused ROW pass + inner product reading ext and `in`
// (the same ext / scratch / in as its phase 1), 3 = both; 0 = only report
// whether the fused form exists (0) or not (-1).  Independent key switches
// run their phase 1 as batched ops, then their accumulating phase 2 in turn.
int sfp_modup_inner_phase(sfp_dev* d, uint64_t* acc0, uint64_t* acc1, const uint64_t* in, uint32_t ell, uint32_t K,
                          uint32_t Lq, uint32_t alpha, const sfp_conv* const* convs, const uint64_t* key,
                          const uint64_t* fold0, const uint64_t* fold1, uint64_t fold_k, int accum,
                          uint32_t inv_from, uint64_t* ext, uint64_t* scratch, int phases);

// Build (and cache) whatever per-level tables the fused ModUp of `ell` limbs
// needs, outside any sort: the context calls it for every level at key
// generation (built lazily, each level's upload drained the device inside
// the first sort).  No-op where no fused form exists (the oracle).
void sfp_modup_prepare(sfp_dev* d, const sfp_conv* const* convs, uint32_t ell, uint32_t K, uint32_t alpha);

// Key inner product:  acc0 = sum_j ext_j * kb_j,  acc1 = sum_j ext_j * ka_j
//   ext  : beta extended polys, each (ell+K) limbs, stride ext_stride.
//   key  : beta digits, each [b rows (Lq+K)][a rows (Lq+K)]; ext limb t maps to
//          key row t (t < ell) or Lq + (t - ell).
void sfp_ks_inner(sfp_dev* d, uint64_t* acc0, uint64_t* acc1, const uint64_t* ext,
                  size_t ext_stride, const uint64_t* key, uint32_t beta, uint32_t ell, uint32_t K,
                  uint32_t Lq);
// sfp_ks_inner of the extended digits under the automorphism X -> X^gal: ext
// is read at the source index sfp_automorph maps each coefficient from, as if
// the digits had been permuted first (a hoisted rotation: the permuted copy
// of its digits is never written).
void sfp_ks_inner_aut(sfp_dev* d, uint64_t* acc0, uint64_t* acc1, const uint64_t* ext,
                      size_t ext_stride, const uint64_t* key, uint32_t beta, uint32_t ell, uint32_t K,
                      uint32_t Lq, uint32_t gal);
// Key inner product times a plaintext in the extended basis, accumulated
// (double hoisting: a hoisted rotation's product with a diagonal before its
// ModDown, EvalRotMultAddHoisted):
//   acc_p (+)= pm (.) sum_j ext_j * key_p,j   per ext limb, pm: ell+K rows
//   (the plaintext's q rows then its P rows, evaluation domain).
void sfp_ks_inner_mul(sfp_dev* d, uint64_t* acc0, uint64_t* acc1, const uint64_t* ext,
                      size_t ext_stride, const uint64_t* key, uint32_t beta, uint32_t ell, uint32_t K,
                      uint32_t Lq, const uint64_t* pm, int accum);
// sfp_ks_inner_mul of the digits under X -> X^gal (as sfp_ks_inner_aut)
void sfp_ks_inner_mul_aut(sfp_dev* d, uint64_t* acc0, uint64_t* acc1, const uint64_t* ext,
                          size_t ext_stride, const uint64_t* key, uint32_t beta, uint32_t ell, uint32_t K,
                          uint32_t Lq, const uint64_t* pm, int accum, uint32_t gal);
// sfp_ks_inner accumulating: acc0 += sum_j ext_j * kb_j, acc1 += sum_j ext_j * ka_j
// (the key switches of a rotation sum share one ModDown, EvalRotateSum).
void sfp_ks_inner_acc(sfp_dev* d, uint64_t* acc0, uint64_t* acc1, const uint64_t* ext,
                      size_t ext_stride, const uint64_t* key, uint32_t beta, uint32_t ell, uint32_t K,
                      uint32_t Lq);

// ModDown of both key-switch accumulators:
//   out_p,i (+)= (acc_p,i - NTT(Conv_{P->Q}(INTT(acc_p,P)))_i) * pinv_i,
//   with the P->Q conversion on centred residues (zero-mean rounding error).
//   acc : two polys of ell+K rows (q rows then P rows, evaluation domain),
//         acc_1 = acc + acc_stride; their P rows are destroyed.
//   add0/add1: accumulate into out0/out1 instead of overwriting.
//   pinv: host array ell of P^{-1} mod q_i.  scratch: 2*ell*n words.
//   row_done: the P rows already had their inverse NTT's first pass
//   (sfp_modup_inner with inv_from = ell).
void sfp_moddown2(sfp_dev* d, uint64_t* out0, uint64_t* out1, uint64_t* acc, size_t acc_stride,
                  uint32_t ell, uint32_t K, uint32_t Lq, const sfp_conv* c, const uint64_t* pinv,
                  int add0, int add1, uint64_t* scratch, int row_done);

// sfp_ks_inner that also folds the relinearised polys' last q row into the
// accumulators: acc_p,l += fold_k * fold_p,l  (l = ell-1, fold_k = P mod q_l),
// the input sfp_moddown_rescale expects.
void sfp_ks_inner_fold(sfp_dev* d, uint64_t* acc0, uint64_t* acc1, const uint64_t* ext,
                       size_t ext_stride, const uint64_t* key, uint32_t beta, uint32_t ell,
                       uint32_t K, uint32_t Lq, const uint64_t* fold0, const uint64_t* fold1,
                       uint64_t fold_k);

// ModDown + add + rescale in one conversion (EvalMult's relinearisation and
// its rescale).  With acc from sfp_ks_inner_fold(fold = d0, d1), l = ell-1:
//   s_p,i = d_p,i + ModDown(acc_p)_i  (i < l),   s_p,l = ModDown(acc_p)_l
//   out_p = Rescale(s_p)  (l rows at out0 / out1)
// Bit-identical to sfp_moddown2(add) + sfp_rescale on unfolded accumulators:
// the dropped row's coefficients r = (INTT(acc_l) - conv_l) P^-1 come out of
// the conversion, and out_i = (acc_i - NTT(conv_i + P [r]_i)) (P q_l)^-1
// + d_i q_l^-1 needs one NTT instead of two.
//   pinv[i] = P^-1, pmod[i] = P mod q_i (i < ell);  qlinv[i] = q_l^-1 mod q_i
//   (i < l).  acc is destroyed.  scratch: 2*l*n words.  row_done: rows
//   [l, ell+K) already had their inverse NTT's first pass (inv_from = l).
void sfp_moddown_rescale(sfp_dev* d, uint64_t* out0, uint64_t* out1, const uint64_t* d0,
                         const uint64_t* d1, uint64_t* acc, size_t acc_stride, uint32_t ell,
                         uint32_t K, uint32_t Lq, const sfp_conv* c, const uint64_t* pinv,
                         const uint64_t* pmod, const uint64_t* qlinv, uint64_t* scratch, int row_done);

// EvalMult(ct, ct) end to end from its operands (a0, a1) and (b0, b1) (ell
// rows each, evaluation domain): the tensor, the relinearisation with `key`
// and the rescale -- bit-identical to sfp_tensor followed by sfp_modup +
// sfp_ks_inner_fold (fold_k = pmod[ell-1]) + sfp_moddown_rescale, with the
// tensor's three products formed inside those passes (never written out).
// out0 / out1: ell - 1 rows.  acc: 2 (ell+K) n words, ext: beta (ell+K) n,
// scratch: 2 ell n.  Returns -1 (nothing done) where the backend has no fused
// form (the caller runs the unfused prims).
int sfp_mult_relin_rescale(sfp_dev* d, uint64_t* out0, uint64_t* out1, const uint64_t* a0, const uint64_t* a1,
                           const uint64_t* b0, const uint64_t* b1, uint32_t ell, uint32_t K, uint32_t Lq,
                           uint32_t alpha, const sfp_conv* const* convs, const uint64_t* key, const sfp_conv* c,
                           const uint64_t* pinv, const uint64_t* pmod, const uint64_t* qlinv, uint64_t* acc,
                           uint64_t* ext, uint64_t* scratch);

// ---- optional: a sum folded into the producing op's last pass ---------------
// Weak declarations: a backend may leave them out (the C oracle does).  The
// host layer calls one only where its address is non-null and, where it
// returns -1 (no fused form here, nothing done), runs the producing prim
// followed by sfp_add / sfp_sub / sfp_add_const -- the same integers, as the
// sum is one modular addition on the canonical residue the last pass stores.
//   (r0, r1): rows of a ciphertext at the output's limb count, added (sign
//   >= 0) or subtracted (sign < 0); may be null.
//   cst: host residues added per row (null: none) -- ell - 1 of them for
//   polynomial 0 in the two relinearising forms, npoly * (ell - 1) (polynomial
//   major; 0 where a polynomial has none) in sfp_rescale_add.
#if defined(__GNUC__)
#define SFP_OPTIONAL __attribute__((weak))
#else
#define SFP_OPTIONAL
#endif
SFP_OPTIONAL int sfp_mult_relin_rescale_add(sfp_dev* d, uint64_t* out0, uint64_t* out1, const uint64_t* a0,
                                            const uint64_t* a1, const uint64_t* b0, const uint64_t* b1, uint32_t ell,
                                            uint32_t K, uint32_t Lq, uint32_t alpha, const sfp_conv* const* convs,
                                            const uint64_t* key, const sfp_conv* c, const uint64_t* pinv,
                                            const uint64_t* pmod, const uint64_t* qlinv, uint64_t* acc, uint64_t* ext,
                                            uint64_t* scratch, const uint64_t* r0, const uint64_t* r1, int sign,
                                            const uint64_t* cst);
SFP_OPTIONAL int sfp_moddown_rescale_add(sfp_dev* d, uint64_t* out0, uint64_t* out1, const uint64_t* d0,
                                         const uint64_t* d1, uint64_t* acc, size_t acc_stride, uint32_t ell,
                                         uint32_t K, uint32_t Lq, const sfp_conv* c, const uint64_t* pinv,
                                         const uint64_t* pmod, const uint64_t* qlinv, uint64_t* scratch, int row_done,
                                         const uint64_t* r0, const uint64_t* r1, int sign, const uint64_t* cst);
SFP_OPTIONAL int sfp_rescale_add(sfp_dev* d, uint64_t* out, const uint64_t* in, uint32_t ell, const uint64_t* qlinv,
                                 uint32_t npoly, size_t in_stride, size_t out_stride, const uint64_t* cst);
// sfp_mul_const_rescale with sfp_rescale_add's per-row constants: out =
// Rescale(in * k_i) + cst.
SFP_OPTIONAL int sfp_mul_const_rescale_add(sfp_dev* d, uint64_t* out, const uint64_t* in, const uint64_t* k,
                                           uint32_t ell, const uint64_t* qlinv, uint32_t npoly, size_t in_stride,
                                           size_t out_stride, const uint64_t* cst);

// ---- optional: the sum of two products relinearised once ------------------------
// out = Rescale(Relin(a (x) b + a' (x) b')) (+- r, + cst): with
//   d0 = a0 b0 + a0' b0',  d1 = a0 b1 + a1 b0 + a0' b1' + a1' b0',  d2 = a1 b1 + a1' b1'
// (each the canonical residue of the sum of the two tensors' canonical
// components: sfp_tensor twice, then sfp_add per component) the integers of
// sfp_modup + sfp_ks_inner_fold (fold_k = pmod[ell-1]) + sfp_moddown_rescale on
// (d0, d1, d2), then the sum of sfp_mult_relin_rescale_add.  The launch chain
// is that of sfp_mult_relin_rescale: the second operand set is read where the
// first is (the ModUp's first pass and own digits, the fold at row ell - 1,
// the last pass's epilogue); no component is written out.  Arguments as
// sfp_mult_relin_rescale_add; (c0, c1), (e0, e1): the second pair's rows.
// Weak like the prims above: where its address is null (the C oracle) or it
// returns -1 (no fused form here, nothing done) the host layer composes it.
SFP_OPTIONAL int sfp_mult2_relin_rescale_add(sfp_dev* d, uint64_t* out0, uint64_t* out1, const uint64_t* a0,
                                             const uint64_t* a1, const uint64_t* b0, const uint64_t* b1,
                                             const uint64_t* c0, const uint64_t* c1, const uint64_t* e0,
                                             const uint64_t* e1, uint32_t ell, uint32_t K, uint32_t Lq, uint32_t alpha,
                                             const sfp_conv* const* convs, const uint64_t* key, const sfp_conv* c,
                                             const uint64_t* pinv, const uint64_t* pmod, const uint64_t* qlinv,
                                             uint64_t* acc, uint64_t* ext, uint64_t* scratch, const uint64_t* r0,
                                             const uint64_t* r1, int sign, const uint64_t* cst);

// ---- optional: the sum of m products relinearised once ---------------------------
// out = Rescale(Relin(sum_i a_i (x) b_i)) (+- r, + cst), 1 <= m <= SFP_MULT_SUM_MAX:
// sfp_mult2_relin_rescale_add's integers with m quadruples -- each component
// the canonical residue of the sum of the m tensors' canonical components
// (sfp_tensor m times, sfp_add per component), then sfp_modup +
// sfp_ks_inner_fold + sfp_moddown_rescale and the sum.  One product's launch
// chain: its three operand-reading passes loop over the further row sets.
// rows: 4 m host pointers, (a0, a1, b0, b1) of product i at rows[4 i ..]; the
// other arguments as sfp_mult_relin_rescale_add.  m = 1 is that prim, m = 2
// is sfp_mult2_relin_rescale_add.  Returns -1 (declined, nothing done) for m
// out of range, a null or misaligned row set, or a ring of one NTT tile.
#define SFP_MULT_SUM_MAX 8
SFP_OPTIONAL int sfp_multn_relin_rescale_add(sfp_dev* d, uint64_t* out0, uint64_t* out1,
                                             const uint64_t* const* rows, uint32_t m, uint32_t ell, uint32_t K,
                                             uint32_t Lq, uint32_t alpha, const sfp_conv* const* convs,
                                             const uint64_t* key, const sfp_conv* c, const uint64_t* pinv,
                                             const uint64_t* pmod, const uint64_t* qlinv, uint64_t* acc, uint64_t* ext,
                                             uint64_t* scratch, const uint64_t* r0, const uint64_t* r1, int sign,
                                             const uint64_t* cst);

// ---- optional: several constant rescales of one input in one launch pair per direction
// Term j of m (2 <= m <= SFP_MAX_CONST_TERMS) is sfp_mul_const_rescale(_add)
// of the input's first ell_j rows: out_j = Rescale(in * k_j) (+ cst_j), k_j
// ell_j host residues, qlinv_j the ell_j - 1 rescale constants of that limb
// count, cst_j null or npoly * (ell_j - 1) host residues.  The terms' dropped
// rows share one inverse NTT launch pair and their kept rows one forward pair
// (a row-group set per term; terms of different limb counts are sets of
// different primes and row counts).  The same integers as the m separate
// calls.  Returns 1 when issued merged, 0 when it issued the terms one by one
// (one-tile rings, more rows than one launch takes), -1 on an error (recorded,
// nothing issued).
#define SFP_MAX_CONST_TERMS 4
typedef struct {
    uint32_t ell;
    const uint64_t* k;
    const uint64_t* qlinv;
    uint64_t* out;
    size_t out_stride;
    const uint64_t* cst;
} sfp_const_term;
SFP_OPTIONAL int sfp_const_terms_rescale(sfp_dev* d, const uint64_t* in, size_t in_stride, uint32_t npoly,
                                         const sfp_const_term* t, uint32_t m);

// ---- optional: the tie-aware rank term's tensor (stable rank sort) ---------------
// With (u0, u1) = (w s0 + k, w s1) -- s a ciphertext (s0, s1), w a plaintext,
// k[limb] host residues, all m.count rows in the evaluation domain -- the
// tensor of s and u in ONE launch:
//   d0 = s0 u0,  d1 = s0 u1 + s1 u0,  d2 = s1 u1
// u is never stored.  The canonical residues of sfp_mul (u0 = s0 w, u1 = s1 w),
// sfp_add_const (u0 += k) and sfp_tensor(s, u): four launches.  The outputs
// may not overlap the inputs.  k travels in the kernel's arguments: no upload
// and no host synchronisation, so the prim may be captured and issued on any
// lane.  Weak like the prims above: where its address is null (the C oracle),
// or it returns -1 (a shape it does not handle: nothing done), the host layer
// runs the four prims.
SFP_OPTIONAL int sfp_tie_tensor(sfp_dev* d, uint64_t* d0, uint64_t* d1, uint64_t* d2, const uint64_t* s0,
                                const uint64_t* s1, const uint64_t* w, const uint64_t* k, sfp_limbs m);

// ---- optional: the lexicographic rank's Horner step (sort by several keys) -------
// With (a0, a1) = (kr - q0, -q1) -- q, v and u ciphertexts, kr[limb] and
// lr[limb] host residues, all m.count rows in the evaluation domain -- the
// tensor of a and u plus lr v in ONE launch:
//   d0 = lr v0 + a0 u0,  d1 = lr v1 + a0 u1 + a1 u0,  d2 = a1 u1
// i.e. lr v + (kr - q) (.) u before its relinearisation.  a is never stored.
// The canonical residues of sfp_neg (q0, q1), sfp_add_const (+ kr),
// sfp_tensor(a, u), sfp_mul_const (lr v0, lr v1) and two sfp_add: eight
// launches.  Each output is one reduction of the exact sum of its products
// (d1: three products of residues below 2^60, under 3 * 2^120).  kr and lr
// travel in the kernel's arguments: no upload and no host synchronisation, so
// the prim may be captured and issued on any lane.  Weak like the prims above:
// where its address is null (the C oracle), or it returns -1 with nothing
// written (more than SFP_MAX_LIMBS rows, a row not 16-byte aligned, an output
// overlapping an input), the host layer runs the generic prims.
SFP_OPTIONAL int sfp_lex_tensor(sfp_dev* d, uint64_t* d0, uint64_t* d1, uint64_t* d2, const uint64_t* v0,
                                const uint64_t* v1, const uint64_t* q0, const uint64_t* q1, const uint64_t* u0,
                                const uint64_t* u1, const uint64_t* kr, const uint64_t* lr, sfp_limbs m);

// ---- optional: the OR of two gates (join on several keys) ------------------------
// With (na0, na1) = (-a0, -a1) -- a and b ciphertexts, ka[limb] and kb[limb]
// host residues (of a's and of b's scale), all m.count rows in the evaluation
// domain -- the tensor of na and b plus kb a + ka b in ONE launch:
//   d0 = kb a0 + ka b0 + na0 b0,  d1 = kb a1 + ka b1 + na0 b1 + na1 b0,  d2 = na1 b1
// i.e. kb a + ka b - a (.) b before its relinearisation.  na is never stored.
// The canonical residues of sfp_neg (a0, a1), sfp_tensor(na, b), four
// sfp_mul_const (kb a0, kb a1, ka b0, ka b1) and four sfp_add: eleven launches.
// Each output is one reduction of the exact sum of its products (d1: four
// products of canonical residues of primes of at most 60 bits, under 2^122).
// ka and kb travel in the kernel's arguments: no upload and no host
// synchronisation, so the prim may be captured and issued on any lane.  Weak
// like the prims above: where its address is null (the C oracle), or it returns
// -1 with nothing written (more than SFP_MAX_LIMBS rows, a row not 16-byte
// aligned, an output overlapping an input or another output), the host layer
// runs the generic prims.
SFP_OPTIONAL int sfp_or_tensor(sfp_dev* d, uint64_t* d0, uint64_t* d1, uint64_t* d2, const uint64_t* a0,
                               const uint64_t* a1, const uint64_t* b0, const uint64_t* b1, const uint64_t* ka,
                               const uint64_t* kb, sfp_limbs m);

// ---- optional: the grouping's gated column sums (GROUP BY an encrypted key) ------
// nb gates q_b (ciphertexts q0[b], q1[b]) shared by nc columns, column c's
// operand of batch b the ciphertext u0[c * nb + b], u1[c * nb + b]; with
// (a0, a1)_b = (kr - q_b0, -q_b1), kr[limb] host residues, all m.count rows in
// the evaluation domain:
//   d0[c] = sum_b a_b0 u_bc0,  d1[c] = sum_b (a_b0 u_bc1 + a_b1 u_bc0),  d2[c] = sum_b a_b1 u_bc1
// i.e. sum_b (kr - q_b) (.) u_bc before its ONE relinearisation per column.
// Issued as tiles of two columns and a remainder of one (kernel
// k_gate_tensor_cols<CT>): a tile reads each q word once for its columns.  The
// canonical residues of, per batch, sfp_neg (q0, q1) and sfp_add_const (+ kr),
// per (b, c) sfp_tensor(a_b, u_bc), and three sfp_add from the second batch
// on.  Each output is one reduction of the exact sum of its products: d1 sums
// 2 nb products of canonical residues of primes of at most 60 bits, below
// 2^125 for nb <= SFP_GATE_MAX_B = 16.  Pointers and kr travel in the kernels'
// arguments: no upload and no host synchronisation, so the prim may be
// captured and issued on any lane.  Weak like the prims above: where its
// address is null (the C oracle), or it returns -1 with nothing written (nb = 0
// or nb > SFP_GATE_MAX_B, nc = 0 or nc > SFP_GATE_MAX_C, more than
// SFP_MAX_LIMBS rows, a row not 16-byte aligned, an output overlapping an
// input or another output), the host layer runs the generic prims.
#define SFP_GATE_MAX_B 16
#define SFP_GATE_MAX_C 8
SFP_OPTIONAL int sfp_gate_tensor_cols(sfp_dev* d, uint64_t* const* d0, uint64_t* const* d1, uint64_t* const* d2,
                                      const uint64_t* const* q0, const uint64_t* const* q1,
                                      const uint64_t* const* u0, const uint64_t* const* u1, const uint64_t* kr,
                                      uint32_t nb, uint32_t nc, sfp_limbs m);

// ---- optional: the window sums' weighted column sums (SUM OVER an ordered frame) --
// nb gates p_b + v_b -- v_b a ciphertext (v0[b], v1[b]), p_b a plaintext row
// p[b] -- shared by nc columns, column c's operand of batch b the ciphertext
// u0[c * nb + b], u1[c * nb + b]; with (a0, a1)_b = (p_b + v_b0 mod q, v_b1),
// a_b0 the canonical residue sfp_add stores, all m.count rows in the evaluation
// domain:
//   d0[c] = sum_b a_b0 u_bc0,  d1[c] = sum_b (a_b0 u_bc1 + a_b1 u_bc0),  d2[c] = sum_b a_b1 u_bc1
// i.e. sum_b (p_b + v_b) (.) u_bc before its ONE relinearisation per column.
// Issued as tiles of two columns and a remainder of one (kernel
// k_weight_tensor_cols<CT>): a tile reads each v and p word once for its
// columns.  The canonical residues of, per batch, sfp_add (v_b0, p_b), per
// (b, c) sfp_tensor(a_b, u_bc), and three sfp_add from the second batch on.
// Each output is one reduction of the exact sum of its products: d1 sums 2 nb
// products of canonical residues of primes of at most 60 bits, below 2^125 for
// nb <= SFP_WEIGHT_MAX_B = 16.  Every pointer travels in the kernels'
// arguments: no upload and no host synchronisation, so the prim may be
// captured and issued on any lane.  Weak like the prims above: where its
// address is null (the C oracle), or it returns -1 with nothing written (nb = 0
// or nb > SFP_WEIGHT_MAX_B, nc = 0 or nc > SFP_WEIGHT_MAX_C, more than
// SFP_MAX_LIMBS rows, a row not 16-byte aligned, an output overlapping an
// input or another output), the host layer runs the generic prims.
#define SFP_WEIGHT_MAX_B 16
#define SFP_WEIGHT_MAX_C 8
SFP_OPTIONAL int sfp_weight_tensor_cols(sfp_dev* d, uint64_t* const* d0, uint64_t* const* d1, uint64_t* const* d2,
                                        const uint64_t* const* v0, const uint64_t* const* v1,
                                        const uint64_t* const* p, const uint64_t* const* u0,
                                        const uint64_t* const* u1, uint32_t nb, uint32_t nc, sfp_limbs m);

// ---- optional: the giant-step sums of several columns under one plaintext set ----
// nc columns (records' payloads placed by one rank) share the ng x nin
// plaintexts b[g * nin + j] of sfp_mac_plain2_multi; column c has its own
// ciphertext rows a0[c * nin + j] / a1[c * nin + j]:
//   out0[c * ng + g] = sum_j a0[c * nin + j] * b[g * nin + j],  out1 likewise with a1
// (ng <= SFP_MAC_COLS_G, nc <= SFP_MAC_COLS_C, nin <= SFP_MAC_MULTI_N; all
// host arrays of device pointers to 16-byte aligned rows).  Issued as tiles of
// giants x columns: each plaintext word is read once for a tile's columns and
// each ciphertext word once for its giants.  The canonical residues of nc
// sfp_mac_plain2_multi calls (nc * ng sfp_mac_plain2 calls).  No upload and no
// host synchronisation: capturable, any lane.  Weak like the prims above:
// where its address is null (the C oracle) or it returns -1 (a shape it does
// not handle: nothing done), the host layer runs sfp_mac_plain2_multi per column.
#define SFP_MAC_COLS_G 64
#define SFP_MAC_COLS_C 16
SFP_OPTIONAL int sfp_mac_plain2_cols(sfp_dev* d, uint64_t* const* out0, uint64_t* const* out1,
                                     const uint64_t* const* a0, const uint64_t* const* a1, const uint64_t* const* b,
                                     uint32_t nin, uint32_t ng, uint32_t nc, sfp_limbs m);

// ---- optional: the key inner products of several rotations of one ciphertext ----
// acc_p = sum_k sum_j sigma_k(ext_j) (.) key_k,p,j for R <= SFP_FOLD_MAX pairs
// (Galois element gals[k], switching key keys[k]) over the SHARED extended
// digits ext (as sfp_ks_inner_aut reads them for one gal): one launch, every
// product of the R terms in the 128-bit accumulators, one reduction.  The
// canonical residues of sfp_automorph of the digits + sfp_ks_inner for the
// first term and + sfp_ks_inner_acc for the others (R permuted copies and R
// launches, the accumulators read back R - 1 times).  keys and gals are host
// arrays that travel in the kernel's arguments: no upload and no host
// synchronisation, so the prim may be captured and issued on any lane.  Weak
// like the prims above: where its address is null (the C oracle) or it returns
// -1 (nothing done: R or R * beta too large, rows not 16-byte aligned, a
// sliced key geometry) the host layer runs the composed form.
#define SFP_FOLD_MAX 7
SFP_OPTIONAL int sfp_ks_inner_aut_sum(sfp_dev* d, uint64_t* acc0, uint64_t* acc1, const uint64_t* ext,
                                      size_t ext_stride, const uint64_t* const* keys, const uint32_t* gals,
                                      uint32_t R, uint32_t beta, uint32_t ell, uint32_t K, uint32_t Lq);

// ---- optional: sfp_ks_inner_aut_sum over several columns that share the keys ----
// for c < nc: acc_c,p = sum_k sum_j sigma_k(ext_c,j) (.) key_k,p,j  (k < R, j < beta)
// nc columns (1 <= nc <= SFP_FOLD_COLS: the payload columns of a selection,
// EvalRotateFoldMany), each with its own extended digits ext[c] (one stride)
// and accumulator pair acc0[c] / acc1[c], share the R <= SFP_FOLD_MAX (Galois
// element, key) pairs.  Issued as tiles of columns: a tile reads each key word
// and computes each source index once for its columns (the keys are two
// thirds of the one-column prim's traffic); a single left-over column runs
// sfp_ks_inner_aut_sum.  Column c's output is the canonical residue of the
// integer sum sfp_ks_inner_aut_sum leaves for it.  Every array is a host array
// that travels in the kernels' arguments: no upload and no host
// synchronisation, any lane.  Returns the number of launches issued (>= 1),
// or -1 with nothing done: nc = 0 or nc > SFP_FOLD_COLS, R > SFP_FOLD_MAX,
// R * beta > 256, a row not 16-byte aligned, a sliced key geometry, an output
// overlapping an input or another output.  Weak like the prims above: where
// its address is null (the C oracle) or it declines, the host layer runs the
// composed form.
#define SFP_FOLD_COLS 16
SFP_OPTIONAL int sfp_ks_inner_aut_sum_cols(sfp_dev* d, uint64_t* const* acc0, uint64_t* const* acc1,
                                           const uint64_t* const* ext, size_t ext_stride, uint32_t nc,
                                           const uint64_t* const* keys, const uint32_t* gals, uint32_t R,
                                           uint32_t beta, uint32_t ell, uint32_t K, uint32_t Lq);

// ---- optional: CKKS decoding on the device (the end of a decryption) ----------
// `count` row sets src + b * srcStride, each nl (1 or 2) COEFFICIENT-domain
// rows of n words modulo primes 0 .. nl-1 (c0 + c1 s after its inverse NTT),
// decoded as `slots`-slot sparse packings: the centred CRT lift of the
// coefficients i gap and n/2 + i gap (gap = n / (2 slots); nothing else is
// read), as doubles divided by scales[b] (host array), through the special
// FFT -- bit-identical to the host path (CryptoContextImpl::Decrypt's lift
// followed by core/encoder.cpp ckks_decode).  out (device): count * slots
// (re, im) pairs, batch-major; it is also the working buffer.  Needs
// sfp_encode_setup's tables.  No host synchronisation of its own (the scales
// travel through the argument ring).  Weak like the prims above: the host
// layer decodes on the host where its address is null (the C oracle).
SFP_OPTIONAL int sfp_decode_batch(sfp_dev* d, const uint64_t* src, size_t srcStride, uint32_t count, uint32_t nl,
                                  uint32_t slots, const double* scales, double* out);

// ---- sampling (counter-based, deterministic) ------------------------------------
// Uniform residues mod each limb's prime: value for (limb, i) is derived from
// splitmix64(seed, stream-id = prime index, i); identical on every backend.
void sfp_sample_uniform(sfp_dev* d, uint64_t* p, sfp_limbs m, uint64_t seed);
// Load signed coefficients (same for every limb) reduced mod each prime.
void sfp_load_i64(sfp_dev* d, uint64_t* p, const int64_t* coeffs, sfp_limbs m);

// ---- optional: small polynomials sampled on the device ---------------------------
// `count` polynomials, polynomial j into the m.count coefficient-domain rows at
// p + j * stride.  Coefficient i of polynomial j is a function of (seeds[j], i)
// alone, r = splitmix64(seeds[j] + i):
//   SFP_SMALL_TERNARY  (int64)(r % 3) - 1
//   SFP_SMALL_CBD20    popcount(r & 0xFFFFF) - popcount((r >> 20) & 0xFFFFF)
// (the host layer's sampleTernary / sampleCBD), stored in every row as
// sfp_load_i64 stores that value: q - |v| for v < 0, v otherwise.  seeds and
// kinds are host arrays; they travel through the argument ring, so the prim
// has no host synchronisation (sfp_load_i64 drains every lane).  Weak like the
// prims above: where its address is null (the C oracle) the host layer samples
// on the host and loads.
#define SFP_SMALL_TERNARY 0u
#define SFP_SMALL_CBD20 1u
SFP_OPTIONAL int sfp_sample_small(sfp_dev* d, uint64_t* p, size_t stride, uint32_t count, const uint64_t* seeds,
                                  const uint32_t* kinds, sfp_limbs m);
// The sums of `count` public-key encryptions at one limb count in one launch.
// Ciphertext b has v, e0, e1 (evaluation domain; ell rows of primes 0 .. ell-1
// and, with ext, one more row of prime ext_prime) at t + (3 b + {0, 1, 2}) *
// stride, and its message's ell rows at msg[b].  pkb / pka: the public key's
// rows, row i < ell for prime i and row pk_ext_row for ext_prime.
//   ext:  out0[b] = v pkb + e0 + k_i msg on the ell rows (k: host array of ell
//         residues, q_ext mod q_i) and v pkb + e0 on the ext row; out1[b] =
//         v pka + e1 -- ell + 1 rows each, the input of sfp_rescale_ext
//   else: out0[b] = v pkb + e0 + msg, out1[b] = v pka + e1 (ell rows; k unused)
// out0[b] / out1[b] may be b's own e0 / e1 rows (in place).  The canonical
// residues of the sfp_mul_add / sfp_mul_const / sfp_add sequence.  msg, out0
// and out1 are host arrays of device pointers (argument ring: no host
// synchronisation).  Weak, as sfp_sample_small.
SFP_OPTIONAL int sfp_encrypt_combine(sfp_dev* d, const uint64_t* t, size_t stride, uint32_t count,
                                     const uint64_t* const* msg, uint64_t* const* out0, uint64_t* const* out1,
                                     const uint64_t* pkb, const uint64_t* pka, uint32_t pk_ext_row, uint32_t ell,
                                     int ext, uint32_t ext_prime, const uint64_t* k);

// ---- CKKS encoding on the device ------------------------------------------------
// The host encoder's tables, uploaded once per device: rot[j] = 5^j mod 2n
// (j < n/2) and ksi[k] = exp(2 pi i k / 2n) as (re, im) pairs (k <= 2n).
void sfp_encode_setup(sfp_dev* d, const uint64_t* rot, const double* ksi);
// p (rows of map m, COEFFICIENT domain) = the residues of the encoding of
// `nvals` slot values (host array: doubles when `real`, else (re, im) pairs)
// zero-padded to `slots`: the special inverse FFT, packed sparsely (gap
// n / (2 slots)), each coefficient round(u * scale).  Bit-identical to the
// host encoder (core/encoder.cpp ckks_encode) followed by sfp_load_i64,
// provided no coefficient needs the encoder's 2^shift range extension (the
// caller checks |value| * scale < 2e18).  No host synchronisation (the values
// travel through the argument ring), so it may run inside a graph capture.
// scratch: 2 * slots words.
void sfp_encode(sfp_dev* d, uint64_t* p, const double* vals, uint32_t nvals, int real, uint32_t slots,
                double scale, sfp_limbs m, uint64_t* scratch);
// `count` encodings at once (one slot count, value count and real-ness):
// rows dst + b * dstStride <- the encoding of vals + b * nvals (* 2 when
// complex), each as sfp_encode; scratch: count * 2 * slots words
void sfp_encode_batch(sfp_dev* d, uint64_t* dst, size_t dstStride, const double* vals, uint32_t nvals,
                      uint32_t count, int real, uint32_t slots, double scale, sfp_limbs m, uint64_t* scratch);
// sfp_ntt of `count` row sets p + b * stride (each the rows of map m), one launch per pass
void sfp_ntt_batch(sfp_dev* d, uint64_t* p, size_t stride, uint32_t count, sfp_limbs m, int inverse);

// ---- lanes: independent in-order queues (HIP streams) ----------------------------
// Every prim launches on the current lane.  Work on different lanes may run
// concurrently; order it with events.  The oracle has one synchronous lane
// and treats every call below as satisfied.
#define SFP_MAX_LANES 16  // (real lanes <= 8; the rest: a batched op's virtual lanes)
typedef struct sfp_event sfp_event;
int sfp_lanes(sfp_dev* d);
void sfp_set_lane(sfp_dev* d, int lane);
int sfp_get_lane(sfp_dev* d);
// Event at the current end of the current lane.
sfp_event* sfp_event_record(sfp_dev* d);
// The current lane waits (device-side) for `e`; no-op for an event of this lane.
void sfp_event_wait(sfp_dev* d, const sfp_event* e);
int sfp_event_done(sfp_dev* d, const sfp_event* e);
void sfp_event_free(sfp_dev* d, sfp_event* e);
// Lane `waiter` waits for everything enqueued so far on lane `waitee`.
void sfp_lane_wait(sfp_dev* d, int waiter, int waitee);

// ---- stacked launches ----------------------------------------------------------
// Between sfp_stack_begin and sfp_stack_end the lanes' work is recorded per
// lane and issued at the end (or at any host synchronisation) on lane 0's
// stream: each lane's work in its own order, every event wait after its
// record, and two lanes' next launches of the same kernel (NTT pass, fused
// key-switch pass, base conversion, ModDown+rescale conversion) over
// different rows merged into ONE launch -- the sort's batches, which run the
// same op sequence on two lanes, take half the launches.  Results are
// bit-identical.  No-op for the oracle, with serialised lanes, or with
// SFHE_STACK=0.  sfp_stack_stats: launches issued merged (pairs) / alone.
void sfp_stack_begin(sfp_dev* d);
void sfp_stack_end(sfp_dev* d);
void sfp_stack_stats(sfp_dev* d, uint64_t* merged, uint64_t* single);

// Batched ops (the same mechanism for independent ops of ONE host lane: the
// Chebyshev PS's products of one tree level, a polynomial's powers of one
// depth).  sfp_batch_begin(d, count) returns 1 if batching is on; the host
// then issues op i after sfp_batch_lane(d, i) and calls sfp_batch_end, which
// issues everything on the caller's lane, identical launches of different ops
// merged into one (up to eight; four for the element-wise kernels).  The ops' buffers must stay allocated until
// sfp_batch_end (their launches are issued there).  Returns 0 (the ops run as
// issued) for the oracle, with SFHE_BATCH=0 or inside a stacked lane region.
// Serialised lanes (sfp_serialize) still batch: a profiling sort then issues
// the same merged launches as the captured sort, each timed as ONE launch
// carrying the bytes of every op merged into it.
#define SFP_BATCH_MAX 8
int sfp_batch_begin(sfp_dev* d, uint32_t count);
void sfp_batch_lane(sfp_dev* d, uint32_t i);
void sfp_batch_end(sfp_dev* d);

// ---- multi-process limb sharding (one process per GPU) --------------------------
// Collectives over the ranks of a sharded context, ordered on the current
// lane like every other primitive.  Two transports:
//   * RCCL (HIP backend, production): sfp_comm_uid on one rank, the 128-byte
//     id shared out of band (torch.distributed), sfp_comm_init_rccl on all;
//   * host callbacks (both backends; tests): the caller's allgather/bcast over
//     host memory (e.g. torch.distributed gloo), after a stream drain.
typedef void (*sfp_host_allgather_fn)(void* user, const void* send, void* recv, size_t bytes);
typedef void (*sfp_host_bcast_fn)(void* user, void* buf, size_t bytes, int root);
// 0 on success; -1 where the backend has no RCCL (the oracle)
int sfp_comm_uid(void* uid128);
int sfp_comm_init_rccl(sfp_dev* d, int rank, int world, const void* uid128);
void sfp_comm_set_host(sfp_dev* d, int rank, int world, sfp_host_allgather_fn ag, sfp_host_bcast_fn bc,
                       void* user);
// 1 when the collectives can be recorded into a graph (RCCL, or no
// communicator at all); 0 for a host transport (it synchronises)
int sfp_comm_capturable(sfp_dev* d);
// recv = world blocks of `bytes`, rank-major (recv may contain send in place)
void sfp_allgather(sfp_dev* d, const void* send, void* recv, size_t bytes);
void sfp_bcast(sfp_dev* d, void* buf, size_t bytes, int root);

// Batch groups (the sort's independent batches split over GPU groups,
// DESIGN.md §7): a second communicator joining the ranks that hold the same
// rows of different batches -- rank `group` of `groups`.  Only an all-gather;
// same transports and ordering as above.
int sfp_group_init_rccl(sfp_dev* d, int group, int groups, const void* uid128);
void sfp_group_set_host(sfp_dev* d, int group, int groups, sfp_host_allgather_fn ag, void* user);
// recv = groups blocks of `bytes`, group-major (recv may contain send in place)
void sfp_group_allgather(sfp_dev* d, const void* send, void* recv, size_t bytes);

// Collective statistics (multi-GPU attribution: the bench splits a sharded
// sort's time into compute and exchange).  sfp_comm_stats_reset zeroes the
// counters; timed != 0 also brackets every collective with events on the
// stream it runs on (eager work only: a captured collective is counted, not
// timed).  sfp_comm_stats: collectives this rank issued since the reset (the
// all-gathers and broadcasts of both communicators that moved data), the
// bytes this rank received through them, and their summed duration in ms
// (0 unless timed).  Synchronises the lanes.
void sfp_comm_stats_reset(sfp_dev* d, int timed);
void sfp_comm_stats(sfp_dev* d, uint64_t* calls, double* bytes, double* ms);

// dst row i = src row rows[i] (count rows of n words; rows: host array)
void sfp_gather_rows(sfp_dev* d, uint64_t* dst, const uint64_t* src, const uint32_t* rows, uint32_t count);

// Rescale with the dropped row supplied in coefficient form (limb sharding:
// the row's owner broadcast it):  out_p,i = (in_p,i - [last_p]_{q_i}) * qlinv_i
// for the rows of map m (evaluation domain), last_p the centred lift of the
// dropped row modulo prime drop_prime.  npoly polys: in / out / last strides.
void sfp_rescale_rows(sfp_dev* d, uint64_t* out, const uint64_t* in, const uint64_t* last,
                      uint32_t drop_prime, sfp_limbs m, const uint64_t* qlinv, uint32_t npoly,
                      size_t in_stride, size_t out_stride, size_t last_stride);

// Key inner product with explicit maps (limb sharding): ext rows follow the
// prime map pm (pm.split Q rows then P rows); ext row t uses key row
// t < pm.split ? t : keyQ + (t - pm.split) of each digit's [b rows][a rows]
// block of key_rows rows -- or, with keyQ == SFP_KEY_ROW_BY_PRIME, the key row
// of its prime (a whole key, key_rows = Lq + K: row r is prime r).
//   accum: acc (+)= the inner product (as sfp_ks_inner_acc)
#define SFP_KEY_ROW_BY_PRIME 0xFFFFFFFFu

// Switching-key geometry (sliced keys).  By default a key digit
// is [b rows][a rows] of Lq + K rows each, row r holding prime r.  A limb-
// sharded rank keeps a slice: the `tail` Q rows of the replicated levels
// (primes 0 .. tail-1), its own dealt Q primes >= tail (first, first + world,
// ... < lq), then the K P rows, `rows` in all (pstart = rows - K):
//   row(p) = p < tail ? p : p < lq ? tail + (p - first) / world : pstart + (p - lq)
// Every key prim then reads that layout: ext row t < ell of a replicated level
// reads row t, its P rows row pstart + (t - ell), and SFP_KEY_ROW_BY_PRIME
// reads row(prime).  rows == 0: whole keys (the default).
typedef struct {
    uint32_t rows, pstart, tail, world, first, lq;
} sfp_key_geom;
void sfp_set_key_geom(sfp_dev* d, const sfp_key_geom* g);
static inline uint32_t sfp_key_row(const sfp_key_geom* g, uint32_t p) {
    if (!g->rows) return p;
    return p < g->tail ? p : p < g->lq ? g->tail + (p - g->first) / g->world : g->pstart + (p - g->lq);
}
void sfp_ks_inner_map(sfp_dev* d, uint64_t* acc0, uint64_t* acc1, const uint64_t* ext,
                      size_t ext_stride, const uint64_t* key, uint32_t beta, sfp_limbs pm,
                      uint32_t keyQ, uint32_t key_rows, int accum);

// ---- graph capture (hipGraph) ---------------------------------------------------
// Between sfp_capture_begin and sfp_capture_end every prim enqueued on lane 0
// -- and on any lane that waited for it (sfp_lane_wait / sfp_event_wait) -- is
// recorded into a graph instead of running; the lanes must be joined back to
// lane 0 before the end.  Small host arrays the prims upload (weights, row
// tables, kernel constants) go to a per-graph device arena filled once at the
// end, so the recorded launches read immutable copies.  Any host
// synchronisation inside the region (a download, an upload, a ring wrap)
// invalidates the capture: sfp_capture_end then returns NULL and records why.
// The oracle backend has no graphs: sfp_capture_begin returns -1.
typedef struct sfp_graph sfp_graph;
int sfp_capture_begin(sfp_dev* d);
// forget the recorded error (an abandoned capture is not a device fault)
void sfp_clear_error(sfp_dev* d);
sfp_graph* sfp_capture_end(sfp_dev* d);
int sfp_capturing(sfp_dev* d);
// Enqueue the whole graph on the current lane (stream-ordered like a prim).
void sfp_graph_launch(sfp_dev* d, sfp_graph* g);
size_t sfp_graph_nodes(const sfp_graph* g);
// The graph's kernel nodes of family `fam` (SFP_FAM_*; SFP_FAM_COUNT = every
// kernel of no family, SFP_FAM_ALL = every kernel node), re-instantiated in
// their captured order as a graph of their own and replayed `reps` times,
// timed with HIP events on the current lane: the family's kernels alone,
// back to back, with exactly the captured launch parameters.  Returns 0 and
// the milliseconds per replay, the launches and the algorithmic bytes of
// their NTT passes per replay; -1 where the backend has no graphs.
int sfp_graph_family_time(sfp_dev* d, sfp_graph* g, uint32_t fam, int reps, double* ms, uint64_t* launches,
                          double* bytes);
void sfp_graph_destroy(sfp_dev* d, sfp_graph* g);

// ---- live kernel timing ---------------------------------------------------------
// Kernel families timed with events recorded on the backend's stream around
// single launches.  Algorithmic bytes per launch (minimum HBM traffic):
//   NTT pass     16 B per coefficient (read + write once; twiddles excluded)
//   CONV         8 B per source coefficient read + 8 B per target written
//   KSINNER      8 B per ext / key / accumulator word touched (k_ks_inner)
//   NTTKS        the same for k_ntt_ks (ModUp's ROW pass fused with the inner product)
// Inside a stacked region the launches are timed as issued (a merged pair is
// one launch with the bytes of both).
enum { SFP_FAM_NTT = 0, SFP_FAM_CONV = 1, SFP_FAM_KSINNER = 2, SFP_FAM_NTTKS = 3, SFP_FAM_COUNT = 4, SFP_FAM_ALL = 5 };
// Time every `period`-th launch of `fam` (0 = off); resets its counters.
void sfp_prof_set(sfp_dev* d, uint32_t fam, uint32_t period);
// Since the last sfp_prof_set: launches seen, launches timed, their summed
// duration (ms) and summed algorithmic bytes.  Synchronises the stream.
int sfp_prof_read(sfp_dev* d, uint32_t fam, uint64_t* launches, uint64_t* timed, double* ms,
                  double* bytes);
// on != 0: every lane's work goes to lane 0's stream in issue order (a valid
// order: the host issues each op after its inputs), so timed launches do not
// overlap other lanes' kernels -- per-launch durations as rocprof reports them.
void sfp_serialize(sfp_dev* d, int on);

#ifdef __cplusplus
}
#endif
