/*
 * phantom_amd.h — C-ABI of the MI355X-native CKKS hot path (libphantom_amd.so).
 *
 * Plain pointers and sizes only.  Device buffers are caller-owned HIP allocations laid out
 * like the reference's: a polynomial is limb-major uint64_t data[limb * n + k], a ciphertext
 * is poly-major data[(poly * L + limb) * n + k], every value in [0, q_limb).  All compute
 * entry points enqueue asynchronously on the given stream (the reference hard-codes
 * cudaStreamPerThread, e.g. src/evaluate.cu:1200) and return a status code instead of
 * throwing.  The entries that copy a pointer or entry table from host memory, or build tables
 * for one call, wait for `stream` once before they return (everything else returns while the
 * stream still runs; tests/test_gpu_stream_order.py holds both lists to the code):
 *   phantom_fast_bconv, phantom_bconv_create, phantom_lt_bsgs, phantom_lt_bsgs_group,
 *   phantom_fast_rotation_ext_batch_group, phantom_leaf_combine, phantom_ext_mac,
 *   phantom_ext_mac_sub, phantom_ext_mac_sub_seeded, phantom_rotate_sum_ext,
 *   phantom_conv2d_prepare, phantom_conv2d_prepare_scaled, phantom_ltprep_stage_products,
 *   phantom_ltprep_presence, phantom_ltprep_finish.
 *
 * Each entry point names the reference interface it replaces (file:line, relative to the
 * PhantomFHE repository root).
 */
#ifndef PHANTOM_AMD_H
#define PHANTOM_AMD_H

#include <stddef.h>
#include <stdint.h>
#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------------------ */
#define PHANTOM_OK 0
#define PHANTOM_ERR_INVALID_ARGUMENT 1 /* std::invalid_argument in the reference (e.g. include/ntt.cuh:149) */
#define PHANTOM_ERR_HIP 2              /* std::runtime_error from PHANTOM_CHECK_CUDA (cuda_wrapper.cuh:19-47) */
#define PHANTOM_ERR_LOGIC 3            /* std::logic_error (e.g. CoeffModulus::Create out of primes) */
#define PHANTOM_ERR_INTERNAL 4

const char *phantom_status_string(int status);
/* message of the last error raised on the calling host thread ("" if none) */
const char *phantom_last_error(void);
/* library build identification, e.g. "phantom-amd 0.1 gfx950" */
const char *phantom_version(void);

/* ---- parameters (src/host/modulus.cu:80-111, src/host/numth.cu:207-332) ----------- */
/* CoeffModulus::Create(poly_modulus_degree, bit_sizes) -> out[count] */
int phantom_coeff_modulus_create(size_t poly_modulus_degree, const int *bit_sizes, size_t count, uint64_t *out);

/* ---- NTT tables (DNTTTable, include/ntt.cuh:36-129; built at src/context.cu:170-183) --- */
typedef struct phantom_ntt_tables phantom_ntt_tables;
int phantom_ntt_tables_create(size_t poly_modulus_degree, const uint64_t *moduli, size_t num_moduli,
                              phantom_ntt_tables **out);
int phantom_ntt_tables_destroy(phantom_ntt_tables *tables);
/* host copies of the tables for modulus index i (each array of length n) */
int phantom_ntt_tables_host(const phantom_ntt_tables *tables, size_t i, uint64_t *tw, uint64_t *tw_shoup,
                            uint64_t *itw, uint64_t *itw_shoup, uint64_t *n_inv);

/* ---- NTT launchers (include/ntt.cuh:157-226) ---------------------------------------- */
/* nwt_2d_radix8_forward_inplace(inout, tables, coeff_modulus_size, start_modulus_idx, stream)
 * (include/ntt.cuh:173-174, src/ntt/fntt_2d.cu:620-653) */
int phantom_nwt_forward_inplace(uint64_t *inout, const phantom_ntt_tables *tables, size_t coeff_modulus_size,
                                size_t start_modulus_idx, hipStream_t stream);
/* nwt_2d_radix8_backward_inplace (include/ntt.cuh:203-204, src/ntt/intt_2d.cu:724-757) */
int phantom_nwt_backward_inplace(uint64_t *inout, const phantom_ntt_tables *tables, size_t coeff_modulus_size,
                                 size_t start_modulus_idx, hipStream_t stream);
/* nwt_2d_radix8_backward(out, in, ...) (include/ntt.cuh:206-207, src/ntt/ntt_modup.cu:9-200) */
int phantom_nwt_backward(uint64_t *out, const uint64_t *in, const phantom_ntt_tables *tables,
                         size_t coeff_modulus_size, size_t start_modulus_idx, hipStream_t stream);
/* nwt_2d_radix8_backward_scale (include/ntt.cuh:209-211, src/ntt/ntt_modup.cu:356-393):
 * out = INTT(in) * scale[limb]; scale/scale_shoup are device arrays of coeff_modulus_size */
int phantom_nwt_backward_scale(uint64_t *out, const uint64_t *in, const phantom_ntt_tables *tables,
                               size_t coeff_modulus_size, size_t start_modulus_idx, const uint64_t *scale,
                               const uint64_t *scale_shoup, hipStream_t stream);
/* nwt_2d_radix8_forward_inplace_include_special_mod_exclude_range (include/ntt.cuh:188-193,
 * src/ntt/ntt_modup.cu:610-657): buffer limbs >= coeff_modulus_size - size_P use the last
 * size_P table rows (the special primes); limbs in [excluded_range_start, excluded_range_end)
 * are skipped. */
int phantom_nwt_forward_include_special_mod_exclude_range(uint64_t *inout, const phantom_ntt_tables *tables,
                                                          size_t coeff_modulus_size, size_t start_modulus_idx,
                                                          size_t size_QP, size_t size_P,
                                                          size_t excluded_range_start, size_t excluded_range_end,
                                                          hipStream_t stream);
/* nwt_2d_radix8_backward_inplace_include_special_mod (include/ntt.cuh:213-216,
 * src/ntt/intt_2d.cu:796-834) */
int phantom_nwt_backward_inplace_include_special_mod(uint64_t *inout, const phantom_ntt_tables *tables,
                                                     size_t coeff_modulus_size, size_t start_modulus_idx,
                                                     size_t size_QP, size_t size_P, hipStream_t stream);

/* nwt_2d_radix8_backward_inplace_scale (include/ntt.cuh:213-215): in place, output times scale[limb] */
int phantom_nwt_backward_inplace_scale(uint64_t *inout, const phantom_ntt_tables *tables, size_t coeff_modulus_size,
                                       size_t start_modulus_idx, const uint64_t *scale, const uint64_t *scale_shoup,
                                       hipStream_t stream);
/* nwt_2d_radix8_forward_inplace_include_special_mod (include/ntt.cuh:187-190) */
int phantom_nwt_forward_include_special_mod(uint64_t *inout, const phantom_ntt_tables *tables,
                                            size_t coeff_modulus_size, size_t start_modulus_idx, size_t size_QP,
                                            size_t size_P, hipStream_t stream);
/* nwt_2d_radix8_forward_inplace_fuse_moddown (include/ntt.cuh:176-180, src/ntt/ntt_moddown.cu:106-261):
 * ct = (cx - NTT(delta)) * bigPInv_mod_q per limb; delta (coefficient form) is the NTT input and
 * is not written back (this engine's epilogue form) */
int phantom_nwt_forward_fuse_moddown(uint64_t *ct, const uint64_t *cx, const uint64_t *bigPInv_mod_q,
                                     const uint64_t *bigPInv_mod_q_shoup, uint64_t *delta,
                                     const phantom_ntt_tables *tables, size_t coeff_modulus_size,
                                     size_t start_modulus_idx, hipStream_t stream);
/* fnwt_1d / inwt_1d (include/ntt.cuh:157-169, src/ntt/ntt_1d.cu): the radix-2 single-workgroup path,
 * n = 2^3 .. 2^11 (the 2-D launchers above use it for n < 2^10).  inwt_1d multiplies by
 * scalar[limb] when scalar / scalar_shoup are given (device arrays, may be NULL). */
int phantom_fnwt_1d(uint64_t *inout, const phantom_ntt_tables *tables, size_t coeff_modulus_size,
                    size_t start_modulus_idx, hipStream_t stream);
int phantom_inwt_1d(uint64_t *inout, const phantom_ntt_tables *tables, size_t coeff_modulus_size,
                    size_t start_modulus_idx, const uint64_t *scalar, const uint64_t *scalar_shoup,
                    hipStream_t stream);

/* ---- context (PhantomContext, include/context.cuh:133-272; src/context.cu:121-232) ------ */
typedef struct phantom_context phantom_context;
/* moduli: the full key-level chain (data primes then special_modulus_size special primes),
 * as produced by CoeffModulus::Create; scheme is CKKS. */
int phantom_context_create(size_t poly_modulus_degree, const uint64_t *moduli, size_t count,
                           size_t special_modulus_size, phantom_context **out);
int phantom_context_destroy(phantom_context *ctx);
/* Opt-in extension, no reference counterpart: on != 0 makes every moddown (and moddown +
 * rescale) mean-unbiased by adding floor(ibase / 2) to each output coefficient (DESIGN.md §3,
 * "Where the precision goes"); 0 (the default) restores the reference's arithmetic bit for bit.
 * Also set by PHX_UNBIASED_MODDOWN=1 at phantom_context_create. */
int phantom_context_set_unbiased_moddown(phantom_context *ctx, int on);
/* number of data primes at chain_index (chain 0 = key level Q u P, 1 = Q, ...) */
size_t phantom_context_coeff_modulus_size(const phantom_context *ctx, size_t chain_index);

/* ---- CKKS evaluation on raw device ciphertexts --------------------------------------- */
/* tensor_prod_2x2_rns_poly (src/polymath.cu:501-536) via bgv_ckks_multiply (src/evaluate.cu:415-473):
 * ct1, ct2 are [2][L][n] at chain_index, out [3][L][n] (out may alias ct1's storage if sized for 3) */
int phantom_multiply(const phantom_context *ctx, size_t chain_index, const uint64_t *ct1, const uint64_t *ct2,
                     uint64_t *out, hipStream_t stream);
/* tensor_square_2x2_rns_poly (src/polymath.cu:538-582), the branch bgv_ckks_multiply takes when both
 * operands are the same ciphertext (src/evaluate.cu:443-450): ct [2][L][n] -> out [3][L][n] =
 * (c0^2, 2 c0 c1, c1^2); out may alias ct's storage if sized for 3 */
int phantom_square(const phantom_context *ctx, size_t chain_index, const uint64_t *ct, uint64_t *out,
                   hipStream_t stream);
/* relinearize_inplace (src/evaluate.cu:1552-1589) -> keyswitch_inplace (src/eval_key_switch.cu:112-212):
 * ct is [3][L][n]; on return its first two polys hold the relinearized ciphertext.
 * key_digits: host array of dnum device pointers, each a [2][size_QP][n] key digit. */
int phantom_relinearize(const phantom_context *ctx, size_t chain_index, uint64_t *ct,
                        const uint64_t *const *key_digits, size_t dnum, hipStream_t stream);
/* relinearize_inplace followed by rescale_to_next_inplace (src/evaluate.cu:1552-1589, 1591-1647) as
 * ONE division by P q_last (the bootstrap's EvalMult + ModReduce path): ct3 [3][L][n] at
 * chain_index -> out [2][L-1][n]; the inner product's first L-1 limbs are formed inside the
 * finish (NTT epilogue).  Equals moddown_from_NTT with {q_last} u P as the special basis applied
 * to the P-scaled extended (c0, c1) + KeySwitch(c2). */
int phantom_relinearize_rescale(const phantom_context *ctx, size_t chain_index, const uint64_t *ct3, uint64_t *out,
                                const uint64_t *const *key_digits, size_t dnum, hipStream_t stream);
/* `count` relinearize + rescale products (1 <= count <= 16) in shared launches: every stage of the key
 * switch (modup INTT, digit conversions, digit NTTs, moddown-rescale INTT, conversion, NTT + finish)
 * runs once over all of them.  Product k: ct3 + k ct3_stride ([3][L][n]) -> out + k out_stride
 * ([2][L-1][n]); bit-identical to phantom_relinearize_rescale on each.  The reference issues one
 * relinearize_inplace + rescale_to_next_inplace per product (src/evaluate.cu:1552-1647); EvalMod's
 * Chebyshev ladder and double angle (src/bootstrap.cu:1657-1668, src/evaluate.cu:3264-3535) run
 * their independent products this way.  Not in place: the output range
 * [out, out + (count - 1) out_stride + 2 (L-1) n) must not meet the ct3 range (rejected). */
int phantom_relinearize_rescale_batch(const phantom_context *ctx, size_t chain_index, const uint64_t *ct3,
                                      size_t ct3_stride, size_t count, uint64_t *out, size_t out_stride,
                                      const uint64_t *const *key_digits, size_t dnum, hipStream_t stream);
/* keyswitch_inplace core: ct [2][L][n] += KeySwitch(c2 [L][n]) */
int phantom_keyswitch(const phantom_context *ctx, size_t chain_index, uint64_t *ct, const uint64_t *c2,
                      const uint64_t *const *key_digits, size_t dnum, hipStream_t stream);
/* DRNSTool::modup (src/rns_bconv.cu:530-628): c2 [L][n] NTT form -> t_mod_up [beta][L+P][n] */
int phantom_modup(const phantom_context *ctx, size_t chain_index, const uint64_t *c2, uint64_t *t_mod_up,
                  hipStream_t stream);
/* key_switch_inner_prod (include/evaluate.cuh:27-29, src/eval_key_switch.cu:88-109) */
int phantom_keyswitch_inner_prod(const phantom_context *ctx, size_t chain_index, const uint64_t *t_mod_up,
                                 const uint64_t *const *key_digits, size_t dnum, uint64_t *cx, hipStream_t stream);
/* DBaseConverter::bConv_BEHZ (src/rns_bconv.cu:212-229; bconv_mult_unroll2_kernel :40-69 and
 * bconv_matmul_unroll2_kernel :143-179): dst[j] = sum_i [src_i * qHat_i^-1]_{q_i} * (qHat_i mod p_j)
 * mod p_j for coefficient-form src [ibase_size][n] -> dst [obase_size][n] (device arrays); ibase /
 * obase are host arrays of moduli.  prescale = 0 skips the [x * qHat^-1] step (src already scaled,
 * as the key-switch drivers pass it).  Builds the converter's tables and synchronizes `stream`
 * before returning (a test / one-off entry; the drivers keep converters per level). */
int phantom_fast_bconv(const uint64_t *ibase, size_t ibase_size, const uint64_t *obase, size_t obase_size,
                       const uint64_t *src, uint64_t *dst, size_t n, int prescale, hipStream_t stream);
/* A converter kept across calls, as the reference's DBaseConverter object (include/rns_bconv.cuh
 * DBaseConverter; init at src/rns_bconv.cu:10-38): phantom_bconv_create builds the tables once
 * (the matrix-core fragments included) from host moduli and synchronizes `stream`;
 * phantom_bconv_run is bConv_BEHZ (src/rns_bconv.cu:212-229) with the same meaning as
 * phantom_fast_bconv, asynchronous on `stream`, no allocation; phantom_bconv_destroy frees the
 * tables (the caller makes sure no run on them is still in flight). */
typedef struct phantom_bconv phantom_bconv;
int phantom_bconv_create(const uint64_t *ibase, size_t ibase_size, const uint64_t *obase, size_t obase_size,
                         hipStream_t stream, phantom_bconv **out);
int phantom_bconv_run(const phantom_bconv *conv, const uint64_t *src, uint64_t *dst, size_t n, int prescale,
                      hipStream_t stream);
int phantom_bconv_destroy(phantom_bconv *conv);
/* DRNSTool::moddown_from_NTT (src/rns_bconv.cu:791-843): cx_i [L+P][n] NTT form (P limbs clobbered)
 * -> out [L][n] = (cx_i - NTT(bconv(INTT(cx_i|P)))) * P^-1 */
int phantom_moddown_from_ntt(const phantom_context *ctx, size_t chain_index, uint64_t *cx_i, uint64_t *out,
                             hipStream_t stream);
/* Fused forms used by the bootstrap (no single reference function; each replaces a pair):
 * phantom_moddown_modup: moddown_from_NTT of one extended-basis polynomial followed by the modup of
 * its result (KeySwitchDown + EvalFastRotationPrecompute in EvalLinearTransform's giant steps,
 * src/bootstrap.cu:1335-1348) = modup(moddown(cx_i)) bit for bit.  cx_i [QlP][n] is clobbered;
 * t_mod_up [beta][QlP][n].
 * phantom_moddown_rescale: moddown_from_NTT followed by rescale_to_next as one division by
 * P q_last (the same algorithm with {q_last} u P as the dropped basis): cx [polys][QlP][n] at
 * chain_index (clobbered) -> out [polys][Ql-1][n]. */
int phantom_moddown_modup(const phantom_context *ctx, size_t chain_index, uint64_t *cx_i, uint64_t *t_mod_up,
                          hipStream_t stream);
/* phantom_moddown_modup over `count` independent polynomials in one launch per stage (the giant
 * steps of one linear-transform level, src/bootstrap.cu:1335-1348): polynomial i at
 * cx + i * cx_stride (elements, >= QlP n; clobbered), its digits at t_mod_up + i * beta * QlP * n. */
int phantom_moddown_modup_batch(const phantom_context *ctx, size_t chain_index, uint64_t *cx, size_t count,
                                size_t cx_stride, uint64_t *t_mod_up, hipStream_t stream);
int phantom_moddown_rescale(const phantom_context *ctx, size_t chain_index, uint64_t *cx, uint64_t *out,
                            size_t polys, hipStream_t stream);
/* ---- the bootstrap's own kernels (src/bootstrap.cu:1157-1405, src/evaluate.cu:2299-3940) ------
 * Extended-basis ("Ext") polynomials are [Ql + P][n] at chain_index: the chain's data limbs, then
 * the special primes; Ext ciphertexts are [2][Ql + P][n].  Host arrays carry device pointers or
 * per-limb residues (copied into the launch here). */
/* EvalLinearTransform's hoisted inner sums (src/bootstrap.cu:1322-1332: EvalMultExt +
 * EvalAddExtInPlace, src/evaluate.cu:3786-3874), all giant steps in one launch:
 * outs[i] = sum_{j<g} babies[j] * pts[i g + j] for i < b (babies / outs Ext ciphertexts, pts Ext
 * plaintexts, host arrays of device pointers; g a power of two <= 32, b <= 64) */
int phantom_lt_bsgs(const phantom_context *ctx, size_t chain_index, const uint64_t *const *babies, size_t g,
                    const uint64_t *const *pts, size_t b, uint64_t *const *outs, hipStream_t stream);
/* KeySwitchExt (src/evaluate.cu:3876-3940): ct [2][Ql][n] -> out = P ct in the Ext basis */
int phantom_keyswitch_ext(const phantom_context *ctx, size_t chain_index, const uint64_t *ct, uint64_t *out,
                          hipStream_t stream);
/* EvalFastRotationExt (src/evaluate.cu:3660-3755) with a fused key: inner product of the shared
 * modup digits [beta][Ql+P][n] with the key, + P c0 when add_first (ct's c0 [Ql][n]), then the
 * NTT-domain automorphism of both polynomials: out [2][Ql+P][n] */
int phantom_fast_rotation_ext(const phantom_context *ctx, size_t chain_index, const uint64_t *ct,
                              const uint64_t *digits, const uint64_t *const *key_digits, size_t dnum,
                              uint32_t galois_elt, int add_first, uint64_t *out, hipStream_t stream);
/* the baby steps of a hoisted linear transform in ONE launch (src/bootstrap.cu:1266-1276: the loop
 * of EvalFastRotationExt(.., digits, true) with KeySwitchExt for rotation 0): for k < count,
 * outs[k] [2][Ql+P][n] = phantom_fast_rotation_ext(ct's c0, digits, key_digits[k], galois_elts[k],
 * add_first = 1), or phantom_keyswitch_ext(ct) where key_digits[k] is NULL; ct [2][Ql][n], the
 * shared digits read once.  key_digits: host array of `count` host arrays of dnum device pointers */
int phantom_fast_rotation_ext_batch(const phantom_context *ctx, size_t chain_index, const uint64_t *ct,
                                    const uint64_t *digits, const uint64_t *const *const *key_digits, size_t dnum,
                                    const uint32_t *galois_elts, size_t count, uint64_t *const *outs,
                                    hipStream_t stream);
/* a giant step of the linear transforms (src/bootstrap.cu:1335-1348: KeySwitchDown + Precompute +
 * EvalFastRotationExt + EvalAddExtInPlace) with c0 kept in the Ext basis:
 * acc (+)= automorphism(KS(modup(moddown(ext c1))) + (ext c0, 0)); ext's c1 P limbs are clobbered */
int phantom_rotate_ext_accumulate(const phantom_context *ctx, size_t chain_index, uint64_t *ext,
                                  const uint64_t *const *key_digits, size_t dnum, uint32_t galois_elt, uint64_t *acc,
                                  int accumulate, hipStream_t stream);
/* ---- lockstep groups: `group` (2..8) ciphertexts of one level through the same keys / plaintexts in
 * ONE launch (a bootstrap batch, src/bootstrap.cu:1157-1405 run per ciphertext by the reference).
 * The ciphertexts' workgroups for the same elements run on one XCD, so the shared operand is read
 * from HBM about once per group; every result equals the single-ciphertext entry above on that
 * ciphertext, bit for bit.
 * phantom_lt_bsgs_group: phantom_lt_bsgs for ciphertext c with babies[c] + j baby_stride (words) as
 * baby j; inner sum 0 goes to acc[c], inner sum i >= 1 to giants[c] + (i - 1) giant_stride.
 * g must be 32 and b <= 8 (the bootstrap's CoeffToSlot / SlotToCoeff levels). */
int phantom_lt_bsgs_group(const phantom_context *ctx, size_t chain_index, size_t group,
                          const uint64_t *const *babies, size_t baby_stride, size_t g, const uint64_t *const *pts,
                          size_t b, uint64_t *const *acc, uint64_t *const *giants, size_t giant_stride,
                          hipStream_t stream);
/* phantom_fast_rotation_ext_batch for ciphertext c = (cts[c], digits[c]) with outputs
 * outs[c * count + k]; the entries (key_digits, galois_elts) are shared, and every ciphertext's outputs
 * must sit at the same offsets from its first output (outs[c * count + k] - outs[c * count]). */
int phantom_fast_rotation_ext_batch_group(const phantom_context *ctx, size_t chain_index, size_t group,
                                          const uint64_t *const *cts, const uint64_t *const *digits,
                                          const uint64_t *const *const *key_digits, size_t dnum,
                                          const uint32_t *galois_elts, size_t count, uint64_t *const *outs,
                                          hipStream_t stream);
/* phantom_rotate_ext_accumulate of ext[c] into acc[c] for c < group by the same rotation key */
int phantom_rotate_ext_accumulate_group(const phantom_context *ctx, size_t chain_index, size_t group,
                                        uint64_t *const *ext, const uint64_t *const *key_digits, size_t dnum,
                                        uint32_t galois_elt, uint64_t *const *acc, int accumulate,
                                        hipStream_t stream);
/* the EvalMod products' tensors in ONE launch (count <= 8 jobs at one level, L = Ql limbs each):
 * out[k] [3][L][n] = factors[k] (ct1[k] x ct2[k]), then out[k][p] += c[k] t[k][p] for p < 2 when t[k]
 * (t[k][p] at t[k] + p t_stride; c[k] host residues per limb), then out[k][0] += consts[k] when
 * consts[k] (host residues per limb); factors[k] >= 1 */
int phantom_tensor_lin_batch(const phantom_context *ctx, size_t chain_index, size_t count, const uint64_t *const *ct1,
                             const uint64_t *const *ct2, uint64_t *const *out, const uint64_t *factors,
                             const uint64_t *const *t, size_t t_stride, const uint64_t *const *c,
                             const uint64_t *const *consts, hipStream_t stream);
/* tensor_prod_2x2 with MulAddRescale's linear epilogue: out [3][Ql][n] = f (ct1 x ct2), then
 * out[p] += c t[p] for p < 2 (t[p] at t + p t_stride; f, c: host residues per limb or NULL) */
int phantom_tensor_lin(const phantom_context *ctx, size_t chain_index, const uint64_t *ct1, const uint64_t *ct2,
                       uint64_t *out, const uint64_t *f, const uint64_t *t, size_t t_stride, const uint64_t *c,
                       hipStream_t stream);
/* d[p] = d[p] ca (ca NULL: unscaled) + (p < t_polys ? t[p] cb : 0), d [d_polys][Ql][n] */
int phantom_lin_comb(const phantom_context *ctx, size_t chain_index, uint64_t *d, size_t d_polys, const uint64_t *ca,
                     const uint64_t *t, size_t t_polys, size_t t_stride, const uint64_t *cb, hipStream_t stream);
/* EvalMultConstInplaceCore / MultByIntegerInPlace in residue form (src/evaluate.cu:2299-2412,
 * :3942-3970): out[p] = in[p] c (+ acc[p]) for `polys` polynomials, in[p] at in + p in_stride
 * (0: contiguous) — a larger stride reads the leading Ql limbs of longer polynomials */
int phantom_mul_scalar(const phantom_context *ctx, size_t chain_index, const uint64_t *in, size_t in_stride,
                       const uint64_t *c, const uint64_t *acc, uint64_t *out, size_t polys, hipStream_t stream);
/* Chebyshev leaves of EvalChebyshevSeriesPS (src/evaluate.cu:3264-3535; EvalLinearWSumMutable
 * :3537-3600 + the free term): out[m] = sum_k in[k] coef[m][k] + (cadd[m], 0) for m < M, k < K
 * (in[k] [2][>= Ql][n] with polynomial stride in_stride[k]; coef host [M][K][Ql], cadd [M][Ql]) */
int phantom_leaf_combine(const phantom_context *ctx, size_t chain_index, const uint64_t *const *in,
                         const size_t *in_stride, size_t K, const uint64_t *coef, const uint64_t *cadd,
                         uint64_t *const *out, size_t M, hipStream_t stream);

/* ---- hoisted encrypted 2-D convolution (DNN::Conv, src/dnn.cu:82-150) --------------------------
 * A tensor is one ciphertext per channel: a width x width image sparse-packed in ns = Lg^2 slots,
 * Lg = width 2^slotstr, pixel (r, c) at slot (r Lg + c) 2^slotstr.  Weights are W[K][K][in_ch][out_ch]
 * doubles, row-major (the reference's weight[a][b][k][h]); a term is (h, k, a, b), b fastest.  The
 * reference runs per term one host sparse encode, one EvalRotateFused, one EvalMultAutoInplace and
 * one EvalAddAutoInplace (src/dnn.cu:99-141); here each input channel is raised once, its K^2
 * rotations stay in the Ext basis, and one launch forms the inner sums of a pass of output channels.
 * Refused with PHANTOM_ERR_INVALID_ARGUMENT before any launch: a null pointer, a count of 0, kernel
 * even or larger than width, width not a power of two, ns > N/2, a chain index of 0 or past the end,
 * no special prime, pt_scale <= 0. */
/* the K^2 tap rotations in tap order (a, b): ((a - K/2) Lg + (b - K/2)) 2^slotstr slots, 0 for the
 * centre tap (src/dnn.cu:114,122; AddRotationIndicesTo, :299-319).  Host only; *count = K^2 */
int phantom_conv_rotations(size_t width, size_t slotstr, size_t kernel, int *out, size_t capacity, size_t *count);
/* the masked slot vectors of `count` terms from first_term (src/dnn.cu:103-113, built on the host
 * there): dev_out [count][ns] complex as interleaved (re, 0); term (h, k, a, b) holds W[a][b][k][h]
 * at slot (r Lg + c) 2^slotstr for r, c < width with r + a - K/2 and c + b - K/2 in [0, width), 0
 * elsewhere.  The host twin fills host memory with the same layout. */
int phantom_conv_weight_slots(size_t width, size_t slotstr, size_t kernel, size_t in_ch, size_t out_ch,
                              const double *dev_W, size_t first_term, size_t count, double *dev_out,
                              hipStream_t stream);
int phantom_conv_weight_slots_host(size_t width, size_t slotstr, size_t kernel, size_t in_ch, size_t out_ch,
                                   const double *W, size_t first_term, size_t count, double *out);
/* general inner sums over the Ext basis (the EvalMultExt + EvalAddExtInPlace form of
 * src/evaluate.cu:3786-3874 for any number of terms; phantom_lt_bsgs stops at 32):
 * outs[o] (+)= sum_{t<T} ins[t] * pts[o T + t] for o < O; ins / outs host arrays of device pointers to
 * Ext ciphertexts, dev_pts a DEVICE table [O][T] of Ext plaintexts without null entries; accumulate
 * != 0 adds the value already in outs[o].  The 128-bit sums are reduced every 32 terms (65 products
 * of 61-bit residues overflow them), so the result is exact for every T. */
int phantom_ext_mac(const phantom_context *ctx, size_t chain_index, const uint64_t *const *ins, size_t T,
                    const uint64_t *const *dev_pts, size_t O, uint64_t *const *outs, int accumulate,
                    hipStream_t stream);
/* the whole layer on raw ciphertexts (src/dnn.cu:82-150): cts[k] [2][Ql][n] for k < in_ch ->
 * outs[h] [2][Ql][n] for h < out_ch, at the input's level; the result's scale is the input's times
 * pt_scale.  Per input channel phantom_modup of c1 and phantom_fast_rotation_ext_batch over the K^2
 * taps (key_digits[tap]: host array of dnum device pointers, NULL at the centre tap, which takes
 * phantom_keyswitch_ext; galois_elts[tap] its Galois element); per pass of `group` output channels
 * (0: chosen from a byte budget for the pass's plaintexts) phantom_conv_weight_slots,
 * phantom_ckks_encode (ext = 1, sparse_slots = ns, scale pt_scale; dev_overflow as there) and
 * phantom_ext_mac; then phantom_moddown_from_ntt of every output polynomial, batched.  The result
 * does not depend on group, bit for bit.  Enqueued on `stream`, scratch from the pool, not
 * synchronised (a rotation key seen for the first time is uploaded as in phantom_keyswitch). */
int phantom_conv2d(const phantom_context *ctx, size_t chain_index, const uint64_t *const *cts, size_t in_ch,
                   size_t out_ch, size_t width, size_t slotstr, size_t kernel, const double *dev_W, double pt_scale,
                   const uint64_t *const *const *key_digits, size_t dnum, const uint32_t *galois_elts, size_t group,
                   uint64_t *const *outs, int *dev_overflow, hipStream_t stream);
/* phantom_ext_mac over compact plaintexts (phantom_ckks_encode_sub): dev_pts[k] is [Ql + P][sub_degree]
 * and word e of a limb multiplies plaintext word e >> log2(N / sub_degree):
 *   outs[o][p][l][e] (+)= sum_{t<T} ins[t][p][l][e] * pts[o T + t][l][e >> log2(N / sub_degree)]  mod q_l.
 * The arithmetic is phantom_ext_mac's, exact for every T; sub_degree is a power of two in [1, N], and
 * sub_degree = N is phantom_ext_mac itself (full-size plaintexts, the same kernel). */
int phantom_ext_mac_sub(const phantom_context *ctx, size_t chain_index, const uint64_t *const *ins, size_t T,
                        const uint64_t *const *dev_pts, size_t sub_degree, size_t O, uint64_t *const *outs,
                        int accumulate, hipStream_t stream);
/* A prepared layer (the weights of src/dnn.cu:82-150 are fixed across inferences; the reference
 * encodes them per call with its sparse encoder, src/ckks.cu:180-270).  prepare runs
 * phantom_conv_weight_slots -> phantom_ckks_encode_sub (ext = 1, sub_slots = ns, scale pt_scale) for
 * all out_ch in_ch K^2 terms into one device allocation owned by the plan (8 out_ch in_ch K^2
 * (Ql + P) 2 ns bytes, phantom_conv_plan_bytes), waits for `stream`, and never reads dev_W again.
 * apply is phantom_conv2d with the plan in place of the weights: the modups and batched rotations,
 * ONE phantom_ext_mac_sub over all output channels, the batched moddown; enqueued in order, no
 * synchronisation, no encode.  Refused (status 1, outputs untouched): every shape phantom_conv2d
 * refuses, 2 ns < 8, a context other than the plan's, a null key at a tap other than the centre, a
 * null pointer.  phantom_conv_plan_destroy frees the plan; no apply may be in flight. */
typedef struct phantom_conv_plan phantom_conv_plan;
int phantom_conv2d_prepare(const phantom_context *ctx, size_t chain_index, size_t in_ch, size_t out_ch, size_t width,
                           size_t slotstr, size_t kernel, const double *dev_W, double pt_scale, int *dev_overflow,
                           hipStream_t stream, phantom_conv_plan **plan);
int phantom_conv_plan_bytes(const phantom_conv_plan *plan, size_t *bytes);
int phantom_conv_plan_destroy(phantom_conv_plan *plan);
int phantom_conv2d_apply(const phantom_context *ctx, const phantom_conv_plan *plan, const uint64_t *const *cts,
                         const uint64_t *const *const *key_digits, size_t dnum, const uint32_t *galois_elts,
                         uint64_t *const *outs, hipStream_t stream);
/* Batch norm, bias and the residual add fused into a prepared layer.  All three are affine in the
 * layer's output: the scale a_h is folded into the weights, and the two additions enter the inner
 * sum in the extended basis as P (m res_h + B_h), which is 0 modulo P and so passes through the
 * moddown exactly: the result is the unseeded entry's plus (m res_h + [polynomial 0] B_h) mod q_l,
 * word for word, at no extra level, launch or pass over memory.
 *   phantom_ext_mac_sub_seeded: phantom_ext_mac_sub (accumulate = 0) whose sum of output o,
 *     polynomial p, limb l < Ql starts at P (res[o][p][l][e] res_mult[l] + [p == 0] bias[o][l]) mod q_l
 *     and at 0 on the limbs of P.  res: host array [O] of device [2][Ql][N] ciphertexts (limb stride
 *     Ql; entries may be null, or res itself); res_mult: host [Ql], required with res; bias: host
 *     [O][Ql], or null.  All residues are taken modulo q_l here.
 *   phantom_conv2d_prepare_scaled: phantom_conv2d_prepare with the weights of output channel h
 *     multiplied by out_scale[h] (host [out_ch], null: 1.0) in FP64 on the device before the encode;
 *     dev_W is not modified.
 *   phantom_conv2d_apply_seeded: phantom_conv2d_apply with res (host [out_ch], at the plan's chain
 *     index), res_mult (host [Ql], m mod q_l) and bias (host [out_ch][Ql], B_h mod q_l) as above.
 *   phantom_scaled_constant_residues: round(value scale) mod moduli[i], i < count, on the host (no
 *     device is touched): the B_h of a bias at a scale that may exceed 2^64; a negative constant gives
 *     q - (|B| mod q).
 * Refused (status 1, outputs untouched): what the unseeded entries refuse, res without res_mult, an
 * out_scale that is not finite; a product that is not finite, a scale that is not positive, a zero
 * modulus. */
int phantom_ext_mac_sub_seeded(const phantom_context *ctx, size_t chain_index, const uint64_t *const *ins, size_t T,
                               const uint64_t *const *dev_pts, size_t sub_degree, size_t O, uint64_t *const *outs,
                               const uint64_t *const *res, const uint64_t *res_mult, const uint64_t *bias,
                               hipStream_t stream);
int phantom_conv2d_prepare_scaled(const phantom_context *ctx, size_t chain_index, size_t in_ch, size_t out_ch,
                                  size_t width, size_t slotstr, size_t kernel, const double *dev_W,
                                  const double *out_scale, double pt_scale, int *dev_overflow, hipStream_t stream,
                                  phantom_conv_plan **plan);
int phantom_conv2d_apply_seeded(const phantom_context *ctx, const phantom_conv_plan *plan, const uint64_t *const *cts,
                                const uint64_t *const *const *key_digits, size_t dnum, const uint32_t *galois_elts,
                                uint64_t *const *outs, const uint64_t *const *res, const uint64_t *res_mult,
                                const uint64_t *bias, hipStream_t stream);
/* the plan's plaintext words copied to host_out (capacity in words, at least phantom_conv_plan_bytes / 8);
 * waits for the device */
int phantom_conv_plan_read(const phantom_conv_plan *plan, uint64_t *host_out, size_t capacity);
int phantom_scaled_constant_residues(double value, double scale, const uint64_t *moduli, size_t count, uint64_t *out);

/* ---- hoisted average pooling + fully connected layer (DNN::AvgPoolFullCon, src/dnn.cu:397-452) ----
 * The reference pools each of the t input channels by 2 log2(width) sequential EvalRotateFused +
 * EvalAddAuto steps, then forms T t constant products and additions, then adds the bias.  Pooling and
 * the fully connected layer commute: here the channels are mixed first (t -> T, no key switch) and only
 * T ciphertexts are pooled, each raised once per direction, the width - 1 rotations of a direction
 * formed from the shared digits and summed in the Ext basis in one launch, then one moddown. */
/* linear combinations with per-limb scalars, any K >= 1 and M >= 1 (phantom_leaf_combine stops at
 * 16 x 8): outs[m] = sum_{k<K} ins[k] coef[m][k] + (cadd[m], 0) for m < M; ins / outs host arrays of
 * device pointers to [2][Ql][n] ciphertexts (no output may alias an input), coef host [M][K][Ql]
 * residues, cadd host [M][Ql] or NULL.  The 128-bit sums are reduced every 32 terms, so the result is
 * the exact residue for every K: phantom_mul_scalar + modular additions term by term, bit for bit.
 * Every input is read once per tile of up to 16 outputs (ceil(M / 16) times). */
int phantom_ct_mix(const phantom_context *ctx, size_t chain_index, const uint64_t *const *ins, size_t K,
                   const uint64_t *coef, const uint64_t *cadd, uint64_t *const *outs, size_t M, hipStream_t stream);
/* hoisted rotate-and-sum in ONE launch: out [2][Ql+P][n] = the modular sum over k < count (1..63) of
 * what phantom_fast_rotation_ext_batch writes for (key_digits[k], galois_elts[k]) with add_first = 1,
 * plus phantom_keyswitch_ext(ct) when identity != 0, bit for bit; the count Ext ciphertexts are never
 * written.  ct [2][Ql][n], digits [beta][Ql+P][n]; no key may be NULL; out must not alias ct / digits */
int phantom_rotate_sum_ext(const phantom_context *ctx, size_t chain_index, const uint64_t *ct, const uint64_t *digits,
                           const uint64_t *const *const *key_digits, size_t dnum, const uint32_t *galois_elts,
                           size_t count, int identity, uint64_t *out, hipStream_t stream);
/* the 2 (width - 1) pooling rotations, columns first: i 2^slotstr for i = 1..width-1, then
 * j Lg 2^slotstr for j = 1..width-1 (Lg = width 2^slotstr).  Host only.  The reference
 * (AddAvgPoolRotationsTo, src/dnn.cu:321-340) uses doubling steps and rotates rows by Lg 2^j, a row
 * step only when slotstr = 0; these are the correct amounts for every slotstr. */
int phantom_avgpool_rotations(size_t width, size_t slotstr, int *out, size_t capacity, size_t *count);
/* the whole layer on raw ciphertexts: cts[k] [2][Ql][n] for k < t -> outs[u] [2][Ql][n] for u < T at the
 * input's level.  In order: phantom_ct_mix (coef host [T][t][Ql], no cadd); per output phantom_modup
 * of c1 and phantom_rotate_sum_ext over the width - 1 column rotations with the identity; the batched
 * phantom_moddown_from_ntt of the 2 T polynomials; the same over the row rotations; cadd_bias (host
 * [T][Ql] residues) added to c0.  col_keys[i] / row_keys[i]: host arrays of dnum device pointers for
 * rotation i + 1 of the direction, col_elts / row_elts their Galois elements.  Enqueued on `stream`,
 * scratch from the pool, not synchronised (a rotation key seen for the first time is uploaded as in
 * phantom_keyswitch).  Refused with PHANTOM_ERR_INVALID_ARGUMENT before any launch: a null pointer,
 * t or T of 0, width not a power of two in 2..64, ns = Lg^2 > N/2, a chain index of 0 or past the end,
 * no special prime, a null key. */
int phantom_avgpool_fc(const phantom_context *ctx, size_t chain_index, const uint64_t *const *cts, size_t t, size_t T,
                       size_t width, size_t slotstr, const uint64_t *coef, const uint64_t *cadd_bias,
                       const uint64_t *const *const *col_keys, const uint64_t *const *const *row_keys, size_t dnum,
                       const uint32_t *col_elts, const uint32_t *row_elts, uint64_t *const *outs, hipStream_t stream);

/* ---- serialization (host memory; no GPU involved) ------------------------------------
 * The byte format of PhantomCiphertext::save / load (include/ciphertext.h:184-225): the header
 * fields one by one (4 x size_t, double, uint64_t, size_t, bool, bool = 58 bytes) followed by
 * size * coeff_modulus_size * poly_modulus_degree uint64_t words. */
typedef struct phantom_ct_header {
  uint64_t chain_index, size, poly_modulus_degree, coeff_modulus_size;
  double scale;
  uint64_t correction_factor, noise_scale_deg;
  int is_ntt_form, is_asymmetric;
} phantom_ct_header;
/* writes the header and data (host) to out[capacity]; *written = bytes (needed size when too small) */
int phantom_ciphertext_serialize(const phantom_ct_header *h, const uint64_t *host_data, uint8_t *out,
                                 size_t capacity, size_t *written);
/* PhantomGaloisKey::save (include/secretkey.h:195-205) of host words (host only, no GPU):
 * host_keys = [count][dnum][2][size_QP][n]; writes count, then per key dnum and dnum key-level
 * ciphertexts (chain 0, size 2, n, size_QP, scale 1, correction 1, degree 1, NTT form, symmetric) */
int phantom_galois_key_serialize(size_t n, size_t size_QP, size_t dnum, size_t count, const uint64_t *host_keys,
                                 uint8_t *out, size_t capacity, size_t *written);
/* parses in[len]; copies the words to host_data[capacity_words] (may be null: header only);
 * *words = the ciphertext's word count */
int phantom_ciphertext_deserialize(const uint8_t *in, size_t len, phantom_ct_header *h, uint64_t *host_data,
                                   size_t capacity_words, size_t *words);

/* rescale_to_next (src/evaluate.cu:1779-1801) -> divide_and_round_q_last_ntt (src/rns.cu:1160-1184):
 * in [polys][L][n] at chain_index -> out [polys][L-1][n] */
int phantom_rescale_to_next(const phantom_context *ctx, size_t chain_index, const uint64_t *in, uint64_t *out,
                            size_t polys, hipStream_t stream);
/* apply_galois_ntt (src/galois.cu:104-119) with the PrecomputeAutoMapKernel table (src/util.cu:941-958);
 * out must not alias in (PHANTOM_ERR_INVALID_ARGUMENT) */
int phantom_apply_galois_ntt(const phantom_context *ctx, uint32_t galois_elt, const uint64_t *in, uint64_t *out,
                             size_t coeff_modulus_size, hipStream_t stream);
/* elementwise ops over limbs [limb_offset, limb_offset + L) of the key-level chain
 * (add_rns_poly / sub_rns_poly / multiply_rns_poly / negate, src/polymath.cu) */
#define PHANTOM_POLY_ADD 0
#define PHANTOM_POLY_SUB 1
#define PHANTOM_POLY_MUL 2
#define PHANTOM_POLY_NEGATE 3
int phantom_poly_op(const phantom_context *ctx, int op, const uint64_t *a, const uint64_t *b, uint64_t *out,
                    size_t limb_offset, size_t coeff_modulus_size, hipStream_t stream);
/* switchModulusKernel as used by RaiseMod (src/evaluate.cu:2414-2503): coefficient-form limb 0
 * lifted to L limbs (centered representative of the q0 residue) */
int phantom_switch_modulus_raise(const phantom_context *ctx, const uint64_t *in_q0, uint64_t *out,
                                 size_t coeff_modulus_size, hipStream_t stream);

/* ---- CKKS encode / decode on the device (PhantomCKKSEncoder, src/ckks.cu:45-521) --------------
 * Slot j sits at the root zeta^(5^j) of X^N + 1 and its conjugate at zeta^(-5^j).  Complex data is
 * interleaved (re, im) doubles; plaintexts are [limbs][n] words, `count` of them back to back.
 * Everything is enqueued on `stream`; scratch comes from the engine's pool on that stream.  Bad
 * arguments (scale <= 0, too many values, a sparse slot count that is no power of two <= N/2, a
 * chain index past the end, ext at chain 0) return PHANTOM_ERR_INVALID_ARGUMENT before any launch.
 * dev_overflow (device int, may be NULL) is set non-zero, never cleared, when some value times the
 * scale is not finite or reaches 2^1000 (the host encoder's "encoded values are too large"); the
 * residues written are then unspecified. */
/* The canonical embedding alone, in FP64: the special FFT pair of src/fft.cu:651-815
 * (special_fft_backward / special_fft_forward, called at src/ckks.cu:143, 509) as one size-N transform.  ns = sparse_slots, or N/2 when 0.
 * forward == 0: in [count][ns] complex -> out [count][N] real coefficients, 1/N included, not
 * scaled; the ns values fill every block of ns slots (set_sparse_encode, include/ckks.h:82-117).
 * forward != 0: in [count][N] reals -> out [count][ns] complex, the first ns slots. */
int phantom_ckks_embed(const phantom_context *ctx, int forward, const double *in, double *out, size_t sparse_slots,
                       size_t count, hipStream_t stream);
/* decompose_array (src/rns_base.cu:49-170; called at src/ckks.cu:171, 348):
 * out[p][i][k] = round_half_even(coeffs[p][k] * scale) mod q_i (negative values as q_i - v), exact
 * for every product below 2^1000, over the Ql basis of chain_index, followed by the special primes
 * when ext != 0 (encode_internal_ext, src/ckks.cu:276-353); ntt_form != 0 applies the forward NTT
 * (src/ckks.cu:174, 350). */
int phantom_ckks_round_rns(const phantom_context *ctx, size_t chain_index, int ext, const double *coeffs, double scale,
                           size_t count, int ntt_form, uint64_t *out, int *dev_overflow, hipStream_t stream);
/* compose_array (src/rns_base.cu:173-260) after the inverse NTT (src/ckks.cu:494-499): plain_ntt
 * [count][Ql][N] (NTT form, not modified) -> coeffs [count][N], the centred integer in (-Q/2, Q/2]
 * of each coefficient as a double (exact below 2^53, else within one ulp of correct rounding), not
 * divided by the scale.  chain_index >= 1. */
int phantom_ckks_compose(const phantom_context *ctx, size_t chain_index, const uint64_t *plain_ntt, size_t count,
                         double *coeffs, hipStream_t stream);
/* PhantomCKKSEncoder::encode_internal (src/ckks.cu:103-178): values [count][num_values] complex
 * (num_values <= ns, zero-padded) -> out [count][limbs][N], NTT form */
int phantom_ckks_encode(const phantom_context *ctx, size_t chain_index, int ext, const double *values,
                        size_t num_values, size_t sparse_slots, double scale, size_t count, uint64_t *out,
                        int *dev_overflow, hipStream_t stream);
/* The compact sparse encoder (the reference's sparse path, src/ckks.cu:180-270: a size-ns FFT,
 * decompose_array over 2 ns coefficients, extend_sparse_ckks).  With M = 2 sub_slots and g = N / M, a
 * plaintext p(X) = p'(X^g) has NTT_N(p)[i] = NTT'_M(p')[i >> log2 g] in the engine's bit-reversed
 * order, NTT'_M the size-M negacyclic transform with root psi_N^g (its twiddles are the first M
 * entries of the size-N table), so p' alone is kept: values [count][num_values] complex (num_values
 * <= sub_slots, zero-padded) -> out [count][limbs][M], the size-M inverse embedding, the round and
 * split over M coefficients and NTT'_M.  sub_slots = N/2 gives phantom_ckks_encode bit for bit.
 * phantom_sub_ntt is NTT'_M (inverse != 0: its exact inverse, M^-1 included) in place on data
 * [count][limbs][sub_degree].  Refused (status 1, nothing enqueued): a subring degree that is not a
 * power of two in [8, N], a bad chain index, a null pointer, scale <= 0. */
int phantom_ckks_encode_sub(const phantom_context *ctx, size_t chain_index, int ext, const double *values,
                            size_t num_values, size_t sub_slots, double scale, size_t count, uint64_t *out,
                            int *dev_overflow, hipStream_t stream);
int phantom_sub_ntt(const phantom_context *ctx, size_t chain_index, int ext, size_t sub_degree, int inverse,
                    uint64_t *data, size_t count, hipStream_t stream);
/* PhantomCKKSEncoder::decode_internal (src/ckks.cu:456-521): plain [count][Ql][N] (NTT form, not
 * modified) -> values [count][N/2] complex = embedding(centred coefficients / scale) */
int phantom_ckks_decode(const phantom_context *ctx, size_t chain_index, const uint64_t *plain, double scale,
                        size_t count, double *values, hipStream_t stream);

/* ---- the bootstrap's linear-transform diagonals on the device (EvalBootstrapSetup's precompute,
 * src/bootstrap.cu:181-560; this engine's slot-domain butterfly stages) --------------
 * Diagonals are complex vectors of interleaved (re, im) doubles; a band is [D][ns] of them with D
 * sorted offsets on ns slots.  The device entry points enqueue on `stream`; the small tables they
 * need are uploaded before the first launch (one wait for `stream`).  ns not a power of two >= 2
 * (or above N/2), a stage outside 1 .. log2 ns, a null pointer or a capacity too small return
 * PHANTOM_ERR_INVALID_ARGUMENT before anything is enqueued.  Each *_host twin runs the host code of
 * the setup (boot::stage / compose / lift_blocks and the pre-rotation) and returns the same layout. */
/* offsets of compose(stage(s_k), .. compose(stage(s_1), I)) on ns slots: set arithmetic alone
 * (each stage adds {0, +h, -h mod ns}, h = 2^(s-1)); sorted, *count of them (host only) */
int phantom_ltprep_stage_offsets(size_t ns, const int *stages, size_t num_stages, int *offsets, size_t capacity,
                                 size_t *count);
/* the diagonals of that product (inverse: the stages of the inverse map, as CoeffToSlot uses them)
 * to dev_out [count][ns]; dev_scratch holds capacity_diagonals x ns complex values like dev_out.
 * Twiddles are the context's embedding roots; the values equal the host twin's. */
int phantom_ltprep_stage_products(const phantom_context *ctx, size_t ns, int inverse, const int *stages,
                                  size_t num_stages, double *dev_out, double *dev_scratch, size_t capacity_diagonals,
                                  hipStream_t stream);
int phantom_ltprep_stage_products_host(size_t ns, int inverse, const int *stages, size_t num_stages, double *out,
                                       size_t capacity_diagonals);
/* dev_flags [2 D] (cleared here): [2 i] = band[i] times the constant (when apply_const) has a
 * non-zero entry at some r with r + offsets[i] < ns, [2 i + 1] = at some r with r + offsets[i] >= ns */
int phantom_ltprep_presence(const double *dev_band, size_t ns, const int *offsets, size_t num_diagonals, double c_re,
                            double c_im, int apply_const, int *dev_flags, hipStream_t stream);
/* offsets on n slots of the block-periodic lift (ns < n: offset a where flags[2 i], a - ns mod n
 * where flags[2 i + 1]; ns == n: a where either), sorted (host only) */
int phantom_ltprep_lifted_offsets(const int *offsets, const int *flags, size_t num_diagonals, size_t ns, size_t n,
                                  int *keys, size_t capacity, size_t *count);
/* baby-step giant-step shape of a level with those offsets (host only):
 * shape = {stride, center, D, g, b}; dim1 = 0 picks g */
int phantom_ltprep_shape(size_t n, const int *keys, size_t num_keys, int stride, uint32_t dim1, int *shape);
/* the level's slot vectors, ready for phantom_ckks_encode: constant (full complex multiply, when
 * apply_const), lift to n slots (ns < n; mask 0 none, 1 the CoeffToSlot output mask {1, -i}, 2 the
 * SlotToCoeff input mask {1, i}, period 2 ns), giant-step pre-rotation.  dev_out [num_keys][n] in
 * slot order, slots_out[num_keys] (host) = each one's slot u, offset (u - center) stride. */
int phantom_ltprep_finish(const double *dev_band, size_t ns, size_t n, const int *band_offsets, size_t num_band,
                          const int *keys, size_t num_keys, const int *shape, double c_re, double c_im,
                          int apply_const, int mask, double *dev_out, int *slots_out, hipStream_t stream);
/* host twin of presence + lifted_offsets + shape + finish from a host band: *count diagonals,
 * keys_out / slots_out [capacity], out [capacity][n] (may be NULL: structure only) */
int phantom_ltprep_finish_host(const double *band, size_t ns, size_t n, const int *band_offsets, size_t num_band,
                               double c_re, double c_im, int apply_const, int mask, int stride, uint32_t dim1,
                               int *shape, int *keys_out, int *slots_out, size_t capacity, size_t *count, double *out);
/* diagonals of a dense row-major slots x slots device matrix (ExtractShiftedDiagonal, src/util.cu:298-312):
 * dev_out[k][p] = A[p][(p + k) mod slots] * scale, dev_flags[k] (cleared here) = diagonal k has a
 * non-zero entry */
int phantom_ltprep_dense_diagonals(const double *dev_A, size_t slots, double scale, double *dev_out, int *dev_flags,
                                   hipStream_t stream);

/* ---- bootstrapping sessions (bootstrapping/bootstrapping_example.cu:69-160; src/bootstrap.cu) ----
 * A session is the SimpleBootstrapExample set-up as one object: N = 2^log_n, Q = {60, depth x 59},
 * P = special x 60 (CoeffModulus::Create), scale 2^59, levelBudget {enc, dec}, num_slots slots
 * (0 = N/2; a smaller power of two = sparse packing, SparseBootStrapping :200-309), numIterations
 * and precision of EvalBootstrap (src/bootstrap.cu:843-900).  Keys are derived from the 32-byte
 * secret `seed`: every rank of a multi-GPU job that passes the same seed regenerates the same keys,
 * so no key crosses the interconnect.
 * Ciphertexts cross this boundary serialized in PhantomCiphertext::save's byte format
 * (include/ciphertext.h:184-225) and held in DEVICE memory, `stride` bytes apart: the form in which
 * a batch is scattered to ranks and gathered back. */
/* algorithmic HBM bytes of the homomorphic operations issued since the last reset (process-wide,
 * host/traffic.h): out[0] key-switching key bytes, out[1] linear-transform plaintext bytes,
 * out[2] ciphertext operand / result bytes — the numerator of the bootstrap's roofline */
int phantom_traffic_read(uint64_t *out);
int phantom_traffic_reset(void);
/* The engine's device allocator (host/buffer.h DevicePool, the reference's cudaMallocAsync pool with
 * an unbounded release threshold, src/context.cu:127-131): out[0] bytes held from the driver,
 * out[1] bytes live (handed out), out[2] peak live and out[3] peak held since the last reset. */
int phantom_pool_stats(uint64_t *out);
int phantom_pool_reset_peak(void);
/* EvalMod's Chebyshev interpolant (host only): out[degree + 1] = coefficients c of
 * (2 pi)^(-2^-r) cos(2 pi (K y - 1/4) / 2^r) on [-1, 1], r = double_angle_iterations, with
 * p(y) = sum_k c_k T_k(y) (c_0 NOT halved; the reference's tables g_coefficientsUniform/Sparse,
 * include/bootstrap.cuh:217-255, hold 2 c_0 first) */
int phantom_eval_mod_coefficients(uint32_t K, uint32_t double_angle_iterations, int degree, double *out);
typedef struct phantom_boot_session phantom_boot_session;
int phantom_boot_session_create(int log_n, int depth, int special, const uint32_t *level_budget, uint32_t num_slots,
                                uint32_t num_iterations, uint32_t precision, const uint8_t *seed,
                                phantom_boot_session **out);
/* phantom_boot_session_create with a flags word: PHANTOM_BOOT_DEVICE_SETUP builds the
 * linear-transform plaintexts on the device (FHECKKSRNS::UseDeviceSetup); unknown bits are refused */
#define PHANTOM_BOOT_DEVICE_SETUP 1u
int phantom_boot_session_create_opts(int log_n, int depth, int special, const uint32_t *level_budget,
                                     uint32_t num_slots, uint32_t num_iterations, uint32_t precision,
                                     const uint8_t *seed, uint32_t flags, phantom_boot_session **out);
int phantom_boot_session_destroy(phantom_boot_session *s);
/* encrypt `count` vectors of num_slots reals (values[count][num_slots]) at chain_index with that
 * level's FLEXIBLEAUTO scale; *ct_bytes = the size of one serialized ciphertext */
int phantom_boot_encrypt(phantom_boot_session *s, const double *values, size_t count, size_t chain_index,
                         uint8_t *dev_out, size_t stride, size_t *ct_bytes);
/* size of one serialized bootstrap output */
int phantom_boot_output_bytes(phantom_boot_session *s, size_t *bytes);
/* the same sizes from the session parameters alone (host only, no GPU): one serialized input at
 * chain_index, one serialized output, and the output's chain index */
int phantom_boot_layout(int log_n, int depth, int special, const uint32_t *level_budget, uint32_t num_slots,
                        uint32_t num_iterations, size_t chain_index, size_t *in_bytes, size_t *out_bytes,
                        size_t *out_chain);
/* EvalBootstrap of `count` serialized ciphertexts, `lanes` side by side (EvalBootstrapBatch) */
int phantom_boot_run(phantom_boot_session *s, const uint8_t *dev_in, size_t in_stride, size_t count, uint8_t *dev_out,
                     size_t out_stride, int lanes);
/* phantom_boot_run with each lane bootstrapping `group` ciphertexts (1..8) at a time in lockstep
 * (phantom_boot_run uses 4; 8 is ~1.5% faster at C5 for ~80 GiB more device memory) */
int phantom_boot_run_grouped(phantom_boot_session *s, const uint8_t *dev_in, size_t in_stride, size_t count,
                             uint8_t *dev_out, size_t out_stride, int lanes, int group);
/* decrypt + decode one serialized ciphertext: the real parts of its num_slots slots */
int phantom_boot_decrypt(phantom_boot_session *s, const uint8_t *dev_in, size_t capacity, double *values_out);
/* phantom_boot_encrypt from DEVICE values [count][num_slots] interleaved complex, through the device
 * encoder and one batched encryption (phantom_encrypt_symmetric_batch with the session's key): the
 * same serialized byte format, header and metadata.  dev_values must be complete when the call is
 * made; the call returns after the session's stream has written everything (one synchronisation). */
int phantom_boot_encrypt_device(phantom_boot_session *s, const double *dev_values, size_t count, size_t chain_index,
                                uint8_t *dev_out, size_t stride, size_t *ct_bytes);
/* `count` serialized ciphertexts `stride` bytes apart, of one chain index, size and scale ->
 * dev_values_out [count][num_slots] interleaved complex, decoded from the two leading limbs as
 * phantom_boot_decrypt does.  The headers are validated on the host (one synchronisation); the
 * values are written in the order of the session's stream: synchronise the device before another
 * stream reads them or reuses dev_in. */
int phantom_boot_decrypt_device(phantom_boot_session *s, const uint8_t *dev_in, size_t stride, size_t count,
                                double *dev_values_out);

/* ---- random sampling (src/prng.cu; seeds: include/prng.cuh:13-24) ---------------------
 * Every draw of key generation and encryption is ChaCha20 keystream (RFC 8439 block function,
 * 64-bit block counter in state words 12-13, 64-bit nonce in words 14-15): draw `nonce` of the
 * stream keyed by key[8].  The reference samples from Salsa20 seeded by std::random_device. */
/* out[16] = ChaCha20 block (host only, no GPU) */
int phantom_chacha20_block(const uint32_t *key, uint64_t counter, uint64_t nonce, uint32_t *out);
/* device polynomial [coeff_modulus_size][n] over the first limbs of the key-level chain:
 *   PHANTOM_SAMPLE_UNIFORM: element e = 128-bit keystream word pair e mod q (sample_uniform_poly)
 *   PHANTOM_SAMPLE_CBD:     centered binomial 21+21 bits of 64-bit word k (sample_error_poly)
 *   PHANTOM_SAMPLE_TERNARY: 64-bit word k mod 3 minus 1 (sample_ternary_poly)
 * the last two write the same signed value to every limb (coefficient form). */
/* the reference's Salsa20 block (src/prng.cu:17-140; host only): seed[64], nonce -> out[16] */
int phantom_salsa20_block(const uint8_t *seed, uint64_t nonce, uint32_t *out);
/* the reference's uniform expansion of a public 64-byte seed (sample_uniform_poly,
 * src/prng.cu:164-197): `a` of a seed-compressed symmetric ciphertext, [coeff_modulus_size][n]
 * over the first limbs of the key-level chain, bit for bit as the reference */
int phantom_sample_uniform_seeded(const phantom_context *ctx, const uint8_t *seed, uint64_t *out,
                                  size_t coeff_modulus_size, hipStream_t stream);
#define PHANTOM_SAMPLE_UNIFORM 0
#define PHANTOM_SAMPLE_CBD 1
#define PHANTOM_SAMPLE_TERNARY 2
int phantom_sample_poly(const phantom_context *ctx, int kind, const uint32_t *key, uint64_t nonce, uint64_t *out,
                        size_t coeff_modulus_size, hipStream_t stream);

/* ---- batched symmetric encryption / decryption on the device (encrypt_symmetric_internal and
 * ckks_decrypt, src/secretkey.cu:576-682, for a whole batch) ------------------------------------
 * Values in device memory -> ciphertexts -> values in device memory with explicit key material: a
 * fixed number of launches per internal chunk of ciphertexts, everything enqueued on `stream`,
 * scratch from the engine's pool on that stream, no synchronisation.  Each result equals the
 * one-at-a-time composition of the entries above bit for bit.  dev_sk is the secret in NTT form
 * over rows 0 .. L-1 of the key-level chain ([>= L][N]).  Ciphertexts are [polys][L][N] words and
 * start 16-byte aligned, an even number of words apart.  Bad arguments (a null pointer, count == 0,
 * a chain index of 0 or past the end, limbs > ct_limbs, polys outside 2..3, a stride smaller than
 * one ciphertext or odd, and whatever phantom_ckks_encode refuses) return
 * PHANTOM_ERR_INVALID_ARGUMENT before any launch. */
/* dev_out [count][N] small signed: e_p[k] = the centered binomial (PHANTOM_SAMPLE_CBD's value) of
 * draw nonces[p] (host array) of the stream keyed by key[8] */
int phantom_sample_cbd_small_batch(const phantom_context *ctx, const uint32_t *key, const uint64_t *nonces,
                                   size_t count, int32_t *dev_out, hipStream_t stream);
/* dev_values [count][num_values] complex (as phantom_ckks_encode) -> ciphertext p = (c0, c1), NTT form,
 * at dev_out + p * out_stride words (0 = 2 L N): c1 = phantom_sample_uniform_seeded(seeds + 64 p),
 * c0 = m - (c1 s + e) with e of draw nonces[p].  seeds [count][64] and nonces [count] are host arrays,
 * read before the call returns.  dev_overflow as phantom_ckks_encode's. */
int phantom_encrypt_symmetric_batch(const phantom_context *ctx, size_t chain_index, const uint64_t *dev_sk,
                                    const double *dev_values, size_t num_values, size_t sparse_slots, double scale,
                                    size_t count, const uint32_t *key, const uint64_t *nonces, const uint8_t *seeds,
                                    uint64_t *dev_out, size_t out_stride, int *dev_overflow, hipStream_t stream);
/* `count` ciphertexts of `polys` polynomials with ct_limbs limbs each, in_stride words apart (0 =
 * polys ct_limbs N) -> dev_plain [count][limbs][N] = c0 + c1 s (+ c2 s^2), NTT form, over the
 * leading limbs <= ct_limbs limbs (dropping limbs of a decryption is exact) */
int phantom_decrypt_batch(const phantom_context *ctx, const uint64_t *dev_sk, const uint64_t *dev_in, size_t in_stride,
                          size_t polys, size_t ct_limbs, size_t limbs, size_t count, uint64_t *dev_plain,
                          hipStream_t stream);
/* the same followed by phantom_ckks_decode over those limbs (limbs <= the data primes):
 * dev_values [count][N/2] complex */
int phantom_decrypt_decode_batch(const phantom_context *ctx, const uint64_t *dev_sk, const uint64_t *dev_in,
                                 size_t in_stride, size_t polys, size_t ct_limbs, size_t limbs, size_t count,
                                 double scale, double *dev_values, hipStream_t stream);
/* host only: ciphertexts per internal chunk at this chain index */
int phantom_encrypt_batch_chunk(const phantom_context *ctx, size_t chain_index, size_t *chunk);

/* ---- batched public-key encryption on the device (encrypt_zero_asymmetric_internal and
 * encrypt_asymmetric, src/secretkey.cu:12-185, for a whole batch) ----------------------------------
 * Values in device memory -> ciphertexts with explicit key material, under the conventions of the
 * symmetric block above: a fixed number of launches per internal chunk, everything enqueued on
 * `stream`, scratch from the engine's pool on that stream, no synchronisation.  Each result equals
 * the one-at-a-time composition of the entries above bit for bit (phantom_sample_poly TERNARY / CBD
 * over the whole key-level chain, phantom_nwt_forward_inplace, phantom_poly_op against the key,
 * phantom_moddown_from_ntt, + phantom_ckks_encode), while only the L data rows and the special rows
 * of the chain are ever formed.  dev_pk is the public key (-(a s + e), a) in NTT form over the whole
 * key-level chain ([2][size_QP][N]), 16-byte aligned; the context needs at least one special prime.
 * Bad arguments (those of the symmetric block, and a misaligned dev_pk) return
 * PHANTOM_ERR_INVALID_ARGUMENT before any launch. */
/* dev_out [count][N] small signed: the value of draw nonces[p] (host array) of the stream keyed by
 * key[8], kind PHANTOM_SAMPLE_CBD (phantom_sample_cbd_small_batch's) or PHANTOM_SAMPLE_TERNARY */
int phantom_sample_small_batch(const phantom_context *ctx, int kind, const uint32_t *key, const uint64_t *nonces,
                               size_t count, int32_t *dev_out, hipStream_t stream);
/* dev_values [count][num_values] complex (as phantom_ckks_encode) -> ciphertext p = (c0, c1), NTT form,
 * at dev_out + p * out_stride words (0 = 2 L N): (pk0 u + e0, pk1 u + e1) divided by the special
 * primes, + m on c0, with the ternary u and the centered binomial e0, e1 of the draws nonces[3 p],
 * nonces[3 p + 1], nonces[3 p + 2].  nonces [count][3] is a host array, read before the call returns.
 * dev_overflow as phantom_ckks_encode's. */
int phantom_encrypt_asymmetric_batch(const phantom_context *ctx, size_t chain_index, const uint64_t *dev_pk,
                                     const double *dev_values, size_t num_values, size_t sparse_slots, double scale,
                                     size_t count, const uint32_t *key, const uint64_t *nonces, uint64_t *dev_out,
                                     size_t out_stride, int *dev_overflow, hipStream_t stream);
/* host only: ciphertexts per internal chunk at this chain index */
int phantom_encrypt_asymmetric_batch_chunk(const phantom_context *ctx, size_t chain_index, size_t *chunk);

/* ---- channel packing for the tensor bootstrap (host/pack.h) -------------------------------------
 * A sparse-packed channel of ns = (width 2^slotstr)^2 slots is a polynomial in X^(N / (2 ns)), so
 * pack <= min(N / (2 ns), 64) channels (a power of two) are interleaved into one ciphertext by
 * monomial shifts, packed = sum_c X^(c D) ct_c with D = N / (2 pack ns); one bootstrap at pack ns
 * slots refreshes them all and a binary tree of rotations takes them apart: level t rotates every
 * node a by rotations[t] = pack ns / 2^(t+1) slots and forms a + rot and (a - rot) X^(2N - powers[t]),
 * powers[t] = D 2^t.  Ciphertexts are [2][L][N] words, NTT form, 16-byte aligned.  Bad arguments
 * (a null pointer, C or count of 0 or above 64, a power >= 2N, a chain index of 0 or past the end, a
 * misaligned ciphertext, an output overlapping an input other than even[k] == a[k]) return
 * PHANTOM_ERR_INVALID_ARGUMENT before any launch. */
/* host only: the log2(pack) tree levels for ring degree 2^log_n: rotations (slots), their Galois
 * elements 5^r mod 2N and the shifts D 2^t the odd children undo (each array may be null); *count is set
 * even when capacity is too small.  Refused: a width that is no power of two, a pack that is no
 * power of two or above min(N / (2 ns), 64), an image that does not fit N / 2 slots. */
int phantom_pack_rotations(size_t width, size_t slotstr, size_t pack, size_t log_n, int *rotations,
                           uint32_t *galois_elts, uint32_t *powers, size_t capacity, size_t *count);
/* out = sum_{c < C} X^(c stride_power) ins[c] (ins: host array of C device pointers) in one launch
 * that reads every input once */
int phantom_ct_pack(const phantom_context *ctx, size_t chain_index, const uint64_t *const *ins, size_t C,
                    uint32_t stride_power, uint64_t *out, hipStream_t stream);
/* one tree level of `count` nodes in one launch: even[k] = a[k] + r[k], odd[k] = (a[k] - r[k]) X^(2N - power)
 * (host arrays of device pointers; even[k] or odd[k] may be null, and one of the two arrays too) */
int phantom_ct_split(const phantom_context *ctx, size_t chain_index, const uint64_t *const *a,
                     const uint64_t *const *r, size_t count, uint32_t power, uint64_t *const *even,
                     uint64_t *const *odd, hipStream_t stream);
/* ---- batched same-key rotations: `count` ciphertexts of one level through ONE Galois key (the
 * levels of the unpacking tree; "rotate every channel by r" of a tensor).  cts, digits and outs are
 * host arrays of device pointers, 16-byte aligned; key_digits as phantom_fast_rotation_ext's.  Each
 * result equals the one-ciphertext entries' bit for bit.  Rejected with an error code before any
 * launch: a null pointer, a bad chain index, a dnum below beta, a misaligned buffer, any output
 * overlapping any input or another output, and a count of 0 or above 64 for the kernel entry. */
/* the key switch alone, one launch with the key read once: outs[k] [2][Ql+P][n] =
 * phantom_fast_rotation_ext(cts[k], digits[k], key_digits, galois_elt, add_first = 1) for k < count
 * (1..64); cts[k] [2][Ql][n] (its c0 is read), digits[k] [beta][Ql+P][n] */
int phantom_keyswitch_rotate_many(const phantom_context *ctx, size_t chain_index, size_t count,
                                  const uint64_t *const *cts, const uint64_t *const *digits,
                                  const uint64_t *const *key_digits, size_t dnum, uint32_t galois_elt,
                                  uint64_t *const *outs, hipStream_t stream);
/* the whole rotation, outs[k] [2][Ql][n] = moddown(keyswitch_rotate(modup(cts[k] c1))) of cts[k]
 * [2][Ql][n], for any count >= 0: per chunk of phantom_rotate_fused_batch_chunk ciphertexts one batched
 * phantom_modup, one phantom_keyswitch_rotate_many and one phantom_moddown_from_ntt over 2 count
 * polynomials; no synchronisation, scratch from the pool */
int phantom_rotate_fused_batch(const phantom_context *ctx, size_t chain_index, size_t count,
                               const uint64_t *const *cts, const uint64_t *const *key_digits, size_t dnum,
                               uint32_t galois_elt, uint64_t *const *outs, hipStream_t stream);
/* host only: the ciphertexts of one chunk at chain_index (min(64, scratch cap / scratch of one)) */
int phantom_rotate_fused_batch_chunk(const phantom_context *ctx, size_t chain_index, size_t *out);

#ifdef __cplusplus
}
#endif
#endif /* PHANTOM_AMD_H */
