// ckks.h — CKKS kernels beside the hot path: device-side sampling for key generation and
// encryption (the reference samples on the GPU too, src/prng.cu + sample_* in src/secretkey.cu),
// and the small bootstrap helpers of src/evaluate.cu (monomial multiply, extended-basis glue).
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "chacha.h"
#include "salsa.h"

namespace phx {

// Sampling from draw `nonce` of the ChaCha20 stream `key` (chacha.h), output [L][n] residues:
// uniform: 128-bit keystream values reduced mod q[l] (one independent value per element)
hipError_t sample_uniform(uint64_t* out, const uint64_t* q, const uint64_t* barrett, size_t n, size_t L,
                          const ChaChaKey& key, uint64_t nonce, hipStream_t s);
// the reference's expansion of a public 64-byte seed into a uniform [L][n] polynomial
// (sample_uniform_poly, src/prng.cu:164-197; salsa.h), bit for bit
hipError_t sample_uniform_seeded(uint64_t* out, const uint64_t* q, const uint64_t* barrett, size_t n, size_t L,
                                 const SalsaSeed& seed, hipStream_t s);
// centered binomial e_k (21 + 21 bits, sigma ~3.24), the same e_k in every limb (coefficient form)
hipError_t sample_cbd(uint64_t* out, const uint64_t* q, size_t n, size_t L, const ChaChaKey& key, uint64_t nonce,
                      hipStream_t s);
// ternary u_k in {-1, 0, 1}, the same u_k in every limb (coefficient form)
hipError_t sample_ternary(uint64_t* out, const uint64_t* q, size_t n, size_t L, const ChaChaKey& key, uint64_t nonce,
                          hipStream_t s);

// out[l][k] = in[l][k] * c[l] mod q[l] + (acc ? acc[l][k] : 0), Shoup constants c/c_shoup per limb
hipError_t mul_scalar_add(const uint64_t* in, const uint64_t* c, const uint64_t* c_shoup, const uint64_t* acc,
                          uint64_t* out, const uint64_t* q, size_t n, size_t L, hipStream_t s);
// out[p][l][k] += in[l][k] * c[l] mod q[l] for p < polys (out[p] at p poly_stride), one launch
hipError_t mul_scalar_accumulate(const uint64_t* in, const uint64_t* c, const uint64_t* c_shoup, uint64_t* out,
                                 size_t poly_stride, size_t polys, const uint64_t* q, size_t n, size_t L, hipStream_t s);

}  // namespace phx

namespace phx {

// ---- hoisted baby-step / giant-step linear transform (bootstrap CoeffToSlot / SlotToCoeff) ----
// For every giant step i < b:
//   out[i][t] = sum_{j < g} baby[j][t] * pts[g i + j]   (t = 0, 1)
// over the extended basis Ql u P ([2][Ql + P][n] ciphertexts, [Ql + P][n] plaintexts).  One
// launch reads every baby and every plaintext once (the reference multiplies and adds one
// (baby, plaintext) pair per launch: EvalMultExt + EvalAddExtInPlace, bootstrap.cu:1322-1332).
// pts is a device array of b * g non-null pointers (absent diagonals point at a zero
// plaintext); every out[i] is non-null.
constexpr int kLtMaxG = 32, kLtMaxB = 64;
struct LtArgs {
  const uint64_t* baby[kLtMaxG];
  uint64_t* out[kLtMaxB];
  const uint64_t* const* pts;  // device array [b][g]
  const uint64_t* q;           // full QP chain
  const uint64_t* barrett;     // [QP][2]
  int g = 0, b = 0, Ql = 0, P = 0, size_Q = 0;
  // every modulus of the chain below 2^60 (phantom::below_2_60): the 30-bit split partial sums
  // may then take 8 (tile kernels) or 16 (lt_bsgs_kernel) products before folding; otherwise a
  // high-half product reaches 2^62 and the sums fold every 4 products (0 is always safe)
  uint32_t q60 = 0;
};
hipError_t lt_bsgs(const LtArgs& a, size_t n, hipStream_t s);
// lt_bsgs of `count` (2..kLtGroupMax) ciphertexts at one level through the same plaintexts
// (bootstraps in lockstep) in one launch, the ciphertexts' blocks for the same elements on one XCD
// so that the plaintexts are read from HBM about once for all.  Each ciphertext's babies are
// contiguous (baby j at baby0[c] + j baby_stride words), its inner sum 0 goes to acc[c] and inner
// sum i >= 1 to giant1[c] + (i - 1) giant_stride; g == 32, b <= 8 (the bootstrap's levels).  Each
// result equals its own lt_bsgs, bit for bit.
#ifndef PHX_GROUP_MAX
#define PHX_GROUP_MAX 8  // ciphertexts of one lockstep group (the grouped kernels' argument arrays)
#endif
constexpr int kLtGroupMax = PHX_GROUP_MAX;
struct LtGroupArgs {
  const uint64_t* const* pts = nullptr;
  const uint64_t* q = nullptr;
  const uint64_t* barrett = nullptr;
  int g = 0, b = 0, Ql = 0, P = 0, size_Q = 0, count = 0;
  uint32_t q60 = 0;  // as LtArgs::q60
  uint64_t baby_stride = 0, giant_stride = 0;
  const uint64_t* baby0[kLtGroupMax] = {};
  uint64_t* acc[kLtGroupMax] = {};
  uint64_t* giant1[kLtGroupMax] = {};
};
hipError_t lt_bsgs_group(const LtGroupArgs& ga, size_t n, hipStream_t s);

// ---- Chebyshev leaves: M linear combinations of the same K ciphertexts in one pass ----------
//   out[m][t][l] = sum_k in[k][t][l] * coef[m][k][l] + (t == 0 ? cadd[m][l] : 0)   (mod q_l)
// in[k]: [2][*][n] ciphertexts with at least L limbs (polynomial stride in_stride[k] elements),
// out[m]: [2][L][n]; coef: device [2][M][K][L] (values, then Shoup quotients), cadd: [M][L].
// Every input is read once for all M outputs (the reference evaluates each leaf by separate
// EvalMult/EvalAdd passes: bootstrap.cu EvalChebyshevSeriesPS).
constexpr int kLeafMaxK = 16, kLeafMaxM = 8;
struct LeafArgs {
  const uint64_t* in[kLeafMaxK];
  size_t in_stride[kLeafMaxK];
  uint64_t* out[kLeafMaxM];
  const uint64_t* coef;
  const uint64_t* cadd;
  const uint64_t* q;
  const uint64_t* barrett;  // [L][2]
  int K = 0, M = 0, L = 0;
};
hipError_t leaf_combine(const LeafArgs& a, size_t n, hipStream_t s);

// ---- ct_mix: M linear combinations of K ciphertexts, K and M arbitrary (pool.hip) -------------
//   out[m][p][l][e] = sum_{k < K} in[k][p][l][e] * c[m][k][l] + (p == 0 ? cadd[m][l] : 0)   (mod q_l)
// in[k], out[m]: contiguous [2][L][n] ciphertexts, each list a device pointer table or (table null) a
// base pointer with a stride in words (as MacArgs).  coef: device [L][K][m_pad] residues below q_l,
// m_pad = mix_tiles(M) * mix_tile(M), the padding zero; cadd: device [M][L] or null.
//
// One thread owns one element of one limb for a tile of mix_tile(M) <= kMixTile outputs, whose
// 128-bit sums stay in registers (no scratch); the coefficients are workgroup-uniform and come
// through the scalar cache.  Every input is read once per tile: once for M <= kMixTile, else
// mix_tiles(M) = ceil(M / kMixTile) times.  A product is below q^2, so with q < 2^61 a 128-bit sum
// holds 64 products and the 65th can overflow (q < 2^60: 256 and the 257th): the sum is
// Barrett-reduced to below q after every kMixBlock = 32 terms and carried on (at most
// q + 32 q^2 < 2^128).  The result is the exact residue, hence bit-identical to mul_scalar and
// add_mod term by term.
constexpr int kMixTile = 16, kMixBlock = 32;
constexpr size_t mix_tiles(size_t M) { return (M + kMixTile - 1) / kMixTile; }
constexpr size_t mix_tile(size_t M) { return (M + mix_tiles(M) - 1) / mix_tiles(M); }
struct MixArgs {
  const uint64_t* const* ins = nullptr;  // device table [K], or
  const uint64_t* in0 = nullptr;
  uint64_t in_stride = 0;
  uint64_t* const* outs = nullptr;  // device table [M], or
  uint64_t* out0 = nullptr;
  uint64_t out_stride = 0;
  const uint64_t* coef = nullptr;
  const uint64_t* cadd = nullptr;
  const uint64_t* q = nullptr;
  const uint64_t* barrett = nullptr;  // [L][2]
  uint32_t K = 0, M = 0, L = 0;
};
hipError_t ct_mix(const MixArgs& a, size_t n, hipStream_t s);

// ---- ct_pack / ct_split: channel packing by monomial shifts and its rotation tree (pack.hip) ------
// Ciphertexts are contiguous [2][L][n], NTT form, 16-byte aligned; q / barrett are the chain's rows.
//   ct_pack:  out[p][l][i] = sum_{c < C} in_c[p][l][i] w[l][i]^c   (mod q_l),  w = NTT(X^D) [L][n]
// by Horner from the top channel down, so w is loaded once per element and every input read once
// (C + 1 reads of 2 L n words, counting w as L n, and one write).  Every step is fully reduced.
// The pointers travel in the argument block for C <= kPackInline, else in a device table [C].
//   ct_split: for node k < count, even_k = a_k + r_k and odd_k = (a_k - r_k) m,  m = NTT of a monomial [L][n]
// in one launch (a_k and r_k read once; 2 reads + m and up to 2 writes per node).  even_k or odd_k
// may be null (a pruned child); even_k may alias a_k, no other output may alias an input.
constexpr int kPackMax = 64, kPackInline = 16, kSplitMax = 64, kSplitInline = 8;
struct PackArgs {
  const uint64_t* in[kPackInline] = {};
  const uint64_t* const* table = nullptr;  // device [C]: read instead of `in` when not null
  const uint64_t* w = nullptr;
  uint64_t* out = nullptr;
  const uint64_t* q = nullptr;
  const uint64_t* barrett = nullptr;  // [L][2]
  uint32_t C = 0, L = 0;
  uint32_t lead = 0;  // out = w^lead sum_c in_c w^c: channel 0 at index `lead` (C + lead <= kPackMax)
};
hipError_t ct_pack(const PackArgs& a, size_t n, hipStream_t s);
struct SplitNode {
  const uint64_t* a;
  const uint64_t* r;
  uint64_t* even;
  uint64_t* odd;
};
struct SplitArgs {
  SplitNode node[kSplitInline] = {};
  const SplitNode* table = nullptr;  // device [count]: read instead of `node` when not null
  const uint64_t* m = nullptr;
  const uint64_t* q = nullptr;
  const uint64_t* barrett = nullptr;  // [L][2]
  uint32_t count = 0, L = 0;
};
hipError_t ct_split(const SplitArgs& a, size_t n, hipStream_t s);

// out[l] = in[l] * c[l] (+ acc[l]) with per-limb constants passed by value (no device upload);
// L <= kMaxScalarLimbs
constexpr int kMaxScalarLimbs = 64;
struct LimbScalars {
  uint64_t v[kMaxScalarLimbs];
  uint64_t vs[kMaxScalarLimbs];  // Shoup quotients (mul) / unused (add)
};
// mul_scalar_v over `polys` polynomials with the same constants: input p at in + p * in_stride
// (0: L n; a larger stride reads the first L limbs of longer polynomials, i.e. drops limbs),
// out and acc contiguous [polys][L][n]: out = in * c (+ acc)
hipError_t mul_scalar_v(const uint64_t* in, const LimbScalars& c, uint64_t* out, const uint64_t* q, size_t n,
                        size_t L, hipStream_t s, size_t polys = 1, size_t in_stride = 0,
                        const uint64_t* acc = nullptr);
// Tensor product of two [2][L][n] ciphertexts into out [3][L][n] with MulAddRescale's linear
// epilogue fused: d = f (ct1 x ct2) (if scale) and, for t, d[p] += t[p] c for p < 2
// (t[p] at t + p * t_stride, its first L limbs).  out must not alias the inputs.
struct TensorLinArgs {
  const uint64_t* ct1;
  const uint64_t* ct2;
  uint64_t* out;
  const uint64_t* t = nullptr;
  size_t t_stride = 0;
  const uint64_t* q;
  const uint64_t* barrett;
  bool scale = false;
  LimbScalars f;
  LimbScalars c;
};
hipError_t tensor_lin(const TensorLinArgs& a, size_t n, size_t L, hipStream_t s);

// tensor_lin of up to kTensorBatchMax independent products at one level in one launch (one grid
// row per product), with the product's constant folded in as well: for product k,
// out[k] = factor ct1 x ct2 (+ t c in polys 0, 1) (+ cadd in poly 0), every per-limb constant a
// residue (c, cadd) in `limb` [count][2][L] by value.  The values are those of tensor_lin followed
// by add_scalar_v, bit for bit.
constexpr int kTensorBatchMax = 8, kTensorBatchLimbWords = 384;
struct TensorLinJob {
  const uint64_t* ct1;
  const uint64_t* ct2;
  uint64_t* out;
  const uint64_t* t;  // null: no term
  uint64_t t_stride;
  uint64_t factor;    // 1: unscaled
  uint32_t has_const;
};
struct TensorLinBatchArgs {
  const uint64_t* q;
  const uint64_t* barrett;
  uint32_t L = 0, count = 0;
  TensorLinJob job[kTensorBatchMax];
  uint64_t limb[kTensorBatchLimbWords];
};
hipError_t tensor_lin_batch(const TensorLinBatchArgs& a, size_t n, hipStream_t s);

// d[p] = d[p] * ca (ca may be null: unscaled) + (p < t_polys ? t[p] * cb : 0) for p < d_polys;
// d contiguous [d_polys][L][n], t[p] at t + p * t_stride (its first L limbs)
hipError_t lin_comb_v(uint64_t* d, size_t d_polys, const LimbScalars* ca, const uint64_t* t, size_t t_polys,
                      size_t t_stride, const LimbScalars& cb, const uint64_t* q, size_t n, size_t L, hipStream_t s);
hipError_t add_scalar_v(const uint64_t* in, const LimbScalars& c, uint64_t* out, const uint64_t* q, size_t n,
                        size_t L, hipStream_t s);

}  // namespace phx
