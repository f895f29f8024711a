// conv.h — kernels of the hoisted encrypted 2-D convolution (the reference's DNN::Conv,
// src/dnn.cu:82-150, which runs one rotation, one plaintext product and one addition per
// (output channel, input channel, tap)): general inner sums over the extended basis, and the
// weight tensor laid out as masked slot vectors.
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace phx {

// ---- general inner sums over the extended basis Ql u P --------------------------------------
//   out[o][p][l][e] (+)= sum_{t < T} in[t][p][l][e] * pt[o T + t][l][e]   (mod q_l),  p < 2, o < O
// in[t], out[o]: [2][Ql + P][n] ciphertexts, pt[k]: [Ql + P][n] plaintexts; T >= 1 and O >= 1 are
// arbitrary (lt_bsgs computes the same form for g a power of two <= 32 and b <= 64).  Each of the
// three operand lists is a device pointer table, or (table null) a base pointer with a stride in
// words: in[t] = in0 + t in_stride, pt[k] = pt0 + k pt_stride, out[o] = out0 + o out_stride.
//
// Arithmetic as lt_bsgs: operands split in 30-bit halves, four 64-bit partial sums per element
// and polynomial, folded into a 128-bit sum every 8 products when every modulus is below 2^60
// (q60), every 4 otherwise.  The 128-bit sum itself is bounded: a product is below q^2, so with
// q < 2^61 the sum of 64 products fits and the 65th can overflow (q < 2^60: 256 and the 257th).
// It is therefore Barrett-reduced to below q after every block of kMacBlock = 32 terms and carried
// on: at most q + 32 q^2 < 2^127 + 2^61.  The result is exact modulo q, hence bit-identical however
// the terms are blocked.
//
// Tiled form (n a multiple of the 128-element tile, n >= kMacTileMinN): one workgroup = 8 waves
// over one tile; a block of 32 inputs x 2 polynomials is staged in LDS as 30-bit halves (64 KiB)
// and shared by the 8 outputs of the workgroup, wave w streaming the plaintexts of output
// 8 blockIdx.y + w; the sums stay in registers across term blocks and the tail block is padded with
// zeros.  Every input is read once per 8 outputs, every plaintext once.  Other shapes take a plain
// one-element-per-thread form.
constexpr int kMacBlock = 32, kMacWaves = 8, kMacEpl = 2, kMacTile = 64 * kMacEpl;
constexpr size_t kMacTileMinN = 1024;
struct MacCore {
  const uint64_t* const* ins = nullptr;  // device table [T], or
  const uint64_t* in0 = nullptr;
  uint64_t in_stride = 0;
  const uint64_t* const* pts = nullptr;  // device table [O][T] (no null entries), or
  const uint64_t* pt0 = nullptr;
  uint64_t pt_stride = 0;
  uint64_t* const* outs = nullptr;  // device table [O], or
  uint64_t* out0 = nullptr;
  uint64_t out_stride = 0;
  const uint64_t* q = nullptr;        // full QP chain
  const uint64_t* barrett = nullptr;  // [QP][2]
  uint32_t T = 0, O = 0, Ql = 0, P = 0, size_Q = 0;
  uint32_t q60 = 0;         // as LtArgs::q60
  uint32_t accumulate = 0;  // add the value already in out[o] (below q)
};
struct MacArgs : MacCore {
  // optional seed (below); all three null: no seed
  const uint64_t* const* seed_res = nullptr;  // device table [O] of [2][Ql][n] ciphertexts; entries may be null
  const uint64_t* seed_mult = nullptr;        // device [Ql], required with seed_res
  const uint64_t* seed_bias = nullptr;        // device [O][Ql]
};
// ---- the seed: an affine term entering the sum in the extended basis --------------------------
// With seed_res or seed_bias set, the sum of output o, polynomial p, limb l, element e starts at
//   l < Ql:   (seed_res[o] ? seed_res[o][p][l][e] seed_mult[l] : 0) + (p == 0 && seed_bias ? seed_bias[o][l] : 0)  (mod q_l)
//   l >= Ql:  0                                                                      (the limbs of P)
// instead of 0.  The residuals are ciphertexts over Ql (limb stride Ql, not Ql + P) with words below
// q_l, read with the kernel's 16-byte accesses; seed_mult and seed_bias hold residues below q_l.  A
// caller that passes (m P) mod q_l and (B_o P) mod q_l adds P (m res_o + [p == 0] B_o), which is
// 0 modulo P, so the moddown of the result is moddown(sum) + m res_o + [p == 0] B_o word for word
// (DESIGN.md §3 "Fused affine terms").  The seed is reduced below q (one Barrett product, one
// conditional subtraction) before it enters the 128-bit sum, where it takes the place of
// `accumulate`'s old value: the bound q + 32 q^2 < 2^127 + 2^61 and the folding schedule above hold
// as written.  A seed together with accumulate, and seed_res without seed_mult, are refused
// (hipErrorInvalidValue).  Both ext_mac and ext_mac_sub take a seed, in the tiled and the plain form.
// The kernels take MacCore by value and the seed as a trailing argument of their seeded instantiations
// only, so a launch without a seed has the signature, the arguments and the code it had before seeds
// existed, and every seeded instantiation keeps its twin's registers and uses no scratch on gfx950
// (DESIGN.md §3).
hipError_t ext_mac(const MacArgs& a, size_t n, hipStream_t s);

// ---- the same sums over compact plaintexts ---------------------------------------------------
//   out[o][p][l][e] (+)= sum_{t < T} in[t][p][l][e] * pt[o T + t][l][e >> log2(n / sub_degree)]   (mod q_l)
// pt[k]: [Ql + P][sub_degree], the subring form of a sparse-packed plaintext (host/encoder.h
// encode_sub_raw: a polynomial in X^(n / sub_degree) takes equal NTT values on blocks of
// g = n / sub_degree words); sub_degree is a power of two in [1, n].  The arithmetic contract is
// ext_mac's (30-bit halves, folds every 8 / 4 products, Barrett reduction every kMacBlock terms), so
// the result is exact for any T and equals ext_mac on the plaintexts expanded g-fold.
//
// Plaintext traffic is 1/g of the input traffic, so the kernel is bound by the input bytes and the
// multiplies, and the tile is chosen for those: one workgroup = kSubWaves = 16 waves over one
// 128-element tile, each wave one output, the staged block of 32 inputs x 2 polynomials (64 KiB of
// LDS) shared by 16 outputs (ext_mac: 8).  1,024 threads and 64 KiB leave one workgroup of 4 waves
// per SIMD on a CU, at most 128 VGPRs per lane; the sums, the double-buffered plaintext words and the
// prefetched rows fit without scratch.  Other shapes (n < kMacTileMinN) take a
// one-element-per-thread form.
constexpr int kSubWaves = 16;
hipError_t ext_mac_sub(const MacArgs& a, size_t n, size_t sub_degree, hipStream_t s);

// ---- the weight tensor as masked slot vectors ------------------------------------------------
// W: [K][K][in_ch][out_ch] doubles, row-major (the reference's weight[a][b][k][h]).  With
// pow = 2^slotstr, Lg = width pow and ns = Lg^2, term (h, k, a, b) is a real vector of ns slots,
// written as interleaved (re, 0): the slot at (r Lg + c) pow, r, c < width, is W[a][b][k][h] when
// r + a - K/2 and c + b - K/2 both lie in [0, width), every other slot 0 (src/dnn.cu:103-113).
// Terms are ordered (h, k, a, b), b fastest; `count` terms from `first_term` go to out [count][ns].
// dev_out_scale (device [out_ch], null: none): the terms of output channel h are multiplied by
// dev_out_scale[h] in FP64, one rounding per weight (a batch norm's scale folded into the layer).
struct ConvShape {
  uint32_t width = 0, slotstr = 0, kernel = 0, in_ch = 0, out_ch = 0;
  size_t large() const { return static_cast<size_t>(width) << slotstr; }
  size_t slots() const { return large() * large(); }
  size_t terms() const { return static_cast<size_t>(out_ch) * in_ch * kernel * kernel; }
};
hipError_t conv_weight_slots(const ConvShape& c, const double* dev_W, size_t first_term, size_t count, double* dev_out,
                             hipStream_t s, const double* dev_out_scale = nullptr);
void conv_weight_slots_host(const ConvShape& c, const double* W, size_t first_term, size_t count, double* out);

// `count` (<= kWordsMax) 64-bit words passed by value written to dst: small device tables built
// without a host-to-device copy, in stream order
constexpr int kWordsMax = 384;
struct Words {
  uint64_t w[kWordsMax];
};
hipError_t write_words(uint64_t* dst, const Words& w, size_t count, hipStream_t s);

}  // namespace phx
