// conv2d.h — the hoisted encrypted 2-D convolution on raw device buffers, shared by the DNN façade
// (host/dnn.h) and the C-ABI (csrc/capi_conv.cpp).
//
// The reference's DNN::Conv (src/dnn.cu:82-150) runs, for each of the out_ch in_ch K^2 terms, one
// host sparse encode, one EvalRotateFused (modup + inner product + moddown), one plaintext product
// and one addition.  Here a layer is
//   in_ch   modups                      (one per input channel, shared by its K^2 rotations)
//   in_ch   batched rotation launches   (K^2 rotations each, kept in the extended basis Ql u P)
//   passes  of `group` output channels: weight slot vectors -> device encode (extended basis,
//           sparse packing) -> one inner-sum launch over all in_ch K^2 terms (phx::ext_mac)
//   1       batched moddown of the 2 out_ch output polynomials
// and no plaintext crosses the host.  A prepared layer (conv2d_prepare / conv2d_apply below) encodes
// the weights once in the compact subring form and runs the same modups, rotations and moddown
// around one inner-sum launch over all output channels (phx::ext_mac_sub).
#pragma once

#include <cstddef>
#include <cstdint>
#include <memory>
#include <vector>

#include "../csrc/conv.h"
#include "context.h"

namespace phantom {

// throws std::invalid_argument unless: width a power of two, kernel odd and <= width, in_ch and
// out_ch >= 1, and ns = (width 2^slotstr)^2 <= n / 2
phx::ConvShape conv_shape(size_t n, size_t width, size_t slotstr, size_t kernel, size_t in_ch, size_t out_ch);
// the K^2 tap rotations in tap order (a, b), b fastest: ((a - K/2) Lg + (b - K/2)) 2^slotstr slots
// (src/dnn.cu:114,122 and AddRotationIndicesTo, :299-319); 0 for the centre tap
std::vector<int> conv_rotations(size_t width, size_t slotstr, size_t kernel);
// output channels per pass when the caller leaves it to the engine: as many as keep the pass's
// extended-basis plaintexts within kConvPlainBudget bytes (at least 1, at most out_ch)
constexpr size_t kConvPlainBudget = size_t(8) << 30;
size_t conv_group(const PhantomContext& ctx, size_t chain_index, const phx::ConvShape& c);
// the modulus tables and flags of an inner-sum launch at chain_index (operand lists left empty)
phx::MacArgs mac_args(const PhantomContext& ctx, size_t chain_index);

// The whole layer.  cts[k]: [2][Ql][n] input channel k, outs[h]: [2][Ql][n] output channel h (host
// arrays of device pointers), dev_W: [K][K][in_ch][out_ch] doubles.  evk[tap]: the device key-digit
// array of tap's rotation (nullptr: the centre tap, no rotation), galois_elts[tap] its Galois
// element.  group: output channels per pass (0: conv_group).  Everything is enqueued on `s` in
// order, scratch comes from the pool, nothing is synchronised.  Arguments are checked
// (std::invalid_argument) before anything is enqueued.
void conv2d_raw(const PhantomContext& ctx, size_t chain_index, const uint64_t* const* cts, const phx::ConvShape& c,
                const double* dev_W, double pt_scale, const uint64_t* const* const* evk, const uint32_t* galois_elts,
                size_t group, uint64_t* const* outs, int* dev_overflow, hipStream_t s);

// A prepared layer.  The weights are fixed across inferences, and a sparse-packed plaintext is a
// polynomial in X^(N / 2 ns), so its subring form (encode_sub_raw; the reference's sparse encoder,
// src/ckks.cu:180-270) takes 2 ns words per limb instead of N: all out_ch in_ch K^2 extended-basis
// plaintexts of a layer stay resident in one device allocation of terms (Ql + P) 2 ns words.
struct ConvPlanData {
  const PhantomContext* ctx = nullptr;
  size_t chain_index = 0;
  phx::ConvShape shape;
  double scale = 0;
  size_t sub_degree = 0;    // 2 ns
  size_t words = 0;         // of pts
  uint64_t* pts = nullptr;  // [terms][Ql + P][sub_degree], terms ordered (h, k, a, b)
  std::vector<double> shift;  // b_h of a folded batch norm (DNN::PrepareConvBN), [out_ch]; empty: none
  ConvPlanData() = default;
  ConvPlanData(const ConvPlanData&) = delete;
  ConvPlanData& operator=(const ConvPlanData&) = delete;
  ~ConvPlanData();
  size_t bytes() const { return words * sizeof(uint64_t); }
};
// conv_weight_slots -> encode_sub_raw (ext, ns slots, pt_scale) of every term, in slices that bound
// the scratch; waits for `s` before returning and never reads dev_W afterwards.  Refuses what
// conv2d_raw refuses, and 2 ns < 8.  out_scale (host [out_ch], null: all 1.0): the weights of output
// channel h are multiplied by out_scale[h] in FP64 on the device before they are encoded (a batch
// norm's a_h folded into the layer); dev_W itself is not modified.
std::unique_ptr<ConvPlanData> conv2d_prepare(const PhantomContext& ctx, size_t chain_index, const phx::ConvShape& c,
                                             const double* dev_W, double pt_scale, int* dev_overflow, hipStream_t s,
                                             const double* out_scale = nullptr);
// conv2d_raw with the plan in place of the weights: the modups and batched rotations, one
// phx::ext_mac_sub launch over all output channels, the batched moddown.  Enqueued in order, nothing
// synchronised, no encode.  Refuses a plan of another context.
//
// Fused affine terms (all optional): res (host [out_ch] of device [2][Ql][n] ciphertexts at the plan's
// chain index, entries may be null) with res_mult (host [Ql], m mod q_l), and bias (host
// [out_ch][Ql], B_h mod q_l).  out_h = layer_h + m res_h + (B_h on c0) modulo q_l, word for word what
// the layer without them returns plus those terms: both enter the one inner-sum launch as its seed,
// multiplied by P mod q_l here, and a multiple of P passes through the moddown exactly (csrc/conv.h).
// The seed's tables are written in stream order (phx::write_words); no other launch, no pass over
// memory and no synchronisation is added.  res without res_mult is refused.
void conv2d_apply(const PhantomContext& ctx, const ConvPlanData& plan, const uint64_t* const* cts,
                  const uint64_t* const* const* evk, const uint32_t* galois_elts, uint64_t* const* outs,
                  hipStream_t s, const uint64_t* const* res = nullptr, const uint64_t* res_mult = nullptr,
                  const uint64_t* bias = nullptr);

// round(value scale) mod q for every q of `moduli`: the constant polynomial of a bias at a scale that
// may exceed 2^64.  The product is one FP64 value, m 2^e with an integer m below 2^53; for e >= 0 it
// is that integer exactly and its residue is (m mod q) 2^e mod q (the mantissa-and-power-of-two path
// of GetElementForEvalAddOrSub, without its cast to 64 bits); below 2^53 it is rounded to the nearest
// integer, halves away from zero.  A negative product gives q - (|B| mod q).  std::invalid_argument:
// a product that is not finite, a scale that is not positive, a zero modulus.
std::vector<uint64_t> scaled_constant_residues(double value, double scale, const uint64_t* moduli, size_t count);

// the seed tables of an inner-sum launch in `table` (device, mac_seed_words(O, Ql) words), written in
// stream order, and their pointers in `a`: res / res_mult / bias as conv2d_apply takes them, with
// res_mult and bias multiplied by P mod q_l.  Refuses res without res_mult.
size_t mac_seed_words(size_t O, size_t Ql);
void mac_seed(const PhantomContext& ctx, size_t chain_index, size_t O, const uint64_t* const* res,
              const uint64_t* res_mult, const uint64_t* bias, uint64_t* table, phx::MacArgs& a, hipStream_t s);

}  // namespace phantom
