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
  ConvPlanData() = default;
  ConvPlanData(const ConvPlanData&) = delete;
  ConvPlanData& operator=(const ConvPlanData&) = delete;
  ~ConvPlanData();
  size_t bytes() const { return words * sizeof(uint64_t); }
};
// conv_weight_slots -> encode_sub_raw (ext, ns slots, pt_scale) of every term, in slices that bound
// the scratch; waits for `s` before returning and never reads dev_W afterwards.  Refuses what
// conv2d_raw refuses, and 2 ns < 8.
std::unique_ptr<ConvPlanData> conv2d_prepare(const PhantomContext& ctx, size_t chain_index, const phx::ConvShape& c,
                                             const double* dev_W, double pt_scale, int* dev_overflow, hipStream_t s);
// conv2d_raw with the plan in place of the weights: the modups and batched rotations, one
// phx::ext_mac_sub launch over all output channels, the batched moddown.  Enqueued in order, nothing
// synchronised, no encode.  Refuses a plan of another context.
void conv2d_apply(const PhantomContext& ctx, const ConvPlanData& plan, const uint64_t* const* cts,
                  const uint64_t* const* const* evk, const uint32_t* galois_elts, uint64_t* const* outs,
                  hipStream_t s);

}  // namespace phantom
