// avgpool.h — the hoisted average pooling + fully connected layer on raw device buffers, shared by
// the DNN façade (host/dnn.h) and the C-ABI (csrc/capi_pool.cpp).
//
// The reference's DNN::AvgPoolFullCon (src/dnn.cu:397-452) pools each of the t input channels by
// 2 log2(width) sequential EvalRotateFused + EvalAddAuto steps (a full key switch each: modup, inner
// product, moddown of two polynomials), then forms T t constant products and additions, then adds
// the bias.  Pooling and the fully connected layer are both linear and commute, so here a layer is
//   1       channel mix t -> T                 (phx::ct_mix, no key switch)
//   T       modups + rotate-and-sum launches   (the width - 1 column rotations of an output and the
//           identity from one set of digits, summed in the extended basis Ql u P: phx::keyswitch_rotate_sum)
//   1       batched moddown of the 2 T polynomials
//   T + T + 1   the same over the width - 1 row rotations
//   T       bias additions to c0
// A full moddown of both polynomials stands between the two directions.
//
// Rotation amounts.  With pow = 2^slotstr and Lg = width pow, pixel (r, c) sits at slot
// (r Lg + c) pow, so a column step is pow slots and a row step Lg pow slots.  The reference
// (src/dnn.cu:334-338, :421) rotates rows by Lg 2^j, a row step only when slotstr = 0; at slotstr = 2,
// width 8 it rotates by 32, 64, 128 with rows 128 slots apart and pools two rows of eight.  The
// amounts here are the correct ones and equal the reference's for slotstr = 0.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "context.h"

namespace phantom {

// throws std::invalid_argument unless width is a power of two in 2..64 and
// ns = (width 2^slotstr)^2 <= n / 2
void avgpool_shape(size_t n, size_t width, size_t slotstr);
// the 2 (width - 1) rotations, columns first: i 2^slotstr for i = 1..width-1, then
// j width 4^slotstr for j = 1..width-1
std::vector<int> avgpool_rotations(size_t width, size_t slotstr);

// The whole layer.  cts[k]: [2][Ql][n] input channel k < t, outs[u]: [2][Ql][n] output u < T (host
// arrays of device pointers; no output may alias an input).  coef: host [T][t][Ql] residues of the
// weights, bias: host [T][Ql] residues added to c0 at the end.  col_evk[i] / row_evk[i], i < width - 1:
// the device key-digit array of rotation i + 1 of the direction, col_elts / row_elts their Galois
// elements.  Everything is enqueued on `s` in order, scratch comes from the pool, nothing is
// synchronised.  Arguments are checked (std::invalid_argument) before anything is enqueued.
void avgpool_fc_raw(const PhantomContext& ctx, size_t chain_index, const uint64_t* const* cts, size_t t, size_t T,
                    size_t width, size_t slotstr, const uint64_t* coef, const uint64_t* bias,
                    const uint64_t* const* const* col_evk, const uint64_t* const* const* row_evk,
                    const uint32_t* col_elts, const uint32_t* row_elts, uint64_t* const* outs, hipStream_t s);

// ct_mix on host coefficient tables: coef [M][K][Ql] and cadd [M][Ql] (or null) are reduced, laid out
// as the kernel reads them and written to `table` (mix_table_words words of device memory) in stream
// order, then the mix ins[k] -> outs[m] is enqueued.  ins / outs: host arrays of device pointers.
size_t mix_table_words(size_t K, size_t M, size_t L);
void ct_mix_raw(const PhantomContext& ctx, size_t chain_index, const uint64_t* const* ins, size_t K,
                const uint64_t* coef, const uint64_t* cadd, uint64_t* const* outs, size_t M, uint64_t* table,
                hipStream_t s);

}  // namespace phantom
