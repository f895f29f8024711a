// encode.h — CKKS encode / decode on gfx950: the canonical embedding in FP64, the rounding and
// RNS split of its coefficients, and the CRT composition of a plaintext's residues.
//
// Replaces the reference's device encoder: the special FFT (src/fft.cu:651-815), decompose_array /
// compose_array (src/rns_base.cu:49-260) and their driver (src/ckks.cu:103-178, 456-521).  Every
// launcher is batched over `count` plaintexts and enqueues on the caller's stream only.
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "ntt.h"

namespace phx {

// Per-context tables of the embedding (host/context.cpp builds them once, in double with cos / sin).
struct EmbedTables {
  size_t n = 0;
  int log_n = 0;
  const double2* zeta = nullptr;     // [2n] zeta^j = exp(2 pi i j / 2n)
  // [n] for position m of the size-n transform (root zeta^(2m + 1)): the slot j whose root that is
  // (zeta^(5^j)), or j | kConjBit when it is the conjugate root zeta^(-5^j)
  const uint32_t* slot_of = nullptr;
  static constexpr uint32_t kConjBit = 0x80000000u;
};

// The embedding is one size-n complex radix-2 transform (decimation in time on bit-reversed input,
// the order of PhantomCKKSEncoder::fft), run as two passes that each keep a tile in LDS: the first
// ceil(log n / 2) stages on contiguous blocks, the rest on strided columns.
//
// inverse: slots -> coefficients.  Plaintext p reads `num_values` complex values at
// in + p * num_values; slot j takes value j mod ns (0 when that index is >= num_values), ns =
// sparse_slots or n/2 when 0.  Writes n doubles per plaintext (1/n included, not scaled).
// `work` holds count * n complex values of scratch.
hipError_t embed_inverse(const EmbedTables& t, const double2* in, size_t num_values, size_t sparse_slots,
                         double* coeffs, double2* work, size_t count, hipStream_t stream);
// forward: coefficients -> slots.  Reads n doubles per plaintext, each times `mul` (decode's
// 1 / scale; 1.0 leaves them as they are), writes the first ns slots (ns as above) at out + p * ns.
hipError_t embed_forward(const EmbedTables& t, const double* coeffs, double mul, size_t sparse_slots, double2* out,
                         double2* work, size_t count, hipStream_t stream);

// Round and split: out[p][i][k] = round_half_even(coeffs[p][k] * scale) mod q_row(i) for the limbs
// of `map` (negative values as q - v), exactly as double_to_residue in host/encoder.cpp for every
// |x| < 2^1000.  A non-finite or larger product sets *overflow (when not null) to 1 and leaves
// unspecified residues.  Coefficient form; `map` gives the limb -> table row assignment only.
hipError_t round_to_rns(const NttTables& t, const double* coeffs, double scale, uint64_t* out, const LimbMap& map,
                        size_t count, int* overflow, hipStream_t stream);

// Per-chain constants of the composition (Garner's mixed radix form over q_0 .. q_{L-1}).
constexpr int kMaxComposeLimbs = 64;
struct ComposeTables {
  int L = 0;
  const uint64_t* prefix = nullptr;        // [L][L]: prefix[i L + j] = q_0 ... q_{j-1} mod q_i (j < i)
  const uint64_t* prefix_shoup = nullptr;  // their Shoup quotients
  const uint64_t* inv_prefix = nullptr;    // [L] (q_0 ... q_{i-1})^-1 mod q_i, then [L] Shoup quotients
  const uint64_t* half_digits = nullptr;   // [L] mixed-radix digits of (Q - 1) / 2
};
// coeffs[p][k] = mul * (the centred integer in (-Q/2, Q/2] with residues res[p][i][k]), accumulated
// from the top digit in double-double: exact below 2^53, else within one ulp of correct rounding.
// res is coefficient form over table rows 0 .. L-1.
hipError_t compose_centred(const NttTables& t, const ComposeTables& c, const uint64_t* res, double mul, double* coeffs,
                           size_t count, hipStream_t stream);

}  // namespace phx
