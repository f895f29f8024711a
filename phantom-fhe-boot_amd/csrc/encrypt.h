// encrypt.h — batched symmetric CKKS encryption and decryption kernels for gfx950.
//
// Replaces, for a whole batch, the per-ciphertext launch chain of encrypt_symmetric_internal and
// ckks_decrypt (src/secretkey.cu:576-682): seed expansion, error sampling, a s + e, negate, + m on
// one side and c0 + c1 s (+ c2 s^2) on the other.  Every launcher checks its arguments first
// (hipErrorInvalidValue, nothing enqueued), enqueues on the caller's stream only and never
// synchronises.  All results are canonical residues, so they equal the sequential path bit for bit.
//
// One chunk of `count` (<= kCtChunkMax) ciphertexts at L limbs is encrypted by
//   embed_inverse (encode.h)      values -> [count][n] doubles
//   sample_cbd_small              e[p] = CBD of draw nonces[p], [count][n] small signed
//   round_to_rns_minus            c0[p] = (round(coeffs[p] scale) - e[p]) mod q_i, coefficient form
//   ntt_forward (ntt.h), batched  c0[p] = NTT(m) - NTT(e): the NTT is linear, e needs no limbs of its own
//   expand_and_finish             c1[p] = the uniform expansion of seeds[p], c0[p] -= c1[p] s
// (7 launches; drawing c1 in a kernel of its own took 86 us per chunk of 32 at N = 2^16, 5 limbs,
// against 68 us for the one kernel, with identical bits)
// and decrypted by decrypt_dot followed by the decoder (INTT, compose_centred, embed_forward).
//
// Chunking.  The per-ciphertext arguments of a chunk (nonces, seeds, addresses) travel by value in
// the launch arguments, so a chunk holds at most kCtChunkMax ciphertexts; the drivers
// (host/keys.h encrypt_symmetric_raw / decrypt_decode_raw) cut a batch into chunks of
//   encrypt_chunk(n) = clamp(kEncryptScratchBytes / (28 n), 1, kCtChunkMax)
// ciphertexts: 28 n bytes of pool scratch each (8 n coefficients, 16 n embedding work area, 4 n
// error), i.e. at most kEncryptScratchBytes = 64 MiB live per call (56 MiB for 32 at n = 2^16).
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "chacha.h"
#include "rns.h"
#include "salsa.h"

namespace phx {

constexpr int kCtChunkMax = 32;
constexpr size_t kEncryptScratchBytes = size_t(64) << 20;
inline size_t encrypt_chunk(size_t n) {
  const size_t c = kEncryptScratchBytes / (28 * n);
  return c < 1 ? 1 : (c > kCtChunkMax ? kCtChunkMax : c);
}

// Where the ciphertexts of a chunk start: p at base + p * stride words, or at ptr[p] when base is
// null.  Every start is 16-byte aligned and stride is even (the kernels move two words per lane).
struct CtChunk {
  uint64_t* base = nullptr;
  size_t stride = 0;
  uint64_t* ptr[kCtChunkMax] = {};
  __host__ __device__ uint64_t* at(int p) const { return base ? base + static_cast<size_t>(p) * stride : ptr[p]; }
};

// e[p][k] for p < count (<= kCtChunkMax): the centered binomial of 64-bit word k of draw nonces[p]
// of the ChaCha20 stream `key`, the signed value sample_cbd spreads over its limbs (|e| <= 21).
// nonces is a host array.  n a multiple of 8.
hipError_t sample_cbd_small(int32_t* out, size_t n, const ChaChaKey& key, const uint64_t* nonces, size_t count,
                            hipStream_t s);

// c0 of ciphertext p, limbs i < L (table rows 0 .. L-1), coefficient form:
//   out.at(p)[i n + k] = (round_half_even(coeffs[p][k] * scale) - e[p][k]) mod q_i
// with round_to_rns's rounding, wide range and overflow flag (encode.h).
hipError_t round_to_rns_minus(ModView m, const double* coeffs, double scale, const int32_t* e, const CtChunk& out,
                              size_t n, size_t L, size_t count, int* overflow, hipStream_t s);

// c1 of ciphertext p (at ct.at(p) + L n) = sample_uniform_seeded(seeds[p]) over rows 0 .. L-1, bit
// for bit, rejection path included, and c0[p] = c0[p] - c1[p] * sk mod q_i in place.  seeds: host,
// count x 64 bytes; sk [>= L][n] in NTT form over rows 0 .. L-1.
hipError_t expand_and_finish(ModView m, const uint8_t* seeds, const uint64_t* sk, const CtChunk& ct, size_t n,
                             size_t L, size_t count, hipStream_t s);

// out[p][i] = c1[p] word i (n / 8) for i < 8 L: the 8 words per limb that PhantomCiphertext::set_seed
// fingerprints, of a whole chunk in one launch (one host copy then serves every ciphertext)
hipError_t gather_c1_samples(const CtChunk& ct, size_t n, size_t L, size_t count, uint64_t* out, hipStream_t s);

// out[p][i][k] = c0 + sk (c1 + sk c2) mod q_i for i < limbs (<= ct_limbs), polys in {2, 3}: the
// leading `limbs` limbs of ciphertext p at in.at(p), polynomial stride ct_limbs n; out contiguous
// [count][limbs][n], NTT form.  The inputs are only read.
hipError_t decrypt_dot(ModView m, const uint64_t* sk, const CtChunk& in, size_t n, size_t ct_limbs, size_t polys,
                       size_t limbs, size_t count, uint64_t* out, hipStream_t s);

}  // namespace phx
