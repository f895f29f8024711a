// encrypt.h — batched symmetric and public-key CKKS encryption and decryption kernels for gfx950
// (the public-key part has its own header comment below).
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

// ---- batched public-key encryption ------------------------------------------------------------
// Replaces, for a whole batch, encrypt_zero_asymmetric_internal + the plaintext add
// (src/secretkey.cu:12-185): (pk0 u + e0, pk1 u + e1) over Q u P, divided by P, + m.  Two identities
// cut the work (DESIGN.md "Batched public-key encryption"): the division by P is per limb, so only
// the `rows` = L + alpha rows {0 .. L-1} u {size_Q .. size_QP-1} of the key chain are ever formed;
// and P m added to the data rows of pk0 u + e0 comes out of the division as + m exactly, so the
// message rides in e0's coefficients and has no buffer, transform or add of its own.
//
// One chunk of `count` (<= kCtChunkMax) ciphertexts at L limbs is encrypted by
//   embed_inverse (encode.h)      values -> [count][n] doubles                               2 launches
//   sample_asym_small             u[p], e0[p], e1[p]: [count][3][n] small signed             1
//   round_lift                    U[p] = u, X[p][0] = e0 (+ [P]_q round(coeffs[p] scale) on
//                                 data rows), X[p][1] = e1: coefficient form, [.][rows][n]   1
//   ntt_forward (ntt.h), batched  the 3 count polynomials over those rows                    2
//   pk_fma                        X[p][j] += U[p] pk_j                                       1
//   RnsTool::moddown_add          2 count polynomials: INTT(P), conversion, NTT + finish     5
// (12 launches; 13 with the opt-in unbiased moddown).  The division writes a contiguous batch in
// place; a padded stride or per-ciphertext outputs go through scatter_ct (one launch more).
//
// Chunking: U and X cost 24 rows n bytes per ciphertext, the embedding and the small samples 36 n
// (8 n coefficients, 16 n work area, 12 n samples), so the driver (host/keys.h
// encrypt_asymmetric_raw) cuts a batch into chunks of
//   asym_chunk(n, rows) = clamp(kAsymScratchBytes / ((24 rows + 36) n), 1, kCtChunkMax)
// ciphertexts.  kAsymScratchBytes = 256 MiB: at n = 2^16 on the bootstrap chain (30 + 10 limbs) that
// is 10 ciphertexts at chain index 26 (15 rows) and 4 at chain index 1 (40 rows, 63 MiB each).  The
// division's own scratch (16 L n per ciphertext in the context's workspace) and the staging of a
// scattered output (16 L n) come on top.
constexpr size_t kAsymScratchBytes = size_t(256) << 20;
inline size_t asym_chunk(size_t n, size_t rows) {
  const size_t c = kAsymScratchBytes / ((24 * rows + 36) * n);
  return c < 1 ? 1 : (c > kCtChunkMax ? kCtChunkMax : c);
}

// Buffer row r of the extended polynomials is key-chain row (r < L ? r : first_p + r - L).
struct AsymRows {
  int L = 0;        // data rows 0 .. L-1
  int alpha = 0;    // special rows first_p .. first_p + alpha - 1
  int first_p = 0;  // size_Q
  int total = 0;    // size_QP: rows of each polynomial of the public key
  __host__ __device__ int rows() const { return L + alpha; }
  __host__ __device__ int table_row(int r) const { return r < L ? r : first_p + (r - L); }
};

// Small signed samples of several draws of one ChaCha20 stream, out[d][k] for d < draws
// (<= 3 kCtChunkMax) from 64-bit word k of draw nonces[d] (host array):
//   kSmallCbd: the centered binomial (sample_cbd's value, |e| <= 21);
//   kSmallTernary: word mod 3, minus 1 (sample_ternary's value);
//   kSmallAsym: ternary for d % 3 == 0, else centered binomial: (u, e0, e1) of ciphertext d / 3.
enum SmallKind : int { kSmallCbd = 0, kSmallTernary = 1, kSmallAsym = 2 };
hipError_t sample_small(int32_t* out, size_t n, SmallKind kind, const ChaChaKey& key, const uint64_t* nonces,
                        size_t draws, hipStream_t s);
// small [count][3][n] = (u, e0, e1)[p] from the draws nonces[3 p], nonces[3 p + 1], nonces[3 p + 2]
inline hipError_t sample_asym_small(int32_t* small, size_t n, const ChaChaKey& key, const uint64_t* nonces,
                                    size_t count, hipStream_t s) {
  if (count > static_cast<size_t>(kCtChunkMax)) return hipErrorInvalidValue;
  return sample_small(small, n, kSmallAsym, key, nonces, 3 * count, s);
}

// Coefficient form over the rows of `rw` (m: the key chain's moduli, indexed by table row):
//   U[p][r][k]    = u[p][k] mod q
//   X[p][0][r][k] = (e0[p][k] + pmod[r] round_half_even(coeffs[p][k] scale)) mod q on data rows,
//                   e0[p][k] mod q on special rows
//   X[p][1][r][k] = e1[p][k] mod q
// with round_to_rns's rounding, wide range and sticky overflow flag.  small as sample_asym_small
// writes it; pmod[r] = P mod q_r for r < L; U [count][rows][n], X [count][2][rows][n].
hipError_t round_lift(ModView m, const AsymRows& rw, const uint64_t* pmod, const double* coeffs, double scale,
                      const int32_t* small, uint64_t* U, uint64_t* X, size_t n, size_t count, int* overflow,
                      hipStream_t s);

// X[p][j][r][k] = X[p][j][r][k] + U[p][r][k] pk[j][table_row(r)][k] mod q for j < 2, everything in
// NTT form; pk [2][rw.total][n] is only read, U[p] once for both products.
hipError_t pk_fma(ModView m, const AsymRows& rw, const uint64_t* pk, const uint64_t* U, uint64_t* X, size_t n,
                  size_t count, hipStream_t s);

// ct.at(p)[w] = src[p][w] for w < words: contiguous ciphertexts to their (strided or separate)
// places; nothing past `words` is written
hipError_t scatter_ct(const uint64_t* src, const CtChunk& ct, size_t words, size_t count, hipStream_t s);

}  // namespace phx
