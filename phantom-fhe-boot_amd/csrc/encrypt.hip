// encrypt.hip — batched symmetric and public-key encryption / decryption kernels for gfx950 (see
// encrypt.h).
//
// The kernels are streaming passes over [count][L][n] words with the chunk's ciphertexts in
// grid y (or z): each lane moves 16 bytes per access (two residues, two coefficients) or, where a
// keystream block is drawn, the 8 values of its block (64 bytes of residues, 32 of error).  A
// ChaCha20 / Salsa20 block is computed once per lane and serves all 8 of its values; the round and
// split kernel reads the error as data, so it draws nothing.
#include "encrypt.h"

#include "arith.h"

namespace phx {
namespace {

constexpr int kThreads = 256;

struct NonceChunk {
  uint64_t v[kCtChunkMax];
};
struct SeedChunk {
  SalsaSeed s[kCtChunkMax];
};

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// count in range, every start non-null and 16-byte aligned, the stride even and at least `words`
bool chunk_ok(const CtChunk& c, size_t count, size_t words) {
  if (count < 1 || count > static_cast<size_t>(kCtChunkMax)) return false;
  if (c.base) return aligned16(c.base) && c.stride % 2 == 0 && c.stride >= words;
  for (size_t p = 0; p < count; ++p)
    if (!c.ptr[p] || !aligned16(c.ptr[p])) return false;
  return true;
}

inline int log2_of(size_t n) { return 63 - __builtin_clzll(n); }
inline bool degree_ok(size_t n) { return n >= 8 && (n & (n - 1)) == 0 && n <= (size_t(1) << 20); }

// ---- error: one ChaCha20 block per lane = 8 coefficients (small_kernel<0>'s values) -----------
__global__ void __launch_bounds__(kThreads)
cbd_small_kernel(int32_t* __restrict__ out, uint32_t blocks, ChaChaKey key, NonceChunk nonces) {
  const uint32_t b = blockIdx.x * kThreads + threadIdx.x;
  if (b >= blocks) return;
  uint32_t w[16];
  chacha20_block(key, b, nonces.v[blockIdx.y], w);
  int v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t r = chacha_word64(w, i);
    v[i] = __popcll(r & 0x1FFFFFull) - __popcll((r >> 21) & 0x1FFFFFull);
  }
  int4* o = reinterpret_cast<int4*>(out + (static_cast<size_t>(blockIdx.y) * blocks + b) * 8);
  o[0] = make_int4(v[0], v[1], v[2], v[3]);
  o[1] = make_int4(v[4], v[5], v[6], v[7]);
}

// ---- round and split with the error subtracted ------------------------------------------------
constexpr int kRoundLimbs = 8;  // limbs per workgroup (grid y), as round_to_rns_kernel

// 2^e mod q, e < 1024
__device__ uint64_t pow2_mod(uint32_t e, uint64_t q, uint64_t r0, uint64_t r1) {
  uint64_t result = 1, base = 2 % q;
  for (int bit = 0; bit < 10; ++bit) {
    if ((e >> bit) & 1) result = mul_mod(result, base, q, r0, r1);
    base = mul_mod(base, base, q, r0, r1);
  }
  return result;
}

// |round_half_even(x)| = mant 2^sh (sh = 0 below 2^63), exactly as round_to_rns_kernel splits it
struct Rounded {
  uint64_t mant;
  uint32_t sh;
  bool neg, big, bad;
};
__device__ __forceinline__ Rounded round_coeff(double x) {
  Rounded c;
  c.bad = !(fabs(x) < 0x1p1000);  // NaN and infinities included
  const double r = c.bad ? 0.0 : rint(x);
  const double a = fabs(r);
  c.neg = r < 0;
  c.big = a >= 0x1p63;
  c.sh = 0;
  if (c.big) {
    const uint64_t bits = static_cast<uint64_t>(__double_as_longlong(a));
    c.mant = (bits & ((1ull << 52) - 1)) | (1ull << 52);
    c.sh = static_cast<uint32_t>(bits >> 52) - 1075u;
  } else {
    c.mant = static_cast<uint64_t>(a);
  }
  return c;
}
// (the rounded value - e) mod q, |e| < q
__device__ __forceinline__ uint64_t residue_minus(const Rounded& c, int e, uint64_t q, uint64_t r0, uint64_t r1) {
  uint64_t v = barrett_reduce_64(c.mant, q, r1);
  if (c.big) v = mul_mod(v, pow2_mod(c.sh, q, r0, r1), q, r0, r1);
  v = (c.neg && v) ? q - v : v;
  return e >= 0 ? sub_mod(v, static_cast<uint64_t>(e), q) : add_mod(v, static_cast<uint64_t>(-e), q);
}

__global__ void __launch_bounds__(kThreads)
round_minus_kernel(const uint64_t* __restrict__ modulus, const uint64_t* __restrict__ barrett,
                   const double* __restrict__ coeffs, double scale, const int32_t* __restrict__ err, const CtChunk out,
                   uint32_t n, int L, int* overflow) {
  const uint32_t k = 2 * (blockIdx.x * kThreads + threadIdx.x);
  if (k >= n) return;
  const int p = blockIdx.z;
  const size_t src = static_cast<size_t>(p) * n + k;
  const double2 x = *reinterpret_cast<const double2*>(coeffs + src);
  const int2 e = *reinterpret_cast<const int2*>(err + src);
  const Rounded c0 = round_coeff(x.x * scale), c1 = round_coeff(x.y * scale);
  if ((c0.bad || c1.bad) && overflow) *overflow = 1;
  const int l0 = blockIdx.y * kRoundLimbs;
  const int l1 = l0 + kRoundLimbs < L ? l0 + kRoundLimbs : L;
  uint64_t* o = out.at(p) + static_cast<size_t>(l0) * n + k;
  for (int i = l0; i < l1; ++i, o += n) {
    const uint64_t q = modulus[i], r0 = barrett[2 * i], r1 = barrett[2 * i + 1];
    *reinterpret_cast<ulonglong2*>(o) =
        make_ulonglong2(residue_minus(c0, e.x, q, r0, r1), residue_minus(c1, e.y, q, r0, r1));
  }
}

// ---- c1 = the expansion of its seed, c0 -= c1 s ----------------------------------------------
// uniform_salsa_kernel per ciphertext (thread t < (n / 8) L draws the 8 words of limb t / (n / 8)
// from the block of nonce t, rejection path included) with the finish in the same lane: `a` is
// multiplied into c0 from registers, so c1 is written and never read back.  The c0 and s loads come
// first, so that they can complete behind the Salsa20 rounds.
__global__ void __launch_bounds__(kThreads)
expand_finish_kernel(const uint64_t* __restrict__ q, const uint64_t* __restrict__ barrett,
                     const uint64_t* __restrict__ sk, uint32_t log_n, uint32_t L, const CtChunk ct,
                     const SeedChunk seeds) {
  const size_t per = (size_t(1) << log_n) >> 3, total = per * L, nl = static_cast<size_t>(L) << log_n;
  const size_t t = blockIdx.x * static_cast<size_t>(kThreads) + threadIdx.x;
  if (t >= total) return;
  const SalsaSeed& seed = seeds.s[blockIdx.y];
  const size_t l = t / per;
  const uint64_t ql = q[l], r0 = barrett[2 * l], r1 = barrett[2 * l + 1];
  uint64_t* c0 = ct.at(blockIdx.y) + 8 * t;
  ulonglong2 m[4], s[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    m[i] = *reinterpret_cast<const ulonglong2*>(c0 + 2 * i);
    s[i] = *reinterpret_cast<const ulonglong2*>(sk + 8 * t + 2 * i);
  }
  const uint64_t max_multiple = ~uint64_t(0) - barrett_reduce_64(~uint64_t(0), ql, r1) - 1;
  uint32_t w[16];
  salsa20_block(seed, t, w);
  uint64_t tries = 1;
  uint64_t v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    uint64_t r = static_cast<uint64_t>(w[2 * i]) | (static_cast<uint64_t>(w[2 * i + 1]) << 32);
    while (r > max_multiple) {
      salsa20_block(seed, t + tries * nl, w);
      ++tries;
      r = static_cast<uint64_t>(w[2 * i]) | (static_cast<uint64_t>(w[2 * i + 1]) << 32);
    }
    v[i] = barrett_reduce_64(r, ql, r1);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    *reinterpret_cast<ulonglong2*>(c0 + nl + 2 * i) = make_ulonglong2(v[2 * i], v[2 * i + 1]);
    *reinterpret_cast<ulonglong2*>(c0 + 2 * i) =
        make_ulonglong2(sub_mod(m[i].x, mul_mod(v[2 * i], s[i].x, ql, r0, r1), ql),
                        sub_mod(m[i].y, mul_mod(v[2 * i + 1], s[i].y, ql, r0, r1), ql));
  }
}

// ---- c0 + s (c1 + s c2) over the leading limbs -------------------------------------------------
template <int POLYS>
__global__ void __launch_bounds__(kThreads)
decrypt_dot_kernel(const uint64_t* __restrict__ q, const uint64_t* __restrict__ barrett,
                   const uint64_t* __restrict__ sk, const CtChunk in, uint32_t log_n, size_t words, size_t poly_stride,
                   uint64_t* __restrict__ out) {
  const size_t e = 2 * (blockIdx.x * static_cast<size_t>(kThreads) + threadIdx.x);
  if (e >= words) return;
  const size_t l = e >> log_n;
  const uint64_t ql = q[l], r0 = barrett[2 * l], r1 = barrett[2 * l + 1];
  const uint64_t* c = in.at(blockIdx.y) + e;
  const ulonglong2 s = *reinterpret_cast<const ulonglong2*>(sk + e);
  ulonglong2 acc = *reinterpret_cast<const ulonglong2*>(c + (POLYS - 1) * poly_stride);
#pragma unroll
  for (int t = POLYS - 2; t >= 0; --t) {
    const ulonglong2 ci = *reinterpret_cast<const ulonglong2*>(c + t * poly_stride);
    acc.x = add_mod(mul_mod(acc.x, s.x, ql, r0, r1), ci.x, ql);
    acc.y = add_mod(mul_mod(acc.y, s.y, ql, r0, r1), ci.y, ql);
  }
  *reinterpret_cast<ulonglong2*>(out + blockIdx.y * words + e) = acc;
}

// out[p][i] = word i (n / 8) of c1[p], i < 8 L
__global__ void __launch_bounds__(kThreads)
gather_c1_samples_kernel(const CtChunk ct, uint32_t n, uint32_t per_ct, uint64_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= per_ct) return;
  out[static_cast<size_t>(blockIdx.y) * per_ct + i] =
      ct.at(blockIdx.y)[static_cast<size_t>(per_ct / 8) * n + static_cast<size_t>(i) * (n / 8)];
}

dim3 pair_grid(size_t words, size_t count) {
  return dim3(static_cast<uint32_t>((words / 2 + kThreads - 1) / kThreads), static_cast<uint32_t>(count));
}

// ---- public-key encryption ---------------------------------------------------------------------
struct DrawChunk {
  uint64_t v[3 * kCtChunkMax];
};

// cbd_small_kernel over the draws of grid y, ternary where the kind says so
__global__ void __launch_bounds__(kThreads)
small_kernel(int32_t* __restrict__ out, uint32_t blocks, int kind, ChaChaKey key, DrawChunk nonces) {
  const uint32_t b = blockIdx.x * kThreads + threadIdx.x;
  if (b >= blocks) return;
  const bool ternary = kind == kSmallTernary || (kind == kSmallAsym && blockIdx.y % 3 == 0);
  uint32_t w[16];
  chacha20_block(key, b, nonces.v[blockIdx.y], w);
  int v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t r = chacha_word64(w, i);
    v[i] = ternary ? static_cast<int>(r % 3) - 1 : __popcll(r & 0x1FFFFFull) - __popcll((r >> 21) & 0x1FFFFFull);
  }
  int4* o = reinterpret_cast<int4*>(out + (static_cast<size_t>(blockIdx.y) * blocks + b) * 8);
  o[0] = make_int4(v[0], v[1], v[2], v[3]);
  o[1] = make_int4(v[4], v[5], v[6], v[7]);
}

// v mod q, |v| < q
__device__ __forceinline__ uint64_t signed_residue(int v, uint64_t q) {
  return v >= 0 ? static_cast<uint64_t>(v) : q - static_cast<uint64_t>(-v);
}

// One lane: two coefficients of ciphertext z over the kRoundLimbs rows of grid y.  The rounding is
// done once and serves every row; the three small samples are read as data.
__global__ void __launch_bounds__(kThreads)
round_lift_kernel(const uint64_t* __restrict__ modulus, const uint64_t* __restrict__ barrett, const AsymRows rw,
                  const uint64_t* __restrict__ pmod, const double* __restrict__ coeffs, double scale,
                  const int32_t* __restrict__ small, uint64_t* __restrict__ U, uint64_t* __restrict__ X, uint32_t n,
                  int* overflow) {
  const uint32_t k = 2 * (blockIdx.x * kThreads + threadIdx.x);
  if (k >= n) return;
  const size_t p = blockIdx.z;
  const double2 x = *reinterpret_cast<const double2*>(coeffs + p * n + k);
  const int32_t* sm = small + 3 * p * n + k;
  const int2 u = *reinterpret_cast<const int2*>(sm);
  const int2 e0 = *reinterpret_cast<const int2*>(sm + n);
  const int2 e1 = *reinterpret_cast<const int2*>(sm + 2 * static_cast<size_t>(n));
  const Rounded c0 = round_coeff(x.x * scale), c1 = round_coeff(x.y * scale);
  if ((c0.bad || c1.bad) && overflow) *overflow = 1;
  const int rows = rw.rows();
  const int r0 = blockIdx.y * kRoundLimbs;
  const int r1 = r0 + kRoundLimbs < rows ? r0 + kRoundLimbs : rows;
  const size_t poly = static_cast<size_t>(rows) * n;
  for (int r = r0; r < r1; ++r) {
    const int t = rw.table_row(r);
    const uint64_t q = modulus[t], b0 = barrett[2 * t], b1 = barrett[2 * t + 1];
    const size_t at = static_cast<size_t>(r) * n + k;
    uint64_t a0 = signed_residue(e0.x, q), a1 = signed_residue(e0.y, q);
    if (r < rw.L) {
      const uint64_t pq = pmod[r];
      a0 = add_mod(a0, mul_mod(residue_minus(c0, 0, q, b0, b1), pq, q, b0, b1), q);
      a1 = add_mod(a1, mul_mod(residue_minus(c1, 0, q, b0, b1), pq, q, b0, b1), q);
    }
    *reinterpret_cast<ulonglong2*>(U + p * poly + at) = make_ulonglong2(signed_residue(u.x, q), signed_residue(u.y, q));
    *reinterpret_cast<ulonglong2*>(X + 2 * p * poly + at) = make_ulonglong2(a0, a1);
    *reinterpret_cast<ulonglong2*>(X + (2 * p + 1) * poly + at) =
        make_ulonglong2(signed_residue(e1.x, q), signed_residue(e1.y, q));
  }
}

// One lane: two words of row r of ciphertext y, both products from one load of U
__global__ void __launch_bounds__(kThreads)
pk_fma_kernel(const uint64_t* __restrict__ modulus, const uint64_t* __restrict__ barrett, const AsymRows rw,
              const uint64_t* __restrict__ pk, const uint64_t* __restrict__ U, uint64_t* __restrict__ X,
              uint32_t log_n, size_t words) {
  const size_t e = 2 * (blockIdx.x * static_cast<size_t>(kThreads) + threadIdx.x);
  if (e >= words) return;
  const int r = static_cast<int>(e >> log_n);
  const int t = rw.table_row(r);
  const uint64_t q = modulus[t], b0 = barrett[2 * t], b1 = barrett[2 * t + 1];
  const size_t p = blockIdx.y;
  const size_t key_at = (static_cast<size_t>(t) << log_n) + (e & ((size_t(1) << log_n) - 1));
  const ulonglong2 u = *reinterpret_cast<const ulonglong2*>(U + p * words + e);
  const ulonglong2 k0 = *reinterpret_cast<const ulonglong2*>(pk + key_at);
  const ulonglong2 k1 = *reinterpret_cast<const ulonglong2*>(pk + (static_cast<size_t>(rw.total) << log_n) + key_at);
  uint64_t* x0 = X + 2 * p * words + e;
  uint64_t* x1 = x0 + words;
  const ulonglong2 a = *reinterpret_cast<const ulonglong2*>(x0);
  const ulonglong2 b = *reinterpret_cast<const ulonglong2*>(x1);
  *reinterpret_cast<ulonglong2*>(x0) = make_ulonglong2(add_mod(a.x, mul_mod(u.x, k0.x, q, b0, b1), q),
                                                       add_mod(a.y, mul_mod(u.y, k0.y, q, b0, b1), q));
  *reinterpret_cast<ulonglong2*>(x1) = make_ulonglong2(add_mod(b.x, mul_mod(u.x, k1.x, q, b0, b1), q),
                                                       add_mod(b.y, mul_mod(u.y, k1.y, q, b0, b1), q));
}

__global__ void __launch_bounds__(kThreads)
scatter_ct_kernel(const uint64_t* __restrict__ src, const CtChunk ct, size_t words) {
  const size_t e = 2 * (blockIdx.x * static_cast<size_t>(kThreads) + threadIdx.x);
  if (e >= words) return;
  *reinterpret_cast<ulonglong2*>(ct.at(blockIdx.y) + e) =
      *reinterpret_cast<const ulonglong2*>(src + blockIdx.y * words + e);
}

bool rows_ok(const AsymRows& rw) {
  return rw.L >= 1 && rw.alpha >= 1 && rw.first_p >= rw.L && rw.total == rw.first_p + rw.alpha && rw.total <= 0xffff;
}

}  // namespace

hipError_t sample_cbd_small(int32_t* out, size_t n, const ChaChaKey& key, const uint64_t* nonces, size_t count,
                            hipStream_t s) {
  if (!out || !nonces || !aligned16(out) || !degree_ok(n) || count < 1 || count > static_cast<size_t>(kCtChunkMax))
    return hipErrorInvalidValue;
  NonceChunk nc{};
  for (size_t p = 0; p < count; ++p) nc.v[p] = nonces[p];
  const uint32_t blocks = static_cast<uint32_t>(n / 8);
  hipLaunchKernelGGL(cbd_small_kernel, dim3((blocks + kThreads - 1) / kThreads, static_cast<uint32_t>(count)),
                     dim3(kThreads), 0, s, out, blocks, key, nc);
  return hipGetLastError();
}

hipError_t round_to_rns_minus(ModView m, const double* coeffs, double scale, const int32_t* e, const CtChunk& out,
                              size_t n, size_t L, size_t count, int* overflow, hipStream_t s) {
  if (!m.q || !m.barrett || !coeffs || !e || !aligned16(coeffs) || !aligned16(e) || !degree_ok(n) || L < 1 ||
      L > 0xffff || !chunk_ok(out, count, L * n))
    return hipErrorInvalidValue;
  const dim3 grid(static_cast<uint32_t>((n / 2 + kThreads - 1) / kThreads),
                  static_cast<uint32_t>((L + kRoundLimbs - 1) / kRoundLimbs), static_cast<uint32_t>(count));
  hipLaunchKernelGGL(round_minus_kernel, grid, dim3(kThreads), 0, s, m.q, m.barrett, coeffs, scale, e, out,
                     static_cast<uint32_t>(n), static_cast<int>(L), overflow);
  return hipGetLastError();
}

hipError_t expand_and_finish(ModView m, const uint8_t* seeds, const uint64_t* sk, const CtChunk& ct, size_t n,
                             size_t L, size_t count, hipStream_t s) {
  if (!m.q || !m.barrett || !seeds || !sk || !aligned16(sk) || !degree_ok(n) || L < 1 || L > 0xffff ||
      !chunk_ok(ct, count, 2 * L * n))
    return hipErrorInvalidValue;
  SeedChunk sc{};
  for (size_t p = 0; p < count; ++p) sc.s[p] = salsa_seed(seeds + 64 * p);
  const size_t total = n / 8 * L;
  hipLaunchKernelGGL(expand_finish_kernel,
                     dim3(static_cast<uint32_t>((total + kThreads - 1) / kThreads), static_cast<uint32_t>(count)),
                     dim3(kThreads), 0, s, m.q, m.barrett, sk, static_cast<uint32_t>(log2_of(n)),
                     static_cast<uint32_t>(L), ct, sc);
  return hipGetLastError();
}

hipError_t gather_c1_samples(const CtChunk& ct, size_t n, size_t L, size_t count, uint64_t* out, hipStream_t s) {
  if (!out || !degree_ok(n) || L < 1 || L > 0xffff || !chunk_ok(ct, count, 2 * L * n)) return hipErrorInvalidValue;
  const uint32_t per_ct = static_cast<uint32_t>(8 * L);
  hipLaunchKernelGGL(gather_c1_samples_kernel, dim3((per_ct + kThreads - 1) / kThreads, static_cast<uint32_t>(count)),
                     dim3(kThreads), 0, s, ct, static_cast<uint32_t>(n), per_ct, out);
  return hipGetLastError();
}

hipError_t sample_small(int32_t* out, size_t n, SmallKind kind, const ChaChaKey& key, const uint64_t* nonces,
                        size_t draws, hipStream_t s) {
  if (!out || !nonces || !aligned16(out) || !degree_ok(n) || draws < 1 || draws > static_cast<size_t>(3 * kCtChunkMax) ||
      kind < kSmallCbd || kind > kSmallAsym || (kind == kSmallAsym && draws % 3))
    return hipErrorInvalidValue;
  DrawChunk nc{};
  for (size_t d = 0; d < draws; ++d) nc.v[d] = nonces[d];
  const uint32_t blocks = static_cast<uint32_t>(n / 8);
  hipLaunchKernelGGL(small_kernel, dim3((blocks + kThreads - 1) / kThreads, static_cast<uint32_t>(draws)),
                     dim3(kThreads), 0, s, out, blocks, static_cast<int>(kind), key, nc);
  return hipGetLastError();
}

hipError_t round_lift(ModView m, const AsymRows& rw, const uint64_t* pmod, const double* coeffs, double scale,
                      const int32_t* small, uint64_t* U, uint64_t* X, size_t n, size_t count, int* overflow,
                      hipStream_t s) {
  if (!m.q || !m.barrett || !pmod || !coeffs || !small || !U || !X || !aligned16(coeffs) || !aligned16(small) ||
      !aligned16(U) || !aligned16(X) || !degree_ok(n) || !rows_ok(rw) || count < 1 ||
      count > static_cast<size_t>(kCtChunkMax))
    return hipErrorInvalidValue;
  const dim3 grid(static_cast<uint32_t>((n / 2 + kThreads - 1) / kThreads),
                  static_cast<uint32_t>((rw.rows() + kRoundLimbs - 1) / kRoundLimbs), static_cast<uint32_t>(count));
  hipLaunchKernelGGL(round_lift_kernel, grid, dim3(kThreads), 0, s, m.q, m.barrett, rw, pmod, coeffs, scale, small, U, X,
                     static_cast<uint32_t>(n), overflow);
  return hipGetLastError();
}

hipError_t pk_fma(ModView m, const AsymRows& rw, const uint64_t* pk, const uint64_t* U, uint64_t* X, size_t n,
                  size_t count, hipStream_t s) {
  if (!m.q || !m.barrett || !pk || !U || !X || !aligned16(pk) || !aligned16(U) || !aligned16(X) || !degree_ok(n) ||
      !rows_ok(rw) || count < 1 || count > static_cast<size_t>(kCtChunkMax))
    return hipErrorInvalidValue;
  const size_t words = static_cast<size_t>(rw.rows()) * n;
  hipLaunchKernelGGL(pk_fma_kernel, pair_grid(words, count), dim3(kThreads), 0, s, m.q, m.barrett, rw, pk, U, X,
                     static_cast<uint32_t>(log2_of(n)), words);
  return hipGetLastError();
}

hipError_t scatter_ct(const uint64_t* src, const CtChunk& ct, size_t words, size_t count, hipStream_t s) {
  if (!src || !aligned16(src) || words < 2 || words % 2 || !chunk_ok(ct, count, words)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(scatter_ct_kernel, pair_grid(words, count), dim3(kThreads), 0, s, src, ct, words);
  return hipGetLastError();
}

hipError_t decrypt_dot(ModView m, const uint64_t* sk, const CtChunk& in, size_t n, size_t ct_limbs, size_t polys,
                       size_t limbs, size_t count, uint64_t* out, hipStream_t s) {
  if (!m.q || !m.barrett || !sk || !out || !aligned16(sk) || !aligned16(out) || !degree_ok(n) || polys < 2 ||
      polys > 3 || limbs < 1 || limbs > ct_limbs || ct_limbs > 0xffff || !chunk_ok(in, count, polys * ct_limbs * n))
    return hipErrorInvalidValue;
  const size_t words = limbs * n, poly_stride = ct_limbs * n;
  const uint32_t log_n = static_cast<uint32_t>(log2_of(n));
  if (polys == 2)
    hipLaunchKernelGGL(decrypt_dot_kernel<2>, pair_grid(words, count), dim3(kThreads), 0, s, m.q, m.barrett, sk, in,
                       log_n, words, poly_stride, out);
  else
    hipLaunchKernelGGL(decrypt_dot_kernel<3>, pair_grid(words, count), dim3(kThreads), 0, s, m.q, m.barrett, sk, in,
                       log_n, words, poly_stride, out);
  return hipGetLastError();
}

}  // namespace phx
