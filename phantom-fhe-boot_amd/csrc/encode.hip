// encode.hip — CKKS encode / decode kernels for gfx950 (see encode.h).
//
// Embedding.  One size-n complex transform per plaintext, radix 2, decimation in time on
// bit-reversed input: the butterflies, their order and their twiddles (read from the zeta table,
// never recomputed) are those of PhantomCKKSEncoder::fft, so both paths round alike.  Stage `len`
// couples elements len/2 apart.  The first s1 = ceil(log n / 2) stages stay inside aligned blocks
// of 2^s1 elements: pass A keeps a tile of kTile contiguous elements in LDS and runs them all.  The
// last s2 = log n - s1 stages couple elements that agree in their low s1 index bits: pass B keeps
// the 2^s2 elements of kTile / 2^s2 neighbouring columns in LDS.  A plaintext crosses HBM twice
// (16 n bytes each way per pass); everything else happens in LDS.
//
// The slot placement, the zeta^k pre-twist (forward) and the zeta^-k post-twist with 1/n
// (inverse) are folded into the first load and the last store.
#include "encode.h"

#include "arith.h"

namespace phx {
namespace {

constexpr int kEmbedThreads = 256;
constexpr uint32_t kTile = 2048;  // complex values per workgroup: 32 KiB of LDS

__device__ __forceinline__ double2 cmul(double2 a, double2 w) {
  return make_double2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x);
}

__device__ __forceinline__ void bfly(double2& a, double2& b, double2 w) {
  const double2 u = a, v = cmul(b, w);
  a = make_double2(u.x + v.x, u.y + v.y);
  b = make_double2(u.x - v.x, u.y - v.y);
}

struct EmbedArgs {
  const double2* zeta;
  const uint32_t* slot_of;
  uint32_t n;
  int log_n, s1, s2;
  uint32_t tile;  // min(n, kTile)
  // inverse input / forward output
  const double2* values;
  double2* slots_out;
  uint32_t num_values, ns;
  // forward input / inverse output
  const double* coeffs_in;
  double* coeffs_out;
  double mul;
  double2* work;
};

// Pass A: load (placing slots or twisting coefficients), stages 2 .. 2^s1, store to work.
template <bool INVERSE>
__global__ void __launch_bounds__(kEmbedThreads) embed_pass_a(const EmbedArgs a) {
  extern __shared__ double2 lds[];
  const uint32_t base = blockIdx.x * a.tile;
  const size_t pl = blockIdx.y;
  for (uint32_t l = threadIdx.x; l < a.tile; l += kEmbedThreads) {
    const uint32_t m = __brev(base + l) >> (32 - a.log_n);
    double2 v;
    if (INVERSE) {
      const uint32_t e = a.slot_of[m];
      const uint32_t idx = (e & ~EmbedTables::kConjBit) & (a.ns - 1);
      v = idx < a.num_values ? a.values[pl * a.num_values + idx] : make_double2(0.0, 0.0);
      if (e & EmbedTables::kConjBit) v.y = -v.y;
    } else {
      const double c = a.coeffs_in[pl * a.n + m] * a.mul;
      const double2 z = a.zeta[m];
      v = make_double2(z.x * c, z.y * c);
    }
    lds[l] = v;
  }
  __syncthreads();
  for (int s = 1; s <= a.s1; ++s) {
    const uint32_t h = 1u << (s - 1);
    const int tw_shift = a.log_n + 1 - s;  // step = 2n / len
    for (uint32_t b = threadIdx.x; b < a.tile / 2; b += kEmbedThreads) {
      const uint32_t j = b & (h - 1);
      const uint32_t i = ((b >> (s - 1)) << s) + j;
      double2 w = a.zeta[j << tw_shift];
      if (INVERSE) w.y = -w.y;
      double2 x = lds[i], y = lds[i + h];
      bfly(x, y, w);
      lds[i] = x;
      lds[i + h] = y;
    }
    __syncthreads();
  }
  for (uint32_t l = threadIdx.x; l < a.tile; l += kEmbedThreads) a.work[pl * a.n + base + l] = lds[l];
}

// Pass B: columns lo0 .. lo0 + T of the [2^s2][2^s1] view, stages 2^(s1+1) .. n, final store.
template <bool INVERSE>
__global__ void __launch_bounds__(kEmbedThreads) embed_pass_b(const EmbedArgs a) {
  extern __shared__ double2 lds[];
  const uint32_t T = a.tile >> a.s2, lo0 = blockIdx.x * T;
  const int log_t = 31 - __clz(T);
  const size_t pl = blockIdx.y;
  for (uint32_t l = threadIdx.x; l < a.tile; l += kEmbedThreads) {
    const uint32_t g = ((l >> log_t) << a.s1) | (lo0 + (l & (T - 1)));
    lds[l] = a.work[pl * a.n + g];
  }
  __syncthreads();
  for (int m = 1; m <= a.s2; ++m) {
    const uint32_t hh = 1u << (m - 1);
    const int tw_shift = a.log_n + 1 - a.s1 - m;
    for (uint32_t b = threadIdx.x; b < a.tile / 2; b += kEmbedThreads) {
      const uint32_t t = b & (T - 1), bh = b >> log_t;
      const uint32_t jh = bh & (hh - 1);
      const uint32_t ih = ((bh >> (m - 1)) << m) + jh;
      const uint32_t i0 = (ih << log_t) + t, i1 = i0 + (hh << log_t);
      const uint32_t j = (jh << a.s1) + lo0 + t;
      double2 w = a.zeta[j << tw_shift];
      if (INVERSE) w.y = -w.y;
      double2 x = lds[i0], y = lds[i1];
      bfly(x, y, w);
      lds[i0] = x;
      lds[i1] = y;
    }
    __syncthreads();
  }
  const double inv_n = 1.0 / static_cast<double>(a.n);
  for (uint32_t l = threadIdx.x; l < a.tile; l += kEmbedThreads) {
    const uint32_t g = ((l >> log_t) << a.s1) | (lo0 + (l & (T - 1)));
    const double2 v = lds[l];
    if (INVERSE) {
      const double2 z = a.zeta[g];  // Re(conj(zeta^g) v) / n
      a.coeffs_out[pl * a.n + g] = (z.x * v.x - (-z.y) * v.y) * inv_n;
    } else {
      const uint32_t e = a.slot_of[g];
      if (e < a.ns) a.slots_out[pl * a.ns + e] = v;  // conjugate roots carry kConjBit: never below ns
    }
  }
}

template <bool INVERSE>
hipError_t launch_embed(EmbedArgs a, size_t count, hipStream_t stream) {
  if (count == 0) return hipSuccess;
  // both passes need their stage group inside one tile: 2^s1 <= kTile and 2^s2 <= kTile
  if (a.log_n < 2 || a.log_n > 20 || count > 65535) return hipErrorInvalidValue;
  a.s1 = (a.log_n + 1) / 2;
  a.s2 = a.log_n - a.s1;
  a.tile = a.n < kTile ? a.n : kTile;
  const size_t lds = a.tile * sizeof(double2);
  const dim3 block(kEmbedThreads);
  hipLaunchKernelGGL(embed_pass_a<INVERSE>, dim3(a.n / a.tile, static_cast<uint32_t>(count)), block, lds, stream, a);
  const uint32_t T = a.tile >> a.s2;
  hipLaunchKernelGGL(embed_pass_b<INVERSE>, dim3((1u << a.s1) / T, static_cast<uint32_t>(count)), block, lds, stream,
                     a);
  return hipGetLastError();
}

EmbedArgs base_args(const EmbedTables& t, size_t sparse_slots, double2* work) {
  EmbedArgs a{};
  a.zeta = t.zeta;
  a.slot_of = t.slot_of;
  a.n = static_cast<uint32_t>(t.n);
  a.log_n = t.log_n;
  a.ns = static_cast<uint32_t>(sparse_slots ? sparse_slots : t.n / 2);
  a.mul = 1.0;
  a.work = work;
  return a;
}

}  // namespace

// the grid's y extent bounds one launch; longer batches go in slices
constexpr size_t kEmbedBatch = 32768;

hipError_t embed_inverse(const EmbedTables& t, const double2* in, size_t num_values, size_t sparse_slots,
                         double* coeffs, double2* work, size_t count, hipStream_t stream) {
  EmbedArgs a = base_args(t, sparse_slots, work);
  if ((a.ns & (a.ns - 1)) || a.ns > t.n / 2 || num_values > a.ns) return hipErrorInvalidValue;
  a.num_values = static_cast<uint32_t>(num_values);
  for (size_t p = 0; p < count; p += kEmbedBatch) {
    a.values = in + p * num_values;
    a.coeffs_out = coeffs + p * t.n;
    const hipError_t e = launch_embed<true>(a, count - p < kEmbedBatch ? count - p : kEmbedBatch, stream);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t embed_forward(const EmbedTables& t, const double* coeffs, double mul, size_t sparse_slots, double2* out,
                         double2* work, size_t count, hipStream_t stream) {
  EmbedArgs a = base_args(t, sparse_slots, work);
  if ((a.ns & (a.ns - 1)) || a.ns > t.n / 2) return hipErrorInvalidValue;
  a.mul = mul;
  for (size_t p = 0; p < count; p += kEmbedBatch) {
    a.coeffs_in = coeffs + p * t.n;
    a.slots_out = out + p * a.ns;
    const hipError_t e = launch_embed<false>(a, count - p < kEmbedBatch ? count - p : kEmbedBatch, stream);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// ---- round and split ---------------------------------------------------------------------------
namespace {

constexpr int kRoundThreads = 256;
constexpr int kRoundLimbs = 8;  // limbs per workgroup (grid y): the coefficient is re-read from L2

__device__ __forceinline__ int map_row(const LimbMap& m, int i) {
  return i < m.split ? m.first_a + i : m.first_b + (i - m.split);
}

// 2^e mod q, e < 1024
__device__ uint64_t pow2_mod(uint32_t e, uint64_t q, uint64_t r0, uint64_t r1) {
  uint64_t result = 1, base = 2 % q;
  for (int bit = 0; bit < 10; ++bit) {
    if ((e >> bit) & 1) result = mul_mod(result, base, q, r0, r1);
    base = mul_mod(base, base, q, r0, r1);
  }
  return result;
}

__global__ void __launch_bounds__(kRoundThreads)
round_to_rns_kernel(const uint64_t* __restrict__ modulus, const uint64_t* __restrict__ barrett,
                    const double* __restrict__ coeffs, double scale, uint64_t* __restrict__ out, const LimbMap map,
                    uint32_t n, int log_n, size_t total, int* overflow) {
  const size_t idx = static_cast<size_t>(blockIdx.x) * kRoundThreads + threadIdx.x;
  if (idx >= total) return;
  const size_t p = idx >> log_n;
  const uint32_t k = static_cast<uint32_t>(idx) & (n - 1);
  const double x = coeffs[idx] * scale;
  const bool bad = !(fabs(x) < 0x1p1000);  // NaN and infinities included
  if (bad && overflow) *overflow = 1;
  const double r = bad ? 0.0 : rint(x);  // round half to even
  const double a = fabs(r);
  const bool neg = r < 0;
  const bool big = a >= 0x1p63;
  // a = mant 2^sh for the wide range (mant < 2^53, 11 <= sh < 948); a itself below 2^63
  uint64_t mant = 0;
  uint32_t sh = 0;
  if (big) {
    const uint64_t bits = static_cast<uint64_t>(__double_as_longlong(a));
    mant = (bits & ((1ull << 52) - 1)) | (1ull << 52);
    sh = static_cast<uint32_t>(bits >> 52) - 1075u;
  } else {
    mant = static_cast<uint64_t>(a);
  }
  const int l0 = blockIdx.y * kRoundLimbs;
  const int l1 = l0 + kRoundLimbs < map.num_limbs ? l0 + kRoundLimbs : map.num_limbs;
  uint64_t* o = out + (p * map.num_limbs + l0) * n + k;
  for (int i = l0; i < l1; ++i, o += n) {
    const int row = map_row(map, i);
    const uint64_t q = modulus[row], r0 = barrett[2 * row], r1 = barrett[2 * row + 1];
    uint64_t v = barrett_reduce_64(mant, q, r1);
    if (big) v = mul_mod(v, pow2_mod(sh, q, r0, r1), q, r0, r1);
    *o = (neg && v) ? q - v : v;
  }
}

}  // namespace

hipError_t round_to_rns(const NttTables& t, const double* coeffs, double scale, uint64_t* out, const LimbMap& map,
                        size_t count, int* overflow, hipStream_t stream) {
  if (count == 0 || map.num_limbs == 0) return hipSuccess;
  const size_t total = count * t.n;
  const size_t blocks = (total + kRoundThreads - 1) / kRoundThreads;
  if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
  const dim3 grid(static_cast<uint32_t>(blocks), (map.num_limbs + kRoundLimbs - 1) / kRoundLimbs);
  hipLaunchKernelGGL(round_to_rns_kernel, grid, dim3(kRoundThreads), 0, stream, t.modulus, t.barrett, coeffs, scale,
                     out, map, static_cast<uint32_t>(t.n), t.log_n, total, overflow);
  return hipGetLastError();
}

// ---- compose -----------------------------------------------------------------------------------
namespace {

constexpr int kComposeThreads = 64;  // one wave; each lane keeps its L digits in a private LDS column

// double-double: value hi + lo with |lo| <= ulp(hi) / 2.  The products use explicit fused
// multiply-adds for their exact error terms (a requested operation, not a contraction).
struct dd {
  double hi, lo;
};
__device__ __forceinline__ dd fast_two_sum(double a, double b) {  // |a| >= |b|
  const double s = a + b;
  return {s, b - (s - a)};
}
__device__ __forceinline__ dd two_sum(double a, double b) {
  const double s = a + b, bb = s - a;
  return {s, (a - (s - bb)) + (b - bb)};
}
__device__ __forceinline__ dd dd_add(dd a, dd b) {
  dd s = two_sum(a.hi, b.hi);
  s.lo += a.lo + b.lo;
  return fast_two_sum(s.hi, s.lo);
}
__device__ __forceinline__ dd dd_mul(dd a, dd b) {
  const double p = a.hi * b.hi;
  double e = __builtin_fma(a.hi, b.hi, -p);
  e += a.hi * b.lo + a.lo * b.hi;
  return fast_two_sum(p, e);
}
// exact for u < 2^63
__device__ __forceinline__ dd dd_from_u64(uint64_t u) {
  const double hi = static_cast<double>(u);
  const double lo = static_cast<double>(static_cast<int64_t>(u - static_cast<uint64_t>(hi)));
  return {hi, lo};
}

__global__ void __launch_bounds__(kComposeThreads)
compose_kernel(const uint64_t* __restrict__ modulus, const ComposeTables c, const uint64_t* __restrict__ res,
               double mul, double* __restrict__ coeffs, uint32_t n, int log_n, size_t total) {
  extern __shared__ uint64_t dig_lds[];  // [L][kComposeThreads]
  const size_t idx = static_cast<size_t>(blockIdx.x) * kComposeThreads + threadIdx.x;
  if (idx >= total) return;  // no barrier below: lanes only touch their own column
  const int L = c.L;
  const size_t p = idx >> log_n;
  const uint32_t k = static_cast<uint32_t>(idx) & (n - 1);
  const uint64_t* r = res + p * L * n + k;
  uint64_t* dig = dig_lds + threadIdx.x;
  // Garner: digit i = (r_i - sum_{j<i} digit_j q_0..q_{j-1}) (q_0..q_{i-1})^-1 mod q_i
  for (int i = 0; i < L; ++i) {
    const uint64_t q = modulus[i];
    uint64_t acc = 0;  // in [0, 2q)
    for (int j = 0; j < i; ++j) {
      acc += mul_shoup_lazy(dig[j * kComposeThreads], c.prefix[i * L + j], c.prefix_shoup[i * L + j], q);
      acc = csub(acc, 2 * q);
    }
    acc = csub(acc, q);
    const uint64_t d = sub_mod(r[static_cast<size_t>(i) * n], acc, q);
    dig[i * kComposeThreads] = mul_shoup(d, c.inv_prefix[i], c.inv_prefix[L + i], q);
  }
  // x > (Q - 1) / 2 ?  compare mixed-radix digits from the top
  int cmp = 0;
  for (int i = L - 1; i >= 0; --i) {
    const uint64_t d = dig[i * kComposeThreads], h = c.half_digits[i];
    if (cmp == 0 && d != h) cmp = d > h ? 1 : -1;
  }
  if (cmp > 0) {  // Q - x: digits (q_i - 1 - d_i) + 1 with carry
    uint64_t carry = 1;
    for (int i = 0; i < L; ++i) {
      const uint64_t q = modulus[i];
      uint64_t d = q - 1 - dig[i * kComposeThreads] + carry;
      carry = d >= q ? 1 : 0;
      if (carry) d -= q;
      dig[i * kComposeThreads] = d;
    }
  }
  // Horner from the top digit: every term is non-negative, so nothing cancels
  dd v = dd_from_u64(dig[(L - 1) * kComposeThreads]);
  for (int i = L - 2; i >= 0; --i) v = dd_add(dd_mul(v, dd_from_u64(modulus[i])), dd_from_u64(dig[i * kComposeThreads]));
  coeffs[idx] = (cmp > 0 ? -v.hi : v.hi) * mul;
}

}  // namespace

hipError_t compose_centred(const NttTables& t, const ComposeTables& c, const uint64_t* res, double mul, double* coeffs,
                           size_t count, hipStream_t stream) {
  if (count == 0) return hipSuccess;
  if (c.L < 1 || c.L > kMaxComposeLimbs) return hipErrorInvalidValue;
  const size_t total = count * t.n;
  const size_t blocks = (total + kComposeThreads - 1) / kComposeThreads;
  if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
  hipLaunchKernelGGL(compose_kernel, dim3(static_cast<uint32_t>(blocks)), dim3(kComposeThreads),
                     static_cast<size_t>(c.L) * kComposeThreads * sizeof(uint64_t), stream, t.modulus, c, res, mul,
                     coeffs, static_cast<uint32_t>(t.n), t.log_n, total);
  return hipGetLastError();
}

}  // namespace phx
