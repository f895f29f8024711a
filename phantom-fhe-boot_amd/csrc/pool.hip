// pool.hip — ct_mix (ckks.h): linear combinations of ciphertexts with per-limb scalars, the
// channel-mixing half of the hoisted average pooling + fully connected layer (host/avgpool.h).
#include "ckks.h"

#include "arith.h"

namespace phx {
namespace {

constexpr int kBlock = 256;

// 8-byte load that is always a global (not FLAT) instruction, also through a pointer read from a table
using GU64 = __attribute__((address_space(1))) unsigned long long;
__device__ __forceinline__ uint64_t ldg(const uint64_t* p) { return *(const GU64*)p; }

// grid: x over the 2 n elements (p, e) of a limb, y = limb, z = output tile (MT outputs from z MT)
template <int MT>
__global__ __launch_bounds__(kBlock) void ct_mix_kernel(MixArgs a, uint32_t log_n) {
  const size_t n = size_t(1) << log_n;
  const size_t e = blockIdx.x * (size_t)kBlock + threadIdx.x;
  if (e >= 2 * n) return;
  const uint32_t l = blockIdx.y, m0 = blockIdx.z * MT;
  const uint32_t p = e >= n ? 1 : 0;
  const size_t ln = static_cast<size_t>(a.L) << log_n;
  const size_t off = p * ln + (static_cast<size_t>(l) << log_n) + (e - p * n);  // inside a ciphertext
  const uint64_t q = a.q[l], r0 = a.barrett[2 * l], r1 = a.barrett[2 * l + 1];
  const uint32_t m_pad = gridDim.z * MT;
  const uint64_t* __restrict__ cf = a.coef + static_cast<size_t>(l) * a.K * m_pad + m0;
  u128 acc[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) acc[m] = u128{0, 0};
  for (uint32_t kb = 0; kb < a.K; kb += kMixBlock) {
    const uint32_t kend = min(a.K, kb + kMixBlock);
#pragma unroll 4
    for (uint32_t k = kb; k < kend; ++k) {
      const uint64_t* in = a.ins ? a.ins[k] : a.in0 + k * a.in_stride;
      const uint64_t x = ldg(in + off);
      const uint64_t* __restrict__ c = cf + static_cast<size_t>(k) * m_pad;
#pragma unroll
      for (int m = 0; m < MT; ++m) add128(acc[m], mul_wide(x, c[m]));
    }
    // at most q - 1 + 32 (q - 1)^2 < 2^128 for q < 2^61: reduce and carry on
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = u128{barrett_reduce_128(acc[m], q, r0, r1), 0};
  }
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    if (m0 + m < a.M) {  // the last tile's padding
      uint64_t v = acc[m].lo;
      if (p == 0 && a.cadd) v = add_mod(v, a.cadd[static_cast<size_t>(m0 + m) * a.L + l], q);
      uint64_t* out = a.outs ? a.outs[m0 + m] : a.out0 + (m0 + m) * a.out_stride;
      out[off] = v;
    }
  }
}

}  // namespace

hipError_t ct_mix(const MixArgs& a, size_t n, hipStream_t s) {
  if (a.K < 1 || a.M < 1 || a.L < 1 || a.L > 65535 || !a.coef || !a.q || !a.barrett || (!a.ins && !a.in0) ||
      (!a.outs && !a.out0) || n < 1 || (n & (n - 1)))
    return hipErrorInvalidValue;
  const size_t tiles = mix_tiles(a.M), mt = mix_tile(a.M);
  if (tiles > 65535) return hipErrorInvalidValue;
  const dim3 grid(static_cast<unsigned>((2 * n + kBlock - 1) / kBlock), a.L, static_cast<unsigned>(tiles));
  const uint32_t log_n = __builtin_ctzll(n);
  switch (mt) {
#define PHX_MIX_CASE(MT) \
  case MT: ct_mix_kernel<MT><<<grid, kBlock, 0, s>>>(a, log_n); break;
    PHX_MIX_CASE(1) PHX_MIX_CASE(2) PHX_MIX_CASE(3) PHX_MIX_CASE(4) PHX_MIX_CASE(5) PHX_MIX_CASE(6)
    PHX_MIX_CASE(7) PHX_MIX_CASE(8) PHX_MIX_CASE(9) PHX_MIX_CASE(10) PHX_MIX_CASE(11) PHX_MIX_CASE(12)
    PHX_MIX_CASE(13) PHX_MIX_CASE(14) PHX_MIX_CASE(15) PHX_MIX_CASE(16)
#undef PHX_MIX_CASE
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace phx
