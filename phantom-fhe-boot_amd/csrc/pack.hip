// pack.hip — ct_pack and ct_split (ckks.h): the monomial interleave of sparse-packed channels into one
// ciphertext and one level of the rotation tree that takes them apart again (host/pack.h).  Both are
// element-wise passes over [2][L][n] NTT-form ciphertexts, 16 bytes per thread and access.
#include "ckks.h"

#include "arith.h"

namespace phx {
namespace {

constexpr int kBlock = 256;

// 16-byte accesses that are always global (not FLAT) instructions, also through a pointer read from a table
typedef unsigned long long v2u64 __attribute__((ext_vector_type(2)));
using GV2 = __attribute__((address_space(1))) v2u64;
__device__ __forceinline__ v2u64 ld2(const uint64_t* p) { return *(const GV2*)p; }
__device__ __forceinline__ void st2(uint64_t* p, uint64_t x, uint64_t y) {
  v2u64 v;
  v.x = x;
  v.y = y;
  *(GV2*)p = v;
}

// thread i owns words 2 i, 2 i + 1 of a ciphertext's 2 L n; they share a limb (n >= 2)
struct Where {
  size_t e, we;  // offset inside the ciphertext, inside a [L][n] table
  uint32_t l;
};
__device__ __forceinline__ Where where(size_t i, uint32_t L, uint32_t log_n) {
  const size_t ln = static_cast<size_t>(L) << log_n, e = 2 * i, we = e >= ln ? e - ln : e;
  return {e, we, static_cast<uint32_t>(we >> log_n)};
}

// Horner from the top channel down: acc = acc w + in_c, every step fully reduced (mul_mod's operands
// are below q whatever the inputs below q are)
__global__ __launch_bounds__(kBlock) void ct_pack_kernel(PackArgs a, uint32_t log_n) {
  const size_t i = blockIdx.x * (size_t)kBlock + threadIdx.x;
  if (i >= (static_cast<size_t>(a.L) << log_n)) return;
  const Where at = where(i, a.L, log_n);
  const uint64_t q = a.q[at.l], r0 = a.barrett[2 * at.l], r1 = a.barrett[2 * at.l + 1];
  auto in = [&](int c) { return (a.table ? a.table[c] : a.in[c]) + at.e; };
  int c = static_cast<int>(a.C) - 1;
  v2u64 acc = ld2(in(c));
  if (c == 0 && a.lead == 0) {
    st2(a.out + at.e, acc.x, acc.y);
    return;
  }
  const v2u64 w = ld2(a.w + at.we);
  auto step = [&](v2u64 x) {
    acc.x = add_mod(mul_mod(acc.x, w.x, q, r0, r1), x.x, q);
    acc.y = add_mod(mul_mod(acc.y, w.y, q, r0, r1), x.y, q);
  };
  for (--c; c >= 3; c -= 4) {  // four channel loads in flight
    const v2u64 x0 = ld2(in(c)), x1 = ld2(in(c - 1)), x2 = ld2(in(c - 2)), x3 = ld2(in(c - 3));
    step(x0);
    step(x1);
    step(x2);
    step(x3);
  }
  for (; c >= 0; --c) step(ld2(in(c)));
  for (uint32_t k = 0; k < a.lead; ++k) {  // channel 0 at index `lead`
    acc.x = mul_mod(acc.x, w.x, q, r0, r1);
    acc.y = mul_mod(acc.y, w.y, q, r0, r1);
  }
  st2(a.out + at.e, acc.x, acc.y);
}

// blockIdx.y: node
__global__ __launch_bounds__(kBlock) void ct_split_kernel(SplitArgs a, uint32_t log_n) {
  const size_t i = blockIdx.x * (size_t)kBlock + threadIdx.x;
  if (i >= (static_cast<size_t>(a.L) << log_n)) return;
  const Where at = where(i, a.L, log_n);
  const SplitNode nd = a.table ? a.table[blockIdx.y] : a.node[blockIdx.y];
  const uint64_t q = a.q[at.l];
  const v2u64 x = ld2(nd.a + at.e), r = ld2(nd.r + at.e);
  if (nd.even) st2(nd.even + at.e, add_mod(x.x, r.x, q), add_mod(x.y, r.y, q));
  if (nd.odd) {
    const uint64_t r0 = a.barrett[2 * at.l], r1 = a.barrett[2 * at.l + 1];
    const v2u64 m = ld2(a.m + at.we);
    st2(nd.odd + at.e, mul_mod(sub_mod(x.x, r.x, q), m.x, q, r0, r1), mul_mod(sub_mod(x.y, r.y, q), m.y, q, r0, r1));
  }
}

bool bad_shape(uint32_t L, size_t n) { return L < 1 || L > 65535 || n < 2 || (n & (n - 1)) || n > (size_t(1) << 20); }

}  // namespace

hipError_t ct_pack(const PackArgs& a, size_t n, hipStream_t s) {
  if (a.C < 1 || a.C + a.lead > kPackMax || (a.C > kPackInline && !a.table) || !a.w || !a.out || !a.q || !a.barrett ||
      bad_shape(a.L, n))
    return hipErrorInvalidValue;
  if (!a.table)
    for (uint32_t c = 0; c < a.C; ++c)
      if (!a.in[c]) return hipErrorInvalidValue;
  const size_t pairs = a.L * n;
  ct_pack_kernel<<<static_cast<unsigned>((pairs + kBlock - 1) / kBlock), kBlock, 0, s>>>(a, __builtin_ctzll(n));
  return hipGetLastError();
}

hipError_t ct_split(const SplitArgs& a, size_t n, hipStream_t s) {
  if (a.count < 1 || a.count > kSplitMax || (a.count > kSplitInline && !a.table) || !a.m || !a.q || !a.barrett ||
      bad_shape(a.L, n))
    return hipErrorInvalidValue;
  if (!a.table)
    for (uint32_t k = 0; k < a.count; ++k)
      if (!a.node[k].a || !a.node[k].r) return hipErrorInvalidValue;
  const size_t pairs = a.L * n;
  const dim3 grid(static_cast<unsigned>((pairs + kBlock - 1) / kBlock), a.count);
  ct_split_kernel<<<grid, kBlock, 0, s>>>(a, __builtin_ctzll(n));
  return hipGetLastError();
}

}  // namespace phx
