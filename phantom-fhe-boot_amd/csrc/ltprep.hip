// ltprep.hip — see ltprep.h.  Every kernel is a pure stream over the slot index: 16 bytes per lane,
// lanes on consecutive slots, no atomics (the presence flags are plain stores of the same value).
#include "ltprep.h"

namespace phx {

namespace {

constexpr int kBlock = 256;

// the host's std::complex product (contraction is off for device code)
__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
  return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

__device__ __forceinline__ bool nonzero(double2 v) { return v.x != 0.0 || v.y != 0.0; }

// 5^e mod 2^32 (the caller masks it down to the power of two it needs)
__device__ __forceinline__ uint32_t pow5(uint32_t e) {
  uint32_t r = 1, b = 5;
  while (e) {
    if (e & 1u) r *= b;
    b *= b;
    e >>= 1;
  }
  return r;
}

// boot::stage's two non-zeros of row p: d0 on the diagonal, d1 at +h (j < h) or -h (j >= h)
__global__ __launch_bounds__(kBlock) void stage_kernel(const double2* __restrict__ zeta, uint32_t zstep, uint32_t ns,
                                                       int s, int inverse, const double2* __restrict__ prev,
                                                       double2* __restrict__ out, const int32_t* __restrict__ src) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= ns) return;
  const uint32_t c = blockIdx.y;
  const uint32_t m = 1u << s, h = m >> 1;
  const uint32_t j = p & (m - 1);
  const bool lo = j < h;
  const uint32_t e = (ns >> s) * (pow5(lo ? j : j - h) & (4 * m - 1));  // (n / m) 5^j mod 4 n
  const double2 t = zeta[static_cast<size_t>(e) * zstep];
  double2 d0, d1;
  if (inverse) {
    d0 = lo ? make_double2(0.5, 0.0) : make_double2(-t.x * 0.5, t.y * 0.5);
    d1 = lo ? make_double2(0.5, 0.0) : make_double2(t.x * 0.5, -t.y * 0.5);
  } else {
    d0 = lo ? make_double2(1.0, 0.0) : make_double2(-t.x, -t.y);
    d1 = lo ? t : make_double2(1.0, 0.0);
  }
  const int32_t i0 = src[3 * c], i1 = src[3 * c + (lo ? 1 : 2)];
  const uint32_t q = lo ? ((p + h) & (ns - 1)) : ((p + ns - h) & (ns - 1));
  double2 acc = make_double2(0.0, 0.0);
  if (i0 >= 0) {
    const double2 b = prev ? prev[static_cast<size_t>(i0) * ns + p] : make_double2(1.0, 0.0);
    const double2 v = cmul(d0, b);
    acc.x += v.x;
    acc.y += v.y;
  }
  if (i1 >= 0) {
    const double2 b = prev ? prev[static_cast<size_t>(i1) * ns + q] : make_double2(1.0, 0.0);
    const double2 v = cmul(d1, b);
    acc.x += v.x;
    acc.y += v.y;
  }
  out[static_cast<size_t>(c) * ns + p] = acc;
}

__global__ __launch_bounds__(kBlock) void presence_kernel(const double2* __restrict__ band, uint32_t ns,
                                                          const int32_t* __restrict__ offsets, double2 cf,
                                                          int apply_const, int* __restrict__ flags) {
  const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
  if (r >= ns) return;
  const uint32_t i = blockIdx.y;
  double2 v = band[static_cast<size_t>(i) * ns + r];
  if (apply_const) v = cmul(v, cf);
  if (nonzero(v)) flags[2 * i + (r + static_cast<uint32_t>(offsets[i]) < ns ? 0 : 1)] = 1;
}

__global__ __launch_bounds__(kBlock) void finish_kernel(const double2* __restrict__ band, uint32_t ns, uint32_t n,
                                                        const LtFinishRow* __restrict__ rows, double2 cf,
                                                        int apply_const, int mask, double2* __restrict__ out) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= n) return;
  const LtFinishRow row = rows[blockIdx.y];
  const uint32_t pp = (p + n - static_cast<uint32_t>(row.sh)) & (n - 1);
  const uint32_t r = pp & (ns - 1);
  double2 v = band[static_cast<size_t>(row.src) * ns + r];
  if (apply_const) v = cmul(v, cf);
  if (ns < n) {
    const bool low = r + static_cast<uint32_t>(row.a) < ns;
    const bool want_low = static_cast<uint32_t>(row.key) < ns;
    if (low != want_low || !nonzero(v)) {
      v = make_double2(0.0, 0.0);
    } else {
      // lift_blocks' masks of period 2 ns: the output slot p', the input slot p' + key
      const uint32_t po = pp & (2 * ns - 1), qi = (pp + static_cast<uint32_t>(row.key)) & (2 * ns - 1);
      if (mask == kLtMaskOut) v = cmul(v, po >= ns ? make_double2(0.0, -1.0) : make_double2(1.0, 0.0));
      if (mask == kLtMaskIn) v = cmul(v, qi >= ns ? make_double2(0.0, 1.0) : make_double2(1.0, 0.0));
    }
  }
  out[static_cast<size_t>(blockIdx.y) * n + p] = v;
}

// 32 rows x 32 diagonals per block: reads run along a row of A (k fastest), writes along a
// diagonal (p fastest), transposed through LDS (one padding column against bank conflicts)
constexpr int kTile = 32;
__global__ __launch_bounds__(kTile* kTile) void dense_kernel(const double2* __restrict__ A, uint32_t slots, double scale,
                                                             double2* __restrict__ out, int* __restrict__ flags) {
  __shared__ double2 tile[kTile][kTile + 1];
  const uint32_t tx = threadIdx.x, ty = threadIdx.y;
  const uint32_t p0 = blockIdx.x * kTile, k0 = blockIdx.y * kTile;
  {
    const uint32_t p = p0 + ty, k = k0 + tx;
    double2 v = make_double2(0.0, 0.0);
    if (p < slots && k < slots) {
      const double2 a = A[static_cast<size_t>(p) * slots + ((p + k) & (slots - 1))];
      v = make_double2(a.x * scale, a.y * scale);
    }
    tile[ty][tx] = v;
  }
  __syncthreads();
  const uint32_t p = p0 + tx, k = k0 + ty;
  if (p < slots && k < slots) {
    const double2 v = tile[tx][ty];
    out[static_cast<size_t>(k) * slots + p] = v;
    if (nonzero(v)) flags[k] = 1;
  }
}

inline bool pow2(size_t x) { return x && !(x & (x - 1)); }
constexpr size_t kMaxSlots = size_t(1) << 24;  // 4 ns and every index stay far inside 32 bits
constexpr int kMaxRows = 65535;  // grid.y

}  // namespace

hipError_t ltprep_stage(const double2* zeta, size_t ring_n, size_t ns, int s, bool inverse, const double2* prev,
                        double2* out, const int32_t* src, int D_out, hipStream_t stream) {
  if (!zeta || !out || !src || D_out < 1 || D_out > kMaxRows) return hipErrorInvalidValue;
  if (!pow2(ring_n) || !pow2(ns) || ns < 2 || ns > ring_n / 2 || ring_n > kMaxSlots) return hipErrorInvalidValue;
  if (s < 1 || (size_t(1) << s) > ns) return hipErrorInvalidValue;
  const dim3 grid(static_cast<unsigned>((ns + kBlock - 1) / kBlock), static_cast<unsigned>(D_out));
  hipLaunchKernelGGL(stage_kernel, grid, dim3(kBlock), 0, stream, zeta, static_cast<uint32_t>(ring_n / (2 * ns)),
                     static_cast<uint32_t>(ns), s, inverse ? 1 : 0, prev, out, src);
  return hipGetLastError();
}

hipError_t ltprep_presence(const double2* band, size_t ns, const int32_t* offsets, int D, double2 cf, bool apply_const,
                           int* flags, hipStream_t stream) {
  if (!band || !offsets || !flags || D < 1 || D > kMaxRows) return hipErrorInvalidValue;
  if (!pow2(ns) || ns > kMaxSlots) return hipErrorInvalidValue;
  const dim3 grid(static_cast<unsigned>((ns + kBlock - 1) / kBlock), static_cast<unsigned>(D));
  hipLaunchKernelGGL(presence_kernel, grid, dim3(kBlock), 0, stream, band, static_cast<uint32_t>(ns), offsets, cf,
                     apply_const ? 1 : 0, flags);
  return hipGetLastError();
}

hipError_t ltprep_finish(const double2* band, size_t ns, size_t n, const LtFinishRow* rows, int K, double2 cf,
                         bool apply_const, int mask, double2* out, hipStream_t stream) {
  if (!band || !rows || !out || K < 1 || K > kMaxRows) return hipErrorInvalidValue;
  if (!pow2(ns) || !pow2(n) || ns > n || n > kMaxSlots) return hipErrorInvalidValue;
  if (mask != kLtMaskNone && mask != kLtMaskOut && mask != kLtMaskIn) return hipErrorInvalidValue;
  const dim3 grid(static_cast<unsigned>((n + kBlock - 1) / kBlock), static_cast<unsigned>(K));
  hipLaunchKernelGGL(finish_kernel, grid, dim3(kBlock), 0, stream, band, static_cast<uint32_t>(ns),
                     static_cast<uint32_t>(n), rows, cf, apply_const ? 1 : 0, mask, out);
  return hipGetLastError();
}

hipError_t ltprep_dense(const double2* A, size_t slots, double scale, double2* out, int* flags, hipStream_t stream) {
  if (!A || !out || !flags || !pow2(slots) || slots > (size_t(1) << 15)) return hipErrorInvalidValue;
  const unsigned t = static_cast<unsigned>((slots + kTile - 1) / kTile);
  hipLaunchKernelGGL(dense_kernel, dim3(t, t), dim3(kTile, kTile), 0, stream, A, static_cast<uint32_t>(slots), scale,
                     out, flags);
  return hipGetLastError();
}

}  // namespace phx
