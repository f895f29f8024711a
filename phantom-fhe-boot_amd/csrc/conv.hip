// conv.hip — kernels of the hoisted encrypted convolution (see conv.h).
#include "conv.h"

#include <algorithm>

#include "arith.h"

namespace phx {
namespace {

constexpr int kBlock = 256;
constexpr uint64_t kM30 = (1ull << 30) - 1;

// The kernels take the operand lists and moduli (MacCore) and, in their seeded instantiations only,
// the seed as a trailing argument (`Seed...` is empty or one MacSeed): without a seed the kernel has
// the signature, the arguments and the code it had before seeds existed.
struct MacSeed {
  const uint64_t* const* res;
  const uint64_t* mult;
  const uint64_t* bias;
};
__device__ __forceinline__ const MacSeed& mac_the_seed(const MacSeed& sd) { return sd; }

// operand k of a list given as a device pointer table or as base + k stride
__device__ __forceinline__ const uint64_t* mac_in(const MacCore& a, uint32_t t) {
  return a.ins ? a.ins[t] : a.in0 + static_cast<size_t>(t) * a.in_stride;
}
__device__ __forceinline__ const uint64_t* mac_pt(const MacCore& a, size_t k) {
  return a.pts ? a.pts[k] : a.pt0 + k * a.pt_stride;
}
__device__ __forceinline__ uint64_t* mac_out(const MacCore& a, uint32_t o) {
  return a.outs ? a.outs[o] : a.out0 + static_cast<size_t>(o) * a.out_stride;
}

// 16-byte global (not flat) accesses of two consecutive elements: they count in vmcnt only
typedef uint64_t mac_u64x2 __attribute__((ext_vector_type(2)));
struct MacVec {
  uint64_t v[kMacEpl];
};
__device__ __forceinline__ MacVec mac_ld(const uint64_t* p) {
  const mac_u64x2 x = *(const __attribute__((address_space(1))) mac_u64x2*)p;
  MacVec r;
  r.v[0] = x.x;
  r.v[1] = x.y;
  return r;
}

// the four 64-bit partial sums of x * w per element and polynomial, x and w split in 30-bit halves
struct MacPart {
  uint64_t ll, m1, m2, hh;
};

__device__ __forceinline__ void mac_fold(u128& acc, MacPart& P) {
  add128(acc, u128{P.ll, 0});
  add128(acc, u128{P.m1 << 30, P.m1 >> 34});
  add128(acc, u128{P.m2 << 30, P.m2 >> 34});
  add128(acc, u128{P.hh << 60, P.hh >> 4});
  P = MacPart{0, 0, 0, 0};
}

constexpr int kMacChunk = 4, kMacChunks = kMacBlock / kMacChunk;

// the seed of one word (conv.h): x seed_mult[l] (x the residual's word, when output o has one) plus
// the bias residue (polynomial 0 only), below q
__device__ __forceinline__ uint64_t mac_seed(bool has_res, uint64_t x, uint64_t mult, uint64_t bias, uint64_t q,
                                             uint64_t r0, uint64_t r1) {
  const uint64_t v = has_res ? mul_mod(x, mult, q, r0, r1) : 0;
  return add_mod(v, bias, q);
}

// chunk c (terms 4c .. 4c + 3 of the block at t0) of output o's plaintexts; terms past the last
// read the last one again (their inputs are staged as zeros)
__device__ __forceinline__ void mac_load_chunk(MacVec (&w)[kMacChunk], const MacCore& a, size_t prow, uint32_t t0, int c,
                                               size_t e) {
#pragma unroll
  for (int j = 0; j < kMacChunk; ++j) {
    const uint32_t t = min(t0 + static_cast<uint32_t>(c * kMacChunk + j), a.T - 1);
    w[j] = mac_ld(mac_pt(a, prow + t) + e);
  }
}

// part += sum_j in(4c + j) * w[j], the inputs from LDS (row 2j + p: term j of the block,
// polynomial p, as {low 30, high 30} bits)
__device__ __forceinline__ void mac_chunk_products(MacPart (&part)[kMacEpl][2], const MacVec (&w)[kMacChunk],
                                                   const uint2 (*xs)[kMacTile], int c, int lane) {
#pragma unroll
  for (int jj = 0; jj < kMacChunk; ++jj) {
    const int j = c * kMacChunk + jj;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const uint4 xx = *reinterpret_cast<const uint4*>(&xs[2 * j + p][2 * lane]);
      const uint2 x[kMacEpl] = {make_uint2(xx.x, xx.y), make_uint2(xx.z, xx.w)};
#pragma unroll
      for (int k = 0; k < kMacEpl; ++k) {
        const uint32_t wl = static_cast<uint32_t>(w[jj].v[k] & kM30), wh = static_cast<uint32_t>(w[jj].v[k] >> 30);
        MacPart& P = part[k][p];
        P.ll += static_cast<uint64_t>(x[k].x) * wl;
        P.m1 += static_cast<uint64_t>(x[k].x) * wh;
        P.m2 += static_cast<uint64_t>(x[k].y) * wl;
        P.hh += static_cast<uint64_t>(x[k].y) * wh;
      }
    }
  }
}

// One workgroup = kMacWaves waves over one tile of kMacTile elements; grid row y serves outputs
// 8 y .. 8 y + 7, wave w output 8 y + w.  Per block of kMacBlock terms: every wave loads 8 of the 64
// input rows (32 terms x 2 polynomials; rows past the last term are zeros) and writes them to LDS
// as 30-bit halves; then each wave with an output streams that output's 32 plaintexts 4 at a time,
// chunk c + 1's loads in flight while chunk c's products run.  The 128-bit sums stay in registers
// and are reduced below q after every block (conv.h).
template <bool Q60, class... Seed>
__global__ __launch_bounds__(64 * kMacWaves) void ext_mac_tile_kernel(MacCore a, uint32_t log_n, size_t total,
                                                                      Seed... seed) {
  constexpr bool Seeded = sizeof...(Seed) != 0;
  constexpr int E = kMacEpl;
  __shared__ uint2 xs[2 * kMacBlock][kMacTile];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const size_t tile = blockIdx.x;
  const size_t e = tile * kMacTile + static_cast<size_t>(lane) * E;
  const uint32_t o = blockIdx.y * kMacWaves + wv;
  const bool active = o < a.O;  // wave-uniform
  const int l = static_cast<int>((tile * kMacTile) >> log_n);
  const int row = l < static_cast<int>(a.Ql) ? l : static_cast<int>(a.size_Q) + (l - static_cast<int>(a.Ql));
  const uint64_t q = a.q[row], r0 = a.barrett[2 * row], r1 = a.barrett[2 * row + 1];
  const size_t prow = static_cast<size_t>(active ? o : 0) * a.T;
  uint64_t* const op = active ? mac_out(a, o) : nullptr;

  u128 acc[E][2];
  MacPart part[E][2];
#pragma unroll
  for (int k = 0; k < E; ++k)
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      acc[k][p] = u128{0, 0};
      part[k][p] = MacPart{0, 0, 0, 0};
    }
  if constexpr (Seeded) {
    // the seed takes accumulate's place: limbs of Ql only, below q (conv.h)
    if (active && l < static_cast<int>(a.Ql)) {
      const MacSeed& sd = mac_the_seed(seed...);
      const uint64_t* const res = sd.res ? sd.res[o] : nullptr;  // wave-uniform
      const uint64_t mult = res ? sd.mult[l] : 0;
      const uint64_t bias = sd.bias ? sd.bias[static_cast<size_t>(o) * a.Ql + l] : 0;
      const size_t res_total = static_cast<size_t>(a.Ql) << log_n;
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        MacVec x{{0, 0}};
        if (res) x = mac_ld(res + p * res_total + e);
#pragma unroll
        for (int k = 0; k < E; ++k) acc[k][p].lo = mac_seed(res != nullptr, x.v[k], mult, p == 0 ? bias : 0, q, r0, r1);
      }
    }
  } else if (active && a.accumulate) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const MacVec old = mac_ld(op + p * total + e);
#pragma unroll
      for (int k = 0; k < E; ++k) acc[k][p].lo = old.v[k];
    }
  }

  for (uint32_t t0 = 0; t0 < a.T; t0 += kMacBlock) {
    const int nb = static_cast<int>(min(a.T - t0, static_cast<uint32_t>(kMacBlock)));
    // staging: wave wv loads rows wv + 8 r, r < 8 (row 2 j + p: term t0 + j, polynomial p)
    MacVec v[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int R = wv + 8 * r, j = R >> 1;
      if (j < nb) v[r] = mac_ld(mac_in(a, t0 + j) + static_cast<size_t>(R & 1) * total + e);
      else v[r] = MacVec{{0, 0}};
    }
    MacVec wbuf[2][kMacChunk];
    if (active) mac_load_chunk(wbuf[0], a, prow, t0, 0, e);
    if (t0) __syncthreads();  // the previous block's LDS reads are done
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
      for (int k = 0; k < E; ++k)
        xs[wv + 8 * r][lane * E + k] =
            make_uint2(static_cast<uint32_t>(v[r].v[k] & kM30), static_cast<uint32_t>(v[r].v[k] >> 30));
    __syncthreads();
    if (active) {
#pragma unroll
      for (int c = 0; c < kMacChunks; ++c) {
        if (c * kMacChunk >= nb) break;  // the rest of a tail block is zeros
        if (c + 1 < kMacChunks) mac_load_chunk(wbuf[(c + 1) & 1], a, prow, t0, c + 1, e);
        // keep the next chunk's loads together and ahead of this chunk's products
        __builtin_amdgcn_sched_barrier(0);
        mac_chunk_products(part, wbuf[c & 1], xs, c, lane);
        // 8 products per partial sum (q < 2^60: each below 2^60, the sum below 2^63), otherwise 4
        // (a high-half product reaches 2^62)
        if ((c & 1) || !Q60) {
#pragma unroll
          for (int k = 0; k < E; ++k)
#pragma unroll
            for (int p = 0; p < 2; ++p) mac_fold(acc[k][p], part[k][p]);
        }
      }
      // a tail block may stop between folds; then the block's sum (at most 32 products and the
      // carried residue, below 2^128) is reduced and carried on
#pragma unroll
      for (int k = 0; k < E; ++k)
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          mac_fold(acc[k][p], part[k][p]);
          acc[k][p] = u128{barrett_reduce_128(acc[k][p], q, r0, r1), 0};
        }
    }
  }
  if (active) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      mac_u64x2 r;
      r.x = acc[0][p].lo;
      r.y = acc[1][p].lo;
      *(__attribute__((address_space(1))) mac_u64x2*)(op + p * total + e) = r;
    }
  }
}

// One element per thread and grid-stride step, grid row y = output y: any n and any tile
// alignment.  Terms 4 at a time (4 products per partial sum fit for every modulus below 2^61),
// the 128-bit sum reduced below q every kMacBlock terms.
template <class... Seed>
__global__ __launch_bounds__(kBlock) void ext_mac_plain_kernel(MacCore a, uint32_t log_n, size_t total, Seed... seed) {
  constexpr bool Seeded = sizeof...(Seed) != 0;
  const uint32_t o = blockIdx.y;
  uint64_t* const op = mac_out(a, o);
  const size_t prow = static_cast<size_t>(o) * a.T;
  for (size_t e = blockIdx.x * (size_t)kBlock + threadIdx.x; e < total; e += (size_t)gridDim.x * kBlock) {
    const int l = static_cast<int>(e >> log_n);
    const int row = l < static_cast<int>(a.Ql) ? l : static_cast<int>(a.size_Q) + (l - static_cast<int>(a.Ql));
    const uint64_t q = a.q[row], r0 = a.barrett[2 * row], r1 = a.barrett[2 * row + 1];
    u128 acc[2] = {{0, 0}, {0, 0}};
    if constexpr (Seeded) {
      if (l < static_cast<int>(a.Ql)) {
        const MacSeed& sd = mac_the_seed(seed...);
        const uint64_t* const res = sd.res ? sd.res[o] : nullptr;
        const uint64_t mult = res ? sd.mult[l] : 0;
        const uint64_t bias = sd.bias ? sd.bias[static_cast<size_t>(o) * a.Ql + l] : 0;
        const size_t res_total = static_cast<size_t>(a.Ql) << log_n;
        acc[0].lo = mac_seed(res != nullptr, res ? res[e] : 0, mult, bias, q, r0, r1);
        acc[1].lo = mac_seed(res != nullptr, res ? res[res_total + e] : 0, mult, 0, q, r0, r1);
      }
    } else if (a.accumulate) {
      acc[0].lo = op[e];
      acc[1].lo = op[total + e];
    }
    for (uint32_t t0 = 0; t0 < a.T; t0 += kMacChunk) {
      const uint32_t cnt = min(a.T - t0, static_cast<uint32_t>(kMacChunk));
      MacPart part[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
      for (uint32_t j = 0; j < cnt; ++j) {
        const uint64_t* in = mac_in(a, t0 + j);
        const uint64_t w = mac_pt(a, prow + t0 + j)[e];
        const uint32_t wl = static_cast<uint32_t>(w & kM30), wh = static_cast<uint32_t>(w >> 30);
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          const uint64_t x = in[p * total + e];
          const uint32_t xl = static_cast<uint32_t>(x & kM30), xh = static_cast<uint32_t>(x >> 30);
          part[p].ll += static_cast<uint64_t>(xl) * wl;
          part[p].m1 += static_cast<uint64_t>(xl) * wh;
          part[p].m2 += static_cast<uint64_t>(xh) * wl;
          part[p].hh += static_cast<uint64_t>(xh) * wh;
        }
      }
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        mac_fold(acc[p], part[p]);
        if ((t0 + kMacChunk) % kMacBlock == 0) acc[p] = u128{barrett_reduce_128(acc[p], q, r0, r1), 0};
      }
    }
    op[e] = barrett_reduce_128(acc[0], q, r0, r1);
    op[total + e] = barrett_reduce_128(acc[1], q, r0, r1);
  }
}

// ---- inner sums over compact plaintexts (conv.h) ---------------------------------------------
// chunk c of output o's plaintext words, one per lane (shared by the lane's two elements); byte
// offset `pofs` from each plaintext's base, 32 bits so that the load takes the scalar base and a
// vector offset
__device__ __forceinline__ void sub_load_chunk(uint64_t (&w)[kMacChunk], const MacCore& a, size_t prow, uint32_t t0,
                                               int c, uint32_t pofs) {
#pragma unroll
  for (int j = 0; j < kMacChunk; ++j) {
    const uint32_t t = min(t0 + static_cast<uint32_t>(c * kMacChunk + j), a.T - 1);
    w[j] = *(const __attribute__((address_space(1))) uint64_t*)(reinterpret_cast<const char*>(mac_pt(a, prow + t)) + pofs);
  }
}

// as mac_chunk_products with one word per lane; Uniform: the word is the same in every lane and
// its halves go to scalar registers once per term
template <bool Uniform>
__device__ __forceinline__ void sub_chunk_products(MacPart (&part)[kMacEpl][2], const uint64_t (&w)[kMacChunk],
                                                   const uint2 (*xs)[kMacTile], int c, int lane) {
#pragma unroll
  for (int jj = 0; jj < kMacChunk; ++jj) {
    const int j = c * kMacChunk + jj;
    uint32_t wl = static_cast<uint32_t>(w[jj] & kM30), wh = static_cast<uint32_t>(w[jj] >> 30);
    if constexpr (Uniform) {
      wl = __builtin_amdgcn_readfirstlane(wl);
      wh = __builtin_amdgcn_readfirstlane(wh);
    }
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const uint4 xx = *reinterpret_cast<const uint4*>(&xs[2 * j + p][2 * lane]);
      const uint2 x[kMacEpl] = {make_uint2(xx.x, xx.y), make_uint2(xx.z, xx.w)};
#pragma unroll
      for (int k = 0; k < kMacEpl; ++k) {
        MacPart& P = part[k][p];
        P.ll += static_cast<uint64_t>(x[k].x) * wl;
        P.m1 += static_cast<uint64_t>(x[k].x) * wh;
        P.m2 += static_cast<uint64_t>(x[k].y) * wl;
        P.hh += static_cast<uint64_t>(x[k].y) * wh;
      }
    }
  }
}

// One workgroup = kSubWaves = 16 waves over one tile of kMacTile elements, wave w forming output
// 16 row + w: a staged block of 32 inputs x 2 polynomials serves 16 outputs, so a layer of up to 16
// output channels reads every input once.  Wave w stages rows w + 16 r, r < 4; the rows of the next
// block are loaded one per two chunks while this block's products run (behind the next chunk's
// plaintext words, so the wait for those words leaves the row in flight), and written to LDS after
// the barrier that ends the block.  Plaintext words (gap >= 2; gap 1 is ext_mac): one per lane,
// shared by its two elements, or with Uniform (gap >= 128) one per tile, its halves in scalar
// registers.  Every address is a wave-uniform base and a 32-bit lane offset, which leaves the
// address registers to the sums.  Workgroups are numbered so
// that the rows of one tile follow each other on one XCD (blocks b and b + 8 share one): with more
// than 16 outputs the re-read of a tile's inputs can hit that XCD's L2.  Placement is for speed
// only; nothing depends on it.
constexpr int kSubRows = 2 * kMacBlock / kSubWaves;
// 16 bytes at base + ofs (a scalar base and a vector offset)
__device__ __forceinline__ MacVec sub_ld2(const uint64_t* base, uint32_t ofs) {
  return mac_ld(reinterpret_cast<const uint64_t*>(reinterpret_cast<const char*>(base) + ofs));
}
template <bool Q60, bool Uniform, class... Seed>
__global__ __launch_bounds__(64 * kSubWaves) void ext_mac_sub_tile_kernel(MacCore a, uint32_t log_n, uint32_t log_g,
                                                                          uint32_t rows, size_t total,
                                                                          Seed... seed) {
  constexpr bool Seeded = sizeof...(Seed) != 0;
  constexpr int E = kMacEpl;
  __shared__ uint2 xs[2 * kMacBlock][kMacTile];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t b = blockIdx.x, bi = b >> 3;
  const size_t tile = static_cast<size_t>(bi / rows) * 8 + (b & 7);
  const size_t e0 = tile * kMacTile;  // the tile's first element (wave-uniform)
  const uint32_t lofs = static_cast<uint32_t>(lane) * (E * sizeof(uint64_t));  // the lane's bytes into the tile
  const uint32_t o = (bi % rows) * kSubWaves + wv;
  const bool active = o < a.O;  // wave-uniform
  const int l = static_cast<int>((tile * kMacTile) >> log_n);
  const int row = l < static_cast<int>(a.Ql) ? l : static_cast<int>(a.size_Q) + (l - static_cast<int>(a.Ql));
  const uint64_t q = a.q[row], r0 = a.barrett[2 * row], r1 = a.barrett[2 * row + 1];
  const size_t prow = static_cast<size_t>(active ? o : 0) * a.T;
  uint64_t* const op = active ? mac_out(a, o) : nullptr;
  // the lane's plaintext word in limb l of [Ql + P][n >> log_g], as a byte offset (a plaintext has
  // at most 64 limbs of 2^17 words)
  const uint32_t ein = static_cast<uint32_t>(e0 & ((size_t(1) << log_n) - 1)) + static_cast<uint32_t>(lane) * E;
  const uint32_t pofs = ((static_cast<uint32_t>(l) << (log_n - log_g)) + (ein >> log_g)) * sizeof(uint64_t);

  u128 acc[E][2];
  MacPart part[E][2];
#pragma unroll
  for (int k = 0; k < E; ++k)
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      acc[k][p] = u128{0, 0};
      part[k][p] = MacPart{0, 0, 0, 0};
    }
  if constexpr (Seeded) {
    // the seed takes accumulate's place: limbs of Ql only, below q (conv.h).  It is formed before the
    // first rows are requested, so it adds nothing to the registers live in the loop.
    if (active && l < static_cast<int>(a.Ql)) {
      const MacSeed& sd = mac_the_seed(seed...);
      const uint64_t* const res = sd.res ? sd.res[o] : nullptr;  // wave-uniform
      const uint64_t mult = res ? sd.mult[l] : 0;
      const uint64_t bias = sd.bias ? sd.bias[static_cast<size_t>(o) * a.Ql + l] : 0;
      const size_t res_total = static_cast<size_t>(a.Ql) << log_n;
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        MacVec x{{0, 0}};
        if (res) x = sub_ld2(res + p * res_total + e0, lofs);
#pragma unroll
        for (int k = 0; k < E; ++k) acc[k][p].lo = mac_seed(res != nullptr, x.v[k], mult, p == 0 ? bias : 0, q, r0, r1);
      }
    }
  } else if (active && a.accumulate) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const MacVec old = sub_ld2(op + p * total + e0, lofs);
#pragma unroll
      for (int k = 0; k < E; ++k) acc[k][p].lo = old.v[k];
    }
  }

  // row R = wv + 16 r of the block at t0: term t0 + R / 2, polynomial R % 2; zeros past the last term
  auto load_row = [&](uint32_t t0, int r) -> MacVec {
    const int R = wv + kSubWaves * r;
    const uint32_t t = t0 + static_cast<uint32_t>(R >> 1);
    if (t < a.T) return sub_ld2(mac_in(a, t) + static_cast<size_t>(R & 1) * total + e0, lofs);
    return MacVec{{0, 0}};
  };
  MacVec v[kSubRows];
#pragma unroll
  for (int r = 0; r < kSubRows; ++r) v[r] = load_row(0, r);

  for (uint32_t t0 = 0; t0 < a.T; t0 += kMacBlock) {
    const int nb = static_cast<int>(min(a.T - t0, static_cast<uint32_t>(kMacBlock)));
    const bool more = t0 + kMacBlock < a.T;  // then nb = kMacBlock and every chunk below runs
    uint64_t wbuf[2][kMacChunk];
    if (active) sub_load_chunk(wbuf[0], a, prow, t0, 0, pofs);
    if (t0) __syncthreads();  // the previous block's LDS reads are done
#pragma unroll
    for (int r = 0; r < kSubRows; ++r)
#pragma unroll
      for (int k = 0; k < E; ++k)
        xs[wv + kSubWaves * r][lane * E + k] =
            make_uint2(static_cast<uint32_t>(v[r].v[k] & kM30), static_cast<uint32_t>(v[r].v[k] >> 30));
    __syncthreads();
#pragma unroll
    for (int c = 0; c < kMacChunks; ++c) {
      if (c * kMacChunk >= nb) break;  // the rest of a tail block is zeros
      if (active && c + 1 < kMacChunks) sub_load_chunk(wbuf[(c + 1) & 1], a, prow, t0, c + 1, pofs);
      if (more && (c & 1) == 0) v[c >> 1] = load_row(t0 + kMacBlock, c >> 1);
      // keep the loads together and ahead of this chunk's products
      __builtin_amdgcn_sched_barrier(0);
      if (active) {
        sub_chunk_products<Uniform>(part, wbuf[c & 1], xs, c, lane);
        // 8 products per partial sum when q < 2^60, otherwise 4 (ext_mac_tile_kernel)
        if ((c & 1) || !Q60) {
#pragma unroll
          for (int k = 0; k < E; ++k)
#pragma unroll
            for (int p = 0; p < 2; ++p) mac_fold(acc[k][p], part[k][p]);
        }
      }
    }
    if (active) {
      // a tail block may stop between folds; the block's sum (at most 32 products and the carried
      // residue, below 2^128) is reduced and carried on
#pragma unroll
      for (int k = 0; k < E; ++k)
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          mac_fold(acc[k][p], part[k][p]);
          acc[k][p] = u128{barrett_reduce_128(acc[k][p], q, r0, r1), 0};
        }
    }
  }
  if (active) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      mac_u64x2 r;
      r.x = acc[0][p].lo;
      r.y = acc[1][p].lo;
      *(__attribute__((address_space(1))) mac_u64x2*)(reinterpret_cast<char*>(op + p * total + e0) + lofs) = r;
    }
  }
}

// ext_mac_plain_kernel with the plaintext word of element e of limb l at l (n >> log_g) + (e >> log_g)
template <class... Seed>
__global__ __launch_bounds__(kBlock) void ext_mac_sub_plain_kernel(MacCore a, uint32_t log_n, uint32_t log_g,
                                                                   size_t total, Seed... seed) {
  constexpr bool Seeded = sizeof...(Seed) != 0;
  const uint32_t o = blockIdx.y;
  uint64_t* const op = mac_out(a, o);
  const size_t prow = static_cast<size_t>(o) * a.T;
  const size_t n1 = (size_t(1) << log_n) - 1;
  for (size_t e = blockIdx.x * (size_t)kBlock + threadIdx.x; e < total; e += (size_t)gridDim.x * kBlock) {
    const int l = static_cast<int>(e >> log_n);
    const int row = l < static_cast<int>(a.Ql) ? l : static_cast<int>(a.size_Q) + (l - static_cast<int>(a.Ql));
    const uint64_t q = a.q[row], r0 = a.barrett[2 * row], r1 = a.barrett[2 * row + 1];
    const size_t poff = (static_cast<size_t>(l) << (log_n - log_g)) + ((e & n1) >> log_g);
    u128 acc[2] = {{0, 0}, {0, 0}};
    if constexpr (Seeded) {
      if (l < static_cast<int>(a.Ql)) {
        const MacSeed& sd = mac_the_seed(seed...);
        const uint64_t* const res = sd.res ? sd.res[o] : nullptr;
        const uint64_t mult = res ? sd.mult[l] : 0;
        const uint64_t bias = sd.bias ? sd.bias[static_cast<size_t>(o) * a.Ql + l] : 0;
        const size_t res_total = static_cast<size_t>(a.Ql) << log_n;
        acc[0].lo = mac_seed(res != nullptr, res ? res[e] : 0, mult, bias, q, r0, r1);
        acc[1].lo = mac_seed(res != nullptr, res ? res[res_total + e] : 0, mult, 0, q, r0, r1);
      }
    } else if (a.accumulate) {
      acc[0].lo = op[e];
      acc[1].lo = op[total + e];
    }
    for (uint32_t t0 = 0; t0 < a.T; t0 += kMacChunk) {
      const uint32_t cnt = min(a.T - t0, static_cast<uint32_t>(kMacChunk));
      MacPart part[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
      for (uint32_t j = 0; j < cnt; ++j) {
        const uint64_t* in = mac_in(a, t0 + j);
        const uint64_t w = mac_pt(a, prow + t0 + j)[poff];
        const uint32_t wl = static_cast<uint32_t>(w & kM30), wh = static_cast<uint32_t>(w >> 30);
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          const uint64_t x = in[p * total + e];
          const uint32_t xl = static_cast<uint32_t>(x & kM30), xh = static_cast<uint32_t>(x >> 30);
          part[p].ll += static_cast<uint64_t>(xl) * wl;
          part[p].m1 += static_cast<uint64_t>(xl) * wh;
          part[p].m2 += static_cast<uint64_t>(xh) * wl;
          part[p].hh += static_cast<uint64_t>(xh) * wh;
        }
      }
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        mac_fold(acc[p], part[p]);
        if ((t0 + kMacChunk) % kMacBlock == 0) acc[p] = u128{barrett_reduce_128(acc[p], q, r0, r1), 0};
      }
    }
    op[e] = barrett_reduce_128(acc[0], q, r0, r1);
    op[total + e] = barrett_reduce_128(acc[1], q, r0, r1);
  }
}

// thread i: slot i % ns of term first + i / ns
__global__ __launch_bounds__(kBlock) void conv_weight_slots_kernel(ConvShape c, const double* W, const double* out_scale,
                                                                   size_t first, size_t total, uint32_t log_ns,
                                                                   double2* out) {
  const uint32_t K = c.kernel, half = K / 2, lg = c.width << c.slotstr;
  const uint32_t log_lg = log_ns / 2;
  for (size_t i = blockIdx.x * (size_t)kBlock + threadIdx.x; i < total; i += (size_t)gridDim.x * kBlock) {
    const uint32_t s = static_cast<uint32_t>(i & ((size_t(1) << log_ns) - 1));
    size_t term = first + (i >> log_ns);
    const uint32_t b = term % K;
    term /= K;
    const uint32_t ta = term % K;
    term /= K;
    const uint32_t k = term % c.in_ch, h = static_cast<uint32_t>(term / c.in_ch);
    double v = 0.0;
    if ((s & ((1u << c.slotstr) - 1)) == 0) {
      const uint32_t m = s >> c.slotstr, r = m >> log_lg, col = m & (lg - 1);
      // r + a - K/2 and col + b - K/2 in [0, width)
      if (r < c.width && col < c.width && r + ta >= half && r + ta < half + c.width && col + b >= half &&
          col + b < half + c.width)
        v = W[((static_cast<size_t>(ta) * K + b) * c.in_ch + k) * c.out_ch + h] * (out_scale ? out_scale[h] : 1.0);
    }
    out[i] = make_double2(v, 0.0);
  }
}

__global__ __launch_bounds__(64) void write_words_kernel(uint64_t* dst, Words w, uint32_t count) {
  for (uint32_t i = threadIdx.x; i < count; i += 64) dst[i] = w.w[i];
}

unsigned grid_for(size_t total) { return static_cast<unsigned>(std::min<size_t>((total + kBlock - 1) / kBlock, 65535)); }

// a seed with accumulate, or a residual table without its multiplier, is refused
bool mac_seeded(const MacArgs& a) { return a.seed_res || a.seed_bias; }
bool mac_seed_ok(const MacArgs& a) { return !(mac_seeded(a) && a.accumulate) && !(a.seed_res && !a.seed_mult); }

}  // namespace

hipError_t ext_mac(const MacArgs& a, size_t n, hipStream_t s) {
  if (a.T == 0 || a.O == 0 || n == 0 || (n & (n - 1))) return hipErrorInvalidValue;
  if ((!a.ins && !a.in0) || (!a.pts && !a.pt0) || (!a.outs && !a.out0)) return hipErrorInvalidValue;
  if (!mac_seed_ok(a)) return hipErrorInvalidValue;
  const bool seeded = mac_seeded(a);
  const MacCore& core = a;
  const MacSeed sd{a.seed_res, a.seed_mult, a.seed_bias};
  const size_t total = static_cast<size_t>(a.Ql + a.P) * n;
  const uint32_t log_n = static_cast<uint32_t>(__builtin_ctzll(n));
  if (n >= kMacTileMinN && n % kMacTile == 0) {
    // a tile never crosses a limb (n is a multiple of it)
    const dim3 grid(static_cast<unsigned>(total / kMacTile), (a.O + kMacWaves - 1) / kMacWaves);
    if (grid.y > 65535) return hipErrorInvalidValue;
    const unsigned threads = 64 * kMacWaves;
    if (a.q60) {
      if (seeded) ext_mac_tile_kernel<true, MacSeed><<<grid, threads, 0, s>>>(core, log_n, total, sd);
      else ext_mac_tile_kernel<true><<<grid, threads, 0, s>>>(core, log_n, total);
    } else {
      if (seeded) ext_mac_tile_kernel<false, MacSeed><<<grid, threads, 0, s>>>(core, log_n, total, sd);
      else ext_mac_tile_kernel<false><<<grid, threads, 0, s>>>(core, log_n, total);
    }
  } else {
    if (a.O > 65535) return hipErrorInvalidValue;
    const dim3 grid(grid_for(total), a.O);
    if (seeded) ext_mac_plain_kernel<MacSeed><<<grid, kBlock, 0, s>>>(core, log_n, total, sd);
    else ext_mac_plain_kernel<><<<grid, kBlock, 0, s>>>(core, log_n, total);
  }
  return hipGetLastError();
}

hipError_t ext_mac_sub(const MacArgs& a, size_t n, size_t sub_degree, hipStream_t s) {
  if (a.T == 0 || a.O == 0 || n == 0 || (n & (n - 1))) return hipErrorInvalidValue;
  if (sub_degree == 0 || sub_degree > n || (sub_degree & (sub_degree - 1))) return hipErrorInvalidValue;
  if ((!a.ins && !a.in0) || (!a.pts && !a.pt0) || (!a.outs && !a.out0)) return hipErrorInvalidValue;
  if (!mac_seed_ok(a)) return hipErrorInvalidValue;
  const bool seeded = mac_seeded(a);
  const MacCore& core = a;
  const MacSeed sd{a.seed_res, a.seed_mult, a.seed_bias};
  const size_t total = static_cast<size_t>(a.Ql + a.P) * n;
  const uint32_t log_n = static_cast<uint32_t>(__builtin_ctzll(n));
  const uint32_t log_g = log_n - static_cast<uint32_t>(__builtin_ctzll(sub_degree));
  if (log_g == 0) return ext_mac(a, n, s);  // full-size plaintexts: two words per lane, ext_mac's form
  if (n >= kMacTileMinN && n % kMacTile == 0) {
    // a tile never crosses a limb, and a limb holds a multiple of 8 tiles (n >= 1024 = 8 tiles), which
    // the kernel's numbering of workgroups relies on
    static_assert(kMacTileMinN % (8 * kMacTile) == 0, "a limb must hold a multiple of 8 tiles");
    const size_t tiles = total / kMacTile, rows = (a.O + kSubWaves - 1) / kSubWaves;
    if (tiles * rows > 0x7fffffffu) return hipErrorInvalidValue;
    const dim3 grid(static_cast<unsigned>(tiles * rows));
    const uint32_t r = static_cast<uint32_t>(rows);
    const bool uniform = (size_t(1) << log_g) >= static_cast<size_t>(kMacTile);  // one word per tile
#define PHX_SUB_LAUNCH(Q, U)                                                                                 \
  do {                                                                                                       \
    if (seeded) ext_mac_sub_tile_kernel<Q, U, MacSeed><<<grid, 64 * kSubWaves, 0, s>>>(core, log_n, log_g, r, total, sd); \
    else ext_mac_sub_tile_kernel<Q, U><<<grid, 64 * kSubWaves, 0, s>>>(core, log_n, log_g, r, total);         \
  } while (0)
    if (a.q60) {
      if (uniform) PHX_SUB_LAUNCH(true, true);
      else PHX_SUB_LAUNCH(true, false);
    } else {
      if (uniform) PHX_SUB_LAUNCH(false, true);
      else PHX_SUB_LAUNCH(false, false);
    }
#undef PHX_SUB_LAUNCH
  } else {
    if (a.O > 65535) return hipErrorInvalidValue;
    const dim3 grid(grid_for(total), a.O);
    if (seeded) ext_mac_sub_plain_kernel<MacSeed><<<grid, kBlock, 0, s>>>(core, log_n, log_g, total, sd);
    else ext_mac_sub_plain_kernel<><<<grid, kBlock, 0, s>>>(core, log_n, log_g, total);
  }
  return hipGetLastError();
}

hipError_t conv_weight_slots(const ConvShape& c, const double* dev_W, size_t first_term, size_t count, double* dev_out,
                             hipStream_t s, const double* dev_out_scale) {
  if (count == 0) return hipSuccess;
  const size_t ns = c.slots(), total = count * ns;
  conv_weight_slots_kernel<<<grid_for(total), kBlock, 0, s>>>(c, dev_W, dev_out_scale, first_term, total,
                                                             static_cast<uint32_t>(__builtin_ctzll(ns)),
                                                             reinterpret_cast<double2*>(dev_out));
  return hipGetLastError();
}

void conv_weight_slots_host(const ConvShape& c, const double* W, size_t first_term, size_t count, double* out) {
  const size_t K = c.kernel, half = K / 2, lg = c.large(), ns = c.slots(), pw = size_t(1) << c.slotstr;
  std::fill(out, out + 2 * count * ns, 0.0);
  for (size_t i = 0; i < count; ++i) {
    size_t term = first_term + i;
    const size_t b = term % K;
    term /= K;
    const size_t a = term % K;
    term /= K;
    const size_t k = term % c.in_ch, h = term / c.in_ch;
    const double w = W[((a * K + b) * c.in_ch + k) * c.out_ch + h];
    for (size_t r = 0; r < c.width; ++r)
      for (size_t col = 0; col < c.width; ++col)
        if (r + a >= half && r + a < half + c.width && col + b >= half && col + b < half + c.width)
          out[2 * (i * ns + (r * lg + col) * pw)] = w;
  }
}

hipError_t write_words(uint64_t* dst, const Words& w, size_t count, hipStream_t s) {
  if (count > static_cast<size_t>(kWordsMax)) return hipErrorInvalidValue;
  if (count == 0) return hipSuccess;
  write_words_kernel<<<1, 64, 0, s>>>(dst, w, static_cast<uint32_t>(count));
  return hipGetLastError();
}

}  // namespace phx
