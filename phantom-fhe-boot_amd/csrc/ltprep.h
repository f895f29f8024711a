// ltprep.h — the bootstrap's linear-transform diagonals on gfx950: the products of the slot-domain
// butterfly stages (boot::stage / boot::compose of host/bootstrap.h), the level constant, the
// block-periodic lift of a sparse setup (boot::lift_blocks), the giant-step pre-rotation, and the
// diagonals of a dense matrix.  Their output is the batch of slot vectors the batched device
// encoder (encode.h) reads.
//
// FP64 streaming kernels: one complex value (16 bytes) per lane, lanes along the slot index, so
// every access is a contiguous run (a rotated read (p + a) mod ns is two of them).  Device code is
// built with contraction off, and every value is formed by the same nesting of complex products
// (a c - b d, a d + b c) as the host code, so the numbers equal the host's (up to the sign of a zero).
// Every launcher enqueues on the caller's stream only and checks its arguments first
// (hipErrorInvalidValue, nothing enqueued).
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace phx {

// One stage applied to a band of diagonals: out = compose(stage(ns, s, inverse), prev).
// zeta: EmbedTables::zeta of a ring of degree ring_n (zeta[j] = exp(2 pi i j / (2 ring_n)));
// ns slots (a power of two, 2 <= ns <= ring_n / 2), 1 <= s <= log2 ns, h = 2^(s-1).
// prev [D_prev][ns] (null: the identity map, one diagonal of ones at offset 0), out [D_out][ns].
// src (device) [D_out][3]: for the output diagonal at offset c, the row of prev holding offset c
// (the stage's diagonal 0), c - h (its diagonal +h) and c + h (its diagonal -h), each mod ns, or -1
// where prev has no such diagonal.  Every row index must be below D_prev (not checked on the device).
hipError_t ltprep_stage(const double2* zeta, size_t ring_n, size_t ns, int s, bool inverse, const double2* prev,
                        double2* out, const int32_t* src, int D_out, hipStream_t stream);

// Presence of a band's diagonals after the level constant: flags [2 D] (device, ints, OR-ed into:
// clear them first).  flags[2 i] is set when some band[i][r] * cf is non-zero with r + offsets[i] < ns,
// flags[2 i + 1] when some is with r + offsets[i] >= ns (the two lifted offsets a and a - ns).
// apply_const = false tests band[i][r] itself.
hipError_t ltprep_presence(const double2* band, size_t ns, const int32_t* offsets, int D, double2 cf, bool apply_const,
                           int* flags, hipStream_t stream);

// One output diagonal of ltprep_finish.
struct LtFinishRow {
  int32_t src;  // row of the band
  int32_t a;    // that row's offset on ns slots
  int32_t key;  // the output diagonal's offset on n slots (ns == n: key == a)
  int32_t sh;   // pre-rotation: out[p] = diag[(p + n - sh) mod n]
};
constexpr int kLtMaskNone = 0, kLtMaskOut = 1, kLtMaskIn = 2;
// out [K][n] from band [.][ns]: value = band[src][r] (times cf when apply_const), r = p' mod ns,
// p' = (p + n - sh) mod n.  ns < n lifts block-periodically: key < ns keeps the entries with
// r + a < ns, any other key those with r + a >= ns, the rest are zero; a non-zero value is then
// times (1, -i)[p' mod 2 ns >= ns] (kLtMaskOut) or (1, i)[(p' + key) mod 2 ns >= ns] (kLtMaskIn).
// ns and n powers of two, ns <= n; rows (device) [K].
hipError_t ltprep_finish(const double2* band, size_t ns, size_t n, const LtFinishRow* rows, int K, double2 cf,
                         bool apply_const, int mask, double2* out, hipStream_t stream);

// Diagonals of a dense row-major slots x slots matrix: out[k][p] = A[p][(p + k) mod slots] * scale,
// flags[k] (device, ints, clear them first) set when diagonal k has a non-zero entry.
hipError_t ltprep_dense(const double2* A, size_t slots, double scale, double2* out, int* flags, hipStream_t stream);

}  // namespace phx
