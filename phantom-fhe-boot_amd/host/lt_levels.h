// lt_levels.h — the setup of the bootstrap's linear transforms (CoeffToSlot / SlotToCoeff levels and
// the dense EvalLinearTransform level) as slot-domain diagonal maps: the stage factorisation, the
// level plan, and the pieces of one level's build that the host and the device back end share.
// FHECKKSRNS (bootstrap.h) drives them in lt_levels.cpp.
#pragma once

#include <complex>
#include <cstdint>
#include <map>
#include <vector>

#include "context.h"
#include "../csrc/ltprep.h"

namespace phantom {

namespace boot {
using cvec = std::vector<std::complex<double>>;
// a slot-domain linear map as diagonals: (T v)[p] = sum_a diag_a[p] v[p + a]  (a mod slots)
using DiagMap = std::map<int, cvec>;

// stage s (1 <= s <= log2 slots) of U's factorisation, or its inverse
DiagMap stage(size_t slots, int s, bool inverse);
// A * B (B applied first)
DiagMap compose(const DiagMap& A, const DiagMap& B, size_t slots);
// a map T on n slots applied to every n-block of an S-slot vector independently (S a multiple of
// n): each diagonal of T becomes the within-block offsets it really is, so the result is correct
// on inputs that are not n-periodic.  out_mask (period 2n) scales output slot p, in_mask (period
// 2n) input slot q; null = 1.
DiagMap lift_blocks(const DiagMap& T, size_t n, size_t S, const cvec* out_mask, const cvec* in_mask);
// apply a DiagMap to a vector (tests)
cvec apply(const DiagMap& T, const cvec& v);

// ---- one linear-transform level: the plan, and the pieces the host and the device setup share ----
// How `budget` levels share the log2(slots) stages (1 <= budget <= logslots after clamping): the
// larger groups first.
std::vector<int> split_stages(int logslots, uint32_t budget);
// One level of CoeffToSlot (encode_dir) or SlotToCoeff: its stages in the order they are composed,
// the stride of its offsets, whether the direction's constant is folded in, and its sparse mask
// (phx::kLtMask*).
struct LevelSpec {
  std::vector<int> stages;
  int stride = 1;
  bool apply_const = false;
  int mask = phx::kLtMaskNone;
};
// The levels of one direction on ns slots of n: `sizes` stages per level, taken in order from
// logslots .. 1 (CoeffToSlot) or 1 .. logslots (SlotToCoeff); stride 2^(min stage - 1); the constant
// on the first CoeffToSlot / last SlotToCoeff level; for ns < n the out mask on the last CoeffToSlot
// and the in mask on the first SlotToCoeff level.  Throws std::invalid_argument unless the sizes are
// positive and sum to log2 ns.
std::vector<LevelSpec> plan_levels(size_t ns, size_t n, const std::vector<int>& sizes, bool encode_dir);

// The baby-step giant-step shape of a level from its diagonal offsets on n ring slots (multiples
// of `stride`; dim1 = 0: g^2 >= 2 D): diagonals (u - center) * stride, u < D, evaluated as baby
// steps j < g and giant steps i < b.
struct LtShape {
  int stride = 1, center = 0, D = 0, g = 1, b = 1;
};
LtShape lt_shape(const std::vector<int>& keys, size_t n, uint32_t dim1, int stride);
// the present slots of a level of `shape` whose offsets on n slots are `keys` (sorted), in slot
// order: slot u, its offset, and the pre-rotation g (u / g) stride mod n that lets the giant
// rotation follow the inner sum
struct LtSlot {
  int u = 0, key = 0;
  size_t shift = 0;
};
std::vector<LtSlot> present_slots(const LtShape& shape, size_t n, const std::vector<int>& keys);
// compose(stage(s_k), .. compose(stage(s_1), I)) on ns slots by set arithmetic alone (compose never
// drops a key): the sorted offsets after every stage, and per stage the table phx::ltprep_stage
// reads ([D_t][3] rows of the previous band, -1 = none), back to back in `src`.
struct StagePlan {
  size_t ns = 0;
  std::vector<int> stages;
  std::vector<std::vector<int>> keys;  // [stage][D_t]
  std::vector<int32_t> src;
  std::vector<size_t> src_at;  // [stage] first word of its table in src
  size_t max_diagonals() const;
  const std::vector<int>& offsets() const { return keys.back(); }
};
// throws std::invalid_argument unless ns is a power of two >= 2 and every 1 <= s <= log2 ns
StagePlan plan_stages(size_t ns, const std::vector<int>& stages);
// the plan's product on the host ...
DiagMap stage_products_host(const StagePlan& plan, bool inverse);
// ... and on the device: runs the stages on `stream`, ping-pong between `first` (written by the
// first stage) and `second` ([max_diagonals()][ns] complex each, device); dev_src = the plan's src
// words in device memory; returns the buffer that holds the result [offsets().size()][ns]
void* stage_products_device(const PhantomContext& cc, const StagePlan& plan, bool inverse, const int32_t* dev_src,
                            void* first, void* second, hipStream_t stream);
// The finish of one level on the host (what phx::ltprep_presence + phx::ltprep_finish do on the
// device): level constant, lift to n slots with the optional out / in mask (mask: phx::kLtMask*),
// and the shape of the offsets that remain.
DiagMap finish_map(DiagMap T, size_t ns, size_t n, std::complex<double> cf, bool apply_const, int mask, uint32_t dim1,
                   int stride, LtShape& shape);
// finish_map, then the present diagonals in slot order, pre-rotated: (slot u, offset on n slots,
// values [n]).  The host setup encodes from finish_map directly, one pre-rotated copy at a time.
struct FinishedDiagonal {
  int slot = 0, key = 0;
  cvec values;
};
std::vector<FinishedDiagonal> finish_host(DiagMap T, size_t ns, size_t n, std::complex<double> cf, bool apply_const,
                                          int mask, uint32_t dim1, int stride, LtShape& shape);
// offsets on n slots of the block-periodic lift of diagonals `offsets` on ns slots, from the
// presence flags of phx::ltprep_presence (ns == n: the offsets themselves)
std::vector<int> lifted_keys(const std::vector<int>& offsets, const std::vector<int>& flags, size_t ns, size_t n);
// the rows phx::ltprep_finish reads for a level of `shape` whose present offsets on n slots are
// `keys`, from a band on ns slots with offsets `band_offsets` (both sorted); returns each row's slot u
std::vector<int> finish_rows(const LtShape& shape, size_t ns, size_t n, const std::vector<int>& band_offsets,
                             const std::vector<int>& keys, std::vector<phx::LtFinishRow>& rows);
}  // namespace boot

}  // namespace phantom
