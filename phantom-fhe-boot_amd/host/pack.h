// pack.h — channel packing for the tensor bootstrap, shared by the DNN façade (host/dnn.h) and the
// C-ABI (csrc/capi_pack.cpp).
//
// A channel of a TensorCT is a sparse-packed message of ns = (width 2^slotstr)^2 slots, i.e. a
// polynomial in X^G with G = N / (2 ns).  Bootstrapping acts on coefficients, so P <= G channels
// (P a power of two, the pack) are interleaved into one ciphertext by monomial shifts,
//   packed = sum_{c < C} X^((lead + c) D) ct_c,   D = G / P = N / (2 P ns),   C <= P,
// (lead = 0 for a full group, 1 otherwise: PackPlan::lead)
// at no key switch and no level.  The packed message lies in the subring of X^D, the subring of a
// P ns-slot ciphertext, with channel c on the powers j of X^D with j mod P = c.  One bootstrap at
// P ns slots refreshes all of them, and a binary tree takes them apart: node 0 is the packed
// ciphertext, and level t = 0 .. g-1 (g = log2 P) does for every node a with index idx
//   rot = rotation of a by r_t = P ns / 2^(t+1) slots      (one key switch)
//   node idx        = a + rot
//   node idx | 2^t  = (a - rot) X^(2N - D 2^t)
// because that rotation multiplies power i of X^(D 2^t) by (-1)^i.  After level g-1 node c holds P
// times the message of the channel at index c.  A node whose subtree holds no channel is not computed:
// P - 1 rotations for C = P, fewer otherwise.  The rotations are {ns 2^i : 0 <= i < g}.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <span>
#include <vector>

#include "ciphertext.h"
#include "context.h"
#include "keys.h"

namespace phantom {

constexpr size_t kPackMax = 64;  // phx::kPackMax

struct PackPlan {
  size_t n = 0, width = 0, slotstr = 0, ns = 0, pack = 1, log_pack = 0;
  uint32_t stride = 0;             // D: channel c is shifted by X^(c D)
  std::vector<int> rotations;      // level t: pack ns / 2^(t+1) slots
  std::vector<uint32_t> galois;    // 5^(rotation) mod 2n
  std::vector<uint32_t> powers;    // level t: D 2^t, the shift the odd child undoes (times X^(2n - D 2^t))
  size_t slots() const { return pack * ns; }  // the packed ciphertext's slot count
  // groups of `pack` channels, in order: channel c is member c % pack of group c / pack
  size_t groups(size_t num_ch) const { return (num_ch + pack - 1) / pack; }
  size_t members(size_t num_ch, size_t group) const { return std::min(pack, num_ch - group * pack); }
  // A group that is not full leaves index 0 free: its C channels sit at the tree indices lead(C) + c.
  // Coefficient 0 and the middle coefficient of the packed polynomial belong to index 0, and they are
  // where a bootstrap's slot-0 offset lands ("Where the precision goes"), so it falls
  // on the unused node and the tree discards it.  A full group has no free index.
  size_t lead(size_t C) const { return C < pack ? 1 : 0; }
  // whether the node whose index has the low `bits` bits `idx` is an ancestor of (or is) one of the
  // C channels' nodes: only those are computed
  bool needed(size_t idx, size_t bits, size_t C) const {
    for (size_t m = lead(C); m < lead(C) + C; ++m)
      if ((m & ((size_t(1) << bits) - 1)) == idx) return true;
    return false;
  }
};

// min(n / (2 ns), kPackMax); std::invalid_argument unless width is a power of two >= 1 and ns <= n / 2
size_t pack_capacity(size_t n, size_t width, size_t slotstr);
// std::invalid_argument also unless pack is a power of two in 1 .. pack_capacity
PackPlan pack_plan(size_t n, size_t width, size_t slotstr, size_t pack);
// the plan's rotations without a ring degree (a key generator's view)
std::vector<int> pack_rotations(size_t width, size_t slotstr, size_t pack);

// Raw forms on host arrays of device pointers to [2][Ql][n] ciphertexts at `chain_index`, enqueued on
// `s` with scratch from the pool and no synchronisation (beyond the first use of a monomial, which
// the context builds and caches).  std::invalid_argument before anything is enqueued: a null pointer,
// C of 0 or above kPackMax, a count of 0 or above kPackMax, a power >= 2n, a chain index of 0 or past
// the end, a misaligned ciphertext, an output overlapping an input other than even[k] == a[k].
// out = X^(lead stride_power) sum_c X^(c stride_power) ins[c]; C + lead <= kPackMax
void ct_pack_raw(const PhantomContext& ctx, size_t chain_index, const uint64_t* const* ins, size_t C,
                 uint32_t stride_power, uint64_t* out, hipStream_t s, uint32_t lead = 0);
// even[k] = a[k] + r[k], odd[k] = (a[k] - r[k]) X^(2n - power): `power` is the shift the odd child undoes.
// even[k] or odd[k] may be null, and one of the two arrays altogether
void ct_split_raw(const PhantomContext& ctx, size_t chain_index, const uint64_t* const* a, const uint64_t* const* r,
                  size_t count, uint32_t power, uint64_t* const* even, uint64_t* const* odd, hipStream_t s);

// sum_c X^((lead(C) + c) D) chans[c] for C <= plan.pack channels of one chain index, degree and scale (checked):
// a new ciphertext with their metadata, on the context's stream
PhantomCiphertext pack_channels(const PhantomContext& ctx, const PackPlan& plan, const PhantomCiphertext* const* chans,
                                size_t C);
// the tree: C ciphertexts with the packed one's metadata, each holding plan.pack times its channel;
// std::invalid_argument when `keys` lacks a rotation of the plan that the C channels need
std::vector<PhantomCiphertext> unpack_channels(const PhantomContext& ctx, const PackPlan& plan,
                                               const PhantomCiphertext& packed, size_t C, const PhantomGaloisKey& keys);
// the trees of several groups level by level: the live nodes of ALL groups at a level share the
// level's key, so they go through one batched rotation (rotate_fused_batch_slab, host/ckks_eval.h:
// one modup, one key switch with the key read once, one moddown) per chunk of min(its chunk size,
// phx::kSplitMax) nodes and one ct_split on the rotated nodes where they lie in the batch's slab.
// Pruning, the lead rule and the output order are unpack_channels'; result [g] equals
// unpack_channels(ctx, plan, *packed[g], channels[g], keys) word for word.  The groups share a chain
// index (std::invalid_argument otherwise, and as unpack_channels), before anything is enqueued.
std::vector<std::vector<PhantomCiphertext>> unpack_channels_batch(const PhantomContext& ctx, const PackPlan& plan,
                                                                  std::span<const PhantomCiphertext* const> packed,
                                                                  std::span<const size_t> channels,
                                                                  const PhantomGaloisKey& keys);

}  // namespace phantom
