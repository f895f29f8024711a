// pack.cpp — see pack.h
#include "pack.h"

#include <algorithm>
#include <cstring>
#include <stdexcept>

#include "../csrc/ckks.h"
#include "../csrc/conv.h"
#include "buffer.h"
#include "ckks_eval.h"
#include "hip_check.h"
#include "rns_tool.h"

namespace phantom {

static_assert(kPackMax == static_cast<size_t>(phx::kPackMax) && kPackMax == static_cast<size_t>(phx::kSplitMax));

namespace {

bool pow2(size_t x) { return x && !(x & (x - 1)); }

// ns = (width 2^slotstr)^2 for a power-of-two width, or std::invalid_argument
size_t pack_ns(size_t width, size_t slotstr) {
  if (!pow2(width)) throw std::invalid_argument("pack: width must be a power of two");
  if (slotstr >= 16 || (width << slotstr) > (size_t(1) << 15)) throw std::invalid_argument("pack: slot stride too large");
  const size_t lg = width << slotstr;
  return lg * lg;
}

size_t checked_pack(size_t pack, size_t capacity) {
  if (!pow2(pack)) throw std::invalid_argument("pack: the pack must be a power of two");
  if (pack > capacity) throw std::invalid_argument("pack: the pack exceeds the capacity min(N / (2 ns), 64)");
  size_t g = 0;
  while ((size_t(1) << g) < pack) ++g;
  return g;
}

// host words to device memory in stream order, without a host-to-device copy (phx::write_words)
void write_table(uint64_t* dst, const std::vector<uint64_t>& w, hipStream_t s) {
  if (w.size() > static_cast<size_t>(phx::kWordsMax)) throw std::logic_error("pack: table too large");
  phx::Words chunk;
  std::memcpy(chunk.w, w.data(), w.size() * sizeof(uint64_t));
  hip_ok(phx::write_words(dst, chunk, w.size(), s), "pack table");
}

size_t checked_limbs(const PhantomContext& ctx, size_t chain_index) {
  if (chain_index < 1 || chain_index >= ctx.total_parm_size()) throw std::invalid_argument("invalid chain index");
  return ctx.get_context_data(chain_index).gpu_rns_tool().size_Ql();
}

bool overlap(const uint64_t* x, const uint64_t* y, size_t words) { return x < y + words && y < x + words; }
bool misaligned(const void* p) { return reinterpret_cast<uintptr_t>(p) & 15; }

void like(const PhantomContext& ctx, const PhantomCiphertext& src, PhantomCiphertext& o) {
  o.resize(ctx, src.chain_index(), 2, ctx.stream(), false);
  o.set_ntt_form(true);
  o.set_scale(src.scale());
  o.SetNoiseScaleDeg(src.GetNoiseScaleDeg());
  o.set_correction_factor(src.correction_factor());
  o.set_asymmetric(src.is_asymmetric());
}

}  // namespace

size_t pack_capacity(size_t n, size_t width, size_t slotstr) {
  const size_t ns = pack_ns(width, slotstr);
  if (!pow2(n) || 2 * ns > n) throw std::invalid_argument("pack: the image does not fit the slots");
  return std::min(n / (2 * ns), kPackMax);
}

PackPlan pack_plan(size_t n, size_t width, size_t slotstr, size_t pack) {
  PackPlan p;
  p.log_pack = checked_pack(pack, pack_capacity(n, width, slotstr));
  p.n = n, p.width = width, p.slotstr = slotstr, p.ns = pack_ns(width, slotstr), p.pack = pack;
  p.stride = static_cast<uint32_t>(n / (2 * pack * p.ns));
  p.rotations = pack_rotations(width, slotstr, pack);
  for (size_t t = 0; t < p.log_pack; ++t) {
    p.galois.push_back(FindAutomorphismIndex2nComplex(p.rotations[t], n));
    p.powers.push_back(p.stride << t);
  }
  return p;
}

std::vector<int> pack_rotations(size_t width, size_t slotstr, size_t pack) {
  const size_t ns = pack_ns(width, slotstr), g = checked_pack(pack, kPackMax);
  if (pack * ns > (size_t(1) << 30)) throw std::invalid_argument("pack: too many slots");
  std::vector<int> r;
  for (size_t t = 0; t < g; ++t) r.push_back(static_cast<int>((pack * ns) >> (t + 1)));
  return r;
}

void ct_pack_raw(const PhantomContext& ctx, size_t chain_index, const uint64_t* const* ins, size_t C,
                 uint32_t stride_power, uint64_t* out, hipStream_t s, uint32_t lead) {
  if (!ins || !out) throw std::invalid_argument("null pointer");
  if (C < 1 || C > kPackMax || lead > kPackMax - C) throw std::invalid_argument("ct_pack: 1 to 64 channels");
  const size_t n = ctx.poly_degree(), L = checked_limbs(ctx, chain_index), words = 2 * L * n;
  if (stride_power >= 2 * n) throw std::invalid_argument("ct_pack: the stride power must be below 2N");
  if (misaligned(out)) throw std::invalid_argument("ct_pack: ciphertexts must be 16-byte aligned");
  for (size_t c = 0; c < C; ++c) {
    if (!ins[c]) throw std::invalid_argument("null input channel");
    if (misaligned(ins[c])) throw std::invalid_argument("ct_pack: ciphertexts must be 16-byte aligned");
    if (overlap(ins[c], out, words)) throw std::invalid_argument("ct_pack: the output overlaps an input");
  }
  phx::PackArgs a;
  a.w = ctx.monomial_ntt(stride_power, L);
  a.out = out;
  a.q = ctx.mod_QP().q;
  a.barrett = ctx.mod_QP().barrett;
  a.C = static_cast<uint32_t>(C);
  a.L = static_cast<uint32_t>(L);
  a.lead = lead;
  DeviceBuffer<uint64_t> table;
  if (C <= static_cast<size_t>(phx::kPackInline)) {
    std::copy(ins, ins + C, a.in);
  } else {
    std::vector<uint64_t> tab(C);
    for (size_t c = 0; c < C; ++c) tab[c] = reinterpret_cast<uint64_t>(ins[c]);
    table = DeviceBuffer<uint64_t>(C, s);
    write_table(table.get(), tab, s);
    a.table = reinterpret_cast<const uint64_t* const*>(table.get());
  }
  hip_ok(phx::ct_pack(a, n, s), "ct_pack");
}

void ct_split_raw(const PhantomContext& ctx, size_t chain_index, const uint64_t* const* av, const uint64_t* const* rv,
                  size_t count, uint32_t power, uint64_t* const* even, uint64_t* const* odd, hipStream_t s) {
  if (!av || !rv || (!even && !odd)) throw std::invalid_argument("null pointer");
  if (count < 1 || count > kPackMax) throw std::invalid_argument("ct_split: 1 to 64 nodes");
  const size_t n = ctx.poly_degree(), L = checked_limbs(ctx, chain_index), words = 2 * L * n;
  if (power >= 2 * n) throw std::invalid_argument("ct_split: the power must be below 2N");
  static_assert(sizeof(phx::SplitNode) == 4 * sizeof(uint64_t), "nodes are copied as words");
  std::vector<phx::SplitNode> nodes(count);
  for (size_t k = 0; k < count; ++k) {
    nodes[k] = {av[k], rv[k], even ? even[k] : nullptr, odd ? odd[k] : nullptr};
    if (!av[k] || !rv[k]) throw std::invalid_argument("null input node");
    if (misaligned(av[k]) || misaligned(rv[k]) || misaligned(nodes[k].even) || misaligned(nodes[k].odd))
      throw std::invalid_argument("ct_split: ciphertexts must be 16-byte aligned");
  }
  // no output may overlap an input or another output, except even[k] == a[k]
  std::vector<std::pair<uint64_t*, size_t>> outs;  // (output, the node whose a it may alias or count)
  for (size_t k = 0; k < count; ++k) {
    if (nodes[k].even) outs.emplace_back(nodes[k].even, k);
    if (nodes[k].odd) outs.emplace_back(nodes[k].odd, count);
  }
  for (size_t x = 0; x < outs.size(); ++x) {
    uint64_t* const o = outs[x].first;
    for (size_t j = 0; j < count; ++j) {
      const bool own_even = outs[x].second == j && o == nodes[j].a;
      if ((!own_even && overlap(o, nodes[j].a, words)) || overlap(o, nodes[j].r, words))
        throw std::invalid_argument("ct_split: an output overlaps an input (only even[k] == a[k] is allowed)");
    }
    for (size_t y = x + 1; y < outs.size(); ++y)
      if (overlap(o, outs[y].first, words)) throw std::invalid_argument("ct_split: two outputs overlap");
  }
  phx::SplitArgs a;
  a.m = ctx.monomial_ntt(static_cast<uint32_t>((2 * n - power) % (2 * n)), L);
  a.q = ctx.mod_QP().q;
  a.barrett = ctx.mod_QP().barrett;
  a.count = static_cast<uint32_t>(count);
  a.L = static_cast<uint32_t>(L);
  DeviceBuffer<uint64_t> table;
  if (count <= static_cast<size_t>(phx::kSplitInline)) {
    std::copy(nodes.begin(), nodes.end(), a.node);
  } else {
    std::vector<uint64_t> tab(4 * count);
    std::memcpy(tab.data(), nodes.data(), tab.size() * sizeof(uint64_t));
    table = DeviceBuffer<uint64_t>(tab.size(), s);
    write_table(table.get(), tab, s);
    a.table = reinterpret_cast<const phx::SplitNode*>(table.get());
  }
  hip_ok(phx::ct_split(a, n, s), "ct_split");
}

PhantomCiphertext pack_channels(const PhantomContext& ctx, const PackPlan& plan, const PhantomCiphertext* const* chans,
                                size_t C) {
  if (!chans || C < 1 || C > plan.pack) throw std::invalid_argument("pack_channels: 1 to pack channels");
  if (plan.n != ctx.poly_degree()) throw std::invalid_argument("pack_channels: the plan is for another ring degree");
  const PhantomCiphertext& first = *chans[0];
  std::vector<const uint64_t*> ins(C);
  for (size_t c = 0; c < C; ++c) {
    const PhantomCiphertext& x = *chans[c];
    if (x.size() != 2 || !x.is_ntt_form() || x.chain_index() != first.chain_index() || x.scale() != first.scale() ||
        x.GetNoiseScaleDeg() != first.GetNoiseScaleDeg())
      throw std::invalid_argument("pack_channels: the channels must share level, noise-scale degree and scale");
    ins[c] = x.data();
  }
  PhantomCiphertext out;
  like(ctx, first, out);
  ct_pack_raw(ctx, first.chain_index(), ins.data(), C, plan.stride, out.data(), ctx.stream(),
              static_cast<uint32_t>(plan.lead(C)));
  return out;
}

std::vector<PhantomCiphertext> unpack_channels(const PhantomContext& ctx, const PackPlan& plan,
                                               const PhantomCiphertext& packed, size_t C, const PhantomGaloisKey& keys) {
  if (C < 1 || C > plan.pack) throw std::invalid_argument("unpack_channels: 1 to pack channels");
  if (plan.n != ctx.poly_degree()) throw std::invalid_argument("unpack_channels: the plan is for another ring degree");
  if (packed.size() != 2 || !packed.is_ntt_form()) throw std::invalid_argument("unpack_channels: a 2-polynomial NTT-form input");
  for (uint32_t e : plan.galois)
    if (!keys.has(e)) throw std::invalid_argument("unpack_channels: no rotation key for a tree level (AddPackRotationsTo)");
  std::vector<PhantomCiphertext> node(plan.pack);
  std::vector<bool> have(plan.pack, false);
  node[0] = packed;
  have[0] = true;
  for (size_t t = 0; t < plan.log_pack; ++t) {
    const size_t half = size_t(1) << t;
    std::vector<PhantomCiphertext> rot;
    std::vector<const uint64_t*> a, r;
    std::vector<uint64_t*> even, odd;
    for (size_t idx = 0; idx < half; ++idx) {
      if (!have[idx]) continue;
      rot.push_back(EvalRotateFused(ctx, node[idx], keys, plan.rotations[t]));
      const size_t child = idx | half;
      const bool ev = plan.needed(idx, t + 1, C), od = plan.needed(child, t + 1, C);
      if (od) like(ctx, packed, node[child]);
      a.push_back(node[idx].data());
      r.push_back(rot.back().data());
      even.push_back(ev ? node[idx].data() : nullptr);
      odd.push_back(od ? node[child].data() : nullptr);
      have[idx] = ev;
      have[child] = od;
    }
    ct_split_raw(ctx, packed.chain_index(), a.data(), r.data(), a.size(), plan.powers[t], even.data(), odd.data(),
                 ctx.stream());
  }
  std::vector<PhantomCiphertext> out(C);
  for (size_t c = 0; c < C; ++c) out[c] = std::move(node[plan.lead(C) + c]);
  return out;
}

std::vector<std::vector<PhantomCiphertext>> unpack_channels_batch(const PhantomContext& ctx, const PackPlan& plan,
                                                                  std::span<const PhantomCiphertext* const> packed,
                                                                  std::span<const size_t> channels,
                                                                  const PhantomGaloisKey& keys) {
  const size_t G = packed.size();
  if (channels.size() != G) throw std::invalid_argument("unpack_channels_batch: one channel count per group");
  if (plan.n != ctx.poly_degree()) throw std::invalid_argument("unpack_channels_batch: the plan is for another ring degree");
  for (size_t g = 0; g < G; ++g) {
    if (!packed[g]) throw std::invalid_argument("unpack_channels_batch: null group");
    if (channels[g] < 1 || channels[g] > plan.pack) throw std::invalid_argument("unpack_channels_batch: 1 to pack channels");
    if (packed[g]->size() != 2 || !packed[g]->is_ntt_form())
      throw std::invalid_argument("unpack_channels_batch: a 2-polynomial NTT-form input");
    if (packed[g]->chain_index() != packed[0]->chain_index())
      throw std::invalid_argument("unpack_channels_batch: the groups must share a chain index");
  }
  for (uint32_t e : plan.galois)
    if (!keys.has(e)) throw std::invalid_argument("unpack_channels_batch: no rotation key for a tree level (AddPackRotationsTo)");
  std::vector<std::vector<PhantomCiphertext>> out(G);
  if (G == 0) return out;
  const size_t chain = packed[0]->chain_index(), words = 2 * checked_limbs(ctx, chain) * ctx.poly_degree();
  const size_t chunk = std::min(rotate_fused_batch_chunk(ctx, chain), static_cast<size_t>(phx::kSplitMax));
  hipStream_t s = ctx.stream();
  std::vector<std::vector<PhantomCiphertext>> node(G);
  std::vector<std::vector<bool>> have(G, std::vector<bool>(plan.pack, false));
  for (size_t g = 0; g < G; ++g) {
    node[g].resize(plan.pack);
    node[g][0] = *packed[g];
    have[g][0] = true;
  }
  for (size_t t = 0; t < plan.log_pack; ++t) {
    const size_t half = size_t(1) << t;
    // the level's live nodes of every group, in unpack_channels' order within a group: they share the key
    std::vector<const uint64_t*> a;
    std::vector<uint64_t*> even, odd;
    std::vector<PhantomCiphertext*> spent;  // nodes whose even child is pruned: read by this level only
    for (size_t g = 0; g < G; ++g)
      for (size_t idx = 0; idx < half; ++idx) {
        if (!have[g][idx]) continue;
        const size_t child = idx | half;
        const bool ev = plan.needed(idx, t + 1, channels[g]), od = plan.needed(child, t + 1, channels[g]);
        if (od) like(ctx, *packed[g], node[g][child]);
        if (!ev) spent.push_back(&node[g][idx]);
        a.push_back(node[g][idx].data());
        even.push_back(ev ? node[g][idx].data() : nullptr);
        odd.push_back(od ? node[g][child].data() : nullptr);
        have[g][idx] = ev;
        have[g][child] = od;
      }
    const uint64_t* const* evk = keys.get(plan.galois[t]).public_keys_ptr();
    for (size_t at = 0; at < a.size(); at += chunk) {
      const size_t c = std::min(chunk, a.size() - at);
      // the rotated nodes stay in the batch's slab: ct_split takes a pointer per node
      DeviceBuffer<uint64_t> slab(c * words, s);
      rotate_fused_batch_slab(ctx, chain, a.data() + at, c, evk, plan.galois[t], slab.get(), s);
      std::vector<const uint64_t*> r(c);
      for (size_t k = 0; k < c; ++k) r[k] = slab.get() + k * words;
      ct_split_raw(ctx, chain, a.data() + at, r.data(), c, plan.powers[t], even.data() + at, odd.data() + at, s);
    }
    // back to the pool in stream order, after the level's splits that read them
    for (PhantomCiphertext* c : spent) {
      c->retag(s);
      *c = PhantomCiphertext();
    }
  }
  for (size_t g = 0; g < G; ++g) {
    out[g].resize(channels[g]);
    for (size_t c = 0; c < channels[g]; ++c) out[g][c] = std::move(node[g][plan.lead(channels[g]) + c]);
  }
  return out;
}

}  // namespace phantom
