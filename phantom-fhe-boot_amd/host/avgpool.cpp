// avgpool.cpp — see avgpool.h
#include "avgpool.h"

#include <algorithm>
#include <cstring>
#include <stdexcept>

#include "../csrc/ckks.h"
#include "../csrc/conv.h"
#include "../csrc/rns.h"
#include "buffer.h"
#include "hip_check.h"
#include "rns_tool.h"

namespace phantom {

void avgpool_shape(size_t n, size_t width, size_t slotstr) {
  if (width < 2 || width > 64 || (width & (width - 1)))
    throw std::invalid_argument("avgpool: width must be a power of two in 2..64");
  if (slotstr >= 32 || (width << slotstr) > (size_t(1) << 31)) throw std::invalid_argument("avgpool: slot stride too large");
  const size_t lg = width << slotstr;
  if (lg * lg > n / 2) throw std::invalid_argument("avgpool: the image does not fit the slots");
}

std::vector<int> avgpool_rotations(size_t width, size_t slotstr) {
  const long pw = 1l << slotstr, lg = static_cast<long>(width) * pw;
  std::vector<int> r;
  r.reserve(2 * (width - 1));
  for (long i = 1; i < static_cast<long>(width); ++i) r.push_back(static_cast<int>(i * pw));
  for (long j = 1; j < static_cast<long>(width); ++j) r.push_back(static_cast<int>(j * lg * pw));
  return r;
}

namespace {

// host words to device memory in stream order, without a host-to-device copy (phx::write_words)
void write_table(uint64_t* dst, const std::vector<uint64_t>& w, hipStream_t s) {
  for (size_t w0 = 0; w0 < w.size(); w0 += phx::kWordsMax) {
    const size_t cnt = std::min<size_t>(phx::kWordsMax, w.size() - w0);
    phx::Words chunk;
    std::memcpy(chunk.w, w.data() + w0, cnt * sizeof(uint64_t));
    hip_ok(phx::write_words(dst + w0, chunk, cnt, s), "avgpool table");
  }
}

const RnsTool& checked_tool(const PhantomContext& ctx, size_t chain_index) {
  if (chain_index < 1 || chain_index >= ctx.total_parm_size()) throw std::invalid_argument("invalid chain index");
  return ctx.get_context_data(chain_index).gpu_rns_tool();
}

}  // namespace

size_t mix_table_words(size_t K, size_t M, size_t L) {
  return L * K * phx::mix_tiles(M) * phx::mix_tile(M) + M * L + K + M;
}

void ct_mix_raw(const PhantomContext& ctx, size_t chain_index, const uint64_t* const* ins, size_t K,
                const uint64_t* coef, const uint64_t* cadd, uint64_t* const* outs, size_t M, uint64_t* table,
                hipStream_t s) {
  if (!ins || !coef || !outs || !table) throw std::invalid_argument("null pointer");
  if (K == 0 || M == 0 || K > (size_t(1) << 20) || M > (size_t(1) << 16))
    throw std::invalid_argument("ct_mix: term and output counts must be at least 1");
  const RnsTool& rt = checked_tool(ctx, chain_index);
  const size_t L = rt.size_Ql(), m_pad = phx::mix_tiles(M) * phx::mix_tile(M);
  const auto& mods = ctx.get_context_data(chain_index).moduli();
  for (size_t k = 0; k < K; ++k)
    if (!ins[k]) throw std::invalid_argument("null input");
  for (size_t m = 0; m < M; ++m)
    if (!outs[m]) throw std::invalid_argument("null output");
  std::vector<uint64_t> tab(mix_table_words(K, M, L), 0);
  for (size_t m = 0; m < M; ++m)
    for (size_t k = 0; k < K; ++k)
      for (size_t l = 0; l < L; ++l) tab[(l * K + k) * m_pad + m] = coef[(m * K + k) * L + l] % mods[l];
  const size_t cadd_at = L * K * m_pad, ins_at = cadd_at + M * L, outs_at = ins_at + K;
  if (cadd)
    for (size_t i = 0; i < M * L; ++i) tab[cadd_at + i] = cadd[i] % mods[i % L];
  for (size_t k = 0; k < K; ++k) tab[ins_at + k] = reinterpret_cast<uint64_t>(ins[k]);
  for (size_t m = 0; m < M; ++m) tab[outs_at + m] = reinterpret_cast<uint64_t>(outs[m]);
  write_table(table, tab, s);
  phx::MixArgs a;
  a.ins = reinterpret_cast<const uint64_t* const*>(table + ins_at);
  a.outs = reinterpret_cast<uint64_t* const*>(table + outs_at);
  a.coef = table;
  a.cadd = cadd ? table + cadd_at : nullptr;
  a.q = ctx.mod_QP().q;
  a.barrett = ctx.mod_QP().barrett;
  a.K = static_cast<uint32_t>(K);
  a.M = static_cast<uint32_t>(M);
  a.L = static_cast<uint32_t>(L);
  hip_ok(phx::ct_mix(a, ctx.poly_degree(), s), "ct_mix");
}

void avgpool_fc_raw(const PhantomContext& ctx, size_t chain_index, const uint64_t* const* cts, size_t t, size_t T,
                    size_t width, size_t slotstr, const uint64_t* coef, const uint64_t* bias,
                    const uint64_t* const* const* col_evk, const uint64_t* const* const* row_evk,
                    const uint32_t* col_elts, const uint32_t* row_elts, uint64_t* const* outs, hipStream_t s) {
  if (!cts || !coef || !bias || !col_evk || !row_evk || !col_elts || !row_elts || !outs)
    throw std::invalid_argument("null pointer");
  if (t == 0 || T == 0 || t > (size_t(1) << 20) || T > (size_t(1) << 16))
    throw std::invalid_argument("avgpool: no channels");
  const size_t n = ctx.poly_degree();
  avgpool_shape(n, width, slotstr);
  const RnsTool& rt = checked_tool(ctx, chain_index);
  if (ctx.size_P() == 0) throw std::invalid_argument("no special primes");
  const size_t R = width - 1;
  for (size_t k = 0; k < t; ++k)
    if (!cts[k]) throw std::invalid_argument("null input channel");
  for (size_t u = 0; u < T; ++u)
    if (!outs[u]) throw std::invalid_argument("null output channel");
  for (size_t i = 0; i < R; ++i)
    if (!col_evk[i] || !row_evk[i]) throw std::invalid_argument("avgpool: null rotation key");
  static_assert(phx::kKsSumMax >= 63, "width <= 64");

  const size_t Ql = rt.size_Ql(), QlP = Ql + ctx.size_P(), beta = rt.beta();
  const size_t ct_words = 2 * Ql * n, ext_words = 2 * QlP * n;
  const phx::NttTables& ntt = ctx.gpu_rns_tables();
  const auto& mods = ctx.get_context_data(chain_index).moduli();

  // the entries of both directions (columns, then rows) and the bias residues, one table
  static_assert(sizeof(phx::KsSumEntry) == 2 * sizeof(uint64_t), "entries are copied as words");
  std::vector<uint64_t> tab(4 * R + T * Ql);
  for (size_t d = 0; d < 2; ++d)
    for (size_t i = 0; i < R; ++i) {
      tab[2 * (d * R + i)] = reinterpret_cast<uint64_t>(d ? row_evk[i] : col_evk[i]);
      tab[2 * (d * R + i) + 1] = reinterpret_cast<uint64_t>(ctx.galois_perm(d ? row_elts[i] : col_elts[i]));
    }
  for (size_t i = 0; i < T * Ql; ++i) tab[4 * R + i] = bias[i] % mods[i % Ql];

  DeviceBuffer<uint64_t> table(tab.size(), s), mix_table(mix_table_words(t, T, Ql), s);
  DeviceBuffer<uint64_t> mixed(T * ct_words, s), acc(T * ext_words, s), digits(beta * QlP * n, s);
  write_table(table.get(), tab, s);

  // 1. the channel mix, t -> T
  std::vector<uint64_t*> mixed_ptrs(T);
  for (size_t u = 0; u < T; ++u) mixed_ptrs[u] = mixed.get() + u * ct_words;
  ct_mix_raw(ctx, chain_index, cts, t, coef, nullptr, mixed_ptrs.data(), T, mix_table.get(), s);

  phx::KsRotateSumArgs ra;
  ra.digits = digits.get();
  ra.count = static_cast<uint32_t>(R);
  ra.identity = 1;
  ra.qp = ctx.mod_QP().q;
  ra.qp_barrett = ctx.mod_QP().barrett;
  ra.pmod = rt.bigP_mod_q();
  ra.pmod_shoup = rt.bigP_mod_q_shoup();
  ra.ql = static_cast<uint32_t>(Ql);
  ra.qlp = static_cast<uint32_t>(QlP);
  ra.size_q = static_cast<uint32_t>(ctx.size_Q());
  ra.size_p = static_cast<uint32_t>(ctx.size_P());
  ra.beta = static_cast<uint32_t>(beta);

  // the outputs' moddown goes straight to outs when they are contiguous
  const bool contiguous = [&] {
    for (size_t u = 1; u < T; ++u)
      if (outs[u] != outs[0] + u * ct_words) return false;
    return true;
  }();
  constexpr size_t kPer = 4;  // ciphertexts per moddown (8 polynomials, the fused conversion's batch)
  for (size_t d = 0; d < 2; ++d) {
    // 2. / 4. per output: modup of c1, the direction's rotations and the identity summed in Ql u P
    ra.entries = reinterpret_cast<const phx::KsSumEntry*>(table.get() + 2 * d * R);
    for (size_t u = 0; u < T; ++u) {
      const uint64_t* ct = mixed.get() + u * ct_words;
      rt.modup(digits.get(), ct + Ql * n, ntt, s);
      ra.ct = ct;
      ra.out = acc.get() + u * ext_words;
      hip_ok(phx::keyswitch_rotate_sum(ra, n, s), "avgpool rotations");
    }
    // 3. / 4. the batched moddown of the 2 T polynomials (the pooled columns replace the mix)
    uint64_t* const dst = d == 0 || !contiguous ? mixed.get() : outs[0];
    for (size_t u0 = 0; u0 < T; u0 += kPer) {
      const size_t g = std::min(kPer, T - u0);
      rt.moddown_add(dst + u0 * ct_words, acc.get() + u0 * ext_words, false, ntt, s, 2 * g);
    }
  }
  if (!contiguous)
    for (size_t u = 0; u < T; ++u)
      PHX_CHECK(hipMemcpyAsync(outs[u], mixed.get() + u * ct_words, ct_words * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
  // 5. the bias on c0
  for (size_t u = 0; u < T; ++u)
    hip_ok(phx::poly_add_scalar(outs[u], table.get() + 4 * R + u * Ql, outs[u], ctx.mod_QP(), n, Ql, s), "avgpool bias");
}

}  // namespace phantom
