// conv2d.cpp — see conv2d.h
#include "conv2d.h"

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstring>
#include <stdexcept>

#include "../csrc/rns.h"
#include "numth.h"
#include "buffer.h"
#include "encoder.h"
#include "hip_check.h"
#include "rns_tool.h"

namespace phantom {

phx::ConvShape conv_shape(size_t n, size_t width, size_t slotstr, size_t kernel, size_t in_ch, size_t out_ch) {
  if (width == 0 || (width & (width - 1))) throw std::invalid_argument("conv: width must be a power of two");
  if (kernel % 2 == 0 || kernel > width) throw std::invalid_argument("conv: kernel must be odd and at most width");
  if (in_ch == 0 || out_ch == 0) throw std::invalid_argument("conv: no channels");
  if (in_ch > (size_t(1) << 20) || out_ch > (size_t(1) << 20)) throw std::invalid_argument("conv: too many channels");
  // ns = (width 2^slotstr)^2 <= n / 2, checked without overflow
  if (slotstr >= 32 || (width << slotstr) > (size_t(1) << 31)) throw std::invalid_argument("conv: slot stride too large");
  const size_t lg = width << slotstr;
  if (lg * lg > n / 2) throw std::invalid_argument("conv: the image does not fit the slots");
  phx::ConvShape c;
  c.width = static_cast<uint32_t>(width);
  c.slotstr = static_cast<uint32_t>(slotstr);
  c.kernel = static_cast<uint32_t>(kernel);
  c.in_ch = static_cast<uint32_t>(in_ch);
  c.out_ch = static_cast<uint32_t>(out_ch);
  return c;
}

std::vector<int> conv_rotations(size_t width, size_t slotstr, size_t kernel) {
  const long lg = static_cast<long>(width << slotstr), half = static_cast<long>(kernel / 2);
  std::vector<int> r;
  r.reserve(kernel * kernel);
  for (long a = 0; a < static_cast<long>(kernel); ++a)
    for (long b = 0; b < static_cast<long>(kernel); ++b)
      r.push_back(static_cast<int>(((a - half) * lg + (b - half)) * (1l << slotstr)));
  return r;
}

size_t conv_group(const PhantomContext& ctx, size_t chain_index, const phx::ConvShape& c) {
  const size_t QlP = ctx.get_context_data(chain_index).gpu_rns_tool().size_Ql() + ctx.size_P();
  const size_t per_output = static_cast<size_t>(c.in_ch) * c.kernel * c.kernel * QlP * ctx.poly_degree() * sizeof(uint64_t);
  return std::clamp<size_t>(kConvPlainBudget / per_output, 1, c.out_ch);
}

phx::MacArgs mac_args(const PhantomContext& ctx, size_t chain_index) {
  if (chain_index < 1 || chain_index >= ctx.total_parm_size()) throw std::invalid_argument("invalid chain index");
  if (ctx.size_P() == 0) throw std::invalid_argument("no special primes");
  phx::MacArgs a;
  a.Ql = static_cast<uint32_t>(ctx.get_context_data(chain_index).gpu_rns_tool().size_Ql());
  a.P = static_cast<uint32_t>(ctx.size_P());
  a.size_Q = static_cast<uint32_t>(ctx.size_Q());
  a.q = ctx.mod_QP().q;
  a.barrett = ctx.mod_QP().barrett;
  a.q60 = below_2_60(ctx.key_moduli());
  return a;
}

namespace {

// the operand checks conv2d_raw and conv2d_apply share, before anything is enqueued
void check_operands(const phx::ConvShape& c, const uint64_t* const* cts, const uint64_t* const* const* evk,
                    uint64_t* const* outs) {
  const size_t K2 = static_cast<size_t>(c.kernel) * c.kernel;
  for (size_t k = 0; k < c.in_ch; ++k)
    if (!cts[k]) throw std::invalid_argument("null input channel");
  for (size_t h = 0; h < c.out_ch; ++h)
    if (!outs[h]) throw std::invalid_argument("null output channel");
  for (size_t t = 0; t < K2; ++t)
    if (!evk[t] && t != K2 / 2) throw std::invalid_argument("conv: only the centre tap goes without a rotation key");
}

// every rotation of every input channel in the extended basis: term (k, tap) at
// rots + (k K^2 + tap) ext_words (in_ch modups and batched rotation launches)
void conv_rotate(const PhantomContext& ctx, size_t chain_index, const uint64_t* const* cts, const phx::ConvShape& c,
                 const uint64_t* const* const* evk, const uint32_t* galois_elts, uint64_t* rots, hipStream_t s) {
  const size_t n = ctx.poly_degree();
  const RnsTool& rt = ctx.get_context_data(chain_index).gpu_rns_tool();
  const size_t Ql = rt.size_Ql(), QlP = Ql + ctx.size_P(), beta = rt.beta();
  const size_t K2 = static_cast<size_t>(c.kernel) * c.kernel, ext_words = 2 * QlP * n;
  const phx::NttTables& ntt = ctx.gpu_rns_tables();

  // the K^2 rotations' entries, the same for every input channel (outputs tap ext_words apart)
  std::vector<phx::KsBatchEntry> e(K2);
  for (size_t t = 0; t < K2; ++t) {
    if (evk[t]) {
      e[t].evk = evk[t];
      e[t].perm = ctx.galois_perm(galois_elts[t]);
      e[t].binv = ctx.galois_block_inv(galois_elts[t]);
    }
    e[t].out_off = static_cast<int64_t>(t * ext_words);
  }
  static_assert(sizeof(phx::KsBatchEntry) % sizeof(uint64_t) == 0, "entries are copied as words");
  const size_t entry_words = K2 * sizeof(phx::KsBatchEntry) / sizeof(uint64_t);
  DeviceBuffer<uint64_t> table(entry_words, s);
  for (size_t w0 = 0; w0 < entry_words; w0 += phx::kWordsMax) {
    const size_t cnt = std::min<size_t>(phx::kWordsMax, entry_words - w0);
    phx::Words w;
    std::memcpy(w.w, reinterpret_cast<const uint64_t*>(e.data()) + w0, cnt * sizeof(uint64_t));
    hip_ok(phx::write_words(table.get() + w0, w, cnt, s), "conv rotation table");
  }

  DeviceBuffer<uint64_t> digits(beta * QlP * n, s);
  phx::KsRotateBatchArgs ba;
  ba.digits = digits.get();
  ba.entries = reinterpret_cast<const phx::KsBatchEntry*>(table.get());
  ba.count = static_cast<uint32_t>(K2);
  ba.qp = ctx.mod_QP().q;
  ba.qp_barrett = ctx.mod_QP().barrett;
  ba.pmod = rt.bigP_mod_q();
  ba.pmod_shoup = rt.bigP_mod_q_shoup();
  ba.ql = static_cast<uint32_t>(Ql);
  ba.qlp = static_cast<uint32_t>(QlP);
  ba.size_q = static_cast<uint32_t>(ctx.size_Q());
  ba.size_p = static_cast<uint32_t>(ctx.size_P());
  ba.beta = static_cast<uint32_t>(beta);
  for (size_t k = 0; k < c.in_ch; ++k) {
    rt.modup(digits.get(), cts[k] + Ql * n, ntt, s);
    ba.ct = cts[k];
    ba.out = rots + k * K2 * ext_words;
    hip_ok(phx::keyswitch_rotate_batch(ba, n, s), "conv rotations");
  }
}

// moddown of the 2 out_ch output polynomials in acc ([out_ch][2][Ql + P][n]) to outs
void conv_moddown(const PhantomContext& ctx, size_t chain_index, const phx::ConvShape& c, uint64_t* acc,
                  uint64_t* const* outs, hipStream_t s) {
  const size_t n = ctx.poly_degree();
  const RnsTool& rt = ctx.get_context_data(chain_index).gpu_rns_tool();
  const size_t Ql = rt.size_Ql(), QlP = Ql + ctx.size_P();
  const size_t ext_words = 2 * QlP * n, ct_words = 2 * Ql * n;
  const phx::NttTables& ntt = ctx.gpu_rns_tables();
  // 8 polynomials per launch set (the fused conversion's batch)
  const bool contiguous = [&] {
    for (size_t h = 1; h < c.out_ch; ++h)
      if (outs[h] != outs[0] + h * ct_words) return false;
    return true;
  }();
  DeviceBuffer<uint64_t> stage;
  if (!contiguous) stage.allocate(c.out_ch * ct_words, s);
  uint64_t* const dst = contiguous ? outs[0] : stage.get();
  constexpr size_t kPer = 4;  // output channels per moddown
  for (size_t h0 = 0; h0 < c.out_ch; h0 += kPer) {
    const size_t g = std::min(kPer, c.out_ch - h0);
    rt.moddown_add(dst + h0 * ct_words, acc + h0 * ext_words, false, ntt, s, 2 * g);
  }
  if (!contiguous)
    for (size_t h = 0; h < c.out_ch; ++h)
      PHX_CHECK(hipMemcpyAsync(outs[h], stage.get() + h * ct_words, ct_words * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
}

}  // namespace

void conv2d_raw(const PhantomContext& ctx, size_t chain_index, const uint64_t* const* cts, const phx::ConvShape& c,
                const double* dev_W, double pt_scale, const uint64_t* const* const* evk, const uint32_t* galois_elts,
                size_t group, uint64_t* const* outs, int* dev_overflow, hipStream_t s) {
  if (!cts || !dev_W || !evk || !galois_elts || !outs) throw std::invalid_argument("null pointer");
  if (!(pt_scale > 0)) throw std::invalid_argument("scale must be positive");
  phx::MacArgs ma = mac_args(ctx, chain_index);  // checks the chain index and the special primes
  const size_t n = ctx.poly_degree();
  (void)conv_shape(n, c.width, c.slotstr, c.kernel, c.in_ch, c.out_ch);
  const RnsTool& rt = ctx.get_context_data(chain_index).gpu_rns_tool();
  const size_t QlP = rt.size_Ql() + ctx.size_P();
  const size_t K2 = static_cast<size_t>(c.kernel) * c.kernel, T = c.in_ch * K2, ns = c.slots();
  check_operands(c, cts, evk, outs);
  if (group == 0) group = conv_group(ctx, chain_index, c);
  group = std::min<size_t>(group, c.out_ch);
  const size_t ext_words = 2 * QlP * n, pt_words = QlP * n;

  DeviceBuffer<uint64_t> rots(T * ext_words, s);
  conv_rotate(ctx, chain_index, cts, c, evk, galois_elts, rots.get(), s);

  // inner sums, `group` output channels per pass
  DeviceBuffer<uint64_t> acc(c.out_ch * ext_words, s), pts(group * T * pt_words, s);
  DeviceBuffer<double> slots(group * T * ns * 2, s);
  ma.in0 = rots.get();
  ma.in_stride = ext_words;
  ma.pt0 = pts.get();
  ma.pt_stride = pt_words;
  ma.out_stride = ext_words;
  ma.T = static_cast<uint32_t>(T);
  for (size_t h0 = 0; h0 < c.out_ch; h0 += group) {
    const size_t g = std::min(group, c.out_ch - h0);
    hip_ok(phx::conv_weight_slots(c, dev_W, h0 * T, g * T, slots.get(), s), "conv weight slots");
    encode_raw(ctx, chain_index, true, reinterpret_cast<const std::complex<double>*>(slots.get()), ns, ns, pt_scale,
               g * T, pts.get(), nullptr, dev_overflow, s);
    ma.out0 = acc.get() + h0 * ext_words;
    ma.O = static_cast<uint32_t>(g);
    hip_ok(phx::ext_mac(ma, n, s), "conv inner sums");
  }
  conv_moddown(ctx, chain_index, c, acc.get(), outs, s);
}

// ---- prepared layers ---------------------------------------------------------------------------

ConvPlanData::~ConvPlanData() {
  if (pts) (void)hipFree(pts);
}

std::unique_ptr<ConvPlanData> conv2d_prepare(const PhantomContext& ctx, size_t chain_index, const phx::ConvShape& c,
                                             const double* dev_W, double pt_scale, int* dev_overflow, hipStream_t s,
                                             const double* out_scale) {
  if (!dev_W) throw std::invalid_argument("null pointer");
  if (!(pt_scale > 0)) throw std::invalid_argument("scale must be positive");
  const phx::MacArgs ma = mac_args(ctx, chain_index);  // checks the chain index and the special primes
  const size_t n = ctx.poly_degree();
  (void)conv_shape(n, c.width, c.slotstr, c.kernel, c.in_ch, c.out_ch);
  const size_t ns = c.slots(), M = 2 * ns, terms = c.terms(), QlP = static_cast<size_t>(ma.Ql) + ma.P;
  if (M < 8) throw std::invalid_argument("conv plan: fewer than 4 slots");
  (void)ctx.sub_ntt_tables(M);  // built (first use) before anything is enqueued
  auto plan = std::make_unique<ConvPlanData>();
  plan->ctx = &ctx;
  plan->chain_index = chain_index;
  plan->shape = c;
  plan->scale = pt_scale;
  plan->sub_degree = M;
  plan->words = terms * QlP * M;
  PHX_CHECK(hipMalloc(&plan->pts, plan->words * sizeof(uint64_t)));
  // slices of terms that bound the slot vectors' scratch (16 MiB)
  const size_t slice = std::max<size_t>(1, (size_t(1) << 20) / ns);
  DeviceBuffer<double> slots(std::min(slice, terms) * ns * 2, s), dscale;
  if (out_scale) {
    for (size_t h = 0; h < c.out_ch; ++h)
      if (!std::isfinite(out_scale[h])) throw std::invalid_argument("conv plan: an output scale is not finite");
    dscale.upload(std::vector<double>(out_scale, out_scale + c.out_ch), s);
  }
  for (size_t t0 = 0; t0 < terms; t0 += slice) {
    const size_t cnt = std::min(slice, terms - t0);
    hip_ok(phx::conv_weight_slots(c, dev_W, t0, cnt, slots.get(), s, out_scale ? dscale.get() : nullptr),
           "conv weight slots");
    encode_sub_raw(ctx, chain_index, true, reinterpret_cast<const std::complex<double>*>(slots.get()), ns, ns, pt_scale,
                   cnt, plan->pts + t0 * QlP * M, dev_overflow, s);
  }
  PHX_CHECK(hipStreamSynchronize(s));  // dev_W is the caller's again, and the plan is complete
  return plan;
}

std::vector<uint64_t> scaled_constant_residues(double value, double scale, const uint64_t* moduli, size_t count) {
  if (!moduli) throw std::invalid_argument("null pointer");
  if (!(scale > 0) || !std::isfinite(scale)) throw std::invalid_argument("scale must be positive and finite");
  const double x = value * scale;
  if (!std::isfinite(x)) throw std::invalid_argument("the scaled constant is not finite");
  int e = 0;
  const double frac = std::frexp(std::fabs(x), &e);  // |x| = frac 2^e, frac in [1/2, 1)
  uint64_t mant;
  int shift = 0;
  if (e > 53) {  // an integer already: its 53 mantissa bits, times 2^(e - 53)
    mant = static_cast<uint64_t>(std::ldexp(frac, 53));
    shift = e - 53;
  } else {  // below 2^53: the nearest integer, halves away from zero
    mant = static_cast<uint64_t>(std::llround(std::fabs(x)));
  }
  std::vector<uint64_t> r(count);
  for (size_t i = 0; i < count; ++i) {
    const uint64_t q = moduli[i];
    if (q == 0) throw std::invalid_argument("zero modulus");
    uint64_t v = mant % q;
    for (int left = shift; left > 0; left -= 60)
      v = arith::mul_mod(v, (uint64_t(1) << std::min(left, 60)) % q, q);
    r[i] = (x < 0 && v) ? q - v : v;
  }
  return r;
}

size_t mac_seed_words(size_t O, size_t Ql) { return O + Ql + O * Ql; }

void mac_seed(const PhantomContext& ctx, size_t chain_index, size_t O, const uint64_t* const* res,
              const uint64_t* res_mult, const uint64_t* bias, uint64_t* table, phx::MacArgs& a, hipStream_t s) {
  if (!res && !bias) return;
  if (res && !res_mult) throw std::invalid_argument("a residual needs its multiplier");
  if (!table) throw std::invalid_argument("null pointer");
  const RnsTool& rt = ctx.get_context_data(chain_index).gpu_rns_tool();
  const size_t Ql = rt.size_Ql();
  const std::vector<uint64_t>& pm = rt.bigP_mod_q_host();
  const auto& mods = ctx.get_context_data(chain_index).moduli();
  // [O] residual pointers, [Ql] (m P) mod q_l, [O][Ql] (B_o P) mod q_l
  std::vector<uint64_t> host(mac_seed_words(O, Ql), 0);
  if (res) {
    for (size_t o = 0; o < O; ++o) host[o] = reinterpret_cast<uint64_t>(res[o]);
    for (size_t l = 0; l < Ql; ++l) host[O + l] = arith::mul_mod(res_mult[l] % mods[l], pm[l], mods[l]);
  }
  if (bias)
    for (size_t o = 0; o < O; ++o)
      for (size_t l = 0; l < Ql; ++l)
        host[O + Ql + o * Ql + l] = arith::mul_mod(bias[o * Ql + l] % mods[l], pm[l], mods[l]);
  for (size_t w0 = 0; w0 < host.size(); w0 += phx::kWordsMax) {
    const size_t cnt = std::min<size_t>(phx::kWordsMax, host.size() - w0);
    phx::Words w;
    std::memcpy(w.w, host.data() + w0, cnt * sizeof(uint64_t));
    hip_ok(phx::write_words(table + w0, w, cnt, s), "inner-sum seed table");
  }
  static_assert(sizeof(uint64_t) == sizeof(const uint64_t*), "pointers are written as words");
  if (res) {
    a.seed_res = reinterpret_cast<const uint64_t* const*>(table);
    a.seed_mult = table + O;
  }
  if (bias) a.seed_bias = table + O + Ql;
}

void conv2d_apply(const PhantomContext& ctx, const ConvPlanData& plan, const uint64_t* const* cts,
                  const uint64_t* const* const* evk, const uint32_t* galois_elts, uint64_t* const* outs,
                  hipStream_t s, const uint64_t* const* res, const uint64_t* res_mult, const uint64_t* bias) {
  if (!cts || !evk || !galois_elts || !outs) throw std::invalid_argument("null pointer");
  if (res && !res_mult) throw std::invalid_argument("conv plan: a residual needs its multiplier");
  if (plan.ctx != &ctx) throw std::invalid_argument("conv plan: prepared for another context");
  const phx::ConvShape& c = plan.shape;
  phx::MacArgs ma = mac_args(ctx, plan.chain_index);
  const size_t n = ctx.poly_degree();
  const size_t QlP = static_cast<size_t>(ma.Ql) + ma.P;
  const size_t K2 = static_cast<size_t>(c.kernel) * c.kernel, T = c.in_ch * K2;
  check_operands(c, cts, evk, outs);
  const size_t ext_words = 2 * QlP * n;

  DeviceBuffer<uint64_t> rots(T * ext_words, s), acc(c.out_ch * ext_words, s);
  conv_rotate(ctx, plan.chain_index, cts, c, evk, galois_elts, rots.get(), s);
  ma.in0 = rots.get();
  ma.in_stride = ext_words;
  ma.pt0 = plan.pts;
  ma.pt_stride = QlP * plan.sub_degree;
  ma.out0 = acc.get();
  ma.out_stride = ext_words;
  ma.T = static_cast<uint32_t>(T);
  ma.O = c.out_ch;
  DeviceBuffer<uint64_t> seed;
  if (res || bias) {
    seed.allocate(mac_seed_words(c.out_ch, ma.Ql), s);
    mac_seed(ctx, plan.chain_index, c.out_ch, res, res_mult, bias, seed.get(), ma, s);
  }
  hip_ok(phx::ext_mac_sub(ma, n, plan.sub_degree, s), "conv inner sums");
  conv_moddown(ctx, plan.chain_index, c, acc.get(), outs, s);
}

}  // namespace phantom
