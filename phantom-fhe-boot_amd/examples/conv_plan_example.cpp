// conv_plan_example — prepared convolution layers (DNN::PrepareConv / Conv(plan), host/dnn.h)
// against the existing DNN::Conv(weight), both through the C++ façade on the same ciphertexts and
// keys.  A plan keeps the layer's out_ch in_ch K^2 weight plaintexts on the device in the compact
// subring form (host/conv2d.h), so an inference runs no encode.
//
// usage: conv_plan_example check
//          N = 2^12, CoeffModulus::Create(N, {60, 50, 50, 50, 50, 60, 60}), two special primes, scale
//          2^50; inputs and weights uniform in [-1, 1] from a fixed seed.  Case 1: width 8, 3 -> 2
//          channels, K = 3, slotstr 0, stride 1.  Case 2: the same shape packed with slotstr 1, stride 2.
//          Per case one JSON line: the maximum absolute error against the cleartext convolution of
//          DNN::Conv(weight) (`hoisted`), of Conv(plan), and of the same plan applied to a second
//          encrypted input (`reuse`, beside DNN::Conv(weight) on that input), both results' metadata
//          and the plan's bytes.  After case 1 a `conv_plan_chain` line: Conv(plan) -> BatchNorm -> Add
//          -> Conv(plan prepared one level down) against the cleartext, within 1e-3.  A last `done`
//          line; exit status 0 iff every line is ok.
//        conv_plan_example time <log_n> <chain> <width> <in_ch> <out_ch> <K> [reps] [plan]
//          log_n = 16 takes the bootstrap's key chain ({60, 29 x 59} + 10 x 60), else the chain of
//          `check`; the input tensor is brought to chain index <chain>.  The prepare time once; then
//          DNN::Conv(weight) and Conv(plan) alternate in one process after one warm-up each, every
//          timed window ending in a stream synchronise; then the two inner-sum kernels alone with
//          events on constant operands: ext_mac_sub on the layer's shape (all output channels) and
//          ext_mac on one pass of DNN::Conv(weight).  One JSON line with the medians and ranges, the
//          plan's bytes and the kernels' shape-derived bytes.  With a trailing `plan` only the prepared
//          layer runs (a kernel trace of it alone; the other fields are 0).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "../csrc/conv.h"
#include "../host/ckks_eval.h"
#include "../host/conv2d.h"
#include "../host/dnn.h"
#include "../host/encoder.h"
#include "../host/evaluate.h"
#include "../host/keys.h"
#include "../host/modulus.h"

using namespace phantom;
using namespace phantom::arith;

static DNN::Tensor3 random_image(size_t width, size_t ch, std::mt19937_64& rng) {
  std::uniform_real_distribution<double> d(-1.0, 1.0);
  DNN::Tensor3 x(width, std::vector<std::vector<double>>(width, std::vector<double>(ch)));
  for (auto& row : x)
    for (auto& px : row)
      for (double& v : px) v = d(rng);
  return x;
}

static DNN::Weight4 random_weight(size_t K, size_t in_ch, size_t out_ch, std::mt19937_64& rng) {
  std::uniform_real_distribution<double> d(-1.0, 1.0);
  DNN::Weight4 w(K, std::vector<std::vector<std::vector<double>>>(
                        K, std::vector<std::vector<double>>(in_ch, std::vector<double>(out_ch))));
  for (auto& a : w)
    for (auto& b : a)
      for (auto& k : b)
        for (double& v : k) v = d(rng);
  return w;
}

// zero-padded "same" cross-correlation, then every stride-th pixel
static DNN::Tensor3 clear_conv(const DNN::Tensor3& x, const DNN::Weight4& w, size_t stride) {
  const long width = static_cast<long>(x.size()), K = static_cast<long>(w.size()), half = K / 2;
  const size_t in_ch = w[0][0].size(), out_ch = w[0][0][0].size(), ow = x.size() / stride;
  DNN::Tensor3 y(ow, std::vector<std::vector<double>>(ow, std::vector<double>(out_ch, 0.0)));
  for (size_t i = 0; i < ow; ++i)
    for (size_t j = 0; j < ow; ++j)
      for (size_t h = 0; h < out_ch; ++h) {
        double s = 0;
        for (long a = 0; a < K; ++a)
          for (long b = 0; b < K; ++b) {
            const long r = static_cast<long>(i * stride) + a - half, c = static_cast<long>(j * stride) + b - half;
            if (r < 0 || r >= width || c < 0 || c >= width) continue;
            for (size_t k = 0; k < in_ch; ++k) s += w[a][b][k][h] * x[r][c][k];
          }
        y[i][j][h] = s;
      }
  return y;
}

static double max_error(const DNN::Tensor3& a, const DNN::Tensor3& b) {
  if (a.size() != b.size()) return INFINITY;
  double e = 0;
  for (size_t i = 0; i < a.size(); ++i)
    for (size_t j = 0; j < a[i].size(); ++j)
      for (size_t k = 0; k < a[i][j].size(); ++k) e = std::max(e, std::fabs(a[i][j][k] - b[i][j][k]));
  return e;
}

static std::string metadata(const TensorCT& t) {
  const PhantomCiphertext& c = t.ctks_.at(0);
  char buf[256];
  std::snprintf(buf, sizeof buf,
                "{\"width\": %zu, \"slotstr\": %zu, \"num_ch\": %zu, \"chain_index\": %zu, \"size\": %zu, "
                "\"limbs\": %zu, \"degree\": %zu, \"log2_scale\": %.6f, \"ntt\": %s}",
                t.width_, t.slotstr_, t.num_ch_, c.chain_index(), c.size(), c.coeff_modulus_size(), c.GetNoiseScaleDeg(),
                std::log2(c.scale()), c.is_ntt_form() ? "true" : "false");
  return buf;
}

static bool same_metadata(const TensorCT& a, const TensorCT& b) {
  if (a.width_ != b.width_ || a.slotstr_ != b.slotstr_ || a.num_ch_ != b.num_ch_ || a.ctks_.size() != b.ctks_.size())
    return false;
  for (size_t h = 0; h < a.ctks_.size(); ++h) {
    const PhantomCiphertext &x = a.ctks_[h], &y = b.ctks_[h];
    if (x.chain_index() != y.chain_index() || x.size() != y.size() || x.scale() != y.scale() ||
        x.coeff_modulus_size() != y.coeff_modulus_size() || x.GetNoiseScaleDeg() != y.GetNoiseScaleDeg() ||
        x.is_ntt_form() != y.is_ntt_form() || x.correction_factor() != y.correction_factor())
      return false;
  }
  return true;
}

static EncryptionParameters make_parms(int log_n) {
  const size_t n = size_t(1) << log_n;
  EncryptionParameters parms(scheme_type::ckks);
  parms.set_poly_modulus_degree(n);
  std::vector<int> bits = {60, 50, 50, 50, 50, 60, 60};
  size_t special = 2;
  if (log_n == 16) {
    bits.assign(1, 60);
    bits.insert(bits.end(), 29, 59);
    bits.insert(bits.end(), 10, 60);
    special = 10;
  }
  parms.set_special_modulus_size(special);
  parms.set_coeff_modulus(CoeffModulus::Create(n, bits));
  return parms;
}

static bool check_case(const char* name, size_t width, size_t slotstr, size_t in_ch, size_t out_ch, size_t K,
                       size_t stride, uint64_t seed) {
  const int log_n = 12;
  PhantomContext ctx(make_parms(log_n));
  PhantomCKKSEncoder encoder(ctx);
  const double scale = std::ldexp(1.0, 50);
  PhantomSecretKey sk(ctx);
  PhantomPublicKey pk = sk.gen_publickey(ctx);
  std::mt19937_64 rng(seed);
  const DNN::Tensor3 image = random_image(width, in_ch, rng), image2 = random_image(width, in_ch, rng);
  const DNN::Weight4 weight = random_weight(K, in_ch, out_ch, rng);

  DNN model(static_cast<size_t>(scale), encoder, ctx);
  model.ComputeRotationIndices(sk, width, K, slotstr);
  TensorCT input = model.EncTensor(image, pk, slotstr), input2 = model.EncTensor(image2, pk, slotstr);
  input.ctks_[0].PreComputeScale(ctx, scale);
  model.setScalingFactors(input.ctks_[0].getScalingFactorsReal(), input.ctks_[0].getScalingFactorsRealBig());

  DNN::ConvPlan plan = model.PrepareConv(weight, width, slotstr, input.ctks_[0].chain_index());
  const DNN::Tensor3 want = clear_conv(image, weight, stride), want2 = clear_conv(image2, weight, stride);
  TensorCT hoisted = model.Conv(input, weight, stride);
  TensorCT planned = model.Conv(input, plan, stride);
  TensorCT hoisted2 = model.Conv(input2, weight, stride);
  TensorCT planned2 = model.Conv(input2, plan, stride);  // the plan reused on a second input
  const double eh = max_error(model.DecTensor(hoisted, sk), want), ep = max_error(model.DecTensor(planned, sk), want);
  const double eh2 = max_error(model.DecTensor(hoisted2, sk), want2),
               ep2 = max_error(model.DecTensor(planned2, sk), want2);
  const bool meta = same_metadata(hoisted, planned) && same_metadata(hoisted2, planned2);
  const size_t QlP = ctx.get_context_data(plan.chain_index()).gpu_rns_tool().size_Ql() + ctx.size_P();
  const size_t want_bytes = 8 * out_ch * in_ch * K * K * QlP * 2 * ((width << slotstr) * (width << slotstr));
  // the existing layer within the bound of ckks_example (1e-3), else the comparison says nothing; the
  // prepared layer at most twice its error (the two differ in how the weight plaintexts are rounded)
  const bool ok = meta && eh < 1e-3 && ep <= 2 * eh && eh2 < 1e-3 && ep2 <= 2 * eh2 && plan.bytes() == want_bytes;
  std::printf("{\"check\": \"%s\", \"log_n\": %d, \"width\": %zu, \"slotstr\": %zu, \"in_ch\": %zu, \"out_ch\": %zu, "
              "\"kernel\": %zu, \"stride\": %zu, \"hoisted_max_error\": %.6e, \"plan_max_error\": %.6e, "
              "\"reuse_hoisted_max_error\": %.6e, \"reuse_plan_max_error\": %.6e, \"metadata_equal\": %s, "
              "\"plan_bytes\": %zu, \"plan_chain_index\": %zu, \"hoisted\": %s, \"plan\": %s, \"ok\": %s}\n",
              name, log_n, width, slotstr, in_ch, out_ch, K, stride, eh, ep, eh2, ep2, meta ? "true" : "false",
              plan.bytes(), plan.chain_index(), metadata(hoisted).c_str(), metadata(planned).c_str(),
              ok ? "true" : "false");
  if (stride != 1) return ok;

  // two prepared layers chained, a degree-2 tensor into every step: Conv(plan) -> BatchNorm -> Add ->
  // Conv(plan2), plan2 prepared at the level the second layer's input has after its rescale
  std::uniform_real_distribution<double> unit(-1.0, 1.0), pos(0.5, 1.5);
  std::vector<double> gamma(out_ch), beta(out_ch), mean(out_ch), var(out_ch);
  for (size_t c = 0; c < out_ch; ++c) {
    gamma[c] = pos(rng);
    beta[c] = unit(rng);
    mean[c] = unit(rng);
    var[c] = pos(rng);
  }
  const DNN::Weight4 weight2 = random_weight(K, out_ch, out_ch, rng);
  TensorCT bn = model.BatchNorm(planned, gamma, beta, mean, var);
  TensorCT sum = model.Add(bn, bn);
  const PhantomCiphertext& s0 = sum.ctks_[0];
  const size_t chain2 = s0.chain_index() + (s0.GetNoiseScaleDeg() == 2 ? 1 : 0);
  DNN::ConvPlan plan2 = model.PrepareConv(weight2, sum.width_, sum.slotstr_, chain2);
  TensorCT second = model.Conv(sum, plan2, 1);
  DNN::Tensor3 mid = want;
  for (auto& row : mid)
    for (auto& px : row)
      for (size_t c = 0; c < out_ch; ++c) {
        const double a = gamma[c] / std::sqrt(var[c] + 1e-5);
        px[c] = 2 * (a * px[c] + beta[c] - a * mean[c]);
      }
  const double e2 = max_error(model.DecTensor(second, sk), clear_conv(mid, weight2, 1));
  // a plan of another level is refused
  bool refused = false;
  try {
    (void)model.Conv(sum, plan, 1);
  } catch (const std::invalid_argument&) {
    refused = true;
  }
  const bool ok2 = e2 < 1e-3 && refused && second.ctks_[0].chain_index() == chain2 && chain2 > plan.chain_index();
  std::printf("{\"check\": \"conv_plan_chain\", \"log_n\": %d, \"max_error\": %.6e, \"first_chain_index\": %zu, "
              "\"second_chain_index\": %zu, \"mismatched_plan_refused\": %s, \"batchnorm\": %s, \"second\": %s, \"ok\": %s}\n",
              log_n, e2, plan.chain_index(), plan2.chain_index(), refused ? "true" : "false", metadata(bn).c_str(),
              metadata(second).c_str(), ok2 ? "true" : "false");
  return ok && ok2;
}

static int run_check() {
  bool all = check_case("conv_plan", 8, 0, 3, 2, 3, 1, 0xC0417);
  all = check_case("conv_plan_stride2", 8, 1, 3, 2, 3, 2, 0xC0418) && all;
  std::printf("{\"done\": \"conv_plan_example check\", \"ok\": %s}\n", all ? "true" : "false");
  return all ? 0 : 1;
}

struct Stat {
  double median, min, max;
};
static Stat stat(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return {v[v.size() / 2], v.front(), v.back()};
}

// `reps` timed launches after one warm-up, by events
template <class F>
static Stat time_kernel(hipStream_t s, int reps, F launch) {
  hipEvent_t e0, e1;
  PHX_CHECK(hipEventCreate(&e0));
  PHX_CHECK(hipEventCreate(&e1));
  std::vector<double> t;
  for (int r = 0; r < reps + 1; ++r) {
    PHX_CHECK(hipEventRecord(e0, s));
    PHX_CHECK(launch());
    PHX_CHECK(hipEventRecord(e1, s));
    PHX_CHECK(hipEventSynchronize(e1));
    float ms = 0;
    PHX_CHECK(hipEventElapsedTime(&ms, e0, e1));
    if (r) t.push_back(ms);
  }
  PHX_CHECK(hipEventDestroy(e0));
  PHX_CHECK(hipEventDestroy(e1));
  return stat(t);
}

static int run_time(int log_n, size_t chain, size_t width, size_t in_ch, size_t out_ch, size_t K, int reps,
                    bool only_plan) {
  PhantomContext ctx(make_parms(log_n));
  if (chain < 1 || chain >= ctx.total_parm_size() || reps < 1) throw std::invalid_argument("bad chain or reps");
  PhantomCKKSEncoder encoder(ctx);
  hipStream_t s = ctx.stream();
  const double scale = std::ldexp(1.0, log_n == 16 ? 59 : 50);
  PhantomSecretKey sk(ctx);
  PhantomPublicKey pk = sk.gen_publickey(ctx);
  std::mt19937_64 rng(7);
  const DNN::Tensor3 image = random_image(width, in_ch, rng);
  const DNN::Weight4 weight = random_weight(K, in_ch, out_ch, rng);
  DNN model(static_cast<size_t>(scale), encoder, ctx);
  model.ComputeRotationIndices(sk, width, K, 0);
  TensorCT input = model.EncTensor(image, pk);
  input.ctks_[0].PreComputeScale(ctx, scale);
  model.setScalingFactors(input.ctks_[0].getScalingFactorsReal(), input.ctks_[0].getScalingFactorsRealBig());
  // the layer's level: drop limbs (the values and the scale stay)
  if (chain > 1)
    for (PhantomCiphertext& c : input.ctks_) ModSwitchLevelInPlace(ctx, c, chain - 1);

  using clock = std::chrono::steady_clock;
  auto ms_since = [](clock::time_point t0) { return std::chrono::duration<double, std::milli>(clock::now() - t0).count(); };
  PHX_CHECK(hipStreamSynchronize(s));
  const auto tp = clock::now();
  DNN::ConvPlan plan = model.PrepareConv(weight, width, 0, chain);  // waits for the stream
  const double prepare_ms = ms_since(tp);

  TensorCT hoisted, planned;
  auto run_hoisted = [&] {
    PHX_CHECK(hipStreamSynchronize(s));
    const auto t0 = clock::now();
    hoisted = model.Conv(input, weight, 1);
    PHX_CHECK(hipStreamSynchronize(s));
    return ms_since(t0);
  };
  auto run_plan = [&] {
    PHX_CHECK(hipStreamSynchronize(s));
    const auto t0 = clock::now();
    planned = model.Conv(input, plan, 1);
    PHX_CHECK(hipStreamSynchronize(s));
    return ms_since(t0);
  };
  if (!only_plan) run_hoisted();  // warm: code objects, pool, workspace, encoder tables
  run_plan();
  std::vector<double> th, tq;
  for (int r = 0; r < reps; ++r) {
    th.push_back(only_plan ? 0.0 : run_hoisted());
    tq.push_back(run_plan());
  }
  const DNN::Tensor3 want = clear_conv(image, weight, 1);
  const double eh = only_plan ? 0.0 : max_error(model.DecTensor(hoisted, sk), want);
  const double ep = max_error(model.DecTensor(planned, sk), want);

  // the inner sums alone on constant operands (words below 2^59; the time does not depend on the
  // values): ext_mac_sub over all output channels, ext_mac over one pass of DNN::Conv(weight)
  const phx::ConvShape shape = conv_shape(ctx.poly_degree(), width, 0, K, in_ch, out_ch);
  const size_t n = ctx.poly_degree(), Ql = ctx.get_context_data(chain).gpu_rns_tool().size_Ql(), QlP = Ql + ctx.size_P();
  const size_t T = in_ch * K * K, group = conv_group(ctx, chain, shape), M = 2 * shape.slots();
  const size_t ext_words = 2 * QlP * n, pt_words = QlP * n;
  Stat msub{0, 0, 0}, mfull{0, 0, 0};
  if (!only_plan) {
    DeviceBuffer<uint64_t> ins(T * ext_words, s), outs(out_ch * ext_words, s);
    PHX_CHECK(hipMemsetAsync(ins.get(), 0x05, T * ext_words * sizeof(uint64_t), s));
    phx::MacArgs a = mac_args(ctx, chain);
    a.in0 = ins.get();
    a.in_stride = ext_words;
    a.out0 = outs.get();
    a.out_stride = ext_words;
    a.T = static_cast<uint32_t>(T);
    {
      DeviceBuffer<uint64_t> pts(out_ch * T * QlP * M, s);
      PHX_CHECK(hipMemsetAsync(pts.get(), 0x03, out_ch * T * QlP * M * sizeof(uint64_t), s));
      a.pt0 = pts.get();
      a.pt_stride = QlP * M;
      a.O = static_cast<uint32_t>(out_ch);
      msub = time_kernel(s, reps, [&] { return phx::ext_mac_sub(a, n, M, s); });
    }
    {
      DeviceBuffer<uint64_t> pts(group * T * pt_words, s);
      PHX_CHECK(hipMemsetAsync(pts.get(), 0x03, group * T * pt_words * sizeof(uint64_t), s));
      a.pt0 = pts.get();
      a.pt_stride = pt_words;
      a.O = static_cast<uint32_t>(group);
      mfull = time_kernel(s, reps, [&] { return phx::ext_mac(a, n, s); });
    }
  }
  // bytes a launch must move.  ext_mac_sub: the inputs once per 16 outputs, the compact plaintexts
  // once, the outputs written once; ext_mac: the inputs once per 8 outputs, the plaintexts once
  const double rows = static_cast<double>((out_ch + phx::kSubWaves - 1) / phx::kSubWaves);
  const double sub_bytes = 8.0 * (rows * T * 2.0 * QlP * n + static_cast<double>(out_ch) * T * QlP * M + out_ch * 2.0 * QlP * n);
  const double full_bytes =
      8.0 * n * (static_cast<double>(group) * T * QlP + ((group + 7) / 8) * T * 2.0 * QlP + group * 2.0 * QlP);
  const double products = 2.0 * out_ch * T * QlP * n;  // 64 x 64-bit products, four 32-bit multiplies each
  const Stat h = stat(th), q = stat(tq);
  std::printf("{\"time\": \"conv_plan\", \"log_n\": %d, \"chain\": %zu, \"Ql\": %zu, \"QlP\": %zu, \"width\": %zu, "
              "\"in_ch\": %zu, \"out_ch\": %zu, \"kernel\": %zu, \"reps\": %d, \"sub_degree\": %zu, "
              "\"prepare_ms\": %.3f, \"plan_bytes\": %zu, \"full_size_plaintext_bytes\": %.0f, "
              "\"hoisted_ms\": {\"median\": %.3f, \"min\": %.3f, \"max\": %.3f}, "
              "\"plan_ms\": {\"median\": %.3f, \"min\": %.3f, \"max\": %.3f}, \"speedup\": %.2f, "
              "\"hoisted_max_error\": %.3e, \"plan_max_error\": %.3e, "
              "\"ext_mac_sub\": {\"terms\": %zu, \"outputs\": %zu, \"ms\": {\"median\": %.3f, \"min\": %.3f, \"max\": %.3f}, "
              "\"bytes\": %.0f, \"tb_per_s\": %.3f, \"products\": %.0f, \"tera_products_per_s\": %.3f}, "
              "\"ext_mac\": {\"terms\": %zu, \"outputs\": %zu, \"ms\": {\"median\": %.3f, \"min\": %.3f, \"max\": %.3f}, "
              "\"bytes\": %.0f, \"tb_per_s\": %.3f}}\n",
              log_n, chain, Ql, QlP, width, in_ch, out_ch, K, reps, M, prepare_ms, plan.bytes(),
              8.0 * n * out_ch * T * QlP, h.median, h.min, h.max, q.median, q.min, q.max,
              q.median > 0 ? h.median / q.median : 0.0, eh, ep, T, out_ch, msub.median, msub.min, msub.max, sub_bytes,
              msub.median > 0 ? sub_bytes / (msub.median * 1e-3) / 1e12 : 0.0, products,
              msub.median > 0 ? products / (msub.median * 1e-3) / 1e12 : 0.0, T, group, mfull.median, mfull.min,
              mfull.max, full_bytes, mfull.median > 0 ? full_bytes / (mfull.median * 1e-3) / 1e12 : 0.0);
  std::printf("{\"done\": \"conv_plan_example time\", \"ok\": true}\n");
  return 0;
}

int main(int argc, char** argv) {
  try {
    if (argc >= 2 && !std::strcmp(argv[1], "check")) return run_check();
    if (argc >= 8 && !std::strcmp(argv[1], "time"))
      return run_time(std::atoi(argv[2]), std::strtoull(argv[3], nullptr, 10), std::strtoull(argv[4], nullptr, 10),
                      std::strtoull(argv[5], nullptr, 10), std::strtoull(argv[6], nullptr, 10),
                      std::strtoull(argv[7], nullptr, 10), argc >= 9 ? std::atoi(argv[8]) : 3,
                      argc >= 10 && !std::strcmp(argv[9], "plan"));
    std::fprintf(stderr, "usage: conv_plan_example check | time <log_n> <chain> <width> <in_ch> <out_ch> <K> [reps] [plan]\n");
    return 2;
  } catch (const std::exception& e) {
    std::printf("{\"error\": \"%s\", \"ok\": false}\n", e.what());
    return 1;
  }
}
