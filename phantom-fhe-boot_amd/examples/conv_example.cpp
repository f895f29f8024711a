// conv_example — the hoisted encrypted convolution (DNN::Conv, host/dnn.h) against the per-term
// sequence it replaces, both through the C++ façade on the same ciphertexts and keys.
//
// The baseline is the layer as the reference runs it (src/dnn.cu:82-150): for every output channel,
// input channel and tap, one masked weight vector encoded on the host (encode_sparse), one
// EvalRotateFused of the input channel, one EvalMultAutoInplace and one EvalAddAutoInplace.
//
// usage: conv_example check
//          N = 2^12, CoeffModulus::Create(N, {60, 50, 50, 50, 50, 60, 60}), two special primes, scale
//          2^50; inputs and weights uniform in [-1, 1] from a fixed seed.  Case 1: width 8, 3 -> 2
//          channels, K = 3, stride 1.  Case 2: the same shape packed with slotstr 1, stride 2.  One JSON
//          line per case with the maximum absolute error of DNN::Conv and of the baseline against the
//          cleartext convolution, the EncTensor -> DecTensor round-trip error and both results'
//          metadata.  After case 1 a `conv_chain` line: Conv -> BatchNorm -> Add -> Conv (2 -> 2
//          channels) against the cleartext, within 1e-3.  A last `done` line; exit status 0 iff every
//          line is ok.
//        conv_example time <log_n> <chain> <width> <in_ch> <out_ch> <K> [reps] [hoisted]
//          log_n = 16 takes the bootstrap's key chain ({60, 29 x 59} + 10 x 60), else the chain of
//          `check`; the input tensor is brought to chain index <chain>.  The hoisted layer and the
//          baseline alternate in one process after a warm-up, every timed window ending in a stream
//          synchronise; then the inner-sum kernel alone on the layer's shape.  One JSON line with the
//          medians and ranges, the operation counts and the shape-derived bytes.  With a trailing
//          `hoisted` only the hoisted layer runs (a kernel trace of it alone; the other fields are 0).
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

// the per-term layer through the façade: encode_sparse -> EvalRotateFused -> EvalMultAutoInplace ->
// EvalAddAutoInplace for every (output channel, input channel, tap)
static TensorCT baseline_conv(DNN& model, const PhantomContext& ctx, const TensorCT& in, const DNN::Weight4& w,
                              size_t stride) {
  const size_t K = w.size(), in_ch = w[0][0].size(), out_ch = w[0][0][0].size();
  const size_t pw = size_t(1) << in.slotstr_, lg = in.width_ * pw, width = in.width_;
  const std::vector<int> rots = conv_rotations(width, in.slotstr_, K);
  const auto& sf = model.scalingFactorsReal();
  const auto& sfBig = model.scalingFactorsRealBig();
  TensorCT out;
  out.ctks_.resize(out_ch);
  for (size_t h = 0; h < out_ch; ++h) {
    bool first = true;
    for (size_t k = 0; k < in_ch; ++k)
      for (size_t a = 0; a < K; ++a)
        for (size_t b = 0; b < K; ++b) {
          std::vector<double> mask(lg * lg, 0.0);
          for (size_t r = 0; r < width; ++r)
            for (size_t c = 0; c < width; ++c)
              if (r + a >= K / 2 && r + a < K / 2 + width && c + b >= K / 2 && c + b < K / 2 + width)
                mask[(r * lg + c) * pw] = w[a][b][k][h];
          PhantomPlaintext pt = model.PlainTextEncode(mask, in.ctks_[k].chain_index());
          PhantomCiphertext term;
          EvalRotateFused(ctx, model.galois_keys(), in.ctks_[k], term, rots[a * K + b]);
          EvalMultAutoInplace(ctx, term, pt, sf, sfBig);
          if (first) out.ctks_[h] = std::move(term);
          else EvalAddAutoInplace(ctx, out.ctks_[h], term, sf, sfBig);
          first = false;
        }
  }
  out.width_ = in.width_ / stride;
  out.num_ch_ = out_ch;
  out.slotstr_ = stride == 2 ? in.slotstr_ + 1 : in.slotstr_;
  return out;
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
  const DNN::Tensor3 image = random_image(width, in_ch, rng);
  const DNN::Weight4 weight = random_weight(K, in_ch, out_ch, rng);

  DNN model(static_cast<size_t>(scale), encoder, ctx);
  model.ComputeRotationIndices(sk, width, K, slotstr);
  TensorCT input = model.EncTensor(image, pk, slotstr);
  input.ctks_[0].PreComputeScale(ctx, scale);
  model.setScalingFactors(input.ctks_[0].getScalingFactorsReal(), input.ctks_[0].getScalingFactorsRealBig());
  const double roundtrip = max_error(model.DecTensor(input, sk), image);

  const DNN::Tensor3 want = clear_conv(image, weight, stride);
  TensorCT hoisted = model.Conv(input, weight, stride);
  TensorCT base = baseline_conv(model, ctx, input, weight, stride);
  const double eh = max_error(model.DecTensor(hoisted, sk), want), eb = max_error(model.DecTensor(base, sk), want);
  const bool meta = same_metadata(hoisted, base);
  // the baseline within the bound of ckks_example (1e-3), else the comparison says nothing; the
  // hoisted layer at most twice the baseline's error (it rounds once per output, not once per term)
  const bool ok = meta && eb < 1e-3 && eh <= 2 * eb && roundtrip < 1e-3;
  std::printf("{\"check\": \"%s\", \"log_n\": %d, \"width\": %zu, \"slotstr\": %zu, \"in_ch\": %zu, \"out_ch\": %zu, "
              "\"kernel\": %zu, \"stride\": %zu, \"hoisted_max_error\": %.6e, \"baseline_max_error\": %.6e, "
              "\"roundtrip_max_error\": %.6e, \"metadata_equal\": %s, \"hoisted\": %s, \"baseline\": %s, \"ok\": %s}\n",
              name, log_n, width, slotstr, in_ch, out_ch, K, stride, eh, eb, roundtrip, meta ? "true" : "false",
              metadata(hoisted).c_str(), metadata(base).c_str(), ok ? "true" : "false");
  if (stride != 1) return ok;

  // two layers chained, a degree-2 tensor into every step: Conv -> BatchNorm -> Add -> Conv
  std::uniform_real_distribution<double> unit(-1.0, 1.0), pos(0.5, 1.5);
  std::vector<double> gamma(out_ch), beta(out_ch), mean(out_ch), var(out_ch);
  for (size_t c = 0; c < out_ch; ++c) {
    gamma[c] = pos(rng);
    beta[c] = unit(rng);
    mean[c] = unit(rng);
    var[c] = pos(rng);
  }
  const DNN::Weight4 weight2 = random_weight(K, out_ch, out_ch, rng);
  TensorCT bn = model.BatchNorm(hoisted, gamma, beta, mean, var);
  TensorCT second = model.Conv(model.Add(bn, bn), weight2, 1);
  DNN::Tensor3 mid = want;
  for (auto& row : mid)
    for (auto& px : row)
      for (size_t c = 0; c < out_ch; ++c) {
        const double a = gamma[c] / std::sqrt(var[c] + 1e-5);
        px[c] = 2 * (a * px[c] + beta[c] - a * mean[c]);
      }
  const double e2 = max_error(model.DecTensor(second, sk), clear_conv(mid, weight2, 1));
  const bool ok2 = e2 < 1e-3;
  std::printf("{\"check\": \"conv_chain\", \"log_n\": %d, \"max_error\": %.6e, \"batchnorm\": %s, \"second\": %s, "
              "\"ok\": %s}\n",
              log_n, e2, metadata(bn).c_str(), metadata(second).c_str(), ok2 ? "true" : "false");
  return ok && ok2;
}

static int run_check() {
  bool all = check_case("conv", 8, 0, 3, 2, 3, 1, 0xC0417);
  all = check_case("conv_stride2", 8, 1, 3, 2, 3, 2, 0xC0418) && all;
  std::printf("{\"done\": \"conv_example check\", \"ok\": %s}\n", all ? "true" : "false");
  return all ? 0 : 1;
}

struct Stat {
  double median, min, max;
};
static Stat stat(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return {v[v.size() / 2], v.front(), v.back()};
}

static int run_time(int log_n, size_t chain, size_t width, size_t in_ch, size_t out_ch, size_t K, int reps,
                    bool only_hoisted) {
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
  TensorCT hoisted, base;
  auto run_hoisted = [&] {
    PHX_CHECK(hipStreamSynchronize(s));
    const auto t0 = clock::now();
    hoisted = model.Conv(input, weight, 1);
    PHX_CHECK(hipStreamSynchronize(s));
    return ms_since(t0);
  };
  auto run_base = [&] {
    PHX_CHECK(hipStreamSynchronize(s));
    const auto t0 = clock::now();
    base = baseline_conv(model, ctx, input, weight, 1);
    PHX_CHECK(hipStreamSynchronize(s));
    return ms_since(t0);
  };
  run_hoisted();  // warm: code objects, pool, workspace, encoder tables
  if (!only_hoisted) run_base();
  std::vector<double> th, tb;
  for (int r = 0; r < reps; ++r) {
    th.push_back(run_hoisted());
    tb.push_back(only_hoisted ? 0.0 : run_base());
  }
  const DNN::Tensor3 want = clear_conv(image, weight, 1);
  const double eh = max_error(model.DecTensor(hoisted, sk), want);
  const double eb = only_hoisted ? 0.0 : max_error(model.DecTensor(base, sk), want);

  // the inner sums alone, on the layer's shape (one pass of `group` output channels)
  const phx::ConvShape shape = conv_shape(ctx.poly_degree(), width, 0, K, in_ch, out_ch);
  const size_t n = ctx.poly_degree(), Ql = ctx.get_context_data(chain).gpu_rns_tool().size_Ql(), QlP = Ql + ctx.size_P();
  const size_t T = in_ch * K * K, group = conv_group(ctx, chain, shape), beta = ctx.get_context_data(chain).gpu_rns_tool().beta();
  const size_t ext_words = 2 * QlP * n, pt_words = QlP * n;
  std::vector<double> tm;
  if (only_hoisted) {
    tm.push_back(0.0);
  } else {
    DeviceBuffer<uint64_t> ins(T * ext_words, s), pts(group * T * pt_words, s), outs(group * ext_words, s);
    // operands: words below 2^59 (the kernel's time does not depend on their values)
    PHX_CHECK(hipMemsetAsync(ins.get(), 0x05, T * ext_words * sizeof(uint64_t), s));
    PHX_CHECK(hipMemsetAsync(pts.get(), 0x03, group * T * pt_words * sizeof(uint64_t), s));
    phx::MacArgs a = mac_args(ctx, chain);
    a.in0 = ins.get();
    a.in_stride = ext_words;
    a.pt0 = pts.get();
    a.pt_stride = pt_words;
    a.out0 = outs.get();
    a.out_stride = ext_words;
    a.T = static_cast<uint32_t>(T);
    a.O = static_cast<uint32_t>(group);
    hipEvent_t e0, e1;
    PHX_CHECK(hipEventCreate(&e0));
    PHX_CHECK(hipEventCreate(&e1));
    for (int r = 0; r < reps + 1; ++r) {
      PHX_CHECK(hipEventRecord(e0, s));
      PHX_CHECK(phx::ext_mac(a, n, s));
      PHX_CHECK(hipEventRecord(e1, s));
      PHX_CHECK(hipEventSynchronize(e1));
      float ms = 0;
      PHX_CHECK(hipEventElapsedTime(&ms, e0, e1));
      if (r) tm.push_back(ms);
    }
    PHX_CHECK(hipEventDestroy(e0));
    PHX_CHECK(hipEventDestroy(e1));
  }
  // bytes one pass's launch must move: every plaintext once, every input once per 8 outputs, the
  // outputs written once
  const double mac_bytes = 8.0 * n * (static_cast<double>(group) * T * QlP + ((group + 7) / 8) * T * 2.0 * QlP + group * 2.0 * QlP);
  const Stat h = stat(th), b = stat(tb), m = stat(tm);
  std::printf("{\"time\": \"conv\", \"log_n\": %d, \"chain\": %zu, \"Ql\": %zu, \"QlP\": %zu, \"beta\": %zu, \"width\": %zu, "
              "\"in_ch\": %zu, \"out_ch\": %zu, \"kernel\": %zu, \"reps\": %d, \"group\": %zu, "
              "\"hoisted_ms\": {\"median\": %.3f, \"min\": %.3f, \"max\": %.3f}, "
              "\"baseline_ms\": {\"median\": %.3f, \"min\": %.3f, \"max\": %.3f}, \"speedup\": %.2f, "
              "\"hoisted_max_error\": %.3e, \"baseline_max_error\": %.3e, "
              "\"hoisted_ops\": {\"modups\": %zu, \"inner_products\": %zu, \"moddowns\": %zu, \"plaintext_bytes\": %.0f}, "
              "\"baseline_ops\": {\"modups\": %zu, \"inner_products\": %zu, \"moddowns\": %zu, \"host_encodes\": %zu}, "
              "\"ext_mac\": {\"terms\": %zu, \"outputs\": %zu, \"ms\": {\"median\": %.3f, \"min\": %.3f, \"max\": %.3f}, "
              "\"bytes\": %.0f, \"tb_per_s\": %.3f}}\n",
              log_n, chain, Ql, QlP, beta, width, in_ch, out_ch, K, reps, group, h.median, h.min, h.max, b.median, b.min,
              b.max, b.median / h.median, eh, eb, in_ch, T, 2 * out_ch, 8.0 * n * out_ch * T * QlP, out_ch * T, out_ch * T,
              2 * out_ch * T, out_ch * T, T, group, m.median, m.min, m.max, mac_bytes, m.median > 0 ? mac_bytes / (m.median * 1e-3) / 1e12 : 0.0);
  std::printf("{\"done\": \"conv_example time\", \"ok\": true}\n");
  return 0;
}

int main(int argc, char** argv) {
  try {
    if (argc >= 2 && !std::strcmp(argv[1], "check")) return run_check();
    if (argc >= 8 && !std::strcmp(argv[1], "time"))
      return run_time(std::atoi(argv[2]), std::strtoull(argv[3], nullptr, 10), std::strtoull(argv[4], nullptr, 10),
                      std::strtoull(argv[5], nullptr, 10), std::strtoull(argv[6], nullptr, 10),
                      std::strtoull(argv[7], nullptr, 10), argc >= 9 ? std::atoi(argv[8]) : 3,
                      argc >= 10 && !std::strcmp(argv[9], "hoisted"));
    std::fprintf(stderr, "usage: conv_example check | time <log_n> <chain> <width> <in_ch> <out_ch> <K> [reps] [hoisted]\n");
    return 2;
  } catch (const std::exception& e) {
    std::printf("{\"error\": \"%s\", \"ok\": false}\n", e.what());
    return 1;
  }
}
