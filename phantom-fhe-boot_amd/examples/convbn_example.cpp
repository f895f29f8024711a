// convbn_example — the residual block's linear part as one layer (DNN::PrepareConvBN, Conv(plan) with
// the plan's shift, DNN::ConvAdd; host/dnn.h) against the sequence it replaces, Conv(plan) ->
// BatchNorm -> Add, both through the C++ façade on the same ciphertexts and keys.  The batch norm's
// scale is folded into the weights, its shift and the residual enter the layer's one inner-sum launch
// as a seed that is a multiple of P (csrc/conv.h), so the fused layer leaves the input's chain index
// where the sequence leaves the next one.
//
// usage: convbn_example check
//          N = 2^12, CoeffModulus::Create(N, {60, 50, 50, 50, 50, 60, 60}), two special primes, scale
//          2^50; width 8, 3 -> 2 channels, K = 3; inputs, weights and batch-norm parameters from fixed
//          seeds, var in [0.5, 2], the rest in [-1, 1].  One JSON line per case, every error the
//          maximum absolute one against the cleartext:
//            convbn           Conv(PrepareConvBN)      | BatchNorm(Conv(PrepareConv))
//            convadd          ConvAdd(x, planBN, r)    | Add(BatchNorm(Conv(plan)), r)
//            convadd_stride2  the same at slotstr 1, stride 2, a residual of width 4 and slotstr 2
//            convadd_earlier_residual  layer at chain index 2, residual at 1 (it loses a limb)
//            resblock_chain   ConvAdd -> Conv(plan2 prepared at chain index 2)
//            refused          a residual of the wrong geometry, one at a later chain index, batch-norm
//                             vectors of the wrong length, a residual with another channel count
//          The sequence (`yardstick`) must be within 1e-3 and the fused layer within twice the
//          yardstick's error.  A last `done` line; exit status 0 iff every line is ok.
//        convbn_example bench [chain] [reps]
//          N = 2^16, the bootstrap's key chain ({60, 29 x 59} + 10 x 60), scale 2^59, a 16 -> 16 channel
//          3x3 layer at width 32 with the input at chain index <chain> (default 20).  Device time from
//          events on the context's stream, median and range of <reps> (default 5) after one warm-up,
//          all in one process: ConvAdd(x, planBN, r), Conv(plan) -> BatchNorm -> Add, and Conv(plan)
//          alone; the chain index each leaves.  One JSON line.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "../host/ckks_eval.h"
#include "../host/dnn.h"
#include "../host/encoder.h"
#include "../host/evaluate.h"
#include "../host/hip_check.h"
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

static BNParams random_bn(size_t ch, std::mt19937_64& rng) {
  std::uniform_real_distribution<double> unit(-1.0, 1.0), var(0.5, 2.0);
  BNParams bn;
  for (size_t c = 0; c < ch; ++c) {
    bn.weight.push_back(unit(rng));
    bn.bias.push_back(unit(rng));
    bn.mean.push_back(unit(rng));
    bn.var.push_back(var(rng));
  }
  return bn;
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

// a y + b per channel, plus r when given
static DNN::Tensor3 clear_bn_add(DNN::Tensor3 y, const BNParams& bn, const DNN::Tensor3* r) {
  for (size_t i = 0; i < y.size(); ++i)
    for (size_t j = 0; j < y[i].size(); ++j)
      for (size_t c = 0; c < y[i][j].size(); ++c) {
        const double a = bn.weight[c] / std::sqrt(bn.var[c] + 1e-5);
        y[i][j][c] = a * y[i][j][c] + bn.bias[c] - a * bn.mean[c] + (r ? (*r)[i][j][c] : 0.0);
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

template <class F>
static bool throws_invalid(F f) {
  try {
    f();
  } catch (const std::invalid_argument&) {
    return true;
  }
  return false;
}

// one context, key set and model for one layer geometry
struct Bed {
  PhantomContext ctx;
  PhantomCKKSEncoder encoder;
  PhantomSecretKey sk;
  PhantomPublicKey pk;
  DNN model;
  double scale;
  Bed(int log_n, double scale_, size_t width, size_t K, size_t slotstr)
      : ctx(make_parms(log_n)), encoder(ctx), sk(ctx), pk(sk.gen_publickey(ctx)),
        model(static_cast<size_t>(scale_), encoder, ctx), scale(scale_) {
    model.ComputeRotationIndices(sk, width, K, slotstr);
  }
  TensorCT encrypt(const DNN::Tensor3& image, size_t slotstr) {
    TensorCT t = model.EncTensor(image, pk, slotstr);
    if (model.scalingFactorsReal().empty()) {
      t.ctks_[0].PreComputeScale(ctx, scale);
      model.setScalingFactors(t.ctks_[0].getScalingFactorsReal(), t.ctks_[0].getScalingFactorsRealBig());
    }
    return t;
  }
};

static bool print_pair(const char* name, size_t slotstr, size_t stride, double fused_err, double yard_err,
                       const TensorCT& fused, const TensorCT& yard, bool extra_ok) {
  // the sequence is existing code, so it is the yardstick: within the bound of ckks_example (1e-3), else
  // the comparison says nothing; the fused layer, which rounds differently, at most twice its error
  const bool ok = yard_err < 1e-3 && fused_err <= 2 * yard_err && extra_ok;
  std::printf("{\"check\": \"%s\", \"log_n\": 12, \"width\": 8, \"slotstr\": %zu, \"in_ch\": 3, \"out_ch\": 2, \"kernel\": 3, "
              "\"stride\": %zu, \"fused_max_error\": %.6e, \"yardstick_max_error\": %.6e, \"fused\": %s, "
              "\"yardstick\": %s, \"ok\": %s}\n",
              name, slotstr, stride, fused_err, yard_err, metadata(fused).c_str(), metadata(yard).c_str(),
              ok ? "true" : "false");
  return ok;
}

static bool check_stride1() {
  const size_t width = 8, in_ch = 3, out_ch = 2, K = 3;
  Bed bed(12, std::ldexp(1.0, 50), width, K, 0);
  DNN& model = bed.model;
  std::mt19937_64 rng(0xC0B11);
  const DNN::Tensor3 image = random_image(width, in_ch, rng), rimage = random_image(width, out_ch, rng);
  const DNN::Weight4 weight = random_weight(K, in_ch, out_ch, rng), weight2 = random_weight(K, out_ch, out_ch, rng);
  const BNParams bn = random_bn(out_ch, rng);
  TensorCT input = bed.encrypt(image, 0), res = bed.encrypt(rimage, 0);
  const size_t chain = input.ctks_[0].chain_index();

  DNN::ConvPlan plan = model.PrepareConv(weight, width, 0, chain);
  DNN::ConvPlan planBN = model.PrepareConvBN(weight, bn, width, 0, chain);
  const DNN::Tensor3 conv = clear_conv(image, weight, 1);
  const DNN::Tensor3 want_bn = clear_bn_add(conv, bn, nullptr), want_add = clear_bn_add(conv, bn, &rimage);

  // convbn
  TensorCT unfused_conv = model.Conv(input, plan, 1);
  TensorCT yard_bn = model.BatchNorm(unfused_conv, bn.weight, bn.bias, bn.mean, bn.var);
  TensorCT fused_bn = model.Conv(input, planBN, 1);
  bool all = print_pair("convbn", 0, 1, max_error(model.DecTensor(fused_bn, bed.sk), want_bn),
                        max_error(model.DecTensor(yard_bn, bed.sk), want_bn), fused_bn, yard_bn,
                        fused_bn.ctks_[0].chain_index() == chain && yard_bn.ctks_[0].chain_index() == chain + 1);

  // convadd
  TensorCT yard_add = model.Add(yard_bn, res);
  TensorCT fused_add = model.ConvAdd(input, planBN, res, 1);
  all = print_pair("convadd", 0, 1, max_error(model.DecTensor(fused_add, bed.sk), want_add),
                   max_error(model.DecTensor(yard_add, bed.sk), want_add), fused_add, yard_add,
                   fused_add.ctks_[0].chain_index() == chain) && all;

  // the layer one chain index down, the residual where it was: it loses a limb on the way in
  {
    TensorCT low = input;
    for (PhantomCiphertext& c : low.ctks_) ModSwitchLevelInPlace(bed.ctx, c, 1);
    DNN::ConvPlan plan_low = model.PrepareConv(weight, width, 0, chain + 1);
    DNN::ConvPlan planBN_low = model.PrepareConvBN(weight, bn, width, 0, chain + 1);
    TensorCT yard = model.Add(model.BatchNorm(model.Conv(low, plan_low, 1), bn.weight, bn.bias, bn.mean, bn.var), res);
    TensorCT fused = model.ConvAdd(low, planBN_low, res, 1);
    all = print_pair("convadd_earlier_residual", 0, 1, max_error(model.DecTensor(fused, bed.sk), want_add),
                     max_error(model.DecTensor(yard, bed.sk), want_add), fused, yard,
                     fused.ctks_[0].chain_index() == chain + 1 && res.ctks_[0].chain_index() == chain) && all;
  }

  // resblock_chain: the second layer's input is the fused layer's degree-2 output, rescaled once
  {
    const PhantomCiphertext& f0 = fused_add.ctks_[0];
    const size_t chain2 = f0.chain_index() + (f0.GetNoiseScaleDeg() == 2 ? 1 : 0);
    DNN::ConvPlan plan2 = model.PrepareConv(weight2, width, 0, chain2);
    TensorCT second = model.Conv(fused_add, plan2, 1);
    const double e2 = max_error(model.DecTensor(second, bed.sk), clear_conv(want_add, weight2, 1));
    const bool ok2 = e2 < 1e-3 && second.ctks_[0].chain_index() == chain2;
    std::printf("{\"check\": \"resblock_chain\", \"log_n\": 12, \"max_error\": %.6e, \"first_chain_index\": %zu, "
                "\"second_chain_index\": %zu, \"first\": %s, \"second\": %s, \"ok\": %s}\n",
                e2, planBN.chain_index(), plan2.chain_index(), metadata(fused_add).c_str(), metadata(second).c_str(),
                ok2 ? "true" : "false");
    all = ok2 && all;
  }

  // refused
  {
    TensorCT narrow = bed.encrypt(random_image(width / 2, out_ch, rng), 0);  // width 4 where 8 is due
    TensorCT wide = bed.encrypt(random_image(width, out_ch + 1, rng), 0);    // 3 channels where 2 are due
    TensorCT later = res;
    for (PhantomCiphertext& c : later.ctks_) ModSwitchLevelInPlace(bed.ctx, c, 1);
    BNParams short_bn = bn;
    short_bn.mean.pop_back();
    const bool geometry = throws_invalid([&] { (void)model.ConvAdd(input, planBN, narrow, 1); });
    const bool later_chain = throws_invalid([&] { (void)model.ConvAdd(input, planBN, later, 1); });
    const bool bn_length = throws_invalid([&] { (void)model.PrepareConvBN(weight, short_bn, width, 0, chain); });
    const bool channels = throws_invalid([&] { (void)model.ConvAdd(input, planBN, wide, 1); });
    const bool okr = geometry && later_chain && bn_length && channels;
    auto tf = [](bool b) { return b ? "true" : "false"; };
    std::printf("{\"check\": \"refused\", \"residual_geometry\": %s, \"residual_later_chain_index\": %s, "
                "\"bn_vector_length\": %s, \"residual_channel_count\": %s, \"ok\": %s}\n",
                tf(geometry), tf(later_chain), tf(bn_length), tf(channels), tf(okr));
    all = okr && all;
  }
  return all;
}

static bool check_stride2() {
  const size_t width = 8, in_ch = 3, out_ch = 2, K = 3, slotstr = 1;
  Bed bed(12, std::ldexp(1.0, 50), width, K, slotstr);
  DNN& model = bed.model;
  std::mt19937_64 rng(0xC0B12);
  const DNN::Tensor3 image = random_image(width, in_ch, rng), rimage = random_image(width / 2, out_ch, rng);
  const DNN::Weight4 weight = random_weight(K, in_ch, out_ch, rng);
  const BNParams bn = random_bn(out_ch, rng);
  TensorCT input = bed.encrypt(image, slotstr), res = bed.encrypt(rimage, slotstr + 1);
  const size_t chain = input.ctks_[0].chain_index();
  DNN::ConvPlan plan = model.PrepareConv(weight, width, slotstr, chain);
  DNN::ConvPlan planBN = model.PrepareConvBN(weight, bn, width, slotstr, chain);
  const DNN::Tensor3 want = clear_bn_add(clear_conv(image, weight, 2), bn, &rimage);
  TensorCT yard = model.Add(model.BatchNorm(model.Conv(input, plan, 2), bn.weight, bn.bias, bn.mean, bn.var), res);
  TensorCT fused = model.ConvAdd(input, planBN, res, 2);
  return print_pair("convadd_stride2", slotstr, 2, max_error(model.DecTensor(fused, bed.sk), want),
                    max_error(model.DecTensor(yard, bed.sk), want), fused, yard,
                    fused.ctks_[0].chain_index() == chain && fused.width_ == width / 2 && fused.slotstr_ == slotstr + 1);
}

static int run_check() {
  bool all = check_stride1();
  all = check_stride2() && all;
  std::printf("{\"done\": \"convbn_example check\", \"ok\": %s}\n", all ? "true" : "false");
  return all ? 0 : 1;
}

struct Stat {
  double median, min, max;
};
static Stat stat(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return {v[v.size() / 2], v.front(), v.back()};
}

// device time of `reps` runs after one warm-up, by events on the stream the work is enqueued on
template <class F>
static Stat time_device(hipStream_t s, int reps, F run) {
  hipEvent_t e0, e1;
  PHX_CHECK(hipEventCreate(&e0));
  PHX_CHECK(hipEventCreate(&e1));
  std::vector<double> t;
  for (int r = 0; r < reps + 1; ++r) {
    PHX_CHECK(hipStreamSynchronize(s));
    PHX_CHECK(hipEventRecord(e0, s));
    run();
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

static int run_bench(size_t chain, int reps) {
  const int log_n = 16;
  const size_t width = 32, ch = 16, K = 3;
  Bed bed(log_n, std::ldexp(1.0, 59), width, K, 0);
  if (chain < 1 || chain + 2 >= bed.ctx.total_parm_size() || reps < 1) throw std::invalid_argument("bad chain or reps");
  DNN& model = bed.model;
  hipStream_t s = bed.ctx.stream();
  std::mt19937_64 rng(11);
  const DNN::Tensor3 image = random_image(width, ch, rng), rimage = random_image(width, ch, rng);
  const DNN::Weight4 weight = random_weight(K, ch, ch, rng);
  const BNParams bn = random_bn(ch, rng);
  TensorCT input = bed.encrypt(image, 0), res = bed.encrypt(rimage, 0);
  // the layer's level: drop limbs (the values and the scale stay)
  if (chain > 1)
    for (TensorCT* t : {&input, &res})
      for (PhantomCiphertext& c : t->ctks_) ModSwitchLevelInPlace(bed.ctx, c, chain - 1);
  DNN::ConvPlan plan = model.PrepareConv(weight, width, 0, chain);
  DNN::ConvPlan planBN = model.PrepareConvBN(weight, bn, width, 0, chain);

  TensorCT fused, unfused, plain;
  const Stat tf = time_device(s, reps, [&] { fused = model.ConvAdd(input, planBN, res, 1); });
  const Stat tu = time_device(s, reps, [&] {
    unfused = model.Add(model.BatchNorm(model.Conv(input, plan, 1), bn.weight, bn.bias, bn.mean, bn.var), res);
  });
  const Stat tp = time_device(s, reps, [&] { plain = model.Conv(input, plan, 1); });
  const DNN::Tensor3 want = clear_bn_add(clear_conv(image, weight, 1), bn, &rimage);
  const double ef = max_error(model.DecTensor(fused, bed.sk), want), eu = max_error(model.DecTensor(unfused, bed.sk), want);
  const size_t Ql = bed.ctx.get_context_data(chain).gpu_rns_tool().size_Ql();
  std::printf("{\"bench\": \"convbn\", \"log_n\": %d, \"chain\": %zu, \"Ql\": %zu, \"QlP\": %zu, \"width\": %zu, \"in_ch\": %zu, "
              "\"out_ch\": %zu, \"kernel\": %zu, \"reps\": %d, "
              "\"fused_ms\": {\"median\": %.3f, \"min\": %.3f, \"max\": %.3f}, "
              "\"unfused_ms\": {\"median\": %.3f, \"min\": %.3f, \"max\": %.3f}, "
              "\"conv_plan_ms\": {\"median\": %.3f, \"min\": %.3f, \"max\": %.3f}, \"speedup\": %.3f, "
              "\"fused_chain_index\": %zu, \"unfused_chain_index\": %zu, \"fused_max_error\": %.3e, "
              "\"unfused_max_error\": %.3e, \"fused\": %s, \"unfused\": %s}\n",
              log_n, chain, Ql, Ql + bed.ctx.size_P(), width, ch, ch, K, reps, tf.median, tf.min, tf.max, tu.median, tu.min,
              tu.max, tp.median, tp.min, tp.max, tf.median > 0 ? tu.median / tf.median : 0.0,
              fused.ctks_[0].chain_index(), unfused.ctks_[0].chain_index(), ef, eu, metadata(fused).c_str(),
              metadata(unfused).c_str());
  std::printf("{\"done\": \"convbn_example bench\", \"ok\": true}\n");
  return 0;
}

int main(int argc, char** argv) {
  try {
    if (argc >= 2 && !std::strcmp(argv[1], "check")) return run_check();
    if (argc >= 2 && !std::strcmp(argv[1], "bench"))
      return run_bench(argc >= 3 ? std::strtoull(argv[2], nullptr, 10) : 20, argc >= 4 ? std::atoi(argv[3]) : 5);
    std::fprintf(stderr, "usage: convbn_example check | bench [chain] [reps]\n");
    return 2;
  } catch (const std::exception& e) {
    std::printf("{\"error\": \"%s\", \"ok\": false}\n", e.what());
    return 1;
  }
}
