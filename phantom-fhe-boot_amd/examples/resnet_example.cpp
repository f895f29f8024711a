// resnet_example — the ResNet inference driver (host/resnet.h) and the .npy weight loader
// (host/npy.h) through the C++ façade.
//
// The chain is bootstrapping_example's: Q = {60, 29 x 59}, P = 10 x 60, scale 2^59, levelBudget {2, 2};
// keys and encryptions are seeded.
//
// usage: resnet_example check wiring <weights_dir> <image.npy> [log_n]
//          the net of tests/test_gpu_resnet_example.py (kDegTwo, width 8, 2 input channels, stages
//          {2, 4} with one block each, 3 classes) from .npy files: both schedules against the cleartext
//          network in double, the traces against the level plan, the chain indices of the two results,
//          rotation_indices() against the AddRotationIndicesTo / AddAvgPoolRotationsTo calls for the
//          geometries, kStreamed against kResident word for word.
//        resnet_example check composite [log_n]
//          kComposite on conv1 -> act -> one identity block -> head with 2 channels and seeded
//          synthetic weights: both schedules against the cleartext net with the same three sign
//          series in double.  The fused, packed path's maximum logit deviation must be at most twice
//          the layer-by-layer pack = 1 path's, which must be below a quarter of the cleartext logits'
//          spread; the series' measured level consumption must be within the plan's budget.
//        resnet_example check refuse [log_n]
//          every std::invalid_argument of the driver, the too-short chain among them.
//        resnet_example run <log_n> <weights_dir> <image.npy> <index> [spec flags]
//          one JSON row: the logits, the argmax, the level plan and the trace.  Spec flags:
//          --width W --in-ch C --stages a,b,c --blocks B --classes K --act composite|degtwo
//          --schedule fused|layers --residency streamed|resident
//        resnet_example infer [weights_dir image.npy index] [--residency both|streamed|resident]
//          the default ResNet-20 at N = 2^16, seeded synthetic weights and image when no directory is
//          given: device time per layer kind and in total, the peak pool bytes and plan bytes of
//          either residency, the argmax beside the cleartext network's.
//        resnet_example clear
//          the cleartext logits and the largest pre-activation of the synthetic nets above, on the host.
// One JSON line per case and a last `done` line; exit status 0 iff every line is ok.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "../host/bootstrap.h"
#include "../host/buffer.h"
#include "../host/ckks_eval.h"
#include "../host/dnn.h"
#include "../host/encoder.h"
#include "../host/keys.h"
#include "../host/modulus.h"
#include "../host/npy.h"
#include "../host/resnet.h"

using namespace phantom;
using namespace phantom::arith;
using Act = ResNetSpec::Activation;
using Sched = ResNetSpec::Schedule;

static const char* tf(bool b) { return b ? "true" : "false"; }

static EncryptionParameters make_parms(int log_n, int q_limbs) {
  const size_t n = size_t(1) << log_n;
  std::vector<int> bits(1, 60);
  bits.insert(bits.end(), q_limbs - 1, 59);
  bits.insert(bits.end(), 10, 60);
  EncryptionParameters parms(scheme_type::ckks);
  parms.set_poly_modulus_degree(n);
  parms.set_special_modulus_size(10);
  parms.set_coeff_modulus(CoeffModulus::Create(n, bits));
  return parms;
}

// context, seeded keys, the model and a bootstrapper
struct Rig {
  PhantomContext ctx;
  PhantomCKKSEncoder encoder;
  PhantomSecretKey sk;
  PhantomPublicKey pk;
  double scale = std::ldexp(1.0, 59);
  std::vector<double> sf, sf_big;
  DNN model;
  FHECKKSRNS boot;
  size_t n;

  explicit Rig(int log_n, int q_limbs = 30)
      : ctx(make_parms(log_n, q_limbs)), encoder(ctx), sk(PhantomSecretKey::for_testing(ctx, 0x9AC4)),
        pk(sk.gen_publickey(ctx)), model(static_cast<size_t>(std::ldexp(1.0, 59)), encoder, ctx), boot(encoder),
        n(size_t(1) << log_n) {
    PhantomCiphertext tmp;
    tmp.PreComputeScale(ctx, scale);
    sf = tmp.getScalingFactorsReal();
    sf_big = tmp.getScalingFactorsRealBig();
    model.setScalingFactors(sf, sf_big);
  }
};

// ---- the cleartext network ------------------------------------------------------------------------

static double cheb(const std::vector<double>& c, double b, double x) {
  const double u = x / b;
  double t0 = 1, t1 = u, s = 0.5 * c[0] + c[1] * u;
  for (size_t k = 2; k < c.size(); ++k) {
    const double t2 = 2 * u * t1 - t0;
    s += c[k] * t2;
    t0 = t1, t1 = t2;
  }
  return s;
}

// 0.5 x (1 + sign(0.1 x)) with DNN's three series
static double relu_composite_clear(double x) {
  double s = 0.1 * x;
  for (size_t k = 0; k < 3; ++k) s = cheb(DNN::SignCoefficients(k), DNN::SignInterval(k), s);
  return 0.5 * x * (s + 1);
}

struct Clear {
  std::vector<double> logits;
  double max_preactivation = 0;  // the largest |x| an activation sees
};

static DNN::Tensor3 clear_conv_bn(const DNN::Tensor3& x, const DNN::Weight4& w, const BNParams& bn, size_t stride) {
  const long width = static_cast<long>(x.size()), K = static_cast<long>(w.size()), half = K / 2;
  const size_t in_ch = w[0][0].size(), out_ch = w[0][0][0].size(), ow = x.size() / stride;
  DNN::Tensor3 y(ow, std::vector<std::vector<double>>(ow, std::vector<double>(out_ch, 0.0)));
  for (size_t i = 0; i < ow; ++i)
    for (size_t j = 0; j < ow; ++j)
      for (long a = 0; a < K; ++a)
        for (long b = 0; b < K; ++b) {
          const long r = static_cast<long>(i * stride) + a - half, c = static_cast<long>(j * stride) + b - half;
          if (r < 0 || r >= width || c < 0 || c >= width) continue;
          for (size_t k = 0; k < in_ch; ++k)
            for (size_t h = 0; h < out_ch; ++h) y[i][j][h] += x[r][c][k] * w[a][b][k][h];
        }
  for (size_t h = 0; h < out_ch; ++h) {
    const double s = bn.weight[h] / std::sqrt(bn.var[h] + 1e-5), t = bn.bias[h] - s * bn.mean[h];
    for (auto& row : y)
      for (auto& px : row) px[h] = s * px[h] + t;
  }
  return y;
}

static void clear_act(DNN::Tensor3& x, Act act, Clear& out) {
  for (auto& row : x)
    for (auto& px : row)
      for (double& v : px) {
        out.max_preactivation = std::max(out.max_preactivation, std::fabs(v));
        v = act == Act::kDegTwo ? v + v * v : relu_composite_clear(v);
      }
}

static Clear clear_forward(const ResNetSpec& spec, const ResNetWeights& w, const DNN::Tensor3& image) {
  Clear out;
  DNN::Tensor3 x = clear_conv_bn(image, w.conv1, w.bn1, 1);
  clear_act(x, spec.activation, out);
  for (size_t s = 0; s < spec.stage_channels.size(); ++s)
    for (size_t i = 0; i < spec.blocks_per_stage; ++i) {
      const ResNetBlockWeights& b = w.stages[s][i];
      const bool project = s > 0 && i == 0;
      const DNN::Tensor3 skip = project ? clear_conv_bn(x, b.down, b.down_bn, 2) : x;
      DNN::Tensor3 y = clear_conv_bn(x, b.conv1, b.bn1, project ? 2 : 1);
      clear_act(y, spec.activation, out);
      y = clear_conv_bn(y, b.conv2, b.bn2, 1);
      for (size_t r = 0; r < y.size(); ++r)
        for (size_t c = 0; c < y.size(); ++c)
          for (size_t h = 0; h < y[r][c].size(); ++h) y[r][c][h] += skip[r][c][h];
      clear_act(y, spec.activation, out);
      x = std::move(y);
    }
  const double area = static_cast<double>(x.size() * x.size());
  out.logits.assign(spec.classes, 0.0);
  for (size_t u = 0; u < spec.classes; ++u) {
    double acc = 0;
    for (const auto& row : x)
      for (const auto& px : row)
        for (size_t k = 0; k < px.size(); ++k) acc += w.fc_weight[u][k] * px[k];
    out.logits[u] = acc / area + w.fc_bias[u];
  }
  return out;
}

// ---- synthetic weights ----------------------------------------------------------------------------

// conv weights He-scaled (variance 2 / fan-in) and damped, batch-norm scales near 1 with variances in
// [0.5, 1.5], so that activations stay well inside [-10, 10], the sign series' interval after the 0.1
struct Synth {
  std::mt19937_64 rng;
  double damp;
  DNN::Weight4 conv(size_t K, size_t in, size_t out) {
    std::normal_distribution<double> g(0.0, damp * std::sqrt(2.0 / static_cast<double>(K * K * in)));
    DNN::Weight4 w(K, std::vector<std::vector<std::vector<double>>>(K, std::vector<std::vector<double>>(in, std::vector<double>(out))));
    for (auto& a : w)
      for (auto& b : a)
        for (auto& c : b)
          for (double& v : c) v = g(rng);
    return w;
  }
  BNParams bn(size_t ch) {
    std::uniform_real_distribution<double> gain(0.8, 1.2), small(-0.1, 0.1), var(0.5, 1.5);
    BNParams p;
    for (size_t h = 0; h < ch; ++h) {
      p.weight.push_back(gain(rng));
      p.bias.push_back(small(rng));
      p.mean.push_back(small(rng));
      p.var.push_back(var(rng));
    }
    return p;
  }
};

// the seeds and dampings of the synthetic nets (`clear` prints what they give, on the host)
static constexpr uint64_t kInferSeed = 0x2E50;
static constexpr double kInferDamp = 0.5, kProjectionDamp = 0.5;

static ResNetWeights synthetic_weights(const ResNetSpec& spec, uint64_t seed, double damp) {
  Synth s{std::mt19937_64(seed), damp};
  ResNetWeights w;
  w.conv1 = s.conv(3, spec.in_ch, spec.stage_channels[0]);
  w.bn1 = s.bn(spec.stage_channels[0]);
  w.stages.resize(spec.stage_channels.size());
  for (size_t st = 0; st < w.stages.size(); ++st)
    for (size_t i = 0; i < spec.blocks_per_stage; ++i) {
      const bool project = st > 0 && i == 0;
      const size_t out = spec.stage_channels[st], in = project ? spec.stage_channels[st - 1] : out;
      ResNetBlockWeights b;
      b.conv1 = s.conv(3, in, out);
      b.bn1 = s.bn(out);
      b.conv2 = s.conv(3, out, out);
      b.bn2 = s.bn(out);
      if (project) {
        b.down = s.conv(1, in, out);
        b.down_bn = s.bn(out);
      }
      w.stages[st].push_back(std::move(b));
    }
  std::uniform_real_distribution<double> unit(-1.0, 1.0);
  const size_t feat = spec.stage_channels.back();
  w.fc_weight.assign(spec.classes, std::vector<double>(feat));
  for (auto& row : w.fc_weight)
    for (double& v : row) v = unit(s.rng);
  for (size_t u = 0; u < spec.classes; ++u) w.fc_bias.push_back(0.5 * unit(s.rng));
  return w;
}

static DNN::Tensor3 synthetic_image(size_t width, size_t ch, uint64_t seed) {
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> unit(-1.0, 1.0);
  DNN::Tensor3 x(width, std::vector<std::vector<double>>(width, std::vector<double>(ch)));
  for (auto& row : x)
    for (auto& px : row)
      for (double& v : px) v = unit(rng);
  return x;
}

// ---- helpers ----------------------------------------------------------------------------------------

static std::vector<uint64_t> words(const PhantomContext& ctx, const PhantomCiphertext& x) {
  std::vector<uint64_t> h(x.size() * x.coeff_modulus_size() * ctx.poly_degree());
  PHX_CHECK(hipMemcpyAsync(h.data(), x.data(), h.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx.stream()));
  PHX_CHECK(hipStreamSynchronize(ctx.stream()));
  return h;
}

static bool same_tensor(const PhantomContext& ctx, const TensorCT& a, const TensorCT& b) {
  if (a.width_ != b.width_ || a.slotstr_ != b.slotstr_ || a.num_ch_ != b.num_ch_ || a.ctks_.size() != b.ctks_.size())
    return false;
  for (size_t k = 0; k < a.ctks_.size(); ++k) {
    const PhantomCiphertext &x = a.ctks_[k], &y = b.ctks_[k];
    if (x.chain_index() != y.chain_index() || x.scale() != y.scale() || x.GetNoiseScaleDeg() != y.GetNoiseScaleDeg() ||
        words(ctx, x) != words(ctx, y))
      return false;
  }
  return true;
}

static std::vector<double> logits_of(Rig& r, const TensorCT& out) {
  const DNN::Tensor3 t = r.model.DecTensor(out, r.sk);
  return t[0][0];
}

// a JSON number, or null for a value that is not finite
static std::string num(double v, const char* fmt = "%.6e") {
  if (!std::isfinite(v)) return "null";
  char buf[48];
  std::snprintf(buf, sizeof buf, fmt, v);
  return buf;
}

static std::string json_list(const std::vector<double>& v, const char* fmt = "%.12e") {
  std::string out = "[";
  for (size_t k = 0; k < v.size(); ++k) out += (k ? ", " : "") + num(v[k], fmt);
  return out + "]";
}

static std::string json_ints(const std::vector<int32_t>& v) {
  std::string out = "[";
  for (size_t k = 0; k < v.size(); ++k) out += (k ? ", " : "") + std::to_string(v[k]);
  return out + "]";
}

static std::string json_steps(const std::vector<ResNetStep>& steps, bool timed) {
  std::string out = "[";
  char buf[320];
  for (size_t k = 0; k < steps.size(); ++k) {
    const ResNetStep& s = steps[k];
    if (timed)
      std::snprintf(buf, sizeof buf,
                    "{\"name\": \"%s\", \"kind\": \"%s\", \"in\": [%zu, %zu], \"out\": [%zu, %zu], \"log2_scale\": [%.6f, %.6f], "
                    "\"device_ms\": %.3f}",
                    s.name.c_str(), s.kind.c_str(), s.in_chain, s.in_degree, s.out_chain, s.out_degree, s.in_log2_scale,
                    s.out_log2_scale, s.device_ms);
    else
      std::snprintf(buf, sizeof buf, "{\"name\": \"%s\", \"kind\": \"%s\", \"in\": [%zu, %zu], \"out\": [%zu, %zu]}",
                    s.name.c_str(), s.kind.c_str(), s.in_chain, s.in_degree, s.out_chain, s.out_degree);
    out += (k ? ", " : "") + std::string(buf);
  }
  return out + "]";
}

static bool trace_matches_plan(const ResNet& net) {
  const auto &p = net.level_plan(), &t = net.trace();
  if (p.size() != t.size()) return false;
  for (size_t k = 0; k < p.size(); ++k)
    if (p[k].name != t[k].name || p[k].kind != t[k].kind || p[k].in_chain != t[k].in_chain ||
        p[k].in_degree != t[k].in_degree || p[k].out_chain != t[k].out_chain || p[k].out_degree != t[k].out_degree)
      return false;
  return true;
}

static size_t argmax(const std::vector<double>& v) { return static_cast<size_t>(std::max_element(v.begin(), v.end()) - v.begin()); }

static double max_abs_diff(const std::vector<double>& a, const std::vector<double>& b) {
  double e = 0;
  for (size_t k = 0; k < a.size(); ++k) {
    const double d = std::fabs(a[k] - b[k]);
    if (!(d <= e)) e = d;  // NaN sticks
  }
  return e;
}

static double max_abs(const std::vector<double>& a) {
  double e = 0;
  for (double v : a) e = std::max(e, std::fabs(v));
  return e;
}

static const char* sched_name(Sched s) { return s == Sched::kFused ? "fused" : "layers"; }
static const char* act_name(Act a) { return a == Act::kComposite ? "composite" : "degtwo"; }

struct Run {
  TensorCT out;
  std::vector<double> logits;
};

// Setup, Prepare and Infer of one net on the rig
static Run run_net(Rig& r, ResNet& net, const ResNetWeights& w, const DNN::Tensor3& image, PlanResidency res, bool setup) {
  if (setup) net.Setup(r.sk, r.boot);
  net.Prepare(w, res);  // with Setup's bootstrapper
  const TensorCT input = r.model.EncTensor(image, r.pk, 0);
  Run run;
  run.out = net.Infer(input);
  run.logits = logits_of(r, run.out);
  return run;
}

// ---- check wiring -----------------------------------------------------------------------------------

static ResNetSpec wiring_spec(Sched schedule) {
  ResNetSpec spec;
  spec.width = 8, spec.in_ch = 2, spec.stage_channels = {2, 4}, spec.blocks_per_stage = 1, spec.classes = 3;
  spec.activation = Act::kDegTwo;
  spec.schedule = schedule;
  return spec;
}

static int run_check_wiring(const std::string& dir, const std::string& image_path, int log_n) {
  Rig r(log_n);
  bool all = true;
  const ResNetWeights w = LoadResNetWeights(dir, wiring_spec(Sched::kFused));
  const DNN::Tensor3 image = LoadImage(image_path, 0);
  const Clear clear = clear_forward(wiring_spec(Sched::kFused), w, image);
  const double largest = max_abs(clear.logits);

  ResNet layers(r.model, r.ctx, wiring_spec(Sched::kLayerByLayer), r.scale);
  ResNet fused(r.model, r.ctx, wiring_spec(Sched::kFused), r.scale);

  {  // the key list against the layers' own calls for the two geometries and the pooled one
    std::vector<int32_t> want;
    r.model.AddRotationIndicesTo(want, 8, 3, 0);
    r.model.AddRotationIndicesTo(want, 4, 3, 1);
    r.model.AddAvgPoolRotationsTo(want, 4, 1);
    std::vector<int32_t> got = fused.rotation_indices(), got_layers = layers.rotation_indices();
    const bool equal = got == want && got_layers == want && fused.bootstrap_slot_counts().empty();
    all = all && equal;
    std::printf("{\"check\": \"rotations\", \"rotation_indices\": %s, \"expected\": %s, \"ok\": %s}\n", json_ints(got).c_str(),
                json_ints(want).c_str(), tf(equal));
  }

  const Run a = run_net(r, layers, w, image, PlanResidency::kStreamed, true);
  const double err_layers = max_abs_diff(a.logits, clear.logits);
  {
    const bool plan_ok = trace_matches_plan(layers);
    const bool ok = plan_ok && err_layers < 1e-3 * largest;
    all = all && ok;
    std::printf("{\"check\": \"layer_by_layer\", \"log_n\": %d, \"logits\": %s, \"clear_logits\": %s, \"max_error\": %.6e, "
                "\"condition\": %.6e, \"trace_matches_plan\": %s, \"input_chain_index\": %zu, \"output_chain_index\": %zu, "
                "\"trace\": %s, \"ok\": %s}\n",
                log_n, json_list(a.logits).c_str(), json_list(clear.logits).c_str(), err_layers, 1e-3 * largest, tf(plan_ok),
                layers.input_chain_index(), a.out.ctks_[0].chain_index(), json_steps(layers.trace(), true).c_str(), tf(ok));
    std::fflush(stdout);
  }

  const Run b = run_net(r, fused, w, image, PlanResidency::kStreamed, true);
  const double err_fused = max_abs_diff(b.logits, clear.logits);
  {
    const bool plan_ok = trace_matches_plan(fused);
    const size_t bns = 1 + 2 * fused.stages() * fused.spec().blocks_per_stage;  // on the main path
    const size_t ca = a.out.ctks_[0].chain_index(), cb = b.out.ctks_[0].chain_index();
    const bool earlier = cb + bns == ca;
    const bool ok = plan_ok && earlier && err_fused <= 2 * err_layers;
    all = all && ok;
    std::printf("{\"check\": \"fused\", \"log_n\": %d, \"logits\": %s, \"max_error\": %.6e, \"layer_by_layer_max_error\": %.6e, "
                "\"trace_matches_plan\": %s, \"output_chain_index\": %zu, \"layer_by_layer_chain_index\": %zu, "
                "\"fused_batch_norms\": %zu, \"plan_bytes_peak\": %zu, \"plan_bytes_total\": %zu, \"trace\": %s, \"ok\": %s}\n",
                log_n, json_list(b.logits).c_str(), err_fused, err_layers, tf(plan_ok), cb, ca, bns, fused.plan_bytes_peak(),
                fused.plan_bytes_total(), json_steps(fused.trace(), true).c_str(), tf(ok));
    std::fflush(stdout);
  }

  {  // the same ciphertext through resident plans
    const TensorCT input = r.model.EncTensor(image, r.pk, 0);
    fused.Prepare(w, &r.boot, PlanResidency::kStreamed);
    const TensorCT streamed = fused.Infer(input);
    const size_t streamed_peak = fused.plan_bytes_peak();
    fused.Prepare(w, &r.boot, PlanResidency::kResident);
    const TensorCT resident = fused.Infer(input);
    const bool equal = same_tensor(r.ctx, streamed, resident);
    const bool ok = equal && fused.plan_bytes_peak() == fused.plan_bytes_total() && streamed_peak < fused.plan_bytes_total();
    all = all && ok;
    std::printf("{\"check\": \"residency\", \"words_equal\": %s, \"streamed_plan_bytes_peak\": %zu, "
                "\"resident_plan_bytes_peak\": %zu, \"plan_bytes_total\": %zu, \"ok\": %s}\n",
                tf(equal), streamed_peak, fused.plan_bytes_peak(), fused.plan_bytes_total(), tf(ok));
  }
  std::printf("{\"done\": \"resnet_example check wiring\", \"ok\": %s}\n", tf(all));
  return all ? 0 : 1;
}

// ---- check composite --------------------------------------------------------------------------------

static std::string json_uints(const std::vector<uint32_t>& v) {
  std::string out = "[";
  for (size_t k = 0; k < v.size(); ++k) out += (k ? ", " : "") + std::to_string(v[k]);
  return out + "]";
}

// both schedules of one kComposite net against the cleartext net with the same series
static bool composite_case(Rig& r, const char* name, ResNetSpec spec, uint64_t seed, double damp) {
  spec.activation = Act::kComposite;
  const ResNetWeights w = synthetic_weights(spec, seed, damp);
  const DNN::Tensor3 image = synthetic_image(spec.width, spec.in_ch, seed + 1);
  const Clear clear = clear_forward(spec, w, image);
  const double spread = *std::max_element(clear.logits.begin(), clear.logits.end()) -
                        *std::min_element(clear.logits.begin(), clear.logits.end());

  spec.schedule = Sched::kLayerByLayer;
  ResNet layers(r.model, r.ctx, spec, r.scale);
  const Run a = run_net(r, layers, w, image, PlanResidency::kStreamed, true);
  const bool plan_a = trace_matches_plan(layers);
  spec.schedule = Sched::kFused;
  ResNet fused(r.model, r.ctx, spec, r.scale);
  const Run b = run_net(r, fused, w, image, PlanResidency::kStreamed, true);
  const bool plan_b = trace_matches_plan(fused);
  std::vector<double> packs;
  for (size_t s = 0; s < fused.stages(); ++s) packs.push_back(static_cast<double>(fused.stage_pack(s)));

  const double dev_layers = max_abs_diff(a.logits, clear.logits), dev_fused = max_abs_diff(b.logits, clear.logits);
  const bool ok = plan_a && plan_b && dev_layers < 0.25 * spread && dev_fused <= 2 * dev_layers;
  std::printf("{\"check\": \"%s\", \"log_n\": %zu, \"seed\": %llu, \"damp\": %.3f, \"clear_logits\": %s, \"spread\": %s, "
              "\"max_preactivation\": %s, \"layer_by_layer_logits\": %s, \"fused_logits\": %s, "
              "\"layer_by_layer_max_deviation\": %s, \"fused_max_deviation\": %s, \"condition\": %s, "
              "\"packs\": %s, \"layer_by_layer_slot_counts\": %s, \"fused_slot_counts\": %s, "
              "\"traces_match_plans\": [%s, %s], \"input_chain_index\": [%zu, %zu], "
              "\"layer_by_layer_trace\": %s, \"fused_trace\": %s, \"ok\": %s}\n",
              name, static_cast<size_t>(std::log2(static_cast<double>(r.n))), static_cast<unsigned long long>(seed), damp,
              json_list(clear.logits).c_str(), num(spread).c_str(), num(clear.max_preactivation).c_str(),
              json_list(a.logits).c_str(), json_list(b.logits).c_str(), num(dev_layers).c_str(), num(dev_fused).c_str(),
              num(0.25 * spread).c_str(), json_list(packs, "%.0f").c_str(),
              json_uints(layers.bootstrap_slot_counts()).c_str(), json_uints(fused.bootstrap_slot_counts()).c_str(), tf(plan_a),
              tf(plan_b), layers.input_chain_index(), fused.input_chain_index(), json_steps(layers.trace(), true).c_str(),
              json_steps(fused.trace(), true).c_str(), tf(ok));
  std::fflush(stdout);
  return ok;
}

static int run_check_composite(int log_n) {
  Rig r(log_n);
  bool all = true;
  ResNetSpec spec;
  spec.width = 8, spec.in_ch = 2, spec.stage_channels = {2}, spec.blocks_per_stage = 1, spec.classes = 3;
  all = composite_case(r, "composite", spec, 0x2E5C, 1.0) && all;
  // a stride-2 block behind it: the projected skip leaves its layer one rescale after the bootstrap
  // the main path comes from, so the fused schedule drops conv2's input to it (host/resnet.h)
  spec.stage_channels = {2, 4};
  all = composite_case(r, "composite_projection", spec, 0x2E5D, kProjectionDamp) && all;

  {  // the first series' level consumption against the plan's budget (a degree-2 argument on [-1, 1])
    const PhantomRelinKey rlk = r.sk.gen_relinkey(r.ctx);
    TensorCT x = r.model.EncTensor(synthetic_image(8, 2, 0x2E5E), r.pk, 0);
    for (PhantomCiphertext& c : x.ctks_) EvalMultConstInplace(r.ctx, c, 0.1, r.sf);
    const size_t before = x.ctks_[0].chain_index();
    const TensorCT s = r.model.Sign(x, rlk, 0);
    const size_t used = s.ctks_[0].chain_index() - before, deg = s.ctks_[0].GetNoiseScaleDeg();
    const size_t budget = ps::GetMultiplicativeDepthByCoeffVector(DNN::SignCoefficients(0), true) + 1;
    const bool ok = used <= budget;
    all = all && ok;
    std::printf("{\"check\": \"series_budget\", \"levels_used\": %zu, \"degree_out\": %zu, \"budget\": %zu, \"ok\": %s}\n", used,
                deg, budget, tf(ok));
  }
  std::printf("{\"done\": \"resnet_example check composite\", \"ok\": %s}\n", tf(all));
  return all ? 0 : 1;
}

// ---- check refuse -----------------------------------------------------------------------------------

template <class F>
static bool refusal(const char* what, F&& f) {
  bool thrown = false;
  std::string why;
  try {
    f();
  } catch (const std::invalid_argument& e) {
    thrown = true;
    why = e.what();
  }
  for (char& c : why)
    if (c == '"' || c == '\\') c = '\'';
  std::printf("{\"check\": \"refusal\", \"case\": \"%s\", \"thrown\": %s, \"what\": \"%s\", \"ok\": %s}\n", what, tf(thrown),
              why.c_str(), tf(thrown));
  std::fflush(stdout);
  return thrown;
}

static int run_check_refuse(int log_n) {
  Rig r(log_n);
  bool all = true;
  const ResNetSpec spec = wiring_spec(Sched::kFused);
  const ResNetWeights w = synthetic_weights(spec, 0x5EF0, 0.5);
  const DNN::Tensor3 image = synthetic_image(spec.width, spec.in_ch, 0x5EF1);

  all = refusal("width halved below 1", [&] {
    ResNetSpec s = spec;
    s.width = 2, s.stage_channels = {2, 2, 2};
    ResNet net(r.model, r.ctx, s, r.scale);
  }) && all;
  all = refusal("width not a power of two", [&] {
    ResNetSpec s = spec;
    s.width = 12;
    ResNet net(r.model, r.ctx, s, r.scale);
  }) && all;
  all = refusal("no stage", [&] {
    ResNetSpec s = spec;
    s.stage_channels.clear();
    ResNet net(r.model, r.ctx, s, r.scale);
  }) && all;

  ResNet net(r.model, r.ctx, spec, r.scale);
  all = refusal("infer before prepare", [&] { net.Infer(r.model.EncTensor(image, r.pk, 0)); }) && all;
  all = refusal("missing rotation key", [&] { net.Prepare(w, &r.boot); }) && all;
  net.Setup(r.sk, r.boot);
  all = refusal("weights of another spec", [&] {
    ResNetWeights bad = w;
    bad.stages[1][0].conv1 = bad.stages[0][0].conv1;  // 2 -> 2 where the spec has 2 -> 4
    net.Prepare(bad, &r.boot);
  }) && all;
  all = refusal("missing projection", [&] {
    ResNetWeights bad = w;
    bad.stages[1][0].down.clear();
    net.Prepare(bad, &r.boot);
  }) && all;
  all = refusal("fc rows differ from the classes", [&] {
    ResNetWeights bad = w;
    bad.fc_weight.pop_back();
    net.Prepare(bad, &r.boot);
  }) && all;
  net.Prepare(w, &r.boot);
  all = refusal("input of another width", [&] { net.Infer(r.model.EncTensor(synthetic_image(4, spec.in_ch, 1), r.pk, 0)); }) && all;
  all = refusal("input with other channels", [&] { net.Infer(r.model.EncTensor(synthetic_image(8, 3, 1), r.pk, 0)); }) && all;
  all = refusal("input at another packing", [&] { net.Infer(r.model.EncTensor(synthetic_image(8, spec.in_ch, 1), r.pk, 1)); }) && all;

  {  // kDegTwo never bootstraps: a net deeper than the chain is refused by the plan, in Prepare
    ResNetSpec s = spec;
    s.stage_channels = {2};
    s.blocks_per_stage = 8;
    ResNet deep(r.model, r.ctx, s, r.scale);
    deep.Setup(r.sk, r.boot);
    const ResNetWeights dw = synthetic_weights(s, 0x5EF2, 0.5);
    const size_t last = deep.level_plan().back().out_chain;
    all = refusal("chain too short for x + x^2", [&] { deep.Prepare(dw, &r.boot); }) && all;
    std::printf("{\"check\": \"deep_plan\", \"planned_last_chain_index\": %zu, \"size_Q\": %zu, \"ok\": %s}\n", last,
                r.ctx.size_Q(), tf(last + 1 > r.ctx.size_Q()));
    all = all && last + 1 > r.ctx.size_Q();
  }
  {  // kComposite
    ResNetSpec s = spec;
    s.activation = Act::kComposite;
    s.stage_channels = {2};
    const ResNetWeights cw = synthetic_weights(s, 0x5EF3, 0.5);
    ResNet comp(r.model, r.ctx, s, r.scale);
    std::vector<int32_t> rots = comp.rotation_indices();
    r.model.BuildGaloisKey(r.sk, rots);
    all = refusal("null bootstrapper", [&] { comp.Prepare(cw, nullptr); }) && all;
    all = refusal("missing bootstrap setup", [&] { comp.Prepare(cw, &r.boot); }) && all;
    r.boot.EvalBootstrapSetup(r.ctx, {2, 2}, r.scale, r.sf, 0, comp.bootstrap_slot_counts().at(0));
    all = refusal("missing bootstrap keys", [&] { comp.Prepare(cw, &r.boot); }) && all;
    // a chain of 24 limbs: the bootstrap returns chain index 19, and a block's consumption from there
    // runs past what the next bootstrap accepts.  Refused by the plan alone: no key, no setup, no launch.
    Rig small(log_n, 24);
    ResNet shortnet(small.model, small.ctx, s, small.scale);
    const DevicePool::Stats before = DevicePool::instance().stats();
    all = refusal("chain too short for the composite activation", [&] { shortnet.Prepare(cw, &small.boot); }) && all;
    const DevicePool::Stats after = DevicePool::instance().stats();
    const bool quiet = before.live == after.live && before.held == after.held;
    std::printf("{\"check\": \"short_chain_no_allocation\", \"size_Q\": %zu, \"pool_unchanged\": %s, \"ok\": %s}\n",
                small.ctx.size_Q(), tf(quiet), tf(quiet));
    all = all && quiet;
  }
  std::printf("{\"done\": \"resnet_example check refuse\", \"ok\": %s}\n", tf(all));
  return all ? 0 : 1;
}

// ---- run / infer --------------------------------------------------------------------------------------

struct Options {
  ResNetSpec spec;
  PlanResidency residency = PlanResidency::kStreamed;
  std::string residency_name = "streamed";
};

static std::vector<size_t> parse_sizes(const std::string& s) {
  std::vector<size_t> v;
  size_t at = 0;
  while (at <= s.size()) {
    const size_t comma = std::min(s.find(',', at), s.size());
    v.push_back(std::strtoull(s.substr(at, comma - at).c_str(), nullptr, 10));
    at = comma + 1;
  }
  return v;
}

static Options parse_flags(int argc, char** argv, int first, bool allow_both) {
  Options o;
  if (allow_both) o.residency_name = "both";
  for (int i = first; i < argc; i += 2) {
    const std::string f = argv[i];
    if (i + 1 >= argc) throw std::invalid_argument("flag " + f + " needs a value");
    const std::string v = argv[i + 1];
    if (f == "--width") o.spec.width = std::strtoull(v.c_str(), nullptr, 10);
    else if (f == "--in-ch") o.spec.in_ch = std::strtoull(v.c_str(), nullptr, 10);
    else if (f == "--stages") o.spec.stage_channels = parse_sizes(v);
    else if (f == "--blocks") o.spec.blocks_per_stage = std::strtoull(v.c_str(), nullptr, 10);
    else if (f == "--classes") o.spec.classes = std::strtoull(v.c_str(), nullptr, 10);
    else if (f == "--act" && (v == "composite" || v == "degtwo")) o.spec.activation = v == "composite" ? Act::kComposite : Act::kDegTwo;
    else if (f == "--schedule" && (v == "fused" || v == "layers")) o.spec.schedule = v == "fused" ? Sched::kFused : Sched::kLayerByLayer;
    else if (f == "--residency" && (v == "streamed" || v == "resident" || (allow_both && v == "both"))) {
      o.residency = v == "resident" ? PlanResidency::kResident : PlanResidency::kStreamed;
      o.residency_name = v;
    } else throw std::invalid_argument("unknown flag or value: " + f + " " + v);
  }
  return o;
}

static int run_run(int log_n, const std::string& dir, const std::string& image_path, size_t index, const Options& o) {
  Rig r(log_n);
  const ResNetWeights w = LoadResNetWeights(dir, o.spec);
  const DNN::Tensor3 image = LoadImage(image_path, index);
  ResNet net(r.model, r.ctx, o.spec, r.scale);
  const Run run = run_net(r, net, w, image, o.residency, true);
  const bool ok = trace_matches_plan(net) && std::isfinite(max_abs(run.logits));
  std::printf("{\"run\": \"resnet_example\", \"log_n\": %d, \"schedule\": \"%s\", \"activation\": \"%s\", \"residency\": \"%s\", "
              "\"logits\": %s, \"argmax\": %zu, \"input_chain_index\": %zu, \"output_chain_index\": %zu, "
              "\"rotation_indices\": %s, \"plan_bytes_peak\": %zu, \"plan_bytes_total\": %zu, \"trace_matches_plan\": %s, "
              "\"plan\": %s, \"trace\": %s, \"ok\": %s}\n",
              log_n, sched_name(o.spec.schedule), act_name(o.spec.activation), o.residency_name.c_str(),
              json_list(run.logits).c_str(), argmax(run.logits), net.input_chain_index(), run.out.ctks_[0].chain_index(),
              json_ints(net.rotation_indices()).c_str(), net.plan_bytes_peak(), net.plan_bytes_total(),
              tf(trace_matches_plan(net)), json_steps(net.level_plan(), false).c_str(), json_steps(net.trace(), true).c_str(),
              tf(ok));
  return ok ? 0 : 1;
}

// the cleartext side of the synthetic nets alone (no device): what the seeds and dampings above give
static int run_clear() {
  auto row = [](const char* name, const ResNetSpec& spec, uint64_t seed, double damp) {
    const Clear c = clear_forward(spec, synthetic_weights(spec, seed, damp), synthetic_image(spec.width, spec.in_ch, seed + 1));
    std::printf("{\"clear\": \"%s\", \"seed\": %llu, \"damp\": %.3f, \"logits\": %s, \"max_preactivation\": %s}\n", name,
                static_cast<unsigned long long>(seed), damp, json_list(c.logits).c_str(), num(c.max_preactivation).c_str());
  };
  ResNetSpec spec;
  spec.width = 8, spec.in_ch = 2, spec.stage_channels = {2}, spec.blocks_per_stage = 1, spec.classes = 3;
  row("composite", spec, 0x2E5C, 1.0);
  spec.stage_channels = {2, 4};
  row("composite_projection", spec, 0x2E5D, kProjectionDamp);
  row("infer", ResNetSpec{}, kInferSeed, kInferDamp);
  return 0;
}

static int run_infer(const std::string& dir, const std::string& image_path, size_t index, const Options& o) {
  const int log_n = 16;
  Rig r(log_n);
  const ResNetSpec spec = o.spec;
  const uint64_t seed = kInferSeed;
  const double damp = kInferDamp;
  const ResNetWeights w = dir.empty() ? synthetic_weights(spec, seed, damp) : LoadResNetWeights(dir, spec);
  const DNN::Tensor3 image = dir.empty() ? synthetic_image(spec.width, spec.in_ch, seed + 1) : LoadImage(image_path, index);
  const Clear clear = clear_forward(spec, w, image);
  ResNet net(r.model, r.ctx, spec, r.scale);
  std::fprintf(stderr, "resnet_example infer: keys and bootstrap setups\n");
  net.Setup(r.sk, r.boot);
  PHX_CHECK(hipDeviceSynchronize());
  bool all = true;
  for (PlanResidency res : {PlanResidency::kStreamed, PlanResidency::kResident}) {
    const bool resident = res == PlanResidency::kResident;
    if (o.residency_name != "both" && resident != (o.residency == PlanResidency::kResident)) continue;
    std::fprintf(stderr, "resnet_example infer: %s plans\n", resident ? "resident" : "streamed");
    DevicePool::instance().reset_peak();
    net.Prepare(w, &r.boot, res);
    const TensorCT input = r.model.EncTensor(image, r.pk, 0);
    const TensorCT out = net.Infer(input);
    const std::vector<double> logits = logits_of(r, out);
    const DevicePool::Stats st = DevicePool::instance().stats();
    std::map<std::string, double> by_kind;
    double total = 0;
    for (const ResNetStep& s : net.trace()) {
      by_kind[s.kind] += s.device_ms;
      total += s.device_ms;
    }
    std::string kinds = "{";
    for (const auto& [k, ms] : by_kind) {
      char buf[64];
      std::snprintf(buf, sizeof buf, "%s\"%s\": %.3f", kinds.size() > 1 ? ", " : "", k.c_str(), ms);
      kinds += buf;
    }
    kinds += "}";
    const double dev = max_abs_diff(logits, clear.logits);
    const bool ok = trace_matches_plan(net) && std::isfinite(dev);
    all = all && ok;
    std::printf("{\"infer\": \"resnet20\", \"log_n\": %d, \"weights\": \"%s\", \"residency\": \"%s\", \"device_ms_by_kind\": %s, "
                "\"device_ms_total\": %.3f, \"pool_peak_live_bytes\": %zu, \"pool_peak_held_bytes\": %zu, "
                "\"plan_bytes_peak\": %zu, \"plan_bytes_total\": %zu, \"logits\": %s, \"clear_logits\": %s, "
                "\"max_deviation\": %s, \"max_preactivation\": %s, \"damp\": %.4f, \"argmax\": %zu, \"clear_argmax\": %zu, "
                "\"trace_matches_plan\": %s, \"trace\": %s, \"ok\": %s}\n",
                log_n, dir.empty() ? "synthetic" : "files", resident ? "resident" : "streamed", kinds.c_str(), total,
                st.peak_live, st.peak_held, net.plan_bytes_peak(), net.plan_bytes_total(), json_list(logits).c_str(),
                json_list(clear.logits).c_str(), num(dev).c_str(), num(clear.max_preactivation).c_str(), damp, argmax(logits),
                argmax(clear.logits),
                tf(trace_matches_plan(net)), json_steps(net.trace(), true).c_str(), tf(ok));
    std::fflush(stdout);
  }
  std::printf("{\"done\": \"resnet_example infer\", \"ok\": %s}\n", tf(all));
  return all ? 0 : 1;
}

int main(int argc, char** argv) {
  try {
    auto log_n_at = [&](int i) {
      const int log_n = argc > i ? std::atoi(argv[i]) : 12;
      if (log_n < 12 || log_n > 16) throw std::invalid_argument("log_n must be 12..16");
      return log_n;
    };
    if (argc >= 5 && !std::strcmp(argv[1], "check") && !std::strcmp(argv[2], "wiring"))
      return run_check_wiring(argv[3], argv[4], log_n_at(5));
    if (argc >= 3 && !std::strcmp(argv[1], "check") && !std::strcmp(argv[2], "composite")) return run_check_composite(log_n_at(3));
    if (argc >= 3 && !std::strcmp(argv[1], "check") && !std::strcmp(argv[2], "refuse")) return run_check_refuse(log_n_at(3));
    if (argc >= 6 && !std::strcmp(argv[1], "run"))
      return run_run(log_n_at(2), argv[3], argv[4], std::strtoull(argv[5], nullptr, 10), parse_flags(argc, argv, 6, false));
    if (argc >= 2 && !std::strcmp(argv[1], "clear")) return run_clear();
    if (argc >= 2 && !std::strcmp(argv[1], "infer")) {
      const bool files = argc >= 5 && std::strncmp(argv[2], "--", 2) != 0;
      return run_infer(files ? argv[2] : "", files ? argv[3] : "", files ? std::strtoull(argv[4], nullptr, 10) : 0,
                       parse_flags(argc, argv, files ? 5 : 2, true));
    }
    std::fprintf(stderr, "usage: resnet_example check wiring <weights_dir> <image.npy> [log_n] | check composite [log_n] | "
                         "check refuse [log_n] | run <log_n> <weights_dir> <image.npy> <index> [spec flags] | "
                         "infer [weights_dir image.npy index] [--residency both|streamed|resident]\n");
    return 2;
  } catch (const std::exception& e) {
    std::printf("{\"error\": \"%s\", \"ok\": false}\n", e.what());
    return 1;
  }
}
