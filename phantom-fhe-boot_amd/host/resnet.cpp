// resnet.cpp — see resnet.h
#include "resnet.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <stdexcept>

#include "avgpool.h"
#include "conv2d.h"
#include "hip_check.h"
#include "npy.h"
#include "pack.h"

namespace phantom {

namespace {

[[noreturn]] void bad(const std::string& why) { throw std::invalid_argument("ResNet: " + why); }

std::string block_name(size_t s, size_t i) { return "layer" + std::to_string(s + 1) + "_" + std::to_string(i); }

void check_weight4(const DNN::Weight4& w, size_t K, size_t in, size_t out, const std::string& name) {
  bool ok = w.size() == K;
  for (size_t a = 0; ok && a < K; ++a) {
    ok = w[a].size() == K;
    for (size_t b = 0; ok && b < K; ++b) {
      ok = w[a][b].size() == in;
      for (size_t k = 0; ok && k < in; ++k) ok = w[a][b][k].size() == out;
    }
  }
  if (!ok)
    bad(name + " must be [" + std::to_string(K) + "][" + std::to_string(K) + "][" + std::to_string(in) + "][" +
        std::to_string(out) + "]");
}

void check_bn(const BNParams& bn, size_t ch, const std::string& name) {
  if (bn.weight.size() != ch || bn.bias.size() != ch || bn.mean.size() != ch || bn.var.size() != ch)
    bad(name + " must hold " + std::to_string(ch) + " weights, biases, means and variances");
}

// the levels a sign series may take: the reference's depth for the coefficient vector (one less
// when the interval is [-1, 1] and no affine map runs), plus the rescale of a degree-2 argument
size_t series_budget(size_t k, size_t degree) {
  const bool unit = ChebyshevUnitInterval(-DNN::SignInterval(k), DNN::SignInterval(k));
  return ps::GetMultiplicativeDepthByCoeffVector(DNN::SignCoefficients(k), unit) + (degree == 2 ? 1 : 0);
}

size_t log2_ceil(size_t x) {
  size_t g = 0;
  while ((size_t(1) << g) < x) ++g;
  return g;
}

}  // namespace

void CheckResNetWeights(const ResNetWeights& w, const ResNetSpec& spec) {
  const size_t S = spec.stage_channels.size();
  if (S == 0) bad("the spec has no stage");
  check_weight4(w.conv1, 3, spec.in_ch, spec.stage_channels[0], "conv1");
  check_bn(w.bn1, spec.stage_channels[0], "bn1");
  if (w.stages.size() != S) bad("the weights hold " + std::to_string(w.stages.size()) + " stages, the spec " + std::to_string(S));
  for (size_t s = 0; s < S; ++s) {
    if (w.stages[s].size() != spec.blocks_per_stage) bad("stage " + std::to_string(s + 1) + " has the wrong number of blocks");
    const size_t out = spec.stage_channels[s];
    for (size_t i = 0; i < spec.blocks_per_stage; ++i) {
      const ResNetBlockWeights& b = w.stages[s][i];
      const std::string name = block_name(s, i);
      const bool project = s > 0 && i == 0;
      const size_t in = project ? spec.stage_channels[s - 1] : out;
      check_weight4(b.conv1, 3, in, out, name + "_conv1");
      check_bn(b.bn1, out, name + "_bn1");
      check_weight4(b.conv2, 3, out, out, name + "_conv2");
      check_bn(b.bn2, out, name + "_bn2");
      if (project) {
        check_weight4(b.down, 1, in, out, name + "_downsample_0");
        check_bn(b.down_bn, out, name + "_downsample_1");
      } else if (!b.down.empty()) {
        bad(name + " has a projection but keeps its stage's geometry");
      }
    }
  }
  if (w.fc_weight.size() != spec.classes) bad("fc_weight must have " + std::to_string(spec.classes) + " rows");
  for (const std::vector<double>& row : w.fc_weight)
    if (row.size() != spec.stage_channels.back()) bad("fc_weight must have " + std::to_string(spec.stage_channels.back()) + " columns");
  if (w.fc_bias.size() != spec.classes) bad("fc_bias must have " + std::to_string(spec.classes) + " entries");
}

ResNetWeights LoadResNetWeights(const std::string& dir, const ResNetSpec& spec) {
  ResNetWeights w;
  w.conv1 = LoadWeight4D(dir + "/conv1_weight.npy");
  w.bn1 = LoadBN(dir, "bn1");
  w.stages.resize(spec.stage_channels.size());
  for (size_t s = 0; s < w.stages.size(); ++s) {
    w.stages[s].resize(spec.blocks_per_stage);
    for (size_t i = 0; i < spec.blocks_per_stage; ++i) {
      ResNetBlockWeights& b = w.stages[s][i];
      const std::string name = block_name(s, i);
      b.conv1 = LoadWeight4D(dir + "/" + name + "_conv1_weight.npy");
      b.bn1 = LoadBN(dir, name + "_bn1");
      b.conv2 = LoadWeight4D(dir + "/" + name + "_conv2_weight.npy");
      b.bn2 = LoadBN(dir, name + "_bn2");
      if (s > 0 && i == 0) {
        b.down = LoadWeight4D(dir + "/" + name + "_downsample_0_weight.npy");
        b.down_bn = LoadBN(dir, name + "_downsample_1");
      }
    }
  }
  w.fc_weight = LoadWeight2D(dir + "/fc_weight.npy");
  w.fc_bias = LoadWeight1D(dir + "/fc_bias.npy");
  CheckResNetWeights(w, spec);
  return w;
}

ResNet::ResNet(DNN& model, const PhantomContext& context, const ResNetSpec& spec, double scale,
               std::vector<uint32_t> levelBudget)
    : model_(model), context_(context), spec_(spec), scale_(scale), budget_(std::move(levelBudget)) {
  const size_t S = spec_.stage_channels.size(), n = context_.poly_degree();
  if (S == 0) bad("the spec has no stage");
  if (spec_.blocks_per_stage == 0) bad("the spec has no block per stage");
  if (spec_.in_ch == 0 || spec_.classes == 0) bad("the input channels and the classes must not be 0");
  for (size_t c : spec_.stage_channels)
    if (c == 0) bad("a stage has 0 channels");
  if (spec_.width == 0 || (spec_.width & (spec_.width - 1))) bad("the input width must be a power of two");
  if (S - 1 >= 8 * sizeof(size_t) || (spec_.width >> (S - 1)) == 0) bad("the stages would halve the width below 1");
  if (budget_.size() != 2) bad("the level budget is {CoeffToSlot, SlotToCoeff}");
  // every geometry the layers will see, refused here as they would refuse it
  for (size_t s = 0; s < S; ++s) {
    const size_t in = s == 0 ? spec_.in_ch : spec_.stage_channels[s];
    (void)conv_shape(n, stage_width(s), stage_slotstr(s), 3, in, spec_.stage_channels[s]);
  }
  avgpool_shape(n, stage_width(S - 1), stage_slotstr(S - 1));
  build_plan();
}

size_t ResNet::stage_pack(size_t s, uint32_t correction) const {
  if (s >= stages()) bad("no such stage");
  if (spec_.schedule != ResNetSpec::Schedule::kFused || spec_.activation != ResNetSpec::Activation::kComposite) return 1;
  size_t pack = size_t(1) << log2_ceil(spec_.stage_channels[s]);
  pack = std::min(pack, model_.PackCapacity(stage_width(s), stage_slotstr(s)));
  if (correction < 8 * sizeof(size_t) - 1) pack = std::min(pack, size_t(1) << correction);
  return pack;
}

std::vector<int32_t> ResNet::rotation_indices(uint32_t correction) const {
  std::vector<int32_t> r;
  for (size_t s = 0; s < stages(); ++s) model_.AddRotationIndicesTo(r, stage_width(s), 3, stage_slotstr(s));
  model_.AddAvgPoolRotationsTo(r, stage_width(stages() - 1), stage_slotstr(stages() - 1));
  for (size_t s = 0; s < stages(); ++s)
    if (stage_pack(s, correction) > 1) model_.AddPackRotationsTo(r, stage_width(s), stage_slotstr(s), stage_pack(s, correction));
  return r;
}

std::vector<uint32_t> ResNet::bootstrap_slot_counts(uint32_t correction) const {
  std::vector<uint32_t> out;
  if (spec_.activation != ResNetSpec::Activation::kComposite) return out;
  for (size_t s = 0; s < stages(); ++s) {
    const size_t lg = stage_width(s) << stage_slotstr(s);
    const uint32_t slots = static_cast<uint32_t>(stage_pack(s, correction) * lg * lg);
    if (std::find(out.begin(), out.end(), slots) == out.end()) out.push_back(slots);
  }
  return out;
}

void ResNet::Setup(PhantomSecretKey& sk, FHECKKSRNS& bootstrapper) {
  std::vector<int32_t> rots = rotation_indices();
  model_.BuildGaloisKey(sk, rots);
  model_.RelinKeyGen(sk);
  relin_ = sk.gen_relinkey(context_);
  have_relin_ = true;
  setup_boot_ = &bootstrapper;
  if (spec_.activation != ResNetSpec::Activation::kComposite) return;
  bootstrapper.EvalMultKeyGen(sk, context_);
  for (uint32_t slots : bootstrap_slot_counts()) {
    bootstrapper.EvalBootstrapSetup(context_, budget_, scale_, model_.scalingFactorsReal(), 0, slots);
    bootstrapper.EvalBootstrapKeyGen(sk, context_, slots);
  }
}

// ---- the level plan -----------------------------------------------------------------------------

ResNet::Level ResNet::plan_step(const std::string& name, const char* kind, Level in, Level out) {
  ResNetStep st;
  st.name = name;
  st.kind = kind;
  st.in_chain = in.chain, st.in_degree = in.degree, st.out_chain = out.chain, st.out_degree = out.degree;
  plan_.push_back(std::move(st));
  // two limbs everywhere: a degree-2 scale does not fit one
  if (plan_error_.empty() && out.chain + 1 > context_.size_Q())
    plan_error_ = "the chain is too short: " + name + " would end at chain index " + std::to_string(out.chain) + " of " +
                  std::to_string(context_.size_Q());
  return out;
}

ResNet::Level ResNet::plan_act(const std::string& name, Level in, size_t stage) {
  const size_t Q = context_.size_Q();
  const Level mult{in.chain + (in.degree == 2 ? 1 : 0), 2};
  if (spec_.activation == ResNetSpec::Activation::kDegTwo) return plan_step(name, "act", in, mult);
  const size_t lg = stage_width(stage) << stage_slotstr(stage);
  const size_t slots = stage_pack(stage) * lg * lg;
  const size_t B = FHECKKSRNS::OutputChainIndex(budget_, static_cast<uint32_t>(log2_ceil(slots)));
  // the first series runs on 0.1 x (degree 2) and hands a degree-2 result to the bootstrap, which
  // rescales it and needs two limbs then (chain index Q - 1 at the latest); the two later series
  // start from the bootstrap's output, the last one followed by the product with x / 2
  const size_t first = mult.chain + series_budget(0, 2) + 1;
  const size_t second = B + series_budget(1, 1) + 1;
  const size_t third = B + series_budget(2, 1) + 1 + 1;
  if (plan_error_.empty() && (first > Q - 1 || second > Q - 1 || third > Q - 1))
    plan_error_ = "the chain is too short: " + name + " enters at chain index " + std::to_string(in.chain) +
                  ", the bootstrap returns chain index " + std::to_string(B) + ", and a sign series would reach " +
                  std::to_string(std::max({first, second, third})) + " where the bootstrap needs " + std::to_string(Q - 1) +
                  " at the latest";
  return plan_step(name, "act", in, Level{B, 1});
}

void ResNet::build_plan() {
  plan_.clear();
  plan_error_.clear();
  const bool fused = spec_.schedule == ResNetSpec::Schedule::kFused;
  const size_t Q = context_.size_Q();
  input_chain_ = 1;
  if (spec_.activation == ResNetSpec::Activation::kComposite) {
    // the latest input from which conv1 (+ bn1), the 0.1 x and the first series still reach the bootstrap
    const size_t need = (fused ? 0 : 1) + 1 + series_budget(0, 2) + 1;
    if (Q < need + 2) plan_error_ = "the chain is too short for the first activation";
    else input_chain_ = Q - 1 - need;
  }
  auto mult = [](Level l) { return Level{l.chain + (l.degree == 2 ? 1 : 0), 2}; };
  // conv (+ bn) (+ skip): the steps of one convolution of either schedule
  auto conv = [&](const std::string& name, Level in, const Level* skip) {
    if (fused) {
      // ConvAdd takes no skip at a later chain index than its own: the input is dropped to it first
      // (a projected skip right after a bootstrap is one rescale further than the main path)
      Level out = mult(in);
      if (skip) out.chain = std::max(out.chain, skip->chain + (skip->degree == 2 ? 1 : 0));
      return plan_step(name, "conv", in, out);
    }
    Level x = plan_step(name, "conv", in, mult(in));
    x = plan_step(name + "_bn", "bn", x, mult(x));
    if (skip) {
      const Level& hi = skip->chain > x.chain || (skip->chain == x.chain && skip->degree > x.degree) ? *skip : x;
      x = plan_step(name + "_add", "add", x, hi);
    }
    return x;
  };
  Level x{input_chain_, 1};
  x = conv("conv1", x, nullptr);
  x = plan_act("act0", x, 0);
  for (size_t s = 0; s < stages(); ++s)
    for (size_t i = 0; i < spec_.blocks_per_stage; ++i) {
      const std::string name = block_name(s, i);
      Level skip = x;
      if (s > 0 && i == 0) skip = conv(name + "_down", x, nullptr);
      Level y = conv(name + "_conv1", x, nullptr);
      y = plan_act(name + "_act1", y, s);
      y = conv(name + "_conv2", y, &skip);
      x = plan_act(name + "_act2", y, s);
    }
  plan_step("head", "head", x, mult(x));
}

// ---- preparation --------------------------------------------------------------------------------

void ResNet::Prepare(const ResNetWeights& weights, FHECKKSRNS* bootstrapper, PlanResidency residency) {
  prepared_ = false;
  plans_.clear();
  plan_live_ = plan_peak_ = plan_total_ = 0;
  CheckResNetWeights(weights, spec_);
  if (!plan_error_.empty()) bad(plan_error_);
  const size_t n = context_.poly_degree();
  const bool composite = spec_.activation == ResNetSpec::Activation::kComposite;
  if (composite && !bootstrapper) bad("the composite activation needs a bootstrapper");
  const uint32_t correction = composite ? bootstrapper->correction_factor() : kDefaultCorrection;
  for (int32_t r : rotation_indices()) {
    const uint32_t e = FindAutomorphismIndex2nComplex(r, n);
    if (e != 1 && !model_.galois_keys().has(e))
      bad("the model has no key for rotation " + std::to_string(r) + " (Setup, or BuildGaloisKey with rotation_indices())");
  }
  if (composite) {
    for (uint32_t slots : bootstrap_slot_counts()) {
      size_t out = 0;
      try {
        out = bootstrapper->output_chain_index(slots);
      } catch (const std::invalid_argument&) {
        bad("no bootstrap setup for " + std::to_string(slots) + " slots (Setup, or EvalBootstrapSetup with bootstrap_slot_counts())");
      }
      if (out != FHECKKSRNS::OutputChainIndex(budget_, static_cast<uint32_t>(log2_ceil(slots))))
        bad("the bootstrap setup for " + std::to_string(slots) + " slots has another level budget than the plan's");
      for (int r : bootstrapper->rotation_indices(slots))
        if (!bootstrapper->GetGaloisKey().has(FindAutomorphismIndex2nComplex(r, n)))
          bad("the bootstrapper has no keys for " + std::to_string(slots) + " slots (EvalBootstrapKeyGen)");
      if (!bootstrapper->GetGaloisKey().has(static_cast<uint32_t>(2 * n - 1)))
        bad("the bootstrapper has no conjugation key (EvalBootstrapKeyGen)");
    }
    for (size_t s = 0; s < stages(); ++s)
      if (log2_ceil(stage_pack(s)) > correction) bad("a stage's pack exceeds the bootstrapper's correction factor");
  } else if (!have_relin_) {
    bad("no relinearisation key (Setup)");
  }
  weights_ = weights;
  // the average's 1 / width^2 goes into the fully connected weights (AvgPoolFullCon sums)
  const double w_last = static_cast<double>(stage_width(stages() - 1));
  for (std::vector<double>& row : weights_.fc_weight)
    for (double& v : row) v /= w_last * w_last;
  boot_ = bootstrapper;
  residency_ = residency;
  prepared_ = true;
  if (residency == PlanResidency::kResident && spec_.schedule == ResNetSpec::Schedule::kFused) {
    // every layer's plan, at the chain index the level plan gives its input after the rescale
    auto at = [&](const std::string& name) {
      for (const ResNetStep& st : plan_)
        if (st.name == name) return st.out_chain;
      bad("no such layer " + name);
    };
    plan_for("conv1", weights_.conv1, weights_.bn1, stage_width(0), 0, at("conv1"));
    for (size_t s = 0; s < stages(); ++s)
      for (size_t i = 0; i < spec_.blocks_per_stage; ++i) {
        const ResNetBlockWeights& b = weights_.stages[s][i];
        const std::string name = block_name(s, i);
        const size_t in_stage = s > 0 && i == 0 ? s - 1 : s;
        if (s > 0 && i == 0)
          plan_for(name + "_down", b.down, b.down_bn, stage_width(in_stage), in_stage, at(name + "_down"));
        plan_for(name + "_conv1", b.conv1, b.bn1, stage_width(in_stage), in_stage, at(name + "_conv1"));
        plan_for(name + "_conv2", b.conv2, b.bn2, stage_width(s), s, at(name + "_conv2"));
      }
  }
}

const DNN::ConvPlan& ResNet::plan_for(const std::string& name, const DNN::Weight4& w, const BNParams& bn, size_t width,
                                      size_t slotstr, size_t chain) {
  for (const auto& p : plans_)
    if (p.first == name) return p.second;
  plans_.emplace_back(name, model_.PrepareConvBN(w, bn, width, slotstr, chain));
  const size_t bytes = plans_.back().second.bytes();
  plan_live_ += bytes;
  plan_total_ += bytes;
  plan_peak_ = std::max(plan_peak_, plan_live_);
  return plans_.back().second;
}

void ResNet::release_plan(const std::string& name) {
  if (residency_ == PlanResidency::kResident) return;
  for (size_t k = 0; k < plans_.size(); ++k)
    if (plans_[k].first == name) {
      // the layer that read it is still in flight: wait for it, then free
      PHX_CHECK(hipStreamSynchronize(context_.stream()));
      plan_live_ -= plans_[k].second.bytes();
      plans_.erase(plans_.begin() + static_cast<std::ptrdiff_t>(k));
      return;
    }
}

// ---- inference ----------------------------------------------------------------------------------

template <class F>
TensorCT ResNet::timed(const std::string& name, const char* kind, const TensorCT& in, F&& f) {
  hipEvent_t e0, e1;
  PHX_CHECK(hipEventCreate(&e0));
  PHX_CHECK(hipEventCreate(&e1));
  events_.emplace_back(e0, e1);
  ResNetStep st;
  st.name = name;
  st.kind = kind;
  const PhantomCiphertext& a = in.ctks_.at(0);
  st.in_chain = a.chain_index(), st.in_degree = a.GetNoiseScaleDeg(), st.in_log2_scale = std::log2(a.scale());
  trace_.push_back(st);
  const size_t at = trace_.size() - 1;
  PHX_CHECK(hipEventRecord(e0, context_.stream()));
  TensorCT out = f();
  PHX_CHECK(hipEventRecord(e1, context_.stream()));
  const PhantomCiphertext& b = out.ctks_.at(0);
  trace_[at].out_chain = b.chain_index(), trace_[at].out_degree = b.GetNoiseScaleDeg();
  trace_[at].out_log2_scale = std::log2(b.scale());
  return out;
}

TensorCT ResNet::run_conv(const std::string& name, const TensorCT& x, const DNN::Weight4& w, const BNParams& bn,
                          size_t stride, const TensorCT* residual) {
  if (spec_.schedule == ResNetSpec::Schedule::kFused) {
    const PhantomCiphertext& a = x.ctks_.at(0);
    size_t chain = a.chain_index() + (a.GetNoiseScaleDeg() == 2 ? 1 : 0), drop = 0;
    if (residual) {
      const PhantomCiphertext& r0 = residual->ctks_.at(0);
      const size_t need = r0.chain_index() + (r0.GetNoiseScaleDeg() == 2 ? 1 : 0);
      if (need > chain) drop = need - chain, chain = need;
    }
    const DNN::ConvPlan& plan = plan_for(name, w, bn, x.width_, x.slotstr_, chain);
    TensorCT y = timed(name, "conv", x, [&] {
      if (!residual) return model_.Conv(x, plan, stride);
      if (!drop) return model_.ConvAdd(x, plan, *residual, stride);
      TensorCT lower = x;  // to the skip's chain index: limbs go, the degree stays
      for (PhantomCiphertext& c : lower.ctks_) ModSwitchLevelInPlace(context_, c, drop);
      return model_.ConvAdd(lower, plan, *residual, stride);
    });
    release_plan(name);
    return y;
  }
  TensorCT y = timed(name, "conv", x, [&] { return model_.Conv(x, w, stride); });
  y = timed(name + "_bn", "bn", y, [&] { return model_.BatchNorm(y, bn.weight, bn.bias, bn.mean, bn.var); });
  if (residual) y = timed(name + "_add", "add", y, [&] { return model_.Add(y, *residual); });
  return y;
}

TensorCT ResNet::run_act(const std::string& name, const TensorCT& x, size_t stage) {
  return timed(name, "act", x, [&] {
    if (spec_.activation == ResNetSpec::Activation::kDegTwo) return model_.ReluDegTwo(x, relin_);
    return model_.ReluComposite(x, *boot_, stage_pack(stage));
  });
}

TensorCT ResNet::Infer(const TensorCT& input) {
  if (!prepared_) bad("Infer before Prepare");
  if (input.width_ != spec_.width || input.slotstr_ != 0 || input.num_ch_ != spec_.in_ch || input.ctks_.size() != spec_.in_ch)
    bad("the input tensor's geometry is not the spec's");
  for (const PhantomCiphertext& c : input.ctks_)
    if (c.size() != 2 || c.GetNoiseScaleDeg() != 1 || c.chain_index() > input_chain_ || c.chain_index() < 1)
      bad("the input must be fresh degree-1 ciphertexts at or above the plan's input chain index");
  for (const auto& e : events_) {  // of an inference that threw
    (void)hipEventDestroy(static_cast<hipEvent_t>(e.first));
    (void)hipEventDestroy(static_cast<hipEvent_t>(e.second));
  }
  events_.clear();
  trace_.clear();
  if (residency_ == PlanResidency::kStreamed) plan_peak_ = plan_live_;
  TensorCT x = input;
  for (PhantomCiphertext& c : x.ctks_)
    if (c.chain_index() < input_chain_) ModSwitchLevelInPlace(context_, c, input_chain_ - c.chain_index());

  x = run_conv("conv1", x, weights_.conv1, weights_.bn1, 1, nullptr);
  x = run_act("act0", x, 0);
  for (size_t s = 0; s < stages(); ++s)
    for (size_t i = 0; i < spec_.blocks_per_stage; ++i) {
      const ResNetBlockWeights& b = weights_.stages[s][i];
      const std::string name = block_name(s, i);
      const bool project = s > 0 && i == 0;
      TensorCT skip = project ? run_conv(name + "_down", x, b.down, b.down_bn, 2, nullptr) : x;
      TensorCT y = run_conv(name + "_conv1", x, b.conv1, b.bn1, project ? 2 : 1, nullptr);
      y = run_act(name + "_act1", y, s);
      y = run_conv(name + "_conv2", y, b.conv2, b.bn2, 1, &skip);
      x = run_act(name + "_act2", y, s);
    }
  x = timed("head", "head", x, [&] { return model_.AvgPoolFullCon(x, weights_.fc_weight, weights_.fc_bias); });

  PHX_CHECK(hipStreamSynchronize(context_.stream()));
  for (size_t k = 0; k < events_.size(); ++k) {
    float ms = 0;
    hipEvent_t e0 = static_cast<hipEvent_t>(events_[k].first), e1 = static_cast<hipEvent_t>(events_[k].second);
    PHX_CHECK(hipEventElapsedTime(&ms, e0, e1));
    trace_[k].device_ms = ms;
    PHX_CHECK(hipEventDestroy(e0));
    PHX_CHECK(hipEventDestroy(e1));
  }
  events_.clear();
  return x;
}

}  // namespace phantom
