// resnet.h — a CIFAR-style ResNet inference driver over the DNN layers (dnn.h), the application the
// reference's Resnet/ program builds by hand (Resnet/models/model_resnet20.cu): conv1 + bn1 +
// activation; per stage, blocks of conv - bn - act - conv - bn (+ skip) - act, the first block of every
// stage after the first with stride 2 and a 1x1 stride-2 projection with its own batch norm on the
// skip; AvgPoolFullCon as the head, the 1 / width^2 of the average folded into its weights here.
//
// It adds no kernel and no layer: it sequences the existing members, keeps the level bookkeeping
// (a plan at the right chain index, a residual at a level the layer accepts, the pack rotations),
// and refuses on the host, before anything runs, what would fail deep inside a layer.
//
// Two schedules compute the same network:
//   kFused (default)   PrepareConvBN + Conv(plan) / ConvAdd(plan, skip), ReluComposite(.., stage_pack)
//   kLayerByLayer      Conv(weight) -> BatchNorm -> Add -> ReluComposite(.., 1): the reference's own
//                      sequence through the plain members; the documented slow path and the yardstick
//                      the fused schedule is tested against.
//
// Level plan (DESIGN.md §3 "ResNet driver").  A state is (chain index c, noise-scale degree d).
//   Conv, BatchNorm, ReluDegTwo, AvgPoolFullCon, the activation's 0.1 x: (c, d) -> (c + [d = 2], 2)
//   ConvAdd: the same, from the later of its input's and its skip's chain index after their rescales
//            (ConvAdd takes no skip later than its own level: the driver drops the input to it, which
//            happens where a projected skip follows a bootstrap)
//   Add: the state of the operand at the later chain index (the larger degree among equals)
//   ReluComposite: (B, 1), B the bootstrap's output chain index (FHECKKSRNS::OutputChainIndex)
// Each sign series is budgeted the reference's depth for its coefficient vector
// (ps::GetMultiplicativeDepthByCoeffVector) plus one level for a degree-2 entry, and a bootstrap
// needs two limbs after the rescale of a degree-2 input.  The input is dropped
// (ModSwitchLevelInPlace) to the latest chain index from which the first activation still fits.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "bootstrap.h"
#include "dnn.h"

namespace phantom {

struct ResNetSpec {
  enum class Activation { kComposite, kDegTwo };    // DNN::ReluComposite | DNN::ReluDegTwo (x + x^2, no bootstrap)
  enum class Schedule { kFused, kLayerByLayer };
  size_t width = 32;                                // input width, a power of two
  size_t in_ch = 3;
  std::vector<size_t> stage_channels = {16, 32, 64};
  size_t blocks_per_stage = 3;
  size_t classes = 10;
  Activation activation = Activation::kComposite;
  Schedule schedule = Schedule::kFused;
};

struct ResNetBlockWeights {
  DNN::Weight4 conv1, conv2;  // [3][3][in][out], [3][3][out][out]
  BNParams bn1, bn2;
  DNN::Weight4 down;          // [1][1][in][out]; empty unless the block projects its skip
  BNParams down_bn;
};

struct ResNetWeights {
  DNN::Weight4 conv1;  // [3][3][in_ch][stage_channels[0]]
  BNParams bn1;
  std::vector<std::vector<ResNetBlockWeights>> stages;  // [stage][block]
  std::vector<std::vector<double>> fc_weight;           // [classes][stage_channels.back()], the plain FC weights
  std::vector<double> fc_bias;                          // [classes]
};

// std::invalid_argument unless every shape is the spec's
void CheckResNetWeights(const ResNetWeights& w, const ResNetSpec& spec);
// conv1_weight.npy, bn1_{weight,bias,running_mean,running_var}.npy, layer<s>_<i>_conv1_weight.npy,
// .._bn1_*, .._conv2_weight.npy, .._bn2_*, layer<s>_<i>_downsample_0_weight.npy, .._downsample_1_*
// (s from 1, i from 0), fc_weight.npy, fc_bias.npy under `dir` (host/npy.h; std::runtime_error for a
// file the loader refuses), then CheckResNetWeights
ResNetWeights LoadResNetWeights(const std::string& dir, const ResNetSpec& spec);

enum class PlanResidency { kStreamed, kResident };

// one step of the level plan, and of an inference's trace
struct ResNetStep {
  std::string name;  // "conv1", "act0", "layer2_0_conv1", "layer2_0_down", "layer2_0_add", "head", ..
  std::string kind;  // "conv" | "bn" | "add" | "act" | "head"
  size_t in_chain = 0, in_degree = 0, out_chain = 0, out_degree = 0;
  // trace only
  double in_log2_scale = 0, out_log2_scale = 0, device_ms = 0;
};

class ResNet {
 public:
  // `scale` is the DNN's; levelBudget the bootstrap setups' (kComposite).  std::invalid_argument: a
  // width that is no power of two or that the stages would halve below 1, no stage, no block, a
  // channel or class count of 0, a geometry the layers refuse (conv_shape, avgpool_shape).
  ResNet(DNN& model, const PhantomContext& context, const ResNetSpec& spec, double scale,
         std::vector<uint32_t> levelBudget = {2, 2});

  const ResNetSpec& spec() const { return spec_; }
  size_t stages() const { return spec_.stage_channels.size(); }
  size_t stage_width(size_t s) const { return spec_.width >> s; }
  size_t stage_slotstr(size_t s) const { return s; }
  // the smallest power of two >= the stage's channels, capped by PackCapacity and 2^correction
  // (`correction`: the bootstrapper's correction factor; the default is the least EvalBootstrapSetup
  // chooses when asked for 0, and Prepare refuses a bootstrapper set up with less); 1 unless the
  // schedule is kFused and the activation kComposite
  size_t stage_pack(size_t s, uint32_t correction = kDefaultCorrection) const;
  // the conv taps of every stage geometry, the pooling rotations, and for kFused + kComposite the
  // pack rotations of every stage, in that order without repeats
  std::vector<int32_t> rotation_indices(uint32_t correction = kDefaultCorrection) const;
  // the distinct stage_pack(s) (width_s 2^s)^2 the stages bootstrap at; empty for kDegTwo
  std::vector<uint32_t> bootstrap_slot_counts(uint32_t correction = kDefaultCorrection) const;
  // the model's rotation and relinearisation keys and, for kComposite, the bootstrapper's
  // multiplication key and its setup and keys for every slot count above
  void Setup(PhantomSecretKey& sk, FHECKKSRNS& bootstrapper);

  // the level plan from an input at chain index input_chain_index(), degree 1
  size_t input_chain_index() const { return input_chain_; }
  const std::vector<ResNetStep>& level_plan() const { return plan_; }
  size_t output_chain_index() const { return plan_.back().out_chain; }

  // Checks the weights against the spec, the keys and bootstrap setups against rotation_indices()
  // and bootstrap_slot_counts(), and the level plan against the chain: std::invalid_argument for a
  // mismatch, a missing key or setup, or a chain too short (for kComposite: the bootstrap's output
  // level minus one block's consumption falls below the bootstrap's input level).  kResident then
  // prepares every layer's plan (kFused); kStreamed prepares each just before its layer in Infer and
  // releases it after.  The weights are copied.
  void Prepare(const ResNetWeights& weights, FHECKKSRNS* bootstrapper, PlanResidency residency = PlanResidency::kStreamed);
  // with the bootstrapper Setup was given (none: kComposite is refused)
  void Prepare(const ResNetWeights& weights, PlanResidency residency = PlanResidency::kStreamed) {
    Prepare(weights, setup_boot_, residency);
  }
  // `classes` ciphertexts; logit u is the value at pixel (0, 0) of channel u.  The input must be an
  // EncTensor of the spec's geometry at or above input_chain_index(); it is dropped to it.
  TensorCT Infer(const TensorCT& input);
  const std::vector<ResNetStep>& trace() const { return trace_; }
  // device bytes of the prepared plans: the most held at once during the last Infer (kStreamed) or
  // since Prepare (kResident), and the sum over all layers
  size_t plan_bytes_peak() const { return plan_peak_; }
  size_t plan_bytes_total() const { return plan_total_; }

  static constexpr uint32_t kDefaultCorrection = 7;

 private:
  struct Level {
    size_t chain, degree;
  };
  void build_plan();
  Level plan_act(const std::string& name, Level in, size_t stage);
  Level plan_step(const std::string& name, const char* kind, Level in, Level out);
  TensorCT run_conv(const std::string& name, const TensorCT& x, const DNN::Weight4& w, const BNParams& bn, size_t stride,
                    const TensorCT* residual);
  TensorCT run_act(const std::string& name, const TensorCT& x, size_t stage);
  template <class F>
  TensorCT timed(const std::string& name, const char* kind, const TensorCT& in, F&& f);
  const DNN::ConvPlan& plan_for(const std::string& name, const DNN::Weight4& w, const BNParams& bn, size_t width,
                                size_t slotstr, size_t chain);
  void release_plan(const std::string& name);

  DNN& model_;
  const PhantomContext& context_;
  ResNetSpec spec_;
  double scale_;
  std::vector<uint32_t> budget_;
  size_t input_chain_ = 1;
  std::vector<ResNetStep> plan_, trace_;
  std::string plan_error_;  // why the chain is too short (empty: it is not)

  ResNetWeights weights_;
  bool prepared_ = false;
  PlanResidency residency_ = PlanResidency::kStreamed;
  FHECKKSRNS* boot_ = nullptr;
  FHECKKSRNS* setup_boot_ = nullptr;  // Setup's
  PhantomRelinKey relin_;  // ReluDegTwo's
  bool have_relin_ = false;
  std::vector<std::pair<std::string, DNN::ConvPlan>> plans_;
  size_t plan_live_ = 0, plan_peak_ = 0, plan_total_ = 0;
  std::vector<std::pair<void*, void*>> events_;  // hipEvent_t pairs of the trace
};

}  // namespace phantom
