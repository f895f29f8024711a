// dnn.h — the reference's privacy-preserving ML layer façade (include/dnn.cuh, src/dnn.cu) on this
// engine: TensorCT and the DNN members that encrypt a tensor, convolve it, and chain two
// convolutions (BatchNorm, Add).  Conv is the hoisted layer of host/conv2d.h instead of the
// reference's out_ch in_ch K^2 rotate / multiply / add steps (src/dnn.cu:82-150); EncTensor and
// DecTensor are one batched device call each.  AvgPoolFullCon is the hoisted layer of
// host/avgpool.h: the channels are mixed first and only the T outputs are pooled, where the reference
// pools every input channel by sequential key switches (src/dnn.cu:397-452).  Its row rotations are
// j width 4^slotstr slots, a whole row; the reference's width 2^slotstr 2^j (src/dnn.cu:334-338,
// :421) is a row step only for slotstr = 0, where both agree.
//
// BootStrap takes a pack: up to PackCapacity channels are interleaved into one ciphertext by monomial
// shifts, bootstrapped once at pack x ns slots and taken apart by a rotation tree (host/pack.h), where
// the reference bootstraps every channel on its own (src/dnn.cu:263-275, pack = 1 here).  Relu, Sign
// and ReluDegTwo are the reference's channel loops; ReluComposite its sequence with the three
// bootstrap loops going through BootStrap(.., pack).
//
// PrepareConvBN / ConvAdd fold the batch norm and the residual add of a residual block into the
// prepared convolution (one level instead of two; host/conv2d.h "fused affine terms").
//
// The weight loader is host/npy.h and the ResNet driver host/resnet.h.  Not built: SoftMax.
#pragma once

#include <cstdint>
#include <memory>
#include <vector>

#include "bootstrap.h"
#include "ciphertext.h"
#include "ckks_eval.h"
#include "context.h"
#include "encoder.h"
#include "keys.h"

namespace phantom {

struct ConvPlanData;  // host/conv2d.h

// one ciphertext per channel: a width_ x width_ image in (width_ 2^slotstr_)^2 sparse-packed slots,
// pixel (r, c) at slot (r width_ 2^slotstr_ + c) 2^slotstr_ (include/dnn.cuh:33-39)
struct TensorCT {
  std::vector<PhantomCiphertext> ctks_;
  size_t width_ = 0;
  size_t slotstr_ = 0;
  size_t num_ch_ = 0;
};

// groups of up to pack_ channels interleaved by monomial shifts (host/pack.h): channel c is member
// c % pack_ of ciphertext c / pack_
struct PackedCT {
  std::vector<PhantomCiphertext> ctks_;
  size_t width_ = 0;
  size_t slotstr_ = 0;
  size_t num_ch_ = 0;
  size_t pack_ = 1;
};

// batch-norm parameters, one entry per channel: y = a x + b with a = weight / sqrt(var + 1e-5),
// b = bias - a mean (DNN::BatchNorm)
struct BNParams {
  std::vector<double> weight, bias, mean, var;
};

class DNN {
 public:
  using Tensor3 = std::vector<std::vector<std::vector<double>>>;  // [width][width][channel]
  using Weight4 = std::vector<std::vector<std::vector<std::vector<double>>>>;  // [K][K][in_ch][out_ch]

  DNN(size_t scale, PhantomCKKSEncoder& encoder, const PhantomContext& context)
      : scale_(scale), context_(context), encoder_(encoder) {}

  void setScalingFactors(const std::vector<double>& scalingFactorsReal, const std::vector<double>& scalingFactorsRealBig) {
    m_scalingFactorsReal_ = scalingFactorsReal;
    m_scalingFactorsRealBig_ = scalingFactorsRealBig;
  }
  void RelinKeyGen(PhantomSecretKey& secret_key);
  // fused rotation keys (EvalRotateKeyGen) for the given slot rotations
  void BuildGaloisKey(PhantomSecretKey& secret_key, std::vector<int32_t>& rotation_indices);
  // ... for the K^2 taps of one layer geometry (src/dnn.cu:270-297)
  void ComputeRotationIndices(PhantomSecretKey& secret_key, size_t input_width, size_t kernel_h, size_t slotstr);
  // appends the taps' rotations that the list lacks (src/dnn.cu:299-319)
  void AddRotationIndicesTo(std::vector<int32_t>& rotation_indices, size_t input_width, size_t kernel_h, size_t slotstr);
  // what a caller needs to run its own steps beside the layers (examples/conv_example.cpp's baseline)
  const PhantomGaloisKeyFused& galois_keys() const { return gk_; }
  const std::vector<double>& scalingFactorsReal() const { return m_scalingFactorsReal_; }
  const std::vector<double>& scalingFactorsRealBig() const { return m_scalingFactorsRealBig_; }

  // encode_sparse at scale_ (src/dnn.cu:75-80); the encoder's sparse slot count is the caller's
  PhantomPlaintext PlainTextEncode(const std::vector<double>& input, size_t chain_index);
  // input[i][j][k] -> one ciphertext per channel at chain index 1 (src/dnn.cu:10-40): the slot
  // vectors are built channel-major, uploaded once and encrypted by one batched public-key call with
  // sparse_slots = (width 2^slotstr)^2 (the encoder is left set to that packing).  slotstr > 0
  // packs the pixels 2^slotstr slots apart, the layout a stride-2 layer leaves.
  TensorCT EncTensor(const Tensor3& input, PhantomPublicKey& pk, size_t slotstr = 0);
  // one batched decrypt + decode (src/dnn.cu:42-71)
  Tensor3 DecTensor(const TensorCT& enc_tensor, PhantomSecretKey& sk);

  // weight[a][b][k][h] (src/dnn.cu:82-150).  stride 1 or 2: stride 2 halves width_ and raises
  // slotstr_ by one, nothing else (:145-147).  The result is at the input's level with noise-scale
  // degree input + 1 and scale ct.scale * scale_; a degree-2 input is rescaled first, as
  // EvalMultAutoInplace does.  std::invalid_argument: mismatched channel counts, channels at
  // different levels, degrees or scales, a stride other than 1 or 2, a missing rotation key.
  TensorCT Conv(const TensorCT& input, const Weight4& weight, size_t stride);
  // the same with the weights already on the device: dev_W [K][K][in_ch][out_ch] doubles, complete
  // in the context's stream order
  TensorCT Conv(const TensorCT& input, const double* dev_W, size_t kernel_h, size_t out_ch, size_t stride);

  // A prepared layer: the weights of one layer geometry at one chain index, encoded once in the
  // compact subring form (host/conv2d.h) at scale_ and kept on the device.  Move-only; it must not
  // outlive the context, and no Conv using it may be in flight when it is destroyed.
  class ConvPlan {
   public:
    ConvPlan() = default;
    ConvPlan(ConvPlan&&) noexcept;
    ConvPlan& operator=(ConvPlan&&) noexcept;
    ~ConvPlan();
    size_t width() const;
    size_t slotstr() const;
    size_t kernel() const;
    size_t in_ch() const;
    size_t out_ch() const;
    size_t chain_index() const;
    double scale() const;
    size_t bytes() const;  // the plan's device size
    explicit operator bool() const { return data_ != nullptr; }

   private:
    friend class DNN;
    std::unique_ptr<ConvPlanData> data_;
  };
  // weight[a][b][k][h] for inputs of `width` x `width` pixels packed with `slotstr` at `chain_index`
  // (the level the layer's input has after the rescale a degree-2 input gets).  Waits for the
  // context's stream.
  ConvPlan PrepareConv(const Weight4& weight, size_t width, size_t slotstr, size_t chain_index);
  ConvPlan PrepareConv(const double* dev_W, size_t kernel_h, size_t in_ch, size_t out_ch, size_t width, size_t slotstr,
                       size_t chain_index);
  // Conv with the plan's weights: the metadata rules of Conv above, no encode.  std::invalid_argument
  // also when the plan's geometry, channel count or chain index differs from the input's (after the
  // rescale).  The result equals Conv(weight) up to the plaintexts' rounding: the compact encoding
  // rounds 2 ns coefficients, the full-size one N.
  TensorCT Conv(const TensorCT& input, const ConvPlan& plan, size_t stride);
  // A prepared layer with the batch norm behind it folded in: a_h multiplies output channel h's
  // weights in FP64 before they are encoded, and Conv(plan) adds the constant round(b_h S_out), S_out
  // the result's scale, to c0 inside the inner sum (host/conv2d.h "fused affine terms").
  // Conv(PrepareConvBN) therefore stands for BatchNorm(Conv(PrepareConv)) at the input's chain index,
  // one level above it.  std::invalid_argument: parameter vectors that are not out_ch long.
  ConvPlan PrepareConvBN(const Weight4& weight, const BNParams& bn, size_t width, size_t slotstr, size_t chain_index);
  ConvPlan PrepareConvBN(const double* dev_W, size_t kernel_h, size_t in_ch, size_t out_ch, const BNParams& bn,
                         size_t width, size_t slotstr, size_t chain_index);
  // Conv(input, plan, stride) + residual in the same launches: the residual enters the inner sum as
  // m residual_h with the integer m = llround(S_out / S_res), which has the result's scale up to a
  // relative 1 / (2 m).  The result's metadata is Conv(plan)'s: the input's chain index, degree
  // input + 1, scale ct.scale * scale_.  The residual's geometry must be the output's (width / stride,
  // slotstr + (stride == 2), out_ch channels); a degree-2 residual is rescaled first, one at an
  // earlier chain index than the layer's loses limbs (ModSwitchLevelInPlace).  std::invalid_argument:
  // what Conv(plan) refuses, another geometry, a residual at a later chain index or with channels at
  // different levels, degrees or scales, m below 2 or above 2^62.
  TensorCT ConvAdd(const TensorCT& input, const ConvPlan& plan, const TensorCT& residual, size_t stride);
  // per channel a x + b with a = weight / sqrt(var + 1e-5), b = bias - a mean (src/dnn.cu:454-480)
  TensorCT BatchNorm(const TensorCT& input, const std::vector<double>& weight, const std::vector<double>& bias,
                     const std::vector<double>& mean, const std::vector<double>& var);
  // channel-wise EvalAddAuto (src/dnn.cu:482-501)
  TensorCT Add(const TensorCT& a, const TensorCT& b);

  // appends the 2 (width - 1) pooling rotations that the list lacks (avgpool_rotations: every column
  // and row step, not the reference's doubling steps, src/dnn.cu:321-340)
  void AddAvgPoolRotationsTo(std::vector<int32_t>& rotation_indices, size_t input_width, size_t slotstr);
  // weight[u][k], u < T, k < t = num_ch_ (src/dnn.cu:397-452): out_u = sum_k weight[u][k] pool(in_k) +
  // bias[u] in every pixel's slot the pooling reaches (pixel (0, 0) holds the full sum); the 1 / width^2
  // of an average is the caller's to fold into the weights, as in the reference.  The coefficients
  // are GetElementForEvalMult's and the bias residues EvalAddConstInPlaceWrap's at the output's scale.
  // The result is at the input's level with noise-scale degree input + 1 and scale
  // ct.scale * sf[level]; a degree-2 input is rescaled first, as EvalMultConstInplace does; width_
  // and slotstr_ stay, num_ch_ = T.  std::invalid_argument: ragged or mismatched weights, channels at
  // different levels, degrees or scales, a missing rotation key.
  TensorCT AvgPoolFullCon(const TensorCT& input, const std::vector<std::vector<double>>& weight,
                          const std::vector<double>& bias);
  // the layer's first stage alone, out_u = sum_k weight[u][k] in_k in one launch (phx::ct_mix): equal
  // to the EvalMultConst / EvalAddAuto loop word for word, with the metadata rules above
  TensorCT MixChannels(const TensorCT& input, const std::vector<std::vector<double>>& weight);

  // ---- the packed tensor bootstrap and the activation layers ----
  // Every member below throws std::invalid_argument for channels at different levels, degrees or
  // scales, a pack that is no power of two or above PackCapacity, log2(pack) above the bootstrapper's
  // correction factor, k > 2, and a missing rotation key.
  // min(N / (2 ns), 64) with ns = (width 2^slotstr)^2: the channels one ciphertext can hold
  size_t PackCapacity(size_t width, size_t slotstr) const;
  // appends the tree's rotations {ns 2^i : i < log2 pack} that the list lacks
  void AddPackRotationsTo(std::vector<int32_t>& rotation_indices, size_t input_width, size_t slotstr, size_t pack);
  // ceil(num_ch / pack) ciphertexts sum_c X^((lead + c) D) ct_c, D = N / (2 pack ns): no key switch, no
  // level; level, degree and scale of the input.  lead = 0 for a full group and 1 otherwise: a group
  // with a free index leaves index 0 free, where a bootstrap's slot-0 offset lands (host/pack.h)
  PackedCT Pack(const TensorCT& input, size_t pack);
  // the rotation tree (pack - 1 key switches for a full group): level, degree and scale() of the packed
  // input; every channel's message is pack_ times the packed one's
  TensorCT Unpack(const PackedCT& packed);
  // how Unpack (and BootStrap / ReluComposite through it) walks the tree: kBatched takes every group's
  // tree level by level through unpack_channels_batch (one batched key switch per level), kPerNode
  // one EvalRotateFused per node through unpack_channels.  The outputs are the same words either way;
  // kBatched is the default: faster at each ResNet-20 stage ("Batched same-key rotations",
  // has the times of both), at a level's worth of scratch drawn from the pool at once.
  enum class UnpackPath { kBatched, kPerNode };
  void set_unpack_path(UnpackPath p) { unpack_path_ = p; }
  UnpackPath unpack_path() const { return unpack_path_; }
  // pack = 1: every channel through EvalBootstrapBatch at ns slots (src/dnn.cu:263-275).  pack = P > 1:
  // rescale a degree-2 input, Pack, EvalBootstrapBatch of the groups at P ns slots with
  // post_shift = log2 P (the tree's factor P is taken out of the bootstrap's closing integer: no
  // precision, no level), Unpack.  The result has the level EvalBootstrap returns for P ns slots,
  // degree 1 and its scale.  The bootstrapper must be set up and keyed for P ns slots, and the
  // model's Galois key must hold the pack rotations (AddPackRotationsTo).
  TensorCT BootStrap(TensorCT& input, FHECKKSRNS& bootstrapper, size_t pack = 1);
  // EvalChebyshevSeries of max(0, x) on [a, b] per channel (src/dnn.cu:152-168)
  TensorCT Relu(const TensorCT& input, const PhantomRelinKey& relin_keys, int a = -1, int b = 1, int deg = 7);
  // stage k <= 2 of the composite sign approximation per channel (src/dnn.cu:170-191)
  TensorCT Sign(const TensorCT& input, const PhantomRelinKey& relin_keys, size_t k);
  static const std::vector<double>& SignCoefficients(size_t k);  // the stage's series, c_0 not halved
  static double SignInterval(size_t k);                         // its interval is [-v, v]
  // x + x^2 per channel (src/dnn.cu:247-261)
  TensorCT ReluDegTwo(const TensorCT& input, const PhantomRelinKey& relin_keys);
  // 0.5 x (1 + sign(0.1 x)) with the three sign stages, a bootstrap after the first two and at the end
  // (src/dnn.cu:193-243), each through BootStrap(.., pack); uses the model's RelinKeyGen key
  TensorCT ReluComposite(const TensorCT& input, FHECKKSRNS& bootstrapper, size_t pack = 1);

 private:
  void check_uniform(const TensorCT& input, const char* who) const;
  // the layer on dev_W (conv2d_raw), or on `plan` when it is not null (conv2d_apply, with the plan's
  // shift and, when not null, the residual)
  TensorCT conv_run(const TensorCT& input, const double* dev_W, const ConvPlanData* plan, size_t kernel_h, size_t out_ch,
                    size_t stride, const TensorCT* residual = nullptr);
  static std::vector<double> flatten_weight(const Weight4& weight, size_t& K, size_t& in_ch, size_t& out_ch,
                                            const char* who);
  // the checks, the rescale of a degree-2 input and the coefficient residues [T][t][L] that
  // AvgPoolFullCon and MixChannels share; `rescaled` holds the channels to read when the input was
  // of degree 2 (else it stays empty and the input's are read), `result` the outputs with their
  // metadata set
  std::vector<uint64_t> mix_setup(const TensorCT& input, const std::vector<std::vector<double>>& weight, const char* who,
                                  std::vector<PhantomCiphertext>& rescaled, TensorCT& result);

  size_t scale_;
  PhantomGaloisKeyFused gk_;
  UnpackPath unpack_path_ = UnpackPath::kBatched;
  const PhantomContext& context_;
  PhantomCKKSEncoder& encoder_;
  std::vector<double> m_scalingFactorsReal_;
  std::vector<double> m_scalingFactorsRealBig_;
  PhantomRelinKey mul_key_;
};

}  // namespace phantom
