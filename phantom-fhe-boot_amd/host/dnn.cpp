// dnn.cpp — see dnn.h
#include "dnn.h"

#include <algorithm>
#include <cmath>
#include <complex>
#include <stdexcept>
#include <string>
#include <unordered_set>

#include "avgpool.h"
#include "buffer.h"
#include "conv2d.h"
#include "hip_check.h"
#include "pack.h"

namespace phantom {

using cplx = std::complex<double>;

void DNN::RelinKeyGen(PhantomSecretKey& secret_key) { mul_key_ = secret_key.gen_relinkey(context_); }

void DNN::BuildGaloisKey(PhantomSecretKey& secret_key, std::vector<int32_t>& rotation_indices) {
  gk_ = secret_key.EvalRotateKeyGen(context_, rotation_indices);
}

void DNN::AddRotationIndicesTo(std::vector<int32_t>& rotation_indices, size_t input_width, size_t kernel_h,
                               size_t slotstr) {
  std::unordered_set<int32_t> existing(rotation_indices.begin(), rotation_indices.end());
  for (int r : conv_rotations(input_width, slotstr, kernel_h))
    if (existing.insert(r).second) rotation_indices.push_back(r);
}

void DNN::ComputeRotationIndices(PhantomSecretKey& secret_key, size_t input_width, size_t kernel_h, size_t slotstr) {
  std::vector<int32_t> idx;
  AddRotationIndicesTo(idx, input_width, kernel_h, slotstr);
  BuildGaloisKey(secret_key, idx);
}

PhantomPlaintext DNN::PlainTextEncode(const std::vector<double>& input, size_t chain_index) {
  PhantomPlaintext x_plain;
  encoder_.encode_sparse(context_, input, static_cast<double>(scale_), x_plain, chain_index);
  return x_plain;
}

TensorCT DNN::EncTensor(const Tensor3& input, PhantomPublicKey& pk, size_t slotstr) {
  if (input.empty() || input[0].size() != input.size() || input[0][0].empty())
    throw std::invalid_argument("EncTensor: input must be [width][width][channels]");
  TensorCT result;
  result.width_ = input.size();
  result.num_ch_ = input[0][0].size();
  result.slotstr_ = slotstr;
  const size_t width = result.width_, ch = result.num_ch_;
  const phx::ConvShape shape = conv_shape(context_.poly_degree(), width, slotstr, 1, ch, 1);
  const size_t lg = shape.large(), ns = shape.slots(), pw = size_t(1) << slotstr;
  std::vector<cplx> values(ch * ns, cplx(0.0, 0.0));
  for (size_t i = 0; i < width; ++i) {
    if (input[i].size() != width) throw std::invalid_argument("EncTensor: input must be [width][width][channels]");
    for (size_t j = 0; j < width; ++j) {
      if (input[i][j].size() != ch) throw std::invalid_argument("EncTensor: ragged channels");
      for (size_t k = 0; k < ch; ++k) values[k * ns + (i * lg + j) * pw] = input[i][j][k];
    }
  }
  DeviceBuffer<cplx> dv;
  dv.upload(values, context_.stream());
  encoder_.set_sparse_encode(2 * ns);
  result.ctks_.resize(ch);
  pk.encrypt_asymmetric_sparse_batch(context_, encoder_, dv.get(), ns, static_cast<double>(scale_), 1, result.ctks_);
  return result;
}

DNN::Tensor3 DNN::DecTensor(const TensorCT& t, PhantomSecretKey& sk) {
  const size_t width = t.width_, ch = t.num_ch_;
  if (ch == 0 || t.ctks_.size() != ch) throw std::invalid_argument("DecTensor: channel count mismatch");
  const phx::ConvShape shape = conv_shape(context_.poly_degree(), width, t.slotstr_, 1, ch, 1);
  const size_t lg = shape.large(), pw = size_t(1) << t.slotstr_, slots = encoder_.slot_count();
  DeviceBuffer<cplx> dv(ch * slots, context_.stream());
  sk.decrypt_decode_batch(context_, encoder_, t.ctks_, 0, dv.get());
  // sparse packing repeats the (width 2^slotstr)^2 values in every block: the first block is read
  const std::vector<cplx> v = dv.download(context_.stream());
  Tensor3 out(width, std::vector<std::vector<double>>(width, std::vector<double>(ch)));
  for (size_t k = 0; k < ch; ++k)
    for (size_t i = 0; i < width; ++i)
      for (size_t j = 0; j < width; ++j) out[i][j][k] = v[k * slots + (i * lg + j) * pw].real();
  return out;
}

std::vector<double> DNN::flatten_weight(const Weight4& weight, size_t& K, size_t& in_ch, size_t& out_ch,
                                        const char* who) {
  const std::string name(who);
  if (weight.empty() || weight[0].size() != weight.size() || weight[0][0].empty() || weight[0][0][0].empty())
    throw std::invalid_argument(name + ": weight must be [K][K][in_ch][out_ch]");
  K = weight.size(), in_ch = weight[0][0].size(), out_ch = weight[0][0][0].size();
  std::vector<double> w(K * K * in_ch * out_ch);
  for (size_t a = 0; a < K; ++a) {
    if (weight[a].size() != K) throw std::invalid_argument(name + ": weight must be [K][K][in_ch][out_ch]");
    for (size_t b = 0; b < K; ++b) {
      if (weight[a][b].size() != in_ch) throw std::invalid_argument(name + ": ragged weight");
      for (size_t k = 0; k < in_ch; ++k) {
        if (weight[a][b][k].size() != out_ch) throw std::invalid_argument(name + ": ragged weight");
        for (size_t h = 0; h < out_ch; ++h) w[((a * K + b) * in_ch + k) * out_ch + h] = weight[a][b][k][h];
      }
    }
  }
  return w;
}

TensorCT DNN::Conv(const TensorCT& input, const Weight4& weight, size_t stride) {
  size_t K, in_ch, out_ch;
  const std::vector<double> w = flatten_weight(weight, K, in_ch, out_ch, "Conv");
  if (in_ch != input.num_ch_) throw std::invalid_argument("Conv: the weight's input channels differ from the tensor's");
  DeviceBuffer<double> dW;
  dW.upload(w, context_.stream());
  return Conv(input, dW.get(), K, out_ch, stride);
}

TensorCT DNN::Conv(const TensorCT& input, const double* dev_W, size_t kernel_h, size_t out_ch, size_t stride) {
  return conv_run(input, dev_W, nullptr, kernel_h, out_ch, stride);
}

DNN::ConvPlan::ConvPlan(ConvPlan&&) noexcept = default;
DNN::ConvPlan& DNN::ConvPlan::operator=(ConvPlan&&) noexcept = default;
DNN::ConvPlan::~ConvPlan() = default;
size_t DNN::ConvPlan::width() const { return data_->shape.width; }
size_t DNN::ConvPlan::slotstr() const { return data_->shape.slotstr; }
size_t DNN::ConvPlan::kernel() const { return data_->shape.kernel; }
size_t DNN::ConvPlan::in_ch() const { return data_->shape.in_ch; }
size_t DNN::ConvPlan::out_ch() const { return data_->shape.out_ch; }
size_t DNN::ConvPlan::chain_index() const { return data_->chain_index; }
double DNN::ConvPlan::scale() const { return data_->scale; }
size_t DNN::ConvPlan::bytes() const { return data_->bytes(); }

DNN::ConvPlan DNN::PrepareConv(const Weight4& weight, size_t width, size_t slotstr, size_t chain_index) {
  size_t K, in_ch, out_ch;
  const std::vector<double> w = flatten_weight(weight, K, in_ch, out_ch, "PrepareConv");
  DeviceBuffer<double> dW;
  dW.upload(w, context_.stream());
  return PrepareConv(dW.get(), K, in_ch, out_ch, width, slotstr, chain_index);
}

DNN::ConvPlan DNN::PrepareConv(const double* dev_W, size_t kernel_h, size_t in_ch, size_t out_ch, size_t width,
                               size_t slotstr, size_t chain_index) {
  if (!dev_W) throw std::invalid_argument("PrepareConv: null weights");
  const phx::ConvShape shape = conv_shape(context_.poly_degree(), width, slotstr, kernel_h, in_ch, out_ch);
  hipStream_t s = context_.stream();
  DeviceBuffer<int> flag(1, s);
  PHX_CHECK(hipMemsetAsync(flag.get(), 0, sizeof(int), s));
  ConvPlan plan;
  plan.data_ = conv2d_prepare(context_, chain_index, shape, dev_W, static_cast<double>(scale_), flag.get(), s);
  if (flag.download(s)[0]) throw std::invalid_argument("PrepareConv: encoded weights are too large");
  return plan;
}

DNN::ConvPlan DNN::PrepareConvBN(const Weight4& weight, const BNParams& bn, size_t width, size_t slotstr,
                                 size_t chain_index) {
  size_t K, in_ch, out_ch;
  const std::vector<double> w = flatten_weight(weight, K, in_ch, out_ch, "PrepareConvBN");
  DeviceBuffer<double> dW;
  dW.upload(w, context_.stream());
  return PrepareConvBN(dW.get(), K, in_ch, out_ch, bn, width, slotstr, chain_index);
}

DNN::ConvPlan DNN::PrepareConvBN(const double* dev_W, size_t kernel_h, size_t in_ch, size_t out_ch, const BNParams& bn,
                                 size_t width, size_t slotstr, size_t chain_index) {
  if (!dev_W) throw std::invalid_argument("PrepareConvBN: null weights");
  if (bn.weight.size() != out_ch || bn.bias.size() != out_ch || bn.mean.size() != out_ch || bn.var.size() != out_ch)
    throw std::invalid_argument("PrepareConvBN: one weight, bias, mean and variance per output channel");
  const phx::ConvShape shape = conv_shape(context_.poly_degree(), width, slotstr, kernel_h, in_ch, out_ch);
  const double eps = 1e-5;  // BatchNorm's
  std::vector<double> a(out_ch), b(out_ch);
  for (size_t h = 0; h < out_ch; ++h) {
    a[h] = bn.weight[h] / std::sqrt(bn.var[h] + eps);
    b[h] = bn.bias[h] - a[h] * bn.mean[h];
    if (!std::isfinite(a[h]) || !std::isfinite(b[h]))
      throw std::invalid_argument("PrepareConvBN: a batch-norm parameter is not finite");
  }
  hipStream_t s = context_.stream();
  DeviceBuffer<int> flag(1, s);
  PHX_CHECK(hipMemsetAsync(flag.get(), 0, sizeof(int), s));
  ConvPlan plan;
  plan.data_ = conv2d_prepare(context_, chain_index, shape, dev_W, static_cast<double>(scale_), flag.get(), s, a.data());
  if (flag.download(s)[0]) throw std::invalid_argument("PrepareConvBN: encoded weights are too large");
  plan.data_->shift = std::move(b);
  return plan;
}

TensorCT DNN::Conv(const TensorCT& input, const ConvPlan& plan, size_t stride) {
  if (!plan) throw std::invalid_argument("Conv: empty plan");
  return conv_run(input, nullptr, plan.data_.get(), plan.kernel(), plan.out_ch(), stride);
}

TensorCT DNN::ConvAdd(const TensorCT& input, const ConvPlan& plan, const TensorCT& residual, size_t stride) {
  if (!plan) throw std::invalid_argument("ConvAdd: empty plan");
  return conv_run(input, nullptr, plan.data_.get(), plan.kernel(), plan.out_ch(), stride, &residual);
}

TensorCT DNN::conv_run(const TensorCT& input, const double* dev_W, const ConvPlanData* plan, size_t kernel_h,
                       size_t out_ch, size_t stride, const TensorCT* residual) {
  if (stride != 1 && stride != 2) throw std::invalid_argument("Conv: stride must be 1 or 2");
  const size_t in_ch = input.num_ch_, n = context_.poly_degree();
  if (in_ch == 0 || input.ctks_.size() != in_ch) throw std::invalid_argument("Conv: channel count mismatch");
  if (!dev_W && !plan) throw std::invalid_argument("Conv: null weights");
  const PhantomCiphertext& first = input.ctks_[0];
  for (const PhantomCiphertext& c : input.ctks_)
    if (c.size() != 2 || c.chain_index() != first.chain_index() || c.scale() != first.scale() ||
        c.GetNoiseScaleDeg() != first.GetNoiseScaleDeg())
      throw std::invalid_argument("Conv: the channels must share level, noise-scale degree and scale");
  const phx::ConvShape shape = conv_shape(n, input.width_, input.slotstr_, kernel_h, in_ch, out_ch);
  // a degree-2 input is rescaled first (EvalMultAutoInplace, src/evaluate.cu:2813-2825)
  std::vector<PhantomCiphertext> rescaled;
  if (first.GetNoiseScaleDeg() == 2) {
    rescaled = input.ctks_;
    for (PhantomCiphertext& c : rescaled) EvalModReduceInPlace(context_, c, 1);
  }
  const std::vector<PhantomCiphertext>& in = rescaled.empty() ? input.ctks_ : rescaled;
  const size_t chain = in[0].chain_index();
  if (plan) {
    const phx::ConvShape& p = plan->shape;
    if (plan->ctx != &context_) throw std::invalid_argument("Conv: the plan was prepared for another context");
    if (p.width != input.width_ || p.slotstr != input.slotstr_ || p.in_ch != in_ch)
      throw std::invalid_argument("Conv: the plan's geometry or channel count differs from the tensor's");
    if (plan->chain_index != chain)
      throw std::invalid_argument("Conv: the plan was prepared at another chain index than the input's");
  }

  const std::vector<int> rots = conv_rotations(input.width_, input.slotstr_, kernel_h);
  std::vector<const uint64_t* const*> evk(rots.size(), nullptr);
  std::vector<uint32_t> elts(rots.size(), 1);
  for (size_t t = 0; t < rots.size(); ++t) {
    if (rots[t] == 0) continue;  // the centre tap
    elts[t] = FindAutomorphismIndex2nComplex(rots[t], n);
    if (!gk_.has(elts[t])) throw std::invalid_argument("Conv: no rotation key for a tap (ComputeRotationIndices)");
    evk[t] = gk_.get(elts[t]).public_keys_ptr();
  }

  TensorCT result;
  result.width_ = input.width_ / stride;
  result.num_ch_ = out_ch;
  result.slotstr_ = stride == 2 ? input.slotstr_ + 1 : input.slotstr_;
  const double out_scale = in[0].scale() * static_cast<double>(scale_);

  // the fused affine terms of a prepared layer (host/conv2d.h), checked before the layer is enqueued
  const size_t Ql = in[0].coeff_modulus_size();
  const auto& mods = context_.get_context_data(chain).moduli();
  std::vector<uint64_t> bias, res_mult;
  std::vector<PhantomCiphertext> res_adj;
  std::vector<const uint64_t*> res;
  if (residual) {
    if (!plan) throw std::invalid_argument("ConvAdd: needs a prepared layer");
    if (residual->width_ != result.width_ || residual->slotstr_ != result.slotstr_ || residual->num_ch_ != out_ch)
      throw std::invalid_argument("ConvAdd: the residual's geometry or channel count differs from the output's");
    check_uniform(*residual, "ConvAdd");
    const PhantomCiphertext& r0 = residual->ctks_[0];
    const size_t res_chain = r0.chain_index() + (r0.GetNoiseScaleDeg() == 2 ? 1 : 0);
    if (r0.GetNoiseScaleDeg() > 2) throw std::invalid_argument("ConvAdd: the residual's noise-scale degree exceeds 2");
    if (res_chain > chain) throw std::invalid_argument("ConvAdd: the residual is at a later chain index than the layer");
    if (r0.GetNoiseScaleDeg() == 2 || res_chain < chain) {
      res_adj = residual->ctks_;
      for (PhantomCiphertext& c : res_adj) {
        if (c.GetNoiseScaleDeg() == 2) EvalModReduceInPlace(context_, c, 1);
        if (c.chain_index() < chain) ModSwitchLevelInPlace(context_, c, chain - c.chain_index());
      }
    }
    const std::vector<PhantomCiphertext>& rc = res_adj.empty() ? residual->ctks_ : res_adj;
    const double ratio = out_scale / rc[0].scale();
    if (!(ratio >= 1.5) || !(ratio <= 0x1p62))
      throw std::invalid_argument("ConvAdd: the output's scale must be 2 to 2^62 times the residual's");
    const uint64_t m = static_cast<uint64_t>(std::llround(ratio));
    res_mult.resize(Ql);
    for (size_t l = 0; l < Ql; ++l) res_mult[l] = m % mods[l];
    res.resize(out_ch);
    for (size_t h = 0; h < out_ch; ++h) res[h] = rc[h].data();
  }
  if (plan && !plan->shift.empty()) {
    if (plan->shift.size() != out_ch) throw std::invalid_argument("Conv: the plan's shifts differ from its output channels");
    bias.resize(out_ch * Ql);
    for (size_t h = 0; h < out_ch; ++h) {
      const std::vector<uint64_t> r = scaled_constant_residues(plan->shift[h], out_scale, mods.data(), Ql);
      std::copy(r.begin(), r.end(), bias.begin() + h * Ql);
    }
  }

  result.ctks_.resize(out_ch);
  hipStream_t s = context_.stream();
  std::vector<const uint64_t*> cts(in_ch);
  std::vector<uint64_t*> outs(out_ch);
  for (size_t k = 0; k < in_ch; ++k) cts[k] = in[k].data();
  for (size_t h = 0; h < out_ch; ++h) {
    PhantomCiphertext& o = result.ctks_[h];
    o.resize(context_, chain, 2, s, false);
    o.set_ntt_form(true);
    o.set_scale(out_scale);
    o.SetNoiseScaleDeg(in[0].GetNoiseScaleDeg() + 1);
    o.set_correction_factor(in[0].correction_factor());
    o.set_asymmetric(in[0].is_asymmetric());
    outs[h] = o.data();
  }
  if (plan) {
    conv2d_apply(context_, *plan, cts.data(), evk.data(), elts.data(), outs.data(), s, res.empty() ? nullptr : res.data(),
                 res_mult.empty() ? nullptr : res_mult.data(), bias.empty() ? nullptr : bias.data());
  } else {
    encoder_.set_sparse_encode(2 * shape.slots());
    conv2d_raw(context_, chain, cts.data(), shape, dev_W, static_cast<double>(scale_), evk.data(), elts.data(), 0,
               outs.data(), nullptr, s);
  }
  return result;
}

TensorCT DNN::BatchNorm(const TensorCT& input, const std::vector<double>& weight, const std::vector<double>& bias,
                        const std::vector<double>& mean, const std::vector<double>& var) {
  const size_t ch = input.num_ch_;
  if (input.ctks_.size() != ch || weight.size() != ch || bias.size() != ch || mean.size() != ch || var.size() != ch)
    throw std::invalid_argument("BatchNorm: one weight, bias, mean and variance per channel");
  const double eps = 1e-5;
  TensorCT output;
  output.ctks_.resize(ch);
  output.width_ = input.width_;
  output.num_ch_ = ch;
  output.slotstr_ = input.slotstr_;
  for (size_t c = 0; c < ch; ++c) {
    const double a = weight[c] / std::sqrt(var[c] + eps);
    const double b = bias[c] - a * mean[c];
    output.ctks_[c] = EvalMultConst(context_, input.ctks_[c], a, m_scalingFactorsReal_);
    EvalAddConstInPlaceWrap(context_, output.ctks_[c], b, m_scalingFactorsReal_, m_scalingFactorsRealBig_);
  }
  return output;
}

TensorCT DNN::Add(const TensorCT& a, const TensorCT& b) {
  if (a.num_ch_ != b.num_ch_ || a.width_ != b.width_ || a.slotstr_ != b.slotstr_ || a.ctks_.size() != a.num_ch_ ||
      b.ctks_.size() != b.num_ch_)
    throw std::invalid_argument("TensorCT dimension mismatch in Add()");
  TensorCT result;
  result.num_ch_ = a.num_ch_;
  result.width_ = a.width_;
  result.slotstr_ = a.slotstr_;
  result.ctks_.resize(a.num_ch_);
  for (size_t u = 0; u < a.num_ch_; ++u)
    result.ctks_[u] = EvalAddAuto(context_, a.ctks_[u], b.ctks_[u], m_scalingFactorsReal_, m_scalingFactorsRealBig_);
  return result;
}

void DNN::AddAvgPoolRotationsTo(std::vector<int32_t>& rotation_indices, size_t input_width, size_t slotstr) {
  avgpool_shape(context_.poly_degree(), input_width, slotstr);
  std::unordered_set<int32_t> existing(rotation_indices.begin(), rotation_indices.end());
  for (int r : avgpool_rotations(input_width, slotstr))
    if (existing.insert(r).second) rotation_indices.push_back(r);
}

std::vector<uint64_t> DNN::mix_setup(const TensorCT& input, const std::vector<std::vector<double>>& weight,
                                     const char* who, std::vector<PhantomCiphertext>& rescaled, TensorCT& result) {
  const std::string name(who);
  const size_t t = input.num_ch_, T = weight.size();
  if (t == 0 || input.ctks_.size() != t) throw std::invalid_argument(name + ": channel count mismatch");
  if (T == 0) throw std::invalid_argument(name + ": weight must be [T][t]");
  for (const std::vector<double>& row : weight)
    if (row.size() != t) throw std::invalid_argument(name + ": ragged weight, or its columns differ from the tensor's channels");
  const PhantomCiphertext& first = input.ctks_[0];
  for (const PhantomCiphertext& c : input.ctks_)
    if (c.size() != 2 || c.chain_index() != first.chain_index() || c.scale() != first.scale() ||
        c.GetNoiseScaleDeg() != first.GetNoiseScaleDeg())
      throw std::invalid_argument(name + ": the channels must share level, noise-scale degree and scale");
  // a degree-2 input is rescaled first (EvalMultConstInplace, include/evaluate.cuh:317-326)
  if (first.GetNoiseScaleDeg() == 2) {
    rescaled = input.ctks_;
    for (PhantomCiphertext& c : rescaled) EvalModReduceInPlace(context_, c, 1);
  }
  const PhantomCiphertext& in0 = rescaled.empty() ? first : rescaled[0];
  const size_t chain = in0.chain_index(), L = in0.coeff_modulus_size();
  std::vector<uint64_t> coef(T * t * L);
  for (size_t u = 0; u < T; ++u)
    for (size_t k = 0; k < t; ++k) {
      const std::vector<uint64_t> r = GetElementForEvalMult(context_, in0, weight[u][k], m_scalingFactorsReal_);
      std::copy(r.begin(), r.begin() + L, coef.begin() + (u * t + k) * L);
    }
  result.width_ = input.width_;
  result.slotstr_ = input.slotstr_;
  result.num_ch_ = T;
  result.ctks_.resize(T);
  for (PhantomCiphertext& o : result.ctks_) {
    o.resize(context_, chain, 2, context_.stream(), false);
    o.set_ntt_form(true);
    o.set_scale(in0.scale() * m_scalingFactorsReal_.at(level_of(in0)));  // EvalMultConstInplaceCore
    o.SetNoiseScaleDeg(in0.GetNoiseScaleDeg() + 1);
    o.set_correction_factor(in0.correction_factor());
    o.set_asymmetric(in0.is_asymmetric());
  }
  return coef;
}

TensorCT DNN::MixChannels(const TensorCT& input, const std::vector<std::vector<double>>& weight) {
  std::vector<PhantomCiphertext> rescaled;
  TensorCT result;
  const std::vector<uint64_t> coef = mix_setup(input, weight, "MixChannels", rescaled, result);
  const std::vector<PhantomCiphertext>& in = rescaled.empty() ? input.ctks_ : rescaled;
  const size_t t = in.size(), T = result.num_ch_, chain = in[0].chain_index();
  std::vector<const uint64_t*> cts(t);
  std::vector<uint64_t*> outs(T);
  for (size_t k = 0; k < t; ++k) cts[k] = in[k].data();
  for (size_t u = 0; u < T; ++u) outs[u] = result.ctks_[u].data();
  hipStream_t s = context_.stream();
  DeviceBuffer<uint64_t> table(mix_table_words(t, T, in[0].coeff_modulus_size()), s);
  ct_mix_raw(context_, chain, cts.data(), t, coef.data(), nullptr, outs.data(), T, table.get(), s);
  return result;
}

TensorCT DNN::AvgPoolFullCon(const TensorCT& input, const std::vector<std::vector<double>>& weight,
                             const std::vector<double>& bias) {
  if (bias.size() != weight.size()) throw std::invalid_argument("AvgPoolFullCon: one bias per weight row");
  const size_t n = context_.poly_degree(), width = input.width_;
  avgpool_shape(n, width, input.slotstr_);
  const std::vector<int> rots = avgpool_rotations(width, input.slotstr_);
  std::vector<const uint64_t* const*> evk(rots.size());
  std::vector<uint32_t> elts(rots.size());
  for (size_t i = 0; i < rots.size(); ++i) {
    elts[i] = FindAutomorphismIndex2nComplex(rots[i], n);
    if (!gk_.has(elts[i])) throw std::invalid_argument("AvgPoolFullCon: no rotation key for a step (AddAvgPoolRotationsTo)");
    evk[i] = gk_.get(elts[i]).public_keys_ptr();
  }
  std::vector<PhantomCiphertext> rescaled;
  TensorCT result;
  const std::vector<uint64_t> coef = mix_setup(input, weight, "AvgPoolFullCon", rescaled, result);
  const std::vector<PhantomCiphertext>& in = rescaled.empty() ? input.ctks_ : rescaled;
  const size_t t = in.size(), T = result.num_ch_, chain = in[0].chain_index(), L = in[0].coeff_modulus_size();
  // the bias residues of EvalAddConstInPlaceWrap at the output's level, degree and scale
  const auto& mods = context_.get_context_data(chain).moduli();
  std::vector<uint64_t> bres(T * L, 0);
  for (size_t u = 0; u < T; ++u) {
    if (bias[u] == 0) continue;
    const std::vector<uint64_t> r = GetElementForEvalAddOrSub(context_, result.ctks_[u], std::fabs(bias[u]),
                                                              m_scalingFactorsReal_, m_scalingFactorsRealBig_);
    for (size_t l = 0; l < L; ++l) bres[u * L + l] = bias[u] > 0 ? r[l] : (r[l] ? mods[l] - r[l] : 0);
  }
  std::vector<const uint64_t*> cts(t);
  std::vector<uint64_t*> outs(T);
  for (size_t k = 0; k < t; ++k) cts[k] = in[k].data();
  for (size_t u = 0; u < T; ++u) outs[u] = result.ctks_[u].data();
  const size_t R = width - 1;
  avgpool_fc_raw(context_, chain, cts.data(), t, T, width, input.slotstr_, coef.data(), bres.data(), evk.data(),
                 evk.data() + R, elts.data(), elts.data() + R, outs.data(), context_.stream());
  return result;
}

void DNN::check_uniform(const TensorCT& input, const char* who) const {
  const std::string name(who);
  if (input.num_ch_ == 0 || input.ctks_.size() != input.num_ch_) throw std::invalid_argument(name + ": channel count mismatch");
  const PhantomCiphertext& first = input.ctks_[0];
  for (const PhantomCiphertext& c : input.ctks_)
    if (c.size() != 2 || c.chain_index() != first.chain_index() || c.scale() != first.scale() ||
        c.GetNoiseScaleDeg() != first.GetNoiseScaleDeg())
      throw std::invalid_argument(name + ": the channels must share level, noise-scale degree and scale");
}

size_t DNN::PackCapacity(size_t width, size_t slotstr) const {
  return pack_capacity(context_.poly_degree(), width, slotstr);
}

void DNN::AddPackRotationsTo(std::vector<int32_t>& rotation_indices, size_t input_width, size_t slotstr, size_t pack) {
  const PackPlan plan = pack_plan(context_.poly_degree(), input_width, slotstr, pack);
  std::unordered_set<int32_t> existing(rotation_indices.begin(), rotation_indices.end());
  for (int r : plan.rotations)
    if (existing.insert(r).second) rotation_indices.push_back(r);
}

PackedCT DNN::Pack(const TensorCT& input, size_t pack) {
  const PackPlan plan = pack_plan(context_.poly_degree(), input.width_, input.slotstr_, pack);
  check_uniform(input, "Pack");
  PackedCT out;
  out.width_ = input.width_;
  out.slotstr_ = input.slotstr_;
  out.num_ch_ = input.num_ch_;
  out.pack_ = pack;
  for (size_t grp = 0; grp < plan.groups(input.num_ch_); ++grp) {
    std::vector<const PhantomCiphertext*> members(plan.members(input.num_ch_, grp));
    for (size_t c = 0; c < members.size(); ++c) members[c] = &input.ctks_[grp * pack + c];
    out.ctks_.push_back(pack_channels(context_, plan, members.data(), members.size()));
  }
  return out;
}

TensorCT DNN::Unpack(const PackedCT& packed) {
  const PackPlan plan = pack_plan(context_.poly_degree(), packed.width_, packed.slotstr_, packed.pack_);
  if (packed.num_ch_ == 0 || packed.ctks_.size() != plan.groups(packed.num_ch_))
    throw std::invalid_argument("Unpack: group count mismatch");
  for (const PhantomCiphertext& c : packed.ctks_)
    if (c.size() != 2 || c.chain_index() != packed.ctks_[0].chain_index() || c.scale() != packed.ctks_[0].scale() ||
        c.GetNoiseScaleDeg() != packed.ctks_[0].GetNoiseScaleDeg())
      throw std::invalid_argument("Unpack: the groups must share level, noise-scale degree and scale");
  for (uint32_t e : plan.galois)
    if (!gk_.has(e)) throw std::invalid_argument("Unpack: no rotation key for a tree level (AddPackRotationsTo)");
  TensorCT out;
  out.width_ = packed.width_;
  out.slotstr_ = packed.slotstr_;
  out.num_ch_ = packed.num_ch_;
  if (unpack_path_ == UnpackPath::kPerNode) {
    for (size_t grp = 0; grp < packed.ctks_.size(); ++grp)
      for (PhantomCiphertext& c : unpack_channels(context_, plan, packed.ctks_[grp], plan.members(packed.num_ch_, grp), gk_))
        out.ctks_.push_back(std::move(c));
    return out;
  }
  // every group's tree level by level, one batched rotation per level (host/pack.h): the same words
  std::vector<const PhantomCiphertext*> groups(packed.ctks_.size());
  std::vector<size_t> members(packed.ctks_.size());
  for (size_t grp = 0; grp < packed.ctks_.size(); ++grp) {
    groups[grp] = &packed.ctks_[grp];
    members[grp] = plan.members(packed.num_ch_, grp);
  }
  for (std::vector<PhantomCiphertext>& g : unpack_channels_batch(context_, plan, groups, members, gk_))
    for (PhantomCiphertext& c : g) out.ctks_.push_back(std::move(c));
  return out;
}

TensorCT DNN::BootStrap(TensorCT& input, FHECKKSRNS& bootstrapper, size_t pack) {
  const PackPlan plan = pack_plan(context_.poly_degree(), input.width_, input.slotstr_, pack);
  check_uniform(input, "BootStrap");
  if (plan.log_pack > bootstrapper.correction_factor())
    throw std::invalid_argument("BootStrap: log2(pack) exceeds the bootstrapper's correction factor");
  const uint32_t slots = static_cast<uint32_t>(plan.slots());
  if (pack == 1) {
    TensorCT result;
    result.ctks_ = bootstrapper.EvalBootstrapBatch(input.ctks_, context_, 1, slots);
    result.width_ = input.width_;
    result.num_ch_ = input.num_ch_;
    result.slotstr_ = input.slotstr_;
    return result;
  }
  for (uint32_t e : plan.galois)
    if (!gk_.has(e)) throw std::invalid_argument("BootStrap: no rotation key for a tree level (AddPackRotationsTo)");
  // a degree-2 input is rescaled first, as the bootstrap does (RaiseWithCorrection)
  TensorCT rescaled;
  if (input.ctks_[0].GetNoiseScaleDeg() == 2) {
    rescaled = input;
    for (PhantomCiphertext& c : rescaled.ctks_) EvalModReduceInPlace(context_, c, 1);
  }
  PackedCT packed = Pack(rescaled.ctks_.empty() ? input : rescaled, pack);
  packed.ctks_ = bootstrapper.EvalBootstrapBatch(packed.ctks_, context_, 1, slots, FHECKKSRNS::kBootGroup,
                                                 static_cast<uint32_t>(plan.log_pack));
  return Unpack(packed);
}

TensorCT DNN::Relu(const TensorCT& input, const PhantomRelinKey& relin_keys, int a, int b, int deg) {
  check_uniform(input, "Relu");
  if (deg < 1 || a >= b) throw std::invalid_argument("Relu: a < b and a degree of at least 1");
  const std::vector<double> coefficients =
      EvalChebyshevCoefficients([](double x) { return std::max(0.0, x); }, a, b, static_cast<uint32_t>(deg));
  TensorCT result;
  for (const PhantomCiphertext& c : input.ctks_)
    result.ctks_.push_back(
        EvalChebyshevSeries(context_, relin_keys, c, coefficients, a, b, m_scalingFactorsReal_, m_scalingFactorsRealBig_));
  result.width_ = input.width_;
  result.num_ch_ = input.num_ch_;
  result.slotstr_ = input.slotstr_;
  return result;
}

const std::vector<double>& DNN::SignCoefficients(size_t k) {
  // src/dnn.cu:173-175
  static const std::vector<std::vector<double>> rows = {
      {0, 0.667972070856, 0, -0.223989523020, 0, 0.136121229346, 0, -0.099160550898, 0, 0.079224867308, 0, -0.067250088206,
       0, 0.059852569462, 0, -0.503955481350},
      {0, 0.955669291788, 0, -0.317870998995, 0, 0.189953989728, 0, -0.134924463410, 0, 0.104260767625, 0, -0.084798113265,
       0, 0.071534728674, 0, -0.282024623439},
      {0, 1.254717353059, 0, -0.371638622338, 0, 0.175181567419, 0, -0.085946606966, 0, 0.039326533561, 0, -0.015616729371,
       0, 0.004903749402, 0, -0.000987938705}};
  if (k > 2) throw std::invalid_argument("Sign: k must be 0, 1 or 2");
  return rows[k];
}

double DNN::SignInterval(size_t k) {
  if (k > 2) throw std::invalid_argument("Sign: k must be 0, 1 or 2");
  return k == 0 ? 1.0 : k == 1 ? 1.908 : 1.332;
}

TensorCT DNN::Sign(const TensorCT& input, const PhantomRelinKey& relin_keys, size_t k) {
  const std::vector<double>& coefficients = SignCoefficients(k);
  const double b = SignInterval(k);
  check_uniform(input, "Sign");
  TensorCT result;
  for (const PhantomCiphertext& c : input.ctks_)
    result.ctks_.push_back(
        EvalChebyshevSeries(context_, relin_keys, c, coefficients, -b, b, m_scalingFactorsReal_, m_scalingFactorsRealBig_));
  result.width_ = input.width_;
  result.num_ch_ = input.num_ch_;
  result.slotstr_ = input.slotstr_;
  return result;
}

TensorCT DNN::ReluDegTwo(const TensorCT& input, const PhantomRelinKey& relin_keys) {
  check_uniform(input, "ReluDegTwo");
  TensorCT result;
  for (const PhantomCiphertext& c : input.ctks_) {
    const PhantomCiphertext x2 = EvalSquare(context_, c, relin_keys, m_scalingFactorsReal_, m_scalingFactorsRealBig_);
    result.ctks_.push_back(EvalAddAuto(context_, c, x2, m_scalingFactorsReal_, m_scalingFactorsRealBig_));
  }
  result.width_ = input.width_;
  result.num_ch_ = input.num_ch_;
  result.slotstr_ = input.slotstr_;
  return result;
}

TensorCT DNN::ReluComposite(const TensorCT& input, FHECKKSRNS& bootstrapper, size_t pack) {
  const PackPlan plan = pack_plan(context_.poly_degree(), input.width_, input.slotstr_, pack);
  check_uniform(input, "ReluComposite");
  if (plan.log_pack > bootstrapper.correction_factor())
    throw std::invalid_argument("ReluComposite: log2(pack) exceeds the bootstrapper's correction factor");
  TensorCT sign = input;
  // scaled down so that it falls into [-1, 1]
  for (PhantomCiphertext& c : sign.ctks_) EvalMultConstInplace(context_, c, 0.1, m_scalingFactorsReal_);
  sign = Sign(sign, mul_key_, 0);
  sign = BootStrap(sign, bootstrapper, pack);
  sign = Sign(sign, mul_key_, 1);
  sign = BootStrap(sign, bootstrapper, pack);
  sign = Sign(sign, mul_key_, 2);
  TensorCT result;
  for (size_t i = 0; i < sign.num_ch_; ++i) {
    EvalAddConstInPlaceWrap(context_, sign.ctks_[i], 1, m_scalingFactorsReal_, m_scalingFactorsRealBig_);
    const PhantomCiphertext half = EvalMultConst(context_, input.ctks_[i], 0.5, m_scalingFactorsReal_);
    result.ctks_.push_back(
        EvalMultAuto(context_, sign.ctks_[i], half, mul_key_, m_scalingFactorsReal_, m_scalingFactorsRealBig_));
  }
  result.width_ = input.width_;
  result.num_ch_ = input.num_ch_;
  result.slotstr_ = input.slotstr_;
  return BootStrap(result, bootstrapper, pack);
}

}  // namespace phantom
