// avgpool_example — the hoisted average pooling + fully connected layer (DNN::AvgPoolFullCon,
// host/dnn.h) against the reference's order of the same layer, both through the C++ façade on the
// same ciphertexts and keys.
//
// The baseline is the layer as the reference schedules it (src/dnn.cu:397-452): per input channel
// the log2(width) doubling steps per direction with EvalRotateFused + EvalAddAuto (rows by
// Lg 2^slotstr 2^j, the corrected amounts: the reference's Lg 2^j is a row step only for slotstr = 0),
// then EvalMultConst / EvalAddAuto over the T t weights and EvalAddConstInPlaceWrap of the bias.
//
// usage: avgpool_example check
//          N = 2^12, CoeffModulus::Create(N, {60, 50, 50, 50, 50, 60, 60}), two special primes, scale
//          2^50 (the context of conv_example check); inputs uniform in [-1, 1], weights uniform in
//          [-1, 1] divided by width^2, bias in [-1, 1], fixed seed.  Case 1: width 8, slotstr 0, 3 -> 2.
//          Case 2: width 4, slotstr 1, 3 -> 2.  One JSON line per case: the hoisted layer's and the
//          baseline's maximum error at pixel (0, 0) against sum_k W[u][k] sum_pixels x + b, the maximum
//          difference of the two decodes over all ns slots, both results' metadata, and whether
//          MixChannels equals the EvalMultConst / EvalAddAuto loop word for word.  A last `done` line;
//          exit status 0 iff every line is ok.
//        avgpool_example time <log_n> <chain> <width> <slotstr> <t> <T> [reps]
//          log_n = 16 takes the bootstrap's key chain ({60, 29 x 59} + 10 x 60), else the chain of
//          `check`; the input is brought to chain index <chain>.  The hoisted layer and the baseline
//          alternate in one process after a warm-up, every timed window ending in a stream
//          synchronise; then keyswitch_rotate_sum alone (width - 1 entries + identity, HIP events)
//          against one keyswitch_rotate_batch launch over the same entries followed by the additions
//          of its outputs, by poly_add_many (each operand read once) and by pairwise poly_add.  One
//          JSON line with medians and ranges, the operation counts and the shape-derived bytes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "../csrc/rns.h"
#include "../host/avgpool.h"
#include "../host/buffer.h"
#include "../host/ckks_eval.h"
#include "../host/dnn.h"
#include "../host/encoder.h"
#include "../host/evaluate.h"
#include "../host/keys.h"
#include "../host/modulus.h"
#include "../host/rns_tool.h"

using namespace phantom;
using namespace phantom::arith;
using cplx = std::complex<double>;
using Matrix = std::vector<std::vector<double>>;

static DNN::Tensor3 random_image(size_t width, size_t ch, std::mt19937_64& rng) {
  std::uniform_real_distribution<double> d(-1.0, 1.0);
  DNN::Tensor3 x(width, std::vector<std::vector<double>>(width, std::vector<double>(ch)));
  for (auto& row : x)
    for (auto& px : row)
      for (double& v : px) v = d(rng);
  return x;
}

// uniform in [-1, 1] / width^2: the average's factor folded into the weights, as a model does
static Matrix random_weight(size_t T, size_t t, size_t width, std::mt19937_64& rng) {
  std::uniform_real_distribution<double> d(-1.0, 1.0);
  Matrix w(T, std::vector<double>(t));
  for (auto& row : w)
    for (double& v : row) v = d(rng) / static_cast<double>(width * width);
  return w;
}

// the reference's schedule through the façade, with whole-row steps
static TensorCT baseline_pool_fc(DNN& model, const PhantomContext& ctx, const TensorCT& in, const Matrix& w,
                                 const std::vector<double>& bias) {
  const auto& sf = model.scalingFactorsReal();
  const auto& sfBig = model.scalingFactorsRealBig();
  const size_t T = w.size(), t = in.num_ch_, pw = size_t(1) << in.slotstr_, lg = in.width_ * pw;
  size_t log_l = 0;
  while ((size_t(1) << log_l) < in.width_) ++log_l;
  std::vector<PhantomCiphertext> pooled(t);
  for (size_t k = 0; k < t; ++k) {
    pooled[k] = in.ctks_[k];
    for (size_t i = 0; i < log_l; ++i) {
      PhantomCiphertext tmp;
      EvalRotateFused(ctx, model.galois_keys(), pooled[k], tmp, static_cast<int>(pw << i));
      pooled[k] = EvalAddAuto(ctx, tmp, pooled[k], sf, sfBig);
    }
    for (size_t j = 0; j < log_l; ++j) {
      PhantomCiphertext tmp;
      EvalRotateFused(ctx, model.galois_keys(), pooled[k], tmp, static_cast<int>((lg * pw) << j));
      pooled[k] = EvalAddAuto(ctx, tmp, pooled[k], sf, sfBig);
    }
  }
  TensorCT out;
  out.ctks_.resize(T);
  for (size_t u = 0; u < T; ++u) {
    for (size_t k = 0; k < t; ++k) {
      PhantomCiphertext term = EvalMultConst(ctx, pooled[k], w[u][k], sf);
      out.ctks_[u] = k == 0 ? std::move(term) : EvalAddAuto(ctx, term, out.ctks_[u], sf, sfBig);
    }
    EvalAddConstInPlaceWrap(ctx, out.ctks_[u], bias[u], sf, sfBig);
  }
  out.width_ = in.width_;
  out.num_ch_ = T;
  out.slotstr_ = in.slotstr_;
  return out;
}

// the EvalMultConst / EvalAddAuto loop on the unpooled channels (what MixChannels must equal)
static TensorCT baseline_mix(DNN& model, const PhantomContext& ctx, const TensorCT& in, const Matrix& w) {
  const auto& sf = model.scalingFactorsReal();
  const auto& sfBig = model.scalingFactorsRealBig();
  TensorCT out;
  out.ctks_.resize(w.size());
  for (size_t u = 0; u < w.size(); ++u)
    for (size_t k = 0; k < in.num_ch_; ++k) {
      PhantomCiphertext term = EvalMultConst(ctx, in.ctks_[k], w[u][k], sf);
      out.ctks_[u] = k == 0 ? std::move(term) : EvalAddAuto(ctx, term, out.ctks_[u], sf, sfBig);
    }
  out.width_ = in.width_;
  out.num_ch_ = w.size();
  out.slotstr_ = in.slotstr_;
  return out;
}

static bool words_equal(const PhantomContext& ctx, const TensorCT& a, const TensorCT& b) {
  if (a.ctks_.size() != b.ctks_.size()) return false;
  for (size_t u = 0; u < a.ctks_.size(); ++u) {
    const PhantomCiphertext &x = a.ctks_[u], &y = b.ctks_[u];
    const size_t words = x.size() * x.coeff_modulus_size() * ctx.poly_degree();
    if (words != y.size() * y.coeff_modulus_size() * ctx.poly_degree()) return false;
    std::vector<uint64_t> hx(words), hy(words);
    PHX_CHECK(hipMemcpyAsync(hx.data(), x.data(), words * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx.stream()));
    PHX_CHECK(hipMemcpyAsync(hy.data(), y.data(), words * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx.stream()));
    PHX_CHECK(hipStreamSynchronize(ctx.stream()));
    if (hx != hy) return false;
  }
  return true;
}

// the first ns decoded slots of every channel: [ch][ns]
static std::vector<std::vector<double>> decode_slots(const PhantomContext& ctx, PhantomCKKSEncoder& encoder,
                                                     PhantomSecretKey& sk, const TensorCT& t, size_t ns) {
  const size_t slots = encoder.slot_count(), ch = t.ctks_.size();
  DeviceBuffer<cplx> dv(ch * slots, ctx.stream());
  sk.decrypt_decode_batch(ctx, encoder, t.ctks_, 0, dv.get());
  const std::vector<cplx> v = dv.download(ctx.stream());
  std::vector<std::vector<double>> out(ch, std::vector<double>(ns));
  for (size_t k = 0; k < ch; ++k)
    for (size_t i = 0; i < ns; ++i) out[k][i] = v[k * slots + i].real();
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

static bool check_case(const char* name, size_t width, size_t slotstr, size_t t, size_t T, uint64_t seed) {
  const int log_n = 12;
  PhantomContext ctx(make_parms(log_n));
  PhantomCKKSEncoder encoder(ctx);
  const double scale = std::ldexp(1.0, 50);
  PhantomSecretKey sk(ctx);
  PhantomPublicKey pk = sk.gen_publickey(ctx);
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> unit(-1.0, 1.0);
  const DNN::Tensor3 image = random_image(width, t, rng);
  const Matrix weight = random_weight(T, t, width, rng);
  std::vector<double> bias(T);
  for (double& b : bias) b = unit(rng);

  DNN model(static_cast<size_t>(scale), encoder, ctx);
  std::vector<int32_t> rots;
  model.AddAvgPoolRotationsTo(rots, width, slotstr);
  model.BuildGaloisKey(sk, rots);
  TensorCT input = model.EncTensor(image, pk, slotstr);
  input.ctks_[0].PreComputeScale(ctx, scale);
  model.setScalingFactors(input.ctks_[0].getScalingFactorsReal(), input.ctks_[0].getScalingFactorsRealBig());

  std::vector<double> want(T);
  for (size_t u = 0; u < T; ++u) {
    double s = bias[u];
    for (size_t k = 0; k < t; ++k) {
      double px = 0;
      for (size_t i = 0; i < width; ++i)
        for (size_t j = 0; j < width; ++j) px += image[i][j][k];
      s += weight[u][k] * px;
    }
    want[u] = s;
  }
  const size_t lg = width << slotstr, ns = lg * lg;
  TensorCT hoisted = model.AvgPoolFullCon(input, weight, bias);
  TensorCT base = baseline_pool_fc(model, ctx, input, weight, bias);
  const auto dh = decode_slots(ctx, encoder, sk, hoisted, ns), db = decode_slots(ctx, encoder, sk, base, ns);
  double eh = 0, eb = 0, diff = 0;
  for (size_t u = 0; u < T; ++u) {
    eh = std::max(eh, std::fabs(dh[u][0] - want[u]));
    eb = std::max(eb, std::fabs(db[u][0] - want[u]));
    for (size_t i = 0; i < ns; ++i) diff = std::max(diff, std::fabs(dh[u][i] - db[u][i]));
  }
  const bool meta = same_metadata(hoisted, base);
  const TensorCT mix = model.MixChannels(input, weight), mix_base = baseline_mix(model, ctx, input, weight);
  const bool mix_equal = same_metadata(mix, mix_base) && words_equal(ctx, mix, mix_base);
  // the baseline within the bound of ckks_example (1e-3), else the comparison says nothing; the hoisted
  // layer at most twice the baseline's error; both compute the same function of every slot
  const bool ok = meta && mix_equal && eb < 1e-3 && eh <= 2 * eb && diff < 1e-3;
  std::printf("{\"check\": \"%s\", \"log_n\": %d, \"width\": %zu, \"slotstr\": %zu, \"t\": %zu, \"T\": %zu, "
              "\"hoisted_max_error\": %.6e, \"baseline_max_error\": %.6e, \"slots_max_difference\": %.6e, "
              "\"metadata_equal\": %s, \"mix_words_equal\": %s, \"log2_sf_level\": %.6f, \"input\": %s, \"hoisted\": %s, "
              "\"baseline\": %s, \"ok\": %s}\n",
              name, log_n, width, slotstr, t, T, eh, eb, diff, meta ? "true" : "false", mix_equal ? "true" : "false",
              std::log2(model.scalingFactorsReal().at(level_of(input.ctks_[0]))), metadata(input).c_str(), metadata(hoisted).c_str(), metadata(base).c_str(), ok ? "true" : "false");
  return ok;
}

static int run_check() {
  bool all = check_case("avgpool", 8, 0, 3, 2, 0xA7601);
  all = check_case("avgpool_slotstr1", 4, 1, 3, 2, 0xA7602) && all;
  std::printf("{\"done\": \"avgpool_example check\", \"ok\": %s}\n", all ? "true" : "false");
  return all ? 0 : 1;
}

struct Stat {
  double median, min, max;
};
static Stat stat(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return {v[v.size() / 2], v.front(), v.back()};
}

static int run_time(int log_n, size_t chain, size_t width, size_t slotstr, size_t t, size_t T, int reps) {
  PhantomContext ctx(make_parms(log_n));
  if (chain < 1 || chain >= ctx.total_parm_size() || reps < 1) throw std::invalid_argument("bad chain or reps");
  PhantomCKKSEncoder encoder(ctx);
  hipStream_t s = ctx.stream();
  const double scale = std::ldexp(1.0, log_n == 16 ? 59 : 50);
  PhantomSecretKey sk(ctx);
  PhantomPublicKey pk = sk.gen_publickey(ctx);
  std::mt19937_64 rng(7);
  std::uniform_real_distribution<double> unit(-1.0, 1.0);
  const DNN::Tensor3 image = random_image(width, t, rng);
  const Matrix weight = random_weight(T, t, width, rng);
  std::vector<double> bias(T);
  for (double& b : bias) b = unit(rng);
  DNN model(static_cast<size_t>(scale), encoder, ctx);
  std::vector<int32_t> rots;
  model.AddAvgPoolRotationsTo(rots, width, slotstr);
  model.BuildGaloisKey(sk, rots);
  TensorCT input = model.EncTensor(image, pk, slotstr);
  input.ctks_[0].PreComputeScale(ctx, scale);
  model.setScalingFactors(input.ctks_[0].getScalingFactorsReal(), input.ctks_[0].getScalingFactorsRealBig());
  if (chain > 1)
    for (PhantomCiphertext& c : input.ctks_) ModSwitchLevelInPlace(ctx, c, chain - 1);

  using clock = std::chrono::steady_clock;
  auto ms_since = [](clock::time_point t0) { return std::chrono::duration<double, std::milli>(clock::now() - t0).count(); };
  TensorCT hoisted, base;
  auto run_hoisted = [&] {
    PHX_CHECK(hipStreamSynchronize(s));
    const auto t0 = clock::now();
    hoisted = model.AvgPoolFullCon(input, weight, bias);
    PHX_CHECK(hipStreamSynchronize(s));
    return ms_since(t0);
  };
  auto run_base = [&] {
    PHX_CHECK(hipStreamSynchronize(s));
    const auto t0 = clock::now();
    base = baseline_pool_fc(model, ctx, input, weight, bias);
    PHX_CHECK(hipStreamSynchronize(s));
    return ms_since(t0);
  };
  run_hoisted();  // warm: code objects, pool, workspace, Galois tables
  run_base();
  std::vector<double> th, tb;
  for (int r = 0; r < reps; ++r) {
    th.push_back(run_hoisted());
    tb.push_back(run_base());
  }
  const size_t lg = width << slotstr, ns = lg * lg;
  const auto dh = decode_slots(ctx, encoder, sk, hoisted, ns), db = decode_slots(ctx, encoder, sk, base, ns);
  double diff = 0;
  for (size_t u = 0; u < T; ++u)
    for (size_t i = 0; i < ns; ++i) diff = std::max(diff, std::fabs(dh[u][i] - db[u][i]));

  // keyswitch_rotate_sum alone (the column entries + identity of output 0) against the composition
  // the engine offered before: one keyswitch_rotate_batch launch, then the sum of its outputs
  const RnsTool& rt = ctx.get_context_data(chain).gpu_rns_tool();
  const size_t n = ctx.poly_degree(), Ql = rt.size_Ql(), P = ctx.size_P(), QlP = Ql + P, beta = rt.beta(), R = width - 1;
  const size_t ext_words = 2 * QlP * n;
  const std::vector<int> amounts = avgpool_rotations(width, slotstr);
  std::vector<phx::KsSumEntry> se(R);
  std::vector<phx::KsBatchEntry> be(R + 1);
  for (size_t i = 0; i < R; ++i) {
    const uint32_t elt = FindAutomorphismIndex2nComplex(amounts[i], n);
    se[i].evk = be[i + 1].evk = model.galois_keys().get(elt).public_keys_ptr();
    se[i].perm = be[i + 1].perm = ctx.galois_perm(elt);
    be[i + 1].binv = ctx.galois_block_inv(elt);
  }
  for (size_t i = 0; i <= R; ++i) be[i].out_off = static_cast<int64_t>(i * ext_words);  // entry 0: the identity
  DeviceBuffer<phx::KsSumEntry> dse;
  DeviceBuffer<phx::KsBatchEntry> dbe;
  dse.upload(se, s);
  dbe.upload(be, s);
  DeviceBuffer<uint64_t> digits(beta * QlP * n, s), fused(ext_words, s), parts((R + 1) * ext_words, s), sum(ext_words, s);
  const uint64_t* ct = input.ctks_[0].data();
  rt.modup(digits.get(), ct + Ql * n, ctx.gpu_rns_tables(), s);
  phx::KsRotateSumArgs sa;
  sa.digits = digits.get();
  sa.entries = dse.get();
  sa.count = static_cast<uint32_t>(R);
  sa.identity = 1;
  sa.qp = ctx.mod_QP().q;
  sa.qp_barrett = ctx.mod_QP().barrett;
  sa.ct = ct;
  sa.pmod = rt.bigP_mod_q();
  sa.pmod_shoup = rt.bigP_mod_q_shoup();
  sa.out = fused.get();
  sa.ql = static_cast<uint32_t>(Ql);
  sa.qlp = static_cast<uint32_t>(QlP);
  sa.size_q = static_cast<uint32_t>(ctx.size_Q());
  sa.size_p = static_cast<uint32_t>(P);
  sa.beta = static_cast<uint32_t>(beta);
  phx::KsRotateBatchArgs ba;
  ba.digits = digits.get();
  ba.entries = dbe.get();
  ba.count = static_cast<uint32_t>(R + 1);
  ba.qp = sa.qp;
  ba.qp_barrett = sa.qp_barrett;
  ba.ct = ct;
  ba.pmod = sa.pmod;
  ba.pmod_shoup = sa.pmod_shoup;
  ba.out = parts.get();
  ba.ql = sa.ql;
  ba.qlp = sa.qlp;
  ba.size_q = sa.size_q;
  ba.size_p = sa.size_p;
  ba.beta = sa.beta;
  // the sum of the R + 1 extended ciphertexts: the Ql limbs and the P limbs have their moduli at
  // different table rows, so two launches per chunk of kAddManyMax operands, both polynomials each
  const phx::ModView mq = ctx.mod_QP(), mp{mq.q + ctx.size_Q(), mq.barrett + 2 * ctx.size_Q()};
  auto add_parts = [&] {
    for (size_t c0 = 0; c0 <= R; c0 += phx::kAddManyMax) {
      phx::AddManyArgs aq, ap;
      aq.count = ap.count = static_cast<int>(std::min<size_t>(phx::kAddManyMax, R + 1 - c0));
      aq.accumulate = ap.accumulate = c0 > 0;
      for (int i = 0; i < aq.count; ++i) {
        aq.in[i] = parts.get() + (c0 + i) * ext_words;
        ap.in[i] = aq.in[i] + Ql * n;
      }
      PHX_CHECK(phx::poly_add_many(aq, sum.get(), mq, n, Ql, s, 2, QlP * n));
      PHX_CHECK(phx::poly_add_many(ap, sum.get() + Ql * n, mp, n, P, s, 2, QlP * n));
    }
  };
  // the same sum by pairwise additions (poly_add takes contiguous polynomials: one launch per
  // polynomial and per part, 4 R launches)
  auto add_pairwise = [&] {
    for (size_t i = 1; i <= R; ++i)
      for (size_t p = 0; p < 2; ++p) {
        const uint64_t* a = (i == 1 ? parts.get() : sum.get()) + p * QlP * n;
        const uint64_t* b = parts.get() + i * ext_words + p * QlP * n;
        uint64_t* o = sum.get() + p * QlP * n;
        PHX_CHECK(phx::poly_add(a, b, o, mq, n, Ql, s));
        PHX_CHECK(phx::poly_add(a + Ql * n, b + Ql * n, o + Ql * n, mp, n, P, s));
      }
  };
  hipEvent_t e0, e1;
  PHX_CHECK(hipEventCreate(&e0));
  PHX_CHECK(hipEventCreate(&e1));
  std::vector<double> tf, tc, tp;
  for (int r = 0; r < reps + 1; ++r) {
    float ms = 0;
    PHX_CHECK(hipEventRecord(e0, s));
    PHX_CHECK(phx::keyswitch_rotate_sum(sa, n, s));
    PHX_CHECK(hipEventRecord(e1, s));
    PHX_CHECK(hipEventSynchronize(e1));
    PHX_CHECK(hipEventElapsedTime(&ms, e0, e1));
    if (r) tf.push_back(ms);
    PHX_CHECK(hipEventRecord(e0, s));
    PHX_CHECK(phx::keyswitch_rotate_batch(ba, n, s));
    add_parts();
    PHX_CHECK(hipEventRecord(e1, s));
    PHX_CHECK(hipEventSynchronize(e1));
    PHX_CHECK(hipEventElapsedTime(&ms, e0, e1));
    if (r) tc.push_back(ms);
    PHX_CHECK(hipEventRecord(e0, s));
    PHX_CHECK(phx::keyswitch_rotate_batch(ba, n, s));
    add_pairwise();
    PHX_CHECK(hipEventRecord(e1, s));
    PHX_CHECK(hipEventSynchronize(e1));
    PHX_CHECK(hipEventElapsedTime(&ms, e0, e1));
    if (r) tp.push_back(ms);
  }
  PHX_CHECK(hipEventDestroy(e0));
  PHX_CHECK(hipEventDestroy(e1));
  std::vector<uint64_t> hf(ext_words), hs(ext_words);
  PHX_CHECK(hipMemcpyAsync(hf.data(), fused.get(), ext_words * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  PHX_CHECK(hipMemcpyAsync(hs.data(), sum.get(), ext_words * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  PHX_CHECK(hipStreamSynchronize(s));
  bool sum_equal = hf == hs;  // the pairwise sum, formed last
  PHX_CHECK(phx::keyswitch_rotate_batch(ba, n, s));
  add_parts();
  PHX_CHECK(hipMemcpyAsync(hs.data(), sum.get(), ext_words * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  PHX_CHECK(hipStreamSynchronize(s));
  sum_equal = sum_equal && hf == hs;
  // shape-derived bytes.  fused: per entry the keys (2 beta QlP n words) and the digits (beta QlP n),
  // the output once (2 QlP n), c0 per entry and the identity's ct (Ql n each, 2 Ql n).  composition: the
  // digits once, the keys per entry, R + 1 extended ciphertexts written and read back, the sum written.
  const double w8 = 8.0 * n;
  const double fused_bytes = w8 * (R * 3.0 * beta * QlP + 2.0 * QlP + (R + 2.0) * Ql);
  const double comp_bytes = w8 * (beta * QlP + R * 2.0 * beta * QlP + 2.0 * Ql + 2.0 * (R + 1) * 2.0 * QlP + 2.0 * QlP);
  // pairwise: the same launch, then R additions that each read two extended ciphertexts and write one
  const double pair_bytes = w8 * (beta * QlP + R * 2.0 * beta * QlP + 2.0 * Ql + (R + 1) * 2.0 * QlP + R * 3.0 * 2.0 * QlP);
  size_t log_l = 0;
  while ((size_t(1) << log_l) < width) ++log_l;
  const Stat h = stat(th), b = stat(tb), f = stat(tf), c = stat(tc), pw = stat(tp);
  std::printf("{\"time\": \"avgpool\", \"log_n\": %d, \"chain\": %zu, \"Ql\": %zu, \"QlP\": %zu, \"beta\": %zu, \"width\": %zu, "
              "\"slotstr\": %zu, \"t\": %zu, \"T\": %zu, \"reps\": %d, "
              "\"hoisted_ms\": {\"median\": %.3f, \"min\": %.3f, \"max\": %.3f}, "
              "\"baseline_ms\": {\"median\": %.3f, \"min\": %.3f, \"max\": %.3f}, \"speedup\": %.2f, "
              "\"slots_max_difference\": %.3e, "
              "\"hoisted_ops\": {\"modups\": %zu, \"rotate_sum_launches\": %zu, \"inner_products\": %zu, "
              "\"moddown_polys\": %zu, \"mix_products\": %zu}, "
              "\"baseline_ops\": {\"key_switches\": %zu, \"moddown_polys\": %zu, \"const_products\": %zu}, "
              "\"rotate_sum\": {\"entries\": %zu, \"identity\": 1, \"equal_to_composition\": %s, "
              "\"fused_ms\": {\"median\": %.3f, \"min\": %.3f, \"max\": %.3f}, \"fused_bytes\": %.0f, \"fused_tb_per_s\": %.3f, "
              "\"composition_ms\": {\"median\": %.3f, \"min\": %.3f, \"max\": %.3f}, \"composition_bytes\": %.0f, "
              "\"composition_tb_per_s\": %.3f, \"fused_over_composition\": %.3f, "
              "\"pairwise_ms\": {\"median\": %.3f, \"min\": %.3f, \"max\": %.3f}, \"pairwise_bytes\": %.0f, "
              "\"pairwise_tb_per_s\": %.3f, \"fused_over_pairwise\": %.3f}}\n",
              log_n, chain, Ql, QlP, beta, width, slotstr, t, T, reps, h.median, h.min, h.max, b.median, b.min, b.max,
              b.median / h.median, diff, 2 * T, 2 * T, 2 * T * R, 4 * T, T * t, 2 * log_l * t, 4 * log_l * t, T * t, R,
              sum_equal ? "true" : "false", f.median, f.min, f.max, fused_bytes, fused_bytes / (f.median * 1e-3) / 1e12,
              c.median, c.min, c.max, comp_bytes, comp_bytes / (c.median * 1e-3) / 1e12, f.median / c.median, pw.median,
              pw.min, pw.max, pair_bytes, pair_bytes / (pw.median * 1e-3) / 1e12, f.median / pw.median);
  std::printf("{\"done\": \"avgpool_example time\", \"ok\": %s}\n", sum_equal ? "true" : "false");
  return sum_equal ? 0 : 1;
}

int main(int argc, char** argv) {
  try {
    if (argc >= 2 && !std::strcmp(argv[1], "check")) return run_check();
    if (argc >= 8 && !std::strcmp(argv[1], "time"))
      return run_time(std::atoi(argv[2]), std::strtoull(argv[3], nullptr, 10), std::strtoull(argv[4], nullptr, 10),
                      std::strtoull(argv[5], nullptr, 10), std::strtoull(argv[6], nullptr, 10),
                      std::strtoull(argv[7], nullptr, 10), argc >= 9 ? std::atoi(argv[8]) : 3);
    std::fprintf(stderr, "usage: avgpool_example check | time <log_n> <chain> <width> <slotstr> <t> <T> [reps]\n");
    return 2;
  } catch (const std::exception& e) {
    std::printf("{\"error\": \"%s\", \"ok\": false}\n", e.what());
    return 1;
  }
}
