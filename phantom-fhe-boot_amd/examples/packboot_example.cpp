// packboot_example — the channel-packed tensor bootstrap (DNN::Pack / Unpack / BootStrap, host/pack.h)
// and the activation layers (DNN::Relu, Sign, ReluDegTwo, ReluComposite) against their plain
// compositions, through the C++ façade on the same ciphertexts and keys.
//
// The chain is bootstrapping_example's: Q = {60, 29 x 59}, P = 10 x 60, scale 2^59, levelBudget {2, 2};
// keys and encryptions are seeded.  Inputs are brought down to 4 limbs before a bootstrap (bench: to
// 10 limbs before ReluComposite).
//
// usage: packboot_example check pack [log_n]
//          per case (width, slotstr, channels C, pack P): Pack against MultByMonomialInPlace + add (a
//          group that is not full leaves tree index 0 free, host/pack.h) and
//          Unpack against EvalRotateFused, add / sub, MultByMonomialInPlace word for word, the decode of
//          Unpack(Pack(x)) / P against x (bound 1e-6, bootstrapping_example ops' bound for a rotation
//          and a monomial multiply), the metadata against the input's.
//        packboot_example check boot [log_n]
//          per case, inputs uniform in [-4, -1] u [1, 4]: the post_shift identity word for word, the
//          metadata of BootStrap(pack = P) against EvalBootstrap's at P ns slots, the packed path's
//          maximum error against twice the error of EvalBootstrap on a fresh ciphertext of P ns
//          random slots (which must stay below 1e-2), and BootStrap(pack = 1)'s error beside them.
//        packboot_example check relu [log_n]
//          Sign(k), Relu and ReluDegTwo on 2 channels against the per-channel calls word for word;
//          ReluComposite on 3 channels of width 8 with pack = 1 and pack = 4 against the cleartext
//          composition of the same three series.
//        packboot_example bench <stage> [side] [reps] [what]
//          log_n = 16, ResNet-20's stage 0 (16 channels x width 32), 1 (32 x width 16, slotstr 1) or
//          2 (64 x width 8, slotstr 2); side = both | pack1 | packed (separate invocations hold one
//          bootstrap setup each); what = boot | relu | all.  Device time from events on the context's
//          stream, median and range of `reps` (default 5) runs after a warm-up, and the maximum error.
//        packboot_example check tree [log_n]
//          EvalRotateFusedBatch against EvalRotateFused word for word (counts 1, 5 and the chunk size
//          + 1, inputs of different scales in one call, once with the unbiased moddown on),
//          unpack_channels_batch against unpack_channels word for word per case (and two full groups),
//          and the refusals of EvalRotateFusedBatch.
//        packboot_example tree <stage> [reps]
//          log_n = 16, the three stages above, the packed groups at the bootstrap's output level (12
//          limbs): device time of Unpack through unpack_channels (one EvalRotateFused per node) and
//          through unpack_channels_batch (one batched rotation per level), both in this process.
// One JSON line per case and a last `done` line; exit status 0 iff every line is ok.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
#include "../host/evaluate.h"
#include "../host/keys.h"
#include "../host/modulus.h"
#include "../host/pack.h"

using namespace phantom;
using namespace phantom::arith;
using cplx = std::complex<double>;

static const char* tf(bool b) { return b ? "true" : "false"; }

static EncryptionParameters make_parms(int log_n) {
  const size_t n = size_t(1) << log_n;
  std::vector<int> bits(1, 60);
  bits.insert(bits.end(), 29, 59);
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

  explicit Rig(int log_n)
      : ctx(make_parms(log_n)), encoder(ctx), sk(PhantomSecretKey::for_testing(ctx, 0x9AC4)), pk(sk.gen_publickey(ctx)),
        model(static_cast<size_t>(std::ldexp(1.0, 59)), encoder, ctx), boot(encoder), n(size_t(1) << log_n) {
    PhantomCiphertext tmp;
    tmp.PreComputeScale(ctx, scale);
    sf = tmp.getScalingFactorsReal();
    sf_big = tmp.getScalingFactorsRealBig();
    model.setScalingFactors(sf, sf_big);
  }
  void setup_boot(const std::vector<uint32_t>& slot_counts) {
    boot.EvalMultKeyGen(sk, ctx);
    for (uint32_t slots : slot_counts) {
      boot.EvalBootstrapSetup(ctx, {2, 2}, scale, sf, 0, slots);
      boot.EvalBootstrapKeyGen(sk, ctx, slots);
    }
  }
};

static DNN::Tensor3 random_image(size_t width, size_t ch, std::mt19937_64& rng, bool away_from_zero) {
  std::uniform_real_distribution<double> unit(-1.0, 1.0), mag(1.0, 4.0);
  DNN::Tensor3 x(width, std::vector<std::vector<double>>(width, std::vector<double>(ch)));
  for (auto& row : x)
    for (auto& px : row)
      for (double& v : px) v = away_from_zero ? (unit(rng) < 0 ? -mag(rng) : mag(rng)) : unit(rng);
  return x;
}

static std::vector<uint64_t> words(const PhantomContext& ctx, const PhantomCiphertext& x) {
  std::vector<uint64_t> h(x.size() * x.coeff_modulus_size() * ctx.poly_degree());
  PHX_CHECK(hipMemcpyAsync(h.data(), x.data(), h.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx.stream()));
  PHX_CHECK(hipStreamSynchronize(ctx.stream()));
  return h;
}

static bool same_meta(const PhantomCiphertext& x, const PhantomCiphertext& y) {
  return x.chain_index() == y.chain_index() && x.size() == y.size() && x.scale() == y.scale() &&
         x.coeff_modulus_size() == y.coeff_modulus_size() && x.GetNoiseScaleDeg() == y.GetNoiseScaleDeg() &&
         x.is_ntt_form() == y.is_ntt_form() && x.correction_factor() == y.correction_factor();
}

static bool same_ct(const PhantomContext& ctx, const PhantomCiphertext& x, const PhantomCiphertext& y) {
  return same_meta(x, y) && words(ctx, x) == words(ctx, y);
}

static bool same_tensor(const PhantomContext& ctx, const TensorCT& a, const TensorCT& b) {
  if (a.width_ != b.width_ || a.slotstr_ != b.slotstr_ || a.num_ch_ != b.num_ch_ || a.ctks_.size() != b.ctks_.size())
    return false;
  for (size_t k = 0; k < a.ctks_.size(); ++k)
    if (!same_ct(ctx, a.ctks_[k], b.ctks_[k])) return false;
  return true;
}

static bool tensor_meta(const TensorCT& t, const TensorCT& like, const PhantomCiphertext& ct_like) {
  if (t.width_ != like.width_ || t.slotstr_ != like.slotstr_ || t.num_ch_ != like.num_ch_ || t.ctks_.size() != t.num_ch_)
    return false;
  for (const PhantomCiphertext& c : t.ctks_)
    if (!same_meta(c, ct_like)) return false;
  return true;
}

static std::string metadata(const PhantomCiphertext& c) {
  char buf[160];
  std::snprintf(buf, sizeof buf, "{\"chain_index\": %zu, \"limbs\": %zu, \"degree\": %zu, \"log2_scale\": %.9f}",
                c.chain_index(), c.coeff_modulus_size(), c.GetNoiseScaleDeg(), std::log2(c.scale()));
  return buf;
}

// per channel, max |decoded / divide - want| over its pixels
static std::vector<double> channel_errors(Rig& r, const TensorCT& t, const DNN::Tensor3& want, double divide) {
  const DNN::Tensor3 got = r.model.DecTensor(t, r.sk);
  std::vector<double> e(want[0][0].size(), 0.0);
  for (size_t i = 0; i < want.size(); ++i)
    for (size_t j = 0; j < want.size(); ++j)
      for (size_t k = 0; k < e.size(); ++k) {
        const double d = std::fabs(got[i][j][k] / divide - want[i][j][k]);
        if (!(d <= e[k])) e[k] = d;  // NaN sticks
      }
  return e;
}

static double max_of(const std::vector<double>& v) {
  double e = 0;
  for (double d : v)
    if (!(d <= e)) e = d;
  return e;
}

// ... over all pixels and channels
static double tensor_error(Rig& r, const TensorCT& t, const DNN::Tensor3& want, double divide) {
  return max_of(channel_errors(r, t, want, divide));
}

static std::string json_list(const std::vector<double>& v) {
  std::string out = "[";
  char buf[32];
  for (size_t k = 0; k < v.size(); ++k) {
    std::snprintf(buf, sizeof buf, "%s%.3e", k ? ", " : "", v[k]);
    out += buf;
  }
  return out + "]";
}

static size_t log2_of(size_t x) {
  size_t g = 0;
  while ((size_t(1) << g) < x) ++g;
  return g;
}

// ---- check pack ---------------------------------------------------------------------------------

static bool check_pack_case(Rig& r, const char* name, size_t width, size_t slotstr, size_t C, size_t P, uint64_t seed) {
  const PhantomContext& ctx = r.ctx;
  std::mt19937_64 rng(seed);
  const DNN::Tensor3 image = random_image(width, C, rng, false);
  const TensorCT input = r.model.EncTensor(image, r.pk, slotstr);
  const PackPlan plan = pack_plan(r.n, width, slotstr, P);
  const uint32_t M = static_cast<uint32_t>(2 * r.n);

  const PackedCT packed = r.model.Pack(input, P);
  bool pack_equal = packed.ctks_.size() == plan.groups(C) && packed.pack_ == P && packed.num_ch_ == C;
  // the plain composition: channel c of a group at tree index lead + c (lead = 1 unless the group is full)
  for (size_t g = 0; pack_equal && g < packed.ctks_.size(); ++g) {
    const size_t members = plan.members(C, g), lead = plan.lead(members);
    PhantomCiphertext acc;
    for (size_t c = 0; c < members; ++c) {
      PhantomCiphertext term = input.ctks_[g * P + c];
      if (lead + c) MultByMonomialInPlace(ctx, term, static_cast<uint32_t>((lead + c) * plan.stride));
      if (c == 0) acc = std::move(term);
      else add_inplace(ctx, acc, term);
    }
    pack_equal = same_ct(ctx, packed.ctks_[g], acc);
  }

  // the whole tree by plain operations (no node left out), the channels read at their indices
  const TensorCT unpacked = r.model.Unpack(packed);
  bool unpack_equal = unpacked.ctks_.size() == C;
  for (size_t g = 0; unpack_equal && g < packed.ctks_.size(); ++g) {
    const size_t members = plan.members(C, g), lead = plan.lead(members);
    std::vector<PhantomCiphertext> node(P);
    node[0] = packed.ctks_[g];
    for (size_t t = 0; t < plan.log_pack; ++t)
      for (size_t idx = 0; idx < (size_t(1) << t); ++idx) {
        const PhantomCiphertext rot = EvalRotateFused(ctx, node[idx], r.model.galois_keys(), plan.rotations[t]);
        const size_t child = idx | (size_t(1) << t);
        node[child] = node[idx];
        sub_inplace(ctx, node[child], rot);
        MultByMonomialInPlace(ctx, node[child], M - (plan.stride << t));
        add_inplace(ctx, node[idx], rot);
      }
    for (size_t c = 0; unpack_equal && c < members; ++c)
      unpack_equal = same_ct(ctx, unpacked.ctks_[g * P + c], node[lead + c]);
  }

  const double err = tensor_error(r, unpacked, image, static_cast<double>(P));
  const bool meta = tensor_meta(unpacked, input, input.ctks_[0]);
  const bool ok = pack_equal && unpack_equal && meta && err < 1e-6;
  std::printf("{\"check\": \"%s\", \"log_n\": %zu, \"width\": %zu, \"slotstr\": %zu, \"channels\": %zu, \"pack\": %zu, "
              "\"groups\": %zu, \"stride_power\": %u, \"pack_words_equal\": %s, \"unpack_words_equal\": %s, "
              "\"max_error\": %.6e, \"bound\": 1e-6, \"metadata_equal\": %s, \"input\": %s, \"unpacked\": %s, \"ok\": %s}\n",
              name, log2_of(r.n), width, slotstr, C, P, packed.ctks_.size(), plan.stride, tf(pack_equal), tf(unpack_equal),
              err, tf(meta), metadata(input.ctks_[0]).c_str(), metadata(unpacked.ctks_.at(0)).c_str(), tf(ok));
  std::fflush(stdout);
  return ok;
}

struct Case {
  const char* name;
  size_t width, slotstr, C, P;
};
static const Case kCases[] = {{"w8_c3_p4", 8, 0, 3, 4}, {"w8s1_c8_p8", 8, 1, 8, 8}, {"w8_c5_p4", 8, 0, 5, 4}};

static void model_keys(Rig& r) {
  std::vector<int32_t> rots;
  for (const Case& c : kCases) r.model.AddPackRotationsTo(rots, c.width, c.slotstr, c.P);
  r.model.BuildGaloisKey(r.sk, rots);
  r.model.RelinKeyGen(r.sk);
}

static int run_check_pack(int log_n) {
  Rig r(log_n);
  model_keys(r);
  bool all = true;
  uint64_t seed = 0x9AC40;
  for (const Case& c : kCases) all = check_pack_case(r, c.name, c.width, c.slotstr, c.C, c.P, ++seed) && all;
  std::printf("{\"done\": \"packboot_example check pack\", \"ok\": %s}\n", tf(all));
  return all ? 0 : 1;
}

// ---- check boot ---------------------------------------------------------------------------------

static void drop_to_limbs(Rig& r, TensorCT& t, size_t limbs) {
  for (PhantomCiphertext& c : t.ctks_) ModSwitchLevelInPlace(r.ctx, c, c.coeff_modulus_size() - limbs);
}

// the maximum error of EvalBootstrap on a fresh ciphertext of `slots` random reals of the tests' range
static double yardstick(Rig& r, uint32_t slots, size_t chain, std::mt19937_64& rng, PhantomCiphertext* out = nullptr) {
  std::uniform_real_distribution<double> unit(-1.0, 1.0), mag(1.0, 4.0);
  std::vector<double> v(slots);
  for (double& x : v) x = unit(rng) < 0 ? -mag(rng) : mag(rng);
  PhantomPlaintext pt;
  if (slots < r.n / 2) {
    r.encoder.set_sparse_encode(2 * size_t(slots));
    r.encoder.encode_sparse(r.ctx, v, r.scale, pt, chain);
  } else {
    r.encoder.encode(r.ctx, v, r.scale, pt, chain);
  }
  PhantomCiphertext ct;
  r.sk.encrypt_symmetric(r.ctx, pt, ct);
  const PhantomCiphertext b = r.boot.EvalBootstrap(ct, r.ctx, slots);
  PhantomPlaintext dp;
  r.sk.decrypt(r.ctx, b, dp);
  std::vector<cplx> z;
  r.encoder.decode(r.ctx, dp, z);
  double e = 0;
  for (size_t i = 0; i < slots; ++i) {
    const double d = std::abs(z[i] - cplx(v[i], 0.0));
    if (!(d <= e)) e = d;
  }
  if (out) *out = b;
  return e;
}

static bool check_boot_case(Rig& r, const Case& c, uint64_t seed) {
  const PhantomContext& ctx = r.ctx;
  std::mt19937_64 rng(seed);
  const DNN::Tensor3 image = random_image(c.width, c.C, rng, true);
  TensorCT input = r.model.EncTensor(image, r.pk, c.slotstr);
  drop_to_limbs(r, input, 4);
  const PackPlan plan = pack_plan(r.n, c.width, c.slotstr, c.P);
  const uint32_t slots = static_cast<uint32_t>(plan.slots()), g = static_cast<uint32_t>(plan.log_pack);

  // the shift, on a packed ciphertext (complex slots)
  const PackedCT packed = r.model.Pack(input, c.P);
  PhantomCiphertext shifted = r.boot.EvalBootstrap(packed.ctks_[0], ctx, slots, 1, 0, g);
  MultByIntegerInPlace(ctx, shifted, uint64_t(1) << g);
  const PhantomCiphertext plain = r.boot.EvalBootstrap(packed.ctks_[0], ctx, slots);
  const bool shift_equal = same_ct(ctx, shifted, plain);

  PhantomCiphertext fresh_boot;
  const double e_slot = yardstick(r, slots, input.ctks_[0].chain_index(), rng, &fresh_boot);
  TensorCT out = r.model.BootStrap(input, r.boot, c.P);
  const bool meta = tensor_meta(out, input, fresh_boot) && out.ctks_[0].GetNoiseScaleDeg() == 1;
  const std::vector<double> ch_packed = channel_errors(r, out, image, 1.0);
  const double e_packed = max_of(ch_packed);
  TensorCT base = r.model.BootStrap(input, r.boot, 1);
  const std::vector<double> ch_base = channel_errors(r, base, image, 1.0);
  const double e_base = max_of(ch_base);

  const bool ok = shift_equal && meta && e_slot < 1e-2 && e_packed <= 2 * e_slot;
  std::printf("{\"check\": \"%s\", \"log_n\": %zu, \"width\": %zu, \"slotstr\": %zu, \"channels\": %zu, \"pack\": %zu, "
              "\"slots\": %u, \"post_shift\": %u, \"correction\": %u, \"shift_words_equal\": %s, \"metadata_equal\": %s, "
              "\"slot_bootstrap_max_error\": %.6e, \"packed_max_error\": %.6e, \"pack1_max_error\": %.6e, "
              "\"packed_channel_errors\": %s, \"pack1_channel_errors\": %s, "
              "\"input\": %s, \"packed\": %s, \"slot_bootstrap\": %s, \"pack1\": %s, \"ok\": %s}\n",
              c.name, log2_of(r.n), c.width, c.slotstr, c.C, c.P, slots, g, r.boot.correction_factor(), tf(shift_equal),
              tf(meta), e_slot, e_packed, e_base, json_list(ch_packed).c_str(), json_list(ch_base).c_str(),
              metadata(input.ctks_[0]).c_str(), metadata(out.ctks_[0]).c_str(),
              metadata(fresh_boot).c_str(), metadata(base.ctks_[0]).c_str(), tf(ok));
  std::fflush(stdout);
  return ok;
}

static int run_check_boot(int log_n) {
  Rig r(log_n);
  model_keys(r);
  r.setup_boot({64, 256, 2048});
  bool all = true;
  uint64_t seed = 0xB0070;
  for (const Case& c : kCases) all = check_boot_case(r, c, ++seed) && all;
  std::printf("{\"done\": \"packboot_example check boot\", \"ok\": %s}\n", tf(all));
  return all ? 0 : 1;
}

// ---- check relu ---------------------------------------------------------------------------------

// sum_k c_k T_k(x / b) with c_0 halved (EvalChebyshevSeries's convention)
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

static double relu_composite_clear(double x) {
  double s = 0.1 * x;
  for (size_t k = 0; k < 3; ++k) s = cheb(DNN::SignCoefficients(k), DNN::SignInterval(k), s);
  return 0.5 * x * (s + 1);
}

static int run_check_relu(int log_n) {
  Rig r(log_n);
  model_keys(r);
  const PhantomContext& ctx = r.ctx;
  const PhantomRelinKey rlk = r.sk.gen_relinkey(ctx);
  std::mt19937_64 rng(0x4E10);
  bool all = true;

  {  // the channel loops against the per-channel calls
    const size_t width = 8, ch = 2;
    const DNN::Tensor3 image = random_image(width, ch, rng, false);
    const TensorCT input = r.model.EncTensor(image, r.pk, 0);
    auto per_channel = [&](auto&& f) {
      TensorCT t;
      t.width_ = input.width_, t.slotstr_ = input.slotstr_, t.num_ch_ = input.num_ch_;
      for (const PhantomCiphertext& c : input.ctks_) t.ctks_.push_back(f(c));
      return t;
    };
    bool sign_equal[3];
    for (size_t k = 0; k < 3; ++k) {
      const double b = DNN::SignInterval(k);
      sign_equal[k] = same_tensor(ctx, r.model.Sign(input, rlk, k), per_channel([&](const PhantomCiphertext& c) {
                                    return EvalChebyshevSeries(ctx, rlk, c, DNN::SignCoefficients(k), -b, b, r.sf, r.sf_big);
                                  }));
    }
    const std::vector<double> relu_coef = EvalChebyshevCoefficients([](double x) { return std::max(0.0, x); }, -1, 1, 7);
    const bool relu_equal = same_tensor(ctx, r.model.Relu(input, rlk), per_channel([&](const PhantomCiphertext& c) {
                                          return EvalChebyshevSeries(ctx, rlk, c, relu_coef, -1, 1, r.sf, r.sf_big);
                                        }));
    const bool deg2_equal = same_tensor(ctx, r.model.ReluDegTwo(input, rlk), per_channel([&](const PhantomCiphertext& c) {
                                          return EvalAddAuto(ctx, c, EvalSquare(ctx, c, rlk, r.sf, r.sf_big), r.sf, r.sf_big);
                                        }));
    bool refused = false;
    try {
      r.model.Sign(input, rlk, 3);
    } catch (const std::invalid_argument&) {
      refused = true;
    }
    const bool ok = sign_equal[0] && sign_equal[1] && sign_equal[2] && relu_equal && deg2_equal && refused;
    all = all && ok;
    std::printf("{\"check\": \"layers\", \"log_n\": %d, \"width\": %zu, \"channels\": %zu, \"sign_words_equal\": [%s, %s, %s], "
                "\"relu_words_equal\": %s, \"relu_deg_two_words_equal\": %s, \"sign_k3_refused\": %s, \"ok\": %s}\n",
                log_n, width, ch, tf(sign_equal[0]), tf(sign_equal[1]), tf(sign_equal[2]), tf(relu_equal), tf(deg2_equal),
                tf(refused), tf(ok));
    std::fflush(stdout);
  }

  {  // ReluComposite, pack = 1 and pack = 4, against the cleartext composition of the same series
    const size_t width = 8, ch = 3, P = 4;
    r.setup_boot({64, 256});
    const DNN::Tensor3 image = random_image(width, ch, rng, true);
    DNN::Tensor3 want = image;
    for (auto& row : want)
      for (auto& px : row)
        for (double& v : px) v = relu_composite_clear(v);
    const TensorCT input = r.model.EncTensor(image, r.pk, 0);
    const TensorCT one = r.model.ReluComposite(input, r.boot, 1);
    const TensorCT packed = r.model.ReluComposite(input, r.boot, P);
    const double e_one = tensor_error(r, one, want, 1.0), e_packed = tensor_error(r, packed, want, 1.0);
    const bool meta = tensor_meta(packed, one, one.ctks_.at(0));
    const bool ok = meta && e_one < 0.35 && e_packed <= 2 * e_one;
    all = all && ok;
    std::printf("{\"check\": \"relu_composite\", \"log_n\": %d, \"width\": %zu, \"channels\": %zu, \"pack\": %zu, "
                "\"pack1_max_deviation\": %.6e, \"packed_max_deviation\": %.6e, \"condition\": 0.35, \"metadata_equal\": %s, "
                "\"pack1\": %s, \"packed\": %s, \"ok\": %s}\n",
                log_n, width, ch, P, e_one, e_packed, tf(meta), metadata(one.ctks_[0]).c_str(),
                metadata(packed.ctks_[0]).c_str(), tf(ok));
    std::fflush(stdout);
  }
  std::printf("{\"done\": \"packboot_example check relu\", \"ok\": %s}\n", tf(all));
  return all ? 0 : 1;
}

// ---- check tree ---------------------------------------------------------------------------------

static bool rotate_batch_case(Rig& r, const char* name, const std::vector<PhantomCiphertext>& in, int index) {
  const PhantomContext& ctx = r.ctx;
  std::vector<const PhantomCiphertext*> ptrs;
  for (const PhantomCiphertext& c : in) ptrs.push_back(&c);
  const std::vector<PhantomCiphertext> got = EvalRotateFusedBatch(ctx, ptrs, r.model.galois_keys(), index);
  bool equal = got.size() == in.size();
  for (size_t k = 0; equal && k < in.size(); ++k)
    equal = same_ct(ctx, got[k], EvalRotateFused(ctx, in[k], r.model.galois_keys(), index));
  std::printf("{\"check\": \"%s\", \"log_n\": %zu, \"count\": %zu, \"chunk\": %zu, \"limbs\": %zu, \"rotation\": %d, "
              "\"unbiased_moddown\": %s, \"rotate_words_equal\": %s, \"ok\": %s}\n",
              name, log2_of(r.n), in.size(), rotate_fused_batch_chunk(ctx, in[0].chain_index()),
              in[0].coeff_modulus_size(), index, tf(ctx.unbiased_moddown()), tf(equal), tf(equal));
  std::fflush(stdout);
  return equal;
}

static bool tree_case(Rig& r, const Case& c, uint64_t seed) {
  const PhantomContext& ctx = r.ctx;
  std::mt19937_64 rng(seed);
  const TensorCT input = r.model.EncTensor(random_image(c.width, c.C, rng, false), r.pk, c.slotstr);
  const PackPlan plan = pack_plan(r.n, c.width, c.slotstr, c.P);
  const PackedCT packed = r.model.Pack(input, c.P);
  std::vector<const PhantomCiphertext*> groups;
  std::vector<size_t> members;
  for (size_t g = 0; g < packed.ctks_.size(); ++g) {
    groups.push_back(&packed.ctks_[g]);
    members.push_back(plan.members(c.C, g));
  }
  const auto got = unpack_channels_batch(ctx, plan, groups, members, r.model.galois_keys());
  bool equal = got.size() == groups.size();
  for (size_t g = 0; equal && g < groups.size(); ++g) {
    const auto want = unpack_channels(ctx, plan, packed.ctks_[g], members[g], r.model.galois_keys());
    equal = want.size() == got[g].size();
    for (size_t k = 0; equal && k < want.size(); ++k) equal = same_ct(ctx, got[g][k], want[k]);
  }
  // the layer through either path
  r.model.set_unpack_path(DNN::UnpackPath::kPerNode);
  const TensorCT per_node = r.model.Unpack(packed);
  r.model.set_unpack_path(DNN::UnpackPath::kBatched);
  const bool layer_equal = same_tensor(ctx, r.model.Unpack(packed), per_node);
  const bool ok = equal && layer_equal;
  std::printf("{\"check\": \"tree_%s\", \"log_n\": %zu, \"width\": %zu, \"slotstr\": %zu, \"channels\": %zu, \"pack\": %zu, "
              "\"groups\": %zu, \"tree_words_equal\": %s, \"unpack_words_equal\": %s, \"ok\": %s}\n",
              c.name, log2_of(r.n), c.width, c.slotstr, c.C, c.P, groups.size(), tf(equal), tf(layer_equal), tf(ok));
  std::fflush(stdout);
  return ok;
}

template <class F>
static bool refusal(const char* what, F&& f) {
  bool thrown = false;
  try {
    f();
  } catch (const std::invalid_argument&) {
    thrown = true;
  }
  std::printf("{\"check\": \"refusal\", \"case\": \"%s\", \"thrown\": %s, \"ok\": %s}\n", what, tf(thrown), tf(thrown));
  std::fflush(stdout);
  return thrown;
}

static int run_check_tree(int log_n) {
  Rig r(log_n);
  model_keys(r);
  const PhantomContext& ctx = r.ctx;
  const PhantomGaloisKey& keys = r.model.galois_keys();
  bool all = true;
  std::mt19937_64 rng(0x7EE0);
  const int index = pack_rotations(8, 0, 4)[0];
  // ciphertexts at one level, every second one with another scale in its metadata
  auto inputs = [&](size_t count, size_t limbs) {
    const TensorCT t = r.model.EncTensor(random_image(8, count, rng, false), r.pk, 0);
    std::vector<PhantomCiphertext> v = t.ctks_;
    for (size_t k = 0; k < v.size(); ++k) {
      if (limbs < v[k].coeff_modulus_size()) ModSwitchLevelInPlace(ctx, v[k], v[k].coeff_modulus_size() - limbs);
      if (k & 1) v[k].set_scale(v[k].scale() * 3.0);
    }
    return v;
  };
  all = rotate_batch_case(r, "rotate_batch_1", inputs(1, 30), index) && all;
  all = rotate_batch_case(r, "rotate_batch_5", inputs(5, 30), index) && all;
  {
    const std::vector<PhantomCiphertext> v = inputs(5, 12);
    const size_t chunk = rotate_fused_batch_chunk(ctx, v[0].chain_index());
    std::vector<PhantomCiphertext> many;
    for (size_t k = 0; k < chunk + 1; ++k) many.push_back(v[k % v.size()]);
    all = rotate_batch_case(r, "rotate_batch_chunk_plus_1", many, index) && all;
  }
  r.ctx.set_unbiased_moddown(true);
  all = rotate_batch_case(r, "rotate_batch_unbiased", inputs(5, 12), index) && all;
  r.ctx.set_unbiased_moddown(false);

  uint64_t seed = 0x7EE40;
  for (const Case& c : kCases) all = tree_case(r, c, ++seed) && all;
  all = tree_case(r, Case{"w8_c8_p4", 8, 0, 8, 4}, ++seed) && all;

  {  // the refusals: nothing may be enqueued, so each is followed by a comparison that still holds
    const std::vector<PhantomCiphertext> v = inputs(3, 12);
    PhantomCiphertext lower = v[1];
    ModSwitchLevelInPlace(ctx, lower, 1);
    PhantomCiphertext coeff = v[1];
    coeff.set_ntt_form(false);
    PhantomCiphertext three = v[1];
    three.resize(ctx, v[1].chain_index(), 3, ctx.stream(), false);
    int missing = 1;
    while (keys.has(FindAutomorphismIndex2nComplex(missing, r.n))) ++missing;
    auto call = [&](const PhantomCiphertext* a, const PhantomCiphertext* b, int idx) {
      const PhantomCiphertext* p[3] = {&v[0], a, b};
      EvalRotateFusedBatch(ctx, p, keys, idx);
    };
    all = refusal("different chain indices", [&] { call(&lower, &v[2], index); }) && all;
    all = refusal("not NTT form", [&] { call(&coeff, &v[2], index); }) && all;
    all = refusal("three polynomials", [&] { call(&three, &v[2], index); }) && all;
    all = refusal("null entry", [&] { call(nullptr, &v[2], index); }) && all;
    all = refusal("missing key", [&] { call(&v[1], &v[2], missing); }) && all;
    const bool empty = EvalRotateFusedBatch(ctx, {}, keys, index).empty();
    std::printf("{\"check\": \"empty_span\", \"empty_result\": %s, \"ok\": %s}\n", tf(empty), tf(empty));
    all = all && empty;
    all = rotate_batch_case(r, "rotate_batch_after_refusals", v, index) && all;
  }
  std::printf("{\"done\": \"packboot_example check tree\", \"ok\": %s}\n", tf(all));
  return all ? 0 : 1;
}

// ---- bench --------------------------------------------------------------------------------------

struct Stat {
  double median, min, max;
};
static Stat stat(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return {v[v.size() / 2], v.front(), v.back()};
}

static int run_bench(int stage, const std::string& side, int reps, const std::string& what) {
  static const Case stages[] = {{"stage0", 32, 0, 16, 16}, {"stage1", 16, 1, 32, 32}, {"stage2", 8, 2, 64, 32}};
  if (stage < 0 || stage > 2 || reps < 1 || (side != "both" && side != "pack1" && side != "packed") ||
      (what != "boot" && what != "relu" && what != "all"))
    throw std::invalid_argument("bench <stage 0..2> [both|pack1|packed] [reps] [boot|relu|all]");
  const Case& c = stages[stage];
  const int log_n = 16;
  Rig r(log_n);
  const PackPlan plan = pack_plan(r.n, c.width, c.slotstr, c.P);
  std::vector<int32_t> rots;
  r.model.AddPackRotationsTo(rots, c.width, c.slotstr, c.P);
  r.model.BuildGaloisKey(r.sk, rots);
  r.model.RelinKeyGen(r.sk);
  std::vector<uint32_t> setups;
  if (side != "packed") setups.push_back(static_cast<uint32_t>(plan.ns));
  if (side != "pack1") setups.push_back(static_cast<uint32_t>(plan.slots()));
  r.setup_boot(setups);
  PHX_CHECK(hipDeviceSynchronize());

  std::mt19937_64 rng(0xBE7C);
  const DNN::Tensor3 image = random_image(c.width, c.C, rng, true);
  DNN::Tensor3 want_relu = image;
  for (auto& row : want_relu)
    for (auto& px : row)
      for (double& v : px) v = relu_composite_clear(v);
  TensorCT full = r.model.EncTensor(image, r.pk, c.slotstr);
  TensorCT input = full, relu_input = full;  // a bootstrap's input at 4 limbs, an activation's at 10
  drop_to_limbs(r, input, 4);
  drop_to_limbs(r, relu_input, 10);

  hipStream_t s = r.ctx.stream();
  hipEvent_t e0, e1;
  PHX_CHECK(hipEventCreate(&e0));
  PHX_CHECK(hipEventCreate(&e1));
  auto timed = [&](auto&& f) {
    std::vector<double> ms;
    for (int i = 0; i <= reps; ++i) {  // run 0 warms up
      PHX_CHECK(hipStreamSynchronize(s));
      PHX_CHECK(hipEventRecord(e0, s));
      f();
      PHX_CHECK(hipEventRecord(e1, s));
      PHX_CHECK(hipEventSynchronize(e1));
      float t = 0;
      PHX_CHECK(hipEventElapsedTime(&t, e0, e1));
      if (i) ms.push_back(t);
    }
    return stat(ms);
  };
  bool all = true;
  auto row = [&](const char* op, size_t pack, const Stat& t, double err, size_t bootstraps, size_t rotations) {
    std::printf("{\"bench\": \"%s\", \"stage\": %d, \"log_n\": %d, \"channels\": %zu, \"width\": %zu, \"slotstr\": %zu, "
                "\"ns\": %zu, \"pack\": %zu, \"slots\": %zu, \"reps\": %d, \"device_ms\": {\"median\": %.3f, \"min\": %.3f, "
                "\"max\": %.3f}, \"max_error\": %.6e, \"bootstraps\": %zu, \"tree_rotations\": %zu}\n",
                op, stage, log_n, c.C, c.width, c.slotstr, plan.ns, pack, pack * plan.ns, reps, t.median, t.min, t.max, err,
                bootstraps, rotations);
    std::fflush(stdout);
    all = all && std::isfinite(err);
  };
  const size_t groups = plan.groups(c.C), tree = groups * (c.P - 1);
  TensorCT out;
  for (size_t pack : {size_t(1), c.P}) {
    if ((pack == 1 && side == "packed") || (pack != 1 && side == "pack1")) continue;
    const bool one = pack == 1;
    if (what != "relu") {
      const Stat t = timed([&] { out = r.model.BootStrap(input, r.boot, pack); });
      row("BootStrap", pack, t, tensor_error(r, out, image, 1.0), one ? c.C : groups, one ? 0 : tree);
    }
    if (what != "boot") {
      const Stat t = timed([&] { out = r.model.ReluComposite(relu_input, r.boot, pack); });
      row("ReluComposite", pack, t, tensor_error(r, out, want_relu, 1.0), 3 * (one ? c.C : groups), one ? 0 : 3 * tree);
    }
  }
  PHX_CHECK(hipEventDestroy(e0));
  PHX_CHECK(hipEventDestroy(e1));
  std::printf("{\"done\": \"packboot_example bench\", \"ok\": %s}\n", tf(all));
  return all ? 0 : 1;
}

// Unpack alone, per node against batched, on packed groups at the bootstrap's output level
static int run_tree(int stage, int reps) {
  static const Case stages[] = {{"stage0", 32, 0, 16, 16}, {"stage1", 16, 1, 32, 32}, {"stage2", 8, 2, 64, 32}};
  if (stage < 0 || stage > 2 || reps < 1) throw std::invalid_argument("tree <stage 0..2> [reps]");
  const Case& c = stages[stage];
  const int log_n = 16;
  const size_t limbs = 12;  // what EvalBootstrap returns on this chain
  Rig r(log_n);
  const PackPlan plan = pack_plan(r.n, c.width, c.slotstr, c.P);
  std::vector<int32_t> rots;
  r.model.AddPackRotationsTo(rots, c.width, c.slotstr, c.P);
  r.model.BuildGaloisKey(r.sk, rots);
  std::mt19937_64 rng(0x7EE5);
  TensorCT input = r.model.EncTensor(random_image(c.width, c.C, rng, true), r.pk, c.slotstr);
  drop_to_limbs(r, input, limbs);
  const PackedCT packed = r.model.Pack(input, c.P);
  PHX_CHECK(hipDeviceSynchronize());

  hipStream_t s = r.ctx.stream();
  hipEvent_t e0, e1;
  PHX_CHECK(hipEventCreate(&e0));
  PHX_CHECK(hipEventCreate(&e1));
  TensorCT out[2];
  Stat t[2];
  const DNN::UnpackPath paths[2] = {DNN::UnpackPath::kPerNode, DNN::UnpackPath::kBatched};
  for (int side = 0; side < 2; ++side) {
    r.model.set_unpack_path(paths[side]);
    std::vector<double> ms;
    for (int i = 0; i <= reps; ++i) {  // run 0 warms up
      PHX_CHECK(hipStreamSynchronize(s));
      PHX_CHECK(hipEventRecord(e0, s));
      out[side] = r.model.Unpack(packed);
      PHX_CHECK(hipEventRecord(e1, s));
      PHX_CHECK(hipEventSynchronize(e1));
      float v = 0;
      PHX_CHECK(hipEventElapsedTime(&v, e0, e1));
      if (i) ms.push_back(v);
    }
    t[side] = stat(ms);
  }
  PHX_CHECK(hipEventDestroy(e0));
  PHX_CHECK(hipEventDestroy(e1));
  const bool equal = same_tensor(r.ctx, out[0], out[1]);
  const size_t groups = plan.groups(c.C);
  std::printf("{\"bench\": \"Unpack\", \"stage\": %d, \"log_n\": %d, \"channels\": %zu, \"width\": %zu, \"slotstr\": %zu, "
              "\"pack\": %zu, \"groups\": %zu, \"limbs\": %zu, \"chunk\": %zu, \"tree_rotations\": %zu, \"levels\": %zu, "
              "\"reps\": %d, \"per_node_ms\": {\"median\": %.3f, \"min\": %.3f, \"max\": %.3f}, "
              "\"batched_ms\": {\"median\": %.3f, \"min\": %.3f, \"max\": %.3f}, \"words_equal\": %s}\n",
              stage, log_n, c.C, c.width, c.slotstr, c.P, groups, limbs,
              rotate_fused_batch_chunk(r.ctx, packed.ctks_[0].chain_index()), groups * (c.P - 1), plan.log_pack, reps,
              t[0].median, t[0].min, t[0].max, t[1].median, t[1].min, t[1].max, tf(equal));
  std::printf("{\"done\": \"packboot_example tree\", \"ok\": %s}\n", tf(equal));
  return equal ? 0 : 1;
}

int main(int argc, char** argv) {
  try {
    if (argc >= 3 && !std::strcmp(argv[1], "check")) {
      const int log_n = argc >= 4 ? std::atoi(argv[3]) : 12;
      if (log_n < 12 || log_n > 16) throw std::invalid_argument("log_n must be 12..16");
      if (!std::strcmp(argv[2], "pack")) return run_check_pack(log_n);
      if (!std::strcmp(argv[2], "boot")) return run_check_boot(log_n);
      if (!std::strcmp(argv[2], "relu")) return run_check_relu(log_n);
      if (!std::strcmp(argv[2], "tree")) return run_check_tree(log_n);
    }
    if (argc >= 3 && !std::strcmp(argv[1], "tree")) return run_tree(std::atoi(argv[2]), argc >= 4 ? std::atoi(argv[3]) : 5);
    if (argc >= 3 && !std::strcmp(argv[1], "bench"))
      return run_bench(std::atoi(argv[2]), argc >= 4 ? argv[3] : "both", argc >= 5 ? std::atoi(argv[4]) : 5,
                       argc >= 6 ? argv[5] : "all");
    std::fprintf(stderr, "usage: packboot_example check pack|boot|relu|tree [log_n] | bench <stage> [both|pack1|packed] [reps] "
                         "[boot|relu|all] | tree <stage> [reps]\n");
    return 2;
  } catch (const std::exception& e) {
    std::printf("{\"error\": \"%s\", \"ok\": false}\n", e.what());
    return 1;
  }
}
