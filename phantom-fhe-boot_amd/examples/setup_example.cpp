// setup_example — EvalBootstrapSetup on the device (FHECKKSRNS::UseDeviceSetup) against the host
// setup, on one context and one key.
//
// usage: setup_example check LOGN [SLOTS]   |   setup_example time LOGN
//   check: a host-setup, a device-setup and a second host-setup FHECKKSRNS with the example's
//          parameters (Q = {60, 29 x 59}, P = 10 x 60, scale 2^59, levelBudget {2, 2}; SLOTS = 0 or
//          absent: full packing).  Reports the equality of rotation indices, output chain and level
//          shapes; per level of Eval{CoeffsToSlots,SlotsToCoeffs}Precompute the largest centred
//          coefficient difference between corresponding plaintexts (bound 1 + 4 e_host scale, e_host =
//          the host embedding's error on that level's diagonals against long double) and how many
//          coefficients differ; a dense EvalLinearTransformPrecompute through the host path, the
//          device path and the device-pointer overload; one bootstrap through each setup.  Every
//          level row and the dense row carry "hash": FNV-1a 64 fingerprints of the plaintext sets
//          (slot, chain, scale bits and raw device words of each present plaintext), and one row
//          that of rotation_indices: two builds compute the same setup iff these lines agree.
//   time : wall-clock medians of the host setup, the device setup and the structure-only setup
//          (precompute = false), each bracketed by hipDeviceSynchronize, and the pool's peak
//          during a device setup (in all, and beyond the plaintexts the setup keeps).
// Prints one JSON object per line; exit status 0 iff every check holds.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../host/bootstrap.h"
#include "../host/ckks_eval.h"
#include "../host/encoder.h"
#include "../host/evaluate.h"
#include "../host/keys.h"
#include "../host/modulus.h"
#include "../host/numth.h"
#include "../csrc/ntt.h"

using namespace phantom;
using namespace phantom::arith;
using cplx = std::complex<double>;
using lcplx = std::complex<long double>;
using PlainSet = std::vector<std::vector<std::shared_ptr<PhantomPlaintext>>>;

static bool g_ok = true;

static void check(const char* name, bool ok, const std::string& extra = "") {
  g_ok = g_ok && ok;
  std::printf("{\"check\": \"%s\", \"ok\": %s%s%s}\n", name, ok ? "true" : "false", extra.empty() ? "" : ", ",
              extra.c_str());
  std::fflush(stdout);
}

static double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// bootstrapping_example.cu:17-41
static double compute_bit_precision(const std::vector<double>& ref, const std::vector<double>& actual) {
  double sum = 0.0;
  int cnt = 0;
  for (size_t i = 0; i < ref.size(); ++i) {
    if (std::abs(ref[i]) < 1e-20) continue;
    double rel = std::abs(ref[i] - actual[i]) / std::abs(ref[i]);
    if (rel < 1e-40) rel = 1e-40;
    sum += -std::log2(rel);
    ++cnt;
  }
  return cnt ? sum / cnt : 0.0;
}

// inverse canonical embedding in long double (radix 2, slot j at zeta^(5^j)): the FP yardstick
static std::vector<long double> slots_to_coeffs_ld(const std::vector<cplx>& values, size_t n) {
  const long double pi = std::acos(-1.0L);
  const size_t m = 2 * n;
  static std::vector<lcplx> zeta;
  if (zeta.size() != m) {
    zeta.resize(m);
    for (size_t j = 0; j < m; ++j) zeta[j] = lcplx(std::cos(2 * pi * j / m), std::sin(2 * pi * j / m));
  }
  std::vector<lcplx> a(n, lcplx(0, 0));
  uint64_t p = 1;
  for (size_t j = 0; j < values.size(); ++j) {
    const size_t idx = (p - 1) / 2;
    a[idx] = lcplx(values[j].real(), values[j].imag());
    a[n - 1 - idx] = std::conj(a[idx]);
    p = (p * 5) % m;
  }
  const int logn = log2_exact(n);
  for (size_t i = 0; i < n; ++i) {
    const size_t r = reverse_bits(static_cast<uint32_t>(i), logn);
    if (i < r) std::swap(a[i], a[r]);
  }
  for (size_t len = 2; len <= n; len <<= 1)
    for (size_t i = 0; i < n; i += len)
      for (size_t j = 0; j < len / 2; ++j) {
        const lcplx w = std::conj(zeta[j * (m / len)]);
        const lcplx u = a[i + j], v = a[i + j + len / 2] * w;
        a[i + j] = u + v;
        a[i + j + len / 2] = u - v;
      }
  std::vector<long double> c(n);
  for (size_t k = 0; k < n; ++k) c[k] = (std::conj(zeta[k]) * a[k]).real() / static_cast<long double>(n);
  return c;
}

// coefficient form of an extended plaintext on the host ([limbs][n])
static std::vector<uint64_t> ext_coefficients(const PhantomContext& ctx, const PhantomPlaintext& pt) {
  hipStream_t s = ctx.stream();
  const phx::LimbMap map = encode_limb_map(ctx, pt.chain_index(), true);
  DeviceBuffer<uint64_t> tmp(static_cast<size_t>(map.num_limbs) * ctx.poly_degree(), s);
  PHX_CHECK(phx::ntt_inverse(ctx.gpu_rns_tables(), pt.data(), tmp.get(), map, nullptr, nullptr, s));
  return tmp.download(s);
}

// FNV-1a 64 of a plaintext set: for each present slot in order, the slot index, the chain index,
// the scale's bit pattern and the plaintext's raw device words (a fingerprint to compare two builds by)
struct Fnv {
  uint64_t h = 0xcbf29ce484222325ull;
  void eat(const void* p, size_t bytes) {
    const unsigned char* c = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < bytes; ++i) h = (h ^ c[i]) * 0x100000001b3ull;
  }
  void word(uint64_t w) { eat(&w, sizeof(w)); }
  std::string hex() const {
    char buf[20];
    std::snprintf(buf, sizeof(buf), "%016llx", static_cast<unsigned long long>(h));
    return buf;
  }
};

static std::string set_hash(const PhantomContext& ctx, const std::vector<std::shared_ptr<PhantomPlaintext>>& set) {
  Fnv f;
  std::vector<uint64_t> words;
  PHX_CHECK(hipStreamSynchronize(ctx.stream()));  // the set's encodings are queued on the stream
  for (size_t u = 0; u < set.size(); ++u) {
    if (!set[u]) continue;
    const double scale = set[u]->scale();
    uint64_t bits;
    std::memcpy(&bits, &scale, sizeof(bits));
    f.word(u);
    f.word(set[u]->chain_index());
    f.word(bits);
    words.resize(set[u]->coeff_modulus_size() * set[u]->poly_modulus_degree());
    PHX_CHECK(hipMemcpy(words.data(), set[u]->data(), words.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    f.eat(words.data(), words.size() * sizeof(uint64_t));
  }
  return f.hex();
}

struct SetDiff {
  bool same_structure = true;  // sizes, which plaintexts exist, chain indices, scales
  double max_diff = 0;         // centred coefficient difference
  size_t differing = 0, coefficients = 0, plaintexts = 0;
};

static SetDiff compare(const PhantomContext& ctx, const std::vector<std::shared_ptr<PhantomPlaintext>>& a,
                       const std::vector<std::shared_ptr<PhantomPlaintext>>& b) {
  SetDiff d;
  d.same_structure = a.size() == b.size();
  const size_t n = ctx.poly_degree();
  for (size_t u = 0; u < std::min(a.size(), b.size()); ++u) {
    if (!a[u] || !b[u]) {
      d.same_structure = d.same_structure && !a[u] && !b[u];
      continue;
    }
    if (a[u]->chain_index() != b[u]->chain_index() || a[u]->scale() != b[u]->scale() ||
        a[u]->coeff_modulus_size() != b[u]->coeff_modulus_size()) {
      d.same_structure = false;
      continue;
    }
    const std::vector<uint64_t> ca = ext_coefficients(ctx, *a[u]), cb = ext_coefficients(ctx, *b[u]);
    const size_t chain = a[u]->chain_index(), size_Ql = ctx.get_context_data(chain).coeff_modulus_size();
    std::vector<uint64_t> mods(ctx.key_moduli().begin(), ctx.key_moduli().begin() + size_Ql);
    mods.insert(mods.end(), ctx.key_moduli().begin() + ctx.size_Q(), ctx.key_moduli().end());
    ++d.plaintexts;
    for (size_t k = 0; k < n; ++k) {
      bool differs = false;
      for (size_t l = 0; l < mods.size(); ++l) {
        const uint64_t q = mods[l], x = ca[l * n + k], y = cb[l * n + k];
        const uint64_t e = x >= y ? x - y : y - x;
        d.max_diff = std::max(d.max_diff, static_cast<double>(std::min(e, q - e)));
        differs = differs || e;
      }
      d.differing += differs;
      ++d.coefficients;
    }
  }
  return d;
}

struct Params {
  EncryptionParameters parms{scheme_type::ckks};
  double scale = std::pow(2.0, 59);
  std::vector<uint32_t> budget = {2, 2};
};

static Params make_params(int log_n) {
  Params p;
  const int depth = 29, special = 10;
  std::vector<int> bits;
  for (int i = 0; i < depth + 1 + special; ++i) bits.push_back(i == 0 ? 60 : (i < depth + 1 ? 59 : 60));
  p.parms.set_poly_modulus_degree(size_t(1) << log_n);
  p.parms.set_special_modulus_size(special);
  p.parms.set_coeff_modulus(CoeffModulus::Create(size_t(1) << log_n, bits));
  return p;
}

static int run_check(int log_n, uint32_t slots_in) {
  const size_t N = size_t(1) << log_n, n = N / 2;
  const uint32_t slots = slots_in ? slots_in : static_cast<uint32_t>(n);
  const int logslots = log2_exact(slots);
  Params P = make_params(log_n);
  PhantomContext ctx(P.parms);
  PhantomSecretKey sk = PhantomSecretKey::for_testing(ctx, 0x5EED);
  PhantomCKKSEncoder enc(ctx);
  if (slots < n) enc.set_sparse_encode(2 * size_t(slots));
  const std::vector<double> sf = precompute_scaling_factors(ctx, P.scale);
  hipStream_t s = ctx.stream();

  FHECKKSRNS host(enc), dev(enc), host2(enc);
  dev.UseDeviceSetup(true);
  check("option_default_off", !host.device_setup() && dev.device_setup());
  for (FHECKKSRNS* b : {&host, &dev, &host2}) b->EvalBootstrapSetup(ctx, P.budget, P.scale, sf, 0, slots);

  // ---- structure
  const uint32_t M = static_cast<uint32_t>(2 * N);
  check("rotation_indices_equal", host.rotation_indices(slots) == dev.rotation_indices(slots));
  check("find_rotation_indices_equal",
        host.FindBootstrapRotationIndices(slots, M) == dev.FindBootstrapRotationIndices(slots, M) &&
            host.FindCoeffsToSlotsRotationIndices(slots, M) == dev.FindCoeffsToSlotsRotationIndices(slots, M) &&
            host.FindSlotsToCoeffsRotationIndices(slots, M) == dev.FindSlotsToCoeffsRotationIndices(slots, M));
  {
    Fnv f;
    for (int r : host.rotation_indices(slots)) f.word(static_cast<uint64_t>(r));
    std::printf("{\"hashes\": \"rotation_indices\", \"hash\": \"%s\"}\n", f.hex().c_str());
  }
  check("output_chain_equal", host.output_chain_index(slots) == dev.output_chain_index(slots),
        "\"chain\": " + std::to_string(dev.output_chain_index(slots)));

  // ---- the level plaintexts through the reference-signature precompute calls
  std::vector<cplx> ksi(2 * N);
  for (size_t j = 0; j < 2 * N; ++j) {
    const double a = 2.0 * M_PI * static_cast<double>(j) / static_cast<double>(2 * N);
    ksi[j] = cplx(std::cos(a), std::sin(a));
  }
  std::vector<uint32_t> rot(slots);
  uint64_t g5 = 1;
  for (uint32_t j = 0; j < slots; ++j, g5 = g5 * 5 % (2 * N)) rot[j] = static_cast<uint32_t>(g5);
  for (int dir = 0; dir < 2; ++dir) {
    const bool encode_dir = dir == 0, flag_i = dir == 1;
    const double constant = encode_dir ? 0.75 : 1.25;
    auto sets = [&](const FHECKKSRNS& b) {
      return encode_dir ? b.EvalCoeffsToSlotsPrecompute(ctx, ksi, rot, sf, flag_i, constant, 0)
                        : b.EvalSlotsToCoeffsPrecompute(ctx, ksi, rot, sf, flag_i, constant, 0);
    };
    const PlainSet ph = sets(host), pd = sets(dev), ph2 = sets(host2);
    // the levels as EvalBootstrapSetup plans them (SlotToCoeff: the mirror image of the split)
    std::vector<int> sizes = boot::split_stages(logslots, P.budget[dir]);
    if (!encode_dir) std::reverse(sizes.begin(), sizes.end());
    const std::vector<boot::LevelSpec> specs = boot::plan_levels(slots, n, sizes, encode_dir);
    bool levels_ok = ph.size() == pd.size() && ph.size() == specs.size() && ph.size() == ph2.size();
    for (size_t gi = 0; levels_ok && gi < ph.size(); ++gi) {
      // the level's diagonals as the host setup forms them: their embedding error, and the shape they imply
      const boot::LevelSpec& spec = specs[gi];
      boot::LtShape shape;
      const std::vector<boot::FinishedDiagonal> diags = boot::finish_host(
          boot::stage_products_host(boot::plan_stages(slots, spec.stages), encode_dir), slots, n,
          flag_i ? cplx(0.0, constant) : cplx(constant, 0.0), spec.apply_const, spec.mask, 0, spec.stride, shape);
      double e_host = 0;
      for (const auto& d : diags) {
        const std::vector<long double> want = slots_to_coeffs_ld(d.values, N);
        const std::vector<double> got = enc.slots_to_coeffs(d.values);
        for (size_t k = 0; k < N; ++k) e_host = std::max(e_host, static_cast<double>(std::fabs(got[k] - want[k])));
      }
      size_t present = 0;
      bool twin_ok = static_cast<size_t>(shape.D) == pd[gi].size();
      for (const auto& p : pd[gi]) present += p != nullptr;
      twin_ok = twin_ok && present == diags.size();
      for (const auto& d : diags) twin_ok = twin_ok && static_cast<size_t>(d.slot) < pd[gi].size() && pd[gi][d.slot];
      const double lvl_scale = sf.at(gi);  // chain 1 + gi
      const double bound = 1 + 4 * e_host * lvl_scale;
      const SetDiff hd = compare(ctx, ph[gi], pd[gi]), hh = compare(ctx, ph[gi], ph2[gi]);
      char buf[768];
      std::snprintf(buf, sizeof(buf),
                    "\"dir\": \"%s\", \"level\": %zu, \"D\": %zu, \"present\": %zu, \"max_diff\": %.1f, \"bound\": %.1f, "
                    "\"e_host\": %.3e, \"differing\": %zu, \"coefficients\": %zu, \"host_vs_host_differing\": %zu, "
                    "\"hash\": {\"host\": \"%s\", \"device\": \"%s\", \"host2\": \"%s\"}",
                    encode_dir ? "CoeffsToSlots" : "SlotsToCoeffs", gi, pd[gi].size(), present, hd.max_diff, bound,
                    e_host, hd.differing, hd.coefficients, hh.differing, set_hash(ctx, ph[gi]).c_str(),
                    set_hash(ctx, pd[gi]).c_str(), set_hash(ctx, ph2[gi]).c_str());
      check("level_shape_equal", hd.same_structure && twin_ok, buf);
      check("level_plaintexts_within_encoder_bound", hd.plaintexts == present && hd.max_diff <= bound, buf);
      check("host_setup_bit_identical", hh.same_structure && hh.differing == 0 && hh.plaintexts == present, buf);
    }
    check("level_count_equal", levels_ok);
  }

  // ---- dense linear transform: a few non-zero diagonals, through the three paths
  {
    std::mt19937_64 rng(0xD1A6);
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    std::vector<std::vector<cplx>> A(n, std::vector<cplx>(n, cplx(0, 0)));
    std::vector<size_t> ks = {0, 1, 2, 31, 32, 33, n / 2, n - 1};
    for (size_t k : ks)
      for (size_t p = 0; p < n; ++p) A[p][(p + k) % n] = cplx(u(rng), u(rng));
    std::vector<cplx> flat(n * n);
    for (size_t p = 0; p < n; ++p) std::copy(A[p].begin(), A[p].end(), flat.begin() + p * n);
    DeviceBuffer<cplx> dA;
    dA.upload(flat, s);
    const uint32_t L = static_cast<uint32_t>(ctx.size_Q() - 3);  // few limbs: chain 1 + L
    const double sc = 0.5;
    const auto th = host.EvalLinearTransformPrecompute(ctx, A, sc, L);
    const auto td = dev.EvalLinearTransformPrecompute(ctx, A, sc, L);
    const auto tp = host.EvalLinearTransformPrecompute(ctx, dA.get(), sc, L);
    double e_host = 0;
    for (size_t k : ks) {
      std::vector<cplx> d(n);
      for (size_t p = 0; p < n; ++p) d[p] = A[p][(p + k) % n] * sc;
      const std::vector<long double> want = slots_to_coeffs_ld(d, N);
      const std::vector<double> got = enc.slots_to_coeffs(d);
      for (size_t c = 0; c < N; ++c) e_host = std::max(e_host, static_cast<double>(std::fabs(got[c] - want[c])));
    }
    const double bound = 1 + 4 * e_host * sf.at(L);
    const SetDiff d1 = compare(ctx, th, td), d2 = compare(ctx, td, tp);
    char buf[512];
    std::snprintf(buf, sizeof(buf), "\"diagonals\": %zu, \"max_diff\": %.1f, \"bound\": %.1f, \"differing\": %zu, "
                  "\"hash\": {\"host\": \"%s\", \"device\": \"%s\", \"device_pointer\": \"%s\"}",
                  d1.plaintexts, d1.max_diff, bound, d1.differing, set_hash(ctx, th).c_str(), set_hash(ctx, td).c_str(),
                  set_hash(ctx, tp).c_str());
    check("dense_device_vs_host", d1.same_structure && d1.plaintexts == ks.size() && d1.max_diff <= bound, buf);
    check("dense_device_pointer_equals_device_path", d2.same_structure && d2.plaintexts == ks.size() && d2.differing == 0);
  }

  // ---- one bootstrap through each setup, the same input
  {
    std::mt19937_64 rng(0xB007);
    std::uniform_real_distribution<double> dis(1.0, 5.0);
    std::vector<double> x(slots);
    for (auto& v : x) v = dis(rng);
    const size_t chain = ctx.size_Q() - 4;
    PhantomPlaintext pt;
    if (slots < n) enc.encode_sparse(ctx, x, sf.at(chain - 1), pt, chain);
    else enc.encode(ctx, x, sf.at(chain - 1), pt, chain);
    PhantomCiphertext ct;
    sk.encrypt_symmetric(ctx, pt, ct);
    double bits[2] = {0, 0};
    std::vector<uint64_t> words[2];
    size_t out_chain[2] = {0, 0};
    int i = 0;
    for (FHECKKSRNS* b : {&host, &dev}) {
      // the same seeded key once more, so both objects draw identical evaluation keys
      PhantomSecretKey sk_b = PhantomSecretKey::for_testing(ctx, 0x5EED);
      b->EvalMultKeyGen(sk_b, ctx);
      b->EvalBootstrapKeyGen(sk_b, ctx, slots);
      const PhantomCiphertext out = b->EvalBootstrap(ct, ctx, slots);
      PHX_CHECK(hipDeviceSynchronize());
      out_chain[i] = out.chain_index();
      words[i].resize(out.size() * out.coeff_modulus_size() * N);
      PHX_CHECK(hipMemcpy(words[i].data(), out.data(), words[i].size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
      PhantomPlaintext dec;
      sk.decrypt(ctx, out, dec);
      std::vector<double> z;
      enc.decode(ctx, dec, z);
      z.resize(slots);
      bits[i++] = compute_bit_precision(x, z);
    }
    char buf[256];
    std::snprintf(buf, sizeof(buf), "\"avg_bits_host\": %.4f, \"avg_bits_device\": %.4f, \"outputs_bit_identical\": %s, "
                  "\"chain_out\": %zu",
                  bits[0], bits[1], words[0] == words[1] ? "true" : "false", out_chain[1]);
    check("bootstrap_precision", bits[1] >= bits[0] - 0.05 && out_chain[0] == out_chain[1] &&
                                     out_chain[1] == dev.output_chain_index(slots), buf);
  }
  std::printf("{\"done\": \"setup_example check\", \"ok\": %s}\n", g_ok ? "true" : "false");
  return g_ok ? 0 : 1;
}

static double median(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}

static int run_time(int log_n) {
  const size_t N = size_t(1) << log_n;
  Params P = make_params(log_n);
  PhantomContext ctx(P.parms);
  PhantomCKKSEncoder enc(ctx);
  const std::vector<double> sf = precompute_scaling_factors(ctx, P.scale);
  std::vector<double> sf_big(sf.size() - 1);
  for (size_t k = 0; k < sf_big.size(); ++k) sf_big[k] = sf[k] * sf[k];
  (void)ctx.embed_tables();
  const int runs = 3;
  std::vector<double> t_host, t_dev, t_struct;
  size_t peak = 0, base = 0, plain = 0;
  for (int r = 0; r < runs + 1; ++r) {  // the first round warms the pool and the tables up
    for (int which = 0; which < 3; ++which) {
      FHECKKSRNS b(enc);
      b.UseDeviceSetup(which == 1);
      PHX_CHECK(hipDeviceSynchronize());
      if (which == 1) {
        DevicePool::instance().reset_peak();
        base = DevicePool::instance().stats().live;
      }
      const double t0 = now_ms();
      if (which == 2) b.EvalBootstrapSetup(ctx, P.budget, P.scale, sf, sf_big, {0, 0}, 0, 0, false);
      else b.EvalBootstrapSetup(ctx, P.budget, P.scale, sf, 0, 0);
      PHX_CHECK(hipDeviceSynchronize());
      const double ms = now_ms() - t0;
      if (which == 1) {
        const DevicePool::Stats st = DevicePool::instance().stats();
        peak = st.peak_live - base;
        plain = st.live - base;  // what the setup keeps: its plaintexts (and their pointer tables)
      }
      if (r == 0) continue;
      (which == 0 ? t_host : which == 1 ? t_dev : t_struct).push_back(ms);
    }
  }
  std::printf("{\"stage\": \"setup_time\", \"log_n\": %d, \"N\": %zu, \"runs\": %d, \"host_setup_ms\": %.2f, "
              "\"device_setup_ms\": %.2f, \"structure_only_ms\": %.2f, \"device_setup_peak_bytes\": %zu, "
              "\"plaintext_bytes\": %zu, \"peak_beyond_plaintexts_bytes\": %zu}\n",
              log_n, N, runs, median(t_host), median(t_dev), median(t_struct), peak, plain, peak - plain);
  for (int r = 0; r < runs; ++r)
    std::printf("{\"run\": %d, \"host_setup_ms\": %.2f, \"device_setup_ms\": %.2f, \"structure_only_ms\": %.2f}\n", r,
                t_host[r], t_dev[r], t_struct[r]);
  std::printf("{\"done\": \"setup_example time\", \"ok\": true}\n");
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "check";
  const int log_n = argc > 2 ? std::atoi(argv[2]) : 12;
  if ((mode != "check" && mode != "time") || log_n < 10 || log_n > 17) {
    std::fprintf(stderr, "usage: setup_example check LOGN [SLOTS] | setup_example time LOGN\n");
    return 2;
  }
  try {
    if (mode == "time") return run_time(log_n);
    return run_check(log_n, argc > 3 ? static_cast<uint32_t>(std::atoi(argv[3])) : 0);
  } catch (const std::exception& e) {
    std::printf("{\"error\": \"%s\"}\n", e.what());
    return 1;
  }
}
