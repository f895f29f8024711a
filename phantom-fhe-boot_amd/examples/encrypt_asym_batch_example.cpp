// encrypt_asym_batch_example — PhantomPublicKey's batched members (encrypt_asymmetric_batch and
// friends; csrc/encrypt.hip) against the one-at-a-time encrypt_asymmetric of the same class, through
// the C++ façade.
//
// usage: encrypt_asym_batch_example check <log_n>
//          N = 2^log_n, CoeffModulus::Create(N, {60, 40, 40, 60}), one special prime, scale 2^40.
//          Two PhantomSecretKey::for_testing keys from the same seed, each with its public key: one
//          encrypts `count` device-encoded plaintexts one by one (encode_device +
//          encrypt_asymmetric), the other all at once.  Both draw the same stream in the same order,
//          so every ciphertext word and the metadata must be equal; then decrypt_decode_batch within
//          the derived noise bound, and a refused call followed by a good one.  One JSON line per
//          check (`mismatches` must be 0); exit status 0 iff all pass.
//        encrypt_asym_batch_example time <log_n> <chain> <count>
//          log_n = 16 takes the bootstrap's key chain ({60, 29 x 59} + 10 x 60), else the chain of
//          `check`.  The batch against the loop of encode + encrypt_asymmetric over the same values (and
//          the same loop with encode_device), in one process, warmed and alternating: 7 wall times
//          each, every one ending in a device synchronise.  One JSON line with the medians and ranges.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../host/encoder.h"
#include "../host/keys.h"
#include "../host/modulus.h"

using namespace phantom;
using namespace phantom::arith;
using cplx = std::complex<double>;

static bool g_all = true;
static void report(const char* name, int log_n, size_t count, size_t mismatches, const char* note = "") {
  const bool ok = mismatches == 0;
  g_all = g_all && ok;
  std::printf("{\"check\": \"%s\", \"log_n\": %d, \"count\": %zu, \"ok\": %s, \"mismatches\": %zu, \"note\": \"%s\"}\n",
              name, log_n, count, ok ? "true" : "false", mismatches, note);
}

template <class T>
static size_t differing(const std::vector<T>& a, const std::vector<T>& b) {
  if (a.size() != b.size()) return a.size() + b.size() + 1;
  size_t d = 0;
  for (size_t i = 0; i < a.size(); ++i) d += std::memcmp(&a[i], &b[i], sizeof(T)) != 0;
  return d;
}

static bool same_metadata(const PhantomCiphertext& a, const PhantomCiphertext& b) {
  return a.chain_index() == b.chain_index() && a.size() == b.size() && a.scale() == b.scale() &&
         a.is_ntt_form() == b.is_ntt_form() && a.correction_factor() == b.correction_factor() &&
         a.GetNoiseScaleDeg() == b.GetNoiseScaleDeg() && a.is_asymmetric() == b.is_asymmetric() &&
         a.seed() == b.seed() && a.coeff_modulus_size() == b.coeff_modulus_size();
}

static std::vector<cplx> random_values(size_t count, uint64_t seed) {
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> d(-1.0, 1.0);
  std::vector<cplx> values(count);
  for (auto& x : values) {
    const double re = d(rng);
    x = cplx(re, d(rng));
  }
  return values;
}

static int run_check(int log_n) {
  const size_t n = size_t(1) << log_n, slots = n / 2;
  EncryptionParameters parms(scheme_type::ckks);
  parms.set_poly_modulus_degree(n);
  parms.set_special_modulus_size(1);
  parms.set_coeff_modulus(CoeffModulus::Create(n, {60, 40, 40, 60}));
  PhantomContext ctx(parms);
  PhantomCKKSEncoder enc(ctx);
  hipStream_t s = ctx.stream();
  const double scale = std::ldexp(1.0, 40);
  const size_t alpha = ctx.size_P();
  // one more than a chunk, so that the batch crosses a chunk boundary
  const size_t count = encrypt_asymmetric_batch_chunk(ctx, 1) + 1;
  const std::vector<cplx> values = random_values(count * slots, 0x5EED + log_n);
  DeviceBuffer<cplx> dv;
  dv.upload(values, s);
  // |c0 + c1 s - m| <= alpha (n + 1) + 1 per coefficient, plus half a unit of rounding, all n terms of
  // a slot aligned
  const double bound = static_cast<double>(n) * (alpha * (n + 1.0) + 1.5) / scale;

  for (size_t chain : {size_t(1), size_t(3)}) {
    const std::string note = "chain " + std::to_string(chain);
    PhantomSecretKey seq = PhantomSecretKey::for_testing(ctx, 2024), bat = PhantomSecretKey::for_testing(ctx, 2024);
    PhantomPublicKey seq_pk = seq.gen_publickey(ctx), bat_pk = bat.gen_publickey(ctx);
    std::vector<PhantomCiphertext> a(count), b(count);
    for (size_t p = 0; p < count; ++p) {
      PhantomPlaintext pt;
      enc.encode_device(ctx, dv.get() + p * slots, slots, scale, pt, chain);
      seq_pk.encrypt_asymmetric(ctx, pt, a[p]);
    }
    bat_pk.encrypt_asymmetric_batch(ctx, enc, dv.get(), slots, scale, chain, b);

    size_t words = 0, meta = 0, throws = 0;
    for (size_t p = 0; p < count; ++p) {
      words += differing(a[p].to_host(s), b[p].to_host(s));
      meta += !same_metadata(a[p], b[p]) || !b[p].is_asymmetric() || !b[p].seed().empty();
      bool threw = false;
      try {
        std::ostringstream os;
        b[p].save_symmetric(os);
      } catch (const std::exception&) {
        threw = true;
      }
      throws += !threw;
    }
    report("ciphertext_words", log_n, count, words, note.c_str());
    report("metadata", log_n, count, meta, note.c_str());
    report("save_symmetric_throws", log_n, count, throws, note.c_str());

    DeviceBuffer<cplx> all(count * slots, s);
    bat.decrypt_decode_batch(ctx, enc, b, 0, all.get());
    const std::vector<cplx> got = all.download(s);
    double err = 0;
    for (size_t i = 0; i < got.size(); ++i) err = std::max(err, std::abs(got[i] - values[i]));
    char buf[96];
    std::snprintf(buf, sizeof buf, "%s max error %.3e bound %.3e", note.c_str(), err, bound);
    report("decrypt_decode_batch", log_n, count, err < bound ? 0 : 1, buf);

    // a refused call (chain index 0) uses no draw: the next batch still matches the loop
    bool threw = false;
    try {
      std::vector<PhantomCiphertext> none(2);
      bat_pk.encrypt_asymmetric_batch(ctx, enc, dv.get(), slots, scale, 0, none);
    } catch (const std::invalid_argument&) {
      threw = true;
    }
    std::vector<PhantomCiphertext> a2(3), b2(3);
    for (size_t p = 0; p < 3; ++p) {
      PhantomPlaintext pt;
      enc.encode_device(ctx, dv.get() + p * slots, slots, scale, pt, chain);
      seq_pk.encrypt_asymmetric(ctx, pt, a2[p]);
    }
    bat_pk.encrypt_asymmetric_batch(ctx, enc, dv.get(), slots, scale, chain, b2);
    size_t after = threw ? 0 : 1;
    for (size_t p = 0; p < 3; ++p) after += differing(a2[p].to_host(s), b2[p].to_host(s));
    report("refused_call_restores_the_stream", log_n, 3, after, note.c_str());

    // the strided form takes the same draws
    const size_t L = b2[0].coeff_modulus_size(), ct_words = 2 * L * n, stride = ct_words + 4;
    DeviceBuffer<uint64_t> flat(3 * stride, s);
    for (size_t p = 0; p < 3; ++p) {
      PhantomPlaintext pt;
      enc.encode_device(ctx, dv.get() + p * slots, slots, scale, pt, chain);
      seq_pk.encrypt_asymmetric(ctx, pt, a2[p]);
    }
    bat_pk.encrypt_asymmetric_batch_to(ctx, dv.get(), slots, 0, scale, chain, 3, flat.get(), stride);
    const std::vector<uint64_t> f = flat.download(s);
    size_t bad = 0;
    for (size_t p = 0; p < 3; ++p)
      bad += differing(a2[p].to_host(s), std::vector<uint64_t>(f.begin() + p * stride, f.begin() + p * stride + ct_words));
    report("batch_to_words", log_n, 3, bad, note.c_str());
  }

  {  // sparse packing: against encode_sparse_device + encrypt_asymmetric
    const size_t ns = slots / 8, c = 3;
    enc.set_sparse_encode(2 * ns);
    PhantomSecretKey seq = PhantomSecretKey::for_testing(ctx, 7), bat = PhantomSecretKey::for_testing(ctx, 7);
    PhantomPublicKey seq_pk = seq.gen_publickey(ctx), bat_pk = bat.gen_publickey(ctx);
    std::vector<PhantomCiphertext> a(c), b(c);
    for (size_t p = 0; p < c; ++p) {
      PhantomPlaintext pt;
      enc.encode_sparse_device(ctx, dv.get() + p * ns, ns, scale, pt, 2);
      seq_pk.encrypt_asymmetric(ctx, pt, a[p]);
    }
    bat_pk.encrypt_asymmetric_sparse_batch(ctx, enc, dv.get(), ns, scale, 2, b);
    size_t words = 0;
    for (size_t p = 0; p < c; ++p) words += differing(a[p].to_host(s), b[p].to_host(s));
    report("sparse_ciphertext_words", log_n, c, words, "chain 2");
  }

  {  // an ungenerated key throws, as encrypt_asymmetric does
    PhantomPublicKey empty;
    std::vector<PhantomCiphertext> one(1);
    bool threw = false;
    try {
      empty.encrypt_asymmetric_batch(ctx, enc, dv.get(), slots, scale, 1, one);
    } catch (const std::invalid_argument&) {
      threw = true;
    }
    report("ungenerated_key_throws", log_n, 1, threw ? 0 : 1);
  }
  PHX_CHECK(hipStreamSynchronize(s));
  std::printf("{\"done\": \"encrypt_asym_batch_example check\", \"ok\": %s}\n", g_all ? "true" : "false");
  return g_all ? 0 : 1;
}

static int run_time(int log_n, size_t chain, size_t count) {
  const size_t n = size_t(1) << log_n, slots = n / 2;
  EncryptionParameters parms(scheme_type::ckks);
  parms.set_poly_modulus_degree(n);
  std::vector<int> bits = {60, 40, 40, 60};
  size_t special = 1;
  if (log_n == 16) {
    bits.assign(1, 60);
    bits.insert(bits.end(), 29, 59);
    bits.insert(bits.end(), 10, 60);
    special = 10;
  }
  parms.set_special_modulus_size(special);
  parms.set_coeff_modulus(CoeffModulus::Create(n, bits));
  PhantomContext ctx(parms);
  PhantomCKKSEncoder enc(ctx);
  hipStream_t s = ctx.stream();
  const double scale = std::ldexp(1.0, 40);
  if (count < 1 || chain < 1 || chain >= ctx.total_parm_size()) throw std::invalid_argument("bad chain or count");
  PhantomSecretKey sk = PhantomSecretKey::for_testing(ctx, 1);
  PhantomPublicKey pk = sk.gen_publickey(ctx);
  const std::vector<cplx> values = random_values(count * slots, 99);
  DeviceBuffer<cplx> dv;
  dv.upload(values, s);
  std::vector<PhantomCiphertext> a(count), b(count);
  using clock = std::chrono::steady_clock;
  auto ms_since = [](clock::time_point t0) { return std::chrono::duration<double, std::milli>(clock::now() - t0).count(); };
  // the loop as a caller writes it today (host encoder), and with the device encoder in its place
  auto loop = [&](bool device_encode) {
    PHX_CHECK(hipStreamSynchronize(s));
    const auto t0 = clock::now();
    for (size_t p = 0; p < count; ++p) {
      PhantomPlaintext pt;
      if (device_encode)
        enc.encode_device(ctx, dv.get() + p * slots, slots, scale, pt, chain);
      else
        enc.encode(ctx, std::vector<cplx>(values.begin() + p * slots, values.begin() + (p + 1) * slots), scale, pt,
                   chain);
      pk.encrypt_asymmetric(ctx, pt, a[p]);
    }
    PHX_CHECK(hipStreamSynchronize(s));
    return ms_since(t0);
  };
  auto batch = [&] {
    PHX_CHECK(hipStreamSynchronize(s));
    const auto t0 = clock::now();
    pk.encrypt_asymmetric_batch(ctx, enc, dv.get(), slots, scale, chain, b);
    PHX_CHECK(hipStreamSynchronize(s));
    return ms_since(t0);
  };
  for (int w = 0; w < 2; ++w) {  // warm: code objects, pool, workspace
    loop(false);
    loop(true);
    batch();
  }
  std::vector<double> tl, td, tb;
  for (int r = 0; r < 7; ++r) {
    tl.push_back(loop(false));
    td.push_back(loop(true));
    tb.push_back(batch());
  }
  std::sort(tl.begin(), tl.end());
  std::sort(td.begin(), td.end());
  std::sort(tb.begin(), tb.end());
  std::printf("{\"time\": \"encrypt_asymmetric\", \"log_n\": %d, \"chain\": %zu, \"limbs\": %zu, \"count\": %zu, "
              "\"chunk\": %zu, \"loop_ms\": {\"median\": %.3f, \"min\": %.3f, \"max\": %.3f}, "
              "\"loop_device_encode_ms\": {\"median\": %.3f, \"min\": %.3f, \"max\": %.3f}, "
              "\"batch_ms\": {\"median\": %.3f, \"min\": %.3f, \"max\": %.3f}, \"speedup\": %.2f, "
              "\"speedup_device_encode\": %.2f}\n",
              log_n, chain, b[0].coeff_modulus_size(), count, encrypt_asymmetric_batch_chunk(ctx, chain), tl[3], tl[0],
              tl[6], td[3], td[0], td[6], tb[3], tb[0], tb[6], tl[3] / tb[3], td[3] / tb[3]);
  std::printf("{\"done\": \"encrypt_asym_batch_example time\", \"ok\": true}\n");
  return 0;
}

int main(int argc, char** argv) {
  try {
    if (argc >= 3 && !std::strcmp(argv[1], "check")) return run_check(std::atoi(argv[2]));
    if (argc >= 5 && !std::strcmp(argv[1], "time"))
      return run_time(std::atoi(argv[2]), std::strtoull(argv[3], nullptr, 10), std::strtoull(argv[4], nullptr, 10));
    std::fprintf(stderr, "usage: encrypt_asym_batch_example check <log_n> | time <log_n> <chain> <count>\n");
    return 2;
  } catch (const std::exception& e) {
    std::printf("{\"error\": \"%s\", \"ok\": false}\n", e.what());
    return 1;
  }
}
