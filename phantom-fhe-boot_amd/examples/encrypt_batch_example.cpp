// encrypt_batch_example — PhantomSecretKey's batched members (encrypt_symmetric_batch,
// decrypt_decode_batch; csrc/encrypt.hip) against the one-at-a-time members of the same class,
// through the C++ façade.
//
// usage: encrypt_batch_example check <log_n>
//          N = 2^log_n, CoeffModulus::Create(N, {60, 40, 40, 60}), one special prime, scale 2^40.
//          Two PhantomSecretKey::for_testing keys from the same seed: one encrypts `count`
//          device-encoded plaintexts one by one (encode_device + encrypt_symmetric), the other all
//          at once.  Both draw the same stream in the same order, so every ciphertext word, every
//          recorded seed and the save_symmetric bytes must be equal; then decrypt_decode_batch
//          against decrypt + decode_device per ciphertext, double for double.  One JSON line per
//          check (`mismatches` must be 0); exit status 0 iff all pass.
#include <hip/hip_runtime.h>

#include <algorithm>
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

static std::string symmetric_bytes(const PhantomCiphertext& ct) {
  std::ostringstream os;
  ct.save_symmetric(os);
  return os.str();
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
  // one more than a chunk, so that the batch crosses a chunk boundary
  const size_t count = encrypt_batch_chunk(ctx) + 1;

  std::mt19937_64 rng(0x5EED + log_n);
  std::uniform_real_distribution<double> d(-1.0, 1.0);
  std::vector<cplx> values(count * slots);
  for (auto& x : values) {
    const double re = d(rng);
    x = cplx(re, d(rng));
  }
  DeviceBuffer<cplx> dv;
  dv.upload(values, s);

  for (size_t chain : {size_t(1), size_t(3)}) {
    const std::string note = "chain " + std::to_string(chain);
    PhantomSecretKey seq = PhantomSecretKey::for_testing(ctx, 2024), bat = PhantomSecretKey::for_testing(ctx, 2024);
    std::vector<PhantomCiphertext> a(count), b(count);
    for (size_t p = 0; p < count; ++p) {
      PhantomPlaintext pt;
      enc.encode_device(ctx, dv.get() + p * slots, slots, scale, pt, chain);
      seq.encrypt_symmetric(ctx, pt, a[p]);
    }
    bat.encrypt_symmetric_batch(ctx, enc, dv.get(), slots, scale, chain, b);

    size_t words = 0, seeds = 0, meta = 0, saved = 0;
    for (size_t p = 0; p < count; ++p) {
      words += differing(a[p].to_host(s), b[p].to_host(s));
      seeds += a[p].seed() != b[p].seed() || b[p].seed().size() != PhantomCiphertext::kSeedBytes;
      meta += a[p].chain_index() != b[p].chain_index() || a[p].size() != b[p].size() || a[p].scale() != b[p].scale() ||
              a[p].is_ntt_form() != b[p].is_ntt_form() || a[p].correction_factor() != b[p].correction_factor() ||
              a[p].GetNoiseScaleDeg() != b[p].GetNoiseScaleDeg() || a[p].is_asymmetric() != b[p].is_asymmetric();
      saved += symmetric_bytes(a[p]) != symmetric_bytes(b[p]);
    }
    report("ciphertext_words", log_n, count, words, note.c_str());
    report("recorded_seeds", log_n, count, seeds, note.c_str());
    report("metadata", log_n, count, meta, note.c_str());
    report("save_symmetric_bytes", log_n, count, saved, note.c_str());

    // decrypt + decode: the batch (all limbs, and the two leading limbs where there are more)
    // against decrypt + decode_device per ciphertext
    std::vector<cplx> want(count * slots);
    DeviceBuffer<cplx> one(slots, s), all(count * slots, s);
    for (size_t p = 0; p < count; ++p) {
      const PhantomPlaintext pt = seq.decrypt(ctx, a[p]);
      enc.decode_device(ctx, pt, one.get());
      const std::vector<cplx> v = one.download(s);
      std::copy(v.begin(), v.end(), want.begin() + p * slots);
    }
    bat.decrypt_decode_batch(ctx, enc, b, 0, all.get());
    report("decrypt_decode_batch", log_n, count, differing(all.download(s), want), note.c_str());
    {  // decrypt_batch: the NTT-form plaintexts
      const size_t L = b[0].coeff_modulus_size();
      DeviceBuffer<uint64_t> plain(count * L * n, s);
      bat.decrypt_batch(ctx, b, 0, plain.get());
      const std::vector<uint64_t> got = plain.download(s);
      size_t bad = 0;
      for (size_t p = 0; p < count; ++p) {
        const PhantomPlaintext pt = seq.decrypt(ctx, a[p]);
        std::vector<uint64_t> w(L * n);
        PHX_CHECK(hipMemcpyAsync(w.data(), pt.data(), w.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        PHX_CHECK(hipStreamSynchronize(s));
        bad += std::memcmp(w.data(), got.data() + p * L * n, w.size() * sizeof(uint64_t)) != 0;
      }
      report("decrypt_batch", log_n, count, bad, note.c_str());
    }
    if (b[0].coeff_modulus_size() > 2) {
      // two limbs hold the message: the values agree with the inputs as well as all limbs do
      bat.decrypt_decode_batch(ctx, enc, b, 2, all.get());
      const std::vector<cplx> two = all.download(s);
      double e2 = 0, e3 = 0;
      for (size_t i = 0; i < two.size(); ++i) {
        e2 = std::max(e2, std::abs(two[i] - values[i]));
        e3 = std::max(e3, std::abs(want[i] - values[i]));
      }
      report("decode_two_limbs", log_n, count, e2 <= 4 * e3 ? 0 : 1, note.c_str());
    }
  }

  {  // sparse packing: against encode_sparse_device + encrypt_symmetric
    const size_t ns = slots / 8, c = 3;
    enc.set_sparse_encode(2 * ns);
    PhantomSecretKey seq = PhantomSecretKey::for_testing(ctx, 7), bat = PhantomSecretKey::for_testing(ctx, 7);
    std::vector<PhantomCiphertext> a(c), b(c);
    for (size_t p = 0; p < c; ++p) {
      PhantomPlaintext pt;
      enc.encode_sparse_device(ctx, dv.get() + p * ns, ns, scale, pt, 2);
      seq.encrypt_symmetric(ctx, pt, a[p]);
    }
    bat.encrypt_symmetric_sparse_batch(ctx, enc, dv.get(), ns, scale, 2, b);
    size_t words = 0;
    for (size_t p = 0; p < c; ++p) words += differing(a[p].to_host(s), b[p].to_host(s));
    report("sparse_ciphertext_words", log_n, c, words, "chain 2");
  }

  {  // mixed batches are refused
    PhantomSecretKey k = PhantomSecretKey::for_testing(ctx, 9);
    std::vector<PhantomCiphertext> mixed(2);
    k.encrypt_symmetric_batch(ctx, enc, dv.get(), slots, scale, 1, std::span<PhantomCiphertext>(mixed.data(), 1));
    k.encrypt_symmetric_batch(ctx, enc, dv.get(), slots, scale, 2, std::span<PhantomCiphertext>(mixed.data() + 1, 1));
    DeviceBuffer<cplx> out(2 * slots, s);
    bool threw = false;
    try {
      k.decrypt_decode_batch(ctx, enc, mixed, 0, out.get());
    } catch (const std::invalid_argument&) {
      threw = true;
    }
    report("mixed_batch_throws", log_n, 2, threw ? 0 : 1);
  }
  PHX_CHECK(hipStreamSynchronize(s));
  std::printf("{\"done\": \"encrypt_batch_example check\", \"ok\": %s}\n", g_all ? "true" : "false");
  return g_all ? 0 : 1;
}

int main(int argc, char** argv) {
  try {
    if (argc >= 3 && !std::strcmp(argv[1], "check")) return run_check(std::atoi(argv[2]));
    std::fprintf(stderr, "usage: encrypt_batch_example check <log_n>\n");
    return 2;
  } catch (const std::exception& e) {
    std::printf("{\"error\": \"%s\", \"ok\": false}\n", e.what());
    return 1;
  }
}
