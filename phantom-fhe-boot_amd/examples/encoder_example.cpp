// encoder_example — the device CKKS encoder / decoder (PhantomCKKSEncoder's *_device members,
// csrc/encode.hip) against the host members of the same class, through the C++ façade.
//
// usage: encoder_example check <log_n>
//          N = 2^log_n, CoeffModulus::Create(N, {60, 40, 40, 60}), one special prime, scale 2^40.
//          One JSON line per check with the device path's error and the host path's error on the
//          same data; a check passes when the device error is within 4 x the host error (the
//          bound of tests/test_gpu_encode.py).  Exit status 0 iff all pass.
//        encoder_example time <log_n> <count>
//          the bootstrap chain (Q = {60, 29 x 59}, P = 10 x 60): per-plaintext time of the batched
//          encode_ext_device at chain 1 (30 + 10 limbs) and of decode_device, the host members
//          beside them, and the device stages one by one.  Warm medians; HIP events for device
//          time, a wall clock around the host members.  Nothing is asserted.
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

#include "../csrc/ntt.h"
#include "../host/encoder.h"
#include "../host/modulus.h"
#include "../host/numth.h"

using namespace phantom;
using namespace phantom::arith;
using cplx = std::complex<double>;
using lcplx = std::complex<long double>;

static std::mt19937_64 g_rng(0x5EED);

static std::vector<cplx> unit_square(size_t count) {
  std::uniform_real_distribution<double> d(-1.0, 1.0);
  std::vector<cplx> v(count);
  for (auto& x : v) {
    const double re = d(g_rng);
    x = cplx(re, d(g_rng));
  }
  return v;
}

static double max_err(const std::vector<cplx>& a, const std::vector<cplx>& b) {
  double e = 0;
  for (size_t i = 0; i < a.size(); ++i) e = std::max(e, std::abs(a[i] - b[i]));
  return e;
}

// inverse canonical embedding in long double (radix 2, slot j at zeta^(5^j)): the FP yardstick
static std::vector<long double> slots_to_coeffs_ld(const std::vector<cplx>& values, size_t n) {
  const long double pi = std::acos(-1.0L);
  const size_t m = 2 * n;
  std::vector<lcplx> zeta(m), a(n, lcplx(0, 0));
  for (size_t j = 0; j < m; ++j) zeta[j] = lcplx(std::cos(2 * pi * j / m), std::sin(2 * pi * j / m));
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

static bool g_all = true;
static void report(const char* name, int log_n, double e_dev, double e_host, double bound, const char* note = "") {
  const bool ok = e_dev <= bound;
  g_all = g_all && ok;
  std::printf("{\"check\": \"%s\", \"log_n\": %d, \"ok\": %s, \"e_dev\": %.6e, \"e_host\": %.6e, \"bound\": %.6e, "
              "\"note\": \"%s\"}\n",
              name, log_n, ok ? "true" : "false", e_dev, e_host, bound, note);
}

// coefficient form of an extended plaintext on the host ([limbs][n])
static std::vector<uint64_t> ext_coefficients(const PhantomContext& ctx, const PhantomPlaintext& pt, size_t chain) {
  hipStream_t s = ctx.stream();
  const phx::LimbMap map = encode_limb_map(ctx, chain, true);
  DeviceBuffer<uint64_t> tmp(static_cast<size_t>(map.num_limbs) * ctx.poly_degree(), s);
  PHX_CHECK(phx::ntt_inverse(ctx.gpu_rns_tables(), pt.data(), tmp.get(), map, nullptr, nullptr, s));
  return tmp.download(s);
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
  const std::vector<cplx> v = unit_square(slots);
  std::vector<cplx> back;
  PhantomPlaintext pt_host, pt_dev;

  enc.encode(ctx, v, scale, pt_host, 1);
  enc.decode(ctx, pt_host, back);
  const double e_host = max_err(back, v);
  enc.encode_on_device(ctx, v, scale, pt_dev, 1);
  enc.decode_on_device(ctx, pt_dev, back);
  report("device_encode_device_decode", log_n, max_err(back, v), e_host, 4 * e_host);
  enc.decode_on_device(ctx, pt_host, back);
  report("host_encode_device_decode", log_n, max_err(back, v), e_host, 4 * e_host);
  enc.decode(ctx, pt_dev, back);
  report("device_encode_host_decode", log_n, max_err(back, v), e_host, 4 * e_host);

  {  // encode_ext_device (two plaintexts in one call) against encode_ext, coefficient by coefficient
    const size_t chain = 2;
    std::vector<cplx> two = v;
    const std::vector<cplx> w = unit_square(slots);
    two.insert(two.end(), w.begin(), w.end());
    DeviceBuffer<cplx> dv;
    dv.upload(two, s);
    std::vector<PhantomPlaintext> outs(2);
    enc.encode_ext_device(ctx, dv.get(), scale, outs, chain);
    // the embedding errors: device and host coefficients against long double
    DeviceBuffer<double> dc(2 * n, s);
    embed_raw(ctx, false, dv.get(), dc.get(), 0, 2, s);
    const std::vector<double> c_dev = dc.download(s);
    double e_emb_dev = 0, e_emb_host = 0, diff = 0;
    std::vector<uint64_t> mods = ctx.get_context_data(chain).moduli();
    mods.insert(mods.end(), ctx.key_moduli().begin() + ctx.size_Q(), ctx.key_moduli().end());
    for (int i = 0; i < 2; ++i) {
      const std::vector<cplx>& vi = i ? w : v;
      const std::vector<long double> want = slots_to_coeffs_ld(vi, n);
      const std::vector<double> c_host = enc.slots_to_coeffs(vi);
      for (size_t k = 0; k < n; ++k) {
        e_emb_dev = std::max(e_emb_dev, static_cast<double>(std::fabs(c_dev[i * n + k] - want[k])));
        e_emb_host = std::max(e_emb_host, static_cast<double>(std::fabs(c_host[k] - want[k])));
      }
      PhantomPlaintext ref;
      enc.encode_ext(ctx, vi, scale, ref, chain);
      const std::vector<uint64_t> a = ext_coefficients(ctx, outs[i], chain), b = ext_coefficients(ctx, ref, chain);
      for (size_t l = 0; l < mods.size(); ++l)
        for (size_t k = 0; k < n; ++k) {
          const uint64_t q = mods[l], d = (a[l * n + k] + q - b[l * n + k]) % q;
          diff = std::max(diff, static_cast<double>(std::min(d, q - d)));
        }
    }
    report("embedding_coefficients", log_n, e_emb_dev, e_emb_host, 4 * e_emb_host);
    report("encode_ext_device_vs_encode_ext", log_n, diff, 0.0, 1 + 4 * e_emb_host * scale,
           "centred coefficient difference");
  }

  {  // sparse packing: both paths against the tiled message, through the host decoder
    const size_t ns = slots / 8;
    enc.set_sparse_encode(2 * ns);
    const std::vector<cplx> sv = unit_square(ns);
    std::vector<cplx> tiled(slots);
    for (size_t j = 0; j < slots; ++j) tiled[j] = sv[j % ns];
    PhantomPlaintext ps_host, ps_dev;
    enc.encode_sparse(ctx, sv, scale, ps_host, 1);
    DeviceBuffer<cplx> dv;
    dv.upload(sv, s);
    enc.encode_sparse_device(ctx, dv.get(), ns, scale, ps_dev, 1);
    enc.decode(ctx, ps_host, back);
    const double es_host = max_err(back, tiled);
    enc.decode(ctx, ps_dev, back);
    report("sparse_device_vs_dense_tiling", log_n, max_err(back, tiled), es_host, 4 * es_host);
  }

  {  // values too large: both paths throw the same std::invalid_argument
    const std::vector<cplx> big(slots, cplx(1e290, 0.0));
    std::string dev_msg, host_msg;
    PhantomPlaintext p;
    try {
      enc.encode_on_device(ctx, big, scale, p, 1);
    } catch (const std::invalid_argument& e) {
      dev_msg = e.what();
    }
    try {
      enc.encode(ctx, big, scale, p, 1);
    } catch (const std::invalid_argument& e) {
      host_msg = e.what();
    }
    const bool ok = dev_msg == "encoded values are too large" && host_msg == dev_msg;
    report("overflow_throws", log_n, ok ? 0.0 : 1.0, 0.0, 0.5, dev_msg.c_str());
  }
  std::printf("{\"done\": \"encoder_example check\", \"ok\": %s}\n", g_all ? "true" : "false");
  return g_all ? 0 : 1;
}

// ---- timing ------------------------------------------------------------------------------------

static double median(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}

template <class F>
static double device_ms(hipStream_t s, F&& f, int reps = 7) {
  hipEvent_t a, b;
  PHX_CHECK(hipEventCreate(&a));
  PHX_CHECK(hipEventCreate(&b));
  f();  // warm: allocations, tables, code objects
  PHX_CHECK(hipStreamSynchronize(s));
  std::vector<double> t;
  for (int r = 0; r < reps; ++r) {
    PHX_CHECK(hipEventRecord(a, s));
    f();
    PHX_CHECK(hipEventRecord(b, s));
    PHX_CHECK(hipEventSynchronize(b));
    float ms = 0;
    PHX_CHECK(hipEventElapsedTime(&ms, a, b));
    t.push_back(ms);
  }
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  return median(t);
}

template <class F>
static double host_ms(F&& f, int reps = 3) {
  f();
  std::vector<double> t;
  for (int r = 0; r < reps; ++r) {
    const auto t0 = std::chrono::steady_clock::now();
    f();
    t.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }
  return median(t);
}

static void line(const char* what, const char* path, size_t count, double ms_total) {
  std::printf("{\"time\": \"%s\", \"path\": \"%s\", \"plaintexts\": %zu, \"ms_total\": %.4f, \"ms_per_plaintext\": %.5f}\n",
              what, path, count, ms_total, ms_total / static_cast<double>(count));
  std::fflush(stdout);
}

static int run_time(int log_n, size_t count) {
  const size_t n = size_t(1) << log_n, slots = n / 2, chain = 1;
  std::vector<int> bits{60};
  bits.insert(bits.end(), 29, 59);
  bits.insert(bits.end(), 10, 60);
  EncryptionParameters parms(scheme_type::ckks);
  parms.set_poly_modulus_degree(n);
  parms.set_special_modulus_size(10);
  parms.set_coeff_modulus(CoeffModulus::Create(n, bits));
  PhantomContext ctx(parms);
  PhantomCKKSEncoder enc(ctx);
  hipStream_t s = ctx.stream();
  const double scale = std::ldexp(1.0, 59);
  const size_t Ql = ctx.get_context_data(chain).coeff_modulus_size(), ext = Ql + ctx.size_P();
  std::printf("{\"config\": \"encoder_example time\", \"log_n\": %d, \"count\": %zu, \"limbs_Ql\": %zu, \"limbs_ext\": %zu, "
              "\"write_floor_bytes_per_plaintext\": %zu}\n",
              log_n, count, Ql, ext, ext * n * sizeof(uint64_t));

  const std::vector<cplx> host_values = unit_square(count * slots);
  DeviceBuffer<cplx> dv;
  dv.upload(host_values, s);
  std::vector<PhantomPlaintext> outs(count);

  // encode_ext: the batched device member, and the host member in a loop over a few plaintexts
  line("encode_ext", "device_batched", count,
       device_ms(s, [&] { enc.encode_ext_device(ctx, dv.get(), scale, outs, chain); }));
  const size_t host_count = std::min<size_t>(count, 8);
  {
    PhantomPlaintext p;
    std::vector<std::vector<cplx>> hv(host_count);
    for (size_t i = 0; i < host_count; ++i) hv[i].assign(host_values.begin() + i * slots, host_values.begin() + (i + 1) * slots);
    line("encode_ext", "host_loop", host_count, host_ms([&] {
           for (size_t i = 0; i < host_count; ++i) enc.encode_ext(ctx, hv[i], scale, p, chain);
         }));
  }
  // the device stages of that encode, each over the whole batch in slices of 32 plaintexts
  {
    const size_t c = std::min<size_t>(count, 32);
    DeviceBuffer<double> coeffs(c * n, s);
    DeviceBuffer<uint64_t> res(c * ext * n, s);
    line("stage_embed_inverse", "device", c, device_ms(s, [&] { embed_raw(ctx, false, dv.get(), coeffs.get(), 0, c, s); }));
    line("stage_round_split", "device", c, device_ms(s, [&] {
           round_rns_raw(ctx, chain, true, coeffs.get(), scale, c, false, res.get(), nullptr, s);
         }));
    line("stage_round_split_ntt", "device", c, device_ms(s, [&] {
           round_rns_raw(ctx, chain, true, coeffs.get(), scale, c, true, res.get(), nullptr, s);
         }));
  }

  // decode at chain 1 (Ql limbs): plaintexts from the device encoder
  std::vector<PhantomPlaintext> pts(count);
  for (size_t i = 0; i < count; ++i) enc.encode_device(ctx, dv.get() + i * slots, slots, scale, pts[i], chain);
  DeviceBuffer<cplx> dout(count * slots, s);
  line("decode", "device_loop", count, device_ms(s, [&] {
         for (size_t i = 0; i < count; ++i) enc.decode_device(ctx, pts[i], dout.get() + i * slots);
       }));
  {
    std::vector<const uint64_t*> ptrs(count);
    for (size_t i = 0; i < count; ++i) ptrs[i] = pts[i].data();
    line("decode", "device_batched", count, device_ms(s, [&] {
           decode_raw(ctx, chain, nullptr, ptrs.data(), scale, count, dout.get(), s);
         }));
    const size_t c = std::min<size_t>(count, 32);
    DeviceBuffer<double> coeffs(c * n, s);
    line("stage_intt_compose", "device", c, device_ms(s, [&] {
           compose_raw(ctx, chain, nullptr, ptrs.data(), c, 1.0 / scale, coeffs.get(), s);
         }));
    line("stage_embed_forward", "device", c, device_ms(s, [&] { embed_raw(ctx, true, coeffs.get(), dout.get(), 0, c, s); }));
  }
  {
    std::vector<cplx> back;
    line("decode", "host_loop", host_count, host_ms([&] {
           for (size_t i = 0; i < host_count; ++i) enc.decode(ctx, pts[i], back);
         }));
    // and the two decoders agree on the last one
    std::vector<cplx> dev_back;
    enc.decode_on_device(ctx, pts[host_count - 1], dev_back);
    std::printf("{\"time\": \"decode_agreement\", \"max_abs_difference\": %.6e}\n", max_err(back, dev_back));
  }
  return 0;
}

int main(int argc, char** argv) {
  try {
    if (argc >= 3 && !std::strcmp(argv[1], "check")) return run_check(std::atoi(argv[2]));
    if (argc >= 4 && !std::strcmp(argv[1], "time")) return run_time(std::atoi(argv[2]), std::strtoull(argv[3], nullptr, 0));
    std::fprintf(stderr, "usage: encoder_example check <log_n> | time <log_n> <count>\n");
    return 2;
  } catch (const std::exception& e) {
    std::printf("{\"error\": \"%s\", \"ok\": false}\n", e.what());
    return 1;
  }
}
