// capi_ltprep.cpp — C-ABI entry points of the device build of the bootstrap's linear-transform
// diagonals (csrc/ltprep.h) and of their host twins (declared in include/phantom_amd.h).  Every
// argument is checked, and every table computed, before the first upload or launch.
#include <algorithm>
#include <complex>
#include <cstring>
#include <vector>

#include "../host/bootstrap.h"
#include "../host/buffer.h"
#include "../host/capi_internal.h"
#include "../host/context.h"
#include "ltprep.h"
#include "phantom_amd.h"

const phantom::PhantomContext& phantom_capi_context(const phantom_context* c);  // capi_ckks.cpp

using phantom::capi::fail;
namespace boot = phantom::boot;

namespace {

std::vector<int> ints(const int* p, size_t count) {
  if (count && !p) throw std::invalid_argument("null pointer");
  return std::vector<int>(p, p + count);
}

void pow2_slots(size_t ns, size_t n) {
  if (ns < 2 || (ns & (ns - 1)) || !n || (n & (n - 1)) || ns > n || n > (size_t(1) << 24))
    throw std::invalid_argument("slot counts must be powers of two, 2 <= ns <= n");
}

void launched(hipError_t e, const char* what) {
  if (e == hipErrorInvalidValue) throw std::invalid_argument(std::string(what) + ": unsupported shape");
  if (e != hipSuccess) throw phantom::hip_error(e, what);
}

boot::LtShape shape_of(const int* shape) {
  if (!shape) throw std::invalid_argument("null pointer");
  boot::LtShape s;
  s.stride = shape[0];
  s.center = shape[1];
  s.D = shape[2];
  s.g = shape[3];
  s.b = shape[4];
  return s;
}

void shape_to(const boot::LtShape& s, int* shape) {
  const int v[5] = {s.stride, s.center, s.D, s.g, s.b};
  std::memcpy(shape, v, sizeof(v));
}

}  // namespace

extern "C" {

int phantom_ltprep_stage_offsets(size_t ns, const int* stages, size_t num_stages, int* offsets, size_t capacity,
                                 size_t* count) {
  PHX_CAPI_GUARD({
    if (!offsets || !count) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null pointer");
    const boot::StagePlan plan = boot::plan_stages(ns, ints(stages, num_stages));
    *count = plan.offsets().size();
    if (*count > capacity) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "offset capacity too small");
    std::copy(plan.offsets().begin(), plan.offsets().end(), offsets);
    return PHANTOM_OK;
  });
}

int phantom_ltprep_stage_products(const phantom_context* ctx, size_t ns, int inverse, const int* stages,
                                  size_t num_stages, double* dev_out, double* dev_scratch, size_t capacity_diagonals,
                                  hipStream_t stream) {
  PHX_CAPI_GUARD({
    const phantom::PhantomContext& cc = phantom_capi_context(ctx);
    if (!dev_out || !dev_scratch || dev_out == dev_scratch) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null pointer");
    const boot::StagePlan plan = boot::plan_stages(ns, ints(stages, num_stages));
    if (ns > cc.poly_degree() / 2) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "more slots than the ring has");
    if (plan.max_diagonals() > capacity_diagonals) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "diagonal capacity too small");
    phantom::DeviceBuffer<int32_t> tab;
    tab.upload(plan.src, stream);
    // the last stage lands in dev_out
    const bool odd = plan.stages.size() % 2 == 1;
    void* res = boot::stage_products_device(cc, plan, inverse != 0, tab.get(), odd ? dev_out : dev_scratch,
                                            odd ? dev_scratch : dev_out, stream);
    if (res != dev_out) return fail(PHANTOM_ERR_INTERNAL, "stage products ended in the scratch buffer");
    return PHANTOM_OK;
  });
}

int phantom_ltprep_stage_products_host(size_t ns, int inverse, const int* stages, size_t num_stages, double* out,
                                       size_t capacity_diagonals) {
  PHX_CAPI_GUARD({
    if (!out) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null pointer");
    const boot::StagePlan plan = boot::plan_stages(ns, ints(stages, num_stages));
    if (plan.offsets().size() > capacity_diagonals) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "diagonal capacity too small");
    const boot::DiagMap T = boot::stage_products_host(plan, inverse != 0);
    std::vector<int> keys;
    for (const auto& kv : T) keys.push_back(kv.first);
    if (keys != plan.offsets()) return fail(PHANTOM_ERR_INTERNAL, "the host product's offsets are not the structural ones");
    size_t i = 0;
    for (const auto& kv : T) std::memcpy(out + 2 * ns * i++, kv.second.data(), ns * sizeof(std::complex<double>));
    return PHANTOM_OK;
  });
}

int phantom_ltprep_presence(const double* dev_band, size_t ns, const int* offsets, size_t num_diagonals, double c_re,
                            double c_im, int apply_const, int* dev_flags, hipStream_t stream) {
  PHX_CAPI_GUARD({
    if (!dev_band || !dev_flags) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null pointer");
    pow2_slots(ns, ns);
    const std::vector<int> off = ints(offsets, num_diagonals);
    if (off.empty() || off.size() > 65535) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "bad diagonal count");
    for (int a : off)
      if (a < 0 || static_cast<size_t>(a) >= ns) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "offset out of range");
    phantom::DeviceBuffer<int32_t> tab;
    tab.upload(off, stream);
    PHX_CHECK(hipMemsetAsync(dev_flags, 0, 2 * off.size() * sizeof(int), stream));
    launched(phx::ltprep_presence(reinterpret_cast<const double2*>(dev_band), ns, tab.get(), static_cast<int>(off.size()),
                                  make_double2(c_re, c_im), apply_const != 0, dev_flags, stream),
             "presence");
    return PHANTOM_OK;
  });
}

int phantom_ltprep_lifted_offsets(const int* offsets, const int* flags, size_t num_diagonals, size_t ns, size_t n,
                                  int* keys, size_t capacity, size_t* count) {
  PHX_CAPI_GUARD({
    if (!keys || !count) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null pointer");
    pow2_slots(ns, n);
    const std::vector<int> k = boot::lifted_keys(ints(offsets, num_diagonals), ints(flags, 2 * num_diagonals), ns, n);
    *count = k.size();
    if (k.size() > capacity) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "offset capacity too small");
    std::copy(k.begin(), k.end(), keys);
    return PHANTOM_OK;
  });
}

int phantom_ltprep_shape(size_t n, const int* keys, size_t num_keys, int stride, uint32_t dim1, int* shape) {
  PHX_CAPI_GUARD({
    if (!shape) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null pointer");
    pow2_slots(2, n);
    if (stride < 1) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "bad stride");
    shape_to(boot::lt_shape(ints(keys, num_keys), n, dim1, stride), shape);
    return PHANTOM_OK;
  });
}

int phantom_ltprep_finish(const double* dev_band, size_t ns, size_t n, const int* band_offsets, size_t num_band,
                          const int* keys, size_t num_keys, const int* shape, double c_re, double c_im,
                          int apply_const, int mask, double* dev_out, int* slots_out, hipStream_t stream) {
  PHX_CAPI_GUARD({
    if (!dev_band || !dev_out || !slots_out) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null pointer");
    pow2_slots(ns, n);
    if (mask < 0 || mask > 2) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "bad mask");
    const std::vector<int> off = ints(band_offsets, num_band), k = ints(keys, num_keys);
    for (int a : off)
      if (a < 0 || static_cast<size_t>(a) >= ns) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "offset out of range");
    std::vector<phx::LtFinishRow> rows;
    const std::vector<int> slots = boot::finish_rows(shape_of(shape), ns, n, off, k, rows);
    if (rows.size() != k.size() || rows.empty())
      return fail(PHANTOM_ERR_INVALID_ARGUMENT, "an offset lies outside the level's shape (or there is none)");
    phantom::DeviceBuffer<phx::LtFinishRow> tab;
    tab.upload(rows, stream);
    launched(phx::ltprep_finish(reinterpret_cast<const double2*>(dev_band), ns, n, tab.get(), static_cast<int>(rows.size()),
                                make_double2(c_re, c_im), apply_const != 0, mask, reinterpret_cast<double2*>(dev_out),
                                stream),
             "finish");
    std::copy(slots.begin(), slots.end(), slots_out);
    return PHANTOM_OK;
  });
}

int phantom_ltprep_finish_host(const double* band, size_t ns, size_t n, const int* band_offsets, size_t num_band,
                               double c_re, double c_im, int apply_const, int mask, int stride, uint32_t dim1,
                               int* shape, int* keys_out, int* slots_out, size_t capacity, size_t* count, double* out) {
  PHX_CAPI_GUARD({
    if (!band || !shape || !keys_out || !slots_out || !count) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null pointer");
    pow2_slots(ns, n);
    if (mask < 0 || mask > 2 || stride < 1) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "bad mask or stride");
    const std::vector<int> off = ints(band_offsets, num_band);
    boot::DiagMap T;
    for (size_t i = 0; i < off.size(); ++i) {
      if (off[i] < 0 || static_cast<size_t>(off[i]) >= ns) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "offset out of range");
      const auto* v = reinterpret_cast<const std::complex<double>*>(band) + i * ns;
      if (!T.emplace(off[i], boot::cvec(v, v + ns)).second) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "offset repeated");
    }
    boot::LtShape sh;
    const std::vector<boot::FinishedDiagonal> d =
        boot::finish_host(std::move(T), ns, n, {c_re, c_im}, apply_const != 0, mask, dim1, stride, sh);
    shape_to(sh, shape);
    *count = d.size();
    if (d.size() > capacity) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "diagonal capacity too small");
    for (size_t i = 0; i < d.size(); ++i) {
      keys_out[i] = d[i].key;
      slots_out[i] = d[i].slot;
      if (out) std::memcpy(out + 2 * n * i, d[i].values.data(), n * sizeof(std::complex<double>));
    }
    return PHANTOM_OK;
  });
}

int phantom_ltprep_dense_diagonals(const double* dev_A, size_t slots, double scale, double* dev_out, int* dev_flags,
                                   hipStream_t stream) {
  PHX_CAPI_GUARD({
    if (!dev_A || !dev_out || !dev_flags) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null pointer");
    if (slots < 2 || (slots & (slots - 1)) || slots > (size_t(1) << 15))
      return fail(PHANTOM_ERR_INVALID_ARGUMENT, "the slot count must be a power of two, 2 .. 2^15");
    PHX_CHECK(hipMemsetAsync(dev_flags, 0, slots * sizeof(int), stream));
    launched(phx::ltprep_dense(reinterpret_cast<const double2*>(dev_A), slots, scale,
                               reinterpret_cast<double2*>(dev_out), dev_flags, stream),
             "dense diagonals");
    return PHANTOM_OK;
  });
}

}  // extern "C"
