// capi_conv.cpp — C-ABI of the hoisted encrypted convolution (declared in include/phantom_amd.h):
// the tap rotations, the weight slot vectors and their host twin, the general inner sums over the
// extended basis, and the whole layer on raw ciphertexts (host/conv2d.h).
#include <memory>
#include <vector>

#include "../host/buffer.h"
#include "../host/capi_internal.h"
#include "../host/context.h"
#include "../host/conv2d.h"
#include "../host/rns_tool.h"
#include "conv.h"
#include "phantom_amd.h"

using phantom::capi::fail;
using phantom::capi::from_hip;

const phantom::PhantomContext& phantom_capi_context(const phantom_context* c);  // capi_ckks.cpp
const uint64_t* const* phantom_capi_key_array(const phantom_context* c, const uint64_t* const* host, size_t dnum,
                                              size_t need);

struct phantom_conv_plan {
  std::unique_ptr<phantom::ConvPlanData> data;
  const phantom_context* owner = nullptr;
};

namespace {

// the shape alone (no ring degree at hand): ns is checked against n = 2 ns, i.e. not at all
phx::ConvShape shape_of(size_t width, size_t slotstr, size_t kernel, size_t in_ch, size_t out_ch) {
  const phx::ConvShape c = phantom::conv_shape(size_t(1) << 63, width, slotstr, kernel, in_ch, out_ch);
  return c;
}

}  // namespace

extern "C" {

int phantom_conv_rotations(size_t width, size_t slotstr, size_t kernel, int* out, size_t capacity, size_t* count) {
  PHX_CAPI_GUARD({
    if (!out || !count) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null pointer");
    (void)shape_of(width, slotstr, kernel, 1, 1);
    const std::vector<int> r = phantom::conv_rotations(width, slotstr, kernel);
    *count = r.size();
    if (capacity < r.size()) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "capacity below kernel^2 rotations");
    for (size_t i = 0; i < r.size(); ++i) out[i] = r[i];
    return PHANTOM_OK;
  });
}

int phantom_conv_weight_slots(size_t width, size_t slotstr, size_t kernel, size_t in_ch, size_t out_ch,
                              const double* dev_W, size_t first_term, size_t count, double* dev_out,
                              hipStream_t stream) {
  PHX_CAPI_GUARD({
    if (!dev_W || !dev_out) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null pointer");
    const phx::ConvShape c = shape_of(width, slotstr, kernel, in_ch, out_ch);
    if (first_term > c.terms() || count > c.terms() - first_term)
      return fail(PHANTOM_ERR_INVALID_ARGUMENT, "terms past out_ch in_ch kernel^2");
    return from_hip(phx::conv_weight_slots(c, dev_W, first_term, count, dev_out, stream));
  });
}

int phantom_conv_weight_slots_host(size_t width, size_t slotstr, size_t kernel, size_t in_ch, size_t out_ch,
                                   const double* W, size_t first_term, size_t count, double* out) {
  PHX_CAPI_GUARD({
    if (!W || !out) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null pointer");
    const phx::ConvShape c = shape_of(width, slotstr, kernel, in_ch, out_ch);
    if (first_term > c.terms() || count > c.terms() - first_term)
      return fail(PHANTOM_ERR_INVALID_ARGUMENT, "terms past out_ch in_ch kernel^2");
    phx::conv_weight_slots_host(c, W, first_term, count, out);
    return PHANTOM_OK;
  });
}

int phantom_ext_mac(const phantom_context* ctx, size_t chain_index, const uint64_t* const* ins, size_t T,
                    const uint64_t* const* dev_pts, size_t O, uint64_t* const* outs, int accumulate,
                    hipStream_t stream) {
  PHX_CAPI_GUARD({
    const auto& pc = phantom_capi_context(ctx);
    if (!ins || !dev_pts || !outs) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null pointer");
    if (T == 0 || O == 0 || T > (size_t(1) << 24) || O > (size_t(1) << 16))
      return fail(PHANTOM_ERR_INVALID_ARGUMENT, "term and output counts must be at least 1");
    phx::MacArgs a = phantom::mac_args(pc, chain_index);
    // one device table: the T input pointers, then the O output pointers
    std::vector<uint64_t*> tab(T + O);
    for (size_t t = 0; t < T; ++t) {
      if (!ins[t]) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null input");
      tab[t] = const_cast<uint64_t*>(ins[t]);  // read only: the kernel takes this half as const
    }
    for (size_t o = 0; o < O; ++o) {
      if (!outs[o]) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null output");
      tab[T + o] = outs[o];
    }
    phantom::DeviceBuffer<uint64_t*> table;
    table.upload(tab, stream);
    a.ins = table.get();
    a.outs = table.get() + T;
    a.pts = dev_pts;
    a.T = static_cast<uint32_t>(T);
    a.O = static_cast<uint32_t>(O);
    a.accumulate = accumulate != 0;
    const hipError_t e = phx::ext_mac(a, pc.poly_degree(), stream);
    PHX_CHECK(hipStreamSynchronize(stream));  // the pointer table is freed on return
    return from_hip(e);
  });
}

int phantom_conv2d(const phantom_context* ctx, size_t chain_index, const uint64_t* const* cts, size_t in_ch,
                   size_t out_ch, size_t width, size_t slotstr, size_t kernel, const double* dev_W, double pt_scale,
                   const uint64_t* const* const* key_digits, size_t dnum, const uint32_t* galois_elts, size_t group,
                   uint64_t* const* outs, int* dev_overflow, hipStream_t stream) {
  PHX_CAPI_GUARD({
    const auto& pc = phantom_capi_context(ctx);
    if (!cts || !dev_W || !key_digits || !galois_elts || !outs) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null pointer");
    if (!(pt_scale > 0)) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "scale must be positive");
    (void)phantom::mac_args(pc, chain_index);  // the chain index and the special primes
    const phx::ConvShape c = phantom::conv_shape(pc.poly_degree(), width, slotstr, kernel, in_ch, out_ch);
    const size_t beta = pc.get_context_data(chain_index).gpu_rns_tool().beta();
    const size_t K2 = kernel * kernel;
    // every check before the first key array is uploaded (conv2d_raw repeats the rest before it enqueues)
    for (size_t k = 0; k < in_ch; ++k)
      if (!cts[k]) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null input channel");
    for (size_t h = 0; h < out_ch; ++h)
      if (!outs[h]) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null output channel");
    for (size_t t = 0; t < K2; ++t)
      if (!key_digits[t] && t != K2 / 2)
        return fail(PHANTOM_ERR_INVALID_ARGUMENT, "only the centre tap goes without a rotation key");
    std::vector<const uint64_t* const*> evk(K2, nullptr);
    for (size_t t = 0; t < K2; ++t)
      if (key_digits[t]) evk[t] = phantom_capi_key_array(ctx, key_digits[t], dnum, beta);
    phantom::conv2d_raw(pc, chain_index, cts, c, dev_W, pt_scale, evk.data(), galois_elts, group, outs, dev_overflow,
                        stream);
    return PHANTOM_OK;
  });
}

static int ext_mac_sub_run(const phantom_context* ctx, size_t chain_index, const uint64_t* const* ins, size_t T,
                           const uint64_t* const* dev_pts, size_t sub_degree, size_t O, uint64_t* const* outs,
                           int accumulate, const uint64_t* const* res, const uint64_t* res_mult, const uint64_t* bias,
                           hipStream_t stream) {
  PHX_CAPI_GUARD({
    const auto& pc = phantom_capi_context(ctx);
    if (!ins || !dev_pts || !outs) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null pointer");
    if (T == 0 || O == 0 || T > (size_t(1) << 24) || O > (size_t(1) << 16))
      return fail(PHANTOM_ERR_INVALID_ARGUMENT, "term and output counts must be at least 1");
    if (sub_degree == 0 || sub_degree > pc.poly_degree() || (sub_degree & (sub_degree - 1)))
      return fail(PHANTOM_ERR_INVALID_ARGUMENT, "the subring degree must be a power of two in [1, N]");
    if (res && !res_mult) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "a residual needs its multiplier");
    phx::MacArgs a = phantom::mac_args(pc, chain_index);
    // one device table: the T input pointers, then the O output pointers
    std::vector<uint64_t*> tab(T + O);
    for (size_t t = 0; t < T; ++t) {
      if (!ins[t]) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null input");
      tab[t] = const_cast<uint64_t*>(ins[t]);  // read only: the kernel takes this half as const
    }
    for (size_t o = 0; o < O; ++o) {
      if (!outs[o]) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null output");
      tab[T + o] = outs[o];
    }
    phantom::DeviceBuffer<uint64_t*> table;
    table.upload(tab, stream);
    a.ins = table.get();
    a.outs = table.get() + T;
    a.pts = dev_pts;
    a.T = static_cast<uint32_t>(T);
    a.O = static_cast<uint32_t>(O);
    a.accumulate = accumulate != 0;
    phantom::DeviceBuffer<uint64_t> seed;
    if (res || bias) {
      seed.allocate(phantom::mac_seed_words(O, a.Ql), stream);
      phantom::mac_seed(pc, chain_index, O, res, res_mult, bias, seed.get(), a, stream);
    }
    const hipError_t e = phx::ext_mac_sub(a, pc.poly_degree(), sub_degree, stream);
    PHX_CHECK(hipStreamSynchronize(stream));  // the tables are freed on return
    return from_hip(e);
  });
}

int phantom_ext_mac_sub(const phantom_context* ctx, size_t chain_index, const uint64_t* const* ins, size_t T,
                        const uint64_t* const* dev_pts, size_t sub_degree, size_t O, uint64_t* const* outs,
                        int accumulate, hipStream_t stream) {
  return ext_mac_sub_run(ctx, chain_index, ins, T, dev_pts, sub_degree, O, outs, accumulate, nullptr, nullptr, nullptr,
                         stream);
}

int phantom_ext_mac_sub_seeded(const phantom_context* ctx, size_t chain_index, const uint64_t* const* ins, size_t T,
                               const uint64_t* const* dev_pts, size_t sub_degree, size_t O, uint64_t* const* outs,
                               const uint64_t* const* res, const uint64_t* res_mult, const uint64_t* bias,
                               hipStream_t stream) {
  return ext_mac_sub_run(ctx, chain_index, ins, T, dev_pts, sub_degree, O, outs, 0, res, res_mult, bias, stream);
}

int phantom_scaled_constant_residues(double value, double scale, const uint64_t* moduli, size_t count, uint64_t* out) {
  PHX_CAPI_GUARD({
    if (!moduli || !out) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null pointer");
    const std::vector<uint64_t> r = phantom::scaled_constant_residues(value, scale, moduli, count);
    for (size_t i = 0; i < count; ++i) out[i] = r[i];
    return PHANTOM_OK;
  });
}

int phantom_conv2d_prepare(const phantom_context* ctx, size_t chain_index, size_t in_ch, size_t out_ch, size_t width,
                           size_t slotstr, size_t kernel, const double* dev_W, double pt_scale, int* dev_overflow,
                           hipStream_t stream, phantom_conv_plan** plan) {
  return phantom_conv2d_prepare_scaled(ctx, chain_index, in_ch, out_ch, width, slotstr, kernel, dev_W, nullptr, pt_scale,
                                       dev_overflow, stream, plan);
}

int phantom_conv2d_prepare_scaled(const phantom_context* ctx, size_t chain_index, size_t in_ch, size_t out_ch,
                                  size_t width, size_t slotstr, size_t kernel, const double* dev_W,
                                  const double* out_scale, double pt_scale, int* dev_overflow, hipStream_t stream,
                                  phantom_conv_plan** plan) {
  PHX_CAPI_GUARD({
    const auto& pc = phantom_capi_context(ctx);
    if (!dev_W || !plan) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null pointer");
    if (!(pt_scale > 0)) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "scale must be positive");
    (void)phantom::mac_args(pc, chain_index);
    const phx::ConvShape c = phantom::conv_shape(pc.poly_degree(), width, slotstr, kernel, in_ch, out_ch);
    auto p = std::make_unique<phantom_conv_plan>();
    p->data = phantom::conv2d_prepare(pc, chain_index, c, dev_W, pt_scale, dev_overflow, stream, out_scale);
    p->owner = ctx;
    *plan = p.release();
    return PHANTOM_OK;
  });
}

int phantom_conv_plan_bytes(const phantom_conv_plan* plan, size_t* bytes) {
  PHX_CAPI_GUARD({
    if (!plan || !bytes) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null pointer");
    *bytes = plan->data->bytes();
    return PHANTOM_OK;
  });
}

int phantom_conv_plan_read(const phantom_conv_plan* plan, uint64_t* host_out, size_t capacity) {
  PHX_CAPI_GUARD({
    if (!plan || !host_out) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null pointer");
    if (capacity < plan->data->words) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "capacity below the plan's words");
    PHX_CHECK(hipDeviceSynchronize());
    PHX_CHECK(hipMemcpy(host_out, plan->data->pts, plan->data->bytes(), hipMemcpyDeviceToHost));
    return PHANTOM_OK;
  });
}

int phantom_conv_plan_destroy(phantom_conv_plan* plan) {
  PHX_CAPI_GUARD({
    delete plan;
    return PHANTOM_OK;
  });
}

int phantom_conv2d_apply(const phantom_context* ctx, const phantom_conv_plan* plan, const uint64_t* const* cts,
                         const uint64_t* const* const* key_digits, size_t dnum, const uint32_t* galois_elts,
                         uint64_t* const* outs, hipStream_t stream) {
  return phantom_conv2d_apply_seeded(ctx, plan, cts, key_digits, dnum, galois_elts, outs, nullptr, nullptr, nullptr,
                                     stream);
}

int phantom_conv2d_apply_seeded(const phantom_context* ctx, const phantom_conv_plan* plan, const uint64_t* const* cts,
                                const uint64_t* const* const* key_digits, size_t dnum, const uint32_t* galois_elts,
                                uint64_t* const* outs, const uint64_t* const* res, const uint64_t* res_mult,
                                const uint64_t* bias, hipStream_t stream) {
  PHX_CAPI_GUARD({
    const auto& pc = phantom_capi_context(ctx);
    if (!plan || !cts || !key_digits || !galois_elts || !outs)
      return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null pointer");
    if (res && !res_mult) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "a residual needs its multiplier");
    if (plan->owner != ctx || plan->data->ctx != &pc)
      return fail(PHANTOM_ERR_INVALID_ARGUMENT, "the plan was prepared for another context");
    const phx::ConvShape& c = plan->data->shape;
    const size_t beta = pc.get_context_data(plan->data->chain_index).gpu_rns_tool().beta();
    const size_t K2 = static_cast<size_t>(c.kernel) * c.kernel;
    // every check before the first key array is uploaded (conv2d_apply repeats them before it enqueues)
    for (size_t k = 0; k < c.in_ch; ++k)
      if (!cts[k]) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null input channel");
    for (size_t h = 0; h < c.out_ch; ++h)
      if (!outs[h]) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null output channel");
    for (size_t t = 0; t < K2; ++t)
      if (!key_digits[t] && t != K2 / 2)
        return fail(PHANTOM_ERR_INVALID_ARGUMENT, "only the centre tap goes without a rotation key");
    std::vector<const uint64_t* const*> evk(K2, nullptr);
    for (size_t t = 0; t < K2; ++t)
      if (key_digits[t]) evk[t] = phantom_capi_key_array(ctx, key_digits[t], dnum, beta);
    phantom::conv2d_apply(pc, *plan->data, cts, evk.data(), galois_elts, outs, stream, res, res_mult, bias);
    return PHANTOM_OK;
  });
}

}  // extern "C"
