// capi_pack.cpp — C-ABI of the channel packing for the tensor bootstrap (declared in
// include/phantom_amd.h): the tree's rotations, the monomial interleave and one tree level on raw
// ciphertexts (host/pack.h), and the batched same-key rotations the tree's levels run on
// (host/ckks_eval.h).
#include <vector>

#include "../host/capi_internal.h"
#include "../host/ckks_eval.h"
#include "../host/context.h"
#include "../host/pack.h"
#include "phantom_amd.h"

using phantom::capi::fail;

const phantom::PhantomContext& phantom_capi_context(const phantom_context* c);  // capi_ckks.cpp
const uint64_t* const* phantom_capi_key_array(const phantom_context* c, const uint64_t* const* host, size_t dnum,
                                              size_t need);

namespace {
// the key's digit pointers on the device, after the checks that must come before them
const uint64_t* const* batch_keys(const phantom_context* ctx, size_t chain_index, const uint64_t* const* key_digits,
                                  size_t dnum) {
  const auto& pc = phantom_capi_context(ctx);
  if (chain_index < 1 || chain_index >= pc.total_parm_size()) throw std::invalid_argument("invalid chain index");
  if (!key_digits) throw std::invalid_argument("null pointer");
  return phantom_capi_key_array(ctx, key_digits, dnum, pc.get_context_data(chain_index).gpu_rns_tool().beta());
}
}  // namespace

extern "C" {

int phantom_pack_rotations(size_t width, size_t slotstr, size_t pack, size_t log_n, int* rotations,
                           uint32_t* galois_elts, uint32_t* powers, size_t capacity, size_t* count) {
  PHX_CAPI_GUARD({
    if (!count) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null pointer");
    if (log_n < 1 || log_n > 20) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "log_n must be 1..20");
    const phantom::PackPlan plan = phantom::pack_plan(size_t(1) << log_n, width, slotstr, pack);
    *count = plan.log_pack;
    if (capacity < plan.log_pack) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "capacity below log2(pack) levels");
    for (size_t t = 0; t < plan.log_pack; ++t) {
      if (rotations) rotations[t] = plan.rotations[t];
      if (galois_elts) galois_elts[t] = plan.galois[t];
      if (powers) powers[t] = plan.powers[t];
    }
    return PHANTOM_OK;
  });
}

int phantom_ct_pack(const phantom_context* ctx, size_t chain_index, const uint64_t* const* ins, size_t C,
                    uint32_t stride_power, uint64_t* out, hipStream_t stream) {
  PHX_CAPI_GUARD({
    phantom::ct_pack_raw(phantom_capi_context(ctx), chain_index, ins, C, stride_power, out, stream);
    return PHANTOM_OK;
  });
}

int phantom_ct_split(const phantom_context* ctx, size_t chain_index, const uint64_t* const* a, const uint64_t* const* r,
                     size_t count, uint32_t power, uint64_t* const* even, uint64_t* const* odd, hipStream_t stream) {
  PHX_CAPI_GUARD({
    phantom::ct_split_raw(phantom_capi_context(ctx), chain_index, a, r, count, power, even, odd, stream);
    return PHANTOM_OK;
  });
}

int phantom_keyswitch_rotate_many(const phantom_context* ctx, size_t chain_index, size_t count,
                                  const uint64_t* const* cts, const uint64_t* const* digits,
                                  const uint64_t* const* key_digits, size_t dnum, uint32_t galois_elt,
                                  uint64_t* const* outs, hipStream_t stream) {
  PHX_CAPI_GUARD({
    const uint64_t* const* evk = batch_keys(ctx, chain_index, key_digits, dnum);
    phantom::keyswitch_rotate_many_raw(phantom_capi_context(ctx), chain_index, count, cts, digits, evk, galois_elt, outs,
                                       stream);
    return PHANTOM_OK;
  });
}

int phantom_rotate_fused_batch(const phantom_context* ctx, size_t chain_index, size_t count, const uint64_t* const* cts,
                               const uint64_t* const* key_digits, size_t dnum, uint32_t galois_elt,
                               uint64_t* const* outs, hipStream_t stream) {
  PHX_CAPI_GUARD({
    const uint64_t* const* evk = batch_keys(ctx, chain_index, key_digits, dnum);
    if (!cts || !outs) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null pointer");
    phantom::rotate_fused_batch_raw(phantom_capi_context(ctx), chain_index, cts, count, evk, galois_elt, outs, stream);
    return PHANTOM_OK;
  });
}

int phantom_rotate_fused_batch_chunk(const phantom_context* ctx, size_t chain_index, size_t* out) {
  PHX_CAPI_GUARD({
    if (!out) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null pointer");
    *out = phantom::rotate_fused_batch_chunk(phantom_capi_context(ctx), chain_index);
    return PHANTOM_OK;
  });
}

}  // extern "C"
