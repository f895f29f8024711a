// capi_pack.cpp — C-ABI of the channel packing for the tensor bootstrap (declared in
// include/phantom_amd.h): the tree's rotations, the monomial interleave and one tree level on raw
// ciphertexts (host/pack.h).
#include <vector>

#include "../host/capi_internal.h"
#include "../host/context.h"
#include "../host/pack.h"
#include "phantom_amd.h"

using phantom::capi::fail;

const phantom::PhantomContext& phantom_capi_context(const phantom_context* c);  // capi_ckks.cpp

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

}  // extern "C"
