// capi_encrypt.cpp — C-ABI entry points of the batched symmetric and public-key encryption / decryption (declared
// in include/phantom_amd.h).  Thin wrappers over the raw drivers of host/keys.h with explicit key
// material; every argument is checked there before the first launch.
#include <complex>
#include <cstring>

#include "../host/capi_internal.h"
#include "../host/context.h"
#include "../host/keys.h"
#include "phantom_amd.h"

using phantom::capi::fail;

const phantom::PhantomContext& phantom_capi_context(const phantom_context* c);  // capi_ckks.cpp

namespace {
phx::ChaChaKey key_of(const uint32_t* k) {
  if (!k) throw std::invalid_argument("null pointer");
  phx::ChaChaKey key;
  std::memcpy(key.k, k, sizeof(key.k));
  return key;
}
}  // namespace

extern "C" {

int phantom_sample_cbd_small_batch(const phantom_context* ctx, const uint32_t* key, const uint64_t* nonces,
                                   size_t count, int32_t* dev_out, hipStream_t stream) {
  PHX_CAPI_GUARD({
    phantom::sample_cbd_small_raw(phantom_capi_context(ctx), key_of(key), nonces, count, dev_out, stream);
    return PHANTOM_OK;
  });
}

int phantom_encrypt_symmetric_batch(const phantom_context* ctx, size_t chain_index, const uint64_t* dev_sk,
                                    const double* dev_values, size_t num_values, size_t sparse_slots, double scale,
                                    size_t count, const uint32_t* key, const uint64_t* nonces, const uint8_t* seeds,
                                    uint64_t* dev_out, size_t out_stride, int* dev_overflow, hipStream_t stream) {
  PHX_CAPI_GUARD({
    if (!dev_out) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null pointer");
    phantom::encrypt_symmetric_raw(phantom_capi_context(ctx), chain_index, dev_sk,
                                   reinterpret_cast<const std::complex<double>*>(dev_values), num_values, sparse_slots,
                                   scale, count, key_of(key), nonces, seeds, dev_out, out_stride, nullptr,
                                   dev_overflow, stream);
    return PHANTOM_OK;
  });
}

int phantom_decrypt_batch(const phantom_context* ctx, const uint64_t* dev_sk, const uint64_t* dev_in, size_t in_stride,
                          size_t polys, size_t ct_limbs, size_t limbs, size_t count, uint64_t* dev_plain,
                          hipStream_t stream) {
  PHX_CAPI_GUARD({
    if (!dev_in) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null pointer");
    phantom::decrypt_raw(phantom_capi_context(ctx), dev_sk, dev_in, in_stride, nullptr, polys, ct_limbs, limbs, count,
                         dev_plain, stream);
    return PHANTOM_OK;
  });
}

int phantom_decrypt_decode_batch(const phantom_context* ctx, const uint64_t* dev_sk, const uint64_t* dev_in,
                                 size_t in_stride, size_t polys, size_t ct_limbs, size_t limbs, size_t count,
                                 double scale, double* dev_values, hipStream_t stream) {
  PHX_CAPI_GUARD({
    if (!dev_in) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null pointer");
    phantom::decrypt_decode_raw(phantom_capi_context(ctx), dev_sk, dev_in, in_stride, nullptr, polys, ct_limbs, limbs,
                                count, scale, reinterpret_cast<std::complex<double>*>(dev_values), stream);
    return PHANTOM_OK;
  });
}

int phantom_encrypt_batch_chunk(const phantom_context* ctx, size_t chain_index, size_t* chunk) {
  PHX_CAPI_GUARD({
    const phantom::PhantomContext& pc = phantom_capi_context(ctx);
    if (!chunk) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null pointer");
    if (chain_index < 1 || chain_index >= pc.total_parm_size())
      return fail(PHANTOM_ERR_INVALID_ARGUMENT, "invalid chain index");
    *chunk = phantom::encrypt_batch_chunk(pc);
    return PHANTOM_OK;
  });
}

int phantom_sample_small_batch(const phantom_context* ctx, int kind, const uint32_t* key, const uint64_t* nonces,
                               size_t count, int32_t* dev_out, hipStream_t stream) {
  PHX_CAPI_GUARD({
    const phantom::PhantomContext& pc = phantom_capi_context(ctx);
    if (kind != PHANTOM_SAMPLE_CBD && kind != PHANTOM_SAMPLE_TERNARY)
      return fail(PHANTOM_ERR_INVALID_ARGUMENT, "kind must be PHANTOM_SAMPLE_CBD or PHANTOM_SAMPLE_TERNARY");
    phantom::sample_small_raw(pc, kind == PHANTOM_SAMPLE_TERNARY, key_of(key), nonces, count, dev_out, stream);
    return PHANTOM_OK;
  });
}

int phantom_encrypt_asymmetric_batch(const phantom_context* ctx, size_t chain_index, const uint64_t* dev_pk,
                                     const double* dev_values, size_t num_values, size_t sparse_slots, double scale,
                                     size_t count, const uint32_t* key, const uint64_t* nonces, uint64_t* dev_out,
                                     size_t out_stride, int* dev_overflow, hipStream_t stream) {
  PHX_CAPI_GUARD({
    if (!dev_out) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null pointer");
    phantom::encrypt_asymmetric_raw(phantom_capi_context(ctx), chain_index, dev_pk,
                                    reinterpret_cast<const std::complex<double>*>(dev_values), num_values, sparse_slots,
                                    scale, count, key_of(key), nonces, dev_out, out_stride, nullptr, dev_overflow,
                                    stream);
    return PHANTOM_OK;
  });
}

int phantom_encrypt_asymmetric_batch_chunk(const phantom_context* ctx, size_t chain_index, size_t* chunk) {
  PHX_CAPI_GUARD({
    const phantom::PhantomContext& pc = phantom_capi_context(ctx);
    if (!chunk) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null pointer");
    *chunk = phantom::encrypt_asymmetric_batch_chunk(pc, chain_index);
    return PHANTOM_OK;
  });
}

}  // extern "C"
