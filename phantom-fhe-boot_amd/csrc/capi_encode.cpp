// capi_encode.cpp — C-ABI entry points of the device CKKS encoder / decoder (declared in
// include/phantom_amd.h).  Thin wrappers over the raw drivers of host/encoder.h; every argument is
// checked there before the first launch.
#include <complex>

#include "../host/capi_internal.h"
#include "../host/context.h"
#include "../host/encoder.h"
#include "phantom_amd.h"

const phantom::PhantomContext& phantom_capi_context(const phantom_context* c);  // capi_ckks.cpp

extern "C" {

int phantom_ckks_embed(const phantom_context* ctx, int forward, const double* in, double* out, size_t sparse_slots,
                       size_t count, hipStream_t stream) {
  PHX_CAPI_GUARD({
    phantom::embed_raw(phantom_capi_context(ctx), forward != 0, in, out, sparse_slots, count, stream);
    return PHANTOM_OK;
  });
}

int phantom_ckks_round_rns(const phantom_context* ctx, size_t chain_index, int ext, const double* coeffs, double scale,
                           size_t count, int ntt_form, uint64_t* out, int* dev_overflow, hipStream_t stream) {
  PHX_CAPI_GUARD({
    phantom::round_rns_raw(phantom_capi_context(ctx), chain_index, ext != 0, coeffs, scale, count, ntt_form != 0, out,
                           dev_overflow, stream);
    return PHANTOM_OK;
  });
}

int phantom_ckks_compose(const phantom_context* ctx, size_t chain_index, const uint64_t* plain_ntt, size_t count,
                         double* coeffs, hipStream_t stream) {
  PHX_CAPI_GUARD({
    phantom::compose_raw(phantom_capi_context(ctx), chain_index, plain_ntt, nullptr, count, 1.0, coeffs, stream);
    return PHANTOM_OK;
  });
}

int phantom_ckks_encode(const phantom_context* ctx, size_t chain_index, int ext, const double* values,
                        size_t num_values, size_t sparse_slots, double scale, size_t count, uint64_t* out,
                        int* dev_overflow, hipStream_t stream) {
  PHX_CAPI_GUARD({
    phantom::encode_raw(phantom_capi_context(ctx), chain_index, ext != 0,
                        reinterpret_cast<const std::complex<double>*>(values), num_values, sparse_slots, scale, count,
                        out, nullptr, dev_overflow, stream);
    return PHANTOM_OK;
  });
}

int phantom_ckks_encode_sub(const phantom_context* ctx, size_t chain_index, int ext, const double* values,
                            size_t num_values, size_t sub_slots, double scale, size_t count, uint64_t* out,
                            int* dev_overflow, hipStream_t stream) {
  PHX_CAPI_GUARD({
    phantom::encode_sub_raw(phantom_capi_context(ctx), chain_index, ext != 0,
                            reinterpret_cast<const std::complex<double>*>(values), num_values, sub_slots, scale, count,
                            out, dev_overflow, stream);
    return PHANTOM_OK;
  });
}

int phantom_sub_ntt(const phantom_context* ctx, size_t chain_index, int ext, size_t sub_degree, int inverse,
                    uint64_t* data, size_t count, hipStream_t stream) {
  PHX_CAPI_GUARD({
    phantom::sub_ntt_raw(phantom_capi_context(ctx), chain_index, ext != 0, sub_degree, inverse != 0, data, count,
                         stream);
    return PHANTOM_OK;
  });
}

int phantom_ckks_decode(const phantom_context* ctx, size_t chain_index, const uint64_t* plain, double scale,
                        size_t count, double* values, hipStream_t stream) {
  PHX_CAPI_GUARD({
    phantom::decode_raw(phantom_capi_context(ctx), chain_index, plain, nullptr, scale, count,
                        reinterpret_cast<std::complex<double>*>(values), stream);
    return PHANTOM_OK;
  });
}

}  // extern "C"
