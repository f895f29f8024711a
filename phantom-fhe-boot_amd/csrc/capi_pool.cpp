// capi_pool.cpp — C-ABI of the hoisted average pooling + fully connected layer (declared in
// include/phantom_amd.h): the channel mix, the rotate-and-sum key switch, the rotation amounts and
// the whole layer on raw ciphertexts (host/avgpool.h).
#include <vector>

#include "../host/avgpool.h"
#include "../host/buffer.h"
#include "../host/capi_internal.h"
#include "../host/context.h"
#include "../host/rns_tool.h"
#include "phantom_amd.h"
#include "rns.h"

using phantom::capi::fail;
using phantom::capi::from_hip;

const phantom::PhantomContext& phantom_capi_context(const phantom_context* c);  // capi_ckks.cpp
const uint64_t* const* phantom_capi_key_array(const phantom_context* c, const uint64_t* const* host, size_t dnum,
                                              size_t need);

extern "C" {

int phantom_ct_mix(const phantom_context* ctx, size_t chain_index, const uint64_t* const* ins, size_t K,
                   const uint64_t* coef, const uint64_t* cadd, uint64_t* const* outs, size_t M, hipStream_t stream) {
  PHX_CAPI_GUARD({
    const auto& pc = phantom_capi_context(ctx);
    if (!ins || !coef || !outs) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null pointer");
    if (K == 0 || M == 0 || K > (size_t(1) << 20) || M > (size_t(1) << 16))
      return fail(PHANTOM_ERR_INVALID_ARGUMENT, "term and output counts must be at least 1");
    if (chain_index < 1 || chain_index >= pc.total_parm_size())
      return fail(PHANTOM_ERR_INVALID_ARGUMENT, "invalid chain index");
    const size_t L = pc.get_context_data(chain_index).gpu_rns_tool().size_Ql();
    phantom::DeviceBuffer<uint64_t> table(phantom::mix_table_words(K, M, L), stream);
    phantom::ct_mix_raw(pc, chain_index, ins, K, coef, cadd, outs, M, table.get(), stream);
    return PHANTOM_OK;
  });
}

int phantom_rotate_sum_ext(const phantom_context* ctx, size_t chain_index, const uint64_t* ct, const uint64_t* digits,
                           const uint64_t* const* const* key_digits, size_t dnum, const uint32_t* galois_elts,
                           size_t count, int identity, uint64_t* out, hipStream_t stream) {
  PHX_CAPI_GUARD({
    const auto& pc = phantom_capi_context(ctx);
    if (!ct || !digits || !key_digits || !galois_elts || !out) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null pointer");
    if (count < 1 || count > phx::kKsSumMax) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "1 to 63 rotations");
    if (chain_index < 1 || chain_index >= pc.total_parm_size())
      return fail(PHANTOM_ERR_INVALID_ARGUMENT, "invalid chain index");
    if (pc.size_P() == 0) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "no special primes");
    const auto& rt = pc.get_context_data(chain_index).gpu_rns_tool();
    const size_t n = pc.poly_degree(), Ql = rt.size_Ql(), QlP = Ql + pc.size_P();
    for (size_t k = 0; k < count; ++k)
      if (!key_digits[k]) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null rotation key");
    std::vector<phx::KsSumEntry> e(count);
    for (size_t k = 0; k < count; ++k) {
      e[k].evk = phantom_capi_key_array(ctx, key_digits[k], dnum, rt.beta());
      e[k].perm = pc.galois_perm(galois_elts[k]);
    }
    phantom::DeviceBuffer<phx::KsSumEntry> table;
    table.upload(e, stream);
    phx::KsRotateSumArgs a;
    a.digits = digits;
    a.entries = table.get();
    a.count = static_cast<uint32_t>(count);
    a.identity = identity ? 1 : 0;
    a.qp = pc.mod_QP().q;
    a.qp_barrett = pc.mod_QP().barrett;
    a.ct = ct;
    a.pmod = rt.bigP_mod_q();
    a.pmod_shoup = rt.bigP_mod_q_shoup();
    a.out = out;
    a.ql = static_cast<uint32_t>(Ql);
    a.qlp = static_cast<uint32_t>(QlP);
    a.size_q = static_cast<uint32_t>(pc.size_Q());
    a.size_p = static_cast<uint32_t>(pc.size_P());
    a.beta = static_cast<uint32_t>(rt.beta());
    const hipError_t err = phx::keyswitch_rotate_sum(a, n, stream);
    PHX_CHECK(hipStreamSynchronize(stream));  // the entry table is freed on return
    return from_hip(err);
  });
}

int phantom_avgpool_rotations(size_t width, size_t slotstr, int* out, size_t capacity, size_t* count) {
  PHX_CAPI_GUARD({
    if (!out || !count) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null pointer");
    phantom::avgpool_shape(size_t(1) << 63, width, slotstr);  // the shape alone: no ring degree at hand
    const std::vector<int> r = phantom::avgpool_rotations(width, slotstr);
    *count = r.size();
    if (capacity < r.size()) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "capacity below 2 (width - 1) rotations");
    for (size_t i = 0; i < r.size(); ++i) out[i] = r[i];
    return PHANTOM_OK;
  });
}

int phantom_avgpool_fc(const phantom_context* ctx, size_t chain_index, const uint64_t* const* cts, size_t t, size_t T,
                       size_t width, size_t slotstr, const uint64_t* coef, const uint64_t* cadd_bias,
                       const uint64_t* const* const* col_keys, const uint64_t* const* const* row_keys, size_t dnum,
                       const uint32_t* col_elts, const uint32_t* row_elts, uint64_t* const* outs, hipStream_t stream) {
  PHX_CAPI_GUARD({
    const auto& pc = phantom_capi_context(ctx);
    if (!cts || !coef || !cadd_bias || !col_keys || !row_keys || !col_elts || !row_elts || !outs)
      return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null pointer");
    if (t == 0 || T == 0 || t > (size_t(1) << 20) || T > (size_t(1) << 16))
      return fail(PHANTOM_ERR_INVALID_ARGUMENT, "no channels");
    phantom::avgpool_shape(pc.poly_degree(), width, slotstr);
    if (chain_index < 1 || chain_index >= pc.total_parm_size())
      return fail(PHANTOM_ERR_INVALID_ARGUMENT, "invalid chain index");
    if (pc.size_P() == 0) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "no special primes");
    const size_t beta = pc.get_context_data(chain_index).gpu_rns_tool().beta(), R = width - 1;
    // every check before the first key array is uploaded (avgpool_fc_raw repeats them before it enqueues)
    for (size_t k = 0; k < t; ++k)
      if (!cts[k]) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null input channel");
    for (size_t u = 0; u < T; ++u)
      if (!outs[u]) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null output channel");
    for (size_t i = 0; i < R; ++i)
      if (!col_keys[i] || !row_keys[i]) return fail(PHANTOM_ERR_INVALID_ARGUMENT, "null rotation key");
    std::vector<const uint64_t* const*> col(R), row(R);
    for (size_t i = 0; i < R; ++i) {
      col[i] = phantom_capi_key_array(ctx, col_keys[i], dnum, beta);
      row[i] = phantom_capi_key_array(ctx, row_keys[i], dnum, beta);
    }
    phantom::avgpool_fc_raw(pc, chain_index, cts, t, T, width, slotstr, coef, cadd_bias, col.data(), row.data(), col_elts,
                            row_elts, outs, stream);
    return PHANTOM_OK;
  });
}

}  // extern "C"
