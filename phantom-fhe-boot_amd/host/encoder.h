// encoder.h — PhantomCKKSEncoder (include/ckks.h, src/ckks.cu): slots <-> NTT-form plaintexts.
//
// Slot j sits at the root zeta^(5^j) of X^N + 1 (zeta = exp(2 pi i / 2N)) and its conjugate at
// zeta^(-5^j), the convention of the reference and of every 5^j rotation group.  The canonical
// embedding and its inverse are evaluated on the host in double precision with one size-N
// complex FFT each (the reference runs its special FFT on the GPU, src/fft.cu); coefficients
// are rounded to integers, reduced into each RNS limb exactly and moved to NTT form on the GPU.
//
// The *_device / *_on_device members run the whole chain on the GPU instead (csrc/encode.h: FP64
// embedding, round and split, CRT composition), stream-ordered and batched.  The host members
// are unchanged and remain what the bootstrap's setup (unless FHECKKSRNS::UseDeviceSetup) and the
// boot session call: the device embedding follows the host FFT's butterfly order, but nothing pins
// the two paths to identical bits, so switching those callers may change their plaintexts' low bits.
#pragma once

#include <complex>
#include <cstdint>
#include <span>
#include <vector>

#include "ciphertext.h"
#include "context.h"

namespace phantom {

class PhantomCKKSEncoder {
 public:
  explicit PhantomCKKSEncoder(const PhantomContext& ctx);
  // host-only maps (slots_to_coeffs / coeffs_to_slots) for ring degree n, no device use
  explicit PhantomCKKSEncoder(size_t n);

  size_t slot_count() const { return n_ / 2; }

  // encode(context, values, scale, plain[, chain_index]) (src/ckks.cu): plaintext in the Ql basis
  // of `chain_index`, NTT form.  Fewer values than slots are zero-padded.
  void encode(const PhantomContext& ctx, const std::vector<std::complex<double>>& values, double scale,
              PhantomPlaintext& out, size_t chain_index = 1) const;
  void encode(const PhantomContext& ctx, const std::vector<double>& values, double scale, PhantomPlaintext& out,
              size_t chain_index = 1) const;
  // sparse packing (the reference's set_sparse_encode / encode_sparse, include/ckks.h:82-117,
  // bootstrapping_example.cu:262-263): `values` (at most sparse_slots of them, zero-padded) fill
  // every block of sparse_slots slots, i.e. the plaintext is m'(X^(N / (2 sparse_slots))), the form
  // a sparse bootstrap expects.  set_sparse_encode takes the subring dimension 2 * sparse_slots.
  void set_sparse_encode(size_t subring_degree) { sparse_slots_ = subring_degree / 2; }
  void set_sparse_encode(const EncryptionParameters& parms, size_t subring_degree) {
    (void)parms;
    set_sparse_encode(subring_degree);
  }
  void encode_sparse(const PhantomContext& ctx, const std::vector<double>& values, double scale, PhantomPlaintext& out,
                     size_t chain_index = 1) const;
  void encode_sparse(const PhantomContext& ctx, const std::vector<std::complex<double>>& values, double scale,
                     PhantomPlaintext& out, size_t chain_index = 1) const;
  size_t sparse_slots() const { return sparse_slots_; }

  // encode_ext (the hoisted linear transforms' plaintexts): the Ql basis of `chain_index`
  // followed by the special primes P, NTT form ([size_Ql + size_P][n]).
  void encode_ext(const PhantomContext& ctx, const std::vector<std::complex<double>>& values, double scale,
                  PhantomPlaintext& out, size_t chain_index) const;
  // encode_ext in two halves, so many plaintexts can be prepared on host threads at once: the
  // host residues (coefficient form, limb-major; `rns_threads` 0 = spread limbs over threads)
  // and their upload + NTT on the context's stream.  `host` must stay alive until the stream
  // has run the upload (synchronise it before reusing or freeing `host`).
  void encode_ext_host(const PhantomContext& ctx, const std::vector<std::complex<double>>& values, double scale,
                       size_t chain_index, std::vector<uint64_t>& host, unsigned rns_threads = 0) const;
  void upload_ext_async(const PhantomContext& ctx, const std::vector<uint64_t>& host, double scale,
                        PhantomPlaintext& out, size_t chain_index) const;

  // decode(context, plain, values) (src/ckks.cu): exact CRT composition of each coefficient,
  // centered, divided by the plaintext's scale, then the canonical embedding.
  void decode(const PhantomContext& ctx, const PhantomPlaintext& plain, std::vector<std::complex<double>>& out) const;
  void decode(const PhantomContext& ctx, const PhantomPlaintext& plain, std::vector<double>& out) const;
  // decode<T>(context, plain) (include/ckks.h:174-206): T = std::complex<double> (the reference's
  // cuDoubleComplex) or double
  template <class T>
  std::vector<T> decode(const PhantomContext& ctx, const PhantomPlaintext& plain) const {
    std::vector<T> v;
    decode(ctx, plain, v);
    return v;
  }

  // ---- device encoder: values and results in device memory, enqueued on ctx.stream(), no host
  // synchronisation.  `dev_overflow` (device int, may be null) is set non-zero when a value times
  // the scale is not finite or reaches 2^1000; it is never cleared here.
  // encode: `num_values` (<= slots, zero-padded) complex values -> plaintext in the Ql basis
  void encode_device(const PhantomContext& ctx, const std::complex<double>* dev_values, size_t num_values,
                     double scale, PhantomPlaintext& out, size_t chain_index = 1, int* dev_overflow = nullptr) const;
  // encode_sparse: the values tile every block of sparse_slots() slots
  void encode_sparse_device(const PhantomContext& ctx, const std::complex<double>* dev_values, size_t num_values,
                            double scale, PhantomPlaintext& out, size_t chain_index = 1,
                            int* dev_overflow = nullptr) const;
  // encode_ext: Ql of `chain_index` followed by P
  void encode_ext_device(const PhantomContext& ctx, const std::complex<double>* dev_values, size_t num_values,
                         double scale, PhantomPlaintext& out, size_t chain_index, int* dev_overflow = nullptr) const;
  // batched encode_ext: outs.size() x slot_count() values fill `outs` in shared launches
  void encode_ext_device(const PhantomContext& ctx, const std::complex<double>* dev_values, double scale,
                         std::span<PhantomPlaintext> outs, size_t chain_index, int* dev_overflow = nullptr) const;
  // decode: slot_count() complex values to dev_out; the plaintext is not modified
  void decode_device(const PhantomContext& ctx, const PhantomPlaintext& plain, std::complex<double>* dev_out) const;
  // host-vector convenience forms computed on the GPU: upload, run, synchronise; encode throws
  // std::invalid_argument("encoded values are too large") as the host path does
  void encode_on_device(const PhantomContext& ctx, const std::vector<std::complex<double>>& values, double scale,
                        PhantomPlaintext& out, size_t chain_index = 1) const;
  void decode_on_device(const PhantomContext& ctx, const PhantomPlaintext& plain,
                        std::vector<std::complex<double>>& out) const;

  // host-side maps, exposed for the bootstrap precomputation and tests
  // slots -> real coefficients (inverse canonical embedding, coefficients not scaled)
  std::vector<double> slots_to_coeffs(const std::vector<std::complex<double>>& values) const;
  // real coefficients -> slots
  std::vector<std::complex<double>> coeffs_to_slots(const std::vector<double>& coeffs) const;

 private:
  // rounds coeffs * scale and writes residues for `moduli` (limb-major) to `out` (host)
  static void to_rns(const std::vector<double>& coeffs, double scale, const std::vector<uint64_t>& moduli,
                     std::vector<uint64_t>& out, unsigned threads = 0);
  void fft(std::vector<std::complex<double>>& a, bool inverse) const;

  size_t n_ = 0;
  int logn_ = 0;
  size_t sparse_slots_ = 0;
  std::vector<std::complex<double>> zeta_pows_;  // zeta^j, j < 2n
  std::vector<uint32_t> slot_index_;             // (5^j mod 2n - 1) / 2 for j < n/2
  std::vector<uint32_t> brev_;
};

// The device encoder on raw pointers, shared by the members above and the C-ABI
// (csrc/capi_encode.cpp).  Complex data is interleaved (re, im) doubles.  Arguments are checked
// (std::invalid_argument) before anything is enqueued on `s`.
// limbs of a plaintext at chain_index: its Ql basis, or Ql followed by P (upload_ext_async's layout)
phx::LimbMap encode_limb_map(const PhantomContext& ctx, size_t chain_index, bool ext);
// throws unless sparse_slots (0 = n / 2) is a power of two <= n / 2 that holds num_values
void check_sparse(size_t n, size_t sparse_slots, size_t num_values);
// the embedding alone.  inverse: count x ns complex -> count x n reals (ns = sparse_slots or n/2,
// the values tiling every block of ns slots); forward: count x n reals -> count x ns complex
void embed_raw(const PhantomContext& ctx, bool forward, const void* in, void* out, size_t sparse_slots, size_t count,
               hipStream_t s);
// out [count][limbs][n] = round(coeffs * scale) mod q, coefficient or NTT form
void round_rns_raw(const PhantomContext& ctx, size_t chain_index, bool ext, const double* coeffs, double scale,
                   size_t count, bool ntt_form, uint64_t* out, int* dev_overflow, hipStream_t s);
// plaintexts (NTT form, Ql basis; `plain` contiguous or `plains` one pointer each) -> mul x centred integer
void compose_raw(const PhantomContext& ctx, size_t chain_index, const uint64_t* plain, const uint64_t* const* plains,
                 size_t count, double mul, double* coeffs, hipStream_t s);
// values [count][num_values] -> plaintexts, written to `out` (contiguous) or to outs[p]
void encode_raw(const PhantomContext& ctx, size_t chain_index, bool ext, const std::complex<double>* values,
                size_t num_values, size_t sparse_slots, double scale, size_t count, uint64_t* out,
                uint64_t* const* outs, int* dev_overflow, hipStream_t s);
void decode_raw(const PhantomContext& ctx, size_t chain_index, const uint64_t* plain, const uint64_t* const* plains,
                double scale, size_t count, std::complex<double>* values, hipStream_t s);
// The compact sparse encoder (the reference's sparse path, src/ckks.cu:180-270: a size-ns FFT,
// decompose_array over 2 ns coefficients, extend_sparse_ckks).  A plaintext whose sub_slots = ns
// values tile every block of ns slots is p'(X^(N / 2 ns)) up to rounding; this writes p' alone:
// values [count][num_values] (zero-padded to ns) -> out [count][limbs][M], M = 2 ns, the size-M
// inverse embedding, round and split over M coefficients, and the size-M forward NTT of
// PhantomContext::sub_ntt_tables(M).  Word e of the full-size NTT-form plaintext is word
// e >> log2(N / M) of this one.  With ns = N / 2 it is encode_raw bit for bit.
void encode_sub_raw(const PhantomContext& ctx, size_t chain_index, bool ext, const std::complex<double>* values,
                    size_t num_values, size_t sub_slots, double scale, size_t count, uint64_t* out, int* dev_overflow,
                    hipStream_t s);
// the subring transform in place on data [count][limbs][sub_degree]; the inverse includes M^-1
void sub_ntt_raw(const PhantomContext& ctx, size_t chain_index, bool ext, size_t sub_degree, bool inverse,
                 uint64_t* data, size_t count, hipStream_t s);

}  // namespace phantom
