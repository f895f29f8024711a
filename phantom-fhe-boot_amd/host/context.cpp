#include "context.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <stdexcept>
#include <thread>

#include "hip_check.h"
#include "numth.h"
#include "../csrc/ntt.h"
#include "../csrc/rns.h"

namespace phantom {

PhantomContext::PhantomContext(const EncryptionParameters& params, hipStream_t stream) : params_(params) {
  if (stream) {
    stream_.s = stream;
  } else {
    PHX_CHECK(hipStreamCreateWithFlags(&stream_.s, hipStreamNonBlocking));
    stream_.owned = true;
  }
  for (int l = 1; l < kLanes; ++l) {
    PHX_CHECK(hipStreamCreateWithFlags(&lane_main_[l].s, hipStreamNonBlocking));
    lane_main_[l].owned = true;
  }
  for (auto& lane : aux_) {
    for (auto& a : lane) {
      PHX_CHECK(hipStreamCreateWithFlags(&a.s, hipStreamNonBlocking));
      a.owned = true;
    }
  }
  hipStream_t s = stream_.s;
  if (params.scheme() != scheme_type::ckks) throw std::invalid_argument("only CKKS is supported by this engine");
  const auto& mods = params.coeff_modulus();
  if (mods.size() < 2) throw std::invalid_argument("The coefficient modulus must be a vector of at least two primes");
  n_ = params.poly_modulus_degree();
  size_P_ = params.special_modulus_size();
  if (size_P_ >= mods.size()) throw std::invalid_argument("special modulus size too large");
  size_Q_ = mods.size() - size_P_;
  for (const auto& m : mods) qp_.push_back(m.value());

  // keep freed stream-ordered allocations cached (src/context.cu:127-131)
  int dev = 0;
  PHX_CHECK(hipGetDevice(&dev));
  hipMemPool_t pool;
  if (hipDeviceGetDefaultMemPool(&pool, dev) == hipSuccess) {
    uint64_t threshold = UINT64_MAX;
    (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &threshold);
  }

  ws_ = std::make_unique<Workspace>();
  ntt_ = std::make_unique<DeviceNttTables>(n_, qp_, s);
  data_.push_back(std::make_unique<ContextData>(0, qp_, &params_));
  for (size_t c = 1; c <= size_Q_; ++c) {
    std::vector<uint64_t> ql(qp_.begin(), qp_.begin() + (size_Q_ - (c - 1)));
    data_.push_back(std::make_unique<ContextData>(c, ql, &params_));
  }
  // per-level RNS tools (host constant generation is O(L^2) per level; run levels in parallel)
  std::vector<std::unique_ptr<RnsTool>> tools(size_Q_ + 1);
  {
    std::vector<std::thread> th;
    const unsigned nt = std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 8u);
    std::vector<std::exception_ptr> errs(nt);
    for (unsigned w = 0; w < nt; ++w)
      th.emplace_back([&, w] {
        try {
          for (size_t c = 1 + w; c <= size_Q_; c += nt)
            tools[c] = std::make_unique<RnsTool>(n_, qp_, size_P_, size_Q_ - (c - 1), s);
        } catch (...) {
          errs[w] = std::current_exception();
        }
      });
    for (auto& t : th) t.join();
    for (auto& e : errs)
      if (e) std::rethrow_exception(e);
  }
  for (size_t c = 1; c <= size_Q_; ++c) {
    tools[c]->set_workspace(ws_.get());
    data_[c]->set_rns_tool(std::move(tools[c]));
  }
  PHX_CHECK(hipStreamSynchronize(s));
  if (const char* e = std::getenv("PHX_UNBIASED_MODDOWN"); e && e[0] == '1') set_unbiased_moddown(true);
}

void PhantomContext::set_unbiased_moddown(bool on) {
  hipStream_t s = stream_.s;
  if (on && !ones_ntt_.get()) {
    std::vector<uint64_t> h(size_Q_ * n_, 1);
    ones_ntt_.upload(h, s);
    PHX_CHECK(phx::ntt_forward(ntt_->get(), ones_ntt_.get(), ones_ntt_.get(),
                               phx::LimbMap::contiguous(static_cast<int>(size_Q_), 0), s));
  }
  for (size_t c = 1; c <= size_Q_; ++c) data_[c]->gpu_rns_tool_mutable().set_unbias(on ? ones_ntt_.get() : nullptr, s);
  PHX_CHECK(hipStreamSynchronize(s));
  unbiased_ = on;
}

std::vector<uint32_t> PhantomContext::key_galois_elts() const {
  if (!params_.galois_elts().empty()) return params_.galois_elts();
  const uint64_t m = 2 * static_cast<uint64_t>(n_);
  std::vector<uint32_t> elts{static_cast<uint32_t>(m - 1)};
  uint64_t pos = 5, neg = arith::inv_mod(5, m);
  for (size_t i = 0; i + 1 < static_cast<size_t>(arith::log2_exact(n_)); ++i) {
    elts.push_back(static_cast<uint32_t>(pos));
    pos = pos * pos & (m - 1);
    elts.push_back(static_cast<uint32_t>(neg));
    neg = neg * neg & (m - 1);
  }
  return elts;
}

const uint32_t* PhantomContext::galois_perm(uint32_t elt) const {
  std::lock_guard<std::mutex> lk(cache_mu_);
  auto it = perms_.find(elt);
  if (it != perms_.end()) return it->second.get();
  if (!(elt & 1) || elt >= 2 * n_) throw std::invalid_argument("invalid Galois element");
  const int logn = arith::log2_exact(n_);
  std::vector<uint32_t> perm(n_);  // [n] permutation, then [n / bsz] block inverse
  for (uint32_t j = 0; j < n_; ++j) {
    const uint64_t idx = ((2ull * j + 1) * elt) % (2ull * n_);
    perm[arith::reverse_bits(j, logn)] = arith::reverse_bits(static_cast<uint32_t>(idx >> 1), logn);
  }
  // + the block inverse (galois_block_inv): output block ob reads source block perm[ob bsz] / bsz
  const uint32_t bsz = static_cast<uint32_t>(std::min<size_t>(n_, phx::kGaloisBlock)), nb = static_cast<uint32_t>(n_) / bsz;
  perm.resize(n_ + nb);
  for (uint32_t ob = 0; ob < nb; ++ob) perm[n_ + perm[static_cast<size_t>(ob) * bsz] / bsz] = ob;
  DeviceBuffer<uint32_t> d;
  d.upload(perm, stream_.s);
  return perms_.emplace(elt, std::move(d)).first->second.get();
}

const uint64_t* PhantomContext::monomial_ntt(uint32_t power, size_t L) const {
  const uint32_t pr = power % static_cast<uint32_t>(2 * n_);
  std::lock_guard<std::mutex> lk(cache_mu_);
  auto key = std::make_pair(pr, L);
  auto it = monomials_.find(key);
  if (it != monomials_.end()) return it->second.get();
  if (L > qp_.size()) throw std::invalid_argument("too many limbs");
  std::vector<uint64_t> h(L * n_, 0);
  for (size_t l = 0; l < L; ++l) h[l * n_ + pr % n_] = pr < n_ ? 1 : qp_[l] - 1;
  DeviceBuffer<uint64_t> d;
  d.upload(h, stream_.s);
  PHX_CHECK(phx::ntt_forward(ntt_->get(), d.get(), d.get(), phx::LimbMap::contiguous(static_cast<int>(L), 0), stream_.s));
  PHX_CHECK(hipStreamSynchronize(stream_.s));
  return monomials_.emplace(key, std::move(d)).first->second.get();
}

// the embedding tables of ring degree n (the caller holds cache_mu_)
void PhantomContext::build_embed(size_t n, DeviceBuffer<double2>& zeta_out, DeviceBuffer<uint32_t>& slot_of_out) const {
  const size_t m = 2 * n;
  std::vector<double2> zeta(m);
  for (size_t j = 0; j < m; ++j) {
    const double a = 2.0 * M_PI * static_cast<double>(j) / static_cast<double>(m);
    zeta[j] = make_double2(std::cos(a), std::sin(a));
  }
  // position (5^j mod 2n - 1) / 2 holds slot j, its mirror n - 1 - that the conjugate
  std::vector<uint32_t> slot_of(n);
  uint64_t p = 1;
  for (size_t j = 0; j < n / 2; ++j) {
    const size_t idx = static_cast<size_t>((p - 1) / 2);
    slot_of[idx] = static_cast<uint32_t>(j);
    slot_of[n - 1 - idx] = static_cast<uint32_t>(j) | phx::EmbedTables::kConjBit;
    p = (p * 5) % m;
  }
  DeviceBuffer<uint32_t> d;
  d.upload(slot_of, stream_.s);
  slot_of_out = std::move(d);
  DeviceBuffer<double2> z;
  z.upload(zeta, stream_.s);
  zeta_out = std::move(z);
}

phx::EmbedTables PhantomContext::embed_tables() const {
  std::lock_guard<std::mutex> lk(cache_mu_);
  if (!embed_zeta_) build_embed(n_, embed_zeta_, embed_slot_of_);
  phx::EmbedTables t;
  t.n = n_;
  t.log_n = arith::log2_exact(n_);
  t.zeta = embed_zeta_.get();
  t.slot_of = embed_slot_of_.get();
  return t;
}

void PhantomContext::check_sub_degree(size_t sub_degree) const {
  if (sub_degree < 8 || sub_degree > n_ || (sub_degree & (sub_degree - 1)))
    throw std::invalid_argument("the subring degree must be a power of two in [8, N]");
}

const phx::NttTables& PhantomContext::sub_ntt_tables(size_t sub_degree) const {
  check_sub_degree(sub_degree);
  if (sub_degree == n_) return ntt_->get();
  std::lock_guard<std::mutex> lk(cache_mu_);
  auto it = sub_ntt_.find(sub_degree);
  if (it == sub_ntt_.end()) {
    // root psi_N^(N/M) per modulus: the subring's twiddles are the first M of the context's
    const std::vector<uint64_t>& psi = ntt_->roots();
    std::vector<uint64_t> roots(qp_.size());
    for (size_t i = 0; i < qp_.size(); ++i) roots[i] = arith::pow_mod(psi[i], n_ / sub_degree, qp_[i]);
    it = sub_ntt_.emplace(sub_degree, std::make_unique<DeviceNttTables>(sub_degree, qp_, roots, stream_.s)).first;
  }
  return it->second->get();
}

phx::EmbedTables PhantomContext::sub_embed_tables(size_t sub_degree) const {
  check_sub_degree(sub_degree);
  if (sub_degree == n_) return embed_tables();
  std::lock_guard<std::mutex> lk(cache_mu_);
  SubEmbed& e = sub_embed_[sub_degree];
  if (!e.zeta) build_embed(sub_degree, e.zeta, e.slot_of);
  phx::EmbedTables t;
  t.n = sub_degree;
  t.log_n = arith::log2_exact(sub_degree);
  t.zeta = e.zeta.get();
  t.slot_of = e.slot_of.get();
  return t;
}

phx::ComposeTables PhantomContext::compose_tables(size_t chain_index) const {
  if (chain_index < 1 || chain_index >= data_.size()) throw std::invalid_argument("invalid chain index");
  const std::vector<uint64_t>& q = data_[chain_index]->moduli();
  const size_t L = q.size();
  if (L > static_cast<size_t>(phx::kMaxComposeLimbs)) throw std::invalid_argument("too many limbs to compose");
  std::lock_guard<std::mutex> lk(cache_mu_);
  auto it = compose_.find(chain_index);
  if (it == compose_.end()) {
    using namespace arith;
    // layout: prefix [L][L], prefix_shoup [L][L], inv_prefix [L] + Shoup [L], half_digits [L]
    std::vector<uint64_t> h(2 * L * L + 3 * L, 0);
    uint64_t* prefix = h.data();
    uint64_t* prefix_shoup = prefix + L * L;
    uint64_t* inv_prefix = prefix_shoup + L * L;
    uint64_t* half = inv_prefix + 2 * L;
    for (size_t i = 0; i < L; ++i) {
      uint64_t pr = 1 % q[i];
      for (size_t j = 0; j < i; ++j) {
        prefix[i * L + j] = pr;
        prefix_shoup[i * L + j] = shoup(pr, q[i]);
        pr = mul_mod(pr, q[j] % q[i], q[i]);
      }
      inv_prefix[i] = i ? inv_mod(pr, q[i]) : 1;
      inv_prefix[L + i] = shoup(inv_prefix[i], q[i]);
    }
    // mixed-radix digits of (Q - 1) / 2, whose residue mod q_i is (q_i - 1) / 2
    for (size_t i = 0; i < L; ++i) {
      uint64_t acc = 0;
      for (size_t j = 0; j < i; ++j) acc = (acc + mul_mod(half[j] % q[i], prefix[i * L + j], q[i])) % q[i];
      const uint64_t d = ((q[i] - 1) / 2 + q[i] - acc) % q[i];
      half[i] = mul_mod(d, inv_prefix[i], q[i]);
    }
    DeviceBuffer<uint64_t> d;
    d.upload(h, stream_.s);
    it = compose_.emplace(chain_index, std::move(d)).first;
  }
  phx::ComposeTables c;
  c.L = static_cast<int>(L);
  c.prefix = it->second.get();
  c.prefix_shoup = c.prefix + L * L;
  c.inv_prefix = c.prefix_shoup + L * L;
  c.half_digits = c.inv_prefix + 2 * L;
  return c;
}

}  // namespace phantom
