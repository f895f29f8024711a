// lt_levels.cpp — the linear-transform setup (lt_levels.h): the slot-domain maps, the level plan and
// finish, and FHECKKSRNS's level builders with their host and device back ends.
#include "lt_levels.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <set>
#include <stdexcept>
#include <string>
#include <thread>

#include "bootstrap.h"
#include "numth.h"

namespace phantom {

namespace boot {

static std::complex<double> root_of_unity(uint64_t e, uint64_t M) {
  const double a = 2.0 * M_PI * static_cast<double>(e % M) / static_cast<double>(M);
  return {std::cos(a), std::sin(a)};
}

DiagMap stage(size_t n, int s, bool inverse) {
  const size_t m = size_t(1) << s, h = m / 2, M = 4 * n;
  if (m > n) throw std::invalid_argument("stage out of range");
  std::vector<uint64_t> pw(h);  // 5^j mod 4m
  uint64_t p5 = 1;
  for (size_t j = 0; j < h; ++j) {
    pw[j] = p5;
    p5 = p5 * 5 % (4 * m);
  }
  cvec d0(n), dp(n), dm(n);
  for (size_t p = 0; p < n; ++p) {
    const size_t j = p % m;
    if (j < h) {
      const std::complex<double> t = root_of_unity((n / m) * pw[j], M);
      d0[p] = inverse ? 0.5 : 1.0;
      dp[p] = inverse ? std::complex<double>(0.5) : t;
    } else {
      const std::complex<double> t = root_of_unity((n / m) * pw[j - h], M);
      if (inverse) {
        dm[p] = std::conj(t) * 0.5;
        d0[p] = -std::conj(t) * 0.5;
      } else {
        d0[p] = -t;
        dm[p] = 1.0;
      }
    }
  }
  DiagMap d;
  auto add = [&](int a, const cvec& v) {
    auto it = d.find(a);
    if (it == d.end()) {
      d.emplace(a, v);
    } else {
      for (size_t i = 0; i < n; ++i) it->second[i] += v[i];
    }
  };
  add(0, d0);
  add(static_cast<int>(h % n), dp);
  add(static_cast<int>((n - h) % n), dm);
  return d;
}

DiagMap compose(const DiagMap& A, const DiagMap& B, size_t n) {
  DiagMap out;
  for (const auto& [a, alpha] : A)
    for (const auto& [b, beta] : B) {
      const int key = static_cast<int>((static_cast<size_t>(a) + static_cast<size_t>(b)) % n);
      cvec& dst = out[key];
      if (dst.empty()) dst.assign(n, {0.0, 0.0});
      for (size_t p = 0; p < n; ++p) dst[p] += alpha[p] * beta[(p + a) % n];
    }
  return out;
}

DiagMap lift_blocks(const DiagMap& T, size_t n, size_t S, const cvec* out_mask, const cvec* in_mask) {
  if (S % n) throw std::invalid_argument("slot count not a multiple of the block size");
  DiagMap out;
  for (const auto& [a, d] : T) {
    for (size_t p = 0; p < S; ++p) {
      const size_t r = p % n;
      std::complex<double> v = d[r];
      if (v == std::complex<double>(0.0, 0.0)) continue;
      // the pair (p, p + a) of the n-dim map stays inside p's block: offset a or a - n
      const long off = r + static_cast<size_t>(a) < n ? static_cast<long>(a) : static_cast<long>(a) - static_cast<long>(n);
      const size_t key = static_cast<size_t>(((off % static_cast<long>(S)) + static_cast<long>(S)) % static_cast<long>(S));
      const size_t q = (p + key) % S;
      if (out_mask) v *= (*out_mask)[p % out_mask->size()];
      if (in_mask) v *= (*in_mask)[q % in_mask->size()];
      cvec& dst = out[static_cast<int>(key)];
      if (dst.empty()) dst.assign(S, {0.0, 0.0});
      dst[p] += v;
    }
  }
  return out;
}

cvec apply(const DiagMap& T, const cvec& v) {
  const size_t n = v.size();
  cvec out(n, {0.0, 0.0});
  for (const auto& [a, d] : T)
    for (size_t p = 0; p < n; ++p) out[p] += d[p] * v[(p + a) % n];
  return out;
}

std::vector<int> split_stages(int logslots, uint32_t budget) {
  budget = std::clamp<uint32_t>(budget, 1, static_cast<uint32_t>(logslots));
  std::vector<int> sz(budget, logslots / static_cast<int>(budget));
  for (int i = 0; i < logslots % static_cast<int>(budget); ++i) ++sz[i];
  return sz;
}

std::vector<LevelSpec> plan_levels(size_t ns, size_t n, const std::vector<int>& sizes, bool encode_dir) {
  if (ns < 2 || (ns & (ns - 1)) || ns > n) throw std::invalid_argument("the slot count must be a power of two >= 2");
  const int logslots = arith::log2_exact(ns);
  int total = 0;
  for (int c : sizes) {
    if (c < 1) throw std::invalid_argument("a level without stages");
    total += c;
  }
  if (total != logslots) throw std::invalid_argument("the level sizes must sum to log2 of the slot count");
  std::vector<LevelSpec> levels(sizes.size());
  int next = encode_dir ? logslots : 1;  // CoeffToSlot: the inverse stages top-down
  for (size_t gi = 0; gi < sizes.size(); ++gi) {
    LevelSpec& lv = levels[gi];
    for (int t = 0; t < sizes[gi]; ++t, next += encode_dir ? -1 : 1) lv.stages.push_back(next);
    lv.stride = 1 << (*std::min_element(lv.stages.begin(), lv.stages.end()) - 1);
    const bool first = gi == 0, last = gi + 1 == sizes.size();
    lv.apply_const = encode_dir ? first : last;
    lv.mask = phx::kLtMaskNone;
    if (ns < n && encode_dir && last) lv.mask = phx::kLtMaskOut;
    if (ns < n && !encode_dir && first) lv.mask = phx::kLtMaskIn;
  }
  return levels;
}

LtShape lt_shape(const std::vector<int>& keys, size_t n, uint32_t dim1, int stride) {
  LtShape lv;
  lv.stride = stride;
  int kmin = 0, kmax = 0;
  for (int a : keys) {
    if (a > static_cast<int>(n / 2)) a -= static_cast<int>(n);
    if (a % lv.stride) throw std::logic_error("diagonal offset not a multiple of the stride");
    kmin = std::min(kmin, a / lv.stride);
    kmax = std::max(kmax, a / lv.stride);
  }
  lv.center = -kmin;
  lv.D = kmax - kmin + 1;
  lv.g = 1;
  if (dim1) {
    if (dim1 & (dim1 - 1)) throw std::invalid_argument("dim1 must be a power of two");
    lv.g = static_cast<int>(std::min<uint32_t>(dim1, static_cast<uint32_t>(phx::kLtMaxG)));
  } else {
    // g^2 >= 2 D: twice the baby steps of the square split.  A hoisted baby step is one fused
    // key switch + automorphism; a giant step is a moddown + modup (one INTT over Ql u P and an
    // NTT over every digit) before its key switch, so fewer giant steps pay: 256 diagonals as
    // g 32 x b 8 instead of 16 x 16 take the bootstrap from 29.7 to 27.9 ms
    // (profiles/r02/lt_baby_giant_split.txt); PHX_LT_SQUARE=1 restores the square split.
    static const bool square = std::getenv("PHX_LT_SQUARE") != nullptr;
    while (lv.g * lv.g < (square ? 1 : 2) * lv.D && lv.g < phx::kLtMaxG) lv.g *= 2;
  }
  lv.b = (lv.D + lv.g - 1) / lv.g;
  if (lv.g > phx::kLtMaxG || lv.b > phx::kLtMaxB) throw std::invalid_argument("linear transform level too large");
  return lv;
}

size_t StagePlan::max_diagonals() const {
  size_t d = 1;
  for (const auto& k : keys) d = std::max(d, k.size());
  return d;
}

StagePlan plan_stages(size_t ns, const std::vector<int>& stages) {
  if (ns < 2 || (ns & (ns - 1)) || ns > (size_t(1) << 24)) throw std::invalid_argument("the slot count must be a power of two >= 2");
  if (stages.empty()) throw std::invalid_argument("no stages");
  const int logns = arith::log2_exact(ns);
  for (int s : stages)
    if (s < 1 || s > logns) throw std::invalid_argument("stage out of range");
  StagePlan plan;
  plan.ns = ns;
  plan.stages = stages;
  std::vector<int> cur{0};
  const auto row_of = [](const std::vector<int>& keys, size_t key) {
    const auto it = std::lower_bound(keys.begin(), keys.end(), static_cast<int>(key));
    return it != keys.end() && *it == static_cast<int>(key) ? static_cast<int32_t>(it - keys.begin()) : int32_t(-1);
  };
  for (int s : stages) {
    const size_t h = size_t(1) << (s - 1);
    std::set<int> next;  // each stage adds {0, +h, -h mod ns}
    for (int b : cur)
      for (size_t a : {size_t(0), h % ns, (ns - h) % ns}) next.insert(static_cast<int>((a + static_cast<size_t>(b)) % ns));
    std::vector<int> keys(next.begin(), next.end());
    plan.src_at.push_back(plan.src.size());
    for (int c : keys) {
      plan.src.push_back(row_of(cur, static_cast<size_t>(c)));
      plan.src.push_back(row_of(cur, (static_cast<size_t>(c) + ns - h) % ns));
      plan.src.push_back(row_of(cur, (static_cast<size_t>(c) + h) % ns));
    }
    plan.keys.push_back(keys);
    cur = std::move(keys);
  }
  return plan;
}

void* stage_products_device(const PhantomContext& cc, const StagePlan& plan, bool inverse, const int32_t* dev_src,
                            void* first, void* second, hipStream_t stream) {
  if (!dev_src || !first || !second || first == second) throw std::invalid_argument("null pointer");
  if (plan.ns > cc.poly_degree() / 2) throw std::invalid_argument("more slots than the ring has");
  const phx::EmbedTables t = cc.embed_tables();
  double2 *out = static_cast<double2*>(first), *other = static_cast<double2*>(second);
  const double2* prev = nullptr;  // the identity
  for (size_t k = 0; k < plan.stages.size(); ++k) {
    const hipError_t e = phx::ltprep_stage(t.zeta, t.n, plan.ns, plan.stages[k], inverse, prev, out,
                                           dev_src + plan.src_at[k], static_cast<int>(plan.keys[k].size()), stream);
    if (e == hipErrorInvalidValue) throw std::invalid_argument("stage products: unsupported shape");
    if (e != hipSuccess) throw hip_error(e, "stage products");
    prev = out;
    std::swap(out, other);
  }
  return const_cast<double2*>(prev);
}

DiagMap stage_products_host(const StagePlan& plan, bool inverse) {
  DiagMap T;
  T.emplace(0, cvec(plan.ns, {1.0, 0.0}));
  for (int s : plan.stages) T = compose(stage(plan.ns, s, inverse), T, plan.ns);
  return T;
}

std::vector<int> lifted_keys(const std::vector<int>& offsets, const std::vector<int>& flags, size_t ns, size_t n) {
  if (flags.size() != 2 * offsets.size()) throw std::invalid_argument("two presence flags per offset");
  std::set<int> keys;
  for (size_t i = 0; i < offsets.size(); ++i) {
    if (ns == n) {
      if (flags[2 * i] || flags[2 * i + 1]) keys.insert(offsets[i]);
      continue;
    }
    if (flags[2 * i]) keys.insert(offsets[i]);
    if (flags[2 * i + 1]) keys.insert(static_cast<int>(n + static_cast<size_t>(offsets[i]) - ns));
  }
  return {keys.begin(), keys.end()};
}

static std::vector<int> offsets_of(const DiagMap& T) {
  std::vector<int> keys;
  for (const auto& kv : T) keys.push_back(kv.first);
  return keys;
}

std::vector<LtSlot> present_slots(const LtShape& lv, size_t n, const std::vector<int>& keys) {
  std::vector<LtSlot> out;
  for (int u = 0; u < lv.D; ++u) {
    const long off = static_cast<long>(u - lv.center) * lv.stride;
    const int key = static_cast<int>(((off % static_cast<long>(n)) + static_cast<long>(n)) % static_cast<long>(n));
    if (!std::binary_search(keys.begin(), keys.end(), key)) continue;
    out.push_back({u, key, static_cast<size_t>((u / lv.g) * lv.g) * lv.stride % n});
  }
  return out;
}

DiagMap finish_map(DiagMap T, size_t ns, size_t n, std::complex<double> cf, bool apply_const, int mask, uint32_t dim1,
                   int stride, LtShape& shape) {
  if (apply_const)
    for (auto& kv : T)
      for (auto& x : kv.second) x *= cf;
  // sparse packing (ns < n): the ns-slot maps act on every ns-block of the ring's slots.  The
  // CoeffToSlot output w = c_lo + i c_hi (ns-periodic) is multiplied by 1 on even blocks and -i on
  // odd ones, so w + conj(w) holds [c_lo | c_hi] in 2 ns-periodic real slots; SlotToCoeff reads
  // them as [c_lo | i c_hi], and a final rotation by ns adds the two halves (EvalBootstrap).
  if (ns < n) {
    cvec out_mask(2 * ns, {1.0, 0.0}), in_mask(2 * ns, {1.0, 0.0});
    for (size_t p = ns; p < 2 * ns; ++p) {
      out_mask[p] = {0.0, -1.0};
      in_mask[p] = {0.0, 1.0};
    }
    T = lift_blocks(T, ns, n, mask == phx::kLtMaskOut ? &out_mask : nullptr, mask == phx::kLtMaskIn ? &in_mask : nullptr);
  }
  shape = lt_shape(offsets_of(T), n, dim1, stride);
  return T;
}

std::vector<FinishedDiagonal> finish_host(DiagMap T, size_t ns, size_t n, std::complex<double> cf, bool apply_const,
                                          int mask, uint32_t dim1, int stride, LtShape& shape) {
  T = finish_map(std::move(T), ns, n, cf, apply_const, mask, dim1, stride, shape);
  std::vector<FinishedDiagonal> out;
  for (const LtSlot& sl : present_slots(shape, n, offsets_of(T))) {
    const cvec& diag = T.at(sl.key);
    FinishedDiagonal d;
    d.slot = sl.u;
    d.key = sl.key;
    d.values.resize(n);
    for (size_t p = 0; p < n; ++p) d.values[p] = diag[(p + n - sl.shift) % n];
    out.push_back(std::move(d));
  }
  return out;
}

std::vector<int> finish_rows(const LtShape& lv, size_t ns, size_t n, const std::vector<int>& band_offsets,
                             const std::vector<int>& keys, std::vector<phx::LtFinishRow>& rows) {
  if (!std::is_sorted(band_offsets.begin(), band_offsets.end()) || !std::is_sorted(keys.begin(), keys.end()))
    throw std::invalid_argument("offsets must be sorted");
  if (lv.stride < 1 || lv.g < 1 || lv.D < 0) throw std::invalid_argument("bad level shape");
  rows.clear();
  std::vector<int> slot_of_row;
  for (const LtSlot& sl : present_slots(lv, n, keys)) {
    const int key = sl.key;
    // the band's diagonal a lifts to offset a (entries with r + a < ns) and a - ns (the others)
    const int a = ns == n || static_cast<size_t>(key) < ns ? key : static_cast<int>(static_cast<size_t>(key) + ns - n);
    const auto it = std::lower_bound(band_offsets.begin(), band_offsets.end(), a);
    if (a < 0 || it == band_offsets.end() || *it != a) throw std::invalid_argument("level diagonal without a source in the band");
    phx::LtFinishRow r;
    r.src = static_cast<int32_t>(it - band_offsets.begin());
    r.a = a;
    r.key = key;
    r.sh = static_cast<int32_t>(sl.shift);
    rows.push_back(r);
    slot_of_row.push_back(sl.u);
  }
  return slot_of_row;
}

}  // namespace boot

// ======================================================================================
// FHECKKSRNS: one direction's levels, and the dense transform's
// ======================================================================================

void FHECKKSRNS::build_levels(const PhantomContext& cc, bool encode_dir, const LevelArgs& args, uint32_t slots,
                              std::vector<LTLevel>& out, bool encode) const {
  const size_t n = cc.poly_degree() / 2;  // slots of the ring
  const size_t ns = slots;                // slots of the (sub)problem: n = full packing
  const std::complex<double> cf =
      args.times_i ? std::complex<double>(0.0, args.constant) : std::complex<double>(args.constant, 0.0);
  out.clear();
  for (const boot::LevelSpec& spec : boot::plan_levels(ns, n, args.sizes, encode_dir)) {
    const boot::StagePlan plan = boot::plan_stages(ns, spec.stages);
    LTLevel lv;
    lv.chain = args.first_chain + out.size();
    if (encode && device_setup_) {
      device_level(cc, plan, encode_dir, spec, cf, args.dim1, lv);
    } else {
      const boot::DiagMap T = boot::finish_map(boot::stage_products_host(plan, encode_dir), ns, n, cf, spec.apply_const,
                                               spec.mask, args.dim1, spec.stride, lv);
      if (encode) encode_level(cc, lv, T);
    }
    out.push_back(std::move(lv));
  }
}

void FHECKKSRNS::encode_level(const PhantomContext& cc, LTLevel& lv, const boot::DiagMap& T) const {
  const size_t n = cc.poly_degree() / 2;
  const double scale = sf_.at(lv.chain - 1);
  lv.pts.clear();
  lv.pts.resize(lv.D);
  // the level's diagonals: their host encodings (FFT + exact RNS rounding) run on host threads,
  // a chunk at a time, each chunk's uploads + NTTs queued on the stream behind it
  const std::vector<boot::LtSlot> jobs = boot::present_slots(lv, n, boot::offsets_of(T));
  const unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  std::vector<std::vector<uint64_t>> host(nt);
  for (size_t c0 = 0; c0 < jobs.size(); c0 += nt) {
    const size_t cnt = std::min<size_t>(nt, jobs.size() - c0);
    auto work = [&](size_t w) {
      const boot::cvec& diag = T.at(jobs[c0 + w].key);
      const size_t sh = jobs[c0 + w].shift;
      boot::cvec rot(n);
      for (size_t p = 0; p < n; ++p) rot[p] = diag[(p + n - sh) % n];
      encoder_.encode_ext_host(cc, rot, scale, lv.chain, host[w], 1);
    };
    std::vector<std::thread> th;
    for (size_t w = 1; w < cnt; ++w) th.emplace_back(work, w);
    work(0);
    for (auto& t : th) t.join();
    for (size_t w = 0; w < cnt; ++w) {
      auto pt = std::make_unique<PhantomPlaintext>();
      encoder_.upload_ext_async(cc, host[w], scale, *pt, lv.chain);
      lv.pts[jobs[c0 + w].u] = std::move(pt);
    }
    PHX_CHECK(hipStreamSynchronize(cc.stream()));  // host[] is rewritten by the next chunk
  }
  std::vector<std::shared_ptr<PhantomPlaintext>> view;  // (attach reads the pointers only)
  attach(cc, lv, view);
}

// the device pointer table [b][g] of a level's plaintexts (lv.pts when `ext` is empty, else the
// caller's set); absent diagonals read a zero plaintext
void FHECKKSRNS::attach(const PhantomContext& cc, LTLevel& lv,
                        const std::vector<std::shared_ptr<PhantomPlaintext>>& ext) const {
  std::vector<const uint64_t*> ptrs(static_cast<size_t>(lv.b) * lv.g, nullptr);
  for (size_t u = 0; u < ptrs.size(); ++u) {
    const PhantomPlaintext* p = nullptr;
    if (u < static_cast<size_t>(lv.D)) p = ext.empty() ? lv.pts[u].get() : ext[u].get();
    if (p) {
      ptrs[u] = p->data();
      continue;
    }
    if (!lv.zero) {
      const size_t limbs = cc.get_context_data(lv.chain).coeff_modulus_size() + cc.size_P();
      lv.zero.allocate(limbs * cc.poly_degree(), cc.stream());
      PHX_CHECK(hipMemsetAsync(lv.zero.get(), 0, limbs * cc.poly_degree() * sizeof(uint64_t), cc.stream()));
    }
    ptrs[u] = lv.zero.get();
  }
  lv.d_pts.upload(ptrs, cc.stream());
}

// ---- device setup (UseDeviceSetup): csrc/ltprep.h builds the diagonals, the batched device encoder
// the plaintexts.  Per level the host waits for the stream twice at most: for the presence flags
// (sparse packing and dense matrices only) and, at the end, in attach's table upload.

namespace {
// page-locked host words for a level's small tables and read-backs: their copies are asynchronous
// for certain, and the words stay alive until the level's final synchronisation
struct PinnedWords {
  int32_t* p = nullptr;
  explicit PinnedWords(size_t words) {
    PHX_CHECK(hipHostMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(words, 1) * sizeof(int32_t), hipHostMallocDefault));
  }
  ~PinnedWords() {
    if (p) (void)hipHostFree(p);
  }
  PinnedWords(const PinnedWords&) = delete;
  PinnedWords& operator=(const PinnedWords&) = delete;
};

void ltprep_ok(hipError_t e, const char* what) {
  if (e == hipErrorInvalidValue) throw std::invalid_argument(std::string(what) + ": unsupported shape");
  if (e != hipSuccess) throw hip_error(e, what);
}
}  // namespace

void FHECKKSRNS::encode_level_device(const PhantomContext& cc, LTLevel& lv, const void* band, size_t ns,
                                     const std::vector<int>& band_offsets, const std::vector<int>& keys,
                                     std::complex<double> cf, bool apply_const, int mask) const {
  const size_t n = cc.poly_degree() / 2;
  const double scale = sf_.at(lv.chain - 1);
  hipStream_t s = cc.stream();
  lv.pts.clear();
  lv.pts.resize(lv.D);
  std::vector<phx::LtFinishRow> rows;
  const std::vector<int> slot_of_row = boot::finish_rows(lv, ns, n, band_offsets, keys, rows);
  const size_t K = rows.size();
  std::vector<std::shared_ptr<PhantomPlaintext>> view;  // (attach reads the pointers only)
  if (K == 0) {
    attach(cc, lv, view);
    return;
  }
  static_assert(sizeof(phx::LtFinishRow) == 4 * sizeof(int32_t), "rows travel as words");
  PinnedWords pin(4 * K + 1);
  DeviceBuffer<int32_t> tab(4 * K + 1, s);
  std::memcpy(pin.p, rows.data(), K * sizeof(phx::LtFinishRow));
  pin.p[4 * K] = 0;  // the encoder's overflow flag
  PHX_CHECK(hipMemcpyAsync(tab.get(), pin.p, (4 * K + 1) * sizeof(int32_t), hipMemcpyHostToDevice, s));
  DeviceBuffer<double2> batch(K * n, s);
  ltprep_ok(phx::ltprep_finish(static_cast<const double2*>(band), ns, n,
                               reinterpret_cast<const phx::LtFinishRow*>(tab.get()), static_cast<int>(K),
                               make_double2(cf.real(), cf.imag()), apply_const, mask, batch.get(), s),
            "level finish");
  const phx::LimbMap map = encode_limb_map(cc, lv.chain, true);
  std::vector<uint64_t*> ptrs(K);
  for (size_t k = 0; k < K; ++k) {
    auto pt = std::make_unique<PhantomPlaintext>();
    pt->resize_ext(cc, lv.chain, static_cast<size_t>(map.num_limbs), s);
    pt->set_scale(scale);
    ptrs[k] = pt->data();
    lv.pts[slot_of_row[k]] = std::move(pt);
  }
  int* overflow = reinterpret_cast<int*>(tab.get() + 4 * K);
  encode_raw(cc, lv.chain, true, reinterpret_cast<const std::complex<double>*>(batch.get()), n, 0, scale, K, nullptr,
             ptrs.data(), overflow, s);
  PHX_CHECK(hipMemcpyAsync(pin.p + 4 * K, overflow, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  attach(cc, lv, view);  // its table upload waits for the stream: the level's final synchronisation
  if (pin.p[4 * K]) throw std::invalid_argument("encoded values are too large");
}

void FHECKKSRNS::device_level(const PhantomContext& cc, const boot::StagePlan& plan, bool inverse,
                              const boot::LevelSpec& spec, std::complex<double> cf, uint32_t dim1, LTLevel& lv) const {
  const size_t n = cc.poly_degree() / 2, ns = plan.ns;
  hipStream_t s = cc.stream();
  const std::vector<int>& offsets = plan.offsets();
  const size_t D = offsets.size(), nsrc = plan.src.size();
  // tables: the stages' source rows, the band's offsets, its presence flags
  PinnedWords pin(nsrc + 3 * D);
  DeviceBuffer<int32_t> tab(nsrc + 3 * D, s);
  std::memcpy(pin.p, plan.src.data(), nsrc * sizeof(int32_t));
  std::memcpy(pin.p + nsrc, offsets.data(), D * sizeof(int32_t));
  PHX_CHECK(hipMemcpyAsync(tab.get(), pin.p, (nsrc + D) * sizeof(int32_t), hipMemcpyHostToDevice, s));
  DeviceBuffer<double2> buf_a(plan.max_diagonals() * ns, s), buf_b(plan.max_diagonals() * ns, s);
  const void* band = boot::stage_products_device(cc, plan, inverse, tab.get(), buf_a.get(), buf_b.get(), s);
  (band == buf_a.get() ? buf_b : buf_a).release();
  std::vector<int> keys = offsets;  // full packing: compose never drops a key
  if (ns < n) {
    // the lift keeps an offset only where it has a non-zero entry
    int* flags = reinterpret_cast<int*>(tab.get() + nsrc + D);
    PHX_CHECK(hipMemsetAsync(flags, 0, 2 * D * sizeof(int), s));
    ltprep_ok(phx::ltprep_presence(static_cast<const double2*>(band), ns, tab.get() + nsrc, static_cast<int>(D),
                                   make_double2(cf.real(), cf.imag()), spec.apply_const, flags, s),
              "level presence");
    PHX_CHECK(hipMemcpyAsync(pin.p + nsrc + D, flags, 2 * D * sizeof(int), hipMemcpyDeviceToHost, s));
    PHX_CHECK(hipStreamSynchronize(s));
    keys = boot::lifted_keys(offsets, std::vector<int>(pin.p + nsrc + D, pin.p + nsrc + 3 * D), ns, n);
  }
  static_cast<boot::LtShape&>(lv) = boot::lt_shape(keys, n, dim1, spec.stride);
  encode_level_device(cc, lv, band, ns, offsets, keys, cf, spec.apply_const, spec.mask);
}

// the dense transform's level: every diagonal offset 0 .. slots-1 (stride 1)
static uint32_t dense_g(uint32_t slots, uint32_t dim) {
  if (dim) return dim;
  uint32_t g = 1;
  while (g * g < slots && g < static_cast<uint32_t>(phx::kLtMaxG)) g *= 2;
  return g;
}

std::vector<int32_t> FHECKKSRNS::FindLinearTransformRotationIndices(uint32_t slots, uint32_t M, uint32_t dim) const {
  if (slots == 0 || slots > M / 4) throw std::invalid_argument("FindLinearTransformRotationIndices: bad slot count");
  const uint32_t g = dense_g(slots, dim), b = (slots + g - 1) / g;
  std::vector<int32_t> r;
  for (uint32_t j = 1; j < g; ++j) r.push_back(static_cast<int32_t>(j % slots));
  for (uint32_t i = 1; i < b; ++i) r.push_back(static_cast<int32_t>((g * i) % slots));
  std::sort(r.begin(), r.end());
  r.erase(std::unique(r.begin(), r.end()), r.end());
  r.erase(std::remove(r.begin(), r.end(), 0), r.end());
  return r;
}

FHECKKSRNS::LTLevel FHECKKSRNS::dense_level(const PhantomContext& cc, uint32_t L) {
  LTLevel lv;
  lv.stride = 1;
  lv.center = 0;
  lv.D = static_cast<int>(cc.poly_degree() / 2);
  lv.g = static_cast<int>(dense_g(static_cast<uint32_t>(lv.D), 0));
  lv.b = (lv.D + lv.g - 1) / lv.g;
  if (lv.g > phx::kLtMaxG || lv.b > phx::kLtMaxB)
    throw std::invalid_argument("EvalLinearTransformPrecompute: more diagonals than one level evaluates (N <= 2^12)");
  lv.chain = 1 + L;
  if (lv.chain >= cc.total_parm_size()) throw std::invalid_argument("EvalLinearTransformPrecompute: L beyond the chain");
  return lv;
}

std::vector<std::shared_ptr<PhantomPlaintext>> FHECKKSRNS::share_plaintexts(LTLevel& lv) {
  return {std::make_move_iterator(lv.pts.begin()), std::make_move_iterator(lv.pts.end())};
}

std::vector<std::shared_ptr<PhantomPlaintext>> FHECKKSRNS::EvalLinearTransformPrecompute(
    const PhantomContext& cc, const std::vector<std::vector<std::complex<double>>>& A, double scale, uint32_t L) const {
  const size_t n = cc.poly_degree() / 2, slots = A.size();
  if (slots != n) throw std::invalid_argument("EvalLinearTransformPrecompute: A must be (N/2) x (N/2) (full packing)");
  for (const auto& row : A)
    if (row.size() != slots) throw std::invalid_argument("EvalLinearTransformPrecompute: A is not square");
  if (device_setup_) {
    // the matrix goes to the device once; its diagonals are cut there
    std::vector<std::complex<double>> flat(slots * slots);
    for (size_t p = 0; p < slots; ++p) std::copy(A[p].begin(), A[p].end(), flat.begin() + p * slots);
    DeviceBuffer<std::complex<double>> dA;
    dA.upload(flat, cc.stream());
    return dense_precompute_device(cc, dA.get(), scale, L);
  }
  // diagonal k: d_k[p] = A[p][(p + k) mod slots] (ExtractShiftedDiagonal, util.cu:298-312)
  boot::DiagMap T;
  for (size_t k = 0; k < slots; ++k) {
    boot::cvec d(slots);
    bool nz = false;
    for (size_t p = 0; p < slots; ++p) {
      d[p] = A[p][(p + k) % slots] * scale;
      nz |= d[p] != std::complex<double>(0.0, 0.0);
    }
    if (nz) T.emplace(static_cast<int>(k), std::move(d));
  }
  LTLevel lv = dense_level(cc, L);
  encode_level(cc, lv, T);
  return share_plaintexts(lv);
}

std::vector<std::shared_ptr<PhantomPlaintext>> FHECKKSRNS::EvalLinearTransformPrecompute(
    const PhantomContext& cc, const std::complex<double>* dev_A, double scale, uint32_t L) const {
  if (!dev_A) throw std::invalid_argument("EvalLinearTransformPrecompute: null matrix");
  return dense_precompute_device(cc, dev_A, scale, L);
}

std::vector<std::shared_ptr<PhantomPlaintext>> FHECKKSRNS::dense_precompute_device(const PhantomContext& cc,
                                                                                   const std::complex<double>* dev_A,
                                                                                   double scale, uint32_t L) const {
  const size_t n = cc.poly_degree() / 2;
  hipStream_t s = cc.stream();
  LTLevel lv = dense_level(cc, L);
  // diagonal k: d_k[p] = A[p][(p + k) mod slots] * scale, and whether it has a non-zero entry
  DeviceBuffer<double2> band(n * n, s);
  DeviceBuffer<int> flags(n, s);
  PinnedWords pin(n);
  PHX_CHECK(hipMemsetAsync(flags.get(), 0, n * sizeof(int), s));
  ltprep_ok(phx::ltprep_dense(reinterpret_cast<const double2*>(dev_A), n, scale, band.get(), flags.get(), s),
            "dense diagonals");
  PHX_CHECK(hipMemcpyAsync(pin.p, flags.get(), n * sizeof(int), hipMemcpyDeviceToHost, s));
  PHX_CHECK(hipStreamSynchronize(s));
  std::vector<int> offsets(n), keys;
  for (size_t k = 0; k < n; ++k) {
    offsets[k] = static_cast<int>(k);
    if (pin.p[k]) keys.push_back(static_cast<int>(k));
  }
  encode_level_device(cc, lv, band.get(), n, offsets, keys, {1.0, 0.0}, false, phx::kLtMaskNone);
  return share_plaintexts(lv);
}

std::vector<std::shared_ptr<PhantomPlaintext>> FHECKKSRNS::EvalLinearTransformPrecompute(
    const PhantomContext&, const std::vector<std::vector<std::complex<double>>>&,
    const std::vector<std::vector<std::complex<double>>>&, uint32_t, double, uint32_t) const {
  throw std::logic_error(
      "EvalLinearTransformPrecompute(A, B, orientation): the reference declares it (include/bootstrap.cuh:133-136) "
      "but defines no body; sparse packing runs through EvalCoeffsToSlots / EvalSlotsToCoeffs instead");
}

}  // namespace phantom
