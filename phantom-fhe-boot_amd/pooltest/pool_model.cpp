// pool_model.cpp — CPU model test of phantom::DevicePool (host/buffer.cpp, compiled unchanged
// against the fake HIP runtime of fake_hip.cpp; no device, no HIP library).
//
//   pool_model random SEED STEPS    random allocations, frees, retags, stream advances, stream
//                                   creation and teardown; after every step: no two live blocks
//                                   overlap, the pool's statistics equal the model's, and the
//                                   ordering invariant below
//   pool_model threads SEED STEPS   4 threads, one stream each, hipMalloc of a chunk sleeping 1 ms
//                                   (the window in which grow() has released the pool's mutex)
//   pool_model scenario NAME        coalesce | slack | ladder | small | forget
//   pool_model doublefree [small]   frees a block twice: must end by abort()
//
// Ordering invariant: when alloc() returns a range for stream s, every earlier use of any byte
// of it whose last toucher was another stream has completed, or s has a happens-before edge past
// it (a hipStreamWaitEvent on an event recorded after that use, directly or through other
// streams).  Past uses live in an interval map that is split at a new block's bounds, so the
// parts of an old range outside the new block keep their history.
// Each mode prints one JSON line and exits 0 only if nothing was violated.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "../host/buffer.h"
#include "fake_hip.h"

using phantom::DevicePool;

namespace {

constexpr size_t KiB = size_t(1) << 10, MiB = size_t(1) << 20, GiB = size_t(1) << 30;

std::atomic<uint64_t> g_failures{0};
void fail(const char* fmt, ...) {
  if (g_failures.fetch_add(1) >= 10) return;
  va_list ap;
  va_start(ap, fmt);
  std::fprintf(stderr, "pool_model: ");
  std::vfprintf(stderr, fmt, ap);
  std::fprintf(stderr, "\n");
  va_end(ap);
}
#define EXPECT(cond, ...) \
  do {                    \
    if (!(cond)) fail(__VA_ARGS__); \
  } while (0)

// the size the pool accounts for a request (buffer.cpp: kGrain multiples from kArenaMin, powers of two below)
size_t rounded(size_t bytes) {
  if (bytes >= DevicePool::kArenaMin) return (bytes + DevicePool::kGrain - 1) / DevicePool::kGrain * DevicePool::kGrain;
  size_t c = 512;
  while (c < bytes) c <<= 1;
  return c;
}

// pools are never destroyed (DevicePool has no destructor that returns its chunks); keeping them
// reachable keeps the leak checker quiet
std::vector<DevicePool*>& g_pools = *new std::vector<DevicePool*>();
DevicePool& new_pool() {
  g_pools.push_back(new DevicePool());
  return *g_pools.back();
}

struct Buf {
  void* p = nullptr;
  size_t bytes = 0, size = 0;  // requested / rounded
  hipStream_t tag = nullptr;   // the stream it is freed on
};

// The test's picture of one pool: live blocks, the last use of every range handed out before,
// and the statistics the pool must report.
class Model {
 public:
  explicit Model(DevicePool& pool) : pool_(pool) { (void)hipEventCreateWithFlags(&ev_, 0); }

  uint64_t allocs = 0, cross_reuses = 0, incomplete_reuses = 0, violations = 0;

  // nullptr when the pool threw (the code is kept in last_error)
  void* alloc(size_t bytes, hipStream_t s, Buf* out = nullptr) {
    void* p = nullptr;
    try {
      p = pool_.alloc(bytes, s);
    } catch (const phantom::hip_error& e) {
      last_error = e.code;
      check_stats();
      return nullptr;
    }
    ++allocs;
    const size_t sz = rounded(bytes);
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    EXPECT(p && fake::inside_allocation(p, sz), "alloc(%zu) returned %p, not inside a hipMalloc'ed range", bytes, p);
    auto nx = live_.upper_bound(a);
    EXPECT(nx == live_.end() || nx->first >= a + sz, "block %p+%zu overlaps the live block at %#zx", p, sz,
           nx == live_.end() ? size_t(0) : size_t(nx->first));
    if (nx != live_.begin()) {
      auto pv = std::prev(nx);
      EXPECT(pv->second <= a, "block %p+%zu overlaps the live block at %#zx", p, sz, size_t(pv->first));
    }
    check_order(a, sz, s);
    live_[a] = a + sz;
    live_bytes_ += sz;
    fake::enqueue_work(s);
    if (out) *out = Buf{p, bytes, sz, s};
    check_stats();
    return p;
  }

  // one more piece of work on the buffer's stream, then the free on that stream
  void free(const Buf& b) {
    const uint64_t pos = fake::enqueue_work(b.tag);
    const uint64_t uid = fake::uid(b.tag);
    pool_.free(b.p, b.bytes, b.tag);
    retire(b, uid, pos);
  }
  // the caller synchronises the device, then frees with completed = true (DeviceBuffer::release_sync)
  void free_completed(const Buf& b) {
    fake::enqueue_work(b.tag);
    (void)hipDeviceSynchronize();
    pool_.free(b.p, b.bytes, nullptr, true);
    retire(b, 0, 0);
  }
  // hands the buffer to stream t behind a wait (DeviceBuffer::set_stream, PhantomCiphertext::retag)
  void retag(Buf& b, hipStream_t t) {
    if (t == b.tag) return;
    fake::enqueue_work(b.tag);
    (void)hipEventRecord(ev_, b.tag);
    (void)hipStreamWaitEvent(t, ev_, 0);
    fake::enqueue_work(t);
    b.tag = t;
  }

  void check_stats() {
    const DevicePool::Stats st = pool_.stats();
    EXPECT(st.live == live_bytes_, "stats().live = %zu, the model has %zu", st.live, live_bytes_);
    EXPECT(st.held == fake::outstanding(), "stats().held = %zu, the runtime has %zu outstanding", st.held,
           fake::outstanding());
    EXPECT(st.peak_live >= st.live && st.peak_held >= st.held, "a peak below the current value");
    EXPECT(st.peak_live >= peak_live_ && st.peak_held >= peak_held_, "a peak decreased without a reset");
    peak_live_ = st.peak_live;
    peak_held_ = st.peak_held;
  }
  void reset_peak() {
    pool_.reset_peak();
    const DevicePool::Stats st = pool_.stats();
    EXPECT(st.peak_live == st.live && st.peak_held == st.held, "reset_peak() did not reset the peaks");
    peak_live_ = st.peak_live;
    peak_held_ = st.peak_held;
  }
  size_t live_bytes() const { return live_bytes_; }
  hipError_t last_error = hipSuccess;

 private:
  struct Piece {
    uintptr_t end;
    uint64_t uid, pos;  // the last use: position `pos` of stream `uid` (pos 0: known complete)
  };
  void split(uintptr_t x) {
    auto it = past_.upper_bound(x);
    if (it == past_.begin()) return;
    --it;
    if (it->first < x && x < it->second.end) {
      Piece right = it->second;
      it->second.end = x;
      past_[x] = right;
    }
  }
  void check_order(uintptr_t a, size_t sz, hipStream_t s) {
    split(a);
    split(a + sz);
    const uint64_t me = fake::uid(s);
    bool cross = false, incomplete = false;
    auto it = past_.lower_bound(a);
    while (it != past_.end() && it->first < a + sz) {
      const Piece& pc = it->second;
      if (pc.pos && pc.uid != me) {
        cross = true;
        if (!fake::completed(pc.uid, pc.pos)) {
          incomplete = true;
          if (!fake::ordered_before(s, pc.uid, pc.pos)) {
            ++violations;
            fail("ordering: [%#zx, %#zx) handed to stream %llu while its use at %llu:%llu is incomplete and unordered",
                 size_t(it->first), size_t(pc.end), (unsigned long long)me, (unsigned long long)pc.uid,
                 (unsigned long long)pc.pos);
          }
        }
      }
      it = past_.erase(it);
    }
    cross_reuses += cross;
    incomplete_reuses += incomplete;
  }
  void retire(const Buf& b, uint64_t uid, uint64_t pos) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(b.p);
    EXPECT(live_.erase(a) == 1, "the test freed a block it does not hold");
    live_bytes_ -= b.size;
    past_[a] = Piece{a + b.size, uid, pos};
    check_stats();
  }

  DevicePool& pool_;
  hipEvent_t ev_ = nullptr;
  std::map<uintptr_t, uintptr_t> live_;  // start -> end
  std::map<uintptr_t, Piece> past_;      // start -> last use, disjoint
  size_t live_bytes_ = 0, peak_live_ = 0, peak_held_ = 0;
};

using Rng = std::mt19937_64;

size_t random_size(Rng& rng) {
  const unsigned cat = rng() % 100;
  if (cat < 40) {  // small path, every class
    const size_t cap = size_t(1) << (1 + rng() % 20);
    return std::min<size_t>(1 + rng() % cap, MiB - 1);
  }
  if (cat < 75) return MiB + rng() % (63 * MiB);                 // arena, any byte count
  if (cat < 90) return (1 + rng() % 64) * MiB;                   // exact multiples of 1 MiB
  if (cat < 98) return (100 + rng() % 300) * MiB + rng() % 4096;  // a few hundred MiB
  return DevicePool::kChunk + 1 + rng() % (256 * MiB);           // a chunk of its own
}

int finish(const char* mode, const std::string& body) {
  const fake::Counters c = fake::counters();
  EXPECT(c.errors == 0, "%llu misuses of the runtime", (unsigned long long)c.errors);
  const bool ok = g_failures.load() == 0;
  std::printf("{\"mode\": \"%s\", %s, \"failures\": %llu, \"runtime_errors\": %llu, \"ok\": %s}\n", mode, body.c_str(),
              (unsigned long long)g_failures.load(), (unsigned long long)c.errors, ok ? "true" : "false");
  return ok ? 0 : 1;
}

std::string kv(const char* k, uint64_t v) { return std::string("\"") + k + "\": " + std::to_string(v); }

// ---------------------------------------------------------------------------------------------
// random driver
int run_random(uint64_t seed, uint64_t steps) {
  constexpr size_t kLiveLimit = 2 * GiB, kLiveCount = 384;
  fake::reset(64 * GiB);  // far above the live set: only the ladder scenario runs out of memory
  DevicePool& pool = DevicePool::instance();
  Model m(pool);
  Rng rng(seed);
  std::vector<hipStream_t> streams{nullptr};
  for (int i = 0; i < 3; ++i) {
    hipStream_t s;
    (void)hipStreamCreate(&s);
    streams.push_back(s);
  }
  std::vector<Buf> live;
  uint64_t retags = 0, completed_frees = 0, created = 3, destroyed = 0, peak_held = 0;

  auto free_at = [&](size_t i) {
    Buf b = live[i];
    live[i] = live.back();
    live.pop_back();
    const unsigned how = rng() % 1000;
    if (how < 3) {
      ++completed_frees;
      m.free_completed(b);
      return;
    }
    if (how < 160) {
      ++retags;
      m.retag(b, streams[rng() % streams.size()]);
    }
    m.free(b);
  };

  for (uint64_t step = 0; step < steps; ++step) {
    const unsigned r = rng() % 1000;
    if (r < 400) {
      const size_t bytes = random_size(rng);
      if (live.size() >= kLiveCount || m.live_bytes() + rounded(bytes) > kLiveLimit) {
        if (!live.empty()) free_at(rng() % live.size());
        continue;
      }
      Buf b;
      if (m.alloc(bytes, streams[rng() % streams.size()], &b))
        live.push_back(b);
      else
        fail("step %llu: alloc(%zu) threw (%s)", (unsigned long long)step, bytes, hipGetErrorString(m.last_error));
    } else if (r < 780) {
      if (!live.empty()) free_at(rng() % live.size());
    } else if (r < 995) {
      fake::advance(streams[rng() % streams.size()], 1 + rng() % 3);
    } else if (r < 997) {
      (void)hipStreamSynchronize(streams[rng() % streams.size()]);
    } else if (r < 998) {
      m.reset_peak();
    } else if (streams.size() < 7 && (streams.size() < 3 || rng() % 2)) {
      hipStream_t s;
      (void)hipStreamCreate(&s);
      streams.push_back(s);
      ++created;
    } else if (streams.size() > 2) {
      // OwnedStream's teardown: whatever is still tagged with the stream is freed on it or handed
      // to another stream first; then synchronise, forget_stream, destroy
      const size_t k = 1 + rng() % (streams.size() - 1);
      hipStream_t s = streams[k];
      streams.erase(streams.begin() + static_cast<long>(k));
      for (size_t i = live.size(); i-- > 0;) {
        if (live[i].tag != s) continue;
        if (rng() % 2) {
          m.retag(live[i], streams[rng() % streams.size()]);
        } else {
          m.free(live[i]);
          live[i] = live.back();
          live.pop_back();
        }
      }
      (void)hipStreamSynchronize(s);
      pool.forget_stream(s);
      (void)hipStreamDestroy(s);
      ++destroyed;
    }
    m.check_stats();
    peak_held = std::max<uint64_t>(peak_held, pool.stats().held);
  }
  const fake::Counters c = fake::counters();
  return finish("random", kv("seed", seed) + ", " + kv("steps", steps) + ", " + kv("allocs", m.allocs) + ", " +
                              kv("cross_stream_reuses", m.cross_reuses) + ", " +
                              kv("incomplete_cross_stream_reuses", m.incomplete_reuses) + ", " +
                              kv("violations", m.violations) + ", " + kv("retags", retags) + ", " +
                              kv("completed_frees", completed_frees) + ", " + kv("streams_created", created) + ", " +
                              kv("streams_destroyed", destroyed) + ", " + kv("stream_waits", c.stream_waits) + ", " +
                              kv("malloc_failures", c.malloc_failures) + ", " + kv("peak_held_MiB", peak_held >> 20));
}

// ---------------------------------------------------------------------------------------------
// threads
class Barrier {
 public:
  explicit Barrier(unsigned n) : n_(n) {}
  void wait() {
    std::unique_lock<std::mutex> lk(mu_);
    const uint64_t gen = gen_;
    if (++count_ == n_) {
      count_ = 0;
      ++gen_;
      cv_.notify_all();
    } else {
      cv_.wait(lk, [&] { return gen_ != gen; });
    }
  }

 private:
  std::mutex mu_;
  std::condition_variable cv_;
  unsigned n_, count_ = 0;
  uint64_t gen_ = 0;
};

int run_threads(uint64_t seed, uint64_t steps) {
  constexpr unsigned kThreads = 4;
  constexpr size_t kLiveLimit = 768 * MiB;  // per thread
  constexpr uint64_t kCheckEvery = 1000;
  fake::reset(64 * GiB);
  fake::set_malloc_sleep_us(1000, DevicePool::kChunk);
  DevicePool& pool = DevicePool::instance();
  std::mutex reg_mu;
  std::map<uintptr_t, uintptr_t> registry;  // live ranges of all threads
  size_t reg_bytes = 0;
  std::atomic<uint64_t> allocs{0};
  Barrier barrier(kThreads);
  hipStream_t streams[kThreads];
  for (auto& s : streams) (void)hipStreamCreate(&s);

  auto worker = [&](unsigned t) {
    Rng rng(seed * 1000003 + t);
    hipStream_t s = streams[t];
    std::vector<Buf> live;
    size_t live_bytes = 0;
    auto release = [&](size_t i) {
      const Buf b = live[i];
      live[i] = live.back();
      live.pop_back();
      live_bytes -= b.size;
      fake::enqueue_work(s);
      {  // out of the registry before the pool may hand the range to another thread
        std::lock_guard<std::mutex> lk(reg_mu);
        EXPECT(registry.erase(reinterpret_cast<uintptr_t>(b.p)) == 1, "thread %u frees a block not registered", t);
        reg_bytes -= b.size;
      }
      pool.free(b.p, b.bytes, s);
    };
    for (uint64_t step = 0; step < steps; ++step) {
      if (step % kCheckEvery == 0) {  // everyone is between two pool calls: the statistics are exact
        barrier.wait();
        if (t == 0) {
          const DevicePool::Stats st = pool.stats();
          std::lock_guard<std::mutex> lk(reg_mu);
          EXPECT(st.live == reg_bytes, "stats().live = %zu, the threads hold %zu", st.live, reg_bytes);
          EXPECT(st.held == fake::outstanding(), "stats().held = %zu, the runtime has %zu outstanding", st.held,
                 fake::outstanding());
          EXPECT(st.peak_live >= st.live && st.peak_held >= st.held, "a peak below the current value");
        }
        barrier.wait();
      }
      const unsigned r = rng() % 100;
      if (r < 40) {
        const size_t bytes = random_size(rng), sz = rounded(bytes);
        if (live_bytes + sz > kLiveLimit && !(live.empty())) {
          release(rng() % live.size());
          continue;
        }
        void* p = nullptr;
        try {
          p = pool.alloc(bytes, s);
        } catch (const phantom::hip_error& e) {
          fail("thread %u: alloc(%zu) threw: %s", t, bytes, e.what());
          continue;
        }
        allocs.fetch_add(1);
        const uintptr_t a = reinterpret_cast<uintptr_t>(p);
        EXPECT(fake::inside_allocation(p, sz), "thread %u: %p+%zu is not inside a hipMalloc'ed range", t, p, sz);
        {
          std::lock_guard<std::mutex> lk(reg_mu);
          auto nx = registry.upper_bound(a);
          EXPECT(nx == registry.end() || nx->first >= a + sz, "thread %u: %p+%zu overlaps a live block", t, p, sz);
          if (nx != registry.begin()) EXPECT(std::prev(nx)->second <= a, "thread %u: %p+%zu overlaps a live block", t, p, sz);
          registry[a] = a + sz;
          reg_bytes += sz;
        }
        fake::enqueue_work(s);
        live.push_back(Buf{p, bytes, sz, s});
        live_bytes += sz;
      } else if (r < 75) {
        if (!live.empty()) release(rng() % live.size());
      } else if (r < 99) {
        fake::advance(s, 1 + rng() % 6);
      } else {
        (void)hipStreamSynchronize(s);
      }
    }
    while (!live.empty()) release(live.size() - 1);
  };
  std::vector<std::thread> th;
  for (unsigned t = 0; t < kThreads; ++t) th.emplace_back(worker, t);
  for (auto& x : th) x.join();
  const DevicePool::Stats st = pool.stats();
  EXPECT(st.live == 0 && registry.empty(), "stats().live = %zu after every thread freed everything", st.live);
  EXPECT(st.held == fake::outstanding(), "stats().held = %zu, the runtime has %zu outstanding", st.held,
         fake::outstanding());
  const fake::Counters c = fake::counters();
  return finish("threads", kv("seed", seed) + ", " + kv("steps", steps) + ", " + kv("threads", kThreads) + ", " +
                               kv("allocs", allocs.load()) + ", " + kv("mallocs", c.mallocs) + ", " +
                               kv("stream_waits", c.stream_waits) + ", " + kv("peak_held_MiB", st.peak_held >> 20));
}

// ---------------------------------------------------------------------------------------------
// scenarios
hipStream_t make_stream() {
  hipStream_t s;
  (void)hipStreamCreate(&s);
  return s;
}

// A chunk filled with blocks that are freed in scrambled order on three streams coalesces back
// into one block: a request of the chunk's size is served without growing.
int scenario_coalesce() {
  fake::reset(64 * GiB);
  DevicePool& pool = new_pool();
  Model m(pool);
  hipStream_t st[3] = {make_stream(), make_stream(), nullptr};
  // 1 GiB = 8 x 64 MiB + 4 x 96 MiB + 127 MiB + 1 MiB  (in 64 KiB grains, not all equal)
  std::vector<size_t> sizes;
  for (int i = 0; i < 8; ++i) sizes.push_back(64 * MiB);
  for (int i = 0; i < 4; ++i) sizes.push_back(96 * MiB);
  sizes.push_back(127 * MiB - 3 * 64 * KiB);
  sizes.push_back(MiB + 3 * 64 * KiB - 5);  // rounds up to 1 MiB + 3 grains
  std::vector<Buf> bufs(sizes.size());
  for (size_t i = 0; i < sizes.size(); ++i) EXPECT(m.alloc(sizes[i], st[i % 3], &bufs[i]), "alloc %zu failed", i);
  const size_t held = pool.stats().held;
  EXPECT(held == DevicePool::kChunk && pool.stats().live == DevicePool::kChunk, "the blocks do not fill one chunk: held %zu", held);
  Rng rng(7);
  for (size_t i = bufs.size(); i-- > 1;) std::swap(bufs[i], bufs[rng() % (i + 1)]);
  for (const Buf& b : bufs) m.free(b);
  // busy: the free space is one block, but no other stream may have it without a wait or growth
  Buf small;
  EXPECT(m.alloc(64, nullptr, &small), "small alloc failed");  // (records the stamps of the frees)
  (void)hipDeviceSynchronize();
  Buf whole;
  EXPECT(m.alloc(DevicePool::kChunk, st[0], &whole), "alloc of the chunk's size failed");
  EXPECT(pool.stats().held == held + 512, "held %zu -> %zu: the chunk did not coalesce", held, pool.stats().held);
  const fake::Counters c = fake::counters();
  EXPECT(c.mallocs == 2 && c.stream_waits == 0, "mallocs %llu, waits %llu", (unsigned long long)c.mallocs,
         (unsigned long long)c.stream_waits);
  return finish("coalesce", kv("blocks", sizes.size()) + ", " + kv("held", pool.stats().held) + ", " + kv("mallocs", c.mallocs));
}

// Above kSlackMin of cached space, a stream takes another stream's busy block behind a wait;
// at or below it, the pool grows.
int scenario_slack() {
  uint64_t waits_above = 0, waits_below = 0;
  {
    fake::reset(64 * GiB);
    DevicePool& pool = new_pool();
    Model m(pool);
    hipStream_t a = make_stream(), b = make_stream();
    Buf x[3];
    for (Buf& v : x) EXPECT(m.alloc(GiB, a, &v), "alloc failed");
    for (Buf& v : x) m.free(v);  // a never advances: all three stay in use
    const size_t held = pool.stats().held;
    EXPECT(held == 3 * GiB, "held %zu", held);
    Buf y;
    EXPECT(m.alloc(GiB, b, &y), "alloc failed");
    const fake::Counters c = fake::counters();
    waits_above = c.stream_waits;
    EXPECT(pool.stats().held == held && c.mallocs == 3, "3 GiB cached and busy: the pool grew (held %zu)", pool.stats().held);
    EXPECT(c.stream_waits == 1, "%llu waits issued, expected 1", (unsigned long long)c.stream_waits);
    EXPECT(y.p == x[0].p || y.p == x[1].p || y.p == x[2].p, "not one of the cached blocks");
    EXPECT(m.incomplete_reuses == 1 && m.violations == 0, "the reuse was not behind a wait");
    EXPECT(fake::backlog(a) > 0, "stream a finished: nothing shown");
  }
  {
    fake::reset(64 * GiB);
    DevicePool& pool = new_pool();
    Model m(pool);
    hipStream_t a = make_stream(), b = make_stream();
    Buf x[2];
    for (Buf& v : x) EXPECT(m.alloc(GiB, a, &v), "alloc failed");
    for (Buf& v : x) m.free(v);
    Buf y;
    EXPECT(m.alloc(GiB, b, &y), "alloc failed");
    const fake::Counters c = fake::counters();
    waits_below = c.stream_waits;
    EXPECT(pool.stats().held == 3 * GiB && c.mallocs == 3, "2 GiB cached and busy: the pool did not grow (held %zu)", pool.stats().held);
    EXPECT(c.stream_waits == 0, "%llu waits issued, expected none", (unsigned long long)c.stream_waits);
    EXPECT(m.incomplete_reuses == 0 && m.cross_reuses == 0, "a busy block was reused");
    // the same stream takes its own block back at once
    Buf z;
    EXPECT(m.alloc(GiB, a, &z), "alloc failed");
    EXPECT(pool.stats().held == 3 * GiB && (z.p == x[0].p || z.p == x[1].p), "stream a did not get its own block back");
  }
  return finish("slack", kv("waits_above_slack", waits_above) + ", " + kv("waits_below_slack", waits_below));
}

// The out-of-memory ladder of alloc(): release of the cache, the wait-carve, the device
// synchronise, and the thrown error; each counted in the fake runtime.
int scenario_ladder() {
  const size_t cap = 3 * GiB + 768 * MiB;
  fake::reset(cap);
  DevicePool& pool = new_pool();
  Model m(pool);
  hipStream_t a = make_stream(), b = make_stream();
  Buf x1, x2, x3, s1, s2, d0;
  EXPECT(m.alloc(GiB, a, &x1) && m.alloc(GiB, a, &x2) && m.alloc(GiB, a, &x3), "setup failed");
  EXPECT(m.alloc(4096, a, &s1) && m.alloc(4096, b, &s2), "setup failed");
  m.free(x1);
  m.free(s1);
  EXPECT(m.alloc(100, b, &d0), "setup failed");  // records the stamp of the two frees
  (void)hipDeviceSynchronize();                  // x1 and s1: cached, uses completed
  m.free(x2);                                    // x2 and s2: cached, in use (nothing advances from here)
  m.free(s2);
  fake::Counters c0 = fake::counters();
  uint64_t tot_fails = 0, tot_frees = 0, tot_waits = 0, tot_dsyncs = 0;  // by the pool, from here on
  auto delta = [&](const char* rung, uint64_t fails, uint64_t frees, uint64_t waits, uint64_t dsyncs) {
    const fake::Counters c = fake::counters();
    EXPECT(c.malloc_failures - c0.malloc_failures == fails && c.frees - c0.frees == frees &&
               c.stream_waits - c0.stream_waits == waits && c.device_syncs - c0.device_syncs == dsyncs,
           "%s: %llu failed hipMalloc, %llu hipFree, %llu waits, %llu device synchronisations; expected %llu, %llu, %llu, %llu",
           rung, (unsigned long long)(c.malloc_failures - c0.malloc_failures), (unsigned long long)(c.frees - c0.frees),
           (unsigned long long)(c.stream_waits - c0.stream_waits), (unsigned long long)(c.device_syncs - c0.device_syncs),
           (unsigned long long)fails, (unsigned long long)frees, (unsigned long long)waits, (unsigned long long)dsyncs);
    tot_fails += c.malloc_failures - c0.malloc_failures;
    tot_frees += c.frees - c0.frees;
    tot_waits += c.stream_waits - c0.stream_waits;
    tot_dsyncs += c.device_syncs - c0.device_syncs;
    c0 = c;
  };
  // rung 1: growth fails; x1's chunk and s1 go back to the runtime, the busy x2 and s2 stay; growth succeeds
  Buf y;
  EXPECT(m.alloc(GiB + 512 * MiB, b, &y), "rung 1: alloc threw");
  delta("release", 1, 2, 0, 0);
  EXPECT(pool.stats().held == 3 * GiB + 512 * MiB + 4096 + 512, "rung 1: held %zu", pool.stats().held);
  // rung 2: nothing to release, growth fails twice, x2's block is taken behind a wait
  Buf z;
  const size_t held2 = pool.stats().held;
  EXPECT(m.alloc(GiB, b, &z), "rung 2: alloc threw");
  delta("wait-carve", 2, 0, 1, 0);
  EXPECT(z.p == x2.p && pool.stats().held == held2, "rung 2: not x2's block, or held changed");
  EXPECT(m.incomplete_reuses == 1, "rung 2: the block's use had completed");
  // rung 3: no block is large enough even with waits; after the device synchronise the two free
  // chunks and s2 are released and growth succeeds
  m.free(x3);
  m.free(z);
  Buf w;
  EXPECT(m.alloc(2 * GiB, a, &w), "rung 3: alloc threw");
  delta("synchronise", 2, 3, 0, 1);
  EXPECT(pool.stats().held == 3 * GiB + 512 * MiB + 512, "rung 3: held %zu", pool.stats().held);
  // rung 4: nothing left to release
  const DevicePool::Stats before = pool.stats();
  Buf v;
  m.last_error = hipSuccess;
  EXPECT(!m.alloc(3 * GiB, a, &v) && m.last_error == hipErrorOutOfMemory, "rung 4: no hipErrorOutOfMemory");
  delta("throw", 3, 0, 0, 1);
  EXPECT(pool.stats().held == before.held && pool.stats().live == before.live, "rung 4: the failed alloc changed the statistics");
  // the pool still works: y's block (busy on b) is carved for a behind a wait
  m.free(y);
  Buf u;
  EXPECT(m.alloc(GiB, a, &u) && u.p == y.p, "after the throw: alloc failed or not y's block");
  delta("after", 2, 0, 1, 0);
  EXPECT(m.violations == 0, "ordering violated");
  return finish("ladder", kv("malloc_failures", tot_fails) + ", " + kv("released_to_runtime", tot_frees) + ", " +
                              kv("wait_carves", tot_waits) + ", " + kv("device_syncs", tot_dsyncs) + ", " +
                              kv("oom_thrown", m.last_error == hipErrorOutOfMemory));
}

// A small block freed on a busy stream goes to that stream only, until the stream has passed the stamp.
int scenario_small() {
  fake::reset(64 * GiB);
  DevicePool& pool = new_pool();
  Model m(pool);
  hipStream_t a = make_stream(), b = make_stream();
  Buf p, q, r, t, u;
  EXPECT(m.alloc(3000, a, &p), "alloc failed");
  m.free(p);
  EXPECT(m.alloc(4096, b, &q) && q.p != p.p, "a's busy block was handed to b");
  EXPECT(pool.stats().held == 2 * 4096, "held %zu", pool.stats().held);
  EXPECT(m.alloc(2049, a, &r) && r.p == p.p, "a did not get its own block back");
  m.free(r);
  EXPECT(m.alloc(4000, b, &t) && t.p != p.p, "a's busy block was handed to b");  // (records a's stamp)
  EXPECT(fake::backlog(a) > 0, "stream a finished: nothing shown");
  fake::advance(a, fake::backlog(a));
  EXPECT(m.alloc(4096, b, &u) && u.p == p.p, "after a passed the stamp, b did not get the block");
  EXPECT(pool.stats().held == 3 * 4096 && m.violations == 0 && m.cross_reuses == 1 && m.incomplete_reuses == 0,
         "held %zu, %llu cross-stream reuses", pool.stats().held, (unsigned long long)m.cross_reuses);
  return finish("small", kv("held", pool.stats().held));
}

// OwnedStream's teardown: after synchronise + forget_stream + destroy, the stream's cached blocks
// are plain free blocks, no call names the stream again, and a new stream behind the same handle
// value starts afresh.
int scenario_forget() {
  fake::reset(64 * GiB);
  DevicePool& pool = new_pool();
  Model m(pool);
  hipStream_t b = make_stream(), x = make_stream();
  Buf big, sm;
  EXPECT(m.alloc(3 * MiB, x, &big) && m.alloc(700, x, &sm), "alloc failed");
  m.free(big);
  m.free(sm);
  (void)hipStreamSynchronize(x);
  pool.forget_stream(x);
  (void)hipStreamDestroy(x);
  const size_t held = pool.stats().held;
  const uint64_t queries = fake::counters().event_queries;
  Buf big2, sm2;
  EXPECT(m.alloc(3 * MiB, b, &big2) && big2.p == big.p, "the forgotten stream's arena block was not reused");
  EXPECT(m.alloc(1000, b, &sm2) && sm2.p == sm.p, "the forgotten stream's small block was not reused");
  EXPECT(pool.stats().held == held, "held %zu -> %zu", held, pool.stats().held);
  EXPECT(fake::counters().event_queries == queries, "the pool queried an event for a forgotten stream");
  // the handle value comes back as a new stream: its frees are not taken for completed ones
  (void)make_stream();  // (the fake runtime reuses a destroyed handle on every second create)
  hipStream_t x2 = make_stream();
  EXPECT(x2 == x, "the fake runtime did not reuse the handle");
  m.free(big2);  // on b
  Buf big3;
  EXPECT(m.alloc(3 * MiB, x2, &big3), "alloc failed");
  m.free(big3);
  Buf big4;
  EXPECT(m.alloc(3 * MiB, b, &big4), "alloc failed");
  EXPECT(m.violations == 0, "ordering violated");
  return finish("forget", kv("held", pool.stats().held));
}

int run_doublefree(bool small) {
  fake::reset(64 * GiB);
  DevicePool& pool = new_pool();
  const size_t bytes = small ? 4096 : 4 * MiB;
  void* p = pool.alloc(bytes, nullptr);
  pool.free(p, bytes, nullptr);
  std::printf("{\"mode\": \"doublefree\", \"freed_once\": true}\n");
  std::fflush(stdout);
  pool.free(p, bytes, nullptr);  // aborts
  std::printf("{\"mode\": \"doublefree\", \"survived\": true}\n");
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  const uint64_t seed = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1;
  const uint64_t steps = argc > 3 ? std::strtoull(argv[3], nullptr, 10) : 200000;
  if (mode == "random") return run_random(seed, steps);
  if (mode == "threads") return run_threads(seed, steps);
  if (mode == "doublefree") return run_doublefree(argc > 2 && !std::strcmp(argv[2], "small"));
  if (mode == "scenario" && argc > 2) {
    const std::string name = argv[2];
    if (name == "coalesce") return scenario_coalesce();
    if (name == "slack") return scenario_slack();
    if (name == "ladder") return scenario_ladder();
    if (name == "small") return scenario_small();
    if (name == "forget") return scenario_forget();
  }
  std::fprintf(stderr, "usage: pool_model random|threads SEED STEPS | scenario coalesce|slack|ladder|small|forget | doublefree [small]\n");
  return 2;
}
