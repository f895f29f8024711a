// fake_hip.cpp — the fake HIP runtime of the DevicePool model test (see fake_hip.h).
#include "fake_hip.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <deque>
#include <map>
#include <mutex>
#include <thread>

struct fakeStream {
  uint64_t uid = 0;
  bool alive = true;
  uint64_t issued = 0, done = 0;  // operations enqueued / completed (positions count from 1)
  struct Wait {
    uint64_t at, uid, pos;  // operation `at` of this stream waits for `pos` on stream `uid`
  };
  std::deque<Wait> waits;        // not yet completed, in order
  std::vector<uint64_t> clock;   // by uid: that stream's position known to happen before our next operation
};

struct fakeEvent {
  bool recorded = false;
  uint64_t uid = 0, pos = 0;
  std::vector<uint64_t> clock;
};

namespace {

std::mutex g_mu;
fakeStream g_null;                          // behind the handle nullptr, uid 0
// (owners of heap objects are themselves never destroyed, so a leak checker still reaches them at exit)
std::vector<fakeStream*>& g_handles = *new std::vector<fakeStream*>();  // every handle ever made (owned)
std::vector<fakeStream*> g_dead;            // destroyed handles, reused by later creates
std::map<uint64_t, fakeStream*> g_by_uid;   // live streams
std::vector<fakeEvent*>& g_events = *new std::vector<fakeEvent*>();     // owned
std::map<uintptr_t, size_t> g_allocs;
uint64_t g_next_uid = 1;
uint64_t g_creates = 0;
uintptr_t g_next_addr = uintptr_t(1) << 44;
size_t g_outstanding = 0, g_capacity = ~size_t(0);
unsigned g_sleep_us = 0;
size_t g_sleep_min = 0;
fake::Counters g_cnt;

void misuse(const char* what, const void* h) {
  if (g_cnt.errors++ < 10) std::fprintf(stderr, "fake hip: %s (%p)\n", what, h);
}

// the live stream behind a handle; nullptr (and one misuse) for a destroyed one
fakeStream* resolve(hipStream_t s, const char* call) {
  if (!s) return &g_null;
  if (!s->alive) {
    misuse(call, s);
    return nullptr;
  }
  return s;
}

bool done_locked(uint64_t uid, uint64_t pos) {
  auto it = g_by_uid.find(uid);
  return it == g_by_uid.end() || it->second->done >= pos;
}

// completes the stream's operations up to `pos`, and first whatever its waits wait for (a wait
// names a position that existed when it was enqueued, so this ends)
void complete_to(fakeStream* st, uint64_t pos) {
  while (st->done < pos) {
    if (!st->waits.empty() && st->waits.front().at == st->done + 1) {
      const fakeStream::Wait w = st->waits.front();
      auto it = g_by_uid.find(w.uid);
      if (it != g_by_uid.end()) complete_to(it->second, w.pos);
      st->waits.pop_front();
    }
    ++st->done;
  }
}

void reset_stream(fakeStream* st, uint64_t uid) {
  st->uid = uid;
  st->alive = true;
  st->issued = st->done = 0;
  st->waits.clear();
  st->clock.clear();
}

}  // namespace

namespace fake {

void reset(size_t capacity_bytes) {
  std::lock_guard<std::mutex> lk(g_mu);
  for (fakeStream* s : g_handles) delete s;
  for (fakeEvent* e : g_events) delete e;
  g_handles.clear();
  g_dead.clear();
  g_events.clear();
  g_by_uid.clear();
  g_allocs.clear();
  reset_stream(&g_null, 0);
  g_by_uid[0] = &g_null;
  g_next_uid = 1;
  g_creates = 0;
  g_outstanding = 0;
  g_capacity = capacity_bytes;
  g_sleep_us = 0;
  g_cnt = Counters();
}

void set_malloc_sleep_us(unsigned us, size_t min_bytes) {
  std::lock_guard<std::mutex> lk(g_mu);
  g_sleep_us = us;
  g_sleep_min = min_bytes;
}

Counters counters() {
  std::lock_guard<std::mutex> lk(g_mu);
  return g_cnt;
}

size_t outstanding() {
  std::lock_guard<std::mutex> lk(g_mu);
  return g_outstanding;
}

bool inside_allocation(const void* p, size_t bytes) {
  std::lock_guard<std::mutex> lk(g_mu);
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  auto it = g_allocs.upper_bound(a);
  if (it == g_allocs.begin()) return false;
  --it;
  return a + bytes <= it->first + it->second;
}

uint64_t uid(hipStream_t s) {
  std::lock_guard<std::mutex> lk(g_mu);
  fakeStream* st = resolve(s, "uid of a destroyed stream");
  return st ? st->uid : 0;
}

uint64_t enqueue_work(hipStream_t s) {
  std::lock_guard<std::mutex> lk(g_mu);
  fakeStream* st = resolve(s, "work enqueued on a destroyed stream");
  return st ? ++st->issued : 0;
}

size_t advance(hipStream_t s, size_t n) {
  std::lock_guard<std::mutex> lk(g_mu);
  fakeStream* st = resolve(s, "advance of a destroyed stream");
  if (!st) return 0;
  size_t k = 0;
  while (k < n && st->done < st->issued) {
    if (!st->waits.empty() && st->waits.front().at == st->done + 1) {
      if (!done_locked(st->waits.front().uid, st->waits.front().pos)) break;
      st->waits.pop_front();
    }
    ++st->done;
    ++k;
  }
  return k;
}

bool completed(uint64_t stream_uid, uint64_t pos) {
  std::lock_guard<std::mutex> lk(g_mu);
  return done_locked(stream_uid, pos);
}

bool ordered_before(hipStream_t s, uint64_t before_uid, uint64_t pos) {
  std::lock_guard<std::mutex> lk(g_mu);
  fakeStream* st = resolve(s, "ordering asked of a destroyed stream");
  if (!st) return false;
  if (st->uid == before_uid) return true;
  return before_uid < st->clock.size() && st->clock[before_uid] >= pos;
}

size_t backlog(hipStream_t s) {
  std::lock_guard<std::mutex> lk(g_mu);
  fakeStream* st = resolve(s, "backlog of a destroyed stream");
  return st ? static_cast<size_t>(st->issued - st->done) : 0;
}

}  // namespace fake

const char* hipGetErrorString(hipError_t e) {
  switch (e) {
    case hipSuccess: return "no error";
    case hipErrorOutOfMemory: return "out of memory";
    case hipErrorNotReady: return "device not ready";
    case hipErrorInvalidHandle: return "invalid resource handle";
    default: return "invalid argument";
  }
}

hipError_t hipGetLastError() { return hipSuccess; }

hipError_t hipGetDevice(int* dev) {
  *dev = 0;
  return hipSuccess;
}

// Addresses come from a counter and are never reused; consecutive allocations are contiguous, so
// a pool that merged blocks across its chunks would be found out.  No memory is touched.
hipError_t hipMalloc(void** p, size_t bytes) {
  unsigned sleep_us = 0;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    if (bytes > g_capacity || g_outstanding > g_capacity - bytes) {
      ++g_cnt.malloc_failures;
      *p = nullptr;
      return hipErrorOutOfMemory;
    }
    ++g_cnt.mallocs;
    *p = reinterpret_cast<void*>(g_next_addr);
    g_allocs[g_next_addr] = bytes;
    g_next_addr += (bytes + 255) / 256 * 256;
    g_outstanding += bytes;
    if (g_sleep_us && bytes >= g_sleep_min) sleep_us = g_sleep_us;
  }
  if (sleep_us) std::this_thread::sleep_for(std::chrono::microseconds(sleep_us));
  return hipSuccess;
}

hipError_t hipFree(void* p) {
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_allocs.find(reinterpret_cast<uintptr_t>(p));
  if (it == g_allocs.end()) {
    misuse("hipFree of a pointer hipMalloc did not return", p);
    return hipErrorInvalidValue;
  }
  ++g_cnt.frees;
  g_outstanding -= it->second;
  g_allocs.erase(it);
  return hipSuccess;
}

hipError_t hipStreamCreate(hipStream_t* s) {
  std::lock_guard<std::mutex> lk(g_mu);
  fakeStream* st = nullptr;
  if ((++g_creates & 1) == 0 && !g_dead.empty()) {  // every second create reuses a destroyed handle
    st = g_dead.front();
    g_dead.erase(g_dead.begin());
  } else {
    st = new fakeStream();
    g_handles.push_back(st);
  }
  reset_stream(st, g_next_uid++);
  g_by_uid[st->uid] = st;
  *s = st;
  return hipSuccess;
}

hipError_t hipStreamDestroy(hipStream_t s) {
  std::lock_guard<std::mutex> lk(g_mu);
  fakeStream* st = resolve(s, "hipStreamDestroy of a destroyed stream");
  if (!st) return hipErrorInvalidHandle;
  if (st == &g_null) {
    misuse("hipStreamDestroy of the null stream", s);
    return hipErrorInvalidHandle;
  }
  complete_to(st, st->issued);
  g_by_uid.erase(st->uid);
  st->alive = false;
  g_dead.push_back(st);
  return hipSuccess;
}

hipError_t hipStreamSynchronize(hipStream_t s) {
  std::lock_guard<std::mutex> lk(g_mu);
  fakeStream* st = resolve(s, "hipStreamSynchronize of a destroyed stream");
  if (!st) return hipErrorInvalidHandle;
  ++g_cnt.stream_syncs;
  complete_to(st, st->issued);
  return hipSuccess;
}

hipError_t hipDeviceSynchronize() {
  std::lock_guard<std::mutex> lk(g_mu);
  ++g_cnt.device_syncs;
  for (auto& kv : g_by_uid) complete_to(kv.second, kv.second->issued);
  return hipSuccess;
}

hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) {
  std::lock_guard<std::mutex> lk(g_mu);
  g_events.push_back(new fakeEvent());
  *e = g_events.back();
  return hipSuccess;
}

hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
  std::lock_guard<std::mutex> lk(g_mu);
  fakeStream* st = resolve(s, "hipEventRecord on a destroyed stream");
  if (!st) return hipErrorInvalidHandle;
  ++g_cnt.event_records;
  e->recorded = true;
  e->uid = st->uid;
  e->pos = ++st->issued;
  e->clock = st->clock;
  if (e->clock.size() <= st->uid) e->clock.resize(st->uid + 1, 0);
  e->clock[st->uid] = e->pos;
  return hipSuccess;
}

hipError_t hipEventQuery(hipEvent_t e) {
  std::lock_guard<std::mutex> lk(g_mu);
  ++g_cnt.event_queries;
  if (!e->recorded) return hipSuccess;
  if (!g_by_uid.count(e->uid)) {
    misuse("hipEventQuery of an event last recorded on a destroyed stream", e);
    return hipSuccess;
  }
  return done_locked(e->uid, e->pos) ? hipSuccess : hipErrorNotReady;
}

hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) {
  std::lock_guard<std::mutex> lk(g_mu);
  fakeStream* st = resolve(s, "hipStreamWaitEvent on a destroyed stream");
  if (!st) return hipErrorInvalidHandle;
  ++g_cnt.stream_waits;
  if (!e->recorded) return hipSuccess;
  if (!g_by_uid.count(e->uid)) {
    misuse("hipStreamWaitEvent on an event last recorded on a destroyed stream", e);
    return hipSuccess;
  }
  st->waits.push_back({++st->issued, e->uid, e->pos});
  if (st->clock.size() < e->clock.size()) st->clock.resize(e->clock.size(), 0);
  for (size_t i = 0; i < e->clock.size(); ++i) st->clock[i] = std::max(st->clock[i], e->clock[i]);
  return hipSuccess;
}

hipError_t hipMemcpyAsync(void*, const void*, size_t, hipMemcpyKind, hipStream_t) { return hipSuccess; }
hipError_t hipMemcpy(void*, const void*, size_t, hipMemcpyKind) { return hipSuccess; }
hipError_t hipMemset(void*, int, size_t) { return hipSuccess; }
hipError_t hipMemsetAsync(void*, int, size_t, hipStream_t) { return hipSuccess; }
