// pool_example.cpp — one check on the device that DevicePool's events order real work
// (tests/test_gpu_pool.py; the allocator's logic is tested on the CPU by pooltest/pool_model.cpp).
// Runtime fills and copies only, no kernel of this project.
//
//   pool_example [FILLS]     FILLS whole-block hipMemsetAsync calls keep stream A busy (default 64)
//
// cross_stream_reuse  a block above kChunk and kSlackMin, filled with 0xAA FILLS times on A and
//                     freed on A, is handed to B while A still runs (same pointer, held unchanged:
//                     the slack rule's wait path); B zero-fills it and reads back the first, middle
//                     and last 4 KiB: all zero, or the pool's wait did not hold B back
// reuse_after_drain   after a device synchronise another stream gets the block, held unchanged
// small_blocks        a small block freed on a busy A is not handed to B; after the synchronise it is
// stream_teardown     allocate and free on a stream, synchronise, forget_stream, destroy it; later
//                     allocations on other streams work and the device synchronises cleanly
// One JSON line per check; exits non-zero at the first HIP error or failed check.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../host/buffer.h"

using phantom::DevicePool;

#define HIP_OK(call)                                                                              \
  do {                                                                                            \
    const hipError_t e_ = (call);                                                                 \
    if (e_ != hipSuccess) {                                                                       \
      std::printf("{\"error\": \"%s\", \"call\": \"%s\", \"line\": %d}\n", hipGetErrorString(e_), #call, __LINE__); \
      std::exit(1);                                                                               \
    }                                                                                             \
  } while (0)

static void verdict(bool ok) {
  if (ok) return;
  std::printf("{\"done\": \"pool_example\", \"ok\": false}\n");
  std::exit(1);
}

// is the stream still running?  (hipErrorNotReady stays as the thread's last error: cleared)
static bool busy(hipStream_t s) {
  const hipError_t r = hipStreamQuery(s);
  if (r == hipErrorNotReady) {
    (void)hipGetLastError();
    return true;
  }
  HIP_OK(r);
  return false;
}

int main(int argc, char** argv) try {
  const int fills = argc > 1 ? std::atoi(argv[1]) : 64;
  constexpr size_t kBig = DevicePool::kSlackMin + (size_t(64) << 20);  // above kChunk and kSlackMin
  constexpr size_t kProbe = 4096;
  static_assert(kBig > DevicePool::kChunk && kBig % DevicePool::kGrain == 0);
  DevicePool& pool = DevicePool::instance();
  hipStream_t a, b;
  HIP_OK(hipStreamCreate(&a));
  HIP_OK(hipStreamCreate(&b));

  // --- cross-stream reuse behind the pool's wait
  char* p = static_cast<char*>(pool.alloc(kBig, a));
  for (int i = 0; i < fills; ++i) HIP_OK(hipMemsetAsync(p, 0xAA, kBig, a));
  pool.free(p, kBig, a);
  const size_t held = pool.stats().held;
  char* q = static_cast<char*>(pool.alloc(kBig, b));
  const bool overlapped = busy(a);  // A was still filling when B got the block
  const bool same = q == p, held_same = pool.stats().held == held;
  HIP_OK(hipMemsetAsync(q, 0x00, kBig, b));
  std::vector<unsigned char> host(3 * kProbe, 0x55);
  const size_t offs[3] = {0, (kBig / 2) / kProbe * kProbe, kBig - kProbe};
  for (int i = 0; i < 3; ++i)
    HIP_OK(hipMemcpyAsync(host.data() + i * kProbe, q + offs[i], kProbe, hipMemcpyDeviceToHost, b));
  HIP_OK(hipStreamSynchronize(b));
  size_t nonzero = 0;
  for (unsigned char c : host) nonzero += c != 0;
  bool ok = same && held_same && overlapped && nonzero == 0;
  std::printf("{\"check\": \"cross_stream_reuse\", \"fills\": %d, \"bytes\": %zu, \"same_pointer\": %s, \"held_unchanged\": %s, "
              "\"overlapped\": %s, \"nonzero_bytes\": %zu, \"ok\": %s}\n",
              fills, kBig, same ? "true" : "false", held_same ? "true" : "false", overlapped ? "true" : "false", nonzero,
              ok ? "true" : "false");
  verdict(ok);

  // --- reuse after a drain, in both directions
  pool.free(q, kBig, b);
  HIP_OK(hipDeviceSynchronize());
  char* r = static_cast<char*>(pool.alloc(kBig, a));
  bool drained = r == p && pool.stats().held == held;
  HIP_OK(hipMemsetAsync(r, 0x11, kBig, a));
  pool.free(r, kBig, a);
  HIP_OK(hipDeviceSynchronize());
  char* t = static_cast<char*>(pool.alloc(kBig, b));
  drained = drained && t == p && pool.stats().held == held;
  std::printf("{\"check\": \"reuse_after_drain\", \"ok\": %s}\n", drained ? "true" : "false");
  verdict(drained);

  // --- small blocks: not across streams while the freeing stream is busy
  pool.free(t, kBig, b);
  HIP_OK(hipDeviceSynchronize());
  char* big = static_cast<char*>(pool.alloc(kBig, a));
  char* sp = static_cast<char*>(pool.alloc(kProbe, a));
  HIP_OK(hipMemsetAsync(sp, 0x22, kProbe, a));
  for (int i = 0; i < fills; ++i) HIP_OK(hipMemsetAsync(big, 0x33, kBig, a));
  pool.free(sp, kProbe, a);
  char* sq = static_cast<char*>(pool.alloc(kProbe, b));
  const bool small_overlapped = busy(a);
  const bool kept = sq != sp;
  HIP_OK(hipMemsetAsync(sq, 0x44, kProbe, b));
  HIP_OK(hipDeviceSynchronize());
  char* sr = static_cast<char*>(pool.alloc(kProbe, b));
  const bool handed = sr == sp;
  ok = small_overlapped && kept && handed;
  std::printf("{\"check\": \"small_blocks\", \"overlapped\": %s, \"kept_from_b_while_busy\": %s, \"handed_to_b_after_sync\": %s, "
              "\"ok\": %s}\n",
              small_overlapped ? "true" : "false", kept ? "true" : "false", handed ? "true" : "false", ok ? "true" : "false");
  verdict(ok);

  // --- stream teardown (OwnedStream's sequence)
  constexpr size_t kMid = size_t(64) << 20;
  hipStream_t c;
  HIP_OK(hipStreamCreate(&c));
  char* cb = static_cast<char*>(pool.alloc(kMid, c));
  char* cs = static_cast<char*>(pool.alloc(kProbe, c));
  HIP_OK(hipMemsetAsync(cb, 0x66, kMid, c));
  HIP_OK(hipMemsetAsync(cs, 0x66, kProbe, c));
  pool.free(cb, kMid, c);
  pool.free(cs, kProbe, c);
  HIP_OK(hipStreamSynchronize(c));
  pool.forget_stream(c);
  HIP_OK(hipStreamDestroy(c));
  const size_t held_before = pool.stats().held;
  hipStream_t ab[2] = {a, b};
  char *mb[2], *ms[2];
  for (int i = 0; i < 2; ++i) {
    mb[i] = static_cast<char*>(pool.alloc(kMid, ab[i]));
    ms[i] = static_cast<char*>(pool.alloc(kProbe, ab[i]));
    HIP_OK(hipMemsetAsync(mb[i], 0x77, kMid, ab[i]));
    HIP_OK(hipMemsetAsync(ms[i], 0x77, kProbe, ab[i]));
  }
  // the forgotten stream's blocks are plain free blocks: the first taker gets them
  const bool reused = mb[0] == cb && ms[0] == cs;
  const bool no_growth = pool.stats().held == held_before + kProbe;  // (only b's small block is new)
  HIP_OK(hipDeviceSynchronize());
  for (int i = 0; i < 2; ++i) {
    pool.free(mb[i], kMid, ab[i]);
    pool.free(ms[i], kProbe, ab[i]);
  }
  pool.free(big, kBig, a);
  pool.free(sq, kProbe, b);
  pool.free(sr, kProbe, b);
  HIP_OK(hipDeviceSynchronize());
  for (hipStream_t s : ab) {
    pool.forget_stream(s);
    HIP_OK(hipStreamDestroy(s));
  }
  ok = reused && no_growth && pool.stats().live == 0;
  std::printf("{\"check\": \"stream_teardown\", \"blocks_reused\": %s, \"no_growth\": %s, \"live_after\": %zu, \"ok\": %s}\n",
              reused ? "true" : "false", no_growth ? "true" : "false", pool.stats().live, ok ? "true" : "false");
  verdict(ok);
  std::printf("{\"done\": \"pool_example\", \"ok\": true}\n");
  return 0;
} catch (const std::exception& e) {
  std::printf("{\"error\": \"%s\"}\n", e.what());
  return 1;
}
