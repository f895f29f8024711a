// fake_hip.h — the test's side of the fake HIP runtime (fake_hip.cpp): a model of streams and
// events in which nothing runs by itself.
//
// A stream is a sequence of operations (work, event record, wait on an event).  Only the test
// completes them (advance, or the synchronise calls); a wait completes only when the position it
// snapshot on the recording stream has.  Every stream carries a vector clock: for each other
// stream, the position up to which that stream's operations happen before whatever is enqueued
// next.  An event record copies the clock (with the stream's own position), a wait merges it, so
// the clocks are transitive.
// Every stream has a unique id for its lifetime; a handle value is reused by a later stream on
// purpose (DevicePool::forget_stream has to cope with that).
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace fake {

struct Counters {
  uint64_t mallocs = 0, malloc_failures = 0, frees = 0;
  uint64_t event_records = 0, event_queries = 0, stream_waits = 0;
  uint64_t stream_syncs = 0, device_syncs = 0;
  uint64_t errors = 0;  // misuse: a destroyed stream named, an event of a destroyed stream queried, ...
};

// forgets every stream, event and allocation; hipMalloc fails when the outstanding bytes would exceed the capacity
void reset(size_t capacity_bytes);
void set_malloc_sleep_us(unsigned us, size_t min_bytes);  // hipMalloc of min_bytes or more sleeps
Counters counters();
size_t outstanding();                // bytes handed out by hipMalloc and not freed
bool inside_allocation(const void* p, size_t bytes);

uint64_t uid(hipStream_t s);         // the live stream behind a handle (0: the null stream)
uint64_t enqueue_work(hipStream_t s);  // returns the operation's position on the stream
size_t advance(hipStream_t s, size_t n);  // completes up to n operations; stops at an unmet wait
bool completed(uint64_t stream_uid, uint64_t pos);  // (a destroyed stream was synchronised: true)
// does `pos` on stream `before_uid` happen before what `s` enqueues next?
bool ordered_before(hipStream_t s, uint64_t before_uid, uint64_t pos);
size_t backlog(hipStream_t s);       // operations enqueued and not completed

}  // namespace fake
