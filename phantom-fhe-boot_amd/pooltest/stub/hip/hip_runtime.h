// Stand-in for <hip/hip_runtime.h> in the CPU model test of DevicePool (pooltest/): only what
// host/buffer.h, host/hip_check.h and host/buffer.cpp name.  The functions are defined by
// pooltest/fake_hip.cpp, a model of streams and events that touches no device.
#pragma once

#include <cstddef>

enum hipError_t {
  hipSuccess = 0,
  hipErrorInvalidValue = 1,
  hipErrorOutOfMemory = 2,
  hipErrorInvalidHandle = 400,
  hipErrorNotReady = 600,
};

enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 };

struct fakeStream;
struct fakeEvent;
typedef fakeStream* hipStream_t;
typedef fakeEvent* hipEvent_t;

constexpr unsigned hipEventDisableTiming = 0x2;
constexpr unsigned hipEventDisableSystemFence = 0x20000000;

const char* hipGetErrorString(hipError_t e);
hipError_t hipGetLastError();
hipError_t hipGetDevice(int* dev);
hipError_t hipMalloc(void** p, size_t bytes);
hipError_t hipFree(void* p);
hipError_t hipStreamCreate(hipStream_t* s);
hipError_t hipStreamDestroy(hipStream_t s);
hipError_t hipStreamSynchronize(hipStream_t s);
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned flags);
hipError_t hipDeviceSynchronize();
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags);
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s);
hipError_t hipEventQuery(hipEvent_t e);
// named by DeviceBuffer's members (never instantiated by the model test)
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s);
hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind);
hipError_t hipMemset(void* dst, int value, size_t bytes);
hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t s);
