// A stand-in for <hip/hip_runtime.h> on a machine without a GPU, for tests/native/resources_harness.cpp only: what
// uav_airvision_amd/csrc/av_resources.h calls, backed by malloc / free so that the address sanitizer sees every block, event and
// stream that is leaked, released twice or touched after its release.  fake_hip_fail_at = k makes the k-th acquiring call fail.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef int hipError_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2 };
typedef struct fake_hip_event { int live; }* hipEvent_t;
typedef struct fake_hip_stream { int live; }* hipStream_t;
enum { hipHostMallocDefault = 0, hipHostMallocMapped = 2, hipEventDefault = 0, hipEventBlockingSync = 1, hipEventDisableTiming = 2, hipStreamNonBlocking = 1 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2, hipMemcpyDeviceToDevice = 3 };

inline long fake_hip_fail_at = 0;           // 1-based index of the acquiring call that fails (0: none)
inline long fake_hip_acquisitions = 0;      // acquiring calls made so far
inline long fake_hip_live = 0;              // blocks + events + streams handed out and not yet taken back
inline bool fake_hip_acquire() { return ++fake_hip_acquisitions != fake_hip_fail_at; }

inline const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "out of memory (injected)"; }
inline hipError_t hipSetDevice(int) { return hipSuccess; }
inline hipError_t hipDeviceSynchronize() { return hipSuccess; }
inline hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }

inline hipError_t fake_hip_malloc(void** p, size_t bytes)
{
    if (!fake_hip_acquire()) return hipErrorOutOfMemory;
    *p = malloc(bytes ? bytes : 1);
    ++fake_hip_live;
    return hipSuccess;
}
inline hipError_t fake_hip_free(void* p) { if (p) { free(p); --fake_hip_live; } return hipSuccess; }
inline hipError_t hipMalloc(void** p, size_t bytes) { return fake_hip_malloc(p, bytes); }
inline hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) { return fake_hip_malloc(p, bytes); }
inline hipError_t hipFree(void* p) { return fake_hip_free(p); }
inline hipError_t hipHostFree(void* p) { return fake_hip_free(p); }
inline hipError_t hipMemset(void* p, int v, size_t bytes) { memset(p, v, bytes); return hipSuccess; }
inline hipError_t hipMemcpyAsync(void* d, const void* s, size_t bytes, hipMemcpyKind, hipStream_t) { memcpy(d, s, bytes); return hipSuccess; }

inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned)
{
    if (!fake_hip_acquire()) return hipErrorOutOfMemory;
    *e = static_cast<hipEvent_t>(malloc(sizeof(fake_hip_event))); (*e)->live = 1;
    ++fake_hip_live;
    return hipSuccess;
}
inline hipError_t hipEventDestroy(hipEvent_t e) { return fake_hip_free(e); }
inline hipError_t hipEventSynchronize(hipEvent_t e) { return e->live ? hipSuccess : hipErrorOutOfMemory; }
inline hipError_t hipEventRecord(hipEvent_t e, hipStream_t) { return e->live ? hipSuccess : hipErrorOutOfMemory; }
inline hipError_t fake_hip_stream_create(hipStream_t* s)
{
    if (!fake_hip_acquire()) return hipErrorOutOfMemory;
    *s = static_cast<hipStream_t>(malloc(sizeof(fake_hip_stream))); (*s)->live = 1;
    ++fake_hip_live;
    return hipSuccess;
}
inline hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned, int) { return fake_hip_stream_create(s); }
inline hipError_t hipExtStreamCreateWithCUMask(hipStream_t* s, uint32_t, const uint32_t*) { return fake_hip_stream_create(s); }
inline hipError_t hipStreamDestroy(hipStream_t s) { return fake_hip_free(s); }
