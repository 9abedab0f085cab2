// av_resources.h -- the one place that acquires and releases device memory, pinned host memory, events and streams.
//
// Every object of the library (av_frontend, av_msckf, av_msckf_batch with its DevPath) holds one AvResources and takes everything it
// keeps on its device from it.  The owner remembers what it handed out, so a *_destroy entry is `res.release()`, an error return
// halfway through a group of acquisitions leaks nothing (what was created before the failure is released with the rest), and a
// member added to an object needs no line in any release list.  AvScratch is the same for the one-shot scratch of an operator entry.
// Four process-wide live counts (device bytes, pinned bytes, events, streams) pass through every acquisition and release; the tests
// read them through av_debug_live_resources.
//
// Left alone on purpose: the process-lifetime diagnostics g_lk_prof (lk.hip) and the DevStamps statics (msckf_dev_host.inc).  They
// are allocated once behind an environment switch and never freed: a static destructor would run after the HIP runtime has gone.
//
// Includes only the HIP runtime header, the public header and the declaration of av_set_error: tests/native/resources_harness.cpp
// compiles this file for the CPU against a stand-in <hip/hip_runtime.h> and runs it under the address sanitizer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <atomic>
#include <vector>

#include "../../include/airvision.h"

void av_set_error(const char* fmt, ...);
#define AV_HIP(call)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            av_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return AV_E_HIP;                                                                      \
        }                                                                                         \
    } while (0)

enum { AV_LIVE_DEV_BYTES = 0, AV_LIVE_PINNED_BYTES = 1, AV_LIVE_EVENTS = 2, AV_LIVE_STREAMS = 3 };
inline std::atomic<int64_t> av_live_counts[4];
inline void av_live_add(int what, int64_t n) { av_live_counts[what].fetch_add(n, std::memory_order_relaxed); }

class AvResources {
public:
    int device = 0;                          // the device everything below lives on (set by the owner's create entry before the first acquisition)

    AvResources() = default;
    AvResources(const AvResources&) = delete;
    AvResources& operator=(const AvResources&) = delete;
    ~AvResources() { release(); }

    // `bytes` of device / pinned memory as the runtime hands them out: no slack, no fill
    template <typename T>
    int dev_bytes(T** p, size_t bytes)
    {
        void* q = nullptr;
        AV_HIP(hipMalloc(&q, bytes));
        dev_.push_back(Block{q, bytes});
        av_live_add(AV_LIVE_DEV_BYTES, (int64_t)bytes);
        *p = reinterpret_cast<T*>(q);
        return AV_OK;
    }
    template <typename T>
    int pinned_bytes(T** p, size_t bytes, unsigned flags = hipHostMallocDefault)
    {
        void* q = nullptr;
        AV_HIP(hipHostMalloc(&q, bytes, flags));
        pinned_.push_back(Block{q, bytes});
        av_live_add(AV_LIVE_PINNED_BYTES, (int64_t)bytes);
        *p = reinterpret_cast<T*>(q);
        return AV_OK;
    }
    // count elements + 256 bytes of slack, every byte set to `fill`.  The fill runs on the null stream and the buffer is used on
    // non-blocking streams that do not wait for it, so the null stream is synchronised before the pointer is handed out
    // (create-time and reserve-time work only).
    template <typename T>
    int dev(T** p, size_t count, int fill = 0)
    {
        const size_t bytes = count * sizeof(T) + 256;
        T* q = nullptr;
        int rc = dev_bytes(&q, bytes);
        if (rc) return rc;
        AV_HIP(hipMemset(q, fill, bytes));
        AV_HIP(hipStreamSynchronize(nullptr));
        *p = q;
        return AV_OK;
    }
    // count elements + 64 bytes of slack, zeroed
    template <typename T>
    int pinned(T** p, size_t count, unsigned flags = hipHostMallocDefault)
    {
        const size_t bytes = count * sizeof(T) + 64;
        T* q = nullptr;
        int rc = pinned_bytes(&q, bytes, flags);
        if (rc) return rc;
        memset(q, 0, bytes);
        *p = q;
        return AV_OK;
    }
    int event(hipEvent_t* e, unsigned flags)
    {
        hipEvent_t q = nullptr;
        AV_HIP(hipEventCreateWithFlags(&q, flags));
        events_.push_back(q);
        av_live_add(AV_LIVE_EVENTS, 1);
        *e = q;
        return AV_OK;
    }
    int stream(hipStream_t* s, unsigned flags, int priority) { return own_stream(s, hipStreamCreateWithPriority(s, flags, priority)); }
    // a stream confined to the compute units of `mask` (hipExtStreamCreateWithCUMask)
    int stream_on_cus(hipStream_t* s, uint32_t words, const uint32_t* mask) { return own_stream(s, hipExtStreamCreateWithCUMask(s, words, mask)); }

    // Hand single blocks or events back before release (growth of a staging area, a new set of timing events).  The caller has made
    // sure that nothing queued still uses them; null is ignored; the handle is null afterwards.
    template <typename T>
    void free_dev(T*& p) { if (p && drop(dev_, p, AV_LIVE_DEV_BYTES)) (void)hipFree(p); p = nullptr; }
    template <typename T>
    void free_pinned(T*& p) { if (p && drop(pinned_, p, AV_LIVE_PINNED_BYTES)) (void)hipHostFree(p); p = nullptr; }
    void free_event(hipEvent_t& e)
    {
        for (size_t i = events_.size(); e && i-- > 0;)          // from the back: the newest are handed back first
            if (events_[i] == e) { (void)hipEventDestroy(e); events_.erase(events_.begin() + (long)i); av_live_add(AV_LIVE_EVENTS, -1); break; }
        e = nullptr;
    }

    // The grow rule of the frame store's scratches: grows only; an old block is freed after `drain` has run dry (earlier launches on
    // it may still read the block), so the caller stalls once per growth and never otherwise; the new capacity is need + 16 elements.
    template <typename T>
    int regrow(T** p, size_t* cap, size_t need, size_t elem_bytes, hipStream_t drain)
    {
        if (need <= *cap) return AV_OK;
        if (*p) { AV_HIP(hipStreamSynchronize(drain)); free_dev(*p); *cap = 0; }
        int rc = dev_bytes(p, (need + 16) * elem_bytes);
        if (rc) return rc;
        *cap = need + 16;
        return AV_OK;
    }

    // DevBuf: the sum of the `growths` of every buffer that takes its memory from this owner
    void attach_growths(const long long* g) { growths_.push_back(g); }
    long long growths() const { long long n = 0; for (const long long* g : growths_) n += *g; return n; }

    // Waits for the device, then events, streams, device memory, pinned memory.  The owner is empty afterwards and may be used again.
    void release()
    {
        if (dev_.empty() && pinned_.empty() && events_.empty() && streams_.empty()) return;
        (void)hipSetDevice(device);
        (void)hipDeviceSynchronize();
        for (hipEvent_t e : events_) (void)hipEventDestroy(e);
        for (hipStream_t s : streams_) (void)hipStreamDestroy(s);
        for (const Block& b : dev_) { (void)hipFree(b.p); av_live_add(AV_LIVE_DEV_BYTES, -(int64_t)b.bytes); }
        for (const Block& b : pinned_) { (void)hipHostFree(b.p); av_live_add(AV_LIVE_PINNED_BYTES, -(int64_t)b.bytes); }
        av_live_add(AV_LIVE_EVENTS, -(int64_t)events_.size());
        av_live_add(AV_LIVE_STREAMS, -(int64_t)streams_.size());
        events_.clear(); streams_.clear(); dev_.clear(); pinned_.clear();
    }

private:
    struct Block { void* p; size_t bytes; };
    std::vector<Block> dev_, pinned_;
    std::vector<hipEvent_t> events_;
    std::vector<hipStream_t> streams_;
    std::vector<const long long*> growths_;

    int own_stream(hipStream_t* s, hipError_t created)
    {
        if (created != hipSuccess) { *s = nullptr; av_set_error("stream creation failed: %s", hipGetErrorString(created)); return AV_E_HIP; }
        streams_.push_back(*s);
        av_live_add(AV_LIVE_STREAMS, 1);
        return AV_OK;
    }
    static bool drop(std::vector<Block>& v, const void* p, int what)
    {
        for (size_t i = 0; i < v.size(); ++i)
            if (v[i].p == p) { av_live_add(what, -(int64_t)v[i].bytes); v.erase(v.begin() + (long)i); return true; }
        return false;
    }
};

// One-shot device scratch of an operator entry: freed on every return path.
struct AvScratch {
    void* p = nullptr; size_t bytes = 0;
    AvScratch() = default;
    AvScratch(const AvScratch&) = delete;
    AvScratch& operator=(const AvScratch&) = delete;
    int alloc(size_t n) { AV_HIP(hipMalloc(&p, n)); bytes = n; av_live_add(AV_LIVE_DEV_BYTES, (int64_t)n); return AV_OK; }
    ~AvScratch() { if (p) { (void)hipFree(p); av_live_add(AV_LIVE_DEV_BYTES, -(int64_t)bytes); } }
};

// N pinned slots of `count` elements with one event each.  A caller takes the next slot -- waiting until the copy that read it N
// calls ago has finished --, fills it, enqueues its copy to the device and records the slot's event behind the copy.
template <typename T, int N>
struct PinnedRing {
    T* h[N] = {}; hipEvent_t ev[N] = {}; int next = 0, cur = 0;
    int create(AvResources& r, size_t count)
    {
        int rc = AV_OK;
        for (int i = 0; i < N && !rc; ++i)
            if (!(rc = r.pinned(&h[i], count))) rc = r.event(&ev[i], hipEventDisableTiming);
        return rc;
    }
    int take(T** slot)
    {
        cur = next; next = (next + 1) % N;
        AV_HIP(hipEventSynchronize(ev[cur]));
        *slot = h[cur];
        return AV_OK;
    }
    int sent(hipStream_t st) { AV_HIP(hipEventRecord(ev[cur], st)); return AV_OK; }
};

// A device buffer that is uploaded every step, with its pinned (mapped) staging.
// Growth is geometric and never frees inside a step: hipFree synchronises the whole device and queued copies / kernels of another
// stream may still read the old allocation, so outgrown blocks stay with the owner until it releases.  `growths` counts the
// reallocations after the first reserve (AvResources::growths sums them).
// (Its user was the host-bookkeeping form of the batched filter, which is gone; tests/native/resources_harness.cpp still drives it.)
template <typename T>
struct DevBuf {
    AvResources* res;
    T* p = nullptr; size_t cap = 0;
    T* stage = nullptr; size_t stage_cap = 0;          // pinned staging: async H2D without a sync per upload
    long long growths = 0;
    explicit DevBuf(AvResources& r) : res(&r) { r.attach_growths(&growths); }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    int ensure(size_t n)
    {
        if (n <= cap) return AV_OK;
        const size_t ncap = n + n / 2 + 64;
        T* q = nullptr;
        int rc = res->dev_bytes(&q, ncap * sizeof(T));
        if (rc) return rc;
        if (p) ++growths;
        p = q; cap = ncap;
        return AV_OK;
    }
    int ensure_stage(size_t n)
    {
        if (n <= stage_cap) return AV_OK;
        const size_t ncap = n + n / 2 + 64;
        T* q = nullptr;
        int rc = res->pinned_bytes(&q, ncap * sizeof(T), hipHostMallocMapped);
        if (rc) return rc;
        if (stage) ++growths;
        stage = q; stage_cap = ncap;
        return AV_OK;
    }
    int reserve(size_t n, bool with_stage) { int rc = ensure(n); if (!rc && with_stage) rc = ensure_stage(n); return rc; }
    // The staging buffer is reused by the next upload of the SAME buffer; every phase of the step synchronises the
    // stream (gate flags / delta_x / variances come back) before any buffer is uploaded again, so the copy has landed.
    int upload(const std::vector<T>& h, hipStream_t st)
    {
        int rc = ensure(h.size());
        if (rc) return rc;
        if (h.empty()) return AV_OK;
        if ((rc = ensure_stage(h.size()))) return rc;
        memcpy(stage, h.data(), h.size() * sizeof(T));
        AV_HIP(hipMemcpyAsync(p, stage, h.size() * sizeof(T), hipMemcpyHostToDevice, st));
        return AV_OK;
    }
    // Fill the pinned staging buffer in place (no intermediate std::vector), then commit(n) enqueues the copy.
    int stage_for(size_t n, hipStream_t st, T** out)
    {
        (void)st;
        int rc = ensure(n);
        if (rc) return rc;
        if ((rc = ensure_stage(n))) return rc;
        *out = stage;
        return AV_OK;
    }
    int commit(size_t n, hipStream_t st)
    {
        if (n == 0) return AV_OK;
        AV_HIP(hipMemcpyAsync(p, stage, n * sizeof(T), hipMemcpyHostToDevice, st));
        return AV_OK;
    }
};
