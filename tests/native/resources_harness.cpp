// resources_harness.cpp -- uav_airvision_amd/csrc/av_resources.h on the CPU, against tests/native/fake_hip (tests/test_resources.py
// builds this with -fsanitize=address,undefined).  A create-like sequence runs once clean and once for every k with the k-th
// acquiring call failing; each time the sequence has to report the failure, and after release the live counts and the stand-in's
// own count have to be back at zero.  What leaks, is released twice or is touched after its release is the sanitizer's to report.
#include <stdarg.h>
#include <stdio.h>

#include "av_resources.h"

static char g_err[512];
void av_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap); }

#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s (fail_at %ld, last error: %s)\n", __LINE__, #cond, fake_hip_fail_at, g_err); return 1; } } while (0)

static bool live_zero() { for (auto& c : av_live_counts) if (c.load() != 0) return false; return fake_hip_live == 0; }

struct Object {
    AvResources res;
    double* d[12] = {}; int* first = nullptr;
    double* h[3] = {};
    hipEvent_t ev[4] = {}; hipStream_t st[2] = {};
    PinnedRing<double, 8> ring;
    DevBuf<int> buf{res}; DevBuf<double> buf2{res};
    uint8_t* scratch = nullptr; size_t scratch_cap = 0;
    uint8_t* up_pin = nullptr; int* up_idx = nullptr;
    long long peak[4] = {};
};

// what a create entry, a reserve and a few steps with growing inputs do; peak = the live counts just before the return
static int sequence(Object& o)
{
    int rc;
    o.res.device = 0;
    for (int i = 0; i < 12; ++i) if ((rc = o.res.dev(&o.d[i], (size_t)100 * (i + 1)))) return rc;
    if ((rc = o.res.dev(&o.first, 64, 1))) return rc;
    if (o.first[63] != 0x01010101 || o.d[0][99] != 0.0 || reinterpret_cast<char*>(o.d[0] + 100)[255] != 0) { av_set_error("fill or slack wrong"); return AV_E_INVALID; }
    for (int i = 0; i < 3; ++i) if ((rc = o.res.pinned(&o.h[i], 50))) return rc;
    if (reinterpret_cast<char*>(o.h[2] + 50)[63] != 0) { av_set_error("pinned slack wrong"); return AV_E_INVALID; }
    for (int i = 0; i < 4; ++i) if ((rc = o.res.event(&o.ev[i], i < 2 ? hipEventDisableTiming : hipEventDefault))) return rc;
    if ((rc = o.res.stream(&o.st[0], hipStreamNonBlocking, 0))) return rc;
    const uint32_t mask[8] = {0xFFu};
    if ((rc = o.res.stream_on_cus(&o.st[1], 8, mask))) return rc;
    if ((rc = o.ring.create(o.res, 30))) return rc;
    for (int k = 0; k < 10; ++k) {            // more takes than slots: the cursor wraps
        double* slot = nullptr;
        if ((rc = o.ring.take(&slot))) return rc;
        slot[29] = k;
        if ((rc = o.ring.sent(o.st[0]))) return rc;
    }
    // a DevBuf that grows twice (device block and staging each), one that only reserves
    for (size_t n : {(size_t)10, (size_t)200, (size_t)5000}) {
        std::vector<int> v(n, 7);
        if ((rc = o.buf.upload(v, o.st[0]))) return rc;
        if (o.buf.p[n - 1] != 7) { av_set_error("upload wrong"); return AV_E_INVALID; }
    }
    if ((rc = o.buf2.reserve(1000, true))) return rc;
    if (o.buf.growths != 4 || o.buf2.growths != 0 || o.res.growths() != 4) { av_set_error("growths %lld", o.res.growths()); return AV_E_INVALID; }
    // the frame store's rule: 2 -> capacity 18, 10 fits, 20 -> 36, 40 -> 56
    const size_t want[4] = {18, 18, 36, 56}; const size_t need[4] = {2, 10, 20, 40};
    for (int k = 0; k < 4; ++k) {
        if ((rc = o.res.regrow(&o.scratch, &o.scratch_cap, need[k], 32, o.st[0]))) return rc;
        if (o.scratch_cap != want[k]) { av_set_error("regrow capacity %zu", o.scratch_cap); return AV_E_INVALID; }
        o.scratch[o.scratch_cap * 32 - 1] = 1;
    }
    // a staging entry that is handed back and built larger, timing events that are replaced
    for (size_t cap : {(size_t)18, (size_t)36}) {
        o.res.free_pinned(o.up_pin); o.res.free_dev(o.up_idx);
        if ((rc = o.res.pinned_bytes(&o.up_pin, cap * 64)) || (rc = o.res.dev_bytes(&o.up_idx, cap * sizeof(int)))) return rc;
    }
    o.res.free_event(o.ev[3]); o.res.free_event(o.ev[2]);
    if (o.ev[2] || o.ev[3]) { av_set_error("free_event left a handle"); return AV_E_INVALID; }
    for (int i = 2; i < 4; ++i) if ((rc = o.res.event(&o.ev[i], hipEventDefault))) return rc;
    {   // an operator entry's one-shot scratch
        AvScratch s;
        if ((rc = s.alloc(4096))) return rc;
        static_cast<char*>(s.p)[4095] = 1;
    }
    for (int i = 0; i < 4; ++i) o.peak[i] = av_live_counts[i].load();
    return AV_OK;
}

int main()
{
    long n_acq = 0;
    long long peak[4];
    {
        Object o;
        CHECK(live_zero());
        CHECK(sequence(o) == AV_OK);
        n_acq = fake_hip_acquisitions;
        for (int i = 0; i < 4; ++i) { peak[i] = o.peak[i]; CHECK(peak[i] > 0); }
        CHECK(peak[2] == 4 + 8 && peak[3] == 2);
        o.res.release();
        CHECK(live_zero());
        // the owner may be used again, and the destructor releases what an explicit release() has not
        double* again = nullptr;
        CHECK(o.res.dev(&again, 10) == AV_OK);
        CHECK(!live_zero());
    }
    CHECK(live_zero());
    CHECK(n_acq > 40);
    for (long k = 1; k <= n_acq; ++k) {
        fake_hip_acquisitions = 0; fake_hip_fail_at = k; g_err[0] = 0;
        {
            Object o;
            CHECK(sequence(o) == AV_E_HIP);
            CHECK(g_err[0] != 0);
            CHECK(fake_hip_acquisitions == k);          // the sequence stopped at the failure
            o.res.release();
            CHECK(live_zero());
        }
        CHECK(live_zero());
    }
    // a second clean cycle peaks where the first did
    fake_hip_fail_at = 0;
    {
        Object o;
        CHECK(sequence(o) == AV_OK);
        for (int i = 0; i < 4; ++i) CHECK(o.peak[i] == peak[i]);
    }
    CHECK(live_zero());
    printf("OK %ld\n", n_acq);
    return 0;
}
