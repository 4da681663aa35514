// Host side of the diagnostic build with in-kernel clock stamps (-DRN_CLOCK, tools/build_clock.sh; never shipped).  Every
// launch of a forward pass gets its own region of one host-visible buffer for the per-workgroup (delta s_memtime, delta
// s_memrealtime) pairs its kernel writes (clock_pair, rn_stage.h).  Nothing is synchronised or printed unless
// RN_CLOCK_REPORT is set in the environment WHEN the pass is enqueued -- set it for the last pass of a multi-second run, so
// that the stamped pass runs back to back with the ones before it.  Without RN_CLOCK the three calls do nothing and no
// kernel gets a buffer.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

#ifdef RN_CLOCK
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

struct ClockRegion {
    char what[32];
    size_t off, nwg;
};
static unsigned long long* g_clock_buf = nullptr;
static std::vector<ClockRegion> g_clock_regions;
static size_t g_clock_used = 0;
// the stamp buffer of a launch of nwg workgroups, reported as `what`
static unsigned long long* rn_clock_region(const char* what, size_t nwg) {
    if (!g_clock_buf) (void)hipHostMalloc(reinterpret_cast<void**>(&g_clock_buf), 16u << 20, 0);
    ClockRegion r{};
    snprintf(r.what, sizeof r.what, "%s", what);
    r.off = g_clock_used;
    r.nwg = nwg;
    g_clock_used += 2 * nwg;
    g_clock_regions.push_back(r);
    return g_clock_buf + r.off;
}
static void rn_clock_begin() {
    g_clock_regions.clear();
    g_clock_used = 0;
}
static void rn_clock_end(hipStream_t stream) {
    if (!getenv("RN_CLOCK_REPORT")) return;
    (void)hipStreamSynchronize(stream);
    for (const ClockRegion& r : g_clock_regions) {
        const unsigned long long* buf = g_clock_buf + r.off;
        std::vector<double> ghz, us;
        for (size_t k = 0; k < r.nwg; ++k)
            if (buf[2 * k + 1]) {
                ghz.push_back(static_cast<double>(buf[2 * k]) / static_cast<double>(buf[2 * k + 1]) * 0.1);
                us.push_back(static_cast<double>(buf[2 * k + 1]) * 0.01);
            }
        if (ghz.empty()) continue;
        std::sort(ghz.begin(), ghz.end());
        std::sort(us.begin(), us.end());
        fprintf(stderr, "[clock] %-12s in-kernel clock %.3f GHz (median of %zu workgroups; 10th / 90th percentile %.3f / %.3f), workgroup lifetime %.1f us median\n",
                r.what, ghz[ghz.size() / 2], ghz.size(), ghz[ghz.size() / 10], ghz[ghz.size() * 9 / 10], us[us.size() / 2]);
    }
}
#else
inline unsigned long long* rn_clock_region(const char*, size_t) { return nullptr; }
inline void rn_clock_begin() {}
inline void rn_clock_end(hipStream_t) {}
#endif
