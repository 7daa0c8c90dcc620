// The native trainer's launch timers (gs_trainer::timer, the bench roofline):
// arming and closing a timed launch, and the read-back API.
#include <cxxabi.h>

#include <algorithm>
#include <cstdlib>
#include <utility>

#include "trainer.hpp"

namespace gs {

LaunchTimer timed_arm(gs_trainer& T, int site) {
    auto& tm = T.timer[site];
    LaunchTimer lt;
    if (tm.n >= static_cast<int64_t>(tm.ev0.size())) return lt;
    if (++tm.calls % tm.every) return lt;
    lt.start = tm.ev0[tm.n];
    lt.stop = tm.ev1[tm.n];
    if (tm.st0) lt.stamp = {tm.st0 + tm.n * kStampBlocks, tm.st1 + tm.n * kStampBlocks};
    return lt;
}
// Timer events only measure: no system-scope release when they complete (a
// system-scope release writes back and invalidates the caches under the work
// that follows, which is what made event-bound launches cost the step time).
static unsigned timer_event_flags() { return hipEventDisableSystemFence; }

static std::string demangle(const char* sym) {
    if (!sym) return "?";
    int status = 0;
    char* d = abi::__cxa_demangle(sym, nullptr, nullptr, &status);
    std::string out = (status == 0 && d) ? d : sym;
    std::free(d);
    return out;
}

void timed_done(gs_trainer& T, int site, const LaunchTimer& lt) {
    if (!lt.start) return;
    auto& tm = T.timer[site];
    GS_REQUIRE(lt.kernel, GS_EINVAL, "timed launch did not reach a kernel");
    if (tm.st0) tm.stamped[tm.n] = lt.stamped;
    // the kernel of the latest timed launch (the layer-1 forward has two instances:
    // with the deferred update pending, and without, at a run's first step)
    tm.kernel = demangle(lt.kernel);
    ++tm.n;
}

}  // namespace gs

void gs_trainer::Timer::drop_events() {
    for (auto* evs : {&ev0, &ev1}) {
        for (hipEvent_t e : *evs)
            if (e) (void)hipEventDestroy(e);
        evs->clear();
    }
}

void gs_trainer::Timer::reset(gs::DevArena& mem, int64_t capacity, bool with_stamps) {
    drop_events();
    n = 0;  // nothing is timed or read back until the new entries are complete
    if (st0) mem.release(std::exchange(st0, nullptr));
    st1 = nullptr;
    stamped.assign(capacity, 0);
    if (with_stamps && capacity > 0) {
        const int64_t words = capacity * gs::kStampBlocks;
        st0 = mem.alloc<unsigned long long>(2 * words);
        st1 = st0 + words;
        gs::hip_ok(hipMemset(st0, 0, 2 * words * sizeof(unsigned long long)), "hipMemset(timer stamps)");
    }
    ev0.assign(capacity, nullptr);
    ev1.assign(capacity, nullptr);
    for (int64_t i = 0; i < capacity; ++i) {
        gs::hip_ok(hipEventCreateWithFlags(&ev0[i], gs::timer_event_flags()), "hipEventCreate");
        gs::hip_ok(hipEventCreateWithFlags(&ev1[i], gs::timer_event_flags()), "hipEventCreate");
    }
    calls = 0;
    kernel.clear();
}

extern "C" {

int gs_trainer_time_kernels(gs_trainer* t, int32_t site_mask, int64_t capacity) {
    return gs_trainer_time_kernels_every(t, site_mask, capacity, 1);
}

int gs_trainer_time_kernels_every(gs_trainer* t, int32_t site_mask, int64_t capacity, int64_t every) {
    GS_API_BEGIN
    GS_REQUIRE(t && capacity >= 0 && every >= 1, GS_EINVAL, "bad arguments");
    for (int s = 0; s < gs_trainer::kSites; ++s) {
        // span stamps for the sites >= 1 (forward, dW, top, slab sum)
        t->timer[s].reset(t->mem, (site_mask >> s) & 1 ? capacity : 0, s >= 1);
        t->timer[s].every = every;
    }
    GS_API_END
}

int gs_trainer_time_agg(gs_trainer* t, int64_t capacity) { return gs_trainer_time_kernels(t, 1, capacity); }

// The stamps of a site's first n timed launches (kStampBlocks starts and ends
// each), once everything issued has finished.
static bool read_stamps(const gs_trainer::Timer& tm, int64_t n, std::vector<unsigned long long>& a,
                        std::vector<unsigned long long>& b) {
    const size_t words = static_cast<size_t>(n) * gs::kStampBlocks;
    a.resize(words);
    b.resize(words);
    return hipDeviceSynchronize() == hipSuccess &&
           hipMemcpy(a.data(), tm.st0, words * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess &&
           hipMemcpy(b.data(), tm.st1, words * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess;
}

int64_t gs_trainer_kernel_times(gs_trainer* t, int32_t site, float* ms, int64_t cap) {
    if (!t || !ms || site < 0 || site >= gs_trainer::kSites) return -1;
    auto& tm = t->timer[site];
    const int64_t n = std::min(cap, tm.n);
    std::vector<unsigned long long> a, b;
    const int64_t W = gs::kStampBlocks;
    if (tm.st0 && n > 0 && !read_stamps(tm, n, a, b)) return -1;
    for (int64_t i = 0; i < n; ++i) {
        if (tm.st0 && tm.stamped[i]) {  // the kernel's own span: min start .. max end, 100 MHz ticks
            unsigned long long lo = ~0ull, hi = 0;
            for (int64_t w = 0; w < W; ++w) {
                if (a[i * W + w]) lo = std::min(lo, a[i * W + w]);
                hi = std::max(hi, b[i * W + w]);
            }
            if (hi == 0 || lo == ~0ull || hi < lo) return -1;
            ms[i] = static_cast<float>(static_cast<double>(hi - lo) * 1e-5);
            continue;
        }
        if (hipEventSynchronize(tm.ev1[i]) != hipSuccess || hipEventElapsedTime(&ms[i], tm.ev0[i], tm.ev1[i]) != hipSuccess)
            return -1;
    }
    return n;
}

int64_t gs_trainer_kernel_stamps(gs_trainer* t, int32_t site, int64_t launch, uint64_t* start, uint64_t* end) {
    if (!t || !start || !end || site < 0 || site >= gs_trainer::kSites) return -1;
    auto& tm = t->timer[site];
    if (!tm.st0 || launch < 0 || launch >= tm.n) return 0;
    const int64_t W = gs::kStampBlocks;
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(start, tm.st0 + launch * W, W * 8, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(end, tm.st1 + launch * W, W * 8, hipMemcpyDeviceToHost) != hipSuccess)
        return -1;
    return W;
}

int64_t gs_trainer_kernel_block_stats(gs_trainer* t, int32_t site, float* us4, int64_t cap) {
    if (!t || !us4 || site < 0 || site >= gs_trainer::kSites) return -1;
    auto& tm = t->timer[site];
    const int64_t n = std::min(cap, tm.n);
    const int64_t W = gs::kStampBlocks;
    if (n <= 0) return 0;
    if (!tm.st0) {  // an event-timed site
        std::fill(us4, us4 + 4 * n, -1.f);
        return n;
    }
    std::vector<unsigned long long> a, b;
    if (!read_stamps(tm, n, a, b)) return -1;
    for (int64_t i = 0; i < n; ++i) {
        float* o = us4 + 4 * i;
        o[0] = o[1] = o[2] = o[3] = -1.f;
        if (!tm.stamped[i]) continue;
        unsigned long long lo = ~0ull, hi = 0, slo = ~0ull, shi = 0, dmax = 0;
        double dsum = 0;
        int64_t nb = 0;
        for (int64_t w = 0; w < W; ++w) {
            const unsigned long long s = a[i * W + w], e = b[i * W + w];
            if (!s || e < s) continue;  // a workgroup past the stamp table, or none
            lo = std::min(lo, s);
            hi = std::max(hi, e);
            slo = std::min(slo, s);
            shi = std::max(shi, s);
            dmax = std::max(dmax, e - s);
            dsum += static_cast<double>(e - s);
            ++nb;
        }
        if (!nb) continue;
        o[0] = static_cast<float>((hi - lo) * 1e-2);  // 100 MHz ticks -> us
        o[1] = static_cast<float>(dsum / nb * 1e-2);
        o[2] = static_cast<float>(dmax * 1e-2);
        o[3] = static_cast<float>((shi - slo) * 1e-2);
    }
    return n;
}

int64_t gs_trainer_agg_times(gs_trainer* t, float* ms, int64_t cap) { return gs_trainer_kernel_times(t, 0, ms, cap); }

const char* gs_trainer_kernel_name(const gs_trainer* t, int32_t site) {
    if (!t || site < 0 || site >= gs_trainer::kSites) return "";
    return t->timer[site].kernel.c_str();
}


}  // extern "C"
