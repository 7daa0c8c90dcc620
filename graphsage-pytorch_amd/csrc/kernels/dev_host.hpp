// Host-side plumbing shared by the handles that own device memory (the two
// device samplers, dsample.hip and fsample.hip, UnsupDev, unsup_ball.hip, the
// trainer, trainer.hpp, and the runner, runner.hip): an owning device arena,
// the ring of per-run results and the layout report.
// Included by .hip files only.
//
// Destruction: an owner's destructor body waits for its outstanding work and
// destroys its own streams and events; its DevArena / RunRing members free
// their memory afterwards, as members are destroyed after the body.  The
// trainer has no work of its own to wait for (its launches go to its callers'
// streams, and hipFree waits for the device): its timers destroy their events
// as members, before the arena declared ahead of them frees.
#pragma once

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "kcommon.hpp"

namespace gs {

// Device allocations freed together.  `label` names the owner in error strings;
// a refused allocation fails with `alloc_status` (GS_ENOMEM where the owner's
// callers expect out-of-memory as such).
struct DevArena {
    explicit DevArena(const char* label, int alloc_status = GS_EHIP) : label_(label), alloc_status_(alloc_status) {}
    DevArena(const DevArena&) = delete;
    DevArena& operator=(const DevArena&) = delete;
    ~DevArena() {
        for (void* p : owned_) (void)hipFree(p);
    }

    template <typename T>
    T* alloc(int64_t n) {
        void* p = nullptr;
        const hipError_t e = hipMalloc(&p, std::max<int64_t>(n, 1) * sizeof(T));
        if (e != hipSuccess) {
            // reported here, once: not again by the next check_launch on this thread
            (void)hipGetLastError();
            fail(alloc_status_, what("hipMalloc") + ": " + hipGetErrorString(e));
        }
        owned_.push_back(p);
        return static_cast<T*>(p);
    }
    // A device copy of `bytes` bytes at `src` (synchronous).
    void* upload(const void* src, size_t bytes) {
        void* p = alloc<uint8_t>(static_cast<int64_t>(bytes));
        if (bytes) hip_ok(hipMemcpy(p, src, bytes, hipMemcpyHostToDevice), what("hipMemcpy").c_str());
        return p;
    }
    // Frees one allocation now; the caller knows that no launch still uses it.
    void release(void* p) {
        owned_.erase(std::remove(owned_.begin(), owned_.end(), p), owned_.end());
        hip_ok(hipFree(p), what("hipFree").c_str());
    }

  private:
    std::string what(const char* call) const { return std::string(call) + "(" + label_ + ")"; }
    const char* label_;
    const int alloc_status_;
    std::vector<void*> owned_;
};

constexpr int kResSlots = 4;  // runs whose results are kept (gs_dsampler_result_of)

// The control blocks of a sampler's last kResSlots runs: run i's is copied
// into pinned slot i % kResSlots at the run's end, with an event behind it.
template <typename CtlT>
struct RunRing {
    RunRing() {
        hip_ok(hipHostMalloc(reinterpret_cast<void**>(&host_), kResSlots * sizeof(CtlT), hipHostMallocDefault),
               "hipHostMalloc");
        std::memset(host_, 0, kResSlots * sizeof(CtlT));
        try {
            for (hipEvent_t& e : done_) hip_ok(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate");
        } catch (...) {
            free_all();
            throw;
        }
    }
    RunRing(const RunRing&) = delete;
    RunRing& operator=(const RunRing&) = delete;
    ~RunRing() { free_all(); }

    // The end of a run on `st`: its control block into the next slot.
    void record(const CtlT* dev_ctl, hipStream_t st) {
        const int slot = static_cast<int>(n_runs_ % kResSlots);
        hip_ok(hipMemcpyAsync(host_ + slot, dev_ctl, sizeof(CtlT), hipMemcpyDeviceToHost, st), "hipMemcpyAsync(ctl)");
        hip_ok(hipEventRecord(done_[slot], st), "hipEventRecord");
        ++n_runs_;
    }
    int64_t runs() const { return n_runs_; }
    // Whether run number `run` has finished (no wait); a run older than the ring has.
    bool ready(int64_t run) const {
        if (run < 0 || run < n_runs_ - kResSlots) return true;
        if (run >= n_runs_) return false;
        const hipError_t e = hipEventQuery(done_[run % kResSlots]);
        if (e == hipErrorNotReady) return false;
        hip_ok(e, "hipEventQuery(device sampler run)");
        return true;
    }
    // Waits for run number `run` (run < 0: the last run) and returns its control block.
    const CtlT& wait(int64_t run) const {
        if (run < 0) {
            if (!n_runs_) fail(GS_EINVAL, "no run to report");
            run = n_runs_ - 1;
        }
        if (run >= n_runs_ || run < n_runs_ - kResSlots)
            fail(GS_ERANGE, "device sampler: run not issued or no longer kept (the last " + std::to_string(kResSlots) +
                                " runs are)");
        const int slot = static_cast<int>(run % kResSlots);
        hip_ok(hipEventSynchronize(done_[slot]), "hipEventSynchronize");
        return host_[slot];
    }
    // Waits for the last run, if there was one.  Returns the wait's status, for
    // hip_ok, or for a destructor to ignore.
    hipError_t wait_last_if_any() const {
        return n_runs_ ? hipEventSynchronize(done_[(n_runs_ - 1) % kResSlots]) : hipSuccess;
    }

  private:
    void free_all() {
        for (hipEvent_t e : done_)
            if (e) (void)hipEventDestroy(e);
        (void)hipHostFree(host_);
    }
    CtlT* host_ = nullptr;
    hipEvent_t done_[kResSlots] = {};
    int64_t n_runs_ = 0;
};

// The layout of the run whose control block is `c`, as the host sampler reports it.
template <typename CtlT>
void report_layout(const CtlT& c, int n_hops, int64_t* hop_sizes, int64_t* offsets, int64_t* used) {
    for (int32_t j = 0; j < GS_MAX_HOPS; ++j) {
        const bool on = j < n_hops;
        const bool last = j == n_hops - 1;
        if (hop_sizes) {
            hop_sizes[4 * j] = on ? c.hop[j].n_dst : 0;
            hop_sizes[4 * j + 1] = on ? c.hop[j].n_pos : 0;
            // as the host sampler: -1 = not materialised (the last hop), 0 past the hops
            hop_sizes[4 * j + 2] = on ? (last ? -1 : c.hop[j].n_src) : 0;
            hop_sizes[4 * j + 3] = on ? (last ? -1 : c.hop[j].n_nbr) : 0;
        }
        if (offsets)
            for (int f = 0; f < GS_PK_NFIELDS; ++f) {
                const bool lastf = f == GS_PK_POS_PTR || f == GS_PK_POS || f == GS_PK_DST_IDS;
                offsets[j * GS_PK_NFIELDS + f] = on && (last == lastf) ? c.hop[j].off[f] : -1;
            }
    }
    if (used) *used = c.used;
}

}  // namespace gs
