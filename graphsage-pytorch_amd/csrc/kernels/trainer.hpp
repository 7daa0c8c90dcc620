#pragma once
// The native trainer's state (gs_trainer) and what its translation units
// share: step.hip (the step itself), step_update.hip (the deferred update and
// the optimiser entry points) and step_timer.hip (the launch timers).
#include <string>
#include <vector>

#include "dev_host.hpp"
#include "internal.hpp"

struct gs_trainer {
    gs_trainer_config cfg;
    // every device buffer of the handle; declared ahead of the timers, so
    // freed after they have destroyed their events (dev_host.hpp)
    gs::DevArena mem{"trainer", GS_ENOMEM};
    std::vector<int64_t> w_off;  // element offset of each parameter in the flat buffer
    std::vector<int64_t> w_rows, w_cols;
    int64_t cls_w_off = 0, cls_b_off = 0, total = 0;
    // optional kernel-bound HIP-event timing (bench roofline): site 0 the
    // layer-1 gather-aggregate, 1 the layer-1 linear forward, 2 its weight
    // gradient (the MFMA kernels), 3 the fused top layer + loss head (top.hip),
    // 4 the step's slab-sum pair launch (sum_slabs_pair_launch)
    static constexpr int kSites = 5;
    struct Timer {
        std::vector<hipEvent_t> ev0, ev1;
        int64_t n = 0;
        int64_t every = 1, calls = 0;  // time one launch of every `every`, the last of each run
        std::string kernel;  // demangled name of the kernel the site last timed
        // sites 1-4: the kernel's own span (KStamp, kcommon.hpp) per entry,
        // when the launch took it (else the entry's events timed it)
        unsigned long long* st0 = nullptr;  // device: per entry, kStampBlocks workgroup starts (100 MHz ticks)
        unsigned long long* st1 = nullptr;  // device: per entry, the workgroup ends
        std::vector<char> stamped;
        // Room for `capacity` timed launches from now on (0: the site is off),
        // with span stamps from `mem` when asked; what the site held goes first.
        void reset(gs::DevArena& mem, int64_t capacity, bool with_stamps);
        Timer() = default;
        Timer(const Timer&) = delete;
        Timer& operator=(const Timer&) = delete;
        ~Timer() { drop_events(); }  // (the stamps are the arena's)

      private:
        void drop_events();
    } timer[kSites];
    // One layer-1 aggregate slot for a gather issued ahead of its step
    // (gs_trainer_gather), so the next batch's gather overlaps this backward,
    // and what is resolved on the side stream with that gather.
    struct GatherSlot {
        // a1_rows rows: the aggregate, or [self | agg] rows of 2F (self_rows below)
        void* a1 = nullptr;
        bool self_in = false;  // the self half was written
        // the layer-1 neighbour ids resolved ahead of the gather (k_ids slots
        // per destination), when reserved with a fanout
        int32_t* ids = nullptr;
        // padded hop-1 records for the fused top launch (trainer_reserve_top: top_rows roots, top_k each)
        int32_t* top = nullptr;
        bool top_ready = false;
        // the layer-2 backward's records of the transposed hop-1 lists (8 ints
        // per layer-1 row, rec_rows rows; written with the top records)
        int32_t* rec = nullptr;
        bool rec_ready = false;
    };
    static constexpr int kSlots = 3;
    GatherSlot slot[kSlots];
    // What the slots' buffers were reserved for; 0 from a reserve's first free
    // to its last allocation, so also after a refused one.
    int64_t a1_rows = 0, top_rows = 0, rec_rows = 0;
    int k_ids = 0, top_k = 0;
    // [self | agg] slots (option GS_TOPT_SELF_ROWS, default on; applied at
    // gs_trainer_gather_reserve): the side-stream gather also copies the
    // layer-1 rows' own features, so the layer-1 forward and dW read one dense
    // block (no self-index round).
    bool self_rows = false;
    // clip-norm partials produced by the fused backward's reduce launches
    // (group 0: the sage weights' slab sums, group 1: the classifier reduce),
    // consumed by gs_trainer_update_local when no all-reduce came between
    // gs_trainer_set_option switches (alternatives the tests compare with the
    // default: bitwise, except top_launch, which matches within fp32 rounding)
    bool fuse_bwd = true;    // GS_TOPT_FUSED_BWD: layers >= 2 backward in fused launches
    bool use_top = true;     // GS_TOPT_TOP_LAUNCH: layer 2 + loss head + dIn2 in one launch
    bool want_self_rows = true;  // GS_TOPT_SELF_ROWS
    bool opt_defer = true;   // GS_TOPT_DEFER_UPDATE: runner loops defer each clip + SGD
    float* norm_part = nullptr;
    int pstride = 0;
    int npart[2] = {0, 0};
    bool norm_ready = false;
    std::function<void(hipStream_t)> upper_hook;  // internal.hpp trainer_set_upper_hook
    std::function<void(hipStream_t, int64_t, int64_t)> w1_chunk_hook;  // trainer_set_w1_chunk_hook
    int w1_chunks = 1;
    // bf16 features: W1 in bf16 for the layer-1 forward.  Cast from the fp32
    // W1 before a forward, except inside a runner loop (lp_keep), where the
    // SGD launch writes it beside W1 (lowp_shadow below) and it stays valid from
    // one step to the next: nothing else writes the parameters there.
    uint16_t* w1_lp = nullptr;
    bool lp_keep = false, lp_valid = false;
    // Deferred update (trainer_defer_update, runner loops without an
    // all-reduce): a step's clip + SGD is not a launch of its own.  The step's
    // last slab sum writes W1's update for clip coefficient 1 into the other
    // W1 buffer, and the next step's layer-1 forward applies the pending
    // update (FwdSpec, kcommon.hpp): W1 from that buffer (or recomputed there
    // when the coefficient is not 1), the other parameters in its prologue.
    // The current W1 lives in w1_buf(w1_cur): buffer 0 is its place in the
    // flat params, buffer 1 w1_alt; trainer_defer_update(false) puts the
    // result of the last pending update back into the flat params.
    bool defer = false, pending = false;
    bool defer_comm = false;  // the all-reduce path: gs_trainer_update leaves the update pending
    // the pending update's norm partials (the step's own, or gs_trainer_update's
    // after the all-reduce), per-group counts and stride, gradient scale
    const float* pend_part = nullptr;
    int pend_pstride = 0;
    int pend_np[2] = {0, 0};
    float pend_scale = 1.f;
    float* w1_alt = nullptr;
    int w1_cur = 0;
    float* w1_buf(int i) { return i == 0 ? cfg.params + w_off[0] : w1_alt; }
    // bf16 features: the forward's bf16 W1 beside each buffer (lp_buf(w1_cur)
    // is current while deferring: the slab sum and the recompute write both)
    uint16_t* w1_lp_alt = nullptr;
    uint16_t* lp_buf(int i) { return i == 0 ? w1_lp : w1_lp_alt; }
    // Parity capture (gs_trainer_capture; tests only): after each training
    // step's launches, the step's root embeddings (the top layer's output) and
    // the flat gradient as the step left it (before its clip + SGD) are copied
    // on the step's stream into caller buffers.
    struct Capture {
        float* emb = nullptr;
        int64_t emb_stride = 0;
        float* grads = nullptr;
        int64_t max_steps = 0, n = 0;
    } cap;
    const float* last_emb = nullptr;  // the last run_step's [B, H] top-layer output
    // The optimiser of gs_trainer_update[_local] (gs_trainer_set_optimizer):
    // clip + SGD, or clip + Adam on the caller's moment buffers, opt.step
    // counting the updates applied to them.  Adam never defers (the deferred
    // update's speculation is sgd_elem): every update is a launch of its own.
    gs_optimizer_config opt{GS_OPT_SGD, 0.9f, 0.999f, 1e-8f, 0.f, nullptr, nullptr, 0};
    // the runner's step-completion flag (trainer_set_done), until the launch that stores it is issued
    gs::DoneFlag done;
    gs::DoneFlag take_done() {
        const gs::DoneFlag d = done;
        done = {};
        return d;
    }
};

namespace gs {

using GatherSlot = gs_trainer::GatherSlot;

// Bump allocator over the workspace (256-byte aligned carves).
struct Carve {
    char* base;
    int64_t cap, at = 0;
    template <class T>
    T* take(int64_t n) {
        at = (at + 255) & ~int64_t(255);
        T* p = base ? reinterpret_cast<T*>(base + at) : nullptr;
        at += n * static_cast<int64_t>(sizeof(T));
        return p;
    }
};

// step_timer.hip.  The timer of site `site`'s next entry when the site has
// capacity left and this call is one it times, else an empty one (which times
// nothing): pass it to the launch, then to timed_done.
LaunchTimer timed_arm(gs_trainer& T, int site);
void timed_done(gs_trainer& T, int site, const LaunchTimer& lt);

// step_update.hip.  The pending clip + SGD (gs_trainer::pending) as the launch
// argument of whatever applies it: W1's speculative update S in the buffer that
// is not current, the norm partials and the other parameters' range.  The
// layer-1 forward adds its recompute buffers (Wn, S_lp, Wn_lp).
FwdSpec pending_spec(gs_trainer& T);

}  // namespace gs
