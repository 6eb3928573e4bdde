// trace_select.h -- which instantiation of the closest-hit kernel (K2) and of the shadow-ray kernel (K3) a launch takes.
//
// One pure function per stage over the knobs of TraceConfig: the passes (rayhip_render.hip.h), the kernel-level hooks
// (rayhip_hooks.hip.h) and the reports (rayhip_closest_hit_form, rayhip_direct_entry) all ask it, and rayhip_trace.hip.h launches what it
// names.  A new kernel form is added here and in that launcher, nowhere else.  No HIP in this header: tests/hostsim/trace_select_check.cpp
// compiles it with the host compiler and prints the whole table (tests/test_trace_select_host.py).
#pragma once

#include <stdint.h>

#include "../../include/rayhip.h" // RAYHIP_FLAG_COUNT_*

namespace rt {

// The knobs the choice and the grids of K2 / K3 read.  Set once per context from the environment (init_trace_config, rayhip_ctx.hip.h) but
// for the two that describe the scene in place, which every upload / instance update sets:
//   RAYHIP_REFILL           0: refill_waves = 0 (the plain K2 everywhere)   1: lane refill on every bounce
//                           2: + refill_secondary_only   3 (default): + refill_primary_whole   4: + refill_pool
//   RAYHIP_REFILL_MULT      blocks per resident wave slot in refill_waves / pool_waves (default 16)
//   RAYHIP_DIRECT_ENTRY     direct_entry
//   RAYHIP_SHADOW_REFILL    shadow_refill
//   RAYHIP_PRIMARY_WAVES    tune_primary_waves          RAYHIP_SHADOW_WAVES    tune_shadow_waves
//   RAYHIP_OVERLAP_SHADOW   overlap_shadow
//   the upload              pool_scene, direct_scene (refresh_top_level_view), small_scene (upload_bottom_level)
struct TraceConfig {
    int refill_waves = 0;     // largest grid of the persistent closest-hit kernel (blocks); 0 = kernel switched off
    int refill_resident = 0;  // ... and the number of its blocks the device holds at once
    int refill_resident4 = 0; // ... of its 4-wide form (the grid of a launch whose chunks are handed out dynamically)
    bool refill_secondary_only = false; // primary rays (coherent, every lane busy to the end) do not refill lane by lane ...
    bool refill_primary_whole = false;  // ... but take the flat kernel with whole-chunk refills (no spill stores in the walk)
    bool refill_pool = false;           // the secondary bounces of 4-wide scenes go through the pooled kernel (k_trace_closest_pool)
    int pool_waves = 0, pool_resident = 0; // its grid
    bool pool_scene = false;               // ... and whether the scene in place suits it
    bool shadow_refill = true; // K3 as the flat persistent kernel (4-wide walk); false: the nested form
    int shadow_resident = 0;   // blocks of k_trace_shadow_refill the device holds at once
    // register footprint of the plain K2 (primary rays) / of K3.  K3 runs at 5 waves per SIMD (96 VGPRs, 32 spilled registers per ray
    // instead of 51 at 6 waves: same time, a third less scratch traffic)
    int tune_primary_waves = 0, tune_shadow_waves = 5;
    bool small_scene = false;  // BLAS nodes + triangles fit one XCD's L2: traversal kernels with the smaller register footprint
    bool direct_entry = true;  // false: one-instance scenes walk their top level like any other (kernels_closest_refill.hip.h: DIRECT)
    bool direct_scene = false; // ... whether the scene in place has ONE instance over the 4-wide tree, SceneView::direct filled
    bool overlap_shadow = true; // K3 of a bounce on the second stream, beside K2 of the next (rayhip_ctx: stream2)
};

// what RAYHIP_REFILL = `mode` (not 0) switches on; the grids (refill_waves ..., not 0 from here on) come from the device
inline void set_refill_mode(TraceConfig &t, const int mode) {
    t.refill_secondary_only = mode == 2 || mode == 3 || mode == 4;
    t.refill_primary_whole = mode == 3 || mode == 4;
    t.refill_pool = mode == 4;
}

// the instantiations of k_trace_closest /k_trace_closest_refill / k_trace_closest_pool in the code object, once each
enum class ClosestForm {
    Counted8, Counted4, Counted0,                      // k_trace_closest<true, W>
    Plain8, Plain8Small, Plain4, Plain4Small, Plain0,  // k_trace_closest<false, W[, RT_TRACE_SMALL_WAVES]>
    Whole8, Whole4, Whole4Direct,                      // k_trace_closest_refill<W, WAVE[, true]>: chunks taken whole
    Lane8, Lane4, Lane4Direct,                         // k_trace_closest_refill<W[, RT_REFILL_MIN_DIRECT, true]>: lanes refill one by one
    Pooled,                                            // k_trace_closest_pool<>
};
// ... and of k_trace_shadow / k_trace_shadow_refill
enum class ShadowForm {
    Counted8, Counted4, Counted0,                     // k_trace_shadow<true, W>
    Plain8, Plain8Small, Plain4, Plain4Small, Plain0, // k_trace_shadow<false, W[, RT_TRACE_SMALL_WAVES]>
    Refill, RefillDirect,                             // k_trace_shadow_refill<[RT_SHADOW_REFILL_MIN_DIRECT, true]>
};

// who launches: a pass on the rays the generator wrote (init_hits == 0), a pass on a later bounce (init_hits != 0), a kernel-level hook
enum class TraceRole { Primary, Secondary, Hook };

inline bool is_whole(ClosestForm f) { return f == ClosestForm::Whole8 || f == ClosestForm::Whole4 || f == ClosestForm::Whole4Direct; }
inline bool is_lane(ClosestForm f) { return f == ClosestForm::Lane8 || f == ClosestForm::Lane4 || f == ClosestForm::Lane4Direct; }
inline bool is_direct(ClosestForm f) { return f == ClosestForm::Whole4Direct || f == ClosestForm::Lane4Direct; }
inline bool is_refill(ShadowForm f) { return f == ShadowForm::Refill || f == ShadowForm::RefillDirect; }
inline bool is_direct(ShadowForm f) { return f == ShadowForm::RefillDirect; }

// K2.  `wide`: the BLAS form the scene was uploaded with (8, 4, or 0 = the reference's BVH2); `direct`: rayhip_ctx::direct();
// `flags`: the RAYHIP_FLAG_* of the call.
inline ClosestForm closest_form(const TraceConfig &t, const int wide, const bool direct, const TraceRole role, const uint32_t flags) {
    const bool hook = role == TraceRole::Hook, primary = role == TraceRole::Primary;
    const bool count_wide = (flags & RAYHIP_FLAG_COUNT_WIDE) != 0;
    // pass / hook: in a pass COUNT_WIDE masks COUNT_TRAVERSAL (a BVH2 scene with both set runs uncounted); the hook reads the raw bit
    const bool count = (flags & RAYHIP_FLAG_COUNT_TRAVERSAL) != 0 && (hook || !count_wide);
    if (count_wide && wide == 8) {
        return ClosestForm::Counted8;
    }
    if (count_wide && wide == 4) {
        return ClosestForm::Counted4;
    }
    if (count) {
        return ClosestForm::Counted0; // (whatever the width: the instrumented walk of the reference's BVH2)
    }
    const bool refill = wide != 0 && t.refill_waves != 0;
    // pass / hook: the hook never takes its chunks whole (it ignores refill_primary_whole)
    if (!hook && primary && refill && t.refill_primary_whole) {
        return wide == 8 ? ClosestForm::Whole8 : direct ? ClosestForm::Whole4Direct : ClosestForm::Whole4;
    }
    // pass / hook: a pass pools the secondary bounces only; the hook pools its rays although it launches with init_hits == 0
    if (!primary && wide == 4 && t.refill_pool && t.pool_scene) {
        return ClosestForm::Pooled;
    }
    // pass / hook: the hook ignores refill_secondary_only (in a pass RAYHIP_REFILL=2 keeps the plain kernel for primary rays)
    if (refill && !(primary && t.refill_secondary_only)) {
        return wide == 8 ? ClosestForm::Lane8 : direct ? ClosestForm::Lane4Direct : ClosestForm::Lane4;
    }
    // pass / hook: the hook never takes the small-footprint forms (it ignores small_scene and RAYHIP_PRIMARY_WAVES)
    const bool small = !hook && (t.small_scene || t.tune_primary_waves == 5);
    if (wide == 8) {
        return small ? ClosestForm::Plain8Small : ClosestForm::Plain8;
    }
    if (wide == 4) {
        return small ? ClosestForm::Plain4Small : ClosestForm::Plain4;
    }
    return ClosestForm::Plain0;
}

// K3.  `hook_refill`: RAYHIP_HOOK_SHADOW_REFILL is set at this call of the hook (read per call, not per context); passes ignore it.
inline ShadowForm shadow_form(const TraceConfig &t, const int wide, const bool direct, const TraceRole role, const uint32_t flags,
                              const bool hook_refill) {
    if (role == TraceRole::Hook) {
        // pass / hook: the hook takes the persistent form on request only, whatever shadow_refill says, ...
        if (hook_refill && wide == 4) {
            return direct ? ShadowForm::RefillDirect : ShadowForm::Refill;
        }
        // ... and otherwise always the instrumented BVH2 walk, whatever the width and the flags (its counters are the hook's output)
        return ShadowForm::Counted0;
    }
    const bool count_wide = (flags & RAYHIP_FLAG_COUNT_WIDE) != 0;
    const bool count = !count_wide && (flags & RAYHIP_FLAG_COUNT_TRAVERSAL) != 0;
    if (count_wide && wide == 8) {
        return ShadowForm::Counted8;
    }
    if (count_wide && wide == 4) {
        return ShadowForm::Counted4;
    }
    if (count) {
        return ShadowForm::Counted0;
    }
    if (wide == 4 && t.shadow_refill) {
        return direct ? ShadowForm::RefillDirect : ShadowForm::Refill;
    }
    const bool small = t.small_scene || t.tune_shadow_waves == 5; // (RAYHIP_SHADOW_WAVES defaults to 5: small is the default)
    if (wide == 8) {
        return small ? ShadowForm::Plain8Small : ShadowForm::Plain8;
    }
    if (wide == 4) {
        return small ? ShadowForm::Plain4Small : ShadowForm::Plain4;
    }
    return ShadowForm::Plain0;
}

} // namespace rt
