// rayhip_trace.hip.h -- part of librayhip's host side (one translation unit: included by rayhip.hip, in this order, after the kernels):
// the launch sites of the closest-hit kernel (K2) and the shadow-ray kernel (K3).  trace_select.h names a form, the caller (a pass, a hook)
// sizes the grid and picks the stream and the spill slab for its role, and every instantiation is written once, here.
#pragma once

#include "trace_select.h"

// what a K2 launch reads and writes
struct ClosestLaunch {
    SceneView sc;
    TraceParams tp;
    RaySoA rays;
    HitSoA hits;
    RayQueue queue;
    int init_hits = 0;
    uint32_t *spill = nullptr;              // the overflow slabs of the traversal stack the launch may use
    unsigned long long *counters = nullptr; // the counted and the plain forms: TRAV_COUNTER_WORDS traversal counters
    Layering layers;
    uint32_t *work = nullptr; // the lane-refill forms: zeroed counter of the dynamic chunk hand-out (wavefront.hip.h), or null
};

static void launch_closest(const ClosestForm form, const int grid, hipStream_t s, const ClosestLaunch &a) {
#define PLAIN_ARGS a.sc, a.tp, a.rays, a.hits, a.queue, a.init_hits, a.spill, a.counters, a.layers
#define REFILL_ARGS a.sc, a.tp, a.rays, a.hits, a.queue, a.init_hits, a.spill, a.layers
    switch (form) {
    case ClosestForm::Counted8: k_trace_closest<true, 8><<<grid, WAVE, 0, s>>>(PLAIN_ARGS); break;
    case ClosestForm::Counted4: k_trace_closest<true, 4><<<grid, WAVE, 0, s>>>(PLAIN_ARGS); break;
    case ClosestForm::Counted0: k_trace_closest<true, 0><<<grid, WAVE, 0, s>>>(PLAIN_ARGS); break;
    case ClosestForm::Plain8: k_trace_closest<false, 8><<<grid, WAVE, 0, s>>>(PLAIN_ARGS); break;
    case ClosestForm::Plain8Small: k_trace_closest<false, 8, RT_TRACE_SMALL_WAVES><<<grid, WAVE, 0, s>>>(PLAIN_ARGS); break;
    case ClosestForm::Plain4: k_trace_closest<false, 4><<<grid, WAVE, 0, s>>>(PLAIN_ARGS); break;
    case ClosestForm::Plain4Small: k_trace_closest<false, 4, RT_TRACE_SMALL_WAVES><<<grid, WAVE, 0, s>>>(PLAIN_ARGS); break;
    case ClosestForm::Plain0: k_trace_closest<false, 0><<<grid, WAVE, 0, s>>>(PLAIN_ARGS); break;
    // chunks taken whole (static walk: such a launch takes a chunk every ~8 ns chip-wide, more than one counter can hand out -- wavefront.hip.h)
    case ClosestForm::Whole8: k_trace_closest_refill<8, WAVE><<<grid, WAVE, 0, s>>>(REFILL_ARGS, nullptr); break;
    case ClosestForm::Whole4: k_trace_closest_refill<4, WAVE><<<grid, WAVE, 0, s>>>(REFILL_ARGS, nullptr); break;
    // (direct: one instance, entered from the kernel arguments -- kernels_closest_refill.hip.h: DIRECT)
    case ClosestForm::Whole4Direct: k_trace_closest_refill<4, WAVE, true><<<grid, WAVE, 0, s>>>(REFILL_ARGS, nullptr); break;
    case ClosestForm::Lane8: k_trace_closest_refill<8><<<grid, WAVE, 0, s>>>(REFILL_ARGS, a.work); break;
    case ClosestForm::Lane4: k_trace_closest_refill<4><<<grid, WAVE, 0, s>>>(REFILL_ARGS, a.work); break;
    case ClosestForm::Lane4Direct: k_trace_closest_refill<4, RT_REFILL_MIN_DIRECT, true><<<grid, WAVE, 0, s>>>(REFILL_ARGS, a.work); break;
    case ClosestForm::Pooled: k_trace_closest_pool<><<<grid, WAVE, 0, s>>>(REFILL_ARGS); break;
    }
#undef PLAIN_ARGS
#undef REFILL_ARGS
}

// what a K3 launch reads and writes
struct ShadowLaunch {
    SceneView sc;
    TraceParams tp;
    ShadowSoA shadow;
    RayQueue queue;
    float limit = 0.0f;      // clamp of a ray's contribution
    int pitch = 0;           // row pitch of `temp`
    float4 *temp = nullptr;  // the per-iteration pixel buffer the contributions are added to ...
    float4 *out_rc = nullptr; // ... or, for the hook, the plane they are written to by ray
    uint32_t *spill = nullptr;
    unsigned long long *counters = nullptr; // the counted and the plain forms
    Layering layers;
    uint32_t *work = nullptr; // the refill forms: as ClosestLaunch::work
};

static void launch_shadow(const ShadowForm form, const int grid, hipStream_t s, const ShadowLaunch &a) {
#define PLAIN_ARGS a.sc, a.tp, a.shadow, a.queue, a.limit, a.pitch, a.temp, a.out_rc, a.spill, a.counters, a.layers
#define REFILL_ARGS a.sc, a.tp, a.shadow, a.queue, a.limit, a.pitch, a.temp, a.out_rc, a.spill, a.layers, a.work
    switch (form) {
    case ShadowForm::Counted8: k_trace_shadow<true, 8><<<grid, WAVE, 0, s>>>(PLAIN_ARGS); break;
    case ShadowForm::Counted4: k_trace_shadow<true, 4><<<grid, WAVE, 0, s>>>(PLAIN_ARGS); break;
    case ShadowForm::Counted0: k_trace_shadow<true, 0><<<grid, WAVE, 0, s>>>(PLAIN_ARGS); break;
    case ShadowForm::Plain8: k_trace_shadow<false, 8><<<grid, WAVE, 0, s>>>(PLAIN_ARGS); break;
    case ShadowForm::Plain8Small: k_trace_shadow<false, 8, RT_TRACE_SMALL_WAVES><<<grid, WAVE, 0, s>>>(PLAIN_ARGS); break;
    case ShadowForm::Plain4: k_trace_shadow<false, 4><<<grid, WAVE, 0, s>>>(PLAIN_ARGS); break;
    case ShadowForm::Plain4Small: k_trace_shadow<false, 4, RT_TRACE_SMALL_WAVES><<<grid, WAVE, 0, s>>>(PLAIN_ARGS); break;
    case ShadowForm::Plain0: k_trace_shadow<false, 0><<<grid, WAVE, 0, s>>>(PLAIN_ARGS); break;
    // the flat persistent form (kernels_shadow.hip.h); direct: one instance, entered from the kernel arguments
    case ShadowForm::Refill: k_trace_shadow_refill<><<<grid, WAVE, 0, s>>>(REFILL_ARGS); break;
    case ShadowForm::RefillDirect: k_trace_shadow_refill<RT_SHADOW_REFILL_MIN_DIRECT, true><<<grid, WAVE, 0, s>>>(REFILL_ARGS); break;
    }
#undef PLAIN_ARGS
#undef REFILL_ARGS
}
