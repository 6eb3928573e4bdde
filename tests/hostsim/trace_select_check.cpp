// trace_select_check.cpp -- stand-alone host program over ray_amd/csrc/trace_select.h: the whole table of which K2 / K3 kernel form a launch takes.
//
//   trace_select_check
//
// One line per combination of BVH width {0, 4, 8}, role {primary, secondary, hook}, the four combinations of the two count flags,
// RAYHIP_REFILL {0..4}, pool_scene, small_scene, direct (width 4 only: rayhip_ctx::direct() implies it), shadow_refill, hook_refill and
// tune_primary_waves / tune_shadow_waves in {0, 5}:
//   wide W role R cw B ct B refill M pool B small B direct B srefill B hrefill B pw N sw N k2 <ClosestForm> k3 <ShadowForm>
// tests/test_trace_select_host.py compiles and runs it and holds the rules the table has to obey.
#include <stdio.h>

#include "../../ray_amd/csrc/trace_select.h"

using namespace rt;

namespace {
const char *name(ClosestForm f) {
    switch (f) {
    case ClosestForm::Counted8: return "counted8";
    case ClosestForm::Counted4: return "counted4";
    case ClosestForm::Counted0: return "counted0";
    case ClosestForm::Plain8: return "plain8";
    case ClosestForm::Plain8Small: return "plain8small";
    case ClosestForm::Plain4: return "plain4";
    case ClosestForm::Plain4Small: return "plain4small";
    case ClosestForm::Plain0: return "plain0";
    case ClosestForm::Whole8: return "whole8";
    case ClosestForm::Whole4: return "whole4";
    case ClosestForm::Whole4Direct: return "whole4direct";
    case ClosestForm::Lane8: return "lane8";
    case ClosestForm::Lane4: return "lane4";
    case ClosestForm::Lane4Direct: return "lane4direct";
    case ClosestForm::Pooled: return "pooled";
    }
    return "?";
}
const char *name(ShadowForm f) {
    switch (f) {
    case ShadowForm::Counted8: return "counted8";
    case ShadowForm::Counted4: return "counted4";
    case ShadowForm::Counted0: return "counted0";
    case ShadowForm::Plain8: return "plain8";
    case ShadowForm::Plain8Small: return "plain8small";
    case ShadowForm::Plain4: return "plain4";
    case ShadowForm::Plain4Small: return "plain4small";
    case ShadowForm::Plain0: return "plain0";
    case ShadowForm::Refill: return "refill";
    case ShadowForm::RefillDirect: return "refilldirect";
    }
    return "?";
}
} // namespace

int main() {
    const int widths[3] = {0, 4, 8};
    const TraceRole roles[3] = {TraceRole::Primary, TraceRole::Secondary, TraceRole::Hook};
    const char *role_names[3] = {"primary", "secondary", "hook"};
    for (const int wide : widths) {
        for (int r = 0; r < 3; ++r) {
            for (int fl = 0; fl < 4; ++fl) {
                const bool cw = (fl & 1) != 0, ct = (fl & 2) != 0;
                const uint32_t flags = (cw ? uint32_t(RAYHIP_FLAG_COUNT_WIDE) : 0u) | (ct ? uint32_t(RAYHIP_FLAG_COUNT_TRAVERSAL) : 0u);
                for (int mode = 0; mode <= 4; ++mode) {
                    for (int bits = 0; bits < 128; ++bits) {
                        const bool pool = bits & 1, small = bits & 2, direct = bits & 4, srefill = bits & 8, hrefill = bits & 16;
                        const int pw = (bits & 32) ? 5 : 0, sw = (bits & 64) ? 5 : 0;
                        if (direct && wide != 4) {
                            continue;
                        }
                        TraceConfig t;
                        if (mode != 0) { // (as init_trace_config: the grids are whatever the device holds, not 0)
                            t.refill_waves = 4096, t.refill_resident = t.refill_resident4 = 256;
                            set_refill_mode(t, mode);
                            if (t.refill_pool) {
                                t.pool_waves = 4096, t.pool_resident = 256;
                            }
                        }
                        t.pool_scene = pool, t.small_scene = small, t.shadow_refill = srefill;
                        t.tune_primary_waves = pw, t.tune_shadow_waves = sw;
                        t.direct_scene = direct;
                        printf("wide %d role %s cw %d ct %d refill %d pool %d small %d direct %d srefill %d hrefill %d pw %d sw %d k2 %s k3 %s\n", wide,
                               role_names[r], int(cw), int(ct), mode, int(pool), int(small), int(direct), int(srefill), int(hrefill), pw, sw,
                               name(closest_form(t, wide, direct, roles[r], flags)), name(shadow_form(t, wide, direct, roles[r], flags, hrefill)));
                    }
                }
            }
        }
    }
    return 0;
}
