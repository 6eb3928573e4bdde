// light_pose.h -- moving and recolouring the ANALYTIC lights of the scene that is on the device (rayhip_scene_set_lights and its
// _device form): complete 64-byte records in, the leaf summaries of the light tree out; the tree itself is then refitted by
// light_refit.h, whose `posed` table makes the leaves of these lights take flux, axis and cosines from their summaries.  Element
// functions shared by the device kernels (light_pose.hip.h) and a plain-loop host driver (tests/hostsim/hostsim_light_pose.cpp), like
// instances.h: IEEE operations in a STATED ORDER without contraction on both sides, so both produce the same bits.
//
//   flux      the scene build's (SceneCPU.cpp, RebuildLightTree_nolock): lum = (col0 + col1) + col2; area = sph.area of a sphere or spot
//             light (1 where it is 0), (PI * r) * r with r = dir.tan_angle of a directional light (1 where r is 0), the record's area of
//             a line, rect or disk light; flux = lum * area.
//   summary   light_refit.h: static_light_summary (box, axis, angles, as the scene build computes them) plus that flux.
//
// A call names light slots; it is refused as a whole (nothing on the device written) when a named slot is outside the light array or
// not named by li_indices (a freed slot of the pool, a directional light baked into the physical sky), is named twice, holds or would
// get a triangle or environment light, would get another word 0 than it holds (type, doublesided, cast_shadow, visible, sky_portal,
// ray_visibility: the counts of visible and blocker lights and the choice of kernels hang on it), or gets a colour or parameter that is
// not finite.
#pragma once

#include <stdint.h>

#include "light_refit.h"

namespace rayhip_light_pose {

using namespace rt;
using rayhip_light_refit::Summary;

// the findings of a call, one counter each
enum { BAD_SLOT = 0, DUPLICATE = 1, BAD_TYPE = 2, FLAGS_CHANGED = 3, NOT_FINITE = 4, N_FINDINGS = 5 };

RT_HD bool finite_f(const float x) { return fabsf(x) <= 3.402823466e+38f; } // (false for NaN)

// the 15 floats of a record
RT_HD bool finite_record(const rayhip_light &l) {
    bool ok = finite_f(l.col[0]) && finite_f(l.col[1]) && finite_f(l.col[2]);
    for (int k = 0; k < 12; ++k) {
        ok = ok && finite_f(l.params[k]);
    }
    return ok;
}

// sphere / spot, directional, line, rect, disk: the lights whose summary is a function of their record alone
RT_HD bool analytic(const rayhip_light &l) { return light_type(l) <= uint32_t(LIGHT_TYPE_DISK); }

RT_HD float analytic_light_flux(const rayhip_light &l) {
    const float lum = (l.col[0] + l.col[1]) + l.col[2];
    const uint32_t type = light_type(l);
    float area = 1.0f;
    if (type == LIGHT_TYPE_DIR) {
        const float r = l.params[4];
        if (r != 0.0f) {
            area = (PI * r) * r;
        }
    } else if (type == LIGHT_TYPE_SPHERE) {
        if (l.params[3] != 0.0f) {
            area = l.params[3];
        }
    } else {
        area = l.params[3];
    }
    return lum * area;
}

RT_HD void analytic_light_summary(const rayhip_light &l, Summary &s) {
    rayhip_light_refit::static_light_summary(l, s);
    s.flux = analytic_light_flux(l);
}

// a slot a call may name: inside the light array and named by li_indices (`live`: one byte per slot)
RT_HD bool slot_ok(const uint32_t slot, const uint8_t *live, const uint32_t n_lights) { return slot < n_lights && live[slot] != 0; }

// what is wrong with the record `l` for a slot that holds `held`
RT_HD bool bad_type(const rayhip_light &held, const rayhip_light &l) { return !analytic(held) || !analytic(l); }
RT_HD bool flags_changed(const rayhip_light &held, const rayhip_light &l) { return held.flags != l.flags; }

// what the findings of a call mean: 0 = go on, 1 = refused
RT_HD int verdict(const uint32_t findings[N_FINDINGS]) {
    uint32_t any = 0;
    for (int k = 0; k < N_FINDINGS; ++k) {
        any |= findings[k];
    }
    return any != 0 ? 1 : 0;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
// `live` of a light array: the slots li_indices names
inline std::vector<uint8_t> live_table(const uint32_t *li_indices, const uint32_t n_li, const uint32_t n_lights) {
    std::vector<uint8_t> live(n_lights, 0);
    for (uint32_t k = 0; k < n_li; ++k) {
        if (li_indices[k] < n_lights) {
            live[li_indices[k]] = 1;
        }
    }
    return live;
}

// check, stage and commit as plain loops: `lights`, `leaf` and `posed` [n_lights] in place.  The findings are counted as the device
// counts them; the arrays are written only where verdict() is 0, which is returned.  The tree is the caller's to refit
// (refit_light_nodes_host with `posed`).
inline int pose_lights_host(rayhip_light *lights, const uint32_t n_lights, const uint8_t *live, uint8_t *posed, Summary *leaf, const uint32_t n,
                            const uint32_t *slots, const rayhip_light *records, uint32_t findings[N_FINDINGS]) {
    for (int k = 0; k < N_FINDINGS; ++k) {
        findings[k] = 0;
    }
    for (uint32_t i = 0; i < n; ++i) {
        findings[NOT_FINITE] += finite_record(records[i]) ? 0u : 1u;
        if (!slot_ok(slots[i], live, n_lights)) {
            findings[BAD_SLOT] += 1;
            continue;
        }
        for (uint32_t j = 0; j < i; ++j) {
            if (slots[j] == slots[i]) {
                findings[DUPLICATE] += 1;
                break;
            }
        }
        findings[BAD_TYPE] += bad_type(lights[slots[i]], records[i]) ? 1u : 0u;
        findings[FLAGS_CHANGED] += flags_changed(lights[slots[i]], records[i]) ? 1u : 0u;
    }
    const int rc = verdict(findings);
    for (uint32_t i = 0; rc == 0 && i < n; ++i) {
        lights[slots[i]] = records[i];
        analytic_light_summary(records[i], leaf[slots[i]]);
        posed[slots[i]] = 1;
    }
    return rc;
}

} // namespace rayhip_light_pose
