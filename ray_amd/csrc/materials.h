// materials.h -- changing the MATERIALS of the scene that is on the device (rayhip_scene_set_materials and its _device form): complete
// 76-byte records in; where a named material is the emitter of triangle lights, their colours follow and the light refit
// (light_refit.h) runs behind them.  Element functions shared by the device kernels (materials.hip.h) and a plain-loop host driver
// (tests/hostsim/hostsim_materials.cpp), like light_pose.h: IEEE operations in a STATED ORDER without contraction on both sides, so
// both produce the same bits.
//
//   may change    base_color, tangent_rotation_or_strength, ior and the eleven *_unorm halves (and the padding half behind them)
//   must stay     textures[5], flags, type, bytewise: for a Mix node two of the textures are its operands, so the node graph stays, and
//                 with it everything an upload derives from the materials -- the solid bits of the triangles, the choice of kernels,
//                 the validity of the texture handles, which triangle light has which emitter
//   emitter       the scene build (SceneCPU.cpp, AddMeshInstance) bakes a material into every triangle light it spawns: the FIRST
//                 Emissive + MAT_FLAG_IMP_SAMPLE material found breadth-first from the triangle's front material through the Mix
//                 operands, col[k] = base_color[k] * strength.  emitter_tables walks that order once per upload or instance update
//                 and leaves one material slot per light slot (NO_EMITTER: none); the kernel searches nothing.
//
// A call names material slots; it is refused as a whole (nothing on the device written) when a named slot is outside the material
// array or no reachable triangle or Mix operand uses it (SLOT_LIVE: the mat_used set of scene_validate.h), is named twice, would get
// another type, flags or texture word than it holds, gets a float that is not finite, or -- an Emissive record -- a negative
// base_color component or strength (a negative flux breaks the importance rows of the light tree).  It needs an upload (2) when a record
// refracts while the passes leave the rays' ior plane alone (plain_ior), or when a named emitter's colour or strength would change
// while the lights cannot be refitted.
#pragma once

#include <stdint.h>
#include <string.h>

#include <vector>

#include "rt_types.h"

namespace rayhip_materials {

using namespace rt;

constexpr uint32_t RECORD_WORDS = 19; // sizeof(rayhip_material) / 4
static_assert(sizeof(rayhip_material) == RECORD_WORDS * 4, "76 bytes");
constexpr uint32_t SLOT_LIVE = 1u;    // per-slot flags: a reachable triangle or a Mix operand uses the slot ...
constexpr uint32_t SLOT_EMITTER = 2u; // ... some triangle light took its colour from it
constexpr uint16_t NO_EMITTER = 0xffffu;
constexpr int MAX_GRAPH = 64; // materials the breadth-first search visits below one triangle side (a Mix graph with a cycle ends here)
// the findings of a call, one counter each; behind them what is no finding: the named entries that are emitters
enum { BAD_SLOT = 0, DUPLICATE = 1, GRAPH_CHANGED = 2, NOT_FINITE = 3, NEGATIVE = 4, REFRACTS = 5, PINNED = 6, N_FINDINGS = 7, EMITTERS_NAMED = 7, N_COUNTERS = 8 };

RT_HD bool finite_f(const float x) { return fabsf(x) <= 3.402823466e+38f; } // (false for NaN)

// the five floats of a record
RT_HD bool finite_record(const rayhip_material &m) {
    return finite_f(m.base_color[0]) && finite_f(m.base_color[1]) && finite_f(m.base_color[2]) && finite_f(m.tangent_rotation_or_strength) && finite_f(m.ior);
}

// a slot a call may name: inside the material array and in use (`flags`: one byte per slot)
RT_HD bool slot_ok(const uint32_t slot, const uint8_t *flags, const uint32_t n_materials) { return slot < n_materials && (flags[slot] & SLOT_LIVE) != 0; }

// what is wrong with the record `m` for a slot that holds `held`
RT_HD bool graph_changed(const rayhip_material &held, const rayhip_material &m) {
    bool same = held.flags == m.flags && held.type == m.type;
    for (int k = 0; k < 5; ++k) {
        same = same && held.textures[k] == m.textures[k];
    }
    return !same;
}
RT_HD bool negative_emission(const rayhip_material &m) {
    return m.type == NODE_EMISSIVE && (m.base_color[0] < 0.0f || m.base_color[1] < 0.0f || m.base_color[2] < 0.0f || m.tangent_rotation_or_strength < 0.0f);
}
// the upload's test (rayhip_upload.hip.h): can the surface change a ray's stack of refractive indices?
RT_HD bool refracts(const rayhip_material &m) { return m.type == NODE_REFRACTIVE || (m.type == NODE_PRINCIPLED && m.transmission_unorm != 0); }
// bytewise: an unchanged colour and strength passes where the lights cannot follow
RT_HD bool emission_changed(const rayhip_material &held, const rayhip_material &m) {
    return float_as_uint(held.base_color[0]) != float_as_uint(m.base_color[0]) || float_as_uint(held.base_color[1]) != float_as_uint(m.base_color[1]) ||
           float_as_uint(held.base_color[2]) != float_as_uint(m.base_color[2]) ||
           float_as_uint(held.tangent_rotation_or_strength) != float_as_uint(m.tangent_rotation_or_strength);
}

// the colour of a triangle light whose emitter is `m`: three single multiplies, the bits the scene build stores
RT_HD void emitter_colour(const rayhip_material &m, float col[3]) {
    col[0] = m.base_color[0] * m.tangent_rotation_or_strength;
    col[1] = m.base_color[1] * m.tangent_rotation_or_strength;
    col[2] = m.base_color[2] * m.tangent_rotation_or_strength;
}

// one entry of a call judged: what it adds to each counter.  `claimed_before`: another entry named the slot already; `refittable`: the
// lights can follow an emitter (rayhip_scene_refit_lights is on and its tables are prepared)
struct Judgement {
    bool bad_slot = false, duplicate = false, changed = false, not_finite = false, negative = false, refracting = false, pinned = false, emitter = false;
};
RT_HD Judgement judge_record(const rayhip_material &m, const rayhip_material &held, const uint8_t slot_flags, const bool claimed_before, const bool plain_ior,
                             const bool refittable) {
    Judgement j;
    j.duplicate = claimed_before;
    j.changed = graph_changed(held, m);
    j.emitter = (slot_flags & SLOT_EMITTER) != 0;
    j.pinned = j.emitter && !refittable && emission_changed(held, m);
    j.not_finite = !finite_record(m), j.negative = negative_emission(m), j.refracting = plain_ior && refracts(m);
    return j;
}

// what the counters of a call mean: 0 = go on, 1 = refused, 2 = the scene needs an upload
RT_HD int verdict(const uint32_t counters[N_COUNTERS]) {
    if ((counters[BAD_SLOT] | counters[DUPLICATE] | counters[GRAPH_CHANGED] | counters[NOT_FINITE] | counters[NEGATIVE]) != 0) {
        return 1;
    }
    return (counters[REFRACTS] | counters[PINNED]) != 0 ? 2 : 0;
}

// the light slot `li` recoloured when its emitter was named in this call (`claim`: one word per material slot, not zero where named)
RT_HD void recolour_tri_light(rayhip_light *lights, const uint32_t li, const uint16_t *light_emitter, const uint32_t *claim, const rayhip_material *materials,
                              const uint32_t n_materials) {
    const uint32_t m = light_emitter[li];
    if (m == NO_EMITTER || m >= n_materials || claim[m] == 0u || light_type(lights[li]) != LIGHT_TYPE_TRI) {
        return;
    }
    emitter_colour(materials[m], lights[li].col);
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
// the emitter of the triangle side whose material is `first`: the scene build's breadth-first search, every index checked
inline uint16_t emitter_of(const rayhip_material *materials, const uint32_t n_materials, const uint32_t first) {
    uint32_t queue[MAX_GRAPH];
    int count = 0;
    queue[count++] = first;
    for (int i = 0; i < count; ++i) {
        if (queue[i] >= n_materials) {
            return NO_EMITTER;
        }
        const rayhip_material &mat = materials[queue[i]];
        if (mat.type == NODE_EMISSIVE && (mat.flags & MAT_FLAG_IMP_SAMPLE) != 0) {
            return uint16_t(queue[i]);
        }
        if (mat.type == NODE_MIX && count + 2 <= MAX_GRAPH) {
            queue[count++] = mat.textures[MIX_MAT1];
            queue[count++] = mat.textures[MIX_MAT2];
        }
    }
    return NO_EMITTER;
}

// light_emitter[n_lights]: per light slot the material a triangle light that li_indices names took its colour from, NO_EMITTER for
// every other slot; `flags` [n_materials]: SLOT_EMITTER cleared, then set for the materials the table names (SLOT_LIVE stays)
inline void emitter_tables(const rayhip_light *lights, const uint32_t n_lights, const uint32_t *li_indices, const uint32_t n_li,
                           const rayhip_tri_mat_data *tri_materials, const uint32_t n_tri_materials, const rayhip_material *materials, const uint32_t n_materials,
                           std::vector<uint16_t> &light_emitter, std::vector<uint8_t> &flags) {
    light_emitter.assign(n_lights, NO_EMITTER);
    flags.resize(n_materials, 0);
    for (uint8_t &f : flags) {
        f &= uint8_t(~SLOT_EMITTER);
    }
    for (uint32_t k = 0; k < n_li; ++k) {
        const uint32_t i = li_indices[k];
        if (i >= n_lights || light_type(lights[i]) != LIGHT_TYPE_TRI) {
            continue;
        }
        const uint32_t tri = float_as_uint(lights[i].params[0]);
        if (tri >= n_tri_materials) {
            continue;
        }
        const uint16_t m = emitter_of(materials, n_materials, tri_materials[tri].front_mi & MATERIAL_INDEX_BITS);
        light_emitter[i] = m;
        if (m != NO_EMITTER) {
            flags[m] |= uint8_t(SLOT_EMITTER);
        }
    }
}

// check and commit as plain loops: `materials` [n_materials] in place, `claim` [n_materials] cleared and marked as the device marks
// it.  The counters are counted as the device counts them; the array is written only where verdict() is 0, which is returned.  The
// lights are the caller's to recolour (recolour_tri_light over every light slot) and refit when counters[EMITTERS_NAMED] is not zero.
inline int set_materials_host(rayhip_material *materials, const uint32_t n_materials, const uint8_t *flags, uint32_t *claim, const bool plain_ior,
                              const bool refittable, const uint32_t n, const uint32_t *slots, const rayhip_material *records, uint32_t counters[N_COUNTERS]) {
    for (int k = 0; k < N_COUNTERS; ++k) {
        counters[k] = 0;
    }
    for (uint32_t m = 0; m < n_materials; ++m) {
        claim[m] = 0;
    }
    for (uint32_t i = 0; i < n; ++i) {
        if (!slot_ok(slots[i], flags, n_materials)) {
            counters[BAD_SLOT] += 1;
            counters[NOT_FINITE] += finite_record(records[i]) ? 0u : 1u;
            continue;
        }
        const Judgement j = judge_record(records[i], materials[slots[i]], flags[slots[i]], claim[slots[i]]++ != 0u, plain_ior, refittable);
        counters[DUPLICATE] += j.duplicate, counters[GRAPH_CHANGED] += j.changed, counters[NOT_FINITE] += j.not_finite, counters[NEGATIVE] += j.negative;
        counters[REFRACTS] += j.refracting, counters[PINNED] += j.pinned, counters[EMITTERS_NAMED] += j.emitter;
    }
    const int rc = verdict(counters);
    for (uint32_t i = 0; rc == 0 && i < n; ++i) {
        materials[slots[i]] = records[i];
    }
    return rc;
}

} // namespace rayhip_materials
