// hostsim_materials.cpp -- TEST INFRASTRUCTURE.  Changing materials as the device does it (ray_amd/csrc/materials.h: the checks of a
// call, the commit, the emitter table of the triangle lights and their recolouring), compiled with g++ (the HOSTSIM_FLAGS of
// hostsim.cpp: no fma contraction, SSE2) over plain arrays, with the prefix hostsim_ and without a context.  The light refit behind a
// recoloured emitter is the one of tests/hostsim/hostsim_lights.cpp and hostsim_light_pose.cpp, called by the tests.
// tests/test_materials_hostsim.py holds these against the scenes the reference built; tests/test_gpu_materials.py holds the device
// (materials.hip.h) against this file.
//
// Never linked into librayhip.so.
#include <string.h>

#include <vector>

#include "../../include/rayhip.h"
#include "../../ray_amd/csrc/materials.h"

#define HS_API extern "C" __attribute__((visibility("default")))

namespace rm = rayhip_materials;

// light_emitter[n_lights]: the material slot every triangle light that li_indices names took its colour from (0xffff: none);
// flags[n_materials] in place: SLOT_EMITTER (2) set for those materials and cleared for the others, SLOT_LIVE (1) kept
HS_API int hostsim_material_emitter_tables(const rayhip_light *lights, uint32_t n_lights, const uint32_t *li_indices, uint32_t n_li,
                                           const rayhip_tri_mat_data *tri_materials, uint32_t n_tri_materials, const rayhip_material *materials,
                                           uint32_t n_materials, uint16_t *light_emitter, uint8_t *flags) {
    std::vector<uint16_t> table;
    std::vector<uint8_t> f(flags, flags + n_materials);
    rm::emitter_tables(lights, n_lights, li_indices, n_li, tri_materials, n_tri_materials, materials, n_materials, table, f);
    if (n_lights) {
        memcpy(light_emitter, table.data(), size_t(n_lights) * sizeof(uint16_t));
    }
    if (n_materials) {
        memcpy(flags, f.data(), n_materials);
    }
    return 0;
}

// check and commit over materials[n_materials] in place; claim[n_materials] as the device leaves it; out_counters[8]: bad slots,
// duplicates, changed type / flags / textures, not finite, negative emission, refracting on a plain_ior scene, pinned emitters, and
// the named entries that are emitters.  Returns what the entry point returns for a context with a scene (0, 1, 2); the array is
// written only with 0.
HS_API int hostsim_set_materials(rayhip_material *materials, uint32_t n_materials, const uint8_t *flags, uint32_t *claim, int plain_ior, int refittable,
                                 uint32_t n, const uint32_t *slots, const rayhip_material *records, uint32_t *out_counters) {
    for (int k = 0; k < rm::N_COUNTERS; ++k) {
        out_counters[k] = 0;
    }
    if (n > 0 && (!slots || !records)) {
        return 1;
    }
    if (n == 0) {
        return 0;
    }
    return rm::set_materials_host(materials, n_materials, flags, claim, plain_ior != 0, refittable != 0, n, slots, records, out_counters);
}

// lights[n_lights] in place: every triangle light whose emitter `claim` marks takes base_color * strength of that material
HS_API int hostsim_recolour_tri_lights(rayhip_light *lights, uint32_t n_lights, const uint16_t *light_emitter, const uint32_t *claim,
                                       const rayhip_material *materials, uint32_t n_materials) {
    for (uint32_t li = 0; li < n_lights; ++li) {
        rm::recolour_tri_light(lights, li, light_emitter, claim, materials, n_materials);
    }
    return 0;
}
