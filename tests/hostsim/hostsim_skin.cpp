// hostsim_skin.cpp -- TEST INFRASTRUCTURE.  Linear-blend skinning as the device does it (ray_amd/csrc/skin.h: the posed record of a
// vertex, the check of its position), compiled with g++ (the HOSTSIM_FLAGS of hostsim.cpp: no fma contraction, SSE2, glibc libm)
// over plain arrays, with the prefix hostsim_ and without a context.  tests/test_skinning_hostsim.py holds these against a numpy
// restatement; tests/test_gpu_skinning.py holds the device (skin.hip.h) against this file.
//
// Never linked into librayhip.so.
#include "../../include/rayhip.h"
#include "../../ray_amd/csrc/skin.h"

#define HS_API extern "C" __attribute__((visibility("default")))

// out[count]: rest[count] posed by bones[bones_count][12]; `used`: per vertex, or null (all in use).  *out_bad = vertices in use whose
// posed position is not finite.  0 = ok, 1 = a bone index outside the palette, 2 = a weight that is negative or not finite.
HS_API int hostsim_skin_vertices(const rayhip_vertex *rest, const uint16_t *indices, const float *weights, uint32_t count, const float *bones,
                                 uint32_t bones_count, const uint8_t *used, rayhip_vertex *out, uint32_t *out_bad) {
    uint32_t where = 0;
    if (const int rc = rayhip_skin::validate_influences(indices, weights, count, bones_count, where)) {
        return rc;
    }
    *out_bad = rayhip_skin::skin_vertices_host(rest, indices, weights, count, bones, used, out);
    return 0;
}

// what the device-pointer update counts over vertices[count] (the range starts at vertex `first`; `used` covers the whole array):
// out[0] = vertices in use without a finite position, out[1] = vertices of triangle lights that differ from the kept records
HS_API int hostsim_check_vertices(const rayhip_vertex *vertices, uint32_t first, uint32_t count, const uint8_t *used, const uint32_t *light_index,
                                  const rayhip_vertex *light_kept, uint32_t n_lights, uint32_t *out) {
    out[0] = out[1] = 0;
    for (uint32_t i = 0; i < count; ++i) {
        out[0] += rayhip_skin::vertex_check(vertices[i], used[first + i] != 0) ? 1u : 0u;
    }
    for (uint32_t i = 0; i < n_lights; ++i) {
        const uint32_t v = light_index[i];
        out[1] += v >= first && v - first < count && !rayhip_skin::same_bytes(vertices[v - first], light_kept[i]) ? 1u : 0u;
    }
    return 0;
}

// palettes up to this many bones are read from LDS by the device kernel, larger ones from memory
HS_API uint32_t hostsim_skin_lds_bones(void) { return rayhip_skin::SKIN_LDS_BONES; }
