// hostsim_pick.cpp -- TEST INFRASTRUCTURE.  One level of the light pick over the importance rows of one node, in both forms
// (ray_amd/csrc/shade_lights.h): all eight children (light_node_importances_rows, what k_light_pick_first runs) and the occupied
// ones only (light_node_occupancy + light_node_importances_sparse, what k_light_pick_sparse runs), compiled with g++ (the
// HOSTSIM_FLAGS of hostsim.cpp: no fma contraction, SSE2) over plain arrays, with the prefix hostsim_ and without a context.
// tests/test_pick_sparse_host.py holds the two against each other word by word.
//
// Never linked into librayhip.so.
#include <stddef.h>
#include <stdint.h>

#include "../../include/rayhip.h"
#include "../../ray_amd/csrc/shade_lights.h"

#define HS_API extern "C" __attribute__((visibility("default")))

// rows[26][4]: one node of the table (fill_light_children); out[2]: masks, slots
HS_API int hostsim_pick_occupancy(const float *rows, uint32_t *out) {
    const rt::LightOccupancy o = rt::light_node_occupancy(reinterpret_cast<const float4 *>(rows));
    out[0] = o.masks, out[1] = o.slots;
    return 0;
}

// P[n][3] -> dense[n][8], sparse[n][8]: the importances of the node's children as seen from every P, by either form
HS_API int hostsim_pick_level(const float *rows, const float *P, uint32_t n, float *dense, float *sparse) {
    const float4 *r = reinterpret_cast<const float4 *>(rows);
    const rt::LightOccupancy o = rt::light_node_occupancy(r);
    for (uint32_t p = 0; p < n; ++p) {
        const rt::f3 at = rt::f3{P[3 * p + 0], P[3 * p + 1], P[3 * p + 2]};
        rt::light_node_importances_rows(r, at, dense + 8 * size_t(p));
        rt::light_node_importances_sparse(r, o, at, sparse + 8 * size_t(p));
    }
    return 0;
}
