// hostsim_light_pose.cpp -- TEST INFRASTRUCTURE.  Moving and recolouring analytic lights as the device does it
// (ray_amd/csrc/light_pose.h: the flux and summary of a record, the checks of a call, the commit; ray_amd/csrc/light_refit.h: the level
// refit with the `posed` table), compiled with g++ (the HOSTSIM_FLAGS of hostsim.cpp: no fma contraction, SSE2) over plain arrays, with
// the prefix hostsim_ and without a context.  tests/test_light_pose_hostsim.py holds these against the scenes the reference built and
// a numpy restatement; tests/test_gpu_light_pose.py holds the device (light_pose.hip.h) against this file.
//
// Never linked into librayhip.so.
#include <string.h>

#include <vector>

#include "../../include/rayhip.h"
#include "../../ray_amd/csrc/light_pose.h"

#define HS_API extern "C" __attribute__((visibility("default")))

using rayhip_light_refit::Summary;

// leaf[n][12]: the complete summaries (flux included) of n analytic records
HS_API int hostsim_analytic_light_summaries(const rayhip_light *records, uint32_t n, float *leaf) {
    for (uint32_t i = 0; i < n; ++i) {
        rayhip_light_pose::analytic_light_summary(records[i], reinterpret_cast<Summary *>(leaf)[i]);
    }
    return 0;
}

// live[n_lights]: 1 where li_indices names the slot
HS_API int hostsim_light_live_table(const uint32_t *li_indices, uint32_t n_li, uint32_t n_lights, uint8_t *live) {
    const std::vector<uint8_t> t = rayhip_light_pose::live_table(li_indices, n_li, n_lights);
    if (!t.empty()) {
        memcpy(live, t.data(), t.size());
    }
    return 0;
}

// the whole call over the arrays in place: lights[n_lights], live / posed [n_lights], leaf[n_lights][12], and the tree (nodes, its
// node_summary scratch, children[n_nodes][26][4], slot_scale[n_nodes][8] or null) refitted under `posed` behind the commit.
// out_findings[5]: bad slots, duplicates, triangle or environment records, changed words 0, records that are not finite.  Returns what
// the entry point returns for a context whose tables are ready (0, 1); the arrays are written only with 0.
HS_API int hostsim_set_lights(rayhip_light *lights, uint32_t n_lights, const uint8_t *live, uint8_t *posed, float *leaf, rayhip_light_cwbvh_node *nodes,
                              uint32_t n_nodes, float *node_summary, float *children, const float *slot_scale, uint32_t n, const uint32_t *slots,
                              const rayhip_light *records, uint32_t *out_findings) {
    for (int k = 0; k < rayhip_light_pose::N_FINDINGS; ++k) {
        out_findings[k] = 0;
    }
    if (n > 0 && (!slots || !records)) {
        return 1;
    }
    if (n == 0) {
        return 0;
    }
    if (const int rc = rayhip_light_pose::pose_lights_host(lights, n_lights, live, posed, reinterpret_cast<Summary *>(leaf), n, slots, records, out_findings)) {
        return rc;
    }
    return rayhip_light_refit::refit_light_nodes_host(nodes, n_nodes, lights, n_lights, reinterpret_cast<const Summary *>(leaf),
                                                      reinterpret_cast<Summary *>(node_summary), reinterpret_cast<float4 *>(children), slot_scale, posed)
               ? 3
               : 0;
}

// the level refit alone under a `posed` table (null: none), as hostsim_refit_light_nodes of hostsim_lights.cpp
HS_API int hostsim_refit_light_nodes_posed(rayhip_light_cwbvh_node *nodes, uint32_t n_nodes, const rayhip_light *lights, uint32_t n_lights, const float *leaf,
                                           float *node_summary, float *children, const float *slot_scale, const uint8_t *posed) {
    return rayhip_light_refit::refit_light_nodes_host(nodes, n_nodes, lights, n_lights, reinterpret_cast<const Summary *>(leaf),
                                                      reinterpret_cast<Summary *>(node_summary), reinterpret_cast<float4 *>(children), slot_scale, posed);
}
