// hostsim_lights.cpp -- TEST INFRASTRUCTURE.  What a vertex update recomputes of the lights when rayhip_scene_refit_lights is on
// (ray_amd/csrc/light_refit.h: the triangle lights' corners and summaries, the light tree level by level, its importance rows),
// compiled with g++ (the HOSTSIM_FLAGS of hostsim.cpp: no fma contraction, SSE2) over plain arrays, with the prefix hostsim_ and
// without a context.  tests/test_light_refit_hostsim.py holds these against the scenes the reference built and against a float64
// model; tests/test_gpu_light_refit.py holds the device (light_refit.hip.h) against this file.
//
// Never linked into librayhip.so.
#include <string.h>

#include <vector>

#include "../../include/rayhip.h"
#include "../../ray_amd/csrc/light_refit.h"

#define HS_API extern "C" __attribute__((visibility("default")))

using rayhip_light_refit::Summary;

// leaf[n_lights] (12 floats each): the lights that are no triangles complete, their flux from the tree; triangle lights zero
HS_API int hostsim_light_leaf_table(const rayhip_light *lights, uint32_t n_lights, const rayhip_light_cwbvh_node *nodes, uint32_t n_nodes, float *leaf) {
    const std::vector<Summary> t = rayhip_light_refit::leaf_table(lights, n_lights, nodes, n_nodes);
    if (!t.empty()) {
        memcpy(leaf, t.data(), t.size() * sizeof(Summary));
    }
    return 0;
}

// tri_geom[n_lights][4][4] and leaf[n_lights][12]: in = as they are, out = the entries of the triangle lights li_indices names
// recomputed; *out_degenerate = those without area
HS_API int hostsim_refit_tri_lights(const rayhip_light *lights, uint32_t n_lights, const uint32_t *li_indices, uint32_t n_li,
                                    const rayhip_mesh_instance *instances, uint32_t n_instances, const uint32_t *vtx_indices, uint32_t n_vtx_indices,
                                    const rayhip_vertex *vertices, uint32_t n_vertices, float *tri_geom, float *leaf, uint32_t *out_degenerate) {
    *out_degenerate = rayhip_light_refit::refit_tri_lights_host(lights, n_lights, li_indices, n_li, instances, n_instances, vtx_indices, n_vtx_indices, vertices,
                                                                n_vertices, reinterpret_cast<float4 *>(tri_geom), reinterpret_cast<Summary *>(leaf));
    return 0;
}

// nodes[n_nodes] and children[n_nodes][26][4]: refitted level by level under the leaf table; node_summary[n_nodes][12] = the
// summaries of the nodes; slot_scale[n_nodes][8] from hostsim_light_slot_scales, or null (1 everywhere).
// 0 = ok, 1 = a link outside the arrays or a child before its parent, 2 = too high
HS_API int hostsim_refit_light_nodes(rayhip_light_cwbvh_node *nodes, uint32_t n_nodes, const rayhip_light *lights, uint32_t n_lights, const float *leaf,
                                     float *node_summary, float *children, const float *slot_scale) {
    return rayhip_light_refit::refit_light_nodes_host(nodes, n_nodes, lights, n_lights, reinterpret_cast<const Summary *>(leaf),
                                                      reinterpret_cast<Summary *>(node_summary), reinterpret_cast<float4 *>(children), slot_scale);
}

// slot_scale[n_nodes][8]: what an upload prepares of the tree `nodes` and the pose (`vertices`, `instances`) it was built at -- per
// inner slot the stored flux over the summed flux below it (light_refit.h: slot_scales)
HS_API int hostsim_light_slot_scales(const rayhip_light *lights, uint32_t n_lights, const uint32_t *li_indices, uint32_t n_li,
                                     const rayhip_mesh_instance *instances, uint32_t n_instances, const uint32_t *vtx_indices, uint32_t n_vtx_indices,
                                     const rayhip_vertex *vertices, uint32_t n_vertices, const rayhip_light_cwbvh_node *nodes, uint32_t n_nodes, float *slot_scale) {
    std::vector<float> out;
    const int rc = rayhip_light_refit::slot_scales(lights, n_lights, li_indices, n_li, instances, n_instances, vtx_indices, n_vtx_indices, vertices, n_vertices,
                                                   nodes, n_nodes, out);
    if (rc == 0 && !out.empty()) {
        memcpy(slot_scale, out.data(), out.size() * sizeof(float));
    }
    return rc;
}

// level_nodes[n_nodes] sorted by height, level_offset[*out_levels + 1] (room for `capacity` words); returns as plan_levels
HS_API int hostsim_light_levels(const rayhip_light_cwbvh_node *nodes, uint32_t n_nodes, uint32_t n_lights, uint32_t *level_nodes, uint32_t *level_offset,
                                uint32_t capacity, uint32_t *out_levels) {
    std::vector<uint32_t> ln, lo;
    const int rc = rayhip_light_refit::plan_levels(nodes, n_nodes, n_lights, ln, lo);
    if (rc || lo.size() > capacity) {
        return rc ? rc : 3;
    }
    memcpy(level_nodes, ln.data(), ln.size() * sizeof(uint32_t));
    memcpy(level_offset, lo.data(), lo.size() * sizeof(uint32_t));
    *out_levels = uint32_t(lo.size() - 1);
    return 0;
}

// children[n_nodes][26][4]: the importance rows as an upload makes them (shade_lights.h: fill_light_children)
HS_API int hostsim_fill_light_children(const rayhip_light_cwbvh_node *nodes, uint32_t n_nodes, float *children) {
    for (uint32_t w = 0; w < n_nodes; ++w) {
        rt::fill_light_children(nodes[w], reinterpret_cast<float4 *>(children) + size_t(w) * rt::LIGHT_CHILDREN_STRIDE);
    }
    return 0;
}

// tri_geom[n_lights][4][4] as an upload makes it (shade_lights.h: fill_light_tri_geom over the slots li_indices names)
HS_API int hostsim_fill_light_tri_geom(const rayhip_light *lights, uint32_t n_lights, const uint32_t *li_indices, uint32_t n_li,
                                       const rayhip_mesh_instance *instances, const uint32_t *vtx_indices, const rayhip_vertex *vertices, float *tri_geom) {
    memset(tri_geom, 0, size_t(n_lights) * 16 * sizeof(float));
    for (uint32_t k = 0; k < n_li; ++k) {
        if (li_indices[k] < n_lights) {
            rt::fill_light_tri_geom(lights[li_indices[k]], instances, vtx_indices, vertices, reinterpret_cast<float4 *>(tri_geom) + size_t(li_indices[k]) * 4);
        }
    }
    return 0;
}

// boxes[n_nodes][8][6] (lo, hi): the decoded child boxes (shade_lights.h: light_child_box)
HS_API int hostsim_light_child_boxes(const rayhip_light_cwbvh_node *nodes, uint32_t n_nodes, float *boxes) {
    for (uint32_t w = 0; w < n_nodes; ++w) {
        for (int i = 0; i < 8; ++i) {
            float *b = boxes + (size_t(w) * 8 + i) * 6;
            rt::light_child_box(nodes[w], i, b, b + 3);
        }
    }
    return 0;
}

// imp[8]: the importances of the children of `node` as seen from P (shade_lights.h: light_child_importance over decode_light_child)
HS_API int hostsim_light_importances(const rayhip_light_cwbvh_node *node, const float *P, float *imp) {
    for (int i = 0; i < 8; ++i) {
        imp[i] = rt::light_child_importance(rt::decode_light_child(*node, i), rt::f3{P[0], P[1], P[2]});
    }
    return 0;
}
