// hostsim_refit.cpp -- TEST INFRASTRUCTURE.  What a vertex update recomputes (ray_amd/csrc/refit.h: triangle records, the boxes of
// the bottom-level trees) and the instance boxes of its top level (scene_rebuild.h: transform_box), compiled with g++ (the
// HOSTSIM_FLAGS of hostsim.cpp: no fma contraction, SSE2, glibc libm) over plain arrays, with the prefix hostsim_ and without a
// context.  tests/test_vertex_update_hostsim.py holds these against the scenes the reference built; tests/test_gpu_vertex_update.py
// holds the device (refit.hip.h) against this file.
//
// Never linked into librayhip.so.
#include <string>

#include "../../include/rayhip.h"
#include "../../ray_amd/csrc/refit.h"
#include "../../ray_amd/csrc/scene_rebuild.h"

#define HS_API extern "C" __attribute__((visibility("default")))

// tris[n_entries]: in = the records as they are, out = every entry that names a triangle recomputed from its corners;
// *out_degenerate = triangles without area
HS_API int hostsim_refit_tris(const rayhip_vertex *vertices, uint32_t n_vertices, const uint32_t *vtx_indices, uint32_t n_vtx_indices,
                              const uint32_t *tri_indices, uint32_t n_entries, rayhip_tri_accel *tris, uint32_t *out_degenerate) {
    *out_degenerate = rayhip_refit::refit_tris_host(vertices, n_vertices, vtx_indices, n_vtx_indices / 3, tri_indices, n_entries, tris);
    return 0;
}

// nodes[n_nodes]: the child boxes of every node below `roots` recomputed bottom-up; 0 = ok, 1 = not a forest, 2 = above 128 levels
HS_API int hostsim_refit_nodes(rayhip_bvh2_node *nodes, uint32_t n_nodes, const uint32_t *roots, uint32_t n_roots, const uint32_t *tri_indices,
                               const uint32_t *vtx_indices, const rayhip_vertex *vertices) {
    return rayhip_refit::refit_nodes_host(nodes, n_nodes, std::vector<uint32_t>(roots, roots + n_roots), tri_indices, vtx_indices, vertices);
}

// out_boxes[n_slots][6] (lo, hi): the world-space box of instance slots[k] -- the box of its tree's root node under its transform
HS_API int hostsim_instance_boxes(const rayhip_bvh2_node *nodes, uint32_t n_nodes, const rayhip_mesh_instance *instances, uint32_t n_instances,
                                  const uint32_t *slots, uint32_t n_slots, float *out_boxes) {
    for (uint32_t k = 0; k < n_slots; ++k) {
        if (slots[k] >= n_instances || instances[slots[k]].node_index >= n_nodes) {
            return 1;
        }
        const rayhip_mesh_instance &mi = instances[slots[k]];
        const rayhip_lbvh::Box b = rayhip_rebuild::transform_box(rayhip_rebuild::node_box(nodes[mi.node_index]), mi.xform);
        memcpy(out_boxes + size_t(k) * 6, &b, sizeof(b));
    }
    return 0;
}
