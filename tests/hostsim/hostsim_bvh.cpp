// hostsim_bvh.cpp -- TEST INFRASTRUCTURE.  The tree builders and the wide node test compiled with g++ (the HOSTSIM_FLAGS of
// hostsim.cpp: no fma contraction, SSE2, glibc libm) behind the signatures of include/rayhip.h's rayhip_k_lbvh_build,
// rayhip_k_bvh4_collapse and rayhip_k_bvh4_test_nodes, with the prefix hostsim_ and without a context:
//   lbvh.h       rayhip_lbvh::build_host
//   bvh4_build.h rayhip_bvh4::build over wide_children / quantise (the host driver: depth-first node order)
//   rt_bvh4.h    rt::bvh4_test_node, the plain-load form
// tests/test_bvh_builders_hostsim.py holds them against the checker of tests/bvh_build_cases.py; tests/test_gpu_bvh_builders.py
// holds the device against this file.
//
// Never linked into librayhip.so.
#include <string>

#include "../../include/rayhip.h"
#include "../../ray_amd/csrc/bvh_hooks.h"

#define HS_API extern "C" __attribute__((visibility("default")))

namespace {
thread_local std::string g_err;
}

HS_API const char *hostsim_bvh_last_error() { return g_err.c_str(); }

HS_API int hostsim_k_lbvh_build(const float *boxes, const uint32_t *groups, uint32_t n_prims, uint32_t n_groups, uint32_t leaf_max,
                                int leaf_is_primitive, int roots_are_nodes, rayhip_bvh2_node *out_nodes, uint32_t nodes_cap, uint32_t *out_entries,
                                uint32_t entries_cap, uint32_t *out_group_root, float *out_bounds, uint32_t *out_counts) {
    if (!rayhip_bvh_hooks::check_lbvh_args(boxes, groups, n_prims, n_groups, leaf_max, g_err)) {
        return 1;
    }
    const rayhip_lbvh::Output out =
        rayhip_lbvh::build_host(rayhip_bvh_hooks::lbvh_input(boxes, groups, n_prims, n_groups, leaf_max, leaf_is_primitive, roots_are_nodes));
    return rayhip_bvh_hooks::copy_lbvh_output(out, out_nodes, nodes_cap, out_entries, entries_cap, out_group_root, out_bounds, out_counts, g_err) ? 0 : 1;
}

HS_API int hostsim_k_bvh4_collapse(const rayhip_bvh2_node *nodes, uint32_t n_nodes, const uint32_t *roots, uint32_t n_roots, void *out_wide,
                                   uint32_t *out_roots4, uint32_t *out_count) {
    return rayhip_bvh_hooks::collapse_host(nodes, n_nodes, roots, n_roots, static_cast<rt::Bvh4Node *>(out_wide), out_roots4, out_count, g_err);
}

HS_API int hostsim_k_bvh4_test_nodes(const void *wide, uint32_t n_wide, const uint32_t *node_index, const float *ray_o, const float *ray_d,
                                     const float *ray_t, uint32_t n_items, uint32_t *out_ref, uint32_t *out_n_hit, float *out_dist) {
    if (!rayhip_bvh_hooks::check_items(node_index, n_items, n_wide, g_err)) {
        return 1;
    }
    const rt::Bvh4Node *w = static_cast<const rt::Bvh4Node *>(wide);
    for (uint32_t i = 0; i < n_items; ++i) {
        rayhip_bvh_hooks::test_node_item(w, node_index[i], ray_o + size_t(i) * 3, ray_d + size_t(i) * 3, ray_t[i], out_ref + size_t(i) * 4, out_n_hit + i,
                                         out_dist + size_t(i) * 4);
    }
    return 0;
}
