// bvh_hooks.h -- the host halves of the builder test hooks (include/rayhip.h: rayhip_k_lbvh_build, rayhip_k_bvh4_collapse,
// rayhip_k_bvh4_test_nodes): argument checks, the host builds, and the copy into caller buffers.  Shared by librayhip's hooks
// (rayhip_hooks.hip.h) and the host build of the same calls (tests/hostsim/hostsim_bvh.cpp), so both refuse the same inputs.
#pragma once

#include <string>
#include <vector>

#include "bvh4_build.h"
#include "lbvh.h"

namespace rayhip_bvh_hooks {

inline bool check_lbvh_args(const float *boxes, const uint32_t *groups, const uint32_t n_prims, const uint32_t n_groups, const uint32_t leaf_max,
                            std::string &why) {
    if (leaf_max < 1 || leaf_max > 8) {
        why = "leaf_max must be 1..8";
        return false;
    }
    if (n_prims >= 0x10000000u) {
        why = "too many primitives for a leaf word";
        return false;
    }
    if (n_prims && (!boxes || !groups)) {
        why = "null input";
        return false;
    }
    for (uint32_t p = 0; p < n_prims; ++p) {
        if (groups[p] >= n_groups) {
            why = "a group id is out of range";
            return false;
        }
    }
    return true;
}

inline rayhip_lbvh::Input lbvh_input(const float *boxes, const uint32_t *groups, const uint32_t n_prims, const uint32_t n_groups,
                                     const uint32_t leaf_max, const int leaf_is_primitive, const int roots_are_nodes) {
    static_assert(sizeof(rayhip_lbvh::Box) == 6 * sizeof(float), "Box is lo.xyz, hi.xyz");
    rayhip_lbvh::Input in;
    in.prim_box = reinterpret_cast<const rayhip_lbvh::Box *>(boxes), in.prim_group = groups, in.group_centroids = nullptr;
    in.n_prims = n_prims, in.n_groups = n_groups, in.leaf_max = leaf_max;
    in.leaf_is_primitive = leaf_is_primitive != 0, in.roots_are_nodes = roots_are_nodes != 0;
    return in;
}

inline bool copy_lbvh_output(const rayhip_lbvh::Output &out, rayhip_bvh2_node *out_nodes, const uint32_t nodes_cap, uint32_t *out_entries,
                             const uint32_t entries_cap, uint32_t *out_group_root, float *out_bounds, uint32_t *out_counts, std::string &why) {
    if (out.nodes.size() > nodes_cap || out.entries.size() > entries_cap) {
        why = "an output buffer is too small";
        return false;
    }
    std::copy(out.nodes.begin(), out.nodes.end(), out_nodes);
    std::copy(out.entries.begin(), out.entries.end(), out_entries);
    std::copy(out.group_root.begin(), out.group_root.end(), out_group_root);
    for (int a = 0; a < 3; ++a) {
        out_bounds[a] = out.bounds.lo[a], out_bounds[3 + a] = out.bounds.hi[a];
    }
    out_counts[0] = uint32_t(out.nodes.size()), out_counts[1] = uint32_t(out.entries.size());
    return true;
}

// the trees below `roots` are trees: links inside the array, every node reached at most once (what keeps the collapse kernel's
// frontier and output inside their n_nodes slots)
inline bool check_forest(const rayhip_bvh2_node *nodes, const uint32_t n_nodes, const uint32_t *roots, const uint32_t n_roots, std::string &why) {
    std::vector<uint8_t> seen(n_nodes, 0);
    std::vector<uint32_t> stack;
    for (uint32_t r = 0; r < n_roots; ++r) {
        stack.push_back(roots[r]);
        while (!stack.empty()) {
            const uint32_t n = stack.back();
            stack.pop_back();
            if (n >= n_nodes || seen[n]) {
                why = n >= n_nodes ? "a link leaves the node array" : "a node is reached twice";
                return false;
            }
            seen[n] = 1;
            for (const uint32_t c : {nodes[n].left_child, nodes[n].right_child}) {
                if (!rayhip_bvh4::is_leaf(c)) {
                    stack.push_back(c);
                }
            }
        }
    }
    return true;
}

// rayhip_bvh4::build (the host driver) over a list of roots: a top level is made up whose leaves are instances 0 .. n_roots - 1 in
// order, instance r standing on roots[r].  Returns 0, 1 (why) or 2 (cannot be quantised).
inline int collapse_host(const rayhip_bvh2_node *nodes, const uint32_t n_nodes, const uint32_t *roots, const uint32_t n_roots, rt::Bvh4Node *out_wide,
                         uint32_t *out_roots4, uint32_t *out_count, std::string &why) {
    *out_count = 0;
    if (n_roots == 0) {
        return 0;
    }
    if (!check_forest(nodes, n_nodes, roots, n_roots, why)) {
        return 1;
    }
    std::vector<rayhip_bvh2_node> all(nodes, nodes + n_nodes);
    std::vector<rayhip_mesh_instance> mis(n_roots);
    for (uint32_t r = 0; r < n_roots; ++r) {
        mis[r] = rayhip_mesh_instance{};
        mis[r].node_index = roots[r];
        rayhip_bvh2_node t = {};
        t.left_child = (1u << 29) | r;
        t.right_child = r + 1 < n_roots ? n_nodes + r + 1 : ((1u << 29) | r);
        all.push_back(t); // (the last one names its instance twice: built once)
    }
    const rayhip_bvh4::Result res = rayhip_bvh4::build(all.data(), uint32_t(all.size()), mis.data(), n_roots, n_nodes);
    if (!res.ok) {
        return 2; // (the forest was checked above: what is left is a box the grid cannot hold)
    }
    if (res.nodes.size() > n_nodes) {
        why = "more wide nodes than BVH2 nodes";
        return 1;
    }
    std::copy(res.nodes.begin(), res.nodes.end(), out_wide);
    std::copy(res.blas_root4.begin(), res.blas_root4.end(), out_roots4);
    *out_count = uint32_t(res.nodes.size());
    return 0;
}

// one item of rayhip_k_bvh4_test_nodes: host and device run this very function
RT_HD void test_node_item(const rt::Bvh4Node *wide, const uint32_t node, const float *o, const float *d, const float t, uint32_t *out_ref,
                          uint32_t *out_n_hit, float *out_dist) {
    const rt::f3 inv_d = rt::safe_invert(rt::f3{d[0], d[1], d[2]});
    uint32_t ref[4], n_hit;
    float dist[4];
    rt::bvh4_test_node(wide, node, rt::f3{o[0], o[1], o[2]}, inv_d, t, ref, n_hit, dist);
    for (int c = 0; c < 4; ++c) {
        out_ref[c] = ref[c], out_dist[c] = dist[c];
    }
    *out_n_hit = n_hit;
}

inline bool check_items(const uint32_t *node_index, const uint32_t n_items, const uint32_t n_wide, std::string &why) {
    for (uint32_t i = 0; i < n_items; ++i) {
        if (node_index[i] >= n_wide) {
            why = "an item names a node outside the array";
            return false;
        }
    }
    return true;
}

} // namespace rayhip_bvh_hooks
