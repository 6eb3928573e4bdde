// refit.h -- what a vertex update (rayhip_scene_update_vertices) recomputes under a KEPT tree: the precomputed triangle
// records and the child boxes of the bottom-level BVH2 nodes.  Element functions shared by the device kernels
// (refit.hip.h) and a plain-loop host driver (tests/hostsim/hostsim_refit.cpp), like lbvh.h / rt_cache.h: IEEE operations
// without contraction on both sides, so both produce the same bits.
//
// Triangle record: the three planes of the reference's PreprocessTri (internal/Core.cpp:212-258) in its operation order
// -- edges, normal, squared length, the two edge planes divided by it, the normalised normal plane.  Checked over every
// fixture of tests/golden: the records a scene carries are this arithmetic applied to its corner positions, bit for bit.
// A triangle without area (squared normal length 0) gets an ALL-ZERO record: intersect_tri (rt_isect.h) computes det == 0
// for it and reports no hit.  (The reference drops such a triangle from the tree when it builds one; here the tree is kept.)
//
// Boxes: a child box of a BVH2 node is the exact min / max of the positions below it (min / max do not round, so a refit
// has one correct answer): a leaf's box from the corners of its entries, an inner child's from the two boxes its node holds.
// Nodes are refitted bottom-up by HEIGHT (1 + max over the children, a leaf child counting 0): all nodes of one height are
// independent of each other, and read only nodes of lower heights.
#pragma once

#include <stdint.h>

#include <vector>

#include "lbvh.h"

namespace rayhip_refit {

using rayhip_lbvh::Box;

constexpr uint32_t COUNT_BITS = 7u << 29, INDEX_BITS = ~COUNT_BITS;
constexpr uint32_t MAX_LEVELS = 128; // a tree higher than this is refused (one kernel launch per level)

// `degenerate`: the triangle has no area and got the all-zero record
RT_HD rayhip_tri_accel tri_accel_from_corners(const float p0[3], const float p1[3], const float p2[3], bool &degenerate) {
    rayhip_tri_accel out = {};
    const float e0[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
    const float e1[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
    float n[3] = {e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2], e0[0] * e1[1] - e0[1] * e1[0]};
    const float len2 = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
    degenerate = len2 == 0.0f;
    if (degenerate) {
        return out;
    }
    const float u[3] = {(e1[1] * n[2] - e1[2] * n[1]) / len2, (e1[2] * n[0] - e1[0] * n[2]) / len2, (e1[0] * n[1] - e1[1] * n[0]) / len2};
    out.u_plane[0] = u[0], out.u_plane[1] = u[1], out.u_plane[2] = u[2];
    out.u_plane[3] = -(u[0] * p0[0] + u[1] * p0[1] + u[2] * p0[2]);
    const float v[3] = {(n[1] * e0[2] - n[2] * e0[1]) / len2, (n[2] * e0[0] - n[0] * e0[2]) / len2, (n[0] * e0[1] - n[1] * e0[0]) / len2};
    out.v_plane[0] = v[0], out.v_plane[1] = v[1], out.v_plane[2] = v[2];
    out.v_plane[3] = -(v[0] * p0[0] + v[1] * p0[1] + v[2] * p0[2]);
    const float len = sqrtf(len2);
    n[0] /= len, n[1] /= len, n[2] /= len;
    out.n_plane[0] = n[0], out.n_plane[1] = n[1], out.n_plane[2] = n[2];
    out.n_plane[3] = n[0] * p0[0] + n[1] * p0[1] + n[2] * p0[2];
    return out;
}

// the record of tris[] entry `entry`; false: the entry names no triangle of the arrays (a free slot of the sparse pools,
// which no leaf reaches -- scene_validate.h) and keeps what it holds
RT_HD bool entry_tri_accel(const uint32_t entry, const uint32_t *tri_indices, const uint32_t *vtx_indices, const uint32_t n_tris,
                           const rayhip_vertex *vertices, const uint32_t n_vertices, rayhip_tri_accel &out, bool &degenerate) {
    const uint32_t t = tri_indices[entry];
    if (t >= n_tris) {
        return false;
    }
    const uint32_t i0 = vtx_indices[size_t(t) * 3], i1 = vtx_indices[size_t(t) * 3 + 1], i2 = vtx_indices[size_t(t) * 3 + 2];
    if (i0 >= n_vertices || i1 >= n_vertices || i2 >= n_vertices) {
        return false;
    }
    out = tri_accel_from_corners(vertices[i0].p, vertices[i1].p, vertices[i2].p, degenerate);
    return true;
}

// box of the leaf word (count - 1) << 29 | first: the corners of entries first .. first + count - 1
// (entry -> tri_indices -> vtx_indices -> vertices; the ranges of reachable leaves were checked at upload)
RT_HD Box leaf_box(const uint32_t word, const uint32_t *tri_indices, const uint32_t *vtx_indices, const rayhip_vertex *vertices) {
    Box b = rayhip_lbvh::empty_box();
    const uint32_t first = word & INDEX_BITS, count = ((word & COUNT_BITS) >> 29) + 1;
    for (uint32_t e = first; e < first + count; ++e) {
        const size_t t = tri_indices[e];
        for (int k = 0; k < 3; ++k) {
            rayhip_lbvh::grow_point(b, vertices[vtx_indices[t * 3 + k]].p);
        }
    }
    return b;
}

// box of an inner child: the union of the two child boxes its node holds
RT_HD Box inner_box(const rayhip_bvh2_node &n) {
    Box b;
    b.lo[0] = fminf(n.ch_data0[0], n.ch_data1[0]), b.hi[0] = fmaxf(n.ch_data0[1], n.ch_data1[1]);
    b.lo[1] = fminf(n.ch_data0[2], n.ch_data1[2]), b.hi[1] = fmaxf(n.ch_data0[3], n.ch_data1[3]);
    b.lo[2] = fminf(n.ch_data2[0], n.ch_data2[2]), b.hi[2] = fmaxf(n.ch_data2[1], n.ch_data2[3]);
    return b;
}

// the two child boxes of node `i` from what lies below it (inner children: already refitted); the links stay
RT_HD void refit_node(rayhip_bvh2_node *nodes, const uint32_t i, const uint32_t *tri_indices, const uint32_t *vtx_indices,
                      const rayhip_vertex *vertices) {
    const uint32_t link[2] = {nodes[i].left_child, nodes[i].right_child};
    Box b[2];
    for (int k = 0; k < 2; ++k) {
        b[k] = (link[k] & COUNT_BITS) ? leaf_box(link[k], tri_indices, vtx_indices, vertices) : inner_box(nodes[link[k]]);
    }
    rayhip_bvh2_node &n = nodes[i];
    n.ch_data0[0] = b[0].lo[0], n.ch_data0[1] = b[0].hi[0], n.ch_data0[2] = b[0].lo[1], n.ch_data0[3] = b[0].hi[1];
    n.ch_data1[0] = b[1].lo[0], n.ch_data1[1] = b[1].hi[0], n.ch_data1[2] = b[1].lo[1], n.ch_data1[3] = b[1].hi[1];
    n.ch_data2[0] = b[0].lo[2], n.ch_data2[1] = b[0].hi[2], n.ch_data2[2] = b[1].lo[2], n.ch_data2[3] = b[1].hi[2];
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
// The nodes below `roots` sorted by height: level_nodes[level_offset[h - 1] .. level_offset[h]) are the nodes of height h
// (h = 1: both children are leaves).  0 = ok, 1 = not a forest of trees inside the array, 2 = higher than MAX_LEVELS.
inline int plan_levels(const rayhip_bvh2_node *nodes, const uint32_t n_nodes, const std::vector<uint32_t> &roots,
                       std::vector<uint32_t> &level_nodes, std::vector<uint32_t> &level_offset) {
    level_nodes.clear(), level_offset.assign(1, 0u);
    std::vector<uint8_t> height(n_nodes, 0); // 0 = not visited, 255 = on the stack
    std::vector<uint32_t> stack, order;
    for (const uint32_t root : roots) {
        if (root >= n_nodes) {
            return 1;
        }
        if (height[root] != 0) {
            continue;
        }
        stack.assign(1, root);
        while (!stack.empty()) {
            const uint32_t w = stack.back();
            const uint32_t link[2] = {nodes[w].left_child, nodes[w].right_child};
            if (height[w] == 0) { // first visit: the children go first
                height[w] = 255;
                if ((link[0] & COUNT_BITS) == 0 && link[0] == link[1]) {
                    return 1;
                }
                for (int k = 0; k < 2; ++k) {
                    if ((link[k] & COUNT_BITS) == 0) {
                        if (link[k] >= n_nodes || height[link[k]] != 0) {
                            return 1; // outside the array, a cycle or a node with two parents
                        }
                        stack.push_back(link[k]);
                    }
                }
                continue;
            }
            stack.pop_back();
            uint32_t h = 0;
            for (int k = 0; k < 2; ++k) {
                h = std::max<uint32_t>(h, (link[k] & COUNT_BITS) ? 0u : height[link[k]]);
            }
            if (h + 1 > MAX_LEVELS) {
                return 2;
            }
            height[w] = uint8_t(h + 1);
            order.push_back(w);
        }
    }
    uint32_t levels = 0;
    for (const uint32_t w : order) {
        levels = std::max<uint32_t>(levels, height[w]);
    }
    level_offset.assign(size_t(levels) + 1, 0u);
    for (const uint32_t w : order) {
        ++level_offset[height[w]];
    }
    for (uint32_t h = 1; h <= levels; ++h) {
        level_offset[h] += level_offset[h - 1];
    }
    level_nodes.resize(order.size());
    std::vector<uint32_t> at(level_offset.begin(), level_offset.end());
    for (const uint32_t w : order) {
        level_nodes[at[height[w] - 1]++] = w;
    }
    return 0;
}

// per triangle the lowest tris[] entry that names it (0xffffffff: none): the entry that counts a triangle without area once,
// however often the leaves repeat it (the reference pads its leaves with repeats, the leaf refinement doubles a lone triangle)
inline std::vector<uint32_t> first_entries(const uint32_t *tri_indices, const uint32_t n_entries, const uint32_t n_tris) {
    std::vector<uint32_t> first(n_tris, 0xffffffffu);
    for (uint32_t e = n_entries; e-- > 0;) {
        if (tri_indices[e] < n_tris) {
            first[tri_indices[e]] = e;
        }
    }
    return first;
}

// plain-loop drivers over the element functions: every record (un-pitched) + the number of triangles without area ...
inline uint32_t refit_tris_host(const rayhip_vertex *vertices, const uint32_t n_vertices, const uint32_t *vtx_indices, const uint32_t n_tris,
                                const uint32_t *tri_indices, const uint32_t n_entries, rayhip_tri_accel *tris) {
    const std::vector<uint32_t> first = first_entries(tri_indices, n_entries, n_tris);
    uint32_t n_degenerate = 0;
    for (uint32_t e = 0; e < n_entries; ++e) {
        rayhip_tri_accel rec;
        bool degenerate = false;
        if (entry_tri_accel(e, tri_indices, vtx_indices, n_tris, vertices, n_vertices, rec, degenerate)) {
            tris[e] = rec;
            n_degenerate += degenerate && first[tri_indices[e]] == e ? 1u : 0u;
        }
    }
    return n_degenerate;
}

// ... and the boxes of the nodes below `roots`, level by level (0 / 1 / 2 as plan_levels)
inline int refit_nodes_host(rayhip_bvh2_node *nodes, const uint32_t n_nodes, const std::vector<uint32_t> &roots, const uint32_t *tri_indices,
                            const uint32_t *vtx_indices, const rayhip_vertex *vertices) {
    std::vector<uint32_t> level_nodes, level_offset;
    const int rc = plan_levels(nodes, n_nodes, roots, level_nodes, level_offset);
    if (rc) {
        return rc;
    }
    for (const uint32_t w : level_nodes) { // (sorted by height: a node comes after everything below it)
        refit_node(nodes, w, tri_indices, vtx_indices, vertices);
    }
    return 0;
}

} // namespace rayhip_refit
