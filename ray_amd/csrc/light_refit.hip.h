// light_refit.hip.h -- the device side of the light refit (rayhip_scene_refit_lights; refit_after_vertices in rayhip_deform.hip.h): the
// element functions of light_refit.h.  The tree is refitted with ONE LAUNCH PER HEIGHT, lowest first, as refit.hip.h refits the BVH:
// a launch reads the summaries the launches before it wrote, and the kernel boundary is what makes them visible -- no flags between
// waves.  Within a launch EIGHT LANES share a node, one per child slot (eight nodes per wavefront): the box union and the fold in
// slot order go through __shfl inside the group of eight, and the three light_children rows of a slot are written by its lane, so
// that the eight lanes of a node write 128 consecutive bytes per row type.
#pragma once

#include <hip/hip_runtime.h>

#include "light_refit.h"

namespace rayhip_light_refit {

// one lane per entry of li_indices; the lanes whose light is a triangle write its four light_tri_geom rows and its leaf summary.
// `n_degenerate` counts the triangles without area.
__global__ void __launch_bounds__(256) k_refit_tri_lights(const rayhip_light *__restrict__ lights, const uint32_t n_lights, const uint32_t *__restrict__ li_indices,
                                                         const uint32_t n_li, const rayhip_mesh_instance *__restrict__ instances, const uint32_t n_instances,
                                                         const uint32_t *__restrict__ vtx_indices, const uint32_t n_vtx_indices,
                                                         const rayhip_vertex *__restrict__ vertices, const uint32_t n_vertices, float4 *__restrict__ tri_geom,
                                                         Summary *__restrict__ leaf, uint32_t *__restrict__ n_degenerate) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_li) {
        return;
    }
    const uint32_t i = li_indices[k];
    if (i >= n_lights) {
        return;
    }
    const rayhip_light l = lights[i];
    if (light_type(l) != LIGHT_TYPE_TRI) {
        return;
    }
    const uint32_t tri = float_as_uint(l.params[0]), mi = float_as_uint(l.params[1]);
    if (mi >= n_instances || uint64_t(tri) * 3 + 2 >= n_vtx_indices) { // (an upload checks both; never followed unchecked)
        return;
    }
    if (vtx_indices[tri * 3] >= n_vertices || vtx_indices[tri * 3 + 1] >= n_vertices || vtx_indices[tri * 3 + 2] >= n_vertices) {
        return;
    }
    float4 geom[4];
    Summary s;
    const bool has_area = tri_light_summary(l, instances, vtx_indices, vertices, geom, s);
    float4 *rows = tri_geom + size_t(i) * 4;
    rows[0] = geom[0], rows[1] = geom[1], rows[2] = geom[2], rows[3] = geom[3];
    float4 *out = reinterpret_cast<float4 *>(leaf + i); // (48-byte records in a 16-byte-aligned array)
    out[0] = float4{s.lo[0], s.lo[1], s.lo[2], s.hi[0]};
    out[1] = float4{s.hi[1], s.hi[2], s.flux, s.axis[0]};
    out[2] = float4{s.axis[1], s.axis[2], s.omega_n, s.omega_e};
    if (!has_area) {
        atomicAdd(n_degenerate, 1u);
    }
}

__device__ __forceinline__ Summary load_summary(const Summary *p) {
    const float4 *q = reinterpret_cast<const float4 *>(p);
    const float4 a = q[0], b = q[1], c = q[2];
    Summary s;
    s.lo[0] = a.x, s.lo[1] = a.y, s.lo[2] = a.z, s.hi[0] = a.w, s.hi[1] = b.x, s.hi[2] = b.y, s.flux = b.z, s.axis[0] = b.w;
    s.axis[1] = c.x, s.axis[2] = c.y, s.omega_n = c.z, s.omega_e = c.w;
    return s;
}

// eight lanes per node of ONE height: level_nodes[0 .. n) name them, lane (g * 8 + i) of the launch has slot i of node g.
// Reads the leaf table, the summaries of lower heights, the slot's flux scale (8 per node) and `posed` (one byte per light slot, or
// null: light_refit.h, posed_leaf), writes its node, the node's summary and its light_children rows.
// Every lane of a wavefront stays in the kernel to its end (the shuffles want their partners): a group past `n` and the lane of an
// empty slot only skip their loads and stores.
__global__ void __launch_bounds__(256) k_refit_light_level(rayhip_light_cwbvh_node *nodes, const uint32_t *__restrict__ level_nodes, const uint32_t n,
                                                          const rayhip_light *__restrict__ lights, const Summary *__restrict__ leaf, Summary *node_summary,
                                                          float4 *__restrict__ children, const float *__restrict__ slot_scale,
                                                          const uint8_t *__restrict__ posed) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t g = t >> 3;
    const int i = int(t & 7u);
    const bool live = g < n;
    const uint32_t w = live ? level_nodes[g] : 0u;
    rayhip_light_cwbvh_node *node = nodes + w;
    const uint32_t link = live ? node->child[i] : EMPTY_SLOT;
    const bool used = link != EMPTY_SLOT;
    Summary c = {};
    if (used) {
        c = load_summary((link & LEAF_NODE_BIT) ? leaf + (link & PRIM_INDEX_BITS) : node_summary + link);
    }
    const bool finite = used && finite_box(c);
    // the node's box: the union over the lanes with a finite child (min / max: exact in any order)
    float nlo[3], nhi[3];
    for (int a = 0; a < 3; ++a) {
        nlo[a] = finite ? c.lo[a] : FLT_MAX, nhi[a] = finite ? c.hi[a] : -FLT_MAX;
    }
    int any_finite = finite ? 1 : 0;
    for (int d = 1; d < 8; d <<= 1) {
        for (int a = 0; a < 3; ++a) {
            nlo[a] = min2(nlo[a], __shfl_xor(nlo[a], d, 8)), nhi[a] = max2(nhi[a], __shfl_xor(nhi[a], d, 8));
        }
        any_finite |= __shfl_xor(any_finite, d, 8);
    }
    // a copy of the node that holds its box and THIS lane's slot at index 0: what decode_light_child reads of slot i
    rayhip_light_cwbvh_node mine = {};
    if (live) {
        for (int a = 0; a < 3; ++a) {
            mine.bbox_min[a] = any_finite ? nlo[a] : node->bbox_min[a], mine.bbox_max[a] = any_finite ? nhi[a] : node->bbox_max[a];
            mine.ch_bbox_min[a][0] = node->ch_bbox_min[a][i], mine.ch_bbox_max[a][0] = node->ch_bbox_max[a][i];
        }
        mine.flux[0] = node->flux[i], mine.axis[0] = node->axis[i], mine.cos_omega_ne[0] = node->cos_omega_ne[i];
    }
    if (used) {
        Slot slot;
        slot.flux = mine.flux[0], slot.axis = mine.axis[0], slot.cosines = mine.cos_omega_ne[0];
        refit_slot(c, slot_takes_cone(link, lights, posed), slot_flux_scale(link, slot_scale, w, i), nlo, nhi, slot, stored_cos_e(link, lights, posed));
        for (int a = 0; a < 3; ++a) {
            node->ch_bbox_min[a][i] = mine.ch_bbox_min[a][0] = slot.lo[a], node->ch_bbox_max[a][i] = mine.ch_bbox_max[a][0] = slot.hi[a];
        }
        node->flux[i] = mine.flux[0] = slot.flux, node->axis[i] = mine.axis[0] = slot.axis, node->cos_omega_ne[i] = mine.cos_omega_ne[0] = slot.cosines;
    }
    // the node's own summary: the fold over the slots in the order 0..7, every lane of the group the same steps on the same values
    Summary own;
    make_infinite(own);
    own.flux = 0.0f, own.axis[0] = 0.0f, own.axis[1] = 1.0f, own.axis[2] = 0.0f, own.omega_n = 0.0f, own.omega_e = 0.0f;
    if (any_finite) {
        for (int a = 0; a < 3; ++a) {
            own.lo[a] = nlo[a], own.hi[a] = nhi[a];
        }
    }
    bool started = false;
    for (int j = 0; j < 8; ++j) {
        Summary cj;
        const int used_j = __shfl(used ? 1 : 0, j, 8);
        cj.flux = __shfl(c.flux, j, 8);
        cj.axis[0] = __shfl(c.axis[0], j, 8), cj.axis[1] = __shfl(c.axis[1], j, 8), cj.axis[2] = __shfl(c.axis[2], j, 8);
        cj.omega_n = __shfl(c.omega_n, j, 8), cj.omega_e = __shfl(c.omega_e, j, 8);
        if (used_j) {
            fold_child(own, started, cj);
            started = true;
        }
    }
    if (!live) {
        return; // (behind the last shuffle)
    }
    if (i == 0) {
        if (any_finite) {
            for (int a = 0; a < 3; ++a) {
                node->bbox_min[a] = nlo[a], node->bbox_max[a] = nhi[a];
            }
        }
        float4 *out = reinterpret_cast<float4 *>(node_summary + w);
        out[0] = float4{own.lo[0], own.lo[1], own.lo[2], own.hi[0]};
        out[1] = float4{own.hi[1], own.hi[2], own.flux, own.axis[0]};
        out[2] = float4{own.axis[1], own.axis[2], own.omega_n, own.omega_e};
    }
    // light_children: rows [2 + 8 r + i] of the node (fill_light_children's layout); its rows 0 and 1 hold the links, which a refit keeps
    const LightChild lc = decode_light_child(mine, 0);
    float4 *rows = children + size_t(w) * LIGHT_CHILDREN_STRIDE + 2;
    rows[0 * 8 + i] = lc.axis_extent, rows[1 * 8 + i] = lc.centre_valid, rows[2 * 8 + i] = lc.cosines;
}

} // namespace rayhip_light_refit
