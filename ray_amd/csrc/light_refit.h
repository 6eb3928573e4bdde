// light_refit.h -- what a vertex update or a pose recomputes of the LIGHTS when rayhip_scene_refit_lights is on: the world-space
// corners of the triangle lights (light_tri_geom), the 8-wide light tree (light_cwnodes: node boxes, quantised child boxes, flux,
// cone axis and cosines per slot) and the per-node importance rows derived from it (light_children).  The tree's TOPOLOGY is kept,
// as the vertex update keeps the BVH's.  Element functions shared by the device kernels (light_refit.hip.h) and a plain-loop host
// driver (tests/hostsim/hostsim_lights.cpp), like refit.h and skin.h: IEEE operations in a STATED ORDER without contraction on both
// sides, the project's polynomial acos / cos (rt_rng.h) where a libm would differ between the two, so both produce the same bits.
//
// Summary (12 floats) of a light or of a subtree: box lo/hi, flux, cone axis, omega_n (half-angle of the normals), omega_e (emission
// half-angle).  lo[0] == -MAX_DIST marks an infinite emitter (directional, environment).
//   triangle light   p1..p3 = the instance transform of the three vertices (fill_light_tri_geom's arithmetic: ((m0*x + m4*y) + m8*z) + m12);
//                    box = min / max of the corners; n = cross(p2 - p1, p3 - p1) (each component a*b - c*d); len = sqrtf((nx*nx + ny*ny) + nz*nz);
//                    flux = ((col.r + col.g) + col.b) * (0.5f * len); axis = n / len; omega_n = PI if doublesided else 0; omega_e = PI / 2.
//                    A triangle without area (len is 0 or not finite): flux 0, axis (0, 1, 0) -- it can never be picked.
//   other lights     do not move with vertices: computed once on the host (static_light_summary), flux taken from the uploaded tree;
//                    one that rayhip_scene_set_lights replaced (light_pose.h) is complete, flux included, and marked in `posed`.
// Node N, slots in the order 0..7, a slot being empty when child[i] == 0x7fffffff:
//   box      the union of the FINITE children's boxes (min / max: exact in any order); without a finite child bbox_min/max keep their bytes
//   per slot finite child: ch_bbox_min = floorf(q(lo)), ch_bbox_max = ceilf(q(hi)), q(v) = clamp((255 * (v - nlo)) / (nhi - nlo), 0, 255) and
//            0 where nlo == nhi; infinite child: min bytes 0xff, max bytes 0; empty slot: untouched.
//            Triangle-light leaves and inner children also get flux, the octahedral axis and the two cosines (cos omega_n,
//            max(cos omega_e, 0)), and so do the leaves of lights marked in `posed`; the slots of other lights keep those three
//            words bytewise.
//            The flux of an INNER child's slot is the child's summed flux times the slot's SCALE: the ratio of the flux the uploaded
//            tree stores there to the sum a refit finds below it at the upload pose (slot_scales, once per upload).  The scene build
//            does not store the sum in every inner slot -- it hands a node's flux on to the parent once the node's left child is
//            counted, so a deeper right subtree arrives too late and such slots are up to half low -- and a refit keeps the tree it
//            was given: at an unchanged pose it gives the uploaded flux back, and a moved emitter changes a slot's flux by the
//            factor its sum changes by.  Where the stored flux is the sum, the scale is 1 to rounding.
//   summary  flux = the sum over the non-empty slots in slot order; the cone a fold in slot order: the first child initialises it,
//            each later child merges by  angle = acos(clamp(dot, -1, 1)), dot = (ax*bx + ay*by) + az*bz;  axis = (a + b) / |a + b| or
//            (0, 1, 0) when the sum has no length;  omega_n = min(0.5 * (an + max(an, angle + bn)), PI);  omega_e = max(ae, be).
// The scene build merges cones and sums flux in the order of its binary tree; the slot-order fold gives a valid tree that differs
// from a fresh build in the last bits of the inner fluxes and in the inner cones.
#pragma once

#include <stdint.h>

#include <vector>

#include "shade_lights.h"

namespace rayhip_light_refit {

using namespace rt;

constexpr uint32_t EMPTY_SLOT = 0x7fffffffu;
constexpr uint32_t MAX_LEVELS = 64; // heights of an 8-wide tree: 2^31 lights need 11

struct Summary {
    float lo[3], hi[3], flux, axis[3], omega_n, omega_e;
};
static_assert(sizeof(Summary) == 48, "12 floats");

RT_HD bool finite_box(const Summary &s) { return s.lo[0] > -MAX_DIST; }

RT_HD void make_infinite(Summary &s) {
    s.lo[0] = s.lo[1] = s.lo[2] = -MAX_DIST;
    s.hi[0] = s.hi[1] = s.hi[2] = MAX_DIST;
}

// min / max as selects: the same bits on both sides and IN ANY ORDER, also for zeros of either sign (-0 is the smaller one)
RT_HD float min2(const float a, const float b) { return (b < a || (b == a && (float_as_uint(b) >> 31) != 0)) ? b : a; }
RT_HD float max2(const float a, const float b) { return (b > a || (b == a && (float_as_uint(b) >> 31) == 0)) ? b : a; }
RT_HD float min3(const float a, const float b, const float c) { return min2(a, min2(b, c)); }
RT_HD float max3(const float a, const float b, const float c) { return max2(a, max2(b, c)); }

// the four light_tri_geom rows and the summary of the triangle light `l`; false: the triangle has no area
RT_HD bool tri_light_summary(const rayhip_light &l, const rayhip_mesh_instance *instances, const uint32_t *vtx_indices, const rayhip_vertex *vertices,
                             float4 *geom /* [4] */, Summary &s) {
    fill_light_tri_geom(l, instances, vtx_indices, vertices, geom);
    const f3 p1 = f3{geom[0].x, geom[0].y, geom[0].z}, p2 = f3{geom[1].x, geom[1].y, geom[1].z}, p3 = f3{geom[2].x, geom[2].y, geom[2].z};
    s.lo[0] = min3(p1.x, p2.x, p3.x), s.lo[1] = min3(p1.y, p2.y, p3.y), s.lo[2] = min3(p1.z, p2.z, p3.z);
    s.hi[0] = max3(p1.x, p2.x, p3.x), s.hi[1] = max3(p1.y, p2.y, p3.y), s.hi[2] = max3(p1.z, p2.z, p3.z);
    const f3 n = cross(p2 - p1, p3 - p1);
    const float len = sqrtf((n.x * n.x + n.y * n.y) + n.z * n.z);
    s.omega_n = light_doublesided(l) ? PI : 0.0f;
    s.omega_e = PI / 2.0f;
    if (!(len > 0.0f) || !(len <= 3.402823466e+38f)) {
        s.flux = 0.0f;
        s.axis[0] = 0.0f, s.axis[1] = 1.0f, s.axis[2] = 0.0f;
        return false;
    }
    const float lum = (l.col[0] + l.col[1]) + l.col[2];
    s.flux = lum * (0.5f * len);
    s.axis[0] = n.x / len, s.axis[1] = n.y / len, s.axis[2] = n.z / len;
    return true;
}

// ---- the encodings of a slot ------------------------------------------------------------------------------------------------------
RT_HD float quantise(const float v, const float lo, const float hi) {
    if (lo == hi) {
        return 0.0f;
    }
    return clampf((255.0f * (v - lo)) / (hi - lo), 0.0f, 255.0f);
}
RT_HD uint32_t snorm16(const float f) { return uint32_t(roundf(clampf((f + 1.0f) / 2.0f, 0.0f, 1.0f) * 65535.0f)) & 0xffffu; }
// octahedral, 2 x 16 bit: the direction over its 1-norm, the lower hemisphere folded over the diagonals
RT_HD uint32_t encode_axis(const float d[3]) {
    const float denom = (fabsf(d[0]) + fabsf(d[1])) + fabsf(d[2]);
    const float v[3] = {d[0] / denom, d[1] / denom, d[2] / denom};
    if (v[2] < 0.0f) {
        return (snorm16((1.0f - fabsf(v[1])) * copysignf(1.0f, v[0])) << 16) | snorm16((1.0f - fabsf(v[0])) * copysignf(1.0f, v[1]));
    }
    return (snorm16(v[0]) << 16) | snorm16(v[1]);
}
RT_HD uint32_t encode_cosines(const float cos_n, const float cos_e) {
    const uint32_t a = uint32_t(floorf(65534.0f * ((cos_n + 1.0f) / 2.0f))), b = uint32_t(floorf(65534.0f * ((cos_e + 1.0f) / 2.0f)));
    return (a << 16) | b;
}

// the words of one slot a refit may write: in = what the node holds, out = what it holds afterwards
struct Slot {
    uint8_t lo[3], hi[3];
    float flux;
    uint32_t axis, cosines;
};

// slot of a non-empty child with summary `c` under a node whose box is [nlo, nhi] (valid when some child is finite, which a finite
// `c` implies).  `cone_too`: a triangle-light leaf, a posed leaf or an inner child; `flux_scale`: the slot's scale (1 for a leaf: its flux
// goes in as it is); `stored_cos_e`: where the cosine of omega_e stands as a libm computed it (stored_cos_e below), or null.
RT_HD void refit_slot(const Summary &c, const bool cone_too, const float flux_scale, const float nlo[3], const float nhi[3], Slot &slot,
                      const float *stored_cos_e = nullptr) {
    if (finite_box(c)) {
        for (int a = 0; a < 3; ++a) {
            slot.lo[a] = uint8_t(floorf(quantise(c.lo[a], nlo[a], nhi[a])));
            slot.hi[a] = uint8_t(ceilf(quantise(c.hi[a], nlo[a], nhi[a])));
        }
    } else {
        slot.lo[0] = slot.lo[1] = slot.lo[2] = 0xff;
        slot.hi[0] = slot.hi[1] = slot.hi[2] = 0;
    }
    if (cone_too) {
        slot.flux = flux_scale == 1.0f ? c.flux : c.flux * flux_scale;
        slot.axis = encode_axis(c.axis);
        slot.cosines = encode_cosines(portable_cos(c.omega_n), max2(stored_cos_e ? *stored_cos_e : portable_cos(c.omega_e), 0.0f));
    }
}

// one step of the fold in slot order: `acc` (started: some earlier child went in) takes the child `c`
RT_HD void fold_child(Summary &acc, const bool started, const Summary &c) {
    if (!started) {
        acc.flux = c.flux;
        acc.axis[0] = c.axis[0], acc.axis[1] = c.axis[1], acc.axis[2] = c.axis[2];
        acc.omega_n = c.omega_n, acc.omega_e = c.omega_e;
        return;
    }
    acc.flux = acc.flux + c.flux;
    const float d = (acc.axis[0] * c.axis[0] + acc.axis[1] * c.axis[1]) + acc.axis[2] * c.axis[2];
    const float angle = portable_acosf(clampf(d, -1.0f, 1.0f));
    const float sum[3] = {acc.axis[0] + c.axis[0], acc.axis[1] + c.axis[1], acc.axis[2] + c.axis[2]};
    const float len = sqrtf((sum[0] * sum[0] + sum[1] * sum[1]) + sum[2] * sum[2]);
    if (len != 0.0f) {
        acc.axis[0] = sum[0] / len, acc.axis[1] = sum[1] / len, acc.axis[2] = sum[2] / len;
    } else {
        acc.axis[0] = 0.0f, acc.axis[1] = 1.0f, acc.axis[2] = 0.0f;
    }
    acc.omega_n = min2(0.5f * (acc.omega_n + max2(acc.omega_n, angle + c.omega_n)), PI);
    acc.omega_e = max2(acc.omega_e, c.omega_e);
}

// what slot `link` of a node refers to: a leaf takes the light's summary, an inner child the one an earlier level wrote
RT_HD Summary child_summary(const uint32_t link, const Summary *leaf, const Summary *node_summary) {
    return (link & LEAF_NODE_BIT) ? leaf[link & PRIM_INDEX_BITS] : node_summary[link];
}
// `posed`: one byte per light slot, not zero where rayhip_scene_set_lights replaced the record (light_pose.h), or null for none.  The
// leaf of such a light takes flux, axis and cosines from its summary as a triangle light's does.
RT_HD bool posed_leaf(const uint32_t link, const uint8_t *posed) {
    return posed != nullptr && (link & LEAF_NODE_BIT) != 0 && posed[link & PRIM_INDEX_BITS] != 0;
}
RT_HD bool slot_takes_cone(const uint32_t link, const rayhip_light *lights, const uint8_t *posed = nullptr) {
    return (link & LEAF_NODE_BIT) == 0 || light_type(lights[link & PRIM_INDEX_BITS]) == LIGHT_TYPE_TRI || posed_leaf(link, posed);
}
// The scene build encodes cosf(omega_e).  Every angle a summary holds is 0, PI / 2 or PI, where portable_cos gives what cosf gives,
// but a directional light's: its cosine is taken from the record, where AddLight stored cosf(angle) (dir.cos_angle, params[3]).
RT_HD const float *stored_cos_e(const uint32_t link, const rayhip_light *lights, const uint8_t *posed) {
    return posed_leaf(link, posed) && light_type(lights[link & PRIM_INDEX_BITS]) == LIGHT_TYPE_DIR ? &lights[link & PRIM_INDEX_BITS].params[3] : nullptr;
}

// the scale of slot i of node w: the table's entry for an inner child, 1 for a leaf
RT_HD float slot_flux_scale(const uint32_t link, const float *slot_scale, const uint32_t w, const int i) {
    return (slot_scale != nullptr && (link & LEAF_NODE_BIT) == 0) ? slot_scale[size_t(w) * 8 + i] : 1.0f;
}

// node `w` as ONE thread refits it (the host driver; the device kernel spreads the same functions over eight lanes)
// `slot_scale`: 8 per node (slot_scales), or null for 1 everywhere; `posed`: one byte per light slot (posed_leaf), or null
RT_HD void refit_light_node(rayhip_light_cwbvh_node *nodes, const uint32_t w, const rayhip_light *lights, const Summary *leaf, Summary *node_summary,
                            float4 *children, const float *slot_scale, const uint8_t *posed = nullptr) {
    rayhip_light_cwbvh_node &n = nodes[w];
    Summary c[8], own;
    float nlo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, nhi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    bool any_finite = false, started = false;
    for (int i = 0; i < 8; ++i) {
        if (n.child[i] == EMPTY_SLOT) {
            continue;
        }
        c[i] = child_summary(n.child[i], leaf, node_summary);
        if (finite_box(c[i])) {
            any_finite = true;
            for (int a = 0; a < 3; ++a) {
                nlo[a] = min2(nlo[a], c[i].lo[a]), nhi[a] = max2(nhi[a], c[i].hi[a]);
            }
        }
    }
    make_infinite(own);
    own.flux = 0.0f, own.axis[0] = 0.0f, own.axis[1] = 1.0f, own.axis[2] = 0.0f, own.omega_n = 0.0f, own.omega_e = 0.0f;
    if (any_finite) {
        for (int a = 0; a < 3; ++a) {
            n.bbox_min[a] = own.lo[a] = nlo[a], n.bbox_max[a] = own.hi[a] = nhi[a];
        }
    }
    for (int i = 0; i < 8; ++i) {
        if (n.child[i] == EMPTY_SLOT) {
            continue;
        }
        Slot slot;
        slot.flux = n.flux[i], slot.axis = n.axis[i], slot.cosines = n.cos_omega_ne[i];
        refit_slot(c[i], slot_takes_cone(n.child[i], lights, posed), slot_flux_scale(n.child[i], slot_scale, w, i), nlo, nhi, slot,
                   stored_cos_e(n.child[i], lights, posed));
        for (int a = 0; a < 3; ++a) {
            n.ch_bbox_min[a][i] = slot.lo[a], n.ch_bbox_max[a][i] = slot.hi[a];
        }
        n.flux[i] = slot.flux, n.axis[i] = slot.axis, n.cos_omega_ne[i] = slot.cosines;
        fold_child(own, started, c[i]);
        started = true;
    }
    node_summary[w] = own;
    fill_light_children(n, children + size_t(w) * LIGHT_CHILDREN_STRIDE);
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
// The nodes sorted by height: level_nodes[level_offset[h] .. level_offset[h + 1]) are those of height h (0: all children are leaves).
// A parent lies before its children in the array (the order the scene build's flattening gives), which is what is checked:
// 0 = ok, 1 = a link outside the arrays or against that order, 2 = higher than MAX_LEVELS.
inline int plan_levels(const rayhip_light_cwbvh_node *nodes, const uint32_t n_nodes, const uint32_t n_lights, std::vector<uint32_t> &level_nodes,
                       std::vector<uint32_t> &level_offset) {
    level_nodes.clear(), level_offset.assign(1, 0u);
    std::vector<uint32_t> height(n_nodes, 0);
    uint32_t levels = 0;
    for (uint32_t w = n_nodes; w-- > 0;) {
        uint32_t h = 0;
        for (int i = 0; i < 8; ++i) {
            const uint32_t link = nodes[w].child[i];
            if (link == EMPTY_SLOT) {
                continue;
            }
            if (link & LEAF_NODE_BIT) {
                if ((link & PRIM_INDEX_BITS) >= n_lights) {
                    return 1;
                }
            } else if (link <= w || link >= n_nodes) {
                return 1;
            } else {
                h = std::max(h, height[link] + 1);
            }
        }
        if (h >= MAX_LEVELS) {
            return 2;
        }
        height[w] = h;
        levels = std::max(levels, h + 1);
    }
    level_offset.assign(size_t(levels) + 1, 0u);
    for (uint32_t w = 0; w < n_nodes; ++w) {
        ++level_offset[height[w] + 1];
    }
    for (uint32_t h = 1; h <= levels; ++h) {
        level_offset[h] += level_offset[h - 1];
    }
    level_nodes.resize(n_nodes);
    std::vector<uint32_t> at(level_offset.begin(), level_offset.end());
    for (uint32_t w = 0; w < n_nodes; ++w) {
        level_nodes[at[height[w]]++] = w;
    }
    return 0;
}

// box, axis and angles of a light that is NOT a triangle (it does not move with vertices), as the scene build computes them:
// sums from the left, cross products as a*b - c*d.  The flux is not set here (leaf_table takes it from the uploaded tree).
// (RT_HD: the host runs it once per upload, k_pose_lights once per record a call replaces.)
RT_HD void corner_box(const f3 *c, const int n, Summary &s) {
    for (int a = 0; a < 3; ++a) {
        s.lo[a] = FLT_MAX, s.hi[a] = -FLT_MAX;
    }
    for (int k = 0; k < n; ++k) {
        const float v[3] = {c[k].x, c[k].y, c[k].z};
        for (int a = 0; a < 3; ++a) {
            s.lo[a] = min2(s.lo[a], v[a]), s.hi[a] = max2(s.hi[a], v[a]);
        }
    }
}
RT_HD void static_light_summary(const rayhip_light &l, Summary &s) {
    const float *p = l.params;
    s.flux = 0.0f;
    s.axis[0] = 0.0f, s.axis[1] = 1.0f, s.axis[2] = 0.0f;
    s.lo[0] = s.lo[1] = s.lo[2] = s.hi[0] = s.hi[1] = s.hi[2] = 0.0f;
    s.omega_n = PI, s.omega_e = PI / 2.0f;
    const uint32_t type = light_type(l);
    if (type == LIGHT_TYPE_SPHERE) {
        const float r = p[7];
        for (int a = 0; a < 3; ++a) {
            s.lo[a] = p[a] - r, s.hi[a] = p[a] + r;
        }
    } else if (type == LIGHT_TYPE_DIR) {
        make_infinite(s);
        s.axis[0] = p[0], s.axis[1] = p[1], s.axis[2] = p[2];
        s.omega_n = 0.0f, s.omega_e = p[5];
    } else if (type == LIGHT_TYPE_LINE) {
        const f3 pos = f3{p[0], p[1], p[2]};
        f3 u = f3{p[4], p[5], p[6]}, dir = f3{p[8], p[9], p[10]};
        f3 v = cross(u, dir);
        u = u * p[7], v = v * p[7], dir = dir * (0.5f * p[11]);
        const f3 c[8] = {pos + dir + u + v, pos + dir + u - v, pos + dir - u + v, pos + dir - u - v,
                         pos - dir + u + v, pos - dir + u - v, pos - dir - u + v, pos - dir - u - v};
        corner_box(c, 8, s);
    } else if (type == LIGHT_TYPE_RECT || type == LIGHT_TYPE_DISK) {
        const f3 pos = f3{p[0], p[1], p[2]};
        const f3 u = f3{0.5f * p[4], 0.5f * p[5], 0.5f * p[6]}, v = f3{0.5f * p[8], 0.5f * p[9], 0.5f * p[10]};
        const f3 c[4] = {pos + u + v, pos + u - v, pos - u + v, pos - u - v};
        corner_box(c, 4, s);
        const f3 n = cross(u, v);
        const float len = sqrtf((n.x * n.x + n.y * n.y) + n.z * n.z);
        if (len > 0.0f && len <= 3.402823466e+38f) { // (a rect or disk without area keeps the axis (0, 1, 0), as a triangle without area does)
            s.axis[0] = n.x / len, s.axis[1] = n.y / len, s.axis[2] = n.z / len;
        }
        s.omega_n = light_doublesided(l) ? PI : 0.0f;
    } else if (type == LIGHT_TYPE_ENV) {
        make_infinite(s);
    }
}

// the leaf summary table, one record per light SLOT: lights that are not triangles complete (flux from the slot of the node that
// names them), triangle lights left zero -- every refit writes those
inline std::vector<Summary> leaf_table(const rayhip_light *lights, const uint32_t n_lights, const rayhip_light_cwbvh_node *nodes, const uint32_t n_nodes) {
    std::vector<Summary> leaf(n_lights, Summary{});
    for (uint32_t w = 0; w < n_nodes; ++w) {
        for (int i = 0; i < 8; ++i) {
            const uint32_t link = nodes[w].child[i];
            if (link == EMPTY_SLOT || (link & LEAF_NODE_BIT) == 0 || (link & PRIM_INDEX_BITS) >= n_lights) {
                continue;
            }
            const rayhip_light &l = lights[link & PRIM_INDEX_BITS];
            if (light_type(l) != LIGHT_TYPE_TRI) {
                static_light_summary(l, leaf[link & PRIM_INDEX_BITS]);
                leaf[link & PRIM_INDEX_BITS].flux = nodes[w].flux[i];
            }
        }
    }
    return leaf;
}

// plain-loop driver: geometry rows and summaries of the triangle lights li_indices names (returns those without area) ...
inline uint32_t refit_tri_lights_host(const rayhip_light *lights, const uint32_t n_lights, const uint32_t *li_indices, const uint32_t n_li,
                                      const rayhip_mesh_instance *instances, const uint32_t n_instances, const uint32_t *vtx_indices,
                                      const uint32_t n_vtx_indices, const rayhip_vertex *vertices, const uint32_t n_vertices, float4 *tri_geom, Summary *leaf) {
    uint32_t degenerate = 0;
    for (uint32_t k = 0; k < n_li; ++k) {
        const uint32_t i = li_indices[k];
        if (i >= n_lights || light_type(lights[i]) != LIGHT_TYPE_TRI) {
            continue;
        }
        const uint32_t tri = float_as_uint(lights[i].params[0]), mi = float_as_uint(lights[i].params[1]);
        if (mi >= n_instances || uint64_t(tri) * 3 + 2 >= n_vtx_indices || vtx_indices[tri * 3] >= n_vertices || vtx_indices[tri * 3 + 1] >= n_vertices ||
            vtx_indices[tri * 3 + 2] >= n_vertices) {
            continue;
        }
        degenerate += tri_light_summary(lights[i], instances, vtx_indices, vertices, tri_geom + size_t(i) * 4, leaf[i]) ? 0u : 1u;
    }
    return degenerate;
}

// ... and the tree, level by level (0 / 1 / 2 as plan_levels).  `node_summary`: n_nodes records of scratch.
inline int refit_light_nodes_host(rayhip_light_cwbvh_node *nodes, const uint32_t n_nodes, const rayhip_light *lights, const uint32_t n_lights,
                                  const Summary *leaf, Summary *node_summary, float4 *children, const float *slot_scale, const uint8_t *posed = nullptr) {
    std::vector<uint32_t> level_nodes, level_offset;
    const int rc = plan_levels(nodes, n_nodes, n_lights, level_nodes, level_offset);
    if (rc) {
        return rc;
    }
    for (const uint32_t w : level_nodes) { // (sorted by height: a node comes after everything below it)
        refit_light_node(nodes, w, lights, leaf, node_summary, children, slot_scale, posed);
    }
    return 0;
}

// The scale table, 8 floats per node: for the slot of an inner child the flux the tree `nodes` stores there over the summed flux a
// refit finds below it under `vertices` and `instances` -- the pose the tree was built at; 1 where either is not a positive finite
// number, and for leaves and empty slots.  Runs the host refit once over a copy of the tree.  `out` stays empty on a malformed tree.
inline int slot_scales(const rayhip_light *lights, const uint32_t n_lights, const uint32_t *li_indices, const uint32_t n_li,
                       const rayhip_mesh_instance *instances, const uint32_t n_instances, const uint32_t *vtx_indices, const uint32_t n_vtx_indices,
                       const rayhip_vertex *vertices, const uint32_t n_vertices, const rayhip_light_cwbvh_node *nodes, const uint32_t n_nodes,
                       std::vector<float> &out) {
    out.clear();
    std::vector<rayhip_light_cwbvh_node> copy(nodes, nodes + n_nodes);
    std::vector<Summary> leaf = leaf_table(lights, n_lights, nodes, n_nodes), sums(n_nodes);
    std::vector<float4> geom(size_t(n_lights) * 4), rows(size_t(n_nodes) * LIGHT_CHILDREN_STRIDE);
    refit_tri_lights_host(lights, n_lights, li_indices, n_li, instances, n_instances, vtx_indices, n_vtx_indices, vertices, n_vertices, geom.data(), leaf.data());
    if (const int rc = refit_light_nodes_host(copy.data(), n_nodes, lights, n_lights, leaf.data(), sums.data(), rows.data(), nullptr)) {
        return rc;
    }
    out.assign(size_t(n_nodes) * 8, 1.0f);
    for (uint32_t w = 0; w < n_nodes; ++w) {
        for (int i = 0; i < 8; ++i) {
            const uint32_t link = nodes[w].child[i];
            if (link == EMPTY_SLOT || (link & LEAF_NODE_BIT) != 0) {
                continue;
            }
            const float stored = nodes[w].flux[i], sum = sums[link].flux;
            if (stored > 0.0f && stored <= 3.402823466e+38f && sum > 0.0f && sum <= 3.402823466e+38f) {
                out[size_t(w) * 8 + i] = stored / sum;
            }
        }
    }
    return 0;
}

} // namespace rayhip_light_refit
