// skin.h -- linear-blend skinning of the vertices a skin drives (rayhip_skin_create / rayhip_scene_pose_skins): the rest pose and the
// weights stay on the device, a pose is a palette of bone matrices.  Element functions shared by the device kernels (skin.hip.h)
// and a plain-loop host driver (tests/hostsim/hostsim_skin.cpp), like refit.h: IEEE operations in a STATED ORDER without
// contraction on both sides, so both produce the same bits.
//
// Palette: `bones_count` row-major 3x4 float matrices (12 floats per bone: m[i][0..2] the linear part, m[i][3] the translation).
// They act in the mesh's OBJECT space; the instance transforms stay on top, as for every other vertex.
// A vertex has four influences (bone index, weight).  An influence of weight 0 is skipped; the others are taken in the order 0..3:
//   position   t_i = ((m[i][0]*p0 + m[i][1]*p1) + m[i][2]*p2) + m[i][3];   first used influence: acc_i = w*t_i, later: acc_i = acc_i + w*t_i
//   normal, bitangent   the same blend with the 3x3 LINEAR PART ONLY (t_i = (m[i][0]*n0 + m[i][1]*n1) + m[i][2]*n2): no translation
//              and NO inverse-transpose -- exact for rigid bones and for uniform scale, an approximation under shear or non-uniform
//              scale.  Then normalised: dot = (x*x + y*y) + z*z, len = sqrtf(dot), x / len; where dot is 0 or not finite the rest
//              vector is copied.
//   uv         copied.
// A vertex whose four weights are all 0 keeps its rest record bytewise.
#pragma once

#include <stdint.h>

#include "rt_types.h"

namespace rayhip_skin {

constexpr uint32_t SKIN_LDS_BONES = 256; // palettes up to this many bones are copied to LDS by the block (12 KB: the occupancy the registers allow stays)
constexpr uint32_t MAX_SKINS = 16;       // live skins per context

RT_HD bool finite_f(const float x) { return fabsf(x) <= 3.402823466e+38f; } // (false for NaN)

// the blend of `v` under the four influences; `translate`: a point (the fourth column counts).  false: no influence has a weight
RT_HD bool blend(const float v[3], const uint16_t idx[4], const float w[4], const float *bones, const bool translate, float acc[3]) {
    bool any = false;
    for (int k = 0; k < 4; ++k) {
        if (w[k] == 0.0f) {
            continue;
        }
        const float *m = bones + size_t(idx[k]) * 12;
        for (int i = 0; i < 3; ++i) {
            float t = (m[i * 4 + 0] * v[0] + m[i * 4 + 1] * v[1]) + m[i * 4 + 2] * v[2];
            if (translate) {
                t = t + m[i * 4 + 3];
            }
            const float wt = w[k] * t;
            acc[i] = any ? acc[i] + wt : wt;
        }
        any = true;
    }
    return any;
}

// `v` normalised into `out`, or `rest` where it has no length / is not finite
RT_HD void normalised_or_rest(const float v[3], const float rest[3], float out[3]) {
    const float dot = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    if (dot == 0.0f || !finite_f(dot)) {
        out[0] = rest[0], out[1] = rest[1], out[2] = rest[2];
        return;
    }
    const float len = sqrtf(dot);
    out[0] = v[0] / len, out[1] = v[1] / len, out[2] = v[2] / len;
}

// the posed record of one vertex.  `idx` are below the palette's bone count (checked when the skin is created).
RT_HD void skin_vertex(const rayhip_vertex &rest, const uint16_t idx[4], const float w[4], const float *bones, rayhip_vertex &out) {
    out = rest;
    float p[3] = {0.0f, 0.0f, 0.0f}, n[3] = {0.0f, 0.0f, 0.0f}, b[3] = {0.0f, 0.0f, 0.0f};
    if (!blend(rest.p, idx, w, bones, true, p)) {
        return; // (all four weights zero: the rest record)
    }
    blend(rest.n, idx, w, bones, false, n);
    blend(rest.b, idx, w, bones, false, b);
    out.p[0] = p[0], out.p[1] = p[1], out.p[2] = p[2];
    normalised_or_rest(n, rest.n, out.n);
    normalised_or_rest(b, rest.b, out.b);
}

// a vertex some triangle uses whose position is not finite: what an update refuses before it writes the vertex array
RT_HD bool vertex_check(const rayhip_vertex &v, const bool used) { return used && !(finite_f(v.p[0]) && finite_f(v.p[1]) && finite_f(v.p[2])); }

// bytewise comparison of two records (what memcmp says, as eleven words)
RT_HD bool same_bytes(const rayhip_vertex &x, const rayhip_vertex &y) {
    const uint32_t *a = reinterpret_cast<const uint32_t *>(&x), *b = reinterpret_cast<const uint32_t *>(&y);
    bool same = true;
    for (int k = 0; k < 11; ++k) {
        same = same && a[k] == b[k];
    }
    return same;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
// plain-loop drivers over the element functions.  `used`: per vertex of the range, or null (every vertex counts).
// Returns the number of used vertices whose posed position is not finite.
inline uint32_t skin_vertices_host(const rayhip_vertex *rest, const uint16_t *indices, const float *weights, const uint32_t count, const float *bones,
                                   const uint8_t *used, rayhip_vertex *out) {
    uint32_t bad = 0;
    for (uint32_t i = 0; i < count; ++i) {
        skin_vertex(rest[i], indices + size_t(i) * 4, weights + size_t(i) * 4, bones, out[i]);
        bad += vertex_check(out[i], used == nullptr || used[i] != 0) ? 1u : 0u;
    }
    return bad;
}

// what rayhip_skin_create checks of the influences: 0 = fine, 1 = an index >= bones_count, 2 = a weight that is negative or not finite
inline int validate_influences(const uint16_t *indices, const float *weights, const uint32_t count, const uint32_t bones_count, uint32_t &where) {
    for (uint32_t i = 0; i < count; ++i) {
        for (int k = 0; k < 4; ++k) {
            where = i;
            if (indices[size_t(i) * 4 + k] >= bones_count) {
                return 1;
            }
            const float w = weights[size_t(i) * 4 + k];
            if (!finite_f(w) || w < 0.0f) {
                return 2;
            }
        }
    }
    return 0;
}

} // namespace rayhip_skin
