// normals.h -- shading normals and bitangents derived from the positions that are in the vertex array (rayhip_normals_create): while a
// normal set is live, every call that writes the vertex array recomputes n and / or b of the set's range in place, from the positions
// and uvs then in the array and the scene's own topology.  Element functions shared by the device kernels (normals.hip.h) and a
// plain-loop host driver (tests/hostsim/hostsim_normals.cpp), like skin.h / morph.h: IEEE operations in a STATED ORDER without
// contraction on both sides, so both produce the same bits.
//
// FACES of a set: the triangles some bottom-level tree reaches (reachable_triangles: the leaf ranges, never the raw index pools, whose
// padding is uninitialised) that have a corner in the range, in ascending triangle number.  A triangle that had no area at upload is in
// no tree and never contributes, whatever its corners become.  Corners outside the range are read like any other.
// Per face (face_frame), p0 p1 p2 / t0 t1 t2 its corners' positions / uvs:
//   dp1 = p1 - p0, dp2 = p2 - p0;  normal = cross(dp1, dp2), NOT normalised: the vertex sums are area-weighted (only + - * / sqrt, which
//              host and device round alike)
//   tangent    the reference's ComputeTangentBasis (internal/TextureUtils.cpp), operation for operation: dt1 = t1 - t0, dt2 = t2 - t0,
//              det = |dt1.x * dt2.y - dt1.y * dt2.x|; det > 1e-7: (dp1 * dt2.y - dp2 * dt1.y) * (1 / det); else the axis fallback: the
//              smallest component of the plane normal picks an axis, two normalised cross products, or zero.
// Per vertex, over the (face, corner) pairs incident to it in ascending face, then ascending corner (a row of build_rows):
//   normal     the sum of the face normals over the pairs of EVERY member of the vertex's weld group (without weld: its own), then
//              rayhip_skin::normalised_or_rest against the normal the record arrived with: a sum without length (or whose squared
//              length is not finite) keeps the arriving normal
//   bitangent  T = the sum of the face tangents over the vertex's OWN pairs (uv seams differ across a weld); where some |T_k| > 1e-7 and
//              l = length(cross(n, T)) > 1e-7 (n: the vertex's final normal): cross(n, T) / l; otherwise T -- what the reference leaves,
//              and what a scene build of the same topology would store.  length(v) = sqrt((x*x + y*y) + z*z).
//   A vertex of the range without an incident face keeps its record bytewise.  Positions and uvs are only read.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "rt_types.h"
#include "skin.h"

namespace rayhip_normals {

constexpr uint32_t MAX_SETS = 16;       // live normal sets per context
constexpr float EPS = 0.0000001f;       // the reference's FLT_EPS (internal/Constants.inl)
constexpr uint32_t FLAG_N = 1u, FLAG_B = 2u;
constexpr uint32_t COUNT_BITS = 7u << 29, INDEX_BITS = ~COUNT_BITS; // a leaf word of a BVH2 node: (count - 1) << 29 | first entry

// what k_face_frames leaves per face for k_vertex_frames to gather.  32 bytes, not 24: a gathered record is then two aligned 16-byte
// loads that never straddle a 32-byte sector or a cache line (a 24-byte record does at every other index), for a third more bytes in the
// one pass that writes them coalesced.
struct FaceFrame {
    float n[3], pad0, t[3], pad1;
};
static_assert(sizeof(FaceFrame) == 32, "face records are gathered as two 16-byte halves");

RT_HD void cross3(const float a[3], const float b[3], float out[3]) {
    out[0] = a[1] * b[2] - a[2] * b[1];
    out[1] = a[2] * b[0] - a[0] * b[2];
    out[2] = a[0] * b[1] - a[1] * b[0];
}

RT_HD float length3(const float v[3]) { return sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }

// the record of the face with corners v0, v1, v2
RT_HD void face_frame(const rayhip_vertex &v0, const rayhip_vertex &v1, const rayhip_vertex &v2, FaceFrame &out) {
    const float dp1[3] = {v1.p[0] - v0.p[0], v1.p[1] - v0.p[1], v1.p[2] - v0.p[2]};
    const float dp2[3] = {v2.p[0] - v0.p[0], v2.p[1] - v0.p[1], v2.p[2] - v0.p[2]};
    const float dt1[2] = {v1.t[0] - v0.t[0], v1.t[1] - v0.t[1]}, dt2[2] = {v2.t[0] - v0.t[0], v2.t[1] - v0.t[1]};
    float plane[3];
    cross3(dp1, dp2, plane);
    out.n[0] = plane[0], out.n[1] = plane[1], out.n[2] = plane[2];
    out.pad0 = 0.0f, out.pad1 = 0.0f;
    const float det = fabsf(dt1[0] * dt2[1] - dt1[1] * dt2[0]);
    if (det > EPS) {
        const float inv_det = 1.0f / det;
        for (int i = 0; i < 3; ++i) {
            out.t[i] = (dp1[i] * dt2[1] - dp2[i] * dt1[1]) * inv_det;
        }
        return;
    }
    // no uv area: an axis by the smallest component of the plane normal
    int w = 2;
    float axis[3] = {0.0f, 1.0f, 0.0f};
    if (fabsf(plane[0]) <= fabsf(plane[1]) && fabsf(plane[0]) <= fabsf(plane[2])) {
        axis[0] = 1.0f, axis[1] = 0.0f, w = 1;
    } else if (fabsf(plane[2]) <= fabsf(plane[0]) && fabsf(plane[2]) <= fabsf(plane[1])) {
        axis[1] = 0.0f, axis[2] = 1.0f, w = 0;
    }
    out.t[0] = 0.0f, out.t[1] = 0.0f, out.t[2] = 0.0f;
    if (fabsf(plane[w]) > EPS) {
        float binormal[3], tangent[3];
        cross3(plane, axis, binormal);
        const float lb = length3(binormal);
        binormal[0] = binormal[0] / lb, binormal[1] = binormal[1] / lb, binormal[2] = binormal[2] / lb;
        cross3(plane, binormal, tangent);
        const float lt = length3(tangent);
        out.t[0] = tangent[0] / lt, out.t[1] = tangent[1] / lt, out.t[2] = tangent[2] / lt;
    }
}

// the running sums of one vertex: zero, then the face records of its row(s) in order
struct Sums {
    float n[3], t[3];
};

RT_HD void add_normal(const FaceFrame &f, Sums &s) { s.n[0] = s.n[0] + f.n[0], s.n[1] = s.n[1] + f.n[1], s.n[2] = s.n[2] + f.n[2]; }
RT_HD void add_tangent(const FaceFrame &f, Sums &s) { s.t[0] = s.t[0] + f.t[0], s.t[1] = s.t[1] + f.t[1], s.t[2] = s.t[2] + f.t[2]; }

// the vertex's normal from the sum over its weld group; `arrived`: the normal of the record as it was written
RT_HD void vertex_normal(const float sum[3], const float arrived[3], float out[3]) { rayhip_skin::normalised_or_rest(sum, arrived, out); }

// the vertex's bitangent from the tangent sum T over its own corners and its final normal
RT_HD void vertex_bitangent(const float T[3], const float n[3], float out[3]) {
    out[0] = T[0], out[1] = T[1], out[2] = T[2];
    if (fabsf(T[0]) > EPS || fabsf(T[1]) > EPS || fabsf(T[2]) > EPS) {
        float c[3];
        cross3(n, T, c);
        const float l = length3(c);
        if (l > EPS) {
            out[0] = c[0] / l, out[1] = c[1] / l, out[2] = c[2] / l;
        }
    }
}

// the record of a vertex that has an incident face, in place: n and / or b by `flags`, p and t untouched
RT_HD void vertex_frame(const Sums &s, const uint32_t flags, rayhip_vertex &v) {
    if (flags & FLAG_N) {
        const float arrived[3] = {v.n[0], v.n[1], v.n[2]};
        vertex_normal(s.n, arrived, v.n);
    }
    if (flags & FLAG_B) {
        vertex_bitangent(s.t, v.n, v.b);
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
// what rayhip_normals_create checks of a description (its pointers and the range against the array are the caller's to check):
// 0 = fine, 1 = flags outside 1..3, 2 = a weld index >= count, 3 = a weld index that is not canonical (weld[weld[i]] != weld[i]).
// `where`: the vertex, relative to the range.
inline int validate_desc(const uint32_t count, const uint32_t flags, const uint32_t *weld, uint32_t &where) {
    where = 0;
    if (flags == 0 || flags > (FLAG_N | FLAG_B)) {
        return 1;
    }
    for (uint32_t i = 0; weld && i < count; ++i) {
        where = i;
        if (weld[i] >= count) {
            return 2;
        }
    }
    for (uint32_t i = 0; weld && i < count; ++i) {
        where = i;
        if (weld[weld[i]] != weld[i]) {
            return 3;
        }
    }
    return 0;
}

// the triangles the trees below `roots` reach, ascending and without repeats (leaves repeat triangles): leaf word -> entries of
// tri_indices -> triangle.  Entries that name no triangle of the arrays, or a triangle with a corner outside the vertex array, are left
// out.  false: a link leaves the node array or the trees are no trees.
inline bool reachable_triangles(const rayhip_bvh2_node *nodes, const uint32_t n_nodes, const uint32_t *roots, const size_t n_roots, const uint32_t *tri_indices,
                                const uint32_t n_entries, const uint32_t *vtx_indices, const uint32_t n_tris, const uint32_t n_vertices,
                                std::vector<uint32_t> &tris) {
    tris.clear();
    std::vector<uint32_t> stack;
    size_t visited = 0;
    for (size_t r = 0; r < n_roots; ++r) {
        stack.assign(1, roots[r]);
        while (!stack.empty()) {
            const uint32_t w = stack.back();
            stack.pop_back();
            if (w & COUNT_BITS) {
                const uint32_t first = w & INDEX_BITS, n = ((w & COUNT_BITS) >> 29) + 1;
                for (uint32_t e = first; e < first + n && e < n_entries; ++e) {
                    const uint32_t t = tri_indices[e];
                    if (t < n_tris && vtx_indices[size_t(t) * 3] < n_vertices && vtx_indices[size_t(t) * 3 + 1] < n_vertices &&
                        vtx_indices[size_t(t) * 3 + 2] < n_vertices) {
                        tris.push_back(t);
                    }
                }
                continue;
            }
            if (w >= n_nodes || ++visited > n_nodes) {
                return false;
            }
            stack.push_back(nodes[w].left_child);
            stack.push_back(nodes[w].right_child);
        }
    }
    std::sort(tris.begin(), tris.end());
    tris.erase(std::unique(tris.begin(), tris.end()), tris.end());
    return true;
}

// the tables of a set over vertices [first, first + count), by counting sort
struct Tables {
    std::vector<uint32_t> faces;   // the set's faces: triangle numbers, ascending
    std::vector<uint32_t> row;     // [count + 1]: vertex i's own (face, corner) pairs are entries[row[i] .. row[i + 1]), by face, then corner
    std::vector<uint32_t> entries; // indices into `faces`
    // with weld and FLAG_N: vertex i's NORMAL row, wentries[wrow[i] .. wrow[i + 1]): the pairs of every member of its weld group, by
    // face, then corner -- every member holds the group's whole row, so that the rows of consecutive vertices stay contiguous (which is
    // what the kernel streams) at the price of one copy per member.  A vertex without a face of its own has an empty one.
    std::vector<uint32_t> wrow, wentries;
};

// `reachable`: reachable_triangles().  `weld`: validated, or null.  0 = built, 4 = more than 2^32 - 1 entries in a row table.
inline int build_rows(const uint32_t *reachable, const size_t n_reachable, const uint32_t *vtx_indices, const uint32_t first, const uint32_t count,
                      const uint32_t *weld, Tables &out) {
    out = Tables{};
    const auto inside = [&](const uint32_t v) { return v >= first && v - first < count; };
    for (size_t k = 0; k < n_reachable; ++k) {
        const uint32_t *c = vtx_indices + size_t(reachable[k]) * 3;
        if (inside(c[0]) || inside(c[1]) || inside(c[2])) {
            out.faces.push_back(reachable[k]);
        }
    }
    // (a face has three corners: at most 3 * 2^32 pairs, counted in 64 bits)
    std::vector<uint64_t> n_own(size_t(count) + 1, 0), n_group(weld ? size_t(count) : 0, 0);
    for (const uint32_t t : out.faces) {
        for (int k = 0; k < 3; ++k) {
            const uint32_t v = vtx_indices[size_t(t) * 3 + k];
            if (inside(v)) {
                ++n_own[size_t(v - first) + 1];
                if (weld) {
                    ++n_group[weld[v - first]];
                }
            }
        }
    }
    uint64_t total = 0, wtotal = 0;
    for (uint32_t i = 0; i < count; ++i) {
        total += n_own[size_t(i) + 1];
        wtotal += weld && n_own[size_t(i) + 1] != 0 ? n_group[weld[i]] : 0;
    }
    if (total > 0xffffffffull || wtotal > 0xffffffffull) {
        return 4;
    }
    out.row.assign(size_t(count) + 1, 0u);
    for (uint32_t i = 0; i < count; ++i) {
        out.row[i + 1] = out.row[i] + uint32_t(n_own[size_t(i) + 1]);
    }
    out.entries.assign(out.row[count], 0u);
    std::vector<uint32_t> cursor(out.row.begin(), out.row.end() - 1);
    for (size_t f = 0; f < out.faces.size(); ++f) { // faces ascending, corners ascending: every row comes out in that order
        for (int k = 0; k < 3; ++k) {
            const uint32_t v = vtx_indices[size_t(out.faces[f]) * 3 + k];
            if (inside(v)) {
                out.entries[cursor[v - first]++] = uint32_t(f);
            }
        }
    }
    if (!weld) {
        return 0;
    }
    // the groups' rows by the same sort (keyed by the canonical vertex), then one copy per member that has a face
    std::vector<uint32_t> grow(size_t(count) + 1, 0u);
    for (uint32_t g = 0; g < count; ++g) {
        grow[g + 1] = grow[g] + uint32_t(n_group[g]); // (the sum over the groups is `total`)
    }
    std::vector<uint32_t> gentries(grow[count], 0u), gcursor(grow.begin(), grow.end() - 1);
    for (size_t f = 0; f < out.faces.size(); ++f) {
        for (int k = 0; k < 3; ++k) {
            const uint32_t v = vtx_indices[size_t(out.faces[f]) * 3 + k];
            if (inside(v)) {
                gentries[gcursor[weld[v - first]]++] = uint32_t(f);
            }
        }
    }
    out.wrow.assign(size_t(count) + 1, 0u);
    for (uint32_t i = 0; i < count; ++i) {
        out.wrow[i + 1] = out.wrow[i] + (out.row[i + 1] != out.row[i] ? grow[weld[i] + 1] - grow[weld[i]] : 0u);
    }
    out.wentries.resize(out.wrow[count]);
    for (uint32_t i = 0; i < count; ++i) {
        std::copy(gentries.begin() + grow[weld[i]], gentries.begin() + grow[weld[i]] + (out.wrow[i + 1] - out.wrow[i]), out.wentries.begin() + out.wrow[i]);
    }
    return 0;
}

// plain-loop driver: the set's range of `vertices` (the whole array) recomputed in place, as the two kernels do it -- every face record
// first (they read positions and uvs only, which the second pass does not write), then vertex after vertex
inline void recompute_host(rayhip_vertex *vertices, const uint32_t *vtx_indices, const Tables &tb, const uint32_t first, const uint32_t count,
                           const uint32_t flags) {
    std::vector<FaceFrame> frames(tb.faces.size());
    for (size_t f = 0; f < tb.faces.size(); ++f) {
        const uint32_t *c = vtx_indices + size_t(tb.faces[f]) * 3;
        face_frame(vertices[c[0]], vertices[c[1]], vertices[c[2]], frames[f]);
    }
    const bool welded = (flags & FLAG_N) && !tb.wrow.empty();
    for (uint32_t i = 0; i < count; ++i) {
        if (tb.row[i] == tb.row[i + 1]) {
            continue; // (no incident face: the record as it is)
        }
        Sums s = {};
        for (uint32_t e = tb.row[i]; e < tb.row[i + 1]; ++e) {
            if ((flags & FLAG_N) && !welded) {
                add_normal(frames[tb.entries[e]], s);
            }
            if (flags & FLAG_B) {
                add_tangent(frames[tb.entries[e]], s);
            }
        }
        for (uint32_t e = welded ? tb.wrow[i] : 0u; welded && e < tb.wrow[i + 1]; ++e) {
            add_normal(frames[tb.wentries[e]], s);
        }
        vertex_frame(s, flags, vertices[first + i]);
    }
}

} // namespace rayhip_normals
