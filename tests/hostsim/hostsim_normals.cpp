// hostsim_normals.cpp -- TEST INFRASTRUCTURE.  Normal sets as the device recomputes them (ray_amd/csrc/normals.h: the faces of a vertex
// range, its row tables, the face record and the vertex's normal and bitangent), compiled with g++ (the HOSTSIM_FLAGS of hostsim.cpp: no
// fma contraction, SSE2, glibc libm) over plain arrays, with the prefix hostsim_ and without a context.  tests/test_normals_hostsim.py
// holds these against a numpy restatement, a float64 model and the reference's own bitangents; tests/test_gpu_normals.py holds the device
// (normals.hip.h) against this file.
//
// Never linked into librayhip.so.
#include <string.h>

#include "../../include/rayhip.h"
#include "../../ray_amd/csrc/normals.h"

#define HS_API extern "C" __attribute__((visibility("default")))

// what rayhip_normals_create says of a description: 0 = fine, 1 = count == 0, a range outside the array of n_vertices, flags outside
// 1..3, a weld index >= count or not canonical (*why: 0 for the range, else what normals.h: validate_desc tells apart)
HS_API int hostsim_normals_validate(uint32_t n_vertices, uint32_t first, uint32_t count, uint32_t flags, const uint32_t *weld, int *why) {
    *why = 0;
    if (count == 0 || uint64_t(first) + count > n_vertices) {
        return 1;
    }
    uint32_t where = 0;
    *why = rayhip_normals::validate_desc(count, flags, weld, where);
    return *why ? 1 : 0;
}

// the triangles the trees below `roots` reach, ascending: written into tris[room]; returns their number (nothing written where it
// exceeds the room), 0xffffffff for malformed trees
HS_API uint32_t hostsim_normals_reachable(const rayhip_bvh2_node *nodes, uint32_t n_nodes, const uint32_t *roots, uint32_t n_roots, const uint32_t *tri_indices,
                                          uint32_t n_entries, const uint32_t *vtx_indices, uint32_t n_tris, uint32_t n_vertices, uint32_t *tris, uint32_t room) {
    std::vector<uint32_t> t;
    if (!rayhip_normals::reachable_triangles(nodes, n_nodes, roots, n_roots, tri_indices, n_entries, vtx_indices, n_tris, n_vertices, t)) {
        return 0xffffffffu;
    }
    if (t.size() <= room && !t.empty()) {
        memcpy(tris, t.data(), t.size() * sizeof(uint32_t));
    }
    return uint32_t(t.size());
}

namespace {
rayhip_normals::Tables g_tables; // the tables of the last hostsim_normals_rows (single-threaded tests)
}

// the tables of a (valid) set over [first, first + count): sizes[4] = faces, entries, wrow words (0 or count + 1), wentries.  Returns
// what build_rows returns; the arrays are fetched with hostsim_normals_table.
HS_API int hostsim_normals_rows(const uint32_t *reachable, uint32_t n_reachable, const uint32_t *vtx_indices, uint32_t first, uint32_t count, const uint32_t *weld,
                                uint32_t *sizes) {
    const int rc = rayhip_normals::build_rows(reachable, n_reachable, vtx_indices, first, count, weld, g_tables);
    sizes[0] = uint32_t(g_tables.faces.size()), sizes[1] = uint32_t(g_tables.entries.size());
    sizes[2] = uint32_t(g_tables.wrow.size()), sizes[3] = uint32_t(g_tables.wentries.size());
    return rc;
}

// which: 0 faces, 1 row [count + 1], 2 entries, 3 wrow, 4 wentries -- copied into dst (sized by the caller from hostsim_normals_rows)
HS_API void hostsim_normals_table(int which, uint32_t *dst) {
    const std::vector<uint32_t> *v[5] = {&g_tables.faces, &g_tables.row, &g_tables.entries, &g_tables.wrow, &g_tables.wentries};
    if (!v[which]->empty()) {
        memcpy(dst, v[which]->data(), v[which]->size() * sizeof(uint32_t));
    }
}

// vertices[n_vertices] with n and / or b of [first, first + count) recomputed in place; 0, or what build_rows refused
HS_API int hostsim_normals_recompute(rayhip_vertex *vertices, const uint32_t *reachable, uint32_t n_reachable, const uint32_t *vtx_indices, uint32_t first,
                                     uint32_t count, uint32_t flags, const uint32_t *weld) {
    rayhip_normals::Tables tb;
    if (const int rc = rayhip_normals::build_rows(reachable, n_reachable, vtx_indices, first, count, (flags & rayhip_normals::FLAG_N) ? weld : nullptr, tb)) {
        return rc;
    }
    rayhip_normals::recompute_host(vertices, vtx_indices, tb, first, count, flags);
    return 0;
}

// one face record (8 floats: normal xyz, 0, tangent xyz, 0) from three vertex records
HS_API void hostsim_normals_face(const rayhip_vertex *v, float *out) {
    rayhip_normals::FaceFrame f;
    rayhip_normals::face_frame(v[0], v[1], v[2], f);
    memcpy(out, &f, sizeof(f));
}
