// normals.hip.h -- the device side of the normal sets (rayhip_normals_create; recompute_normal_sets in rayhip_deform.hip.h): the element
// functions of normals.h in two kernels, an inverted index instead of a scatter -- no atomics, every sum in the fixed order of its row.
//
//   k_face_frames    one lane per face of the set: three indices, three gathered records (positions and uvs), one 32-byte face record
//                    (unnormalised normal, tangent) written coalesced into a scratch array the set owns.
//   k_vertex_frames  one lane per vertex of the range, 256 per block: the rows of a block are CONTIGUOUS in the row table, so the block
//                    streams them through LDS in chunks of ROW_CHUNK entries (4 bytes each: a face of the set) with coalesced loads and
//                    each lane adds ITS row from there in row order, gathering the face records by entry -- the form morph.hip.h
//                    arrived at by measurement.  A row longer than a chunk spans several.  Then n and / or b of the live record are
//                    rewritten; positions and uvs are only read, by either kernel, so the pass runs in place.
//
// Built: the two-pass form only.  Not built: a fused one-pass form (each corner would recompute its face and gather three records per
// entry where this gathers one), and a walk of the rows in memory without LDS (measured slower for the morph rows, whose shape these
// share).
#pragma once

#include <hip/hip_runtime.h>

#include "normals.h"

namespace rayhip_normals {

constexpr uint32_t ROW_CHUNK = 256; // entries of a block's rows that are in LDS at a time (1 KB)

// `faces`: triangle numbers, their corners inside the vertex array (normals.h: reachable_triangles)
__global__ void __launch_bounds__(256) k_face_frames(const rayhip_vertex *__restrict__ vertices, const uint32_t *__restrict__ vtx_indices,
                                                    const uint32_t *__restrict__ faces, const uint32_t n_faces, FaceFrame *__restrict__ frames) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n_faces) {
        return;
    }
    const size_t t = faces[f];
    const uint32_t i0 = vtx_indices[t * 3], i1 = vtx_indices[t * 3 + 1], i2 = vtx_indices[t * 3 + 2];
    FaceFrame out;
    face_frame(vertices[i0], vertices[i1], vertices[i2], out);
    float4 *dst = reinterpret_cast<float4 *>(frames + f);
    dst[0] = make_float4(out.n[0], out.n[1], out.n[2], out.pad0);
    dst[1] = make_float4(out.t[0], out.t[1], out.t[2], out.pad1);
}

// the sums of the lane's vertex over its row [r0, r1) of `entries` (both 0 for a lane that adds nothing); [block_r0, block_r1): the rows
// of the block.  EVERY lane of the block comes here: the chunks are filled by all of them, between barriers.
template <bool WITH_N, bool WITH_T>
__device__ inline void row_sums(const uint32_t *__restrict__ entries, const uint32_t r0, const uint32_t r1, const uint32_t block_r0, const uint32_t block_r1,
                                const FaceFrame *__restrict__ frames, uint32_t *chunk, Sums &s) {
    const float4 *halves = reinterpret_cast<const float4 *>(frames);
    for (uint32_t c0 = block_r0; c0 < block_r1;) {
        const uint32_t n = min(ROW_CHUNK, block_r1 - c0), c1 = c0 + n;
        __syncthreads(); // (the lanes are done with the chunk before)
        for (uint32_t k = threadIdx.x; k < n; k += blockDim.x) {
            chunk[k] = entries[c0 + k];
        }
        __syncthreads();
        const uint32_t lo = max(r0, c0), hi = min(r1, c1);
        for (uint32_t e = lo; e < hi; ++e) {
            const size_t f = chunk[e - c0];
            FaceFrame ff = {};
            if (WITH_N) {
                const float4 a = halves[f * 2];
                ff.n[0] = a.x, ff.n[1] = a.y, ff.n[2] = a.z;
                add_normal(ff, s);
            }
            if (WITH_T) {
                const float4 b = halves[f * 2 + 1];
                ff.t[0] = b.x, ff.t[1] = b.y, ff.t[2] = b.z;
                add_tangent(ff, s);
            }
        }
        c0 = c1;
    }
}

// `vertices`: the LIVE vertex array from the set's first vertex on.  row / entries: the vertices' own rows; wrow / wentries: the normal
// rows of a welded set, or null.  flags: FLAG_N | FLAG_B.
__global__ void __launch_bounds__(256) k_vertex_frames(rayhip_vertex *vertices, const uint32_t *__restrict__ row, const uint32_t *__restrict__ entries,
                                                      const uint32_t *__restrict__ wrow, const uint32_t *__restrict__ wentries,
                                                      const FaceFrame *__restrict__ frames, const uint32_t count, const uint32_t flags) {
    __shared__ uint32_t chunk[ROW_CHUNK];
    const uint32_t v0 = blockIdx.x * blockDim.x, i = v0 + threadIdx.x, last = min(v0 + blockDim.x, count);
    const bool active = i < count;
    const uint32_t r0 = active ? row[i] : 0u, r1 = active ? row[i + 1] : 0u;
    const bool welded = wrow != nullptr && (flags & FLAG_N) != 0u; // (uniform over the launch, as `flags` is)
    Sums s = {};
    if (!welded && flags == (FLAG_N | FLAG_B)) {
        row_sums<true, true>(entries, r0, r1, row[v0], row[last], frames, chunk, s);
    } else {
        if ((flags & FLAG_N) && !welded) {
            row_sums<true, false>(entries, r0, r1, row[v0], row[last], frames, chunk, s);
        }
        if (flags & FLAG_B) {
            row_sums<false, true>(entries, r0, r1, row[v0], row[last], frames, chunk, s);
        }
        if (welded) {
            row_sums<true, false>(wentries, active ? wrow[i] : 0u, active ? wrow[i + 1] : 0u, wrow[v0], wrow[last], frames, chunk, s);
        }
    }
    if (!active || r0 == r1) {
        return; // (no incident face: the record as it is)
    }
    rayhip_vertex v = {};
    v.n[0] = vertices[i].n[0], v.n[1] = vertices[i].n[1], v.n[2] = vertices[i].n[2];
    vertex_frame(s, flags, v);
    if (flags & FLAG_N) {
        vertices[i].n[0] = v.n[0], vertices[i].n[1] = v.n[1], vertices[i].n[2] = v.n[2];
    }
    if (flags & FLAG_B) {
        vertices[i].b[0] = v.b[0], vertices[i].b[1] = v.b[1], vertices[i].b[2] = v.b[2];
    }
}

} // namespace rayhip_normals
