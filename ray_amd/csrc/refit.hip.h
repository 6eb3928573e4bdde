// refit.hip.h -- the device side of a vertex update (rayhip_scene_update_vertices, rayhip_deform.hip.h): the element functions
// of refit.h, one lane per item.  The tree is refitted with ONE LAUNCH PER HEIGHT LEVEL: a launch reads what the launches
// before it wrote, and the kernel boundary is what makes that visible -- no flags between waves, no fences to get wrong.
#pragma once

#include <hip/hip_runtime.h>

#include "refit.h"

namespace rayhip_refit {

// one lane per tris[] entry: three positions gathered, the 48-byte record written as three 16-byte rows of a table of `pitch`
// rows per record (3, or 4 after RAYHIP_TRI_PITCH=64: the fourth row keeps its zeros).  Entries that repeat a triangle write
// identical bytes.  `n_degenerate`: triangles without area, each counted by its first entry.
__global__ void __launch_bounds__(256) k_refit_tris(const rayhip_vertex *__restrict__ vertices, const uint32_t n_vertices,
                                                   const uint32_t *__restrict__ vtx_indices, const uint32_t n_tris,
                                                   const uint32_t *__restrict__ tri_indices, const uint32_t *__restrict__ first_entry,
                                                   const uint32_t n_entries, float4 *__restrict__ tris, const uint32_t pitch,
                                                   uint32_t *__restrict__ n_degenerate) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_entries) {
        return;
    }
    rayhip_tri_accel rec;
    bool degenerate = false;
    if (!entry_tri_accel(e, tri_indices, vtx_indices, n_tris, vertices, n_vertices, rec, degenerate)) {
        return;
    }
    float4 *row = tris + size_t(e) * pitch;
    row[0] = float4{rec.n_plane[0], rec.n_plane[1], rec.n_plane[2], rec.n_plane[3]};
    row[1] = float4{rec.u_plane[0], rec.u_plane[1], rec.u_plane[2], rec.u_plane[3]};
    row[2] = float4{rec.v_plane[0], rec.v_plane[1], rec.v_plane[2], rec.v_plane[3]};
    if (degenerate && first_entry[tri_indices[e]] == e) {
        atomicAdd(n_degenerate, 1u);
    }
}

// one lane per node of ONE height: level_nodes[0 .. n) name them.  Reads nodes of lower heights (written by earlier launches),
// writes the boxes of its own node.
__global__ void __launch_bounds__(256) k_refit_level(rayhip_bvh2_node *nodes, const uint32_t *__restrict__ level_nodes, const uint32_t n,
                                                    const uint32_t *__restrict__ tri_indices, const uint32_t *__restrict__ vtx_indices,
                                                    const rayhip_vertex *__restrict__ vertices) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        refit_node(nodes, level_nodes[i], tri_indices, vtx_indices, vertices);
    }
}

// the root nodes of the meshes in use, gathered for one copy to the host (their boxes make the instance boxes)
__global__ void __launch_bounds__(256) k_gather_nodes(const rayhip_bvh2_node *__restrict__ nodes, const uint32_t *__restrict__ which, const uint32_t n,
                                                     rayhip_bvh2_node *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        out[i] = nodes[which[i]];
    }
}

} // namespace rayhip_refit
