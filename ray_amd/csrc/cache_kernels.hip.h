// cache_kernels.hip.h -- the spatial radiance cache's kernels (rt_cache.h; the entry points rayhip_cache_* / rayhip_k_cache_* are in
// rayhip_cache.hip.h).
//
//   k_cache_update         one lane per vertex of a cache-update bounce: insert the vertex's key (64-bit CAS), add its radiance to
//                          this frame's voxels along the path (32-bit atomic adds).  The path state is SoA planes per path.
//   k_cache_resolve_slots  phase 1 of the resolve: one lane per slot, the slot's resolved voxel written over this frame's voxel.
//                          Reads of other buckets (the adjacent-level lookup) see the key table as update left it.
//   k_cache_compact        phase 2: one lane per slot, two 32-slot buckets per wave; a ballot of the "keep" mask and mbcnt of the
//                          lanes below give every kept slot its place at the front of its bucket.
// Two launches instead of the reference's in-place serial loop (RadCacheRef.cpp:311-393): no slot is compacted while another
// lane may still look it up, so the result does not depend on scheduling.
#pragma once

#include "../../include/rayhip.h"
#include "rt_cache.h"

namespace rt {
namespace cache {

static_assert(sizeof(GridParams) == sizeof(rayhip_cache_grid), "GridParams == rayhip_cache_grid");
static_assert(sizeof(Voxel) == 16, "packed_cache_voxel_t");
static_assert(sizeof(rayhip_cache_vertex) == 80, "rayhip_cache_vertex");

// cache_data_t of every path of a pass, SoA: entries [4][n], weights [4][3][n], length [n] (68 B per path)
struct PathPlanes {
    uint32_t *entries;
    float *weight;
    int32_t *len;
    uint32_t n;
};

RT_HD f3 vertex_position(const rayhip_cache_vertex &v) {
    // ro + inter.t * I (RadCacheRef.cpp:265): t * d per lane, then the sum
    return mk3(v.o) + v.t * mk3(v.d);
}

#if defined(__HIPCC__)
__global__ __launch_bounds__(256) void k_cache_update(const rayhip_cache_vertex *__restrict__ verts, uint32_t count, PathPlanes pp, GridParams g,
                                                      uint64_t *entries, Voxel *voxels_curr) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
        const rayhip_cache_vertex v = verts[i];
        const uint32_t p = v.path;
        if (p >= pp.n) {
            continue; // (rejected on the host already)
        }
        PathData pd;
        for (int j = 0; j < PROPAGATION_DEPTH; ++j) {
            pd.entries[j] = pp.entries[size_t(j) * pp.n + p];
            pd.weight[j] = mk3(pp.weight[size_t(3 * j + 0) * pp.n + p], pp.weight[size_t(3 * j + 1) * pp.n + p], pp.weight[size_t(3 * j + 2) * pp.n + p]);
        }
        pd.len = pp.len[p];
        update_path(pd, vertex_position(v), mk3(v.n), mk3(v.radiance), mk3(v.c), v.ends != 0, g, entries, ENTRIES_COUNT, voxels_curr);
        for (int j = 0; j < PROPAGATION_DEPTH; ++j) {
            pp.entries[size_t(j) * pp.n + p] = pd.entries[j];
            pp.weight[size_t(3 * j + 0) * pp.n + p] = pd.weight[j].x;
            pp.weight[size_t(3 * j + 1) * pp.n + p] = pd.weight[j].y;
            pp.weight[size_t(3 * j + 2) * pp.n + p] = pd.weight[j].z;
        }
        pp.len[p] = pd.len;
    }
}

__global__ __launch_bounds__(256) void k_cache_resolve_slots(GridParams g, int cam_moved, const uint64_t *__restrict__ entries, Voxel *voxels_curr,
                                                             const Voxel *__restrict__ voxels_prev) {
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < ENTRIES_COUNT; s += gridDim.x * blockDim.x) {
        const uint64_t key = entries[s];
        if (key != INVALID_KEY) {
            voxels_curr[s] = resolve_voxel(key, voxels_prev[s], voxels_curr[s], cam_moved != 0, g, entries, ENTRIES_COUNT, voxels_prev);
        }
    }
}

// (wave64: the two halves of a wave are two buckets; the grid-stride loop keeps whole waves together because ENTRIES_COUNT is a
// multiple of the block)
__global__ __launch_bounds__(256) void k_cache_compact(uint64_t *entries, Voxel *voxels) {
    static_assert(BUCKET_SIZE == 32, "two buckets per wave64");
    const uint32_t lane = __lane_id();
    const uint32_t half = lane >> 5, lane_in_bucket = lane & 31u;
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < ENTRIES_COUNT; s += gridDim.x * blockDim.x) {
        const uint64_t key = entries[s];
        // (an empty slot's voxel is zero: update only adds into slots that hold a key, the previous compaction cleared the rest)
        const Voxel v = key != INVALID_KEY ? voxels[s] : Voxel{{0, 0, 0, 0}};
        const bool keep = key != INVALID_KEY && v.v[3] != 0;
        const unsigned long long mask = __ballot(keep);
        const uint32_t lo = uint32_t(mask), hi = uint32_t(mask >> 32);
        // kept lanes below this one, in the whole wave, minus the other bucket's when this lane is in the upper half
        const uint32_t below = __builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, 0u)) - (half ? uint32_t(__popc(lo)) : 0u);
        const uint32_t kept = uint32_t(__popc(half ? hi : lo));
        const uint32_t base = s - lane_in_bucket;
        // the kept ones go to [base, base + kept) (never above their own slot, and the loads above are complete before any lane
        // stores), the slots from `kept` on are cleared; a slot whose content is already right (a key in place, an empty slot) is
        // not written: on a sparse table almost nothing is
        if (keep && below != lane_in_bucket) {
            entries[base + below] = key;
            voxels[base + below] = v;
        }
        if (lane_in_bucket >= kept && key != INVALID_KEY) {
            entries[s] = INVALID_KEY;
            voxels[s] = Voxel{{0, 0, 0, 0}};
        }
    }
}

__global__ __launch_bounds__(256) void k_cache_query(const float *__restrict__ points, uint32_t count, GridParams g, const uint64_t *__restrict__ entries,
                                                     const Voxel *__restrict__ voxels, float4 *out) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
        const float *pt = points + size_t(i) * 6;
        f3 rad = splat3(0.0f);
        const uint32_t n = query(entries, voxels, ENTRIES_COUNT, mk3(pt), mk3(pt + 3), g, rad);
        out[i] = n ? make_float4(rad.x, rad.y, rad.z, float(n)) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}
#endif

} // namespace cache
} // namespace rt
