// morph.hip.h -- the device side of morph targets (rayhip_scene_pose; rayhip_deform.hip.h): the element functions of morph.h, one lane
// per vertex.  Both kernels keep the contract of k_skin_vertices (skin.hip.h): they only READ what a render pass reads, the posed
// vertices go to a staging array and the findings to the same counter, so a refused pose has touched nothing.
//
// How a row is read was decided by measurement (profiles/morph/README.md).  Rows are ragged, and a lane that walks its own row in
// memory reads 40-byte records at a stride its neighbours do not share.  But the rows of a block are CONTIGUOUS in the table --
// [row[v0], row[v0 + 256]) -- so the block streams them into LDS with coalesced loads, ROW_CHUNK entries at a time, and each lane adds
// the entries of ITS row from there in row order: the order of the adds, hence the bits, is that of the walk.  The walk in memory was
// built too, measured slower on the face-like set and deleted.
#pragma once

#include <hip/hip_runtime.h>

#include "morph.h"
#include "skin.hip.h"

namespace rayhip_morph {

constexpr uint32_t ROW_CHUNK = 256;                        // entries of a block's rows that are in LDS at a time (10 KB)
constexpr uint32_t ROW_CHUNK_WORDS = ROW_CHUNK * sizeof(Entry) / 4;

// the weights of a pose go to LDS for up to MORPH_LDS_TARGETS targets and are read from memory otherwise (uniform over the launch):
// the same values either way, hence the same bits.  (The callers branch on it so that each side keeps its address space.)
__device__ inline bool stage_weights(float *lds, const float *__restrict__ weights, const uint32_t targets_count) {
    if (targets_count > MORPH_LDS_TARGETS) {
        return false;
    }
    for (uint32_t k = threadIdx.x; k < targets_count; k += blockDim.x) {
        lds[k] = weights[k];
    }
    return true;
}

// the sums of the lane's vertex over its row [r0, r1) (both 0 for a lane without a vertex); [block_r0, block_r1): the rows of the block.
// EVERY lane of the block comes here: the chunks are filled by all of them, between barriers.
__device__ inline void row_sums(const Entry *__restrict__ entries, const uint32_t r0, const uint32_t r1, const uint32_t block_r0, const uint32_t block_r1,
                                const float *w, uint32_t *chunk, Sums &s) {
    for (uint32_t c0 = block_r0; c0 < block_r1; c0 += ROW_CHUNK) {
        const uint32_t c1 = min(c0 + ROW_CHUNK, block_r1);
        const uint32_t *src = reinterpret_cast<const uint32_t *>(entries + c0);
        __syncthreads(); // (the lanes are done with the chunk before)
        for (uint32_t k = threadIdx.x; k < (c1 - c0) * (sizeof(Entry) / 4); k += blockDim.x) {
            chunk[k] = src[k];
        }
        __syncthreads();
        const uint32_t lo = max(r0, c0), hi = min(r1, c1);
        if (lo < hi) {
            morph_add(reinterpret_cast<const Entry *>(chunk) + (lo - c0), hi - lo, w, s);
        }
    }
}

// one lane per vertex of ONE morph set that lies in no skin: base record (44 bytes), two row offsets and the row's entries (40 bytes
// each) in, the posed record out into `staged` (never the live vertex array).  `used`: per vertex of the set's range, some triangle
// uses it.  `n_bad` counts used vertices whose posed position is not finite.
__global__ void __launch_bounds__(256) k_morph_vertices(const rayhip_vertex *__restrict__ base, const uint32_t *__restrict__ row, const Entry *__restrict__ entries,
                                                       const uint32_t count, const float *__restrict__ weights, const uint32_t targets_count,
                                                       const uint8_t *__restrict__ used, rayhip_vertex *__restrict__ staged, uint32_t *__restrict__ n_bad) {
    __shared__ float lds_weights[MORPH_LDS_TARGETS];
    __shared__ uint32_t chunk[ROW_CHUNK_WORDS];
    const bool w_lds = stage_weights(lds_weights, weights, targets_count);
    __syncthreads();
    const uint32_t v0 = blockIdx.x * blockDim.x, i = v0 + threadIdx.x;
    const bool active = i < count;
    const uint32_t r0 = active ? row[i] : 0u, r1 = active ? row[i + 1] : 0u;
    rayhip_vertex b = {};
    Sums s = {};
    if (active) {
        b = base[i];
        morph_begin(b, s);
    }
    const uint32_t block_r0 = row[v0], block_r1 = row[min(v0 + blockDim.x, count)];
    if (w_lds) {
        row_sums(entries, r0, r1, block_r0, block_r1, lds_weights, chunk, s);
    } else {
        row_sums(entries, r0, r1, block_r0, block_r1, weights, chunk, s);
    }
    if (!active) {
        return;
    }
    rayhip_vertex out;
    morph_end(b, s, out);
    staged[i] = out;
    if (rayhip_skin::vertex_check(out, used[i] != 0)) {
        atomicAdd(n_bad, 1u);
    }
}

// one lane per vertex of a morph set that a skin covers: the morphed record goes straight into skin_vertex and never through memory.
// base / row / used / staged and the skin's `indices` / `skin_weights` all start at the set's first vertex (8-byte index records and
// 16-byte weight records stay aligned at any vertex offset); the palette as in k_skin_vertices.
__global__ void __launch_bounds__(256)
    k_morph_skin_vertices(const rayhip_vertex *__restrict__ base, const uint32_t *__restrict__ row, const Entry *__restrict__ entries, const uint32_t count,
                          const float *__restrict__ weights, const uint32_t targets_count, const uint16_t *__restrict__ indices,
                          const float *__restrict__ skin_weights, const float *__restrict__ bones, const uint32_t bones_count, const uint8_t *__restrict__ used,
                          rayhip_vertex *__restrict__ staged, uint32_t *__restrict__ n_bad) {
    __shared__ float palette[rayhip_skin::SKIN_LDS_BONES * 12];
    __shared__ float lds_weights[MORPH_LDS_TARGETS];
    __shared__ uint32_t chunk[ROW_CHUNK_WORDS];
    const bool in_lds = bones_count <= rayhip_skin::SKIN_LDS_BONES; // (uniform over the launch)
    if (in_lds) {
        for (uint32_t k = threadIdx.x; k < bones_count * 12u; k += blockDim.x) {
            palette[k] = bones[k];
        }
    }
    const bool w_lds = stage_weights(lds_weights, weights, targets_count);
    __syncthreads();
    const uint32_t v0 = blockIdx.x * blockDim.x, i = v0 + threadIdx.x;
    const bool active = i < count;
    const uint32_t r0 = active ? row[i] : 0u, r1 = active ? row[i + 1] : 0u;
    rayhip_vertex b = {};
    Sums s = {};
    uint2 packed = {};
    float4 w4 = {};
    if (active) {
        b = base[i];
        morph_begin(b, s);
        packed = reinterpret_cast<const uint2 *>(indices)[i]; // (the influences: asked for before the barriers of the row loop)
        w4 = reinterpret_cast<const float4 *>(skin_weights)[i];
    }
    const uint32_t block_r0 = row[v0], block_r1 = row[min(v0 + blockDim.x, count)];
    if (w_lds) {
        row_sums(entries, r0, r1, block_r0, block_r1, lds_weights, chunk, s);
    } else {
        row_sums(entries, r0, r1, block_r0, block_r1, weights, chunk, s);
    }
    if (!active) {
        return;
    }
    rayhip_vertex morphed, out;
    morph_end(b, s, morphed);
    const uint16_t idx[4] = {uint16_t(packed.x & 0xffffu), uint16_t(packed.x >> 16), uint16_t(packed.y & 0xffffu), uint16_t(packed.y >> 16)};
    const float sw[4] = {w4.x, w4.y, w4.z, w4.w};
    if (in_lds) {
        rayhip_skin::skin_vertex(morphed, idx, sw, palette, out);
    } else {
        rayhip_skin::skin_vertex(morphed, idx, sw, bones, out);
    }
    staged[i] = out;
    if (rayhip_skin::vertex_check(out, used[i] != 0)) {
        atomicAdd(n_bad, 1u);
    }
}

} // namespace rayhip_morph
