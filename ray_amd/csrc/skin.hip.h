// skin.hip.h -- the device side of skinning (rayhip_scene_pose_skins, rayhip_scene_update_vertices_device; rayhip_deform.hip.h): the
// element functions of skin.h, one lane per vertex.  Both kernels only READ what a render pass reads: the posed vertices go to a
// staging array and the findings to counters, so a refused update has touched nothing.
#pragma once

#include <hip/hip_runtime.h>

#include "skin.h"

namespace rayhip_skin {

// one lane per vertex of ONE skin: rest record (44 bytes), four bone indices (8 bytes), four weights (16 bytes) in, the posed record
// out into `staged` (never the live vertex array).  `used`: per vertex of the skin's range, some triangle uses it.  `n_bad` counts
// used vertices whose posed position is not finite.  Palettes of up to SKIN_LDS_BONES bones are copied to LDS by the block first,
// larger ones are read from memory: the same arithmetic over the same values, hence the same bits.
__global__ void __launch_bounds__(256) k_skin_vertices(const rayhip_vertex *__restrict__ rest, const uint16_t *__restrict__ indices,
                                                      const float *__restrict__ weights, const uint32_t count, const float *__restrict__ bones,
                                                      const uint32_t bones_count, const uint8_t *__restrict__ used, rayhip_vertex *__restrict__ staged,
                                                      uint32_t *__restrict__ n_bad) {
    __shared__ float palette[SKIN_LDS_BONES * 12];
    const bool in_lds = bones_count <= SKIN_LDS_BONES; // (uniform over the launch)
    if (in_lds) {
        for (uint32_t k = threadIdx.x; k < bones_count * 12u; k += blockDim.x) {
            palette[k] = bones[k];
        }
        __syncthreads();
    }
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) {
        return;
    }
    const rayhip_vertex r = rest[i];
    const uint2 packed = reinterpret_cast<const uint2 *>(indices)[i];
    const float4 w4 = reinterpret_cast<const float4 *>(weights)[i];
    const uint16_t idx[4] = {uint16_t(packed.x & 0xffffu), uint16_t(packed.x >> 16), uint16_t(packed.y & 0xffffu), uint16_t(packed.y >> 16)};
    const float w[4] = {w4.x, w4.y, w4.z, w4.w};
    rayhip_vertex out;
    if (in_lds) {
        skin_vertex(r, idx, w, palette, out);
    } else {
        skin_vertex(r, idx, w, bones, out);
    }
    staged[i] = out;
    if (vertex_check(out, used[i] != 0)) {
        atomicAdd(n_bad, 1u);
    }
}

// what the device-pointer update checks of the caller's array before it is copied: lane i < count looks at vertex first + i
// (counters[0]: used vertices whose position is not finite), lane i < n_lights at the i-th vertex of a triangle light
// (counters[1]: those inside the range whose 44 bytes differ from the kept ones)
__global__ void __launch_bounds__(256) k_check_vertices(const rayhip_vertex *__restrict__ vertices, const uint32_t first, const uint32_t count,
                                                       const uint8_t *__restrict__ used, const uint32_t *__restrict__ light_index,
                                                       const rayhip_vertex *__restrict__ light_kept, const uint32_t n_lights,
                                                       uint32_t *__restrict__ counters) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count && vertex_check(vertices[i], used[first + i] != 0)) {
        atomicAdd(&counters[0], 1u);
    }
    if (i < n_lights) {
        const uint32_t v = light_index[i];
        if (v >= first && v - first < count && !same_bytes(vertices[v - first], light_kept[i])) {
            atomicAdd(&counters[1], 1u);
        }
    }
}

} // namespace rayhip_skin
