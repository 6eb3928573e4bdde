// texture_update.hip.h -- the kernels that turn new texels into the blocks and mips a texture of the pool holds (element functions:
// texture_update.h; launcher: rayhip_textures.hip.h).  ONE LANE PER 4 x 4 BLOCK: it gathers its sixteen RGBA8 words (rows of four
// adjacent words; clamped texel by texel only in the last column of a ragged level), keeps every intermediate in registers -- no LDS,
// no scratch --, and stores its 8 or 16 bytes.  Source, staging and destination are assumed 4-byte aligned and no more: the pool packs
// textures word by word.  The launcher checked every level against the pool before the first launch.
#pragma once

#include <hip/hip_runtime.h>

#include "texture_update.h"

namespace rayhip_texture_update {

constexpr int LANES = 64; // a wavefront per workgroup: a 64 x 64 texture has 256 blocks, and four workgroups spread over four CUs

// level 0 from the caller's RGBA8 words (w x h, row-major) into `dst`, the level's blocks in row-major tile order
template <uint32_t storage> __global__ void __launch_bounds__(LANES) k_tex_compress(const uint32_t *__restrict__ src, const int w, const int h, uint32_t *__restrict__ dst) {
    const uint32_t tx = tiles(uint32_t(w)), n = tx * tiles(uint32_t(h));
    const uint32_t i = blockIdx.x * LANES + threadIdx.x;
    if (i >= n) {
        return;
    }
    uint32_t rgba[16], out[4];
    gather_block(src, w, h, int(i % tx), int(i / tx), rgba);
    emit_block<storage>(rgba, out);
    uint32_t *d = dst + size_t(i) * block_words(storage);
    for (uint32_t k = 0; k < block_words(storage); ++k) {
        d[k] = out[k];
    }
}

// level i (w x h) from level i - 1 (`src`, sw x sh with w = sw / 2, h = sh / 2): the lane that owns a block reads its 8 x 8 source
// texels, averages them, emits the block and leaves the averaged texels in `stage` (null behind the last level) for the next launch
template <uint32_t storage>
__global__ void __launch_bounds__(LANES) k_tex_mip_compress(const uint32_t *__restrict__ src, const int sw, const int w, const int h, uint32_t *__restrict__ stage,
                                                            uint32_t *__restrict__ dst) {
    const uint32_t tx = tiles(uint32_t(w)), n = tx * tiles(uint32_t(h));
    const uint32_t i = blockIdx.x * LANES + threadIdx.x;
    if (i >= n) {
        return;
    }
    uint32_t rgba[16], out[4];
    gather_mip_block(src, sw, w, h, int(i % tx), int(i / tx), stage, rgba);
    emit_block<storage>(rgba, out);
    uint32_t *d = dst + size_t(i) * block_words(storage);
    for (uint32_t k = 0; k < block_words(storage); ++k) {
        d[k] = out[k];
    }
}

} // namespace rayhip_texture_update
