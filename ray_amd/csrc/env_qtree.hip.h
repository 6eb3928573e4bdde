// env_qtree.hip.h -- the kernels that build the environment map's importance quadtree on the device (element functions: env_qtree.h;
// launcher: rayhip_environment.hip.h).  Every kernel writes the FULL pyramid of the map's res, mips one behind the other, finest first.
#pragma once

#include <hip/hip_runtime.h>

#include "env_qtree.h"
#include "light_refit.h"

namespace rayhip_env_qtree {

// A workgroup computes a tile of TILE x TILE cells of the finest level.  The 25 taps of a cell lie on the half-cell grid and
// neighbouring cells share them, so the tile's (2 TILE + 3)^2 grid points are evaluated ONCE into LDS -- 4.8 chains of sqrtf, sinf,
// cosf, acosf, atan2f and a texel read per cell instead of 25 -- and the 5 x 5 stride-2 stencil runs out of LDS in the reference's
// order.  The wrap-around is part of the tap (fract), so a tile at the map's edge takes no other path.  TILE 16, 256 lanes: 1225 + 256
// floats of LDS (5.8 KB), one cell per lane; each quad leaves as one float4.
constexpr int TILE = 16, TAPS = 2 * TILE + 3;

__global__ void __launch_bounds__(TILE *TILE) k_env_qtree_finest(const uint32_t *__restrict__ map, const int w, const int h, const int res, float4 *__restrict__ pyramid) {
    __shared__ float taps[TAPS * TAPS];
    __shared__ float cells[TILE * TILE];
    const int x0 = int(blockIdx.x) * TILE, y0 = int(blockIdx.y) * TILE;
    // the part of the tile that lies inside the level (res is a power of two: below TILE, or a multiple of it)
    const int nx = res - x0 < TILE ? res - x0 : TILE, ny = res - y0 < TILE ? res - y0 : TILE;
    const int tx = 2 * nx + 3, ty = 2 * ny + 3;
    for (int i = int(threadIdx.x); i < tx * ty; i += TILE * TILE) {
        const int ax = i % tx, ay = i / tx;
        taps[ay * TAPS + ax] = tap_luminance(map, w, h, res, 2 * x0 - 1 + ax, 2 * y0 - 1 + ay);
    }
    __syncthreads();
    const int cx = int(threadIdx.x) % TILE, cy = int(threadIdx.x) / TILE;
    if (cx < nx && cy < ny) {
        const float v = finest_cell(x0 + cx, y0 + cy, [&](const int hx, const int hy) { return taps[(hy - (2 * y0 - 1)) * TAPS + (hx - (2 * x0 - 1))]; });
        // the four cells of a quad side by side, in the quad's order
        cells[((cy / 2) * (TILE / 2) + cx / 2) * 4 + ((cx & 1) | ((cy & 1) << 1))] = v;
    }
    __syncthreads();
    const int qx = int(threadIdx.x) % (TILE / 2), qy = int(threadIdx.x) / (TILE / 2);
    if (threadIdx.x < (TILE / 2) * (TILE / 2) && 2 * qx < nx && 2 * qy < ny) {
        const float *c = &cells[(qy * (TILE / 2) + qx) * 4];
        pyramid[size_t(y0 / 2 + qy) * quads_per_side(res, 0) + size_t(x0 / 2 + qx)] = mkfloat4(c[0], c[1], c[2], c[3]);
    }
}

// one upper mip from the one below it, a quad per lane (the mips too large for the single workgroup below)
__global__ void __launch_bounds__(256) k_env_qtree_level(const float4 *__restrict__ below, float4 *__restrict__ mip, const uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n * n) {
        mip[i] = upper_quad(below, n, i % n, i / n);
    }
}

// the mips from `first` up to the coarsest in ONE workgroup: at most TOP_QUADS quads per side at `first`, a barrier between the levels
// (a level reads what the same workgroup wrote to global memory before the barrier)
constexpr uint32_t TOP_QUADS = 16;

__global__ void __launch_bounds__(256) k_env_qtree_top(float4 *pyramid, const int res, const int first, const int n_levels) {
    for (int l = first; l < n_levels; ++l) {
        const uint32_t n = quads_per_side(res, l);
        const float4 *below = pyramid + level_offset(res, l - 1);
        float4 *mip = pyramid + level_offset(res, l);
        for (uint32_t i = threadIdx.x; i < n * n; i += blockDim.x) {
            mip[i] = upper_quad(below, n, i % n, i / n);
        }
        __threadfence_block();
        __syncthreads();
    }
}

// The flags: blockIdx.y is the mip, the blocks of a row stride over its quads.  A wavefront that holds a quad with a cell above the
// threshold sets the mip's word with one atomic.  total_lum is the coarsest quad's sum, which every lane computes for itself; the first
// lane of the grid writes it and medium_lum next to the flags (zeroed by the caller).
__global__ void __launch_bounds__(256) k_env_qtree_flags(const float4 *__restrict__ pyramid, const int res, const int n_levels, Block *__restrict__ block) {
    const int l = int(blockIdx.y);
    const float total = total_luminance(pyramid[level_offset(res, n_levels - 1)]);
    const uint32_t n = quads_per_side(res, l), count = n * n;
    const float4 *mip = pyramid + level_offset(res, l);
    bool any = false;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
        any = any || quad_needs_subdivision(mip[i], total);
    }
    if (__ballot(any) != 0ull && (threadIdx.x & 63u) == 0u) {
        atomicOr(&block->flag[l], 1u);
    }
    if (l == 0 && blockIdx.x == 0 && threadIdx.x == 0) {
        block->total_lum = total;
        block->medium_lum = medium_luminance(total, res);
    }
}

// the environment light's leaf of the light refit takes its flux from the block; the slot is marked in `posed`, so that the level
// launches write flux, axis and cosines of its slot from the summary (light_refit.h)
__global__ void k_env_light_leaf(const Block *__restrict__ block, const uint32_t light_index, rayhip_light_refit::Summary *__restrict__ leaf, uint8_t *__restrict__ posed) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        leaf[light_index].flux = env_light_flux(block->medium_lum);
        posed[light_index] = 1;
    }
}

} // namespace rayhip_env_qtree
