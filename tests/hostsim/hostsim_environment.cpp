// hostsim_environment.cpp -- TEST INFRASTRUCTURE.  The environment map's importance quadtree as the device builds it
// (ray_amd/csrc/env_qtree.h: the tap, the finest level, the upper levels, the sums, the level decision, the environment light's flux),
// compiled with g++ (the HOSTSIM_FLAGS of hostsim.cpp: no fma contraction, SSE2, glibc libm) over plain arrays, with the prefix hostsim_
// and without a context.  tests/test_env_hostsim.py holds these against the quadtrees the reference built and a float64 numpy model;
// tests/test_gpu_environment.py holds the device (env_qtree.hip.h) against this file.
//
// Never linked into librayhip.so, and links nothing of the reference.
#include <string.h>

#include "../../include/rayhip.h"
#include "../../ray_amd/csrc/env_qtree.h"

#define HS_API extern "C" __attribute__((visibility("default")))

namespace eq = rayhip_env_qtree;

HS_API int hostsim_env_qtree_res(int w, int h) { return eq::finest_res(w, h); }

// quads of the full pyramid of `res`, and the first quad of each of its mips in offsets[16] (finest first)
HS_API uint32_t hostsim_env_qtree_layout(int res, uint32_t *offsets) {
    const int n = eq::full_levels(res);
    for (int l = 0; l < eq::MAX_LEVELS; ++l) {
        offsets[l] = eq::level_offset(res, l < n ? l : n);
    }
    return eq::level_offset(res, n);
}

// positions[2 res][2 res][2]: (u * w, theta * h) of the tap at half-grid point (hx, hy), 0 <= hx, hy < 2 res -- every tap of the level
// is one of these (the coordinate wraps) -- and lum[2 res][2 res], its luminance
HS_API int hostsim_env_qtree_taps(const uint32_t *map, int w, int h, float *positions, float *lum) {
    const int res = eq::finest_res(w, h);
    for (int hy = 0; hy < 2 * res; ++hy) {
        for (int hx = 0; hx < 2 * res; ++hx) {
            const rt::f2 p = eq::tap_map_position(w, h, res, hx, hy);
            const size_t i = size_t(hy) * (2 * res) + hx;
            positions[2 * i] = p.x, positions[2 * i + 1] = p.y;
            lum[i] = eq::tap_luminance(map, w, h, res, hx, hy);
        }
    }
    return 0;
}

// the full pyramid of a map and its block (18 words: 16 flags, total_lum, medium_lum); 1: the map is too small to have a quad
HS_API int hostsim_env_qtree_build(const uint32_t *map, int w, int h, float *pyramid, void *block) {
    const int res = eq::finest_res(w, h), n = eq::full_levels(res);
    if (n < 1 || n > eq::MAX_LEVELS) {
        return 1;
    }
    eq::finest_host(map, w, h, reinterpret_cast<float4 *>(pyramid));
    eq::Block b;
    eq::finish_host(res, reinterpret_cast<float4 *>(pyramid), b);
    memcpy(block, &b, sizeof(b));
    return 0;
}

// the upper mips, sums and flags over a finest level that is in place in `pyramid`
HS_API int hostsim_env_qtree_finish(int res, float *pyramid, void *block) {
    const int n = eq::full_levels(res);
    if (n < 1 || n > eq::MAX_LEVELS) {
        return 1;
    }
    eq::Block b;
    eq::finish_host(res, reinterpret_cast<float4 *>(pyramid), b);
    memcpy(block, &b, sizeof(b));
    return 0;
}

HS_API int hostsim_env_levels_kept(const uint32_t *flags, int n) { return eq::levels_kept(flags, n); }

HS_API float hostsim_env_light_flux(float medium_lum) { return eq::env_light_flux(medium_lum); }

// env_libm.h over arrays: which 0 sinf, 1 cosf, 2 acosf (a), 3 atan2f (a = y, b = x)
HS_API int hostsim_env_libm(int which, uint32_t n, const float *a, const float *b, float *out) {
    namespace lm = rayhip_env_libm;
    for (uint32_t i = 0; i < n; ++i) {
        out[i] = which == 0 ? lm::sin_f(a[i]) : which == 1 ? lm::cos_f(a[i]) : which == 2 ? lm::acos_f(a[i]) : lm::atan2_f(a[i], b[i]);
    }
    return 0;
}
