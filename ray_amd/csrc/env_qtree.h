// env_qtree.h -- the importance quadtree of the environment map as the DEVICE builds it when the map's texels change on the device
// (rayhip_scene_set_env_map, rayhip_scene_set_sky): a restatement of Ray::Cpu::Scene::PrepareEnvMapQTree_nolock (SceneCPU.cpp:1058-1212)
// and of the environment light's flux in RebuildLightTree_nolock (SceneCPU.cpp:1344-1358).  Element functions shared by the device
// kernels (env_qtree.hip.h) and a plain-loop host driver (tests/hostsim/hostsim_environment.cpp), like instances.h and light_pose.h:
// IEEE operations in a STATED ORDER without contraction on both sides.  The taps take sinf, cosf, acosf and atan2f from env_libm.h,
// which restates the reference's C library bit for bit: on a map whose width is a power of two EVERY tap's coordinate u * w is a whole
// number in exact arithmetic, the texel read there hangs on the last bit of atan2f, and with a libm of its own the device built another
// (equally valid) tree than the reference -- 53 of 1364 cells on a 128 x 64 map -- whose frames differ pixel by pixel.  With them host
// build, device and reference produce the same finest level.
//
//   res        the largest power of two with 2 * (res / 2) < min(w, h): start at 1, double while 2 * res < min(w, h)
//   tap        at the half-cell grid point (hx, hy), hx = 2 * qx + 1 + ii for tap ii = -2 .. 2 of cell qx: the reference's
//              (float(qx) + 0.5f + ii * 0.5f) is 0.5f * hx exactly, and so are the division by res and the 1 + ..., hence neighbouring
//              cells share their taps bit for bit and a tap is a function of (hx, hy) alone:
//                q = fract(1 + 0.5 * h / res) per axis;  d = square_to_direction(q, 0) (shade_lights.h: the reference's CanonicalToDir), restated
//                here over env_libm.h;
//                theta = acosf(clamp(d.y, -1, 1)) / PI;  phi = atan2f(d.z, d.x) wrapped into [0, 2 PI];  u = fract(0.5 * phi / PI);
//                texel (clamp(int(u * w), 0, w - 1), clamp(int(theta * h), 0, h - 1));  RGBE decode as latlong_rgbe;  (r + g) + b
//   finest     cell = the 25 taps in the reference's loop order, jj outer, ii inner: acc = acc + lum * W[ii + 2][jj + 2], W = k / 273.0f
//   upper      cell = ((p0 + p1) + p2) + p3 of the quad below it: given the same finest level every upper level has the reference's bits
//   total_lum  the coarsest quad summed ((a + b) + c) + d.  DIFFERENT FROM THE REFERENCE ON PURPOSE: it adds the finest level up in one
//              running sum of n float additions (65536 at res 512), whose worst-case error grows with n; the pyramid's own top is the
//              pairwise sum of the same cells, more accurate, and needs no serial pass.
//   medium_lum total_lum / float((res / 2) * (res / 2))
//   levels     per level "some cell > 0.005f * total_lum"; walking from the coarsest level down, the first level without such a cell
//              is the last one kept.  Finer levels are not addressed; nothing is copied.
//   env flux   (((1 + 1) + 1) / 3.0f) * medium_lum, times area 1: the environment light's colour is (1, 1, 1)
//
// Layout: mip L (0 = finest) has n = res >> (L + 1) quads per side, quad (x, y) at y * n + x, its four cells (cx & 1) | ((cy & 1) << 1);
// the full pyramid holds the mips one behind the other, finest first -- rayhip_scene_desc::env_qtree with every level kept.
#pragma once

#include <stdint.h>

#include "env_libm.h"
#include "shade_lights.h"

namespace rayhip_env_qtree {

using namespace rt;

constexpr int MAX_LEVELS = 16; // (rayhip_environment::qtree_levels: 0 .. 16; SceneView::env_qtree_offset)
constexpr float LUM_FRACT_THRESHOLD = 0.005f;

// what the flag pass leaves for the host: one word per level of the FULL pyramid (finest first), then the two sums
struct Block {
    uint32_t flag[MAX_LEVELS];
    float total_lum, medium_lum;
};
static_assert(sizeof(Block) == 72, "16 flags and 2 floats");

RT_HD int finest_res(const int w, const int h) {
    const int lowest = w < h ? w : h;
    int res = 1;
    while (2 * res < lowest) {
        res *= 2;
    }
    return res;
}
// mips of the full pyramid: log2(res); 0 for a map too small to have a quad
RT_HD int full_levels(const int res) {
    int n = 0;
    for (int r = res; r > 1; r /= 2) {
        ++n;
    }
    return n;
}
RT_HD uint32_t quads_per_side(const int res, const int level) { return uint32_t(res) >> (level + 1); }
// first quad of mip `level` in the full pyramid
RT_HD uint32_t level_offset(const int res, const int level) {
    uint32_t off = 0;
    for (int l = 0; l < level; ++l) {
        off += quads_per_side(res, l) * quads_per_side(res, l);
    }
    return off;
}

// the shared-exponent decode of latlong_rgbe (shade_lights.h; CoreRef.h:229-237), summed as the reference sums it
RT_HD float rgbe_luminance(const uint32_t px) {
    const float scale = exp2f(float((px >> 24) & 0xffu) - 128.0f);
    const uint32_t m0 = px & 0xffu, m1 = (px >> 8) & 0xffu, m2 = (px >> 16) & 0xffu;
    const float r = (uint_as_float(0x3f800000u + m0 * 0x8080u + (m0 + 1) / 2) - 1.0f) * scale;
    const float g = (uint_as_float(0x3f800000u + m1 * 0x8080u + (m1 + 1) / 2) - 1.0f) * scale;
    const float b = (uint_as_float(0x3f800000u + m2 * 0x8080u + (m2 + 1) / 2) - 1.0f) * scale;
    return (r + g) + b;
}

// coordinate of half-grid point `h` on an axis of `res` cells, as the reference computes it for (cell, tap)
RT_HD float tap_coordinate(const int res, const int h) { return fractf(1.0f + (0.5f * float(h)) / float(res)); }

// where the tap (hx, hy) reads the map: (u * w, theta * h) before the conversion to a texel (the tests measure these)
RT_HD f2 tap_map_position(const int w, const int h, const int res, const int hx, const int hy) {
    namespace lm = rayhip_env_libm;
    // square_to_direction(q, 0), operation for operation
    const float cos_theta = 2 * tap_coordinate(res, hx) - 1;
    const float dir_phi = wrap_two_pi(2 * PI * tap_coordinate(res, hy) + 0.0f);
    const float sin_theta = sqrtf(1 - cos_theta * cos_theta);
    const f3 d = f3{sin_theta * lm::cos_f(dir_phi), cos_theta, -sin_theta * lm::sin_f(dir_phi)};
    const float theta = lm::acos_f(clampf(d.y, -1.0f, 1.0f)) / PI;
    const float phi = wrap_two_pi(lm::atan2_f(d.z, d.x));
    const float u = fractf(0.5f * phi / PI);
    return f2{u * float(w), theta * float(h)};
}

// `map`: level 0 of the environment map, w x h RGBE8 texels, row-major
RT_HD float tap_luminance(const uint32_t *map, const int w, const int h, const int res, const int hx, const int hy) {
    const f2 p = tap_map_position(w, h, res, hx, hy);
    const int ix = clampi(int(p.x), 0, w - 1), iy = clampi(int(p.y), 0, h - 1);
    return rgbe_luminance(map[size_t(iy) * size_t(w) + size_t(ix)]);
}

// the 5 x 5 filter: k / 273.0f as the reference writes it (symmetric, so [ii + 2][jj + 2] is [jj + 2][ii + 2])
RT_HD float filter_weight(const int i, const int j) {
    const float k[5][5] = {{1 / 273.0f, 4 / 273.0f, 7 / 273.0f, 4 / 273.0f, 1 / 273.0f},
                           {4 / 273.0f, 16 / 273.0f, 26 / 273.0f, 16 / 273.0f, 4 / 273.0f},
                           {7 / 273.0f, 26 / 273.0f, 41 / 273.0f, 26 / 273.0f, 7 / 273.0f},
                           {4 / 273.0f, 16 / 273.0f, 26 / 273.0f, 16 / 273.0f, 4 / 273.0f},
                           {1 / 273.0f, 4 / 273.0f, 7 / 273.0f, 4 / 273.0f, 1 / 273.0f}};
    return k[i][j];
}

// cell (qx, qy) of the finest level from tap luminances: taps(hx, hy) for hx = 2 * qx - 1 .. 2 * qx + 3, the same for hy
template <typename Taps> RT_HD float finest_cell(const int qx, const int qy, const Taps &taps) {
    float acc = 0.0f;
    for (int jj = -2; jj <= 2; ++jj) {
        for (int ii = -2; ii <= 2; ++ii) {
            acc = acc + taps(2 * qx + 1 + ii, 2 * qy + 1 + jj) * filter_weight(ii + 2, jj + 2);
        }
    }
    return acc;
}

RT_HD float quad_sum(const float4 q) { return ((q.x + q.y) + q.z) + q.w; }

// quad (x, y) of an upper mip with n quads per side from the mip below it (2 n quads per side): its cell (cx, cy) is the sum of the
// lower quad (cx, cy) -- the reference's prev_mip[y * cur_res + x]
RT_HD float4 upper_quad(const float4 *below, const uint32_t n, const uint32_t x, const uint32_t y) {
    const size_t row0 = size_t(2 * y) * (2 * n), row1 = size_t(2 * y + 1) * (2 * n);
    return mkfloat4(quad_sum(below[row0 + 2 * x]), quad_sum(below[row0 + 2 * x + 1]), quad_sum(below[row1 + 2 * x]), quad_sum(below[row1 + 2 * x + 1]));
}

RT_HD float total_luminance(const float4 coarsest) { return quad_sum(coarsest); }
RT_HD float medium_luminance(const float total, const int res) { return total / float((res / 2) * (res / 2)); }
RT_HD bool quad_needs_subdivision(const float4 q, const float total) {
    const float t = LUM_FRACT_THRESHOLD * total;
    return q.x > t || q.y > t || q.z > t || q.w > t;
}
// levels kept, from the flags of the full pyramid's n mips (finest first): the walk from the coarsest mip down stops at the first one
// that needs no subdivision, which is the finest kept
RT_HD int levels_kept(const uint32_t *flag, const int n) {
    int kept = 0;
    for (int l = n - 1; l >= 0; --l) {
        ++kept;
        if (flag[l] == 0) {
            break;
        }
    }
    return kept;
}
RT_HD float env_light_flux(const float medium_lum) {
    const float lum = (1.0f + 1.0f) + 1.0f;
    return ((lum / 3.0f) * medium_lum) * 1.0f;
}

// ---- host side: plain loops over the functions above ---------------------------------------------------------------------------------
// the finest mip of a map's pyramid (quads_per_side(res, 0) squared quads)
inline void finest_host(const uint32_t *map, const int w, const int h, float4 *pyramid) {
    const int res = finest_res(w, h);
    const uint32_t n0 = quads_per_side(res, 0);
    for (int qy = 0; qy < res; ++qy) {
        for (int qx = 0; qx < res; ++qx) {
            const float v = finest_cell(qx, qy, [&](const int hx, const int hy) { return tap_luminance(map, w, h, res, hx, hy); });
            reinterpret_cast<float *>(&pyramid[size_t(qy / 2) * n0 + size_t(qx / 2)])[(qx & 1) | ((qy & 1) << 1)] = v;
        }
    }
}
// the upper mips, the sums and the flags over a finest level that is in place (the device's, in the tests)
inline void finish_host(const int res, float4 *pyramid, Block &block) {
    const int n_levels = full_levels(res);
    for (int l = 1; l < n_levels; ++l) {
        const uint32_t n = quads_per_side(res, l);
        const float4 *below = pyramid + level_offset(res, l - 1);
        float4 *mip = pyramid + level_offset(res, l);
        for (uint32_t y = 0; y < n; ++y) {
            for (uint32_t x = 0; x < n; ++x) {
                mip[size_t(y) * n + x] = upper_quad(below, n, x, y);
            }
        }
    }
    block = Block{};
    block.total_lum = total_luminance(pyramid[level_offset(res, n_levels - 1)]);
    block.medium_lum = medium_luminance(block.total_lum, res);
    for (int l = 0; l < n_levels; ++l) {
        const uint32_t n = quads_per_side(res, l);
        const float4 *mip = pyramid + level_offset(res, l);
        for (size_t i = 0; i < size_t(n) * n; ++i) {
            if (quad_needs_subdivision(mip[i], block.total_lum)) {
                block.flag[l] = 1;
                break;
            }
        }
    }
}

} // namespace rayhip_env_qtree
