// texture_update.h -- new texels for a texture the scene holds, as the DEVICE turns them into what the texel pool keeps
// (rayhip_scene_set_texture): a restatement of the reference's real-time block compressor (internal/TextureUtils.cpp,
// TextureUtilsSSE2.cpp) and of the mip builder of TexStorageBCn<N>::Allocate (TextureStorageCPU.cpp:314-417).  Element functions shared
// by the device kernels (texture_update.hip.h) and a plain-loop host driver (tests/hostsim/hostsim_texture.cpp), like env_qtree.h and
// materials.h.  Integer arithmetic only, in a STATED ORDER; every function names the reference form it follows.  The reference has a
// _Ref and an _SSE2 form of each step and runs the _SSE2 one on x86, so that is the form restated where the two are written
// differently (pmulhw in place of divisions, pavgb, saturating byte adds, psadbw).  tests/test_texture_hostsim.py holds the result
// against pools the reference built, bit for bit; no input was found on which the two forms disagree.
//
//   storage 5 (BC3, YCoCg)   RGB -> (Co, Cg, 0, Y) per texel (RGB_to_YCoCg, ConvertRGB_to_CoCgxY), then Emit_BC3_Block_SSE2<true>:
//                            the box of all four bytes WITHOUT inset, ScaleYCoCg, InsetYCoCgBBox, SelectYCoCgDiagonal, the 6-step
//                            ramp over Y (bytes 0-7), the colour block over (Co, Cg, scale) (bytes 8-15)
//   storage 6 (BC4)          Emit_BC4_Block_SSE2 over R: end points max, min, then sixteen 3-bit selectors
//   storage 7 (BC5)          two such blocks, R then G
//   incomplete block         a level whose side is no multiple of 4 (or below 4) repeats its last column / row
//                            (ExtractIncomplete4x4Block_Ref): the texel coordinate clamped to the level
//   mip i from mip i - 1     of the SOURCE channels, not of decoded blocks: (c00 + c10 + c11 + c01) / 4 per channel, res[i] = res[i - 1] / 2,
//                            a level exists while both sides of the one above are >= 4.  The reference clamps its taps with
//                            min(2 x + 1, w - 1); under that halving 2 x + 1 <= 2 (w / 2 - 1) + 1 <= w - 1, so the clamp never
//                            binds and is left out.
//
// A block is computed by ONE unit (a lane; an iteration of the host loop) from sixteen RGBA8 words it gathered, all state in registers.
#pragma once

#include <stdint.h>

#include "rt_base.h"

namespace rayhip_texture_update {

constexpr uint32_t STORAGE_BC1 = 4, STORAGE_BC3 = 5, STORAGE_BC4 = 6, STORAGE_BC5 = 7;
constexpr int MAX_LEVELS = 12; // rayhip_texture::offset[12]

// 32-bit words of a 4 x 4 block of a storage
RT_HD uint32_t block_words(const uint32_t storage) { return (storage == STORAGE_BC3 || storage == STORAGE_BC5) ? 4u : 2u; }
RT_HD uint32_t tiles(const uint32_t n) { return (n + 3u) / 4u; }
// words a level of w x h texels takes in the pool: blocks in row-major tile order for the block storages, texels otherwise
RT_HD uint64_t level_words(const uint32_t storage, const bool blocks, const uint32_t w, const uint32_t h) {
    return blocks ? uint64_t(tiles(w)) * tiles(h) * block_words(storage) : uint64_t(w) * h;
}

// pmulhw with a positive multiplier on a non-negative 16-bit value: the high half of the product
RT_HD int mulhi16(const int a, const int b) { return (a * b) >> 16; }
// packuswb of a 16-bit lane
RT_HD int packus(const int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// ---- the 6-step ramp of a single channel: EmitAlphaIndicesInternal_SSE2 -----------------------------------------------------------------
// v[16]: the channel's bytes; returns the sixteen 3-bit selectors, texel k at bits 3 k .. 3 k + 2.  Divisions by 14 and 7 as pmulhw
// with (1 << 16) / 14 + 1 and (1 << 16) / 7 + 1; the thresholds saturate (packuswb); "a <= ab" is min(ab, a) == a.
RT_HD uint64_t ramp_selectors(const uint32_t v[16], const int mn, const int mx) {
    const int mid = mulhi16(mx - mn, (1 << 16) / 14 + 1);
    int ab[7];
    ab[0] = packus(mn + mid);
    for (int k = 1; k < 7; ++k) {
        ab[k] = packus(mulhi16((7 - k) * mx + k * mn, (1 << 16) / 7 + 1) + mid);
    }
    uint64_t bits = 0;
    for (int i = 0; i < 16; ++i) {
        const int a = int(v[i]);
        int index = 0;
        for (int k = 0; k < 7; ++k) {
            index += a <= ab[k] ? 1 : 0;
        }
        index = (index + 1) & 7;
        index ^= (2 > index) ? 1 : 0;
        bits |= uint64_t(uint32_t(index)) << (3 * i);
    }
    return bits;
}

// Emit_BC4_Block_SSE2: the box of the sixteen bytes (GetMinMaxAlphaByBBox_SSE2), max, min, the selectors
RT_HD void emit_bc4(const uint32_t v[16], uint32_t out[2]) {
    uint32_t mn = 255u, mx = 0u;
    for (int i = 0; i < 16; ++i) {
        mn = v[i] < mn ? v[i] : mn;
        mx = v[i] > mx ? v[i] : mx;
    }
    const uint64_t block = uint64_t(mx) | (uint64_t(mn) << 8) | (ramp_selectors(v, int(mn), int(mx)) << 16);
    out[0] = uint32_t(block), out[1] = uint32_t(block >> 32);
}

// ---- the colour block: EmitColorIndices_SSE2 --------------------------------------------------------------------------------------------
// an end point as the decoder sees it after RGB565: the top bits replicated into the low ones; byte 3 is 0
RT_HD uint32_t through_565(const uint32_t c) {
    const uint32_t r = c & 0xf8u, g = (c >> 8) & 0xfcu, b = (c >> 16) & 0xf8u;
    return (r | (r >> 5)) | ((g | (g >> 6)) << 8) | ((b | (b >> 5)) << 16);
}
// rgb888_to_rgb565
RT_HD uint32_t to_565(const uint32_t c) { return (((c & 0xffu) >> 3) << 11) | ((((c >> 8) & 0xffu) >> 2) << 5) | (((c >> 16) & 0xffu) >> 3); }
// (2 a + b) / 3 per channel, the division as pmulhw with (1 << 16) / 3 + 1
RT_HD uint32_t two_to_one(const uint32_t a, const uint32_t b) {
    uint32_t out = 0;
    for (int s = 0; s < 24; s += 8) {
        const int ca = int((a >> s) & 0xffu), cb = int((b >> s) & 0xffu);
        out |= uint32_t(packus(mulhi16(ca + ca + cb, (1 << 16) / 3 + 1))) << s;
    }
    return out;
}
// psadbw over the four bytes of a texel and a palette colour (whose byte 3 is 0: the texel's byte 3 enters every distance alike)
RT_HD uint32_t sad4(const uint32_t a, const uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sad_u8(a, b, 0u);
#else
    uint32_t d = 0;
    for (int s = 0; s < 32; s += 8) {
        const int x = int((a >> s) & 0xffu) - int((b >> s) & 0xffu);
        d += uint32_t(x < 0 ? -x : x);
    }
    return d;
#endif
}
// px[16]: the texels; mn, mx: the end points (bytes 0-2).  Sixteen 2-bit selectors, texel k at bits 2 k, 2 k + 1
RT_HD uint32_t colour_selectors(const uint32_t px[16], const uint32_t mn, const uint32_t mx) {
    const uint32_t c0 = through_565(mx), c1 = through_565(mn);
    const uint32_t c2 = two_to_one(c0, c1), c3 = two_to_one(c1, c0);
    uint32_t result = 0;
    for (int i = 0; i < 16; ++i) {
        const uint32_t d0 = sad4(px[i], c0), d1 = sad4(px[i], c1), d2 = sad4(px[i], c2), d3 = sad4(px[i], c3);
        const uint32_t b0 = d0 > d3, b1 = d1 > d2, b2 = d0 > d2, b3 = d1 > d3, b4 = d2 > d3;
        const uint32_t x0 = b1 & b2, x1 = b0 & b3, x2 = b0 & b4;
        result |= (x2 | ((x0 | x1) << 1)) << (2 * i);
    }
    return result;
}

// ---- storage 5: BC3 over YCoCg ----------------------------------------------------------------------------------------------------------
// RGB_to_YCoCg + ConvertRGB_to_CoCgxY: (Co, Cg, 0, Y) of an RGBA8 word; C's division, which truncates towards zero
RT_HD uint32_t to_cocg_y(const uint32_t rgba) {
    const int r = int(rgba & 0xffu), g = int((rgba >> 8) & 0xffu), b = int((rgba >> 16) & 0xffu);
    const int y = (r + 2 * g + b) / 4, co = packus(128 + (r - b) / 2), cg = packus(128 + (-r + 2 * g - b) / 4);
    return uint32_t(co) | (uint32_t(cg) << 8) | (uint32_t(y) << 24);
}

// Emit_BC3_Block_SSE2<true> over sixteen RGBA8 texels
RT_HD void emit_bc3_ycocg(const uint32_t rgba[16], uint32_t out[4]) {
    uint32_t px[16];
    int mn[4] = {255, 255, 255, 255}, mx[4] = {0, 0, 0, 0};
    // GetMinMaxColorByBBox_SSE2<true, true>: the box of all four bytes, no inset
    for (int i = 0; i < 16; ++i) {
        px[i] = to_cocg_y(rgba[i]);
        for (int ch = 0; ch < 4; ++ch) {
            const int v = int((px[i] >> (8 * ch)) & 0xffu);
            mn[ch] = v < mn[ch] ? v : mn[ch];
            mx[ch] = v > mx[ch] ? v : mx[ch];
        }
    }
    { // ScaleYCoCg_SSE2: chroma that stays within 63 / 31 of 128 is doubled / quadrupled; the scale goes into byte 2 of both end points.
      // The 16-bit multiply of the SSE2 form carries from Co into Cg, and its mask ~(scale - 1) takes the carry off again: per byte it
      // is (c - 128) * scale + 128 modulo 256, the _Ref form.
        int m0 = mn[0] - 128, m1 = mn[1] - 128, m2 = mx[0] - 128, m3 = mx[1] - 128;
        m0 = m0 < 0 ? -m0 : m0, m1 = m1 < 0 ? -m1 : m1, m2 = m2 < 0 ? -m2 : m2, m3 = m3 < 0 ? -m3 : m3;
        m0 = m1 > m0 ? m1 : m0;
        m2 = m3 > m2 ? m3 : m2;
        m0 = m2 > m0 ? m2 : m0;
        const int scale = 1 + (m0 <= 128 / 2 - 1 ? 1 : 0) + (m0 <= 128 / 4 - 1 ? 2 : 0);
        for (int ch = 0; ch < 2; ++ch) {
            mn[ch] = ((mn[ch] - 128) * scale + 128) & 0xff;
            mx[ch] = ((mx[ch] - 128) * scale + 128) & 0xff;
        }
        mn[2] = mx[2] = (scale - 1) * 8;
        for (int i = 0; i < 16; ++i) {
            const int co = ((int(px[i] & 0xffu) - 128) * scale + 128) & 0xff, cg = ((int((px[i] >> 8) & 0xffu) - 128) * scale + 128) & 0xff;
            px[i] = (px[i] & 0xffff0000u) | uint32_t(co) | (uint32_t(cg) << 8);
        }
    }
    { // InsetYCoCgBBox_SSE2: lanes Co, Cg by 1 / 16 with rounding term 7, Y by 1 / 32 with 15, the scale byte without inset; pmulhw by
      // 1 << (16 - shift) is the arithmetic shift (floor), and pmaxsw with 0 follows, so a negative sum gives 0 as the _Ref form's
      // truncating division does; then the RGB565 mask and the replicated top bits on lanes 0-2, packuswb
        const int shift[4] = {4, 4, 4, 5}, mask[4] = {0xf8, 0xfc, 0xf8, 0xff}, rep[4] = {5, 6, 5, 16};
        for (int ch = 0; ch < 4; ++ch) {
            const int inset = ch == 2 ? 0 : (mx[ch] - mn[ch]) - ((1 << (shift[ch] - 1)) - 1);
            int lo = (mn[ch] << shift[ch]) + inset, hi = (mx[ch] << shift[ch]) - inset;
            lo = lo < 0 ? 0 : lo >> shift[ch];
            hi = hi < 0 ? 0 : hi >> shift[ch];
            lo &= mask[ch], hi &= mask[ch];
            mn[ch] = packus(lo | (lo >> rep[ch])), mx[ch] = packus(hi | (hi >> rep[ch]));
        }
    }
    { // SelectYCoCgDiagonal_SSE2: the mid point with pavgb, the texels on the other diagonal counted (psadbw), Cg's end points swapped
      // when they are more than 8
        const uint32_t mid0 = uint32_t(mn[0] + mx[0] + 1) >> 1, mid1 = uint32_t(mn[1] + mx[1] + 1) >> 1;
        uint32_t side = 0;
        for (int i = 0; i < 16; ++i) {
            side += uint32_t((px[i] & 0xffu) >= mid0) ^ uint32_t(((px[i] >> 8) & 0xffu) >= mid1);
        }
        if (side > 8u) {
            const int t = mn[1];
            mn[1] = mx[1], mx[1] = t;
        }
    }
    uint32_t y[16];
    for (int i = 0; i < 16; ++i) {
        y[i] = px[i] >> 24;
    }
    const uint64_t alpha = uint64_t(uint32_t(mx[3])) | (uint64_t(uint32_t(mn[3])) << 8) | (ramp_selectors(y, mn[3], mx[3]) << 16);
    const uint32_t cmn = uint32_t(mn[0]) | (uint32_t(mn[1]) << 8) | (uint32_t(mn[2]) << 16);
    const uint32_t cmx = uint32_t(mx[0]) | (uint32_t(mx[1]) << 8) | (uint32_t(mx[2]) << 16);
    out[0] = uint32_t(alpha), out[1] = uint32_t(alpha >> 32);
    out[2] = to_565(cmx) | (to_565(cmn) << 16);
    out[3] = colour_selectors(px, cmn, cmx);
}

// the block of `storage` (5 with the YCoCg bit, 6 or 7) over sixteen RGBA8 texels: block_words(storage) words
template <uint32_t storage> RT_HD void emit_block(const uint32_t rgba[16], uint32_t *out) {
    if (storage == STORAGE_BC3) {
        emit_bc3_ycocg(rgba, out);
    } else {
        uint32_t v[16];
        for (int i = 0; i < 16; ++i) {
            v[i] = rgba[i] & 0xffu;
        }
        emit_bc4(v, out);
        if (storage == STORAGE_BC5) {
            for (int i = 0; i < 16; ++i) {
                v[i] = (rgba[i] >> 8) & 0xffu;
            }
            emit_bc4(v, out + 2);
        }
    }
}

// ---- gathering the sixteen texels of block (bx, by) -------------------------------------------------------------------------------------
// from a level of w x h RGBA8 words, row-major: coordinates clamped to the level (ExtractIncomplete4x4Block_Ref)
RT_HD void gather_block(const uint32_t *__restrict__ src, const int w, const int h, const int bx, const int by, uint32_t rgba[16]) {
    if (4 * bx + 3 < w) { // a complete row of four: adjacent words
        for (int j = 0; j < 4; ++j) {
            const int y = 4 * by + j < h ? 4 * by + j : h - 1;
            const uint32_t *row = src + size_t(y) * size_t(w) + size_t(4 * bx);
            rgba[4 * j + 0] = row[0], rgba[4 * j + 1] = row[1], rgba[4 * j + 2] = row[2], rgba[4 * j + 3] = row[3];
        }
    } else {
        for (int j = 0; j < 4; ++j) {
            const int y = 4 * by + j < h ? 4 * by + j : h - 1;
            for (int i = 0; i < 4; ++i) {
                const int x = 4 * bx + i < w ? 4 * bx + i : w - 1;
                rgba[4 * j + i] = src[size_t(y) * size_t(w) + size_t(x)];
            }
        }
    }
}

// (a + b + c + d) / 4 per byte of four RGBA8 words
RT_HD uint32_t average4(const uint32_t a, const uint32_t b, const uint32_t c, const uint32_t d) {
    const uint32_t even = (a & 0x00ff00ffu) + (b & 0x00ff00ffu) + (c & 0x00ff00ffu) + (d & 0x00ff00ffu);
    const uint32_t odd = ((a >> 8) & 0x00ff00ffu) + ((b >> 8) & 0x00ff00ffu) + ((c >> 8) & 0x00ff00ffu) + ((d >> 8) & 0x00ff00ffu);
    return ((even >> 2) & 0x00ff00ffu) | (((odd >> 2) & 0x00ff00ffu) << 8);
}

// The sixteen texels of block (bx, by) of a level of w x h = (sw / 2) x (sh / 2), averaged from the level above it (`src`, sw x sh RGBA8
// words); the texels that lie inside the level are also written to `stage` (w x h words, row-major; may be null), the source of the
// next level.  Order of the sum as the reference's: c00 + c10 + c11 + c01 (integer, so any order gives the same).
RT_HD void gather_mip_block(const uint32_t *__restrict__ src, const int sw, const int w, const int h, const int bx, const int by, uint32_t *__restrict__ stage,
                            uint32_t rgba[16]) {
    for (int j = 0; j < 4; ++j) {
        const int y = 4 * by + j < h ? 4 * by + j : h - 1;
        for (int i = 0; i < 4; ++i) {
            const int x = 4 * bx + i < w ? 4 * bx + i : w - 1;
            const uint32_t *p = src + size_t(2 * y) * size_t(sw) + size_t(2 * x);
            const uint32_t v = average4(p[0], p[1], p[size_t(sw) + 1], p[size_t(sw)]);
            rgba[4 * j + i] = v;
            if (stage && 4 * bx + i < w && 4 * by + j < h) {
                stage[size_t(y) * size_t(w) + size_t(x)] = v;
            }
        }
    }
}

// ---- the levels a texture holds ---------------------------------------------------------------------------------------------------------
// a level is held where its offset differs from the one before it (a missing level aliases the last real one)
template <typename Texture> RT_HD int levels_held(const Texture &t) {
    int n = 1;
    while (n < MAX_LEVELS && t.offset[n] != t.offset[n - 1]) {
        ++n;
    }
    return n;
}
// do the held levels follow TexStorageBCn<N>::Allocate: res[i] = res[i - 1] / 2 while both sides of the one above are >= 4?
template <typename Texture> RT_HD bool halving_chain(const Texture &t, const int n) {
    for (int i = 1; i < n; ++i) {
        if (t.width[i - 1] < 4u || t.height[i - 1] < 4u || t.width[i] != t.width[i - 1] / 2u || t.height[i] != t.height[i - 1] / 2u) {
            return false;
        }
    }
    return true;
}

} // namespace rayhip_texture_update
