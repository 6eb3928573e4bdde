// rt_cache.h -- the spatial radiance cache: a hash grid of 64-bit voxel keys with integer radiance sums per voxel.
//
// Restates the reference's SHARC-style cache (internal/RadCacheRef.{h,cpp}, constants internal/Constants.inl:113-144, types
// internal/Core.h:480-535) as RT_HD functions, so that the same source runs in the device kernels (cache_kernels.hip.h) and in
// the host build (tests/hostsim/hostsim_cache.cpp).  The arithmetic keeps the reference's order and its SSE2 conversions
// (_mm_cvttps_epi32, the SSE2 floor of simd_sse.h:195-201), so the host build is bit-exact with the reference.
//
// The only memory writes are the 64-bit compare-and-swap of an insert and the 32-bit adds of an accumulation; both go through
// the small shim below (device atomics on gfx950, __atomic builtins on the host).
#pragma once

#include "rt_base.h"

namespace rt {
namespace cache {

// ---- constants: Constants.inl:113-144 --------------------------------------------------------------
constexpr uint32_t ENTRIES_COUNT = (1u << 22);
constexpr uint32_t POSITION_BIT_NUM = 17u;
constexpr uint32_t POSITION_BIT_MASK = (1u << POSITION_BIT_NUM) - 1;
constexpr uint32_t LEVEL_BIT_NUM = 10u;
constexpr uint32_t LEVEL_BIT_MASK = (1u << LEVEL_BIT_NUM) - 1;
constexpr uint32_t NORMAL_BIT_MASK = 7u;
constexpr uint32_t BUCKET_SIZE = 32u;
constexpr uint32_t INVALID_ENTRY = 0xFFFFFFFFu;
constexpr uint32_t LEVEL_BIAS = 2u;
constexpr uint64_t INVALID_KEY = 0u;

constexpr uint32_t SAMPLE_COUNT_MAX = 128;
constexpr uint32_t SAMPLE_COUNT_MIN = 8;
constexpr float RADIANCE_SCALE = 1e4f;
constexpr uint32_t SAMPLE_COUNTER_BIT_NUM = 20;
constexpr uint32_t SAMPLE_COUNTER_BIT_MASK = (1u << SAMPLE_COUNTER_BIT_NUM) - 1;
constexpr uint32_t FRAME_COUNTER_BIT_NUM = 32 - SAMPLE_COUNTER_BIT_NUM;
constexpr uint32_t FRAME_COUNTER_BIT_MASK = (1u << FRAME_COUNTER_BIT_NUM) - 1;
constexpr float LOGARITHM_BASE = 2.0f;
constexpr uint32_t STALE_FRAME_NUM_MAX = 128;
constexpr int DOWNSAMPLING_FACTOR = 4;
constexpr int PROPAGATION_DEPTH = 4;
constexpr float GRID_SCALE = 50.0f;
constexpr float MIN_ROUGHNESS = 0.4f;

// cache_grid_params_t (Core.h:496-501) == rayhip_cache_grid
struct GridParams {
    float cam_pos_curr[3], cam_pos_prev[3];
    float log_base, scale, exposure;
};

// packed_cache_voxel_t (Core.h:486-488): r, g, b sums scaled by RADIANCE_SCALE; samples (low 20 bits) | idle frames (high 12)
struct alignas(16) Voxel {
    uint32_t v[4];
};

// ---- atomics shim ----------------------------------------------------------------------------------
RT_HD uint64_t atomic_cas64(uint64_t *p, uint64_t expected, uint64_t desired) {
#if defined(__HIP_DEVICE_COMPILE__)
    return uint64_t(atomicCAS(reinterpret_cast<unsigned long long *>(p), (unsigned long long)expected, (unsigned long long)desired));
#else
    __atomic_compare_exchange_n(p, &expected, desired, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST);
    return expected; // the value found (== the expected one when the swap happened)
#endif
}
RT_HD void atomic_add32(uint32_t *p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(p, v);
#else
    __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST);
#endif
}

// ---- the reference's SSE2 conversions --------------------------------------------------------------
// _mm_cvttps_epi32: truncation, 0x80000000 for NaN and out-of-range lanes (the device's own conversion saturates instead)
RT_HD int32_t cvtt(float x) { return (x > -2147483904.0f && x < 2147483648.0f) ? int32_t(x) : int32_t(0x80000000u); }
// floor of simd_sse.h:195-201 (the non-SSE4.1 branch the reference is built with)
RT_HD float sse_floor(float x) {
    const float t = float(cvtt(x));
    return t - ((x < t) ? 1.0f : 0.0f);
}

// ---- hashing: RadCacheRef.h:12-25 ------------------------------------------------------------------
RT_HD uint32_t hash_jenkins32(uint32_t a) {
    a = (a + 0x7ed55d16u) + (a << 12);
    a = (a ^ 0xc761c23cu) ^ (a >> 19);
    a = (a + 0x165667b1u) + (a << 5);
    a = (a + 0xd3a2646cu) ^ (a << 9);
    a = (a + 0xfd7046c5u) + (a << 3);
    a = (a ^ 0xb55a4f09u) ^ (a >> 16);
    return a;
}
RT_HD uint32_t hash64(uint64_t key) { return hash_jenkins32(uint32_t(key & 0xffffffffu)) ^ hash_jenkins32(uint32_t(key >> 32)); }

// ---- grid: Core.h:546,564-566, RadCacheRef.cpp:7-13,245-250 ----------------------------------------
// The device's logf is not glibc's: a few floats below a power of two its quotient can reach the integer and the point lands
// one level over (108 of the 1023 points 2^k (1 +- m ulp), k in [-6, 24], |m| <= 16).  On the device the logarithms are taken
// in double and rounded once: that gives glibc's level at all of them (tests/test_spatial_cache_hostsim.py pins the formula).
RT_HD float log_base(float x, float base) {
#if defined(__HIP_DEVICE_COMPILE__)
    return float(log(double(x))) / float(log(double(base)));
#else
    return logf(x) / logf(base);
#endif
}
RT_HD uint32_t calc_grid_level(f3 p, const GridParams &g) {
    const float distance = length(mk3(g.cam_pos_curr) - p);
    const float l = floorf(log_base(distance, g.log_base) + float(LEVEL_BIAS));
    return uint32_t(l < 1.0f ? 1.0f : (l > float(LEVEL_BIT_MASK) ? float(LEVEL_BIT_MASK) : l));
}
RT_HD float calc_voxel_size(uint32_t level, const GridParams &g) {
    return powf(g.log_base, float(level)) / (g.scale * powf(g.log_base, float(LEVEL_BIAS)));
}
RT_HD uint64_t pack_key(int32_t x, int32_t y, int32_t z, uint32_t level) {
    return ((uint64_t(uint32_t(x)) & POSITION_BIT_MASK) << (POSITION_BIT_NUM * 0)) |
           ((uint64_t(uint32_t(y)) & POSITION_BIT_MASK) << (POSITION_BIT_NUM * 1)) |
           ((uint64_t(uint32_t(z)) & POSITION_BIT_MASK) << (POSITION_BIT_NUM * 2)) |
           ((uint64_t(level) & LEVEL_BIT_MASK) << (POSITION_BIT_NUM * 3));
}
// RadCacheRef.cpp:23-40 (with normals)
RT_HD uint64_t compute_hash(f3 p, f3 n, const GridParams &g) {
    const uint32_t level = calc_grid_level(p, g);
    const float voxel_size = calc_voxel_size(level, g);
    uint64_t key = pack_key(cvtt(sse_floor(p.x / voxel_size)), cvtt(sse_floor(p.y / voxel_size)), cvtt(sse_floor(p.z / voxel_size)), level);
    const uint32_t normal_bits = (n.x >= 0.0f ? 1u : 0u) + (n.y >= 0.0f ? 2u : 0u) + (n.z >= 0.0f ? 4u : 0u);
    key |= uint64_t(normal_bits) << (POSITION_BIT_NUM * 3 + LEVEL_BIT_NUM);
    return key;
}
// RadCacheRef.cpp:42-94: the key of the same place one level coarser (camera moved closer) or finer (farther)
RT_HD uint64_t get_adjacent_level_hash(uint64_t key, const GridParams &g) {
    const uint32_t NegativeBit = 1u << (POSITION_BIT_NUM - 1);
    const uint32_t NegativeMask = ~((1u << POSITION_BIT_NUM) - 1);
    int32_t gp[3];
    for (int i = 0; i < 3; ++i) {
        const uint32_t c = uint32_t(key >> (POSITION_BIT_NUM * i)) & POSITION_BIT_MASK;
        gp[i] = int32_t((c & NegativeBit) ? (c | NegativeMask) : c);
    }
    int32_t level = int32_t(uint32_t(key >> (POSITION_BIT_NUM * 3)) & LEVEL_BIT_MASK);
    const float voxel_size = calc_voxel_size(uint32_t(level), g);
    // grid_dist2 in wrapping 32-bit arithmetic
    uint32_t d_curr = 0, d_prev = 0;
    for (int i = 0; i < 3; ++i) {
        const uint32_t vc = uint32_t(cvtt(sse_floor(g.cam_pos_curr[i] / voxel_size))) - uint32_t(gp[i]);
        const uint32_t vp = uint32_t(cvtt(sse_floor(g.cam_pos_prev[i] / voxel_size))) - uint32_t(gp[i]);
        d_curr += vc * vc;
        d_prev += vp * vp;
    }
    if (int32_t(d_curr) < int32_t(d_prev)) {
        for (int i = 0; i < 3; ++i) {
            gp[i] = cvtt(sse_floor(float(gp[i]) / g.log_base));
        }
        level = level + 1 < int32_t(LEVEL_BIT_MASK) ? level + 1 : int32_t(LEVEL_BIT_MASK);
    } else {
        for (int i = 0; i < 3; ++i) {
            gp[i] = cvtt(sse_floor(float(gp[i]) * g.log_base));
        }
        level = level - 1 > 1 ? level - 1 : 1;
    }
    return pack_key(gp[0], gp[1], gp[2], uint32_t(level)) | (key & (uint64_t(NORMAL_BIT_MASK) << (POSITION_BIT_NUM * 3 + LEVEL_BIT_NUM)));
}

// ---- hash map: RadCacheRef.cpp:96-127 --------------------------------------------------------------
RT_HD uint32_t bucket_base(uint64_t key, uint32_t entries_count) { return ((hash64(key) % entries_count) / BUCKET_SIZE) * BUCKET_SIZE; }

// first free (or equal) slot of the key's bucket, INVALID_ENTRY when the bucket is full of other keys (the reference answers slot 0
// there, so its losing keys' samples pile up in slot 0's voxel; this restatement drops them -- its one departure from the reference)
RT_HD uint32_t hash_map_insert(uint64_t *entries, uint32_t entries_count, uint64_t key) {
    const uint32_t base = bucket_base(key, entries_count);
    for (uint32_t off = 0; off < BUCKET_SIZE && base < entries_count; ++off) {
        const uint64_t prev = atomic_cas64(&entries[base + off], INVALID_KEY, key);
        if (prev == INVALID_KEY || prev == key) {
            return base + off;
        }
    }
    return INVALID_ENTRY;
}
// a bucket is compacted (its keys are a prefix of it), so the first empty slot ends the search
RT_HD uint32_t hash_map_find(const uint64_t *entries, uint32_t entries_count, uint64_t key) {
    const uint32_t base = bucket_base(key, entries_count);
    for (uint32_t off = 0; off < BUCKET_SIZE; ++off) {
        const uint64_t stored = entries[base + off];
        if (stored == key) {
            return base + off;
        } else if (stored == INVALID_KEY) {
            return INVALID_ENTRY;
        }
    }
    return INVALID_ENTRY;
}

// ---- voxels: Core.h:490-500, RadCacheRef.cpp:146-163 -----------------------------------------------
RT_HD void accumulate_voxel(Voxel &voxel, f3 r, uint32_t sample_data) {
    const uint32_t d0 = uint32_t(cvtt(r.x * RADIANCE_SCALE)), d1 = uint32_t(cvtt(r.y * RADIANCE_SCALE)), d2 = uint32_t(cvtt(r.z * RADIANCE_SCALE));
    if (d0) {
        atomic_add32(&voxel.v[0], d0);
    }
    if (d1) {
        atomic_add32(&voxel.v[1], d1);
    }
    if (d2) {
        atomic_add32(&voxel.v[2], d2);
    }
    if (sample_data) {
        atomic_add32(&voxel.v[3], sample_data);
    }
}
RT_HD uint32_t voxel_samples(const Voxel &v) { return v.v[3] & SAMPLE_COUNTER_BIT_MASK; }
RT_HD uint32_t voxel_frames(const Voxel &v) { return (v.v[3] >> SAMPLE_COUNTER_BIT_NUM) & FRAME_COUNTER_BIT_MASK; }

// The query of the shade path (ShadeRef.cpp:1380-1389): mean radiance of the voxel at (p, n) over the exposure, when the voxel
// holds at least SAMPLE_COUNT_MIN samples.  Returns the sample count (0: no answer).
RT_HD uint32_t query(const uint64_t *entries, const Voxel *voxels, uint32_t entries_count, f3 p, f3 n, const GridParams &g, f3 &out) {
    const uint32_t e = hash_map_find(entries, entries_count, compute_hash(p, n, g));
    if (e == INVALID_ENTRY) {
        return 0;
    }
    const Voxel v = voxels[e];
    const uint32_t count = voxel_samples(v);
    if (count < SAMPLE_COUNT_MIN) {
        return 0;
    }
    const f3 rad = mk3(float(v.v[0]) / RADIANCE_SCALE, float(v.v[1]) / RADIANCE_SCALE, float(v.v[2]) / RADIANCE_SCALE);
    out = (rad / float(count)) / g.exposure;
    return count;
}

// ---- the update step of one path (RadCacheRef.cpp:252-309) -----------------------------------------
// cache_data_t of one downsampled pixel, held by the caller (the device keeps it as SoA planes)
struct PathData {
    uint32_t entries[PROPAGATION_DEPTH];
    f3 weight[PROPAGATION_DEPTH];
    int32_t len;
};

// One vertex of the update pass: the radiance the bounce gathered at the pixel (the per-bounce colour of the update-mode shade,
// throughput not applied), the throughput of the ray that reached the vertex, and the vertex (position, geometric normal).
// `ends`: the ray left the scene or hit a light -- nothing is inserted, the radiance only flows back along the path.
RT_HD void update_path(PathData &pd, f3 p, f3 n, f3 radiance, f3 ray_c, bool ends, const GridParams &g, uint64_t *entries, uint32_t entries_count,
                       Voxel *voxels_curr) {
    f3 rad = radiance * g.exposure;
    pd.weight[0] *= ray_c;
    if (ends || pd.len == PROPAGATION_DEPTH) {
        for (int j = 0; j < PROPAGATION_DEPTH; ++j) {
            if (j < pd.len) {
                rad *= pd.weight[j];
                if (pd.entries[j] != INVALID_ENTRY) {
                    accumulate_voxel(voxels_curr[pd.entries[j]], rad, 0);
                }
            }
        }
    } else {
        for (int j = PROPAGATION_DEPTH - 1; j > 0; --j) {
            if (j <= pd.len) {
                pd.entries[j] = pd.entries[j - 1];
                pd.weight[j] = pd.weight[j - 1];
            }
        }
        pd.weight[0] = splat3(1.0f);
        pd.entries[0] = hash_map_insert(entries, entries_count, compute_hash(p, n, g));
        if (pd.entries[0] != INVALID_ENTRY) {
            accumulate_voxel(voxels_curr[pd.entries[0]], rad, 1);
        }
        ++pd.len;
        for (int j = 1; j < PROPAGATION_DEPTH; ++j) {
            if (j < pd.len) {
                rad *= pd.weight[j];
                if (pd.entries[j] != INVALID_ENTRY) {
                    accumulate_voxel(voxels_curr[pd.entries[j]], rad, 0);
                }
            }
        }
    }
}

// ---- resolve: RadCacheRef.cpp:311-393 --------------------------------------------------------------
RT_HD bool camera_moved(const GridParams &g) { return length2(mk3(g.cam_pos_curr) - mk3(g.cam_pos_prev)) > FLT_EPS_; }

// The resolved voxel of one live key: this frame's samples added to the previous frames', topped up from the adjacent level
// when the camera moved and the voxel is young, capped at SAMPLE_COUNT_MAX samples, with its idle-frame counter; all zero when
// it went stale.  `entries` / `voxels_prev` are only read for the adjacent-level lookup.  `topups` (host build: may be non-null) counts
// the adjacent-level top-ups.
RT_HD Voxel resolve_voxel(uint64_t key, const Voxel &prev, const Voxel &curr, bool cam_moved, const GridParams &g, const uint64_t *entries,
                          uint32_t entries_count, const Voxel *voxels_prev, uint32_t *topups = nullptr) {
    Voxel d = {{prev.v[0] + curr.v[0], prev.v[1] + curr.v[1], prev.v[2] + curr.v[2], prev.v[3] + curr.v[3]}};
    uint32_t sample_count = d.v[3] & SAMPLE_COUNTER_BIT_MASK;
    if (cam_moved && sample_count < SAMPLE_COUNT_MIN && curr.v[3]) {
        const uint32_t e = hash_map_find(entries, entries_count, get_adjacent_level_hash(key, g));
        if (e != INVALID_ENTRY) {
            const Voxel adj = voxels_prev[e];
            const uint32_t adj_count = adj.v[3] & SAMPLE_COUNTER_BIT_MASK;
            if (adj_count > SAMPLE_COUNT_MIN) {
                const float k = float(SAMPLE_COUNT_MIN) / float(adj_count);
                d.v[0] += uint32_t(float(adj.v[0]) * k);
                d.v[1] += uint32_t(float(adj.v[1]) * k);
                d.v[2] += uint32_t(float(adj.v[2]) * k);
                sample_count += SAMPLE_COUNT_MIN;
                if (topups) {
                    ++*topups;
                }
            }
        }
    }
    if (sample_count > SAMPLE_COUNT_MAX) {
        const float k = float(SAMPLE_COUNT_MAX) / float(sample_count);
        d.v[0] = uint32_t(float(d.v[0]) * k);
        d.v[1] = uint32_t(float(d.v[1]) * k);
        d.v[2] = uint32_t(float(d.v[2]) * k);
        sample_count = SAMPLE_COUNT_MAX;
    }
    uint32_t frame_count = voxel_frames(prev);
    d.v[3] = sample_count;
    // (the reference tests this frame's word with the frame-counter mask: a voxel that got no sample ages by one frame)
    if ((curr.v[3] & FRAME_COUNTER_BIT_MASK) == 0) {
        ++frame_count;
        d.v[3] |= (frame_count & FRAME_COUNTER_BIT_MASK) << SAMPLE_COUNTER_BIT_NUM;
    }
    if (frame_count > STALE_FRAME_NUM_MAX) {
        d = Voxel{{0, 0, 0, 0}};
    }
    return d;
}

// The reference's own order (one portion, serial): bucket after bucket, every key resolved and compacted in place.  An
// adjacent-level lookup may then read a bucket that was already compacted -- the reference's parallel portions race on it
// (RendererCPU.h:1187).  Host build only: the device resolves every slot first and compacts after (cache_kernels.hip.h).
RT_HD void resolve_serial(const GridParams &g, uint64_t *entries, uint32_t entries_count, Voxel *voxels_curr, const Voxel *voxels_prev, uint32_t start,
                          uint32_t count, uint32_t *topups = nullptr) {
    const bool moved = camera_moved(g);
    for (uint32_t i = start; i < start + count; i += BUCKET_SIZE) {
        uint32_t ndx = i;
        for (uint32_t j = 0; j < BUCKET_SIZE; ++j) {
            const uint64_t key = entries[i + j];
            if (key == INVALID_KEY) {
                continue;
            }
            const Voxel d = resolve_voxel(key, voxels_prev[i + j], voxels_curr[i + j], moved, g, entries, entries_count, voxels_prev, topups);
            entries[i + j] = INVALID_KEY;
            voxels_curr[i + j] = Voxel{{0, 0, 0, 0}};
            if (d.v[3]) {
                entries[ndx] = key;
                voxels_curr[ndx++] = d;
            }
        }
    }
}

} // namespace cache
} // namespace rt
