// rayhip_environment.hip.h -- part of librayhip's host side (one translation unit: included by rayhip.hip behind rayhip_deform.hip.h,
// whose preconditions, stamps and light refit it uses): the environment changed ON THE DEVICE.  rayhip_scene_set_environment (colours
// and rotations), rayhip_scene_set_env_map / _device (new texels for the map the scene holds) and rayhip_scene_set_sky (the suns and
// the atmosphere of a physical sky, the map re-baked in place by k_bake_sky).  The calls that change texels end with the common tail:
// the map's importance quadtree rebuilt by the kernels of env_qtree.hip.h, the environment light's flux put into its leaf summary,
// the light tree refitted by the level launches of the vertex update, the scene view pointed at the new pyramid.
#pragma once

// ---- the environment map the scene holds ----------------------------------------------------------------------------------------------
struct HeldEnvMap {
    int w = 0, h = 0;
    uint32_t *texels = nullptr; // level 0, in the texel pool
};

// 0, or 2: the scene has no environment map to write into.  (One record comes back from the texture table: the stream is idle.)
static int held_env_map(rayhip_ctx *c, const char *who, HeldEnvMap &m) {
    const uint32_t handle = c->sc.env.env_map;
    const uint64_t index = uint64_t(c->tex_table[0]) + (handle & 0x00ffffffu);
    if (handle == 0xffffffffu || (handle >> 28) != 0u || index >= c->textures_count) {
        (void)fail("%s: the uploaded scene has no environment map", who);
        return 2;
    }
    rayhip_texture t;
    HIP_TRY(hipMemcpy(&t, c->textures.as<rayhip_texture>() + index, sizeof(t), hipMemcpyDeviceToHost));
    if (t.width[0] == 0 || t.height[0] == 0 || t.width[0] > 16384u || t.height[0] > 16384u ||
        (uint64_t(t.offset[0]) + uint64_t(t.width[0]) * t.height[0]) * sizeof(uint32_t) > c->texels.bytes) {
        return fail("%s: the environment map's record leaves the texel pool", who);
    }
    m.w = int(t.width[0]), m.h = int(t.height[0]);
    m.texels = c->texels.as<uint32_t>() + t.offset[0];
    return 0;
}

static bool has_env_light(const rayhip_ctx *c) { return c->sc.env.light_index != 0xffffffffu; }

// ---- the common tail: what a call that changes the map's texels needs, asked BEFORE it writes, and what it ends with -----------------
// 0 = go on (the buffers of the build are allocated), 1 / 2 = the return code
static int env_tail_possible(rayhip_ctx *c, const char *who, const HeldEnvMap &m) {
    namespace eq = rayhip_env_qtree;
    if (!has_env_light(c)) {
        return 0;
    }
    const rayhip_ctx::LightRefit &lr = c->light_refit;
    if (!lr.on || !lr.ready) {
        (void)fail("%s: the scene has an environment light, and rayhip_scene_refit_lights is off or its tables are not prepared", who);
        return 2;
    }
    if (c->sc.env.light_index >= lr.lights_count) {
        return fail("%s: the environment light's slot %u is outside the %u light slots", who, c->sc.env.light_index, lr.lights_count);
    }
    const int res = eq::finest_res(m.w, m.h), n_levels = eq::full_levels(res);
    if (n_levels < 1 || n_levels > eq::MAX_LEVELS) {
        (void)fail("%s: a %d x %d map has no quadtree", who, m.w, m.h);
        return 2;
    }
    rayhip_ctx::EnvBuild &eb = c->env_build;
    const int half = c->sc.env_qtree == eb.pyramid[0].as<float4>() ? 1 : 0;
    return eb.pyramid[half].alloc(size_t(eq::level_offset(res, n_levels)) * sizeof(float4)) || eb.block.alloc(sizeof(eq::Block)) ||
                   c->light_counters.alloc(8 * sizeof(uint32_t))
               ? 1
               : 0;
}

// The quadtree of the texels that are on the device now, built into the half of the double buffer the scene view does not point at:
// the finest level (one tile of cells per workgroup, taps through LDS), one launch per upper mip while it is large and ONE workgroup
// for the rest, the flag pass; then the environment light's leaf and the level launches of the light refit; one read-back (16 flags,
// two floats), from which the host derives the levels kept and their offsets.  The view changes last.  Without an environment light
// the texels are all that changed.
static int env_tail(rayhip_ctx *c, const VertexStamps &st, const HeldEnvMap &m) {
    namespace eq = rayhip_env_qtree;
    hipStream_t s = c->stream;
    if (!has_env_light(c)) {
        HIP_TRY(hipStreamSynchronize(s));
        return 0;
    }
    rayhip_ctx::EnvBuild &eb = c->env_build;
    rayhip_ctx::LightRefit &lr = c->light_refit;
    const int res = eq::finest_res(m.w, m.h), n_levels = eq::full_levels(res);
    const int half = c->sc.env_qtree == eb.pyramid[0].as<float4>() ? 1 : 0;
    float4 *pyramid = eb.pyramid[half].as<float4>();
    eq::Block *d_block = eb.block.as<eq::Block>();
    HIP_TRY(hipMemsetAsync(d_block, 0, sizeof(eq::Block), s));
    const unsigned tiles = unsigned((res + eq::TILE - 1) / eq::TILE);
    eq::k_env_qtree_finest<<<dim3(tiles, tiles), eq::TILE * eq::TILE, 0, s>>>(m.texels, m.w, m.h, res, pyramid);
    HIP_TRY(hipGetLastError());
    HIP_TRY(st.stamp("finest level"));
    int l = 1;
    for (; l < n_levels && eq::quads_per_side(res, l) > eq::TOP_QUADS; ++l) {
        const uint32_t n = eq::quads_per_side(res, l);
        eq::k_env_qtree_level<<<blocks_of(size_t(n) * n), 256, 0, s>>>(pyramid + eq::level_offset(res, l - 1), pyramid + eq::level_offset(res, l), n);
        HIP_TRY(hipGetLastError());
    }
    if (l < n_levels) {
        eq::k_env_qtree_top<<<1, 256, 0, s>>>(pyramid, res, l, n_levels);
        HIP_TRY(hipGetLastError());
    }
    const uint32_t n0 = eq::quads_per_side(res, 0);
    eq::k_env_qtree_flags<<<dim3(std::min(64u, blocks_of(size_t(n0) * n0)), unsigned(n_levels)), 256, 0, s>>>(pyramid, res, n_levels, d_block);
    HIP_TRY(hipGetLastError());
    HIP_TRY(st.stamp("pyramid and flags"));
    eq::k_env_light_leaf<<<1, 64, 0, s>>>(d_block, c->sc.env.light_index, lr.leaf.as<rayhip_light_refit::Summary>(), lr.posed.as<uint8_t>());
    HIP_TRY(hipGetLastError());
    // (the level launches read the summary of EVERY leaf: where no pass over the triangle lights ran yet it runs here, as in set_lights)
    uint32_t *d_counters = c->light_counters.as<uint32_t>();
    if (!lr.tri_leaves) {
        HIP_TRY(hipMemsetAsync(d_counters, 0, 8 * sizeof(uint32_t), s));
        if (refit_lights(c, d_counters + rayhip_light_pose::N_FINDINGS, st)) {
            return 1;
        }
        HIP_TRY(hipMemcpyAsync(&lr.degenerate, d_counters + rayhip_light_pose::N_FINDINGS, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    } else if (refit_light_levels(c)) {
        return 1;
    }
    eq::Block block;
    HIP_TRY(hipMemcpyAsync(&block, d_block, sizeof(block), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(st.stamp("light tree refitted"));
    // (everything is on the device: from here on the scene view is written)
    const int kept = eq::levels_kept(block.flag, n_levels);
    SceneView &v = c->sc;
    v.env_qtree = pyramid;
    v.env.qtree_levels = kept;
    for (int lod = 0; lod < 16; ++lod) {
        v.env_qtree_offset[lod] = eq::level_offset(res, lod < kept ? n_levels - kept + lod : n_levels);
    }
    eb.total_lum = block.total_lum, eb.medium_lum = block.medium_lum;
    return 0;
}

// ---- colours and rotations ------------------------------------------------------------------------------------------------------------
static bool colour_ok(const float *col) {
    return std::isfinite(col[0]) && std::isfinite(col[1]) && std::isfinite(col[2]) && col[0] >= 0.0f && col[1] >= 0.0f && col[2] >= 0.0f;
}
static bool all_positive(const float *col) { return col[0] > 0.0f && col[1] > 0.0f && col[2] > 0.0f; }

int rayhip_scene_set_environment(rayhip_ctx *c, const float env_col[3], const float back_col[3], float env_map_rotation, float back_map_rotation) {
    const char *who = "rayhip_scene_set_environment";
    if (!c || use_device(c)) {
        return 1;
    }
    if (const int rc = scene_change_possible(c, who, !env_col || !back_col, false)) {
        return rc;
    }
    if (!colour_ok(env_col) || !colour_ok(back_col)) {
        return fail("%s: a colour component is negative or not finite", who);
    }
    if (!std::isfinite(env_map_rotation) || !std::isfinite(back_map_rotation)) {
        return fail("%s: a rotation is not finite", who);
    }
    if (all_positive(env_col) != all_positive(c->sc.env.env_col)) {
        return fail("%s: env_col would change whether every component is positive, the condition under which a scene has its environment light", who);
    }
    HIP_TRY(hipStreamSynchronize(c->stream)); // pending passes were launched with the old view
    rayhip_environment &e = c->sc.env;
    memcpy(e.env_col, env_col, 12), memcpy(e.back_col, back_col, 12);
    e.env_map_rotation = env_map_rotation, e.back_map_rotation = back_map_rotation;
    return 0;
}

// ---- new texels for the map ---------------------------------------------------------------------------------------------------------------
// `from_device`: rgbe8 is memory of the context's device, 4-byte aligned, complete and stable until the call returns
static int set_env_map(rayhip_ctx *c, const char *who, const int w, const int h, const uint32_t *rgbe8, const bool from_device) {
    if (!c || use_device(c)) {
        return 1;
    }
    if (const int rc = scene_change_possible(c, who, !rgbe8, false)) {
        return rc;
    }
    const VertexStamps st{c, who};
    HIP_TRY(hipStreamSynchronize(c->stream)); // pending passes read the old texels
    HIP_TRY(st.stamp("begin"));
    HeldEnvMap m;
    if (const int rc = held_env_map(c, who, m)) {
        return rc;
    }
    if (w != m.w || h != m.h) {
        return fail("%s: %d x %d texels for a map of %d x %d; a map of another size needs an upload", who, w, h, m.w, m.h);
    }
    if (from_device && (reinterpret_cast<uintptr_t>(rgbe8) & 3u) != 0u) {
        return fail("%s: the texels are not 4-byte aligned", who);
    }
    if (const int rc = env_tail_possible(c, who, m)) {
        return rc;
    }
    // (everything is checked: from here on the texel pool is written)
    HIP_TRY(hipMemcpyAsync(m.texels, rgbe8, size_t(w) * size_t(h) * sizeof(uint32_t), from_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    HIP_TRY(st.stamp("texels"));
    return env_tail(c, st, m); // (it waits for the stream: host texels may go away then)
}

int rayhip_scene_set_env_map(rayhip_ctx *c, int w, int h, const uint32_t *rgbe8) { return set_env_map(c, "rayhip_scene_set_env_map", w, h, rgbe8, false); }

int rayhip_scene_set_env_map_device(rayhip_ctx *c, int w, int h, const uint32_t *device_rgbe8) {
    return set_env_map(c, "rayhip_scene_set_env_map_device", w, h, device_rgbe8, true);
}

// ---- the physical sky: suns and atmosphere ------------------------------------------------------------------------------------------------
static bool floats_finite(const float *f, const size_t n) {
    for (size_t i = 0; i < n; ++i) {
        if (!std::isfinite(f[i])) {
            return false;
        }
    }
    return true;
}

// The checks run on the host against what comes back from the device: the list of the suns' slots, the records those slots hold and
// the held rayhip_sky (a few hundred bytes; the stream is idle).  Then records, sky and tables go to their places, k_bake_sky writes the
// map's texels where they lie in the texel pool -- the scene's own sky view and light array are its arguments --, and the common tail runs.
int rayhip_scene_set_sky(rayhip_ctx *c, uint32_t n, const uint32_t *slots, const rayhip_light *records, const rayhip_sky *sky, const float *transmittance_lut,
                         const float *multiscatter_lut) {
    const char *who = "rayhip_scene_set_sky";
    if (!c || use_device(c)) {
        return 1;
    }
    const int tables = int(sky != nullptr) + int(transmittance_lut != nullptr) + int(multiscatter_lut != nullptr);
    if (const int rc = scene_change_possible(c, who, (n > 0 && (!slots || !records)) || (tables != 0 && tables != 3), false)) {
        return rc;
    }
    if (!c->sky_view.desc || !(c->sc.env.sky_map_spread_angle > 0.0f)) {
        (void)fail("%s: the uploaded scene has no physical sky", who);
        return 2;
    }
    const VertexStamps st{c, who};
    hipStream_t s = c->stream;
    HIP_TRY(hipStreamSynchronize(s)); // pending passes read the old sky
    HIP_TRY(st.stamp("begin"));
    HeldEnvMap m;
    if (const int rc = held_env_map(c, who, m)) {
        return rc;
    }
    if (const int rc = env_tail_possible(c, who, m)) {
        return rc;
    }
    if (n == 0 && !sky) {
        return 0;
    }
    const uint32_t n_lights = uint32_t(c->lights.bytes / sizeof(rayhip_light)) < c->light_refit.lights_count ? uint32_t(c->lights.bytes / sizeof(rayhip_light))
                                                                                                           : c->light_refit.lights_count;
    std::vector<uint32_t> suns(c->sky_view.dir_lights_count);
    if (!suns.empty()) {
        HIP_TRY(hipMemcpy(suns.data(), c->sky_view.dir_lights, suns.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    for (uint32_t i = 0; i < n; ++i) {
        if (slots[i] >= n_lights || std::find(suns.begin(), suns.end(), slots[i]) == suns.end()) {
            return fail("%s: slot %u is none of the %zu directional lights of the sky", who, slots[i], suns.size());
        }
        if (std::find(slots, slots + i, slots[i]) != slots + i) {
            return fail("%s: slot %u is named more than once", who, slots[i]);
        }
        rayhip_light held;
        HIP_TRY(hipMemcpy(&held, c->lights.as<rayhip_light>() + slots[i], sizeof(held), hipMemcpyDeviceToHost));
        if (held.flags != records[i].flags) {
            return fail("%s: word 0 of the record for slot %u (type and flags) differs from the one the slot holds", who, slots[i]);
        }
        if (!floats_finite(records[i].col, 15)) {
            return fail("%s: the record for slot %u has a colour or a parameter that is not finite", who, slots[i]);
        }
    }
    if (sky) {
        rayhip_sky held;
        HIP_TRY(hipMemcpy(&held, c->sky_desc.p, sizeof(held), hipMemcpyDeviceToHost));
        if (memcmp(&held.transmittance_lut_w, &sky->transmittance_lut_w, 9 * sizeof(int32_t)) != 0) {
            return fail("%s: the sizes of the sky's tables and textures differ from the held ones", who);
        }
        const float *a = &sky->atmosphere.planet_radius;
        const size_t tl = size_t(sky->transmittance_lut_w) * size_t(sky->transmittance_lut_h) * 4, ml = size_t(sky->multiscatter_lut_res) * size_t(sky->multiscatter_lut_res) * 4;
        if (!floats_finite(a, 21) || !floats_finite(sky->atmosphere.moon_dir, 28) || !floats_finite(transmittance_lut, tl) || !floats_finite(multiscatter_lut, ml)) {
            return fail("%s: the atmosphere or one of its tables has a float that is not finite", who);
        }
        if (tl * sizeof(float) > c->sky_transmittance_lut.bytes || ml * sizeof(float) > c->sky_multiscatter_lut.bytes) {
            return fail("%s: the tables do not fit the held ones", who);
        }
        // (everything is checked: from here on the device is written)
        HIP_TRY(hipMemcpyAsync(c->sky_desc.p, sky, sizeof(rayhip_sky), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(c->sky_transmittance_lut.p, transmittance_lut, tl * sizeof(float), hipMemcpyHostToDevice, s));
        if (ml) {
            HIP_TRY(hipMemcpyAsync(c->sky_multiscatter_lut.p, multiscatter_lut, ml * sizeof(float), hipMemcpyHostToDevice, s));
        }
    }
    for (uint32_t i = 0; i < n; ++i) {
        HIP_TRY(hipMemcpyAsync(c->lights.as<rayhip_light>() + slots[i], &records[i], sizeof(rayhip_light), hipMemcpyHostToDevice, s));
    }
    HIP_TRY(st.stamp("records and sky committed"));
    const size_t texels = size_t(m.w) * size_t(m.h);
    k_bake_sky<<<unsigned((texels + 63) / 64), 64, 0, s>>>(c->sky_view, c->lights.as<rayhip_light>(), m.w, m.h, m.texels);
    HIP_TRY(hipGetLastError());
    HIP_TRY(st.stamp("sky baked"));
    return env_tail(c, st, m); // (it waits for the stream: the caller's arrays may go away then)
}
