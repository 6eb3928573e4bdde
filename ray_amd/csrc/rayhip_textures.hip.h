// rayhip_textures.hip.h -- part of librayhip's host side (one translation unit: included by rayhip.hip behind rayhip_environment.hip.h,
// whose preconditions and stamps it uses): a texture's texels changed ON THE DEVICE.  rayhip_scene_set_texture / _device take RGBA8 words
// for level 0 of a texture the scene holds -- copied as they are into an uncompressed storage; compressed into the blocks of the BC3
// (YCoCg), BC4 and BC5 storages, every held mip rebuilt, by the kernels of texture_update.hip.h -- and rayhip_scene_set_texture_blocks
// takes ready blocks for the whole chain of a block storage.  Every check runs on the host before the first write.
#pragma once

// ---- the texture a handle names -------------------------------------------------------------------------------------------------------
struct HeldTexture {
    uint32_t storage = 0;
    bool blocks = false; // its levels are 4 x 4 blocks (a block storage on a scene uploaded with RAYHIP_TEX_RAW_BC)
    int levels = 1;
    rayhip_texture t = {};
    uint64_t words = 0; // of all held levels
};

// 0, or 1: the handle names no texture of the scene, or the environment map, or its record leaves the pool.  (One record comes back from
// the texture table: the stream is idle.)
static int held_texture(rayhip_ctx *c, const char *who, const uint32_t handle, HeldTexture &m) {
    namespace tu = rayhip_texture_update;
    const uint32_t storage = handle >> 28, index = handle & 0x00ffffffu;
    const uint64_t entry = storage < 8u ? uint64_t(c->tex_table[storage]) + index : ~uint64_t(0);
    if (storage >= 8u || entry >= c->textures_count || (storage < 7u && entry >= c->tex_table[storage + 1u])) {
        return fail("%s: handle 0x%08x names no texture of the uploaded scene", who, handle);
    }
    const uint32_t env_map = c->sc.env.env_map;
    if (env_map != 0xffffffffu && ((env_map ^ handle) & 0xf0ffffffu) == 0u) {
        return fail("%s: handle 0x%08x is the environment map, which rayhip_scene_set_env_map changes (it rebuilds the quadtree)", who, handle);
    }
    HIP_TRY(hipMemcpy(&m.t, c->textures.as<rayhip_texture>() + entry, sizeof(m.t), hipMemcpyDeviceToHost));
    m.storage = storage;
    m.blocks = storage >= tu::STORAGE_BC1 && (c->tex_flags & RAYHIP_TEX_RAW_BC) != 0u;
    m.levels = tu::levels_held(m.t);
    m.words = 0;
    for (int l = 0; l < m.levels; ++l) {
        const uint64_t words = tu::level_words(storage, m.blocks, m.t.width[l], m.t.height[l]);
        if (m.t.width[l] == 0u || m.t.height[l] == 0u || m.t.width[l] > 16384u || m.t.height[l] > 16384u || uint64_t(m.t.offset[l]) + words > c->texels_count) {
            return fail("%s: level %d of the texture's record leaves the texel pool", who, l);
        }
        m.words += words;
    }
    return 0;
}

// ---- new texels ---------------------------------------------------------------------------------------------------------------------------
// (this file is included inside rayhip.hip's extern "C" block, where no template can be declared: the storage is chosen at each launch)
#define TEX_LAUNCH(kernel, grid, ...)                                                                                                      \
    if (m.storage == tu::STORAGE_BC3) {                                                                                                    \
        tu::kernel<tu::STORAGE_BC3><<<grid, tu::LANES, 0, s>>>(__VA_ARGS__);                                                              \
    } else if (m.storage == tu::STORAGE_BC4) {                                                                                             \
        tu::kernel<tu::STORAGE_BC4><<<grid, tu::LANES, 0, s>>>(__VA_ARGS__);                                                              \
    } else {                                                                                                                               \
        tu::kernel<tu::STORAGE_BC5><<<grid, tu::LANES, 0, s>>>(__VA_ARGS__);                                                              \
    }

static int compress_levels(rayhip_ctx *c, const VertexStamps &st, const HeldTexture &m, const uint32_t *d_src) {
    namespace tu = rayhip_texture_update;
    hipStream_t s = c->stream;
    uint32_t *pool = c->texels.as<uint32_t>();
    const auto grid = [](const uint32_t w, const uint32_t h) { return (tu::tiles(w) * tu::tiles(h) + tu::LANES - 1u) / tu::LANES; };
    TEX_LAUNCH(k_tex_compress, grid(m.t.width[0], m.t.height[0]), d_src, int(m.t.width[0]), int(m.t.height[0]), pool + m.t.offset[0])
    HIP_TRY(hipGetLastError());
    // level l is averaged from level l - 1: the caller's texels, then the staging halves in turn (odd levels in the first, even ones in
    // the second; level 1 and level 2 are the largest of each)
    uint32_t *half[2] = {c->texture_stage.as<uint32_t>(), c->texture_stage.as<uint32_t>() + (m.levels > 1 ? size_t(m.t.width[1]) * m.t.height[1] : 0)};
    const uint32_t *src = d_src;
    for (int l = 1; l < m.levels; ++l) {
        uint32_t *stage = l + 1 < m.levels ? half[(l - 1) & 1] : nullptr;
        TEX_LAUNCH(k_tex_mip_compress, grid(m.t.width[l], m.t.height[l]), src, int(m.t.width[l - 1]), int(m.t.width[l]), int(m.t.height[l]), stage, pool + m.t.offset[l])
        HIP_TRY(hipGetLastError());
        src = stage;
    }
    HIP_TRY(st.stamp("levels compressed"));
    return 0;
}
#undef TEX_LAUNCH

// `from_device`: rgba8 is memory of the context's device, 4-byte aligned, complete and stable until the call returns
static int set_texture(rayhip_ctx *c, const char *who, const uint32_t handle, const int w, const int h, const uint32_t *rgba8, const bool from_device) {
    namespace tu = rayhip_texture_update;
    if (!c || use_device(c)) {
        return 1;
    }
    if (const int rc = scene_change_possible(c, who, !rgba8, false)) {
        return rc;
    }
    const VertexStamps st{c, who};
    hipStream_t s = c->stream;
    HIP_TRY(hipStreamSynchronize(s)); // pending passes read the old texels
    HIP_TRY(st.stamp("begin"));
    HeldTexture m;
    if (held_texture(c, who, handle, m)) {
        return 1;
    }
    if (m.storage == tu::STORAGE_BC1 || (m.storage == tu::STORAGE_BC3 && (handle & rt::TEX_YCOCG_BIT) == 0u)) {
        (void)fail("%s: the reference compresses nothing into BC1 or plain BC3; such a texture takes ready blocks (rayhip_scene_set_texture_blocks)", who);
        return 2;
    }
    if (m.storage >= tu::STORAGE_BC1 && !m.blocks) {
        (void)fail("%s: the scene was uploaded with its block storages decoded (no RAYHIP_TEX_RAW_BC); their mips cannot be rebuilt from new texels", who);
        return 2;
    }
    if (m.blocks ? !tu::halving_chain(m.t, m.levels) : m.levels != 1) {
        (void)fail("%s: the texture's %d levels are not the chain the reference builds for its storage", who, m.levels);
        return 2;
    }
    if (w != int(m.t.width[0]) || h != int(m.t.height[0])) {
        return fail("%s: %d x %d texels for a texture of %u x %u; another size needs an upload", who, w, h, m.t.width[0], m.t.height[0]);
    }
    if (from_device && (reinterpret_cast<uintptr_t>(rgba8) & 3u) != 0u) {
        return fail("%s: the texels are not 4-byte aligned", who);
    }
    const size_t texels = size_t(w) * size_t(h);
    const hipMemcpyKind kind = from_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (!m.blocks) {
        // (everything is checked: from here on the texel pool is written)
        HIP_TRY(hipMemcpyAsync(c->texels.as<uint32_t>() + m.t.offset[0], rgba8, texels * sizeof(uint32_t), kind, s));
        HIP_TRY(hipStreamSynchronize(s)); // host texels may go away
        return 0;
    }
    // staging: host texels first (behind the two halves of the mips), then level 1 and level 2
    const size_t l1 = m.levels > 1 ? size_t(m.t.width[1]) * m.t.height[1] : 0, l2 = m.levels > 2 ? size_t(m.t.width[2]) * m.t.height[2] : 0;
    if (c->texture_stage.alloc((l1 + l2 + (from_device ? 0 : texels)) * sizeof(uint32_t))) {
        return 1;
    }
    const uint32_t *d_src = rgba8;
    if (!from_device) {
        uint32_t *up = c->texture_stage.as<uint32_t>() + l1 + l2;
        HIP_TRY(hipMemcpyAsync(up, rgba8, texels * sizeof(uint32_t), kind, s));
        d_src = up;
    }
    HIP_TRY(st.stamp("texels"));
    // (everything is checked: from here on the texel pool is written)
    if (compress_levels(c, st, m, d_src)) {
        return 1;
    }
    HIP_TRY(hipStreamSynchronize(s)); // the caller's texels may go away
    return 0;
}

int rayhip_scene_set_texture(rayhip_ctx *c, uint32_t handle, int w, int h, const uint32_t *rgba8) {
    return set_texture(c, "rayhip_scene_set_texture", handle, w, h, rgba8, false);
}

int rayhip_scene_set_texture_device(rayhip_ctx *c, uint32_t handle, int w, int h, const uint32_t *device_rgba8) {
    return set_texture(c, "rayhip_scene_set_texture_device", handle, w, h, device_rgba8, true);
}

// ---- ready blocks for the whole chain -------------------------------------------------------------------------------------------------------
int rayhip_scene_set_texture_blocks(rayhip_ctx *c, uint32_t handle, const void *blocks, size_t bytes) {
    namespace tu = rayhip_texture_update;
    const char *who = "rayhip_scene_set_texture_blocks";
    if (!c || use_device(c)) {
        return 1;
    }
    if (const int rc = scene_change_possible(c, who, !blocks, false)) {
        return rc;
    }
    hipStream_t s = c->stream;
    HIP_TRY(hipStreamSynchronize(s)); // pending passes read the old blocks
    HeldTexture m;
    if (held_texture(c, who, handle, m)) {
        return 1;
    }
    if (m.storage < tu::STORAGE_BC1) {
        return fail("%s: storage %u holds texels, not blocks (rayhip_scene_set_texture)", who, m.storage);
    }
    if (!m.blocks) {
        (void)fail("%s: the scene was uploaded with its block storages decoded (no RAYHIP_TEX_RAW_BC)", who);
        return 2;
    }
    if (bytes != m.words * sizeof(uint32_t)) {
        return fail("%s: %zu bytes for a texture that holds %llu in %d levels", who, bytes, static_cast<unsigned long long>(m.words * sizeof(uint32_t)), m.levels);
    }
    // (everything is checked: from here on the texel pool is written; the levels of a texture need not be adjacent in the pool)
    const uint8_t *src = static_cast<const uint8_t *>(blocks);
    for (int l = 0; l < m.levels; ++l) {
        const size_t n = size_t(tu::level_words(m.storage, true, m.t.width[l], m.t.height[l])) * sizeof(uint32_t);
        HIP_TRY(hipMemcpyAsync(c->texels.as<uint32_t>() + m.t.offset[l], src, n, hipMemcpyHostToDevice, s));
        src += n;
    }
    HIP_TRY(hipStreamSynchronize(s)); // the caller's blocks may go away
    return 0;
}
