// hostsim_texture.cpp -- TEST INFRASTRUCTURE.  New texels for a texture of the pool as the device turns them into blocks and mips
// (ray_amd/csrc/texture_update.h: the block emitters of the BC3-YCoCg, BC4 and BC5 storages, the clamped gather, the mip average),
// compiled with g++ (the HOSTSIM_FLAGS of hostsim.cpp) as plain loops over a pool, with the prefix hostsim_ and without a context.
// tests/test_texture_hostsim.py holds these against the pools the reference built; tests/test_gpu_texture_update.py holds the device
// (texture_update.hip.h) against this file.
//
// Never linked into librayhip.so, and links nothing of the reference.
#include <string.h>

#include <vector>

#include "../../include/rayhip.h"
#include "../../ray_amd/csrc/texture_update.h"

#define HS_API extern "C" __attribute__((visibility("default")))

namespace tu = rayhip_texture_update;

template <uint32_t storage> static void compress_chain(uint32_t *pool, const rayhip_texture &t, const int levels, const uint32_t *texels) {
    std::vector<uint32_t> above, stage;
    const uint32_t *src = texels;
    for (int l = 0; l < levels; ++l) {
        const int w = int(t.width[l]), h = int(t.height[l]), tx = int(tu::tiles(t.width[l])), ty = int(tu::tiles(t.height[l]));
        stage.assign(size_t(w) * size_t(h), 0u);
        for (int by = 0; by < ty; ++by) {
            for (int bx = 0; bx < tx; ++bx) {
                uint32_t rgba[16];
                if (l == 0) {
                    tu::gather_block(src, w, h, bx, by, rgba);
                } else {
                    tu::gather_mip_block(src, int(t.width[l - 1]), w, h, bx, by, stage.data(), rgba);
                }
                tu::emit_block<storage>(rgba, pool + t.offset[l] + (size_t(by) * size_t(tx) + size_t(bx)) * tu::block_words(storage));
            }
        }
        if (l > 0) {
            above.swap(stage);
            src = above.data();
        }
    }
}

// rayhip_scene_set_texture over host arrays: pool (pool_words), the records, tex_table[8], texture_flags; returns its codes (without the
// environment-map and null-pointer checks, which need a context)
HS_API int hostsim_set_texture(uint32_t *pool, uint32_t pool_words, const rayhip_texture *records, uint32_t n_records, const uint32_t *tex_table, uint32_t flags,
                               uint32_t handle, int w, int h, const uint32_t *texels) {
    const uint32_t storage = handle >> 28, index = handle & 0x00ffffffu;
    if (storage >= 8u || uint64_t(tex_table[storage]) + index >= n_records || (storage < 7u && tex_table[storage] + index >= tex_table[storage + 1u])) {
        return 1;
    }
    const rayhip_texture &t = records[tex_table[storage] + index];
    const bool blocks = storage >= tu::STORAGE_BC1 && (flags & RAYHIP_TEX_RAW_BC) != 0u;
    const int levels = tu::levels_held(t);
    for (int l = 0; l < levels; ++l) {
        if (uint64_t(t.offset[l]) + tu::level_words(storage, blocks, t.width[l], t.height[l]) > pool_words) {
            return 1;
        }
    }
    if (storage == tu::STORAGE_BC1 || (storage == tu::STORAGE_BC3 && (handle & rt::TEX_YCOCG_BIT) == 0u) || (storage >= tu::STORAGE_BC1 && !blocks) ||
        (blocks ? !tu::halving_chain(t, levels) : levels != 1)) {
        return 2;
    }
    if (w != int(t.width[0]) || h != int(t.height[0])) {
        return 1;
    }
    if (!blocks) {
        memcpy(pool + t.offset[0], texels, size_t(w) * size_t(h) * sizeof(uint32_t));
    } else if (storage == tu::STORAGE_BC3) {
        compress_chain<tu::STORAGE_BC3>(pool, t, levels, texels);
    } else if (storage == tu::STORAGE_BC4) {
        compress_chain<tu::STORAGE_BC4>(pool, t, levels, texels);
    } else {
        compress_chain<tu::STORAGE_BC5>(pool, t, levels, texels);
    }
    return 0;
}

// rayhip_scene_set_texture_blocks over host arrays
HS_API int hostsim_set_texture_blocks(uint32_t *pool, uint32_t pool_words, const rayhip_texture *records, uint32_t n_records, const uint32_t *tex_table, uint32_t flags,
                                      uint32_t handle, const void *blocks, size_t bytes) {
    const uint32_t storage = handle >> 28, index = handle & 0x00ffffffu;
    if (storage >= 8u || storage < tu::STORAGE_BC1 || uint64_t(tex_table[storage]) + index >= n_records ||
        (storage < 7u && tex_table[storage] + index >= tex_table[storage + 1u])) {
        return 1;
    }
    if ((flags & RAYHIP_TEX_RAW_BC) == 0u) {
        return 2;
    }
    const rayhip_texture &t = records[tex_table[storage] + index];
    const int levels = tu::levels_held(t);
    uint64_t words = 0;
    for (int l = 0; l < levels; ++l) {
        const uint64_t n = tu::level_words(storage, true, t.width[l], t.height[l]);
        if (uint64_t(t.offset[l]) + n > pool_words) {
            return 1;
        }
        words += n;
    }
    if (bytes != words * sizeof(uint32_t)) {
        return 1;
    }
    const uint8_t *src = static_cast<const uint8_t *>(blocks);
    for (int l = 0; l < levels; ++l) {
        const size_t n = size_t(tu::level_words(storage, true, t.width[l], t.height[l])) * sizeof(uint32_t);
        memcpy(pool + t.offset[l], src, n);
        src += n;
    }
    return 0;
}

// one block of a storage (5, 6 or 7) over sixteen RGBA8 texels: the named cases of the tests
HS_API int hostsim_texture_block(uint32_t storage, const uint32_t *rgba, uint32_t *out) {
    if (storage == tu::STORAGE_BC3) {
        tu::emit_block<tu::STORAGE_BC3>(rgba, out);
    } else if (storage == tu::STORAGE_BC4) {
        tu::emit_block<tu::STORAGE_BC4>(rgba, out);
    } else if (storage == tu::STORAGE_BC5) {
        tu::emit_block<tu::STORAGE_BC5>(rgba, out);
    } else {
        return 1;
    }
    return 0;
}
