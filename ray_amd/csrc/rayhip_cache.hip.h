// rayhip_cache.hip.h -- part of librayhip's host side (included by rayhip.hip after the other parts): the spatial radiance cache's
// entry points (include/rayhip.h, rayhip_cache_* and the hooks rayhip_k_cache_*), over the kernels of cache_kernels.hip.h.
#pragma once

namespace {

constexpr size_t CACHE_KEY_BYTES = size_t(cache::ENTRIES_COUNT) * sizeof(uint64_t);    // 32 MiB
constexpr size_t CACHE_VOXEL_BYTES = size_t(cache::ENTRIES_COUNT) * sizeof(cache::Voxel); // 64 MiB
constexpr size_t CACHE_PATH_WORDS = size_t(cache::PROPAGATION_DEPTH) * 4 + 1;          // entries, weights, length: 68 B per path

int cache_ready(rayhip_ctx *c) {
    if (use_device(c)) {
        return 1;
    }
    if (!c->cache_on) {
        return fail("the spatial cache is not enabled (rayhip_cache_enable)");
    }
    return 0;
}

cache::PathPlanes cache_path_planes(rayhip_ctx *c) {
    const uint32_t n = c->cache_path_count;
    uint32_t *base = c->cache_paths.as<uint32_t>();
    return cache::PathPlanes{base, reinterpret_cast<float *>(base + size_t(cache::PROPAGATION_DEPTH) * n),
                             reinterpret_cast<int32_t *>(base + size_t(cache::PROPAGATION_DEPTH) * 4 * n), n};
}

// runs `launch` on the context stream and waits for it; its GPU time (HIP events) is added to stage `stage` of
// rayhip_get_stage_times (9: time_cache_update_us, 10: time_cache_resolve_us), none when stage < 0
template <typename F> int cache_timed(rayhip_ctx *c, int stage, F &&launch) {
    float ms_ = 0.0f;
    float *out_ms = stage >= 0 ? &ms_ : nullptr;
    hipEvent_t e[2] = {nullptr, nullptr};
    if (out_ms) {
        HIP_TRY(hipEventCreate(&e[0]));
        if (hipEventCreate(&e[1]) != hipSuccess) {
            (void)hipEventDestroy(e[0]);
            return fail("hipEventCreate failed");
        }
        (void)hipEventRecord(e[0], c->stream);
    }
    const int rc = launch();
    const hipError_t le = hipGetLastError();
    if (out_ms) {
        (void)hipEventRecord(e[1], c->stream);
    }
    const hipError_t se = hipStreamSynchronize(c->stream);
    if (out_ms) {
        float ms = 0.0f;
        if (rc == 0 && le == hipSuccess && se == hipSuccess) {
            (void)hipEventElapsedTime(&ms, e[0], e[1]);
        }
        *out_ms = ms;
        (void)hipEventDestroy(e[0]);
        (void)hipEventDestroy(e[1]);
        c->stage_us[stage] += double(ms) * 1000.0;
    }
    if (rc) {
        return rc;
    }
    if (le != hipSuccess || se != hipSuccess) {
        return fail("spatial cache kernel failed: %s", hipGetErrorString(le != hipSuccess ? le : se));
    }
    return 0;
}

} // namespace

int rayhip_cache_enable(rayhip_ctx *c, int on) {
    if (use_device(c)) {
        return 1;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (!on) {
        for (DevBuf *b : {&c->cache_entries, &c->cache_voxels[0], &c->cache_voxels[1], &c->cache_paths, &c->cache_io}) {
            b->release();
        }
        c->cache_on = false;
        c->cache_path_count = 0;
        return 0;
    }
    if (c->cache_on) {
        return 0;
    }
    // (DevBuf::alloc zero-fills: an empty table, empty voxels)
    if (c->cache_entries.alloc(CACHE_KEY_BYTES) || c->cache_voxels[0].alloc(CACHE_VOXEL_BYTES) || c->cache_voxels[1].alloc(CACHE_VOXEL_BYTES)) {
        for (DevBuf *b : {&c->cache_entries, &c->cache_voxels[0], &c->cache_voxels[1]}) {
            b->release();
        }
        return 1;
    }
    c->cache_prev = 0;
    c->cache_cam_prev[0] = c->cache_cam_prev[1] = c->cache_cam_prev[2] = 0.0f;
    c->cache_on = true;
    return 0;
}

int rayhip_k_cache_begin_paths(rayhip_ctx *c, int paths) {
    if (cache_ready(c)) {
        return 1;
    }
    if (paths <= 0) {
        return fail("rayhip_k_cache_begin_paths: bad path count %d", paths);
    }
    const size_t bytes = CACHE_PATH_WORDS * 4 * size_t(paths);
    if (c->cache_paths.alloc(bytes)) {
        return 1;
    }
    c->cache_path_count = uint32_t(paths);
    // rect_fill(cache_data_t{}) of RendererCPU.h:1103: all zero
    HIP_TRY(hipMemsetAsync(c->cache_paths.p, 0, bytes, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int rayhip_k_cache_update_vertices(rayhip_ctx *c, const rayhip_cache_grid *grid, const rayhip_cache_vertex *verts, int count) {
    if (cache_ready(c)) {
        return 1;
    }
    if (!grid || count < 0 || (count && !verts)) {
        return fail("rayhip_k_cache_update_vertices: bad arguments");
    }
    if (!c->cache_path_count) {
        return fail("rayhip_k_cache_update_vertices before rayhip_k_cache_begin_paths");
    }
    // one lane per vertex updates its path's state without atomics: two vertices of one path in a call would race
    std::vector<uint8_t> seen(c->cache_path_count, 0);
    for (int i = 0; i < count; ++i) {
        if (verts[i].path >= c->cache_path_count) {
            return fail("rayhip_k_cache_update_vertices: vertex %d names path %u of %u", i, verts[i].path, c->cache_path_count);
        }
        if (seen[verts[i].path]++) {
            return fail("rayhip_k_cache_update_vertices: vertex %d names path %u a second time (one vertex per path and call)", i, verts[i].path);
        }
    }
    if (count == 0) {
        return 0;
    }
    if (upload(c, c->cache_io, verts, size_t(count) * sizeof(rayhip_cache_vertex))) {
        return 1;
    }
    cache::GridParams g;
    memcpy(&g, grid, sizeof(g));
    cache::Voxel *curr = c->cache_voxels[c->cache_prev ^ 1].as<cache::Voxel>();
    return cache_timed(c, 9, [&]() {
        cache::k_cache_update<<<grid_for(c, size_t(count), 256), 256, 0, c->stream>>>(c->cache_io.as<rayhip_cache_vertex>(), uint32_t(count),
                                                                                      cache_path_planes(c), g, c->cache_entries.as<uint64_t>(), curr);
        return 0;
    });
}

int rayhip_cache_resolve(rayhip_ctx *c, const rayhip_camera *cam) {
    if (cache_ready(c)) {
        return 1;
    }
    if (!cam) {
        return fail("rayhip_cache_resolve: no camera");
    }
    const float *cam_pos = cam->origin;
    cache::GridParams g = {};
    memcpy(g.cam_pos_curr, cam_pos, sizeof(g.cam_pos_curr));
    memcpy(g.cam_pos_prev, c->cache_cam_prev, sizeof(g.cam_pos_prev));
    g.log_base = cache::LOGARITHM_BASE, g.scale = cache::GRID_SCALE, g.exposure = 1.0f;
    const int moved = cache::camera_moved(g) ? 1 : 0;
    uint64_t *entries = c->cache_entries.as<uint64_t>();
    cache::Voxel *prev = c->cache_voxels[c->cache_prev].as<cache::Voxel>(), *curr = c->cache_voxels[c->cache_prev ^ 1].as<cache::Voxel>();
    const int grid = int(cache::ENTRIES_COUNT / 256);
    const int rc = cache_timed(c, 10, [&]() {
        cache::k_cache_resolve_slots<<<grid, 256, 0, c->stream>>>(g, moved, entries, curr, prev);
        cache::k_cache_compact<<<grid, 256, 0, c->stream>>>(entries, curr);
        return 0;
    });
    if (rc) {
        return rc;
    }
    // the resolved voxels become the previous frames'; the old previous array is this frame's, cleared
    c->cache_prev ^= 1;
    HIP_TRY(hipMemsetAsync(c->cache_voxels[c->cache_prev ^ 1].p, 0, CACHE_VOXEL_BYTES, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    memcpy(c->cache_cam_prev, cam_pos, sizeof(c->cache_cam_prev));
    return 0;
}

int rayhip_cache_reset(rayhip_ctx *c) {
    if (cache_ready(c)) {
        return 1;
    }
    HIP_TRY(hipMemsetAsync(c->cache_voxels[c->cache_prev].p, 0, CACHE_VOXEL_BYTES, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int rayhip_cache_readback(rayhip_ctx *c, uint64_t *keys, uint32_t *voxels, int which, uint32_t count) {
    if (cache_ready(c)) {
        return 1;
    }
    if (count > cache::ENTRIES_COUNT || (which != 0 && which != 1)) {
        return fail("rayhip_cache_readback: bad arguments (count %u, which %d)", count, which);
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (keys && count) {
        HIP_TRY(hipMemcpy(keys, c->cache_entries.p, size_t(count) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    }
    if (voxels && count) {
        HIP_TRY(hipMemcpy(voxels, c->cache_voxels[which == 0 ? c->cache_prev : (c->cache_prev ^ 1)].p, size_t(count) * sizeof(cache::Voxel),
                          hipMemcpyDeviceToHost));
    }
    return 0;
}

int rayhip_k_cache_query(rayhip_ctx *c, const rayhip_cache_grid *grid, const float *points, int count, float *out) {
    if (cache_ready(c)) {
        return 1;
    }
    if (!grid || count < 0 || (count && (!points || !out))) {
        return fail("rayhip_k_cache_query: bad arguments");
    }
    if (count == 0) {
        return 0;
    }
    const size_t in_bytes = size_t(count) * 6 * sizeof(float), out_off = (in_bytes + 255) & ~size_t(255);
    if (c->cache_io.alloc(out_off + size_t(count) * sizeof(float4))) {
        return 1;
    }
    HIP_TRY(hipMemcpyAsync(c->cache_io.p, points, in_bytes, hipMemcpyHostToDevice, c->stream));
    cache::GridParams g;
    memcpy(&g, grid, sizeof(g));
    float4 *dev_out = reinterpret_cast<float4 *>(static_cast<char *>(c->cache_io.p) + out_off);
    const int rc = cache_timed(c, -1, [&]() {
        cache::k_cache_query<<<grid_for(c, size_t(count), 256), 256, 0, c->stream>>>(c->cache_io.as<float>(), uint32_t(count), g,
                                                                                     c->cache_entries.as<uint64_t>(),
                                                                                     c->cache_voxels[c->cache_prev].as<cache::Voxel>(), dev_out);
        return 0;
    });
    if (rc) {
        return rc;
    }
    HIP_TRY(hipMemcpy(out, dev_out, size_t(count) * sizeof(float4), hipMemcpyDeviceToHost));
    return 0;
}
