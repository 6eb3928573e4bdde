// rayhip_hooks.hip.h -- part of librayhip's host side (one translation unit: included by rayhip.hip, in this order, after the kernels):
// kernel-level test hooks (rayhip_k_*): single stages on caller-supplied rays, for the parity tests.
#pragma once

// ---- kernel-level hooks ---------------------------------------------------------------------------------------

int rayhip_k_generate_primary_rays(rayhip_ctx *c, const rayhip_camera *cam, const int rect[4], int iteration,
                                   rayhip_ray *out_rays, rayhip_hit *out_hits, int *out_count) {
    if (use_device(c)) {
        return 1;
    }
    if (!c->w || !c->pmj.p || !c->filter_table.p) {
        return fail("k_generate_primary_rays needs resize + upload_static + set_filter_table first");
    }
    hipStream_t s = c->stream;
    const RayGenTiling tiling = make_raygen_tiling(c->w, c->h, rect[2], rect[3], c->shard);
    const size_t nslots = size_t(tiling.tiles) * 64u;
    if (c->clear_queues(1, s)) {
        return fail("queue counter clear failed");
    }
    const RayGenParams rg = make_raygen_params(*cam, c->w, c->h, rect, iteration, c->shard);
    // kernel-level hooks use one dense stripe so that the host sees a plain array
    k_raygen<<<grid_for(c, nslots, 256), 256, 0, s>>>(rg, c->sc.pmj, c->filter_table.as<float>(), c->px.required_samples,
                                                      c->rays[0], c->hits, c->ray_queue(0, nslots, 1), single_layer(c->w, c->h), tiling);
    HIP_TRY(hipGetLastError());
    uint32_t n = 0;
    HIP_TRY(hipMemcpyAsync(&n, c->ray_count(0), 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    HostRays hr;
    HostHits hh;
    if (download_rays(c, 0, n, hr) || download_hits(c, n, hh)) {
        return 1;
    }
    HIP_TRY(hipStreamSynchronize(s));
    rays_from_soa(hr, n, out_rays);
    hits_from_soa(hh, n, out_hits);
    *out_count = int(n);
    return 0;
}

int rayhip_k_intersect_closest(rayhip_ctx *c, const rayhip_camera *cam, rayhip_ray *rays, rayhip_hit *hits, int count,
                               int iteration, uint32_t flags, rayhip_trav_counters *out_counters) {
    if (use_device(c)) {
        return 1;
    }
    if (!c->have_scene || !c->pmj.p) {
        return fail("k_intersect_closest needs a scene and the PMJ table");
    }
    if (size_t(count) > size_t(c->w) * size_t(c->h)) {
        return fail("ray count exceeds the wavefront buffers (w*h)");
    }
    hipStream_t s = c->stream;
    HostRays hr;
    HostHits hh;
    if (upload_rays(c, rays, count, hr) || upload_hits(c, hits, count, hh)) {
        return 1;
    }
    const uint32_t n = uint32_t(count);
    HIP_TRY(hipMemcpyAsync(c->ray_count(0), &n, 4, hipMemcpyHostToDevice, s));
    unsigned long long *tc = c->trav_counters.as<unsigned long long>();
    CounterScope ks;
    if (counters_begin(c, tc, ks)) {
        return 1;
    }
    const TraceParams tp = make_trace_params(*cam, c->sc.tlas_root, iteration);
    const int g = int(std::min<size_t>(size_t(c->grid_waves), (size_t(count) + WAVE - 1) / WAVE));
    const RayQueue q = c->ray_queue(0, size_t(count), 1);
    {
        // "the kernel the passes launch", in the hook's reading of the knobs (trace_select.h: TraceRole::Hook)
        const ClosestForm form = closest_form(c->trace, c->wide, c->direct(), TraceRole::Hook, flags);
        ClosestLaunch a;
        a.sc = c->sc, a.tp = tp, a.rays = c->rays[0], a.hits = c->hits, a.queue = q, a.init_hits = 0; // (the pooled form also takes preset hits)
        a.spill = c->stack_spill.as<uint32_t>(), a.counters = tc, a.layers = single_layer(c->w, c->h);
        const int grid = form == ClosestForm::Pooled ? std::min(g, c->trace.pool_waves) : is_lane(form) ? std::min(g, c->trace.refill_waves) : g;
        launch_closest(form, std::max(1, grid), s, a);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    if (counters_end(c, tc, ks, out_counters)) {
        return 1;
    }
    if (download_rays(c, 0, size_t(count), hr, 2, 2) || download_hits(c, size_t(count), hh)) { // (of a ray the walk changes throughput and depth)
        return 1;
    }
    HIP_TRY(hipStreamSynchronize(s));
    for (int i = 0; i < count; ++i) {
        rays[i].c[0] = hr.pl[2][i].x, rays[i].c[1] = hr.pl[2][i].y, rays[i].c[2] = hr.pl[2][i].z;
        rays[i].depth = hr.xd[i].y;
    }
    hits_from_soa(hh, size_t(count), hits);
    return 0;
}

int rayhip_k_intersect_shadow(rayhip_ctx *c, const rayhip_camera *cam, const rayhip_shadow_ray *rays, int count,
                              int iteration, float *out_rc, rayhip_trav_counters *out_counters) {
    if (use_device(c)) {
        return 1;
    }
    if (!c->have_scene || !c->pmj.p) {
        return fail("k_intersect_shadow needs a scene and the PMJ table");
    }
    if (size_t(count) > size_t(c->w) * size_t(c->h)) {
        return fail("ray count exceeds the wavefront buffers (w*h)");
    }
    hipStream_t s = c->stream;
    std::vector<float4> pl[3];
    for (int k = 0; k < 3; ++k) {
        pl[k].resize(size_t(count));
    }
    for (int i = 0; i < count; ++i) {
        float depth_f, xy_f;
        memcpy(&depth_f, &rays[i].depth, 4), memcpy(&xy_f, &rays[i].xy, 4);
        pl[0][i] = make_float4(rays[i].o[0], rays[i].o[1], rays[i].o[2], depth_f);
        pl[1][i] = make_float4(rays[i].d[0], rays[i].d[1], rays[i].d[2], rays[i].dist);
        pl[2][i] = make_float4(rays[i].c[0], rays[i].c[1], rays[i].c[2], xy_f);
    }
    for (int k = 0; k < 3; ++k) {
        HIP_TRY(hipMemcpyAsync(c->shadow_planes[k].p, pl[k].data(), size_t(count) * 16, hipMemcpyHostToDevice, s));
    }
    const uint32_t n = uint32_t(count);
    HIP_TRY(hipMemcpyAsync(c->shadow_count(0), &n, 4, hipMemcpyHostToDevice, s));
    unsigned long long *tc = c->trav_counters.as<unsigned long long>() + TRAV_COUNTER_WORDS;
    CounterScope ks;
    if (counters_begin(c, tc, ks)) {
        return 1;
    }
    const TraceParams tp = make_trace_params(*cam, c->sc.tlas_root, iteration);
    const int g = int(std::min<size_t>(size_t(c->grid_waves), (size_t(count) + WAVE - 1) / WAVE));
    {
        // RAYHIP_HOOK_SHADOW_REFILL (read at every call): the product's flat persistent form over the 4-wide tree, in its direct-entry form where
        // the passes launch that (no counters); otherwise the instrumented walk of the reference's BVH2
        const ShadowForm form = shadow_form(c->trace, c->wide, c->direct(), TraceRole::Hook, 0u, getenv("RAYHIP_HOOK_SHADOW_REFILL") != nullptr);
        ShadowLaunch a;
        a.sc = c->sc, a.tp = tp, a.shadow = c->shadow, a.queue = c->shadow_queue(0, size_t(count), 1);
        a.limit = FLT_MAX, a.pitch = c->w, a.temp = c->px.temp;
        a.out_rc = c->hit_planes[0].as<float4>(); // results land in the (otherwise idle) hit plane
        a.spill = c->stack_spill.as<uint32_t>(), a.counters = tc, a.layers = single_layer(c->w, c->h);
        launch_shadow(form, g ? g : 1, s, a);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    if (counters_end(c, tc, ks, out_counters)) {
        return 1;
    }
    HIP_TRY(hipMemcpyAsync(out_rc, c->hit_planes[0].p, size_t(count) * 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

int rayhip_k_shade(rayhip_ctx *c, const rayhip_camera *cam, int bounce, int iteration, const rayhip_ray *rays, const rayhip_hit *hits,
                   int count, float *inout_color, rayhip_ray *out_secondary, int *out_secondary_count, rayhip_shadow_ray *out_shadow,
                   int *out_shadow_count) {
    if (use_device(c)) {
        return 1;
    }
    if (!c->have_scene || !c->pmj.p || !c->w) {
        return fail("k_shade needs resize + upload_static + scene_upload first");
    }
    if (count < 0 || size_t(count) > size_t(c->w) * size_t(c->h)) {
        return fail("ray count exceeds the wavefront buffers (w*h)");
    }
    if (bounce < 0 || bounce + 2 > MAX_BOUNCE_SLOTS || iteration < 1) {
        return fail("bad bounce / iteration");
    }
    hipStream_t s = c->stream;
    const size_t npix = size_t(c->w) * size_t(c->h);
    HostRays hr;
    HostHits hh;
    if (upload_rays(c, rays, count, hr) || upload_hits(c, hits, count, hh)) {
        return 1;
    }
    HIP_TRY(hipMemcpyAsync(c->px.temp, inout_color, npix * 16, hipMemcpyHostToDevice, s));
    if (c->clear_queues(bounce + 2, s)) {
        return fail("queue counter clear failed");
    }
    const uint32_t n = uint32_t(count);
    HIP_TRY(hipMemcpyAsync(c->ray_count(bounce), &n, 4, hipMemcpyHostToDevice, s));
    const int g = std::max(1, int(std::min<size_t>(size_t(c->grid_waves), (size_t(count) + WAVE - 1) / WAVE)));
    // one dense stripe, so the host sees plain arrays; the kernels are the ones rayhip_render launches
    launch_shade(c, *cam, iteration, bounce, 0, size_t(count), 1, g, c->w, 1.0f / float(iteration), single_layer(c->w, c->h));
    HIP_TRY(hipGetLastError());
    uint32_t n_sec = 0, n_sh = 0;
    HIP_TRY(hipMemcpyAsync(&n_sec, c->ray_count(bounce + 1), 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&n_sh, c->shadow_count(bounce), 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(inout_color, c->px.temp, npix * 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (download_rays(c, 1, n_sec, hr)) {
        return 1;
    }
    std::vector<float4> sp_[3];
    for (int k = 0; k < 3; ++k) {
        sp_[k].resize(n_sh);
        HIP_TRY(hipMemcpyAsync(sp_[k].data(), c->shadow_planes[k].p, size_t(n_sh) * 16, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    rays_from_soa(hr, n_sec, out_secondary);
    for (uint32_t i = 0; i < n_sh; ++i) {
        rayhip_shadow_ray &r = out_shadow[i];
        r.o[0] = sp_[0][i].x, r.o[1] = sp_[0][i].y, r.o[2] = sp_[0][i].z, memcpy(&r.depth, &sp_[0][i].w, 4);
        r.d[0] = sp_[1][i].x, r.d[1] = sp_[1][i].y, r.d[2] = sp_[1][i].z, r.dist = sp_[1][i].w;
        r.c[0] = sp_[2][i].x, r.c[1] = sp_[2][i].y, r.c[2] = sp_[2][i].z, memcpy(&r.xy, &sp_[2][i].w, 4);
    }
    *out_secondary_count = int(n_sec), *out_shadow_count = int(n_sh);
    return 0;
}

int rayhip_k_scrambled_rand(rayhip_ctx *c, const uint32_t *dims, const uint32_t *seeds, const int32_t *samples, int count,
                            float *out_xy) {
    if (use_device(c)) {
        return 1;
    }
    if (!c->pmj.p) {
        return fail("k_scrambled_rand needs the PMJ table");
    }
    hipStream_t s = c->stream;
    DevBuf d, sd, sm, o;
    if (d.alloc(size_t(count) * 4) || sd.alloc(size_t(count) * 4) || sm.alloc(size_t(count) * 4) || o.alloc(size_t(count) * 8)) {
        return 1;
    }
    HIP_TRY(hipMemcpyAsync(d.p, dims, size_t(count) * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(sd.p, seeds, size_t(count) * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(sm.p, samples, size_t(count) * 4, hipMemcpyHostToDevice, s));
    k_scrambled_rand<<<(count + 255) / 256, 256, 0, c->stream>>>(d.as<uint32_t>(), sd.as<uint32_t>(), sm.as<int32_t>(), count,
                                                                 c->sc.pmj, o.as<float2>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpyAsync(out_xy, o.p, size_t(count) * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    d.release(), sd.release(), sm.release(), o.release();
    return 0;
}

// ---- the tree builders and the wide node test on caller-supplied inputs (tests/bvh_build_cases.py) --------------------------

int rayhip_k_lbvh_build(rayhip_ctx *c, const float *boxes, const uint32_t *groups, uint32_t n_prims, uint32_t n_groups, uint32_t leaf_max,
                        int leaf_is_primitive, int roots_are_nodes, int on_host, rayhip_bvh2_node *out_nodes, uint32_t nodes_cap,
                        uint32_t *out_entries, uint32_t entries_cap, uint32_t *out_group_root, float *out_bounds, uint32_t *out_counts) {
    std::string why;
    if (!rayhip_bvh_hooks::check_lbvh_args(boxes, groups, n_prims, n_groups, leaf_max, why)) {
        return fail("k_lbvh_build: %s", why.c_str());
    }
    const rayhip_lbvh::Input in = rayhip_bvh_hooks::lbvh_input(boxes, groups, n_prims, n_groups, leaf_max, leaf_is_primitive, roots_are_nodes);
    rayhip_lbvh::Output out;
    if (on_host) {
        out = rayhip_lbvh::build_host(in);
    } else {
        if (use_device(c)) {
            return 1;
        }
        if (!rayhip_lbvh::build_device(c->stream, in, out, why)) {
            return fail("k_lbvh_build: %s", why.c_str());
        }
    }
    if (!rayhip_bvh_hooks::copy_lbvh_output(out, out_nodes, nodes_cap, out_entries, entries_cap, out_group_root, out_bounds, out_counts, why)) {
        return fail("k_lbvh_build: %s", why.c_str());
    }
    return 0;
}

int rayhip_k_bvh4_collapse(rayhip_ctx *c, const rayhip_bvh2_node *nodes, uint32_t n_nodes, const uint32_t *roots, uint32_t n_roots,
                           void *out_wide, uint32_t *out_roots4, uint32_t *out_count) {
    if (use_device(c)) {
        return 1;
    }
    *out_count = 0;
    if (n_roots == 0) {
        return 0;
    }
    std::string why;
    if (!rayhip_bvh_hooks::check_forest(nodes, n_nodes, roots, n_roots, why)) {
        return fail("k_bvh4_collapse: %s", why.c_str());
    }
    hipStream_t s = c->stream;
    DevBuf d_nodes, d_wide;
    if (d_nodes.alloc(size_t(n_nodes) * sizeof(rayhip_bvh2_node)) || d_wide.alloc(size_t(n_nodes) * sizeof(Bvh4Node))) {
        return 1;
    }
    HIP_TRY(hipMemcpyAsync(d_nodes.p, nodes, size_t(n_nodes) * sizeof(rayhip_bvh2_node), hipMemcpyHostToDevice, s));
    const std::vector<uint32_t> root_list(roots, roots + n_roots);
    uint32_t n_wide = 0;
    bool unquantisable = false;
    if (!rayhip_bvh4::build_device(s, d_nodes.as<rayhip_bvh2_node>(), n_nodes, root_list, d_wide.as<Bvh4Node>(), n_wide, why, &unquantisable)) {
        d_nodes.release(), d_wide.release();
        if (unquantisable) {
            return 2;
        }
        return fail("k_bvh4_collapse: %s", why.c_str());
    }
    HIP_TRY(hipMemcpyAsync(out_wide, d_wide.p, size_t(n_wide) * sizeof(Bvh4Node), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    d_nodes.release(), d_wide.release();
    for (uint32_t r = 0; r < n_roots; ++r) {
        out_roots4[r] = r; // (bvh4_build.hip.h: the wide node of roots[r] is r)
    }
    *out_count = n_wide;
    return 0;
}

// one thread per item; inv_d derived as the walks derive it
__global__ void __launch_bounds__(256) k_bvh4_test_nodes(const Bvh4Node *__restrict__ wide, const uint32_t *__restrict__ node_index,
                                                        const float *__restrict__ ray_o, const float *__restrict__ ray_d,
                                                        const float *__restrict__ ray_t, const uint32_t n_items, uint32_t *__restrict__ out_ref,
                                                        uint32_t *__restrict__ out_n_hit, float *__restrict__ out_dist) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_items) {
        rayhip_bvh_hooks::test_node_item(wide, node_index[i], ray_o + size_t(i) * 3, ray_d + size_t(i) * 3, ray_t[i], out_ref + size_t(i) * 4,
                                         out_n_hit + i, out_dist + size_t(i) * 4);
    }
}

int rayhip_k_bvh4_test_nodes(rayhip_ctx *c, const void *wide, uint32_t n_wide, const uint32_t *node_index, const float *ray_o, const float *ray_d,
                             const float *ray_t, uint32_t n_items, uint32_t *out_ref, uint32_t *out_n_hit, float *out_dist) {
    if (use_device(c)) {
        return 1;
    }
    if (n_items == 0) {
        return 0;
    }
    std::string why;
    if (!rayhip_bvh_hooks::check_items(node_index, n_items, n_wide, why)) {
        return fail("k_bvh4_test_nodes: %s", why.c_str());
    }
    hipStream_t s = c->stream;
    const size_t n = n_items;
    DevBuf d_wide, d_idx, d_o, d_d, d_t, d_ref, d_hit, d_dist;
    if (d_wide.alloc(size_t(n_wide) * sizeof(Bvh4Node)) || d_idx.alloc(n * 4) || d_o.alloc(n * 12) || d_d.alloc(n * 12) || d_t.alloc(n * 4) ||
        d_ref.alloc(n * 16) || d_hit.alloc(n * 4) || d_dist.alloc(n * 16)) {
        return 1;
    }
    HIP_TRY(hipMemcpyAsync(d_wide.p, wide, size_t(n_wide) * sizeof(Bvh4Node), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_idx.p, node_index, n * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_o.p, ray_o, n * 12, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_d.p, ray_d, n * 12, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_t.p, ray_t, n * 4, hipMemcpyHostToDevice, s));
    k_bvh4_test_nodes<<<(n_items + 255) / 256, 256, 0, s>>>(d_wide.as<Bvh4Node>(), d_idx.as<uint32_t>(), d_o.as<float>(), d_d.as<float>(),
                                                            d_t.as<float>(), n_items, d_ref.as<uint32_t>(), d_hit.as<uint32_t>(), d_dist.as<float>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out_ref, d_ref.p, n * 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out_n_hit, d_hit.p, n * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out_dist, d_dist.p, n * 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    d_wide.release(), d_idx.release(), d_o.release(), d_d.release(), d_t.release(), d_ref.release(), d_hit.release(), d_dist.release();
    return 0;
}

#if defined(RT_PROFILE_SHADE) || defined(RT_PROFILE_TRACE)
// tuning build only (tools/variants.py): cycles per shade-kernel section, see RT_PROF in kernels.hip.h
__attribute__((visibility("default"))) int rayhip_tuning_read_profile(rayhip_ctx *c, unsigned long long out[32], int reset) {
    if (use_device(c)) {
        return 1;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(rt::g_prof_acc), 32 * sizeof(unsigned long long)));
    if (reset) {
        unsigned long long z[32] = {};
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(rt::g_prof_acc), z, sizeof(z)));
    }
    return 0;
}
#endif

} // extern "C"
