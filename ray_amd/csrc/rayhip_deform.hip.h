// rayhip_deform.hip.h -- part of librayhip's host side (one translation unit: included by rayhip.hip before rayhip_upload.hip.h):
// deforming a scene that is on the device.  In reading order:
//   - the tables an upload or instance update leaves behind (prepare_refit, keep_light_vertices, upload_vertex_checks,
//     upload_instance_checks, upload_material_checks, prepare_light_refit);
//   - what the entry points share: the phase stamps, the preconditions, the launch grid, the read-back;
//   - the light refit and the geometry refit behind new vertices, and the top level behind either;
//   - the vertex updates (rayhip_scene_update_vertices, its _blob and _device forms; refit.h);
//   - the calls that take slots and records, each from host or device memory: the instances that move
//     (rayhip_scene_set_instance_transforms[_device]; instances.h), the analytic lights that move or change colour
//     (rayhip_scene_set_lights[_device]; light_pose.h) and the materials that change, with the triangle lights they colour
//     (rayhip_scene_set_materials[_device]; materials.h);
//   - the handles over vertex ranges: skins (rayhip_skin_create / _destroy; skin.h), morph sets (rayhip_morph_create / _destroy;
//     morph.h) and normal sets (rayhip_normals_create / _destroy; normals.h: recomputed at the top of the geometry refit);
//   - the poses (rayhip_scene_pose, and rayhip_scene_pose_skins, which is the same without morph sets);
//   - the switch (rayhip_scene_refit_lights; light_refit.h).
#pragma once

// what the refit needs of the upload's half of the launcher (rayhip_upload.hip.h)
static int rebuild_top_level(rayhip_ctx *c, const rayhip_update::Plan &up, uint32_t &tlas_root, rayhip_lbvh::Box &root_box);
static void refresh_top_level_view(rayhip_ctx *c, uint32_t tlas_root, const rayhip_lbvh::Box &root_box, uint32_t live_instances);

// ---- what a later rayhip_scene_update_vertices needs of an upload (refit.h) -----------------------------------------------------
// the bottom-level nodes sorted by height and the first entry of every triangle, on the device; the root list of the collapse; the
// live instances and the instance array on the host.  `nodes` / `instances` / `tri_indices`: the arrays as uploaded.
static int prepare_refit(rayhip_ctx *c, const rayhip_bvh2_node *nodes, const uint32_t nodes_count, const rayhip_mesh_instance *instances,
                         const uint32_t instances_count, const uint32_t tlas_root, const uint32_t *tri_indices, const uint32_t entries,
                         const uint32_t *vtx_indices, const uint32_t n_tris, const uint32_t n_vertices, const bool rebased_for_bvh8) {
    rayhip_ctx::Refit &r = c->refit;
    r.level_offset.clear(), r.roots.clear(), r.ordinal_of_root.clear(), r.live.clear();
    r.levels_rc = 2, r.entries = entries, r.degenerate = 0;
    // the vertices some triangle of the table uses: the vertex array is a sparse pool, a free slot may hold anything
    r.vertex_used.assign(n_vertices, 0);
    for (uint32_t e = 0; e < entries; ++e) {
        for (uint32_t k = 0; tri_indices[e] < n_tris && k < 3; ++k) {
            const uint32_t v = vtx_indices[size_t(tri_indices[e]) * 3 + k];
            if (v < n_vertices) {
                r.vertex_used[v] = 1;
            }
        }
    }
    r.instances.assign(instances, instances + instances_count);
    std::vector<std::pair<uint32_t, uint32_t>> top;
    if (tlas_root != 0xffffffffu && rayhip_rebuild::collect_leaf_ranges(nodes, nodes_count, tlas_root, top)) {
        for (const auto &leaf : top) {
            r.live.push_back(leaf.first);
        }
        std::sort(r.live.begin(), r.live.end());
        r.live.erase(std::unique(r.live.begin(), r.live.end()), r.live.end());
    }
    if (rebased_for_bvh8) {
        return 0; // (the 8-wide builder is host-only: such a context refuses the vertex update)
    }
    std::vector<uint32_t> root_of_instance;
    if (!rayhip_bvh4::collect_roots(nodes, nodes_count, instances, instances_count, tlas_root, r.roots, root_of_instance)) {
        r.roots.clear();
    }
    for (size_t k = 0; k < r.roots.size(); ++k) {
        r.ordinal_of_root[r.roots[k]] = uint32_t(k);
    }
    std::vector<uint32_t> level_nodes;
    r.levels_rc = rayhip_refit::plan_levels(nodes, nodes_count, r.roots, level_nodes, r.level_offset);
    if (r.levels_rc != 0) {
        return 0; // (a tree above 128 levels: the update says so when it is asked for)
    }
    const std::vector<uint32_t> first = rayhip_refit::first_entries(tri_indices, entries, n_tris);
    if (upload(c, r.level_nodes, level_nodes.data(), level_nodes.size() * sizeof(uint32_t)) ||
        upload(c, r.first_entry, first.data(), first.size() * sizeof(uint32_t)) ||
        r.scratch.alloc(256 + r.roots.size() * (sizeof(uint32_t) + sizeof(rayhip_bvh2_node)) + 64)) {
        return 1;
    }
    HIP_TRY(hipStreamSynchronize(c->stream)); // the two vectors go out of scope
    return 0;
}

// f(light) for every triangle light that li_indices names: params[0] is its triangle, params[1] its instance slot, both as bits
static void for_each_triangle_light(const rayhip_scene_desc *d, const std::function<void(const rayhip_light &)> &f) {
    for (uint32_t k = 0; k < d->li_indices_count; ++k) {
        const uint32_t i = d->li_indices[k];
        if (i < d->lights_count && light_type(d->lights[i]) == LIGHT_TYPE_TRI) {
            f(d->lights[i]);
        }
    }
}

// the vertices some triangle light's triangle uses, as they are on the device: the light arrays are not rebuilt by a vertex update,
// so it refuses to move one of these
static void keep_light_vertices(rayhip_ctx *c, const rayhip_scene_desc *d) {
    std::vector<std::pair<uint32_t, rayhip_vertex>> &kept = c->refit.light_vertices;
    kept.clear();
    for_each_triangle_light(d, [&](const rayhip_light &l) {
        const size_t tri = float_as_uint(l.params[0]);
        for (size_t j = tri * 3; j < tri * 3 + 3 && j < d->vtx_indices_count; ++j) {
            if (d->vtx_indices[j] < d->vertices_count) {
                kept.emplace_back(d->vtx_indices[j], d->vertices[d->vtx_indices[j]]);
            }
        }
    });
    std::sort(kept.begin(), kept.end(), [](const auto &x, const auto &y) { return x.first < y.first; });
    kept.erase(std::unique(kept.begin(), kept.end(), [](const auto &x, const auto &y) { return x.first == y.first; }), kept.end());
}

// ... and on the device, with the per-vertex `used` flags, for the updates whose vertices never pass through the host
// (k_skin_vertices, k_check_vertices: skin.hip.h).  `with_used`: the flags too (they change with an upload only).
static int upload_vertex_checks(rayhip_ctx *c, const bool with_used) {
    rayhip_ctx::Refit &r = c->refit;
    std::vector<uint32_t> index(r.light_vertices.size());
    std::vector<rayhip_vertex> kept(r.light_vertices.size());
    for (size_t k = 0; k < r.light_vertices.size(); ++k) {
        index[k] = r.light_vertices[k].first, kept[k] = r.light_vertices[k].second;
    }
    if (upload(c, r.d_light_index, index.data(), index.size() * sizeof(uint32_t)) ||
        upload(c, r.d_light_vertices, kept.data(), kept.size() * sizeof(rayhip_vertex)) ||
        (with_used && upload(c, r.d_vertex_used, r.vertex_used.data(), r.vertex_used.size()))) {
        return 1;
    }
    HIP_TRY(hipStreamSynchronize(c->stream)); // the two vectors go out of scope
    return 0;
}

// ... and what a call that moves instances checks its slots against (rayhip_scene_set_instance_transforms; instances.h, k_pose_instances):
// per slot of the instance array whether the top level names it (refit.live, refit.instances: set before this is called) and whether a
// triangle light hangs on it, on the host and on the device, with the live slots and one claim word per slot.  `d`: the light arrays.
static int upload_instance_checks(rayhip_ctx *c, const rayhip_scene_desc *d) {
    rayhip_ctx::Refit &r = c->refit;
    r.slot_flags.assign(r.instances.size(), 0);
    for (const uint32_t mi : r.live) {
        if (mi < r.slot_flags.size()) {
            r.slot_flags[mi] |= uint8_t(rayhip_instances::SLOT_LIVE);
        }
    }
    for_each_triangle_light(d, [&](const rayhip_light &l) {
        const uint32_t mi = float_as_uint(l.params[1]);
        if (mi < r.slot_flags.size()) {
            r.slot_flags[mi] |= uint8_t(rayhip_instances::SLOT_TRI_LIGHTS);
        }
    });
    if (upload(c, r.d_slot_flags, r.slot_flags.data(), r.slot_flags.size()) || upload(c, r.d_live, r.live.data(), r.live.size() * sizeof(uint32_t)) ||
        r.d_slot_claim.alloc(r.slot_flags.size() * sizeof(uint32_t)) || hipStreamSynchronize(c->stream) != hipSuccess) {
        r.slot_flags.clear(); // (no table on the device: a call that moves instances says that it needs an upload)
        return fail("the per-slot table of the instances could not be uploaded");
    }
    return 0;
}

// ... and what a call that changes materials checks its slots against (rayhip_scene_set_materials; materials.h, k_check_materials): per
// material slot whether the scene uses it and whether a triangle light took its colour from it, on the host and on the device, one
// claim word per slot, and per light slot its emitter (k_recolour_tri_lights).  `d`: the light arrays, tri_materials and materials;
// `used`: the validation's per-slot bytes (an upload), or null: the slots in use stay (an instance update names no mesh the upload
// did not bring) and only the emitters are found again, by the graph of `d`'s materials
static int upload_material_checks(rayhip_ctx *c, const rayhip_scene_desc *d, const std::vector<uint8_t> *used) {
    namespace rm = rayhip_materials;
    rayhip_ctx::MaterialChecks &mc = c->material_checks;
    if (used) {
        mc.flags.assign(d->materials_count, 0);
        for (size_t m = 0; m < mc.flags.size() && m < used->size(); ++m) {
            mc.flags[m] = (*used)[m] ? uint8_t(rm::SLOT_LIVE) : uint8_t(0);
        }
    } else if (mc.flags.size() != d->materials_count) { // (an upload that failed half-way: nothing to keep)
        mc.flags.clear();
        return 0;
    }
    std::vector<uint16_t> light_emitter;
    rm::emitter_tables(d->lights, d->lights_count, d->li_indices, d->li_indices_count, d->tri_materials, d->tri_materials_count, d->materials, d->materials_count,
                       light_emitter, mc.flags);
    if (upload(c, mc.d_flags, mc.flags.data(), mc.flags.size()) || upload(c, mc.d_light_emitter, light_emitter.data(), light_emitter.size() * sizeof(uint16_t)) ||
        mc.d_claim.alloc(mc.flags.size() * sizeof(uint32_t)) || hipStreamSynchronize(c->stream) != hipSuccess) {
        mc.flags.clear(); // (no table on the device: a call that changes materials says that it needs an upload)
        return fail("the per-slot table of the materials could not be uploaded");
    }
    return 0;
}

// ---- what a light refit needs of the lights that are on the device (rayhip_scene_refit_lights; light_refit.h) ------------------------
// the tree's nodes sorted by height, the leaf summary table (lights that are no triangles complete: they do not move with vertices;
// their flux from the tree as uploaded, since the environment light's is the quadtree's mean luminance, which the device computes
// only when the map changes there: rayhip_environment.hip.h), the flux scales of the inner slots (light_refit.h: slot_scales, one host refit at the pose the tree was built at) and the
// scratch of the level launches.  `d`: the light arrays, vertices, indices and instances as they are on the device.
static int prepare_light_refit(rayhip_ctx *c, const rayhip_scene_desc *d) {
    const rayhip_light *lights = d->lights;
    const rayhip_light_cwbvh_node *nodes = d->light_cwnodes;
    const uint32_t n_lights = d->lights_count, n_nodes = d->light_cwnodes_count;
    rayhip_ctx::LightRefit &lr = c->light_refit;
    lr.ready = false, lr.tri_leaves = false;
    std::vector<uint32_t> level_nodes;
    if (const int rc = rayhip_light_refit::plan_levels(nodes, n_nodes, n_lights, level_nodes, lr.level_offset)) {
        return rc == 2 ? fail("rayhip_scene_refit_lights: the light tree is higher than %u levels", rayhip_light_refit::MAX_LEVELS)
                       : fail("rayhip_scene_refit_lights: a link of the light tree leaves its arrays, or a child lies before its parent");
    }
    const std::vector<rayhip_light_refit::Summary> leaf = rayhip_light_refit::leaf_table(lights, n_lights, nodes, n_nodes);
    std::vector<float> scales;
    if (rayhip_light_refit::slot_scales(lights, n_lights, d->li_indices, d->li_indices_count, d->mesh_instances, d->mesh_instances_count, d->vtx_indices,
                                        d->vtx_indices_count, d->vertices, d->vertices_count, nodes, n_nodes, scales)) {
        return fail("rayhip_scene_refit_lights: the light tree could not be refitted on the host");
    }
    if (upload(c, lr.slot_scale, scales.data(), scales.size() * sizeof(float)) || upload(c, lr.level_nodes, level_nodes.data(), level_nodes.size() * sizeof(uint32_t)) ||
        upload(c, lr.leaf, leaf.data(), leaf.size() * sizeof(rayhip_light_refit::Summary)) ||
        lr.node_summary.alloc(size_t(n_nodes) * sizeof(rayhip_light_refit::Summary))) {
        return 1;
    }
    // ... and what rayhip_scene_set_lights checks its slots against (light_pose.h): the slots li_indices names, one claim word per slot,
    // and the table of the lights it replaced -- none: the tree just uploaded holds the words of every leaf
    const std::vector<uint8_t> live = rayhip_light_pose::live_table(d->li_indices, d->li_indices_count, n_lights);
    if (upload(c, lr.live, live.data(), live.size()) || lr.posed.alloc(n_lights) || lr.claim.alloc(size_t(n_lights) * sizeof(uint32_t))) {
        return 1;
    }
    HIP_TRY(hipMemsetAsync(lr.posed.p, 0, lr.posed.bytes, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream)); // the four vectors go out of scope
    lr.ready = true;
    return 0;
}

// ---- the phase stamps of a vertex update (RAYHIP_TRACE_UPLOAD) ------------------------------------------------------------------------
// A stamp waits for the device first, so that the phases can be told apart -- only when tracing.  `who`: the entry point the line names.
struct VertexStamps {
    rayhip_ctx *c;
    const char *who;
    bool on = getenv("RAYHIP_TRACE_UPLOAD") != nullptr;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now(); // the start of the call
    hipError_t stamp(const char *msg) const {
        const hipError_t e = on ? hipStreamSynchronize(c->stream) : hipSuccess;
        if (on && e == hipSuccess) {
            fprintf(stderr, "%s: %9.3f ms  %s\n", who, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), msg);
        }
        return e;
    }
};

// ---- what the entry points share: the preconditions, the launch grid, the read-back -------------------------------------------------------
// blocks of 256 lanes over n items
static unsigned blocks_of(const size_t n) { return unsigned((n + 255) / 256); }

// `bytes` of a device buffer onto the host, now
static bool read_back(void *dst, const DevBuf &src, const size_t bytes) {
    return bytes == 0 || hipMemcpy(dst, src.p, bytes, hipMemcpyDeviceToHost) == hipSuccess;
}

// the refusals of every call that changes the scene on the device: a pointer the caller had to give and did not (`null_pointer`), no
// scene, and -- of the calls that rebuild a tree (`builds_trees`) -- the 8-wide form.  0 = go on, 1 / 2 = the return code
static int scene_change_possible(rayhip_ctx *c, const char *who, const bool null_pointer, const bool builds_trees) {
    if (null_pointer) {
        return fail("%s: a null pointer", who);
    }
    if (!c->have_scene) {
        (void)fail("%s before rayhip_scene_upload", who);
        return 2;
    }
    if (builds_trees && c->wide == 8) {
        (void)fail("%s: the context walks the 8-wide tree, whose builder runs on the host only", who);
        return 2;
    }
    return 0;
}

// 0 = the context can take a vertex update, 2 = it needs rayhip_scene_upload
static int vertex_update_possible(rayhip_ctx *c, const char *who) {
    if (const int rc = scene_change_possible(c, who, false, true)) {
        return rc;
    }
    // (vertex_used: prepare_refit assigns one flag per vertex, so after a successful upload the sizes agree; only an upload that
    // failed after it, over a scene that was there, leaves them apart -- and the checks below index the flags by the scene's count)
    if (c->refit.levels_rc != 0 || c->refit.vertex_used.size() != c->geometry.vertices) {
        (void)fail("%s: a bottom-level tree is higher than %u levels", who, rayhip_refit::MAX_LEVELS);
        return 2;
    }
    return 0;
}

static int outside_the_scene(const rayhip_ctx *c, const char *who, const uint32_t first, const uint32_t count) {
    return fail("%s: vertices [%u, %u + %u) are outside the %u of the uploaded scene", who, first, first, count, c->geometry.vertices);
}

// Light vertices are pinned unless the switch is on (rayhip_scene_refit_lights: the lights follow their vertices).  The lowest vertex of
// [first, first + count) that a triangle light uses and that would move, or null: `vertices` are the new ones, of which a bytewise
// unchanged one passes; without them every light vertex of the range counts.  (The device form: k_check_vertices, skin.hip.h.)
static const uint32_t *pinned_light_vertex(const rayhip_ctx *c, const uint32_t first, const uint32_t count, const rayhip_vertex *vertices) {
    if (c->light_refit.on) {
        return nullptr;
    }
    for (const auto &kept : c->refit.light_vertices) { // (ascending; few)
        if (kept.first >= first && kept.first - first < count &&
            (!vertices || memcmp(&vertices[kept.first - first], &kept.second, sizeof(rayhip_vertex)) != 0)) {
            return &kept.first;
        }
    }
    return nullptr;
}

// ---- the light refit, in stream order behind whatever moved the lights (light_refit.hip.h) ------------------------------------------------
// the tree alone, one launch per height, lowest first: under the leaf table as it is on the device now
static int refit_light_levels(rayhip_ctx *c) {
    rayhip_ctx::LightRefit &lr = c->light_refit;
    for (size_t h = 0; h + 1 < lr.level_offset.size(); ++h) {
        const uint32_t n = lr.level_offset[h + 1] - lr.level_offset[h];
        if (n == 0) {
            continue;
        }
        rayhip_light_refit::k_refit_light_level<<<blocks_of(size_t(n) * 8), 256, 0, c->stream>>>(
            c->light_cwnodes.as<rayhip_light_cwbvh_node>(), lr.level_nodes.as<uint32_t>() + lr.level_offset[h], n, c->lights.as<rayhip_light>(),
            lr.leaf.as<rayhip_light_refit::Summary>(), lr.node_summary.as<rayhip_light_refit::Summary>(), c->light_children.as<float4>(),
            lr.slot_scale.as<float>(), lr.posed.as<uint8_t>());
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// the whole of it: the triangle lights' corners and summaries from the vertices and instances that are on the device now, then the tree.
// `d_degenerate`: where the triangle lights without area are counted (device memory, zeroed by the caller)
static int refit_lights(rayhip_ctx *c, uint32_t *d_degenerate, const VertexStamps &st) {
    rayhip_ctx::LightRefit &lr = c->light_refit;
    if (!lr.ready) {
        return fail("rayhip_scene_refit_lights is on, but its tables are not prepared");
    }
    hipStream_t s = c->stream;
    if (lr.li_count) {
        rayhip_light_refit::k_refit_tri_lights<<<blocks_of(lr.li_count), 256, 0, s>>>(
            c->lights.as<rayhip_light>(), lr.lights_count, c->li_indices.as<uint32_t>(), lr.li_count, c->mesh_instances.as<rayhip_mesh_instance>(), c->instances_count,
            c->vtx_indices.as<uint32_t>(), c->geometry.vtx_indices, c->vertices.as<rayhip_vertex>(), c->geometry.vertices, c->light_tri_geom.as<float4>(),
            lr.leaf.as<rayhip_light_refit::Summary>(), d_degenerate);
        HIP_TRY(hipGetLastError());
    }
    lr.tri_leaves = true;
    HIP_TRY(st.stamp("light corners"));
    if (refit_light_levels(c)) {
        return 1;
    }
    HIP_TRY(st.stamp("light tree refitted"));
    return 0;
}

// ---- the top level behind new instance boxes: what a vertex update and a call that moves instances end with ------------------------------
// `up`: the live slots and their boxes (and, of a vertex update, the instance array and the 4-wide roots).  The arrays under the top
// level are the new ones already, so a plan that "needs an upload" (2) is an error here.  The line names `st.who`.
static int rebuild_top_level_behind(rayhip_ctx *c, const rayhip_update::Plan &up, const VertexStamps &st) {
    uint32_t tlas_root = 0xffffffffu;
    rayhip_lbvh::Box root_box = rayhip_lbvh::empty_box();
    if (const int rc = rebuild_top_level(c, up, tlas_root, root_box)) {
        return rc == 2 ? fail("%s: %s", st.who, std::string(g_err).c_str()) : rc;
    }
    refresh_top_level_view(c, tlas_root, root_box, uint32_t(up.live.size()));
    HIP_TRY(st.stamp("top level built"));
    return 0;
}

// ---- vertex update: meshes deform in place, the trees are kept and refitted on the device ----------------------------------------
// Kept: tree topology, triangle order (tri_indices), materials, lights, instances.  Recomputed from the new positions, all in stream
// order: the triangle records (k_refit_tris), the child boxes of every bottom-level BVH2 node (k_refit_level, one launch per height),
// the per-triangle vertex table (k_fill_tri_verts), the 4-wide collapse over the same root list, the instance boxes (host, from the root
// nodes read back) and the top level (the path of rayhip_scene_update_instances).  refit.h / refit.hip.h.

// the live normal sets (rayhip_normals_create; normals.h, normals.hip.h): n and / or b of every set's range recomputed in place from the
// positions and uvs that are in the vertex array now -- every set, whatever range the call wrote, as the refit refits every tree.  The
// sets do not depend on each other: a face record is made of positions and uvs, which no set writes.  Nothing is launched, stamped or
// waited for while no set is live.
static int recompute_normal_sets(rayhip_ctx *c, const VertexStamps &st) {
    bool any = false;
    for (const rayhip_ctx::Normals &n : c->normal_sets) {
        if (!n.live) {
            continue;
        }
        any = true;
        if (n.faces_count == 0) {
            continue; // (no tree reaches a triangle of the range: every record stays)
        }
        rayhip_normals::k_face_frames<<<blocks_of(n.faces_count), 256, 0, c->stream>>>(c->vertices.as<rayhip_vertex>(), c->vtx_indices.as<uint32_t>(),
                                                                                       n.faces.as<uint32_t>(), n.faces_count,
                                                                                       n.frames.as<rayhip_normals::FaceFrame>());
        HIP_TRY(hipGetLastError());
        rayhip_normals::k_vertex_frames<<<blocks_of(n.count), 256, 0, c->stream>>>(
            c->vertices.as<rayhip_vertex>() + n.first, n.row.as<uint32_t>(), n.entries.as<uint32_t>(), n.welded ? n.wrow.as<uint32_t>() : nullptr,
            n.welded ? n.wentries.as<uint32_t>() : nullptr, n.frames.as<rayhip_normals::FaceFrame>(), n.count, n.flags);
        HIP_TRY(hipGetLastError());
    }
    if (any) {
        HIP_TRY(st.stamp("normals recomputed"));
    }
    return 0;
}

// everything a vertex update recomputes once the new vertices are in c->vertices (in stream order behind them).  `st`: the caller's
// stamps, for the start of the call; the lines written from here name rayhip_scene_update_vertices whichever entry point called
// (tools/vertex_update_bench.py reads the phases by that prefix)
static int refit_after_vertices(rayhip_ctx *c, VertexStamps st) {
    st.who = "rayhip_scene_update_vertices";
    if (recompute_normal_sets(c, st)) { // first: the table of k_fill_tri_verts, the light refit and the frames read the new n and b
        return 1;
    }
    rayhip_ctx::Refit &r = c->refit;
    hipStream_t s = c->stream;
    const uint32_t n_tris = c->geometry.vtx_indices / 3;
    uint32_t *d_degenerate = r.scratch.as<uint32_t>();
    HIP_TRY(hipMemsetAsync(d_degenerate, 0, 2 * sizeof(uint32_t), s)); // ([1]: triangle LIGHTS without area, when the lights are refitted)
    if (r.entries) {
        rayhip_refit::k_refit_tris<<<blocks_of(r.entries), 256, 0, s>>>(c->vertices.as<rayhip_vertex>(), c->geometry.vertices, c->vtx_indices.as<uint32_t>(),
                                                                        n_tris, c->tri_indices.as<uint32_t>(), r.first_entry.as<uint32_t>(), r.entries,
                                                                        c->tris.as<float4>(), c->tri_pitch, d_degenerate);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(st.stamp("triangle records"));
    for (size_t h = 1; h < r.level_offset.size(); ++h) {
        const uint32_t n = r.level_offset[h] - r.level_offset[h - 1];
        rayhip_refit::k_refit_level<<<blocks_of(n), 256, 0, s>>>(c->nodes.as<rayhip_bvh2_node>(), r.level_nodes.as<uint32_t>() + r.level_offset[h - 1], n,
                                                                 c->tri_indices.as<uint32_t>(), c->vtx_indices.as<uint32_t>(), c->vertices.as<rayhip_vertex>());
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(st.stamp("boxes refitted"));
    if (n_tris) {
        k_fill_tri_verts<<<blocks_of(n_tris), 256, 0, s>>>(c->vertices.as<rayhip_vertex>(), c->geometry.vertices, c->vtx_indices.as<uint32_t>(), n_tris,
                                                           c->tri_materials.as<rayhip_tri_mat_data>(), c->geometry.tri_materials, c->tri_verts.as<float4>(),
                                                           c->tri_bitangents.as<float4>());
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(st.stamp("tri_verts done"));
    if (c->light_refit.on) { // rayhip_scene_refit_lights: the lights follow the vertices just written
        if (refit_lights(c, d_degenerate + 1, st)) {
            return 1;
        }
        HIP_TRY(hipMemcpyAsync(&c->light_refit.degenerate, d_degenerate + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    }
    // the root node of every mesh in use -> the host; the count of triangles without area comes with them
    std::vector<rayhip_bvh2_node> root_nodes(r.roots.size());
    {
        uint32_t *d_which = reinterpret_cast<uint32_t *>(r.scratch.as<uint8_t>() + 256);
        rayhip_bvh2_node *d_roots = reinterpret_cast<rayhip_bvh2_node *>(r.scratch.as<uint8_t>() + 256 + ((r.roots.size() * sizeof(uint32_t) + 63) & ~size_t(63)));
        if (!r.roots.empty()) {
            HIP_TRY(hipMemcpyAsync(d_which, r.roots.data(), r.roots.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
            rayhip_refit::k_gather_nodes<<<blocks_of(r.roots.size()), 256, 0, s>>>(c->nodes.as<rayhip_bvh2_node>(), d_which, uint32_t(r.roots.size()),
                                                                                   d_roots);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(root_nodes.data(), d_roots, r.roots.size() * sizeof(rayhip_bvh2_node), hipMemcpyDeviceToHost, s));
        }
        HIP_TRY(hipMemcpyAsync(&r.degenerate, d_degenerate, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    }
    // the 4-wide trees over the boxes just written: the same root list as at upload, so the wide node of roots[k] is k again
    if (c->wide == 4 && !r.roots.empty()) {
        uint32_t n_wide = 0;
        std::string why;
        bool unquantisable = false;
        if (!rayhip_bvh4::build_device(s, c->nodes.as<rayhip_bvh2_node>(), c->nodes_used, r.roots, c->nodes4.as<Bvh4Node>(), n_wide, why, &unquantisable)) {
            if (!unquantisable) {
                return fail("4-wide collapse failed: %s", why.c_str());
            }
            // a box the grid cannot hold: the kernels walk the BVH2 from here on, as after an upload of such a scene
            c->wide = 0, c->trace.small_scene = false;
            c->sc.nodes4 = nullptr, c->sc.blas_root4 = nullptr;
            for (auto &ref : c->mesh_refs) {
                ref.second.root4 = 0;
            }
        }
    }
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(st.stamp(c->wide == 4 ? "bvh4 built" : "no wide BLAS"));
    if (st.on) {
        fprintf(stderr, "rayhip_scene_update_vertices: %u triangles without area\n", r.degenerate);
        if (c->light_refit.on) {
            fprintf(stderr, "rayhip_scene_update_vertices: %u triangle lights without area\n", c->light_refit.degenerate);
        }
    }
    // the top level over the new instance boxes: the live slots and the instance array of the last upload / instance update.  The leaf
    // numbering is the one scene_update.h: plan documents (a leaf names the slot the host's leaf named); the box of a slot is made from
    // that slot's own mesh and transform, which is what the walk follows the leaf to.
    rayhip_update::Plan up;
    up.live = r.live, up.instances = r.instances;
    up.root4.assign(up.instances.size(), 0u);
    for (const uint32_t mi : up.live) {
        const auto it = mi < up.instances.size() ? r.ordinal_of_root.find(up.instances[mi].node_index) : r.ordinal_of_root.end();
        if (it == r.ordinal_of_root.end()) {
            return fail("rayhip_scene_update_vertices: instance %u has no tree on the device", mi);
        }
        up.root4[mi] = c->wide == 4 ? it->second : 0u;
        up.boxes.push_back(rayhip_rebuild::transform_box(rayhip_rebuild::node_box(root_nodes[it->second]), up.instances[mi].xform));
    }
    if (c->wide == 4) {
        for (auto &ref : c->mesh_refs) {
            const auto it = r.ordinal_of_root.find(ref.second.node_index);
            if (it != r.ordinal_of_root.end()) {
                ref.second.root4 = it->second;
            }
        }
        if (upload(c, c->blas_root4, up.root4.data(), up.root4.size() * sizeof(uint32_t))) {
            return 1;
        }
        HIP_TRY(hipStreamSynchronize(s));
    }
    return rebuild_top_level_behind(c, up, st);
}

// ---- the entry points ----------------------------------------------------------------------------------------------------------------------
// vertices from the host: checked here, in loops, before anything is copied
int rayhip_scene_update_vertices(rayhip_ctx *c, uint32_t first_vertex, uint32_t count, const rayhip_vertex *vertices) {
    if (use_device(c)) {
        return 1;
    }
    if (const int rc = vertex_update_possible(c, "rayhip_scene_update_vertices")) {
        return rc;
    }
    if (uint64_t(first_vertex) + count > c->geometry.vertices || (count != 0 && vertices == nullptr)) {
        return outside_the_scene(c, "rayhip_scene_update_vertices", first_vertex, count);
    }
    for (uint32_t i = 0; i < count; ++i) {
        if (c->refit.vertex_used[first_vertex + i] &&
            (!std::isfinite(vertices[i].p[0]) || !std::isfinite(vertices[i].p[1]) || !std::isfinite(vertices[i].p[2]))) {
            return fail("rayhip_scene_update_vertices: the position of vertex %u is not finite", first_vertex + i);
        }
    }
    if (const uint32_t *pinned = pinned_light_vertex(c, first_vertex, count, vertices)) {
        (void)fail("rayhip_scene_update_vertices: vertex %u belongs to a triangle light; lights are not rebuilt by this call", *pinned);
        return 2;
    }
    const VertexStamps st{c, "rayhip_scene_update_vertices"};
    HIP_TRY(hipStreamSynchronize(c->stream)); // pending passes read the old arrays
    HIP_TRY(st.stamp("begin"));
    if (count) {
        HIP_TRY(hipMemcpyAsync(c->vertices.as<rayhip_vertex>() + first_vertex, vertices, size_t(count) * sizeof(rayhip_vertex), hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(st.stamp("vertices copied"));
    return refit_after_vertices(c, st);
}

int rayhip_scene_update_vertices_blob(rayhip_ctx *c, const void *blob, size_t size) {
    rayhip_scene_desc d;
    rayhip_camera cam;
    const float *ft = nullptr;
    int ftn = 0;
    std::string err;
    if (!rayhip_blob::deserialize(blob, size, d, cam, &ft, &ftn, err, nullptr)) {
        return fail("%s", err.c_str());
    }
    if (c && c->have_scene && (d.vertices_count != c->geometry.vertices || d.vtx_indices_count != c->geometry.vtx_indices)) {
        return fail("rayhip_scene_update_vertices_blob: the blob holds %u vertices / %u indices, the uploaded scene %u / %u", d.vertices_count,
                    d.vtx_indices_count, c->geometry.vertices, c->geometry.vtx_indices);
    }
    return rayhip_scene_update_vertices(c, 0, d.vertices_count, d.vertices);
}

// ---- vertex updates whose vertices never pass through the host: arrays the caller holds on the device, and poses --------------------
// Both run kernels over the new vertices BEFORE the vertex array is written (checked where the caller has them / posed into a staging
// array), read the counters back, and only then copy device to device and refit: a refused update has touched nothing.  skin.h,
// skin.hip.h.  The two flows share that order and the refit (refit_after_vertices), and nothing between: one kernel here and one per
// segment of a pose, two counters judged or one, one copy or one per range.  What the flows further down do share step for step is
// written once: the two forms of a slots-and-records call (set_records), the three kinds of handle (RangeTable in rayhip_ctx.hip.h and
// the helpers above rayhip_skin_create), the two poses (pose_ranges) and the top level behind new boxes (rebuild_top_level_behind).
int rayhip_scene_update_vertices_device(rayhip_ctx *c, uint32_t first_vertex, uint32_t count, const rayhip_vertex *device_vertices) {
    if (!c || use_device(c)) {
        return 1;
    }
    if (const int rc = vertex_update_possible(c, "rayhip_scene_update_vertices_device")) {
        return rc;
    }
    if (uint64_t(first_vertex) + count > c->geometry.vertices || (count != 0 && device_vertices == nullptr)) {
        return outside_the_scene(c, "rayhip_scene_update_vertices_device", first_vertex, count);
    }
    const VertexStamps st{c, "rayhip_scene_update_vertices_device"};
    HIP_TRY(hipStreamSynchronize(c->stream)); // pending passes read the old arrays
    HIP_TRY(st.stamp("begin"));
    hipStream_t s = c->stream;
    rayhip_ctx::Refit &r = c->refit;
    if (c->skin_counters.alloc(2 * sizeof(uint32_t))) {
        return 1;
    }
    uint32_t *d_counters = c->skin_counters.as<uint32_t>();
    uint32_t counters[2] = {0, 0};
    const uint32_t n_lights = c->light_refit.on ? 0u : uint32_t(r.light_vertices.size()); // (refitted lights may move: nothing to compare)
    if (count) {
        HIP_TRY(hipMemsetAsync(d_counters, 0, 2 * sizeof(uint32_t), s));
        rayhip_skin::k_check_vertices<<<blocks_of(std::max(count, n_lights)), 256, 0, s>>>(device_vertices, first_vertex, count, r.d_vertex_used.as<uint8_t>(),
                                                                                           r.d_light_index.as<uint32_t>(), r.d_light_vertices.as<rayhip_vertex>(),
                                                                                           n_lights, d_counters);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(counters, d_counters, sizeof(counters), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    HIP_TRY(st.stamp("vertices checked"));
    if (counters[0] != 0) {
        return fail("rayhip_scene_update_vertices_device: the position of %u vertices is not finite", counters[0]);
    }
    if (counters[1] != 0) {
        (void)fail("rayhip_scene_update_vertices_device: %u vertices of triangle lights changed; lights are not rebuilt by this call", counters[1]);
        return 2;
    }
    // (the counters are back and zero: from here on the live vertex array is written)
    if (count) {
        HIP_TRY(hipMemcpyAsync(c->vertices.as<rayhip_vertex>() + first_vertex, device_vertices, size_t(count) * sizeof(rayhip_vertex), hipMemcpyDeviceToDevice, s));
    }
    HIP_TRY(st.stamp("vertices copied"));
    return refit_after_vertices(c, st);
}

// ---- calls that take slots and records: n slots of an array on the device and n records of RecordBytes for them -----------------------
// What the host and the device form of such a call do around its body.  `possible`: the preconditions, asked first; an empty call that
// passes them returns 0 with nothing touched.  `host_args`: the context's buffer that takes a copy of the caller's HOST arrays, [n]
// records then [n] slots; null: `slots` and `records` are device memory, complete and stable until the call returns, and go to the
// body as they are.  (The body waits for the stream before it returns: host arrays may go away then.)  RecordBytes: a multiple of 4 --
// the size of Record, but for a record that is passed as its first float (a transform: sixteen).
extern "C++" template <typename Record, size_t RecordBytes = sizeof(Record)>
static int set_records(rayhip_ctx *c, const char *who, const uint32_t n, const uint32_t *slots, const Record *records, DevBuf rayhip_ctx::*host_args,
                       int (*possible)(rayhip_ctx *, const char *, uint32_t, const void *, const void *),
                       int (*body)(rayhip_ctx *, const VertexStamps &, uint32_t, const uint32_t *, const Record *)) {
    if (!c || use_device(c)) {
        return 1;
    }
    if (const int rc = possible(c, who, n, slots, records)) {
        return rc;
    }
    if (n == 0) {
        return 0;
    }
    const VertexStamps st{c, who};
    HIP_TRY(hipStreamSynchronize(c->stream)); // pending passes read the old arrays
    HIP_TRY(st.stamp("begin"));
    if (!host_args) {
        return body(c, st, n, slots, records);
    }
    DevBuf &args = c->*host_args;
    static_assert(RecordBytes % 4 == 0, "the slots lie behind the records");
    if (args.alloc(size_t(n) * (RecordBytes + 4))) {
        return 1;
    }
    Record *d_records = args.as<Record>();
    uint32_t *d_slots = reinterpret_cast<uint32_t *>(args.as<uint8_t>() + size_t(n) * RecordBytes);
    HIP_TRY(hipMemcpyAsync(d_records, records, size_t(n) * RecordBytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_slots, slots, size_t(n) * 4, hipMemcpyHostToDevice, c->stream));
    return body(c, st, n, d_slots, d_records);
}

// ---- moving instances: transforms in, inverses and world boxes on the device, the top level rebuilt (instances.h, instances.hip.h) ----
// Meshes, trees, materials, skins, morph sets and normal sets live in object space and stay.  k_pose_instances stages the new records
// and counts what is wrong with the call; only when its counters came back zero are the records scattered into the instance array
// (k_commit_instances), the boxes of EVERY live slot recomputed from the root nodes as they are on the device now (k_instance_boxes: a
// deformed mesh moves with its deformed box), the lights re-placed when a named slot carries some (the switch is on, or the call was
// refused), and the top level rebuilt by the path of the vertex update.  The kernels are tiny: the call is bound by its launches, its
// two read-backs and the top-level build.
// `d_slots` / `d_xforms`: device memory, complete and stable until the call returns.
static int set_instance_transforms(rayhip_ctx *c, const VertexStamps &st, const uint32_t n, const uint32_t *d_slots, const float *d_xforms) {
    namespace ri = rayhip_instances;
    rayhip_ctx::Refit &r = c->refit;
    hipStream_t s = c->stream;
    const uint32_t n_live = uint32_t(r.live.size());
    // one block, read back in one copy: [n] staged records of 128 bytes, [n_live] boxes of 24 bytes, [n] slots
    const size_t boxes_at = size_t(n) * 128, slots_at = (boxes_at + size_t(n_live) * 24 + 15) & ~size_t(15), stage_bytes = slots_at + size_t(n) * 4;
    if (c->instance_stage.alloc(stage_bytes) || c->instance_counters.alloc(8 * sizeof(uint32_t))) {
        return 1;
    }
    float4 *d_staged = c->instance_stage.as<float4>();
    float *d_boxes = reinterpret_cast<float *>(c->instance_stage.as<uint8_t>() + boxes_at);
    uint32_t *d_staged_slots = reinterpret_cast<uint32_t *>(c->instance_stage.as<uint8_t>() + slots_at);
    uint32_t *d_counters = c->instance_counters.as<uint32_t>(); // ([N_FINDINGS]: triangle lights without area)
    rayhip_mesh_instance *d_instances = c->mesh_instances.as<rayhip_mesh_instance>();
    HIP_TRY(hipMemsetAsync(d_counters, 0, 8 * sizeof(uint32_t), s));
    if (!r.slot_flags.empty()) {
        HIP_TRY(hipMemsetAsync(r.d_slot_claim.p, 0, r.slot_flags.size() * sizeof(uint32_t), s));
    }
    ri::k_pose_instances<<<blocks_of(n), 256, 0, s>>>(d_slots, d_xforms, n, (reinterpret_cast<uintptr_t>(d_xforms) & 15u) == 0u, r.d_slot_flags.as<uint8_t>(),
                                                      r.d_slot_claim.as<uint32_t>(), d_instances, c->instances_count, !c->light_refit.on, d_staged,
                                                      d_staged_slots, d_counters);
    HIP_TRY(hipGetLastError());
    uint32_t findings[ri::N_FINDINGS] = {};
    HIP_TRY(hipMemcpyAsync(findings, d_counters, sizeof(findings), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (findings[ri::BAD_SLOT] != 0) {
        return fail("%s: %u of the slots are outside the %u instance slots, or not in the top level", st.who, findings[ri::BAD_SLOT], c->instances_count);
    }
    if (findings[ri::DUPLICATE] != 0) {
        return fail("%s: %u slots are named more than once", st.who, findings[ri::DUPLICATE]);
    }
    if (findings[ri::NOT_FINITE] != 0) {
        return fail("%s: %u transforms have an element that is not finite, or an inverse that has one (a singular matrix)", st.who, findings[ri::NOT_FINITE]);
    }
    if (findings[ri::PINNED] != 0) {
        (void)fail("%s: %u of the slots carry triangle lights; lights are not rebuilt by this call (rayhip_scene_refit_lights)", st.who, findings[ri::PINNED]);
        return 2;
    }
    // (the counters are back and zero: from here on the live instance array is written)
    ri::k_commit_instances<<<blocks_of(n), 256, 0, s>>>(d_staged, d_staged_slots, n, d_instances, c->instances_count);
    HIP_TRY(hipGetLastError());
    if (n_live) {
        ri::k_instance_boxes<<<blocks_of(n_live), 256, 0, s>>>(r.d_live.as<uint32_t>(), n_live, d_instances, c->instances_count, c->nodes.as<rayhip_bvh2_node>(),
                                                               c->nodes_used, d_boxes);
        HIP_TRY(hipGetLastError());
    }
    std::vector<uint8_t> back(stage_bytes);
    HIP_TRY(hipMemcpyAsync(back.data(), c->instance_stage.p, stage_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(st.stamp("instances posed"));
    // the host's copy of the instance array follows: the source of the direct entry's arguments and of a later vertex update's boxes
    bool lights_moved = false;
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t slot = 0;
        memcpy(&slot, back.data() + slots_at + size_t(i) * 4, sizeof(slot));
        memcpy(r.instances[slot].xform, back.data() + size_t(i) * 128, 128); // (xform and inv_xform lie side by side)
        lights_moved = lights_moved || (r.slot_flags[slot] & ri::SLOT_TRI_LIGHTS) != 0;
    }
    if (lights_moved && c->light_refit.on) { // the triangle lights are re-placed by the instance array that is on the device now
        if (refit_lights(c, d_counters + ri::N_FINDINGS, st)) {
            return 1;
        }
        HIP_TRY(hipMemcpyAsync(&c->light_refit.degenerate, d_counters + ri::N_FINDINGS, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    rayhip_update::Plan up;
    up.live = r.live;
    up.boxes.resize(n_live);
    if (n_live) {
        memcpy(up.boxes.data(), back.data() + boxes_at, size_t(n_live) * sizeof(rayhip_lbvh::Box));
    }
    return rebuild_top_level_behind(c, up, st);
}

// what both forms check before anything else: 0 = go on, 1 / 2 = the return code
static int instance_move_possible(rayhip_ctx *c, const char *who, const uint32_t n, const void *slots, const void *xforms) {
    if (const int rc = scene_change_possible(c, who, n > 0 && (!slots || !xforms), true)) {
        return rc;
    }
    if (c->refit.slot_flags.size() != c->instances_count || c->refit.instances.size() != c->instances_count) { // (an upload that failed half-way)
        (void)fail("%s: the tables of the last upload are incomplete", who);
        return 2;
    }
    if (c->light_refit.on && !c->light_refit.ready) {
        return fail("%s: rayhip_scene_refit_lights is on, but its tables are not prepared", who);
    }
    return 0;
}

int rayhip_scene_set_instance_transforms(rayhip_ctx *c, uint32_t n, const uint32_t *slots, const float *xforms) {
    return set_records<float, 64>(c, "rayhip_scene_set_instance_transforms", n, slots, xforms, &rayhip_ctx::instance_args, instance_move_possible, set_instance_transforms);
}

int rayhip_scene_set_instance_transforms_device(rayhip_ctx *c, uint32_t n, const uint32_t *device_slots, const float *device_xforms) {
    return set_records<float, 64>(c, "rayhip_scene_set_instance_transforms_device", n, device_slots, device_xforms, nullptr, instance_move_possible, set_instance_transforms);
}

// ---- analytic lights that move or change colour: records in, leaf summaries on the device, the light tree refitted (light_pose.h) ----
// Sphere, spot, directional, line, rect and disk lights.  k_pose_lights stages the new records with their summaries and counts what is
// wrong with the call; only when its counters came back zero are they scattered into the light array and the leaf table of the light
// refit (k_commit_lights, which also marks the slots in `posed`), and the tree is refitted by the level launches of the vertex update:
// boxes, quantised child boxes, flux, cones and light_children rows.  The triangle lights' corners and summaries are where the last
// refit left them -- no record of theirs changes here, so no pass over them but the first.  The call is bound by its launches and its
// one read-back.
// `d_slots` / `d_records`: device memory, complete and stable until the call returns.
static int set_lights(rayhip_ctx *c, const VertexStamps &st, const uint32_t n, const uint32_t *d_slots, const rayhip_light *d_records) {
    namespace lp = rayhip_light_pose;
    rayhip_ctx::LightRefit &lr = c->light_refit;
    hipStream_t s = c->stream;
    // one block: [n] staged records of 64 bytes, [n] summaries of 48 bytes, [n] slots
    const size_t leaf_at = size_t(n) * 64, slots_at = leaf_at + size_t(n) * 48;
    if (c->light_stage.alloc(slots_at + size_t(n) * 4) || c->light_counters.alloc(8 * sizeof(uint32_t))) {
        return 1;
    }
    float4 *d_staged = c->light_stage.as<float4>();
    float4 *d_staged_leaf = reinterpret_cast<float4 *>(c->light_stage.as<uint8_t>() + leaf_at);
    uint32_t *d_staged_slots = reinterpret_cast<uint32_t *>(c->light_stage.as<uint8_t>() + slots_at);
    uint32_t *d_counters = c->light_counters.as<uint32_t>();
    HIP_TRY(hipMemsetAsync(d_counters, 0, 8 * sizeof(uint32_t), s));
    if (lr.lights_count) {
        HIP_TRY(hipMemsetAsync(lr.claim.p, 0, size_t(lr.lights_count) * sizeof(uint32_t), s));
    }
    lp::k_pose_lights<<<blocks_of(n), 256, 0, s>>>(d_slots, d_records, n, (reinterpret_cast<uintptr_t>(d_records) & 15u) == 0u, c->lights.as<rayhip_light>(),
                                                   lr.lights_count, lr.live.as<uint8_t>(), lr.claim.as<uint32_t>(), d_staged, d_staged_leaf, d_staged_slots,
                                                   d_counters);
    HIP_TRY(hipGetLastError());
    uint32_t findings[lp::N_FINDINGS] = {};
    HIP_TRY(hipMemcpyAsync(findings, d_counters, sizeof(findings), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(st.stamp("lights checked"));
    if (findings[lp::BAD_SLOT] != 0) {
        return fail("%s: %u of the slots are outside the %u light slots, or not named by li_indices", st.who, findings[lp::BAD_SLOT], lr.lights_count);
    }
    if (findings[lp::DUPLICATE] != 0) {
        return fail("%s: %u slots are named more than once", st.who, findings[lp::DUPLICATE]);
    }
    if (findings[lp::BAD_TYPE] != 0) {
        return fail("%s: %u of the held or new records are triangle or environment lights", st.who, findings[lp::BAD_TYPE]);
    }
    if (findings[lp::FLAGS_CHANGED] != 0) {
        return fail("%s: word 0 of %u records (type and flags) differs from the one the slot holds", st.who, findings[lp::FLAGS_CHANGED]);
    }
    if (findings[lp::NOT_FINITE] != 0) {
        return fail("%s: %u records have a colour or a parameter that is not finite", st.who, findings[lp::NOT_FINITE]);
    }
    // (the counters are back and zero: from here on the live light arrays are written)
    lp::k_commit_lights<<<blocks_of(n), 256, 0, s>>>(d_staged, d_staged_leaf, d_staged_slots, n, c->lights.as<rayhip_light>(),
                                                     lr.leaf.as<rayhip_light_refit::Summary>(), lr.posed.as<uint8_t>(), lr.lights_count);
    HIP_TRY(hipGetLastError());
    HIP_TRY(st.stamp("lights committed"));
    // the level launches read the summary of EVERY leaf.  Those of the triangle lights are written by the first pass over them, not when
    // the tables are prepared: where none ran yet it runs here (corners and summaries of the pose that is on the device, the bytes a
    // vertex update would write); afterwards no record of theirs changes in this call, and the tree alone is refitted
    if (!lr.tri_leaves) {
        if (refit_lights(c, d_counters + lp::N_FINDINGS, st)) {
            return 1;
        }
        HIP_TRY(hipMemcpyAsync(&lr.degenerate, d_counters + lp::N_FINDINGS, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    } else if (refit_light_levels(c)) {
        return 1;
    }
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(st.stamp("light tree refitted"));
    return 0;
}

// what both forms check before anything else: 0 = go on, 1 / 2 = the return code
static int light_move_possible(rayhip_ctx *c, const char *who, const uint32_t n, const void *slots, const void *records) {
    if (const int rc = scene_change_possible(c, who, n > 0 && (!slots || !records), false)) { // (no tree of the geometry is rebuilt)
        return rc;
    }
    if (!c->light_refit.on || !c->light_refit.ready) {
        (void)fail("%s: rayhip_scene_refit_lights is off, or its tables are not prepared; the switch keeps the light tree refittable", who);
        return 2;
    }
    return 0;
}

int rayhip_scene_set_lights(rayhip_ctx *c, uint32_t n, const uint32_t *slots, const rayhip_light *records) {
    return set_records(c, "rayhip_scene_set_lights", n, slots, records, &rayhip_ctx::light_args, light_move_possible, set_lights);
}

int rayhip_scene_set_lights_device(rayhip_ctx *c, uint32_t n, const uint32_t *device_slots, const rayhip_light *device_records) {
    return set_records(c, "rayhip_scene_set_lights_device", n, device_slots, device_records, nullptr, light_move_possible, set_lights);
}

// ---- materials that change: records in, the triangle lights they colour recoloured, the light tree refitted (materials.h) ------------
// The node graph stays (type, flags, textures), so everything an upload derives from the materials stays valid.  k_check_materials
// stages the new records and counts what is wrong with the call; only when its counters came back clean are the records scattered into
// the material array (k_commit_materials).  Where a named material is the emitter of triangle lights -- whether its colour changed or
// not: an instance update may have brought other colours since -- the lights take base_color * strength of the committed record
// (k_recolour_tri_lights) and the light refit runs as it is behind a vertex update: summaries with the new flux, then the level
// launches.  A call that names no emitter launches nothing over the light arrays.  Bound by its launches and its one read-back.
// `d_slots` / `d_records`: device memory, complete and stable until the call returns, 4-byte aligned.
static int set_materials(rayhip_ctx *c, const VertexStamps &st, const uint32_t n, const uint32_t *d_slots, const rayhip_material *d_records) {
    namespace rm = rayhip_materials;
    rayhip_ctx::MaterialChecks &mc = c->material_checks;
    rayhip_ctx::LightRefit &lr = c->light_refit;
    hipStream_t s = c->stream;
    const uint32_t n_materials = c->geometry.materials;
    // one block: [n] staged records of 76 bytes, [n] slots
    const size_t slots_at = size_t(n) * sizeof(rayhip_material);
    if (c->material_stage.alloc(slots_at + size_t(n) * 4) || c->material_counters.alloc(16 * sizeof(uint32_t))) {
        return 1;
    }
    uint32_t *d_staged = c->material_stage.as<uint32_t>();
    uint32_t *d_staged_slots = reinterpret_cast<uint32_t *>(c->material_stage.as<uint8_t>() + slots_at);
    uint32_t *d_counters = c->material_counters.as<uint32_t>(); // ([N_COUNTERS]: triangle lights without area)
    const bool refittable = lr.on && lr.ready;
    HIP_TRY(hipMemsetAsync(d_counters, 0, 16 * sizeof(uint32_t), s));
    HIP_TRY(hipMemsetAsync(mc.d_claim.p, 0, size_t(n_materials) * sizeof(uint32_t), s));
    rm::k_check_materials<<<blocks_of(n), 256, 0, s>>>(d_slots, reinterpret_cast<const uint32_t *>(d_records), n, c->materials.as<rayhip_material>(), n_materials,
                                                       mc.d_flags.as<uint8_t>(), mc.d_claim.as<uint32_t>(), c->plain_ior, refittable, d_staged, d_staged_slots,
                                                       d_counters);
    HIP_TRY(hipGetLastError());
    uint32_t counters[rm::N_COUNTERS] = {};
    HIP_TRY(hipMemcpyAsync(counters, d_counters, sizeof(counters), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(st.stamp("materials checked"));
    if (counters[rm::BAD_SLOT] != 0) {
        return fail("%s: %u of the slots are outside the %u material slots, or used by no triangle of the scene", st.who, counters[rm::BAD_SLOT], n_materials);
    }
    if (counters[rm::DUPLICATE] != 0) {
        return fail("%s: %u slots are named more than once", st.who, counters[rm::DUPLICATE]);
    }
    if (counters[rm::GRAPH_CHANGED] != 0) {
        return fail("%s: type, flags or a texture word of %u records differ from those the slot holds", st.who, counters[rm::GRAPH_CHANGED]);
    }
    if (counters[rm::NOT_FINITE] != 0) {
        return fail("%s: %u records have a colour, a strength or an ior that is not finite", st.who, counters[rm::NOT_FINITE]);
    }
    if (counters[rm::NEGATIVE] != 0) {
        return fail("%s: %u emissive records have a negative colour or strength", st.who, counters[rm::NEGATIVE]);
    }
    if (counters[rm::REFRACTS] != 0) {
        (void)fail("%s: %u records refract, and the uploaded scene had no refractive surface: its passes do not carry the rays' ior stacks", st.who,
                   counters[rm::REFRACTS]);
        return 2;
    }
    if (counters[rm::PINNED] != 0) {
        (void)fail("%s: %u of the materials colour triangle lights; lights are not rebuilt by this call (rayhip_scene_refit_lights)", st.who, counters[rm::PINNED]);
        return 2;
    }
    // (the counters are back and clean: from here on the live material array is written)
    rm::k_commit_materials<<<blocks_of(size_t(n) * rm::RECORD_WORDS), 256, 0, s>>>(d_staged, d_staged_slots, n, c->materials.as<uint32_t>(), n_materials);
    HIP_TRY(hipGetLastError());
    HIP_TRY(st.stamp("materials committed"));
    if (counters[rm::EMITTERS_NAMED] != 0 && refittable && lr.lights_count != 0) {
        rm::k_recolour_tri_lights<<<blocks_of(lr.lights_count), 256, 0, s>>>(c->lights.as<rayhip_light>(), lr.lights_count, mc.d_light_emitter.as<uint16_t>(),
                                                                             mc.d_claim.as<uint32_t>(), c->materials.as<rayhip_material>(), n_materials);
        HIP_TRY(hipGetLastError());
        HIP_TRY(st.stamp("lights recoloured"));
        if (refit_lights(c, d_counters + rm::N_COUNTERS, st)) {
            return 1;
        }
        HIP_TRY(hipMemcpyAsync(&lr.degenerate, d_counters + rm::N_COUNTERS, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

// what both forms check before anything else: 0 = go on, 1 / 2 = the return code
static int material_change_possible(rayhip_ctx *c, const char *who, const uint32_t n, const void *slots, const void *records) {
    if (const int rc = scene_change_possible(c, who, n > 0 && (!slots || !records), false)) { // (no tree of the geometry is rebuilt)
        return rc;
    }
    if (c->material_checks.flags.size() != c->geometry.materials) { // (an upload that failed half-way)
        (void)fail("%s: the tables of the last upload are incomplete", who);
        return 2;
    }
    return 0;
}

int rayhip_scene_set_materials(rayhip_ctx *c, uint32_t n, const uint32_t *slots, const rayhip_material *records) {
    return set_records(c, "rayhip_scene_set_materials", n, slots, records, &rayhip_ctx::material_args, material_change_possible, set_materials);
}

int rayhip_scene_set_materials_device(rayhip_ctx *c, uint32_t n, const uint32_t *device_slots, const rayhip_material *device_records) {
    return set_records(c, "rayhip_scene_set_materials_device", n, device_slots, device_records, nullptr, material_change_possible, set_materials);
}

// ---- handles over vertex ranges: what creating and destroying a skin, a morph set and a normal set share ----------------------------
// (the records and their tables: rayhip_ctx::RangeHead, RangeTable.)  A create asks, in this order: its pointers; the context and the
// range (range_possible); what only its kind knows of the description's sizes; a free slot clear of the live records
// (RangeTable::free_slot); the description's arrays; the pinned light vertices (range_not_pinned) -- and issues the handle
// (RangeTable::issue) when its tables are on the device.  A destroy is RangeTable::destroy.
static int range_possible(rayhip_ctx *c, const char *who, const uint32_t first, const uint32_t count) {
    if (const int rc = vertex_update_possible(c, who)) {
        return rc;
    }
    if (count == 0 || uint64_t(first) + count > c->geometry.vertices) {
        return outside_the_scene(c, who, first, count);
    }
    return 0;
}

// `mover`: what would move the vertices of the range -- it may put them anywhere
static int range_not_pinned(rayhip_ctx *c, const char *who, const uint32_t first, const uint32_t count, const char *mover) {
    if (const uint32_t *pinned = pinned_light_vertex(c, first, count, nullptr)) {
        (void)fail("%s: vertex %u belongs to a triangle light; lights are not rebuilt by %s", who, *pinned, mover);
        return 2;
    }
    return 0;
}

// ---- the skins ---------------------------------------------------------------------------------------------------------------------------
int rayhip_skin_create(rayhip_ctx *c, const rayhip_skin_desc *d, int *out_skin) {
    if (!c || use_device(c)) {
        return 1;
    }
    if (!d || !out_skin || !d->bone_indices || !d->bone_weights) {
        return fail("rayhip_skin_create: a null pointer");
    }
    if (const int rc = range_possible(c, "rayhip_skin_create", d->first_vertex, d->count)) {
        return rc;
    }
    if (d->bones_count == 0 || d->bones_count > 65536u) {
        return fail("rayhip_skin_create: %u bones (bone indices are 16-bit)", d->bones_count);
    }
    int slot = -1;
    if (c->skins.free_slot("rayhip_skin_create", d->first_vertex, d->count, slot)) {
        return 1;
    }
    {
        uint32_t where = 0;
        if (const int bad = rayhip_skin::validate_influences(d->bone_indices, d->bone_weights, d->count, d->bones_count, where)) {
            return bad == 1 ? fail("rayhip_skin_create: vertex %u names a bone outside the palette of %u", d->first_vertex + where, d->bones_count)
                            : fail("rayhip_skin_create: a weight of vertex %u is negative or not finite", d->first_vertex + where);
        }
    }
    if (const int rc = range_not_pinned(c, "rayhip_skin_create", d->first_vertex, d->count, "a pose")) {
        return rc;
    }
    rayhip_ctx::Skin &k = c->skins.slots[slot];
    const size_t n = d->count;
    if (k.rest.alloc(n * sizeof(rayhip_vertex)) || upload(c, k.indices, d->bone_indices, n * 4 * sizeof(uint16_t)) ||
        upload(c, k.weights, d->bone_weights, n * 4 * sizeof(float))) {
        return 1;
    }
    HIP_TRY(hipMemcpyAsync(k.rest.p, d->rest ? static_cast<const void *>(d->rest) : static_cast<const void *>(c->vertices.as<rayhip_vertex>() + d->first_vertex),
                           n * sizeof(rayhip_vertex), d->rest ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream)); // the caller's arrays may go away after this call
    k.bones_count = d->bones_count;
    *out_skin = c->skins.issue(slot, d->first_vertex, d->count);
    return 0;
}

int rayhip_skin_destroy(rayhip_ctx *c, int skin) { return !c || use_device(c) ? 1 : c->skins.destroy(c->stream, "rayhip_skin_destroy", skin); }

// ---- morph sets (morph.h, morph.hip.h) ------------------------------------------------------------------------------------------------------
int rayhip_morph_create(rayhip_ctx *c, const rayhip_morph_desc *d, int *out_morph) {
    if (!c || use_device(c)) {
        return 1;
    }
    if (!d || !out_morph || !d->targets) {
        return fail("rayhip_morph_create: a null pointer");
    }
    if (const int rc = range_possible(c, "rayhip_morph_create", d->first_vertex, d->count)) {
        return rc;
    }
    if (d->targets_count == 0 || d->targets_count > rayhip_morph::MAX_TARGETS) {
        return fail("rayhip_morph_create: %u targets (1 .. %u)", d->targets_count, rayhip_morph::MAX_TARGETS);
    }
    int slot = -1;
    if (c->morphs.free_slot("rayhip_morph_create", d->first_vertex, d->count, slot)) {
        return 1;
    }
    {
        uint32_t where = 0;
        if (const int bad = rayhip_morph::validate_targets(d->targets, d->targets_count, d->count, where)) {
            return bad == 1   ? fail("rayhip_morph_create: a null pointer in target %u", where)
                   : bad == 2 ? fail("rayhip_morph_create: the vertices of target %u are not strictly ascending below %u", where, d->count)
                   : bad == 3 ? fail("rayhip_morph_create: a delta of target %u is not finite", where)
                              : fail("rayhip_morph_create: more than 2^32 - 1 entries in all");
        }
    }
    if (const int rc = range_not_pinned(c, "rayhip_morph_create", d->first_vertex, d->count, "a pose")) {
        return rc;
    }
    std::vector<uint32_t> row;
    std::vector<rayhip_morph::Entry> entries;
    rayhip_morph::build_rows(d->targets, d->targets_count, d->count, row, entries);
    rayhip_ctx::Morph &m = c->morphs.slots[slot];
    const size_t n = d->count;
    if (m.base.alloc(n * sizeof(rayhip_vertex)) || upload(c, m.row, row.data(), row.size() * sizeof(uint32_t)) ||
        upload(c, m.entries, entries.data(), entries.size() * sizeof(rayhip_morph::Entry))) {
        return 1;
    }
    HIP_TRY(hipMemcpyAsync(m.base.p, d->base ? static_cast<const void *>(d->base) : static_cast<const void *>(c->vertices.as<rayhip_vertex>() + d->first_vertex),
                           n * sizeof(rayhip_vertex), d->base ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream)); // the table and the caller's arrays may go away after this call
    m.targets_count = d->targets_count;
    *out_morph = c->morphs.issue(slot, d->first_vertex, d->count);
    return 0;
}

int rayhip_morph_destroy(rayhip_ctx *c, int morph) { return !c || use_device(c) ? 1 : c->morphs.destroy(c->stream, "rayhip_morph_destroy", morph); }

// ---- normal sets (normals.h, normals.hip.h) ---------------------------------------------------------------------------------------------------
// The topology is read back once, here: the nodes, the entry table and the indices as they are on the device (the leaf refinement of an
// upload changed the first two; the faces of a set are the triangles the device's own trees reach).
int rayhip_normals_create(rayhip_ctx *c, const rayhip_normals_desc *d, int *out_set) {
    if (!c || use_device(c)) {
        return 1;
    }
    if (!d || !out_set) {
        return fail("rayhip_normals_create: a null pointer");
    }
    if (const int rc = range_possible(c, "rayhip_normals_create", d->first_vertex, d->count)) {
        return rc;
    }
    int slot = -1;
    if (c->normal_sets.free_slot("rayhip_normals_create", d->first_vertex, d->count, slot)) {
        return 1;
    }
    {
        uint32_t where = 0;
        if (const int bad = rayhip_normals::validate_desc(d->count, d->flags, d->weld, where)) {
            return bad == 1   ? fail("rayhip_normals_create: flags %u (RAYHIP_NORMALS_N | RAYHIP_NORMALS_B, at least one)", d->flags)
                   : bad == 2 ? fail("rayhip_normals_create: the weld index of vertex %u is outside the range of %u", d->first_vertex + where, d->count)
                              : fail("rayhip_normals_create: the weld index of vertex %u is not canonical (weld[weld[i]] != weld[i])", d->first_vertex + where);
        }
    }
    if (const int rc = range_not_pinned(c, "rayhip_normals_create", d->first_vertex, d->count, "a recompute")) {
        return rc;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<rayhip_bvh2_node> nodes(c->nodes_used);
    std::vector<uint32_t> tri_indices(c->refit.entries), vtx_indices(c->geometry.vtx_indices);
    if (!read_back(nodes.data(), c->nodes, nodes.size() * sizeof(rayhip_bvh2_node)) ||
        !read_back(tri_indices.data(), c->tri_indices, tri_indices.size() * sizeof(uint32_t)) ||
        !read_back(vtx_indices.data(), c->vtx_indices, vtx_indices.size() * sizeof(uint32_t))) {
        return fail("rayhip_normals_create: reading the topology back failed");
    }
    std::vector<uint32_t> reachable;
    if (!rayhip_normals::reachable_triangles(nodes.data(), uint32_t(nodes.size()), c->refit.roots.data(), c->refit.roots.size(), tri_indices.data(),
                                             uint32_t(tri_indices.size()), vtx_indices.data(), uint32_t(vtx_indices.size() / 3), c->geometry.vertices, reachable)) {
        return fail("rayhip_normals_create: a bottom-level tree on the device is malformed");
    }
    rayhip_normals::Tables tb;
    if (rayhip_normals::build_rows(reachable.data(), reachable.size(), vtx_indices.data(), d->first_vertex, d->count,
                                   (d->flags & RAYHIP_NORMALS_N) ? d->weld : nullptr, tb)) {
        return fail("rayhip_normals_create: more than 2^32 - 1 row entries");
    }
    rayhip_ctx::Normals &n = c->normal_sets.slots[slot];
    const bool welded = !tb.wrow.empty();
    if (upload(c, n.faces, tb.faces.data(), tb.faces.size() * sizeof(uint32_t)) || upload(c, n.row, tb.row.data(), tb.row.size() * sizeof(uint32_t)) ||
        upload(c, n.entries, tb.entries.data(), tb.entries.size() * sizeof(uint32_t)) ||
        (welded && (upload(c, n.wrow, tb.wrow.data(), tb.wrow.size() * sizeof(uint32_t)) ||
                    upload(c, n.wentries, tb.wentries.data(), tb.wentries.size() * sizeof(uint32_t)))) ||
        n.frames.alloc(tb.faces.size() * sizeof(rayhip_normals::FaceFrame))) {
        n.release();
        return 1;
    }
    HIP_TRY(hipStreamSynchronize(c->stream)); // the tables go out of scope
    n.flags = d->flags, n.faces_count = uint32_t(tb.faces.size()), n.welded = welded;
    *out_set = c->normal_sets.issue(slot, d->first_vertex, d->count);
    return 0;
}

int rayhip_normals_destroy(rayhip_ctx *c, int set) { return !c || use_device(c) ? 1 : c->normal_sets.destroy(c->stream, "rayhip_normals_destroy", set); }

// ---- the poses (rayhip_scene_pose_skins, rayhip_scene_pose): morph sets and skins posed into a staging array, then ONE refit -------------
// vertices [first, first + count) of the scene, posed into the staging array from record `at` on
struct StagedRange {
    uint32_t first, count;
    size_t at;
};

// k_skin_vertices over vertices [off, off + count) of skin `k` (its pointers offset: 8-byte index records and 16-byte weight records stay
// aligned at any vertex), posed into the staging array where the skin's range begins at record `at`
static int launch_skin_segment(rayhip_ctx *c, const rayhip_ctx::Skin &k, const uint32_t off, const uint32_t count, const float *d_palette, const size_t at) {
    if (count == 0) {
        return 0;
    }
    rayhip_skin::k_skin_vertices<<<blocks_of(count), 256, 0, c->stream>>>(k.rest.as<rayhip_vertex>() + off, k.indices.as<uint16_t>() + size_t(off) * 4,
                                                                          k.weights.as<float>() + size_t(off) * 4, count, d_palette, k.bones_count,
                                                                          c->refit.d_vertex_used.as<uint8_t>() + k.first + off,
                                                                          c->skin_stage.as<rayhip_vertex>() + at + off, c->skin_counters.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    return 0;
}

// Morph sets and skins in one pose.  A skin's range is staged as a sequence of launches over segments -- [plain][set A][plain][set B]... --
// plain ones by k_skin_vertices with its pointers offset, covered ones by the fused kernel: no kernel looks for the set it is in.
// The entry points have checked the counts and the outer pointers and asked vertex_update_possible, each in its own order.
// `who`: the entry point the texts and stamps name; `together`: how its text tells the caller to pose a skin with the sets it holds.
static int pose_ranges(rayhip_ctx *c, const char *who, const char *together, const int n_morphs, const int *morphs, const float *const *weights, const int n_skins,
                       const int *skins, const float *const *palettes) {
    size_t stage_vertices = 0, floats = 0;
    for (int i = 0; i < n_morphs; ++i) {
        const rayhip_ctx::Morph *m = c->morphs.of(morphs[i]);
        if (!m) {
            (void)fail("%s: morph set %d is not live", who, morphs[i]);
            return 2;
        }
        if (!weights[i]) {
            return fail("%s: no weights for morph set %d", who, morphs[i]);
        }
        for (int j = 0; j < i; ++j) {
            if (morphs[j] == morphs[i]) {
                return fail("%s: morph set %d is named twice", who, morphs[i]);
            }
        }
        for (uint32_t t = 0; t < m->targets_count; ++t) {
            if (!rayhip_skin::finite_f(weights[i][t])) {
                return fail("%s: the weight of target %u of morph set %d is not finite", who, t, morphs[i]);
            }
        }
        floats += m->targets_count;
    }
    for (int i = 0; i < n_skins; ++i) {
        if (!c->skins.of(skins[i])) {
            (void)fail("%s: skin %d is not live", who, skins[i]);
            return 2;
        }
        if (!palettes[i]) {
            return fail("%s: no palette for skin %d", who, skins[i]);
        }
        for (int j = 0; j < i; ++j) {
            if (skins[j] == skins[i]) {
                return fail("%s: skin %d is named twice", who, skins[i]);
            }
        }
        stage_vertices += c->skins.of(skins[i])->count, floats += size_t(c->skins.of(skins[i])->bones_count) * 12;
    }
    const auto named = [](const int *ids, const int n, const int id) { return std::find(ids, ids + n, id) != ids + n; };
    const auto overlap = [](const rayhip_ctx::Morph &m, const rayhip_ctx::Skin &k) { return m.first < k.first + k.count && k.first < m.first + m.count; };
    std::vector<bool> in_a_skin(size_t(n_morphs), false);
    for (int i = 0; i < n_morphs; ++i) {
        const rayhip_ctx::Morph &m = *c->morphs.of(morphs[i]);
        for (const rayhip_ctx::Skin &k : c->skins) {
            if (!k.live || !overlap(m, k)) {
                continue;
            }
            if (m.first < k.first || m.first + m.count > k.first + k.count) {
                return fail("%s: morph set %d straddles the boundary of skin %d", who, m.id, k.id);
            }
            if (!named(skins, n_skins, k.id)) {
                return fail("%s: morph set %d lies inside skin %d; pose them together", who, m.id, k.id);
            }
            in_a_skin[size_t(i)] = true;
        }
        stage_vertices += in_a_skin[size_t(i)] ? 0 : m.count;
    }
    for (int i = 0; i < n_skins; ++i) {
        const rayhip_ctx::Skin &k = *c->skins.of(skins[i]);
        for (const rayhip_ctx::Morph &m : c->morphs) {
            if (m.live && overlap(m, k) && !named(morphs, n_morphs, m.id)) {
                return fail("%s: skin %d holds morph set %d; %s", who, k.id, m.id, together);
            }
        }
    }
    if (n_morphs == 0 && n_skins == 0) {
        return 0;
    }
    const VertexStamps st{c, who};
    HIP_TRY(hipStreamSynchronize(c->stream)); // pending passes read the old arrays
    HIP_TRY(st.stamp("begin"));
    // room: the staged records, the palettes and weights, the counters (zeroed)
    if (c->skin_stage.alloc(stage_vertices * sizeof(rayhip_vertex)) || c->skin_palettes.alloc(floats * sizeof(float)) || c->skin_counters.alloc(2 * sizeof(uint32_t))) {
        return 1;
    }
    hipStream_t s = c->stream;
    uint32_t *d_counters = c->skin_counters.as<uint32_t>();
    HIP_TRY(hipMemsetAsync(d_counters, 0, 2 * sizeof(uint32_t), s));
    const uint8_t *d_used = c->refit.d_vertex_used.as<uint8_t>();
    std::vector<StagedRange> staged;
    size_t at_vertex = 0, at_float = 0;
    std::vector<const float *> d_weights(size_t(n_morphs), nullptr);
    for (int i = 0; i < n_morphs; ++i) {
        const rayhip_ctx::Morph &m = *c->morphs.of(morphs[i]);
        float *d_w = c->skin_palettes.as<float>() + at_float;
        HIP_TRY(hipMemcpyAsync(d_w, weights[i], size_t(m.targets_count) * sizeof(float), hipMemcpyHostToDevice, s));
        d_weights[size_t(i)] = d_w, at_float += m.targets_count;
    }
    for (int i = 0; i < n_skins; ++i) {
        const rayhip_ctx::Skin &k = *c->skins.of(skins[i]);
        float *d_palette = c->skin_palettes.as<float>() + at_float;
        HIP_TRY(hipMemcpyAsync(d_palette, palettes[i], size_t(k.bones_count) * 12 * sizeof(float), hipMemcpyHostToDevice, s));
        std::vector<int> inside; // the named sets this skin holds, by first vertex
        for (int j = 0; j < n_morphs; ++j) {
            if (overlap(*c->morphs.of(morphs[j]), k)) {
                inside.push_back(j);
            }
        }
        std::sort(inside.begin(), inside.end(), [&](const int x, const int y) { return c->morphs.of(morphs[x])->first < c->morphs.of(morphs[y])->first; });
        uint32_t at = 0; // vertices of the skin staged so far
        for (const int j : inside) {
            const rayhip_ctx::Morph &m = *c->morphs.of(morphs[j]);
            const uint32_t off = m.first - k.first;
            if (launch_skin_segment(c, k, at, off - at, d_palette, at_vertex)) {
                return 1;
            }
            rayhip_morph::k_morph_skin_vertices<<<blocks_of(m.count), 256, 0, s>>>(
                m.base.as<rayhip_vertex>(), m.row.as<uint32_t>(), m.entries.as<rayhip_morph::Entry>(), m.count, d_weights[size_t(j)], m.targets_count,
                k.indices.as<uint16_t>() + size_t(off) * 4, k.weights.as<float>() + size_t(off) * 4, d_palette, k.bones_count, d_used + m.first,
                c->skin_stage.as<rayhip_vertex>() + at_vertex + off, d_counters);
            HIP_TRY(hipGetLastError());
            at = off + m.count;
        }
        if (launch_skin_segment(c, k, at, k.count - at, d_palette, at_vertex)) {
            return 1;
        }
        staged.push_back({k.first, k.count, at_vertex});
        at_vertex += k.count, at_float += size_t(k.bones_count) * 12;
    }
    for (int i = 0; i < n_morphs; ++i) {
        if (in_a_skin[size_t(i)]) {
            continue;
        }
        const rayhip_ctx::Morph &m = *c->morphs.of(morphs[i]);
        rayhip_morph::k_morph_vertices<<<blocks_of(m.count), 256, 0, s>>>(m.base.as<rayhip_vertex>(), m.row.as<uint32_t>(), m.entries.as<rayhip_morph::Entry>(),
                                                                          m.count, d_weights[size_t(i)], m.targets_count, d_used + m.first,
                                                                          c->skin_stage.as<rayhip_vertex>() + at_vertex, d_counters);
        HIP_TRY(hipGetLastError());
        staged.push_back({m.first, m.count, at_vertex});
        at_vertex += m.count;
    }
    // behind the launches: the counter comes back; where it is zero the staged ranges are copied into the vertex array and ONE refit follows
    uint32_t counters[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(counters, d_counters, sizeof(counters), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s)); // (the caller's palettes and weights may go away after this)
    HIP_TRY(st.stamp("vertices posed"));
    if (counters[0] != 0) {
        return fail("%s: the posed position of %u vertices is not finite", who, counters[0]);
    }
    // (the counter is back and zero: from here on the live vertex array is written)
    for (const StagedRange &r : staged) {
        HIP_TRY(hipMemcpyAsync(c->vertices.as<rayhip_vertex>() + r.first, c->skin_stage.as<rayhip_vertex>() + r.at, size_t(r.count) * sizeof(rayhip_vertex),
                               hipMemcpyDeviceToDevice, s));
    }
    HIP_TRY(st.stamp("vertices copied"));
    return refit_after_vertices(c, st);
}

// skins alone: rayhip_scene_pose without morph sets, under its own name.  (It asks the context before it lets an empty call pass.)
int rayhip_scene_pose_skins(rayhip_ctx *c, int n, const int *skins, const float *const *palettes) {
    if (!c || use_device(c)) {
        return 1;
    }
    if (n < 0 || n > int(rayhip_skin::MAX_SKINS) || (n > 0 && (!skins || !palettes))) {
        return fail("rayhip_scene_pose_skins: bad arguments");
    }
    if (const int rc = vertex_update_possible(c, "rayhip_scene_pose_skins")) {
        return rc;
    }
    return pose_ranges(c, "rayhip_scene_pose_skins", "pose them together (rayhip_scene_pose)", 0, nullptr, nullptr, n, skins, palettes);
}

int rayhip_scene_pose(rayhip_ctx *c, int n_morphs, const int *morphs, const float *const *weights, int n_skins, const int *skins, const float *const *palettes) {
    if (!c || use_device(c)) {
        return 1;
    }
    if (n_morphs < 0 || n_morphs > int(rayhip_morph::MAX_MORPHS) || n_skins < 0 || n_skins > int(rayhip_skin::MAX_SKINS) ||
        (n_morphs > 0 && (!morphs || !weights)) || (n_skins > 0 && (!skins || !palettes))) {
        return fail("rayhip_scene_pose: bad arguments");
    }
    if (n_morphs == 0 && n_skins == 0) {
        return 0;
    }
    if (const int rc = vertex_update_possible(c, "rayhip_scene_pose")) {
        return rc;
    }
    return pose_ranges(c, "rayhip_scene_pose", "pose them together", n_morphs, morphs, weights, n_skins, skins, palettes);
}

// ---- the switch: vertex updates and poses may move triangle lights (light_refit.h) --------------------------------------------------
// A property of the context.  Whichever comes second of this call and the upload prepares the tables (prepare_light_refit): here from
// the light arrays read back, which hold the topology and the fluxes of the lights that are no triangles whatever refits ran before.
int rayhip_scene_refit_lights(rayhip_ctx *c, int on) {
    if (!c || use_device(c)) {
        return 1;
    }
    rayhip_ctx::LightRefit &lr = c->light_refit;
    if (!on) {
        if (!lr.on) {
            return 0;
        }
        for (const auto &[r, noun] : c->vertex_ranges()) { // (skins, morph sets, normal sets)
            for (const auto &kept : c->refit.light_vertices) {
                if (r->live && r->covers(kept.first)) {
                    return fail("rayhip_scene_refit_lights: %s %d covers vertex %u of a triangle light; destroy it first", noun, r->id, kept.first);
                }
            }
        }
        // from here on a changed light vertex is refused again: "changed" against what the lights on the device describe NOW
        if (c->have_scene && !c->refit.light_vertices.empty()) {
            HIP_TRY(hipStreamSynchronize(c->stream));
            std::vector<rayhip_vertex> now(c->geometry.vertices);
            HIP_TRY(hipMemcpy(now.data(), c->vertices.p, now.size() * sizeof(rayhip_vertex), hipMemcpyDeviceToHost));
            for (auto &kept : c->refit.light_vertices) {
                if (kept.first < now.size()) {
                    kept.second = now[kept.first];
                }
            }
            if (upload_vertex_checks(c, false)) {
                return 1;
            }
        }
        lr.on = false;
        return 0;
    }
    if (lr.on) {
        return 0;
    }
    if (c->have_scene && !lr.ready) {
        // everything the tables are made from, read back: the tree is the one the last upload or instance update brought (no refit ran
        // since: the switch was off).  The pose it describes is that of the KEPT light vertices -- taken from the host's arrays with the
        // tree, re-taken from the device when the switch went off, and unchangeable while it is off -- not necessarily what the vertex
        // array holds: an instance update that came while the switch was off left a deformed emitter where it was
        HIP_TRY(hipStreamSynchronize(c->stream));
        std::vector<rayhip_light> lights(lr.lights_count);
        std::vector<rayhip_light_cwbvh_node> nodes(lr.nodes_count);
        std::vector<uint32_t> li(lr.li_count), vi(c->geometry.vtx_indices);
        std::vector<rayhip_vertex> vertices(c->geometry.vertices);
        std::vector<rayhip_mesh_instance> instances(c->instances_count);
        if (!read_back(lights.data(), c->lights, lights.size() * sizeof(rayhip_light)) || !read_back(nodes.data(), c->light_cwnodes, nodes.size() * sizeof(rayhip_light_cwbvh_node)) ||
            !read_back(li.data(), c->li_indices, li.size() * sizeof(uint32_t)) || !read_back(vi.data(), c->vtx_indices, vi.size() * sizeof(uint32_t)) ||
            !read_back(vertices.data(), c->vertices, vertices.size() * sizeof(rayhip_vertex)) ||
            !read_back(instances.data(), c->mesh_instances, instances.size() * sizeof(rayhip_mesh_instance))) {
            return fail("rayhip_scene_refit_lights: reading the scene back failed");
        }
        for (const auto &kept : c->refit.light_vertices) {
            if (kept.first < vertices.size()) {
                vertices[kept.first] = kept.second;
            }
        }
        rayhip_scene_desc d = {};
        d.lights = lights.data(), d.lights_count = lr.lights_count, d.light_cwnodes = nodes.data(), d.light_cwnodes_count = lr.nodes_count;
        d.li_indices = li.data(), d.li_indices_count = lr.li_count, d.vtx_indices = vi.data(), d.vtx_indices_count = uint32_t(vi.size());
        d.vertices = vertices.data(), d.vertices_count = uint32_t(vertices.size());
        d.mesh_instances = instances.data(), d.mesh_instances_count = uint32_t(instances.size());
        if (prepare_light_refit(c, &d)) {
            return 1;
        }
    }
    lr.on = true;
    return 0;
}
