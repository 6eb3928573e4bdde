"""Meshes that deform in place (rayhip_scene_update_vertices): new vertex data for an uploaded scene, everything that depends on
positions recomputed ON THE DEVICE under the trees the upload made -- triangle records, refitted boxes, the 4-wide collapse, the
top level (ray_amd/csrc/refit.h, refit.hip.h).

What is asserted: the device arrays equal the host build of the same element functions bit for bit; and, a BVH being a culling
structure, the hits and frames after an update are those of a context that uploaded the deformed scene afresh (another tree over the
same surfaces) -- bit for bit, the scenes having no exact-distance ties (tests/test_vertex_update_hostsim.py checks that on the host)."""
import os

import numpy as np
import pytest

import util
import vertex_update_cases as V
from ray_amd import api, hip

pytestmark = [pytest.mark.gpu]

W, H, SPP = 96, 64, 4


@pytest.fixture(scope="module")
def gpu_lib():
    lib = hip.Library()
    assert lib.device_count() > 0, "no HIP device: the product has no CPU path, -m gpu tests cannot run here"
    return lib


def _need_host_lib():
    if not os.path.exists(api.HIP_HOST_LIB):
        pytest.skip("libray_hip.so not built (needs the reference tree at build time)")


def _context(lib, blob=None, w=W, h=H):
    ctx = hip.Context(0, lib)
    ctx.upload_static(util.pmj())
    ctx.resize(w, h)
    if blob is not None:
        ctx.upload_scene_blob(blob)
    return ctx


def _frames(ctx, flags=0):
    ctx.clear()
    return util.render_frames(ctx, SPP, flags=flags).copy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_device_arrays_equal_the_host_build(gpu_lib):
    """cornell_instances under perturbed vertices (five meshes, trees that are a single pair of leaves, a last block that is a partial
    wave): records and bottom-level nodes against tests/hostsim/hostsim_refit.cpp over the arrays the device held before"""
    assert V.have_refit_lib(), "tests/hostsim/hostsim_refit.cpp is not built (run __graft_entry__.build())"
    blob = util.golden_scene("cornell_instances")
    a = V.Arrays(blob)
    ctx = _context(gpu_lib, blob)
    nodes0, tris0, tri_indices = ctx.read_accel(0).copy(), ctx.read_accel(1).copy(), ctx.read_accel(2).copy()
    assert len(tris0) == len(tri_indices) and len(tris0) % 64 != 0 and len(nodes0) >= len(a.nodes)
    v = V.perturbed_vertices(a)
    assert ctx.update_vertices(0, v) == 0
    recs, nodes, n_degenerate = V.host_refit(a, v, nodes=nodes0, tri_indices=tri_indices, tris=tris0)
    assert n_degenerate == 0 and not np.array_equal(recs, tris0)
    assert np.array_equal(ctx.read_accel(2), tri_indices)
    assert np.array_equal(bits(ctx.read_accel(1)), bits(recs))
    assert np.array_equal(ctx.read_accel(0), nodes)
    assert np.array_equal(bits(recs), bits(V.numpy_entry_records(a, v, np.arange(len(recs)), tri_indices)))  # (the refinement keeps reachable entries only)
    # one triangle collapsed to a point: the zero record
    t, moved = V.collapse_one_triangle(a, v)
    assert ctx.update_vertices(moved, v[moved:moved + 1]) == 0  # (a range of one vertex, not the whole array)
    recs, nodes, n_degenerate = V.host_refit(a, v, nodes=nodes0, tri_indices=tri_indices, tris=tris0)
    got = ctx.read_accel(1)
    assert n_degenerate == 1 and (tri_indices == t).any() and not got[tri_indices == t].any()
    assert np.array_equal(bits(got), bits(recs)) and np.array_equal(ctx.read_accel(0), nodes)
    ctx.render(1)  # and the scene with an unhittable triangle renders
    assert np.isfinite(ctx.readback(hip.BUF_RAW)).all()


def test_hits_after_an_update_are_those_of_a_fresh_upload(gpu_lib):
    _need_host_lib()
    ctx = _context(gpu_lib, V.scene_blob("sheet", 0))
    assert ctx.update_vertices_blob(V.scene_blob("sheet", 1)) == 0
    fresh = _context(gpu_lib, V.scene_blob("sheet", 1))
    rays, hits = fresh.k_generate_primary_rays(1)
    _, want, _ = fresh.k_intersect_closest(rays, hits, 1, flags=0)
    _, got, _ = ctx.k_intersect_closest(rays, hits, 1, flags=0)  # (the same rays: the hook hands them out in no fixed order)
    assert (want["v"] >= 0).sum() > len(want) // 2
    util.assert_hits_identical(got, want)


@pytest.mark.parametrize("name", sorted(V.SCENES))
def test_frames_after_an_update_are_those_of_a_fresh_upload(gpu_lib, name):
    _need_host_lib()
    old, new = V.scene_blob(name, 0), V.scene_blob(name, 1)
    ctx = _context(gpu_lib, old)
    first = _frames(ctx)
    assert ctx.update_vertices_blob(new) == 0
    updated = _frames(ctx)
    fresh_ctx = _context(gpu_lib, new)
    fresh = _frames(fresh_ctx)
    assert not np.array_equal(first, updated)
    assert np.array_equal(updated, fresh)
    # the top level: the same live slots as after a fresh upload.  The BOXES are transform_box's, which rounds its sums in another order
    # than the scene build's TransformBoundingBox (tests/test_vertex_update_hostsim.py: test_instance_boxes_against_the_scene_build): they
    # equal the host build's bit for bit and the fresh upload's to a few ulps
    got, want = ctx.read_accel(3), fresh_ctx.read_accel(3)
    assert np.array_equal(got[:, 0], want[:, 0]) and len(got) == len(V.Arrays(new).live_instances())
    a = V.Arrays(old)
    if V.have_refit_lib():
        host = V.instance_boxes(ctx.read_accel(0), a.mesh_instances, got[:, 0])
        assert np.array_equal(got[:, 1:], bits(host))
    gb, wb = got[:, 1:].copy().view(np.float32), want[:, 1:].copy().view(np.float32)
    assert np.all(np.abs(gb - wb) <= 4 * np.spacing(np.maximum(np.abs(gb), np.abs(wb))))
    # and back: the same tree, the same boxes, the same records -- no tie clause
    assert ctx.update_vertices_blob(old) == 0
    assert np.array_equal(_frames(ctx), first)


def test_an_instance_update_after_a_vertex_update(gpu_lib):
    _need_host_lib()
    ctx = _context(gpu_lib, V.scene_blob("sheets_instanced", 0))
    assert ctx.update_vertices_blob(V.scene_blob("sheets_instanced", 1)) == 0
    before = _frames(ctx)
    moved = V.scene_blob("sheets_instanced", 1, moved=True)
    assert ctx.update_instances(moved) == 0
    got = _frames(ctx)
    assert not np.array_equal(got, before)
    assert np.array_equal(got, _frames(_context(gpu_lib, moved)))
    # ... and a vertex update after that keeps the moved instance
    assert ctx.update_vertices_blob(V.scene_blob("sheets_instanced", 0, moved=True)) == 0
    assert np.array_equal(_frames(ctx), _frames(_context(gpu_lib, V.scene_blob("sheets_instanced", 0, moved=True))))


def test_the_instrumented_walk_agrees_after_an_update(gpu_lib):
    """the counting kernels walk the BVH2, the product kernels its 4-wide collapse: the same frame from both says the refitted boxes and
    the collapsed ones belong together"""
    _need_host_lib()
    ctx = _context(gpu_lib, V.scene_blob("sheet", 0))
    assert ctx.update_vertices_blob(V.scene_blob("sheet", 1)) == 0
    assert ctx.bvh_width() == 4
    plain = _frames(ctx)
    assert np.array_equal(_frames(ctx, flags=hip.FLAG_COUNT_TRAVERSAL), plain)


def test_refusals(gpu_lib, monkeypatch):
    blob = util.golden_scene("cornell_instances")
    a = V.Arrays(blob)
    v = V.perturbed_vertices(a)
    empty = _context(gpu_lib)
    assert empty.update_vertices(0, v) == 2  # nothing uploaded yet
    ctx = _context(gpu_lib, blob)
    first = _frames(ctx)
    with pytest.raises(RuntimeError, match="outside"):
        ctx.update_vertices(len(v) - 3, v[:4])
    assert np.array_equal(_frames(ctx), first)
    bad = v.copy()
    used = int(a.vtx_indices[3 * int(a.tri_indices[a.reachable_entries()[0]])])
    bad["p"][used, 1] = np.nan
    with pytest.raises(RuntimeError, match="not finite"):
        ctx.update_vertices(0, bad)
    assert np.array_equal(_frames(ctx), first)
    lit = v.copy()
    lv = a.light_vertices()
    lit["p"][lv[0], 0] += 0.01
    assert ctx.update_vertices(0, lit) == 2
    assert np.array_equal(_frames(ctx), first)
    monkeypatch.setenv("RAYHIP_BVH_WIDTH", "8")
    wide = _context(gpu_lib, blob)
    monkeypatch.delenv("RAYHIP_BVH_WIDTH")
    assert wide.bvh_width() == 8
    wide_first = _frames(wide)
    assert wide.update_vertices(0, v) == 2
    assert np.array_equal(_frames(wide), wide_first)
    # the light's vertices unchanged inside a larger range: fine
    assert ctx.update_vertices(min(lv) - 1, v[min(lv) - 1:max(lv) + 2]) == 0
    assert not np.array_equal(_frames(ctx), first)
