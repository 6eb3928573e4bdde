"""Emissive meshes that deform (rayhip_scene_refit_lights): with the switch on, a vertex update or a pose may move the vertices of
triangle lights, and their world-space corners, the 8-wide light tree and its importance rows are refitted ON THE DEVICE behind the
geometry (ray_amd/csrc/light_refit.h, light_refit.hip.h).

What is asserted: with the switch off every refusal is the one it was; with it on the light arrays equal the host build of the same
element functions (tests/hostsim/hostsim_lights.cpp) bit for bit, through all four entry points; frames equal those of a context that
uploaded the deformed scene afresh with the refitted tree put in its place; an instance update in between is survived; the
refitted tree samples without bias; and what stays refused leaves every array as it was.  tests/test_light_refit_hostsim.py holds
the host build against the reference's trees and a float64 model."""
import os

import numpy as np
import pytest
import torch  # noqa: F401  (FIRST: torch brings its own HIP runtime, and it must be the one that opens the device -- tests/test_gpu_comm.py)

import light_refit_cases as L
import skin_cases as S
import util
import vertex_update_cases as V
from ray_amd import api, hip

pytestmark = [pytest.mark.gpu]

W, H, SPP = 96, 64, 4
bits = L.bits


@pytest.fixture(scope="module")
def gpu_lib():
    lib = hip.Library()
    assert lib.device_count() > 0, "no HIP device: the product has no CPU path, -m gpu tests cannot run here"
    assert L.have_lights_lib() and V.have_refit_lib() and S.have_skin_lib(), "tests/hostsim is not built (run __graft_entry__.build())"
    return lib


def _need_host_lib(name):
    if name != "fixture" and not os.path.exists(api.HIP_HOST_LIB):
        pytest.skip("libray_hip.so not built (needs the reference tree at build time)")


def _context(lib, blob=None, refit=False, w=W, h=H):
    ctx = hip.Context(0, lib)
    ctx.upload_static(util.pmj())
    ctx.resize(w, h)
    if refit:
        ctx.refit_lights(True)  # (before the upload: the upload prepares the tables)
    if blob is not None:
        ctx.upload_scene_blob(blob)
    return ctx


def _frames(ctx, spp=SPP):
    ctx.clear()
    return util.render_frames(ctx, spp).copy()


def _arrays(ctx, kinds=(0, 1, 2, 4, 5, 6, 7)):
    return {k: ctx.read_accel(k).copy() for k in kinds}


def _same(x, y):
    return all(np.array_equal(bits(x[k]), bits(y[k])) for k in x)


def _on_device(array):
    t = torch.from_numpy(np.ascontiguousarray(array).view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return t


_cases = {}


def _case(name):
    """(blob at rest, its arrays, the vertices of the moved pose, a serialised scene AT that pose a fresh upload takes)"""
    _need_host_lib(name)
    if name not in _cases:
        blob = L.scene_blob(name, 0)
        a = L.Arrays(blob)
        if name == "fixture":
            v = L.moved_vertices(a)
            twin = L.twin_blob(blob, a, v)
        else:
            twin = L.scene_blob(name, 1)
            v = L.Arrays(twin).vertices
        assert not np.array_equal(bits(v["p"][a.light_vertices()]), bits(a.vertices["p"][a.light_vertices()]))
        _cases[name] = (blob, a, v, twin)
    return _cases[name]


def _light_skin(a, seed=5):
    """a skin from vertex 1 to the end of the fixture's array: the four vertices of its triangle light are inside"""
    s = S.Skin(a, 1, len(a.vertices) - 1, 3, seed)
    assert set(a.light_vertices()) <= set(range(s.first, s.first + s.count)) and (s.weights[np.array(a.light_vertices()) - 1] != 0).any()
    return s


def test_the_switch(gpu_lib):
    blob, a, v, _ = _case("fixture")
    whole = V.patched_blob(blob, vertices=v)
    skin = _light_skin(a)
    ctx = _context(gpu_lib, blob)
    before = _arrays(ctx)
    t = _on_device(v)
    # off (the default): a moved vertex of a triangle light is refused by every entry point, nothing touched
    assert ctx.update_vertices(0, v) == 2 and ctx.update_vertices_blob(whole) == 2 and ctx.update_vertices_device(0, len(v), t.data_ptr()) == 2
    assert ctx.create_skin(skin.first, skin.rest, skin.indices, skin.weights, 3) == 2
    assert _same(_arrays(ctx), before)
    # on, after the upload: the same calls are taken
    assert ctx.refit_lights(True) == 0 and ctx.refit_lights(True) == 0
    assert ctx.update_vertices(0, v) == 0 and ctx.update_vertices_blob(whole) == 0 and ctx.update_vertices_device(0, len(v), t.data_ptr()) == 0
    moved = _arrays(ctx)
    assert not np.array_equal(bits(moved[5]), bits(before[5])) and not np.array_equal(bits(moved[7]), bits(before[7]))
    sid = ctx.create_skin(skin.first, skin.rest, skin.indices, skin.weights, 3)
    assert sid >= 16
    # off again: not under a live skin over light vertices
    with pytest.raises(RuntimeError, match="covers vertex"):
        ctx.refit_lights(False)
    assert ctx.pose_skins({sid: S.identity_palette(3)}) == 0  # (still on)
    assert ctx.destroy_skin(sid) == 0 and ctx.refit_lights(False) == 0
    # ... and the refusals are back, judged against the vertices the lights describe now
    now = ctx.read_accel(4).copy()
    lit = now.copy()
    lit["p"][a.light_vertices()[0], 0] += 0.01
    assert ctx.update_vertices(0, lit) == 2 and ctx.update_vertices(0, now) == 0
    # the switch survives an upload
    assert ctx.refit_lights(True) == 0
    ctx.upload_scene_blob(blob)
    assert ctx.update_vertices(0, v) == 0 and _same(_arrays(ctx), moved)


@pytest.mark.parametrize("name", ["fixture", "one_emitter", "emissive_sheet"])
def test_light_arrays_equal_the_host_build(gpu_lib, name):
    """read-backs 5, 6 and 7 after update_vertices against tests/hostsim/hostsim_lights.cpp over the arrays the device held before; the
    geometry arrays still equal hostsim_refit.  emissive_sheet: five heights, 179 nodes at the lowest -- six blocks of the level kernel"""
    blob, a, v, _ = _case(name)
    ctx = _context(gpu_lib, blob, refit=name != "fixture")
    if name == "fixture":
        ctx.refit_lights(True)  # (after the upload: the switch prepares the tables from the arrays read back)
    old = _arrays(ctx)
    assert np.array_equal(bits(old[5]), bits(a.cwnodes)) and np.array_equal(bits(old[6]), bits(L.fill_children(a.cwnodes)))
    assert ctx.update_vertices(0, v) == 0
    got = _arrays(ctx)
    want = L.host_refit(a, v, cwnodes=old[5], children=old[6], tri_geom=old[7])
    assert not np.array_equal(bits(want.cwnodes), bits(old[5])) and not np.array_equal(bits(want.tri_geom), bits(old[7]))
    assert np.array_equal(bits(got[7]), bits(want.tri_geom))
    assert np.array_equal(bits(got[5]), bits(want.cwnodes))
    assert np.array_equal(bits(got[6]), bits(want.children))
    recs, nodes, _ = V.host_refit(a, v, nodes=old[0], tri_indices=old[2], tris=old[1])
    assert np.array_equal(bits(got[1]), bits(recs)) and np.array_equal(got[0], nodes) and np.array_equal(bits(got[4]), bits(v))
    # a second refit from the refitted state: the same arrays (nothing accumulates), and back at rest the tree of the rest pose
    assert ctx.update_vertices(0, v) == 0 and _same(_arrays(ctx), got)
    assert ctx.update_vertices(0, a.vertices) == 0
    back = L.host_refit(a, a.vertices, cwnodes=got[5], children=got[6], tri_geom=got[7])
    assert np.array_equal(bits(ctx.read_accel(5)), bits(back.cwnodes)) and np.array_equal(bits(ctx.read_accel(7)), bits(old[7]))


def test_every_entry_point_leaves_the_same_arrays(gpu_lib):
    blob, a, _, _ = _case("fixture")
    skin = _light_skin(a)
    palette = S.palette(3, 31, S.extent(a))
    posed = S.host_posed(a, [skin], [palette])
    assert not np.array_equal(bits(posed["p"][a.light_vertices()]), bits(a.vertices["p"][a.light_vertices()]))
    ctxs = [_context(gpu_lib, blob, refit=True) for _ in range(4)]
    assert ctxs[0].update_vertices(0, posed) == 0
    t = _on_device(posed)
    assert ctxs[1].update_vertices_device(0, len(posed), t.data_ptr()) == 0
    assert ctxs[2].update_vertices_blob(V.patched_blob(blob, vertices=posed)) == 0
    sid = ctxs[3].create_skin(skin.first, skin.rest, skin.indices, skin.weights, 3)
    assert sid >= 16 and ctxs[3].pose_skins({sid: palette}) == 0
    first = _arrays(ctxs[0])
    assert np.array_equal(bits(first[4]), bits(posed))
    want = L.host_refit(a, posed)
    assert np.array_equal(bits(first[5]), bits(want.cwnodes)) and np.array_equal(bits(first[6]), bits(want.children))
    for ctx in ctxs[1:]:
        assert _same(_arrays(ctx), first)
    frames = _frames(ctxs[0])
    assert all(np.array_equal(_frames(ctx), frames) for ctx in ctxs[1:])


@pytest.mark.parametrize("name", ["fixture", "emissive_sheet"])
def test_frames_equal_a_fresh_upload_with_the_refitted_tree(gpu_lib, name):
    blob, a, v, twin = _case(name)
    ctx = _context(gpu_lib, blob, refit=True)
    first = _frames(ctx)
    assert ctx.update_vertices(0, v) == 0
    updated = _frames(ctx)
    tree = ctx.read_accel(5).copy()
    fresh = _context(gpu_lib, L.with_section(twin, "light_cwnodes", tree))  # (the build at the moved pose has a tree of its own, of another size)
    assert np.array_equal(bits(fresh.read_accel(6)), bits(ctx.read_accel(6))) and np.array_equal(bits(fresh.read_accel(7)), bits(ctx.read_accel(7)))
    assert np.array_equal(updated, _frames(fresh)) and not np.array_equal(updated, first)
    assert np.isfinite(updated).all()


def test_pose_instance_update_pose(gpu_lib):
    """pose, then an instance update that moves the instance the light hangs on (the host's lights, tree and vertices replace the
    device's), then another pose: arrays and frames of a context that got the moved instance and the second pose only"""
    blob, a, _, _ = _case("fixture")
    skin = _light_skin(a)
    ext = S.extent(a)
    pose_a, pose_b = S.palette(3, 41, ext), S.palette(3, 42, ext)
    slot = int(a.lights[a.tri_lights()[0], 5])
    ctx, other = _context(gpu_lib, blob, refit=True), _context(gpu_lib, blob, refit=True)
    sid = ctx.create_skin(skin.first, skin.rest, skin.indices, skin.weights, 3)
    assert ctx.pose_skins({sid: pose_a}) == 0
    posed_a = _frames(ctx)
    moved = S.moved_blob(blob, a, S.host_posed(a, [skin], [pose_a]), slot, (0.03, -0.04, 0.02))
    assert ctx.update_instances(moved) == 0
    assert np.array_equal(bits(ctx.read_accel(5)), bits(a.cwnodes))  # the host's tree: it describes the HOST's vertices until the next pose
    assert ctx.pose_skins({sid: pose_b}) == 0  # (the skin outlives the instance update)
    assert other.update_instances(S.moved_blob(blob, a, a.vertices, slot, (0.03, -0.04, 0.02))) == 0
    assert other.update_vertices(0, S.host_posed(a, [skin], [pose_b])) == 0
    assert _same(_arrays(ctx), _arrays(other)) and np.array_equal(ctx.read_accel(3), other.read_accel(3))
    mi = L.Arrays(moved).mesh_instances
    want = L.host_refit(a, S.host_posed(a, [skin], [pose_b]), instances=mi)
    assert np.array_equal(bits(ctx.read_accel(5)), bits(want.cwnodes)) and np.array_equal(bits(ctx.read_accel(7)), bits(want.tri_geom))
    final = _frames(ctx)
    assert np.array_equal(final, _frames(other)) and not np.array_equal(final, posed_a)


def test_the_refitted_tree_is_a_fair_sampler(gpu_lib):
    """emissive_sheet, 64 x 64, 256 samples per pixel: the frame mean of RAW under the refitted tree against the mean under the tree the
    reference built for the same pose.  The noise floor is the difference of two renders with the reference-built tree over disjoint
    iterations (1..256 and 257..512; RAW is a running mean, so the second is 2 * mean(1..512) - mean(1..256)).  A biased estimator fails
    at any factor; the 3 only keeps noise from failing it."""
    blob, a, v, twin = _case("emissive_sheet")
    ctx = _context(gpu_lib, blob, refit=True, w=64, h=64)
    assert ctx.update_vertices(0, v) == 0
    refitted = float(_frames(ctx, 256)[..., :3].astype(np.float64).mean())
    rebuilt_ctx = _context(gpu_lib, twin, w=64, h=64)
    rebuilt_ctx.clear()
    m256 = float(util.render_frames(rebuilt_ctx, 256)[..., :3].astype(np.float64).mean())
    for it in range(257, 513):
        rebuilt_ctx.render(it)
    m512 = float(rebuilt_ctx.readback(hip.BUF_RAW)[..., :3].astype(np.float64).mean())
    second = 2.0 * m512 - m256
    floor, gap = abs(m256 - second), abs(refitted - m256)
    print(f"frame mean: refitted tree {refitted:.6f}, rebuilt tree {m256:.6f} (iterations 1..256) and {second:.6f} (257..512); "
          f"refit against rebuilt {gap:.3e}, noise floor {floor:.3e}")
    assert not np.array_equal(bits(ctx.read_accel(5)), bits(rebuilt_ctx.read_accel(5)))
    assert m256 > 0 and gap <= 3.0 * floor


def test_refusals_that_remain(gpu_lib, monkeypatch):
    blob, a, v, _ = _case("fixture")
    skin = _light_skin(a)
    ctx = _context(gpu_lib, blob, refit=True)
    assert ctx.update_vertices(0, v) == 0
    sid = ctx.create_skin(skin.first, None, skin.indices, skin.weights, 3)
    before = _arrays(ctx, (4, 5, 6, 7))
    frames = _frames(ctx)
    # a position of a vertex in use that is not finite: an error from every entry point, nothing written
    bad = v.copy()
    bad["p"][a.light_vertices()[1], 2] = np.inf
    t_bad = _on_device(bad)
    with_inf = S.palette(3, 7, S.extent(a))
    with_inf[:, 1, 3] = np.inf
    for call in (lambda: ctx.update_vertices(0, bad), lambda: ctx.update_vertices_device(0, len(bad), t_bad.data_ptr()),
                 lambda: ctx.update_vertices_blob(V.patched_blob(blob, vertices=bad)), lambda: ctx.pose_skins({sid: with_inf})):
        with pytest.raises(RuntimeError, match="not finite"):
            call()
        assert _same(_arrays(ctx, (4, 5, 6, 7)), before)
    assert np.array_equal(_frames(ctx), frames)
    # the 8-wide tree is built on the host only: the switch changes nothing about that
    monkeypatch.setenv("RAYHIP_BVH_WIDTH", "8")
    wide = _context(gpu_lib, blob, refit=True)
    monkeypatch.delenv("RAYHIP_BVH_WIDTH")
    assert wide.bvh_width() == 8
    wide_before = _arrays(wide, (4, 5, 6, 7))
    t = _on_device(v)
    assert wide.update_vertices(0, v) == 2 and wide.update_vertices_device(0, len(v), t.data_ptr()) == 2
    assert wide.create_skin(skin.first, skin.rest, skin.indices, skin.weights, 3) == 2
    assert _same(_arrays(wide, (4, 5, 6, 7)), wide_before)
