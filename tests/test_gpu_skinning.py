"""Skinning on the device (rayhip_skin_create / rayhip_scene_pose_skins) and vertex updates from device memory
(rayhip_scene_update_vertices_device): a pose is a palette of bone matrices, the vertices are posed by a kernel into a staging
array, checked there, copied device to device and refitted as rayhip_scene_update_vertices refits (ray_amd/csrc/skin.h,
skin.hip.h).

What is asserted: the posed vertices equal the host build of the same element functions (tests/hostsim/hostsim_skin.cpp) bit for
bit; every array and frame after a pose equals that of a context which got the host-skinned vertices through update_vertices -- the
same arrays under the same trees, so no tie clause; and every refusal leaves the frames as they were.  The scene is the committed
fixture cornell_instances: 128 vertices, so every pose here is ONE block of k_skin_vertices (launches of many blocks are compared
with the host build by tools/skin_bench.py on the scenes it times)."""
import numpy as np
import pytest
import torch  # noqa: F401  (FIRST: torch brings its own HIP runtime, and it must be the one that opens the device -- tests/test_gpu_comm.py)

import skin_cases as S
import util
import vertex_update_cases as V
from ray_amd import hip

pytestmark = [pytest.mark.gpu]

W, H, SPP = 96, 64, 4
bits = S.bits


@pytest.fixture(scope="module")
def gpu_lib():
    lib = hip.Library()
    assert lib.device_count() > 0, "no HIP device: the product has no CPU path, -m gpu tests cannot run here"
    assert S.have_skin_lib() and V.have_refit_lib(), "tests/hostsim is not built (run __graft_entry__.build())"
    return lib


@pytest.fixture(scope="module")
def fixture_scene():
    blob, a = S.scene()
    return blob, a, S.extent(a)


def _context(lib, blob=None):
    ctx = hip.Context(0, lib)
    ctx.upload_static(util.pmj())
    ctx.resize(W, H)
    if blob is not None:
        ctx.upload_scene_blob(blob)
    return ctx


def _frames(ctx):
    ctx.clear()
    return util.render_frames(ctx, SPP).copy()


def _create(ctx, s, with_rest=True):
    return ctx.create_skin(s.first, s.rest if with_rest else None, s.indices, s.weights, s.bones_count)


def _accel(ctx):
    return [ctx.read_accel(k).copy() for k in (0, 1, 2)]


def _same_accel(x, y):
    return all(np.array_equal(bits(p), bits(q)) for p, q in zip(x, y))


@pytest.fixture(scope="module")
def unposed(gpu_lib, fixture_scene):
    """(frames, vertex array) of the scene as uploaded: computed once, never changed"""
    ctx = _context(gpu_lib, fixture_scene[0])
    return _frames(ctx), ctx.read_accel(4).copy()


@pytest.mark.parametrize("bones", S.BONES)
def test_posed_vertices_equal_the_host_build(gpu_lib, fixture_scene, unposed, bones):
    """palettes of 1, 3 and 257 bones (read from LDS / from memory); a skin that starts at vertex 1 with a count that is no multiple
    of 64 posed TOGETHER with a disjoint second one in one call; then a skin of one vertex; vertices outside every skin keep their bytes"""
    blob, a, ext = fixture_scene
    first, second, single = S.seeded_skins(a, bones)
    assert np.array_equal(bits(unposed[1]), bits(a.vertices))
    ctx = _context(gpu_lib, blob)
    ids = [_create(ctx, first), _create(ctx, second, with_rest=False)]  # (the second: the rest pose the device holds)
    assert ids[0] != ids[1] and all(i >= 16 for i in ids)  # (handles, never a return code)
    palettes = [S.palette(bones, 40 + k, ext) for k in range(2)]
    assert ctx.pose_skins(dict(zip(ids, palettes))) == 0
    want = S.host_posed(a, [first, second], palettes)
    got = ctx.read_accel(4)
    assert got.dtype == hip.VERTEX_DTYPE and np.array_equal(bits(got), bits(want))
    outside = np.r_[0, first.first + first.count:second.first]
    assert np.array_equal(bits(got[outside]), bits(a.vertices[outside])) and not np.array_equal(bits(got), bits(a.vertices))
    # one skin of the two alone: the other keeps its last pose
    again = S.palette(bones, 50, ext)
    assert ctx.pose_skins({ids[0]: again}) == 0
    want = S.host_posed(a, [first], [again], vertices=want)
    assert np.array_equal(bits(ctx.read_accel(4)), bits(want))
    # a skin of one vertex, in the place of the second
    assert ctx.destroy_skin(ids[1]) == 0 and ctx.destroy_skin(ids[1]) == 2
    one = _create(ctx, single)
    lone = S.palette(bones, 51, ext)
    assert ctx.pose_skins({one: lone}) == 0
    want = S.host_posed(a, [single], [lone], vertices=want)
    assert np.array_equal(bits(ctx.read_accel(4)), bits(want))


def test_arrays_and_frames_after_a_pose_equal_a_host_skinned_update(gpu_lib, fixture_scene, unposed):
    blob, a, ext = fixture_scene
    skins = S.seeded_skins(a, 3)[:2]
    palettes = [S.palette(3, 60 + k, ext) for k in range(2)]
    ctx = _context(gpu_lib, blob)
    ids = [_create(ctx, s) for s in skins]
    assert ctx.pose_skins(dict(zip(ids, palettes))) == 0
    other = _context(gpu_lib, blob)
    assert other.update_vertices(0, S.host_posed(a, skins, palettes)) == 0
    assert _same_accel(_accel(ctx), _accel(other)) and np.array_equal(ctx.read_accel(3), other.read_accel(3))
    assert np.array_equal(bits(ctx.read_accel(4)), bits(other.read_accel(4)))
    posed = _frames(ctx)
    assert np.array_equal(posed, _frames(other))
    assert not np.array_equal(posed, unposed[0])


def test_poses_do_not_accumulate(gpu_lib, fixture_scene, unposed):
    """pose A then pose B is pose B.  And back: an identity pose of the seeded skins gives what the host build makes of the REST pose
    (positions within 2^-21 of it: tests/test_skinning_hostsim.py derives the bound; normals normalised); with skins whose identity
    pose is the rest pose bytewise (skin_cases.exact_identity_skin) the vertex array and the frames are the first ones again"""
    blob, a, ext = fixture_scene
    skins = S.seeded_skins(a, 3)[:2]
    pose_a, pose_b = ([S.palette(3, seed + k, ext) for k in range(2)] for seed in (70, 80))
    ctx = _context(gpu_lib, blob)
    ids = [_create(ctx, s) for s in skins]
    assert ctx.pose_skins(dict(zip(ids, pose_a))) == 0
    frames_a = _frames(ctx)
    assert ctx.pose_skins(dict(zip(ids, pose_b))) == 0
    frames_b = _frames(ctx)
    alone = _context(gpu_lib, blob)
    alone_ids = [_create(alone, s) for s in skins]
    assert alone.pose_skins(dict(zip(alone_ids, pose_b))) == 0
    assert np.array_equal(bits(ctx.read_accel(4)), bits(alone.read_accel(4))) and _same_accel(_accel(ctx), _accel(alone))
    assert np.array_equal(frames_b, _frames(alone)) and not np.array_equal(frames_a, frames_b)
    identity = [S.identity_palette(3)] * 2
    assert ctx.pose_skins(dict(zip(ids, identity))) == 0
    got = ctx.read_accel(4)
    assert np.array_equal(bits(got), bits(S.host_posed(a, skins, identity)))
    assert np.all(np.abs(got["p"] - a.vertices["p"]) <= np.abs(a.vertices["p"]) * np.float32(2.0 ** -21))
    # the skins whose identity pose is exact
    for i in ids:
        assert ctx.destroy_skin(i) == 0
    exact = [S.exact_identity_skin(a, s) for s in skins]
    assert sum(s.count - len(s.unweighted) for s in exact) >= 16
    assert ctx.update_vertices(0, a.vertices) == 0  # (the rest pose the skins are created over)
    ids = [_create(ctx, s, with_rest=False) for s in exact]
    assert ctx.pose_skins(dict(zip(ids, pose_a))) == 0
    assert not np.array_equal(_frames(ctx), unposed[0])
    assert ctx.pose_skins(dict(zip(ids, identity))) == 0
    assert np.array_equal(bits(ctx.read_accel(4)), bits(unposed[1]))
    assert np.array_equal(_frames(ctx), unposed[0])


def test_update_vertices_from_device_memory(gpu_lib, fixture_scene, unposed):
    blob, a, _ = fixture_scene
    v = V.perturbed_vertices(a)

    def on_device(array):
        t = torch.from_numpy(np.ascontiguousarray(array).view(np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        return t

    ctx, other = _context(gpu_lib, blob), _context(gpu_lib, blob)
    t = on_device(v)
    assert ctx.update_vertices_device(0, len(v), t.data_ptr()) == 0
    assert other.update_vertices(0, v) == 0
    assert np.array_equal(bits(ctx.read_accel(4)), bits(v))
    assert _same_accel(_accel(ctx), _accel(other)) and np.array_equal(ctx.read_accel(3), other.read_accel(3))
    moved = _frames(ctx)
    assert np.array_equal(moved, _frames(other)) and not np.array_equal(moved, unposed[0])
    # a range in the middle of the array, the light's vertices inside it and unchanged: fine
    lv = a.light_vertices()
    lo, hi = min(lv) - 3, max(lv) + 6
    part = on_device(a.vertices[lo:hi])
    assert ctx.update_vertices_device(lo, hi - lo, part.data_ptr()) == 0 and other.update_vertices(lo, a.vertices[lo:hi]) == 0
    assert np.array_equal(bits(ctx.read_accel(4)), bits(other.read_accel(4))) and _same_accel(_accel(ctx), _accel(other))
    before = _frames(ctx)
    # a changed vertex of the light: 2; a NaN in a used position: an error; a range outside the array: an error -- nothing touched
    lit = v.copy()
    lit["p"][lv[1], 2] += 0.01
    t_lit = on_device(lit)
    assert ctx.update_vertices_device(0, len(v), t_lit.data_ptr()) == 2
    bad = v.copy()
    used = int(S.used_vertices(a)[-1])
    bad["p"][used, 1] = np.nan
    t_bad = on_device(bad)
    with pytest.raises(RuntimeError, match="not finite"):
        ctx.update_vertices_device(0, len(v), t_bad.data_ptr())
    unused = np.setdiff1d(np.arange(len(v)), S.used_vertices(a))
    with pytest.raises(RuntimeError, match="outside"):
        ctx.update_vertices_device(len(v) - 3, 4, t.data_ptr())
    assert np.array_equal(bits(ctx.read_accel(4)), bits(other.read_accel(4)))
    assert np.array_equal(_frames(ctx), before)
    # ... while a NaN in a slot no triangle uses is the caller's business
    free = v.copy()
    free["p"][unused[0]] = np.nan
    t_free = on_device(free)
    assert ctx.update_vertices_device(0, len(v), t_free.data_ptr()) == 0
    assert np.array_equal(_frames(ctx), moved)


def test_instance_updates_and_poses_keep_each_other(gpu_lib, fixture_scene):
    """the fixture's own instances: after a pose, instance 2 moves (rayhip_scene_update_instances) and the pose stays; after that, another
    pose and the instance stays where it went.  Held against a context that reaches the same states by update_vertices."""
    blob, a, ext = fixture_scene
    skins = S.seeded_skins(a, 3)[:2]
    pose_a, pose_b = ([S.palette(3, seed + k, ext) for k in range(2)] for seed in (90, 95))
    ctx, other = _context(gpu_lib, blob), _context(gpu_lib, blob)
    ids = [_create(ctx, s) for s in skins]
    assert ctx.pose_skins(dict(zip(ids, pose_a))) == 0 and other.update_vertices(0, S.host_posed(a, skins, pose_a)) == 0
    posed = _frames(ctx)
    moved = S.moved_blob(blob, a, S.host_posed(a, skins, pose_a), 2, (0.07, 0.1, -0.05))
    assert ctx.update_instances(moved) == 0 and other.update_instances(moved) == 0
    assert np.array_equal(bits(ctx.read_accel(4)), bits(S.host_posed(a, skins, pose_a)))  # the pose stayed
    assert np.array_equal(ctx.read_accel(3), other.read_accel(3))
    after_move = _frames(ctx)
    assert np.array_equal(after_move, _frames(other)) and not np.array_equal(after_move, posed)
    assert ctx.pose_skins(dict(zip(ids, pose_b))) == 0 and other.update_vertices(0, S.host_posed(a, skins, pose_b)) == 0  # the skins outlive an instance update
    assert _same_accel(_accel(ctx), _accel(other)) and np.array_equal(ctx.read_accel(3), other.read_accel(3))
    after_pose = _frames(ctx)
    assert np.array_equal(after_pose, _frames(other)) and not np.array_equal(after_pose, after_move)
    # the instance stayed where it went: the same pose without the move looks different
    still = _context(gpu_lib, blob)
    assert still.update_vertices(0, S.host_posed(a, skins, pose_b)) == 0
    assert not np.array_equal(after_pose, _frames(still))


def test_refusals(gpu_lib, fixture_scene, unposed, monkeypatch):
    blob, a, ext = fixture_scene
    first, second, _ = S.seeded_skins(a, 3)
    some = torch.zeros(len(a.vertices) * 44, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    empty = _context(gpu_lib)  # nothing uploaded yet
    assert _create(empty, first) == 2 and empty.pose_skins({16: S.identity_palette(3)}) == 2
    assert empty.update_vertices_device(0, len(a.vertices), some.data_ptr()) == 2
    ctx = _context(gpu_lib, blob)
    skin = _create(ctx, second)
    assert skin >= 16
    with pytest.raises(RuntimeError, match="overlap"):
        ctx.create_skin(second.first + second.count - 1, None, second.indices[:1], second.weights[:1], 3)
    with pytest.raises(RuntimeError, match="outside"):
        ctx.create_skin(len(a.vertices) - 1, None, second.indices[:2], second.weights[:2], 3)
    idx = first.indices.copy()
    idx[-1, 0] = 3  # == bones_count
    with pytest.raises(RuntimeError, match="outside the palette"):
        ctx.create_skin(first.first, first.rest, idx, first.weights, 3)
    for w_bad in (-0.5, np.nan):
        w = first.weights.copy()
        w[0, 1] = w_bad
        with pytest.raises(RuntimeError, match="negative or not finite"):
            ctx.create_skin(first.first, first.rest, first.indices, w, 3)
    lights = a.light_vertices()
    over = slice(lights[-1] - 2, lights[-1] + 1)  # ends on a vertex of the light, clear of the live skin
    assert ctx.create_skin(over.start, None, first.indices[:3], first.weights[:3], 3) == 2
    assert ctx.pose_skins({skin + 1: S.identity_palette(3)}) == 2 and ctx.pose_skins({5: S.identity_palette(3)}) == 2  # no such skins
    with_inf = S.palette(3, 7, ext)
    with_inf[1, 2, 3] = np.inf
    reached = np.arange(second.count)[((second.indices == 1) & (second.weights != 0)).any(axis=1)] + second.first
    assert np.isin(reached, S.used_vertices(a)).any()
    with pytest.raises(RuntimeError, match="not finite"):
        ctx.pose_skins({skin: with_inf})
    assert np.array_equal(bits(ctx.read_accel(4)), bits(unposed[1]))
    assert np.array_equal(_frames(ctx), unposed[0])
    # sixteen skins are live at most
    assert ctx.destroy_skin(skin) == 0
    free = [i for i in range(len(a.vertices)) if i not in lights][:17]
    many = [ctx.create_skin(i, None, first.indices[:1], first.weights[:1], 3) for i in free[:16]]
    assert len(set(many)) == 16 and min(many) >= 16 and skin not in many
    with pytest.raises(RuntimeError, match="live already"):
        ctx.create_skin(free[16], None, first.indices[:1], first.weights[:1], 3)
    assert np.array_equal(_frames(ctx), unposed[0])
    # an upload discards them all
    ctx.upload_scene_blob(blob)
    assert ctx.pose_skins({many[3]: S.identity_palette(3)}) == 2
    assert np.array_equal(_frames(ctx), unposed[0])
    again = _create(ctx, first)
    assert again >= 16 and again not in many  # (a new skin in the first one's place: a new id, the old one stays dead)
    assert ctx.pose_skins({many[0]: S.identity_palette(3)}) == 2 and ctx.pose_skins({again: S.identity_palette(3)}) == 0
    # the 8-wide tree is built on the host only
    monkeypatch.setenv("RAYHIP_BVH_WIDTH", "8")
    wide = _context(gpu_lib, blob)
    monkeypatch.delenv("RAYHIP_BVH_WIDTH")
    assert wide.bvh_width() == 8
    wide_first = _frames(wide)
    assert _create(wide, first) == 2 and wide.pose_skins({16: S.identity_palette(3)}) == 2
    assert wide.update_vertices_device(0, len(a.vertices), some.data_ptr()) == 2
    assert np.array_equal(_frames(wide), wide_first)
