"""Morph targets on the device (rayhip_morph_create / rayhip_scene_pose), alone and ahead of a skin: a pose is one weight per target,
the vertices are posed by a kernel into a staging array, checked there, copied device to device and refitted as
rayhip_scene_update_vertices refits (ray_amd/csrc/morph.h, morph.hip.h).

What is asserted: the posed vertices equal the host build of the same element functions (tests/hostsim/hostsim_morph.cpp) bit for bit;
every array and frame after a pose equals that of a context which got the host-built vertices through update_vertices -- the same
arrays under the same trees, so no tolerance; and every refusal leaves arrays and frames as they were.  The scene is the committed
fixture cornell_instances: 128 vertices, so every launch here is ONE block (launches of many blocks are compared with the host build
by tools/morph_bench.py on the scenes it times)."""
import numpy as np
import pytest
import torch  # noqa: F401  (FIRST: torch brings its own HIP runtime, and it must be the one that opens the device -- tests/test_gpu_comm.py)

import morph_cases as M
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
    assert M.have_morph_lib() and S.have_skin_lib() and V.have_refit_lib(), "tests/hostsim is not built (run __graft_entry__.build())"
    return lib


@pytest.fixture(scope="module")
def fixture_scene():
    blob, a = S.scene()
    return blob, a, S.extent(a)


def _context(lib, blob=None, refit=False):
    ctx = hip.Context(0, lib)
    ctx.upload_static(util.pmj())
    ctx.resize(W, H)
    if refit:
        ctx.refit_lights(True)
    if blob is not None:
        ctx.upload_scene_blob(blob)
    return ctx


def _frames(ctx):
    ctx.clear()
    return util.render_frames(ctx, SPP).copy()


def _create(ctx, ms, with_base=True):
    return ctx.create_morph(ms.first, ms.count, ms.base if with_base else None, ms.targets)


def _create_skin(ctx, s):
    return ctx.create_skin(s.first, s.rest, s.indices, s.weights, s.bones_count)


def _accel(ctx, kinds=(0, 1, 2, 4)):
    return [ctx.read_accel(k).copy() for k in kinds]


def _same(x, y):
    return all(np.array_equal(bits(p), bits(q)) for p, q in zip(x, y))


@pytest.fixture(scope="module")
def unposed(gpu_lib, fixture_scene):
    """(frames, arrays 0, 1, 2, 4) of the scene as uploaded: computed once, never changed"""
    ctx = _context(gpu_lib, fixture_scene[0])
    return _frames(ctx), _accel(ctx)


@pytest.mark.parametrize("targets", M.TARGETS)
def test_posed_vertices_equal_the_host_build(gpu_lib, fixture_scene, unposed, targets):
    """a set in no skin, 1 / 3 / 1025 targets (weights from LDS / from memory), from vertex 1 with a count that is no multiple of 64:
    rows of length 0, rows with every target, a row whose entries all have weight 0, a target without vertices, targets without
    normal deltas, weights -0.5 and 1.5.  A second pose is independent of the first; all weights 0 give the base records back."""
    blob, a, _ = fixture_scene
    first, count = M.standalone_range(a)
    ms = M.seeded_set(a, first, count, targets, 5)
    ctx = _context(gpu_lib, blob)
    mid = _create(ctx, ms, with_base=False)  # (the base records the device holds)
    assert mid >= 16
    outside = np.r_[0, first + count:len(a.vertices)]
    for seed in (1, 2):  # (the second pose starts from the base again, not from the first)
        w = M.seeded_weights(targets, seed)
        assert ctx.pose({mid: w}, {}) == 0
        want = M.host_morphed(a, [ms], [w])
        got = ctx.read_accel(4)
        assert got.dtype == hip.VERTEX_DTYPE and np.array_equal(bits(got), bits(want))
        assert np.array_equal(bits(got[outside]), bits(a.vertices[outside])) and not np.array_equal(bits(got), bits(a.vertices))
    assert ctx.pose({mid: np.zeros(targets, dtype=np.float32)}, {}) == 0
    assert np.array_equal(bits(ctx.read_accel(4)), bits(unposed[1][3]))
    assert np.array_equal(_frames(ctx), unposed[0])


@pytest.mark.parametrize("bones", (3, 257))
@pytest.mark.parametrize("targets", M.TARGETS)
def test_morph_then_skin_equals_the_host_build(gpu_lib, fixture_scene, targets, bones):
    """one call: a skin (palette in LDS / in memory) that holds two disjoint sets -- the first between two plain segments, no boundary at
    a multiple of 64 -- and a set in no skin elsewhere"""
    blob, a, ext = fixture_scene
    skin = S.seeded_skins(a, bones)[1]
    inside = [M.seeded_set(a, f, c, targets, 8 + k) for k, (f, c) in enumerate(M.ranges_inside(skin))]
    alone = M.seeded_set(a, *M.standalone_range(a), targets, 5)
    ctx = _context(gpu_lib, blob)
    sets = [alone] + inside
    ids = [_create(ctx, inside[1]), _create_skin(ctx, skin), _create(ctx, alone), _create(ctx, inside[0])]  # (either may be created first)
    mids, sid = [ids[2], ids[3], ids[0]], ids[1]
    assert len(set(mids)) == 3 and min(mids) >= 16
    for seed in (1, 2):
        weights = [M.seeded_weights(targets, seed + k) for k in range(3)]
        palette = S.palette(bones, 40 + seed, ext)
        assert ctx.pose(dict(zip(mids, weights)), {sid: palette}) == 0
        want = M.host_morphed(a, sets, weights, [skin], [palette])
        got = ctx.read_accel(4)
        assert np.array_equal(bits(got), bits(want))
        outside = np.r_[0, alone.first + alone.count:skin.first]
        assert np.array_equal(bits(got[outside]), bits(a.vertices[outside]))
        plain = S.host_posed(a, [skin], [palette])  # the skin's plain segments are the skin alone, its covered ones are not
        covered = np.zeros(len(got), dtype=bool)
        for ms in sets:
            covered[ms.first:ms.first + ms.count] = True
        assert np.array_equal(bits(got[~covered]), bits(plain[~covered])) and not np.array_equal(bits(got[covered]), bits(plain[covered]))
    # the set in no skin alone: the others keep their last pose
    w = M.seeded_weights(targets, 7)
    assert ctx.pose({mids[0]: w}, {}) == 0
    assert np.array_equal(bits(ctx.read_accel(4)), bits(M.host_morphed(a, [alone], [w], vertices=want)))


def test_arrays_and_frames_after_a_pose_equal_a_host_built_update(gpu_lib, fixture_scene, unposed):
    blob, a, ext = fixture_scene
    skin = S.seeded_skins(a, 3)[1]
    inside = [M.seeded_set(a, f, c, 3, 8 + k) for k, (f, c) in enumerate(M.ranges_inside(skin))]
    alone = M.seeded_set(a, *M.standalone_range(a), 1025, 5)
    sets = [alone] + inside
    weights = [M.seeded_weights(ms.targets_count, 3 + k) for k, ms in enumerate(sets)]
    palette = S.palette(3, 61, ext)
    ctx = _context(gpu_lib, blob)
    mids = [_create(ctx, ms) for ms in sets]
    sid = _create_skin(ctx, skin)
    assert ctx.pose(dict(zip(mids, weights)), {sid: palette}) == 0
    other = _context(gpu_lib, blob)
    assert other.update_vertices(0, M.host_morphed(a, sets, weights, [skin], [palette])) == 0
    assert _same(_accel(ctx), _accel(other)) and np.array_equal(ctx.read_accel(3), other.read_accel(3))
    posed = _frames(ctx)
    assert np.array_equal(posed, _frames(other))
    assert not np.array_equal(posed, unposed[0])
    # a second pose is independent of the first: the same as on a fresh context
    weights_b = [M.seeded_weights(ms.targets_count, 13 + k) for k, ms in enumerate(sets)]
    palette_b = S.palette(3, 62, ext)
    assert ctx.pose(dict(zip(mids, weights_b)), {sid: palette_b}) == 0
    assert other.update_vertices(0, M.host_morphed(a, sets, weights_b, [skin], [palette_b])) == 0
    assert _same(_accel(ctx), _accel(other)) and np.array_equal(_frames(ctx), _frames(other))


def test_refusals(gpu_lib, fixture_scene, unposed, monkeypatch):
    blob, a, ext = fixture_scene
    skin = S.seeded_skins(a, 3)[1]
    first, count = M.standalone_range(a)
    alone = M.seeded_set(a, first, count, 3, 5)
    alone.targets[0] = (alone.targets[0][0], np.full_like(alone.targets[0][1], 2.0)) + alone.targets[0][2:]  # (a weight of 3e38 overflows)
    inside = M.seeded_set(a, *M.ranges_inside(skin)[0], 3, 8)
    w3 = M.seeded_weights(3, 1)
    identity = S.identity_palette(3)
    empty = _context(gpu_lib)  # nothing uploaded yet
    assert _create(empty, alone) == 2 and empty.pose({16: w3}, {}) == 2 and empty.pose({}, {}) == 0
    ctx = _context(gpu_lib, blob)
    mid = _create(ctx, alone)
    assert mid >= 16
    # -- rayhip_morph_create --
    with pytest.raises(RuntimeError, match="overlap"):
        ctx.create_morph(first + count - 1, 8, None, M.seeded_set(a, first + count - 1, 8, 1, 1).targets)
    with pytest.raises(RuntimeError, match="outside"):
        ctx.create_morph(len(a.vertices) - 7, 8, None, inside.targets)
    with pytest.raises(RuntimeError, match="outside"):
        ctx.create_morph(40, 0, None, inside.targets)
    with pytest.raises(RuntimeError, match="targets"):
        ctx.create_morph(inside.first, inside.count, None, [])
    vertices, dp, dn, db = inside.targets[0]
    swapped = vertices.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    beyond = vertices.copy()
    beyond[-1] = inside.count
    for bad in (swapped, beyond):
        with pytest.raises(RuntimeError, match="strictly ascending"):
            ctx.create_morph(inside.first, inside.count, None, [(bad, dp, dn, db)] + inside.targets[1:])
    nan = dn.copy()
    nan[0, 1] = np.nan
    with pytest.raises(RuntimeError, match="not finite"):
        ctx.create_morph(inside.first, inside.count, None, [(vertices, dp, nan, db)] + inside.targets[1:])
    with pytest.raises(RuntimeError, match="null pointer"):
        ctx.create_morph(inside.first, inside.count, None, [(vertices, None, dn, db)])
    lights = a.light_vertices()
    over = M.seeded_set(a, lights[0], 8, 1, 1)  # begins on a vertex of the light, clear of the live set
    assert _create(ctx, over) == 2
    # -- rayhip_scene_pose --
    assert ctx.pose({mid + 1: w3}, {}) == 2 and ctx.pose({5: w3}, {}) == 2 and ctx.pose({mid: w3}, {16: identity}) == 2  # no such set / skin
    bad_w = w3.copy()
    bad_w[2] = np.inf
    with pytest.raises(RuntimeError, match="not finite"):
        ctx.pose({mid: bad_w}, {})
    c_ids, c_ptrs = (hip.C.c_int * 2)(mid, mid), (hip.C.c_void_p * 2)(w3.ctypes.data, w3.ctypes.data)
    assert gpu_lib.fn("scene_pose")(ctx._ctx, 2, c_ids, c_ptrs, 0, None, None) == 1 and b"named twice" in gpu_lib.fn("last_error")()
    assert gpu_lib.fn("scene_pose")(ctx._ctx, 1, c_ids, None, 0, None, None) == 1 and gpu_lib.fn("scene_pose")(ctx._ctx, -1, c_ids, c_ptrs, 0, None, None) == 1
    assert gpu_lib.fn("scene_pose")(ctx._ctx, 17, c_ids, c_ptrs, 0, None, None) == 1
    huge = np.array([3.0e38, 0.0, 0.0], dtype=np.float32)  # the posed positions overflow
    reached = alone.targets[0][0] + alone.first
    assert np.isin(reached, S.used_vertices(a)).any()
    with pytest.raises(RuntimeError, match="not finite"):
        ctx.pose({mid: huge}, {})
    # a set and the skin around it are posed together; a set may not straddle a skin's boundary
    sid = _create_skin(ctx, skin)
    iid = _create(ctx, inside)
    with pytest.raises(RuntimeError, match="pose them together"):
        ctx.pose({iid: w3}, {})
    with pytest.raises(RuntimeError, match="pose them together"):
        ctx.pose({mid: w3}, {sid: identity})
    with pytest.raises(RuntimeError, match="pose them together"):
        ctx.pose_skins({sid: identity})
    assert ctx.destroy_morph(iid) == 0 and ctx.destroy_morph(iid) == 2 and ctx.pose({iid: w3}, {sid: identity}) == 2
    across = M.seeded_set(a, skin.first + skin.count - 12, 12, 1, 2)
    assert ctx.destroy_skin(sid) == 0
    short = S.Skin(a, skin.first, skin.count - 5, 3, 4)  # ends inside `across`
    xid, sid = _create(ctx, across), _create_skin(ctx, short)
    with pytest.raises(RuntimeError, match="straddles"):
        ctx.pose({xid: M.seeded_weights(1, 1)}, {sid: identity})
    assert _same(_accel(ctx), unposed[1])
    assert np.array_equal(_frames(ctx), unposed[0])
    # with no set alive inside it, pose_skins behaves as before
    assert ctx.destroy_morph(xid) == 0 and ctx.pose_skins({sid: S.palette(3, 9, ext)}) == 0
    assert np.array_equal(bits(ctx.read_accel(4)), bits(S.host_posed(a, [short], [S.palette(3, 9, ext)])))
    # sixteen sets are live at most; handles are distinct and never reused; an upload discards them all
    ctx.upload_scene_blob(blob)
    assert ctx.pose({mid: w3}, {}) == 2
    free = [i for i in range(len(a.vertices)) if i not in lights][:17]
    one = [(np.zeros(1, dtype=np.uint32), np.full((1, 3), 0.01, dtype=np.float32), None, None)]
    many = [ctx.create_morph(i, 1, None, one) for i in free[:16]]
    assert len(set(many)) == 16 and min(many) >= 16 and mid not in many and iid not in many and xid not in many
    with pytest.raises(RuntimeError, match="live already"):
        ctx.create_morph(free[16], 1, None, one)
    assert _same(_accel(ctx), unposed[1]) and np.array_equal(_frames(ctx), unposed[0])
    assert ctx.pose({many[3]: [1.0]}, {}) == 0 and not _same(_accel(ctx), unposed[1])
    ctx.upload_scene_blob(blob)
    assert ctx.pose({many[3]: [1.0]}, {}) == 2 and ctx.destroy_morph(many[3]) == 2
    again = _create(ctx, alone)
    assert again >= 16 and again not in many and again != mid and ctx.pose({again: w3}, {}) == 0
    # the 8-wide tree is built on the host only
    monkeypatch.setenv("RAYHIP_BVH_WIDTH", "8")
    wide = _context(gpu_lib, blob)
    monkeypatch.delenv("RAYHIP_BVH_WIDTH")
    assert wide.bvh_width() == 8
    wide_first = _frames(wide)
    assert _create(wide, alone) == 2 and wide.pose({16: w3}, {}) == 2
    assert np.array_equal(_frames(wide), wide_first)


def test_a_set_over_the_vertices_of_a_triangle_light(gpu_lib, fixture_scene):
    blob, a, _ = fixture_scene
    lights = a.light_vertices()
    first, count = lights[0] - 3, len(lights) + 8
    assert set(lights) <= set(range(first, first + count))
    rng = np.random.RandomState(3)
    every = np.arange(count, dtype=np.uint32)
    ms = M.MorphSet(a, first, count, [M._target(rng, every, S.extent(a), 1.0), M._target(rng, every[::2], S.extent(a), 1.0, with_frame=False)])
    w = np.array([1.5, -0.5], dtype=np.float32)
    off = _context(gpu_lib, blob)
    before = _accel(off, (0, 1, 2, 4, 5, 6, 7))
    assert _create(off, ms) == 2 and _same(_accel(off, (0, 1, 2, 4, 5, 6, 7)), before)  # the switch is off: lights are not rebuilt by a pose
    ctx, other = _context(gpu_lib, blob, refit=True), _context(gpu_lib, blob, refit=True)
    mid = _create(ctx, ms)
    assert mid >= 16 and ctx.pose({mid: w}, {}) == 0
    want = M.host_morphed(a, [ms], [w])
    assert not np.array_equal(bits(want["p"][lights]), bits(a.vertices["p"][lights]))
    assert other.update_vertices(0, want) == 0
    assert _same(_accel(ctx, (0, 1, 2, 4, 5, 6, 7)), _accel(other, (0, 1, 2, 4, 5, 6, 7)))
    assert not np.array_equal(bits(ctx.read_accel(5)), bits(before[4]))
    assert np.array_equal(_frames(ctx), _frames(other))
    with pytest.raises(RuntimeError, match="covers vertex"):
        ctx.refit_lights(False)
    assert ctx.destroy_morph(mid) == 0 and ctx.refit_lights(False) == 0
