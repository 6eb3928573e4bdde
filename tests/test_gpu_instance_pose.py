"""Moving instances on the device (rayhip_scene_set_instance_transforms and its _device form): transforms in; inverses, the world
boxes of every live slot and the top level out (ray_amd/csrc/instances.h, instances.hip.h).

What is asserted: the instance array and the leaves of the top level equal the host build of the same element functions
(tests/hostsim/hostsim_instances.cpp) bit for bit; arrays and frames equal those of a context that got the same scene through
rayhip_scene_update_instances, and frames those of a fresh upload (tests/test_instance_pose_hostsim.py holds the tie check that
licenses this); the direct entry of a one-instance scene follows; launches of 1 to 296 entries; the device-pointer form; every
refusal leaves arrays and frames as they were; triangle lights follow with rayhip_scene_refit_lights on; and a move commutes with a
pose."""
import os

import numpy as np
import pytest
import torch  # noqa: F401  (FIRST: torch brings its own HIP runtime, and it must be the one that opens the device -- tests/test_gpu_comm.py)

import instance_pose_cases as IP
import light_refit_cases as L
import skin_cases as S
import util
import vertex_update_cases as V
from ray_amd import api, hip, scenes

pytestmark = [pytest.mark.gpu]

W, H, SPP = 64, 48, 3
bits = IP.bits
SCENE = "cornell_instances"


@pytest.fixture(scope="module")
def gpu_lib():
    lib = hip.Library()
    assert lib.device_count() > 0, "no HIP device: the product has no CPU path, -m gpu tests cannot run here"
    assert os.path.exists(IP.INSTANCES_LIB) and V.have_refit_lib() and S.have_skin_lib() and L.have_lights_lib(), \
        "tests/hostsim is not built (run __graft_entry__.build())"
    return lib


def _need_host_lib():
    if not os.path.exists(api.HIP_HOST_LIB):
        pytest.skip("libray_hip.so not built (needs the reference tree at build time)")


def _context(lib, blob=None, refit=False):
    ctx = hip.Context(0, lib)
    ctx.upload_static(util.pmj())
    ctx.resize(W, H)
    if refit:
        ctx.refit_lights(True)  # (before the upload: the upload prepares the tables)
    if blob is not None:
        ctx.upload_scene_blob(blob)
    return ctx


def _frames(ctx):
    ctx.clear()
    return util.render_frames(ctx, SPP).copy()


def _on_device(array):
    t = torch.from_numpy(np.ascontiguousarray(array).view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return t


def _state(ctx):
    return ctx.read_accel(8).copy(), ctx.read_accel(3).copy()


def _same_state(x, y):
    return x[0].tobytes() == y[0].tobytes() and np.array_equal(x[1], y[1])


def _expected(ctx, a, flags, slots, xforms, pin_lights=True):
    """(instance array, top-level leaves) the device must hold after the call, by the host build: from the device's own records and root
    nodes as they are before it"""
    rc, mi, findings = IP.host_pose(ctx.read_accel(8), flags, slots, xforms, pin_lights)
    assert rc == 0, findings
    return mi, IP.leaves_of(a, mi, nodes=ctx.read_accel(0))


def _holds(ctx, want):
    got = ctx.read_accel(8)
    assert got.dtype == hip.MESH_INSTANCE_DTYPE and got.tobytes() == want[0].tobytes()
    # (a lone instance: the device builder's root holds it twice, the second time behind a far-away point box, and the hook returns the
    # union of the two -- the slot and the lower corner are the leaf's)
    words = 4 if len(want[1]) == 1 else 7
    assert np.array_equal(ctx.read_accel(3)[:, :words], want[1][:, :words])


@pytest.fixture(scope="module")
def scene():
    blob = util.golden_scene(SCENE)
    a = V.Arrays(blob)
    flags, lamps = IP.slot_flags(a), IP.light_slots(a)
    free = [s for s in a.live_instances() if s not in lamps]
    assert len(a.live_instances()) == 7 and len(lamps) == 1 and len(free) == 6
    return blob, a, flags, lamps[0], free


@pytest.fixture(scope="module")
def unmoved(gpu_lib, scene):
    """(frames, instance array, leaves) of the scene as uploaded: computed once, never changed"""
    ctx = _context(gpu_lib, scene[0])
    return (_frames(ctx),) + _state(ctx)


def test_arrays_equal_the_host_build(gpu_lib, scene, unmoved):
    """three slots named in descending order; the records nobody named keep their bytes"""
    blob, a, flags, lamp, free = scene
    ctx = _context(gpu_lib, blob)
    slots = sorted(free, reverse=True)[:3]
    x = IP.gentle_xforms(a, slots, seed=1)
    want = _expected(ctx, a, flags, slots, x)
    assert ctx.set_instance_transforms(slots, x) == 0
    _holds(ctx, want)
    got = ctx.read_accel(8)
    assert np.array_equal(bits(got["xform"][slots]), bits(x)) and np.array_equal(bits(got["inv_xform"][slots]), bits(IP.numpy_inverse(x)))
    rest = [s for s in range(len(got)) if s not in slots]
    assert got[rest].tobytes() == unmoved[1][rest].tobytes() and got.tobytes() != unmoved[1].tobytes()
    for field in ("mesh_index", "node_index", "lights_index", "ray_visibility"):
        assert np.array_equal(got[field], unmoved[1][field])
    assert ctx.set_instance_transforms([], np.zeros((0, 16), dtype=np.float32)) == 0  # n == 0: nothing happens
    _holds(ctx, want)


def test_arrays_and_frames_equal_an_instance_update_and_a_fresh_upload(gpu_lib, scene, unmoved):
    blob, a, flags, lamp, free = scene
    slots = [free[4], free[0], free[2]]
    x = IP.gentle_xforms(a, slots, seed=2)
    moved = IP.moved_blob(blob, a, slots, x)
    ctx, other = _context(gpu_lib, blob), _context(gpu_lib, blob)
    assert ctx.set_instance_transforms(slots, x) == 0 and other.update_instances(moved) == 0
    assert np.array_equal(ctx.read_accel(3), other.read_accel(3))
    assert np.array_equal(bits(ctx.read_accel(8)["xform"]), bits(other.read_accel(8)["xform"]))
    assert np.array_equal(bits(ctx.read_accel(8)["inv_xform"]), bits(other.read_accel(8)["inv_xform"]))
    frames = _frames(ctx)
    assert np.array_equal(frames, _frames(other))
    assert np.array_equal(frames, _frames(_context(gpu_lib, moved)))
    assert not np.array_equal(frames, unmoved[0])


def test_the_transforms_in_place_change_nothing(gpu_lib, scene, unmoved):
    """every live slot -- the one with the lamp too: a transform bytewise equal to the one in place passes -- named with what it has"""
    blob, a, flags, lamp, free = scene
    ctx = _context(gpu_lib, blob)
    live = a.live_instances()
    want = _expected(ctx, a, flags, live, a.mesh_instances["xform"][live])
    assert ctx.set_instance_transforms(live, a.mesh_instances["xform"][live]) == 0
    assert ctx.read_accel(8).tobytes() == unmoved[1].tobytes()
    # (the leaves are this call's boxes now: an ulp or two from the ones the scene build stored, which the upload took --
    # tests/test_vertex_update_hostsim.py::test_instance_boxes_against_the_scene_build.  Each bound is six float32 roundings of values
    # below 1.3 in this room from the exact one, so two of them lie within 12 x 2^-24 x 1.3 < 2^-20 of each other)
    _holds(ctx, want)
    assert np.abs(ctx.read_accel(3)[:, 1:].view(np.float32) - unmoved[2][:, 1:].view(np.float32)).max() <= 2.0 ** -20
    assert np.array_equal(_frames(ctx), unmoved[0])


def test_the_direct_entry_follows(gpu_lib):
    """cornell_basic: ONE instance, whose record the direct-entry kernels take from their arguments -- a launch that kept the old
    inv_xform there would render the old frame.  Its lamp is part of the one mesh, so the lights are refitted, and the fresh upload it
    is held against gets the refitted tree (the form of test_gpu_light_refit.py::test_frames_equal_a_fresh_upload_with_the_refitted_tree)."""
    blob = util.golden_scene("cornell_basic")
    a = V.Arrays(blob)
    assert a.live_instances() == [0] and IP.light_slots(a) == [0]
    ctx = _context(gpu_lib, blob, refit=True)
    assert ctx.direct_entry() == 1
    first = _frames(ctx)
    x = IP.gentle_xforms(a, [0], seed=3, shift=0.03, turn_deg=8.0)
    assert _context(gpu_lib, blob).set_instance_transforms([0], x) == 2  # (the lights are pinned while they are not refitted)
    want = _expected(ctx, a, IP.slot_flags(a), [0], x, pin_lights=False)
    assert ctx.set_instance_transforms([0], x) == 0
    _holds(ctx, want)
    assert ctx.direct_entry() == 1
    moved = _frames(ctx)
    fresh = _context(gpu_lib, L.with_section(IP.moved_blob(blob, a, [0], x), "light_cwnodes", ctx.read_accel(5).copy()))
    assert fresh.direct_entry() == 1
    assert np.array_equal(moved, _frames(fresh)) and not np.array_equal(moved, first)


def test_lanes_and_blocks(gpu_lib):
    """instance_field(300): 301 slots, five of them lamps.  Calls of 1, 64, 65, 256, 257 and all 296 other slots -- one lane, a whole
    wavefront, one more, a whole block, one more, two blocks with a ragged end -- each held against the host build"""
    _need_host_lib()
    s = api.CreateSceneHIP()
    scenes.instance_field(s, 300)
    blob = api.export_scene_blob(s)
    a = V.Arrays(blob)
    flags, lamps = IP.slot_flags(a), IP.light_slots(a)
    free = [m for m in a.live_instances() if m not in lamps]
    assert len(a.live_instances()) == 301 and len(lamps) == 5 and len(free) == 296  # (in a pool of 512 slots)
    ctx = _context(gpu_lib, blob)
    rng = np.random.RandomState(9)
    for k, n in enumerate((1, 64, 65, 256, 257, len(free))):
        slots = [free[i] for i in rng.permutation(len(free))[:n]]
        now = V.Arrays(blob)
        now.mesh_instances = ctx.read_accel(8).copy()  # (gentle: relative to where the instances are now)
        x = IP.gentle_xforms(now, slots, seed=20 + k, shift=0.01)
        want = _expected(ctx, a, flags, slots, x)
        assert ctx.set_instance_transforms(slots, x) == 0, n
        _holds(ctx, want)
    assert np.isfinite(_frames(ctx)).all()


def test_the_device_form(gpu_lib, scene):
    """slots and matrices in a tensor on the device: the arrays of the host form in a sibling context.  Once 16-byte aligned (the
    matrices come as 16-byte loads), once four bytes off."""
    blob, a, flags, lamp, free = scene
    slots = np.array([free[1], free[5], free[3], free[0]], dtype=np.uint32)
    x = IP.gentle_xforms(a, slots, seed=4)
    sibling = _context(gpu_lib, blob)
    assert sibling.set_instance_transforms(slots, x) == 0
    for off in (0, 4):
        ctx = _context(gpu_lib, blob)
        d_slots = _on_device(slots)
        d_x = _on_device(np.concatenate([np.zeros(off, dtype=np.uint8), x.view(np.uint8).ravel()]))
        assert d_x.data_ptr() % 16 == 0
        assert ctx.set_instance_transforms_device(len(slots), d_slots.data_ptr(), d_x.data_ptr() + off) == 0
        assert _same_state(_state(ctx), _state(sibling))
    assert np.array_equal(_frames(ctx), _frames(sibling))


def test_refusals_touch_nothing(gpu_lib, scene, unmoved, monkeypatch):
    blob, a, flags, lamp, free = scene
    ctx = _context(gpu_lib, blob)
    fn, fn_d = gpu_lib.fn("scene_set_instance_transforms"), gpu_lib.fn("scene_set_instance_transforms_device")
    good = IP.gentle_xforms(a, free[:2], seed=5)
    nan, singular = good.copy(), good.copy()
    nan[1, 13] = np.nan
    singular[0, 0:3] = 0.0  # every element finite, inv_det = inf
    d_good = _on_device(good)
    for slots, x, code in [([free[0], free[0]], good, 1), ([free[0], len(a.mesh_instances)], good, 1), ([free[0], 0xffffffff], good, 1),
                           (free[:2], nan, 1), (free[:2], singular, 1), ([free[0], lamp], good, 2)]:
        slots = np.array(slots, dtype=np.uint32)
        assert fn(ctx._ctx, 2, slots.ctypes.data, x.ctypes.data) == code, (slots, code)
        assert gpu_lib.fn("last_error")()
        d_slots, d_x = _on_device(slots), _on_device(x)
        assert fn_d(ctx._ctx, 2, d_slots.data_ptr(), d_x.data_ptr()) == code, (slots, code)
        assert _same_state(_state(ctx), unmoved[1:])
    slots = np.array(free[:2], dtype=np.uint32)
    assert fn(ctx._ctx, 2, None, good.ctypes.data) == 1 and fn(ctx._ctx, 2, slots.ctypes.data, None) == 1  # a null pointer with n > 0
    assert fn_d(ctx._ctx, 2, None, d_good.data_ptr()) == 1
    assert _same_state(_state(ctx), unmoved[1:])
    assert np.array_equal(_frames(ctx), unmoved[0])
    empty = _context(gpu_lib)  # nothing uploaded yet
    assert empty.set_instance_transforms(free[:2], good) == 2
    monkeypatch.setenv("RAYHIP_BVH_WIDTH", "8")
    wide = _context(gpu_lib, blob)
    assert wide.bvh_width() == 8 and wide.set_instance_transforms(free[:2], good) == 2
    assert wide.set_instance_transforms_device(2, _on_device(slots).data_ptr(), d_good.data_ptr()) == 2


def test_a_freed_slot_is_refused(gpu_lib):
    """cornell_instances_mutable after RemoveMeshInstance, through an instance update: the pool keeps the slot, the top level does not
    name it"""
    _need_host_lib()
    s = api.CreateSceneHIP()
    scenes.cornell_instances_mutable(s)
    before = api.export_scene_blob(s)
    scenes.mutate_instances_scene(s)
    after = api.export_scene_blob(s)
    a, b = V.Arrays(before), V.Arrays(after)
    dead = sorted(set(a.live_instances()) - set(b.live_instances()))
    assert len(dead) == 1 and dead[0] < len(b.mesh_instances)
    flags, lamps = IP.slot_flags(b), IP.light_slots(b)
    free = [m for m in b.live_instances() if m not in lamps]
    ctx = _context(gpu_lib, before)
    x = IP.gentle_xforms(a, [dead[0], free[0]], seed=6)
    assert ctx.set_instance_transforms([dead[0], free[0]], x) == 0  # (alive still)
    assert ctx.update_instances(after) == 0
    state, frames = _state(ctx), _frames(ctx)
    with pytest.raises(RuntimeError, match="not in the top level"):  # (return code 1: the wrapper raises)
        ctx.set_instance_transforms([dead[0], free[0]], x)
    assert _same_state(_state(ctx), state) and np.array_equal(_frames(ctx), frames)
    want = _expected(ctx, b, flags, [free[0]], x[1:])
    assert ctx.set_instance_transforms([free[0]], x[1:]) == 0
    _holds(ctx, want)
    assert not np.array_equal(_frames(ctx), frames)


def test_triangle_lights_follow_with_the_switch_on(gpu_lib):
    """the slot the emitter hangs on moves: corners, tree and importance rows equal the host build of the light refit under the moved
    instance array; frames equal a fresh upload with the refitted tree put in its place"""
    blob = L.scene_blob("fixture", 0)
    a = L.Arrays(blob)
    slot = int(a.lights[a.tri_lights()[0], 5])
    assert IP.light_slots(a) == [slot]
    other = [m for m in a.live_instances() if m != slot][2]
    slots = [other, slot]
    x = IP.gentle_xforms(a, slots, seed=7, shift=0.03, turn_deg=6.0)
    ctx = _context(gpu_lib, blob, refit=True)
    first = _frames(ctx)
    want = _expected(ctx, a, IP.slot_flags(a), slots, x, pin_lights=False)
    assert ctx.set_instance_transforms(slots, x) == 0
    _holds(ctx, want)
    lights = L.host_refit(a, a.vertices, instances=want[0])
    assert np.array_equal(bits(ctx.read_accel(5)), bits(lights.cwnodes)) and np.array_equal(bits(ctx.read_accel(6)), bits(lights.children))
    assert np.array_equal(bits(ctx.read_accel(7)), bits(lights.tri_geom))
    assert not np.array_equal(bits(ctx.read_accel(7)), bits(L.fill_tri_geom(a, a.vertices)))
    moved = _frames(ctx)
    fresh = _context(gpu_lib, L.with_section(IP.moved_blob(blob, a, slots, x), "light_cwnodes", ctx.read_accel(5).copy()))
    assert np.array_equal(bits(fresh.read_accel(6)), bits(ctx.read_accel(6))) and np.array_equal(bits(fresh.read_accel(7)), bits(ctx.read_accel(7)))
    assert np.array_equal(moved, _frames(fresh)) and not np.array_equal(moved, first)
    assert np.isfinite(moved).all()


def test_a_move_and_a_pose_commute(gpu_lib, scene, unmoved):
    """pose two skins, then move -- against move, then pose, in a second context: the same leaves, vertices, records and frames.  The
    leaves of the moved slots are those of the POSED trees' roots, so the boxes come from the nodes as they are on the device."""
    blob, a, flags, lamp, free = scene
    skins = S.seeded_skins(a, 3)[:2]
    palettes = [S.palette(3, 30 + k, S.extent(a)) for k in range(2)]
    slots = free[::2]
    x = IP.gentle_xforms(a, slots, seed=8)
    pose_first, move_first = _context(gpu_lib, blob), _context(gpu_lib, blob)
    ids = [c.create_skin(s.first, s.rest, s.indices, s.weights, s.bones_count) for c in (pose_first, move_first) for s in skins]
    assert pose_first.pose_skins(dict(zip(ids[:2], palettes))) == 0
    want = _expected(pose_first, a, flags, slots, x)
    assert pose_first.set_instance_transforms(slots, x) == 0
    _holds(pose_first, want)
    assert move_first.set_instance_transforms(slots, x) == 0
    unposed_leaves = move_first.read_accel(3).copy()
    assert move_first.pose_skins(dict(zip(ids[2:], palettes))) == 0
    assert _same_state(_state(pose_first), _state(move_first))
    assert not np.array_equal(pose_first.read_accel(3), unposed_leaves)  # (the pose changed a root box: the move read the refitted one)
    assert np.array_equal(S.bits(pose_first.read_accel(4)), S.bits(move_first.read_accel(4)))
    frames = _frames(pose_first)
    assert np.array_equal(frames, _frames(move_first)) and not np.array_equal(frames, unmoved[0])
