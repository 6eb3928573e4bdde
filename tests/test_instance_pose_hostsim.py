"""Moving instances, without a GPU (ray_amd/csrc/instances.h compiled for the host: tests/hostsim/hostsim_instances.cpp): the inverse
is the one the reference's scene build stores, bit for bit; the world boxes are the vertex update's, bit for bit; every refusal has
its code and writes nothing; and a scene moved this way renders the frames of the reference's moved scene (the host build of the
renderer), which is what licenses the frame equalities of tests/test_gpu_instance_pose.py."""
import os

import numpy as np
import pytest

import instance_pose_cases as IP
import oracle_lib as O
import util
import vertex_update_cases as V
from ray_amd import api, scenes


def test_the_host_build_exists():
    """(no skip in this file: __graft_entry__.build() makes the library)"""
    assert os.path.exists(IP.INSTANCES_LIB), "tests/hostsim/hostsim_instances.cpp not built (run __graft_entry__.build())"


# ---- 1: the inverse -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", V.fixture_names())
def test_inverse_equals_what_the_scene_build_stored(name):
    a = V.Arrays(util.golden_scene(name))
    live = a.live_instances()
    assert live
    got = IP.host_inverse(a.mesh_instances["xform"][live])
    assert np.array_equal(IP.bits(got), IP.bits(a.mesh_instances["inv_xform"][live]))


def test_every_fixture_instance_is_covered():
    assert sum(len(V.Arrays(util.golden_scene(n)).live_instances()) for n in V.fixture_names()) == 13


@pytest.mark.parametrize("mirrored", [False, True])
def test_inverse_equals_the_numpy_restatement(mirrored):
    x = IP.seeded_xforms(257, seed=5 + int(mirrored), mirrored=mirrored)
    det = np.linalg.det(x.reshape(-1, 4, 4).astype(np.float64))
    assert np.all(det < 0) if mirrored else np.all(det > 0)
    got = IP.host_inverse(x)
    assert np.array_equal(IP.bits(got), IP.bits(IP.numpy_inverse(x)))
    # ... and it is an inverse: against float64, to the conditioning of these matrices
    ref = np.linalg.inv(x.reshape(-1, 4, 4).astype(np.float64)).reshape(-1, 16)
    assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max()
    eye = IP.identity()[None]
    # (the identity's inverse is the identity in value; the negated cofactors make some of its zeros -0.0, as in the reference)
    assert np.array_equal(IP.host_inverse(eye), eye) and np.array_equal(IP.bits(IP.host_inverse(eye)), IP.bits(IP.numpy_inverse(eye)))


# ---- 2: the boxes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", V.fixture_names())
def test_world_boxes_equal_the_vertex_updates(name):
    """... over the fixtures' root nodes, under the transforms in place and under seeded ones"""
    a = V.Arrays(util.golden_scene(name))
    live = a.live_instances()
    assert np.array_equal(IP.bits(IP.host_world_boxes(a.nodes, a.mesh_instances, live)), IP.bits(V.instance_boxes(a.nodes, a.mesh_instances, live)))
    mi = IP.moved_instances(a, live, IP.seeded_xforms(len(live), seed=11, mirrored=True))
    assert np.array_equal(IP.bits(IP.host_world_boxes(a.nodes, mi, live)), IP.bits(V.instance_boxes(a.nodes, mi, live)))


@pytest.mark.parametrize("name", V.fixture_names())
def test_world_boxes_hold_what_the_scene_build_stored(name):
    """the containment check of test_vertex_update_hostsim.py::test_instance_boxes_against_the_scene_build, with its slack: each box
    holds the float64 transforms of the vertices of its instance up to six float32 roundings -- and lies that close to the box the
    scene build stored for the slot"""
    a = V.Arrays(util.golden_scene(name))
    live = a.live_instances()
    boxes = IP.host_world_boxes(a.nodes, a.mesh_instances, live)
    stored = a.top_level_leaves()
    for k, mi in enumerate(live):
        inst = a.mesh_instances[mi]
        ranges, stack = [], [int(inst["node_index"])]
        while stack:
            for link in a.nodes[stack.pop(), 12:14]:
                if link & V.COUNT_BITS:
                    ranges.extend(range(link & V.INDEX_BITS, (link & V.INDEX_BITS) + ((link & V.COUNT_BITS) >> 29) + 1))
                else:
                    stack.append(int(link))
        t = a.tri_indices[ranges].astype(np.int64)
        p = a.vertices["p"][np.unique(np.concatenate([a.vtx_indices[3 * t], a.vtx_indices[3 * t + 1], a.vtx_indices[3 * t + 2]]))].astype(np.float64)
        m = inst["xform"].astype(np.float64).reshape(4, 4)
        world = p @ m[:3, :3] + m[3, :3]
        slack = 6 * 2.0 ** -24 * (np.abs(p) @ np.abs(m[:3, :3]) + np.abs(m[3, :3])).max(axis=0)
        lo, hi = world.min(axis=0), world.max(axis=0)
        print(f"{name} slot {mi}: bit-equal to the stored box {bool(np.array_equal(IP.bits(boxes[k]), IP.bits(stored[mi])))}, "
              f"apart by at most {float(np.abs(boxes[k].astype(np.float64) - stored[mi]).max()):.3g}")
        assert np.all(lo >= boxes[k][:3] - slack) and np.all(hi <= boxes[k][3:] + slack), mi
        assert np.all(lo >= stored[mi][:3] - slack) and np.all(hi <= stored[mi][3:] + slack), mi


# ---- 3: validation --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    a = V.Arrays(util.golden_scene("cornell_instances"))
    flags = IP.slot_flags(a)
    lamps = IP.light_slots(a)
    assert len(a.live_instances()) == 7 and len(lamps) == 1
    return a, flags, lamps[0], [s for s in a.live_instances() if s != lamps[0]]


def _refused(scene, slots, xforms, code, finding, pin_lights=True, flags=None):
    a, f, _, _ = scene
    rc, mi, findings = IP.host_pose(a.mesh_instances, f if flags is None else flags, slots, xforms, pin_lights)
    assert rc == code, (rc, findings)
    assert findings[finding] >= 1
    assert mi.tobytes() == a.mesh_instances.tobytes()  # nothing was written


def test_an_accepted_call_writes_the_named_records_only(scene):
    a, flags, lamp, free = scene
    slots = free[::-1][:3]  # descending
    x = IP.seeded_xforms(3, seed=2)
    rc, mi, findings = IP.host_pose(a.mesh_instances, flags, slots, x)
    assert rc == 0 and not findings.any()
    assert np.array_equal(IP.bits(mi["xform"][slots]), IP.bits(x)) and np.array_equal(IP.bits(mi["inv_xform"][slots]), IP.bits(IP.numpy_inverse(x)))
    rest = [s for s in range(len(mi)) if s not in slots]
    assert mi[rest].tobytes() == a.mesh_instances[rest].tobytes()
    for field in ("mesh_index", "node_index", "lights_index", "ray_visibility"):
        assert np.array_equal(mi[field], a.mesh_instances[field])
    rc, _, _ = IP.host_pose(a.mesh_instances, flags, [], np.zeros((0, 16), dtype=np.float32))
    assert rc == 0


def test_bad_slots_are_refused(scene):
    a, flags, lamp, free = scene
    x = IP.seeded_xforms(2, seed=3)
    _refused(scene, [free[0], len(a.mesh_instances)], x, 1, IP.BAD_SLOT)  # outside the array
    _refused(scene, [free[0], 0xffffffff], x, 1, IP.BAD_SLOT)
    dead = flags.copy()
    dead[free[1]] &= ~np.uint8(IP.SLOT_LIVE)  # a freed slot of the pool: the top level does not name it
    _refused(scene, [free[0], free[1]], x, 1, IP.BAD_SLOT, flags=dead)
    _refused(scene, [free[0], free[0]], x, 1, IP.DUPLICATE)
    assert IP.instances_lib().hostsim_pose_instances(None, 0, None, 1, 2, None, None, None) == 1  # null pointers with n > 0


def test_bad_matrices_are_refused(scene):
    a, flags, lamp, free = scene
    for bad in (np.nan, np.inf, -np.inf):
        x = IP.seeded_xforms(2, seed=4)
        x[1, 6] = bad
        assert not IP.host_finite16(x[1]) and IP.host_finite16(x[0])
        _refused(scene, free[:2], x, 1, IP.NOT_FINITE)
    x = IP.seeded_xforms(2, seed=4)
    x[0, 0:3] = 0.0  # a singular matrix: every element finite, inv_det = inf
    assert IP.host_finite16(x[0]) and not np.isfinite(IP.host_inverse(x[0])).all()
    _refused(scene, free[:2], x, 1, IP.NOT_FINITE)


def test_a_slot_with_triangle_lights_is_pinned_while_the_lights_are_not_refitted(scene):
    a, flags, lamp, free = scene
    x = IP.seeded_xforms(2, seed=6)
    _refused(scene, [free[0], lamp], x, 2, IP.PINNED)
    _refused(scene, [lamp, lamp], x, 1, IP.DUPLICATE)  # (an error outranks the need for an upload)
    x[1] = a.mesh_instances["xform"][lamp]  # the transform in place, bytewise: passes
    rc, mi, findings = IP.host_pose(a.mesh_instances, flags, [free[0], lamp], x)
    assert rc == 0 and not findings.any()
    assert mi[lamp].tobytes() == a.mesh_instances[lamp].tobytes()  # (the fixture's inverse is this function's: test 1)
    x[1] = IP.seeded_xforms(1, seed=7)[0]
    rc, mi, findings = IP.host_pose(a.mesh_instances, flags, [free[0], lamp], x, pin_lights=False)  # the switch is on: it moves
    assert rc == 0 and np.array_equal(IP.bits(mi["xform"][lamp]), IP.bits(x[1]))


# ---- 4: against the reference ------------------------------------------------------------------------------------------------------------
def _need_host_lib():
    if not os.path.exists(api.HIP_HOST_LIB):
        pytest.skip("libray_hip.so not built (needs the reference tree at build time)")


def _moved_by_the_reference(name):
    """(blob before, blob after SetMeshInstanceTransform + Finalize, slots moved): no instance or light comes or goes"""
    s = api.CreateSceneHIP()
    if name == "cornell_instances_mutable":
        scenes.cornell_instances_mutable(s)
        before = api.export_scene_blob(s)
        h = s._test_handles
        s.SetMeshInstanceTransform(h["scaled"], scenes._xform(translate=(-0.33, 0.05, 0.05), rot_y_deg=-15.0, scale=(0.5, 1.5, 0.7)))
        s.SetMeshInstanceTransform(h["hidden"], scenes._xform(translate=(0.10, 0.22, -0.14), rot_y_deg=50.0, rot_z_deg=-10.0, scale=(0.4, 0.6, 0.5)))
        s.Finalize()
    else:
        scenes.instance_field(s, 300)
        before = api.export_scene_blob(s)
        scenes.move_instance_field(s)
    after = api.export_scene_blob(s)
    a, b = V.Arrays(before), V.Arrays(after)
    assert a.live_instances() == b.live_instances() and len(a.mesh_instances) == len(b.mesh_instances)
    moved = [m for m in a.live_instances() if a.mesh_instances["xform"][m].tobytes() != b.mesh_instances["xform"][m].tobytes()]
    return before, after, moved


@pytest.mark.parametrize("name", ["cornell_instances_mutable", "instance_field_300"])
def test_records_equal_the_references(name):
    """SetMeshInstanceTransform + Finalize through the reference: the exported xform / inv_xform are the host build's, bit for bit"""
    _need_host_lib()
    before, after, moved = _moved_by_the_reference(name)
    a, b = V.Arrays(before), V.Arrays(after)
    assert len(moved) == (2 if name == "cornell_instances_mutable" else 300)
    mi = IP.moved_instances(a, moved, b.mesh_instances["xform"][moved])
    assert mi.tobytes() == b.mesh_instances.tobytes()


@pytest.mark.parametrize("name", ["cornell_instances_mutable", "instance_field_300"])
def test_a_moved_scene_renders_the_frames_of_the_references(name):
    """the tie check, as test_a_refitted_scene_renders_the_frames_of_a_fresh_one: the reference's moved scene (its boxes, its top
    level) against the scene carrying this call's boxes.  A BVH only culls, so frames differ only where two hits tie at the same
    distance; these scenes have no such pixel at this size."""
    _need_host_lib()
    if not O.have_hostsim() or not O.have_ref():
        pytest.skip("tests/hostsim or the oracle not built")
    before, after, moved = _moved_by_the_reference(name)
    a, b = V.Arrays(before), V.Arrays(after)
    if name == "cornell_instances_mutable":
        # no light hangs on a moved slot: the scene BEFORE with this call's records and boxes is the whole moved scene
        ours = IP.moved_blob(before, a, moved, b.mesh_instances["xform"][moved])
    else:
        # the lamps moved, and their lights with them: the reference's arrays, the top level with this call's boxes
        ours = IP.moved_blob(after, b, [], np.zeros((0, 16), dtype=np.float32))
    assert V.Arrays(ours).mesh_instances.tobytes() == b.mesh_instances.tobytes()
    w, h, spp = 64, 48, 2
    got = util.render_frames(O.hostsim_context(w, h, ours, util.pmj()), spp)
    ref = util.render_frames(O.hostsim_context(w, h, after, util.pmj()), spp)
    old = util.render_frames(O.hostsim_context(w, h, before, util.pmj()), spp)
    assert not np.array_equal(ref, old)
    differing = int((np.abs(got - ref).max(axis=-1) > 0).sum())
    print("pixels differing from the reference's moved scene:", differing)
    assert differing == 0
