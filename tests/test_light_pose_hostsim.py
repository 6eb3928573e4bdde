"""Moving and recolouring analytic lights, without a GPU (ray_amd/csrc/light_pose.h and the `posed` table of light_refit.h compiled for
the host: tests/hostsim/hostsim_light_pose.cpp): the flux, axis and cosine words a posed leaf gets are the ones the reference's scene
build stores for the same record, bit for bit; the numpy packers make the records the reference's AddLight makes; a numpy restatement
agrees with the host build; an identity call is a plain refit; and every refusal has its code, its counter and writes nothing.
tests/test_gpu_light_pose.py holds the device against this host build."""
import os

import numpy as np
import pytest

import light_pose_cases as P
import light_refit_cases as L
import util
from ray_amd import api, scenes

bits = L.bits


def test_the_host_build_exists():
    """(no skip for it in this file: __graft_entry__.build() makes the library)"""
    assert os.path.exists(P.POSE_LIB), "tests/hostsim/hostsim_light_pose.cpp not built (run __graft_entry__.build())"


def _need_host_lib():
    if not os.path.exists(api.HIP_HOST_LIB):
        pytest.skip("libray_hip.so not built (needs the reference tree at build time)")


def _random_cornell_blob(seed):
    key = ("random_cornell", seed)
    if key not in L._blobs:
        s = api.CreateSceneHIP()
        scenes.random_cornell(s, seed)
        L._blobs[key] = api.export_scene_blob(s)
    return L._blobs[key]


def _blob(name):
    if name == "cornell_instances":
        return util.golden_scene(name)
    _need_host_lib()
    if name == "cornell_lights":
        return P.cornell_blob()
    if name == "light_field_130":
        return P.field_blob(130)
    return _random_cornell_blob(int(name.rsplit("_", 1)[1]))


IDENTITY_SCENES = ["cornell_lights", "cornell_instances", "light_field_130"] + [f"random_cornell_{k}" for k in range(8)]


# ---- 1: identity against the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IDENTITY_SCENES)
def test_posed_leaf_words_equal_the_scene_builds(name):
    """every analytic light named with the record it holds: the flux, axis and cosine words its leaf slot gets from its summary are the
    words the reference-built tree holds there"""
    a = L.Arrays(_blob(name))
    slots = P.analytic_slots(a)
    if not slots:
        return
    rc, findings, after = P.host_set_lights(P.State(a), slots, a.lights[slots])
    assert rc == 0 and not findings.any()
    paths = L.paths(a.cwnodes)
    for s in slots:
        want, got = P.leaf_words(a.cwnodes, paths, s), P.leaf_words(after.cwnodes, paths, s)
        assert got == want, (name, s, int(a.lights[s, 0] & 7), [hex(x) for x in got], [hex(x) for x in want])
    assert after.posed[slots].all() and after.posed.sum() == len(slots)


def test_the_identity_scenes_cover_every_kind():
    """sphere, directional, line, rect and disk lights all occur, spot lights among the spheres"""
    _need_host_lib()
    kinds = []
    for name in IDENTITY_SCENES:
        a = L.Arrays(_blob(name))
        kinds += [int(a.lights[s, 0] & 7) if a.lights[s:s + 1, 12].view(np.float32)[0] < 0 or a.lights[s, 0] & 7 else "spot" for s in P.analytic_slots(a)]
    assert set(kinds) == {P.TYPE_SPHERE, "spot", P.TYPE_DIR, P.TYPE_LINE, P.TYPE_RECT, P.TYPE_DISK}
    assert len(kinds) == 152


# ---- 2: moved lights ---------------------------------------------------------------------------------------------------------------
def _moved_records(base: L.Arrays, moved: L.Arrays, kinds):
    """(slots, records): the numpy packers' records of the moved lights of `kinds`; the directional record from the reference's scene"""
    slot_of = P.cornell_slots(base)
    slots = [slot_of[k] for k in kinds]
    records = [moved.lights[slot_of[k]] if k == "directional" else P.pack(k, base.lights[slot_of[k], 0], **P.CORNELL_MOVES[k]) for k in kinds]
    return np.array(slots, dtype=np.uint32), np.array(records, dtype=np.uint32)


@pytest.mark.parametrize("kinds", [[k] for k in P.KINDS] + [P.KINDS], ids=P.KINDS + ["all"])
def test_moved_lights_against_the_reference(kinds):
    """cornell_lights with one light of each kind, then all six, moved, turned, resized and recoloured through the reference's scene
    build: the packed records are the reference's; after the host set_lights the leaf words of each named light are those of the
    reference's freshly built tree; and the root box is the reference's root box.

    Root boxes: measured equal to the bit in all seven cases (the root's box is a min / max union of the lights' boxes on both
    sides), so it is asserted."""
    _need_host_lib()
    base, moved = L.Arrays(P.cornell_blob()), L.Arrays(P.cornell_blob(kinds))
    named = np.sort(base.li_indices)  # (the light array is a pool: a free slot holds anything)
    assert np.array_equal(named, np.sort(moved.li_indices)) and np.array_equal(base.lights[named, 0], moved.lights[named, 0])
    slots, records = _moved_records(base, moved, kinds)
    assert np.array_equal(records, moved.lights[slots]), [k for k, r, s in zip(kinds, records, slots) if not np.array_equal(r, moved.lights[s])]
    assert not any(np.array_equal(base.lights[s], moved.lights[s]) for s in slots)
    rc, findings, after = P.host_set_lights(P.State(base), slots, records)
    assert rc == 0 and not findings.any()
    assert np.array_equal(after.lights[named], moved.lights[named])
    ours, theirs = L.paths(after.cwnodes), L.paths(moved.cwnodes)
    for k, s in zip(kinds, slots):
        got, want = P.leaf_words(after.cwnodes, ours, int(s)), P.leaf_words(moved.cwnodes, theirs, int(s))
        assert got == want, (k, [hex(x) for x in got], [hex(x) for x in want])
    same_root = np.array_equal(bits(after.cwnodes["bbox_min"][0]), bits(moved.cwnodes["bbox_min"][0])) and \
        np.array_equal(bits(after.cwnodes["bbox_max"][0]), bits(moved.cwnodes["bbox_max"][0]))
    print("root box equal to the reference's, bit for bit:", same_root, after.cwnodes["bbox_min"][0], moved.cwnodes["bbox_min"][0],
          after.cwnodes["bbox_max"][0], moved.cwnodes["bbox_max"][0])
    assert same_root


# ---- 3: numpy restatement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_lights", "light_field_130"])
def test_the_numpy_restatement_equals_the_host_build(name):
    """lights, leaf table, light_cwnodes and light_children after a call that moves every analytic light.  The restatement makes the
    records' summaries and the three words of their leaf slots; with those written into the tree, the level refit as it was before this
    call existed (tests/hostsim/hostsim_lights.cpp, which knows no posed lights and keeps such words bytewise) must leave the arrays
    the host build of the call leaves -- so every word the `posed` table adds is held against numpy."""
    _need_host_lib()
    if name == "cornell_lights":
        base, moved = L.Arrays(P.cornell_blob()), L.Arrays(P.cornell_blob(P.KINDS))
        slots, records = _moved_records(base, moved, P.KINDS)
    else:
        base = L.Arrays(P.field_blob(130))
        slots, records = P.field_records(base, 130)
    state = P.State(base)
    rc, findings, after = P.host_set_lights(state, slots, records)
    assert rc == 0 and not findings.any()
    summaries = P.np_summaries(records)
    assert np.array_equal(bits(summaries), bits(P.host_summaries(records)))
    lights, leaf, cwnodes = state.lights.copy(), state.leaf.copy(), state.cwnodes.copy()
    lights[slots], leaf[slots] = records, summaries
    paths = L.paths(cwnodes)
    for s, r in zip(slots, records):
        w, i = paths[int(s)][-1]
        flux, axis, cosines = P.np_leaf_words(r)
        cwnodes["flux"][w, i:i + 1] = np.array([flux], dtype=np.uint32).view(np.float32)
        cwnodes["axis"][w, i], cwnodes["cos_omega_ne"][w, i] = axis, cosines
    children = state.children.copy()
    scratch = np.zeros(len(cwnodes), dtype=L.SUMMARY)
    lights = np.ascontiguousarray(lights)
    assert L.lights_lib().hostsim_refit_light_nodes(cwnodes.ctypes.data, len(cwnodes), lights.ctypes.data, len(lights), leaf.ctypes.data, scratch.ctypes.data,
                                                    children.ctypes.data, state.scales.ctypes.data) == 0
    assert np.array_equal(lights, after.lights) and np.array_equal(bits(leaf), bits(after.leaf))
    assert np.array_equal(bits(cwnodes), bits(after.cwnodes)) and np.array_equal(bits(children), bits(after.children))
    assert not np.array_equal(bits(after.cwnodes), bits(state.cwnodes))


# ---- 4: an identity call -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_lights", "cornell_instances", "light_field_130"])
def test_an_identity_call_is_a_plain_refit(name):
    a = L.Arrays(_blob(name))
    state = P.State(a)
    plain = P.host_refit_posed(state, posed=False)
    slots = P.analytic_slots(a)
    rc, findings, after = P.host_set_lights(state, slots, a.lights[slots])
    assert rc == 0 and not findings.any()
    for k in ("lights", "cwnodes", "children", "leaf"):
        assert np.array_equal(bits(after.arrays()[k]), bits(plain.arrays()[k])), k
    # naming some: the others keep their three words bytewise, posed or not
    some = slots[::2]
    rc, _, half = P.host_set_lights(state, some, a.lights[some])
    assert rc == 0 and half.posed.sum() == len(some)
    paths = L.paths(a.cwnodes)
    for s in slots:
        assert P.leaf_words(half.cwnodes, paths, s) == P.leaf_words(a.cwnodes, paths, s)
    # an all-zero table is no table
    assert P.host_refit_posed(state, posed=True).same(plain)


# ---- 5: refusals -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def field():
    _need_host_lib()
    a = L.Arrays(P.field_blob(130))
    slots, records = P.field_records(a, 130)
    return a, P.State(a), slots, records


def _refused(state, slots, records, finding, count=None):
    rc, findings, after = P.host_set_lights(state, slots, records)
    assert rc == 1, (rc, findings)
    assert findings[finding] >= 1 and (count is None or findings[finding] == count), findings
    assert after.same(state)  # nothing was written
    return findings


def test_bad_slots_and_duplicates_are_refused(field):
    a, state, slots, records = field
    for bad in (len(state.lights), 0xffffffff):
        s = slots.copy()
        s[1] = bad
        _refused(state, s, records, P.BAD_SLOT, 1)
    dead = state.copy()
    dead.live[slots[3]] = 0  # a freed slot of the pool, a directional light baked into the sky: li_indices does not name it
    _refused(dead, slots, records, P.BAD_SLOT, 1)
    for first, second in ((0, 1), (0, 64), (63, 64), (5, 129)):  # at distance 1 and across a wavefront boundary
        s, r = slots.copy(), records.copy()
        s[second], r[second] = s[first], r[first]  # (the record with it: only the slot is wrong with the entry)
        f = _refused(state, s, r, P.DUPLICATE, 1)
        assert f.sum() == 1
    s, r = slots.copy(), records.copy()
    s[[10, 20, 30]], r[[10, 20, 30]] = s[0], r[0]
    assert _refused(state, s, r, P.DUPLICATE, 3).sum() == 3
    assert P.pose_lib().hostsim_set_lights(None, 0, None, None, None, None, 0, None, None, None, 2, None, None, np.zeros(5, dtype=np.uint32).ctypes.data) == 1
    rc, findings, after = P.host_set_lights(state, [], np.zeros((0, 16), dtype=np.uint32))  # n == 0
    assert rc == 0 and after.same(state)


def test_bad_records_are_refused(field):
    a, state, slots, records = field
    for word in range(1, 16):  # each of the 15 floats
        for bad in (np.nan, np.inf, -np.inf):
            r = records.copy()
            r[64, word] = np.array([bad], dtype=np.float32).view(np.uint32)[0]
            _refused(state, slots, r, P.NOT_FINITE, 1)
    r = records.copy()
    r[7, 0] ^= 1 << 5  # `visible`
    f = _refused(state, slots, r, P.FLAGS_CHANGED, 1)
    assert f[P.BAD_TYPE] == 0
    r = records.copy()
    r[7, 0] = (r[7, 0] & ~np.uint32(7)) | ((r[7, 0] + 1) & 3)  # another analytic type: a changed word 0, not a bad type
    f = _refused(state, slots, r, P.FLAGS_CHANGED, 1)
    assert f[P.BAD_TYPE] == 0
    for kind in (P.TYPE_TRI, P.TYPE_ENV, 7):
        r = records.copy()
        r[129, 0] = (r[129, 0] & ~np.uint32(7)) | kind
        f = _refused(state, slots, r, P.BAD_TYPE, 1)
        assert f[P.FLAGS_CHANGED] == 1


def test_a_triangle_light_is_refused():
    """the held record is a triangle light: refused even with that record itself"""
    a = L.Arrays(util.golden_scene("cornell_instances"))
    tri = a.tri_lights()
    assert len(tri)
    _refused(P.State(a), tri[:1], a.lights[tri[:1]], P.BAD_TYPE, 1)
