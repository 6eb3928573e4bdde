"""Changing materials as the device does it, without a GPU: the host build of ray_amd/csrc/materials.h
(tests/hostsim/hostsim_materials.cpp) against the scenes the reference built.

What is asserted: numpy packers that restate AddMaterial make the reference's records bytewise; the emitter table names, for every
triangle light, a material whose base_color * strength is the light's colour bit for bit -- the emitter found through a Mix node
included -- and no light for an Emissive material that is not importance-sampled; after a call with the records of a moved scene the
material array, the light array and the leaf fluxes of the light tree are the reference's; and every refusal returns its code and
leaves the state bytewise as it was.  tests/test_gpu_materials.py holds the device against this host build."""
import os

import numpy as np
import pytest

import light_refit_cases as L
import material_cases as M
from ray_amd import api
from ray_amd.api import eShadingNode

bits = L.bits
SCENES = ("cornell_materials", "material_field")


@pytest.fixture(scope="module", autouse=True)
def _built():
    assert os.path.exists(M.MATERIALS_LIB) and L.have_lights_lib(), "tests/hostsim is not built (run __graft_entry__.build())"
    if not os.path.exists(api.HIP_HOST_LIB):
        pytest.skip("libray_hip.so not built (needs the reference tree at build time)")


_cases = {}


def _case(name):
    """(arrays at rest, arrays of the moved scene, state at rest)"""
    if name not in _cases:
        a = M.Arrays(M.blob(name, 0))
        _cases[name] = (a, M.Arrays(M.blob(name, 1)), M.State(a))
    return _cases[name]


# ---- the packers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_the_packers_make_the_references_records(name):
    a, moved, _ = _case(name)
    for phase, want in ((0, a), (1, moved)):
        slots, records = M.packed(M.descs(name, phase), a)
        assert np.array_equal(np.nonzero(a.used_materials())[0], slots)  # every slot in use, and no other
        assert np.array_equal(M.words(records), M.words(want.materials[slots])), phase
    # the phases differ only in what a call may change
    for k in ("textures", "flags", "type"):
        assert np.array_equal(a.materials[k][slots], moved.materials[k][slots]), k
    assert len(M.changed_slots(a, moved)) >= len(slots) - 3


# ---- the emitter table -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_the_emitter_table_names_the_material_the_scene_build_baked(name):
    for a in _case(name)[:2]:
        emitter, flags = M.emitter_tables(a)
        tri = a.tri_lights()
        assert len(tri) > 0 and (emitter[tri] != M.NO_EMITTER).all()
        others = np.setdiff1d(np.arange(len(a.lights)), tri)
        assert (emitter[others] == M.NO_EMITTER).all()
        m = a.materials[emitter[tri]]
        assert (m["type"] == eShadingNode.Emissive).all() and (m["flags"] & M.IMP_SAMPLE).all()
        col = m["base_color"] * m["tangent_rotation_or_strength"][:, None]  # float32: one rounding per product
        assert col.dtype == np.float32 and np.array_equal(bits(col), a.lights[tri, 1:4])
        assert np.array_equal(np.nonzero(flags & M.SLOT_EMITTER)[0], np.unique(emitter[tri]))
        assert np.array_equal((flags & M.SLOT_LIVE) != 0, a.used_materials() != 0)
    a = _case(name)[0]
    emitter, flags = M.emitter_tables(a)
    if name == "cornell_materials":
        # the lamp's two triangles name the lamp; the four of the emitting Principled name its Emissive record, which only the additive
        # Mix over it (the triangles' own material) leads to; the Emissive that is not importance-sampled colours no light
        lamp, glow, principled, emission, mix = 3, 6, 8, 9, 10
        assert a.materials["type"][mix] == eShadingNode.Mix and list(a.materials["textures"][mix, 3:5]) == [principled, emission]
        named = emitter[a.tri_lights()]
        assert sorted(named.tolist()) == [lamp] * 2 + [emission] * 4
        fronts = a.tri_materials[a.lights[a.tri_lights(), 4], 0] & M.MAT_INDEX_BITS
        assert sorted(fronts.tolist()) == [lamp] * 2 + [mix] * 4
        assert a.materials["type"][glow] == eShadingNode.Emissive and not flags[glow] & M.SLOT_EMITTER and glow not in named
    else:
        assert sorted(set(emitter[a.tri_lights()].tolist())) == [3 + k for k in range(0, 130, 5)]


# ---- the host build -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_the_host_build_leaves_the_references_materials_and_lights(name):
    a, moved, state = _case(name)
    slots = M.changed_slots(a, moved)
    rc, counters, after = M.host_set_materials(state, slots, moved.materials[slots])
    assert rc == 0 and not counters[:M.EMITTERS_NAMED].any() and counters[M.EMITTERS_NAMED] == np.count_nonzero(state.flags[slots] & M.SLOT_EMITTER) > 0
    used = a.used_materials() != 0
    assert np.array_equal(M.words(after.materials[used]), M.words(moved.materials[used]))
    assert np.array_equal(M.words(after.materials[~used]), M.words(a.materials[~used]))
    li = np.sort(a.li_indices)
    assert np.array_equal(after.lights[li], moved.lights[li]) and not np.array_equal(after.lights[li], a.lights[li])
    # the leaf fluxes of the recoloured triangle lights: the words of the tree the reference built for the moved scene
    ours, theirs = L.paths(after.cwnodes), L.paths(moved.cwnodes)
    for i in a.tri_lights():
        (w, k), (rw, rk) = ours[int(i)][-1], theirs[int(i)][-1]
        got = bits(after.cwnodes["flux"][w, k:k + 1])[0]
        assert got == bits(moved.cwnodes["flux"][rw, rk:rk + 1])[0] == bits(after.leaf["flux"][i:i + 1])[0], int(i)
        assert got != bits(a.cwnodes["flux"][w, k:k + 1])[0]
    # no light moved: the root box stays
    assert np.array_equal(bits(after.cwnodes["bbox_min"][0]), bits(a.cwnodes["bbox_min"][0]))
    assert np.array_equal(bits(after.cwnodes["bbox_max"][0]), bits(a.cwnodes["bbox_max"][0]))
    assert np.array_equal(bits(after.tri_geom), bits(state.tri_geom))
    # a call that names no emitter leaves every light array alone
    quiet = slots[(state.flags[slots] & M.SLOT_EMITTER) == 0]
    rc, counters, only = M.host_set_materials(state, quiet, moved.materials[quiet])
    assert rc == 0 and not counters.any() and len(quiet) > 0
    assert all(np.array_equal(bits(getattr(only, k)), bits(getattr(state, k))) for k in ("lights", "cwnodes", "children", "leaf"))
    assert np.array_equal(M.words(only.materials[quiet]), M.words(moved.materials[quiet]))


# ---- every refusal ----------------------------------------------------------------------------------------------------------------------
def _refused(state, slots, records, code, counter, **kw):
    rc, counters, after = M.host_set_materials(state, slots, records, **kw)
    assert rc == code and (counter is None or counters[counter] > 0), (rc, counters)
    assert after.same(state) and np.array_equal(bits(after.tri_geom), bits(state.tri_geom))


def test_every_refusal_leaves_the_state_as_it_was():
    a, moved, state = _case("cornell_materials")
    slots = M.changed_slots(a, moved)
    records = moved.materials[slots].copy()
    lamp = int(np.nonzero(slots == 3)[0][0])
    assert state.flags[3] & M.SLOT_EMITTER
    for bad in (len(a.materials), 0xffffffff):
        s = slots.copy()
        s[2] = bad
        _refused(state, s, records, 1, M.BAD_SLOT)  # outside the array
    dead = int(np.nonzero(a.used_materials() == 0)[0][0])
    _refused(state, [dead], a.materials[[dead]], 1, M.BAD_SLOT)  # a slot no triangle uses, with the very record it holds
    s = slots.copy()
    s[4] = s[1]
    _refused(state, s, records, 1, M.DUPLICATE)
    for field, index in (("type", None), ("flags", None), ("textures", 0), ("textures", 3), ("textures", 4)):
        r = records.copy()
        if index is None:
            r[field][5] ^= 1 if field == "flags" else 7
        else:
            r[field][5, index] ^= 1
        _refused(state, slots, r, 1, M.GRAPH_CHANGED)
    for value in (np.nan, np.inf, -np.inf):
        for field, index in (("base_color", 0), ("base_color", 1), ("base_color", 2), ("tangent_rotation_or_strength", None), ("ior", None)):
            r = records.copy()
            if index is None:
                r[field][1] = value
            else:
                r[field][1, index] = value
            _refused(state, slots, r, 1, M.NOT_FINITE)
    for field, index in (("tangent_rotation_or_strength", None), ("base_color", 1)):
        r = records.copy()
        if index is None:
            r[field][lamp] = -1.0
        else:
            r[field][lamp, index] = -0.5
        _refused(state, slots, r, 1, M.NEGATIVE)
    r = records.copy()
    r["base_color"][0] = (-0.5, 0.5, 0.5)  # a Diffuse record may: only a flux must not be negative
    assert M.host_set_materials(state, slots, r)[0] == 0
    rc, _, after = M.host_set_materials(state, slots[:0], records[:0])
    assert rc == 0 and after.same(state)  # n == 0
    assert M.materials_lib().hostsim_set_materials(None, 0, None, None, 0, 1, 3, None, None, np.zeros(8, dtype=np.uint32).ctypes.data) == 1  # null pointers
    # an emitter recoloured while the lights cannot follow: 2; the same emitter with colour and strength bytewise as held: 0
    _refused(state, slots, records, 2, M.PINNED, refittable=False)
    _refused(state, slots[lamp:lamp + 1], records[lamp:lamp + 1], 2, M.PINNED, refittable=False)
    r = records.copy()
    r["base_color"][lamp], r["tangent_rotation_or_strength"][lamp] = a.materials["base_color"][3], a.materials["tangent_rotation_or_strength"][3]
    r["roughness_unorm"][lamp] = 1234
    keep = [i for i in range(len(slots)) if not state.flags[slots[i]] & M.SLOT_EMITTER or i == lamp]
    rc, counters, after = M.host_set_materials(state, slots[keep], r[keep], refittable=False)
    assert rc == 0 and counters[M.EMITTERS_NAMED] == 1 and not counters[:M.EMITTERS_NAMED].any()
    assert np.array_equal(M.words(after.materials[slots[keep]]), M.words(r[keep])) and np.array_equal(after.lights, state.lights)
    assert np.array_equal(bits(after.cwnodes), bits(state.cwnodes))
    # a record that refracts on a scene whose passes leave the rays' ior plane alone: 2 -- and the other way round passes
    fa, fmoved, fstate = _case("material_field")
    assert fstate.plain_ior and not state.plain_ior
    fslots = M.changed_slots(fa, fmoved)
    frecords = fmoved.materials[fslots].copy()
    principled = int(np.nonzero(frecords["type"] == eShadingNode.Principled)[0][0])
    r = frecords.copy()
    r["transmission_unorm"][principled] = 1
    _refused(fstate, fslots, r, 2, M.REFRACTS)
    assert M.host_set_materials(fstate, fslots, r, plain_ior=False)[0] == 0
    opaque = records.copy()
    opaque["transmission_unorm"][records["type"] == eShadingNode.Principled] = 0
    assert M.host_set_materials(state, slots, opaque)[0] == 0
    # a duplicate across a wavefront boundary: entries 0 and 64
    s = fslots[:65].copy()
    s[64] = s[0]
    _refused(fstate, s, frecords[:65], 1, M.DUPLICATE)
    # findings of both kinds: 1 wins over 2
    r = frecords.copy()
    r["transmission_unorm"][principled], r["ior"][0] = 1, np.nan
    _refused(fstate, fslots, r, 1, M.REFRACTS)
