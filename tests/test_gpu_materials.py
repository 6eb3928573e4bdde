"""Materials that change on the device (rayhip_scene_set_materials and its _device form; ray_amd/csrc/materials.h, materials.hip.h): new
76-byte records for named material slots, the triangle lights a named emitter colours recoloured, the light tree refitted behind them.

What is asserted: the material array, the light array, the leaf table, the tree and its importance rows equal the host build of the
same element functions (tests/hostsim/hostsim_materials.cpp) bit for bit, from host and from device memory, aligned or not, below, at
and above a wavefront of entries; frames equal those of a fresh upload of the scene the reference built with the new materials (no
emitter named: the light arrays untouched) or of the scene with the host build's materials, lights and tree (emitters named); the
refitted tree samples without bias against the tree the reference builds for the recoloured scene; a refused call leaves arrays and
frames as they were; the call commutes with moved instances and with a vertex update; and after an instance update, which brings the
host's lights, naming the emitters again restores the recoloured arrays.  tests/test_materials_hostsim.py holds the host build against
the reference's scenes."""
import os

import numpy as np
import pytest
import torch  # noqa: F401  (FIRST: torch brings its own HIP runtime, and it must be the one that opens the device -- tests/test_gpu_comm.py)

import instance_pose_cases as IP
import light_refit_cases as L
import material_cases as M
import util
import vertex_update_cases as V
from ray_amd import api, hip
from ray_amd.api import eShadingNode

pytestmark = [pytest.mark.gpu]

W, H, SPP = 96, 64, 4  # (tests/test_gpu_light_refit.py)
bits = L.bits
ARRAYS = (11, 9, 10, 5, 6)
LIGHT_ARRAYS = (5, 6, 9, 10)
SCENES = ("cornell_materials", "material_field")


@pytest.fixture(scope="module")
def gpu_lib():
    lib = hip.Library()
    assert lib.device_count() > 0, "no HIP device: the product has no CPU path, -m gpu tests cannot run here"
    assert os.path.exists(M.MATERIALS_LIB) and L.have_lights_lib() and V.have_refit_lib(), "tests/hostsim is not built (run __graft_entry__.build())"
    if not os.path.exists(api.HIP_HOST_LIB):
        pytest.skip("libray_hip.so not built (needs the reference tree at build time)")
    return lib


def _context(lib, blob=None, refit=True, w=W, h=H):
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


def _arrays(ctx, kinds=ARRAYS):
    return {k: ctx.read_accel(k).copy() for k in kinds}


def _same(x, y):
    return all(np.array_equal(bits(x[k]), bits(y[k])) for k in x)


def _equals_state(got, state: M.State, leaf=None):
    """`leaf`: what array 10 must hold (default: the state's table; a context that ran no light refit yet holds no triangle summaries)"""
    return (np.array_equal(M.words(got[11]), M.words(state.materials)), np.array_equal(bits(got[9]), bits(state.lights)),
            np.array_equal(bits(got[10]).ravel(), bits(state.leaf if leaf is None else leaf).ravel()), np.array_equal(bits(got[5]), bits(state.cwnodes)),
            np.array_equal(bits(got[6]), bits(state.children)))


def _on_device(slots, records, offset_bytes=0):
    """(tensors kept alive, slots pointer, records pointer): the records `offset_bytes` behind a 256-byte-aligned allocation"""
    records = np.ascontiguousarray(records)
    raw = np.zeros(offset_bytes + records.nbytes, dtype=np.uint8)
    raw[offset_bytes:] = records.view(np.uint8).ravel()
    ts, tr = torch.from_numpy(np.ascontiguousarray(slots, dtype=np.uint32).view(np.int32).copy()).cuda(), torch.from_numpy(raw).cuda()
    torch.cuda.synchronize()
    assert tr.data_ptr() % 16 == 0
    return (ts, tr), ts.data_ptr(), tr.data_ptr() + offset_bytes


_cases = {}


def _case(name):
    """(blob, arrays, arrays of the scene moved in everything, arrays of the scene moved in everything but its emitters, state)"""
    if name not in _cases:
        blob = M.blob(name, 0)
        a = M.Arrays(blob)
        _cases[name] = (blob, a, M.Arrays(M.blob(name, 1)), M.Arrays(M.blob(name, 2)), M.State(a))
    return _cases[name]


def _three_forms(lib, blob, state, slots, records):
    """set_materials, set_materials_device with aligned records and with records 4 bytes off a 16-byte boundary: each on a context of its
    own against the host build"""
    rc, counters, want = M.host_set_materials(state, slots, records)
    assert rc == 0 and not counters[:M.EMITTERS_NAMED].any() and not want.same(state)
    for form in ("host", "device", "device+4"):
        ctx = _context(lib, blob)
        before = _arrays(ctx)
        assert all(_equals_state(before, state, before[10]))
        leaf = want.leaf if counters[M.EMITTERS_NAMED] else before[10]
        if form == "host":
            assert ctx.set_materials(slots, records) == 0
        else:
            keep, ps, pr = _on_device(slots, records, 4 if form == "device+4" else 0)
            assert pr % 16 == (4 if form == "device+4" else 0)
            assert ctx.set_materials_device(len(slots), ps, pr) == 0
            del keep
        ok = _equals_state(_arrays(ctx), want, leaf)
        assert all(ok), (form, len(slots), ok)
        # a second call with the same records: the same arrays (nothing accumulates)
        assert ctx.set_materials(slots, records) == 0 and all(_equals_state(_arrays(ctx), want, leaf))


# ---- 1: device against host build ------------------------------------------------------------------------------------------------
def test_cornell_materials_equal_the_host_build(gpu_lib):
    blob, a, moved, _, state = _case("cornell_materials")
    slots = np.nonzero(a.used_materials())[0].astype(np.uint32)  # every slot in use: the additive Mix too, whose record is the same in both phases
    assert len(slots) == 11 and len(M.changed_slots(a, moved)) == 10
    _three_forms(gpu_lib, blob, state, slots, moved.materials[slots])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_material_field_equals_the_host_build(gpu_lib, n):
    """material_field(130): 1, 63, 64, 65 and 130 named entries in shuffled slot order (the one entry: an emitter)"""
    blob, a, moved, _, state = _case("material_field")
    order = np.random.RandomState(5).permutation(130) + 3
    pick = order[:n] if n > 1 else np.array([3 + 35])
    assert state.flags[pick[0]] & M.SLOT_EMITTER or n > 1
    _three_forms(gpu_lib, blob, state, pick.astype(np.uint32), moved.materials[pick])


# ---- 2: no emitter named ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_without_an_emitter_the_lights_stay_and_frames_equal_a_fresh_upload(gpu_lib, name):
    blob, a, _, quiet, state = _case(name)
    slots = M.changed_slots(a, quiet)
    assert len(slots) > 0 and not (state.flags[slots] & M.SLOT_EMITTER).any()
    li = np.sort(a.li_indices)
    assert np.array_equal(a.lights[li], quiet.lights[li]) and a.cwnodes.tobytes() == quiet.cwnodes.tobytes()  # the scenes differ in materials only
    ctx = _context(gpu_lib, blob)
    first, before = _frames(ctx), _arrays(ctx, LIGHT_ARRAYS)
    assert ctx.set_materials(slots, quiet.materials[slots]) == 0
    assert _same(_arrays(ctx, LIGHT_ARRAYS), before)
    used = a.used_materials() != 0
    assert np.array_equal(M.words(ctx.read_accel(11)[used]), M.words(quiet.materials[used]))
    updated = _frames(ctx)
    fresh = _context(gpu_lib, M.blob(name, 2), refit=False)
    assert np.array_equal(updated, _frames(fresh)) and not np.array_equal(updated, first) and np.isfinite(updated).all()


# ---- 3: emitters named -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_with_emitters_frames_equal_a_fresh_upload_of_the_host_builds_scene(gpu_lib, name):
    blob, a, moved, _, state = _case(name)
    slots = M.changed_slots(a, moved)
    rc, counters, want = M.host_set_materials(state, slots, moved.materials[slots])
    assert rc == 0 and counters[M.EMITTERS_NAMED] > 0
    ctx = _context(gpu_lib, blob)
    first = _frames(ctx)
    assert ctx.set_materials(slots, moved.materials[slots]) == 0
    assert all(_equals_state(_arrays(ctx), want))
    updated = _frames(ctx)
    twin = L.with_section(L.with_section(L.with_section(blob, "materials", want.materials), "lights", want.lights), "light_cwnodes", want.cwnodes)
    fresh = _context(gpu_lib, twin, refit=False)
    assert np.array_equal(bits(fresh.read_accel(6)), bits(want.children))
    assert np.array_equal(updated, _frames(fresh)) and not np.array_equal(updated, first) and np.isfinite(updated).all()


# ---- 4: the sampler --------------------------------------------------------------------------------------------------------------
def test_the_refitted_tree_is_a_fair_sampler(gpu_lib):
    """cornell_materials with every material changed, its two emitters recoloured: 64 x 64, 256 samples per pixel: the frame mean of RAW
    under the refitted tree against the mean under the tree the reference built for the recoloured scene.  The noise floor is the
    difference of two renders with the reference-built tree over disjoint iterations (1..256 and 257..512; RAW is a running mean, so the
    second is 2 * mean(1..512) - mean(1..256)).  A biased estimator fails at any factor; the 3 only keeps noise from failing it.
    (The method of tests/test_gpu_light_pose.py::test_the_refitted_tree_is_a_fair_sampler.)"""
    blob, a, moved, _, state = _case("cornell_materials")
    slots = M.changed_slots(a, moved)
    ctx = _context(gpu_lib, blob, w=64, h=64)
    assert ctx.set_materials(slots, moved.materials[slots]) == 0
    refitted = float(_frames(ctx, 256)[..., :3].astype(np.float64).mean())
    rebuilt_ctx = _context(gpu_lib, M.blob("cornell_materials", 1), refit=False, w=64, h=64)
    rebuilt_ctx.clear()
    m256 = float(util.render_frames(rebuilt_ctx, 256)[..., :3].astype(np.float64).mean())
    for it in range(257, 513):
        rebuilt_ctx.render(it)
    m512 = float(rebuilt_ctx.readback(hip.BUF_RAW)[..., :3].astype(np.float64).mean())
    second = 2.0 * m512 - m256
    floor, gap = abs(m256 - second), abs(refitted - m256)
    print(f"frame mean: refitted tree {refitted:.6f}, rebuilt tree {m256:.6f} (iterations 1..256) and {second:.6f} (257..512); "
          f"refit against rebuilt {gap:.3e}, noise floor {floor:.3e}")
    li = np.sort(a.li_indices)
    assert np.array_equal(bits(ctx.read_accel(9)[li]), bits(rebuilt_ctx.read_accel(9)[li]))
    assert m256 > 0 and gap <= 3.0 * floor


# ---- 5: a refused call -----------------------------------------------------------------------------------------------------------
def test_a_refused_call_touches_nothing(gpu_lib):
    blob, a, moved, _, state = _case("cornell_materials")
    slots = M.changed_slots(a, moved)
    records = moved.materials[slots].copy()
    lamp = int(np.nonzero(slots == 3)[0][0])
    ctx = _context(gpu_lib, blob)
    assert ctx.set_materials(slots[:2], records[:2]) == 0
    before, frames = _arrays(ctx), _frames(ctx)

    def refused(c, s, r, match, kinds=ARRAYS, held=None):
        held = before if held is None else held
        with pytest.raises(RuntimeError, match=match):
            c.set_materials(s, r)
        assert _same(_arrays(c, kinds), held), match
        keep, ps, pr = _on_device(s, r, 4)
        with pytest.raises(RuntimeError, match=match):
            c.set_materials_device(len(s), ps, pr)
        assert _same(_arrays(c, kinds), held), (match, "device")

    s = slots.copy()
    s[2] = len(a.materials)
    refused(ctx, s, records, "outside")
    dead = np.nonzero(a.used_materials() == 0)[0][:1].astype(np.uint32)
    refused(ctx, dead, a.materials[dead], "outside")
    s = slots.copy()
    s[4] = s[1]
    refused(ctx, s, records, "more than once")
    for field in ("type", "flags", "textures"):
        r = records.copy()
        r[field][5] ^= 1
        refused(ctx, slots, r, "differ from those the slot holds")
    for value in (np.nan, np.inf):
        r = records.copy()
        r["ior"][1] = value
        refused(ctx, slots, r, "not finite")
    r = records.copy()
    r["tangent_rotation_or_strength"][lamp] = -1.0
    refused(ctx, slots, r, "negative")
    with pytest.raises(RuntimeError, match="null pointer"):
        ctx.set_materials_device(3, 0, 0)
    assert ctx.set_materials(slots[:0], records[:0]) == 0 and ctx.set_materials_device(0, 0, 0) == 0  # n == 0
    assert _same(_arrays(ctx), before) and np.array_equal(_frames(ctx), frames)
    # 2: no scene; an emitter recoloured with the switch off (bytewise unchanged, it passes); a refracting record on a plain_ior scene
    none = hip.Context(0, gpu_lib)
    assert none.set_materials(slots, records) == 2
    off = _context(gpu_lib, blob, refit=False)
    held, off_frames = _arrays(off, (11, 9, 5, 6)), _frames(off)
    keep, ps, pr = _on_device(slots, records)
    assert off.set_materials(slots, records) == 2 and off.set_materials_device(len(slots), ps, pr) == 2
    assert _same(_arrays(off, (11, 9, 5, 6)), held) and np.array_equal(_frames(off), off_frames)
    r = records[lamp:lamp + 1].copy()
    r["base_color"], r["tangent_rotation_or_strength"], r["roughness_unorm"] = a.materials["base_color"][3], a.materials["tangent_rotation_or_strength"][3], 999
    assert off.set_materials(slots[lamp:lamp + 1], r) == 0
    got = _arrays(off, (11, 9, 5, 6))
    assert np.array_equal(M.words(got[11][3:4]), M.words(r)) and _same({k: got[k] for k in (9, 5, 6)}, {k: held[k] for k in (9, 5, 6)})
    fblob, fa, fmoved, _, fstate = _case("material_field")
    fslots = M.changed_slots(fa, fmoved)
    frecords = fmoved.materials[fslots].copy()
    frecords["transmission_unorm"][np.nonzero(frecords["type"] == eShadingNode.Principled)[0][0]] = 1
    field = _context(gpu_lib, fblob)
    held, field_frames = _arrays(field, (11, 9, 5, 6)), _frames(field)
    keep, ps, pr = _on_device(fslots, frecords, 4)
    assert field.set_materials(fslots, frecords) == 2 and field.set_materials_device(len(fslots), ps, pr) == 2
    assert _same(_arrays(field, (11, 9, 5, 6)), held) and np.array_equal(_frames(field), field_frames)
    # a duplicate across a wavefront boundary: entries 0 and 64
    s = fslots[:65].copy()
    s[64] = s[0]
    refused(field, s, fmoved.materials[fslots[:65]], "more than once", (11, 9, 5, 6), held)


# ---- 6: commuting ----------------------------------------------------------------------------------------------------------------
def test_it_commutes_with_moved_instances_and_with_a_vertex_update(gpu_lib):
    blob, a, moved, _, state = _case("cornell_materials")
    slots = M.changed_slots(a, moved)
    records = moved.materials[slots]
    lit = IP.light_slots(a)
    assert len(lit) > 0
    xforms = IP.gentle_xforms(a, lit, seed=3)
    kinds = (5, 6, 7, 8, 9, 10, 11)
    one, other = _context(gpu_lib, blob), _context(gpu_lib, blob)
    rest = one.read_accel(7).copy()
    assert one.set_materials(slots, records) == 0 and one.set_instance_transforms(lit, xforms) == 0
    assert other.set_instance_transforms(lit, xforms) == 0 and other.set_materials(slots, records) == 0
    got = _arrays(one, kinds)
    assert _same(got, _arrays(other, kinds)) and np.array_equal(one.read_accel(3), other.read_accel(3))
    assert not np.array_equal(bits(got[7]), bits(rest)) and np.array_equal(M.words(got[11][slots]), M.words(records))
    assert np.array_equal(_frames(one), _frames(other))
    # ... and a vertex update that moves the lamp (and everything else)
    v = L.moved_vertices(a)
    kinds = (4, 5, 6, 7, 9, 10, 11)
    one, other = _context(gpu_lib, blob), _context(gpu_lib, blob)
    assert one.set_materials(slots, records) == 0 and one.update_vertices(0, v) == 0
    assert other.update_vertices(0, v) == 0 and other.set_materials(slots, records) == 0
    got = _arrays(one, kinds)
    assert _same(got, _arrays(other, kinds)) and np.array_equal(one.read_accel(3), other.read_accel(3))
    assert not np.array_equal(bits(got[7]), bits(rest))
    rc, _, want = M.host_set_materials(state, slots, records)
    assert rc == 0 and np.array_equal(bits(got[9]), bits(want.lights)) and not np.array_equal(bits(got[5]), bits(want.cwnodes))
    assert np.array_equal(_frames(one), _frames(other))


# ---- 7: after an instance update -------------------------------------------------------------------------------------------------
def test_naming_the_emitters_again_after_an_instance_update_restores_the_lights(gpu_lib):
    blob, a, moved, _, state = _case("cornell_materials")
    slots = M.changed_slots(a, moved)
    records = moved.materials[slots]
    rc, _, want = M.host_set_materials(state, slots, records)
    assert rc == 0
    ctx = _context(gpu_lib, blob)
    assert ctx.set_materials(slots, records) == 0 and all(_equals_state(_arrays(ctx), want))
    assert ctx.update_instances(blob) == 0  # the unchanged host scene: the device's materials stay, the host's lights come
    got = _arrays(ctx, (11, 9, 5))
    assert np.array_equal(M.words(got[11]), M.words(want.materials))
    assert np.array_equal(bits(got[9]), bits(a.lights)) and np.array_equal(bits(got[5]), bits(a.cwnodes))
    assert ctx.set_materials(slots, records) == 0  # bytewise the records in place: the lights of every named emitter are recoloured all the same
    assert all(_equals_state(_arrays(ctx), want))
