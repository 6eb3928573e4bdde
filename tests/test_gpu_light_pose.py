"""Analytic lights that move or change colour on the device (rayhip_scene_set_lights and its _device form; ray_amd/csrc/light_pose.h,
light_pose.hip.h): new 64-byte records for named light slots, their leaf summaries, and the light tree refitted behind them.

What is asserted: the light array, the leaf table, the tree and its importance rows equal the host build of the same element functions
(tests/hostsim/hostsim_light_pose.cpp) bit for bit, from host and from device memory, aligned or not, below, at and above a wavefront
of entries; frames equal those of a context that uploaded the scene with the new records and the refitted tree; the refitted tree
samples without bias against the tree the reference builds for the moved scene; a refused call leaves arrays and frames as they were;
the call commutes with a vertex update and with moved instances; and it needs the switch.  tests/test_light_pose_hostsim.py holds the
host build against the reference's trees and records."""
import os

import numpy as np
import pytest
import torch  # noqa: F401  (FIRST: torch brings its own HIP runtime, and it must be the one that opens the device -- tests/test_gpu_comm.py)

import instance_pose_cases as IP
import light_pose_cases as P
import light_refit_cases as L
import util
import vertex_update_cases as V
from ray_amd import api, hip

pytestmark = [pytest.mark.gpu]

W, H, SPP = 96, 64, 4  # (tests/test_gpu_light_refit.py)
bits = L.bits
LIGHT_ARRAYS = (5, 6, 9, 10)


@pytest.fixture(scope="module")
def gpu_lib():
    lib = hip.Library()
    assert lib.device_count() > 0, "no HIP device: the product has no CPU path, -m gpu tests cannot run here"
    assert os.path.exists(P.POSE_LIB) and L.have_lights_lib() and V.have_refit_lib(), "tests/hostsim is not built (run __graft_entry__.build())"
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


def _arrays(ctx, kinds=LIGHT_ARRAYS):
    return {k: ctx.read_accel(k).copy() for k in kinds}


def _same(x, y):
    return all(np.array_equal(bits(x[k]), bits(y[k])) for k in x)


def _equals_state(got, state: P.State):
    return (np.array_equal(bits(got[9]), bits(state.lights)), np.array_equal(bits(got[10]).ravel(), bits(state.leaf).ravel()),
            np.array_equal(bits(got[5]), bits(state.cwnodes)), np.array_equal(bits(got[6]), bits(state.children)))


def _on_device(slots, records, offset_bytes=0):
    """(tensors kept alive, slots pointer, records pointer): the records `offset_bytes` behind a 256-byte-aligned allocation"""
    raw = np.zeros(offset_bytes + records.nbytes, dtype=np.uint8)
    raw[offset_bytes:] = np.ascontiguousarray(records).view(np.uint8).ravel()
    ts, tr = torch.from_numpy(np.ascontiguousarray(slots, dtype=np.uint32).view(np.int32).copy()).cuda(), torch.from_numpy(raw).cuda()
    torch.cuda.synchronize()
    assert tr.data_ptr() % 16 == 0
    return (ts, tr), ts.data_ptr(), tr.data_ptr() + offset_bytes


_cornell = {}


def _cornell_case():
    """(blob, arrays, state, slots, records of all six lights moved, the state the host build leaves)"""
    if not _cornell:
        blob = P.cornell_blob()
        a, moved = L.Arrays(blob), L.Arrays(P.cornell_blob(P.KINDS))
        slot_of = P.cornell_slots(a)
        slots = np.array([slot_of[k] for k in P.KINDS], dtype=np.uint32)
        records = moved.lights[slots].copy()  # (the reference's records: the numpy packers make the same, test_light_pose_hostsim.py)
        state = P.State(a)
        rc, findings, after = P.host_set_lights(state, slots, records)
        assert rc == 0 and not findings.any()
        _cornell["case"] = (blob, a, state, slots, records, after)
    return _cornell["case"]


def _three_forms(lib, blob, state, slots, records):
    """set_lights, set_lights_device with aligned records and with records 4 bytes off: each on a context of its own against the host build"""
    rc, findings, want = P.host_set_lights(state, slots, records)
    assert rc == 0 and not findings.any() and not want.same(state)
    for form in ("host", "device", "device+4"):
        ctx = _context(lib, blob)
        before = _arrays(ctx, (5, 6, 9))
        assert np.array_equal(bits(before[9]), bits(state.lights)) and np.array_equal(bits(before[5]), bits(state.cwnodes))
        if form == "host":
            assert ctx.set_lights(slots, records) == 0
        else:
            keep, ps, pr = _on_device(slots, records, 4 if form == "device+4" else 0)
            assert ctx.set_lights_device(len(slots), ps, pr) == 0
            del keep
        got = _arrays(ctx)
        ok = _equals_state(got, want)
        rows = np.nonzero((bits(got[10]).reshape(len(want.leaf), -1) != bits(want.leaf).reshape(len(want.leaf), -1)).any(axis=1))[0]
        assert all(ok), (form, len(slots), ok, [(int(r), int(want.lights[r, 0] & 7), got[10][r].tolist(), want.leaf[r].tolist()) for r in rows[:4]])
        # a second call with the same records: the same arrays (nothing accumulates)
        assert ctx.set_lights(slots, records) == 0 and all(_equals_state(_arrays(ctx), want))


# ---- 1: device against host build ------------------------------------------------------------------------------------------------
def test_cornell_lights_equal_the_host_build(gpu_lib):
    blob, a, state, slots, records, _ = _cornell_case()
    _three_forms(gpu_lib, blob, state, slots, records)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_light_field_equals_the_host_build(gpu_lib, n):
    """light_field(130): a tree of 37 nodes in four heights; 1, 63, 64, 65 and 130 named entries (the last ones in descending slot order)"""
    blob = P.field_blob(130)
    a = L.Arrays(blob)
    slots, records = P.field_records(a, 130)
    pick = np.arange(130)[::-1][:n] if n > 1 else np.array([77])
    _three_forms(gpu_lib, blob, P.State(a), slots[pick], records[pick])


# ---- 2: frames -------------------------------------------------------------------------------------------------------------------
def test_frames_equal_a_fresh_upload_with_the_refitted_tree(gpu_lib):
    blob, a, state, slots, records, after = _cornell_case()
    ctx = _context(gpu_lib, blob)
    first = _frames(ctx)
    assert ctx.set_lights(slots, records) == 0
    updated = _frames(ctx)
    got = _arrays(ctx)
    assert all(_equals_state(got, after))
    fresh = _context(gpu_lib, V.patched_blob(blob, lights=got[9], light_cwnodes=got[5]), refit=False)
    assert np.array_equal(bits(fresh.read_accel(6)), bits(got[6])) and np.array_equal(bits(fresh.read_accel(7)), bits(ctx.read_accel(7)))
    assert np.array_equal(updated, _frames(fresh)) and not np.array_equal(updated, first)
    assert np.isfinite(updated).all()


# ---- 3: the sampler --------------------------------------------------------------------------------------------------------------
def test_the_refitted_tree_is_a_fair_sampler(gpu_lib):
    """cornell_lights with all six lights moved, 64 x 64, 256 samples per pixel: the frame mean of RAW under the refitted tree against
    the mean under the tree the reference built for the moved scene.  The noise floor is the difference of two renders with the
    reference-built tree over disjoint iterations (1..256 and 257..512; RAW is a running mean, so the second is
    2 * mean(1..512) - mean(1..256)).  A biased estimator fails at any factor; the 3 only keeps noise from failing it.
    (The method of tests/test_gpu_light_refit.py::test_the_refitted_tree_is_a_fair_sampler.)"""
    blob, a, state, slots, records, _ = _cornell_case()
    ctx = _context(gpu_lib, blob, w=64, h=64)
    assert ctx.set_lights(slots, records) == 0
    refitted = float(_frames(ctx, 256)[..., :3].astype(np.float64).mean())
    rebuilt_ctx = _context(gpu_lib, P.cornell_blob(P.KINDS), refit=False, w=64, h=64)
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
    assert np.array_equal(bits(ctx.read_accel(9)[np.sort(a.li_indices)]), bits(rebuilt_ctx.read_accel(9)[np.sort(a.li_indices)]))
    assert m256 > 0 and gap <= 3.0 * floor


# ---- 4: a refused call -----------------------------------------------------------------------------------------------------------
def test_a_refused_call_touches_nothing(gpu_lib):
    blob = P.field_blob(130)
    a = L.Arrays(blob)
    slots, records = P.field_records(a, 130)
    ctx = _context(gpu_lib, blob)
    assert ctx.set_lights(slots[:8], records[:8]) == 0  # (so that the leaf table holds every summary and some lights are posed)
    before, frames = _arrays(ctx), _frames(ctx)
    nan = np.array([np.nan], dtype=np.float32).view(np.uint32)[0]
    for n, at in ((1, 0), (64, 63), (65, 64)):  # the bad entry alone, as lane 63 of 64, as entry 64 of 65
        for what, match in (("slot", "outside"), ("duplicate", "more than once"), ("type", "triangle or environment"), ("flags", "word 0"),
                            ("float", "not finite")):
            s, r = slots[20:20 + n].copy(), records[20:20 + n].copy()
            if what == "slot":
                s[at] = len(a.lights)
            elif what == "duplicate":
                if n == 1:
                    continue
                s[at], r[at] = s[0], r[0]
            elif what == "type":
                r[at, 0] = (r[at, 0] & ~np.uint32(7)) | P.TYPE_TRI
            elif what == "flags":
                r[at, 0] ^= 1 << 4  # cast_shadow
            else:
                r[at, 9] = nan
            with pytest.raises(RuntimeError, match=match):
                ctx.set_lights(s, r)
            assert _same(_arrays(ctx), before), (n, what)
            keep, ps, pr = _on_device(s, r, 4)
            with pytest.raises(RuntimeError, match=match):
                ctx.set_lights_device(n, ps, pr)
            assert _same(_arrays(ctx), before), (n, what, "device")
    with pytest.raises(RuntimeError, match="null pointer"):
        ctx.set_lights_device(3, 0, 0)
    assert ctx.set_lights(slots[:0], records[:0]) == 0 and ctx.set_lights_device(0, 0, 0) == 0  # n == 0
    assert _same(_arrays(ctx), before) and np.array_equal(_frames(ctx), frames)
    # a triangle light's slot: refused with the very record it holds
    fix = util.golden_scene("cornell_instances")
    fa = L.Arrays(fix)
    tri_ctx = _context(gpu_lib, fix)
    held = _arrays(tri_ctx, (5, 6, 9))
    with pytest.raises(RuntimeError, match="triangle or environment"):
        tri_ctx.set_lights(fa.tri_lights()[:1], fa.lights[fa.tri_lights()[:1]])
    assert _same(_arrays(tri_ctx, (5, 6, 9)), held)


# ---- 5: commuting ----------------------------------------------------------------------------------------------------------------
def _sheet_case():
    """emissive_sheet of tests/light_refit_cases.py (578 triangle lights, and -- in its builder -- a sphere, a rect and a directional
    light): (blob, arrays, moved vertices, slots and moved records of the sphere and the rect light)"""
    blob = L.scene_blob("emissive_sheet", 0)
    a = L.Arrays(blob)
    v = L.Arrays(L.scene_blob("emissive_sheet", 1)).vertices
    slots = P.analytic_slots(a)
    sphere = next(s for s in slots if a.lights[s, 0] & 7 == P.TYPE_SPHERE)
    rect = next(s for s in slots if a.lights[s, 0] & 7 == P.TYPE_RECT)
    records = np.array([P.pack("sphere", a.lights[sphere, 0], color=(2.0, 3.5, 3.0), position=(-0.20, 0.36, -0.18), radius=0.03),
                        P.pack("rect", a.lights[rect, 0], color=(5.0, 3.0, 4.5), width=0.10, height=0.12,
                               xform=P.scenes._translate(-0.26, 0.50, -0.40, rot_x_deg=15.0, rot_z_deg=10.0))], dtype=np.uint32)
    return blob, a, v, np.array([sphere, rect], dtype=np.uint32), records


def test_it_commutes_with_a_vertex_update(gpu_lib):
    blob, a, v, slots, records = _sheet_case()
    kinds = (4, 5, 6, 7, 9, 10)
    one, other = _context(gpu_lib, blob), _context(gpu_lib, blob)
    rest = _arrays(one, (5, 9))
    assert one.set_lights(slots, records) == 0 and one.update_vertices(0, v) == 0
    assert other.update_vertices(0, v) == 0 and other.set_lights(slots, records) == 0
    got = _arrays(one, kinds)
    assert _same(got, _arrays(other, kinds))
    assert not np.array_equal(bits(got[5]), bits(rest[5])) and np.array_equal(bits(got[9][slots]), bits(records))
    assert np.array_equal(_frames(one), _frames(other))
    # ... and the host build says the same: the vertex update's refit under the posed table
    state = P.State(a)
    rc, _, posed = P.host_set_lights(state, slots, records)
    assert rc == 0
    want = L.host_refit(a, v)
    posed.leaf[a.tri_lights()] = want.leaf[a.tri_lights()]
    want_tree = P.host_refit_posed(posed)
    assert np.array_equal(bits(got[5]), bits(want_tree.cwnodes)) and np.array_equal(bits(got[10]).ravel(), bits(want_tree.leaf).ravel())


def test_it_commutes_with_moved_instances(gpu_lib):
    blob, a, v, slots, records = _sheet_case()
    kinds = (5, 6, 7, 8, 9, 10)
    lit = IP.light_slots(a)
    xforms = IP.gentle_xforms(a, lit, seed=3)
    one, other = _context(gpu_lib, blob), _context(gpu_lib, blob)
    rest = one.read_accel(7).copy()
    assert one.set_lights(slots, records) == 0 and one.set_instance_transforms(lit, xforms) == 0
    assert other.set_instance_transforms(lit, xforms) == 0 and other.set_lights(slots, records) == 0
    got = _arrays(one, kinds)
    assert _same(got, _arrays(other, kinds)) and np.array_equal(one.read_accel(3), other.read_accel(3))
    assert not np.array_equal(bits(got[7]), bits(rest)) and np.array_equal(bits(got[9][slots]), bits(records))
    assert np.array_equal(_frames(one), _frames(other))
    # an instance update brings the host's lights and tree: nothing is posed any more
    plain = _context(gpu_lib, blob)
    assert one.update_instances(blob) == 0 and plain.update_instances(blob) == 0
    assert np.array_equal(bits(one.read_accel(9)), bits(a.lights)) and np.array_equal(bits(one.read_accel(5)), bits(a.cwnodes))
    assert one.update_vertices(0, v) == 0 and plain.update_vertices(0, v) == 0
    assert _same(_arrays(one, kinds), _arrays(plain, kinds))


# ---- 6: the switch ---------------------------------------------------------------------------------------------------------------
def test_the_switch(gpu_lib):
    blob, a, state, slots, records, after = _cornell_case()
    ctx = _context(gpu_lib, blob, refit=False)
    before, frames = _arrays(ctx, (5, 6, 9)), _frames(ctx)
    keep, ps, pr = _on_device(slots, records)
    assert ctx.set_lights(slots, records) == 2 and ctx.set_lights_device(len(slots), ps, pr) == 2  # off: nothing touched
    assert _same(_arrays(ctx, (5, 6, 9)), before) and np.array_equal(_frames(ctx), frames)
    none = hip.Context(0, gpu_lib)
    none.refit_lights(True)
    assert none.set_lights(slots, records) == 2  # no scene
    # on, after the upload: the switch prepares the tables from the arrays read back
    assert ctx.refit_lights(True) == 0 and ctx.set_lights(slots, records) == 0
    got = _arrays(ctx)
    assert all(_equals_state(got, after))
    # off and on again: the posed lights keep their leaf words through the next refit
    assert ctx.refit_lights(False) == 0 and ctx.set_lights(slots, records) == 2
    assert ctx.refit_lights(True) == 0
    assert ctx.update_vertices(0, a.vertices) == 0
    assert _same(_arrays(ctx), got)
    # ... and one light moved back
    assert ctx.set_lights(slots[:1], state.lights[slots[:1]]) == 0
    rc, _, back = P.host_set_lights(after, slots[:1], state.lights[slots[:1]])
    assert rc == 0 and all(_equals_state(_arrays(ctx), back))
