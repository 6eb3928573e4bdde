"""The environment changed on the device (rayhip_scene_set_environment, rayhip_scene_set_env_map and its _device form,
rayhip_scene_set_sky; ray_amd/csrc/env_qtree.h, env_qtree.hip.h, rayhip_environment.hip.h): colours and rotations; new texels for the
map, the importance quadtree rebuilt by kernels, the environment light's flux and the light tree behind it; the physical sky re-baked in
place.

What is asserted: the device's finest level lies, cell by cell, in the interval the float64 model of tests/env_cases.py allows (a tap
within DELTA of a texel's edge may read either texel; on the maps used there no tap lies so), and the whole quadtree equals the host
build's bit for bit on every map, since both take their sinf, cosf, acosf and atan2f from env_libm.h; upper levels, sums, flags and the level count equal the host build (tests/hostsim/hostsim_environment.cpp) run on the device's
finest level, bit for bit; the light tree, its rows and the leaf table equal the host build's refit under the new flux; frames equal
those of a fresh context that uploaded what the device holds, and pass the frame gate of tests/test_sky_bake.py against the reference's
render of the changed scene; a refused call leaves arrays and frames as they were; the calls commute with their siblings.
tests/test_env_hostsim.py holds the host build against the reference's own quadtrees."""
import os

import numpy as np
import pytest
import torch  # noqa: F401  (FIRST: torch brings its own HIP runtime, and it must be the one that opens the device -- tests/test_gpu_comm.py)

import env_cases as E
import light_pose_cases as P
import light_refit_cases as L
import util
import vertex_update_cases as V
from ray_amd import hip

pytestmark = [pytest.mark.gpu]

W, H, SPP = 96, 64, 4  # (tests/test_gpu_light_refit.py)
bits = L.bits
f32 = np.float32
KINDS = (5, 6, 9, 10, 12, 13, 14)


@pytest.fixture(scope="module")
def gpu_lib():
    lib = hip.Library()
    assert lib.device_count() > 0, "no HIP device: the product has no CPU path, -m gpu tests cannot run here"
    assert os.path.exists(E.ENV_LIB) and os.path.exists(P.POSE_LIB) and L.have_lights_lib(), "tests/hostsim is not built (run __graft_entry__.build())"
    assert E.O.have_ref(), "oracle/_ref is not built (needs the reference tree at build time)"
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


def _arrays(ctx, kinds=KINDS):
    return {k: ctx.read_accel(k).copy() for k in kinds}


def _same(x, y):
    return all(np.array_equal(bits(x[k]), bits(y[k])) for k in x)


def _same_frames(x, y):
    """bit for bit (the physical-sky scene at envmap_resolution 64 has pixels that are not finite, in the reference's render too)"""
    return np.array_equal(bits(x), bits(y))


def _env_of(words):
    """(the rayhip_environment, total_lum, medium_lum) of array 13"""
    return words[:16].view(E.ENV)[0], words[16:18].view(f32)[0], words[16:18].view(f32)[1]


def _texels_on_device(texels, offset_bytes=0):
    raw = np.zeros(offset_bytes + texels.nbytes, dtype=np.uint8)
    raw[offset_bytes:] = np.ascontiguousarray(texels).view(np.uint8).ravel()
    t = torch.from_numpy(raw).cuda()
    torch.cuda.synchronize()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + offset_bytes


def _upper_levels_are_sums(quads, levels):
    """every kept mip above the finest kept one is ((p0 + p1) + p2) + p3 of the quads below it, in float32"""
    mips = E.qtree_mips(quads, levels)
    for lod in range(1, levels):
        below = mips[lod - 1].astype(f32)
        sums = ((below[:, 0] + below[:, 1]) + below[:, 2]) + below[:, 3]
        n = int(round(np.sqrt(len(sums))))
        if not np.array_equal(bits(E.cell_grid(mips[lod])), bits(sums.reshape(n, n))):
            return False
    return True


def _host_lights_after(blob, flux):
    """the light arrays the host build leaves when the environment light's leaf takes `flux`: (state before, state after)"""
    a = L.Arrays(blob)
    state = P.State(a)
    env = int(E.blob_env(blob)["light_index"])
    posed = state.copy()
    posed.leaf["flux"][env] = flux
    posed.posed[env] = 1
    return state, P.host_refit_posed(posed)


def _check_built(ctx, img, got=None):
    """arrays 12, 13, 14 after a build over `img`: texels; upper levels, sums, flags and levels as the host build makes them of the
    device's finest level (where every level is kept and the finest one can be read) -- else the kept mips are each other's sums"""
    got = got or _arrays(ctx)
    t = E.texels_of(img)
    assert np.array_equal(got[14], t.ravel())
    env, total, medium = _env_of(got[13])
    levels = int(env["qtree_levels"])
    h, w = t.shape
    res = E.env_lib().hostsim_env_qtree_res(w, h)
    full = int(np.log2(res))
    assert _upper_levels_are_sums(got[12], levels)
    if levels == full:
        want = E.host_finish(res, got[12][:(res // 2) ** 2])
        assert want.kept == levels and np.array_equal(bits(got[12]), bits(want.kept_quads()))
        assert bits(np.array([total, medium], dtype=f32)).tolist() == bits(np.array([want.total, want.medium], dtype=f32)).tolist()
    top = got[12][-1].astype(f32)
    assert total == ((top[0] + top[1]) + top[2]) + top[3] and medium == total / f32((res // 2) * (res // 2))
    return got, levels, medium


# ---- 1: the device's finest level against the float64 model; the rest against the host build -----------------------------------------
@pytest.mark.parametrize("name", E.DEVICE_MODEL_MAPS)
def test_finest_level_lies_in_the_models_intervals(gpu_lib, name):
    img = E.env_map(name)
    m = E.Model(img)
    assert m.ambiguous.mean() <= 0.01 and m.kept == m.levels and m.threshold_margin() >= 1e-4  # conditions, on the model
    ctx = _context(gpu_lib, E.map_blob(name))
    assert ctx.set_env_map(img) == 0
    got, levels, medium = _check_built(ctx, img)
    assert levels == m.kept
    finest = E.cell_grid(got[12][:(m.res // 2) ** 2]).astype(np.float64)
    low, high = finest < m.lo * (1 - 29 * E.EPS), finest > m.hi * (1 + 29 * E.EPS)
    host = E.cell_grid(E.host_pyramid(img).mip(0))
    print(f"{name}: res {m.res}, {int(m.ambiguous.sum())} ambiguous taps of {m.ambiguous.size}; {int((bits(finest.astype(f32)) != bits(host)).sum())} of "
          f"{finest.size} cells differ from the host build's; largest miss of an interval {float(np.maximum(m.lo - finest, finest - m.hi).max()):.3e}")
    assert not low.any() and not high.any(), (name, int(low.sum()), int(high.sum()))
    bound = (25 + 2 * np.log2(m.res) + 4) * E.EPS
    if not m.ambiguous.any():
        assert abs(float(medium) - m.medium) <= bound * m.medium


@pytest.mark.parametrize("name", ["16x8", "64x32", "100x50", "rgbe_sky", "uniform", "black", "one_texel", "sun_moved"] + list(E.DEVICE_MODEL_MAPS))
def test_quadtree_equals_the_host_build_on_every_map(gpu_lib, name):
    """the maps of tests/test_env_hostsim.py, on most of which nearly every tap lies exactly on a texel's edge: kept levels, level count,
    sums and the environment leaf's flux are the host build's bit for bit -- and with that the reference's levels"""
    img = E.env_map(name)
    ctx = _context(gpu_lib, E.map_blob(name))
    uploaded = ctx.read_accel(12).copy()
    assert ctx.set_env_map(img) == 0
    got, levels, medium = _check_built(ctx, img)
    want = E.host_pyramid(img)
    assert levels == want.kept and np.array_equal(bits(got[12]), bits(want.kept_quads())), (name, levels, want.kept)
    assert np.array_equal(bits(got[12]), bits(uploaded))  # (the reference built its tree on the same map)
    env, total, _ = _env_of(got[13])
    assert bits(np.array([total, medium], dtype=f32)).tolist() == bits(np.array([want.total, want.medium], dtype=f32)).tolist()
    w_, i_ = E.env_leaf(got[5], int(env["light_index"]))
    assert bits(got[5]["flux"][w_, i_:i_ + 1])[0] == bits(np.array([want.flux], dtype=f32))[0]


# ---- 2: set_env_map in its three forms ---------------------------------------------------------------------------------------------------
def test_three_forms_leave_the_same_arrays(gpu_lib):
    blob, img = E.map_blob("rgbe_sky"), E.env_map("sun_moved")
    t = E.texels_of(img)
    results = []
    for form in ("host", "device", "device+4"):
        ctx = _context(gpu_lib, blob)
        before = _arrays(ctx)
        assert np.array_equal(bits(before[12]), bits(E.blob_qtree(blob))) and np.array_equal(before[14], E.blob_env_texels(blob).ravel())
        if form == "host":
            assert ctx.set_env_map(img) == 0
        else:
            keep, p = _texels_on_device(t, 4 if form == "device+4" else 0)
            assert ctx.set_env_map_device(t.shape[1], t.shape[0], p) == 0
            del keep
        got, levels, medium = _check_built(ctx, img)
        assert not np.array_equal(bits(got[12]), bits(before[12]))
        # tree, rows and leaf table: the host build's refit with the new flux
        state, want = _host_lights_after(blob, medium)
        assert np.array_equal(bits(before[5]), bits(state.cwnodes)) and np.array_equal(bits(before[10]).ravel(), bits(state.leaf).ravel())
        assert np.array_equal(bits(got[5]), bits(want.cwnodes)) and np.array_equal(bits(got[6]), bits(want.children))
        assert np.array_equal(bits(got[10]).ravel(), bits(want.leaf).ravel()) and np.array_equal(bits(got[9]), bits(state.lights))
        w_, i_ = E.env_leaf(got[5], int(E.blob_env(blob)["light_index"]))
        assert got[5]["flux"][w_, i_] == medium and not np.array_equal(bits(got[5]), bits(before[5]))
        # a second identical call leaves the same bytes (the other half of the double buffer)
        assert ctx.set_env_map(img) == 0 and _same(_arrays(ctx), got)
        results.append(got)
    assert _same(results[0], results[1]) and _same(results[0], results[2])


def test_levels_grow_and_shrink(gpu_lib):
    uniform, one = E.env_map("uniform"), E.env_map("one_texel")
    ctx = _context(gpu_lib, E.map_blob("uniform"))
    assert _env_of(ctx.read_accel(13))[0]["qtree_levels"] == 4
    assert ctx.set_env_map(one) == 0
    got, levels, _ = _check_built(ctx, one)
    assert levels == 5 and len(got[12]) == 256 + 64 + 16 + 4 + 1
    assert np.isfinite(_frames(ctx)).all()
    assert ctx.set_env_map(uniform) == 0
    got, levels, medium = _check_built(ctx, uniform)
    assert levels == 4 and len(got[12]) == 64 + 16 + 4 + 1
    assert abs(float(medium) - float(E.host_pyramid(uniform).medium)) <= 33 * E.EPS * float(medium)
    back = _context(gpu_lib, E.map_blob("one_texel"))
    assert _env_of(back.read_accel(13))[0]["qtree_levels"] == 5 and back.set_env_map(uniform) == 0
    assert _same(_arrays(back, (12, 14)), {k: got[k] for k in (12, 14)}) and _env_of(back.read_accel(13))[0]["qtree_levels"] == 4


# ---- 3: frames ---------------------------------------------------------------------------------------------------------------------
def _fresh_with_what_the_device_holds(lib, blob, got):
    env = _env_of(got[13])[0]
    patched = E.with_qtree(E.with_env_texels(V.patched_blob(blob, lights=got[9], light_cwnodes=got[5]), got[14]), got[12], int(env["qtree_levels"]))
    return _context(lib, patched, refit=False)


def test_frames_after_the_sun_moved(gpu_lib):
    blob, img = E.map_blob("rgbe_sky"), E.env_map("sun_moved")
    ctx = _context(gpu_lib, blob)
    first = _frames(ctx)
    assert ctx.set_env_map(img) == 0
    updated, got = _frames(ctx), _arrays(ctx)
    fresh = _fresh_with_what_the_device_holds(gpu_lib, blob, got)
    assert np.array_equal(bits(fresh.read_accel(12)), bits(got[12])) and np.array_equal(bits(fresh.read_accel(6)), bits(got[6]))
    assert np.array_equal(updated, _frames(fresh)) and not np.array_equal(updated, first) and np.isfinite(updated).all()


def test_frame_gate_against_the_reference_after_the_sun_moved(gpu_lib):
    """The frame after the call against the reference's render of the scene it built on the new map, by the gate of
    tests/test_sky_bake.py (util.MIN_FRACTION of the pixels within tolerance, PSNR >= 55).  The map is 128 x 64 and the level's res
    32, so u * w = j * 128 / 64 is a whole number for EVERY tap and the texel read hangs on the last bit of atan2f: the gate holds
    because env_libm.h gives the device the reference's bits there (with the device's own libm 53 of 1364 cells differed, and 54.5 % of
    the pixels were within tolerance at PSNR 18.1)."""
    blob, img = E.map_blob("rgbe_sky"), E.env_map("sun_moved")
    ctx = _context(gpu_lib, blob)
    assert ctx.set_env_map(img) == 0
    updated = _frames(ctx)
    ref = E.reference_render(("map", "sun_moved"), lambda s: E.env_scene(s, img), W, H, SPP)
    m = util.frame_metrics(updated, ref)
    refq, devq = E.blob_qtree(E.map_blob("sun_moved")), ctx.read_accel(12)
    print("sun moved, against the reference's render of the scene built on the new map:", m, "|", int((bits(refq) != bits(devq)).sum()), "of", refq.size,
          "quadtree cells differ from the reference's")
    assert m["frac_within"] >= util.MIN_FRACTION and m["psnr"] >= 55.0, m
    assert np.array_equal(bits(refq), bits(devq))  # (every level is kept: the finest one is the reference's too)


def test_the_environment_leaf_flux_is_fair_to_the_pick(gpu_lib):
    """cornell_env with one rect light beside the environment light, the sun moved: 64 x 64, 256 samples per pixel, the frame mean under
    the refitted tree against the mean under the tree the reference built for the new map; the noise floor as
    tests/test_gpu_light_pose.py::test_the_refitted_tree_is_a_fair_sampler measures it."""
    img = E.env_map("sun_moved")
    ctx = _context(gpu_lib, E.map_blob("rgbe_sky", True), w=64, h=64)
    assert ctx.set_env_map(img) == 0
    refitted = float(_frames(ctx, 256)[..., :3].astype(np.float64).mean())
    rebuilt = _context(gpu_lib, E.map_blob("sun_moved", True), refit=False, w=64, h=64)
    rebuilt.clear()
    m256 = float(util.render_frames(rebuilt, 256)[..., :3].astype(np.float64).mean())
    for it in range(257, 513):
        rebuilt.render(it)
    m512 = float(rebuilt.readback(hip.BUF_RAW)[..., :3].astype(np.float64).mean())
    second = 2.0 * m512 - m256
    floor, gap = abs(m256 - second), abs(refitted - m256)
    print(f"frame mean: refitted tree {refitted:.6f}, reference-built tree {m256:.6f} (iterations 1..256) and {second:.6f} (257..512); "
          f"refit against rebuilt {gap:.3e}, noise floor {floor:.3e}")
    assert m256 > 0 and gap <= 3.0 * floor


# ---- 4: set_environment ----------------------------------------------------------------------------------------------------------------
def test_set_environment_equals_a_fresh_upload(gpu_lib):
    blob = E.map_blob("rgbe_sky")
    ctx = _context(gpu_lib, blob)
    first, before = _frames(ctx), _arrays(ctx)
    fields = dict(env_col=(0.8, 0.9, 1.1), back_col=(0.5, 0.6, 0.4), env_map_rotation=1.2, back_map_rotation=-0.7)
    assert ctx.set_environment(fields["env_col"], fields["back_col"], fields["env_map_rotation"], fields["back_map_rotation"]) == 0
    after = _arrays(ctx)
    assert _same({k: after[k] for k in (5, 6, 9, 10, 12, 14)}, {k: before[k] for k in (5, 6, 9, 10, 12, 14)})
    env = _env_of(after[13])[0]
    assert env["env_col"].tolist() == np.asarray(fields["env_col"], dtype=f32).tolist() and env["back_map_rotation"] == f32(-0.7)
    updated = _frames(ctx)
    fresh = _context(gpu_lib, E.with_env(blob, **fields), refit=False)
    assert np.array_equal(updated, _frames(fresh)) and not np.array_equal(updated, first)


# ---- 5: the physical sky -----------------------------------------------------------------------------------------------------------------
def _sky_case():
    blob = E.reference_blob(("sky", False), lambda s: E.sky_scene(s))
    moved = E.reference_blob(("sky", True), lambda s: E.sky_scene(s, moved=True))
    slots = E.section(blob, "sky_dir_lights", "<u4")
    assert len(slots) == 1 and np.array_equal(slots, E.section(moved, "sky_dir_lights", "<u4"))
    records = L.Arrays(moved).lights[slots]
    return blob, moved, slots, records, E.section(moved, "sky", np.uint8), E.section(moved, "sky_transmittance_lut", "<f4"), E.section(moved, "sky_multiscatter_lut", "<f4")


def test_set_sky_rebakes_and_rebuilds(gpu_lib):
    """The baked map is 64 x 32: nearly every tap lies exactly on a texel's edge in x, so the model's intervals span both readings there
    -- the check bites less than on the maps of test 1, which is why those are other maps; the bake itself is held bit for bit."""
    blob, moved, slots, records, sky, tlut, mlut = _sky_case()
    ctx = _context(gpu_lib, blob)
    first, before = _frames(ctx), _arrays(ctx)
    assert ctx.set_sky(slots, records, sky, tlut, mlut) == 0
    got = _arrays(ctx)
    _, w, h = E.blob_env_map(blob)
    baked = hip.Context(0, gpu_lib).bake_sky(w, h, moved)  # the same kernel on the same inputs
    assert np.array_equal(got[14], E.texels_of(baked).ravel()) and not np.array_equal(got[14], before[14])
    assert np.array_equal(bits(got[9][slots]), bits(records)) and not np.array_equal(bits(got[9]), bits(before[9]))
    _, levels, medium = _check_built(ctx, baked, got)
    m = E.Model(baked)
    if levels == m.levels:
        finest = E.cell_grid(got[12][:(m.res // 2) ** 2]).astype(np.float64)
        assert (finest >= m.lo * (1 - 29 * E.EPS)).all() and (finest <= m.hi * (1 + 29 * E.EPS)).all()
    state, want = _host_lights_after(V.patched_blob(blob, lights=got[9]), medium)
    assert np.array_equal(bits(got[5]), bits(want.cwnodes)) and np.array_equal(bits(got[10]).ravel(), bits(want.leaf).ravel())
    assert not _same_frames(_frames(ctx), first)
    # the suns alone, then the sky alone: the same state
    two = _context(gpu_lib, blob)
    assert two.set_sky(slots, records) == 0 and two.set_sky(sky=sky, transmittance_lut=tlut, multiscatter_lut=mlut) == 0
    assert _same(_arrays(two), got)


def test_frame_gate_against_the_reference_after_the_sky_moved(gpu_lib):
    """The frame after set_sky against the reference's render of the moved scene, by the same gate on the full frame: floor and walls
    under the re-baked map, and -- the analytic narrow-ray path -- the sky behind the box and the sun's reflection in the mirror block.
    The frame before the call does not pass it.

    The REFERENCE's own render of cornell_sky at envmap_resolution 64 has pixels that are not finite (801 of 6144 before the move, 202
    after it; a plain upload of the reference-built scene has them at the same pixels), and util.frame_metrics of such a frame is nan.
    So the pixels that are not finite must be the reference's, one for one, and the gate is taken over all the others."""
    blob, moved, slots, records, sky, tlut, mlut = _sky_case()
    ctx = _context(gpu_lib, blob)
    first = _frames(ctx)
    assert ctx.set_sky(slots, records, sky, tlut, mlut) == 0
    updated = _frames(ctx)
    ref = E.reference_render(("sky", True), lambda s: E.sky_scene(s, moved=True), W, H, SPP)
    ok = np.isfinite(ref).all(axis=-1)
    assert np.array_equal(np.isfinite(updated).all(axis=-1), ok) and ok.mean() > 0.9
    mt, before_gate = util.frame_metrics(updated[ok][None], ref[ok][None]), util.frame_metrics(np.nan_to_num(first[ok][None]), ref[ok][None])
    print("sky moved, against the reference's render of the moved scene:", mt, "| the frame before the call:", before_gate, "|", int((~ok).sum()),
          "pixels of the reference's frame are not finite")
    assert before_gate["frac_within"] < util.MIN_FRACTION or before_gate["psnr"] < 55.0
    assert mt["frac_within"] >= util.MIN_FRACTION and mt["psnr"] >= 55.0, mt


# ---- 6: refusals -------------------------------------------------------------------------------------------------------------------
def test_a_refused_call_touches_nothing(gpu_lib):
    blob, img = E.map_blob("rgbe_sky"), E.env_map("sun_moved")
    ctx = _context(gpu_lib, blob)
    assert ctx.set_env_map(img) == 0  # (a built pyramid is live)
    before, frames = _arrays(ctx), _frames(ctx)
    t = E.texels_of(img)
    nan, inf = float("nan"), float("inf")
    one, rot = (1.0, 1.0, 1.0), (0.3, 0.3)
    fn = gpu_lib.fn
    with pytest.raises(RuntimeError, match="64 x 32"):
        ctx.set_env_map(E.env_map("64x32"))
    keep, p = _texels_on_device(t)
    with pytest.raises(RuntimeError, match="64 x 128"):
        ctx.set_env_map_device(64, 128, p)
    with pytest.raises(RuntimeError, match="null pointer"):
        ctx.set_env_map_device(128, 64, 0)
    with pytest.raises(RuntimeError, match="4-byte aligned"):
        ctx.set_env_map_device(128, 64, p + 2)
    for env_col, back_col, r, match in (((1.0, nan, 1.0), one, rot, "negative or not finite"), (one, (1.0, 1.0, -0.5), rot, "negative or not finite"),
                                        (one, (inf, 1.0, 1.0), rot, "negative or not finite"), (one, one, (nan, 0.0), "rotation"), (one, one, (0.0, inf), "rotation"),
                                        ((1.0, 0.0, 1.0), one, rot, "environment light")):
        with pytest.raises(RuntimeError, match=match):
            ctx.set_environment(env_col, back_col, *r)
    assert fn("scene_set_environment")(ctx._ctx, None, None, 0.0, 0.0) == 1 and "null pointer" in gpu_lib.fn("last_error")().decode()
    with pytest.raises(RuntimeError, match="null pointer"):
        ctx.set_sky(sky=np.zeros(256, np.uint8))  # the sky without its tables
    assert fn("scene_set_sky")(ctx._ctx, 1, None, None, None, None, None) == 1
    assert ctx.set_sky([0], np.zeros((1, 16), np.uint32)) == 2  # no physical sky
    assert _same(_arrays(ctx), before)
    # the switch: a scene with an environment light needs it; the context renders what it rendered
    off = _context(gpu_lib, blob, refit=False)
    held, held_frames = _arrays(off, (5, 6, 9, 12, 13, 14)), _frames(off)
    assert off.set_env_map(img) == 2 and off.set_env_map_device(128, 64, p) == 2
    assert _same(_arrays(off, (5, 6, 9, 12, 13, 14)), held) and np.array_equal(_frames(off), held_frames)
    assert off.set_environment((0.5, 0.5, 0.5), one, 0.0, 0.0) == 0  # (no tree behind it: no switch needed)
    # no scene; a scene without an environment map
    none = hip.Context(0, gpu_lib)
    none.refit_lights(True)
    assert none.set_env_map(img) == 2 and none.set_environment(one, one, 0.0, 0.0) == 2 and none.set_sky([0], np.zeros((1, 16), np.uint32)) == 2
    plain = _context(gpu_lib, util.golden_scene("cornell_instances"))
    kinds = (5, 6, 9, 10, 12, 13, 14)
    plain_before = _arrays(plain, kinds)
    assert plain.set_env_map(img) == 2 and "no environment map" in gpu_lib.fn("last_error")().decode()
    assert _same(_arrays(plain, kinds), plain_before)
    # the physical sky: bad slots, records and tables
    sblob, moved, slots, records, sky, tlut, mlut = _sky_case()
    sctx = _context(gpu_lib, sblob)
    sbefore, sframes = _arrays(sctx), _frames(sctx)
    env_slot = np.array([E.blob_env(sblob)["light_index"]], dtype=np.uint32)
    bad = records.copy()
    bad[0, 0] ^= 1 << 4
    nf = records.copy()
    nf[0, 5] = np.array([nan], dtype=f32).view(np.uint32)[0]
    bad_sky = sky.copy()
    bad_sky.view(np.int32)[52] += 1  # transmittance_lut_w
    nan_sky = sky.copy()
    nan_sky.view(f32)[9] = nan  # clouds_offset_x
    nan_lut = tlut.copy()
    nan_lut[7] = nan
    for call, match in ((lambda: sctx.set_sky(env_slot, records), "none of the"), (lambda: sctx.set_sky([len(sbefore[9])], records), "none of the"),
                        (lambda: sctx.set_sky(np.repeat(slots, 2), np.repeat(records, 2, axis=0)), "more than once"), (lambda: sctx.set_sky(slots, bad), "word 0"),
                        (lambda: sctx.set_sky(slots, nf), "not finite"), (lambda: sctx.set_sky(slots, records, bad_sky, tlut, mlut), "sizes"),
                        (lambda: sctx.set_sky(slots, records, nan_sky, tlut, mlut), "not finite"), (lambda: sctx.set_sky(slots, records, sky, nan_lut, mlut), "not finite")):
        with pytest.raises(RuntimeError, match=match):
            call()
        assert _same(_arrays(sctx), sbefore), match
    assert sctx.set_sky() == 0 and _same(_arrays(sctx), sbefore)  # nothing named
    soff = _context(gpu_lib, sblob, refit=False)
    assert soff.set_sky(slots, records, sky, tlut, mlut) == 2
    assert _same_frames(_frames(sctx), sframes)
    del keep
    assert _same(_arrays(ctx), before) and np.array_equal(_frames(ctx), frames)


# ---- 7: commuting ----------------------------------------------------------------------------------------------------------------
def test_it_commutes_with_set_lights_and_survives_moved_instances(gpu_lib):
    blob, img = E.map_blob("rgbe_sky", True), E.env_map("sun_moved")
    a = L.Arrays(blob)
    rect = next(s for s in P.analytic_slots(a) if a.lights[s, 0] & 7 == P.TYPE_RECT)
    slots = np.array([rect], dtype=np.uint32)
    records = np.array([P.pack("rect", a.lights[rect, 0], color=(3.0, 5.0, 6.0), width=0.2, height=0.1, xform=P.scenes._translate(-0.2, 0.5, -0.3, rot_x_deg=10.0))],
                       dtype=np.uint32)
    one, other = _context(gpu_lib, blob), _context(gpu_lib, blob)
    rest = _arrays(one)
    assert one.set_env_map(img) == 0 and one.set_lights(slots, records) == 0
    assert other.set_lights(slots, records) == 0 and other.set_env_map(img) == 0
    got = _arrays(one)
    assert _same(got, _arrays(other)) and not np.array_equal(bits(got[5]), bits(rest[5]))
    assert np.array_equal(_frames(one), _frames(other))
    # moved instances: the environment leaf keeps its new flux in the leaf table and in the tree
    env = int(E.blob_env(blob)["light_index"])
    medium = _env_of(got[13])[2]
    xform = a.mesh_instances["xform"][:1].astype(f32).reshape(1, 16).copy()
    xform[0, 12] += f32(0.01)
    assert one.set_instance_transforms(np.array([0], dtype=np.uint32), xform) == 0
    after = _arrays(one)
    w_, i_ = E.env_leaf(after[5], env)
    assert after[10][env, 6] == medium and after[5]["flux"][w_, i_] == medium
    assert _same({k: after[k] for k in (12, 13, 14)}, {k: got[k] for k in (12, 13, 14)})
    # an instance update brings the host's environment and quadtree; the texels stay
    assert one.update_instances(blob) == 0
    back = _arrays(one)
    assert np.array_equal(bits(back[12]), bits(E.blob_qtree(blob))) and np.array_equal(bits(back[5]), bits(a.cwnodes)) and np.array_equal(back[14], got[14])
