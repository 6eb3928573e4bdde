"""k_light_pick_sparse (the light pick that evaluates only the occupied children of a node; shade_kernels.hip) against the kernels it
stands in for: k_light_pick_first with the table in LDS (RAYHIP_PICK_SPARSE=0) and with every row from memory (RAYHIP_PICK_LDS=0).
Round 6's form of the shade stage is pinned (RAYHIP_SHADE_SPLIT=29).  Every point gets the pick it got, so frames, variance images
and the kernel-level outputs of the shade stage are compared as raw bits.  tests/test_pick_sparse_host.py holds one level of the
descent in both forms against each other on the host."""
import os

import numpy as np
import pytest
import torch  # noqa: F401  (FIRST: torch brings its own HIP runtime, and it must be the one that opens the device -- tests/test_gpu_comm.py)

import light_refit_cases as L
import util
from ray_amd import api, hip

pytestmark = [pytest.mark.gpu]

MODES = {"sparse": {"RAYHIP_PICK_SPARSE": "1"}, "dense": {"RAYHIP_PICK_SPARSE": "0"}, "memory": {"RAYHIP_PICK_LDS": "0"}}
SWITCHES = ("RAYHIP_PICK_SPARSE", "RAYHIP_PICK_LDS", "RAYHIP_PICK_SPARSE_MAX_NODES")
bits = L.bits


@pytest.fixture(scope="module")
def gpu_lib():
    lib = hip.Library()
    assert lib.device_count() > 0, "no HIP device: the product has no CPU path, -m gpu tests cannot run here"
    return lib


_atrium = []


def atrium_blob():
    """scenes.atrium(s, 0.02): a light tree of several levels with sparse nodes; most shade points end their descent without a light"""
    if not os.path.exists(api.HIP_HOST_LIB):
        pytest.skip("libray_hip.so not built (needs the reference tree at build time)")
    if not _atrium:
        from ray_amd import scenes
        s = api.CreateSceneHIP(use_tex_compression=False)
        scenes.atrium(s, 0.02)
        _atrium.append(api.export_scene_blob(s))
    return _atrium[0]


def _context(lib, monkeypatch, mode, blob, w, h, refit=False, **env):
    """a context that reads the switches of `mode` (a context reads them when it is created)"""
    monkeypatch.setenv("RAYHIP_SHADE_SPLIT", "29")
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in {**MODES[mode], **env}.items():
        monkeypatch.setenv(name, value)
    ctx = hip.Context(0, lib)
    ctx.upload_static(util.pmj())
    ctx.resize(w, h)
    if refit:
        ctx.refit_lights(True)
    ctx.upload_scene_blob(blob)
    return ctx


def _passes(ctx):
    """a layered pass and a single-layer pass behind it"""
    ctx.render_batch(1, 6)
    ctx.render(7)
    return ctx.readback(hip.BUF_RAW).copy(), ctx.readback(hip.BUF_VARIANCE).copy()


def _shade_outputs(ctx, rays, hits, bounce, color):
    color, sec, sh = ctx.k_shade(bounce, 1, rays, hits, color)
    return color, util.sort_by_xy(sec), util.sort_by_xy(sh)


def _same_bits(x, y):
    return all(a.tobytes() == b.tobytes() for a, b in zip(x, y))


def test_the_tables_the_scenes_give_are_sparse():
    """what the frame comparisons below stand on: the atrium's light table has several levels and nodes with few occupied children"""
    a = L.Arrays(atrium_blob())
    rows = L.fill_children(a.cwnodes)
    arith = (rows[:, 10:18, 3] != 0) & (rows[:, 18:26, 3] != 0)
    inner = (rows[:, 0:2, :].reshape(-1, 8).view(np.uint32) & 0x80000000) == 0
    assert len(rows) > 9 and (inner & arith).sum() == len(rows) - 1  # (more than a root and its children)
    assert arith.sum(axis=1).min() <= 4 and arith.sum(axis=1).max() == 8


def test_atrium_frames_and_shade_outputs_are_the_same_bits(gpu_lib, monkeypatch):
    """160 x 90: 1350 chunks in the layered pass (the stacks fill, drain and fill again in every wavefront), 225 in the single-layer one;
    then the shade stage alone (rayhip_k_shade: the static chunk walk) on the scene's own primary and secondary rays"""
    blob = atrium_blob()
    got = {}
    for mode in MODES:
        ctx = _context(gpu_lib, monkeypatch, mode, blob, 160, 90)
        frames = _passes(ctx)
        rays, hits = ctx.k_generate_primary_rays(1)
        rays, hits, _ = ctx.k_intersect_closest(rays, hits, 1, flags=0)
        shade0 = _shade_outputs(ctx, rays, hits, 0, np.zeros((90, 160, 4), np.float32))
        rays1, hits1, _ = ctx.k_intersect_closest(shade0[1], np.zeros(len(shade0[1]), dtype=hip.HIT_DTYPE), 1, flags=0)
        shade1 = _shade_outputs(ctx, rays1, hits1, 1, shade0[0])
        got[mode] = (frames, shade0, shade1)
    assert float(got["dense"][0][0].sum()) > 0.0 and len(got["dense"][1][2]) > 0 and len(got["dense"][2][2]) > 0  # (lit pixels, shadow rays)
    for mode in ("sparse", "memory"):
        for part in range(3):
            assert _same_bits(got[mode][part], got["dense"][part]), (mode, part)


def test_every_analytic_light_type_and_a_box_less_child(gpu_lib, monkeypatch):
    """cornell_lights at 64 x 64: the directional light is a child without a box -- its flux is its importance, no arithmetic"""
    a = L.Arrays(util.golden_scene("cornell_lights"))
    rows = L.fill_children(a.cwnodes)
    assert ((rows[:, 10:18, 3] == 0) & (rows[:, 18:26, 3] != 0)).any()
    g = util.golden_ref("cornell_lights")
    got = {}
    for mode in MODES:
        ctx = _context(gpu_lib, monkeypatch, mode, util.golden_scene("cornell_lights"), 64, 64)
        frames = _passes(ctx)
        shade0 = _shade_outputs(ctx, g["primary_rays_traced"], g["primary_hits"], 0, np.zeros((64, 64, 4), np.float32))
        shade1 = _shade_outputs(ctx, g["secondary_rays_traced"], g["secondary_hits"], 1, g["shade0_color"])
        got[mode] = (frames, shade0, shade1)
    assert len(got["dense"][1][2]) > 0 and len(got["dense"][2][2]) > 0
    for mode in ("sparse", "memory"):
        for part in range(3):
            assert _same_bits(got[mode][part], got["dense"][part]), (mode, part)


@pytest.mark.parametrize("w,h", [(5, 3), (8, 8), (9, 8)])
def test_small_rects(gpu_lib, monkeypatch, w, h):
    """15, 64 and 72 primary points in single-layer passes: a partial first chunk, exactly one chunk, and a second chunk of eight --
    stacks that are drained with fewer than 64 points in them.  (Each pass over a rect starts from a fresh context.)"""
    blob = atrium_blob()
    got = {}
    for mode in ("sparse", "dense"):
        ctx = _context(gpu_lib, monkeypatch, mode, blob, 160, 90)
        for it in (1, 2, 3):
            ctx.render(it, rect=(70, 50, w, h))
        got[mode] = (ctx.readback(hip.BUF_RAW).copy(), ctx.readback(hip.BUF_VARIANCE).copy())
    assert float(got["dense"][0][50:50 + h, 70:70 + w, :3].sum()) > 0.0
    assert _same_bits(got["sparse"], got["dense"])


def test_an_emitter_without_area_beside_a_normal_one(gpu_lib, monkeypatch):
    """the fixture's lamp is two emissive triangles; a vertex update (with the device's light refit on) puts the corner only one of
    them has on the edge they share: that triangle light keeps its box and gets flux 0 (include/rayhip.h, rayhip_scene_refit_lights),
    the other stays an emitter.  The rows are rewritten on the device, and the occupancy the kernel derives from them follows."""
    blob = util.golden_scene("cornell_instances")
    a = L.Arrays(blob)
    tris = [int(a.lights[i, 4]) for i in a.tri_lights()]
    assert len(tris) == 2
    corners = [set(int(k) for k in a.vtx_indices[3 * t:3 * t + 3]) for t in tris]
    shared, own = sorted(corners[0] & corners[1]), sorted(corners[0] - corners[1])
    assert len(shared) == 2 and len(own) == 1
    v = a.vertices.copy()
    v["p"][own[0]] = np.float32(0.5) * (v["p"][shared[0]] + v["p"][shared[1]])
    got = {}
    for mode in ("sparse", "dense"):
        ctx = _context(gpu_lib, monkeypatch, mode, blob, 64, 64, refit=True)
        assert ctx.update_vertices(0, v) == 0
        rows = ctx.read_accel(6).reshape(-1, 26, 4)
        boxed, flux = rows[:, 10:18, 3] != 0, rows[:, 18:26, 3]
        assert (boxed & (flux == 0)).sum() >= 1 and (boxed & (flux != 0)).sum() >= 1
        got[mode] = _passes(ctx)
    assert float(got["dense"][0].sum()) > 0.0 and np.isfinite(got["dense"][0]).all()
    assert _same_bits(got["sparse"], got["dense"])


def test_a_table_above_the_cap_takes_the_dense_kernel(gpu_lib, monkeypatch):
    """RAYHIP_PICK_SPARSE_MAX_NODES=1: the launcher takes k_light_pick_first for the atrium, as it does for a scene above the kernel's own
    cap; the same frame as either kernel"""
    blob = atrium_blob()
    capped = _passes(_context(gpu_lib, monkeypatch, "sparse", blob, 160, 90, RAYHIP_PICK_SPARSE_MAX_NODES="1"))
    for mode in ("sparse", "dense"):
        assert _same_bits(capped, _passes(_context(gpu_lib, monkeypatch, mode, blob, 160, 90))), mode
