"""The direct-entry form of the persistent walks (k_trace_closest_refill<4, *, true>, k_trace_shadow_refill<*, true>): scenes whose top
level holds ONE instance over the 4-wide tree hand that instance to the kernels in their arguments, and no ray walks the top level.

Every comparison here is bit for bit between a context created with RAYHIP_DIRECT_ENTRY=0 (the generic kernels) and one created with
RAYHIP_DIRECT_ENTRY=1: the BUF_RAW frames of small renders (2 spp, depth 4: secondary bounces and shadow rays run), and at kernel level --
through the hooks, which launch what the passes launch -- the hit records of the closest-hit kernel and the throughputs of the any-hit kernel
on the same rays.  There is no tolerance.

Not covered: a mesh without triangles (a BLAS whose root is the sentinel) -- the scene API does not build one."""
import os

import numpy as np
import pytest

import test_gpu_walk_loop as WL  # the strip whose walks leave the LDS part of the stack, its rays
import util
from ray_amd import api, hip, scenes
from ray_amd.api import ShadingNode, eShadingNode

pytestmark = pytest.mark.gpu

W = H = 96  # 9216 pixels: room for the hooks' ray batches
SPP = 2
DEFAULT_ON = 1  # what a context does for a one-instance scene when RAYHIP_DIRECT_ENTRY is not set (profiles/direct_entry/README.md)
# rotation, non-uniform scale, translation
XFORM = dict(translate=(0.21, -0.13, 0.17), rot_y_deg=25.0, rot_z_deg=-10.0, scale=(1.3, 0.8, 1.1))
XFORM_MOVED = dict(translate=(0.15, -0.02, 0.05), rot_y_deg=-15.0, rot_z_deg=5.0, scale=(0.9, 1.1, 1.2))


@pytest.fixture(scope="module")
def gpu_lib():
    lib = hip.Library()
    assert lib.device_count() > 0, "no HIP device: the product has no CPU path, -m gpu tests cannot run here"
    return lib


def _bumpy_floor(u, v):
    """a patch above the floor of the box, 12 x 12 quads"""
    P = np.stack([-0.50 + 0.44 * u, 0.02 + 0.03 * np.sin(9.0 * u) * np.cos(7.0 * v), -0.50 + 0.44 * v], axis=-1)
    return P


def _camera_through(xf, **kw):
    """the Cornell camera carried along with the instance, so that the frame shows the box under any transform"""
    m = np.asarray(xf, np.float64).reshape(4, 4).T  # (column-major memory -> matrix)
    o = m @ np.array([-0.278, 0.273, 0.8, 1.0])
    f = m[:3, :3] @ np.array([0.0, 0.0, -1.0])
    f /= np.linalg.norm(f)
    return dict(origin=tuple(float(x) for x in o[:3]), fwd=tuple(float(x) for x in f), max_total_depth=4, **kw)


def box_scene(scene, solid=True, xform=XFORM, n_tris=None, **vis):
    """ONE mesh (the Cornell box with its blocks and lamp, a bumpy patch of 288 triangles on its floor), ONE instance of it under `xform`, a
    sphere light beside the lamp.  solid=False: the blocks are a Transparent / Diffuse mix and the patch is Transparent (all_solid == 0:
    transparency rounds in K2, throughputs multiplied in K3).  n_tris: only the first triangles of the floor instead (1 or 2: the BLAS root
    is a leaf word)"""
    scene.SetEnvironment(env_col=(0.05, 0.06, 0.08))
    grey = scene.AddMaterial(ShadingNode(type=eShadingNode.Diffuse, base_color=(0.5, 0.5, 0.5)))
    red = scene.AddMaterial(ShadingNode(type=eShadingNode.Diffuse, base_color=(0.5, 0.0, 0.0)))
    green = scene.AddMaterial(ShadingNode(type=eShadingNode.Diffuse, base_color=(0.0, 0.5, 0.0)))
    lamp = scene.AddMaterial(ShadingNode(type=eShadingNode.Emissive, strength=100.0, importance_sample=True))
    blue = scene.AddMaterial(ShadingNode(type=eShadingNode.Diffuse, base_color=(0.1, 0.2, 0.7)))
    if solid:
        blocks = patch = blue
    else:
        patch = scene.AddMaterial(ShadingNode(type=eShadingNode.Transparent, base_color=(0.7, 0.9, 0.7)))
        blocks = scene.AddMaterial(ShadingNode(type=eShadingNode.Mix, strength=0.5, mix_materials=(blue, patch)))
    attrs, idx = scenes.cornell_mesh_arrays()  # floor, ceiling, back | left | right | lamp | the two blocks
    if n_tris is not None:
        idx, groups = idx[:3 * n_tris], [(grey, None, 0, 3 * n_tris)]
    else:
        pa, pi = scenes._grid(12, 12, scenes._finite_normals(_bumpy_floor))
        groups = [(grey, None, 0, 18), (red, None, 18, 6), (green, None, 24, 6), (lamp, 0xFFFFFFFF, 30, 6), (blocks, blocks, 36, 60),
                  (patch, patch, 96, len(pi))]
        assert len(idx) == 96
        idx = np.concatenate([idx, pi + np.uint32(len(attrs))])
        attrs = np.concatenate([attrs, pa])
    mesh = scene.AddMesh(attrs, idx, groups)
    xf = scenes._xform(**xform)
    mi = scene.AddMeshInstance(mesh, xf, **vis)
    m = np.asarray(xf, np.float64).reshape(4, 4).T
    scene.AddLight("sphere", color=(6.0, 5.0, 4.0), position=tuple(float(x) for x in (m @ np.array([-0.2, 0.4, -0.2, 1.0]))[:3]), radius=0.02)
    scenes._cornell_camera(scene, **_camera_through(xf))
    scene.Finalize()
    return mi


def strip_scene_one(scene):
    """the strip of test_gpu_walk_loop.py as ONE instance, turned and moved (STRIP_XFORM: rigid, so that distances stay what they are): a chain
    the walk descends with a growing stack"""
    scene.SetEnvironment(env_col=(0.0, 0.0, 0.0))
    grey = scene.AddMaterial(ShadingNode(type=eShadingNode.Diffuse, base_color=(0.5, 0.5, 0.5)))
    pts = WL.strip_points()
    nrm = np.cross(pts[:, 1] - pts[:, 0], pts[:, 2] - pts[:, 0])
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    attrs = np.zeros((3 * len(pts), 8), dtype=np.float32)
    attrs[:, 0:3] = pts.reshape(-1, 3)
    attrs[:, 3:6] = np.repeat(nrm, 3, axis=0)
    mesh = scene.AddMesh(attrs, np.arange(len(attrs), dtype=np.uint32), [(grey, grey, 0, len(attrs))])
    scene.AddMeshInstance(mesh, scenes._xform(**STRIP_XFORM))
    scenes._cornell_camera(scene, origin=(0.5, 0.0, 0.0), fwd=(1.0, 0.0, 0.0))
    scene.Finalize()


STRIP_XFORM = dict(translate=(0.3, -0.2, 0.1), rot_y_deg=30.0, rot_z_deg=12.0)


def _carried(rays, xform):
    """rays of the instance's object space carried into the world"""
    m = np.asarray(scenes._xform(**xform), np.float64).reshape(4, 4).T
    out = rays.copy()
    out["o"] = rays["o"].astype(np.float64) @ m[:3, :3].T + m[:3, 3]
    d = rays["d"].astype(np.float64) @ m[:3, :3].T
    out["d"] = d / np.linalg.norm(d, axis=-1, keepdims=True)
    return out


_blobs = {}


def blob_of(key, build):
    if key not in _blobs:
        assert os.path.exists(api.HIP_HOST_LIB), "the drop-in's host library is not built (run __graft_entry__.build() where the reference tree is)"
        s = api.CreateSceneHIP()
        build(s)
        _blobs[key] = api.export_scene_blob(s)
    return _blobs[key]


def _context(lib, blob, monkeypatch, direct):
    monkeypatch.setenv("RAYHIP_DIRECT_ENTRY", "1" if direct else "0")  # (read when the context is created)
    ctx = hip.Context(0, lib)
    ctx.upload_static(util.pmj())
    ctx.resize(W, H)
    ctx.upload_scene_blob(blob)
    assert ctx.bvh_width() == 4
    assert ctx.direct_entry() == (1 if direct else 0)
    return ctx


def _both(lib, blob, monkeypatch):
    return _context(lib, blob, monkeypatch, False), _context(lib, blob, monkeypatch, True)


def _frames_identical(generic, direct, lit=True):
    a, b = util.render_frames(generic, SPP), util.render_frames(direct, SPP)
    assert np.isfinite(a).all()
    if lit:
        assert len(np.unique(a[..., :3].reshape(-1, 3), axis=0)) > 100  # (a picture, not a flat frame)
    assert a.tobytes() == b.tobytes()
    return a


def fan_rays(cam, n=4096, seed=11):
    """rays from around the camera into the scene (most hit, some leave through the open front), rays that miss the scene's bounds altogether,
    and rays through the world origin exactly -- where the duplicate link of a one-leaf top level has its point box"""
    rs = np.random.RandomState(seed)
    rays = np.zeros(n, dtype=hip.RAY_DTYPE)
    o = np.asarray(cam["origin"]) + rs.uniform(-0.05, 0.05, size=(n, 3))
    d = np.asarray(cam["fwd"]) + 0.4 * rs.normal(size=(n, 3))
    k = n // 4
    # away from everything: from far outside, pointing outwards
    o[:k] = rs.choice([-1.0, 1.0], size=(k, 3)) * rs.uniform(20.0, 30.0, size=(k, 3))
    d[:k] = o[:k] + rs.normal(size=(k, 3))
    # through (0, 0, 0) exactly: all three coordinates reach zero at the same t
    axes = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1], [1, 1, 1], [-1, 1, 1], [1, -1, 1], [1, 1, -1],
                     [-1, -1, -1], [1, 1, 0], [0, -1, 1], [-1, 0, -1]], dtype=np.float64)
    dz = axes[rs.randint(len(axes), size=k)]
    o[k:2 * k] = -dz * rs.choice([0.5, 1.0, 2.0, 4.0], size=(k, 1))
    d[k:2 * k] = dz
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    rays["o"], rays["d"] = o, d
    rays["pdf"], rays["c"], rays["ior"] = 1e6, 1.0, -1.0
    rays["xy"] = ((np.arange(n) % W) << 16) | (np.arange(n) // W)
    hits = np.zeros(n, dtype=hip.HIT_DTYPE)
    hits["obj_index"], hits["prim_index"], hits["t"], hits["v"] = -1, -1, 3.402823466e+38, -1.0
    return rays, hits


def fan_shadow_rays(cam, n=4096, seed=12):
    rays, _ = fan_rays(cam, n, seed)
    rs = np.random.RandomState(seed + 1)
    sh = np.zeros(n, dtype=hip.SHADOW_RAY_DTYPE)
    sh["o"], sh["d"] = rays["o"], rays["d"]
    sh["dist"] = np.where(rs.randint(4, size=n) == 0, -1.0, rs.uniform(0.0, 6.0, size=n))  # (<= 0: no limit; some shorter than HIT_BIAS allows)
    sh["c"] = rs.uniform(0.2, 1.0, size=(n, 3))
    sh["xy"] = rays["xy"]
    return sh


def _kernels_identical(generic, direct, rays, hits_in, shadow, monkeypatch, some_hit=True):
    """the closest-hit launch and the flat any-hit launch of both contexts on the same rays"""
    ra, ha, _ = generic.k_intersect_closest(rays, hits_in, 1, flags=0)
    rb, hb, _ = direct.k_intersect_closest(rays, hits_in, 1, flags=0)
    if some_hit:
        assert 0 < (ha["v"] >= 0).sum() < len(ha)
    util.assert_hits_identical(hb, ha)
    assert hb.tobytes() == ha.tobytes() and rb.tobytes() == ra.tobytes()
    monkeypatch.setenv("RAYHIP_HOOK_SHADOW_REFILL", "1")
    sa, _ = generic.k_intersect_shadow(shadow, 1)
    sb, _ = direct.k_intersect_shadow(shadow, 1)
    if some_hit:
        assert 0 < (sa[:, :3].max(axis=-1) > 0).sum() < len(sa)  # some blocked, some arrive
    assert sb.tobytes() == sa.tobytes()
    return ha, sa


def _cam(xform=XFORM):
    return _camera_through(scenes._xform(**xform))


@pytest.mark.parametrize("solid", [True, False], ids=["solid", "transparent"])
def test_transformed_instance(gpu_lib, monkeypatch, solid):
    """cases 1 and 2: rotation, non-uniform scale and translation; every side solid (the origin reload of the finish step is skipped), and with
    Transparent / Mix materials (the transparency round re-enters begin_round, the reload stays, K3 multiplies throughputs); case 4: rays that
    miss the bounds and rays through the world origin, at kernel level"""
    blob = blob_of(("box", solid), lambda s: box_scene(s, solid=solid))
    generic, direct = _both(gpu_lib, blob, monkeypatch)
    _frames_identical(generic, direct)
    rays, hits_in = fan_rays(_cam())
    ha, sa = _kernels_identical(generic, direct, rays, hits_in, fan_shadow_rays(_cam()), monkeypatch)
    k = len(rays) // 4
    assert (ha["v"][:k] < 0).all() and (ha["v"][k:2 * k] >= 0).any()  # outside the bounds: no hit; through the origin: some hit
    if not solid:
        part = (sa[:, :3].max(axis=-1) > 0) & (sa[:, :3] < fan_shadow_rays(_cam())["c"]).any(axis=-1)
        assert part.any()  # throughputs that crossed a surface and came out smaller


@pytest.mark.parametrize("hidden_from", ["camera", "shadow"])
def test_ray_visibility(gpu_lib, monkeypatch, hidden_from):
    """case 3: the instance hidden from one ray type -- begin_round ends the round at once"""
    blob = blob_of(("vis", hidden_from), lambda s: box_scene(s, **{hidden_from: False}))
    generic, direct = _both(gpu_lib, blob, monkeypatch)
    _frames_identical(generic, direct, lit=hidden_from != "camera")
    rays, hits_in = fan_rays(_cam())  # (depth 0: camera rays)
    ha, sa = _kernels_identical(generic, direct, rays, hits_in, fan_shadow_rays(_cam()), monkeypatch, some_hit=False)
    if hidden_from == "camera":
        assert (ha["v"] < 0).all()
    else:
        assert (ha["v"] >= 0).any() and sa[:, :3].tobytes() == fan_shadow_rays(_cam())["c"].astype(np.float32).tobytes()  # nothing blocks


@pytest.mark.parametrize("n_tris", [1, 2])
def test_root_is_a_leaf(gpu_lib, monkeypatch, n_tris):
    """case 5: a mesh of one or two triangles -- the word begin_round puts into `cur` is a leaf word"""
    blob = blob_of(("tiny", n_tris), lambda s: box_scene(s, n_tris=n_tris))
    generic, direct = _both(gpu_lib, blob, monkeypatch)
    _frames_identical(generic, direct, lit=False)
    rays, hits_in = fan_rays(_cam())
    shadow = fan_shadow_rays(_cam())
    # straight down onto the floor, whose first triangle(s) the mesh is, so that some rays do hit
    rs = np.random.RandomState(5)
    down = np.zeros(1024, dtype=hip.RAY_DTYPE)
    down["o"] = np.stack([rs.uniform(-0.55, 0.0, 1024), np.full(1024, 0.4), rs.uniform(-0.55, 0.0, 1024)], axis=-1)
    down["d"] = (0.0, -1.0, 0.0)
    down = _carried(down, XFORM)
    for batch in (rays, shadow):
        batch["o"][-1024:], batch["d"][-1024:] = down["o"], down["d"]
    shadow["dist"][-1024:] = 5.0
    _kernels_identical(generic, direct, rays, hits_in, shadow, monkeypatch)


def test_deep_stacks(gpu_lib, monkeypatch):
    """case 6: walks deeper than the LDS part of the stack (the strip of test_gpu_walk_loop.py): the single sentinel under a stack that spills"""
    blob = blob_of("strip", strip_scene_one)
    generic, direct = _both(gpu_lib, blob, monkeypatch)
    rays, hits_in = WL.strip_rays()
    rays, shadow = _carried(rays, STRIP_XFORM), _carried(WL.strip_shadow_rays(), STRIP_XFORM)
    tc = generic.k_intersect_closest(rays, hits_in, 1, flags=hip.FLAG_COUNT_WIDE)[2]
    assert tc["max_stack"] > WL.LDS_STACK_DEPTH + 3, tc
    _kernels_identical(generic, direct, rays, hits_in, shadow, monkeypatch)
    _frames_identical(generic, direct, lit=False)


def test_form_is_not_selected_elsewhere(gpu_lib, monkeypatch):
    """case 7: two instances, and the 8-wide tree, keep the generic kernels (the one-instance cases assert the selection in _context)"""
    monkeypatch.setenv("RAYHIP_DIRECT_ENTRY", "1")
    ctx = hip.Context(0, gpu_lib)
    ctx.upload_static(util.pmj())
    ctx.resize(W, H)
    ctx.upload_scene_blob(WL.strip_blob())  # the strip twice
    assert ctx.bvh_width() == 4 and ctx.direct_entry() == 0
    ctx.upload_scene_blob(blob_of(("box", True), lambda s: box_scene(s)))  # ... and the same context with one instance
    assert ctx.direct_entry() == 1
    monkeypatch.setenv("RAYHIP_BVH_WIDTH", "8")
    ctx8 = hip.Context(0, gpu_lib)
    ctx8.upload_static(util.pmj())
    ctx8.resize(W, H)
    ctx8.upload_scene_blob(blob_of(("box", True), lambda s: box_scene(s)))
    assert ctx8.bvh_width() == 8 and ctx8.direct_entry() == 0
    monkeypatch.delenv("RAYHIP_DIRECT_ENTRY")
    monkeypatch.delenv("RAYHIP_BVH_WIDTH")
    default = hip.Context(0, gpu_lib)
    default.upload_static(util.pmj())
    default.resize(W, H)
    default.upload_scene_blob(blob_of(("box", True), lambda s: box_scene(s)))
    assert default.direct_entry() == DEFAULT_ON


def test_moved_instance(gpu_lib, monkeypatch):
    """case 8: rayhip_scene_update_instances moves the one instance -- the next frame is the frame of a fresh upload with that transform, in
    both forms (the kernel arguments carry the new transform)"""
    if "moved" not in _blobs:
        assert os.path.exists(api.HIP_HOST_LIB), "the drop-in's host library is not built (run __graft_entry__.build() where the reference tree is)"
        s = api.CreateSceneHIP()
        mi = box_scene(s)
        before = api.export_scene_blob(s)
        s.SetMeshInstanceTransform(mi, scenes._xform(**XFORM_MOVED))
        s.Finalize()
        _blobs["moved"] = (before, api.export_scene_blob(s))
    before, after = _blobs["moved"]
    frames = {}
    for direct in (False, True):
        ctx = _context(gpu_lib, before, monkeypatch, direct)
        first = util.render_frames(ctx, SPP)
        assert ctx.update_instances(after) == 0
        assert ctx.direct_entry() == (1 if direct else 0)
        ctx.clear()
        updated = util.render_frames(ctx, SPP)
        fresh = util.render_frames(_context(gpu_lib, after, monkeypatch, direct), SPP)
        assert first.tobytes() != updated.tobytes()
        assert updated.tobytes() == fresh.tobytes()
        frames[direct] = updated
    assert frames[False].tobytes() == frames[True].tobytes()
