"""The walk loop of the persistent traversal kernels (k_trace_closest_refill, k_trace_shadow_refill) and of walk_bvh4, on what the committed
scenes do not reach: stacks that leave the LDS part, and launches whose wavefronts are partly filled.

Everything goes through the hooks (k_intersect_closest(..., flags=0), k_intersect_shadow) and is compared bit for bit with the host build of
the same sources (tests/hostsim), which walks one ray at a time: no ballots, no votes, no LDS.

The strip: triangles along +x whose size grows geometrically, so that a top-down builder peels them off one at a time and the tree is a
chain.  A ray that starts at the small end and looks along the strip enters the cluster of small triangles first at every node and pushes
the large siblings: its stack grows with every level.  Found on the host build: N_STRIP triangles at RATIO give a deepest stack of 34
entries (LDS_STACK_DEPTH is 24), and most rays of the fan end their walk inside the chain, i.e. pop straight down to the sentinel."""
import os

import numpy as np
import pytest

import oracle_lib as O
import util
from ray_amd import api, hip, scenes
from ray_amd.api import ShadingNode, eShadingNode

pytestmark = pytest.mark.gpu

LDS_STACK_DEPTH = 24  # kernels.hip.h: RT_LDS_STACK_DEPTH
N_STRIP, RATIO = 2400, 1.006
N_RAYS = 4096
W = H = 65  # 4225 pixels: room for 4097 rays in the wavefront buffers


@pytest.fixture(scope="module")
def gpu_lib():
    lib = hip.Library()
    assert lib.device_count() > 0, "no HIP device: the product has no CPU path, -m gpu tests cannot run here"
    return lib


@pytest.fixture(scope="module")
def hostsim_lib():
    assert O.have_hostsim(), "tests/hostsim is not built (run __graft_entry__.build())"
    return hip.Library(O.HOSTSIM_LIB, prefix="hostsim_")


def strip_points(n=N_STRIP, ratio=RATIO):
    """[n][3][3]: triangle k spans x in [x_k, x_k r] with x_k = r^k, as high and as deep as it is long, leaning so that its box has a volume"""
    x0 = ratio ** np.arange(n, dtype=np.float64)
    s = x0 * (ratio - 1.0)
    sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    a = np.stack([x0, -0.5 * s, -0.5 * s * sign], axis=-1)
    b = np.stack([x0 + s, 0.5 * s, -0.5 * s * sign], axis=-1)
    c = np.stack([x0 + 0.5 * s, 0.0 * s, 0.5 * s * sign], axis=-1)
    return np.stack([a, b, c], axis=1).astype(np.float32)


def strip_scene(scene):
    """the strip twice (the second instance turned and lifted: a top level with two overlapping instances) and nothing else"""
    scene.SetEnvironment(env_col=(0.0, 0.0, 0.0))
    grey = scene.AddMaterial(ShadingNode(type=eShadingNode.Diffuse, base_color=(0.5, 0.5, 0.5)))
    pts = strip_points()
    nrm = np.cross(pts[:, 1] - pts[:, 0], pts[:, 2] - pts[:, 0])
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    attrs = np.zeros((3 * len(pts), 8), dtype=np.float32)
    attrs[:, 0:3] = pts.reshape(-1, 3)
    attrs[:, 3:6] = np.repeat(nrm, 3, axis=0)
    mesh = scene.AddMesh(attrs, np.arange(len(attrs), dtype=np.uint32), [(grey, grey, 0, len(attrs))])
    scene.AddMeshInstance(mesh)
    scene.AddMeshInstance(mesh, scenes._xform(translate=(0.0, 0.02, 0.0), rot_y_deg=3.0))
    scenes._cornell_camera(scene, origin=(0.5, 0.0, 0.0), fwd=(1.0, 0.0, 0.0))
    scene.Finalize()


_cache = {}


def strip_blob():
    if "blob" not in _cache:
        assert os.path.exists(api.HIP_HOST_LIB), "the drop-in's host library is not built (run __graft_entry__.build() where the reference tree is)"
        s = api.CreateSceneHIP()
        strip_scene(s)
        _cache["blob"] = api.export_scene_blob(s)
    return _cache["blob"]


def strip_rays(n=N_RAYS, seed=3):
    """a fan from in front of the small end along the strip: most rays graze the chain of boxes, a few hit a triangle far out"""
    rs = np.random.RandomState(seed)
    rays = np.zeros(n, dtype=hip.RAY_DTYPE)
    rays["o"] = np.array([0.9, 0.0, 0.0]) + rs.uniform(-1.0, 1.0, size=(n, 3)) * np.array([0.05, 0.002, 0.002])
    d = np.stack([np.ones(n), rs.normal(size=n) * 2e-3, rs.normal(size=n) * 2e-3], axis=-1)
    rays["d"] = d / np.linalg.norm(d, axis=-1, keepdims=True)
    rays["pdf"], rays["c"], rays["ior"] = 1e6, 1.0, -1.0
    rays["xy"] = ((np.arange(n) % W) << 16) | (np.arange(n) // W)
    hits = np.zeros(n, dtype=hip.HIT_DTYPE)
    hits["obj_index"], hits["prim_index"], hits["t"], hits["v"] = -1, -1, 3.402823466e+38, -1.0
    return rays, hits


def strip_shadow_rays(n=N_RAYS, seed=4):
    """shadow rays aimed through the strip, from the small end to points beside its far end (finite distances: some end inside the chain)"""
    rs = np.random.RandomState(seed)
    rays = np.zeros(n, dtype=hip.SHADOW_RAY_DTYPE)
    rays["o"] = np.array([0.9, 0.0, 0.0]) + rs.uniform(-1.0, 1.0, size=(n, 3)) * np.array([0.05, 0.002, 0.002])
    d = np.stack([np.ones(n), rs.normal(size=n) * 2e-3, rs.normal(size=n) * 2e-3], axis=-1)
    rays["d"] = d / np.linalg.norm(d, axis=-1, keepdims=True)
    rays["dist"] = RATIO ** rs.uniform(0.0, N_STRIP, size=n)
    rays["c"] = 1.0
    rays["xy"] = ((np.arange(n) % W) << 16) | (np.arange(n) // W)
    return rays


def _context(lib, blob, w=W, h=H):
    ctx = hip.Context(0, lib)
    ctx.upload_static(util.pmj())
    ctx.resize(w, h)
    ctx.upload_scene_blob(blob)
    return ctx


def _host_env(monkeypatch):
    """the trees the device walks: leaves refined to <= 2 triangles, no layout pass, collapsed four wide"""
    monkeypatch.setenv("HOSTSIM_REFINE", "2")
    monkeypatch.setenv("HOSTSIM_NO_LAYOUT", "1")
    monkeypatch.setenv("HOSTSIM_BVH4", "1")


def host_strip(hostsim_lib, monkeypatch):
    """(hits, counters) of the fan and the throughputs of the shadow rays in the host build, computed once"""
    if "host" not in _cache:
        _host_env(monkeypatch)
        host = _context(hostsim_lib, strip_blob())
        rays, hits_in = strip_rays()
        _, hits, tc = host.k_intersect_closest(rays, hits_in, 1, flags=hip.FLAG_COUNT_WIDE)
        rc, tc_sh = host.k_intersect_shadow(strip_shadow_rays(), 1)
        _cache["host"] = (hits, tc, rc, tc_sh)
    return _cache["host"]


def test_deep_stacks_closest(gpu_lib, hostsim_lib, monkeypatch):
    """stacks deeper than the LDS part: the three-store push, the generic push at the boundary, the spill to memory and pops straight to the
    sentinel, through the plain kernel (RAYHIP_REFILL=0: walk_bvh4) and the persistent one (1, 2)"""
    want, tc_h, _, _ = host_strip(hostsim_lib, monkeypatch)
    assert tc_h["max_stack"] > LDS_STACK_DEPTH + 3, tc_h
    assert tc_h["max_stack"] < 2 * 48, tc_h  # (inside the whole stack: nothing is dropped)
    assert 0 < (want["v"] >= 0).sum() < len(want)
    rays, hits_in = strip_rays()
    for mode in ("0", "1", "2"):
        monkeypatch.setenv("RAYHIP_REFILL", mode)
        ctx = _context(gpu_lib, strip_blob())
        _, got, _ = ctx.k_intersect_closest(rays, hits_in, 1, flags=0)
        util.assert_hits_identical(got, want)
    monkeypatch.delenv("RAYHIP_REFILL")
    ctx = _context(gpu_lib, strip_blob())
    _, got, tc_g = ctx.k_intersect_closest(rays, hits_in, 1, flags=hip.FLAG_COUNT_WIDE)
    util.assert_hits_identical(got, want)
    assert (tc_g["nodes4"], tc_g["tris"]) == (tc_h["nodes4"], tc_h["tris"]), (tc_g, tc_h)
    assert tc_g["max_stack"] == tc_h["max_stack"]


def test_deep_stacks_shadow(gpu_lib, hostsim_lib, monkeypatch):
    """the same strip under the flat any-hit kernel and the nested one"""
    _, tc_h, want, tc_sh = host_strip(hostsim_lib, monkeypatch)
    assert tc_sh["max_stack"] > LDS_STACK_DEPTH + 3, tc_sh
    assert 0 < (want[:, :3].max(axis=-1) > 0).sum() < len(want)  # some rays are blocked, some arrive
    rays = strip_shadow_rays()
    monkeypatch.setenv("RAYHIP_HOOK_SHADOW_REFILL", "1")
    flat, _ = _context(gpu_lib, strip_blob()).k_intersect_shadow(rays, 1)
    monkeypatch.delenv("RAYHIP_HOOK_SHADOW_REFILL")
    assert flat[:, :3].tobytes() == want[:, :3].tobytes()
    nested, _ = _context(gpu_lib, strip_blob()).k_intersect_shadow(rays, 1)
    assert nested[:, :3].tobytes() == want[:, :3].tobytes()


RAGGED = (1, 63, 64, 65, 4097)


def _tiled(a, n):
    return np.tile(a, -(-n // len(a)))[:n].copy()


@pytest.mark.parametrize("name", ["cornell_instances", "cornell_principled"])
def test_ragged_launches_closest(gpu_lib, hostsim_lib, name, monkeypatch):
    """1, 63, 64, 65 and 4097 rays: wavefronts that start partly filled, lanes that are dead from the first iteration -- the exit conditions of
    the loop header -- over a top level with visibility masks (cornell_instances) and transparency rounds (cornell_principled)"""
    _host_env(monkeypatch)
    g = util.golden_ref(name)
    blob = util.golden_scene(name)
    n_max = max(RAGGED)
    rays, hits_in = _tiled(g["primary_rays"], n_max), _tiled(g["primary_hits_in"], n_max)
    host = _context(hostsim_lib, blob)
    got_rays_h, want, _ = host.k_intersect_closest(rays, hits_in, 1, flags=0)
    gpu = _context(gpu_lib, blob)
    for n in RAGGED:
        got_rays, got, _ = gpu.k_intersect_closest(rays[:n], hits_in[:n], 1, flags=0)
        util.assert_hits_identical(got, want[:n])
        assert got_rays.tobytes() == got_rays_h[:n].tobytes(), n  # (throughput and depth after transparent surfaces)


@pytest.mark.parametrize("name", ["cornell_instances", "cornell_principled"])
def test_ragged_launches_shadow(gpu_lib, hostsim_lib, name, monkeypatch):
    _host_env(monkeypatch)
    g = util.golden_ref(name)
    blob = util.golden_scene(name)
    rays = _tiled(g["shadow_rays"], max(RAGGED))
    want, _ = _context(hostsim_lib, blob).k_intersect_shadow(rays, 1)
    gpu = _context(gpu_lib, blob)
    monkeypatch.setenv("RAYHIP_HOOK_SHADOW_REFILL", "1")
    for n in RAGGED:
        got, _ = gpu.k_intersect_shadow(rays[:n], 1)
        assert got[:, :3].tobytes() == want[:n, :3].tobytes(), n
