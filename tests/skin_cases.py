"""Cases of skinning on the device (rayhip_skin_create / rayhip_scene_pose_skins; ray_amd/csrc/skin.h): seeded skins over the
committed fixture cornell_instances, seeded palettes, the host build of the element functions (tests/hostsim/hostsim_skin.cpp) and
an independent numpy restatement of what they compute.  Shared by tests/test_skinning_hostsim.py and tests/test_gpu_skinning.py.

The fixture has 128 vertices (the four of its triangle light are 20..23), so a skin here is at most 104 vertices long: one block of
the device kernel.  Launches of many blocks are held against the host build by tools/skin_bench.py on the scenes it times."""
import ctypes as C
import os

import numpy as np

import util
import vertex_update_cases as V
from ray_amd import hip

SKIN_LIB = os.path.join(util.ROOT, "tests", "hostsim", "_build", "libhostsim_skin.so")
SCENE = "cornell_instances"
BONES = (1, 3, 257)  # one bone, a few, and more than the device kernel keeps in LDS (skin.h: SKIN_LDS_BONES = 256)


class Skin:
    """rest pose and influences of vertices [first, first + count) of the scene `a`"""

    def __init__(self, a: V.Arrays, first, count, bones_count, seed):
        rng = np.random.RandomState(seed)
        self.first, self.count, self.bones_count = int(first), int(count), int(bones_count)
        self.rest = a.vertices[first:first + count].copy()
        self.indices = rng.randint(0, bones_count, size=(count, 4)).astype(np.uint16)
        # 1 to 4 influences with a weight, at random places among the four; the weights sum to 1 (as float32 sums do)
        w = rng.uniform(0.05, 1.0, size=(count, 4))
        for i in range(count):
            w[i, rng.permutation(4)[:rng.randint(0, 4)]] = 0.0  # (0 to 3 of them switched off)
        w /= w.sum(axis=1, keepdims=True)
        self.weights = w.astype(np.float32)
        self.unweighted = np.arange(count)[(np.arange(count) * 7 + seed) % 5 == 0] if count > 1 else np.zeros(0, dtype=np.int64)
        self.weights[self.unweighted] = 0.0  # ... and some vertices that no bone moves

    def influences(self):
        return (self.weights != 0).sum(axis=1)


def scene():
    blob = util.golden_scene(SCENE)
    return blob, V.Arrays(blob)


def extent(a: V.Arrays):
    p = a.vertices["p"][used_vertices(a)]
    return (p.max(axis=0) - p.min(axis=0)).astype(np.float32)


def used_vertices(a: V.Arrays):
    t = a.tri_indices[a.reachable_entries()].astype(np.int64)
    return np.unique(np.concatenate([a.vtx_indices[3 * t], a.vtx_indices[3 * t + 1], a.vtx_indices[3 * t + 2]]))


def free_ranges(a: V.Arrays):
    """(first, count) of the runs of the vertex array that hold no vertex of a triangle light, longest first"""
    lights = set(a.light_vertices())
    runs, start = [], None
    for i in range(len(a.vertices) + 1):
        free = i < len(a.vertices) and i not in lights
        if free and start is None:
            start = i
        if not free and start is not None:
            runs.append((start, i - start))
            start = None
    return sorted(runs, key=lambda r: -r[1])


def seeded_skins(a: V.Arrays, bones_count, seed=3):
    """the skins the tests pose: [0] starts at vertex 1 and has a length that is no multiple of 64 -- it ends where the light's vertices
    begin; [1], disjoint from it, runs from behind the light's vertices to the end of the array; [2] is a single vertex of [1]'s range
    (an alternative to [1], not to be alive next to it)"""
    lights = a.light_vertices()
    first_light, last_light = min(lights), max(lights)
    assert first_light > 2 and (first_light - 1) % 64 != 0 and last_light + 2 < len(a.vertices)
    tail = last_light + 1
    return [Skin(a, 1, first_light - 1, bones_count, seed), Skin(a, tail, len(a.vertices) - tail, bones_count, seed + 1),
            Skin(a, tail + 5, 1, bones_count, seed + 2)]


def exact_identity_skin(a: V.Arrays, skin: Skin):
    """`skin` with one influence of weight 1 per vertex -- and none for the vertices whose identity pose would not be the rest record
    bytewise (a normal or bitangent that is not of unit length is normalised, a -0.0 becomes +0.0): such a vertex keeps its record by
    the all-weights-zero rule.  Posed with identity matrices, this skin reproduces the bytes of its rest pose."""
    out = Skin(a, skin.first, skin.count, skin.bones_count, 0)
    out.indices = skin.indices.copy()
    out.weights = np.zeros_like(skin.weights)
    out.weights[:, 1] = 1.0
    same = (bits(numpy_skin(out.rest, out.indices, out.weights, identity_palette(out.bones_count))) == bits(out.rest)).all(axis=1)
    out.weights[~same] = 0.0
    out.unweighted = np.arange(out.count)[~same]
    return out


def palette(bones_count, seed, ext):
    """[bones][3][4] float32: rotations by up to 0.15 rad about random axes, translations within 5 % of the scene's extent `ext`"""
    rng = np.random.RandomState(seed)
    axis = rng.normal(size=(bones_count, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    angle = rng.uniform(-0.15, 0.15, size=bones_count)
    K = np.zeros((bones_count, 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -axis[:, 2], axis[:, 1], axis[:, 2], -axis[:, 0], -axis[:, 1], axis[:, 0]
    R = np.eye(3)[None] + np.sin(angle)[:, None, None] * K + (1.0 - np.cos(angle))[:, None, None] * (K @ K)
    out = np.zeros((bones_count, 3, 4), dtype=np.float32)
    out[:, :, :3] = R
    out[:, :, 3] = rng.uniform(-0.05, 0.05, size=(bones_count, 3)) * ext
    return out


def identity_palette(bones_count):
    out = np.zeros((bones_count, 3, 4), dtype=np.float32)
    out[:, 0, 0] = out[:, 1, 1] = out[:, 2, 2] = 1.0
    return out


# ---- the host build -------------------------------------------------------------------------------------------------------------
def have_skin_lib():
    return os.path.exists(SKIN_LIB)


_lib = None


def skin_lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(SKIN_LIB)
        vp, u32 = C.c_void_p, C.c_uint32
        _lib.hostsim_skin_vertices.argtypes = [vp, vp, vp, u32, vp, u32, vp, vp, C.POINTER(u32)]
        _lib.hostsim_check_vertices.argtypes = [vp, u32, u32, vp, vp, vp, u32, vp]
        _lib.hostsim_skin_lds_bones.restype = u32
    return _lib


def host_skin(rest, indices, weights, bones, used=None):
    """(posed VERTEX_DTYPE records, used vertices whose posed position is not finite) by tests/hostsim/hostsim_skin.cpp"""
    rest, indices, weights = np.ascontiguousarray(rest), np.ascontiguousarray(indices, dtype=np.uint16), np.ascontiguousarray(weights, dtype=np.float32)
    bones = np.ascontiguousarray(bones, dtype=np.float32)
    assert rest.dtype == hip.VERTEX_DTYPE and indices.shape == (len(rest), 4) and weights.shape == (len(rest), 4) and bones.shape[1:] == (3, 4)
    used = None if used is None else np.ascontiguousarray(used, dtype=np.uint8)
    out = np.zeros(len(rest), dtype=hip.VERTEX_DTYPE)
    bad = C.c_uint32(0)
    rc = skin_lib().hostsim_skin_vertices(rest.ctypes.data, indices.ctypes.data, weights.ctypes.data, len(rest), bones.ctypes.data, len(bones),
                                          None if used is None else used.ctypes.data, out.ctypes.data, C.byref(bad))
    assert rc == 0, rc
    return out, int(bad.value)


def host_posed(a: V.Arrays, skins, palettes, vertices=None):
    """the scene's vertex array with every skin posed by its palette (the host build); everything else as it was"""
    v = (a.vertices if vertices is None else vertices).copy()
    for s, m in zip(skins, palettes):
        v[s.first:s.first + s.count], bad = host_skin(s.rest, s.indices, s.weights, m)
        assert bad == 0
    return v


def moved_blob(blob, a: V.Arrays, vertices, slot, delta):
    """the scene with instance `slot` translated by `delta` in world space, as rayhip_scene_update_instances wants it: the instance
    array with the new transform and its inverse, and the leaves of the top level with the world-space boxes of the instances under
    `vertices` (an instance update takes the boxes the host's top level holds; tests/hostsim/hostsim_refit.cpp computes them here)"""
    mi = a.mesh_instances.copy()
    m = mi["xform"][slot].astype(np.float64).reshape(4, 4)
    m[3, :3] += np.asarray(delta, dtype=np.float64)
    mi["xform"][slot] = m.ravel().astype(np.float32)
    mi["inv_xform"][slot] = np.linalg.inv(m).ravel().astype(np.float32)
    _, refitted, _ = V.host_refit(a, vertices)
    slots = a.live_instances()
    boxes = V.instance_boxes(refitted, mi, slots)
    nodes = a.nodes.copy()
    f = nodes.view(np.float32)
    stack, seen = [a.tlas_root], 0
    while stack:
        w = stack.pop()
        for k, link in enumerate(a.nodes[w, 12:14]):
            if not link & V.COUNT_BITS:
                stack.append(int(link))
                continue
            b = boxes[slots.index(int(link & V.INDEX_BITS))]
            f[w, [0, 2, 8, 1, 3, 9] if k == 0 else [4, 6, 10, 5, 7, 11]] = b  # (vertex_update_cases.child_box: lo.xyz, hi.xyz)
            seen += 1
    assert seen == len(slots)
    return V.patched_blob(blob, mesh_instances=mi, nodes=nodes)


# ---- numpy restatement: float32, one rounding per operation, the order of skin.h written out ---------------------------------------
def _blend(v, idx, w, bones, translate):
    """([n][3] blended vectors, [n] some influence has a weight): influences 0..3 in order, those of weight 0 skipped"""
    f = np.float32
    n = len(v)
    acc = np.zeros((n, 3), dtype=f)
    started = np.zeros(n, dtype=bool)
    for k in range(4):
        use = w[:, k] != 0
        m = bones[idx[:, k].astype(np.int64)]  # [n][3][4]
        for i in range(3):
            t = (m[:, i, 0] * v[:, 0] + m[:, i, 1] * v[:, 1]) + m[:, i, 2] * v[:, 2]
            if translate:
                t = t + m[:, i, 3]
            wt = w[:, k] * t
            assert t.dtype == f and wt.dtype == f
            acc[:, i] = np.where(use, np.where(started, acc[:, i] + wt, wt), acc[:, i])
        started |= use
    return acc, started


def _normalised_or_rest(v, rest):
    f = np.float32
    dot = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    ok = (dot != 0) & np.isfinite(dot)
    length = np.sqrt(np.where(ok, dot, f(1.0)))
    assert dot.dtype == f and length.dtype == f
    return np.where(ok[:, None], v / length[:, None], rest)


def numpy_skin(rest, indices, weights, bones):
    """posed VERTEX_DTYPE records: linear-blend skinning as ray_amd/csrc/skin.h states it"""
    f = np.float32
    bones, weights = np.asarray(bones, dtype=f), np.asarray(weights, dtype=f)
    out = rest.copy()
    with np.errstate(all="ignore"):
        p, moved = _blend(rest["p"], indices, weights, bones, True)
        n, _ = _blend(rest["n"], indices, weights, bones, False)
        b, _ = _blend(rest["b"], indices, weights, bones, False)
        n, b = _normalised_or_rest(n, rest["n"]), _normalised_or_rest(b, rest["b"])
    out["p"][moved], out["n"][moved], out["b"][moved] = p[moved], n[moved], b[moved]
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype != hip.VERTEX_DTYPE else a.view(np.uint32).reshape(-1, 11)
