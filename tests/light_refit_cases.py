"""Cases of the light refit (rayhip_scene_refit_lights; ray_amd/csrc/light_refit.h): scenes whose emitters deform, the light arrays of
a serialised scene, the host build of the refit (tests/hostsim/hostsim_lights.cpp), a crafted two-level tree written directly as
arrays, and an independent float64 restatement of what a refit computes.  Shared by tests/test_light_refit_hostsim.py and
tests/test_gpu_light_refit.py."""
import ctypes as C
import os

import numpy as np

import util
import vertex_update_cases as V
from ray_amd import hip, scenes
from ray_amd.api import ShadingNode, eShadingNode

LIGHTS_LIB = os.path.join(util.ROOT, "tests", "hostsim", "_build", "libhostsim_lights.so")
EMPTY, LEAF_BIT, INDEX_BITS = 0x7fffffff, 0x80000000, 0x7fffffff
MAX_DIST = np.float32(3.402823466e+30)
TYPE_SPHERE, TYPE_DIR, TYPE_RECT, TYPE_TRI = 0, 1, 3, 5
NODE = hip.LIGHT_NODE_DTYPE
SUMMARY = np.dtype([("lo", "<f4", 3), ("hi", "<f4", 3), ("flux", "<f4"), ("axis", "<f4", 3), ("omega_n", "<f4"), ("omega_e", "<f4")])
assert SUMMARY.itemsize == 48


def bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype == hip.VERTEX_DTYPE:
        return a.view(np.uint32).reshape(-1, 11)
    if a.dtype == NODE:
        return a.view(np.uint32).reshape(-1, 52)
    return a.view(np.uint32)


# ---- scenes -----------------------------------------------------------------------------------------------------------------
def one_emitter(scene, phase=0.0):
    """a Cornell room without its lamp whose only light is ONE emissive triangle, axis-aligned (in a plane of constant y): the root of
    the light tree has a single leaf, and the node box has no extent on one axis.  `phase` slides and stretches the triangle in its plane."""
    scene.SetEnvironment(env_col=(0.0, 0.0, 0.0))
    grey = scene.AddMaterial(ShadingNode(type=eShadingNode.Diffuse, base_color=(0.5, 0.5, 0.5)))
    red = scene.AddMaterial(ShadingNode(type=eShadingNode.Diffuse, base_color=(0.5, 0.0, 0.0)))
    green = scene.AddMaterial(ShadingNode(type=eShadingNode.Diffuse, base_color=(0.0, 0.5, 0.0)))
    emit = scene.AddMaterial(ShadingNode(type=eShadingNode.Emissive, strength=60.0, importance_sample=True))
    attrs, idx = scenes.cornell_mesh_arrays(scenes._CORNELL_QUADS)
    scene.AddMeshInstance(scene.AddMesh(attrs, idx, [(grey, None, 0, 18), (red, None, 18, 6), (green, None, 24, 6), (grey, None, 30, 6)]))
    s = 0.03 * float(phase)
    tri = np.array([[-0.36 + s, 0.5, -0.36, 0, -1, 0, 0, 0], [-0.36 + s, 0.5, -0.20 + s, 0, -1, 0, 0, 1], [-0.20 + 2 * s, 0.5, -0.36, 0, -1, 0, 1, 0]],
                   dtype=np.float32)
    scene.AddMeshInstance(scene.AddMesh(tri, np.arange(3, dtype=np.uint32), [(emit, 0xFFFFFFFF, 0, 3)]))
    scenes._cornell_camera(scene)
    scene.Finalize()


def emissive_sheet(scene, phase, moved=False):
    """the room of vertex_update_cases (its lamp: two triangle lights) plus an EMISSIVE sheet of 12 x 12 quads (288 triangle lights) as
    a mesh of its own, instanced twice under rotation and non-uniform scale (576 triangle lights), plus a sphere, a rect and a
    directional light (an infinite child of the tree).  `moved`: the second instance somewhere else."""
    scene.SetEnvironment(env_col=(0.0, 0.0, 0.0))
    V._room(scene)
    glow = scene.AddMaterial(ShadingNode(type=eShadingNode.Emissive, strength=4.0, base_color=(0.9, 0.7, 0.4), importance_sample=True))
    b = scenes._MeshBuilder()
    b.add(*V._sheet_mesh(12, phase, -0.10, 0.10, -0.10, 0.10, 0.0, 0.03, seed=21), glow)
    attrs, idx, groups = b.finish()
    mesh = scene.AddMesh(attrs, idx, groups, **V._SHEET_LAYOUT)
    scene.AddMeshInstance(mesh, scenes._xform(translate=(-0.38, 0.16, -0.36), rot_y_deg=20.0, rot_z_deg=10.0, scale=(1.3, 0.7, 0.9)))
    second = (-0.18, 0.30, -0.22) if not moved else (-0.22, 0.36, -0.28)
    scene.AddMeshInstance(mesh, scenes._xform(translate=second, rot_y_deg=-35.0, rot_z_deg=-25.0, scale=(0.8, 1.5, 1.2)))
    scene.AddLight("sphere", color=(3.0, 2.5, 2.0), position=(-0.12, 0.42, -0.12), radius=0.02)
    scene.AddLight("rect", color=(4.0, 4.0, 3.5), width=0.12, height=0.08, xform=scenes._translate(-0.30, 0.52, -0.44))
    scene.AddLight("directional", color=(0.4, 0.4, 0.5), direction=(0.25, -0.45, -1.0), angle=4.0)
    scenes._cornell_camera(scene)
    scene.Finalize()


SCENES = {"one_emitter": one_emitter, "emissive_sheet": emissive_sheet}
_blobs = {}


def scene_blob(name, phase, **kw):
    """the serialised scene `name` at `phase`, built once per process (needs the host library of the drop-in); "fixture": the
    committed cornell_instances, which has no phases"""
    if name == "fixture":
        return util.golden_scene("cornell_instances")
    from ray_amd import api
    key = (name, phase, tuple(sorted(kw.items())))
    if key not in _blobs:
        s = api.CreateSceneHIP()
        SCENES[name](s, float(phase), **kw)
        _blobs[key] = api.export_scene_blob(s)
    return _blobs[key]


class Arrays(V.Arrays):
    """... and the light arrays"""

    def __init__(self, blob):
        super().__init__(blob)
        off, size = V.sections(blob)["light_cwnodes"]
        self.cwnodes = np.frombuffer(blob, dtype=NODE, count=size // NODE.itemsize, offset=off).copy()

    def light_types(self):
        return (self.lights[:, 0] & 7).astype(np.int64)

    def tri_lights(self):
        """light slots li_indices names that hold triangle lights"""
        return np.array([int(i) for i in self.li_indices if self.lights[i, 0] & 7 == TYPE_TRI], dtype=np.int64)

    def tri_light_corners(self, vertices, instances=None):
        """{light slot: [3][3] float64 world corners} by the transform of its instance"""
        mi_all = self.mesh_instances if instances is None else instances
        out = {}
        for i in self.tri_lights():
            tri, mi = int(self.lights[i, 4]), int(self.lights[i, 5])
            m = mi_all["xform"][mi].astype(np.float64).reshape(4, 4)  # (column vectors: element 4 c + r)
            p = vertices["p"][self.vtx_indices[3 * tri:3 * tri + 3]].astype(np.float64)
            out[int(i)] = p @ m[:3, :3] + m[3, :3]
        return out


def moved_vertices(a: Arrays, seed=9, fraction=0.02):
    """every position moved by up to +-`fraction` of the scene's extent (seeded) -- those of the triangle lights too"""
    v = a.vertices.copy()
    t = a.tri_indices[a.reachable_entries()].astype(np.int64)
    used = np.unique(np.concatenate([a.vtx_indices[3 * t], a.vtx_indices[3 * t + 1], a.vtx_indices[3 * t + 2]]))
    ext = (v["p"][used].max(axis=0) - v["p"][used].min(axis=0)).astype(np.float32)
    v["p"] = v["p"] + np.random.RandomState(seed).uniform(-fraction, fraction, size=v["p"].shape).astype(np.float32) * ext
    return v


def twin_blob(blob, a: Arrays, vertices):
    """the scene `blob` with `vertices` and everything its host arrays derive from them: triangle records, bottom-level boxes
    (tests/hostsim/hostsim_refit.cpp) and the boxes of the top level, leaves and inner nodes -- a scene a fresh upload takes"""
    recs, nodes, _ = V.host_refit(a, vertices)
    f = nodes.view(np.float32)
    slots = a.live_instances()
    boxes = V.instance_boxes(nodes, a.mesh_instances, slots)

    def refit(w):
        out = []
        for k, link in enumerate(a.nodes[w, 12:14]):
            b = boxes[slots.index(int(link & V.INDEX_BITS))] if link & V.COUNT_BITS else refit(int(link))
            f[w, [0, 2, 8, 1, 3, 9] if k == 0 else [4, 6, 10, 5, 7, 11]] = b
            out.append(b)
        return np.concatenate([np.minimum(out[0][:3], out[1][:3]), np.maximum(out[0][3:], out[1][3:])])

    if a.tlas_root != 0xffffffff:
        refit(a.tlas_root)
    return V.patched_blob(blob, vertices=vertices, tris=recs, nodes=nodes)


def with_section(blob, name, array):
    """`blob` with the section `name` replaced by `array`, of whatever size: the new bytes go behind the old ones (16-byte aligned)
    and the section table points at them -- a scene built at another pose may have a light tree of another node count"""
    import struct
    raw = np.ascontiguousarray(array).tobytes()
    b = bytearray(blob) + bytes(-len(blob) % 16)
    count = struct.unpack_from("<I", b, 8)[0]
    for i in range(count):
        at = V.HEADER + i * V.SECTION
        if struct.unpack_from("<24s", b, at)[0].rstrip(b"\0").decode() == name:
            struct.pack_into("<QQ", b, at + 24, len(b), len(raw))
            return bytes(b + raw)
    raise KeyError(name)


# ---- the host build ---------------------------------------------------------------------------------------------------------------
def have_lights_lib():
    return os.path.exists(LIGHTS_LIB)


_lib = None


def lights_lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(LIGHTS_LIB)
        vp, u32 = C.c_void_p, C.c_uint32
        _lib.hostsim_light_leaf_table.argtypes = [vp, u32, vp, u32, vp]
        _lib.hostsim_refit_tri_lights.argtypes = [vp, u32, vp, u32, vp, u32, vp, u32, vp, u32, vp, vp, C.POINTER(u32)]
        _lib.hostsim_refit_light_nodes.argtypes = [vp, u32, vp, u32, vp, vp, vp, vp]
        _lib.hostsim_light_slot_scales.argtypes = [vp, u32, vp, u32, vp, u32, vp, u32, vp, u32, vp, u32, vp]
        _lib.hostsim_light_levels.argtypes = [vp, u32, u32, vp, vp, u32, C.POINTER(u32)]
        _lib.hostsim_fill_light_children.argtypes = [vp, u32, vp]
        _lib.hostsim_fill_light_tri_geom.argtypes = [vp, u32, vp, u32, vp, vp, vp, vp]
        _lib.hostsim_light_child_boxes.argtypes = [vp, u32, vp]
        _lib.hostsim_light_importances.argtypes = [vp, vp, vp]
    return _lib


def _c(x, dtype=None):
    return np.ascontiguousarray(x) if dtype is None else np.ascontiguousarray(x, dtype=dtype)


def leaf_table(lights, cwnodes):
    lights, cwnodes = _c(lights, np.uint32), _c(cwnodes)
    out = np.zeros(len(lights), dtype=SUMMARY)
    assert lights_lib().hostsim_light_leaf_table(lights.ctypes.data, len(lights), cwnodes.ctypes.data, len(cwnodes), out.ctypes.data) == 0
    return out


def fill_children(cwnodes):
    cwnodes = _c(cwnodes)
    out = np.zeros((len(cwnodes), 26, 4), dtype=np.float32)
    assert lights_lib().hostsim_fill_light_children(cwnodes.ctypes.data, len(cwnodes), out.ctypes.data) == 0
    return out


def fill_tri_geom(a: Arrays, vertices, instances=None):
    lights, li, mi = _c(a.lights, np.uint32), _c(a.li_indices, np.uint32), _c(a.mesh_instances if instances is None else instances)
    vi, v = _c(a.vtx_indices, np.uint32), _c(vertices)
    out = np.zeros((len(lights), 4, 4), dtype=np.float32)
    assert lights_lib().hostsim_fill_light_tri_geom(lights.ctypes.data, len(lights), li.ctypes.data, len(li), mi.ctypes.data, vi.ctypes.data, v.ctypes.data,
                                                    out.ctypes.data) == 0
    return out


def child_boxes(cwnodes):
    """[n][8][6] float32 (lo, hi): the decoded boxes of the children (shade_lights.h: light_child_box)"""
    cwnodes = _c(cwnodes)
    out = np.zeros((len(cwnodes), 8, 6), dtype=np.float32)
    assert lights_lib().hostsim_light_child_boxes(cwnodes.ctypes.data, len(cwnodes), out.ctypes.data) == 0
    return out


def importances(node, P):
    node, P = _c(node), _c(P, np.float32)
    out = np.zeros(8, dtype=np.float32)
    assert lights_lib().hostsim_light_importances(node.ctypes.data, P.ctypes.data, out.ctypes.data) == 0
    return out


def levels(cwnodes, n_lights):
    """(level_nodes, level_offset): the nodes sorted by height"""
    cwnodes = _c(cwnodes)
    ln, lo, n = np.zeros(len(cwnodes), dtype=np.uint32), np.zeros(80, dtype=np.uint32), C.c_uint32(0)
    rc = lights_lib().hostsim_light_levels(cwnodes.ctypes.data, len(cwnodes), n_lights, ln.ctypes.data, lo.ctypes.data, len(lo), C.byref(n))
    assert rc == 0, rc
    return ln, lo[:n.value + 1]


class Refitted:
    pass


def slot_scales(lights, li_indices, mesh_instances, vtx_indices, vertices, cwnodes):
    """[n][8] float32: what an upload prepares of the tree `cwnodes` and the pose it was built at -- per inner slot the stored flux over
    the summed flux below it (light_refit.h: slot_scales)"""
    lights, li, mi = _c(lights, np.uint32), _c(li_indices, np.uint32), _c(mesh_instances)
    vi, v, cwnodes = _c(vtx_indices, np.uint32), _c(vertices), _c(cwnodes)
    out = np.ones((len(cwnodes), 8), dtype=np.float32)
    rc = lights_lib().hostsim_light_slot_scales(lights.ctypes.data, len(lights), li.ctypes.data, len(li), mi.ctypes.data, len(mi), vi.ctypes.data, len(vi),
                                                v.ctypes.data, len(v), cwnodes.ctypes.data, len(cwnodes), out.ctypes.data)
    assert rc == 0, rc
    return out


def host_refit_arrays(lights, li_indices, mesh_instances, vtx_indices, vertices, cwnodes, children=None, tri_geom=None, scales=None):
    """the light arrays after a refit under `vertices`, by tests/hostsim/hostsim_lights.cpp.  `cwnodes` / `children` / `tri_geom`: what a
    device held before (default: what an upload makes of `cwnodes`; no corners).  `scales`: slot_scales of the upload (None: 1)."""
    lights, li, mi = _c(lights, np.uint32), _c(li_indices, np.uint32), _c(mesh_instances)
    vi, v = _c(vtx_indices, np.uint32), _c(vertices)
    r = Refitted()
    r.cwnodes = _c(cwnodes).copy()
    r.children = fill_children(cwnodes) if children is None else _c(children, np.float32).copy()
    r.tri_geom = np.zeros((len(lights), 4, 4), dtype=np.float32) if tri_geom is None else _c(tri_geom, np.float32).copy()
    r.leaf = leaf_table(lights, cwnodes)
    r.node_summary = np.zeros(len(r.cwnodes), dtype=SUMMARY)
    r.scales = None if scales is None else _c(scales, np.float32)
    n = C.c_uint32(0)
    L = lights_lib()
    assert L.hostsim_refit_tri_lights(lights.ctypes.data, len(lights), li.ctypes.data, len(li), mi.ctypes.data, len(mi), vi.ctypes.data, len(vi), v.ctypes.data,
                                      len(v), r.tri_geom.ctypes.data, r.leaf.ctypes.data, C.byref(n)) == 0
    r.degenerate = int(n.value)
    rc = L.hostsim_refit_light_nodes(r.cwnodes.ctypes.data, len(r.cwnodes), lights.ctypes.data, len(lights), r.leaf.ctypes.data, r.node_summary.ctypes.data,
                                     r.children.ctypes.data, None if r.scales is None else r.scales.ctypes.data)
    assert rc == 0, rc
    return r


def host_refit(a: Arrays, vertices, cwnodes=None, children=None, tri_geom=None, instances=None):
    """... of the scene `a`, as a context does it that uploaded `a` (or, with `instances`, got them by an instance update of `a`'s own
    tree and vertices): the scales are those of a.cwnodes at a.vertices"""
    mi = a.mesh_instances if instances is None else instances
    scales = slot_scales(a.lights, a.li_indices, mi, a.vtx_indices, a.vertices, a.cwnodes)
    return host_refit_arrays(a.lights, a.li_indices, mi, a.vtx_indices, vertices, a.cwnodes if cwnodes is None else cwnodes, children, tri_geom, scales)


# ---- walking a tree ----------------------------------------------------------------------------------------------------------------
def lights_below(cwnodes, link):
    """light slots below the child link `link`"""
    if link & LEAF_BIT:
        return [int(link & INDEX_BITS)]
    out = []
    for c in cwnodes["child"][int(link)]:
        if c != EMPTY:
            out += lights_below(cwnodes, int(c))
    return out


def paths(cwnodes):
    """{light slot: [(node, slot), ...] from the root down to the leaf slot that names it}"""
    out = {}

    def walk(w, trail):
        for i, c in enumerate(cwnodes["child"][w]):
            if c == EMPTY:
                continue
            if c & LEAF_BIT:
                out[int(c & INDEX_BITS)] = trail + [(w, i)]
            else:
                walk(int(c), trail + [(w, i)])

    if len(cwnodes):
        walk(0, [])
    return out


def decode_axis(word):
    """[..., 3] float64 unit axes of octahedral words (shade_lights.h: decode_light_child)"""
    word = np.asarray(word, dtype=np.uint32)
    x = -1.0 + 2.0 * ((word >> 16) & 0xffff).astype(np.float64) / 65535.0
    y = -1.0 + 2.0 * (word & 0xffff).astype(np.float64) / 65535.0
    z = 1.0 - np.abs(x) - np.abs(y)
    fold = z < 0
    x, y = np.where(fold, (1.0 - np.abs(y)) * np.copysign(1.0, x), x), np.where(fold, (1.0 - np.abs(x)) * np.copysign(1.0, y), y)
    d = np.stack([x, y, z], axis=-1)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def decode_cosines(word):
    word = np.asarray(word, dtype=np.uint32)
    return np.stack([2.0 * (((word >> 16) & 0xffff) / 65534.0) - 1.0, 2.0 * ((word & 0xffff) / 65534.0) - 1.0], axis=-1)


# ---- a crafted tree, written directly as arrays --------------------------------------------------------------------------------------
class Crafted:
    """Two levels.  Root (node 0): slot 0 -> node 1, slot 1 EMPTY (a hole in the middle), slot 2 -> the sphere light (slot 4 of the
    light array), slot 3 -> node 2, slot 5 -> the directional light (an infinite child).  Node 1: triangle lights 0, 1 and, behind an
    empty slot, 2 -- which has NO AREA (two corners coincide).  Node 2: the directional light 5 alone and an env-like second infinite
    leaf: a subtree without a finite child.  One identity instance; the light array is a pool of 7 slots of which slot 3 is free."""

    def __init__(self):
        f = np.float32
        P = np.array([[0.1, 0.2, 0.3], [0.6, 0.25, 0.3], [0.2, 0.7, 0.45],   # light 0
                      [-0.4, 0.1, -0.2], [-0.1, 0.15, -0.6], [-0.3, 0.5, -0.3],  # light 1
                      [0.8, 0.8, 0.8], [0.8, 0.8, 0.8], [0.9, 0.7, 0.6]], dtype=f)  # light 2: no area
        self.vertices = np.zeros(len(P), dtype=hip.VERTEX_DTYPE)
        self.vertices["p"], self.vertices["n"], self.vertices["b"] = P, (0, 1, 0), (1, 0, 0)
        self.vertices["t"] = np.random.RandomState(3).uniform(0, 1, size=(len(P), 2)).astype(f)
        self.vtx_indices = np.arange(9, dtype=np.uint32)
        self.mesh_instances = np.zeros(1, dtype=V.MESH_INSTANCE_DTYPE)
        self.mesh_instances["xform"][0] = self.mesh_instances["inv_xform"][0] = np.eye(4, dtype=f).ravel()
        lights = np.zeros((7, 16), dtype=np.uint32)
        lf = lights.view(f)
        for k, (col, doublesided) in enumerate([((3.0, 2.0, 1.0), 0), ((0.5, 4.0, 0.25), 1), ((9.0, 9.0, 9.0), 0)]):
            lights[k, 0] = TYPE_TRI | (doublesided << 3) | (1 << 5)
            lf[k, 1:4] = col
            lights[k, 4], lights[k, 5] = k, 0  # params[0] the triangle, params[1] the instance
        lights[4, 0] = TYPE_SPHERE | (1 << 5)
        lf[4, 1:4], lf[4, 4:7], lf[4, 7], lf[4, 11] = (2.0, 2.0, 2.0), (0.3, -0.5, 0.1), 0.0314, 0.05  # col, pos, area, radius
        lights[5, 0] = TYPE_DIR
        lf[5, 1:4], lf[5, 4:7], lf[5, 9] = (1.0, 1.0, 1.0), (0.0, -0.6, -0.8), 0.05  # col, dir, angle
        lights[6, 0] = TYPE_DIR
        lf[6, 1:4], lf[6, 4:7], lf[6, 9] = (0.5, 0.5, 0.5), (0.6, -0.8, 0.0), 0.02
        self.lights, self.li_indices = lights, np.array([0, 1, 2, 4, 5, 6], dtype=np.uint32)
        n = np.zeros(3, dtype=NODE)
        n["child"][:] = EMPTY
        n["ch_bbox_min"][:], n["ch_bbox_max"][:] = 0xff, 0xff  # (an empty slot as the scene build leaves it)
        n["child"][0, [0, 2, 3, 5]] = 1, LEAF_BIT | 4, 2, LEAF_BIT | 5
        n["child"][1, [0, 1, 3]] = LEAF_BIT | 0, LEAF_BIT | 1, LEAF_BIT | 2
        n["child"][2, [0, 4]] = LEAF_BIT | 5, LEAF_BIT | 6
        # what only an upload knows: the fluxes, axes and cosines of the lights that are no triangles; boxes that mean nothing yet
        n["bbox_min"][:], n["bbox_max"][:] = (-7.0, -7.0, -7.0), (7.0, 7.0, 7.0)
        for w, i, flux, axis, cosines in [(0, 2, 0.1884, 0x7fffffff, 0x00007fff), (0, 5, 3.0, 0x4000b000, 0xfffeffbc), (2, 0, 3.0, 0x4000b000, 0xfffeffbc),
                                          (2, 4, 1.5, 0xc0005000, 0xfffefff0)]:
            n["flux"][w, i], n["axis"][w, i], n["cos_omega_ne"][w, i] = flux, axis, cosines
        n["flux"][0, 0] = 0.25  # (the inner slot over node 1 stores less than the sum below it; the one over node 2 stores nothing: scale 1)
        # the hole in the middle of the root carries bytes of its own: a refit must not touch them
        n["ch_bbox_min"][0, :, 1], n["ch_bbox_max"][0, :, 1] = (1, 2, 3), (4, 5, 6)
        n["flux"][0, 1], n["axis"][0, 1], n["cos_omega_ne"][0, 1] = 123.0, 0xdeadbeef, 0x12345678
        self.cwnodes = n

    def refit(self, vertices=None):
        scales = slot_scales(self.lights, self.li_indices, self.mesh_instances, self.vtx_indices, self.vertices, self.cwnodes)
        return host_refit_arrays(self.lights, self.li_indices, self.mesh_instances, self.vtx_indices, self.vertices if vertices is None else vertices,
                                 self.cwnodes, scales=scales)


# ---- float64 restatement -------------------------------------------------------------------------------------------------------------
def _static_summary64(l_words):
    """(lo, hi, axis, omega_n, omega_e) of a light that is no triangle, in float64 from its float32 record"""
    p = l_words.view(np.float32).astype(np.float64)[4:]
    kind, doublesided = int(l_words[0] & 7), bool((l_words[0] >> 3) & 1)
    inf = np.full(3, float(MAX_DIST))
    up = np.array([0.0, 1.0, 0.0])
    if kind == TYPE_SPHERE:
        return p[0:3] - p[7], p[0:3] + p[7], up, np.pi, np.pi / 2
    if kind == TYPE_DIR:
        return -inf, inf, p[0:3], 0.0, p[5]
    if kind == 2:  # line
        u, d = p[4:7], p[8:11]
        v = np.cross(u, d) * p[7]
        u, d = u * p[7], d * (0.5 * p[11])
        c = np.array([p[0:3] + sd * d + su * u + sv * v for sd in (1, -1) for su in (1, -1) for sv in (1, -1)])
        return c.min(axis=0), c.max(axis=0), up, np.pi, np.pi / 2
    if kind in (TYPE_RECT, 4):
        u, v = 0.5 * p[4:7], 0.5 * p[8:11]
        c = np.array([p[0:3] + su * u + sv * v for su in (1, -1) for sv in (1, -1)])
        n = np.cross(u, v)
        return c.min(axis=0), c.max(axis=0), n / np.linalg.norm(n), np.pi if doublesided else 0.0, np.pi / 2
    return -inf, inf, up, np.pi, np.pi / 2  # environment


def model64(lights, li_indices, mesh_instances, vtx_indices, vertices, cwnodes):
    """What section 3 of the refit asks for, restated in float64 over the float32 inputs: {light slot: summary} for the leaves and
    {node: summary}, a summary being a dict(lo, hi, flux, axis, omega_n, omega_e, finite).  Fluxes of lights that are no triangles
    come from the slot that names them, as on the device."""
    lights = np.ascontiguousarray(lights, dtype=np.uint32)
    leaf, node = {}, {}
    for w in range(len(cwnodes)):
        for i, c in enumerate(cwnodes["child"][w]):
            if c != EMPTY and c & LEAF_BIT and lights[int(c & INDEX_BITS), 0] & 7 != TYPE_TRI:
                lo, hi, axis, on, oe = _static_summary64(lights[int(c & INDEX_BITS)])
                leaf[int(c & INDEX_BITS)] = dict(lo=lo, hi=hi, flux=float(cwnodes["flux"][w, i]), axis=axis, omega_n=on, omega_e=oe, finite=lo[0] > -float(MAX_DIST))
    for i in li_indices:
        l = lights[int(i)]
        if l[0] & 7 != TYPE_TRI:
            continue
        m = mesh_instances["xform"][int(l[5])].astype(np.float64).reshape(4, 4)
        p = vertices["p"][vtx_indices[3 * int(l[4]):3 * int(l[4]) + 3]].astype(np.float64) @ m[:3, :3] + m[3, :3]
        n = np.cross(p[1] - p[0], p[2] - p[0])
        length = np.linalg.norm(n)
        col = l.view(np.float32)[1:4].astype(np.float64)
        s = dict(lo=p.min(axis=0), hi=p.max(axis=0), omega_n=np.pi if (l[0] >> 3) & 1 else 0.0, omega_e=np.pi / 2, finite=True)
        if length > 0:
            s.update(flux=col.sum() * 0.5 * length, axis=n / length)
        else:
            s.update(flux=0.0, axis=np.array([0.0, 1.0, 0.0]))
        leaf[int(i)] = s

    def summary(w):
        if w in node:
            return node[w]
        own = None
        lo, hi, finite = np.full(3, np.inf), np.full(3, -np.inf), False
        for c in cwnodes["child"][w]:  # slot order
            if c == EMPTY:
                continue
            s = leaf[int(c & INDEX_BITS)] if c & LEAF_BIT else summary(int(c))
            if s["finite"]:
                lo, hi, finite = np.minimum(lo, s["lo"]), np.maximum(hi, s["hi"]), True
            if own is None:
                own = dict(flux=s["flux"], axis=s["axis"].copy(), omega_n=s["omega_n"], omega_e=s["omega_e"])
                continue
            own["flux"] += s["flux"]
            angle = np.arccos(np.clip(np.dot(own["axis"], s["axis"]), -1.0, 1.0))
            total = own["axis"] + s["axis"]
            length = np.linalg.norm(total)
            own["axis"] = total / length if length != 0 else np.array([0.0, 1.0, 0.0])
            own["omega_n"] = min(0.5 * (own["omega_n"] + max(own["omega_n"], angle + s["omega_n"])), np.pi)
            own["omega_e"] = max(own["omega_e"], s["omega_e"])
        own.update(lo=lo, hi=hi, finite=finite)
        node[w] = own
        return own

    for w in range(len(cwnodes)):
        summary(w)
    return leaf, node


def model64_slot(cwnodes, leaf, node, w, i):
    """the summary slot i of node w refers to"""
    c = int(cwnodes["child"][w, i])
    return leaf[c & INDEX_BITS] if c & LEAF_BIT else node[c]
