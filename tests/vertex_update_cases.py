"""Cases of the vertex update (rayhip_scene_update_vertices; ray_amd/csrc/refit.h): deforming scenes, the serialised-scene
arrays a test reads and patches, the host build of the refit (tests/hostsim/hostsim_refit.cpp) and an independent numpy
restatement of what it computes.  Shared by tests/test_vertex_update_hostsim.py and tests/test_gpu_vertex_update.py."""
import ctypes as C
import glob
import os
import struct

import numpy as np

import util
from ray_amd import hip, scenes
from ray_amd.api import PrincipledMat, ShadingNode, eShadingNode

REFIT_LIB = os.path.join(util.ROOT, "tests", "hostsim", "_build", "libhostsim_refit.so")
HEADER, SECTION = 16, 40  # scene_blob.h: Header {magic[8], count, pad}, Section {name[24], offset u64, size u64}
COUNT_BITS = 7 << 29
INDEX_BITS = ~COUNT_BITS & 0xffffffff
LIGHT_TYPE_TRI = 5  # rt_base.h
MESH_INSTANCE_DTYPE = np.dtype([("mesh_index", "<u4"), ("node_index", "<u4"), ("lights_index", "<u4"), ("ray_visibility", "<u4"),
                                ("xform", "<f4", 16), ("inv_xform", "<f4", 16)])
assert MESH_INSTANCE_DTYPE.itemsize == 144


# ---- scenes -----------------------------------------------------------------------------------------------------------------
def _room(scene):
    """the Cornell box with its light: one mesh, one instance; its vertices are the same in every phase"""
    grey = scene.AddMaterial(ShadingNode(type=eShadingNode.Diffuse, base_color=(0.5, 0.5, 0.5)))
    red = scene.AddMaterial(ShadingNode(type=eShadingNode.Diffuse, base_color=(0.5, 0.0, 0.0)))
    green = scene.AddMaterial(ShadingNode(type=eShadingNode.Diffuse, base_color=(0.0, 0.5, 0.0)))
    emit = scene.AddMaterial(ShadingNode(type=eShadingNode.Emissive, strength=100.0, importance_sample=True))
    attrs, idx = scenes.cornell_mesh_arrays(scenes._CORNELL_QUADS)
    room = scene.AddMesh(attrs, idx, [(grey, None, 0, 18), (red, None, 18, 6), (green, None, 24, 6), (emit, 0xFFFFFFFF, 30, 6)])
    scene.AddMeshInstance(room)


def _sheet_mesh(n, phase, x0, x1, z0, z1, y0, amplitude, seed):
    """n x n quads of y = y0 + a sin(kx + phase) cos(kz) over [x0, x1] x [z0, z1], every vertex lifted by a fixed jitter of its own
    (a seeded RNG, the same in every phase): no two vertices share a height, so no two box faces or triangle edges tie"""
    jitter = np.random.RandomState(seed).uniform(-0.15, 0.15, size=(n + 1, n + 1)) * amplitude

    def pos(u, v):
        x, z = x0 + (x1 - x0) * u, z0 + (z1 - z0) * v
        y = y0 + amplitude * np.sin(9.0 * u + phase) * np.cos(7.0 * v) + jitter
        return np.stack([x, y, z], axis=-1)

    attrs, idx = scenes._grid(n, n, scenes._finite_normals(pos))
    # bitangents come with the mesh: left to the scene build, it derives them from the uvs and SPLITS vertices where neighbouring
    # triangles disagree -- which would make the vertex and index arrays depend on the phase
    nrm = attrs[:, 3:6].astype(np.float64)
    tangent = np.array([1.0, 0.0, 0.0]) - nrm * nrm[:, :1]
    tangent /= np.linalg.norm(tangent, axis=-1, keepdims=True)
    return np.concatenate([attrs, np.cross(nrm, tangent).astype(np.float32)], axis=-1), idx


_SHEET_LAYOUT = dict(stride=11, bnm_offset=8)  # position3, normal3, uv2, bitangent3


def sheet(scene, phase):
    """the Cornell box plus ONE diffuse sheet of 48 x 48 quads (4608 triangles) as a mesh of its own: several 256-lane blocks,
    leaves of one or two triangles after the refinement, a tree of more than ten levels"""
    scene.SetEnvironment(env_col=(0.0, 0.0, 0.0))
    _room(scene)
    blue = scene.AddMaterial(ShadingNode(type=eShadingNode.Diffuse, base_color=(0.2, 0.3, 0.7)))
    b = scenes._MeshBuilder()
    b.add(*_sheet_mesh(48, phase, -0.52, -0.04, -0.52, -0.04, 0.18, 0.05, seed=11), blue)
    attrs, idx, groups = b.finish()
    scene.AddMeshInstance(scene.AddMesh(attrs, idx, groups, **_SHEET_LAYOUT))
    scenes._cornell_camera(scene)
    scene.Finalize()


def sheets_instanced(scene, phase, moved=False):
    """one 24 x 24 sheet (1152 triangles) with a normal-mapped material (the per-triangle bitangent table is in use), instanced
    three times under rotation, non-uniform scale and translation; the Cornell box is the other mesh.  `moved`: the second
    instance somewhere else (the instance path after the vertex path)"""
    scene.SetEnvironment(env_col=(0.0, 0.0, 0.0))
    _room(scene)
    t_nrm = scene.AddTexture(scenes.bump_normal_map(64), is_srgb=False, is_normalmap=True)
    bumpy = scene.AddMaterial(PrincipledMat(base_color=(0.7, 0.6, 0.3), roughness=0.6, normal_map=t_nrm, normal_map_intensity=1.0, specular=0.5))
    b = scenes._MeshBuilder()
    b.add(*_sheet_mesh(24, phase, -0.12, 0.12, -0.12, 0.12, 0.0, 0.03, seed=12), bumpy)
    attrs, idx, groups = b.finish()
    mesh = scene.AddMesh(attrs, idx, groups, **_SHEET_LAYOUT)
    scene.AddMeshInstance(mesh, scenes._xform(translate=(-0.37, 0.12, -0.37), rot_y_deg=20.0))
    second = (-0.22, 0.30, -0.30) if not moved else (-0.27, 0.36, -0.24)
    scene.AddMeshInstance(mesh, scenes._xform(translate=second, rot_y_deg=-35.0, rot_z_deg=15.0, scale=(1.3, 0.7, 0.9)))
    scene.AddMeshInstance(mesh, scenes._xform(translate=(-0.30, 0.20, -0.18), rot_z_deg=-25.0, scale=(0.8, 1.5, 1.2)))
    scenes._cornell_camera(scene)
    scene.Finalize()


SCENES = {"sheet": sheet, "sheets_instanced": sheets_instanced}
_blobs = {}


def scene_blob(name, phase, **kw):
    """the serialised scene `name` at `phase`, built once per process (needs the host library of the drop-in)"""
    from ray_amd import api
    key = (name, phase, tuple(sorted(kw.items())))
    if key not in _blobs:
        s = api.CreateSceneHIP()
        SCENES[name](s, float(phase), **kw)
        _blobs[key] = api.export_scene_blob(s)
    return _blobs[key]


# ---- serialised scenes ----------------------------------------------------------------------------------------------------
def fixture_names():
    return sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(util.GOLDEN, "*.rayscene")))


def sections(blob) -> dict:
    count = struct.unpack_from("<I", blob, 8)[0]
    out = {}
    for i in range(count):
        name, off, size = struct.unpack_from("<24sQQ", blob, HEADER + i * SECTION)
        out[name.rstrip(b"\0").decode()] = (off, size)
    return out


class Arrays:
    """the arrays of a serialised scene the refit reads, as writable copies"""

    def __init__(self, blob):
        s = sections(blob)

        def arr(name, dtype):
            off, size = s[name]
            return np.frombuffer(blob, dtype=dtype, count=size // np.dtype(dtype).itemsize, offset=off).copy()

        self.nodes = arr("nodes", "<u4").reshape(-1, 16)
        self.tris = arr("tris", "<f4").reshape(-1, 12)
        self.tri_indices = arr("tri_indices", "<u4")
        self.vertices = arr("vertices", hip.VERTEX_DTYPE)
        self.vtx_indices = arr("vtx_indices", "<u4")
        self.mesh_instances = arr("mesh_instances", MESH_INSTANCE_DTYPE)
        self.lights = arr("lights", "<u4").reshape(-1, 16)
        self.li_indices = arr("li_indices", "<u4")
        off, size = s["scalars"]
        self.tlas_root = struct.unpack_from("<I", blob, off + size - 40)[0]  # scene_blob.h: Scalars ends with 4 words + 2 x 3 floats

    def live_instances(self):
        """instance slots the top level names, ascending"""
        if self.tlas_root == 0xffffffff:
            return []
        out, stack = set(), [self.tlas_root]
        while stack:
            for link in self.nodes[stack.pop(), 12:14]:
                if link & COUNT_BITS:
                    out.add(int(link & INDEX_BITS))
                else:
                    stack.append(int(link))
        return sorted(out)

    def roots(self):
        """distinct bottom-level roots of the live instances"""
        return sorted({int(self.mesh_instances["node_index"][mi]) for mi in self.live_instances()})

    def blas_nodes(self):
        """(node indices below the roots ascending, the leaf words they hold) -- level by level, so that a large scene takes numpy time"""
        nodes, leaves, frontier = [], [], np.array(self.roots(), dtype=np.int64)
        while len(frontier):
            nodes.append(frontier)
            links = self.nodes[frontier, 12:14].ravel()
            leaf = (links & COUNT_BITS) != 0
            leaves.append(links[leaf])
            frontier = links[~leaf].astype(np.int64)
        if not nodes:
            return [], []
        return sorted(int(w) for w in np.concatenate(nodes)), [int(w) for w in np.concatenate(leaves)]

    def reachable_entries(self):
        words = np.array(self.blas_nodes()[1], dtype=np.int64)
        first, count = words & INDEX_BITS, ((words & COUNT_BITS) >> 29) + 1
        if not len(words):
            return np.zeros(0, dtype=np.int64)
        offs = np.arange(count.sum()) - np.repeat(np.cumsum(count) - count, count)
        return np.unique(np.repeat(first, count) + offs)

    def light_vertices(self):
        """vertices the triangles of triangle lights use"""
        out = set()
        for i in self.li_indices:
            if self.lights[i, 0] & 7 == LIGHT_TYPE_TRI:
                tri = int(self.lights[i, 4])  # params[0]: the triangle, as bits
                out.update(int(v) for v in self.vtx_indices[3 * tri:3 * tri + 3])
        return sorted(out)

    def top_level_leaves(self):
        """{instance slot: [lo.xyz, hi.xyz]} as the top level stores them (the union, where a slot is stored twice)"""
        out, stack = {}, [] if self.tlas_root == 0xffffffff else [self.tlas_root]
        f = self.nodes.view(np.float32)
        while stack:
            w = stack.pop()
            for k, link in enumerate(self.nodes[w, 12:14]):
                if not link & COUNT_BITS:
                    stack.append(int(link))
                    continue
                box = child_box(f[w], k)
                if np.all(box[:3] <= box[3:]):
                    mi = int(link & INDEX_BITS)
                    out[mi] = box if mi not in out else np.concatenate([np.minimum(out[mi][:3], box[:3]), np.maximum(out[mi][3:], box[3:])])
        return out


def child_box(node_f32, k):
    """[lo.xyz, hi.xyz] of child k of a BVH2 node given as 16 float words"""
    n = node_f32
    if k == 0:
        return np.array([n[0], n[2], n[8], n[1], n[3], n[9]], dtype=np.float32)
    return np.array([n[4], n[6], n[10], n[5], n[7], n[11]], dtype=np.float32)


def patched_blob(blob, **arrays):
    """`blob` with the named sections replaced by arrays of the same size"""
    b, s = bytearray(blob), sections(blob)
    for name, a in arrays.items():
        raw = np.ascontiguousarray(a).tobytes()
        off, size = s[name]
        assert len(raw) == size, (name, len(raw), size)
        b[off:off + size] = raw
    return bytes(b)


def perturbed_vertices(a: Arrays, seed=7, fraction=0.05):
    """the positions moved by up to +-`fraction` of the scene's extent (seeded), the vertices of triangle lights left alone"""
    v = a.vertices.copy()
    t = a.tri_indices[a.reachable_entries()].astype(np.int64)  # (the arrays are sparse pools: only what a leaf reaches is a triangle)
    used = np.unique(np.concatenate([a.vtx_indices[3 * t], a.vtx_indices[3 * t + 1], a.vtx_indices[3 * t + 2]]))
    ext = v["p"][used].max(axis=0) - v["p"][used].min(axis=0)
    d = np.random.RandomState(seed).uniform(-fraction, fraction, size=v["p"].shape).astype(np.float32) * ext.astype(np.float32)
    d[a.light_vertices()] = 0.0
    v["p"] = v["p"] + d
    return v


def collapse_one_triangle(a: Arrays, v):
    """(triangle, vertex moved): one triangle of `v` made a line -- a corner that no other triangle uses is put onto another corner, so
    exactly one triangle loses its area; not a triangle of a light"""
    t_all = np.unique(a.tri_indices[a.reachable_entries()]).astype(np.int64)
    corners = a.vtx_indices[(3 * t_all[:, None] + np.arange(3)).ravel()]
    uses = np.bincount(corners, minlength=len(v))
    lights = set(a.light_vertices())
    for t in t_all:
        c = [int(i) for i in a.vtx_indices[3 * t:3 * t + 3]]
        lone = [i for i in c if uses[i] == 1 and i not in lights]
        if lone:
            v["p"][lone[0]] = v["p"][[i for i in c if i != lone[0]][0]]
            return int(t), lone[0]
    raise AssertionError("no triangle with a corner of its own")


# ---- the host build of the refit ------------------------------------------------------------------------------------------------
def have_refit_lib():
    return os.path.exists(REFIT_LIB)


_lib = None


def refit_lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(REFIT_LIB)
        vp, u32 = C.c_void_p, C.c_uint32
        _lib.hostsim_refit_tris.argtypes = [vp, u32, vp, u32, vp, u32, vp, C.POINTER(u32)]
        _lib.hostsim_refit_nodes.argtypes = [vp, u32, vp, u32, vp, vp, vp]
        _lib.hostsim_instance_boxes.argtypes = [vp, u32, vp, u32, vp, u32, vp]
    return _lib


def refit_tris(vertices, vtx_indices, tri_indices, tris):
    """(records [n][12] f32, triangles without area): `tris` with every entry that names a triangle recomputed"""
    vertices, vtx_indices, tri_indices = (np.ascontiguousarray(x) for x in (vertices, vtx_indices, tri_indices))
    out = np.ascontiguousarray(tris, dtype=np.float32).copy()
    n = C.c_uint32(0)
    rc = refit_lib().hostsim_refit_tris(vertices.ctypes.data, len(vertices), vtx_indices.ctypes.data, len(vtx_indices), tri_indices.ctypes.data,
                                        len(tri_indices), out.ctypes.data, C.byref(n))
    assert rc == 0
    return out, int(n.value)


def refit_nodes(nodes, roots, tri_indices, vtx_indices, vertices):
    """nodes [n][16] u32 words with the child boxes of everything below `roots` recomputed"""
    vertices, vtx_indices, tri_indices = (np.ascontiguousarray(x) for x in (vertices, vtx_indices, tri_indices))
    out = np.ascontiguousarray(nodes, dtype=np.uint32).copy()
    roots = np.ascontiguousarray(roots, dtype=np.uint32)
    rc = refit_lib().hostsim_refit_nodes(out.ctypes.data, len(out), roots.ctypes.data, len(roots), tri_indices.ctypes.data, vtx_indices.ctypes.data,
                                         vertices.ctypes.data)
    assert rc == 0, rc
    return out


def instance_boxes(nodes, mesh_instances, slots):
    """[n][6] f32 (lo, hi): the box of each slot's tree root under its transform"""
    nodes = np.ascontiguousarray(nodes, dtype=np.uint32)
    mesh_instances = np.ascontiguousarray(mesh_instances, dtype=MESH_INSTANCE_DTYPE)
    slots = np.ascontiguousarray(slots, dtype=np.uint32)
    out = np.zeros((len(slots), 6), dtype=np.float32)
    rc = refit_lib().hostsim_instance_boxes(nodes.ctypes.data, len(nodes), mesh_instances.ctypes.data, len(mesh_instances), slots.ctypes.data,
                                            len(slots), out.ctypes.data)
    assert rc == 0
    return out


def host_refit(a: Arrays, vertices, nodes=None, tri_indices=None, tris=None):
    """(records, nodes, triangles without area) of the scene `a` under new vertices; `nodes` / `tri_indices` / `tris`: the arrays a
    device holds instead of the blob's (after the leaf refinement)"""
    nodes = a.nodes if nodes is None else nodes
    tri_indices = a.tri_indices if tri_indices is None else tri_indices
    tris = a.tris if tris is None else tris
    recs, n_degenerate = refit_tris(vertices, a.vtx_indices, tri_indices, tris)
    return recs, refit_nodes(nodes, a.roots(), tri_indices, a.vtx_indices, vertices), n_degenerate


# ---- numpy restatement: float32, one rounding per operation ----------------------------------------------------------------------
def numpy_tri_accel(p0, p1, p2):
    """[n][12] records (n_plane, u_plane, v_plane) of triangles with corners p0, p1, p2 ([n][3] float32): the arithmetic of the
    reference's PreprocessTri (internal/Core.cpp:212-258) in its operation order; a triangle without area gets zeros"""
    f = np.float32
    p0, p1, p2 = (np.asarray(p, dtype=f) for p in (p0, p1, p2))
    e0, e1 = p1 - p0, p2 - p0
    n = np.stack([e0[:, 1] * e1[:, 2] - e0[:, 2] * e1[:, 1], e0[:, 2] * e1[:, 0] - e0[:, 0] * e1[:, 2], e0[:, 0] * e1[:, 1] - e0[:, 1] * e1[:, 0]], axis=-1)
    len2 = n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2]
    ok = len2 != 0
    d = np.where(ok, len2, f(1.0))
    u = np.stack([(e1[:, 1] * n[:, 2] - e1[:, 2] * n[:, 1]) / d, (e1[:, 2] * n[:, 0] - e1[:, 0] * n[:, 2]) / d, (e1[:, 0] * n[:, 1] - e1[:, 1] * n[:, 0]) / d], axis=-1)
    v = np.stack([(n[:, 1] * e0[:, 2] - n[:, 2] * e0[:, 1]) / d, (n[:, 2] * e0[:, 0] - n[:, 0] * e0[:, 2]) / d, (n[:, 0] * e0[:, 1] - n[:, 1] * e0[:, 0]) / d], axis=-1)
    uw = -(u[:, 0] * p0[:, 0] + u[:, 1] * p0[:, 1] + u[:, 2] * p0[:, 2])
    vw = -(v[:, 0] * p0[:, 0] + v[:, 1] * p0[:, 1] + v[:, 2] * p0[:, 2])
    length = np.sqrt(d)
    nn = n / length[:, None]
    nw = nn[:, 0] * p0[:, 0] + nn[:, 1] * p0[:, 1] + nn[:, 2] * p0[:, 2]
    out = np.concatenate([nn, nw[:, None], u, uw[:, None], v, vw[:, None]], axis=-1).astype(f)
    assert out.dtype == f and len2.dtype == f
    out[~ok] = 0.0
    return out


def numpy_entry_records(a: Arrays, vertices, entries, tri_indices=None):
    tri_indices = a.tri_indices if tri_indices is None else tri_indices
    t = tri_indices[entries].astype(np.int64)
    p = vertices["p"]
    return numpy_tri_accel(p[a.vtx_indices[3 * t]], p[a.vtx_indices[3 * t + 1]], p[a.vtx_indices[3 * t + 2]])


def numpy_boxes_below(a: Arrays, vertices, nodes, tri_indices=None):
    """{(node, child): [lo, hi]} for every node below the roots: the min / max of the positions below that child"""
    tri_indices = a.tri_indices if tri_indices is None else tri_indices
    p, out = vertices["p"], {}

    def box_of(link):
        if link & COUNT_BITS:
            first, count = link & INDEX_BITS, ((link & COUNT_BITS) >> 29) + 1
            t = tri_indices[first:first + count].astype(np.int64)
            pts = p[np.concatenate([a.vtx_indices[3 * t], a.vtx_indices[3 * t + 1], a.vtx_indices[3 * t + 2]])]
            return np.concatenate([pts.min(axis=0), pts.max(axis=0)])
        boxes = [visit(int(link), k) for k in range(2)]
        return np.concatenate([np.minimum(boxes[0][:3], boxes[1][:3]), np.maximum(boxes[0][3:], boxes[1][3:])])

    def visit(w, k):
        if (w, k) not in out:
            out[(w, k)] = box_of(int(nodes[w, 12 + k]))
        return out[(w, k)]

    for root in a.roots():
        visit(root, 0), visit(root, 1)
    return out
