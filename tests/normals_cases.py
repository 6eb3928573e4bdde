"""Cases of the normal sets (rayhip_normals_create; ray_amd/csrc/normals.h): one scene of deforming meshes whose bitangents the
reference's scene build derived itself, seeded poses, the host build of the element functions (tests/hostsim/hostsim_normals.cpp), an
independent numpy restatement of what they compute and a float64 model of the normals.  Shared by tests/test_normals_hostsim.py and
tests/test_gpu_normals.py.

The scene `cloth` (through the drop-in's scene build, so the vertex array holds the twins it appends and the bitangents it derives):
  room     the Cornell box with its light (vertex_update_cases._room)
  sheet    a 48 x 48 wavy sheet WITHOUT a bitangent layout: many blocks of 256 vertices
  mirror   the same sheet, 24 x 24, its u mirrored about the middle of a quad column: twin vertices along the mirror and faces without
           uv area (the axis fallback of the tangent); under a normal-mapped material, so the per-triangle bitangent table is read
  fan      a hub with 300 triangles: its row is longer than one chunk of the device kernel (normals.hip.h: ROW_CHUNK = 256)
  sphere   a closed 16 x 8 uv-sphere with a duplicated seam column: the weld case
A pose is a smooth seeded displacement field, a function of the uploaded POSITION, added to the positions -- coincident vertices move
together -- while n, b and t are sent as uploaded: what a caller that computes positions only has."""
import ctypes as C
import os

import numpy as np

import skin_cases as S
import util
import vertex_update_cases as V
from ray_amd import hip, scenes
from ray_amd.api import PrincipledMat, ShadingNode, eShadingNode

NORMALS_LIB = os.path.join(util.ROOT, "tests", "hostsim", "_build", "libhostsim_normals.so")
N, B = 1, 2  # RAYHIP_NORMALS_N / _B
EPS = np.float32(0.0000001)  # the reference's FLT_EPS
MESHES = ("room", "sheet", "mirror", "fan", "sphere")
FAN_TRIANGLES = 300
POSES = (1, 2, 3)  # seeds of the deformed poses (0: the upload pose)


# ---- the scene ------------------------------------------------------------------------------------------------------------------
def _fan_mesh(n, cx, cy, cz, radius):
    """hub + n rim vertices, n triangles (hub, rim[i + 1], rim[i]): a shallow jittered cone that opens upwards, planar uvs"""
    rng = np.random.RandomState(21)
    th = 2.0 * np.pi * np.arange(n) / n
    r = radius * (1.0 + rng.uniform(-0.05, 0.05, size=n))
    rim = np.stack([cx + r * np.cos(th), cy + 0.25 * radius + rng.uniform(-0.02, 0.02, size=n) * radius, cz + r * np.sin(th)], axis=-1)
    pos = np.concatenate([[[cx, cy, cz]], rim])
    idx = np.stack([np.zeros(n, dtype=np.int64), 1 + (np.arange(n) + 1) % n, 1 + np.arange(n)], axis=-1)
    uv = np.stack([(pos[:, 0] - cx) / radius + 1.5, (pos[:, 2] - cz) / radius + 1.5], axis=-1)
    return _with_normals(pos, idx, uv)


def _sphere_mesh(segments, stacks, cx, cy, cz, radius):
    """two pole vertices and stacks - 1 rings of segments + 1 vertices: the last column repeats the first at u = 4 (the seam)"""
    pos, uv = [[cx, cy + radius, cz]], [[2.0, 0.0]]
    for s in range(1, stacks):
        phi = np.pi * s / stacks
        for k in range(segments + 1):
            th = 2.0 * np.pi * (k % segments) / segments
            pos.append([cx + radius * np.sin(phi) * np.cos(th), cy + radius * np.cos(phi), cz + radius * np.sin(phi) * np.sin(th)])
            uv.append([4.0 * k / segments, 4.0 * s / stacks])
    pos.append([cx, cy - radius, cz])
    uv.append([2.0, 4.0])
    ring = lambda s: 1 + (s - 1) * (segments + 1)  # noqa: E731
    south = len(pos) - 1
    idx = []
    for k in range(segments):
        idx.append([0, ring(1) + k + 1, ring(1) + k])
        idx.append([south, ring(stacks - 1) + k, ring(stacks - 1) + k + 1])
        for s in range(1, stacks - 1):
            a, b = ring(s) + k, ring(s + 1) + k
            idx += [[a, a + 1, b + 1], [a, b + 1, b]]
    pos, idx = np.asarray(pos), np.asarray(idx, dtype=np.int64)
    # wound so that every face normal points away from the centre
    fn = np.cross(pos[idx[:, 1]] - pos[idx[:, 0]], pos[idx[:, 2]] - pos[idx[:, 0]])
    inward = (fn * (pos[idx].mean(axis=1) - [cx, cy, cz])).sum(axis=1) < 0
    idx[inward] = idx[inward][:, [0, 2, 1]]
    return _with_normals(pos, idx, np.asarray(uv))


def _with_normals(pos, idx, uv):
    """(attrs [n][8] position3 normal3 uv2, indices): area-weighted normals over coincident positions, in float64"""
    fn = np.cross(pos[idx[:, 1]] - pos[idx[:, 0]], pos[idx[:, 2]] - pos[idx[:, 0]])
    _, group = np.unique(np.round(pos, 9), axis=0, return_inverse=True)
    group = group.ravel()
    acc = np.zeros((group.max() + 1, 3))
    for k in range(3):
        np.add.at(acc, group[idx[:, k]], fn)
    nrm = acc[group]
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return np.concatenate([pos, nrm, uv], axis=1).astype(np.float32), idx.reshape(-1).astype(np.uint32)


def cloth(scene):
    scene.SetEnvironment(env_col=(0.0, 0.0, 0.0))
    V._room(scene)
    blue = scene.AddMaterial(ShadingNode(type=eShadingNode.Diffuse, base_color=(0.2, 0.3, 0.7)))
    t_nrm = scene.AddTexture(scenes.bump_normal_map(64), is_srgb=False, is_normalmap=True)
    bumpy = scene.AddMaterial(PrincipledMat(base_color=(0.7, 0.6, 0.3), roughness=0.6, normal_map=t_nrm, normal_map_intensity=1.0, specular=0.5))
    white = scene.AddMaterial(ShadingNode(type=eShadingNode.Diffuse, base_color=(0.7, 0.7, 0.7)))

    def add(attrs, idx, mat, xform=None):
        b = scenes._MeshBuilder()
        b.add(attrs, idx, mat)
        mesh = scene.AddMesh(*b.finish())  # position3, normal3, uv2: the bitangents are the scene build's to derive
        if xform is None:
            scene.AddMeshInstance(mesh)
        else:
            scene.AddMeshInstance(mesh, xform)

    attrs, idx = V._sheet_mesh(48, 0.0, -0.52, -0.04, -0.52, -0.04, 0.18, 0.05, seed=11)
    add(attrs[:, :8], idx, blue)
    attrs, idx = V._sheet_mesh(24, 0.0, -0.12, 0.12, -0.12, 0.12, 0.0, 0.03, seed=12)
    attrs = attrs[:, :8].copy()
    attrs[:, 6] = np.abs(attrs[:, 6] - np.float32(4.0 * 12.5 / 24.0))  # u mirrored about the middle of quad column 12
    add(attrs, idx, bumpy, scenes._xform(translate=(-0.28, 0.34, -0.30), rot_y_deg=20.0))
    add(*_fan_mesh(FAN_TRIANGLES, -0.13, 0.40, -0.15, 0.09), white)
    add(*_sphere_mesh(16, 8, -0.43, 0.44, -0.15, 0.07), white)
    scenes._cornell_camera(scene)
    scene.Finalize()


_scene = None


class Mesh:
    """one mesh of the scene: its vertex range [first, first + count) (the scene build's twins included) and its triangles, ascending"""

    def __init__(self, first, count, tris):
        self.first, self.count, self.tris = int(first), int(count), tris


def scene():
    """(blob, Arrays, {name: Mesh}) of `cloth`, built once per process (needs the host library of the drop-in)"""
    global _scene
    if _scene is None:
        from ray_amd import api
        s = api.CreateSceneHIP()
        cloth(s)
        blob = api.export_scene_blob(s)
        a = V.Arrays(blob)
        meshes = {}
        assert len(a.mesh_instances) >= len(MESHES)
        for name, mi in zip(MESHES, a.live_instances()):
            tris = tree_triangles(a, int(a.mesh_instances["node_index"][mi]))
            corners = a.vtx_indices[(3 * tris[:, None] + np.arange(3)).ravel()]
            meshes[name] = Mesh(corners.min(), corners.max() - corners.min() + 1, tris)
        _scene = (blob, a, meshes)
    return _scene


def tree_triangles(a: V.Arrays, root):
    """the triangles the bottom-level tree below `root` reaches, ascending (leaf word -> entries -> tri_indices)"""
    out, stack = set(), [root]
    while stack:
        for link in a.nodes[stack.pop(), 12:14]:
            if link & V.COUNT_BITS:
                first, count = int(link & V.INDEX_BITS), int((link & V.COUNT_BITS) >> 29) + 1
                out.update(int(t) for t in a.tri_indices[first:first + count])
            else:
                stack.append(int(link))
    return np.array(sorted(out), dtype=np.int64)


def corners_of(a: V.Arrays):
    """[triangles][3] vertex indices (the index array is a pool whose length need be no multiple of three)"""
    return a.vtx_indices[:len(a.vtx_indices) // 3 * 3].reshape(-1, 3)


def reachable(a: V.Arrays):
    """every triangle some bottom-level tree reaches, ascending, uint32"""
    return np.unique(a.tri_indices[a.reachable_entries()]).astype(np.uint32)


def posed(a: V.Arrays, meshes, seed, names=("sheet", "mirror", "fan", "sphere"), amplitude=0.012):
    """the vertex array with the positions of the named meshes displaced by a smooth field of their uploaded position (three sines per
    axis, seeded); seed 0: the upload pose.  n, b and t stay as uploaded."""
    v = a.vertices.copy()
    if seed == 0:
        return v
    rng = np.random.RandomState(100 + seed)
    k, phase, amp = rng.uniform(15.0, 45.0, size=(3, 3, 3)), rng.uniform(0.0, 6.28, size=(3, 3)), rng.uniform(0.3, 1.0, size=(3, 3))
    for name in names:
        m = meshes[name]
        p = v["p"][m.first:m.first + m.count].astype(np.float64)
        d = np.zeros_like(p)
        for axis in range(3):
            for j in range(3):
                d[:, axis] += amp[axis, j] * np.sin(p @ k[axis, j] + phase[axis, j])
        v["p"][m.first:m.first + m.count] = (p + amplitude / 3.0 * d).astype(np.float32)
    return v


# ---- the host build -------------------------------------------------------------------------------------------------------------
def have_normals_lib():
    return os.path.exists(NORMALS_LIB)


_lib = None


def normals_lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(NORMALS_LIB)
        vp, u32 = C.c_void_p, C.c_uint32
        _lib.hostsim_normals_validate.argtypes = [u32, u32, u32, u32, vp, C.POINTER(C.c_int)]
        _lib.hostsim_normals_reachable.argtypes = [vp, u32, vp, u32, vp, u32, vp, u32, u32, vp, u32]
        _lib.hostsim_normals_reachable.restype = u32
        _lib.hostsim_normals_rows.argtypes = [vp, u32, vp, u32, u32, vp, vp]
        _lib.hostsim_normals_table.argtypes = [C.c_int, vp]
        _lib.hostsim_normals_table.restype = None
        _lib.hostsim_normals_recompute.argtypes = [vp, vp, u32, vp, u32, u32, u32, vp]
        _lib.hostsim_normals_face.argtypes = [vp, vp]
        _lib.hostsim_normals_face.restype = None
    return _lib


def _weld_ptr(weld, count):
    if weld is None:
        return None, None
    w = np.ascontiguousarray(weld, dtype=np.uint32)
    assert w.shape == (count,)
    return w, w.ctypes.data


def host_validate(n_vertices, first, count, flags, weld=None):
    """(the code rayhip_normals_create returns for this description, which check refused it)"""
    keep = None if weld is None else np.ascontiguousarray(weld, dtype=np.uint32)
    why = C.c_int(0)
    rc = normals_lib().hostsim_normals_validate(n_vertices, first, count, flags, None if keep is None else keep.ctypes.data, C.byref(why))
    return rc, int(why.value)


def host_reachable(a: V.Arrays, nodes=None, tri_indices=None):
    """normals.h: reachable_triangles over the scene's bottom-level roots; `nodes` / `tri_indices`: the arrays a device holds"""
    nodes = np.ascontiguousarray(a.nodes if nodes is None else nodes, dtype=np.uint32)
    tri_indices = np.ascontiguousarray(a.tri_indices if tri_indices is None else tri_indices, dtype=np.uint32)
    roots = np.array(a.roots(), dtype=np.uint32)
    vi = np.ascontiguousarray(a.vtx_indices)
    out = np.zeros(len(vi) // 3, dtype=np.uint32)
    n = normals_lib().hostsim_normals_reachable(nodes.ctypes.data, len(nodes), roots.ctypes.data, len(roots), tri_indices.ctypes.data, len(tri_indices),
                                                vi.ctypes.data, len(vi) // 3, len(a.vertices), out.ctypes.data, len(out))
    assert n != 0xffffffff and n <= len(out)
    return out[:n].copy()


def host_rows(a: V.Arrays, tris, first, count, weld=None):
    """(rc, {faces, row, entries, wrow, wentries}) by the counting sort of normals.h"""
    tris = np.ascontiguousarray(tris, dtype=np.uint32)
    vi = np.ascontiguousarray(a.vtx_indices)
    keep, ptr = _weld_ptr(weld, count)
    sizes = (C.c_uint32 * 4)()
    rc = normals_lib().hostsim_normals_rows(tris.ctypes.data, len(tris), vi.ctypes.data, first, count, ptr, sizes)
    out = {}
    for which, (name, n) in enumerate((("faces", sizes[0]), ("row", count + 1 if rc == 0 else 0), ("entries", sizes[1]), ("wrow", sizes[2]), ("wentries", sizes[3]))):
        out[name] = np.zeros(n, dtype=np.uint32)
        if n:
            normals_lib().hostsim_normals_table(which, out[name].ctypes.data)
    return rc, out


def host_recompute(a: V.Arrays, vertices, tris, first, count, flags, weld=None):
    """`vertices` (the whole array) with n and / or b of [first, first + count) recomputed by tests/hostsim/hostsim_normals.cpp"""
    v = np.ascontiguousarray(vertices).copy()
    assert v.dtype == hip.VERTEX_DTYPE and len(v) == len(a.vertices)
    tris = np.ascontiguousarray(tris, dtype=np.uint32)
    vi = np.ascontiguousarray(a.vtx_indices)
    keep, ptr = _weld_ptr(weld, count)
    rc = normals_lib().hostsim_normals_recompute(v.ctypes.data, tris.ctypes.data, len(tris), vi.ctypes.data, first, count, flags, ptr)
    assert rc == 0, rc
    return v


def host_face(v3):
    """the 8 floats of the face record of three VERTEX_DTYPE records"""
    v3 = np.ascontiguousarray(v3)
    assert v3.dtype == hip.VERTEX_DTYPE and len(v3) == 3
    out = np.zeros(8, dtype=np.float32)
    normals_lib().hostsim_normals_face(v3.ctypes.data, out.ctypes.data)
    return out


# ---- numpy restatement: float32, one rounding per operation, the order of normals.h written out -------------------------------------
def python_rows(a: V.Arrays, tris, first, count, weld=None):
    """the tables made the slow way: every (vertex, face, corner) triple, sorted.  {faces, row, entries, wrow, wentries}"""
    corners = corners_of(a)
    inside = lambda v: first <= v < first + count  # noqa: E731
    faces = [int(t) for t in sorted(int(t) for t in tris) if any(inside(int(v)) for v in corners[t])]
    triples = sorted((int(v) - first, f, k) for f, t in enumerate(faces) for k, v in enumerate(corners[t]) if inside(int(v)))
    row = np.zeros(count + 1, dtype=np.uint32)
    for v, _, _ in triples:
        row[v + 1] += 1
    out = {"faces": np.array(faces, dtype=np.uint32), "row": np.cumsum(row, dtype=np.uint32), "entries": np.array([f for _, f, _ in triples], dtype=np.uint32),
           "wrow": np.zeros(0, dtype=np.uint32), "wentries": np.zeros(0, dtype=np.uint32)}
    if weld is not None:
        group = {}
        for v, f, k in triples:
            group.setdefault(int(weld[v]), []).append((f, k))
        wrow, wentries = [0], []
        for i in range(count):
            mine = sorted(group[int(weld[i])]) if row[i + 1] else []
            wentries += [f for f, _ in mine]
            wrow.append(len(wentries))
        out["wrow"], out["wentries"] = np.array(wrow, dtype=np.uint32), np.array(wentries, dtype=np.uint32)
    return out


def _cross(x, y):
    return np.stack([x[:, 1] * y[:, 2] - x[:, 2] * y[:, 1], x[:, 2] * y[:, 0] - x[:, 0] * y[:, 2], x[:, 0] * y[:, 1] - x[:, 1] * y[:, 0]], axis=-1)


def _length(x):
    return np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2])


def numpy_face_frames(v0, v1, v2):
    """([n][3] unnormalised face normals, [n][3] face tangents, [n] the face took the axis fallback) of faces with corner records v0 v1 v2"""
    f = np.float32
    with np.errstate(all="ignore"):
        dp1, dp2 = v1["p"] - v0["p"], v2["p"] - v0["p"]
        dt1, dt2 = v1["t"] - v0["t"], v2["t"] - v0["t"]
        plane = _cross(dp1, dp2)
        det = np.abs(dt1[:, 0] * dt2[:, 1] - dt1[:, 1] * dt2[:, 0])
        mapped = det > EPS
        inv = f(1.0) / np.where(mapped, det, f(1.0))
        tangent = (dp1 * dt2[:, 1:2] - dp2 * dt1[:, 1:2]) * inv[:, None]
        ax, ay, az = np.abs(plane[:, 0]), np.abs(plane[:, 1]), np.abs(plane[:, 2])
        pick_x = (ax <= ay) & (ax <= az)
        pick_z = ~pick_x & (az <= ax) & (az <= ay)
        axis = np.zeros_like(plane)
        axis[:, 1] = 1.0
        axis[pick_x], axis[pick_z] = (1.0, 0.0, 0.0), (0.0, 0.0, 1.0)
        w = np.where(pick_x, 1, np.where(pick_z, 0, 2))
        binormal = _cross(plane, axis)
        binormal = binormal / _length(binormal)[:, None]
        t2 = _cross(plane, binormal)
        t2 = t2 / _length(t2)[:, None]
        t2[~(np.abs(plane[np.arange(len(plane)), w]) > EPS)] = 0.0
        tangent = np.where(mapped[:, None], tangent, t2)
    assert plane.dtype == f and tangent.dtype == f
    return plane, tangent, ~mapped


def _row_sums(values, row, entries):
    """[count][3]: per vertex the float32 sum of values[entries[row[i] .. row[i + 1])] in row order, from zero"""
    count = len(row) - 1
    acc = np.zeros((count, 3), dtype=np.float32)
    length = (row[1:] - row[:-1]).astype(np.int64)
    for k in range(int(length.max()) if count else 0):
        has = length > k
        acc[has] = acc[has] + values[entries[row[:-1][has].astype(np.int64) + k]]
    return acc


def numpy_recompute(a: V.Arrays, vertices, tables, first, count, flags):
    """(`vertices` with the range recomputed, [count] the vertex took the branch b = T) from tables of python_rows / host_rows"""
    f = np.float32
    v = vertices.copy()
    c = corners_of(a)[tables["faces"].astype(np.int64)].astype(np.int64)
    fn, ft, _ = numpy_face_frames(vertices[c[:, 0]], vertices[c[:, 1]], vertices[c[:, 2]])
    row = tables["row"]
    has_face = row[1:] != row[:-1]
    part = v[first:first + count]
    n = part["n"].copy()
    raw = np.zeros(count, dtype=bool)
    with np.errstate(all="ignore"):
        if flags & N:
            welded = len(tables["wrow"]) > 0
            s = _row_sums(fn, tables["wrow"] if welded else row, tables["wentries"] if welded else tables["entries"])
            n = np.where(has_face[:, None], S._normalised_or_rest(s, part["n"]), part["n"]).astype(f)
        if flags & B:
            T = _row_sums(ft, row, tables["entries"])
            cr = _cross(n, T)
            length = _length(cr)
            use = (np.abs(T) > EPS).any(axis=1) & (length > EPS)
            b = np.where(use[:, None], cr / np.where(use, length, f(1.0))[:, None], T).astype(f)
            raw = has_face & ~use
            part["b"][has_face] = b[has_face]
        part["n"] = n
    v[first:first + count] = part
    return v, raw


def float64_normals(a: V.Arrays, vertices, tris, first, count, weld=None):
    """[count][3] float64 unit normals of the range: area-weighted sums over the weld groups, from the float32 positions; NaN where a
    vertex has no face"""
    corners = corners_of(a)[np.asarray(tris, dtype=np.int64)].astype(np.int64)
    p = vertices["p"].astype(np.float64)
    fn = np.cross(p[corners[:, 1]] - p[corners[:, 0]], p[corners[:, 2]] - p[corners[:, 0]])
    acc, own = np.zeros((count, 3)), np.zeros(count, dtype=bool)
    group = np.arange(count) if weld is None else np.asarray(weld, dtype=np.int64)
    for k in range(3):
        inside = (corners[:, k] >= first) & (corners[:, k] < first + count)
        np.add.at(acc, group[corners[inside, k] - first], fn[inside])
        own[corners[inside, k] - first] = True
    out = acc[group]
    out /= np.linalg.norm(out, axis=1, keepdims=True)
    out[~own] = np.nan
    return out


def angle(x, y):
    """[n] the angle between unit vectors, radians, in float64 (atan2 form: exact for small angles)"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return np.arctan2(np.linalg.norm(np.cross(x, y), axis=-1), (x * y).sum(axis=-1))


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype != hip.VERTEX_DTYPE else x.view(np.uint32).reshape(-1, 11)
