"""Cases of moving and recolouring analytic lights on the device (rayhip_scene_set_lights; ray_amd/csrc/light_pose.h): the host build
of the element functions (tests/hostsim/hostsim_light_pose.cpp), numpy packers that restate the reference's AddLight, a numpy
restatement of the summary, the flux and the three words of a leaf slot, a generated scene with many small lights, and the state a
context holds as plain arrays.  Shared by tests/test_light_pose_hostsim.py and tests/test_gpu_light_pose.py."""
import ctypes as C
import os

import numpy as np

import light_refit_cases as L
import util
from ray_amd import scenes
from ray_amd.api import ShadingNode, eShadingNode

POSE_LIB = os.path.join(util.ROOT, "tests", "hostsim", "_build", "libhostsim_light_pose.so")
BAD_SLOT, DUPLICATE, BAD_TYPE, FLAGS_CHANGED, NOT_FINITE, N_FINDINGS = 0, 1, 2, 3, 4, 5  # light_pose.h
TYPE_SPHERE, TYPE_DIR, TYPE_LINE, TYPE_RECT, TYPE_DISK, TYPE_TRI, TYPE_ENV = range(7)  # rt_base.h
f32 = np.float32
PI = f32(3.14159265358979323846)
bits = L.bits


# ---- the host build -------------------------------------------------------------------------------------------------------------
_lib = None


def pose_lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(POSE_LIB)
        vp, u32 = C.c_void_p, C.c_uint32
        _lib.hostsim_analytic_light_summaries.argtypes = [vp, u32, vp]
        _lib.hostsim_light_live_table.argtypes = [vp, u32, u32, vp]
        _lib.hostsim_set_lights.argtypes = [vp, u32, vp, vp, vp, vp, u32, vp, vp, vp, u32, vp, vp, vp]
        _lib.hostsim_refit_light_nodes_posed.argtypes = [vp, u32, vp, u32, vp, vp, vp, vp, vp]
    return _lib


def host_summaries(records):
    records = np.ascontiguousarray(records, dtype=np.uint32).reshape(-1, 16)
    out = np.zeros(len(records), dtype=L.SUMMARY)
    with np.errstate(all="ignore"):
        assert pose_lib().hostsim_analytic_light_summaries(records.ctypes.data, len(records), out.ctypes.data) == 0
    return out


class State:
    """what a context holds of the lights once rayhip_scene_refit_lights prepared its tables, as plain arrays: lights [n][16] u32, the
    tree, its importance rows, the leaf table, the flux scales of the inner slots, and the `live` and `posed` bytes"""

    def __init__(self, a: L.Arrays):
        self.lights = np.ascontiguousarray(a.lights, dtype=np.uint32).copy()
        self.cwnodes = a.cwnodes.copy()
        self.children = L.fill_children(a.cwnodes)
        self.leaf = L.leaf_table(a.lights, a.cwnodes)
        self.scales = L.slot_scales(a.lights, a.li_indices, a.mesh_instances, a.vtx_indices, a.vertices, a.cwnodes)
        # (the triangle lights' summaries: every refit of a context writes them; here once, at the pose of the upload)
        r = L.host_refit(a, a.vertices)
        tri = a.tri_lights()
        self.leaf[tri] = r.leaf[tri]
        self.live = np.zeros(len(self.lights), dtype=np.uint8)
        li = np.ascontiguousarray(a.li_indices, dtype=np.uint32)
        assert pose_lib().hostsim_light_live_table(li.ctypes.data, len(li), len(self.lights), self.live.ctypes.data) == 0
        self.posed = np.zeros(len(self.lights), dtype=np.uint8)

    def copy(self):
        s = State.__new__(State)
        for k, v in self.__dict__.items():
            setattr(s, k, v.copy())
        return s

    def arrays(self):
        return dict(lights=self.lights, cwnodes=self.cwnodes, children=self.children, leaf=self.leaf, posed=self.posed)

    def same(self, other):
        return all(np.array_equal(bits(v), bits(other.arrays()[k])) for k, v in self.arrays().items())


def host_set_lights(state: State, slots, records):
    """(return code, findings [5], the state after the call) by tests/hostsim/hostsim_light_pose.cpp"""
    s = state.copy()
    slots = np.ascontiguousarray(slots, dtype=np.uint32).ravel()
    records = np.ascontiguousarray(records, dtype=np.uint32).reshape(-1, 16)
    assert len(slots) == len(records)
    findings = np.zeros(N_FINDINGS, dtype=np.uint32)
    scratch = np.zeros(len(s.cwnodes), dtype=L.SUMMARY)
    with np.errstate(all="ignore"):
        rc = pose_lib().hostsim_set_lights(s.lights.ctypes.data, len(s.lights), s.live.ctypes.data, s.posed.ctypes.data, s.leaf.ctypes.data,
                                           s.cwnodes.ctypes.data, len(s.cwnodes), scratch.ctypes.data, s.children.ctypes.data, s.scales.ctypes.data,
                                           len(slots), slots.ctypes.data, records.ctypes.data, findings.ctypes.data)
    return rc, findings, s


def host_refit_posed(state: State, posed=True):
    """the state after a level refit alone, under its `posed` table or (posed=False) under none"""
    s = state.copy()
    scratch = np.zeros(len(s.cwnodes), dtype=L.SUMMARY)
    rc = pose_lib().hostsim_refit_light_nodes_posed(s.cwnodes.ctypes.data, len(s.cwnodes), s.lights.ctypes.data, len(s.lights), s.leaf.ctypes.data,
                                                    scratch.ctypes.data, s.children.ctypes.data, s.scales.ctypes.data, s.posed.ctypes.data if posed else None)
    assert rc == 0
    return s


def analytic_slots(a: L.Arrays):
    """light slots li_indices names that hold sphere, spot, directional, line, rect or disk lights, ascending"""
    return sorted(int(i) for i in a.li_indices if a.lights[i, 0] & 7 <= TYPE_DISK)


def leaf_words(cwnodes, paths, slot):
    """(flux bits, axis word, cosine word) of the leaf slot that names light `slot`"""
    w, i = paths[slot][-1]
    return int(bits(cwnodes["flux"][w, i:i + 1])[0]), int(cwnodes["axis"][w, i]), int(cwnodes["cos_omega_ne"][w, i])


# ---- numpy packers: the reference's AddLight (SceneCPU.cpp:617-766), float32, one rounding per operation, its order ----------------
def _record(word0, color, params):
    r = np.zeros(16, dtype=np.uint32)
    r[0] = word0
    r[1:4] = np.asarray(color, dtype=f32).view(np.uint32)
    r[4:16] = np.asarray(params, dtype=f32).view(np.uint32)
    return r


def _direction(x, y, z, m):
    """TransformDirection (CoreRef.cpp:2806): (m0 * x + m4 * y) + m8 * z, per row"""
    x, y, z = f32(x), f32(y), f32(z)
    return np.array([(m[0] * x + m[4] * y) + m[8] * z, (m[1] * x + m[5] * y) + m[9] * z, (m[2] * x + m[6] * y) + m[10] * z], dtype=f32)


def pack(kind, word0, **kw):
    """the 64-byte record AddLight makes of a light description, with `word0` as the slot holds it; kw as scene.AddLight takes them"""
    col = np.asarray(kw["color"], dtype=f32)
    z = f32(0.0)
    if kind in ("sphere", "spot"):
        r = f32(kw["radius"])
        area = ((f32(4.0) * PI) * r) * r
        pos = np.asarray(kw["position"], dtype=f32)
        if kind == "sphere":
            return _record(word0, col, [*pos, area, z, z, z, r, f32(-1.0), f32(-1.0), z, z])
        d = np.asarray(kw["direction"], dtype=f32)
        spot = ((f32(0.5) * PI) * f32(kw["spot_size"])) / f32(180.0)
        blend = f32(kw["spot_blend"]) * f32(kw["spot_blend"])
        return _record(word0, col, [*pos, area, *d, r, spot, blend, z, z])
    m = np.asarray(kw["xform"], dtype=f32).ravel()
    pos = m[12:15]
    if kind == "rect":
        w, h = f32(kw["width"]), f32(kw["height"])
        return _record(word0, col, [*pos, w * h, *(w * _direction(1, 0, 0, m)), z, *(h * _direction(0, 0, 1, m)), z])
    if kind == "disk":
        w, h = f32(kw["width"]), f32(kw["height"])
        return _record(word0, col, [*pos, ((f32(0.25) * PI) * w) * h, *(w * _direction(1, 0, 0, m)), z, *(h * _direction(0, 0, 1, m)), z])
    assert kind == "line"
    r, h = f32(kw["radius"]), f32(kw["height"])
    return _record(word0, col, [*pos, ((f32(2.0) * PI) * r) * h, *_direction(1, 0, 0, m), r, *_direction(0, 1, 0, m), h])


# ---- numpy restatement of light_pose.h / light_refit.h: summary, flux, the words of a leaf slot -------------------------------------
def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], dtype=f32)


def np_summary(record):
    """one SUMMARY record: RebuildLightTree_nolock (SceneCPU.cpp:1235-1358) in float32, sums from the left"""
    record = np.ascontiguousarray(record, dtype=np.uint32).reshape(16)
    kind, doublesided = int(record[0] & 7), bool((record[0] >> 3) & 1)
    col, p = record[1:4].view(f32), record[4:16].view(f32)
    s = np.zeros(1, dtype=L.SUMMARY)[0]
    s["axis"], s["omega_n"], s["omega_e"] = (0.0, 1.0, 0.0), PI, PI / f32(2.0)
    area = f32(1.0)
    with np.errstate(all="ignore"):
        if kind == TYPE_SPHERE:
            s["lo"], s["hi"] = p[0:3] - p[7], p[0:3] + p[7]
            if p[3] != 0:
                area = p[3]
        elif kind == TYPE_DIR:
            s["lo"], s["hi"], s["axis"] = -L.MAX_DIST, L.MAX_DIST, p[0:3]
            s["omega_n"], s["omega_e"] = 0.0, p[5]
            if p[4] != 0:
                area = (PI * p[4]) * p[4]
        elif kind == TYPE_LINE:
            pos, u, d = p[0:3], p[4:7], p[8:11]
            v = _cross(u, d)
            u, v, d = u * p[7], v * p[7], d * (f32(0.5) * p[11])
            c = np.array([((pos + sd * d) + su * u) + sv * v for sd in (1, -1) for su in (1, -1) for sv in (1, -1)], dtype=f32)
            s["lo"], s["hi"] = c.min(axis=0), c.max(axis=0)
            area = p[3]
        else:
            assert kind in (TYPE_RECT, TYPE_DISK)
            pos, u, v = p[0:3], f32(0.5) * p[4:7], f32(0.5) * p[8:11]
            c = np.array([(pos + su * u) + sv * v for su in (1, -1) for sv in (1, -1)], dtype=f32)
            s["lo"], s["hi"] = c.min(axis=0), c.max(axis=0)
            n = _cross(u, v)
            length = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
            if length > 0 and np.isfinite(length):
                s["axis"] = n / length
            s["omega_n"] = PI if doublesided else f32(0.0)
            area = p[3]
        s["flux"] = ((col[0] + col[1]) + col[2]) * area
    assert all(s[k].dtype == f32 for k in ("lo", "hi", "flux", "axis"))
    return s


def np_summaries(records):
    records = np.ascontiguousarray(records, dtype=np.uint32).reshape(-1, 16)
    return np.array([np_summary(r) for r in records], dtype=L.SUMMARY)


def _snorm16(x):
    x = np.clip((f32(x) + f32(1.0)) / f32(2.0), f32(0.0), f32(1.0)) * f32(65535.0)
    return int(np.floor(np.float64(x) + 0.5)) & 0xffff  # roundf of a float that is not negative


def np_axis_word(axis):
    """light_refit.h: encode_axis"""
    d = np.asarray(axis, dtype=f32)
    denom = (np.abs(d[0]) + np.abs(d[1])) + np.abs(d[2])
    v = d / denom
    if v[2] < 0:
        return (_snorm16((f32(1.0) - np.abs(v[1])) * np.copysign(f32(1.0), v[0])) << 16) | _snorm16((f32(1.0) - np.abs(v[0])) * np.copysign(f32(1.0), v[1]))
    return (_snorm16(v[0]) << 16) | _snorm16(v[1])


def np_cosine_word(record, summary):
    """light_refit.h: encode_cosines of (cos omega_n, max(cos omega_e, 0)).  omega_n is 0 or PI and omega_e PI / 2, whose cosines are
    1, -1 and 0 -- but a directional light's omega_e, whose cosine is the record's cos_angle (params[3])"""
    record = np.ascontiguousarray(record, dtype=np.uint32).reshape(16)
    cos_n = f32(1.0) if summary["omega_n"] == 0 else f32(-1.0)
    cos_e = max(record[7:8].view(f32)[0], f32(0.0)) if int(record[0] & 7) == TYPE_DIR else f32(0.0)
    a = int(np.floor(f32(65534.0) * ((cos_n + f32(1.0)) / f32(2.0))))
    b = int(np.floor(f32(65534.0) * ((cos_e + f32(1.0)) / f32(2.0))))
    return (a << 16) | b


def np_leaf_words(record):
    s = np_summary(record)
    return int(bits(s["flux"].reshape(1))[0]), np_axis_word(s["axis"]), np_cosine_word(record, s)


# ---- scenes -----------------------------------------------------------------------------------------------------------------------
class Relit:
    """a scene whose AddLight takes overrides by kind ({kind: {keyword: value}}): one of ray_amd.scenes' builders makes the same scene
    with some lights elsewhere"""

    def __init__(self, scene, overrides):
        self._scene, self._overrides = scene, overrides

    def __getattr__(self, name):
        return getattr(self._scene, name)

    def AddLight(self, kind, **kw):
        kw.update(self._overrides.get(kind, {}))
        return self._scene.AddLight(kind, **kw)


# cornell_lights (ray_amd/scenes.py) with every analytic light moved, turned, resized and recoloured: {kind: keywords}
CORNELL_MOVES = {
    "sphere": dict(color=(3.0, 6.5, 4.5), position=(-0.20, 0.38, -0.16), radius=0.035),
    "spot": dict(color=(24.0, 16.0, 20.0), position=(-0.40, 0.48, -0.14), direction=(0.30, -0.90, -0.2), radius=0.02, spot_size=40.0, spot_blend=0.35),
    "rect": dict(color=(5.0, 9.0, 8.0), width=0.12, height=0.14, xform=scenes._translate(-0.24, 0.50, -0.40, rot_x_deg=20.0, rot_z_deg=-15.0)),
    "disk": dict(color=(4.0, 5.0, 3.5), width=0.12, height=0.08, xform=scenes._translate(-0.53, 0.26, -0.24, rot_x_deg=10.0, rot_z_deg=-80.0)),
    "line": dict(color=(5.0, 3.0, 4.0), radius=0.009, height=0.20, xform=scenes._translate(-0.06, 0.30, -0.26, rot_x_deg=70.0, rot_z_deg=25.0)),
    "directional": dict(color=(0.9, 1.3, 1.1), direction=(-0.15, -0.60, -0.8), angle=7.0),
}
KINDS = ["sphere", "spot", "rect", "disk", "line", "directional"]  # the order cornell_lights adds them in: their light slots ascend


def cornell_blob(moves=None):
    """cornell_lights through the reference's scene build, with the lights of `moves` (kinds of CORNELL_MOVES) moved; built once"""
    from ray_amd import api
    key = ("cornell_lights", tuple(sorted(moves or ())))
    if key not in L._blobs:
        s = api.CreateSceneHIP()
        scenes.cornell_lights(Relit(s, {k: CORNELL_MOVES[k] for k in (moves or ())}))
        L._blobs[key] = api.export_scene_blob(s)
    return L._blobs[key]


def cornell_slots(a: L.Arrays):
    """{kind: light slot} of cornell_lights"""
    slots = analytic_slots(a)
    assert len(slots) == 6
    return dict(zip(KINDS, slots))


def field_specs(n, phase=0):
    """[(kind, keywords)] of light_field: n small sphere / rect / disk / line lights in turn, seeded; `phase` 1: every one of them
    somewhere else, turned, of another size and colour"""
    rng = np.random.RandomState(77 + int(phase))
    out = []
    for k in range(n):
        pos = (rng.uniform(-0.50, -0.06), rng.uniform(0.08, 0.50), rng.uniform(-0.50, -0.06))
        col = tuple(float(x) for x in rng.uniform(0.5, 4.0, size=3))
        turn = dict(rot_x_deg=float(rng.uniform(-80, 80)), rot_z_deg=float(rng.uniform(-80, 80)))
        kind = ("sphere", "rect", "disk", "line")[k % 4]
        if kind == "sphere":
            out.append((kind, dict(color=col, position=pos, radius=float(rng.uniform(0.004, 0.012)))))
        elif kind == "line":
            out.append((kind, dict(color=col, radius=float(rng.uniform(0.002, 0.004)), height=float(rng.uniform(0.02, 0.05)), xform=scenes._translate(*pos, **turn))))
        else:
            out.append((kind, dict(color=col, width=float(rng.uniform(0.01, 0.03)), height=float(rng.uniform(0.01, 0.03)), doublesided=bool(k % 8 < 4),
                                   xform=scenes._translate(*pos, **turn))))
    return out


def light_field(scene, n, phase=0):
    """a Cornell room without its lamp, lit by the n small lights of field_specs and one directional light: the light tree of
    n = 130 has 37 nodes in four heights, and a call that names every light has more than two wavefronts of entries"""
    scene.SetEnvironment(env_col=(0.0, 0.0, 0.0))
    grey = scene.AddMaterial(ShadingNode(type=eShadingNode.Diffuse, base_color=(0.5, 0.5, 0.5)))
    red = scene.AddMaterial(ShadingNode(type=eShadingNode.Diffuse, base_color=(0.5, 0.0, 0.0)))
    green = scene.AddMaterial(ShadingNode(type=eShadingNode.Diffuse, base_color=(0.0, 0.5, 0.0)))
    attrs, idx = scenes.cornell_mesh_arrays(scenes._CORNELL_QUADS)
    scene.AddMeshInstance(scene.AddMesh(attrs, idx, [(grey, None, 0, 18), (red, None, 18, 6), (green, None, 24, 6), (grey, None, 30, 6)]))
    for kind, kw in field_specs(n, phase):
        scene.AddLight(kind, **kw)
    scene.AddLight("directional", color=(0.3, 0.3, 0.35) if phase == 0 else (0.25, 0.35, 0.3), direction=(0.25, -0.45, -1.0) if phase == 0 else (-0.2, -0.7, -0.6),
                   angle=4.0 if phase == 0 else 6.0)
    scenes._cornell_camera(scene)
    scene.Finalize()


def field_blob(n, phase=0):
    from ray_amd import api
    key = ("light_field", n, phase)
    if key not in L._blobs:
        s = api.CreateSceneHIP()
        light_field(s, n, phase)
        L._blobs[key] = api.export_scene_blob(s)
    return L._blobs[key]


def field_records(a: L.Arrays, n, phase=1):
    """(slots, records) of the n small lights of light_field(n) at `phase`, packed by numpy with the words 0 the slots hold"""
    slots = analytic_slots(a)
    assert len(slots) == n + 1
    return np.array(slots[:n], dtype=np.uint32), np.array([pack(kind, a.lights[s, 0], **kw) for s, (kind, kw) in zip(slots, field_specs(n, phase))], dtype=np.uint32)
