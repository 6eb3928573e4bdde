"""Cases of changing materials on the device (rayhip_scene_set_materials; ray_amd/csrc/materials.h): the host build of the element
functions (tests/hostsim/hostsim_materials.cpp), numpy packers that restate the reference's AddMaterial, two scenes whose `phase`
changes only what the call may change, a numpy restatement of which material slots a scene uses, and the state a context holds as plain
arrays.  Shared by tests/test_materials_hostsim.py and tests/test_gpu_materials.py."""
import ctypes as C
import os

import numpy as np

import light_pose_cases as P
import light_refit_cases as L
import util
import vertex_update_cases as V
from ray_amd import hip, scenes
from ray_amd.api import PrincipledMat, ShadingNode, eShadingNode

MATERIALS_LIB = os.path.join(util.ROOT, "tests", "hostsim", "_build", "libhostsim_materials.so")
MATERIAL = hip.MATERIAL_DTYPE
BAD_SLOT, DUPLICATE, GRAPH_CHANGED, NOT_FINITE, NEGATIVE, REFRACTS, PINNED, EMITTERS_NAMED, N_COUNTERS = range(9)  # materials.h
SLOT_LIVE, SLOT_EMITTER, NO_EMITTER = 1, 2, 0xffff
MIX_MAT1, MIX_MAT2, MAT_INDEX_BITS, IMP_SAMPLE = 3, 4, 16383, 1  # rt_base.h
f32 = np.float32
PI = f32(3.14159265358979323846)
bits = L.bits


def words(records):
    """[n][19] uint32 of MATERIAL records"""
    return np.ascontiguousarray(records).view(np.uint32).reshape(-1, 19)


class Arrays(L.Arrays):
    """... and the materials"""

    def __init__(self, blob):
        super().__init__(blob)
        s = V.sections(blob)
        off, size = s["materials"]
        self.materials = np.frombuffer(blob, dtype=MATERIAL, count=size // MATERIAL.itemsize, offset=off).copy()
        off, size = s["tri_materials"]
        self.tri_materials = np.frombuffer(blob, dtype="<u2", count=size // 2, offset=off).copy().reshape(-1, 2)

    def used_materials(self):
        """uint8 [slots]: 1 where a triangle some leaf reaches, or a Mix node in use, names the slot (scene_validate.h: mat_used)"""
        tris = np.unique(self.tri_indices[self.reachable_entries()].astype(np.int64))
        todo = set(int(m) & MAT_INDEX_BITS for m in self.tri_materials[tris, 0])
        todo |= set(int(m) & MAT_INDEX_BITS for m in self.tri_materials[tris, 1] if m != 0xffff)
        used = np.zeros(len(self.materials), dtype=np.uint8)
        while todo:
            m = todo.pop()
            if used[m]:
                continue
            used[m] = 1
            if self.materials["type"][m] == eShadingNode.Mix:
                todo |= {int(self.materials["textures"][m, MIX_MAT1]), int(self.materials["textures"][m, MIX_MAT2])}
        return used


# ---- the host build -------------------------------------------------------------------------------------------------------------
_lib = None


def materials_lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(MATERIALS_LIB)
        vp, u32 = C.c_void_p, C.c_uint32
        _lib.hostsim_material_emitter_tables.argtypes = [vp, u32, vp, u32, vp, u32, vp, u32, vp, vp]
        _lib.hostsim_set_materials.argtypes = [vp, u32, vp, vp, C.c_int, C.c_int, u32, vp, vp, vp]
        _lib.hostsim_recolour_tri_lights.argtypes = [vp, u32, vp, vp, vp, u32]
    return _lib


def emitter_tables(a: Arrays):
    """(light_emitter uint16 [light slots], flags uint8 [material slots]) of the scene `a` by the host build"""
    lights, li = np.ascontiguousarray(a.lights, dtype=np.uint32), np.ascontiguousarray(a.li_indices, dtype=np.uint32)
    tm, mats = np.ascontiguousarray(a.tri_materials), np.ascontiguousarray(a.materials)
    emitter = np.zeros(len(lights), dtype=np.uint16)
    flags = (a.used_materials() * SLOT_LIVE).astype(np.uint8)
    assert materials_lib().hostsim_material_emitter_tables(lights.ctypes.data, len(lights), li.ctypes.data, len(li), tm.ctypes.data, len(tm), mats.ctypes.data,
                                                           len(mats), emitter.ctypes.data, flags.ctypes.data) == 0
    return emitter, flags


class State(P.State):
    """what a context holds of materials and lights as plain arrays: P.State plus the material array, the per-slot flags, the emitter of
    every light slot, the corners of the triangle lights, and whether the passes leave the rays' ior plane alone"""

    def __init__(self, a: Arrays):
        super().__init__(a)
        self.materials = a.materials.copy()
        self.emitter, self.flags = emitter_tables(a)
        self.tri_geom = L.fill_tri_geom(a, a.vertices)
        m = a.materials
        self.plain_ior = not bool(((m["type"] == eShadingNode.Refractive) | ((m["type"] == eShadingNode.Principled) & (m["transmission_unorm"] != 0))).any())
        self._a = a

    def copy(self):
        s = State.__new__(State)
        for k, v in self.__dict__.items():
            setattr(s, k, v.copy() if isinstance(v, np.ndarray) else v)
        return s

    def arrays(self):
        return dict(super().arrays(), materials=self.materials)


def host_set_materials(state: State, slots, records, refittable=True, plain_ior=None):
    """(return code, counters [8], the state after the call) by tests/hostsim/hostsim_materials.cpp, then -- when an emitter was named --
    the light refit of tests/hostsim/hostsim_lights.cpp over the recoloured lights, as the device runs it"""
    s = state.copy()
    a = s._a
    slots = np.ascontiguousarray(slots, dtype=np.uint32).ravel()
    records = np.ascontiguousarray(words(records))
    assert len(slots) == len(records)
    counters, claim = np.zeros(N_COUNTERS, dtype=np.uint32), np.zeros(len(s.materials), dtype=np.uint32)
    lib = materials_lib()
    with np.errstate(all="ignore"):
        rc = lib.hostsim_set_materials(s.materials.ctypes.data, len(s.materials), s.flags.ctypes.data, claim.ctypes.data, int(s.plain_ior if plain_ior is None else plain_ior),
                                       int(refittable), len(slots), slots.ctypes.data if len(slots) else None, records.ctypes.data if len(slots) else None,
                                       counters.ctypes.data)
    if rc == 0 and counters[EMITTERS_NAMED] and refittable:
        assert lib.hostsim_recolour_tri_lights(s.lights.ctypes.data, len(s.lights), s.emitter.ctypes.data, claim.ctypes.data, s.materials.ctypes.data,
                                               len(s.materials)) == 0
        li, mi = np.ascontiguousarray(a.li_indices, dtype=np.uint32), np.ascontiguousarray(a.mesh_instances)
        vi, v = np.ascontiguousarray(a.vtx_indices, dtype=np.uint32), np.ascontiguousarray(a.vertices)
        n = C.c_uint32(0)
        assert L.lights_lib().hostsim_refit_tri_lights(s.lights.ctypes.data, len(s.lights), li.ctypes.data, len(li), mi.ctypes.data, len(mi), vi.ctypes.data, len(vi),
                                                       v.ctypes.data, len(v), s.tri_geom.ctypes.data, s.leaf.ctypes.data, C.byref(n)) == 0
        refitted = P.host_refit_posed(s)
        s.cwnodes, s.children = refitted.cwnodes, refitted.children
    return rc, counters, s


# ---- numpy packers: the reference's AddMaterial (SceneCPU.cpp:209-340), float32, one rounding per operation, its order ---------------
def _unorm16(x):
    """pack_unorm_16(clamp(x, 0, 1)): uint16_t(x * 65535.0f)"""
    return np.uint16(int(np.clip(f32(x), f32(0.0), f32(1.0)) * f32(65535.0)))


_NODE_DEFAULTS = dict(base_color=(1.0, 1.0, 1.0), normal_map_intensity=1.0, roughness=0.0, anisotropic_rotation=0.0, sheen=0.0, strength=1.0, ior=1.0, tint=0.0)
_PRINCIPLED_DEFAULTS = dict(base_color=(1.0, 1.0, 1.0), metallic=0.0, specular=0.5, specular_tint=0.0, roughness=0.5, anisotropic=0.0, anisotropic_rotation=0.0,
                            sheen=0.0, sheen_tint=0.5, clearcoat=0.0, clearcoat_roughness=0.0, ior=1.45, transmission=0.0, transmission_roughness=0.0,
                            emission_color=(0.0, 0.0, 0.0), emission_strength=1.0, normal_map_intensity=1.0, importance_sample=False)


def _blank(held):
    """a record with the words that must stay taken from `held` and everything a call may change zero"""
    r = np.zeros(1, dtype=MATERIAL)[0]
    r["textures"], r["flags"], r["type"] = held["textures"], held["flags"], held["type"]
    return r


def _get(desc, defaults, key):
    v = getattr(desc, key, None)
    return defaults[key] if v is None else v


def _pack_node(desc: ShadingNode, held):
    g = lambda k: _get(desc, _NODE_DEFAULTS, k)  # noqa: E731
    r = _blank(held)
    r["roughness_unorm"] = _unorm16(g("roughness"))
    r["base_color"], r["ior"] = np.asarray(g("base_color"), dtype=f32), f32(g("ior"))
    if desc.type == eShadingNode.Diffuse:
        r["sheen_unorm"], r["sheen_tint_unorm"] = _unorm16(f32(0.5) * f32(g("sheen"))), _unorm16(g("tint"))
    elif desc.type == eShadingNode.Glossy:
        r["tangent_rotation_or_strength"] = (f32(2.0) * PI) * f32(g("anisotropic_rotation"))
        r["tint_unorm"] = _unorm16(g("tint"))
    elif desc.type in (eShadingNode.Emissive, eShadingNode.Mix):
        r["tangent_rotation_or_strength"] = f32(g("strength"))
    r["normal_map_strength_unorm"] = _unorm16(g("normal_map_intensity"))
    return r


def pack(desc, held):
    """the records AddMaterial makes of a description, with the textures, flags and type the slots hold (`held`: the records of the
    slots the description took, in slot order): one of a ShadingNode; of a PrincipledMat the Principled record and -- where it emits --
    the Emissive record and the additive Mix over the two"""
    if isinstance(desc, ShadingNode):
        assert len(held) == 1
        return [_pack_node(desc, held[0])]
    g = lambda k: _get(desc, _PRINCIPLED_DEFAULTS, k)  # noqa: E731
    r = _blank(held[0])
    r["base_color"] = np.asarray(g("base_color"), dtype=f32)
    r["sheen_unorm"], r["sheen_tint_unorm"] = _unorm16(f32(0.5) * f32(g("sheen"))), _unorm16(g("sheen_tint"))
    r["roughness_unorm"] = _unorm16(g("roughness"))
    r["tangent_rotation_or_strength"] = (f32(2.0) * PI) * np.clip(f32(g("anisotropic_rotation")), f32(0.0), f32(1.0))
    r["metallic_unorm"], r["ior"] = _unorm16(g("metallic")), f32(g("ior"))
    r["transmission_unorm"], r["transmission_roughness_unorm"] = _unorm16(g("transmission")), _unorm16(g("transmission_roughness"))
    r["normal_map_strength_unorm"], r["anisotropic_unorm"] = _unorm16(g("normal_map_intensity")), _unorm16(g("anisotropic"))
    r["specular_unorm"], r["specular_tint_unorm"] = _unorm16(g("specular")), _unorm16(g("specular_tint"))
    r["clearcoat_unorm"], r["clearcoat_roughness_unorm"] = _unorm16(g("clearcoat")), _unorm16(g("clearcoat_roughness"))
    out = [r]
    if g("emission_strength") > 0 and max(g("emission_color")) > 0:
        assert len(held) == 3
        out.append(_pack_node(ShadingNode(type=eShadingNode.Emissive, base_color=g("emission_color"), strength=g("emission_strength")), held[1]))
        out.append(_pack_node(ShadingNode(type=eShadingNode.Mix, strength=0.5, ior=0.0), held[2]))
    else:
        assert len(held) == 1
    return out


def slots_of(descs):
    """the material slots every description of a scene took ([[slot, ...]] in the order of `descs`): slots ascend as materials are added"""
    out, at = [], 0
    for d in descs:
        k = 3 if isinstance(d, PrincipledMat) and (d.emission_strength or 0) > 0 and max(d.emission_color or (0, 0, 0)) > 0 else 1
        out.append(list(range(at, at + k)))
        at += k
    return out


def packed(descs, a: Arrays):
    """(slots, records) of every description of `descs` packed by numpy over the records `a` holds"""
    slots, records = [], []
    for d, s in zip(descs, slots_of(descs)):
        slots += s
        records += pack(d, [a.materials[k] for k in s])
    return np.array(slots, dtype=np.uint32), np.array(records, dtype=MATERIAL)


# ---- scenes -----------------------------------------------------------------------------------------------------------------------
def cornell_descs(phase=0):
    """the materials of cornell_materials in the order they are added; `phase` 1: every value a call may change is another one;
    `phase` 2: the same but for the two emitters of triangle lights (the lamp, the emission of the last Principled), which stay"""
    p, e = int(phase) == 0, int(phase) != 1  # (p: the rest values; e: the emitters' rest values)
    return [
        ShadingNode(type=eShadingNode.Diffuse, base_color=(0.5, 0.5, 0.5) if p else (0.6, 0.55, 0.4), sheen=0.0 if p else 0.8, tint=0.0 if p else 0.3),
        ShadingNode(type=eShadingNode.Diffuse, base_color=(0.5, 0.0, 0.0) if p else (0.1, 0.2, 0.6)),
        ShadingNode(type=eShadingNode.Diffuse, base_color=(0.0, 0.5, 0.0) if p else (0.5, 0.45, 0.0)),
        ShadingNode(type=eShadingNode.Emissive, strength=100.0 if e else 55.0, base_color=(1.0, 1.0, 1.0) if e else (1.0, 0.7, 0.45), importance_sample=True),
        ShadingNode(type=eShadingNode.Glossy, base_color=(0.9, 0.9, 0.9) if p else (0.9, 0.6, 0.3), roughness=0.1 if p else 0.35,
                    anisotropic_rotation=0.0 if p else 0.25, tint=0.0 if p else 0.5),
        PrincipledMat(base_color=(0.8, 0.9, 1.0) if p else (1.0, 0.8, 0.8), transmission=0.7 if p else 0.35, roughness=0.05 if p else 0.2,
                      ior=1.45 if p else 1.6, transmission_roughness=0.0 if p else 0.1),
        ShadingNode(type=eShadingNode.Emissive, strength=1.5 if p else 4.0, base_color=(0.3, 0.5, 1.0) if p else (1.0, 0.4, 0.2)),  # no light
        ShadingNode(type=eShadingNode.Refractive, base_color=(1.0, 1.0, 1.0) if p else (0.8, 1.0, 0.9), ior=1.5 if p else 1.33, roughness=0.0 if p else 0.1),
        PrincipledMat(base_color=(0.6, 0.6, 0.6) if p else (0.3, 0.5, 0.7), roughness=0.4 if p else 0.7, metallic=0.0 if p else 0.6,
                      clearcoat=0.0 if p else 0.5, emission_color=(0.2, 0.9, 0.4) if e else (0.9, 0.3, 0.6), emission_strength=3.0 if e else 5.0,
                      importance_sample=True),
    ]


def cornell_materials(scene, phase=0):
    """a Cornell room with both blocks and eleven material slots (fewer than 48: the shade stage takes its LDS material table):
    Diffuse walls, the two-triangle lamp (Emissive, importance-sampled), the short block Glossy and a Principled that transmits, its top
    an Emissive that is NOT importance-sampled (no light), the tall block Refractive and a Principled that emits -- which the scene
    build turns into Principled + Emissive under an additive Mix: the emitter of its four triangle lights is found only through the
    Mix -- and a sphere light, so the light tree has an analytic leaf"""
    scene.SetEnvironment(env_col=(0.0, 0.0, 0.0))
    grey, red, green, lamp, gloss, glass, glow, refr, emitting = [scene.AddMaterial(d) for d in cornell_descs(phase)]
    attrs, idx = scenes.cornell_mesh_arrays()
    groups = [(grey, None, 0, 18), (red, None, 18, 6), (green, None, 24, 6), (lamp, 0xFFFFFFFF, 30, 6), (gloss, None, 36, 12), (glass, None, 48, 12),
              (glow, None, 60, 6), (refr, None, 66, 12), (emitting, None, 78, 12), (grey, None, 90, 6)]
    scene.AddMeshInstance(scene.AddMesh(attrs, idx, groups))
    scene.AddLight("sphere", color=(3.0, 2.5, 2.0), position=(-0.12, 0.42, -0.12), radius=0.02)
    scenes._cornell_camera(scene)
    scene.Finalize()


def field_descs(n, phase=0):
    """the materials of material_field: three for the room, then one per quad -- every fifth an importance-sampled emitter, the others
    Diffuse, Glossy, Principled (opaque) and Diffuse with sheen in turn, seeded; `phase` 1: other values everywhere; `phase` 2: other
    values everywhere but in the emitters"""
    rest, moved = np.random.RandomState(311), np.random.RandomState(312)
    out = [ShadingNode(type=eShadingNode.Diffuse, base_color=c) for c in ((0.5, 0.5, 0.5), (0.5, 0.0, 0.0), (0.0, 0.5, 0.0))]
    for k in range(n):
        draws = [(tuple(float(x) for x in rng.uniform(0.1, 0.9, size=3)), [float(x) for x in rng.uniform(0.0, 1.0, size=4)]) for rng in (rest, moved)]
        col, u = draws[0 if int(phase) == 0 or (int(phase) == 2 and k % 5 == 0) else 1]
        if k % 5 == 0:
            out.append(ShadingNode(type=eShadingNode.Emissive, base_color=col, strength=20.0 + 60.0 * u[0], importance_sample=True))
        elif k % 5 == 1:
            out.append(ShadingNode(type=eShadingNode.Diffuse, base_color=col))
        elif k % 5 == 2:
            out.append(ShadingNode(type=eShadingNode.Glossy, base_color=col, roughness=0.05 + 0.6 * u[0], anisotropic_rotation=u[1], tint=u[2]))
        elif k % 5 == 3:
            out.append(PrincipledMat(base_color=col, roughness=0.1 + 0.8 * u[0], metallic=u[1], specular=u[2], clearcoat=u[3], sheen=2.0 * u[0]))
        else:
            out.append(ShadingNode(type=eShadingNode.Diffuse, base_color=col, sheen=2.0 * u[0], tint=u[1]))
    return out


def material_field(scene, n, phase=0):
    """a Cornell room without its lamp and n small quads above its floor with a material each (n = 130: more than the 48 slots of the
    shade stage's LDS table, so the table is read from memory; a call that names every one has more than two wavefronts of entries).
    Nothing refracts: the passes leave the rays' ior plane alone."""
    scene.SetEnvironment(env_col=(0.0, 0.0, 0.0))
    mats = [scene.AddMaterial(d) for d in field_descs(n, phase)]
    attrs, idx = scenes.cornell_mesh_arrays(scenes._CORNELL_QUADS)
    scene.AddMeshInstance(scene.AddMesh(attrs, idx, [(mats[0], None, 0, 18), (mats[1], None, 18, 6), (mats[2], None, 24, 6), (mats[0], None, 30, 6)]))
    quads, cols = [], 13
    for k in range(n):
        x, z, y = -0.52 + 0.038 * (k % cols), -0.52 + 0.046 * (k // cols), 0.02 + 0.004 * (k % 7)
        s = 0.028
        quads.append((((x, y, z + s), (x + s, y, z + s), (x + s, y, z), (x, y, z)), (0.0, 1.0, 0.0), ((0.0, 1.0), (1.0, 1.0), (1.0, 0.0), (0.0, 0.0)), scenes._P_B))
    attrs, idx = scenes.cornell_mesh_arrays(quads)
    scene.AddMeshInstance(scene.AddMesh(attrs, idx, [(mats[3 + k], 0xFFFFFFFF if k % 5 == 0 else None, 6 * k, 6) for k in range(n)]))
    scenes._cornell_camera(scene)
    scene.Finalize()


class _Reglowed:
    """a scene whose AddMaterial gives the emissive sheet's `glow` material (Emissive, strength 4) another colour and strength"""

    def __init__(self, scene):
        self._scene = scene

    def __getattr__(self, name):
        return getattr(self._scene, name)

    def AddMaterial(self, desc):
        if isinstance(desc, ShadingNode) and desc.type == eShadingNode.Emissive and desc.strength == 4.0:
            desc = ShadingNode(type=eShadingNode.Emissive, strength=2.5, base_color=(0.4, 0.8, 0.9), importance_sample=True)
        return self._scene.AddMaterial(desc)


def sheet_renamed(scene, phase=0):
    """emissive_sheet of tests/light_refit_cases.py at its rest pose (578 triangle lights); `phase` 1: its `glow` material renamed"""
    L.emissive_sheet(_Reglowed(scene) if int(phase) else scene, 0.0)


def blob(name, phase=0, n=130):
    """the serialised scene "cornell_materials", "material_field" or "emissive_sheet" at `phase`, built once per process (needs the host
    library of the drop-in)"""
    from ray_amd import api
    key = ("materials", name, int(phase), n)
    if key not in L._blobs:
        s = api.CreateSceneHIP()
        if name == "cornell_materials":
            cornell_materials(s, phase)
        elif name == "material_field":
            material_field(s, n, phase)
        else:
            sheet_renamed(s, phase)
        L._blobs[key] = api.export_scene_blob(s)
    return L._blobs[key]


def descs(name, phase=0, n=130):
    return cornell_descs(phase) if name == "cornell_materials" else field_descs(n, phase)


def changed_slots(a: Arrays, moved: Arrays):
    """material slots in use whose record differs between the two phases, ascending"""
    used = a.used_materials()
    return np.array([m for m in range(len(a.materials)) if used[m] and a.materials[m].tobytes() != moved.materials[m].tobytes()], dtype=np.uint32)
