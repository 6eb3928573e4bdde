"""ctypes binding of include/rayhip.h -- the C-ABI of librayhip.so (hand-written HIP kernels for gfx950).

`Context` is a thin object over the rayhip_* entry points; it takes scenes as serialised blobs
(ray_amd/csrc/scene_blob.h) or as rayhip_scene_desc and returns numpy arrays.  There is no CPU path: creating a
Context without a GPU raises.  (`prefix`/`lib_path` exist so that tests can point the same wrapper at
tests/hostsim, the host-compiled copy of the kernel sources used to debug parity without a GPU.)
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
RAYHIP_LIB = os.path.join(_HERE, "csrc", "_build", "librayhip.so")

BUF_FINAL, BUF_RAW, BUF_BASE_COLOR, BUF_DEPTH_NORMALS, BUF_VARIANCE = 0, 1, 2, 3, 4
REDUCE_RADIANCE, REDUCE_BASE_COLOR, REDUCE_DEPTH_NORMALS, REDUCE_VARIANCE, REDUCE_ALL = 1, 2, 4, 8, 15
COMM_ID_BYTES = 128
FLAG_SORT_RAYS = 1 << 0
FLAG_COUNT_TRAVERSAL = 1 << 1
FLAG_TIME_STAGES = 1 << 2
FLAG_COUNT_WIDE = 1 << 3


class PassSettings(C.Structure):
    _fields_ = [
        ("max_diff_depth", C.c_uint8), ("max_spec_depth", C.c_uint8), ("max_refr_depth", C.c_uint8),
        ("max_transp_depth", C.c_uint8), ("max_total_depth", C.c_uint8), ("min_total_depth", C.c_uint8),
        ("min_transp_depth", C.c_uint8), ("flags", C.c_uint8),
        ("clamp_direct", C.c_float), ("clamp_indirect", C.c_float), ("min_samples", C.c_int32),
        ("variance_threshold", C.c_float), ("regularize_alpha", C.c_float),
    ]


class Camera(C.Structure):  # rayhip_camera == Ray::camera_t
    _fields_ = [
        ("type", C.c_uint8), ("filter", C.c_uint8), ("view_transform", C.c_uint8), ("ltype", C.c_uint8),
        ("filter_width", C.c_float),
        ("fov", C.c_float), ("exposure", C.c_float), ("gamma", C.c_float), ("sensor_height", C.c_float),
        ("focus_distance", C.c_float), ("focal_length", C.c_float), ("fstop", C.c_float),
        ("lens_rotation", C.c_float), ("lens_ratio", C.c_float),
        ("lens_blades", C.c_int32),
        ("clip_start", C.c_float), ("clip_end", C.c_float),
        ("origin", C.c_float * 3), ("fwd", C.c_float * 3), ("side", C.c_float * 3), ("up", C.c_float * 3),
        ("shift", C.c_float * 2),
        ("mi_index", C.c_uint32), ("uv_index", C.c_uint32),
        ("pass_settings", PassSettings),
    ]


class Stats(C.Structure):
    _fields_ = [("t", C.c_ulonglong * 11)]
    NAMES = ("primary_ray_gen", "primary_trace", "primary_shade", "primary_shadow", "secondary_sort",
             "secondary_trace", "secondary_shade", "secondary_shadow", "denoise", "cache_update", "cache_resolve")

    def as_dict(self):
        return {n: int(self.t[i]) for i, n in enumerate(self.NAMES)}


class TravCounters(C.Structure):
    _fields_ = [("rays", C.c_ulonglong), ("nodes", C.c_ulonglong), ("tris", C.c_ulonglong), ("instances", C.c_ulonglong),
                ("max_stack", C.c_ulonglong), ("nodes4", C.c_ulonglong)]

    def as_dict(self):
        return {"rays": int(self.rays), "nodes": int(self.nodes), "tris": int(self.tris), "instances": int(self.instances),
                "max_stack": int(self.max_stack), "nodes4": int(self.nodes4)}


class CacheGrid(C.Structure):  # rayhip_cache_grid == Ray::cache_grid_params_t
    _fields_ = [("cam_pos_curr", C.c_float * 3), ("cam_pos_prev", C.c_float * 3), ("log_base", C.c_float), ("scale", C.c_float),
                ("exposure", C.c_float)]

    @classmethod
    def make(cls, cam_pos, exposure=1.0, cam_pos_prev=(0.0, 0.0, 0.0)):
        return cls((C.c_float * 3)(*cam_pos), (C.c_float * 3)(*cam_pos_prev), 2.0, 50.0, exposure)


class SkinDesc(C.Structure):  # rayhip_skin_desc
    _fields_ = [("first_vertex", C.c_uint32), ("count", C.c_uint32), ("rest", C.c_void_p), ("bone_indices", C.c_void_p), ("bone_weights", C.c_void_p),
                ("bones_count", C.c_uint32)]


class MorphTarget(C.Structure):  # rayhip_morph_target
    _fields_ = [("count", C.c_uint32), ("vertices", C.c_void_p), ("dp", C.c_void_p), ("dn", C.c_void_p), ("db", C.c_void_p)]


class MorphDesc(C.Structure):  # rayhip_morph_desc
    _fields_ = [("first_vertex", C.c_uint32), ("count", C.c_uint32), ("base", C.c_void_p), ("targets_count", C.c_uint32),
                ("targets", C.POINTER(MorphTarget))]


class NormalsDesc(C.Structure):  # rayhip_normals_desc
    _fields_ = [("first_vertex", C.c_uint32), ("count", C.c_uint32), ("flags", C.c_uint32), ("weld", C.c_void_p)]


NORMALS_N, NORMALS_B = 1, 2  # RAYHIP_NORMALS_N / _B

CACHE_ENTRIES = 1 << 22  # slots of the spatial cache's key table (rt_cache.h)
# rayhip_cache_vertex: one vertex of a cache-update bounce
CACHE_VERTEX_DTYPE = np.dtype([("o", "<f4", 3), ("t", "<f4"), ("d", "<f4", 3), ("path", "<u4"), ("n", "<f4", 3), ("ends", "<u4"),
                               ("radiance", "<f4", 3), ("_pad0", "<f4"), ("c", "<f4", 3), ("_pad1", "<f4")])
assert CACHE_VERTEX_DTYPE.itemsize == 80

RAY_DTYPE = np.dtype([("o", "<f4", 3), ("d", "<f4", 3), ("pdf", "<f4"), ("c", "<f4", 3), ("ior", "<f4", 4),
                      ("cone_width", "<f4"), ("cone_spread", "<f4"), ("xy", "<u4"), ("depth", "<u4")])
SHADOW_RAY_DTYPE = np.dtype([("o", "<f4", 3), ("depth", "<u4"), ("d", "<f4", 3), ("dist", "<f4"), ("c", "<f4", 3),
                             ("xy", "<u4")])
HIT_DTYPE = np.dtype([("obj_index", "<i4"), ("prim_index", "<i4"), ("t", "<f4"), ("u", "<f4"), ("v", "<f4")])
assert RAY_DTYPE.itemsize == 72 and SHADOW_RAY_DTYPE.itemsize == 48 and HIT_DTYPE.itemsize == 20
VERTEX_DTYPE = np.dtype([("p", "<f4", 3), ("n", "<f4", 3), ("b", "<f4", 3), ("t", "<f4", 2)])  # rayhip_vertex
assert VERTEX_DTYPE.itemsize == 44
LIGHT_NODE_DTYPE = np.dtype([("bbox_min", "<f4", 3), ("_unused0", "<f4"), ("bbox_max", "<f4", 3), ("_unused1", "<f4"), ("ch_bbox_min", "u1", (3, 8)),
                             ("ch_bbox_max", "u1", (3, 8)), ("child", "<u4", 8), ("flux", "<f4", 8), ("axis", "<u4", 8),
                             ("cos_omega_ne", "<u4", 8)])  # rayhip_light_cwbvh_node
assert LIGHT_NODE_DTYPE.itemsize == 208
MESH_INSTANCE_DTYPE = np.dtype([("mesh_index", "<u4"), ("node_index", "<u4"), ("lights_index", "<u4"), ("ray_visibility", "<u4"),
                                ("xform", "<f4", 16), ("inv_xform", "<f4", 16)])  # rayhip_mesh_instance
assert MESH_INSTANCE_DTYPE.itemsize == 144
MATERIAL_DTYPE = np.dtype([("textures", "<u4", 5), ("base_color", "<f4", 3), ("flags", "<u4"), ("type", "<u4"), ("tangent_rotation_or_strength", "<f4"),
                           ("roughness_unorm", "<u2"), ("anisotropic_unorm", "<u2"), ("ior", "<f4"), ("sheen_unorm", "<u2"), ("sheen_tint_unorm", "<u2"),
                           ("tint_unorm", "<u2"), ("metallic_unorm", "<u2"), ("transmission_unorm", "<u2"), ("transmission_roughness_unorm", "<u2"),
                           ("specular_unorm", "<u2"), ("specular_tint_unorm", "<u2"), ("clearcoat_unorm", "<u2"), ("clearcoat_roughness_unorm", "<u2"),
                           ("normal_map_strength_unorm", "<u2"), ("_pad", "<u2")])  # rayhip_material
assert MATERIAL_DTYPE.itemsize == 76

# every symbol include/rayhip.h declares (tests check that the built library exports all of them)
ENTRY_POINTS = (
    "last_error", "abi_version", "device_count", "ctx_create", "ctx_destroy", "ctx_device_name", "upload_static", "resize", "clear",
    "scene_upload", "bake_sky", "bake_sky_blob", "scene_bvh_width", "closest_hit_form", "direct_entry", "scene_upload_blob", "scene_update_instances", "scene_update_instances_blob", "scene_update_vertices", "scene_update_vertices_blob", "scene_update_vertices_device", "skin_create", "skin_destroy", "scene_pose_skins", "morph_create", "morph_destroy", "scene_pose", "normals_create", "normals_destroy", "scene_refit_lights", "scene_set_instance_transforms", "scene_set_instance_transforms_device", "scene_set_lights", "scene_set_lights_device", "scene_set_materials", "scene_set_materials_device", "scene_set_environment", "scene_set_env_map", "scene_set_env_map_device", "scene_set_sky", "scene_set_texture", "scene_set_texture_device", "scene_set_texture_blocks", "set_filter_table", "render", "render_batch", "max_batch", "reserve_batch", "set_tonemap_lut", "denoise_nlm", "readback", "readback_device", "set_raw_device",
    "sync", "set_shard", "get_trav_counters", "get_trav_timing", "get_stage_times", "k_generate_primary_rays", "k_intersect_closest",
    "k_intersect_shadow", "k_scrambled_rand", "k_shade",
    "comm_create", "comm_probe", "comm_info", "comm_unique_id", "comm_create_rank", "comm_bind", "comm_reduce_framebuffers", "comm_destroy",
    "unet_init", "denoise_unet", "unet_set_precision", "unet_read_tensor",
    "export_shard_device", "owned_bytes", "export_owned", "import_owned", "finish_import",
    "cache_enable", "cache_resolve", "cache_reset", "cache_readback", "k_cache_begin_paths", "k_cache_update_vertices", "k_cache_query",
    "k_lbvh_build", "k_bvh4_collapse", "k_bvh4_test_nodes", "k_read_accel",
)


def _aligned_copy(buf: bytes, align: int = 64) -> np.ndarray:
    raw = np.empty(len(buf) + align, dtype=np.uint8)
    off = (-raw.ctypes.data) % align
    out = raw[off:off + len(buf)]
    out[:] = np.frombuffer(buf, dtype=np.uint8)
    return out


def weld_by_position(positions) -> np.ndarray:
    """uint32 [count]: per vertex the lowest index among the vertices whose position is bytewise equal to its own -- the `weld` of
    Context.create_normals for a range whose smoothing groups are its coincident vertices (the twins a scene build appends when it
    derives bitangents are such)"""
    p = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
    if len(p) == 0:
        return np.zeros(0, dtype=np.uint32)
    keys = p.view(np.uint32)
    order = np.lexsort((np.arange(len(p)), keys[:, 2], keys[:, 1], keys[:, 0]))  # equal keys together, ascending index within them
    sorted_keys = keys[order]
    starts = np.r_[True, np.any(sorted_keys[1:] != sorted_keys[:-1], axis=1)]
    lowest = order[np.flatnonzero(starts)][np.cumsum(starts) - 1]
    out = np.empty(len(p), dtype=np.uint32)
    out[order] = lowest
    return out


class Library:
    def __init__(self, lib_path: str = RAYHIP_LIB, prefix: str = "rayhip_"):
        if not os.path.exists(lib_path):
            raise RuntimeError(f"{lib_path} is not built; run `python -c 'import __graft_entry__ as g; g.build()'`")
        self.lib = C.CDLL(lib_path)
        self.prefix = prefix
        vp = C.c_void_p
        f = self.fn
        f("last_error").restype = C.c_char_p
        f("ctx_create").argtypes = [C.c_int, C.POINTER(vp)]
        f("ctx_destroy").argtypes = [vp]
        f("ctx_destroy").restype = None
        f("ctx_device_name").argtypes = [vp, C.c_char_p, C.c_int]
        f("upload_static").argtypes = [vp, vp, C.c_uint32]
        f("resize").argtypes = [vp, C.c_int, C.c_int]
        f("clear").argtypes = [vp, C.POINTER(C.c_float * 4)]
        f("scene_upload_blob").argtypes = [vp, vp, C.c_size_t, C.POINTER(Camera)]
        f("set_filter_table").argtypes = [vp, vp, C.c_int]
        if prefix == "rayhip_":
            f("bake_sky_blob").argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_int, vp]
        else:
            f("bake_sky").argtypes = [vp, C.c_int, C.c_int, vp]
            f("env_map_texels").argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_int * 2)]
        f("render").argtypes = [vp, C.POINTER(Camera), C.POINTER(C.c_int * 4), C.c_int, C.c_uint32, C.POINTER(Stats)]
        f("render_batch").argtypes = [vp, C.POINTER(Camera), C.POINTER(C.c_int * 4), C.c_int, C.c_int, C.c_uint32, C.POINTER(Stats)]
        f("max_batch").argtypes = [vp]
        f("scene_bvh_width").argtypes = [vp]
        if prefix == "rayhip_":
            f("closest_hit_form").argtypes = [vp]
            f("direct_entry").argtypes = [vp]
        f("reserve_batch").argtypes = [vp, C.c_int]
        f("set_tonemap_lut").argtypes = [vp, C.c_int, vp, C.c_int]
        f("denoise_nlm").argtypes = [vp, C.POINTER(Camera), C.POINTER(C.c_int * 4), C.c_int]
        f("readback").argtypes = [vp, C.c_int, vp, C.c_int]
        f("sync").argtypes = [vp]
        f("set_shard").argtypes = [vp, C.c_int, C.c_int, C.c_int]
        f("get_trav_counters").argtypes = [vp, C.POINTER(TravCounters * 2), C.c_int]
        f("k_generate_primary_rays").argtypes = [vp, C.POINTER(Camera), C.POINTER(C.c_int * 4), C.c_int, vp, vp, C.POINTER(C.c_int)]
        f("k_intersect_closest").argtypes = [vp, C.POINTER(Camera), vp, vp, C.c_int, C.c_int, C.c_uint32, C.POINTER(TravCounters)]
        f("k_intersect_shadow").argtypes = [vp, C.POINTER(Camera), vp, C.c_int, C.c_int, vp, C.POINTER(TravCounters)]
        f("k_scrambled_rand").argtypes = [vp, vp, vp, vp, C.c_int, vp]
        f("k_shade").argtypes = [vp, C.POINTER(Camera), C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, C.POINTER(C.c_int), vp,
                                 C.POINTER(C.c_int)]
        f("scene_update_instances_blob").argtypes = [vp, vp, C.c_size_t, C.POINTER(Camera)]
        f("owned_bytes").argtypes = [vp, C.c_uint32, C.c_int, C.c_int]
        f("owned_bytes").restype = C.c_size_t
        f("export_owned").argtypes = [vp, C.c_uint32, vp, C.c_size_t]
        f("import_owned").argtypes = [vp, C.c_uint32, C.c_int, vp, C.c_size_t]
        f("finish_import").argtypes = [vp, C.POINTER(Camera)]
        if prefix == "rayhip_":
            f("unet_init").argtypes = [vp, vp, C.c_int, vp, C.c_int]
            f("denoise_unet").argtypes = [vp, C.POINTER(Camera), C.POINTER(C.c_int * 4), C.c_int]
            f("unet_read_tensor").argtypes = [vp, C.c_int, vp, C.c_size_t, C.POINTER(C.c_int * 3)]
            f("unet_set_precision").argtypes = [vp, C.c_int]
            f("readback_device").argtypes = [vp, C.c_int, vp, C.c_int]
            f("set_raw_device").argtypes = [vp, vp, C.c_int, C.POINTER(Camera)]
            f("export_shard_device").argtypes = [vp, C.c_int, vp]
            f("comm_create").argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(vp)]
            f("comm_unique_id").argtypes = [vp, C.c_size_t]
            f("comm_probe").argtypes = []
            f("comm_info").argtypes = [vp, C.POINTER(C.c_int * 4)]
            f("comm_create_rank").argtypes = [vp, C.c_int, C.c_int, vp, C.POINTER(vp)]
            f("comm_bind").argtypes = [vp, C.c_int, vp]
            f("comm_reduce_framebuffers").argtypes = [vp, C.c_int, C.c_uint32, C.POINTER(Camera)]
            f("comm_destroy").argtypes = [vp]
            f("comm_destroy").restype = None
            f("get_trav_timing").argtypes = [vp, C.POINTER(C.c_double * 2), C.POINTER(C.c_ulonglong * 2), C.c_int]
            f("get_stage_times").argtypes = [vp, C.POINTER(Stats), C.c_int]
            f("cache_enable").argtypes = [vp, C.c_int]
            f("cache_resolve").argtypes = [vp, C.POINTER(Camera)]
            f("cache_reset").argtypes = [vp]
            f("cache_readback").argtypes = [vp, vp, vp, C.c_int, C.c_uint32]
            f("k_cache_begin_paths").argtypes = [vp, C.c_int]
            f("k_cache_update_vertices").argtypes = [vp, C.POINTER(CacheGrid), vp, C.c_int]
            f("k_cache_query").argtypes = [vp, C.POINTER(CacheGrid), vp, C.c_int, vp]
            u32 = C.c_uint32
            f("k_lbvh_build").argtypes = [vp, vp, vp, u32, u32, u32, C.c_int, C.c_int, C.c_int, vp, u32, vp, u32, vp, vp, vp]
            f("k_bvh4_collapse").argtypes = [vp, vp, u32, vp, u32, vp, vp, vp]
            f("k_bvh4_test_nodes").argtypes = [vp, vp, u32, vp, vp, vp, vp, u32, vp, vp, vp]
            f("scene_update_vertices").argtypes = [vp, u32, u32, vp]
            f("scene_update_vertices_blob").argtypes = [vp, vp, C.c_size_t]
            f("k_read_accel").argtypes = [vp, C.c_int, vp, C.c_size_t, C.POINTER(C.c_size_t)]
            f("scene_update_vertices_device").argtypes = [vp, u32, u32, vp]
            f("skin_create").argtypes = [vp, C.POINTER(SkinDesc), C.POINTER(C.c_int)]
            f("skin_destroy").argtypes = [vp, C.c_int]
            f("scene_pose_skins").argtypes = [vp, C.c_int, C.POINTER(C.c_int), C.POINTER(vp)]
            f("morph_create").argtypes = [vp, C.POINTER(MorphDesc), C.POINTER(C.c_int)]
            f("morph_destroy").argtypes = [vp, C.c_int]
            f("scene_pose").argtypes = [vp, C.c_int, C.POINTER(C.c_int), C.POINTER(vp), C.c_int, C.POINTER(C.c_int), C.POINTER(vp)]
            f("normals_create").argtypes = [vp, C.POINTER(NormalsDesc), C.POINTER(C.c_int)]
            f("normals_destroy").argtypes = [vp, C.c_int]
            f("scene_refit_lights").argtypes = [vp, C.c_int]
            f("scene_set_instance_transforms").argtypes = [vp, u32, vp, vp]
            f("scene_set_instance_transforms_device").argtypes = [vp, u32, vp, vp]
            f("scene_set_lights").argtypes = [vp, u32, vp, vp]
            f("scene_set_lights_device").argtypes = [vp, u32, vp, vp]
            f("scene_set_materials").argtypes = [vp, u32, vp, vp]
            f("scene_set_materials_device").argtypes = [vp, u32, vp, vp]
            f("scene_set_environment").argtypes = [vp, vp, vp, C.c_float, C.c_float]
            f("scene_set_env_map").argtypes = [vp, C.c_int, C.c_int, vp]
            f("scene_set_env_map_device").argtypes = [vp, C.c_int, C.c_int, vp]
            f("scene_set_sky").argtypes = [vp, u32, vp, vp, vp, vp, vp]
            f("scene_set_texture").argtypes = [vp, u32, C.c_int, C.c_int, vp]
            f("scene_set_texture_device").argtypes = [vp, u32, C.c_int, C.c_int, vp]
            f("scene_set_texture_blocks").argtypes = [vp, u32, vp, C.c_size_t]

    def fn(self, name):
        return getattr(self.lib, self.prefix + name)

    def device_count(self) -> int:
        return int(self.fn("device_count")())

    def abi_version(self) -> int:
        """RAYHIP_ABI_VERSION of the header the library was built from (include/rayhip.h)"""
        return int(self.fn("abi_version")())

    def check(self, status: int):
        if status != 0:
            raise RuntimeError(f"{self.prefix}*: " + self.fn("last_error")().decode())


class Context:
    """One rayhip context = one GPU (rayhip.h).  Mirrors what RendererHIP holds on the C++ side."""

    def __init__(self, device: int = 0, library: Library = None):
        self.L = library or Library()
        self._ctx = C.c_void_p()
        self.L.check(self.L.fn("ctx_create")(device, C.byref(self._ctx)))
        self.w = self.h = 0
        self.cam = None
        self._blob = None

    def close(self):
        if self._ctx:
            self.L.fn("ctx_destroy")(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def device_name(self) -> str:
        buf = C.create_string_buffer(256)
        self.L.check(self.L.fn("ctx_device_name")(self._ctx, buf, 256))
        return buf.value.decode()

    def upload_static(self, pmj: np.ndarray):
        pmj = np.ascontiguousarray(pmj, dtype=np.uint32)
        self.L.check(self.L.fn("upload_static")(self._ctx, pmj.ctypes.data, pmj.size))

    def resize(self, w: int, h: int):
        self.L.check(self.L.fn("resize")(self._ctx, w, h))
        self.w, self.h = w, h

    def clear(self, rgba=(0.0, 0.0, 0.0, 0.0)):
        v = (C.c_float * 4)(*rgba)
        self.L.check(self.L.fn("clear")(self._ctx, C.byref(v)))

    def upload_scene_blob(self, blob: bytes) -> Camera:
        self._blob = _aligned_copy(blob)
        cam = Camera()
        self.L.check(self.L.fn("scene_upload_blob")(self._ctx, self._blob.ctypes.data, self._blob.size, C.byref(cam)))
        self.cam = cam
        return cam

    def bake_sky(self, w: int, h: int, blob: bytes = None) -> np.ndarray:
        """the sky environment map ([h, w, 4] uint8: shared-exponent RGBE) of a physical-sky scene: on the device from `blob` (default: the blob
        this context uploaded last) -- rayhip_bake_sky_blob; with the host build of the kernels, from the uploaded scene"""
        out = np.zeros((h, w), dtype=np.uint32)
        if self.L.prefix == "rayhip_":
            b = self._blob if blob is None else _aligned_copy(blob)
            self.L.check(self.L.fn("bake_sky_blob")(self._ctx, b.ctypes.data, b.size, w, h, out.ctypes.data))
        else:
            self.L.check(self.L.fn("bake_sky")(self._ctx, w, h, out.ctypes.data))
        return out.view(np.uint8).reshape(h, w, 4)

    def env_map_texels(self) -> np.ndarray:
        """(host build only) the texels of the environment map the uploaded scene came with, [h, w, 4] uint8"""
        buf = np.zeros(4096 * 2048, dtype=np.uint32)
        wh = (C.c_int * 2)()
        self.L.check(self.L.fn("env_map_texels")(self._ctx, buf.ctypes.data, buf.size, C.byref(wh)))
        return buf[:wh[0] * wh[1]].view(np.uint8).reshape(wh[1], wh[0], 4).copy()

    def update_instances(self, blob: bytes) -> int:
        """instances / lights / environment of `blob` over the geometry that is on the device; the top level is rebuilt
        there (rayhip_scene_update_instances).  Returns 0, or 2 if the change needs a full upload_scene()."""
        self._blob2 = _aligned_copy(blob)
        cam = Camera()
        rc = self.L.fn("scene_update_instances_blob")(self._ctx, self._blob2.ctypes.data, self._blob2.size, C.byref(cam))
        if rc == 2:
            return 2
        self.L.check(rc)
        self.cam = cam
        return 0

    def update_vertices(self, first: int, array: np.ndarray) -> int:
        """new vertices [first, first + len(array)) of the uploaded scene (VERTEX_DTYPE records, or [n][11] float32: position, normal,
        bitangent, uv); the trees are refitted on the device (rayhip_scene_update_vertices).  Returns 0, or 2 if the change needs a
        full upload_scene_blob(); an error raises."""
        array = np.ascontiguousarray(array)
        if array.dtype != VERTEX_DTYPE:
            array = np.ascontiguousarray(array, dtype=np.float32).reshape(-1, 11)
        rc = self.L.fn("scene_update_vertices")(self._ctx, int(first), len(array), array.ctypes.data)
        if rc == 2:
            return 2
        self.L.check(rc)
        return 0

    def update_vertices_blob(self, blob: bytes) -> int:
        """the vertex array of `blob`, a scene of the topology that is on the device (rayhip_scene_update_vertices_blob); returns as
        update_vertices()"""
        b = blob if isinstance(blob, np.ndarray) else _aligned_copy(blob)  # (an array: uint8, 16-byte aligned -- a caller that sends a scene repeatedly)
        assert b.dtype == np.uint8 and b.ctypes.data % 16 == 0
        rc = self.L.fn("scene_update_vertices_blob")(self._ctx, b.ctypes.data, b.size)
        if rc == 2:
            return 2
        self.L.check(rc)
        return 0

    def update_vertices_device(self, first: int, count: int, device_pointer: int) -> int:
        """new vertices [first, first + count) from `count` 44-byte records that are on this context's device already: `device_pointer`
        is their address as an int (a tensor's data_ptr(), say), the data complete when the call is made
        (rayhip_scene_update_vertices_device); returns as update_vertices()"""
        rc = self.L.fn("scene_update_vertices_device")(self._ctx, int(first), int(count), C.c_void_p(int(device_pointer)))
        if rc == 2:
            return 2
        self.L.check(rc)
        return 0

    def create_skin(self, first: int, rest, indices: np.ndarray, weights: np.ndarray, bones_count: int) -> int:
        """a skin over vertices [first, first + len(indices)) (rayhip_skin_create): `rest` VERTEX_DTYPE records or None (what the device
        holds for the range now), `indices` [n][4] uint16, `weights` [n][4] float32.  Returns the skin's id (16 or more), or 2 where the ABI returns 2
        (the context needs a full upload, or the range holds a vertex of a triangle light); an error raises."""
        indices = np.ascontiguousarray(indices, dtype=np.uint16).reshape(-1, 4)
        weights = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1, 4)
        assert len(indices) == len(weights)
        if rest is not None:
            rest = np.ascontiguousarray(rest)
            assert rest.dtype == VERTEX_DTYPE and len(rest) == len(indices)
        d = SkinDesc(int(first), len(indices), rest.ctypes.data if rest is not None else None, indices.ctypes.data, weights.ctypes.data, int(bones_count))
        out = C.c_int(-1)
        rc = self.L.fn("skin_create")(self._ctx, C.byref(d), C.byref(out))
        if rc == 2:
            return 2
        self.L.check(rc)
        return int(out.value)

    def destroy_skin(self, skin: int) -> int:
        rc = self.L.fn("skin_destroy")(self._ctx, int(skin))
        if rc == 2:
            return 2
        self.L.check(rc)
        return 0

    def pose_skins(self, palettes: dict) -> int:
        """{skin id: palette [bones][3][4] float32}: every named skin posed from its rest pose and ONE refit (rayhip_scene_pose_skins);
        returns as update_vertices()"""
        ids = list(palettes)
        arrays = [np.ascontiguousarray(palettes[k], dtype=np.float32) for k in ids]
        assert all(a.ndim == 3 and a.shape[1:] == (3, 4) for a in arrays)
        c_ids = (C.c_int * max(len(ids), 1))(*ids)
        c_ptrs = (C.c_void_p * max(len(ids), 1))(*[a.ctypes.data for a in arrays])
        rc = self.L.fn("scene_pose_skins")(self._ctx, len(ids), c_ids, c_ptrs)
        if rc == 2:
            return 2
        self.L.check(rc)
        return 0

    def create_morph(self, first: int, count: int, base, targets) -> int:
        """a morph set over vertices [first, first + count) (rayhip_morph_create): `base` VERTEX_DTYPE records or None (what the device
        holds for the range now), `targets` a list of (vertices, dp, dn or None, db or None) -- indices relative to `first`, strictly
        ascending, and [n][3] float32 deltas.  Returns the set's id (16 or more), or 2 where the ABI returns 2; an error raises."""
        if base is not None:
            base = np.ascontiguousarray(base)
            assert base.dtype == VERTEX_DTYPE and len(base) == count
        keep = []  # the arrays the description points into

        def ptr(a, dtype, shape):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dtype).reshape(shape)
            keep.append(a)
            return a.ctypes.data

        c_targets = (MorphTarget * max(len(targets), 1))()
        for k, (vertices, dp, dn, db) in enumerate(targets):
            n = len(vertices)
            c_targets[k] = MorphTarget(n, ptr(vertices, np.uint32, (n,)), ptr(dp, np.float32, (n, 3)), ptr(dn, np.float32, (n, 3)),
                                       ptr(db, np.float32, (n, 3)))
        d = MorphDesc(int(first), int(count), base.ctypes.data if base is not None else None, len(targets), c_targets)
        out = C.c_int(-1)
        rc = self.L.fn("morph_create")(self._ctx, C.byref(d), C.byref(out))
        if rc == 2:
            return 2
        self.L.check(rc)
        return int(out.value)

    def destroy_morph(self, morph: int) -> int:
        rc = self.L.fn("morph_destroy")(self._ctx, int(morph))
        if rc == 2:
            return 2
        self.L.check(rc)
        return 0

    def pose(self, morph_weights: dict, palettes: dict) -> int:
        """{morph set id: weights [targets] float32} and {skin id: palette [bones][3][4] float32}: every named set and skin posed from its
        base / rest records -- morph, then skin, where a skin holds a set -- and ONE refit (rayhip_scene_pose); returns as pose_skins()"""
        m_ids, k_ids = list(morph_weights), list(palettes)
        w = [np.ascontiguousarray(morph_weights[k], dtype=np.float32).ravel() for k in m_ids]
        p = [np.ascontiguousarray(palettes[k], dtype=np.float32) for k in k_ids]
        assert all(a.ndim == 3 and a.shape[1:] == (3, 4) for a in p)
        c_m = (C.c_int * max(len(m_ids), 1))(*m_ids)
        c_w = (C.c_void_p * max(len(m_ids), 1))(*[a.ctypes.data for a in w])
        c_k = (C.c_int * max(len(k_ids), 1))(*k_ids)
        c_p = (C.c_void_p * max(len(k_ids), 1))(*[a.ctypes.data for a in p])
        rc = self.L.fn("scene_pose")(self._ctx, len(m_ids), c_m, c_w, len(k_ids), c_k, c_p)
        if rc == 2:
            return 2
        self.L.check(rc)
        return 0

    def create_normals(self, first: int, count: int, normals: bool = True, bitangents: bool = True, weld=None) -> int:
        """a normal set over vertices [first, first + count) (rayhip_normals_create): while it is live, every vertex update and pose
        recomputes the normals and / or bitangents of the range on the device from the positions then in the vertex array.  `weld`: None,
        or [count] uint32 relative to `first`, the canonical vertex of each vertex's smoothing group (weld_by_position).  Returns the
        set's id (16 or more), or 2 where the ABI returns 2; an error raises."""
        if weld is not None:
            weld = np.ascontiguousarray(weld, dtype=np.uint32)
            assert weld.shape == (count,)
        d = NormalsDesc(int(first), int(count), (NORMALS_N if normals else 0) | (NORMALS_B if bitangents else 0), weld.ctypes.data if weld is not None else None)
        out = C.c_int(-1)
        rc = self.L.fn("normals_create")(self._ctx, C.byref(d), C.byref(out))
        if rc == 2:
            return 2
        self.L.check(rc)
        return int(out.value)

    def destroy_normals(self, handle: int) -> int:
        rc = self.L.fn("normals_destroy")(self._ctx, int(handle))
        if rc == 2:
            return 2
        self.L.check(rc)
        return 0

    def refit_lights(self, on: bool) -> int:
        """the switch rayhip_scene_refit_lights: with it on, vertex updates and poses may move the vertices of triangle lights -- their
        corners, the light tree and its importance rows are refitted on the device behind the geometry.  Returns 0; turning it off under
        a live skin that covers a vertex of a triangle light raises."""
        self.L.check(self.L.fn("scene_refit_lights")(self._ctx, 1 if on else 0))
        return 0

    def set_instance_transforms(self, slots, xforms) -> int:
        """new transforms for the instance slots `slots` of the uploaded scene: `xforms` [n][16] float32 in the layout of
        rayhip_mesh_instance::xform; inverses, world boxes and the top level follow on the device
        (rayhip_scene_set_instance_transforms).  Returns as update_vertices(): 0, or 2 where the ABI returns 2; an error raises."""
        slots = np.ascontiguousarray(slots, dtype=np.uint32).ravel()
        xforms = np.ascontiguousarray(xforms, dtype=np.float32).reshape(-1, 16)
        assert len(slots) == len(xforms)
        rc = self.L.fn("scene_set_instance_transforms")(self._ctx, len(slots), slots.ctypes.data, xforms.ctypes.data)
        if rc == 2:
            return 2
        self.L.check(rc)
        return 0

    def set_instance_transforms_device(self, n: int, slots_pointer: int, xforms_pointer: int) -> int:
        """the same from `n` uint32 slots and `n` x 16 float32 that are on this context's device already: their addresses as ints (a
        tensor's data_ptr(), say), the data complete when the call is made (rayhip_scene_set_instance_transforms_device)"""
        rc = self.L.fn("scene_set_instance_transforms_device")(self._ctx, int(n), C.c_void_p(int(slots_pointer)), C.c_void_p(int(xforms_pointer)))
        if rc == 2:
            return 2
        self.L.check(rc)
        return 0

    def set_lights(self, slots, records) -> int:
        """new records for the light slots `slots` of the uploaded scene: `records` [n][16] 32-bit words, complete rayhip_light records
        whose word 0 is the one the slot holds; sphere, spot, directional, line, rect and disk lights.  The leaf summaries and the light
        tree follow on the device (rayhip_scene_set_lights; needs refit_lights(True)).  Returns as update_vertices(): 0, or 2 where the
        ABI returns 2; an error raises."""
        slots = np.ascontiguousarray(slots, dtype=np.uint32).ravel()
        records = np.ascontiguousarray(records)
        records = (records if records.dtype == np.uint32 else records.view(np.uint32)).reshape(-1, 16)
        assert len(slots) == len(records)
        rc = self.L.fn("scene_set_lights")(self._ctx, len(slots), slots.ctypes.data, records.ctypes.data)
        if rc == 2:
            return 2
        self.L.check(rc)
        return 0

    def set_lights_device(self, n: int, slots_pointer: int, records_pointer: int) -> int:
        """the same from `n` uint32 slots and `n` 64-byte records that are on this context's device already: their addresses as ints (a
        tensor's data_ptr(), say), the data complete when the call is made (rayhip_scene_set_lights_device)"""
        rc = self.L.fn("scene_set_lights_device")(self._ctx, int(n), C.c_void_p(int(slots_pointer)), C.c_void_p(int(records_pointer)))
        if rc == 2:
            return 2
        self.L.check(rc)
        return 0

    def set_materials(self, slots, records) -> int:
        """new records for the material slots `slots` of the uploaded scene: `records` [n] MATERIAL_DTYPE (or [n][19] 32-bit words),
        complete rayhip_material records whose textures, flags and type are the ones the slot holds.  The triangle lights a named
        material colours and the light tree follow on the device (rayhip_scene_set_materials; recolouring an emitter needs
        refit_lights(True)).  Returns as update_vertices(): 0, or 2 where the ABI returns 2; an error raises."""
        slots = np.ascontiguousarray(slots, dtype=np.uint32).ravel()
        records = np.ascontiguousarray(records)
        records = (records if records.dtype == np.uint32 else records.view(np.uint32)).reshape(-1, 19)
        assert len(slots) == len(records)
        rc = self.L.fn("scene_set_materials")(self._ctx, len(slots), slots.ctypes.data, records.ctypes.data)
        if rc == 2:
            return 2
        self.L.check(rc)
        return 0

    def set_materials_device(self, n: int, slots_pointer: int, records_pointer: int) -> int:
        """the same from `n` uint32 slots and `n` 76-byte records that are on this context's device already: their addresses as ints (a
        tensor's data_ptr(), say), 4-byte aligned, the data complete when the call is made (rayhip_scene_set_materials_device)"""
        rc = self.L.fn("scene_set_materials_device")(self._ctx, int(n), C.c_void_p(int(slots_pointer)), C.c_void_p(int(records_pointer)))
        if rc == 2:
            return 2
        self.L.check(rc)
        return 0

    def _changed(self, rc: int) -> int:
        if rc == 2:
            return 2
        self.L.check(rc)
        return 0

    def set_environment(self, env_col, back_col, env_map_rotation: float, back_map_rotation: float) -> int:
        """new colours and rotations of the environment; no texel changes, no quadtree (rayhip_scene_set_environment).  Returns as
        update_vertices(): 0, or 2 where the ABI returns 2; an error raises."""
        e, b = np.ascontiguousarray(env_col, dtype=np.float32), np.ascontiguousarray(back_col, dtype=np.float32)
        assert e.size == 3 and b.size == 3
        return self._changed(self.L.fn("scene_set_environment")(self._ctx, e.ctypes.data, b.ctypes.data, float(env_map_rotation), float(back_map_rotation)))

    def set_env_map(self, rgbe8) -> int:
        """new texels for the environment map the scene holds: `rgbe8` [h][w] uint32 (or [h][w][4] uint8) RGBE8 of the held map's size.
        Quadtree, the environment light's flux and the light tree follow on the device (rayhip_scene_set_env_map; a scene with an
        environment light needs refit_lights(True)).  Returns as set_environment()."""
        t = np.ascontiguousarray(rgbe8)
        t = t.view(np.uint32).reshape(t.shape[0], t.shape[1]) if t.dtype == np.uint8 else np.ascontiguousarray(t, dtype=np.uint32)
        assert t.ndim == 2
        return self._changed(self.L.fn("scene_set_env_map")(self._ctx, t.shape[1], t.shape[0], t.ctypes.data))

    def set_env_map_device(self, w: int, h: int, texels_pointer: int) -> int:
        """the same from w x h uint32 that are on this context's device already: their address as an int (a tensor's data_ptr(), say),
        4-byte aligned, the data complete when the call is made (rayhip_scene_set_env_map_device)"""
        return self._changed(self.L.fn("scene_set_env_map_device")(self._ctx, int(w), int(h), C.c_void_p(int(texels_pointer))))

    def set_sky(self, slots=(), records=None, sky=None, transmittance_lut=None, multiscatter_lut=None) -> int:
        """the physical sky: new records [n][16] 32-bit words for the suns in light slots `slots`, and / or a new 256-byte rayhip_sky
        (bytes or an array) with its two look-up tables (float32; all three or none).  The map is re-baked in place, then as
        set_env_map() (rayhip_scene_set_sky)."""
        slots = np.ascontiguousarray(slots, dtype=np.uint32).ravel()
        rec = np.zeros((0, 16), np.uint32) if records is None else np.ascontiguousarray(records)
        rec = (rec if rec.dtype == np.uint32 else rec.view(np.uint32)).reshape(-1, 16)
        assert len(slots) == len(rec)
        keep = []

        def ptr(a, dtype):
            if a is None:
                return None
            a = np.frombuffer(a, dtype=dtype).copy() if isinstance(a, (bytes, bytearray)) else np.ascontiguousarray(a).view(dtype).ravel()
            keep.append(a)
            return a.ctypes.data

        s = ptr(sky, np.uint8)
        assert s is None or keep[-1].nbytes == 256
        return self._changed(self.L.fn("scene_set_sky")(self._ctx, len(slots), slots.ctypes.data if len(slots) else None, rec.ctypes.data if len(slots) else None,
                                                        s, ptr(transmittance_lut, np.float32), ptr(multiscatter_lut, np.float32)))

    def set_texture(self, handle: int, rgba8) -> int:
        """new texels for the texture `handle` names (the reference's handle word): `rgba8` [h][w] uint32 (or [h][w][4] uint8) of the
        size of the held texture's level 0.  An uncompressed storage takes the words as they are; the BC3 (YCoCg), BC4 and BC5 storages
        are compressed and their mips rebuilt on the device (rayhip_scene_set_texture).  Returns as set_environment()."""
        t = np.ascontiguousarray(rgba8)
        t = t.view(np.uint32).reshape(t.shape[0], t.shape[1]) if t.dtype == np.uint8 else np.ascontiguousarray(t, dtype=np.uint32)
        assert t.ndim == 2
        return self._changed(self.L.fn("scene_set_texture")(self._ctx, int(handle), t.shape[1], t.shape[0], t.ctypes.data))

    def set_texture_device(self, handle: int, w: int, h: int, texels_pointer: int) -> int:
        """the same from w x h uint32 that are on this context's device already: their address as an int (a tensor's data_ptr(), say),
        4-byte aligned, the data complete when the call is made (rayhip_scene_set_texture_device)"""
        return self._changed(self.L.fn("scene_set_texture_device")(self._ctx, int(handle), int(w), int(h), C.c_void_p(int(texels_pointer))))

    def set_texture_blocks(self, handle: int, blocks) -> int:
        """ready 4 x 4 blocks (bytes, or a uint8 array) for the whole mip chain of a texture of a block storage, level 0 first
        (rayhip_scene_set_texture_blocks)"""
        b = np.frombuffer(blocks, dtype=np.uint8).copy() if isinstance(blocks, (bytes, bytearray)) else np.ascontiguousarray(blocks).view(np.uint8).ravel()
        return self._changed(self.L.fn("scene_set_texture_blocks")(self._ctx, int(handle), b.ctypes.data, b.nbytes))

    def read_accel(self, which: int) -> np.ndarray:
        """test hook (rayhip_k_read_accel): 0 the BVH2 nodes [n][16] u32 words, 1 the triangle records [n][12] f32, 2 tri_indices [n] u32,
        3 the live top-level leaves [n][7] u32 words (instance slot, lo.xyz, hi.xyz as float bits), by slot, 4 the vertex array as
        VERTEX_DTYPE records, 5 the light tree as LIGHT_NODE_DTYPE records (208 bytes each), 6 its importance rows [nodes][26][4] f32,
        7 the world-space corners of the triangle lights [light slots][4][4] f32, 8 the instance array as MESH_INSTANCE_DTYPE records,
        9 the light array [light slots][16] u32 words, 10 the leaf summaries of the light refit [light slots][12] f32, 11 the material
        array as MATERIAL_DTYPE records, 12 the environment map's quadtree [quads][4] f32 (the kept levels, finest first), 13 the 64-byte
        rayhip_environment the kernels see + total_lum, medium_lum as 18 u32 words, 14 the environment map's level-0 texels [w * h] u32,
        15 the whole texel pool as u32 words, 16 the rayhip_texture records (36 words each), tex_table[8] and texture_flags as u32 words"""
        n = C.c_size_t(0)
        self.L.fn("k_read_accel")(self._ctx, which, None, 0, C.byref(n))  # (refused: the size comes back)
        buf = np.zeros(max(int(n.value), 4) // 4, dtype=np.uint32)
        self.L.check(self.L.fn("k_read_accel")(self._ctx, which, buf.ctypes.data, buf.nbytes, C.byref(n)))
        buf = buf[:n.value // 4]
        return {0: lambda: buf.reshape(-1, 16), 1: lambda: buf.view(np.float32).reshape(-1, 12), 2: lambda: buf, 3: lambda: buf.reshape(-1, 7),
                4: lambda: buf.view(VERTEX_DTYPE), 5: lambda: buf.view(LIGHT_NODE_DTYPE), 6: lambda: buf.view(np.float32).reshape(-1, 26, 4),
                7: lambda: buf.view(np.float32).reshape(-1, 4, 4), 8: lambda: buf.view(MESH_INSTANCE_DTYPE), 9: lambda: buf.reshape(-1, 16),
                10: lambda: buf.view(np.float32).reshape(-1, 12), 11: lambda: buf.view(MATERIAL_DTYPE),
                12: lambda: buf.view(np.float32).reshape(-1, 4), 13: lambda: buf, 14: lambda: buf, 15: lambda: buf, 16: lambda: buf}[which]()

    def render(self, iteration: int, rect=None, cam: Camera = None, flags: int = 0, stats: Stats = None):
        rect = (0, 0, self.w, self.h) if rect is None else rect
        r = (C.c_int * 4)(*rect)
        cam = cam or self.cam
        self.L.check(self.L.fn("render")(self._ctx, C.byref(cam), C.byref(r), iteration, flags,
                                         C.byref(stats) if stats is not None else None))

    def render_batch(self, first_iteration: int, count: int, rect=None, cam: Camera = None, flags: int = 0, stats: Stats = None):
        """iterations first_iteration .. first_iteration + count - 1 in as few wavefront passes as possible (same pixels as
        `count` render() calls, bit for bit)"""
        rect = (0, 0, self.w, self.h) if rect is None else rect
        r = (C.c_int * 4)(*rect)
        cam = cam or self.cam
        self.L.check(self.L.fn("render_batch")(self._ctx, C.byref(cam), C.byref(r), first_iteration, count, flags,
                                               C.byref(stats) if stats is not None else None))

    def bvh_width(self) -> int:
        """8 / 4: the wide quantised BLAS form the kernels walk; 2: the reference's BVH2"""
        return int(self.L.fn("scene_bvh_width")(self._ctx))

    def closest_hit_form(self) -> int:
        """0: one ray per lane; 1: persistent refill kernel; 2: the pooled kernel (include/rayhip.h)"""
        return int(self.L.fn("closest_hit_form")(self._ctx)) if self.L.prefix == "rayhip_" else 0

    def direct_entry(self) -> int:
        """1: the persistent walks enter the scene's one instance from their arguments; 0: they walk the top level (include/rayhip.h)"""
        return int(self.L.fn("direct_entry")(self._ctx)) if self.L.prefix == "rayhip_" else 0

    def max_batch(self) -> int:
        """largest number of iterations one wavefront pass of the current frame can carry"""
        return int(self.L.fn("max_batch")(self._ctx))

    def set_tonemap_lut(self, view_transform: int, lut: np.ndarray):
        """dims^3 RGB10_A2 table of a non-Standard view transform (uint32, x fastest)"""
        lut = np.ascontiguousarray(lut, dtype=np.uint32).reshape(-1)
        dims = round(lut.size ** (1.0 / 3.0))
        assert dims ** 3 == lut.size, "the table must be a cube"
        self.L.check(self.L.fn("set_tonemap_lut")(self._ctx, view_transform, lut.ctypes.data, dims))

    def denoise_nlm(self, iteration: int, rect=None, cam: Camera = None):
        """RendererBase::DenoiseImage(region): NLM filter of what `iteration` iterations accumulated -> RAW, FINAL"""
        rect = (0, 0, self.w, self.h) if rect is None else rect
        r = (C.c_int * 4)(*rect)
        cam = cam or self.cam
        self.L.check(self.L.fn("denoise_nlm")(self._ctx, C.byref(cam), C.byref(r), iteration))

    def reserve_batch(self, count: int):
        """allocate the buffers passes of `count` iterations need (under the current shard) ahead of time"""
        self.L.check(self.L.fn("reserve_batch")(self._ctx, count))

    def readback(self, which: int = BUF_RAW, out: np.ndarray = None) -> np.ndarray:
        """`out`: a [h, w, 4] float32 array to fill (a caller that reads frames repeatedly should reuse one: the HIP runtime
        pins the destination pages for the copy, and unmapping pinned pages -- numpy freeing a large array -- makes the kernel
        driver stop and restart the process's GPU queues, 15-30 ms during which running kernels stand still)"""
        if out is None:
            out = np.empty((self.h, self.w, 4), dtype=np.float32)
        assert out.shape == (self.h, self.w, 4) and out.dtype == np.float32 and out.flags["C_CONTIGUOUS"]
        self.L.check(self.L.fn("readback")(self._ctx, which, out.ctypes.data, self.w))
        return out

    def readback_device(self, which: int, device_ptr: int, pitch_px: int = None):
        self.L.check(self.L.fn("readback_device")(self._ctx, which, C.c_void_p(device_ptr), pitch_px or self.w))

    def set_raw_device(self, device_ptr: int, pitch_px: int = None, cam: Camera = None):
        cam = cam or self.cam
        self.L.check(self.L.fn("set_raw_device")(self._ctx, C.c_void_p(device_ptr), pitch_px or self.w, C.byref(cam)))

    def export_shard_device(self, which: int, device_ptr: int):
        """this rank's OWNED pixels of image `which` (zero elsewhere) into device memory: the operand of the frame reduce"""
        self.L.check(self.L.fn("export_shard_device")(self._ctx, which, C.c_void_p(device_ptr)))

    # the exchange with the caller's transport (rayhip.h: rayhip_export_owned & co.): the tiles a rank owns, densely packed
    def owned_bytes(self, what: int, nranks: int, rank: int) -> int:
        return int(self.L.fn("owned_bytes")(self._ctx, what, nranks, rank))

    def export_owned(self, what: int, device_ptr: int, capacity_bytes: int):
        self.L.check(self.L.fn("export_owned")(self._ctx, what, C.c_void_p(device_ptr), capacity_bytes))

    def import_owned(self, what: int, from_rank: int, device_ptr: int, nbytes: int):
        self.L.check(self.L.fn("import_owned")(self._ctx, what, from_rank, C.c_void_p(device_ptr), nbytes))

    def finish_import(self, cam: Camera = None):
        self.L.check(self.L.fn("finish_import")(self._ctx, C.byref(cam or self.cam)))

    # spatial radiance cache (rayhip.h: rayhip_cache_*; GPU times in stage_times(): cache_update / cache_resolve)
    def cache_enable(self, on: bool = True):
        self.L.check(self.L.fn("cache_enable")(self._ctx, int(bool(on))))

    def cache_resolve(self, cam_pos=None, cam: Camera = None):
        """ResolveSpatialCache at `cam` (its origin), or at a camera standing at `cam_pos`"""
        if cam is None:
            cam = Camera()
            cam.origin[:] = [float(v) for v in cam_pos]
        self.L.check(self.L.fn("cache_resolve")(self._ctx, C.byref(cam)))

    def cache_reset(self):
        self.L.check(self.L.fn("cache_reset")(self._ctx))

    def cache_readback(self, which: int = 0, count: int = CACHE_ENTRIES):
        """(keys u64 [count], voxels u32 [count][4]) of the first `count` slots; which 0: previous frames' voxels, 1: this frame's"""
        keys = np.zeros(count, dtype=np.uint64)
        vox = np.zeros((count, 4), dtype=np.uint32)
        self.L.check(self.L.fn("cache_readback")(self._ctx, keys.ctypes.data, vox.ctypes.data, which, count))
        return keys, vox

    # test hooks of the cache kernels (rayhip.h: rayhip_k_cache_*)
    def k_cache_begin_paths(self, paths: int):
        self.L.check(self.L.fn("k_cache_begin_paths")(self._ctx, int(paths)))

    def k_cache_update_vertices(self, grid: CacheGrid, verts: np.ndarray):
        """one bounce of CACHE_VERTEX_DTYPE vertices, at most one per path"""
        verts = np.ascontiguousarray(verts, dtype=CACHE_VERTEX_DTYPE)
        self.L.check(self.L.fn("k_cache_update_vertices")(self._ctx, C.byref(grid), verts.ctypes.data, len(verts)))

    def k_cache_query(self, grid: CacheGrid, points: np.ndarray) -> np.ndarray:
        """points [n][6] (position, normal) -> [n][4] (mean radiance / exposure, samples; zero: no answer)"""
        points = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 6)
        out = np.zeros((len(points), 4), dtype=np.float32)
        self.L.check(self.L.fn("k_cache_query")(self._ctx, C.byref(grid), points.ctypes.data, len(points), out.ctypes.data))
        return out

    # test hooks of the tree builders and the wide node test (rayhip.h; the host build of the same calls: tests/bvh_build_cases.py)
    def k_lbvh_build(self, boxes: np.ndarray, groups: np.ndarray, n_groups: int, leaf_max: int, leaf_is_primitive: bool, roots_are_nodes: bool,
                     on_host: bool = False):
        """boxes [n][6] (lo, hi), groups [n] -> dict(nodes [k][16] u32 words, entries, group_root, bounds [6])"""
        boxes = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 6)
        groups = np.ascontiguousarray(groups, dtype=np.uint32)
        n = len(boxes)
        nodes = np.zeros((max(n - 1, 0) + n_groups + 1, 16), dtype=np.uint32)
        entries = np.zeros(2 * n + 1, dtype=np.uint32)
        root = np.zeros(n_groups + 1, dtype=np.uint32)
        bounds = np.zeros(6, dtype=np.float32)
        counts = np.zeros(2, dtype=np.uint32)
        self.L.check(self.L.fn("k_lbvh_build")(self._ctx, boxes.ctypes.data, groups.ctypes.data, n, n_groups, leaf_max, int(leaf_is_primitive),
                                               int(roots_are_nodes), int(on_host), nodes.ctypes.data, len(nodes) - 1, entries.ctypes.data,
                                               len(entries) - 1, root.ctypes.data, bounds.ctypes.data, counts.ctypes.data))
        return {"nodes": nodes[:counts[0]].copy(), "entries": entries[:counts[1]].copy(), "group_root": root[:n_groups].copy(), "bounds": bounds}

    def k_bvh4_collapse(self, nodes: np.ndarray, roots: np.ndarray):
        """BVH2 nodes [k][16] u32 words, roots -> (wide nodes [m][16] u32 words, the wide node of each root), or None: a box cannot be quantised"""
        nodes = np.ascontiguousarray(nodes, dtype=np.uint32).reshape(-1, 16)
        roots = np.ascontiguousarray(roots, dtype=np.uint32)
        wide = np.zeros((len(nodes) + 1, 16), dtype=np.uint32)
        roots4 = np.zeros(len(roots) + 1, dtype=np.uint32)
        count = C.c_uint32(0)
        rc = self.L.fn("k_bvh4_collapse")(self._ctx, nodes.ctypes.data, len(nodes), roots.ctypes.data, len(roots), wide.ctypes.data,
                                          roots4.ctypes.data, C.addressof(count))
        if rc == 2:
            return None
        self.L.check(rc)
        return wide[:count.value].copy(), roots4[:len(roots)].copy()

    def k_bvh4_test_nodes(self, wide: np.ndarray, node_index, ray_o, ray_d, ray_t):
        """one node visit per item -> (ref [n][4], n_hit [n], dist [n][4])"""
        wide = np.ascontiguousarray(wide, dtype=np.uint32).reshape(-1, 16)
        node_index = np.ascontiguousarray(node_index, dtype=np.uint32)
        n = len(node_index)
        o, d = (np.ascontiguousarray(a, dtype=np.float32).reshape(n, 3) for a in (ray_o, ray_d))
        t = np.ascontiguousarray(ray_t, dtype=np.float32).reshape(n)
        ref, n_hit, dist = np.zeros((n, 4), np.uint32), np.zeros(n, np.uint32), np.zeros((n, 4), np.float32)
        self.L.check(self.L.fn("k_bvh4_test_nodes")(self._ctx, wide.ctypes.data, len(wide), node_index.ctypes.data, o.ctypes.data, d.ctypes.data,
                                                    t.ctypes.data, n, ref.ctypes.data, n_hit.ctypes.data, dist.ctypes.data))
        return ref, n_hit, dist

    # UNet denoiser (rayhip.h: rayhip_unet_init / rayhip_denoise_unet)
    def unet_init(self, weights: np.ndarray, offsets: np.ndarray, alignment: int = 8):
        weights = np.ascontiguousarray(weights, dtype=np.float32)
        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        assert offsets.size == 32
        self.L.check(self.L.fn("unet_init")(self._ctx, weights.ctypes.data, weights.size, offsets.ctypes.data, alignment))

    def unet_precision(self, half: bool):
        """False: the exact f32 form (default); True: f16 tensors / weights with f32 accumulators (what the reference's GPU backends run)"""
        self.L.check(self.L.fn("unet_set_precision")(self._ctx, int(bool(half))))

    def denoise_unet(self, pass_index: int = -1, rect=None, cam: Camera = None):
        r = (C.c_int * 4)(*((0, 0, self.w, self.h) if rect is None else rect))
        self.L.check(self.L.fn("denoise_unet")(self._ctx, C.byref(cam or self.cam), C.byref(r), pass_index))

    def unet_read_tensor(self, which: int) -> np.ndarray:
        """activation tensor 0 .. 14 of the current precision with its one-pixel border, [rows, columns, channels] (f16 tensors widened);
        15: the 16-channel image-inputs tensor pass 0 / pass 13 wrote"""
        wr, hr = 16 * ((self.w + 15) // 16), 16 * ((self.h + 15) // 16)
        buf = np.zeros((wr + 2) * (hr + 2) * 112, dtype=np.float32)
        dims = (C.c_int * 3)()
        self.L.check(self.L.fn("unet_read_tensor")(self._ctx, which, buf.ctypes.data, buf.size, C.byref(dims)))
        n = dims[0] * dims[1] * dims[2]
        return buf[:n].reshape(dims[0], dims[1], dims[2]).copy()

    def set_shard(self, tile: int, shard_count: int, shard_index: int):
        """multi-GPU tile sharding: render only the tiles whose ordinal % shard_count == shard_index"""
        self.L.check(self.L.fn("set_shard")(self._ctx, tile, shard_count, shard_index))

    def sync(self):
        self.L.check(self.L.fn("sync")(self._ctx))

    def trav_counters(self, reset=True):
        out = (TravCounters * 2)()
        self.L.check(self.L.fn("get_trav_counters")(self._ctx, C.byref(out), int(reset)))
        return out[0].as_dict(), out[1].as_dict()

    def trav_timing(self, reset=True):
        ms = (C.c_double * 2)()
        n = (C.c_ulonglong * 2)()
        self.L.check(self.L.fn("get_trav_timing")(self._ctx, C.byref(ms), C.byref(n), int(reset)))
        return (float(ms[0]), int(n[0])), (float(ms[1]), int(n[1]))

    def stage_times(self, reset=True) -> dict:
        st = Stats()
        self.L.check(self.L.fn("get_stage_times")(self._ctx, C.byref(st), int(reset)))
        return st.as_dict()

    # ---- kernel-level hooks ------------------------------------------------------------------------------
    def k_generate_primary_rays(self, iteration: int, rect=None, cam: Camera = None):
        rect = (0, 0, self.w, self.h) if rect is None else rect
        n = rect[2] * rect[3]
        rays = np.zeros(n, dtype=RAY_DTYPE)
        hits = np.zeros(n, dtype=HIT_DTYPE)
        cnt = C.c_int(0)
        r = (C.c_int * 4)(*rect)
        self.L.check(self.L.fn("k_generate_primary_rays")(self._ctx, C.byref(cam or self.cam), C.byref(r), iteration,
                                                          rays.ctypes.data, hits.ctypes.data, C.byref(cnt)))
        return rays[:cnt.value], hits[:cnt.value]

    def k_intersect_closest(self, rays: np.ndarray, hits: np.ndarray, iteration: int, cam: Camera = None,
                            flags: int = FLAG_COUNT_TRAVERSAL):
        """flags=FLAG_COUNT_TRAVERSAL: instrumented walk of the reference BVH2 (+ visit counters); 0: the product kernel"""
        rays = np.ascontiguousarray(rays.copy())
        hits = np.ascontiguousarray(hits.copy())
        tc = TravCounters()
        self.L.check(self.L.fn("k_intersect_closest")(self._ctx, C.byref(cam or self.cam), rays.ctypes.data,
                                                      hits.ctypes.data, len(rays), iteration, flags, C.byref(tc)))
        return rays, hits, tc.as_dict()

    def k_intersect_shadow(self, rays: np.ndarray, iteration: int, cam: Camera = None):
        rays = np.ascontiguousarray(rays)
        out = np.zeros((len(rays), 4), dtype=np.float32)
        tc = TravCounters()
        self.L.check(self.L.fn("k_intersect_shadow")(self._ctx, C.byref(cam or self.cam), rays.ctypes.data, len(rays),
                                                     iteration, out.ctypes.data, C.byref(tc)))
        return out, tc.as_dict()

    def k_shade(self, bounce: int, iteration: int, rays: np.ndarray, hits: np.ndarray, color: np.ndarray, cam: Camera = None):
        """ShadePrimary (bounce 0) / ShadeSecondary on host (ray, hit) pairs; returns (color, secondary rays, shadow rays)
        -- the twin of the oracle's refk_shade.  Emitted rays come back in no particular order."""
        rays, hits = np.ascontiguousarray(rays), np.ascontiguousarray(hits)
        color = np.ascontiguousarray(color.copy(), dtype=np.float32)
        assert color.shape == (self.h, self.w, 4)
        n = len(rays)
        sec = np.zeros(n + 1, dtype=RAY_DTYPE)
        sh = np.zeros(n + 1, dtype=SHADOW_RAY_DTYPE)
        nsec, nsh = C.c_int(), C.c_int()
        self.L.check(self.L.fn("k_shade")(self._ctx, C.byref(cam or self.cam), bounce, iteration, rays.ctypes.data, hits.ctypes.data, n,
                                          color.ctypes.data, sec.ctypes.data, C.byref(nsec), sh.ctypes.data, C.byref(nsh)))
        return color, sec[:nsec.value], sh[:nsh.value]

    def k_scrambled_rand(self, dims, seeds, samples):
        dims = np.ascontiguousarray(dims, dtype=np.uint32)
        seeds = np.ascontiguousarray(seeds, dtype=np.uint32)
        samples = np.ascontiguousarray(samples, dtype=np.int32)
        out = np.zeros((len(dims), 2), dtype=np.float32)
        self.L.check(self.L.fn("k_scrambled_rand")(self._ctx, dims.ctypes.data, seeds.ctypes.data, samples.ctypes.data,
                                                   len(dims), out.ctypes.data))
        return out


class Comm:
    """rayhip_comm: the frame reduce over RCCL behind the C ABI.  `Comm(lib, devices)` drives all GPUs from this process
    (what a C++ host does); `Comm.for_rank(lib, id, nranks, rank, ctx)` is the one-process-per-GPU form."""

    def __init__(self, library: Library, devices=None, _handle=None):
        self.L = library
        self._h = C.c_void_p()
        if _handle is not None:
            self._h = _handle
            return
        devs = (C.c_int * len(devices))(*devices)
        self.L.check(self.L.fn("comm_create")(len(devices), devs, C.byref(self._h)))

    @staticmethod
    def probe(library: Library) -> str:
        """'' if this process can load RCCL with every symbol the exchange needs, else the reason -- local, not collective"""
        if library.fn("comm_probe")() == 0:
            return ""
        return (library.fn("last_error")() or b"RCCL unavailable").decode()

    def info(self) -> dict:
        out = (C.c_int * 4)()
        self.L.check(self.L.fn("comm_info")(self._h, C.byref(out)))
        return {"nranks": out[0], "rank": out[1], "nccl_comm_count": out[2], "in_process": bool(out[3])}

    @staticmethod
    def unique_id(library: Library) -> bytes:
        buf = C.create_string_buffer(COMM_ID_BYTES)
        library.check(library.fn("comm_unique_id")(buf, COMM_ID_BYTES))
        return buf.raw

    @classmethod
    def for_rank(cls, library: Library, unique_id: bytes, nranks: int, rank: int, ctx: "Context"):
        h = C.c_void_p()
        library.check(library.fn("comm_create_rank")(C.c_char_p(unique_id), nranks, rank, ctx._ctx, C.byref(h)))
        return cls(library, _handle=h)

    def bind(self, rank: int, ctx: "Context"):
        self.L.check(self.L.fn("comm_bind")(self._h, rank, ctx._ctx))

    def reduce_framebuffers(self, root: int, cam: Camera, what: int = REDUCE_ALL):
        self.L.check(self.L.fn("comm_reduce_framebuffers")(self._h, root, what, C.byref(cam)))

    def close(self):
        if self._h:
            self.L.fn("comm_destroy")(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
