"""Spatial radiance cache: a reproducible update workload and the three implementations it is fed to.

TEST INFRASTRUCTURE.  The same bounces of a cache-update pass are handed to
  * the reference's own Ref::SpatialCacheUpdate / Ref::SpatialCacheResolve, exported by the oracle (oracle/_ref/libray_ref.so),
  * the host build of ray_amd/csrc/rt_cache.h (tests/hostsim/_build/libhostsim_cache.so),
  * the device (librayhip's rayhip_cache_*),
in the reference's data layout: ray_data_t + hit_data_t per ray, the per-bounce radiance and depth-normal images indexed
y * img_w + x with the downsampled pixel (x, y) of the ray, and the path state per downsampled pixel y * (img_w / 4) + x
(RadCacheRef.cpp:252-309).
"""
import ctypes as C
import os

import numpy as np

from ray_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libray_ref.so")
HOST_LIB = os.path.join(ROOT, "tests", "hostsim", "_build", "libhostsim_cache.so")
N = hip.CACHE_ENTRIES
FORM_DEVICE, FORM_SERIAL = 0, 1


class Span(C.Structure):
    _fields_ = [("p", C.c_void_p), ("n", C.c_int64)]


def span(a: np.ndarray) -> Span:
    return Span(a.ctypes.data, len(a))


# ---- the workload ------------------------------------------------------------------------------------
class Workload:
    """`frames` frames of a cache-update pass over a pw x ph downsampled frame (img_w = 4 * pw), up to `bounces` bounces per path.
    Vertices lie on a few hundred spots of a box so that voxels collect many samples over the frames; some rays miss or hit a
    light; the throughput of every ray and the radiance of every bounce are random."""

    def __init__(self, seed=1, pw=48, ph=32, frames=5, bounces=5, cams=None):
        self.pw, self.ph, self.img_w = pw, ph, 4 * pw
        self.frames, self.bounces = frames, bounces
        self.cams = cams or [(0.1, 0.2, 2.5)] * frames
        rng = np.random.default_rng(seed)
        spots = rng.uniform(-1.0, 1.0, size=(400, 3)).astype(np.float32)
        normals = rng.normal(size=(400, 3)).astype(np.float32)
        self.passes = []
        for f in range(frames):
            cam = np.array(self.cams[f], dtype=np.float32)
            alive = np.ones(pw * ph, dtype=bool)
            bounces_of_frame = []
            for b in range(bounces):
                idx = np.nonzero(alive)[0]
                if len(idx) == 0:
                    break
                n = len(idx)
                rays = np.zeros(n, dtype=hip.RAY_DTYPE)
                hits = np.zeros(n, dtype=hip.HIT_DTYPE)
                x, y = idx % pw, idx // pw
                rays["xy"] = (x.astype(np.uint32) << 16) | y.astype(np.uint32)
                which = rng.integers(0, len(spots), size=n)
                target = spots[which] + rng.normal(scale=0.002, size=(n, 3)).astype(np.float32)
                o = (cam + rng.normal(scale=0.3, size=(n, 3))).astype(np.float32) if b == 0 else \
                    rng.uniform(-1.0, 1.0, size=(n, 3)).astype(np.float32)
                dv = target - o
                dist = np.linalg.norm(dv, axis=1).astype(np.float32)
                rays["o"] = o
                rays["d"] = (dv / dist[:, None]).astype(np.float32)
                rays["c"] = rng.uniform(0.2, 1.0, size=(n, 3)).astype(np.float32)
                rays["pdf"] = 1.0
                hits["t"] = dist
                hits["u"] = 0.3
                kind = rng.uniform(size=n)
                miss, light = kind < 0.08, (kind >= 0.08) & (kind < 0.12)
                hits["v"] = np.where(miss, -1.0, 0.2).astype(np.float32)
                hits["obj_index"] = np.where(light, -1, 0)
                hits["prim_index"] = 0
                radiance = np.zeros((self.img_w * ph, 4), dtype=np.float32)
                dn = np.zeros((self.img_w * ph, 4), dtype=np.float32)
                pix = y * self.img_w + x
                radiance[pix, :3] = rng.exponential(0.5, size=(n, 3)).astype(np.float32)
                dn[pix, :3] = normals[which]
                dn[pix, 3] = dist
                bounces_of_frame.append((rays, hits, radiance, dn))
                ended = miss | light | (rng.uniform(size=n) < 0.15)
                alive[idx[ended]] = False
            self.passes.append((cam, bounces_of_frame))

    def grid(self, f, exposure=1.0):
        return hip.CacheGrid.make(tuple(float(v) for v in self.passes[f][0]), exposure)

    def vertices(self, rays, hits, radiance, dn):
        """the bounce as rayhip_cache_vertex records"""
        v = np.zeros(len(rays), dtype=hip.CACHE_VERTEX_DTYPE)
        x, y = rays["xy"] >> 16, rays["xy"] & 0xffff
        pix = y * self.img_w + x
        v["o"], v["d"], v["t"] = rays["o"], rays["d"], hits["t"]
        v["path"] = y * (self.img_w // 4) + x
        v["n"] = dn[pix, :3]
        v["ends"] = ((hits["v"] < 0.0) | (hits["obj_index"] < 0)).astype(np.uint32)
        v["radiance"] = radiance[pix, :3]
        v["c"] = rays["c"]
        return v

    def run(self, cache, exposure=1.0, frames=None):
        """update + resolve, frame after frame, on any of the three caches below"""
        for f in range(self.frames if frames is None else frames):
            cam, bounces = self.passes[f]
            g = self.grid(f, exposure)
            cache.begin_paths(self.pw * self.ph)
            for rays, hits, radiance, dn in bounces:
                cache.update(g, self, rays, hits, radiance, dn)
            cache.resolve(cam)


# ---- the three caches ----------------------------------------------------------------------------
class HostCache:
    """the host build of rt_cache.h"""
    _lib = None

    @classmethod
    def lib(cls):
        if cls._lib is None:
            L = C.CDLL(HOST_LIB)
            vp = C.c_void_p
            L.hostsim_cache_create.restype = vp
            L.hostsim_cache_destroy.argtypes = [vp]
            L.hostsim_cache_destroy.restype = None
            L.hostsim_cache_begin_paths.argtypes = [vp, C.c_int]
            L.hostsim_cache_update_vertices.argtypes = [vp, C.POINTER(hip.CacheGrid), vp, C.c_int]
            L.hostsim_cache_resolve.argtypes = [vp, C.POINTER(C.c_float * 3), C.c_int]
            L.hostsim_cache_reset.argtypes = [vp]
            L.hostsim_cache_readback.argtypes = [vp, vp, vp, C.c_int, C.c_uint32]
            L.hostsim_cache_query.argtypes = [vp, C.POINTER(hip.CacheGrid), vp, C.c_int, vp]
            L.hostsim_cache_hash64.argtypes = [C.c_uint64]
            L.hostsim_cache_hash64.restype = C.c_uint32
            L.hostsim_cache_compute_hash.argtypes = [C.POINTER(hip.CacheGrid), C.POINTER(C.c_float * 3), C.POINTER(C.c_float * 3)]
            L.hostsim_cache_compute_hash.restype = C.c_uint64
            L.hostsim_cache_grid_level.argtypes = [C.POINTER(hip.CacheGrid), C.POINTER(C.c_float * 3)]
            L.hostsim_cache_grid_level.restype = C.c_uint32
            L.hostsim_cache_adjacent_hash.argtypes = [C.c_uint64, C.POINTER(hip.CacheGrid)]
            L.hostsim_cache_adjacent_hash.restype = C.c_uint64
            L.hostsim_cache_insert_key.argtypes = [vp, C.c_uint64]
            L.hostsim_cache_insert_key.restype = C.c_uint32
            L.hostsim_cache_find_key.argtypes = [vp, C.c_uint64]
            L.hostsim_cache_find_key.restype = C.c_uint32
            L.hostsim_cache_accumulate.argtypes = [vp, C.c_uint32, C.POINTER(C.c_float * 3), C.c_uint32]
            L.hostsim_cache_accumulate.restype = None
            L.hostsim_cache_topups.argtypes = [vp]
            L.hostsim_cache_topups.restype = C.c_uint32
            cls._lib = L
        return cls._lib

    def __init__(self, form=FORM_DEVICE):
        self.L = self.lib()
        self.h = C.c_void_p(self.L.hostsim_cache_create())
        self.form = form

    def close(self):
        if self.h:
            self.L.hostsim_cache_destroy(self.h)
            self.h = None

    def begin_paths(self, n):
        assert self.L.hostsim_cache_begin_paths(self.h, n) == 0

    def update_vertices(self, g, verts):
        verts = np.ascontiguousarray(verts)
        assert self.L.hostsim_cache_update_vertices(self.h, C.byref(g), verts.ctypes.data, len(verts)) == 0

    def update(self, g, wl, rays, hits, radiance, dn):
        self.update_vertices(g, wl.vertices(rays, hits, radiance, dn))

    def resolve(self, cam):
        assert self.L.hostsim_cache_resolve(self.h, C.byref((C.c_float * 3)(*[float(v) for v in cam])), self.form) == 0

    def reset(self):
        assert self.L.hostsim_cache_reset(self.h) == 0

    def readback(self, which=0):
        keys = np.zeros(N, dtype=np.uint64)
        vox = np.zeros((N, 4), dtype=np.uint32)
        assert self.L.hostsim_cache_readback(self.h, keys.ctypes.data, vox.ctypes.data, which, N) == 0
        return keys, vox

    def query(self, g, points):
        points = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 6)
        out = np.zeros((len(points), 4), dtype=np.float32)
        assert self.L.hostsim_cache_query(self.h, C.byref(g), points.ctypes.data, len(points), out.ctypes.data) == 0
        return out

    def topups(self):
        """adjacent-level top-ups over all resolves so far"""
        return int(self.L.hostsim_cache_topups(self.h))

    def insert_key(self, key):
        return int(self.L.hostsim_cache_insert_key(self.h, key))

    def find_key(self, key):
        return int(self.L.hostsim_cache_find_key(self.h, key))

    def accumulate(self, slot, rad, samples):
        self.L.hostsim_cache_accumulate(self.h, slot, C.byref((C.c_float * 3)(*rad)), samples)


class RefCache:
    """the reference's Ref::SpatialCacheUpdate / Ref::SpatialCacheResolve on arrays held here, scheduled as RendererCPU.h:1010-1232"""
    _fns = None
    UPDATE = "_ZN3Ray3Ref18SpatialCacheUpdateERKNS_19cache_grid_params_tENS_4SpanIKNS0_10hit_data_tEEENS4_IKNS0_10ray_data_tEEENS4_INS_12cache_data_tEEEPKNS_7color_tIfLi4EEESG_iNS4_ImEENS4_INS_20packed_cache_voxel_tEEE"
    RESOLVE = "_ZN3Ray3Ref19SpatialCacheResolveERKNS_19cache_grid_params_tENS_4SpanImEENS4_INS_20packed_cache_voxel_tEEENS4_IKS6_EEjj"
    CACHE_DATA = np.dtype([("entries", "<u4", 4), ("weight", "<f4", (4, 3)), ("len", "<i4")])

    @classmethod
    def fns(cls):
        if cls._fns is None:
            L = C.CDLL(REF_LIB)
            up, res = getattr(L, cls.UPDATE), getattr(L, cls.RESOLVE)
            vp = C.c_void_p
            up.argtypes = [C.POINTER(hip.CacheGrid), Span, Span, Span, vp, vp, C.c_int, Span, Span]
            up.restype = None
            res.argtypes = [C.POINTER(hip.CacheGrid), Span, Span, Span, C.c_uint32, C.c_uint32]
            res.restype = None
            cls._fns = (up, res)
        return cls._fns

    def __init__(self):
        assert self.CACHE_DATA.itemsize == 68
        self.up, self.res = self.fns()
        self.entries = np.zeros(N, dtype=np.uint64)
        self.vox = [np.zeros((N, 4), dtype=np.uint32), np.zeros((N, 4), dtype=np.uint32)]  # prev, curr
        self.cam_prev = (0.0, 0.0, 0.0)
        self.paths = None

    def begin_paths(self, n):
        self.paths = np.zeros(n, dtype=self.CACHE_DATA)

    def update(self, g, wl, rays, hits, radiance, dn):
        self.up(C.byref(g), span(hits), span(rays), span(self.paths), radiance.ctypes.data, dn.ctypes.data, wl.img_w, span(self.entries),
                span(self.vox[1]))

    def resolve(self, cam):
        g = hip.CacheGrid.make(tuple(float(v) for v in cam), 1.0, self.cam_prev)
        for start in range(0, N, 32768):
            self.res(C.byref(g), span(self.entries), span(self.vox[1]), span(self.vox[0]), start, 32768)
        self.vox = [self.vox[1], self.vox[0]]
        self.vox[1][:] = 0
        self.cam_prev = tuple(float(v) for v in cam)

    def reset(self):
        self.vox[0][:] = 0

    def readback(self, which=0):
        return self.entries.copy(), self.vox[which].copy()


class DeviceCache:
    """librayhip's rayhip_cache_* and rayhip_k_cache_* on a context"""

    def __init__(self, ctx: hip.Context):
        self.ctx = ctx
        ctx.cache_enable(True)

    def times_us(self):
        """GPU time (us) of the update and resolve kernels so far (the context's stage times, not reset)"""
        t = self.ctx.stage_times(reset=False)
        return t["cache_update"], t["cache_resolve"]

    def begin_paths(self, n):
        self.ctx.k_cache_begin_paths(n)

    def update_vertices(self, g, verts):
        self.ctx.k_cache_update_vertices(g, verts)

    def update(self, g, wl, rays, hits, radiance, dn):
        self.update_vertices(g, wl.vertices(rays, hits, radiance, dn))

    def resolve(self, cam):
        self.ctx.cache_resolve([float(v) for v in cam])

    def reset(self):
        self.ctx.cache_reset()

    def readback(self, which=0):
        return self.ctx.cache_readback(which)

    def query(self, g, points):
        return self.ctx.k_cache_query(g, points)


def as_map(keys: np.ndarray, vox: np.ndarray) -> dict:
    """key -> voxel words of the live slots (slot order inside a bucket depends on the order of the inserts)"""
    live = np.nonzero(keys)[0]
    return {int(k): tuple(int(x) for x in v) for k, v in zip(keys[live], vox[live])}


def buckets_compacted(keys: np.ndarray) -> bool:
    """every bucket's keys are a prefix of it"""
    b = keys.reshape(-1, 32) != 0
    return bool(np.all(b[:, 1:] <= b[:, :-1]))
