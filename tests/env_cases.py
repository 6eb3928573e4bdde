"""Cases of changing the environment on the device (rayhip_scene_set_environment / _set_env_map / _set_sky; ray_amd/csrc/env_qtree.h):
the host build of the element functions (tests/hostsim/hostsim_environment.cpp), crafted RGBE maps, a float64 numpy model of the
quadtree, readers and patchers of the environment's parts of a scene blob, and the scenes.  Shared by tests/test_env_hostsim.py and
tests/test_gpu_environment.py."""
import ctypes as C
import math
import os
import struct

import numpy as np

import light_refit_cases as L
import oracle_lib as O
import util
import vertex_update_cases as V
from ray_amd import api, scenes
from ray_amd.scenes import PrincipledMat, ShadingNode, eShadingNode

ENV_LIB = os.path.join(util.ROOT, "tests", "hostsim", "_build", "libhostsim_environment.so")
f32 = np.float32
EPS = 2.0 ** -24
PI32 = float(f32(math.pi))  # rt_base.h: PI, the float the code divides and multiplies by
THRESHOLD = float(f32(0.005))  # env_qtree.h: LUM_FRACT_THRESHOLD
WEIGHTS = (np.array([[1, 4, 7, 4, 1], [4, 16, 26, 16, 4], [7, 26, 41, 26, 7], [4, 16, 26, 16, 4], [1, 4, 7, 4, 1]], dtype=f32) / f32(273.0)).astype(np.float64)

# How close to a texel's edge a tap's map coordinate (u * w, theta * h) must lie for the tap to count as AMBIGUOUS, in texels: 4 x the
# largest deviation of the host build's float32 coordinates (glibc) from the float64 model below over every tap of every map of MAPS.
# Measured on the CPU by measured_delta() -- 3.05e-05 texels, at theta * h of rgbe_sky (h = 64: half a float32 ulp of a coordinate near
# 64 is 3.8e-06, and the chain sqrt, sin / cos, acos, divide adds a few of them) -- and asserted against it by
# tests/test_env_hostsim.py::test_delta_is_what_the_host_build_measures.
DELTA = 3.06e-5

bits = L.bits


# ---- the host build -------------------------------------------------------------------------------------------------------------
_lib = None


def env_lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(ENV_LIB)
        vp, i32 = C.c_void_p, C.c_int
        _lib.hostsim_env_qtree_res.argtypes = [i32, i32]
        _lib.hostsim_env_qtree_layout.argtypes = [i32, vp]
        _lib.hostsim_env_qtree_layout.restype = C.c_uint32
        _lib.hostsim_env_qtree_taps.argtypes = [vp, i32, i32, vp, vp]
        _lib.hostsim_env_qtree_build.argtypes = [vp, i32, i32, vp, vp]
        _lib.hostsim_env_qtree_finish.argtypes = [i32, vp, vp]
        _lib.hostsim_env_levels_kept.argtypes = [vp, i32]
        _lib.hostsim_env_light_flux.argtypes = [C.c_float]
        _lib.hostsim_env_light_flux.restype = C.c_float
        _lib.hostsim_env_libm.argtypes = [i32, C.c_uint32, vp, vp, vp]
    return _lib


def host_libm(which, a, b=None):
    """env_libm.h over float32 arrays by the host build: 0 sinf, 1 cosf, 2 acosf, 3 atan2f(a, b)"""
    a = np.ascontiguousarray(a, dtype=f32)
    b = a if b is None else np.ascontiguousarray(b, dtype=f32)
    out = np.zeros(len(a), dtype=f32)
    assert env_lib().hostsim_env_libm(which, len(a), a.ctypes.data, b.ctypes.data, out.ctypes.data) == 0
    return out


def texels_of(img):
    """[h][w] uint32 of an [h][w][4] uint8 RGBE image (or of texels)"""
    img = np.ascontiguousarray(img)
    return img.view(np.uint32).reshape(img.shape[0], img.shape[1]).copy() if img.dtype == np.uint8 else np.ascontiguousarray(img, dtype=np.uint32)


class Pyramid:
    """the FULL pyramid of a map as env_qtree.h lays it out: quads [n][4] f32 (finest mip first), the first quad of each mip, the
    16 flags, total_lum, medium_lum; `kept`, the view of the kept levels and the environment light's flux as the host derives them"""

    def __init__(self, res, quads, block):
        self.res, self.quads = res, quads
        self.levels = int(math.log2(res))
        off = np.zeros(16, dtype=np.uint32)
        assert env_lib().hostsim_env_qtree_layout(res, off.ctypes.data) == len(quads)
        self.offsets = [int(o) for o in off]
        self.flags = block[:16].copy()
        self.total, self.medium = block[16:18].view(f32)
        self.kept = env_lib().hostsim_env_levels_kept(self.flags.ctypes.data, self.levels)
        self.flux = f32(env_lib().hostsim_env_light_flux(self.medium))

    def mip(self, level):
        end = self.offsets[level + 1] if level + 1 < self.levels else len(self.quads)
        return self.quads[self.offsets[level]:end]

    def kept_quads(self):
        """what rayhip_scene_desc::env_qtree holds: the kept levels, finest first"""
        return self.quads[self.offsets[self.levels - self.kept]:]


def host_pyramid(img) -> Pyramid:
    t = texels_of(img)
    h, w = t.shape
    res = env_lib().hostsim_env_qtree_res(w, h)
    off = np.zeros(16, dtype=np.uint32)
    quads = np.zeros((env_lib().hostsim_env_qtree_layout(res, off.ctypes.data), 4), dtype=f32)
    block = np.zeros(18, dtype=np.uint32)
    assert env_lib().hostsim_env_qtree_build(t.ctypes.data, w, h, quads.ctypes.data, block.ctypes.data) == 0
    return Pyramid(res, quads, block)


def host_finish(res, finest_quads) -> Pyramid:
    """the host build's upper mips, sums and flags over a finest mip that somebody else computed (the device)"""
    off = np.zeros(16, dtype=np.uint32)
    quads = np.zeros((env_lib().hostsim_env_qtree_layout(res, off.ctypes.data), 4), dtype=f32)
    quads[:len(finest_quads)] = finest_quads
    block = np.zeros(18, dtype=np.uint32)
    assert env_lib().hostsim_env_qtree_finish(res, quads.ctypes.data, block.ctypes.data) == 0
    return Pyramid(res, quads, block)


def host_taps(img):
    """(positions [2 res][2 res][2], luminances [2 res][2 res]) of every tap of the finest level, float32, by the host build"""
    t = texels_of(img)
    h, w = t.shape
    res = env_lib().hostsim_env_qtree_res(w, h)
    pos, lum = np.zeros((2 * res, 2 * res, 2), dtype=f32), np.zeros((2 * res, 2 * res), dtype=f32)
    assert env_lib().hostsim_env_qtree_taps(t.ctypes.data, w, h, pos.ctypes.data, lum.ctypes.data) == 0
    return pos, lum


def cell_grid(quads):
    """[2 n][2 n] cells of a mip of n x n quads: cell (cx, cy) is component (cx & 1) | ((cy & 1) << 1) of quad (cx / 2, cy / 2)"""
    n = int(round(math.sqrt(len(quads))))
    assert n * n == len(quads)
    return np.asarray(quads).reshape(n, n, 2, 2).transpose(0, 2, 1, 3).reshape(2 * n, 2 * n)


# ---- the maps -------------------------------------------------------------------------------------------------------------------
def to_rgbe(rgb):
    """[h][w][4] uint8 RGBE8 of [h][w][3] float radiance (the packing of ray_amd.scenes.rgbe_sky)"""
    rgb = np.asarray(rgb, dtype=np.float64)
    m = rgb.max(axis=-1)
    e = np.where(m > 1e-32, np.ceil(np.log2(np.maximum(m, 1e-32))), 0.0)
    scale = np.where(m > 1e-32, 256.0 / np.exp2(e), 0.0)
    img = np.zeros(rgb.shape[:2] + (4,), dtype=np.uint8)
    img[..., :3] = np.clip(np.floor(rgb * scale[..., None]), 0, 255).astype(np.uint8)
    img[..., 3] = np.where(m > 1e-32, np.clip(e + 128, 0, 255), 0).astype(np.uint8)
    return img


def sky_map(w=128, h=64, sun_dir=(0.35, 0.75, 0.55)):
    """ray_amd.scenes.rgbe_sky with its sun where `sun_dir` says (the default: the very map)"""
    v, u = np.meshgrid((np.arange(h) + 0.5) / h, (np.arange(w) + 0.5) / w, indexing="ij")
    theta, phi = v * math.pi, u * 2 * math.pi
    up = np.cos(theta)
    sky = np.stack([0.25 + 0.2 * (1 - up), 0.35 + 0.25 * (1 - up), 0.7 + 0.1 * up], axis=-1) * np.clip(up * 0.5 + 0.6, 0.05, None)[..., None]
    horizon = np.exp(-((theta - math.pi / 2) / 0.12) ** 2)[..., None] * np.array([0.9, 0.55, 0.3])
    d = np.stack([np.sin(theta) * np.cos(phi), np.cos(theta), np.sin(theta) * np.sin(phi)], axis=-1)
    sun = (np.clip((d * np.asarray(scenes._unit(sun_dir))).sum(-1), 0, 1) ** 600)[..., None] * np.array([900.0, 820.0, 640.0])
    return to_rgbe(sky + horizon + sun)


MOVED_SUN = (-0.55, 0.45, 0.30)


def noise_map(w, h, seed):
    """smooth radiance between 0.05 and 3 with a few bright spots: every level has cells on both sides of the threshold, none near it"""
    rng = np.random.RandomState(seed)
    v, u = np.meshgrid((np.arange(h) + 0.5) / h, (np.arange(w) + 0.5) / w, indexing="ij")
    rgb = np.stack([0.4 + 0.3 * np.sin(2 * math.pi * (u * (k + 1) + rng.uniform())) * np.cos(math.pi * (v * (k + 2) + rng.uniform())) for k in range(3)], axis=-1) + 0.3
    for _ in range(3):
        cu, cv = rng.uniform(0.1, 0.9, size=2)
        rgb += (np.exp(-(((u - cu) / 0.06) ** 2 + ((v - cv) / 0.08) ** 2))[..., None] * rng.uniform(20.0, 60.0, size=3))
    return to_rgbe(rgb)


def uniform_map(w=128, h=64, value=0.5):
    return to_rgbe(np.full((h, w, 3), value))


def black_map(w=64, h=32):
    return np.zeros((h, w, 4), dtype=np.uint8)


def one_texel_map(w=128, h=64, at=(37, 21)):
    img = black_map(w, h)
    img[at[1], at[0]] = (200, 180, 160, 133)
    return img


MAPS = {
    "16x8": lambda: noise_map(16, 8, 1),          # res 4, two levels: the smallest map that has an upper level
    "64x32": lambda: noise_map(64, 32, 2),
    "100x50": lambda: noise_map(100, 50, 3),      # not a power of two, res 32
    "rgbe_sky": lambda: scenes.rgbe_sky(),        # 128 x 64, the sun three orders above the sky
    "uniform": lambda: uniform_map(),             # cells at 1/64 and 1/256 of the total: the decision stops at 4 levels
    "black": lambda: black_map(),                 # total 0, one level, flux 0
    "one_texel": lambda: one_texel_map(),         # full depth
    "sun_moved": lambda: sky_map(sun_dir=MOVED_SUN),  # rgbe_sky with its sun somewhere else: what the frame tests change to
    # the maps the DEVICE's finest level is held against the model on.  A map whose width divides by a power of two has many taps
    # exactly on texel edges (u * w = j * w / (2 res)), where the texel read is decided by the libm's last bit; odd sizes that 3 does
    # not divide (theta = 1 / 3 and 1 / 2 are taps too) leave no tap within DELTA of an edge
    "37x19": lambda: noise_map(37, 19, 4),                       # res 16: one tile of cells, partly filled
    "101x49": lambda: noise_map(101, 49, 5),                     # res 32: four tiles
    "sky_127x65": lambda: sky_map(127, 65),                      # res 64: sixteen tiles, the sun three orders above the sky
}
DEVICE_MODEL_MAPS = ("37x19", "101x49", "sky_127x65")
_maps = {}


def env_map(name):
    if name not in _maps:
        _maps[name] = MAPS[name]()
    return _maps[name]


# ---- the float64 model of env_qtree.h -----------------------------------------------------------------------------------------------
def rgbe_luminance64(texels):
    """exact r + g + b of RGBE8 texels: the mantissas as the float32 bit trick of latlong_rgbe decodes them, times 2^(e - 128)"""
    t = np.asarray(texels, dtype=np.uint32)
    scale = np.exp2(((t >> 24) & 0xff).astype(np.float64) - 128.0)
    out = np.zeros(t.shape, dtype=np.float64)
    for shift in (0, 8, 16):
        m = (t >> shift) & 0xff
        out += ((np.uint32(0x3f800000) + m * np.uint32(0x8080) + (m + 1) // 2).astype(np.uint32).view(f32).astype(np.float64) - 1.0) * scale
    return out


def tap_positions64(w, h, res):
    """[2 res][2 res][2]: (u * w, theta * h) of every tap in float64, the formulas of env_qtree.h with the code's float PI"""
    q = ((1.0 + 0.5 * np.arange(2 * res) / res) % 1.0)  # (exact in float32 as well)
    qy, qx = np.meshgrid(q, q, indexing="ij")
    cos_theta = 2.0 * qx - 1.0
    phi = 2.0 * PI32 * qy
    phi = np.where(phi < 0, phi + 2 * PI32, phi)
    phi = np.where(phi > 2 * PI32, phi - 2 * PI32, phi)
    sin_theta = np.sqrt(1.0 - cos_theta * cos_theta)
    dx, dy, dz = sin_theta * np.cos(phi), cos_theta, -sin_theta * np.sin(phi)
    theta = np.arccos(np.clip(dy, -1.0, 1.0)) / PI32
    p = np.arctan2(dz, dx)
    p = np.where(p < 0, p + 2 * PI32, p)
    p = np.where(p > 2 * PI32, p - 2 * PI32, p)
    u = (0.5 * p / PI32) % 1.0
    return np.stack([u * w, theta * h], axis=-1)


class Model:
    """float64: per finest cell the interval [lo, hi] its value may lie in (a tap whose coordinate lies within `delta` of a texel's
    edge may read either texel), the pyramid over the unambiguous reading, the sums, the levels kept"""

    def __init__(self, img, delta=DELTA):
        t = texels_of(img)
        h, w = t.shape
        self.res = res = 1
        while 2 * self.res < min(w, h):
            self.res *= 2
        res = self.res
        lum = rgbe_luminance64(t)
        pos = tap_positions64(w, h, res)
        self.positions = pos

        def candidates(x, n, wraps):
            k = np.floor(x)
            near_lo, near_hi = (x - k) <= delta, (k + 1.0 - x) <= delta
            base = np.clip(k, 0, n - 1).astype(np.int64)
            other = np.where(near_lo, np.clip(k - 1, 0, n - 1), np.where(near_hi, np.clip(k + 1, 0, n - 1), base)).astype(np.int64)
            if wraps:  # (u = fract(...): a coordinate that rounds up to w reads texel 0)
                other = np.where(near_hi & (k + 1 >= n), 0, other)
            return base, other, near_lo | near_hi

        bx, ox, _ = candidates(pos[..., 0], w, True)
        by, oy, _ = candidates(pos[..., 1], h, False)
        self.ambiguous = (ox != bx) | (oy != by)  # (a coordinate at an edge of the map, where both readings are one texel, is not)
        self.reads = np.stack([lum[by, bx], lum[by, ox], lum[oy, bx], lum[oy, ox]])
        self.lo, self.hi = self._cells(self.reads.min(axis=0)), self._cells(self.reads.max(axis=0))
        self._sums(self.reads[0])

    def _cells(self, tap):
        res = self.res
        out = np.zeros((res, res))
        at = 2 * np.arange(res) + 1
        for jj in range(-2, 3):
            for ii in range(-2, 3):
                out += WEIGHTS[ii + 2][jj + 2] * tap[np.ix_((at + jj) % (2 * res), (at + ii) % (2 * res))]
        return out

    def _sums(self, tap):
        self.tap = tap
        self.grids = [self._cells(tap)]  # cell grids, finest first: grids[l] has res >> l cells per side
        while len(self.grids[-1]) > 2:
            g = self.grids[-1]
            self.grids.append(g.reshape(len(g) // 2, 2, len(g) // 2, 2).sum(axis=(1, 3)))
        self.levels = len(self.grids)
        self.total = float(self.grids[0].sum())
        self.medium = self.total / float((self.res // 2) * (self.res // 2))
        self.kept = 0
        for g in reversed(self.grids):
            self.kept += 1
            if not (g > THRESHOLD * self.total).any():
                break

    def resolve(self, tap_lum32):
        """The model's pyramid and sums with every AMBIGUOUS tap read as `tap_lum32` [2 res][2 res] (somebody's float32 tap luminances:
        the host build's) read it -- either texel is right for such a tap, and a sum is compared with a sum over the same texels.
        Every tap must be one of the model's readings to 3 float32 roundings, ambiguous or not; returns the worst relative miss."""
        got = np.asarray(tap_lum32, dtype=np.float64)
        miss = np.abs(self.reads - got[None])
        pick = miss.argmin(axis=0)
        chosen = np.take_along_axis(self.reads, pick[None], axis=0)[0]
        worst = float((miss.min(axis=0) / np.maximum(chosen, 1e-300)).max())
        assert (pick[~self.ambiguous] == 0).all() or np.array_equal(chosen[~self.ambiguous], self.reads[0][~self.ambiguous])
        self._sums(chosen)
        return worst

    def threshold_margin(self):
        """the smallest relative distance of any cell of any level from 0.005 * total (inf for a black map)"""
        t = THRESHOLD * self.total
        return min(float(np.abs(g - t).min()) / t for g in self.grids) if t > 0 else math.inf


def measured_delta():
    """4 x the largest deviation of the host build's tap coordinates from the model's, over MAPS"""
    worst = 0.0
    for name in MAPS:
        img = env_map(name)
        pos, _ = host_taps(img)
        worst = max(worst, float(np.abs(pos.astype(np.float64) - Model(img).positions).max()))
    return 4.0 * worst


# ---- the environment's parts of a scene blob ----------------------------------------------------------------------------------------
TEXTURE = np.dtype([("width", "<u4", (12,)), ("height", "<u4", (12,)), ("offset", "<u4", (12,))])
ENV = np.dtype([("env_col", "<f4", (3,)), ("env_map", "<u4"), ("back_col", "<f4", (3,)), ("back_map", "<u4"), ("env_map_rotation", "<f4"),
                ("back_map_rotation", "<f4"), ("light_index", "<u4"), ("sky_map_spread_angle", "<f4"), ("qtree_levels", "<i4"), ("_pad", "<u4", (3,))])
assert ENV.itemsize == 64 and TEXTURE.itemsize == 144


def section(blob, name, dtype):
    off, size = V.sections(blob)[name]
    return np.frombuffer(blob, dtype=dtype, count=size // np.dtype(dtype).itemsize, offset=off).copy()


def blob_env(blob):
    off, _ = V.sections(blob)["scalars"]
    return np.frombuffer(blob, dtype=ENV, count=1, offset=off + 32)[0].copy()


def with_env(blob, **fields):
    """`blob` with fields of its rayhip_environment changed"""
    e = blob_env(blob)
    for k, v in fields.items():
        e[k] = v
    b = bytearray(blob)
    off, _ = V.sections(blob)["scalars"]
    b[off + 32:off + 96] = e.tobytes()
    return bytes(b)


def blob_env_map(blob):
    """(first texel in the pool, w, h) of level 0 of the blob's environment map"""
    off, _ = V.sections(blob)["scalars"]
    tex_table = struct.unpack_from("<8I", blob, off)
    e = blob_env(blob)
    t = section(blob, "textures", TEXTURE)[tex_table[0] + (int(e["env_map"]) & 0xffffff)]
    return int(t["offset"][0]), int(t["width"][0]), int(t["height"][0])


def blob_env_texels(blob):
    at, w, h = blob_env_map(blob)
    return section(blob, "texels", "<u4")[at:at + w * h].reshape(h, w)


def with_env_texels(blob, texels):
    at, w, h = blob_env_map(blob)
    pool = section(blob, "texels", "<u4")
    pool[at:at + w * h] = np.asarray(texels, dtype=np.uint32).ravel()
    return V.patched_blob(blob, texels=pool)


def blob_qtree(blob):
    """[quads][4] f32: the kept levels, finest first"""
    return section(blob, "env_qtree", "<f4").reshape(-1, 4)


def qtree_mips(quads, levels):
    """the kept levels of a quadtree apart, finest first"""
    out, at = [], 0
    for lod in range(levels):
        n = 4 ** (levels - 1 - lod)
        out.append(quads[at:at + n])
        at += n
    assert at == len(quads)
    return out


def with_qtree(blob, quads, levels):
    return with_env(L.with_section(blob, "env_qtree", np.ascontiguousarray(quads, dtype=f32)), qtree_levels=levels)


def env_leaf(cwnodes, light_index):
    """(node, slot) of the leaf that names the environment light"""
    for w in range(len(cwnodes)):
        for i in range(8):
            link = int(cwnodes["child"][w, i])
            if link != 0x7fffffff and link & 0x80000000 and (link & 0x7fffffff) == light_index:
                return w, i
    raise KeyError(light_index)


# ---- the scenes -----------------------------------------------------------------------------------------------------------------
def env_scene(scene, img, rect_light=False, rotation=0.3, **cam):
    """ray_amd.scenes.cornell_env with `img` as its map; rect_light: one rect light beside the environment light, so that the
    environment leaf's flux matters to the pick"""
    sky = scene.AddTexture(img, is_srgb=False)
    scene.SetEnvironment(env_col=(1.0, 1.0, 1.0), back_col=(1.0, 1.0, 1.0), env_map=sky, back_map=sky, env_map_rotation=rotation, back_map_rotation=rotation,
                         importance_sample=True)
    grey = scene.AddMaterial(ShadingNode(type=eShadingNode.Diffuse, base_color=(0.5, 0.5, 0.5)))
    red = scene.AddMaterial(ShadingNode(type=eShadingNode.Diffuse, base_color=(0.5, 0.05, 0.05)))
    green = scene.AddMaterial(ShadingNode(type=eShadingNode.Diffuse, base_color=(0.05, 0.5, 0.05)))
    shiny = scene.AddMaterial(PrincipledMat(base_color=(0.8, 0.8, 0.85), metallic=1.0, roughness=0.15))
    q = scenes._CORNELL_QUADS
    attrs, idx = scenes.cornell_mesh_arrays([q[0], q[1], q[3], q[4]] + scenes._block_quads("short") + scenes._block_quads("tall"))
    scene.AddMeshInstance(scene.AddMesh(attrs, idx, [(grey, None, 0, 12), (red, None, 12, 6), (green, None, 18, 6), (grey, None, 24, 30), (shiny, None, 54, 30)]))
    if rect_light:
        scene.AddLight("rect", color=(6.0, 5.0, 4.0), width=0.16, height=0.12, xform=scenes._translate(-0.278, 0.5, -0.28))
    scenes._cornell_camera(scene, **cam)
    scene.Finalize()


def sky_scene(scene, moved=False, envmap_resolution=64, **cam):
    """ray_amd.scenes.cornell_sky at envmap_resolution 64 (or another); moved: the sun turned and the clouds drifted"""
    atmosphere = dict(clouds_offset_x=1500.0) if moved else {}
    scene.SetEnvironment(env_col=(1.0, 1.0, 1.0), back_col=(1.0, 1.0, 1.0), env_map=api.PhysicalSkyTexture, back_map=api.PhysicalSkyTexture,
                         importance_sample=True, envmap_resolution=envmap_resolution, clouds_density=0.6, cirrus_clouds_amount=0.6, **atmosphere)
    grey = scene.AddMaterial(ShadingNode(type=eShadingNode.Diffuse, base_color=(0.5, 0.5, 0.5)))
    red = scene.AddMaterial(ShadingNode(type=eShadingNode.Diffuse, base_color=(0.5, 0.05, 0.05)))
    green = scene.AddMaterial(ShadingNode(type=eShadingNode.Diffuse, base_color=(0.05, 0.5, 0.05)))
    mirror = scene.AddMaterial(PrincipledMat(base_color=(0.9, 0.9, 0.9), metallic=1.0, roughness=0.0))
    q = scenes._CORNELL_QUADS
    attrs, idx = scenes.cornell_mesh_arrays([q[0], q[3], q[4]] + scenes._block_quads("short") + scenes._block_quads("tall"))
    scene.AddMeshInstance(scene.AddMesh(attrs, idx, [(grey, None, 0, 6), (red, None, 6, 6), (green, None, 12, 6), (grey, None, 18, 30), (mirror, None, 48, 30)]))
    scene.AddLight("directional", color=(12.0, 11.0, 10.0), direction=(-0.35, -0.6, -0.8) if moved else (0.3, -0.5, -1.0), angle=0.6)
    scenes._cornell_camera(scene, **cam)
    scene.Finalize()


_blobs, _renders = {}, {}


def reference_blob(key, scene_fn):
    """the serialised scene the REFERENCE built (its own PrepareEnvMapQTree, light tree and sky bake), once per process"""
    if key not in _blobs:
        r = O.create_renderer(8, 8, "REF")  # (kept alive while its scene is in use)
        s = r.CreateScene()
        scene_fn(s)
        _blobs[key] = O.export_scene(s)
    return _blobs[key]


def map_blob(name, rect_light=False):
    return reference_blob(("map", name, rect_light), lambda s: env_scene(s, env_map(name), rect_light))


def reference_render(key, scene_fn, w, h, spp):
    """RAW of the reference's renderer over the scene, once per process"""
    if key not in _renders:
        r, _ = O.render_ref(scene_fn, w, h, spp)
        _renders[key] = r.get_raw_pixels_ref().copy()
    return _renders[key]
