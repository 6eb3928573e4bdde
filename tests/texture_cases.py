"""Cases of changing a texture's texels on the device (rayhip_scene_set_texture / _device / _blocks; ray_amd/csrc/texture_update.h):
the host build of the element functions (tests/hostsim/hostsim_texture.cpp), seeded images of the kinds and sizes the compressor can go
wrong on, scenes whose pool holds one texture of each storage between neighbours, and readers of the texture parts of a scene blob.
Shared by tests/test_texture_hostsim.py and tests/test_gpu_texture_update.py."""
import ctypes as C
import os
import struct

import numpy as np

import util
import vertex_update_cases as V
from ray_amd import api, scenes
from ray_amd.scenes import PrincipledMat, ShadingNode, eShadingNode, eTextureFormat

TEX_LIB = os.path.join(util.ROOT, "tests", "hostsim", "_build", "libhostsim_texture.so")
TEXTURE = np.dtype([("width", "<u4", (12,)), ("height", "<u4", (12,)), ("offset", "<u4", (12,))])
assert TEXTURE.itemsize == 144
RAW_BC, YCOCG_BIT = 1, 4 << 24
BLOCK_WORDS = {4: 2, 5: 4, 6: 2, 7: 4}

# (w, h, generate_mipmaps): see the table in the module docstring of tests/test_texture_hostsim.py
SIZES = ((1, 1, True), (3, 5, True), (4, 4, True), (5, 4, True), (16, 16, True), (20, 12, True), (67, 33, True), (64, 32, True), (16, 16, False))
KINDS = ("random", "constant", "two_colours", "gradient", "saturated", "grey31", "grey63", "alternating")
# the textures of a scene that take new texels: how AddTexture gets them, and the storage they land in with / without compression
TARGETS = ("bc3", "bc4", "bc5_rgba", "bc5_rg")
PLAIN = ("rgba", "rgb", "rg", "r")


def have_host_scene_lib():
    return os.path.exists(api.HIP_HOST_LIB)


# ---- the host build -------------------------------------------------------------------------------------------------------------
_lib = None


def tex_lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(TEX_LIB)
        vp, u32, i32 = C.c_void_p, C.c_uint32, C.c_int
        _lib.hostsim_set_texture.argtypes = [vp, u32, vp, u32, vp, u32, u32, i32, i32, vp]
        _lib.hostsim_set_texture_blocks.argtypes = [vp, u32, vp, u32, vp, u32, u32, vp, C.c_size_t]
        _lib.hostsim_texture_block.argtypes = [u32, vp, vp]
    return _lib


def host_block(storage, rgba16):
    """the block of storage 5 / 6 / 7 over sixteen RGBA8 words, as words"""
    t = np.ascontiguousarray(rgba16, dtype=np.uint32).ravel()
    assert t.size == 16
    out = np.zeros(BLOCK_WORDS[storage], dtype=np.uint32)
    assert tex_lib().hostsim_texture_block(storage, t.ctypes.data, out.ctypes.data) == 0
    return out


# ---- the texture parts of a scene blob ------------------------------------------------------------------------------------------------
class Pool:
    """texel pool, records, tex_table and texture_flags of a serialised scene (or of a context: from_context)"""

    def __init__(self, words, records, tex_table, flags):
        self.words = np.ascontiguousarray(words, dtype=np.uint32).copy()
        self.records = np.ascontiguousarray(records).view(TEXTURE).copy()
        self.tex_table = np.ascontiguousarray(tex_table, dtype=np.uint32).copy()
        self.flags = int(flags)

    @classmethod
    def of_blob(cls, blob):
        s = V.sections(blob)
        off, _ = s["scalars"]
        table = struct.unpack_from("<8I", blob, off)
        flags = struct.unpack_from("<I", blob, off + 32 + 64 + 12)[0]

        def section(name, dtype):
            o, size = s[name]
            return np.frombuffer(blob, dtype=dtype, count=size // np.dtype(dtype).itemsize, offset=o)

        return cls(section("texels", "<u4"), section("textures", TEXTURE), table, flags)

    @classmethod
    def of_context(cls, ctx):
        """arrays 15 and 16 of rayhip_k_read_accel"""
        meta = ctx.read_accel(16)
        n = (len(meta) - 9) // 36
        return cls(ctx.read_accel(15), meta[:36 * n].view(TEXTURE), meta[36 * n:36 * n + 8], meta[36 * n + 8])

    def copy(self):
        return Pool(self.words, self.records, self.tex_table, self.flags)

    def record(self, handle):
        return self.records[int(self.tex_table[handle >> 28]) + (handle & 0xffffff)]

    def levels(self, handle):
        """[(w, h, first word, words)] of the levels the texture holds"""
        t, storage = self.record(handle), handle >> 28
        out = []
        for lod in range(12):
            if lod and t["offset"][lod] == t["offset"][lod - 1]:
                break
            w, h = int(t["width"][lod]), int(t["height"][lod])
            n = ((w + 3) // 4) * ((h + 3) // 4) * BLOCK_WORDS[storage] if storage >= 4 and self.flags & RAW_BC else w * h
            out.append((w, h, int(t["offset"][lod]), n))
        return out

    def mask(self, handle):
        """True at the words the texture holds"""
        m = np.zeros(len(self.words), dtype=bool)
        for _, _, at, n in self.levels(handle):
            m[at:at + n] = True
        return m

    def same_meta(self, other):
        return self.records.tobytes() == other.records.tobytes() and np.array_equal(self.tex_table, other.tex_table) and self.flags == other.flags


def host_set_texture(pool: Pool, handle, texels):
    """(return code, the pool afterwards) of rayhip_scene_set_texture by the host build; texels [h][w] uint32"""
    t = np.ascontiguousarray(texels, dtype=np.uint32)
    out = pool.copy()
    rc = tex_lib().hostsim_set_texture(out.words.ctypes.data, len(out.words), out.records.ctypes.data, len(out.records), out.tex_table.ctypes.data, out.flags,
                                       int(handle), t.shape[1], t.shape[0], t.ctypes.data)
    return rc, out


def host_set_texture_blocks(pool: Pool, handle, blocks):
    b = np.ascontiguousarray(blocks).view(np.uint8).ravel()
    out = pool.copy()
    rc = tex_lib().hostsim_set_texture_blocks(out.words.ctypes.data, len(out.words), out.records.ctypes.data, len(out.records), out.tex_table.ctypes.data, out.flags,
                                              int(handle), b.ctypes.data, b.nbytes)
    return rc, out


# ---- images ---------------------------------------------------------------------------------------------------------------------------
def image(kind, w, h, seed):
    """[h][w][4] uint8, seeded; the fourth channel is noise that no compressed storage reads"""
    rs = np.random.RandomState(7000 + 131 * seed + 17 * w + h)
    by, bx = (h + 3) // 4, (w + 3) // 4
    per_block = lambda a: np.repeat(np.repeat(a, 4, axis=0), 4, axis=1)[:h, :w]  # noqa: E731
    if kind == "random":
        img = rs.randint(0, 256, size=(h, w, 4))
    elif kind == "constant":  # min == max in every block
        img = np.broadcast_to(rs.randint(0, 256, size=(1, 1, 4)), (h, w, 4))
    elif kind == "two_colours":
        a, b = per_block(rs.randint(0, 256, size=(by, bx, 4))), per_block(rs.randint(0, 256, size=(by, bx, 4)))
        img = np.where(rs.randint(0, 2, size=(h, w, 1)) == 1, a, b)
    elif kind == "gradient":
        y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        p = rs.uniform(0.0, 6.0, size=4)
        img = np.stack([127.5 + 127.5 * np.sin(0.11 * (k + 1) * x + 0.07 * (4 - k) * y + p[k]) for k in range(4)], axis=-1)
    elif kind == "saturated":  # blocks all 0, all 255, or texels of both
        mode = per_block(rs.randint(0, 3, size=(by, bx, 4)))
        img = np.where(mode == 0, 0, np.where(mode == 1, 255, 255 * rs.randint(0, 2, size=(h, w, 4))))
    elif kind in ("grey31", "grey63"):  # chroma within +-31 (scale 4) / within +-63 and, in every block, beyond +-31 (scale 2) of 128
        reach = 10 if kind == "grey31" else 45
        grey = rs.randint(64, 192, size=(h, w, 1))
        img = grey + rs.randint(-reach, reach + 1, size=(h, w, 4))
        if kind == "grey63":
            img[::4, ::4, 0] = grey[::4, ::4, 0] + 45  # Co = 128 + 45
            img[::4, ::4, 2] = grey[::4, ::4, 0] - 45
    elif kind == "alternating":  # 0 / 255 per texel
        y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        img = np.broadcast_to((((x + y + seed) & 1) * 255)[..., None], (h, w, 4))
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(np.clip(np.rint(img), 0, 255).astype(np.uint8))


def words_of(rgba):
    rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
    return rgba.view(np.uint32).reshape(rgba.shape[0], rgba.shape[1]).copy()


def texels_for(target, img):
    """[h][w] uint32: what rayhip_scene_set_texture takes for `img` [h][w][4] going into a texture added as `target`.  The compressed
    storages read R, G, B / R / R, G and the rest stays noise; an uncompressed one takes the channel replication of an upload."""
    t = img.copy()
    if target == "rgb":
        t[..., 3] = t[..., 2]
    elif target == "rg":
        t[..., 2] = t[..., 3] = t[..., 1]
    elif target == "r":
        t[..., 1] = t[..., 2] = t[..., 3] = t[..., 0]
    return words_of(t)


def add_texture(scene, target, img, mips):
    """AddTexture of `img` [h][w][4] the way that lands it in the storage `target` names; returns the handle"""
    F = eTextureFormat
    kw = dict(generate_mipmaps=mips, force_no_compression=target in PLAIN)
    if target in ("bc3", "rgb"):
        return scene.AddTexture(img[..., :3], fmt=F.RGB888, is_srgb=True, **kw)
    if target in ("bc4", "r"):
        return scene.AddTexture(img[..., :1], fmt=F.R8, is_srgb=False, **kw)
    if target == "bc5_rgba":  # (AddTexture repacks R, G; B only decides reconstruct_z)
        return scene.AddTexture(img, fmt=F.RGBA8888, is_srgb=False, is_normalmap=True, **kw)
    if target in ("bc5_rg", "rg"):
        return scene.AddTexture(img[..., :2], fmt=F.RG88, is_srgb=False, is_normalmap=target == "bc5_rg", **kw)
    if target == "rgba":
        return scene.AddTexture(img, fmt=F.RGBA8888, is_srgb=True, **kw)
    raise KeyError(target)


def _box(scene, mats):
    attrs, idx = scenes.cornell_mesh_arrays()
    groups = [(mats[0], None, 0, 6), (mats[1 % len(mats)], None, 6, 6), (mats[2 % len(mats)], None, 12, 6), (mats[0], None, 19, 6), (mats[0], None, 25, 6),
              (mats[-1], 0xFFFFFFFF, 31, 6), (mats[0], None, 37, 60)]
    scene.AddMeshInstance(scene.AddMesh(attrs, idx, groups))
    scenes._cornell_camera(scene)
    scene.Finalize()


def pool_scene(scene, targets, images, mips, odd=True):
    """A box with, per target, a neighbour texture ahead of it and one behind it in the same storage.  odd: a 3 x 3 uncompressed R8
    texture puts every block texture at an odd word of the pool.  Returns {target: handle}."""
    scene.SetEnvironment(env_col=(0.0, 0.0, 0.0))
    n = lambda k, w, h: image("random", w, h, 900 + k)  # noqa: E731  (the neighbours: the same in every build)
    add_texture(scene, "rgba", n(0, 4, 4), False)
    if odd:
        add_texture(scene, "r", n(1, 3, 3), False)
    handles = {}
    for k, target in enumerate(targets):
        add_texture(scene, target, n(10 + k, 8, 8), True)
        handles[target] = add_texture(scene, target, images[target], mips)
        add_texture(scene, target, n(20 + k, 4, 4), False)
    grey = scene.AddMaterial(ShadingNode(type=eShadingNode.Diffuse, base_color=(0.5, 0.5, 0.5)))
    emit = scene.AddMaterial(ShadingNode(type=eShadingNode.Emissive, strength=100.0, importance_sample=True))
    _box(scene, [grey, emit])
    return handles


def alignment_scene(scene, images, odd):
    """16 words of RGBA, a BC3 texture, a one-block BC4 texture without mips (2 words) and a BC5 texture, which therefore starts 8 bytes
    off a 16-byte boundary.  odd: a 3 x 3 uncompressed R8 texture (9 words) ahead of them puts every block texture at an odd word.
    (Every block texture takes an even number of words, so one pool cannot hold both cases.)"""
    scene.SetEnvironment(env_col=(0.0, 0.0, 0.0))
    add_texture(scene, "rgba", image("random", 4, 4, 900), False)
    if odd:
        add_texture(scene, "r", image("random", 3, 3, 902), False)
    handles = {"bc3": add_texture(scene, "bc3", images["bc3"], True)}
    add_texture(scene, "bc4", image("random", 4, 4, 901), False)
    handles["bc5_rg"] = add_texture(scene, "bc5_rg", images["bc5_rg"], True)
    grey = scene.AddMaterial(ShadingNode(type=eShadingNode.Diffuse, base_color=(0.5, 0.5, 0.5)))
    emit = scene.AddMaterial(ShadingNode(type=eShadingNode.Emissive, strength=100.0, importance_sample=True))
    _box(scene, [grey, emit])
    return handles


# ---- ray_amd.scenes.cornell_textures with given images ------------------------------------------------------------------------------
def cornell_images(which):
    """(rgb [64][64][3], roughness [64][64][1], normal map [64][64][4]): set "A" is what scenes.cornell_textures draws, set "B" another"""
    res = 64
    i, j = np.meshgrid(np.arange(res), np.arange(res), indexing="ij")
    if which == "A":
        rgb = np.empty((res, res, 3), dtype=np.uint8)
        rgb[..., 0] = (40 + 180 * (0.5 + 0.5 * np.sin(i * 0.31) * np.cos(j * 0.17))).astype(np.uint8)
        rgb[..., 1] = (30 + 200 * (j / (res - 1.0))).astype(np.uint8)
        rgb[..., 2] = np.where(((i // 8) + (j // 8)) % 2 == 0, 220, 60).astype(np.uint8)
        rough = (20 + 200 * (0.5 + 0.5 * np.sin(i * 0.23 + j * 0.41))).astype(np.uint8)[..., None]
        return rgb, rough, scenes.bump_normal_map(res)
    rgb = np.empty((res, res, 3), dtype=np.uint8)
    rgb[..., 0] = np.where(((i // 4) + (j // 16)) % 2 == 0, 230, 40).astype(np.uint8)
    rgb[..., 1] = (60 + 150 * (0.5 + 0.5 * np.cos(i * 0.21 + j * 0.13))).astype(np.uint8)
    rgb[..., 2] = (20 + 210 * (i / (res - 1.0))).astype(np.uint8)
    rough = (30 + 180 * (0.5 + 0.5 * np.cos(i * 0.37 - j * 0.19))).astype(np.uint8)[..., None]
    nrm = np.ascontiguousarray(np.transpose(scenes.bump_normal_map(res), (1, 0, 2))[::-1])  # (its blue stays above 250 or below alike)
    nrm[..., 0] = 255 - nrm[..., 0]
    return rgb, rough, nrm


def cornell_textures_scene(scene, which):
    """scenes.cornell_textures over cornell_images(which); returns the handles (base colour, roughness, normal map) and the slot of
    the red wall's material"""
    rgb, rough, nrm = cornell_images(which)
    scene.SetEnvironment(env_col=(0.0, 0.0, 0.0))
    kw = dict(generate_mipmaps=True, force_no_compression=False)
    t_rgb = scene.AddTexture(rgb, fmt=eTextureFormat.RGB888, is_srgb=True, **kw)
    t_rough = scene.AddTexture(rough, fmt=eTextureFormat.R8, is_srgb=False, **kw)
    t_nrm = scene.AddTexture(nrm, is_srgb=False, is_normalmap=True, **kw)
    tex = scene.AddMaterial(PrincipledMat(base_texture=t_rgb, roughness=1.0, roughness_texture=t_rough, normal_map=t_nrm, normal_map_intensity=1.0, specular=0.5))
    red = scene.AddMaterial(ShadingNode(type=eShadingNode.Diffuse, base_color=(0.5, 0.0, 0.0)))
    green = scene.AddMaterial(ShadingNode(type=eShadingNode.Diffuse, base_color=(0.0, 0.5, 0.0)))
    grey = scene.AddMaterial(ShadingNode(type=eShadingNode.Diffuse, base_color=(0.5, 0.5, 0.5)))
    emit = scene.AddMaterial(ShadingNode(type=eShadingNode.Emissive, strength=100.0, importance_sample=True))
    attrs, idx = scenes.cornell_mesh_arrays()
    groups = [(tex, None, 0, 6), (grey, None, 6, 6), (tex, None, 12, 6), (red, None, 19, 6), (green, None, 25, 6), (emit, 0xFFFFFFFF, 31, 6), (tex, None, 37, 60)]
    scene.AddMeshInstance(scene.AddMesh(attrs, idx, groups))
    scenes._cornell_camera(scene)
    scene.Finalize()
    return (t_rgb, t_rough, t_nrm), red


def cornell_texels(which):
    """what set_texture takes for the three textures of cornell_textures_scene(which)"""
    rgb, rough, nrm = cornell_images(which)
    pad = lambda a: np.concatenate([a, np.zeros(a.shape[:2] + (4 - a.shape[2],), dtype=np.uint8)], axis=-1)  # noqa: E731
    return words_of(pad(rgb)), words_of(pad(rough)), words_of(nrm)


# ---- scenes with pre-compressed textures (rayhip_scene_set_texture_blocks) -----------------------------------------------------------
BLOCK_TEXTURES = {"bc1": (eTextureFormat.BC1, 24, 20, 3), "bc3": (eTextureFormat.BC3, 18, 30, 2), "bc4": (eTextureFormat.BC4, 32, 32, 4),
                  "bc5": (eTextureFormat.BC5, 16, 16, 1)}  # (format, w, h, mips) as scenes.cornell_block_textures adds them


def block_data(name, seed):
    fmt, w, h, mips = BLOCK_TEXTURES[name]
    return scenes.random_blocks(fmt, w, h, mips, seed)


def cornell_block_scene(scene, seeds):
    """scenes.cornell_block_textures with the blocks of texture `name` drawn from seeds[name]; returns {name: handle}"""
    scene.SetEnvironment(env_col=(0.0, 0.0, 0.0))
    t = {}
    for name, (fmt, w, h, mips) in BLOCK_TEXTURES.items():
        t[name] = scene.AddTexture(block_data(name, seeds[name]), fmt=fmt, size=(w, h), mips_count=mips, is_srgb=name in ("bc1", "bc3"), is_normalmap=name == "bc5")
    m1 = scene.AddMaterial(PrincipledMat(base_texture=t["bc1"], roughness=1.0, roughness_texture=t["bc4"], specular=0.5))
    m3 = scene.AddMaterial(ShadingNode(type=eShadingNode.Diffuse, base_texture=t["bc3"], normal_map=t["bc5"], normal_map_intensity=0.6))
    m4 = scene.AddMaterial(ShadingNode(type=eShadingNode.Glossy, base_texture=t["bc1"], roughness=0.8, roughness_texture=t["bc4"]))
    red = scene.AddMaterial(ShadingNode(type=eShadingNode.Diffuse, base_color=(0.5, 0.0, 0.0)))
    emit = scene.AddMaterial(ShadingNode(type=eShadingNode.Emissive, strength=100.0, importance_sample=True))
    attrs, idx = scenes.cornell_mesh_arrays()
    groups = [(m1, None, 0, 6), (m3, None, 6, 6), (m3, None, 12, 6), (red, None, 19, 6), (m4, None, 25, 6), (emit, 0xFFFFFFFF, 31, 6), (m1, None, 37, 30),
              (m4, None, 67, 30)]
    scene.AddMeshInstance(scene.AddMesh(attrs, idx, groups))
    scenes._cornell_camera(scene)
    scene.Finalize()
    return t


BLOCK_SEEDS = {"bc1": 1, "bc3": 2, "bc4": 3, "bc5": 4}


# ---- reference-built scenes, once per process ---------------------------------------------------------------------------------------
_built = {}


def reference_scene(key, scene_fn, compress=True):
    """(blob, what scene_fn returned) of a scene the REFERENCE's host code built (its AddTexture, its block compressor, its mips),
    exported with the block storages as blocks"""
    if key not in _built:
        s = api.CreateSceneHIP(use_tex_compression=compress)
        ret = scene_fn(s)
        _built[key] = (api.export_scene_blob(s), ret)
    return _built[key]
