"""Cases of the NLM filter (rayhip_denoise_nlm; ray_amd/csrc/rt_denoise.h, kernels.hip.h: k_nlm_prepare_h / k_nlm_prepare_v / k_nlm_filter):
crafted input images, their injection into a context byte for byte through the exchange calls (rayhip_import_owned scatters exactly the
four images the filter reads), a plain numpy restatement of the filter and of the tonemap in any float type, and variants of that
restatement with one typical kernel error each.  Shared by tests/test_nlm_model_hostsim.py and tests/test_gpu_nlm_model.py."""
import copy
import os

import numpy as np

import util
from ray_amd import hip

EXT = 8                 # NLM_EXT_RADIUS
ULP = 2.0 ** -23
MASK = hip.REDUCE_ALL   # always explicit: 0 means three images on the host build and four in the library
# the host build with the variance image importable and readable: tests/hostsim_nlm (tests/hostsim/hostsim.cpp, unchanged, plus mask
# bit 3 and RAYHIP_BUF_VARIANCE)
HOST_LIB = os.path.join(util.ROOT, "tests", "hostsim_nlm", "_build", "libhostsim_nlm.so")


def host_library():
    assert os.path.exists(HOST_LIB), "tests/hostsim_nlm is not built (run __graft_entry__.build())"
    return hip.Library(HOST_LIB, prefix="hostsim_")


# ---- frames, rects, cases ------------------------------------------------------------------------------------------------------------
W, H = 53, 41  # no multiple of 16 in either direction


def rects(w=W, h=H):
    """whole frame; the 1 x 1 corners; 17 x 19 at the origin; 18 x 16 at the far corner; a 16 x 16 interior tile at a multiple of 16;
    an interior rect at an odd origin with sides 16 k + 1; a row; a column"""
    return [(0, 0, w, h), (0, 0, 1, 1), (w - 1, 0, 1, 1), (0, h - 1, 1, 1), (w - 1, h - 1, 1, 1), (0, 0, 17, 19), (w - 18, h - 16, 18, 16),
            (16, 16, 16, 16), (5, 3, 33, 17), (9, 20, 33, 1), (26, 2, 1, 37)]


PARTITION = [(0, 0, 21, 17), (21, 0, W - 21, 17), (0, 17, 37, H - 17), (37, 17, W - 37, H - 17)]  # four ragged rects: cuts at x = 21 / 37, y = 17

CASES = {"level1": dict(level=1.0, seed=11), "level8": dict(level=8.0, seed=12), "level60": dict(level=60.0, seed=13),
         "zero_variance": dict(level=8.0, seed=14, zero_variance=True)}
# the adaptive mark: variance that slopes across the frame, and a camera threshold (the filter compares with 0.5 * 0.2^2 = 0.02) that
# arms about half of it
ADAPTIVE_CASE = dict(level=8.0, seed=15, variance_slope=True)
ADAPTIVE_THRESHOLD = 0.2


def crafted(w, h, level=1.0, seed=1, zero_variance=False, variance_slope=False):
    """(full, base, dn, variance), float32 [h, w, 4], nothing negative, nothing non-finite.  Radiance: smooth part x hard vertical
    edge x multiplicative noise at brightness `level`, alpha not constant; variance skewed toward small values with about a fifth of
    the pixels exactly 0 (or all of them; `variance_slope`: times a slope across the frame); base colour in horizontal bands (the feature weight cuts the window); smooth depth-normals"""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    smooth = 0.55 + 0.4 * np.sin(0.21 * x + 0.3) * np.cos(0.17 * y - 0.2)
    edge = np.where(x >= int(0.55 * w), 0.35, 1.0)
    tint = np.stack([1.0 + 0.0 * x, 0.8 + 0.15 * np.sin(0.11 * y), np.where(x >= int(0.55 * w), 1.3, 0.6)], axis=-1)
    noise = np.maximum(1.0 + 0.25 * rs.standard_normal((h, w, 3)), 0.05)
    full = np.empty((h, w, 4))
    full[..., :3] = level * (smooth * edge)[..., None] * tint * noise
    full[..., 3] = 0.3 + 0.7 * (0.5 + 0.5 * np.sin(0.13 * x + 0.29 * y)) * np.maximum(1.0 + 0.1 * rs.standard_normal((h, w)), 0.5)
    variance = 0.5 * rs.uniform(0.0, 1.0, (h, w, 4)) ** 6
    variance[rs.uniform(0.0, 1.0, (h, w)) < 0.2] = 0.0
    if zero_variance:
        variance[:] = 0.0
    if variance_slope:  # small at the origin, large at the far corner: a threshold cuts the frame somewhere in between
        variance *= (((x + 0.5 * y) / (w + 0.5 * h)) ** 3)[..., None]
    band = (y.astype(np.int64) // 7) % 3
    colours = np.array([[0.8, 0.3, 0.2, 0.0], [0.35, 0.6, 0.25, 0.0], [0.5, 0.5, 0.75, 0.0]])
    base = colours[band] + 0.03 * np.sin(0.4 * x)[..., None]
    base[..., 3] = 0.0
    dn = np.stack([np.sin(0.05 * x + 0.02 * y), np.cos(0.05 * x + 0.02 * y) * 0.8, 0.3 + 0.001 * x * y / max(1, w), 0.2 + 0.6 * (x + 2.0 * y) / (w + 2.0 * h)], axis=-1)
    out = tuple(np.ascontiguousarray(a, dtype=np.float32) for a in (full, base, dn, variance))
    assert all(np.isfinite(a).all() for a in out) and all((a >= 0).all() for a in (out[0], out[1], out[3]))
    return out


_cases = {}


def case_images(name):
    """the crafted images of CASES[name] at W x H (made once)"""
    if name not in _cases:
        _cases[name] = crafted(W, H, **CASES[name])
    return _cases[name]


# ---- injection -----------------------------------------------------------------------------------------------------------------------
def pack(images, w, h, tile, nranks, rank):
    """what rank `rank` of `nranks` exports of `images` ([h, w, 4] each): owned tile j is frame tile rank + j * nranks, a tile x tile slot
    of float4 each, ragged tiles padded with zeros, the images one after the other (rt_base.h: shard_slot_pixel)"""
    tiles_x, tiles_y = (w + tile - 1) // tile, (h + tile - 1) // tile
    owned = list(range(rank, tiles_x * tiles_y, nranks))
    out = np.zeros((len(images), len(owned), tile, tile, 4), dtype=np.float32)
    for k, img in enumerate(images):
        assert img.shape == (h, w, 4) and img.dtype == np.float32
        for j, t in enumerate(owned):
            x0, y0 = (t % tiles_x) * tile, (t // tiles_x) * tile
            part = img[y0:y0 + tile, x0:x0 + tile]
            out[k, j, :part.shape[0], :part.shape[1]] = part
    return out.reshape(-1)


def is_device(ctx):
    return ctx.L.prefix == "rayhip_"


def _import(ctx, from_rank, buf):
    if is_device(ctx):
        import torch
        t = torch.from_numpy(buf if buf.size else np.zeros(4, dtype=np.float32)).cuda()
        torch.cuda.synchronize()  # (the copy runs on torch's stream, the unpack on the library's own)
        ctx.import_owned(MASK, from_rank, t.data_ptr(), buf.nbytes)  # (returns after the unpack)
    else:
        ctx.import_owned(MASK, from_rank, buf.ctypes.data, buf.nbytes)


def inject(ctx, full, base, dn, variance, tile=64, cam=None):
    """the four images the filter reads, into `ctx` byte for byte: an import takes another rank's tiles only, so the context stands in
    for rank 1 of 2 and takes rank 0's, then for rank 0 and takes rank 1's; RAW and FINAL follow from `full` (finish_import)"""
    images = [full, base, dn, variance]
    ctx.set_shard(tile, 2, 1)
    _import(ctx, 0, pack(images, ctx.w, ctx.h, tile, 2, 0))
    ctx.set_shard(tile, 2, 0)
    _import(ctx, 1, pack(images, ctx.w, ctx.h, tile, 2, 1))
    ctx.set_shard(64, 1, 0)
    ctx.finish_import(cam)


BUFFERS = (("raw", hip.BUF_RAW), ("final", hip.BUF_FINAL), ("base", hip.BUF_BASE_COLOR), ("dn", hip.BUF_DEPTH_NORMALS), ("variance", hip.BUF_VARIANCE))


def read_all(ctx):
    return {k: ctx.readback(b).copy() for k, b in BUFFERS}


def context(lib, w=W, h=H, scene="cornell_filmic"):
    """a context of `lib` (library or host build) with the scene's camera and, for cornell_filmic, its look-up table"""
    return util.make_context(lib, scene, w, h)


def camera(cam, **kw):
    """a copy of `cam` with fields replaced; min_samples / variance_threshold go to its pass settings"""
    c = copy.copy(cam)
    for k, v in kw.items():
        if k in ("min_samples", "variance_threshold"):
            setattr(c.pass_settings, k, v)
        else:
            setattr(c, k, v)
    return c


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def crop(img, rect):
    return img[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]]


def outside_equal(a, b, rect):
    """do [h, w, 4] images a and b have the same bits outside `rect`?"""
    same = bits(a) == bits(b)
    same[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]] = True
    return bool(same.all())


def check_pixels_outside_the_rect(lib):
    """after a rect filter on a context of `lib`, RAW and FINAL outside the rect keep their bits (and change inside), and base colour,
    depth-normals and variance keep theirs everywhere"""
    images = case_images("level60")
    ctx = context(lib)
    for rect in rects()[1:]:
        inject(ctx, *images, tile=12)
        before = read_all(ctx)
        ctx.denoise_nlm(1, rect=rect)
        after = read_all(ctx)
        assert outside_equal(after["raw"], before["raw"], rect) and outside_equal(after["final"], before["final"], rect), rect
        assert not np.array_equal(crop(after["raw"], rect), crop(before["raw"], rect)), rect
        for key in ("base", "dn", "variance"):
            assert np.array_equal(bits(after[key]), bits(before[key])), (rect, key)


# ---- the filter in plain numpy ----------------------------------------------------------------------------------------------------------
MUTANTS = ("clamp_right", "skip_offset", "swap_offset", "patch_8_taps", "seam_column", "var_rim_short", "alpha_kept")
_GAUSS = (0.2270270270, 0.1945945946, 0.1216216216, 0.0540540541, 0.0162162162)


def filter_domain(raw, dtype=np.float64):
    """reversible_tonemap (rt_accum.h) of a RAW image: the domain the filter works in"""
    c = np.asarray(raw).astype(dtype)
    m = np.maximum(c[..., 0], np.maximum(c[..., 1], c[..., 2]))
    return c / (m + dtype(1.0))[..., None]


def _sse_max(a, b):
    return np.where(a > b, a, b)


def _sse_min(a, b):
    return np.where(a < b, a, b)


def _sum4(v):
    return ((v[..., 0] + v[..., 1]) + v[..., 2]) + v[..., 3]


def nlm_model(full, variance, base, dn, rect, dtype=np.float64, mutant=None):
    """(tm, raw, var): the filtered image in the filter's domain, RAW = reversible_tonemap_invert of it, and the filtered variance, at the
    pixels of `rect` ([rect h, rect w, 4] each).  A restatement of rt_denoise.h over whole arrays: every constant is the kernel's float32
    one, every sum runs in the kernel's order, so with dtype = float32 this is the f32 twin and with float64 the same real function at
    higher precision.  `mutant`: one of MUTANTS, the restatement with that error."""
    assert mutant is None or mutant in MUTANTS
    T = dtype
    f32 = np.float32
    h, w = full.shape[:2]
    rx, ry, rw, rh = rect
    ew, eh = rw + 2 * EXT, rh + 2 * EXT
    xx, yy = rx - EXT + np.arange(ew), ry - EXT + np.arange(eh)  # frame coordinates of the extended region
    g = [T(f32(v)) for v in _GAUSS]

    def fetch(img, xs):  # clamped fetches from a frame buffer, rows yy
        flat = img.reshape(-1, 4)
        cy = np.clip(yy, 0, h - 1)
        cx = np.maximum(xs, 0) if mutant == "clamp_right" else np.clip(xs, 0, w - 1)  # (the mutant runs on into the next row)
        return flat[np.minimum(cy[:, None] * w + cx[None, :], w * h - 1)]

    F, V, B, D = (np.ascontiguousarray(a).astype(T) for a in (full, variance, base, dn))
    # stage 1: nlm_prepare_h
    tm = filter_domain(fetch(F, xx), T)
    center = fetch(V, xx)
    res = center * g[0]
    for i in range(4):
        res = res + fetch(V, xx - i + 1) * g[i + 1]
        res = res + fetch(V, xx + i + 1) * g[i + 1]
    var_h = _sse_max(res, center)
    # stage 2: nlm_prepare_v, the extended region minus a 4-pixel rim (what lies outside is never read: poisoned here)
    rim = 5 if mutant == "var_rim_short" else 4
    var = np.full((eh, ew, 4), 0.0 if mutant == "var_rim_short" else np.nan, dtype=T)
    ys = np.arange(rim, eh - rim)
    center = var_h[ys, rim:ew - rim]
    res = center * g[0]
    for i in range(4):
        res = res + var_h[ys - i + 1, rim:ew - rim] * g[i + 1]
        res = res + var_h[ys + i + 1, rim:ew - rim] * g[i + 1]
    var[rim:eh - rim, rim:ew - rim] = _sse_max(res, center)
    f0, f1 = fetch(B, xx), fetch(D, xx)

    # stage 3: nlm_filter_pixel over the columns [xa, xb) of the rect
    c_eps, c_damp = T(f32(0.0001)), T(f32(0.45) * f32(0.45))
    c_patch, c_quarter, c_f0, c_f1, c_cap = T(f32(0.25) * f32(9.0)), T(0.25), T(64.0), T(32.0), T(10000.0)

    def filt(tm, var, xa, xb):
        n = xb - xa

        def sl(a, dy, dx, pad):
            return a[EXT - pad + dy:EXT + rh + pad + dy, EXT + xa - pad + dx:EXT + xb + pad + dx]

        f0_i, f1_i = sl(f0, 0, 0, 0), sl(f1, 0, 0, 0)
        ipx, ivar = sl(tm, 0, 0, 1), sl(var, 0, 0, 1)
        sum_output, sum_weight = np.zeros((rh, n, 4), dtype=T), np.zeros((rh, n), dtype=T)
        for k in range(-3, 4):
            for l in range(-3, 4):
                if mutant == "skip_offset" and (k, l) == (3, 3):
                    continue
                dk, dl = (l, k) if mutant == "swap_offset" else (k, l)  # (the distance image of the transposed offset)
                jpx, jvar = sl(tm, dk, dl, 1), sl(var, dk, dl, 1)
                dist = ((ipx - jpx) * (ipx - jpx) - T(1.0) * (ivar + _sse_min(ivar, jvar))) / (c_eps + c_damp * (ivar + jvar))
                cd = np.zeros((rh, n, 4), dtype=T)
                for q in range(-1, 2):
                    for pp in range(-1, 2):
                        if mutant == "patch_8_taps" and (q, pp) == (1, 1):
                            continue
                        cd = cd + dist[1 + q:1 + q + rh, 1 + pp:1 + pp + n]
                weight = np.exp(-np.maximum(T(0.0), c_patch * _sum4(cd)))
                a, b = f0_i - sl(f0, k, l, 0), f1_i - sl(f1, k, l, 0)
                fd = _sse_max((c_f0 * a) * a, (c_f1 * b) * b)
                fw = np.exp(-np.maximum(T(0.0), np.minimum(c_cap, c_quarter * _sum4(fd))))
                weight = np.minimum(weight, fw)
                sum_output = sum_output + sl(tm, k, l, 0) * weight[..., None]
                sum_weight = sum_weight + weight
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where((sum_weight != 0)[..., None], sum_output / sum_weight[..., None], sum_output)

    if mutant == "seam_column":  # per 16-wide tile: the first staged rim column of every tile but the first holds its right neighbour
        parts = []
        for xa in range(0, rw, 16):
            tm_t, var_t = tm.copy(), var.copy()
            if xa > 0:
                tm_t[:, xa + EXT - 4], var_t[:, xa + EXT - 4] = tm[:, xa + EXT - 3], var[:, xa + EXT - 3]
            parts.append(filt(tm_t, var_t, xa, min(xa + 16, rw)))
        out = np.concatenate(parts, axis=1)
    else:
        out = filt(tm, var, 0, rw)
    m = np.maximum(out[..., 0], np.maximum(out[..., 1], out[..., 2]))
    raw = out / (T(1.0) - m)[..., None]  # reversible_tonemap_invert
    if mutant == "alpha_kept":
        raw[..., 3] = out[..., 3]
    assert np.isfinite(out).all(), "the restatement read what stage 2 does not write"
    return out, raw, var[EXT:EXT + rh, EXT:EXT + rw]


def e_ref_bound(tm):
    """sanity condition on the model: the host build (float32, the same operations) stays this close to it"""
    return 8 * ULP * max(1.0, float(np.abs(tm).max()))


def distance(raw, model_tm):
    """largest absolute distance, all four channels, of a float32 RAW crop from the model in the filter's domain"""
    return float(np.abs(filter_domain(raw) - model_tm).max())


# ---- the tonemap in plain numpy --------------------------------------------------------------------------------------------------------
def tonemap_model(raw, cam, lut=None, dims=0, dtype=np.float64):
    """tonemap() of rt_accum.h over an array [..., 4]: Standard curve or the table's trilinear form, gamma, saturate"""
    T, f32 = dtype, np.float32
    c = np.asarray(raw).astype(T)
    rgb, alpha = c[..., :3], c[..., 3]
    if cam.view_transform == 0:
        with np.errstate(invalid="ignore"):
            rgb = np.where(rgb < T(f32(0.0031308)), T(f32(12.92)) * rgb, T(f32(1.055)) * np.power(rgb, T(f32(1.0) / f32(2.4))) - T(f32(0.055)))
    else:
        lut = np.asarray(lut, dtype=np.uint32).reshape(-1)
        uv = (rgb / (rgb + T(1.0))) * T(f32(dims - 1))
        i = uv.astype(np.int64)  # truncation
        f = uv - np.floor(uv)
        j = np.minimum(i + 1, dims - 1)

        def texel(ix, iy, iz):
            v = lut[(iz * dims + iy) * dims + ix]
            s = T(f32(1.0) / f32(1023.0))
            return np.stack([(v & 0x3ff).astype(T) * s, ((v >> 10) & 0x3ff).astype(T) * s, ((v >> 20) & 0x3ff).astype(T) * s], axis=-1)

        (ix, iy, iz), (jx, jy, jz) = (i[..., k] for k in range(3)), (j[..., k] for k in range(3))
        fx, fy, fz = (f[..., k][..., None] for k in range(3))
        one = T(1.0)
        c00x = (one - fx) * texel(ix, iy, iz) + fx * texel(jx, iy, iz)
        c01x = (one - fx) * texel(ix, jy, iz) + fx * texel(jx, jy, iz)
        c10x = (one - fx) * texel(ix, iy, jz) + fx * texel(jx, iy, jz)
        c11x = (one - fx) * texel(ix, jy, jz) + fx * texel(jx, jy, jz)
        c0xx, c1xx = (one - fy) * c00x + fy * c01x, (one - fy) * c10x + fy * c11x
        rgb = (one - fz) * c0xx + fz * c1xx
    inv_gamma = f32(1.0) / f32(cam.gamma)
    if inv_gamma != f32(1.0):
        rgb = np.power(rgb, T(inv_gamma))  # (alpha: powf(a, 1) = a)
    out = np.concatenate([rgb, alpha[..., None]], axis=-1)
    return _sse_max(T(0.0), _sse_min(out, T(1.0)))


def tonemap_bound(cam, lut, dims):
    """sanity condition on tonemap_model: how far a float32 evaluation may lie from it.  Eight roundings of values up to 1 on the curve
    and the interpolation; on the table path the coordinate c / (c + 1) * (dims - 1) carries two roundings of a value up to dims - 1,
    which moves the result by that times the largest step between neighbouring texels, once per axis; a gamma g after that maps an
    error e to at most e^(1/g) (|a^p - b^p| <= |a - b|^p for p < 1)"""
    bound = 8 * ULP
    if cam.view_transform != 0:
        t = np.asarray(lut, dtype=np.uint32).reshape(dims, dims, dims)
        rgb = np.stack([t & 0x3ff, (t >> 10) & 0x3ff, (t >> 20) & 0x3ff], axis=-1).astype(np.float64) / 1023.0
        step = max(float(np.abs(np.diff(rgb, axis=a)).max()) for a in range(3))
        bound += 3 * ULP * (dims - 1) * step
    inv_gamma = float(np.float32(1.0) / np.float32(cam.gamma))
    return bound if inv_gamma == 1.0 else bound ** min(inv_gamma, 1.0) + 8 * ULP


# the four tonemaps of the FINAL tests: cornell_filmic's table or the Standard curve, gamma 1 or not
TONEMAPS = [dict(gamma=1.0), dict(gamma=2.2), dict(view_transform=0, gamma=1.0), dict(view_transform=0, gamma=2.2)]
TONEMAP_IDS = ["lut", "lut_gamma", "standard", "standard_gamma"]


def lut_of_blob(blob):
    """(table, dims) of the look-up table a scene blob carries"""
    import struct
    for i in range(struct.unpack_from("<I", blob, 8)[0]):  # scene_blob.h: Header {magic[8], count, pad}, Section {name[24], offset, size}
        name, off, size = struct.unpack_from("<24sQQ", blob, 16 + i * 40)
        if name.rstrip(b"\0") == b"tonemap_lut":
            break
    else:
        raise KeyError("tonemap_lut")
    lut = np.frombuffer(blob, dtype=np.uint32, count=size // 4, offset=off).copy()
    dims = round(lut.size ** (1.0 / 3.0))
    assert dims ** 3 == lut.size
    return lut, dims


def ramp_values(dims):
    """non-negative finite float32 radiances that hold 0, denormals, both neighbours of 0.0031308, 1, values up to 6e4, the values c
    at which c / (c + 1) * (dims - 1) is an integer with their float neighbours, and one that lands in the table's last cell"""
    f32 = np.float32
    edge = f32(0.0031308)
    v = [0.0, 1e-45, 3e-42, 1e-39, 1.17549435e-38, 1e-30, 1e-6, 0.001, np.nextafter(edge, f32(0)), edge, np.nextafter(edge, f32(1)), 0.01, 0.18,
         0.5, np.nextafter(f32(1), f32(0)), 1.0, np.nextafter(f32(1), f32(2)), 2.0, 7.5, 60.0, 1000.0, 6e4, 2.0 ** 25]
    for k in range(dims - 1):
        c = f32(k) / f32(dims - 1 - k)
        v += [np.nextafter(c, f32(0)), c, np.nextafter(c, f32(1e9))]
    v = np.unique(np.maximum(np.array(v, dtype=np.float32), 0))
    assert np.isfinite(v).all()
    return v


def ramp_image(dims, w=64):
    """the ramp as a frame: grey pixels first, then every value against two others in the other channels; alpha varies"""
    v = ramp_values(dims)
    n = len(v)
    k = np.arange(n)
    px = np.concatenate([np.stack([v, v, v], axis=-1), np.stack([v, v[(7 * k + 3) % n], v[(13 * k + 5) % n]], axis=-1),
                         np.stack([v[(5 * k + 1) % n], v[(11 * k + 2) % n], v], axis=-1)])
    h = (len(px) + w - 1) // w
    img = np.zeros((h * w, 4), dtype=np.float32)
    img[:len(px), :3] = px
    img[:, 3] = np.linspace(0.0, 1.5, h * w, dtype=np.float32)
    return img.reshape(h, w, 4)


# ---- the adaptive mark -------------------------------------------------------------------------------------------------------------------
def armed_prediction(images):
    """(armed, near): the pixels whose filtered variance (float64 model) reaches the filter's threshold 0.5 * ADAPTIVE_THRESHOLD^2 in a
    channel, and those that lie within 4 * 2^-23 relative of it in a channel, where float32 may decide either way"""
    _, _, var_model = nlm_model(images[0], images[3], images[1], images[2], (0, 0, W, H))
    threshold = float(np.float32(0.5) * np.float32(ADAPTIVE_THRESHOLD) * np.float32(ADAPTIVE_THRESHOLD))
    armed = (var_model >= threshold).any(axis=-1)
    near = (np.abs(var_model - threshold) <= 4 * ULP * threshold).any(axis=-1)
    return armed, near


def adaptive_changed(lib, images, cam_threshold, tile=12):
    """the pixels whose running mean moves in the iteration after the filter.  One iteration under a camera whose threshold is not in
    force yet leaves every pixel due at iteration 2 and no later; the images are injected; the filter, at iteration 2 under a camera
    with min_samples 1, re-arms the pixels whose filtered variance reaches the threshold; iteration 3 samples those and no others."""
    ctx = context(lib, W, H, "cornell_basic")
    ctx.render(1, cam=camera(ctx.cam, min_samples=2, variance_threshold=cam_threshold))
    cam = camera(ctx.cam, min_samples=1, variance_threshold=cam_threshold)
    inject(ctx, *images, tile=tile, cam=cam)
    before = ctx.readback(hip.BUF_RAW).copy()
    assert np.array_equal(bits(before), bits(images[0]))
    ctx.denoise_nlm(2, cam=cam)
    ctx.render(3, cam=cam)
    after = ctx.readback(hip.BUF_RAW)  # (a render leaves the running mean in RAW)
    return (bits(after) != bits(before)).any(axis=-1)
