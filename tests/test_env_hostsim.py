"""The environment map's importance quadtree as the device builds it (ray_amd/csrc/env_qtree.h), in its HOST build
(tests/hostsim/hostsim_environment.cpp), against the quadtree the reference itself built for a scene on the same map
(Scene::PrepareEnvMapQTree_nolock: the env_qtree and the environment leaf's flux of the blob the oracle exports) and against the float64
model of tests/env_cases.py.

What is asserted, per map: every level the reference kept -- the finest one too wherever it kept them all -- equals the host build's
bit for bit; the number of levels is the reference's; medium_lum and the environment light's flux differ from the reference's by at
most n * 2^-24 relative, n the number of finest cells -- the worst-case error of the reference's own running sum, which the pyramid's
top replaces here on purpose -- and from the float64 model by at most (25 + 2 * log2(res) + 4) * 2^-24.  The model's precondition: no
cell of any level lies within 1e-4 relative of 0.005 * total, so no decision hangs on a last bit.

The model against sums: on a map whose width divides by a power of two most taps lie EXACTLY on a texel's edge in x (u * w = j * w /
(2 res)), and which texel is read there is the libm's last bit.  The model therefore reads every such tap as the host build read it
(env_cases.Model.resolve, which also holds every tap luminance of the host build against the model's readings) before the sums are
compared; the unambiguous taps are the model's own."""
import os

import numpy as np
import pytest

import env_cases as E
import light_refit_cases as L
import oracle_lib as O

pytestmark = pytest.mark.skipif(not (O.have_ref() and os.path.exists(E.ENV_LIB)), reason="oracle/_ref or tests/hostsim not built")
bits = E.bits
HOST_MAPS = ("16x8", "64x32", "100x50", "rgbe_sky", "uniform", "black", "one_texel", "sun_moved")


def _reference(name):
    """(kept mips finest first, levels, medium_lum = the environment leaf's flux) as the reference built them"""
    blob = E.map_blob(name)
    env = E.blob_env(blob)
    a = L.Arrays(blob)
    assert env["light_index"] != 0xffffffff and (a.lights[env["light_index"], 0] & 7) == 6
    w, i = E.env_leaf(a.cwnodes, int(env["light_index"]))
    return E.qtree_mips(E.blob_qtree(blob), int(env["qtree_levels"])), int(env["qtree_levels"]), np.float32(a.cwnodes["flux"][w, i])


@pytest.mark.parametrize("name", HOST_MAPS)
def test_host_build_against_the_reference_quadtree(name):
    img = E.env_map(name)
    assert np.array_equal(E.blob_env_texels(E.map_blob(name)), E.texels_of(img)), "the blob carries the map as it was given"
    p = E.host_pyramid(img)
    mips, levels, ref_flux = _reference(name)
    assert p.kept == levels, (name, p.kept, levels, p.flags[:p.levels].tolist())
    for lod, ref in enumerate(mips):
        got = p.mip(p.levels - p.kept + lod)
        assert np.array_equal(bits(got), bits(ref)), (name, lod, int((bits(got) != bits(ref)).sum()))
    assert np.array_equal(bits(p.kept_quads()), bits(E.blob_qtree(E.map_blob(name))))
    n = p.res * p.res
    # the reference's medium_lum is its leaf's flux: (3 / 3) * medium_lum * 1
    assert p.flux == p.medium
    print(f"{name}: res {p.res}, {p.kept} of {p.levels} levels; medium_lum {p.medium!r} against the reference's {ref_flux!r}")
    if ref_flux == 0:
        assert p.medium == 0 and p.total == 0 and p.kept == 1
    else:
        assert abs(float(p.medium) - float(ref_flux)) <= n * E.EPS * float(ref_flux), (name, p.medium, ref_flux)


@pytest.mark.parametrize("name", HOST_MAPS + E.DEVICE_MODEL_MAPS)
def test_host_build_against_the_float64_model(name):
    img = E.env_map(name)
    p, m = E.host_pyramid(img), E.Model(img)
    margin = m.threshold_margin()
    worst_tap = m.resolve(E.host_taps(img)[1])
    margin = min(margin, m.threshold_margin())
    assert margin >= 1e-4, (name, margin)  # the precondition, on the model
    assert worst_tap <= 3 * E.EPS, (name, worst_tap)
    assert (p.res, p.levels, p.kept) == (m.res, m.levels, m.kept)
    finest = E.cell_grid(p.mip(0)).astype(np.float64)
    assert (finest >= m.lo * (1 - 29 * E.EPS)).all() and (finest <= m.hi * (1 + 29 * E.EPS)).all()
    assert (np.abs(finest - m.grids[0]) <= 29 * E.EPS * m.grids[0]).all()
    bound = (25 + 2 * np.log2(p.res) + 4) * E.EPS
    for got, want in ((p.medium, m.medium), (p.flux, m.medium), (p.total, m.total)):
        assert abs(float(got) - want) <= bound * want, (name, got, want)
    for level in range(1, p.levels):  # (three additions of positive numbers per level: 3 roundings on top of the finest cell's 29)
        g = E.cell_grid(p.mip(level)).astype(np.float64)
        assert (np.abs(g - m.grids[level]) <= (29 + 3 * level) * E.EPS * m.grids[level]).all(), (name, level)


def test_the_crafted_maps_decide_as_planned():
    uniform, black, one = (E.host_pyramid(E.env_map(n)) for n in ("uniform", "black", "one_texel"))
    assert (uniform.levels, uniform.kept) == (5, 4)  # cells at 1/64 of the total subdivide, cells at 1/256 do not
    assert (black.kept, float(black.total), float(black.flux)) == (1, 0.0, 0.0)
    assert one.kept == one.levels == 5
    small = E.host_pyramid(E.env_map("16x8"))
    assert (small.res, small.levels) == (4, 2)
    assert E.host_pyramid(E.env_map("100x50")).res == 32


def test_delta_is_what_the_host_build_measures():
    """env_cases.DELTA: 4 x the largest deviation of the host build's tap coordinates from the model's, rounded up"""
    measured = E.measured_delta()
    assert measured <= E.DELTA <= 1.05 * measured, (measured, E.DELTA)
    for name in E.DEVICE_MODEL_MAPS:  # the condition under which the device test bites: few taps may read either texel
        assert E.Model(E.env_map(name)).ambiguous.mean() <= 0.01, name


def test_env_libm_equals_the_c_library():
    """env_libm.h restates the sinf, cosf, acosf and atan2f of the C library the reference is built against: the same bits on the
    arguments the taps of a res-512 level pass them, and on 400000 seeded random arguments each (edges of the branches included)"""
    import ctypes as C
    import ctypes.util
    m = C.CDLL(ctypes.util.find_library("m"))
    for name in ("sinf", "cosf", "acosf", "atan2f"):
        getattr(m, name).restype = C.c_float
        getattr(m, name).argtypes = [C.c_float] * (2 if name == "atan2f" else 1)
    f32, rng = np.float32, np.random.RandomState(5)
    q = ((1.0 + 0.5 * np.arange(1024) / 512) % 1.0).astype(f32)
    phi = (f32(2) * E.f32(np.pi)) * q
    cos_theta = f32(2) * q - f32(1)
    sin_theta = np.sqrt(f32(1) - cos_theta * cos_theta)
    s, c = E.host_libm(0, phi), E.host_libm(1, phi)
    dz, dx = (-sin_theta[::9, None] * s[None, :]).ravel(), (sin_theta[::9, None] * c[None, :]).ravel()
    edges = np.array([0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 0.4375, 0.6875, 1.1875, 2.4375, 2.0 ** -12, 0.7853982, 1e-30], dtype=f32)
    cases = {0: (np.concatenate([phi, rng.uniform(-7, 7, 400000).astype(f32), edges]), None), 2: (np.concatenate([cos_theta, rng.uniform(-1, 1, 400000).astype(f32), edges[:6]]), None),
             3: (np.concatenate([dz, rng.uniform(-1, 1, 400000).astype(f32) * f32(10) ** rng.randint(-6, 1, 400000).astype(f32), np.repeat(edges, len(edges))]),
                 np.concatenate([dx, rng.uniform(-1, 1, 400000).astype(f32), np.tile(edges, len(edges))]))}
    cases[1] = cases[0]
    for which, (a, b) in cases.items():
        got = E.host_libm(which, a, b)
        fn = getattr(m, ("sinf", "cosf", "acosf", "atan2f")[which])
        want = np.array([fn(x) for x in a.tolist()] if b is None else [fn(y, x) for y, x in zip(a.tolist(), b.tolist())], dtype=f32)
        differ = bits(got) != bits(want)
        assert not differ.any(), (which, int(differ.sum()), a[differ][:3].tolist())
