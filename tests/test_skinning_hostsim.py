"""Skinning without a GPU (ray_amd/csrc/skin.h through tests/hostsim/hostsim_skin.cpp): the host build of the element functions
equals an independent numpy restatement bit for bit, keeps what the header says it keeps, and the seeded poses of
tests/skin_cases.py leave no triangle without area -- which is what licenses the frame comparisons of tests/test_gpu_skinning.py."""
import numpy as np
import pytest

import skin_cases as S
import vertex_update_cases as V
from ray_amd import hip

bits = S.bits


@pytest.fixture(scope="module")
def fixture_scene():
    assert S.have_skin_lib(), "tests/hostsim/hostsim_skin.cpp is not built (run __graft_entry__.build())"
    return S.scene()[1]


def test_the_host_build_exists_and_knows_the_lds_threshold():
    assert S.have_skin_lib(), "tests/hostsim/hostsim_skin.cpp is not built (run __graft_entry__.build())"
    lds_bones = int(S.skin_lib().hostsim_skin_lds_bones())
    assert min(S.BONES) <= lds_bones < max(S.BONES)  # the palettes of the tests lie on both sides of it


def test_the_seeded_skins_are_what_the_tests_need(fixture_scene):
    a = fixture_scene
    lights = set(a.light_vertices())
    for bones in S.BONES:
        first, second, single = S.seeded_skins(a, bones)
        assert first.first == 1 and first.count % 64 != 0 and single.count == 1
        assert first.first + first.count <= second.first  # disjoint
        for s in (first, second, single):
            assert not lights & set(range(s.first, s.first + s.count))
            assert s.indices.max() < bones and np.all(s.weights >= 0)
            moved = np.setdiff1d(np.arange(s.count), s.unweighted)
            assert np.all(np.abs(s.weights[moved].sum(axis=1) - 1.0) < 1e-6) and not s.weights[s.unweighted].any()
        assert set(np.unique(second.influences())) == {0, 1, 2, 3, 4}


@pytest.mark.parametrize("bones", S.BONES)
def test_the_host_build_equals_the_numpy_restatement(fixture_scene, bones):
    a = fixture_scene
    for k, s in enumerate(S.seeded_skins(a, bones)):
        m = S.palette(bones, 20 + k, S.extent(a))
        got, bad = S.host_skin(s.rest, s.indices, s.weights, m)
        assert bad == 0
        assert np.array_equal(bits(got), bits(S.numpy_skin(s.rest, s.indices, s.weights, m)))
        moved = np.setdiff1d(np.arange(s.count), s.unweighted)
        assert not np.array_equal(got["p"][moved], s.rest["p"][moved])
        assert np.array_equal(got["t"], s.rest["t"])  # uvs are copied
        for f in ("n", "b"):  # unit length, or the rest vector where there is nothing to normalise
            length = np.linalg.norm(got[f][moved].astype(np.float64), axis=1)
            nothing = np.linalg.norm(s.rest[f][moved].astype(np.float64), axis=1) == 0
            assert np.all(np.abs(length[~nothing] - 1.0) < 1e-6) and np.array_equal(got[f][moved][nothing], s.rest[f][moved][nothing])


@pytest.mark.parametrize("bones", S.BONES)
def test_identity_palettes_reproduce_the_rest_positions(fixture_scene, bones):
    """Under identity matrices t_i is p_i exactly ((1*p0 + 0*p1) + 0*p2 + 0, up to the sign of a zero), so a vertex with ONE influence
    of weight 1 gets its rest position back as a value.  With several influences the position is sum_k fl(w_k * p): the float32
    weights sum to 1 within 2^-25 * 4, each of the four products and three additions rounds by at most 2^-24 of a magnitude <= |p|,
    so the result lies within 8 * 2^-24 = 2^-21 of |p| -- the bound asserted here, not an exact equality."""
    a = fixture_scene
    for s in S.seeded_skins(a, bones):
        one = S.exact_identity_skin(a, s)
        one.weights[:] = 0.0
        one.weights[:, 3] = 1.0  # every vertex, one influence
        got, _ = S.host_skin(one.rest, one.indices, one.weights, S.identity_palette(bones))
        assert np.array_equal(got["p"], s.rest["p"])  # (as values: -0.0 may have become +0.0)
        got, _ = S.host_skin(s.rest, s.indices, s.weights, S.identity_palette(bones))
        assert np.all(np.abs(got["p"] - s.rest["p"]) <= np.abs(s.rest["p"]) * np.float32(2.0 ** -21))
        single = s.influences() == 1
        exact = single & (s.weights.max(axis=1) == 1.0)
        assert np.array_equal(got["p"][exact], s.rest["p"][exact])
        # and the skin the GPU test poses back with: bytes of the rest pose
        e = S.exact_identity_skin(a, s)
        got, _ = S.host_skin(e.rest, e.indices, e.weights, S.identity_palette(bones))
        assert np.array_equal(bits(got), bits(e.rest))
    assert len(S.exact_identity_skin(a, S.seeded_skins(a, bones)[0]).unweighted) < S.seeded_skins(a, bones)[0].count // 2


def test_a_vertex_without_weights_keeps_its_record_bytewise(fixture_scene):
    a = fixture_scene
    s = S.seeded_skins(a, 3)[1]
    assert len(s.unweighted) >= 8
    odd = s.rest.copy()  # records no pose would leave alone: a NaN normal, a -0.0, a denormal
    odd["n"][s.unweighted[0]] = np.nan
    odd["p"][s.unweighted[1]] = -0.0
    odd["b"][s.unweighted[2]] = 1e-42
    got, bad = S.host_skin(odd, s.indices, s.weights, S.palette(3, 5, S.extent(a)))
    assert bad == 0 and np.array_equal(bits(got[s.unweighted]), bits(odd[s.unweighted]))


def test_a_blended_normal_without_length_falls_back_to_the_rest_normal(fixture_scene):
    """two bones whose linear parts are I and -I at weights of one half each: 0.5 * n + 0.5 * (-n) is exactly zero"""
    a = fixture_scene
    s = S.seeded_skins(a, 3)[1]
    m = S.identity_palette(2)
    m[1, :, :3] *= -1.0
    m[1, :, 3] = (0.25, -0.5, 0.125)
    idx = np.tile(np.array([0, 1, 0, 1], dtype=np.uint16), (s.count, 1))
    w = np.tile(np.array([0.5, 0.5, 0.0, 0.0], dtype=np.float32), (s.count, 1))
    got, bad = S.host_skin(s.rest, idx, w, m)
    assert bad == 0
    assert np.array_equal(bits(got["n"]), bits(s.rest["n"])) and np.array_equal(bits(got["b"]), bits(s.rest["b"]))
    assert np.isfinite(got["p"]).all() and not np.array_equal(got["p"], s.rest["p"])
    assert np.array_equal(bits(got), bits(S.numpy_skin(s.rest, idx, w, m)))


def test_the_check_counts_used_vertices_without_a_finite_position(fixture_scene):
    a = fixture_scene
    s = S.seeded_skins(a, 3)[1]
    m = S.palette(3, 5, S.extent(a))
    m[1, 0, 3] = np.inf
    reached = np.arange(s.count)[((s.indices == 1) & (s.weights != 0)).any(axis=1)]
    assert 0 < len(reached) < s.count
    got, bad = S.host_skin(s.rest, s.indices, s.weights, m)
    assert bad == len(reached) and not np.isfinite(got["p"][reached]).all(axis=1).any()
    used = np.ones(s.count, dtype=np.uint8)
    used[reached[0]] = 0  # (a free slot of the pool may hold anything)
    assert S.host_skin(s.rest, s.indices, s.weights, m, used=used)[1] == len(reached) - 1
    with np.errstate(all="ignore"):
        assert np.array_equal(bits(got), bits(S.numpy_skin(s.rest, s.indices, s.weights, m)))


def test_bad_influences_are_named(fixture_scene):
    import ctypes as C
    a = fixture_scene
    s = S.seeded_skins(a, 3)[0]
    out, bad = np.zeros(s.count, dtype=hip.VERTEX_DTYPE), C.c_uint32(0)
    m = S.identity_palette(3)

    def rc(indices, weights):
        return S.skin_lib().hostsim_skin_vertices(s.rest.ctypes.data, indices.ctypes.data, weights.ctypes.data, s.count, m.ctypes.data, 3, None,
                                                  out.ctypes.data, C.byref(bad))

    idx = s.indices.copy()
    idx[-1, 3] = 3
    assert rc(s.indices, s.weights) == 0 and rc(idx, s.weights) == 1
    for w_bad in (-0.25, np.nan, np.inf):
        w = s.weights.copy()
        w[0, 0] = w_bad
        assert rc(s.indices, w) == 2


def test_the_seeded_poses_leave_no_triangle_without_area(fixture_scene):
    """the refit of host-skinned vertices (tests/hostsim/hostsim_refit.cpp): every triangle keeps its area, so the frames of
    tests/test_gpu_skinning.py compare scenes in which every record is a real plane"""
    assert V.have_refit_lib(), "tests/hostsim/hostsim_refit.cpp is not built (run __graft_entry__.build())"
    a = fixture_scene
    for bones in S.BONES:
        skins = S.seeded_skins(a, bones)[:2]
        for seed in (31, 32):
            v = S.host_posed(a, skins, [S.palette(bones, seed + k, S.extent(a)) for k in range(2)])
            recs, _, n_degenerate = V.host_refit(a, v)
            assert n_degenerate == 0 and not np.array_equal(recs, a.tris)
            outside = np.setdiff1d(np.arange(len(v)), np.concatenate([np.arange(s.first, s.first + s.count) for s in skins]))
            assert np.array_equal(bits(v[outside]), bits(a.vertices[outside]))
