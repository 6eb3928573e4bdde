"""Normal sets without a GPU (ray_amd/csrc/normals.h through tests/hostsim/hostsim_normals.cpp): the host build of the element functions
against an independent numpy restatement bit for bit, against the bitangents the reference's scene build stored -- bit for bit, on the
committed fixtures and on every mesh of normals_cases.cloth -- and against a float64 model of the normals; the row tables against a slow
sort; and the preconditions of the scene and its poses that the GPU tests rely on."""
import os

import numpy as np
import pytest

import normals_cases as NC
import util
import vertex_update_cases as V
from ray_amd import hip

N, B = NC.N, NC.B
bits = NC.bits
ALL_POSES = (0,) + NC.POSES

# The largest angle between a float32 normal of the host build and the float64 model (area-weighted sums over the weld groups, from the same
# float32 positions), radians: measured here on the CPU over the upload pose and the three deformed poses, every mesh of `cloth`, with
# and without weld: 1.704e-06 -- test_normals_against_the_float64_model prints it.  It is a rim vertex of the fan (pose 2, no weld): its
# two faces are slivers of 1.2 degrees, whose cross products cancel in float32; the other meshes stay below 2e-7.  The test asserts four
# times this (the margin is for other seeds); the device adds nothing, it equals the host build to the bit.
MAX_ANGLE_MEASURED = 1.71e-6

# vertices whose bitangent is the raw tangent sum (b = T: no length left in cross(n, T), or no tangent at all), per mesh, at every pose:
# the four of the room are the ones the reference leaves so in every Cornell fixture
RAW_BITANGENTS = {"room": 4, "sheet": 0, "mirror": 0, "fan": 0, "sphere": 0}
TRIANGLES = {"room": 12, "sheet": 2 * 48 * 48, "mirror": 2 * 24 * 24, "fan": NC.FAN_TRIANGLES, "sphere": 2 * 16 * 7}
FALLBACK_FACES = {"room": 10, "sheet": 0, "mirror": 2 * 24, "fan": 0, "sphere": 0}  # faces without uv area (the axis fallback of the tangent)

pytestmark = pytest.mark.skipif(not NC.have_normals_lib(), reason="tests/hostsim is not built (run __graft_entry__.build())")


@pytest.fixture(scope="module")
def cloth():
    from ray_amd import api
    if not os.path.exists(api.HIP_HOST_LIB):
        pytest.skip("libray_hip.so not built (needs the reference tree at build time)")
    blob, a, meshes = NC.scene()
    return a, meshes, NC.reachable(a)


def _weld(a, first, count):
    return hip.weld_by_position(a.vertices["p"][first:first + count])


def _ranges(meshes):
    """every mesh whole; a range from vertex 1 whose length is no multiple of 64 and that ends inside the sheet; one that begins and ends
    inside the sheet -- faces straddle both ends"""
    sheet = meshes["sheet"]
    out = [(name, m.first, m.count) for name, m in meshes.items()]
    out += [("from vertex 1", 1, sheet.first + 1003), ("inside the sheet", sheet.first + 700, 901)]
    assert all(c % 64 != 0 for _, _, c in out[-2:])
    return out


def test_the_scene_and_its_poses_are_what_the_tests_assume(cloth):
    a, meshes, tris = cloth
    assert np.array_equal(NC.host_reachable(a), tris)
    assert np.array_equal(np.concatenate([meshes[name].tris for name in NC.MESHES]), tris.astype(np.int64))  # every mesh triangle is reachable
    corners = NC.corners_of(a)
    for name in NC.MESHES:
        m = meshes[name]
        assert len(m.tris) == TRIANGLES[name]
        c = corners[m.tris]
        assert c.min() == m.first and c.max() == m.first + m.count - 1
    assert [meshes[name].first for name in NC.MESHES] == sorted(meshes[name].first for name in NC.MESHES)
    # the scene build appended twins where it split vertices: the weld has something to do
    assert meshes["mirror"].count > 25 * 25 and meshes["sphere"].count > 2 + 7 * 17 and meshes["sheet"].count > 49 * 49
    for name in ("mirror", "sphere", "fan"):
        m = meshes[name]
        w = _weld(a, m.first, m.count)
        assert (w != np.arange(m.count)).sum() >= m.count - (25 * 25 if name == "mirror" else 2 + 7 * 16 if name == "sphere" else 301)
    rc, fan = NC.host_rows(a, tris, meshes["fan"].first, meshes["fan"].count)
    assert rc == 0 and int((fan["row"][1:] - fan["row"][:-1]).max()) > 256  # the hub's row is longer than a chunk of the device kernel
    for seed in ALL_POSES:
        v = NC.posed(a, meshes, seed)
        c = corners[tris.astype(np.int64)].astype(np.int64)
        plane, _, fallback = NC.numpy_face_frames(v[c[:, 0]], v[c[:, 1]], v[c[:, 2]])
        assert ((plane[:, 0] * plane[:, 0] + plane[:, 1] * plane[:, 1] + plane[:, 2] * plane[:, 2]) != 0).all()  # no triangle without area (refit.h's test)
        for name in NC.MESHES:
            m = meshes[name]
            assert int(fallback[np.isin(tris, m.tris)].sum()) == FALLBACK_FACES[name], name
            tb = NC.python_rows(a, tris, m.first, m.count)
            for flags in (B, N | B):
                _, raw = NC.numpy_recompute(a, v, tb, m.first, m.count, flags)
                assert int(raw.sum()) == RAW_BITANGENTS[name], (name, seed, flags)
    # at the upload pose the recomputed normals lie on the side of the uploaded ones, for every vertex in use
    for name in NC.MESHES:
        m = meshes[name]
        for weld in (None, _weld(a, m.first, m.count)):
            got = NC.host_recompute(a, a.vertices, tris, m.first, m.count, N, weld)[m.first:m.first + m.count]
            used = np.isin(np.arange(m.first, m.first + m.count), corners[m.tris])
            assert used.any() and ((got["n"] * a.vertices["n"][m.first:m.first + m.count]).sum(axis=1)[used] > 0).all()


@pytest.mark.parametrize("seed", ALL_POSES)
def test_the_host_build_equals_the_numpy_restatement(cloth, seed):
    a, meshes, tris = cloth
    v = NC.posed(a, meshes, seed)
    for name, first, count in _ranges(meshes):
        for weld in (None, _weld(a, first, count)):
            tb = NC.python_rows(a, tris, first, count, weld)
            for flags in (N, B, N | B):
                got = NC.host_recompute(a, v, tris, first, count, flags, weld)
                want, _ = NC.numpy_recompute(a, v, tb if flags & N else dict(tb, wrow=tb["wrow"][:0], wentries=tb["wentries"][:0]), first, count, flags)
                assert np.array_equal(bits(got), bits(want)), (name, flags, weld is not None)
                outside = np.r_[0:first, first + count:len(v)]
                assert np.array_equal(bits(got[outside]), bits(v[outside]))
                assert np.array_equal(bits(got["p"]), bits(v["p"])) and np.array_equal(bits(got["t"]), bits(v["t"]))
                if not flags & N:
                    assert np.array_equal(bits(got["n"]), bits(v["n"]))
                if not flags & B:
                    assert np.array_equal(bits(got["b"]), bits(v["b"]))
                if seed and name != "room":  # (the room is in no pose)
                    assert not np.array_equal(bits(got), bits(v))


def test_bitangents_equal_the_reference_scene_builds_on_every_fixture():
    """RAYHIP_NORMALS_B alone, one set over the whole vertex array of a committed scene: the bitangents the reference stored, bit for bit"""
    names = V.fixture_names()
    assert len(names) >= 7
    for name in names:
        a = V.Arrays(util.golden_scene(name))
        got = NC.host_recompute(a, a.vertices, NC.reachable(a), 0, len(a.vertices), B)
        assert np.array_equal(bits(got), bits(a.vertices)), name


def test_bitangents_equal_the_reference_scene_builds_on_every_mesh(cloth):
    """... and on meshes whose bitangents the scene build derived from real uvs: twins, a mirrored u, faces without uv area, a long fan"""
    a, meshes, tris = cloth
    for name in NC.MESHES:
        m = meshes[name]
        assert np.array_equal(bits(NC.host_recompute(a, a.vertices, tris, m.first, m.count, B)), bits(a.vertices)), name
    assert np.array_equal(bits(NC.host_recompute(a, a.vertices, tris, 0, len(a.vertices), B)), bits(a.vertices))
    junk = a.vertices.copy()
    junk["b"] = 7.0  # (what arrives in b is not read)
    used = np.unique(NC.corners_of(a)[tris.astype(np.int64)])
    assert np.array_equal(bits(NC.host_recompute(a, junk, tris, 0, len(a.vertices), B)[used]), bits(a.vertices[used]))


def test_normals_against_the_float64_model(cloth):
    a, meshes, tris = cloth
    worst = 0.0
    for seed in ALL_POSES:
        v = NC.posed(a, meshes, seed)
        for name in NC.MESHES:
            m = meshes[name]
            for weld in (None, _weld(a, m.first, m.count)):
                got = NC.host_recompute(a, v, tris, m.first, m.count, N, weld)["n"][m.first:m.first + m.count]
                model = NC.float64_normals(a, v, tris, m.first, m.count, weld)
                has = ~np.isnan(model[:, 0])
                assert has.any()
                worst = max(worst, float(NC.angle(got[has], model[has]).max()))
                assert np.abs(np.linalg.norm(got[has].astype(np.float64), axis=1) - 1.0).max() < 2.0e-7
    print(f"largest angle between the host build's normals and the float64 model: {worst:.3e} rad (MAX_ANGLE_MEASURED = {MAX_ANGLE_MEASURED:.3e})")
    assert worst <= 4.0 * MAX_ANGLE_MEASURED


def test_the_row_tables_equal_a_slow_sort(cloth):
    a, meshes, tris = cloth
    for name, first, count in _ranges(meshes):
        for weld in (None, _weld(a, first, count)):
            rc, got = NC.host_rows(a, tris, first, count, weld)
            want = NC.python_rows(a, tris, first, count, weld)
            assert rc == 0
            for key in want:
                assert np.array_equal(got[key], want[key]), (name, key)
            n = np.diff(got["row"].astype(np.int64))
            assert n.sum() == len(got["entries"]) and (got["entries"] < len(got["faces"])).all() and (np.diff(got["faces"].astype(np.int64)) > 0).all()
            for i in np.flatnonzero(n > 1)[:50]:
                assert (np.diff(got["entries"][got["row"][i]:got["row"][i + 1]].astype(np.int64)) >= 0).all()  # a row is in ascending face order


def test_weld_by_position_and_welded_normals(cloth):
    a, meshes, tris = cloth
    p = np.array([[1, 2, 3], [0, 0, 0], [1, 2, 3], [-0.0, 0, 0], [1, 2, 3], [5, 5, 5]], dtype=np.float32)
    assert hip.weld_by_position(p).tolist() == [0, 1, 0, 3, 0, 5] and hip.weld_by_position(p).dtype == np.uint32  # (bytewise: -0.0 is not 0.0)
    assert hip.weld_by_position(np.zeros((0, 3), dtype=np.float32)).shape == (0,)
    for name in ("sphere", "mirror"):
        m = meshes[name]
        w = _weld(a, m.first, m.count)
        assert NC.host_validate(len(a.vertices), m.first, m.count, N, w) == (0, 0) and (w[w] == w).all() and (w <= np.arange(m.count)).all()
        grouped = np.flatnonzero(w != np.arange(m.count))
        assert len(grouped) > 0
        for seed in (0, 2):
            v = NC.posed(a, meshes, seed)
            assert np.array_equal(bits(v["p"][m.first + grouped]), bits(v["p"][m.first + w[grouped]]))  # coincident vertices move together
            got = NC.host_recompute(a, v, tris, m.first, m.count, N | B, w)[m.first:m.first + m.count]
            assert np.array_equal(bits(got["n"][grouped]), bits(got["n"][w[grouped]]))
            alone = NC.host_recompute(a, v, tris, m.first, m.count, N | B)[m.first:m.first + m.count]
            assert not np.array_equal(bits(alone["n"][grouped]), bits(alone["n"][w[grouped]]))  # (without the weld the twins' normals part)


def test_vertices_without_a_face_keep_their_bytes(cloth):
    a, meshes, tris = cloth
    used = np.unique(NC.corners_of(a)[tris.astype(np.int64)])
    free = np.setdiff1d(np.arange(len(a.vertices)), used)
    assert len(free) > 0  # (the vertex array is a pool: its tail is in no triangle)
    v = NC.posed(a, meshes, 1)
    v["n"][free], v["b"][free], v["p"][free] = 3.0, np.nan, -7.0
    for weld in (None, np.arange(len(v), dtype=np.uint32)):
        got = NC.host_recompute(a, v, tris, 0, len(v), N | B, weld)
        assert np.array_equal(bits(got[free]), bits(v[free])) and not np.array_equal(bits(got[used]), bits(v[used]))


def test_faces_and_neighbourhoods_without_area(cloth):
    a, meshes, tris = cloth
    one = a.vertices[meshes["fan"].first:meshes["fan"].first + 1]
    assert not NC.host_face(np.concatenate([one, one, one])).any()  # three corners in one place: no normal, no tangent
    # every corner of the fan in one place: the sums are zero, every vertex keeps the normal it arrived with -- and b = T = 0
    fan = meshes["fan"]
    v = a.vertices.copy()
    v["p"][fan.first:fan.first + fan.count] = v["p"][fan.first]
    arrived = np.random.RandomState(2).uniform(-1.0, 1.0, size=(fan.count, 3)).astype(np.float32)
    v["n"][fan.first:fan.first + fan.count] = arrived
    got = NC.host_recompute(a, v, tris, fan.first, fan.count, N | B)[fan.first:fan.first + fan.count]
    used = np.isin(np.arange(fan.first, fan.first + fan.count), NC.corners_of(a)[fan.tris])
    assert used.all() and np.array_equal(bits(got["n"]), bits(arrived)) and not got["b"].any()
    # one collapsed face among sound ones contributes nothing: the others' sum is the normal
    t = int(fan.tris[5])
    c = NC.corners_of(a)[t]
    v = a.vertices.copy()
    rim = [int(i) for i in c if (NC.corners_of(a)[fan.tris] == i).sum() == 2]  # a rim vertex: in two triangles
    assert rim
    w = v.copy()
    w["p"][rim[0]] = w["p"][[int(i) for i in c if i != rim[0]][0]]  # (collapses t; the rim vertex's other triangle keeps an area)
    got = NC.host_recompute(a, w, tris, fan.first, fan.count, N)
    others = np.array([x for x in fan.tris if x != t], dtype=np.uint32)
    assert np.array_equal(bits(got[rim[0]]), bits(NC.host_recompute(a, w, others, fan.first, fan.count, N)[rim[0]]))


def test_malformed_descriptions_are_refused(cloth):
    a, meshes, tris = cloth
    n = len(a.vertices)
    ok = np.arange(8, dtype=np.uint32)
    assert NC.host_validate(n, 4, 8, N | B, ok) == (0, 0) and NC.host_validate(n, n - 8, 8, B) == (0, 0)
    assert NC.host_validate(n, 4, 0, N)[0] == 1 and NC.host_validate(n, n - 7, 8, N)[0] == 1 and NC.host_validate(n, 0xffffffff, 2, N)[0] == 1
    assert NC.host_validate(n, 4, 8, 0) == (1, 1) and NC.host_validate(n, 4, 8, 4) == (1, 1) and NC.host_validate(n, 4, 8, 7) == (1, 1)
    beyond = ok.copy()
    beyond[5] = 8
    assert NC.host_validate(n, 4, 8, N, beyond) == (1, 2)
    chain = ok.copy()
    chain[3], chain[2] = 2, 1
    assert NC.host_validate(n, 4, 8, N, chain) == (1, 3)
