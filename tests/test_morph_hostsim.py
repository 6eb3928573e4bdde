"""Morph targets without a GPU (ray_amd/csrc/morph.h through tests/hostsim/hostsim_morph.cpp): the host build of the element functions
equals an independent numpy restatement bit for bit, the composition with a skin is the skin applied to the morphed records, the row
table is the one a slow sort makes, malformed descriptions are refused, and the seeded poses of tests/morph_cases.py leave no triangle
without area -- which is what licenses the frame comparisons of tests/test_gpu_morph.py."""
import numpy as np
import pytest

import morph_cases as M
import skin_cases as S
import vertex_update_cases as V

bits = M.bits


@pytest.fixture(scope="module")
def fixture_scene():
    assert M.have_morph_lib(), "tests/hostsim/hostsim_morph.cpp is not built (run __graft_entry__.build())"
    assert S.have_skin_lib(), "tests/hostsim/hostsim_skin.cpp is not built (run __graft_entry__.build())"
    return S.scene()[1]


def test_the_host_build_exists_and_knows_the_lds_cap():
    assert M.have_morph_lib(), "tests/hostsim/hostsim_morph.cpp is not built (run __graft_entry__.build())"
    cap = int(M.morph_lib().hostsim_morph_lds_targets())
    assert cap == 1024 and max(M.TARGETS) == cap + 1 and min(M.TARGETS) == 1  # the weight arrays of the tests lie on both sides of it


def test_the_seeded_sets_are_what_the_tests_need(fixture_scene):
    a = fixture_scene
    first, count = M.standalone_range(a)
    lights = set(a.light_vertices())
    assert first == 1 and count % 64 != 0 and not lights & set(range(first, first + count))
    one, three, many = (M.seeded_set(a, first, count, t, 5) for t in M.TARGETS)
    for ms in (one, three, many):
        lengths = ms.row_lengths()
        assert (lengths == 0).any()  # rows of length 0
        for vertices, dp, dn, db in ms.targets:
            assert np.all(np.diff(vertices.astype(np.int64)) > 0) and (len(vertices) == 0 or vertices[-1] < count)
    assert (one.row_lengths() == 1).any() and three.row_lengths()[0] == 3  # a row with an entry for every target
    assert three.row_lengths()[count - 1] == 1 and count - 1 in three.targets[1][0] and M.seeded_weights(3, 1)[1] == 0  # only entries of weight 0
    assert three.targets[1][2] is None and three.targets[1][3] is None  # a target without dn / db
    assert len(many.targets[500][0]) == 0 and sorted(set(many.row_lengths())) == [0, 1024]  # a target with count == 0; dense on a few vertices
    for t in M.TARGETS:
        for seed in (1, 2):
            w = M.seeded_weights(t, seed)
            assert np.isfinite(w).all() and (w.min() == np.float32(-0.5) or t == 1) and (w.max() == np.float32(1.5) or t == 1)
    assert {float(M.seeded_weights(1, 1)[0]), float(M.seeded_weights(1, 2)[0])} == {-0.5, 1.5}


@pytest.mark.parametrize("targets", M.TARGETS)
def test_the_row_table_equals_a_table_built_in_python(fixture_scene, targets):
    a = fixture_scene
    first, count = M.standalone_range(a)
    ms = M.seeded_set(a, first, count, targets, 9)
    row, entries = M.host_rows(ms.targets, count)
    want_row, want_entries = M.python_rows(ms.targets, count)
    assert np.array_equal(row, want_row) and np.array_equal(entries.view(np.uint32), want_entries.view(np.uint32))
    assert np.array_equal(np.diff(row.astype(np.int64)), ms.row_lengths())
    for v in range(count):
        assert np.all(np.diff(entries["target"][row[v]:row[v + 1]].astype(np.int64)) > 0)  # ascending target within a vertex


def test_the_row_table_of_shuffled_target_lists(fixture_scene):
    """targets over seeded shuffles of the vertices, of every length from none to all: the counting sort against the slow sort"""
    a = fixture_scene
    rng = np.random.RandomState(4)
    count = 50
    ext = S.extent(a)
    targets = [M._target(rng, rng.permutation(count)[:n], ext, 1.0, with_frame=bool(n % 3)) for n in rng.permutation(count + 1)[:24]]
    row, entries = M.host_rows(targets, count)
    want_row, want_entries = M.python_rows(targets, count)
    assert np.array_equal(row, want_row) and np.array_equal(entries.view(np.uint32), want_entries.view(np.uint32))


@pytest.mark.parametrize("targets", M.TARGETS)
def test_the_host_build_equals_the_numpy_restatement(fixture_scene, targets):
    a = fixture_scene
    first, count = M.standalone_range(a)
    ms = M.seeded_set(a, first, count, targets, 5)
    for seed in (1, 2):
        w = M.seeded_weights(targets, seed)
        got, bad = M.host_morph(ms, w)
        assert bad == 0
        assert np.array_equal(bits(got), bits(M.numpy_morph(ms.base, ms.targets, w)))
        assert np.array_equal(got["t"], ms.base["t"])  # uvs are copied
        untouched = ms.row_lengths() == 0
        assert np.array_equal(bits(got[untouched]), bits(ms.base[untouched]))
        assert not np.array_equal(got["p"][~untouched], ms.base["p"][~untouched])
        if targets == 3:  # the row whose only entry has weight 0: the base record bytewise
            assert np.array_equal(bits(got[count - 1]), bits(ms.base[count - 1]))
    # all weights 0: the base records
    got, _ = M.host_morph(ms, np.zeros(targets, dtype=np.float32))
    assert np.array_equal(bits(got), bits(ms.base))


def test_a_vertex_that_no_weighted_target_moves_keeps_its_record_bytewise(fixture_scene):
    a = fixture_scene
    first, count = M.standalone_range(a)
    ms = M.seeded_set(a, first, count, 3, 5)
    ms.base["n"][2] = np.nan  # (vertex 2: in no target; the last vertex: in target 1 only) records no pose would leave alone
    ms.base["p"][count - 1] = -0.0
    ms.base["b"][count - 1] = 1e-42
    got, bad = M.host_morph(ms, M.seeded_weights(3, 1))
    assert bad == 0 and np.array_equal(bits(got[[2, count - 1]]), bits(ms.base[[2, count - 1]]))
    with np.errstate(all="ignore"):
        assert np.array_equal(bits(got), bits(M.numpy_morph(ms.base, ms.targets, M.seeded_weights(3, 1))))


def test_a_morphed_normal_without_length_falls_back_to_the_base_normal(fixture_scene):
    """one target whose normal delta is minus the normal, at weight 1: n + 1 * (-n) is exactly zero"""
    a = fixture_scene
    first, count = M.standalone_range(a)
    base = a.vertices[first:first + count]
    every = np.arange(count, dtype=np.uint32)
    ms = M.MorphSet(a, first, count, [(every, np.full((count, 3), 0.01, dtype=np.float32), -base["n"], -base["b"])])
    got, bad = M.host_morph(ms, [1.0])
    assert bad == 0 and np.array_equal(bits(got["n"]), bits(base["n"])) and np.array_equal(bits(got["b"]), bits(base["b"]))
    assert not np.array_equal(got["p"], base["p"])
    assert np.array_equal(bits(got), bits(M.numpy_morph(ms.base, ms.targets, [1.0])))


@pytest.mark.parametrize("bones", (3, 257))
@pytest.mark.parametrize("targets", M.TARGETS)
def test_morph_then_skin_is_the_skin_applied_to_the_morphed_records(fixture_scene, targets, bones):
    a = fixture_scene
    skin = S.seeded_skins(a, bones)[1]
    palette = S.palette(bones, 21, S.extent(a))
    for k, (first, count) in enumerate(M.ranges_inside(skin)):
        ms = M.seeded_set(a, first, count, targets, 6 + k)
        w = M.seeded_weights(targets, 1 + k)
        idx, sw = M.skin_part(skin, ms)
        got, bad = M.host_morph(ms, w, skin=(idx, sw), bones=palette)
        morphed, _ = M.host_morph(ms, w)
        want, want_bad = S.host_skin(morphed, idx, sw, palette)
        assert bad == want_bad == 0 and np.array_equal(bits(got), bits(want))
        assert np.array_equal(bits(got), bits(S.numpy_skin(M.numpy_morph(ms.base, ms.targets, w), idx, sw, palette)))
        # ... and it is not the skin alone: the skin's own rest record is not what is posed
        alone, _ = S.host_skin(ms.base, idx, sw, palette)
        assert not np.array_equal(bits(got), bits(alone))


def test_host_morphed_composes_plain_and_covered_segments(fixture_scene):
    a = fixture_scene
    skins = S.seeded_skins(a, 3)[:2]
    palettes = [S.palette(3, 30 + k, S.extent(a)) for k in range(2)]
    inside = [M.seeded_set(a, f, c, 3, 8 + k) for k, (f, c) in enumerate(M.ranges_inside(skins[1]))]
    weights = [M.seeded_weights(3, 1 + k) for k in range(2)]
    v = M.host_morphed(a, inside, weights, skins, palettes)
    plain = S.host_posed(a, skins, palettes)
    covered = np.zeros(len(v), dtype=bool)
    for ms in inside:
        covered[ms.first:ms.first + ms.count] = True
    assert np.array_equal(bits(v[~covered]), bits(plain[~covered])) and not np.array_equal(bits(v[covered]), bits(plain[covered]))


def test_the_check_counts_used_vertices_without_a_finite_position(fixture_scene):
    a = fixture_scene
    first, count = M.standalone_range(a)
    ms = M.seeded_set(a, first, count, 3, 5)
    w = np.array([3.0e38, 0.0, 1.0], dtype=np.float32)
    ms.targets[0] = (ms.targets[0][0], np.full_like(ms.targets[0][1], 2.0), ms.targets[0][2], ms.targets[0][3])  # 3e38 * 2 overflows
    reached = ms.targets[0][0]
    with np.errstate(all="ignore"):
        got, bad = M.host_morph(ms, w)
        assert bad == len(reached) and not np.isfinite(got["p"][reached]).all(axis=1).any()
        used = np.ones(count, dtype=np.uint8)
        used[reached[0]] = 0  # (a free slot of the pool may hold anything)
        assert M.host_morph(ms, w, used=used)[1] == len(reached) - 1
        assert np.array_equal(bits(got), bits(M.numpy_morph(ms.base, ms.targets, w)))


def test_malformed_descriptions_are_refused(fixture_scene):
    """every one with the code rayhip_morph_create gives it (1), and for the reason meant (morph.h: validate_targets)"""
    a = fixture_scene
    first, count = M.standalone_range(a)
    ms = M.seeded_set(a, first, count, 3, 5)
    assert M.host_validate(ms.targets, count) == (0, 0)
    assert M.host_validate(ms.targets, count, targets_count=0) == (1, 5) and M.host_validate(ms.targets, count, targets_count=65537) == (1, 5)
    vertices, dp, dn, db = ms.targets[0]

    def with_first(t):
        return [t] + ms.targets[1:]

    assert M.host_validate(with_first((vertices, None, dn, db)), count) == (1, 1)  # no position deltas
    swapped = vertices.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    twice = vertices.copy()
    twice[1] = twice[0]
    beyond = vertices.copy()
    beyond[-1] = count
    for bad in (swapped, twice, beyond):
        assert M.host_validate(with_first((bad, dp, dn, db)), count) == (1, 2)
    for k, value in ((1, np.nan), (2, np.inf), (3, -np.inf)):
        t = [vertices, dp.copy(), dn.copy(), db.copy()]
        t[k][-1, 2] = value
        assert M.host_validate(with_first(tuple(t)), count) == (1, 3)


def test_the_seeded_poses_leave_no_triangle_without_area(fixture_scene):
    """the refit of host-morphed vertices (tests/hostsim/hostsim_refit.cpp): every triangle keeps its area, so the frames of
    tests/test_gpu_morph.py compare scenes in which every record is a real plane"""
    assert V.have_refit_lib(), "tests/hostsim/hostsim_refit.cpp is not built (run __graft_entry__.build())"
    a = fixture_scene
    skins = S.seeded_skins(a, 3)[:2]
    palettes = [S.palette(3, 60 + k, S.extent(a)) for k in range(2)]
    first, count = M.standalone_range(a)
    for targets in M.TARGETS:
        sets = [M.seeded_set(a, f, c, targets, 8 + k) for k, (f, c) in enumerate(M.ranges_inside(skins[1]))]
        weights = [M.seeded_weights(targets, 1 + k) for k in range(2)]
        alone = M.seeded_set(a, first, count, targets, 5)
        for v in (M.host_morphed(a, sets, weights, skins[1:], palettes[1:]), M.host_morphed(a, [alone], [M.seeded_weights(targets, 1)])):
            recs, _, n_degenerate = V.host_refit(a, v)
            assert n_degenerate == 0 and not np.array_equal(recs, a.tris)
