"""The tree builders and the wide node test, host build (tests/hostsim/hostsim_bvh.cpp), against the independent checker of
tests/bvh_build_cases.py: build_host of lbvh.h, the host collapse of bvh4_build.h (wide_children, quantise) and bvh4_test_node of
rt_bvh4.h.  tests/test_gpu_bvh_builders.py holds the device kernels against the same checker and against this build."""
import os
from fractions import Fraction

import numpy as np
import pytest

import bvh_build_cases as B

LEAF_SIZES = (1, 2, 4, 8)


@pytest.fixture(scope="module")
def host():
    if not os.path.exists(B.HOST_LIB):
        pytest.skip("host build of the builders missing (__graft_entry__.build())")
    return B.Host()


def _configs():
    for flags in (B.REFINE, B.MESH, B.TOP):
        for leaf_max in ((1,) if flags == B.TOP else LEAF_SIZES):  # (the top level is built with leaves of one instance)
            yield flags, leaf_max


# ---- hand-worked small cases: equal keys, the index tie-break alone shapes the tree ---------------------------------------------------
def _same_box(n):
    """n boxes around one centroid (1, 2, 3), half extent i + 1: every key is equal, the boxes are told apart by their size"""
    c, h = np.array([[1, 2, 3]], np.float32), np.arange(1, n + 1, dtype=np.float32)[:, None]
    return np.concatenate([c - h, c + h], 1)


def test_hand_worked_n1(host):
    b, g = _same_box(1), np.zeros(1, np.uint32)
    out = host.k_lbvh_build(b, g, 1, 2, *B.REFINE)  # refinement: the group is one leaf, its primitive written twice
    assert len(out["nodes"]) == 0 and out["entries"].tolist() == [0, 0] and out["group_root"].tolist() == [1 << 29]
    out = host.k_lbvh_build(b, g, 1, 2, *B.MESH)  # a mesh of one triangle: a node with the triangle on both sides
    assert out["entries"].tolist() == [0, 0] and out["group_root"].tolist() == [0]
    assert np.array_equal(out["nodes"][0], B.make_node(b[0, :3], b[0, 3:], 1 << 29, b[0, :3], b[0, 3:], 1 << 29))
    out = host.k_lbvh_build(b, g, 1, 1, *B.TOP)  # top level: the second child is the point at FLT_MAX
    far = np.full(3, B.FLT_MAX, np.float32)
    assert out["group_root"].tolist() == [0]
    assert np.array_equal(out["nodes"][0], B.make_node(b[0, :3], b[0, 3:], 1 << 29, far, far, 1 << 29))
    assert np.array_equal(out["bounds"], b[0])


def test_hand_worked_n2(host):
    b, g = _same_box(2), np.zeros(2, np.uint32)
    out = host.k_lbvh_build(b, g, 1, 2, *B.REFINE)  # two primitives fit one leaf
    assert len(out["nodes"]) == 0 and out["entries"].tolist() == [0, 1] and out["group_root"].tolist() == [1 << 29]
    for flags, leaf_max, entries, links in ((B.MESH, 2, [0, 0, 1, 1], (1 << 29 | 0, 1 << 29 | 2)), (B.REFINE, 1, [0, 0, 1, 1], (1 << 29 | 0, 1 << 29 | 2)),
                                            (B.TOP, 1, [0, 0, 1, 1], (1 << 29 | 0, 1 << 29 | 1))):
        out = host.k_lbvh_build(b, g, 1, leaf_max, *flags)  # a root that has to be a node: each primitive a leaf of its own
        assert out["entries"].tolist() == entries and out["group_root"].tolist() == [0]
        assert np.array_equal(out["nodes"], B.make_node(b[0, :3], b[0, 3:], links[0], b[1, :3], b[1, 3:], links[1])[None])
    assert np.array_equal(out["bounds"], b[1])


def test_hand_worked_n3(host):
    """keys 0 0 0: the prefixes come from the indices 00 01 10, so the root splits {0, 1} | {2}"""
    b, g = _same_box(3), np.zeros(3, np.uint32)
    u01 = (b[1, :3], b[1, 3:])
    out = host.k_lbvh_build(b, g, 1, 2, *B.MESH)
    assert out["entries"].tolist() == [0, 1, 2, 2] and out["group_root"].tolist() == [0]
    assert np.array_equal(out["nodes"], B.make_node(*u01, 1 << 29 | 0, b[2, :3], b[2, 3:], 1 << 29 | 2)[None])
    out = host.k_lbvh_build(b, g, 1, 1, *B.MESH)
    assert out["entries"].tolist() == [0, 0, 1, 1, 2, 2]
    want = np.stack([B.make_node(*u01, 1, b[2, :3], b[2, 3:], 1 << 29 | 4), B.make_node(b[0, :3], b[0, 3:], 1 << 29 | 0, b[1, :3], b[1, 3:], 1 << 29 | 2)])
    assert np.array_equal(out["nodes"], want) and out["group_root"].tolist() == [0]
    out = host.k_lbvh_build(b, g, 1, 4, *B.REFINE)
    assert len(out["nodes"]) == 0 and out["entries"].tolist() == [0, 1, 2] and out["group_root"].tolist() == [2 << 29]
    # two groups, one empty between them: 0 -> {0, 2}, 1 -> {}, 2 -> {1}
    out = host.k_lbvh_build(b, np.array([0, 2, 0], np.uint32), 3, 2, *B.REFINE)
    assert out["entries"].tolist() == [0, 2, 1, 1] and out["group_root"].tolist() == [1 << 29 | 0, B.NONE, 1 << 29 | 2] and len(out["nodes"]) == 0


# ---- every case through the host build and the checker ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def prim_cases():
    return B.prim_cases()


@pytest.mark.parametrize("flags,leaf_max", list(_configs()))
def test_linear_builder_and_collapse_of_its_trees(host, prim_cases, flags, leaf_max):
    for name, (boxes, groups, n_groups) in prim_cases.items():
        out = host.k_lbvh_build(boxes, groups, n_groups, leaf_max, *flags)
        try:
            B.check_lbvh(boxes, groups, n_groups, leaf_max, flags, out)
            roots = B.node_roots(out)
            if flags != B.TOP and len(roots):  # (the top level stays two-wide)
                wide, roots4 = host.k_bvh4_collapse(out["nodes"], roots)
                B.check_collapse(out["nodes"], roots, wide, roots4)
        except AssertionError as e:
            raise AssertionError(f"case {name}: {e}") from e


def test_zero_primitives(host):
    out = host.k_lbvh_build(np.zeros((0, 6), np.float32), np.zeros(0, np.uint32), 3, 2, *B.REFINE)
    B.check_lbvh(np.zeros((0, 6), np.float32), np.zeros(0, np.uint32), 3, 2, B.REFINE, out)
    assert out["group_root"].tolist() == [B.NONE] * 3


def test_overflowing_centroids_are_built_and_the_wide_grid_clamps_them(host):
    """coordinates near FLT_MAX whose centroid sum is infinite: the linear builder's output is a correct tree (every Morton cell
    clamps); the collapse contains every child but (hi - lo) overflows in quantise and qhi clamps to plane 255, which is not the
    tightest plane.  Pinned as such; the device file leaves this collapse out."""
    boxes, groups, n_groups = B.overflow_case()
    out = host.k_lbvh_build(boxes, groups, n_groups, 2, *B.MESH)
    B.check_lbvh(boxes, groups, n_groups, 2, B.MESH, out)
    wide, roots4 = host.k_bvh4_collapse(out["nodes"], B.node_roots(out))
    with pytest.raises(AssertionError, match="tightness"):
        B.check_collapse(out["nodes"], B.node_roots(out), wide, roots4)


@pytest.mark.parametrize("name", ["large_refinement", "large_mesh"])
def test_large_case(host, name):
    (boxes, groups, n_groups), flags, leaf_max = B.large_cases()[name]
    out = host.k_lbvh_build(boxes, groups, n_groups, leaf_max, *flags)
    print(name, B.check_lbvh(boxes, groups, n_groups, leaf_max, flags, out))
    roots = B.node_roots(out)
    wide, roots4 = host.k_bvh4_collapse(out["nodes"], roots)
    B.check_collapse(out["nodes"], roots, wide, roots4)


HAND_TREES = {"chain_2000": B.chain_tree, "perfect": B.perfect_tree, "equal_half_areas": lambda: B.perfect_tree(8, equal_areas=True),
              "grid_edges": B.grid_edge_nodes}


@pytest.mark.parametrize("name", list(HAND_TREES))
def test_collapse_of_hand_made_trees(host, name):
    nodes, roots = HAND_TREES[name]()
    wide, roots4 = host.k_bvh4_collapse(nodes, roots)
    B.check_collapse(nodes, roots, wide, roots4)
    if name == "equal_half_areas":  # the tie rule: of two inner children with equal half-area the FIRST is opened first
        first = wide[roots4[0]]
        lo2, hi2, link2 = B.child_boxes(nodes)
        assert B.half_area32(lo2[0, 0], hi2[0, 0]) == B.half_area32(lo2[0, 1], hi2[0, 1])


def test_unquantisable_is_a_return_value_not_an_error(host):
    assert host.k_bvh4_collapse(*B.unquantisable_nodes()) is None


def test_a_forest_that_is_not_one_is_refused(host):
    nodes, roots = B.perfect_tree(3)
    nodes[1, 12] = 0  # a link back to the root
    with pytest.raises(RuntimeError):
        host.k_bvh4_collapse(nodes, roots)


def test_exact_plane_comparison_against_fractions():
    """the checker's plane_sign (float64 with the two-sum error term) is exact: held against rationals where float64 alone is not"""
    rng = np.random.default_rng(7)
    org = (rng.uniform(-1, 1, 400) * 2.0 ** rng.integers(-60, 60, 400)).astype(np.float32)
    step = (2.0 ** rng.integers(-120, 100, 400)).astype(np.float32)
    q = rng.integers(0, 256, 400)
    x = np.where(rng.uniform(size=400) < 0.5, (org.astype(np.float64) + q * step.astype(np.float64)).astype(np.float32), org)
    got = B.plane_sign(org, q, step, x)
    for i in range(400):
        exact = Fraction(float(org[i])) + int(q[i]) * Fraction(float(step[i])) - Fraction(float(x[i]))
        assert got[i] == (exact > 0) - (exact < 0), i


# ---- the node test ----------------------------------------------------------------------------------------------------------------------------
def test_node_visit_contract(host):
    """per ray category, over the wide nodes of five trees: whatever either reference accepts is reported hit, entry distances do not
    exceed the reference's, ref[] is a sorted permutation, empty slots are never hit.  The inputs' own condition first: in every
    category the fp32 reference accepts at least a fifth and rejects at least a fifth of the (item, child) pairs."""
    totals = {c: {"pairs": 0, "acc32": 0, "acc64": 0, "extra_hits": 0} for c in B.RAY_CATEGORIES}
    for tree, (nodes, roots) in B.node_test_trees(host).items():
        wide, roots4 = host.k_bvh4_collapse(nodes, roots)
        info, _ = B.check_collapse(nodes, roots, wide, roots4)
        info = B.with_grid(info, wide)
        pool = B.distinct_children(wide)
        assert len(pool) >= 0.9 * len(wide)
        for i, cat in enumerate(B.RAY_CATEGORIES):
            node, o, d, t = B.make_rays(cat, info, pool, 6000, 100 + i)
            try:
                c = B.check_node_test(info, wide, node, o, d, t, host.k_bvh4_test_nodes(wide, node, o, d, t))
            except AssertionError as e:
                raise AssertionError(f"tree {tree}, rays {cat}: {e}") from e
            for k in c:
                totals[cat][k] += c[k]
    for cat, c in totals.items():
        frac = c["acc32"] / c["pairs"]
        print(f"{cat:18s} pairs {c['pairs']:7d}  fp32 reference accepts {frac:.3f}  float64 {c['acc64'] / c['pairs']:.3f}  "
              f"hits both reject {c['extra_hits'] / c['pairs']:.3f}")
        assert 0.2 <= frac <= 0.8, (cat, frac)
