"""The device tree builders (lbvh.hip.h: k_keys .. k_emit; bvh4_build.hip.h: k_collapse_level) and the wide node test on the
device (rt_bvh4.h: bvh4_test_node, the pinned-fetch form), through the hooks rayhip_k_lbvh_build / _bvh4_collapse / _bvh4_test_nodes.

For every case: the device output equals the host build's word for word (the wide array after canonical renumbering: the device
lays nodes out breadth-first, the host depth-first), AND the independent checker of tests/bvh_build_cases.py passes on the device
output itself, so nothing here rests on the host build being right.  Inputs that the host build clamps (the overflowing centroids'
collapse) are pinned in tests/test_bvh_builders_hostsim.py and left out here."""
import os

import numpy as np
import pytest

import bvh_build_cases as B
from ray_amd import hip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    L = hip.Library()
    if L.device_count() <= 0:
        pytest.skip("no HIP device")
    if not os.path.exists(B.HOST_LIB):
        pytest.skip("host build of the builders missing (__graft_entry__.build())")
    return L


@pytest.fixture
def builders(lib):
    ctx = hip.Context(0, lib)
    yield B.Device(ctx), B.Host()
    ctx.close()


def _configs():
    for flags in (B.REFINE, B.MESH, B.TOP):
        for leaf_max in ((1,) if flags == B.TOP else (1, 2, 4, 8)):
            yield flags, leaf_max


def _both_collapses(dev, host, nodes, roots):
    """device and host collapse of the same BVH2: the checker on the device's, canonical forms equal; -> (wide, info) of the device"""
    wide_d, roots_d = dev.k_bvh4_collapse(nodes, roots)
    wide_h, roots_h = host.k_bvh4_collapse(nodes, roots)
    info, canon_d = B.check_collapse(nodes, roots, wide_d, roots_d)
    _, canon_h = B.check_collapse(nodes, roots, wide_h, roots_h)
    assert canon_d.shape == canon_h.shape and np.array_equal(canon_d, canon_h), "wide nodes differ after renumbering"
    return wide_d, info


@pytest.mark.parametrize("flags,leaf_max", list(_configs()))
def test_device_builders_equal_the_host_build_and_pass_the_checker(builders, flags, leaf_max):
    dev, host = builders
    cases = dict(B.prim_cases())
    cases["overflowing_centroids"] = B.overflow_case()  # (the linear builder only: its collapse is clamped, pinned on the CPU)
    for name, (boxes, groups, n_groups) in cases.items():
        try:
            out = dev.k_lbvh_build(boxes, groups, n_groups, leaf_max, *flags)
            B.check_lbvh(boxes, groups, n_groups, leaf_max, flags, out)
            B.same_lbvh(out, host.k_lbvh_build(boxes, groups, n_groups, leaf_max, *flags))
            roots = B.node_roots(out)
            if flags != B.TOP and len(roots) and name != "overflowing_centroids":
                _both_collapses(dev, host, out["nodes"], roots)
        except AssertionError as e:
            raise AssertionError(f"case {name}: {e}") from e


def test_zero_primitives(builders):
    dev, _ = builders
    out = dev.k_lbvh_build(np.zeros((0, 6), np.float32), np.zeros(0, np.uint32), 3, 2, *B.REFINE)
    B.check_lbvh(np.zeros((0, 6), np.float32), np.zeros(0, np.uint32), 3, 2, B.REFINE, out)


@pytest.mark.parametrize("name", ["large_refinement", "large_mesh"])
def test_large_case_across_blocks_twice(builders, name):
    """2^20 + 3 primitives: 4097 blocks per kernel, more than the device holds at once, so k_fit's second-to-arrive protocol,
    k_parents and the index hand-out of k_collapse_level run across blocks and compute dies.  Two runs in one process: identical
    linear-builder arrays; the wide array only after renumbering -- its raw order legitimately depends on the order in which threads
    take indices from the atomic counter"""
    dev, host = builders
    (boxes, groups, n_groups), flags, leaf_max = B.large_cases()[name]
    out = dev.k_lbvh_build(boxes, groups, n_groups, leaf_max, *flags)
    print(name, B.check_lbvh(boxes, groups, n_groups, leaf_max, flags, out))
    B.same_lbvh(out, host.k_lbvh_build(boxes, groups, n_groups, leaf_max, *flags))
    B.same_lbvh(out, dev.k_lbvh_build(boxes, groups, n_groups, leaf_max, *flags))
    roots = B.node_roots(out)
    _both_collapses(dev, host, out["nodes"], roots)
    wide2, roots2 = dev.k_bvh4_collapse(out["nodes"], roots)
    wide1, roots1 = dev.k_bvh4_collapse(out["nodes"], roots)
    assert np.array_equal(B.check_collapse(out["nodes"], roots, wide1, roots1)[1], B.check_collapse(out["nodes"], roots, wide2, roots2)[1])


HAND_TREES = {"chain_2000": B.chain_tree, "perfect": B.perfect_tree, "equal_half_areas": lambda: B.perfect_tree(8, equal_areas=True),
              "grid_edges": B.grid_edge_nodes}


@pytest.mark.parametrize("name", list(HAND_TREES))
def test_collapse_of_hand_made_trees(builders, name):
    dev, host = builders
    nodes, roots = HAND_TREES[name]()
    _both_collapses(dev, host, nodes, roots)


def test_unquantisable_is_a_return_value_not_an_error(builders):
    dev, _ = builders
    assert dev.k_bvh4_collapse(*B.unquantisable_nodes()) is None


def test_node_visit_on_the_device(builders):
    """the contract of bvh4_test_node on the device's own wide nodes, per ray category, and its outputs equal to the host build's
    exactly, distances included (both sides use fused multiply-adds in the same places)"""
    dev, host = builders
    totals = {c: {"pairs": 0, "acc32": 0, "acc64": 0, "extra_hits": 0} for c in B.RAY_CATEGORIES}
    for tree, (nodes, roots) in B.node_test_trees(dev).items():
        wide, info = _both_collapses(dev, host, nodes, roots)
        info = B.with_grid(info, wide)
        pool = B.distinct_children(wide)
        for i, cat in enumerate(B.RAY_CATEGORIES):
            node, o, d, t = B.make_rays(cat, info, pool, 6000, 100 + i)
            got = dev.k_bvh4_test_nodes(wide, node, o, d, t)
            try:
                c = B.check_node_test(info, wide, node, o, d, t, got)
            except AssertionError as e:
                raise AssertionError(f"tree {tree}, rays {cat}: {e}") from e
            want = host.k_bvh4_test_nodes(wide, node, o, d, t)
            for g, w, what in zip(got, want, ("ref", "n_hit", "dist")):
                assert np.array_equal(g, w), f"tree {tree}, rays {cat}: {what} differs from the host build"  # (values: -0 == +0)
            for k in c:
                totals[cat][k] += c[k]
    for cat, c in totals.items():
        frac = c["acc32"] / c["pairs"]
        print(f"{cat:18s} pairs {c['pairs']:7d}  fp32 reference accepts {frac:.3f}  hits both reject {c['extra_hits'] / c['pairs']:.3f}")
        assert 0.2 <= frac <= 0.8, (cat, frac)
