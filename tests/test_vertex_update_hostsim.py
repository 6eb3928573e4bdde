"""The vertex update without a GPU (ray_amd/csrc/refit.h through tests/hostsim/hostsim_refit.cpp): the triangle records and the
child boxes a refit computes are the ones the reference's scene build stores, bit for bit; under moved vertices they equal an
independent numpy restatement; and a scene patched with refitted arrays renders the frames of the scene built afresh -- which is what
licenses the equality assertions of tests/test_gpu_vertex_update.py."""
import os

import numpy as np
import pytest

import oracle_lib as O
import util
import vertex_update_cases as V
from ray_amd import api

pytestmark = pytest.mark.skipif(not V.have_refit_lib(), reason="tests/hostsim/hostsim_refit.cpp not built (run __graft_entry__.build())")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _need_host_lib():
    if not os.path.exists(api.HIP_HOST_LIB):
        pytest.skip("libray_hip.so not built (needs the reference tree at build time)")


@pytest.mark.parametrize("name", V.fixture_names())
def test_fixture_triangle_records(name):
    """the records the reference built are PreprocessTri over the corner positions: refit_tris over a scene's own vertices changes
    no reachable record"""
    a = V.Arrays(util.golden_scene(name))
    recs, n_degenerate = V.refit_tris(a.vertices, a.vtx_indices, a.tri_indices, np.zeros_like(a.tris))
    e = a.reachable_entries()
    assert len(e) > 0 and n_degenerate == 0
    assert np.array_equal(bits(recs[e]), bits(a.tris[e]))


@pytest.mark.parametrize("name", V.fixture_names())
def test_fixture_node_boxes(name):
    """... and every child box below a bottom-level root is the min / max of the positions below it: refit_nodes changes no node"""
    a = V.Arrays(util.golden_scene(name))
    zeroed = a.nodes.copy()
    below, _ = a.blas_nodes()
    zeroed[below, :12] = 0
    got = V.refit_nodes(zeroed, a.roots(), a.tri_indices, a.vtx_indices, a.vertices)
    assert len(below) > 0
    assert np.array_equal(got[below], a.nodes[below])
    rest = np.setdiff1d(np.arange(len(a.nodes)), below)
    assert np.array_equal(got[rest], zeroed[rest])  # the top level and free slots are not the refit's


@pytest.fixture(scope="module")
def perturbed():
    a = V.Arrays(util.golden_scene("cornell_instances"))
    v = V.perturbed_vertices(a)
    recs, nodes, n_degenerate = V.host_refit(a, v)
    return a, v, recs, nodes, n_degenerate


def test_perturbed_records_equal_the_numpy_restatement(perturbed):
    a, v, recs, _, n_degenerate = perturbed
    e = a.reachable_entries()
    assert not np.array_equal(recs[e], a.tris[e]) and n_degenerate == 0
    assert np.array_equal(v[a.light_vertices()], a.vertices[a.light_vertices()]) and len(a.light_vertices()) >= 3
    assert np.array_equal(bits(recs[e]), bits(V.numpy_entry_records(a, v, e)))


def test_perturbed_boxes_are_the_extent_of_what_lies_below(perturbed):
    a, v, _, nodes, _ = perturbed
    want = V.numpy_boxes_below(a, v, a.nodes)
    below, _ = a.blas_nodes()
    assert sorted({w for w, _ in want}) == below
    f = nodes.view(np.float32)
    for (w, k), box in want.items():
        assert np.array_equal(bits(V.child_box(f[w], k)), bits(box.astype(np.float32))), (w, k)
    assert np.array_equal(nodes[:, 12:], a.nodes[:, 12:])  # links stay


def test_a_triangle_without_area_gets_the_zero_record():
    a = V.Arrays(util.golden_scene("cornell_instances"))
    v = V.perturbed_vertices(a)
    e = a.reachable_entries()
    t, _ = V.collapse_one_triangle(a, v)
    recs, _, n_degenerate = V.host_refit(a, v)
    hit = e[a.tri_indices[e] == t]
    assert len(hit) >= 1 and not recs[hit].any()
    assert n_degenerate == 1
    # entries repeat triangles (the reference pads leaves, the refinement doubles a lone triangle): every repeat gets the record, the
    # triangle is counted once
    twice, n2 = V.refit_tris(v, a.vtx_indices, np.concatenate([a.tri_indices, a.tri_indices]), np.concatenate([a.tris, a.tris]))
    assert n2 == 1 and np.array_equal(bits(twice[:len(recs)][e]), bits(recs[e])) and np.array_equal(bits(twice[len(recs):][e]), bits(recs[e]))
    others = e[a.tri_indices[e] != t]
    assert recs[others].any(axis=1).all()
    assert np.array_equal(bits(recs[others]), bits(V.numpy_entry_records(a, v, others)))


@pytest.mark.parametrize("height, rc", [(128, 0), (129, 2)])
def test_a_tree_above_128_levels_is_refused(height, rc):
    """one launch per height level: a chain of `height` nodes (left child a leaf, right child the next node) is the highest tree of
    that many nodes"""
    nodes = np.zeros((height, 16), dtype=np.uint32)
    nodes[:, 12] = (1 << 29) | 0  # a leaf of entries 0, 1
    nodes[:-1, 13] = np.arange(1, height)
    nodes[-1, 13] = (1 << 29) | 0
    v = np.zeros(3, dtype=V.hip.VERTEX_DTYPE)
    v["p"] = [[0, 0, 0], [1, 0, 0], [0, 2, 3]]
    vp, u32 = V.C.c_void_p, np.uint32
    roots, ti, vi = np.array([0], u32), np.array([0, 0], u32), np.array([0, 1, 2], u32)
    got = V.refit_lib().hostsim_refit_nodes(nodes.ctypes.data, height, roots.ctypes.data, 1, ti.ctypes.data, vi.ctypes.data, v.ctypes.data)
    assert got == rc
    if rc == 0:
        f = nodes.view(np.float32)
        assert all(np.array_equal(V.child_box(f[w], k), np.array([0, 0, 0, 1, 2, 3], np.float32)) for w in (0, height - 1) for k in (0, 1))
    else:
        assert not nodes[:, :12].any()  # nothing was written


def test_instance_boxes_against_the_scene_build():
    """the world box of an instance.  NOT bit-equal to the boxes the reference's scene build stores: its TransformBoundingBox
    (internal/Core.cpp:1368-1388) starts each bound at the translation and adds, per axis, the smaller / larger of the two products
    m[i][j] * lo[i], m[i][j] * hi[i] -- three additions in the order t + x + y + z -- while transform_box (scene_rebuild.h) transforms
    the eight corners as m0 x + m4 y + m8 z + t and takes their min / max: the same real numbers, summed in another order, so the
    ADDITIONS round differently (by an ulp or two).  Hence the containment form: each box holds the float64 transforms of the vertices of
    its instance (a rotated box is wider than what it holds by far more than a rounding; the room's transform is the identity, which is exact)."""
    _need_host_lib()
    a = V.Arrays(V.scene_blob("sheets_instanced", 1))
    slots = a.live_instances()
    assert len(slots) == 4
    boxes = V.instance_boxes(a.nodes, a.mesh_instances, slots)
    stored = a.top_level_leaves()
    print("instance boxes bit-equal to the scene build's:", [bool(np.array_equal(bits(boxes[k]), bits(stored[mi]))) for k, mi in enumerate(slots)])
    print("largest difference:", max(float(np.abs(boxes[k].astype(np.float64) - stored[mi]).max()) for k, mi in enumerate(slots)))
    for k, mi in enumerate(slots):
        inst = a.mesh_instances[mi]
        ranges, stack = [], [int(inst["node_index"])]
        while stack:
            for link in a.nodes[stack.pop(), 12:14]:
                if link & V.COUNT_BITS:
                    ranges.extend(range(link & V.INDEX_BITS, (link & V.INDEX_BITS) + ((link & V.COUNT_BITS) >> 29) + 1))
                else:
                    stack.append(int(link))
        t = a.tri_indices[ranges].astype(np.int64)
        p = a.vertices["p"][np.unique(np.concatenate([a.vtx_indices[3 * t], a.vtx_indices[3 * t + 1], a.vtx_indices[3 * t + 2]]))].astype(np.float64)
        m = inst["xform"].astype(np.float64).reshape(4, 4)  # column-major: world = p @ m[:3, :3] + m[3, :3]
        world = p @ m[:3, :3] + m[3, :3]
        # A float32 bound cannot hold a float64 value exactly: each bound is the result of three products and three additions rounded to
        # float32 (half an ulp each, of values no larger than |m| |p| + |t|) -- the reference's own stored boxes miss strict containment
        # by the same ulp (printed below).  So: containment up to those six roundings.
        slack = 6 * 2.0 ** -24 * (np.abs(p) @ np.abs(m[:3, :3]) + np.abs(m[3, :3])).max(axis=0)
        lo, hi = world.min(axis=0), world.max(axis=0)
        print(f"slot {mi}: strictly inside ours {bool(np.all(lo >= boxes[k][:3]) and np.all(hi <= boxes[k][3:]))}, the scene build's "
              f"{bool(np.all(lo >= stored[mi][:3]) and np.all(hi <= stored[mi][3:]))}; outside ours by at most "
              f"{max(float((boxes[k][:3] - lo).max()), float((hi - boxes[k][3:]).max()), 0.0):.3g}, slack {float(slack.min()):.3g}")
        assert np.all(lo >= boxes[k][:3] - slack) and np.all(hi <= boxes[k][3:] + slack), mi


@pytest.mark.parametrize("name", sorted(V.SCENES))
def test_a_refitted_scene_renders_the_frames_of_a_fresh_one(name):
    """the tie check: phase 0's trees refitted to phase 1's vertices against phase 1 built afresh (another tree, the same surfaces).
    A BVH only culls, so the frames differ only where two hits tie at the same distance; these scenes have no such pixel."""
    _need_host_lib()
    if not O.have_hostsim() or not O.have_ref():
        pytest.skip("tests/hostsim or the oracle not built")
    old, new = V.scene_blob(name, 0), V.scene_blob(name, 1)
    a, b = V.Arrays(old), V.Arrays(new)
    n_idx = 3 * (int(a.tri_indices[a.reachable_entries()].max()) + 1)  # (behind the triangles the pool holds whatever it held)
    assert np.array_equal(a.vtx_indices[:n_idx], b.vtx_indices[:n_idx]) and len(a.vertices) == len(b.vertices)
    assert not np.array_equal(a.vertices["p"], b.vertices["p"])
    lv = a.light_vertices()
    assert np.array_equal(a.vertices[lv], b.vertices[lv])
    recs, nodes, n_degenerate = V.host_refit(a, b.vertices)
    assert n_degenerate == 0
    # the top level: the boxes of the live instances from the refitted roots (one instance per leaf in these scenes)
    f = nodes.view(np.float32)
    slots = a.live_instances()
    boxes = dict(zip(slots, V.instance_boxes(nodes, a.mesh_instances, slots)))

    def fit_top(w):
        out = []
        for k, link in enumerate(nodes[w, 12:14]):
            box = boxes[int(link & V.INDEX_BITS)] if link & V.COUNT_BITS else fit_top(int(link))
            lo, hi = box[:3], box[3:]
            if k == 0:
                f[w, [0, 2, 8]], f[w, [1, 3, 9]] = lo, hi
            else:
                f[w, [4, 6, 10]], f[w, [5, 7, 11]] = lo, hi
            out.append(box)
        return np.concatenate([np.minimum(out[0][:3], out[1][:3]), np.maximum(out[0][3:], out[1][3:])])

    fit_top(a.tlas_root)
    patched = V.patched_blob(old, vertices=b.vertices, tris=recs, nodes=nodes)
    w, h, spp = 96, 64, 4
    got = util.render_frames(O.hostsim_context(w, h, patched, util.pmj()), spp)
    fresh = util.render_frames(O.hostsim_context(w, h, new, util.pmj()), spp)
    first = util.render_frames(O.hostsim_context(w, h, old, util.pmj()), spp)
    assert not np.array_equal(first, fresh)
    assert np.array_equal(got, fresh)
