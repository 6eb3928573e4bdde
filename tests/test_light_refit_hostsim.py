"""The light refit without a GPU (ray_amd/csrc/light_refit.h through tests/hostsim/hostsim_lights.cpp): refitting a scene the
reference built, with its vertices unchanged, gives back the light tree the reference stored (bit for bit but for the sums the refit
takes in another order); at a moved pose the tree agrees with a float64 restatement of what a refit is asked to compute; the child
boxes on the path to every triangle light contain it; and a crafted tree with a hole, a triangle without area and infinite
children comes out as stated.  tests/test_gpu_light_refit.py holds the device against the same host build."""
import os

import numpy as np
import pytest

import light_refit_cases as L
import vertex_update_cases as V
from ray_amd import api

bits = L.bits
STEP_COS, STEP_AXIS = 2.0 / 65534.0, 2.0 / 65535.0
# Largest gaps between the decoded words of the refitted trees and the float64 model over the cases of this file, measured on the
# CPU (test_against_the_float64_model_at_a_moved_pose prints them): 1.289e-05 in a cosine (0.42 quantisation steps; the crafted tree --
# the scenes' cones are 0, pi / 2 and pi, which the words hold exactly) and 5.223e-05 in an axis component (1.71 steps;
# emissive_sheet).  The gates are twice that, and may never pass 8 quantisation steps.
MEASURED_COS_GAP, MEASURED_AXIS_GAP = 1.289e-05, 5.223e-05
GATE_COS, GATE_AXIS = 2.0 * MEASURED_COS_GAP, 2.0 * MEASURED_AXIS_GAP
assert GATE_COS <= 8 * STEP_COS and GATE_AXIS <= 8 * STEP_AXIS
# Containment slack, in units of the node's extent on the axis: how far a corner of a triangle light lies outside the decoded child
# boxes on its path in the trees the REFERENCE built at the moved pose (measured by test_containment over them, printed there):
# 5.808e-08 on emissive_sheet, 0 on the other two -- the float32 rounding of lo + byte * step.  The refitted trees must pass with the
# same slack (they come out at the same 5.808e-08).
CONTAINMENT_SLACK = 5.81e-08
Q_WINDOW = 255.0 * 3.0 * 2.0 ** -24  # 4.6e-05: see _model_gaps


def _need_lib():
    assert L.have_lights_lib() and V.have_refit_lib(), "tests/hostsim/hostsim_lights.cpp is not built (run __graft_entry__.build())"


def _need_host_lib():
    if not os.path.exists(api.HIP_HOST_LIB):
        pytest.skip("libray_hip.so not built (needs the reference tree at build time)")


def _scene(name, phase=0):
    _need_lib()
    if name != "fixture":
        _need_host_lib()
    blob = L.scene_blob(name, phase)
    return blob, L.Arrays(blob)


def _moved(name):
    """(arrays of the scene as built at rest, the vertices of its moved pose, arrays of the reference's build AT that pose or None)"""
    _, a = _scene(name)
    if name == "fixture":
        return a, L.moved_vertices(a), None
    _, b = _scene(name, 1)
    # (the arrays are sparse pools, a free slot holds anything: what the lights name is compared)
    assert np.array_equal(a.li_indices, b.li_indices) and np.array_equal(a.lights[a.li_indices], b.lights[b.li_indices])
    t = a.lights[a.tri_lights(), 4].astype(np.int64)
    assert all(np.array_equal(a.vtx_indices[3 * t + k], b.vtx_indices[3 * t + k]) for k in range(3)) and len(a.vertices) == len(b.vertices)
    assert not np.array_equal(bits(a.vertices["p"][a.light_vertices()]), bits(b.vertices["p"][a.light_vertices()]))
    return a, b.vertices, b


SCENES = ("fixture", "one_emitter", "emissive_sheet")


@pytest.mark.parametrize("name", SCENES)
def test_identity(name):
    _, a = _scene(name)
    r = L.host_refit(a, a.vertices)
    old, new = a.cwnodes, r.cwnodes
    assert r.degenerate == 0 and len(old) > 0
    assert np.array_equal(old["child"], new["child"])
    assert np.array_equal(bits(old["bbox_min"]), bits(new["bbox_min"])) and np.array_equal(bits(old["bbox_max"]), bits(new["bbox_max"]))
    flat = old["bbox_min"] == old["bbox_max"]  # [n][3]: the node's box has no extent on the axis
    boxes_old, boxes_new = L.child_boxes(old), L.child_boxes(new)
    types = a.light_types()
    n_tri = n_other = n_inner = 0
    for w in range(len(old)):
        for ax in range(3):
            if flat[w, ax]:
                used = old["child"][w] != L.EMPTY
                assert np.array_equal(bits(boxes_old[w, used][:, [ax, 3 + ax]]), bits(boxes_new[w, used][:, [ax, 3 + ax]]))
            else:
                assert np.array_equal(old["ch_bbox_min"][w, ax], new["ch_bbox_min"][w, ax]) and np.array_equal(old["ch_bbox_max"][w, ax], new["ch_bbox_max"][w, ax])
        for i, c in enumerate(old["child"][w]):
            words = [bits(n[f][w, i:i + 1])[0] for n in (old, new) for f in ("flux", "axis", "cos_omega_ne")]
            if c == L.EMPTY or (c & L.LEAF_BIT):
                assert words[:3] == words[3:], (w, i)  # an empty slot, a triangle light, another light: bytewise
                n_tri += c != L.EMPTY and types[c & L.INDEX_BITS] == L.TYPE_TRI
                n_other += c != L.EMPTY and types[c & L.INDEX_BITS] != L.TYPE_TRI
                continue
            n_inner += 1  # (their fluxes: the two tests below)
    assert n_tri == len(a.tri_lights()) and n_other == len(a.li_indices) - n_tri
    if name == "emissive_sheet":
        ln, lo = L.levels(old, len(a.lights))
        assert len(lo) - 1 >= 3 and lo[1] - lo[0] > 32 and n_inner >= 32 and n_other == 3 and n_tri == 578
        assert (old["ch_bbox_min"][:, 0] == 0xff).any()  # the directional light: an infinite child
    if name == "one_emitter":
        assert len(old) == 1 and n_tri == 1 and flat[0].sum() == 1 and (old["child"][0, 1:] == L.EMPTY).all()
    # the corners, and where nothing but box bytes on flat axes may differ, the importance rows
    assert np.array_equal(bits(r.tri_geom), bits(L.fill_tri_geom(a, a.vertices)))
    if n_inner == 0:
        assert np.array_equal(bits(r.children), bits(L.fill_children(old)))


def _inner_fluxes(a, r):
    """per inner-child slot: (node, slot, lights below, flux as uploaded, flux refitted, the child's summed flux as the refit found it,
    the float64 sum of the leaf fluxes below)"""
    old = a.cwnodes
    leaf = {int(c & L.INDEX_BITS): float(old["flux"][w, i]) for w in range(len(old)) for i, c in enumerate(old["child"][w]) if c != L.EMPTY and c & L.LEAF_BIT}
    rows = []
    for w in range(len(old)):
        for i, c in enumerate(old["child"][w]):
            if c != L.EMPTY and not c & L.LEAF_BIT:
                below = L.lights_below(old, int(c))
                rows.append((w, i, len(below), float(old["flux"][w, i]), float(r.cwnodes["flux"][w, i]), float(r.node_summary["flux"][int(c)]),
                             sum(leaf[k] for k in below)))
    return rows


@pytest.mark.parametrize("name", SCENES)
def test_identity_inner_flux(name):
    """An inner-child slot over n lights has its flux within 2 (n - 1) 2^-24 relative of the UPLOADED value: the bound for re-ordering a
    sum of n non-negative floats.

    This holds through the slot scales (light_refit.h: slot_scales), not because the uploaded value is that sum: in emissive_sheet 9
    of 212 inner slots store 0.7 % to 55 % LESS than the sum of what lies below them (the scene build hands a node's flux on to its
    parent once the node's left child is counted, so a deeper right subtree arrives too late).  A refit keeps the ratio of the stored
    flux to the sum, taken at the upload pose; test_inner_sums_and_scales holds sums and ratios against float64."""
    _, a = _scene(name)
    rows = _inner_fluxes(a, L.host_refit(a, a.vertices))
    off = [(w, i, n, new / old - 1.0) for w, i, n, old, new, _, _ in rows if abs(new - old) > 2 * (n - 1) * 2.0 ** -24 * old]
    print(f"{name}: {len(off)} of {len(rows)} inner slots outside 2 (n - 1) 2^-24 of the uploaded flux:", [(w, i, n, f"{d:+.3e}") for w, i, n, d in off])
    assert not off


@pytest.mark.parametrize("name", SCENES)
def test_inner_sums_and_scales(name):
    """the summed flux a refit finds below an inner slot against the float64 sum of the fluxes of the n lights below it: within
    2 (n - 1) 2^-24 relative (n - 1 float32 additions in some order, twice for the levels in between); the uploaded value is never ABOVE
    that sum, and the slot's scale is their ratio -- 1 to rounding wherever the scene build stored the sum"""
    _, a = _scene(name)
    r = L.host_refit(a, a.vertices)
    rows = _inner_fluxes(a, r)
    low = 0
    for w, i, n, old, _, summed, exact in rows:
        bound = 2 * (n - 1) * 2.0 ** -24
        assert abs(summed - exact) <= bound * exact, (w, i, n)
        assert old <= exact * (1.0 + bound), (w, i, n)
        assert abs(float(r.scales[w, i]) - old / exact) <= (bound + 2.0 ** -23) * old / exact, (w, i, n)
        low += old < exact * (1.0 - bound)
    assert np.all(r.scales[(a.cwnodes["child"] == L.EMPTY) | ((a.cwnodes["child"] & L.LEAF_BIT) != 0)] == 1)
    if rows:
        print(f"{name}: {low} of {len(rows)} inner slots store less than the sum below them; scales in [{min(r.scales[w, i] for w, i, *_ in rows):.4f}, "
              f"{max(r.scales[w, i] for w, i, *_ in rows):.4f}]; summed / exact - 1 in [{min(x[5] / x[6] for x in rows) - 1:+.3e}, {max(x[5] / x[6] for x in rows) - 1:+.3e}]")
    if name == "emissive_sheet":
        assert low == 9


def _model_gaps(lights, li_indices, mesh_instances, vtx_indices, r):
    """(cosine gap, axis gap) of the refitted arrays `r` against the float64 model over the float32 world corners r.tri_geom holds;
    asserts the exact parts: node boxes, quantised child boxes, fluxes to float32 rounding"""
    corners = np.zeros(len(r.tri_geom) * 3, dtype=L.hip.VERTEX_DTYPE)
    corners["p"] = r.tri_geom[:, :3, :3].reshape(-1, 3)  # (the transform is fill_light_tri_geom's, tested elsewhere: the model starts behind it)
    tri = lights.copy()
    identity = np.zeros(1, dtype=V.MESH_INSTANCE_DTYPE)
    identity["xform"][0] = np.eye(4, dtype=np.float32).ravel()
    is_tri = (tri[:, 0] & 7) == L.TYPE_TRI
    tri[is_tri, 4], tri[is_tri, 5] = np.arange(len(tri), dtype=np.uint32)[is_tri], 0
    leaf, node = L.model64(tri, li_indices, identity, np.arange(len(corners), dtype=np.uint32), corners, r.cwnodes)
    n = r.cwnodes
    gap_cos = gap_axis = 0.0
    one_off = n_bytes = 0
    for w in range(len(n)):
        own = node[w]
        if own["finite"]:
            assert np.array_equal(n["bbox_min"][w], own["lo"].astype(np.float32)) and np.array_equal(n["bbox_max"][w], own["hi"].astype(np.float32))
        lo, hi = n["bbox_min"][w].astype(np.float64), n["bbox_max"][w].astype(np.float64)
        for i, c in enumerate(n["child"][w]):
            if c == L.EMPTY:
                continue
            s = L.model64_slot(n, leaf, node, w, i)
            qlo, qhi = n["ch_bbox_min"][w, :, i].astype(int), n["ch_bbox_max"][w, :, i].astype(int)
            if not s["finite"]:
                assert (qlo == 0xff).all() and (qhi == 0).all()
            else:
                ext = np.where(hi > lo, hi - lo, 1.0)
                want_lo = np.where(hi > lo, np.floor(np.clip(255.0 * (s["lo"] - lo) / ext, 0, 255)), 0)
                want_hi = np.where(hi > lo, np.ceil(np.clip(255.0 * (s["hi"] - lo) / ext, 0, 255)), 0)
                # The bytes are the float64 ones, but for a quotient that misses an integer by less than the float32 code's own error: the
                # difference, the product and the quotient round once each, 3 * 2^-24 relative of a value of at most 255 (Q_WINDOW).  Such
                # a byte may be one off, either way; the slots that take this are counted and printed
                for got, want, q in ((qlo, want_lo, 255.0 * (s["lo"] - lo) / ext), (qhi, want_hi, 255.0 * (s["hi"] - lo) / ext)):
                    differs = got != want
                    assert (np.abs(got - want)[differs] == 1).all() and (np.abs(q - np.round(q))[differs] <= Q_WINDOW).all(), (w, i)
                    one_off += int(differs.sum())
                n_bytes += 6
            if (c & L.LEAF_BIT) and lights[int(c & L.INDEX_BITS), 0] & 7 != L.TYPE_TRI:
                continue  # (kept bytewise)
            below = 1 if c & L.LEAF_BIT else len(L.lights_below(n, int(c)))
            scale = 1.0 if r.scales is None or c & L.LEAF_BIT else float(r.scales[w, i])  # (an inner slot: the summed flux times the slot's scale)
            assert abs(float(n["flux"][w, i]) - s["flux"] * scale) <= (below + 8) * 2.0 ** -24 * abs(s["flux"] * scale), (w, i)
            cosines = L.decode_cosines(n["cos_omega_ne"][w, i])
            gap_cos = max(gap_cos, abs(cosines[0] - np.cos(s["omega_n"])), abs(cosines[1] - max(np.cos(s["omega_e"]), 0.0)))
            gap_axis = max(gap_axis, float(np.abs(L.decode_axis(n["axis"][w, i]) - s["axis"]).max()))
    return gap_cos, gap_axis, one_off, n_bytes


@pytest.mark.parametrize("name", SCENES + ("crafted",))
def test_against_the_float64_model_at_a_moved_pose(name):
    _need_lib()
    if name == "crafted":
        c = L.Crafted()
        v = c.vertices.copy()
        v["p"][:6] += np.random.RandomState(5).uniform(-0.2, 0.2, size=(6, 3)).astype(np.float32)
        gaps = _model_gaps(c.lights, c.li_indices, c.mesh_instances, c.vtx_indices, c.refit(v))
    else:
        a, v, _ = _moved(name)
        r = L.host_refit(a, v)
        assert not np.array_equal(bits(r.cwnodes), bits(a.cwnodes))
        gaps = _model_gaps(a.lights, a.li_indices, a.mesh_instances, a.vtx_indices, r)
        # the model starts at the float32 world corners: those against the float64 transform of the vertices -- three products and three
        # sums, each rounded once: 6 * 2^-24 of the sum of the terms' magnitudes
        for light, want in a.tri_light_corners(v).items():
            tri, mi = int(a.lights[light, 4]), int(a.lights[light, 5])
            m = np.abs(a.mesh_instances["xform"][mi].astype(np.float64).reshape(4, 4))
            size = np.abs(v["p"][a.vtx_indices[3 * tri:3 * tri + 3]].astype(np.float64)) @ m[:3, :3] + m[3, :3]
            assert (np.abs(r.tri_geom[light, :3, :3].astype(np.float64) - want) <= 6 * 2.0 ** -24 * size).all(), light
    print(f"{name}: largest gap to the float64 model: cosine {gaps[0]:.3e} ({gaps[0] / STEP_COS:.2f} steps), axis component {gaps[1]:.3e} "
          f"({gaps[1] / STEP_AXIS:.2f} steps); {gaps[2]} of {gaps[3]} quantised box bytes one off the float64 byte, each within {Q_WINDOW:.1e} of an integer")
    assert gaps[2] == 0  # (measured: no byte of any case takes the window -- every quantised byte is the float64 one)
    assert gaps[0] <= GATE_COS and gaps[1] <= GATE_AXIS


def _worst_outside(a, cwnodes, vertices):
    """how far a corner of a triangle light lies outside a decoded child box on its path, at worst, in units of the node's extent"""
    boxes = L.child_boxes(cwnodes).astype(np.float64)
    geom = L.fill_tri_geom(a, vertices)
    trails = L.paths(cwnodes)
    worst, seen = 0.0, 0
    for light in a.tri_lights():
        p = geom[light, :3, :3].astype(np.float64)
        for w, i in trails[int(light)]:
            lo, hi = boxes[w, i, :3], boxes[w, i, 3:]
            ext = (cwnodes["bbox_max"][w] - cwnodes["bbox_min"][w]).astype(np.float64)
            out = np.maximum(np.maximum(lo - p, p - hi), 0.0).max(axis=0)
            worst = max(worst, float((out[ext > 0] / ext[ext > 0]).max(initial=0.0)), 0.0 if (out[ext == 0] == 0).all() else np.inf)  # (outside a box without extent: by any measure)
            seen += 1
    assert seen >= len(a.tri_lights()) > 0
    return worst


@pytest.mark.parametrize("name", SCENES)
def test_containment(name):
    a, v, rebuilt = _moved(name)
    reference = _worst_outside(rebuilt, rebuilt.cwnodes, v) if rebuilt is not None else _worst_outside(a, a.cwnodes, a.vertices)
    r = L.host_refit(a, v)
    refitted = _worst_outside(a, r.cwnodes, v)
    print(f"{name}: a corner outside a child box on its path, in node extents: reference-built {reference:.3e}, refitted {refitted:.3e}")
    assert reference <= CONTAINMENT_SLACK
    assert refitted <= CONTAINMENT_SLACK
    stale = _worst_outside(a, a.cwnodes, v)  # ... which the tree as uploaded does not
    assert name == "one_emitter" or stale > 100 * CONTAINMENT_SLACK


def test_crafted_tree():
    _need_lib()
    c = L.Crafted()
    r = c.refit()
    old, new = c.cwnodes, r.cwnodes
    assert r.degenerate == 1 and np.array_equal(old["child"], new["child"])
    # empty slots: all 24 bytes untouched -- the hole in the middle of the root with its own bytes among them
    for w in range(3):
        for i in np.flatnonzero(old["child"][w] == L.EMPTY):
            for f in ("ch_bbox_min", "ch_bbox_max"):
                assert np.array_equal(old[f][w, :, i], new[f][w, :, i])
            for f in ("flux", "axis", "cos_omega_ne"):
                assert bits(old[f][w, i:i + 1])[0] == bits(new[f][w, i:i + 1])[0]
    assert new["flux"][0, 1] == np.float32(123.0) and new["axis"][0, 1] == 0xdeadbeef and tuple(new["ch_bbox_min"][0, :, 1]) == (1, 2, 3)
    # the triangle without area: flux 0, axis (0, 1, 0), and its slot can never be picked, from anywhere
    assert r.leaf["flux"][2] == 0 and tuple(r.leaf["axis"][2]) == (0.0, 1.0, 0.0) and new["flux"][1, 3] == 0
    for P in ([0.8, 0.6, 0.7], [0.0, 0.0, 0.0], [5.0, -3.0, 2.0]):
        imp = L.importances(new[1], P)
        assert imp[3] == 0 and imp[0] > 0
    summed = np.float32(np.float32(r.leaf["flux"][0] + r.leaf["flux"][1]) + np.float32(0.0))  # slot order
    assert r.node_summary["flux"][1] == summed
    # ... which the root's slot holds times its scale: the crafted tree stores 0.25 there, less than the sum, as a scene build may
    assert r.scales[0, 0] == np.float32(0.25) / summed and 0 < r.scales[0, 0] < 0.5 and new["flux"][0, 0] == summed * r.scales[0, 0]
    assert abs(float(new["flux"][0, 0]) - 0.25) <= 2.0 ** -24 and r.scales[0, 3] == 1 and new["flux"][0, 3] == np.float32(4.5)
    twice = c.vertices.copy()
    twice["p"][:6] *= np.float32(2.0)  # the two emitters twice as large: four times the flux, the slot keeps its ratio
    assert abs(float(c.refit(twice).cwnodes["flux"][0, 0]) - 1.0) <= 8 * 2.0 ** -24
    # infinite children: (0xff, 0), left out of the node's box; a node without a finite child keeps its box bytes and is infinite itself
    for w, i in ((0, 5), (2, 0), (2, 4), (0, 3)):
        assert (new["ch_bbox_min"][w, :, i] == 0xff).all() and (new["ch_bbox_max"][w, :, i] == 0).all()
    assert np.array_equal(bits(new["bbox_min"][2]), bits(old["bbox_min"][2])) and np.array_equal(bits(new["bbox_max"][2]), bits(old["bbox_max"][2]))
    assert r.node_summary["lo"][2, 0] == -L.MAX_DIST and r.node_summary["flux"][2] == np.float32(4.5)
    finite = np.concatenate([r.leaf["lo"][[0, 1, 2, 4]], r.leaf["hi"][[0, 1, 2, 4]]])
    assert np.array_equal(new["bbox_min"][0], finite.min(axis=0)) and np.array_equal(new["bbox_max"][0], finite.max(axis=0))
    assert np.abs(new["bbox_max"][0]).max() < 2.0  # (no MAX_DIST in it)
    # lights that are no triangles keep flux, axis and cosines bytewise; their box is re-quantised under the new node box
    for w, i in ((0, 2), (0, 5), (2, 0), (2, 4)):
        for f in ("flux", "axis", "cos_omega_ne"):
            assert bits(old[f][w, i:i + 1])[0] == bits(new[f][w, i:i + 1])[0]
    assert not np.array_equal(old["ch_bbox_min"][0, :, 2], new["ch_bbox_min"][0, :, 2])
    # and the importance rows are fill_light_children of the nodes just written
    assert np.array_equal(bits(r.children), bits(L.fill_children(new)))
    assert np.array_equal(bits(r.tri_geom[:3, :3, :3]), bits(c.vertices["p"].reshape(3, 3, 3)))
