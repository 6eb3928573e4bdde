"""One level of the light pick over the occupied children of a node only (shade_lights.h: light_node_occupancy,
light_node_importances_sparse -- what k_light_pick_sparse runs) against the level over all eight children
(light_node_importances_rows -- k_light_pick_first), without a GPU: both compiled for the host (tests/hostsim/hostsim_pick.cpp) and
compared as uint32 words, so that NaNs and the sign of a zero compare too.  The nodes: every node of the golden scenes' light tables
and hand-made ones with 0, 1, 3 and 8 occupied slots, a box-less child (flux alone), a boxed child without flux and a flux of -0.
The points: random ones, the children's centres (d2 == 0), points inside a child's bounding sphere, and far away.
tests/test_gpu_pick_sparse.py holds the device kernel against k_light_pick_first."""
import ctypes as C
import os

import numpy as np
import pytest

import light_refit_cases as L
import util

PICK_LIB = os.path.join(util.ROOT, "tests", "hostsim", "_build", "libhostsim_pick.so")
GOLDEN_SCENES = ["cornell_basic", "cornell_principled", "cornell_lights", "cornell_env", "cornell_filmic", "cornell_instances", "cornell_sky"]
_lib = None


def pick_lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(PICK_LIB)
        _lib.hostsim_pick_occupancy.argtypes = [C.c_void_p, C.c_void_p]
        _lib.hostsim_pick_level.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    return _lib


def test_the_host_build_exists():
    """(no skip for it in this file: __graft_entry__.build() makes the library)"""
    assert os.path.exists(PICK_LIB), "tests/hostsim/hostsim_pick.cpp not built (run __graft_entry__.build())"


def occupancy(rows):
    out = np.zeros(2, dtype=np.uint32)
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    assert pick_lib().hostsim_pick_occupancy(rows.ctypes.data, out.ctypes.data) == 0
    return int(out[0]), int(out[1])


def levels(rows, points):
    """([n][8] uint32, [n][8] uint32): the importances over all children, over the occupied ones"""
    rows, points = np.ascontiguousarray(rows, dtype=np.float32), np.ascontiguousarray(points, dtype=np.float32)
    dense, sparse = np.full((len(points), 8), 7.0, dtype=np.float32), np.full((len(points), 8), 9.0, dtype=np.float32)
    assert pick_lib().hostsim_pick_level(rows.ctypes.data, points.ctypes.data, len(points), dense.ctypes.data, sparse.ctypes.data) == 0
    return dense.view(np.uint32), sparse.view(np.uint32)


def points_for(rows, seed):
    """random points around the node, every child's centre, points inside every child's bounding sphere, and far away"""
    rng = np.random.RandomState(seed)
    centres, half_diag = rows[10:18, :3], rows[2:10, 3]
    span = max(1.0, float(np.abs(centres).max()))
    away = rng.normal(size=(8, 3)).astype(np.float32)
    away /= np.linalg.norm(away, axis=1, keepdims=True)
    inside = centres + away * (np.float32(0.5) * half_diag[:, None])
    far = np.concatenate([away * np.float32(1e3), away * np.float32(1e6), away[:2] * np.float32(1e18)])
    return np.concatenate([rng.uniform(-2.0 * span, 2.0 * span, size=(64, 3)).astype(np.float32), centres, inside, far]).astype(np.float32)


def expected_occupancy(rows):
    """a numpy restatement: the final select of light_child_importance, slot by slot"""
    valid, flux = rows[10:18, 3], rows[18:26, 3]
    with np.errstate(invalid="ignore"):
        arith = (valid != 0) & (flux != 0)
    alone = ~arith & (flux.view(np.uint32) != 0)
    slots = [i for i in range(8) if arith[i]]
    masks = sum(1 << i for i in slots) | sum(0x100 << i for i in range(8) if alone[i]) | len(slots) << 16
    return masks, sum(s << (4 * k) for k, s in enumerate(slots))


def check_node(rows, seed):
    assert occupancy(rows) == expected_occupancy(rows)
    dense, sparse = levels(rows, points_for(rows, seed))
    assert np.array_equal(dense, sparse), np.argwhere(dense != sparse)[:4]
    return dense


@pytest.mark.parametrize("name", GOLDEN_SCENES)
def test_sparse_level_equals_the_dense_level_on_the_golden_light_tables(name):
    a = L.Arrays(util.golden_scene(name))
    if len(a.cwnodes) == 0:
        return
    table = L.fill_children(a.cwnodes)
    seen = 0
    for n, rows in enumerate(table):
        seen += int(np.count_nonzero(check_node(rows, 100 + n).view(np.float32)))
    assert seen > 0  # (the comparison saw importances that are not zero)


def child(centre=(0.0, 0.0, 0.0), half_diag=0.1, axis=(0.0, -1.0, 0.0), cos_o=1.0, cos_e=0.0, flux=1.0, valid=1.0):
    return dict(axis=(*axis, half_diag), centre=(*centre, valid), cosines=(cos_o, float(np.sqrt(max(0.0, 1.0 - cos_o * cos_o))), cos_e, flux))


def node_of(children):
    """{slot: child(...)} -> rows[26][4]; the other slots are empty (zero rows, as decode_light_child leaves them)"""
    rows = np.zeros((26, 4), dtype=np.float32)
    rows[0:2] = np.full(8, 0x7fffffff, dtype=np.uint32).view(np.float32).reshape(2, 4)
    for i, c in children.items():
        rows[2 + i], rows[10 + i], rows[18 + i] = c["axis"], c["centre"], c["cosines"]
    return rows


def _spread(k):
    return (0.3 * k - 1.0, 0.5 - 0.1 * k, 0.2 * k)


HAND_MADE = {
    "empty": {},
    "one_in_slot_5": {5: child(centre=_spread(1), flux=3.0)},
    "three_apart": {0: child(centre=_spread(0), flux=2.0), 3: child(centre=_spread(3), flux=0.5, cos_o=0.3, cos_e=-0.2, axis=(1.0, 0.0, 0.0)),
                    7: child(centre=_spread(7), flux=8.0, half_diag=0.4, cos_o=-1.0, cos_e=-1.0)},
    "full": {i: child(centre=_spread(i), flux=1.0 + i, half_diag=0.05 * (i + 1), cos_o=1.0 - 0.25 * i, cos_e=0.1 * i - 0.4) for i in range(8)},
    "flux_alone_beside_two": {1: child(centre=_spread(1), flux=2.0), 2: child(valid=0.0, flux=0.75, half_diag=0.0, axis=(0.0, 0.0, 0.0), cos_o=0.0),
                              6: child(centre=_spread(6), flux=1.5)},
    "box_without_flux_beside_one": {2: child(centre=_spread(2), flux=0.0), 4: child(centre=_spread(4), flux=4.0)},
    "flux_of_minus_zero": {0: child(centre=_spread(0), flux=-0.0), 1: child(centre=_spread(1), flux=1.0)},
    "point_sized_children": {3: child(centre=_spread(3), half_diag=0.0, flux=5.0), 4: child(centre=_spread(4), half_diag=0.0, flux=6.0)},
}
HAND_MADE_COUNTS = {"empty": 0, "one_in_slot_5": 1, "three_apart": 3, "full": 8, "flux_alone_beside_two": 2, "box_without_flux_beside_one": 1,
                    "flux_of_minus_zero": 1, "point_sized_children": 2}


@pytest.mark.parametrize("name", sorted(HAND_MADE))
def test_sparse_level_equals_the_dense_level_on_hand_made_nodes(name):
    rows = node_of(HAND_MADE[name])
    masks, _ = occupancy(rows)
    assert masks >> 16 == HAND_MADE_COUNTS[name]
    dense = check_node(rows, 7)
    if name == "empty":
        assert not dense.any()  # (+0 in every slot)
    if name == "flux_alone_beside_two":
        assert masks & 0xff00 == 0x100 << 2 and (dense[:, 2] == np.float32(0.75).view(np.uint32)).all()
    if name == "flux_of_minus_zero":
        assert masks & 0xff00 == 0x100 and (dense[:, 0] == 0x80000000).all()
    if name == "box_without_flux_beside_one":
        assert masks & 0xffff == 1 << 4 and not dense[:, 2].any()
