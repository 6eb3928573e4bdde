"""Inputs and an independent checker for the tree builders (lbvh.h / lbvh.hip.h, bvh4_build.h / bvh4_build.hip.h) and the wide node
test (rt_bvh4.h: bvh4_test_node), reached through the hooks rayhip_k_lbvh_build / rayhip_k_bvh4_collapse / rayhip_k_bvh4_test_nodes
and their host build (tests/hostsim/hostsim_bvh.cpp).

The checker is plain numpy and calls no product code: a tree is judged by what it must satisfy (coverage, exact boxes, leaf
sizes, tight quantisation, the children wide_children defines), not by being equal to another build.  Everything walks level by
level over whole arrays, so the large cases (2^20 + 3 primitives) stay vectorised.

Word layouts (u32 views; floats by bit pattern):
  BVH2 node [16]: 0-3 child 0 {xmin, xmax, ymin, ymax}, 4-7 child 1, 8-11 {z0min, z0max, z1min, z1max}, 12 left, 13 right
  wide node [16]: 0-2 org, 3 step.x, 4-7 child, 8-10 qlo[xyz] (byte c = child c), 11-13 qhi[xyz], 14 step.y, 15 step.z
"""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_LIB = os.path.join(ROOT, "tests", "hostsim", "_build", "libhostsim_bvh.so")

NONE = 0xFFFFFFFF
EMPTY = 0xFFFFFFFF
COUNT_BITS = 7 << 29
INDEX_BITS = (1 << 29) - 1
FLT_MAX = np.float32(3.402823466e+38)
FLT_EPS = np.float32(0.0000001)
f32 = np.float32

# the three flag combinations the product uses: (leaf_is_primitive, roots_are_nodes)
REFINE, MESH, TOP = (False, False), (False, True), (True, True)


# ---- the host build behind the interface of ray_amd.hip.Context's k_* methods ---------------------------------------------------
class Host:
    _lib = None

    def __init__(self, path=HOST_LIB):
        if Host._lib is None or path != HOST_LIB:
            L = C.CDLL(path)
            vp, u32 = C.c_void_p, C.c_uint32
            L.hostsim_bvh_last_error.restype = C.c_char_p
            L.hostsim_k_lbvh_build.argtypes = [vp, vp, u32, u32, u32, C.c_int, C.c_int, vp, u32, vp, u32, vp, vp, vp]
            L.hostsim_k_bvh4_collapse.argtypes = [vp, u32, vp, u32, vp, vp, vp]
            L.hostsim_k_bvh4_test_nodes.argtypes = [vp, u32, vp, vp, vp, vp, u32, vp, vp, vp]
            if path != HOST_LIB:
                self.L = L
                return
            Host._lib = L
        self.L = Host._lib

    def check(self, rc):
        if rc != 0:
            raise RuntimeError("hostsim_bvh: " + self.L.hostsim_bvh_last_error().decode())

    def k_lbvh_build(self, boxes, groups, n_groups, leaf_max, leaf_is_primitive, roots_are_nodes):
        boxes = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 6)
        groups = np.ascontiguousarray(groups, dtype=np.uint32)
        n = len(boxes)
        nodes = np.zeros((max(n - 1, 0) + n_groups + 1, 16), dtype=np.uint32)
        entries = np.zeros(2 * n + 1, dtype=np.uint32)
        root = np.zeros(n_groups + 1, dtype=np.uint32)
        bounds = np.zeros(6, dtype=np.float32)
        counts = np.zeros(2, dtype=np.uint32)
        self.check(self.L.hostsim_k_lbvh_build(boxes.ctypes.data, groups.ctypes.data, n, n_groups, leaf_max, int(leaf_is_primitive),
                                               int(roots_are_nodes), nodes.ctypes.data, len(nodes) - 1, entries.ctypes.data, len(entries) - 1,
                                               root.ctypes.data, bounds.ctypes.data, counts.ctypes.data))
        return {"nodes": nodes[:counts[0]].copy(), "entries": entries[:counts[1]].copy(), "group_root": root[:n_groups].copy(), "bounds": bounds}

    def k_bvh4_collapse(self, nodes, roots):
        nodes = np.ascontiguousarray(nodes, dtype=np.uint32).reshape(-1, 16)
        roots = np.ascontiguousarray(roots, dtype=np.uint32)
        wide = np.zeros((len(nodes) + 1, 16), dtype=np.uint32)
        roots4 = np.zeros(len(roots) + 1, dtype=np.uint32)
        count = C.c_uint32(0)
        rc = self.L.hostsim_k_bvh4_collapse(nodes.ctypes.data, len(nodes), roots.ctypes.data, len(roots), wide.ctypes.data, roots4.ctypes.data,
                                            C.addressof(count))
        if rc == 2:
            return None
        self.check(rc)
        return wide[:count.value].copy(), roots4[:len(roots)].copy()

    def k_bvh4_test_nodes(self, wide, node_index, ray_o, ray_d, ray_t):
        wide = np.ascontiguousarray(wide, dtype=np.uint32).reshape(-1, 16)
        node_index = np.ascontiguousarray(node_index, dtype=np.uint32)
        n = len(node_index)
        o, d = (np.ascontiguousarray(a, dtype=np.float32).reshape(n, 3) for a in (ray_o, ray_d))
        t = np.ascontiguousarray(ray_t, dtype=np.float32).reshape(n)
        ref, n_hit, dist = np.zeros((n, 4), np.uint32), np.zeros(n, np.uint32), np.zeros((n, 4), np.float32)
        self.check(self.L.hostsim_k_bvh4_test_nodes(wide.ctypes.data, len(wide), node_index.ctypes.data, o.ctypes.data, d.ctypes.data, t.ctypes.data,
                                                    n, ref.ctypes.data, n_hit.ctypes.data, dist.ctypes.data))
        return ref, n_hit, dist


class Device:
    """the same three calls on a ray_amd.hip.Context"""

    def __init__(self, ctx):
        self.ctx = ctx

    def k_lbvh_build(self, boxes, groups, n_groups, leaf_max, leaf_is_primitive, roots_are_nodes):
        return self.ctx.k_lbvh_build(boxes, groups, n_groups, leaf_max, leaf_is_primitive, roots_are_nodes, on_host=False)

    def k_bvh4_collapse(self, nodes, roots):
        return self.ctx.k_bvh4_collapse(nodes, roots)

    def k_bvh4_test_nodes(self, wide, node_index, ray_o, ray_d, ray_t):
        return self.ctx.k_bvh4_test_nodes(wide, node_index, ray_o, ray_d, ray_t)


# ---- BVH2 words --------------------------------------------------------------------------------------------------------------------
def child_boxes(nodes):
    """[m][16] u32 -> lo [m][2][3], hi [m][2][3] (float32), link [m][2]"""
    f = nodes.view(np.float32)
    lo = np.stack([np.stack([f[:, 0], f[:, 2], f[:, 8]], -1), np.stack([f[:, 4], f[:, 6], f[:, 10]], -1)], 1)
    hi = np.stack([np.stack([f[:, 1], f[:, 3], f[:, 9]], -1), np.stack([f[:, 5], f[:, 7], f[:, 11]], -1)], 1)
    return lo, hi, nodes[:, 12:14]


def make_node(lo0, hi0, link0, lo1, hi1, link1):
    w = np.zeros(16, dtype=np.uint32)
    f = w.view(np.float32)
    f[0], f[1], f[2], f[3], f[8], f[9] = lo0[0], hi0[0], lo0[1], hi0[1], lo0[2], hi0[2]
    f[4], f[5], f[6], f[7], f[10], f[11] = lo1[0], hi1[0], lo1[1], hi1[1], lo1[2], hi1[2]
    w[12], w[13] = link0, link1
    return w


def is_leaf(w):
    return (w & np.uint32(COUNT_BITS)) != 0


def leaf_word(first, count):
    return ((max(count, 2) - 1) << 29) | first


# ---- checker: the linear builder -----------------------------------------------------------------------------------------------------
def _leaf_sets(words, entries, leaf_is_primitive, n_prims):
    """leaf words -> (prims [k][8] int64 with -1 padding, count [k]); a lone primitive (two equal entries) counts once"""
    words = words.astype(np.int64)
    k = len(words)
    prims = np.full((k, 8), -1, dtype=np.int64)
    if leaf_is_primitive:
        assert np.all((words >> 29) == 1), "a top-level leaf is 1 << 29 | primitive"
        prims[:, 0] = words & INDEX_BITS
        assert np.all(prims[:, 0] < n_prims), "a leaf names a primitive outside the input"
        return prims, np.ones(k, dtype=np.int64)
    cnt = (words >> 29) + 1
    first = words & INDEX_BITS
    assert np.all(cnt >= 2), "a leaf word cannot say 1"
    assert np.all(first + cnt <= len(entries)), "a leaf leaves the entries array"
    for j in range(8):
        m = j < cnt
        prims[m, j] = entries[first[m] + j]
    assert np.all(prims[prims >= 0] < n_prims), "an entry names a primitive outside the input"
    lone = (cnt == 2) & (prims[:, 0] == prims[:, 1])
    prims[lone, 1] = -1
    cnt = np.where(lone, 1, cnt)
    return prims, cnt


def _union(boxes, prims):
    """union box of the primitives of each row (prims padded with -1): exact min / max"""
    lo = np.full((len(prims), 3), np.inf, dtype=np.float32)
    hi = np.full((len(prims), 3), -np.inf, dtype=np.float32)
    for j in range(prims.shape[1]):
        m = prims[:, j] >= 0
        if not m.any():
            continue
        b = boxes[prims[m, j]]
        lo[m] = np.minimum(lo[m], b[:, :3])
        hi[m] = np.maximum(hi[m], b[:, 3:])
    return lo, hi


def check_lbvh(boxes, groups, n_groups, leaf_max, flags, out):
    """asserts everything a linear-builder output must satisfy; returns a small census"""
    leaf_is_primitive, roots_are_nodes = flags
    boxes = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 6)
    groups = np.asarray(groups, dtype=np.int64)
    n = len(boxes)
    nodes, entries, group_root = out["nodes"], out["entries"], out["group_root"]
    n_nodes = len(nodes)
    assert len(group_root) == n_groups
    # bounds
    if n:
        want = np.concatenate([boxes[:, :3].min(0), boxes[:, 3:].max(0)])
    else:
        want = np.array([FLT_MAX] * 3 + [-FLT_MAX] * 3, dtype=np.float32)
    assert np.array_equal(out["bounds"], want), ("bounds", out["bounds"], want)
    sizes = np.bincount(groups, minlength=n_groups)
    assert np.array_equal(group_root == NONE, sizes == 0), "group_root is NONE exactly for empty groups"
    live = np.nonzero(sizes > 0)[0]
    links, owner = group_root[live].astype(np.uint32), live
    if roots_are_nodes:
        assert not np.any(is_leaf(links)), "with roots_are_nodes every group's link is a node"
    visits = np.zeros(n_nodes, dtype=np.int64)
    prim_seen = np.zeros(n, dtype=np.int64)
    entry_seen = np.zeros(len(entries), dtype=np.int64)
    lo2, hi2, link2 = child_boxes(nodes) if n_nodes else (np.zeros((0, 2, 3), f32), np.zeros((0, 2, 3), f32), np.zeros((0, 2), np.uint32))

    def account_leaves(words, own, count_entries=True):
        prims, cnt = _leaf_sets(words, entries, leaf_is_primitive, n)
        assert np.all(cnt <= leaf_max), f"a leaf holds {cnt.max()} primitives, leaf_max {leaf_max}"
        real = prims >= 0
        assert np.all(groups[prims[real]] == np.broadcast_to(own[:, None], prims.shape)[real]), "a leaf holds a primitive of another group"
        np.add.at(prim_seen, prims[real], 1)
        if not leaf_is_primitive and count_entries:
            w = words.astype(np.int64)
            c, first = (w >> 29) + 1, w & INDEX_BITS
            for j in range(8):
                m = j < c
                np.add.at(entry_seen, first[m] + j, 1)
        lo, hi = _union(boxes, prims)
        return lo, hi, cnt

    # one-primitive groups under roots_are_nodes: the documented node form, outside the general walk
    if roots_are_nodes:
        single = sizes[owner] == 1
        s_nodes, s_own = links[single], owner[single]
        assert np.all(s_nodes < n_nodes), "a link leaves the node array"
        np.add.at(visits, s_nodes, 1)
        if len(s_nodes):
            w0, w1 = link2[s_nodes, 0], link2[s_nodes, 1]
            assert np.array_equal(w0, w1) and np.all(is_leaf(w0)), "a one-primitive group's node names its leaf twice"
            plo, phi, cnt = account_leaves(w0, s_own)
            assert np.all(cnt == 1)
            assert np.array_equal(lo2[s_nodes, 0], plo) and np.array_equal(hi2[s_nodes, 0], phi), "one-primitive node: first child box"
            if leaf_is_primitive:
                assert np.all(lo2[s_nodes, 1] == FLT_MAX) and np.all(hi2[s_nodes, 1] == FLT_MAX), "top level: second child is the point at FLT_MAX"
            else:
                assert np.array_equal(lo2[s_nodes, 1], plo) and np.array_equal(hi2[s_nodes, 1], phi), "one-triangle mesh: the same box twice"
        links, owner = links[~single], owner[~single]
    # root links that are leaves (refinement: a group small enough to be one leaf)
    rl = is_leaf(links)
    if rl.any():
        account_leaves(links[rl], owner[rl])
    root_nodes = links[~rl]
    # top-down: levels of (node, group)
    levels = []
    cur, own = links[~rl].astype(np.int64), owner[~rl]
    total = 0
    while len(cur):
        assert np.all(cur < n_nodes), "a link leaves the node array"
        total += len(cur)
        assert total <= n_nodes, "more visits than nodes: not a forest"
        np.add.at(visits, cur, 1)
        levels.append((cur, own))
        ch = link2[cur]
        inner = ~is_leaf(ch)
        cur, own = ch[inner].astype(np.int64), np.repeat(own, 2).reshape(-1, 2)[inner]
        assert len(levels) < 4096
    assert np.all(visits == 1), f"nodes array is not dense: {np.count_nonzero(visits == 0)} orphans, {np.count_nonzero(visits > 1)} reached twice"
    # bottom-up: the exact box and the primitive count below every node; stored child boxes must equal them
    sub_lo = np.zeros((n_nodes, 3), dtype=np.float32)
    sub_hi = np.zeros((n_nodes, 3), dtype=np.float32)
    sub_cnt = np.zeros(n_nodes, dtype=np.int64)
    n_leaves = 0
    for cur, own in reversed(levels):
        clo = np.zeros((len(cur), 2, 3), dtype=np.float32)
        chi = np.zeros((len(cur), 2, 3), dtype=np.float32)
        ccnt = np.zeros((len(cur), 2), dtype=np.int64)
        for k in range(2):
            w = link2[cur, k]
            lf = is_leaf(w)
            if lf.any():
                clo[lf, k], chi[lf, k], ccnt[lf, k] = account_leaves(w[lf], own[lf])
                n_leaves += int(lf.sum())
            clo[~lf, k], chi[~lf, k], ccnt[~lf, k] = sub_lo[w[~lf]], sub_hi[w[~lf]], sub_cnt[w[~lf]]
        bad = np.nonzero(np.any((lo2[cur] != clo) | (hi2[cur] != chi), axis=(1, 2)))[0]
        assert len(bad) == 0, f"{len(bad)} nodes store a child box that is not the union of the primitives below, first node {cur[bad[0]]}: " \
                              f"{lo2[cur[bad[0]]]}, {hi2[cur[bad[0]]]} vs {clo[bad[0]]}, {chi[bad[0]]}"
        sub_lo[cur] = np.minimum(clo[:, 0], clo[:, 1])
        sub_hi[cur] = np.maximum(chi[:, 0], chi[:, 1])
        sub_cnt[cur] = ccnt.sum(1)
    # the cut: a range of at most leaf_max primitives is a leaf, so every node holds more -- a group's root under roots_are_nodes aside
    if levels:
        small = np.nonzero(sub_cnt[np.concatenate([c for c, _ in levels])] <= leaf_max)[0]
        small_nodes = np.concatenate([c for c, _ in levels])[small]
        if roots_are_nodes:
            small_nodes = np.setdiff1d(small_nodes, root_nodes)
        assert len(small_nodes) == 0, f"{len(small_nodes)} nodes hold at most leaf_max primitives and should be leaves"
    assert np.all(prim_seen == 1), f"{np.count_nonzero(prim_seen == 0)} primitives in no leaf, {np.count_nonzero(prim_seen > 1)} in several"
    if not leaf_is_primitive:
        assert np.all(entry_seen == 1), "entries are not exactly the leaves' ranges"
    return {"nodes": n_nodes, "depth": len(levels), "leaves": n_leaves}


def same_lbvh(a, b):
    for k in ("nodes", "entries", "group_root", "bounds"):
        x, y = a[k], b[k]
        if k == "bounds":
            x, y = x.view(np.uint32), y.view(np.uint32)
        assert x.shape == y.shape, (k, x.shape, y.shape)
        assert np.array_equal(x, y), f"{k} differ in {np.count_nonzero(x != y)} words"


def node_roots(out):
    """the group links that are node indices (what a collapse can start from)"""
    r = out["group_root"]
    return r[(r != NONE) & ~is_leaf(r)]


# ---- checker: the wide collapse ------------------------------------------------------------------------------------------------------
def half_area32(lo, hi):
    d = (hi - lo).astype(np.float32)
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    with np.errstate(all="ignore"):
        return ((dx * dy).astype(f32) + (dy * dz).astype(f32)).astype(f32) + (dz * dx).astype(f32)


def expected_slots(nodes2, at):
    """wide_children restated: for BVH2 nodes `at` -> ref [m][4], lo [m][4][3], hi [m][4][3], n_slots [m]"""
    lo2, hi2, link2 = child_boxes(nodes2)
    m = len(at)
    ref = np.full((m, 4), EMPTY, dtype=np.uint32)
    lo = np.zeros((m, 4, 3), dtype=np.float32)
    hi = np.zeros((m, 4, 3), dtype=np.float32)
    ref[:, :2], lo[:, :2], hi[:, :2] = link2[at], lo2[at], hi2[at]
    n_slots = np.full(m, 2, dtype=np.int64)
    alive = np.ones(m, dtype=bool)  # (the loop breaks for good once nothing can be opened)
    rows = np.arange(m)
    for _ in range(2):
        valid = np.arange(4)[None, :] < n_slots[:, None]
        area = half_area32(lo, hi)
        with np.errstate(invalid="ignore"):
            cand = valid & ~is_leaf(ref) & (area > np.float32(-1.0)) & alive[:, None]
        best = np.argmax(np.where(cand, area, -np.inf), axis=1)  # (the first of equal areas: the comparison is strict)
        has = cand.any(1)
        alive &= has
        r = rows[has]
        opened = ref[r, best[has]].astype(np.int64)
        assert np.all(opened < len(nodes2))
        ref[r, n_slots[r]], lo[r, n_slots[r]], hi[r, n_slots[r]] = link2[opened, 1], lo2[opened, 1], hi2[opened, 1]
        ref[r, best[has]], lo[r, best[has]], hi[r, best[has]] = link2[opened, 0], lo2[opened, 0], hi2[opened, 0]
        n_slots[r] += 1
    return ref, lo, hi, n_slots


def plane_sign(org, q, step, x):
    """sign of (org + q * step) - x in exact arithmetic.  q * step is exact in float64; the sum is made exact with the error term
    of a two-sum: s = fl(a + b), e = (a + b) - s exactly"""
    a = org.astype(np.float64)
    b = q.astype(np.float64) * step.astype(np.float64)
    x = x.astype(np.float64)
    s = a + b
    bb = s - a
    e = (a - (s - bb)) + (b - bb)
    return np.where(s != x, np.sign(s - x), np.sign(e))


def check_collapse(nodes2, roots, wide, roots4):
    """asserts containment, tightness and structure of a collapse output; returns per wide node the exact child boxes it stands for
    (info: ref, lo, hi, n_slots indexed by wide node) and the canonical form of the wide array"""
    nodes2 = np.ascontiguousarray(nodes2, dtype=np.uint32).reshape(-1, 16)
    n_wide = len(wide)
    wf = wide.view(np.float32)
    info = {"ref": np.full((n_wide, 4), EMPTY, np.uint32), "lo": np.zeros((n_wide, 4, 3), f32), "hi": np.zeros((n_wide, 4, 3), f32),
            "n_slots": np.zeros(n_wide, np.int64)}
    visits = np.zeros(n_wide, dtype=np.int64)
    canon_of = np.full(n_wide, -1, dtype=np.int64)
    order = []
    cur2, cur4, tag = np.asarray(roots, dtype=np.int64), np.asarray(roots4, dtype=np.int64), np.arange(len(roots))
    wide_leaves = []
    while len(cur2):
        assert np.all(cur4 < n_wide), "a wide link leaves the array"
        np.add.at(visits, cur4, 1)
        assert visits.sum() <= n_wide, "more visits than wide nodes"
        canon_of[cur4] = len(np.concatenate(order)) + np.arange(len(cur4)) if order else np.arange(len(cur4))
        order.append(cur4)
        ref, lo, hi, n_slots = expected_slots(nodes2, cur2)
        info["ref"][cur4], info["lo"][cur4], info["hi"][cur4], info["n_slots"][cur4] = ref, lo, hi, n_slots
        w = wide[cur4]
        child = w[:, 4:8]
        valid = np.arange(4)[None, :] < n_slots[:, None]
        leaf = valid & is_leaf(ref)
        inner = valid & ~is_leaf(ref)
        assert np.array_equal(child[leaf], ref[leaf]), "a leaf child is not the word wide_children defines"
        assert np.all(child[~valid] == EMPTY), "an unused slot is not BVH4_EMPTY"
        assert not np.any(is_leaf(child[inner])) and np.all(child[inner] != EMPTY), "an inner child is not a node index"
        # grid: org = node minimum, steps powers of two, the smallest that reach the node maximum
        nlo = np.where(valid[:, :, None], lo, np.inf).min(1).astype(np.float32)
        nhi = np.where(valid[:, :, None], hi, -np.inf).max(1).astype(np.float32)
        org = wf[cur4][:, 0:3]
        assert np.array_equal(org, nlo), "org is not the node minimum"
        stepw = w[:, [3, 14, 15]]
        step = stepw.view(np.float32)
        e = (stepw >> 23).astype(np.int64)
        assert np.all((stepw & np.uint32(0x807FFFFF)) == 0) and np.all((e >= 1) & (e < 254)), "a step is not a power of two"
        q255 = np.full(org.shape, 255.0)
        assert np.all(plane_sign(org, q255, step, nhi) >= 0), "plane 255 does not reach the node maximum"
        loose = (e > 1) & (plane_sign(org, q255, (step * np.float32(0.5)).astype(f32), nhi) >= 0)
        assert not loose.any(), f"{np.count_nonzero(loose.any(1))} nodes have a step twice as large as needed, first BVH2 node {cur2[np.nonzero(loose.any(1))[0][0]]}"
        for a in range(3):
            qlo = ((w[:, 8 + a][:, None] >> (8 * np.arange(4, dtype=np.uint32))[None, :]) & 0xFF).astype(np.int64)
            qhi = ((w[:, 11 + a][:, None] >> (8 * np.arange(4, dtype=np.uint32))[None, :]) & 0xFF).astype(np.int64)
            assert np.all(qlo[~valid] == 0) and np.all(qhi[~valid] == 0), "an unused slot has plane bytes"
            o_, s_ = np.broadcast_to(org[:, a:a + 1], qlo.shape), np.broadcast_to(step[:, a:a + 1], qlo.shape)
            clo, chi = lo[:, :, a], hi[:, :, a]
            v = valid
            assert np.all(plane_sign(o_, qlo, s_, clo)[v] <= 0), "containment: a qlo plane lies above the child's lo"
            assert np.all(plane_sign(o_, qhi, s_, chi)[v] >= 0), "containment: a qhi plane lies below the child's hi"
            t_lo = (qlo == 255) | (plane_sign(o_, qlo + 1, s_, clo) > 0)
            t_hi = (qhi == 0) | (plane_sign(o_, qhi - 1, s_, chi) < 0)
            assert np.all(t_lo[v]), f"tightness: {np.count_nonzero(~t_lo[v])} qlo planes are not the largest below the child's lo (axis {a})"
            assert np.all(t_hi[v]), f"tightness: {np.count_nonzero(~t_hi[v])} qhi planes are not the smallest above the child's hi (axis {a})"
        wide_leaves.append(np.stack([np.repeat(tag, 4).reshape(-1, 4)[leaf], ref[leaf].astype(np.int64)], 1))
        cur2, cur4, tag = ref[inner].astype(np.int64), child[inner].astype(np.int64), np.repeat(tag, 4).reshape(-1, 4)[inner]
    assert np.all(visits == 1), f"wide array: {np.count_nonzero(visits == 0)} orphans, {np.count_nonzero(visits > 1)} reached twice"
    # the leaves under each root: the BVH2 subtree's, as a multiset
    two_leaves = []
    cur, tag = np.asarray(roots, dtype=np.int64), np.arange(len(roots))
    while len(cur):
        ch = nodes2[cur, 12:14]
        lf = is_leaf(ch)
        tg = np.repeat(tag, 2).reshape(-1, 2)
        two_leaves.append(np.stack([tg[lf], ch[lf].astype(np.int64)], 1))
        cur, tag = ch[~lf].astype(np.int64), tg[~lf]
    a = np.concatenate(wide_leaves) if wide_leaves else np.zeros((0, 2), np.int64)
    b = np.concatenate(two_leaves) if two_leaves else np.zeros((0, 2), np.int64)
    a, b = a[np.lexsort((a[:, 1], a[:, 0]))], b[np.lexsort((b[:, 1], b[:, 0]))]
    assert np.array_equal(a, b), "the leaf words under a root are not those of the BVH2 subtree"
    # canonical form: nodes in walk order (roots, then level by level in slot order), inner links renumbered
    order = np.concatenate(order) if order else np.zeros(0, np.int64)
    canon = wide[order].copy()
    ch = canon[:, 4:8]
    inner = ~is_leaf(ch) & (ch != EMPTY)
    ch[inner] = canon_of[ch[inner]].astype(np.uint32)
    canon[:, 4:8] = ch
    return info, canon


# ---- checker: the node test ------------------------------------------------------------------------------------------------------------
def safe_invert32(d):
    d = np.asarray(d, dtype=np.float32)
    den = np.where(np.abs(d) > FLT_EPS, d, np.copysign(FLT_EPS, d)).astype(np.float32)
    return (np.float32(1.0) / den).astype(np.float32)


def reference_slabs(info, node, o, d, t):
    """the two references on the exact fp32 child boxes: (accept32 [n][4], tmin32 [n][4], accept64 [n][4], valid [n][4]).
    fp32: bbox_test of rt_isect.h, operation by operation in float32 (separate multiply and subtract, the 1.00000024f stretch);
    float64: the slab test in real arithmetic on the same box and the same inv_d"""
    o, t = np.asarray(o, np.float32), np.asarray(t, np.float32)
    inv = safe_invert32(d)
    lo, hi = info["lo"][node], info["hi"][node]
    valid = np.arange(4)[None, :] < info["n_slots"][node][:, None]
    with np.errstate(all="ignore"):
        a = (inv[:, None, :] * (lo - o[:, None, :]).astype(f32)).astype(f32)
        b = (inv[:, None, :] * (hi - o[:, None, :]).astype(f32)).astype(f32)
        tmin = np.fmax(np.fmax(np.fmin(a, b)[..., 0], np.fmin(a, b)[..., 1]), np.fmin(a, b)[..., 2])
        tmax = np.fmin(np.fmin(np.fmax(a, b)[..., 0], np.fmax(a, b)[..., 1]), np.fmax(a, b)[..., 2])
        tmax = (tmax * np.float32(1.00000024)).astype(f32)
        acc32 = (tmin <= tmax) & (tmin <= t[:, None]) & (tmax > 0) & valid
        i64, o64 = inv.astype(np.float64), o.astype(np.float64)
        a = i64[:, None, :] * (lo.astype(np.float64) - o64[:, None, :])
        b = i64[:, None, :] * (hi.astype(np.float64) - o64[:, None, :])
        tmin64, tmax64 = np.minimum(a, b).max(-1), np.maximum(a, b).min(-1)
        acc64 = (tmin64 <= tmax64) & (tmin64 <= t[:, None].astype(np.float64)) & (tmax64 > 0) & valid
    return acc32, tmin, acc64, valid


def check_node_test(info, wide, node, o, d, t, result):
    """asserts the contract of bvh4_test_node on every item; returns counts (pairs, accepted by fp32 / float64, hits the references
    both reject)"""
    ref, n_hit, dist = result
    node = np.asarray(node, dtype=np.int64)
    acc32, tmin32, acc64, valid = reference_slabs(info, node, o, d, t)
    words = wide[node][:, 4:8]
    assert np.array_equal(np.sort(ref, 1), np.sort(words, 1)), "ref[] is not a permutation of the node's child words"
    pos = np.arange(4)[None, :]
    is_hit = pos < n_hit[:, None]
    assert np.all(n_hit <= 4)
    assert np.all(dist[is_hit] < FLT_MAX) and np.all(dist[~is_hit] == FLT_MAX), "n_hit does not match the distances"
    assert np.all(np.diff(dist, axis=1) >= 0), "children are not sorted by entry distance"
    assert not np.any(ref[is_hit] == EMPTY), "an empty slot was hit"
    # per slot: hit? at which distance?  (child words of the tested nodes are distinct: see distinct_children)
    eq = ref[:, None, :] == words[:, :, None]  # [item][slot][position]
    where = eq.argmax(2)
    slot_hit = np.take_along_axis(is_hit, where, 1) & valid
    slot_dist = np.take_along_axis(dist, where, 1)
    need = (acc32 | acc64) & valid
    lost = need & ~slot_hit
    assert not lost.any(), f"{np.count_nonzero(lost)} children the reference accepts are reported missed, first item {np.nonzero(lost.any(1))[0][0]}"
    with np.errstate(invalid="ignore"):
        late = slot_hit & (slot_dist > np.fmax(tmin32, np.float32(0.0)))
    assert not late.any(), f"{np.count_nonzero(late)} entry distances exceed the reference's tmin"
    return {"pairs": int(valid.sum()), "acc32": int(acc32.sum()), "acc64": int(acc64.sum()), "extra_hits": int((slot_hit & ~need).sum())}


def distinct_children(wide):
    """indices of the wide nodes whose non-empty child words are all different (a one-triangle mesh names its leaf twice; with equal
    words the output cannot say which slot was hit)"""
    ch = np.sort(wide[:, 4:8].astype(np.int64), 1)
    dup = (ch[:, 1:] == ch[:, :-1]) & (ch[:, 1:] != EMPTY)
    return np.nonzero(~dup.any(1))[0]


# ---- inputs: primitives ------------------------------------------------------------------------------------------------------------------
def _boxes_around(c, half):
    c, half = np.asarray(c, np.float32), np.asarray(half, np.float32)
    # (+ 0.0: no negative zeros -- which of -0 and +0 a min / max returns is unspecified, host and device differ in it, and
    # the builders are compared word for word)
    return np.concatenate([(c - half).astype(f32), (c + half).astype(f32)], 1) + np.float32(0.0)


def random_boxes(rng, n, scale=1.0, size=0.02):
    c = rng.uniform(-1, 1, (n, 3)) * scale
    return _boxes_around(c, rng.uniform(0, size, (n, 3)) * scale)


def groups_refinement(rng, n):
    """groups of 1 to 12 primitives handed over group after group"""
    sizes = rng.integers(1, 13, n)
    g = np.repeat(np.arange(n), sizes)[:n]
    return g.astype(np.uint32), int(g[-1]) + 1 if n else 0


def prim_cases(seed=1):
    """name -> (boxes, groups, n_groups); small and mid-size inputs, every degeneracy the host build digests cleanly"""
    rng = np.random.default_rng(seed)
    cases = {}
    for n in (1, 2, 3, 63, 64, 65, 255, 256, 257, 4097):
        cases[f"one_group_{n}"] = (random_boxes(rng, n), np.zeros(n, np.uint32), 1)
    for n in (3, 257, 4097):
        g, ng = groups_refinement(rng, n)
        cases[f"refinement_{n}"] = (random_boxes(rng, n), g, ng)
    n = 1500
    g, ng = groups_refinement(rng, n)
    cases["gaps"] = (random_boxes(rng, n), (g * 3 + 1).astype(np.uint32), ng * 3 + 2)  # group ids with gaps: empty groups
    cases["interleaved"] = (random_boxes(rng, n), rng.integers(0, 40, n).astype(np.uint32), 40)  # not sorted, not contiguous
    # key degeneracy
    same = np.tile(_boxes_around([[0.25, -0.5, 0.125]], [[0.5, 0.25, 0.125]]), (300, 1))
    same[:, 3:] += rng.uniform(0, 1, (300, 1)).astype(f32) * 0  # (identical centroids, identical boxes)
    cases["identical_centroids"] = (same, np.zeros(300, np.uint32), 1)
    half = rng.uniform(0.01, 0.5, (300, 3))
    cases["identical_centroids_other_boxes"] = (_boxes_around(np.zeros((300, 3)), half), np.zeros(300, np.uint32), 1)
    two = np.where(np.arange(400)[:, None] % 2 == 0, [[-1.0, -1.0, -1.0]], [[2.0, 3.0, 4.0]])
    cases["two_clusters"] = (_boxes_around(two, np.full((400, 3), 0.25)), (np.arange(400) // 100).astype(np.uint32), 4)
    tline = rng.uniform(-1, 1, (500, 1))
    cases["on_a_line"] = (_boxes_around(tline * [[1.0, 2.0, -0.5]], np.full((500, 3), 0.01)), np.zeros(500, np.uint32), 1)
    plane = rng.uniform(-1, 1, (500, 3)) * [[1.0, 1.0, 0.0]]
    cases["on_a_plane"] = (_boxes_around(plane, np.full((500, 3), 0.0)), (np.arange(500) % 3).astype(np.uint32), 3)
    dense = rng.integers(0, 5000, (6000, 3)) / 5000.0  # more than 1024 positions per axis: Morton cells collide
    cases["morton_collisions"] = (_boxes_around(dense, np.full((6000, 3), 1e-4)), np.zeros(6000, np.uint32), 1)
    # box degeneracy
    pts = rng.uniform(-1, 1, (300, 3))
    cases["zero_volume"] = (_boxes_around(pts, np.zeros((300, 3))), (np.arange(300) // 7).astype(np.uint32), 43)
    base = (np.float32(1e6) + rng.integers(0, 64, (300, 3)).astype(f32) * np.spacing(np.float32(1e6))).astype(f32)
    far = np.concatenate([base, base + rng.integers(0, 4, (300, 3)).astype(f32) * np.spacing(np.float32(1e6))], 1).astype(f32)
    cases["far_few_ulp"] = (far, (np.arange(300) // 50).astype(np.uint32), 6)
    ext = np.array([[2.0 ** -100, 1.0, 2.0 ** 100]])
    cases["extents_2pm100"] = (_boxes_around(rng.uniform(-1, 1, (300, 3)) * ext, rng.uniform(0, 0.05, (300, 3)) * ext), np.zeros(300, np.uint32), 1)
    return cases


def overflow_case(seed=2):
    """finite coordinates near FLT_MAX whose centroid sum overflows (lo + hi = inf): the host build digests it -- the centroid is
    inf, the Morton cell clamps -- so it stays an ordinary case for the linear builder; the wide grid cannot hold it"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.7, 0.99, (200, 3)) * float(FLT_MAX)
    b = np.concatenate([c * 0.999, c], 1).astype(np.float32)
    b[::2] *= np.float32(-1.0)
    b[::2] = b[::2][:, [3, 4, 5, 0, 1, 2]]
    return b, np.zeros(200, np.uint32), 1


def large_cases(seed=3):
    """2^20 + 3 primitives: the refinement's shape (about 2^18 groups handed over group after group) and one mesh of that size:
    4097 blocks of 256 threads, more than the device holds at once"""
    rng = np.random.default_rng(seed)
    n = (1 << 20) + 3
    sizes = rng.integers(1, 8, n // 3)
    g = np.repeat(np.arange(len(sizes)), sizes)[:n].astype(np.uint32)
    assert len(g) == n
    centre = rng.uniform(-50, 50, (int(g[-1]) + 1, 3))
    c = centre[g] + rng.uniform(-0.1, 0.1, (n, 3))
    refinement = (_boxes_around(c, rng.uniform(0, 0.02, (n, 3))), g, int(g[-1]) + 1)
    mesh = (random_boxes(rng, n, scale=10.0, size=0.002), np.zeros(n, np.uint32), 1)
    return {"large_refinement": (refinement, REFINE, 2), "large_mesh": (mesh, MESH, 4)}


# ---- inputs: hand-made BVH2 trees for the collapse ---------------------------------------------------------------------------------------
def _leaf(i):
    return (1 << 29) | i


def chain_tree(depth=2000):
    """left-deep: node i = (node i + 1, leaf)"""
    nodes = []
    for i in range(depth):
        hi = np.float32(depth - i)
        inner_lo, inner_hi = np.zeros(3, f32), np.full(3, hi - 1, f32)
        leaf_lo, leaf_hi = np.full(3, hi - 1, f32), np.full(3, hi, f32)
        if i + 1 < depth:
            nodes.append(make_node(inner_lo, inner_hi, i + 1, leaf_lo, leaf_hi, _leaf(2 * i)))
        else:
            nodes.append(make_node(inner_lo, inner_hi, _leaf(2 * i + 2), leaf_lo, leaf_hi, _leaf(2 * i)))
    return np.stack(nodes), np.array([0], np.uint32)


def perfect_tree(levels=9, seed=5, equal_areas=False):
    """heap order; leaves are random boxes (or, equal_areas: congruent boxes, so every sibling pair ties in half-area and the first
    one must be opened)"""
    rng = np.random.default_rng(seed)
    n_inner, n_leaf = (1 << levels) - 1, 1 << levels
    if equal_areas:
        c = np.stack(np.meshgrid(np.arange(n_leaf // 16), np.arange(4), np.arange(4), indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
        lb = _boxes_around(c * 2.0, np.full((n_leaf, 3), 0.5))
    else:
        lb = random_boxes(rng, n_leaf)
    lo = np.zeros((n_inner + n_leaf, 3), f32)
    hi = np.zeros((n_inner + n_leaf, 3), f32)
    lo[n_inner:], hi[n_inner:] = lb[:, :3], lb[:, 3:]
    for i in range(n_inner - 1, -1, -1):
        lo[i], hi[i] = np.minimum(lo[2 * i + 1], lo[2 * i + 2]), np.maximum(hi[2 * i + 1], hi[2 * i + 2])
    link = lambda k: k if k < n_inner else _leaf(2 * (k - n_inner))
    nodes = [make_node(lo[2 * i + 1], hi[2 * i + 1], link(2 * i + 1), lo[2 * i + 2], hi[2 * i + 2], link(2 * i + 2)) for i in range(n_inner)]
    return np.stack(nodes), np.array([0], np.uint32)


def two_leaf_nodes(boxes_a, boxes_b):
    """one root per pair: a node of two leaves with the given boxes"""
    nodes = [make_node(a[:3], a[3:], _leaf(4 * i), b[:3], b[3:], _leaf(4 * i + 2)) for i, (a, b) in enumerate(zip(boxes_a, boxes_b))]
    return np.stack(nodes), np.arange(len(nodes), dtype=np.uint32)


def grid_edge_nodes():
    """node extents just below, at and just above 255 * 2^k, the exponent floor, children flat in one axis, and children whose
    distance from the node minimum rounds onto a grid plane (the widening loops of quantise)"""
    a, b = [], []
    for k in (-20, -3, 0, 7, 40):
        full = np.float32(255.0 * 2.0 ** k)
        for ext in (np.nextafter(full, f32(0)), full, np.nextafter(full, f32(np.inf)), full * f32(0.5), np.nextafter(full * f32(0.5), f32(np.inf))):
            for org in (0.0, -3.0 * 2.0 ** k, 1.0 * 2.0 ** k):
                lo = np.full(3, org, f32)
                a.append(np.concatenate([lo, lo + ext * f32(0.25)]))
                b.append(np.concatenate([lo + ext * f32(0.5), (lo + ext).astype(f32)]))
    tiny = np.float32(2.0 ** -140)  # need so small that the exponent clamps to 1
    a.append(np.array([0, 0, 0, tiny, 0, 1], f32)), b.append(np.array([0, 0, 0, 2 * tiny, 0, 1], f32))  # (and flat in y)
    a.append(np.array([1, 1, 1, 1, 1, 1], f32)), b.append(np.array([1, 1, 1, 1, 1, 1], f32))  # a point
    a.append(np.array([-1, -1, 5, 1, 1, 5], f32)), b.append(np.array([-2, 0, 5, 0, 3, 5], f32))  # flat in z
    # node [-192, 60]: step 1; a child starts 2^-30 below plane 192 and ends 2^-30 above it: fl(lo - org) = 192 exactly
    e = np.float32(2.0 ** -30)
    a.append(np.array([-192, -192, -192, -e, -e, -e], f32)), b.append(np.array([e, e, e, 60, 60, 60], f32))
    a.append(np.array([-192, -192, -192, e, e, e], f32)), b.append(np.array([-e, -e, -e, 60, 60, 60], f32))
    return two_leaf_nodes(a, b)


def unquantisable_nodes():
    """a child box with an infinite coordinate: the grid cannot hold it, the collapse says so (the scene then keeps its BVH2)"""
    a = [np.array([0, 0, 0, 1, 1, 1], f32), np.array([-1, 0, 0, 0, 1, 1], f32)]
    b = [np.array([2, 2, 2, 3, 3, 3], f32), np.array([0, 0, 0, np.inf, 1, 1], f32)]
    return two_leaf_nodes(a, b)


# ---- inputs: rays for the node test ------------------------------------------------------------------------------------------------------
RAY_CATEGORIES = ("aimed", "graze", "origin_inside", "origin_on_face", "origin_on_plane", "axis_parallel_1", "axis_parallel_2", "t_edge",
                  "far_origin", "huge_node")


def _ulp_nudge(x, k):
    x = np.asarray(x, dtype=np.float32).copy()
    for _ in range(4):
        m = k > 0
        x[m] = np.nextafter(x[m], f32(np.inf))
        m2 = k < 0
        x[m2] = np.nextafter(x[m2], f32(-np.inf))
        k = k - np.sign(k)
    return x


def make_rays(category, info, nodes_pool, n, seed):
    """-> (node [n], o [n][3], d [n][3], t [n]) of one category over wide nodes drawn from nodes_pool"""
    rng = np.random.default_rng(seed)
    node = rng.choice(nodes_pool, n)
    slot = (rng.integers(0, 4, n) % info["n_slots"][node]).astype(np.int64)
    lo, hi = info["lo"][node, slot].astype(np.float64), info["hi"][node, slot].astype(np.float64)
    nlo = np.where((np.arange(4)[None, :] < info["n_slots"][node][:, None])[:, :, None], info["lo"][node], np.inf).min(1).astype(np.float64)
    nhi = np.where((np.arange(4)[None, :] < info["n_slots"][node][:, None])[:, :, None], info["hi"][node], -np.inf).max(1).astype(np.float64)
    size = np.maximum((nhi - nlo).max(1, keepdims=True), 1e-30)
    u = rng.uniform(0, 1, (n, 3))
    point = lo + u * (hi - lo)
    dirs = rng.normal(size=(n, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    t = np.full(n, FLT_MAX, dtype=np.float32)
    if category == "aimed":
        # half aimed at a point of the child, half at a point of the node's surroundings
        aim = np.where(rng.uniform(size=(n, 1)) < 0.5, point, nlo + (rng.uniform(-0.5, 1.5, (n, 3))) * (nhi - nlo))
        o = aim - dirs * size * rng.uniform(0.5, 3.0, (n, 1))
        d = dirs
    elif category == "graze":
        # parallel to a face / edge / corner diagonal of the child box, -4 .. 4 ulp outside it in one, two or three axes
        k_axes = rng.integers(1, 4, n)
        on = np.argsort(rng.uniform(size=(n, 3)), 1) < k_axes[:, None]  # the axes that sit on a boundary
        side = rng.integers(0, 2, (n, 3))
        ulps = np.where(rng.uniform(size=(n, 3)) < 0.8, -rng.integers(0, 5, (n, 3)), rng.integers(1, 5, (n, 3)))  # (> 0: outside)
        bound = np.where(side == 1, hi, lo).astype(np.float32)
        out = _ulp_nudge(bound, np.where(side == 1, ulps, -ulps))
        o = np.where(on, out, point)
        d = np.where(on, 0.0, dirs)
        free = ~on.all(1)
        d[~free] = dirs[~free]  # (a corner: any direction)
        o = o - d * size * rng.uniform(0.0, 2.0, (n, 1)) * (~on)
        o = np.where(on, out, o)
    elif category == "origin_inside":
        o, d = point, dirs
        t = (size[:, 0] * rng.uniform(0, 0.3, n) ** 2).astype(np.float32)
    elif category == "origin_on_face":
        ax = rng.integers(0, 3, n)
        side = rng.integers(0, 2, n)
        o = point.copy()
        o[np.arange(n), ax] = np.where(side[:, None] == 1, hi, lo)[np.arange(n), ax]
        inward = np.where(side == 1, -1.0, 1.0)  # 7 in 10 head into the box
        d = dirs.copy()
        d[np.arange(n), ax] = np.abs(d[np.arange(n), ax]) * inward * np.where(rng.uniform(size=n) < 0.7, 1.0, -1.0)
        t = (size[:, 0] * rng.uniform(0, 1.5, n)).astype(np.float32)
    elif category == "origin_on_plane":
        # mostly inside the child, one coordinate moved onto the nearest plane of the node's grid
        ax = rng.integers(0, 3, n)
        o = np.where(rng.uniform(size=(n, 1)) < 0.7, point, nlo + rng.uniform(-0.2, 1.2, (n, 3)) * (nhi - nlo))
        g_org, g_step = info["org"][node, ax].astype(np.float64), info["step"][node, ax].astype(np.float64)
        q = np.clip(np.rint((o[np.arange(n), ax] - g_org) / g_step), 0, 255)
        o[np.arange(n), ax] = g_org + q * g_step
        d = dirs
        t = (size[:, 0] * rng.uniform(0, 1.5, n)).astype(np.float32)
    elif category in ("axis_parallel_1", "axis_parallel_2"):
        zeros = 1 if category == "axis_parallel_1" else 2
        z = np.argsort(rng.uniform(size=(n, 3)), 1) < zeros
        d = np.where(z, np.where(rng.integers(0, 2, (n, 3)) == 1, 0.0, -0.0), np.sign(dirs) * np.maximum(np.abs(dirs), 0.05))
        aim = np.where(rng.uniform(size=(n, 1)) < 0.6, point, nlo + rng.uniform(-0.3, 1.3, (n, 3)) * (nhi - nlo))
        o = aim - d * size * rng.uniform(0.2, 2.0, (n, 1))
    elif category == "t_edge":
        o = point - dirs * size * rng.uniform(0.5, 3.0, (n, 1))
        d = dirs
        o32, d32 = o.astype(np.float32), d.astype(np.float32)
        tmin = reference_slabs(info, node, o32, d32, t)[1][np.arange(n), slot]
        which = rng.choice(3, n, p=[0.4, 0.2, 0.4])
        with np.errstate(invalid="ignore"):
            tm = np.where(np.isfinite(tmin) & (tmin > 0), tmin, f32(1.0)).astype(np.float32)
        t = np.where(which == 0, tm, np.where(which == 1, np.nextafter(tm, f32(-np.inf)), FLT_MAX)).astype(np.float32)
        # (t below the entry of the aimed child: rejected; other children of the node further along: rejected as well)
        t = np.where(rng.uniform(size=n) < 0.05, (tm * f32(0.5)).astype(f32), t)
    elif category == "far_origin":
        # 1e7 node sizes away: the direction's rounding moves the ray by about a node size at the node
        aim = nlo + rng.uniform(-0.5, 1.5, (n, 3)) * (nhi - nlo)
        o = aim - dirs * size * 1e7
        d = dirs
    elif category == "huge_node":
        # the reverse: an origin within 1e-7 node sizes of a face of the child
        ax = rng.integers(0, 3, n)
        side = rng.integers(0, 2, n)
        o = point.copy()
        face = np.where(side[:, None] == 1, hi, lo)[np.arange(n), ax]
        o[np.arange(n), ax] = face + rng.normal(size=n) * size[:, 0] * 1e-7
        d = dirs.copy()
        d[np.arange(n), ax] = np.abs(d[np.arange(n), ax]) * np.where(side == 1, -1.0, 1.0) * np.where(rng.uniform(size=n) < 0.7, 1.0, -1.0)
        t = (size[:, 0] * 10.0 ** rng.uniform(-7.5, -3, n)).astype(np.float32)
    else:
        raise KeyError(category)
    return node, o.astype(np.float32), np.asarray(d, dtype=np.float32), t


def with_grid(info, wide):
    """adds org / step [m][3] of every wide node to `info` (the ray generators place origins on grid planes)"""
    wf = wide.view(np.float32)
    info = dict(info)
    info["org"], info["step"] = wf[:, 0:3].copy(), wf[:, [3, 14, 15]].copy()
    return info


def node_test_trees(builder):
    """name -> (BVH2 nodes, roots): the trees whose wide nodes the node test is run on -- linear-builder outputs of an ordinary
    mesh, of tiny (1e-2) and huge (1e5) ones and of a far one, and the hand-made grid-edge nodes"""
    rng = np.random.default_rng(11)
    trees = {}
    for name, scale, offset in (("unit", 1.0, 0.0), ("tiny", 1e-2, 0.0), ("huge", 1e5, 0.0), ("far", 1.0, 1e4)):
        boxes = random_boxes(rng, 3000, scale=scale, size=0.05)
        boxes = (boxes + np.float32(offset)).astype(np.float32)
        out = builder.k_lbvh_build(boxes, np.zeros(3000, np.uint32), 1, 2, *MESH)
        trees[name] = (out["nodes"], node_roots(out))
    trees["grid_edges"] = grid_edge_nodes()
    return trees
