"""Cases of morph targets on the device (rayhip_morph_create / rayhip_scene_pose; ray_amd/csrc/morph.h): seeded morph sets over the
committed fixture cornell_instances, seeded weights, the host build of the element functions (tests/hostsim/hostsim_morph.cpp) and an
independent numpy restatement of what they compute.  Shared by tests/test_morph_hostsim.py and tests/test_gpu_morph.py.

The fixture has 128 vertices (the four of its triangle light are 20..23), so every launch here is ONE block; launches of many blocks
are held against the host build by tools/morph_bench.py on the scenes it times."""
import ctypes as C
import os

import numpy as np

import skin_cases as S
import util
import vertex_update_cases as V
from ray_amd import hip

MORPH_LIB = os.path.join(util.ROOT, "tests", "hostsim", "_build", "libhostsim_morph.so")
TARGETS = (1, 3, 1025)  # one target, a few, and one more than the device kernels keep in LDS (morph.h: MORPH_LDS_TARGETS = 1024)
ENTRY_DTYPE = np.dtype([("target", "<u4"), ("dp", "<f4", 3), ("dn", "<f4", 3), ("db", "<f4", 3)])
assert ENTRY_DTYPE.itemsize == 40


class MorphSet:
    """base records and targets of vertices [first, first + count) of the scene `a`.  targets: [(vertices uint32 ascending, relative to
    `first`; dp [n][3]; dn [n][3] or None; db [n][3] or None)]"""

    def __init__(self, a: V.Arrays, first, count, targets):
        self.first, self.count = int(first), int(count)
        self.base = a.vertices[first:first + count].copy()
        self.targets = targets

    @property
    def targets_count(self):
        return len(self.targets)

    def row_lengths(self):
        n = np.zeros(self.count, dtype=np.int64)
        for vertices, *_ in self.targets:
            n[vertices] += 1
        return n


def _target(rng, vertices, ext, scale, with_frame=True):
    vertices = np.asarray(sorted(vertices), dtype=np.uint32)
    n = len(vertices)
    dp = (rng.uniform(-0.03, 0.03, size=(n, 3)) * ext * scale).astype(np.float32)
    if not with_frame:
        return (vertices, dp, None, None)
    return (vertices, dp, (rng.uniform(-0.3, 0.3, size=(n, 3)) * scale).astype(np.float32), (rng.uniform(-0.3, 0.3, size=(n, 3)) * scale).astype(np.float32))


def seeded_set(a: V.Arrays, first, count, targets_count, seed):
    """a morph set of 1, 3 or 1025 targets over [first, first + count), count >= 8:
      1     one target over a seeded half of the vertices: rows of length 0 and rows with an entry for every target
      3     target 0 over a seeded half, target 1 over vertices 0, 1 and the LAST vertex -- whose row holds nothing else, so a pose with
            weights[1] == 0 leaves it with entries of weight 0 only -- and without normal / bitangent deltas, target 2 over a seeded
            half; vertex 0 is in all three (an entry for every target), vertex 2 in none
      1025  every target over vertices 1, 4 and count - 2 (dense there: rows longer than any chunk a kernel holds) and over nothing
            else; target 500 moves no vertex at all (count == 0), the odd targets have no normal / bitangent deltas"""
    assert count >= 8 and targets_count in TARGETS
    rng = np.random.RandomState(seed)
    ext = S.extent(a)
    if targets_count == 1:
        return MorphSet(a, first, count, [_target(rng, rng.permutation(count)[:count // 2], ext, 1.0)])
    if targets_count == 3:
        middle = np.arange(3, count - 1)
        half = [set(rng.permutation(middle)[:len(middle) // 2].tolist()) | {0} for _ in range(2)]
        return MorphSet(a, first, count, [_target(rng, half[0], ext, 1.0), _target(rng, {0, 1, count - 1}, ext, 1.0, with_frame=False),
                                          _target(rng, half[1], ext, 1.0)])
    dense = [1, 4, count - 2]
    return MorphSet(a, first, count, [_target(rng, [] if t == 500 else dense, ext, 1.0 / 64, with_frame=t % 2 == 0) for t in range(targets_count)])


def seeded_weights(targets_count, seed):
    """the weights of a pose: -0.5 and 1.5 are among them (artists use both); of three targets the middle one is 0; of 1025 every
    seventh is 0"""
    rng = np.random.RandomState(seed)
    w = rng.uniform(-0.5, 1.5, size=targets_count).astype(np.float32)
    w[0] = -0.5 if seed % 2 else 1.5
    if targets_count == 3:
        w[1], w[2] = 0.0, (1.5 if seed % 2 else -0.5)
    if targets_count > 3:
        w[1], w[2] = 1.5, -0.5
        w[::7][1:] = 0.0
    return w


def standalone_range(a: V.Arrays):
    """the range of skin_cases.seeded_skins(...)[0]: it starts at vertex 1 and its length is no multiple of 64"""
    s = S.seeded_skins(a, 3)[0]
    assert s.first == 1 and s.count % 64 != 0
    return s.first, s.count


def ranges_inside(skin: S.Skin):
    """two disjoint ranges inside `skin` (the long second skin of skin_cases.seeded_skins): the first starts and ends in the middle of the
    skin -- plain segments on both sides -- and none of its boundaries, nor the skin's own start, is at a multiple of 64, as an index
    of the array or within the skin"""
    r = [(skin.first + 13, 30), (skin.first + 56, 21)]
    assert r[1][0] + r[1][1] < skin.first + skin.count
    for b in (skin.first, r[0][0], r[0][0] + r[0][1]):
        assert b % 64 != 0 and (b == skin.first or (b - skin.first) % 64 != 0)
    return r


# ---- the host build -------------------------------------------------------------------------------------------------------------
def have_morph_lib():
    return os.path.exists(MORPH_LIB)


_lib = None


def morph_lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(MORPH_LIB)
        vp, u32 = C.c_void_p, C.c_uint32
        _lib.hostsim_morph_validate.argtypes = [vp, u32, u32, C.POINTER(C.c_int)]
        _lib.hostsim_morph_rows.argtypes = [vp, u32, u32, vp, vp, u32]
        _lib.hostsim_morph_rows.restype = u32
        _lib.hostsim_morph_vertices.argtypes = [vp, vp, vp, u32, vp, vp, vp]
        _lib.hostsim_morph_vertices.restype = u32
        _lib.hostsim_morph_skin_vertices.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp, vp, vp]
        _lib.hostsim_morph_skin_vertices.restype = u32
        _lib.hostsim_morph_lds_targets.restype = u32
    return _lib


def c_targets(targets):
    """(the rayhip_morph_target array of `targets`, the arrays it points into)"""
    keep, out = [], (hip.MorphTarget * max(len(targets), 1))()

    def ptr(x, dtype):
        if x is None:
            return None
        keep.append(np.ascontiguousarray(x, dtype=dtype))
        return keep[-1].ctypes.data

    for k, (vertices, dp, dn, db) in enumerate(targets):
        out[k] = hip.MorphTarget(len(vertices), ptr(vertices, np.uint32), ptr(dp, np.float32), ptr(dn, np.float32), ptr(db, np.float32))
    return out, keep


def host_validate(targets, count, targets_count=None):
    """(the code rayhip_morph_create returns for these targets, which check of morph.h: validate_targets refused them)"""
    arr, keep = c_targets(targets)
    why = C.c_int(0)
    rc = morph_lib().hostsim_morph_validate(C.addressof(arr), len(targets) if targets_count is None else targets_count, count, C.byref(why))
    return rc, int(why.value)


def host_rows(targets, count):
    """(row [count + 1] uint32, entries ENTRY_DTYPE) by the counting sort of morph.h"""
    arr, keep = c_targets(targets)
    row = np.zeros(count + 1, dtype=np.uint32)
    room = sum(len(t[0]) for t in targets)
    entries = np.zeros(room, dtype=ENTRY_DTYPE)
    n = morph_lib().hostsim_morph_rows(C.addressof(arr), len(targets), count, row.ctypes.data, entries.ctypes.data, room)
    assert n == room == row[-1]
    return row, entries


def host_morph(ms: MorphSet, weights, used=None, skin=None, bones=None):
    """(posed VERTEX_DTYPE records of the set, used vertices whose posed position is not finite) by tests/hostsim/hostsim_morph.cpp.
    `skin`: (indices [count][4], weights [count][4]) of the set's vertices and `bones` their palette -- morph, then skin"""
    assert host_validate(ms.targets, ms.count) == (0, 0)
    row, entries = host_rows(ms.targets, ms.count)
    weights = np.ascontiguousarray(weights, dtype=np.float32)
    assert weights.shape == (ms.targets_count,)
    used = None if used is None else np.ascontiguousarray(used, dtype=np.uint8)
    base = np.ascontiguousarray(ms.base)
    out = np.zeros(ms.count, dtype=hip.VERTEX_DTYPE)
    if skin is None:
        bad = morph_lib().hostsim_morph_vertices(base.ctypes.data, row.ctypes.data, entries.ctypes.data, ms.count, weights.ctypes.data,
                                                 None if used is None else used.ctypes.data, out.ctypes.data)
    else:
        idx, sw = np.ascontiguousarray(skin[0], dtype=np.uint16), np.ascontiguousarray(skin[1], dtype=np.float32)
        bones = np.ascontiguousarray(bones, dtype=np.float32)
        assert idx.shape == (ms.count, 4) and sw.shape == (ms.count, 4) and bones.shape[1:] == (3, 4) and idx.max() < len(bones)
        bad = morph_lib().hostsim_morph_skin_vertices(base.ctypes.data, row.ctypes.data, entries.ctypes.data, ms.count, weights.ctypes.data, idx.ctypes.data,
                                                      sw.ctypes.data, bones.ctypes.data, None if used is None else used.ctypes.data, out.ctypes.data)
    return out, int(bad)


def skin_part(skin: S.Skin, ms: MorphSet):
    """the influences of the vertices of `ms` in `skin`, which holds the set"""
    off = ms.first - skin.first
    assert 0 <= off and off + ms.count <= skin.count
    return skin.indices[off:off + ms.count], skin.weights[off:off + ms.count]


def host_morphed(a: V.Arrays, sets, weights, skins=(), palettes=(), vertices=None):
    """the scene's vertex array after rayhip_scene_pose of `sets` at `weights` and `skins` at `palettes` (the host build): a skin's plain
    segments skinned from its rest pose, a set inside a skin morphed then skinned, a set in no skin morphed; everything else as it was"""
    v = S.host_posed(a, skins, palettes, vertices=vertices)
    for ms, w in zip(sets, weights):
        around = [(s, m) for s, m in zip(skins, palettes) if s.first <= ms.first and ms.first + ms.count <= s.first + s.count]
        assert len(around) <= 1
        if around:
            v[ms.first:ms.first + ms.count], bad = host_morph(ms, w, skin=skin_part(around[0][0], ms), bones=around[0][1])
        else:
            v[ms.first:ms.first + ms.count], bad = host_morph(ms, w)
        assert bad == 0
    return v


# ---- numpy restatement: float32, one rounding per operation, the order of morph.h written out -----------------------------------------
def python_rows(targets, count):
    """the row table made the slow way: every (vertex, target) pair, sorted"""
    pairs = sorted((int(v), t, k) for t, (vertices, *_) in enumerate(targets) for k, v in enumerate(vertices))
    row = np.zeros(count + 1, dtype=np.uint32)
    entries = np.zeros(len(pairs), dtype=ENTRY_DTYPE)
    for e, (v, t, k) in enumerate(pairs):
        row[v + 1] += 1
        _, dp, dn, db = targets[t]
        entries[e] = (t, dp[k], dn[k] if dn is not None else (0, 0, 0), db[k] if db is not None else (0, 0, 0))
    return np.cumsum(row, dtype=np.uint32), entries


def numpy_morph(base, targets, weights):
    """posed VERTEX_DTYPE records: target after target in ascending order -- which is, per vertex, the order of its row"""
    f = np.float32
    weights = np.asarray(weights, dtype=f)
    p, n, b = base["p"].copy(), base["n"].copy(), base["b"].copy()
    moved = np.zeros(len(base), dtype=bool)
    zeros = None
    with np.errstate(all="ignore"):
        for t, (vertices, dp, dn, db) in enumerate(targets):
            w = weights[t]
            if w == 0 or len(vertices) == 0:
                continue
            zeros = np.zeros((len(vertices), 3), dtype=f)
            for acc, d in ((p, dp), (n, zeros if dn is None else dn), (b, zeros if db is None else db)):
                term = w * np.asarray(d, dtype=f)
                assert term.dtype == f
                acc[vertices] = acc[vertices] + term
            moved[vertices] = True
        n, b = S._normalised_or_rest(n, base["n"]), S._normalised_or_rest(b, base["b"])
    out = base.copy()
    out["p"][moved], out["n"][moved], out["b"][moved] = p[moved], n[moved], b[moved]
    return out


bits = S.bits
