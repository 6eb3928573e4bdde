"""Spatial radiance cache: crafted inputs at the edges of the cache kernels, shared by tests/test_spatial_cache_edges_hostsim.py
(host build against the reference) and tests/test_gpu_spatial_cache_edges.py (device against the host build).

TEST INFRASTRUCTURE, over the three caches of spatial_cache_util.py: points whose keys land in chosen buckets, the invariants of a
key table, the reference's form of crafted vertices, coverage statistics, and the scenarios themselves."""
import ctypes as C

import numpy as np

from ray_amd import hip
from spatial_cache_util import N, DeviceCache, HostCache, RefCache, buckets_compacted


def readback(cache, which=0, count=N):
    """key table and voxel array `which` (0: resolved, 1: this frame's) of the first `count` slots, from any of the three caches"""
    if isinstance(cache, HostCache):
        keys = np.zeros(count, dtype=np.uint64)
        vox = np.zeros((count, 4), dtype=np.uint32)
        assert cache.L.hostsim_cache_readback(cache.h, keys.ctypes.data, vox.ctypes.data, which, count) == 0
        return keys, vox
    if isinstance(cache, RefCache):
        return cache.entries[:count].copy(), cache.vox[which][:count].copy()
    assert isinstance(cache, DeviceCache)
    return cache.ctx.cache_readback(which, count)


# ---- dense buckets, invariants, coverage ---------------------------------------------------------------
# Dense buckets come from voxel centres of a shell around a camera at the origin: distances 5.2 .. 7.3 are all grid level 4
# (floor(log2(d) + 2), boundaries at 4 and 8), voxel 2^4 / (50 * 2^2) = 0.08.  With the 8 normal octants that is ~20 M keys,
# ~150 per bucket of the 131 072.
DENSE_CAM = (0.0, 0.0, 0.0)
DENSE_LEVEL, DENSE_VOXEL = 4, 0.08


def jenkins32(a: np.ndarray) -> np.ndarray:
    """hash_jenkins32 of rt_cache.h over a uint32 array"""
    a = np.asarray(a, dtype=np.uint32)
    u = np.uint32
    with np.errstate(over="ignore"):
        a = (a + u(0x7ed55d16)) + (a << u(12))
        a = (a ^ u(0xc761c23c)) ^ (a >> u(19))
        a = (a + u(0x165667b1)) + (a << u(5))
        a = (a + u(0xd3a2646c)) ^ (a << u(9))
        a = (a + u(0xfd7046c5)) + (a << u(3))
        a = (a ^ u(0xb55a4f09)) ^ (a >> u(16))
    return a


def bucket_of(keys: np.ndarray) -> np.ndarray:
    """the bucket (slot // 32) a key's hash names"""
    keys = np.asarray(keys, dtype=np.uint64)
    h = jenkins32((keys & np.uint64(0xffffffff)).astype(np.uint32)) ^ jenkins32((keys >> np.uint64(32)).astype(np.uint32))
    return (h % np.uint32(N)) // np.uint32(32)


def pack_key(gx, gy, gz, level, normal_bits) -> np.ndarray:
    m = np.uint64(0x1ffff)
    g = [np.asarray(v).astype(np.int64).astype(np.uint64) & m for v in (gx, gy, gz)]
    return g[0] | (g[1] << np.uint64(17)) | (g[2] << np.uint64(34)) | (np.uint64(level) << np.uint64(51)) | \
        (np.asarray(normal_bits).astype(np.uint64) << np.uint64(61))


def normals_of_bits(bits: np.ndarray) -> np.ndarray:
    """a normal whose octant gives `bits` (component >= 0 <=> bit set)"""
    bits = np.asarray(bits)
    return np.stack([np.where(bits & (1 << i), 1.0, -1.0) for i in range(3)], axis=-1).astype(np.float32)


_lattice = None


def _dense_lattice():
    global _lattice
    if _lattice is None:
        r = np.arange(-94, 95, dtype=np.int32)
        gx, gy, gz = np.meshgrid(r, r, r, indexing="ij")
        gx, gy, gz = gx.ravel(), gy.ravel(), gz.ravel()
        c = (np.stack([gx, gy, gz], axis=1) + 0.5) * DENSE_VOXEL
        d = np.linalg.norm(c, axis=1)
        sel = (d > 5.2) & (d < 7.3)
        _lattice = (np.stack([gx[sel], gy[sel], gz[sel]], axis=1), c[sel].astype(np.float32))
    return _lattice


def compute_hash(g, p, n) -> int:
    """the host build's compute_hash of one point"""
    L = HostCache.lib()
    return int(L.hostsim_cache_compute_hash(C.byref(g), C.byref((C.c_float * 3)(*[float(v) for v in p])),
                                            C.byref((C.c_float * 3)(*[float(v) for v in n]))))


def bucket_points(buckets, count):
    """`count` points (voxel centres at grid level 4 seen from DENSE_CAM) and normals whose keys land in each of `buckets`:
    arrays [len(buckets), count, 3] (positions, normals) and [len(buckets), count] (keys).  Every key is checked against the host
    build's compute_hash."""
    buckets = np.asarray(buckets, dtype=np.uint32)
    g, pts = _dense_lattice()
    want = np.zeros(N // 32, dtype=bool)
    want[buckets] = True
    found = {int(b): [] for b in buckets}
    for nb in range(8):
        keys = pack_key(g[:, 0], g[:, 1], g[:, 2], DENSE_LEVEL, nb)
        b = bucket_of(keys)
        for i in np.nonzero(want[b])[0]:
            lst = found[int(b[i])]
            if len(lst) < count:
                lst.append((i, nb, int(keys[i])))
    pos = np.zeros((len(buckets), count, 3), dtype=np.float32)
    nrm = np.zeros((len(buckets), count, 3), dtype=np.float32)
    keys = np.zeros((len(buckets), count), dtype=np.uint64)
    grid = hip.CacheGrid.make(DENSE_CAM)
    for bi, b in enumerate(buckets):
        lst = found[int(b)]
        assert len(lst) == count, f"bucket {b}: only {len(lst)} candidates"
        for j, (i, nb, key) in enumerate(lst):
            pos[bi, j], nrm[bi, j], keys[bi, j] = pts[i], normals_of_bits(nb), key
            assert compute_hash(grid, pos[bi, j], nrm[bi, j]) == key, (b, j)
    return pos, nrm, keys


def vertices_at(pos, nrm, radiance, path, c=1.0, ends=0) -> np.ndarray:
    """one CACHE_VERTEX_DTYPE record per point: o = the point, t = 0 (o + 0 * d is the point bit for bit)"""
    pos = np.asarray(pos, dtype=np.float32).reshape(-1, 3)
    v = np.zeros(len(pos), dtype=hip.CACHE_VERTEX_DTYPE)
    v["o"], v["t"], v["d"] = pos, 0.0, (0.0, 0.0, 1.0)
    v["n"] = np.asarray(nrm, dtype=np.float32).reshape(-1, 3)
    v["radiance"] = np.broadcast_to(np.asarray(radiance, dtype=np.float32), (len(pos), 3)) if np.ndim(radiance) < 2 else radiance
    v["c"] = c
    v["path"] = path
    v["ends"] = ends
    return v


class _Frame:
    def __init__(self, pw):
        self.img_w = 4 * pw


def reference_bounce(verts: np.ndarray, pw: int):
    """the inverse of Workload.vertices: CACHE_VERTEX_DTYPE records as the reference's rays, hits, radiance and depth-normal images
    (path p is the downsampled pixel (p % pw, p // pw) of a frame img_w = 4 * pw wide)"""
    path = verts["path"].astype(np.uint32)
    x, y = path % pw, path // pw
    ph = int(y.max()) + 1 if len(verts) else 1
    img_w = 4 * pw
    rays = np.zeros(len(verts), dtype=hip.RAY_DTYPE)
    hits = np.zeros(len(verts), dtype=hip.HIT_DTYPE)
    rays["xy"] = (x << np.uint32(16)) | y
    rays["o"], rays["d"], rays["c"], rays["pdf"] = verts["o"], verts["d"], verts["c"], 1.0
    hits["t"], hits["u"] = verts["t"], 0.3
    hits["v"] = np.where(verts["ends"] != 0, -1.0, 0.2).astype(np.float32)
    radiance = np.zeros((img_w * ph, 4), dtype=np.float32)
    dn = np.zeros((img_w * ph, 4), dtype=np.float32)
    pix = y * img_w + x
    radiance[pix, :3] = verts["radiance"]
    dn[pix, :3] = verts["n"]
    dn[pix, 3] = verts["t"]
    return rays, hits, radiance, dn


def feed(cache, g, verts: np.ndarray, pw: int):
    """one bounce of crafted vertices into any of the three caches (the reference through reference_bounce)"""
    if isinstance(cache, RefCache):
        cache.update(g, _Frame(pw), *reference_bounce(verts, pw))
    else:
        cache.update_vertices(g, verts)


def table_invariants(keys: np.ndarray, prev: np.ndarray):
    """a key table (or a prefix of it) and its resolved voxels: every key in the bucket its hash names, no key twice, every bucket
    a prefix of keys, every empty slot's voxel zero"""
    live = np.nonzero(keys)[0]
    assert np.array_equal(bucket_of(keys[live]), (live // 32).astype(np.uint32)), "a key outside its bucket"
    assert len(np.unique(keys[live])) == len(live), "a key held twice"
    assert buckets_compacted(keys), "a bucket with a hole"
    assert not prev[keys == 0].any(), "an empty slot with a non-zero voxel"


def coverage(keys: np.ndarray, before: np.ndarray = None) -> dict:
    """buckets holding >= 2, >= 16 and 32 keys; with `before` (the table one resolve earlier) the kept keys whose slot changed"""
    per = np.count_nonzero(keys.reshape(-1, 32), axis=1)
    out = {"ge2": int(np.sum(per >= 2)), "ge16": int(np.sum(per >= 16)), "full": int(np.sum(per == 32))}
    if before is not None:
        slot_before = {int(k): s for s, k in enumerate(before) if k}
        out["moved"] = sum(1 for s, k in enumerate(keys) if k and slot_before.get(int(k), s) != s)
    return out


# ---- scenarios shared by the host and device tests ----------------------------------------------------
class Scenario:
    """a list of steps -- ("begin", paths), ("update", grid, vertices), ("resolve", cam), ("check", label) -- played the same on any
    of the three caches"""

    def __init__(self, pw):
        self.pw, self.steps = pw, []

    def step(self, cache, s):
        if s[0] == "begin":
            cache.begin_paths(s[1])
        elif s[0] == "update":
            feed(cache, s[1], s[2], self.pw)
        elif s[0] == "resolve":
            cache.resolve(s[1])

    def play(self, cache):
        for s in self.steps:
            self.step(cache, s)


# survival patterns of a bucket pair (2j, 2j+1): key counts of the two buckets and the slots whose key keeps getting samples
def _pair_patterns(j, rng):
    full = np.ones(32, dtype=bool)
    alt = np.arange(32) % 2 == 1
    rnd_lo, rnd_hi = rng.uniform(size=32) < 0.5, rng.uniform(size=32) < 0.5
    n = 1 + (7 * j) % 32  # 1 .. 32 keys
    one = lambda s: np.arange(32) == s  # noqa: E731
    return [
        ((32, n), (full, full)),                      # all survive
        ((n, 32), (~full, ~full)),                    # none survive
        ((32, 32), (one(0), one(0))),                 # only slot 0
        ((32, 32), (one(31), one(31))),               # only slot 31
        ((32, 32), (alt, ~alt)),                      # alternating slots
        ((32, 1 + j % 5), (rnd_lo, one(j % 5))),      # lower full, upper sparse
        ((1 + j % 5, 32), (one(j % 5), rnd_hi)),      # upper full, lower sparse
        ((0, 32), (full, alt)),                       # upper bucket only
        ((n, 33 - n), (rnd_lo, rnd_hi)),              # random
    ][j % 9]


DENSE_PAIRS = 144  # buckets 0 .. 287: slots 0 .. 9215


def dense_compaction_scenario(pairs=DENSE_PAIRS, frames=130):
    """bucket pairs filled with 0-32 keys each, one key per bucket per update call (slot order deterministic everywhere), frame 1;
    then frames 2 .. `frames` in which only each pair's surviving keys get a sample: the others go stale at frame 130.  Checks
    after frames 1, 128, 129 and 130 (labels are frame numbers)."""
    rng = np.random.default_rng(41)
    counts = np.zeros(2 * pairs, dtype=int)
    survive = np.zeros((2 * pairs, 32), dtype=bool)
    for j in range(pairs):
        (counts[2 * j], counts[2 * j + 1]), (survive[2 * j], survive[2 * j + 1]) = _pair_patterns(j, rng)
    pos, nrm, keys = bucket_points(np.arange(2 * pairs), 32)
    rad = rng.uniform(0.05, 2.0, size=(2 * pairs, 32, 3)).astype(np.float32)
    path = np.arange(2 * pairs * 32, dtype=np.uint32).reshape(2 * pairs, 32)
    present = np.arange(32)[None, :] < counts[:, None]
    sc = Scenario(pw=128)
    g = hip.CacheGrid.make(DENSE_CAM)
    for f in range(1, frames + 1):
        sc.steps.append(("begin", 2 * pairs * 32))
        if f == 1:
            for k in range(32):
                b = np.nonzero(counts > k)[0]
                sc.steps.append(("update", g, vertices_at(pos[b, k], nrm[b, k], rad[b, k], path[b, k])))
        else:
            m = present & survive
            sc.steps.append(("update", g, vertices_at(pos[m], nrm[m], rad[m], path[m])))
        sc.steps.append(("resolve", DENSE_CAM))
        if f in (1, 128, 129, 130):
            sc.steps.append(("check", f))
    sc.keys, sc.counts, sc.survive, sc.slots = keys, counts, survive, 2 * pairs * 32
    return sc


# radiance values at the edges of the SSE2 conversion (x RADIANCE_SCALE, truncated; 0x80000000 for NaN and out of range)
EDGE_RADIANCE = np.array([0.0, 1e-40, 1e-4, np.nextafter(np.float32(1e-4), np.float32(0)), np.nextafter(np.float32(1e-4), np.float32(1)),
                          214748.36, 214748.38, 1e30, np.inf, -np.inf, np.nan, -1.0], dtype=np.float32)
EDGE_EXPOSURES = (1.0, 0.5, 3.0, 1e-8)


def cvtt(x) -> np.ndarray:
    """_mm_cvttps_epi32 over float32 values, as uint32 words"""
    x = np.asarray(x, dtype=np.float32)
    ok = (x > np.float32(-2147483904.0)) & (x < np.float32(2147483648.0))
    return np.where(ok, np.trunc(np.where(ok, x, 0)).astype(np.int64), -(1 << 31)).astype(np.int64).astype(np.uint32)


def conversion_scenario():
    """per exposure one key per edge value (x = the value, y and z = the next two), then a second bounce whose throughput holds
    inf / NaN (it flows back into the first key), then a third that ends every path; one resolve"""
    nv = len(EDGE_RADIANCE)
    ne = len(EDGE_EXPOSURES)
    pos, nrm, keys = bucket_points(np.arange(600, 600 + 2 * nv * ne), 1)
    pos, nrm = pos.reshape(ne, 2, nv, 3), nrm.reshape(ne, 2, nv, 3)
    rad = np.stack([np.roll(EDGE_RADIANCE, -s) for s in range(3)], axis=1)
    c2 = np.array([(np.inf, 1.0, 0.5), (np.nan, 2.0, 1.0), (1.0, -np.inf, 0.0), (0.0, 1.0, np.nan)], dtype=np.float32)
    sc = Scenario(pw=16)
    path = np.arange(nv, dtype=np.uint32)
    for e, ex in enumerate(EDGE_EXPOSURES):
        g = hip.CacheGrid.make(DENSE_CAM, ex)
        sc.steps.append(("begin", nv))
        sc.steps.append(("update", g, vertices_at(pos[e, 0], nrm[e, 0], rad, path)))
        sc.steps.append(("update", g, vertices_at(pos[e, 1], nrm[e, 1], rad[::-1], path, c=c2[path % 4])))
        sc.steps.append(("update", g, vertices_at(pos[e, 1], nrm[e, 1], (0.5, 0.25, 2.0), path, c=(0.5, 1.5, 1.0), ends=1)))
    sc.steps.append(("check", "update"))
    sc.steps.append(("resolve", DENSE_CAM))
    sc.steps.append(("check", "resolve"))
    sc.slots = 32 * (600 + 2 * nv * ne)
    return sc


def geometric_points():
    """(camera, positions, normals) groups at the edges of compute_hash"""
    rng = np.random.default_rng(43)
    groups = []
    # grid coordinates past +-2^16 (wrapping into 17 bits): level-1 voxels (0.01) around a camera ~1e4 from the origin
    cam = np.array([10000.0, -7000.5, 3.0], dtype=np.float32)
    p = cam + rng.uniform(-0.3, 0.3, size=(64, 3)).astype(np.float32)
    groups.append((tuple(cam), p, rng.normal(size=(64, 3))))
    # voxel faces: multiples of the level-4 voxel; zero and negative-zero normal components; the camera itself (logf(0): level 1)
    vs = np.float32(16.0) / np.float32(200.0)
    i = rng.integers(-90, 90, size=(64, 3)).astype(np.float32)
    f = (i * vs).astype(np.float32)
    f[:, 0] = np.sign(f[:, 0] + 0.5) * np.float32(6.0)  # keep them in the level-4 shell
    zeros = np.array([[0.0, 0.0, 0.0], [-0.0, -0.0, -0.0], [-0.0, 0.0, -1.0], [0.0, -0.0, 1.0]], dtype=np.float32)
    pz = np.array([[6.0, 0.0, 0.0], [0.0, -6.0, 0.0], [0.0, 0.0, 0.0], [-0.0, -0.0, -0.0]], dtype=np.float32)
    groups.append(((0.0, 0.0, 0.0), np.concatenate([f, pz, pz]), np.concatenate([rng.normal(size=(64, 3)), zeros, zeros[::-1]])))
    # distances around 1e6, and +-inf / NaN positions
    far = rng.normal(size=(32, 3))
    far = (far / np.linalg.norm(far, axis=1, keepdims=True) * rng.uniform(0.9e6, 1.1e6, size=(32, 1))).astype(np.float32)
    bad = np.array([[np.inf, 0, 0], [-np.inf, 1, 2], [0, np.nan, 0], [np.nan, np.nan, np.nan], [np.inf, -np.inf, np.nan], [1, 2, np.inf]],
                   dtype=np.float32)
    groups.append(((0.5, -0.25, 1.0), np.concatenate([far, bad]), rng.normal(size=(38, 3))))
    return [(c, np.asarray(p, np.float32), np.asarray(n, np.float32)) for c, p, n in groups]


def boundary_points(k_lo=-6, k_hi=24, m_max=16):
    """points on the +x axis (camera at the origin: the distance is the coordinate, sqrt(x * x) == x) at 2^k stepped m float
    neighbours down and up, k in [k_lo, k_hi], |m| <= m_max: where floor(log2(d) + 2) changes"""
    out = []
    for k in range(k_lo, k_hi + 1):
        c = np.float32(2.0 ** k)
        lo = hi = c
        out.append(c)
        for _ in range(m_max):
            lo, hi = np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(np.inf))
            out += [lo, hi]
    x = np.array(out, dtype=np.float32)
    return np.stack([x, np.zeros_like(x), np.zeros_like(x)], axis=1)


BIG = (1 << 20) + 5


def contention_frames():
    """frame 1: key A gets 2^20 + 5 samples, key B 4096; frames 2 and 3: B gets 4096 again"""
    pos, nrm, keys = bucket_points([2000, 2001], 1)
    a = vertices_at(np.repeat(pos[0], BIG, axis=0), np.repeat(nrm[0], BIG, axis=0), (0.5, 0.25, 0.125), np.arange(BIG, dtype=np.uint32))
    b = vertices_at(np.repeat(pos[1], 4096, axis=0), np.repeat(nrm[1], 4096, axis=0), (0.75, 0.5, 0.3), np.arange(BIG, BIG + 4096, dtype=np.uint32))
    return keys[:, 0], a, b


def contention_expected():
    """hand-computed words of A and B: after frame 1's update, then after the resolves of frames 1, 2 and 3"""
    m32 = (1 << 32) - 1
    f = np.float32
    a_upd = [(5000 * BIG) & m32, (2500 * BIG) & m32, 1250 * BIG, BIG]  # the sums wrap; the count carries into the frame bits
    b_per = [7500 * 4096, 5000 * 4096, 3000 * 4096]
    b_upd = b_per + [4096]
    # A: 5 samples (the carry left the low 20 bits), this frame's word has a count -> not idle; then idle, one frame per resolve
    a_res = [a_upd[:3] + [5], a_upd[:3] + [5 | (1 << 20)], a_upd[:3] + [5 | (2 << 20)]]
    # B: 4096 samples capped to 128 (k = 1/32); 4096 & 0xfff == 0 -> ages as if idle (the reference's frame-mask test)
    b_res, prev = [], [0, 0, 0, 0]
    for frame in range(3):
        d = [(prev[i] + b_upd[i]) & m32 for i in range(4)]
        count = d[3] & 0xfffff
        k = f(128) / f(count)
        sums = [int(f(f(v) * k)) for v in d[:3]]
        prev = sums + [128 | ((frame + 1) << 20)]
        b_res.append(prev)
    return a_upd, b_upd, a_res, b_res
