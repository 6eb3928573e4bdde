"""The spatial radiance cache's device kernels (cache_kernels.hip.h) at their edges: dense buckets that make k_cache_compact move keys
in both halves of a wave, full buckets raced by more keys than they hold, one voxel hammered by 2^20 + 5 atomic adds, the SSE2
conversion's edges, geometric edges of the key, level boundaries, a moving camera, and the query.

Every test feeds the device and the host build of rt_cache.h (tests/hostsim/_build/libhostsim_cache.so) identical vertices and
requires equal words, slot for slot where the slot order is deterministic.  The host build itself is held against the reference in
tests/test_spatial_cache_hostsim.py on the same scenarios."""
import os

import numpy as np
import pytest

import spatial_cache_edges as E
import spatial_cache_util as U
from ray_amd import hip

pytestmark = pytest.mark.gpu

MOVING = [(0.1, 0.2, 2.5), (0.1, 0.2, 2.5), (0.1, 0.2, 2.5), (0.1, 0.2, 0.9), (0.4, -0.1, 0.4), (0.1, 0.2, 2.9)]


@pytest.fixture(scope="module")
def lib():
    L = hip.Library()
    if L.device_count() <= 0:
        pytest.skip("no HIP device")
    if not os.path.exists(U.HOST_LIB):
        pytest.skip("host build of the cache missing (__graft_entry__.build())")
    return L


@pytest.fixture
def caches(lib):
    ctx = hip.Context(0, lib)
    dev, host = U.DeviceCache(ctx), U.HostCache()
    yield dev, host
    host.close()
    ctx.cache_enable(False)
    ctx.close()


def _same(dev, host, count, which=(0, 1)):
    """key table and voxel arrays `which` of the first `count` slots, slot for slot"""
    for w in which:
        kd, vd = E.readback(dev, w, count)
        kh, vh = E.readback(host, w, count)
        assert np.array_equal(kd, kh), f"keys differ in {np.count_nonzero(kd != kh)} slots"
        bad = np.nonzero(np.any(vd != vh, axis=1))[0]
        assert len(bad) == 0, f"voxels[{w}] differ in {len(bad)} slots, first {bad[:4]}: {vd[bad[:4]]} vs {vh[bad[:4]]}"
    return kd


# ---- a. dense compaction across both halves of a wave -------------------------------------------------
def test_dense_compaction_both_halves(caches):
    """bucket pairs (2j, 2j+1) with 0-32 keys and their own survival pattern over 130 frames: at frames 1, 128, 129 and 130 the
    device's key table and both voxel arrays are the host build's, slot for slot, and the table keeps its invariants"""
    dev, host = caches
    sc = E.dense_compaction_scenario()
    stats = {}
    before = {}

    def check(frame):
        kd = _same(dev, host, sc.slots)
        E.table_invariants(kd, E.readback(dev, 0, sc.slots)[1])
        stats[frame] = E.coverage(kd, before.get("k"))
        before["k"] = kd

    for s in sc.steps:  # (both caches step by step: the checks compare them between steps)
        if s[0] == "check":
            check(s[1])
        else:
            sc.step(dev, s), sc.step(host, s)
    print("dense compaction coverage:", stats)
    assert stats[1]["ge16"] >= 64 and stats[1]["full"] >= 64 and stats[1]["ge2"] >= 200
    assert stats[129]["moved"] == 0 and stats[130]["moved"] >= 500
    # the stale keys left; the table holds nothing outside the crafted buckets
    kd, vd = E.readback(dev, 0)
    E.table_invariants(kd, vd)
    assert np.count_nonzero(kd) == np.count_nonzero(kd[:sc.slots]) == int(np.sum(sc.survive & (np.arange(32) < sc.counts[:, None])))


# ---- b. full buckets under concurrency ---------------------------------------------------------------
def test_full_buckets_under_concurrency(caches):
    """48 new keys per bucket in one launch into 16 buckets, 8 of which already hold 20: each bucket ends with exactly 32 distinct
    keys of its candidates.  The host build, fed the same vertices with the device's winners first (in the device's slot order),
    picks the same winners; a second bounce that ends every path puts radiance only into the winners' voxels, as on the host"""
    dev, host = caches
    buckets = np.arange(1000, 1016)
    pre = 20
    pos, nrm, keys = E.bucket_points(buckets, pre + 48)
    rng = np.random.default_rng(47)
    n_all = len(buckets) * 48
    span = 32 * 1016
    g = hip.CacheGrid.make(E.DENSE_CAM)
    for c in (dev, host):
        c.begin_paths(n_all)
        for k in range(pre):
            c.update_vertices(g, E.vertices_at(pos[::2, k], nrm[::2, k], (0.5, 0.5, 0.5), np.arange(8, dtype=np.uint32) + 8 * k))
        c.resolve(E.DENSE_CAM)
        c.begin_paths(n_all)
    rad = rng.uniform(0.1, 1.0, size=(len(buckets), 48, 3)).astype(np.float32)
    path = np.arange(n_all, dtype=np.uint32).reshape(len(buckets), 48)
    race = E.vertices_at(pos[:, pre:], nrm[:, pre:], rad.reshape(-1, 3), path.ravel())
    dev.update_vertices(g, race)
    kd, _ = E.readback(dev, 1, span)
    cand = keys[:, pre:]
    overflowed = 0
    for i, b in enumerate(buckets):
        got = kd[32 * b:32 * b + 32]
        assert np.all(got != 0) and len(np.unique(got)) == 32, b
        if i % 2 == 0:
            assert np.array_equal(got[:pre], keys[i, :pre])  # the keys already there keep their slots
            assert np.all(np.isin(got[pre:], cand[i]))
        else:
            assert np.all(np.isin(got, cand[i]))
        overflowed += int(48 + (pre if i % 2 == 0 else 0) > 32)
    print("full buckets: overflowed", overflowed)
    assert overflowed >= 8
    # the host with the device's winners first, in slot order, then the losers
    flat = cand.ravel()
    slot_of = {int(k): s for s, k in enumerate(kd) if k}
    order = sorted(range(n_all), key=lambda i: (slot_of.get(int(flat[i]), 1 << 40), i))
    host.update_vertices(g, race[order])
    _same(dev, host, span, which=(1,))
    # a second bounce ends every path: radiance flows back only into the winners' voxels
    back = E.vertices_at(pos[:, pre:], nrm[:, pre:], (0.3, 0.6, 0.9), path.ravel(), c=(0.5, 2.0, 1.0), ends=1)
    dev.update_vertices(g, back)
    host.update_vertices(g, back[order])
    _same(dev, host, span, which=(1,))
    _, vd = E.readback(dev, 1, span)
    winners = np.isin(flat, kd)
    assert np.count_nonzero(vd[:, 0]) == int(np.sum(winners))  # (the 20 older keys got nothing this frame)
    dev.resolve(E.DENSE_CAM), host.resolve(E.DENSE_CAM)
    _same(dev, host, span)
    # a query at a losing key: the full bucket holds no empty slot to stop at, the key is not there
    lose = np.nonzero(~winners)[0][:8]
    pts = np.concatenate([race["o"][lose], race["n"][lose]], axis=1)
    assert not dev.query(g, pts).any() and not host.query(g, pts).any()


# ---- c. same-address contention ----------------------------------------------------------------------
def test_same_address_contention(caches):
    """2^20 + 5 samples on one key in one launch: the sample counter carries into the frame bits and the radiance sums wrap; 4096
    samples a frame on another key age it.  Device == host == the hand-computed words after the update and after every resolve"""
    dev, host = caches
    keys, a, b = E.contention_frames()
    a_upd, b_upd, a_res, b_res = E.contention_expected()
    span = 32 * 2002
    g = hip.CacheGrid.make(E.DENSE_CAM)
    for frame in range(3):
        for c in (dev, host):
            c.begin_paths(E.BIG + 4096)
            c.update_vertices(g, np.concatenate([a, b]) if frame == 0 else b)
        if frame == 0:
            kd = _same(dev, host, span, which=(1,))
            _, vd = E.readback(dev, 1, span)
            sa, sb = int(np.nonzero(kd == keys[0])[0][0]), int(np.nonzero(kd == keys[1])[0][0])
            assert list(vd[sa]) == a_upd and list(vd[sb]) == b_upd
        for c in (dev, host):
            c.resolve(E.DENSE_CAM)
        kd = _same(dev, host, span)
        _, vd = E.readback(dev, 0, span)
        assert list(vd[sa]) == a_res[frame] and list(vd[sb]) == b_res[frame], frame


# ---- d. conversion edges -----------------------------------------------------------------------------
def test_conversion_edges(caches):
    """radiance 0, denormal, 1e-4 and its neighbours, 214748.36 / .38, 1e30, +-inf, NaN and -1 at exposures 1, 0.5, 3 and 1e-8,
    throughputs holding inf / NaN on the second bounce: the device's words are the host build's (the SSE2 truncation, not the
    device's saturating conversion)"""
    dev, host = caches
    sc = E.conversion_scenario()
    sc.play(dev)
    sc.play(host)
    kd = _same(dev, host, sc.slots)
    assert np.count_nonzero(kd) == 2 * len(E.EDGE_RADIANCE) * len(E.EDGE_EXPOSURES)


def test_conversion_edges_before_resolve(caches):
    dev, host = caches
    sc = E.conversion_scenario()
    sc.steps = sc.steps[:sc.steps.index(("check", "update"))]
    sc.play(dev)
    sc.play(host)
    _same(dev, host, sc.slots, which=(1,))


# ---- e. geometric edges ------------------------------------------------------------------------------
def _inserted_map(cache):
    k, v = E.readback(cache, 1)
    return U.as_map(k, v)


def test_geometric_edges(caches):
    """keys the update inserts for coordinates wrapping past +-2^16, voxel faces, +-0 normal components, a point at the camera,
    distances ~1e6, +-inf and NaN positions: the device's key -> voxel map is the host build's"""
    dev, host = caches
    groups = E.geometric_points()
    total = sum(len(p) for _, p, _ in groups)
    path0 = 0
    for c in (dev, host):
        c.begin_paths(total)
    for cam, p, n in groups:
        g = hip.CacheGrid.make(cam)
        v = E.vertices_at(p, n, (0.5, 0.25, 0.125), np.arange(path0, path0 + len(p), dtype=np.uint32))
        path0 += len(p)
        for i in range(len(v)):  # one vertex per launch: slot order is the host's serial one
            dev.update_vertices(g, v[i:i + 1])
        host.update_vertices(g, v)
    md, mh = _inserted_map(dev), _inserted_map(host)
    assert md == mh
    # the wrap is real: x ~ 1e4 / 0.01 = 1e6 is 82 496 + 7 * 2^17, a 17-bit field with its sign bit set
    xs = [k & 0x1ffff for k in mh if (k >> 51) & 0x3ff == 1 and k & 0x1ffff >= 1 << 16]
    assert len(xs) > 50
    assert {1, 4, 1023} <= {(k >> 51) & 0x3ff for k in mh}


# ---- f. level boundaries -----------------------------------------------------------------------------
def test_level_boundaries(caches):
    """points at 2^k stepped up to 16 floats down and up, k in [-6, 24]: every point's key on the device is the host build's (each
    point carries its own radiance, so a point that lands one level over changes two voxels)"""
    dev, host = caches
    p = E.boundary_points()
    n = np.ones_like(p)
    rad = np.zeros_like(p)
    rad[:, 0] = np.arange(1, len(p) + 1, dtype=np.float32) * np.float32(1e-3)
    rad[:, 1] = 1.0
    g = hip.CacheGrid.make((0.0, 0.0, 0.0))
    v = E.vertices_at(p, n, rad, np.arange(len(p), dtype=np.uint32))
    for c in (dev, host):
        c.begin_paths(len(p))
        c.update_vertices(g, v)
    md, mh = _inserted_map(dev), _inserted_map(host)
    if md != mh:
        hk = np.array([E.compute_hash(g, q, (1.0, 1.0, 1.0)) for q in p], dtype=np.uint64)
        off = [float(p[i, 0]) for i in range(len(p)) if int(hk[i]) not in md]
        pytest.fail(f"{len(off)} of {len(p)} points land in another voxel on the device, e.g. distances {off[:6]}")
    assert len(mh) > 2 * 31


# ---- g. exact contents with a moving camera ----------------------------------------------------------
def _filtered_workload():
    """the moving-camera workload without the vertices whose distance to the camera is within 1e-3 (relative) of a power of two"""
    wl = U.Workload(seed=11, frames=6, cams=MOVING)
    for f, (cam, bounces) in enumerate(wl.passes):
        out = []
        for rays, hits, radiance, dn in bounces:
            p = rays["o"] + hits["t"][:, None] * rays["d"]
            d = np.linalg.norm(p.astype(np.float64) - np.asarray(cam, np.float64), axis=1)
            l2 = np.log2(np.maximum(d, 1e-30))
            keep = np.abs(l2 - np.round(l2)) > 2e-3
            out.append((rays[keep], hits[keep], radiance, dn))
        wl.passes[f] = (cam, out)
    return wl


def _topup_buckets(wl):
    """buckets of the adjacent-level keys that the resolves of a host dry run look up and find"""
    h = U.HostCache()
    found = set()
    cam_prev = (0.0, 0.0, 0.0)
    for f in range(wl.frames):
        cam, bounces = wl.passes[f]
        h.begin_paths(wl.pw * wl.ph)
        for b in bounces:
            h.update(wl.grid(f), wl, *b)
        keys, _ = E.readback(h, 0)
        g = hip.CacheGrid.make(tuple(float(v) for v in cam), 1.0, cam_prev)
        live = set(int(k) for k in keys[keys != 0])
        for k in live:
            a = int(h.L.hostsim_cache_adjacent_hash(k, g))
            if a in live:
                found.add(int(E.bucket_of(np.array([a], dtype=np.uint64))[0]))
        h.resolve(cam)
        cam_prev = tuple(float(v) for v in cam)
    h.close()
    return sorted(found)


def test_moving_camera_exact(caches):
    """the moving-camera workload away from level boundaries, plus filler keys that make the buckets of the top-ups' adjacent-level
    keys dense: the device's key -> voxel map equals the host build's (device resolve order) exactly, with > 100 top-ups"""
    dev, host = caches
    wl = _filtered_workload()
    buckets = _topup_buckets(wl)[:96]
    assert len(buckets) >= 16
    fill = 20
    pos, nrm, _ = E.bucket_points(buckets, fill)
    g0 = hip.CacheGrid.make(E.DENSE_CAM)
    for c in (dev, host):
        c.begin_paths(len(buckets) * fill)
        for k in range(fill):
            c.update_vertices(g0, E.vertices_at(pos[:, k], nrm[:, k], (0.2, 0.2, 0.2), np.arange(len(buckets), dtype=np.uint32) + k * len(buckets)))
        wl.run(c)
    kd, vd = E.readback(dev, 0)
    kh, vh = E.readback(host, 0)
    E.table_invariants(kd, vd)
    md, mh = U.as_map(kd, vd), U.as_map(kh, vh)
    per = np.count_nonzero(kh.reshape(-1, 32)[buckets], axis=1)
    print(f"moving camera: keys {len(mh)}, top-ups {host.topups()}, dense top-up buckets {len(buckets)} (min keys {per.min()})")
    assert host.topups() > 100 and len(mh) > 500
    assert md == mh


# ---- h. query edges ----------------------------------------------------------------------------------
def test_query_edges(caches):
    """queries at voxels with 7, 8 and 200 (capped to 128) samples, at slot 31 of a full bucket, at the 33rd (losing) key of that
    bucket, with update exposure 0.5 and query exposure 2.5: the device answers what the host answers, bit for bit"""
    dev, host = caches
    pos, nrm, keys = E.bucket_points([3000, 3001, 3002, 3003], 33)
    g = hip.CacheGrid.make(E.DENSE_CAM, 0.5)
    counts = [7, 8, 200]
    for c in (dev, host):
        c.begin_paths(512)
        for s in range(200):  # one sample per launch and key
            idx = [i for i in range(3) if s < counts[i]]
            c.begin_paths(512)
            c.update_vertices(g, E.vertices_at(pos[idx, 0], nrm[idx, 0], (0.5, 0.25, 3.0), np.array(idx, dtype=np.uint32)))
        c.begin_paths(512)
        for k in range(33):  # bucket 3003 full of 32 keys, the 33rd loses
            c.update_vertices(g, E.vertices_at(pos[3:, k], nrm[3:, k], (1.0, 2.0, 4.0), np.array([k], dtype=np.uint32)))
        for _ in range(9):  # 9 more samples for every key of the full bucket
            c.begin_paths(512)
            c.update_vertices(g, E.vertices_at(pos[3, :32], nrm[3, :32], (0.125, 0.5, 1.0), np.arange(32, dtype=np.uint32)))
        c.resolve(E.DENSE_CAM)
    q = hip.CacheGrid.make(E.DENSE_CAM, 2.5)
    pts = np.concatenate([np.stack([pos[0, 0], pos[1, 0], pos[2, 0], pos[3, 31], pos[3, 32], pos[3, 0]]),
                          np.stack([nrm[0, 0], nrm[1, 0], nrm[2, 0], nrm[3, 31], nrm[3, 32], nrm[3, 0]])], axis=1)
    qd, qh = dev.query(q, pts), host.query(q, pts)
    assert np.array_equal(qd.view(np.uint32), qh.view(np.uint32)), (qd, qh)
    assert qd[0, 3] == 0 and qd[1, 3] == 8 and qd[2, 3] == 128 and qd[3, 3] == 10 and not qd[4].any()
    # by hand: 8 samples of 0.5 * exposure 0.5 -> 2500 each, sum 20000; 20000 / 1e4 / 8 / 2.5
    f = np.float32
    assert qd[1, 0] == f(f(f(20000) / f(1e4)) / f(8)) / f(2.5)
    kd = E.readback(dev, 0, 32 * 3004)[0]
    assert kd[32 * 3003 + 31] == keys[3, 31] and keys[3, 32] not in kd
