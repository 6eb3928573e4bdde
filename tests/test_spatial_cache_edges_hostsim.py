"""The spatial radiance cache without a GPU, at the edges of its kernels: the scenarios of tests/test_gpu_spatial_cache_edges.py
(dense buckets, full buckets, the sample counter's carry, the SSE2 conversion, geometric edges and level boundaries) through the
reference's own Ref::SpatialCacheUpdate / Ref::SpatialCacheResolve and the host build of rt_cache.h, slot for slot, plus
hand-computed words.  So the device tests' "device == host build" means "device == reference".

Needs oracle/_ref/libray_ref.so and tests/hostsim/_build/libhostsim_cache.so (__graft_entry__.build())."""
import ctypes as C
import os

import numpy as np
import pytest

import spatial_cache_edges as E
import spatial_cache_util as U
from ray_amd import hip

pytestmark = pytest.mark.skipif(not (os.path.exists(U.REF_LIB) and os.path.exists(U.HOST_LIB)),
                                reason="needs the oracle and the host build (__graft_entry__.build())")


def _lockstep(sc, caches, on_check):
    """play a scenario on several caches step by step, calling on_check(label) between steps"""
    for s in sc.steps:
        if s[0] == "check":
            on_check(s[1])
        else:
            for c in caches:
                sc.step(c, s)


def _same_prefix(a, b, count, which=(0, 1)):
    """key table and voxel arrays `which` of the first `count` slots, slot for slot; returns the table and voxels[which[0]]"""
    out = []
    for w in which:
        ka, va = E.readback(a, w, count)
        kb, vb = E.readback(b, w, count)
        assert np.array_equal(ka, kb) and np.array_equal(va, vb), (type(b).__name__, w)
        out.append((ka, va))
    return out[0]


def test_dense_compaction_matches_the_reference():
    """bucket pairs with 0-32 keys and survival patterns over 130 frames (still camera): the reference, the serial host form and
    the device's two-phase form hold the same table and voxels, slot for slot, at frames 1, 128, 129 and 130"""
    sc = E.dense_compaction_scenario()
    ref, serial, dev = U.RefCache(), U.HostCache(U.FORM_SERIAL), U.HostCache(U.FORM_DEVICE)
    stats, before = {}, {}

    def check(frame):
        for c in (serial, dev):
            k, v = _same_prefix(ref, c, sc.slots)
        E.table_invariants(k, v)
        stats[frame] = E.coverage(k, before.get("k"))
        before["k"] = k

    _lockstep(sc, (ref, serial, dev), check)
    print("dense compaction coverage:", stats)
    assert stats[1]["ge16"] >= 64 and stats[1]["full"] >= 64 and stats[130]["moved"] >= 500
    for c in (serial, dev):
        _same_prefix(ref, c, U.N, which=(0,))
    serial.close(), dev.close()


def test_full_buckets_match_the_reference():
    """16 buckets offered 68 keys each in one bounce (serial insert: the first 32 win): reference == host, slot for slot, and the
    bounce that ends every path puts radiance only into the winners -- except the reference's own slip: its hash_map_insert
    hands a losing key slot 0 (RadCacheRef.cpp: cache_entry = 0 on a full bucket), so the losers' samples pile up in slot 0's
    voxel; rt_cache.h answers INVALID_ENTRY and drops them"""
    buckets = np.arange(1000, 1016)
    pos, nrm, keys = E.bucket_points(buckets, 68)
    g = hip.CacheGrid.make(E.DENSE_CAM)
    n = len(buckets) * 68
    path = np.arange(n, dtype=np.uint32)
    first = E.vertices_at(pos, nrm, np.random.default_rng(3).uniform(0.1, 1, size=(n, 3)), path)
    back = E.vertices_at(pos, nrm, (0.3, 0.6, 0.9), path, c=(0.5, 2.0, 1.0), ends=1)
    ref, host = U.RefCache(), U.HostCache(U.FORM_SERIAL)
    span = 32 * 1016
    for c in (ref, host):
        c.begin_paths(n)
        E.feed(c, g, first, 64)
        E.feed(c, g, back, 64)
    kr, vr = E.readback(ref, 1, span)
    kh, vh = E.readback(host, 1, span)
    assert np.array_equal(kr, kh) and np.array_equal(vr[1:], vh[1:])
    assert np.array_equal(kh.reshape(-1, 32)[buckets], keys[:, :32])  # in order of the bounce
    assert np.count_nonzero(vh[:, 3]) == 32 * len(buckets) and not vh[0].any()
    assert kr[0] == 0 and vr[0, 3] == 36 * len(buckets)  # the reference: every loser's sample in (empty) slot 0
    host.close()


def test_conversion_edges_match_the_reference():
    sc = E.conversion_scenario()
    ref, host = U.RefCache(), U.HostCache(U.FORM_SERIAL)
    _lockstep(sc, (ref, host), lambda label: _same_prefix(ref, host, sc.slots))
    host.close()


def test_conversion_table():
    """the SSE2 truncation of radiance x 1e4, by hand: 0x80000000 for NaN, +-inf and |x| >= 2^31 (the device's own conversion
    would saturate), wrap of negative values into the unsigned sums, no add at all for a zero"""
    expect = [0, 0, 1, 0, 1, 0x80000000, 0x80000000, 0x80000000, 0x80000000, 0x80000000, 0x80000000, 0xffffd8f0]
    assert np.array_equal(E.cvtt(E.EDGE_RADIANCE * np.float32(1e4)), np.array(expect, dtype=np.uint32))
    h = U.HostCache()
    for i, r in enumerate(E.EDGE_RADIANCE):
        h.accumulate(i, (float(r), float(r), 0.25), 0)
        h.accumulate(i, (float(r), 0.0, 0.25), 0)
    _, curr = E.readback(h, 1, len(expect))
    e = np.array(expect, dtype=np.uint64)
    assert np.array_equal(curr[:, 0], ((2 * e) & 0xffffffff).astype(np.uint32))
    assert np.array_equal(curr[:, 1], np.array(expect, dtype=np.uint32)) and np.all(curr[:, 2] == 5000) and not curr[:, 3].any()
    h.close()


def test_sample_counter_carry_and_frame_mask():
    """2^20 + 5 samples on one key carry into the frame bits (5 samples, sums wrapped mod 2^32); 4096 samples a frame on another
    make it age as if idle (the reference tests this frame's word with the 12-bit frame mask).  Hand-computed words, and the
    reference's"""
    keys, a, b = E.contention_frames()
    a_upd, b_upd, a_res, b_res = E.contention_expected()
    ref, host = U.RefCache(), U.HostCache(U.FORM_SERIAL)
    span, pw = 32 * 2002, 1024
    for frame in range(3):
        for c in (ref, host):
            c.begin_paths(E.BIG + 4096)
            E.feed(c, hip.CacheGrid.make(E.DENSE_CAM), np.concatenate([a, b]) if frame == 0 else b, pw)
        if frame == 0:
            k, v = _same_prefix(ref, host, span, which=(1,))
            sa, sb = int(np.nonzero(k == keys[0])[0][0]), int(np.nonzero(k == keys[1])[0][0])
            assert list(v[sa]) == a_upd and list(v[sb]) == b_upd
        for c in (ref, host):
            c.resolve(E.DENSE_CAM)
        _, v = _same_prefix(ref, host, span)
        assert list(v[sa]) == a_res[frame] and list(v[sb]) == b_res[frame], frame
    host.close()


def test_geometric_edges_and_level_boundaries_match_the_reference():
    """the keys of the device's geometric-edge and level-boundary points: reference == host build"""
    groups = E.geometric_points() + [((0.0, 0.0, 0.0), E.boundary_points(), np.ones((1023, 3), np.float32))]
    ref, host = U.RefCache(), U.HostCache(U.FORM_SERIAL)
    for cam, p, n in groups:
        g = hip.CacheGrid.make(cam)
        v = E.vertices_at(p, n, (0.5, 0.25, 0.125), np.arange(len(p), dtype=np.uint32))
        for c in (ref, host):
            c.begin_paths(len(p))
            E.feed(c, g, v, 64)
    _same_prefix(ref, host, U.N, which=(1,))
    host.close()


def test_device_level_formula_gives_the_host_levels():
    """the device takes the grid level's logarithms in double, rounded once to float (rt_cache.h log_base): over 2^k stepped up to
    64 floats down and up, k in [-10, 30], that formula's level is the host build's (glibc logf) at every point"""
    h = U.HostCache()
    g = hip.CacheGrid.make((0.0, 0.0, 0.0))
    p = E.boundary_points(-10, 30, 64)
    host = np.array([h.L.hostsim_cache_grid_level(C.byref(g), C.byref((C.c_float * 3)(float(x), 0.0, 0.0))) for x in p[:, 0]])
    q = np.log(p[:, 0].astype(np.float64)).astype(np.float32) / np.float32(np.log(2.0))
    dev = np.clip(np.floor(q + np.float32(2.0)), 1, 1023).astype(np.int64)
    assert len(p) == 41 * 129 and np.array_equal(dev, host), np.nonzero(dev != host)[0][:8]
    # the levels do step in the sweep: 2^k is level k + 2 (k in [2, 12]; at 2^30 glibc's quotient is just below 30, and the
    # device follows it there too), and every k sees both of its levels among its 129 points except where the quotient rounds
    at = 129 * (np.arange(2, 13) + 10)
    assert host[0] == 1 and np.array_equal(host[at], np.arange(4, 15)) and host[129 * 40] == 31
    assert sum(len(set(host[129 * i:129 * i + 129])) == 2 for i in range(41)) >= 10
    h.close()
