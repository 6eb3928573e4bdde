"""The spatial radiance cache without a GPU: the host build of ray_amd/csrc/rt_cache.h against the reference's own
Ref::SpatialCacheUpdate / Ref::SpatialCacheResolve (exported by the oracle), bit for bit, and against hand-computed cases.

Needs oracle/_ref/libray_ref.so and tests/hostsim/_build/libhostsim_cache.so (__graft_entry__.build())."""
import ctypes as C
import os

import numpy as np
import pytest

import spatial_cache_util as U
from ray_amd import hip

pytestmark = pytest.mark.skipif(not (os.path.exists(U.REF_LIB) and os.path.exists(U.HOST_LIB)),
                                reason="needs the oracle and the host build (__graft_entry__.build())")

MOVING = [(0.1, 0.2, 2.5), (0.1, 0.2, 2.5), (0.1, 0.2, 2.5), (0.1, 0.2, 0.9), (0.4, -0.1, 0.4), (0.1, 0.2, 2.9)]


def _run_all(wl, *caches):
    for c in caches:
        wl.run(c)
    return [c.readback(0) + c.readback(1)[1:] for c in caches]


def test_static_camera_bit_exact_with_the_reference():
    """five frames of update + resolve with a still camera: key table and both voxel arrays equal the reference's, slot for slot,
    in the reference's serial resolve order and in the device's two-phase order"""
    wl = U.Workload(seed=3, frames=5)
    ref, serial, dev = U.RefCache(), U.HostCache(U.FORM_SERIAL), U.HostCache(U.FORM_DEVICE)
    (kr, vr, cr), (ks, vs, cs), (kd, vd, cd) = _run_all(wl, ref, serial, dev)
    assert np.count_nonzero(kr) > 500
    assert np.count_nonzero(vr[:, 3] & 0xfffff >= 8) > 100
    assert serial.topups() == 0 and dev.topups() == 0  # a still camera: no adjacent-level lookup
    for k, v, c in ((ks, vs, cs), (kd, vd, cd)):
        assert np.array_equal(k, kr) and np.array_equal(v, vr) and np.array_equal(c, cr)
    assert U.buckets_compacted(kr)
    serial.close(), dev.close()


def test_moving_camera_serial_order_bit_exact_and_two_phase_close():
    """a camera that moves between frames exercises the adjacent-level top-up: the serial host form is the reference bit for bit;
    the device's two-phase form may differ in the voxels whose top-up looked into a bucket the serial order had already compacted"""
    wl = U.Workload(seed=5, frames=6, cams=MOVING)
    ref, serial, dev = U.RefCache(), U.HostCache(U.FORM_SERIAL), U.HostCache(U.FORM_DEVICE)
    (kr, vr, _), (ks, vs, _), (kd, vd, _) = _run_all(wl, ref, serial, dev)
    assert np.array_equal(ks, kr) and np.array_equal(vs, vr)
    # the workload must exercise the top-up (594 of them for this seed): without it this is a still-camera test
    assert serial.topups() > 100 and dev.topups() > 100
    mr, md = U.as_map(kr, vr), U.as_map(kd, vd)
    assert set(mr) == set(md)
    differ = sum(mr[k] != md[k] for k in mr)
    assert differ <= 0.02 * len(mr), (differ, len(mr))
    serial.close(), dev.close()


def test_the_cache_answers_queries():
    """after the frames, the query of the shade path finds voxels with >= 8 samples and returns sum / n / exposure; a point in
    empty space gets no answer"""
    wl = U.Workload(seed=3, frames=5)
    h = U.HostCache()
    wl.run(h, exposure=2.0)
    keys, vox = h.readback(0)
    cam = wl.passes[-1][0]
    g = hip.CacheGrid.make(tuple(float(v) for v in cam), 2.0)
    # query at the vertices of the last frame's first bounce
    rays, hits, radiance, dn = wl.passes[-1][1][0]
    v = wl.vertices(rays, hits, radiance, dn)
    pts = np.concatenate([v["o"] + v["t"][:, None] * v["d"], v["n"]], axis=1).astype(np.float32)
    out = h.query(g, pts)
    answered = out[:, 3] > 0
    assert answered.mean() > 0.3
    assert np.all(out[answered, 3] >= 8)
    # one answer by hand: the slot holding the answered point's key
    i = int(np.nonzero(answered)[0][0])
    p = (C.c_float * 3)(*[float(x) for x in pts[i, :3]])
    n = (C.c_float * 3)(*[float(x) for x in pts[i, 3:]])
    key = h.L.hostsim_cache_compute_hash(C.byref(g), C.byref(p), C.byref(n))
    slot = int(np.nonzero(keys == key)[0][0])
    cnt = int(vox[slot, 3] & 0xfffff)
    expect = ((vox[slot, :3].astype(np.float32) / np.float32(1e4)) / np.float32(cnt)) / np.float32(2.0)
    assert np.array_equal(out[i, :3], expect) and out[i, 3] == cnt
    far = np.array([[50.0, 50.0, 50.0, 0.0, 1.0, 0.0]], dtype=np.float32)
    assert np.all(h.query(g, far) == 0)
    h.close()


# ---- hand-computed cases -----------------------------------------------------------------------
def _jenkins(a):
    m = 0xffffffff
    a = ((a + 0x7ed55d16) + (a << 12)) & m
    a = ((a ^ 0xc761c23c) ^ (a >> 19)) & m
    a = ((a + 0x165667b1) + (a << 5)) & m
    a = ((a + 0xd3a2646c) ^ (a << 9)) & m
    a = ((a + 0xfd7046c5) + (a << 3)) & m
    a = ((a ^ 0xb55a4f09) ^ (a >> 16)) & m
    return a


def _bucket(key):
    return ((_jenkins(key & 0xffffffff) ^ _jenkins(key >> 32)) % U.N) // 32 * 32


def _keys_of_bucket(b, count, start=1):
    out, k = [], start
    while len(out) < count:
        if _bucket(k) == b:
            out.append(k)
        k += 1
    return out


def test_hash_and_key_layout():
    h = U.HostCache()
    for key in (1, 0x123456789abcdef, (1 << 63) | 5):
        assert h.L.hostsim_cache_hash64(key) == _jenkins(key & 0xffffffff) ^ _jenkins(key >> 32)
    # camera at the origin, p at distance 3: level floor(log2(3) + 2) = 3, voxel 2^3 / 200 = 0.04
    g = hip.CacheGrid.make((0.0, 0.0, 0.0))
    p, n = (C.c_float * 3)(3.0, 0.0, 0.0), (C.c_float * 3)(-1.0, 0.5, 0.0)
    assert h.L.hostsim_cache_grid_level(C.byref(g), C.byref(p)) == 3
    key = h.L.hostsim_cache_compute_hash(C.byref(g), C.byref(p), C.byref(n))
    gx = int(np.floor(np.float32(3.0) / np.float32(0.04)))
    assert key == gx | (0 << 17) | (0 << 34) | (3 << 51) | ((2 + 4) << 61)
    # a negative coordinate wraps into its 17 bits and the adjacent level decodes it back:
    # camera moved away (curr farther than prev): one level finer, coordinates doubled
    p2 = (C.c_float * 3)(0.0, -3.0, 0.0)
    k2 = h.L.hostsim_cache_compute_hash(C.byref(g), C.byref(p2), C.byref(n))
    gy = int(np.floor(np.float32(-3.0) / np.float32(0.04)))
    assert (k2 >> 17) & 0x1ffff == gy & 0x1ffff
    away = hip.CacheGrid.make((0.0, 5.0, 0.0), 1.0, (0.0, 0.0, 0.0))
    adj = h.L.hostsim_cache_adjacent_hash(k2, C.byref(away))
    assert (adj >> 51) & 0x3ff == 2 and (adj >> 17) & 0x1ffff == (2 * gy) & 0x1ffff and adj >> 61 == k2 >> 61
    closer = hip.CacheGrid.make((0.0, -2.0, 0.0), 1.0, (0.0, 0.0, 0.0))
    adj = h.L.hostsim_cache_adjacent_hash(k2, C.byref(closer))
    assert (adj >> 51) & 0x3ff == 4 and (adj >> 17) & 0x1ffff == (gy // 2) & 0x1ffff
    h.close()


def test_full_bucket_refuses_the_33rd_key():
    h = U.HostCache()
    keys = _keys_of_bucket(4096 * 32, 33)
    slots = [h.insert_key(k) for k in keys]
    assert slots[:32] == list(range(4096 * 32, 4096 * 32 + 32))
    assert slots[32] == 0xffffffff
    assert h.insert_key(keys[5]) == 4096 * 32 + 5  # a key already there is found again
    assert h.find_key(keys[31]) == 4096 * 32 + 31 and h.find_key(keys[32]) == 0xffffffff
    h.close()


def test_compaction_order_and_stale_frames():
    """keys that get samples every frame stay, in their order, at the front of the bucket; keys that get none age one frame per
    resolve and are dropped after 128 idle frames"""
    h = U.HostCache()
    base = 777 * 32
    keys = _keys_of_bucket(base, 6)
    for k in keys:
        h.insert_key(k)
    live = [keys[1], keys[3], keys[4]]
    for frame in range(129):
        for k in live:
            h.accumulate(h.find_key(k), (0.5, 0.25, 0.125), 1)
        h.resolve((0.0, 0.0, 0.0))
        kk, vv = h.readback(0)
        if frame < 128:
            assert list(kk[base:base + 6]) == keys
            idle = vv[base + np.array([0, 2, 5]), 3] >> 20
            assert np.all(idle == frame + 1)
            assert np.all(vv[base + np.array([1, 3, 4]), 3] >> 20 == 0)
    kk, vv = h.readback(0)
    assert list(kk[base:base + 4]) == live + [0]
    assert np.all(vv[base + 3:base + 32] == 0)
    assert U.buckets_compacted(kk)
    h.close()


def test_sample_cap():
    """200 samples of (0.5, 0.25, 0.125): the resolve keeps 128 and scales the sums by 128 / 200"""
    h = U.HostCache()
    key = _keys_of_bucket(99 * 32, 1)[0]
    slot = h.insert_key(key)
    for _ in range(200):
        h.accumulate(slot, (0.5, 0.25, 0.125), 1)
    _, curr = h.readback(1)
    assert list(curr[slot]) == [200 * 5000, 200 * 2500, 200 * 1250, 200]
    h.resolve((0.0, 0.0, 0.0))
    _, prev = h.readback(0)
    k = np.float32(128) / np.float32(200)
    assert list(prev[slot, :3]) == [int(np.float32(v) * k) for v in (1000000, 500000, 250000)]
    assert prev[slot, 3] == 128  # samples capped, frame counter reset by this frame's samples
    h.close()


def test_reset_clears_the_previous_voxels_only():
    wl = U.Workload(seed=7, frames=2)
    h = U.HostCache()
    wl.run(h)
    keys, _ = h.readback(0)
    h.begin_paths(wl.pw * wl.ph)
    h.update(wl.grid(1), wl, *wl.passes[1][1][0])
    _, curr = h.readback(1)
    h.reset()
    k2, prev2 = h.readback(0)
    _, curr2 = h.readback(1)
    assert np.array_equal(k2[keys != 0], keys[keys != 0]) and not prev2.any() and np.array_equal(curr, curr2) and curr.any()
    h.close()
