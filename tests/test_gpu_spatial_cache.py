"""The spatial radiance cache on the device (rayhip_cache_*): contents against the host build of rt_cache.h after several
update + resolve rounds, the shade-path query, reset, the enable switch, and cache-off renders untouched by it."""
import os

import numpy as np
import pytest

import spatial_cache_util as U
import util
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


def _compare(dev_map, host_map):
    """share of keys on one side only, share of common keys whose four words differ"""
    common = set(dev_map) & set(host_map)
    only = len(set(dev_map) ^ set(host_map)) / max(1, len(set(dev_map) | set(host_map)))
    differ = sum(dev_map[k] != host_map[k] for k in common) / max(1, len(common))
    return only, differ, common


@pytest.mark.parametrize("cams", ["static", "moving"])
def test_device_contents_match_the_host_build(lib, cams):
    """after 6 update + resolve rounds the device's key -> voxel map is the host build's.  The only arithmetic that may differ is the
    device logf of the grid level (a point can land one level over); measured on this workload: no key differs.  Bound: 0.5 %."""
    wl = U.Workload(seed=11, frames=6, cams=MOVING if cams == "moving" else None)
    ctx = hip.Context(0, lib)
    dev, host = U.DeviceCache(ctx), U.HostCache(U.FORM_DEVICE)
    wl.run(dev)
    wl.run(host)
    kd, vd = dev.readback(0)
    kh, vh = host.readback(0)
    assert U.buckets_compacted(kd)
    md, mh = U.as_map(kd, vd), U.as_map(kh, vh)
    assert len(mh) > 500
    only, differ, common = _compare(md, mh)
    print(f"keys {len(mh)}: one side only {only:.5f}, common keys with other words {differ:.5f}")
    assert only <= 0.005 and differ <= 0.005
    # keys with >= 8 samples: sample counts exact, radiance sums to 1e-3
    rich = [k for k in common if (mh[k][3] & 0xfffff) >= 8]
    assert len(rich) > 100
    a = np.array([md[k] for k in rich], dtype=np.float64)
    b = np.array([mh[k] for k in rich], dtype=np.float64)
    assert np.mean((a[:, 3] % (1 << 20)) == (b[:, 3] % (1 << 20))) >= 0.995
    assert np.mean(np.all(np.abs(a[:, :3] - b[:, :3]) <= 1e-3 * np.maximum(b[:, :3], 1.0), axis=1)) >= 0.995
    # the query of the shade path answers what the host build answers
    g = wl.grid(wl.frames - 1)
    v = wl.vertices(*wl.passes[-1][1][0])
    pts = np.concatenate([v["o"] + v["t"][:, None] * v["d"], v["n"]], axis=1).astype(np.float32)
    qd, qh = dev.query(g, pts), host.query(g, pts)
    assert (qh[:, 3] > 0).mean() > 0.3
    assert np.mean(np.all(qd == qh, axis=1)) >= 0.995
    host.close()
    ctx.cache_enable(False)
    ctx.close()


def test_update_before_resolve_matches(lib):
    """one frame's update alone: this frame's voxels (before any resolve) are the host build's, key for key"""
    wl = U.Workload(seed=13, frames=1)
    ctx = hip.Context(0, lib)
    dev, host = U.DeviceCache(ctx), U.HostCache()
    for c in (dev, host):
        c.begin_paths(wl.pw * wl.ph)
        for b in wl.passes[0][1]:
            c.update(wl.grid(0), wl, *b)
    kd, vd = dev.readback(1)
    kh, vh = host.readback(1)
    only, differ, _ = _compare(U.as_map(kd, vd), U.as_map(kh, vh))
    assert only <= 0.005 and differ <= 0.005
    assert dev.times_us()[0] > 0
    host.close()
    ctx.close()


def test_reset_clears_previous_voxels_only(lib):
    wl = U.Workload(seed=17, frames=2)
    ctx = hip.Context(0, lib)
    dev = U.DeviceCache(ctx)
    wl.run(dev)
    keys, prev = dev.readback(0)
    assert prev.any()
    dev.begin_paths(wl.pw * wl.ph)
    dev.update(wl.grid(1), wl, *wl.passes[1][1][0])
    _, curr = dev.readback(1)
    dev.reset()
    k2, prev2 = dev.readback(0)
    _, curr2 = dev.readback(1)
    assert np.array_equal(k2, keys) and not prev2.any() and np.array_equal(curr2, curr) and curr.any()
    ctx.close()


def test_enable_switch(lib):
    """every cache call fails while the cache is off; enabling gives an empty table; disabling frees it"""
    ctx = hip.Context(0, lib)
    with pytest.raises(RuntimeError, match="not enabled"):
        ctx.cache_resolve((0.0, 0.0, 0.0))
    ctx.cache_enable(True)
    keys, vox = ctx.cache_readback(0)
    assert not keys.any() and not vox.any()
    with pytest.raises(RuntimeError, match="begin_paths"):
        ctx.k_cache_update_vertices(hip.CacheGrid.make((0.0, 0.0, 0.0)), np.zeros(1, dtype=hip.CACHE_VERTEX_DTYPE))
    ctx.k_cache_begin_paths(4)
    bad = np.zeros(1, dtype=hip.CACHE_VERTEX_DTYPE)
    bad["path"] = 4
    with pytest.raises(RuntimeError, match="path 4 of 4"):
        ctx.k_cache_update_vertices(hip.CacheGrid.make((0.0, 0.0, 0.0)), bad)
    # two vertices of one path in a call would race on the path's state: refused, nothing written
    twice = np.zeros(2, dtype=hip.CACHE_VERTEX_DTYPE)
    twice["path"] = 1
    twice["t"] = 1.0
    twice["d"] = (0.0, 0.0, 1.0)
    with pytest.raises(RuntimeError, match="second time"):
        ctx.k_cache_update_vertices(hip.CacheGrid.make((0.0, 0.0, 0.0)), twice)
    keys, vox = ctx.cache_readback(1)
    assert not keys.any() and not vox.any()
    ctx.cache_enable(False)
    with pytest.raises(RuntimeError, match="not enabled"):
        ctx.cache_readback(0, 16)
    ctx.close()


def test_cache_off_render_unchanged_by_a_cache_elsewhere(lib):
    """a render on a context without the cache is bit-identical whether or not another context holds a populated cache"""
    a = util.make_context(lib, "cornell_principled")
    a.render(1)
    first = a.readback(hip.BUF_RAW).copy()
    a.close()
    other = hip.Context(0, lib)
    wl = U.Workload(seed=19, frames=2)
    wl.run(U.DeviceCache(other))
    b = util.make_context(lib, "cornell_principled")
    b.render(1)
    second = b.readback(hip.BUF_RAW).copy()
    b.close()
    other.close()
    assert np.array_equal(first, second)


def test_stale_keys_dropped_and_buckets_compacted(lib):
    """130 frames in which only every other key gets a sample: the idle keys go stale after 128 frames and leave their buckets; the
    device's compaction (which writes only the slots whose content changes) leaves the host build's key -> voxel map, every bucket
    a prefix of keys"""
    rng = np.random.default_rng(29)
    n = 4000
    verts = np.zeros(n, dtype=hip.CACHE_VERTEX_DTYPE)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    verts["o"] = (0.1, 0.2, 0.3)
    verts["d"] = d
    verts["t"] = rng.uniform(0.5, 4.0, size=n).astype(np.float32)
    verts["n"] = -d
    verts["radiance"] = rng.uniform(0.1, 1.0, size=(n, 3)).astype(np.float32)
    verts["c"] = 1.0
    verts["path"] = np.arange(n, dtype=np.uint32)
    g = hip.CacheGrid.make((0.1, 0.2, 0.3))
    ctx = hip.Context(0, lib)
    dev, host = U.DeviceCache(ctx), U.HostCache()
    for frame in range(131):
        vs = verts if frame == 0 else verts[::2]
        for c in (dev, host):
            c.begin_paths(n)
            c.update_vertices(g, vs)
            c.resolve((0.1, 0.2, 0.3))
        if frame in (1, 128, 130):
            kd, vd = dev.readback(0)
            kh, vh = host.readback(0)
            assert U.buckets_compacted(kd)
            md, mh = U.as_map(kd, vd), U.as_map(kh, vh)
            assert md == mh, frame
            idle = sum((v[3] >> 20) > 0 for v in mh.values())
            if frame == 128:
                assert idle > 500, idle  # the unsampled half, 128 frames idle: still there
                before = len(mh)
    # after 129 idle frames the unsampled half is gone: the survivors are the sampled keys
    assert idle == 0 and 0 < len(mh) < before - 500
    host.close()
    ctx.close()
