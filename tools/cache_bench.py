"""Spatial radiance cache kernels on the device: one JSON line per workload.

  update: the update kernel over a 1080p cache pass (480 x 270 downsampled paths, up to 5 bounces), vertices from the synthetic
          workload of tests/spatial_cache_util.py fed through the test hook rayhip_k_cache_update_vertices; GPU time of
          k_cache_update summed over the bounces (the context's stage time; the hook's host-to-device copy of the vertices,
          `upload_mib_per_pass`, is outside it, and the renderer's own update pass would not make it)
  resolve: GPU time of k_cache_resolve_slots + k_cache_compact on the table the update frames left.  `bytes_min`: what the two
          kernels must move at least -- the key table read twice (2 x 32 MiB) plus, per live key, its two voxels read and the resolved
          one written in phase 1 and read again in phase 2 (64 B) -- and that over the time as a fraction of 8 TB/s

usage: python tools/cache_bench.py [--frames 8] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import spatial_cache_util as U  # noqa: E402
from ray_amd import hip  # noqa: E402

MIB = 1 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = hip.Library()
    if L.device_count() <= 0:
        sys.exit("cache_bench needs a GPU")
    ctx = hip.Context(0, L)
    dev = U.DeviceCache(ctx)
    wl = U.Workload(seed=23, pw=480, ph=270, frames=a.frames, bounces=5)
    lines = []
    upd, res, verts = [], [], []
    for f in range(a.frames):
        cam, bounces = wl.passes[f]
        g = wl.grid(f)
        dev.begin_paths(wl.pw * wl.ph)
        u0, r0 = dev.times_us()
        n = 0
        for b in bounces:
            v = wl.vertices(*b)
            dev.update_vertices(g, v)
            n += len(v)
        dev.resolve(cam)
        u1, r1 = dev.times_us()
        upd.append((u1 - u0) * 1e-3)
        verts.append(n)
        res.append((r1 - r0) * 1e-3)
    keys, _ = ctx.cache_readback(0)
    live = int(np.count_nonzero(keys))
    # the first frame pays first-touch costs: report the median of the rest
    u, r = float(np.median(upd[1:])), float(np.median(res[1:]))
    nv = int(np.median(verts[1:]))
    lines.append({"workload": "cache_update_1080p", "paths": wl.pw * wl.ph, "vertices_per_pass": nv,
                  "upload_mib_per_pass": round(nv * hip.CACHE_VERTEX_DTYPE.itemsize / MIB, 1), "update_ms": round(u, 4),
                  "per_frame_ms": [round(x, 4) for x in upd]})
    bytes_min = 2 * 32 * MIB + 64 * live
    lines.append({"workload": "cache_resolve", "entries": hip.CACHE_ENTRIES, "live_keys": live, "resolve_ms": round(r, 4),
                  "bytes_min": bytes_min, "tb_per_s": round(bytes_min / (r * 1e-3) / 1e12, 3),
                  "fraction_of_8TBps": round(bytes_min / (r * 1e-3) / 8e12, 3), "per_frame_ms": [round(x, 4) for x in res]})
    ctx.cache_enable(False)
    ctx.close()
    out = open(a.out, "w") if a.out else None
    for line in lines:
        s = json.dumps(line)
        print(s)
        if out:
            out.write(s + "\n")
    if out:
        out.close()


if __name__ == "__main__":
    main()
