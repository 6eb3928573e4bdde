"""What new texels for a texture cost on the device (rayhip_scene_set_texture, rayhip_scene_set_texture_device), against the only route
there was: one JSON line per case, everything in one process.

Cases: a box whose pool holds a BC3 (YCoCg), a BC4, a BC5 and an RGBA texture of 64^2, 512^2 and 2048^2 texels with their mip chains
(tests/texture_cases.py: pool_scene), built by the reference's scene code with settings_t::use_tex_compression.  Paths, per texture:
  set_texture          RGBA8 words from host memory: the copy to the device, level 0 compressed, one launch per further level
  set_texture_device   the same from device memory (no copy)
  upload route         what a caller had to do: the reference's AddTexture of the same image on the host (its block compressor and mip
                       builder, one thread: add_texture_ms), the scene export (export_ms) and rayhip_scene_upload_blob into a second
                       context (upload_blob_ms; it also rebuilds every tree); route_ms is their sum
Every device path is called twice first (the first call allocates the staging), then REPS times, alternating between two images; `ms` is
the wall time of a call between two synchronisations (median, with the lowest and highest).

usage: python tools/texture_bench.py [--out profiles/texture_update/texture_bench.jsonl] [--sizes 64 512 2048]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

REPS = 9
TARGETS = ("bc3", "bc4", "bc5_rg", "rgba")


def med(t):
    return {"median": round(float(np.median(t)), 4), "lowest": round(min(t), 4), "highest": round(max(t), 4)}


def measure(L, res):
    import torch
    import texture_cases as T
    import util
    from ray_amd import api, hip
    images = [{t: T.image("gradient" if k else "random", res, res, 1 + k + 10 * j) for j, t in enumerate(TARGETS)} for k in (0, 1)]
    # the upload route, host side: AddTexture of each image alone, then the export of the whole scene
    add_ms = {}
    for t in TARGETS:
        s = api.CreateSceneHIP(use_tex_compression=True)
        times = []
        for k in range(3):
            t0 = time.perf_counter()
            T.add_texture(s, t, images[k & 1][t], True)
            times.append((time.perf_counter() - t0) * 1e3)
        add_ms[t] = round(min(times), 3)
    scene = api.CreateSceneHIP(use_tex_compression=True)
    handles = T.pool_scene(scene, TARGETS, images[0], True)
    export = []
    for _ in range(3):
        t0 = time.perf_counter()
        blob = api.export_scene_blob(scene)
        export.append((time.perf_counter() - t0) * 1e3)

    def context():
        c = hip.Context(0, L)
        c.upload_static(util.pmj())
        c.resize(64, 64)
        c.upload_scene_blob(blob)
        return c

    ctx, ctx_up = context(), context()
    texels = [{t: T.texels_for(t, img[t]) for t in TARGETS} for img in images]
    on_device = [{t: torch.from_numpy(tx[t].view(np.int32)).cuda() for t in TARGETS} for tx in texels]
    torch.cuda.synchronize()
    paths = {}
    for t in TARGETS:
        paths[f"set_texture/{t}"] = (ctx, lambda k, t=t: ctx.set_texture(handles[t], texels[k][t]))
        paths[f"set_texture_device/{t}"] = (ctx, lambda k, t=t: ctx.set_texture_device(handles[t], res, res, on_device[k][t].data_ptr()))
    paths["upload_blob"] = (ctx_up, lambda k: ctx_up.upload_scene_blob(blob) and 0)
    times = {p: [] for p in paths}
    for r in range(2 + REPS):
        for p, (c, run) in paths.items():
            c.sync()
            t0 = time.perf_counter()
            assert not run(r & 1)
            c.sync()
            if r >= 2:
                times[p].append((time.perf_counter() - t0) * 1e3)
    # what the device holds is what the host build makes of the last image set (REPS is odd: set 0 went last)
    want = T.Pool.of_blob(blob)
    for t in TARGETS:
        rc, want = T.host_set_texture(want, handles[t], texels[(1 + REPS) & 1][t])
        assert rc == 0
    assert np.array_equal(T.Pool.of_context(ctx).words, want.words), "the device's pool is not the host build's"
    upload = float(np.median(times["upload_blob"]))
    out = []
    for t in TARGETS:
        route = add_ms[t] + float(np.median(export)) + upload
        out.append({"case": f"{t}_{res}x{res}", "levels": len(want.levels(handles[t])), "ms": {"set_texture": med(times[f"set_texture/{t}"]),
                                                                                             "set_texture_device": med(times[f"set_texture_device/{t}"])},
                    "upload_route": {"add_texture_ms": add_ms[t], "export_ms": round(float(np.median(export)), 3), "upload_blob_ms": round(upload, 3),
                                     "route_ms": round(route, 3)}, "blob_bytes": len(blob), "reps": REPS})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texture_update", "texture_bench.jsonl"))
    ap.add_argument("--sizes", type=int, nargs="*", default=[64, 512, 2048])
    a = ap.parse_args()
    import torch  # noqa: F401  (before librayhip is loaded: torch brings its own HIP runtime, and it must be the one that opens the device)
    from ray_amd import hip
    L = hip.Library()
    assert L.device_count() > 0, "no HIP device"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for res in a.sizes:
            for row in measure(L, res):
                line = json.dumps(row)
                print(line, flush=True)
                f.write(line + "\n")


if __name__ == "__main__":
    main()
