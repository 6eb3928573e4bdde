"""What changing the environment costs on the device (rayhip_scene_set_environment, rayhip_scene_set_env_map, rayhip_scene_set_sky),
against the only route there was: one JSON line per scene, everything in one process.

Scenes (tests/env_cases.py): the Cornell room under an HDR map of 128 x 64 and of 2048 x 1024 texels (env_scene), and under the
physical sky at envmap_resolution 64 and 512 (sky_scene), each built by the reference's scene code.  Paths:
  set_environment  colours and rotations: no launch
  set_env_map      new texels from host memory, the quadtree rebuilt, the environment leaf's flux, the light tree refitted
  set_sky          the sun's record and a rayhip_sky with its tables, the map re-baked in place, then as set_env_map
  upload_blob      rayhip_scene_upload_blob of the same scene in a second context: what a caller of the C ABI had to do (the host's
                   scene build, sky bake and quadtree are not in the figure)
  host_loop_ms     the quadtree of the same map by the host build of env_qtree.h (tests/hostsim/hostsim_environment.cpp: the loop of
                   Scene::PrepareEnvMapQTree, 25 taps per cell, one thread), on the machine the tool runs on
Every path is called twice first (the first call allocates), then REPS times in turn with the others, alternating between two sets of
inputs; `ms` is the wall time of an untraced call between two synchronisations (median, with the lowest and highest), `phases_ms` the
differences of the RAYHIP_TRACE_UPLOAD stamps of one more call -- each stamp waits for the device first.

usage: python tools/environment_bench.py [--cache DIR] [--out profiles/environment/environment_bench.jsonl]
  --cache DIR   keep the reference-built scene blobs there and use the ones that are there (the sky bake at 512 takes the host a while)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

REPS = 9


def cached(cache, name, build):
    path = os.path.join(cache, name + ".rayscene") if cache else None
    if path and os.path.exists(path):
        with open(path, "rb") as f:
            return f.read()
    blob = build()
    if path:
        os.makedirs(cache, exist_ok=True)
        with open(path, "wb") as f:
            f.write(blob)
    return blob


def blobs(cache):
    import env_cases as E
    maps = {"map_128x64": [E.sky_map(), E.sky_map(sun_dir=E.MOVED_SUN)], "map_2048x1024": [E.sky_map(2048, 1024), E.sky_map(2048, 1024, sun_dir=E.MOVED_SUN)]}
    out = {}
    for name, imgs in maps.items():
        out[name] = ("map", cached(cache, name, lambda: E.reference_blob(("bench", name), lambda s: E.env_scene(s, imgs[0]))), imgs)
    for res in (64, 512):
        pair = [cached(cache, f"sky_{res}_{k}", lambda: E.reference_blob(("bench", res, k), lambda s: E.sky_scene(s, moved=bool(k), envmap_resolution=res))) for k in (0, 1)]
        out[f"sky_{res}"] = ("sky", pair[0], pair)
    return out


def measure(L, name, kind, blob, inputs):
    import env_cases as E
    import light_refit_cases as LR
    from instance_pose_bench import stamps_of
    from light_pose_bench import context
    from vertex_update_bench import traced
    ctx, ctx_up = context(L, blob, True), context(L, blob, False)
    paths = {"set_environment": (ctx, lambda k: ctx.set_environment((1.0, 1.0 - 0.1 * k, 1.0), (1.0, 1.0, 1.0), 0.3 + k, 0.3))}
    if kind == "map":
        paths["set_env_map"] = (ctx, lambda k: ctx.set_env_map(inputs[k]))
    else:
        args = []
        for b in inputs:
            slots = E.section(b, "sky_dir_lights", "<u4")
            args.append((slots, LR.Arrays(b).lights[slots], E.section(b, "sky", np.uint8), E.section(b, "sky_transmittance_lut", "<f4"),
                         E.section(b, "sky_multiscatter_lut", "<f4")))
        paths["set_sky"] = (ctx, lambda k: ctx.set_sky(*args[k]))
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
    phases = {}
    for p in paths:
        if p.startswith("set_") and p != "set_environment":
            _, log = traced(lambda: paths[p][1](0))
            phases[p] = stamps_of(log)[0]
    _, w, h = E.blob_env_map(blob)
    texels = ctx.read_accel(14).reshape(h, w)
    t0 = time.perf_counter()
    host = E.host_pyramid(texels)
    host_ms = (time.perf_counter() - t0) * 1e3
    env = ctx.read_accel(13)
    return {"scene": name, "map": [w, h], "res": host.res, "levels_kept": int(env[12].view(np.int32)), "blob_bytes": len(blob),
            "ms": {p: {"median": round(float(np.median(t)), 4), "lowest": round(min(t), 4), "highest": round(max(t), 4)} for p, t in times.items()},
            "phases_ms": phases, "host_loop_ms": round(host_ms, 2), "reps": REPS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cache", default=None)
    ap.add_argument("--build-only", action="store_true", help="build the scene blobs into --cache and stop (needs no GPU)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "environment", "environment_bench.jsonl"))
    a = ap.parse_args()
    scenes = blobs(a.cache)
    if a.build_only:
        return
    import torch  # noqa: F401  (before librayhip is loaded: torch brings its own HIP runtime, and it must be the one that opens the device)
    from ray_amd import hip
    L = hip.Library()
    assert L.device_count() > 0, "no HIP device"
    with open(a.out, "w") as f:
        for name, (kind, blob, inputs) in scenes.items():
            line = json.dumps(measure(L, name, kind, blob, inputs))
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
