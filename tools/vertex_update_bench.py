"""What a vertex update costs on the device, against the only route there was before it: one JSON line per scene.

  update:  rayhip_scene_update_vertices_blob(B) on a context that uploaded A -- B is A with its vertices displaced by a wave (the vertices of
           triangle lights stay).  The THIRD call is timed (the first allocates the builders' scratch buffers); its phases come from the
           RAYHIP_TRACE_UPLOAD stamps, each of which waits for the device first: vertices copied, triangle records, boxes refitted,
           tri_verts, the 4-wide collapse, the top level.  `update_ms` is the wall time of a call WITHOUT the trace.
  before:  rayhip_scene_upload_blob(B) (`upload_ms`, its second call) plus the host scene build that makes B's arrays in the first place
           (`scene_build_s`: the reference's serial SAH over the scene's meshes, through the drop-in's host library; null where that library
           is not built) -- reported separately, they are different machines' work.

Scenes: atrium_small, and the headline atrium (bench.py: bistro) if bench.py's scene cache holds it -- it is not built here.

usage: python tools/vertex_update_bench.py [--out profiles/vertex_update/refit_bench.jsonl]
"""
import argparse
import json
import os
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import util  # noqa: E402
import vertex_update_cases as V  # noqa: E402
from ray_amd import api, hip, scenes  # noqa: E402


def displaced(blob):
    """the scene with every vertex that no triangle light uses moved along y by a wave of 2 % of the scene's height"""
    a = V.Arrays(blob)
    v = a.vertices.copy()
    t = a.tri_indices[a.reachable_entries()].astype(np.int64)
    used = np.unique(np.concatenate([a.vtx_indices[3 * t], a.vtx_indices[3 * t + 1], a.vtx_indices[3 * t + 2]]))
    p = v["p"][used]
    ext = p.max(axis=0) - p.min(axis=0)
    dy = (0.02 * ext[1] * np.sin(p[:, 0] * (25.0 / ext[0])) * np.cos(p[:, 2] * (19.0 / ext[2]))).astype(np.float32)
    dy[np.isin(used, a.light_vertices())] = 0.0
    v["p"][used, 1] = p[:, 1] + dy
    return V.patched_blob(blob, vertices=v), dict(vertices=int(len(used)), entries=int(len(a.tri_indices)), unique_triangles=int(len(np.unique(t))),
                                                   bvh2_nodes=int(len(a.nodes)), light_vertices=len(a.light_vertices()))


def traced(fn):
    """(result, stderr text) of fn() with RAYHIP_TRACE_UPLOAD set: the library writes its stamps to the C stderr"""
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as f:
        os.dup2(f.fileno(), 2)
        os.environ["RAYHIP_TRACE_UPLOAD"] = "1"
        try:
            out = fn()
        finally:
            del os.environ["RAYHIP_TRACE_UPLOAD"]
            os.dup2(keep, 2)
            os.close(keep)
        f.seek(0)
        return out, f.read().decode(errors="replace")


def measure(L, name, blob, build_s):
    b_blob, sizes = displaced(blob)
    ctx = hip.Context(0, L)
    ctx.upload_static(util.pmj())
    ctx.resize(256, 256)
    ctx.upload_scene_blob(blob)
    ctx.render(1)
    a_arr, b_arr = hip._aligned_copy(blob), hip._aligned_copy(b_blob)  # (aligned once: the copy is the wrapper's, not the library's)
    assert ctx.update_vertices_blob(b_arr) == 0 and ctx.update_vertices_blob(a_arr) == 0
    ctx.sync()
    t0 = time.perf_counter()
    assert ctx.update_vertices_blob(b_arr) == 0
    update_ms = (time.perf_counter() - t0) * 1e3
    assert ctx.update_vertices_blob(a_arr) == 0
    _, log = traced(lambda: ctx.update_vertices_blob(b_arr))
    stamps = [(float(m.group(1)), m.group(2).strip()) for m in re.finditer(r"rayhip_scene_update_vertices:\s+([0-9.]+) ms\s+(.*)", log)]
    phases, prev = {}, None
    for ms, what in stamps:
        if prev is not None:
            phases[what] = round(ms - prev, 4)
        prev = ms
    m = re.search(r"(\d+) triangles without area", log)
    ctx.render(1)
    ctx.upload_scene_blob(b_blob)
    ctx.sync()
    t0 = time.perf_counter()
    ctx.upload_scene_blob(b_blob)
    ctx.sync()
    upload_ms = (time.perf_counter() - t0) * 1e3
    out = dict(scene=name, device=ctx.device_name(), bvh_width=ctx.bvh_width(), **sizes, update_ms=round(update_ms, 3),
               update_traced_total_ms=round(stamps[-1][0] - stamps[0][0], 3) if stamps else None, phases_ms=phases,
               triangles_without_area=int(m.group(1)) if m else None, upload_ms=round(upload_ms, 2), scene_build_s=build_s,
               blob_mib=round(len(blob) / 2 ** 20, 1))
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vertex_update", "refit_bench.jsonl"))
    a = ap.parse_args()
    L = hip.Library()
    if L.device_count() <= 0:
        sys.exit("vertex_update_bench needs a GPU")
    jobs = []
    if os.path.exists(api.HIP_HOST_LIB):
        t0 = time.perf_counter()
        s = api.CreateSceneHIP()
        scenes.atrium_small(s)
        blob = api.export_scene_blob(s)
        jobs.append(("atrium_small", blob, round(time.perf_counter() - t0, 3)))
    else:
        print("the drop-in's host library is not built: no atrium_small", file=sys.stderr)
    cache_dir = os.environ.get("RAY_AMD_CACHE", os.path.join(tempfile.gettempdir(), f"ray_amd_cache_{os.getuid()}"))
    headline = os.path.join(cache_dir, "bistro_4.3.rayscene")  # bench.py: get_scene_blob
    if os.path.exists(headline):
        with open(headline, "rb") as f:
            jobs.append(("bistro (headline atrium, from bench.py's scene cache)", f.read(), None))
    lines = [json.dumps(measure(L, *job)) for job in jobs]
    for line in lines:
        print(line)
    if lines:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
