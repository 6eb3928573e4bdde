"""What the light refit costs (rayhip_scene_refit_lights): one JSON line for a generated scene whose emitter is a sheet of 256 x 256
quads -- 131 072 triangle lights, a light tree of some 40 k nodes -- in one process:

  (a) refit_on:     rayhip_scene_update_vertices_device with the switch ON, the emitter moving between two poses
  (b) refit_off:    the same call on the same scene with the switch OFF and the emitter left still (its vertices arrive bytewise equal,
                    which the call accepts): the geometry refit alone
  (c) full_upload:  rayhip_scene_upload_blob of the same scene: the only way to move an emitter without the switch -- and that is without
                    the host scene build in front of it, whose time is reported as scene_build_s

(a) - (b) is the light refit.  Every path is called twice first (the first call allocates), then REPS times in turn with the others; `ms`
is the host clock around a call that returns when the device is done (median, lowest, highest).  `phases_ms` are the differences of the
RAYHIP_TRACE_UPLOAD stamps of one more call of (a) -- each stamp waits for the device first, so they add up to more than an untraced
call; "light corners" is k_refit_tri_lights, "light tree refitted" the level launches of k_refit_light_level.  `level_bytes` is what those
launches move, counted from the tree: per node the node read and written (2 x 208), its 24 importance rows written (384), its summary
written (48), its eight slot scales (32) and its index read (4); per non-empty slot the child's summary read (48).  After the last timed (a) the three light arrays
are read back and compared with the host build (tests/hostsim/hostsim_lights.cpp), bit for bit.

usage: python tools/light_refit_bench.py [--quads 256] [--out profiles/light_refit/light_refit_bench.jsonl]
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
import torch  # noqa: E402  (before librayhip is loaded: torch brings its own HIP runtime, and it must be the one that opens the device)

import light_refit_cases as LR  # noqa: E402
import util  # noqa: E402
import vertex_update_cases as V  # noqa: E402
from ray_amd import api, hip, scenes  # noqa: E402
from ray_amd.api import ShadingNode, eShadingNode  # noqa: E402
from skin_bench import stamps_of  # noqa: E402
from vertex_update_bench import traced  # noqa: E402

REPS = 7


def sheet_scene(quads):
    """(blob, seconds of the host scene build): the room of the vertex-update cases and one emissive sheet of quads x quads quads"""
    t0 = time.perf_counter()
    s = api.CreateSceneHIP()
    s.SetEnvironment(env_col=(0.0, 0.0, 0.0))
    V._room(s)
    glow = s.AddMaterial(ShadingNode(type=eShadingNode.Emissive, strength=2.0, base_color=(0.9, 0.7, 0.4), importance_sample=True))
    b = scenes._MeshBuilder()
    b.add(*V._sheet_mesh(quads, 0.0, -0.2, 0.2, -0.2, 0.2, 0.0, 0.03, seed=31), glow)
    attrs, idx, groups = b.finish()
    s.AddMeshInstance(s.AddMesh(attrs, idx, groups, **V._SHEET_LAYOUT), scenes._xform(translate=(-0.28, 0.25, -0.28), rot_y_deg=20.0, scale=(1.1, 0.8, 0.9)))
    scenes._cornell_camera(s)
    s.Finalize()
    blob = api.export_scene_blob(s)
    return blob, time.perf_counter() - t0


def measure(L, blob, build_s):
    a = LR.Arrays(blob)
    lv = np.array(a.light_vertices())
    poses = [a.vertices.copy(), a.vertices.copy()]
    poses[1]["p"][lv, 1] += (0.01 * np.sin(40.0 * poses[1]["p"][lv, 0])).astype(np.float32)  # the emitter waves; everything else stays
    on_device = [torch.from_numpy(v.view(np.uint8).copy()).cuda() for v in poses]
    torch.cuda.synchronize()

    def context(on):
        ctx = hip.Context(0, L)
        ctx.upload_static(util.pmj())
        ctx.resize(256, 256)
        ctx.refit_lights(on)
        ctx.upload_scene_blob(blob)
        ctx.render(1)
        ctx.sync()
        return ctx

    ctx_on, ctx_off, ctx_up = context(True), context(False), context(False)
    old = {k: ctx_on.read_accel(k).copy() for k in (5, 6, 7)}

    def run_on(k):
        assert ctx_on.update_vertices_device(0, len(a.vertices), on_device[k].data_ptr()) == 0

    def run_off(k):
        assert ctx_off.update_vertices_device(0, len(a.vertices), on_device[0].data_ptr()) == 0

    def run_upload(k):
        ctx_up.upload_scene_blob(blob)

    paths = {"refit_on": (ctx_on, run_on), "refit_off": (ctx_off, run_off), "full_upload": (ctx_up, run_upload)}
    times = {p: [] for p in paths}
    for r in range(2 + REPS):
        for p, (ctx, run) in paths.items():
            ctx.sync()
            t0 = time.perf_counter()
            run((r + 1) & 1)
            ctx.sync()
            if r >= 2:
                times[p].append((time.perf_counter() - t0) * 1e3)
    last = (2 + REPS) & 1
    got = {k: ctx_on.read_accel(k) for k in (5, 6, 7)}
    want = LR.host_refit(a, poses[last], cwnodes=old[5], children=old[6], tri_geom=old[7])
    equal = bool(np.array_equal(LR.bits(got[5]), LR.bits(want.cwnodes)) and np.array_equal(LR.bits(got[6]), LR.bits(want.children)) and
                 np.array_equal(LR.bits(got[7]), LR.bits(want.tri_geom)))
    _, log = traced(lambda: run_on(0))
    phases, traced_total = stamps_of(log)
    _, level_offset = LR.levels(a.cwnodes, len(a.lights))
    nodes, slots = len(a.cwnodes), int((a.cwnodes["child"] != LR.EMPTY).sum())
    level_bytes = nodes * (2 * 208 + 384 + 48 + 32 + 4) + slots * 48
    med = {p: float(np.median(t)) for p, t in times.items()}
    tree_ms = phases.get("light tree refitted")
    out = dict(scene=f"emissive sheet of {int(round((len(a.tri_lights()) // 2) ** 0.5))} x {int(round((len(a.tri_lights()) // 2) ** 0.5))} quads", device=ctx_on.device_name(),
               triangle_lights=int(len(a.tri_lights())), light_tree_nodes=nodes, nodes_per_height=[int(x) for x in np.diff(level_offset)],
               vertices=int(len(a.vertices)), entries=int(len(a.tri_indices)), reps=REPS, scene_build_s=round(build_s, 2),
               paths={p: dict(ms=round(med[p], 3), ms_min=round(min(times[p]), 3), ms_max=round(max(times[p]), 3)) for p in paths},
               light_refit_ms=round(med["refit_on"] - med["refit_off"], 3), traced_total_ms=traced_total, phases_ms=phases,
               level_bytes=level_bytes, level_gb_per_s=None if not tree_ms else round(level_bytes / (tree_ms * 1e-3) / 1e9, 2),
               triangle_lights_without_area=int(want.degenerate), light_arrays_equal_host_build=equal)
    for ctx in (ctx_on, ctx_off, ctx_up):
        ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quads", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "light_refit", "light_refit_bench.jsonl"))
    args = ap.parse_args()
    L = hip.Library()
    if L.device_count() <= 0:
        sys.exit("light_refit_bench needs a GPU")
    assert LR.have_lights_lib(), "tests/hostsim/hostsim_lights.cpp is not built (run __graft_entry__.build())"
    if not os.path.exists(api.HIP_HOST_LIB):
        sys.exit("the drop-in's host library is not built: no scene")
    blob, build_s = sheet_scene(args.quads)
    line = json.dumps(measure(L, blob, build_s))
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
