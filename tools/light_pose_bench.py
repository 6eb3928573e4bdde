"""What moving and recolouring analytic lights costs on the device (rayhip_scene_set_lights), against the only route there was: one
JSON line, everything in one process.

Two scenes:
  light_field(130)   tests/light_pose_cases.py: a Cornell room with 130 small sphere / rect / disk / line lights and a directional one; a
                     light tree of four heights
  emissive sheet     the scene of tools/light_refit_bench.py (a sheet of quads x quads emissive quads: 2 quads^2 triangle lights, a
                     tree of seven heights at 256) with four analytic lights added
and per scene three paths:
  set_lights_one     rayhip_scene_set_lights of ONE light: slot and record go up, k_pose_lights, the counters come back,
                     k_commit_lights, one k_refit_light_level launch per height
  set_lights_all     the same over every analytic light the scene build placed (but the directional one)
  upload_blob        rayhip_scene_upload_blob of the same scene in a second context: what a caller of the C ABI had to do (the host's
                     scene build is not in the figure)
Every path is called twice first (the first call allocates, and runs the one pass over the triangle lights the leaf table needs),
then REPS times in turn with the others, alternating between two sets of records; `ms` is the wall time of an untraced call between
two synchronisations (median, with the lowest and highest), `phases_ms` the differences of the RAYHIP_TRACE_UPLOAD stamps of one more
call -- each stamp waits for the device first.  On light_field the arrays are compared with the host build afterwards
(tests/hostsim/hostsim_light_pose.cpp).

usage: python tools/light_pose_bench.py [--quads 256] [--out profiles/light_pose/light_pose_bench.jsonl]
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
import torch  # noqa: E402,F401  (before librayhip is loaded: torch brings its own HIP runtime, and it must be the one that opens the device)

import light_pose_cases as P  # noqa: E402
import light_refit_cases as LR  # noqa: E402
import util  # noqa: E402
import vertex_update_cases as V  # noqa: E402
from instance_pose_bench import stamps_of  # noqa: E402
from ray_amd import api, hip, scenes  # noqa: E402
from ray_amd.api import ShadingNode, eShadingNode  # noqa: E402
from vertex_update_bench import traced  # noqa: E402

REPS = 9
SHEET_LIGHTS = [  # (kind, keywords at pose 0, keywords at pose 1)
    ("sphere", dict(color=(3.0, 2.5, 2.0), position=(-0.12, 0.42, -0.12), radius=0.02), dict(color=(2.0, 3.5, 3.0), position=(-0.20, 0.36, -0.18), radius=0.03)),
    ("rect", dict(color=(4.0, 4.0, 3.5), width=0.12, height=0.08, xform=scenes._translate(-0.30, 0.52, -0.44)),
     dict(color=(5.0, 3.0, 4.5), width=0.10, height=0.12, xform=scenes._translate(-0.26, 0.50, -0.40, rot_x_deg=15.0, rot_z_deg=10.0))),
    ("disk", dict(color=(2.0, 4.0, 2.5), width=0.09, height=0.12, xform=scenes._translate(-0.50, 0.30, -0.30, rot_z_deg=-90.0)),
     dict(color=(3.0, 3.0, 3.5), width=0.12, height=0.08, xform=scenes._translate(-0.48, 0.26, -0.24, rot_x_deg=10.0, rot_z_deg=-80.0))),
    ("line", dict(color=(4.0, 2.0, 2.0), radius=0.006, height=0.25, xform=scenes._translate(-0.06, 0.35, -0.30, rot_x_deg=90.0)),
     dict(color=(3.0, 3.0, 4.0), radius=0.009, height=0.20, xform=scenes._translate(-0.08, 0.30, -0.26, rot_x_deg=70.0, rot_z_deg=25.0))),
]


def sheet_scene(quads):
    """tools/light_refit_bench.py: sheet_scene, plus SHEET_LIGHTS at pose 0"""
    s = api.CreateSceneHIP()
    s.SetEnvironment(env_col=(0.0, 0.0, 0.0))
    V._room(s)
    glow = s.AddMaterial(ShadingNode(type=eShadingNode.Emissive, strength=2.0, base_color=(0.9, 0.7, 0.4), importance_sample=True))
    b = scenes._MeshBuilder()
    b.add(*V._sheet_mesh(quads, 0.0, -0.2, 0.2, -0.2, 0.2, 0.0, 0.03, seed=31), glow)
    attrs, idx, groups = b.finish()
    s.AddMeshInstance(s.AddMesh(attrs, idx, groups, **V._SHEET_LAYOUT), scenes._xform(translate=(-0.28, 0.25, -0.28), rot_y_deg=20.0, scale=(1.1, 0.8, 0.9)))
    for kind, kw, _ in SHEET_LIGHTS:
        s.AddLight(kind, **kw)
    scenes._cornell_camera(s)
    s.Finalize()
    return api.export_scene_blob(s)


def context(L, blob, refit):
    ctx = hip.Context(0, L)
    ctx.upload_static(util.pmj())
    ctx.resize(256, 256)
    ctx.refit_lights(refit)
    ctx.upload_scene_blob(blob)
    ctx.render(1)
    ctx.sync()
    return ctx


def measure(L, name, blob, slots, records, check):
    """`records`: two sets for `slots`"""
    a = LR.Arrays(blob)
    ctx, ctx_up = context(L, blob, True), context(L, blob, False)

    def run_one(k):
        assert ctx.set_lights(slots[:1], records[k][:1]) == 0

    def run_all(k):
        assert ctx.set_lights(slots, records[k]) == 0

    def run_upload(k):
        ctx_up.upload_scene_blob(blob)

    paths = {"set_lights_one": (ctx, run_one), "set_lights_all": (ctx, run_all), "upload_blob": (ctx_up, run_upload)}
    times = {p: [] for p in paths}
    for r in range(2 + REPS):
        for p, (c, run) in paths.items():
            c.sync()
            t0 = time.perf_counter()
            run(r & 1)
            c.sync()
            if r >= 2:
                times[p].append((time.perf_counter() - t0) * 1e3)
    phases, traced_total = {}, {}
    for p in ("set_lights_one", "set_lights_all"):
        _, log = traced(lambda: paths[p][1](0))
        phases[p], traced_total[p] = stamps_of(log)
    equal = None
    if check:
        rc, _, want = P.host_set_lights(P.State(a), slots, records[0])
        equal = bool(rc == 0 and np.array_equal(ctx.read_accel(9), want.lights) and np.array_equal(LR.bits(ctx.read_accel(10)).ravel(), LR.bits(want.leaf).ravel()) and
                     np.array_equal(LR.bits(ctx.read_accel(5)), LR.bits(want.cwnodes)) and np.array_equal(LR.bits(ctx.read_accel(6)), LR.bits(want.children)))
    ctx.render(1)
    ctx.sync()
    _, level_offset = LR.levels(a.cwnodes, len(a.lights))
    out = dict(scene=name, lights=int(len(a.li_indices)), triangle_lights=int(len(a.tri_lights())), named_by_all=int(len(slots)), light_nodes=int(len(a.cwnodes)),
               tree_heights=int(len(level_offset) - 1), blob_bytes=len(blob), reps=REPS,
               paths={p: dict(ms=round(float(np.median(times[p])), 3), ms_min=round(min(times[p]), 3), ms_max=round(max(times[p]), 3),
                              traced_total_ms=traced_total.get(p), phases_ms=phases.get(p)) for p in paths},
               arrays_equal_host_build=equal)
    ctx.close(), ctx_up.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quads", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "light_pose", "light_pose_bench.jsonl"))
    args = ap.parse_args()
    L = hip.Library()
    if L.device_count() <= 0:
        sys.exit("light_pose_bench needs a GPU")
    assert os.path.exists(P.POSE_LIB), "tests/hostsim/hostsim_light_pose.cpp is not built (run __graft_entry__.build())"
    if not os.path.exists(api.HIP_HOST_LIB):
        sys.exit("the drop-in's host library is not built: no scenes")
    results = []
    blob = P.field_blob(130)
    a = LR.Arrays(blob)
    slots, rest = P.field_records(a, 130, phase=0)
    _, moved = P.field_records(a, 130, phase=1)
    results.append(measure(L, "light_field(130)", blob, slots, [moved, rest], True))
    blob = sheet_scene(args.quads)
    a = LR.Arrays(blob)
    slots = np.array(P.analytic_slots(a), dtype=np.uint32)
    assert len(slots) == len(SHEET_LIGHTS)
    records = [np.array([P.pack(kind, a.lights[s, 0], **kws[k]) for s, (kind, *kws) in zip(slots, SHEET_LIGHTS)], dtype=np.uint32) for k in (1, 0)]
    assert np.array_equal(records[1], a.lights[slots])  # (the packers make the records the scene build made)
    results.append(measure(L, f"emissive sheet of {args.quads} x {args.quads} quads + {len(slots)} analytic lights", blob, slots, records, False))
    dev = hip.Context(0, L)
    line = json.dumps(dict(device=dev.device_name(), scenes=results))
    dev.close()
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
