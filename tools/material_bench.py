"""What changing materials costs on the device (rayhip_scene_set_materials), against the only route there was: one JSON line,
everything in one process.

Two scenes:
  material_field(130)  tests/material_cases.py: a Cornell room and 130 small quads with a material each, every fifth an importance-sampled
                       emitter (52 triangle lights)
  emissive sheet       the scene of tools/light_refit_bench.py (a sheet of quads x quads emissive quads: 2 quads^2 triangle lights, all
                       coloured by ONE material, `glow`, which is given another colour and strength)
and per scene up to four paths:
  set_materials_plain  rayhip_scene_set_materials of ONE material that colours no light: slot and record go up, k_check_materials, the
                       counters come back, k_commit_materials
  set_materials_glow   the same of ONE emitter: behind the commit k_recolour_tri_lights, the pass over every triangle light
                       (k_refit_tri_lights) and one k_refit_light_level launch per height of the light tree
  set_materials_all    every material of material_field (133 entries, 26 emitters)
  upload_blob          rayhip_scene_upload_blob of the same scene in a second context: what a caller of the C ABI had to do (the host's
                       scene build is not in the figure)
Every path is called twice first (the first call allocates), then REPS times in turn with the others, alternating between two sets of
records; `ms` is the wall time of an untraced call between two synchronisations (median, with the lowest and highest), `phases_ms` the
differences of the RAYHIP_TRACE_UPLOAD stamps of one more call -- each stamp waits for the device first.  On material_field the arrays
are compared with the host build afterwards (tests/hostsim/hostsim_materials.cpp).

usage: python tools/material_bench.py [--quads 256] [--out profiles/materials/material_bench.jsonl]
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

import light_refit_cases as LR  # noqa: E402
import material_cases as M  # noqa: E402
from instance_pose_bench import stamps_of  # noqa: E402
from light_pose_bench import context  # noqa: E402
from light_refit_bench import sheet_scene  # noqa: E402
from ray_amd import api, hip  # noqa: E402
from vertex_update_bench import traced  # noqa: E402

REPS = 9


def measure(L, name, blob, calls, check):
    """`calls`: {path: (slots, [records, records])} -- two sets of records per path"""
    a = M.Arrays(blob)
    ctx, ctx_up = context(L, blob, True), context(L, blob, False)

    def setter(slots, records):
        def run(k):
            assert ctx.set_materials(slots, records[k]) == 0
        return run

    paths = {p: (ctx, setter(s, r)) for p, (s, r) in calls.items()}
    paths["upload_blob"] = (ctx_up, lambda k: ctx_up.upload_scene_blob(blob))
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
    for p in calls:
        _, log = traced(lambda: paths[p][1](0))
        phases[p], traced_total[p] = stamps_of(log)
    equal = None
    if check:
        state = M.State(a)
        for p, (s, r) in calls.items():  # (the order of the traced calls above: each left its first set of records)
            rc, _, state = M.host_set_materials(state, s, r[0])
            assert rc == 0
        equal = bool(np.array_equal(M.words(ctx.read_accel(11)), M.words(state.materials)) and np.array_equal(ctx.read_accel(9), state.lights) and
                     np.array_equal(LR.bits(ctx.read_accel(10)).ravel(), LR.bits(state.leaf).ravel()) and
                     np.array_equal(LR.bits(ctx.read_accel(5)), LR.bits(state.cwnodes)) and np.array_equal(LR.bits(ctx.read_accel(6)), LR.bits(state.children)))
    ctx.render(1)
    ctx.sync()
    _, level_offset = LR.levels(a.cwnodes, len(a.lights))
    out = dict(scene=name, materials=int(a.used_materials().sum()), triangle_lights=int(len(a.tri_lights())), light_nodes=int(len(a.cwnodes)),
               tree_heights=int(len(level_offset) - 1), blob_bytes=len(blob), reps=REPS, named={p: int(len(s)) for p, (s, _) in calls.items()},
               paths={p: dict(ms=round(float(np.median(times[p])), 3), ms_min=round(min(times[p]), 3), ms_max=round(max(times[p]), 3),
                              traced_total_ms=traced_total.get(p), phases_ms=phases.get(p)) for p in paths},
               arrays_equal_host_build=equal)
    ctx.close(), ctx_up.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quads", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "materials", "material_bench.jsonl"))
    args = ap.parse_args()
    L = hip.Library()
    if L.device_count() <= 0:
        sys.exit("material_bench needs a GPU")
    assert os.path.exists(M.MATERIALS_LIB), "tests/hostsim/hostsim_materials.cpp is not built (run __graft_entry__.build())"
    if not os.path.exists(api.HIP_HOST_LIB):
        sys.exit("the drop-in's host library is not built: no scenes")
    results = []
    blob = M.blob("material_field", 0)
    a, moved = M.Arrays(blob), M.Arrays(M.blob("material_field", 1))
    every = M.changed_slots(a, moved)
    plain, glow = np.array([4], dtype=np.uint32), np.array([3], dtype=np.uint32)  # (the first two quads: an emitter, a Diffuse material)
    two = lambda s: (s, [moved.materials[s], a.materials[s]])  # noqa: E731
    results.append(measure(L, "material_field(130)", blob, dict(set_materials_plain=two(plain), set_materials_glow=two(glow), set_materials_all=two(every)), True))
    blob, _ = sheet_scene(args.quads)
    a = M.Arrays(blob)
    glow = np.array([4], dtype=np.uint32)  # (after the room's four)
    assert a.materials["type"][4] == 3 and M.State(a).flags[4] & M.SLOT_EMITTER
    renamed = a.materials[glow].copy()
    renamed["base_color"], renamed["tangent_rotation_or_strength"] = (0.4, 0.8, 0.9), 1.25
    grey = np.array([0], dtype=np.uint32)
    regrey = a.materials[grey].copy()
    regrey["base_color"] = (0.6, 0.55, 0.4)
    results.append(measure(L, f"emissive sheet of {args.quads} x {args.quads} quads", blob,
                           dict(set_materials_plain=(grey, [regrey, a.materials[grey]]), set_materials_glow=(glow, [renamed, a.materials[glow]])), False))
    dev = hip.Context(0, L)
    line = json.dumps(dict(device=dev.device_name(), scenes=results))
    dev.close()
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
