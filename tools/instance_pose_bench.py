"""What moving the instances of a scene costs on the device, the ways there are, in one process: one JSON line.

  (a) update_instances:               rayhip_scene_update_instances of a serialised scene the HOST has moved, finalised and exported already
                                      (the only route there was; the host's work -- inverses, its top level, its light tree, the export --
                                      is not in the figure): the instance array, lights, light tree, environment quadtree and sky go up,
                                      the top level is rebuilt on the device
  (b) set_instance_transforms:        rayhip_scene_set_instance_transforms of the moved slots that carry no triangle lights: slots and
                                      matrices go up, k_pose_instances, the counters come back, k_commit_instances, k_instance_boxes,
                                      records and boxes come back, the same top-level build
  (c) set_instance_transforms_device: the same from a device buffer
  (d) set_instance_transforms_lights: (b) over EVERY moved slot, the lamps too, in a second context with rayhip_scene_refit_lights on: the
                                      triangle lights are re-placed and the light tree refitted behind the commit

The scene is instance_field(1000) (ray_amd/scenes.py: 1001 slots, 16 of them lamps with 12 triangle lights each) at its two poses.  Every
path is called twice first (the first call allocates), then REPS times in turn with the others, alternating between the poses; `ms` is the
wall time of an untraced call between two synchronisations (median, with the lowest and highest), `phases_ms` the differences of the
RAYHIP_TRACE_UPLOAD stamps of one more call -- each stamp waits for the device first.  After the timed calls of (b), (c) and (d) the instance
array and the leaves of the top level are read back and compared with the host build of instances.h (tests/hostsim/hostsim_instances.cpp).

usage: python tools/instance_pose_bench.py [--count 1000] [--out profiles/instance_pose/instance_pose_bench.jsonl]
"""
import argparse
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before librayhip is loaded: torch brings its own HIP runtime, and it must be the one that opens the device)

import instance_pose_cases as IP  # noqa: E402
import util  # noqa: E402
import vertex_update_cases as V  # noqa: E402
from ray_amd import api, hip, scenes  # noqa: E402
from vertex_update_bench import traced  # noqa: E402

REPS = 9


def stamps_of(log):
    """{phase: ms} from the stamps of one traced call, whichever entry point wrote them"""
    stamps = [(float(m.group(1)), m.group(2).strip()) for m in re.finditer(r"rayhip_scene_\w+:\s+([0-9.]+) ms\s+(.*)", log)]
    phases, prev = {}, None
    for ms, what in stamps:
        if prev is not None:
            phases[what] = round(ms - prev, 4)
        prev = ms
    return phases, (round(stamps[-1][0] - stamps[0][0], 3) if stamps else None)


def context(L, blob, refit):
    ctx = hip.Context(0, L)
    ctx.upload_static(util.pmj())
    ctx.resize(256, 256)
    if refit:
        ctx.refit_lights(True)
    ctx.upload_scene_blob(blob)
    ctx.render(1)
    return ctx


def measure(L, count):
    s = api.CreateSceneHIP()
    scenes.instance_field(s, count)
    blobs = [api.export_scene_blob(s)]
    scenes.move_instance_field(s)
    blobs.append(api.export_scene_blob(s))
    arrays = [V.Arrays(b) for b in blobs]
    a = arrays[0]
    live = a.live_instances()
    moved = [m for m in live if arrays[0].mesh_instances["xform"][m].tobytes() != arrays[1].mesh_instances["xform"][m].tobytes()]
    flags, lamps = IP.slot_flags(a), set(IP.light_slots(a))
    free = np.array([m for m in moved if m not in lamps], dtype=np.uint32)
    every = np.array(moved, dtype=np.uint32)
    x_free = [np.ascontiguousarray(arr.mesh_instances["xform"][free]) for arr in arrays]
    x_every = [np.ascontiguousarray(arr.mesh_instances["xform"][every]) for arr in arrays]
    d_free = torch.from_numpy(free.view(np.uint8).copy()).cuda()
    d_x_free = [torch.from_numpy(x.view(np.uint8).ravel().copy()).cuda() for x in x_free]
    torch.cuda.synchronize()
    ctx, lit = context(L, blobs[0], False), context(L, blobs[0], True)
    aligned = [hip._aligned_copy(b) for b in blobs]  # (what update_instances copies per call otherwise: the wrapper's work, not the library's)

    def run_a(k):
        cam = hip.Camera()
        rc = L.fn("scene_update_instances_blob")(ctx._ctx, aligned[k].ctypes.data, aligned[k].size, hip.C.byref(cam))
        assert rc == 0, rc

    def run_b(k):
        assert ctx.set_instance_transforms(free, x_free[k]) == 0

    def run_c(k):
        assert ctx.set_instance_transforms_device(len(free), d_free.data_ptr(), d_x_free[k].data_ptr()) == 0

    def run_d(k):
        assert lit.set_instance_transforms(every, x_every[k]) == 0

    paths = {"update_instances": (ctx, run_a), "set_instance_transforms": (ctx, run_b), "set_instance_transforms_device": (ctx, run_c),
             "set_instance_transforms_lights": (lit, run_d)}
    times = {p: [] for p in paths}
    equal = {}

    def holds(c, slots, x, pin):
        """the device's records and leaves after a call against the host build over what it held before"""
        before, nodes = c.read_accel(8).copy(), c.read_accel(0).copy()

        def check():
            rc, mi, _ = IP.host_pose(before, flags, slots, x, pin)
            return rc == 0 and c.read_accel(8).tobytes() == mi.tobytes() and bool(np.array_equal(c.read_accel(3), IP.leaves_of(a, mi, nodes=nodes)))
        return check

    def timed(c, run, k):
        c.sync()
        t0 = time.perf_counter()
        run(k)
        c.sync()
        return (time.perf_counter() - t0) * 1e3

    for r in range(2 + REPS):
        for p, (c, run) in paths.items():
            check = None
            if p != "update_instances":
                check = holds(c, every if c is lit else free, (x_every if c is lit else x_free)[r & 1], c is not lit)
            ms = timed(c, run, r & 1)
            if check:
                equal[p] = equal.get(p, True) and check()
            if r >= 2:
                times[p].append(ms)
    phases, traced_total = {}, {}
    for p, (c, run) in paths.items():
        _, log = traced(lambda: run(0))
        phases[p], traced_total[p] = stamps_of(log)
    for c in (ctx, lit):
        c.render(1)
        c.sync()
    out = dict(scene=f"instance_field({count})", device=ctx.device_name(), bvh_width=ctx.bvh_width(), slots=int(len(a.mesh_instances)), live=len(live),
               moved=len(moved), moved_without_lights=int(len(free)), lamps=len(lamps), blob_bytes=len(blobs[0]), reps=REPS,
               paths={p: dict(ms=round(float(np.median(times[p])), 3), ms_min=round(min(times[p]), 3), ms_max=round(max(times[p]), 3),
                              traced_total_ms=traced_total[p], phases_ms=phases[p]) for p in paths},
               arrays_equal_host_build=equal)
    ctx.close(), lit.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "instance_pose", "instance_pose_bench.jsonl"))
    args = ap.parse_args()
    L = hip.Library()
    if L.device_count() <= 0:
        sys.exit("instance_pose_bench needs a GPU")
    assert os.path.exists(IP.INSTANCES_LIB), "tests/hostsim/hostsim_instances.cpp is not built (run __graft_entry__.build())"
    if not os.path.exists(api.HIP_HOST_LIB):
        sys.exit("the drop-in's host library is not built: no instance_field")
    line = json.dumps(measure(L, args.count))
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
