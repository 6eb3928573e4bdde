"""What a skinned frame costs on the device, three ways in one process: one JSON line per scene.

  (a) update_vertices:        rayhip_scene_update_vertices of vertices the HOST has posed already (the route there was before; the host's
                              skinning loop is not in the figure) -- 44 bytes per vertex through pageable memory, then the refit
  (b) pose_skins_<bones>:     rayhip_scene_pose_skins of ONE skin over the longest run of the vertex array that holds no vertex of a triangle
                              light, at 64 and at 1024 bones (the palette in LDS / read from memory): the palette goes up, k_skin_vertices poses
                              into the staging array, the counter comes back, one device-to-device copy, the same refit
  (c) update_vertices_device: rayhip_scene_update_vertices_device of the same vertices as (a) from a device buffer: k_check_vertices, the
                              device-to-device copy, the refit

Every path is called twice first (the first call allocates), then REPS times in turn with the others; `ms` is the wall time of an untraced
call (median, with the lowest and highest), `phases_ms` the differences of the RAYHIP_TRACE_UPLOAD stamps of one more call -- each stamp
waits for the device first, so the phases add up to more than an untraced call.  The phase "vertices posed" holds the palette copy, the
kernel and the read-back of the counter; the kernel alone is timed by running this tool under `rocprofv3 --kernel-trace --stats`.
After every timed pose the vertex array is read back and compared with the host build of skin.h (tests/hostsim/hostsim_skin.cpp): launches of
thousands of blocks, bit for bit.

Scenes: atrium_small, and the headline atrium (bench.py: bistro), from bench.py's scene cache or built into it.

usage: python tools/skin_bench.py [--scenes atrium_small,bistro] [--out profiles/skinning/skin_bench.jsonl]
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

import skin_cases as S  # noqa: E402
import util  # noqa: E402
import vertex_update_cases as V  # noqa: E402
from ray_amd import api, hip, scenes  # noqa: E402
from vertex_update_bench import traced  # noqa: E402

REPS = 7
POSE_BYTES_PER_VERTEX = 44 + 8 + 16 + 1 + 44  # rest record, indices, weights, the `used` flag in; the posed record out


def whole_mesh_skin(a, bones, seed):
    first, count = S.free_ranges(a)[0]
    rng = np.random.RandomState(seed)
    s = S.Skin.__new__(S.Skin)
    s.first, s.count, s.bones_count = first, count, bones
    s.rest = a.vertices[first:first + count].copy()
    s.indices = rng.randint(0, bones, size=(count, 4)).astype(np.uint16)
    w = rng.uniform(0.05, 1.0, size=(count, 4))
    w[rng.uniform(size=(count, 4)) < 0.4] = 0.0  # (1 to 4 influences mostly; a few vertices end up with none and keep their record)
    total = w.sum(axis=1, keepdims=True)
    s.weights = (w / np.where(total == 0, 1.0, total)).astype(np.float32)
    return s


def stamps_of(log):
    """{phase: ms} from the stamps of one traced call, whichever entry point wrote them"""
    stamps = [(float(m.group(1)), m.group(2).strip()) for m in re.finditer(r"rayhip_scene_\w+:\s+([0-9.]+) ms\s+(.*)", log)]
    phases, prev = {}, None
    for ms, what in stamps:
        if prev is not None:
            phases[what] = round(ms - prev, 4)
        prev = ms
    return phases, (round(stamps[-1][0] - stamps[0][0], 3) if stamps else None)


def measure(L, name, blob):
    a = V.Arrays(blob)
    ext = S.extent(a)
    ctx = hip.Context(0, L)
    ctx.upload_static(util.pmj())
    ctx.resize(256, 256)
    ctx.upload_scene_blob(blob)
    ctx.render(1)
    skins = {bones: whole_mesh_skin(a, bones, 5) for bones in (64, 1024)}
    palettes = {bones: [S.palette(bones, 10 + k, ext * np.float32(0.4)) for k in range(2)] for bones in skins}  # (translations within 2 % of the extent)
    posed = {bones: [S.host_posed(a, [skins[bones]], [m]) for m in palettes[bones]] for bones in skins}
    host_vertices = posed[64]  # what (a) and (c) send
    on_device = [torch.from_numpy(v.view(np.uint8).copy()).cuda() for v in host_vertices]
    torch.cuda.synchronize()
    ids = {}

    def run_a(k):
        assert ctx.update_vertices(0, host_vertices[k]) == 0

    def run_c(k):
        assert ctx.update_vertices_device(0, len(a.vertices), on_device[k].data_ptr()) == 0

    def pose(bones):
        def run(k):
            assert ctx.pose_skins({ids[bones]: palettes[bones][k]}) == 0
        return run

    paths = {"update_vertices": run_a, "update_vertices_device": run_c}
    # one skin is live at a time: both drive the same range
    order = ["update_vertices", "pose_skins_64", "pose_skins_1024", "update_vertices_device"]
    times = {p: [] for p in order}
    phases, traced_total, equal = {}, {}, {}

    def with_skin(bones, fn):
        ids[bones] = ctx.create_skin(skins[bones].first, skins[bones].rest, skins[bones].indices, skins[bones].weights, bones)
        assert ids[bones] != 2
        try:
            return fn()
        finally:
            assert ctx.destroy_skin(ids[bones]) == 0

    def timed(run, k):
        ctx.sync()
        t0 = time.perf_counter()
        run(k)
        return (time.perf_counter() - t0) * 1e3

    def one_round(r, record):
        for p in order:
            bones = int(p.rsplit("_", 1)[1]) if p.startswith("pose_skins") else None
            run = pose(bones) if bones else paths[p]

            def go():
                ms = timed(run, r & 1)
                if bones:
                    equal[p] = equal.get(p, True) and bool(np.array_equal(S.bits(ctx.read_accel(4)), S.bits(posed[bones][r & 1])))
                return ms
            ms = with_skin(bones, go) if bones else go()
            if record:
                times[p].append(ms)

    for r in range(2):
        one_round(r, False)
    for r in range(REPS):
        one_round(r, True)
    for p in order:
        bones = int(p.rsplit("_", 1)[1]) if p.startswith("pose_skins") else None
        run = pose(bones) if bones else paths[p]
        _, log = with_skin(bones, lambda: traced(lambda: run(0))) if bones else traced(lambda: run(0))
        phases[p], traced_total[p] = stamps_of(log)
    ctx.render(1)
    ctx.sync()
    out = dict(scene=name, device=ctx.device_name(), bvh_width=ctx.bvh_width(), vertices=int(len(a.vertices)), skin_vertices=int(skins[64].count),
               entries=int(len(a.tri_indices)), light_vertices=len(a.light_vertices()), reps=REPS,
               pose_kernel_bytes=int(skins[64].count) * POSE_BYTES_PER_VERTEX,
               paths={p: dict(ms=round(float(np.median(times[p])), 3), ms_min=round(min(times[p]), 3), ms_max=round(max(times[p]), 3),
                              traced_total_ms=traced_total[p], phases_ms=phases[p]) for p in order},
               posed_vertices_equal_host_build=equal)
    ctx.close()
    return out


def scene_blobs(names):
    for name in names:
        if name == "atrium_small":
            if not os.path.exists(api.HIP_HOST_LIB):
                print("the drop-in's host library is not built: no atrium_small", file=sys.stderr)
                continue
            s = api.CreateSceneHIP()
            scenes.atrium_small(s)
            yield name, api.export_scene_blob(s)
        else:
            import bench
            blob, _ = bench.get_scene_blob(name, bench.WORKLOADS[name], 0, 1, lambda: None, bench.reference_scene_library())
            yield f"{name} (headline atrium, bench.py's scene)", blob


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="atrium_small,bistro")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "skinning", "skin_bench.jsonl"))
    a = ap.parse_args()
    L = hip.Library()
    if L.device_count() <= 0:
        sys.exit("skin_bench needs a GPU")
    assert S.have_skin_lib(), "tests/hostsim/hostsim_skin.cpp is not built (run __graft_entry__.build())"
    lines = [json.dumps(measure(L, name, blob)) for name, blob in scene_blobs(a.scenes.split(","))]
    for line in lines:
        print(line)
    if lines:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
