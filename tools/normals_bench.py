"""What a live normal set adds to a vertex update and to a pose: one JSON line per scene.

One set, normals and bitangents (RAYHIP_NORMALS_N | _B, no weld), over the longest run of the vertex array that holds no vertex of a
triangle light -- the run tools/skin_bench.py and tools/morph_bench.py use.  Two paths, each WITHOUT and WITH the set, called in turn in one
process:

  update_device:  rayhip_scene_update_vertices_device of the whole vertex array with seeded displaced positions (a tensor on the device)
  pose_skins:     rayhip_scene_pose_skins of ONE skin of 64 bones over the same run

Every variant is called twice first (the first call allocates), then REPS times alternating with the others -- the set is created and
destroyed in every round, and the call that follows either is not timed (see one_round); `ms` is the wall time of an
untraced call between two device synchronisations (median, with the lowest and highest), `phases_ms` the differences of the
RAYHIP_TRACE_UPLOAD stamps of one more call -- "normals recomputed" is the two kernels together, each stamp waits for the device first.
The kernels alone are timed by running this tool under `rocprofv3 --kernel-trace --stats`.  `kernel_bytes` comes from the shapes, twice:
`requested` is what the lanes ask for (a corner vertex is gathered by every face that uses it, a face record by each of its corners),
`unique` counts every gathered record once -- what has to come from HBM when the repeats hit a cache.  In the warm-up rounds and the traced
round -- not in the timed ones, which are followed by no readback -- the vertex array is read back after every call with the set and
compared with the host build of normals.h (tests/hostsim/hostsim_normals.cpp): launches of thousands of blocks, bit for bit.

Scenes: atrium_small, and the headline atrium (bench.py: bistro), from bench.py's scene cache or built into it.

usage: python tools/normals_bench.py [--scenes atrium_small,bistro] [--reps 7] [--out profiles/normals/normals_bench.jsonl]
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

import normals_cases as NC  # noqa: E402
import skin_cases as S  # noqa: E402
import util  # noqa: E402
import vertex_update_cases as V  # noqa: E402
from ray_amd import hip  # noqa: E402
from skin_bench import scene_blobs, stamps_of, whole_mesh_skin  # noqa: E402
from vertex_update_bench import traced  # noqa: E402

BONES = 64
FACE_BYTES = 4 + 12 + 32   # k_face_frames per face: its number and three indices in, the face record out ...
CORNER_BYTES = 20          # ... and per gathered corner the position and the uv (requested), or per distinct corner vertex its 44-byte record (unique)
VERTEX_BYTES = 8 + 12 + 24  # k_vertex_frames per vertex: two row offsets and the arriving normal in; normal and bitangent out ...
ENTRY_BYTES = 4            # ... per row entry the entry itself (through LDS) ...
FRAME_BYTES = 32           # ... and the face record: per entry (requested), or per face (unique); both halves with N | B


def measure(L, name, blob, reps):
    a = V.Arrays(blob)
    ext = S.extent(a)
    ctx = hip.Context(0, L)
    ctx.upload_static(util.pmj())
    ctx.resize(256, 256)
    ctx.upload_scene_blob(blob)
    ctx.render(1)
    first, count = S.free_ranges(a)[0]
    skin = whole_mesh_skin(a, BONES, 5)
    assert (skin.first, skin.count) == (first, count)
    tris = NC.reachable(a)
    rc, tables = NC.host_rows(a, tris, first, count)
    assert rc == 0
    lengths = np.diff(tables["row"].astype(np.int64))
    moved = [V.perturbed_vertices(a, seed=7 + k, fraction=0.002) for k in range(2)]
    on_device = [torch.from_numpy(v.view(np.uint8).copy()).cuda() for v in moved]
    torch.cuda.synchronize()
    palettes = [S.palette(BONES, 10 + k, ext * np.float32(0.4)) for k in range(2)]
    posed = [S.host_posed(a, [skin], [m], vertices=v) for m, v in zip(palettes, moved)]  # (pose k follows update k: the other runs hold its positions)
    ids = {}
    run = {"update_device": lambda k: ctx.update_vertices_device(0, len(a.vertices), on_device[k].data_ptr()),
           "pose_skins": lambda k: ctx.pose_skins({ids["skin"]: palettes[k]})}
    # what the vertex array holds after a call: the pose calls write the skin's range only, over what the call before left elsewhere --
    # which lies outside the set's range too, so the set's range is a function of the call alone
    want = {"update_device": [NC.host_recompute(a, v, tris, first, count, NC.N | NC.B) for v in moved],
            "pose_skins": [NC.host_recompute(a, v, tris, first, count, NC.N | NC.B) for v in posed]}
    variants = [(p, s) for s in ("", "+set") for p in run]
    times = {p + s: [] for p, s in variants}
    phases, traced_total, equal = {}, {}, {}
    ids["skin"] = ctx.create_skin(skin.first, skin.rest, skin.indices, skin.weights, BONES)
    assert ids["skin"] >= 16

    def timed(p, s, k, check=False):
        ctx.sync()
        t0 = time.perf_counter()
        assert run[p](k) == 0
        ms = (time.perf_counter() - t0) * 1e3
        if s and check:
            got = ctx.read_accel(4)[first:first + count]
            equal[p] = equal.get(p, True) and bool(np.array_equal(NC.bits(got), NC.bits(want[p][k][first:first + count])))
        return ms

    def one_round(r, each):
        """the two paths without the set, then with it.  Creating the set is a second of host work (the topology read back, the counting
        sort over three million triangles) during which the device idles, and the first call behind it was measured at 3.5 to 20 ms: so
        each half begins with one call that is not timed, the half without the set too"""
        assert run["update_device"](r & 1) == 0
        for p in run:
            each(p, "", r)
        ids["set"] = ctx.create_normals(first, count)
        assert ids["set"] >= 16
        assert run["update_device"](r & 1) == 0
        for p in run:
            each(p, "+set", r)
        assert ctx.destroy_normals(ids["set"]) == 0

    for r in range(2):
        one_round(r, lambda p, s, r: timed(p, s, r & 1, check=True))
    for r in range(reps):
        one_round(r, lambda p, s, r: times[p + s].append(timed(p, s, r & 1)))

    def trace_one(p, s, r):
        _, log = traced(lambda: run[p](0))
        phases[p + s], traced_total[p + s] = stamps_of(log)
        if s:
            equal[p] = equal[p] and bool(np.array_equal(NC.bits(ctx.read_accel(4)[first:first + count]), NC.bits(want[p][0][first:first + count])))

    one_round(0, trace_one)
    ctx.render(1)
    ctx.sync()
    n_faces, n_entries = int(len(tables["faces"])), int(len(tables["entries"]))
    n_corners = int(len(np.unique(NC.corners_of(a)[tables["faces"].astype(np.int64)])))
    out = dict(scene=name, device=ctx.device_name(), bvh_width=ctx.bvh_width(), vertices=int(len(a.vertices)), set_vertices=int(count), faces=n_faces,
               entries=n_entries, row_length=dict(median=float(np.median(lengths)), max=int(lengths.max()), mean=round(n_entries / count, 3)), reps=reps,
               corner_vertices=n_corners,
               kernel_bytes=dict(k_face_frames=dict(requested=n_faces * (FACE_BYTES + 3 * CORNER_BYTES), unique=n_faces * FACE_BYTES + n_corners * 44),
                                 k_vertex_frames=dict(requested=int(count) * VERTEX_BYTES + n_entries * (ENTRY_BYTES + FRAME_BYTES),
                                                      unique=int(count) * VERTEX_BYTES + n_entries * ENTRY_BYTES + n_faces * FRAME_BYTES)),
               paths={v: dict(ms=round(float(np.median(times[v])), 3), ms_min=round(min(times[v]), 3), ms_max=round(max(times[v]), 3),
                              traced_total_ms=traced_total[v], phases_ms=phases[v]) for v in times},
               vertices_equal_host_build=equal)
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="atrium_small,bistro")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normals", "normals_bench.jsonl"))
    a = ap.parse_args()
    L = hip.Library()
    if L.device_count() <= 0:
        sys.exit("normals_bench needs a GPU")
    assert NC.have_normals_lib() and S.have_skin_lib(), "tests/hostsim is not built (run __graft_entry__.build())"
    lines = []
    for name, blob in scene_blobs(a.scenes.split(",")):
        lines.append(json.dumps(measure(L, name, blob, a.reps)))
        print(lines[-1], flush=True)
    if lines:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
