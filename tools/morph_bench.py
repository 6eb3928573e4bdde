"""What a morphed frame costs on the device, next to the route there was: one JSON line per scene and morph set.

  update_vertices:   rayhip_scene_update_vertices of vertices the HOST has morphed already (the route there was before; the host's morph
                     loop is not in the figure) -- 44 bytes per vertex through pageable memory, then the refit
  pose_skins:        rayhip_scene_pose_skins of ONE skin of 64 bones over the longest run of the vertex array that holds no vertex of a
                     triangle light, no morph set alive: the yardstick the morph's added cost is read against
  pose_morph_skin:   rayhip_scene_pose of a morph set over the same run TOGETHER with that skin: k_morph_skin_vertices, the fused kernel
  pose_morph:        rayhip_scene_pose of the morph set alone (the skin destroyed): k_morph_vertices

Two seeded sets over the run: FACE -- 52 targets, each over a compact seeded stretch of 2 to 20 % of the vertices, so the rows are
skewed (`row_length`: median and maximum) -- and DENSE -- 4 targets that touch every vertex.

Every path is called twice first (the first call allocates), then REPS times in turn with the others; `ms` is the wall time of an
untraced call between two device synchronisations (median, with the lowest and highest), `phases_ms` the differences of the
RAYHIP_TRACE_UPLOAD stamps of one more call -- each stamp waits for the device first, so the phases add up to more than an untraced call.
The kernels alone are timed by running this tool under `rocprofv3 --kernel-trace --stats`; `kernel_bytes` is what each needs to move, from
the shapes: base record, two row offsets, the row's entries, the `used` flag and the staged record per vertex, and the influences where a
skin follows.  After every timed pose the vertex array is read back and compared with the host build of morph.h
(tests/hostsim/hostsim_morph.cpp): launches of thousands of blocks, bit for bit.

Scenes: atrium_small, and the headline atrium (bench.py: bistro), from bench.py's scene cache or built into it.

usage: python tools/morph_bench.py [--scenes atrium_small,bistro] [--sets face,dense] [--reps 7] [--out profiles/morph/morph_bench.jsonl]
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

import morph_cases as M  # noqa: E402
import skin_cases as S  # noqa: E402
import util  # noqa: E402
import vertex_update_cases as V  # noqa: E402
from ray_amd import hip  # noqa: E402
from skin_bench import scene_blobs, stamps_of, whole_mesh_skin  # noqa: E402
from vertex_update_bench import traced  # noqa: E402

BONES = 64
VERTEX_BYTES = 44 + 8 + 1 + 44  # base record, the two row offsets, the `used` flag in; the posed record out
INFLUENCE_BYTES = 8 + 16        # bone indices and weights, where a skin follows
ENTRY_BYTES = 40


def whole_mesh_set(a, kind, seed):
    """FACE or DENSE (see above) over the longest run without a vertex of a triangle light"""
    first, count = S.free_ranges(a)[0]
    rng = np.random.RandomState(seed)
    ext = S.extent(a) * np.float32(0.2)  # (position deltas within 0.6 % of the extent per target)

    def target(lo, n):
        return (np.arange(lo, lo + n, dtype=np.uint32), (rng.uniform(-0.03, 0.03, size=(n, 3)) * ext).astype(np.float32),
                rng.uniform(-0.1, 0.1, size=(n, 3)).astype(np.float32), rng.uniform(-0.1, 0.1, size=(n, 3)).astype(np.float32))

    if kind == "dense":
        return M.MorphSet(a, first, count, [target(0, count) for _ in range(4)])
    targets = []
    for _ in range(52):
        n = max(1, int(rng.uniform(0.02, 0.2) * count))
        targets.append(target(int(rng.randint(0, count - n + 1)), n))
    return M.MorphSet(a, first, count, targets)


def measure(L, name, blob, kind, reps):
    a = V.Arrays(blob)
    ext = S.extent(a)
    ctx = hip.Context(0, L)
    ctx.upload_static(util.pmj())
    ctx.resize(256, 256)
    ctx.upload_scene_blob(blob)
    ctx.render(1)
    ms = whole_mesh_set(a, kind, 7)
    skin = whole_mesh_skin(a, BONES, 5)
    assert (skin.first, skin.count) == (ms.first, ms.count)
    lengths = ms.row_lengths()
    weights = [np.random.RandomState(20 + k).uniform(-0.5, 1.5, size=ms.targets_count).astype(np.float32) for k in range(2)]
    palettes = [S.palette(BONES, 10 + k, ext * np.float32(0.4)) for k in range(2)]
    want = {"pose_skins": [S.host_posed(a, [skin], [m]) for m in palettes],
            "pose_morph_skin": [M.host_morphed(a, [ms], [w], [skin], [m]) for w, m in zip(weights, palettes)],
            "pose_morph": [M.host_morphed(a, [ms], [w]) for w in weights]}
    host_vertices = want["pose_morph"]  # what the host route sends
    ids = {}
    run = {"update_vertices": lambda k: ctx.update_vertices(0, host_vertices[k]),
           "pose_skins": lambda k: ctx.pose_skins({ids["skin"]: palettes[k]}),
           "pose_morph_skin": lambda k: ctx.pose({ids["set"]: weights[k]}, {ids["skin"]: palettes[k]}),
           "pose_morph": lambda k: ctx.pose({ids["set"]: weights[k]}, {})}
    order = list(run)
    times = {p: [] for p in order}
    phases, traced_total, equal = {}, {}, {}

    def timed(p, k):
        ctx.sync()
        t0 = time.perf_counter()
        assert run[p](k) == 0
        ms_ = (time.perf_counter() - t0) * 1e3
        if p in want:
            equal[p] = equal.get(p, True) and bool(np.array_equal(S.bits(ctx.read_accel(4)), S.bits(want[p][k])))
        return ms_

    def one_round(r, each):
        """every path in turn: the skin alone first (pose_skins refuses a skin that holds a live set), then the set with it, then the set alone"""
        each("update_vertices", r)
        ids["skin"] = ctx.create_skin(skin.first, skin.rest, skin.indices, skin.weights, BONES)
        each("pose_skins", r)
        ids["set"] = ctx.create_morph(ms.first, ms.count, ms.base, ms.targets)
        assert ids["skin"] >= 16 and ids["set"] >= 16
        each("pose_morph_skin", r)
        assert ctx.destroy_skin(ids["skin"]) == 0
        each("pose_morph", r)
        assert ctx.destroy_morph(ids["set"]) == 0

    for r in range(2):
        one_round(r, lambda p, r: timed(p, r & 1))
    for r in range(reps):
        one_round(r, lambda p, r: times[p].append(timed(p, r & 1)))

    def trace_one(p, r):
        _, log = traced(lambda: run[p](0))
        phases[p], traced_total[p] = stamps_of(log)

    one_round(0, trace_one)
    ctx.render(1)
    ctx.sync()
    n, e = int(ms.count), int(lengths.sum())
    out = dict(scene=name, set=kind, device=ctx.device_name(), bvh_width=ctx.bvh_width(), vertices=int(len(a.vertices)), set_vertices=n,
               targets=ms.targets_count, entries=e, row_length=dict(median=float(np.median(lengths)), max=int(lengths.max()), mean=round(e / n, 3)),
               reps=reps,
               kernel_bytes=dict(k_morph_vertices=n * VERTEX_BYTES + e * ENTRY_BYTES, k_morph_skin_vertices=n * (VERTEX_BYTES + INFLUENCE_BYTES) + e * ENTRY_BYTES,
                                 k_skin_vertices=n * (44 + 8 + 16 + 1 + 44)),
               paths={p: dict(ms=round(float(np.median(times[p])), 3), ms_min=round(min(times[p]), 3), ms_max=round(max(times[p]), 3),
                              traced_total_ms=traced_total[p], phases_ms=phases[p]) for p in order},
               posed_vertices_equal_host_build=equal)
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="atrium_small,bistro")
    ap.add_argument("--sets", default="face,dense")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "morph", "morph_bench.jsonl"))
    a = ap.parse_args()
    L = hip.Library()
    if L.device_count() <= 0:
        sys.exit("morph_bench needs a GPU")
    assert M.have_morph_lib() and S.have_skin_lib(), "tests/hostsim is not built (run __graft_entry__.build())"
    lines = []
    for name, blob in scene_blobs(a.scenes.split(",")):
        for kind in a.sets.split(","):
            lines.append(json.dumps(measure(L, name, blob, kind, a.reps)))
            print(lines[-1], flush=True)
    if lines:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
