#!/usr/bin/env python3
"""Per level of a workload's light tree: nodes, the children whose importance needs arithmetic (centre_valid.w != 0 and
cosines.w != 0 in the rows fill_light_children makes -- the final select of light_child_importance), their maximum per node,
and the children that carry a flux without arithmetic.  The premise of k_light_pick_sparse (profiles/pick_sparse).
Usage: python tools/light_tree_occupancy.py [workload ...]   (CPU only; needs the host libraries build() makes)"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from ray_amd import hip  # noqa: E402

LEAF_BIT = 0x80000000


def light_rows(blob):
    """[n][26][4] float32: the importance rows of the blob's light tree, by the host build of fill_light_children"""
    import struct
    count = struct.unpack_from("<I", blob, 8)[0]
    for i in range(count):
        name, off, size = struct.unpack_from("<24sQQ", blob, 16 + i * 40)
        if name.rstrip(b"\0").decode() == "light_cwnodes":
            break
    else:
        raise SystemExit("the scene has no light tree")
    nodes = np.frombuffer(blob, dtype=hip.LIGHT_NODE_DTYPE, count=size // hip.LIGHT_NODE_DTYPE.itemsize, offset=off).copy()
    lib = C.CDLL(os.path.join(ROOT, "tests", "hostsim", "_build", "libhostsim_lights.so"))
    lib.hostsim_fill_light_children.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    rows = np.zeros((len(nodes), 26, 4), dtype=np.float32)
    assert lib.hostsim_fill_light_children(nodes.ctypes.data, len(nodes), rows.ctypes.data) == 0
    return rows


def table(rows):
    links = rows[:, 0:2, :].reshape(len(rows), 8).view(np.uint32)
    arith = (rows[:, 10:18, 3] != 0) & (rows[:, 18:26, 3] != 0)
    flux_only = ~arith & (rows[:, 18:26, 3].view(np.uint32) != 0)
    out, level = [], [0]
    while level:
        a = arith[level].sum(axis=1)
        out.append((len(level), int(a.sum()), int(a.max()), int(flux_only[level].sum())))
        level = [int(c) for n in level for c, occ in zip(links[n], arith[n] | flux_only[n]) if occ and not c & LEAF_BIT]
    return out, int(arith.sum()), int(flux_only.sum())


def main():
    library = bench.reference_scene_library()
    for name in sys.argv[1:] or ["bistro", "bistro_assets"]:
        blob = bench.export_reference_scene(bench.WORKLOADS[name], library)[0]
        rows = light_rows(blob)
        levels, arith, flux_only = table(rows)
        print(f"{name}: {len(rows)} nodes, {arith} children with arithmetic + {flux_only} with a flux alone in {8 * len(rows)} slots "
              f"({100.0 * (1.0 - arith / (8.0 * len(rows))):.0f} % of the evaluations on slots that need none)")
        print("| level | nodes | children with arithmetic | per node | max per node | flux alone |")
        print("|---|---|---|---|---|---|")
        for d, (n, a, m, f) in enumerate(levels):
            print(f"| {d} | {n} | {a} | {a / n:.2f} | {m} | {f} |")


if __name__ == "__main__":
    main()
