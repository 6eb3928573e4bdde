#!/usr/bin/env python3
"""rocprofv3 counter CSVs -> the address-path table of the shade kernels (profiles/r08/shade_address_path_*.txt).

    python tools/shade_address_path.py <out.txt> <ta_dir> <sq_dir> <bench.log> [<title>]

ta_dir / sq_dir: output directories of two runs of
    rocprofv3 --kernel-trace --pmc <group> --output-format csv -- python bench.py --steps 4 --warmup 1 --no-cpu-baseline
with the groups  TA_BUSY_avr GRBM_GUI_ACTIVE  and  SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_WAIT_INST_ANY
(counters in runs of their own: no other tracing next to them); bench.log: the output of the same command (its last line is the JSON result).

Per kernel:
  TA busy       TA_BUSY_avr / (GRBM_GUI_ACTIVE / 8) over every dispatch of the run: the share of the kernel's time in which a CU's
                texture-address unit (the address path of every vector-memory instruction) is busy.  The divisor 8 is the one
                profiles/r02/pmc_sq_tcc_ta_summary.txt was read with (GRBM_GUI_ACTIVE is summed over the eight XCDs); the closest-hit kernels
                are listed for comparison.
  per chunk     wave-level instruction counts over the chunks of 64 rays the kernel walked, over the FULL frames of the run (the priming, warm-up
                and timed frames: a frame starts at a primary k_surface_scatter dispatch of the largest grid and ends at the next primary
                dispatch; the one-iteration instrumented passes at the end are left out).  The hardware does not count chunks; they come from
                the bench line: a frame has W x H x spp / 64 primary chunks and (rays_per_sample - 1) times as many secondary ones (queues are
                dense: a partly filled chunk per stripe and bounce is ignored); the pick walks both.  The next-event kernel walks the lit
                records, which the bench line does not count: its chunks are taken as the shadow rays / 64, which it emits for a subset of
                the records -- a LOWER bound of its chunks, so its per-chunk columns are upper bounds.
  waiting       SQ_WAIT_INST_ANY / SQ_WAVE_CYCLES, every dispatch."""
import csv, glob, os, re, sys
from collections import defaultdict

SHADE = ("shade::k_surface_scatter", "shade::k_scatter<true, false", "shade::k_light_pick_first")
COMPARE = ("k_trace_closest_refill", "k_trace_closest_pool", "k_trace_closest<false")

def short(name):
    name = name.split("(")[0].replace("void ", "").replace("rt::", "")
    return re.sub(r"\s+", " ", name).strip()


def read(d):
    """{dispatch id: (kernel, blocks, {counter: value})} of one profile directory"""
    out = {}
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                i = int(row.get("Dispatch_Id", 0))
                grid = float(row.get("Grid_Size", row.get("Grid_Size_X", 0)) or 0)
                wg = float(row.get("Workgroup_Size", row.get("Workgroup_Size_X", 0)) or 0)
                e = out.setdefault(i, (short(row.get("Kernel_Name", "")), int(grid / wg) if wg else 0, {}))
                e[2][row["Counter_Name"]] = e[2].get(row["Counter_Name"], 0.0) + float(row["Counter_Value"] or 0)
    return out


def frame_chunks(bench_log):
    """{kernel prefix: chunks per full frame} from the JSON line of the bench run"""
    import json
    with open(bench_log) as fh:
        d = json.loads([l for l in fh.read().splitlines() if l.startswith("{")][-1])
    c = d["config"]
    primary = c["width"] * c["height"] * c["spp"] / 64.0
    rps = d["roofline"]["rays_per_sample"]
    shadow = d["roofline"]["shadow_kernel"]["rays_per_sample"]
    return {"shade::k_surface_scatter<true": primary, "shade::k_surface_scatter<false": (rps - 1.0) * primary,
            "shade::k_light_pick_first": rps * primary, "shade::k_scatter<true, false": shadow * primary,
            "k_trace_closest_refill<4, 64": primary, "k_trace_closest_refill<4, 40": (rps - 1.0) * primary}


def full_frames(rows):
    """(dispatch ids inside full frames, number of full frames)"""
    ids = sorted(rows)
    prim = [i for i in ids if "k_surface_scatter<true" in rows[i][0]]
    if not prim:
        return set(), 0
    big = max(rows[i][1] for i in prim)
    inside, n = set(), 0
    for k, i in enumerate(prim):
        if rows[i][1] != big:
            continue
        n += 1
        # (the pick and the closest-hit launch of the primary rays precede the primary shade kernel: from the previous frame's end)
        lo = prim[k - 1] if k > 0 else -1
        prev_end = max((j for j in ids if lo < j < i and "k_surface_scatter<false" in rows[j][0]), default=lo)
        hi = prim[k + 1] if k + 1 < len(prim) else ids[-1] + 1
        nxt_start = max((j for j in ids if i < j < hi and "k_surface_scatter<false" in rows[j][0]), default=i)
        inside.update(j for j in ids if prev_end < j <= max(nxt_start, i) + 3)
    return inside, n


def main():
    out_path, ta_dir, sq_dir, bench_log = sys.argv[1:5]
    title = sys.argv[5] if len(sys.argv) > 5 else ""
    ta, sq = read(ta_dir), read(sq_dir)
    wanted = lambda k: any(s in k for s in SHADE + COMPARE)
    lines = [f"# {title}".rstrip(), "# rocprofv3 --kernel-trace --pmc <group> -- python bench.py --steps 4 --warmup 1 --no-cpu-baseline (bistro, 1080p, 64 spp), "
             "one run per group; tools/shade_address_path.py", "#"]
    lines.append(f"# {'kernel':50s} {'disp':>5s} {'TA_BUSY_avr':>12s} {'GRBM_GUI_ACT':>12s} {'TA busy':>8s}")
    acc = defaultdict(lambda: defaultdict(float))
    for k, _, c in ta.values():
        if wanted(k):
            acc[k]["n"] += 1
            for name, v in c.items():
                acc[k][name] += v
    for k in sorted(acc):
        a = acc[k]
        frac = a["TA_BUSY_avr"] / (a["GRBM_GUI_ACTIVE"] / 8.0) if a["GRBM_GUI_ACTIVE"] else 0.0
        lines.append(f"  {k[:50]:50s} {int(a['n']):5d} {a['TA_BUSY_avr']:12.4g} {a['GRBM_GUI_ACTIVE']:12.4g} {frac:8.3f}")
    lines += ["#", f"# {'kernel':50s} {'disp':>5s} {'VMEM_RD':>10s} {'VMEM_WR':>10s} {'LDS':>10s} {'WAVE_CYC':>10s} {'WAIT_INST':>10s} {'waiting':>8s} "
              f"{'disp used':>9s} {'chunks':>10s} {'RD/chunk':>9s} {'WR/chunk':>9s} {'VMEM/chunk':>10s} {'LDS/chunk':>9s}"]
    per_frame = frame_chunks(bench_log)
    inside, n_frames = full_frames(sq)
    lines.insert(3, f"# full frames in the run: {n_frames}; chunks per frame: " + ", ".join(f"{k.replace('shade::', '')}...: {v:.4g}" for k, v in per_frame.items()))
    acc = defaultdict(lambda: defaultdict(float))
    for i, (k, _, c) in sq.items():
        if not wanted(k):
            continue
        a = acc[k]
        a["n"] += 1
        for name, v in c.items():
            a[name] += v
        if i in inside:
            a["used"] += 1
            a["chunks"] = n_frames * next((v for p, v in per_frame.items() if p in k), 0.0)
            for name in ("SQ_INSTS_VMEM_RD", "SQ_INSTS_VMEM_WR", "SQ_INSTS_LDS"):
                a["c_" + name] += c.get(name, 0.0)
    for k in sorted(acc):
        a = acc[k]
        wait = a["SQ_WAIT_INST_ANY"] / a["SQ_WAVE_CYCLES"] if a["SQ_WAVE_CYCLES"] else 0.0
        per = (lambda name: a["c_" + name] / a["chunks"]) if a["chunks"] else (lambda name: 0.0)
        lines.append(f"  {k[:50]:50s} {int(a['n']):5d} {a['SQ_INSTS_VMEM_RD']:10.4g} {a['SQ_INSTS_VMEM_WR']:10.4g} {a['SQ_INSTS_LDS']:10.4g} "
                     f"{a['SQ_WAVE_CYCLES']:10.4g} {a['SQ_WAIT_INST_ANY']:10.4g} {wait:8.3f} {int(a['used']):9d} {a['chunks']:10.4g} "
                     f"{per('SQ_INSTS_VMEM_RD'):9.2f} {per('SQ_INSTS_VMEM_WR'):9.2f} {per('SQ_INSTS_VMEM_RD') + per('SQ_INSTS_VMEM_WR'):10.2f} {per('SQ_INSTS_LDS'):9.2f}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
