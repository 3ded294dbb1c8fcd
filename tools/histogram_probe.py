#!/usr/bin/env python3
"""K9 (plane statistics + histogram) kernel times over the bench's C2 data.

256 distinct 1024^2 big-endian uint16 planes (512 MiB, larger than the Infinity Cache), in
batches of 32 planes per call: histogram (256 bins, explicit range 0..65535) and statistics, then
the same over constant planes (every pixel in one bin: the LDS contention case).  The kernel
durations come from a rocprofv3 kernel trace of this script, a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- \\
        python3 tools/histogram_probe.py run --plan PLAN.json [--sweep]
    python3 tools/histogram_probe.py summarize DIR/.../t_kernel_trace.csv PLAN.json

`run` executes a list of configurations one after the other (route: 0 the library's choice,
1 fp64 evaluation, 2 LDS table; rep: sub-histogram copies per workgroup, 0 the library's choice;
both through the OMR_HIST_ROUTE / OMR_HIST_REP measurement switches) and writes the list with the
number of launches of each to PLAN.json; `summarize` cuts the trace's K9 launches into those
groups in launch order, drops each group's warm-up pass and prints the median per group with
bytes / time as a fraction of the 8 TB/s HBM peak.  --sweep adds the replication factors.
"""
import argparse
import csv
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "omero-ms-image-region_amd"))

PLANES, BATCH, SIDE = 256, 32, 1024
HBM_PEAK = 8.0e12


def configs(sweep, which):
    out = []
    for data in which:
        out.append({"op": "stats", "data": data, "route": 0, "rep": 0})
        out.append({"op": "hist", "data": data, "route": 0, "rep": 0})
        out.append({"op": "hist", "data": data, "route": 1, "rep": 0})
        out.append({"op": "hist", "data": data, "route": 2, "rep": 0})
        if sweep:
            for route in (1, 2):
                for rep in (1, 2, 4, 8, 16, 32):
                    out.append({"op": "hist", "data": data, "route": route, "rep": rep})
    return out


def run(args):
    import torch
    import omr
    from omr import _lib
    from omr.synthetic import torch_tiles_u16
    dev = torch.device("cuda", 0)
    tiles = torch_tiles_u16(PLANES // 4, 4, SIDE, SIDE, dev)
    micro = tiles.view(torch.uint8).view(PLANES, SIDE, SIDE, 2).flip(-1).contiguous().view(torch.int16).view(
        PLANES, SIDE, SIDE)                                                        # -> big-endian bytes
    del tiles
    const = torch.full((PLANES, SIDE, SIDE), 600, dtype=torch.int16, device=dev)
    const = const.view(torch.uint8).view(PLANES, SIDE, SIDE, 2).flip(-1).contiguous().view(torch.int16).view(
        PLANES, SIDE, SIDE)
    torch.cuda.synchronize()
    plan = configs(args.sweep, ("microscopy", "constant") if args.data == "both" else (args.data,))
    with omr.Context(0) as ctx:
        for cfg in plan:
            os.environ["OMR_HIST_ROUTE"] = str(cfg["route"])
            os.environ["OMR_HIST_REP"] = str(cfg["rep"])
            data = micro if cfg["data"] == "microscopy" else const
            launches = 0
            for p in range(args.warmup + args.passes):
                for b in range(0, PLANES, BATCH):
                    planes = [data[i] for i in range(b, b + BATCH)]
                    if cfg["op"] == "hist":
                        counts, info = ctx.histogram(planes, _lib.PIXELS_UINT16, SIDE, SIDE, [(0.0, 65535.0)],
                                                     bins=256, big_endian=True)
                        assert int(counts[0].sum()) + info[0]["above"] + info[0]["below"] == SIDE * SIDE
                    else:
                        ctx.plane_stats(planes, _lib.PIXELS_UINT16, SIDE, SIDE, big_endian=True)
                    launches += 1
            cfg["launches"] = launches
            cfg["warmup_launches"] = args.warmup * (PLANES // BATCH)
    os.environ.pop("OMR_HIST_ROUTE", None)
    os.environ.pop("OMR_HIST_REP", None)
    try:
        sys.path.insert(0, REPO)
        import bench
        build = bench.kernel_build_id()
    except Exception:
        build = None
    with open(args.plan, "w") as fh:
        json.dump({"build_id": build, "planes_per_launch": BATCH, "bytes_per_launch": BATCH * SIDE * SIDE * 2,
                   "configs": plan}, fh, indent=1)
    print(f"{len(plan)} configurations, plan in {args.plan}")


def summarize(args):
    plan = json.load(open(args.plan))
    hist, stats = [], []
    with open(args.trace) as fh:
        for r in csv.DictReader(fh):
            name = r["Kernel_Name"]
            row = (int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), name,
                   r.get("LDS_Block_Size", ""), r.get("Grid_Size_X", r.get("Grid_Size", "")),
                   r.get("Workgroup_Size_X", r.get("Workgroup_Size", "")))
            if "k_plane_histogram" in name:
                hist.append(row)
            elif "k_plane_minmax" in name and "k_plane_minmax_final" not in name:
                stats.append(row)
    hist.sort()
    stats.sort()
    pos = {"hist": 0, "stats": 0}
    rows = []
    for cfg in plan["configs"]:
        src = hist if cfg["op"] == "hist" else stats
        grp = src[pos[cfg["op"]]:pos[cfg["op"]] + cfg["launches"]]
        pos[cfg["op"]] += cfg["launches"]
        d = sorted(g[1] for g in grp[cfg["warmup_launches"]:])
        if not d:
            continue
        med = d[len(d) // 2]
        rows.append(dict(cfg, kernel=grp[-1][2].split("(")[0], lds=grp[-1][3], grid_x=grp[-1][4], block=grp[-1][5],
                         timed=len(d), median_us=med / 1e3, p10_us=d[len(d) // 10] / 1e3,
                         p90_us=d[(len(d) * 9) // 10] / 1e3,
                         hbm_fraction=round(plan["bytes_per_launch"] / (med * 1e-9) / HBM_PEAK, 3)))
    for r in rows:
        print(f"{r['op']:5s} {r['data']:10s} route={r['route']} rep={r['rep']:2d}  median {r['median_us']:8.1f} us  "
              f"(p10 {r['p10_us']:.1f}, p90 {r['p90_us']:.1f}, n={r['timed']})  {r['hbm_fraction']:.3f} of HBM peak  "
              f"lds={r['lds']} grid_x={r['grid_x']} block={r['block']}  {r['kernel'][-60:]}")
    if args.json:
        with open(args.json, "w") as fh:
            json.dump({"build_id": plan.get("build_id"), "bytes_per_launch": plan["bytes_per_launch"], "rows": rows}, fh,
                      indent=1)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--plan", required=True)
    r.add_argument("--sweep", action="store_true")
    r.add_argument("--passes", type=int, default=4, help="timed passes over the 256 planes per configuration")
    r.add_argument("--warmup", type=int, default=1)
    r.add_argument("--data", choices=["both", "microscopy", "constant"], default="both",
                   help="one data set only (a counter run tells its kernels apart by name alone)")
    s = sub.add_parser("summarize")
    s.add_argument("trace")
    s.add_argument("plan")
    s.add_argument("--json", default=None)
    a = ap.parse_args()
    run(a) if a.cmd == "run" else summarize(a)


if __name__ == "__main__":
    main()
