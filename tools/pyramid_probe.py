#!/usr/bin/env python3
"""K11 (pyramid levels) kernel times over the bench's C2 data.

256 distinct 1024^2 four-channel big-endian uint16 tiles (1,024 planes, 2 GiB, far larger than the
Infinity Cache).  A pass builds the pyramids of all 1,024 planes with n_levels = 5 (1024 -> 64) in
32 calls of 32 planes; each call is one launch of k_pyramid (levels 1-3 in each lane's registers,
level 4 by an exchange between neighbouring lanes).  The bar is K2 rendering the same 256 tiles at
full size in one launch (omr_render_batch_strided_device): a pass of K11 moves 0.89 of K2's bytes
and must take no longer.

  mean, subsample   per pass: the sum of its 32 launches; per launch: one 32-plane launch
  k2                one launch per 256 tiles

The kernel durations come from a rocprofv3 kernel trace of this script, a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- \\
        python3 tools/pyramid_probe.py run --plan PLAN.json
    python3 tools/pyramid_probe.py summarize DIR/.../t_kernel_trace.csv PLAN.json --json OUT.json

`run` also records each launch's own dispatch timestamps (omr_ctx_kernel_timings) in PLAN.json, so
a run without the profiler still yields the series; `summarize` cuts the trace's launches into the
sections in launch order, drops each section's warm-up pass and prints median and p10-p90.
"""
import argparse
import csv
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "omero-ms-image-region_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from scaled_probe import CH, SIDE, TILES, _series, build_tiles   # noqa: E402  (the same data)

PLANES, BATCH, LEVELS = TILES * CH, 32, 5
CALLS = PLANES // BATCH
HBM_PEAK = 8.0e12
LEVEL_PX = [(SIDE >> k) ** 2 for k in range(LEVELS)]
# mean reads every pixel of its source; subsample needs the even rows only (but whole 16-byte chunks of them)
MAIN_BYTES = {"mean": BATCH * 2 * sum(LEVEL_PX), "subsample": BATCH * 2 * (LEVEL_PX[0] // 2 + sum(LEVEL_PX[1:]))}
PASS_BYTES = {"mean": PLANES * 2 * sum(LEVEL_PX), "subsample": PLANES * 2 * (LEVEL_PX[0] // 2 + sum(LEVEL_PX[1:])),
              "k2": PLANES * SIDE * SIDE * 2 + TILES * SIDE * SIDE * 4}
LAUNCHES_PER_CALL = 1


def _pass_series(ms, per_pass):
    """Per-pass sums (ms) and the first launch of every call."""
    passes = [sum(ms[i:i + per_pass]) for i in range(0, len(ms), per_pass)]
    return _series(passes), _series(ms[0::LAUNCHES_PER_CALL])


def run(args):
    import torch
    import omr
    from omr import _lib
    from omr.context import make_bindings, make_qdef
    from omr.synthetic import c2_channels
    dev = torch.device("cuda", 0)
    data = build_tiles(torch, dev)                               # [256][4][1024][1024] big-endian uint16
    planes = data.view(PLANES, SIDE, SIDE)
    outs = [torch.empty((BATCH, SIDE >> k, SIDE >> k), dtype=torch.int16, device=dev) for k in range(1, LEVELS)]
    full = torch.empty((TILES, SIDE, SIDE), dtype=torch.int32, device=dev)
    status = torch.empty(TILES, dtype=torch.int32, device=dev)
    q, chans = make_qdef("rgb"), c2_channels(CH)
    binds = make_bindings(chans)
    pb = SIDE * SIDE * 2
    ptrs = [planes.data_ptr() + i * pb for i in range(PLANES)]
    torch.cuda.synchronize()
    n = args.warmup + args.passes
    plan = {"planes": PLANES, "planes_per_call": BATCH, "n_levels": LEVELS, "calls_per_pass": CALLS,
            "launches_per_call": LAUNCHES_PER_CALL, "warmup": args.warmup, "sections": [], "events_us": {}}
    with omr.Context(0, torch_order=False) as ctx:
        for key, rule in (("mean", _lib.PYRAMID_MEAN), ("subsample", _lib.PYRAMID_SUBSAMPLE)):
            ctx.enable_kernel_timing(True)
            for _ in range(n):
                for c in range(CALLS):
                    ctx.pyramid_build_device(ptrs[c * BATCH:(c + 1) * BATCH], _lib.PIXELS_UINT16, SIDE, SIDE, outs, LEVELS,
                                             rule=rule, big_endian=True)
                ctx.synchronize()
            ms = [m for m, k in ctx.kernel_timings() if k == 12]
            ctx.enable_kernel_timing(False)
            per_pass = CALLS * LAUNCHES_PER_CALL
            assert len(ms) == n * per_pass, (key, len(ms))
            ps, ls = _pass_series(ms[args.warmup * per_pass:], per_pass)
            plan["events_us"][key + "_pass"], plan["events_us"][key + "_launch"] = ps, ls
            plan["sections"].append({"key": key, "kernel": "k_pyramid", "launches": n * per_pass})
            # the last call's level 4 against torch on the same planes (subsample: a strided view)
            if rule == _lib.PYRAMID_SUBSAMPLE:
                assert torch.equal(outs[3], planes[PLANES - BATCH:, ::16, ::16]), "subsample level 4 differs"
        ctx.enable_kernel_timing(True)
        for _ in range(n):
            ctx.render_batch_strided_device(q, chans, data, CH * pb, pb, TILES, _lib.PIXELS_UINT16, SIDE, SIDE, full, status,
                                            big_endian=True, bindings=binds)
            ctx.synchronize()
        ms = [m for m, k in ctx.kernel_timings() if k == 2]
        ctx.enable_kernel_timing(False)
        assert len(ms) == n, len(ms)
        plan["events_us"]["k2"] = _series(ms[args.warmup:])
        plan["sections"].append({"key": "k2", "kernel": "k_render", "launches": n})
    try:
        sys.path.insert(0, REPO)
        import bench
        plan["build_id"] = bench.kernel_build_id()
    except Exception:
        plan["build_id"] = None
    report(plan["events_us"], "dispatch timestamps")
    with open(args.plan, "w") as fh:
        json.dump(plan, fh, indent=1)


def report(series, source):
    k2 = series.get("k2")
    for key, s in series.items():
        rule = key.split("_")[0]
        nbytes = PASS_BYTES[rule] if key.endswith("_pass") or key == "k2" else MAIN_BYTES[rule]
        s["hbm_fraction"] = round(nbytes / (s["median_us"] * 1e-6) / HBM_PEAK, 3)
        extra = ""
        if key.endswith("_pass") and k2:
            s["vs_k2"] = round(s["median_us"] / k2["median_us"], 3)
            extra = f"  {s['vs_k2']:.3f} x K2 ({'meets' if s['vs_k2'] <= 1.0 else 'MISSES'} the bar)"
        print(f"{key:18s} median {s['median_us']:9.1f} us (p10 {s['p10_us']:.1f}, p90 {s['p90_us']:.1f}, n={s['n']})  "
              f"{s['hbm_fraction']:.3f} of HBM peak{extra}  [{source}]")


def summarize(args):
    plan = json.load(open(args.plan))
    rows = {}
    with open(args.trace) as fh:
        for r in csv.DictReader(fh):
            name = r["Kernel_Name"]
            if "k_pyramid" in name:
                kern = "k_pyramid"
            elif "k_render<" in name or "k_render_pipe<" in name:      # K2
                kern = "k_render"
            else:
                continue
            rows.setdefault(kern, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]),
                                              name, r.get("VGPR_Count", "")))
    for v in rows.values():
        v.sort()
    pos, series, info = {}, {}, {}
    per_pass = plan["calls_per_pass"] * plan["launches_per_call"]
    for sec in plan["sections"]:
        src = rows.get(sec["kernel"], [])
        p = pos.get(sec["kernel"], 0)
        grp = src[p:p + sec["launches"]]
        pos[sec["kernel"]] = p + sec["launches"]
        if len(grp) != sec["launches"]:
            print(f"{sec['key']}: {len(grp)} of {sec['launches']} launches in the trace, skipped")
            continue
        info[sec["key"]] = {"kernel": grp[0][2].split("(")[0][-90:], "vgprs": grp[0][3]}
        if sec["key"] == "k2":
            series["k2"] = _series([g[1] * 1e-6 for g in grp[plan["warmup"]:]])             # ns -> ms
        else:
            d = [g[1] * 1e-6 for g in grp[plan["warmup"] * per_pass:]]
            series[sec["key"] + "_pass"], series[sec["key"] + "_launch"] = _pass_series(d, per_pass)
    series = dict(sorted(series.items(), key=lambda kv: kv[0] != "k2"))                     # k2 first: the bar
    report(series, "kernel trace")
    for key, v in info.items():
        print(f"{key:18s} vgprs={v['vgprs']}  {v['kernel']}")
    if args.json:
        with open(args.json, "w") as fh:
            json.dump({"build_id": plan.get("build_id"), "planes": plan["planes"], "n_levels": plan["n_levels"],
                       "trace_us": series, "events_us": plan["events_us"], "kernels": info}, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--plan", required=True)
    r.add_argument("--passes", type=int, default=32, help="timed passes over the 1,024 planes per rule (and K2 launches)")
    r.add_argument("--warmup", type=int, default=1)
    s = sub.add_parser("summarize")
    s.add_argument("trace")
    s.add_argument("plan")
    s.add_argument("--json", default=None)
    a = ap.parse_args()
    run(a) if a.cmd == "run" else summarize(a)


if __name__ == "__main__":
    main()
