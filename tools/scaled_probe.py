#!/usr/bin/env python3
"""K10 (scaled render) kernel times over the bench's C2 data.

256 distinct 1024^2 four-channel big-endian uint16 tiles (2 GiB of planes, far larger than the
Infinity Cache) scaled to 96 x 96 through the strided entry points, one launch per 256 tiles:

  fused     omr_render_scaled_batch_strided_device: k_render_scale (8 MiB read + 36 KiB written
            per tile)
  k2        omr_render_batch_strided_device at full size on the same tiles: the bar
  unfused   the same scaled call on an OMR_SCALE_FUSED=0 context: K2 into the context buffer, then
            k_scale_argb
  jpeg      omr_render_thumbnail_jpeg_batch_device, q 0.9: wall-clock thumbnails per second

The kernel durations come from a rocprofv3 kernel trace of this script, a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- \\
        python3 tools/scaled_probe.py run --plan PLAN.json
    python3 tools/scaled_probe.py summarize DIR/.../t_kernel_trace.csv PLAN.json --json OUT.json

`run` also records each launch's own dispatch timestamps (omr_ctx_kernel_timings) in PLAN.json, so
a run without the profiler still yields the series; `summarize` cuts the trace's launches into the
sections in launch order, drops each section's warm-up pass and prints median and p10-p90.
"""
import argparse
import csv
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "omero-ms-image-region_amd"))

TILES, UNIQUE, CH, SIDE, OUT = 256, 64, 4, 1024, 96
HBM_PEAK = 8.0e12
READ_BYTES = TILES * CH * SIDE * SIDE * 2
BYTES = {"fused": READ_BYTES + TILES * OUT * OUT * 4, "k2": READ_BYTES + TILES * SIDE * SIDE * 4,
         "unfused_k2": READ_BYTES + TILES * SIDE * SIDE * 4, "unfused_scale": TILES * (SIDE * SIDE + OUT * OUT) * 4}
KERNEL_OF = {"fused": "k_render_scale", "k2": "k_render", "unfused_k2": "k_render", "unfused_scale": "k_scale_argb"}


def _series(ms):
    d = sorted(ms)
    return {"n": len(d), "median_us": d[len(d) // 2] * 1e3, "p10_us": d[len(d) // 10] * 1e3,
            "p90_us": d[(len(d) * 9) // 10] * 1e3}


def build_tiles(torch, dev):
    """256 distinct tiles from 64 generated ones: tile t is tile t % 64 rolled down by 256 * (t // 64) rows."""
    from omr.synthetic import torch_tiles_u16
    uniq = torch_tiles_u16(UNIQUE, CH, SIDE, SIDE, dev)
    uniq = uniq.view(torch.uint8).view(UNIQUE, CH, SIDE, SIDE, 2).flip(-1).contiguous().view(torch.int16).view(
        UNIQUE, CH, SIDE, SIDE)                                                    # -> big-endian bytes
    data = torch.empty((TILES, CH, SIDE, SIDE), dtype=torch.int16, device=dev)
    for t in range(TILES):
        data[t].copy_(torch.roll(uniq[t % UNIQUE], 256 * (t // UNIQUE), dims=1))
    return data


def run(args):
    import torch
    import omr
    from omr import _lib
    from omr.context import make_bindings, make_qdef
    from omr.synthetic import c2_channels
    dev = torch.device("cuda", 0)
    data = build_tiles(torch, dev)
    pb = SIDE * SIDE * 2
    table = torch.tensor([[data.data_ptr() + (t * CH + c) * pb for c in range(CH)] for t in range(TILES)],
                         dtype=torch.int64, device=dev)
    small = torch.empty((TILES, OUT, OUT), dtype=torch.int32, device=dev)
    full = torch.empty((TILES, SIDE, SIDE), dtype=torch.int32, device=dev)
    status = torch.empty(TILES, dtype=torch.int32, device=dev)
    q, chans = make_qdef("rgb"), c2_channels(CH)
    binds = make_bindings(chans)
    torch.cuda.synchronize()
    os.environ["OMR_SCALE_FUSED"] = "0"
    ctx_u = omr.Context(0, torch_order=False)
    os.environ.pop("OMR_SCALE_FUSED")
    ctx = omr.Context(0, torch_order=False)
    n = args.warmup + args.launches
    plan = {"tiles": TILES, "out": OUT, "warmup": args.warmup, "sections": [], "events_us": {}}

    def scaled(c):
        c.render_scaled_batch_strided_device(q, chans, data, CH * pb, pb, TILES, _lib.PIXELS_UINT16, SIDE, SIDE, small,
                                             OUT, OUT, status, big_endian=True, bindings=binds)

    def k2(c):
        c.render_batch_strided_device(q, chans, data, CH * pb, pb, TILES, _lib.PIXELS_UINT16, SIDE, SIDE, full, status,
                                      big_endian=True, bindings=binds)

    for name, c, call, kinds in (("fused", ctx, scaled, {10: "fused"}), ("k2", ctx, k2, {2: "k2"}),
                                 ("unfused", ctx_u, scaled, {2: "unfused_k2", 11: "unfused_scale"})):
        c.enable_kernel_timing(True)
        for _ in range(n):
            call(c)
            c.synchronize()
        got = c.kernel_timings()
        c.enable_kernel_timing(False)
        for kind, key in kinds.items():
            ms = [m for m, k in got if k == kind]
            assert len(ms) == n, (name, kind, len(ms))
            plan["events_us"][key] = _series(ms[args.warmup:])
            plan["sections"].append({"key": key, "kernel": KERNEL_OF[key], "launches": n})
    ref = small.clone()
    scaled(ctx)
    ctx.synchronize()
    assert torch.equal(ref, small), "fused and unfused routes differ"
    # thumbnails per second: the whole call (scaled render + the batched encoder), files left in HBM
    d_out = torch.empty(TILES * (OUT * OUT * 4 + 4096), dtype=torch.uint8, device=dev)
    offs = torch.empty(TILES, dtype=torch.int64, device=dev)
    lens = torch.empty(TILES, dtype=torch.int32, device=dev)
    wall = []
    for _ in range(n):
        t0 = time.perf_counter()
        ctx.render_thumbnail_jpeg_batch_device(q, chans, table, TILES, _lib.PIXELS_UINT16, SIDE, SIDE, OUT, OUT, 0.9,
                                               d_out, offs, lens, status, big_endian=True, bindings=binds)
        ctx.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    s = _series(wall[args.warmup:])
    plan["jpeg"] = dict(s, thumbnails_per_s=round(TILES / (s["median_us"] * 1e-6), 1),
                        mean_file_bytes=round(float(lens.float().mean().item()), 1))
    ctx.close()
    ctx_u.close()
    try:
        sys.path.insert(0, REPO)
        import bench
        plan["build_id"] = bench.kernel_build_id()
    except Exception:
        plan["build_id"] = None
    for key, s in plan["events_us"].items():
        s["hbm_fraction"] = round(BYTES[key] / (s["median_us"] * 1e-6) / HBM_PEAK, 3)
        print(f"{key:14s} median {s['median_us']:8.1f} us (p10 {s['p10_us']:.1f}, p90 {s['p90_us']:.1f}, n={s['n']})  "
              f"{s['hbm_fraction']:.3f} of HBM peak  [dispatch timestamps]")
    print(f"jpeg           median {plan['jpeg']['median_us']:8.1f} us per {TILES} thumbnails: "
          f"{plan['jpeg']['thumbnails_per_s']:.0f} thumbnails/s, {plan['jpeg']['mean_file_bytes']:.0f} B per file")
    with open(args.plan, "w") as fh:
        json.dump(plan, fh, indent=1)


def summarize(args):
    plan = json.load(open(args.plan))
    rows = {}
    with open(args.trace) as fh:
        for r in csv.DictReader(fh):
            name = r["Kernel_Name"]
            if "k_render_scale" in name:
                kern = "k_render_scale"
            elif "k_scale_argb" in name:
                kern = "k_scale_argb"
            elif "k_render<" in name or "k_render_pipe<" in name:      # K2
                kern = "k_render"
            else:
                continue
            rows.setdefault(kern, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]),
                                              name, r.get("VGPR_Count", ""), r.get("LDS_Block_Size", "")))
    for v in rows.values():
        v.sort()
    pos = {}
    out = {"build_id": plan.get("build_id"), "tiles": plan["tiles"], "trace_us": {}, "events_us": plan["events_us"],
           "jpeg": plan["jpeg"]}
    for sec in plan["sections"]:
        src = rows.get(sec["kernel"], [])
        p = pos.get(sec["kernel"], 0)
        grp = src[p:p + sec["launches"]]
        pos[sec["kernel"]] = p + sec["launches"]
        d = [g[1] * 1e-6 for g in grp[plan["warmup"]:]]                             # ns -> ms
        if not d:
            continue
        s = _series(d)
        s["hbm_fraction"] = round(BYTES[sec["key"]] / (s["median_us"] * 1e-6) / HBM_PEAK, 3)
        s["kernel"], s["vgprs"], s["lds"] = grp[-1][2].split("(")[0][-90:], grp[-1][3], grp[-1][4]
        out["trace_us"][sec["key"]] = s
        print(f"{sec['key']:14s} median {s['median_us']:8.1f} us (p10 {s['p10_us']:.1f}, p90 {s['p90_us']:.1f}, "
              f"n={s['n']})  {s['hbm_fraction']:.3f} of HBM peak  vgprs={s['vgprs']} lds={s['lds']}  {s['kernel']}")
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--plan", required=True)
    r.add_argument("--launches", type=int, default=32, help="timed launches per section")
    r.add_argument("--warmup", type=int, default=1)
    s = sub.add_parser("summarize")
    s.add_argument("trace")
    s.add_argument("plan")
    s.add_argument("--json", default=None)
    a = ap.parse_args()
    run(a) if a.cmd == "run" else summarize(a)


if __name__ == "__main__":
    main()
