#!/usr/bin/env python3
"""K12 (raw grey PNG tiles) kernel times over the bench's C2 data.

256 distinct 1024^2 big-endian uint16 planes (one channel each) -> 256 grey-16 PNG files per call
of omr_encode_png_gray_batch_device, through the wave filter (the default) and through the
workgroup filter (a context created with OMR_PNG_GRAY_WAVE=0); then, in the same process, the
batched RGB PNG of 256 rendered C2 tiles (omr_encode_png_batch_device, the bench's png.batched
case) as the yardstick of the filter stage.  One warm-up call and 32 timed calls per
configuration.  The kernel durations come from a rocprofv3 kernel trace of this script, a run of
its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- \\
        python3 tools/raw_png_probe.py run --plan PLAN.json
    python3 tools/raw_png_probe.py summarize DIR/.../t_kernel_trace.csv PLAN.json [--json OUT.json]

`run` also takes the wall time of the calls (tiles/s), the mean file size and, for the first
tiles, the size of PIL.Image.save(format="png") of the same pixels, and writes them with the
launch plan to PLAN.json.  `summarize` cuts the trace into calls at each filter launch, drops the
warm-up calls and prints per kernel the median and p10-p90 of its time per call, and the filter
stage's time per byte of filtered stream.
"""
import argparse
import csv
import io
import json
import os
import re
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "omero-ms-image-region_amd"))

N, SIDE = 256, 1024
FILTERS = ("k_pngb_filter_gray", "k_pngb_filter_wave", "k_pngb_filter")


def run(args):
    import numpy as np
    import torch
    import omr
    from omr import _lib
    from omr.context import make_bindings, make_qdef
    from omr.synthetic import c2_channels, torch_tiles_u16
    dev = torch.device("cuda", 0)
    tiles = torch_tiles_u16(N // 4, 4, SIDE, SIDE, dev)
    planes = tiles.view(torch.uint8).view(N, SIDE, SIDE, 2).flip(-1).contiguous().view(torch.int16).view(
        N, SIDE, SIDE)                                                             # -> big-endian bytes
    del tiles
    torch.cuda.synchronize()
    calls = args.warmup + args.passes
    plan = []

    def timed(step, ctx):
        for _ in range(args.warmup):
            step()
        ctx.synchronize()
        t = []
        for _ in range(args.passes):
            t0 = time.perf_counter()
            step()
            ctx.synchronize()
            t.append(time.perf_counter() - t0)
        t.sort()
        return t[len(t) // 2]

    # grey-16 files of the 256 planes, both filter routes
    cap = _lib.lib.omr_png_gray_batch_max_bytes(SIDE, SIDE, 2, N)
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    offs = torch.empty(N, dtype=torch.int64, device=dev)
    lens = torch.empty(N, dtype=torch.int32, device=dev)
    stat = torch.empty(N, dtype=torch.int32, device=dev)
    spec = [(planes[i], SIDE, 0, 0) for i in range(N)]
    files = {}
    for route in ("wave", "workgroup"):
        if route == "workgroup":
            os.environ["OMR_PNG_GRAY_WAVE"] = "0"
        ctx = omr.Context(0, torch_order=False)
        os.environ.pop("OMR_PNG_GRAY_WAVE", None)
        med = timed(lambda: ctx.encode_png_gray_batch_device(spec, _lib.PIXELS_UINT16, SIDE, SIDE, out, offs, lens,
                                                              stat, big_endian=True), ctx)
        assert int((stat == 0).sum().item()) == N
        ln, oo, ob = lens.cpu().numpy().astype(np.int64), offs.cpu().numpy(), out.cpu().numpy()
        files[route] = [ob[oo[k]:oo[k] + ln[k]].tobytes() for k in range(args.pil_tiles)]
        plan.append({"name": "gray16_" + route, "calls": calls, "warmup_calls": args.warmup, "tiles": N,
                     "stream_bytes": N * (2 * SIDE + 1) * SIDE, "input_bytes": N * SIDE * SIDE * 2,
                     "file_bytes": int(ln.sum()), "ms_per_call": round(1e3 * med, 4),
                     "tiles_per_s": round(N / med, 1)})
        ctx.close()
    assert files["wave"] == files["workgroup"], "the two filter routes disagree"
    # file sizes beside PIL's encoder on the same pixels (sizes only)
    from PIL import Image
    pil = []
    for k in range(args.pil_tiles):
        a = planes[k].cpu().numpy().view(">u2").astype(np.uint16)
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(files["wave"][k]))).astype(np.uint16), a)
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, format="png")
        pil.append(buf.tell())
    sizes = {"tiles": args.pil_tiles, "raw_bytes": SIDE * SIDE * 2,
             "omr_mean_bytes": int(np.mean([len(f) for f in files["wave"]])), "pil_mean_bytes": int(np.mean(pil))}
    del out, planes, spec
    # the yardstick: batched RGB PNG of 256 rendered C2 tiles (the bench's png.batched case)
    sys.path.insert(0, REPO)
    import bench
    ctx = omr.Context(0, torch_order=False)
    data, _, _ = bench.build_batch(torch, N, 8, dev)
    q, ch = make_qdef("rgb"), c2_channels(4)
    argb = torch.empty((N, SIDE, SIDE), dtype=torch.int32, device=dev)
    pb = SIDE * SIDE * 2
    torch.cuda.synchronize()
    ctx.render_batch_strided_device(q, ch, data, 4 * pb, pb, N, _lib.PIXELS_UINT16, SIDE, SIDE, argb, big_endian=True,
                                    bindings=make_bindings(ch))
    ctx.synchronize()
    out = torch.empty(_lib.lib.omr_png_batch_max_bytes(SIDE, SIDE, 3, N), dtype=torch.uint8, device=dev)
    med = timed(lambda: ctx.encode_png_batch_device(argb, N, SIDE, SIDE, out, offs, lens, stat), ctx)
    assert int((stat == 0).sum().item()) == N
    plan.append({"name": "rgb_c2", "calls": calls, "warmup_calls": args.warmup, "tiles": N,
                 "stream_bytes": N * (3 * SIDE + 1) * SIDE, "input_bytes": N * SIDE * SIDE * 4,
                 "file_bytes": int(lens.cpu().numpy().astype(np.int64).sum()), "ms_per_call": round(1e3 * med, 4),
                 "tiles_per_s": round(N / med, 1)})
    ctx.close()
    with open(args.plan, "w") as fh:
        json.dump({"build_id": bench.kernel_build_id(), "configs": plan,
                   "file_sizes": sizes}, fh, indent=1)
    print(json.dumps({"configs": plan, "file_sizes": sizes}))


def summarize(args):
    plan = json.load(open(args.plan))
    rows = []
    with open(args.trace) as fh:
        for r in csv.DictReader(fh):
            m = re.search(r"k_pngb_[a-z_]+", r["Kernel_Name"])    # plain or mangled names
            if m:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]),
                             m.group(0)))
    rows.sort()
    calls, cur = [], None                     # a call begins at its filter launch
    for _, d, name in rows:
        if name in FILTERS:
            cur = {}
            calls.append(cur)
        if cur is not None:
            cur[name] = cur.get(name, 0) + d
    pos, table = 0, []
    for cfg in plan["configs"]:
        grp = calls[pos + cfg["warmup_calls"]:pos + cfg["calls"]]
        pos += cfg["calls"]
        kernels = {}
        for name in sorted({k for c in grp for k in c}):
            d = sorted(c.get(name, 0) for c in grp)
            kernels[name] = {"median_us": d[len(d) // 2] / 1e3, "p10_us": d[len(d) // 10] / 1e3,
                             "p90_us": d[(len(d) * 9) // 10] / 1e3}
        tot = sorted(sum(c.values()) for c in grp)
        flt = next(kernels[f] for f in FILTERS if f in kernels)
        row = dict(cfg, timed_calls=len(grp), kernels=kernels, kernels_total_us=tot[len(tot) // 2] / 1e3,
                   filter_ps_per_stream_byte={k: round(flt[k + "_us"] * 1e6 / cfg["stream_bytes"], 3)
                                              for k in ("median", "p10", "p90")})
        table.append(row)
        print(f"{cfg['name']}: {cfg['tiles_per_s']} tiles/s wall ({cfg['ms_per_call']} ms per call), kernels "
              f"{row['kernels_total_us']:.1f} us per call, files {cfg['file_bytes'] / cfg['tiles']:.0f} B per tile, "
              f"filter {row['filter_ps_per_stream_byte']} ps per stream byte")
        for name, k in kernels.items():
            print(f"    {name:28s} median {k['median_us']:9.1f} us  (p10 {k['p10_us']:.1f}, p90 {k['p90_us']:.1f})")
    print("file sizes:", plan.get("file_sizes"))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump({"build_id": plan.get("build_id"), "rows": table,
                       "file_sizes": plan.get("file_sizes")}, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--plan", required=True)
    r.add_argument("--passes", type=int, default=32, help="timed calls per configuration")
    r.add_argument("--warmup", type=int, default=1)
    r.add_argument("--pil-tiles", type=int, default=8, help="tiles whose file size is set beside PIL's")
    s = sub.add_parser("summarize")
    s.add_argument("trace")
    s.add_argument("plan")
    s.add_argument("--json", default=None)
    a = ap.parse_args()
    run(a) if a.cmd == "run" else summarize(a)


if __name__ == "__main__":
    main()
