#!/usr/bin/env python3
"""K17 (JPEG-compressed TIFF tiles decoded on the device) on the RGB workload of the K13 probe.

The 8-bit RGB image of tools/tiff_read_probe.py (4096 x 8192, bits 4..11 of the first three
microscopy channels), its 32 tile-aligned 1024^2 positions rendered once each with red / green /
blue bindings by TiffImage.render_tiles, served from

  rgb_jpeg_rst_256     JPEG quality 85, 4:2:0, 256 x 256 tiles, a restart marker per MCU row (16 MCUs)
  rgb_jpeg_256         the same without restart markers: one interval, so one wave, per tile
  rgb_deflate_256      the chunky Deflate + predictor 2 file of the K13 probe (K14a + K13b strided + K2)

Per pass: wall time, and the kernel times of omr_ctx_kernel_timings (36 K17a entropy decode, 37
K17b IDCT, 38 K17c upsample / colour / store, 31 K13b, 2 K2; 32 K14a for the Deflate file), as
medians of the passes after a warm-up with min..max beside them.  CPU figure for the same tiles:
omr_jpeg_decode_host on 16 threads.  The two JPEG files hold the same pixels (restart markers do
not change them), so their renders must be equal; one region is also compared with get_tile.
Needs Pillow to write the files.

    python3 tools/tiff_jpeg_probe.py --json profiles/k17/tiff_jpeg_probe.json

With --split (K18) the two JPEG files are also served with the split entropy decode on every
interval (39 K18a, 40 K18b in place of 36), at the default subsequence size and, for the file
without restart markers, at those of --split-bits; the runs are named FILE+split and
FILE+split_S<bits>, and all are compared with the first run's pixels.

    python3 tools/tiff_jpeg_probe.py --split --json profiles/k18/tiff_jpeg_probe.json
"""
import argparse
import json
import multiprocessing
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "omero-ms-image-region_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from tiff_read_probe import SIDE, build_pixels, segment_table, series   # noqa: E402

TILE = 256


def host_decoder(path, tables):
    """omr_jpeg_decode_host over every tile of the file on 16 threads: seconds."""
    from omr import _lib
    segs = segment_table(path, 1)
    with open(path, "rb") as f:
        blob = np.frombuffer(f.read(), dtype=np.uint8)
    outs = [np.empty(TILE * TILE * 3, dtype=np.uint8) for _ in range(16)]
    tab = np.frombuffer(tables, dtype=np.uint8) if tables else None

    def work(k):
        for off, cnt in segs[k::16]:
            st = _lib.lib.omr_jpeg_decode_host(tab.ctypes.data if tab is not None else None, len(tables or b""),
                                               blob.ctypes.data + off, cnt, TILE, TILE, 3, 1, outs[k].ctypes.data, None, 0)
            assert st == 0
    t0 = time.perf_counter()
    with ThreadPoolExecutor(16) as ex:
        list(ex.map(work, range(16)))
    return time.perf_counter() - t0, len(segs), int(sum(c for _, c in segs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cols", type=int, default=4)
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--split", action="store_true", help="also run the JPEG files with K18 (Context.set_jpeg_split) on every interval")
    ap.add_argument("--split-bits", default="256,4096", help="with --split: further subsequence sizes for the file without restart markers")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import omr
    rgb = np.ascontiguousarray((build_pixels(args.cols, args.rows)[:, :3] >> 4).astype(np.uint8))
    H, W = rgb.shape[3:]
    result = {"image": [W, H], "region": SIDE, "tile": TILE, "passes": args.passes, "raw_bytes": rgb.nbytes, "files": {},
              "runs": {}}
    tmp = tempfile.mkdtemp(prefix="tiff_jpeg_probe_")
    paths = {}
    common = dict(quality=85, subsampling="4:2:0", tables="shared")
    for key, opt in (("rgb_jpeg_rst_256", dict(common, restart_blocks=TILE // 16)), ("rgb_jpeg_256", common)):
        paths[key] = os.path.join(tmp, key + ".tif")
        omr.write_tiled_tiff(paths[key], rgb, tile=(TILE, TILE), compression=7, samples_per_pixel=3, jpeg=opt)
    with multiprocessing.Pool(15) as pool:                       # before the GPU is opened
        paths["rgb_deflate_256"] = os.path.join(tmp, "rgb_deflate_256.tif")
        omr.write_tiled_tiff(paths["rgb_deflate_256"], rgb, tile=(TILE, TILE), compression=8, predictor=2, samples_per_pixel=3,
                             mapper=lambda f, xs: pool.map(f, xs, chunksize=4))
    for key, path in paths.items():
        size = os.path.getsize(path)
        result["files"][key] = {"file_bytes": size, "compression_ratio": rgb.nbytes / size}
    for key in ("rgb_jpeg_rst_256", "rgb_jpeg_256"):
        sys.path.insert(0, os.path.join(REPO, "tests"))
        import tiff_jpeg_cases as jc
        tables = jc.ifd_of(open(paths[key], "rb").read())[347][3]
        walls = []
        for _ in range(args.warmup + args.passes):
            s, n, cbytes = host_decoder(paths[key], tables)
            walls.append(s)
        walls = walls[args.warmup:]
        result["files"][key]["cpu"] = {"segments": n, "compressed_bytes": cbytes, "host_decoder_16_threads_s": series(walls),
                                       "host_decoder_16_threads_gb_s": rgb.nbytes / statistics.median(walls) / 1e9}
    print(json.dumps(result["files"], indent=1), flush=True)

    if not args.cpu_only:
        import torch
        from omr.context import make_bindings, make_qdef
        from omr.synthetic import c2_channels
        q = make_qdef("rgb")
        chans = [dict(c, rgba=col, input_start=0.0, input_end=255.0, global_min=0.0, global_max=255.0)
                 for c, col in zip(c2_channels(3), ((255, 0, 0, 255), (0, 255, 0, 255), (0, 0, 255, 255)))]
        binds = make_bindings(chans)
        positions = [(0, 0, k * SIDE, r * SIDE) for r in range(args.rows) for k in range(args.cols)]
        out = torch.empty((len(positions), SIDE, SIDE), dtype=torch.int32, device="cuda:0")
        region_bytes = len(positions) * 3 * SIDE * SIDE
        accepts = {"rgb_deflate_256": ("deflate", "samples")}
        first = None
        with omr.Context(0) as ctx:
            runs = [("rgb_jpeg_rst_256", None), ("rgb_jpeg_256", None), ("rgb_deflate_256", None)]
            if args.split:                                   # K18 on every interval: the default S, and two others on the file it is for
                runs[2:2] = [("rgb_jpeg_rst_256", 0), ("rgb_jpeg_256", 0)] + [("rgb_jpeg_256", int(b)) for b in args.split_bits.split(",") if b]
            for key, split_bits in runs:
                src = omr.TiffImage(paths[key], 1, 3, 1, accept=accepts.get(key, ("jpeg", "samples")))
                ctx.set_jpeg_split(0 if split_bits is None else 1, split_bits or 0)
                run_key = key if split_bits is None else key + "+split" + ("_S%d" % split_bits if split_bits else "")
                walls, kinds = [], {}
                ctx.enable_kernel_timing(True)
                for p in range(args.warmup + args.passes):
                    ctx.kernel_timings()
                    t0 = time.perf_counter()
                    src.render_tiles(ctx, q, chans, 0, positions, SIDE, SIDE, out=out, bindings=binds)
                    wall = time.perf_counter() - t0
                    tm = ctx.kernel_timings()
                    if p >= args.warmup:
                        walls.append(wall)
                        per = {}
                        for ms, kind in tm:
                            per[kind] = per.get(kind, 0.0) + ms
                        for kind, ms in per.items():
                            kinds.setdefault(kind, []).append(ms)
                        launches = {str(kind): sum(1 for _, k in tm if k == kind) for kind in sorted(per)}
                ctx.enable_kernel_timing(False)
                run = {"requests": len(positions), "wall_s": series(walls),
                       "region_gb_per_s_wall": region_bytes / statistics.median(walls) / 1e9}
                run["launches_per_pass"] = launches              # of the last pass, by timing kind
                for name, kind in (("k17a_entropy", 36), ("k18a_entropy_split", 39), ("k18b_dc_sum", 40), ("k17b_idct", 37),
                                   ("k17c_pixels", 38), ("k14a_inflate", 32), ("k13b_place", 31), ("k2_render", 2)):
                    if kind in kinds:
                        run[name + "_ms_per_pass"] = series(kinds[kind])
                        run[name + "_region_gb_per_s"] = region_bytes / (statistics.median(kinds[kind]) / 1e3) / 1e9
                if 36 in kinds or 39 in kinds:
                    if 36 in kinds:
                        k17 = [a + b + c for a, b, c in zip(kinds[36], kinds[37], kinds[38])]
                        run["k17_abc_ms_per_pass"] = series(k17)
                        run["k17_abc_region_gb_per_s"] = region_bytes / (statistics.median(k17) / 1e3) / 1e9
                    else:
                        k18 = [a + b + c + d for a, b, c, d in zip(kinds[39], kinds[40], kinds[37], kinds[38])]
                        run["k18_ab_k17_bc_ms_per_pass"] = series(k18)
                        run["k18_ab_k17_bc_region_gb_per_s"] = region_bytes / (statistics.median(k18) / 1e3) / 1e9
                    got = out[:8].cpu().numpy()
                    if first is None:
                        first = got
                    run["equals_rgb_jpeg_rst"] = bool(np.array_equal(got, first))
                    dev = src.read_regions(ctx, 0, [(0, 1, 0, 300, 500)], 700, 300).cpu().numpy()[0, :700 * 300]
                    run["read_regions_equals_get_tile"] = bool(dev.tobytes() == src.get_tile(0, 0, 1, 0, 300, 500, 700, 300).tobytes())
                result["runs"][run_key] = run
                src.close()
                print(run_key, json.dumps(run), flush=True)
            ctx.set_jpeg_split(0)
    for p in paths.values():
        os.unlink(p)
    os.rmdir(tmp)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
