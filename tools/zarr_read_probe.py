#!/usr/bin/env python3
"""K14 (OME-Zarr read, zlib chunks inflated on the device) beside K13 and the ROMIO path, in one
session.

The workload of tools/tiff_read_probe.py: 256 C2 requests -- 1024^2, four 16-bit channels,
omr.synthetic.microscopy_u16 pixels -- of one 4096 x 8192 image whose 32 aligned 1024^2 positions
are asked for eight times over, so no group of requests shares a chunk.  The same pixels are
served from

  zlib1_256 / zlib1_512   Zarr, zlib level 1, 256^2 / 512^2 chunks   ZarrImage.render_tiles (K14a + K13b + K2)
  zlib6_256 / zlib6_512   Zarr, zlib level 6                         "
  zraw_256                Zarr, uncompressed 256^2 chunks            " (K13b + K2; K14a is skipped)
  lzw_p2_256 / lzw_p2_512 TIFF, LZW + predictor 2                    TiffImage.render_tiles (K13a + K13b + K2)
  romio                   a ROMIO file                               Context.render_pixel_buffer_tiles

each into device memory, three passes after a warm-up.  Per row: wall time, requests/s, the kernel
times of omr_ctx_kernel_timings (kind 32 K14a, 30 K13a, 31 K13b, 2 K2) with the decoded GB/s they
give, and the compression ratio of the probe's files.  CPU figures for the same chunks: the
library's host decoder (omr_inflate_host) on 16 threads and Python's zlib.decompress on one.

    python3 tools/zarr_read_probe.py --json profiles/k14/zarr_read_probe.json
    python3 tools/zarr_read_probe.py --cpu-only        (files and the CPU figures, no GPU)
"""
import argparse
import json
import multiprocessing
import os
import shutil
import statistics
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "omero-ms-image-region_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from tiff_read_probe import CH, SIDE, build_pixels, cpu_figures, series  # noqa: E402


def chunk_files(group):
    out = []
    for root, _, files in os.walk(os.path.join(group, "0")):
        out += [os.path.join(root, f) for f in files if not f.startswith(".")]
    return sorted(out)


def zarr_cpu_figures(group, chunk, decoded_bytes):
    from omr import _lib
    blobs = [open(p, "rb").read() for p in chunk_files(group)]
    expected = chunk * chunk * 2
    outs = [np.empty(expected, dtype=np.uint8) for _ in range(16)]
    srcs = [np.frombuffer(b, dtype=np.uint8) for b in blobs]

    def work(k):
        out = outs[k]
        for s in srcs[k::16]:
            assert _lib.lib.omr_inflate_host(s.ctypes.data, s.size, out.ctypes.data, expected) == 0
    t0 = time.perf_counter()
    with ThreadPoolExecutor(16) as ex:
        list(ex.map(work, range(16)))
    host = time.perf_counter() - t0
    t0 = time.perf_counter()
    for b in blobs:
        zlib.decompress(b)
    py = time.perf_counter() - t0
    return {"chunks": len(blobs), "compressed_bytes": sum(len(b) for b in blobs),
            "host_decoder_16_threads_s": host, "host_decoder_16_threads_gb_s": decoded_bytes / host / 1e9,
            "python_zlib_1_thread_s": py, "python_zlib_1_thread_gb_s": decoded_bytes / py / 1e9}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cols", type=int, default=4)
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--requests", type=int, default=256)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--procs", type=int, default=15, help="processes that LZW-encode the TIFF files")
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import omr
    from omr import _lib
    pixels = build_pixels(args.cols, args.rows)
    H, W = pixels.shape[3:]
    raw_bytes = pixels.nbytes
    result = {"image": [W, H], "channels": CH, "requests": args.requests, "region": SIDE, "passes": args.passes,
              "raw_bytes": raw_bytes, "files": {}, "runs": {}}
    tmp = tempfile.mkdtemp(prefix="zarr_read_probe_")
    paths = {}
    t0 = time.perf_counter()
    zarr_rows = (("zlib1_256", 256, "zlib", 1), ("zlib1_512", 512, "zlib", 1), ("zlib6_256", 256, "zlib", 6),
                 ("zlib6_512", 512, "zlib", 6), ("zraw_256", 256, None, 1))
    for key, chunk, comp, level in zarr_rows:
        paths[key] = os.path.join(tmp, key + ".zarr")
        omr.write_zarr(paths[key], pixels, chunk=(chunk, chunk), compressor=comp, level=level)
        size = sum(os.path.getsize(p) for p in chunk_files(paths[key]))
        result["files"][key] = {"chunk": chunk, "chunk_bytes": size, "compression_ratio": raw_bytes / size}
    with multiprocessing.Pool(args.procs) as pool:               # before the GPU is opened
        mapper = lambda f, xs: pool.map(f, xs, chunksize=4)      # noqa: E731
        for key, tile in (("lzw_p2_256", 256), ("lzw_p2_512", 512)):
            paths[key] = os.path.join(tmp, key + ".tif")
            omr.write_tiled_tiff(paths[key], pixels, tile=(tile, tile), compression=5, predictor=2, mapper=mapper)
            size = os.path.getsize(paths[key])
            result["files"][key] = {"tile": tile, "file_bytes": size, "compression_ratio": raw_bytes / size}
    paths["romio"] = os.path.join(tmp, "romio.raw")
    omr.write_romio(paths["romio"], pixels, _lib.PIXELS_UINT16)
    result["files_written_s"] = time.perf_counter() - t0
    for key, chunk, comp, level in zarr_rows:
        if comp:
            result["files"][key]["cpu"] = zarr_cpu_figures(paths[key], chunk, raw_bytes)
    for key, tile in (("lzw_p2_256", 256), ("lzw_p2_512", 512)):
        result["files"][key]["cpu"] = cpu_figures(paths[key], tile, CH, raw_bytes)
    print(json.dumps(result["files"], indent=1), flush=True)

    if not args.cpu_only:
        import torch
        from omr.context import make_bindings, make_qdef
        from omr.synthetic import c2_channels
        q, chans = make_qdef("rgb"), c2_channels(CH)
        binds = make_bindings(chans)
        positions = [(0, 0, k * SIDE, r * SIDE) for r in range(args.rows) for k in range(args.cols)]
        reqs = [positions[i % len(positions)] for i in range(args.requests)]
        region_bytes = args.requests * CH * SIDE * SIDE * 2
        out = torch.empty((args.requests, SIDE, SIDE), dtype=torch.int32, device="cuda:0")
        ref = None
        with omr.Context(0) as ctx:
            for key in ["romio"] + [r[0] for r in zarr_rows] + ["lzw_p2_256", "lzw_p2_512"]:
                if key == "romio":
                    src = omr.PixelBuffer(paths[key], W, H, 1, CH, 1, _lib.PIXELS_UINT16)
                    call = lambda: ctx.render_pixel_buffer_tiles(q, chans, src, reqs, SIDE, SIDE, out=out, bindings=binds)  # noqa: E731
                else:
                    src = omr.TiffImage(paths[key], 1, CH, 1) if key.startswith("lzw") else omr.ZarrImage(paths[key])
                    call = lambda: src.render_tiles(ctx, q, chans, 0, reqs, SIDE, SIDE, out=out, bindings=binds)  # noqa: E731
                walls, kinds = [], {}
                ctx.enable_kernel_timing(True)
                for p in range(args.warmup + args.passes):
                    ctx.kernel_timings()
                    t0 = time.perf_counter()
                    call()
                    wall = time.perf_counter() - t0
                    tm = ctx.kernel_timings()
                    if p >= args.warmup:
                        walls.append(wall)
                        per = {}
                        for ms, kind in tm:
                            per[kind] = per.get(kind, 0.0) + ms
                        for kind, ms in per.items():
                            kinds.setdefault(kind, []).append(ms)
                ctx.enable_kernel_timing(False)
                got = out[:32].cpu().numpy()
                if ref is None:
                    ref = got
                run = {"wall_s": series(walls), "requests_per_s": args.requests / statistics.median(walls),
                       "region_gb_per_s_wall": region_bytes / statistics.median(walls) / 1e9,
                       "equals_romio": bool(np.array_equal(got, ref))}
                for name, kind in (("k14a_inflate", 32), ("k13a_lzw_decode", 30), ("k13b_place", 31), ("k2_render", 2)):
                    v = kinds.get(kind)
                    if v:
                        run[name + "_ms_per_pass"] = series(v)
                        run[name + "_region_gb_per_s"] = region_bytes / (statistics.median(v) / 1e3) / 1e9
                result["runs"][key] = run
                src.close()
                print(key, json.dumps(run), flush=True)
        base = result["runs"]["romio"]["requests_per_s"]
        for key, run in result["runs"].items():
            run["requests_per_s_vs_romio"] = run["requests_per_s"] / base
        for lv in (1, 6):
            a, b = result["runs"][f"zlib{lv}_256"], result["runs"][f"zlib{lv}_512"]
            result[f"k14a_zlib{lv}_512_over_256_time"] = (b["k14a_inflate_ms_per_pass"]["median"] /
                                                          a["k14a_inflate_ms_per_pass"]["median"])
    shutil.rmtree(tmp)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
