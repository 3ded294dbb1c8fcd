#!/usr/bin/env python3
"""K19 (reversible JPEG 2000 TIFF tiles decoded on the device) on the workload of the K13 / K17 probes.

The image of tools/tiff_read_probe.py (4096 x 8192), its 32 tile-aligned 1024^2 positions rendered
once each by TiffImage.render_tiles, served from two lossless files with 256 x 256 tiles, 64 x 64
code-blocks and OpenJPEG's default five decomposition levels:

  rgb8_j2k_256     bits 4..11 of the first three microscopy channels as 8-bit RGB with the RCT,
                   red / green / blue bindings
  grey16_j2k_256   the first channel as 16-bit grey, one greyscale binding

Per pass: wall time, and the kernel times of omr_ctx_kernel_timings (41 K19a code-blocks, 42 K19b
inverse 5/3 summed over its launches, 43 K19c colour / level shift / store, 31 K13b, 2 K2), as
medians of the passes after a warm-up with min..max beside them.  CPU figures for the same tiles:
omr_j2k_decode_host on 16 threads (one tile per thread at a time) and Pillow's OpenJPEG on one
thread.  One region of each file is also compared with get_tile.  Needs Pillow.

--lossy (K20) serves one file in their place:

  rgb8_j2k97_256   the same 8-bit RGB, irreversible: the 9/7 transform and the ICT, rate-cut to about
                   10 : 1 (Pillow's quality_mode "rates", one layer of 10)

with kind 44 (K20b inverse 9/7) in place of 42, the host decoder through omr_j2k_decode_host_ex,
and the largest error against the source picture in place of equality with it.

    python3 tools/tiff_j2k_probe.py --json profiles/k19/tiff_j2k_probe.json
    python3 tools/tiff_j2k_probe.py --lossy --json profiles/k20/tiff_j2k_probe_lossy.json
"""
import argparse
import io
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


def host_decoder(path, samples, bits):
    """omr_j2k_decode_host_ex over every tile of the file, 16 tiles at a time: seconds."""
    from omr import _lib
    segs = segment_table(path, 1)
    with open(path, "rb") as f:
        blob = np.frombuffer(f.read(), dtype=np.uint8)
    outs = [np.empty(TILE * TILE * samples, dtype=np.uint16 if bits == 16 else np.uint8) for _ in range(16)]

    def work(k):
        for off, cnt in segs[k::16]:
            st = _lib.lib.omr_j2k_decode_host_ex(blob.ctypes.data + off, cnt, TILE, TILE, samples, bits, _lib.J2K_ALLOW_IRREVERSIBLE,
                                                 outs[k].ctypes.data, None, 0)
            assert st == 0
    t0 = time.perf_counter()
    with ThreadPoolExecutor(16) as ex:
        list(ex.map(work, range(16)))
    return time.perf_counter() - t0, len(segs), int(sum(c for _, c in segs))


def pillow_decoder(path):
    """Pillow's OpenJPEG over every tile of the file on one thread: seconds."""
    from PIL import Image
    segs = segment_table(path, 1)
    raw = open(path, "rb").read()
    t0 = time.perf_counter()
    for off, cnt in segs:
        np.asarray(Image.open(io.BytesIO(raw[off:off + cnt])))
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cols", type=int, default=4)
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--lossy", action="store_true", help="K20: one irreversible RGB file at about 10 : 1")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import omr
    px = build_pixels(args.cols, args.rows)
    rgb = np.ascontiguousarray((px[:, :3] >> 4).astype(np.uint8))
    grey = np.ascontiguousarray(px[:, :1])
    H, W = rgb.shape[3:]
    result = {"image": [W, H], "region": SIDE, "tile": TILE, "code_block": 64, "passes": args.passes, "files": {}, "runs": {}}
    tmp = tempfile.mkdtemp(prefix="tiff_j2k_probe_")
    opt = dict(codeblock_size=(64, 64))
    files = {"rgb8_j2k_256": (rgb, 3, 8, dict(opt, mct=1)), "grey16_j2k_256": (grey, 1, 16, opt)}
    if args.lossy:
        files = {"rgb8_j2k97_256": (rgb, 3, 8, dict(opt, mct=1, irreversible=True, quality_mode="rates", quality_layers=[10]))}
    paths = {}
    with multiprocessing.Pool(15) as pool:                       # before the GPU is opened
        for key, (a, n, bits, o) in files.items():
            paths[key] = os.path.join(tmp, key + ".tif")
            omr.write_tiled_tiff(paths[key], a, tile=(TILE, TILE), compression=34712, samples_per_pixel=n, jpeg2000=o,
                                 mapper=lambda f, xs: pool.map(f, xs, chunksize=4))
    for key, (a, n, bits, o) in files.items():
        size = os.path.getsize(paths[key])
        walls, pil = [], []
        for _ in range(args.warmup + args.passes):
            s, count, cbytes = host_decoder(paths[key], n, bits)
            walls.append(s)
            pil.append(pillow_decoder(paths[key]))
        walls, pil = walls[args.warmup:], pil[args.warmup:]
        result["files"][key] = {"raw_bytes": a.nbytes, "file_bytes": size, "compression_ratio": a.nbytes / size,
                                "cpu": {"segments": count, "compressed_bytes": cbytes, "host_decoder_16_threads_s": series(walls),
                                        "host_decoder_16_threads_gb_s": a.nbytes / statistics.median(walls) / 1e9,
                                        "pillow_1_thread_s": series(pil),
                                        "pillow_1_thread_gb_s": a.nbytes / statistics.median(pil) / 1e9}}
    print(json.dumps(result["files"], indent=1), flush=True)

    if not args.cpu_only:
        import torch
        from omr.context import make_bindings, make_qdef
        from omr.synthetic import c2_channels
        positions = [(0, 0, k * SIDE, r * SIDE) for r in range(args.rows) for k in range(args.cols)]
        out = torch.empty((len(positions), SIDE, SIDE), dtype=torch.int32, device="cuda:0")
        with omr.Context(0) as ctx:
            for key, (a, n, bits, o) in files.items():
                if n == 3:
                    q = make_qdef("rgb")
                    chans = [dict(c, rgba=col, input_start=0.0, input_end=255.0, global_min=0.0, global_max=255.0)
                             for c, col in zip(c2_channels(3), ((255, 0, 0, 255), (0, 255, 0, 255), (0, 0, 255, 255)))]
                else:
                    q = make_qdef("greyscale")
                    chans = c2_channels(1)
                binds = make_bindings(chans)
                region_bytes = len(positions) * n * SIDE * SIDE * (bits // 8)
                src = omr.TiffImage(paths[key], 1, n, 1, accept=("jpeg2000", "jpeg2000-lossy", "samples"))
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
                run = {"requests": len(positions), "region_bytes": region_bytes, "wall_s": series(walls),
                       "region_gb_per_s_wall": region_bytes / statistics.median(walls) / 1e9}
                run["launches_per_pass"] = launches              # of the last pass, by timing kind
                for name, kind in (("k19a_t1", 41), ("k19b_idwt53", 42), ("k20b_idwt97", 44), ("k19c_pixels", 43), ("k13b_place", 31), ("k2_render", 2)):
                    if kind in kinds:
                        run[name + "_ms_per_pass"] = series(kinds[kind])
                        run[name + "_region_gb_per_s"] = region_bytes / (statistics.median(kinds[kind]) / 1e3) / 1e9
                k19 = [x + y + z for x, y, z in zip(kinds[41], kinds[44 if args.lossy else 42], kinds[43])]
                run["k19_abc_ms_per_pass"] = series(k19)
                run["k19_abc_region_gb_per_s"] = region_bytes / (statistics.median(k19) / 1e3) / 1e9
                dev = src.read_regions(ctx, 0, [(0, n - 1, 0, 300, 500)], 700, 300).cpu().numpy()[0, :700 * 300 * (bits // 8)]
                run["read_regions_equals_get_tile"] = bool(dev.tobytes() == src.get_tile(0, 0, n - 1, 0, 300, 500, 700, 300).tobytes())
                want = a[0, n - 1, 0, 500:800, 300:1000]
                got = src.get_tile(0, 0, n - 1, 0, 300, 500, 700, 300)
                if args.lossy:
                    run["get_tile_max_error_against_source"] = int(np.abs(got.astype(np.int64) - want.astype(np.int64)).max())
                else:
                    run["get_tile_equals_source"] = bool(np.array_equal(got, want))
                result["runs"][key] = run
                src.close()
                print(key, json.dumps(run), flush=True)
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
