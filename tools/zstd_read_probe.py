#!/usr/bin/env python3
"""K16 (Blosc-Zstd OME-Zarr chunks, Zstandard frames decoded on the device) beside K15 and K14, in
one session.

The workload of tools/zarr_read_probe.py: C2 requests -- 1024^2, four 16-bit channels,
omr.synthetic.microscopy_u16 pixels -- of one image whose aligned 1024^2 positions are asked for
in turn.  The same pixels are served from

  bzstd1_256 / bzstd1_512   Zarr, Blosc (byte shuffle, split) with Zstd level 1, 256^2 / 512^2 chunks
  bzstd5_256 / bzstd5_512   the same at level 5                     ZarrImage.render_tiles (K16a + K15b + K2)
  blz4_256                  Zarr, Blosc with LZ4 (the project's encoder)          (K15a + K15b + K2)
  zlib1_256                 Zarr, zlib level 1                                    (K14a + K13b + K2)

each into device memory, --passes passes after a warm-up.  The Zstandard frames come from libzstd
(libzstd.so.1 through ctypes) when it loads and from the project's encoder (omr.zstd_encode, which
knows no levels and entropy-codes nothing) otherwise; "zstd_encoder" in the result says which.  Per
row: wall time, requests/s, the kernel times of omr_ctx_kernel_timings (35 K16a, 33 K15a, 32 K14a,
34 K15b, 31 K13b, 2 K2) with the decoded GB/s they give, the compression ratio, and the library's
host decoder on 16 threads over the same chunk files.

    python3 tools/zstd_read_probe.py --json profiles/k16/zstd_read_probe.json
    python3 tools/zstd_read_probe.py --cpu-only        (files and the CPU figures, no GPU)
"""
import argparse
import ctypes
import json
import multiprocessing
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "omero-ms-image-region_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from tiff_read_probe import CH, SIDE, build_pixels, series  # noqa: E402
from zarr_read_probe import chunk_files  # noqa: E402
from blosc_read_probe import BLOCK, cpu_figures  # noqa: E402


def libzstd():
    try:
        z = ctypes.CDLL("libzstd.so.1")
    except OSError:
        return None
    z.ZSTD_compressBound.restype = ctypes.c_size_t
    z.ZSTD_compressBound.argtypes = [ctypes.c_size_t]
    z.ZSTD_compress.restype = ctypes.c_size_t
    z.ZSTD_compress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]
    z.ZSTD_isError.argtypes = [ctypes.c_size_t]
    return z


def _encode_file(job):
    path, cname, level = job
    import omr
    codec = "lz4"
    if cname == "zstd":
        z = libzstd()
        codec = "zstd"
        if z is not None:
            def codec(part):
                cap = z.ZSTD_compressBound(len(part))
                out = ctypes.create_string_buffer(cap)
                n = z.ZSTD_compress(out, cap, bytes(part), len(part), level)
                assert not z.ZSTD_isError(n)
                return out.raw[:n]
    with open(path, "rb") as f:
        raw = f.read()
    with open(path, "wb") as f:
        f.write(omr.blosc_encode(raw, 2, 1, min(BLOCK, len(raw)), None, codec=codec))
    return path


def write_blosc_group(omr, path, pixels, chunk, cname, level, pool):
    """write_zarr's uncompressed group, its chunk files then encoded in place by the pool."""
    omr.write_zarr(path, pixels, chunk=(chunk, chunk), compressor=None)
    pool.map(_encode_file, [(p, cname, level) for p in chunk_files(path)], chunksize=8)
    meta_path = os.path.join(path, "0", ".zarray")
    with open(meta_path) as f:
        meta = json.load(f)
    meta["compressor"] = {"id": "blosc", "cname": cname, "clevel": level, "shuffle": 1, "blocksize": 0}
    with open(meta_path, "w") as f:
        json.dump(meta, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cols", type=int, default=4)
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--requests", type=int, default=256)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--procs", type=int, default=15, help="processes that encode the chunk files")
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import omr
    from omr import _lib
    pixels = build_pixels(args.cols, args.rows)
    H, W = pixels.shape[3:]
    raw_bytes = pixels.nbytes
    result = {"image": [W, H], "channels": CH, "requests": args.requests, "region": SIDE, "passes": args.passes,
              "raw_bytes": raw_bytes, "zstd_encoder": "libzstd" if libzstd() is not None else "omr.zstd_encode",
              "files": {}, "runs": {}}
    tmp = tempfile.mkdtemp(prefix="zstd_read_probe_")
    rows = (("bzstd1_256", 256, "zstd", 1), ("bzstd1_512", 512, "zstd", 1), ("bzstd5_256", 256, "zstd", 5),
            ("bzstd5_512", 512, "zstd", 5), ("blz4_256", 256, "lz4", 5), ("zlib1_256", 256, None, 1))
    paths = {}
    t0 = time.perf_counter()
    with multiprocessing.Pool(args.procs) as pool:               # before the GPU is opened
        for key, chunk, cname, level in rows:
            paths[key] = os.path.join(tmp, key + ".zarr")
            if cname:
                write_blosc_group(omr, paths[key], pixels, chunk, cname, level, pool)
            else:
                omr.write_zarr(paths[key], pixels, chunk=(chunk, chunk), compressor="zlib", level=level)
            size = sum(os.path.getsize(p) for p in chunk_files(paths[key]))
            result["files"][key] = {"chunk": chunk, "chunk_bytes": size, "compression_ratio": raw_bytes / size}
    result["files_written_s"] = time.perf_counter() - t0
    ex = _lib.lib.omr_blosc_decode_host_ex
    for key, chunk, cname, level in rows:
        fn = _lib.lib.omr_inflate_host if not cname else (lambda s, n, d, e: ex(s, n, d, e, 3))
        result["files"][key]["cpu"] = cpu_figures(paths[key], chunk, raw_bytes, fn, passes=3)
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
            for key, chunk, cname, level in rows:
                src = omr.ZarrImage(paths[key], codecs=("zlib", "blosc", "blosc-zstd"))
                walls, kinds = [], {}
                ctx.enable_kernel_timing(True)
                for p in range(args.warmup + args.passes):
                    ctx.kernel_timings()
                    t0 = time.perf_counter()
                    src.render_tiles(ctx, q, chans, 0, reqs, SIDE, SIDE, out=out, bindings=binds)
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
                got = out[:min(32, args.requests)].cpu().numpy()
                if ref is None:
                    ref = got
                run = {"wall_s": series(walls), "requests_per_s": args.requests / statistics.median(walls),
                       "region_gb_per_s_wall": region_bytes / statistics.median(walls) / 1e9,
                       "equals_first_row": bool(np.array_equal(got, ref))}
                for name, kind in (("k16a_zstd_decode", 35), ("k15a_lz4_decode", 33), ("k14a_inflate", 32), ("k15b_place", 34),
                                   ("k13b_place", 31), ("k2_render", 2)):
                    v = kinds.get(kind)
                    if v:
                        run[name + "_ms_per_pass"] = series(v)
                        run[name + "_region_gb_per_s"] = region_bytes / (statistics.median(v) / 1e3) / 1e9
                result["runs"][key] = run
                src.close()
                print(key, json.dumps(run), flush=True)
    shutil.rmtree(tmp)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
