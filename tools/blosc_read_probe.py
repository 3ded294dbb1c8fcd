#!/usr/bin/env python3
"""K15 (OME-Zarr read, Blosc chunks with their LZ4 streams decoded on the device) beside K14's
zlib-1 and uncompressed rows and the ROMIO path, in one session.

The workload of tools/zarr_read_probe.py: 256 C2 requests -- 1024^2, four 16-bit channels,
omr.synthetic.microscopy_u16 pixels -- of one 4096 x 8192 image whose 32 aligned 1024^2 positions
are asked for eight times over.  The same pixels are served from

  blosc_256 / blosc_512                 Zarr, Blosc-LZ4, byte shuffle, split    ZarrImage.render_tiles (K15a + K15b + K2)
  blosc_nosplit_256 / blosc_nosplit_512 the same with flag 0x10 (do not split)  "
  zlib1_256                             Zarr, zlib level 1, 256^2 chunks        " (K14a + K13b + K2)
  zraw_256                              Zarr, uncompressed 256^2 chunks         " (K13b + K2)
  romio                                 a ROMIO file                            Context.render_pixel_buffer_tiles

each into device memory, three passes after a warm-up.  The Blosc chunks are written by the
product's pure-Python encoder (omr.blosc_encode) with the block size c-blosc would choose as
recalled, not checked against c-blosc: 256 KiB for uint16 at clevel 5, clamped to the chunk, so a
256^2 chunk (128 KiB) is one block of two streams and a 512^2 chunk (512 KiB) two blocks of two.  Per
row: wall time, requests/s, the kernel times of omr_ctx_kernel_timings (kind 33 K15a, 34 K15b, 32
K14a, 31 K13b, 2 K2) with the decoded GB/s they give, and the compression ratio of the probe's
files (every row's ARGB is asserted equal to the ROMIO row's, all 256 outputs).  CPU figures for the
same chunks: omr_blosc_decode_host and omr_inflate_host on 16 threads, the median of five passes
over all chunks after an untimed one that starts the threads.

    python3 tools/blosc_read_probe.py --json profiles/k15/blosc_read_probe.json
    python3 tools/blosc_read_probe.py --cpu-only        (files and the CPU figures, no GPU)
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
from concurrent.futures import ThreadPoolExecutor

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "omero-ms-image-region_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from tiff_read_probe import CH, SIDE, build_pixels, series  # noqa: E402
from zarr_read_probe import chunk_files  # noqa: E402

BLOCK = 256 << 10     # c-blosc's block size for uint16 at clevel 5, as recalled


def _encode_file(job):
    path, split = job
    import omr
    with open(path, "rb") as f:
        raw = f.read()
    with open(path, "wb") as f:
        f.write(omr.blosc_encode(raw, 2, 1, min(BLOCK, len(raw)), split))
    return path


def write_blosc_group(omr, path, pixels, chunk, split, pool):
    """write_zarr's uncompressed group, its chunk files then encoded in place by the pool."""
    omr.write_zarr(path, pixels, chunk=(chunk, chunk), compressor=None)
    pool.map(_encode_file, [(p, split) for p in chunk_files(path)], chunksize=8)
    meta_path = os.path.join(path, "0", ".zarray")
    with open(meta_path) as f:
        meta = json.load(f)
    meta["compressor"] = {"id": "blosc", "cname": "lz4", "clevel": 5, "shuffle": 1, "blocksize": 0}
    with open(meta_path, "w") as f:
        json.dump(meta, f, indent=1)


def cpu_figures(group, chunk, decoded_bytes, fn, passes=5):
    """The host decoder `fn` over all chunk files of `group` on 16 threads: the pool is started and one
    untimed pass run first, then the median of `passes` timed passes (all chunks, in memory)."""
    blobs = [open(p, "rb").read() for p in chunk_files(group)]
    expected = chunk * chunk * 2
    outs = [np.empty(expected, dtype=np.uint8) for _ in range(16)]
    srcs = [np.frombuffer(b, dtype=np.uint8) for b in blobs]

    def work(k):
        out = outs[k]
        for s in srcs[k::16]:
            assert fn(s.ctypes.data, s.size, out.ctypes.data, expected) == 0
    times = []
    with ThreadPoolExecutor(16) as ex:
        list(ex.map(work, range(16)))                            # threads started, buffers touched
        for _ in range(passes):
            t0 = time.perf_counter()
            list(ex.map(work, range(16)))
            times.append(time.perf_counter() - t0)
    host = statistics.median(times)
    return {"chunks": len(blobs), "compressed_bytes": sum(len(b) for b in blobs),
            "host_decoder_16_threads_s": series(times), "host_decoder_16_threads_gb_s": decoded_bytes / host / 1e9}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cols", type=int, default=4)
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--requests", type=int, default=256)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--procs", type=int, default=15, help="processes that encode the Blosc chunks")
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import omr
    from omr import _lib
    pixels = build_pixels(args.cols, args.rows)
    H, W = pixels.shape[3:]
    raw_bytes = pixels.nbytes
    result = {"image": [W, H], "channels": CH, "requests": args.requests, "region": SIDE, "passes": args.passes,
              "raw_bytes": raw_bytes, "blosc_block_bytes": BLOCK, "files": {}, "runs": {}}
    tmp = tempfile.mkdtemp(prefix="blosc_read_probe_")
    paths = {}
    t0 = time.perf_counter()
    blosc_rows = (("blosc_256", 256, None), ("blosc_512", 512, None), ("blosc_nosplit_256", 256, False),
                  ("blosc_nosplit_512", 512, False))
    with multiprocessing.Pool(args.procs) as pool:               # before the GPU is opened
        for key, chunk, split in blosc_rows:
            paths[key] = os.path.join(tmp, key + ".zarr")
            write_blosc_group(omr, paths[key], pixels, chunk, split, pool)
    for key, comp in (("zlib1_256", "zlib"), ("zraw_256", None)):
        paths[key] = os.path.join(tmp, key + ".zarr")
        omr.write_zarr(paths[key], pixels, chunk=(256, 256), compressor=comp, level=1)
    for key in paths:
        files = chunk_files(paths[key])
        size = sum(os.path.getsize(p) for p in files)
        result["files"][key] = {"chunk": 512 if key.endswith("512") else 256, "chunks": len(files), "chunk_bytes": size,
                                "compression_ratio": raw_bytes / size}
    paths["romio"] = os.path.join(tmp, "romio.raw")
    omr.write_romio(paths["romio"], pixels, _lib.PIXELS_UINT16)
    result["files_written_s"] = time.perf_counter() - t0
    for key, chunk, split in blosc_rows:
        with open(chunk_files(paths[key])[0], "rb") as f:
            head = f.read(16)
        result["files"][key]["first_chunk_header"] = {"flags": head[2], "typesize": head[3],
                                                      "blocksize": int.from_bytes(head[8:12], "little")}
        result["files"][key]["cpu"] = cpu_figures(paths[key], chunk, raw_bytes, _lib.lib.omr_blosc_decode_host)
    result["files"]["zlib1_256"]["cpu"] = cpu_figures(paths["zlib1_256"], 256, raw_bytes, _lib.lib.omr_inflate_host)
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
            for key in ["romio"] + [r[0] for r in blosc_rows] + ["zlib1_256", "zraw_256"]:
                if key == "romio":
                    src = omr.PixelBuffer(paths[key], W, H, 1, CH, 1, _lib.PIXELS_UINT16)
                    call = lambda: ctx.render_pixel_buffer_tiles(q, chans, src, reqs, SIDE, SIDE, out=out, bindings=binds)  # noqa: E731
                else:
                    src = omr.ZarrImage(paths[key], codecs=("zlib", "blosc"))
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
                got = out.cpu().numpy()
                if ref is None:
                    ref = got
                assert np.array_equal(got, ref), f"{key}: ARGB differs from the ROMIO row's"
                run = {"wall_s": series(walls), "requests_per_s": args.requests / statistics.median(walls),
                       "region_gb_per_s_wall": region_bytes / statistics.median(walls) / 1e9,
                       "equals_romio": bool(np.array_equal(got, ref))}
                for name, kind in (("k15a_lz4_decode", 33), ("k15b_blosc_place", 34), ("k14a_inflate", 32),
                                   ("k13b_place", 31), ("k2_render", 2)):
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
            for other in ("zlib1_256", "zraw_256"):
                run["requests_per_s_vs_" + other] = run["requests_per_s"] / result["runs"][other]["requests_per_s"]
    shutil.rmtree(tmp)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
