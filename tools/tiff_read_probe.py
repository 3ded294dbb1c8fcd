#!/usr/bin/env python3
"""K13 (tiled TIFF read, LZW decoded on the device) against the ROMIO host-fed path.

256 C2 requests -- 1024^2, four 16-bit channels, omr.synthetic.microscopy_u16 pixels -- of one
4096 x 8192 image whose 32 tile-aligned 1024^2 positions are asked for eight times over, so every
group of 32 requests the library works off shares no segment and a pass decodes the full 2 GiB.
The same pixels are served from

  lzw_p2_256   LZW + predictor 2, 256 x 256 tiles      TiffImage.render_tiles (K13a + K13b + K2)
  lzw_p2_512   LZW + predictor 2, 512 x 512 tiles      "
  raw_256      uncompressed 256 x 256 tiles            " (K13b + K2; K13a is skipped)
  deflate_p2_256  Deflate (zlib level 6) + predictor 2, 256 x 256 tiles   " (K14a + K13b + K2), opened with accept
  zstd_p2_256     zstd (libzstd level 3) + predictor 2, 256 x 256 tiles   " (K16a + K13b + K2); skipped without libzstd.so.1
  romio        a ROMIO file                            Context.render_pixel_buffer_tiles

each into device memory, and the RGB variant of the run: bits 4..11 of the first three channels as
an 8-bit image (noisy low bits, as hard for the coders as the 16-bit files), the 32 positions once
each (a group of the renderer holds 85 such requests, so repeats would share their segments and be
decoded once) with red / green / blue bindings, served from

  rgb_lzw_planes_256  three IFDs per plane position, LZW + predictor 2        (K13a + K13b + K2)
  rgb_deflate_256     one chunky IFD of three samples, Deflate + predictor 2  (K14a + K13b strided + K2):
                      every segment is read and inflated once and placed three times

Per pass: wall time, requests/s, and the kernel times of omr_ctx_kernel_timings (kind 30 K13a, 32
K14a, 35 K16a, 31 K13b, 2 K2) with the decoded GB/s they give.  CPU figures for the same segments:
the library's host decoder (omr_lzw_decode_host, omr_inflate_host, omr_zstd_decode_host) on 16
threads, and Pillow / libtiff decoding the same file frame by frame on one thread.

    python3 tools/tiff_read_probe.py --json profiles/k13/tiff_read_probe.json
    python3 tools/tiff_read_probe.py --cpu-only        (files and the CPU figures, no GPU)
"""
import argparse
import json
import multiprocessing
import os
import statistics
import struct
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "omero-ms-image-region_amd"))

CH, SIDE = 4, 1024


def build_pixels(cols, rows):
    """[1][4][1][rows*1024][cols*1024] uint16: eight microscopy tiles, shifted per position and channel."""
    from omr.synthetic import microscopy_u16
    rng = np.random.default_rng(13)
    base = [microscopy_u16(SIDE, SIDE, rng) for _ in range(8)]
    a = np.empty((1, CH, 1, rows * SIDE, cols * SIDE), dtype=np.uint16)
    for c in range(CH):
        for r in range(rows):
            for k in range(cols):
                p = r * cols + k
                a[0, c, 0, r * SIDE:(r + 1) * SIDE, k * SIDE:(k + 1) * SIDE] = \
                    np.roll(base[(p + 3 * c) % 8], (37 * p + 11, 91 * c + 5), (0, 1))
    return a


def segment_table(path, n_planes):
    """[(offset, count)] of every level-0 segment of a classic little-endian tiled TIFF."""
    out = []
    with open(path, "rb") as f:
        raw = f.read(8)
        ifd = struct.unpack("<I", raw[4:])[0]
        for _ in range(n_planes):
            f.seek(ifd)
            n = struct.unpack("<H", f.read(2))[0]
            ent = f.read(12 * n + 4)
            tags = {}
            for k in range(n):
                t, typ, cnt, val = struct.unpack_from("<HHII", ent, 12 * k)
                tags[t] = (cnt, val)
            arrays = []
            for tag in (324, 325):
                cnt, val = tags[tag]
                f.seek(val)
                arrays.append(struct.unpack("<%dI" % cnt, f.read(4 * cnt)))
            out += list(zip(*arrays))
            ifd = struct.unpack_from("<I", ent, 12 * n)[0]
    return out


def libzstd():
    """libzstd.so.1 through ctypes, or None: the project's own zstd_encode stores noisy tiles raw."""
    import ctypes
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


def zstd_level3(raw):
    import ctypes
    z = libzstd()
    cap = z.ZSTD_compressBound(len(raw))
    out = ctypes.create_string_buffer(cap)
    n = z.ZSTD_compress(out, cap, raw, len(raw), 3)
    assert not z.ZSTD_isError(n)
    return out.raw[:n]


def cpu_figures(path, expected, n_planes, decoded_bytes, decoder="omr_lzw_decode_host"):
    from omr import _lib
    segs = segment_table(path, n_planes)
    with open(path, "rb") as f:
        blob = np.frombuffer(f.read(), dtype=np.uint8)
    outs = [np.empty(expected, dtype=np.uint8) for _ in range(16)]
    decode = getattr(_lib.lib, decoder)

    def work(k):
        out = outs[k]
        for off, cnt in segs[k::16]:
            st = decode(blob.ctypes.data + off, cnt, out.ctypes.data, expected)
            assert st == 0
    t0 = time.perf_counter()
    with ThreadPoolExecutor(16) as ex:
        list(ex.map(work, range(16)))
    host = time.perf_counter() - t0
    res = {"segments": len(segs), "compressed_bytes": int(sum(c for _, c in segs)),
           "host_decoder_16_threads_s": host, "host_decoder_16_threads_gb_s": decoded_bytes / host / 1e9}
    try:
        from PIL import Image, features
        if not features.check("libtiff"):
            raise ImportError("Pillow without libtiff")
        Image.MAX_IMAGE_PIXELS = None
        t0 = time.perf_counter()
        with Image.open(path) as im:
            for k in range(n_planes):
                im.seek(k)
                im.load()
        lt = time.perf_counter() - t0
        res.update({"libtiff_1_thread_s": lt, "libtiff_1_thread_gb_s": decoded_bytes / lt / 1e9})
    except Exception as e:                                     # not measured
        res["libtiff"] = f"not measured: {e}"
    return res


def series(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cols", type=int, default=4)
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--requests", type=int, default=256)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--procs", type=int, default=15, help="processes that LZW-encode the probe's files")
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--only", default=None, help="comma-separated run keys (romio and rgb_lzw_planes_256 are the references)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import omr
    from omr import _lib
    pixels = build_pixels(args.cols, args.rows)
    H, W = pixels.shape[3:]
    raw_bytes = pixels.nbytes
    result = {"image": [W, H], "channels": CH, "requests": args.requests, "region": SIDE, "passes": args.passes,
              "raw_bytes": raw_bytes, "files": {}, "runs": {}}
    tmp = tempfile.mkdtemp(prefix="tiff_read_probe_")
    paths = {}
    t0 = time.perf_counter()
    with multiprocessing.Pool(args.procs) as pool:               # before the GPU is opened
        mapper = lambda f, xs: pool.map(f, xs, chunksize=4)      # noqa: E731
        rgb = np.ascontiguousarray((pixels[:, :3] >> 4).astype(np.uint8))
        wanted = lambda key: args.only is None or key in args.only.split(",")  # noqa: E731
        variants = [("lzw_p2_256", 256, 5, pixels, 1, None), ("lzw_p2_512", 512, 5, pixels, 1, None),
                    ("raw_256", 256, 1, pixels, 1, None), ("deflate_p2_256", 256, 8, pixels, 1, None),
                    ("zstd_p2_256", 256, 50000, pixels, 1, zstd_level3),
                    ("rgb_lzw_planes_256", 256, 5, rgb, 1, None), ("rgb_deflate_256", 256, 8, rgb, 3, None)]
        for key, tile, comp, px, spp, encoder in variants:
            if not wanted(key):
                continue
            if comp == 50000 and libzstd() is None:
                result["files"][key] = "not measured: no libzstd.so.1 to write the file with"
                continue
            paths[key] = os.path.join(tmp, key + ".tif")
            omr.write_tiled_tiff(paths[key], px, tile=(tile, tile), compression=comp, predictor=1 if comp == 1 else 2,
                                 mapper=mapper, samples_per_pixel=spp, encoder=encoder)
            size = os.path.getsize(paths[key])
            result["files"][key] = {"tile": tile, "file_bytes": size, "compression_ratio": px.nbytes / size}
    if wanted("romio"):
        paths["romio"] = os.path.join(tmp, "romio.raw")
        omr.write_romio(paths["romio"], pixels, _lib.PIXELS_UINT16)
    result["files_written_s"] = time.perf_counter() - t0
    for key, expected, planes, nbytes, decoder in (
            ("lzw_p2_256", 256 * 256 * 2, CH, raw_bytes, "omr_lzw_decode_host"),
            ("lzw_p2_512", 512 * 512 * 2, CH, raw_bytes, "omr_lzw_decode_host"),
            ("deflate_p2_256", 256 * 256 * 2, CH, raw_bytes, "omr_inflate_host"),
            ("zstd_p2_256", 256 * 256 * 2, CH, raw_bytes, "omr_zstd_decode_host"),
            ("rgb_lzw_planes_256", 256 * 256, 3, rgb.nbytes, "omr_lzw_decode_host"),
            ("rgb_deflate_256", 256 * 256 * 3, 1, rgb.nbytes, "omr_inflate_host")):
        if key in paths:
            result["files"][key]["cpu"] = cpu_figures(paths[key], expected, planes, nbytes, decoder)
    print(json.dumps(result["files"], indent=1), flush=True)

    if not args.cpu_only:
        import torch
        from omr.context import make_bindings, make_qdef
        from omr.synthetic import c2_channels
        q, chans = make_qdef("rgb"), c2_channels(CH)
        binds = make_bindings(chans)
        rgb_chans = [dict(c, rgba=col, input_start=0.0, input_end=255.0, global_min=0.0, global_max=255.0)
                     for c, col in zip(c2_channels(3), ((255, 0, 0, 255), (0, 255, 0, 255), (0, 0, 255, 255)))]
        rgb_binds = make_bindings(rgb_chans)
        positions = [(0, 0, k * SIDE, r * SIDE) for r in range(args.rows) for k in range(args.cols)]
        reqs = [positions[i % len(positions)] for i in range(args.requests)]
        out = torch.empty((args.requests, SIDE, SIDE), dtype=torch.int32, device="cuda:0")
        ref = rgb_ref = None
        accepts = {"deflate_p2_256": ("deflate",), "zstd_p2_256": ("zstd",), "rgb_deflate_256": ("deflate", "samples")}
        with omr.Context(0) as ctx:
            for key in ("romio", "lzw_p2_256", "lzw_p2_512", "raw_256", "deflate_p2_256", "zstd_p2_256",
                        "rgb_lzw_planes_256", "rgb_deflate_256"):
                if key not in paths:
                    continue
                is_rgb = key.startswith("rgb_")
                n_req = len(positions) if is_rgb else args.requests
                region_bytes = n_req * (3 * SIDE * SIDE if is_rgb else CH * SIDE * SIDE * 2)
                if key == "romio":
                    src = omr.PixelBuffer(paths[key], W, H, 1, CH, 1, _lib.PIXELS_UINT16)
                    call = lambda: ctx.render_pixel_buffer_tiles(q, chans, src, reqs, SIDE, SIDE, out=out, bindings=binds)  # noqa: E731
                elif is_rgb:
                    src = omr.TiffImage(paths[key], 1, 3, 1, accept=accepts.get(key, ()))
                    call = lambda: src.render_tiles(ctx, q, rgb_chans, 0, positions, SIDE, SIDE, out=out, bindings=rgb_binds)  # noqa: E731
                else:
                    src = omr.TiffImage(paths[key], 1, CH, 1, accept=accepts.get(key, ()))
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
                            kinds.setdefault(("pass", kind), []).append(ms)
                ctx.enable_kernel_timing(False)
                got = out[:32].cpu().numpy()
                if is_rgb:
                    if rgb_ref is None:
                        rgb_ref = got
                    same = {"equals_rgb_lzw_planes": bool(np.array_equal(got, rgb_ref))}
                else:
                    if ref is None:
                        ref = got
                    same = {"equals_romio": bool(np.array_equal(got, ref))}
                run = {"requests": n_req, "wall_s": series(walls), "requests_per_s": n_req / statistics.median(walls),
                       "region_gb_per_s_wall": region_bytes / statistics.median(walls) / 1e9}
                run.update(same)
                for name, kind in (("k13a_lzw_decode", 30), ("k14a_inflate", 32), ("k16a_zstd_decode", 35),
                                   ("k13b_place", 31), ("k2_render", 2)):
                    v = kinds.get(("pass", kind))
                    if v:
                        run[name + "_ms_per_pass"] = series(v)
                        run[name + "_region_gb_per_s"] = region_bytes / (statistics.median(v) / 1e3) / 1e9
                result["runs"][key] = run
                src.close()
                print(key, json.dumps(run), flush=True)
        if "romio" in result["runs"]:
            base = result["runs"]["romio"]["requests_per_s"]
            for key in ("lzw_p2_256", "lzw_p2_512", "raw_256", "deflate_p2_256", "zstd_p2_256"):
                if key in result["runs"]:
                    result["runs"][key]["requests_per_s_vs_romio"] = result["runs"][key]["requests_per_s"] / base
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
