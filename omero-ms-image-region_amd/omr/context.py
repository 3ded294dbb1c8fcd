"""Context: Python handle on one omr_ctx (device + stream + workspace).

Host arrays are numpy; device buffers are torch tensors on the context's GPU (torch is
only used as the device-memory allocator — all compute runs in libomr.so kernels).
"""
import ctypes
import functools

import numpy as np

from . import _lib
from ._lib import lib, check


def _ptr(a):
    """Address of a numpy array, torch tensor, bytes-like or int."""
    if a is None:
        return None
    if isinstance(a, int):
        return a
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    if hasattr(a, "data_ptr"):
        return a.data_ptr()
    raise TypeError(f"cannot take the address of {type(a)}")


def _region(region):
    """omr_region* of (x, y, width, height), or NULL for the whole plane."""
    if region is None:
        return None
    return ctypes.pointer(_lib.Region(*[int(v) for v in region]))


def _info_dict(i):
    return {"lo": i.lo, "hi": i.hi, "below": int(i.below), "above": int(i.above), "nan_count": int(i.nan_count)}


def make_bindings(channels):
    """ChannelBinding[] from a list of dicts / ChannelSettings; keeps LUT buffers alive."""
    n = len(channels)
    arr = (_lib.ChannelBinding * max(n, 1))()
    keep = []
    for i, ch in enumerate(channels):
        d = ch if isinstance(ch, dict) else ch.as_dict()
        b = arr[i]
        b.active = int(bool(d.get("active", True)))
        b.family = int(d.get("family", _lib.FAMILY_LINEAR))
        b.coefficient = float(d.get("coefficient", 1.0))
        b.noise_reduction = int(bool(d.get("noise_reduction", False)))
        b.reverse = int(bool(d.get("reverse", False)))
        b.input_start = float(d["input_start"])
        b.input_end = float(d["input_end"])
        b.global_min = float(d.get("global_min", 0.0))
        b.global_max = float(d.get("global_max", 0.0))
        rgba = d.get("rgba", (255, 0, 0, 255))
        for k in range(4):
            b.rgba[k] = int(rgba[k])
        lut = d.get("lut")
        if lut is not None:
            buf = np.ascontiguousarray(np.asarray(lut, dtype=np.uint8).reshape(768))
            keep.append(buf)
            b.lut = buf.ctypes.data_as(_lib._u8p)
        else:
            b.lut = None
    return arr, keep


def make_qdef(model, cd_start=0, cd_end=255, bit_resolution=255):
    q = _lib.QuantumDef()
    q.cd_start, q.cd_end, q.bit_resolution = cd_start, cd_end, bit_resolution
    q.model = _lib.MODEL_RGB if model in (_lib.MODEL_RGB, "rgb", "c") else _lib.MODEL_GREYSCALE
    return q


def thumbnail_size(size_x, size_y, longest_side=96):
    """(width, height) of a thumbnail by the longest-side rule (omr_thumbnail_size): no upscaling."""
    w, h = ctypes.c_int32(0), ctypes.c_int32(0)
    check(lib.omr_thumbnail_size(int(size_x), int(size_y), int(longest_side), ctypes.byref(w), ctypes.byref(h)))
    return w.value, h.value


def pyramid_level_count(size_x, size_y, min_side=256):
    """Levels (level 0 included) until the longer side is <= min_side (omr_pyramid_level_count)."""
    n = lib.omr_pyramid_level_count(int(size_x), int(size_y), int(min_side))
    if n < 1:
        raise _lib.OmrError(-n, f"pyramid_level_count({size_x}, {size_y}, {min_side})")
    return n


def pyramid_level_sizes(size_x, size_y, n_levels):
    """[[w, h]] of levels 0..n_levels-1, largest first (omr_pyramid_level_sizes)."""
    out = (ctypes.c_int32 * (2 * max(int(n_levels), 1)))()
    check(lib.omr_pyramid_level_sizes(int(size_x), int(size_y), int(n_levels), out))
    return [[out[2 * k], out[2 * k + 1]] for k in range(n_levels)]


class Context:
    """One omr_ctx.  Its launches run on the context's own non-blocking HIP stream.

    torch_order (default True): every *_device call is stream-ordered with torch's current
    stream at the API boundary, without a host sync: the context stream first waits for the
    work torch has queued (the inputs), and torch's stream then waits for the call's kernels
    (the outputs), so a following tensor op (.cpu(), a kernel, a free) sees the result.  Keep
    tensors alive until the call's work is done when torch might reuse their memory (the
    caching allocator reuses on torch's stream, which the second wait orders).  With
    torch_order=False (the bench: explicit synchronize around timed regions) nothing is added
    to a call; order_after_torch() / order_torch_after() do the same by hand."""

    def __init__(self, device=0, torch_order=True):
        h = ctypes.c_void_p()
        st = lib.omr_ctx_create(int(device), ctypes.byref(h))
        if st != _lib.OK:
            raise _lib.OmrError(st, f"omr_ctx_create(device={device}) failed")
        self.h = h
        self.device = device
        self.torch_order = bool(torch_order)
        self._ext = None

    def close(self):
        if self.h:
            lib.omr_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def stream(self):
        return lib.omr_ctx_get_stream(self.h)

    def set_stream(self, stream_ptr):
        check(lib.omr_ctx_set_stream(self.h, stream_ptr), self.h)

    def synchronize(self):
        check(lib.omr_ctx_synchronize(self.h), self.h)

    def _ext_stream(self):
        import torch
        if self._ext is None or self._ext[0] != self.stream:
            self._ext = (self.stream, torch.cuda.ExternalStream(self.stream, device=torch.device("cuda", self.device)))
        return self._ext[1]

    def order_after_torch(self):
        """The context's stream waits for the work queued so far on torch's current stream."""
        import torch
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(torch.device("cuda", self.device)))
        self._ext_stream().wait_event(ev)

    def order_torch_after(self):
        """torch's current stream waits for the work queued so far on the context's stream."""
        import torch
        ev = torch.cuda.Event()
        ev.record(self._ext_stream())
        torch.cuda.current_stream(torch.device("cuda", self.device)).wait_event(ev)

    def set_semantics(self, flags):
        """OMR_SEM_* switches (omr._lib.SEM_*) for later calls on this context."""
        check(lib.omr_ctx_set_semantics(self.h, int(flags)), self.h)

    @property
    def semantics(self):
        return int(lib.omr_ctx_get_semantics(self.h))

    def set_jpeg_split(self, min_interval_bytes, subsequence_bits=0):
        """K18 (omr_ctx_set_jpeg_split): JPEG restart intervals of at least min_interval_bytes
        entropy-coded bytes are decoded by a whole workgroup in subsequences of subsequence_bits bits
        (0: the library's default) in later TIFF reads, renders and jpeg_decode_batch_device calls on
        this context.  min_interval_bytes = 0 or None: off, the default."""
        if not min_interval_bytes:
            check(lib.omr_ctx_set_jpeg_split(self.h, None), self.h)
            return
        opt = _lib.JpegSplitOptions(ctypes.sizeof(_lib.JpegSplitOptions), int(min_interval_bytes), int(subsequence_bits))
        check(lib.omr_ctx_set_jpeg_split(self.h, ctypes.byref(opt)), self.h)

    def enable_kernel_timing(self, enable=True):
        check(lib.omr_ctx_enable_kernel_timing(self.h, int(enable)), self.h)

    def kernel_timings(self, cap=1 << 16):
        """[(ms, kind)] of the timed hot-kernel launches since the last call (kind 2 render,
        3 projection, 4 jpeg, 10 fused scaled render, 11 ARGB scaler, 12 pyramid levels, 20..26 the
        batched PNG stages, 27 the grey wave filter, 30 LZW decode, 31 TIFF place, 36..38 the JPEG decode,
        39 and 40 its split entropy decode and DC sums, 41..43 the JPEG 2000 decode; omr.h has the whole list);
        synchronises the stream."""
        ms = np.zeros(cap, np.float32)
        kind = np.zeros(cap, np.int32)
        n = lib.omr_ctx_kernel_timings(self.h, ms.ctypes.data, kind.ctypes.data, cap)
        if n < 0:
            raise _lib.OmrError(_lib.DEVICE, "kernel timing query failed")
        return list(zip(ms[:n].tolist(), kind[:n].tolist()))

    def last_error(self):
        raw = lib.omr_last_error(self.h)
        return raw.decode() if raw else ""

    # ---- render -----------------------------------------------------------------------
    def render_packed_int(self, qdef, channels, planes, pixel_type, width, height,
                          big_endian=False, flip_h=False, flip_v=False, row_stride=0):
        arr, keep = make_bindings(channels)
        ptrs = (ctypes.c_void_p * max(len(planes), 1))(*[_ptr(p) for p in planes])
        out = np.empty((height, width), dtype=np.uint32)
        check(lib.omr_render_packed_int(self.h, ctypes.byref(qdef), arr, len(channels), ptrs,
                                        row_stride, pixel_type, int(big_endian), width, height,
                                        int(flip_h), int(flip_v), out.ctypes.data), self.h)
        return out

    def render_packed_int_device(self, qdef, channels, planes, pixel_type, width, height, out,
                                 big_endian=False, flip_h=False, flip_v=False, row_stride=0):
        arr, keep = make_bindings(channels)
        ptrs = (ctypes.c_void_p * max(len(planes), 1))(*[_ptr(p) for p in planes])
        check(lib.omr_render_packed_int_device(self.h, ctypes.byref(qdef), arr, len(channels),
                                               ptrs, row_stride, pixel_type, int(big_endian),
                                               width, height, int(flip_h), int(flip_v),
                                               _ptr(out)), self.h)
        return out

    def render_batch_device(self, qdef, channels, d_plane_ptrs, n_tiles, pixel_type, width, height,
                            out, status=None, big_endian=False, flip_h=False, flip_v=False,
                            row_stride=0, bindings=None):
        if bindings is None:
            bindings = make_bindings(channels)
        arr, keep = bindings
        check(lib.omr_render_batch_device(self.h, ctypes.byref(qdef), arr, len(channels),
                                          _ptr(d_plane_ptrs), n_tiles, row_stride, pixel_type,
                                          int(big_endian), width, height, int(flip_h),
                                          int(flip_v), _ptr(out), _ptr(status)), self.h)
        return out

    def render_batch_strided_device(self, qdef, channels, d_base, tile_stride, channel_stride, n_tiles,
                                    pixel_type, width, height, out, status=None, big_endian=False,
                                    flip_h=False, flip_v=False, row_stride=0, bindings=None):
        """Batch whose planes sit at d_base + t*tile_stride + c*channel_stride (bytes)."""
        if bindings is None:
            bindings = make_bindings(channels)
        arr, keep = bindings
        check(lib.omr_render_batch_strided_device(self.h, ctypes.byref(qdef), arr, len(channels),
                                                  _ptr(d_base), tile_stride, channel_stride, n_tiles,
                                                  row_stride, pixel_type, int(big_endian), width,
                                                  height, int(flip_h), int(flip_v), _ptr(out),
                                                  _ptr(status)), self.h)
        return out

    # ---- scaled render: thumbnails, bird's-eye views (K10) ---------------------------------
    pyramid_level_count = staticmethod(pyramid_level_count)
    pyramid_level_sizes = staticmethod(pyramid_level_sizes)

    def pyramid_build_device(self, planes, pixel_type, width, height, levels_out, n_levels, rule=_lib.PYRAMID_MEAN,
                             big_endian=True, row_stride=0):
        """K11 (omr_pyramid_build_device): levels 1..n_levels-1 of the device planes (tensors or
        addresses) into levels_out[k-1], one device buffer per level holding the planes' level-k
        images back to back ([n_planes][h_k][w_k], packed)."""
        ptrs = (ctypes.c_void_p * max(len(planes), 1))(*[_ptr(p) for p in planes])
        outs = (ctypes.c_void_p * max(len(levels_out), 1))(*[_ptr(p) for p in levels_out])
        if len(levels_out) < int(n_levels) - 1:
            raise _lib.OmrError(_lib.INVALID_ARGUMENT, "levels_out shorter than n_levels - 1")
        check(lib.omr_pyramid_build_device(self.h, ptrs if planes else None, len(planes), int(pixel_type),
                                           int(big_endian), int(width), int(height), int(row_stride), int(rule),
                                           int(n_levels), outs if levels_out else None), self.h)
        return levels_out

    def scale_argb_device(self, src, n, src_w, src_h, dst, dst_w, dst_h, row_stride=0, image_stride=0):
        """The scaling rule (exact area-weighted mean, rounded half up; omr.h) on n device ARGB
        images [n][src_h][row_stride] -> dst [n][dst_h][dst_w]."""
        check(lib.omr_scale_argb_device(self.h, _ptr(src), n, src_w, src_h, row_stride, image_stride, _ptr(dst),
                                        dst_w, dst_h), self.h)
        return dst

    def render_scaled_batch_device(self, qdef, channels, d_plane_ptrs, n_tiles, pixel_type, width, height,
                                   out, out_w, out_h, status=None, big_endian=False, flip_h=False, flip_v=False,
                                   row_stride=0, bindings=None):
        """render_batch_device at out_w x out_h: out is [n_tiles][out_h][out_w]."""
        arr, keep = make_bindings(channels) if bindings is None else bindings
        check(lib.omr_render_scaled_batch_device(self.h, ctypes.byref(qdef), arr, len(channels),
                                                 _ptr(d_plane_ptrs), n_tiles, row_stride, pixel_type,
                                                 int(big_endian), width, height, int(flip_h), int(flip_v),
                                                 _ptr(out), _ptr(status), out_w, out_h), self.h)
        return out

    def render_scaled_batch_strided_device(self, qdef, channels, d_base, tile_stride, channel_stride, n_tiles,
                                           pixel_type, width, height, out, out_w, out_h, status=None,
                                           big_endian=False, flip_h=False, flip_v=False, row_stride=0,
                                           bindings=None):
        """render_batch_strided_device at out_w x out_h."""
        arr, keep = make_bindings(channels) if bindings is None else bindings
        check(lib.omr_render_scaled_batch_strided_device(self.h, ctypes.byref(qdef), arr, len(channels),
                                                         _ptr(d_base), tile_stride, channel_stride, n_tiles,
                                                         row_stride, pixel_type, int(big_endian), width, height,
                                                         int(flip_h), int(flip_v), _ptr(out), _ptr(status),
                                                         out_w, out_h), self.h)
        return out

    def render_thumbnail_jpeg_batch_device(self, qdef, channels, d_plane_ptrs, n_tiles, pixel_type, width, height,
                                           out_w, out_h, quality, d_out, d_offsets, d_lengths, d_status=None,
                                           big_endian=False, flip_h=False, flip_v=False, row_stride=0,
                                           bindings=None):
        """Scaled render + JPEG of n_tiles planes sets: files packed in d_out, as
        render_jpeg_batch_device."""
        arr, keep = make_bindings(channels) if bindings is None else bindings
        check(lib.omr_render_thumbnail_jpeg_batch_device(
            self.h, ctypes.byref(qdef), arr, len(channels), _ptr(d_plane_ptrs), n_tiles, row_stride, pixel_type,
            int(big_endian), width, height, int(flip_h), int(flip_v), out_w, out_h, float(quality), _ptr(d_out),
            d_out.numel(), _ptr(d_offsets), _ptr(d_lengths), _ptr(d_status)), self.h)

    def render_pixel_buffer_tiles(self, qdef, channels, pixbuf, requests, width, height, out=None,
                                  flip_h=False, flip_v=False, bindings=None):
        """Pipelined host-fed tiles: requests = [(z, t, x, y)]; out: host numpy [n][h][w] uint32
        (allocated when None) or a device tensor (rendered in place)."""
        if bindings is None:
            bindings = make_bindings(channels)
        arr, keep = bindings
        n = len(requests)
        reqs = (_lib.TileRequest * max(n, 1))(*[_lib.TileRequest(*r) for r in requests])
        on_device = out is not None and hasattr(out, "data_ptr")
        if out is None:
            out = np.empty((n, height, width), dtype=np.uint32)
        check(lib.omr_render_pixel_buffer_tiles(self.h, pixbuf.h, ctypes.byref(qdef), arr, len(channels), reqs, n,
                                                width, height, int(flip_h), int(flip_v), _ptr(out),
                                                int(on_device)), self.h)
        return out

    def flip_argb_device(self, src, dst, width, height, flip_h, flip_v):
        check(lib.omr_flip_argb_device(self.h, _ptr(src), _ptr(dst), width, height, int(flip_h),
                                       int(flip_v)), self.h)

    def flip_mask_device(self, src, dst, width, height, flip_h, flip_v):
        check(lib.omr_flip_mask_device(self.h, _ptr(src), _ptr(dst), width, height, int(flip_h),
                                       int(flip_v)), self.h)

    # ---- projection --------------------------------------------------------------------
    def project_stack(self, stack, pixel_type, size_x, size_y, size_z, algorithm, start, end,
                      stepping=1, big_endian_in=False, big_endian_out=False):
        bpp = _lib.BYTES_PER_PIXEL[pixel_type]
        out = np.empty(size_x * size_y * bpp, dtype=np.uint8)
        check(lib.omr_project_stack(self.h, _ptr(stack), pixel_type, int(big_endian_in), size_x,
                                    size_y, size_z, algorithm, start, end, stepping,
                                    out.ctypes.data, int(big_endian_out)), self.h)
        return out

    def project_stack_device(self, stack, pixel_type, size_x, size_y, size_z, algorithm, start,
                             end, out, stepping=1, big_endian_in=False, big_endian_out=False):
        check(lib.omr_project_stack_device(self.h, _ptr(stack), pixel_type, int(big_endian_in),
                                           size_x, size_y, size_z, algorithm, start, end,
                                           stepping, _ptr(out), int(big_endian_out)), self.h)
        return out

    def project_stacks_device(self, stacks, pixel_type, size_x, size_y, size_z, algorithm, start, end, outs,
                              stepping=1, big_endian_in=False, big_endian_out=False):
        """Several same-geometry stacks projected in one launch (the glue's K3)."""
        n = len(stacks)
        s = (ctypes.c_void_p * max(n, 1))(*[_ptr(x) for x in stacks])
        o = (ctypes.c_void_p * max(n, 1))(*[_ptr(x) for x in outs])
        check(lib.omr_project_stacks_device(self.h, s, n, pixel_type, int(big_endian_in), size_x, size_y, size_z,
                                            algorithm, start, end, stepping, o, int(big_endian_out)), self.h)
        return outs

    def render_projected_device(self, qdef, channels, stacks, pixel_type, size_x, size_y, size_z,
                                algorithm, start, end, out, stepping=1, big_endian=False,
                                flip_h=False, flip_v=False, bindings=None):
        arr, keep = make_bindings(channels) if bindings is None else bindings
        ptrs = (ctypes.c_void_p * max(len(stacks), 1))(*[_ptr(s) for s in stacks])
        check(lib.omr_render_projected_device(self.h, ctypes.byref(qdef), arr, len(channels), ptrs,
                                              pixel_type, int(big_endian), size_x, size_y, size_z,
                                              algorithm, start, end, stepping, int(flip_h),
                                              int(flip_v), _ptr(out)), self.h)
        return out

    # ---- statistics and histograms (K9) --------------------------------------------------
    def _device_planes(self, planes):
        """Device addresses of planes: numpy arrays are uploaded (bytes as they are), tensors and
        addresses used in place.  Returns (ctypes pointer array, tensors to keep alive)."""
        import torch
        keep = []
        for p in planes:
            if isinstance(p, np.ndarray):
                host = np.ascontiguousarray(p).view(np.uint8).reshape(-1)
                p = torch.from_numpy(host).to(torch.device("cuda", self.device))
            keep.append(p)
        return (ctypes.c_void_p * max(len(keep), 1))(*[_ptr(p) for p in keep]), keep

    def plane_stats(self, planes, pixel_type, width, height, big_endian=False, row_stride=0, region=None):
        """[{min, max, count, nan_count}] of each plane's region (omr_plane_stats_device): what
        fills a channel's global_min / global_max when no StatsInfo is at hand."""
        ptrs, keep = self._device_planes(planes)
        n = len(planes)
        out = (_lib.PlaneStats * max(n, 1))()
        check(lib.omr_plane_stats_device(self.h, ptrs, n, pixel_type, int(big_endian), width, height, row_stride,
                                         _region(region), out), self.h)
        return [{"min": s.min, "max": s.max, "count": int(s.count), "nan_count": int(s.nan_count)} for s in out[:n]]

    def histogram(self, planes, pixel_type, width, height, ranges, bins=256, big_endian=False, row_stride=0,
                  region=None):
        """Histograms of each plane's region over ranges = [(lo, hi)] (one pair: every plane):
        (counts[n][bins] uint32, [{lo, hi, below, above, nan_count}]) (omr_histogram_device)."""
        ptrs, keep = self._device_planes(planes)
        n = len(planes)
        ranges = list(ranges)
        if len(ranges) == 2 and not hasattr(ranges[0], "__len__"):
            ranges = [tuple(ranges)]
        if len(ranges) == 1:
            ranges = ranges * n
        if len(ranges) != n:
            raise ValueError("one (lo, hi) per plane")
        lo = (ctypes.c_double * max(n, 1))(*[float(r[0]) for r in ranges])
        hi = (ctypes.c_double * max(n, 1))(*[float(r[1]) for r in ranges])
        counts = np.zeros((n, max(int(bins), 0)), dtype=np.uint32)
        info = (_lib.HistogramInfo * max(n, 1))()
        check(lib.omr_histogram_device(self.h, ptrs, n, pixel_type, int(big_endian), width, height, row_stride,
                                       _region(region), lo, hi, int(bins), counts.ctypes.data, info), self.h)
        return counts, [_info_dict(i) for i in info[:n]]

    def histogram_host(self, plane, pixel_type, width, height, bins=256, range_mode=_lib.HIST_RANGE_TYPE, lo=None,
                       hi=None, big_endian=False, region=None):
        """One host plane through omr_histogram: (counts[bins], info, stats)."""
        plane = np.ascontiguousarray(plane)
        counts = np.zeros(max(int(bins), 0), dtype=np.uint32)
        info, stats = _lib.HistogramInfo(), _lib.PlaneStats()
        check(lib.omr_histogram(self.h, plane.ctypes.data, pixel_type, int(big_endian), width, height,
                                _region(region), int(range_mode), float(lo or 0.0), float(hi or 0.0), int(bins),
                                counts.ctypes.data, ctypes.byref(info), ctypes.byref(stats)), self.h)
        return counts, _info_dict(info), {"min": stats.min, "max": stats.max, "count": int(stats.count),
                                          "nan_count": int(stats.nan_count)}

    # ---- encode ------------------------------------------------------------------------
    def _encode(self, fn, src, *args, cap):
        out = np.empty(cap, dtype=np.uint8)
        n = ctypes.c_size_t(0)
        check(fn(self.h, _ptr(src), *args, out.ctypes.data, cap, ctypes.byref(n)), self.h)
        return out[:n.value].tobytes()

    def encode_jpeg(self, argb, width, height, quality):
        argb = np.ascontiguousarray(argb, dtype=np.uint32)
        return self._encode(lib.omr_encode_jpeg, argb, width, height, float(quality),
                            cap=lib.omr_jpeg_max_bytes(width, height))

    def encode_jpeg_device(self, d_argb, width, height, quality):
        return self._encode(lib.omr_encode_jpeg_device, d_argb, width, height, float(quality),
                            cap=lib.omr_jpeg_max_bytes(width, height))

    def encode_jpeg_batch_device(self, d_argb, n_tiles, width, height, quality, d_out, d_offsets,
                                 d_lengths, d_status=None, tile_stride=0):
        """Async batch encode on the device; files packed in d_out (uint8 tensor)."""
        check(lib.omr_encode_jpeg_batch_device(self.h, _ptr(d_argb), tile_stride, n_tiles, width, height,
                                               float(quality), _ptr(d_out), d_out.numel(), _ptr(d_offsets),
                                               _ptr(d_lengths), _ptr(d_status)), self.h)

    def render_jpeg_batch_strided_device(self, qdef, channels, d_base, tile_stride, channel_stride, n_tiles,
                                         pixel_type, width, height, quality, d_out, d_offsets, d_lengths,
                                         d_status=None, big_endian=False, flip_h=False, flip_v=False, row_stride=0,
                                         bindings=None):
        """Render + JPEG of a strided plane batch in one call (fused F1 kernel where it applies):
        files packed in d_out, as encode_jpeg_batch_device."""
        arr, keep = make_bindings(channels) if bindings is None else bindings
        check(lib.omr_render_jpeg_batch_strided_device(
            self.h, ctypes.byref(qdef), arr, len(channels), _ptr(d_base), tile_stride, channel_stride, n_tiles,
            row_stride, pixel_type, int(big_endian), width, height, int(flip_h), int(flip_v), float(quality),
            _ptr(d_out), d_out.numel(), _ptr(d_offsets), _ptr(d_lengths), _ptr(d_status)), self.h)

    def render_jpeg_device(self, qdef, channels, planes, pixel_type, width, height, quality, big_endian=False,
                           flip_h=False, flip_v=False, row_stride=0, bindings=None):
        """One request in the default format (omr_render_jpeg): device planes (one tensor or
        address per channel, None for an inactive one) -> JPEG bytes."""
        arr, keep = make_bindings(channels) if bindings is None else bindings
        ptrs = (ctypes.c_void_p * max(len(planes), 1))(*[_ptr(p) for p in planes])
        cap = lib.omr_jpeg_max_bytes(width, height)
        out = np.empty(cap, dtype=np.uint8)
        n = ctypes.c_size_t(0)
        check(lib.omr_render_jpeg(self.h, ctypes.byref(qdef), arr, len(channels), ptrs, row_stride, pixel_type,
                                  int(big_endian), width, height, int(flip_h), int(flip_v), float(quality),
                                  out.ctypes.data, cap, ctypes.byref(n)), self.h)
        return out[:n.value].tobytes()

    def render_jpeg_batch_device(self, qdef, channels, d_plane_ptrs, n_tiles, pixel_type, width, height, quality,
                                 d_out, d_offsets, d_lengths, d_status=None, big_endian=False, flip_h=False,
                                 flip_v=False, row_stride=0, bindings=None):
        arr, keep = make_bindings(channels) if bindings is None else bindings
        check(lib.omr_render_jpeg_batch_device(
            self.h, ctypes.byref(qdef), arr, len(channels), _ptr(d_plane_ptrs), n_tiles, row_stride, pixel_type,
            int(big_endian), width, height, int(flip_h), int(flip_v), float(quality), _ptr(d_out), d_out.numel(),
            _ptr(d_offsets), _ptr(d_lengths), _ptr(d_status)), self.h)

    def encode_jpeg_batch(self, d_argb, n_tiles, width, height, quality, cap=None, tile_stride=0):
        """Batch encode device ARGB tiles -> list of JPEG byte strings (one host sync)."""
        if cap is None:
            cap = n_tiles * (width * height + 4096)
        out = np.empty(cap, dtype=np.uint8)
        offs = np.zeros(n_tiles, dtype=np.uint64)
        lens = np.zeros(n_tiles, dtype=np.uint32)
        check(lib.omr_encode_jpeg_batch(self.h, _ptr(d_argb), tile_stride, n_tiles, width, height,
                                        float(quality), out.ctypes.data, cap, offs.ctypes.data,
                                        lens.ctypes.data), self.h)
        return [out[int(o):int(o) + int(n)].tobytes() for o, n in zip(offs, lens)]

    def encode_png(self, argb, width, height):
        argb = np.ascontiguousarray(argb, dtype=np.uint32)
        return self._encode(lib.omr_encode_png, argb, width, height,
                            cap=lib.omr_png_max_bytes(width, height, 3))

    def encode_png_device(self, d_argb, width, height):
        return self._encode(lib.omr_encode_png_device, d_argb, width, height,
                            cap=lib.omr_png_max_bytes(width, height, 3))

    def encode_png_batch_device(self, d_argb, n_tiles, width, height, d_out, d_offsets=None, d_lengths=None,
                                d_status=None, tile_stride=0):
        """Batched PNG of n_tiles device ARGB tiles into d_out (device bytes); asynchronous."""
        check(lib.omr_encode_png_batch_device(self.h, _ptr(d_argb), tile_stride, n_tiles, width, height,
                                              _ptr(d_out), d_out.numel() * d_out.element_size(), _ptr(d_offsets),
                                              _ptr(d_lengths), _ptr(d_status)), self.h)

    def encode_png_gray_batch_device(self, tiles, pixel_type, width, height, d_out, d_offsets=None, d_lengths=None,
                                     d_status=None, big_endian=True):
        """Batched greyscale PNG of raw plane regions (K12).  tiles: [(plane, pitch_px, x, y)] with
        plane a device tensor (or address) of the plane's first pixel; every tile is the width x
        height region at (x, y).  Files into d_out (device bytes) as encode_png_batch_device
        packs them; asynchronous."""
        n = len(tiles)
        tab = (_lib.RawTile * max(n, 1))()
        for i, (plane, pitch, x, y) in enumerate(tiles):
            tab[i].d_plane, tab[i].pitch_px, tab[i].x, tab[i].y = _ptr(plane), int(pitch), int(x), int(y)
        check(lib.omr_encode_png_gray_batch_device(self.h, ctypes.addressof(tab), n, int(pixel_type),
                                                   int(bool(big_endian)), width, height, _ptr(d_out),
                                                   d_out.numel() * d_out.element_size() if d_out is not None else 0,
                                                   _ptr(d_offsets), _ptr(d_lengths), _ptr(d_status)), self.h)

    def render_shape_mask_png_batch(self, masks, cap=None):
        """masks: [(bits, width, height, rgba, flip_h, flip_v)] -> [(status, png bytes)] (host in/out)."""
        n = len(masks)
        keep = [np.frombuffer(bytes(m[0]), dtype=np.uint8).copy() if m[0] is not None else None for m in masks]
        jobs = (_lib.MaskJob * max(n, 1))()
        for i, (m, b) in enumerate(zip(masks, keep)):
            jobs[i].bits = b.ctypes.data if b is not None and b.size else None
            jobs[i].n_bytes = 0 if b is None else b.size
            jobs[i].width, jobs[i].height = int(m[1]), int(m[2])
            jobs[i].rgba[:] = [int(v) for v in m[3]]
            jobs[i].flip_h, jobs[i].flip_v = int(bool(m[4])), int(bool(m[5]))
        if cap is None:
            cap = sum(lib.omr_png_batch_max_bytes(max(1, int(m[1])), max(1, int(m[2])), 1, 1) for m in masks)
        out = np.empty(max(cap, 1), dtype=np.uint8)
        offs = np.zeros(max(n, 1), np.uint64)
        lens = np.zeros(max(n, 1), np.uint32)
        stat = np.zeros(max(n, 1), np.int32)
        check(lib.omr_render_shape_mask_png_batch(self.h, jobs, n, out.ctypes.data, cap, offs.ctypes.data,
                                                  lens.ctypes.data, stat.ctypes.data), self.h)
        return [(int(stat[i]), out[int(offs[i]):int(offs[i]) + int(lens[i])].tobytes() if stat[i] == 0 else b"")
                for i in range(n)]

    def encode_tiff(self, argb, width, height):
        argb = np.ascontiguousarray(argb, dtype=np.uint32)
        return self._encode(lib.omr_encode_tiff, argb, width, height,
                            cap=lib.omr_tiff_max_bytes(width, height))

    def encode_tiff_device(self, d_argb, width, height):
        return self._encode(lib.omr_encode_tiff_device, d_argb, width, height,
                            cap=lib.omr_tiff_max_bytes(width, height))

    def render_shape_mask_png(self, bits, width, height, rgba, flip_h=False, flip_v=False):
        bits = np.frombuffer(bytes(bits), dtype=np.uint8).copy()
        col = (ctypes.c_uint8 * 4)(*[int(v) for v in rgba])
        cap = lib.omr_png_max_bytes(width, height, 1)
        out = np.empty(cap, dtype=np.uint8)
        n = ctypes.c_size_t(0)
        check(lib.omr_render_shape_mask_png(self.h, bits.ctypes.data if bits.size else None,
                                            bits.size, width, height, col, int(flip_h),
                                            int(flip_v), out.ctypes.data, cap, ctypes.byref(n)),
              self.h)
        return out[:n.value].tobytes()


def _torch_ordered(fn):
    """Wrap a *_device method: inputs after torch's queued work, torch after the outputs."""
    @functools.wraps(fn)
    def call(self, *a, **k):
        if self.torch_order:
            self.order_after_torch()
        try:
            return fn(self, *a, **k)
        finally:
            if self.torch_order and self.h:
                self.order_torch_after()
    return call


for _name in [n for n in vars(Context)
              if n.endswith("_device") or n in ("encode_jpeg_batch", "plane_stats", "histogram")]:
    setattr(Context, _name, _torch_ordered(getattr(Context, _name)))
