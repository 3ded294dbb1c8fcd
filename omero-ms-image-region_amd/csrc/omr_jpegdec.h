// omr_jpegdec.h — K17: what the host decoder (omr_jpegdec.cpp) and the device decoder
// (omr_jpegdec.hip) of baseline JPEG segments share: the lookup tables as both read them, the
// descriptors the host writes for the kernels, and the arithmetic behind the entropy decode -- the
// islow IDCT of one block and the upsample + colour of one output pixel -- as one set of
// __host__ __device__ functions, so that the two routes cannot differ.
//
// All of it is integer arithmetic.  Products and sums of the IDCT are taken in uint32_t, that is
// modulo 2^32: for every stream an encoder writes they are libjpeg's numbers (jidctint.c, nothing
// comes near 2^31), and for a crafted stream with absurd coefficients they are still defined and
// the same on both routes.
#pragma once

#include "omr_internal.h"

namespace omr {

// One Huffman table.  lut: the 9 leading bits of the window -> length << 8 | symbol, 0 where the
// code is longer than 9 bits (or there is none); the longer codes by the canonical rule: the first
// l bits are a code of length l when they are <= maxcode[l] (-1: no code of that length), and its
// symbol is vals[code + valoff[l]].
struct JpegHuff {
    uint16_t lut[512];
    int32_t maxcode[18];
    int32_t valoff[17];
    uint8_t vals[256];
};
// The tables of one scan, resolved per component (components that name the same table hold copies):
// h[c][0] the DC and h[c][1] the AC table of component c, q[c] its quantisation table in natural order.
struct JpegTables {
    JpegHuff h[3][2];
    uint16_t q[3][64];
};
constexpr size_t kJpegHuffBytes = sizeof(JpegHuff) * 2;      // per component, what K17a keeps in LDS

// One segment for the kernels.  Component 0 has hs x vs blocks per MCU (1x1, 2x1 or 2x2), the
// others one; a single component is always 1x1.  Blocks are numbered per component in raster order
// of its grid (mcux * H across, mcuy * V down), component after component; block b has its 64
// coefficients at coef + 64 * b (int16, natural order, still quantised) and its samples in the
// component's plane, which starts at plane + 64 * (first block of the component) and has rows of
// 8 * mcux * H bytes.
struct JpegSegDesc {
    uint64_t dst_off;        // chunky [h][w][ncomp] bytes in the decoders' destination
    uint64_t coef_off;       // bytes into the workspace, a multiple of 16
    uint64_t plane_off;
    int32_t w, h, ncomp, hs, vs, ycc;
    int32_t mcux, mcuy;
    int32_t tables;          // index of its JpegTables
    int32_t pad;
};
// One restart interval: len entropy-coded bytes at src_off (markers and fill bytes cut off, FF 00
// still stuffed; the host has checked that every FF in it is followed by 00) that hold the MCUs
// [first_mcu, first_mcu + n_mcu) of segment seg, all of them inside the segment's mcux * mcuy.
struct JpegIvDesc {
    uint64_t src_off;
    uint32_t len, seg, first_mcu, n_mcu;
};

__host__ __device__ inline int32_t jpeg_total_blocks(int32_t ncomp, int32_t hs, int32_t vs, int32_t mcux, int32_t mcuy) {
    return mcux * mcuy * (ncomp == 1 ? 1 : hs * vs + (ncomp - 1));
}
// First block of component c and the blocks across its grid.
__host__ __device__ inline int32_t jpeg_comp_base(int32_t c, int32_t hs, int32_t vs, int32_t mcux, int32_t mcuy) {
    return c == 0 ? 0 : mcux * mcuy * (hs * vs + (c - 1));
}

// zigzag position -> natural index
#define OMR_JPEG_ZIGZAG                                                                                          \
    {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,                      \
     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,                      \
     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}

// ---- the IDCT: jidctint.c's islow, CONST_BITS 13, PASS1_BITS 2 ------------------------------------

struct JpegW {               // a 32-bit integer whose sums and products wrap
    uint32_t v;
    __host__ __device__ JpegW() : v(0) {}
    __host__ __device__ JpegW(int32_t x) : v((uint32_t)x) {}
    __host__ __device__ JpegW operator+(JpegW o) const { JpegW r; r.v = v + o.v; return r; }
    __host__ __device__ JpegW operator-(JpegW o) const { JpegW r; r.v = v - o.v; return r; }
    __host__ __device__ JpegW operator*(int32_t c) const { JpegW r; r.v = v * (uint32_t)c; return r; }
    __host__ __device__ JpegW shl(int n) const { JpegW r; r.v = v << n; return r; }
    // (x + 2^(n-1)) >> n, the shift arithmetic
    __host__ __device__ JpegW descale(int n) const {
        const uint32_t s = v + (1u << (n - 1));
        JpegW r;
        r.v = (s >> n) | ((s & 0x80000000u) ? ~(0xFFFFFFFFu >> n) : 0u);
        return r;
    }
    __host__ __device__ int32_t i() const { return (int32_t)v; }
};

__host__ __device__ inline void jpeg_idct_1d(const JpegW in[8], JpegW out[8], int shift) {
    JpegW z2 = in[2], z3 = in[6];
    JpegW z1 = (z2 + z3) * 4433;
    JpegW tmp2 = z1 + z3 * -15137;
    JpegW tmp3 = z1 + z2 * 6270;
    JpegW tmp0 = (in[0] + in[4]).shl(13);
    JpegW tmp1 = (in[0] - in[4]).shl(13);
    const JpegW tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7]; tmp1 = in[5]; tmp2 = in[3]; tmp3 = in[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    JpegW z4 = tmp1 + tmp3;
    const JpegW z5 = (z3 + z4) * 9633;
    tmp0 = tmp0 * 2446; tmp1 = tmp1 * 16819; tmp2 = tmp2 * 25172; tmp3 = tmp3 * 12299;
    z1 = z1 * -7373; z2 = z2 * -20995; z3 = z3 * -16069; z4 = z4 * -3196;
    z3 = z3 + z5; z4 = z4 + z5;
    tmp0 = tmp0 + z1 + z3; tmp1 = tmp1 + z2 + z4; tmp2 = tmp2 + z2 + z3; tmp3 = tmp3 + z1 + z4;
    out[0] = (tmp10 + tmp3).descale(shift); out[7] = (tmp10 - tmp3).descale(shift);
    out[1] = (tmp11 + tmp2).descale(shift); out[6] = (tmp11 - tmp2).descale(shift);
    out[2] = (tmp12 + tmp1).descale(shift); out[5] = (tmp12 - tmp1).descale(shift);
    out[3] = (tmp13 + tmp0).descale(shift); out[4] = (tmp13 - tmp0).descale(shift);
}

// One block: 64 quantised coefficients in natural order times q, columns (descale 11), rows
// (descale 18), + 128, clamped; sample (x, y) to out[y * pitch + x].
__host__ __device__ inline void jpeg_idct_block(const int16_t* coef, const uint16_t* q, uint8_t* out, size_t pitch) {
    int16_t cf[64];                                        // coef is 128-byte aligned, out and pitch 8-byte
    std::memcpy(cf, __builtin_assume_aligned(coef, 16), 128);
    JpegW ws[64];
#pragma unroll
    for (int x = 0; x < 8; ++x) {
        JpegW in[8], o[8];
#pragma unroll
        for (int y = 0; y < 8; ++y) in[y] = JpegW((int32_t)cf[y * 8 + x]) * (int32_t)q[y * 8 + x];
        jpeg_idct_1d(in, o, 11);
#pragma unroll
        for (int y = 0; y < 8; ++y) ws[y * 8 + x] = o[y];
    }
#pragma unroll
    for (int y = 0; y < 8; ++y) {
        JpegW o[8];
        jpeg_idct_1d(ws + y * 8, o, 18);
        uint64_t row = 0;
#pragma unroll
        for (int x = 0; x < 8; ++x) {
            const int32_t s = o[x].i() + 128;
            row |= (uint64_t)(s < 0 ? 0 : s > 255 ? 255 : s) << (8 * x);
        }
        std::memcpy(__builtin_assume_aligned(out + (size_t)y * pitch, 8), &row, 8);   // little-endian hosts and the GPU
    }
}

// ---- upsample and colour --------------------------------------------------------------------------

// Chroma sample at output pixel (x, y) of a component stored at half width (and, v2, half height):
// libjpeg's "fancy" triangle filter (jdsample.c), which it uses when the component is more than two
// samples wide and replaces by plain replication otherwise.  cw x ch: the component's true size,
// ceil(w / 2) x (v2 ? ceil(h / 2) : h); p, pitch: its plane.
__host__ __device__ inline int32_t jpeg_chroma(const uint8_t* p, size_t pitch, int32_t cw, int32_t ch, bool v2, int32_t x,
                                               int32_t y) {
    const int32_t i = x >> 1;
    if (!v2) {
        const uint8_t* r = p + (size_t)y * pitch;
        const int32_t a = r[i];
        if (cw <= 2) return a;
        if (x & 1) return i == cw - 1 ? a : (3 * a + r[i + 1] + 2) >> 2;
        return i == 0 ? a : (3 * a + r[i - 1] + 1) >> 2;
    }
    const int32_t j = y >> 1;
    const uint8_t* near = p + (size_t)j * pitch;
    if (cw <= 2) return near[i];
    int32_t jf = (y & 1) ? j + 1 : j - 1;                  // beyond the first and the last row: the edge row itself
    jf = jf < 0 ? 0 : jf > ch - 1 ? ch - 1 : jf;
    const uint8_t* far = p + (size_t)jf * pitch;
    const int32_t s = 3 * near[i] + far[i];
    if (x & 1) return i == cw - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * near[i + 1] + far[i + 1] + 7) >> 4;
    return i == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * near[i - 1] + far[i - 1] + 8) >> 4;
}

__host__ __device__ inline uint8_t jpeg_clamp8(int32_t v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

// Output pixel (x, y) of a segment, ncomp bytes to out: the samples of the planes, the chroma
// upsampled, and with ycc the conversion of jdcolor.c (16 fractional bits, arithmetic shifts).
__host__ __device__ inline void jpeg_pixel(const JpegSegDesc& S, const uint8_t* planes, int32_t x, int32_t y, uint8_t* out) {
    const size_t pitch0 = (size_t)8 * S.mcux * (S.ncomp == 1 ? 1 : S.hs);
    const int32_t c0 = planes[(size_t)y * pitch0 + x];
    if (S.ncomp == 1) {
        out[0] = (uint8_t)c0;
        return;
    }
    int32_t c12[2];
    const size_t pitch = (size_t)8 * S.mcux;
    for (int c = 1; c < 3; ++c) {
        const uint8_t* p = planes + (size_t)64 * jpeg_comp_base(c, S.hs, S.vs, S.mcux, S.mcuy);
        if (S.hs == 1) c12[c - 1] = p[(size_t)y * pitch + x];
        else c12[c - 1] = jpeg_chroma(p, pitch, (S.w + 1) / 2, S.vs == 2 ? (S.h + 1) / 2 : S.h, S.vs == 2, x, y);
    }
    if (!S.ycc) {
        out[0] = (uint8_t)c0; out[1] = (uint8_t)c12[0]; out[2] = (uint8_t)c12[1];
        return;
    }
    const int32_t cb = c12[0] - 128, cr = c12[1] - 128;
    out[0] = jpeg_clamp8(c0 + ((91881 * cr + 32768) >> 16));
    out[1] = jpeg_clamp8(c0 + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    out[2] = jpeg_clamp8(c0 + ((116130 * cb + 32768) >> 16));
}

// ---- the host half (omr_jpegdec.cpp) --------------------------------------------------------------

struct JpegInterval {
    size_t off, len;         // in the segment's stream
    uint32_t first_mcu, n_mcu;
};
// A segment's header, parsed and checked against what the caller expects of it.
struct JpegPlan {
    int32_t w = 0, h = 0, ncomp = 0, hs = 1, vs = 1, mcux = 0, mcuy = 0;
    JpegTables tables;
    std::vector<JpegInterval> intervals;
    uint32_t forms = 0;      // the OMR_JPEG_FORM_* bits the header and the marker scan show
};
// tables (may be null): the TIFF's JPEGTables stream; src: the segment's.  The frame must be w x h
// with `samples` components.  OMR_INVALID_ARGUMENT with *why naming it: a valid form that is out of
// scope; OMR_INTERNAL: damage (*why says what).  On OMR_OK every interval lies inside src, its MCUs
// inside the frame, and every FF inside an interval is followed by 00.
omr_status jpeg_prepare(const uint8_t* tables, size_t tables_len, const uint8_t* src, size_t len, int32_t w, int32_t h,
                        int32_t samples, JpegPlan& out, std::string* why);
// The workspace of one segment: coefficients, then planes.
inline size_t jpeg_coef_bytes(const JpegPlan& P) {
    return align_up((size_t)128 * (size_t)jpeg_total_blocks(P.ncomp, P.hs, P.vs, P.mcux, P.mcuy), 256);
}
inline size_t jpeg_plane_bytes(const JpegPlan& P) {
    return align_up((size_t)64 * (size_t)jpeg_total_blocks(P.ncomp, P.hs, P.vs, P.mcux, P.mcuy), 256);
}

// K17a, K17b, K17c (omr_jpegdec.hip), all tables in device memory: n_iv intervals of n_seg
// segments whose bytes are at src; coefficients and planes in ws; status[seg] must hold OMR_OK and
// gets OMR_INTERNAL when an interval of the segment is damaged.  max_blocks, max_pixels: the
// largest jpeg_total_blocks and w * h of the segments.
omr_status launch_jpeg_decode(Ctx* ctx, const uint8_t* src, const JpegSegDesc* segs, int32_t n_seg, const JpegIvDesc* ivs,
                              int32_t n_iv, const JpegTables* tables, uint8_t* ws, uint8_t* dst, int32_t* status,
                              int32_t max_blocks, int64_t max_pixels);

}  // namespace omr
