// omr_jpegdec.h — K17: what the host decoder (omr_jpegdec.cpp) and the device decoder
// (omr_jpegdec.hip) of baseline JPEG segments share: the lookup tables as both read them, the
// descriptors the host writes for the kernels, and the arithmetic behind the entropy decode -- the
// islow IDCT of one block and the upsample + colour of one output pixel -- as one set of
// __host__ __device__ functions, so that the two routes cannot differ.  K18 adds, in the same way,
// one lane of the split entropy decode (k_jpeg_entropy_split and its host emulation).
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

// ---- K18: one lane of the split entropy decode ----------------------------------------------------
//
// The self-synchronising parallel Huffman decode (Weissenberger and Schmidt, ICPP 2018, and its
// JPEG form of 2021): an interval is cut into subsequences of S bits, one lane decodes one
// subsequence from a guessed state, lanes then adopt their predecessor's exit state until nothing
// changes, and a last pass writes the coefficients.  Here is what one lane does, for the kernel
// (k_jpeg_entropy_split, omr_jpegdec.hip) and for the host emulation (omr_jpeg_decode_host_split,
// omr_jpegdec.cpp) alike.
//
// Stuffing: subsequences are cut over the RAW bytes and the 00 behind an FF is dropped on the fly.
// A position is a raw bit position in the interval; no position a lane records lies inside a
// stuffed 00 (the bit behind the last bit of an FF is the first bit of the byte behind its 00), and
// a lane that is told to begin on a stuffed 00 skips it, so the positions of two lanes that stand
// at the same bit are equal.

constexpr uint32_t kJpegSplitLanes = 256;                  // K18a's workgroup
constexpr uint32_t kJpegSplitDefaultBits = 1024;
constexpr uint32_t kJpegSplitMaxLen = 1u << 27;            // longer intervals stay with K17a: 8 * len + a round fits 32 bits

// Where a lane stands.  meta: k (zigzag index inside the current block, 0: before a DC code) |
// blk << 8 (the block inside its MCU) | kJpegLaneStop when the interval ran out of bits there (the
// soft stop).  A lane that starts from a stopped state decodes nothing.
struct JpegLaneState {
    uint32_t pos, meta;
};
constexpr uint32_t kJpegLaneStop = 1u << 16;
__host__ __device__ inline bool operator==(const JpegLaneState& a, const JpegLaneState& b) { return a.pos == b.pos && a.meta == b.meta; }
__host__ __device__ inline bool operator!=(const JpegLaneState& a, const JpegLaneState& b) { return !(a == b); }
// What a lane records: its exit state, the blocks it finished (a soft stop lies in block `blocks`
// of its own) and in which of its blocks it met its FIRST hard error (no such code, k past 63, a DC
// category above 11, an AC category above 10), kJpegLaneNoError if none.
//
// A hard error does not end a lane's decode.  A lane that started from a guess runs into one soon
// where the blocks are long -- its zigzag index is off, so it leaves the block -- and had it to stop
// there, it could never fall into step with the true decode and its successors would have to wait
// for the true state to reach them one lane per iteration.  So the lane notes the error, takes the
// block to end there (behind an unknown code it skips one bit) and goes on; what it decodes from
// there on is a guess again.  For the lanes in their final, true states this changes nothing that
// counts: the first of them with an error has met it where the serial decoder meets it, at ordinal
// first + err, and everything behind that ordinal -- its own later blocks, the lanes after it -- is
// either behind a failure (ordinal below the interval's total: OMR_INTERNAL) or behind the total.
struct JpegLaneRun {
    JpegLaneState exit;
    uint32_t blocks, err;
};
constexpr uint32_t kJpegLaneNoError = 0xFFFFFFFFu;

// The bit window of a lane: the next 57..64 bits at the top of acc, un-stuffed; mark has a one at
// the last bit of every FF in it, so that taking bits steps pos over the stuffed 00 behind it.
struct JpegLaneBits {
    const uint8_t* src;
    uint32_t len, p, pos;    // p: the next raw byte to load; pos: the raw bit position of the window's first bit
    uint64_t acc, mark;
    int nbits, fake;         // fake: zero bits behind the interval's last byte, all at the bottom
    __host__ __device__ void fill() {
        while (nbits <= 56) {
            uint32_t b = 0;
            if (p < len) {
                b = src[p++];
                if (b == 0xFFu && p < len) {               // its stuffed 00 (jpeg_prepare checked it)
                    ++p;
                    mark |= 1ull << (56 - nbits);
                }
            } else {
                fake += 8;
            }
            acc |= (uint64_t)b << (56 - nbits);
            nbits += 8;
        }
    }
    __host__ __device__ void drop(int n) {                 // n in [1, 16], n <= nbits - fake
        pos += (uint32_t)n + 8u * (uint32_t)__builtin_popcountll(mark >> (64 - n));
        acc <<= n;
        mark <<= n;
        nbits -= n;
    }
    // At raw bit position at (any value): nothing is read outside src[0, len).
    __host__ __device__ void open(const uint8_t* s, uint32_t l, uint32_t at) {
        src = s; len = l; acc = mark = 0; nbits = fake = 0;
        uint32_t b0 = at >> 3;
        const int o = (int)(at & 7u);
        if (b0 >= l) {
            p = l; pos = 8u * l;
            return;
        }
        if (o == 0 && b0 > 0u && s[b0] == 0u && s[b0 - 1u] == 0xFFu) ++b0;   // it begins on a stuffed 00
        p = b0; pos = 8u * b0;
        fill();
        if (o && b0 < l) drop(o);                          // (b0 == l: the 00 was the last byte)
    }
    __host__ __device__ bool take(int n, uint32_t& v) {    // n in [0, 16]
        if (nbits < 32) fill();
        if (nbits - fake < n) return false;
        v = n ? (uint32_t)(acc >> (64 - n)) : 0u;
        if (n) drop(n);
        return true;
    }
};

// One symbol of table H (K17a's lookup); -1: no such code, -2: the interval ends inside it.
__host__ __device__ inline int jpeg_lane_symbol(JpegLaneBits& B, const JpegHuff* H) {
    if (B.nbits < 32) B.fill();
    const uint32_t peek = (uint32_t)(B.acc >> 48);
    int len = 0, sym = 0;
    const uint32_t e = H->lut[peek >> 7];
    if (e) {
        len = (int)(e >> 8);
        sym = (int)(e & 255u);
    } else {
        for (int l = 10; l <= 16; ++l) {
            const int32_t code = (int32_t)(peek >> (16 - l));
            if (code <= H->maxcode[l]) {
                const int32_t idx = code + H->valoff[l];
                if (idx < 0 || idx > 255) return -1;
                len = l;
                sym = H->vals[idx];
                break;
            }
        }
        if (!len) return B.nbits - B.fake < 16 ? -2 : -1;
    }
    if (len < 1 || len > 16) return -1;                    // (a table always gives 1..16)
    if (B.nbits - B.fake < len) return -2;
    B.drop(len);
    return sym;
}

__host__ __device__ inline int32_t jpeg_extend(uint32_t v, int s) {
    return v < (1u << (s - 1)) ? (int32_t)v - (1 << s) + 1 : (int32_t)v;
}

// A lane's decode of src[0, len) from `start` up to the first symbol boundary at or behind raw bit
// `end`, the end of the bits or `max_blocks` finished blocks, whichever comes first (and, with
// kWrite, its first hard error).  huff: the tables as K17a keeps them (component c: huff[2 c] DC,
// huff[2 c + 1] AC); zz: zigzag -> natural; b0: the blocks of component 0 in an MCU, bpm: the
// blocks of an MCU.  With kWrite, put(b, natural index, value) gets every non-zero AC coefficient
// and non-zero DC DIFFERENCE of the lane's block b (0: the one `start` stands in).  Every turn of
// the loop takes at least one bit (a symbol does; behind an unknown code one bit is skipped), so it
// ends after at most end - start.pos + 1 turns, and 8 * len whatever the arguments are.
template <bool kWrite, class Put>
__host__ __device__ inline JpegLaneRun jpeg_lane_decode(const uint8_t* src, uint32_t len, const JpegHuff* huff, const uint8_t* zz,
                                                        uint32_t b0, uint32_t bpm, JpegLaneState start, uint32_t end,
                                                        uint32_t max_blocks, Put put) {
    JpegLaneRun R{start, 0u, kJpegLaneNoError};
    if (start.meta & kJpegLaneStop) return R;
    uint32_t k = start.meta & 255u, blk = (start.meta >> 8) & 255u;
    if (k > 63u || blk >= bpm) {                           // no state a lane records
        R.exit = JpegLaneState{8u * len, kJpegLaneStop};
        R.err = 0u;
        return R;
    }
    JpegLaneBits B;
    B.open(src, len, start.pos);
    bool stop = false;
    while (B.pos < end && R.blocks < max_blocks) {
        const uint32_t c = blk < b0 ? 0u : blk - b0 + 1u;
        uint32_t v = 0;
        bool hard = false;
        if (k == 0u) {
            const int s = jpeg_lane_symbol(B, huff + 2u * c);
            if (s == -2) { stop = true; break; }
            if (s < 0 || s > 11) {
                hard = true;
                if (s < 0 && !B.take(1, v)) { stop = true; break; }
            } else {
                if (!B.take(s, v)) { stop = true; break; }
                if (kWrite && s) {
                    const int32_t d = jpeg_extend(v, s);
                    if (d) put(R.blocks, 0u, d);
                }
                k = 1u;
            }
        } else {
            const int rs = jpeg_lane_symbol(B, huff + 2u * c + 1u);
            if (rs == -2) { stop = true; break; }
            const uint32_t r = (uint32_t)rs >> 4;
            const int s = rs & 15;
            if (rs < 0) {
                hard = true;
                if (!B.take(1, v)) { stop = true; break; }
            } else if (s == 0) {
                if (r != 15u) k = 64u;                     // EOB
                else if ((k += 16u) > 63u) hard = true;
            } else {
                k += r;
                if (k > 63u || s > 10) {
                    hard = true;
                } else {
                    if (!B.take(s, v)) { stop = true; break; }
                    if (kWrite) put(R.blocks, (uint32_t)zz[k], jpeg_extend(v, s));
                    ++k;
                }
            }
        }
        if (hard) {
            if (R.err == kJpegLaneNoError) R.err = R.blocks;
            if (kWrite) break;                             // the write pass has nothing to add behind it
            k = 64u;                                       // the block is taken to end here
        }
        if (k >= 64u) {
            k = 0u;
            ++R.blocks;
            blk = blk + 1u == bpm ? 0u : blk + 1u;
        }
    }
    R.exit = stop ? JpegLaneState{8u * len, kJpegLaneStop} : JpegLaneState{B.pos, k | blk << 8};
    return R;
}
struct JpegNoPut {
    __host__ __device__ void operator()(uint32_t, uint32_t, int32_t) const {}
};

// The block that ordinal o of an interval (its o-th block in decode order) is, exactly as K17a
// computes it from m, c, by, bx.  o < n_mcu * bpm, so m < first_mcu + n_mcu.
__host__ __device__ inline int32_t jpeg_block_of_ordinal(uint32_t o, uint32_t first_mcu, int32_t ncomp, int32_t hs, int32_t vs,
                                                         int32_t mcux, int32_t mcuy) {
    const uint32_t b0 = ncomp == 1 ? 1u : (uint32_t)(hs * vs), bpm = ncomp == 1 ? 1u : b0 + 2u;
    const uint32_t m = first_mcu + o / bpm, j = o % bpm;
    const int32_t mx = (int32_t)(m % (uint32_t)mcux), my = (int32_t)(m / (uint32_t)mcux);
    const int32_t c = j < b0 ? 0 : (int32_t)(j - b0) + 1;
    const int32_t H = c == 0 ? hs : 1, V = c == 0 ? vs : 1;
    const int32_t by = c == 0 ? (int32_t)j / hs : 0, bx = c == 0 ? (int32_t)j % hs : 0;
    return jpeg_comp_base(c, hs, vs, mcux, mcuy) + (my * V + by) * (mcux * H) + mx * H + bx;
}
// The t-th block of component c in the decode order of an interval (K18b's walk).
__host__ __device__ inline int32_t jpeg_block_of_comp(uint32_t t, int32_t c, uint32_t first_mcu, int32_t hs, int32_t vs,
                                                      int32_t mcux, int32_t mcuy) {
    const uint32_t per = c == 0 ? (uint32_t)(hs * vs) : 1u;
    const uint32_t m = first_mcu + t / per, j = t % per;
    const int32_t mx = (int32_t)(m % (uint32_t)mcux), my = (int32_t)(m / (uint32_t)mcux);
    const int32_t H = c == 0 ? hs : 1, V = c == 0 ? vs : 1;
    const int32_t by = c == 0 ? (int32_t)j / hs : 0, bx = c == 0 ? (int32_t)j % hs : 0;
    return jpeg_comp_base(c, hs, vs, mcux, mcuy) + (my * V + by) * (mcux * H) + mx * H + bx;
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
// largest jpeg_total_blocks and w * h of the segments.  Behind the n_iv intervals of K17a stand
// n_split more (each shorter than kJpegSplitMaxLen) for K18a + K18b in subsequences of split_bits
// bits; the coefficients of their segments must be zero.
omr_status launch_jpeg_decode(Ctx* ctx, const uint8_t* src, const JpegSegDesc* segs, int32_t n_seg, const JpegIvDesc* ivs,
                              int32_t n_iv, const JpegTables* tables, uint8_t* ws, uint8_t* dst, int32_t* status,
                              int32_t max_blocks, int64_t max_pixels, int32_t n_split, uint32_t split_bits);

}  // namespace omr
