// omr_j2kdec.h — K19 and K20: what the host decoder (omr_j2kdec.cpp) and the device decoder
// (omr_j2kdec.hip) of JPEG 2000 codestreams, reversible (K19) and irreversible (K20), share: the descriptors the host writes for
// the kernels, and all arithmetic behind tier 2 -- the MQ decoder, the three coding passes of one
// code-block, the 5/3 inverse lifting of one output sample, the inverse RCT with level shift and
// clamp -- as one set of __host__ __device__ functions, so that the two routes cannot differ (the
// omr_jpegdec.h pattern).
//
// All of K19 is integer arithmetic.  Sums are taken in uint32_t, that is modulo 2^32: for every
// stream an encoder writes they are OpenJPEG's numbers, and for a crafted stream they are still
// defined and the same on both routes.  Shifts of such sums to the right are arithmetic (j2k_asr).
//
// Coefficients carry one fractional bit while a code-block is decoded, as in OpenJPEG: a sample that
// becomes significant in bit-plane p gets 3 << p (its bit and the half below it), a refinement in
// bit-plane p adds or takes 1 << p, and the finished magnitude is the value halved towards zero.
// When every bit-plane is coded that is the exact magnitude; when the stream was truncated (fewer
// passes than 3 * planes - 2) it is the mid-point of what is left open: magnitude | 1 << (p - 1)
// for a sample whose last coded bit-plane is p >= 1.  tests/golden/tiff_j2k.npz pins this rule on
// two truncated streams against OpenJPEG's decode.
//
// K20, the irreversible path (the 9/7 transform, scalar quantisation, the irreversible colour
// transform), is float32 arithmetic with a fixed order and no contraction (the library is built
// with -ffp-contract=off), written once below for both routes: a finished sample keeps its
// fractional bit and becomes (float)signed value * step, step = half the subband's quantiser step
// (j2k_dequantise); a coefficient then is that float's bits in the 4 bytes that hold the int32 of
// the reversible path.  Every lifting step is j2k_lift97_step, every scaling a single product, the
// pixel j2k_pixel97: each sample has one expression tree, whichever route evaluates it.
#pragma once

#include "omr_internal.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define OMR_J2K_UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))   // the wave decodes one block: every value is uniform
#else
#define OMR_J2K_UNI(x) ((uint32_t)(x))
#endif

namespace omr {

constexpr uint32_t kJ2kMaxBlockArea = 4096;                // T.800: xcb + ycb <= 12
constexpr uint32_t kJ2kMaxFlagBytes = 6160;                // (1024 + 2) * (4 + 2) = 6156, rounded up to 16
constexpr int kJ2kContexts = 19;
constexpr int kJ2kMaxPlanes = 30;                          // M_b: 3 << 29 fits 31 bits

// len bytes of a code-block at off in its segment's stream: one per layer that contributes.
struct J2kRange {
    uint32_t off, len;
};
// One code-block.  Its w x h coefficients go to coefficient ws_off + y * stride + x (int32 units) of
// its segment's coefficient area; orient: 0 LL, 1 HL, 2 LH, 3 HH; planes: M_b minus the zero
// bit-planes, at most kJ2kMaxPlanes; passes: all layers' together, at most 3 * planes - 2 (0: the block
// is zero); its bytes are the n_ranges ranges from range0 on.
struct J2kBlock {
    uint32_t ws_off, stride;
    uint32_t range0, n_ranges;
    uint16_t w, h;
    uint16_t passes;
    uint8_t orient, planes;
    uint32_t seg;
    float step;              // K20: half the quantiser step of the block's subband; 0 in a reversible stream
};
// One segment for the kernels.  The workspace holds, per component, the subbands in the nested
// (Mallat) layout in a plane of w x h int32 (a), and two planes the lifting alternates between: x
// of w x h and y of ceil(w / 2) x ceil(h / 2).  Level l of `levels` (1: the lowest) writes x when
// levels - l is even and y otherwise, so the image ends up in x (or stays in a when levels is 0).
struct J2kSegDesc {
    uint64_t dst_off;        // chunky [h][w][ncomp] samples of bits / 8 bytes in the decoders' destination
    uint64_t src_off;        // the segment's stream in the uploaded bytes
    uint64_t a_off, x_off, y_off;   // bytes into the workspace, multiples of 256
    int32_t w, h, ncomp, bits, levels, mct;
    int32_t swap16;          // 16-bit samples are stored byte-swapped (a big-endian file)
    int32_t lossy;           // K20: the coefficients are floats, the transform is 9/7 and mct means the ICT
};

__host__ __device__ inline int32_t j2k_asr(uint32_t v, int n) {
    return (int32_t)((v >> n) | ((v & 0x80000000u) ? ~(0xFFFFFFFFu >> n) : 0u));
}
// ceil(v / 2^s) for v >= 1 and any s >= 0
__host__ __device__ inline int32_t j2k_ceil_shift(int32_t v, int s) {
    return s >= 31 ? 1 : (int32_t)(((int64_t)v + (((int64_t)1) << s) - 1) >> s);
}

// ---- the MQ decoder (T.800 Annex C, software conventions) ----------------------------------------

// Table C.2 as Qe | NMPS << 16 | NLPS << 22 | SWITCH << 28.
#define OMR_J2K_MQ(qe, nm, nl, sw) ((uint32_t)(qe) | (uint32_t)(nm) << 16 | (uint32_t)(nl) << 22 | (uint32_t)(sw) << 28)
#define OMR_J2K_MQ_TABLE                                                                                          \
    {OMR_J2K_MQ(0x5601, 1, 1, 1),    OMR_J2K_MQ(0x3401, 2, 6, 0),    OMR_J2K_MQ(0x1801, 3, 9, 0),                     \
     OMR_J2K_MQ(0x0AC1, 4, 12, 0),   OMR_J2K_MQ(0x0521, 5, 29, 0),   OMR_J2K_MQ(0x0221, 38, 33, 0),                   \
     OMR_J2K_MQ(0x5601, 7, 6, 1),    OMR_J2K_MQ(0x5401, 8, 14, 0),   OMR_J2K_MQ(0x4801, 9, 14, 0),                    \
     OMR_J2K_MQ(0x3801, 10, 14, 0),  OMR_J2K_MQ(0x3001, 11, 17, 0),  OMR_J2K_MQ(0x2401, 12, 18, 0),                   \
     OMR_J2K_MQ(0x1C01, 13, 20, 0),  OMR_J2K_MQ(0x1601, 29, 21, 0),  OMR_J2K_MQ(0x5601, 15, 14, 1),                   \
     OMR_J2K_MQ(0x5401, 16, 14, 0),  OMR_J2K_MQ(0x5101, 17, 15, 0),  OMR_J2K_MQ(0x4801, 18, 16, 0),                   \
     OMR_J2K_MQ(0x3801, 19, 17, 0),  OMR_J2K_MQ(0x3401, 20, 18, 0),  OMR_J2K_MQ(0x3001, 21, 19, 0),                   \
     OMR_J2K_MQ(0x2801, 22, 19, 0),  OMR_J2K_MQ(0x2401, 23, 20, 0),  OMR_J2K_MQ(0x2201, 24, 21, 0),                   \
     OMR_J2K_MQ(0x1C01, 25, 22, 0),  OMR_J2K_MQ(0x1801, 26, 23, 0),  OMR_J2K_MQ(0x1601, 27, 24, 0),                   \
     OMR_J2K_MQ(0x1401, 28, 25, 0),  OMR_J2K_MQ(0x1201, 29, 26, 0),  OMR_J2K_MQ(0x1101, 30, 27, 0),                   \
     OMR_J2K_MQ(0x0AC1, 31, 28, 0),  OMR_J2K_MQ(0x09C1, 32, 29, 0),  OMR_J2K_MQ(0x08A1, 33, 30, 0),                   \
     OMR_J2K_MQ(0x0521, 34, 31, 0),  OMR_J2K_MQ(0x0441, 35, 32, 0),  OMR_J2K_MQ(0x02A1, 36, 33, 0),                   \
     OMR_J2K_MQ(0x0221, 37, 34, 0),  OMR_J2K_MQ(0x0141, 38, 35, 0),  OMR_J2K_MQ(0x0111, 39, 36, 0),                   \
     OMR_J2K_MQ(0x0085, 40, 37, 0),  OMR_J2K_MQ(0x0049, 41, 38, 0),  OMR_J2K_MQ(0x0025, 42, 39, 0),                   \
     OMR_J2K_MQ(0x0015, 43, 40, 0),  OMR_J2K_MQ(0x0009, 44, 41, 0),  OMR_J2K_MQ(0x0005, 45, 42, 0),                   \
     OMR_J2K_MQ(0x0001, 45, 43, 0),  OMR_J2K_MQ(0x5601, 46, 46, 0),  0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u,     \
     0u, 0u, 0u, 0u, 0u, 0u}

// The forms omr_j2k_stream_forms reports (bit f of its word); the first 26 are met inside a code-block.
enum : int {
    kJ2kFormZc0 = 0,         // .. 8: the zero-coding contexts
    kJ2kFormSc = 9,          // 9: context 9; then contexts 10..13 without and with the XOR flip: 10 + 2 * (ctx - 10) + xor
    kJ2kFormMr0 = 18,        // .. 20: the refinement contexts 14, 15, 16
    kJ2kFormRunTaken = 21,
    kJ2kFormRunBroken = 22,
    kJ2kFormMpsExchange = 23,
    kJ2kFormLpsExchange = 24,
    kJ2kFormFfBody = 25,
};

// The decoder's registers, the byte source (the block's ranges, then FF for ever) and the contexts'
// states (index << 1 | MPS) at cx.  All members are uniform across the wave on the device.
struct J2kMq {
    const uint8_t* base;
    const J2kRange* rg;
    uint32_t nr, ri, p, e;
    uint32_t a, c, ct, b;
    uint8_t* cx;
    uint64_t forms;

    // The next unread byte; nothing is read outside the block's ranges.
    __host__ __device__ uint32_t cur() {
        while (p == e && ri + 1u < nr) {
            ++ri;
            p = OMR_J2K_UNI(rg[ri].off);
            e = p + OMR_J2K_UNI(rg[ri].len);
        }
        return p < e ? OMR_J2K_UNI(base[p]) : 0xFFu;
    }
    template <bool kForms>
    __host__ __device__ void bytein() {
        const uint32_t nb = cur();
        if (b == 0xFFu) {
            if (kForms && p < e) forms |= 1ull << kJ2kFormFfBody;
            if (nb > 0x8Fu) {
                c += 0xFF00u;
                ct = 8u;
                return;
            }
            if (p < e) ++p;
            b = nb;
            c += nb << 9;
            ct = 7u;
            return;
        }
        if (p < e) ++p;
        b = nb;
        c += nb << 8;
        ct = 8u;
    }
    template <bool kForms>
    __host__ __device__ void init(const uint8_t* src, const J2kRange* ranges, uint32_t n, uint8_t* states) {
        base = src; rg = ranges; nr = n; ri = 0u; p = e = 0u;
        cx = states;
        forms = 0;
        if (n) {
            p = OMR_J2K_UNI(rg[0].off);
            e = p + OMR_J2K_UNI(rg[0].len);
        }
        for (int k = 0; k < kJ2kContexts; ++k) cx[k] = 0;
        cx[0] = 4 << 1;
        cx[17] = 3 << 1;
        cx[18] = 46 << 1;
        b = cur();
        if (p < e) ++p;
        c = b << 16;
        bytein<kForms>();
        c <<= 7;
        ct -= 7u;
        a = 0x8000u;
    }
    template <bool kForms>
    __host__ __device__ uint32_t decode(uint32_t ctx) {
        const uint32_t tab[64] = OMR_J2K_MQ_TABLE;
        const uint32_t s = OMR_J2K_UNI(cx[ctx]);
        uint32_t mps = s & 1u;
        const uint32_t t = tab[(s >> 1) & 63u], qe = t & 0xFFFFu;
        uint32_t d, next;
        a -= qe;
        if ((c >> 16) < qe) {
            if (a < qe) {
                d = mps;
                next = (t >> 16) & 63u;
                if (kForms) forms |= 1ull << kJ2kFormLpsExchange;
            } else {
                d = mps ^ 1u;
                next = (t >> 22) & 63u;
                mps ^= (t >> 28) & 1u;
            }
            a = qe;
        } else {
            c -= qe << 16;
            if (a & 0x8000u) return mps;
            if (a < qe) {
                d = mps ^ 1u;
                next = (t >> 22) & 63u;
                mps ^= (t >> 28) & 1u;
                if (kForms) forms |= 1ull << kJ2kFormMpsExchange;
            } else {
                d = mps;
                next = (t >> 16) & 63u;
            }
        }
        cx[ctx] = (uint8_t)(next << 1 | mps);
        do {                                               // at most 15 turns: a >= 1 here
            if (ct == 0u) bytein<kForms>();
            a <<= 1;
            c <<= 1;
            --ct;
        } while (!(a & 0x8000u));
        a &= 0xFFFFu;
        return d;
    }
};

// ---- one code-block: the three coding passes over stripes of four rows ---------------------------

constexpr uint32_t kJ2kSig = 1u, kJ2kNeg = 2u, kJ2kVisited = 4u, kJ2kRefined = 8u;

// Table D.1: the zero-coding context from the significant neighbours across (h), up and down (v)
// and diagonal (d).
__host__ __device__ inline uint32_t j2k_zc_context(uint32_t orient, uint32_t h, uint32_t v, uint32_t d) {
    if (orient == 3u) {
        const uint32_t hv = h + v;
        if (d >= 3u) return 8u;
        if (d == 2u) return hv ? 7u : 6u;
        if (d == 1u) return hv >= 2u ? 5u : hv ? 4u : 3u;
        return hv >= 2u ? 2u : hv;
    }
    if (orient == 1u) {                                    // HL: across and down change places
        const uint32_t t = h;
        h = v;
        v = t;
    }
    if (h == 2u) return 8u;
    if (h == 1u) return v ? 7u : d ? 6u : 5u;
    if (v) return 2u + v;
    return d >= 2u ? 2u : d;
}

// What a neighbour adds to the sign context: +1 significant and positive, -1 negative.
__host__ __device__ inline int32_t j2k_sign_part(uint32_t f) { return (f & kJ2kSig) ? ((f & kJ2kNeg) ? -1 : 1) : 0; }

// The block B of the stream at src (ranges at rg + B.range0) into mag (B.w * B.h values with one
// fractional bit, rows B.w apart) and fl (a flag byte per sample with a border of one:
// (B.w + 2) * (B.h + 2) bytes); both must be zero.  cx: kJ2kContexts bytes.  Every index into mag
// and fl comes from B.w and B.h alone; the stream's bytes decide values.  Returns the forms met.
template <bool kForms>
__host__ __device__ inline uint64_t j2k_t1_decode(const uint8_t* src, const J2kRange* rg, const J2kBlock& B, uint32_t* mag,
                                                  uint8_t* fl, uint8_t* cx) {
    const uint32_t w = B.w, h = B.h, fw = w + 2u, orient = B.orient;
    int32_t plane = (int32_t)B.planes - 1;
    if (B.passes == 0u || plane < 0 || plane >= kJ2kMaxPlanes) return 0;
    J2kMq M;
    M.init<kForms>(src, rg + B.range0, B.n_ranges, cx);
    uint32_t type = 2u;                                    // 0 significance propagation, 1 refinement, 2 clean-up
    // the sign of a sample that has just become significant, and its flags and value
    auto become = [&](uint8_t* q, uint32_t* m, int32_t pl) {
        const int32_t hc = j2k_sign_part(OMR_J2K_UNI(q[-1])) + j2k_sign_part(OMR_J2K_UNI(q[1]));
        const int32_t vc = j2k_sign_part(OMR_J2K_UNI(q[-(int32_t)fw])) + j2k_sign_part(OMR_J2K_UNI(q[fw]));
        const int32_t H = hc > 0 ? 1 : hc < 0 ? -1 : 0, V = vc > 0 ? 1 : vc < 0 ? -1 : 0;
        uint32_t ctx, x = 0u;
        if (H == 0) {
            ctx = V == 0 ? 9u : 10u;
            x = V < 0;
        } else {
            const int32_t sv = H > 0 ? V : -V;             // (-1, v) mirrors (1, -v) with the flip
            ctx = sv > 0 ? 13u : sv == 0 ? 12u : 11u;
            x = H < 0;
        }
        if (kForms) M.forms |= 1ull << (ctx == 9u ? kJ2kFormSc : kJ2kFormSc + 1 + 2 * (int)(ctx - 10u) + (int)x);
        const uint32_t neg = M.template decode<kForms>(ctx) ^ x;
        *q = (uint8_t)(*q | kJ2kSig | (neg ? kJ2kNeg : 0u));
        *m = 3u << pl;
    };
    auto around = [&](const uint8_t* q, uint32_t& hh, uint32_t& vv, uint32_t& dd) {
        const int32_t f = (int32_t)fw;
        hh = (OMR_J2K_UNI(q[-1]) & 1u) + (OMR_J2K_UNI(q[1]) & 1u);
        vv = (OMR_J2K_UNI(q[-f]) & 1u) + (OMR_J2K_UNI(q[f]) & 1u);
        dd = (OMR_J2K_UNI(q[-f - 1]) & 1u) + (OMR_J2K_UNI(q[-f + 1]) & 1u) + (OMR_J2K_UNI(q[f - 1]) & 1u) + (OMR_J2K_UNI(q[f + 1]) & 1u);
    };
    for (uint32_t pass = 0; pass < B.passes && plane >= 0; ++pass) {
        for (uint32_t y0 = 0; y0 < h; y0 += 4u) {
            const uint32_t rows = h - y0 < 4u ? h - y0 : 4u;
            for (uint32_t x = 0; x < w; ++x) {
                uint32_t first = 0u;                       // clean-up: the row the column's run leaves off at
                bool forced = false;                       // and whether that row is significant without a decision
                if (type == 2u && rows == 4u) {
                    uint32_t any = 0u;
                    const uint8_t* q = fl + (size_t)y0 * fw + x;    // the flag left of and above the column's first sample
                    for (uint32_t r = 0; r < 6u; ++r, q += fw) {
                        const uint32_t mid = OMR_J2K_UNI(q[1]);
                        any |= (OMR_J2K_UNI(q[0]) | mid | OMR_J2K_UNI(q[2])) & kJ2kSig;
                        if (r >= 1u && r <= 4u) any |= mid & kJ2kVisited;
                    }
                    if (!any) {
                        if (!M.template decode<kForms>(17u)) {
                            if (kForms) M.forms |= 1ull << kJ2kFormRunTaken;
                            continue;                      // (none of the four is visited: nothing to clear)
                        }
                        if (kForms) M.forms |= 1ull << kJ2kFormRunBroken;
                        first = M.template decode<kForms>(18u) << 1;
                        first |= M.template decode<kForms>(18u);
                        forced = true;
                    }
                }
                for (uint32_t r = first; r < rows; ++r) {
                    uint8_t* q = fl + (size_t)(y0 + r + 1u) * fw + x + 1u;
                    uint32_t* m = mag + (size_t)(y0 + r) * w + x;
                    const uint32_t f = OMR_J2K_UNI(*q);
                    uint32_t hh, vv, dd;
                    if (type == 0u) {
                        if (f & kJ2kSig) continue;
                        around(q, hh, vv, dd);
                        if (!(hh + vv + dd)) continue;
                        const uint32_t ctx = j2k_zc_context(orient, hh, vv, dd);
                        if (kForms) M.forms |= 1ull << (kJ2kFormZc0 + (int)ctx);
                        *q = (uint8_t)(f | kJ2kVisited);
                        if (M.template decode<kForms>(ctx)) become(q, m, plane);
                    } else if (type == 1u) {
                        if ((f & (kJ2kSig | kJ2kVisited)) != kJ2kSig) continue;
                        uint32_t ctx = 16u;
                        if (!(f & kJ2kRefined)) {
                            around(q, hh, vv, dd);
                            ctx = (hh + vv + dd) ? 15u : 14u;
                        }
                        if (kForms) M.forms |= 1ull << (kJ2kFormMr0 + (int)(ctx - 14u));
                        const uint32_t half = 1u << plane;
                        *m = OMR_J2K_UNI(*m) + (M.template decode<kForms>(ctx) ? half : 0u - half);
                        *q = (uint8_t)(f | kJ2kRefined);
                    } else {
                        if (forced && r == first) {
                            become(q, m, plane);
                            continue;
                        }
                        if (f & kJ2kVisited) {
                            *q = (uint8_t)(f & ~kJ2kVisited);
                            continue;
                        }
                        if (f & kJ2kSig) continue;
                        around(q, hh, vv, dd);
                        const uint32_t ctx = j2k_zc_context(orient, hh, vv, dd);
                        if (kForms) M.forms |= 1ull << (kJ2kFormZc0 + (int)ctx);
                        if (M.template decode<kForms>(ctx)) become(q, m, plane);
                    }
                }
            }
        }
        if (type == 2u) --plane;
        type = type == 2u ? 0u : type + 1u;
    }
    return M.forms;
}

// The coefficient of a decoded sample: the value halved towards zero, with its sign.
__host__ __device__ inline int32_t j2k_coefficient(uint32_t value, uint32_t flags) {
    const uint32_t m = value >> 1;
    return (int32_t)((flags & kJ2kNeg) ? 0u - m : m);
}

// K20: the coefficient of a decoded sample of an irreversible stream.  The fractional bit stays: a
// truncated block's samples land on the mid-point OpenJPEG reconstructs.
__host__ __device__ inline float j2k_dequantise(uint32_t value, uint32_t flags, float step) {
    const int32_t v = (int32_t)((flags & kJ2kNeg) ? 0u - value : value);
    return (float)v * step;
}
__host__ __device__ inline uint32_t j2k_float_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
__host__ __device__ inline float j2k_bits_float(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// ---- the 5/3 inverse lifting (T.800 F.3.8.1, origin 0, whole-sample symmetric extension) ----------

// Output sample i of n from the low-pass samples s(0 .. ceil(n / 2)) and the high-pass samples
// d(0 .. floor(n / 2)): x[2k] = s[k] - floor((d[k - 1] + d[k] + 2) / 4), x[2k + 1] = d[k] +
// floor((x[2k] + x[2k + 2]) / 2), with d[-1] = d[0], d[n / 2] = d[n / 2 - 1] and x[n] = x[n - 2].  One
// sample is itself; two follow the rule with both neighbours the same.
template <class S, class D>
__host__ __device__ inline int32_t j2k_lift_at(int32_t i, int32_t n, const S& s, const D& d) {
    if (n == 1) return s(0);
    const int32_t sn = (n + 1) >> 1, dn = n >> 1, k = i >> 1;
    auto even = [&](int32_t j) {
        const int32_t lo = j > 0 ? j - 1 : 0, hi = j < dn ? j : dn - 1;
        return (int32_t)((uint32_t)s(j) - (uint32_t)j2k_asr((uint32_t)d(lo) + (uint32_t)d(hi) + 2u, 2));
    };
    if (!(i & 1)) return even(k);
    const int32_t k1 = k + 1 < sn ? k + 1 : sn - 1;
    const uint32_t e0 = (uint32_t)even(k), e1 = k1 == k ? e0 : (uint32_t)even(k1);
    return (int32_t)((uint32_t)d(k) + (uint32_t)j2k_asr(e0 + e1, 1));
}

// Output sample (x, y) of a resolution of rw x rh samples from its four subbands in the nested
// layout, get(column, row): rows first (horizontal lifting), then columns.
template <class G>
__host__ __device__ inline int32_t j2k_idwt53_at(int32_t rw, int32_t rh, int32_t x, int32_t y, const G& get) {
    const int32_t lw = (rw + 1) >> 1, lh = (rh + 1) >> 1;
    auto row = [&](int32_t r) {
        return j2k_lift_at(x, rw, [&](int32_t j) { return get(j, r); }, [&](int32_t j) { return get(lw + j, r); });
    };
    return j2k_lift_at(y, rh, [&](int32_t k) { return row(k); }, [&](int32_t k) { return row(lh + k); });
}

// ---- K20: the 9/7 inverse lifting (T.800 F.3.8.2 with OpenJPEG's constants and its order) ----------
//
// A line of n >= 2 interleaved samples, the low-pass ones at the even places: both parities are
// scaled, then four steps follow, each adding to every sample of one parity the sum of its two
// neighbours times a constant; a missing neighbour is the one across the edge (whole-sample
// symmetric extension, which every step preserves, so a route may as well extend the line first
// and let the steps run over the extension).  A line of one sample is left as it is.

constexpr int kJ2kLift97Steps = 4;
constexpr int kJ2kLift97Halo = 4;      // samples a tile needs beyond each edge: one per step
// step k adds to parity (k & 1): even, odd, even, odd
__host__ __device__ inline float j2k_lift97_const(int k) {
    return k == 0 ? -0.443506852f : k == 1 ? -0.882911075f : k == 2 ? 0.052980118f : 1.586134342f;
}
__host__ __device__ inline float j2k_lift97_scale(float v, int parity) { return v * (parity ? 1.625732422f : 1.230174105f); }
__host__ __device__ inline float j2k_lift97_step(float a, float l, float r, float c) { return a + (l + r) * c; }
// i reflected into [0, n) with period 2 * (n - 1), for any i; n >= 1
__host__ __device__ inline int32_t j2k_reflect(int32_t i, int32_t n) {
    if (n <= 1) return 0;
    const int32_t p = 2 * (n - 1);
    int32_t m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - m;
}
// The place in the nested layout of interleaved sample i of a line of n: the low-pass half in front.
__host__ __device__ inline int32_t j2k_nested_index(int32_t i, int32_t n) { return (i & 1) ? ((n + 1) >> 1) + (i >> 1) : i >> 1; }
// A whole line in place (the host route): v[i * stride], i < n, interleaved.
__host__ __device__ inline void j2k_lift97_line(float* v, int32_t n, size_t stride) {
    if (n < 2) return;
    for (int32_t i = 0; i < n; ++i) v[i * stride] = j2k_lift97_scale(v[i * stride], i & 1);
    for (int k = 0; k < kJ2kLift97Steps; ++k) {
        const float c = j2k_lift97_const(k);
        for (int32_t i = k & 1; i < n; i += 2) {
            const int32_t l = i > 0 ? i - 1 : 1, r = i + 1 < n ? i + 1 : n - 2;
            v[i * stride] = j2k_lift97_step(v[i * stride], v[l * stride], v[r * stride], c);
        }
    }
}

// ---- colour, level shift, clamp -----------------------------------------------------------------

// v: the ncomp reconstructed values of one pixel -> its unsigned samples of `bits` bits.
__host__ __device__ inline void j2k_pixel(const int32_t* v, int32_t ncomp, bool mct, int32_t bits, uint32_t* out) {
    uint32_t c[3] = {(uint32_t)v[0], ncomp == 3 ? (uint32_t)v[1] : 0u, ncomp == 3 ? (uint32_t)v[2] : 0u};
    if (mct && ncomp == 3) {                               // G = Y - floor((U + V) / 4), R = V + G, B = U + G
        const uint32_t g = c[0] - (uint32_t)j2k_asr(c[1] + c[2], 2);
        const uint32_t r = c[2] + g, b = c[1] + g;
        c[0] = r; c[1] = g; c[2] = b;
    }
    const int32_t top = (1 << bits) - 1;
    for (int k = 0; k < ncomp; ++k) {
        const int32_t s = (int32_t)(c[k] + (1u << (bits - 1)));
        out[k] = (uint32_t)(s < 0 ? 0 : s > top ? top : s);
    }
}

// K20: the same for an irreversible stream: the inverse ICT when mct, then round to nearest (ties to
// even), level shift and clamp.  A value outside int32 (or a NaN, which no stream an encoder writes
// gives) is clamped before it is converted.
__host__ __device__ inline int32_t j2k_round97(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float2int_rn(v);
#else
    return (int32_t)lrintf(v);
#endif
}
__host__ __device__ inline void j2k_pixel97(const float* v, int32_t ncomp, bool mct, int32_t bits, uint32_t* out) {
    float c[3] = {v[0], ncomp == 3 ? v[1] : 0.f, ncomp == 3 ? v[2] : 0.f};
    if (mct && ncomp == 3) {
        const float y = c[0], u = c[1], w = c[2];
        c[0] = y + w * 1.402f;
        c[1] = y - u * 0.34413f - w * 0.71414f;
        c[2] = y + u * 1.772f;
    }
    const int32_t top = (1 << bits) - 1, shift = 1 << (bits - 1);
    for (int k = 0; k < ncomp; ++k) {
        int32_t s;
        if (!(c[k] > -1073741824.f)) s = c[k] != c[k] ? shift : 0;
        else if (c[k] >= 1073741824.f) s = top;
        else s = j2k_round97(c[k]) + shift;
        out[k] = (uint32_t)(s < 0 ? 0 : s > top ? top : s);
    }
}

// The resolution a level writes and where: see J2kSegDesc.
__host__ __device__ inline bool j2k_level_writes_x(int32_t levels, int32_t level) { return ((levels - level) & 1) == 0; }

// ---- the host half (omr_j2kdec.cpp) ---------------------------------------------------------------

// A codestream, parsed and checked against what the caller expects of it, its packets walked.
struct J2kPlan {
    int32_t w = 0, h = 0, ncomp = 0, bits = 0, levels = 0;
    bool mct = false;
    bool lossy = false;      // K20: the 9/7 transform with scalar quantisation; mct then means the ICT
    uint32_t lossy_forms = 0;   // the OMR_J2K_LOSSY_FORM_* bits the headers and tier 2 show (0 for a reversible stream)
    std::vector<J2kBlock> blocks;     // every code-block of every subband: together they cover the coefficient area
    std::vector<J2kRange> ranges;
    uint64_t forms = 0;      // the OMR_J2K_FORM_* bits tier 2 and the headers show
};
// src: one raw codestream.  The frame must be w x h with `samples` components of `bits` bits.
// OMR_INVALID_ARGUMENT with *why naming it: a valid form that is out of scope; OMR_INTERNAL: damage
// (*why says what).  On OMR_OK every range lies inside src, every block inside the coefficient area
// of ncomp * w * h values (ws_off and stride say where), and passes <= 3 * planes - 2 and planes <=
// kJ2kMaxPlanes hold for every block with passes.  kinds: the kJ2kTake* bits of the transforms the
// caller takes; a stream of another is OMR_INVALID_ARGUMENT by name.  In an irreversible plan every
// block's step is finite and positive.
constexpr uint32_t kJ2kTakeReversible = 1u, kJ2kTakeIrreversible = 2u;
omr_status j2k_prepare(const uint8_t* src, size_t len, int32_t w, int32_t h, int32_t samples, int32_t bits, J2kPlan& out,
                       std::string* why, uint32_t kinds = kJ2kTakeReversible);
// get_tile's decoder: omr_j2k_decode_host_ex with the kinds spelled out.
omr_status j2k_decode_host_kinds(const uint8_t* src, size_t len, int32_t w, int32_t h, int32_t samples, int32_t bits, uint8_t* dst,
                                 uint32_t kinds, std::string* why);

bool j2k_sizes_ok(int32_t w, int32_t h, int32_t samples, int32_t bits);   // what the entry points accept

inline size_t j2k_plane_bytes(int32_t w, int32_t h, int32_t ncomp) { return align_up((size_t)4 * (size_t)w * (size_t)h * (size_t)ncomp, 256); }
inline size_t j2k_half_bytes(int32_t w, int32_t h, int32_t ncomp) {
    return align_up((size_t)4 * (size_t)((w + 1) / 2) * (size_t)((h + 1) / 2) * (size_t)ncomp, 256);
}

}  // namespace omr
