// omr_jpegdec.cpp — K17, host half: baseline JPEG segments of a TIFF (Compression 7).
//
// The header parser (jpeg_prepare: the TIFF's JPEGTables stream and the segment's own markers up
// to SOS, the tables resolved per component, the restart intervals listed by one pass over the
// entropy-coded bytes), the serial decoder of the host route (omr_jpeg_decode_host: get_tile's, and
// the reference of the device route) and omr_jpeg_stream_forms.  The device route
// (omr_jpegdec.hip) takes its tables and intervals from the same jpeg_prepare and shares the
// arithmetic behind the entropy decode with this file through omr_jpegdec.h.  Also here: the host
// emulation of the split entropy decode (K18, omr_jpeg_decode_host_split), which plays the lanes of
// k_jpeg_entropy_split with the per-lane decoder of omr_jpegdec.h.
//
// All input is user-uploaded bytes: every read is behind a comparison with the stream's length
// (Rd), the only allocations are sized by the caller's width and height (the frame must match
// them), and the interval list is bounded by the frame's MCU count.
//
// In scope: SOF0, 8 bits, one or three components in one interleaved scan, luma 1x1, 2x1 or 2x2
// over 1x1 chroma, DRI with RST0..7 in order, APPn / COM skipped, fill bytes before a marker.
// Stricter than libjpeg, which pads damaged data with zeros and goes on: a code that is not in the
// table, a coefficient index past 63 (a ZRL that leaves the block included), a DC category above 11
// or an AC category above 10 (no 8-bit stream holds them), a DC value outside [-2048, 2047], bits
// missing at the end of an interval, a missing, surplus or out-of-order RST and a missing EOI are
// all damage.
#include "omr_jpegdec.h"

#include <memory>

namespace omr {
namespace {

constexpr uint64_t kMaxDecoded = (uint64_t)256 << 20;
const uint8_t kZigzag[64] = OMR_JPEG_ZIGZAG;

struct RawHuff {
    bool defined = false, from_tables = false;
    uint8_t counts[17] = {0};
    uint8_t vals[256] = {0};
};
struct RawQuant {
    bool defined = false, from_tables = false;
    uint16_t q[64] = {0};    // natural order
};
struct TableStore {
    RawQuant q[4];
    RawHuff h[2][4];         // [class: 0 DC, 1 AC][id]
};

struct Fail {
    omr_status st = OMR_OK;
    std::string* why;
    omr_status set(omr_status s, const char* what) {
        st = s;
        if (why) *why = what;
        return s;
    }
};

// DQT and DHT bodies (p[0, n): what follows the length word).
omr_status take_dqt(const uint8_t* p, size_t n, TableStore& T, bool tables_stream, uint32_t& forms, Fail& F) {
    int count = 0;
    while (n) {
        const int pq = p[0] >> 4, tq = p[0] & 15;
        if (pq == 1) return F.set(OMR_INVALID_ARGUMENT, "jpeg: 16-bit quantisation table");
        if (pq != 0 || tq > 3) return F.set(OMR_INTERNAL, "jpeg: bad DQT");
        if (n < 65) return F.set(OMR_INTERNAL, "jpeg: short DQT");
        RawQuant& Q = T.q[tq];
        if (!tables_stream && Q.defined && Q.from_tables) forms |= 1u << OMR_JPEG_FORM_TABLE_OVERRIDE;
        for (int k = 0; k < 64; ++k) Q.q[kZigzag[k]] = p[1 + k];
        Q.defined = true;
        Q.from_tables = tables_stream;
        p += 65;
        n -= 65;
        if (++count == 2) forms |= 1u << OMR_JPEG_FORM_MULTI_TABLE;
    }
    return OMR_OK;
}

omr_status take_dht(const uint8_t* p, size_t n, TableStore& T, bool tables_stream, uint32_t& forms, Fail& F) {
    int count = 0;
    while (n) {
        const int tc = p[0] >> 4, th = p[0] & 15;
        if (tc > 1 || th > 3) return F.set(OMR_INTERNAL, "jpeg: bad DHT");
        if (n < 17) return F.set(OMR_INTERNAL, "jpeg: short DHT");
        size_t total = 0;
        for (int l = 1; l <= 16; ++l) total += p[l];
        if (total > 256 || n < 17 + total) return F.set(OMR_INTERNAL, "jpeg: short DHT");
        RawHuff& H = T.h[tc][th];
        if (!tables_stream && H.defined && H.from_tables) forms |= 1u << OMR_JPEG_FORM_TABLE_OVERRIDE;
        H.counts[0] = 0;
        std::memcpy(H.counts + 1, p + 1, 16);
        std::memset(H.vals, 0, sizeof H.vals);
        std::memcpy(H.vals, p + 17, total);
        H.defined = true;
        H.from_tables = tables_stream;
        p += 17 + total;
        n -= 17 + total;
        if (++count == 2) forms |= 1u << OMR_JPEG_FORM_MULTI_TABLE;
    }
    return OMR_OK;
}

// The canonical code of a DHT as the decoders' lookup table; false: the lengths oversubscribe the code space.
bool build_huff(const RawHuff& R, JpegHuff& H) {
    std::memset(&H, 0, sizeof H);
    std::memcpy(H.vals, R.vals, 256);
    uint32_t code = 0;
    int p = 0;
    for (int l = 1; l <= 16; ++l) {
        const int n = R.counts[l];
        H.valoff[l] = p - (int32_t)code;
        for (int k = 0; k < n; ++k, ++p, ++code)
            if (l <= 9)
                for (uint32_t e = code << (9 - l), e1 = (code + 1) << (9 - l); e < e1 && e < 512; ++e)
                    H.lut[e] = (uint16_t)(l << 8 | R.vals[p]);
        H.maxcode[l] = n ? (int32_t)code - 1 : -1;
        if (code >= (1u << l)) return false;               // as libjpeg: the all-ones code stays free
        code <<= 1;
    }
    H.maxcode[0] = -1;
    H.maxcode[17] = 0x7FFFFFFF;
    return true;
}

// A marker segment's body at src[pos]: its length word checked against len.  false: it runs past the stream.
bool body_of(const uint8_t* src, size_t len, size_t pos, size_t& body, size_t& n) {
    if (pos > len || len - pos < 2) return false;
    const size_t L = (size_t)src[pos] << 8 | src[pos + 1];
    if (L < 2 || L > len - pos) return false;
    body = pos + 2;
    n = L - 2;
    return true;
}

// The marker at or behind pos (fill FF bytes skipped); pos then points behind it.  -1: none.
int next_marker(const uint8_t* src, size_t len, size_t& pos, uint32_t* forms) {
    if (pos >= len || src[pos] != 0xFF) return -1;
    size_t k = pos + 1;
    while (k < len && src[k] == 0xFF) ++k;
    if (k >= len) return -1;
    if (forms && k != pos + 1) *forms |= 1u << OMR_JPEG_FORM_FILL_BYTES;
    pos = k + 1;
    return src[k];
}

// The TIFF's JPEGTables: SOI, DQT / DHT (and skipped APPn / COM), EOI.
omr_status take_tables_stream(const uint8_t* t, size_t len, TableStore& T, uint32_t& forms, Fail& F) {
    size_t pos = 0;
    if (next_marker(t, len, pos, nullptr) != 0xD8) return F.set(OMR_INTERNAL, "jpeg: JPEGTables without SOI");
    for (;;) {
        const int m = next_marker(t, len, pos, &forms);
        if (m < 0) return F.set(OMR_INTERNAL, "jpeg: JPEGTables cut short");
        if (m == 0xD9) return OMR_OK;
        size_t body, n;
        if (m == 0xD8 || (m >= 0xD0 && m <= 0xD7) || m == 0x01 || !body_of(t, len, pos, body, n))
            return F.set(OMR_INTERNAL, "jpeg: JPEGTables cut short");
        omr_status st = OMR_OK;
        if (m == 0xDB) st = take_dqt(t + body, n, T, true, forms, F);
        else if (m == 0xC4) st = take_dht(t + body, n, T, true, forms, F);
        if (st) return st;
        pos = body + n;
    }
}

const char* sof_name(int m) {
    switch (m) {
    case 0xC1: return "jpeg: extended sequential DCT (SOF1)";
    case 0xC2: return "jpeg: progressive DCT (SOF2)";
    case 0xC3: return "jpeg: lossless (SOF3)";
    case 0xC5: case 0xC6: case 0xC7: return "jpeg: differential (hierarchical) frame";
    default: return "jpeg: arithmetic coding (SOF9 and above)";
    }
}

// ---- the entropy decoder of the host route ---------------------------------------------------------

struct Bits {
    const uint8_t* p;
    const uint8_t* end;
    uint64_t acc = 0;
    int nbits = 0, fake = 0;     // fake: zero bits appended behind the interval's last byte (all at the bottom of acc)
    void fill() {
        while (nbits <= 56) {
            uint32_t b = 0;
            if (p < end) {
                b = *p++;
                if (b == 0xFF && p < end) ++p;             // its stuffed 00 (jpeg_prepare checked it)
            } else {
                fake += 8;
            }
            acc |= (uint64_t)b << (56 - nbits);
            nbits += 8;
        }
    }
    bool take(int n, uint32_t& v) {                       // n in [0, 16]
        if (nbits < 32) fill();
        if (nbits - fake < n) return false;
        v = n ? (uint32_t)(acc >> (64 - n)) : 0u;
        acc = n ? acc << n : acc;
        nbits -= n;
        return true;
    }
};

struct Decoder {
    const JpegPlan& P;
    uint32_t forms = 0;

    // One symbol; -1: no such code, or the interval ends inside it.
    int symbol(Bits& B, const JpegHuff& H) {
        if (B.nbits < 32) B.fill();
        const uint32_t peek = (uint32_t)(B.acc >> 48);
        int len = 0, sym = 0;
        const uint32_t e = H.lut[peek >> 7];
        if (e) {
            len = (int)(e >> 8);
            sym = (int)(e & 255u);
        } else {
            for (int l = 10; l <= 16; ++l) {
                const int32_t code = (int32_t)(peek >> (16 - l));
                if (code <= H.maxcode[l]) {
                    const int32_t idx = code + H.valoff[l];
                    if (idx < 0 || idx > 255) return -1;
                    len = l;
                    sym = H.vals[idx];
                    break;
                }
            }
            if (!len) return -1;
        }
        if (B.nbits - B.fake < len) return -1;
        if (len >= 12) forms |= 1u << OMR_JPEG_FORM_LONG_CODE;
        B.acc <<= len;
        B.nbits -= len;
        return sym;
    }
    static int32_t extend(uint32_t v, int s) { return v < (1u << (s - 1)) ? (int32_t)v - (1 << s) + 1 : (int32_t)v; }

    // The MCUs of one interval into coef (the layout of JpegSegDesc).
    bool interval(const uint8_t* src, const JpegInterval& iv, int16_t* coef) {
        Bits B{src + iv.off, src + iv.off + iv.len};
        int32_t pred[3] = {0, 0, 0};
        for (uint32_t m = iv.first_mcu; m < iv.first_mcu + iv.n_mcu; ++m) {
            const int32_t mx = (int32_t)(m % (uint32_t)P.mcux), my = (int32_t)(m / (uint32_t)P.mcux);
            for (int c = 0; c < P.ncomp; ++c) {
                const int32_t H = c == 0 ? P.hs : 1, V = c == 0 ? P.vs : 1;
                const int32_t base = jpeg_comp_base(c, P.hs, P.vs, P.mcux, P.mcuy), bw = P.mcux * H;
                for (int32_t by = 0; by < V; ++by)
                    for (int32_t bx = 0; bx < H; ++bx) {
                        int16_t* blk = coef + (size_t)64 * (size_t)(base + (my * V + by) * bw + mx * H + bx);
                        std::memset(blk, 0, 128);
                        int s = symbol(B, P.tables.h[c][0]);
                        if (s < 0 || s > 11) return false;
                        if (s >= 9) forms |= 1u << OMR_JPEG_FORM_DC_CAT9;
                        uint32_t v;
                        if (!B.take(s, v)) return false;
                        pred[c] += s ? extend(v, s) : 0;
                        if (pred[c] < -2048 || pred[c] > 2047) return false;
                        blk[0] = (int16_t)pred[c];
                        int k = 1;
                        while (k < 64) {
                            const int rs = symbol(B, P.tables.h[c][1]);
                            if (rs < 0) return false;
                            const int r = rs >> 4;
                            s = rs & 15;
                            if (s == 0) {
                                if (r != 15) {
                                    forms |= 1u << OMR_JPEG_FORM_EOB_EARLY;
                                    break;
                                }
                                forms |= 1u << OMR_JPEG_FORM_ZRL;
                                k += 16;
                                if (k > 63) return false;
                                continue;
                            }
                            k += r;
                            if (k > 63 || s > 10) return false;
                            if (!B.take(s, v)) return false;
                            blk[kZigzag[k]] = (int16_t)extend(v, s);
                            if (k == 63) forms |= 1u << OMR_JPEG_FORM_FULL_BLOCK;
                            ++k;
                        }
                    }
            }
        }
        // what is left of the last byte touched are the pad bits in front of the marker
        const int real = B.nbits - B.fake;
        if (real >= 0 && (real & 7)) forms |= 1u << OMR_JPEG_FORM_PAD_BITS;
        return true;
    }
};

// Coefficients -> out (chunky [h][w][ncomp]).
void reconstruct(const JpegPlan& P, bool ycc, const int16_t* coef, uint8_t* planes, uint8_t* out) {
    for (int c = 0; c < P.ncomp; ++c) {
        const int32_t H = c == 0 ? P.hs : 1, V = c == 0 ? P.vs : 1;
        const int32_t base = jpeg_comp_base(c, P.hs, P.vs, P.mcux, P.mcuy), bw = P.mcux * H, bh = P.mcuy * V;
        const size_t pitch = (size_t)8 * bw;
        for (int32_t b = 0; b < bw * bh; ++b)
            jpeg_idct_block(coef + (size_t)64 * (size_t)(base + b), P.tables.q[c],
                            planes + (size_t)64 * base + (size_t)(b / bw) * 8 * pitch + (size_t)(b % bw) * 8, pitch);
    }
    JpegSegDesc S{};
    S.w = P.w; S.h = P.h; S.ncomp = P.ncomp; S.hs = P.hs; S.vs = P.vs; S.ycc = ycc; S.mcux = P.mcux; S.mcuy = P.mcuy;
    for (int32_t y = 0; y < P.h; ++y)
        for (int32_t x = 0; x < P.w; ++x) jpeg_pixel(S, planes, x, y, out + ((size_t)y * P.w + x) * P.ncomp);
}

// ---- K18 on the host: plain loops play the lanes of k_jpeg_entropy_split ---------------------------

// One interval through the rounds of K18a (omr_jpegdec.hip): guess, settle, scan, write.  The settle
// step is the kernel's: every lane looks at its predecessor's exit state as the iteration before
// left it (the kernel has a barrier between the look and the decode).  coef must be zero where the
// interval's blocks are; the DC places get differences (split_dc_sums turns them into values).
bool split_interval(const JpegPlan& P, const uint8_t* src, const JpegInterval& iv, int16_t* coef, uint32_t S, uint32_t L,
                    omr_jpeg_split_stats& st) {
    const uint8_t* s = src + iv.off;
    const uint32_t len = (uint32_t)iv.len;
    const uint32_t b0 = P.ncomp == 1 ? 1u : (uint32_t)(P.hs * P.vs), bpm = P.ncomp == 1 ? 1u : b0 + 2u;
    const uint32_t total = iv.n_mcu * bpm;
    const uint32_t nsub = (uint32_t)(((uint64_t)8 * len + S - 1) / S), rounds = (nsub + L - 1) / L;
    const JpegHuff* huff = &P.tables.h[0][0];
    std::vector<JpegLaneState> start(L);
    std::vector<JpegLaneRun> run(L), seen(L);
    std::vector<uint32_t> end(L);
    JpegLaneState carry{0u, 0u};
    uint32_t done = 0;                                     // blocks the earlier rounds finished
    bool good = true;
    st.subsequences += nsub;
    uint32_t r = 0;
    for (; r < rounds; ++r) {
        const uint32_t live = std::min(L, nsub - r * L);   // the lanes that have a subsequence: the others sit still
        for (uint32_t i = 0; i < L; ++i) {                 // 1. guess
            const uint32_t sub = r * L + i;
            start[i] = i == 0 ? carry : JpegLaneState{sub * S, 0u};
            end[i] = sub < nsub ? (uint32_t)std::min<uint64_t>((uint64_t)(sub + 1) * S, (uint64_t)8 * len) : 0u;
            run[i] = jpeg_lane_decode<false>(s, len, huff, kZigzag, b0, bpm, start[i], end[i], 0xFFFFFFFFu, JpegNoPut());
        }
        uint32_t it = 0;
        for (; it < L; ++it) {                             // 2. settle
            seen = run;
            bool changed = false;
            for (uint32_t i = 1; i < live; ++i)
                if (seen[i - 1].exit != start[i]) {
                    start[i] = seen[i - 1].exit;
                    run[i] = jpeg_lane_decode<false>(s, len, huff, kZigzag, b0, bpm, start[i], end[i], 0xFFFFFFFFu, JpegNoPut());
                    changed = true;
                    ++st.redecodes;
                }
            if (!changed) break;
        }
        st.max_settle_iterations = std::max(st.max_settle_iterations, it);
        uint32_t first = done;                             // 3. scan
        for (uint32_t i = 0; i < L; ++i) {                 // 4. write
            const uint32_t room = total > first ? total - first : 0u;
            const uint32_t fm = iv.first_mcu;
            jpeg_lane_decode<true>(s, len, huff, kZigzag, b0, bpm, start[i], end[i], room, [&](uint32_t b, uint32_t n, int32_t v) {
                coef[(size_t)64 * (size_t)jpeg_block_of_ordinal(first + b, fm, P.ncomp, P.hs, P.vs, P.mcux, P.mcuy) + n] = (int16_t)v;
            });
            if ((run[i].exit.meta & kJpegLaneStop) && first + run[i].blocks < total) good = false;
            if (run[i].err != kJpegLaneNoError && first + run[i].err < total) good = false;
            first += run[i].blocks;
        }
        done = first;
        carry = run[live - 1].exit;
        if ((carry.meta & kJpegLaneStop) || done >= total) {
            ++r;
            break;
        }
    }
    st.rounds = std::max(st.rounds, r);
    return good && done >= total;
}

// K18b on the host: the DC differences of an interval's blocks into values, component by component
// in decode order, the predictor from 0; false: a value outside [-2048, 2047].
bool split_dc_sums(const JpegPlan& P, const JpegInterval& iv, int16_t* coef) {
    for (int c = 0; c < P.ncomp; ++c) {
        const uint32_t n = iv.n_mcu * (c == 0 ? (uint32_t)(P.hs * P.vs) : 1u);
        int32_t pred = 0;
        for (uint32_t t = 0; t < n; ++t) {
            int16_t* dc = coef + (size_t)64 * (size_t)jpeg_block_of_comp(t, c, iv.first_mcu, P.hs, P.vs, P.mcux, P.mcuy);
            pred += *dc;
            if (pred < -2048 || pred > 2047) return false;
            *dc = (int16_t)pred;
        }
    }
    return true;
}

// split_bits != 0: the entropy decode by split_interval / split_dc_sums with `lanes` lanes.
omr_status decode(const uint8_t* tables, size_t tables_len, const uint8_t* src, size_t len, int32_t w, int32_t h,
                  int32_t samples, bool ycc, uint8_t* dst, uint32_t* forms, std::string* why, uint32_t split_bits = 0,
                  uint32_t lanes = 0, omr_jpeg_split_stats* stats = nullptr) {
    std::unique_ptr<JpegPlan> P(new JpegPlan);
    const omr_status st = jpeg_prepare(tables, tables_len, src, len, w, h, samples, *P, why);
    if (st) return st;
    const size_t blocks = (size_t)jpeg_total_blocks(P->ncomp, P->hs, P->vs, P->mcux, P->mcuy);
    std::vector<int16_t> coef(blocks * 64);
    Decoder D{*P};
    D.forms = P->forms;
    for (const JpegInterval& iv : P->intervals) {
        const bool split = split_bits && iv.len < kJpegSplitMaxLen;
        if (split ? !(split_interval(*P, src, iv, coef.data(), split_bits, lanes, *stats) && split_dc_sums(*P, iv, coef.data()))
                  : !D.interval(src, iv, coef.data())) {
            if (why) *why = "jpeg: damaged entropy-coded data";
            return OMR_INTERNAL;
        }
    }
    if (forms) *forms = D.forms;
    if (dst) {
        std::vector<uint8_t> planes(blocks * 64);
        reconstruct(*P, ycc, coef.data(), planes.data(), dst);
    }
    return OMR_OK;
}

}  // namespace

omr_status jpeg_prepare(const uint8_t* tables, size_t tables_len, const uint8_t* src, size_t len, int32_t w, int32_t h,
                        int32_t samples, JpegPlan& out, std::string* why) {
    Fail F{OMR_OK, why};
    std::unique_ptr<TableStore> T(new TableStore);
    uint32_t forms = 0;
    if (tables && tables_len) {
        const omr_status st = take_tables_stream(tables, tables_len, *T, forms, F);
        if (st) return st;
        forms |= 1u << OMR_JPEG_FORM_TABLES_STREAM;
    }
    size_t pos = 0;
    if (next_marker(src, len, pos, nullptr) != 0xD8) return F.set(OMR_INTERNAL, "jpeg: no SOI");
    bool have_frame = false;
    int32_t ncomp = 0, ri = 0;
    uint8_t cid[3] = {0}, chv[3] = {0}, ctq[3] = {0}, ctd[3] = {0}, cta[3] = {0};
    for (;;) {
        const int m = next_marker(src, len, pos, &forms);
        if (m < 0) return F.set(OMR_INTERNAL, "jpeg: header cut short");
        if (m == 0xD8 || m == 0xD9 || (m >= 0xD0 && m <= 0xD7) || m == 0x01 || m == 0xC8)
            return F.set(OMR_INTERNAL, "jpeg: marker out of place");
        size_t body, n;
        if (!body_of(src, len, pos, body, n)) return F.set(OMR_INTERNAL, "jpeg: header cut short");
        const uint8_t* p = src + body;
        omr_status st = OMR_OK;
        if (m == 0xDB) {
            st = take_dqt(p, n, *T, false, forms, F);
        } else if (m == 0xC4) {
            st = take_dht(p, n, *T, false, forms, F);
        } else if (m == 0xDC) {
            return F.set(OMR_INVALID_ARGUMENT, "jpeg: DNL");
        } else if (m == 0xDD) {
            if (n != 2) return F.set(OMR_INTERNAL, "jpeg: bad DRI");
            ri = p[0] << 8 | p[1];
        } else if (m == 0xFE) {
            forms |= 1u << OMR_JPEG_FORM_COM;
        } else if (m >= 0xC1 && m <= 0xCF) {
            return F.set(OMR_INVALID_ARGUMENT, sof_name(m));
        } else if (m == 0xC0) {
            if (have_frame || n < 6) return F.set(OMR_INTERNAL, "jpeg: bad SOF");
            if (p[0] != 8) return F.set(OMR_INVALID_ARGUMENT, p[0] == 12 ? "jpeg: 12-bit samples" : "jpeg: sample precision");
            const int32_t fh = p[1] << 8 | p[2], fw = p[3] << 8 | p[4];
            ncomp = p[5];
            if (n != (size_t)(6 + 3 * ncomp)) return F.set(OMR_INTERNAL, "jpeg: bad SOF");
            if (ncomp == 4) return F.set(OMR_INVALID_ARGUMENT, "jpeg: four components");
            if ((ncomp != 1 && ncomp != 3) || ncomp != samples)
                return F.set(OMR_INVALID_ARGUMENT, "jpeg: component count differs from SamplesPerPixel");
            if (fh == 0) return F.set(OMR_INVALID_ARGUMENT, "jpeg: DNL");
            if (fw != w || fh != h) return F.set(OMR_INTERNAL, "jpeg: frame size differs from the segment's");
            for (int c = 0; c < ncomp; ++c) {
                cid[c] = p[6 + 3 * c];
                chv[c] = p[7 + 3 * c];
                ctq[c] = p[8 + 3 * c];
                if (ctq[c] > 3) return F.set(OMR_INTERNAL, "jpeg: bad SOF");
            }
            have_frame = true;
        } else if (m == 0xDA) {
            if (!have_frame) return F.set(OMR_INTERNAL, "jpeg: SOS before SOF");
            if (n < 1) return F.set(OMR_INTERNAL, "jpeg: bad SOS");
            const int ns = p[0];
            if (ns < 1 || ns > 4 || n != (size_t)(4 + 2 * ns)) return F.set(OMR_INTERNAL, "jpeg: bad SOS");
            if (ns != ncomp) return F.set(OMR_INVALID_ARGUMENT, "jpeg: more than one scan");
            for (int c = 0; c < ns; ++c) {
                if (p[1 + 2 * c] != cid[c]) return F.set(OMR_INVALID_ARGUMENT, "jpeg: scan components out of frame order");
                ctd[c] = p[2 + 2 * c] >> 4;
                cta[c] = p[2 + 2 * c] & 15;
                if (ctd[c] > 3 || cta[c] > 3) return F.set(OMR_INTERNAL, "jpeg: bad SOS");
            }
            pos = body + n;
            break;
        }
        if (st) return st;
        pos = body + n;
    }
    // sampling
    out.w = w; out.h = h; out.ncomp = ncomp; out.hs = out.vs = 1;
    if (ncomp == 3) {
        if (chv[1] != 0x11 || chv[2] != 0x11 || (chv[0] != 0x11 && chv[0] != 0x21 && chv[0] != 0x22))
            return F.set(OMR_INVALID_ARGUMENT, "jpeg: chroma sampling other than 4:4:4, 4:2:2, 4:2:0");
        out.hs = chv[0] >> 4;
        out.vs = chv[0] & 15;
    } else if ((chv[0] >> 4) < 1 || (chv[0] >> 4) > 4 || (chv[0] & 15) < 1 || (chv[0] & 15) > 4) {
        return F.set(OMR_INTERNAL, "jpeg: bad SOF");
    }
    out.mcux = (w + 8 * out.hs - 1) / (8 * out.hs);
    out.mcuy = (h + 8 * out.vs - 1) / (8 * out.vs);
    // tables
    for (int c = 0; c < ncomp; ++c) {
        const RawQuant& Q = T->q[ctq[c]];
        const RawHuff &D = T->h[0][ctd[c]], &A = T->h[1][cta[c]];
        if (!Q.defined || !D.defined || !A.defined) return F.set(OMR_INTERNAL, "jpeg: a table is referenced but never defined");
        std::memcpy(out.tables.q[c], Q.q, sizeof Q.q);
        if (!build_huff(D, out.tables.h[c][0]) || !build_huff(A, out.tables.h[c][1]))
            return F.set(OMR_INTERNAL, "jpeg: bad Huffman table");
    }
    for (int c = ncomp; c < 3; ++c) {
        std::memset(out.tables.q[c], 0, sizeof out.tables.q[c]);
        std::memset(out.tables.h[c], 0, sizeof out.tables.h[c]);
    }
    // the restart intervals: one pass over the entropy-coded bytes
    const uint32_t total = (uint32_t)out.mcux * (uint32_t)out.mcuy;
    const uint32_t per = ri ? (uint32_t)ri : total;
    const uint32_t want = (total + per - 1) / per;
    out.intervals.clear();
    size_t start = pos, i = pos;
    for (;;) {
        const uint8_t* f = i < len ? static_cast<const uint8_t*>(std::memchr(src + i, 0xFF, len - i)) : nullptr;
        if (!f) return F.set(OMR_INTERNAL, "jpeg: entropy-coded data cut short");
        const size_t j = (size_t)(f - src);
        size_t k = j + 1;
        while (k < len && src[k] == 0xFF) ++k;
        if (k >= len) return F.set(OMR_INTERNAL, "jpeg: entropy-coded data cut short");
        const int m = src[k];
        if (m == 0) {
            if (k != j + 1) return F.set(OMR_INTERNAL, "jpeg: fill bytes inside entropy-coded data");
            forms |= 1u << OMR_JPEG_FORM_STUFFED_FF;
            i = k + 1;
            continue;
        }
        if (k != j + 1) forms |= 1u << OMR_JPEG_FORM_FILL_BYTES;
        const uint32_t done = (uint32_t)out.intervals.size();
        out.intervals.push_back({start, j - start, done * per, std::min(per, total - done * per)});
        if (m >= 0xD0 && m <= 0xD7) {
            if (!ri || m != 0xD0 + (int)(done & 7u) || done + 1 >= want)
                return F.set(OMR_INTERNAL, "jpeg: restart marker missing, surplus or out of order");
            forms |= 1u << OMR_JPEG_FORM_RESTART;
            start = i = k + 1;
            continue;
        }
        if (done + 1 != want) return F.set(OMR_INTERNAL, "jpeg: restart marker missing, surplus or out of order");
        if (m == 0xDC) return F.set(OMR_INVALID_ARGUMENT, "jpeg: DNL");
        // behind the scan: EOI, or further marker segments; a second SOS is a form out of scope
        size_t q = k + 1;
        int mk = m;
        while (mk != 0xD9) {
            if (mk == 0xDA) return F.set(OMR_INVALID_ARGUMENT, "jpeg: more than one scan");
            size_t body, n;
            if (mk == 0xD8 || (mk >= 0xD0 && mk <= 0xD7) || mk == 0x01 || !body_of(src, len, q, body, n))
                return F.set(OMR_INTERNAL, "jpeg: no EOI");
            q = body + n;
            mk = next_marker(src, len, q, nullptr);
            if (mk < 0) return F.set(OMR_INTERNAL, "jpeg: no EOI");
        }
        break;
    }
    out.forms = forms;
    return OMR_OK;
}

}  // namespace omr

using namespace omr;

extern "C" {

omr_status omr_jpeg_decode_host(const uint8_t* tables, size_t tables_length, const uint8_t* src, size_t length,
                                int32_t width, int32_t height, int32_t samples, int32_t ycbcr, uint8_t* dst,
                                char* why, size_t why_cap) {
    if (why && why_cap) why[0] = 0;
    if (!src || !dst || (!tables && tables_length) || width < 1 || height < 1 || (samples != 1 && samples != 3) ||
        width > 65535 || height > 65535 || (uint64_t)width * (uint64_t)height * (uint64_t)samples > kMaxDecoded)
        return OMR_INVALID_ARGUMENT;
    std::string msg;
    const omr_status st = decode(tables, tables_length, src, length, width, height, samples, ycbcr != 0, dst, nullptr, &msg);
    if (why && why_cap) {
        std::strncpy(why, msg.c_str(), why_cap - 1);
        why[why_cap - 1] = 0;
    }
    return st;
}

omr_status omr_jpeg_decode_host_split(const uint8_t* tables, size_t tables_length, const uint8_t* src, size_t length,
                                      int32_t width, int32_t height, int32_t samples, int32_t ycbcr,
                                      uint32_t subsequence_bits, uint32_t lanes, uint8_t* dst, omr_jpeg_split_stats* stats) {
    if (!src || !dst || !stats || (!tables && tables_length) || width < 1 || height < 1 || (samples != 1 && samples != 3) ||
        width > 65535 || height > 65535 || (uint64_t)width * (uint64_t)height * (uint64_t)samples > kMaxDecoded ||
        subsequence_bits < 32 || subsequence_bits > 4096 || subsequence_bits % 32 || lanes < 1 || lanes > kJpegSplitLanes)
        return OMR_INVALID_ARGUMENT;
    *stats = omr_jpeg_split_stats{0, 0, 0, 0};
    return decode(tables, tables_length, src, length, width, height, samples, ycbcr != 0, dst, nullptr, nullptr,
                  subsequence_bits, lanes, stats);
}

omr_status omr_jpeg_stream_forms(const uint8_t* tables, size_t tables_length, const uint8_t* src, size_t length,
                                 uint32_t* forms) {
    if (!src || !forms || (!tables && tables_length)) return OMR_INVALID_ARGUMENT;
    *forms = 0;
    // the frame's own size and component count: the SOF0 is found by the marker walk of a first parse
    size_t pos = 0;
    if (next_marker(src, length, pos, nullptr) != 0xD8) return OMR_INTERNAL;
    int32_t w = 0, h = 0, nc = 0;
    for (;;) {
        const int m = next_marker(src, length, pos, nullptr);
        size_t body, n;
        if (m < 0 || m == 0xDA || m == 0xD9 || !body_of(src, length, pos, body, n)) return OMR_INTERNAL;
        if (m == 0xC0 && n >= 6) {
            h = src[body + 1] << 8 | src[body + 2];
            w = src[body + 3] << 8 | src[body + 4];
            nc = src[body + 5];
            break;
        }
        pos = body + n;
    }
    if (w < 1 || h < 1 || (uint64_t)w * (uint64_t)h * 3u > kMaxDecoded) return OMR_INVALID_ARGUMENT;
    return decode(tables, tables_length, src, length, w, h, nc, false, nullptr, forms, nullptr);
}

}  // extern "C"
