// omr_zstd.cpp — K16, host half: one Zstandard frame (RFC 8878) as the OME-Zarr reader takes it
// (include/omr/omr.h).  A plain serial decoder in the style of lz4_decode (omr_blosc.cpp): chunk
// files are user-uploaded data, so every read is behind a check against the frame's length and
// every write behind one against `expected`; the tables are sized by the format's limits (Huffman
// code lengths up to 11, accuracy logs up to 9, 8, 9 and 6), nothing recurses and nothing is
// allocated from a size the stream states (the literal buffer is one block, 128 KiB).  The output
// buffer is the window.  omr_zstd_frame_forms walks a frame with the same code and reports the
// forms it met.  Nothing links libzstd; the format is pinned against libzstd 1.4.8 by the tests.
#include "omr_internal.h"

#include <memory>

namespace omr {
namespace {

constexpr size_t kBlockMax = (size_t)128 << 10;
constexpr size_t kFormsOutputMax = (size_t)256 << 20;

struct FseEntry {
    uint8_t sym, nbits;
    uint16_t base;
};
struct Fse {
    FseEntry e[512];
    uint32_t log = 0;
    bool valid = false;
};
struct Huf {
    uint8_t sym[2048], nbits[2048];
    uint32_t log = 0;
    bool valid = false;
};

inline int high_bit(uint32_t v) { return 31 - __builtin_clz(v); }      // v != 0

// Forward bits, LSB first (an FSE table description).  Bits behind the end read as zero and set `over`.
struct Fwd {
    const uint8_t* s;
    size_t len, bit = 0;
    bool over = false;
    uint32_t take(int n) {
        uint32_t v = 0;
        for (int k = 0; k < n; ++k, ++bit) {
            const size_t b = bit >> 3;
            if (b >= len) over = true;
            else v |= (uint32_t)((s[b] >> (bit & 7)) & 1u) << k;
        }
        return v;
    }
};

// Backward bits: the stream's bits [0, pos) are unread, a read takes the n below pos.  Bits below
// the stream's first read as zero and leave pos negative.
struct Back {
    const uint8_t* s = nullptr;
    int64_t len = 0, pos = 0;
    bool init(const uint8_t* p, size_t n) {
        if (n == 0 || p[n - 1] == 0) return false;
        s = p;
        len = (int64_t)n;
        pos = (len - 1) * 8 + high_bit(p[n - 1]);
        return true;
    }
    uint32_t take(int n) {                                 // n <= 32
        pos -= n;
        if (n == 0) return 0;
        const int64_t b0 = pos >> 3;                       // floor, also below zero
        uint64_t v = 0;
        for (int k = 0; k < 6; ++k) {
            const int64_t i = b0 + k;
            if (i >= 0 && i < len) v |= (uint64_t)s[i] << (8 * k);
        }
        return (uint32_t)((v >> (pos - b0 * 8)) & ((1ull << n) - 1));
    }
};

// The decoding table of a normalized distribution: freq[0, n), -1 = "less than 1", summing to 1 << log.
bool fse_build(const int16_t* freq, int n, uint32_t log, Fse& t) {
    const uint32_t size = 1u << log, mask = size - 1;
    uint16_t next[256];
    uint32_t high = size;
    for (int s = 0; s < n; ++s)
        if (freq[s] == -1) {
            t.e[--high].sym = (uint8_t)s;
            next[s] = 1;
        }
    const uint32_t step = (size >> 1) + (size >> 3) + 3;
    uint32_t pos = 0;
    for (int s = 0; s < n; ++s) {
        if (freq[s] <= 0) continue;
        next[s] = (uint16_t)freq[s];
        for (int k = 0; k < freq[s]; ++k) {
            t.e[pos].sym = (uint8_t)s;
            do pos = (pos + step) & mask;
            while (pos >= high);
        }
    }
    if (pos != 0) return false;
    for (uint32_t i = 0; i < size; ++i) {
        const uint32_t x = next[t.e[i].sym]++;
        const uint32_t nb = log - (uint32_t)high_bit(x);
        t.e[i].nbits = (uint8_t)nb;
        t.e[i].base = (uint16_t)((x << nb) - size);
    }
    t.log = log;
    t.valid = true;
    return true;
}

// An FSE table description at s[0, len): *used = its bytes.  At most max_sym symbols, log <= max_log.
bool fse_read(const uint8_t* s, size_t len, uint32_t max_log, int max_sym, Fse& t, size_t* used) {
    Fwd f{s, len};
    const uint32_t log = f.take(4) + 5;
    if (f.over || log > max_log) return false;
    int32_t remaining = 1 << log;
    int16_t freq[64];
    int n = 0;
    while (remaining > 0 && n < max_sym) {
        const int bits = high_bit((uint32_t)remaining + 1) + 1;
        uint32_t v = f.take(bits);
        const uint32_t lower = (1u << (bits - 1)) - 1, threshold = (1u << bits) - 1 - ((uint32_t)remaining + 1);
        if ((v & lower) < threshold) {
            --f.bit;
            v &= lower;
        } else if (v > lower) {
            v -= threshold;
        }
        const int32_t p = (int32_t)v - 1;
        remaining -= p < 0 ? 1 : p;
        freq[n++] = (int16_t)p;
        if (p == 0) {
            uint32_t rep;
            do {
                rep = f.take(2);
                for (uint32_t k = 0; k < rep && n < max_sym; ++k) freq[n++] = 0;
            } while (rep == 3 && !f.over);
        }
        if (f.over) return false;
    }
    if (remaining != 0 || f.over) return false;
    *used = (f.bit + 7) >> 3;
    if (*used > len) return false;
    return fse_build(freq, n, log, t);
}

const int16_t kLLDefault[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
const int16_t kOFDefault[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};
const int16_t kMLDefault[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
const uint32_t kLLBase[36] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 20, 22, 24, 28, 32, 40,
                              48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536};
const uint8_t kLLBits[36] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
const uint32_t kMLBase[53] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29,
                              30, 31, 32, 33, 34, 35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099,
                              8195, 16387, 32771, 65539};
const uint8_t kMLBits[53] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                             0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};

struct Decoder {
    const uint8_t* s;
    size_t len;
    uint8_t* d;
    size_t cap;                       // the bytes d may take
    std::vector<uint8_t>* grow;       // frame_forms: d is this vector's storage and may grow to kFormsOutputMax
    uint32_t* forms;
    size_t op = 0;
    Fse ll, of, ml;
    Huf huf;
    uint32_t rep[3] = {1, 4, 8};
    std::vector<uint8_t> litbuf;

    void form(int f) {
        if (forms) forms[f >> 5] |= 1u << (f & 31);
    }
    bool room(size_t n) {
        if (n <= cap - op) return true;
        if (!grow || n > kFormsOutputMax - op) return false;
        grow->resize(std::max(op + n, grow->size() * 2));
        d = grow->data();
        cap = grow->size();
        return true;
    }

    // The Huffman table description at p[0, n): *used = its bytes.
    bool huf_read(const uint8_t* p, size_t n, size_t* used) {
        if (n < 1) return false;
        uint8_t w[256];
        int nw = 0;
        const uint32_t hb = p[0];
        if (hb >= 128) {
            nw = (int)hb - 127;
            const size_t bytes = ((size_t)nw + 1) / 2;
            if (bytes > n - 1) return false;
            for (int k = 0; k < nw; ++k) w[k] = k & 1 ? p[1 + k / 2] & 15 : p[1 + k / 2] >> 4;
            *used = 1 + bytes;
            form(OMR_ZSTD_FORM_WEIGHTS_DIRECT);
        } else {
            if (hb > n - 1) return false;
            Fse t;
            size_t tu;
            if (!fse_read(p + 1, hb, 6, 13, t, &tu)) return false;
            Back b;
            if (tu >= hb || !b.init(p + 1 + tu, hb - tu)) return false;
            uint32_t s1 = b.take((int)t.log), s2 = b.take((int)t.log);
            if (b.pos < 0) return false;
            for (;;) {                                     // two states by turns, until the bits run out
                if (nw > 253) return false;
                w[nw++] = t.e[s1].sym;
                s1 = t.e[s1].base + b.take(t.e[s1].nbits);
                if (b.pos < 0) {
                    w[nw++] = t.e[s2].sym;
                    break;
                }
                w[nw++] = t.e[s2].sym;
                s2 = t.e[s2].base + b.take(t.e[s2].nbits);
                if (b.pos < 0) {
                    w[nw++] = t.e[s1].sym;
                    break;
                }
            }
            *used = 1 + hb;
            form(OMR_ZSTD_FORM_WEIGHTS_FSE);
        }
        // the last weight completes a power of two
        uint32_t sum = 0;
        for (int k = 0; k < nw; ++k) {
            if (w[k] > 11) return false;
            if (w[k]) sum += 1u << (w[k] - 1);
        }
        if (sum == 0 || nw > 255) return false;
        const uint32_t log = (uint32_t)high_bit(sum) + 1;
        if (log > 11) return false;
        const uint32_t left = (1u << log) - sum;
        if (left & (left - 1)) return false;               // left >= 1: sum < 1 << log
        w[nw++] = (uint8_t)(high_bit(left) + 1);
        // entries sorted by (weight, symbol), a symbol of weight w taking 1 << (w - 1) of them
        uint32_t start[13] = {0};
        for (int k = 0; k < nw; ++k)
            if (w[k]) start[w[k] + 1] += 1u << (w[k] - 1);
        for (int k = 1; k < 13; ++k) start[k] += start[k - 1];
        for (int k = 0; k < nw; ++k) {
            if (!w[k]) continue;
            const uint32_t cnt = 1u << (w[k] - 1);
            for (uint32_t i = 0; i < cnt; ++i) {
                huf.sym[start[w[k]] + i] = (uint8_t)k;
                huf.nbits[start[w[k]] + i] = (uint8_t)(log + 1 - w[k]);
            }
            start[w[k]] += cnt;
        }
        huf.log = log;
        huf.valid = true;
        return true;
    }

    // n symbols from the stream p[0, m) into out; the stream must end exactly at its first bit.
    bool huf_stream(const uint8_t* p, size_t m, uint8_t* out, size_t n) {
        Back b;
        if (!b.init(p, m)) return false;
        const uint32_t log = huf.log, mask = (1u << log) - 1;
        uint32_t state = b.take((int)log);
        // `state` holds the log bits below the position bits_left; a symbol may only begin inside the stream
        int64_t bits_left = b.pos + log;
        for (size_t k = 0; k < n; ++k) {
            if (bits_left <= 0) return false;
            const uint32_t nb = huf.nbits[state];
            out[k] = huf.sym[state];
            state = ((state << nb) | b.take((int)nb)) & mask;
            bits_left -= nb;
        }
        return bits_left == 0;
    }

    bool table(uint32_t mode, Fse& t, const int16_t* def, int ndef, uint32_t def_log, uint32_t max_log, int max_sym,
               size_t& ip, size_t end, int form0) {
        form(form0 + (int)mode);
        switch (mode) {
        case 0: return fse_build(def, ndef, def_log, t);
        case 1:
            if (ip >= end || s[ip] >= max_sym) return false;
            t.e[0].sym = s[ip++];
            t.e[0].nbits = 0;
            t.e[0].base = 0;
            t.log = 0;
            t.valid = true;
            return true;
        case 2: {
            size_t used;
            if (!fse_read(s + ip, end - ip, max_log, max_sym, t, &used)) return false;
            ip += used;
            return true;
        }
        default: return t.valid;
        }
    }

    // A compressed block s[ip, end).
    bool block(size_t ip, size_t end, size_t block_max) {
        if (end - ip < 1) return false;
        const size_t op0 = op;
        // literals
        const uint32_t b0 = s[ip], type = b0 & 3, sf = (b0 >> 2) & 3;
        const uint8_t* lit = nullptr;                      // type 1: one byte
        size_t nlit = 0;
        form(OMR_ZSTD_FORM_LIT_RAW + (int)type);
        if (type < 2) {
            const size_t hdr = sf == 1 ? 2 : sf == 3 ? 3 : 1;
            if (end - ip < hdr) return false;
            nlit = sf == 1 ? (b0 >> 4) + ((size_t)s[ip + 1] << 4)
                 : sf == 3 ? (b0 >> 4) + ((size_t)s[ip + 1] << 4) + ((size_t)s[ip + 2] << 12) : b0 >> 3;
            ip += hdr;
            if (nlit > kBlockMax) return false;
            const size_t take = type == 0 ? nlit : 1;
            if (end - ip < take) return false;
            lit = s + ip;
            ip += take;
        } else {
            const size_t hdr = sf < 2 ? 3 : sf == 2 ? 4 : 5;
            if (end - ip < hdr) return false;
            uint64_t v = 0;
            for (size_t k = 0; k < hdr; ++k) v |= (uint64_t)s[ip + k] << (8 * k);
            v >>= 4;
            const uint32_t nb = sf < 2 ? 10 : sf == 2 ? 14 : 18;
            nlit = (size_t)(v & ((1u << nb) - 1));
            size_t csize = (size_t)((v >> nb) & ((1u << nb) - 1));
            ip += hdr;
            if (nlit > kBlockMax || csize > end - ip) return false;
            const uint8_t* p = s + ip;
            ip += csize;
            if (type == 2) {
                size_t used;
                if (!huf_read(p, csize, &used)) return false;
                p += used;
                csize -= used;
            } else if (!huf.valid) {
                return false;
            }
            uint8_t* out = litbuf.data();
            if (sf == 0) {
                form(OMR_ZSTD_FORM_STREAMS_1);
                if (!huf_stream(p, csize, out, nlit)) return false;
            } else {
                form(OMR_ZSTD_FORM_STREAMS_4);
                if (csize < 6) return false;
                const size_t c1 = p[0] | (size_t)p[1] << 8, c2 = p[2] | (size_t)p[3] << 8, c3 = p[4] | (size_t)p[5] << 8;
                const size_t q = (nlit + 3) / 4;
                if (c1 + c2 + c3 > csize - 6 || 3 * q > nlit) return false;
                const size_t c4 = csize - 6 - c1 - c2 - c3;
                p += 6;
                if (!huf_stream(p, c1, out, q) || !huf_stream(p + c1, c2, out + q, q) ||
                    !huf_stream(p + c1 + c2, c3, out + 2 * q, q) || !huf_stream(p + c1 + c2 + c3, c4, out + 3 * q, nlit - 3 * q))
                    return false;
            }
            lit = out;
        }
        const bool rle = type == 1;
        size_t lp = 0;                                     // literals used
        auto put_literals = [&](size_t n) {                // n <= nlit - lp, room(n) holds
            if (rle && n) std::memset(d + op, lit[0], n);
            else if (n) std::memcpy(d + op, lit + lp, n);
            lp += n;
            op += n;
        };
        // sequences
        if (end - ip < 1) return false;
        uint32_t nseq = s[ip++];
        if (nseq == 0) {
            form(OMR_ZSTD_FORM_SEQ_ZERO);
        } else if (nseq < 128) {
            form(OMR_ZSTD_FORM_SEQ_SHORT);
        } else if (nseq < 255) {
            if (end - ip < 1) return false;
            nseq = ((nseq - 128) << 8) + s[ip++];
            form(OMR_ZSTD_FORM_SEQ_2BYTE);
        } else {
            if (end - ip < 2) return false;
            nseq = s[ip] + ((uint32_t)s[ip + 1] << 8) + 0x7F00u;
            ip += 2;
            form(OMR_ZSTD_FORM_SEQ_3BYTE);
        }
        if (nseq == 0) {
            if (ip != end) return false;
        } else {
            if (end - ip < 1) return false;
            const uint32_t modes = s[ip++];
            if (modes & 3) return false;
            if (!table(modes >> 6, ll, kLLDefault, 36, 6, 9, 36, ip, end, OMR_ZSTD_FORM_LL_PREDEFINED) ||
                !table((modes >> 4) & 3, of, kOFDefault, 29, 5, 8, 32, ip, end, OMR_ZSTD_FORM_OF_PREDEFINED) ||
                !table((modes >> 2) & 3, ml, kMLDefault, 53, 6, 9, 53, ip, end, OMR_ZSTD_FORM_ML_PREDEFINED))
                return false;
            Back b;
            if (ip >= end || !b.init(s + ip, end - ip)) return false;
            uint32_t sl = b.take((int)ll.log), so = b.take((int)of.log), sm = b.take((int)ml.log);
            for (uint32_t k = 0; k < nseq; ++k) {
                const uint32_t oc = of.e[so].sym, mc = ml.e[sm].sym, lc = ll.e[sl].sym;   // tables hold codes below 32, 53, 36
                const uint32_t ov = (1u << oc) + b.take((int)oc);
                const size_t mlen = kMLBase[mc] + b.take(kMLBits[mc]);
                const size_t llen = kLLBase[lc] + b.take(kLLBits[lc]);
                if (b.pos < 0) return false;
                uint32_t off;
                if (ov > 3) {
                    off = ov - 3;
                    rep[2] = rep[1]; rep[1] = rep[0]; rep[0] = off;
                } else {
                    const uint32_t idx = ov - 1 + (llen == 0 ? 1u : 0u);
                    if (idx == 0) {
                        off = rep[0];
                    } else {
                        off = idx < 3 ? rep[idx] : rep[0] - 1;
                        if (off == 0) return false;
                        if (idx > 1) rep[2] = rep[1];
                        rep[1] = rep[0];
                        rep[0] = off;
                    }
                }
                if (llen > nlit - lp || !room(llen)) return false;
                put_literals(llen);
                if (off > op || !room(mlen)) return false;
                for (size_t i = 0; i < mlen; ++i, ++op) d[op] = d[op - off];
                if (k + 1 < nseq) {
                    sl = ll.e[sl].base + b.take(ll.e[sl].nbits);
                    sm = ml.e[sm].base + b.take(ml.e[sm].nbits);
                    so = of.e[so].base + b.take(of.e[so].nbits);
                    if (b.pos < 0) return false;
                }
            }
            if (b.pos != 0) return false;
        }
        if (!room(nlit - lp)) return false;
        put_literals(nlit - lp);
        return op - op0 <= block_max;
    }

    bool frame() {
        if (len < 6) return false;
        if (s[0] != 0x28 || s[1] != 0xB5 || s[2] != 0x2F || s[3] != 0xFD) return false;
        const uint32_t fhd = s[4];
        size_t ip = 5;
        if (fhd & 0x08) return false;
        const bool single = fhd & 0x20, checksum = fhd & 0x04;
        uint64_t window = 0;
        if (!single) {
            if (ip >= len) return false;
            const uint32_t wd = s[ip++], wlog = 10 + (wd >> 3);
            if (wlog > 31) return false;
            window = (1ull << wlog) + ((1ull << wlog) >> 3) * (wd & 7);
        }
        const uint32_t did = fhd & 3, did_bytes = did == 3 ? 4 : did;
        if (len - ip < did_bytes) return false;
        for (uint32_t k = 0; k < did_bytes; ++k)
            if (s[ip++] != 0) return false;
        const uint32_t fcs_flag = fhd >> 6, fcs_bytes = fcs_flag == 0 ? (single ? 1 : 0) : 1u << fcs_flag;
        if (len - ip < fcs_bytes) return false;
        uint64_t fcs = 0;
        for (uint32_t k = 0; k < fcs_bytes; ++k) fcs |= (uint64_t)s[ip++] << (8 * k);
        if (fcs_bytes == 2) fcs += 256;
        form(single ? OMR_ZSTD_FORM_SINGLE_SEGMENT : OMR_ZSTD_FORM_WINDOWED);
        form(fcs_bytes == 0 ? OMR_ZSTD_FORM_FCS_ABSENT : fcs_bytes == 1 ? OMR_ZSTD_FORM_FCS_1 : fcs_bytes == 2 ? OMR_ZSTD_FORM_FCS_2
             : fcs_bytes == 4 ? OMR_ZSTD_FORM_FCS_4 : OMR_ZSTD_FORM_FCS_8);
        if (checksum) form(OMR_ZSTD_FORM_CHECKSUM);
        if (fcs_bytes && !grow && fcs != cap) return false;
        if (single) window = fcs;
        const size_t block_max = (size_t)std::min<uint64_t>(window, kBlockMax);
        int blocks = 0;
        for (;;) {
            if (len - ip < 3) return false;
            const uint32_t bh = s[ip] | (uint32_t)s[ip + 1] << 8 | (uint32_t)s[ip + 2] << 16;
            ip += 3;
            const uint32_t type = (bh >> 1) & 3;
            const size_t size = bh >> 3;
            if (type == 3 || size > block_max) return false;
            if (++blocks == 2) form(OMR_ZSTD_FORM_MULTI_BLOCK);
            form(OMR_ZSTD_FORM_BLOCK_RAW + (int)type);
            if (type == 0) {
                if (size > len - ip || !room(size)) return false;
                if (size) std::memcpy(d + op, s + ip, size);
                op += size;
                ip += size;
            } else if (type == 1) {
                if (len - ip < 1 || !room(size)) return false;
                if (size) std::memset(d + op, s[ip], size);
                ++ip;
                op += size;
            } else {
                if (size > len - ip || !block(ip, ip + size, block_max)) return false;
                ip += size;
            }
            if (bh & 1) break;
        }
        if (grow ? fcs_bytes && fcs != op : op != cap) return false;
        if (checksum) {
            if (len - ip < 4) return false;
            const uint32_t want = s[ip] | (uint32_t)s[ip + 1] << 8 | (uint32_t)s[ip + 2] << 16 | (uint32_t)s[ip + 3] << 24;
            ip += 4;
            if ((uint32_t)xxh64(d, op) != want) return false;
        }
        return ip == len;
    }

    static uint64_t rotl(uint64_t v, int r) { return v << r | v >> (64 - r); }
    static uint64_t rd64(const uint8_t* p) {
        uint64_t v = 0;
        for (int k = 0; k < 8; ++k) v |= (uint64_t)p[k] << (8 * k);
        return v;
    }
    static uint64_t xxh64(const uint8_t* p, size_t n) {
        const uint64_t P1 = 0x9E3779B185EBCA87ull, P2 = 0xC2B2AE3D27D4EB4Full, P3 = 0x165667B19E3779F9ull,
                       P4 = 0x85EBCA77C2B2AE63ull, P5 = 0x27D4EB2F165667C5ull;
        auto round = [&](uint64_t acc, uint64_t in) { return rotl(acc + in * P2, 31) * P1; };
        size_t i = 0;
        uint64_t h;
        if (n >= 32) {
            uint64_t v[4] = {P1 + P2, P2, 0, 0 - P1};
            for (; i + 32 <= n; i += 32)
                for (int k = 0; k < 4; ++k) v[k] = round(v[k], rd64(p + i + 8 * k));
            h = rotl(v[0], 1) + rotl(v[1], 7) + rotl(v[2], 12) + rotl(v[3], 18);
            for (int k = 0; k < 4; ++k) h = (h ^ round(0, v[k])) * P1 + P4;
        } else {
            h = P5;
        }
        h += (uint64_t)n;
        for (; i + 8 <= n; i += 8) h = rotl(h ^ round(0, rd64(p + i)), 27) * P1 + P4;
        if (i + 4 <= n) {
            const uint64_t w = p[i] | (uint64_t)p[i + 1] << 8 | (uint64_t)p[i + 2] << 16 | (uint64_t)p[i + 3] << 24;
            h = rotl(h ^ w * P1, 23) * P2 + P3;
            i += 4;
        }
        for (; i < n; ++i) h = rotl(h ^ p[i] * P5, 11) * P1;
        h ^= h >> 33;
        h *= P2;
        h ^= h >> 29;
        h *= P3;
        h ^= h >> 32;
        return h;
    }
};

}  // namespace

bool zstd_decode(const uint8_t* s, size_t len, uint8_t* d, size_t expected) {
    std::unique_ptr<Decoder> D(new Decoder{s, len, d, expected, nullptr, nullptr});
    D->litbuf.resize(kBlockMax);
    return D->frame();
}

}  // namespace omr

extern "C" {

omr_status omr_zstd_decode_host(const uint8_t* src, size_t length, uint8_t* dst, size_t expected) {
    if ((!src && length) || (!dst && expected)) return OMR_INVALID_ARGUMENT;
    return omr::zstd_decode(src, length, dst, expected) ? OMR_OK : OMR_INTERNAL;
}

omr_status omr_zstd_frame_forms(const uint8_t* src, size_t length, uint32_t* forms) {
    if ((!src && length) || !forms) return OMR_INVALID_ARGUMENT;
    for (int k = 0; k < OMR_ZSTD_FORM_WORDS; ++k) forms[k] = 0;
    uint32_t met[OMR_ZSTD_FORM_WORDS] = {0};
    std::vector<uint8_t> out((size_t)1 << 16);
    std::unique_ptr<omr::Decoder> D(new omr::Decoder{src, length, out.data(), out.size(), &out, met});
    D->litbuf.resize(omr::kBlockMax);
    if (!D->frame()) return OMR_INTERNAL;
    for (int k = 0; k < OMR_ZSTD_FORM_WORDS; ++k) forms[k] = met[k];
    return OMR_OK;
}

}  // extern "C"
