// omr_tiffread.cpp — K13, host half: tiled TIFF / OME-TIFF pixel data (include/omr/omr.h).
//
// The second backend of pixelsService.getPixelBuffer: pyramidal OME-TIFF
// as raw2ometiff writes it, one IFD per plane and the lower resolutions in SubIFDs.  This file
// holds the parser (pread, every offset bounds-checked: a file is user-uploaded data), the plain
// serial LZW decoder of the host route (omr_tiff_image_get_tile: the reference of the tests and
// the route of single reads) and what the device route needs to know of a TIFF (TiffSource): a
// segment's offset and byte count from the IFD tables, the rows of a short last strip, and the
// pread of the segments' bytes from the one file.  omr_tiff_image_open_ex widens what a file may
// use: Deflate and Zstandard segments (decoded on the host by omr_inflate_host and
// omr_zstd_decode_host, on the device by K14a and K16a), the floating-point predictor and chunky
// pixels of 2..4 samples, of which a read takes one, and baseline JPEG segments (Compression 7 with
// the JPEGTables of tag 347; omr_jpeg_decode_host here, K17a .. K17c on the device: omr_jpegdec.*)
// and JPEG 2000 codestreams (Compression 33003, 33004, 33005, 34712; the host decoder of
// omr_j2kdec.cpp here, K19a .. K19c and K20b on the device: omr_j2kdec.*), reversible ones with
// OMR_TIFF_ACCEPT_JPEG2000 and irreversible ones with OMR_TIFF_ACCEPT_JPEG2000_LOSSY.
// The device route itself -- staging, planning,
// K13a's and K13b's launches (omr_tiffread.hip), the tile renderer -- is omr_segread.cpp, shared
// with the Zarr reader; this file calls no HIP function.
#include "omr_segread.h"

#include "omr_j2kdec.h"
#include "omr_jpegdec.h"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cerrno>
#include <memory>
#include <unordered_set>

namespace {

constexpr uint64_t kMaxSegmentBytes = (uint64_t)256 << 20;   // decoded size of one segment
constexpr uint64_t kMaxStreamBytes = ((uint64_t)512 << 20) - 1;
constexpr uint32_t kMaxIfds = 1u << 20;
constexpr uint64_t kMaxJpegTables = 64u << 10;               // tag 347

struct Level {
    int32_t w = 0, h = 0;          // image size at this level
    int32_t seg_w = 0, seg_h = 0;  // tile size, or (w, rows per strip)
    int32_t across = 0, down = 0;
    bool tiled = false;
    bool operator==(const Level& o) const {
        return w == o.w && h == o.h && seg_w == o.seg_w && seg_h == o.seg_h && tiled == o.tiled;
    }
};

struct Segments {
    std::vector<uint64_t> off, cnt;   // [down][across]
    std::vector<uint8_t> jpeg_tables; // Compression 7: the IFD's JPEGTables stream (tag 347), if any
};

}  // namespace

struct omr_tiff_image {
    int fd = -1;
    uint64_t file_len = 0;
    bool big = false, bigtiff = false;
    int32_t sz = 0, sc = 0, st = 0;
    int64_t stride_z = 0, stride_c = 0, stride_t = 0;   // plane index = z*stride_z + c*stride_c + t*stride_t
    int32_t pt = 0, bpp = 0, compression = 1, predictor = 1;
    int32_t spp = 1;                                    // samples per pixel (chunky): channel c is sample c % spp
    bool jpeg_ycc = false;                              // Compression 7 with Photometric 6: YCbCr -> RGB on decode
    uint32_t j2k_kinds = 0;                             // JPEG 2000: the omr::kJ2kTake* transforms the open's accept bits allow
    std::vector<Level> levels;
    std::vector<std::vector<Segments>> segs;   // [plane][level]
    ~omr_tiff_image() {
        if (fd >= 0) ::close(fd);
    }
};

namespace {

// pread until done (short reads, EINTR).
bool read_full(int fd, void* dst, size_t n, uint64_t off) {
    uint8_t* d = static_cast<uint8_t*>(dst);
    while (n) {
        const ssize_t r = ::pread(fd, d, n, (off_t)off);
        if (r < 0) {
            if (errno == EINTR) continue;
            return false;
        }
        if (r == 0) return false;
        d += r;
        n -= (size_t)r;
        off += (uint64_t)r;
    }
    return true;
}

struct Ifd {
    uint64_t w = 0, h = 0, bps = 1, comp = 1, fill = 1, spp = 1, rps = 0xFFFFFFFFull, pred = 1, tw = 0, th = 0, fmt = 1;
    uint64_t photometric = 1, planar = 1;
    bool has_tw = false, has_th = false;
    bool mixed = false;            // BitsPerSample or SampleFormat differ between the samples of a pixel
    std::vector<uint64_t> strip_off, strip_cnt, tile_off, tile_cnt, sub;
    std::vector<uint8_t> jpeg_tables;
};

struct Parser {
    int fd;
    uint64_t len;
    bool big = false, bigtiff = false;

    bool rd(uint64_t off, void* dst, uint64_t n) const {
        if (off > len || n > len - off) return false;
        return n == 0 || read_full(fd, dst, (size_t)n, off);
    }
    uint64_t u(const uint8_t* p, int n) const {
        uint64_t v = 0;
        for (int k = 0; k < n; ++k) v = v << 8 | p[big ? k : n - 1 - k];
        return v;
    }
    // The values of one IFD entry (e: its 12 or 20 bytes).  OMR_INTERNAL: count or offset past the file.
    omr_status values(const uint8_t* e, std::vector<uint64_t>& out) const {
        const uint32_t type = (uint32_t)u(e + 2, 2);
        const uint64_t count = bigtiff ? u(e + 4, 8) : u(e + 4, 4);
        const uint8_t* field = e + (bigtiff ? 12 : 8);
        const int field_bytes = bigtiff ? 8 : 4;
        int ts;
        switch (type) {
        case 1: ts = 1; break;
        case 3: ts = 2; break;
        case 4: case 13: ts = 4; break;
        case 16: case 18: ts = 8; break;
        default: return OMR_INVALID_ARGUMENT;
        }
        if (count > len) return OMR_INTERNAL;           // count * ts <= 8 * len: no overflow below
        const uint64_t bytes = count * (uint64_t)ts;
        std::vector<uint8_t> buf;
        const uint8_t* src = field;
        if (bytes > (uint64_t)field_bytes) {
            buf.resize((size_t)bytes);
            if (!rd(u(field, field_bytes), buf.data(), bytes)) return OMR_INTERNAL;
            src = buf.data();
        }
        out.resize((size_t)count);
        for (uint64_t k = 0; k < count; ++k) out[(size_t)k] = u(src + k * ts, ts);
        return OMR_OK;
    }
    omr_status scalar(const uint8_t* e, uint64_t& v, bool* mixed = nullptr) const {
        std::vector<uint64_t> vals;
        const omr_status st = values(e, vals);
        if (st) return st;
        if (vals.empty()) return OMR_INTERNAL;
        v = vals[0];
        if (mixed)
            for (uint64_t o : vals) *mixed = *mixed || o != v;
        return OMR_OK;
    }
    // The bytes of a BYTE or UNDEFINED entry of at most `cap` values (JPEGTables).
    omr_status bytes(const uint8_t* e, uint64_t cap, std::vector<uint8_t>& out) const {
        const uint32_t type = (uint32_t)u(e + 2, 2);
        const uint64_t count = bigtiff ? u(e + 4, 8) : u(e + 4, 4);
        const uint8_t* field = e + (bigtiff ? 12 : 8);
        const int field_bytes = bigtiff ? 8 : 4;
        if (type != 1 && type != 7) return OMR_INVALID_ARGUMENT;
        if (count > cap) return OMR_INVALID_ARGUMENT;
        out.resize((size_t)count);
        if (count <= (uint64_t)field_bytes) {
            std::memcpy(out.data(), field, (size_t)count);
            return OMR_OK;
        }
        return rd(u(field, field_bytes), out.data(), count) ? OMR_OK : OMR_INTERNAL;
    }
    // Entry count and the offset of the next IFD; with `ifd`, the tags too.
    omr_status read_ifd(uint64_t off, Ifd* ifd, uint64_t& next) const {
        uint8_t head[8];
        const int cb = bigtiff ? 8 : 2, es = bigtiff ? 20 : 12, nb = bigtiff ? 8 : 4;
        if (!rd(off, head, (uint64_t)cb)) return OMR_INTERNAL;
        const uint64_t n = u(head, cb);
        if (n > len / (uint64_t)es) return OMR_INTERNAL;
        const uint64_t body = n * (uint64_t)es;
        uint8_t nx[8];
        if (!rd(off + (uint64_t)cb + body, nx, (uint64_t)nb)) return OMR_INTERNAL;   // off + cb <= len (rd above)
        next = u(nx, nb);
        if (!ifd) return OMR_OK;
        std::vector<uint8_t> ent((size_t)body);
        if (!rd(off + (uint64_t)cb, ent.data(), body)) return OMR_INTERNAL;
        for (uint64_t k = 0; k < n; ++k) {
            const uint8_t* e = ent.data() + k * es;
            omr_status st = OMR_OK;
            switch ((uint32_t)u(e, 2)) {
            case 256: st = scalar(e, ifd->w); break;
            case 257: st = scalar(e, ifd->h); break;
            case 258: st = scalar(e, ifd->bps, &ifd->mixed); break;
            case 259: st = scalar(e, ifd->comp); break;
            case 262: st = scalar(e, ifd->photometric); break;
            case 266: st = scalar(e, ifd->fill); break;
            case 273: st = values(e, ifd->strip_off); break;
            case 277: st = scalar(e, ifd->spp); break;
            case 278: st = scalar(e, ifd->rps); break;
            case 279: st = values(e, ifd->strip_cnt); break;
            case 284: st = scalar(e, ifd->planar); break;
            case 317: st = scalar(e, ifd->pred); break;
            case 322: st = scalar(e, ifd->tw); ifd->has_tw = true; break;
            case 323: st = scalar(e, ifd->th); ifd->has_th = true; break;
            case 324: st = values(e, ifd->tile_off); break;
            case 325: st = values(e, ifd->tile_cnt); break;
            case 330: st = values(e, ifd->sub); break;
            case 339: st = scalar(e, ifd->fmt, &ifd->mixed); break;
            case 347: st = bytes(e, kMaxJpegTables, ifd->jpeg_tables); break;
            default: break;
            }
            if (st) return st;
        }
        return OMR_OK;
    }
};

int pixel_type_of(uint64_t bps, uint64_t fmt) {
    if (fmt == 1) return bps == 8 ? OMR_PIXELS_UINT8 : bps == 16 ? OMR_PIXELS_UINT16 : bps == 32 ? OMR_PIXELS_UINT32 : -1;
    if (fmt == 2) return bps == 8 ? OMR_PIXELS_INT8 : bps == 16 ? OMR_PIXELS_INT16 : bps == 32 ? OMR_PIXELS_INT32 : -1;
    if (fmt == 3) return bps == 32 ? OMR_PIXELS_FLOAT : bps == 64 ? OMR_PIXELS_DOUBLE : -1;
    return -1;
}

// Rows of segment row sy (the last strip of an image is short; tiles are stored whole).
inline int32_t rows_in_segment(const Level& L, int32_t sy) {
    return L.tiled ? L.seg_h : std::min(L.seg_h, L.h - sy * L.seg_h);
}

// One IFD into the image: geometry, format and the segment table, all checked.
// accept: the OMR_TIFF_ACCEPT_* bits of the open; a feature the file uses without its bit is refused.
omr_status take_ifd(const Parser& P, const Ifd& f, uint32_t accept, Level& L, Segments& S, int32_t& pt, int32_t& comp,
                    int32_t& pred, int32_t& spp, bool& ycc) {
    if (f.fill != 1) return OMR_INVALID_ARGUMENT;
    if (f.spp != 1) {
        if (!(accept & OMR_TIFF_ACCEPT_SAMPLES) || f.spp < 1 || f.spp > 4) return OMR_INVALID_ARGUMENT;
        if (f.planar != 1 || (f.photometric == 6 && f.comp != 7) || f.mixed) return OMR_INVALID_ARGUMENT;
    }
    ycc = false;
    switch (f.comp) {
    case 1: case 5: comp = (int32_t)f.comp; break;
    case 8: case 32946:
        if (!(accept & OMR_TIFF_ACCEPT_DEFLATE)) return OMR_INVALID_ARGUMENT;
        comp = 8;
        break;
    case 50000:
        if (!(accept & OMR_TIFF_ACCEPT_ZSTD)) return OMR_INVALID_ARGUMENT;
        comp = 50000;
        break;
    case 7:                                              // one baseline JPEG stream per segment (K17)
        if (!(accept & OMR_TIFF_ACCEPT_JPEG)) return OMR_INVALID_ARGUMENT;
        if (f.bps != 8 || f.fmt != 1 || f.pred != 1 || f.mixed) return OMR_INVALID_ARGUMENT;
        if (f.spp == 1 ? f.photometric > 1 : f.spp != 3 || (f.photometric != 2 && f.photometric != 6)) return OMR_INVALID_ARGUMENT;
        ycc = f.photometric == 6;
        comp = 7;
        break;
    case 33003: case 33004: case 33005: case 34712:      // one JPEG 2000 codestream per segment (K19; K20: irreversible ones)
        if (!(accept & (OMR_TIFF_ACCEPT_JPEG2000 | OMR_TIFF_ACCEPT_JPEG2000_LOSSY))) return OMR_INVALID_ARGUMENT;
        if (f.fmt != 1 || f.pred != 1 || f.mixed) return OMR_INVALID_ARGUMENT;
        if (f.bps == 8 ? (f.spp == 1 ? f.photometric > 1 : f.spp != 3 || f.photometric != 2) : f.bps != 16 || f.spp != 1 || f.photometric > 1)
            return OMR_INVALID_ARGUMENT;
        comp = 34712;
        break;
    default: return OMR_INVALID_ARGUMENT;
    }
    if (f.pred == 3) {                                   // float and double, one sample per pixel
        if (!(accept & OMR_TIFF_ACCEPT_PREDICTOR3) || f.fmt != 3 || f.spp != 1) return OMR_INVALID_ARGUMENT;
    } else if (f.pred != 1 && f.pred != 2) {
        return OMR_INVALID_ARGUMENT;
    }
    pt = pixel_type_of(f.bps, f.fmt);
    if (pt < 0) return OMR_INVALID_ARGUMENT;
    if (f.pred == 2 && f.bps == 64) return OMR_INVALID_ARGUMENT;
    if (f.w < 1 || f.h < 1 || f.w > 0x7FFFFFFFull || f.h > 0x7FFFFFFFull) return OMR_INVALID_ARGUMENT;
    pred = (int32_t)f.pred;
    spp = (int32_t)f.spp;
    const uint64_t bpp = f.bps / 8 * f.spp;              // bytes per pixel, all samples
    L.w = (int32_t)f.w;
    L.h = (int32_t)f.h;
    const std::vector<uint64_t>*off, *cnt;
    if (f.has_tw || f.has_th || !f.tile_off.empty()) {
        if (f.tw < 1 || f.th < 1 || f.tw > 0x7FFFFFFFull || f.th > 0x7FFFFFFFull) return OMR_INTERNAL;
        L.tiled = true;
        L.seg_w = (int32_t)f.tw;
        L.seg_h = (int32_t)f.th;
        off = &f.tile_off;
        cnt = &f.tile_cnt;
    } else {
        if (f.rps < 1) return OMR_INTERNAL;
        L.tiled = false;
        L.seg_w = L.w;
        L.seg_h = (int32_t)std::min<uint64_t>(f.rps, f.h);
        off = &f.strip_off;
        cnt = &f.strip_cnt;
    }
    L.across = (int32_t)((f.w + (uint64_t)L.seg_w - 1) / (uint64_t)L.seg_w);
    L.down = (int32_t)((f.h + (uint64_t)L.seg_h - 1) / (uint64_t)L.seg_h);
    uint64_t n_seg, seg_bytes;
    if (__builtin_mul_overflow((uint64_t)L.across, (uint64_t)L.down, &n_seg)) return OMR_INTERNAL;
    if (__builtin_mul_overflow((uint64_t)L.seg_w, (uint64_t)L.seg_h, &seg_bytes) ||
        __builtin_mul_overflow(seg_bytes, bpp, &seg_bytes))
        return OMR_INTERNAL;
    if (off->size() != n_seg || cnt->size() != n_seg) return OMR_INTERNAL;
    if (seg_bytes > kMaxSegmentBytes) return OMR_INVALID_ARGUMENT;
    for (uint64_t k = 0; k < n_seg; ++k) {
        const uint64_t o = (*off)[(size_t)k], c = (*cnt)[(size_t)k];
        if (c == 0) continue;                                        // reads as zeros
        if (o > P.len || c > P.len - o) return OMR_INTERNAL;
        if (comp == 1) {
            const uint64_t need = (uint64_t)rows_in_segment(L, (int32_t)(k / (uint64_t)L.across)) * L.seg_w * bpp;
            if (c < need) return OMR_INTERNAL;
        } else if (c > kMaxStreamBytes) {
            return OMR_INVALID_ARGUMENT;
        }
    }
    S.off = *off;
    S.cnt = *cnt;
    if (comp == 7) S.jpeg_tables = f.jpeg_tables;
    return OMR_OK;
}

// TIFF LZW, serial (the rules: omr.h at omr_tiff_image_get_tile).  true: exactly `expected` bytes out.
bool lzw_decode(const uint8_t* s, size_t len, uint8_t* d, size_t expected) {
    if (len >= 2 && s[0] == 0 && (s[1] & 1)) return false;   // old-style LSB-first stream
    uint16_t prefix[4096], length[4096];
    uint8_t suffix[4096], first[4096];
    const uint64_t nbits = (uint64_t)len * 8;
    uint64_t bit = 0;
    uint32_t next = 258, width = 9;
    int32_t prev = -1;
    size_t out = 0;
    auto len_of = [&](uint32_t c) -> uint32_t { return c < 256 ? 1u : length[c]; };
    auto first_of = [&](uint32_t c) -> uint8_t { return c < 256 ? (uint8_t)c : first[c]; };
    while (out < expected) {
        if (bit + width > nbits) return false;                // the stream ends early
        const uint64_t b = bit >> 3;
        uint32_t v = (uint32_t)s[b] << 16;
        if (b + 1 < len) v |= (uint32_t)s[b + 1] << 8;
        if (b + 2 < len) v |= (uint32_t)s[b + 2];
        const uint32_t code = (v >> (24 - width - (uint32_t)(bit & 7))) & ((1u << width) - 1);
        bit += width;
        if (code == 256) {
            next = 258;
            width = 9;
            prev = -1;
            continue;
        }
        if (code == 257) return false;                        // EOI before the segment is full
        uint32_t n;        // length of this code's string
        uint8_t f;         // and its first byte
        if (prev < 0) {
            if (code > 255) return false;
            n = 1;
            f = (uint8_t)code;
        } else if (code < next) {
            n = len_of(code);
            f = first_of(code);
        } else if (code == next && next < 4096) {             // the string of prev + its own first byte
            n = len_of((uint32_t)prev) + 1;
            f = first_of((uint32_t)prev);
        } else {
            return false;                                     // a code above the next free entry
        }
        if (prev >= 0 && next < 4096) {
            prefix[next] = (uint16_t)prev;
            suffix[next] = f;
            length[next] = (uint16_t)(len_of((uint32_t)prev) + 1);
            first[next] = first_of((uint32_t)prev);
            ++next;
            width = next < 511 ? 9 : next < 1023 ? 10 : next < 2047 ? 11 : 12;
        }
        size_t p = out + n;                                   // backwards along the prefix chain
        uint32_t c = code;
        for (uint32_t k = n; k > 1; --k) {
            --p;
            if (p < expected) d[p] = suffix[c];
            c = prefix[c];
        }
        --p;
        if (p < expected) d[p] = (uint8_t)c;
        out += n;
        prev = (int32_t)code;
    }
    return true;
}

template <typename T>
T swap_bytes(T v) {
    if (sizeof(T) == 2) return (T)__builtin_bswap16((uint16_t)v);
    if (sizeof(T) == 4) return (T)__builtin_bswap32((uint32_t)v);
    return v;
}

// Undo predictor 2 on `rows` rows of `w` pixels of spp samples: running sums per component (spp
// samples apart) in the sample's own width.
template <typename T>
void unpredict(uint8_t* buf, int64_t rows, int64_t w, int64_t spp, bool swap) {
    for (int64_t r = 0; r < rows; ++r) {
        uint8_t* row = buf + (size_t)(r * w * spp) * sizeof(T);
        T acc[4] = {0, 0, 0, 0};
        for (int64_t x = 0; x < w * spp; ++x) {
            T v;
            std::memcpy(&v, row + x * sizeof(T), sizeof(T));
            if (swap) v = swap_bytes(v);
            T& a = acc[x % spp];
            a = (T)(a + v);
            v = swap ? swap_bytes(a) : a;
            std::memcpy(row + x * sizeof(T), &v, sizeof(T));
        }
    }
}

// Undo predictor 3 (libtiff's fpAcc) on `rows` rows of `w` samples of B bytes: the running byte sum
// over the row's w * B bytes gives B planes of w bytes, the most significant first; sample x is
// their bytes at x, put back in the file's byte order.
void unpredict_fp(uint8_t* buf, int64_t rows, int64_t w, int64_t B, bool big, std::vector<uint8_t>& tmp) {
    tmp.resize((size_t)(w * B));
    for (int64_t r = 0; r < rows; ++r) {
        uint8_t* row = buf + (size_t)(r * w * B);
        uint8_t acc = 0;
        for (int64_t k = 0; k < w * B; ++k) tmp[(size_t)k] = acc = (uint8_t)(acc + row[k]);
        for (int64_t x = 0; x < w; ++x)
            for (int64_t b = 0; b < B; ++b) row[x * B + (big ? b : B - 1 - b)] = tmp[(size_t)(b * w + x)];
    }
}

bool host_little_endian() {
    const uint16_t one = 1;
    uint8_t b;
    std::memcpy(&b, &one, 1);
    return b == 1;
}

// The IFD of channel c: the spp channels of one chunky pixel share it.
int64_t plane_index(const omr_tiff_image* im, int32_t z, int32_t c, int32_t t) {
    return z * im->stride_z + (c / im->spp) * im->stride_c + t * im->stride_t;
}

// "XY" and a permutation of Z, C, T: the first of the three varies fastest along the IFD chain,
// which holds c_planes = size_c / spp IFDs per (z, t).
bool set_strides(omr_tiff_image* im, const char* order, int32_t c_planes) {
    if (std::strlen(order) != 5 || order[0] != 'X' || order[1] != 'Y') return false;
    im->stride_z = im->stride_c = im->stride_t = 0;
    int64_t stride = 1;
    for (int k = 2; k < 5; ++k) {
        switch (order[k]) {
        case 'Z': if (im->stride_z) return false; im->stride_z = stride; stride *= im->sz; break;
        case 'C': if (im->stride_c) return false; im->stride_c = stride; stride *= c_planes; break;
        case 'T': if (im->stride_t) return false; im->stride_t = stride; stride *= im->st; break;
        default: return false;
        }
    }
    return true;
}

bool region_in_bounds(const omr_tiff_image* im, const Level& L, int32_t z, int32_t c, int32_t t, int32_t x, int32_t y,
                      int32_t w, int32_t h) {
    return z >= 0 && z < im->sz && c >= 0 && c < im->sc && t >= 0 && t < im->st && x >= 0 && y >= 0 && w >= 0 &&
           h >= 0 && (int64_t)x + w <= L.w && (int64_t)y + h <= L.h;
}

// Segment (sx, sy) of a plane, decoded and with the predictor undone: rows * seg_w pixels of spp
// samples.  A Deflate or zstd segment must decode to exactly that (omr_inflate_host,
// omr_zstd_decode_host); an LZW string that overruns it is cut.
omr_status load_segment(const omr_tiff_image* im, const Level& L, const Segments& S, int32_t sx, int32_t sy,
                        std::vector<uint8_t>& comp, std::vector<uint8_t>& out) {
    const size_t k = (size_t)sy * L.across + sx;
    const int32_t rows = rows_in_segment(L, sy);
    const size_t expected = (size_t)rows * L.seg_w * im->bpp * im->spp;
    out.assign(expected, 0);
    const uint64_t cnt = S.cnt[k];
    if (cnt == 0) return OMR_OK;
    if (im->compression == 1) {
        if (!read_full(im->fd, out.data(), expected, S.off[k])) return OMR_INTERNAL;
    } else {
        comp.resize((size_t)cnt);
        if (!read_full(im->fd, comp.data(), (size_t)cnt, S.off[k])) return OMR_INTERNAL;
        bool ok;
        switch (im->compression) {
        case 5: ok = lzw_decode(comp.data(), (size_t)cnt, out.data(), expected); break;
        case 8: ok = omr_inflate_host(comp.data(), (size_t)cnt, out.data(), expected) == OMR_OK; break;
        case 50000: ok = omr_zstd_decode_host(comp.data(), (size_t)cnt, out.data(), expected) == OMR_OK; break;
        case 7: {
            const omr_status st = omr_jpeg_decode_host(S.jpeg_tables.empty() ? nullptr : S.jpeg_tables.data(), S.jpeg_tables.size(),
                                                       comp.data(), (size_t)cnt, L.seg_w, rows, im->spp, im->jpeg_ycc,
                                                       out.data(), nullptr, 0);
            if (st == OMR_INVALID_ARGUMENT) return st;      // a valid form out of scope
            ok = st == OMR_OK;
            break;
        }
        case 34712: {
            const omr_status st = omr::j2k_decode_host_kinds(comp.data(), (size_t)cnt, L.seg_w, rows, im->spp, 8 * im->bpp, out.data(),
                                                             im->j2k_kinds, nullptr);
            if (st == OMR_INVALID_ARGUMENT) return st;      // a valid form out of scope
            ok = st == OMR_OK;
            if (ok && im->bpp == 2 && im->big == host_little_endian())   // the decoder's samples are the host's: into the file's order
                for (size_t k = 0; k + 1 < expected; k += 2) std::swap(out[k], out[k + 1]);
            break;
        }
        default: ok = false; break;
        }
        if (!ok) return OMR_INTERNAL;
    }
    if (im->predictor == 2) {
        const bool swap = im->big == host_little_endian();
        if (im->bpp == 1) unpredict<uint8_t>(out.data(), rows, L.seg_w, im->spp, false);
        else if (im->bpp == 2) unpredict<uint16_t>(out.data(), rows, L.seg_w, im->spp, swap);
        else if (im->bpp == 4) unpredict<uint32_t>(out.data(), rows, L.seg_w, im->spp, swap);
    } else if (im->predictor == 3) {
        unpredict_fp(out.data(), rows, L.seg_w, im->bpp, im->big, comp);
    }
    return OMR_OK;
}

// ---- device route: what the shared pipeline (omr_segread.h) asks of a TIFF ---------------------------

struct TiffSource final : omr::SegSource {
    const omr_tiff_image* im;
    size_t level;
    TiffSource(const omr_tiff_image* img, int32_t lv) : im(img), level((size_t)lv) {
        kind = omr::SegKind::tiff;
        tag = "tiff";
        noun = "segment";
        if (lv < 0 || level >= im->levels.size()) return;   // the checks of the entry points refuse it (dims())
        const Level& L = im->levels[level];
        geom.seg_w = L.seg_w; geom.seg_h = L.seg_h; geom.across = L.across; geom.down = L.down; geom.bpp = im->bpp;
        geom.spp = im->spp;
        switch (im->compression) {                        // K13a, K14a, K16a
        case 5: codec = omr::SegCodec::lzw; break;
        case 8: codec = omr::SegCodec::zlib; break;
        case 50000: codec = omr::SegCodec::zstd; break;
        case 7: codec = omr::SegCodec::jpeg; break;
        case 34712: codec = omr::SegCodec::j2k; break;
        default: codec = omr::SegCodec::none; break;
        }
        predictor = im->predictor;
        swap = im->big == host_little_endian();
        pt = im->pt; big = im->big;
        jpeg_ycc = im->jpeg_ycc;
        j2k_kinds = im->j2k_kinds;
    }
    omr::SegImageDims dims() const {
        return {(int32_t)level, (int32_t)im->levels.size(), im->bpp, im->sc,
                [this](const omr_raw_tile_request& r, int32_t w, int32_t h) {
                    return region_in_bounds(im, im->levels[level], r.z, r.c, r.t, r.x, r.y, w, h);
                }};
    }
    const uint8_t* jpeg_tables(const omr::SegKey& k, size_t* len) const override {
        const std::vector<uint8_t>& t = table(k).jpeg_tables;
        *len = t.size();
        return t.empty() ? nullptr : t.data();
    }
    const Segments& table(const omr::SegKey& k) const { return im->segs[(size_t)k.plane][level]; }
    size_t slot(const omr::SegKey& k) const { return (size_t)k.sy * geom.across + k.sx; }
    int64_t plane_of(const omr_raw_tile_request& r) const override { return plane_index(im, r.z, r.c, r.t); }
    int32_t sample_of(const omr_raw_tile_request& r) const override { return r.c % im->spp; }
    omr_status sizes(omr::Ctx*, const std::vector<omr::SegKey>& keys, std::vector<omr::SegBytes>& out) override {
        for (size_t k = 0; k < keys.size(); ++k) {
            out[k].expected =
                (uint32_t)((size_t)rows_in_segment(im->levels[level], keys[k].sy) * geom.seg_w * geom.bpp * geom.spp);
            out[k].cnt = table(keys[k]).cnt[slot(keys[k])];
            if (out[k].cnt && codec == omr::SegCodec::none) out[k].cnt = out[k].expected;   // the stored bytes we need
        }
        return OMR_OK;
    }
    bool read(const std::vector<omr::SegKey>& keys, const std::vector<omr::SegBytes>& segs, uint8_t* pin, size_t in_bytes) override {
        std::atomic<bool> io_error{false};
        omr::parallel_for((int)segs.size(), in_bytes > ((size_t)4 << 20), [&](int k) {
            const omr::SegBytes& u = segs[(size_t)k];
            const omr::SegKey& key = keys[(size_t)k];
            if (u.cnt && !read_full(im->fd, pin + u.in_off, (size_t)u.cnt, table(key).off[slot(key)])) io_error = true;
        });
        return !io_error;
    }
};

}  // namespace

using namespace omr;

extern "C" {

omr_status omr_tiff_image_open(const char* path, int32_t size_z, int32_t size_c, int32_t size_t_,
                               const char* dimension_order, omr_tiff_image** out) {
    return omr_tiff_image_open_ex(path, size_z, size_c, size_t_, dimension_order, nullptr, out);
}

omr_status omr_tiff_image_open_ex(const char* path, int32_t size_z, int32_t size_c, int32_t size_t_,
                                  const char* dimension_order, const omr_tiff_open_options* opt, omr_tiff_image** out) {
    if (!out) return OMR_INVALID_ARGUMENT;
    *out = nullptr;
    uint32_t accept = 0;
    if (opt) {
        if (opt->struct_size < sizeof(omr_tiff_open_options)) return OMR_INVALID_ARGUMENT;
        accept = opt->accept;
        if (accept & ~(OMR_TIFF_ACCEPT_DEFLATE | OMR_TIFF_ACCEPT_ZSTD | OMR_TIFF_ACCEPT_PREDICTOR3 | OMR_TIFF_ACCEPT_SAMPLES |
                       OMR_TIFF_ACCEPT_JPEG | OMR_TIFF_ACCEPT_JPEG2000 | OMR_TIFF_ACCEPT_JPEG2000_LOSSY))
            return OMR_INVALID_ARGUMENT;
    }
    if (!path || !dimension_order || size_z <= 0 || size_c <= 0 || size_t_ <= 0) return OMR_INVALID_ARGUMENT;
    int64_t n_planes = size_z;
    if (__builtin_mul_overflow(n_planes, (int64_t)size_c, &n_planes) ||
        __builtin_mul_overflow(n_planes, (int64_t)size_t_, &n_planes) || n_planes > (int64_t)kMaxIfds)
        return OMR_INVALID_ARGUMENT;
    std::unique_ptr<omr_tiff_image> im(new omr_tiff_image);
    im->sz = size_z; im->sc = size_c; im->st = size_t_;
    im->j2k_kinds = ((accept & OMR_TIFF_ACCEPT_JPEG2000) ? omr::kJ2kTakeReversible : 0u) |
                    ((accept & OMR_TIFF_ACCEPT_JPEG2000_LOSSY) ? omr::kJ2kTakeIrreversible : 0u);
    if (!set_strides(im.get(), dimension_order, size_c)) return OMR_INVALID_ARGUMENT;   // again below, once spp is known
    im->fd = ::open(path, O_RDONLY | O_CLOEXEC);
    if (im->fd < 0) return errno == ENOENT ? OMR_NOT_FOUND : OMR_INVALID_ARGUMENT;
    struct stat sb;
    if (::fstat(im->fd, &sb) != 0 || !S_ISREG(sb.st_mode)) return OMR_INVALID_ARGUMENT;
    Parser P{im->fd, (uint64_t)sb.st_size};
    im->file_len = P.len;
    uint8_t hdr[16];
    if (!P.rd(0, hdr, 8)) return OMR_INTERNAL;
    if (hdr[0] == 'I' && hdr[1] == 'I') P.big = false;
    else if (hdr[0] == 'M' && hdr[1] == 'M') P.big = true;
    else return OMR_INVALID_ARGUMENT;
    const uint64_t magic = P.u(hdr + 2, 2);
    uint64_t ifd_off;
    if (magic == 42) {
        ifd_off = P.u(hdr + 4, 4);
    } else if (magic == 43) {
        P.bigtiff = true;
        if (!P.rd(0, hdr, 16)) return OMR_INTERNAL;
        if (P.u(hdr + 4, 2) != 8 || P.u(hdr + 6, 2) != 0) return OMR_INVALID_ARGUMENT;
        ifd_off = P.u(hdr + 8, 8);
    } else {
        return OMR_INVALID_ARGUMENT;
    }
    im->big = P.big;
    im->bigtiff = P.bigtiff;

    std::unordered_set<uint64_t> seen;
    int64_t n_ifds = 0;
    bool first = true;
    while (ifd_off != 0) {
        if (!seen.insert(ifd_off).second || seen.size() > kMaxIfds) return OMR_INTERNAL;   // the chain loops
        uint64_t next = 0;
        if (n_ifds >= n_planes) {                        // behind the planes: only walk the chain
            const omr_status st = P.read_ifd(ifd_off, nullptr, next);
            if (st) return st;
            ++n_ifds;
            ifd_off = next;
            continue;
        }
        Ifd main;
        omr_status st = P.read_ifd(ifd_off, &main, next);
        if (st) return st;
        std::vector<Level> lv(1 + main.sub.size());
        std::vector<Segments> sg(1 + main.sub.size());
        for (size_t k = 0; k < lv.size(); ++k) {
            Ifd sub;
            if (k > 0) {
                uint64_t ignored = 0;
                if (!seen.insert(main.sub[k - 1]).second || seen.size() > kMaxIfds) return OMR_INTERNAL;
                st = P.read_ifd(main.sub[k - 1], &sub, ignored);
                if (st) return st;
            }
            int32_t pt = 0, comp = 0, pred = 0, spp = 1;
            bool ycc = false;
            st = take_ifd(P, k ? sub : main, accept, lv[k], sg[k], pt, comp, pred, spp, ycc);
            if (st) return st;
            if (first) {
                im->pt = pt;
                im->bpp = bytes_per_pixel(pt);
                im->compression = comp;
                im->predictor = pred;
                im->spp = spp;
                im->jpeg_ycc = ycc;
                first = false;
                if (spp > 1) {                           // the chain holds Z * (C / spp) * T IFDs
                    if (size_c % spp) return OMR_INVALID_ARGUMENT;
                    n_planes = n_planes / size_c * (size_c / spp);
                    (void)set_strides(im.get(), dimension_order, size_c / spp);
                }
            } else if (pt != im->pt || comp != im->compression || pred != im->predictor || spp != im->spp || ycc != im->jpeg_ycc) {
                return OMR_INVALID_ARGUMENT;             // planes or levels that disagree
            }
        }
        if (n_ifds == 0) im->levels = lv;
        else if (!(lv == im->levels)) return OMR_INVALID_ARGUMENT;
        im->segs.push_back(std::move(sg));
        ++n_ifds;
        ifd_off = next;
    }
    if (n_ifds < n_planes) return OMR_INVALID_ARGUMENT;
    *out = im.release();
    return OMR_OK;
}

void omr_tiff_image_close(omr_tiff_image* img) { delete img; }

int32_t omr_tiff_image_samples_per_pixel(const omr_tiff_image* img) { return img ? img->spp : -(int32_t)OMR_INVALID_ARGUMENT; }

omr_status omr_tiff_image_info(const omr_tiff_image* img, omr_tiff_info* info) {
    if (!img || !info) return OMR_INVALID_ARGUMENT;
    const Level& L = img->levels[0];
    info->size_x = L.w; info->size_y = L.h;
    info->size_z = img->sz; info->size_c = img->sc; info->size_t_ = img->st;
    info->pixel_type = img->pt;
    info->big_endian = img->big;
    info->n_levels = (int32_t)img->levels.size();
    info->compression = img->compression;
    info->predictor = img->predictor;
    info->tiled = L.tiled;
    info->segment_width = L.seg_w;
    info->segment_height = L.seg_h;
    info->big_tiff = img->bigtiff;
    return OMR_OK;
}

int32_t omr_tiff_image_level_sizes(const omr_tiff_image* img, int32_t* sizes_out, int32_t cap_pairs) {
    if (!img || (!sizes_out && cap_pairs > 0)) return -(int32_t)OMR_INVALID_ARGUMENT;
    const int32_t n = (int32_t)img->levels.size();
    for (int32_t k = 0; k < n && k < cap_pairs; ++k) {
        sizes_out[2 * k] = img->levels[(size_t)k].w;
        sizes_out[2 * k + 1] = img->levels[(size_t)k].h;
    }
    return n;
}

omr_status omr_lzw_decode_host(const uint8_t* src, size_t length, uint8_t* dst, size_t expected) {
    if ((!src && length) || (!dst && expected)) return OMR_INVALID_ARGUMENT;
    return lzw_decode(src, length, dst, expected) ? OMR_OK : OMR_INTERNAL;
}

omr_status omr_tiff_image_get_tile(const omr_tiff_image* img, int32_t level, int32_t z, int32_t c, int32_t t,
                                   int32_t x, int32_t y, int32_t w, int32_t h, void* dst, size_t cap) {
    if (!img || !dst || level < 0 || level >= (int32_t)img->levels.size()) return OMR_INVALID_ARGUMENT;
    const Level& L = img->levels[(size_t)level];
    if (!region_in_bounds(img, L, z, c, t, x, y, w, h)) return OMR_INVALID_ARGUMENT;   // DimensionsOutOfBounds
    if (cap < (size_t)w * h * img->bpp) return OMR_BUFFER_TOO_SMALL;
    if (w == 0 || h == 0) return OMR_OK;
    const Segments& S = img->segs[(size_t)plane_index(img, z, c, t)][(size_t)level];
    std::vector<uint8_t> comp, seg;
    uint8_t* out = static_cast<uint8_t*>(dst);
    const size_t bpp = (size_t)img->bpp, spp = (size_t)img->spp, sample = (size_t)(c % img->spp);
    for (int32_t sy = y / L.seg_h; sy <= (y + h - 1) / L.seg_h; ++sy)
        for (int32_t sx = x / L.seg_w; sx <= (x + w - 1) / L.seg_w; ++sx) {
            const omr_status st = load_segment(img, L, S, sx, sy, comp, seg);
            if (st) return st;
            const int32_t ox = sx * L.seg_w, oy = sy * L.seg_h;
            const int32_t X0 = std::max(x, ox), X1 = std::min(x + w, ox + L.seg_w);
            const int32_t Y0 = std::max(y, oy), Y1 = std::min(y + h, oy + L.seg_h);
            for (int32_t yy = Y0; yy < Y1; ++yy) {
                uint8_t* d = out + ((size_t)(yy - y) * w + (X0 - x)) * bpp;
                const uint8_t* s = seg.data() + (((size_t)(yy - oy) * L.seg_w + (X0 - ox)) * spp + sample) * bpp;
                if (spp == 1) std::memcpy(d, s, (size_t)(X1 - X0) * bpp);
                else                                        // the one sample out of each chunky pixel
                    for (int32_t xx = 0; xx < X1 - X0; ++xx) std::memcpy(d + (size_t)xx * bpp, s + (size_t)xx * spp * bpp, bpp);
            }
        }
    return OMR_OK;
}

omr_status omr_tiff_image_read_regions_device(omr_ctx* ctx, const omr_tiff_image* img, int32_t level,
                                              const omr_raw_tile_request* reqs, int32_t n, int32_t width,
                                              int32_t height, void* d_dst, int64_t region_stride_bytes) {
    if (!ctx) return OMR_INVALID_ARGUMENT;
    if (!img) return fail(ctx, OMR_INVALID_ARGUMENT, "tiff: null argument");
    TiffSource src(img, level);
    return read_regions_checked(ctx, src, src.dims(), reqs, n, width, height, d_dst, region_stride_bytes);
}

omr_status omr_render_tiff_tiles(omr_ctx* ctx, const omr_tiff_image* img, int32_t level, const omr_quantum_def* qdef,
                                 const omr_channel_binding* channels, int32_t size_c, const omr_tile_request* reqs,
                                 int32_t n, int32_t width, int32_t height, int32_t flip_h, int32_t flip_v,
                                 uint32_t* argb_out, int32_t out_on_device) {
    if (!ctx) return OMR_INVALID_ARGUMENT;
    if (!img) return fail(ctx, OMR_INVALID_ARGUMENT, "null argument");
    TiffSource src(img, level);
    return render_tiles_checked(ctx, src, src.dims(), qdef, channels, size_c, reqs, n, width, height, flip_h, flip_v, argb_out,
                                out_on_device);
}

}  // extern "C"
