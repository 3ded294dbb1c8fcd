// omr_zarr.cpp — K14, host half: OME-Zarr pixel data (include/omr/omr.h).
//
// The third backend of pixelsService.getPixelBuffer: a Zarr v2 directory as bioformats2raw writes
// it, one 5-D TCZYX array per resolution and one file per chunk.  This file holds the small JSON
// reader of the metadata (.zattrs, .zarray: user-uploaded data, so it has a depth and a length
// limit and never reads past its buffer), the image model, the plain serial inflate of the host
// route (omr_inflate_host, omr_zarr_image_get_tile: the reference of the tests and the route of
// single reads) and the staging of the device route: the chunks the requested regions touch are
// listed once each, their files go to pinned memory and in one copy to the device with the chunk
// table, K14a inflates them (omr_inflate.hip) and K13b places them (omr_tiffread.hip).  Blosc chunks
// (K15, omr_zarr_image_open_ex) take the same staging: their container is read by omr_blosc.cpp, on
// the device route into K15a's stream table, and K15b places them (omr_blosc.hip).  Zstandard (K16)
// comes in both ways: as the inner codec of Blosc chunks, whose streams then go to K16a
// (omr_zstd.hip) in a launch of their own, and as the bare zstd codec, which takes the zlib path
// with K16a in place of K14a.
#include "omr_internal.h"

#include <dirent.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <cerrno>
#include <memory>
#include <thread>
#include <unordered_map>

// The stand-alone host checks link this file without the kernels: the Blosc launches may be absent.
namespace omr {
omr_status launch_lz4_decode(Ctx* ctx, const uint8_t* d_src, const uint64_t* d_offsets, const uint32_t* d_lengths,
                             const uint32_t* d_expected, const uint8_t* d_raw, int32_t n, uint8_t* d_dst,
                             const uint64_t* d_dst_offsets, int32_t* d_status) __attribute__((weak));
omr_status launch_blosc_place(Ctx* ctx, const BloscPlace* d_places, int32_t n, int32_t max_rows, int32_t bps)
    __attribute__((weak));
omr_status launch_zstd_decode(Ctx* ctx, const uint8_t* d_src, const uint64_t* d_offsets, const uint32_t* d_lengths,
                              const uint32_t* d_expected, const uint8_t* d_raw, int32_t n, uint8_t* d_dst,
                              const uint64_t* d_dst_offsets, int32_t* d_status, void** lit, size_t* lit_cap)
    __attribute__((weak));
}  // namespace omr

namespace {

constexpr int kNone = 0, kZlib = 1, kBlosc = 2, kZstd = 3;  // omr_zarr_info.compression
constexpr uint64_t kMaxChunkBytes = (uint64_t)256 << 20;    // decoded size of one chunk
constexpr uint64_t kMaxStreamBytes = ((uint64_t)512 << 20) - 1;
constexpr size_t kMaxJsonBytes = (size_t)1 << 20;
constexpr int kMaxJsonDepth = 64;
constexpr int kMaxLevels = 64;

// ---- JSON ---------------------------------------------------------------------------------------

struct Json {
    enum Type { Null, Bool, Number, String, Array, Object } type = Null;
    bool b = false;
    bool is_int = false;          // Number: written without fraction or exponent and inside int64
    int64_t i = 0;
    double d = 0;
    std::string s;
    std::vector<Json> arr;
    std::vector<std::pair<std::string, Json>> obj;
    const Json* get(const char* key) const {
        if (type != Object) return nullptr;
        for (const auto& kv : obj)
            if (kv.first == key) return &kv.second;
        return nullptr;
    }
};

// RFC 8259, recursive descent over [p, end): every read is behind a p < end check.
struct JsonParser {
    const char* p;
    const char* end;
    void ws() {
        while (p < end && (*p == ' ' || *p == '\t' || *p == '\n' || *p == '\r')) ++p;
    }
    bool lit(const char* word) {
        const size_t n = std::strlen(word);
        if ((size_t)(end - p) < n || std::memcmp(p, word, n) != 0) return false;
        p += n;
        return true;
    }
    bool string(std::string& out) {
        if (p >= end || *p != '"') return false;
        ++p;
        while (p < end && *p != '"') {
            unsigned char c = (unsigned char)*p++;
            if (c < 0x20) return false;
            if (c != '\\') {
                out.push_back((char)c);
                continue;
            }
            if (p >= end) return false;
            c = (unsigned char)*p++;
            switch (c) {
            case '"': case '\\': case '/': out.push_back((char)c); break;
            case 'b': out.push_back('\b'); break;
            case 'f': out.push_back('\f'); break;
            case 'n': out.push_back('\n'); break;
            case 'r': out.push_back('\r'); break;
            case 't': out.push_back('\t'); break;
            case 'u': {
                if (end - p < 4) return false;
                uint32_t v = 0;
                for (int k = 0; k < 4; ++k) {
                    const char h = *p++;
                    v <<= 4;
                    if (h >= '0' && h <= '9') v |= (uint32_t)(h - '0');
                    else if (h >= 'a' && h <= 'f') v |= (uint32_t)(h - 'a' + 10);
                    else if (h >= 'A' && h <= 'F') v |= (uint32_t)(h - 'A' + 10);
                    else return false;
                }
                // names and paths here are ASCII; anything else is kept as UTF-8 of the code unit
                if (v < 0x80) out.push_back((char)v);
                else if (v < 0x800) { out.push_back((char)(0xC0 | v >> 6)); out.push_back((char)(0x80 | (v & 0x3F))); }
                else { out.push_back((char)(0xE0 | v >> 12)); out.push_back((char)(0x80 | ((v >> 6) & 0x3F))); out.push_back((char)(0x80 | (v & 0x3F))); }
                break;
            }
            default: return false;
            }
        }
        if (p >= end) return false;
        ++p;                                   // the closing quote
        return true;
    }
    bool number(Json& v) {
        const char* s = p;
        bool integral = true;
        if (p < end && *p == '-') ++p;
        if (p >= end || *p < '0' || *p > '9') return false;
        if (*p == '0') ++p;
        else while (p < end && *p >= '0' && *p <= '9') ++p;
        if (p < end && *p == '.') {
            integral = false;
            ++p;
            if (p >= end || *p < '0' || *p > '9') return false;
            while (p < end && *p >= '0' && *p <= '9') ++p;
        }
        if (p < end && (*p == 'e' || *p == 'E')) {
            integral = false;
            ++p;
            if (p < end && (*p == '+' || *p == '-')) ++p;
            if (p >= end || *p < '0' || *p > '9') return false;
            while (p < end && *p >= '0' && *p <= '9') ++p;
        }
        const std::string text(s, p);          // a copy: strtod needs a terminator
        if (text.size() > 400) return false;
        v.type = Json::Number;
        v.d = std::strtod(text.c_str(), nullptr);
        if (integral) {
            errno = 0;
            const long long ll = std::strtoll(text.c_str(), nullptr, 10);
            v.is_int = errno == 0;
            v.i = ll;
        }
        return true;
    }
    bool value(Json& v, int depth) {
        if (depth > kMaxJsonDepth) return false;
        ws();
        if (p >= end) return false;
        switch (*p) {
        case 'n': v.type = Json::Null; return lit("null");
        case 't': v.type = Json::Bool; v.b = true; return lit("true");
        case 'f': v.type = Json::Bool; v.b = false; return lit("false");
        case '"': v.type = Json::String; return string(v.s);
        case '[':
            v.type = Json::Array;
            ++p;
            ws();
            if (p < end && *p == ']') { ++p; return true; }
            for (;;) {
                v.arr.emplace_back();
                if (!value(v.arr.back(), depth + 1)) return false;
                ws();
                if (p >= end) return false;
                if (*p == ',') { ++p; continue; }
                if (*p == ']') { ++p; return true; }
                return false;
            }
        case '{':
            v.type = Json::Object;
            ++p;
            ws();
            if (p < end && *p == '}') { ++p; return true; }
            for (;;) {
                ws();
                std::string key;
                if (!string(key)) return false;
                ws();
                if (p >= end || *p != ':') return false;
                ++p;
                v.obj.emplace_back(std::move(key), Json());
                if (!value(v.obj.back().second, depth + 1)) return false;
                ws();
                if (p >= end) return false;
                if (*p == ',') { ++p; continue; }
                if (*p == '}') { ++p; return true; }
                return false;
            }
        default: return number(v);
        }
    }
};

bool json_parse(const char* text, size_t n, Json& out) {
    if (n > kMaxJsonBytes) return false;
    JsonParser P{text, text + n};
    if (!P.value(out, 0)) return false;
    P.ws();
    return P.p == P.end;
}

// ---- files --------------------------------------------------------------------------------------

enum class Slurp { Ok, Missing, Error };

// A whole file of at most `limit` bytes.
Slurp read_file(const std::string& path, uint64_t limit, std::vector<uint8_t>& out) {
    const int fd = ::open(path.c_str(), O_RDONLY | O_CLOEXEC);
    if (fd < 0) return errno == ENOENT || errno == ENOTDIR ? Slurp::Missing : Slurp::Error;
    struct stat sb;
    if (::fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode) || (uint64_t)sb.st_size > limit) {
        ::close(fd);
        return Slurp::Error;
    }
    out.resize((size_t)sb.st_size);
    size_t got = 0;
    while (got < out.size()) {
        const ssize_t r = ::read(fd, out.data() + got, out.size() - got);
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) break;
        got += (size_t)r;
    }
    ::close(fd);
    return got == out.size() ? Slurp::Ok : Slurp::Error;
}

struct Level {
    std::string dir;              // group_path/<dataset path>
    int32_t w = 0, h = 0;         // image size at this level
    int32_t cw = 0, ch = 0;       // chunk size
    int32_t across = 0, down = 0;
    char sep = '.';
};

}  // namespace

struct omr_zarr_image {
    int32_t sz = 0, sc = 0, st = 0;
    int32_t pt = 0, bpp = 0;
    bool big = false;
    int comp = kNone;
    uint32_t inner = 0;           // kBlosc: the OMR_BLOSC_INNER_* formats the open allowed
    std::vector<Level> levels;
};

namespace {

std::string chunk_path(const Level& L, int32_t t, int32_t c, int32_t z, int32_t cy, int32_t cx) {
    const int32_t idx[5] = {t, c, z, cy, cx};
    std::string p = L.dir;
    for (int k = 0; k < 5; ++k) {
        p.push_back(k ? L.sep : '/');
        p += std::to_string(idx[k]);
    }
    return p;
}

// ---- inflate (RFC 1950 / 1951), serial ------------------------------------------------------------

struct Bits {
    const uint8_t* s;
    size_t len, pos = 0;          // next byte
    uint64_t buf = 0;
    int cnt = 0;
    bool over = false;            // bits were asked for behind the end of the stream
    // n <= 32 bits, LSB first
    uint32_t take(int n) {
        while (cnt < n) {
            if (pos < len) buf |= (uint64_t)s[pos++] << cnt;
            else over = true;
            cnt += 8;
        }
        const uint32_t v = (uint32_t)(buf & ((1ull << n) - 1));
        buf >>= n;
        cnt -= n;
        return v;
    }
    void align() {
        buf >>= cnt & 7;
        cnt &= ~7;
    }
};

// A canonical Huffman code in the form of Mark Adler's puff: symbols sorted by (length, value) and
// the number of codes per length.
struct Huff {
    uint16_t count[16];
    uint16_t symbol[288];
};

// false: over-subscribed, or incomplete with anything but codes of one bit (zlib's rule: one
// single code of length 1, or no code at all, may stay incomplete).
bool huff_build(Huff& h, const uint8_t* lens, int n) {
    for (int l = 0; l < 16; ++l) h.count[l] = 0;
    for (int k = 0; k < n; ++k) ++h.count[lens[k] & 15];
    int left = 1;
    for (int l = 1; l < 16; ++l) {
        left <<= 1;
        left -= h.count[l];
        if (left < 0) return false;
    }
    if (left > 0 && n - h.count[0] != h.count[1]) return false;
    uint16_t offs[16];
    offs[1] = 0;
    for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + h.count[l]);
    for (int k = 0; k < n; ++k)
        if (lens[k] & 15) h.symbol[offs[lens[k] & 15]++] = (uint16_t)k;
    return true;
}

// -1: no such code (an incomplete set), or the stream ended.
int huff_decode(Bits& b, const Huff& h) {
    int code = 0, first = 0, index = 0;
    for (int l = 1; l < 16; ++l) {
        code |= (int)b.take(1);
        if (b.over) return -1;
        const int count = h.count[l];
        if (code - count < first) return h.symbol[index + (code - first)];
        index += count;
        first += count;
        first <<= 1;
        code <<= 1;
    }
    return -1;
}

inline void length_of(int sym, int& base, int& extra) {     // sym 257 .. 285
    const int i = sym - 257;
    if (i < 8) { base = 3 + i; extra = 0; }
    else if (i == 28) { base = 258; extra = 0; }
    else { extra = (i - 4) >> 2; base = 3 + ((4 + (i & 3)) << extra); }
}
inline void distance_of(int sym, int& base, int& extra) {   // sym 0 .. 29
    if (sym < 4) { base = 1 + sym; extra = 0; }
    else { extra = (sym - 2) >> 1; base = 1 + ((2 + (sym & 1)) << extra); }
}

bool inflate(const uint8_t* s, size_t len, uint8_t* d, size_t expected) {
    if (len < 2) return false;
    if ((s[0] & 15) != 8 || (s[0] >> 4) > 7 || (((uint32_t)s[0] << 8) | s[1]) % 31 != 0 || (s[1] & 0x20)) return false;
    Bits b{s + 2, len - 2};
    size_t out = 0;
    Huff lit, dist;
    uint8_t lens[320];
    static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    for (;;) {
        const uint32_t last = b.take(1), type = b.take(2);
        if (b.over) return false;
        if (type == 3) return false;
        if (type == 0) {
            b.align();
            const uint32_t n = b.take(16), nn = b.take(16);
            if (b.over || (n ^ 0xFFFFu) != nn) return false;
            // the bit buffer holds whole bytes now: hand them back and copy
            b.pos -= (size_t)(b.cnt >> 3);
            b.buf = 0;
            b.cnt = 0;
            if (n > b.len - b.pos || n > expected - out) return false;
            if (n) std::memcpy(d + out, b.s + b.pos, n);
            b.pos += n;
            out += n;
        } else {
            if (type == 1) {
                int k = 0;
                for (; k < 144; ++k) lens[k] = 8;
                for (; k < 256; ++k) lens[k] = 9;
                for (; k < 280; ++k) lens[k] = 7;
                for (; k < 288; ++k) lens[k] = 8;
                huff_build(lit, lens, 288);
                for (k = 0; k < 32; ++k) lens[k] = 5;
                huff_build(dist, lens, 32);
            } else {
                const int hlit = (int)b.take(5) + 257, hdist = (int)b.take(5) + 1, hclen = (int)b.take(4) + 4;
                if (b.over || hlit > 286 || hdist > 30) return false;
                uint8_t cl[19] = {0};
                for (int k = 0; k < hclen; ++k) cl[order[k]] = (uint8_t)b.take(3);
                if (b.over) return false;
                Huff clh;
                if (!huff_build(clh, cl, 19)) return false;
                int k = 0;
                while (k < hlit + hdist) {
                    const int sym = huff_decode(b, clh);
                    if (sym < 0) return false;
                    if (sym < 16) {
                        lens[k++] = (uint8_t)sym;
                        continue;
                    }
                    int v = 0, rep;
                    if (sym == 16) {
                        if (k == 0) return false;         // nothing to repeat
                        v = lens[k - 1];
                        rep = 3 + (int)b.take(2);
                    } else if (sym == 17) {
                        rep = 3 + (int)b.take(3);
                    } else {
                        rep = 11 + (int)b.take(7);
                    }
                    if (b.over || k + rep > hlit + hdist) return false;
                    while (rep--) lens[k++] = (uint8_t)v;
                }
                if (lens[256] == 0) return false;         // no end-of-block code
                if (!huff_build(lit, lens, hlit) || !huff_build(dist, lens + hlit, hdist)) return false;
            }
            for (;;) {
                const int sym = huff_decode(b, lit);
                if (sym < 0) return false;
                if (sym < 256) {
                    if (out >= expected) return false;
                    d[out++] = (uint8_t)sym;
                    continue;
                }
                if (sym == 256) break;
                if (sym > 285) return false;
                int base, extra;
                length_of(sym, base, extra);
                const size_t n = (size_t)base + b.take(extra);
                const int ds = huff_decode(b, dist);
                if (ds < 0 || ds > 29) return false;
                distance_of(ds, base, extra);
                const size_t dd = (size_t)base + b.take(extra);
                if (b.over || dd > out || n > expected - out) return false;
                for (size_t k = 0; k < n; ++k, ++out) d[out] = d[out - dd];
            }
        }
        if (last) break;
    }
    if (out != expected) return false;
    b.align();
    uint32_t want = 0;
    for (int k = 0; k < 4; ++k) want = want << 8 | b.take(8);
    if (b.over) return false;
    uint32_t a1 = 1, a2 = 0;
    for (size_t k = 0; k < out;) {
        const size_t stop = std::min(out, k + 5552);      // the sums stay below 2^32 for 5552 bytes
        for (; k < stop; ++k) {
            a1 += d[k];
            a2 += a1;
        }
        a1 %= 65521u;
        a2 %= 65521u;
    }
    return want == (a2 << 16 | a1);
}

// ---- the image model ------------------------------------------------------------------------------

struct ArrayMeta {
    int64_t shape[5], chunks[5];
    int32_t pt = 0;
    bool big = false;
    int comp = kNone;
    char sep = '.';
};

// A list of five positive integers.  OMR_INVALID_ARGUMENT: not five; OMR_INTERNAL: not positive integers.
omr_status five(const Json* v, int64_t* out) {
    if (!v || v->type != Json::Array) return OMR_INTERNAL;
    for (const Json& e : v->arr)
        if (e.type != Json::Number || !e.is_int || e.i <= 0) return OMR_INTERNAL;
    if (v->arr.size() != 5) return OMR_INVALID_ARGUMENT;
    for (int k = 0; k < 5; ++k) out[k] = v->arr[(size_t)k].i;
    return OMR_OK;
}

omr_status parse_zarray(const std::vector<uint8_t>& text, uint32_t codecs, ArrayMeta& m) {
    Json j;
    if (!json_parse(reinterpret_cast<const char*>(text.data()), text.size(), j) || j.type != Json::Object) return OMR_INTERNAL;
    const Json* v = j.get("zarr_format");
    if (!v || v->type != Json::Number || v->d != 2) return OMR_INVALID_ARGUMENT;
    omr_status st = five(j.get("shape"), m.shape);
    if (st) return st;
    st = five(j.get("chunks"), m.chunks);
    if (st) return st;
    v = j.get("order");
    if (!v || v->type != Json::String || v->s != "C") return OMR_INVALID_ARGUMENT;
    v = j.get("dtype");
    if (!v || v->type != Json::String || v->s.size() != 3) return OMR_INVALID_ARGUMENT;
    static const struct { const char* name; int pt; } kTypes[] = {
        {"u1", OMR_PIXELS_UINT8}, {"i1", OMR_PIXELS_INT8}, {"u2", OMR_PIXELS_UINT16}, {"i2", OMR_PIXELS_INT16},
        {"u4", OMR_PIXELS_UINT32}, {"i4", OMR_PIXELS_INT32}, {"f4", OMR_PIXELS_FLOAT}, {"f8", OMR_PIXELS_DOUBLE}};
    m.pt = -1;
    for (const auto& t : kTypes)
        if (v->s.compare(1, 2, t.name) == 0) m.pt = t.pt;
    if (m.pt < 0) return OMR_INVALID_ARGUMENT;
    const bool one_byte = v->s[2] == '1';
    if (one_byte ? v->s[0] != '|' : (v->s[0] != '<' && v->s[0] != '>')) return OMR_INVALID_ARGUMENT;
    m.big = v->s[0] == '>';
    v = j.get("filters");
    if (v && v->type != Json::Null && !(v->type == Json::Array && v->arr.empty())) return OMR_INVALID_ARGUMENT;
    v = j.get("compressor");
    m.comp = kNone;
    if (v && v->type != Json::Null) {
        const Json* id = v->get("id");
        if (!id || id->type != Json::String) return OMR_INVALID_ARGUMENT;
        if (id->s == "zlib" && (codecs & OMR_ZARR_CODEC_ZLIB)) {
            m.comp = kZlib;
        } else if (id->s == "zstd" && (codecs & OMR_ZARR_CODEC_ZSTD)) {
            m.comp = kZstd;                                // level and checksum: the frames say it themselves
        } else if (id->s == "blosc" && (codecs & (OMR_ZARR_CODEC_BLOSC | OMR_ZARR_CODEC_BLOSC_ZSTD))) {
            // LZ4 inside (lz4hc writes the same block format) or Zstd, each under its own bit; byte
            // shuffle or none.  -1 is numcodecs' automatic choice: byte shuffle for types wider than a
            // byte, bit shuffle for the others.
            const Json* cname = v->get("cname");
            if (!cname || cname->type != Json::String) return OMR_INVALID_ARGUMENT;
            const bool lz4 = (cname->s == "lz4" || cname->s == "lz4hc") && (codecs & OMR_ZARR_CODEC_BLOSC);
            if (!lz4 && !(cname->s == "zstd" && (codecs & OMR_ZARR_CODEC_BLOSC_ZSTD))) return OMR_INVALID_ARGUMENT;
            if (const Json* sh = v->get("shuffle")) {
                if (sh->type != Json::Number || !sh->is_int) return OMR_INVALID_ARGUMENT;
                if (sh->i != 0 && sh->i != 1 && !(sh->i == -1 && !one_byte)) return OMR_INVALID_ARGUMENT;
            }
            m.comp = kBlosc;
        } else {
            return OMR_INVALID_ARGUMENT;
        }
    }
    v = j.get("fill_value");
    if (v && v->type != Json::Null && !(v->type == Json::Number && v->d == 0)) return OMR_INVALID_ARGUMENT;
    v = j.get("dimension_separator");
    m.sep = '.';
    if (v && v->type != Json::Null) {
        if (v->type != Json::String || (v->s != "." && v->s != "/")) return OMR_INVALID_ARGUMENT;
        m.sep = v->s[0];
    }
    uint64_t bytes;
    if (__builtin_mul_overflow((uint64_t)m.chunks[3], (uint64_t)m.chunks[4], &bytes) ||
        __builtin_mul_overflow(bytes, (uint64_t)omr::bytes_per_pixel(m.pt), &bytes) ||
        __builtin_mul_overflow(bytes, (uint64_t)m.chunks[0], &bytes) ||
        __builtin_mul_overflow(bytes, (uint64_t)m.chunks[1], &bytes) ||
        __builtin_mul_overflow(bytes, (uint64_t)m.chunks[2], &bytes))
        return OMR_INTERNAL;
    uint64_t elems = 1;
    for (int k = 0; k < 5; ++k)
        if (__builtin_mul_overflow(elems, (uint64_t)m.shape[k], &elems)) return OMR_INTERNAL;
    if (m.chunks[0] != 1 || m.chunks[1] != 1 || m.chunks[2] != 1) return OMR_INVALID_ARGUMENT;
    if (bytes > kMaxChunkBytes) return OMR_INVALID_ARGUMENT;
    for (int k = 0; k < 5; ++k)
        if (m.shape[k] > 0x7FFFFFFFll) return OMR_INVALID_ARGUMENT;
    return OMR_OK;
}

// A dataset path stays inside the group: relative, no empty, "." or ".." component.
bool safe_relative(const std::string& p) {
    if (p.empty() || p.size() > 1024 || p[0] == '/') return false;
    size_t a = 0;
    while (a <= p.size()) {
        const size_t b = std::min(p.find('/', a), p.size());
        const std::string part = p.substr(a, b - a);
        if (part.empty() || part == "." || part == ".." || part.find('\0') != std::string::npos) return false;
        a = b + 1;
    }
    return true;
}

// The level paths of .zattrs; `have` = false when there is no multiscales entry.
omr_status multiscale_paths(const std::vector<uint8_t>& text, std::vector<std::string>& paths, bool& have) {
    have = false;
    Json j;
    if (!json_parse(reinterpret_cast<const char*>(text.data()), text.size(), j)) return OMR_INTERNAL;
    const Json* ms = j.get("multiscales");
    if (!ms) return OMR_OK;
    if (ms->type != Json::Array || ms->arr.empty() || ms->arr[0].type != Json::Object) return OMR_INVALID_ARGUMENT;
    const Json& m0 = ms->arr[0];
    if (const Json* axes = m0.get("axes")) {
        static const char* kNames[5] = {"t", "c", "z", "y", "x"};
        if (axes->type != Json::Array || axes->arr.size() != 5) return OMR_INVALID_ARGUMENT;
        for (int k = 0; k < 5; ++k) {
            const Json& a = axes->arr[(size_t)k];                 // NGFF 0.4: {"name": "t", ...}; 0.3: "t"
            const Json* name = a.type == Json::Object ? a.get("name") : &a;
            if (!name || name->type != Json::String || name->s != kNames[k]) return OMR_INVALID_ARGUMENT;
        }
    }
    const Json* ds = m0.get("datasets");
    if (!ds || ds->type != Json::Array || ds->arr.empty() || ds->arr.size() > (size_t)kMaxLevels) return OMR_INVALID_ARGUMENT;
    for (const Json& e : ds->arr) {
        const Json* p = e.get("path");
        if (!p || p->type != Json::String || !safe_relative(p->s)) return OMR_INVALID_ARGUMENT;
        paths.push_back(p->s);
    }
    have = true;
    return OMR_OK;
}

bool region_in_bounds(const omr_zarr_image* im, const Level& L, int32_t z, int32_t c, int32_t t, int32_t x, int32_t y,
                      int32_t w, int32_t h) {
    return z >= 0 && z < im->sz && c >= 0 && c < im->sc && t >= 0 && t < im->st && x >= 0 && y >= 0 && w >= 0 &&
           h >= 0 && (int64_t)x + w <= L.w && (int64_t)y + h <= L.h;
}

// Chunk (cx, cy) of a plane, decoded: ch * cw samples.
omr_status load_chunk(const omr_zarr_image* im, const Level& L, int32_t t, int32_t c, int32_t z, int32_t cy, int32_t cx,
                      std::vector<uint8_t>& comp, std::vector<uint8_t>& out) {
    const size_t expected = (size_t)L.ch * L.cw * im->bpp;
    const std::string path = chunk_path(L, t, c, z, cy, cx);
    if (im->comp == kNone) {
        const Slurp r = read_file(path, expected, out);
        if (r == Slurp::Missing) {
            out.assign(expected, 0);
            return OMR_OK;
        }
        return r == Slurp::Ok && out.size() == expected ? OMR_OK : OMR_INTERNAL;
    }
    const Slurp r = read_file(path, kMaxStreamBytes, comp);
    out.assign(expected, 0);
    if (r == Slurp::Missing) return OMR_OK;
    if (r != Slurp::Ok) return OMR_INTERNAL;
    if (im->comp == kBlosc) return omr_blosc_decode_host_ex(comp.data(), comp.size(), out.data(), expected, im->inner);
    if (im->comp == kZstd) return omr::zstd_decode(comp.data(), comp.size(), out.data(), expected) ? OMR_OK : OMR_INTERNAL;
    return inflate(comp.data(), comp.size(), out.data(), expected) ? OMR_OK : OMR_INTERNAL;
}

// ---- device route: staging of one context -------------------------------------------------------

struct ZarrPipe {
    void* pin = nullptr;      // chunk files + tables (+ the statuses coming back)
    void* d_in = nullptr;
    size_t in_cap = 0;
    void* d_scratch = nullptr;   // inflated chunks
    size_t scratch_cap = 0;
    void* d_regions = nullptr;   // omr_render_zarr_tiles: [tile][channel][h][w]
    size_t regions_cap = 0;
    void* d_out = nullptr;       // and its ARGB when the caller's output is host memory
    size_t out_cap = 0;
    void* pin_tab = nullptr;     // Blosc: the stream table and the placements, sized after the files are read
    void* d_tab = nullptr;
    size_t tab_cap = 0;
    void* d_lit = nullptr;       // K16a: one literal buffer per workgroup of its grid
    size_t lit_cap = 0;
    ~ZarrPipe() {
        if (pin) (void)hipHostFree(pin);
        if (pin_tab) (void)hipHostFree(pin_tab);
        for (void* p : {d_in, d_scratch, d_regions, d_out, d_tab, d_lit})
            if (p) (void)hipFree(p);
    }
};

void free_zarr_pipe(void* p) { delete static_cast<ZarrPipe*>(p); }

ZarrPipe* get_zarr_pipe(omr::Ctx* c) {
    if (!c->zarr_state) {
        c->zarr_state = new ZarrPipe;
        c->zarr_state_free = free_zarr_pipe;
    }
    return static_cast<ZarrPipe*>(c->zarr_state);
}

omr_status grow_device(omr::Ctx* c, void*& p, size_t& cap, size_t bytes) {
    if (bytes <= cap) return OMR_OK;
    if (p) OMR_HIP(c, hipFree(p));
    p = nullptr;
    cap = 0;
    OMR_HIP(c, hipMalloc(&p, bytes));
    cap = bytes;
    return OMR_OK;
}

// job(i) for i in [0, n) on up to 16 threads (the calling one included).
template <typename F>
void parallel_for(int n, bool threaded, const F& job) {
    const unsigned hw = std::thread::hardware_concurrency();
    const int extra = threaded ? std::min<int>(n, (int)std::min(hw ? hw : 4u, 16u)) - 1 : 0;
    std::atomic<int> next{0};
    auto work = [&] {
        for (int i; (i = next.fetch_add(1)) < n;) job(i);
    };
    std::vector<std::thread> th;
    for (int k = 0; k < extra; ++k) th.emplace_back(work);
    work();
    for (auto& t : th) t.join();
}

struct UniqueChunk {
    std::string path;
    uint64_t cnt = 0;            // file size; 0: the chunk is missing
    uint64_t in_off = 0, scratch_off = 0;
};

constexpr size_t kGroupInBytes = (size_t)128 << 20;        // chunk file bytes per group (as K13)
constexpr size_t kGroupScratchBytes = (size_t)512 << 20;   // decoded bytes per group
constexpr size_t kRenderGroupBytes = (size_t)256 << 20;    // region bytes per render group

// The Blosc half of read_group, from the chunk files in pinned memory on: the host checks every
// chunk's container and lists its streams (a bad one ends the call before any launch), the bytes go
// up, the tables behind them in a copy of their own (their size is known only now), K15a decodes
// the streams into the chunks' scratch and K15b places with the un-shuffle in its loads.
omr_status finish_blosc(omr::Ctx* ctx, ZarrPipe* T, const std::vector<UniqueChunk>& chunks,
                        const std::vector<omr::TiffPlace>& places, const std::vector<int32_t>& place_chunk,
                        uint32_t expected, size_t in_bytes, int32_t max_rows, int32_t bpp, uint32_t inner) {
    using omr::align_up;
    using omr::BloscPlace;
    if (!omr::launch_lz4_decode || !omr::launch_blosc_place || !omr::launch_zstd_decode)
        return omr::fail(ctx, OMR_DEVICE, "zarr: built without the Blosc kernels");
    uint8_t* pin = static_cast<uint8_t*>(T->pin);
    uint8_t* din = static_cast<uint8_t*>(T->d_in);
    uint8_t* dscr = static_cast<uint8_t*>(T->d_scratch);
    std::vector<omr::BloscLayout> layouts(chunks.size());
    size_t m = 0, m_lz4 = 0;                               // streams; those of LZ4 chunks come first in the tables
    for (size_t k = 0; k < chunks.size(); ++k) {
        const UniqueChunk& u = chunks[k];
        if (!u.cnt) continue;
        if (!omr::blosc_parse(pin + u.in_off, (size_t)u.cnt, expected, layouts[k], inner))
            return omr::fail(ctx, OMR_INTERNAL, "zarr: corrupt blosc chunk");
        m += layouts[k].streams.size();
        if (layouts[k].format != 4u) m_lz4 += layouts[k].streams.size();
    }
    // tables: [offsets u64 m][dst offsets u64 m][lengths u32 m][expected u32 m][raw u8 m][places] | [status i32 m]
    const size_t o_dst = 8 * m, o_len = o_dst + 8 * m, o_exp = o_len + 4 * m, o_raw = o_exp + 4 * m;
    const size_t o_place = align_up(o_raw + m, 16), up_bytes = o_place + places.size() * sizeof(BloscPlace);
    const size_t o_status = align_up(up_bytes, 256), total = o_status + 4 * m;
    if (total > T->tab_cap) {
        if (T->pin_tab) OMR_HIP(ctx, hipHostFree(T->pin_tab));
        T->pin_tab = nullptr;
        const size_t keep = T->tab_cap;
        T->tab_cap = 0;
        omr_status st = grow_device(ctx, T->d_tab, T->tab_cap, std::max(total, keep + keep / 2));
        if (st) return st;
        const hipError_t e = hipHostMalloc(&T->pin_tab, T->tab_cap, hipHostMallocDefault);
        if (e != hipSuccess) {
            T->tab_cap = 0;                              // both are made again on the next call
            return omr::hip_fail(ctx, e, "hipHostMalloc(zarr tables)");
        }
    }
    uint8_t* tab = static_cast<uint8_t*>(T->pin_tab);
    uint8_t* dtab = static_cast<uint8_t*>(T->d_tab);
    uint64_t* h_off = reinterpret_cast<uint64_t*>(tab);
    uint64_t* h_dst = reinterpret_cast<uint64_t*>(tab + o_dst);
    uint32_t* h_len = reinterpret_cast<uint32_t*>(tab + o_len);
    uint32_t* h_exp = reinterpret_cast<uint32_t*>(tab + o_exp);
    uint8_t* h_raw = tab + o_raw;
    size_t j_lz4 = 0, j_zstd = m_lz4;                      // a stored split goes with its chunk's launch
    for (size_t k = 0; k < chunks.size(); ++k)
        for (const omr::BloscStream& s : layouts[k].streams) {
            const size_t j = layouts[k].format != 4u ? j_lz4++ : j_zstd++;
            h_off[j] = chunks[k].in_off + s.src_off;
            h_dst[j] = chunks[k].scratch_off + s.dst_off;
            h_len[j] = s.csize;
            h_exp[j] = s.neblock;
            h_raw[j] = s.raw;
        }
    BloscPlace* h_place = reinterpret_cast<BloscPlace*>(tab + o_place);
    for (size_t k = 0; k < places.size(); ++k) {
        const size_t ck = (size_t)place_chunk[k];
        const UniqueChunk& u = chunks[ck];
        const omr::BloscLayout& L = layouts[ck];
        const omr::TiffPlace& p = places[k];
        BloscPlace b;
        b.src = !u.cnt ? nullptr : L.memcpyed ? din + u.in_off + 16 : dscr + u.scratch_off;
        b.dst = p.dst;
        b.seg_w = p.seg_w; b.dst_pitch = p.dst_pitch;
        b.x0 = p.x0; b.x1 = p.x1; b.y0 = p.y0; b.y1 = p.y1;
        b.blocksize = L.blocksize; b.nbytes = L.nbytes; b.typesize = L.typesize;
        b.shuffled = u.cnt && L.shuffled && !L.memcpyed;
        h_place[k] = b;
    }
    if (in_bytes) OMR_HIP(ctx, hipMemcpyAsync(din, pin, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    OMR_HIP(ctx, hipMemcpyAsync(dtab, tab, up_bytes, hipMemcpyHostToDevice, ctx->stream));
    omr_status st = omr::launch_lz4_decode(ctx, din, reinterpret_cast<const uint64_t*>(dtab),
                                           reinterpret_cast<const uint32_t*>(dtab + o_len),
                                           reinterpret_cast<const uint32_t*>(dtab + o_exp), dtab + o_raw, (int32_t)m_lz4, dscr,
                                           reinterpret_cast<const uint64_t*>(dtab + o_dst),
                                           reinterpret_cast<int32_t*>(dtab + o_status));
    if (st) return st;
    st = omr::launch_zstd_decode(ctx, din, reinterpret_cast<const uint64_t*>(dtab) + m_lz4,
                                 reinterpret_cast<const uint32_t*>(dtab + o_len) + m_lz4,
                                 reinterpret_cast<const uint32_t*>(dtab + o_exp) + m_lz4, dtab + o_raw + m_lz4,
                                 (int32_t)(m - m_lz4), dscr, reinterpret_cast<const uint64_t*>(dtab + o_dst) + m_lz4,
                                 reinterpret_cast<int32_t*>(dtab + o_status) + m_lz4, &T->d_lit, &T->lit_cap);
    if (st) return st;
    st = omr::launch_blosc_place(ctx, reinterpret_cast<const BloscPlace*>(dtab + o_place), (int32_t)places.size(), max_rows, bpp);
    if (st) return st;
    if (m) OMR_HIP(ctx, hipMemcpyAsync(tab + o_status, dtab + o_status, 4 * m, hipMemcpyDeviceToHost, ctx->stream));
    OMR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int32_t* h_status = reinterpret_cast<const int32_t*>(tab + o_status);
    for (size_t i = 0; i < m; ++i)
        if (h_status[i] != OMR_OK) return omr::fail(ctx, OMR_INTERNAL, "zarr: corrupt blosc chunk");
    return OMR_OK;
}

// One group of regions: reqs[r0, r1).
omr_status read_group(omr::Ctx* ctx, const omr_zarr_image* im, int32_t level, const omr_raw_tile_request* reqs, int32_t r0,
                      int32_t r1, int32_t width, int32_t height, uint8_t* d_dst, int64_t stride) {
    using omr::align_up;
    using omr::TiffPlace;
    const Level& L = im->levels[(size_t)level];
    const uint32_t expected = (uint32_t)((size_t)L.ch * L.cw * im->bpp);
    std::unordered_map<uint64_t, int32_t> index;      // plane * chunks + k -> unique chunk
    std::vector<UniqueChunk> chunks;
    std::vector<TiffPlace> places;
    std::vector<int32_t> place_chunk;
    const uint64_t per_plane = (uint64_t)L.across * L.down;
    int32_t max_rows = 0;
    for (int32_t i = r0; i < r1; ++i) {
        const omr_raw_tile_request& r = reqs[i];
        const uint64_t plane = ((uint64_t)r.t * im->sc + r.c) * im->sz + r.z;
        for (int32_t cy = r.y / L.ch; cy <= (r.y + height - 1) / L.ch; ++cy)
            for (int32_t cx = r.x / L.cw; cx <= (r.x + width - 1) / L.cw; ++cx) {
                const uint64_t key = plane * per_plane + (uint64_t)cy * L.across + cx;
                auto it = index.find(key);
                if (it == index.end()) {
                    UniqueChunk u;
                    u.path = chunk_path(L, r.t, r.c, r.z, cy, cx);
                    it = index.emplace(key, (int32_t)chunks.size()).first;
                    chunks.push_back(std::move(u));
                }
                const int32_t ox = cx * L.cw, oy = cy * L.ch;
                const int32_t X0 = std::max(r.x, ox), X1 = std::min(r.x + width, ox + L.cw);
                const int32_t Y0 = std::max(r.y, oy), Y1 = std::min(r.y + height, oy + L.ch);
                TiffPlace p;
                p.src = nullptr;
                p.dst = d_dst + (int64_t)i * stride + ((int64_t)(Y0 - r.y) * width + (X0 - r.x)) * im->bpp;
                p.seg_w = L.cw;
                p.dst_pitch = width;
                p.x0 = X0 - ox; p.x1 = X1 - ox; p.y0 = Y0 - oy; p.y1 = Y1 - oy;
                max_rows = std::max(max_rows, Y1 - Y0);
                places.push_back(p);
                place_chunk.push_back(it->second);
            }
    }
    if (places.empty()) return OMR_OK;
    // the sizes of the chunk files (a file per chunk: nothing but the file system knows them)
    const bool threaded = chunks.size() >= 32;
    std::atomic<int> bad{0};                               // 1: I/O error, 2: a file of the wrong size
    parallel_for((int)chunks.size(), threaded, [&](int k) {
        UniqueChunk& u = chunks[(size_t)k];
        struct stat sb;
        if (::stat(u.path.c_str(), &sb) != 0) {
            if (errno != ENOENT && errno != ENOTDIR) bad = 1;
            return;
        }
        if (!S_ISREG(sb.st_mode)) bad = 1;
        else if (im->comp != kNone ? (uint64_t)sb.st_size > kMaxStreamBytes || sb.st_size == 0 : (uint64_t)sb.st_size != expected) bad = 2;
        else u.cnt = (uint64_t)sb.st_size;
    });
    if (bad == 1) return omr::fail(ctx, OMR_INTERNAL, "zarr: chunk file cannot be read");
    if (bad == 2) return omr::fail(ctx, OMR_INTERNAL, "zarr: chunk file of the wrong size");
    size_t in_bytes = 0, scratch_bytes = 0;
    std::vector<int32_t> coded;                        // the chunks K14a inflates, or K16a decodes
    for (size_t k = 0; k < chunks.size(); ++k) {
        UniqueChunk& u = chunks[k];
        if (!u.cnt) continue;
        u.in_off = in_bytes;
        in_bytes += align_up((size_t)u.cnt, 16);
        if (im->comp != kNone) {
            u.scratch_off = scratch_bytes;
            scratch_bytes += align_up((size_t)expected, 16);
            if (im->comp == kZlib || im->comp == kZstd) coded.push_back((int32_t)k);
        }
    }
    const bool blosc = im->comp == kBlosc;                 // its tables go up behind the bytes, from T->pin_tab
    const size_t m = coded.size();
    // staging: [bytes][offsets u64 m][dst offsets u64 m][lengths u32 m][expected u32 m][places] | [status i32 m]
    const size_t o_off = align_up(in_bytes, 256), o_dst = o_off + 8 * m, o_len = o_dst + 8 * m, o_exp = o_len + 4 * m;
    const size_t o_place = align_up(o_exp + 4 * m, 16), up_bytes = o_place + (blosc ? 0 : places.size() * sizeof(TiffPlace));
    const size_t o_status = align_up(up_bytes, 256), total = o_status + 4 * m;
    ZarrPipe* T = get_zarr_pipe(ctx);
    if (total > T->in_cap) {
        if (T->pin) OMR_HIP(ctx, hipHostFree(T->pin));
        T->pin = nullptr;
        const size_t keep = T->in_cap;
        T->in_cap = 0;
        omr_status st = grow_device(ctx, T->d_in, T->in_cap, std::max(total, keep + keep / 2));
        if (st) return st;
        const hipError_t e = hipHostMalloc(&T->pin, T->in_cap, hipHostMallocDefault);
        if (e != hipSuccess) {
            T->in_cap = 0;                               // both are made again on the next call
            return omr::hip_fail(ctx, e, "hipHostMalloc(zarr staging)");
        }
    }
    omr_status st = grow_device(ctx, T->d_scratch, T->scratch_cap, scratch_bytes);
    if (st) return st;
    uint8_t* pin = static_cast<uint8_t*>(T->pin);
    uint8_t* din = static_cast<uint8_t*>(T->d_in);
    uint8_t* dscr = static_cast<uint8_t*>(T->d_scratch);
    std::atomic<bool> io_error{false};
    parallel_for((int)chunks.size(), threaded, [&](int k) {
        const UniqueChunk& u = chunks[(size_t)k];
        if (!u.cnt) return;
        const int fd = ::open(u.path.c_str(), O_RDONLY | O_CLOEXEC);
        if (fd < 0) {
            io_error = true;
            return;
        }
        size_t got = 0;
        while (got < u.cnt) {                              // a file that shrank since the stat is an error
            const ssize_t r = ::pread(fd, pin + u.in_off + got, (size_t)u.cnt - got, (off_t)got);
            if (r < 0 && errno == EINTR) continue;
            if (r <= 0) break;
            got += (size_t)r;
        }
        ::close(fd);
        if (got != u.cnt) io_error = true;
    });
    if (io_error) return omr::fail(ctx, OMR_INTERNAL, "zarr: chunk read failed");
    if (blosc) return finish_blosc(ctx, T, chunks, places, place_chunk, expected, in_bytes, max_rows, im->bpp, im->inner);
    uint64_t* h_off = reinterpret_cast<uint64_t*>(pin + o_off);
    uint64_t* h_dst = reinterpret_cast<uint64_t*>(pin + o_dst);
    uint32_t* h_len = reinterpret_cast<uint32_t*>(pin + o_len);
    uint32_t* h_exp = reinterpret_cast<uint32_t*>(pin + o_exp);
    for (size_t j = 0; j < m; ++j) {
        const UniqueChunk& u = chunks[(size_t)coded[j]];
        h_off[j] = u.in_off;
        h_dst[j] = u.scratch_off;
        h_len[j] = (uint32_t)u.cnt;
        h_exp[j] = expected;
    }
    TiffPlace* h_place = reinterpret_cast<TiffPlace*>(pin + o_place);
    for (size_t k = 0; k < places.size(); ++k) {
        const UniqueChunk& u = chunks[(size_t)place_chunk[k]];
        places[k].src = !u.cnt ? nullptr : im->comp != kNone ? dscr + u.scratch_off : din + u.in_off;
        h_place[k] = places[k];
    }
    OMR_HIP(ctx, hipMemcpyAsync(din, pin, up_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (im->comp == kZstd) {
        if (!omr::launch_zstd_decode) return omr::fail(ctx, OMR_DEVICE, "zarr: built without the Zstandard kernel");
        st = omr::launch_zstd_decode(ctx, din, reinterpret_cast<const uint64_t*>(din + o_off),
                                     reinterpret_cast<const uint32_t*>(din + o_len), reinterpret_cast<const uint32_t*>(din + o_exp),
                                     nullptr, (int32_t)m, dscr, reinterpret_cast<const uint64_t*>(din + o_dst),
                                     reinterpret_cast<int32_t*>(din + o_status), &T->d_lit, &T->lit_cap);
    } else {
        st = omr::launch_inflate(ctx, din, reinterpret_cast<const uint64_t*>(din + o_off),
                                 reinterpret_cast<const uint32_t*>(din + o_len), reinterpret_cast<const uint32_t*>(din + o_exp),
                                 (int32_t)m, dscr, reinterpret_cast<const uint64_t*>(din + o_dst),
                                 reinterpret_cast<int32_t*>(din + o_status));
    }
    if (st) return st;
    st = omr::launch_tiff_place(ctx, reinterpret_cast<const TiffPlace*>(din + o_place), (int32_t)places.size(), max_rows,
                                im->bpp, 1, false);
    if (st) return st;
    if (m) OMR_HIP(ctx, hipMemcpyAsync(pin + o_status, din + o_status, 4 * m, hipMemcpyDeviceToHost, ctx->stream));
    OMR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int32_t* h_status = reinterpret_cast<const int32_t*>(pin + o_status);
    for (size_t j = 0; j < m; ++j)
        if (h_status[j] != OMR_OK)
            return omr::fail(ctx, OMR_INTERNAL, im->comp == kZstd ? "zarr: corrupt zstd chunk" : "zarr: corrupt zlib chunk");
    return OMR_OK;
}

}  // namespace

namespace omr {
omr_status zarr_zstd_literals(Ctx* ctx, void*** lit, size_t** lit_cap) {
    ZarrPipe* T = get_zarr_pipe(ctx);
    *lit = &T->d_lit;
    *lit_cap = &T->lit_cap;
    return OMR_OK;
}
}  // namespace omr

using namespace omr;

extern "C" {

omr_status omr_zarr_image_open(const char* group_path, omr_zarr_image** out) {
    return omr_zarr_image_open_ex(group_path, nullptr, out);
}

omr_status omr_zarr_image_open_ex(const char* group_path, const omr_zarr_open_options* opt, omr_zarr_image** out) {
    if (!out) return OMR_INVALID_ARGUMENT;
    *out = nullptr;
    if (!group_path || !*group_path) return OMR_INVALID_ARGUMENT;
    uint32_t codecs = OMR_ZARR_CODEC_ZLIB;
    if (opt) {
        if (opt->struct_size < sizeof(omr_zarr_open_options)) return OMR_INVALID_ARGUMENT;
        if (opt->codecs & ~(OMR_ZARR_CODEC_ZLIB | OMR_ZARR_CODEC_BLOSC | OMR_ZARR_CODEC_BLOSC_ZSTD | OMR_ZARR_CODEC_ZSTD))
            return OMR_INVALID_ARGUMENT;
        codecs = opt->codecs;
    }
    std::string root(group_path);
    while (root.size() > 1 && root.back() == '/') root.pop_back();
    struct stat sb;
    if (::stat(root.c_str(), &sb) != 0) return errno == ENOENT || errno == ENOTDIR ? OMR_NOT_FOUND : OMR_INVALID_ARGUMENT;
    if (!S_ISDIR(sb.st_mode)) return OMR_INVALID_ARGUMENT;
    std::vector<uint8_t> text;
    std::vector<std::string> paths;
    bool listed = false;
    const Slurp za = read_file(root + "/.zattrs", kMaxJsonBytes, text);
    if (za == Slurp::Error) return OMR_INTERNAL;
    if (za == Slurp::Ok) {
        const omr_status st = multiscale_paths(text, paths, listed);
        if (st) return st;
    }
    std::unique_ptr<omr_zarr_image> im(new omr_zarr_image);
    im->inner = (codecs & OMR_ZARR_CODEC_BLOSC ? OMR_BLOSC_INNER_LZ4 : 0u) | (codecs & OMR_ZARR_CODEC_BLOSC_ZSTD ? OMR_BLOSC_INNER_ZSTD : 0u);
    char sep0 = '.';
    for (int k = 0; listed ? k < (int)paths.size() : k < kMaxLevels; ++k) {
        Level L;
        L.dir = root + "/" + (listed ? paths[(size_t)k] : std::to_string(k));
        const Slurp r = read_file(L.dir + "/.zarray", kMaxJsonBytes, text);
        if (r == Slurp::Missing) {
            if (k == 0) return OMR_NOT_FOUND;
            if (!listed) break;                          // the bare route ends at the first gap
            return OMR_INTERNAL;                         // a level the metadata names is not there
        }
        if (r != Slurp::Ok) return OMR_INTERNAL;
        ArrayMeta m;
        const omr_status st = parse_zarray(text, codecs, m);
        if (st) return st;
        if (k == 0) {
            im->st = (int32_t)m.shape[0]; im->sc = (int32_t)m.shape[1]; im->sz = (int32_t)m.shape[2];
            im->pt = m.pt;
            im->bpp = bytes_per_pixel(m.pt);
            im->big = m.big;
            im->comp = m.comp;
            sep0 = m.sep;
        } else if (m.pt != im->pt || m.big != im->big || m.comp != im->comp || m.sep != sep0 || m.shape[0] != im->st ||
                   m.shape[1] != im->sc || m.shape[2] != im->sz) {
            return OMR_INVALID_ARGUMENT;                 // levels that disagree
        }
        L.h = (int32_t)m.shape[3]; L.w = (int32_t)m.shape[4];
        L.ch = (int32_t)m.chunks[3]; L.cw = (int32_t)m.chunks[4];
        L.across = (int32_t)(((int64_t)L.w + L.cw - 1) / L.cw);
        L.down = (int32_t)(((int64_t)L.h + L.ch - 1) / L.ch);
        L.sep = m.sep;
        im->levels.push_back(std::move(L));
    }
    *out = im.release();
    return OMR_OK;
}

void omr_zarr_image_close(omr_zarr_image* img) { delete img; }

omr_status omr_zarr_image_info(const omr_zarr_image* img, omr_zarr_info* info) {
    if (!img || !info) return OMR_INVALID_ARGUMENT;
    const Level& L = img->levels[0];
    info->size_x = L.w; info->size_y = L.h;
    info->size_z = img->sz; info->size_c = img->sc; info->size_t_ = img->st;
    info->pixel_type = img->pt;
    info->big_endian = img->big;
    info->n_levels = (int32_t)img->levels.size();
    info->compression = img->comp;
    info->chunk_width = L.cw;
    info->chunk_height = L.ch;
    info->dimension_separator = L.sep;
    return OMR_OK;
}

int32_t omr_zarr_image_level_sizes(const omr_zarr_image* img, int32_t* sizes_out, int32_t cap_pairs) {
    if (!img || (!sizes_out && cap_pairs > 0)) return -(int32_t)OMR_INVALID_ARGUMENT;
    const int32_t n = (int32_t)img->levels.size();
    for (int32_t k = 0; k < n && k < cap_pairs; ++k) {
        sizes_out[2 * k] = img->levels[(size_t)k].w;
        sizes_out[2 * k + 1] = img->levels[(size_t)k].h;
    }
    return n;
}

omr_status omr_inflate_host(const uint8_t* src, size_t length, uint8_t* dst, size_t expected) {
    if ((!src && length) || (!dst && expected)) return OMR_INVALID_ARGUMENT;
    return inflate(src, length, dst, expected) ? OMR_OK : OMR_INTERNAL;
}

omr_status omr_zarr_image_get_tile(const omr_zarr_image* img, int32_t level, int32_t z, int32_t c, int32_t t,
                                   int32_t x, int32_t y, int32_t w, int32_t h, void* dst, size_t cap) {
    if (!img || !dst || level < 0 || level >= (int32_t)img->levels.size()) return OMR_INVALID_ARGUMENT;
    const Level& L = img->levels[(size_t)level];
    if (!region_in_bounds(img, L, z, c, t, x, y, w, h)) return OMR_INVALID_ARGUMENT;   // DimensionsOutOfBounds
    if (cap < (size_t)w * h * img->bpp) return OMR_BUFFER_TOO_SMALL;
    if (w == 0 || h == 0) return OMR_OK;
    std::vector<uint8_t> comp, chunk;
    uint8_t* out = static_cast<uint8_t*>(dst);
    const size_t bpp = (size_t)img->bpp;
    for (int32_t cy = y / L.ch; cy <= (y + h - 1) / L.ch; ++cy)
        for (int32_t cx = x / L.cw; cx <= (x + w - 1) / L.cw; ++cx) {
            const omr_status st = load_chunk(img, L, t, c, z, cy, cx, comp, chunk);
            if (st) return st;
            const int32_t ox = cx * L.cw, oy = cy * L.ch;
            const int32_t X0 = std::max(x, ox), X1 = std::min(x + w, ox + L.cw);
            const int32_t Y0 = std::max(y, oy), Y1 = std::min(y + h, oy + L.ch);
            for (int32_t yy = Y0; yy < Y1; ++yy)
                std::memcpy(out + ((size_t)(yy - y) * w + (X0 - x)) * bpp,
                            chunk.data() + ((size_t)(yy - oy) * L.cw + (X0 - ox)) * bpp, (size_t)(X1 - X0) * bpp);
        }
    return OMR_OK;
}

omr_status omr_zarr_image_read_regions_device(omr_ctx* ctx, const omr_zarr_image* img, int32_t level,
                                              const omr_raw_tile_request* reqs, int32_t n, int32_t width,
                                              int32_t height, void* d_dst, int64_t region_stride_bytes) {
    if (!ctx) return OMR_INVALID_ARGUMENT;
    if (!img || n < 0 || (n && (!reqs || !d_dst))) return fail(ctx, OMR_INVALID_ARGUMENT, "zarr: null argument");
    if (level < 0 || level >= (int32_t)img->levels.size()) return fail(ctx, OMR_INVALID_ARGUMENT, "zarr: no such level");
    if (width < 0 || height < 0) return fail(ctx, OMR_INVALID_ARGUMENT, "zarr: bad region size");
    const Level& L = img->levels[(size_t)level];
    const int64_t region_bytes = (int64_t)width * height * img->bpp;
    if (region_stride_bytes < region_bytes || region_stride_bytes % img->bpp ||
        reinterpret_cast<uintptr_t>(d_dst) % (uintptr_t)img->bpp)
        return fail(ctx, OMR_INVALID_ARGUMENT, "zarr: region stride or destination not a multiple of the sample size");
    for (int32_t i = 0; i < n; ++i)
        if (!region_in_bounds(img, L, reqs[i].z, reqs[i].c, reqs[i].t, reqs[i].x, reqs[i].y, width, height))
            return fail(ctx, OMR_INVALID_ARGUMENT, "zarr: region " + std::to_string(i) + " outside the image");
    if (n == 0 || width == 0 || height == 0) return OMR_OK;
    OMR_HIP(ctx, hipSetDevice(ctx->device));
    // groups of requests within the staging budgets (a request's chunks counted without sharing)
    const size_t chunk_dec = align_up((size_t)L.cw * L.ch * img->bpp, 16);
    const size_t per_req = (size_t)((width - 1) / L.cw + 2) * (size_t)((height - 1) / L.ch + 2) * chunk_dec;
    const int32_t G = (int32_t)std::max<size_t>(1, std::min<size_t>((size_t)n, std::min(kGroupInBytes, kGroupScratchBytes) / per_req));
    for (int32_t r0 = 0; r0 < n; r0 += G) {
        const omr_status st = read_group(ctx, img, level, reqs, r0, std::min(n, r0 + G), width, height,
                                         static_cast<uint8_t*>(d_dst), region_stride_bytes);
        if (st) return st;
    }
    return OMR_OK;
}

omr_status omr_render_zarr_tiles(omr_ctx* ctx, const omr_zarr_image* img, int32_t level, const omr_quantum_def* qdef,
                                 const omr_channel_binding* channels, int32_t size_c, const omr_tile_request* reqs,
                                 int32_t n, int32_t width, int32_t height, int32_t flip_h, int32_t flip_v,
                                 uint32_t* argb_out, int32_t out_on_device) {
    if (!ctx) return OMR_INVALID_ARGUMENT;
    if (!img || !qdef || !channels || !reqs || !argb_out || n < 0) return fail(ctx, OMR_INVALID_ARGUMENT, "null argument");
    if (size_c != img->sc) return fail(ctx, OMR_INVALID_ARGUMENT, "channel bindings do not match the image's sizeC");
    if (width <= 0 || height <= 0) return fail(ctx, OMR_INVALID_ARGUMENT, "bad tile size");
    if (level < 0 || level >= (int32_t)img->levels.size()) return fail(ctx, OMR_INVALID_ARGUMENT, "zarr: no such level");
    if (n == 0) return OMR_OK;
    // the rendered channels, compacted: [tile][active channel][h][w] with their bindings in order
    std::vector<int32_t> act;
    std::vector<omr_channel_binding> bind;
    for (int c = 0; c < size_c; ++c)
        if (channels[c].active) {
            if (qdef->model == OMR_MODEL_GREYSCALE && !act.empty()) break;   // first active only
            act.push_back(c);
            bind.push_back(channels[c]);
        }
    const int na = (int)act.size();
    if (act.empty()) bind.assign(channels, channels + size_c);   // nothing to read: the render's own answer
    OMR_HIP(ctx, hipSetDevice(ctx->device));
    ZarrPipe* T = get_zarr_pipe(ctx);
    const size_t plane_al = align_up((size_t)width * height * img->bpp, 16);   // K2's vector path: 16-byte strides
    const size_t tile_out = (size_t)width * height * 4;
    const int32_t G = (int32_t)std::max<size_t>(1, std::min<size_t>((size_t)n, kRenderGroupBytes / (plane_al * std::max(na, 1))));
    omr_status st = grow_device(ctx, T->d_regions, T->regions_cap, std::max<size_t>(16, plane_al * na * (size_t)G));
    if (st) return st;
    if (!out_on_device) {
        st = grow_device(ctx, T->d_out, T->out_cap, tile_out * (size_t)G);
        if (st) return st;
    }
    std::vector<omr_raw_tile_request> rr;
    for (int32_t t0 = 0; t0 < n; t0 += G) {
        const int32_t cnt = std::min(G, n - t0);
        rr.clear();
        for (int32_t i = 0; i < cnt; ++i)
            for (int a = 0; a < na; ++a) rr.push_back({reqs[t0 + i].z, act[(size_t)a], reqs[t0 + i].t, reqs[t0 + i].x, reqs[t0 + i].y});
        st = omr_zarr_image_read_regions_device(ctx, img, level, rr.data(), cnt * na, width, height, T->d_regions,
                                                (int64_t)plane_al);
        if (st) return st;
        uint32_t* dout = out_on_device ? argb_out + (size_t)t0 * width * height : static_cast<uint32_t*>(T->d_out);
        st = omr_render_batch_strided_device(ctx, qdef, bind.data(), (int32_t)bind.size(), T->d_regions, (int64_t)(plane_al * na),
                                             (int64_t)plane_al, cnt, 0, img->pt, img->big, width, height, flip_h, flip_v,
                                             dout, nullptr);
        if (st) return st;
        if (!out_on_device) {
            st = omr_ctx_synchronize(ctx);
            if (st) return st;
            OMR_HIP(ctx, hipMemcpy(reinterpret_cast<uint8_t*>(argb_out) + (size_t)t0 * tile_out, dout,
                                   tile_out * (size_t)cnt, hipMemcpyDeviceToHost));
        }
    }
    return out_on_device ? omr_ctx_synchronize(ctx) : OMR_OK;
}

}  // extern "C"
