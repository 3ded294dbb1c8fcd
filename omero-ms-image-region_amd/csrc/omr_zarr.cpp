// omr_zarr.cpp — K14, host half: OME-Zarr pixel data (include/omr/omr.h).
//
// The third backend of pixelsService.getPixelBuffer: a Zarr v2 directory as bioformats2raw writes
// it, one 5-D TCZYX array per resolution and one file per chunk.  This file holds the small JSON
// reader of the metadata (.zattrs, .zarray: user-uploaded data, so it has a depth and a length
// limit and never reads past its buffer), the image model, the plain serial inflate of the host
// route (omr_inflate_host, omr_zarr_image_get_tile: the reference of the tests and the route of
// single reads) and what the device route needs to know of a Zarr group (ZarrSource): a chunk's
// path, the stat pass that sizes the chunk files, and the read of one file per chunk.  The device
// route itself -- staging, planning, the launches of K14a (zlib), K16a (zstd) and, for Blosc chunks
// (K15, omr_zarr_image_open_ex), of K15a, K16a and K15b behind omr_blosc.cpp's container parser,
// the tile renderer -- is omr_segread.cpp, shared with the TIFF reader; this file calls no HIP
// function.
#include "omr_segread.h"

#include <dirent.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cerrno>
#include <memory>

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

// ---- device route: what the shared pipeline (omr_segread.h) asks of a Zarr group ----------------------

struct ZarrSource final : omr::SegSource {
    const omr_zarr_image* im;
    const int32_t level;
    const Level& L;                      // of a level outside the image: the first; the entry points' checks refuse it (dims())
    std::vector<std::string> paths;      // of the group's chunks, from sizes() to read()
    ZarrSource(const omr_zarr_image* img, int32_t lv)
        : im(img), level(lv), L(img->levels[lv >= 0 && (size_t)lv < img->levels.size() ? (size_t)lv : 0]) {
        kind = omr::SegKind::zarr;
        tag = "zarr";
        noun = "chunk";
        geom.seg_w = L.cw; geom.seg_h = L.ch; geom.across = L.across; geom.down = L.down; geom.bpp = im->bpp;
        codec = im->comp == kZlib ? omr::SegCodec::zlib : im->comp == kZstd ? omr::SegCodec::zstd
                : im->comp == kBlosc ? omr::SegCodec::blosc : omr::SegCodec::none;
        blosc_inner = im->inner;
        pt = im->pt; big = im->big;
    }
    omr::SegImageDims dims() const {
        return {level, (int32_t)im->levels.size(), im->bpp, im->sc,
                [this](const omr_raw_tile_request& r, int32_t w, int32_t h) {
                    return region_in_bounds(im, L, r.z, r.c, r.t, r.x, r.y, w, h);
                }};
    }
    bool threaded(size_t chunks) const { return chunks >= 32; }
    int64_t plane_of(const omr_raw_tile_request& r) const override { return ((int64_t)r.t * im->sc + r.c) * im->sz + r.z; }
    // the sizes of the chunk files (a file per chunk: nothing but the file system knows them)
    omr_status sizes(omr::Ctx* ctx, const std::vector<omr::SegKey>& keys, std::vector<omr::SegBytes>& out) override {
        const uint32_t expected = (uint32_t)((size_t)L.ch * L.cw * im->bpp);
        paths.resize(keys.size());
        std::atomic<int> bad{0};                               // 1: I/O error, 2: a file of the wrong size
        omr::parallel_for((int)keys.size(), threaded(keys.size()), [&](int k) {
            const omr::SegKey& key = keys[(size_t)k];
            const int64_t zc = key.plane / im->sz;
            paths[(size_t)k] = chunk_path(L, (int32_t)(zc / im->sc), (int32_t)(zc % im->sc), (int32_t)(key.plane % im->sz), key.sy, key.sx);
            out[(size_t)k].expected = expected;
            struct stat sb;
            if (::stat(paths[(size_t)k].c_str(), &sb) != 0) {
                if (errno != ENOENT && errno != ENOTDIR) bad = 1;
                return;
            }
            if (!S_ISREG(sb.st_mode)) bad = 1;
            else if (im->comp != kNone ? (uint64_t)sb.st_size > kMaxStreamBytes || sb.st_size == 0 : (uint64_t)sb.st_size != expected) bad = 2;
            else out[(size_t)k].cnt = (uint64_t)sb.st_size;
        });
        if (bad == 1) return omr::fail(ctx, OMR_INTERNAL, "zarr: chunk file cannot be read");
        if (bad == 2) return omr::fail(ctx, OMR_INTERNAL, "zarr: chunk file of the wrong size");
        return OMR_OK;
    }
    bool read(const std::vector<omr::SegKey>&, const std::vector<omr::SegBytes>& segs, uint8_t* pin, size_t) override {
        std::atomic<bool> io_error{false};
        omr::parallel_for((int)segs.size(), threaded(segs.size()), [&](int k) {
            const omr::SegBytes& u = segs[(size_t)k];
            if (!u.cnt) return;
            const int fd = ::open(paths[(size_t)k].c_str(), O_RDONLY | O_CLOEXEC);
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
        return !io_error;
    }
};

}  // namespace


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
    if (!img) return fail(ctx, OMR_INVALID_ARGUMENT, "zarr: null argument");
    ZarrSource src(img, level);
    return read_regions_checked(ctx, src, src.dims(), reqs, n, width, height, d_dst, region_stride_bytes);
}

omr_status omr_render_zarr_tiles(omr_ctx* ctx, const omr_zarr_image* img, int32_t level, const omr_quantum_def* qdef,
                                 const omr_channel_binding* channels, int32_t size_c, const omr_tile_request* reqs,
                                 int32_t n, int32_t width, int32_t height, int32_t flip_h, int32_t flip_v,
                                 uint32_t* argb_out, int32_t out_on_device) {
    if (!ctx) return OMR_INVALID_ARGUMENT;
    if (!img) return fail(ctx, OMR_INVALID_ARGUMENT, "null argument");
    ZarrSource src(img, level);
    return render_tiles_checked(ctx, src, src.dims(), qdef, channels, size_c, reqs, n, width, height, flip_h, flip_v, argb_out,
                                out_on_device);
}

}  // extern "C"
