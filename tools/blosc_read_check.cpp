// blosc_read_check.cpp — the Blosc container parser, the host LZ4 and Blosc decoders
// (omr_blosc.cpp) and omr_zarr_image_open_ex / omr_zarr_image_get_tile on a Blosc group
// (omr_zarr.cpp, K15) under AddressSanitizer and UBSan, as a stand-alone CPU program: chunks are
// built here (a small greedy LZ4 encoder and the container writer below), read back, then damaged
// in the ways user-uploaded data can be -- the corrupt chunks and malformed streams of
// tests/test_blosc_read_host.py -- and after that byte by byte at random, from a fixed seed; every
// damaged input must be answered with OMR_OK or OMR_INTERNAL, never with a read or write out of
// bounds.  The decoders' buffers are exactly as large as their data, so a byte touched past one is
// caught.
// Built and run by `make -C omero-ms-image-region_amd blosc-read-check`.
#include <sys/stat.h>
#include <unistd.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "read_check_stubs.h"

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

typedef std::vector<uint8_t> Bytes;

static void put_len(Bytes& out, size_t v) {            // the extension of a length whose nibble is 15
    v -= 15;
    for (; v >= 255; v -= 255) out.push_back(255);
    out.push_back((uint8_t)v);
}

// One sequence: literals, then (mlen >= 4) a match; mlen 0: the literals alone.
static void put_seq(Bytes& out, const uint8_t* lits, size_t nlit, size_t offset, size_t mlen) {
    const size_t ml = mlen ? mlen - 4 : 0;
    out.push_back((uint8_t)((nlit < 15 ? nlit : 15) << 4 | (ml < 15 ? ml : 15)));
    if (nlit >= 15) put_len(out, nlit);
    out.insert(out.end(), lits, lits + nlit);
    if (mlen) {
        out.push_back((uint8_t)offset);
        out.push_back((uint8_t)(offset >> 8));
        if (ml >= 15) put_len(out, ml);
    }
}

// A greedy encoder: the last position of every four bytes, by a small hash table.
static Bytes lz4_encode(const Bytes& d) {
    Bytes out;
    const size_t n = d.size();
    std::vector<int64_t> table(1 << 12, -1);
    size_t anchor = 0, i = 0;
    while (i + 12 <= n) {
        uint32_t v;
        std::memcpy(&v, d.data() + i, 4);
        const uint32_t h = (v * 2654435761u) >> 20;
        const int64_t cand = table[h];
        table[h] = (int64_t)i;
        if (cand < 0 || i - (size_t)cand > 65535 || std::memcmp(d.data() + cand, d.data() + i, 4) != 0) {
            ++i;
            continue;
        }
        size_t m = 4;
        while (i + m < n - 5 && d[(size_t)cand + m] == d[i + m]) ++m;
        put_seq(out, d.data() + anchor, i - anchor, i - (size_t)cand, m);
        i += m;
        anchor = i;
    }
    put_seq(out, d.data() + anchor, n - anchor, 0, 0);
    return out;
}

static void put32(Bytes& b, size_t at, int64_t v) {
    for (int k = 0; k < 4; ++k) b[at + (size_t)k] = (uint8_t)((uint32_t)v >> (8 * k));
}
static void add32(Bytes& b, int64_t v) {
    b.resize(b.size() + 4);
    put32(b, b.size() - 4, v);
}
static int64_t get32(const Bytes& b, size_t at) {
    return (int32_t)((uint32_t)b[at] | (uint32_t)b[at + 1] << 8 | (uint32_t)b[at + 2] << 16 | (uint32_t)b[at + 3] << 24);
}

// A Blosc 1 chunk of d: the container of include/omr/omr.h.
static Bytes blosc_encode(const Bytes& d, size_t ts, bool shuffle, size_t blocksize, bool nosplit, bool memcpyed) {
    const size_t n = d.size();
    Bytes c{2, 1, (uint8_t)(1u << 5 | (shuffle ? 1u : 0u) | (nosplit ? 0x10u : 0u) | (memcpyed ? 2u : 0u)), (uint8_t)ts};
    add32(c, (int64_t)n);
    add32(c, (int64_t)blocksize);
    add32(c, 0);
    if (memcpyed) {
        c.insert(c.end(), d.begin(), d.end());
        put32(c, 12, (int64_t)c.size());
        return c;
    }
    const size_t nblocks = (n + blocksize - 1) / blocksize;
    c.resize(16 + 4 * nblocks);
    for (size_t b = 0; b < nblocks; ++b) {
        const size_t nb = std::min(blocksize, n - b * blocksize), q = nb / ts;
        Bytes blk(d.begin() + (long)(b * blocksize), d.begin() + (long)(b * blocksize + nb));
        if (shuffle && ts > 1) {
            const Bytes src = blk;
            for (size_t j = 0; j < ts; ++j)
                for (size_t i = 0; i < q; ++i) blk[j * q + i] = src[i * ts + j];
        }
        const bool split = !nosplit && ts <= 16 && blocksize / ts >= 128 && nb == blocksize;
        const size_t nsplits = split ? ts : 1, ne = nb / nsplits;
        put32(c, 16 + 4 * b, (int64_t)c.size());
        for (size_t k = 0; k < nsplits; ++k) {
            const Bytes part(blk.begin() + (long)(k * ne), blk.begin() + (long)((k + 1) * ne));
            Bytes s = lz4_encode(part);
            if (s.size() >= ne) s = part;
            add32(c, (int64_t)s.size());
            c.insert(c.end(), s.begin(), s.end());
        }
    }
    put32(c, 12, (int64_t)c.size());
    return c;
}

static omr_status lz4_exact(const Bytes& s, size_t expected) {
    Bytes out(expected), in(s);               // exactly: ASan guards the rest
    return omr_lz4_decode_host(in.data(), in.size(), out.data(), expected);
}
static omr_status blosc_exact(const Bytes& s, size_t expected, Bytes* got = nullptr) {
    Bytes out(expected), in(s);
    const omr_status st = omr_blosc_decode_host(in.data(), in.size(), out.data(), expected);
    if (got) *got = out;
    return st;
}

// The image: 40 x 50 uint16 in 24 x 32 chunks, two channels; data[i] of a chunk below.
constexpr int CW = 24, CH_ = 32, CHUNK = CW * CH_ * 2, W = 40, H = 50;
static std::string g_dir;

static Bytes chunk_data() {
    Bytes d((size_t)CHUNK);
    uint32_t r = 12345;
    for (int i = 0; i < CHUNK / 2; ++i) {
        r = r * 1664525u + 1013904223u;
        d[2 * (size_t)i] = (uint8_t)(r >> 24);                       // low byte: noise
        d[2 * (size_t)i + 1] = (uint8_t)(i / 100 + (i % 7 == 0));     // high byte: compresses
    }
    return d;
}

static void put_file(const std::string& rel, const void* data, size_t n) {
    const std::string path = g_dir + "/" + rel;
    for (size_t k = g_dir.size() + 1; k < path.size(); ++k)
        if (path[k] == '/') ::mkdir(path.substr(0, k).c_str(), 0700);
    std::FILE* fp = std::fopen(path.c_str(), "wb");
    if (!fp || std::fwrite(data, 1, n, fp) != n) {
        std::printf("cannot write %s\n", path.c_str());
        std::exit(2);
    }
    std::fclose(fp);
}
static void put_text(const std::string& rel, const std::string& s) { put_file(rel, s.data(), s.size()); }
static void put_bytes(const std::string& rel, const Bytes& b) { put_file(rel, b.data(), b.size()); }

static std::string zarray(const std::string& compressor, const std::string& dtype = "<u2") {
    return "{\"zarr_format\": 2, \"shape\": [1, 2, 1, 50, 40], \"chunks\": [1, 1, 1, 32, 24], \"dtype\": \"" + dtype +
           "\", \"compressor\": " + compressor + ", \"fill_value\": 0, \"order\": \"C\", \"filters\": null, "
           "\"dimension_separator\": \".\"}";
}
static const char* kBlosc = "{\"id\": \"blosc\", \"cname\": \"lz4\", \"clevel\": 5, \"shuffle\": 1, \"blocksize\": 0}";

static std::vector<Bytes> g_chunks;       // the good group's eight chunk files, every container variant

static void write_good() {
    put_text("0/.zarray", zarray(kBlosc));
    for (int k = 0; k < 8; ++k) {
        char name[32];
        std::snprintf(name, sizeof name, "0/0.%d.0.%d.%d", k / 4, k / 2 % 2, k % 2);
        put_bytes(name, g_chunks[(size_t)k]);
    }
}

static omr_status open_with(uint32_t codecs, omr_zarr_image** img) {
    omr_zarr_open_options opt = {sizeof(omr_zarr_open_options), codecs};
    return omr_zarr_image_open_ex(g_dir.c_str(), &opt, img);
}

// Open with both codecs and, when that works, read both channels whole and one pixel; the first failing status.
static omr_status run(bool expect_pixels = false) {
    omr_zarr_image* img = nullptr;
    omr_status st = open_with(OMR_ZARR_CODEC_ZLIB | OMR_ZARR_CODEC_BLOSC, &img);
    if (st) {
        CHECK(img == nullptr);
        return st;
    }
    omr_zarr_info info;
    CHECK(omr_zarr_image_info(img, &info) == OMR_OK && info.compression == 2);
    omr_status first = OMR_OK;
    const Bytes d = chunk_data();
    for (int c = 0; c < 2; ++c) {
        Bytes out((size_t)W * H * 2);                              // exactly: ASan guards the rest
        st = omr_zarr_image_get_tile(img, 0, 0, c, 0, 0, 0, W, H, out.data(), out.size());
        if (st && !first) first = st;
        if (!st && expect_pixels)
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < 2 * W; ++x) CHECK(out[(size_t)y * 2 * W + x] == d[(size_t)(y % CH_) * 2 * CW + x % (2 * CW)]);
        Bytes one(2);
        st = omr_zarr_image_get_tile(img, 0, 0, c, 0, W - 1, H - 1, 1, 1, one.data(), one.size());
        if (st && !first) first = st;
    }
    omr_zarr_image_close(img);
    return first;
}

// `chunk` as the one chunk of a 1 x e array of bytes (a chunk of any size; the decoder follows the
// header's typesize), read whole through open_ex and get_tile.  The good group is written again after.
static omr_status run_one_chunk(const Bytes& chunk, size_t e) {
    const std::string n = std::to_string(e);
    put_text("0/.zarray", "{\"zarr_format\": 2, \"shape\": [1, 1, 1, 1, " + n + "], \"chunks\": [1, 1, 1, 1, " + n +
                              "], \"dtype\": \"|u1\", \"compressor\": " + kBlosc + ", \"fill_value\": 0, \"order\": \"C\", "
                              "\"filters\": null, \"dimension_separator\": \".\"}");
    put_bytes("0/0.0.0.0.0", chunk);
    omr_zarr_image* img = nullptr;
    omr_status st = open_with(OMR_ZARR_CODEC_BLOSC, &img);
    CHECK(st == OMR_OK && img);
    if (st) return st;
    Bytes out(e);                                                  // exactly: ASan guards the rest
    st = omr_zarr_image_get_tile(img, 0, 0, 0, 0, 0, 0, (int32_t)e, 1, out.data(), out.size());
    omr_zarr_image_close(img);
    return st;
}

int main() {
    char tmpl[] = "/tmp/blosc_read_check_XXXXXX";
    if (!mkdtemp(tmpl)) return 2;
    g_dir = tmpl;
    const Bytes d = chunk_data();
    // the variants: split, 0x10 set, unshuffled, three blocks, a leftover block, blocks too small to
    // split, memcpyed, another typesize
    g_chunks = {blosc_encode(d, 2, true, CHUNK, false, false), blosc_encode(d, 2, true, CHUNK, true, false),
                blosc_encode(d, 2, false, CHUNK, false, false), blosc_encode(d, 2, true, 512, false, false),
                blosc_encode(d, 2, true, 1000, false, false), blosc_encode(d, 8, true, 512, false, false),
                blosc_encode(d, 2, true, CHUNK, false, true), blosc_encode(d, 3, true, 500, true, false)};
    for (const Bytes& c : g_chunks) {
        Bytes got;
        CHECK(blosc_exact(c, CHUNK, &got) == OMR_OK && got == d);
        CHECK(blosc_exact(c, CHUNK - 1) == OMR_INTERNAL && blosc_exact(c, CHUNK + 1) == OMR_INTERNAL);
    }
    CHECK(get32(g_chunks[0], 20) == CHUNK / 2);                    // the low-byte split is stored raw
    put_text(".zattrs", "{\"multiscales\": [{\"version\": \"0.4\", \"datasets\": [{\"path\": \"0\"}]}]}");
    write_good();
    CHECK(run(true) == OMR_OK);
    ::unlink((g_dir + "/0/0.1.0.1.1").c_str());
    CHECK(run() == OMR_OK);                                        // a missing chunk reads as zeros
    write_good();

    // the open rules
    {
        omr_zarr_image* img = nullptr;
        CHECK(omr_zarr_image_open(g_dir.c_str(), &img) == OMR_INVALID_ARGUMENT && !img);
        CHECK(omr_zarr_image_open_ex(g_dir.c_str(), nullptr, &img) == OMR_INVALID_ARGUMENT && !img);
        CHECK(open_with(OMR_ZARR_CODEC_ZLIB, &img) == OMR_INVALID_ARGUMENT && !img);
        CHECK(open_with(7u, &img) == OMR_INVALID_ARGUMENT && !img);
        omr_zarr_open_options small = {4, 3};
        CHECK(omr_zarr_image_open_ex(g_dir.c_str(), &small, &img) == OMR_INVALID_ARGUMENT && !img);
        CHECK(open_with(OMR_ZARR_CODEC_BLOSC, &img) == OMR_OK && img);
        omr_zarr_image_close(img);
    }
    for (const char* comp : {"{\"id\": \"blosc\", \"cname\": \"zstd\", \"shuffle\": 1}", "{\"id\": \"blosc\", \"cname\": \"blosclz\"}",
                             "{\"id\": \"blosc\", \"cname\": \"lz4\", \"shuffle\": 2}", "{\"id\": \"blosc\"}",
                             "{\"id\": \"blosc\", \"cname\": 4}", "{\"id\": \"lz4\"}"}) {
        put_text("0/.zarray", zarray(comp));
        CHECK(run() == OMR_INVALID_ARGUMENT);
    }
    put_text("0/.zarray", zarray("{\"id\": \"blosc\", \"cname\": \"lz4\", \"shuffle\": -1}", "|u1"));
    CHECK(run() == OMR_INVALID_ARGUMENT);                          // bit shuffle by numcodecs' rule
    put_text("0/.zarray", zarray("{\"id\": \"blosc\", \"cname\": \"lz4hc\", \"shuffle\": -1}"));
    CHECK(run(true) == OMR_OK);
    write_good();

    // malformed LZ4 streams, alone
    const uint8_t* L = d.data();
    std::vector<std::pair<Bytes, size_t>> bad;
    bad.push_back({Bytes(), 10});                                                       // empty
    { Bytes s; put_seq(s, L, 4, 0, 8); put_seq(s, L, 1, 0, 0); bad.push_back({s, 13}); }      // offset 0
    { Bytes s; put_seq(s, L, 4, 5, 8); put_seq(s, L, 1, 0, 0); bad.push_back({s, 13}); }      // one beyond the bytes produced
    bad.push_back({Bytes{0x50, 'a', 'b', 'c'}, 5});                                     // literals past the input
    { Bytes s; put_seq(s, L, 10, 0, 0); bad.push_back({s, 5}); }                              // literals past expected
    { Bytes s; put_seq(s, L, 4, 4, 20); put_seq(s, L, 0, 0, 0); bad.push_back({s, 10}); }     // match past expected
    { Bytes s; put_seq(s, L, 4, 4, 19); s.pop_back(); bad.push_back({s, 23}); }               // cut after the offset
    bad.push_back({Bytes{0xF0, 0xFF}, 600});                                            // cut inside a length extension
    { Bytes s; put_seq(s, L, 4, 4, 300); s.pop_back(); bad.push_back({s, 304}); }
    { Bytes s; put_seq(s, L, 4, 4, 8); bad.push_back({s, 12}); }                              // ends after a match
    Bytes plane((size_t)CHUNK / 2);
    for (size_t i = 0; i < plane.size(); ++i) plane[i] = d[2 * i + 1];
    const Bytes good = lz4_encode(plane);
    CHECK(good.size() < plane.size() && lz4_exact(good, plane.size()) == OMR_OK);
    bad.push_back({good, plane.size() + 1});                                            // one byte short of expected
    bad.push_back({good, plane.size() - 1});                                            // one byte over
    bad.push_back({Bytes(good.begin(), good.begin() + (long)good.size() / 2), plane.size()});   // cut in half
    for (size_t k = 0; k < bad.size(); ++k)
        if (lz4_exact(bad[k].first, bad[k].second) != OMR_INTERNAL) {
            std::printf("FAILED: malformed stream %zu is not OMR_INTERNAL\n", k);
            ++g_fail;
        }

    // corrupt containers, alone and as a chunk of the group
    const Bytes& g3 = g_chunks[3];                                 // three blocks of two splits
    const size_t table_end = 16 + 4 * 3;
    CHECK((size_t)get32(g3, 16) == table_end);
    std::vector<Bytes> corrupt;
    auto with32 = [](Bytes b, size_t at, int64_t v) { put32(b, at, v); return b; };
    auto with8 = [](Bytes b, size_t at, uint8_t v) { b[at] = v; return b; };
    corrupt.push_back(Bytes(g3.begin(), g3.begin() + 15));                              // under 16 bytes
    corrupt.push_back(with8(g3, 0, 3));                                                 // version 3
    corrupt.push_back(with32(g3, 4, CHUNK + 1));
    corrupt.push_back(with32(g3, 4, CHUNK - 1));
    corrupt.push_back(with32(g3, 8, 0));
    corrupt.push_back(with32(g3, 8, CHUNK + 1));
    corrupt.push_back(with32(g3, 8, -512));
    corrupt.push_back(with32(g3, 12, (int64_t)g3.size() + 1));                          // cbytes not the file size
    corrupt.push_back(with8(g3, 3, 0));                                                 // typesize 0
    corrupt.push_back(with32(g3, 20, (int64_t)table_end - 4));                          // a bstart inside the table
    corrupt.push_back(with32(g3, 24, (int64_t)g3.size() + 1));                          // and past the file
    corrupt.push_back(with32(g3, 16, -1));
    corrupt.push_back(with32(g3, table_end, 0));                                        // csize 0
    corrupt.push_back(with32(g3, table_end, -5));
    corrupt.push_back(with32(g3, table_end, 257));                                      // neblock + 1
    {
        Bytes b(g3.begin(), g3.end() - 1);                                              // the last stream past the file
        put32(b, 12, (int64_t)b.size());
        corrupt.push_back(b);
        Bytes t(g3.begin(), g3.begin() + 20);                                           // a truncated table
        put32(t, 12, 20);
        corrupt.push_back(t);
    }
    corrupt.push_back(with8(g3, 2, (uint8_t)(g3[2] & 0x1F)));                           // compressor format 0
    corrupt.push_back(with8(g3, 2, (uint8_t)((g3[2] & 0x1F) | 4 << 5)));                // and 4
    corrupt.push_back(with8(g3, 2, (uint8_t)(g3[2] | 4)));                              // bit shuffle
    corrupt.push_back(with8(g3, 2, (uint8_t)(g3[2] | 2)));                              // memcpyed with a wrong cbytes
    for (size_t k = 0; k < bad.size(); ++k) {                                           // each bad stream as the one split of a chunk,
        const Bytes& s = bad[k].first;                                                  // (an empty or over-long one is stopped by the csize rule)
        const size_t e = bad[k].second;
        Bytes c{2, 1, 0x30, 2};
        add32(c, (int64_t)e); add32(c, (int64_t)e); add32(c, (int64_t)(24 + s.size())); add32(c, 20); add32(c, (int64_t)s.size());
        c.insert(c.end(), s.begin(), s.end());
        if (blosc_exact(c, e) != OMR_INTERNAL || run_one_chunk(c, e) != OMR_INTERNAL) {      // alone, and through get_tile
            std::printf("FAILED: malformed stream %zu as a split is not OMR_INTERNAL\n", k);
            ++g_fail;
        }
    }
    {
        // all bstarts of a chunk of one-byte blocks on one stored split: the list may not outgrow the file
        Bytes c{2, 1, 0x30, 2};
        add32(c, CHUNK); add32(c, 1); add32(c, 16 + 4 * CHUNK + 5);
        for (int k = 0; k < CHUNK; ++k) add32(c, 16 + 4 * CHUNK);
        add32(c, 1);
        c.push_back(7);
        omr::BloscLayout lay;
        CHECK(!omr::blosc_parse(c.data(), c.size(), CHUNK, lay) && lay.streams.size() <= 1);
        corrupt.push_back(c);
    }
    write_good();
    {
        // a chunk-sized carrier for a bad stream: the high-byte split of chunk 0 overwritten with 0xFF
        Bytes c = g_chunks[0];
        const size_t at = (size_t)get32(c, 16), low = (size_t)get32(c, at);
        for (size_t k = at + 4 + low + 4; k < c.size(); ++k) c[k] = 0xFF;
        corrupt.push_back(c);
    }
    for (size_t k = 0; k < corrupt.size(); ++k) {
        if (blosc_exact(corrupt[k], CHUNK) != OMR_INTERNAL) {
            std::printf("FAILED: corrupt chunk %zu is not OMR_INTERNAL\n", k);
            ++g_fail;
        }
        put_bytes("0/0.0.0.0.0", corrupt[k]);
        CHECK(run() == OMR_INTERNAL);
    }
    write_good();
    CHECK(run(true) == OMR_OK);

    // random damage: OMR_OK or OMR_INTERNAL, no bad access (the sanitizers are the check)
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto next = [&] {
        rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17;
        return rng;
    };
    auto damage = [&](Bytes f) {
        const int hits = 1 + (int)(next() % 4);
        for (int k = 0; k < hits && !f.empty(); ++k) {
            // the header and the table are hit as often as the streams
            const size_t at = next() % 2 ? next() % std::min<size_t>(f.size(), 48) : next() % f.size();
            f[at] = next() % 3 ? (uint8_t)next() : (uint8_t)(next() % 2 ? 0xFF : 0x00);
        }
        if (next() % 7 == 0 && !f.empty()) f.resize(next() % f.size());
        return f;
    };
    int ok_streams = 0, ok_chunks = 0, opened = 0;
    std::vector<Bytes> seeds = {good};
    for (const auto& b : bad)
        if (!b.first.empty()) seeds.push_back(b.first);
    for (int it = 0; it < 6000; ++it) {
        const omr_status st = lz4_exact(damage(seeds[(size_t)it % seeds.size()]), it % 11 == 0 ? (size_t)(next() % 2000) : plane.size());
        CHECK(st == OMR_OK || st == OMR_INTERNAL);
        ok_streams += st == OMR_OK;
    }
    for (int it = 0; it < 6000; ++it) {
        Bytes c = damage(g_chunks[(size_t)it % g_chunks.size()]);
        if (it % 3 == 0 && c.size() >= 16) put32(c, 12, (int64_t)c.size());             // let a cut file pass the size check
        const omr_status st = blosc_exact(c, it % 13 == 0 ? (size_t)(next() % 4000) : (size_t)CHUNK);
        CHECK(st == OMR_OK || st == OMR_INTERNAL);
        ok_chunks += st == OMR_OK;
        omr::BloscLayout lay;
        if (omr::blosc_parse(c.data(), c.size(), CHUNK, lay))
            for (const omr::BloscStream& s : lay.streams)                               // what the device route would upload
                CHECK((uint64_t)s.src_off + s.csize <= c.size() && (uint64_t)s.dst_off + s.neblock <= (uint64_t)CHUNK &&
                      s.csize > 0 && s.csize <= s.neblock && s.raw == (s.csize == s.neblock));
    }
    for (int it = 0; it < 1500; ++it) {
        const size_t k = (size_t)it % 8;
        char name[32];
        std::snprintf(name, sizeof name, "0/0.%d.0.%d.%d", (int)k / 4, (int)k / 2 % 2, (int)k % 2);
        Bytes c = damage(g_chunks[k]);
        if (it % 2 == 0 && c.size() >= 16) put32(c, 12, (int64_t)c.size());
        put_bytes(name, c);
        const omr_status st = run();
        CHECK(st == OMR_OK || st == OMR_INTERNAL);
        opened += st == OMR_OK;
        put_bytes(name, g_chunks[k]);
    }
    std::printf("blosc_read_check: %d of 6000 damaged streams, %d of 6000 damaged chunks and %d of 1500 damaged groups still read\n",
                ok_streams, ok_chunks, opened);
    const std::string rm = "rm -rf '" + g_dir + "'";
    if (std::system(rm.c_str()) != 0) std::printf("could not remove %s\n", g_dir.c_str());
    std::printf(g_fail ? "blosc_read_check: %d check(s) failed\n" : "blosc_read_check: ok\n", g_fail);
    return g_fail ? 1 : 0;
}
