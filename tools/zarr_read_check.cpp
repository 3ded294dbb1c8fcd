// zarr_read_check.cpp — the Zarr reader's JSON reader, image model and host inflate (omr_zarr.cpp,
// K14) under AddressSanitizer and UBSan, as a stand-alone CPU program: a small zlib-compressed
// group is built here (its chunk streams embedded below, made once with Python's zlib, or stored
// blocks written here), read back, then damaged in the ways user-uploaded data can be -- the
// corrupt groups and malformed streams of tests/test_zarr_read_host.py -- and after that byte by
// byte at random; every damaged input must be answered with a status, never with a read or write
// out of bounds.  The decoder's output buffers are exactly as large as the chunk, so a byte written
// past one is caught.
// Built and run by `make -C omero-ms-image-region_amd zarr-read-check`.
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

// One chunk: 24 x 32 uint8, data[i] = i * i % 9 + i / 64 % 3; a dynamic and a fixed block of it
// (zlib.compressobj(9, DEFLATED, 15, 8, Z_DEFAULT_STRATEGY / Z_FIXED)).
constexpr int CW = 24, CH_ = 32, CHUNK = CW * CH_, W = 40, H = 50;
static const uint8_t kDynamic[64] = {
    120, 218, 213, 210, 185, 1, 0, 32, 16, 2, 65, 192, 231, 180, 255, 134, 165, 134, 35, 50, 155, 112, 131, 5,
    39, 170, 48, 137, 30, 180, 120, 14, 151, 216, 196, 214, 189, 218, 67, 163, 137, 40, 222, 136, 226, 141, 40, 222,
    136, 226, 141, 40, 222, 136, 226, 13, 124, 254, 207, 3, 5, 106, 10, 254,
};
static const uint8_t kFixed[73] = {
    120, 1, 99, 96, 100, 97, 96, 103, 103, 96, 97, 100, 32, 143, 193, 196, 202, 200, 193, 193, 200, 202, 196, 72,
    38, 131, 141, 137, 147, 147, 137, 141, 153, 137, 153, 76, 6, 69, 142, 7, 50, 40, 114, 60, 144, 65, 145, 227,
    129, 12, 138, 28, 15, 100, 80, 228, 120, 32, 131, 34, 199, 3, 25, 12, 67, 60, 253, 0, 0, 5, 106, 10,
    254,
};

static Bytes chunk_data() {
    Bytes d(CHUNK);
    for (int i = 0; i < CHUNK; ++i) d[(size_t)i] = (uint8_t)(i * i % 9 + i / 64 % 3);
    return d;
}

static uint32_t adler32(const Bytes& d) {
    uint32_t a = 1, b = 0;
    for (uint8_t v : d) {
        a = (a + v) % 65521u;
        b = (b + a) % 65521u;
    }
    return b << 16 | a;
}

// Deflate's bit order: fields LSB first, Huffman codes MSB first.
struct BitWriter {
    Bytes out{0x78, 0x01};
    uint32_t acc = 0;
    int n = 0;
    BitWriter& put(uint32_t v, int bits) {
        for (int k = 0; k < bits; ++k) {
            acc |= ((v >> k) & 1u) << n;
            if (++n == 8) {
                out.push_back((uint8_t)acc);
                acc = 0;
                n = 0;
            }
        }
        return *this;
    }
    BitWriter& code(uint32_t c, int bits) {
        for (int k = bits - 1; k >= 0; --k) put((c >> k) & 1u, 1);
        return *this;
    }
    BitWriter& align() {
        if (n) put(0, 8 - n);
        return *this;
    }
    BitWriter& raw(const Bytes& d) {
        out.insert(out.end(), d.begin(), d.end());
        return *this;
    }
    BitWriter& be32(uint32_t v) {
        for (int k = 3; k >= 0; --k) out.push_back((uint8_t)(v >> (8 * k)));
        return *this;
    }
    Bytes done(int pad) {
        align();
        out.insert(out.end(), (size_t)pad, 0);
        return out;
    }
};

// Stored blocks of at most `piece` bytes.
static Bytes stored_stream(const Bytes& d, size_t piece) {
    BitWriter w;
    size_t at = 0;
    do {
        const size_t n = std::min(piece, d.size() - at);
        w.put(at + n == d.size(), 1).put(0, 2).align().put((uint32_t)n, 16).put(~(uint32_t)n & 0xFFFFu, 16);
        w.raw(Bytes(d.begin() + (long)at, d.begin() + (long)(at + n)));
        at += n;
    } while (at < d.size());
    return w.be32(adler32(d)).done(0);
}

static std::string g_dir;

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

static const char* kZattrs =
    "{\"multiscales\": [{\"version\": \"0.4\", \"axes\": [{\"name\": \"t\", \"type\": \"time\"}, {\"name\": \"c\"}, "
    "{\"name\": \"z\"}, {\"name\": \"y\"}, {\"name\": \"x\"}], \"datasets\": [{\"path\": \"0\"}]}]}";

static std::string zarray(const std::string& shape = "[1, 2, 1, 50, 40]", const std::string& chunks = "[1, 1, 1, 32, 24]",
                          const std::string& compressor = "{\"id\": \"zlib\", \"level\": 1}",
                          const std::string& extra = "\"fill_value\": 0") {
    return "{\n \"zarr_format\": 2, \"shape\": " + shape + ", \"chunks\": " + chunks + ", \"dtype\": \"|u1\", \"compressor\": " +
           compressor + ", " + extra + ", \"order\": \"C\", \"filters\": null, \"dimension_separator\": \".\"\n}";
}

static std::vector<Bytes> g_streams;      // the good group's eight chunk streams

static void write_good(bool compressed = true) {
    put_text(".zattrs", kZattrs);
    put_text("0/.zarray", compressed ? zarray() : zarray("[1, 2, 1, 50, 40]", "[1, 1, 1, 32, 24]", "null"));
    const Bytes d = chunk_data();
    for (int k = 0; k < 8; ++k) {
        char name[32];
        std::snprintf(name, sizeof name, "0/0.%d.0.%d.%d", k / 4, k / 2 % 2, k % 2);
        put_bytes(name, compressed ? g_streams[(size_t)k] : d);
    }
}

// Open and, when that works, read both channels whole and one pixel; returns the first failing status.
static omr_status run(bool expect_pixels = false) {
    omr_zarr_image* img = nullptr;
    omr_status st = omr_zarr_image_open(g_dir.c_str(), &img);
    if (st) {
        CHECK(img == nullptr);
        return st;
    }
    omr_zarr_info info;
    CHECK(omr_zarr_image_info(img, &info) == OMR_OK);
    int32_t sizes[2] = {0, 0};
    CHECK(omr_zarr_image_level_sizes(img, sizes, 1) >= 1);
    omr_status first = OMR_OK;
    const Bytes d = chunk_data();
    if (sizes[0] <= 4096 && sizes[1] <= 4096 && (int64_t)info.chunk_width * info.chunk_height <= (1 << 24)) {
        for (int c = 0; c < info.size_c && c < 2; ++c) {
            Bytes out((size_t)sizes[0] * sizes[1] * omr::bytes_per_pixel(info.pixel_type));   // exactly: ASan guards the rest
            st = omr_zarr_image_get_tile(img, 0, 0, c, 0, 0, 0, sizes[0], sizes[1], out.data(), out.size());
            if (st && !first) first = st;
            if (!st && expect_pixels)
                for (int y = 0; y < H; ++y)
                    for (int x = 0; x < W; ++x) CHECK(out[(size_t)y * W + x] == d[(size_t)(y % CH_) * CW + x % CW]);
            Bytes one(8);
            st = omr_zarr_image_get_tile(img, 0, 0, c, 0, sizes[0] - 1, sizes[1] - 1, 1, 1, one.data(), one.size());
            if (st && !first) first = st;
        }
    }
    omr_zarr_image_close(img);
    return first;
}

static omr_status inflate_exact(const Bytes& s, size_t expected) {
    Bytes out(expected);                      // exactly: ASan guards the rest
    Bytes in(s);                              // and the end of the stream
    return omr_inflate_host(in.data(), in.size(), out.data(), expected);
}

int main() {
    char tmpl[] = "/tmp/zarr_read_check_XXXXXX";
    if (!mkdtemp(tmpl)) return 2;
    g_dir = tmpl;
    const Bytes d = chunk_data();
    const Bytes dyn(kDynamic, kDynamic + sizeof kDynamic), fix(kFixed, kFixed + sizeof kFixed);
    for (int k = 0; k < 8; ++k)
        g_streams.push_back(k % 4 == 0 ? dyn : k % 4 == 1 ? fix : k % 4 == 2 ? stored_stream(d, 65535) : stored_stream(d, 100));
    for (const Bytes& s : g_streams) {
        Bytes out(CHUNK);
        CHECK(omr_inflate_host(s.data(), s.size(), out.data(), CHUNK) == OMR_OK && out == d);
    }
    write_good();
    CHECK(run(true) == OMR_OK);
    write_good(false);
    CHECK(run(true) == OMR_OK);
    put_bytes("0/0.1.0.1.1", Bytes(d.begin(), d.end() - 1));
    CHECK(run() == OMR_INTERNAL);                          // a wrong-sized raw chunk
    ::unlink((g_dir + "/0/0.1.0.1.1").c_str());
    CHECK(run() == OMR_OK);                                // a missing chunk reads as zeros
    write_good();

    // the corrupt and unsupported groups of tests/test_zarr_read_host.py
    const std::string good = zarray();
    put_text("0/.zarray", good.substr(0, good.size() / 2));
    CHECK(run() == OMR_INTERNAL);                          // truncated JSON
    put_text("0/.zarray", std::string(300, '[') + std::string(300, ']'));
    CHECK(run() == OMR_INTERNAL);                          // 300-deep nesting
    std::string deep;
    for (int k = 0; k < 300; ++k) deep += "{\"a\":";
    put_text("0/.zarray", deep + "1" + std::string(300, '}'));
    CHECK(run() == OMR_INTERNAL);
    put_text("0/.zarray", "{\"a\": \"\\u12");
    CHECK(run() == OMR_INTERNAL);
    put_text("0/.zarray", "");
    CHECK(run() == OMR_INTERNAL);
    put_text("0/.zarray", zarray("[1, 1, 1, -5, 7]"));
    CHECK(run() == OMR_INTERNAL);
    put_text("0/.zarray", zarray("[1, 2, 1, 1.5, 40]"));
    CHECK(run() == OMR_INTERNAL);
    put_text("0/.zarray", zarray("[1, 2, 1, 50, 40]", "[1, 1, 1, 1099511627776, 1099511627776]"));
    CHECK(run() == OMR_INTERNAL);                          // a chunk whose product overflows
    put_text("0/.zarray", zarray("[1, 2, 1, 50, 40]", "[1, 1, 1, 99999999999999999999999999, 24]"));
    CHECK(run() == OMR_INTERNAL);
    put_text("0/.zarray", zarray("[1, 2, 1, 50, 40]", "[1, 1, 1, 16384, 16385]"));
    CHECK(run() == OMR_INVALID_ARGUMENT);                  // a chunk above 256 MiB
    put_text("0/.zarray", zarray("[1, 2, 1, 50, 40]", "[1, 2, 1, 32, 24]"));
    CHECK(run() == OMR_INVALID_ARGUMENT);
    put_text("0/.zarray", zarray("[2, 1, 50, 40]", "[1, 1, 32, 24]"));
    CHECK(run() == OMR_INVALID_ARGUMENT);
    put_text("0/.zarray", zarray("[1, 2, 1, 50, 40]", "[1, 1, 1, 32, 24]", "{\"id\": \"blosc\", \"cname\": \"lz4\"}"));
    CHECK(run() == OMR_INVALID_ARGUMENT);
    put_text("0/.zarray", zarray("[1, 2, 1, 50, 40]", "[1, 1, 1, 32, 24]", "null", "\"fill_value\": 7"));
    CHECK(run() == OMR_INVALID_ARGUMENT);
    put_text("0/.zarray", good);
    put_text(".zattrs", "{\"multiscales\": [{\"datasets\": [{\"path\": \"0\"}]}");
    CHECK(run() == OMR_INTERNAL);
    put_text(".zattrs", "{\"multiscales\": [{\"datasets\": [{\"path\": \"../x\"}]}]}");
    CHECK(run() == OMR_INVALID_ARGUMENT);
    put_text(".zattrs", kZattrs);
    CHECK(run(true) == OMR_OK);
    {
        omr_zarr_image* img = nullptr;
        CHECK(omr_zarr_image_open((g_dir + "/nothing").c_str(), &img) == OMR_NOT_FOUND && !img);
    }

    // the malformed streams of the tests, alone and as a chunk
    std::vector<std::pair<Bytes, size_t>> bad;
    bad.push_back({Bytes(), 10});                                                       // empty
    Bytes s = dyn;
    s[0] = 0x77; s[1] = (uint8_t)((31 - 0x7700 % 31) % 31);
    bad.push_back({s, CHUNK});                                                          // CM != 8
    s = dyn; s[1] ^= 1;
    bad.push_back({s, CHUNK});                                                          // FCHECK
    s = dyn; s[1] = 0x20; s[0] = 0x78;
    s.insert(s.begin() + 2, 4, 0);
    bad.push_back({s, CHUNK});                                                          // FDICT
    bad.push_back({BitWriter().put(1, 1).put(3, 2).done(8), 64});                       // block type 3
    bad.push_back({BitWriter().put(1, 1).put(0, 2).align().put(5, 16).put((~5u & 0xFFFFu) ^ 1u, 16)
                       .raw(Bytes{'h', 'e', 'l', 'l', 'o'}).be32(0x062C0215u).done(0), 5});   // LEN != ~NLEN
    bad.push_back({BitWriter().put(1, 1).put(2, 2).put(30, 5).put(0, 5).put(0, 4).done(64), 64});   // HLIT = 287
    bad.push_back({BitWriter().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(0, 4).put(1, 3).put(1, 3).put(1, 3).put(1, 3)
                       .done(64), 64});                                                 // over-subscribed
    bad.push_back({BitWriter().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(0, 4).put(1, 3).put(0, 3).put(0, 3).put(1, 3)
                       .code(1, 1).put(0, 2).done(64), 64});                            // repeat code 16 first
    {
        BitWriter w;
        w.put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(1, 4).put(0, 3).put(0, 3).put(0, 3).put(1, 3).put(1, 3);
        for (int k = 0; k < 256; ++k) w.code(1, 1);
        w.code(0, 1).code(0, 1);
        for (char c : std::string("hello")) w.code((uint8_t)c, 8);
        bad.push_back({w.done(64), 5});                                                 // no end-of-block code
    }
    bad.push_back({BitWriter().put(1, 1).put(1, 2).code(0x30 + 0x61, 8).code(0xC6, 8).done(64), 64});              // symbol 286
    bad.push_back({BitWriter().put(1, 1).put(1, 2).code(0x30 + 0x61, 8).code(1, 7).code(30, 5).done(64), 64});     // distance 30
    bad.push_back({BitWriter().put(1, 1).put(1, 2).code(0x30 + 0x61, 8).code(1, 7).code(1, 5).code(0, 7).done(64), 4});   // before the start
    bad.push_back({Bytes(dyn.begin(), dyn.begin() + (long)dyn.size() / 2), CHUNK});     // cut in half
    bad.push_back({dyn, CHUNK - 1});                                                    // more than expected
    bad.push_back({fix, CHUNK + 1});                                                    // fewer than expected
    {
        BitWriter w;                                                                    // final block missing
        w.put(0, 1).put(0, 2).align().put(CHUNK, 16).put(~(uint32_t)CHUNK & 0xFFFFu, 16).raw(d);
        bad.push_back({w.done(0), CHUNK});
    }
    s = fix; s.back() ^= 0xFF;
    bad.push_back({s, CHUNK});                                                          // Adler-32
    for (size_t k = 0; k < bad.size(); ++k) {
        if (inflate_exact(bad[k].first, bad[k].second) != OMR_INTERNAL) {
            std::printf("FAILED: malformed stream %zu is not OMR_INTERNAL\n", k);
            ++g_fail;
        }
        if (bad[k].second == (size_t)CHUNK) {
            put_bytes("0/0.0.0.0.0", bad[k].first);
            CHECK(run() == OMR_INTERNAL);
        }
    }
    write_good();

    // random damage: any status, no bad access (the sanitizers are the check)
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto next = [&] {
        rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17;
        return rng;
    };
    auto damage = [&](Bytes f) {
        const int hits = 1 + (int)(next() % 4);
        for (int k = 0; k < hits && !f.empty(); ++k)
            f[next() % f.size()] = next() % 3 ? (uint8_t)next() : (uint8_t)(next() % 2 ? 0xFF : 0x00);
        if (next() % 7 == 0 && !f.empty()) f.resize(next() % f.size());
        return f;
    };
    int ok_streams = 0;
    const Bytes st100 = stored_stream(d, 100);
    for (int it = 0; it < 20000; ++it) {
        const Bytes& src = it % 3 == 0 ? dyn : it % 3 == 1 ? fix : st100;
        ok_streams += inflate_exact(damage(src), it % 11 == 0 ? (size_t)(next() % 2000) : (size_t)CHUNK) == OMR_OK;
    }
    int opened = 0;
    const Bytes meta(good.begin(), good.end()), attrs(kZattrs, kZattrs + std::strlen(kZattrs));
    for (int it = 0; it < 3000; ++it) {
        const int what = it % 3;
        if (what == 0) put_bytes("0/.zarray", damage(meta));
        else if (what == 1) put_bytes(".zattrs", damage(attrs));
        else put_bytes("0/0.1.0.0.1", damage(g_streams[5]));
        opened += run() == OMR_OK;
        if (what == 0) put_bytes("0/.zarray", meta);
        else if (what == 1) put_bytes(".zattrs", attrs);
        else put_bytes("0/0.1.0.0.1", g_streams[5]);
    }
    std::printf("zarr_read_check: %d of 20000 damaged streams and %d of 3000 damaged groups still read\n", ok_streams, opened);
    const std::string rm = "rm -rf '" + g_dir + "'";
    if (std::system(rm.c_str()) != 0) std::printf("could not remove %s\n", g_dir.c_str());
    std::printf(g_fail ? "zarr_read_check: %d check(s) failed\n" : "zarr_read_check: ok\n", g_fail);
    return g_fail ? 1 : 0;
}
