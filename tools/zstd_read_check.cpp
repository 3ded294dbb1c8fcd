// zstd_read_check.cpp — the host Zstandard decoder and omr_zstd_frame_forms (omr_zstd.cpp),
// omr_blosc_decode_host_ex (omr_blosc.cpp) and omr_zarr_image_open_ex / omr_zarr_image_get_tile on a
// Blosc-Zstd and a zstd group (omr_zarr.cpp, K16) under AddressSanitizer and UBSan, as a stand-alone
// CPU program.  Its inputs are files that tests/zstd_streams.py dump() wrote (argv[1]): good frames
// (libzstd's from tests/golden, crafted and edge ones), the malformed frames of the tests, Blosc
// chunks and two groups.  Good inputs must read back; then every frame is truncated at every length
// and damaged byte by byte at random, from a fixed seed, chunks and chunk files likewise; every
// damaged input must be answered with OMR_OK or OMR_INTERNAL, never with a read or write out of
// bounds.  The decoders' buffers are exactly as large as their data, so a byte touched past one is
// caught.
// Built and run by `make -C omero-ms-image-region_amd zstd-read-check`.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "read_check_stubs.h"

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

typedef std::vector<uint8_t> Bytes;

static Bytes slurp(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    return Bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
static void spit(const std::string& path, const Bytes& b) {
    std::ofstream f(path, std::ios::binary | std::ios::trunc);
    f.write(reinterpret_cast<const char*>(b.data()), (std::streamsize)b.size());
}

static uint64_t g_seed = 0x243F6A8885A308D3ull;
static uint32_t rnd() {
    g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_seed >> 33);
}

// The decoder on an input copied into a buffer of exactly its size, into one of exactly `expected`.
static omr_status zstd(const Bytes& in, size_t n, size_t expected, Bytes* out = nullptr) {
    Bytes src(in.begin(), in.begin() + (std::ptrdiff_t)n), dst(expected);
    const omr_status st = omr_zstd_decode_host(src.data(), src.size(), dst.data(), expected);
    uint32_t forms[OMR_ZSTD_FORM_WORDS];
    const omr_status sf = omr_zstd_frame_forms(src.data(), src.size(), forms);
    CHECK(sf == OMR_OK || sf == OMR_INTERNAL);
    if (st == OMR_OK) CHECK(sf == OMR_OK);                 // what decodes can be walked
    if (out) *out = dst;
    return st;
}
static omr_status blosc(const Bytes& in, size_t expected, uint32_t inner) {
    Bytes src(in), dst(expected);
    return omr_blosc_decode_host_ex(src.data(), src.size(), dst.data(), expected, inner);
}
static Bytes damage(const Bytes& good) {
    Bytes b(good);
    for (uint32_t k = 0, n = 1 + rnd() % 3; k < n && !b.empty(); ++k) b[rnd() % b.size()] ^= (uint8_t)(1 + rnd() % 255);
    return b;
}

static void check_group(const std::string& dir, const char* name, uint32_t codecs, const Bytes& pixels) {
    const std::string path = dir + "/" + name;
    omr_zarr_open_options opt = {sizeof(omr_zarr_open_options), codecs};
    omr_zarr_image* img = nullptr;
    CHECK(omr_zarr_image_open_ex(path.c_str(), &opt, &img) == OMR_OK);
    if (!img) return;
    omr_zarr_info info;
    CHECK(omr_zarr_image_info(img, &info) == OMR_OK);
    const size_t bytes = (size_t)info.size_x * info.size_y * 2;
    CHECK(bytes == pixels.size());
    Bytes out(bytes);
    CHECK(omr_zarr_image_get_tile(img, 0, 0, 0, 0, 0, 0, info.size_x, info.size_y, out.data(), out.size()) == OMR_OK);
    CHECK(out == pixels);
    // every chunk file truncated and damaged in place, read through the image, and put back
    int refused = 0;
    for (int cy = 0; cy < 2; ++cy)
        for (int cx = 0; cx < 2; ++cx) {
            const std::string file = path + "/0/0.0.0." + std::to_string(cy) + "." + std::to_string(cx);
            const Bytes good = slurp(file);
            CHECK(!good.empty());
            for (int k = 0; k < 300; ++k) {
                Bytes bad = k < 100 ? Bytes(good.begin(), good.begin() + (std::ptrdiff_t)(rnd() % good.size())) : damage(good);
                spit(file, bad);
                Bytes tile((size_t)64 * 48 * 2);
                const omr_status st = omr_zarr_image_get_tile(img, 0, 0, 0, 0, cx * 64, cy * 48, 64, 48, tile.data(), tile.size());
                CHECK(st == OMR_OK || st == OMR_INTERNAL);
                refused += st == OMR_INTERNAL;
            }
            spit(file, good);
        }
    CHECK(refused > 400);
    CHECK(omr_zarr_image_get_tile(img, 0, 0, 0, 0, 0, 0, info.size_x, info.size_y, out.data(), out.size()) == OMR_OK);
    CHECK(out == pixels);
    omr_zarr_image_close(img);
    // the group does not open under the other bits
    CHECK(omr_zarr_image_open(path.c_str(), &img) == OMR_INVALID_ARGUMENT);
    opt.codecs = OMR_ZARR_CODEC_ZLIB | OMR_ZARR_CODEC_BLOSC;
    CHECK(omr_zarr_image_open_ex(path.c_str(), &opt, &img) == OMR_INVALID_ARGUMENT);
    opt.codecs = codecs | 4u;
    CHECK(omr_zarr_image_open_ex(path.c_str(), &opt, &img) == OMR_INVALID_ARGUMENT);
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::printf("usage: zstd_read_check <directory written by zstd_streams.dump>\n");
        return 2;
    }
    const std::string dir = argv[1];
    std::ifstream index(dir + "/index.txt");
    std::string kind, file;
    size_t expected;
    int good = 0, bad = 0, chunks = 0, accepted = 0;
    long cases = 0;
    while (index >> kind >> file >> expected) {
        const Bytes in = slurp(dir + "/" + file);
        if (kind == "good") {
            ++good;
            CHECK(zstd(in, in.size(), expected) == OMR_OK);
            if (expected) CHECK(zstd(in, in.size(), expected - 1) == OMR_INTERNAL);
            CHECK(zstd(in, in.size(), expected + 1) == OMR_INTERNAL);
            for (size_t n = 0; n < in.size(); ++n, ++cases) CHECK(zstd(in, n, expected) == OMR_INTERNAL);   // every length
            const int rounds = in.size() < 2000 ? 2000 : in.size() < 20000 ? 300 : 60;
            for (int k = 0; k < rounds; ++k, ++cases) {
                const Bytes b = damage(in);
                const omr_status st = zstd(b, b.size(), expected);
                CHECK(st == OMR_OK || st == OMR_INTERNAL);
                accepted += st == OMR_OK;
            }
        } else if (kind == "bad") {
            ++bad;
            CHECK(zstd(in, in.size(), expected) == OMR_INTERNAL);
            for (int k = 0; k < 200; ++k, ++cases) {
                const Bytes b = damage(in);
                const omr_status st = zstd(b, b.size(), expected);
                CHECK(st == OMR_OK || st == OMR_INTERNAL);
            }
        } else if (kind == "blosc") {
            ++chunks;
            CHECK(blosc(in, expected, OMR_BLOSC_INNER_ZSTD) == OMR_OK);
            CHECK(blosc(in, expected, OMR_BLOSC_INNER_LZ4 | OMR_BLOSC_INNER_ZSTD) == OMR_OK);
            CHECK(blosc(in, expected, OMR_BLOSC_INNER_LZ4) == OMR_INTERNAL);
            CHECK(blosc(in, expected, 0u) == OMR_INVALID_ARGUMENT);
            CHECK(blosc(in, expected, 4u) == OMR_INVALID_ARGUMENT);
            {
                Bytes src(in), dst(expected);
                CHECK(omr_blosc_decode_host(src.data(), src.size(), dst.data(), expected) == OMR_INTERNAL);
            }
            for (int k = 0; k < 1500; ++k, ++cases) {
                const Bytes b = k < 500 ? Bytes(in.begin(), in.begin() + (std::ptrdiff_t)(rnd() % in.size())) : damage(in);
                const omr_status st = blosc(b, expected, OMR_BLOSC_INNER_LZ4 | OMR_BLOSC_INNER_ZSTD);
                CHECK(st == OMR_OK || st == OMR_INTERNAL);
            }
        }
    }
    CHECK(good >= 40 && bad >= 40 && chunks == 4);
    const Bytes pixels = slurp(dir + "/pixels.bin");
    check_group(dir, "g_blosc", OMR_ZARR_CODEC_BLOSC_ZSTD, pixels);
    check_group(dir, "g_zstd", OMR_ZARR_CODEC_ZSTD, pixels);
    std::printf("zstd_read_check: %d good and %d malformed frames, %d chunks, %ld truncated or damaged inputs (%d accepted), "
                "2 groups: %s\n", good, bad, chunks, cases, accepted, g_fail ? "FAILED" : "ok");
    return g_fail ? 1 : 0;
}
