// jpeg_split_check.cpp — the split JPEG entropy decode on the host (omr_jpeg_decode_host_split,
// omr_jpegdec.cpp, with the per-lane decoder of omr_jpegdec.h that K18a runs on the device) against
// the serial decoder (omr_jpeg_decode_host) under AddressSanitizer and UBSan, as a stand-alone CPU
// program.  Its argument is a directory that `tools/make_tiff_jpeg_golden.py --unpack` and
// `tools/make_jpeg_split_golden.py --unpack` have written, in a Python that never sees this
// program: every stream of tests/golden/tiff_jpeg.npz and tests/golden/jpeg_split.npz.  At
// subsequences of 32, 64 and 1024 bits and workgroups of 1, 3, 64 and 256 lanes, on the good
// streams, on every truncation of some and on a few thousand seeded damaged copies, both decoders
// must return the same status and, on OMR_OK, the same bytes; the copies are exactly as long as the
// stream and the output exactly as large as the frame, so a read or write past either is caught.
// Built and run by `make -C omero-ms-image-region_amd jpeg-split-check`.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "omr/omr.h"

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

static std::vector<uint8_t> slurp(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static uint32_t g_rng = 181818u;
static uint32_t rnd() {
    g_rng = g_rng * 1664525u + 1013904223u;
    return g_rng >> 8;
}

struct Stream {
    std::string name;
    int k, w, h, spp, ycc;
    std::vector<uint8_t> tables, bytes;
};

static const uint32_t kBits[] = {32, 64, 1024}, kLanes[] = {1, 3, 64, 256};
static size_t g_decodes = 0, g_good = 0;

// The serial decode of len bytes, then the split decode at the given configurations (all: 12 of them).
static omr_status compare(const Stream& s, const uint8_t* src, size_t len, bool all) {
    const size_t n = (size_t)s.w * s.h * s.spp;
    std::vector<uint8_t> copy(src, src + len), tcopy(s.tables), want(n), got(n);
    const uint8_t* t = tcopy.empty() ? nullptr : tcopy.data();
    const omr_status st = omr_jpeg_decode_host(t, tcopy.size(), copy.data(), copy.size(), s.w, s.h, s.spp, s.ycc, want.data(), nullptr, 0);
    const uint32_t pick = rnd();
    for (int b = 0; b < 3; ++b)
        for (int l = 0; l < 4; ++l) {
            if (!all && (uint32_t)(b * 4 + l) != pick % 12u && (uint32_t)(b * 4 + l) != (pick / 12u) % 12u) continue;
            omr_jpeg_split_stats stats;
            std::memset(got.data(), 0x5A, n);
            const omr_status sp = omr_jpeg_decode_host_split(t, tcopy.size(), copy.data(), copy.size(), s.w, s.h, s.spp, s.ycc,
                                                             kBits[b], kLanes[l], got.data(), &stats);
            ++g_decodes;
            if (sp != st || (st == OMR_OK && got != want)) {
                std::printf("FAILED %s.%d len %zu S %u lanes %u: serial %d split %d\n", s.name.c_str(), s.k, len, kBits[b], kLanes[l],
                            (int)st, (int)sp);
                ++g_fail;
            }
        }
    if (st == OMR_OK) ++g_good;
    return st;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        std::printf("usage: jpeg_split_check DIR\n");
        return 2;
    }
    const std::string dir = argv[1];
    std::vector<Stream> streams;
    for (const char* list : {"/streams.txt", "/split_streams.txt"}) {
        std::ifstream idx(dir + list);
        Stream s;
        size_t tl;
        while (idx >> s.name >> s.k >> s.w >> s.h >> s.spp >> s.ycc >> tl) {
            s.tables = slurp(dir + "/" + s.name + ".tables");
            s.bytes = slurp(dir + "/" + s.name + "." + std::to_string(s.k) + ".jpg");
            CHECK(s.tables.size() == tl && !s.bytes.empty());
            streams.push_back(s);
        }
    }
    CHECK(streams.size() > 55);
    size_t n_trunc = 0, n_damaged = 0;
    for (const Stream& s : streams) {
        CHECK(compare(s, s.bytes.data(), s.bytes.size(), true) == OMR_OK);
        // every truncation of the short streams (two configurations each), every 37th of the long ones
        const size_t step = s.bytes.size() < 3000 && (s.k == 0 || s.name == "ycc420_rst_q95_opt") ? 1 : 37;
        for (size_t cut = 1; cut < s.bytes.size(); cut += step, ++n_trunc) {
            CHECK(compare(s, s.bytes.data(), cut, false) != OMR_OK);
            // the same cut with an EOI behind it: the header parser lets it through, the interval runs out of bits
            std::vector<uint8_t> b(s.bytes.begin(), s.bytes.begin() + cut);
            b.push_back(0xFF);
            b.push_back(0xD9);
            compare(s, b.data(), b.size(), false);
        }
    }
    const size_t good_before = g_good;
    for (int round = 0; round < 4000; ++round, ++n_damaged) {
        const Stream& s = streams[rnd() % streams.size()];
        std::vector<uint8_t> b = s.bytes;
        const int hits = 1 + (int)(rnd() % 3);
        for (int k = 0; k < hits; ++k) {
            // most hits behind the header, where the entropy-coded bytes are
            const size_t lo = (rnd() % 8) ? std::min<size_t>(b.size() - 1, 600) : 0;
            const size_t at = lo + rnd() % (b.size() - lo);
            switch (rnd() % 4) {
            case 0: b[at] = (uint8_t)rnd(); break;
            case 1: b[at] ^= (uint8_t)(1u << (rnd() % 8)); break;
            case 2: b[at] = 0xFF; break;                   // an FF without its 00, or a marker
            default: b[at] = 0x00; break;
            }
        }
        compare(s, b.data(), b.size(), false);
    }
    std::printf("streams: %zu good, %zu truncations, %zu damaged copies (%zu of them still decode), %zu split decodes\n", streams.size(),
                n_trunc, n_damaged, g_good - good_before, g_decodes);
    std::printf(g_fail ? "jpeg_split_check: %d FAILED\n" : "jpeg_split_check: ok\n", g_fail);
    return g_fail ? 1 : 0;
}
