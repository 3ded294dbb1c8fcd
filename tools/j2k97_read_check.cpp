// j2k97_read_check.cpp — j2k_read_check for the irreversible path (K20): j2k_prepare with the 9/7
// transform and scalar quantisation taken, the host decoder's float half and omr_j2k_stream_forms_ex
// (omr_j2kdec.cpp) and omr_tiff_image_open_ex / get_tile on TIFFs with irreversible and mixed JPEG
// 2000 segments (omr_tiffread.cpp) under AddressSanitizer and UBSan, as a stand-alone CPU program.
// Its argument is a directory written by `tools/make_tiff_j2k97_golden.py --unpack` from
// tests/golden/tiff_j2k97.npz, in a Python that never sees this program: the fixture's streams and
// files with OpenJPEG's pixels and the number of samples the host decoder may differ from them on
// (by 1; the fixture's tool counted them).  Good streams and files must decode to that; every
// truncation of every stream must be answered with a failure, and a few thousand copies damaged at
// random (streams and files) with a status, never with a read or write out of bounds: the input
// copies and the output buffers are exactly as large as the stream and the segment, so a byte read
// or written past one is caught.  A damaged stream that still decodes must decode to the same
// bytes twice.  Of every plan j2k_prepare accepts its promises are checked, among them that every
// block of an irreversible plan has a finite, positive step (and a reversible one step 0).
// Built and run by `make -C omero-ms-image-region_amd j2k97-read-check`.
#include <unistd.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "omr_j2kdec.h"
#include "read_check_stubs.h"

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

static std::vector<uint8_t> slurp(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static void spit(const std::string& path, const uint8_t* p, size_t n) {
    std::ofstream f(path, std::ios::binary | std::ios::trunc);
    f.write(reinterpret_cast<const char*>(p), (std::streamsize)n);
}

static uint32_t g_rng = 12345u;
static uint32_t rnd() {
    g_rng = g_rng * 1664525u + 1013904223u;
    return g_rng >> 8;
}

struct Stream {
    std::string name;
    int w, h, spp, bits;
    long differing;
    std::vector<uint8_t> bytes, px;
};

// got against OpenJPEG's pixels: no sample more than 1 off, at most `differing` samples off at all.
static bool agrees(const std::vector<uint8_t>& got, const std::vector<uint8_t>& want, int bits, long differing) {
    if (got.size() != want.size()) return false;
    long n = 0;
    for (size_t i = 0; i < got.size(); i += (size_t)bits / 8) {
        long a = got[i], b = want[i];
        if (bits == 16) {
            uint16_t x, y;
            std::memcpy(&x, &got[i], 2);
            std::memcpy(&y, &want[i], 2);
            a = x;
            b = y;
        }
        if (std::labs(a - b) > 1) return false;
        n += a != b;
    }
    return n <= differing;
}

// One decode into a buffer of exactly the segment's size; returns the status.  What j2k_prepare
// promises of its plan is checked on every stream it accepts.
static omr_status decode(const Stream& s, const uint8_t* src, size_t len, std::vector<uint8_t>* out = nullptr) {
    std::vector<uint16_t> dst(((size_t)s.w * s.h * s.spp * (s.bits / 8) + 1) / 2);
    std::vector<uint8_t> copy(src, src + len);               // exactly len bytes: a read past them is caught
    char why[64];
    const omr_status st = omr_j2k_decode_host_ex(copy.data(), copy.size(), s.w, s.h, s.spp, s.bits, OMR_J2K_ALLOW_IRREVERSIBLE,
                                                 reinterpret_cast<uint8_t*>(dst.data()), why, sizeof why);
    omr::J2kPlan plan;
    const omr_status sp = omr::j2k_prepare(copy.data(), copy.size(), s.w, s.h, s.spp, s.bits, plan, nullptr,
                                           omr::kJ2kTakeReversible | omr::kJ2kTakeIrreversible);
    CHECK(sp == st || copy.empty());                         // (no bytes at all: the entry point refuses the null pointer)
    if (sp == OMR_OK) {
        const uint64_t area = (uint64_t)s.w * s.h * plan.ncomp;
        uint64_t covered = 0;
        for (const omr::J2kBlock& b : plan.blocks) {
            CHECK(b.w >= 1 && b.h >= 1 && (uint32_t)b.w * b.h <= omr::kJ2kMaxBlockArea);
            CHECK((uint64_t)b.ws_off + (uint64_t)(b.h - 1) * b.stride + b.w <= area);
            CHECK(b.passes == 0 || (b.planes <= omr::kJ2kMaxPlanes && b.passes <= 3 * b.planes - 2));
            CHECK((uint64_t)b.range0 + b.n_ranges <= plan.ranges.size());
            CHECK(plan.lossy ? std::isfinite(b.step) && b.step > 0.f : b.step == 0.f);
            covered += (uint64_t)b.w * b.h;
        }
        CHECK(covered == area);
        for (const omr::J2kRange& r : plan.ranges) CHECK((uint64_t)r.off + r.len <= copy.size());
        uint64_t forms = 0;
        uint32_t lossy = 0;
        CHECK(omr_j2k_stream_forms_ex(copy.data(), copy.size(), OMR_J2K_ALLOW_IRREVERSIBLE, &forms, &lossy) == OMR_OK);
        CHECK((lossy != 0) == plan.lossy && lossy == plan.lossy_forms);
        // without the flag the same stream is refused, or was reversible all along
        CHECK((omr_j2k_stream_forms(copy.data(), copy.size(), &forms) == OMR_OK) == !plan.lossy);
    }
    if (out) out->assign(reinterpret_cast<uint8_t*>(dst.data()), reinterpret_cast<uint8_t*>(dst.data()) + (size_t)s.w * s.h * s.spp * (s.bits / 8));
    return st;
}

// Every channel of the whole image through open_ex / get_tile; OMR_OK only when all of it read.
static omr_status read_file(const std::string& path, int nc, int w, int h, int bits, std::vector<uint8_t>* planes) {
    omr_tiff_open_options opt = {sizeof(omr_tiff_open_options),
                                 OMR_TIFF_ACCEPT_JPEG2000 | OMR_TIFF_ACCEPT_JPEG2000_LOSSY | OMR_TIFF_ACCEPT_SAMPLES};
    omr_tiff_image* img = nullptr;
    omr_status st = omr_tiff_image_open_ex(path.c_str(), 1, nc, 1, "XYZCT", &opt, &img);
    if (st) return st;
    omr_tiff_info info;
    CHECK(omr_tiff_image_info(img, &info) == OMR_OK);
    if (info.size_x != w || info.size_y != h || info.pixel_type != (bits == 8 ? OMR_PIXELS_UINT8 : OMR_PIXELS_UINT16)) {
        omr_tiff_image_close(img);
        return OMR_INVALID_ARGUMENT;
    }
    const size_t plane = (size_t)w * h * (bits / 8);
    std::vector<uint8_t> buf(plane);
    if (planes) planes->clear();
    for (int c = 0; c < nc && !st; ++c) {
        st = omr_tiff_image_get_tile(img, 0, 0, c, 0, 0, 0, w, h, buf.data(), buf.size());
        if (!st && planes) {
            if (bits == 16 && info.big_endian)               // the stored pixels are in the host's order
                for (size_t i = 0; i + 1 < plane; i += 2) std::swap(buf[i], buf[i + 1]);
            planes->insert(planes->end(), buf.begin(), buf.end());
        }
    }
    omr_tiff_image_close(img);
    return st;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        std::printf("usage: j2k97_read_check DIR\n");
        return 2;
    }
    const std::string dir = argv[1];
    std::vector<Stream> streams;
    {
        std::ifstream idx(dir + "/streams.txt");
        Stream s;
        while (idx >> s.name >> s.w >> s.h >> s.spp >> s.bits >> s.differing) {
            s.bytes = slurp(dir + "/" + s.name + ".j2k");
            s.px = slurp(dir + "/" + s.name + ".px");
            CHECK(!s.bytes.empty() && s.px.size() == (size_t)s.w * s.h * s.spp * (s.bits / 8));
            streams.push_back(s);
        }
    }
    CHECK(streams.size() >= 16);
    size_t n_trunc = 0, n_damaged = 0, n_still_good = 0;
    for (const Stream& s : streams) {
        std::vector<uint8_t> got;
        CHECK(decode(s, s.bytes.data(), s.bytes.size(), &got) == OMR_OK);
        CHECK(agrees(got, s.px, s.bits, s.differing));
        const size_t step = s.bytes.size() > 4000 ? 29 : 1;  // every truncation of the short streams, every 29th of the long
        for (size_t cut = 0; cut < s.bytes.size(); cut += step, ++n_trunc) CHECK(decode(s, s.bytes.data(), cut) != OMR_OK);
    }
    for (int round = 0; round < 3000; ++round) {
        const Stream& s = streams[rnd() % streams.size()];
        std::vector<uint8_t> b = s.bytes;
        const int hits = 1 + (int)(rnd() % 3);
        for (int k = 0; k < hits; ++k) {
            // half of the hits into the headers, where the structure is
            const size_t span = (rnd() & 1) ? std::min<size_t>(b.size(), 200) : b.size();
            b[rnd() % span] = (rnd() & 1) ? (uint8_t)rnd() : (uint8_t)(0xFF * (rnd() & 1));
        }
        ++n_damaged;
        std::vector<uint8_t> one, two;
        if (decode(s, b.data(), b.size(), &one) == OMR_OK) {
            ++n_still_good;
            CHECK(decode(s, b.data(), b.size(), &two) == OMR_OK && one == two);
        }
    }
    std::printf("streams: %zu good, %zu truncations, %zu damaged copies (%zu of them still decode)\n", streams.size(), n_trunc,
                n_damaged, n_still_good);

    std::ifstream idx(dir + "/files.txt");
    std::string name;
    int nc, w, h, bits;
    long differing;
    const std::string tmp = dir + "/damaged.tif";
    size_t n_files = 0, n_file_trunc = 0, n_file_damaged = 0;
    while (idx >> name >> w >> h >> nc >> bits >> differing) {
        const std::string path = dir + "/" + name + ".tif";
        const std::vector<uint8_t> file = slurp(path), px = slurp(path + ".px");
        CHECK(px.size() == (size_t)w * h * nc * (bits / 8));
        std::vector<uint8_t> got;
        CHECK(read_file(path, nc, w, h, bits, &got) == OMR_OK);
        CHECK(agrees(got, px, bits, differing));
        ++n_files;
        omr_tiff_image* img = nullptr;                       // refused without its bit
        CHECK(omr_tiff_image_open(path.c_str(), 1, nc, 1, "XYZCT", &img) == OMR_INVALID_ARGUMENT);
        omr_tiff_open_options opt = {sizeof(omr_tiff_open_options), OMR_TIFF_ACCEPT_SAMPLES | OMR_TIFF_ACCEPT_DEFLATE | OMR_TIFF_ACCEPT_JPEG};
        CHECK(omr_tiff_image_open_ex(path.c_str(), 1, nc, 1, "XYZCT", &opt, &img) == OMR_INVALID_ARGUMENT);
        for (size_t cut = 0; cut < file.size(); cut += 13, ++n_file_trunc) {
            spit(tmp, file.data(), cut);
            CHECK(read_file(tmp, nc, w, h, bits, nullptr) != OMR_OK);
        }
        for (int round = 0; round < 100; ++round, ++n_file_damaged) {
            std::vector<uint8_t> b = file;
            const int hits = 1 + (int)(rnd() % 3);
            for (int k = 0; k < hits; ++k) b[rnd() % b.size()] = (rnd() & 1) ? (uint8_t)rnd() : (uint8_t)(0xFF * (rnd() & 1));
            spit(tmp, b.data(), b.size());
            (void)read_file(tmp, nc, w, h, bits, nullptr);
        }
    }
    CHECK(n_files >= 6);
    ::unlink(tmp.c_str());
    std::printf("files: %zu good, %zu truncations, %zu damaged copies\n", n_files, n_file_trunc, n_file_damaged);
    std::printf(g_fail ? "j2k97-read-check: %d FAILED\n" : "j2k97-read-check: ok\n", g_fail);
    return g_fail ? 1 : 0;
}
