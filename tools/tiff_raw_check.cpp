// tiff_raw_check.cpp — the raw TIFF host writer (omr_tiff.cpp, K12) under AddressSanitizer and
// UBSan, as a stand-alone CPU program: every pixel type, both input byte orders, sizes around the
// strip rule, each into a buffer of exactly omr_tiff_raw_max_bytes (so a byte written past it is
// caught), the strips read back through the IFD and compared with the pixels, and the rejected
// arguments.  Built and run by `make -C omero-ms-image-region_amd tiff-raw-check`.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "omr_internal.h"

// what omr_tiff.cpp takes from the rest of the library
namespace omr {
int bytes_per_pixel(int32_t t) {
    switch (t) {
    case OMR_PIXELS_INT8: case OMR_PIXELS_UINT8: return 1;
    case OMR_PIXELS_INT16: case OMR_PIXELS_UINT16: return 2;
    case OMR_PIXELS_INT32: case OMR_PIXELS_UINT32: case OMR_PIXELS_FLOAT: return 4;
    case OMR_PIXELS_DOUBLE: return 8;
    default: return 0;
    }
}
omr_status fail(Ctx*, omr_status s, const std::string&) { return s; }
omr_status hip_fail(Ctx*, hipError_t, const char*) { return OMR_DEVICE; }
}  // namespace omr

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

static uint32_t be16(const uint8_t* p) { return (uint32_t)p[0] << 8 | p[1]; }
static uint32_t be32(const uint8_t* p) { return be16(p) << 16 | be16(p + 2); }

// {count, first value or offset of the values} of IFD tag `id`
static bool find_tag(const std::vector<uint8_t>& f, uint32_t id, uint32_t& type, uint32_t& count, uint32_t& value) {
    const uint32_t ifd = be32(&f[4]), n = be16(&f[ifd]);
    for (uint32_t k = 0; k < n; ++k) {
        const uint8_t* e = &f[ifd + 2 + 12 * k];
        if (be16(e) != id) continue;
        type = be16(e + 2);
        count = be32(e + 4);
        value = type == 3 && count == 1 ? be16(e + 8) : be32(e + 8);
        return true;
    }
    return false;
}

static void one(int pt, int be, int w, int h) {
    const int bps = omr::bytes_per_pixel(pt);
    std::vector<uint8_t> px((size_t)w * h * bps);
    for (size_t i = 0; i < px.size(); ++i) px[i] = (uint8_t)(i * 131 + pt * 7 + 3);
    const size_t cap = omr_tiff_raw_max_bytes(w, h, pt);
    CHECK(cap > px.size());
    std::vector<uint8_t> out(cap);                       // exactly cap: ASan guards the byte after
    size_t len = 0;
    CHECK(omr_encode_tiff_raw(px.data(), pt, be, w, h, out.data(), cap, &len) == OMR_OK);
    CHECK(len == cap);
    uint32_t type, count, value, cnt_type, cnt_count, cnt_value;
    CHECK(find_tag(out, 258, type, count, value) && value == 8u * bps);
    CHECK(find_tag(out, 273, type, count, value) && find_tag(out, 279, cnt_type, cnt_count, cnt_value));
    CHECK(count == cnt_count);
    std::vector<uint8_t> strips;
    for (uint32_t s = 0; s < count; ++s) {
        const uint32_t off = count == 1 ? value : be32(&out[value + 4 * s]);
        const uint32_t n = count == 1 ? cnt_value : be32(&out[cnt_value + 4 * s]);
        CHECK((size_t)off + n <= out.size());
        if ((size_t)off + n <= out.size()) strips.insert(strips.end(), out.begin() + off, out.begin() + off + n);
    }
    CHECK(strips.size() == px.size());
    bool same = strips.size() == px.size();
    for (size_t i = 0; same && i < px.size(); ++i) {
        const size_t s = i / bps * bps, k = i - s;       // sample start, byte in it
        same = strips[i] == (be ? px[i] : px[s + bps - 1 - k]);
    }
    CHECK(same);
    if (cap > 1) {
        std::vector<uint8_t> small(cap - 1);
        CHECK(omr_encode_tiff_raw(px.data(), pt, be, w, h, small.data(), cap - 1, &len) == OMR_BUFFER_TOO_SMALL);
        CHECK(len == cap);
    }
}

int main() {
    const int sizes[][2] = {{1, 1}, {7, 3}, {300, 200}, {1000, 37}, {8191, 2}, {8192, 3}, {8193, 2}, {1, 9000}, {4096, 5}};
    for (int pt = OMR_PIXELS_INT8; pt <= OMR_PIXELS_DOUBLE; ++pt)
        for (int be = 0; be < 2; ++be)
            for (const auto& s : sizes) one(pt, be, s[0], s[1]);
    uint8_t px[16] = {}, out[512];
    size_t len = 0;
    CHECK(omr_encode_tiff_raw(nullptr, OMR_PIXELS_UINT8, 1, 4, 4, out, sizeof out, &len) == OMR_INVALID_ARGUMENT);
    CHECK(omr_encode_tiff_raw(px, 8, 1, 4, 4, out, sizeof out, &len) == OMR_INVALID_ARGUMENT);
    CHECK(omr_encode_tiff_raw(px, -1, 1, 4, 4, out, sizeof out, &len) == OMR_INVALID_ARGUMENT);
    CHECK(omr_encode_tiff_raw(px, OMR_PIXELS_UINT8, 1, 0, 4, out, sizeof out, &len) == OMR_INVALID_ARGUMENT);
    CHECK(omr_encode_tiff_raw(px, OMR_PIXELS_UINT8, 1, 4, 65536, out, sizeof out, &len) == OMR_INVALID_ARGUMENT);
    CHECK(omr_encode_tiff_raw(px, OMR_PIXELS_UINT8, 1, 4, 4, nullptr, 0, &len) == OMR_BUFFER_TOO_SMALL);
    CHECK(omr_encode_tiff_raw(px, OMR_PIXELS_UINT8, 1, 4, 4, out, sizeof out, nullptr) == OMR_OK);
    CHECK(omr_tiff_raw_max_bytes(65535, 65535, OMR_PIXELS_DOUBLE) == 0);
    std::printf(g_fail ? "tiff_raw_check: %d check(s) failed\n" : "tiff_raw_check: ok\n", g_fail);
    return g_fail ? 1 : 0;
}
