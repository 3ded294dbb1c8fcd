// omr_j2kdec.cpp — K19 and K20, host half: JPEG 2000 codestreams, reversible (K19) and irreversible
// (K20), the segments of a TIFF with Compression 33003, 33004, 33005 or 34712.
//
// j2k_prepare parses the main header and the one tile-part header and walks tier 2 -- the packets
// in the stream's progression order, the inclusion and zero-bit-plane tag trees, the pass counts,
// Lblock and the segment lengths, with the bit stuffing behind an FF -- and lists every code-block
// with the byte ranges the layers give it.  omr_j2k_decode_host (get_tile's decoder and the
// reference of the device route) decodes the blocks, runs the inverse 5/3 transform level by level
// and stores the pixels, all through the functions of omr_j2kdec.h, which the kernels of
// omr_j2kdec.hip share.  omr_j2k_stream_forms reports the coding forms a stream uses.
//
// All input is user-uploaded bytes.  Every read of the stream is behind a comparison with its
// length; sizes are computed in 64 bits and compared with the caller's width and height before
// anything is allocated; the numbers of precincts and code-blocks are bounded by the frame's
// area, and the walk over the packets ends when the stream does, since every packet takes a bit.
//
// In scope: one tile that covers the image, one tile-part, offsets 0; 1 or 3 unsigned components
// of 8 or 16 bits without subsampling; the reversible 5/3 transform without quantisation (QCD style
// 0), with the reversible colour transform when COD says so; 0..32 decomposition levels; every legal
// code-block size; user precincts; 1..65535 layers; the five progression orders; COM (and the
// pointer segments TLM, PLM, PLT, CRG, which say nothing the walk needs) skipped.  For a caller that
// takes irreversible streams (kJ2kTakeIrreversible) also the 9/7 transform with QCD style 1 or 2
// and the irreversible colour transform: tier 2 and the code-blocks are the same, j2k_prepare adds
// every block's quantiser step, and the decoder runs the float path of omr_j2kdec.h.
//
// Damage that cannot be seen: without the termination styles (which are refused) nothing in a
// code-block's bytes can be checked, so a damaged packet BODY decodes to defined, in-bounds
// garbage with OMR_OK.  What can be seen is OMR_INTERNAL: a stream cut inside a marker segment or a
// packet header, a packet body that runs past the tile-part, more passes than 3 * planes - 2, more
// zero bit-planes than M_b, a frame size other than the segment's, no EOC.
#include "omr_j2kdec.h"

#include <algorithm>
#include <atomic>
#include <memory>

#include "omr_segread.h"

namespace omr {
namespace {

constexpr uint64_t kMaxDecoded = (uint64_t)256 << 20;
constexpr uint64_t kMaxPrecincts = (uint64_t)1 << 20;
constexpr uint64_t kMaxBlocks = (uint64_t)1 << 22;
constexpr size_t kThreadedCoefficients = (size_t)1 << 16;  // from a 256 x 256 tile on, the blocks go to 16 threads

struct Fail {
    std::string* why;
    omr_status set(omr_status s, const char* what) {
        if (why) *why = what;
        return s;
    }
};

// A tag tree over w x h leaves (T.800 B.10.2).
struct TagTree {
    struct Node {
        int32_t parent;
        uint32_t value, low;
    };
    std::vector<Node> nodes;
    void make(uint32_t w, uint32_t h) {
        nodes.clear();
        std::vector<std::pair<uint32_t, uint32_t>> dims;
        size_t total = 0;
        for (uint32_t a = w, b = h;; a = (a + 1) / 2, b = (b + 1) / 2) {
            dims.push_back({a, b});
            total += (size_t)a * b;
            if (a * b <= 1) break;
        }
        nodes.resize(total);
        size_t base = 0;
        for (size_t l = 0; l < dims.size(); ++l) {
            const uint32_t a = dims[l].first, b = dims[l].second;
            const size_t next = base + (size_t)a * b;
            for (uint32_t y = 0; y < b; ++y)
                for (uint32_t x = 0; x < a; ++x) {
                    Node& n = nodes[base + (size_t)y * a + x];
                    n.parent = l + 1 < dims.size() ? (int32_t)(next + (size_t)(y / 2) * dims[l + 1].first + x / 2) : -1;
                    n.value = 0x7FFFFFFFu;
                    n.low = 0;
                }
            base = next;
        }
    }
};

// The bits of a packet header: behind an FF byte the next holds seven.
struct HeaderBits {
    const uint8_t* s;
    size_t pos, end;
    uint32_t buf = 0;
    int ct = 0;
    bool bad = false, ff = false;
    uint32_t bit() {
        if (ct == 0) {
            const bool after_ff = buf == 0xFFu;
            if (pos >= end) {
                bad = true;
                return 0;
            }
            buf = s[pos++];
            ct = after_ff ? 7 : 8;
            if (buf == 0xFFu) ff = true;
        }
        --ct;
        return (buf >> ct) & 1u;
    }
    uint32_t bits(int n) {                                 // n in [0, 32]
        uint32_t v = 0;
        for (int k = 0; k < n; ++k) v = v << 1 | bit();
        return v;
    }
    void align() {                                         // the header ends on a byte; behind an FF its stuffed byte goes too
        if (buf == 0xFFu) {
            if (pos >= end) bad = true;
            else ++pos;
        }
        buf = 0;
        ct = 0;
    }
};

bool tag_decode(TagTree& T, HeaderBits& B, uint32_t leaf, uint32_t threshold) {
    int32_t stack[40];
    int depth = 0;
    for (int32_t n = (int32_t)leaf; n >= 0 && depth < 40; n = T.nodes[(size_t)n].parent) stack[depth++] = n;
    uint32_t low = 0;
    while (depth) {
        TagTree::Node& n = T.nodes[(size_t)stack[--depth]];
        if (low > n.low) n.low = low;
        else low = n.low;
        while (low < threshold && low < n.value && !B.bad) {
            if (B.bit()) n.value = low;
            else ++low;
        }
        n.low = low;
    }
    return T.nodes[leaf].value < threshold;
}

struct BandGeom {
    uint32_t orient = 0, w = 0, h = 0, ox = 0, oy = 0;     // its size and its place in the nested layout
    int32_t mb = 0;
    float step = 0.f;                                      // K20: half the quantiser step (0: reversible)
};
struct PrecinctBand {
    uint32_t ncw = 0, nch = 0, first = 0;                  // its code-blocks: first .. first + ncw * nch in raster order
    TagTree incl, imsb;
};
struct Precinct {
    PrecinctBand b[3];
};
struct Resolution {
    uint32_t w = 0, h = 0, pw = 0, ph = 0, ppx = 15, ppy = 15;
    int nb = 0;
    BandGeom band[3];
    std::vector<Precinct> prec;
};
struct BlockState {
    bool included = false;
    uint8_t lenbits = 3;
    uint32_t passes = 0;
    int32_t planes = 0;
};
struct Piece {
    uint32_t block, off, len;
};

struct Header {
    int32_t w = 0, h = 0, ncomp = 0, bits = 0;
    int32_t order = 0, layers = 0, levels = 0, xcb = 0, ycb = 0;
    bool mct = false, user_precincts = false;
    uint8_t pp[33] = {0};
    uint8_t guard = 0;
    uint8_t expo[97] = {0};
    uint16_t mant[97] = {0};
    bool lossy = false;                                    // the 9/7 transform
    int qstyle = 0;
    size_t body = 0, body_end = 0;
};

size_t be16(const uint8_t* p) { return (size_t)p[0] << 8 | p[1]; }
uint64_t be32(const uint8_t* p) { return (uint64_t)p[0] << 24 | (uint64_t)p[1] << 16 | (uint64_t)p[2] << 8 | p[3]; }

// The main header and the tile-part header, up to SOD; then what follows the tile-part.
omr_status parse_headers(const uint8_t* src, size_t len, int32_t w, int32_t h, int32_t samples, int32_t bits, uint32_t kinds,
                         Header& H, Fail& F) {
    const bool take97 = (kinds & kJ2kTakeIrreversible) != 0;
    const uint8_t* qcd = nullptr;                          // QCD's body behind Sqcd, looked at once the transform is known
    size_t qcd_n = 0;
    if (len >= 12 && be32(src) == 12 && be32(src + 4) == 0x6A502020u) return F.set(OMR_INVALID_ARGUMENT, "j2k: a JP2 box wrapper");
    if (len < 2 || src[0] != 0xFF || src[1] != 0x4F) return F.set(OMR_INTERNAL, "j2k: no SOC");
    size_t pos = 2;
    bool have_siz = false, have_cod = false, have_qcd = false, in_tile = false;
    size_t sot_at = 0;
    uint64_t psot = 0;
    for (;;) {
        if (len - pos < 2) return F.set(OMR_INTERNAL, "j2k: header cut short");
        if (src[pos] != 0xFF) return F.set(OMR_INTERNAL, "j2k: marker expected");
        const int m = src[pos + 1];
        if (m == 0x93) {                                   // SOD
            if (!in_tile) return F.set(OMR_INTERNAL, "j2k: SOD before SOT");
            pos += 2;
            break;
        }
        if (m == 0xD9 || m == 0x4F) return F.set(OMR_INTERNAL, "j2k: marker out of place");
        if (len - pos < 4) return F.set(OMR_INTERNAL, "j2k: header cut short");
        const size_t L = be16(src + pos + 2);
        if (L < 2 || L > len - pos - 2) return F.set(OMR_INTERNAL, "j2k: header cut short");
        const uint8_t* p = src + pos + 4;
        const size_t n = L - 2;
        if (!have_siz && m != 0x51) return F.set(OMR_INTERNAL, "j2k: SIZ is not the first marker segment");
        switch (m) {
        case 0x51: {                                       // SIZ
            if (have_siz || n < 36) return F.set(OMR_INTERNAL, "j2k: bad SIZ");
            const uint64_t xs = be32(p + 2), ys = be32(p + 6), xo = be32(p + 10), yo = be32(p + 14);
            const uint64_t xt = be32(p + 18), yt = be32(p + 22), xto = be32(p + 26), yto = be32(p + 30);
            const size_t nc = be16(p + 34);
            if (n != 36 + 3 * nc || nc < 1) return F.set(OMR_INTERNAL, "j2k: bad SIZ");
            if (xo || yo || xto || yto) return F.set(OMR_INVALID_ARGUMENT, "j2k: non-zero image or tile offsets");
            if (xt < xs || yt < ys) return F.set(OMR_INVALID_ARGUMENT, "j2k: several tiles");
            if (nc != 1 && nc != 3) return F.set(OMR_INVALID_ARGUMENT, "j2k: component count other than 1 or 3");
            if ((int32_t)nc != samples) return F.set(OMR_INVALID_ARGUMENT, "j2k: component count differs from SamplesPerPixel");
            for (size_t c = 0; c < nc; ++c) {
                const uint8_t* q = p + 36 + 3 * c;
                if (q[0] & 0x80) return F.set(OMR_INVALID_ARGUMENT, "j2k: signed components");
                if (q[1] != 1 || q[2] != 1) return F.set(OMR_INVALID_ARGUMENT, "j2k: subsampled components");
                const int prec = (q[0] & 0x7F) + 1;
                if (prec != 8 && prec != 16) return F.set(OMR_INVALID_ARGUMENT, "j2k: sample precision other than 8 or 16");
                if (prec != bits) return F.set(OMR_INVALID_ARGUMENT, "j2k: sample precision differs from BitsPerSample");
            }
            if (bits == 16 && nc == 3) return F.set(OMR_INVALID_ARGUMENT, "j2k: 16-bit samples with three components");
            if (xs != (uint64_t)w || ys != (uint64_t)h) return F.set(OMR_INTERNAL, "j2k: frame size differs from the segment's");
            H.w = w; H.h = h; H.ncomp = (int32_t)nc; H.bits = bits;
            have_siz = true;
            break;
        }
        case 0x52: {                                       // COD
            if (in_tile) return F.set(OMR_INVALID_ARGUMENT, "j2k: COD in a tile-part header");
            if (n < 10) return F.set(OMR_INTERNAL, "j2k: bad COD");
            const int scod = p[0];
            if (scod & 2) return F.set(OMR_INVALID_ARGUMENT, "j2k: SOP markers");
            if (scod & 4) return F.set(OMR_INVALID_ARGUMENT, "j2k: EPH markers");
            H.user_precincts = scod & 1;
            H.order = p[1];
            H.layers = (int32_t)be16(p + 2);
            H.mct = p[4] != 0;
            H.levels = p[5];
            H.xcb = p[6] + 2;
            H.ycb = p[7] + 2;
            if (H.order > 4 || H.layers < 1 || H.levels > 32 || p[4] > 1) return F.set(OMR_INTERNAL, "j2k: bad COD");
            if (p[6] > 8 || p[7] > 8 || H.xcb + H.ycb > 12) return F.set(OMR_INTERNAL, "j2k: bad code-block size");
            const int style = p[8];
            if (style & 1) return F.set(OMR_INVALID_ARGUMENT, "j2k: code-block style: selective arithmetic coding bypass");
            if (style & 2) return F.set(OMR_INVALID_ARGUMENT, "j2k: code-block style: reset of context probabilities");
            if (style & 4) return F.set(OMR_INVALID_ARGUMENT, "j2k: code-block style: termination on each coding pass");
            if (style & 8) return F.set(OMR_INVALID_ARGUMENT, "j2k: code-block style: vertically causal context");
            if (style & 16) return F.set(OMR_INVALID_ARGUMENT, "j2k: code-block style: predictable termination");
            if (style & 32) return F.set(OMR_INVALID_ARGUMENT, "j2k: code-block style: segmentation symbols");
            if (style & 0xC0) return F.set(OMR_INVALID_ARGUMENT, "j2k: code-block style of a later part of the standard");
            if (p[9] == 0 && !take97) return F.set(OMR_INVALID_ARGUMENT, "j2k: the irreversible 9/7 transform");
            if (p[9] > 1) return F.set(OMR_INVALID_ARGUMENT, take97 ? "j2k: a transform other than 5/3 and 9/7" : "j2k: a transform other than 5/3");
            H.lossy = p[9] == 0;
            if (n != (size_t)10 + (H.user_precincts ? (size_t)H.levels + 1 : 0)) return F.set(OMR_INTERNAL, "j2k: bad COD");
            for (int r = 0; r <= H.levels; ++r) H.pp[r] = H.user_precincts ? p[10 + r] : 0xFF;
            have_cod = true;
            break;
        }
        case 0x5C: {                                       // QCD
            if (in_tile) return F.set(OMR_INVALID_ARGUMENT, "j2k: QCD in a tile-part header");
            if (n < 1) return F.set(OMR_INTERNAL, "j2k: bad QCD");
            const int style = p[0] & 31;
            if (style == 1 && !take97) return F.set(OMR_INVALID_ARGUMENT, "j2k: scalar derived quantisation");
            if (style == 2 && !take97) return F.set(OMR_INVALID_ARGUMENT, "j2k: scalar expounded quantisation");
            if (style > 2 || (style == 0 && n - 1 > 97)) return F.set(OMR_INTERNAL, "j2k: bad QCD");
            H.guard = (uint8_t)(p[0] >> 5);
            H.qstyle = style;
            qcd = p + 1;
            qcd_n = n - 1;
            have_qcd = true;
            break;
        }
        case 0x53: return F.set(OMR_INVALID_ARGUMENT, "j2k: COC");
        case 0x5D: return F.set(OMR_INVALID_ARGUMENT, "j2k: QCC");
        case 0x5E: return F.set(OMR_INVALID_ARGUMENT, "j2k: RGN");
        case 0x5F: return F.set(OMR_INVALID_ARGUMENT, "j2k: POC");
        case 0x60: return F.set(OMR_INVALID_ARGUMENT, "j2k: PPM");
        case 0x61: return F.set(OMR_INVALID_ARGUMENT, "j2k: PPT");
        case 0x90: {                                       // SOT
            if (in_tile || n != 8) return F.set(OMR_INTERNAL, "j2k: bad SOT");
            if (!have_cod || !have_qcd) return F.set(OMR_INTERNAL, "j2k: COD or QCD missing");
            if (be16(p) != 0) return F.set(OMR_INVALID_ARGUMENT, "j2k: several tiles");
            if (p[6] != 0 || p[7] > 1) return F.set(OMR_INVALID_ARGUMENT, "j2k: several tile-parts");
            psot = be32(p + 2);
            sot_at = pos;
            in_tile = true;
            break;
        }
        default: break;                                    // COM, TLM, PLM, PLT, CRG and unknown segments with a length: skipped
        }
        pos += 2 + L;
    }
    H.body = pos;
    if (psot) {
        if (psot < pos - sot_at || psot > len - sot_at) return F.set(OMR_INTERNAL, "j2k: tile-part runs past the stream");
        H.body_end = sot_at + (size_t)psot;
    } else {
        if (len - pos < 2) return F.set(OMR_INTERNAL, "j2k: no EOC");
        H.body_end = len - 2;
    }
    // behind the tile-part: EOC; another SOT is a form out of scope
    if (len - H.body_end >= 2 && src[H.body_end] == 0xFF && src[H.body_end + 1] == 0x90)
        return F.set(OMR_INVALID_ARGUMENT, "j2k: several tiles or tile-parts");
    if (len - H.body_end < 2 || src[H.body_end] != 0xFF || src[H.body_end + 1] != 0xD9) return F.set(OMR_INTERNAL, "j2k: no EOC");
    if ((size_t)(3 * H.levels + 1) > 97) return F.set(OMR_INTERNAL, "j2k: bad COD");
    // the transform and the quantisation style come in pairs: 5/3 with none, 9/7 with a scalar one
    if (H.lossy && H.qstyle == 0) return F.set(OMR_INVALID_ARGUMENT, "j2k: the 9/7 transform without quantisation (QCD style 0)");
    if (!H.lossy && H.qstyle != 0) return F.set(OMR_INVALID_ARGUMENT, "j2k: the 5/3 transform with scalar quantisation (QCD style 1 or 2)");
    if (!H.lossy && !(kinds & kJ2kTakeReversible))
        return F.set(OMR_INVALID_ARGUMENT, "j2k: the reversible 5/3 transform (only irreversible streams are taken here)");
    std::memset(H.expo, 0xFF, sizeof H.expo);
    if (H.qstyle == 0) {
        for (size_t k = 0; k < qcd_n; ++k) H.expo[k] = (uint8_t)(qcd[k] >> 3);
    } else if (H.qstyle == 1) {                            // one pair; a subband n levels up has the exponent less n (OpenJPEG stops at 0)
        if (qcd_n != 2) return F.set(OMR_INTERNAL, "j2k: bad QCD");
        const int e0 = qcd[0] >> 3;
        for (int k = 0; k < 3 * H.levels + 1; ++k) {
            H.expo[k] = (uint8_t)std::max(e0 - (k ? (k - 1) / 3 : 0), 0);
            H.mant[k] = (uint16_t)(be16(qcd) & 0x7FFu);
        }
    } else {
        if ((qcd_n & 1) || qcd_n / 2 > 97) return F.set(OMR_INTERNAL, "j2k: bad QCD");
        for (size_t k = 0; k < qcd_n / 2; ++k) {
            H.expo[k] = (uint8_t)(qcd[2 * k] >> 3);
            H.mant[k] = (uint16_t)(be16(qcd + 2 * k) & 0x7FFu);
        }
    }
    for (int k = 0; k < 3 * H.levels + 1; ++k) {
        if (H.expo[k] == 0xFF) return F.set(OMR_INTERNAL, "j2k: QCD holds too few subbands");
        const int mb = (int)H.guard + (int)H.expo[k] - 1;
        if (mb > kJ2kMaxPlanes) return F.set(OMR_INVALID_ARGUMENT, "j2k: more than 30 magnitude bit-planes");
        if (mb < 0) return F.set(OMR_INTERNAL, "j2k: bad QCD");
    }
    return OMR_OK;
}

}  // namespace

omr_status j2k_prepare(const uint8_t* src, size_t len, int32_t w, int32_t h, int32_t samples, int32_t bits, J2kPlan& out,
                       std::string* why, uint32_t kinds) {
    Fail F{why};
    Header H;
    omr_status st = parse_headers(src, len, w, h, samples, bits, kinds, H, F);
    if (st) return st;
    uint64_t forms = 0;
    uint32_t lossy_forms = 0;
    if (H.mct && H.ncomp == 3 && !H.lossy) forms |= 1ull << OMR_J2K_FORM_RCT;
    if (H.bits == 16) forms |= 1ull << OMR_J2K_FORM_BITS16;
    const int NL = H.levels, NC = H.ncomp;
    if (H.lossy) {
        lossy_forms |= 1u << OMR_J2K_LOSSY_FORM_W97;
        lossy_forms |= 1u << (H.qstyle == 1 ? OMR_J2K_LOSSY_FORM_QCD_DERIVED : OMR_J2K_LOSSY_FORM_QCD_EXPOUNDED);
        if (NC == 3) lossy_forms |= 1u << (H.mct ? OMR_J2K_LOSSY_FORM_ICT : OMR_J2K_LOSSY_FORM_NO_MCT_3);
        if (H.bits == 16) lossy_forms |= 1u << OMR_J2K_LOSSY_FORM_BITS16;
        for (int r = 1; r <= NL; ++r) {
            const int32_t rw = j2k_ceil_shift(w, NL - r), rh = j2k_ceil_shift(h, NL - r);
            if (rw == 1 || rh == 1) lossy_forms |= 1u << OMR_J2K_LOSSY_FORM_LINE_OF_1;
            if (rw == 2 || rh == 2) lossy_forms |= 1u << OMR_J2K_LOSSY_FORM_LINE_OF_2;
        }
    }
    // K20: half the quantiser step of subband q of the QCD.  OpenJPEG adds no subband gain for 9/7
    // (the lifting's scaling makes up for it): delta = (1 + mantissa / 2048) * 2^(precision - exponent),
    // exact in double and in float (12 significant bits, an exponent in [-31, 17]).
    auto half_step = [&](int q) -> float {
        if (!H.lossy) return 0.f;
        const float delta = (float)std::ldexp(1.0 + (double)H.mant[q] / 2048.0, H.bits - (int)H.expo[q]);
        return 0.5f * delta;
    };
    // the geometry: resolutions, subbands, precincts, code-blocks
    std::vector<std::vector<Resolution>> comps((size_t)NC);
    std::vector<J2kBlock> blocks;
    uint64_t n_prec = 0;
    for (int c = 0; c < NC; ++c) {
        comps[(size_t)c].resize((size_t)NL + 1);
        for (int r = 0; r <= NL; ++r) {
            Resolution& R = comps[(size_t)c][(size_t)r];
            R.w = (uint32_t)j2k_ceil_shift(w, NL - r);
            R.h = (uint32_t)j2k_ceil_shift(h, NL - r);
            R.ppx = H.pp[r] & 15;
            R.ppy = H.pp[r] >> 4;
            if (r > 0 && (R.ppx == 0 || R.ppy == 0)) return F.set(OMR_INTERNAL, "j2k: bad precinct size");
            R.pw = (uint32_t)(((uint64_t)R.w + (1ull << R.ppx) - 1) >> R.ppx);
            R.ph = (uint32_t)(((uint64_t)R.h + (1ull << R.ppy) - 1) >> R.ppy);
            n_prec += (uint64_t)R.pw * R.ph;
            if (n_prec > kMaxPrecincts) return F.set(OMR_INVALID_ARGUMENT, "j2k: too many precincts");
            const uint32_t lw = (R.w + 1) / 2, lh = (R.h + 1) / 2;
            if (r == 0) {
                R.nb = 1;
                R.band[0] = {0u, R.w, R.h, 0u, 0u, (int32_t)H.guard + H.expo[0] - 1, half_step(0)};
            } else {
                R.nb = 3;
                const int q = 3 * (r - 1) + 1;
                R.band[0] = {1u, R.w / 2, lh, lw, 0u, (int32_t)H.guard + H.expo[q] - 1, half_step(q)};
                R.band[1] = {2u, lw, R.h / 2, 0u, lh, (int32_t)H.guard + H.expo[q + 1] - 1, half_step(q + 1)};
                R.band[2] = {3u, R.w / 2, R.h / 2, lw, lh, (int32_t)H.guard + H.expo[q + 2] - 1, half_step(q + 2)};
            }
            const uint32_t cpx = r ? R.ppx - 1 : R.ppx, cpy = r ? R.ppy - 1 : R.ppy;
            const uint32_t bx = std::min<uint32_t>((uint32_t)H.xcb, cpx), by = std::min<uint32_t>((uint32_t)H.ycb, cpy);
            R.prec.resize((size_t)R.pw * R.ph);
            for (int b = 0; b < R.nb; ++b) {
                const BandGeom& G = R.band[b];
                for (uint32_t py = 0; py < R.ph; ++py)
                    for (uint32_t px = 0; px < R.pw; ++px) {
                        PrecinctBand& P = R.prec[(size_t)py * R.pw + px].b[b];
                        const uint64_t x0 = (uint64_t)px << cpx, x1 = std::min<uint64_t>(((uint64_t)px + 1) << cpx, G.w);
                        const uint64_t y0 = (uint64_t)py << cpy, y1 = std::min<uint64_t>(((uint64_t)py + 1) << cpy, G.h);
                        if (x0 >= x1 || y0 >= y1) continue;
                        const uint64_t cx0 = x0 >> bx, cy0 = y0 >> by;
                        P.ncw = (uint32_t)(((x1 - 1) >> bx) - cx0 + 1);
                        P.nch = (uint32_t)(((y1 - 1) >> by) - cy0 + 1);
                        if ((uint64_t)blocks.size() + (uint64_t)P.ncw * P.nch > kMaxBlocks)
                            return F.set(OMR_INVALID_ARGUMENT, "j2k: too many code-blocks");
                        P.first = (uint32_t)blocks.size();
                        P.incl.make(P.ncw, P.nch);
                        P.imsb.make(P.ncw, P.nch);
                        if ((uint64_t)P.ncw * P.nch > 1) forms |= 1ull << OMR_J2K_FORM_TAG_TREE_DEEP;
                        for (uint32_t j = 0; j < P.nch; ++j)
                            for (uint32_t i = 0; i < P.ncw; ++i) {
                                const uint64_t ax0 = std::max<uint64_t>(x0, (cx0 + i) << bx), ax1 = std::min<uint64_t>(x1, (cx0 + i + 1) << bx);
                                const uint64_t ay0 = std::max<uint64_t>(y0, (cy0 + j) << by), ay1 = std::min<uint64_t>(y1, (cy0 + j + 1) << by);
                                J2kBlock K{};
                                K.ws_off = (uint32_t)((uint64_t)c * (uint64_t)w * (uint64_t)h + (G.oy + ay0) * (uint64_t)w + G.ox + ax0);
                                K.stride = (uint32_t)w;
                                K.w = (uint16_t)(ax1 - ax0);
                                K.h = (uint16_t)(ay1 - ay0);
                                K.orient = (uint8_t)G.orient;
                                K.step = G.step;
                                if (K.w != (1u << bx) || K.h != (1u << by)) forms |= 1ull << OMR_J2K_FORM_PARTIAL_BLOCK;
                                blocks.push_back(K);
                            }
                    }
            }
        }
    }
    // tier 2: the packets in progression order
    std::vector<BlockState> state(blocks.size());
    std::vector<Piece> pieces;
    struct Visit {
        uint64_t y, x;
        int32_t c, r;
        uint32_t p;
    };
    std::vector<Visit> visits;
    for (int c = 0; c < NC; ++c)
        for (int r = 0; r <= NL; ++r) {
            const Resolution& R = comps[(size_t)c][(size_t)r];
            for (uint32_t p = 0; p < R.pw * R.ph; ++p)
                visits.push_back({(uint64_t)(p / R.pw) << (R.ppy + (uint32_t)(NL - r)), (uint64_t)(p % R.pw) << (R.ppx + (uint32_t)(NL - r)), c, r, p});
        }
    // the order of (component, resolution, precinct) inside one layer; `outer` says where the layer loop sits
    auto key = [&](const Visit& v, int k) -> uint64_t {
        switch (H.order) {
        case 0: case 1: { const uint64_t f[3] = {(uint64_t)v.r, (uint64_t)v.c, v.p}; return f[k]; }                      // LRCP, RLCP
        case 2: { const uint64_t f[5] = {(uint64_t)v.r, v.y, v.x, (uint64_t)v.c, v.p}; return k < 5 ? f[k] : 0; }        // RPCL
        case 3: { const uint64_t f[5] = {v.y, v.x, (uint64_t)v.c, (uint64_t)v.r, v.p}; return k < 5 ? f[k] : 0; }        // PCRL
        default: { const uint64_t f[5] = {(uint64_t)v.c, v.y, v.x, (uint64_t)v.r, v.p}; return k < 5 ? f[k] : 0; }       // CPRL
        }
    };
    const int nkeys = H.order <= 1 ? 3 : 5;
    std::stable_sort(visits.begin(), visits.end(), [&](const Visit& a, const Visit& b) {
        for (int k = 0; k < nkeys; ++k) {
            const uint64_t ka = key(a, k), kb = key(b, k);
            if (ka != kb) return ka < kb;
        }
        return false;
    });
    HeaderBits B{src, H.body, H.body_end};
    std::vector<std::pair<uint32_t, uint32_t>> pending;
    auto packet = [&](const Visit& v, int32_t layer) -> omr_status {
        Resolution& R = comps[(size_t)v.c][(size_t)v.r];
        Precinct& P = R.prec[v.p];
        B.buf = 0;
        B.ct = 0;
        pending.clear();
        if (!B.bit()) {
            if (B.bad) return F.set(OMR_INTERNAL, "j2k: stream cut inside a packet header");
            B.align();                                     // an empty packet (OpenJPEG writes none: it has no form bit)
            return OMR_OK;
        }
        for (int b = 0; b < R.nb; ++b) {
            PrecinctBand& Q = P.b[b];
            const int32_t mb = R.band[b].mb;
            for (uint32_t k = 0; k < Q.ncw * Q.nch; ++k) {
                BlockState& S = state[Q.first + k];
                const bool in = S.included ? B.bit() != 0 : tag_decode(Q.incl, B, k, (uint32_t)layer + 1u);
                if (B.bad) return F.set(OMR_INTERNAL, "j2k: stream cut inside a packet header");
                if (!in) continue;
                if (!S.included) {
                    uint32_t i = 1;
                    while (!tag_decode(Q.imsb, B, k, i)) {
                        if (B.bad) return F.set(OMR_INTERNAL, "j2k: stream cut inside a packet header");
                        if (++i > (uint32_t)mb + 1u) return F.set(OMR_INTERNAL, "j2k: more zero bit-planes than the subband has");
                    }
                    S.included = true;
                    S.planes = mb - (int32_t)(i - 1u);
                    if (i > 1u) forms |= 1ull << OMR_J2K_FORM_ZERO_BIT_PLANES;
                    if (layer > 0) forms |= 1ull << OMR_J2K_FORM_LATE_INCLUSION;
                }
                uint32_t n;
                if (!B.bit()) { n = 1; forms |= 1ull << OMR_J2K_FORM_PASSES_1; }
                else if (!B.bit()) { n = 2; forms |= 1ull << OMR_J2K_FORM_PASSES_2; }
                else if ((n = B.bits(2)) != 3) { n += 3; forms |= 1ull << OMR_J2K_FORM_PASSES_3_5; }
                else if ((n = B.bits(5)) != 31) { n += 6; forms |= 1ull << OMR_J2K_FORM_PASSES_6_36; }
                else { n = 37 + B.bits(7); forms |= 1ull << OMR_J2K_FORM_PASSES_37_164; }
                uint32_t inc = 0;
                while (B.bit()) {
                    if (++inc > 32u) return F.set(OMR_INTERNAL, "j2k: bad Lblock");
                }
                if (inc) forms |= 1ull << OMR_J2K_FORM_LBLOCK;
                S.lenbits = (uint8_t)(S.lenbits + inc);
                int lg = 0;
                while ((n >> (lg + 1)) != 0) ++lg;
                if (S.lenbits + lg > 32) return F.set(OMR_INTERNAL, "j2k: bad Lblock");
                const uint32_t seg_len = B.bits(S.lenbits + lg);
                if (B.bad) return F.set(OMR_INTERNAL, "j2k: stream cut inside a packet header");
                S.passes += n;
                if ((int64_t)S.passes > 3 * (int64_t)S.planes - 2) return F.set(OMR_INTERNAL, "j2k: more coding passes than the bit-planes hold");
                pending.push_back({Q.first + k, seg_len});
            }
        }
        B.align();
        if (B.bad) return F.set(OMR_INTERNAL, "j2k: stream cut inside a packet header");
        for (const auto& pe : pending) {
            if (pe.second > B.end - B.pos) return F.set(OMR_INTERNAL, "j2k: packet body runs past the tile-part");
            if (pe.second) pieces.push_back({pe.first, (uint32_t)B.pos, pe.second});
            B.pos += pe.second;
        }
        return OMR_OK;
    };
    if (H.order == 0) {                                    // LRCP: the layer loop outside
        for (int32_t l = 0; l < H.layers; ++l)
            for (const Visit& v : visits)
                if ((st = packet(v, l))) return st;
    } else if (H.order == 1) {                             // RLCP: inside the resolution loop
        size_t i = 0;
        while (i < visits.size()) {
            size_t j = i;
            while (j < visits.size() && visits[j].r == visits[i].r) ++j;
            for (int32_t l = 0; l < H.layers; ++l)
                for (size_t k = i; k < j; ++k)
                    if ((st = packet(visits[k], l))) return st;
            i = j;
        }
    } else {                                               // RPCL, PCRL, CPRL: innermost
        for (const Visit& v : visits)
            for (int32_t l = 0; l < H.layers; ++l)
                if ((st = packet(v, l))) return st;
    }
    if (B.ff) forms |= 1ull << OMR_J2K_FORM_FF_HEADER;
    // the blocks with their ranges, layer after layer
    if (len > 0xFFFFFFFFull) return F.set(OMR_INVALID_ARGUMENT, "j2k: stream of 4 GiB or more");
    std::vector<uint32_t> count(blocks.size() + 1, 0);
    for (const Piece& p : pieces) ++count[p.block + 1];
    for (size_t k = 0; k < blocks.size(); ++k) count[k + 1] += count[k];
    out.ranges.assign(pieces.size(), J2kRange{0, 0});
    for (size_t k = 0; k < blocks.size(); ++k) {
        blocks[k].range0 = count[k];
        blocks[k].n_ranges = count[k + 1] - count[k];
        blocks[k].passes = (uint16_t)state[k].passes;
        blocks[k].planes = (uint8_t)std::max(state[k].planes, 0);
        if (H.lossy && state[k].passes && (int64_t)state[k].passes < 3 * (int64_t)state[k].planes - 2)
            lossy_forms |= 1u << OMR_J2K_LOSSY_FORM_TRUNCATED_BLOCK;
    }
    std::vector<uint32_t> at(count.begin(), count.end() - 1);
    for (const Piece& p : pieces) out.ranges[at[p.block]++] = {p.off, p.len};
    out.w = w; out.h = h; out.ncomp = NC; out.bits = H.bits; out.levels = NL; out.mct = H.mct && NC == 3;
    out.lossy = H.lossy;
    out.lossy_forms = lossy_forms;
    out.blocks = std::move(blocks);
    out.forms = forms;
    return OMR_OK;
}

namespace {

// The blocks into the coefficient area a (ncomp planes of w x h), then level by level into x and
// y, then the pixels: what K19a, K19b and K19c do, by the same functions.
void store_sample(uint8_t* dst, int32_t bits, size_t at, uint32_t v) {
    if (bits == 8) dst[at] = (uint8_t)v;
    else reinterpret_cast<uint16_t*>(dst)[at] = (uint16_t)v;
}

// K20: the float half of decode below: a holds the coefficients' bits.  Level by level, all rows
// and then all columns (OpenJPEG's order; in float the order decides the bits), each line by
// j2k_lift97_line, then the pixels by j2k_pixel97: what K20b and K19c compute.
void finish97(const J2kPlan& P, const std::vector<int32_t>& a, int32_t w, int32_t h, int32_t bits, uint8_t* dst) {
    const size_t plane = (size_t)w * h;
    const int32_t L = P.levels, NC = P.ncomp;
    const float* af = reinterpret_cast<const float*>(a.data());
    std::vector<float> prev, cur;                          // NC planes of the level before and of this one, rows pw and rw apart
    int32_t pw = 0, ph = 0;
    for (int32_t l = 1; l <= L; ++l) {
        const int32_t rw = j2k_ceil_shift(w, L - l), rh = j2k_ceil_shift(h, L - l), lw = (rw + 1) / 2, lh = (rh + 1) / 2;
        cur.assign((size_t)rw * rh * NC, 0.f);
        const bool threaded = (size_t)rw * rh >= kThreadedCoefficients;
        for (int32_t c = 0; c < NC; ++c) {
            const float* ap = af + plane * (size_t)c;
            const float* lp = l == 1 ? ap : prev.data() + (size_t)pw * ph * c;
            const int32_t lstride = l == 1 ? w : pw;
            float* op = cur.data() + (size_t)rw * rh * c;
            parallel_for(rh, threaded, [&](int r) {        // nested row r is interleaved row y
                float* line = op + (size_t)(r < lh ? 2 * r : 2 * (r - lh) + 1) * rw;
                for (int32_t j = 0; j < rw; ++j)
                    line[j < lw ? 2 * j : 2 * (j - lw) + 1] = j < lw && r < lh ? lp[(size_t)r * lstride + j] : ap[(size_t)r * w + j];
                j2k_lift97_line(line, rw, 1);
            });
            parallel_for(rw, threaded, [&](int x) { j2k_lift97_line(op + x, rh, (size_t)rw); });
        }
        prev.swap(cur);
        pw = rw;
        ph = rh;
    }
    for (size_t p = 0; p < plane; ++p) {
        float v[3] = {0.f, 0.f, 0.f};
        uint32_t o[3];
        for (int32_t c = 0; c < NC; ++c) v[c] = L ? prev[plane * (size_t)c + p] : af[plane * (size_t)c + p];
        j2k_pixel97(v, NC, P.mct, bits, o);
        for (int32_t c = 0; c < NC; ++c) store_sample(dst, bits, p * (size_t)NC + c, o[c]);
    }
}

omr_status decode(const uint8_t* src, size_t len, int32_t w, int32_t h, int32_t samples, int32_t bits, uint8_t* dst,
                  uint64_t* forms, std::string* why, uint32_t kinds = kJ2kTakeReversible, uint32_t* lossy_forms = nullptr) {
    std::unique_ptr<J2kPlan> P(new J2kPlan);
    const omr_status st = j2k_prepare(src, len, w, h, samples, bits, *P, why, kinds);
    if (st) return st;
    if (lossy_forms) *lossy_forms = P->lossy_forms;
    const size_t plane = (size_t)w * h, total = plane * (size_t)P->ncomp;
    std::vector<int32_t> a(total);
    std::atomic<uint64_t> met{P->forms};
    const int nb = (int)P->blocks.size();
    const int chunk = 8, jobs = (nb + chunk - 1) / chunk;
    parallel_for(jobs, total >= kThreadedCoefficients && jobs > 1, [&](int job) {
        std::vector<uint32_t> mag(kJ2kMaxBlockArea);
        std::vector<uint8_t> fl(kJ2kMaxFlagBytes);
        uint8_t cx[kJ2kContexts];
        uint64_t f = 0;
        for (int k = job * chunk; k < std::min(nb, (job + 1) * chunk); ++k) {
            const J2kBlock& K = P->blocks[(size_t)k];
            const size_t area = (size_t)K.w * K.h, fbytes = (size_t)(K.w + 2) * (K.h + 2);
            std::memset(mag.data(), 0, 4 * area);
            std::memset(fl.data(), 0, fbytes);
            f |= forms ? j2k_t1_decode<true>(src, P->ranges.data(), K, mag.data(), fl.data(), cx)
                       : j2k_t1_decode<false>(src, P->ranges.data(), K, mag.data(), fl.data(), cx);
            for (uint32_t y = 0; y < K.h; ++y)
                for (uint32_t x = 0; x < K.w; ++x)
                    a[(size_t)K.ws_off + (size_t)y * K.stride + x] =
                        P->lossy ? (int32_t)j2k_float_bits(j2k_dequantise(mag[(size_t)y * K.w + x], fl[(size_t)(y + 1) * (K.w + 2) + x + 1], K.step))
                                 : j2k_coefficient(mag[(size_t)y * K.w + x], fl[(size_t)(y + 1) * (K.w + 2) + x + 1]);
        }
        met.fetch_or(f);
    });
    if (forms) *forms = met.load();
    if (!dst) return OMR_OK;
    if (P->lossy) {
        finish97(*P, a, w, h, bits, dst);
        return OMR_OK;
    }
    const int32_t L = P->levels, yw = (w + 1) / 2, yh = (h + 1) / 2;
    std::vector<int32_t> xb(L ? total : 0), yb(L > 1 ? (size_t)yw * yh * P->ncomp : 0);
    for (int32_t l = 1; l <= L; ++l) {
        const int32_t rw = j2k_ceil_shift(w, L - l), rh = j2k_ceil_shift(h, L - l), lw = (rw + 1) / 2, lh = (rh + 1) / 2;
        const bool to_x = j2k_level_writes_x(L, l);
        for (int32_t c = 0; c < P->ncomp; ++c) {
            const int32_t* ap = a.data() + plane * (size_t)c;
            const int32_t* lp = l == 1 ? ap : to_x ? yb.data() + (size_t)yw * yh * c : xb.data() + plane * (size_t)c;
            const int32_t lstride = l == 1 || !to_x ? w : yw;
            int32_t* op = to_x ? xb.data() + plane * (size_t)c : yb.data() + (size_t)yw * yh * c;
            const int32_t ostride = to_x ? w : yw;
            parallel_for(rh, (size_t)rw * rh >= kThreadedCoefficients, [&](int y) {
                for (int32_t x = 0; x < rw; ++x)
                    op[(size_t)y * ostride + x] = j2k_idwt53_at(rw, rh, x, y, [&](int32_t col, int32_t row) {
                        return col < lw && row < lh ? lp[(size_t)row * lstride + col] : ap[(size_t)row * w + col];
                    });
            });
        }
    }
    const int32_t* img = L ? xb.data() : a.data();
    for (size_t p = 0; p < plane; ++p) {
        int32_t v[3] = {0, 0, 0};
        uint32_t o[3];
        for (int32_t c = 0; c < P->ncomp; ++c) v[c] = img[plane * (size_t)c + p];
        j2k_pixel(v, P->ncomp, P->mct, bits, o);
        for (int32_t c = 0; c < P->ncomp; ++c) {
            if (bits == 8) dst[p * (size_t)P->ncomp + c] = (uint8_t)o[c];
            else reinterpret_cast<uint16_t*>(dst)[p * (size_t)P->ncomp + c] = (uint16_t)o[c];
        }
    }
    return OMR_OK;
}

bool sizes_ok(int32_t w, int32_t h, int32_t samples, int32_t bits) {
    return w >= 1 && h >= 1 && (samples == 1 || samples == 3) && (bits == 8 || bits == 16) &&
           (uint64_t)w * (uint64_t)h * (uint64_t)samples * (uint64_t)(bits / 8) <= kMaxDecoded;
}

}  // namespace

bool j2k_sizes_ok(int32_t w, int32_t h, int32_t samples, int32_t bits) { return sizes_ok(w, h, samples, bits); }

omr_status j2k_decode_host_kinds(const uint8_t* src, size_t len, int32_t w, int32_t h, int32_t samples, int32_t bits, uint8_t* dst,
                                 uint32_t kinds, std::string* why) {
    if (!src || !dst || !sizes_ok(w, h, samples, bits)) return OMR_INVALID_ARGUMENT;
    if (bits == 16 && (reinterpret_cast<uintptr_t>(dst) & 1u)) return OMR_INVALID_ARGUMENT;
    return decode(src, len, w, h, samples, bits, dst, nullptr, why, kinds);
}

}  // namespace omr

using namespace omr;

extern "C" {

omr_status omr_j2k_decode_host(const uint8_t* src, size_t length, int32_t width, int32_t height, int32_t samples, int32_t bits,
                               uint8_t* dst, char* why, size_t why_cap) {
    return omr_j2k_decode_host_ex(src, length, width, height, samples, bits, 0u, dst, why, why_cap);
}

omr_status omr_j2k_decode_host_ex(const uint8_t* src, size_t length, int32_t width, int32_t height, int32_t samples, int32_t bits,
                                  uint32_t flags, uint8_t* dst, char* why, size_t why_cap) {
    if (why && why_cap) why[0] = 0;
    if (flags & ~OMR_J2K_ALLOW_IRREVERSIBLE) return OMR_INVALID_ARGUMENT;
    std::string msg;
    const omr_status st = j2k_decode_host_kinds(src, length, width, height, samples, bits, dst,
                                                kJ2kTakeReversible | (flags ? kJ2kTakeIrreversible : 0u), &msg);
    if (why && why_cap) {
        std::strncpy(why, msg.c_str(), why_cap - 1);
        why[why_cap - 1] = 0;
    }
    return st;
}

omr_status omr_j2k_stream_forms(const uint8_t* src, size_t length, uint64_t* forms) {
    return omr_j2k_stream_forms_ex(src, length, 0u, forms, nullptr);
}

omr_status omr_j2k_stream_forms_ex(const uint8_t* src, size_t length, uint32_t flags, uint64_t* forms, uint32_t* lossy_forms) {
    if (!src || !forms || (flags & ~OMR_J2K_ALLOW_IRREVERSIBLE)) return OMR_INVALID_ARGUMENT;
    *forms = 0;
    if (lossy_forms) *lossy_forms = 0;
    // the frame's own size, component count and precision: SIZ stands behind SOC
    if (length < 2 + 4 + 36 + 3 || src[0] != 0xFF || src[1] != 0x4F || src[2] != 0xFF || src[3] != 0x51) return OMR_INTERNAL;
    const uint8_t* p = src + 6;
    const uint64_t w = be32(p + 2), h = be32(p + 6);
    const size_t nc = be16(p + 34);
    const int bits = (p[36] & 0x7F) + 1;
    if (w > 0x7FFFFFFFull || h > 0x7FFFFFFFull || !sizes_ok((int32_t)w, (int32_t)h, (int32_t)nc, bits)) return OMR_INVALID_ARGUMENT;
    return decode(src, length, (int32_t)w, (int32_t)h, (int32_t)nc, bits, nullptr, forms, nullptr,
                  kJ2kTakeReversible | (flags ? kJ2kTakeIrreversible : 0u), lossy_forms);
}

}  // extern "C"
