// omr_segread.h — the device-read pipeline that the TIFF and the Zarr reader share (K13 .. K19).
//
// Both readers answer a batch of regions the same way: the segments (tiles, strips, chunks) the
// regions touch are listed once each, their bytes go to pinned memory and in one copy to the device
// with a stream table, a decoder kernel decodes them into scratch and a place kernel cuts the
// regions out.  What is the same lives here: the staging of one context (SegPipe), the planner that
// turns regions into placements and unique segments (pure host code, checked without a GPU by
// tools/segread_plan_check.cpp), the layout of the stream table, and -- in omr_segread.cpp, the
// only part that calls HIP -- the group loop, the run stage and the tile renderer.  A front-end
// (omr_tiffread.cpp, omr_zarr.cpp) supplies a SegSource: where a segment's size comes from and how
// its bytes are read.
#pragma once

#include <atomic>
#include <functional>
#include <thread>
#include <unordered_map>

#include "omr_internal.h"

namespace omr {

constexpr size_t kGroupInBytes = (size_t)128 << 20;        // compressed bytes per group
constexpr size_t kGroupScratchBytes = (size_t)512 << 20;   // decoded bytes per group
constexpr size_t kRenderGroupBytes = (size_t)256 << 20;    // region bytes per render group

// ---- staging of one context ---------------------------------------------------------------------

struct SegPipe {
    void* pin = nullptr;         // segment bytes + tables (+ the statuses coming back)
    void* d_in = nullptr;
    size_t in_cap = 0;
    void* d_scratch = nullptr;   // decoded segments
    size_t scratch_cap = 0;
    void* d_regions = nullptr;   // render_tiles: [tile][channel][h][w]
    size_t regions_cap = 0;
    void* d_out = nullptr;       // and its ARGB when the caller's output is host memory
    size_t out_cap = 0;
    void* pin_tab = nullptr;     // Blosc: the stream table and the placements, sized after the files are read
    void* d_tab = nullptr;
    size_t tab_cap = 0;
    void* d_lit = nullptr;       // K16a: one literal buffer per workgroup of its grid
    size_t lit_cap = 0;
    void* d_coef = nullptr;      // K17: the JPEG segments' coefficients (int16) and sample planes; K19: the JPEG 2000 segments' planes
    size_t coef_cap = 0;
    ~SegPipe();
};

// A context keeps two, one per reader (Ctx::tiff_state, Ctx::zarr_state); made on first use.
enum class SegKind { tiff, zarr };
SegPipe* seg_pipe(Ctx* c, SegKind kind);

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

// ---- the planner: regions -> placements and unique segments (no HIP) ------------------------------

// One level: segments of seg_w x seg_h samples (a strip: seg_w = the level's width), `across` per
// segment row, samples of bpp bytes.  Segments are stored whole but for the rows of a last strip,
// which no region inside the level reaches.  spp: samples per pixel of a chunky TIFF segment
// (seg_w counts pixels; a segment row is seg_w * spp samples); a region takes one of them.
struct SegGeom {
    int32_t seg_w = 0, seg_h = 0, across = 0, down = 0, bpp = 0, spp = 1;
};
struct SegKey {
    int64_t plane;
    int32_t sx, sy;
};
struct SegPlan {
    std::vector<TiffPlace> places;     // src still null
    std::vector<int32_t> place_seg;    // places[k] reads segs[place_seg[k]]
    std::vector<SegKey> segs;          // every segment touched, once, in first-touch order
    int32_t max_rows = 0;              // of the tallest placement
};

// The regions reqs[r0, r1) of width x height samples (inside the level), region i to
// dst + i * stride bytes with rows `width` samples apart; plane_of(request) numbers the planes (the
// IFDs of a TIFF: the channels of one chunky pixel share a plane, and so its segments) and
// sample_of(request) in [0, g.spp) picks the request's sample out of each pixel.
template <typename PlaneOf, typename SampleOf>
SegPlan plan_regions(const SegGeom& g, const omr_raw_tile_request* reqs, int32_t r0, int32_t r1, int32_t width,
                     int32_t height, uint8_t* dst, int64_t stride, const PlaneOf& plane_of, const SampleOf& sample_of) {
    SegPlan P;
    if (width <= 0 || height <= 0) return P;
    std::unordered_map<uint64_t, int32_t> index;      // plane * segments + k -> unique segment
    const uint64_t per_plane = (uint64_t)g.across * g.down;
    for (int32_t i = r0; i < r1; ++i) {
        const omr_raw_tile_request& r = reqs[i];
        const int64_t plane = plane_of(r);
        const int32_t sample = (int32_t)sample_of(r);
        for (int32_t sy = r.y / g.seg_h; sy <= (r.y + height - 1) / g.seg_h; ++sy)
            for (int32_t sx = r.x / g.seg_w; sx <= (r.x + width - 1) / g.seg_w; ++sx) {
                const uint64_t key = (uint64_t)plane * per_plane + (uint64_t)sy * g.across + sx;
                auto it = index.find(key);
                if (it == index.end()) {
                    it = index.emplace(key, (int32_t)P.segs.size()).first;
                    P.segs.push_back({plane, sx, sy});
                }
                const int32_t ox = sx * g.seg_w, oy = sy * g.seg_h;
                const int32_t X0 = std::max(r.x, ox), X1 = std::min(r.x + width, ox + g.seg_w);
                const int32_t Y0 = std::max(r.y, oy), Y1 = std::min(r.y + height, oy + g.seg_h);
                TiffPlace p;
                p.src = nullptr;
                p.dst = dst + (int64_t)i * stride + ((int64_t)(Y0 - r.y) * width + (X0 - r.x)) * g.bpp;
                p.seg_w = g.seg_w;
                p.dst_pitch = width;
                p.x0 = X0 - ox; p.x1 = X1 - ox; p.y0 = Y0 - oy; p.y1 = Y1 - oy;
                p.spp = g.spp;
                p.sample = sample;
                P.max_rows = std::max(P.max_rows, Y1 - Y0);
                P.places.push_back(p);
                P.place_seg.push_back(it->second);
            }
    }
    return P;
}
// One sample per pixel.
template <typename PlaneOf>
SegPlan plan_regions(const SegGeom& g, const omr_raw_tile_request* reqs, int32_t r0, int32_t r1, int32_t width,
                     int32_t height, uint8_t* dst, int64_t stride, const PlaneOf& plane_of) {
    return plan_regions(g, reqs, r0, r1, width, height, dst, stride, plane_of, [](const omr_raw_tile_request&) { return 0; });
}

// Requests per group: as many of the n as fit the budget at per_req bytes each, and at least one.
inline int32_t group_size(int32_t n, size_t budget, size_t per_req) {
    return (int32_t)std::max<size_t>(1, std::min<size_t>((size_t)std::max(n, 0), budget / per_req));
}
// The staging a read request can need: its segments counted whole and without sharing.
inline size_t read_bytes_per_request(const SegGeom& g, int32_t width, int32_t height) {
    const size_t seg_dec = (((size_t)g.seg_w * g.seg_h * g.bpp * g.spp) + 15) / 16 * 16;
    return (size_t)((width - 1) / g.seg_w + 2) * (size_t)((height - 1) / g.seg_h + 2) * seg_dec;
}

// ---- the stream table ---------------------------------------------------------------------------

// [bytes][offsets u64 m][dst offsets u64 m][lengths u32 m][expected u32 m][raw u8 m][places] | [status i32 m]:
// everything before the bar goes up in one copy of up_bytes, the statuses come back.  in_bytes = 0:
// a table in a buffer of its own (Blosc); without has_raw the raw column is empty.
struct TableLayout {
    size_t m, o_off, o_dst, o_len, o_exp, o_raw, o_place, o_status, up_bytes, total;
    TableLayout(size_t in_bytes, size_t m_, size_t place_bytes, bool has_raw) : m(m_) {
        o_off = (in_bytes + 255) / 256 * 256;
        o_dst = o_off + 8 * m;
        o_len = o_dst + 8 * m;
        o_exp = o_len + 4 * m;
        o_raw = o_exp + 4 * m;
        o_place = (o_raw + (has_raw ? m : 0) + 15) / 16 * 16;
        up_bytes = o_place + place_bytes;
        o_status = (up_bytes + 255) / 256 * 256;
        total = o_status + 4 * m;
    }
    uint64_t* off(uint8_t* base) const { return reinterpret_cast<uint64_t*>(base + o_off); }
    uint64_t* dst(uint8_t* base) const { return reinterpret_cast<uint64_t*>(base + o_dst); }
    uint32_t* len(uint8_t* base) const { return reinterpret_cast<uint32_t*>(base + o_len); }
    uint32_t* exp(uint8_t* base) const { return reinterpret_cast<uint32_t*>(base + o_exp); }
    uint8_t* raw(uint8_t* base) const { return base + o_raw; }
    int32_t* status(uint8_t* base) const { return reinterpret_cast<int32_t*>(base + o_status); }
    // Rows [first, first + n) of the table at d_tab as a decoder's argument (raw column only where has_raw).
    StreamTable rows(const uint8_t* d_src, uint8_t* d_tab, size_t first, size_t n, uint8_t* d_dst, bool has_raw) const {
        return {d_src, off(d_tab) + first, len(d_tab) + first, exp(d_tab) + first, has_raw ? raw(d_tab) + first : nullptr,
                (int32_t)n, d_dst, dst(d_tab) + first, status(d_tab) + first};
    }
};

// ---- what a front-end supplies ------------------------------------------------------------------

enum class SegCodec { none, lzw, zlib, zstd, blosc, jpeg, j2k };

// What a read request of an image-codec level can need beside read_bytes_per_request: the decoder's
// workspace for the same segments, so that a group's workspace stays within kGroupScratchBytes as its
// decoded bytes do.  JPEG: K17's coefficients and sample planes.  JPEG 2000: K19's workspace of 4
// bytes per coefficient, three times -- the subbands as K19a leaves them and the two planes K19b's
// levels alternate between, the second of a quarter of the size (J2kSegDesc, omr_j2kdec.h).  Any
// other codec: nothing.
inline size_t codec_workspace_per_request(SegCodec codec, const SegGeom& g, int32_t width, int32_t height) {
    const size_t w = (size_t)g.seg_w, h = (size_t)g.seg_h;
    size_t per_seg = 0;
    if (codec == SegCodec::jpeg) per_seg = (size_t)3 * g.spp * ((w + 15) / 16 * 16) * ((h + 15) / 16 * 16) + 512;
    if (codec == SegCodec::j2k) per_seg = (size_t)4 * g.spp * (2 * w * h + ((w + 1) / 2) * ((h + 1) / 2)) + 768;
    return (size_t)((width - 1) / g.seg_w + 2) * (size_t)((height - 1) / g.seg_h + 2) * per_seg;
}

// One unique segment of a group: cnt bytes to read (0: the segment reads as zeros) that hold, or
// decode to, `expected` bytes.  The pipeline sets the two offsets.
struct SegBytes {
    uint64_t cnt = 0;
    uint32_t expected = 0;
    uint64_t in_off = 0, scratch_off = 0;
};

// One level of an open image, for the time of a call.
struct SegSource {
    SegKind kind;
    const char* tag;             // "tiff" | "zarr", and "segment" | "chunk": the words of the messages
    const char* noun;
    SegGeom geom;
    SegCodec codec = SegCodec::none;
    int32_t predictor = 1;       // of K13b
    bool swap = false;           // the file's byte order is not the host's (it matters to predictor 2 only)
    uint32_t blosc_inner = 0;    // SegCodec::blosc: the OMR_BLOSC_INNER_* formats the open allowed
    int32_t pt = 0;              // render_tiles: the image's pixel type and byte order
    bool big = false;
    virtual ~SegSource() = default;
    virtual int64_t plane_of(const omr_raw_tile_request& r) const = 0;
    virtual int32_t sample_of(const omr_raw_tile_request&) const { return 0; }   // in [0, geom.spp)
    // cnt and expected of every segment of the group (a failure sets the context's message itself).
    virtual omr_status sizes(Ctx* ctx, const std::vector<SegKey>& keys, std::vector<SegBytes>& out) = 0;
    // cnt bytes of every segment to pin + in_off; in_bytes: their sum.  false: an I/O error.
    virtual bool read(const std::vector<SegKey>& keys, const std::vector<SegBytes>& segs, uint8_t* pin, size_t in_bytes) = 0;
    // SegCodec::jpeg: the JPEGTables stream of a segment's IFD (*len = 0: none) and whether the
    // three components are YCbCr (Photometric 6).
    virtual const uint8_t* jpeg_tables(const SegKey&, size_t* len) const { *len = 0; return nullptr; }
    bool jpeg_ycc = false;
    uint32_t j2k_kinds = 1u;     // SegCodec::j2k: the kJ2kTake* transforms the open allowed (omr_j2kdec.h)
};

// ---- K17, K19: one group of image-codec segments (omr_jpegdec.hip, omr_j2kdec.hip) ---------------

struct JpegPlan;
struct J2kPlan;
// One stream: its bytes are at d_src + in_off, it decodes to d_dst + dst_off; parsed: what the
// codec's prepare said of it (anything but OMR_OK: it is not decoded and that is its status).
struct CodecJob {
    uint64_t in_off = 0, dst_off = 0;
    omr_status parsed = OMR_OK;
};
// What a decode group leaves for fetch_codec_statuses: st, the call's own result; the statuses its
// kernels write, one word per entry of `live` (indices into the jobs) at `off` in T->d_tab and
// T->pin_tab.  live empty: no kernel of the group reports anything.
struct CodecLaunched {
    omr_status st = OMR_OK;
    size_t off = 0;
    std::vector<int32_t> live;
    CodecLaunched(omr_status s = OMR_OK) : st(s) {}
};
// The descriptor table of the jobs (plans[k]: job k's prepare) into T->pin_tab, up in one copy, the
// workspace in T->d_coef, and the kernels on the context's stream: K17a, K17b, K17c, or K19a, K19b
// per level and K19c (swap16: 16-bit samples are stored byte-swapped).  status: filled with the
// jobs' parsed; K17's kernels add theirs through fetch_codec_statuses, K19's have none to add.
CodecLaunched jpeg_decode_group(Ctx* ctx, SegPipe* T, const std::vector<CodecJob>& jobs, const std::vector<JpegPlan>& plans,
                                int32_t samples, bool ycc, const uint8_t* d_src, uint8_t* d_dst, std::vector<int32_t>& status);
CodecLaunched j2k_decode_group(Ctx* ctx, SegPipe* T, const std::vector<CodecJob>& jobs, const std::vector<J2kPlan>& plans,
                               bool swap16, const uint8_t* d_src, uint8_t* d_dst, std::vector<int32_t>& status);
// The end of every decode group: the kernels' status words back (when there are any), the one
// synchronisation of the stream, and the words into status[live[j]].
omr_status fetch_codec_statuses(Ctx* ctx, SegPipe* T, const CodecLaunched& launched, std::vector<int32_t>& status);

// The body of omr_{jpeg,j2k}_decode_batch_device behind its checks and its prepare loop: the parsed
// jobs' streams (src + offsets[k], lengths[k]) laid out 16-byte aligned in the pipe's pinned buffer
// (grown under "<codec> staging") and uploaded, decode(status) launched -- it finds the jobs' in_off
// set and the bytes at T->d_in -- and the statuses fetched and copied to status_out[0, jobs.size()).
using DecodeGroupFn = std::function<CodecLaunched(std::vector<int32_t>& status)>;
omr_status decode_batch_staged(Ctx* ctx, SegPipe* T, const char* codec, std::vector<CodecJob>& jobs, const uint8_t* src,
                               const uint64_t* offsets, const uint32_t* lengths, const DecodeGroupFn& decode,
                               int32_t* status_out);

// Growth of a pipe's buffers (omr_segread.cpp): device memory, and a pinned buffer with its device
// twin of at least `total` bytes (by half again when they grow); what: the words of the message.
omr_status grow_device(Ctx* c, void*& p, size_t& cap, size_t bytes);
omr_status grow_pinned(Ctx* c, void*& pin, void*& dev, size_t& cap, size_t total, const std::string& what);

// ---- the device route (omr_segread.cpp) ---------------------------------------------------------

// What the four front-end entry points check before they read: the image's side of it.  in_bounds:
// whether a width x height region at a request lies inside level `level` (called once the level is
// known to exist).
struct SegImageDims {
    int32_t level, n_levels, bpp, sc;
    std::function<bool(const omr_raw_tile_request&, int32_t width, int32_t height)> in_bounds;
};

// omr_{tiff,zarr}_image_read_regions_device behind its null checks of ctx and img: the argument
// checks, their messages under S.tag, then n regions in groups within the staging budgets.  S may
// have been made for a level outside the image; it is refused here before its geometry is read.
omr_status read_regions_checked(Ctx* ctx, SegSource& S, const SegImageDims& im, const omr_raw_tile_request* reqs, int32_t n,
                                int32_t width, int32_t height, void* d_dst, int64_t region_stride_bytes);

// omr_render_{tiff,zarr}_tiles behind the same two checks: its argument checks, the active
// channels compacted, groups of kRenderGroupBytes read by read_regions_checked into the pipe's
// region buffer, rendered, and copied back when the output is on the host.
omr_status render_tiles_checked(omr_ctx* ctx, SegSource& S, const SegImageDims& im, const omr_quantum_def* qdef,
                                const omr_channel_binding* channels, int32_t size_c, const omr_tile_request* reqs, int32_t n,
                                int32_t width, int32_t height, int32_t flip_h, int32_t flip_v, uint32_t* argb_out,
                                int32_t out_on_device);

}  // namespace omr
