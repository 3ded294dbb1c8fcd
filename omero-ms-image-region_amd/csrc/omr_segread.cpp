// omr_segread.cpp — the device route of the TIFF and the Zarr reader (omr_segread.h): the staging
// of a context and its growth, one group of regions from plan to status scan (the run stage with
// the decoder of the source's codec: K13a, K14a or K16a, then K13b; Blosc chunks through their own
// finish: container parsing, K15a and K16a side by side, K15b; JPEG and JPEG 2000 segments through
// the image-codec finish: the codec's prepare, K17a .. K17c or K19a .. K19c, K13b), the group loop,
// the tile renderer, the argument checks of the front-ends' entry points and the staging of the two
// batch decoders.  Every HIP call of the two readers is in this file, but for the JPEG and JPEG 2000
// groups' table uploads and launches (omr_jpegdec.hip, omr_j2kdec.hip).
#include "omr_segread.h"

#include "omr_j2kdec.h"
#include "omr_jpegdec.h"

namespace omr {

SegPipe::~SegPipe() {
    if (pin) (void)hipHostFree(pin);
    if (pin_tab) (void)hipHostFree(pin_tab);
    for (void* p : {d_in, d_scratch, d_regions, d_out, d_tab, d_lit, d_coef})
        if (p) (void)hipFree(p);
}

omr_status grow_device(Ctx* c, void*& p, size_t& cap, size_t bytes) {
    if (bytes <= cap) return OMR_OK;
    if (p) OMR_HIP(c, hipFree(p));
    p = nullptr;
    cap = 0;
    OMR_HIP(c, hipMalloc(&p, bytes));
    cap = bytes;
    return OMR_OK;
}

omr_status grow_pinned(Ctx* c, void*& pin, void*& dev, size_t& cap, size_t total, const std::string& what) {
    if (total <= cap) return OMR_OK;
    if (pin) OMR_HIP(c, hipHostFree(pin));
    pin = nullptr;
    const size_t keep = cap;
    cap = 0;
    const omr_status st = grow_device(c, dev, cap, std::max(total, keep + keep / 2));
    if (st) return st;
    const hipError_t e = hipHostMalloc(&pin, cap, hipHostMallocDefault);
    if (e != hipSuccess) {
        cap = 0;                                         // both are made again on the next call
        return hip_fail(c, e, ("hipHostMalloc(" + what + ")").c_str());
    }
    return OMR_OK;
}

namespace {

void free_seg_pipe(void* p) { delete static_cast<SegPipe*>(p); }

std::string said(const SegSource& S, const char* what) { return std::string(S.tag) + ": " + what; }

// After the launches: the statuses back (one stream synchronisation) and their scan.
omr_status scan_statuses(Ctx* ctx, const SegSource& S, const TableLayout& t, uint8_t* tab, uint8_t* dtab, const char* codec) {
    if (t.m) OMR_HIP(ctx, hipMemcpyAsync(tab + t.o_status, dtab + t.o_status, 4 * t.m, hipMemcpyDeviceToHost, ctx->stream));
    OMR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int32_t* h_status = t.status(tab);
    for (size_t j = 0; j < t.m; ++j)
        if (h_status[j] != OMR_OK) return fail(ctx, OMR_INTERNAL, said(S, "corrupt ") + codec + " " + S.noun);
    return OMR_OK;
}

// The Blosc half of read_group, from the chunk files in pinned memory on: the host checks every
// chunk's container and lists its streams (a bad one ends the call before any launch), the bytes go
// up, the tables behind them in a copy of their own (their size is known only now), K15a and K16a
// decode the streams into the chunks' scratch and K15b places with the un-shuffle in its loads.
omr_status finish_blosc(Ctx* ctx, SegPipe* T, const SegSource& S, const SegPlan& plan, const std::vector<SegBytes>& chunks,
                        size_t in_bytes) {
    uint8_t* pin = static_cast<uint8_t*>(T->pin);
    uint8_t* din = static_cast<uint8_t*>(T->d_in);
    uint8_t* dscr = static_cast<uint8_t*>(T->d_scratch);
    std::vector<BloscLayout> layouts(chunks.size());
    size_t m = 0, m_lz4 = 0;                               // streams; those of LZ4 chunks come first in the tables
    for (size_t k = 0; k < chunks.size(); ++k) {
        const SegBytes& u = chunks[k];
        if (!u.cnt) continue;
        if (!blosc_parse(pin + u.in_off, (size_t)u.cnt, u.expected, layouts[k], S.blosc_inner))
            return fail(ctx, OMR_INTERNAL, said(S, "corrupt blosc ") + S.noun);
        m += layouts[k].streams.size();
        if (layouts[k].format != 4u) m_lz4 += layouts[k].streams.size();
    }
    const TableLayout t(0, m, plan.places.size() * sizeof(BloscPlace), true);
    const omr_status grown = grow_pinned(ctx, T->pin_tab, T->d_tab, T->tab_cap, t.total, std::string(S.tag) + " tables");
    if (grown) return grown;
    uint8_t* tab = static_cast<uint8_t*>(T->pin_tab);
    uint8_t* dtab = static_cast<uint8_t*>(T->d_tab);
    size_t j_lz4 = 0, j_zstd = m_lz4;                      // a stored split goes with its chunk's launch
    for (size_t k = 0; k < chunks.size(); ++k)
        for (const BloscStream& s : layouts[k].streams) {
            const size_t j = layouts[k].format != 4u ? j_lz4++ : j_zstd++;
            t.off(tab)[j] = chunks[k].in_off + s.src_off;
            t.dst(tab)[j] = chunks[k].scratch_off + s.dst_off;
            t.len(tab)[j] = s.csize;
            t.exp(tab)[j] = s.neblock;
            t.raw(tab)[j] = s.raw;
        }
    BloscPlace* h_place = reinterpret_cast<BloscPlace*>(tab + t.o_place);
    for (size_t k = 0; k < plan.places.size(); ++k) {
        const size_t ck = (size_t)plan.place_seg[k];
        const SegBytes& u = chunks[ck];
        const BloscLayout& L = layouts[ck];
        const TiffPlace& p = plan.places[k];
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
    OMR_HIP(ctx, hipMemcpyAsync(dtab, tab, t.up_bytes, hipMemcpyHostToDevice, ctx->stream));
    omr_status st = launch_lz4_decode(ctx, t.rows(din, dtab, 0, m_lz4, dscr, true));
    if (st) return st;
    st = launch_zstd_decode(ctx, t.rows(din, dtab, m_lz4, m - m_lz4, dscr, true), &T->d_lit, &T->lit_cap);
    if (st) return st;
    st = launch_blosc_place(ctx, reinterpret_cast<const BloscPlace*>(dtab + t.o_place), (int32_t)plan.places.size(),
                            plan.max_rows, S.geom.bpp);
    if (st) return st;
    return scan_statuses(ctx, S, t, tab, dtab, "blosc");
}

// The placements of a group behind its bytes and rows (t.o_place), their sources set, and the
// staging copy: everything up to t.up_bytes goes up.
omr_status upload_staging(Ctx* ctx, SegPipe* T, SegPlan& plan, const std::vector<SegBytes>& segs, const TableLayout& t, bool decoded) {
    uint8_t* pin = static_cast<uint8_t*>(T->pin);
    uint8_t* din = static_cast<uint8_t*>(T->d_in);
    uint8_t* dscr = static_cast<uint8_t*>(T->d_scratch);
    TiffPlace* h_place = reinterpret_cast<TiffPlace*>(pin + t.o_place);
    for (size_t k = 0; k < plan.places.size(); ++k) {
        const SegBytes& u = segs[(size_t)plan.place_seg[k]];
        plan.places[k].src = !u.cnt ? nullptr : decoded ? dscr + u.scratch_off : din + u.in_off;
        h_place[k] = plan.places[k];
    }
    OMR_HIP(ctx, hipMemcpyAsync(din, pin, t.up_bytes, hipMemcpyHostToDevice, ctx->stream));
    return OMR_OK;
}

// The image-codec half of read_group (JPEG: K17, JPEG 2000: K19), from the segments' bytes in pinned
// memory on.  While they are there the host runs the codec's prepare on every coded segment (JPEG:
// the header up to SOS merged with the IFD's JPEGTables, the lookup tables and the restart intervals;
// JPEG 2000: the headers and the packet walk), on threads when the group holds more than
// `threaded_over` bytes; a segment it refuses ends the call before any launch.  The bytes and the
// placements go up in the staging copy (t: a layout without stream rows), the codec's descriptors
// behind them in a copy of their own; its kernels decode into the segments' scratch as chunky
// samples and K13b places them as it places a chunky Deflate segment of the same sample type.
// prepare(key, segment, its bytes, plan, why) and decode(jobs, plans, status) are all a codec adds.
template <typename Plan, typename Prepare, typename Decode>
omr_status finish_image_codec(Ctx* ctx, SegPipe* T, const SegSource& S, SegPlan& plan, const std::vector<SegBytes>& segs,
                              const TableLayout& t, size_t in_bytes, const std::string& name, size_t threaded_over,
                              const Prepare& prepare, const Decode& decode) {
    const uint8_t* pin = static_cast<const uint8_t*>(T->pin);
    std::vector<int32_t> coded;
    for (size_t k = 0; k < segs.size(); ++k)
        if (segs[k].cnt) coded.push_back((int32_t)k);
    const size_t m = coded.size();
    std::vector<CodecJob> jobs(m);
    std::vector<Plan> plans(m);
    std::vector<std::string> why(m);
    parallel_for((int)m, in_bytes > threaded_over, [&](int j) {
        const size_t k = (size_t)coded[(size_t)j];
        jobs[(size_t)j].in_off = segs[k].in_off;
        jobs[(size_t)j].dst_off = segs[k].scratch_off;
        jobs[(size_t)j].parsed = prepare(plan.segs[k], segs[k], pin + segs[k].in_off, plans[(size_t)j], &why[(size_t)j]);
    });
    for (size_t j = 0; j < m; ++j)
        if (jobs[j].parsed == OMR_INVALID_ARGUMENT) return fail(ctx, OMR_INVALID_ARGUMENT, said(S, "unsupported ") + name + " segment: " + why[j]);
        else if (jobs[j].parsed) return fail(ctx, OMR_INTERNAL, said(S, "corrupt ") + name + " " + S.noun + " (" + why[j] + ")");
    omr_status st = upload_staging(ctx, T, plan, segs, t, true);
    if (st) return st;
    std::vector<int32_t> status;
    const CodecLaunched launched = decode(jobs, plans, status);
    if (launched.st) return launched.st;
    st = launch_tiff_place(ctx, reinterpret_cast<const TiffPlace*>(static_cast<const uint8_t*>(T->d_in) + t.o_place),
                           (int32_t)plan.places.size(), plan.max_rows, S.geom.bpp, 1, false, S.geom.spp);
    if (st) return st;
    st = fetch_codec_statuses(ctx, T, launched, status);
    if (st) return st;
    for (int32_t s : status)
        if (s != OMR_OK) return fail(ctx, OMR_INTERNAL, said(S, "corrupt ") + name + " " + S.noun);
    return OMR_OK;
}

// The two image codecs: their names, thresholds, row arithmetic and calls.
omr_status finish_image(Ctx* ctx, SegPipe* T, const SegSource& S, SegPlan& plan, const std::vector<SegBytes>& segs,
                        const TableLayout& t, size_t in_bytes) {
    const SegGeom& g = S.geom;
    uint8_t* din = static_cast<uint8_t*>(T->d_in);
    uint8_t* dscr = static_cast<uint8_t*>(T->d_scratch);
    if (S.codec == SegCodec::jpeg)
        return finish_image_codec<JpegPlan>(
            ctx, T, S, plan, segs, t, in_bytes, "JPEG", (size_t)1 << 20,
            [&](const SegKey& key, const SegBytes& u, const uint8_t* bytes, JpegPlan& P, std::string* why) {
                size_t tl = 0;
                const uint8_t* tb = S.jpeg_tables(key, &tl);
                const int32_t rows = (int32_t)(u.expected / ((uint32_t)g.seg_w * (uint32_t)g.spp));
                return jpeg_prepare(tb, tl, bytes, (size_t)u.cnt, g.seg_w, rows, g.spp, P, why);
            },
            [&](const std::vector<CodecJob>& jobs, const std::vector<JpegPlan>& plans, std::vector<int32_t>& status) {
                return jpeg_decode_group(ctx, T, jobs, plans, g.spp, S.jpeg_ycc, din, dscr, status);
            });
    return finish_image_codec<J2kPlan>(
        ctx, T, S, plan, segs, t, in_bytes, "JPEG 2000", (size_t)1 << 18,
        [&](const SegKey&, const SegBytes& u, const uint8_t* bytes, J2kPlan& P, std::string* why) {
            const int32_t rows = (int32_t)(u.expected / ((uint32_t)g.seg_w * (uint32_t)g.spp * (uint32_t)g.bpp));
            return j2k_prepare(bytes, (size_t)u.cnt, g.seg_w, rows, g.spp, 8 * g.bpp, P, why, S.j2k_kinds);
        },
        [&](const std::vector<CodecJob>& jobs, const std::vector<J2kPlan>& plans, std::vector<int32_t>& status) {
            return j2k_decode_group(ctx, T, jobs, plans, S.swap, din, dscr, status);
        });
}

// One group of regions: reqs[r0, r1).
omr_status read_group(Ctx* ctx, SegSource& S, const omr_raw_tile_request* reqs, int32_t r0, int32_t r1, int32_t width,
                      int32_t height, uint8_t* d_dst, int64_t stride) {
    SegPlan plan = plan_regions(S.geom, reqs, r0, r1, width, height, d_dst, stride,
                                [&](const omr_raw_tile_request& r) { return S.plane_of(r); },
                                [&](const omr_raw_tile_request& r) { return S.sample_of(r); });
    if (plan.places.empty()) return OMR_OK;
    std::vector<SegBytes> segs(plan.segs.size());
    omr_status st = S.sizes(ctx, plan.segs, segs);
    if (st) return st;
    const bool blosc = S.codec == SegCodec::blosc;         // its tables go up behind the bytes, from T->pin_tab
    const bool image = S.codec == SegCodec::jpeg || S.codec == SegCodec::j2k;   // descriptors of their own, as Blosc
    const bool decoded = S.codec != SegCodec::none;
    size_t in_bytes = 0, scratch_bytes = 0;
    std::vector<int32_t> coded;                            // the segments a stream-table decoder gets
    for (size_t k = 0; k < segs.size(); ++k) {
        SegBytes& u = segs[k];
        if (!u.cnt) continue;
        u.in_off = in_bytes;
        in_bytes += align_up((size_t)u.cnt, 16);
        if (decoded) {
            u.scratch_off = scratch_bytes;
            scratch_bytes += align_up((size_t)u.expected, 16);
            if (!blosc && !image) coded.push_back((int32_t)k);
        }
    }
    const size_t m = coded.size();
    const TableLayout t(in_bytes, m, blosc ? 0 : plan.places.size() * sizeof(TiffPlace), false);
    SegPipe* T = seg_pipe(ctx, S.kind);
    st = grow_pinned(ctx, T->pin, T->d_in, T->in_cap, t.total, std::string(S.tag) + " staging");
    if (st) return st;
    st = grow_device(ctx, T->d_scratch, T->scratch_cap, scratch_bytes);
    if (st) return st;
    uint8_t* pin = static_cast<uint8_t*>(T->pin);
    uint8_t* din = static_cast<uint8_t*>(T->d_in);
    uint8_t* dscr = static_cast<uint8_t*>(T->d_scratch);
    if (!S.read(plan.segs, segs, pin, in_bytes)) return fail(ctx, OMR_INTERNAL, said(S, S.noun) + " read failed");
    if (blosc) return finish_blosc(ctx, T, S, plan, segs, in_bytes);
    if (image) return finish_image(ctx, T, S, plan, segs, t, in_bytes);
    for (size_t j = 0; j < m; ++j) {
        const SegBytes& u = segs[(size_t)coded[j]];
        t.off(pin)[j] = u.in_off;
        t.dst(pin)[j] = u.scratch_off;
        t.len(pin)[j] = (uint32_t)u.cnt;
        t.exp(pin)[j] = u.expected;
    }
    st = upload_staging(ctx, T, plan, segs, t, decoded);
    if (st) return st;
    const StreamTable rows = t.rows(din, din, 0, m, dscr, false);
    const char* codec = "";
    switch (S.codec) {
    case SegCodec::lzw: codec = "LZW"; st = launch_lzw_decode(ctx, rows); break;
    case SegCodec::zlib: codec = "zlib"; st = launch_inflate(ctx, rows); break;
    case SegCodec::zstd: codec = "zstd"; st = launch_zstd_decode(ctx, rows, &T->d_lit, &T->lit_cap); break;
    default: break;
    }
    if (st) return st;
    st = launch_tiff_place(ctx, reinterpret_cast<const TiffPlace*>(din + t.o_place), (int32_t)plan.places.size(),
                           plan.max_rows, S.geom.bpp, S.predictor, S.swap, S.geom.spp);
    if (st) return st;
    return scan_statuses(ctx, S, t, pin, din, codec);
}

}  // namespace

SegPipe* seg_pipe(Ctx* c, SegKind kind) {
    void*& state = kind == SegKind::tiff ? c->tiff_state : c->zarr_state;
    if (!state) {
        state = new SegPipe;
        (kind == SegKind::tiff ? c->tiff_state_free : c->zarr_state_free) = free_seg_pipe;
    }
    return static_cast<SegPipe*>(state);
}

omr_status fetch_codec_statuses(Ctx* ctx, SegPipe* T, const CodecLaunched& launched, std::vector<int32_t>& status) {
    const size_t m = launched.live.size();
    uint8_t* tab = static_cast<uint8_t*>(T->pin_tab);
    if (m) OMR_HIP(ctx, hipMemcpyAsync(tab + launched.off, static_cast<uint8_t*>(T->d_tab) + launched.off, 4 * m,
                                       hipMemcpyDeviceToHost, ctx->stream));
    OMR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int32_t* h = reinterpret_cast<const int32_t*>(tab + launched.off);
    for (size_t j = 0; j < m; ++j) status[(size_t)launched.live[j]] = h[j];
    return OMR_OK;
}

omr_status decode_batch_staged(Ctx* ctx, SegPipe* T, const char* codec, std::vector<CodecJob>& jobs, const uint8_t* src,
                               const uint64_t* offsets, const uint32_t* lengths, const DecodeGroupFn& decode,
                               int32_t* status_out) {
    size_t in_bytes = 0;
    for (size_t k = 0; k < jobs.size(); ++k) {
        jobs[k].in_off = in_bytes;
        if (jobs[k].parsed == OMR_OK) in_bytes += align_up((size_t)lengths[k], 16);
    }
    omr_status st = grow_pinned(ctx, T->pin, T->d_in, T->in_cap, std::max<size_t>(in_bytes, 16), std::string(codec) + " staging");
    if (st) return st;
    uint8_t* pin = static_cast<uint8_t*>(T->pin);
    for (size_t k = 0; k < jobs.size(); ++k)
        if (jobs[k].parsed == OMR_OK) std::memcpy(pin + jobs[k].in_off, src + offsets[k], lengths[k]);
    if (in_bytes) OMR_HIP(ctx, hipMemcpyAsync(T->d_in, pin, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    std::vector<int32_t> status;
    const CodecLaunched launched = decode(status);
    if (launched.st) return launched.st;
    st = fetch_codec_statuses(ctx, T, launched, status);
    if (st) return st;
    std::copy(status.begin(), status.end(), status_out);
    return OMR_OK;
}

omr_status read_regions_checked(Ctx* ctx, SegSource& S, const SegImageDims& im, const omr_raw_tile_request* reqs, int32_t n,
                                int32_t width, int32_t height, void* d_dst, int64_t region_stride_bytes) {
    if (n < 0 || (n && (!reqs || !d_dst))) return fail(ctx, OMR_INVALID_ARGUMENT, said(S, "null argument"));
    if (im.level < 0 || im.level >= im.n_levels) return fail(ctx, OMR_INVALID_ARGUMENT, said(S, "no such level"));
    if (width < 0 || height < 0) return fail(ctx, OMR_INVALID_ARGUMENT, said(S, "bad region size"));
    const int64_t region_bytes = (int64_t)width * height * im.bpp;
    if (region_stride_bytes < region_bytes || region_stride_bytes % im.bpp || reinterpret_cast<uintptr_t>(d_dst) % (uintptr_t)im.bpp)
        return fail(ctx, OMR_INVALID_ARGUMENT, said(S, "region stride or destination not a multiple of the sample size"));
    for (int32_t i = 0; i < n; ++i)
        if (!im.in_bounds(reqs[i], width, height))
            return fail(ctx, OMR_INVALID_ARGUMENT, said(S, "region ") + std::to_string(i) + " outside the image");
    if (n == 0 || width == 0 || height == 0) return OMR_OK;
    OMR_HIP(ctx, hipSetDevice(ctx->device));
    const size_t per_req = read_bytes_per_request(S.geom, width, height) + codec_workspace_per_request(S.codec, S.geom, width, height);
    const int32_t G = group_size(n, std::min(kGroupInBytes, kGroupScratchBytes), per_req);
    for (int32_t r0 = 0; r0 < n; r0 += G) {
        const omr_status st = read_group(ctx, S, reqs, r0, std::min(n, r0 + G), width, height, static_cast<uint8_t*>(d_dst),
                                         region_stride_bytes);
        if (st) return st;
    }
    return OMR_OK;
}

omr_status render_tiles_checked(omr_ctx* ctx, SegSource& src, const SegImageDims& im, const omr_quantum_def* qdef,
                                const omr_channel_binding* channels, int32_t size_c, const omr_tile_request* reqs, int32_t n,
                                int32_t width, int32_t height, int32_t flip_h, int32_t flip_v, uint32_t* argb_out,
                                int32_t out_on_device) {
    if (!qdef || !channels || !reqs || !argb_out || n < 0) return fail(ctx, OMR_INVALID_ARGUMENT, "null argument");
    if (size_c != im.sc) return fail(ctx, OMR_INVALID_ARGUMENT, "channel bindings do not match the image's sizeC");
    if (width <= 0 || height <= 0) return fail(ctx, OMR_INVALID_ARGUMENT, "bad tile size");
    if (im.level < 0 || im.level >= im.n_levels) return fail(ctx, OMR_INVALID_ARGUMENT, said(src, "no such level"));
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
    SegPipe* T = seg_pipe(ctx, src.kind);
    const size_t plane_al = align_up((size_t)width * height * src.geom.bpp, 16);   // K2's vector path: 16-byte strides
    const size_t tile_out = (size_t)width * height * 4;
    const int32_t G = group_size(n, kRenderGroupBytes, plane_al * std::max(na, 1));
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
        st = read_regions_checked(ctx, src, im, rr.data(), cnt * na, width, height, T->d_regions, (int64_t)plane_al);
        if (st) return st;
        uint32_t* dout = out_on_device ? argb_out + (size_t)t0 * width * height : static_cast<uint32_t*>(T->d_out);
        st = omr_render_batch_strided_device(ctx, qdef, bind.data(), (int32_t)bind.size(), T->d_regions, (int64_t)(plane_al * na),
                                             (int64_t)plane_al, cnt, 0, src.pt, src.big, width, height, flip_h, flip_v,
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

}  // namespace omr
