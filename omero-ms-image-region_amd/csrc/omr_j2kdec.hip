// omr_j2kdec.hip — K19 and K20, device half: JPEG 2000 codestreams decoded on the GPU, reversible
// (K19) and irreversible (K20) ones side by side.
//
// The host (j2k_prepare, omr_j2kdec.cpp) has parsed every segment's headers and walked its packets;
// j2k_decode_group here puts its code-block list into one descriptor table, and three kernels do
// the rest, all through the functions of omr_j2kdec.h that the host decoder runs too:
//
//   K19a  k_j2k_t1      one wave (a workgroup of 64 threads) per code-block.  The MQ chain is
//         serial -- every decision depends on the one before it through the decoder's registers and
//         the contexts' states -- so the decode runs wave-uniform, as K17a, K14a and K16a do: all
//         lanes execute j2k_t1_decode on the same values (what is loaded goes through
//         readfirstlane, so the branches are scalar) and store the same bytes to the same LDS
//         addresses.  The block's state lives in LDS, bounded by the standard's cap of 4096 samples
//         per block: 16 KiB of magnitudes, at most 6,156 B of bordered flags (the 1024 x 4 and 4 x
//         1024 shapes) and the 19 context states, 22,576 B per workgroup, so seven fit a CU.  The
//         lanes share the work where there is work to share: they zero the state and they store the
//         finished block as signed int32 into its subband's place in the component's plane, a row
//         of the block across the lanes.
//   K19b  k_j2k_idwt53  one launch per decomposition level for the whole batch, lowest resolution
//         first, one lane per output sample of that resolution: the horizontal then the vertical
//         5/3 lifting of j2k_idwt53_at, which reads the low-pass quadrant from the level before and
//         the other three from the coefficient planes.  A segment with fewer levels idles.
//   K19c  k_j2k_pixels  one lane per pixel: the inverse RCT where the stream asks for it, the level
//         shift, the clamp and the chunky 8- or 16-bit store.
//
// K20.  A segment's descriptor says whether its stream is irreversible (J2kSegDesc::lossy).  K19a
// then stores j2k_dequantise's float in the coefficient's four bytes, K19c runs j2k_pixel97 (the
// inverse ICT, round to nearest even, level shift, clamp), K19b leaves the segment alone and
//   K20b  k_j2k_idwt97  transforms it, again one launch per level for the batch.  A 9/7 output
//         sample reaches 9 x 9 inputs through four dependent lifting steps, so K19b's scheme of one
//         lane per output sample does not carry over: one workgroup of 256 lanes takes one 64 x 32
//         output tile of the level (of one component of one segment).  It stages the tile with a
//         halo of four samples on each side, interleaved, in LDS -- 40 rows of 72 floats, a row
//         pitch of 73 -- reading the low quadrant from the level before and the rest from the
//         coefficient planes; a place beyond the level's edge takes the sample at the reflected
//         index (period 2 (n - 1), so lines of 2, 3 and 4 samples work), which is what whole-sample
//         symmetric extension means and what every lifting step preserves.  The samples are scaled
//         as they are loaded; then the four steps run along the rows of all 40 rows in place, each
//         writing one parity and reading the other, a barrier between two steps; the outermost
//         samples, whose neighbours are not in the tile, go stale by one place per step, four in
//         all: the halo.  Then the same along the columns of the 64 inner columns, and the 64 x 32
//         interior is stored.  Every value is computed by j2k_lift97_scale and j2k_lift97_step on
//         the operands the host's j2k_lift97_line gives them, so the two routes agree bit for bit.
//         LDS banking (ds_read_b32 and ds_write_b32: bank = dword address mod 32, conflicts within
//         a half-wave): in the row steps consecutive lanes take consecutive ROWS of one column,
//         73 = 9 mod 32 dwords apart, so the 32 lanes of a half-wave hit 32 banks where a walk
//         along the row at stride 2 would pair them up; in the column steps and in the load and
//         store consecutive lanes take consecutive columns of one row.
//
// Bounds.  K19a takes a block's size from its descriptor and leaves at once when it is not one the
// LDS arrays hold (the host never writes such a one); j2k_t1_decode indexes the magnitudes with
// y * w + x and the flags with (y + 1) * (w + 2) + x + 1 +- (w + 2) +- 1 for x < w and y < h, all
// inside w * h <= 4096 values and (w + 2) * (h + 2) <= 6156 bytes; the stream's bytes decide values
// alone, and its passes loop over at most 88 passes of at most 4096 samples.  It reads src only at
// positions inside the block's ranges (J2kMq::cur compares with the range's end), which the host
// laid inside the segment's uploaded bytes; behind them it is fed FF.  The finished block goes to
// a_off + 4 * (ws_off + y * stride + x), inside the segment's ncomp * w * h coefficients by
// j2k_prepare.  K19b and K19c take every size from the host's descriptors and none from the stream:
// output sample (x, y) of a resolution of rw x rh reads columns below rw and rows below rh of planes
// whose rows are w >= rw (or ceil(w / 2) >= rw for the half-size plane) apart, and writes its own
// place; pixel p < w * h reads its ncomp values and writes ncomp samples at dst_off + p * ncomp *
// bits / 8, inside the bytes the segment owns.  K20b takes its sizes from the descriptors too: a
// staged place (tx, ty) < (72, 40) reads the level's sample at reflected indices, in [0, rw) x [0, rh)
// by j2k_reflect, from the planes K19b reads, the steps touch s_t[ty * 73 + tx +- 1] for 1 <= tx <= 70
// and s_t[(ty +- 1) * 73 + tx] for 1 <= ty <= 38, and only places with x < rw and y < rh are stored.
// No kernel can fail: the damage that can be seen is
// seen on the host, before any launch.
#include "omr_j2kdec.h"
#include "omr_segread.h"

namespace omr {
namespace {

constexpr int kKindJ2kT1 = 41;         // omr_ctx_kernel_timings kinds (omr.h)
constexpr int kKindJ2kIdwt = 42;
constexpr int kKindJ2kPixels = 43;
constexpr int kKindJ2kIdwt97 = 44;

constexpr int kT97W = 64, kT97H = 32;                      // K20b: the output tile of one workgroup
constexpr int kT97LW = kT97W + 2 * kJ2kLift97Halo, kT97LH = kT97H + 2 * kJ2kLift97Halo, kT97Pitch = kT97LW + 1;
static_assert((kT97W % 2) == 0 && (kT97H % 2) == 0 && (kJ2kLift97Halo % 2) == 0, "a staged place's parity is its sample's");

// K19a.  The bounds argument is at the head of this file.
__global__ void __launch_bounds__(64) k_j2k_t1(const uint8_t* __restrict__ src, const J2kSegDesc* __restrict__ segs,
                                               const J2kBlock* __restrict__ blocks, const J2kRange* __restrict__ ranges,
                                               uint8_t* __restrict__ ws) {
    __shared__ uint32_t s_mag[kJ2kMaxBlockArea];
    __shared__ uint32_t s_fl[kJ2kMaxFlagBytes / 4];
    __shared__ uint32_t s_cx[8];
    const uint32_t lane = threadIdx.x;
    J2kBlock B = blocks[blockIdx.x];
    B.ws_off = OMR_J2K_UNI(B.ws_off); B.stride = OMR_J2K_UNI(B.stride);
    B.range0 = OMR_J2K_UNI(B.range0); B.n_ranges = OMR_J2K_UNI(B.n_ranges);
    B.w = (uint16_t)OMR_J2K_UNI(B.w); B.h = (uint16_t)OMR_J2K_UNI(B.h);
    B.passes = (uint16_t)OMR_J2K_UNI(B.passes);
    B.orient = (uint8_t)OMR_J2K_UNI(B.orient); B.planes = (uint8_t)OMR_J2K_UNI(B.planes);
    B.seg = OMR_J2K_UNI(B.seg);
    const uint32_t w = B.w, h = B.h, area = w * h, fbytes = (w + 2u) * (h + 2u);
    if (w < 1u || h < 1u || area > kJ2kMaxBlockArea || fbytes > kJ2kMaxFlagBytes) return;
    for (uint32_t i = lane; i < area; i += 64u) s_mag[i] = 0u;
    for (uint32_t i = lane; i < (fbytes + 3u) / 4u; i += 64u) s_fl[i] = 0u;
    __syncthreads();
    const uint64_t src_off = segs[B.seg].src_off, a_off = segs[B.seg].a_off;
    uint8_t* fl = reinterpret_cast<uint8_t*>(s_fl);
    j2k_t1_decode<false>(src + src_off, ranges, B, s_mag, fl, reinterpret_cast<uint8_t*>(s_cx));
    __syncthreads();
    int32_t* a = reinterpret_cast<int32_t*>(ws + a_off) + B.ws_off;
    const bool lossy = OMR_J2K_UNI(segs[B.seg].lossy) != 0u;
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = lane; x < w; x += 64u) {
            const uint32_t m = s_mag[y * w + x], f = fl[(y + 1u) * (w + 2u) + x + 1u];
            a[(size_t)y * B.stride + x] = lossy ? (int32_t)j2k_float_bits(j2k_dequantise(m, f, B.step)) : j2k_coefficient(m, f);
        }
}

// K19b: output sample p of component blockIdx.z of segment blockIdx.y (+ k * gridDim.y), level `level`.
__global__ void __launch_bounds__(256) k_j2k_idwt53(const J2kSegDesc* __restrict__ segs, int32_t n_seg, uint8_t* ws, int32_t level) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int32_t c = (int32_t)blockIdx.z;
    for (int32_t seg = (int32_t)blockIdx.y; seg < n_seg; seg += (int32_t)gridDim.y) {
        const J2kSegDesc S = segs[seg];
        if (S.lossy || level > S.levels || c >= S.ncomp) continue;
        const int32_t rw = j2k_ceil_shift(S.w, S.levels - level), rh = j2k_ceil_shift(S.h, S.levels - level);
        if (p >= (int64_t)rw * rh) continue;
        const int32_t x = (int32_t)(p % rw), y = (int32_t)(p / rw), lw = (rw + 1) / 2, lh = (rh + 1) / 2;
        const int32_t yw = (S.w + 1) / 2, yh = (S.h + 1) / 2;
        const size_t plane = (size_t)S.w * S.h, half = (size_t)yw * yh;
        const int32_t* ap = reinterpret_cast<const int32_t*>(ws + S.a_off) + plane * (size_t)c;
        int32_t* xp = reinterpret_cast<int32_t*>(ws + S.x_off) + plane * (size_t)c;
        int32_t* yp = reinterpret_cast<int32_t*>(ws + S.y_off) + half * (size_t)c;
        const bool to_x = j2k_level_writes_x(S.levels, level);
        const int32_t* lp = level == 1 ? ap : to_x ? yp : xp;
        const int32_t lstride = (level == 1 || !to_x) ? S.w : yw;
        const int32_t v = j2k_idwt53_at(rw, rh, x, y, [&](int32_t col, int32_t row) {
            return col < lw && row < lh ? lp[(size_t)row * lstride + col] : ap[(size_t)row * S.w + col];
        });
        (to_x ? xp : yp)[(size_t)y * (to_x ? S.w : yw) + x] = v;
    }
}

// K20b: output tile blockIdx.x of component blockIdx.z of segment blockIdx.y (+ k * gridDim.y), level
// `level`.  The scheme and the bounds argument are at the head of this file.  Every `continue` is
// uniform across the workgroup, so the barriers are.
__global__ void __launch_bounds__(256) k_j2k_idwt97(const J2kSegDesc* __restrict__ segs, int32_t n_seg, uint8_t* ws, int32_t level) {
    __shared__ float s_t[kT97LH * kT97Pitch];
    const int32_t tid = (int32_t)threadIdx.x, c = (int32_t)blockIdx.z;
    for (int32_t seg = (int32_t)blockIdx.y; seg < n_seg; seg += (int32_t)gridDim.y) {
        const J2kSegDesc S = segs[seg];
        if (!S.lossy || level > S.levels || c >= S.ncomp) continue;
        const int32_t rw = j2k_ceil_shift(S.w, S.levels - level), rh = j2k_ceil_shift(S.h, S.levels - level);
        const int32_t tiles_x = (rw + kT97W - 1) / kT97W, tiles_y = (rh + kT97H - 1) / kT97H;
        if ((int64_t)blockIdx.x >= (int64_t)tiles_x * tiles_y) continue;
        const int32_t x0 = (int32_t)(blockIdx.x % (uint32_t)tiles_x) * kT97W, y0 = (int32_t)(blockIdx.x / (uint32_t)tiles_x) * kT97H;
        const int32_t lw = (rw + 1) / 2, lh = (rh + 1) / 2, yw = (S.w + 1) / 2, yh = (S.h + 1) / 2;
        const size_t plane = (size_t)S.w * S.h, half = (size_t)yw * yh;
        const uint32_t* ap = reinterpret_cast<const uint32_t*>(ws + S.a_off) + plane * (size_t)c;
        uint32_t* xp = reinterpret_cast<uint32_t*>(ws + S.x_off) + plane * (size_t)c;
        uint32_t* yp = reinterpret_cast<uint32_t*>(ws + S.y_off) + half * (size_t)c;
        const bool to_x = j2k_level_writes_x(S.levels, level);
        const uint32_t* lp = level == 1 ? ap : to_x ? yp : xp;
        const int32_t lstride = (level == 1 || !to_x) ? S.w : yw;
        const bool rows = rw >= 2, cols = rh >= 2;         // a line of one sample passes through
        // the tile with its halo, interleaved, the samples scaled for the row steps
        for (int32_t i = tid; i < kT97LW * kT97LH; i += 256) {
            const int32_t tx = i % kT97LW, ty = i / kT97LW;
            const int32_t col = j2k_nested_index(j2k_reflect(x0 - kJ2kLift97Halo + tx, rw), rw);
            const int32_t row = j2k_nested_index(j2k_reflect(y0 - kJ2kLift97Halo + ty, rh), rh);
            const float v = j2k_bits_float(col < lw && row < lh ? lp[(size_t)row * lstride + col] : ap[(size_t)row * S.w + col]);
            s_t[ty * kT97Pitch + tx] = rows ? j2k_lift97_scale(v, tx & 1) : v;
        }
        __syncthreads();
        if (rows)
            for (int k = 0; k < kJ2kLift97Steps; ++k) {
                const float cst = j2k_lift97_const(k);
                for (int32_t i = tid; i < (kT97LW / 2) * kT97LH; i += 256) {
                    const int32_t ty = i % kT97LH, tx = 2 * (i / kT97LH) + (k & 1);
                    if (tx < 1 || tx > kT97LW - 2) continue;
                    float* q = s_t + ty * kT97Pitch + tx;
                    *q = j2k_lift97_step(*q, q[-1], q[1], cst);
                }
                __syncthreads();
            }
        if (cols) {
            for (int32_t i = tid; i < kT97W * kT97LH; i += 256) {
                const int32_t tx = kJ2kLift97Halo + i % kT97W, ty = i / kT97W;
                s_t[ty * kT97Pitch + tx] = j2k_lift97_scale(s_t[ty * kT97Pitch + tx], ty & 1);
            }
            __syncthreads();
            for (int k = 0; k < kJ2kLift97Steps; ++k) {
                const float cst = j2k_lift97_const(k);
                for (int32_t i = tid; i < kT97W * (kT97LH / 2); i += 256) {
                    const int32_t tx = kJ2kLift97Halo + i % kT97W, ty = 2 * (i / kT97W) + (k & 1);
                    if (ty < 1 || ty > kT97LH - 2) continue;
                    float* q = s_t + ty * kT97Pitch + tx;
                    *q = j2k_lift97_step(*q, q[-kT97Pitch], q[kT97Pitch], cst);
                }
                __syncthreads();
            }
        }
        uint32_t* op = to_x ? xp : yp;
        const int32_t ostride = to_x ? S.w : yw;
        for (int32_t i = tid; i < kT97W * kT97H; i += 256) {
            const int32_t dx = i % kT97W, dy = i / kT97W;
            if (x0 + dx < rw && y0 + dy < rh)
                op[(size_t)(y0 + dy) * ostride + x0 + dx] = j2k_float_bits(s_t[(dy + kJ2kLift97Halo) * kT97Pitch + dx + kJ2kLift97Halo]);
        }
        __syncthreads();                                   // the next segment's load overwrites the tile
    }
}

// K19c: pixel p of segment blockIdx.y (+ k * gridDim.y).
__global__ void __launch_bounds__(256) k_j2k_pixels(const J2kSegDesc* __restrict__ segs, int32_t n_seg,
                                                    const uint8_t* __restrict__ ws, uint8_t* __restrict__ dst) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (int32_t seg = (int32_t)blockIdx.y; seg < n_seg; seg += (int32_t)gridDim.y) {
        const J2kSegDesc S = segs[seg];
        const size_t plane = (size_t)S.w * S.h;
        if (p >= (int64_t)plane) continue;
        const int32_t* img = reinterpret_cast<const int32_t*>(ws + (S.levels ? S.x_off : S.a_off));
        int32_t v[3] = {0, 0, 0};
        uint32_t o[3];
        const int32_t nc = S.ncomp == 3 ? 3 : 1;
        for (int32_t c = 0; c < nc; ++c) v[c] = img[plane * (size_t)c + (size_t)p];
        if (S.lossy) {
            const float f[3] = {j2k_bits_float((uint32_t)v[0]), j2k_bits_float((uint32_t)v[1]), j2k_bits_float((uint32_t)v[2])};
            j2k_pixel97(f, nc, S.mct != 0, S.bits == 16 ? 16 : 8, o);
        } else {
            j2k_pixel(v, nc, S.mct != 0, S.bits == 16 ? 16 : 8, o);
        }
        if (S.bits == 16) {
            uint16_t* d = reinterpret_cast<uint16_t*>(dst + S.dst_off) + (size_t)p * (size_t)nc;
            for (int32_t c = 0; c < nc; ++c) d[c] = (uint16_t)(S.swap16 ? (o[c] >> 8 | (o[c] & 255u) << 8) : o[c]);
        } else {
            uint8_t* d = dst + S.dst_off + (size_t)p * (size_t)nc;
            for (int32_t c = 0; c < nc; ++c) d[c] = (uint8_t)o[c];
        }
    }
}

}  // namespace

// The descriptor table of one group: [J2kSegDesc m][J2kBlock b][J2kRange r], up in one copy.
CodecLaunched j2k_decode_group(Ctx* ctx, SegPipe* T, const std::vector<CodecJob>& jobs, const std::vector<J2kPlan>& plans,
                               bool swap16, const uint8_t* d_src, uint8_t* d_dst, std::vector<int32_t>& status) {
    const size_t n = jobs.size();
    status.assign(n, OMR_OK);
    std::vector<int32_t> live;                             // the jobs that decode
    size_t n_blocks = 0, n_ranges = 0;
    for (size_t k = 0; k < n; ++k)
        if (jobs[k].parsed == OMR_OK) {
            live.push_back((int32_t)k);
            n_blocks += plans[k].blocks.size();
            n_ranges += plans[k].ranges.size();
        } else {
            status[k] = jobs[k].parsed;
        }
    const size_t m = live.size();
    if (!m) return OMR_OK;
    if (n_blocks > 0x7FFFFFFFull || n_ranges > 0xFFFFFFFFull) return fail(ctx, OMR_INVALID_ARGUMENT, "j2k: too many code-blocks in one group");
    const size_t o_blk = align_up(m * sizeof(J2kSegDesc), 16), o_rng = o_blk + align_up(n_blocks * sizeof(J2kBlock), 16);
    const size_t total = o_rng + n_ranges * sizeof(J2kRange);
    omr_status st = grow_pinned(ctx, T->pin_tab, T->d_tab, T->tab_cap, std::max<size_t>(total, 16), "j2k tables");
    if (st) return st;
    uint8_t* tab = static_cast<uint8_t*>(T->pin_tab);
    uint8_t* dtab = static_cast<uint8_t*>(T->d_tab);
    J2kSegDesc* hs = reinterpret_cast<J2kSegDesc*>(tab);
    J2kBlock* hb = reinterpret_cast<J2kBlock*>(tab + o_blk);
    J2kRange* hr = reinterpret_cast<J2kRange*>(tab + o_rng);
    size_t ws_bytes = 0, b_at = 0, r_at = 0;
    int32_t max_levels = 0, max_comp = 1;
    int64_t max_pixels = 0;
    for (size_t j = 0; j < m; ++j) {
        const CodecJob& J = jobs[(size_t)live[j]];
        const J2kPlan& P = plans[(size_t)live[j]];
        J2kSegDesc& S = hs[j];
        S.dst_off = J.dst_off;
        S.src_off = J.in_off;
        S.a_off = ws_bytes;
        ws_bytes += j2k_plane_bytes(P.w, P.h, P.ncomp);
        S.x_off = ws_bytes;
        if (P.levels > 0) ws_bytes += j2k_plane_bytes(P.w, P.h, P.ncomp);
        S.y_off = ws_bytes;
        if (P.levels > 1) ws_bytes += j2k_half_bytes(P.w, P.h, P.ncomp);
        S.w = P.w; S.h = P.h; S.ncomp = P.ncomp; S.bits = P.bits; S.levels = P.levels; S.mct = P.mct;
        S.swap16 = swap16 && P.bits == 16;
        S.lossy = P.lossy;
        max_levels = std::max(max_levels, P.levels);
        max_comp = std::max(max_comp, P.ncomp);
        max_pixels = std::max(max_pixels, (int64_t)P.w * P.h);
        for (const J2kBlock& K : P.blocks) {
            J2kBlock& D = hb[b_at++];
            D = K;
            D.range0 = (uint32_t)(K.range0 + r_at);
            D.seg = (uint32_t)j;
        }
        if (!P.ranges.empty()) std::memcpy(hr + r_at, P.ranges.data(), P.ranges.size() * sizeof(J2kRange));
        r_at += P.ranges.size();
    }
    st = grow_device(ctx, T->d_coef, T->coef_cap, std::max<size_t>(ws_bytes, 256));
    if (st) return st;
    OMR_HIP(ctx, hipMemcpyAsync(dtab, tab, total, hipMemcpyHostToDevice, ctx->stream));
    const J2kSegDesc* dsegs = reinterpret_cast<const J2kSegDesc*>(dtab);
    uint8_t* ws = static_cast<uint8_t*>(T->d_coef);
    const unsigned gy = (unsigned)std::min<size_t>(m, 65535);
    if (n_blocks) {
        KernelTimer timer(ctx, kKindJ2kT1, true);
        omr_launch(k_j2k_t1, dim3((unsigned)n_blocks), dim3(64), 0u, ctx->stream, d_src, dsegs,
                   reinterpret_cast<const J2kBlock*>(dtab + o_blk), reinterpret_cast<const J2kRange*>(dtab + o_rng), ws);
        OMR_HIP(ctx, hipGetLastError());
    }
    for (int32_t level = 1; level <= max_levels; ++level) {
        int64_t px = 1, tiles = 0;                         // the largest resolution this launch writes, in samples (K19b) and in tiles (K20b)
        bool any53 = false;
        for (size_t j = 0; j < m; ++j)
            if (hs[j].levels >= level) {
                const int64_t rw = j2k_ceil_shift(hs[j].w, hs[j].levels - level), rh = j2k_ceil_shift(hs[j].h, hs[j].levels - level);
                if (hs[j].lossy) {
                    tiles = std::max(tiles, ((rw + kT97W - 1) / kT97W) * ((rh + kT97H - 1) / kT97H));
                } else {
                    px = std::max(px, rw * rh);
                    any53 = true;
                }
            }
        if (any53) {
            KernelTimer timer(ctx, kKindJ2kIdwt, true);
            omr_launch(k_j2k_idwt53, dim3((unsigned)((px + 255) / 256), gy, (unsigned)max_comp), dim3(256), 0u, ctx->stream, dsegs,
                       (int32_t)m, ws, level);
            OMR_HIP(ctx, hipGetLastError());
        }
        if (tiles) {
            KernelTimer timer(ctx, kKindJ2kIdwt97, true);
            omr_launch(k_j2k_idwt97, dim3((unsigned)tiles, gy, (unsigned)max_comp), dim3(256), 0u, ctx->stream, dsegs, (int32_t)m, ws,
                       level);
            OMR_HIP(ctx, hipGetLastError());
        }
    }
    {
        KernelTimer timer(ctx, kKindJ2kPixels, true);
        omr_launch(k_j2k_pixels, dim3((unsigned)((max_pixels + 255) / 256), gy), dim3(256), 0u, ctx->stream, dsegs, (int32_t)m,
                   static_cast<const uint8_t*>(ws), d_dst);
        OMR_HIP(ctx, hipGetLastError());
    }
    return OMR_OK;
}

}  // namespace omr

using namespace omr;

extern "C" omr_status omr_j2k_decode_batch_device(omr_ctx* ctx, const uint8_t* src, const uint64_t* offsets, const uint32_t* lengths,
                                                  const int32_t* widths, const int32_t* heights, int32_t n, int32_t samples,
                                                  int32_t bits, uint8_t* d_dst, const uint64_t* dst_offsets, int32_t* status) {
    return omr_j2k_decode_batch_device_ex(ctx, src, offsets, lengths, widths, heights, n, samples, bits, 0u, d_dst, dst_offsets, status);
}

extern "C" omr_status omr_j2k_decode_batch_device_ex(omr_ctx* ctx, const uint8_t* src, const uint64_t* offsets, const uint32_t* lengths,
                                                     const int32_t* widths, const int32_t* heights, int32_t n, int32_t samples,
                                                     int32_t bits, uint32_t flags, uint8_t* d_dst, const uint64_t* dst_offsets,
                                                     int32_t* status) {
    if (!ctx) return OMR_INVALID_ARGUMENT;
    if (flags & ~OMR_J2K_ALLOW_IRREVERSIBLE) return fail(ctx, OMR_INVALID_ARGUMENT, "j2k: unknown flags");
    const uint32_t kinds = kJ2kTakeReversible | (flags ? kJ2kTakeIrreversible : 0u);
    if (n < 0) return fail(ctx, OMR_INVALID_ARGUMENT, "j2k: negative stream count");
    if (n == 0) return OMR_OK;
    if (!src || !offsets || !lengths || !widths || !heights || !d_dst || !dst_offsets || !status)
        return fail(ctx, OMR_INVALID_ARGUMENT, "j2k: null argument");
    if (samples != 1 && samples != 3) return fail(ctx, OMR_INVALID_ARGUMENT, "j2k: samples must be 1 or 3");
    if (bits != 8 && bits != 16) return fail(ctx, OMR_INVALID_ARGUMENT, "j2k: bits must be 8 or 16");
    OMR_HIP(ctx, hipSetDevice(ctx->device));
    SegPipe* T = seg_pipe(ctx, SegKind::tiff);
    std::vector<CodecJob> jobs((size_t)n);
    std::vector<J2kPlan> plans((size_t)n);
    for (int32_t k = 0; k < n; ++k) {
        CodecJob& J = jobs[(size_t)k];
        J.dst_off = dst_offsets[k];
        if (!j2k_sizes_ok(widths[k], heights[k], samples, bits) || (bits == 16 && (dst_offsets[k] & 1u))) {
            J.parsed = OMR_INVALID_ARGUMENT;
            continue;
        }
        J.parsed = j2k_prepare(src + offsets[k], lengths[k], widths[k], heights[k], samples, bits, plans[(size_t)k], nullptr, kinds);
    }
    return decode_batch_staged(ctx, T, "j2k", jobs, src, offsets, lengths, [&](std::vector<int32_t>& stv) {
        return j2k_decode_group(ctx, T, jobs, plans, false, static_cast<const uint8_t*>(T->d_in), d_dst, stv);
    }, status);
}
