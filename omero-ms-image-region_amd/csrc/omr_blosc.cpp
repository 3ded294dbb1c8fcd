// omr_blosc.cpp — K15, host half: the Blosc 1 container and the LZ4 block format as the OME-Zarr
// reader takes them (include/omr/omr.h).  A plain serial LZ4 decoder (omr_lz4_decode_host), the
// container parser that both routes share (blosc_parse: the host route decodes what it lists, the
// device route uploads the list as K15a's stream table) and omr_blosc_decode_host.  Chunk files are
// user-uploaded data: every read is behind a check against the file's length and every write
// behind one against the chunk's size.  Nothing links liblz4 or Blosc; the container layout is as
// recalled, not pinned against c-blosc.
#include "omr_internal.h"

namespace omr {

bool lz4_decode(const uint8_t* s, size_t len, uint8_t* d, size_t expected) {
    size_t ip = 0, op = 0;
    for (;;) {
        if (ip >= len) return false;                       // empty, or the input ends after a match
        const uint32_t token = s[ip++];
        size_t lit = token >> 4;
        if (lit == 15) {
            uint32_t b;
            do {
                if (ip >= len) return false;
                b = s[ip++];
                lit += b;
            } while (b == 255);
        }
        if (lit > len - ip || lit > expected - op) return false;
        if (lit) std::memcpy(d + op, s + ip, lit);
        ip += lit;
        op += lit;
        if (ip == len) return op == expected;              // the last sequence: literals only
        if (len - ip < 2) return false;
        const size_t offset = (size_t)s[ip] | (size_t)s[ip + 1] << 8;
        ip += 2;
        if (offset == 0 || offset > op) return false;
        size_t n = (token & 15u) + 4u;
        if ((token & 15u) == 15u) {
            uint32_t b;
            do {
                if (ip >= len) return false;
                b = s[ip++];
                n += b;
            } while (b == 255);
        }
        if (n > expected - op) return false;
        for (size_t k = 0; k < n; ++k, ++op) d[op] = d[op - offset];
    }
}

namespace {

inline int64_t le32(const uint8_t* p) {
    return (int32_t)((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24);
}

}  // namespace

bool blosc_parse(const uint8_t* p, size_t len, size_t expected, BloscLayout& out, uint32_t inner) {
    out = BloscLayout();
    if (len < 16 || len > 0x7FFFFFFFu || expected > 0x7FFFFFFFu) return false;
    const uint32_t flags = p[2];
    const int64_t nbytes = le32(p + 4), blocksize = le32(p + 8), cbytes = le32(p + 12);
    const uint32_t format = flags >> 5;
    const bool known = (format == 1u && (inner & OMR_BLOSC_INNER_LZ4)) || (format == 4u && (inner & OMR_BLOSC_INNER_ZSTD));
    if (p[0] != 2 || (flags & 0x04u) || !known) return false;
    out.format = format;
    if (p[3] < 1 || nbytes != (int64_t)expected || cbytes != (int64_t)len || blocksize <= 0 || blocksize > nbytes)
        return false;
    out.nbytes = (uint32_t)nbytes;
    out.blocksize = (uint32_t)blocksize;
    out.typesize = p[3];
    if (flags & 0x02u) {
        if (cbytes != nbytes + 16) return false;
        out.memcpyed = true;
        return true;
    }
    out.shuffled = (flags & 0x01u) && out.typesize > 1;
    const int64_t nblocks = (nbytes + blocksize - 1) / blocksize;
    const int64_t table_end = 16 + 4 * nblocks;
    if (table_end > (int64_t)len || nblocks > (int64_t)kMaxBloscStreams) return false;
    const int64_t ts = out.typesize;
    const bool may_split = !(flags & 0x10u) && ts <= 16 && blocksize / ts >= 128;
    // bstarts need not ascend (a threaded writer may place blocks as they finish), but blocks that
    // alias one another must not multiply the work: the streams listed, each with its csize word, may
    // not add up to more than the bytes behind the table
    int64_t budget = (int64_t)len - table_end;
    out.streams.reserve((size_t)std::min<int64_t>(nblocks * (may_split ? ts : 1), budget / 5));
    for (int64_t b = 0; b < nblocks; ++b) {
        const bool leftover = b == nblocks - 1 && nbytes % blocksize != 0;
        const int64_t nb = leftover ? nbytes % blocksize : blocksize;
        const bool split = may_split && !leftover;
        if (split && blocksize % ts != 0) return false;
        const int64_t nsplits = split ? ts : 1, neblock = nb / nsplits;
        int64_t at = le32(p + 16 + 4 * b);
        if (at < table_end || at > (int64_t)len) return false;
        if (out.streams.size() + (size_t)nsplits > kMaxBloscStreams) return false;
        for (int64_t k = 0; k < nsplits; ++k) {
            if ((int64_t)len - at < 4) return false;
            const int64_t csize = le32(p + at);
            at += 4;
            if (csize <= 0 || csize > neblock || csize > (int64_t)len - at) return false;
            budget -= 4 + csize;
            if (budget < 0) return false;
            BloscStream s;
            s.src_off = (uint32_t)at;
            s.csize = (uint32_t)csize;
            s.dst_off = (uint32_t)(b * blocksize + k * neblock);
            s.neblock = (uint32_t)neblock;
            s.raw = csize == neblock;
            out.streams.push_back(s);
            at += csize;
        }
    }
    return true;
}

namespace {

// dst (decoded order) from src (shuffled per block), both nbytes long.
void unshuffle(const BloscLayout& L, const uint8_t* src, uint8_t* dst) {
    const size_t ts = L.typesize;
    for (size_t b0 = 0; b0 < L.nbytes; b0 += L.blocksize) {
        const size_t nb = std::min<size_t>(L.blocksize, L.nbytes - b0), q = nb / ts;
        const uint8_t* s = src + b0;
        uint8_t* d = dst + b0;
        for (size_t j = 0; j < ts; ++j)
            for (size_t i = 0; i < q; ++i) d[i * ts + j] = s[j * q + i];
        for (size_t k = q * ts; k < nb; ++k) d[k] = s[k];
    }
}

bool blosc_decode(const uint8_t* p, size_t len, uint8_t* d, size_t expected, uint32_t inner) {
    BloscLayout L;
    if (!blosc_parse(p, len, expected, L, inner)) return false;
    if (L.memcpyed) {
        std::memcpy(d, p + 16, expected);                  // cbytes == nbytes + 16 == len: checked
        return true;
    }
    std::vector<uint8_t> tmp;
    uint8_t* to = d;
    if (L.shuffled) {
        tmp.resize(expected);
        to = tmp.data();
    }
    for (const BloscStream& s : L.streams) {               // src_off + csize <= len, dst_off + neblock <= nbytes
        if (s.raw) std::memcpy(to + s.dst_off, p + s.src_off, s.neblock);
        else if (!(L.format == 4u ? zstd_decode : lz4_decode)(p + s.src_off, s.csize, to + s.dst_off, s.neblock)) return false;
    }
    if (L.shuffled) unshuffle(L, tmp.data(), d);
    return true;
}

}  // namespace
}  // namespace omr

extern "C" {

omr_status omr_lz4_decode_host(const uint8_t* src, size_t length, uint8_t* dst, size_t expected) {
    if ((!src && length) || (!dst && expected)) return OMR_INVALID_ARGUMENT;
    return omr::lz4_decode(src, length, dst, expected) ? OMR_OK : OMR_INTERNAL;
}

omr_status omr_blosc_decode_host(const uint8_t* src, size_t length, uint8_t* dst, size_t expected) {
    if ((!src && length) || (!dst && expected)) return OMR_INVALID_ARGUMENT;
    return omr::blosc_decode(src, length, dst, expected, OMR_BLOSC_INNER_LZ4) ? OMR_OK : OMR_INTERNAL;
}

omr_status omr_blosc_decode_host_ex(const uint8_t* src, size_t length, uint8_t* dst, size_t expected, uint32_t inner) {
    if ((!src && length) || (!dst && expected)) return OMR_INVALID_ARGUMENT;
    if (!inner || (inner & ~(OMR_BLOSC_INNER_LZ4 | OMR_BLOSC_INNER_ZSTD))) return OMR_INVALID_ARGUMENT;
    return omr::blosc_decode(src, length, dst, expected, inner) ? OMR_OK : OMR_INTERNAL;
}

}  // extern "C"
