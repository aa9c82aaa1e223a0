// s3hc_index.cpp — the frame index of a range file: entries, span lookup and the side-car format
// (INTEGRATION.md "Seek index"). Pure host code with no HIP include: tests/cpu
// compiles this file alone under the address and undefined-behaviour sanitizers.
//
// Side-car layout (little-endian):
//   bytes 0-6   "S3HCIDX"
//   byte  7     format version (1)
//   u32         entry count n
//   n x {u32 c_len, u32 u_len}
//   u32         xxh32 (seed 0) of every byte before it
#include "s3hc_index.hpp"

#include <string.h>

#include <algorithm>
#include <new>

#include "s3hc_lz4.h"

namespace {
constexpr uint8_t kIdxMagic[7] = {'S', '3', 'H', 'C', 'I', 'D', 'X'};
constexpr uint8_t kIdxVersion = 1;
constexpr size_t kIdxFixed = 8 + 4 + 4;  // magic + version, count, checksum

inline uint32_t ld32(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
inline void st32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)v;
    p[1] = (uint8_t)(v >> 8);
    p[2] = (uint8_t)(v >> 16);
    p[3] = (uint8_t)(v >> 24);
}
inline uint32_t rotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

uint32_t xxh32(const uint8_t* p, size_t n) {
    constexpr uint32_t P1 = 2654435761u, P2 = 2246822519u, P3 = 3266489917u, P4 = 668265263u, P5 = 374761393u;
    const uint8_t* const end = p + n;
    uint32_t h;
    if (n >= 16) {
        uint32_t v1 = P1 + P2, v2 = P2, v3 = 0, v4 = 0u - P1;
        do {
            v1 = rotl(v1 + ld32(p) * P2, 13) * P1;
            v2 = rotl(v2 + ld32(p + 4) * P2, 13) * P1;
            v3 = rotl(v3 + ld32(p + 8) * P2, 13) * P1;
            v4 = rotl(v4 + ld32(p + 12) * P2, 13) * P1;
            p += 16;
        } while (end - p >= 16);
        h = rotl(v1, 1) + rotl(v2, 7) + rotl(v3, 12) + rotl(v4, 18);
    } else {
        h = P5;
    }
    h += (uint32_t)n;
    for (; end - p >= 4; p += 4) h = rotl(h + ld32(p) * P3, 17) * P4;
    for (; p < end; ++p) h = rotl(h + *p * P5, 11) * P1;
    h ^= h >> 15;
    h *= P2;
    h ^= h >> 13;
    h *= P3;
    h ^= h >> 16;
    return h;
}
}  // namespace

s3hc_index* s3hc::index_make(const uint32_t* c_len, const uint32_t* u_len, uint32_t n, int* rc) {
    s3hc_index* I = new (std::nothrow) s3hc_index;
    if (!I) {
        *rc = S3HC_NO_MEMORY;
        return nullptr;
    }
    try {
        I->c_len.assign(c_len, c_len + n);
        I->u_len.assign(u_len, u_len + n);
        I->c_off.resize((size_t)n + 1);
        I->u_off.resize((size_t)n + 1);
    } catch (const std::bad_alloc&) {
        delete I;
        *rc = S3HC_NO_MEMORY;
        return nullptr;
    }
    uint64_t c = 0, u = 0;
    for (uint32_t i = 0; i < n; ++i) {
        I->c_off[i] = c;
        I->u_off[i] = u;
        if (c_len[i] == 0 || c + c_len[i] < c || u + u_len[i] < u) {
            delete I;
            *rc = S3HC_INVALID_ARG;
            return nullptr;
        }
        c += c_len[i];
        u += u_len[i];
    }
    I->c_off[n] = c;
    I->u_off[n] = u;
    *rc = S3HC_OK;
    return I;
}

extern "C" int s3hc_index_from_entries(const uint32_t* c_len, const uint32_t* u_len, uint32_t n, s3hc_index** out) {
    if (!out || (n && (!c_len || !u_len))) return S3HC_INVALID_ARG;
    int rc;
    *out = s3hc::index_make(c_len, u_len, n, &rc);
    return rc;
}

extern "C" void s3hc_index_free(s3hc_index* idx) { delete idx; }

extern "C" uint32_t s3hc_index_count(const s3hc_index* idx) { return idx ? (uint32_t)idx->c_len.size() : 0; }

extern "C" int s3hc_index_entry(const s3hc_index* idx, uint32_t i, uint64_t out[4]) {
    if (!idx || !out || i >= idx->c_len.size()) return S3HC_INVALID_ARG;
    out[0] = idx->c_off[i];
    out[1] = idx->u_off[i];
    out[2] = idx->c_len[i];
    out[3] = idx->u_len[i];
    return S3HC_OK;
}

extern "C" int s3hc_index_total(const s3hc_index* idx, uint64_t* c_total, uint64_t* u_total) {
    if (!idx) return S3HC_INVALID_ARG;
    if (c_total) *c_total = idx->c_off.back();
    if (u_total) *u_total = idx->u_off.back();
    return S3HC_OK;
}

extern "C" int s3hc_index_span(const s3hc_index* idx, uint64_t lo, uint64_t hi, uint32_t* first, uint32_t* count,
                               uint64_t* c_off, uint64_t* c_len) {
    if (!idx || !first || !count || !c_off || !c_len || lo > hi || hi > idx->u_off.back()) return S3HC_INVALID_ARG;
    *first = 0;
    *count = 0;
    *c_off = 0;
    *c_len = 0;
    if (lo == hi) return S3HC_OK;
    // the frame holding byte lo: the last one that starts at or before it; the frames end with
    // the first one that starts at or after hi (u_off has the total as its last entry)
    const auto b = idx->u_off.begin(), e = idx->u_off.end();
    const size_t f = (size_t)(std::upper_bound(b, e, lo) - b) - 1;
    const size_t l = (size_t)(std::lower_bound(b, e, hi) - b);
    *first = (uint32_t)f;
    *count = (uint32_t)(l - f);
    *c_off = idx->c_off[f];
    *c_len = idx->c_off[l] - idx->c_off[f];
    return S3HC_OK;
}

extern "C" size_t s3hc_index_serialized_size(const s3hc_index* idx) {
    return idx ? kIdxFixed + 8 * idx->c_len.size() : 0;
}

extern "C" int s3hc_index_serialize(const s3hc_index* idx, uint8_t* dst, size_t cap, size_t* n) {
    if (!idx || !dst || !n) return S3HC_INVALID_ARG;
    const size_t need = s3hc_index_serialized_size(idx);
    if (cap < need) return S3HC_DST_TOO_SMALL;
    memcpy(dst, kIdxMagic, 7);
    dst[7] = kIdxVersion;
    const uint32_t cnt = (uint32_t)idx->c_len.size();
    st32(dst + 8, cnt);
    for (uint32_t i = 0; i < cnt; ++i) {
        st32(dst + 12 + 8 * (size_t)i, idx->c_len[i]);
        st32(dst + 16 + 8 * (size_t)i, idx->u_len[i]);
    }
    st32(dst + need - 4, xxh32(dst, need - 4));
    *n = need;
    return S3HC_OK;
}

extern "C" int s3hc_index_load(const uint8_t* src, size_t n, s3hc_index** out) {
    if (!out || (!src && n)) return S3HC_INVALID_ARG;
    *out = nullptr;
    if (n < kIdxFixed || memcmp(src, kIdxMagic, 7) != 0 || src[7] != kIdxVersion) return S3HC_CORRUPT;
    const uint32_t cnt = ld32(src + 8);
    // the count must account for every byte of the blob (checked before anything is sized by it)
    if ((n - kIdxFixed) % 8 != 0 || (n - kIdxFixed) / 8 != cnt) return S3HC_CORRUPT;
    if (ld32(src + n - 4) != xxh32(src, n - 4)) return S3HC_CORRUPT;
    std::vector<uint32_t> c, u;
    try {
        c.resize(cnt);
        u.resize(cnt);
    } catch (const std::bad_alloc&) {
        return S3HC_NO_MEMORY;
    }
    for (uint32_t i = 0; i < cnt; ++i) {
        c[i] = ld32(src + 12 + 8 * (size_t)i);
        u[i] = ld32(src + 16 + 8 * (size_t)i);
    }
    int rc;
    *out = s3hc::index_make(c.data(), u.data(), cnt, &rc);
    return rc == S3HC_INVALID_ARG ? S3HC_CORRUPT : rc;
}
