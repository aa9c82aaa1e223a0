// Stand-alone check of the frame index's host code (csrc/s3hc_index.cpp alone, no HIP): built
// and run by tests/test_index.py under the address and undefined-behaviour sanitizers.
// Entries and offsets, span lookup against a linear scan, the side-car round trip, and the
// corruption loop: every single-bit flip, every truncation, a trailing byte and a forged count
// must load as S3HC_CORRUPT (and touch no memory they should not).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "s3hc_lz4.h"

static int fails = 0;
#define CHECK(c)                                              \
    do {                                                      \
        if (!(c)) {                                           \
            printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
            ++fails;                                          \
        }                                                     \
    } while (0)

static uint32_t rnd_state = 12345;
static uint32_t rnd() {
    rnd_state = rnd_state * 1664525u + 1013904223u;
    return rnd_state >> 8;
}

// load must fail with S3HC_CORRUPT and leave no index behind; the blob is an exact-size heap
// copy so a read past it is a sanitizer report
static void expect_corrupt(const std::vector<uint8_t>& b) {
    std::vector<uint8_t> exact(b);
    s3hc_index* x = (s3hc_index*)1;
    const int rc = s3hc_index_load(exact.data(), exact.size(), &x);
    CHECK(rc == S3HC_CORRUPT);
    CHECK(x == nullptr);
    if (rc == S3HC_OK) s3hc_index_free(x);
}

int main() {
    // entries and offsets
    const uint32_t c[3] = {10, 70000, 33}, u[3] = {100, 65536, 1};
    s3hc_index* idx = nullptr;
    CHECK(s3hc_index_from_entries(c, u, 3, &idx) == S3HC_OK && idx);
    CHECK(s3hc_index_count(idx) == 3);
    uint64_t e[4], ct, ut;
    CHECK(s3hc_index_entry(idx, 2, e) == S3HC_OK && e[0] == 70010 && e[1] == 65636 && e[2] == 33 && e[3] == 1);
    CHECK(s3hc_index_entry(idx, 3, e) == S3HC_INVALID_ARG);
    CHECK(s3hc_index_total(idx, &ct, &ut) == S3HC_OK && ct == 70043 && ut == 65637);
    {
        s3hc_index* z = nullptr;
        const uint32_t zc[2] = {5, 0};
        CHECK(s3hc_index_from_entries(zc, u, 2, &z) == S3HC_INVALID_ARG && z == nullptr);
        CHECK(s3hc_index_from_entries(nullptr, nullptr, 0, &z) == S3HC_OK && z && s3hc_index_count(z) == 0);
        uint32_t f, k;
        uint64_t o, n;
        CHECK(s3hc_index_span(z, 0, 0, &f, &k, &o, &n) == S3HC_OK && k == 0);
        CHECK(s3hc_index_span(z, 0, 1, &f, &k, &o, &n) == S3HC_INVALID_ARG);
        s3hc_index_free(z);
    }
    // span lookup against a linear scan
    static const uint32_t sizes[5] = {1, 7, 65536, 65537, 1u << 20};
    for (int it = 0; it < 200; ++it) {
        const uint32_t n = 1 + rnd() % 50;
        std::vector<uint32_t> cl(n), ul(n);
        for (uint32_t i = 0; i < n; ++i) {
            cl[i] = sizes[rnd() % 5];
            ul[i] = sizes[rnd() % 5];
        }
        s3hc_index* r = nullptr;
        CHECK(s3hc_index_from_entries(cl.data(), ul.data(), n, &r) == S3HC_OK);
        uint64_t tc, tu;
        s3hc_index_total(r, &tc, &tu);
        for (int q = 0; q < 40; ++q) {
            uint64_t lo = (uint64_t)rnd() * 977 % (tu + 1), hi = (uint64_t)rnd() * 991 % (tu + 1);
            if (q == 0) { lo = 0; hi = tu; }
            if (lo > hi) { const uint64_t t = lo; lo = hi; hi = t; }
            uint32_t f, k;
            uint64_t o, len;
            CHECK(s3hc_index_span(r, lo, hi, &f, &k, &o, &len) == S3HC_OK);
            uint32_t bf = 0, bk = 0;
            uint64_t bo = 0, bl = 0, cu = 0, cc = 0;
            for (uint32_t i = 0; i < n; ++i) {
                if (cu < hi && cu + ul[i] > lo) {
                    if (!bk) { bf = i; bo = cc; }
                    ++bk;
                    bl += cl[i];
                }
                cu += ul[i];
                cc += cl[i];
            }
            if (lo == hi) CHECK(k == 0);
            else CHECK(f == bf && k == bk && o == bo && len == bl);
        }
        uint32_t f, k;
        uint64_t o, len;
        CHECK(s3hc_index_span(r, 0, tu + 1, &f, &k, &o, &len) == S3HC_INVALID_ARG);
        CHECK(s3hc_index_span(r, 1, 0, &f, &k, &o, &len) == S3HC_INVALID_ARG);
        s3hc_index_free(r);
    }
    // side-car round trip
    std::vector<uint8_t> blob(s3hc_index_serialized_size(idx));
    size_t bn = 0;
    CHECK(s3hc_index_serialize(idx, blob.data(), blob.size() - 1, &bn) == S3HC_DST_TOO_SMALL);
    CHECK(s3hc_index_serialize(idx, blob.data(), blob.size(), &bn) == S3HC_OK && bn == blob.size() && bn == 16 + 8 * 3);
    {
        s3hc_index* back = nullptr;
        CHECK(s3hc_index_load(blob.data(), blob.size(), &back) == S3HC_OK && back);
        CHECK(s3hc_index_count(back) == 3);
        for (uint32_t i = 0; i < 3; ++i) {
            uint64_t a[4], b[4];
            s3hc_index_entry(idx, i, a);
            s3hc_index_entry(back, i, b);
            CHECK(memcmp(a, b, sizeof a) == 0);
        }
        s3hc_index_free(back);
    }
    // corruption loop
    for (size_t bit = 0; bit < 8 * blob.size(); ++bit) {
        std::vector<uint8_t> b(blob);
        b[bit / 8] ^= (uint8_t)(1u << (bit % 8));
        expect_corrupt(b);
    }
    for (size_t len = 0; len < blob.size(); ++len) expect_corrupt(std::vector<uint8_t>(blob.begin(), blob.begin() + len));
    {
        std::vector<uint8_t> b(blob);
        b.push_back(0);
        expect_corrupt(b);
        b = blob;
        memset(b.data() + 8, 0xFF, 4);  // count 0xFFFFFFFF
        expect_corrupt(b);
    }
    s3hc_index_free(idx);
    if (fails) return 1;
    printf("index ok\n");
    return 0;
}
