// s3hc_index.hpp — the frame index of one range file: host data only, no HIP.
#pragma once
#include <stdint.h>

#include <vector>

struct s3hc_index {
    std::vector<uint32_t> c_len, u_len;  // per frame: framed bytes, decoded bytes
    std::vector<uint64_t> c_off, u_off;  // exclusive prefix sums, n + 1 entries (the last = the totals)
};

namespace s3hc {
// A new index over n frames (nullptr: a zero c_len, an offset overflow or no memory; *rc says which).
s3hc_index* index_make(const uint32_t* c_len, const uint32_t* u_len, uint32_t n, int* rc);
}  // namespace s3hc
