// s3hc_index.hip — the frame size scan: the decoded length of every frame of a
// launch, from the frames' token chains alone. No decoded byte is written and no token or
// sequence record leaves the workgroup; a launch stores two words per frame.
//
// A frame's decoded length is the sum of its blocks' (lz4_flex FrameDecoder, compression.rs:479-480);
// a stored block is its own length, a compressed block the sum of its sequences' literal and match
// lengths. That sum needs the token chain (token, literal-length run, literals, offset,
// match-length run, next token) but neither history nor output, so linked blocks, block checksums
// and content-size fields change nothing.
//
// One 256-thread workgroup per frame walks the frame's header and block words (every thread the
// same bytes) and scans its compressed blocks in chunks of 256 segments of 64 compressed bytes,
// staged in LDS (a walk's hops are dependent loads: LDS latency, not L2's; bytes of a token that
// reaches past the staged chunk come from global memory):
//   walk 1   thread g walks the token chain from the first byte of segment g as if a token began
//            there, to the segment's end, marking the positions it visits in a 64-bit mask (one
//            per segment, in LDS). Thread 0 starts at the chunk's true entry instead.
//   walk 2   it keeps walking until it lands on a position a later segment's walk marked (a chain
//            is a function of its position, so from there on the two walks are one), or leaves
//            the chunk, or the block ends.
//   chain    those "merged into" links form a list over the segments; the segments reachable
//            from segment 0 (pointer doubling, 8 steps) are the ones the true chain runs through,
//            and each learns its first true token from its predecessor.
//   sum      every segment on the chain walks from its first true token to its merge point,
//            adding literal and match lengths; one LDS add per segment.
// The last segment of the chain hands the next chunk its entry (the chunk starts at the segment
// holding it), or ends the block. Every walk moves forward and stops at the block's last byte, no
// walk waits for another workgroup, and no load leaves [frame_off, frame_off + frame_len).
//
// The same k_dtok / k_lbt_walk idea (s3hc_fast.hip, s3hc_lb.hip) without their bitmaps in global
// memory and record tables: those kernels are not touched, their generated code is the same.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "s3hc_lz4.h"
#include "s3hc_plan.hpp"

namespace s3hc {
namespace {
constexpr uint32_t kT = 256;             // threads = segments per chunk
constexpr uint32_t kLv = 8;              // log2(kT): doubling steps
constexpr uint32_t kSegB = 64;           // compressed bytes per segment (one mask word)
constexpr uint32_t kChunk = kT * kSegB;  // 16 KiB
constexpr uint32_t END = 0xFFFFFFFEu;    // the chain ended with the block's last sequence
constexpr uint32_t BAD = 0xFFFFFFFFu;    // malformed token
constexpr uint32_t kNone = 0xFFFFFFFFu;

typedef uint64_t __attribute__((aligned(1))) u64u;
typedef uint4 __attribute__((aligned(1))) uint4u;

__device__ __forceinline__ uint32_t rd32(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
__device__ __forceinline__ uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
// xxh32 (seed 0) of n < 16 bytes: the frame descriptor
__device__ uint32_t xxh32_small(const uint8_t* p, uint32_t n) {
    constexpr uint32_t P1 = 2654435761u, P2 = 2246822519u, P3 = 3266489917u, P4 = 668265263u, P5 = 374761393u;
    uint32_t h = P5 + n, t = 0;
    for (; t + 4 <= n; t += 4) h = rotl32(h + rd32(p + t) * P3, 17) * P4;
    for (; t < n; ++t) h = rotl32(h + (uint32_t)p[t] * P5, 11) * P1;
    h ^= h >> 15;
    h *= P2;
    h ^= h >> 13;
    h *= P3;
    h ^= h >> 16;
    return h;
}

// The compressed block as the walks read it: the chunk in hand from its LDS copy, bytes past the
// copy (a token, its literals or a length run reaching over the chunk's end) from global memory.
struct Src {
    const uint8_t* in;  // the block
    const uint8_t* st;  // LDS copy of block bytes [c0, c0 + nst)
    uint32_t c0, nst;
    __device__ __forceinline__ uint32_t operator[](uint32_t p) const {
        const uint32_t r = p - c0;
        return r < nst ? st[r] : in[p];
    }
    // block bytes [p, p + 8) are all 255 (the caller keeps p + 8 inside the block)
    __device__ __forceinline__ bool all255x8(uint32_t p) const {
        const uint32_t r = p - c0;
        return (r + 8u <= nst ? *(const u64u*)(st + r) : *(const u64u*)(in + p)) == ~0ull;
    }
};

// A length-extension run at block byte q (the nibble was 15): its sum; q moves past it, or to
// C + 1 when the run reaches the block's end. Runs of 255 are taken eight bytes at a time while
// eight bytes of the block remain.
__device__ __forceinline__ uint32_t ext_run(const Src& in, uint32_t& q, uint32_t C) {
    uint32_t acc = 0;
    for (;;) {
        if (q >= C) {
            q = C + 1u;
            return acc;
        }
        if (C - q >= 8u && in.all255x8(q)) {
            acc += 8u * 255u;
            q += 8u;
            continue;
        }
        const uint32_t e = in[q];
        ++q;
        acc += e;
        if (e != 255u) return acc;
    }
}

// The token at block byte p < C (lz4_flex decompress_internal's parse): the next token's position,
// END or BAD; *len = the sequence's literal + match bytes (0 when BAD). A block ends right after a
// literal run; a run, literals or an offset reaching past the end, or no token after a match, are
// malformed. Lengths fit 32 bits: a run adds less than 255 per byte of a block of <= 4 MiB.
__device__ __forceinline__ uint32_t hop(const Src& in, uint32_t p, uint32_t C, uint32_t* len) {
    *len = 0;
    const uint32_t t = in[p];
    uint32_t L = t >> 4, q = p + 1u;
    if (L == 15u) L += ext_run(in, q, C);
    if (q > C || L > C - q) return BAD;
    const uint32_t mp = q + L;
    if (mp == C) {
        *len = L;
        return END;
    }
    if (C - mp < 2u) return BAD;
    uint32_t M = (t & 15u) + 4u, q2 = mp + 2u;
    if ((t & 15u) == 15u) M += ext_run(in, q2, C);
    if (q2 >= C) return BAD;
    *len = L + M;
    return q2;
}

constexpr uint32_t kStagePad = 64;  // bytes staged past the chunk: most tokens that straddle its end
struct ScanLds {
    __attribute__((aligned(16))) uint8_t stage[kChunk + kStagePad];  // the chunk's compressed bytes
    uint64_t mask[kT];        // walk-1 marks of each segment
    uint32_t vfrom[kT];       // per segment on the chain: its first true token
    uint16_t J[2][kT + 2];    // succ^(2^k) per segment, ping-pong; kT = the terminal
    uint8_t reach[kT + 2];    // segment is on the true chain
    uint32_t next;            // the chain's position after the chunk, END or BAD
    unsigned long long sum;   // decoded bytes of the block so far
};

// Decoded bytes of the compressed block in[0, C), 1 <= C <= 4 MiB (workgroup-uniform arguments and
// result); false: the chain is malformed.
__device__ bool scan_block(const uint8_t* __restrict__ blk, const uint32_t C, ScanLds& S, uint64_t* total) {
    const uint32_t g = threadIdx.x;
    __syncthreads();  // (the previous block's readers of S are done)
    if (g == 0) S.sum = 0ull;
    uint32_t e = 0;  // the true chain's position
    for (;;) {
        const uint32_t c0 = e & ~(kSegB - 1u);
        const uint32_t c1 = C - c0 > kChunk ? c0 + kChunk : C;
        const uint32_t s0 = c0 + g * kSegB;
        const uint32_t s1 = s0 + kSegB < c1 ? s0 + kSegB : c1;
        uint32_t len;
        // ---- stage block bytes [c0, c0 + nst): 16 bytes per thread and step, the tail bytewise
        // (the previous chunk's walks ended at the barrier before its S.next was read)
        const uint32_t nst = C - c0 > kChunk + kStagePad ? kChunk + kStagePad : C - c0;
        for (uint32_t i = g * 16u; i < nst; i += kT * 16u) {
            if (nst - i >= 16u) {
                *(uint4*)(S.stage + i) = *(const uint4u*)(blk + c0 + i);
            } else {
                for (uint32_t k = i; k < nst; ++k) S.stage[k] = blk[c0 + k];
            }
        }
        __syncthreads();
        const Src in{blk, S.stage, c0, nst};
        // ---- walk 1
        uint64_t mk = 0;
        uint32_t p = BAD;
        if (s0 < c1) {
            p = g == 0 ? e : s0;
            while (p < s1) {
                mk |= 1ull << (p - s0);
                p = hop(in, p, C, &len);
            }
        }
        S.mask[g] = mk;
        S.vfrom[g] = kNone;
        S.reach[g] = g == 0 ? 1 : 0;
        if (g == 0) {
            S.J[0][kT] = S.J[1][kT] = (uint16_t)kT;
            S.reach[kT] = 0;
        }
        __syncthreads();
        // ---- walk 2: on to a marked position of a later segment, or out of the chunk
        uint32_t m = p;
        while (m < c1) {
            const uint32_t r = m - c0;
            if ((S.mask[r >> 6] >> (r & 63u)) & 1ull) break;
            m = hop(in, m, C, &len);
        }
        S.J[0][g] = (uint16_t)(m < c1 ? (m - c0) >> 6 : kT);
        __syncthreads();
        // ---- the true chain: segment 0, the segment its walk merged into, ... (after step k every
        // segment within 2^(k+1) links of segment 0 is marked)
#pragma unroll
        for (uint32_t k = 0; k < kLv; ++k) {
            const uint32_t h = S.J[k & 1][g];
            if (S.reach[g]) S.reach[h] = 1;
            S.J[(k + 1) & 1][g] = S.J[k & 1][h];
            __syncthreads();
        }
        if (S.reach[g]) {
            if (m < c1) S.vfrom[(m - c0) >> 6] = m;
            else S.next = m;  // (the chain's last segment of this chunk: exactly one)
        }
        __syncthreads();
        // ---- sum: from my first true token to my merge point
        const uint32_t vf = g == 0 ? e : S.vfrom[g];
        if (vf != kNone) {
            uint64_t s = 0;
            uint32_t q = vf;
            while (q != m && q < C) {
                q = hop(in, q, C, &len);
                s += len;
            }
            atomicAdd(&S.sum, (unsigned long long)s);
        }
        __syncthreads();
        const uint32_t nx = S.next;
        if (nx >= END) {
            *total = S.sum;
            return nx == END;
        }
        e = nx;
    }
}

// The frame f[0, avail): FrameInfo::read and FrameDecoder::read_more's structure rules as the
// decoders apply them (k_dframe_count: one frame per entry, no trailing bytes), the blocks' sizes
// from scan_block. Workgroup-uniform.
__device__ int scan_frame(const uint8_t* __restrict__ f, const uint32_t avail, ScanLds& S, uint64_t* out) {
    *out = 0;
    if (avail < 4u) return S3HC_CORRUPT;
    const uint32_t magic = rd32(f);
    if (magic == 0x184C2102u || (magic & 0xFFFFFFF0u) == 0x184D2A50u) return S3HC_UNSUPPORTED;
    if (magic != kMagic || avail < 7u) return S3HC_CORRUPT;
    const uint32_t flg = f[4], bd = f[5];
    const uint32_t need = 7u + ((flg & 0x08u) ? 8u : 0u) + ((flg & 0x01u) ? 4u : 0u);
    if (avail < need || (flg & 0xC0u) != 0x40u || (flg & 0x02u) || (bd & 0x8Fu)) return S3HC_CORRUPT;
    const uint32_t code = (bd >> 4) & 7u;
    if (code < 4u) return S3HC_CORRUPT;
    const uint32_t bmax = 1u << (16u + 2u * (code - 4u));
    if (((xxh32_small(f + 4, need - 5u) >> 8) & 0xFFu) != f[need - 1u]) return S3HC_CORRUPT;
    if (flg & 0x01u) return S3HC_UNSUPPORTED;
    const uint32_t cs = (flg & 0x10u) ? 4u : 0u;
    uint64_t tot = 0;
    uint32_t ip = need;
    for (;;) {
        if (avail - ip < 4u) return S3HC_CORRUPT;
        const uint32_t w = rd32(f + ip);
        ip += 4u;
        if (w == 0u) {
            if (flg & 0x04u) {
                if (avail - ip < 4u) return S3HC_CORRUPT;
                ip += 4u;
            }
            break;
        }
        const uint32_t len = w & 0x7FFFFFFFu;
        if (len > bmax || avail - ip < len + cs) return S3HC_CORRUPT;
        if (w & kStoredBit) {
            tot += len;
        } else {
            uint64_t bt;
            if (!scan_block(f + ip, len, S, &bt) || bt > bmax) return S3HC_CORRUPT;
            tot += bt;
        }
        ip += len + cs;
    }
    if (ip != avail) return S3HC_CORRUPT;
    if ((flg & 0x08u) && (rd32(f + 6) | ((uint64_t)rd32(f + 10) << 32)) != tot) return S3HC_CORRUPT;
    if (tot > 0xFFFFFFFFull) return S3HC_CORRUPT;
    *out = tot;
    return S3HC_OK;
}

__global__ __launch_bounds__(kT) void k_frame_sizes(const uint8_t* __restrict__ src,
                                                    const uint64_t* __restrict__ frame_off,
                                                    const uint32_t* __restrict__ frame_len, uint32_t nframes,
                                                    uint32_t* __restrict__ u_len, int32_t* __restrict__ status) {
    __shared__ ScanLds S;
    for (uint32_t f = blockIdx.x; f < nframes; f += gridDim.x) {
        uint64_t tot;
        const int st = scan_frame(src + frame_off[f], frame_len[f], S, &tot);
        if (threadIdx.x == 0) {
            u_len[f] = st == S3HC_OK ? (uint32_t)tot : 0u;
            status[f] = st;
        }
    }
}
}  // namespace

hipError_t launch_frame_sizes(const uint8_t* src, const uint64_t* frame_off, const uint32_t* frame_len, uint32_t n,
                              uint32_t* u_len, int32_t* status, hipStream_t st) {
    if (!n) return hipSuccess;
    const uint32_t grid = n < 16384u ? n : 16384u;
    hipLaunchKernelGGL(k_frame_sizes, dim3(grid), dim3(kT), 0, st, src, frame_off, frame_len, n, u_len, status);
    return hipGetLastError();
}
}  // namespace s3hc
