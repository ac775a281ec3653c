// What the int_bits <= 64 PRF kernels of kernels.hip and the wire kernels of wire.hip share: the per-launch constants and the map from an
// AES block of the vector to its elements and its counter.  A lane encrypts one AES block = the masks of m = 128 / int_bits consecutive
// elements; the chunking chunks_idx(range(n), n_jobs) restarts the counter at every chunk, so the last block of a chunk may hold fewer.
#pragma once
#include "device_common.h"

namespace flashe {

constexpr int kSmallThreads = 1024;

struct SmallParams {
    uint64_t n;               // length of the whole vector (defines the chunking)
    uint32_t n_jobs, iter;
    int b, m;
    int no_direct;            // A/B knob FLASHE_SMALL_DIRECT: 0 = stage every output through the LDS rows, 2 = general walk instead of the b <= 32 fast walk
    int swp_prio;             // wave priority rising through the rounds of a block pair (device_common.h): set per launch from the measured table
    int no_fixed_width;       // A/B knob FLASHE_SMALL_FIXED=0: the compact layout's kernels with int_bits at run time even at the compiled-in widths
    uint32_t m_magic;         // ceil(2^32 / m): x / m == (x * m_magic) >> 32 for x < 2^13
    uint64_t mask_lo;
    uint64_t top_lo, top_hi;  // the top bit of every b-bit slot of the 128-bit word (SWAR subtraction)
    uint32_t nb1_magic, nb0_magic;   // floor(2^32 / nb1), floor(2^32 / nb0): 32-bit block -> chunk division without a divide
    const uint32_t *te0;
    Codec cq;                 // optional fused quantise front end / unquantise back end (single-job launches)
};

// x / dsr for 32-bit operands with magic = floor(2^32 / dsr) (dsr >= 2; dsr == 1 is handled by the caller): the estimate is at most
// two short, fixed up by comparisons -- ~8 instructions instead of the ~100 of a 64-bit division per AES block.
__device__ __forceinline__ uint32_t udiv_magic(uint32_t x, uint32_t dsr, uint32_t magic)
{
    uint32_t q = __umulhi(x, magic);
    uint32_t rem = x - q * dsr;
    if (rem >= dsr) { q++; rem -= dsr; }
    if (rem >= dsr) { q++; }
    return q;
}

// block B of the vector (global block numbering) -> first element j0, elements in the block cnt, PRF counter (n < 2^32)
__device__ __forceinline__ void small_block_params(uint32_t B32, uint32_t nb1_32, uint32_t nb0_32, uint32_t d32, uint32_t r32, uint32_t m,
                                                   const SmallParams &p, uint64_t *j0, int *cnt, uint32_t *ctr)
{
    uint32_t begin, len, i;
    if (B32 < r32 * nb1_32) {
        const uint32_t c = nb1_32 == 1 ? B32 : udiv_magic(B32, nb1_32, p.nb1_magic);
        i = B32 - c * nb1_32; begin = c * (d32 + 1u); len = d32 + 1u;
    } else {
        const uint32_t B2 = B32 - r32 * nb1_32, c = nb0_32 == 1 ? B2 : udiv_magic(B2, nb0_32, p.nb0_magic);
        i = B2 - c * nb0_32; begin = r32 * (d32 + 1u) + c * d32; len = d32;
    }
    const uint32_t rem = len - i * m;
    *j0 = static_cast<uint64_t>(begin) + static_cast<uint64_t>(i) * m;
    *cnt = static_cast<int>(rem < m ? rem : m);
    *ctr = begin + i;
}

// host side (kernels.hip): the per-launch constants of the b <= 64 kernels (n < 2^32), and the AES-block index (global block numbering)
// of element j of an n-vector cut into J chunks of m-element blocks
SmallParams small_params_of(const LaunchEnv &env, uint32_t iter, uint64_t n, uint32_t n_jobs);
uint64_t block_of(uint64_t j, uint64_t n, uint64_t J, uint64_t m);

}  // namespace flashe
