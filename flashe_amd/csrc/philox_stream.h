// The stream of NumPy's np.random.Philox (Philox4x64-10) as Generator.random draws it, stated once: the block function, the order in
// which a generator state hands out the words of its blocks, the state after n draws, the counter and word of draw i, and the checks of
// a table of output segments.  No HIP header, so that tests/host_philox_stream_check.cpp runs it on the host under sanitizers (as
// cohort_streams.h and layer_tables.h are); philox.hip compiles the same functions for the device through FLASHE_HD.
//   block(counter[4], key[2]) -> word[4]: ten rounds; before each of rounds 2 .. 10 the key is bumped by the Weyl constants;
//     a round maps (c0, c1, c2, c3) to (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0));
//   NumPy INCREMENTS the 256-bit counter (four little-endian 64-bit words, wrapping at 2^256) BEFORE it generates a block, and keeps
//     the block's words in `buffer` with buffer_pos = the next word to hand out: a state (counter, buffer_pos = p < 4) next returns
//     words p .. 3 of block(counter), then all of block(counter + 1), ...; p = 4 (fresh or exhausted) starts at block(counter + 1);
//   draw = (word >> 11) * 2^-53.
// So with  base = counter (p < 4) or counter + 1 (p = 4)  and  skip = p (p < 4) or 0:  draw i is word (skip + i) % 4 of
// block(base + (skip + i) / 4).
#pragma once
#include "draw_segments.h"

namespace flashe_philox {

using namespace flashe_draw;                         // kMaxSegments, kMaxDraws, to_double, SegmentsStatus and its values

constexpr uint64_t kM0 = 0xD2E7470EE14C6C93ull, kM1 = 0xCA5A826395121157ull;
constexpr uint64_t kWeyl0 = 0x9E3779B97F4A7C15ull, kWeyl1 = 0xBB67AE8584CAA73Bull;

FLASHE_HD void mulhilo(uint64_t a, uint64_t b, uint64_t &hi, uint64_t &lo)
{
    const unsigned __int128 p = static_cast<unsigned __int128>(a) * b;
    hi = static_cast<uint64_t>(p >> 64);
    lo = static_cast<uint64_t>(p);
}

FLASHE_HD void block(const uint64_t counter[4], const uint64_t key[2], uint64_t word[4])
{
    uint64_t c0 = counter[0], c1 = counter[1], c2 = counter[2], c3 = counter[3], k0 = key[0], k1 = key[1];
FLASHE_UNROLL
    for (int r = 0; r < 10; r++) {
        if (r) { k0 += kWeyl0; k1 += kWeyl1; }
        uint64_t hi0, lo0, hi1, lo1;
        mulhilo(kM0, c0, hi0, lo0);
        mulhilo(kM1, c2, hi1, lo1);
        c0 = hi1 ^ c1 ^ k0; c1 = lo1;
        c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    }
    word[0] = c0; word[1] = c1; word[2] = c2; word[3] = c3;
}

// out = counter + add mod 2^256
FLASHE_HD void counter_add(const uint64_t counter[4], uint64_t add, uint64_t out[4])
{
    uint64_t carry = add;
FLASHE_UNROLL
    for (int w = 0; w < 4; w++) {
        const uint64_t s = counter[w] + carry;
        carry = s < carry ? 1 : 0;
        out[w] = s;
    }
}

// Where the draws of a state (counter, buffer_pos <= 4) start: base[4] and skip (see the head of this file).
FLASHE_HD void stream_start(const uint64_t counter[4], uint32_t buffer_pos, uint64_t base[4], uint32_t &skip)
{
    counter_add(counter, buffer_pos < 4 ? 0 : 1, base);
    skip = buffer_pos < 4 ? buffer_pos : 0;
}

// Position arithmetic: draw i of the state is word `word` of block(at).
FLASHE_HD void position(const uint64_t counter[4], uint32_t buffer_pos, uint64_t i, uint64_t at[4], uint32_t &word)
{
    uint64_t base[4];
    uint32_t skip;
    stream_start(counter, buffer_pos, base, skip);
    const uint64_t v = skip + i;
    counter_add(base, v >> 2, at);
    word = static_cast<uint32_t>(v & 3);
}

// The state after n draws, in place: counter, buffer_pos and the buffered words (recomputed from the counter).  n = 0 changes nothing
// -- a fresh generator's buffer is zeros, not a block, and stays so.
inline void advance(const uint64_t key[2], uint64_t counter[4], uint32_t &buffer_pos, uint64_t buffer[4], uint64_t n)
{
    if (n == 0) return;
    uint64_t at[4];
    uint32_t word;
    position(counter, buffer_pos, n - 1, at, word);
    for (int w = 0; w < 4; w++) counter[w] = at[w];
    buffer_pos = word + 1;
    block(counter, key, buffer);
}

// One output segment of a launch: n draws of the state to draws [offset, offset + n) of the output buffer.
struct Segment { uint64_t key[2]; uint64_t counter[4]; uint32_t buffer_pos; uint64_t n, offset; };

constexpr SegmentsStatus kSegmentsBadPos = kSegmentsOwn;

// kSegmentsBadPos: a buffer_pos above 4; the rest is flashe_draw::check_segments.
inline SegmentsStatus check_segments(const Segment *segs, int n_segments, int max_segments = kMaxSegments)
{
    return flashe_draw::check_segments(segs, n_segments, max_segments, [](const Segment &s) { return s.buffer_pos <= 4; });
}

// The launch's view of a segment: whole blocks j = 0 .. blocks - 1 of block(base + j); block j holds the virtual draws 4 j .. 4 j + 3, of
// which [skip, skip + n) exist and go to out draw  offset + v - skip.  Tiles of kTileBlocks blocks belong to one segment: tile_first is the
// segment's first tile in the launch.
constexpr uint32_t kTileBlocks = 256;
struct Plan { uint64_t key[2]; uint64_t base[4]; uint64_t n, offset, tile_first; uint32_t skip, reserved; };

inline uint64_t segment_blocks(uint32_t skip, uint64_t n) { return (skip + n + 3) / 4; }

// The plans of the non-empty segments (checked already); returns the launch's tiles.
inline uint64_t plan_segments(const Segment *segs, int n_segments, std::vector<Plan> &plans)
{
    plans.clear();
    uint64_t tiles = 0;
    for (int s = 0; s < n_segments; s++) {
        if (!segs[s].n) continue;
        Plan p{};
        p.key[0] = segs[s].key[0]; p.key[1] = segs[s].key[1];
        stream_start(segs[s].counter, segs[s].buffer_pos, p.base, p.skip);
        p.n = segs[s].n; p.offset = segs[s].offset; p.tile_first = tiles;
        tiles += (segment_blocks(p.skip, p.n) + kTileBlocks - 1) / kTileBlocks;
        plans.push_back(p);
    }
    return tiles;
}

// A caller's segment struct (flashe_philox_segment's fields) as a Segment.
template <class CSegment> inline void from_c(const CSegment &s, Segment &o)
{
    o.key[0] = s.key[0]; o.key[1] = s.key[1];
    for (int w = 0; w < 4; w++) o.counter[w] = s.counter[w];
    o.buffer_pos = s.buffer_pos; o.n = s.n; o.offset = s.offset;
}

// ---- the draws of a cohort generated inside the launch that consumes them (codec.hip's quantize_philox_combine_cohort_kernel) ----
// One plan per client, 56 bytes: the client's draw for its value k is word (skip + k) % 4 of block(base + (skip + k) / 4), skip < 4.
struct ClientPlan { uint64_t key[2]; uint64_t base[4]; uint32_t skip, reserved; };

// The plan of the stretch that starts at draw `first` of a segment's state.
inline ClientPlan client_plan(const Segment &s, uint64_t first)
{
    ClientPlan p{};
    p.key[0] = s.key[0]; p.key[1] = s.key[1];
    position(s.counter, s.buffer_pos, first, p.base, p.skip);
    return p;
}

// The draw of value k under a plan, one draw at a time (the launch's value-by-value path; its runs of four take whole blocks).
FLASHE_HD double client_draw(const uint64_t key[2], const uint64_t base[4], uint32_t skip, uint64_t k)
{
    const uint64_t v = skip + k;
    uint64_t at[4], w[4];
    counter_add(base, v >> 2, at);
    block(at, key, w);
    const uint32_t i = static_cast<uint32_t>(v & 3);
    return to_double(i == 0 ? w[0] : i == 1 ? w[1] : i == 2 ? w[2] : w[3]);
}

// The four draws of values k0 .. k0 + 3 (k0 % 4 == 0) under a plan: one block where skip is 0, else the tail of one and the head of the next.
FLASHE_HD void client_draws4(const uint64_t key[2], const uint64_t base[4], uint32_t skip, uint64_t k0, double d[4])
{
    uint64_t at[4], w[8];
    counter_add(base, k0 >> 2, at);
    block(at, key, w);
    if (skip) {
        uint64_t nx[4], again[2] = {key[0], key[1]};
        counter_add(at, 1, nx);
#if defined(__HIP_DEVICE_COMPILE__)
        // (the key is uniform over the launch: taken as new here, so that the round keys of the first block are not kept in scalar
        // registers for the second -- the kernels that call this hold no spare ones)
        __asm__ volatile("" : "+s"(again[0]), "+s"(again[1]));
#endif
        block(nx, again, w + 4);
    } else {
        w[4] = w[5] = w[6] = 0;
    }
FLASHE_UNROLL
    for (int t = 0; t < 4; t++) d[t] = to_double(skip == 0 ? w[t] : skip == 1 ? w[t + 1] : skip == 2 ? w[t + 2] : w[t + 3]);
}

// block() for a caller that computes many blocks under one launch-uniform key: on the device the key is taken as new at every call, so
// that the round keys of one block are not kept in scalar registers for the next (client_draws4's note).
FLASHE_HD void block_fresh_key(const uint64_t counter[4], const uint64_t key[2], uint64_t word[4])
{
    uint64_t again[2] = {key[0], key[1]};
#if defined(__HIP_DEVICE_COMPILE__)
    __asm__ volatile("" : "+s"(again[0]), "+s"(again[1]));
#endif
    block(counter, again, word);
}

// ---- a RUN of values [k, k + m) under a plan (codec.hip's quantize_batch_philox_combine_cohort_kernel: the values of a group of
// batched elements are consecutive values of their client) ----
// Stated once: the run's draws are words word, word + 1, ... of block(first), block(first + 1), ...; it touches `blocks` blocks -- m / 4
// where the run starts at a block's first word and m is a multiple of four, one more where it does not.  m = 0: no block.
FLASHE_HD void client_run(const uint64_t base[4], uint32_t skip, uint64_t k, uint64_t m, uint64_t first[4], uint64_t &blocks, uint32_t &word)
{
    const uint64_t v = skip + k;
    counter_add(base, v >> 2, first);
    word = static_cast<uint32_t>(v & 3);
    blocks = m ? (word + m + 3) / 4 : 0;
}

// The run walked one draw at a time: the current block is kept and a new one is computed only when the word index wraps, so m draws
// cost client_run's `blocks` blocks (made counts them) and never one per value.
struct RunWalk {
    uint64_t at[4], w[4];
    uint32_t word, made;
    FLASHE_HD void start(const uint64_t key[2], const uint64_t base[4], uint32_t skip, uint64_t k)
    {
        uint64_t blocks;
        client_run(base, skip, k, 1, at, blocks, word);
        block_fresh_key(at, key, w);
        made = 1;
    }
    FLASHE_HD double next(const uint64_t key[2])
    {
        if (word == 4) {
            uint64_t nx[4];
            counter_add(at, 1, nx);
FLASHE_UNROLL
            for (int i = 0; i < 4; i++) at[i] = nx[i];
            block_fresh_key(at, key, w);
            word = 0;
            made++;
        }
        const uint64_t x = word == 0 ? w[0] : word == 1 ? w[1] : word == 2 ? w[2] : w[3];
        word++;
        return to_double(x);
    }
};

// The draws of the 4 Q values k0 .. k0 + 4 Q - 1 for a lane that takes them four at a time, in order: step(i) gives values
// k0 + 4 i .. k0 + 4 i + 3.  Every block of the run is computed once -- Q where the run starts at a block's first word, Q + 1 where it
// does not (the words behind the run's start of one block, then the words in front of it of the next).
struct RunBlocks {
    uint64_t at[4], w[8];
    uint32_t word;
    FLASHE_HD void start(const uint64_t key[2], const uint64_t base[4], uint32_t skip, uint64_t k0)
    {
        uint64_t blocks;
        client_run(base, skip, k0, 4, at, blocks, word);
        block_fresh_key(at, key, w + 4);
    }
    FLASHE_HD void next_block(const uint64_t key[2])
    {
        uint64_t nx[4];
        counter_add(at, 1, nx);
FLASHE_UNROLL
        for (int i = 0; i < 4; i++) at[i] = nx[i];
        block_fresh_key(at, key, w + 4);
    }
    // first: the run's first four values (the block start() made is theirs)
    FLASHE_HD void step(const uint64_t key[2], bool first, double d[4])
    {
FLASHE_UNROLL
        for (int t = 0; t < 4; t++) w[t] = w[t + 4];
        if (word || !first) next_block(key);
        // word 0: w[t + 4], else w[t + word] -- picked with masks, so that the four picks stay straight-line code on the device
        const uint64_t odd = 0 - static_cast<uint64_t>(word & 1), high = 0 - static_cast<uint64_t>((word >> 1) & 1);
FLASHE_UNROLL
        for (int t = 0; t < 4; t++) {
            const uint64_t a = w[t + 4] ^ ((w[t + 4] ^ w[t + 1]) & odd), b = w[t + 2] ^ ((w[t + 2] ^ w[t + 3]) & odd);
            d[t] = to_double(a ^ ((a ^ b) & high));
        }
    }
};

// The plans of n_clients clients of n draws each from checked segments: draw_segments.h's cohort_stretches (its contract and status
// values: kCohortPlansTooMany, kCohortPlansNotTiled, kCohortPlansSplitClient), one client_plan per stretch.  No plans unless kCohortPlansOk.
inline CohortPlansStatus cohort_plans(const Segment *segs, int n_segments, uint64_t n_clients, uint64_t n, std::vector<ClientPlan> &plans)
{
    plans.clear();
    const CohortPlansStatus st = cohort_stretches(segs, n_segments, n_clients, n, [] { return kCohortPlansOk; },
                                                  [&](const Segment &s, uint64_t first) { plans.push_back(client_plan(s, first)); });
    if (st != kCohortPlansOk) plans.clear();
    return st;
}

}  // namespace flashe_philox
