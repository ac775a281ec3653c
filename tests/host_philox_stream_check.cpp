// Host check of flashe_amd/csrc/philox_stream.h (the stream of NumPy's Philox4x64-10 generator as the device launch and the host state
// hand-back read it), built with -fsanitize=address,undefined by tests/test_philox_stream_sanitized.py.  The closed forms -- the counter
// and word of draw i, the state after n draws, the blocks and tiles of a launch's segments -- against a generator written here on its own
// that walks the stream ONE draw at a time the way NumPy does (increment the counter with carry, word by word, before every new block),
// at counters whose increment carries and wraps; then the checks of a segment table.
#include "philox_stream.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace flashe_philox;

#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

// NumPy's philox_next64, step by step
struct Walker {
    uint64_t key[2], counter[4], buffer[4];
    uint32_t pos;
    void increment()
    {
        for (int w = 0; w < 4; w++)
            if (++counter[w] != 0) break;
    }
    uint64_t next()
    {
        if (pos < 4) return buffer[pos++];
        increment();
        block(counter, key, buffer);
        pos = 1;
        return buffer[0];
    }
};

static long g_cases = 0;

static void check_stream(const uint64_t key[2], const uint64_t counter[4], uint32_t pre)
{
    // a generator pre-advanced by `pre` draws from a fresh state: buffer_pos 4, 1, 2, 3, 4
    Walker w{};
    memcpy(w.key, key, sizeof w.key);
    memcpy(w.counter, counter, sizeof w.counter);
    w.pos = 4;
    for (uint32_t i = 0; i < pre; i++) w.next();
    const Walker start = w;
    CHECK(start.pos == (pre == 0 ? 4u : (pre - 1) % 4 + 1));
    // draw i by position arithmetic against the walk; the state after i + 1 draws against the walker's
    for (uint64_t i = 0; i < 41; i++) {
        uint64_t at[4], words[4];
        uint32_t word;
        position(start.counter, start.pos, i, at, word);
        block(at, key, words);
        const uint64_t got = w.next();
        CHECK(words[word] == got);
        CHECK(to_double(got) == static_cast<double>(got >> 11) / 9007199254740992.0 && to_double(got) < 1.0);
        uint64_t c[4], b[4];
        uint32_t p = start.pos;
        memcpy(c, start.counter, sizeof c);
        memcpy(b, start.buffer, sizeof b);
        advance(key, c, p, b, i + 1);
        CHECK(memcmp(c, w.counter, sizeof c) == 0 && p == w.pos && memcmp(b, w.buffer, sizeof b) == 0);
        g_cases++;
    }
    // n = 0 changes nothing, not even a fresh generator's all-zero buffer
    uint64_t c[4], b[4] = {0, 0, 0, 0};
    uint32_t p = start.pos;
    memcpy(c, start.counter, sizeof c);
    advance(key, c, p, b, 0);
    CHECK(memcmp(c, start.counter, sizeof c) == 0 && p == start.pos && b[0] == 0 && b[3] == 0);
    // the launch's plan of this state: block j of the segment is block(base + j); the virtual draws [skip, skip + n) are the stream
    for (uint64_t n : {1ull, 2ull, 3ull, 4ull, 5ull, 1023ull, 1024ull, 1025ull}) {
        Segment s{};
        memcpy(s.key, key, sizeof s.key);
        memcpy(s.counter, start.counter, sizeof s.counter);
        s.buffer_pos = start.pos; s.n = n; s.offset = 7;
        std::vector<Plan> plans;
        const uint64_t tiles = plan_segments(&s, 1, plans);
        CHECK(plans.size() == 1 && plans[0].skip == (start.pos < 4 ? start.pos : 0) && plans[0].n == n && plans[0].offset == 7);
        const uint64_t blocks = segment_blocks(plans[0].skip, n);
        CHECK(4 * blocks >= plans[0].skip + n && 4 * (blocks - 1) < plans[0].skip + n);
        CHECK(tiles == (blocks + kTileBlocks - 1) / kTileBlocks);
        Walker v = start;
        for (uint64_t i = 0; i < n; i++) {
            const uint64_t virt = plans[0].skip + i;
            uint64_t at[4], words[4];
            counter_add(plans[0].base, virt / 4, at);
            block(at, key, words);
            CHECK(words[virt % 4] == v.next());
        }
    }
}

static void check_counter_add()
{
    const uint64_t ones[4] = {~0ull, ~0ull, ~0ull, ~0ull}, edge[4] = {~0ull - 1, ~0ull, 5, 0};
    uint64_t out[4];
    counter_add(ones, 1, out);
    CHECK(out[0] == 0 && out[1] == 0 && out[2] == 0 && out[3] == 0);                 // wraps at 2^256
    counter_add(ones, 3, out);
    CHECK(out[0] == 2 && out[1] == 0 && out[2] == 0 && out[3] == 0);
    counter_add(edge, 1, out);
    CHECK(out[0] == ~0ull && out[1] == ~0ull && out[2] == 5 && out[3] == 0);
    counter_add(edge, 2, out);
    CHECK(out[0] == 0 && out[1] == 0 && out[2] == 6 && out[3] == 0);                 // the carry runs through two words
    counter_add(edge, ~0ull, out);
    CHECK(out[0] == ~0ull - 2 && out[1] == 0 && out[2] == 6 && out[3] == 0);
    counter_add(edge, 0, out);
    CHECK(memcmp(out, edge, sizeof out) == 0);
}

static Segment seg(uint32_t pos, uint64_t n, uint64_t offset)
{
    Segment s{};
    s.key[0] = 1; s.buffer_pos = pos; s.n = n; s.offset = offset;
    return s;
}

static void check_segments_table()
{
    std::vector<Segment> t = {seg(4, 5, 0), seg(1, 4099, 5), seg(3, 1, 4104)};
    CHECK(check_segments(t.data(), 3) == kSegmentsOk);
    CHECK(check_segments(nullptr, 0) == kSegmentsOk);
    CHECK(check_segments(nullptr, 1) == kSegmentsBadCount && check_segments(t.data(), -1) == kSegmentsBadCount);
    // back to back is fine in any order; one shared draw is not; an empty segment overlaps nothing
    std::vector<Segment> r = {seg(4, 3, 10), seg(4, 10, 0), seg(0, 0, 5)};
    CHECK(check_segments(r.data(), 3) == kSegmentsOk);
    r[1].n = 11;
    CHECK(check_segments(r.data(), 3) == kSegmentsOverlap);
    r[1].n = 10; r[0].offset = 9;
    CHECK(check_segments(r.data(), 3) == kSegmentsOverlap);
    std::vector<Segment> same = {seg(4, 1, 2), seg(4, 1, 2)};
    CHECK(check_segments(same.data(), 2) == kSegmentsOverlap);
    // buffer_pos 0 .. 4
    for (uint32_t p = 0; p <= 5; p++) {
        Segment s = seg(p, 1, 0);
        CHECK(check_segments(&s, 1) == (p <= 4 ? kSegmentsOk : kSegmentsBadPos));
    }
    // counts and offsets whose byte counts would leave 64 bits
    Segment big = seg(4, kMaxDraws, 0);
    CHECK(check_segments(&big, 1) == kSegmentsOk);
    big.offset = 1;
    CHECK(check_segments(&big, 1) == kSegmentsOverflow);
    big = seg(4, kMaxDraws + 1, 0);
    CHECK(check_segments(&big, 1) == kSegmentsOverflow);
    big = seg(4, 1, ~0ull);
    CHECK(check_segments(&big, 1) == kSegmentsOverflow);
    big = seg(4, ~0ull, 2);                                     // offset + n wraps to 1
    CHECK(check_segments(&big, 1) == kSegmentsOverflow);
    // the segments a launch holds
    std::vector<Segment> many;
    for (int s = 0; s < kMaxSegments + 1; s++) many.push_back(seg(4, 3, 3 * static_cast<uint64_t>(s)));
    CHECK(check_segments(many.data(), kMaxSegments) == kSegmentsOk);
    CHECK(check_segments(many.data(), kMaxSegments + 1) == kSegmentsBadCount);
    CHECK(check_segments(many.data(), 3, 2) == kSegmentsBadCount);
    // the plans: empty segments take no tile, every other segment whole tiles of its own, in order
    std::vector<Segment> mix = {seg(4, 5, 0), seg(2, 0, 5), seg(1, 4099, 5), seg(3, 1, 4104)};
    std::vector<Plan> plans;
    const uint64_t tiles = plan_segments(mix.data(), 4, plans);
    CHECK(plans.size() == 3 && tiles == 1 + 5 + 1);             // 2 blocks; (1 + 4099 + 3) / 4 = 1025 blocks = 5 tiles; 1 block
    CHECK(plans[0].tile_first == 0 && plans[1].tile_first == 1 && plans[2].tile_first == 6);
    CHECK(plans[1].skip == 1 && plans[2].skip == 3 && plans[0].skip == 0 && plans[0].base[0] == 1 && plans[1].base[0] == 0);
}

int main()
{
    const uint64_t keys[2][2] = {{0, 0}, {0x0123456789abcdefull, ~0ull}};
    const uint64_t counters[4][4] = {{0, 0, 0, 0}, {~0ull - 1, ~0ull, 5, 0}, {~0ull, ~0ull, ~0ull, ~0ull}, {~0ull - 3, ~0ull, ~0ull, ~0ull}};
    for (const auto &key : keys)
        for (const auto &counter : counters)
            for (uint32_t pre = 0; pre <= 4; pre++) check_stream(key, counter, pre);
    check_counter_add();
    check_segments_table();
    printf("PHILOX_STREAM_OK %ld draws\n", g_cases);
    return 0;
}
