// Host check of what the prepared cohort launch that generates its own Philox draws added to flashe_amd/csrc/philox_stream.h (client_plan,
// client_draw, client_draws4, cohort_plans) and to layer_tables.h (prepared_block with plans), built with -fsanitize=address,undefined by
// tests/test_prepared_philox_host.py.  Every client's plan -- from one segment shared by all clients, from a segment per client in any
// table order, from a generator continued over several segments -- against a generator written here that walks the stream ONE draw at a
// time the way NumPy does: every buffer_pos 0 .. 4, client offsets of every residue mod 4, counters whose increment carries and wraps;
// the staging block built the way abi_layers.hip builds it and read back through the offsets; the tiling check of the segments.
#include "layer_tables.h"
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

static const uint64_t M = ~0ull;
static const uint64_t kCounters[][4] = {{0, 0, 0, 0}, {12345, 6, 7, 8}, {M - 2, 0, 0, 0}, {M - 1, M, 5, 0}, {M - 2, M, M, 9}, {M, M, M, M}, {M - 3, M, M, M}};
static long g_draws = 0, g_blocks = 0;

// a state at buffer_pos `pos`: below 4 the buffer holds block(counter), as NumPy's does
static Walker walker_of(const uint64_t key[2], const uint64_t counter[4], uint32_t pos)
{
    Walker w{};
    memcpy(w.key, key, sizeof w.key);
    memcpy(w.counter, counter, sizeof w.counter);
    w.pos = pos;
    if (pos < 4) block(w.counter, w.key, w.buffer);
    return w;
}

static Segment segment_of(const Walker &w, uint64_t n, uint64_t offset)
{
    Segment s{};
    memcpy(s.key, w.key, sizeof s.key);
    memcpy(s.counter, w.counter, sizeof s.counter);
    s.buffer_pos = w.pos; s.n = n; s.offset = offset;
    return s;
}

// client c's n draws under its plan -- one at a time and in runs of four -- are the walker's next n
static void check_client(const ClientPlan &p, Walker &w, uint64_t n)
{
    CHECK(p.skip < 4 && p.reserved == 0 && p.key[0] == w.key[0] && p.key[1] == w.key[1]);
    std::vector<double> want(n);
    for (uint64_t k = 0; k < n; k++) want[k] = to_double(w.next());
    for (uint64_t k = 0; k < n; k++) {
        CHECK(client_draw(p.key, p.base, p.skip, k) == want[k]);
        g_draws++;
    }
    for (uint64_t k0 = 0; k0 < n; k0 += 4) {
        double d[4];
        client_draws4(p.key, p.base, p.skip, k0, d);
        for (uint64_t t = 0; t < 4 && k0 + t < n; t++) CHECK(d[t] == want[k0 + t]);
        g_blocks++;
    }
}

// the staging block as quantize_combine_cohort builds it: mask pointers, ciphertext pointers, the plans; behind a front of any size
static void check_block(const std::vector<ClientPlan> &plans, size_t front_bytes)
{
    using namespace flashe_tables;
    static_assert(sizeof(ClientPlan) == 56, "seven 8-byte words per plan");
    const int C = static_cast<int>(plans.size());
    const size_t plan_words = sizeof(ClientPlan) / 8;
    std::vector<uint64_t> extra(2 * static_cast<size_t>(C));
    for (int c = 0; c < C; c++) {
        extra[static_cast<size_t>(c)] = 0x1000u + 16u * static_cast<uint64_t>(c);
        extra[static_cast<size_t>(C) + c] = 0x900000u + 16u * static_cast<uint64_t>(c);
    }
    const PreparedBlock at = prepared_block(C, 0, plan_words);
    extra.resize(at.words);
    memcpy(extra.data() + 2 * static_cast<size_t>(C), plans.data(), plans.size() * sizeof(ClientPlan));
    CHECK(at.mask == 0 && at.ct == 8 * static_cast<size_t>(C) && at.plans == 16 * static_cast<size_t>(C) && at.words == 9 * static_cast<size_t>(C));
    CHECK(at.plans + sizeof(ClientPlan) * plans.size() == 8 * at.words);
    CHECK(prepared_block(C).rows == at.plans && at.rows == at.plans && at.groups == at.plans);      // (the pointers lie where the buffer form has them; no rows, no groups)
    Blob blob;
    std::vector<char> front(front_bytes, 'x');
    blob.add(front.data(), front.size());
    const size_t extra_at = blob.add(extra.data(), extra.size() * sizeof(uint64_t));
    CHECK(extra_at % 16 == 0 && blob.bytes.size() == extra_at + 8 * at.words);
    const char *dev = blob.bytes.data() + extra_at;
    for (int c = 0; c < C; c++) {
        uint64_t m, t;
        memcpy(&m, dev + at.mask + 8 * static_cast<size_t>(c), 8);
        memcpy(&t, dev + at.ct + 8 * static_cast<size_t>(c), 8);
        CHECK(m == 0x1000u + 16u * static_cast<uint64_t>(c) && t == 0x900000u + 16u * static_cast<uint64_t>(c));
        ClientPlan p;
        memcpy(&p, dev + at.plans + sizeof(ClientPlan) * static_cast<size_t>(c), sizeof p);
        CHECK(memcmp(&p, &plans[c], sizeof p) == 0);
        CHECK((extra_at + at.plans + sizeof(ClientPlan) * static_cast<size_t>(c)) % 8 == 0);
    }
}

static void check_cohort(const uint64_t counter[4], uint32_t pos, int C, uint64_t n)
{
    const uint64_t key[2] = {0x0123456789abcdefull + pos, 0xfedcba9876543210ull - static_cast<uint64_t>(C)};
    // 1. one segment for all clients: client c starts c n draws into the stream
    {
        Walker w = walker_of(key, counter, pos);
        const Segment s = segment_of(w, static_cast<uint64_t>(C) * n, 0);
        std::vector<ClientPlan> plans;
        CHECK(check_segments(&s, 1) == kSegmentsOk);
        CHECK(cohort_plans(&s, 1, C, n, plans) == kCohortPlansOk && plans.size() == static_cast<size_t>(C));
        for (int c = 0; c < C; c++) {
            CHECK(plans[c].skip == ((pos < 4 ? pos : 0) + static_cast<uint64_t>(c) * n) % 4);
            check_client(plans[c], w, n);
        }
        check_block(plans, static_cast<size_t>((7 * C + pos) % 41));
        // 2. the same generator continued over one segment per client (what listing one Generator C times makes): the same plans
        std::vector<Segment> segs;
        uint64_t c4[4], b4[4] = {0, 0, 0, 0};
        uint32_t p = pos;
        memcpy(c4, counter, sizeof c4);
        for (int c = 0; c < C; c++) {
            Segment t{};
            memcpy(t.key, key, sizeof t.key);
            memcpy(t.counter, c4, sizeof c4);
            t.buffer_pos = p; t.n = n; t.offset = static_cast<uint64_t>(c) * n;
            segs.push_back(t);
            advance(key, c4, p, b4, n);
        }
        std::vector<ClientPlan> again;
        CHECK(cohort_plans(segs.data(), C, C, n, again) == kCohortPlansOk && again.size() == plans.size());
        for (int c = 0; c < C; c++)
            CHECK(again[c].skip == plans[c].skip && memcmp(again[c].base, plans[c].base, 32) == 0 && memcmp(again[c].key, plans[c].key, 16) == 0);
    }
    // 3. a generator per client, each at another key, counter and position; the table lists them last client first, with empty segments
    // between where it holds them (a table holds kMaxSegments; more clients than that share generators)
    if (C <= kMaxSegments) {
        std::vector<Walker> ws;
        std::vector<Segment> segs;
        for (int c = 0; c < C; c++) {
            const uint64_t k2[2] = {key[0] ^ (0x9e37ull * static_cast<uint64_t>(c + 1)), key[1] + static_cast<uint64_t>(c)};
            uint64_t cn[4];
            counter_add(counter, static_cast<uint64_t>(c) * 3, cn);
            ws.push_back(walker_of(k2, cn, (pos + static_cast<uint32_t>(c)) % 5));
        }
        for (int c = C - 1; c >= 0; c--) {
            segs.push_back(segment_of(ws[c], n, static_cast<uint64_t>(c) * n));
            if (2 * C <= kMaxSegments) segs.push_back(segment_of(ws[c], 0, 12345));
        }
        std::vector<ClientPlan> plans;
        CHECK(check_segments(segs.data(), static_cast<int>(segs.size())) == kSegmentsOk);
        CHECK(cohort_plans(segs.data(), static_cast<int>(segs.size()), C, n, plans) == kCohortPlansOk && plans.size() == static_cast<size_t>(C));
        for (int c = 0; c < C; c++) check_client(plans[c], ws[c], n);
        check_block(plans, static_cast<size_t>((3 * C + pos) % 17));
    }
}

static void check_tiling()
{
    const uint64_t key[2] = {1, 2}, counter[4] = {3, 4, 5, 6};
    const Walker w = walker_of(key, counter, 4);
    const uint64_t n = 10;
    std::vector<ClientPlan> plans;
    auto two = [&](uint64_t n0, uint64_t off0, uint64_t n1, uint64_t off1) {
        Segment s[2] = {segment_of(w, n0, off0), segment_of(w, n1, off1)};
        if (check_segments(s, 2) != kSegmentsOk) return -static_cast<int>(check_segments(s, 2));
        return static_cast<int>(cohort_plans(s, 2, 2, n, plans));
    };
    CHECK(two(n, 0, n, n) == kCohortPlansOk && plans.size() == 2);
    CHECK(two(n, n, n, 0) == kCohortPlansOk);
    CHECK(two(n, 0, n, n + 1) == kCohortPlansNotTiled);                           // a gap, and beyond 2 n
    CHECK(two(n - 1, 0, n, n) == kCohortPlansNotTiled);                           // a gap inside
    CHECK(two(n, 1, n - 1, n + 1) == kCohortPlansNotTiled);                       // a gap in front
    CHECK(two(n, 0, n, n - 1) == -static_cast<int>(kSegmentsOverlap));            // an overlap is check_segments' to find ...
    {
        Segment s[2] = {segment_of(w, n, 0), segment_of(w, n, n - 1)};
        CHECK(cohort_plans(s, 2, 2, n, plans) == kCohortPlansNotTiled && plans.empty());       // ... and does not pass here either
    }
    CHECK(two(n, 0, n + 1, n) == kCohortPlansNotTiled);                           // beyond 2 n
    CHECK(two(n, 0, n - 1, n) == kCohortPlansNotTiled);                           // short of 2 n
    CHECK(two(n + 1, 0, n - 1, n + 1) == kCohortPlansSplitClient && plans.empty());   // tiled, but client 1 spans two segments
    CHECK(two(2 * n, 0, 0, 99) == kCohortPlansOk && plans.size() == 2);           // one segment for both, and an empty one anywhere
    CHECK(two(0, 0, 0, 0) == kCohortPlansNotTiled);                               // nothing for 2 n draws
    Segment one = segment_of(w, 3 * n, 0);
    CHECK(cohort_plans(&one, 1, 3, n, plans) == kCohortPlansOk && plans.size() == 3);
    CHECK(cohort_plans(&one, 1, 2, n, plans) == kCohortPlansNotTiled && cohort_plans(&one, 1, 4, n, plans) == kCohortPlansNotTiled);
    CHECK(cohort_plans(nullptr, 0, 1, n, plans) == kCohortPlansNotTiled);
    // an empty model: every segment empty, no plans
    Segment none = segment_of(w, 0, 0);
    CHECK(cohort_plans(&none, 1, 3, 0, plans) == kCohortPlansOk && plans.empty());
    CHECK(cohort_plans(nullptr, 0, 3, 0, plans) == kCohortPlansOk && plans.empty());
    CHECK(cohort_plans(&one, 1, 3, 0, plans) == kCohortPlansNotTiled);
    // n_clients n beyond what a segment may hold
    Segment big = segment_of(w, kMaxDraws, 0);
    CHECK(cohort_plans(&big, 1, 1ull << 40, 1ull << 21, plans) == kCohortPlansTooMany);
    CHECK(cohort_plans(&big, 1, 1, kMaxDraws, plans) == kCohortPlansOk && plans.size() == 1);
    CHECK(cohort_plans(&big, 1, 2, kMaxDraws, plans) == kCohortPlansTooMany && plans.empty());
}

int main()
{
    for (const auto &counter : kCounters)
        for (uint32_t pos = 0; pos <= 4; pos++)
            for (int C : {1, 2, 3, 5})
                for (uint64_t n : {1ull, 2ull, 3ull, 4ull, 5ull, 7ull, 9ull, 30ull}) check_cohort(counter, pos, C, n);
    // the plan table at its largest
    for (int C : {10, 127, 128, 130}) check_cohort(kCounters[2], 3, C, 5);
    check_tiling();
    printf("PREPARED_PHILOX_OK %ld draws %ld runs\n", g_draws, g_blocks);
    return 0;
}
