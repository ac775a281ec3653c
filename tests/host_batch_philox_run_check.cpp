// Host check of the run arithmetic the BATCHED prepared cohort launch that generates its own Philox draws added to
// flashe_amd/csrc/philox_stream.h (client_run, RunWalk, RunBlocks) and to layer_tables.h (batched_groups, prepared_block with groups and plans),
// built with -fsanitize=address,undefined by tests/test_batch_philox_run_host.py.  Everything is compared with brute force: position() +
// block(), value by value.  Every skip 0 .. 3, bs 1 .. 10 and 128, row starts 0 .. 7, runs of four whole elements and runs that end
// in pads, counters whose increment carries into word 1 and wraps at 2^256; the blocks a walk computes are counted; a segment table that
// tiles C n_elems instead of C n_values is refused by cohort_plans.
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

static const uint64_t M = ~0ull;
static const uint64_t kCounters[][4] = {{0, 0, 0, 0}, {12345, 6, 7, 8}, {M - 1, 0, 0, 0}, {M - 1, M, 5, 0}, {M, M, M, M}, {M - 2, M, M, M}};
static long g_values = 0, g_walks = 0, g_groups = 0;

// brute force: draw k of the plan (base, skip) is word (skip + k) % 4 of block(base + (skip + k) / 4): position() on a state at base
static double brute(const uint64_t key[2], const uint64_t base[4], uint32_t skip, uint64_t k)
{
    uint64_t at[4], w[4];
    uint32_t word;
    position(base, skip, k, at, word);              // (buffer_pos = skip < 4: base and skip are the state's own)
    block(at, key, w);
    return to_double(w[word]);
}

// a run of values [k, k + m): client_run's first block, word and block count; RunWalk's draws and the blocks it made
static void check_walk(const uint64_t key[2], const uint64_t base[4], uint32_t skip, uint64_t k, uint64_t m)
{
    uint64_t first[4], blocks, at[4];
    uint32_t word, w0;
    client_run(base, skip, k, m, first, blocks, word);
    position(base, skip, k, at, w0);
    CHECK(memcmp(first, at, sizeof at) == 0 && word == w0);
    CHECK(blocks == (m ? (w0 + m + 3) / 4 : 0));
    CHECK(!m || m % 4 || blocks == m / 4 + (w0 ? 1 : 0));                   // four values per block, one more block when misaligned
    if (!m) return;
    RunWalk rw;
    rw.start(key, base, skip, k);
    for (uint64_t i = 0; i < m; i++) {
        CHECK(rw.next(key) == brute(key, base, skip, k + i));
        g_values++;
    }
    CHECK(rw.made == blocks);                                         // never one block per value
    g_walks++;
}

// four whole elements of bs values from value k0 on: RunBlocks' bs steps of four
static void check_group(const uint64_t key[2], const uint64_t base[4], uint32_t skip, uint64_t k0, int bs)
{
    RunBlocks rb;
    rb.start(key, base, skip, k0);
    for (int i = 0; i < bs; i++) {
        double d[4];
        rb.step(key, i == 0, d);
        for (int t = 0; t < 4; t++) CHECK(d[t] == brute(key, base, skip, k0 + 4 * static_cast<uint64_t>(i) + t));
    }
    // the last block it made is the run's last: first + blocks - 1
    uint64_t first[4], blocks, last[4];
    uint32_t word;
    client_run(base, skip, k0, 4 * static_cast<uint64_t>(bs), first, blocks, word);
    counter_add(first, blocks - 1, last);
    CHECK(memcmp(rb.at, last, sizeof last) == 0 && blocks == static_cast<uint64_t>(bs) + (word ? 1 : 0));
    g_groups++;
}

// a row of `elems` elements of bs values whose last element holds `tail` values (1 .. bs), walked the way the kernel walks it
static void check_row(const uint64_t key[2], const uint64_t base[4], uint32_t skip, uint64_t row_start, int bs, uint64_t elems, int tail)
{
    const uint64_t size = (elems - 1) * bs + tail;
    for (uint64_t first = 0; first < elems; first += 4) {
        const uint64_t j0 = first * bs;
        if (j0 + 4ull * bs <= size) {
            if (bs <= 10) check_group(key, base, skip, row_start + j0, bs);
            check_walk(key, base, skip, row_start + j0, 4ull * bs);
        } else {
            check_walk(key, base, skip, row_start + j0, size - j0);   // the row's last elements: the pads draw nothing
        }
    }
}

static void check_tables()
{
    using namespace flashe_tables;
    // rows of 1, 4, 5, 8, 27 elements at bs 6 (value counts with pads): groups 1, 1, 2, 2, 7
    const uint64_t bs = 6, rows[] = {0, 1, 1, 24, 5, 25, 10, 48, 18, 27 * 6 - 5};
    uint64_t first_group[5];
    CHECK(batched_groups(rows, 5, bs, first_group) == 13);
    const uint64_t want[] = {0, 1, 2, 4, 6};
    CHECK(memcmp(first_group, want, sizeof want) == 0);
    const PreparedBlock at = prepared_block(3, 5, sizeof(ClientPlan) / 8, true);
    CHECK(at.mask == 0 && at.ct == 24 && at.rows == 48 && at.groups == 48 + 80 && at.plans == 48 + 120 && at.words == 6 + 15 + 21);
    CHECK(at.rows == prepared_block(3, 5).rows && at.groups == 8 * prepared_block(3, 5).words);       // (the buffer form's block, then groups and plans)
    // the segments tile the clients' VALUES: a table over the elements is refused
    const uint64_t key[2] = {1, 2}, counter[4] = {3, 4, 5, 6};
    const uint64_t n_values = 1 + 24 + 25 + 48 + 27 * 6 - 5, n_elems = 1 + 4 + 5 + 8 + 27, C = 3;
    Segment s{};
    memcpy(s.key, key, sizeof key);
    memcpy(s.counter, counter, sizeof counter);
    s.buffer_pos = 2; s.offset = 0;
    std::vector<ClientPlan> plans;
    s.n = C * n_values;
    CHECK(check_segments(&s, 1) == kSegmentsOk && cohort_plans(&s, 1, C, n_values, plans) == kCohortPlansOk && plans.size() == C);
    for (uint64_t c = 0; c < C; c++) {
        CHECK(plans[c].skip == (2 + c * n_values) % 4);
        check_walk(plans[c].key, plans[c].base, plans[c].skip, 0, 9);
    }
    s.n = C * n_elems;
    CHECK(check_segments(&s, 1) == kSegmentsOk && cohort_plans(&s, 1, C, n_values, plans) == kCohortPlansNotTiled && plans.empty());
    Segment per[3] = {s, s, s};
    for (uint64_t c = 0; c < C; c++) { per[c].n = n_elems; per[c].offset = c * n_elems; }
    CHECK(check_segments(per, 3) == kSegmentsOk && cohort_plans(per, 3, C, n_values, plans) == kCohortPlansNotTiled && plans.empty());
    for (uint64_t c = 0; c < C; c++) { per[c].n = n_values; per[c].offset = c * n_values; }
    CHECK(cohort_plans(per, 3, C, n_values, plans) == kCohortPlansOk && plans.size() == C);
}

int main()
{
    const int sizes[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 128};
    for (const auto &counter : kCounters) {
        const uint64_t key[2] = {0x0123456789abcdefull ^ counter[0], 0xfedcba9876543210ull + counter[1]};
        for (uint32_t skip = 0; skip < 4; skip++)
            for (const int bs : sizes)
                for (uint64_t row_start = 0; row_start < 8; row_start++) {
                    check_row(key, counter, skip, row_start, bs, 4, bs);                    // one whole group
                    check_row(key, counter, skip, row_start, bs, 7, 1);                     // a group, then three elements, the last with one value
                    check_row(key, counter, skip, row_start, bs, 8, bs > 1 ? bs - 1 : 1);   // two groups, the second with a pad (bs > 1)
                    check_row(key, counter, skip, row_start, bs, 1, 1);                     // a one-value row
                    check_walk(key, counter, skip, row_start, 0);
                }
    }
    check_tables();
    printf("BATCH_PHILOX_RUN_OK %ld values %ld walks %ld groups\n", g_values, g_walks, g_groups);
    return 0;
}
