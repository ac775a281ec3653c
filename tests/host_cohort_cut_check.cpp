// Host check of flashe_amd/csrc/cohort_cut.h (into how many runs of consecutive clients a short cohort's summed chain is cut), built with
// -fsanitize=address,undefined by tests/test_cohort_cut_host.py.  Over a grid of clients, lengths and chip sizes: the bounds of the piece
// count, the pieces tile [0, C) without gap or overlap, the launch's streams fit its table, an uncut launch from half an item per
// wave upward, a chip filled once at the most; then it prints the table "C n cus compact int_bits parts" that the Python mirror is held against.
#include "cohort_cut.h"
#include "cohort_streams.h"

#include <cstdio>
#include <cstdlib>

using namespace flashe_tables;

#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

// the AES blocks of an n-element vector at int_bits <= 64 cut into n_jobs chunks, written here on its own (a loop over the chunks)
static uint64_t blocks_of(uint64_t n, int int_bits, uint32_t n_jobs)
{
    const uint64_t m = 128 / int_bits, d = n / n_jobs, r = n % n_jobs;
    uint64_t blocks = 0;
    for (uint32_t j = 0; j < n_jobs; j++) {
        const uint64_t len = d + (j < r ? 1 : 0);
        blocks += (len + m - 1) / m;
    }
    return blocks;
}

static long g_cases = 0;

static void check_case(int C, uint64_t n, int cus, bool compact, int int_bits)
{
    const uint64_t items = compact ? cohort_cut_items_compact(blocks_of(n, int_bits, 16)) : cohort_cut_items_wide(n);
    const int parts = cohort_cut_parts(C, items, cus);
    const uint64_t waves = static_cast<uint64_t>(cus) * 16;
    CHECK(parts >= 1 && parts <= 16 && parts <= C);
    CHECK(C + parts <= kCohortMaxStreams);
    if (2 * items > waves) CHECK(parts == 1);                       // (from half an item per wave upward: two pieces would not fit the chip once)
    if (parts > 1) CHECK(C / parts >= kCutMinOutputs);
    // the pieces: consecutive, none empty, together [0, C)
    CHECK(cohort_cut_begin(C, parts, 0) == 0 && cohort_cut_begin(C, parts, parts) == C);
    int covered = 0;
    for (int p = 0; p < parts; p++) {
        const int a = cohort_cut_begin(C, parts, p), b = cohort_cut_begin(C, parts, p + 1);
        CHECK(a == covered && b > a);
        covered = b;
    }
    CHECK(covered == C);
    // the pieces fill the chip once at the most: every wave takes one item or none
    if (parts > 1) CHECK(items * static_cast<uint64_t>(parts) <= waves);
    // and one piece more would not, unless a cap holds the count
    if (parts < 16 && (C / (parts + 1)) >= kCutMinOutputs) CHECK(items * static_cast<uint64_t>(parts + 1) > waves);
    if (!compact) CHECK(cohort_cut_all_half(n, parts, cus) == (((n + 255) / 256) * static_cast<uint64_t>(parts) < 2 * waves));
    printf("%d %llu %d %d %d %d\n", C, static_cast<unsigned long long>(n), cus, compact ? 1 : 0, int_bits, parts);
    g_cases++;
}

int main()
{
    const int clients[] = {1, 2, 3, 4, 5, 7, 8, 16, 17, 40, 63, 64, 100, 127, 128};
    const int chips[] = {1, 8, 104, 256, 304};
    const int widths[] = {16, 20, 23, 24, 32};
    for (const int cus : chips) {
        const uint64_t waves = static_cast<uint64_t>(cus) * 16;
        // lengths around every edge of the rule: one item, half, one and two half tiles per wave, the uncut admission, 2^32 - 1
        const uint64_t lens[] = {1, 2, 255, 256, 257, 700, 61706, 128 * waves - 1, 128 * waves, 128 * waves + 1, 256 * (waves - 1) + 1, 256 * waves,
                                 256 * waves + 1, (2 * waves - 1) * 256, (2 * waves - 1) * 256 + 1, 1000000, 0xffffffffull};
        for (const int C : clients)
            for (const uint64_t n : lens) {
                check_case(C, n, cus, false, 128);
                for (const int b : widths) check_case(C, n, cus, true, b);
            }
    }
    // the edge of the cut on 256 CUs: uncut from half an item per wave upward, whatever the cohort
    CHECK(cohort_cut_parts(128, cohort_cut_items_wide(256ull * 4096), 256) == 1);
    CHECK(cohort_cut_parts(128, cohort_cut_items_wide(256ull * 1025), 256) == 1);           // 2,050 items: two pieces outnumber the 4,096 waves
    CHECK(cohort_cut_parts(128, cohort_cut_items_wide(256ull * 1024), 256) == 2);           // 2,048 items: two pieces fill the chip once
    CHECK(cohort_cut_parts(100, cohort_cut_items_wide(61706), 256) == 8);                   // LeNet x 100: 484 items
    // 128 clients in 16 pieces: 144 streams, the table's limit
    CHECK(cohort_cut_parts(128, cohort_cut_items_wide(700), 256) == 16 && 128 + 16 == kCohortMaxStreams);
    // what the launch does not take
    CHECK(cohort_cut_parts(0, 6, 256) == 0 && cohort_cut_parts(129, 6, 256) == 0 && cohort_cut_parts(3, 0, 256) == 0 && cohort_cut_parts(3, 6, 0) == 0);
    printf("COHORT_CUT_OK %ld cases\n", g_cases);
    return 0;
}
