// Host check of cohort_cut_pieces in flashe_amd/csrc/cohort_cut.h (the pieces of a short cohort given by ANY strictly ascending cipher
// indices: every gap is a cut), built with -fsanitize=address,undefined by tests/test_cohort_cut_pieces_host.py.  One run gives exactly
// cohort_cut_parts / cohort_cut_begin; the pinned examples; over a fixed-seed fuzz: at most 16 pieces, C + pieces streams fit the table,
// every run boundary is a piece boundary, a gapped cohort never has one piece, a split run keeps kCutMinOutputs clients per piece; the
// refusals; then it prints "items cus C idx.. | parts begins.." per case for the Python mirror to be held against.
#include "cohort_cut.h"
#include "cohort_streams.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace flashe_tables;

#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

static long g_cases = 0;

// begins on the heap, exactly kCutMaxParts + 1 entries: a write past them is the sanitizer's to report
static std::vector<int> pieces(const std::vector<uint32_t> &idx, uint64_t items, int cus, bool print = true)
{
    std::vector<int> begins(kCutMaxParts + 1, -1);
    const int parts = cohort_cut_pieces(idx.data(), static_cast<int>(idx.size()), items, cus, begins.data());
    CHECK(parts >= 0 && parts <= kCutMaxParts);
    begins.resize(parts ? parts + 1 : 0);
    if (print) {
        printf("%llu %d %zu", static_cast<unsigned long long>(items), cus, idx.size());
        for (const uint32_t v : idx) printf(" %u", v);
        printf(" | %d", parts);
        for (const int b : begins) printf(" %d", b);
        printf("\n");
        g_cases++;
    }
    return begins;
}

static std::vector<uint32_t> range(uint32_t a, uint32_t b, uint32_t step = 1)
{
    std::vector<uint32_t> v;
    for (uint32_t i = a; i < b; i += step) v.push_back(i);
    return v;
}

static std::vector<uint32_t> without(std::vector<uint32_t> v, const std::vector<uint32_t> &drop)
{
    std::vector<uint32_t> out;
    for (const uint32_t x : v) {
        bool gone = false;
        for (const uint32_t d : drop) gone |= d == x;
        if (!gone) out.push_back(x);
    }
    return out;
}

static void check_invariants(const std::vector<uint32_t> &idx, uint64_t items, int cus)
{
    const int C = static_cast<int>(idx.size());
    const std::vector<int> begins = pieces(idx, items, cus);
    CohortStreams st;
    CHECK(cohort_streams(idx.data(), C, 4 * C, st) == kCohortStreamsOk);
    const int rule = cohort_cut_parts(C, items, cus);
    if (st.runs > kCutMaxParts || !rule) { CHECK(begins.empty()); return; }
    const int parts = static_cast<int>(begins.size()) - 1;
    CHECK(parts >= st.runs && parts >= 1 && parts <= kCutMaxParts);
    CHECK(C + parts <= kCohortMaxStreams && C + parts <= kCutMaxStreams);
    CHECK(begins[0] == 0 && begins[parts] == C);
    if (st.runs > 1) CHECK(parts >= 2);
    if (parts > st.runs) CHECK(parts <= rule);                 // (the rule splits runs only up to its own count)
    for (int p = 0; p < parts; p++) {
        CHECK(begins[p + 1] > begins[p]);
        // a piece is one run of consecutive indices
        for (int v = begins[p] + 1; v < begins[p + 1]; v++) CHECK(idx[v] == idx[v - 1] + 1u);
    }
    // every run boundary is a piece boundary, and a run that was split keeps kCutMinOutputs clients per piece
    for (int v = 1; v < C; v++) {
        if (idx[v] == idx[v - 1] + 1u) continue;
        bool found = false;
        for (int p = 1; p < parts; p++) found |= begins[p] == v;
        CHECK(found);
    }
    for (int p = 0; p + 1 < parts; p++) {
        const bool inside = idx[begins[p + 1]] == idx[begins[p + 1] - 1] + 1u;      // a cut of the rule's, not a gap
        if (inside) CHECK(begins[p + 1] - begins[p] >= kCutMinOutputs && begins[p + 2] - begins[p + 1] >= kCutMinOutputs);
    }
}

int main()
{
    // one run: exactly today's rule, whatever the first index
    const uint64_t item_counts[] = {1, 2, 6, 100, 484, 1024, 2048, 2050, 3000, 4096, 8191, 100000};
    for (int C = 1; C <= kCutMaxClients; C++)
        for (const uint64_t items : item_counts)
            for (const int cus : {8, 256}) {
                const std::vector<int> begins = pieces(range(7, 7 + C), items, cus, C % 9 == 1);
                const int parts = cohort_cut_parts(C, items, cus);
                CHECK(parts >= 1 && static_cast<int>(begins.size()) == parts + 1);
                for (int p = 0; p <= parts; p++) CHECK(begins[p] == cohort_cut_begin(C, parts, p));
            }
    // the pinned examples on 256 CUs
    using V = std::vector<int>;
    CHECK(pieces({0, 2}, 6, 256) == V({0, 1, 2}));
    CHECK(pieces({0, 1, 3, 4}, 6, 256) == V({0, 2, 4}));
    CHECK(pieces(without(range(0, 41), {24}), 6, 256) == V({0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40}));
    const std::vector<uint32_t> lenet = without(range(0, 100), {3, 40, 41, 77, 99});
    CHECK(pieces(lenet, 484, 256) == V({0, 3, 15, 27, 39, 56, 74, 84, 95}));
    CHECK(pieces(lenet, 3000, 256) == V({0, 3, 39, 74, 95}));
    CHECK(pieces(range(0, 32, 2), 6, 256) == V({0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16}));
    CHECK(pieces(range(0, 34, 2), 6, 256).empty());                                       // seventeen runs
    // the refusals
    CHECK(pieces({3, 2, 5}, 6, 256).empty() && pieces({2, 2, 5}, 6, 256).empty());        // unsorted, duplicate
    CHECK(pieces({5, 0xffffffffu}, 6, 256).empty() && pieces({0xfffffffeu, 0xffffffffu}, 6, 256).empty());
    CHECK(pieces({0xfffffffdu, 0xfffffffeu}, 6, 256) == V({0, 2}));                       // (its last stream is 2^32 - 1: fits)
    CHECK(pieces(range(0, 129), 6, 256).empty());                                         // 129 clients
    CHECK(pieces({1, 2, 3}, 0, 256).empty() && pieces({1, 2, 3}, 6, 0).empty());
    {
        int begins[kCutMaxParts + 1];
        const uint32_t one[] = {4};
        CHECK(cohort_cut_pieces(nullptr, 1, 6, 256, begins) == 0 && cohort_cut_pieces(one, 1, 6, 256, nullptr) == 0 && cohort_cut_pieces(one, 0, 6, 256, begins) == 0);
        CHECK(cohort_cut_pieces(one, 1, 6, 256, begins) == 1 && begins[0] == 0 && begins[1] == 1);
    }
    // a fixed-seed fuzz over federations with dropped clients
    uint64_t state = 0x9e3779b97f4a7c15ull;
    auto next = [&state]() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; };
    for (int t = 0; t < 3000; t++) {
        const int fed = 1 + static_cast<int>(next() % 160);
        const uint32_t base = (t % 7 == 0) ? 0xffffffffu - 1u - static_cast<uint32_t>(fed) : static_cast<uint32_t>(next() % 1000);
        const unsigned keep = 1 + static_cast<unsigned>(next() % 16);          // keep a client with probability keep / 16
        std::vector<uint32_t> idx;
        for (int i = 0; i < fed && static_cast<int>(idx.size()) < kCutMaxClients; i++)
            if (next() % 16 < keep) idx.push_back(base + static_cast<uint32_t>(i));
        if (idx.empty()) idx.push_back(base);
        check_invariants(idx, item_counts[next() % 12], (t & 1) ? 256 : 80);
    }
    // 128 clients in sixteen runs: 144 streams, the table's limit
    {
        std::vector<uint32_t> idx;
        for (uint32_t r = 0; r < 16; r++)
            for (uint32_t i = 0; i < 8; i++) idx.push_back(r * 9 + i);
        check_invariants(idx, 6, 256);
        CHECK(pieces(idx, 6, 256, false).size() == 17);
    }
    printf("COHORT_CUT_PIECES_OK %ld cases\n", g_cases);
    return 0;
}
