// Host check of flashe_amd/csrc/cohort_streams.h (the stream table of a cohort round with dropped-out clients), built with
// -fsanitize=address,undefined by tests/test_cohort_streams_host.py.  Every non-empty subset of ten clients, at first_idx 0 and
// 2^32 - 12, against a brute-force closed form written here on its own (membership tests over 64-bit indices, no run analysis), then the
// refusals.
#include "cohort_streams.h"

#include <cstdio>
#include <cstdlib>
#include <set>

using namespace flashe_tables;

#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

static long g_cases = 0;

static void check_subset(uint32_t first_idx, unsigned subset)
{
    std::vector<uint32_t> P;
    std::set<uint64_t> in;
    for (int c = 0; c < 10; c++)
        if (subset >> c & 1u) { P.push_back(first_idx + static_cast<uint32_t>(c)); in.insert(static_cast<uint64_t>(first_idx) + c); }
    CohortStreams t;
    CHECK(cohort_streams(P.data(), static_cast<int>(P.size()), kCohortMaxStreams, t) == kCohortStreamsOk);
    // the closed form: walk every candidate index of the window (64-bit, so that 2^32 - 1 + 1 does not wrap)
    std::vector<uint64_t> S;
    std::vector<int> completes, opens;
    int runs = 0;
    for (uint64_t s = first_idx; s <= static_cast<uint64_t>(first_idx) + 10; s++) {
        const bool op = in.count(s) != 0, co = s > 0 && in.count(s - 1) != 0;
        if (!op && !co) continue;
        S.push_back(s); completes.push_back(co); opens.push_back(op);
        if (op && !co) runs++;
    }
    CHECK(t.idx.size() == S.size() && t.bits.size() == S.size() && t.link.size() == S.size());
    CHECK(t.runs == runs && S.size() == P.size() + static_cast<size_t>(runs));
    int next_link = 0, net = 0;
    for (size_t i = 0; i < S.size(); i++) {
        CHECK(t.idx[i] == S[i]);
        CHECK(((t.bits[i] & kStreamCompletes) != 0) == (completes[i] != 0));
        CHECK(((t.bits[i] & kStreamOpens) != 0) == (opens[i] != 0));
        CHECK((t.bits[i] & ~(kStreamCompletes | kStreamOpens)) == 0);
        if (completes[i]) {
            // links are finished in the order of P, by the stream one above the client's own, which is the stream before it in S
            CHECK(t.link[i] == next_link && static_cast<uint64_t>(P[next_link]) + 1 == S[i] && i > 0 && S[i - 1] + 1 == S[i]);
            next_link++;
        } else
            CHECK(t.link[i] == -1);
        // the decrypt mask's signed terms are those of the telescoped lists: + one past every run's end, - every run's start
        if (completes[i] && !opens[i]) { CHECK(in.count(S[i]) == 0 && in.count(S[i] - 1) != 0); net++; }
        if (opens[i] && !completes[i]) { CHECK(in.count(S[i]) != 0 && (S[i] == 0 || in.count(S[i] - 1) == 0)); net--; }
    }
    CHECK(next_link == static_cast<int>(P.size()) && net == 0);
    CHECK((t.bits.front() & (kStreamCompletes | kStreamOpens)) == kStreamOpens && t.bits.back() == kStreamCompletes);
    g_cases++;
}

static void check_refusals()
{
    CohortStreams t;
    const uint32_t unsorted[] = {0, 2, 1}, dup[] = {3, 3}, top[] = {5, 0xffffffffu}, last_ok[] = {5, 0xfffffffeu};
    CHECK(cohort_streams(unsorted, 3, kCohortMaxStreams, t) == kCohortStreamsBadIdx);
    CHECK(cohort_streams(dup, 2, kCohortMaxStreams, t) == kCohortStreamsBadIdx);
    CHECK(cohort_streams(top, 2, kCohortMaxStreams, t) == kCohortStreamsBadIdx);
    CHECK(cohort_streams(top, 0, kCohortMaxStreams, t) == kCohortStreamsBadIdx);
    CHECK(cohort_streams(nullptr, 1, kCohortMaxStreams, t) == kCohortStreamsBadIdx);
    CHECK(cohort_streams(last_ok, 2, kCohortMaxStreams, t) == kCohortStreamsOk && t.idx.back() == 0xffffffffu && t.runs == 2);
    // 72 singletons are 144 streams; a 73rd run is one too many.  128 clients in 16 runs fit, in 17 they do not.
    std::vector<uint32_t> P;
    for (uint32_t c = 0; c < 73; c++) P.push_back(2 * c);
    CHECK(cohort_streams(P.data(), 72, kCohortMaxStreams, t) == kCohortStreamsOk && t.idx.size() == 144 && t.runs == 72);
    CHECK(cohort_streams(P.data(), 73, kCohortMaxStreams, t) == kCohortStreamsTooMany);
    for (int runs = 16; runs <= 17; runs++) {
        P.clear();
        for (uint32_t c = 0, at = 0; c < 128; c++) {
            P.push_back(at);
            at += (c % 7 == 6 && static_cast<int>(c / 7) + 1 < runs) ? 2 : 1;      // a gap behind every seventh client, runs - 1 of them
        }
        const CohortStreamsStatus rc = cohort_streams(P.data(), 128, kCohortMaxStreams, t);
        CHECK(rc == (runs == 16 ? kCohortStreamsOk : kCohortStreamsTooMany));
        if (runs == 16) CHECK(t.runs == 16 && t.idx.size() == 144);
    }
    // a smaller table
    const uint32_t two[] = {1, 2};
    CHECK(cohort_streams(two, 2, 3, t) == kCohortStreamsOk && t.idx.size() == 3);
    CHECK(cohort_streams(two, 2, 2, t) == kCohortStreamsTooMany);
}

int main()
{
    for (unsigned subset = 1; subset < 1024; subset++) {
        check_subset(0, subset);
        check_subset(0xffffffffu - 11u, subset);          // 2^32 - 12: the tenth client is 2^32 - 3, the last stream 2^32 - 2
    }
    check_refusals();
    printf("COHORT_STREAMS_OK %ld subsets\n", g_cases);
    return 0;
}
