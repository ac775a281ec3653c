// Host check of what the prepared cohort launch that generates its own PCG64 / PCG64DXSM draws added to flashe_amd/csrc/pcg64_stream.h
// (client_plan, cohort_plans, the RunTable, workgroup_jump, lane_jump, stride_jump, next_pass, run_words, run_word, lane_draws) and of the
// tiling walk draw_segments.h now states for both kinds (cohort_stretches), built with -fsanitize=address,undefined by
// tests/test_prepared_pcg64_host.py.  Every client's plan -- from one segment shared by all clients, from a segment per client in any
// table order, from a generator continued over several segments -- and the lane walk over it against a generator written here that steps
// ONE draw at a time with the compiler's own 128-bit multiply: both variants, an even inc, a state of 2^128 - 1, client offsets of every
// residue mod 4, grids of 1, 3 and 2048 workgroups over three passes, lanes of the first, a middle and the last workgroup; then the
// refusals of a table: gap, overlap, overrun, split client, mixed variants, too many draws, a variant that is neither.
#include "pcg64_stream.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace flashe_pcg64;

#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

// NumPy's pcg64_next64 / pcg64_cm_next64, step by step
struct Walker {
    u128 state, inc;
    uint32_t variant;
    uint64_t next()
    {
        if (variant == kPcg64) {
            state = state * ((static_cast<u128>(0x2360ED051FC65DA4ull) << 64) | 0x4385DF649FCCF645ull) + inc;
            const uint64_t hi = static_cast<uint64_t>(state >> 64), lo = static_cast<uint64_t>(state), x = hi ^ lo;
            const unsigned rot = static_cast<unsigned>(state >> 122);
            return rot ? (x >> rot) | (x << (64 - rot)) : x;
        }
        uint64_t hi = static_cast<uint64_t>(state >> 64);
        const uint64_t lo = static_cast<uint64_t>(state) | 1;
        state = state * static_cast<u128>(0xDA942042E4DD58B5ull) + inc;
        hi ^= hi >> 32;
        hi *= 0xDA942042E4DD58B5ull;
        hi ^= hi >> 48;
        hi *= lo;
        return hi;
    }
};

static const u128 kAll = ~static_cast<u128>(0);
static long g_draws = 0, g_lanes = 0;

static Segment segment_of(const Walker &w, uint64_t n, uint64_t offset) { return Segment{w.state, w.inc, w.variant, n, offset}; }

static const Pow2Table kPow2[kVariants] = {make_pow2_table(kPcg64), make_pow2_table(kDxsm)};
static const RunTable kRuns[kVariants] = {make_run_table(kPcg64), make_run_table(kDxsm)};

// The lane that owns run `run` of a grid of `workgroups`, over `passes` passes under plan p, against the draws of the client (want: its
// stretch from its first draw on, one walker draw each): run_words through lane_draws, and run_word's indexing of the same runs.
static void check_lane(const ClientPlan &p, uint32_t variant, const std::vector<double> &want, uint64_t workgroups, uint64_t run, uint64_t passes)
{
    std::vector<double> got(kRunDraws * passes);
    if (variant == kPcg64) lane_draws<kPcg64>(kPow2[0], kRuns[0], p, workgroups, run, passes, got.data());
    else lane_draws<kDxsm>(kPow2[1], kRuns[1], p, workgroups, run, passes, got.data());
    const Jump stride = stride_jump(static_cast<Variant>(variant), workgroups);
    Jump j = lane_jump(workgroup_jump(kPow2[variant], run / kLanes), kRuns[variant].row[run % kLanes]);
    const u128 o = make128(p.origin[1], p.origin[0]), inc = make128(p.inc[1], p.inc[0]);
    for (uint64_t pass = 0; pass < passes; pass++) {
        const uint64_t k0 = kRunDraws * (run + kLanes * workgroups * pass);
        for (uint32_t i = 0; i < kRunDraws; i++) {
            CHECK(k0 + i < want.size());
            CHECK(got[kRunDraws * pass + i] == want[k0 + i]);
            const uint64_t w = variant == kPcg64 ? run_word<kPcg64>(j, o, inc, i) : run_word<kDxsm>(j, o, inc, i);
            CHECK(to_double(w) == want[k0 + i]);
            g_draws++;
        }
        j = next_pass(j, stride);
    }
    g_lanes++;
}

// client c's plan of a table against the walker that stands at the client's first draw
static void check_client(const ClientPlan &p, Walker w, uint64_t workgroups, uint64_t passes)
{
    CHECK(p.inc[0] == lo64(w.inc) && p.inc[1] == hi64(w.inc));
    const u128 first = w.variant == kPcg64 ? w.state * multiplier(kPcg64) + w.inc : w.state;       // the state the first draw outputs from
    CHECK(p.origin[0] == lo64(first) && p.origin[1] == hi64(first));
    const uint64_t runs = kLanes * workgroups, draws = kRunDraws * runs * passes;
    std::vector<double> want(draws);
    for (uint64_t k = 0; k < draws; k++) want[k] = to_double(w.next());
    const uint64_t lanes[] = {0, 1, 63, 64, kLanes - 1, runs / 2 + 7 < runs ? runs / 2 + 7 : 0, runs - kLanes, runs - 2, runs - 1};
    for (const uint64_t run : lanes) check_lane(p, w.variant, want, workgroups, run, passes);
}

static void check_tables(uint32_t variant, u128 state, u128 inc, uint64_t pre, uint64_t n, uint64_t workgroups)
{
    const uint64_t C = 5, passes = 3;
    Walker g{state, inc, variant};
    for (uint64_t i = 0; i < pre; i++) g.next();
    std::vector<ClientPlan> plans;
    // one segment shared by all clients: client c starts c n draws in -- with n % 4 == 1 every residue mod 4
    {
        const Segment s = segment_of(g, C * n, 0);
        CHECK(check_segments(&s, 1) == kSegmentsOk);
        Variant v = kVariants;
        CHECK(cohort_plans(&s, 1, C, n, plans, &v) == kCohortPlansOk && plans.size() == C && v == variant);
        Walker w = g;
        for (uint64_t c = 0; c < C; c++) {
            check_client(plans[c], w, workgroups, c < 2 || workgroups < 100 ? passes : 0);
            for (uint64_t k = 0; k < n; k++) w.next();
        }
    }
    // a segment per client in another table order, client c's generator c + 1 draws further than client 0's; an empty segment between
    {
        std::vector<Walker> ws(C, g);
        std::vector<Segment> segs;
        const uint64_t order[] = {3, 0, 4, 1, 2};
        for (uint64_t c = 0; c < C; c++)
            for (uint64_t i = 0; i < c + (c > 0); i++) ws[c].next();
        for (const uint64_t c : order) {
            segs.push_back(segment_of(ws[c], n, c * n));
            if (c == 4) segs.push_back(segment_of(ws[c], 0, 77));
        }
        CHECK(check_segments(segs.data(), static_cast<int>(segs.size())) == kSegmentsOk);
        CHECK(cohort_plans(segs.data(), static_cast<int>(segs.size()), C, n, plans) == kCohortPlansOk && plans.size() == C);
        for (uint64_t c = 0; c < C; c++) check_client(plans[c], ws[c], workgroups, c == 3 || workgroups < 100 ? passes : 0);
    }
    // one generator continued over two segments of two and three clients (the second starts where advance leaves the first)
    {
        Segment segs[2] = {segment_of(g, 2 * n, 0), segment_of(g, 3 * n, 2 * n)};
        segs[1].state = advance(static_cast<Variant>(variant), g.state, g.inc, 2 * n);
        Walker w = g;
        for (uint64_t k = 0; k < 2 * n; k++) w.next();
        CHECK(w.state == segs[1].state);
        CHECK(cohort_plans(segs, 2, C, n, plans) == kCohortPlansOk && plans.size() == C);
        w = g;
        for (uint64_t c = 0; c < C; c++) {
            check_client(plans[c], w, workgroups, c == 2 || workgroups < 100 ? passes : 0);
            for (uint64_t k = 0; k < n; k++) w.next();
        }
    }
}

static void check_refusals()
{
    const Walker a{12345, 7, kPcg64}, d{999, 8, kDxsm};
    const uint64_t n = 1001;
    std::vector<ClientPlan> plans;
    auto status = [&](std::vector<Segment> segs, uint64_t C, uint64_t each) {
        CHECK(check_segments(segs.data(), static_cast<int>(segs.size())) == kSegmentsOk);
        const CohortPlansStatus st = cohort_plans(segs.data(), static_cast<int>(segs.size()), C, each, plans);
        CHECK(st == kCohortPlansOk || plans.empty());
        return st;
    };
    CHECK(status({segment_of(a, n, 0), segment_of(a, n, n)}, 2, n) == kCohortPlansOk && plans.size() == 2);
    CHECK(status({segment_of(a, n, 0), segment_of(a, n, n + 1)}, 2, n) == kCohortPlansNotTiled);          // a gap (and an overrun)
    CHECK(status({segment_of(a, n - 1, 0), segment_of(a, n, n)}, 2, n) == kCohortPlansNotTiled);          // a gap inside
    CHECK(status({segment_of(a, n, 0), segment_of(a, n + 1, n)}, 2, n) == kCohortPlansNotTiled);          // beyond C n
    CHECK(status({segment_of(a, 2 * n - 1, 0)}, 2, n) == kCohortPlansNotTiled);
    CHECK(status({segment_of(a, 2 * n + 1, 0)}, 2, n) == kCohortPlansNotTiled);
    CHECK(status({segment_of(a, n, n)}, 2, n) == kCohortPlansNotTiled);                                   // nothing at 0
    CHECK(status({segment_of(a, n + 1, 0), segment_of(a, n - 1, n + 1)}, 2, n) == kCohortPlansSplitClient);
    CHECK(status({segment_of(a, n, 0), segment_of(d, n, n)}, 2, n) == kCohortPlansMixedVariants);
    CHECK(status({segment_of(d, n, n), segment_of(a, n, 0)}, 2, n) == kCohortPlansMixedVariants);
    CHECK(status({segment_of(a, 2 * n, 0), segment_of(d, 0, 5)}, 2, n) == kCohortPlansOk);                // (an empty segment draws nothing: no variant)
    CHECK(status({segment_of(d, n, 0), segment_of(d, n, n)}, 2, n) == kCohortPlansOk);
    CHECK(status({segment_of(a, n, 0), segment_of(d, n + 1, n)}, 2, n) == kCohortPlansNotTiled);          // the tiling comes first
    CHECK(status({segment_of(a, kMaxDraws, 0)}, 2, kMaxDraws / 2 + 1) == kCohortPlansTooMany);
    CHECK(status({segment_of(a, 0, 0), segment_of(d, 0, 9)}, 3, 0) == kCohortPlansOk && plans.empty());   // n = 0
    CHECK(status({segment_of(a, 1, 0)}, 3, 0) == kCohortPlansNotTiled);
    CHECK(status({}, 0, n) == kCohortPlansOk && plans.empty());
    // an overlap and a variant that is neither are check_segments' to find
    const Segment over[2] = {segment_of(a, n, 0), segment_of(a, n, n - 1)};
    CHECK(check_segments(over, 2) == kSegmentsOverlap);
    Segment bad = segment_of(a, n, 0);
    bad.variant = 2;
    CHECK(check_segments(&bad, 1) == kSegmentsBadVariant);
}

int main()
{
    static_assert(sizeof(ClientPlan) == 32, "four 64-bit words");
    const u128 states[] = {0, make128(0x0123456789ABCDEFull, 0xFEDCBA9876543210ull), kAll};
    const u128 incs[] = {make128(0x5851F42D4C957F2Dull, 0x14057B7EF767814Full), make128(0x9E3779B97F4A7C15ull, 0xF39CC0605CEDC834ull) & ~static_cast<u128>(1), 0};
    for (uint32_t variant = 0; variant < kVariants; variant++) {
        // the RunTable's rows and the workgroup's jump against the doubling
        for (uint64_t t = 0; t < kLanes; t += 37) {
            const Jump a = from_row(kRuns[variant].row[t]), b = jump(static_cast<Variant>(variant), kRunDraws * t);
            CHECK(a.mul == b.mul && a.add == b.add);
        }
        for (const uint64_t wg : {0ull, 1ull, 2ull, 1023ull, 2047ull, 123456789ull}) {
            const Jump a = workgroup_jump(kPow2[variant], wg), b = jump(static_cast<Variant>(variant), static_cast<u128>(kRunDraws * kLanes) * wg);
            CHECK(a.mul == b.mul && a.add == b.add);
        }
        for (const u128 state : states)
            for (const u128 inc : incs)
                for (const uint64_t workgroups : {1ull, 3ull})
                    check_tables(variant, state, inc, state == kAll ? 3 : 0, 1001, workgroups);
        check_tables(variant, states[1], incs[1], 5, 1001, 2048);                            // (an even inc on the widest grid)
    }
    check_refusals();
    printf("PREPARED_PCG64_OK %ld draws of %ld lanes\n", g_draws, g_lanes);
    return 0;
}
