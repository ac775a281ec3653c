// A table of output segments of a device draw call, stated once for the generator kinds (philox_stream.h, pcg64_stream.h): a segment gives
// n draws of one generator state to draws [offset, offset + n) of the output buffer.  Here is what does not depend on the kind: the limits,
// the word -> double step, the check of the ranges and the search that finds a tile's segment in the launch's plan table.  No HIP header:
// the stream headers run on the host under sanitizers, and the .hip files compile the same functions for the device through FLASHE_HD.
#pragma once
#include <cstddef>
#include <cstdint>
#include <algorithm>
#include <vector>

#ifndef FLASHE_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define FLASHE_HD __host__ __device__ __forceinline__
#else
#define FLASHE_HD inline
#endif
#endif
#ifdef __clang__
#define FLASHE_UNROLL _Pragma("unroll")
#else
#define FLASHE_UNROLL
#endif

namespace flashe_draw {

constexpr int kMaxSegments = 128;                   // the segments one launch holds
constexpr uint64_t kMaxDraws = 1ull << 60;          // per segment, and offset + n: their byte counts stay inside 64 bits

// Generator.random's double of a 64-bit word
FLASHE_HD double to_double(uint64_t word) { return static_cast<double>(word >> 11) * (1.0 / 9007199254740992.0); }

// kSegmentsOwn is the kind's own refusal, which it names itself (kSegmentsBadPos, kSegmentsBadVariant).
enum SegmentsStatus { kSegmentsOk = 0, kSegmentsBadCount = 1, kSegmentsOwn = 2, kSegmentsOverflow = 3, kSegmentsOverlap = 4 };

// kSegmentsBadCount: n_segments < 0 or more than max_segments (or a null table with segments); kSegmentsOwn: own_ok(segment), the kind's
// check of one segment, is false -- it comes before that segment's range; kSegmentsOverflow: an n, an offset or offset + n above
// kMaxDraws; kSegmentsOverlap: two non-empty output ranges share a draw.
template <class Segment, class OwnOk> inline SegmentsStatus check_segments(const Segment *segs, int n_segments, int max_segments, OwnOk own_ok)
{
    if (n_segments < 0 || n_segments > max_segments || (n_segments && !segs)) return kSegmentsBadCount;
    std::vector<std::pair<uint64_t, uint64_t>> ranges;
    for (int s = 0; s < n_segments; s++) {
        if (!own_ok(segs[s])) return kSegmentsOwn;
        if (segs[s].n > kMaxDraws || segs[s].offset > kMaxDraws || segs[s].offset + segs[s].n > kMaxDraws) return kSegmentsOverflow;
        if (segs[s].n) ranges.emplace_back(segs[s].offset, segs[s].offset + segs[s].n);
    }
    std::sort(ranges.begin(), ranges.end());
    for (size_t r = 1; r < ranges.size(); r++)
        if (ranges[r].first < ranges[r - 1].second) return kSegmentsOverlap;
    return kSegmentsOk;
}

// The segment of tile t of a launch: the last plan whose first tile is not above t (plans[0].tile_first is 0).
template <class Plan> FLASHE_HD const Plan &tile_plan(const Plan *plans, int n_plans, uint64_t t)
{
    int lo = 0, hi = n_plans - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (plans[mid].tile_first <= t) lo = mid; else hi = mid - 1;
    }
    return plans[lo];
}

// ---- the draws of a cohort generated inside the launch that consumes them: the walk the kinds share ----
// kCohortPlansOwn is the kind's own refusal, which it names itself (pcg64_stream.h: kCohortPlansMixedVariants).
enum CohortPlansStatus { kCohortPlansOk = 0, kCohortPlansTooMany = 1, kCohortPlansNotTiled = 2, kCohortPlansSplitClient = 3, kCohortPlansOwn = 4 };

// n_clients clients of n draws each from checked segments (check_segments: no overlap, nothing overflows): the non-empty segments must tile
// the client-major draws [0, n_clients n) exactly -- no gap, nothing beyond (kCohortPlansNotTiled; an overlap is check_segments' to find)
// -- and every client's stretch [c n, (c + 1) n) must lie inside ONE segment, since a client has one plan (kCohortPlansSplitClient).
// kCohortPlansTooMany: n_clients n above kMaxDraws.  tiled() is asked once the tiling holds (the kind's own refusal of the table as a whole: its
// status is returned unless it is kCohortPlansOk); emit(segment, first) is then called for every client in order: its stretch starts
// `first` draws into that segment.  n = 0: every segment must be empty; nothing is emitted.
template <class Segment, class Tiled, class Emit>
inline CohortPlansStatus cohort_stretches(const Segment *segs, int n_segments, uint64_t n_clients, uint64_t n, Tiled tiled, Emit emit)
{
    if (n && n_clients > kMaxDraws / n) return kCohortPlansTooMany;
    const uint64_t total = n_clients * n;
    std::vector<int> order;
    for (int s = 0; s < n_segments; s++)
        if (segs[s].n) order.push_back(s);
    std::sort(order.begin(), order.end(), [&](int a, int b) { return segs[a].offset < segs[b].offset; });
    uint64_t at = 0;
    for (const int s : order) {
        if (segs[s].offset != at) return kCohortPlansNotTiled;
        at += segs[s].n;
    }
    if (at != total) return kCohortPlansNotTiled;
    if (const CohortPlansStatus own = tiled()) return own;
    if (!n) return kCohortPlansOk;
    size_t i = 0;
    for (uint64_t c = 0; c < n_clients; c++) {                   // (a client that no segment holds whole is found before anything of it is emitted)
        const uint64_t first = c * n;
        while (segs[order[i]].offset + segs[order[i]].n <= first) i++;
        const Segment &s = segs[order[i]];
        if (first + n > s.offset + s.n) return kCohortPlansSplitClient;
        emit(s, first - s.offset);
    }
    return kCohortPlansOk;
}

}  // namespace flashe_draw
