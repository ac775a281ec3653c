// The PRF streams of a cohort round in which some clients dropped out: which streams a strictly ascending list P of cipher indices
// needs, which of them complete an output and which open a run.  No HIP header, so that tests/host_cohort_streams_check.cpp runs it on
// the host under sanitizers (as layer_tables.h is).
//   S = { s : s in P or s - 1 in P }, ascending: |P| + runs streams (consecutive clients share one), not 2 |P|;
//   stream s COMPLETES client s - 1's output when s - 1 in P: ct = pt + term(s - 1) - term(s) (jzf_flashe.py:349-354) -- the stream
//     before it in S is then s - 1;
//   stream s OPENS a client when s in P;
//   the decrypt mask is D = sum over (completes, not opens) term(s) - sum over (opens, not completes) term(s): what a decrypt with the
//     lists of telescope(P) (jzf_flashe.py:356-367) adds to the sum of the ciphertexts.
// Streams strictly inside a dropped run of two or more clients are in neither set and are not computed.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace flashe_tables {

// The streams one chained launch holds: its ChainTable has kMaxLinks + kMaxChains = 128 + 16 prefix slots (kernels.hip asserts the sum), so
// 128 present clients may form up to 16 runs, and fewer clients more (|P| + runs <= 144).
constexpr int kCohortMaxStreams = 144;

constexpr uint8_t kStreamCompletes = 1, kStreamOpens = 2;

struct CohortStreams {
    std::vector<uint32_t> idx;      // S, ascending
    std::vector<uint8_t> bits;      // kStreamCompletes | kStreamOpens of every stream
    std::vector<int> link;          // the position in P of the client whose output the stream completes, -1 where it completes none
    int runs = 0;                   // runs of consecutive indices in P
};

enum CohortStreamsStatus { kCohortStreamsOk = 0, kCohortStreamsBadIdx = 1, kCohortStreamsTooMany = 2 };

// P[0 .. n_present) -> out.  kCohortStreamsBadIdx: n_present < 1, an index that is not above the one before it (unsorted or duplicate), or
// an index of 2^32 - 1 (its closing stream 2^32 does not fit the 4-byte prefix field); kCohortStreamsTooMany: more than max_streams
// streams.  out is only valid with kCohortStreamsOk.
inline CohortStreamsStatus cohort_streams(const uint32_t *P, int n_present, int max_streams, CohortStreams &out)
{
    out.idx.clear(); out.bits.clear(); out.link.clear(); out.runs = 0;
    if (!P || n_present < 1) return kCohortStreamsBadIdx;
    for (int v = 0; v < n_present; v++) {
        if (P[v] == 0xffffffffu) return kCohortStreamsBadIdx;
        if (v && P[v] <= P[v - 1]) return kCohortStreamsBadIdx;
    }
    for (int v = 0; v < n_present; v++) {
        const bool run_start = v == 0 || P[v] != P[v - 1] + 1u, run_end = v + 1 == n_present || P[v + 1] != P[v] + 1u;
        // the client's own stream: it opens the client, and completes the one before it inside a run
        out.idx.push_back(P[v]);
        out.bits.push_back(static_cast<uint8_t>(kStreamOpens | (run_start ? 0 : kStreamCompletes)));
        out.link.push_back(run_start ? -1 : v - 1);
        if (run_start) out.runs++;
        if (run_end) {
            out.idx.push_back(P[v] + 1u);
            out.bits.push_back(kStreamCompletes);
            out.link.push_back(v);
        }
        if (out.idx.size() > static_cast<size_t>(max_streams)) return kCohortStreamsTooMany;
    }
    return kCohortStreamsOk;
}

}  // namespace flashe_tables
