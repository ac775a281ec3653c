// The cut of a SHORT cohort's summed chain: into how many runs of consecutive clients one launch cuts a cohort whose vector does not fill
// the chip uncut, and which clients each run holds.  No HIP header, so that tests/host_cohort_cut_check.cpp runs it on the host under
// sanitizers (as cohort_streams.h is); flashe_amd/block.py mirrors it (cohort_cut_parts) and tests/test_cohort_cut_host.py holds the two
// against each other.
//   Piece p of `parts` holds clients [C p / parts, C (p + 1) / parts): every piece is its own double-mask chain over the SAME elements, so
//   a cut costs one PRF stream (the stream at the cut is computed by both neighbours: C + parts streams instead of C + 1).  Each piece
//   writes the sum of its own outputs and its own decrypt mask S(b_p) - S(a_p); one memory-bound pass adds them up:
//     sum_c out_c = sum_p (piece p's sum),   sum_p (S(b_p) - S(a_p)) = S(last) - S(first)   (b_p = a_{p+1}: the masks telescope).
//   The rule: as many pieces as fill the chip ONCE -- the largest count whose items do not outnumber the chip's waves --, never fewer
//   than four outputs per piece, at most kCutMaxParts pieces, at most C.  An ITEM is two AES blocks per lane and stream: a half tile of
//   128 elements in the wide layout (int_bits > 64), a tile of 128 AES blocks in the compact one (int_bits <= 32).  From half an item
//   per wave upward the launch is not cut (parts = 1: it writes the sum and the mask where they belong and no combine pass runs).
//   It started from launch_prf_chains' rule for short unsummed chains (the nearest count to 1.15 items per wave) and was changed on
//   the measurement (tests/perf/cut_cohort_step.py, profiles/r30_cut_cohort_step_rule115.log: 61,706 x 100 at int_bits 128, 484 items against
//   4,096 waves): 10 pieces, what 1.15 gave, ran 0.319 ms, 8 pieces 0.289, 12 0.294, 16 0.290, 4 0.337.  A wave's time is the items it
//   gets times the streams of an item, ceil(items parts / waves) (C / parts + 1): 14, 16, 20, 22 and 26 for 8, 16, 12, 10 and 4 pieces,
//   the order measured -- one item more than the chip has waves doubles it.
#pragma once
#include <cstdint>

namespace flashe_tables {

constexpr int kCutMaxParts = 16;         // chains of one launch (kMaxChains, kernels.hip)
constexpr int kCutMaxClients = 128;      // outputs of one launch (kMaxLinks, kernels.hip)
constexpr int kCutWavesPerCu = 16;       // the chained kernels run 1,024-thread workgroups, one per CU
constexpr int kCutMinOutputs = 4;        // outputs of a piece at the least (a cut costs one stream)

// the items of one uncut chain: half tiles of the n-element vector (wide), tiles of its `blocks` AES blocks (compact)
inline uint64_t cohort_cut_items_wide(uint64_t n) { return 2 * ((n + 255) / 256); }
inline uint64_t cohort_cut_items_compact(uint64_t blocks) { return (blocks + 127) / 128; }

// pieces of a cohort of n_clients (1 .. kCutMaxClients) whose uncut chain has `items` items (>= 1) on a chip of num_cus CUs; 0 = not a
// shape of the cut launch
inline int cohort_cut_parts(int n_clients, uint64_t items, int num_cus)
{
    if (n_clients < 1 || n_clients > kCutMaxClients || items < 1 || num_cus < 1) return 0;
    const uint64_t waves = static_cast<uint64_t>(num_cus) * kCutWavesPerCu;
    uint64_t parts = waves / items;                                   // the most pieces whose items every wave takes at most one of
    const uint64_t cap = n_clients / kCutMinOutputs > 1 ? static_cast<uint64_t>(n_clients / kCutMinOutputs) : 1;
    if (parts > cap) parts = cap;
    if (parts > static_cast<uint64_t>(kCutMaxParts)) parts = kCutMaxParts;
    if (parts < 1) parts = 1;
    return static_cast<int>(parts);
}

// the first client of piece p (p = parts: one past the last client)
inline int cohort_cut_begin(int n_clients, int parts, int p)
{
    return static_cast<int>(static_cast<int64_t>(n_clients) * p / parts);
}

// does the wide launch run entirely in half tiles?  (fewer than two whole tiles per wave, all pieces together)
inline bool cohort_cut_all_half(uint64_t n, int parts, int num_cus)
{
    return ((n + 255) / 256) * static_cast<uint64_t>(parts) < 2 * static_cast<uint64_t>(num_cus) * kCutWavesPerCu;
}

// ---- pieces that respect RUNS: a round in which clients dropped out (any strictly ascending cipher indices) ----
// A gap in the cipher indices is a cut the round imposes: a run of consecutive present clients [a .. b] is by itself a chain over streams
// a .. b + 1, and the pieces' masks S(b_p + 1) - S(a_p) add up to the decrypt mask of the telescoped lists (jzf_flashe.py:356-367) whether
// the cuts come from gaps or from the rule above.  So: every run starts as one piece; while the pieces number fewer than
// max(runs, cohort_cut_parts(...)) the run with the most clients per piece takes one more (compared as len_r k_best > len_best k_r, the
// lower run on a tie), as long as its pieces keep kCutMinOutputs clients (len / (k + 1), rounded down); inside a run of k pieces that
// starts at position a, piece q begins at a + len q / k.  One run gives exactly cohort_cut_parts / cohort_cut_begin.  More runs than
// kCutMaxParts do not fit one table: 0, as for every shape cohort_cut_parts declines and for indices that are not strictly ascending or
// hold 2^32 - 1 (cohort_streams.h).  A gapped cohort never has one piece: it always runs the combine pass.
// (The tie-break and the floor for split runs are first guesses: tests/perf/cut_cohort_any_step.py times the 16-run shape.)
constexpr int kCutMaxStreams = kCutMaxClients + kCutMaxParts;      // kCohortMaxStreams (cohort_streams.h): C + pieces never exceeds it

// idx[0 .. n_clients) -> begins[0 .. parts] (the first present-client POSITION of every piece, begins[parts] = n_clients); returns parts.
// begins holds kCutMaxParts + 1 entries.
inline int cohort_cut_pieces(const uint32_t *idx, int n_clients, uint64_t items, int num_cus, int *begins)
{
    const int rule = cohort_cut_parts(n_clients, items, num_cus);
    if (!idx || !begins || !rule) return 0;
    int start[kCutMaxParts + 1], k[kCutMaxParts], runs = 0;
    for (int v = 0; v < n_clients; v++) {
        if (idx[v] == 0xffffffffu || (v && idx[v] <= idx[v - 1])) return 0;
        if (v == 0 || idx[v] != idx[v - 1] + 1u) {
            if (runs == kCutMaxParts) return 0;
            start[runs] = v; k[runs] = 1; runs++;
        }
    }
    start[runs] = n_clients;
    const int want = rule > runs ? rule : runs;
    for (int pieces = runs; pieces < want; pieces++) {
        int best = -1;
        for (int r = 0; r < runs; r++) {
            const int len = start[r + 1] - start[r];
            if (len / (k[r] + 1) < kCutMinOutputs) continue;
            if (best < 0 || static_cast<int64_t>(len) * k[best] > static_cast<int64_t>(start[best + 1] - start[best]) * k[r]) best = r;
        }
        if (best < 0) break;
        k[best]++;
    }
    int parts = 0;
    for (int r = 0; r < runs; r++) {
        const int len = start[r + 1] - start[r];
        for (int q = 0; q < k[r]; q++) begins[parts++] = start[r] + static_cast<int>(static_cast<int64_t>(len) * q / k[r]);
    }
    begins[parts] = n_clients;
    return parts;
}

}  // namespace flashe_tables
