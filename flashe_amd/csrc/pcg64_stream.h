// The streams of NumPy's np.random.PCG64 (PCG XSL-RR 128/64) and np.random.PCG64DXSM (PCG CM-DXSM 128/64) as Generator.random draws them,
// stated once: the step, the two output functions, the jump over k steps, the state after n draws, the tables the device launch jumps
// with, and the checks of a table of output segments.  No HIP header, so that tests/host_pcg64_stream_check.cpp runs it on the host under
// sanitizers (as philox_stream.h is); pcg64.hip compiles the same functions for the device through FLASHE_HD, and codec.hip those of the
// cohort launch that generates its draws itself (the last part of this file; tests/host_prepared_pcg64_check.cpp).
//   Both are the 128-bit LCG  state' = A state + inc  mod 2^128  with a 64-bit output function; inc is whatever the state holds (NumPy's
//   state setter takes any 128-bit value, an even one included), so nothing here assumes it odd.
//   PCG64:      A = 0x2360ED051FC65DA44385DF649FCCF645; a draw STEPS first and outputs from the NEW state: w = rotr64(hi ^ lo, state >> 122).
//   PCG64DXSM:  A = 0xDA942042E4DD58B5 (64 bits); a draw outputs from the OLD state, then steps:
//               lo |= 1; hi ^= hi >> 32; hi *= A; hi ^= hi >> 48; hi *= lo; w = hi.
//   draw = (w >> 11) * 2^-53.  Generator.random neither reads nor changes has_uint32 / uinteger.
// k steps are themselves an affine map:  state_k = A^k state + G_k inc,  G_k = 1 + A + ... + A^(k-1): (A^k, G_k) -- a Jump -- depends on
// the variant only, not on the generator, and is found by doubling in at most 128 rounds.  With  origin = the state the FIRST draw outputs
// from (the state stepped once for PCG64, the state itself for DXSM), draw i outputs from  A^i origin + G_i inc  for both variants.
#pragma once
#include "draw_segments.h"

namespace flashe_pcg64 {

using namespace flashe_draw;                         // kMaxSegments, kMaxDraws, to_double, SegmentsStatus and its values

typedef unsigned __int128 u128;

enum Variant : uint32_t { kPcg64 = 0, kDxsm = 1, kVariants = 2 };

constexpr uint64_t kMultHi = 0x2360ED051FC65DA4ull, kMultLo = 0x4385DF649FCCF645ull;   // PCG64's multiplier
constexpr uint64_t kCheapMult = 0xDA942042E4DD58B5ull;                                   // PCG64DXSM's, and its output function's

constexpr u128 make128(uint64_t hi, uint64_t lo) { return (static_cast<u128>(hi) << 64) | lo; }
constexpr uint64_t lo64(u128 v) { return static_cast<uint64_t>(v); }
constexpr uint64_t hi64(u128 v) { return static_cast<uint64_t>(v >> 64); }

constexpr u128 multiplier(Variant v) { return v == kPcg64 ? make128(kMultHi, kMultLo) : make128(0, kCheapMult); }

// a b mod 2^128 from one 64 x 64 -> 128 product and two 64 x 64 -> 64 ones (written out: no 128-bit multiply routine is asked of the compiler)
constexpr u128 mul(u128 a, u128 b)
{
    const u128 p = static_cast<u128>(lo64(a)) * lo64(b);
    return make128(hi64(p) + lo64(a) * hi64(b) + hi64(a) * lo64(b), lo64(p));
}

constexpr u128 step(Variant v, u128 state, u128 inc) { return mul(state, multiplier(v)) + inc; }

FLASHE_HD uint64_t output_xsl_rr(u128 state)
{
    const uint64_t x = hi64(state) ^ lo64(state);
    const unsigned rot = static_cast<unsigned>(hi64(state) >> 58);                        // state >> 122
    return (x >> rot) | (x << ((64 - rot) & 63));
}

FLASHE_HD uint64_t output_dxsm(u128 state)
{
    uint64_t hi = hi64(state);
    const uint64_t lo = lo64(state) | 1;
    hi ^= hi >> 32;
    hi *= kCheapMult;
    hi ^= hi >> 48;
    hi *= lo;
    return hi;
}

template <Variant V> FLASHE_HD uint64_t output(u128 state) { return V == kPcg64 ? output_xsl_rr(state) : output_dxsm(state); }

// k steps as one map: state -> mul state + add inc
struct Jump { u128 mul, add; };

constexpr u128 apply(const Jump &j, u128 state, u128 inc) { return mul(j.mul, state) + mul(j.add, inc); }

// first a, then b
constexpr Jump compose(const Jump &a, const Jump &b) { return Jump{mul(b.mul, a.mul), mul(b.mul, a.add) + b.add}; }

// (A^k, G_k) for any k < 2^128, by doubling: cur = the jump over 2^bit steps
constexpr Jump jump(Variant v, u128 k)
{
    Jump acc{1, 0}, cur{multiplier(v), 1};
    while (k) {
        if (k & 1) acc = compose(acc, cur);
        cur = compose(cur, cur);
        k >>= 1;
    }
    return acc;
}

// The state the first draw outputs from, and the state after n draws (one step per draw, whichever side of the step the output reads).
constexpr u128 origin(Variant v, u128 state, u128 inc) { return v == kPcg64 ? step(v, state, inc) : state; }
constexpr u128 advance(Variant v, u128 state, u128 inc, u128 n) { return apply(jump(v, n), state, inc); }

// One output segment of a launch: n draws of the generator (variant, state, inc) to draws [offset, offset + n) of the output buffer.
struct Segment { u128 state, inc; uint32_t variant; uint64_t n, offset; };

constexpr SegmentsStatus kSegmentsBadVariant = kSegmentsOwn;

// kSegmentsBadVariant: a variant that is neither kPcg64 nor kDxsm; the rest is flashe_draw::check_segments.
inline SegmentsStatus check_segments(const Segment *segs, int n_segments, int max_segments = kMaxSegments)
{
    return flashe_draw::check_segments(segs, n_segments, max_segments, [](const Segment &s) { return s.variant < kVariants; });
}

// A caller's segment struct (flashe_pcg64_segment's fields: two-word state and inc, low word first) as a Segment.
template <class CSegment> inline void from_c(const CSegment &s, Segment &o)
{
    o.state = make128(s.state[1], s.state[0]); o.inc = make128(s.inc[1], s.inc[0]);
    o.variant = s.variant; o.n = s.n; o.offset = s.offset;
}

// ---- the launch's view ----
// A segment is cut into tiles of kTileDraws = kLanes x kStretch draws; a tile belongs to one segment.  Lane t of the workgroup that holds
// tile k owns the draws  k kTileDraws + t + r kLanes,  r = 0 .. kStretch - 1: it jumps ONCE to the first of them -- over k kTileDraws steps
// with the Pow2 table (entries kTileLog2 and up, one per set bit of k; the same for every lane of the workgroup), then over t steps with
// one row of the Lane table -- and walks the rest at the stride kLanes, whose map is (A^kLanes, inc G_kLanes): the second is per segment
// and rides in the plan row.  A wave's 64 stores of one r are then 512 contiguous bytes.
constexpr uint32_t kLanes = 256, kLanesLog2 = 8, kStretch = 16, kTileDraws = kLanes * kStretch, kTileLog2 = 12;
static_assert(kLanes == 1u << kLanesLog2 && kTileDraws == 1u << kTileLog2, "the tables are indexed by these logarithms");

struct Row { uint64_t mul[2], add[2]; };                                                    // a Jump as four words (low first)
constexpr Jump from_row(const Row &r) { return Jump{make128(r.mul[1], r.mul[0]), make128(r.add[1], r.add[0])}; }
constexpr Row to_row(const Jump &j) { return Row{{lo64(j.mul), hi64(j.mul)}, {lo64(j.add), hi64(j.add)}}; }

struct Pow2Table { Row row[64]; };                  // row[b]: the jump over 2^b steps (a segment holds at most 2^60 draws)
struct LaneTable { Row row[kLanes]; };              // row[t]: the jump over t steps

constexpr Pow2Table make_pow2_table(Variant v)
{
    Pow2Table t{};
    Jump cur{multiplier(v), 1};
    for (int b = 0; b < 64; b++) {
        t.row[b] = to_row(cur);
        cur = compose(cur, cur);
    }
    return t;
}

constexpr LaneTable make_lane_table(Variant v)
{
    LaneTable t{};
    Jump cur{1, 0};
    const Jump one{multiplier(v), 1};
    for (uint32_t l = 0; l < kLanes; l++) {
        t.row[l] = to_row(cur);
        cur = compose(cur, one);
    }
    return t;
}

// The state tile `tile` of a segment starts at (the output state of its draw tile kTileDraws): one table row per set bit of `tile`.
FLASHE_HD u128 tile_origin(const Pow2Table &pow2, u128 origin0, u128 inc, uint64_t tile)
{
    u128 s = origin0;
    for (int b = kTileLog2; tile; b++, tile >>= 1)
        if (tile & 1) s = apply(from_row(pow2.row[b]), s, inc);
    return s;
}

// The plan row of a non-empty segment.
struct Plan { uint64_t origin[2], inc[2], stride_add[2], n, offset, tile_first; uint32_t variant, reserved; };

inline uint64_t segment_tiles(uint64_t n) { return (n + kTileDraws - 1) / kTileDraws; }

// The plans of the non-empty segments of one variant (checked already), in table order; returns their tiles.
inline uint64_t plan_segments(const Segment *segs, int n_segments, Variant v, std::vector<Plan> &plans)
{
    plans.clear();
    uint64_t tiles = 0;
    const u128 g_stride = jump(v, kLanes).add;
    for (int s = 0; s < n_segments; s++) {
        if (!segs[s].n || segs[s].variant != v) continue;
        Plan p{};
        const u128 o = origin(v, segs[s].state, segs[s].inc), sa = mul(g_stride, segs[s].inc);
        p.origin[0] = lo64(o); p.origin[1] = hi64(o);
        p.inc[0] = lo64(segs[s].inc); p.inc[1] = hi64(segs[s].inc);
        p.stride_add[0] = lo64(sa); p.stride_add[1] = hi64(sa);
        p.n = segs[s].n; p.offset = segs[s].offset; p.tile_first = tiles; p.variant = v;
        tiles += segment_tiles(p.n);
        plans.push_back(p);
    }
    return tiles;
}

// ---- the draws of a cohort generated inside the launch that consumes them (codec.hip's quantize_pcg64_combine_cohort_kernel) ----
// Client c rounds its value k with the draw that outputs from  A^k origin_c + G_k inc_c  (the head of this file).  The launch's lane owns
// RUNS of kRunDraws = 4 consecutive values: run g is values 4 g .. 4 g + 3, lane t of workgroup w takes runs  g0 = w kLanes + t,
// g0 + W kLanes, g0 + 2 W kLanes, ...  of a grid of W workgroups.  The jump over 4 g steps depends on neither the client nor its
// generator, so the lane keeps ONE jump for all clients: built once for g0 -- the workgroup's part, over w 4 kLanes steps, from the Pow2
// rows (uniform); the lane's part, over 4 t steps, one row of a RunTable --, and composed with the stride jump over 4 kLanes W steps at the
// end of every pass (the host computes that one for the launch's grid).  A client is then its 32-byte plan: apply the jump to
// (origin_c, inc_c), output, and three steps on.  One launch is one variant: the multiplier is a literal.
constexpr uint32_t kRunDraws = 4, kRunLog2 = 2;
static_assert(kRunDraws == 1u << kRunLog2, "a run's first draw is its number shifted");

// One plan per client: the state its first draw outputs from, and its inc (low word first).
struct ClientPlan { uint64_t origin[2], inc[2]; };

// The plan of the stretch that starts at draw `first` of a segment's state (any first: a stretch starts anywhere in a segment).
inline ClientPlan client_plan(const Segment &s, uint64_t first)
{
    const Variant v = static_cast<Variant>(s.variant);
    const u128 o = apply(jump(v, first), origin(v, s.state, s.inc), s.inc);
    return ClientPlan{{lo64(o), hi64(o)}, {lo64(s.inc), hi64(s.inc)}};
}

constexpr CohortPlansStatus kCohortPlansMixedVariants = kCohortPlansOwn;

// The plans of n_clients clients of n draws each from checked segments: draw_segments.h's cohort_stretches (the contract and the status
// values of flashe_philox::cohort_plans), and kCohortPlansMixedVariants where the non-empty segments are not all of one variant -- the
// lane's jump is shared by the clients, so a launch has one.  *variant: that variant (kPcg64 where nothing is drawn).  No plans unless
// kCohortPlansOk.
inline CohortPlansStatus cohort_plans(const Segment *segs, int n_segments, uint64_t n_clients, uint64_t n, std::vector<ClientPlan> &plans,
                                      Variant *variant = nullptr)
{
    plans.clear();
    uint32_t seen = 0;
    for (int s = 0; s < n_segments; s++)
        if (segs[s].n) seen |= 1u << segs[s].variant;
    if (variant) *variant = seen == 1u << kDxsm ? kDxsm : kPcg64;
    const CohortPlansStatus st =
        cohort_stretches(segs, n_segments, n_clients, n, [&] { return seen == 3 ? kCohortPlansMixedVariants : kCohortPlansOk; },
                         [&](const Segment &s, uint64_t first) { plans.push_back(client_plan(s, first)); });
    if (st != kCohortPlansOk) plans.clear();
    return st;
}

struct RunTable { Row row[kLanes]; };               // row[t]: the jump over kRunDraws t steps

constexpr RunTable make_run_table(Variant v)
{
    RunTable t{};
    Jump cur{1, 0};
    const Jump run = jump(v, kRunDraws);
    for (uint32_t l = 0; l < kLanes; l++) {
        t.row[l] = to_row(cur);
        cur = compose(cur, run);
    }
    return t;
}

// The jump over workgroup kRunDraws kLanes steps -- to the first run of workgroup `workgroup`: one Pow2 row per set bit.
FLASHE_HD Jump workgroup_jump(const Pow2Table &pow2, uint64_t workgroup)
{
    Jump j{1, 0};
    for (int b = kRunLog2 + kLanesLog2; workgroup; b++, workgroup >>= 1)
        if (workgroup & 1) j = compose(j, from_row(pow2.row[b]));
    return j;
}

// The jump of the lane whose RunTable row is `lane_row`, from its workgroup's.
FLASHE_HD Jump lane_jump(const Jump &workgroup, const Row &lane_row) { return compose(workgroup, from_row(lane_row)); }

// The jump from one pass to the next of a grid of `workgroups` workgroups (host: a kernel argument).
inline Jump stride_jump(Variant v, uint64_t workgroups) { return jump(v, static_cast<u128>(kRunDraws * kLanes) * workgroups); }

// One pass on: the lane's jump composed with the stride jump.
FLASHE_HD Jump next_pass(const Jump &lane, const Jump &stride) { return compose(lane, stride); }

// The words of a client's kRunDraws draws of the run the lane's jump leads to: apply, output, and three steps with an output each.
template <Variant V> FLASHE_HD void run_words(const Jump &lane, u128 origin_c, u128 inc_c, uint64_t (&w)[kRunDraws])
{
    u128 s = apply(lane, origin_c, inc_c);
FLASHE_UNROLL
    for (uint32_t i = 0; i < kRunDraws; i++) {
        w[i] = output<V>(s);
        if (i + 1 < kRunDraws) s = step(V, s, inc_c);
    }
}

// Word i < kRunDraws of the same run alone (the launch's value-by-value path: the same draws, indexed).
template <Variant V> FLASHE_HD uint64_t run_word(const Jump &lane, u128 origin_c, u128 inc_c, uint32_t i)
{
    u128 s = apply(lane, origin_c, inc_c);
FLASHE_UNROLL
    for (uint32_t j = 0; j + 1 < kRunDraws; j++)
        if (j < i) s = step(V, s, inc_c);
    return output<V>(s);
}

// The draws the lane that owns run `run` (workgroup run / kLanes, lane run % kLanes) of a grid of `workgroups` generates in its first
// `iterations` passes under a plan, through the functions above and nothing else: out[kRunDraws p + i] = its draw i of pass p.
template <Variant V>
inline void lane_draws(const Pow2Table &pow2, const RunTable &runs, const ClientPlan &p, uint64_t workgroups, uint64_t run, uint64_t iterations, double *out)
{
    const Jump stride = stride_jump(V, workgroups);
    Jump j = lane_jump(workgroup_jump(pow2, run / kLanes), runs.row[run % kLanes]);
    const u128 o = make128(p.origin[1], p.origin[0]), inc = make128(p.inc[1], p.inc[0]);
    for (uint64_t it = 0; it < iterations; it++) {
        uint64_t w[kRunDraws];
        run_words<V>(j, o, inc, w);
        for (uint32_t i = 0; i < kRunDraws; i++) out[kRunDraws * it + i] = to_double(w[i]);
        j = next_pass(j, stride);
    }
}

}  // namespace flashe_pcg64
