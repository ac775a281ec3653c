// Host check of flashe_amd/csrc/pcg64_stream.h (the streams of NumPy's PCG64 and PCG64DXSM generators as the device launch and the host
// state hand-back read them), built with -fsanitize=address,undefined by tests/test_pcg64_stream_sanitized.py.  For both variants: jump(k),
// the advanced state and the launch's route to a draw (tile jump by the Pow2 table, lane jump by the Lane table, the stride walk with the
// plan row's constants) against a generator written here on its own that walks the stream ONE draw at a time the way NumPy does;
// jump(a + b) = jump(b) o jump(a) at distances up to 2^127; states and increments of 0 and 2^128 - 1 and an even inc; the checks of a
// segment table.  The known first outputs of the two generators pin the constants themselves.
#include "pcg64_stream.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace flashe_pcg64;

#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

// NumPy's pcg64_next64 (pcg_setseq_128_xsl_rr_64_random_r) and pcg64_cm_next64 (pcg_cm_random_r), step by step, in 64-bit pieces of its own
struct Walker {
    Variant v;
    uint64_t hi, lo, inc_hi, inc_lo;
    void step_once()
    {
        const uint64_t a_hi = v == kPcg64 ? 0x2360ED051FC65DA4ull : 0, a_lo = v == kPcg64 ? 0x4385DF649FCCF645ull : 0xDA942042E4DD58B5ull;
        const unsigned __int128 p = static_cast<unsigned __int128>(lo) * a_lo;
        uint64_t nhi = static_cast<uint64_t>(p >> 64) + lo * a_hi + hi * a_lo, nlo = static_cast<uint64_t>(p);
        const uint64_t slo = nlo + inc_lo;
        nhi += inc_hi + (slo < nlo ? 1 : 0);
        hi = nhi; lo = slo;
    }
    uint64_t next()
    {
        if (v == kPcg64) {
            step_once();
            const uint64_t x = hi ^ lo;
            const unsigned rot = static_cast<unsigned>(hi >> 58);
            return rot ? (x >> rot) | (x << (64 - rot)) : x;
        }
        uint64_t h = hi;
        const uint64_t l = lo | 1;
        h ^= h >> 32;
        h *= 0xDA942042E4DD58B5ull;
        h ^= h >> 48;
        h *= l;
        step_once();
        return h;
    }
    u128 state() const { return make128(hi, lo); }
};

static long g_draws = 0;
static const u128 kOnes = ~static_cast<u128>(0);

static Walker walker(Variant v, u128 state, u128 inc) { return Walker{v, hi64(state), lo64(state), hi64(inc), lo64(inc)}; }

// draw i of a segment by the launch's route
static uint64_t launch_draw(Variant v, const Plan &p, const Pow2Table &pow2, const LaneTable &lane, uint64_t i)
{
    const uint64_t k = i / kTileDraws, t = i % kLanes, r = (i % kTileDraws) / kLanes;
    const u128 inc = make128(p.inc[1], p.inc[0]);
    u128 s = apply(from_row(lane.row[t]), tile_origin(pow2, make128(p.origin[1], p.origin[0]), inc, k), inc);
    const Jump stride = from_row(pow2.row[kLanesLog2]);
    for (uint64_t q = 0; q < r; q++) s = mul(s, stride.mul) + make128(p.stride_add[1], p.stride_add[0]);
    return v == kPcg64 ? output<kPcg64>(s) : output<kDxsm>(s);
}

static void check_stream(Variant v, u128 state, u128 inc, const Pow2Table &pow2, const LaneTable &lane)
{
    // jump(k), advance and the origin of draw k against the walk, k = 0 .. 600 (past a lane table and two strides)
    Walker w = walker(v, state, inc);
    for (uint64_t k = 0; k <= 600; k++) {
        const Jump j = jump(v, k);
        CHECK(apply(j, state, inc) == w.state() && advance(v, state, inc, k) == w.state());
        Walker peek = w;
        const uint64_t word = peek.next();
        const u128 at = apply(j, origin(v, state, inc), inc);
        CHECK((v == kPcg64 ? output<kPcg64>(at) : output<kDxsm>(at)) == word);
        CHECK(to_double(word) == static_cast<double>(word >> 11) / 9007199254740992.0 && to_double(word) < 1.0);
        w.next();
        g_draws++;
    }
    // the launch's route: every draw of a segment of two tiles and a ragged third
    const uint64_t n = 2 * kTileDraws + 1031;
    Segment seg{state, inc, static_cast<uint32_t>(v), n, 9};
    std::vector<Plan> plans;
    CHECK(plan_segments(&seg, 1, v, plans) == 3 && plans.size() == 1 && plans[0].n == n && plans[0].offset == 9 && plans[0].tile_first == 0);
    CHECK(plans[0].variant == static_cast<uint32_t>(v));
    Walker x = walker(v, state, inc);
    for (uint64_t i = 0; i < n; i++) {
        CHECK(launch_draw(v, plans[0], pow2, lane, i) == x.next());
        g_draws++;
    }
    CHECK(advance(v, state, inc, n) == x.state());
}

static void check_tables(Variant v, const Pow2Table &pow2, const LaneTable &lane)
{
    for (int b = 0; b < 64; b++) {
        const Jump j = jump(v, static_cast<u128>(1) << b), t = from_row(pow2.row[b]);
        CHECK(j.mul == t.mul && j.add == t.add);
    }
    for (uint32_t l = 0; l < kLanes; l++) {
        const Jump j = jump(v, l), t = from_row(lane.row[l]);
        CHECK(j.mul == t.mul && j.add == t.add);
    }
    // a far tile: the table route against jump
    const u128 s0 = make128(0x0123456789abcdefull, 0xfedcba9876543210ull), inc = make128(5, 7);
    for (uint64_t tile : {1ull, 2ull, 3ull, 0x5a5a5ull, (1ull << 48) - 1, 1ull << 47})
        CHECK(tile_origin(pow2, s0, inc, tile) == apply(jump(v, static_cast<u128>(tile) << kTileLog2), s0, inc));
    CHECK(tile_origin(pow2, s0, inc, 0) == s0);
}

static void check_jump_composition(Variant v)
{
    const u128 one = 1;
    const u128 dist[] = {0, 1, 2, 255, 256, (one << 32) - 1, (one << 32) + 1, (one << 64) - 1, one << 64, (one << 64) + 1, (one << 100) + 12345,
                         (one << 127) - 1, one << 127};
    const u128 states[] = {0, kOnes, make128(0x0123456789abcdefull, 0xfedcba9876543210ull)};
    const u128 incs[] = {0, kOnes, 2, make128(1, 0), make128(0xdeadbeefull, 0x12345679ull)};      // 2 and 2^64: even increments
    const Jump id = jump(v, 0);
    CHECK(id.mul == 1 && id.add == 0);
    for (u128 a : dist)
        for (u128 b : dist) {
            const Jump ja = jump(v, a), jb = jump(v, b), jab = jump(v, a + b), c = compose(ja, jb);      // (a + b wraps at 2^128: so does the LCG's period)
            CHECK(c.mul == jab.mul && c.add == jab.add);
            for (u128 s : states)
                for (u128 inc : incs) CHECK(apply(jb, apply(ja, s, inc), inc) == apply(jab, s, inc) && advance(v, advance(v, s, inc, a), inc, b) == advance(v, s, inc, a + b));
        }
    // one step is the step
    const Jump j1 = jump(v, 1);
    CHECK(j1.mul == multiplier(v) && j1.add == 1);
    for (u128 s : states)
        for (u128 inc : incs) CHECK(apply(j1, s, inc) == step(v, s, inc));
    // the full period of a generator with an odd increment brings it back
    const Jump half = jump(v, one << 127), full = compose(half, half);
    CHECK(full.mul == 1 && full.add == 0);
}

static Segment seg(uint32_t variant, uint64_t n, uint64_t offset) { return Segment{make128(1, 2), make128(3, 5), variant, n, offset}; }

static void check_segments_table()
{
    std::vector<Segment> t = {seg(0, 5, 0), seg(1, 4099, 5), seg(0, 1, 4104)};
    CHECK(check_segments(t.data(), 3) == kSegmentsOk);
    CHECK(check_segments(nullptr, 0) == kSegmentsOk);
    CHECK(check_segments(nullptr, 1) == kSegmentsBadCount && check_segments(t.data(), -1) == kSegmentsBadCount);
    // back to back is fine in any order; one shared draw is not; an empty segment overlaps nothing
    std::vector<Segment> r = {seg(0, 3, 10), seg(1, 10, 0), seg(0, 0, 5)};
    CHECK(check_segments(r.data(), 3) == kSegmentsOk);
    r[1].n = 11;
    CHECK(check_segments(r.data(), 3) == kSegmentsOverlap);
    r[1].n = 10; r[0].offset = 9;
    CHECK(check_segments(r.data(), 3) == kSegmentsOverlap);
    std::vector<Segment> same = {seg(0, 1, 2), seg(1, 1, 2)};
    CHECK(check_segments(same.data(), 2) == kSegmentsOverlap);
    // the two variants
    for (uint32_t v = 0; v <= 3; v++) {
        Segment s = seg(v, 1, 0);
        CHECK(check_segments(&s, 1) == (v <= 1 ? kSegmentsOk : kSegmentsBadVariant));
    }
    // counts and offsets whose byte counts would leave 64 bits
    Segment big = seg(0, kMaxDraws, 0);
    CHECK(check_segments(&big, 1) == kSegmentsOk);
    big.offset = 1;
    CHECK(check_segments(&big, 1) == kSegmentsOverflow);
    big = seg(1, kMaxDraws + 1, 0);
    CHECK(check_segments(&big, 1) == kSegmentsOverflow);
    big = seg(0, 1, ~0ull);
    CHECK(check_segments(&big, 1) == kSegmentsOverflow);
    big = seg(0, ~0ull, 2);                                     // offset + n wraps to 1
    CHECK(check_segments(&big, 1) == kSegmentsOverflow);
    // the segments a launch holds
    std::vector<Segment> many;
    for (int s = 0; s < kMaxSegments + 1; s++) many.push_back(seg(s & 1, 3, 3 * static_cast<uint64_t>(s)));
    CHECK(check_segments(many.data(), kMaxSegments) == kSegmentsOk);
    CHECK(check_segments(many.data(), kMaxSegments + 1) == kSegmentsBadCount);
    CHECK(check_segments(many.data(), 3, 2) == kSegmentsBadCount);
    // the plans: a variant's non-empty segments in table order, whole tiles of their own
    std::vector<Segment> mix = {seg(0, 5, 0), seg(0, 0, 5), seg(1, 4099, 5), seg(0, 4096, 4104), seg(1, 1, 8200), seg(0, 4097, 8201)};
    std::vector<Plan> plans;
    CHECK(plan_segments(mix.data(), 6, kPcg64, plans) == 1 + 1 + 2 && plans.size() == 3);
    CHECK(plans[0].tile_first == 0 && plans[1].tile_first == 1 && plans[2].tile_first == 2 && plans[2].offset == 8201);
    CHECK(plan_segments(mix.data(), 6, kDxsm, plans) == 2 + 1 && plans.size() == 2 && plans[1].tile_first == 2 && plans[1].n == 1);
    CHECK(segment_tiles(0) == 0 && segment_tiles(1) == 1 && segment_tiles(kTileDraws) == 1 && segment_tiles(kTileDraws + 1) == 2);
    CHECK(segment_tiles(kMaxDraws) == kMaxDraws / kTileDraws);
}

int main()
{
    // the constants: the first words of PCG64 and PCG64DXSM from the states NumPy's SeedSequence gives seed 1 (values of NumPy 2.2.6)
    {
        const u128 s = make128(0x9c5b484bfedb756cull, 0x2a6e7d6f320fbc7eull), inc = make128(0x922af2da2645f895ull, 0xa19857b95740937bull);
        const uint64_t want[2][3] = {{0x8306bdf37922e4ffull, 0xf35196bbc152a866ull, 0x24e7a4f608ec18cdull},
                                     {0x4569de53b956589full, 0x47838278a68528bfull, 0x8a62dbc712b1acedull}};
        for (Variant v : {kPcg64, kDxsm}) {
            Walker w = walker(v, s, inc);
            u128 at = origin(v, s, inc);
            for (int i = 0; i < 3; i++) {
                CHECK(w.next() == want[v][i]);
                CHECK((v == kPcg64 ? output<kPcg64>(at) : output<kDxsm>(at)) == want[v][i]);
                at = step(v, at, inc);
            }
        }
    }
    static const Pow2Table pow2[2] = {make_pow2_table(kPcg64), make_pow2_table(kDxsm)};
    static const LaneTable lane[2] = {make_lane_table(kPcg64), make_lane_table(kDxsm)};
    const u128 states[] = {0, kOnes, make128(0x0123456789abcdefull, 0xfedcba9876543210ull)};
    const u128 incs[] = {0, kOnes, 2, make128(0xdeadbeefull, 0x12345679ull)};
    for (Variant v : {kPcg64, kDxsm}) {
        check_tables(v, pow2[v], lane[v]);
        check_jump_composition(v);
        for (u128 s : states)
            for (u128 inc : incs) check_stream(v, s, inc, pow2[v], lane[v]);
    }
    check_segments_table();
    printf("PCG64_STREAM_OK %ld draws\n", g_draws);
    return 0;
}
