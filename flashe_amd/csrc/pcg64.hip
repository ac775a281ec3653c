// Generator(PCG64).random(n) and Generator(PCG64DXSM).random(n) on the device, bit for bit: the stochastic-rounding draws of a caller's own
// np.random.Generator (rng=) when it is the one np.random.default_rng returns.
//
// Both are a 128-bit LCG with a 64-bit output function (pcg64_stream.h).  An LCG is sequential, but k steps of it are one affine map
// (A^k, G_k) that does not depend on the generator: a lane jumps ONCE to its first draw and then walks a fixed stride, one 128 x 128 -> 128
// low product and one output function per draw.  A launch is cut into tiles of 4,096 draws that belong to one segment; a workgroup walks
// tiles blockIdx.x, + gridDim.x, ... (stream_grid's rule: at most 8 workgroups per CU), finds the tile's segment by a search of the plan
// table and the tile's first state from the table of the jumps over 2^b steps -- both uniform over the workgroup: scalar work.  Lane t then
// jumps t draws on with one row of a 256-row table and walks 16 draws at a stride of 256, so that a wave's 64 stores are 512 contiguous
// bytes; they are 8-byte non-temporal stores, which is all the alignment an output range has (a cohort's client stretch starts at any
// draw).  Nothing outside [offset, offset + n) is written.  The variant is a template parameter: a table that holds both is two launches.
// The states are advanced on the host (one jump per segment), so nothing is read back and the call does not synchronise.
//
// Here: the tile body, the two kernels that call it, and the entry points.  pcg64_stream.h: the streams' arithmetic, the jump tables, the
// segment checks and the plans (no HIP: run on the host under sanitizers).  draw_segments.h, draw_launch.h: what the launch of a plan table
// shares with philox.hip -- the range checks and the tile search; where the table rides, the launch and the entry points' common checks.
#include "draw_launch.h"
#include "pcg64_stream.h"

namespace {

using flashe_draw::st_draw;
using flashe_pcg64::Plan;
using flashe_pcg64::u128;
using flashe_pcg64::Variant;
using ArgPlans = flashe_draw::ArgPlans<Plan>;
static_assert(sizeof(Plan) == 80, "the plan rows are 80 bytes");
static_assert(flashe_pcg64::kLanes == flashe::kStreamThreads, "a tile is kStretch draws per thread of a stream workgroup");

// the jump tables of the two variants (pcg64_stream.h), built by the compiler
alignas(32) __device__ const flashe_pcg64::Pow2Table kPow2[flashe_pcg64::kVariants] = {flashe_pcg64::make_pow2_table(flashe_pcg64::kPcg64),
                                                                          flashe_pcg64::make_pow2_table(flashe_pcg64::kDxsm)};
alignas(32) __device__ const flashe_pcg64::LaneTable kLane[flashe_pcg64::kVariants] = {flashe_pcg64::make_lane_table(flashe_pcg64::kPcg64),
                                                                          flashe_pcg64::make_lane_table(flashe_pcg64::kDxsm)};

template <Variant V>
__device__ __forceinline__ void pcg64_tiles(const Plan *__restrict__ plans, int n_plans, uint64_t tiles, double *__restrict__ out)
{
    using namespace flashe_pcg64;
    constexpr Jump kStride = from_row(make_pow2_table(V).row[kLanesLog2]);               // (A^256, G_256): the multiplier is a literal
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const Plan &p = flashe_draw::tile_plan(plans, n_plans, t);
        const uint64_t k = t - p.tile_first, i0 = k * kTileDraws + threadIdx.x, n = p.n;     // the lane's first draw of the segment
        if (i0 >= n) continue;
        const u128 inc = make128(p.inc[1], p.inc[0]), stride_add = make128(p.stride_add[1], p.stride_add[0]);
        const u128 first = tile_origin(kPow2[V], make128(p.origin[1], p.origin[0]), inc, k);  // uniform over the workgroup
        const uint64_t *row = kLane[V].row[threadIdx.x].mul;
        const u128 lm = flashe::ld128_g(row), la = flashe::ld128_g(row + 2);
        u128 s = mul(lm, first) + mul(la, inc);
        uintptr_t o = reinterpret_cast<uintptr_t>(out) + 8 * (p.offset + i0);
        if (i0 + (kStretch - 1) * kLanes < n) {
#pragma unroll
            for (uint32_t r = 0; r < kStretch; r++) {
                st_draw(o, to_double(output<V>(s)));
                s = mul(s, kStride.mul) + stride_add;
                o += 8 * kLanes;
            }
        } else {
            for (uint64_t i = i0; i < n; i += kLanes) {
                st_draw(o, to_double(output<V>(s)));
                s = mul(s, kStride.mul) + stride_add;
                o += 8 * kLanes;
            }
        }
    }
}

template <Variant V>
__global__ __launch_bounds__(flashe::kStreamThreads) void pcg64_random_args_kernel(const ArgPlans tab, int n_plans, uint64_t tiles, double *__restrict__ out)
{
    pcg64_tiles<V>(tab.p, n_plans, tiles, out);
}

template <Variant V>
__global__ __launch_bounds__(flashe::kStreamThreads) void pcg64_random_table_kernel(const Plan *__restrict__ plans, int n_plans, uint64_t tiles,
                                                                                    double *__restrict__ out)
{
    pcg64_tiles<V>(plans, n_plans, tiles, out);
}

u128 from_words(const uint64_t w[2]) { return flashe_pcg64::make128(w[1], w[0]); }

// One variant's segments of the table: a launch of their tiles (none: nothing).  Rows [0, *tab_rows) of the ctx table are in use by the
// launch of the other variant; the rows this one takes are added.
template <Variant V>
int launch_variant(flashe_ctx *ctx, const std::vector<flashe_pcg64::Segment> &segs, size_t *tab_rows, double *u_dev)
{
    std::vector<Plan> plans;
    const uint64_t tiles = flashe_pcg64::plan_segments(segs.data(), static_cast<int>(segs.size()), V, plans);
    const size_t first = *tab_rows;
    if (plans.size() > static_cast<size_t>(flashe_draw::kArgPlans)) *tab_rows += plans.size();
    return flashe_draw::launch_plans(ctx, plans, tiles, first, pcg64_random_args_kernel<V>, pcg64_random_table_kernel<V>, u_dev);
}

}  // namespace

extern "C" int flashe_pcg64_advance(uint32_t variant, uint64_t state[2], const uint64_t inc[2], const uint64_t n[2])
{
    if (!state || !inc || !n || variant >= flashe_pcg64::kVariants) return FLASHE_EINVAL;
    const u128 s = flashe_pcg64::advance(static_cast<Variant>(variant), from_words(state), from_words(inc), from_words(n));
    state[0] = flashe_pcg64::lo64(s); state[1] = flashe_pcg64::hi64(s);
    return FLASHE_OK;
}

extern "C" int flashe_pcg64_grid(flashe_ctx *ctx, uint64_t n, uint32_t *workgroups, uint64_t *tiles, uint32_t *tile_draws)
{
    if (!ctx || !workgroups || !tiles || n > flashe_pcg64::kMaxDraws) return FLASHE_EINVAL;
    *tiles = flashe_pcg64::segment_tiles(n);
    *workgroups = static_cast<uint32_t>(flashe::stream_grid(ctx->env, *tiles * flashe::kStreamThreads));
    if (tile_draws) *tile_draws = flashe_pcg64::kTileDraws;
    return FLASHE_OK;
}

extern "C" int flashe_pcg64_random_dev(flashe_ctx *ctx, flashe_pcg64_segment *segments, int n_segments, double *u_dev)
{
    CHECK_CTX(ctx);
    std::vector<flashe_pcg64::Segment> segs;
    if (int rc = flashe_draw::read_segments(ctx, "flashe_pcg64_random_dev", segments, n_segments, u_dev, flashe_pcg64::from_c<flashe_pcg64_segment>, flashe_pcg64::check_segments,
                                            "a variant that is neither PCG64 (0) nor PCG64DXSM (1)", segs))
        return rc;
    size_t tab_rows = 0;
    if (int rc = launch_variant<flashe_pcg64::kPcg64>(ctx, segs, &tab_rows, u_dev)) return rc;
    if (int rc = launch_variant<flashe_pcg64::kDxsm>(ctx, segs, &tab_rows, u_dev)) return rc;
    for (int s = 0; s < n_segments; s++) {
        const u128 a = flashe_pcg64::advance(static_cast<Variant>(segs[s].variant), segs[s].state, segs[s].inc, segs[s].n);
        segments[s].state[0] = flashe_pcg64::lo64(a); segments[s].state[1] = flashe_pcg64::hi64(a);
    }
    return FLASHE_OK;
}
