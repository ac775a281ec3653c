// Generator(Philox).random(n) on the device, bit for bit: the stochastic-rounding draws of a caller's own np.random.Generator (rng=).
//
// NumPy's global generator can only be MT19937, a sequential recurrence that mt19937.hip parallelises with jump-ahead trees and one twist
// wave per substream, behind a synchronous call.  Philox4x64-10 (np.random.Philox) is counter based: every block of four draws is a pure
// function of (key, counter), so there is no jump and no chain -- a lane owns whole blocks (four draws = 32 bytes), any number of streams
// (the clients of a cohort) run in ONE launch, and the state after n draws is a few host additions (philox_stream.h), so nothing is read
// back and the call does not synchronise.  The work per block is 20 64 x 64 -> 128 products, built from 32-bit multiply-adds.
//
// A launch is cut into tiles of 256 blocks that belong to one segment; the search of the plan table that finds a tile's segment is uniform
// over the workgroup.  Output ranges are only 8-byte aligned (a cohort's client stretch starts at any draw): a whole block is written as
// two 16-byte non-temporal stores where its address allows, as 8 + 16 + 8 where it does not, and the ragged first and last block of a
// segment word by word; nothing outside [offset, offset + n) is written.
//
// Here: the tile body, the two kernels that call it, and the entry points.  philox_stream.h: the stream's arithmetic, the segment checks and
// the plans (no HIP: run on the host under sanitizers).  draw_segments.h, draw_launch.h: what the launch of a plan table shares with
// pcg64.hip -- the range checks and the tile search; where the table rides, the launch and the entry points' common checks.
#include "draw_launch.h"
#include "philox_stream.h"

namespace {

using flashe_draw::st_draw;
using flashe_philox::Plan;
using ArgPlans = flashe_draw::ArgPlans<Plan>;
static_assert(sizeof(Plan) == 80, "the plan rows are 80 bytes");
static_assert(flashe_philox::kTileBlocks == flashe::kStreamThreads, "a tile is one block per thread of a stream workgroup");

typedef double f64x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void st_draws2(uintptr_t at, double a, double b)
{
    f64x2 v;
    v[0] = a; v[1] = b;
    __builtin_nontemporal_store(v, FLASHE_GLOBAL(f64x2, at));
}

__device__ __forceinline__ void philox_tiles(const Plan *__restrict__ plans, int n_plans, uint64_t tiles, double *__restrict__ out)
{
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const Plan &p = flashe_draw::tile_plan(plans, n_plans, t);
        const uint64_t j = (t - p.tile_first) * flashe_philox::kTileBlocks + threadIdx.x;
        const uint64_t v0 = 4 * j, skip = p.skip, end = skip + p.n;       // the block's virtual draws v0 .. v0 + 3; [skip, end) exist
        if (v0 >= end) continue;
        uint64_t base[4] = {p.base[0], p.base[1], p.base[2], p.base[3]}, key[2] = {p.key[0], p.key[1]}, at[4], w[4];
        flashe_philox::counter_add(base, j, at);
        flashe_philox::block(at, key, w);
        const double d0 = flashe_philox::to_double(w[0]), d1 = flashe_philox::to_double(w[1]), d2 = flashe_philox::to_double(w[2]),
                     d3 = flashe_philox::to_double(w[3]);
        // virtual draw v lies at out[offset + v - skip] (mod 2^64 for the draws of a first block that do not exist: never formed into a store)
        const uintptr_t o = reinterpret_cast<uintptr_t>(out) + 8 * (p.offset + v0 - skip);
        if (v0 >= skip && v0 + 4 <= end) {
            if ((o & 15) == 0) {
                st_draws2(o, d0, d1);
                st_draws2(o + 16, d2, d3);
            } else {
                st_draw(o, d0);
                st_draws2(o + 8, d1, d2);
                st_draw(o + 24, d3);
            }
        } else {
            if (v0 >= skip && v0 < end) st_draw(o, d0);
            if (v0 + 1 >= skip && v0 + 1 < end) st_draw(o + 8, d1);
            if (v0 + 2 >= skip && v0 + 2 < end) st_draw(o + 16, d2);
            if (v0 + 3 >= skip && v0 + 3 < end) st_draw(o + 24, d3);
        }
    }
}

__global__ __launch_bounds__(flashe::kStreamThreads) void philox_random_args_kernel(const ArgPlans tab, int n_plans, uint64_t tiles, double *__restrict__ out)
{
    philox_tiles(tab.p, n_plans, tiles, out);
}

__global__ __launch_bounds__(flashe::kStreamThreads) void philox_random_table_kernel(const Plan *__restrict__ plans, int n_plans, uint64_t tiles,
                                                                                     double *__restrict__ out)
{
    philox_tiles(plans, n_plans, tiles, out);
}

}  // namespace

extern "C" int flashe_philox_block(const uint64_t counter[4], const uint64_t key[2], uint64_t words[4])
{
    if (!counter || !key || !words) return FLASHE_EINVAL;
    flashe_philox::block(counter, key, words);
    return FLASHE_OK;
}

extern "C" int flashe_philox_advance(const uint64_t key[2], uint64_t counter[4], uint32_t *buffer_pos, uint64_t buffer[4], uint64_t n)
{
    if (!key || !counter || !buffer_pos || !buffer || *buffer_pos > 4u || n > flashe_philox::kMaxDraws) return FLASHE_EINVAL;
    flashe_philox::advance(key, counter, *buffer_pos, buffer, n);
    return FLASHE_OK;
}

extern "C" int flashe_philox_grid(flashe_ctx *ctx, uint64_t n, uint32_t buffer_pos, uint32_t *workgroups, uint64_t *tiles)
{
    if (!ctx || !workgroups || !tiles || buffer_pos > 4u || n > flashe_philox::kMaxDraws) return FLASHE_EINVAL;
    const uint64_t blocks = flashe_philox::segment_blocks(buffer_pos < 4 ? buffer_pos : 0, n);
    *tiles = (blocks + flashe_philox::kTileBlocks - 1) / flashe_philox::kTileBlocks;
    *workgroups = static_cast<uint32_t>(flashe::stream_grid(ctx->env, *tiles * flashe::kStreamThreads));
    return FLASHE_OK;
}

extern "C" int flashe_philox_random_dev(flashe_ctx *ctx, flashe_philox_segment *segments, int n_segments, double *u_dev)
{
    CHECK_CTX(ctx);
    std::vector<flashe_philox::Segment> segs;
    if (int rc = flashe_draw::read_segments(ctx, "flashe_philox_random_dev", segments, n_segments, u_dev, flashe_philox::from_c<flashe_philox_segment>, flashe_philox::check_segments, "a buffer_pos above 4", segs))
        return rc;
    std::vector<Plan> plans;
    const uint64_t tiles = flashe_philox::plan_segments(segs.data(), n_segments, plans);
    if (int rc = flashe_draw::launch_plans(ctx, plans, tiles, 0, philox_random_args_kernel, philox_random_table_kernel, u_dev)) return rc;
    for (int s = 0; s < n_segments; s++)
        flashe_philox::advance(segments[s].key, segments[s].counter, segments[s].buffer_pos, segments[s].buffer, segments[s].n);
    return FLASHE_OK;
}
