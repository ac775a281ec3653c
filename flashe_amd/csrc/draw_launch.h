// The launch of a table of plans, stated once for the draw calls (philox.hip, pcg64.hip).  A launch is cut into tiles that belong to one
// segment; a workgroup walks tiles blockIdx.x, + gridDim.x, ... (stream_grid's rule: at most 8 workgroups per CU) and finds the tile's
// plan with flashe_draw::tile_plan.  The table rides in the kernel-argument block up to kArgPlans plans -- no copy, nothing for the host to
// wait for -- and in ctx->draw_tab beyond that.  A kind brings its Plan (a tile_first member, 80 bytes at most), its tile body and the
// two kernels that call it: one takes the table by value, the other by address.
#pragma once
#include "ctx.h"
#include "device_common.h"
#include "draw_segments.h"

#include <vector>

namespace flashe_draw {

constexpr int kArgPlans = 48;                         // 48 x 80 bytes + the other arguments < the 4-KiB kernel-argument block
constexpr size_t kPlanBytes = 80;                     // the larger plan row: ctx->draw_tab holds kMaxSegments of them

template <class Plan> struct ArgPlans { Plan p[kArgPlans]; };

// (the addresses are integers: said to be global memory, so that the stores are global_store and not flat_store -- FLASHE_GLOBAL)
__device__ __forceinline__ void st_draw(uintptr_t at, double d) { __builtin_nontemporal_store(d, FLASHE_GLOBAL(double, at)); }

// One launch of `tiles` tiles over `plans` (no tiles: nothing).  A table too long for the kernel arguments goes to rows tab_first and up
// of ctx->draw_tab.  (Pageable source: the copy has left `plans` when the call returns.  Every draw call of a ctx, whatever its kind,
// copies and launches on the ctx stream, so stream order keeps an earlier launch's table intact until that launch has ended.)
template <class Plan>
int launch_plans(flashe_ctx *ctx, const std::vector<Plan> &plans, uint64_t tiles, size_t tab_first,
                 void (*args_kernel)(const ArgPlans<Plan>, int, uint64_t, double *), void (*table_kernel)(const Plan *, int, uint64_t, double *),
                 double *u_dev)
{
    static_assert(sizeof(Plan) <= kPlanBytes, "ctx->draw_tab is sized by kPlanBytes");
    if (!tiles) return FLASHE_OK;
    const int n_plans = static_cast<int>(plans.size());
    const dim3 grid(flashe::stream_grid(ctx->env, tiles * flashe::kStreamThreads)), wg(flashe::kStreamThreads);
    if (n_plans <= kArgPlans) {
        ArgPlans<Plan> tab{};
        std::copy(plans.begin(), plans.end(), tab.p);
        hipLaunchKernelGGL(args_kernel, grid, wg, 0, ctx->env.stream, tab, n_plans, tiles, u_dev);
    } else {
        if (int rc = flashe_host::ensure(ctx, ctx->draw_tab, kMaxSegments * kPlanBytes)) return rc;
        Plan *tab = static_cast<Plan *>(ctx->draw_tab.p) + tab_first;
        HIP_TRY(ctx, hipMemcpyAsync(tab, plans.data(), plans.size() * sizeof(Plan), hipMemcpyHostToDevice, ctx->env.stream));
        hipLaunchKernelGGL(table_kernel, grid, wg, 0, ctx->env.stream, static_cast<const Plan *>(tab), n_plans, tiles, u_dev);
    }
    HIP_TRY(ctx, hipGetLastError());
    return FLASHE_OK;
}

// The front of the entry point `name`: the caller's table as the kind's segments, refused (FLASHE_EINVAL, the message set) for its count, a null table,
// a graph being captured, what the kind's check_segments finds (`own`: its words for kSegmentsOwn) and, when there is anything to draw, for u_dev
// (with_out = false: a call that writes no draw buffer).
template <class CSegment, class Segment>
int read_segments(flashe_ctx *ctx, const char *name, const CSegment *segments, int n_segments, const double *u_dev, void (*to_segment)(const CSegment &, Segment &),
                  SegmentsStatus (*check_segments)(const Segment *, int, int), const char *own, std::vector<Segment> &segs, bool with_out = true)
{
    using flashe_host::fail;
    if (n_segments < 0 || n_segments > kMaxSegments) return fail(ctx, FLASHE_EINVAL, "%s: %d segments, a launch holds 0 .. %d", name, n_segments, kMaxSegments);
    if (n_segments && !segments) return fail(ctx, FLASHE_EINVAL, "%s: no segment table", name);
    if (ctx->capturing) return fail(ctx, FLASHE_EINVAL, "%s advances the generator states it is given: a replay would repeat the draws", name);
    segs.resize(static_cast<size_t>(n_segments));
    bool any = false;
    for (int s = 0; s < n_segments; s++) {
        to_segment(segments[s], segs[s]);
        any = any || segs[s].n;
    }
    switch (check_segments(segs.data(), n_segments, kMaxSegments)) {
    case kSegmentsOk: break;
    case kSegmentsOwn: return fail(ctx, FLASHE_EINVAL, "%s: %s", name, own);
    case kSegmentsOverflow: return fail(ctx, FLASHE_EINVAL, "%s: a segment's offset + n overflows", name);
    case kSegmentsOverlap: return fail(ctx, FLASHE_EINVAL, "%s: two segments' output ranges overlap", name);
    default: return fail(ctx, FLASHE_EINVAL, "%s: bad segment table", name);
    }
    if (with_out && any && (!u_dev || (reinterpret_cast<uintptr_t>(u_dev) & 7u))) return fail(ctx, FLASHE_EINVAL, "%s: u_dev must be an 8-byte aligned device pointer", name);
    return FLASHE_OK;
}

}  // namespace flashe_draw
