// A PRECOMPUTE job's online client step straight to and from the packed WIRE form (JZFTransferableWeights.compress / decompress,
// jzf_weights.py:155-231: element j of n at bits [b (n - 1 - j), b (n - j)) of one integer): the masks are the ones prepare_encrypt /
// prepare_decrypt left in the ctx (jzf_flashe.py:599-666), so nothing here runs AES and nothing ties the tiling to AES blocks.
//   combine_small_pack_kernel       float model + draws + cached masks -> quantise -> (q + add - minus) mod 2^b -> packed limbs   (16 .. 64)
//   combine_small_unpack_kernel     packed limbs of the sum + cached masks -> unquantise -> float64 model                         (16 .. 64)
//   combine_wide_pack_kernel<BS>    the batched job's: quantise + batch + masks -> packed limbs                                   (65 .. 128)
//   combine_wide_unpack_kernel<BS>  packed limbs of the sum + masks -> unbatch -> unquantise -> float64 model                     (65 .. 128)
// The tiles are anchored at the END of the vector, as wire_wide.hip states it: with k = n - 1 - j, any 64 consecutive k are exactly b whole
// limbs for EVERY b.  At 16 .. 64 a wave's tile is the kPrepTile = 64 T elements k in [64 T t, 64 T (t + 1)) = the limbs [b T t, b T (t + 1)).
// No limb is shared between tiles: every limb is written once, by one wave, with a plain coalesced 8-byte store -- no fill launch in front,
// no atomic, no T-tables in LDS, and the output need not be zero on entry.  The only partial tile is the top one (the first n mod 64 T
// elements): its wave writes ceil(cnt b / 64) limbs, the unused top bits zero.
//   pack: lane L takes the T elements e_lo + 64 i + L of the tile -- every stream (4 or 8 bytes of the model, 8 of the draws, 8 per mask)
//   is lane-contiguous, all T of each requested before the arithmetic.  A tile inside one table row quantises with the row's parameters
//   from SGPRs (cohort_quantize_raw), a tile that straddles rows with codec_quantize per lane.  The b-bit ciphertexts go to the wave's LDS
//   rows, 8 bytes each, row = the element's k inside the tile (ascending row = ascending bit position; the rows past a partial tile's
//   elements are zero); limb i of the tile then gathers the fields that overlap it -- at most five -- and ORs them shifted.
//   unpack: the tile's limbs are loaded lane-contiguously into the same rows; a lane extracts each of its T fields with two 8-byte LDS
//   reads, adds the masks, unquantises (the row's parameters from SGPRs, or codec_unquantize per lane) and stores float64 coalesced.
// At 65 .. 128 the kernels are prf_wide_pack_kernel / prf_wide_unpack_kernel (wire_wide.hip) with two 16-byte mask loads per lane in place
// of the two AES blocks: tile, batched front end, stitch and walk back come from wire_tiles.h.
#include "wire_tiles.h"

namespace flashe {

namespace {

constexpr int kPrepT = 4;                          // 64-element groups per tile (tests/test_gpu_wire_prepared.py states the same T)
constexpr int kPrepTile = 64 * kPrepT;             // elements per tile = LDS rows per wave
constexpr int kPrepThreads = 1024;

struct PrepWire {
    Codec cq;                                      // pack: the front-end table and the draws; unpack: the back-end table and fout (k0 = 0)
    const uint64_t *add, *minus;                   // the cached masks, one limb per element; minus null: the single-mask cache
    uint64_t n, mask;
    uint32_t b, b_magic;                           // b_magic = ceil(2^32 / b): x / b == (x * b_magic) >> 32 for x < 2^14
};

// tile t: the elements [e_lo, e_lo + cnt), all wave-uniform
struct PrepTile { uint64_t e_lo; uint32_t cnt; int row; };
__device__ __forceinline__ PrepTile prep_tile(const PrepWire &p, uint64_t t)
{
    PrepTile w;
    const uint64_t left = p.n - static_cast<uint64_t>(kPrepTile) * t;
    w.cnt = left < static_cast<uint64_t>(kPrepTile) ? static_cast<uint32_t>(left) : static_cast<uint32_t>(kPrepTile);
    w.e_lo = left - w.cnt;
    w.row = wire_tile_row(p.cq, w.e_lo, w.e_lo + w.cnt, p.n);
    return w;
}

}  // namespace

// packed: ceil(n b / 64) limbs, every one written here (none needs to be zero on entry)
__global__ __launch_bounds__(kPrepThreads) void combine_small_pack_kernel(const PrepWire p, uint64_t *__restrict__ packed)
{
    __shared__ uint64_t rows[(kPrepThreads / 64) * kPrepTile];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
    uint64_t *row0 = rows + wave * kPrepTile;
    const uint32_t b = p.b;
    const uint64_t n_tiles = (p.n + kPrepTile - 1) / kPrepTile, n_waves = static_cast<uint64_t>(gridDim.x) * (kPrepThreads / 64);
    for (uint64_t t = static_cast<uint64_t>(blockIdx.x) * (kPrepThreads / 64) + wave; t < n_tiles; t += n_waves) {
        const PrepTile w = prep_tile(p, t);
        // 1. the masks, requested first: D = add - minus of the lane's T elements
        uint64_t ct[kPrepT];
#pragma unroll
        for (int i = 0; i < kPrepT; i++) {
            const uint32_t jj = 64u * i + lane;
            ct[i] = 0;
            if (jj < w.cnt) {
                ct[i] = __builtin_nontemporal_load(p.add + w.e_lo + jj);
                if (p.minus) ct[i] -= __builtin_nontemporal_load(p.minus + w.e_lo + jj);
            }
        }
        // 2. the plaintexts: ct = (q + add - minus) mod 2^b
        if (w.row >= 0) {
            const CodecLayer *L = p.cq.layers + w.row;
            const uint64_t ls = *FLASHE_CONSTANT(const uint64_t, &L->start);
            const void *const xs = reinterpret_cast<const void *>(*FLASHE_CONSTANT(const uintptr_t, &L->x));
            const bool f64 = *FLASHE_CONSTANT(const int, &L->x_is_f64) != 0;
            const double p0 = *FLASHE_CONSTANT(const double, &L->p0), p1 = *FLASHE_CONSTANT(const double, &L->p1), p2 = *FLASHE_CONSTANT(const double, &L->p2);
            uint64_t raw[kPrepT], ub[kPrepT];
#pragma unroll
            for (int i = 0; i < kPrepT; i++) {
                const uint32_t jj = 64u * i + lane;
                raw[i] = ub[i] = 0;
                if (jj < w.cnt) {
                    raw[i] = cohort_load(xs, f64, p.cq.k0 + w.e_lo + jj - ls);
                    ub[i] = __builtin_nontemporal_load(reinterpret_cast<const uint64_t *>(p.cq.u) + w.e_lo + jj);
                }
            }
#pragma unroll
            for (int i = 0; i < kPrepT; i++)
                ct[i] = (ct[i] + cohort_quantize_raw(raw[i], f64, p0, p1, p2, __longlong_as_double(static_cast<long long>(ub[i])))) & p.mask;
        } else {
            // a tile that straddles a table row: the row looked up per lane
#pragma unroll 1
            for (int i = 0; i < kPrepT; i++) {
                const uint32_t jj = 64u * i + lane;
                if (jj < w.cnt) ct[i] = (ct[i] + codec_quantize(p.cq, w.e_lo + jj)) & p.mask;
            }
        }
        // 3. the fields into the wave's rows: element e_lo + jj is k = cnt - 1 - jj of the tile; the rows [cnt, 64 T) are zero
#pragma unroll
        for (int i = 0; i < kPrepT; i++) {
            const uint32_t jj = 64u * i + lane;
            row0[jj < w.cnt ? w.cnt - 1u - jj : jj] = jj < w.cnt ? ct[i] : 0;
        }
        __builtin_amdgcn_wave_barrier();
        // 4. limb i of the tile: field r = floor(64 i / b) from its bit `in` on, then the fields above it until the limb is full (64 i + 63 <
        // 64 b T: every one of them is one of the wave's rows)
        const uint64_t l0 = static_cast<uint64_t>(b) * kPrepT * t;
        const uint32_t tile_limbs = (w.cnt * b + 63u) >> 6;                                  // b T for a whole tile
        for (uint32_t i = lane; i < tile_limbs; i += 64u) {
            const uint32_t q = 64u * i;
            uint32_t r = static_cast<uint32_t>((static_cast<uint64_t>(q) * p.b_magic) >> 32);
            const uint32_t in = q - r * b;
            uint64_t val = row0[r] >> in;
            for (uint32_t have = b - in; have < 64u; have += b) val |= row0[++r] << have;
            __builtin_nontemporal_store(val, packed + l0 + i);
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// cq.fout[j] = unquantise((element j of the packed sum + add[j] - minus[j]) mod 2^b)
__global__ __launch_bounds__(kPrepThreads) void combine_small_unpack_kernel(const PrepWire p, const uint64_t *__restrict__ packed)
{
#pragma clang fp contract(off)
    __shared__ uint64_t rows[(kPrepThreads / 64) * kPrepTile];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
    uint64_t *row0 = rows + wave * kPrepTile;
    const uint32_t b = p.b;
    double *const out = p.cq.fout;
    const uint64_t n_tiles = (p.n + kPrepTile - 1) / kPrepTile, n_waves = static_cast<uint64_t>(gridDim.x) * (kPrepThreads / 64);
    for (uint64_t t = static_cast<uint64_t>(blockIdx.x) * (kPrepThreads / 64) + wave; t < n_tiles; t += n_waves) {
        const PrepTile w = prep_tile(p, t);
        // 1. the tile's limbs into the wave's rows, lane-contiguously; the masks requested behind them
        const uint64_t l0 = static_cast<uint64_t>(b) * kPrepT * t;
        const uint32_t tile_limbs = (w.cnt * b + 63u) >> 6;
        for (uint32_t i = lane; i < tile_limbs; i += 64u) row0[i] = __builtin_nontemporal_load(packed + l0 + i);
        uint64_t d[kPrepT];
#pragma unroll
        for (int i = 0; i < kPrepT; i++) {
            const uint32_t jj = 64u * i + lane;
            d[i] = 0;
            if (jj < w.cnt) {
                d[i] = __builtin_nontemporal_load(p.add + w.e_lo + jj);
                if (p.minus) d[i] -= __builtin_nontemporal_load(p.minus + w.e_lo + jj);
            }
        }
        __builtin_amdgcn_wave_barrier();
        double p0 = 0, p1 = 0, p2 = 0;
        if (w.row >= 0) {
            const CodecLayer *L = p.cq.layers + w.row;
            p0 = *FLASHE_CONSTANT(const double, &L->p0); p1 = *FLASHE_CONSTANT(const double, &L->p1); p2 = *FLASHE_CONSTANT(const double, &L->p2);
        }
        // 2. the lane's fields: element e_lo + jj lies at bit b (cnt - 1 - jj) of the tile, in one limb or across two (both inside the
        // tile's cnt b bits)
#pragma unroll
        for (int i = 0; i < kPrepT; i++) {
            const uint32_t jj = 64u * i + lane;
            if (jj >= w.cnt) continue;
            const uint32_t pos = b * (w.cnt - 1u - jj), wd = pos >> 6, sh = pos & 63u;
            uint64_t v = row0[wd] >> sh;
            if (sh + b > 64u) v |= row0[wd + 1u] << (64u - sh);
            v = (v + d[i]) & p.mask;
            double res;
            if (w.row >= 0) res = u128_to_double(v) * p1 / p2 - p0;       // codec_unquantize's arithmetic on the row's parameters from SGPRs
            else res = codec_unquantize(p.cq, w.e_lo + jj, v);
            __builtin_nontemporal_store(res, out + w.e_lo + jj);
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// packed: ceil(n b / 64) limbs, every one written here
template <int BS>
__global__ __launch_bounds__(kWideWireThreads) void combine_wide_pack_kernel(const WideTiles p, const uint64_t *__restrict__ add, const uint64_t *__restrict__ minus,
                                                                            uint64_t *__restrict__ packed)
{
    __shared__ uint32_t rows[(kWideWireThreads / 64) * 256];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
    uint32_t *row0 = rows + wave * 256;
    const u128 mask = (static_cast<u128>(p.mask_hi) << 64) | p.mask_lo;
    const uint64_t n_tiles = (p.n + 63) / 64;
    for (uint64_t t = static_cast<uint64_t>(blockIdx.x) * (kWideWireThreads / 64) + wave; t < n_tiles; t += wide_wire_grid_waves()) {
        const WideTile w = wide_tile(p, t);
        const bool valid = lane < w.cnt;
        const uint64_t e = w.e_lo + (valid ? w.cnt - 1u - lane : 0u);
        u128 D = 0;                                                                          // the element's masks, requested first
        if (valid) {
            D = ld128_nt(add + 2 * e);
            if (minus) D -= ld128_nt(minus + 2 * e);
        }
        const u128 F = (wide_plaintext<BS>(p, w, valid, e) + D) & mask;
        wide_stitch(p, w, t, lane, valid, F, row0, packed);
    }
}

// p.out[value] = unquantise(field of (element of the packed sum + add - minus) mod 2^b)
template <int BS>
__global__ __launch_bounds__(kWideWireThreads) void combine_wide_unpack_kernel(const WideTiles p, const uint64_t *__restrict__ add, const uint64_t *__restrict__ minus,
                                                                              const uint64_t *__restrict__ packed)
{
    __shared__ uint32_t rows[(kWideWireThreads / 64) * 256];
    wide_unpack_tiles<BS>(p, rows, [&](uint64_t e) {
        u128 D = ld128_nt(add + 2 * e);
        if (minus) D -= ld128_nt(minus + 2 * e);
        return D;
    }, packed);
}

bool combine_small_wire_admits(const LaunchEnv &env, uint64_t n) { return env.b >= 16 && env.b <= 64 && n >= 1 && n < (1ull << 32); }
bool combine_wide_wire_admits(const LaunchEnv &env, uint64_t n_elems) { return env.b >= 65 && env.b <= 128 && n_elems >= 1 && n_elems < (1ull << 32); }

static PrepWire prep_wire_params(const LaunchEnv &env, uint64_t n, const Codec &cq, const uint64_t *add_dev, const uint64_t *minus_dev)
{
    PrepWire p{};
    uint64_t hi;
    p.cq = cq; p.add = add_dev; p.minus = minus_dev; p.n = n; p.b = static_cast<uint32_t>(env.b);
    p.b_magic = static_cast<uint32_t>(((1ull << 32) + p.b - 1) / p.b);
    masks_of(env.b, &p.mask, &hi);
    return p;
}

// no tables to fill: two workgroups of 16 waves per CU
static dim3 prep_wire_grid(const LaunchEnv &env, uint64_t n)
{
    const uint64_t tiles = (n + kPrepTile - 1) / kPrepTile, groups = (tiles + kPrepThreads / 64 - 1) / (kPrepThreads / 64), cap = 2 * static_cast<uint64_t>(env.num_cus);
    return dim3(static_cast<unsigned>(groups < cap ? groups : cap));
}

hipError_t launch_combine_small_pack(const LaunchEnv &env, uint64_t n, const Codec &cq, const uint64_t *add_dev, const uint64_t *minus_dev, uint64_t *packed_dev)
{
    if (!combine_small_wire_admits(env, n) || !cq.layers || !cq.u || cq.k0 != 0 || !add_dev || !packed_dev) return hipErrorNotSupported;
    hipLaunchKernelGGL(combine_small_pack_kernel, prep_wire_grid(env, n), dim3(kPrepThreads), 0, env.stream, prep_wire_params(env, n, cq, add_dev, minus_dev), packed_dev);
    return hipGetLastError();
}

hipError_t launch_combine_small_unpack(const LaunchEnv &env, uint64_t n, const uint64_t *packed_dev, const uint64_t *add_dev, const uint64_t *minus_dev, const Codec &cq)
{
    if (!combine_small_wire_admits(env, n) || !cq.layers || !cq.fout || cq.k0 != 0 || !add_dev || !packed_dev) return hipErrorNotSupported;
    hipLaunchKernelGGL(combine_small_unpack_kernel, prep_wire_grid(env, n), dim3(kPrepThreads), 0, env.stream, prep_wire_params(env, n, cq, add_dev, minus_dev), packed_dev);
    return hipGetLastError();
}

hipError_t launch_combine_wide_pack(const LaunchEnv &env, const BatchLayer *layers_dev, int n_layers, int field_bits, const double *u_dev, uint64_t n_elems,
                                    const uint64_t *add_dev, const uint64_t *minus_dev, uint64_t *packed_dev)
{
    if (!combine_wide_wire_admits(env, n_elems) || !layers_dev || n_layers < 1 || !u_dev || !add_dev || !packed_dev || field_bits < 1 || field_bits > env.b)
        return hipErrorNotSupported;
    WideTiles p = wide_tiles_params(env, layers_dev, n_layers, field_bits, n_elems);
    p.u = u_dev;
    const dim3 grid = wide_wire_grid(env, n_elems), block(kWideWireThreads);
    switch (p.bs) {
    case 5: hipLaunchKernelGGL(combine_wide_pack_kernel<5>, grid, block, 0, env.stream, p, add_dev, minus_dev, packed_dev); break;
    case 6: hipLaunchKernelGGL(combine_wide_pack_kernel<6>, grid, block, 0, env.stream, p, add_dev, minus_dev, packed_dev); break;
    case 7: hipLaunchKernelGGL(combine_wide_pack_kernel<7>, grid, block, 0, env.stream, p, add_dev, minus_dev, packed_dev); break;
    default: hipLaunchKernelGGL(combine_wide_pack_kernel<0>, grid, block, 0, env.stream, p, add_dev, minus_dev, packed_dev); break;
    }
    return hipGetLastError();
}

hipError_t launch_combine_wide_unpack(const LaunchEnv &env, const BatchLayer *layers_dev, int n_layers, int field_bits, const uint64_t *packed_dev, uint64_t n_elems,
                                      const uint64_t *add_dev, const uint64_t *minus_dev, double *out_dev)
{
    if (!combine_wide_wire_admits(env, n_elems) || !layers_dev || n_layers < 1 || !packed_dev || !add_dev || !out_dev || field_bits < 1 || field_bits > env.b)
        return hipErrorNotSupported;
    WideTiles p = wide_tiles_params(env, layers_dev, n_layers, field_bits, n_elems);
    p.out = out_dev;
    const dim3 grid = wide_wire_grid(env, n_elems), block(kWideWireThreads);
    switch (p.bs) {
    case 5: hipLaunchKernelGGL(combine_wide_unpack_kernel<5>, grid, block, 0, env.stream, p, add_dev, minus_dev, packed_dev); break;
    case 6: hipLaunchKernelGGL(combine_wide_unpack_kernel<6>, grid, block, 0, env.stream, p, add_dev, minus_dev, packed_dev); break;
    case 7: hipLaunchKernelGGL(combine_wide_unpack_kernel<7>, grid, block, 0, env.stream, p, add_dev, minus_dev, packed_dev); break;
    default: hipLaunchKernelGGL(combine_wide_unpack_kernel<0>, grid, block, 0, env.stream, p, add_dev, minus_dev, packed_dev); break;
    }
    return hipGetLastError();
}

}  // namespace flashe
