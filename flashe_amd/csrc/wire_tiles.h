// What the kernels that go straight to and from the packed WIRE form share (wire.hip, wire_wide.hip: the masks from the PRF;
// wire_prepared.hip: the masks from the ctx's precompute cache): the table rows of a tile and, at int_bits 65 .. 128, the tile anchored at
// the END of the vector with its batched front end, its stitch into limbs and its walk back (stated in wire_wide.hip's head comment).
#pragma once
#include "device_common.h"

namespace flashe {

// the wave-uniform table row that holds flat element `key` (the last row with start <= key), found with scalar loads
__device__ __forceinline__ int wire_row_of(const CodecLayer *layers, int n_layers, uint64_t key)
{
    int lo = 0, hi = n_layers - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (*FLASHE_CONSTANT(const uint64_t, &layers[mid].start) <= key) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// The row that holds ALL of the elements [e0, e1) of a tile, or -1 when they straddle a row boundary (at most one tile per layer: those
// look every element's row up per lane).  e0, e1: wave-uniform.
__device__ __forceinline__ int wire_tile_row(const Codec &cq, uint64_t e0, uint64_t e1, uint64_t n)
{
    const int row = wire_row_of(cq.layers, cq.n_layers, cq.k0 + e0);
    const uint64_t end = row + 1 < cq.n_layers ? *FLASHE_CONSTANT(const uint64_t, &cq.layers[row + 1].start) : cq.k0 + n;
    return cq.k0 + e1 <= end ? row : -1;
}

// ---- int_bits 65 .. 128, batched ----
constexpr int kWideWireThreads = 1024;

struct WideTiles {
    const BatchLayer *layers;
    const double *u;           // pack: the model's draws, value-indexed
    double *out;               // unpack: the model's float64 values, value-indexed
    uint64_t n;                // batched elements
    uint64_t mask_lo, mask_hi;
    uint32_t b_magic;          // ceil(2^32 / b): x / b == (x * b_magic) >> 32 for x < 2^13
    int n_layers, b, bs, field_bits;
};
// the same for a launch that runs the PRF (wire_wide.hip)
struct WideWire : WideTiles {
    const uint32_t *te0;
    uint32_t iter;
};

// the wave-uniform table row that holds batched element `key` (the last row with elem_start <= key), found with scalar loads
__device__ __forceinline__ int wide_row_of(const BatchLayer *layers, int n_layers, uint64_t key)
{
    int lo = 0, hi = n_layers - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (*FLASHE_CONSTANT(const uint64_t, &layers[mid].elem_start) <= key) lo = mid; else hi = mid - 1;
    }
    return lo;
}
// the same per lane
__device__ __forceinline__ const BatchLayer *wide_layer_of(const BatchLayer *layers, int n_layers, uint64_t key)
{
    int lo = 0, hi = n_layers - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (layers[mid].elem_start <= key) lo = mid; else hi = mid - 1;
    }
    return layers + lo;
}

// One row of the table in SGPRs.
struct WideRow {
    uint64_t es, vs, size;
    const void *x;
    double p0, p1, p2;
    bool f64;
};
__device__ __forceinline__ WideRow wide_row(const BatchLayer *L)
{
    return WideRow{*FLASHE_CONSTANT(const uint64_t, &L->elem_start), *FLASHE_CONSTANT(const uint64_t, &L->value_start), *FLASHE_CONSTANT(const uint64_t, &L->size),
                   reinterpret_cast<const void *>(*FLASHE_CONSTANT(const uintptr_t, &L->x)), *FLASHE_CONSTANT(const double, &L->p0),
                   *FLASHE_CONSTANT(const double, &L->p1), *FLASHE_CONSTANT(const double, &L->p2), *FLASHE_CONSTANT(const int, &L->x_is_f64) != 0};
}

// Tile t of the vector: the elements [e_lo, e_lo + cnt) = k in [64 t, 64 t + cnt), k = n - 1 - element.  row: the table row that holds
// ALL of them with every one a whole element of bs values (none is the row's padded last element), or -1.  All wave-uniform.
struct WideTile { uint64_t e_lo; uint32_t cnt; int row; };
__device__ __forceinline__ WideTile wide_tile(const WideTiles &p, uint64_t t)
{
    WideTile w;
    const uint64_t left = p.n - 64u * t;
    w.cnt = left < 64u ? static_cast<uint32_t>(left) : 64u;
    w.e_lo = left - w.cnt;
    const int row = wide_row_of(p.layers, p.n_layers, w.e_lo);
    const uint64_t es = *FLASHE_CONSTANT(const uint64_t, &p.layers[row].elem_start), size = *FLASHE_CONSTANT(const uint64_t, &p.layers[row].size);
    // (the elements past the row's last one belong to the next row: (e - es) bs >= size for them too)
    w.row = (w.e_lo + w.cnt - es) * static_cast<uint64_t>(p.bs) <= size ? row : -1;
    return w;
}

__device__ __forceinline__ uint32_t wide_wire_grid_waves() { return gridDim.x * (kWideWireThreads / 64); }

// the batched plaintext of the lane's element e of tile w (quantize_batch_model_kernel's arithmetic)
template <int BS>
__device__ __forceinline__ u128 wide_plaintext(const WideTiles &p, const WideTile &w, bool valid, uint64_t e)
{
    u128 P = 0;
    if (w.row >= 0) {
        const WideRow r = wide_row(p.layers + w.row);
        if (valid) {
            const uint64_t j0 = (e - r.es) * static_cast<uint64_t>(p.bs);
            if constexpr (BS != 0) P = cohort_batch_element<BS>(r.x, r.f64, r.p0, r.p1, r.p2, p.u + r.vs, j0, r.size, p.field_bits);
            else P = cohort_batch_walk<0>(r.x, r.f64, r.p0, r.p1, r.p2, p.u + r.vs, j0, r.size, p.field_bits, p.bs);
        }
    } else if (valid) {
        const BatchLayer *L = wide_layer_of(p.layers, p.n_layers, e);
        P = cohort_batch_walk<BS>(L->x, L->x_is_f64 != 0, L->p0, L->p1, L->p2, p.u + L->value_start, (e - L->elem_start) * static_cast<uint64_t>(p.bs), L->size,
                                  p.field_bits, p.bs);
    }
    return P;
}

// The limbs of tile t from the lanes' b-bit fields F (lane L: k = 64 t + L) through the wave's 16-byte LDS rows row0: limb i of the tile
// starts in field r = floor(64 i / b) and, b being above 64, overlaps at most field r + 1 too; lane i emits limb i (and i + 64),
// coalesced non-temporal 8-byte stores.  b = 128: the field is two whole limbs, stored directly.
__device__ __forceinline__ void wide_stitch(const WideTiles &p, const WideTile &w, uint64_t t, uint32_t lane, bool valid, u128 F, uint32_t *row0,
                                            uint64_t *__restrict__ packed)
{
    const uint32_t b = static_cast<uint32_t>(p.b);
    const uint64_t l0 = static_cast<uint64_t>(b) * t;
    if (b == 128u) {
        if (valid) st128_nt(packed + l0 + 2u * lane, F);
        return;
    }
    if (!valid) F = 0;                                                                   // (the top tile: its limbs' unused bits)
    *reinterpret_cast<uint4 *>(row0 + 4 * lane) = make_uint4(static_cast<uint32_t>(F), static_cast<uint32_t>(F >> 32), static_cast<uint32_t>(F >> 64), static_cast<uint32_t>(F >> 96));
    __builtin_amdgcn_wave_barrier();
    const uint32_t tile_limbs = (w.cnt * b + 63u) >> 6;                                  // b for a whole tile
    for (uint32_t i = lane; i < tile_limbs; i += 64u) {
        const uint32_t q = 64u * i;                                                      // the limb's first bit in the tile
        const uint32_t r = static_cast<uint32_t>((static_cast<uint64_t>(q) * p.b_magic) >> 32);
        const uint32_t in = q - r * b, have = b - in;                                    // field r from its bit `in` on: `have` >= 1 bits
        const uint4 a = *reinterpret_cast<const uint4 *>(row0 + 4 * r);
        const u128 Fa = (static_cast<u128>((static_cast<uint64_t>(a.w) << 32) | a.z) << 64) | ((static_cast<uint64_t>(a.y) << 32) | a.x);
        uint64_t val = static_cast<uint64_t>(Fa >> in);
        if (have < 64u) {                                                                // (q + 63 < 64 b: field r + 1 is one of the wave's rows)
            const uint2 c = *reinterpret_cast<const uint2 *>(row0 + 4 * (r + 1u));
            val |= ((static_cast<uint64_t>(c.y) << 32) | c.x) << have;
        }
        __builtin_nontemporal_store(val, packed + l0 + i);
    }
    __builtin_amdgcn_wave_barrier();
}

// The way back over every tile of the launch: mid(e) = the mask S_add - S_minus (mod 2^128) of element e (asked of every lane; a lane
// past the top tile's elements asks for the tile's first one).  rows: 256 words per wave.
template <int BS, class Mid>
__device__ __forceinline__ void wide_unpack_tiles(const WideTiles &p, uint32_t *rows, const Mid &mid, const uint64_t *__restrict__ packed)
{
#pragma clang fp contract(off)
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
    uint32_t *row0 = rows + wave * 256;
    const u128 mask = (static_cast<u128>(p.mask_hi) << 64) | p.mask_lo;
    const uint32_t b = static_cast<uint32_t>(p.b), fb = static_cast<uint32_t>(p.field_bits);
    const u128 fmask = fb >= 128u ? ~static_cast<u128>(0) : (static_cast<u128>(1) << fb) - 1;
    double *const out = p.out;
    const uint64_t n_tiles = (p.n + 63) / 64;
    for (uint64_t t = static_cast<uint64_t>(blockIdx.x) * (kWideWireThreads / 64) + wave; t < n_tiles; t += wide_wire_grid_waves()) {
        const WideTile w = wide_tile(p, t);
        const bool valid = lane < w.cnt;
        const uint64_t e = w.e_lo + (valid ? w.cnt - 1u - lane : 0u);
        // 1. the limbs the lane's field [b k, b k + b) overlaps, requested before the mask: b > 64, so always two, and a third one when
        // the field ends past them (all inside the integer's n b bits)
        const uint64_t pos = static_cast<uint64_t>(b) * (64u * t + lane);
        const uint64_t l = pos >> 6;
        const uint32_t sh = static_cast<uint32_t>(pos) & 63u;
        uint64_t g0 = 0, g1 = 0, g2 = 0;
        if (valid) {
            g0 = __builtin_nontemporal_load(packed + l);
            g1 = __builtin_nontemporal_load(packed + l + 1);
            if (sh + b > 128u) g2 = __builtin_nontemporal_load(packed + l + 2);
        }
        // 2. the element's mask
        const u128 D = mid(e);
        u128 F = (static_cast<u128>(g1) << 64) | g0;
        if (sh) F = (F >> sh) | (static_cast<u128>(g2) << (128u - sh));
        const u128 X = (F + D) & mask;                                                       // the decrypted element
        // 3. the fields: value t of the element is its field bs - 1 - t (the first value most significant)
        if (BS != 0 && w.row >= 0) {
            // a whole tile of whole elements inside one row: through the wave's rows, then cnt BS consecutive values lane-contiguously
            const WideRow r = wide_row(p.layers + w.row);
            *reinterpret_cast<uint4 *>(row0 + 4 * lane) = make_uint4(static_cast<uint32_t>(X), static_cast<uint32_t>(X >> 32), static_cast<uint32_t>(X >> 64), static_cast<uint32_t>(X >> 96));
            __builtin_amdgcn_wave_barrier();
            double *const o = out + r.vs + (w.e_lo - r.es) * static_cast<uint64_t>(BS);
            const uint32_t n_vals = w.cnt * static_cast<uint32_t>(BS ? BS : 1);
            for (uint32_t v = lane; v < n_vals; v += 64u) {
                const uint32_t eo = v / static_cast<uint32_t>(BS ? BS : 1), slot = v - eo * static_cast<uint32_t>(BS ? BS : 1);
                const uint4 a = *reinterpret_cast<const uint4 *>(row0 + 4 * (w.cnt - 1u - eo));
                const u128 Xa = (static_cast<u128>((static_cast<uint64_t>(a.w) << 32) | a.z) << 64) | ((static_cast<uint64_t>(a.y) << 32) | a.x);
                const uint64_t f = static_cast<uint64_t>(Xa >> (fb * (static_cast<uint32_t>(BS) - 1u - slot))) & static_cast<uint64_t>(fmask);   // BS >= 5: a field has at most 25 bits
                const double res = static_cast<double>(f) * r.p1 / r.p2 - r.p0;          // unbatch_unquantize_model_kernel's arithmetic, the row's parameters from SGPRs
                __builtin_nontemporal_store(res, o + v);
            }
            __builtin_amdgcn_wave_barrier();
        } else if (valid) {
            const BatchLayer *L = wide_layer_of(p.layers, p.n_layers, e);
            const uint64_t j0 = (e - L->elem_start) * static_cast<uint64_t>(p.bs), size = L->size;
            const double p0 = L->p0, p1 = L->p1, p2 = L->p2;
            double *const o = out + L->value_start + j0;
#pragma unroll 1
            for (int tt = 0; tt < p.bs && j0 + tt < size; tt++) {                            // pads store nothing
                const u128 f = (X >> (fb * static_cast<uint32_t>(p.bs - 1 - tt))) & fmask;
                o[tt] = u128_to_double(f) * p1 / p2 - p0;
            }
        }
    }
}

// the launch's parameters but u / out
static inline WideTiles wide_tiles_params(const LaunchEnv &env, const BatchLayer *layers_dev, int n_layers, int field_bits, uint64_t n_elems)
{
    WideTiles p{};
    p.layers = layers_dev; p.n_layers = n_layers; p.n = n_elems;
    p.b = env.b; p.field_bits = field_bits; p.bs = env.b / field_bits;
    p.b_magic = static_cast<uint32_t>(((1ull << 32) + static_cast<uint32_t>(env.b) - 1) / static_cast<uint32_t>(env.b));
    masks_of(env.b, &p.mask_lo, &p.mask_hi);
    return p;
}

static inline dim3 wide_wire_grid(const LaunchEnv &env, uint64_t n_elems)
{
    const uint64_t tiles = (n_elems + 63) / 64, groups = (tiles + kWideWireThreads / 64 - 1) / (kWideWireThreads / 64), cus = static_cast<uint64_t>(env.num_cus);
    return dim3(static_cast<unsigned>(groups < cus ? groups : cus));
}

}  // namespace flashe
