// The BATCHED client step straight to and from the packed WIRE form at int_bits 65 .. 128 (the *_q16_b6_* jobs: int_bits 120, six
// quantised values per element; JZFTransferableWeights.compress / decompress, jzf_weights.py:155-231):
//   prf_wide_pack_kernel<DBL, BS>   float model + draws -> quantise -> batch -> encrypt -> packed limbs   (no 16-byte vector in HBM)
//   prf_wide_unpack_kernel<BS>      packed limbs of the sum -> decrypt -> unbatch -> unquantise -> float64 model
//   prf_wide_unpack_lists_kernel<BS>  the same with prefix LISTS of up to kMaxIdx each (a dropout, the single mask's decrypt; wire_lists.h)
// At these widths an element is ONE AES block and its counter is the element index: the chunking does not enter, and nothing ties the
// tiling to AES blocks.  It is tied to the LIMBS of the integer instead, and anchored at the END of the vector: element j of n sits at bits
// [b (n - 1 - j), b (n - j)); with k = n - 1 - j, tile t = the elements k in [64 t, 64 t + 64) covers bits [64 b t, 64 b (t + 1)) --
// exactly the b whole limbs b t .. b t + b - 1.  So no limb is shared between tiles: every limb is written once with a plain store, there
// is no atomic OR and no fill launch in front.  The only partial tile is the top one (the first n mod 64 elements): its wave writes
// ceil(cnt b / 64) limbs, the unused top bits zero.
// Lane L of the wave that owns tile t takes k = 64 t + L: ascending lane = ascending bit position, and its b-bit field goes to the
// wave's 16-byte LDS row L as it is.
//   pack: plaintext (quantize_batch_model_kernel's arithmetic, built BEFORE the rounds: only one 128-bit word lives through them), the
//   element's add block and (DBL) its minus block as one pipelined pair, ct = (pt + S_add - S_minus) mod 2^b, then the stitch: limb i of
//   the tile starts in field r = floor(64 i / b) and, b being above 64, overlaps at most field r + 1 too; lane i emits limb i (and
//   i + 64), coalesced non-temporal 8-byte stores.  b = 128: the field is two whole limbs, stored directly.
//   unpack: the lane loads the two or three limbs its field overlaps before the rounds, decrypts, and the bs fields become floats.  A tile
//   inside one row goes through the wave's rows and is walked lane-contiguously (64 bs consecutive float64 values, coalesced stores); a
//   tile that crosses rows or holds a row's padded last element stores from registers, the row looked up per lane.
#include "device_common.h"
#include "wire_lists.h"

namespace flashe {

namespace {

constexpr int kWideWireThreads = 1024;

struct WideWire {
    const BatchLayer *layers;
    const double *u;           // pack: the model's draws, value-indexed
    double *out;               // unpack: the model's float64 values, value-indexed
    const uint32_t *te0;
    uint64_t n;                // batched elements
    uint64_t mask_lo, mask_hi;
    uint32_t iter, b_magic;    // b_magic = ceil(2^32 / b): x / b == (x * b_magic) >> 32 for x < 2^13
    int n_layers, b, bs, field_bits;
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
__device__ __forceinline__ WideTile wide_tile(const WideWire &p, uint64_t t)
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

}  // namespace

// packed: ceil(n b / 64) limbs, every one written here (none needs to be zero on entry)
template <bool DBL, int BS>
__global__ __launch_bounds__(kWideWireThreads) void prf_wide_pack_kernel(const RoundKeys rk, const WideWire p, uint32_t add_idx, uint32_t minus_idx,
                                                                        uint64_t *__restrict__ packed)
{
    const uint32_t iter = p.iter + p.te0[kIterShiftWord];
    __shared__ uint32_t tab[kTabWords];
    __shared__ uint32_t rows[(kWideWireThreads / 64) * 256];
    fill_tables(tab, p.te0);
    const LaneRegs lr = lane_regs(tab);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
    uint32_t *row0 = rows + wave * 256;
    const u128 mask = (static_cast<u128>(p.mask_hi) << 64) | p.mask_lo;
    const uint32_t b = static_cast<uint32_t>(p.b);
    const CtrPrefix pre_a = scalar_prefix(ctr_prefix(rk, lr, iter, add_idx, 0u));            // n < 2^32 (host-checked): the high counter word is 0
    CtrPrefix pre_b{};
    if (DBL) pre_b = scalar_prefix(ctr_prefix(rk, lr, iter, minus_idx, 0u));
    const uint64_t n_tiles = (p.n + 63) / 64;
    for (uint64_t t = static_cast<uint64_t>(blockIdx.x) * (kWideWireThreads / 64) + wave; t < n_tiles; t += wide_wire_grid_waves()) {
        const WideTile w = wide_tile(p, t);
        const bool valid = lane < w.cnt;
        const uint64_t e = w.e_lo + (valid ? w.cnt - 1u - lane : 0u);                        // the lane's element = its PRF counter
        // 1. the batched plaintext, before the AES rounds
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
        // 2. + 3. the element's blocks, ct = (pt + S_add - S_minus) mod 2^b
        const CtrVar x = ctr_var(rk, lr, static_cast<uint32_t>(e));
        u128 F;
        if constexpr (DBL) {
            uint32_t s[2][4];
            ctr_round1(pre_a, x, s[0]);
            ctr_round1(pre_b, x, s[1]);
            aes256_rounds<2, 2>(rk, lr, s, true);
            F = (P + words_to_u128(s[0]) - words_to_u128(s[1])) & mask;
        } else {
            uint32_t s[4];
            ctr_round1(pre_a, x, s);
            aes256_rounds1_deep<2>(rk, lr, s, true);
            F = (P + words_to_u128(s)) & mask;
        }
        // 4. the limbs
        const uint64_t l0 = static_cast<uint64_t>(b) * t;
        if (b == 128u) {
            if (valid) st128_nt(packed + l0 + 2u * lane, F);
            continue;
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
}

// The way back, shared by the one-prefix and the lists kernel: mid(x) = the element's mask S_add - S_minus (mod 2^128) at counter part x.
template <int BS, class Mid>
__device__ __forceinline__ void wide_unpack_tiles(const RoundKeys &rk, const WideWire &p, const LaneRegs lr, uint32_t *rows, const Mid &mid,
                                                  const uint64_t *__restrict__ packed)
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
        // 1. the limbs the lane's field [b k, b k + b) overlaps, requested before the rounds: b > 64, so always two, and a third one when
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
        // 2. the prefixes the host's telescoping left
        const u128 D = mid(ctr_var(rk, lr, static_cast<uint32_t>(e)));
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

// out[value] = unquantise(field of (element of the packed sum + S_add - S_minus) mod 2^b); flags: bit 0 = an add prefix, bit 1 = a minus prefix
template <int BS>
__global__ __launch_bounds__(kWideWireThreads) void prf_wide_unpack_kernel(const RoundKeys rk, const WideWire p, uint32_t add_idx, uint32_t minus_idx, int flags,
                                                                          const uint64_t *__restrict__ packed)
{
    const uint32_t iter = p.iter + p.te0[kIterShiftWord];
    __shared__ uint32_t tab[kTabWords];
    __shared__ uint32_t rows[(kWideWireThreads / 64) * 256];
    fill_tables(tab, p.te0);
    const LaneRegs lr = lane_regs(tab);
    const bool has_add = (flags & 1) != 0, has_minus = (flags & 2) != 0;
    const CtrPrefix pre_a = scalar_prefix(ctr_prefix(rk, lr, iter, has_add ? add_idx : minus_idx, 0u));        // n < 2^32 (host-checked)
    CtrPrefix pre_b{};
    if (has_add && has_minus) pre_b = scalar_prefix(ctr_prefix(rk, lr, iter, minus_idx, 0u));
    wide_unpack_tiles<BS>(rk, p, lr, rows, [&](const CtrVar &x) {
        if (has_add && has_minus) {
            uint32_t s[2][4];
            ctr_round1(pre_a, x, s[0]);
            ctr_round1(pre_b, x, s[1]);
            aes256_rounds<2, 2>(rk, lr, s, true);
            return words_to_u128(s[0]) - words_to_u128(s[1]);
        }
        uint32_t s[4];
        ctr_round1(pre_a, x, s);
        aes256_rounds1_deep<2>(rk, lr, s, true);
        const u128 D = words_to_u128(s);
        return has_add ? D : -D;
    }, packed);
}

// The same with prefix LISTS (a round with a dropout, the single mask's decrypt): the element's mask is sum_k S(add[k]) - sum_k S(minus[k])
// mod 2^128 (the back end masks to b bits), the prefixes' round-1 states in an LDS table the kernel builds (wire_lists.h).
template <int BS>
__global__ __launch_bounds__(kWideWireThreads) void prf_wide_unpack_lists_kernel(const RoundKeys rk, const WideWire p, const WireLists ls,
                                                                                const uint64_t *__restrict__ packed)
{
    const uint32_t iter = p.iter + p.te0[kIterShiftWord];
    __shared__ uint32_t tab[kTabWords];
    __shared__ uint32_t rows[(kWideWireThreads / 64) * 256];
    __shared__ uint4 pre[2 * kMaxIdx];
    fill_tables(tab, p.te0);
    const LaneRegs lr = lane_regs(tab);
    wire_prefix_table(rk, lr, iter, ls, pre);
    wide_unpack_tiles<BS>(rk, p, lr, rows, [&](const CtrVar &x) {
        return wire_lists_mask<true>(rk, lr, pre, ls.n_add, ls.n, x, [](u128 D, u128 S, bool add) { return add ? D + S : D - S; });
    }, packed);
}

bool wide_wire_admits(const LaunchEnv &env, uint64_t n_elems)
{
    return env.b >= 65 && env.b <= 128 && n_elems >= 1 && n_elems < (1ull << 32) && (env.prf_backend == PRF_AUTO || env.prf_backend == PRF_TABLE);
}

static WideWire wide_wire_params(const LaunchEnv &env, uint32_t iter, const BatchLayer *layers_dev, int n_layers, int field_bits, uint64_t n_elems)
{
    WideWire p{};
    p.layers = layers_dev; p.n_layers = n_layers; p.te0 = env.te0_dev; p.n = n_elems; p.iter = iter;
    p.b = env.b; p.field_bits = field_bits; p.bs = env.b / field_bits;
    p.b_magic = static_cast<uint32_t>(((1ull << 32) + static_cast<uint32_t>(env.b) - 1) / static_cast<uint32_t>(env.b));
    masks_of(env.b, &p.mask_lo, &p.mask_hi);
    return p;
}

static dim3 wide_wire_grid(const LaunchEnv &env, uint64_t n_elems)
{
    const uint64_t tiles = (n_elems + 63) / 64, groups = (tiles + kWideWireThreads / 64 - 1) / (kWideWireThreads / 64), cus = static_cast<uint64_t>(env.num_cus);
    return dim3(static_cast<unsigned>(groups < cus ? groups : cus));
}

template <bool DBL>
static void wide_pack_launch(const LaunchEnv &env, const WideWire &p, uint32_t add_idx, uint32_t minus_idx, uint64_t *packed_dev)
{
    const dim3 grid = wide_wire_grid(env, p.n), block(kWideWireThreads);
    switch (p.bs) {
    case 5: hipLaunchKernelGGL((prf_wide_pack_kernel<DBL, 5>), grid, block, 0, env.stream, env.rk, p, add_idx, minus_idx, packed_dev); break;
    case 6: hipLaunchKernelGGL((prf_wide_pack_kernel<DBL, 6>), grid, block, 0, env.stream, env.rk, p, add_idx, minus_idx, packed_dev); break;
    case 7: hipLaunchKernelGGL((prf_wide_pack_kernel<DBL, 7>), grid, block, 0, env.stream, env.rk, p, add_idx, minus_idx, packed_dev); break;
    default: hipLaunchKernelGGL((prf_wide_pack_kernel<DBL, 0>), grid, block, 0, env.stream, env.rk, p, add_idx, minus_idx, packed_dev); break;
    }
}

hipError_t launch_wide_pack(const LaunchEnv &env, uint32_t iter, uint32_t add_idx, bool dbl, uint32_t minus_idx, const BatchLayer *layers_dev, int n_layers,
                            int field_bits, const double *u_dev, uint64_t n_elems, uint64_t *packed_dev)
{
    if (!wide_wire_admits(env, n_elems) || !layers_dev || n_layers < 1 || !u_dev || !packed_dev || field_bits < 1 || field_bits > env.b) return hipErrorNotSupported;
    WideWire p = wide_wire_params(env, iter, layers_dev, n_layers, field_bits, n_elems);
    p.u = u_dev;
    if (dbl) wide_pack_launch<true>(env, p, add_idx, minus_idx, packed_dev);
    else wide_pack_launch<false>(env, p, add_idx, 0u, packed_dev);
    return hipGetLastError();
}

hipError_t launch_wide_unpack(const LaunchEnv &env, uint32_t iter, bool has_add, uint32_t add_idx, bool has_minus, uint32_t minus_idx, const BatchLayer *layers_dev,
                              int n_layers, int field_bits, const uint64_t *packed_dev, uint64_t n_elems, double *out_dev)
{
    if (!wide_wire_admits(env, n_elems) || !layers_dev || n_layers < 1 || !packed_dev || !out_dev || field_bits < 1 || field_bits > env.b || !(has_add || has_minus))
        return hipErrorNotSupported;
    WideWire p = wide_wire_params(env, iter, layers_dev, n_layers, field_bits, n_elems);
    p.out = out_dev;
    const dim3 grid = wide_wire_grid(env, n_elems), block(kWideWireThreads);
    const int flags = (has_add ? 1 : 0) | (has_minus ? 2 : 0);
    switch (p.bs) {
    case 5: hipLaunchKernelGGL(prf_wide_unpack_kernel<5>, grid, block, 0, env.stream, env.rk, p, add_idx, minus_idx, flags, packed_dev); break;
    case 6: hipLaunchKernelGGL(prf_wide_unpack_kernel<6>, grid, block, 0, env.stream, env.rk, p, add_idx, minus_idx, flags, packed_dev); break;
    case 7: hipLaunchKernelGGL(prf_wide_unpack_kernel<7>, grid, block, 0, env.stream, env.rk, p, add_idx, minus_idx, flags, packed_dev); break;
    default: hipLaunchKernelGGL(prf_wide_unpack_kernel<0>, grid, block, 0, env.stream, env.rk, p, add_idx, minus_idx, flags, packed_dev); break;
    }
    return hipGetLastError();
}

hipError_t launch_wide_unpack_lists(const LaunchEnv &env, uint32_t iter, const uint32_t *add, int n_add, const uint32_t *minus, int n_minus,
                                    const BatchLayer *layers_dev, int n_layers, int field_bits, const uint64_t *packed_dev, uint64_t n_elems, double *out_dev)
{
    if (!wide_wire_admits(env, n_elems) || !wire_lists_admit(n_add, n_minus) || !layers_dev || n_layers < 1 || !packed_dev || !out_dev || field_bits < 1 ||
        field_bits > env.b)
        return hipErrorNotSupported;
    WideWire p = wide_wire_params(env, iter, layers_dev, n_layers, field_bits, n_elems);
    p.out = out_dev;
    const dim3 grid = wide_wire_grid(env, n_elems), block(kWideWireThreads);
    const WireLists ls = wire_lists_of(add, n_add, minus, n_minus);
    switch (p.bs) {
    case 5: hipLaunchKernelGGL(prf_wide_unpack_lists_kernel<5>, grid, block, 0, env.stream, env.rk, p, ls, packed_dev); break;
    case 6: hipLaunchKernelGGL(prf_wide_unpack_lists_kernel<6>, grid, block, 0, env.stream, env.rk, p, ls, packed_dev); break;
    case 7: hipLaunchKernelGGL(prf_wide_unpack_lists_kernel<7>, grid, block, 0, env.stream, env.rk, p, ls, packed_dev); break;
    default: hipLaunchKernelGGL(prf_wide_unpack_lists_kernel<0>, grid, block, 0, env.stream, env.rk, p, ls, packed_dev); break;
    }
    return hipGetLastError();
}

}  // namespace flashe
