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
#include "wire_tiles.h"
#include "wire_lists.h"

namespace flashe {

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
    const CtrPrefix pre_a = scalar_prefix(ctr_prefix(rk, lr, iter, add_idx, 0u));            // n < 2^32 (host-checked): the high counter word is 0
    CtrPrefix pre_b{};
    if (DBL) pre_b = scalar_prefix(ctr_prefix(rk, lr, iter, minus_idx, 0u));
    const uint64_t n_tiles = (p.n + 63) / 64;
    for (uint64_t t = static_cast<uint64_t>(blockIdx.x) * (kWideWireThreads / 64) + wave; t < n_tiles; t += wide_wire_grid_waves()) {
        const WideTile w = wide_tile(p, t);
        const bool valid = lane < w.cnt;
        const uint64_t e = w.e_lo + (valid ? w.cnt - 1u - lane : 0u);                        // the lane's element = its PRF counter
        // 1. the batched plaintext, before the AES rounds
        const u128 P = wide_plaintext<BS>(p, w, valid, e);
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
        wide_stitch(p, w, t, lane, valid, F, row0, packed);
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
    wide_unpack_tiles<BS>(p, rows, [&](uint64_t e) {
        const CtrVar x = ctr_var(rk, lr, static_cast<uint32_t>(e));
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
    wide_unpack_tiles<BS>(p, rows, [&](uint64_t e) {
        return wire_lists_mask<true>(rk, lr, pre, ls.n_add, ls.n, ctr_var(rk, lr, static_cast<uint32_t>(e)), [](u128 D, u128 S, bool add) { return add ? D + S : D - S; });
    }, packed);
}

bool wide_wire_admits(const LaunchEnv &env, uint64_t n_elems)
{
    return env.b >= 65 && env.b <= 128 && n_elems >= 1 && n_elems < (1ull << 32) && (env.prf_backend == PRF_AUTO || env.prf_backend == PRF_TABLE);
}

static WideWire wide_wire_params(const LaunchEnv &env, uint32_t iter, const BatchLayer *layers_dev, int n_layers, int field_bits, uint64_t n_elems)
{
    WideWire p{};
    static_cast<WideTiles &>(p) = wide_tiles_params(env, layers_dev, n_layers, field_bits, n_elems);
    p.te0 = env.te0_dev; p.iter = iter;
    return p;
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
