// gfx950 kernels of the FLASHE cipher engine that are bound by HBM streaming: combine (precomputed masks), the arbiter's element-wise
// and packed reduces with their multi-GPU slice helpers, the bit-packing codec, and the sparse passes (span bounds / span reduce,
// scatter, run-edge masks, shared positions).  The AES core they need comes from device_common.h.
#include "device_common.h"

namespace flashe {

// ------------------------------------------------------------------------------------------
// Streaming kernels (HBM-bound)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kStreamThreads) void widen_u32_kernel(uint64_t n, const uint32_t *in, uint64_t *out)
{
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x; j < n; j += static_cast<uint64_t>(gridDim.x) * kStreamThreads)
        out[j] = in[j];
}
__global__ __launch_bounds__(kStreamThreads) void narrow_u32_kernel(uint64_t n, const uint64_t *in, uint32_t *out)
{
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x; j < n; j += static_cast<uint64_t>(gridDim.x) * kStreamThreads)
        out[j] = static_cast<uint32_t>(in[j]);
}
hipError_t launch_widen_u32(const LaunchEnv &env, uint64_t n, const uint32_t *in_dev, uint64_t *out_dev)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(widen_u32_kernel, dim3(stream_grid(env, n)), dim3(kStreamThreads), 0, env.stream, n, in_dev, out_dev);
    return hipGetLastError();
}
hipError_t launch_narrow_u32(const LaunchEnv &env, uint64_t n, const uint64_t *in_dev, uint32_t *out_dev)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(narrow_u32_kernel, dim3(stream_grid(env, n)), dim3(kStreamThreads), 0, env.stream, n, in_dev, out_dev);
    return hipGetLastError();
}

// out = (in + add - minus) & mask.  L = 2: one 16-B element per lane-iteration.
__global__ __launch_bounds__(kStreamThreads) void combine_wide_kernel(uint64_t n, const uint64_t *in, int in_limbs,
                                                                      const uint64_t *add, const uint64_t *minus,
                                                                      uint64_t *out, uint64_t mask_lo, uint64_t mask_hi)
{
    const u128 mask = (static_cast<u128>(mask_hi) << 64) | mask_lo;
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x; j < n;
         j += static_cast<uint64_t>(gridDim.x) * kStreamThreads) {
        u128 v = in_limbs == 2 ? ld128_nt(in + 2 * j) : static_cast<u128>(__builtin_nontemporal_load(in + j));
        if (add) v += ld128_nt(add + 2 * j);
        if (minus) v -= ld128_nt(minus + 2 * j);
        st128_nt(out + 2 * j, v & mask);
    }
}

__global__ __launch_bounds__(kStreamThreads) void combine_small_kernel(uint64_t n, const uint64_t *in, const uint64_t *add,
                                                                       const uint64_t *minus, uint64_t *out, uint64_t mask)
{
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x; j < n;
         j += static_cast<uint64_t>(gridDim.x) * kStreamThreads) {
        uint64_t v = in[j];
        if (add) v += add[j];
        if (minus) v -= minus[j];
        out[j] = v & mask;
    }
}

// Several combines of equal length in one launch (the online encrypts of the clients a process hosts when their masks were
// precomputed: a hundred LeNet-sized vectors are launch-bound one by one).  blockIdx.y = vector.
constexpr int kMaxCombine = 64;
struct CombineTable {
    const uint64_t *in[kMaxCombine], *add[kMaxCombine], *minus[kMaxCombine];
    uint64_t *out[kMaxCombine];
};

template <bool WIDE>
__global__ __launch_bounds__(kStreamThreads) void combine_batch_kernel(uint64_t n, const CombineTable tb, int in_limbs, uint64_t mask_lo, uint64_t mask_hi)
{
    const int v = blockIdx.y;
    const uint64_t *in = tb.in[v], *add = tb.add[v], *minus = tb.minus[v];
    uint64_t *out = tb.out[v];
    const u128 mask = (static_cast<u128>(mask_hi) << 64) | mask_lo;
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x; j < n;
         j += static_cast<uint64_t>(gridDim.x) * kStreamThreads) {
        if (WIDE) {
            u128 x = in_limbs == 2 ? ld128_nt(in + 2 * j) : static_cast<u128>(__builtin_nontemporal_load(in + j));
            if (add) x += ld128_nt(add + 2 * j);
            if (minus) x -= ld128_nt(minus + 2 * j);
            st128_nt(out + 2 * j, x & mask);
        } else {
            uint64_t x = in[j];
            if (add) x += add[j];
            if (minus) x -= minus[j];
            out[j] = x & mask_lo;
        }
    }
}

hipError_t launch_combine_batch(const LaunchEnv &env, uint64_t n, int n_vec, const uint64_t *const *in_dev, int in_limbs,
                                const uint64_t *const *add_dev, const uint64_t *const *minus_dev, uint64_t *const *out_dev)
{
    if (n == 0 || n_vec == 0) return hipSuccess;
    uint64_t lo, hi;
    masks_of(env.b, &lo, &hi);
    for (int v0 = 0; v0 < n_vec; v0 += kMaxCombine) {
        const int nv = std::min(kMaxCombine, n_vec - v0);
        CombineTable tb{};
        for (int v = 0; v < nv; v++) {
            tb.in[v] = in_dev[v0 + v]; tb.add[v] = add_dev ? add_dev[v0 + v] : nullptr;
            tb.minus[v] = minus_dev ? minus_dev[v0 + v] : nullptr; tb.out[v] = out_dev[v0 + v];
        }
        // enough blocks per vector to fill the chip together, at most 8 x 256 threads per CU in all
        uint64_t bx = (n + kStreamThreads - 1) / kStreamThreads;
        const uint64_t cap = std::max<uint64_t>(1, static_cast<uint64_t>(env.num_cus) * 8 / nv);
        if (bx > cap) bx = cap;
        const dim3 grid(static_cast<unsigned>(bx), static_cast<unsigned>(nv));
        if (env.b > 64) hipLaunchKernelGGL(combine_batch_kernel<true>, grid, dim3(kStreamThreads), 0, env.stream, n, tb, in_limbs, lo, hi);
        else hipLaunchKernelGGL(combine_batch_kernel<false>, grid, dim3(kStreamThreads), 0, env.stream, n, tb, in_limbs, lo, hi);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// The same combines AND the sum of their results in one pass (round 5): out[v] = in[v] + add[v] - minus[v], sum_out = sum_v out[v]
// (mod 2^b) -- the online encrypts of the clients a process hosts with precomputed masks plus the arbiter's reduce of what they wrote
// (jzf_flashe.py:480-481 x C, then jzf_aggregator.py:424-430): every ciphertext passes through the registers of the lane that owns
// the element, so the reduce costs one more store instead of a second launch that reads all C ciphertexts back (config 3: 100 LeNet-
// sized vectors, 0.046 + 0.030 ms as two launches).  A lane walks the vectors of its element in steps of kSumStep with all of a step's
// loads in flight; more than kMaxCombine vectors take several launches that carry the running sum (accumulate).
// A workgroup owns 64 consecutive elements; its four waves split the vectors among them (wave g takes v = g, g + 4, ...: a hundred
// LeNet-sized vectors are only 61,706 elements -- one lane per element would leave the chip a single wave per SIMD deep in memory latency)
// and add their partial sums up through the LDS.
constexpr int kSumStep = 8, kSumWaves = kStreamThreads / 64;
// Round 6: batches without a minus operand (the online encrypts of the double mask carry ONE precomputed difference per client) take a
// three-pointer table of kMaxCombine3 entries -- config 3's hundred clients are ONE launch instead of two that hand the running sum
// over through memory -- and the last launch of a batch may also DECRYPT the sum it has just completed with precomputed masks
// (dec_out = sum + dec_add - dec_minus: jzf_flashe.py:557-571 on the arbiter's reduce, the lane that owns the element holds it).
constexpr int kMaxCombine3 = 120;        // 3 x 120 pointers + the scalars stay inside the 4 KiB of kernel arguments
struct CombineTable3 {
    const uint64_t *in[kMaxCombine3], *add[kMaxCombine3];
    uint64_t *out[kMaxCombine3];
};
__device__ __forceinline__ const uint64_t *minus_of(const CombineTable &tb, int v) { return tb.minus[v]; }
__device__ __forceinline__ const uint64_t *minus_of(const CombineTable3 &, int) { return nullptr; }
struct SumDecrypt { const uint64_t *add, *minus; uint64_t *out; };       // all null: no decrypt in this launch

template <bool WIDE, class TB>
__global__ __launch_bounds__(kStreamThreads) void combine_batch_sum_kernel(uint64_t n, int n_vec, const TB tb, int in_limbs, bool accumulate, uint64_t *sum_out,
                                                                           const SumDecrypt dec, uint64_t mask_lo, uint64_t mask_hi)
{
    __shared__ unsigned long long part[kSumWaves][64][2];
    const u128 mask = (static_cast<u128>(mask_hi) << 64) | mask_lo;
    // (the wave index as a scalar: the pointer table is indexed with it -- from a VGPR index the kernel-argument table would be copied to scratch)
    const int g = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), e = threadIdx.x & 63;
    const uint64_t n_tiles = (n + 63) / 64;
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint64_t j = t * 64 + e;
        const bool live = j < n;
        const uint64_t jc = live ? j : n - 1;                         // (lanes beyond the vector re-read its last element and store nothing)
        // the decrypt masks of the element, requested before the batch is walked (the first wave finishes the element)
        u128 da = 0, dm = 0;
        if (g == 0 && dec.out) {
            if (WIDE) { da = dec.add ? ld128_nt(dec.add + 2 * jc) : 0; dm = dec.minus ? ld128_nt(dec.minus + 2 * jc) : 0; }
            else { da = dec.add ? __builtin_nontemporal_load(dec.add + jc) : 0; dm = dec.minus ? __builtin_nontemporal_load(dec.minus + jc) : 0; }
        }
        u128 sum = 0;
        for (int v0 = g; v0 < n_vec; v0 += kSumWaves * kSumStep) {
            u128 x[kSumStep], a[kSumStep], m[kSumStep];
#pragma unroll
            for (int u = 0; u < kSumStep; u++) {
                const int vv = v0 + kSumWaves * u, v = vv < n_vec ? vv : v0;              // (surplus slots of the last step re-read a vector and are dropped)
                const uint64_t *mv = minus_of(tb, v);
                if (WIDE) {
                    x[u] = in_limbs == 2 ? ld128_nt(tb.in[v] + 2 * jc) : static_cast<u128>(__builtin_nontemporal_load(tb.in[v] + jc));
                    a[u] = tb.add[v] ? ld128_nt(tb.add[v] + 2 * jc) : 0;
                    m[u] = mv ? ld128_nt(mv + 2 * jc) : 0;
                } else {
                    x[u] = __builtin_nontemporal_load(tb.in[v] + jc);
                    a[u] = tb.add[v] ? __builtin_nontemporal_load(tb.add[v] + jc) : 0;
                    m[u] = mv ? __builtin_nontemporal_load(mv + jc) : 0;
                }
            }
#pragma unroll
            for (int u = 0; u < kSumStep; u++) {
                const int vv = v0 + kSumWaves * u;
                if (vv >= n_vec) continue;
                const u128 r = (x[u] + a[u] - m[u]) & mask;
                if (live) {
                    if (WIDE) st128_nt(tb.out[vv] + 2 * j, r);
                    else __builtin_nontemporal_store(static_cast<uint64_t>(r), tb.out[vv] + j);
                }
                sum += r;
            }
        }
        part[g][e][0] = static_cast<unsigned long long>(sum); part[g][e][1] = static_cast<unsigned long long>(sum >> 64);
        __syncthreads();
        if (g == 0 && live) {
            u128 tot = 0;
            if (accumulate) tot = WIDE ? ld128(sum_out + 2 * j) : static_cast<u128>(sum_out[j]);
#pragma unroll
            for (int w = 0; w < kSumWaves; w++) tot += (static_cast<u128>(part[w][e][1]) << 64) | part[w][e][0];
            tot &= mask;
            if (WIDE) st128_nt(sum_out + 2 * j, tot);
            else sum_out[j] = static_cast<uint64_t>(tot);
            if (dec.out) {
                const u128 d = (tot + da - dm) & mask;
                if (WIDE) st128_nt(dec.out + 2 * j, d);
                else __builtin_nontemporal_store(static_cast<uint64_t>(d), dec.out + j);
            }
        }
        __syncthreads();
    }
}

// dec_out_dev (may be null): the decrypt of the completed sum with precomputed masks, written by the LAST launch of the batch
hipError_t launch_combine_batch_sum(const LaunchEnv &env, uint64_t n, int n_vec, const uint64_t *const *in_dev, int in_limbs,
                                    const uint64_t *const *add_dev, const uint64_t *const *minus_dev, uint64_t *const *out_dev, uint64_t *sum_out_dev,
                                    const uint64_t *dec_add_dev, const uint64_t *dec_minus_dev, uint64_t *dec_out_dev)
{
    if (n == 0) return hipSuccess;
    uint64_t lo, hi;
    masks_of(env.b, &lo, &hi);
    const SumDecrypt dec_all{dec_add_dev, dec_minus_dev, dec_out_dev}, dec_none{nullptr, nullptr, nullptr};
    if (n_vec == 0) {
        hipError_t e = hipMemsetAsync(sum_out_dev, 0, static_cast<size_t>(n) * (env.b > 64 ? 16 : 8), env.stream);
        if (e == hipSuccess && dec_out_dev) e = launch_combine(env, n, sum_out_dev, env.b > 64 ? 2 : 1, dec_add_dev, dec_minus_dev, dec_out_dev);
        return e;
    }
    bool any_minus = false;
    for (int v = 0; v < n_vec && minus_dev; v++) any_minus = any_minus || minus_dev[v] != nullptr;
    const uint64_t tiles = (n + 63) / 64, cap = static_cast<uint64_t>(env.num_cus) * 8;
    const dim3 grid(static_cast<unsigned>(tiles < cap ? tiles : cap));
    const int per = any_minus ? kMaxCombine : kMaxCombine3;
    for (int v0 = 0; v0 < n_vec; v0 += per) {
        const int nv = std::min(per, n_vec - v0);
        const SumDecrypt &dec = v0 + nv == n_vec ? dec_all : dec_none;
        if (any_minus) {
            CombineTable tb{};
            for (int v = 0; v < nv; v++) {
                tb.in[v] = in_dev[v0 + v]; tb.add[v] = add_dev ? add_dev[v0 + v] : nullptr;
                tb.minus[v] = minus_dev[v0 + v]; tb.out[v] = out_dev[v0 + v];
            }
            if (env.b > 64) hipLaunchKernelGGL((combine_batch_sum_kernel<true, CombineTable>), grid, dim3(kStreamThreads), 0, env.stream, n, nv, tb, in_limbs, v0 != 0, sum_out_dev, dec, lo, hi);
            else hipLaunchKernelGGL((combine_batch_sum_kernel<false, CombineTable>), grid, dim3(kStreamThreads), 0, env.stream, n, nv, tb, in_limbs, v0 != 0, sum_out_dev, dec, lo, hi);
        } else {
            CombineTable3 tb{};
            for (int v = 0; v < nv; v++) { tb.in[v] = in_dev[v0 + v]; tb.add[v] = add_dev ? add_dev[v0 + v] : nullptr; tb.out[v] = out_dev[v0 + v]; }
            if (env.b > 64) hipLaunchKernelGGL((combine_batch_sum_kernel<true, CombineTable3>), grid, dim3(kStreamThreads), 0, env.stream, n, nv, tb, in_limbs, v0 != 0, sum_out_dev, dec, lo, hi);
            else hipLaunchKernelGGL((combine_batch_sum_kernel<false, CombineTable3>), grid, dim3(kStreamThreads), 0, env.stream, n, nv, tb, in_limbs, v0 != 0, sum_out_dev, dec, lo, hi);
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_combine(const LaunchEnv &env, uint64_t n, const uint64_t *in_dev, int in_limbs,
                          const uint64_t *add_dev, const uint64_t *minus_dev, uint64_t *out_dev)
{
    if (n == 0) return hipSuccess;
    uint64_t lo, hi;
    masks_of(env.b, &lo, &hi);
    const int grid = stream_grid(env, n);
    if (env.b > 64)
        hipLaunchKernelGGL(combine_wide_kernel, dim3(grid), dim3(kStreamThreads), 0, env.stream, n, in_dev, in_limbs,
                           add_dev, minus_dev, out_dev, lo, hi);
    else
        hipLaunchKernelGGL(combine_small_kernel, dim3(grid), dim3(kStreamThreads), 0, env.stream, n, in_dev, add_dev,
                           minus_dev, out_dev, lo);
    return hipGetLastError();
}

// C-way element-wise mod-add.  WIDE: 128-bit elements (carry between the two limbs);
// otherwise each limb is its own element and a 16-B slot simply carries two of them.
template <bool WIDE>
__global__ __launch_bounds__(kStreamThreads) void aggregate_elem_kernel(int C, const PtrTable ops, uint64_t n_limbs,
                                                                        uint64_t *out, uint64_t mask_lo, uint64_t mask_hi)
{
    const uint64_t *const *tab = ops.p;
    const uint64_t n_slots = n_limbs / 2;
    for (uint64_t s = static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x; s < n_slots;
         s += static_cast<uint64_t>(gridDim.x) * kStreamThreads) {
        uint64_t a0 = 0, a1 = 0;
        u128 acc = 0;
#pragma unroll 4
        for (int c = 0; c < C; c++) {
            // every operand byte is read exactly once: stream past the caches
            const u64x2 v = __builtin_nontemporal_load(reinterpret_cast<const u64x2 *>(tab[c] + 2 * s));
            if (WIDE) acc += (static_cast<u128>(v[1]) << 64) | v[0];
            else { a0 += v[0]; a1 += v[1]; }
        }
        if (WIDE) { a0 = static_cast<uint64_t>(acc); a1 = static_cast<uint64_t>(acc >> 64); }
        u64x2 r;
        r[0] = a0 & mask_lo; r[1] = a1 & (WIDE ? mask_hi : mask_lo);
        __builtin_nontemporal_store(r, reinterpret_cast<u64x2 *>(out + 2 * s));
    }
    if (!WIDE && (n_limbs & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        uint64_t a = 0;
        for (int c = 0; c < C; c++) a += tab[c][n_limbs - 1];
        out[n_limbs - 1] = a & mask_lo;
    }
}

// one-limb vectors whose operands are only 8-byte aligned (a sub-range that starts at an odd element): one element per lane
__global__ __launch_bounds__(kStreamThreads) void aggregate_elem8_kernel(int C, const PtrTable ops, uint64_t n, uint64_t *out, uint64_t mask_lo)
{
    const uint64_t *const *tab = ops.p;
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x; j < n; j += static_cast<uint64_t>(gridDim.x) * kStreamThreads) {
        uint64_t a = 0;
#pragma unroll 4
        for (int c = 0; c < C; c++) a += __builtin_nontemporal_load(tab[c] + j);
        __builtin_nontemporal_store(a & mask_lo, out + j);
    }
}

// two-limb vectors with an operand that is only 8-byte aligned: one element per lane, its limbs in two 8-byte loads (out is 16-byte aligned)
__global__ __launch_bounds__(kStreamThreads) void aggregate_elem8_wide_kernel(int C, const PtrTable ops, uint64_t n, uint64_t *out, uint64_t mask_lo,
                                                                              uint64_t mask_hi)
{
    const uint64_t *const *tab = ops.p;
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x; j < n; j += static_cast<uint64_t>(gridDim.x) * kStreamThreads) {
        u128 acc = 0;
#pragma unroll 4
        for (int c = 0; c < C; c++) {
            const uint64_t lo = __builtin_nontemporal_load(tab[c] + 2 * j), hi = __builtin_nontemporal_load(tab[c] + 2 * j + 1);
            acc += (static_cast<u128>(hi) << 64) | lo;
        }
        u64x2 r;
        r[0] = static_cast<uint64_t>(acc) & mask_lo; r[1] = static_cast<uint64_t>(acc >> 64) & mask_hi;
        __builtin_nontemporal_store(r, reinterpret_cast<u64x2 *>(out + 2 * j));
    }
}

// compact layout (int_bits <= 32, uint32 elements): four elements per lane in 16-byte accesses; 32-bit sums wrap mod 2^32, which 2^b divides
template <bool VEC>
__global__ __launch_bounds__(kStreamThreads) void aggregate_elem_u32_kernel(int C, const PtrTable ops, uint64_t n, uint32_t *out, uint32_t mask)
{
    const uint64_t *const *tab = ops.p;
    if (VEC) {
        const uint64_t n4 = n / 4;
        for (uint64_t s = static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x; s < n4; s += static_cast<uint64_t>(gridDim.x) * kStreamThreads) {
            uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
#pragma unroll 4
            for (int c = 0; c < C; c++) {
                const u64x2 v = __builtin_nontemporal_load(reinterpret_cast<const u64x2 *>(tab[c]) + s);
                a0 += static_cast<uint32_t>(v[0]); a1 += static_cast<uint32_t>(v[0] >> 32);
                a2 += static_cast<uint32_t>(v[1]); a3 += static_cast<uint32_t>(v[1] >> 32);
            }
            u64x2 r;
            r[0] = (a0 & mask) | (static_cast<uint64_t>(a1 & mask) << 32);
            r[1] = (a2 & mask) | (static_cast<uint64_t>(a3 & mask) << 32);
            __builtin_nontemporal_store(r, reinterpret_cast<u64x2 *>(out) + s);
        }
        if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
            const uint64_t j = n4 * 4 + threadIdx.x;
            uint32_t a = 0;
            for (int c = 0; c < C; c++) a += reinterpret_cast<const uint32_t *>(tab[c])[j];
            out[j] = a & mask;
        }
    } else {
        for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x; j < n; j += static_cast<uint64_t>(gridDim.x) * kStreamThreads) {
            uint32_t a = 0;
#pragma unroll 4
            for (int c = 0; c < C; c++) a += __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(tab[c]) + j);
            __builtin_nontemporal_store(a & mask, out + j);
        }
    }
}

static inline PtrTable make_table(int C, const uint64_t *const *ops)
{
    PtrTable t;
    for (int c = 0; c < kMaxOps; c++) t.p[c] = c < C ? ops[c] : nullptr;
    return t;
}

hipError_t launch_aggregate_elem_u32(const LaunchEnv &env, int C, const uint32_t *const *ops, uint64_t n, uint32_t *out_dev)
{
    if (n == 0) return hipSuccess;
    if (C > kMaxOps || env.b > 32) return hipErrorInvalidValue;
    const PtrTable tab_dev = make_table(C, reinterpret_cast<const uint64_t *const *>(ops));
    const uint32_t mask = env.b == 32 ? 0xffffffffu : ((1u << env.b) - 1u);
    bool a16 = (reinterpret_cast<uintptr_t>(out_dev) & 15u) == 0;
    for (int c = 0; c < C; c++) a16 = a16 && (reinterpret_cast<uintptr_t>(ops[c]) & 15u) == 0;
    const int bpc = C >= 3 ? 2 : 8;
    int grid = stream_grid(env, a16 ? n / 4 + 1 : n);
    if (grid > env.num_cus * bpc) grid = env.num_cus * bpc;
    if (a16) hipLaunchKernelGGL(aggregate_elem_u32_kernel<true>, dim3(grid), dim3(kStreamThreads), 0, env.stream, C, tab_dev, n, out_dev, mask);
    else hipLaunchKernelGGL(aggregate_elem_u32_kernel<false>, dim3(grid), dim3(kStreamThreads), 0, env.stream, C, tab_dev, n, out_dev, mask);
    return hipGetLastError();
}

hipError_t launch_aggregate_elem(const LaunchEnv &env, int C, const uint64_t *const *ops, uint64_t n, uint64_t *out_dev)
{
    if (n == 0) return hipSuccess;
    if (C > kMaxOps) return hipErrorInvalidValue;
    const PtrTable tab_dev = make_table(C, ops);
    uint64_t lo, hi;
    masks_of(env.b, &lo, &hi);
    const uint64_t n_limbs = env.b > 64 ? 2 * n : n;
    bool a16 = (reinterpret_cast<uintptr_t>(out_dev) & 15u) == 0;
    for (int c = 0; c < C; c++) a16 = a16 && (reinterpret_cast<uintptr_t>(ops[c]) & 15u) == 0;
    if (!a16) {
        if (env.b > 64) {
            if (reinterpret_cast<uintptr_t>(out_dev) & 15u) return hipErrorInvalidValue;
            hipLaunchKernelGGL(aggregate_elem8_wide_kernel, dim3(stream_grid(env, n)), dim3(kStreamThreads), 0, env.stream, C, tab_dev, n, out_dev, lo, hi);
            return hipGetLastError();
        }
        hipLaunchKernelGGL(aggregate_elem8_kernel, dim3(stream_grid(env, n)), dim3(kStreamThreads), 0, env.stream, C, tab_dev, n, out_dev, lo);
        return hipGetLastError();
    }
    // a lane has C 16-byte loads in flight per slot: with many operands FEWER resident waves stream faster (measured at
    // C = 10, n = 1e7: 8 / 4 / 2 / 1 blocks per CU -> 5.5 / 5.9 / 6.0 / 4.4 TB/s; two operands want 4-8)
    const int bpc = C >= 3 ? 2 : 8;
    int grid = stream_grid(env, n_limbs / 2 + 1);
    if (grid > env.num_cus * bpc) grid = env.num_cus * bpc;
    if (env.b > 64)
        hipLaunchKernelGGL(aggregate_elem_kernel<true>, dim3(grid), dim3(kStreamThreads), 0, env.stream, C, tab_dev, n_limbs,
                           out_dev, lo, hi);
    else
        hipLaunchKernelGGL(aggregate_elem_kernel<false>, dim3(grid), dim3(kStreamThreads), 0, env.stream, C, tab_dev, n_limbs,
                           out_dev, lo, hi);
    return hipGetLastError();
}

// ---- the combine pass of a CUT cohort launch (cohort_cut.h; launch_prf_cohort_cut / launch_small_cohort_cut, kernels.hip) ----
// sum[k] = sum_p psum[p n + k] mod 2^b and, where the launch keeps a decrypt mask, dmask[k] = sum_p pmask[p n + k] mod 2^b: the pieces' sums
// add up and their masks telescope to what the uncut launch writes.  Two-limb elements, one per lane and trip in 16-byte accesses; the
// scratch is read once (non-temporal loads), the results are read again by the next pass (plain stores).  parts <= 16.
__global__ __launch_bounds__(kStreamThreads) void cohort_cut_combine_kernel(int parts, uint64_t n, const uint64_t *__restrict__ psum, uint64_t *__restrict__ sum,
                                                                            const uint64_t *__restrict__ pmask, uint64_t *__restrict__ dmask,
                                                                            uint64_t mask_lo, uint64_t mask_hi)
{
    const u128 mask = (static_cast<u128>(mask_hi) << 64) | mask_lo;
    for (uint64_t k = static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x; k < n; k += static_cast<uint64_t>(gridDim.x) * kStreamThreads) {
        u128 acc = 0, macc = 0;
#pragma unroll 4
        for (int p = 0; p < parts; p++) acc += ld128_nt(psum + 2 * (static_cast<uint64_t>(p) * n + k));
        if (pmask != nullptr) {
#pragma unroll 4
            for (int p = 0; p < parts; p++) macc += ld128_nt(pmask + 2 * (static_cast<uint64_t>(p) * n + k));
        }
        st128(sum + 2 * k, acc & mask);
        if (pmask != nullptr) st128(dmask + 2 * k, macc & mask);
    }
}

// the compact layout's form: uint32 sums masked to b bits, no mask.  VEC: n is a multiple of four and every pointer 16-byte aligned, so
// every piece's block is too -- four elements per lane in 16-byte accesses; otherwise one element per lane.
template <bool VEC>
__global__ __launch_bounds__(kStreamThreads) void cohort_cut_combine_u32_kernel(int parts, uint64_t n, const uint32_t *__restrict__ psum, uint32_t *__restrict__ sum,
                                                                                uint32_t mask)
{
    if (VEC) {
        const uint64_t n4 = n / 4;
        for (uint64_t s = static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x; s < n4; s += static_cast<uint64_t>(gridDim.x) * kStreamThreads) {
            uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
#pragma unroll 4
            for (int p = 0; p < parts; p++) {
                const u64x2 v = __builtin_nontemporal_load(reinterpret_cast<const u64x2 *>(psum + static_cast<uint64_t>(p) * n) + s);
                a0 += static_cast<uint32_t>(v[0]); a1 += static_cast<uint32_t>(v[0] >> 32);
                a2 += static_cast<uint32_t>(v[1]); a3 += static_cast<uint32_t>(v[1] >> 32);
            }
            u64x2 r;
            r[0] = (a0 & mask) | (static_cast<uint64_t>(a1 & mask) << 32);
            r[1] = (a2 & mask) | (static_cast<uint64_t>(a3 & mask) << 32);
            *(reinterpret_cast<u64x2 *>(sum) + s) = r;
        }
    } else {
        for (uint64_t k = static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x; k < n; k += static_cast<uint64_t>(gridDim.x) * kStreamThreads) {
            uint32_t a = 0;
#pragma unroll 4
            for (int p = 0; p < parts; p++) a += __builtin_nontemporal_load(psum + static_cast<uint64_t>(p) * n + k);
            sum[k] = a & mask;
        }
    }
}

hipError_t launch_cohort_cut_combine(const LaunchEnv &env, int parts, uint64_t n, const uint64_t *psum_dev, uint64_t *sum_dev, const uint64_t *pmask_dev,
                                     uint64_t *dmask_dev)
{
    if (n == 0) return hipSuccess;
    if (parts < 1 || env.b <= 64 || !psum_dev || !sum_dev || (pmask_dev && !dmask_dev)) return hipErrorInvalidValue;
    uint64_t lo, hi;
    masks_of(env.b, &lo, &hi);
    hipLaunchKernelGGL(cohort_cut_combine_kernel, dim3(stream_grid(env, n)), dim3(kStreamThreads), 0, env.stream, parts, n, psum_dev, sum_dev, pmask_dev,
                       dmask_dev, lo, hi);
    return hipGetLastError();
}

hipError_t launch_cohort_cut_combine_u32(const LaunchEnv &env, int parts, uint64_t n, const uint32_t *psum_dev, uint32_t *sum_dev)
{
    if (n == 0) return hipSuccess;
    if (parts < 1 || env.b > 32 || !psum_dev || !sum_dev) return hipErrorInvalidValue;
    const uint32_t mask = env.b == 32 ? 0xffffffffu : ((1u << env.b) - 1u);
    const bool vec = n % 4 == 0 && ((reinterpret_cast<uintptr_t>(psum_dev) | reinterpret_cast<uintptr_t>(sum_dev)) & 15u) == 0;
    if (vec) hipLaunchKernelGGL(cohort_cut_combine_u32_kernel<true>, dim3(stream_grid(env, n / 4)), dim3(kStreamThreads), 0, env.stream, parts, n, psum_dev, sum_dev, mask);
    else hipLaunchKernelGGL(cohort_cut_combine_u32_kernel<false>, dim3(stream_grid(env, n)), dim3(kStreamThreads), 0, env.stream, parts, n, psum_dev, sum_dev, mask);
    return hipGetLastError();
}

// ---- packed aggregate: C-way add of n_limbs-limb integers with full carry propagation ----
// Stage 1 (this kernel): per 16-B slot the C-way column sums (lo, hi = overflow count), the
// fold hi -> next limb, and a (generate, propagate) carry scan inside the 256-slot block via
// wave ballots + the integer-add trick; the block is resolved with carry-in 0 and publishes
// (G, P).  Stage 2 (packed_fixup_kernel): look-back over the block summaries and ripple the
// (rare) +1 into blocks whose carry-in is 1.
constexpr int kPackedThreads = 256;
uint64_t packed_num_blocks(uint64_t n_limbs) { return ((n_limbs + 1) / 2 + kPackedThreads - 1) / kPackedThreads; }

__device__ __forceinline__ void column_sums(int C, const PtrTable &ops, uint64_t slot, uint64_t n_limbs,
                                            uint64_t &lo0, uint64_t &hi0, uint64_t &lo1, uint64_t &hi1)
{
    const uint64_t *const *tab = ops.p;
    u128 a0 = 0, a1 = 0;
    const bool full = 2 * slot + 1 < n_limbs;
    if (full) {
#pragma unroll 4
        for (int c = 0; c < C; c++) {
            const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(tab[c] + 2 * slot);
            a0 += v.x; a1 += v.y;
        }
    } else {
        for (int c = 0; c < C; c++) a0 += tab[c][2 * slot];
    }
    lo0 = static_cast<uint64_t>(a0); hi0 = static_cast<uint64_t>(a0 >> 64);
    lo1 = static_cast<uint64_t>(a1); hi1 = static_cast<uint64_t>(a1 >> 64);
}

__global__ __launch_bounds__(kPackedThreads) void aggregate_packed_kernel(int C, const PtrTable tab, uint64_t n_limbs,
                                                                          uint64_t top_mask, uint64_t *out, uint32_t *summaries)
{
    __shared__ uint64_t sh_hi[kPackedThreads];
    __shared__ uint32_t sh_zc[kPackedThreads];
    __shared__ uint32_t sh_wg[kPackedThreads / 64], sh_wp[kPackedThreads / 64];
    const uint64_t n_slots = (n_limbs + 1) / 2;
    const uint64_t slot = static_cast<uint64_t>(blockIdx.x) * kPackedThreads + threadIdx.x;
    const bool live = slot < n_slots;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    uint64_t lo0 = 0, hi0 = 0, lo1 = 0, hi1 = 0;
    if (live) column_sums(C, tab, slot, n_limbs, lo0, hi0, lo1, hi1);
    // limb 2s+1: z1 = lo1 + hi0
    const uint64_t zl1 = lo1 + hi0;
    const uint32_t zc1 = zl1 < lo1;
    sh_hi[tid] = hi1;
    sh_zc[tid] = zc1;
    __syncthreads();
    uint64_t hi_prev = 0; uint32_t zc_prev = 0;
    if (tid > 0) { hi_prev = sh_hi[tid - 1]; zc_prev = sh_zc[tid - 1]; }
    else if (slot > 0 && live) {
        uint64_t pl0, ph0, pl1, ph1;
        column_sums(C, tab, slot - 1, n_limbs, pl0, ph0, pl1, ph1);
        const uint64_t pz = pl1 + ph0;
        hi_prev = ph1; zc_prev = pz < pl1;
    }
    // limb 2s: z0 = lo0 + hi_prev
    const uint64_t zl0 = lo0 + hi_prev;
    const uint32_t zc0 = zl0 < lo0;
    // X + Y with Y = z-carry of the previous limb
    const uint64_t s0 = zl0 + zc_prev;
    const uint32_t g0 = s0 < zl0, p0 = s0 == ~0ull;
    const uint64_t s1 = zl1 + zc0;
    const uint32_t g1 = s1 < zl1, p1 = s1 == ~0ull;
    const uint32_t Gt = live ? (g1 | (p1 & g0)) : 0u;
    const uint32_t Pt = live ? (p1 & p0) : 1u;      // dead lanes are transparent
    const uint64_t Gm = __ballot(Gt), Pm = __ballot(Pt);
    const uint64_t a = Gm | Pm, bb = Gm;
    const uint64_t sum0 = a + bb;
    if (lane == 0) { sh_wg[wave] = sum0 < a; sh_wp[wave] = Pm == ~0ull; }
    __syncthreads();
    uint32_t cin = 0;
    for (int v = 0; v < wave; v++) cin = sh_wg[v] | (sh_wp[v] & cin);
    const uint64_t cv = (a + bb + cin) ^ Pm;
    const uint32_t ct = (cv >> lane) & 1u;
    const uint64_t r0 = s0 + ct;
    const uint32_t k0 = g0 | (p0 & ct);
    const uint64_t r1 = s1 + k0;
    if (live) {
        const uint64_t i0 = 2 * slot, i1 = i0 + 1;
        if (i1 < n_limbs) {
            *reinterpret_cast<ulonglong2 *>(out + i0) =
                make_ulonglong2(r0, i1 == n_limbs - 1 ? (r1 & top_mask) : r1);
        } else {
            out[i0] = r0 & top_mask;
        }
    }
    if (tid == 0) {
        uint32_t c = 0, pall = 1;
        for (int v = 0; v < kPackedThreads / 64; v++) { c = sh_wg[v] | (sh_wp[v] & c); pall &= sh_wp[v]; }
        summaries[blockIdx.x] = c | (pall << 1);
    }
}

__global__ void packed_fixup_kernel(uint64_t n_blocks, uint64_t n_limbs, uint64_t top_mask, const uint32_t *summaries, uint64_t *out)
{
    const uint64_t B = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x + 1;
    if (B >= n_blocks) return;
    uint32_t cin = 0;
    for (uint64_t v = B; v-- > 0;) {
        const uint32_t s = summaries[v];
        if (s & 1u) { cin = 1; break; }
        if (!(s & 2u)) break;
    }
    if (!cin) return;
    const uint64_t first = B * kPackedThreads * 2;
    uint64_t last = first + kPackedThreads * 2;
    if (last > n_limbs) last = n_limbs;
    for (uint64_t i = first; i < last; i++) {
        uint64_t v = out[i] + 1;
        if (i == n_limbs - 1) v &= top_mask;
        out[i] = v;
        if (v != 0) break;
    }
}

hipError_t launch_aggregate_packed(const LaunchEnv &env, int C, const uint64_t *const *ops, uint64_t n_limbs,
                                   uint64_t total_bits, uint64_t *out_dev, uint32_t *summaries_dev)
{
    if (n_limbs == 0) return hipSuccess;
    if (C > kMaxOps) return hipErrorInvalidValue;
    const PtrTable tab_dev = make_table(C, ops);
    const unsigned top = static_cast<unsigned>(total_bits % 64);
    const uint64_t top_mask = top ? ((1ull << top) - 1) : ~0ull;
    const uint64_t nb = packed_num_blocks(n_limbs);
    hipLaunchKernelGGL(aggregate_packed_kernel, dim3(static_cast<unsigned>(nb)), dim3(kPackedThreads), 0, env.stream, C, tab_dev,
                       n_limbs, top_mask, out_dev, summaries_dev);
    if (nb > 1) {
        const unsigned fb = static_cast<unsigned>((nb - 1 + 255) / 256);
        hipLaunchKernelGGL(packed_fixup_kernel, dim3(fb), dim3(256), 0, env.stream, nb, n_limbs, top_mask, summaries_dev, out_dev);
    }
    return hipGetLastError();
}

// ---- packed aggregate in the ELEMENT domain: unpack(sum_c pack(ct_c) mod 2^(n b)) with no packed vector ----
// Element j of n sits at bit (n - 1 - j) b of the packed integer (pack_kernel), so a carry leaves element j + 1 and enters element j.
// With M = 2^b - 1, S_j = sum_c (ct_c[j] & M) = h_j 2^b + s_j (h_j <= C - 1) and t_j = s_j + h_{j+1} the packed sum is a ONE-BIT
// carry chain over the elements as long as C <= 2^b: g_j = t_j > M, p_j = t_j == M, k_j = g_j | (p_j & k_{j+1}), out_j =
// (t_j + k_{j+1}) & M.  The same two stages as the packed kernels above: lane `tid` of block B owns rank e = 256 B + tid, element
// j = n - 1 - e (descending j, so the carry travels towards higher lanes and blocks and the ballot trick applies unchanged; a wave's
// reversed addresses still coalesce); h of rank e - 1 comes through LDS, the first lane recomputes its neighbour's column.
// Config 2 (n = 1e7, b = 128, C = 10): 0.317 ms = 5.6 TB/s against 0.938 ms for C packs + the packed reduce + the unpack; ten compact
// 25,557,032-element operands at b = 20: 0.220 ms = 5.1 TB/s against 1.425 ms (profiles/r31_packed_elems_reduce.log).
// LAYOUT 0: uint32 elements (b <= 32; one per lane: the form for vectors that are only 4-byte aligned), 1: one uint64 limb (b <= 64), 2: two limbs (b > 64; A16: every operand is 16-byte aligned).
template <int LAYOUT> struct ElemValue { typedef u128 type; };
template <> struct ElemValue<0> { typedef uint64_t type; };

template <int LAYOUT, bool A16>
__device__ __forceinline__ void elem_column(int C, const PtrTable &ops, uint64_t j, int b, typename ElemValue<LAYOUT>::type M,
                                            typename ElemValue<LAYOUT>::type &s, uint32_t &h)
{
    const uint64_t *const *tab = ops.p;
    if (LAYOUT == 0) {
        uint64_t acc = 0;
#pragma unroll 4
        for (int c = 0; c < C; c++) acc += __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(tab[c]) + j) & static_cast<uint32_t>(M);
        s = acc & static_cast<uint64_t>(M);
        h = static_cast<uint32_t>(acc >> b);
    } else if (LAYOUT == 1) {
        u128 acc = 0;
#pragma unroll 4
        for (int c = 0; c < C; c++) acc += __builtin_nontemporal_load(tab[c] + j) & static_cast<uint64_t>(M);
        s = acc & M;
        h = static_cast<uint32_t>(acc >> b);
    } else {
        // the sum of up to 64 operands below 2^b needs b + 6 bits: `ov` counts the overflows of the 128-bit adds, and at
        // 122 <= b < 128 the high part h straddles the accumulator's top bits and that count
        u128 acc = 0;
        uint32_t ov = 0;
#pragma unroll 4
        for (int c = 0; c < C; c++) {
            u128 v;
            if (A16) v = ld128_nt(tab[c] + 2 * j);
            else v = (static_cast<u128>(__builtin_nontemporal_load(tab[c] + 2 * j + 1)) << 64) | __builtin_nontemporal_load(tab[c] + 2 * j);
            v &= M;
            acc += v;
            ov += acc < v;
        }
        s = acc & M;
        h = b == 128 ? ov : static_cast<uint32_t>(static_cast<uint64_t>(acc >> b) | (static_cast<uint64_t>(ov) << (128 - b)));
    }
}

template <int LAYOUT, bool A16>
__global__ __launch_bounds__(kPackedThreads) void aggregate_packed_elems_kernel(int C, const PtrTable tab, uint64_t n, int b, uint64_t mask_lo,
                                                                                uint64_t mask_hi, void *out, uint32_t *summaries)
{
    typedef typename ElemValue<LAYOUT>::type V;
    __shared__ uint32_t sh_h[kPackedThreads];
    __shared__ uint32_t sh_wg[kPackedThreads / 64], sh_wp[kPackedThreads / 64];
    const V M = LAYOUT == 0 ? static_cast<V>(mask_lo) : static_cast<V>((static_cast<u128>(mask_hi) << 64) | mask_lo);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t e = static_cast<uint64_t>(blockIdx.x) * kPackedThreads + tid;
    const bool live = e < n;
    const uint64_t j = n - 1 - e;                   // (only used when live)

    V s = 0;
    uint32_t h = 0;
    if (live) elem_column<LAYOUT, A16>(C, tab, j, b, M, s, h);
    sh_h[tid] = h;
    __syncthreads();
    uint32_t h_in = 0;                              // h_{j+1}; h_n = 0
    if (tid > 0) h_in = sh_h[tid - 1];
    else if (e > 0 && live) { V ps; elem_column<LAYOUT, A16>(C, tab, j + 1, b, M, ps, h_in); }
    const V t = s + h_in;                           // <= 2 M: wraps only in the two-limb layout at b = 128
    const uint32_t g = live ? ((t < s) | (t > M)) : 0u;
    const V tm = t & M;
    const uint32_t p = live ? (tm == M) : 1u;       // dead lanes are transparent; g and p exclude each other (t - M - 1 < M)
    const uint64_t Gm = __ballot(g), Pm = __ballot(p);
    const uint64_t a = Gm | Pm, bb = Gm;
    const uint64_t sum0 = a + bb;
    if (lane == 0) { sh_wg[wave] = sum0 < a; sh_wp[wave] = Pm == ~0ull; }
    __syncthreads();
    uint32_t cin = 0;
    for (int v = 0; v < wave; v++) cin = sh_wg[v] | (sh_wp[v] & cin);
    const uint64_t cv = (a + bb + cin) ^ Pm;
    const V r = (tm + static_cast<V>((cv >> lane) & 1u)) & M;
    if (live) {
        if (LAYOUT == 0) static_cast<uint32_t *>(out)[j] = static_cast<uint32_t>(r);
        else if (LAYOUT == 1) static_cast<uint64_t *>(out)[j] = static_cast<uint64_t>(r);
        else st128(static_cast<uint64_t *>(out) + 2 * j, r);
    }
    if (tid == 0) {
        uint32_t c = 0, pall = 1;
        for (int v = 0; v < kPackedThreads / 64; v++) { c = sh_wg[v] | (sh_wp[v] & c); pall &= sh_wp[v]; }
        summaries[blockIdx.x] = c | (pall << 1);
    }
}

// The compact layout with every pointer 16-byte aligned: FOUR elements per lane in 16-byte accesses.  The vector is thought padded with
// zeros below element n - 1 up to n4 = a multiple of four elements (zeros under the least significant element carry nothing), so that
// a lane's group -- elements [4 m, 4 m + 4), group rank q = n4 / 4 - 1 - m -- is aligned in memory; only the group that holds element
// n - 1 can be partial.  Inside the lane the carry runs from element 4 m + 3 to 4 m; the lane's (G, P) is the composition of its four.
__device__ __forceinline__ void elem_column_u32x4(int C, const PtrTable &ops, uint64_t m, uint64_t n, uint32_t M, uint64_t (&a)[4])
{
    const uint64_t *const *tab = ops.p;
    a[0] = a[1] = a[2] = a[3] = 0;
    if (4 * m + 3 < n) {
#pragma unroll 4
        for (int c = 0; c < C; c++) {
            const u64x2 v = __builtin_nontemporal_load(reinterpret_cast<const u64x2 *>(tab[c]) + m);
            a[0] += static_cast<uint32_t>(v[0]) & M; a[1] += static_cast<uint32_t>(v[0] >> 32) & M;
            a[2] += static_cast<uint32_t>(v[1]) & M; a[3] += static_cast<uint32_t>(v[1] >> 32) & M;
        }
    } else {
        for (int c = 0; c < C; c++)
            for (int i = 0; i < 4; i++)
                if (4 * m + i < n) a[i] += reinterpret_cast<const uint32_t *>(tab[c])[4 * m + i] & M;
    }
}

__global__ __launch_bounds__(kPackedThreads) void aggregate_packed_elems_u32x4_kernel(int C, const PtrTable tab, uint64_t n, int b, uint32_t M,
                                                                                      uint32_t *out, uint32_t *summaries)
{
    __shared__ uint32_t sh_h[kPackedThreads];
    __shared__ uint32_t sh_wg[kPackedThreads / 64], sh_wp[kPackedThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t groups = (n + 3) / 4;
    const uint64_t q = static_cast<uint64_t>(blockIdx.x) * kPackedThreads + tid;
    const bool live = q < groups;
    const uint64_t m = groups - 1 - q;              // (only used when live)

    uint64_t a[4] = {0, 0, 0, 0};
    if (live) elem_column_u32x4(C, tab, m, n, M, a);
    sh_h[tid] = static_cast<uint32_t>(a[0] >> b);
    __syncthreads();
    uint32_t h_in = 0;                              // h of element 4 m + 4, the next group's first; 0 under element n - 1
    if (tid > 0) h_in = sh_h[tid - 1];
    else if (q > 0 && live) {
        uint64_t acc = 0;
        for (int c = 0; c < C; c++) acc += reinterpret_cast<const uint32_t *>(tab.p[c])[4 * (m + 1)] & M;
        h_in = static_cast<uint32_t>(acc >> b);
    }
    uint32_t g[4], p[4], tm[4];
#pragma unroll
    for (int i = 3; i >= 0; i--) {
        const uint64_t t = (a[i] & M) + (i == 3 ? h_in : static_cast<uint32_t>(a[i + 1] >> b));
        g[i] = t > M; tm[i] = static_cast<uint32_t>(t) & M; p[i] = tm[i] == M;
    }
    const uint32_t Gt = live ? (g[0] | (p[0] & (g[1] | (p[1] & (g[2] | (p[2] & g[3])))))) : 0u;
    const uint32_t Pt = live ? (p[0] & p[1] & p[2] & p[3]) : 1u;
    const uint64_t Gm = __ballot(Gt), Pm = __ballot(Pt);
    const uint64_t aa = Gm | Pm, bb = Gm;
    const uint64_t sum0 = aa + bb;
    if (lane == 0) { sh_wg[wave] = sum0 < aa; sh_wp[wave] = Pm == ~0ull; }
    __syncthreads();
    uint32_t cin = 0;
    for (int v = 0; v < wave; v++) cin = sh_wg[v] | (sh_wp[v] & cin);
    const uint64_t cv = (aa + bb + cin) ^ Pm;
    uint32_t k = static_cast<uint32_t>(cv >> lane) & 1u, r[4];
#pragma unroll
    for (int i = 3; i >= 0; i--) { r[i] = (tm[i] + k) & M; k = g[i] | (p[i] & k); }
    if (live) {
        if (4 * m + 3 < n) {
            u64x2 w;
            w[0] = r[0] | (static_cast<uint64_t>(r[1]) << 32); w[1] = r[2] | (static_cast<uint64_t>(r[3]) << 32);
            *(reinterpret_cast<u64x2 *>(out) + m) = w;
        } else {
            for (int i = 0; i < 4; i++)
                if (4 * m + i < n) out[4 * m + i] = r[i];
        }
    }
    if (tid == 0) {
        uint32_t c = 0, pall = 1;
        for (int v = 0; v < kPackedThreads / 64; v++) { c = sh_wg[v] | (sh_wp[v] & c); pall &= sh_wp[v]; }
        summaries[blockIdx.x] = c | (pall << 1);
    }
}

// Stage 2: block B's carry-in by look-back over the summaries of the blocks below it; the rare +1 ripples through the elements equal to
// M (they become 0) and stops at the first that is not -- inside the block, whose own P says whether the carry leaves it.
// (tile: ranks per stage-1 block; n: the length rank 0 is counted from -- the vector kernel's padded length)
template <int LAYOUT>
__global__ void packed_elems_fixup_kernel(uint64_t n_blocks, uint64_t n, uint64_t tile, uint64_t mask_lo, uint64_t mask_hi, const uint32_t *summaries,
                                          void *out)
{
    const uint64_t B = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x + 1;
    if (B >= n_blocks) return;
    uint32_t cin = 0;
    for (uint64_t v = B; v-- > 0;) {
        const uint32_t s = summaries[v];
        if (s & 1u) { cin = 1; break; }
        if (!(s & 2u)) break;
    }
    if (!cin) return;
    const uint64_t first = B * tile;
    uint64_t last = first + tile;
    if (last > n) last = n;
    for (uint64_t e = first; e < last; e++) {
        const uint64_t j = n - 1 - e;
        bool zero;
        if (LAYOUT == 0) {
            uint32_t *q = static_cast<uint32_t *>(out) + j;
            const uint32_t v = (*q + 1u) & static_cast<uint32_t>(mask_lo);
            *q = v; zero = v == 0;
        } else if (LAYOUT == 1) {
            uint64_t *q = static_cast<uint64_t *>(out) + j;
            const uint64_t v = (*q + 1u) & mask_lo;
            *q = v; zero = v == 0;
        } else {
            uint64_t *q = static_cast<uint64_t *>(out) + 2 * j;
            const u128 v = (((static_cast<u128>(q[1]) << 64) | q[0]) + 1u) & ((static_cast<u128>(mask_hi) << 64) | mask_lo);
            st128(q, v); zero = v == 0;
        }
        if (!zero) break;
    }
}

uint64_t packed_elems_num_blocks(uint64_t n) { return (n + kPackedThreads - 1) / kPackedThreads; }

hipError_t launch_aggregate_packed_elems(const LaunchEnv &env, int C, const uint64_t *const *ops, uint64_t n, int elem_bytes, void *out_dev,
                                         uint32_t *summaries_dev)
{
    if (n == 0) return hipSuccess;
    if (C < 1 || C > kMaxOps || (elem_bytes == 4 ? env.b > 32 : elem_bytes != (env.b > 64 ? 16 : 8))) return hipErrorInvalidValue;
    if (env.b < 6 && C > (1 << env.b)) return hipErrorNotSupported;       // the carry between elements would need more than one bit
    const PtrTable tab_dev = make_table(C, ops);
    uint64_t lo, hi;
    masks_of(env.b, &lo, &hi);
    const uint64_t nb = packed_elems_num_blocks(n);
    if (nb > 0x7fffffffull) return hipErrorInvalidValue;
    const dim3 grid(static_cast<unsigned>(nb)), block(kPackedThreads), fgrid(static_cast<unsigned>((nb - 1 + 255) / 256));
    const uint64_t tile = kPackedThreads;
    if (elem_bytes == 4) {
        bool a16 = (reinterpret_cast<uintptr_t>(out_dev) & 15u) == 0;
        for (int c = 0; c < C; c++) a16 = a16 && (reinterpret_cast<uintptr_t>(ops[c]) & 15u) == 0;
        if (a16) {
            // four elements per lane: blocks of 4 x kPackedThreads ranks counted from the padded length
            const uint64_t n4 = (n + 3) / 4 * 4, nb4 = (n4 / 4 + kPackedThreads - 1) / kPackedThreads;
            hipLaunchKernelGGL(aggregate_packed_elems_u32x4_kernel, dim3(static_cast<unsigned>(nb4)), block, 0, env.stream, C, tab_dev, n, env.b,
                               static_cast<uint32_t>(lo), static_cast<uint32_t *>(out_dev), summaries_dev);
            if (nb4 > 1)
                hipLaunchKernelGGL(packed_elems_fixup_kernel<0>, dim3(static_cast<unsigned>((nb4 - 1 + 255) / 256)), dim3(256), 0, env.stream, nb4, n4,
                                   4 * tile, lo, hi, summaries_dev, out_dev);
            return hipGetLastError();
        }
        hipLaunchKernelGGL((aggregate_packed_elems_kernel<0, false>), grid, block, 0, env.stream, C, tab_dev, n, env.b, lo, hi, out_dev, summaries_dev);
        if (nb > 1) hipLaunchKernelGGL(packed_elems_fixup_kernel<0>, fgrid, dim3(256), 0, env.stream, nb, n, tile, lo, hi, summaries_dev, out_dev);
    } else if (elem_bytes == 8) {
        hipLaunchKernelGGL((aggregate_packed_elems_kernel<1, false>), grid, block, 0, env.stream, C, tab_dev, n, env.b, lo, hi, out_dev, summaries_dev);
        if (nb > 1) hipLaunchKernelGGL(packed_elems_fixup_kernel<1>, fgrid, dim3(256), 0, env.stream, nb, n, tile, lo, hi, summaries_dev, out_dev);
    } else {
        bool a16 = true;
        for (int c = 0; c < C; c++) a16 = a16 && (reinterpret_cast<uintptr_t>(ops[c]) & 15u) == 0;
        if (a16) hipLaunchKernelGGL((aggregate_packed_elems_kernel<2, true>), grid, block, 0, env.stream, C, tab_dev, n, env.b, lo, hi, out_dev, summaries_dev);
        else hipLaunchKernelGGL((aggregate_packed_elems_kernel<2, false>), grid, block, 0, env.stream, C, tab_dev, n, env.b, lo, hi, out_dev, summaries_dev);
        if (nb > 1) hipLaunchKernelGGL(packed_elems_fixup_kernel<2>, fgrid, dim3(256), 0, env.stream, nb, n, tile, lo, hi, summaries_dev, out_dev);
    }
    return hipGetLastError();
}

// ---- slice helpers for a packed reduce that is cut across GPUs (flashe_amd/dist.py run_packed) ----
// probe: x holds a slice sum as n_limbs - 1 body limbs plus one carry limb on top.
// info[0] = x[0], info[1] = 1 iff body limbs [1, n_limbs - 1) are all ~0, info[2] = x[n_limbs - 1].
__global__ __launch_bounds__(kStreamThreads) void packed_probe_kernel(uint64_t n_limbs, const uint64_t *x, uint64_t *info)
{
    bool ones = true;
    for (uint64_t i = 1 + static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x; i + 1 < n_limbs;
         i += static_cast<uint64_t>(gridDim.x) * kStreamThreads)
        ones &= __builtin_nontemporal_load(x + i) == ~0ull;
    if (!__all(ones) && (threadIdx.x & 63) == 0) info[1] = 0;     // every writer stores the same value
    if (blockIdx.x == 0 && threadIdx.x == 0) { info[0] = x[0]; info[2] = x[n_limbs - 1]; }
}
__global__ void packed_probe_init_kernel(uint64_t *info) { info[0] = 0; info[1] = 1; info[2] = 0; }

// x = (x + cin) mod 2^total_bits in place, one workgroup: the ripple stops at the first limb that is
// not all ones, which is limb 0 or 1 for anything but adversarial data.
constexpr int kRippleThreads = 1024;
// infos != null: the carry-in is derived on the device from the (low limb, body-all-ones, carry-out) triples of the limb
// slices below this one (ranks 0 .. n_below - 1 of a packed reduce cut across GPUs): a slice passes its carry-in on when all its
// body limbs are ones and the low limb overflows, on top of its own carry-out.
// stride: words from one slice's triple to the next more significant one's (3 = slice 0 first; -3 = the lowest slice's triple is the
// LAST of the gathered ones and infos points at it: slices numbered from the most significant end, as element slices of a packed
// vector are -- element 0 is the most significant, jzf_weights.py:59-62).
__global__ __launch_bounds__(kRippleThreads) void packed_add_carry_kernel(uint64_t n_limbs, uint64_t top_mask, uint64_t cin, uint64_t *x,
                                                                          const uint64_t *__restrict__ infos, int n_below, int stride)
{
    __shared__ int first_stop;
    const int tid = threadIdx.x;
    if (infos) {
        uint64_t carry = 0;
        for (int g = 0; g < n_below; g++) {
            const uint64_t *t = infos + static_cast<int64_t>(g) * stride;
            const uint64_t low = t[0], ones = t[1], cout = t[2];
            carry = cout + ((ones && low + carry < low) ? 1ull : 0ull);
        }
        cin = carry;
    }
    const uint64_t x0 = x[0];
    __syncthreads();
    const uint64_t s0 = x0 + cin;
    if (tid == 0) x[0] = s0;
    if (s0 < x0) {
        for (uint64_t base = 1; base < n_limbs; base += kRippleThreads) {
            const uint64_t i = base + tid;
            const uint64_t v = i < n_limbs ? x[i] : 0;
            if (tid == 0) first_stop = kRippleThreads;
            __syncthreads();
            if (v != ~0ull) atomicMin(&first_stop, tid);
            __syncthreads();
            const int f = first_stop;
            if (tid < f) x[i] = 0;
            else if (tid == f && i < n_limbs) x[i] = v + 1;
            __syncthreads();
            if (f < kRippleThreads) break;
        }
    }
    __syncthreads();
    if (tid == 0) x[n_limbs - 1] &= top_mask;
}

hipError_t launch_packed_probe(const LaunchEnv &env, uint64_t n_limbs, const uint64_t *x_dev, uint64_t *info_dev)
{
    hipLaunchKernelGGL(packed_probe_init_kernel, dim3(1), dim3(1), 0, env.stream, info_dev);
    if (n_limbs == 0) return hipGetLastError();
    hipLaunchKernelGGL(packed_probe_kernel, dim3(stream_grid(env, n_limbs)), dim3(kStreamThreads), 0, env.stream, n_limbs, x_dev, info_dev);
    return hipGetLastError();
}

hipError_t launch_packed_add_carry(const LaunchEnv &env, uint64_t n_limbs, uint64_t total_bits, uint64_t cin, uint64_t *x_dev)
{
    if (n_limbs == 0) return hipSuccess;
    const unsigned top = static_cast<unsigned>(total_bits % 64);
    const uint64_t top_mask = top ? ((1ull << top) - 1) : ~0ull;
    hipLaunchKernelGGL(packed_add_carry_kernel, dim3(1), dim3(kRippleThreads), 0, env.stream, n_limbs, top_mask, cin, x_dev,
                       static_cast<const uint64_t *>(nullptr), 0, 3);
    return hipGetLastError();
}

hipError_t launch_packed_resolve_carry(const LaunchEnv &env, uint64_t n_limbs, uint64_t total_bits, const uint64_t *infos_dev, int n_below,
                                       uint64_t *x_dev, int stride_words)
{
    if (n_limbs == 0) return hipSuccess;
    const unsigned top = static_cast<unsigned>(total_bits % 64);
    const uint64_t top_mask = top ? ((1ull << top) - 1) : ~0ull;
    hipLaunchKernelGGL(packed_add_carry_kernel, dim3(1), dim3(kRippleThreads), 0, env.stream, n_limbs, top_mask, 0ull, x_dev, infos_dev, n_below,
                       stride_words);
    return hipGetLastError();
}

// ---- bit-packing codec ----
// pack: one output limb per lane, gathering every element that overlaps bits [64w, 64w + 64).
__global__ __launch_bounds__(kStreamThreads) void pack_kernel(uint64_t n, int b, int L, const uint64_t *in, uint64_t *out,
                                                              uint64_t n_limbs, uint64_t mask_lo, uint64_t mask_hi)
{
    const u128 mask = (static_cast<u128>(mask_hi) << 64) | mask_lo;
    for (uint64_t w = static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x; w < n_limbs;
         w += static_cast<uint64_t>(gridDim.x) * kStreamThreads) {
        const uint64_t bit0 = 64 * w;
        uint64_t e = bit0 / b;
        uint64_t e_last = (bit0 + 63) / b;
        if (e_last >= n) e_last = n - 1;
        uint64_t acc = 0;
        for (; e <= e_last; e++) {
            const uint64_t j = n - 1 - e;
            const u128 v = (L == 2 ? ld128(in + 2 * j) : static_cast<u128>(in[j])) & mask;
            const uint64_t pos = e * b;
            if (pos >= bit0) acc |= static_cast<uint64_t>(v) << (pos - bit0);
            else acc |= static_cast<uint64_t>(v >> (bit0 - pos));
        }
        out[w] = acc;
    }
}

__global__ __launch_bounds__(kStreamThreads) void unpack_kernel(uint64_t n, int b, int L, const uint64_t *in, uint64_t *out,
                                                                uint64_t n_limbs, uint64_t mask_lo, uint64_t mask_hi)
{
    const u128 mask = (static_cast<u128>(mask_hi) << 64) | mask_lo;
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x; j < n;
         j += static_cast<uint64_t>(gridDim.x) * kStreamThreads) {
        const uint64_t pos = (n - 1 - j) * b;
        const uint64_t w = pos / 64;
        const unsigned s = static_cast<unsigned>(pos % 64);
        const u128 l0 = in[w];
        const u128 l1 = w + 1 < n_limbs ? in[w + 1] : 0;
        const u128 l2 = w + 2 < n_limbs ? in[w + 2] : 0;
        u128 v = l0 >> s;
        if (s) { v |= l1 << (64 - s); v |= l2 << (128 - s); }
        else v |= l1 << 64;
        v &= mask;
        if (L == 2) st128(out + 2 * j, v);
        else out[j] = static_cast<uint64_t>(v);
    }
}

// b = 128: the packed integer is the element order reversed (element 0 most significant) -- one 16-byte move per lane,
// the same kernel packs and unpacks.
__global__ __launch_bounds__(kStreamThreads) void reverse128_kernel(uint64_t n, const uint64_t *in, uint64_t *out)
{
    for (uint64_t e = static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x; e < n;
         e += static_cast<uint64_t>(gridDim.x) * kStreamThreads)
        st128_nt(out + 2 * e, ld128_nt(in + 2 * (n - 1 - e)));
}

hipError_t launch_pack(const LaunchEnv &env, uint64_t n, const uint64_t *in_dev, uint64_t *out_dev)
{
    if (n == 0) return hipSuccess;
    if (env.b == 128) {
        hipLaunchKernelGGL(reverse128_kernel, dim3(stream_grid(env, n)), dim3(kStreamThreads), 0, env.stream, n, in_dev, out_dev);
        return hipGetLastError();
    }
    uint64_t lo, hi;
    masks_of(env.b, &lo, &hi);
    const uint64_t n_limbs = (n * static_cast<uint64_t>(env.b) + 63) / 64;
    hipLaunchKernelGGL(pack_kernel, dim3(stream_grid(env, n_limbs)), dim3(kStreamThreads), 0, env.stream, n, env.b,
                       env.b > 64 ? 2 : 1, in_dev, out_dev, n_limbs, lo, hi);
    return hipGetLastError();
}

hipError_t launch_unpack(const LaunchEnv &env, uint64_t n, const uint64_t *in_dev, uint64_t *out_dev)
{
    if (n == 0) return hipSuccess;
    if (env.b == 128) {
        hipLaunchKernelGGL(reverse128_kernel, dim3(stream_grid(env, n)), dim3(kStreamThreads), 0, env.stream, n, in_dev, out_dev);
        return hipGetLastError();
    }
    uint64_t lo, hi;
    masks_of(env.b, &lo, &hi);
    const uint64_t n_limbs = (n * static_cast<uint64_t>(env.b) + 63) / 64;
    hipLaunchKernelGGL(unpack_kernel, dim3(stream_grid(env, n)), dim3(kStreamThreads), 0, env.stream, n, env.b,
                       env.b > 64 ? 2 : 1, in_dev, out_dev, n_limbs, lo, hi);
    return hipGetLastError();
}

// ---- sparse helpers ----
__global__ __launch_bounds__(kStreamThreads) void fill_kernel(uint64_t n, int L, uint64_t lo, uint64_t hi, uint64_t *out)
{
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x; j < n;
         j += static_cast<uint64_t>(gridDim.x) * kStreamThreads) {
        if (L == 2) *reinterpret_cast<ulonglong2 *>(out + 2 * j) = make_ulonglong2(lo, hi);
        else out[j] = lo;
    }
}

// out[loc[q]] = vals[q]  or  out[loc[q]] = (out[loc[q]] + vals[q]) mod 2^b.  loc must hold
// distinct positions within one launch (the reference's location lists are sets).
// sub (a constant, < 2^b) is subtracted from every value first: the sparse reduce adds vals[q] - zero.
__global__ __launch_bounds__(kStreamThreads) void scatter_kernel(uint64_t total, uint64_t k, int L, const uint32_t *loc, const uint64_t *vals,
                                                                 uint64_t *out, bool accumulate, uint64_t mask_lo, uint64_t mask_hi,
                                                                 uint64_t sub_lo, uint64_t sub_hi, uint32_t *err_flag)
{
    const u128 mask = (static_cast<u128>(mask_hi) << 64) | mask_lo;
    const u128 sub = (static_cast<u128>(sub_hi) << 64) | sub_lo;
    for (uint64_t q = static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x; q < k;
         q += static_cast<uint64_t>(gridDim.x) * kStreamThreads) {
        const uint64_t p = loc[q];
        if (p >= total) { *err_flag = 1; continue; }       // never write outside the dense vector: skip and report
        if (L == 2) {
            u128 v = ld128(vals + 2 * q) - sub;
            if (accumulate) v += ld128(out + 2 * p);
            st128(out + 2 * p, v & mask);
        } else {
            uint64_t v = vals[q] - sub_lo;
            if (accumulate) v += out[p];
            out[p] = v & mask_lo;
        }
    }
}

// Sparse reduce over SORTED location lists, two launches for any number of clients.
// The dense vector is cut into spans of kSpan positions, one workgroup each.  Kernel A: start[s][c] = first entry of
// client c at or beyond position s * kSpan -- one thread per ENTRY: entry q opens every span between the span of entry
// q - 1 and its own (most entries open none), one coalesced pass over the location lists instead of a binary search per
// (span, client); it also reports lists that are not strictly increasing or reach beyond the vector.  Kernel B: the
// workgroup (1,024 threads: the gathers are the slow part, measured against 256 / 512 threads and 1 K ... 8 K spans) clears a
// span-sized accumulator in LDS, adds every client's entries that fall into its span (128-bit add =
// two LDS atomics; the low one returns the old value, which tells the lane exactly whether ITS add wrapped -- integer
// adds commute, so the sum does not depend on the order), then writes src + accumulator (or src - accumulator, base
// instead of src when there is none) for the WHOLE span: the dense output is written exactly once, coalesced.
constexpr int kSpan = kSpanReduce;  // positions per span: 64 KiB of 128-bit accumulators, two workgroups per CU (8,192 = 128 KiB, one workgroup per CU,
                                    // twice as long slices per client: aggregate 0.171 against 0.169 ms, fused decrypt 0.442 against 0.420 -- config 5)
constexpr int kSpanThreads = 1024;
constexpr int kSpanBatch = 2;       // entries whose loads a lane keeps in flight at once (config 5, aggregate / fused decrypt: 8: 0.256 / 0.484 ms,
                                    // 4: 0.171 / 0.416, 2: 0.163 / 0.407, 1: 0.167 / 0.407 -- fewer gathers in flight stream faster here too)
struct ScatterTable {
    const uint32_t *loc[kMaxScatter];
    const uint64_t *vals[kMaxScatter];
    uint64_t k[kMaxScatter], sub_lo[kMaxScatter], sub_hi[kMaxScatter];
};

constexpr int kBoundsPerThread = 8;
// entry q of client c (prev = the entry before it, cur = itself; q == k closes the list) opens the spans of SPAN positions between them:
// start[span * C + c] = q (the transposed table, start[c][span], measured no faster: tests/perf/experiments/README.md)
template <int SPAN>
__device__ __forceinline__ void span_open(uint32_t *start, int C, int c, uint64_t q, bool live, uint64_t k, uint64_t prev, uint64_t cur, uint64_t total,
                                          uint32_t lane)
{
    const uint64_t n_spans = (total + SPAN - 1) / SPAN;
    const uint64_t row = static_cast<uint64_t>(c), step = static_cast<uint64_t>(C);
    const uint64_t s_last = q < k ? std::min<uint64_t>(static_cast<uint32_t>(cur) / static_cast<uint32_t>(SPAN), n_spans) : n_spans;
    const uint64_t s_first = !live ? s_last + 1 : q ? std::min<uint64_t>(static_cast<uint32_t>(prev) / static_cast<uint32_t>(SPAN), n_spans) + 1 : 0;
    const bool is_long = s_first + 16 <= s_last;
    if (!is_long)
        for (uint64_t sp = s_first; sp <= s_last; sp++) start[row + sp * step] = static_cast<uint32_t>(q);
    // a long run of empty spans (a short list over a long vector, an empty client): the wave fills it together instead of one
    // lane storing span after span
    uint64_t pending = __ballot(is_long);
    while (pending) {
        const int src = __ffsll(static_cast<unsigned long long>(pending)) - 1;
        const uint64_t a = __shfl(s_first, src, 64), b = __shfl(s_last, src, 64);
        const uint32_t qq = static_cast<uint32_t>(__shfl(q, src, 64));
        for (uint64_t x = a + lane; x <= b; x += 64u) start[row + x * step] = qq;
        pending &= pending - 1;
    }
}

// start_reduce / start_fused: the table at kSpanReduce / kSpanFused positions per span (either may be null): one pass over the lists
// serves the plain reduce and the passes with the PRF inside.  A thread takes kBoundsPerThread CONSECUTIVE entries: two 16-byte loads
// (VEC: every list 16-byte aligned) and the entry in front of them, instead of two 4-byte loads per entry.
template <bool VEC>
__global__ __launch_bounds__(kStreamThreads) void span_bounds_kernel(const ScatterTable tb, int C, uint64_t total, uint32_t *start_reduce, uint32_t *start_fused,
                                                                     uint32_t *err_flag)
{
    static_assert(kBoundsPerThread == 8, "two uint4 loads per thread");
    const int c = blockIdx.y;
    const uint64_t k = tb.k[c];
    const uint32_t *loc = tb.loc[c];
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t q0 = (static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x) * kBoundsPerThread;
    uint32_t v[kBoundsPerThread + 1];                    // v[0] = the entry in front of this thread's, v[1 + i] = entry q0 + i
    v[0] = q0 && q0 <= k ? loc[q0 - 1] : 0u;
    if (VEC && q0 + kBoundsPerThread <= k) {
        const uint4 a = *reinterpret_cast<const uint4 *>(loc + q0), b = *reinterpret_cast<const uint4 *>(loc + q0 + 4);
        v[1] = a.x; v[2] = a.y; v[3] = a.z; v[4] = a.w; v[5] = b.x; v[6] = b.y; v[7] = b.z; v[8] = b.w;
    } else {
#pragma unroll
        for (int i = 0; i < kBoundsPerThread; i++) v[1 + i] = q0 + i < k ? loc[q0 + i] : 0u;
    }
#pragma unroll
    for (int i = 0; i < kBoundsPerThread; i++) {
        const uint64_t q = q0 + i;
        // q == k closes the list (the spans behind the last entry); lanes beyond it open nothing
        const bool live = q <= k;
        const uint64_t prev = live && q ? v[i] : 0, cur = live && q < k ? v[1 + i] : 0;
        if (live && q < k && (cur >= total || (q && cur <= prev))) *err_flag = 1;
        if (start_reduce) span_open<kSpanReduce>(start_reduce, C, c, q, live, k, prev, cur, total, lane);
        if (start_fused) span_open<kSpanFused>(start_fused, C, c, q, live, k, prev, cur, total, lane);
    }
}

// One batch of a span's entries, gathered into registers: flat entry f belongs to the client c with prefix[c] <= f < prefix[c + 1].
struct SpanBatch { uint32_t r[kSpanBatch]; int own[kSpanBatch]; u128 v[kSpanBatch]; };

template <int THREADS>
__device__ __forceinline__ void span_gather(SpanBatch &g, uint32_t f0, uint32_t n_entries, const uint32_t *prefix, const uint32_t *begin,
                                            const uint32_t *const *s_loc, const uint64_t *const *s_vals, int L, uint32_t p0)
{
#pragma unroll
    for (int e = 0; e < kSpanBatch; e++) {
        const uint32_t fe = f0 + e * THREADS;
        const uint32_t f = fe < n_entries ? fe : f0;     // surplus slots re-read the first entry (f0 < n_entries) and are not added
        int c = 0;
#pragma unroll
        for (int step = 32; step; step >>= 1)
            if (prefix[c + step] <= f) c += step;
        g.own[e] = c;
        const uint64_t q = static_cast<uint64_t>(begin[c]) + (f - prefix[c]);
        g.r[e] = ld32_g(s_loc[c] + q) - p0;
        g.v[e] = L == 2 ? ld128_g(s_vals[c] + 2 * q) : static_cast<u128>(ld64_g(s_vals[c] + q));
    }
}

template <int THREADS>
__device__ __forceinline__ void span_add(const SpanBatch &g, uint32_t f0, uint32_t n_entries, unsigned long long *acc, const uint64_t *s_sub, int L,
                                         uint64_t span_len, uint32_t *err_flag)
{
#pragma unroll
    for (int e = 0; e < kSpanBatch; e++) {
        if (f0 + e * THREADS >= n_entries) break;
        if (g.r[e] >= span_len) { *err_flag = 1; continue; }      // position >= total, or a list that is not strictly increasing
        const u128 w = g.v[e] - ((static_cast<u128>(s_sub[2 * g.own[e] + 1]) << 64) | s_sub[2 * g.own[e]]);
        const unsigned long long wlo = static_cast<unsigned long long>(w), whi = static_cast<unsigned long long>(w >> 64);
        if (L == 2) {
            const unsigned long long old = atomicAdd(&acc[2 * g.r[e]], wlo);
            atomicAdd(&acc[2 * g.r[e] + 1], whi + (old + wlo < old ? 1ull : 0ull));
        } else {
            atomicAdd(&acc[g.r[e]], wlo);
        }
    }
}

template <int SPAN, int THREADS>
__global__ __launch_bounds__(THREADS) void span_reduce_kernel(const ScatterTable tb, int C, int L, uint64_t total, const uint32_t *start,
                                                              uint64_t base_lo, uint64_t base_hi, uint64_t mask_lo, uint64_t mask_hi,
                                                              const uint64_t *src, bool negate, uint64_t *out, uint32_t *err_flag)
{
    __shared__ unsigned long long acc[2 * SPAN];
    __shared__ uint32_t s_begin[kMaxScatter], s_prefix[2 * kMaxScatter + 2];
    __shared__ const uint32_t *s_loc[kMaxScatter];
    __shared__ const uint64_t *s_vals[kMaxScatter];
    __shared__ uint64_t s_sub[2 * kMaxScatter];
    const uint64_t span = blockIdx.x, p0 = span * SPAN;
    const uint64_t span_len = total - p0 < SPAN ? total - p0 : SPAN;
    const int tid = threadIdx.x;
    for (int i = tid; i < (L == 2 ? 2 : 1) * SPAN; i += THREADS) acc[i] = 0;
    // this span's slice [begin, begin + count) of every client's list (clamped: a malformed list was reported by kernel A and
    // must not turn into reads outside the lists) and the running total of the counts, by a shuffle scan in the first wave:
    // the entries of ALL clients are then walked as one flat index space -- consecutive lanes read consecutive entries
    if (tid < 64) {
        uint32_t cnt = 0;
        if (tid < C) {
            const uint32_t kc = static_cast<uint32_t>(tb.k[tid]);
            const uint32_t b0 = min(start[span * C + tid], kc), b1 = min(start[(span + 1) * C + tid], kc);
            cnt = b1 > b0 ? b1 - b0 : 0;
            s_begin[tid] = b0;
            s_loc[tid] = tb.loc[tid]; s_vals[tid] = tb.vals[tid];
            s_sub[2 * tid] = tb.sub_lo[tid]; s_sub[2 * tid + 1] = tb.sub_hi[tid];
        }
        uint32_t run = cnt;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(run, d, 64);
            if (tid >= d) run += up;
        }
        if (tid == 0) s_prefix[0] = 0;
        s_prefix[tid + 1] = tid < C ? run : 0xffffffffu;        // sentinels: the owner search needs no bounds
        s_prefix[tid + 65] = 0xffffffffu;
    }
    __syncthreads();
    const uint32_t n_entries = s_prefix[C];
    for (uint32_t f0 = tid; f0 < n_entries; f0 += kSpanBatch * THREADS) {
        SpanBatch g;
        span_gather<THREADS>(g, f0, n_entries, s_prefix, s_begin, s_loc, s_vals, L, static_cast<uint32_t>(p0));
        span_add<THREADS>(g, f0, n_entries, acc, s_sub, L, span_len, err_flag);
    }
    __syncthreads();
    const u128 mask = (static_cast<u128>(mask_hi) << 64) | mask_lo;
    const u128 base = (static_cast<u128>(base_hi) << 64) | base_lo;
    for (uint64_t r = tid; r < span_len; r += THREADS) {
        if (L == 2) {
            const u128 a = (static_cast<u128>(acc[2 * r + 1]) << 64) | acc[2 * r];
            const u128 from = src ? ld128_nt(src + 2 * (p0 + r)) : base;
            st128_nt(out + 2 * (p0 + r), (negate ? from - a : from + a) & mask);
        } else {
            const uint64_t from = src ? __builtin_nontemporal_load(src + p0 + r) : base_lo;
            __builtin_nontemporal_store((negate ? from - acc[r] : from + acc[r]) & mask_lo, out + p0 + r);
        }
    }
}

uint64_t span_count(uint64_t total, int span) { return (total + static_cast<uint64_t>(span) - 1) / static_cast<uint64_t>(span); }

// The first list entry of each of the C <= kMaxScatter clients in every span: start_reduce_dev / start_fused_dev (either may be null)
// = (span_count(total, kSpanReduce / kSpanFused) + 1) * C words.
hipError_t launch_span_bounds(const LaunchEnv &env, int C, const uint32_t *const *loc_dev, const uint64_t *k, uint64_t total, uint32_t *start_reduce_dev,
                              uint32_t *start_fused_dev)
{
    if (C > kMaxScatter || C < 1 || (!start_reduce_dev && !start_fused_dev)) return hipErrorInvalidValue;
    if (total == 0) return hipSuccess;
    ScatterTable tb{};
    uint64_t kmax = 0;
    for (int c = 0; c < C; c++) {
        if (k[c] >= (1ull << 32)) return hipErrorInvalidValue;
        tb.loc[c] = loc_dev[c]; tb.k[c] = k[c];
        kmax = std::max(kmax, k[c]);
    }
    bool vec = true;
    for (int c = 0; c < C; c++) vec = vec && (reinterpret_cast<uintptr_t>(loc_dev[c]) & 15u) == 0;
    const dim3 grid(static_cast<unsigned>(kmax / (kStreamThreads * kBoundsPerThread) + 1), C);
    if (vec)
        hipLaunchKernelGGL(span_bounds_kernel<true>, grid, dim3(kStreamThreads), 0, env.stream, tb, C, total, start_reduce_dev, start_fused_dev, env.err_flag);
    else
        hipLaunchKernelGGL(span_bounds_kernel<false>, grid, dim3(kStreamThreads), 0, env.stream, tb, C, total, start_reduce_dev, start_fused_dev, env.err_flag);
    return hipGetLastError();
}

// out[p] = from[p] +/- sum over clients c and entries q with loc[c][q] == p of (vals[c][q] - sub[c])   (mod 2^b), every p < total,
// from = src_dev when given (may be out_dev), the constant base otherwise; loc[c] strictly increasing.
// start_dev: (span_count(total, kSpanReduce) + 1) * C words of scratch.
hipError_t launch_span_reduce(const LaunchEnv &env, int C, const uint32_t *const *loc_dev, const uint64_t *const *vals_dev,
                              const uint64_t *k, const uint64_t *sub, uint64_t base_lo, uint64_t base_hi, uint64_t total,
                              uint32_t *start_dev, const uint64_t *src_dev, bool negate, uint64_t *out_dev, bool bounds_ready)
{
    if (C > kMaxScatter || C < 1) return hipErrorInvalidValue;
    if (total == 0) return hipSuccess;
    const int L = env.b > 64 ? 2 : 1;
    ScatterTable tb{};
    for (int c = 0; c < C; c++) {
        if (k[c] >= (1ull << 32)) return hipErrorInvalidValue;
        tb.loc[c] = loc_dev[c]; tb.vals[c] = vals_dev[c]; tb.k[c] = k[c];
        tb.sub_lo[c] = sub ? sub[static_cast<size_t>(L) * c] : 0;
        tb.sub_hi[c] = sub && L == 2 ? sub[2 * c + 1] : 0;
    }
    uint64_t lo, hi;
    masks_of(env.b, &lo, &hi);
    const uint64_t n_spans = span_count(total, kSpanReduce);
    if (!bounds_ready) {
        const hipError_t e = launch_span_bounds(env, C, loc_dev, k, total, start_dev, nullptr);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((span_reduce_kernel<kSpan, kSpanThreads>), dim3(static_cast<unsigned>(n_spans)), dim3(kSpanThreads), 0, env.stream, tb, C, L, total,
                       start_dev, base_lo, base_hi, lo, hi, src_dev, negate, out_dev, env.err_flag);
    return hipGetLastError();
}

// ---- the span reduce with the PRF inside (int_bits > 64, table PRF) ---------------------------------------------------------------
// The sparse single-mask passes spend more time generating their compact mask streams (one AES block per list entry, LDS-lookup bound)
// than reducing them (HBM bound), and the streams make a round trip through HBM in between.  Here the two run in ONE persistent kernel,
// one workgroup per CU: the AES tables (128 KiB) and the accumulators of a span (kSpanFused positions, 27.5 KiB) share the CU's 160 KiB,
// entry q of client c gets its block term(iter, idx[c], q) computed where the span reduce would have gathered a stored value -- the
// block needs (c, q) only, so the load of the entry's POSITION (and, ENC, of its plaintext) is in flight under the 14 rounds -- and the
// dense read / write of the span (prefetched before the entries, written after them) overlaps with the next span's rounds.
//   ENC = 0    : out[p] = from[p] +/- sum of the masks of the entries at p   (sparse minus-mask / sparse decrypt, a-13)
//   ENC = 1, 2 : ct[c][q] = (pt[c][q] + mask) mod 2^b is stored AND out[p] = base + sum (ct[c][q] - sub[c]): the clients a GPU plays
//                encrypt and their uploads are summed in the same pass (the sparse twin of the chained encrypt's partial aggregate);
//                the value of ENC is the number of limbs of a plaintext
struct SpanPrfTable {
    const uint32_t *loc[kMaxScatter];
    const uint64_t *pt[kMaxScatter];
    uint64_t *ct[kMaxScatter];
    uint32_t k[kMaxScatter], idx[kMaxScatter];
    uint64_t sub_lo[kMaxScatter], sub_hi[kMaxScatter];
};

#ifdef FLASHE_TUNING
__device__ unsigned long long g_span_prf_cycles[24];      // phase cycle sums of workgroup 0, wave 0 (FLASHE_SPAN_PROBE=9)
#define SPAN_PRF_TICK(i) do { if (probe == 9 && blockIdx.x == 0 && tid == 0) { const unsigned long long t_ = __builtin_readcyclecounter(); \
                                                                                g_span_prf_cycles[i] += t_ - tick_; tick_ = t_; } } while (0)
#else
#define SPAN_PRF_TICK(i) do { } while (0)
#endif

// inclusive prefix sum over the 64 lanes without the LDS (row shifts, then the two row broadcasts of the GFX9 DPP set): the shuffle
// form costs six LDS round trips on the one wave every other wave of the workgroup waits for
__device__ __forceinline__ uint32_t wave_scan_u32(uint32_t v)
{
    v += __builtin_amdgcn_update_dpp(0u, v, 0x111, 0xf, 0xf, false);      // row_shr:1
    v += __builtin_amdgcn_update_dpp(0u, v, 0x112, 0xf, 0xf, false);      // row_shr:2
    v += __builtin_amdgcn_update_dpp(0u, v, 0x114, 0xf, 0xf, false);      // row_shr:4
    v += __builtin_amdgcn_update_dpp(0u, v, 0x118, 0xf, 0xf, false);      // row_shr:8
    v += __builtin_amdgcn_update_dpp(0u, v, 0x142, 0xa, 0xf, false);      // row_bcast:15 into rows 1 and 3
    v += __builtin_amdgcn_update_dpp(0u, v, 0x143, 0xc, 0xf, false);      // row_bcast:31 into rows 2 and 3
    return v;
}

// One list entry on its way through the kernel: which client, which compact position, where it lands, and what round 1 needs.
struct SpanPrfEntry {
    bool valid;
    int c;
    uint32_t q, pos;
    uint4 pre;           // CtrPrefix of the client
    CtrVar x;            // the four round-1 lookups on the counter
    u128 pt;             // ENC: the plaintext
};

// Round 5: no barrier in the loop.  A span's accumulators go through two phases -- they RECEIVE the entries' masks (atomics), then they
// are WRITTEN OUT (read, zeroed, `from +/- sum` stored) -- and each phase may start only when every wave is through with the other.
// Round 4 put a workgroup barrier at both boundaries: twice per span all sixteen waves stopped, the last ones ran their final rounds
// alone on their SIMD, and for a fifth of the time no AES lookup was in flight on the CU (58 % LDS-busy).  Now both boundaries are
// split-phase: a wave ARRIVES (one LDS add) when it is through with a phase and WAITS (polls that counter) only where it needs the
// other waves -- the write-out of span i - 1 sits in the middle of the rounds of span i (its accumulators were completed at the end of
// the previous iteration: six rounds earlier), the atomics of span i at the end of its rounds (the accumulators were emptied six rounds
// earlier) -- so a wait almost never blocks, waves drift up to half a span apart, and one wave's atomics, table reads and loop head run
// under the other waves' rounds.  The counters only grow (sixteen arrivals per phase and span).
//
// The protocol leans on two properties of the gfx9 LDS that the C++ memory model does not give: a wave's LDS operations complete in
// issue order (the arrival that lane 0 issues is behind the other 63 lanes' atomics and stores of the same instruction stream), and
// what follows the poll that saw the count cannot be older than it.  This library is built for gfx950 alone; another target must
// not compile these helpers silently.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__) && !defined(__gfx942__) && !defined(__gfx90a__)
#error "span_prf_kernel's split-phase LDS counters assume the in-order LDS of gfx9 (built for gfx950): port phase_arrive / phase_wait first"
#endif
#ifndef FLASHE_SPAN_WRSPLIT
#define FLASHE_SPAN_WRSPLIT 0    // 1 (A/B builds): the write-out of a span by the waves of the two lighter SIMDs only -- measured in round 6: the encrypting pass
                                 // 0.2696 against 0.2704 ms with all sixteen waves writing: nothing (the heavier SIMDs' waves shed a tenth of their instructions
                                 // and the wait in front of the write-out, and the span's period does not move)
#endif

__device__ __forceinline__ void phase_arrive(uint32_t *ctr)
{
    // (workgroup-scope release on this target: s_waitcnt lgkmcnt(0) -- the LDS runs a wave's operations in order, so whatever this wave
    // did to the accumulators or the span tables is ahead of its arrival; no wait for outstanding global stores)
    if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// a look at a counter that nobody waits for: the value is used a round later (threaded through the rounds one step ahead of the wait,
// so that the common case -- everybody arrived long ago -- costs no LDS round trip where the wait stands)
__device__ __forceinline__ uint32_t phase_peek(uint32_t *ctr)
{
    return __hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void phase_wait(uint32_t *ctr, uint32_t target, uint32_t peeked)
{
    uint32_t seen = __builtin_amdgcn_readfirstlane(peeked);
    while (static_cast<int32_t>(seen - target) < 0) {
        __builtin_amdgcn_s_sleep(1);
        seen = __builtin_amdgcn_readfirstlane(__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
    }
    // nothing below moves above the wait -- as a COMPILER barrier: the LDS returns a wave's reads in order, so what follows the read
    // that saw the count cannot be older than it; an acquire fence at workgroup scope also drains the memory counter on this target
    // (s_waitcnt vmcnt(0)), i.e. it would wait here for the dense values that were just requested a span ahead
    asm volatile("" ::: "memory");
}

// SRC: the dense vector `src` is given (the sparse decrypt: out = src - masks); without it the result starts from the constant base and
// the lanes hold no prefetched dense values (sixteen registers with four positions per writing lane: the encrypting instantiations spilled)
template <int ENC, bool SRC>
__global__ __launch_bounds__(kPrfThreads) void span_prf_kernel(const RoundKeys rk, const SpanPrfTable tb, int C, uint32_t iter0, uint64_t total, uint32_t n_spans,
                                                               uint32_t sp_first, uint32_t sp_end, const uint32_t *__restrict__ start, uint64_t base_lo, uint64_t base_hi, uint64_t mask_lo,
                                                               uint64_t mask_hi, const uint64_t *src, bool negate, uint64_t *out,
                                                               const uint32_t *__restrict__ te0, uint32_t *err_flag, int probe)
{
    constexpr int SPAN = kSpanFused, THREADS = kPrfThreads, WAVES = THREADS / 64;
    // Who writes a finished span out (round 6).  A workgroup's waves w and w + 4 share a SIMD; the sixteenth wave keeps the span tables and
    // the fifteenth has entries in one span of four, so fourteen busy waves are 4 + 4 + 3 + 3 on the four SIMDs, and the waves of the two
    // fuller SIMDs finish their rounds 800-1,300 cycles after the others (phase probes, profiles/r06_span_probe9.log): they set the span's
    // period.  FLASHE_SPAN_WRSPLIT: only the waves of the two LIGHTER SIMDs (w mod 4 in {2, 3}: eight waves, four positions per lane)
    // write out; the other eight carry neither the write-out steps nor the wait in front of them.
    // (not with a dense source: four prefetched values per writing lane on top of the rounds' registers spill, 24-72 bytes per lane)
    constexpr bool WRSPLIT = FLASHE_SPAN_WRSPLIT != 0 && !SRC;
    constexpr int WR_WAVES = WRSPLIT ? WAVES / 2 : WAVES, WR_LANES = 64 * WR_WAVES, PER = (SPAN + WR_LANES - 1) / WR_LANES;
    const uint32_t iter = iter0 + te0[kIterShiftWord];
    __shared__ uint32_t tab[kTabWords];
    // the accumulators, low limbs in [0, SPAN), high limbs in [SPAN, 2 SPAN): with the limbs in planes of their own the two 64-bit
    // atomics of an entry spread over twice as many banks as with 16-byte slots (round 6, in-process A/B: both passes -2 %)
    __shared__ __attribute__((aligned(16))) unsigned long long acc[2 * SPAN];
    // (prefix, begin) per client of the span in flight and of the NEXT one: entry f of a span belongs to the client c with
    // pb[c].x <= f < pb[c + 1].x and is entry pb[c].y + (f - pb[c].x) of that client's list; pb[C].x = entries in the span
    __shared__ uint2 s_pb[2][kMaxScatter + 2];
    __shared__ uint4 s_pref[kMaxScatter];                     // CtrPrefix of (iter, idx[c], counter high word 0): round 1 costs 4 lookups
    __shared__ const uint32_t *s_loc[kMaxScatter];
    __shared__ const uint64_t *s_pt[ENC ? kMaxScatter : 1];
    __shared__ uint64_t *s_ct[ENC ? kMaxScatter : 1];
    __shared__ uint64_t s_sub[ENC ? 2 * kMaxScatter : 2];
    __shared__ uint32_t s_phase[2];                           // arrivals: [0] a wave's entries of a span are in, [1] its share of a span is written out
    fill_tables(tab, te0);
    const LaneRegs lr = lane_regs(tab);
    const int tid = threadIdx.x;
    for (int i = tid; i < 2 * SPAN; i += THREADS) acc[i] = 0;
    if (tid < 2) s_phase[tid] = 0;
    // (writer rank: waves 2, 3, 6, 7, 10, 11, 14, 15 -> 0 .. 7; wtid = this lane's index among the writing lanes)
    const int wv = tid >> 6;
    const bool writer = !WRSPLIT || (wv & 2) != 0;
    const int wtid = WRSPLIT ? ((((wv >> 2) << 1) | (wv & 1)) << 6) | (tid & 63) : tid;
    // the LAST wave keeps the span tables: it is the wave with the fewest entries (none at all while a span holds at most 960)
    const int ln = tid & 63;
    const bool keeper = tid >= THREADS - 64;
    const uint32_t kc = keeper && ln < C ? tb.k[ln] : 0u;
    if (tid < C) {
        const CtrPrefix p = ctr_prefix(rk, lr, iter, tb.idx[tid], 0u);
        s_pref[tid] = make_uint4(p.u[0], p.u[1], p.u[2], p.u[3]);
        s_loc[tid] = tb.loc[tid];
        if (ENC) { s_pt[tid] = tb.pt[tid]; s_ct[tid] = tb.ct[tid]; s_sub[2 * tid] = tb.sub_lo[tid]; s_sub[2 * tid + 1] = tb.sub_hi[tid]; }
    }
    const u128 mask = (static_cast<u128>(mask_hi) << 64) | mask_lo;
    const u128 base = (static_cast<u128>(base_hi) << 64) | base_lo;
    const uint32_t stride = gridDim.x;
    // The keeper wave: the slice [f0, f1) of client `ln`'s list in a span (clamped like span_reduce_kernel's) is loaded THREE spans
    // ahead and published TWO spans ahead -- early in an iteration (behind the wait for the previous span's entries, which every wave
    // passes in the middle of its rounds), into the table of the span in flight, which nobody reads any more (its entry count travels in
    // a register) unless the span is crowded (more than 1,024 entries: a second pass looks entries up in it; the table is then published
    // between two barriers at the end of the iteration).  Every lane can so look its entry of the next span up under the rounds of this
    // one, and no wave waits for the keeper.  The loads are unconditional (clamped indices).
    uint32_t f0 = 0, f1 = 0;
    bool f_live = false;
    const uint32_t ln_c = static_cast<uint32_t>(min(ln, C - 1));
#define SPAN_PRF_FETCH(spx)                                                                                              \
    do {                                                                                                                 \
        const uint64_t sp_ = (spx), sc_ = sp_ < n_spans ? sp_ : n_spans - 1;                                             \
        f_live = ln < C && sp_ < sp_end;                                                                                 \
        f0 = start[sc_ * C + ln_c]; f1 = start[(sc_ + 1) * C + ln_c];                                                    \
    } while (0)
#define SPAN_PRF_PUBLISH(buf)                                                                                            \
    do {                                                                                                                 \
        const uint32_t b0_ = min(f0, kc), b1_ = min(f1, kc);                                                             \
        const uint32_t run_ = wave_scan_u32(f_live && b1_ > b0_ ? b1_ - b0_ : 0u);                                       \
        if (ln == 0) s_pb[buf][0].x = 0;                                                                                 \
        if (ln < C) s_pb[buf][ln].y = b0_;                                                                               \
        s_pb[buf][ln + 1].x = ln < C ? run_ : 0xffffffffu;           /* sentinels: the owner search needs no bounds */   \
    } while (0)
    // entry f of the span whose table is s_pb[buf], without anything to hide behind (first span, entries beyond the first 1,024)
    auto lookup = [&](int buf, uint32_t f, uint32_t n_in_span) {
        SpanPrfEntry e;
        int c = 0;
#pragma unroll
        for (int step = 32; step; step >>= 1)
            if (s_pb[buf][c + step].x <= f) c += step;
        const uint2 pb = s_pb[buf][c];
        e.valid = f < n_in_span;
        e.c = c;
        e.q = pb.y + (f - pb.x);
        e.pos = e.valid ? ld32_g(s_loc[c] + e.q) : 0u;
        e.pt = 0;
        if (ENC && e.valid) e.pt = ENC == 2 ? ld128_nt_g(s_pt[c] + 2 * static_cast<uint64_t>(e.q)) : static_cast<u128>(ld64_nt_g(s_pt[c] + e.q));
        e.pre = s_pref[c];
        e.x = ctr_var(rk, lr, e.q);
        return e;
    };
    // what an entry's block is worth once the rounds are done: ENC stores the ciphertext on the way
    auto settle = [&](const SpanPrfEntry &e, const uint32_t (&s)[4], uint32_t p0_lo, uint32_t span_len) {
        if (!e.valid) return;
        u128 w = words_to_u128(s) & mask;
        if (ENC) {
            w = (e.pt + w) & mask;
#ifdef FLASHE_TUNING
            if (probe != 5)
#endif
            if (s_ct[e.c]) st128_nt_g(s_ct[e.c] + 2 * static_cast<uint64_t>(e.q), w);
            w -= (static_cast<u128>(s_sub[2 * e.c + 1]) << 64) | s_sub[2 * e.c];
        }
        const uint32_t r = e.pos - p0_lo;
        if (r >= span_len) { *err_flag = 1; return; }            // a list that is not strictly increasing or reaches beyond the vector
        const unsigned long long wlo = static_cast<unsigned long long>(w), whi = static_cast<unsigned long long>(w >> 64);
#ifdef FLASHE_TUNING
        if (probe == 3) { if (wlo == 0x1234567ull) acc[r] = whi; return; }
#endif
        const unsigned long long old = atomicAdd(&acc[r], wlo);
        atomicAdd(&acc[SPAN + r], whi + (old + wlo < old ? 1ull : 0ull));
    };
    // The last five round keys live in VGPRs: sixty key words + the kernel's pointers do not fit the SGPR file, and what the compiler
    // spills it re-reads with v_readlane inside the rounds (VALU issue is what bounds them)
    uint32_t rkv[20];
#pragma unroll
    for (int i = 0; i < 20; i++) {
        rkv[i] = rk.w[40 + i];
        asm volatile("" : "+v"(rkv[i]));
    }
    uint64_t sp = static_cast<uint64_t>(sp_first) + blockIdx.x;        // (a launch covers the spans [sp_first, sp_end): the whole vector, or one GPU's position range)
    if (keeper) {
        SPAN_PRF_FETCH(sp); SPAN_PRF_PUBLISH(0);
        SPAN_PRF_FETCH(sp + stride); SPAN_PRF_PUBLISH(1);
        SPAN_PRF_FETCH(sp + 2 * static_cast<uint64_t>(stride));
    }
    __syncthreads();
    uint32_t n_entries = s_pb[0][C].x;
    SpanPrfEntry cur = lookup(0, tid, n_entries);
    // (the first entry's loads are waited for HERE: left pending into the loop, they make the compiler guard the entry's use in EVERY
    // iteration with a full wait)
    __builtin_amdgcn_s_waitcnt(0x0f70);          // vmcnt(0)
    __syncthreads();                             // (the keeper's first act in the loop overwrites the table this lookup read; the last barrier of the common path)
    int buf = 0;
    // the span whose accumulators are complete and not yet written out (the one of the previous iteration), the dense vector's values at
    // this lane's positions of it (requested a span ahead of their use: under load a gather from HBM takes several thousand cycles), and
    // how many iterations are behind this wave (the phase counters stand at sixteen arrivals per finished iteration)
    uint64_t wp0 = 0;
    uint32_t wlen = 0, done = 0;
    u128 from[SRC ? PER : 1];
#pragma unroll
    for (int e = 0; e < (SRC ? PER : 1); e++) from[e] = base;
    // the write-out of the previous span, in three steps that the rounds thread one by one (or that a wave without entries runs in a row)
    // (WRSPLIT: a writing lane has four positions; they go through the registers two at a time, one half per round -- all four at once
    // spilled: 84-132 bytes of scratch per lane and the passes 20-70 % slower)
    constexpr int HALVES = WRSPLIT ? 2 : 1, PH = PER / HALVES;
    static_assert(PER % HALVES == 0, "positions per writing lane split evenly over the write-out steps");
    u128 wa[PH];
    auto wout_wait = [&](uint32_t seen, int buf, bool early) {
        phase_wait(&s_phase[0], WAVES * done, seen);                       // every wave's entries of the previous span are in
        // ... which also says that every wave is through with the PREVIOUS iteration, where the table of the span now in flight was
        // searched for this iteration's entries: the keeper may put the table of the span after next in its place
        // (the loads of the slices three spans ahead are issued BEHIND the write-out, see from_load's call sites: the write-out waits for
        // everything the wave has in flight, and every wave waits for the keeper's share of the accumulators at the end of its rounds)
        if (keeper && early) SPAN_PRF_PUBLISH(buf);
    };
    auto wout_read = [&](int h) {
#pragma unroll
        for (int e = 0; e < PH; e++) {
            const uint32_t r = min(static_cast<uint32_t>(wtid + (h * PH + e) * WR_LANES), static_cast<uint32_t>(SPAN - 1));
            wa[e] = (static_cast<u128>(acc[SPAN + r]) << 64) | acc[r];
        }
    };
    auto wout_store = [&](int h) {
#pragma unroll
        for (int e = 0; e < PH; e++) {
            const uint32_t r = wtid + (h * PH + e) * WR_LANES;
            if (r < wlen) {
                acc[r] = 0; acc[SPAN + r] = 0;
#ifdef FLASHE_TUNING
                if (probe == 4 && static_cast<uint64_t>(wa[e]) != 0x1234567ull) continue;      // 4 = no dense read / write
#endif
                const u128 fr = SRC ? from[SRC ? h * PH + e : 0] : base;
                st128_nt(out + 2 * (wp0 + r), (negate ? fr - wa[e] : fr + wa[e]) & mask);
            }
        }
        if (h == HALVES - 1) phase_arrive(&s_phase[1]);                    // this wave's share of the accumulators is empty
    };
    auto from_load = [&](uint64_t q0, uint32_t qlen) {                     // for the NEXT iteration's write-out: the span in flight now
        if (!SRC) return;
#pragma unroll
        for (int e = 0; e < (SRC ? PER : 0); e++) {
            const uint32_t r_ = wtid + e * WR_LANES;
#ifdef FLASHE_TUNING
            from[e] = src && r_ < qlen && probe != 4 ? ld128_nt(src + 2 * (q0 + r_)) : base;
#else
            from[e] = src && r_ < qlen ? ld128_nt(src + 2 * (q0 + r_)) : base;
#endif
        }
    };
#ifdef FLASHE_TUNING
    unsigned long long tick_ = __builtin_readcyclecounter();
#endif
    for (; sp < sp_end; sp += stride, buf ^= 1, done++) {
        const uint64_t p0 = sp * SPAN;
        const uint32_t span_len = static_cast<uint32_t>(total - p0 < SPAN ? total - p0 : SPAN);
        SPAN_PRF_TICK(7);
#ifdef FLASHE_TUNING
        const unsigned long long head_ = __builtin_readcyclecounter();
        if (probe == 2) n_entries = 0;                                     // timing probes (wrong results): 1 = no entries at all (the skeleton: tables, waits, write-out), 2 = no second pass, 3 = no atomics
        if (probe == 1) cur.valid = false;
#endif
        const bool early = n_entries <= THREADS;                           // nobody will look an entry up in this span's table any more
        const int nbuf = buf ^ 1;
#ifdef FLASHE_TUNING
        const uint32_t n_next = probe == 1 ? 0u : (sp + stride < sp_end ? s_pb[nbuf][C].x : 0u);
#else
        const uint32_t n_next = sp + stride < sp_end ? s_pb[nbuf][C].x : 0u;
#endif
        // The first 1,024 entries, one per lane: its block's rounds with everything else threaded through them, one step per round (each a
        // dependent LDS read or a memory request whose latency the sixteen lookups of a round hide): the owner search for the lane's entry
        // of the NEXT span (r = 2..7), that entry's position / plaintext load (8) and round-1 lookups (9); the write-out of the PREVIOUS
        // span (4: peek at the arrivals, 5: wait + read the accumulators, 6: zero them, store, arrive), the dense read for the next
        // write-out (7), a peek at the write-out arrivals for the wait in front of this span's atomics (12).
        SpanPrfEntry nxt;
        nxt.valid = false; nxt.c = 0; nxt.q = 0; nxt.pos = 0; nxt.pt = 0; nxt.pre = make_uint4(0, 0, 0, 0); nxt.x = CtrVar{{0, 0, 0, 0}};
        const uint32_t f = tid;
        uint32_t s[4] = {0, 0, 0, 0};
        uint32_t seen_out = 0;
        if (__builtin_amdgcn_ballot_w64(cur.valid || f < n_next)) {
            const CtrPrefix pre{{cur.pre.x, cur.pre.y, cur.pre.z, cur.pre.w}};
            ctr_round1(pre, cur.x, s);
            int cn = 0;
            uint32_t pv, seen_in = 0;
            uint2 pbn = make_uint2(0, 0);
            const uint32_t *locn = nullptr;
            Lk16 k = issue_main(lr, s);
            pv = s_pb[nbuf][32].x;
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int r = 2; r < 14; r++) {
                // waves that are ahead yield to the ones behind (3, 2, 1, 0 from rounds 2 / 5 / 8 / 11): a wave that runs its rounds alone
                // on its SIMD sees the full lookup latency every round while the other SIMD slots idle (the other schedules measured:
                // tests/perf/experiments/README.md)
                if (r == 2) __builtin_amdgcn_s_setprio(3);
                else if (r == 5) __builtin_amdgcn_s_setprio(2);
                else if (r == 8) __builtin_amdgcn_s_setprio(1);
                else if (r == 11) __builtin_amdgcn_s_setprio(0);
                if (r < 10) finish_main(rk, r, k, s);
                else {
#pragma unroll
                    for (int j = 0; j < 4; j++) s[j] = xor3(xor3(k.v[4 * j], k.v[4 * j + 1], k.v[4 * j + 2]), k.v[4 * j + 3], rkv[4 * (r - 10) + j]);
                }
                if (r <= 7) {                                        // r = 2 .. 7: the six steps 32, 16, .. 1 of the search
                    const int step = 32 >> (r - 2);
                    if (pv <= f) cn += step;
                    if (r < 7) pv = s_pb[nbuf][cn + (step >> 1)].x;
                    else { pbn = s_pb[nbuf][cn]; locn = s_loc[cn]; nxt.pre = s_pref[cn]; }
                } else if (r == 8) {
                    nxt.valid = f < n_next;
                    nxt.c = cn;
                    nxt.q = pbn.y + (f - pbn.x);
#ifdef FLASHE_TUNING
                    if (probe == 5) { nxt.pos = static_cast<uint32_t>(p0 + SPAN * static_cast<uint64_t>(stride)) + (f & 1023u); }    // 5 = no entry loads, no ciphertext stores
                    else
#endif
                    if (nxt.valid) {
                        nxt.pos = ld32_g(locn + nxt.q);
                        if (ENC) nxt.pt = ENC == 2 ? ld128_nt_g(s_pt[cn] + 2 * static_cast<uint64_t>(nxt.q)) : static_cast<u128>(ld64_nt_g(s_pt[cn] + nxt.q));
                    }
                } else if (r == 9) {
                    nxt.x = ctr_var(rk, lr, nxt.q);
                }
                if (writer) {                                        // (wave-uniform)
                    // (WRSPLIT: the dense values of the span that is written out NOW, three rounds ahead of their use -- requested a
                    // span ahead, four of them per lane lived through every round of the span and the decrypt pass spilled)
                    if (WRSPLIT && r == 3) from_load(wp0, wlen);
                    if (r == 4) seen_in = phase_peek(&s_phase[0]);
                    else if (r == 5) { wout_wait(seen_in, buf, early); wout_read(0); }
                    else if (r == 6) {
                        // (in front of the next entry's loads of r = 8: what is outstanding here was requested a span ago)
                        __builtin_amdgcn_s_waitcnt(0x0f70);          // vmcnt(0)
                        wout_store(0);
                        if (HALVES == 2) wout_read(1);
                    }
                    if (r == 7) {
                        if (HALVES == 2) wout_store(1);
                        if (!WRSPLIT) from_load(p0, span_len);
                        if (keeper && early) SPAN_PRF_FETCH(sp + 3 * static_cast<uint64_t>(stride));
                    }
                }
                if (r == 12) seen_out = phase_peek(&s_phase[1]);
                k = r < 13 ? issue_main(lr, s) : issue_final(lr, s);
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int j = 0; j < 4; j++)
                s[j] = bfi(0xff000000u, k.v[4 * j], bfi(0x00ff0000u, k.v[4 * j + 1], bfi(0x0000ff00u, k.v[4 * j + 2], k.v[4 * j + 3]))) ^ rkv[16 + j];
            __builtin_amdgcn_sched_barrier(0);
        } else {
            // a wave without entries in this span and the next: the same steps in a row
            if (writer) {
                if (WRSPLIT) from_load(wp0, wlen);
                wout_wait(phase_peek(&s_phase[0]), buf, early);
                __builtin_amdgcn_s_waitcnt(0x0f70);
#pragma unroll
                for (int h = 0; h < HALVES; h++) { wout_read(h); wout_store(h); }
                if (!WRSPLIT) from_load(p0, span_len);
                if (keeper && early) SPAN_PRF_FETCH(sp + 3 * static_cast<uint64_t>(stride));
            }
            seen_out = phase_peek(&s_phase[1]);
        }
        SPAN_PRF_TICK(1);                                                  // rounds 2 .. 14 (+ everything threaded through them)
#ifdef FLASHE_TUNING
        if (probe == 9 && blockIdx.x == 0 && (tid & 63) == 0) g_span_prf_cycles[8 + (tid >> 6)] += __builtin_readcyclecounter() - head_;
#endif
        // this span's entries go into the accumulators once every wave has emptied its share of them (arrivals of THIS iteration's r = 10)
        phase_wait(&s_phase[1], WR_WAVES * (done + 1), seen_out);
        SPAN_PRF_TICK(4);
        settle(cur, s, static_cast<uint32_t>(p0), span_len);
        SPAN_PRF_TICK(2);
        // entries beyond the first 1,024 of a crowded span: looked up and computed one after the other
        for (uint32_t f2 = tid + THREADS; f2 < n_entries; f2 += THREADS) {
            const SpanPrfEntry e = lookup(buf, f2, n_entries);
            const CtrPrefix pre{{e.pre.x, e.pre.y, e.pre.z, e.pre.w}};
            uint32_t s2[4];
            ctr_round1(pre, e.x, s2);
            aes256_rounds1_deep<2>(rk, lr, s2);
            __builtin_amdgcn_sched_barrier(0);
            settle(e, s2, static_cast<uint32_t>(p0), span_len);
        }
        SPAN_PRF_TICK(3);
        phase_arrive(&s_phase[0]);                                         // this wave's entries of the span are in
        wp0 = p0; wlen = span_len;
        if (!early) {                                                      // (workgroup-uniform; rare: more than 1,024 entries in a span)
            // the table of the span in flight was read by the second pass: published once every wave is through with it, and visible
            // before the next iteration's lookups read it
            __syncthreads();
            if (keeper) { SPAN_PRF_PUBLISH(buf); SPAN_PRF_FETCH(sp + 3 * static_cast<uint64_t>(stride)); }
            __syncthreads();
        }
        SPAN_PRF_TICK(6);
        cur = nxt;
        n_entries = n_next;
    }
    if (wlen && writer) {
        // the last span of this workgroup: nothing is left to hide behind
        if (WRSPLIT) from_load(wp0, wlen);
        wout_wait(phase_peek(&s_phase[0]), 0, false);
        __builtin_amdgcn_s_waitcnt(0x0f70);
#pragma unroll
        for (int h = 0; h < HALVES; h++) { wout_read(h); wout_store(h); }
    }
#undef SPAN_PRF_FETCH
#undef SPAN_PRF_PUBLISH
}

#ifdef FLASHE_TUNING
hipError_t span_prf_cycles(unsigned long long *out8, bool reset)
{
    hipError_t e = hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_span_prf_cycles), 24 * sizeof(unsigned long long));
    if (e == hipSuccess && reset) { const unsigned long long z[24] = {}; e = hipMemcpyToSymbol(HIP_SYMBOL(g_span_prf_cycles), z, sizeof z); }
    return e;
}
#endif

// ---- the same passes at int_bits <= 64 (one limb, table PRF) -----------------------------------------------------------------------
// At b <= 64 an AES block carries m = 128 / b terms and the counters depend on the chunking (jzf_flashe.py:19-45, :316-343): client c's
// k = k[c] compact entries are cut into n_jobs chunks (d, r = divmod(k, n_jobs): the first r chunks hold d + 1 entries), and entry q
// of the chunk [begin, end) is slot (q - begin) % m -- bits [b slot, b slot + b) -- of AES(key, iter | idx[c] | begin + (q - begin) / m).
// Number a client's blocks 0, 1, ... in list order, chunk after chunk: entry q lies in block g(q), g never decreases, so the entries
// [f0, f1) the client has in a span share the blocks g(f0) .. g(f1 - 1).  Those blocks are the span's work items -- per span
// sum_c (g(f1 - 1) - g(f0) + 1) blocks, i.e. entries / m + one per client and per chunk edge in the span (a block cut by a span edge is
// computed by both spans) -- and the lane that computes a block adds the terms of its up-to-m entries into ONE u64 accumulator plane
// (mod 2^64: exact, 2^b divides 2^64; the write-out masks to b bits).  The phases meet at barriers: the AES work of these widths is
// small (config 5's shape at b = 20: about 2.1 M blocks), the pass is bound by the LDS atomics and the dense read / write.
//   ENC = false: out[p] = from[p] +/- sum of the terms of the entries at p;  ENC = true: ct[c][q] = (pt[c][q] + term) mod 2^b is
//   stored where ct[c] is not null, and out[p] = from[p] + sum (ct - sub[c]).  (from = src when SRC, the constant base otherwise)
struct SpanSmallTable {
    const uint32_t *loc[kMaxScatter];
    const uint64_t *pt[kMaxScatter];
    uint64_t *ct[kMaxScatter];
    uint32_t k[kMaxScatter], idx[kMaxScatter];
    uint64_t sub[kMaxScatter];
};

// block number of entry q of a list with chunk geometry g = (d, r, blocks of a (d + 1)-entry chunk, blocks of a d-entry chunk)
__device__ __forceinline__ uint32_t small_block_of(const uint4 g, uint32_t q, uint32_t m)
{
    const uint32_t big = g.y * (g.x + 1);
    if (q < big) {
        const uint32_t j = q / (g.x + 1);
        return j * g.z + (q - j * (g.x + 1)) / m;
    }
    const uint32_t q2 = q - big, j = q2 / g.x;
    return g.y * g.z + j * g.w + (q2 - j * g.x) / m;
}

constexpr int kSmallBatch = 8;       // entries of a block whose position / plaintext loads are in flight at once (the first batch under the rounds)

template <bool ENC, bool SRC>
__global__ __launch_bounds__(kPrfThreads) void span_prf_small_kernel(const RoundKeys rk, const SpanSmallTable tb, int C, uint32_t iter0, uint32_t n_jobs,
                                                                     uint32_t b, uint64_t total, uint32_t n_spans, uint32_t sp_first, uint32_t sp_end,
                                                                     const uint32_t *__restrict__ start, uint64_t base, uint64_t mask, const uint64_t *src,
                                                                     bool negate, uint64_t *out, const uint32_t *__restrict__ te0, uint32_t *err_flag)
{
    constexpr int SPAN = kSpanFused, THREADS = kPrfThreads, PER = (SPAN + THREADS - 1) / THREADS;
    const uint32_t iter = iter0 + te0[kIterShiftWord];
    const uint32_t m = 128u / b;
    __shared__ uint32_t tab[kTabWords];
    __shared__ unsigned long long acc[SPAN];
    __shared__ uint4 s_pref[kMaxScatter];                     // CtrPrefix of (iter, idx[c], counter high word 0)
    __shared__ uint4 s_geo[kMaxScatter];                      // chunk geometry of client c's list (small_block_of)
    __shared__ const uint32_t *s_loc[kMaxScatter];
    __shared__ const uint64_t *s_pt[ENC ? kMaxScatter : 1];
    __shared__ uint64_t *s_ct[ENC ? kMaxScatter : 1];
    __shared__ uint64_t s_sub[ENC ? kMaxScatter : 1];
    // the span in flight: client c's entries [s_f0[c], s_f1[c]) lie in it and touch its blocks s_g0[c] ..; work items s_w[c] .. s_w[c + 1]
    // are client c's (s_w[C] = the span's blocks; the entries past C are sentinels, so the owner search needs no bounds)
    __shared__ uint32_t s_w[kMaxScatter + 1], s_f0[kMaxScatter], s_f1[kMaxScatter], s_g0[kMaxScatter];
    fill_tables(tab, te0);
    const LaneRegs lr = lane_regs(tab);
    const int tid = threadIdx.x;
    for (int i = tid; i < SPAN; i += THREADS) acc[i] = 0;
    if (tid < C) {
        const CtrPrefix p = ctr_prefix(rk, lr, iter, tb.idx[tid], 0u);
        s_pref[tid] = make_uint4(p.u[0], p.u[1], p.u[2], p.u[3]);
        const uint32_t kc = tb.k[tid], d = kc / n_jobs, r = kc % n_jobs;
        s_geo[tid] = make_uint4(d, r, static_cast<uint32_t>((static_cast<uint64_t>(d) + m) / m), static_cast<uint32_t>((static_cast<uint64_t>(d) + m - 1) / m));
        s_loc[tid] = tb.loc[tid];
        if (ENC) { s_pt[tid] = tb.pt[tid]; s_ct[tid] = tb.ct[tid]; s_sub[tid] = tb.sub[tid]; }
    }
    __syncthreads();
    // wave 0: the work items of span sp (the slice [f0, f1) of client `tid`'s list, clamped like span_reduce_kernel's)
    auto span_table = [&](uint64_t sp) {
        const uint32_t ln_c = static_cast<uint32_t>(min(tid, C - 1));
        uint32_t f0 = start[sp * C + ln_c], f1 = start[(sp + 1) * C + ln_c];
        const uint32_t kc = tb.k[ln_c];
        f0 = min(f0, kc); f1 = min(f1, kc);
        uint32_t nw = 0, g0 = 0;
        if (tid < C && f1 > f0) {
            const uint4 geo = s_geo[tid];
            g0 = small_block_of(geo, f0, m);
            nw = small_block_of(geo, f1 - 1, m) - g0 + 1;
        }
        const uint32_t run = wave_scan_u32(nw);
        if (tid == 0) s_w[0] = 0;
        if (tid < C) { s_f0[tid] = f0; s_f1[tid] = f1; s_g0[tid] = g0; }
        s_w[tid + 1] = tid < C ? run : 0xffffffffu;
    };
    uint64_t sp = static_cast<uint64_t>(sp_first) + blockIdx.x;
    const uint32_t stride = gridDim.x;
    if (tid < 64 && sp < sp_end) span_table(sp);
    __syncthreads();
    for (; sp < sp_end; sp += stride) {
        const uint64_t p0 = sp * SPAN;
        const uint32_t span_len = static_cast<uint32_t>(total - p0 < SPAN ? total - p0 : SPAN);
        // the dense values this lane writes out at the end of the span, requested ahead of the span's rounds
        uint64_t from[PER];
#pragma unroll
        for (int e = 0; e < PER; e++) {
            const uint32_t r = tid + e * THREADS;
            from[e] = SRC && r < span_len ? __builtin_nontemporal_load(src + p0 + r) : base;
        }
        const uint32_t n_work = s_w[C];
        for (uint32_t w = tid; w < n_work; w += THREADS) {
            int c = 0;
#pragma unroll
            for (int step = 32; step; step >>= 1)
                if (s_w[c + step] <= w) c += step;
            const uint4 geo = s_geo[c];
            const uint32_t G = s_g0[c] + (w - s_w[c]);
            uint32_t begin, len, i;
            if (G < geo.y * geo.z) {
                const uint32_t j = G / geo.z;
                i = G - j * geo.z; begin = j * (geo.x + 1); len = geo.x + 1;
            } else {
                const uint32_t G2 = G - geo.y * geo.z, j = G2 / geo.w;
                i = G2 - j * geo.w; begin = geo.y * (geo.x + 1) + j * geo.x; len = geo.x;
            }
            const uint32_t e_first = begin + i * m;                                   // the block's slot 0
            const uint32_t e_end = begin + static_cast<uint32_t>(min(static_cast<uint64_t>(len), static_cast<uint64_t>(i + 1) * m));
            const uint32_t q0 = max(e_first, s_f0[c]), q1 = min(e_end, s_f1[c]);
            const uint32_t *loc = s_loc[c];
            const uint64_t *pt = ENC ? s_pt[c] : nullptr;
            uint32_t pos[kSmallBatch];
            uint64_t pv[kSmallBatch];
            auto fetch = [&](uint32_t qa) {
#pragma unroll
                for (int u = 0; u < kSmallBatch; u++) {
                    const bool on = qa + u < q1;
                    pos[u] = on ? ld32_g(loc + qa + u) : 0u;
                    pv[u] = ENC && on ? ld64_nt_g(pt + qa + u) : 0ull;
                }
            };
            fetch(q0);                                                             // in flight under the rounds
            const uint4 pr = s_pref[c];
            const CtrPrefix pre{{pr.x, pr.y, pr.z, pr.w}};
            uint32_t s[4];
            ctr_round1(pre, ctr_var(rk, lr, begin + i), s);
            aes256_rounds1_deep<2>(rk, lr, s);
            const u128 S = words_to_u128(s);
            for (uint32_t qa = q0; qa < q1; qa += kSmallBatch) {
                if (qa != q0) fetch(qa);
#pragma unroll
                for (int u = 0; u < kSmallBatch; u++) {
                    const uint32_t q = qa + u;
                    if (q >= q1) break;
                    uint64_t t = static_cast<uint64_t>(S >> (b * (q - e_first))) & mask;
                    if (ENC) {
                        t = (pv[u] + t) & mask;
                        if (s_ct[c]) __builtin_nontemporal_store(t, FLASHE_GLOBAL(uint64_t, s_ct[c] + q));
                        t -= s_sub[c];
                    }
                    const uint32_t r = pos[u] - static_cast<uint32_t>(p0);
                    if (r >= span_len) { *err_flag = 1; continue; }          // a list that is not strictly increasing or reaches beyond the vector
                    atomicAdd(&acc[r], static_cast<unsigned long long>(t));
                }
            }
        }
        __syncthreads();                                                           // every entry of the span is in
#pragma unroll
        for (int e = 0; e < PER; e++) {
            const uint32_t r = tid + e * THREADS;
            if (r < span_len) {
                const uint64_t v = acc[r];
                acc[r] = 0;
                __builtin_nontemporal_store((negate ? from[e] - v : from[e] + v) & mask, out + p0 + r);
            }
        }
        // (the span table was last read before the barrier above)
        if (tid < 64 && sp + stride < sp_end) span_table(sp + stride);
        __syncthreads();
    }
}

// launch_span_prf at int_bits <= 64 (the arguments checked there, src_dev / out_dev already moved back to position 0)
static hipError_t launch_span_prf_small(const LaunchEnv &env, uint32_t iter, uint32_t n_jobs, int C, const uint32_t *idx, const uint32_t *const *loc_dev,
                                        const uint64_t *k, const uint64_t *const *pt_dev, uint64_t *const *ct_dev, const uint64_t *sub, uint64_t base,
                                        uint64_t total, uint64_t n_spans, uint32_t sp_first, uint32_t sp_end, const uint32_t *start_dev, const uint64_t *src_dev,
                                        bool negate, uint64_t *out_dev)
{
    SpanSmallTable tb{};
    for (int c = 0; c < C; c++) {
        tb.loc[c] = loc_dev[c]; tb.k[c] = static_cast<uint32_t>(k[c]); tb.idx[c] = idx[c];
        if (pt_dev) { tb.pt[c] = pt_dev[c]; tb.ct[c] = ct_dev ? ct_dev[c] : nullptr; tb.sub[c] = sub ? sub[c] : 0; }
    }
    uint64_t lo, hi;
    masks_of(env.b, &lo, &hi);
    const dim3 grid(static_cast<unsigned>(std::min<uint64_t>(sp_end - sp_first, static_cast<uint64_t>(std::max(env.num_cus, 1)))));
#define SPAN_PRF_SMALL_LAUNCH(E, S)                                                                                                      \
    hipLaunchKernelGGL((span_prf_small_kernel<E, S>), grid, dim3(kPrfThreads), 0, env.stream, env.rk, tb, C, iter, n_jobs,              \
                       static_cast<uint32_t>(env.b), total, static_cast<uint32_t>(n_spans), sp_first, sp_end, start_dev, base, lo, src_dev, negate, \
                       out_dev, env.te0_dev, env.err_flag)
    if (!pt_dev) { if (src_dev) SPAN_PRF_SMALL_LAUNCH(false, true); else SPAN_PRF_SMALL_LAUNCH(false, false); }
    else { if (src_dev) SPAN_PRF_SMALL_LAUNCH(true, true); else SPAN_PRF_SMALL_LAUNCH(true, false); }
#undef SPAN_PRF_SMALL_LAUNCH
    return hipGetLastError();
}

// start_dev: the bounds of exactly these lists at kSpanFused positions per span (launch_span_bounds).  first / count: the position
// range the launch covers -- first a multiple of kSpanFused, first + count a multiple of it or the end of the vector; src_dev / out_dev
// address position `first`.  sub: L words per client (L = limbs of int_bits); n_jobs: the chunking of every list (int_bits <= 64 counters).
hipError_t launch_span_prf(const LaunchEnv &env, uint32_t iter, uint32_t n_jobs, int C, const uint32_t *idx, const uint32_t *const *loc_dev, const uint64_t *k,
                           const uint64_t *const *pt_dev, int pt_limbs, uint64_t *const *ct_dev, const uint64_t *sub, uint64_t base_lo, uint64_t base_hi,
                           uint64_t total, const uint32_t *start_dev, const uint64_t *src_dev, bool negate, uint64_t *out_dev, uint64_t first, uint64_t count)
{
    const int L = env.b > 64 ? 2 : 1;
    if (C > kMaxScatter || C < 1 || env.b < 1 || n_jobs == 0 || (pt_dev && pt_limbs != 1 && pt_limbs != L)) return hipErrorInvalidValue;
    if (first > total || count > total - first || first % kSpanFused || (first + count != total && (first + count) % kSpanFused)) return hipErrorInvalidValue;
    if (total == 0 || count == 0) return hipSuccess;
    for (int c = 0; c < C; c++)
        if (k[c] >= (1ull << 32)) return hipErrorInvalidValue;
    const uint64_t n_spans = span_count(total, kSpanFused);
    if (n_spans >= (1ull << 32)) return hipErrorInvalidValue;
    const uint32_t sp_first = static_cast<uint32_t>(first / kSpanFused), sp_end = static_cast<uint32_t>(span_count(first + count, kSpanFused));
    // the kernel indexes the dense vectors by absolute position: pointers that address position `first` are moved back by it
    const uint64_t back = 8 * static_cast<uint64_t>(L) * first;
    if (src_dev) src_dev = reinterpret_cast<const uint64_t *>(reinterpret_cast<uintptr_t>(src_dev) - back);
    out_dev = reinterpret_cast<uint64_t *>(reinterpret_cast<uintptr_t>(out_dev) - back);
    if (L == 1)
        return launch_span_prf_small(env, iter, n_jobs, C, idx, loc_dev, k, pt_dev, ct_dev, sub, base_lo, total, n_spans, sp_first, sp_end, start_dev,
                                     src_dev, negate, out_dev);
    SpanPrfTable tb{};
    for (int c = 0; c < C; c++) {
        tb.loc[c] = loc_dev[c]; tb.k[c] = static_cast<uint32_t>(k[c]); tb.idx[c] = idx[c];
        if (pt_dev) {
            tb.pt[c] = pt_dev[c]; tb.ct[c] = ct_dev ? ct_dev[c] : nullptr;
            tb.sub_lo[c] = sub ? sub[2 * c] : 0; tb.sub_hi[c] = sub ? sub[2 * c + 1] : 0;
        }
    }
    uint64_t lo, hi;
    masks_of(env.b, &lo, &hi);
    const dim3 grid(static_cast<unsigned>(std::min<uint64_t>(sp_end - sp_first, static_cast<uint64_t>(std::max(env.num_cus, 1)))));
    const char *pe = FLASHE_TUNE_ENV("FLASHE_SPAN_PROBE");
    const int probe = pe ? atoi(pe) : 0;
#define SPAN_PRF_LAUNCH(E, S)                                                                                                                 \
    hipLaunchKernelGGL((span_prf_kernel<E, S>), grid, dim3(kPrfThreads), 0, env.stream, env.rk, tb, C, iter, total, static_cast<uint32_t>(n_spans), sp_first, \
                       sp_end, start_dev,                                                                                                          \
                       base_lo, base_hi, lo, hi, src_dev, negate, out_dev, env.te0_dev, env.err_flag, probe)
    // (the encrypting passes are given a dense source only by the second and later groups of more than kMaxScatter clients)
    if (!pt_dev) { if (src_dev) SPAN_PRF_LAUNCH(0, true); else SPAN_PRF_LAUNCH(0, false); }
    else if (pt_limbs == 1) { if (src_dev) SPAN_PRF_LAUNCH(1, true); else SPAN_PRF_LAUNCH(1, false); }
    else { if (src_dev) SPAN_PRF_LAUNCH(2, true); else SPAN_PRF_LAUNCH(2, false); }
#undef SPAN_PRF_LAUNCH
    return hipGetLastError();
}

// ---- sparse + double mask: the masks of the run EDGES, computed only where they are needed -------------------------------------
// set_idx_list's sparse branch of the double mask (jzf_flashe.py:388-426) runs a per-position analysis of the clients' one-hot
// location vectors: position p of client c needs term(c + 1, p) on the ADD side unless client c + 1 holds p too (the masks of
// neighbouring clients telescope), and term(c, p) on the MINUS side unless client c - 1 holds p -- _static_prepare_decrypt_spar
// (:155-225) then evaluates the PRF at exactly the selected dense positions (a block without a selected slot costs no AES).  Here
// the work items are the clients' own list entries: entry q of client c looks its position up in the two neighbouring (sorted)
// lists and computes at most two AES blocks with the counter of the DENSE position (one chunk, begin = 0: counter = p / m, slot
// p % m), writing compact (add, minus) values that the span reduce then scatters -- sum_c k_c block pairs instead of
// (C + 1) x total blocks and no per-list one-hot of `total` bytes.
struct EdgeTable {
    const uint32_t *loc[kMaxScatter + 2];     // entry e + 1 = client c0 + e; entries 0 and nc + 1 = the neighbours outside the group (or null)
    uint64_t k[kMaxScatter + 2];
    uint64_t *va[kMaxScatter], *vm[kMaxScatter];
    uint64_t end[kMaxScatter];                // running total of the group's entries
};

__device__ __forceinline__ bool sorted_contains(const uint32_t *__restrict__ a, uint64_t n, uint32_t x)
{
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo < n && a[lo] == x;
}

__global__ __launch_bounds__(kPrfThreads) void sparse_edge_prf_kernel(const RoundKeys rk, const EdgeTable tb, int nc, uint32_t c0, uint32_t iter0, int b,
                                                                      uint64_t mask_lo, uint64_t mask_hi, const uint32_t *__restrict__ te0)
{
    const uint32_t iter = iter0 + te0[kIterShiftWord];
    __shared__ uint32_t tab[kTabWords];
    fill_tables(tab, te0);
    const LaneRegs lr = lane_regs(tab);
    const u128 mask = (static_cast<u128>(mask_hi) << 64) | mask_lo;
    const uint32_t m = b > 64 ? 1u : 128u / static_cast<uint32_t>(b);
    const uint64_t n_items = tb.end[nc - 1];
    for (uint64_t f = static_cast<uint64_t>(blockIdx.x) * kPrfThreads + threadIdx.x; f < n_items; f += static_cast<uint64_t>(gridDim.x) * kPrfThreads) {
        int e = 0;
#pragma unroll
        for (int step = 32; step; step >>= 1)
            if (e + step < nc && tb.end[e + step - 1] <= f) e += step;
        const uint64_t q = f - (e ? tb.end[e - 1] : 0);
        const uint32_t p = tb.loc[e + 1][q];
        const bool in_prev = tb.loc[e] && sorted_contains(tb.loc[e], tb.k[e], p);
        const bool in_next = tb.loc[e + 2] && sorted_contains(tb.loc[e + 2], tb.k[e + 2], p);
        const uint32_t c = c0 + static_cast<uint32_t>(e);
        const uint64_t ctr = p / m;
        uint32_t s[2][4];
        set_block(s[0], iter, c + 1u, ctr);            // add side: list (prefix) c + 1
        set_block(s[1], iter, c, ctr);                 // minus side: list c
        aes256_encrypt<2>(rk, lr, s, true);
        const int sh = static_cast<int>(static_cast<uint32_t>(b) * (p - static_cast<uint32_t>(ctr) * m));
        const u128 A = in_next ? static_cast<u128>(0) : (words_to_u128(s[0]) >> sh) & mask;
        const u128 M = in_prev ? static_cast<u128>(0) : (words_to_u128(s[1]) >> sh) & mask;
        if (b > 64) { st128(tb.va[e] + 2 * q, A); st128(tb.vm[e] + 2 * q, M); }
        else { tb.va[e][q] = static_cast<uint64_t>(A); tb.vm[e][q] = static_cast<uint64_t>(M); }
    }
}

hipError_t launch_sparse_edge_prf(const LaunchEnv &env, uint32_t iter, int nc, uint32_t c0, const uint32_t *const *loc_with_neighbours,
                                  const uint64_t *k_with_neighbours, uint64_t *const *va_dev, uint64_t *const *vm_dev)
{
    if (nc < 1 || nc > kMaxScatter) return hipErrorInvalidValue;
    EdgeTable tb{};
    uint64_t total = 0;
    for (int e = 0; e < nc + 2; e++) { tb.loc[e] = loc_with_neighbours[e]; tb.k[e] = k_with_neighbours[e]; }
    for (int e = 0; e < nc; e++) { tb.va[e] = va_dev[e]; tb.vm[e] = vm_dev[e]; total += tb.k[e + 1]; tb.end[e] = total; }
    if (total == 0) return hipSuccess;
    uint64_t lo, hi;
    masks_of(env.b, &lo, &hi);
    hipLaunchKernelGGL(sparse_edge_prf_kernel, dim3(grid_for(env, total, kPrfThreads)), dim3(kPrfThreads), 0, env.stream, env.rk, tb, nc, c0, iter, env.b, lo,
                       hi, env.te0_dev);
    return hipGetLastError();
}

// ---- Arbiter.dynamic_masking's cost model on the device (jzf_flashe_block.py:92-112) -----------------------------------------------
// canceled_out_pairs = sum over consecutive clients (c, c + 1) of the positions both hold (the reference ANDs one-hot vectors of
// `total` entries): every list entry of client c looks its position up in client c + 1's sorted list -- the neighbour lookup of
// sparse_edge_prf_kernel without the AES -- and the hits are counted (wave ballot, one atomic per wave).
__global__ __launch_bounds__(kStreamThreads) void shared_positions_kernel(const EdgeTable tb, int nc, unsigned long long *count)
{
    const uint64_t n_items = tb.end[nc - 1];
    unsigned long long mine = 0;
    for (uint64_t f = static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x; f < n_items; f += static_cast<uint64_t>(gridDim.x) * kStreamThreads) {
        int e = 0;
#pragma unroll
        for (int step = 32; step; step >>= 1)
            if (e + step < nc && tb.end[e + step - 1] <= f) e += step;
        const uint64_t q = f - (e ? tb.end[e - 1] : 0);
        const uint32_t p = tb.loc[e + 1][q];
        if (tb.loc[e + 2] && sorted_contains(tb.loc[e + 2], tb.k[e + 2], p)) mine++;
    }
    for (int off = 32; off; off >>= 1) mine += __shfl_down(mine, off, 64);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(count, mine);
}

hipError_t launch_shared_positions(const LaunchEnv &env, int nc, const uint32_t *const *loc_with_next, const uint64_t *k_with_next,
                                   unsigned long long *count_dev)
{
    if (nc < 1 || nc > kMaxScatter) return hipErrorInvalidValue;
    EdgeTable tb{};
    uint64_t total = 0;
    for (int e = 0; e < nc; e++) { tb.loc[e + 1] = loc_with_next[e]; tb.k[e + 1] = k_with_next[e]; total += k_with_next[e]; tb.end[e] = total; }
    tb.loc[nc + 1] = loc_with_next[nc]; tb.k[nc + 1] = k_with_next[nc];
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(shared_positions_kernel, dim3(stream_grid(env, total)), dim3(kStreamThreads), 0, env.stream, tb, nc, count_dev);
    return hipGetLastError();
}

// out[p] = (out[p] + (sel[p] ? stream[p] : 0)) mod 2^b
__global__ __launch_bounds__(kStreamThreads) void sel_accumulate_kernel(uint64_t n, int L, const uint8_t *sel, const uint64_t *stream,
                                                                        uint64_t *out, uint64_t mask_lo, uint64_t mask_hi)
{
    const u128 mask = (static_cast<u128>(mask_hi) << 64) | mask_lo;
    for (uint64_t p = static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x; p < n;
         p += static_cast<uint64_t>(gridDim.x) * kStreamThreads) {
        if (!sel[p]) continue;
        if (L == 2) st128(out + 2 * p, (ld128(out + 2 * p) + ld128(stream + 2 * p)) & mask);
        else out[p] = (out[p] + stream[p]) & mask_lo;
    }
}

hipError_t launch_fill(const LaunchEnv &env, uint64_t n, uint64_t lo, uint64_t hi, uint64_t *out_dev)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(fill_kernel, dim3(stream_grid(env, n)), dim3(kStreamThreads), 0, env.stream, n, env.b > 64 ? 2 : 1, lo, hi, out_dev);
    return hipGetLastError();
}

hipError_t launch_scatter(const LaunchEnv &env, uint64_t total, uint64_t k, const uint32_t *loc_dev, const uint64_t *vals_dev,
                          uint64_t *out_dev, bool accumulate, uint64_t sub_lo, uint64_t sub_hi)
{
    if (k == 0) return hipSuccess;
    uint64_t lo, hi;
    masks_of(env.b, &lo, &hi);
    hipLaunchKernelGGL(scatter_kernel, dim3(stream_grid(env, k)), dim3(kStreamThreads), 0, env.stream, total, k, env.b > 64 ? 2 : 1,
                       loc_dev, vals_dev, out_dev, accumulate, lo, hi, sub_lo, sub_hi, env.err_flag);
    return hipGetLastError();
}

// One list entry of _static_prepare_decrypt_spar: the whole-vector stream for prefix iter|list_idx
// (one chunk, begin = 0) must already be in stream_dev; selected positions are accumulated.
hipError_t launch_sel_accumulate(const LaunchEnv &env, uint64_t total, const uint8_t *sel_dev, const uint64_t *stream_dev,
                                 uint64_t *out_dev)
{
    if (total == 0) return hipSuccess;
    uint64_t lo, hi;
    masks_of(env.b, &lo, &hi);
    hipLaunchKernelGGL(sel_accumulate_kernel, dim3(stream_grid(env, total)), dim3(kStreamThreads), 0, env.stream, total,
                       env.b > 64 ? 2 : 1, sel_dev, stream_dev, out_dev, lo, hi);
    return hipGetLastError();
}

}  // namespace flashe
