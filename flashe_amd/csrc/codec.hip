// gfx950 kernels of the quantise / batch codec either side of the cipher and the host-side descriptors of the fused codec.
#include "device_common.h"
#include "pcg64_stream.h"
#include "philox_stream.h"

#include <type_traits>

namespace flashe {

// ------------------------------------------------------------------------------------------
// Quantise / batch codec either side of the cipher (streaming, HBM-bound)
// ------------------------------------------------------------------------------------------
// float arithmetic below must round exactly like numpy's: no contraction into FMAs
template <typename T>
__global__ __launch_bounds__(kStreamThreads) void quantize_kernel(uint64_t n, const T *x, T alpha, T scale, T den,
                                                                  const double *u, uint64_t *q)
{
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x; j < n;
         j += static_cast<uint64_t>(gridDim.x) * kStreamThreads)
        q[j] = quantize_one<T>(x[j], alpha, scale, den, u[j]);
}

__global__ __launch_bounds__(kStreamThreads) void unquantize_kernel(uint64_t n, const uint64_t *v, int v_limbs, double ac,
                                                                    double two_a, double den, double *out)
{
#pragma clang fp contract(off)
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x; j < n;
         j += static_cast<uint64_t>(gridDim.x) * kStreamThreads) {
        const u128 x = v_limbs == 2 ? ld128(v + 2 * j) : static_cast<u128>(v[j]);
        const double d = u128_to_double(x);
        out[j] = d * two_a / den - ac;
    }
}

// one batch (bs consecutive values, first most significant) per lane
__global__ __launch_bounds__(kStreamThreads) void batch_kernel(uint64_t n, uint64_t nb, const uint64_t *vals, int L, int bs,
                                                               int field_bits, uint64_t *out)
{
    for (uint64_t b = static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x; b < nb;
         b += static_cast<uint64_t>(gridDim.x) * kStreamThreads) {
        u128 t = 0;
        for (int i = 0; i < bs; i++) {
            const uint64_t j = b * bs + i;
            t = (field_bits >= 128 ? 0 : t << field_bits) + (j < n ? vals[j] : 0ull);
        }
        if (L == 2) st128(out + 2 * b, t);
        else out[b] = static_cast<uint64_t>(t);
    }
}

__global__ __launch_bounds__(kStreamThreads) void unbatch_kernel(uint64_t nb, const uint64_t *in, int L, int bs, int field_bits,
                                                                 uint64_t *out)
{
    const u128 mk = field_bits >= 128 ? ~static_cast<u128>(0) : ((static_cast<u128>(1) << field_bits) - 1);
    for (uint64_t b = static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x; b < nb;
         b += static_cast<uint64_t>(gridDim.x) * kStreamThreads) {
        u128 item = L == 2 ? ld128(in + 2 * b) : static_cast<u128>(in[b]);
        for (int i = 0; i < bs; i++) {
            out[b * bs + (bs - 1 - i)] = static_cast<uint64_t>(item & mk);
            item = field_bits >= 128 ? 0 : item >> field_bits;
        }
    }
}

// ---- the batched codec over a flattened model: quantise + batch in one launch, unbatch + unquantise in one launch ----
template <bool BY_VALUE>
__device__ __forceinline__ const BatchLayer *batch_layer_of(const BatchLayer *layers, int n_layers, uint64_t key)
{
    int lo = 0, hi = n_layers - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((BY_VALUE ? layers[mid].value_start : layers[mid].elem_start) <= key) lo = mid; else hi = mid - 1;
    }
    return layers + lo;
}

__global__ __launch_bounds__(kStreamThreads) void quantize_batch_model_kernel(const BatchLayer *__restrict__ layers, int n_layers, int L, int bs,
                                                                              int field_bits, const double *__restrict__ u, uint64_t n_elems,
                                                                              uint64_t *out)
{
    for (uint64_t e = static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x; e < n_elems; e += static_cast<uint64_t>(gridDim.x) * kStreamThreads) {
        const BatchLayer *Ly = batch_layer_of<false>(layers, n_layers, e);
        const uint64_t j0 = (e - Ly->elem_start) * static_cast<uint64_t>(bs);
        u128 t = 0;
        for (int i = 0; i < bs; i++) {
            const uint64_t j = j0 + i;
            uint64_t v = 0;
            if (j < Ly->size) {
                const double draw = u[Ly->value_start + j];
                v = Ly->x_is_f64 ? quantize_one<double>(*FLASHE_GLOBAL(const double, static_cast<const double *>(Ly->x) + j), Ly->p0, Ly->p1, Ly->p2, draw)
                                 : quantize_one<float>(*FLASHE_GLOBAL(const float, static_cast<const float *>(Ly->x) + j), static_cast<float>(Ly->p0), static_cast<float>(Ly->p1),
                                                       static_cast<float>(Ly->p2), draw);
            }
            t = (field_bits >= 128 ? 0 : t << field_bits) + v;          // temp *= mod; temp += value (jzf_quantize.py:178-181)
        }
        if (L == 2) st128(out + 2 * e, t);
        else out[e] = static_cast<uint64_t>(t);
    }
}

__global__ __launch_bounds__(kStreamThreads) void unbatch_unquantize_model_kernel(const BatchLayer *__restrict__ layers, int n_layers, int L, int bs,
                                                                                  int field_bits, const uint64_t *__restrict__ in, uint64_t n_values,
                                                                                  double *out)
{
#pragma clang fp contract(off)
    const u128 mk = field_bits >= 128 ? ~static_cast<u128>(0) : ((static_cast<u128>(1) << field_bits) - 1);
    for (uint64_t g = static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x; g < n_values; g += static_cast<uint64_t>(gridDim.x) * kStreamThreads) {
        const BatchLayer *Ly = batch_layer_of<true>(layers, n_layers, g);
        const uint64_t j = g - Ly->value_start;
        if (j >= Ly->size) continue;                                    // (cannot happen for a well-formed table)
        const uint64_t e = Ly->elem_start + j / static_cast<uint64_t>(bs);
        const int slot = static_cast<int>(j % static_cast<uint64_t>(bs));
        const u128 item = L == 2 ? ld128(in + 2 * e) : static_cast<u128>(in[e]);
        const int sh = field_bits * (bs - 1 - slot);                    // the first value of an element is its most significant field (:240-246)
        const u128 v = (sh >= 128 ? static_cast<u128>(0) : item >> sh) & mk;
        out[g] = u128_to_double(v) * Ly->p1 / Ly->p2 - Ly->p0;          // _static_unquantize_padding_asymmetric (:102-107)
    }
}

hipError_t launch_quantize_batch_model(const LaunchEnv &env, const BatchLayer *layers_dev, int n_layers, int field_bits, const double *u_dev,
                                       uint64_t n_elems, uint64_t *out_dev)
{
    if (n_elems == 0) return hipSuccess;
    if (field_bits < 1 || field_bits > env.b || n_layers < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(quantize_batch_model_kernel, dim3(stream_grid(env, n_elems)), dim3(kStreamThreads), 0, env.stream, layers_dev, n_layers,
                       env.b > 64 ? 2 : 1, env.b / field_bits, field_bits, u_dev, n_elems, out_dev);
    return hipGetLastError();
}

hipError_t launch_unbatch_unquantize_model(const LaunchEnv &env, const BatchLayer *layers_dev, int n_layers, int field_bits, const uint64_t *in_dev,
                                           uint64_t n_values, double *out_dev)
{
    if (n_values == 0) return hipSuccess;
    if (field_bits < 1 || field_bits > env.b || n_layers < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(unbatch_unquantize_model_kernel, dim3(stream_grid(env, n_values)), dim3(kStreamThreads), 0, env.stream, layers_dev, n_layers,
                       env.b > 64 ? 2 : 1, env.b / field_bits, field_bits, in_dev, n_values, out_dev);
    return hipGetLastError();
}

BatchLayer batch_layer_front(uint64_t elem_start, uint64_t value_start, uint64_t size, const void *x_dev, bool is_f64, double alpha, int bits)
{
    const Codec c = codec_quantize_front(x_dev, is_f64, alpha, bits, nullptr);
    return BatchLayer{elem_start, value_start, size, x_dev, c.alpha, c.scale, c.den, c.x_is_f64, 0};
}

BatchLayer batch_layer_back(uint64_t elem_start, uint64_t value_start, uint64_t size, double alpha, int bits, int num_clients)
{
    Codec c{};
    codec_unquantize_back(&c, alpha, bits, num_clients, nullptr);
    return BatchLayer{elem_start, value_start, size, nullptr, c.ac, c.two_a, c.uden, 0, 0};
}

// (2^bits - 1) * num_clients as the reference forms it on Python ints: the exact product, rounded once to float64.  In 64 bits it
// wraps from (62, 5) on; int -> float64 of a 128-bit integer is correctly rounded on the host
static double codec_denominator(int bits, int num_clients)
{
    return static_cast<double>(static_cast<unsigned __int128>((1ull << bits) - 1) * static_cast<unsigned __int128>(num_clients));
}

Codec codec_quantize_front(const void *x_dev, bool is_f64, double alpha, int bits, const double *u_dev)
{
    Codec c{};
    c.x = x_dev; c.u = u_dev; c.alpha = alpha; c.scale = static_cast<double>((1ull << bits) - 1); c.den = 2 * alpha; c.x_is_f64 = is_f64 ? 1 : 0;
    return c;
}

void codec_unquantize_back(Codec *c, double alpha, int bits, int num_clients, double *out_dev)
{
    c->fout = out_dev;
    c->ac = alpha * static_cast<double>(num_clients);
    c->two_a = 2 * c->ac;
    c->uden = codec_denominator(bits, num_clients);
}

CodecLayer codec_layer_front(uint64_t start, const void *x_dev, bool is_f64, double alpha, int bits)
{
    const Codec c = codec_quantize_front(x_dev, is_f64, alpha, bits, nullptr);
    return CodecLayer{start, x_dev, c.alpha, c.scale, c.den, c.x_is_f64, 0};
}

CodecLayer codec_layer_back(uint64_t start, double alpha, int bits, int num_clients)
{
    Codec c{};
    codec_unquantize_back(&c, alpha, bits, num_clients, nullptr);
    return CodecLayer{start, nullptr, c.ac, c.two_a, c.uden, 0, 0};
}

// x <- x + shift (normalize: shift = -mean, unnormalize: shift = +mean; a - b and a + (-b) round identically)
template <typename T, bool WIDE>
__global__ __launch_bounds__(kStreamThreads) void shift_kernel(uint64_t n, T *x, double shift)
{
#pragma clang fp contract(off)
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x; j < n;
         j += static_cast<uint64_t>(gridDim.x) * kStreamThreads)
        x[j] = WIDE ? static_cast<T>(static_cast<double>(x[j]) + shift) : x[j] + static_cast<T>(shift);
}

hipError_t launch_shift(const LaunchEnv &env, uint64_t n, void *x_dev, bool is_f64, double shift, bool wide)
{
    if (n == 0) return hipSuccess;
    const dim3 g(stream_grid(env, n)), t(kStreamThreads);
    if (is_f64) hipLaunchKernelGGL((shift_kernel<double, false>), g, t, 0, env.stream, n, static_cast<double *>(x_dev), shift);
    else if (wide) hipLaunchKernelGGL((shift_kernel<float, true>), g, t, 0, env.stream, n, static_cast<float *>(x_dev), shift);
    else hipLaunchKernelGGL((shift_kernel<float, false>), g, t, 0, env.stream, n, static_cast<float *>(x_dev), shift);
    return hipGetLastError();
}

// part[block] = sum over the block's elements of (x - center)^POW in float64: per-thread partial, wave shuffle tree, one LDS hop
template <typename T, int POW>
__global__ __launch_bounds__(kStreamThreads) void moment_kernel(uint64_t n, const T *x, double center, double *part)
{
    __shared__ double ws[kStreamThreads / 64];
    double acc = 0;
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x; j < n;
         j += static_cast<uint64_t>(gridDim.x) * kStreamThreads) {
        const double d = static_cast<double>(x[j]) - center;
        acc += POW == 1 ? d : d * d;
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0;
        for (int w = 0; w < kStreamThreads / 64; w++) t += ws[w];
        part[blockIdx.x] = t;
    }
}

int moments_grid(const LaunchEnv &env, uint64_t n) { return stream_grid(env, n); }

hipError_t launch_moment(const LaunchEnv &env, uint64_t n, const void *x_dev, bool is_f64, double center, int pow, double *part_dev)
{
    if (n == 0) return hipSuccess;
    const dim3 g(stream_grid(env, n)), t(kStreamThreads);
    if (is_f64 && pow == 1) hipLaunchKernelGGL((moment_kernel<double, 1>), g, t, 0, env.stream, n, static_cast<const double *>(x_dev), center, part_dev);
    else if (is_f64) hipLaunchKernelGGL((moment_kernel<double, 2>), g, t, 0, env.stream, n, static_cast<const double *>(x_dev), center, part_dev);
    else if (pow == 1) hipLaunchKernelGGL((moment_kernel<float, 1>), g, t, 0, env.stream, n, static_cast<const float *>(x_dev), center, part_dev);
    else hipLaunchKernelGGL((moment_kernel<float, 2>), g, t, 0, env.stream, n, static_cast<const float *>(x_dev), center, part_dev);
    return hipGetLastError();
}

hipError_t launch_quantize(const LaunchEnv &env, uint64_t n, const void *x_dev, bool is_f64, double alpha, int bits,
                           const double *u_dev, uint64_t *q_dev)
{
    if (n == 0) return hipSuccess;
    const double scale = static_cast<double>((1ull << bits) - 1);
    if (is_f64)
        hipLaunchKernelGGL(quantize_kernel<double>, dim3(stream_grid(env, n)), dim3(kStreamThreads), 0, env.stream, n,
                           static_cast<const double *>(x_dev), alpha, scale, 2 * alpha, u_dev, q_dev);
    else
        hipLaunchKernelGGL(quantize_kernel<float>, dim3(stream_grid(env, n)), dim3(kStreamThreads), 0, env.stream, n,
                           static_cast<const float *>(x_dev), static_cast<float>(alpha), static_cast<float>(scale),
                           static_cast<float>(2 * alpha), u_dev, q_dev);
    return hipGetLastError();
}

// the back end of a flattened model alone (the values are already plaintext sums, e.g. after the sparse decrypt): element k of
// [first, first + count) comes back as float64 with its layer's parameters
__global__ __launch_bounds__(kStreamThreads) void unquantize_model_kernel(uint64_t count, const uint64_t *v, int v_limbs, const Codec cq, double *out)
{
    for (uint64_t k = static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x; k < count; k += static_cast<uint64_t>(gridDim.x) * kStreamThreads) {
        const u128 x = v_limbs == 2 ? ld128_nt(v + 2 * k) : static_cast<u128>(__builtin_nontemporal_load(v + k));
        __builtin_nontemporal_store(codec_unquantize(cq, k, x), out + k);
    }
}

hipError_t launch_unquantize_model(const LaunchEnv &env, uint64_t count, const uint64_t *v_dev, const Codec &cq, double *out_dev)
{
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(unquantize_model_kernel, dim3(stream_grid(env, count)), dim3(kStreamThreads), 0, env.stream, count, v_dev, env.b > 64 ? 2 : 1, cq,
                       out_dev);
    return hipGetLastError();
}

hipError_t launch_unquantize(const LaunchEnv &env, uint64_t n, const uint64_t *v_dev, int v_limbs, double alpha, int bits,
                             int num_clients, double *out_dev)
{
    if (n == 0) return hipSuccess;
    const double ac = alpha * static_cast<double>(num_clients);
    const double den = codec_denominator(bits, num_clients);
    hipLaunchKernelGGL(unquantize_kernel, dim3(stream_grid(env, n)), dim3(kStreamThreads), 0, env.stream, n, v_dev, v_limbs, ac,
                       2 * ac, den, out_dev);
    return hipGetLastError();
}

// ---- the client step with the ctx's precomputed masks (jzf_flashe.py:456-488, :537-582 with the caches populated): the codec of the
// model-wide kernels above and the combine of stream.hip in one pass, no AES.  Masks read once are non-temporal loads, 16 bytes per
// 128-bit element; add / minus / ct / in address the launch's first element ----
template <bool WIDE>
__global__ __launch_bounds__(kStreamThreads) void quantize_combine_model_kernel(uint64_t count, const Codec cq, const uint64_t *__restrict__ add,
                                                                                const uint64_t *__restrict__ minus, uint64_t *out, uint64_t mask_lo,
                                                                                uint64_t mask_hi)
{
    const u128 mask = (static_cast<u128>(mask_hi) << 64) | mask_lo;
    for (uint64_t k = static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x; k < count; k += static_cast<uint64_t>(gridDim.x) * kStreamThreads) {
        const uint64_t q = codec_quantize(cq, k);
        if (WIDE) {
            u128 v = static_cast<u128>(q) + ld128_nt(add + 2 * k);
            if (minus) v -= ld128_nt(minus + 2 * k);
            st128_nt(out + 2 * k, v & mask);
        } else {
            uint64_t v = q + __builtin_nontemporal_load(add + k);
            if (minus) v -= __builtin_nontemporal_load(minus + k);
            out[k] = v & mask_lo;
        }
    }
}

template <bool WIDE>
__global__ __launch_bounds__(kStreamThreads) void combine_unquantize_model_kernel(uint64_t count, const uint64_t *__restrict__ in,
                                                                                  const uint64_t *__restrict__ add, const uint64_t *__restrict__ minus,
                                                                                  const Codec cq, double *out, uint64_t mask_lo, uint64_t mask_hi)
{
    const u128 mask = (static_cast<u128>(mask_hi) << 64) | mask_lo;
    for (uint64_t k = static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x; k < count; k += static_cast<uint64_t>(gridDim.x) * kStreamThreads) {
        u128 v;
        if (WIDE) {
            v = ld128_nt(in + 2 * k);
            if (add) v += ld128_nt(add + 2 * k);                        // (NULL = zeros: flashe_combine_unquantize_model_dev admits it)
            if (minus) v -= ld128_nt(minus + 2 * k);
            v &= mask;
        } else {
            uint64_t x = __builtin_nontemporal_load(in + k);
            if (add) x += __builtin_nontemporal_load(add + k);
            if (minus) x -= __builtin_nontemporal_load(minus + k);
            v = static_cast<u128>(x & mask_lo);
        }
        __builtin_nontemporal_store(codec_unquantize(cq, k, v), out + k);
    }
}

// the batched walks of quantize_batch_model_kernel / unbatch_unquantize_model_kernel with the combine folded in.  On the way back the
// bs lanes of one element read it and its masks side by side: plain loads, so the element stays in cache for its neighbours
template <bool WIDE>
__global__ __launch_bounds__(kStreamThreads) void quantize_batch_combine_model_kernel(const BatchLayer *__restrict__ layers, int n_layers, int bs,
                                                                                      int field_bits, const double *__restrict__ u, uint64_t n_elems,
                                                                                      const uint64_t *__restrict__ add, const uint64_t *__restrict__ minus,
                                                                                      uint64_t *out, uint64_t mask_lo, uint64_t mask_hi)
{
    const u128 mask = (static_cast<u128>(mask_hi) << 64) | mask_lo;
    for (uint64_t e = static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x; e < n_elems; e += static_cast<uint64_t>(gridDim.x) * kStreamThreads) {
        const BatchLayer *Ly = batch_layer_of<false>(layers, n_layers, e);
        const uint64_t j0 = (e - Ly->elem_start) * static_cast<uint64_t>(bs);
        u128 t = 0;
        for (int i = 0; i < bs; i++) {
            const uint64_t j = j0 + i;
            uint64_t v = 0;
            if (j < Ly->size) {
                const double draw = u[Ly->value_start + j];
                v = Ly->x_is_f64 ? quantize_one<double>(*FLASHE_GLOBAL(const double, static_cast<const double *>(Ly->x) + j), Ly->p0, Ly->p1, Ly->p2, draw)
                                 : quantize_one<float>(*FLASHE_GLOBAL(const float, static_cast<const float *>(Ly->x) + j), static_cast<float>(Ly->p0),
                                                       static_cast<float>(Ly->p1), static_cast<float>(Ly->p2), draw);
            }
            t = (field_bits >= 128 ? 0 : t << field_bits) + v;
        }
        if (WIDE) {
            t += ld128_nt(add + 2 * e);
            if (minus) t -= ld128_nt(minus + 2 * e);
            st128_nt(out + 2 * e, t & mask);
        } else {
            uint64_t x = static_cast<uint64_t>(t) + __builtin_nontemporal_load(add + e);
            if (minus) x -= __builtin_nontemporal_load(minus + e);
            out[e] = x & mask_lo;
        }
    }
}

template <bool WIDE>
__global__ __launch_bounds__(kStreamThreads) void combine_unbatch_unquantize_model_kernel(const BatchLayer *__restrict__ layers, int n_layers, int bs,
                                                                                          int field_bits, const uint64_t *__restrict__ in,
                                                                                          const uint64_t *__restrict__ add, const uint64_t *__restrict__ minus,
                                                                                          uint64_t n_values, double *out, uint64_t mask_lo, uint64_t mask_hi)
{
#pragma clang fp contract(off)
    const u128 mask = (static_cast<u128>(mask_hi) << 64) | mask_lo;
    const u128 mk = field_bits >= 128 ? ~static_cast<u128>(0) : ((static_cast<u128>(1) << field_bits) - 1);
    for (uint64_t g = static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x; g < n_values; g += static_cast<uint64_t>(gridDim.x) * kStreamThreads) {
        const BatchLayer *Ly = batch_layer_of<true>(layers, n_layers, g);
        const uint64_t j = g - Ly->value_start;
        if (j >= Ly->size) continue;                                    // (cannot happen for a well-formed table)
        const uint64_t e = Ly->elem_start + j / static_cast<uint64_t>(bs);
        const int slot = static_cast<int>(j % static_cast<uint64_t>(bs));
        u128 item;
        if (WIDE) {
            item = ld128(in + 2 * e);
            if (add) item += ld128(add + 2 * e);                        // (NULL = zeros: flashe_combine_unbatch_unquantize_model_dev admits it)
            if (minus) item -= ld128(minus + 2 * e);
            item &= mask;
        } else {
            uint64_t x = in[e];
            if (add) x += add[e];
            if (minus) x -= minus[e];
            item = static_cast<u128>(x & mask_lo);
        }
        const int sh = field_bits * (bs - 1 - slot);
        const u128 v = (sh >= 128 ? static_cast<u128>(0) : item >> sh) & mk;
        out[g] = u128_to_double(v) * Ly->p1 / Ly->p2 - Ly->p0;
    }
}

hipError_t launch_quantize_combine_model(const LaunchEnv &env, uint64_t count, const Codec &cq, const uint64_t *add_dev, const uint64_t *minus_dev,
                                         uint64_t *ct_dev)
{
    if (count == 0) return hipSuccess;
    uint64_t lo, hi;
    masks_of(env.b, &lo, &hi);
    const dim3 g(stream_grid(env, count)), t(kStreamThreads);
    if (env.b > 64) hipLaunchKernelGGL(quantize_combine_model_kernel<true>, g, t, 0, env.stream, count, cq, add_dev, minus_dev, ct_dev, lo, hi);
    else hipLaunchKernelGGL(quantize_combine_model_kernel<false>, g, t, 0, env.stream, count, cq, add_dev, minus_dev, ct_dev, lo, hi);
    return hipGetLastError();
}

hipError_t launch_combine_unquantize_model(const LaunchEnv &env, uint64_t count, const uint64_t *in_dev, const uint64_t *add_dev,
                                           const uint64_t *minus_dev, const Codec &cq, double *out_dev)
{
    if (count == 0) return hipSuccess;
    uint64_t lo, hi;
    masks_of(env.b, &lo, &hi);
    const dim3 g(stream_grid(env, count)), t(kStreamThreads);
    if (env.b > 64) hipLaunchKernelGGL(combine_unquantize_model_kernel<true>, g, t, 0, env.stream, count, in_dev, add_dev, minus_dev, cq, out_dev, lo, hi);
    else hipLaunchKernelGGL(combine_unquantize_model_kernel<false>, g, t, 0, env.stream, count, in_dev, add_dev, minus_dev, cq, out_dev, lo, hi);
    return hipGetLastError();
}

hipError_t launch_quantize_batch_combine_model(const LaunchEnv &env, const BatchLayer *layers_dev, int n_layers, int field_bits, const double *u_dev,
                                               uint64_t n_elems, const uint64_t *add_dev, const uint64_t *minus_dev, uint64_t *ct_dev)
{
    if (n_elems == 0) return hipSuccess;
    if (field_bits < 1 || field_bits > env.b || n_layers < 1) return hipErrorInvalidValue;
    uint64_t lo, hi;
    masks_of(env.b, &lo, &hi);
    const dim3 g(stream_grid(env, n_elems)), t(kStreamThreads);
    if (env.b > 64)
        hipLaunchKernelGGL(quantize_batch_combine_model_kernel<true>, g, t, 0, env.stream, layers_dev, n_layers, env.b / field_bits, field_bits, u_dev,
                           n_elems, add_dev, minus_dev, ct_dev, lo, hi);
    else
        hipLaunchKernelGGL(quantize_batch_combine_model_kernel<false>, g, t, 0, env.stream, layers_dev, n_layers, env.b / field_bits, field_bits, u_dev,
                           n_elems, add_dev, minus_dev, ct_dev, lo, hi);
    return hipGetLastError();
}

hipError_t launch_combine_unbatch_unquantize_model(const LaunchEnv &env, const BatchLayer *layers_dev, int n_layers, int field_bits, const uint64_t *in_dev,
                                                   const uint64_t *add_dev, const uint64_t *minus_dev, uint64_t n_values, double *out_dev)
{
    if (n_values == 0) return hipSuccess;
    if (field_bits < 1 || field_bits > env.b || n_layers < 1) return hipErrorInvalidValue;
    uint64_t lo, hi;
    masks_of(env.b, &lo, &hi);
    const dim3 g(stream_grid(env, n_values)), t(kStreamThreads);
    if (env.b > 64)
        hipLaunchKernelGGL(combine_unbatch_unquantize_model_kernel<true>, g, t, 0, env.stream, layers_dev, n_layers, env.b / field_bits, field_bits,
                           in_dev, add_dev, minus_dev, n_values, out_dev, lo, hi);
    else
        hipLaunchKernelGGL(combine_unbatch_unquantize_model_kernel<false>, g, t, 0, env.stream, layers_dev, n_layers, env.b / field_bits, field_bits,
                           in_dev, add_dev, minus_dev, n_values, out_dev, lo, hi);
    return hipGetLastError();
}

// ---- a COHORT's online step with masks the caller holds (flashe_quantize_combine_cohort*_dev): C float models + C precomputed masks ->
// C ciphertexts + their sum in ONE memory-bound pass, no AES, no integer plaintext in HBM.  E = the element type of masks, ciphertexts
// and sum: uint32_t (compact layout), uint64_t (one limb) or u128 (two limbs).
// Un-batched: a lane owns FOUR consecutive values.  Where they lie inside one layer -- all but the few runs across a layer boundary and
// the model's tail -- every stream is read and written in 16-byte accesses at the element's own alignment (layer starts are arbitrary):
// four float32 or two float64, two draws, four uint32 / two uint64 / one 128-bit element; masks and draws are non-temporal loads, the
// ciphertexts non-temporal stores.  The clients are walked G at a time (3 G streams in flight per lane, the running sum in registers):
// fewer streams at once stream faster (NOTES section 4); G is kPrepCohortGroup.
template <class E> __device__ __forceinline__ E prep_ld(const void *p, uint64_t k)
{
    if constexpr (sizeof(E) == 16) return ld128_nt_g(static_cast<const uint64_t *>(p) + 2 * k);
    else return __builtin_nontemporal_load(FLASHE_GLOBAL(const E, static_cast<const E *>(p) + k));
}
template <class E> __device__ __forceinline__ void prep_st(void *p, uint64_t k, E v)
{
    if constexpr (sizeof(E) == 16) st128_nt_g(static_cast<uint64_t *>(p) + 2 * k, v);
    else __builtin_nontemporal_store(v, FLASHE_GLOBAL(E, static_cast<E *>(p) + k));
}
__device__ __forceinline__ void prep_ld4(const void *p, uint64_t k, uint32_t (&v)[4])
{
    const cohort_u32x4 x = __builtin_nontemporal_load(FLASHE_GLOBAL(const cohort_u32x4, static_cast<const uint32_t *>(p) + k));
    v[0] = x[0]; v[1] = x[1]; v[2] = x[2]; v[3] = x[3];
}
__device__ __forceinline__ void prep_ld4(const void *p, uint64_t k, uint64_t (&v)[4])
{
    const cohort_u64x2 a = __builtin_nontemporal_load(FLASHE_GLOBAL(const cohort_u64x2, static_cast<const uint64_t *>(p) + k));
    const cohort_u64x2 b = __builtin_nontemporal_load(FLASHE_GLOBAL(const cohort_u64x2, static_cast<const uint64_t *>(p) + k + 2));
    v[0] = a[0]; v[1] = a[1]; v[2] = b[0]; v[3] = b[1];
}
__device__ __forceinline__ void prep_ld4(const void *p, uint64_t k, u128 (&v)[4])
{
#pragma unroll
    for (int t = 0; t < 4; t++) v[t] = ld128_nt_g(static_cast<const uint64_t *>(p) + 2 * (k + t));
}
__device__ __forceinline__ void prep_st4(void *p, uint64_t k, const uint32_t (&v)[4])
{
    const cohort_u32x4 x = {v[0], v[1], v[2], v[3]};
    __builtin_nontemporal_store(x, FLASHE_GLOBAL(cohort_u32x4, static_cast<uint32_t *>(p) + k));
}
__device__ __forceinline__ void prep_st4(void *p, uint64_t k, const uint64_t (&v)[4])
{
    const cohort_u64x2 a = {v[0], v[1]}, b = {v[2], v[3]};
    __builtin_nontemporal_store(a, FLASHE_GLOBAL(cohort_u64x2, static_cast<uint64_t *>(p) + k));
    __builtin_nontemporal_store(b, FLASHE_GLOBAL(cohort_u64x2, static_cast<uint64_t *>(p) + k + 2));
}
__device__ __forceinline__ void prep_st4(void *p, uint64_t k, const u128 (&v)[4])
{
#pragma unroll
    for (int t = 0; t < 4; t++) st128_nt_g(static_cast<uint64_t *>(p) + 2 * (k + t), v[t]);
}
// the float bits of four values of a row: one 16-byte access (float32) or two (float64)
__device__ __forceinline__ void prep_src4(const void *x, bool f64, uint64_t r, uint64_t (&raw)[4])
{
    if (f64) {
        const cohort_u64x2 a = *FLASHE_GLOBAL(const cohort_u64x2, static_cast<const uint64_t *>(x) + r);
        const cohort_u64x2 b = *FLASHE_GLOBAL(const cohort_u64x2, static_cast<const uint64_t *>(x) + r + 2);
        raw[0] = a[0]; raw[1] = a[1]; raw[2] = b[0]; raw[3] = b[1];
    } else {
        const cohort_u32x4 a = *FLASHE_GLOBAL(const cohort_u32x4, static_cast<const uint32_t *>(x) + r);
        raw[0] = a[0]; raw[1] = a[1]; raw[2] = a[2]; raw[3] = a[3];
    }
}

// Where a launch's stochastic-rounding draws come from.  BufferDraws: the client-major buffer pc.u an earlier launch wrote -- the bits of
// four draws are loaded with the group's other streams (load4) and turned into doubles when the client is computed (draws4).
// PhiloxDraws: np.random.Philox streams generated here (philox_stream.h: client c's draw for value k is word (skip_c + k) % 4 of
// block(base_c + (skip_c + k) / 4)) from one 56-byte plan per client -- nothing is loaded; a lane's four values are one block where
// skip_c = 0, else words skip_c .. 3 of one block and 0 .. skip_c - 1 of the next, both computed by the lane (sharing the second with
// the neighbouring lane is not built); skip_c is uniform over the launch, so that choice is a scalar branch.
struct BufferDraws {
    const double *u;
    uint64_t n_values;
    __device__ __forceinline__ void load4(int c, uint64_t k0, uint64_t (&ub)[4]) const { prep_ld4(u, static_cast<uint64_t>(c) * n_values + k0, ub); }
    __device__ __forceinline__ void draws4(int, uint64_t, const uint64_t (&ub)[4], double (&d)[4]) const
    {
#pragma unroll
        for (int t = 0; t < 4; t++) d[t] = __longlong_as_double(static_cast<long long>(ub[t]));
    }
    __device__ __forceinline__ double draw(int c, uint64_t k) const
    {
        return __longlong_as_double(static_cast<long long>(ld64_nt_g(reinterpret_cast<const uint64_t *>(u) + static_cast<uint64_t>(c) * n_values + k)));
    }
    __device__ __forceinline__ void start() {}
    __device__ __forceinline__ void next_pass() {}
};
using flashe_philox::ClientPlan;
static_assert(sizeof(ClientPlan) == 56, "the plan rows are 56 bytes");
struct PhiloxDraws {
    const ClientPlan *__restrict__ plans;
    __device__ __forceinline__ void load4(int, uint64_t, uint64_t (&)[4]) const {}
    __device__ __forceinline__ void draws4(int c, uint64_t k0, const uint64_t (&)[4], double (&d)[4]) const
    {
        __asm__ volatile("" ::: "memory");            // (one client's plan in scalar registers at a time)
        const ClientPlan &p = plans[c];
        const uint64_t key[2] = {p.key[0], p.key[1]}, base[4] = {p.base[0], p.base[1], p.base[2], p.base[3]};
        flashe_philox::client_draws4(key, base, p.skip, k0, d);
    }
    __device__ __forceinline__ double draw(int c, uint64_t k) const
    {
        const ClientPlan &p = plans[c];
        const uint64_t key[2] = {p.key[0], p.key[1]}, base[4] = {p.base[0], p.base[1], p.base[2], p.base[3]};
        return flashe_philox::client_draw(key, base, p.skip, k);
    }
    __device__ __forceinline__ void start() {}
    __device__ __forceinline__ void next_pass() {}
};

// Pcg64Draws: np.random.PCG64 / PCG64DXSM streams generated here (pcg64_stream.h: client c's draw for value k outputs from
// A^k origin_c + G_k inc_c) from one 32-byte plan per client -- nothing is loaded.  The lane holds ONE jump, over 4 g steps for its run g,
// whatever the client: start() builds it from the tables (the workgroup's part is uniform), next_pass() composes it with the grid's
// stride jump; a client is then its plan, read as scalars: apply, four outputs, three steps between them.  The value-by-value path takes
// the same run's draws and indexes them.  One launch is one variant V.  (The Pow2 rows are built by the function pcg64.hip builds its own
// with; device code is not linked across translation units here, so each keeps its 4 KiB.)
alignas(32) __device__ const flashe_pcg64::Pow2Table kCohortPow2[flashe_pcg64::kVariants] = {flashe_pcg64::make_pow2_table(flashe_pcg64::kPcg64),
                                                                                          flashe_pcg64::make_pow2_table(flashe_pcg64::kDxsm)};
alignas(32) __device__ const flashe_pcg64::RunTable kCohortRun[flashe_pcg64::kVariants] = {flashe_pcg64::make_run_table(flashe_pcg64::kPcg64),
                                                                                        flashe_pcg64::make_run_table(flashe_pcg64::kDxsm)};
static_assert(flashe_pcg64::kLanes == kStreamThreads, "a RunTable row per thread of a stream workgroup");
static_assert(sizeof(flashe_pcg64::ClientPlan) == 32, "the plan rows are 32 bytes");
template <flashe_pcg64::Variant V> struct Pcg64Draws {
    const flashe_pcg64::ClientPlan *__restrict__ plans;
    flashe_pcg64::Jump stride, lane;
    __device__ __forceinline__ void start()
    {
        const uint64_t *row = kCohortRun[V].row[threadIdx.x].mul;
        const flashe_pcg64::Row mine{{row[0], row[1]}, {row[2], row[3]}};
        lane = flashe_pcg64::lane_jump(flashe_pcg64::workgroup_jump(kCohortPow2[V], blockIdx.x), mine);
    }
    __device__ __forceinline__ void next_pass() { lane = flashe_pcg64::next_pass(lane, stride); }
    __device__ __forceinline__ void load4(int, uint64_t, uint64_t (&)[4]) const {}
    __device__ __forceinline__ void draws4(int c, uint64_t, const uint64_t (&)[4], double (&d)[4]) const
    {
        const flashe_pcg64::ClientPlan &p = plans[c];
        uint64_t w[4];
        flashe_pcg64::run_words<V>(lane, flashe_pcg64::make128(p.origin[1], p.origin[0]), flashe_pcg64::make128(p.inc[1], p.inc[0]), w);
#pragma unroll
        for (int t = 0; t < 4; t++) d[t] = flashe_pcg64::to_double(w[t]);
    }
    __device__ __forceinline__ double draw(int c, uint64_t k) const
    {
        const flashe_pcg64::ClientPlan &p = plans[c];
        return flashe_pcg64::to_double(flashe_pcg64::run_word<V>(lane, flashe_pcg64::make128(p.origin[1], p.origin[0]),
                                                                 flashe_pcg64::make128(p.inc[1], p.inc[0]), static_cast<uint32_t>(k & 3)));
    }
};

// clients c .. c + G - 1 over the four values k0 .. k0 + 3 of table row `row` (r = k0 - the row's start)
template <class E, int G, class Draws>
__device__ __forceinline__ void prep_cohort_run(const PrepCohort &pc, const Draws &dr, int row, bool f64, double p0, double p1, double p2, int c, uint64_t k0,
                                                uint64_t r, E modmask, E (&sum)[4])
{
    uint64_t raw[G][4], ub[G][4];
    E mk[G][4];
#pragma unroll
    for (int i = 0; i < G; i++) {
        prep_src4(pc.src[static_cast<size_t>(c + i) * pc.n_layers + row], f64, r, raw[i]);
        dr.load4(c + i, k0, ub[i]);
        prep_ld4(pc.mask[c + i], k0, mk[i]);
    }
#pragma unroll
    for (int i = 0; i < G; i++) {
        double d[4];
        dr.draws4(c + i, k0, ub[i], d);
        E v[4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            v[t] = (static_cast<E>(cohort_quantize_raw(raw[i][t], f64, p0, p1, p2, d[t])) + mk[i][t]) & modmask;
            sum[t] += v[t];
        }
        prep_st4(pc.ct[c + i], k0, v);
    }
}

// the un-batched launch over either source of draws: the layer of a lane's run of four, the run for the clients in groups of G, and
// value by value for a run across a layer boundary or the model's tail.  A source that keeps lane state is told where the walk starts
// (start: run blockIdx.x kStreamThreads + threadIdx.x) and of every pass on (next_pass: gridDim.x kStreamThreads runs further).
template <class E, int G, class Draws> __device__ __forceinline__ void prep_cohort_body(const PrepCohort &pc, Draws &dr, E modmask)
{
    const uint64_t n = pc.n, runs = (n + 3) / 4;
    const int C = pc.n_clients;
    dr.start();
    for (uint64_t g = static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x; g < runs;
         g += static_cast<uint64_t>(gridDim.x) * kStreamThreads, dr.next_pass()) {
        const uint64_t k0 = 4 * g;
        int lo = 0, hi = pc.n_layers - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (pc.layers[mid].start <= k0) lo = mid; else hi = mid - 1;
        }
        const uint64_t end = lo + 1 < pc.n_layers ? pc.layers[lo + 1].start : n;
        if (k0 + 4 <= end) {
            const CodecLayer *L = pc.layers + lo;
            const bool f64 = L->x_is_f64 != 0;
            const double p0 = L->p0, p1 = L->p1, p2 = L->p2;
            const uint64_t r = k0 - L->start;
            E sum[4] = {0, 0, 0, 0};
            int c = 0;
            for (; c + G <= C; c += G) prep_cohort_run<E, G>(pc, dr, lo, f64, p0, p1, p2, c, k0, r, modmask, sum);
            for (; c < C; c++) prep_cohort_run<E, 1>(pc, dr, lo, f64, p0, p1, p2, c, k0, r, modmask, sum);
            if (pc.sum) {
#pragma unroll
                for (int t = 0; t < 4; t++) sum[t] &= modmask;
                prep_st4(pc.sum, k0, sum);
            }
            continue;
        }
        // a run across a layer boundary, or the model's tail: value by value (the rows hold no empty layer: starts ascend strictly)
        const uint64_t kend = k0 + 4 < n ? k0 + 4 : n;
        for (uint64_t k = k0; k < kend; k++) {
            while (lo + 1 < pc.n_layers && pc.layers[lo + 1].start <= k) lo++;
            const CodecLayer *L = pc.layers + lo;
            const bool f64 = L->x_is_f64 != 0;
            E sum = 0;
            for (int c = 0; c < C; c++) {
                const double u = dr.draw(c, k);
                const uint64_t q = cohort_quantize_raw(cohort_load(pc.src[static_cast<size_t>(c) * pc.n_layers + lo], f64, k - L->start), f64, L->p0, L->p1, L->p2, u);
                const E v = (static_cast<E>(q) + prep_ld<E>(pc.mask[c], k)) & modmask;
                prep_st<E>(pc.ct[c], k, v);
                sum += v;
            }
            if (pc.sum) prep_st<E>(pc.sum, k, sum & modmask);
        }
    }
}

template <class E, int G>
__global__ __launch_bounds__(kStreamThreads) void quantize_combine_cohort_kernel(const PrepCohort pc, E modmask)
{
    BufferDraws dr{pc.u, pc.n_values};
    prep_cohort_body<E, G>(pc, dr, modmask);
}

// the same launch with the draws generated inside it (flashe_quantize_combine_cohort_philox*_dev): no draw buffer is written by an earlier
// launch and none is read here -- 16 bytes less per value and client, one launch less.  pc.u is not read.  The batched job's form is
// quantize_batch_philox_combine_cohort_kernel further down: its lane owns four elements, so that no block is computed twice.
template <class E, int G>
__global__ __launch_bounds__(kStreamThreads) void quantize_philox_combine_cohort_kernel(const PrepCohort pc, const ClientPlan *__restrict__ plans, E modmask)
{
    PhiloxDraws dr{plans};
    prep_cohort_body<E, G>(pc, dr, modmask);
}

// the same with the draws of np.random.PCG64 (V = kPcg64) or np.random.PCG64DXSM (kDxsm) streams generated inside it
// (flashe_quantize_combine_cohort_pcg64*_dev): Pcg64Draws.  stride: the jump over 4 kStreamThreads gridDim.x steps.  pc.u is not read.
template <class E, int G, flashe_pcg64::Variant V>
__global__ __launch_bounds__(kStreamThreads) void quantize_pcg64_combine_cohort_kernel(const PrepCohort pc, const flashe_pcg64::ClientPlan *__restrict__ plans,
                                                                                       const flashe_pcg64::Row stride, E modmask)
{
    Pcg64Draws<V> dr{plans, flashe_pcg64::from_row(stride), {}};
    prep_cohort_body<E, G>(pc, dr, modmask);
}

// The batched job: a lane owns one batched element of every client -- quantize_batch_model_kernel's plaintext (every layer padded to whole
// elements on its own, the first value most significant; a whole element reads its floats and draws in 16-byte runs where BS is compiled
// in, 5 / 6 / 7; BS = 0: any bs, value by value) -- plus the client's mask.  pc.n counts elements, pc.rows[2 r], pc.rows[2 r + 1] = row
// r's first element and its value count, layers[r].start = its first value.
template <class E, int G, int BS>
__device__ __forceinline__ void prep_batch_run(const PrepCohort &pc, int row, bool f64, double p0, double p1, double p2, uint64_t vstart, uint64_t j0,
                                               uint64_t size, int c, uint64_t e, E modmask, E &sum)
{
    u128 x[G];
    E mk[G];
#pragma unroll
    for (int i = 0; i < G; i++) {
        const void *xs = pc.src[static_cast<size_t>(c + i) * pc.n_layers + row];
        const double *ud = pc.u + static_cast<uint64_t>(c + i) * pc.n_values + vstart;
        mk[i] = prep_ld<E>(pc.mask[c + i], e);
        if constexpr (BS != 0) x[i] = cohort_batch_element<BS>(xs, f64, p0, p1, p2, ud, j0, size, pc.field_bits);
        else x[i] = cohort_batch_walk<0>(xs, f64, p0, p1, p2, ud, j0, size, pc.field_bits, pc.bs);
    }
#pragma unroll
    for (int i = 0; i < G; i++) {
        const E v = (static_cast<E>(x[i]) + mk[i]) & modmask;
        prep_st<E>(pc.ct[c + i], e, v);
        sum += v;
    }
}

template <class E, int G, int BS>
__global__ __launch_bounds__(kStreamThreads) void quantize_batch_combine_cohort_kernel(const PrepCohort pc, E modmask)
{
    const int C = pc.n_clients;
    for (uint64_t e = static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x; e < pc.n; e += static_cast<uint64_t>(gridDim.x) * kStreamThreads) {
        int lo = 0, hi = pc.n_layers - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (pc.rows[2 * mid] <= e) lo = mid; else hi = mid - 1;
        }
        const CodecLayer *L = pc.layers + lo;
        const bool f64 = L->x_is_f64 != 0;
        const double p0 = L->p0, p1 = L->p1, p2 = L->p2;
        const uint64_t vstart = L->start, size = pc.rows[2 * lo + 1], j0 = (e - pc.rows[2 * lo]) * static_cast<uint64_t>(BS ? BS : pc.bs);
        E sum = 0;
        int c = 0;
        for (; c + G <= C; c += G) prep_batch_run<E, G, BS>(pc, lo, f64, p0, p1, p2, vstart, j0, size, c, e, modmask, sum);
        for (; c < C; c++) prep_batch_run<E, 1, BS>(pc, lo, f64, p0, p1, p2, vstart, j0, size, c, e, modmask, sum);
        if (pc.sum) prep_st<E>(pc.sum, e, sum & modmask);
    }
}

// clients per group of the kernels above.  NOT MEASURED yet: 2 is the largest group at which every instantiation stays within 128 VGPRs
// (4 takes up to 178).  tests/perf/prepared_cohort_step.py alternates 1 / 2 / 4 in one process on the tuning build; no log of it exists.
constexpr int kPrepCohortGroup = 2;

// ---- the batched job with the draws generated inside the launch (flashe_quantize_batch_combine_cohort_philox_dev): pc.u is not read ----
// A lane owns a GROUP of four consecutive elements of one row (groups[r] = row r's first group; a row's last group may hold fewer).  The
// 4 BS values of four whole elements are consecutive values of the client, so they are words of BS Philox blocks where the client's
// stream is block-aligned at the group's first value and of BS + 1 where it is not (philox_stream.h: RunBlocks; the phase is the same for
// every group of a client and row, so the branch on it diverges only in a wave that straddles rows): the lane computes each block once,
// in order, reads the four floats that go with it in one 16-byte access (two for float64), one run ahead of the block that rounds
// them, and packs the four elements as the blocks arrive -- one element at a time: its mask is requested when its first value is
// packed, and it is masked, stored and added to the sum when its last one is (four packed elements and four masks at once do not fit
// the streaming budget at 128 bits); the sum is stored four elements at a time.
// A client's body is BS + 1 inlined blocks long, so the clients are walked by a ROLLED loop and not kPrepCohortGroup at a time: two
// bodies would not leave the registers of the streaming budget, and three (a group and the remainder) would not fit the instruction cache.
// A row's last fewer-than-four elements, an element with pads and every element of a run-time bs (BS = 0) walk value by value with
// RunWalk: the current block is kept and a new one computed only when its words run out.
// It shares no body with quantize_batch_combine_cohort_kernel: that one's lane owns ONE element (its draws are a load), and giving it
// the groups of four would change the code the buffer form runs.
template <class E> __device__ __forceinline__ E prep_shl(E x, int s) { return s >= static_cast<int>(8 * sizeof(E)) ? static_cast<E>(0) : x << s; }

// client c over the four whole elements e0 .. e0 + 3 of row `row`: the row's values j0 .. j0 + 4 BS - 1 (vstart = the row's first flat value)
template <class E, int BS, bool f64>
__device__ __forceinline__ void prep_batch_group4(const PrepCohort &pc, const ClientPlan *__restrict__ plans, int row, double p0, double p1, double p2,
                                                  uint64_t vstart, uint64_t j0, int c, uint64_t e0, E modmask, E (&sum)[4])
{
    __asm__ volatile("" ::: "memory");                // (one client's plan in scalar registers at a time)
    const ClientPlan &p = plans[c];
    const uint64_t key[2] = {p.key[0], p.key[1]}, base[4] = {p.base[0], p.base[1], p.base[2], p.base[3]};
    const void *xs = pc.src[static_cast<size_t>(c) * pc.n_layers + row];
    E mk[4];
    uint64_t raw[4];
    prep_src4(xs, f64, j0, raw);
    flashe_philox::RunBlocks rb;
    rb.start(key, base, p.skip, vstart + j0);
    E x = 0;                                          // the element being packed: one at a time, masked, stored and summed when its last value is in
#pragma unroll
    for (int i = 0; i < BS; i++) {
        uint64_t ahead[4] = {0, 0, 0, 0};
        double d[4];
        if (i + 1 < BS) prep_src4(xs, f64, j0 + 4 * (i + 1), ahead);
#pragma unroll
        for (int t = 0; t < 4; t++)
            if ((4 * i + t) % BS == 0) mk[(4 * i + t) / BS] = prep_ld<E>(pc.mask[c], e0 + (4 * i + t) / BS);      // (an element's mask: asked for a block before it is used)
        __asm__ volatile("" ::: "memory");            // (the later runs are not requested before this block: they would all be live at once)
        rb.step(key, i == 0, d);
        uint64_t q[4];
#pragma unroll
        for (int t = 0; t < 4; t++) q[t] = cohort_quantize_raw(raw[t], f64, p0, p1, p2, d[t]);
        // (the next block's counter is made to wait for these four: left to itself the scheduler computes all the blocks first, while the
        // floats arrive, and keeps every block's words)
        __asm__ volatile("" : "+v"(q[0]), "+v"(q[1]), "+v"(q[2]), "+v"(q[3]), "+v"(rb.at[0]));
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int m = 4 * i + t;                                                                    // value m of the group: slot m % BS of element m / BS
            x = (x << pc.field_bits) + static_cast<E>(q[t]);                                            // temp *= mod; temp += value
            if (m % BS == BS - 1) {
                const E v = (x + mk[m / BS]) & modmask;
                prep_st<E>(pc.ct[c], e0 + m / BS, v);
                sum[m / BS] += v;
                x = 0;
            }
            raw[t] = ahead[t];
        }
    }
}

// client c over the ne <= 4 elements from e0 on, value by value: the row's values from j0 on, those at or past `size` are pads
template <class E>
__device__ __forceinline__ void prep_batch_group_walk(const PrepCohort &pc, const ClientPlan *__restrict__ plans, int row, bool f64, double p0, double p1, double p2,
                                                      uint64_t vstart, uint64_t j0, uint64_t size, int bs, int ne, int c, uint64_t e0, E modmask, E (&sum)[4])
{
    __asm__ volatile("" ::: "memory");
    const ClientPlan &p = plans[c];
    const uint64_t key[2] = {p.key[0], p.key[1]}, base[4] = {p.base[0], p.base[1], p.base[2], p.base[3]};
    const void *xs = pc.src[static_cast<size_t>(c) * pc.n_layers + row];
    flashe_philox::RunWalk rw;
    rw.start(key, base, p.skip, vstart + j0);     // (j0 < size: the group's first element holds a value)
    uint64_t j = j0;
#pragma unroll
    for (int t = 0; t < 4; t++) {
        if (t < ne) {
            E x = 0;
#pragma unroll 1
            for (int i = 0; i < bs; i++, j++) {
                uint64_t q = 0;
                if (j < size) q = cohort_quantize_raw(cohort_load(xs, f64, j), f64, p0, p1, p2, rw.next(key));
                x = prep_shl<E>(x, pc.field_bits) + static_cast<E>(q);
            }
            const E v = (x + prep_ld<E>(pc.mask[c], e0 + t)) & modmask;
            prep_st<E>(pc.ct[c], e0 + t, v);
            sum[t] += v;
        }
    }
}

template <class E, int BS>
__global__ __launch_bounds__(kStreamThreads) void quantize_batch_philox_combine_cohort_kernel(const PrepCohort pc, const ClientPlan *__restrict__ plans,
                                                                                              const uint64_t *__restrict__ groups, uint64_t n_groups, E modmask)
{
    const int C = pc.n_clients, bs = BS ? BS : pc.bs;
    for (uint64_t g = static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x; g < n_groups; g += static_cast<uint64_t>(gridDim.x) * kStreamThreads) {
        int lo = 0, hi = pc.n_layers - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (groups[mid] <= g) lo = mid; else hi = mid - 1;
        }
        const CodecLayer *L = pc.layers + lo;
        const bool f64 = L->x_is_f64 != 0;
        const double p0 = L->p0, p1 = L->p1, p2 = L->p2;
        const uint64_t vstart = L->start, size = pc.rows[2 * lo + 1], first = 4 * (g - groups[lo]);       // first: the group's first element of the row
        const uint64_t e0 = pc.rows[2 * lo] + first, j0 = first * static_cast<uint64_t>(bs);
        E sum[4] = {0, 0, 0, 0};
        int c = 0;
        if (BS != 0 && j0 + 4 * static_cast<uint64_t>(BS) <= size) {
            if constexpr (BS != 0) {
                // (the row's float type picks the body: its rounding is not decided value by value)
                if (f64) {
#pragma unroll 1
                    for (; c < C; c++) prep_batch_group4<E, BS, true>(pc, plans, lo, p0, p1, p2, vstart, j0, c, e0, modmask, sum);
                } else {
#pragma unroll 1
                    for (; c < C; c++) prep_batch_group4<E, BS, false>(pc, plans, lo, p0, p1, p2, vstart, j0, c, e0, modmask, sum);
                }
            }
            if (pc.sum) {
#pragma unroll
                for (int t = 0; t < 4; t++) sum[t] &= modmask;
                prep_st4(pc.sum, e0, sum);
            }
            continue;
        }
        const uint64_t left = (size - j0 + static_cast<uint64_t>(bs) - 1) / static_cast<uint64_t>(bs);     // the row's elements from e0 on, >= 1
        const int ne = left < 4 ? static_cast<int>(left) : 4;
#pragma unroll 1
        for (; c < C; c++) prep_batch_group_walk<E>(pc, plans, lo, f64, p0, p1, p2, vstart, j0, size, bs, ne, c, e0, modmask, sum);
        if (pc.sum) {
#pragma unroll
            for (int t = 0; t < 4; t++)
                if (t < ne) prep_st<E>(pc.sum, e0 + t, sum[t] & modmask);
        }
    }
}

// ---- the one launcher of the kernels above (kernels.h: PrepDraws says where the draws come from) ----
int prep_pcg64_grid(const LaunchEnv &env, uint64_t n) { return stream_grid(env, (n + 3) / 4); }

// f(modmask): the vectors' element type -- uint32_t, uint64_t or u128, by elem_bytes and the ctx's int_bits -- and its mask of env.b bits
template <class F> static hipError_t prep_with_elem(const LaunchEnv &env, int elem_bytes, F &&f)
{
    uint64_t lo, hi;
    masks_of(env.b, &lo, &hi);
    if (elem_bytes == 4) return env.b > 32 ? hipErrorInvalidValue : f(static_cast<uint32_t>(lo));
    if (elem_bytes == 8) return env.b > 64 ? hipErrorInvalidValue : f(lo);
    if (elem_bytes == 16) return env.b <= 64 ? hipErrorInvalidValue : f((static_cast<u128>(hi) << 64) | lo);
    return hipErrorInvalidValue;
}

// f(BS): the batched kernels' compiled-in values per element, 5 / 6 / 7, or 0 for any other bs (read from pc.bs)
template <class F> static void prep_with_bs(int bs, F &&f)
{
    if (bs == 5) f(std::integral_constant<int, 5>{});
    else if (bs == 6) f(std::integral_constant<int, 6>{});
    else if (bs == 7) f(std::integral_constant<int, 7>{});
    else f(std::integral_constant<int, 0>{});
}

// the buffer form with G clients per group (there is no batched job on uint32 vectors)
template <class E, int G> static hipError_t prep_launch_buffer(const LaunchEnv &env, const PrepCohort &pc, bool batched, E modmask)
{
    const dim3 g(stream_grid(env, batched ? pc.n : (pc.n + 3) / 4)), t(kStreamThreads);
    if (!batched) hipLaunchKernelGGL((quantize_combine_cohort_kernel<E, G>), g, t, 0, env.stream, pc, modmask);
    else if constexpr (sizeof(E) == 4) return hipErrorInvalidValue;
    else prep_with_bs(pc.bs, [&](auto bs) { hipLaunchKernelGGL((quantize_batch_combine_cohort_kernel<E, G, decltype(bs)::value>), g, t, 0, env.stream, pc, modmask); });
    return hipGetLastError();
}

hipError_t launch_prep_cohort(const LaunchEnv &env, const PrepCohort &pc, const PrepDraws &draws, int elem_bytes)
{
    const bool drawn = draws.kind != PrepDraws::kBuffer, grouped = drawn && draws.batched;       // grouped: a lane owns a group of four elements
    if (pc.n == 0 || pc.n_clients == 0 || (grouped && draws.n_groups == 0)) return hipSuccess;
    if (pc.n_layers < 1 || (drawn && !draws.plans) || (grouped && !draws.groups)) return hipErrorInvalidValue;
    if (draws.batched && (elem_bytes == 4 || draws.kind == PrepDraws::kPcg64 || pc.bs < 1 || pc.field_bits < 1 || pc.field_bits > env.b)) return hipErrorInvalidValue;
    const dim3 t(kStreamThreads);
    if (!drawn) {
        int group = kPrepCohortGroup;
        if (const char *e = FLASHE_TUNE_ENV("FLASHE_PREP_COHORT_GROUP")) group = atoi(e);      // (read per call: an in-process A/B alternates it)
        return prep_with_elem(env, elem_bytes, [&](auto modmask) {
            using E = decltype(modmask);
#ifdef FLASHE_TUNING
            if (group == 1) return prep_launch_buffer<E, 1>(env, pc, draws.batched, modmask);      // (the alternatives of the A/B ride in the tuning build only)
            if (group == 4) return prep_launch_buffer<E, 4>(env, pc, draws.batched, modmask);
#endif
            (void)group;
            return prep_launch_buffer<E, kPrepCohortGroup>(env, pc, draws.batched, modmask);
        });
    }
    if (draws.kind == PrepDraws::kPhilox && !draws.batched)
        return prep_with_elem(env, elem_bytes, [&](auto modmask) {
            hipLaunchKernelGGL((quantize_philox_combine_cohort_kernel<decltype(modmask), kPrepCohortGroup>), dim3(stream_grid(env, (pc.n + 3) / 4)), t, 0, env.stream, pc,
                               static_cast<const ClientPlan *>(draws.plans), modmask);
            return hipGetLastError();
        });
    if (draws.kind == PrepDraws::kPcg64) {
        if (draws.variant >= flashe_pcg64::kVariants) return hipErrorInvalidValue;
        const flashe_pcg64::ClientPlan *plans = static_cast<const flashe_pcg64::ClientPlan *>(draws.plans);
        const int workgroups = prep_pcg64_grid(env, pc.n);
        const flashe_pcg64::Row stride = flashe_pcg64::to_row(flashe_pcg64::stride_jump(static_cast<flashe_pcg64::Variant>(draws.variant), static_cast<uint64_t>(workgroups)));
        return prep_with_elem(env, elem_bytes, [&](auto modmask) {
            using E = decltype(modmask);
            if (draws.variant == flashe_pcg64::kPcg64)
                hipLaunchKernelGGL((quantize_pcg64_combine_cohort_kernel<E, kPrepCohortGroup, flashe_pcg64::kPcg64>), dim3(workgroups), t, 0, env.stream, pc, plans, stride, modmask);
            else
                hipLaunchKernelGGL((quantize_pcg64_combine_cohort_kernel<E, kPrepCohortGroup, flashe_pcg64::kDxsm>), dim3(workgroups), t, 0, env.stream, pc, plans, stride, modmask);
            return hipGetLastError();
        });
    }
    // the batched job drawing its Philox streams
    return prep_with_elem(env, elem_bytes, [&](auto modmask) {
        using E = decltype(modmask);
        if constexpr (sizeof(E) != 4)
            prep_with_bs(pc.bs, [&](auto bs) {
                hipLaunchKernelGGL((quantize_batch_philox_combine_cohort_kernel<E, decltype(bs)::value>), dim3(stream_grid(env, draws.n_groups)), t, 0, env.stream, pc,
                                   static_cast<const ClientPlan *>(draws.plans), draws.groups, draws.n_groups, modmask);
            });
        return hipGetLastError();
    });
}

hipError_t launch_batch(const LaunchEnv &env, uint64_t n, const uint64_t *vals_dev, int field_bits, uint64_t *out_dev)
{
    const int bs = env.b / field_bits;
    const uint64_t nb = (n + bs - 1) / bs;
    if (nb == 0) return hipSuccess;
    hipLaunchKernelGGL(batch_kernel, dim3(stream_grid(env, nb)), dim3(kStreamThreads), 0, env.stream, n, nb, vals_dev,
                       env.b > 64 ? 2 : 1, bs, field_bits, out_dev);
    return hipGetLastError();
}

hipError_t launch_unbatch(const LaunchEnv &env, uint64_t nb, const uint64_t *in_dev, int field_bits, uint64_t *out_dev)
{
    if (nb == 0) return hipSuccess;
    hipLaunchKernelGGL(unbatch_kernel, dim3(stream_grid(env, nb)), dim3(kStreamThreads), 0, env.stream, nb, in_dev,
                       env.b > 64 ? 2 : 1, env.b / field_bits, field_bits, out_dev);
    return hipGetLastError();
}

}  // namespace flashe
