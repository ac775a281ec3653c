// gfx950 kernels either side of the fused codec for caller-owned tensors (flashe_quantize_encrypt_tensors_dev,
// flashe_quantize_batch_tensors_dev, flashe_store_layers_dev): the front end that turns float16 / bfloat16 / float32 / float64 layers
// (optionally normalised) into the compute type the codec reads, the back end that writes the unquantised float64 values into the
// caller's tensors in their own dtype, and NumPy's blocked pairwise summation of every layer for unnormalize's statistics.
// All three are HBM-bound streaming passes; the layer tables are small device arrays staged per call.  Beside them, the two passes that
// carry the aggregator's degree scaling (flashe_stage_layers_dev, flashe_finish_layers_dev; jzf_aggregator.py:676, :902-907).
#include "device_common.h"

namespace flashe {

namespace {

template <class Tab>
__device__ __forceinline__ int layer_by(const Tab *tab, int n, uint64_t key, uint64_t Tab::*field)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid].*field <= key) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ float bf16_to_f32(uint16_t h) { return __builtin_bit_cast(float, static_cast<uint32_t>(h) << 16); }
__device__ __forceinline__ float f16_to_f32(uint16_t h) { return static_cast<float>(__builtin_bit_cast(_Float16, h)); }
// the hardware converts (round to nearest even; a NaN stays a NaN): v_cvt_f16_f32 / v_cvt_pk_bf16_f32
__device__ __forceinline__ uint16_t f32_to_f16(float f) { return __builtin_bit_cast(uint16_t, static_cast<_Float16>(f)); }
__device__ __forceinline__ uint16_t f32_to_bf16(float f) { return __builtin_bit_cast(uint16_t, static_cast<__bf16>(f)); }

}  // namespace

// ---- front end: one value per lane, grid-stride over the staged values of all layers ----
__global__ __launch_bounds__(kStreamThreads) void stage_layers_kernel(const TensorStage *__restrict__ tab, int n_tab, uint64_t total)
{
#pragma clang fp contract(off)
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x; j < total; j += static_cast<uint64_t>(gridDim.x) * kStreamThreads) {
        const TensorStage &L = tab[layer_by(tab, n_tab, j, &TensorStage::start)];
        const uint64_t k = j - L.start;
        if (L.dtype == kTensorF64) {
            double x = static_cast<const double *>(L.src)[k];
            if (L.flags & kTensorShift) x = x + L.shift;
            static_cast<double *>(L.dst)[k] = x;
            continue;
        }
        float x;                                                        // 1. exact upcast of a 16-bit value
        if (L.dtype == kTensorF32) x = static_cast<const float *>(L.src)[k];
        else if (L.dtype == kTensorF16) x = f16_to_f32(static_cast<const uint16_t *>(L.src)[k]);
        else x = bf16_to_f32(static_cast<const uint16_t *>(L.src)[k]);
        if (L.flags & kTensorShift)                                     // 2. normalise in float32 (shift_kernel's arithmetic)
            x = (L.flags & kTensorShiftWide) ? static_cast<float>(static_cast<double>(x) + L.shift) : x + static_cast<float>(L.shift);
        if (L.flags & kTensorLoopF64) static_cast<double *>(L.dst)[k] = static_cast<double>(x);   // 3. exact widening
        else static_cast<float *>(L.dst)[k] = x;
    }
}

hipError_t launch_stage_layers(const LaunchEnv &env, const TensorStage *tab_dev, int n_tab, uint64_t total)
{
    if (total == 0 || n_tab < 1) return hipSuccess;
    hipLaunchKernelGGL(stage_layers_kernel, dim3(stream_grid(env, total)), dim3(kStreamThreads), 0, env.stream, tab_dev, n_tab, total);
    return hipGetLastError();
}

// ---- the sparse job's front end for a cohort: C clients' compact layers -> C plaintext vectors in one launch ----
// What Client.secure_aggregate does to the compact layers Client.sparsify kept (jzf_aggregator.py:717-743: quantize, flatten, strip the
// quantised 'zzz' value, encrypt, re-append it) starts with QuantizingClient.quantize (jzf_quantize.py:433-465) per client.  Here: a
// workgroup owns a 1024-value tile of ONE client's compact vector (blockIdx.y = the client), finds the tile's table row once with
// scalar loads and keeps the row's alpha / scale / den / shift in SGPRs; a lane takes four consecutive values -- one 16-byte load of
// float32 values, two of the draws, two 16-byte stores of the plaintexts where the pointers allow them, scalar accesses at row ends and
// on odd alignments -- and normalises (stage_layers_kernel's rule) and quantises (quantize_one) in registers.  Only a tile that
// straddles a row boundary (at most one per row) looks the row up per value.  The extra workgroup blockIdx.x == n_tiles quantises the
// client's trailing 'zzz' value (alpha 1.0, :433-435) with the draw behind the client's n.
constexpr int kQcThreads = 256;
constexpr uint64_t kQcTile = 4 * kQcThreads;

struct QcRowRegs {             // one row's parameters and one client's source of it
    const void *x;
    uint64_t start;
    double alpha, scale, den, shift;
    int dtype, flags, loop64;
};

__device__ __forceinline__ uint64_t qc_quantize(const QcRowRegs &R, uint64_t r, double u)
{
#pragma clang fp contract(off)
    if (R.dtype == kTensorF64) {
        double x = static_cast<const double *>(R.x)[r];
        if (R.flags & kTensorShift) x = x + R.shift;
        return quantize_one<double>(x, R.alpha, R.scale, R.den, u);
    }
    float x;
    if (R.dtype == kTensorF32) x = static_cast<const float *>(R.x)[r];
    else if (R.dtype == kTensorF16) x = f16_to_f32(static_cast<const uint16_t *>(R.x)[r]);
    else x = bf16_to_f32(static_cast<const uint16_t *>(R.x)[r]);
    if (R.flags & kTensorShift)
        x = (R.flags & kTensorShiftWide) ? static_cast<float>(static_cast<double>(x) + R.shift) : x + static_cast<float>(R.shift);
    return R.loop64 ? quantize_one<double>(static_cast<double>(x), R.alpha, R.scale, R.den, u)
                    : quantize_one<float>(x, static_cast<float>(R.alpha), static_cast<float>(R.scale), static_cast<float>(R.den), u);
}

// the same on a float32 value already in a register (the vector path of float32 sources)
__device__ __forceinline__ uint64_t qc_quantize_f32(const QcRowRegs &R, float x, double u)
{
#pragma clang fp contract(off)
    if (R.flags & kTensorShift)
        x = (R.flags & kTensorShiftWide) ? static_cast<float>(static_cast<double>(x) + R.shift) : x + static_cast<float>(R.shift);
    return R.loop64 ? quantize_one<double>(static_cast<double>(x), R.alpha, R.scale, R.den, u)
                    : quantize_one<float>(x, static_cast<float>(R.alpha), static_cast<float>(R.scale), static_cast<float>(R.den), u);
}

__global__ __launch_bounds__(kQcThreads) void quantize_cohort_kernel(const QuantCohort qc, uint64_t n, const double *__restrict__ u_all, uint64_t u_stride,
                                                                     uint32_t n_tiles)
{
#pragma clang fp contract(off)
    const uint32_t c = blockIdx.y;
    const double *u = u_all + static_cast<uint64_t>(c) * u_stride;
    if (blockIdx.x >= n_tiles) {                                      // the trailing value: not encrypted, element n of the upload
        if (threadIdx.x == 0) {
            const double v = qc.zzz[c];
            const uint64_t q = qc.zrow.loop_f64 ? quantize_one<double>(v, qc.zrow.alpha, qc.zrow.scale, qc.zrow.den, u[n])
                                                : quantize_one<float>(static_cast<float>(v), static_cast<float>(qc.zrow.alpha),
                                                                      static_cast<float>(qc.zrow.scale), static_cast<float>(qc.zrow.den), u[n]);
            qc.zeros[c] = q;
            uint64_t *t = qc.tail[c];
            if (t) {
                t[0] = q;
                if (qc.tail_limbs == 2) t[1] = 0;
            }
        }
        return;
    }
    const uint64_t t0 = static_cast<uint64_t>(blockIdx.x) * kQcTile;
    const uint64_t t1 = t0 + kQcTile < n ? t0 + kQcTile : n;
    uint64_t *pt = reinterpret_cast<uint64_t *>(*FLASHE_CONSTANT(const uint64_t, reinterpret_cast<const uint64_t *>(qc.pt) + c));
    const uint64_t j0 = t0 + 4u * threadIdx.x;
    // the tile's first row, with scalar loads (t0 is uniform over the workgroup)
    int lo = 0, hi = qc.n_rows - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (*FLASHE_CONSTANT(const uint64_t, &qc.rows[mid].start) <= t0) lo = mid; else hi = mid - 1;
    }
    const uint64_t next = lo + 1 < qc.n_rows ? *FLASHE_CONSTANT(const uint64_t, &qc.rows[lo + 1].start) : n;
    if (next >= t1) {
        // the whole tile lies in row `lo`: its parameters and the client's source pointer are wave-uniform
        const QuantCohortRow *row = qc.rows + lo;
        const size_t at = static_cast<size_t>(c) * qc.n_rows + lo;
        QcRowRegs R;
        R.x = reinterpret_cast<const void *>(*FLASHE_CONSTANT(const uint64_t, reinterpret_cast<const uint64_t *>(qc.src) + at));
        R.dtype = *FLASHE_CONSTANT(const int32_t, qc.src_dtype + at);
        R.start = *FLASHE_CONSTANT(const uint64_t, &row->start);
        R.alpha = *FLASHE_CONSTANT(const double, &row->alpha);
        R.scale = *FLASHE_CONSTANT(const double, &row->scale);
        R.den = *FLASHE_CONSTANT(const double, &row->den);
        R.shift = *FLASHE_CONSTANT(const double, &row->shift);
        R.flags = *FLASHE_CONSTANT(const int32_t, &row->flags);
        R.loop64 = *FLASHE_CONSTANT(const int32_t, &row->loop_f64);
        if (j0 >= t1) return;
        const uint64_t r = j0 - R.start;
        if (j0 + 4 > t1) {                                            // the vector's last lane
            for (uint64_t j = j0; j < t1; j++) pt[j] = qc_quantize(R, j - R.start, u[j]);
            return;
        }
        double uu[4];
        if ((reinterpret_cast<uintptr_t>(u + j0) & 15u) == 0) {
            const double2 a = *reinterpret_cast<const double2 *>(u + j0), b = *reinterpret_cast<const double2 *>(u + j0 + 2);
            uu[0] = a.x; uu[1] = a.y; uu[2] = b.x; uu[3] = b.y;
        } else {
#pragma unroll
            for (int t = 0; t < 4; t++) uu[t] = u[j0 + t];
        }
        uint64_t q[4];
        if (R.dtype == kTensorF32 && (reinterpret_cast<uintptr_t>(static_cast<const float *>(R.x) + r) & 15u) == 0) {
            const float4 v = *reinterpret_cast<const float4 *>(static_cast<const float *>(R.x) + r);
            q[0] = qc_quantize_f32(R, v.x, uu[0]); q[1] = qc_quantize_f32(R, v.y, uu[1]);
            q[2] = qc_quantize_f32(R, v.z, uu[2]); q[3] = qc_quantize_f32(R, v.w, uu[3]);
        } else {
#pragma unroll
            for (int t = 0; t < 4; t++) q[t] = qc_quantize(R, r + t, uu[t]);
        }
        if ((reinterpret_cast<uintptr_t>(pt + j0) & 15u) == 0) {
            *reinterpret_cast<ulonglong2 *>(pt + j0) = make_ulonglong2(q[0], q[1]);
            *reinterpret_cast<ulonglong2 *>(pt + j0 + 2) = make_ulonglong2(q[2], q[3]);
        } else {
#pragma unroll
            for (int t = 0; t < 4; t++) pt[j0 + t] = q[t];
        }
        return;
    }
    // a tile that straddles a row boundary: every value finds its own row (the search starts at the tile's first row)
    for (uint64_t j = j0; j < j0 + 4 && j < t1; j++) {
        int a = lo, b = qc.n_rows - 1;
        while (a < b) {
            const int mid = (a + b + 1) >> 1;
            if (qc.rows[mid].start <= j) a = mid; else b = mid - 1;
        }
        const QuantCohortRow &row = qc.rows[a];
        const size_t at = static_cast<size_t>(c) * qc.n_rows + a;
        const QcRowRegs R{qc.src[at], row.start, row.alpha, row.scale, row.den, row.shift, qc.src_dtype[at], row.flags, row.loop_f64};
        pt[j] = qc_quantize(R, j - row.start, u[j]);
    }
}

hipError_t launch_quantize_cohort(const LaunchEnv &env, const QuantCohort &qc, uint64_t n, const double *u_dev, uint64_t u_stride)
{
    if (qc.n_clients < 1 || qc.n_clients > 65535 || (n && qc.n_rows < 1)) return hipErrorInvalidValue;
    const uint64_t tiles = (n + kQcTile - 1) / kQcTile;
    if (tiles >= (1ull << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(quantize_cohort_kernel, dim3(static_cast<unsigned>(tiles) + 1u, static_cast<unsigned>(qc.n_clients)), dim3(kQcThreads), 0, env.stream,
                       qc, n, u_dev, u_stride, static_cast<uint32_t>(tiles));
    return hipGetLastError();
}

// ---- back end: eight values of one layer per lane; 16-byte stores where the layer's pointer allows them ----
__global__ __launch_bounds__(kStreamThreads) void store_layers_kernel(const TensorStore *__restrict__ tab, int n_tab, uint64_t n_groups,
                                                                      const double *__restrict__ in)
{
#pragma clang fp contract(off)
    for (uint64_t g = static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x; g < n_groups; g += static_cast<uint64_t>(gridDim.x) * kStreamThreads) {
        const TensorStore &L = tab[layer_by(tab, n_tab, g, &TensorStore::group_start)];
        const uint64_t j0 = (g - L.group_start) * 8;
        const int cnt = L.size - j0 < 8 ? static_cast<int>(L.size - j0) : 8;
        double y[8];
#pragma unroll
        for (int t = 0; t < 8; t++) {
            y[t] = t < cnt ? in[L.start + j0 + t] : 0.0;
            if (L.flags & kTensorShift) y[t] = y[t] + L.shift;
        }
        const bool vec = cnt == 8 && (reinterpret_cast<uintptr_t>(L.dst) & 15u) == 0;
        if (L.dtype == kTensorF64) {
            double *d = static_cast<double *>(L.dst) + j0;
            if (vec) {
#pragma unroll
                for (int t = 0; t < 8; t += 2) *reinterpret_cast<double2 *>(d + t) = make_double2(y[t], y[t + 1]);
            } else {
                for (int t = 0; t < cnt; t++) d[t] = y[t];
            }
        } else if (L.dtype == kTensorF32) {
            float *d = static_cast<float *>(L.dst) + j0;
            if (vec) {
#pragma unroll
                for (int t = 0; t < 8; t += 4)
                    *reinterpret_cast<float4 *>(d + t) = make_float4(static_cast<float>(y[t]), static_cast<float>(y[t + 1]), static_cast<float>(y[t + 2]),
                                                                     static_cast<float>(y[t + 3]));
            } else {
                for (int t = 0; t < cnt; t++) d[t] = static_cast<float>(y[t]);
            }
        } else {
            // f64 -> f32 -> 16 bits, each step round to nearest even (what torch's .to(float16 / bfloat16) of a float64 tensor does)
            uint16_t h[8];
#pragma unroll
            for (int t = 0; t < 8; t++) {
                const float f = static_cast<float>(y[t]);
                h[t] = L.dtype == kTensorF16 ? f32_to_f16(f) : f32_to_bf16(f);
            }
            uint16_t *d = static_cast<uint16_t *>(L.dst) + j0;
            if (vec) {
                uint4 w;
                w.x = h[0] | (static_cast<uint32_t>(h[1]) << 16); w.y = h[2] | (static_cast<uint32_t>(h[3]) << 16);
                w.z = h[4] | (static_cast<uint32_t>(h[5]) << 16); w.w = h[6] | (static_cast<uint32_t>(h[7]) << 16);
                *reinterpret_cast<uint4 *>(d) = w;
            } else {
                for (int t = 0; t < cnt; t++) d[t] = h[t];
            }
        }
    }
}

hipError_t launch_store_layers(const LaunchEnv &env, const TensorStore *tab_dev, int n_tab, uint64_t n_groups, const double *in_dev)
{
    if (n_groups == 0 || n_tab < 1) return hipSuccess;
    hipLaunchKernelGGL(store_layers_kernel, dim3(stream_grid(env, n_groups)), dim3(kStreamThreads), 0, env.stream, tab_dev, n_tab, n_groups, in_dev);
    return hipGetLastError();
}

// ---- NumPy's np.sum of a C-contiguous float64 array, bit for bit ----
// The reduction runs over buffers of `block` (np.getbufsize()) values, added left to right to an accumulator that starts at 0.0; each
// buffer is summed by the pairwise tree of NumPy's loops: n < 8 sequential from 0.0; n <= 128 eight strided accumulators combined as
// ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)) plus the tail in order; otherwise split at n2 = n / 2 - (n / 2) % 8.  One wave per
// buffer: lane 0 lists the leaves of the tree in order (LDS), the lanes sum the leaves, lane 0 combines them in the tree's order.
// pass 0 sums y = x (+ shift); pass 1 sums (y - mean)^2 with the layer's mean from pass 0.
constexpr int kStatThreads = 64;
constexpr int kStatMaxLeaves = 512;        // enough for buffers of up to 16,384 values (every leaf of a split tree holds > 56)
constexpr int kStatMaxDepth = 32;

// y of a table row: what the row's store pass stores before its cast (StatLayer: in (+ shift))
__device__ __forceinline__ double stat_value(const StatLayer &L, double x)
{
#pragma clang fp contract(off)
    if (L.flags & kTensorShift) x = x + L.shift;
    return x;
}

// y2 of jzf_aggregator.py:902-904 (FinishStat / FinishRow: in / div_total + shift), the value unnormalize's statistics see
__device__ __forceinline__ double finish_y2(double x, int flags, double div_total, double shift)
{
#pragma clang fp contract(off)
    if (flags & kFinishDivTotal) x = x / div_total;
    if (flags & kFinishShift) x = x + shift;
    return x;
}

__device__ __forceinline__ double stat_value(const FinishStat &L, double x) { return finish_y2(x, L.flags, L.div_total, L.shift); }

template <class Tab>
__device__ __forceinline__ void stat_blocks_body(const Tab *__restrict__ tab, int n_tab, uint64_t n_blocks, const double *__restrict__ in, uint64_t block,
                                                 int pass, const double *__restrict__ means, double *__restrict__ bsum)
{
#pragma clang fp contract(off)
    __shared__ uint32_t leaf_off[kStatMaxLeaves];
    __shared__ uint32_t leaf_len[kStatMaxLeaves];
    __shared__ double leaf_sum[kStatMaxLeaves];
    __shared__ uint32_t st_len[kStatMaxDepth];
    __shared__ uint32_t st_off[kStatMaxDepth];
    __shared__ uint32_t st_state[kStatMaxDepth];
    __shared__ double st_left[kStatMaxDepth];
    __shared__ int n_leaves;
    for (uint64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        const int li = layer_by(tab, n_tab, b, &Tab::blk_start);
        const Tab &L = tab[li];
        const uint64_t off0 = (b - L.blk_start) * block;
        const uint32_t m = static_cast<uint32_t>(L.size - off0 < block ? L.size - off0 : block);
        const double *x = in + L.start + off0;
        const double mean = pass ? means[li] : 0.0;
        if (threadIdx.x == 0) {                                         // the leaves, left to right
            int sp = 0, nl = 0;
            st_off[0] = 0; st_len[0] = m;
            while (sp >= 0) {
                const uint32_t o = st_off[sp], len = st_len[sp];
                sp--;
                if (len <= 128) { leaf_off[nl] = o; leaf_len[nl] = len; nl++; continue; }
                uint32_t n2 = len / 2;
                n2 -= n2 % 8;
                sp++; st_off[sp] = o + n2; st_len[sp] = len - n2;         // right child below the left one
                sp++; st_off[sp] = o; st_len[sp] = n2;
            }
            n_leaves = nl;
        }
        __syncthreads();
        const int nl = n_leaves;
        for (int l = threadIdx.x; l < nl; l += kStatThreads) {
            const uint32_t o = leaf_off[l], len = leaf_len[l];
            auto val = [&](uint32_t i) {
                double y = stat_value(L, x[o + i]);
                if (pass) { const double d = y - mean; y = d * d; }
                return y;
            };
            double res;
            if (len < 8) {
                res = 0.0;
                for (uint32_t i = 0; i < len; i++) res += val(i);
            } else {
                double r0 = val(0), r1 = val(1), r2 = val(2), r3 = val(3), r4 = val(4), r5 = val(5), r6 = val(6), r7 = val(7);
                uint32_t i = 8;
                for (; i < len - (len % 8); i += 8) {
                    r0 += val(i); r1 += val(i + 1); r2 += val(i + 2); r3 += val(i + 3);
                    r4 += val(i + 4); r5 += val(i + 5); r6 += val(i + 6); r7 += val(i + 7);
                }
                res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
                for (; i < len; i++) res += val(i);
            }
            leaf_sum[l] = res;
        }
        __syncthreads();
        if (threadIdx.x == 0) {                                         // the tree, combined in its own order (post-order walk)
            int sp = 0, leaf = 0;
            st_len[0] = m; st_state[0] = 0;
            double ret = 0.0;
            bool have = false;
            while (true) {
                if (have) {
                    if (sp < 0) break;
                    if (st_state[sp] == 1) {                            // left child done: descend into the right one
                        st_left[sp] = ret;
                        st_state[sp] = 2;
                        uint32_t n2 = st_len[sp] / 2;
                        n2 -= n2 % 8;
                        const uint32_t right = st_len[sp] - n2;
                        sp++; st_len[sp] = right; st_state[sp] = 0;
                        have = false;
                    } else {                                            // both children done
                        ret = st_left[sp] + ret;
                        sp--;
                    }
                    continue;
                }
                const uint32_t len = st_len[sp];
                if (len <= 128) { ret = leaf_sum[leaf++]; sp--; have = true; continue; }
                uint32_t n2 = len / 2;
                n2 -= n2 % 8;
                st_state[sp] = 1;
                sp++; st_len[sp] = n2; st_state[sp] = 0;
            }
            bsum[b] = ret;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kStatThreads) void stat_blocks_kernel(const StatLayer *__restrict__ tab, int n_tab, uint64_t n_blocks,
                                                                   const double *__restrict__ in, uint64_t block, int pass,
                                                                   const double *__restrict__ means, double *__restrict__ bsum)
{
    stat_blocks_body(tab, n_tab, n_blocks, in, block, pass, means, bsum);
}

// one lane per layer: the buffer sums added in order from 0.0; pass 0 also leaves the layer's mean (S / n) for pass 1
template <class Tab>
__device__ __forceinline__ void stat_combine_body(const Tab *__restrict__ tab, int n_tab, const double *__restrict__ bsum, uint64_t block, int pass,
                                                  double *__restrict__ means, double *__restrict__ stats)
{
#pragma clang fp contract(off)
    const int l = blockIdx.x * kStreamThreads + threadIdx.x;
    if (l >= n_tab) return;
    const Tab &L = tab[l];
    const uint64_t nb = (L.size + block - 1) / block;
    double s = 0.0;
    for (uint64_t b = 0; b < nb; b++) s += bsum[L.blk_start + b];
    stats[2 * L.out_index + pass] = s;
    if (pass == 0) means[l] = s / static_cast<double>(L.size);
}

__global__ __launch_bounds__(kStreamThreads) void stat_combine_kernel(const StatLayer *__restrict__ tab, int n_tab, const double *__restrict__ bsum,
                                                                      uint64_t block, int pass, double *__restrict__ means, double *__restrict__ stats)
{
    stat_combine_body(tab, n_tab, bsum, block, pass, means, stats);
}

// ---- the aggregator's degree scaling either side of the step (jzf_aggregator.py:676, :902-907) ----
// Eight values of one row per lane, as store_layers_kernel: 16-byte accesses where the row's pointer allows them (a group starts a
// multiple of 16 bytes behind it), scalar ones at the row's end and on odd alignments.
namespace {

__device__ __forceinline__ bool vec_ok(const void *p, int cnt) { return cnt == 8 && (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// values [j0, j0 + cnt) of a float32 / float16 / bfloat16 row as float32 (a 16-bit value upcast exactly); the rest 0
__device__ __forceinline__ void load8_f32(const void *p, int dtype, uint64_t j0, int cnt, float x[8])
{
    if (dtype == kTensorF32) {
        const float *s = static_cast<const float *>(p) + j0;
        if (vec_ok(p, cnt)) {
            const float4 a = *reinterpret_cast<const float4 *>(s), b = *reinterpret_cast<const float4 *>(s + 4);
            x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
        } else {
#pragma unroll
            for (int t = 0; t < 8; t++) x[t] = t < cnt ? s[t] : 0.0f;
        }
        return;
    }
    const uint16_t *s = static_cast<const uint16_t *>(p) + j0;
    uint16_t h[8];
    if (vec_ok(p, cnt)) {
        const uint4 w = *reinterpret_cast<const uint4 *>(s);
        h[0] = static_cast<uint16_t>(w.x); h[1] = static_cast<uint16_t>(w.x >> 16); h[2] = static_cast<uint16_t>(w.y); h[3] = static_cast<uint16_t>(w.y >> 16);
        h[4] = static_cast<uint16_t>(w.z); h[5] = static_cast<uint16_t>(w.z >> 16); h[6] = static_cast<uint16_t>(w.w); h[7] = static_cast<uint16_t>(w.w >> 16);
    } else {
#pragma unroll
        for (int t = 0; t < 8; t++) h[t] = t < cnt ? s[t] : static_cast<uint16_t>(0);
    }
#pragma unroll
    for (int t = 0; t < 8; t++) x[t] = dtype == kTensorF16 ? f16_to_f32(h[t]) : bf16_to_f32(h[t]);
}

__device__ __forceinline__ void load8_f64(const void *p, uint64_t j0, int cnt, double x[8])
{
    const double *s = static_cast<const double *>(p) + j0;
    if (vec_ok(p, cnt)) {
#pragma unroll
        for (int t = 0; t < 8; t += 2) {
            const double2 a = *reinterpret_cast<const double2 *>(s + t);
            x[t] = a.x; x[t + 1] = a.y;
        }
    } else {
#pragma unroll
        for (int t = 0; t < 8; t++) x[t] = t < cnt ? s[t] : 0.0;
    }
}

// y[0 .. cnt) into values [j0, j0 + cnt) of a row stored as dtype: float64 -> float32 -> 16 bits, each step round to nearest even
// (store_layers_kernel's stores)
__device__ __forceinline__ void store8(void *p, int dtype, uint64_t j0, int cnt, const double y[8])
{
    const bool vec = vec_ok(p, cnt);
    if (dtype == kTensorF64) {
        double *d = static_cast<double *>(p) + j0;
        if (vec) {
#pragma unroll
            for (int t = 0; t < 8; t += 2) *reinterpret_cast<double2 *>(d + t) = make_double2(y[t], y[t + 1]);
        } else {
            for (int t = 0; t < cnt; t++) d[t] = y[t];
        }
    } else if (dtype == kTensorF32) {
        float *d = static_cast<float *>(p) + j0;
        if (vec) {
#pragma unroll
            for (int t = 0; t < 8; t += 4)
                *reinterpret_cast<float4 *>(d + t) = make_float4(static_cast<float>(y[t]), static_cast<float>(y[t + 1]), static_cast<float>(y[t + 2]),
                                                                 static_cast<float>(y[t + 3]));
        } else {
            for (int t = 0; t < cnt; t++) d[t] = static_cast<float>(y[t]);
        }
    } else {
        uint16_t h[8];
#pragma unroll
        for (int t = 0; t < 8; t++) {
            float f = static_cast<float>(y[t]);
            // two roundings, as torch's .to() of a float64 tensor: behind a division the compiler otherwise folds the pair into ONE
            // float64 -> float16 conversion, which differs wherever the float32 value is a tie of the 16-bit format
            asm volatile("" : "+v"(f));
            h[t] = dtype == kTensorF16 ? f32_to_f16(f) : f32_to_bf16(f);
        }
        uint16_t *d = static_cast<uint16_t *>(p) + j0;
        if (vec) {
            uint4 w;
            w.x = h[0] | (static_cast<uint32_t>(h[1]) << 16); w.y = h[2] | (static_cast<uint32_t>(h[3]) << 16);
            w.z = h[4] | (static_cast<uint32_t>(h[5]) << 16); w.w = h[6] | (static_cast<uint32_t>(h[7]) << 16);
            *reinterpret_cast<uint4 *>(d) = w;
        } else {
            for (int t = 0; t < cnt; t++) d[t] = h[t];
        }
    }
}

// One float32 value through `weights *= degree` and normalize, in the types NumPy gives the layer: float32 * float32(scale), or -- WIDE,
// an np.float64 degree -- float64 from there on; the shift by stage_layers_kernel's rule.  A float32 result widens exactly.
__device__ __forceinline__ double stage_value(const StageRow &L, float x)
{
#pragma clang fp contract(off)
    if (L.flags & kStageScaleWide) {
        double d = static_cast<double>(x) * L.scale;
        if (L.flags & kStageShift) d = d + L.shift;
        return d;
    }
    if (L.flags & kStageScale) x = x * static_cast<float>(L.scale);
    if (L.flags & kStageShift)
        x = (L.flags & kStageShiftWide) ? static_cast<float>(static_cast<double>(x) + L.shift) : x + static_cast<float>(L.shift);
    return static_cast<double>(x);
}

__device__ __forceinline__ double stage_value(const StageRow &L, double x)
{
#pragma clang fp contract(off)
    if (L.flags & kStageScale) x = x * L.scale;
    if (L.flags & kStageShift) x = x + L.shift;
    return x;
}

}  // namespace

__global__ __launch_bounds__(kStreamThreads) void stage_rows_kernel(const StageRow *__restrict__ tab, int n_tab, uint64_t n_groups)
{
#pragma clang fp contract(off)
    for (uint64_t g = static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x; g < n_groups; g += static_cast<uint64_t>(gridDim.x) * kStreamThreads) {
        const StageRow &L = tab[layer_by(tab, n_tab, g, &StageRow::group_start)];
        const uint64_t j0 = (g - L.group_start) * 8;
        const int cnt = L.size - j0 < 8 ? static_cast<int>(L.size - j0) : 8;
        double y[8];
        if (L.dtype == kTensorF64) {
            double x[8];
            load8_f64(L.src, j0, cnt, x);
#pragma unroll
            for (int t = 0; t < 8; t++) y[t] = stage_value(L, x[t]);
        } else {
            float x[8];
            load8_f32(L.src, L.dtype, j0, cnt, x);
#pragma unroll
            for (int t = 0; t < 8; t++) y[t] = stage_value(L, x[t]);
        }
        store8(L.dst, (L.flags & kStageOutF64) ? kTensorF64 : kTensorF32, j0, cnt, y);
    }
}

hipError_t launch_stage_rows(const LaunchEnv &env, const StageRow *tab_dev, int n_tab, uint64_t n_groups)
{
    if (n_groups == 0 || n_tab < 1) return hipSuccess;
    hipLaunchKernelGGL(stage_rows_kernel, dim3(stream_grid(env, n_groups)), dim3(kStreamThreads), 0, env.stream, tab_dev, n_tab, n_groups);
    return hipGetLastError();
}

// (no __restrict__ on the rows' pointers: last may be dst, and a lane has read its eight values of last before it stores)
__global__ __launch_bounds__(kStreamThreads) void finish_layers_kernel(const FinishRow *__restrict__ tab, int n_tab, uint64_t n_groups,
                                                                       const double *__restrict__ in)
{
#pragma clang fp contract(off)
    for (uint64_t g = static_cast<uint64_t>(blockIdx.x) * kStreamThreads + threadIdx.x; g < n_groups; g += static_cast<uint64_t>(gridDim.x) * kStreamThreads) {
        const FinishRow &L = tab[layer_by(tab, n_tab, g, &FinishRow::group_start)];
        const uint64_t j0 = (g - L.group_start) * 8;
        const int cnt = L.size - j0 < 8 ? static_cast<int>(L.size - j0) : 8;
        double y[8];
#pragma unroll
        for (int t = 0; t < 8; t++) {
            y[t] = finish_y2(t < cnt ? in[L.start + j0 + t] : 0.0, L.flags, L.div_total, L.shift);
            if (L.flags & kFinishDivOwn) y[t] = y[t] / L.div_own;
        }
        if (L.flags & kFinishAddLast) {
            double w[8];                                                // last, upcast exactly (16 bits -> float32 -> float64)
            if (L.last_dtype == kTensorF64) {
                load8_f64(L.last, j0, cnt, w);
            } else {
                float f[8];
                load8_f32(L.last, L.last_dtype, j0, cnt, f);
#pragma unroll
                for (int t = 0; t < 8; t++) w[t] = static_cast<double>(f[t]);
            }
#pragma unroll
            for (int t = 0; t < 8; t++) y[t] = w[t] + y[t];
        }
        store8(L.dst, L.dtype, j0, cnt, y);
    }
}

hipError_t launch_finish_layers(const LaunchEnv &env, const FinishRow *tab_dev, int n_tab, uint64_t n_groups, const double *in_dev)
{
    if (n_groups == 0 || n_tab < 1) return hipSuccess;
    hipLaunchKernelGGL(finish_layers_kernel, dim3(stream_grid(env, n_groups)), dim3(kStreamThreads), 0, env.stream, tab_dev, n_tab, n_groups, in_dev);
    return hipGetLastError();
}

// the statistics of y2: stat_blocks_kernel's tree and combine over rows that divide before they shift
__global__ __launch_bounds__(kStatThreads) void finish_stat_blocks_kernel(const FinishStat *__restrict__ tab, int n_tab, uint64_t n_blocks,
                                                                          const double *__restrict__ in, uint64_t block, int pass,
                                                                          const double *__restrict__ means, double *__restrict__ bsum)
{
    stat_blocks_body(tab, n_tab, n_blocks, in, block, pass, means, bsum);
}

__global__ __launch_bounds__(kStreamThreads) void finish_stat_combine_kernel(const FinishStat *__restrict__ tab, int n_tab, const double *__restrict__ bsum,
                                                                             uint64_t block, int pass, double *__restrict__ means,
                                                                             double *__restrict__ stats)
{
    stat_combine_body(tab, n_tab, bsum, block, pass, means, stats);
}

hipError_t launch_finish_stats(const LaunchEnv &env, const FinishStat *tab_dev, int n_tab, uint64_t n_blocks, const double *in_dev, uint64_t block,
                               double *bsum_dev, double *means_dev, double *stats_dev)
{
    if (n_blocks == 0 || n_tab < 1) return hipSuccess;
    if (block < 1 || block > 16384) return hipErrorInvalidValue;
    const int grid = static_cast<int>(n_blocks < 65536 ? n_blocks : 65536);
    const int cgrid = (n_tab + kStreamThreads - 1) / kStreamThreads;
    for (int pass = 0; pass < 2; pass++) {
        hipLaunchKernelGGL(finish_stat_blocks_kernel, dim3(grid), dim3(kStatThreads), 0, env.stream, tab_dev, n_tab, n_blocks, in_dev, block, pass,
                           means_dev, bsum_dev);
        hipLaunchKernelGGL(finish_stat_combine_kernel, dim3(cgrid), dim3(kStreamThreads), 0, env.stream, tab_dev, n_tab, bsum_dev, block, pass, means_dev,
                           stats_dev);
    }
    return hipGetLastError();
}

hipError_t launch_layer_stats(const LaunchEnv &env, const StatLayer *tab_dev, int n_tab, uint64_t n_blocks, const double *in_dev, uint64_t block,
                              double *bsum_dev, double *means_dev, double *stats_dev)
{
    if (n_blocks == 0 || n_tab < 1) return hipSuccess;
    if (block < 1 || block > 16384) return hipErrorInvalidValue;
    const int grid = static_cast<int>(n_blocks < 65536 ? n_blocks : 65536);
    const int cgrid = (n_tab + kStreamThreads - 1) / kStreamThreads;
    for (int pass = 0; pass < 2; pass++) {
        hipLaunchKernelGGL(stat_blocks_kernel, dim3(grid), dim3(kStatThreads), 0, env.stream, tab_dev, n_tab, n_blocks, in_dev, block, pass, means_dev,
                           bsum_dev);
        hipLaunchKernelGGL(stat_combine_kernel, dim3(cgrid), dim3(kStreamThreads), 0, env.stream, tab_dev, n_tab, bsum_dev, block, pass, means_dev,
                           stats_dev);
    }
    return hipGetLastError();
}

}  // namespace flashe
