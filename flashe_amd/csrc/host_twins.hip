// Host-pointer twins of the C ABI (include/flashe.h): each stages its host arrays in device blocks leased from the ctx's StagingPool
// (ctx.h `Tmp`), calls the exported flashe_*_dev entry point and copies the results back.  Synchronous.
#include "ctx.h"

#include <algorithm>
#include <cstdlib>
#include <vector>

using flashe_host::fail;
using flashe_host::Tmp;
using flashe_host::vec_bytes;

namespace {

// A staging block as the _dev call sees it: converts to whatever pointer type the parameter has.
struct Dev {
    void *p = nullptr;
    template <class T> operator T *() const { return static_cast<T *>(p); }
};

// One host array of a twin and the device block it travels through, `copy` bytes each way: uploaded before the call (from src, or
// from n_parts arrays that land bytes / n_parts apart in the block), downloaded to dst after it, or both.  An absent operand (an
// optional array the caller left out) gets no block, and the _dev call gets null.
struct Operand {
    size_t bytes = 0, copy = 0;
    const void *src = nullptr;
    const void *const *parts = nullptr;
    int n_parts = 0;
    void *dst = nullptr;
    bool absent = false;
};
Operand up(const void *src, size_t bytes) { return Operand{bytes, bytes, src, nullptr, 1}; }
Operand down(void *dst, size_t bytes, size_t block = 0) { return Operand{block ? block : bytes, bytes, nullptr, nullptr, 0, dst}; }
Operand up_down(void *p, size_t bytes) { return Operand{bytes, bytes, p, nullptr, 1, p}; }
template <class T> Operand gather(const T *const *srcs, int n, size_t bytes, size_t stride)
{
    return Operand{stride * n, bytes, nullptr, reinterpret_cast<const void *const *>(srcs), n};
}
Operand optional(const Operand &o) { return o.src ? o : Operand{0, 0, nullptr, nullptr, 0, nullptr, true}; }
Operand unless_empty(const Operand &o) { return o.bytes ? o : Operand{0, 0, nullptr, nullptr, 0, nullptr, true}; }

// the device addresses of a gathered operand's parts
template <class T> std::vector<const T *> parts_of(const Dev &d, int n, size_t stride)
{
    std::vector<const T *> v(n);
    for (int c = 0; c < n; c++) v[c] = reinterpret_cast<const T *>(static_cast<char *>(d.p) + stride * c);
    return v;
}

// `bytes` of every part of an operand from offset `off` on, onto the ctx stream
hipError_t upload(flashe_ctx *ctx, const Operand &o, void *block, size_t off, size_t bytes)
{
    hipError_t e = hipSuccess;
    for (int p = 0; p < o.n_parts && e == hipSuccess; p++) {
        const char *src = static_cast<const char *>(o.parts ? o.parts[p] : o.src);
        e = hipMemcpyAsync(static_cast<char *>(block) + p * (o.bytes / o.n_parts) + off, src ? src + off : nullptr, bytes, hipMemcpyHostToDevice,
                           ctx->env.stream);
    }
    return e;
}

// Pipelined form of the big twins (encrypt / decrypt / aggregate_elem): the vector is cut into chunks; chunk q's upload and kernel run
// on the ctx stream while chunk q - 1's result travels back on a second stream, so a call costs max(upload, download) instead of
// their sum.  It needs a PAGE-LOCKED destination: a download into pageable memory blocks the host until it is done (measured: an H2D
// and a D2H issued on two streams take 5.96 ms with pageable buffers, 3.46 ms pinned, tests/perf/pcie_probe.py), while an upload from
// pageable memory -- blocking as well -- runs at the pinned rate and overlaps with a download that is already in flight.  So the
// path is taken when the caller's output pointer is pinned (flashe_host_alloc / hipHostMalloc / hipHostRegister; the Python layer's
// result pool hands out such arrays) and the vector is large enough for chunks to matter.
constexpr size_t kPipeMinBytes = 16u << 20;

bool host_pinned(const void *p)
{
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }      // plain malloc memory: an error, not a type
    return a.type == hipMemoryTypeHost;
}

// elements per chunk: FLASHE_TWIN_CHUNK_MB of output (default 32 MB), a multiple of 4096 elements (block- and tile-aligned for every b)
uint64_t pipe_chunk_elems(const flashe_ctx *ctx)
{
    const char *e = getenv("FLASHE_TWIN_CHUNK_MB");          // read per call: a tuning knob, and tests shrink it
    const long v = e ? atol(e) : 32;
    const size_t mb = static_cast<size_t>(v < 1 ? 1 : v);
    const uint64_t per = (mb << 20) / (static_cast<size_t>(ctx->limbs) * 8);
    return std::max<uint64_t>(4096, per & ~static_cast<uint64_t>(4095));
}

bool pipe_wanted(const flashe_ctx *ctx, uint64_t n, const void *out_host)
{
    const char *e = getenv("FLASHE_TWIN_PIPELINE");
    const bool off = e && atoi(e) == 0;
    return !off && !ctx->capturing && ctx->env.stream2 && vec_bytes(ctx, n) >= kPipeMinBytes && n > pipe_chunk_elems(ctx) && host_pinned(out_host);
}

// Leases a block per operand (in list order: the pool's best-fit choice depends on it) and runs chunk(first, count, d) over elements
// [0, n) -- d[i] points at element `first` of operand i, every operand is element-wise (copy = n x its bytes per element) -- each chunk's
// slice of the inputs uploaded before it and its slice of the outputs downloaded after it.  Pipelined (pipe_wanted: the big twins,
// output last) the chunks are pipe_chunk_elems long and the results travel on the second stream; otherwise there is one chunk [0, n)
// and one synchronisation of the ctx stream.  The blocks go back to the pool when it returns.
template <class Chunk>
int staged_chunks(flashe_ctx *ctx, uint64_t n, const std::vector<Operand> &ops, Chunk &&chunk)
{
    if (int rc = flashe_host::refuse_in_capture(ctx, "a host-pointer call (it copies from and to host memory and waits)")) return rc;
    std::vector<Tmp> blocks(ops.size());
    for (size_t i = 0; i < ops.size(); i++)
        if (!ops[i].absent) HIP_TRY(ctx, blocks[i].alloc(ctx, ops[i].bytes));
    const bool pipe = n > 1 && pipe_wanted(ctx, n, ops.back().dst);
    auto run = [&]() -> int {
        const uint64_t ch = pipe ? pipe_chunk_elems(ctx) : n;
        std::vector<Dev> d(ops.size());
        for (uint64_t f = 0, q = 0; f < n; f += ch, q++) {
            const uint64_t cnt = std::min(ch, n - f);
            for (size_t i = 0; i < ops.size(); i++) {
                const size_t elem = ops[i].copy / n;
                d[i].p = blocks[i].p ? static_cast<char *>(blocks[i].p) + f * elem : nullptr;
                if (cnt * elem) HIP_TRY(ctx, upload(ctx, ops[i], blocks[i].p, f * elem, cnt * elem));
            }
            if (int rc = chunk(f, cnt, d.data())) return rc;
            for (size_t i = 0; i < ops.size(); i++) {
                const size_t elem = ops[i].copy / n;
                if (!ops[i].dst || cnt * elem == 0) continue;
                char *dst = static_cast<char *>(ops[i].dst) + f * elem;
                if (!pipe) { HIP_TRY(ctx, hipMemcpyAsync(dst, d[i].p, cnt * elem, hipMemcpyDeviceToHost, ctx->env.stream)); continue; }
                // device -> pinned host on the second stream, behind everything the ctx stream has been given so far
                hipEvent_t &ev = ctx->ev_copy[q & 1];
                if (!ev) HIP_TRY(ctx, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
                HIP_TRY(ctx, hipEventRecord(ev, ctx->env.stream));
                HIP_TRY(ctx, hipStreamWaitEvent(ctx->env.stream2, ev, 0));
                HIP_TRY(ctx, hipMemcpyAsync(dst, d[i].p, cnt * elem, hipMemcpyDeviceToHost, ctx->env.stream2));
            }
        }
        return FLASHE_OK;
    };
    if (!pipe) {
        if (int rc = run()) return rc;
        HIP_TRY(ctx, hipStreamSynchronize(ctx->env.stream));
        return FLASHE_OK;
    }
    // both streams idle before the blocks go back, on the error paths too: a copy must not outlive its block's lease
    const int rc = run();
    const hipError_t a = hipStreamSynchronize(ctx->env.stream), b = hipStreamSynchronize(ctx->env.stream2);
    if (rc) return rc;
    HIP_TRY(ctx, a != hipSuccess ? a : b);
    return FLASHE_OK;
}

// the synchronous twins: one chunk holding everything
template <class Call> int staged(flashe_ctx *ctx, const std::vector<Operand> &ops, Call &&call)
{
    return staged_chunks(ctx, 1, ops, [&](uint64_t, uint64_t, Dev *d) { return call(d); });
}

}  // namespace

extern "C" {

int flashe_mask(flashe_ctx *ctx, uint32_t iter, const uint32_t *idx, int n_idx, uint64_t n, uint32_t n_jobs, uint64_t *out)
{
    CHECK_CTX(ctx);
    if (n == 0) return FLASHE_OK;
    if (!out) return fail(ctx, FLASHE_EINVAL, "null output");
    return staged(ctx, {down(out, vec_bytes(ctx, n))}, [&](Dev *d) { return flashe_mask_dev(ctx, iter, idx, n_idx, n, n_jobs, d[0]); });
}

int flashe_encrypt(flashe_ctx *ctx, uint32_t iter, uint32_t idx, int scheme, uint64_t n, uint32_t n_jobs, const uint64_t *pt,
                   int pt_limbs, uint64_t *ct)
{
    CHECK_CTX(ctx);
    if (int rc = flashe_host::check_double_idx(ctx, scheme, &idx, 1)) return rc;
    if (n == 0) return FLASHE_OK;
    if (!pt || !ct) return fail(ctx, FLASHE_EINVAL, "null vector");
    if (pt_limbs != 1 && pt_limbs != ctx->limbs) return fail(ctx, FLASHE_EINVAL, "pt_limbs must be 1 or %d", ctx->limbs);
    return staged_chunks(ctx, n, {up(pt, static_cast<size_t>(n) * pt_limbs * 8), down(ct, vec_bytes(ctx, n))}, [&](uint64_t f, uint64_t cnt, Dev *d) {
        return flashe_encrypt_range_dev(ctx, iter, idx, scheme, n, n_jobs, f, cnt, d[0], pt_limbs, d[1]);
    });
}

// host-pointer twins of the prepared calls (synchronous: H2D + one HBM-bound kernel + D2H; the masks never leave the device)
int flashe_encrypt_prepared(flashe_ctx *ctx, uint64_t n, const uint64_t *pt, int pt_limbs, uint64_t *ct)
{
    CHECK_CTX(ctx);
    if (n && (!pt || !ct)) return fail(ctx, FLASHE_EINVAL, "null vector");
    if (pt_limbs != 1 && pt_limbs != ctx->limbs) return fail(ctx, FLASHE_EINVAL, "pt_limbs must be 1 or %d", ctx->limbs);
    if (n == 0) return flashe_encrypt_prepared_dev(ctx, 0, nullptr, pt_limbs, nullptr);
    return staged(ctx, {up(pt, static_cast<size_t>(n) * pt_limbs * 8), down(ct, vec_bytes(ctx, n))},
                  [&](Dev *d) { return flashe_encrypt_prepared_dev(ctx, n, d[0], pt_limbs, d[1]); });
}

int flashe_decrypt_prepared(flashe_ctx *ctx, uint32_t iter, const uint32_t *add_idx, int n_add, const uint32_t *minus_idx, int n_minus,
                            uint64_t n, uint32_t n_jobs, const uint64_t *in, uint64_t *out)
{
    CHECK_CTX(ctx);
    if (n && (!in || !out)) return fail(ctx, FLASHE_EINVAL, "null vector");
    if (n == 0) return flashe_decrypt_prepared_dev(ctx, iter, add_idx, n_add, minus_idx, n_minus, 0, n_jobs, nullptr, nullptr);
    return staged(ctx, {up(in, vec_bytes(ctx, n)), down(out, vec_bytes(ctx, n))},
                  [&](Dev *d) { return flashe_decrypt_prepared_dev(ctx, iter, add_idx, n_add, minus_idx, n_minus, n, n_jobs, d[0], d[1]); });
}

int flashe_decrypt(flashe_ctx *ctx, uint32_t iter, const uint32_t *add_idx, int n_add, const uint32_t *minus_idx, int n_minus,
                   uint64_t n, uint32_t n_jobs, const uint64_t *in, uint64_t *out)
{
    CHECK_CTX(ctx);
    if (n == 0) return FLASHE_OK;
    if (!in || !out) return fail(ctx, FLASHE_EINVAL, "null vector");
    return staged_chunks(ctx, n, {up(in, vec_bytes(ctx, n)), down(out, vec_bytes(ctx, n))}, [&](uint64_t f, uint64_t cnt, Dev *d) {
        return flashe_decrypt_range_dev(ctx, iter, add_idx, n_add, minus_idx, n_minus, n, n_jobs, f, cnt, d[0], d[1]);
    });
}

int flashe_combine(flashe_ctx *ctx, uint64_t n, const uint64_t *in, int in_limbs, const uint64_t *add, const uint64_t *minus, uint64_t *out)
{
    CHECK_CTX(ctx);
    if (n == 0) return FLASHE_OK;
    if (!in || !out) return fail(ctx, FLASHE_EINVAL, "null vector");
    if (in_limbs != 1 && in_limbs != ctx->limbs) return fail(ctx, FLASHE_EINVAL, "in_limbs must be 1 or %d", ctx->limbs);
    enum { IN, OUT, ADD, MINUS };                                 // (the order the blocks are leased in)
    return staged(ctx, {up(in, static_cast<size_t>(n) * in_limbs * 8), down(out, vec_bytes(ctx, n)), optional(up(add, vec_bytes(ctx, n))),
                        optional(up(minus, vec_bytes(ctx, n)))},
                  [&](Dev *d) { return flashe_combine_dev(ctx, n, d[IN], in_limbs, d[ADD], d[MINUS], d[OUT]); });
}

int flashe_aggregate_elem(flashe_ctx *ctx, int C, const uint64_t *const *cts, uint64_t n, uint64_t *out)
{
    CHECK_CTX(ctx);
    if (C < 1 || !cts) return fail(ctx, FLASHE_EINVAL, "aggregate_elem: bad arguments (C = %d)", C);
    if (n == 0) return FLASHE_OK;
    if (!out) return fail(ctx, FLASHE_EINVAL, "null output");
    for (int c = 0; c < C; c++)
        if (!cts[c]) return fail(ctx, FLASHE_EINVAL, "operand %d is null", c);
    // (pipelined: upload bound, C vectors up and one down -- the chunks hide the reduce kernels and the download under the uploads)
    const size_t vb = (vec_bytes(ctx, n) + 15) & ~static_cast<size_t>(15);
    return staged_chunks(ctx, n, {gather(cts, C, vec_bytes(ctx, n), vb), down(out, vec_bytes(ctx, n), vb)}, [&](uint64_t, uint64_t cnt, Dev *d) {
        return flashe_aggregate_elem_dev(ctx, C, parts_of<uint64_t>(d[0], C, vb).data(), cnt, d[1]);
    });
}

int flashe_aggregate_packed(flashe_ctx *ctx, int C, const uint64_t *const *packed, uint64_t n_limbs, uint64_t total_bits, uint64_t *out)
{
    CHECK_CTX(ctx);
    if (C < 1 || !packed) return fail(ctx, FLASHE_EINVAL, "aggregate_packed: bad arguments (C = %d)", C);
    if (n_limbs != (total_bits + 63) / 64) return fail(ctx, FLASHE_EINVAL, "n_limbs must equal ceil(total_bits / 64)");
    if (n_limbs == 0) return FLASHE_OK;
    if (!out) return fail(ctx, FLASHE_EINVAL, "null output");
    for (int c = 0; c < C; c++)
        if (!packed[c]) return fail(ctx, FLASHE_EINVAL, "operand %d is null", c);
    const size_t bytes = static_cast<size_t>(n_limbs) * 8, vb = (bytes + 15) & ~static_cast<size_t>(15);
    return staged(ctx, {gather(packed, C, bytes, vb), down(out, bytes, vb)}, [&](Dev *d) {
        return flashe_aggregate_packed_dev(ctx, C, parts_of<uint64_t>(d[0], C, vb).data(), n_limbs, total_bits, d[1]);
    });
}

int flashe_pack(flashe_ctx *ctx, uint64_t n, const uint64_t *in, uint64_t *out)
{
    CHECK_CTX(ctx);
    if (n == 0) return FLASHE_OK;
    if (!in || !out) return fail(ctx, FLASHE_EINVAL, "null vector");
    const size_t ob = static_cast<size_t>((n * ctx->int_bits + 63) / 64) * 8;
    return staged(ctx, {up(in, vec_bytes(ctx, n)), down(out, ob)}, [&](Dev *d) { return flashe_pack_dev(ctx, n, d[0], d[1]); });
}

int flashe_unpack(flashe_ctx *ctx, uint64_t n, const uint64_t *in, uint64_t *out)
{
    CHECK_CTX(ctx);
    if (n == 0) return FLASHE_OK;
    if (!in || !out) return fail(ctx, FLASHE_EINVAL, "null vector");
    const size_t ib = static_cast<size_t>((n * ctx->int_bits + 63) / 64) * 8;
    return staged(ctx, {up(in, ib), down(out, vec_bytes(ctx, n))}, [&](Dev *d) { return flashe_unpack_dev(ctx, n, d[0], d[1]); });
}

int flashe_expand_to_dense(flashe_ctx *ctx, uint64_t total, uint64_t k, const uint32_t *loc, const uint64_t *vals,
                           const uint64_t *zero, uint64_t *out)
{
    CHECK_CTX(ctx);
    if (total == 0) return FLASHE_OK;
    if (!out || !zero || (k && (!loc || !vals))) return fail(ctx, FLASHE_EINVAL, "null argument");
    for (uint64_t q = 0; q < k; q++)
        if (loc[q] >= total) return fail(ctx, FLASHE_EINVAL, "location %llu out of range", static_cast<unsigned long long>(loc[q]));
    return staged(ctx, {up(loc, static_cast<size_t>(k) * 4), up(vals, vec_bytes(ctx, k)), down(out, vec_bytes(ctx, total))},
                  [&](Dev *d) { return flashe_expand_to_dense_dev(ctx, total, k, d[0], d[1], zero, d[2]); });
}

int flashe_sparse_minus_mask(flashe_ctx *ctx, uint32_t iter, int C, const uint32_t *const *loc, const uint64_t *k, uint64_t total,
                             uint32_t n_jobs, uint64_t *out)
{
    CHECK_CTX(ctx);
    if (total == 0) return FLASHE_OK;
    if (C < 0 || (C && (!loc || !k)) || !out) return fail(ctx, FLASHE_EINVAL, "bad arguments");
    std::vector<Operand> ops;
    bool sorted = true;            // the reference's lists are (jzf_aggregator.py:598); then the one-pass span reduce applies
    for (int c = 0; c < C; c++) {
        for (uint64_t q = 0; q < k[c]; q++) {
            if (loc[c][q] >= total) return fail(ctx, FLASHE_EINVAL, "client %d location out of range", c);
            if (q && loc[c][q] <= loc[c][q - 1]) sorted = false;
        }
        ops.push_back(up(loc[c], static_cast<size_t>(k[c]) * 4));
    }
    ops.push_back(down(out, vec_bytes(ctx, total)));
    return staged(ctx, ops, [&](Dev *d) {
        const std::vector<const uint32_t *> lists(d, d + C);
        return (sorted ? flashe_sparse_minus_mask_sorted_dev : flashe_sparse_minus_mask_dev)(ctx, iter, C, lists.data(), k, total, n_jobs, d[C]);
    });
}

int flashe_sparse_dense_mask(flashe_ctx *ctx, uint32_t iter, int n_lists, const uint8_t *const *sel, uint64_t total, uint64_t *out)
{
    CHECK_CTX(ctx);
    if (total == 0) return FLASHE_OK;
    if (n_lists < 0 || (n_lists && !sel) || !out) return fail(ctx, FLASHE_EINVAL, "bad arguments");
    std::vector<Operand> ops;
    for (int i = 0; i < n_lists; i++) ops.push_back(up(sel[i], static_cast<size_t>(total)));
    ops.push_back(down(out, vec_bytes(ctx, total)));
    return staged(ctx, ops, [&](Dev *d) {
        const std::vector<const uint8_t *> lists(d, d + n_lists);
        return flashe_sparse_dense_mask_dev(ctx, iter, n_lists, lists.data(), total, d[n_lists]);
    });
}

int flashe_quantize(flashe_ctx *ctx, uint64_t n, const void *x, int x_is_f64, double alpha, int element_bits, const double *u,
                    uint64_t *q)
{
    CHECK_CTX(ctx);
    if (n == 0) return FLASHE_OK;
    if (!x || !u || !q) return fail(ctx, FLASHE_EINVAL, "null vector");
    const size_t xb = static_cast<size_t>(n) * (x_is_f64 ? 8 : 4);
    return staged(ctx, {up(x, xb), up(u, static_cast<size_t>(n) * 8), down(q, static_cast<size_t>(n) * 8)},
                  [&](Dev *d) { return flashe_quantize_dev(ctx, n, d[0], x_is_f64, alpha, element_bits, d[1], d[2]); });
}

int flashe_unquantize(flashe_ctx *ctx, uint64_t n, const uint64_t *v, int v_limbs, double alpha, int element_bits, int num_clients,
                      double *out)
{
    CHECK_CTX(ctx);
    if (n == 0) return FLASHE_OK;
    if (!v || !out) return fail(ctx, FLASHE_EINVAL, "null vector");
    if (v_limbs != 1 && v_limbs != 2) return fail(ctx, FLASHE_EINVAL, "v_limbs must be 1 or 2");
    return staged(ctx, {up(v, static_cast<size_t>(n) * v_limbs * 8), down(out, static_cast<size_t>(n) * 8)},
                  [&](Dev *d) { return flashe_unquantize_dev(ctx, n, d[0], v_limbs, alpha, element_bits, num_clients, d[1]); });
}

int flashe_batch(flashe_ctx *ctx, uint64_t n, const uint64_t *vals, int field_bits, uint64_t *out)
{
    CHECK_CTX(ctx);
    if (n == 0) return FLASHE_OK;
    if (!vals || !out) return fail(ctx, FLASHE_EINVAL, "null vector");
    if (int rc = flashe_host::check_field_bits(ctx, field_bits)) return rc;
    const uint64_t bs = ctx->int_bits / field_bits, nb = (n + bs - 1) / bs;
    return staged(ctx, {up(vals, static_cast<size_t>(n) * 8), down(out, vec_bytes(ctx, nb))},
                  [&](Dev *d) { return flashe_batch_dev(ctx, n, d[0], field_bits, d[1]); });
}

int flashe_unbatch(flashe_ctx *ctx, uint64_t n_batches, const uint64_t *in, int field_bits, uint64_t *out)
{
    CHECK_CTX(ctx);
    if (n_batches == 0) return FLASHE_OK;
    if (!in || !out) return fail(ctx, FLASHE_EINVAL, "null vector");
    if (int rc = flashe_host::check_field_bits(ctx, field_bits)) return rc;
    const uint64_t bs = ctx->int_bits / field_bits;
    return staged(ctx, {up(in, vec_bytes(ctx, n_batches)), down(out, static_cast<size_t>(n_batches * bs) * 8)},
                  [&](Dev *d) { return flashe_unbatch_dev(ctx, n_batches, d[0], field_bits, d[1]); });
}

int flashe_sparsify(flashe_ctx *ctx, uint64_t n, uint64_t k, const void *x, int x_is_f64, void *residual, uint32_t *loc, void *vals)
{
    CHECK_CTX(ctx);
    if (n == 0 || (k == 0 && !residual)) return FLASHE_OK;          // (k == 0 with a residual: the layer only updates it)
    if (!x || (k && (!loc || !vals))) return fail(ctx, FLASHE_EINVAL, "null vector");
    const size_t es = x_is_f64 ? 8 : 4;
    enum { X, LOC, VALS, RESIDUAL };                              // (the order the blocks are leased in)
    return staged(ctx, {up(x, n * es), unless_empty(down(loc, k * 4)), unless_empty(down(vals, k * es)), optional(up_down(residual, n * es))},
                  [&](Dev *d) { return flashe_sparsify_dev(ctx, n, k, d[X], x_is_f64, d[RESIDUAL], d[LOC], d[VALS]); });
}

int flashe_sparsify_batch(flashe_ctx *ctx, int n_layers, const uint64_t *n, const uint64_t *k, const void *x, int x_is_f64, void *residual,
                          uint32_t *loc, void *vals)
{
    CHECK_CTX(ctx);
    if (n_layers < 0 || (n_layers && (!n || !k))) return fail(ctx, FLASHE_EINVAL, "sparsify_batch: bad arguments");
    uint64_t total = 0, total_k = 0;
    for (int l = 0; l < n_layers; l++) { total += n[l]; total_k += k[l]; }
    if (total == 0 || (total_k == 0 && !residual)) return FLASHE_OK;
    if (!x || (total_k && (!loc || !vals))) return fail(ctx, FLASHE_EINVAL, "null vector");
    const size_t es = x_is_f64 ? 8 : 4;
    enum { X, LOC, VALS, RESIDUAL };
    return staged(ctx, {up(x, total * es), unless_empty(down(loc, total_k * 4)), unless_empty(down(vals, total_k * es)), optional(up_down(residual, total * es))},
                  [&](Dev *d) { return flashe_sparsify_batch_dev(ctx, n_layers, n, k, d[X], x_is_f64, d[RESIDUAL], d[LOC], d[VALS]); });
}

}  // extern "C"
