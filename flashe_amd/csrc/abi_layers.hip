// C ABI of libflashe_hip.so, the codec and sparsifier entry points (see include/flashe.h): the flat forms and every form that takes a
// per-layer table -- the model-wide codec, batched and tensor forms, the prepared client step, the cohorts, flashe_store_layers_dev,
// flashe_stage_layers_dev / flashe_finish_layers_dev.
// Host-side glue only: argument checks, the tables and the stage pass; what it shares with abi.hip is declared in ctx.h.
#include "ctx.h"
#include "layer_tables.h"
#include "cohort_streams.h"
#include "cohort_cut.h"
#include "draw_launch.h"
#include "pcg64_stream.h"
#include "philox_stream.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

using namespace flashe;
using namespace flashe_host;

namespace {

using flashe_tables::layer_end;

// ---- the checks of this family, each stated once ----
int check_codec_bits(flashe_ctx *ctx, int element_bits)
{
    return element_bits < 1 || element_bits > 62 ? fail(ctx, FLASHE_EINVAL, "element_bits must be in [1, 62], got %d", element_bits) : FLASHE_OK;
}

// the front end's range: what it quantises to must fit an element
int check_element_bits(flashe_ctx *ctx, int element_bits)
{
    const bool ok = element_bits >= 1 && element_bits <= 62 && element_bits <= ctx->int_bits;
    return ok ? FLASHE_OK : fail(ctx, FLASHE_EINVAL, "element_bits must be in [1, min(62, int_bits)], got %d", element_bits);
}

// the batched form's widths; *bs = the values an element holds
int check_batch_bits(flashe_ctx *ctx, int element_bits, int field_bits, uint64_t *bs)
{
    if (element_bits < 1 || element_bits > 62 || field_bits < element_bits || field_bits > ctx->int_bits)
        return fail(ctx, FLASHE_EINVAL, "need 1 <= element_bits <= field_bits <= int_bits (element_bits <= 62)");
    *bs = static_cast<uint64_t>(ctx->int_bits / field_bits);
    return FLASHE_OK;
}

int check_batched_count(flashe_ctx *ctx, uint64_t e, uint64_t n_elems)
{
    return e == n_elems ? FLASHE_OK : fail(ctx, FLASHE_EINVAL, "the layers batch into %llu elements, n_elems says %llu", static_cast<unsigned long long>(e),
                                           static_cast<unsigned long long>(n_elems));
}

// every pointer a multiple of `align` bytes (a null pointer passes: who needs the vector has checked)
int check_aligned(flashe_ctx *ctx, std::initializer_list<const void *> ps, unsigned align)
{
    for (const void *p : ps)
        if (reinterpret_cast<uintptr_t>(p) & (align - 1u)) return fail(ctx, FLASHE_EINVAL, "misaligned vector");
    return FLASHE_OK;
}
// ... like ciphertext vectors (ct_aligned's rule)
int check_vec_aligned(flashe_ctx *ctx, std::initializer_list<const void *> vecs) { return check_aligned(ctx, vecs, ctx->limbs == 2 ? 16 : 8); }

int check_f64_aligned(flashe_ctx *ctx, const void *p, const char *what)
{ return (reinterpret_cast<uintptr_t>(p) & 7u) ? fail(ctx, FLASHE_EINVAL, "%s must be 8-byte aligned", what) : FLASHE_OK; }

// What the model-wide front ends share once their mask source is settled (the online forms: check_scheme first; the prepared forms:
// check_prepared first): the vectors given, the width, the ciphertext vector, the range, the draws.
int check_model_front(flashe_ctx *ctx, uint64_t n, uint32_t n_jobs, uint64_t first, uint64_t count, int element_bits, const double *u_dev,
                      const uint64_t *ct_dev)
{
    if (count && (!u_dev || !ct_dev)) return fail(ctx, FLASHE_EINVAL, "null vector");
    int rc = check_element_bits(ctx, element_bits);
    if (rc || (rc = check_prf_args(ctx, 0, 0, n_jobs, ct_dev, nullptr, 0)) || (rc = check_range(ctx, n, first, count))) return rc;
    return check_f64_aligned(ctx, u_dev, "u_dev");
}

Codec codec_model_front(const CodecLayer *tab, int n_tab, const double *u_dev, uint64_t first)
{
    Codec cq{};
    cq.x = tab;                     // (non-null = front end on; the values come through the table)
    cq.u = u_dev; cq.layers = tab; cq.n_layers = n_tab; cq.k0 = first;
    return cq;
}

Codec codec_model_back(const CodecLayer *tab, int n_tab, double *out_dev, uint64_t first)
{
    Codec cq{};
    cq.fout = out_dev; cq.layers = tab; cq.n_layers = n_tab; cq.k0 = first;
    return cq;
}

// The stage pass (tensors.hip): every source that is not read where it lies is converted into ctx->tensor_ws, all in ONE launch.
// add() books a source and returns its slot; place() settles every st[slot].dst; run() then uploads the table and launches.
struct StagePass {
    std::vector<TensorStage> st;
    flashe_tables::StageSlots slots;
    size_t add(const void *src, int32_t dtype, double shift, int32_t flags, uint64_t size, bool f64)
    {
        st.push_back(TensorStage{slots.total, src, nullptr, shift, dtype, flags | (f64 ? kTensorLoopF64 : 0)});
        return slots.add(size, f64);
    }
    int place(flashe_ctx *ctx)
    {
        if (st.empty()) return FLASHE_OK;
        if (int rc = ensure(ctx, ctx->tensor_ws, slots.bytes)) return rc;
        for (size_t i = 0; i < st.size(); i++) st[i].dst = static_cast<char *>(ctx->tensor_ws.p) + slots.at[i];
        return FLASHE_OK;
    }
    int run(flashe_ctx *ctx)
    {
        if (st.empty()) return FLASHE_OK;
        const TensorStage *tab = nullptr;
        if (int rc = upload_tab(ctx, ctx->tensor_tab, st, &tab)) return rc;
        HIP_TRY(ctx, launch_stage_layers(ctx->env, tab, static_cast<int>(st.size()), slots.total));
        return FLASHE_OK;
    }
};

}  // namespace

extern "C" {

// ---- quantise / batch codec ----
int flashe_quantize_dev(flashe_ctx *ctx, uint64_t n, const void *x_dev, int x_is_f64, double alpha, int element_bits,
                        const double *u_dev, uint64_t *q_dev)
{
    CHECK_CTX(ctx);
    if (n && (!x_dev || !u_dev || !q_dev)) return fail(ctx, FLASHE_EINVAL, "null vector");
    if (!(alpha > 0)) return fail(ctx, FLASHE_EINVAL, "alpha must be positive");
    int rc = check_codec_bits(ctx, element_bits);
    if (rc) return rc;
    HIP_TRY(ctx, launch_quantize(ctx->env, n, x_dev, x_is_f64 != 0, alpha, element_bits, u_dev, q_dev));
    return FLASHE_OK;
}

int flashe_unquantize_dev(flashe_ctx *ctx, uint64_t n, const uint64_t *v_dev, int v_limbs, double alpha, int element_bits,
                          int num_clients, double *out_dev)
{
    CHECK_CTX(ctx);
    if (n && (!v_dev || !out_dev)) return fail(ctx, FLASHE_EINVAL, "null vector");
    if (v_limbs != 1 && v_limbs != 2) return fail(ctx, FLASHE_EINVAL, "v_limbs must be 1 or 2");
    if (v_limbs == 2 && !aligned16(v_dev)) return fail(ctx, FLASHE_EINVAL, "device vectors must be 16-byte aligned");
    if (num_clients < 1) return fail(ctx, FLASHE_EINVAL, "num_clients must be >= 1");
    int rc = check_codec_bits(ctx, element_bits);
    if (rc) return rc;
    HIP_TRY(ctx, launch_unquantize(ctx->env, n, v_dev, v_limbs, alpha, element_bits, num_clients, out_dev));
    return FLASHE_OK;
}

int flashe_batch_dev(flashe_ctx *ctx, uint64_t n, const uint64_t *vals_dev, int field_bits, uint64_t *out_dev)
{
    CHECK_CTX(ctx);
    if (n && (!vals_dev || !out_dev)) return fail(ctx, FLASHE_EINVAL, "null vector");
    int rc = check_field_bits(ctx, field_bits);
    if (rc || (rc = check_wide_aligned(ctx, {out_dev}))) return rc;
    HIP_TRY(ctx, launch_batch(ctx->env, n, vals_dev, field_bits, out_dev));
    return FLASHE_OK;
}

int flashe_unbatch_dev(flashe_ctx *ctx, uint64_t n_batches, const uint64_t *in_dev, int field_bits, uint64_t *out_dev)
{
    CHECK_CTX(ctx);
    if (n_batches && (!in_dev || !out_dev)) return fail(ctx, FLASHE_EINVAL, "null vector");
    int rc = check_field_bits(ctx, field_bits);
    if (rc || (rc = check_wide_aligned(ctx, {in_dev}))) return rc;
    HIP_TRY(ctx, launch_unbatch(ctx->env, n_batches, in_dev, field_bits, out_dev));
    return FLASHE_OK;
}

// ---- sparsifier ----
int flashe_sparsify_dev(flashe_ctx *ctx, uint64_t n, uint64_t k, const void *x_dev, int x_is_f64, void *residual_dev, uint32_t *loc_dev,
                        void *vals_dev)
{
    CHECK_CTX(ctx);
    if (n >= (1ull << 32)) return fail(ctx, FLASHE_EINVAL, "sparsify: n must be < 2^32");
    if (k > n) return fail(ctx, FLASHE_EINVAL, "sparsify: k (%llu) > n (%llu)", static_cast<unsigned long long>(k),
                           static_cast<unsigned long long>(n));
    // (a layer that keeps nothing only updates its residual: x is read whenever there is something to write, loc / vals only when k > 0)
    if (n && (k || residual_dev) && !x_dev) return fail(ctx, FLASHE_EINVAL, "null vector");
    if (n && k && (!loc_dev || !vals_dev)) return fail(ctx, FLASHE_EINVAL, "null vector");
    int rc = ensure(ctx, ctx->sp_ws, sparsify_workspace_bytes(n));
    if (rc) return rc;
    HIP_TRY(ctx, launch_sparsify(ctx->env, n, k, x_dev, x_is_f64 != 0, residual_dev, loc_dev, vals_dev, ctx->sp_ws.p));
    return FLASHE_OK;
}

// Every layer of a model at once: layer l = elements [off_l, off_l + n[l]) of the flat vectors (layers back to back), its k[l] entries go
// to [koff_l, koff_l + k[l]) of the flat outputs, locations relative to the layer.  n and k are HOST arrays.
int flashe_sparsify_batch_dev(flashe_ctx *ctx, int n_layers, const uint64_t *n, const uint64_t *k, const void *x_dev, int x_is_f64, void *residual_dev,
                              uint32_t *loc_dev, void *vals_dev)
{
    CHECK_CTX(ctx);
    if (n_layers < 0 || (n_layers && (!n || !k))) return fail(ctx, FLASHE_EINVAL, "sparsify_batch: bad arguments");
    if (n_layers == 0) return FLASHE_OK;
    if (ctx->capturing) return fail(ctx, FLASHE_EINVAL, "sparsify_batch: not inside a graph capture (the layer table is uploaded synchronously)");
    uint64_t total = 0, total_k = 0;
    for (int l = 0; l < n_layers; l++) {
        if (n[l] >= (1ull << 32)) return fail(ctx, FLASHE_EINVAL, "sparsify_batch: layer %d: n must be < 2^32", l);
        if (k[l] > n[l]) return fail(ctx, FLASHE_EINVAL, "sparsify_batch: layer %d: k (%llu) > n (%llu)", l, static_cast<unsigned long long>(k[l]),
                                     static_cast<unsigned long long>(n[l]));
        total += n[l]; total_k += k[l];
    }
    if (total == 0 || (total_k == 0 && !residual_dev)) return FLASHE_OK;       // (total_k == 0 with a residual: every layer only updates it)
    if (!x_dev || (total_k && (!loc_dev || !vals_dev))) return fail(ctx, FLASHE_EINVAL, "null vector");
    std::vector<unsigned char> desc(sparsify_batch_desc_bytes(n_layers));
    const uint64_t blocks = sparsify_batch_layout(n_layers, n, k, desc.data());
    if (blocks >= (1ull << 32)) return fail(ctx, FLASHE_EINVAL, "sparsify_batch: too many elements");
    int rc = ensure(ctx, ctx->sp_ws, sparsify_batch_workspace_bytes(n_layers, blocks));
    if (rc || (rc = upload_bytes(ctx, ctx->sp_ws.p, desc.data(), desc.size()))) return rc;
    HIP_TRY(ctx, launch_sparsify_batch(ctx->env, n_layers, blocks, x_dev, x_is_f64 != 0, residual_dev, loc_dev, vals_dev, ctx->sp_ws.p));
    return FLASHE_OK;
}

// the PRF launch with the quantising front end cq over elements [first, first + count)
static int launch_quantize_encrypt(flashe_ctx *ctx, const Codec &cq, uint32_t iter, uint32_t idx, int scheme, uint64_t n, uint32_t n_jobs, uint64_t first,
                                   uint64_t count, uint64_t *ct_dev)
{
    LaunchEnv env = ctx->env;
    env.codec = &cq;
    if (int rc = check_double_idx(ctx, scheme, &idx, 1)) return rc;
    const uint32_t add = idx, minus = idx + 1;
    HIP_TRY(ctx, launch_prf(env, iter, &add, 1, &minus, scheme == FLASHE_SCHEME_DOUBLE ? 1 : 0, n, n_jobs, first, count, nullptr, 0, ct_dev));
    return FLASHE_OK;
}

// ---- fused codec: quantise -> encrypt and decrypt -> unquantise in ONE launch each ----
int flashe_quantize_encrypt_dev(flashe_ctx *ctx, uint32_t iter, uint32_t idx, int scheme, uint64_t n, uint32_t n_jobs, const void *x_dev,
                                int x_is_f64, double alpha, int element_bits, const double *u_dev, uint64_t *ct_dev)
{
    CHECK_CTX(ctx);
    if (int rc = check_scheme(ctx, scheme)) return rc;
    if (n && (!x_dev || !u_dev || !ct_dev)) return fail(ctx, FLASHE_EINVAL, "null vector");
    if (!(alpha > 0)) return fail(ctx, FLASHE_EINVAL, "alpha must be positive");
    int rc = check_element_bits(ctx, element_bits);
    if (rc || (rc = check_prf_args(ctx, 1, scheme, n_jobs, ct_dev, nullptr, 0))) return rc;
    return launch_quantize_encrypt(ctx, codec_quantize_front(x_dev, x_is_f64 != 0, alpha, element_bits, u_dev), iter, idx, scheme, n, n_jobs, 0, n, ct_dev);
}

// the unmask + unquantise of prefix lists of any length: all but the last group accumulate into ctx scratch, the last launch writes
// the floats
static int prf_lists_unquantize(flashe_ctx *ctx, const Codec &cq, uint32_t iter, const uint32_t *add_idx, int n_add, const uint32_t *minus_idx,
                                int n_minus, uint64_t n, uint32_t n_jobs, uint64_t first, uint64_t count, const uint64_t *in_dev)
{
    const uint64_t *src = in_dev;
    int a = 0, m = 0;
    if (n_add > kMaxIdx || n_minus > kMaxIdx) {
        const int rc = ensure(ctx, ctx->stream_tmp, vec_bytes(ctx, count));
        if (rc) return rc;
        uint64_t *tmp = static_cast<uint64_t *>(ctx->stream_tmp.p);
        while (n_add - a > kMaxIdx || n_minus - m > kMaxIdx) {
            const int na = std::min(kMaxIdx, n_add - a), nm = std::min(kMaxIdx, n_minus - m);
            HIP_TRY(ctx, launch_prf(ctx->env, iter, add_idx + a, na, minus_idx + m, nm, n, n_jobs, first, count, src, ctx->limbs, tmp));
            a += na; m += nm; src = tmp;
        }
    }
    LaunchEnv env = ctx->env;
    env.codec = &cq;
    HIP_TRY(ctx, launch_prf(env, iter, add_idx + a, n_add - a, minus_idx + m, n_minus - m, n, n_jobs, first, count, src, ctx->limbs,
                            const_cast<uint64_t *>(src)));
    return FLASHE_OK;
}

int flashe_decrypt_unquantize_dev(flashe_ctx *ctx, uint32_t iter, const uint32_t *add_idx, int n_add, const uint32_t *minus_idx, int n_minus,
                                  uint64_t n, uint32_t n_jobs, const uint64_t *in_dev, double alpha, int element_bits, int num_clients,
                                  double *out_dev)
{
    CHECK_CTX(ctx);
    if (n && (!in_dev || !out_dev)) return fail(ctx, FLASHE_EINVAL, "null vector");
    if (!(alpha > 0) || num_clients < 1) return fail(ctx, FLASHE_EINVAL, "alpha must be positive and num_clients >= 1");
    int rc = check_codec_bits(ctx, element_bits);
    if (rc || (rc = check_prf_args(ctx, n_add, n_minus, n_jobs, in_dev, in_dev, ctx->limbs))) return rc;
    if (n == 0) return FLASHE_OK;
    Codec cq{};
    codec_unquantize_back(&cq, alpha, element_bits, num_clients, out_dev);
    if (n_add == 0 && n_minus == 0) {
        // nothing to unmask: reduce mod 2^b like every decrypt does, then unquantise (two launches; not a shape a round produces)
        rc = ensure(ctx, ctx->stream_tmp, vec_bytes(ctx, n));
        if (rc) return rc;
        uint64_t *tmp = static_cast<uint64_t *>(ctx->stream_tmp.p);
        HIP_TRY(ctx, launch_combine(ctx->env, n, in_dev, ctx->limbs, nullptr, nullptr, tmp));
        HIP_TRY(ctx, launch_unquantize(ctx->env, n, tmp, ctx->limbs, alpha, element_bits, num_clients, out_dev));
        return FLASHE_OK;
    }
    return prf_lists_unquantize(ctx, cq, iter, add_idx, n_add, minus_idx, n_minus, n, n_jobs, 0, n, in_dev);
}

// ---- the same over a flattened model: one launch, per-layer parameters from a device table (jzf_aggregator.py:721-741, :887-899) ----
// validates the caller's table, stages the entries of the non-empty layers on the device (ctx->codec_tab) and sets *cq up over them: the
// front end (u_dev: the draws) or the back end (out_dev: the floats) from element `first` on
static int stage_codec_layers(flashe_ctx *ctx, uint64_t n, const flashe_codec_layer *layers, int n_layers, bool front, int element_bits,
                              int num_clients, uint64_t first, uint64_t count, const double *u_dev, double *out_dev, Codec *cq)
{
    if (n_layers < 1 || !layers) return fail(ctx, FLASHE_EINVAL, "the layer table needs at least one entry");
    if (layers[0].start != 0) return fail(ctx, FLASHE_EINVAL, "layers[0].start must be 0");
    if (ctx->capturing) return fail(ctx, FLASHE_EINVAL, "the model-wide codec calls stage their layer table per call and cannot be captured into a graph");
    std::vector<CodecLayer> tab;
    tab.reserve(static_cast<size_t>(n_layers));
    for (int l = 0; l < n_layers; l++) {
        const flashe_codec_layer &e = layers[l];
        const uint64_t end = layer_end(layers, n_layers, l, n);
        if (e.start > end || end > n) return fail(ctx, FLASHE_EINVAL, "layer %d: starts must ascend and stay within n", l);
        if (e.reserved) return fail(ctx, FLASHE_EINVAL, "layer %d: reserved field must be 0", l);
        if (e.start == end) continue;                                   // an empty layer holds no element
        if (!(e.alpha > 0)) return fail(ctx, FLASHE_EINVAL, "layer %d: alpha must be positive", l);
        const bool touched = e.start < first + count && end > first;
        if (front && touched && !e.x_dev) return fail(ctx, FLASHE_EINVAL, "layer %d: null x_dev", l);
        if (front && (reinterpret_cast<uintptr_t>(e.x_dev) & (e.x_is_f64 ? 7u : 3u))) return fail(ctx, FLASHE_EINVAL, "layer %d: x_dev is misaligned", l);
        tab.push_back(front ? codec_layer_front(e.start, e.x_dev, e.x_is_f64 != 0, e.alpha, element_bits)
                            : codec_layer_back(e.start, e.alpha, element_bits, num_clients));
    }
    const CodecLayer *tab_dev = nullptr;
    int n_tab = 0;
    if (int rc = upload_tab(ctx, ctx->codec_tab, tab, &tab_dev, &n_tab)) return rc;
    *cq = front ? codec_model_front(tab_dev, n_tab, u_dev, first) : codec_model_back(tab_dev, n_tab, out_dev, first);
    return FLASHE_OK;
}

// the model-wide front end behind its argument checks (the codec-layer and the tensor form)
static int quantize_encrypt_model(flashe_ctx *ctx, uint32_t iter, uint32_t idx, int scheme, uint64_t n, uint32_t n_jobs, uint64_t first, uint64_t count,
                                  const flashe_codec_layer *layers, int n_layers, int element_bits, const double *u_dev, uint64_t *ct_dev)
{
    Codec cq{};
    int rc = stage_codec_layers(ctx, n, layers, n_layers, true, element_bits, 1, first, count, u_dev, nullptr, &cq);
    if (rc || count == 0) return rc;
    return launch_quantize_encrypt(ctx, cq, iter, idx, scheme, n, n_jobs, first, count, ct_dev);
}

int flashe_quantize_encrypt_model_dev(flashe_ctx *ctx, uint32_t iter, uint32_t idx, int scheme, uint64_t n, uint32_t n_jobs, uint64_t first,
                                      uint64_t count, const flashe_codec_layer *layers, int n_layers, int element_bits, const double *u_dev,
                                      uint64_t *ct_dev)
{
    CHECK_CTX(ctx);
    int rc = check_scheme(ctx, scheme);
    if (rc || (rc = check_model_front(ctx, n, n_jobs, first, count, element_bits, u_dev, ct_dev))) return rc;
    return quantize_encrypt_model(ctx, iter, idx, scheme, n, n_jobs, first, count, layers, n_layers, element_bits, u_dev, ct_dev);
}

int flashe_decrypt_unquantize_model_dev(flashe_ctx *ctx, uint32_t iter, const uint32_t *add_idx, int n_add, const uint32_t *minus_idx, int n_minus,
                                        uint64_t n, uint32_t n_jobs, uint64_t first, uint64_t count, const uint64_t *in_dev,
                                        const flashe_codec_layer *layers, int n_layers, int element_bits, int num_clients, double *out_dev)
{
    CHECK_CTX(ctx);
    if (count && (!in_dev || !out_dev)) return fail(ctx, FLASHE_EINVAL, "null vector");
    if (num_clients < 1) return fail(ctx, FLASHE_EINVAL, "num_clients must be >= 1");
    if (n_add + n_minus == 0) return fail(ctx, FLASHE_EINVAL, "decrypt_unquantize_model: at least one prefix (a round always has one)");
    int rc = check_codec_bits(ctx, element_bits);
    if (rc || (rc = check_prf_args(ctx, n_add, n_minus, n_jobs, in_dev, in_dev, ctx->limbs)) || (rc = check_range(ctx, n, first, count))) return rc;
    if ((n_add && !add_idx) || (n_minus && !minus_idx)) return fail(ctx, FLASHE_EINVAL, "null prefix list");
    Codec cq{};
    rc = stage_codec_layers(ctx, n, layers, n_layers, false, element_bits, num_clients, first, count, nullptr, out_dev, &cq);
    if (rc || count == 0) return rc;
    return prf_lists_unquantize(ctx, cq, iter, add_idx, n_add, minus_idx, n_minus, n, n_jobs, first, count, in_dev);
}

// unflatten_weights + QuantizingClient.unquantize (jzf_aggregator.py:652-671, jzf_quantize.py:493-540) of a flattened vector that is
// already decrypted -- the sparse job's way back, whose decrypt is the sparse minus-mask pass, not a prefix list
int flashe_unquantize_model_dev(flashe_ctx *ctx, uint64_t n, uint64_t first, uint64_t count, const uint64_t *in_dev,
                                const flashe_codec_layer *layers, int n_layers, int element_bits, int num_clients, double *out_dev)
{
    CHECK_CTX(ctx);
    if (count && (!in_dev || !out_dev)) return fail(ctx, FLASHE_EINVAL, "null vector");
    if (num_clients < 1) return fail(ctx, FLASHE_EINVAL, "num_clients must be >= 1");
    int rc = check_codec_bits(ctx, element_bits);
    if (rc || (rc = check_range(ctx, n, first, count)) || (rc = check_vec_aligned(ctx, {in_dev})) || (rc = check_aligned(ctx, {out_dev}, 8))) return rc;
    Codec cq{};
    rc = stage_codec_layers(ctx, n, layers, n_layers, false, element_bits, num_clients, first, count, nullptr, out_dev, &cq);
    if (rc || count == 0) return rc;
    HIP_TRY(ctx, launch_unquantize_model(ctx->env, count, in_dev, cq, out_dev));
    return FLASHE_OK;
}

// ---- the BATCHED codec over a flattened model (the paper's main job configuration, "batch": true) ----
struct BatchTab { const BatchLayer *tab = nullptr; int n_tab = 0; uint64_t n_values = 0; };
// validates the caller's table against n_elems and stages the entries of the non-empty layers on the device (ctx->codec_tab)
static int stage_batch_layers(flashe_ctx *ctx, const flashe_batch_layer *layers, int n_layers, bool front, int element_bits, int field_bits,
                              int num_clients, uint64_t n_elems, BatchTab *bt)
{
    if (n_layers < 1 || !layers) return fail(ctx, FLASHE_EINVAL, "the layer table needs at least one entry");
    if (ctx->capturing) return fail(ctx, FLASHE_EINVAL, "the model-wide codec calls stage their layer table per call and cannot be captured into a graph");
    uint64_t bs = 0;
    if (int rc = check_batch_bits(ctx, element_bits, field_bits, &bs)) return rc;
    for (int l = 0; l < n_layers; l++) {
        const flashe_batch_layer &y = layers[l];
        if (y.reserved) return fail(ctx, FLASHE_EINVAL, "layer %d: reserved field must be 0", l);
        if (y.size == 0) continue;
        if (!(y.alpha > 0)) return fail(ctx, FLASHE_EINVAL, "layer %d: alpha must be positive", l);
        if (front && (!y.x_dev || (reinterpret_cast<uintptr_t>(y.x_dev) & (y.x_is_f64 ? 7u : 3u)))) return fail(ctx, FLASHE_EINVAL, "layer %d: null or misaligned x_dev", l);
    }
    std::vector<BatchLayer> tab;
    const uint64_t e = flashe_tables::batched_elems(n_layers, bs, [&](int l) { return layers[l].size; }, [&](int l, uint64_t elem, uint64_t value) {
        const flashe_batch_layer &y = layers[l];
        tab.push_back(front ? batch_layer_front(elem, value, y.size, y.x_dev, y.x_is_f64 != 0, y.alpha, element_bits)
                            : batch_layer_back(elem, value, y.size, y.alpha, element_bits, num_clients));
        bt->n_values += y.size;
    });
    if (int rc = check_batched_count(ctx, e, n_elems)) return rc;
    return upload_tab(ctx, ctx->codec_tab, tab, &bt->tab, &bt->n_tab);
}

int flashe_quantize_batch_model_dev(flashe_ctx *ctx, const flashe_batch_layer *layers, int n_layers, int element_bits, int field_bits,
                                    const double *u_dev, uint64_t n_elems, uint64_t *out_dev)
{
    CHECK_CTX(ctx);
    BatchTab bt;
    int rc = stage_batch_layers(ctx, layers, n_layers, true, element_bits, field_bits, 1, n_elems, &bt);
    if (rc) return rc;
    if (n_elems && (!u_dev || !out_dev)) return fail(ctx, FLASHE_EINVAL, "null vector");
    if ((rc = check_vec_aligned(ctx, {out_dev})) || (rc = check_aligned(ctx, {u_dev}, 8))) return rc;
    if (n_elems) HIP_TRY(ctx, launch_quantize_batch_model(ctx->env, bt.tab, bt.n_tab, field_bits, u_dev, n_elems, out_dev));
    return FLASHE_OK;
}

int flashe_unbatch_unquantize_model_dev(flashe_ctx *ctx, const flashe_batch_layer *layers, int n_layers, int element_bits, int field_bits,
                                        int num_clients, const uint64_t *in_dev, uint64_t n_elems, double *out_dev)
{
    CHECK_CTX(ctx);
    if (num_clients < 1) return fail(ctx, FLASHE_EINVAL, "num_clients must be >= 1");
    BatchTab bt;
    int rc = stage_batch_layers(ctx, layers, n_layers, false, element_bits, field_bits, num_clients, n_elems, &bt);
    if (rc) return rc;
    if (bt.n_values && (!in_dev || !out_dev)) return fail(ctx, FLASHE_EINVAL, "null vector");
    if ((rc = check_vec_aligned(ctx, {in_dev})) || (rc = check_aligned(ctx, {out_dev}, 8))) return rc;
    if (bt.n_values) HIP_TRY(ctx, launch_unbatch_unquantize_model(ctx->env, bt.tab, bt.n_tab, field_bits, in_dev, bt.n_values, out_dev));
    return FLASHE_OK;
}

// ---- caller-owned tensors either side of the model-wide codec (tensors.hip) ----
static int tensor_elem_bytes(int32_t dtype)
{
    return dtype == FLASHE_TENSOR_F64 ? 8 : dtype == FLASHE_TENSOR_F32 ? 4 : (dtype == FLASHE_TENSOR_F16 || dtype == FLASHE_TENSOR_BF16) ? 2 : 0;
}

// the table's shape, dtypes and flags, and with_ptrs the pointers of its non-empty layers (a cohort's shared rows carry none); nothing is
// launched before every layer passed
static int check_tensor_layers(flashe_ctx *ctx, uint64_t n, const flashe_tensor_layer *layers, int n_layers, bool with_ptrs)
{
    if (n_layers < 1 || !layers) return fail(ctx, FLASHE_EINVAL, "the layer table needs at least one entry");
    if (layers[0].start != 0) return fail(ctx, FLASHE_EINVAL, "layers[0].start must be 0");
    if (ctx->capturing) return fail(ctx, FLASHE_EINVAL, "the tensor codec calls stage their layer table per call and cannot be captured into a graph");
    for (int l = 0; l < n_layers; l++) {
        const flashe_tensor_layer &y = layers[l];
        const uint64_t end = layer_end(layers, n_layers, l, n);
        if (y.start > end || end > n) return fail(ctx, FLASHE_EINVAL, "layer %d: starts must ascend and stay within n", l);
        const int es = tensor_elem_bytes(y.dtype);
        if (!es) return fail(ctx, FLASHE_EINVAL, "layer %d: unknown dtype %d", l, static_cast<int>(y.dtype));
        if (y.flags & ~(FLASHE_TENSOR_SHIFT | FLASHE_TENSOR_SHIFT_WIDE | FLASHE_TENSOR_LOOP_F64))
            return fail(ctx, FLASHE_EINVAL, "layer %d: unknown flags 0x%x", l, static_cast<unsigned>(y.flags));
        if (y.start == end || !with_ptrs) continue;
        if (!y.ptr) return fail(ctx, FLASHE_EINVAL, "layer %d: null ptr", l);
        if (reinterpret_cast<uintptr_t>(y.ptr) % static_cast<uintptr_t>(es)) return fail(ctx, FLASHE_EINVAL, "layer %d: ptr is not aligned to its element size", l);
    }
    return FLASHE_OK;
}

// the codec rows of a checked tensor table over [first, first + count): where the codec reads every layer and its loop dtype; the layers
// that are not read where they lie go through the stage pass
static int stage_tensor_front(flashe_ctx *ctx, uint64_t n, const flashe_tensor_layer *layers, int n_layers, uint64_t first, uint64_t count,
                              std::vector<flashe_codec_layer> &cl)
{
    cl.resize(static_cast<size_t>(n_layers));
    StagePass sp;
    std::vector<int> which;
    for (int l = 0; l < n_layers; l++) {
        const flashe_tensor_layer &y = layers[l];
        const uint64_t end = layer_end(layers, n_layers, l, n);
        const bool loop64 = y.dtype == FLASHE_TENSOR_F64 || (y.flags & FLASHE_TENSOR_LOOP_F64);
        cl[l] = flashe_codec_layer{y.start, y.ptr, y.alpha, loop64 ? 1 : 0, 0};
        const bool touched = y.start < first + count && end > first;
        const bool direct = !(y.flags & FLASHE_TENSOR_SHIFT) && (y.dtype == FLASHE_TENSOR_F64 || (y.dtype == FLASHE_TENSOR_F32 && !loop64));
        if (y.start == end || !touched || direct) continue;
        sp.add(y.ptr, y.dtype, y.shift, y.flags, end - y.start, loop64);
        which.push_back(l);
    }
    if (int rc = sp.place(ctx)) return rc;
    for (size_t i = 0; i < which.size(); i++) cl[which[i]].x_dev = sp.st[i].dst;
    return sp.run(ctx);
}

// the codec table of the model-wide front end from a checked tensor table: alphas checked, the stage pass run (what the prepared and
// the online forms share)
static int tensor_codec_layers(flashe_ctx *ctx, uint64_t n, const flashe_tensor_layer *layers, int n_layers, uint64_t first, uint64_t count,
                               std::vector<flashe_codec_layer> &cl)
{
    for (int l = 0; l < n_layers; l++)
        if (!(layers[l].alpha > 0) && layer_end(layers, n_layers, l, n) > layers[l].start)
            return fail(ctx, FLASHE_EINVAL, "layer %d: alpha must be positive", l);
    return stage_tensor_front(ctx, n, layers, n_layers, first, count, cl);
}

// the batched form: the checks of flashe_quantize_batch_model_dev that do not need the staged table, the stage pass, the batch table
static int tensor_batch_layers(flashe_ctx *ctx, const flashe_tensor_layer *layers, int n_layers, uint64_t n_values, int element_bits, int field_bits,
                               const double *u_dev, uint64_t n_elems, const uint64_t *out_dev, std::vector<flashe_batch_layer> &bl)
{
    uint64_t bs = 0;
    int rc = check_batch_bits(ctx, element_bits, field_bits, &bs);
    if (rc) return rc;
    auto size_of = [&](int l) { return layer_end(layers, n_layers, l, n_values) - layers[l].start; };
    for (int l = 0; l < n_layers; l++)
        if (size_of(l) && !(layers[l].alpha > 0)) return fail(ctx, FLASHE_EINVAL, "layer %d: alpha must be positive", l);
    if ((rc = check_batched_count(ctx, flashe_tables::batched_elems(n_layers, bs, size_of, [](int, uint64_t, uint64_t) {}), n_elems))) return rc;
    if (n_elems && (!u_dev || !out_dev)) return fail(ctx, FLASHE_EINVAL, "null vector");
    std::vector<flashe_codec_layer> cl;
    if ((rc = check_vec_aligned(ctx, {out_dev})) || (rc = check_aligned(ctx, {u_dev}, 8)) || (rc = stage_tensor_front(ctx, n_values, layers, n_layers, 0, n_values, cl))) return rc;
    for (int l = 0; l < n_layers; l++) bl.push_back(flashe_batch_layer{size_of(l), cl[l].x_dev, cl[l].alpha, cl[l].x_is_f64, 0});
    return FLASHE_OK;
}

int flashe_quantize_encrypt_tensors_dev(flashe_ctx *ctx, uint32_t iter, uint32_t idx, int scheme, uint64_t n, uint32_t n_jobs, uint64_t first,
                                        uint64_t count, const flashe_tensor_layer *layers, int n_layers, int element_bits, const double *u_dev,
                                        uint64_t *ct_dev)
{
    CHECK_CTX(ctx);
    // every check that does not need the staged table, before the stage pass launches
    int rc = check_scheme(ctx, scheme);
    if (rc || (rc = check_model_front(ctx, n, n_jobs, first, count, element_bits, u_dev, ct_dev)) ||
        (rc = check_tensor_layers(ctx, n, layers, n_layers, true)) || (rc = check_double_idx(ctx, scheme, &idx, 1)))
        return rc;
    std::vector<flashe_codec_layer> cl;
    if ((rc = tensor_codec_layers(ctx, n, layers, n_layers, first, count, cl))) return rc;
    return quantize_encrypt_model(ctx, iter, idx, scheme, n, n_jobs, first, count, cl.data(), n_layers, element_bits, u_dev, ct_dev);
}

// what every chained cohort asks of its arguments before its cipher indices
static int cohort_check_args(flashe_ctx *ctx, const char *who, int n_clients, uint64_t n, const flashe_tensor_layer *layers, int n_layers,
                             const void *const *src_dev, bool outs, int element_bits, const double *u_dev)
{
    if (n_clients < 1) return fail(ctx, FLASHE_EINVAL, "%s: n_clients must be >= 1", who);
    if (!src_dev || !outs || (n && !u_dev)) return fail(ctx, FLASHE_EINVAL, "%s: null argument", who);
    int rc = check_element_bits(ctx, element_bits);
    if (rc || (rc = check_f64_aligned(ctx, u_dev, "u_dev")) || (rc = check_tensor_layers(ctx, n, layers, n_layers, false))) return rc;
    return FLASHE_OK;
}

// ---- a cohort of co-located clients: C float models -> C ciphertexts + their sum (+ the decrypt mask) in one chained launch ----
// The shared layer table, the C x n_layers sources and their storage dtypes.  A source already in its row's compute type without SHIFT is
// read where it lies; every other one goes through ONE stage pass (tensors.hip) into ctx scratch, all clients together.
// (every form of the launch runs through one body, quantize_encrypt_cohort below)

// a cohort's shared row names the type its layer is computed in
static int check_compute_row(flashe_ctx *ctx, int l, int32_t dtype)
{
    return dtype == FLASHE_TENSOR_F32 || dtype == FLASHE_TENSOR_F64
               ? FLASHE_OK : fail(ctx, FLASHE_EINVAL, "layer %d: the shared row names the COMPUTE type, FLASHE_TENSOR_F32 or FLASHE_TENSOR_F64", l);
}

// client c's source of layer l: a known storage dtype and, where the layer holds anything (needed), given and aligned to its element
// size.  same_class: of the shared row's compute class (the sparse cohorts; asked before the pointer); else only a float64 source under
// a float32 row is refused (the dense cohorts widen a float32 source in the stage pass; asked behind the pointer)
static int check_cohort_source(flashe_ctx *ctx, int c, int l, int32_t dtype, const void *p, bool row_f64, bool needed, bool same_class)
{
    const int es = tensor_elem_bytes(dtype);
    if (!es) return fail(ctx, FLASHE_EINVAL, "client %d layer %d: unknown dtype %d", c, l, static_cast<int>(dtype));
    if (same_class && (dtype == FLASHE_TENSOR_F64) != row_f64)
        return fail(ctx, FLASHE_EINVAL, "client %d layer %d: the source is of another compute class than the shared row", c, l);
    if (needed && (!p || reinterpret_cast<uintptr_t>(p) % static_cast<uintptr_t>(es)))
        return fail(ctx, FLASHE_EINVAL, "client %d layer %d: null or misaligned source", c, l);
    if (!same_class && dtype == FLASHE_TENSOR_F64 && !row_f64) return fail(ctx, FLASHE_EINVAL, "client %d layer %d: a float64 source under a float32 row", c, l);
    return FLASHE_OK;
}

// row_of = the non-empty layers of a cohort's shared table (the rows of the device table), each with a positive alpha and a compute dtype
static int cohort_rows(flashe_ctx *ctx, uint64_t n, const flashe_tensor_layer *layers, int n_layers, std::vector<int> &row_of)
{
    row_of.clear();
    for (int l = 0; l < n_layers; l++) {
        const flashe_tensor_layer &y = layers[l];
        if (y.start == layer_end(layers, n_layers, l, n)) continue;
        if (!(y.alpha > 0)) return fail(ctx, FLASHE_EINVAL, "layer %d: alpha must be positive", l);
        if (int rc = check_compute_row(ctx, l, y.dtype)) return rc;
        row_of.push_back(l);
    }
    return FLASHE_OK;
}

// rows of the device table (non-empty layers), the sources behind them, and ONE stage pass for every source that is not read in place
// (extra / extra_dev: a further small block for the same launch, uploaded behind the table -- the sparse cohort's 'zzz' values; rows: what
// cohort_rows gave a caller that has asked already)
static int cohort_stage(flashe_ctx *ctx, int n_clients, uint64_t n, const flashe_tensor_layer *layers, int n_layers, const void *const *src_dev,
                        const int32_t *src_dtype, int element_bits, CohortCodec &cc, const void *extra = nullptr, size_t extra_bytes = 0,
                        const char **extra_dev = nullptr, const std::vector<int> *rows = nullptr)
{
    int rc;
    std::vector<int> own_rows;
    if (!rows && (rc = cohort_rows(ctx, n, layers, n_layers, own_rows))) return rc;
    const std::vector<int> &row_of = rows ? *rows : own_rows;
    std::vector<CodecLayer> tab;
    for (const int l : row_of) {
        const flashe_tensor_layer &y = layers[l];
        tab.push_back(codec_layer_front(y.start, nullptr, y.dtype == FLASHE_TENSOR_F64 || (y.flags & FLASHE_TENSOR_LOOP_F64), y.alpha, element_bits));
    }
    const size_t n_tab = tab.size();
    std::vector<const void *> src(static_cast<size_t>(n_clients) * n_tab);
    StagePass sp;
    std::vector<size_t> staged;                 // the entry of src behind every slot of the stage pass
    for (int c = 0; c < n_clients; c++)
        for (size_t r = 0; r < n_tab; r++) {
            const int l = row_of[r];
            const flashe_tensor_layer &y = layers[l];
            const size_t at = static_cast<size_t>(c) * n_layers + l;
            const int32_t dt = src_dtype ? src_dtype[at] : y.dtype;
            const void *p = src_dev[at];
            const bool f64 = tab[r].x_is_f64 != 0;
            if ((rc = check_cohort_source(ctx, c, l, dt, p, f64, true, false))) return rc;
            const bool direct = !(y.flags & FLASHE_TENSOR_SHIFT) && (dt == FLASHE_TENSOR_F64 || (dt == FLASHE_TENSOR_F32 && !f64));
            src[static_cast<size_t>(c) * n_tab + r] = p;
            if (direct) continue;
            sp.add(p, dt, y.shift, y.flags & (FLASHE_TENSOR_SHIFT | FLASHE_TENSOR_SHIFT_WIDE), layer_end(layers, n_layers, l, n) - y.start, f64);
            staged.push_back(static_cast<size_t>(c) * n_tab + r);
        }
    if ((rc = sp.place(ctx))) return rc;
    for (size_t i = 0; i < staged.size(); i++) src[staged[i]] = sp.st[i].dst;
    // one block in ctx->codec_tab: the rows, then the source pointers, then the caller's extra block
    flashe_tables::Blob blob;
    blob.add(tab.data(), n_tab * sizeof(CodecLayer));
    const size_t src_at = blob.add(src.data(), src.size() * sizeof(void *));
    const size_t extra_at = extra ? blob.add(extra, extra_bytes) : 0;
    const char *blob_dev = nullptr;
    if ((rc = upload_tab(ctx, ctx->codec_tab, blob.bytes, &blob_dev))) return rc;
    if (extra_dev) *extra_dev = blob_dev + extra_at;
    if ((rc = sp.run(ctx))) return rc;
    cc.layers = reinterpret_cast<const CodecLayer *>(blob_dev);
    cc.src = reinterpret_cast<const void *const *>(blob_dev + src_at);
    cc.n_layers = static_cast<int>(n_tab);
    return FLASHE_OK;
}

// the outputs of a double-mask cohort: every client's ciphertext non-null, aligned for its element type (uint64: a two-limb vector's 16
// bytes, check_prf_args; uint32: 4 bytes) and apart from the sum and the mask, then the sum and the mask themselves
extern "C++" template <class T> static int cohort_check_outs(flashe_ctx *ctx, int n_clients, uint32_t n_jobs, T *const *ct_dev, const T *sum_out_dev, const T *dmask_dev)
{
    constexpr bool wide = sizeof(T) == 8;
    for (int c = 0; c < n_clients; c++) {
        if (!ct_dev[c]) return fail(ctx, FLASHE_EINVAL, "client %d: null ciphertext", c);
        if constexpr (wide) {
            if (int rc = check_prf_args(ctx, 1, 1, n_jobs, ct_dev[c], nullptr, 0)) return rc;
        } else if (reinterpret_cast<uintptr_t>(ct_dev[c]) & 3u)
            return fail(ctx, FLASHE_EINVAL, "client %d: the ciphertext is not 4-byte aligned", c);
        if (ct_dev[c] == sum_out_dev || ct_dev[c] == dmask_dev)
            return fail(ctx, FLASHE_EINVAL, "client %d: the ciphertext aliases the sum%s", c, wide ? " or the mask" : "");
    }
    if constexpr (!wide) return (reinterpret_cast<uintptr_t>(sum_out_dev) & 3u) ? fail(ctx, FLASHE_EINVAL, "sum_out_dev must be 4-byte aligned") : FLASHE_OK;
    if (int rc = check_sum_aligned(ctx, sum_out_dev)) return rc;
    if (dmask_dev && (!aligned16(dmask_dev) || dmask_dev == sum_out_dev)) return fail(ctx, FLASHE_EINVAL, "dmask_dev must be 16-byte aligned and apart from the sum");
    return FLASHE_OK;
}

// A shape the chained launch `what` does not take: asked of the launcher's own predicate before anything is staged, and once more of the
// launcher's answer (hipErrorNotSupported = nothing launched), which is the final word.
static int cohort_declined(flashe_ctx *ctx, const char *who, const char *what)
{
    return fail(ctx, FLASHE_ENOTSUP, "%s: not a shape of the chained %s launch", who, what);
}
static int cohort_launched(flashe_ctx *ctx, hipError_t e, const char *who, const char *what)
{
    if (e == hipErrorNotSupported) return cohort_declined(ctx, who, what);
    HIP_TRY(ctx, e);
    return FLASHE_OK;
}

// the scratch of a cut launch: needed from two pieces upward, 16-byte aligned, and none of the launch's outputs
static int cohort_check_scratch(flashe_ctx *ctx, int parts, int n_clients, const void *scratch_dev, const void *const *ct_dev, const void *sum_out_dev,
                                const void *dmask_dev)
{
    if (!scratch_dev) return parts > 1 ? fail(ctx, FLASHE_EINVAL, "scratch_dev is null: the launch runs %d pieces (flashe_cohort_cut_parts)", parts) : FLASHE_OK;
    if (!aligned16(scratch_dev)) return fail(ctx, FLASHE_EINVAL, "scratch_dev must be 16-byte aligned");
    if (scratch_dev == sum_out_dev || scratch_dev == dmask_dev) return fail(ctx, FLASHE_EINVAL, "scratch_dev aliases the sum or the mask");
    for (int c = 0; c < n_clients; c++)
        if (scratch_dev == ct_dev[c]) return fail(ctx, FLASHE_EINVAL, "scratch_dev aliases client %d's ciphertext", c);
    return FLASHE_OK;
}

// What tells the thirteen chained cohort entry points apart, besides the element type T of their vectors (uint64_t: the wide two-limb
// layout, or the one-limb layout of the `one_limb` form; uint32_t: the compact one, no decrypt mask).  `what` names the launch in a refusal.
struct CohortForm {
    const char *who, *what;
    bool by_list;            // the cipher indices: the list idx of the clients that report (the *_runs_* forms), else first_idx + c
    bool batched;            // a batched job: the table and sources over n_values values, the chain over n_elems batched elements
    bool cut;                // the short cohort (cohort_cut.h): no length rule, the chain cut into pieces, scratch_dev
    bool one_limb;           // int_bits 33 .. 64 in the one-limb layout (limb_cohort_admits): uint64 vectors, no decrypt mask
};

// The one body of those entry points, every step once and in the order the refusals are documented in: the arguments and the cipher
// indices (a list that needs more streams than one launch holds is not an error of the arguments but a shape the launch declines), the
// batched rows and their count, the outputs, the admission -- asked of the launcher's own predicate before anything is staged --, the
// scratch of a cut launch, the stage pass, and launch(idx, cc, cb) (cb: null unless batched).  Not batched: n_values == n_elems.
extern "C++" template <class T, class Launch>
static int quantize_encrypt_cohort(flashe_ctx *ctx, const CohortForm &f, uint32_t first_idx, const uint32_t *idx, int n_clients, uint64_t n_values,
                                   uint64_t n_elems, uint32_t n_jobs, const flashe_tensor_layer *layers, int n_layers, const void *const *src_dev,
                                   const int32_t *src_dtype, int element_bits, int field_bits, const double *u_dev, T *const *ct_dev, T *sum_out_dev,
                                   T *dmask_dev, T *scratch_dev, Launch launch)
{
    constexpr bool compact = sizeof(T) == 4;
    int rc = cohort_check_args(ctx, f.who, n_clients, n_values, layers, n_layers, src_dev, ct_dev && sum_out_dev && (idx || !f.by_list), element_bits, u_dev);
    if (rc) return rc;
    std::vector<uint32_t> consecutive;
    bool too_many = false;
    if (f.by_list) {
        // strictly ascending and below 2^32 - 1 (cohort_streams.h)
        flashe_tables::CohortStreams st;
        const flashe_tables::CohortStreamsStatus v = flashe_tables::cohort_streams(idx, n_clients, flashe_tables::kCohortMaxStreams, st);
        if (v == flashe_tables::kCohortStreamsBadIdx)
            return fail(ctx, FLASHE_EINVAL, "%s: the cipher indices must be strictly ascending and below 2^32 - 1 (idx + 1 has to fit the 4-byte prefix field, jzf_flashe.py:352-353)", f.who);
        too_many = v == flashe_tables::kCohortStreamsTooMany;
    } else {
        consecutive.resize(static_cast<size_t>(n_clients));
        for (int c = 0; c < n_clients; c++) {
            consecutive[c] = first_idx + static_cast<uint32_t>(c);
            if (consecutive[c] < first_idx) return fail(ctx, FLASHE_EINVAL, "the cohort's cipher indices wrap around 2^32");
        }
        idx = consecutive.data();
        if ((rc = check_double_idx(ctx, FLASHE_SCHEME_DOUBLE, idx, n_clients))) return rc;
    }
    // the batched rows of the non-empty layers (cohort_stage's rows, in its order): first element, value count
    uint64_t bs = 0;
    std::vector<uint64_t> rows;
    if (f.batched) {
        if ((rc = check_batch_bits(ctx, element_bits, field_bits, &bs))) return rc;
        auto size_of = [&](int l) { return layer_end(layers, n_layers, l, n_values) - layers[l].start; };
        const uint64_t e = flashe_tables::batched_elems(n_layers, bs, size_of, [&](int l, uint64_t elem, uint64_t) { rows.push_back(elem); rows.push_back(size_of(l)); });
        if ((rc = check_batched_count(ctx, e, n_elems))) return rc;
    }
    if (compact && n_jobs == 0) return fail(ctx, FLASHE_EINVAL, "n_jobs must be >= 1");
    if ((rc = cohort_check_outs<T>(ctx, n_clients, n_jobs, ct_dev, sum_out_dev, compact ? nullptr : dmask_dev))) return rc;
    // a cut launch answers with its pieces (consecutive clients: cohort_cut_parts_of; a list, where every gap is a cut: cohort_cut_pieces_of)
    const bool gated = too_many || (compact && flashe_ctx_compact_layout(ctx) != 1);
    int parts = 0, begins[flashe_tables::kCutMaxParts + 1];
    if (f.cut && !gated && !(f.batched && (bs < 5 || bs > 7)))
        parts = f.by_list ? cohort_cut_pieces_of(ctx->env, n_clients, idx, n_elems, n_jobs, compact, static_cast<int>(bs), begins)
                          : cohort_cut_parts_of(ctx->env, n_clients, n_elems, n_jobs, compact);
    const bool admitted = f.cut ? parts != 0
                                : !gated && (compact      ? small_cohort_admits(ctx->env, n_clients, n_elems, n_jobs, true)
                                             : f.one_limb ? limb_cohort_admits(ctx->env, n_clients, n_elems, n_jobs)
                                                          : cohort_chain_admits(ctx->env, n_clients, n_elems, static_cast<int>(bs)));
    if (!admitted) return cohort_declined(ctx, f.who, f.what);
    if (f.cut && (rc = cohort_check_scratch(ctx, parts, n_clients, scratch_dev, reinterpret_cast<const void *const *>(ct_dev), sum_out_dev,
                                            compact ? nullptr : dmask_dev)))
        return rc;
    CohortCodec cc{};
    const char *rows_dev = nullptr;
    if ((rc = cohort_stage(ctx, n_clients, n_values, layers, n_layers, src_dev, src_dtype, element_bits, cc, f.batched ? rows.data() : nullptr,
                           rows.size() * sizeof(uint64_t), &rows_dev)))
        return rc;
    CohortBatch cb{};
    cb.rows = reinterpret_cast<const uint64_t *>(rows_dev);
    cb.n_values = n_values;
    cb.field_bits = field_bits;
    return cohort_launched(ctx, launch(idx, cc, f.batched ? &cb : nullptr), f.who, f.what);
}

int flashe_quantize_encrypt_cohort_dev(flashe_ctx *ctx, uint32_t iter, uint32_t first_idx, int n_clients, uint64_t n, uint32_t n_jobs,
                                       const flashe_tensor_layer *layers, int n_layers, const void *const *src_dev, const int32_t *src_dtype,
                                       int element_bits, const double *u_dev, uint64_t *const *ct_dev, uint64_t *sum_out_dev, uint64_t *dmask_dev)
{
    CHECK_CTX(ctx);
    return quantize_encrypt_cohort<uint64_t>(
        ctx, {"flashe_quantize_encrypt_cohort_dev", "cohort", false, false, false}, first_idx, nullptr, n_clients, n, n, n_jobs, layers, n_layers, src_dev,
        src_dtype, element_bits, 0, u_dev, ct_dev, sum_out_dev, dmask_dev, nullptr, [&](const uint32_t *ids, const CohortCodec &cc, const CohortBatch *) {
            return launch_prf_cohort_sum(ctx->env, iter, n_clients, ids, cc, nullptr, u_dev, ct_dev, sum_out_dev, n, n_jobs, dmask_dev);
        });
}

// the same cohort in the compact layout at int_bits <= 32 (prf_small_cohort_kernel): uint32 ciphertexts and their uint32 sum, no decrypt mask
int flashe_quantize_encrypt_cohort_u32_dev(flashe_ctx *ctx, uint32_t iter, uint32_t first_idx, int n_clients, uint64_t n, uint32_t n_jobs,
                                           const flashe_tensor_layer *layers, int n_layers, const void *const *src_dev, const int32_t *src_dtype,
                                           int element_bits, const double *u_dev, uint32_t *const *ct_dev, uint32_t *sum_out_dev)
{
    CHECK_CTX(ctx);
    return quantize_encrypt_cohort<uint32_t>(
        ctx, {"flashe_quantize_encrypt_cohort_u32_dev", "compact cohort", false, false, false}, first_idx, nullptr, n_clients, n, n, n_jobs, layers, n_layers,
        src_dev, src_dtype, element_bits, 0, u_dev, ct_dev, sum_out_dev, nullptr, nullptr, [&](const uint32_t *ids, const CohortCodec &cc, const CohortBatch *) {
            return launch_small_cohort_sum(ctx->env, iter, n_clients, ids, cc, u_dev, ct_dev, sum_out_dev, n, n_jobs);
        });
}

// the same cohort in the one-limb layout at int_bits 33 .. 64 (prf_limb_cohort_kernel): uint64 ciphertexts and their uint64 sum, no decrypt mask
int flashe_quantize_encrypt_cohort_u64_dev(flashe_ctx *ctx, uint32_t iter, uint32_t first_idx, int n_clients, uint64_t n, uint32_t n_jobs,
                                           const flashe_tensor_layer *layers, int n_layers, const void *const *src_dev, const int32_t *src_dtype,
                                           int element_bits, const double *u_dev, uint64_t *const *ct_dev, uint64_t *sum_out_dev)
{
    CHECK_CTX(ctx);
    return quantize_encrypt_cohort<uint64_t>(
        ctx, {"flashe_quantize_encrypt_cohort_u64_dev", "one-limb cohort", false, false, false, true}, first_idx, nullptr, n_clients, n, n, n_jobs, layers, n_layers,
        src_dev, src_dtype, element_bits, 0, u_dev, ct_dev, sum_out_dev, nullptr, nullptr, [&](const uint32_t *ids, const CohortCodec &cc, const CohortBatch *) {
            return launch_limb_cohort_sum(ctx->env, iter, n_clients, ids, cc, u_dev, ct_dev, sum_out_dev, n, n_jobs);
        });
}

// the cohort of a BATCHED job (prf_chain_cohort_batch_kernel): the same table, sources and stage pass over the n_values values; the chain
// runs over the n_elems batched elements
int flashe_quantize_batch_encrypt_cohort_dev(flashe_ctx *ctx, uint32_t iter, uint32_t first_idx, int n_clients, uint64_t n_values, uint64_t n_elems,
                                             uint32_t n_jobs, const flashe_tensor_layer *layers, int n_layers, const void *const *src_dev,
                                             const int32_t *src_dtype, int element_bits, int field_bits, const double *u_dev, uint64_t *const *ct_dev,
                                             uint64_t *sum_out_dev, uint64_t *dmask_dev)
{
    CHECK_CTX(ctx);
    return quantize_encrypt_cohort<uint64_t>(
        ctx, {"flashe_quantize_batch_encrypt_cohort_dev", "batched cohort", false, true, false}, first_idx, nullptr, n_clients, n_values, n_elems, n_jobs, layers,
        n_layers, src_dev, src_dtype, element_bits, field_bits, u_dev, ct_dev, sum_out_dev, dmask_dev, nullptr,
        [&](const uint32_t *ids, const CohortCodec &cc, const CohortBatch *cb) {
            return launch_prf_cohort_sum(ctx->env, iter, n_clients, ids, cc, cb, u_dev, ct_dev, sum_out_dev, n_elems, n_jobs, dmask_dev);
        });
}

// ---- the same four launches for a round in which clients DROPPED OUT: the cipher indices of the clients that report, any strictly
// ascending list (one run: the launches above, bit for bit; several runs: prf_chain_cohort_runs_kernel / prf_small_cohort_runs_kernel /
// prf_limb_cohort_runs_kernel / prf_chain_cohort_batch_runs_kernel) ----
int flashe_quantize_encrypt_cohort_runs_dev(flashe_ctx *ctx, uint32_t iter, const uint32_t *idx, int n_clients, uint64_t n, uint32_t n_jobs,
                                            const flashe_tensor_layer *layers, int n_layers, const void *const *src_dev, const int32_t *src_dtype,
                                            int element_bits, const double *u_dev, uint64_t *const *ct_dev, uint64_t *sum_out_dev, uint64_t *dmask_dev)
{
    CHECK_CTX(ctx);
    return quantize_encrypt_cohort<uint64_t>(
        ctx, {"flashe_quantize_encrypt_cohort_runs_dev", "cohort", true, false, false}, 0, idx, n_clients, n, n, n_jobs, layers, n_layers, src_dev, src_dtype,
        element_bits, 0, u_dev, ct_dev, sum_out_dev, dmask_dev, nullptr, [&](const uint32_t *ids, const CohortCodec &cc, const CohortBatch *) {
            return launch_prf_cohort_sum(ctx->env, iter, n_clients, ids, cc, nullptr, u_dev, ct_dev, sum_out_dev, n, n_jobs, dmask_dev);
        });
}

int flashe_quantize_encrypt_cohort_runs_u32_dev(flashe_ctx *ctx, uint32_t iter, const uint32_t *idx, int n_clients, uint64_t n, uint32_t n_jobs,
                                                const flashe_tensor_layer *layers, int n_layers, const void *const *src_dev, const int32_t *src_dtype,
                                                int element_bits, const double *u_dev, uint32_t *const *ct_dev, uint32_t *sum_out_dev)
{
    CHECK_CTX(ctx);
    return quantize_encrypt_cohort<uint32_t>(
        ctx, {"flashe_quantize_encrypt_cohort_runs_u32_dev", "compact cohort", true, false, false}, 0, idx, n_clients, n, n, n_jobs, layers, n_layers, src_dev,
        src_dtype, element_bits, 0, u_dev, ct_dev, sum_out_dev, nullptr, nullptr, [&](const uint32_t *ids, const CohortCodec &cc, const CohortBatch *) {
            return launch_small_cohort_sum(ctx->env, iter, n_clients, ids, cc, u_dev, ct_dev, sum_out_dev, n, n_jobs);
        });
}

// the one-limb layout at int_bits 33 .. 64 (several runs: prf_limb_cohort_runs_kernel): uint64 ciphertexts and their uint64 sum, no decrypt mask
int flashe_quantize_encrypt_cohort_runs_u64_dev(flashe_ctx *ctx, uint32_t iter, const uint32_t *idx, int n_clients, uint64_t n, uint32_t n_jobs,
                                                const flashe_tensor_layer *layers, int n_layers, const void *const *src_dev, const int32_t *src_dtype,
                                                int element_bits, const double *u_dev, uint64_t *const *ct_dev, uint64_t *sum_out_dev)
{
    CHECK_CTX(ctx);
    return quantize_encrypt_cohort<uint64_t>(
        ctx, {"flashe_quantize_encrypt_cohort_runs_u64_dev", "one-limb cohort", true, false, false, true}, 0, idx, n_clients, n, n, n_jobs, layers, n_layers, src_dev,
        src_dtype, element_bits, 0, u_dev, ct_dev, sum_out_dev, nullptr, nullptr, [&](const uint32_t *ids, const CohortCodec &cc, const CohortBatch *) {
            return launch_limb_cohort_sum(ctx->env, iter, n_clients, ids, cc, u_dev, ct_dev, sum_out_dev, n, n_jobs);
        });
}

int flashe_quantize_batch_encrypt_cohort_runs_dev(flashe_ctx *ctx, uint32_t iter, const uint32_t *idx, int n_clients, uint64_t n_values, uint64_t n_elems,
                                                  uint32_t n_jobs, const flashe_tensor_layer *layers, int n_layers, const void *const *src_dev,
                                                  const int32_t *src_dtype, int element_bits, int field_bits, const double *u_dev, uint64_t *const *ct_dev,
                                                  uint64_t *sum_out_dev, uint64_t *dmask_dev)
{
    CHECK_CTX(ctx);
    return quantize_encrypt_cohort<uint64_t>(
        ctx, {"flashe_quantize_batch_encrypt_cohort_runs_dev", "batched cohort", true, true, false}, 0, idx, n_clients, n_values, n_elems, n_jobs, layers,
        n_layers, src_dev, src_dtype, element_bits, field_bits, u_dev, ct_dev, sum_out_dev, dmask_dev, nullptr,
        [&](const uint32_t *ids, const CohortCodec &cc, const CohortBatch *cb) {
            return launch_prf_cohort_sum(ctx->env, iter, n_clients, ids, cc, cb, u_dev, ct_dev, sum_out_dev, n_elems, n_jobs, dmask_dev);
        });
}

// ---- the SHORT cohort: the two launches above for a vector that does not fill the chip uncut (cohort_cut.h) -- the chain cut into runs of
// consecutive clients, their sums and decrypt masks added up by one combine pass.  The twins' checks, stage pass and refusals; the
// admission is theirs without the length rule ----
int flashe_cohort_cut_parts(flashe_ctx *ctx, int n_clients, uint64_t n, uint32_t n_jobs, int compact, int *parts)
{
    CHECK_CTX(ctx);
    static const char who[] = "flashe_cohort_cut_parts";
    if (!parts) return fail(ctx, FLASHE_EINVAL, "%s: null argument", who);
    *parts = 0;
    if (n_clients < 1) return fail(ctx, FLASHE_EINVAL, "%s: n_clients must be >= 1", who);
    if (compact && n_jobs == 0) return fail(ctx, FLASHE_EINVAL, "n_jobs must be >= 1");
    const int k = compact && flashe_ctx_compact_layout(ctx) != 1 ? 0 : cohort_cut_parts_of(ctx->env, n_clients, n, n_jobs, compact != 0);
    if (!k) return cohort_declined(ctx, who, compact ? "cut compact cohort" : "cut cohort");
    *parts = k;
    return FLASHE_OK;
}

// ---- the SHORT cohort for any strictly ascending cipher indices in at most kCutMaxParts runs, and for a batched job (cohort_cut_pieces,
// cohort_cut.h: every gap is a cut): the _runs_ entry points' checks, the _cut_ entry points' scratch and admission ----
int flashe_cohort_cut_pieces(flashe_ctx *ctx, const uint32_t *idx, int n_clients, uint64_t n, uint32_t n_jobs, int compact, int *parts, int *begins)
{
    CHECK_CTX(ctx);
    static const char who[] = "flashe_cohort_cut_pieces";
    if (!parts) return fail(ctx, FLASHE_EINVAL, "%s: null argument", who);
    *parts = 0;
    if (n_clients < 1) return fail(ctx, FLASHE_EINVAL, "%s: n_clients must be >= 1", who);
    if (compact && n_jobs == 0) return fail(ctx, FLASHE_EINVAL, "n_jobs must be >= 1");
    flashe_tables::CohortStreams st;
    if (flashe_tables::cohort_streams(idx, n_clients, 2 * n_clients, st) == flashe_tables::kCohortStreamsBadIdx)
        return fail(ctx, FLASHE_EINVAL, "%s: the cipher indices must be strictly ascending and below 2^32 - 1", who);
    int own[flashe_tables::kCutMaxParts + 1];
    const int k = compact && flashe_ctx_compact_layout(ctx) != 1 ? 0 : cohort_cut_pieces_of(ctx->env, n_clients, idx, n, n_jobs, compact != 0, 0, own);
    if (!k) return cohort_declined(ctx, who, compact ? "cut compact cohort" : "cut cohort");
    *parts = k;
    if (begins) for (int p = 0; p <= k; p++) begins[p] = own[p];
    return FLASHE_OK;
}

int flashe_quantize_encrypt_cohort_cut_dev(flashe_ctx *ctx, uint32_t iter, uint32_t first_idx, int n_clients, uint64_t n, uint32_t n_jobs,
                                           const flashe_tensor_layer *layers, int n_layers, const void *const *src_dev, const int32_t *src_dtype,
                                           int element_bits, const double *u_dev, uint64_t *const *ct_dev, uint64_t *sum_out_dev, uint64_t *dmask_dev,
                                           uint64_t *scratch_dev)
{
    CHECK_CTX(ctx);
    return quantize_encrypt_cohort<uint64_t>(
        ctx, {"flashe_quantize_encrypt_cohort_cut_dev", "cut cohort", false, false, true}, first_idx, nullptr, n_clients, n, n, n_jobs, layers, n_layers, src_dev,
        src_dtype, element_bits, 0, u_dev, ct_dev, sum_out_dev, dmask_dev, scratch_dev, [&](const uint32_t *ids, const CohortCodec &cc, const CohortBatch *) {
            return launch_prf_cohort_cut(ctx->env, iter, n_clients, ids, cc, u_dev, ct_dev, sum_out_dev, n, n_jobs, dmask_dev, scratch_dev);
        });
}

int flashe_quantize_encrypt_cohort_cut_u32_dev(flashe_ctx *ctx, uint32_t iter, uint32_t first_idx, int n_clients, uint64_t n, uint32_t n_jobs,
                                               const flashe_tensor_layer *layers, int n_layers, const void *const *src_dev, const int32_t *src_dtype,
                                               int element_bits, const double *u_dev, uint32_t *const *ct_dev, uint32_t *sum_out_dev, uint32_t *scratch_dev)
{
    CHECK_CTX(ctx);
    return quantize_encrypt_cohort<uint32_t>(
        ctx, {"flashe_quantize_encrypt_cohort_cut_u32_dev", "cut compact cohort", false, false, true}, first_idx, nullptr, n_clients, n, n, n_jobs, layers,
        n_layers, src_dev, src_dtype, element_bits, 0, u_dev, ct_dev, sum_out_dev, nullptr, scratch_dev,
        [&](const uint32_t *ids, const CohortCodec &cc, const CohortBatch *) {
            return launch_small_cohort_cut(ctx->env, iter, n_clients, ids, cc, u_dev, ct_dev, sum_out_dev, n, n_jobs, scratch_dev);
        });
}

int flashe_quantize_encrypt_cohort_cut_runs_dev(flashe_ctx *ctx, uint32_t iter, const uint32_t *idx, int n_clients, uint64_t n, uint32_t n_jobs,
                                                const flashe_tensor_layer *layers, int n_layers, const void *const *src_dev, const int32_t *src_dtype,
                                                int element_bits, const double *u_dev, uint64_t *const *ct_dev, uint64_t *sum_out_dev,
                                                uint64_t *dmask_dev, uint64_t *scratch_dev)
{
    CHECK_CTX(ctx);
    return quantize_encrypt_cohort<uint64_t>(
        ctx, {"flashe_quantize_encrypt_cohort_cut_runs_dev", "cut cohort", true, false, true}, 0, idx, n_clients, n, n, n_jobs, layers, n_layers, src_dev,
        src_dtype, element_bits, 0, u_dev, ct_dev, sum_out_dev, dmask_dev, scratch_dev, [&](const uint32_t *ids, const CohortCodec &cc, const CohortBatch *) {
            return launch_prf_cohort_cut(ctx->env, iter, n_clients, ids, cc, u_dev, ct_dev, sum_out_dev, n, n_jobs, dmask_dev, scratch_dev);
        });
}

int flashe_quantize_encrypt_cohort_cut_runs_u32_dev(flashe_ctx *ctx, uint32_t iter, const uint32_t *idx, int n_clients, uint64_t n, uint32_t n_jobs,
                                                    const flashe_tensor_layer *layers, int n_layers, const void *const *src_dev,
                                                    const int32_t *src_dtype, int element_bits, const double *u_dev, uint32_t *const *ct_dev,
                                                    uint32_t *sum_out_dev, uint32_t *scratch_dev)
{
    CHECK_CTX(ctx);
    return quantize_encrypt_cohort<uint32_t>(
        ctx, {"flashe_quantize_encrypt_cohort_cut_runs_u32_dev", "cut compact cohort", true, false, true}, 0, idx, n_clients, n, n, n_jobs, layers, n_layers,
        src_dev, src_dtype, element_bits, 0, u_dev, ct_dev, sum_out_dev, nullptr, scratch_dev,
        [&](const uint32_t *ids, const CohortCodec &cc, const CohortBatch *) {
            return launch_small_cohort_cut(ctx->env, iter, n_clients, ids, cc, u_dev, ct_dev, sum_out_dev, n, n_jobs, scratch_dev);
        });
}

int flashe_quantize_batch_encrypt_cohort_cut_runs_dev(flashe_ctx *ctx, uint32_t iter, const uint32_t *idx, int n_clients, uint64_t n_values,
                                                      uint64_t n_elems, uint32_t n_jobs, const flashe_tensor_layer *layers, int n_layers,
                                                      const void *const *src_dev, const int32_t *src_dtype, int element_bits, int field_bits,
                                                      const double *u_dev, uint64_t *const *ct_dev, uint64_t *sum_out_dev, uint64_t *dmask_dev,
                                                      uint64_t *scratch_dev)
{
    CHECK_CTX(ctx);
    return quantize_encrypt_cohort<uint64_t>(
        ctx, {"flashe_quantize_batch_encrypt_cohort_cut_runs_dev", "cut batched cohort", true, true, true}, 0, idx, n_clients, n_values, n_elems, n_jobs, layers,
        n_layers, src_dev, src_dtype, element_bits, field_bits, u_dev, ct_dev, sum_out_dev, dmask_dev, scratch_dev,
        [&](const uint32_t *ids, const CohortCodec &cc, const CohortBatch *cb) {
            return launch_prf_cohort_batch_cut(ctx->env, iter, n_clients, ids, cc, *cb, u_dev, ct_dev, sum_out_dev, n_elems, n_jobs, dmask_dev, scratch_dev);
        });
}

// ---- the cohort's ONLINE step with masks the caller holds (a precompute job's cohort: the mask chain ran in idle time) ----
// What tells the eight entry points apart, besides where their draws come from: what masks, ciphertexts and sum are made of, and whether
// the job is batched (then the table and the draws are over n_values values and the launch over the n_elems batched elements).
struct PrepForm { const char *who; int elem_bytes; bool batched; };
// the draw plans of a form that draws inside the launch: one row per client (flashe_philox::ClientPlan, or flashe_pcg64::ClientPlan of the one variant)
struct DrawPlans { PrepDraws::Kind kind; const void *rows; size_t count, row_bytes; uint32_t variant; };

// The one body, every step once and in the order of its refusals:
//    1. n_clients < 1
//    2. drawn forms: the segment table's own refusals (flashe_draw::read_segments: its count, a null table, a capture, check_segments)
//    3. drawn forms: the plan statuses -- overflow, not tiled, split client and, for PCG64, mixed variants
//    4. null argument
//    5. element_bits
//    6. u_dev's alignment
//    7. the layer table
//    8. batched: the batch bits, then the batched count
//    9. per client: null, then misaligned, then the sum aliases its mask or ciphertext
//   10. the sum's alignment
//   11. the sum aliases a source
//   12. the compact layout declined (FLASHE_ENOTSUP)
//   13. the empty model: FLASHE_OK with nothing staged
//   14. stage: cohort_stage's table, sources and stage pass, with the block of flashe_tables::prepared_block behind them in the same upload
//   15. launch (launch_prep_cohort)
//   16. drawn forms: the caller's segments advance -- after the launch has been made, and only when n != 0
// Steps 2, 3 and 16 are quantize_combine_cohort_drawn's, below.  plans: the launch generates the draws and u_dev is not read.
static int quantize_combine_cohort(flashe_ctx *ctx, const PrepForm &f, int n_clients, uint64_t n_values, uint64_t n_elems_arg, const flashe_tensor_layer *layers,
                                   int n_layers, const void *const *src_dev, const int32_t *src_dtype, int element_bits, int field_bits, const double *u_dev,
                                   const void *const *mask_dev, void *const *ct_dev, void *sum_out_dev, const DrawPlans *plans = nullptr)
{
    if (n_clients < 1) return fail(ctx, FLASHE_EINVAL, "%s: n_clients must be >= 1", f.who);
    if (!src_dev || !mask_dev || !ct_dev || (n_values && !u_dev && !plans)) return fail(ctx, FLASHE_EINVAL, "%s: null argument", f.who);
    int rc = check_element_bits(ctx, element_bits);
    if (rc || (rc = check_f64_aligned(ctx, u_dev, "u_dev")) || (rc = check_tensor_layers(ctx, n_values, layers, n_layers, false))) return rc;
    // the batched rows of the non-empty layers (cohort_stage's rows, in its order): first element, value count
    uint64_t bs = 1, n_elems = n_values;
    std::vector<uint64_t> rows;
    if (f.batched) {
        if ((rc = check_batch_bits(ctx, element_bits, field_bits, &bs))) return rc;
        auto size_of = [&](int l) { return layer_end(layers, n_layers, l, n_values) - layers[l].start; };
        n_elems = flashe_tables::batched_elems(n_layers, bs, size_of, [&](int l, uint64_t elem, uint64_t) { rows.push_back(elem); rows.push_back(size_of(l)); });
        if ((rc = check_batched_count(ctx, n_elems, n_elems_arg))) return rc;
    }
    const uintptr_t amask = static_cast<uintptr_t>(f.elem_bytes - 1);
    for (int c = 0; c < n_clients; c++) {
        if (n_elems && (!mask_dev[c] || !ct_dev[c])) return fail(ctx, FLASHE_EINVAL, "client %d: null mask or ciphertext", c);
        if ((reinterpret_cast<uintptr_t>(mask_dev[c]) | reinterpret_cast<uintptr_t>(ct_dev[c])) & amask)
            return fail(ctx, FLASHE_EINVAL, "client %d: the mask or the ciphertext is not %d-byte aligned", c, f.elem_bytes);
        if (sum_out_dev && (mask_dev[c] == sum_out_dev || ct_dev[c] == sum_out_dev)) return fail(ctx, FLASHE_EINVAL, "client %d: the sum aliases the mask or the ciphertext", c);
    }
    if (reinterpret_cast<uintptr_t>(sum_out_dev) & amask) return fail(ctx, FLASHE_EINVAL, "sum_out_dev must be %d-byte aligned", f.elem_bytes);
    if (sum_out_dev)
        for (size_t i = 0; i < flashe_tables::cohort_sources(n_clients, n_layers); i++)
            if (src_dev[i] == sum_out_dev) return fail(ctx, FLASHE_EINVAL, "the sum aliases a source (client %d layer %d)", static_cast<int>(i / n_layers), static_cast<int>(i % n_layers));
    if (f.elem_bytes == 4 && flashe_ctx_compact_layout(ctx) != 1) return cohort_declined(ctx, f.who, "prepared compact cohort");
    if (n_elems == 0) return FLASHE_OK;                                    // (an empty model: nothing staged, nothing launched)
    // the block behind cohort_stage's tables: the pointers, the rows, a batched drawn form's groups, the plans
    const bool grouped = plans && f.batched;
    const size_t n_rows = rows.size() / 2;
    const flashe_tables::PreparedBlock at = flashe_tables::prepared_block(n_clients, n_rows, plans ? plans->row_bytes / sizeof(uint64_t) : 0, grouped);
    std::vector<uint64_t> extra(at.words);
    for (int c = 0; c < n_clients; c++) {
        extra[at.mask / 8 + static_cast<size_t>(c)] = reinterpret_cast<uintptr_t>(mask_dev[c]);
        extra[at.ct / 8 + static_cast<size_t>(c)] = reinterpret_cast<uintptr_t>(ct_dev[c]);
    }
    std::copy(rows.begin(), rows.end(), extra.begin() + at.rows / 8);
    PrepDraws draws{plans ? plans->kind : PrepDraws::kBuffer, f.batched, nullptr, plans ? plans->variant : 0, nullptr, 0};
    if (grouped) draws.n_groups = flashe_tables::batched_groups(rows.data(), n_rows, bs, extra.data() + at.groups / 8);
    if (plans) memcpy(extra.data() + at.plans / 8, plans->rows, plans->count * plans->row_bytes);
    CohortCodec cc{};
    const char *extra_dev = nullptr;
    if ((rc = cohort_stage(ctx, n_clients, n_values, layers, n_layers, src_dev, src_dtype, element_bits, cc, extra.data(), extra.size() * sizeof(uint64_t), &extra_dev)))
        return rc;
    const bool no_rows = plans && !f.batched;      // (an un-batched drawn form reads neither rows nor bs: it keeps the null and the 0 it has been launched with)
    PrepCohort pc{};
    pc.layers = cc.layers; pc.src = cc.src; pc.n_layers = cc.n_layers;
    pc.mask = reinterpret_cast<const void *const *>(extra_dev + at.mask); pc.ct = reinterpret_cast<void *const *>(extra_dev + at.ct);
    pc.rows = no_rows ? nullptr : reinterpret_cast<const uint64_t *>(extra_dev + at.rows);
    pc.u = u_dev; pc.sum = sum_out_dev; pc.n = n_elems; pc.n_values = n_values; pc.n_clients = n_clients; pc.field_bits = field_bits; pc.bs = no_rows ? 0 : static_cast<int>(bs);
    if (plans) draws.plans = extra_dev + at.plans;
    if (grouped) draws.groups = reinterpret_cast<const uint64_t *>(extra_dev + at.groups);
    HIP_TRY(ctx, launch_prep_cohort(ctx->env, pc, draws, f.elem_bytes));
    return FLASHE_OK;
}

// What a kind of generator brings to the forms that draw inside the launch: its C segment and how it is read and checked
// (flashe_draw::read_segments; own_segment: its words for the kind's own refusal of a segment), its plans (own_plans: its words for the
// kind's own refusal of the table as a whole, none: it has no such status), and how a segment is advanced and handed back.
struct PhiloxKind {
    using CSegment = flashe_philox_segment; using Segment = flashe_philox::Segment; using Plan = flashe_philox::ClientPlan;
    static constexpr PrepDraws::Kind kind = PrepDraws::kPhilox;
    static constexpr const char *own_segment = "a buffer_pos above 4", *own_plans = nullptr;
    static constexpr auto from_c = flashe_philox::from_c<CSegment>;
    static constexpr flashe_draw::SegmentsStatus (*check_segments)(const Segment *, int, int) = flashe_philox::check_segments;
    static auto cohort_plans(const Segment *segs, int n_segs, uint64_t C, uint64_t n, std::vector<Plan> &plans, flashe_pcg64::Variant *)
    { return flashe_philox::cohort_plans(segs, n_segs, C, n, plans); }
    static void advance(CSegment &c, const Segment &) { flashe_philox::advance(c.key, c.counter, c.buffer_pos, c.buffer, c.n); }
};
struct Pcg64Kind {
    using CSegment = flashe_pcg64_segment; using Segment = flashe_pcg64::Segment; using Plan = flashe_pcg64::ClientPlan;
    static constexpr PrepDraws::Kind kind = PrepDraws::kPcg64;
    static constexpr const char *own_segment = "a variant that is neither PCG64 (0) nor PCG64DXSM (1)",
                                *own_plans = "PCG64 and PCG64DXSM segments in one table: a launch has one variant";
    static constexpr auto from_c = flashe_pcg64::from_c<CSegment>;
    static constexpr flashe_draw::SegmentsStatus (*check_segments)(const Segment *, int, int) = flashe_pcg64::check_segments;
    static auto cohort_plans(const Segment *segs, int n_segs, uint64_t C, uint64_t n, std::vector<Plan> &plans, flashe_pcg64::Variant *v)
    { return flashe_pcg64::cohort_plans(segs, n_segs, C, n, plans, v); }
    static void advance(CSegment &c, const Segment &s)
    {
        const flashe_pcg64::u128 a = flashe_pcg64::advance(static_cast<flashe_pcg64::Variant>(s.variant), s.state, s.inc, s.n);
        c.state[0] = flashe_pcg64::lo64(a); c.state[1] = flashe_pcg64::hi64(a);
    }
};

// The forms with the draws of the caller's generators generated inside the launch: the segment table's own refusals come first (those of
// the kind's flashe_*_random_dev, without a draw buffer), then the tiling of the clients' stretches, then quantize_combine_cohort's; one
// advance per segment on the host, after the launch has been made.  The segments tile the clients' n_values VALUES, batched or not.
extern "C++" template <class K>
static int quantize_combine_cohort_drawn(flashe_ctx *ctx, const PrepForm &f, int n_clients, uint64_t n_values, uint64_t n_elems_arg, const flashe_tensor_layer *layers,
                                         int n_layers, const void *const *src_dev, const int32_t *src_dtype, int element_bits, int field_bits,
                                         typename K::CSegment *segments, int n_segments, const void *const *mask_dev, void *const *ct_dev, void *sum_out_dev)
{
    if (n_clients < 1) return fail(ctx, FLASHE_EINVAL, "%s: n_clients must be >= 1", f.who);
    std::vector<typename K::Segment> segs;
    if (int rc = flashe_draw::read_segments(ctx, f.who, segments, n_segments, nullptr, K::from_c, K::check_segments, K::own_segment, segs, false)) return rc;
    std::vector<typename K::Plan> plans;
    flashe_pcg64::Variant variant = flashe_pcg64::kPcg64;
    switch (K::cohort_plans(segs.data(), n_segments, static_cast<uint64_t>(n_clients), n_values, plans, &variant)) {
    case flashe_draw::kCohortPlansOk: break;
    case flashe_draw::kCohortPlansSplitClient: return fail(ctx, FLASHE_EINVAL, "%s: a client's n draws must come from one segment", f.who);
    case flashe_draw::kCohortPlansTooMany: return fail(ctx, FLASHE_EINVAL, "%s: n_clients x n draws overflow", f.who);
    case flashe_draw::kCohortPlansOwn:
        if (K::own_plans) return fail(ctx, FLASHE_EINVAL, "%s: %s", f.who, K::own_plans);
        [[fallthrough]];
    default: return fail(ctx, FLASHE_EINVAL, "%s: the segments must tile the draws [0, n_clients x n) exactly", f.who);
    }
    const DrawPlans rows{K::kind, plans.data(), plans.size(), sizeof(typename K::Plan), variant};
    if (int rc = quantize_combine_cohort(ctx, f, n_clients, n_values, n_elems_arg, layers, n_layers, src_dev, src_dtype, element_bits, field_bits, nullptr, mask_dev,
                                         ct_dev, sum_out_dev, &rows))
        return rc;
    for (int s = 0; n_values && s < n_segments; s++) K::advance(segments[s], segs[s]);
    return FLASHE_OK;
}

// the vectors' element: a two-limb or a one-limb element of the ctx's layout; the _u32 forms': 4 bytes
static int prep_elem_bytes(const flashe_ctx *ctx) { return ctx->limbs == 2 ? 16 : 8; }
static const void *const *prep_in(const void *p) { return static_cast<const void *const *>(p); }
static void *const *prep_out(const void *p) { return static_cast<void *const *>(const_cast<void *>(p)); }

int flashe_quantize_combine_cohort_dev(flashe_ctx *ctx, int n_clients, uint64_t n, const flashe_tensor_layer *layers, int n_layers, const void *const *src_dev,
                                       const int32_t *src_dtype, int element_bits, const double *u_dev, const uint64_t *const *mask_dev,
                                       uint64_t *const *ct_dev, uint64_t *sum_out_dev)
{
    CHECK_CTX(ctx);
    return quantize_combine_cohort(ctx, {"flashe_quantize_combine_cohort_dev", prep_elem_bytes(ctx), false}, n_clients, n, n, layers, n_layers, src_dev, src_dtype,
                                   element_bits, 0, u_dev, prep_in(mask_dev), prep_out(ct_dev), sum_out_dev);
}

// the same in the compact layout at int_bits <= 32 (any such width: there is no AES here): uint32 masks, ciphertexts and sum
int flashe_quantize_combine_cohort_u32_dev(flashe_ctx *ctx, int n_clients, uint64_t n, const flashe_tensor_layer *layers, int n_layers, const void *const *src_dev,
                                           const int32_t *src_dtype, int element_bits, const double *u_dev, const uint32_t *const *mask_dev,
                                           uint32_t *const *ct_dev, uint32_t *sum_out_dev)
{
    CHECK_CTX(ctx);
    if (ctx->int_bits > 32) return fail(ctx, FLASHE_EINVAL, "the uint32 layout needs int_bits <= 32, this ctx has %d", ctx->int_bits);
    return quantize_combine_cohort(ctx, {"flashe_quantize_combine_cohort_u32_dev", 4, false}, n_clients, n, n, layers, n_layers, src_dev, src_dtype, element_bits, 0,
                                   u_dev, prep_in(mask_dev), prep_out(ct_dev), sum_out_dev);
}

// the BATCHED job over its n_elems elements (any bs = int_bits / field_bits >= 1)
int flashe_quantize_batch_combine_cohort_dev(flashe_ctx *ctx, int n_clients, uint64_t n_values, uint64_t n_elems, const flashe_tensor_layer *layers, int n_layers,
                                             const void *const *src_dev, const int32_t *src_dtype, int element_bits, int field_bits, const double *u_dev,
                                             const uint64_t *const *mask_dev, uint64_t *const *ct_dev, uint64_t *sum_out_dev)
{
    CHECK_CTX(ctx);
    return quantize_combine_cohort(ctx, {"flashe_quantize_batch_combine_cohort_dev", prep_elem_bytes(ctx), true}, n_clients, n_values, n_elems, layers, n_layers,
                                   src_dev, src_dtype, element_bits, field_bits, u_dev, prep_in(mask_dev), prep_out(ct_dev), sum_out_dev);
}

// the draws of np.random.Philox streams generated inside the launch
int flashe_quantize_combine_cohort_philox_dev(flashe_ctx *ctx, int n_clients, uint64_t n, const flashe_tensor_layer *layers, int n_layers, const void *const *src_dev,
                                              const int32_t *src_dtype, int element_bits, flashe_philox_segment *segments, int n_segments,
                                              const uint64_t *const *mask_dev, uint64_t *const *ct_dev, uint64_t *sum_out_dev)
{
    CHECK_CTX(ctx);
    return quantize_combine_cohort_drawn<PhiloxKind>(ctx, {"flashe_quantize_combine_cohort_philox_dev", prep_elem_bytes(ctx), false}, n_clients, n, n, layers, n_layers,
                                                     src_dev, src_dtype, element_bits, 0, segments, n_segments, prep_in(mask_dev), prep_out(ct_dev), sum_out_dev);
}

int flashe_quantize_combine_cohort_philox_u32_dev(flashe_ctx *ctx, int n_clients, uint64_t n, const flashe_tensor_layer *layers, int n_layers,
                                                  const void *const *src_dev, const int32_t *src_dtype, int element_bits, flashe_philox_segment *segments,
                                                  int n_segments, const uint32_t *const *mask_dev, uint32_t *const *ct_dev, uint32_t *sum_out_dev)
{
    CHECK_CTX(ctx);
    if (ctx->int_bits > 32) return fail(ctx, FLASHE_EINVAL, "the uint32 layout needs int_bits <= 32, this ctx has %d", ctx->int_bits);
    return quantize_combine_cohort_drawn<PhiloxKind>(ctx, {"flashe_quantize_combine_cohort_philox_u32_dev", 4, false}, n_clients, n, n, layers, n_layers, src_dev,
                                                     src_dtype, element_bits, 0, segments, n_segments, prep_in(mask_dev), prep_out(ct_dev), sum_out_dev);
}

// the BATCHED job with the draws generated inside the launch: the segments tile the clients' n_values values
int flashe_quantize_batch_combine_cohort_philox_dev(flashe_ctx *ctx, int n_clients, uint64_t n_values, uint64_t n_elems, const flashe_tensor_layer *layers, int n_layers,
                                                    const void *const *src_dev, const int32_t *src_dtype, int element_bits, int field_bits,
                                                    flashe_philox_segment *segments, int n_segments, const uint64_t *const *mask_dev, uint64_t *const *ct_dev,
                                                    uint64_t *sum_out_dev)
{
    CHECK_CTX(ctx);
    return quantize_combine_cohort_drawn<PhiloxKind>(ctx, {"flashe_quantize_batch_combine_cohort_philox_dev", prep_elem_bytes(ctx), true}, n_clients, n_values, n_elems,
                                                     layers, n_layers, src_dev, src_dtype, element_bits, field_bits, segments, n_segments, prep_in(mask_dev),
                                                     prep_out(ct_dev), sum_out_dev);
}

// the draws of np.random.PCG64 / PCG64DXSM streams generated inside the launch (un-batched only)
int flashe_quantize_combine_cohort_pcg64_dev(flashe_ctx *ctx, int n_clients, uint64_t n, const flashe_tensor_layer *layers, int n_layers, const void *const *src_dev,
                                             const int32_t *src_dtype, int element_bits, flashe_pcg64_segment *segments, int n_segments,
                                             const uint64_t *const *mask_dev, uint64_t *const *ct_dev, uint64_t *sum_out_dev)
{
    CHECK_CTX(ctx);
    return quantize_combine_cohort_drawn<Pcg64Kind>(ctx, {"flashe_quantize_combine_cohort_pcg64_dev", prep_elem_bytes(ctx), false}, n_clients, n, n, layers, n_layers,
                                                    src_dev, src_dtype, element_bits, 0, segments, n_segments, prep_in(mask_dev), prep_out(ct_dev), sum_out_dev);
}

int flashe_quantize_combine_cohort_pcg64_u32_dev(flashe_ctx *ctx, int n_clients, uint64_t n, const flashe_tensor_layer *layers, int n_layers,
                                                 const void *const *src_dev, const int32_t *src_dtype, int element_bits, flashe_pcg64_segment *segments,
                                                 int n_segments, const uint32_t *const *mask_dev, uint32_t *const *ct_dev, uint32_t *sum_out_dev)
{
    CHECK_CTX(ctx);
    if (ctx->int_bits > 32) return fail(ctx, FLASHE_EINVAL, "the uint32 layout needs int_bits <= 32, this ctx has %d", ctx->int_bits);
    return quantize_combine_cohort_drawn<Pcg64Kind>(ctx, {"flashe_quantize_combine_cohort_pcg64_u32_dev", 4, false}, n_clients, n, n, layers, n_layers, src_dev,
                                                    src_dtype, element_bits, 0, segments, n_segments, prep_in(mask_dev), prep_out(ct_dev), sum_out_dev);
}

// host only: the grid of that launch for n values, and one lane's draws through the header functions its kernel compiles
int flashe_pcg64_cohort_grid(flashe_ctx *ctx, uint64_t n, uint32_t *workgroups)
{
    if (!ctx || !workgroups || n > flashe_pcg64::kMaxDraws) return FLASHE_EINVAL;
    *workgroups = static_cast<uint32_t>(prep_pcg64_grid(ctx->env, n));
    return FLASHE_OK;
}

int flashe_pcg64_cohort_lane_draws(uint32_t variant, const uint64_t state[2], const uint64_t inc[2], uint64_t first, uint32_t workgroups, uint64_t run,
                                   uint64_t iterations, double *out)
{
    using namespace flashe_pcg64;
    if (!state || !inc || (iterations && !out) || variant >= kVariants || workgroups < 1 || run >= static_cast<uint64_t>(workgroups) * kLanes) return FLASHE_EINVAL;
    if (first > kMaxDraws || iterations > kMaxDraws / kRunDraws) return FLASHE_EINVAL;
    static const Pow2Table pow2[kVariants] = {make_pow2_table(kPcg64), make_pow2_table(kDxsm)};
    static const RunTable runs[kVariants] = {make_run_table(kPcg64), make_run_table(kDxsm)};
    Segment seg{make128(state[1], state[0]), make128(inc[1], inc[0]), variant, 0, 0};
    const ClientPlan plan = client_plan(seg, first);
    if (variant == kPcg64) lane_draws<kPcg64>(pow2[0], runs[0], plan, workgroups, run, iterations, out);
    else lane_draws<kDxsm>(pow2[1], runs[1], plan, workgroups, run, iterations, out);
    return FLASHE_OK;
}

int flashe_combine_unquantize_model_dev(flashe_ctx *ctx, uint64_t n, const uint64_t *in_dev, const uint64_t *add_dev, const uint64_t *minus_dev,
                                        const flashe_codec_layer *layers, int n_layers, int element_bits, int num_clients, double *out_dev)
{
    CHECK_CTX(ctx);
    if (n && (!in_dev || !out_dev)) return fail(ctx, FLASHE_EINVAL, "null vector");
    if (num_clients < 1) return fail(ctx, FLASHE_EINVAL, "num_clients must be >= 1");
    int rc = check_codec_bits(ctx, element_bits);
    if (rc || (rc = check_vec_aligned(ctx, {in_dev, add_dev, minus_dev})) || (rc = check_f64_aligned(ctx, out_dev, "out_dev"))) return rc;
    Codec cq{};
    if ((rc = stage_codec_layers(ctx, n, layers, n_layers, false, element_bits, num_clients, 0, n, nullptr, out_dev, &cq)) || n == 0) return rc;
    HIP_TRY(ctx, launch_combine_unquantize_model(ctx->env, n, in_dev, add_dev, minus_dev, cq, out_dev));
    return FLASHE_OK;
}

// the batched sibling: unbatch + unquantise over (in + add - minus) mod 2^b, the masks held by the caller
int flashe_combine_unbatch_unquantize_model_dev(flashe_ctx *ctx, const flashe_batch_layer *layers, int n_layers, int element_bits, int field_bits,
                                                int num_clients, const uint64_t *in_dev, const uint64_t *add_dev, const uint64_t *minus_dev,
                                                uint64_t n_elems, double *out_dev)
{
    CHECK_CTX(ctx);
    if (num_clients < 1) return fail(ctx, FLASHE_EINVAL, "num_clients must be >= 1");
    BatchTab bt;
    int rc = stage_batch_layers(ctx, layers, n_layers, false, element_bits, field_bits, num_clients, n_elems, &bt);
    if (rc) return rc;
    if (bt.n_values && (!in_dev || !out_dev)) return fail(ctx, FLASHE_EINVAL, "null vector");
    if ((rc = check_vec_aligned(ctx, {in_dev, add_dev, minus_dev})) || (rc = check_f64_aligned(ctx, out_dev, "out_dev"))) return rc;
    if (bt.n_values) HIP_TRY(ctx, launch_combine_unbatch_unquantize_model(ctx->env, bt.tab, bt.n_tab, field_bits, in_dev, add_dev, minus_dev, bt.n_values, out_dev));
    return FLASHE_OK;
}

int flashe_quantize_batch_tensors_dev(flashe_ctx *ctx, const flashe_tensor_layer *layers, int n_layers, uint64_t n_values, int element_bits,
                                      int field_bits, const double *u_dev, uint64_t n_elems, uint64_t *out_dev)
{
    CHECK_CTX(ctx);
    int rc = check_tensor_layers(ctx, n_values, layers, n_layers, true);
    std::vector<flashe_batch_layer> bl;
    if (rc || (rc = tensor_batch_layers(ctx, layers, n_layers, n_values, element_bits, field_bits, u_dev, n_elems, out_dev, bl))) return rc;
    return flashe_quantize_batch_model_dev(ctx, bl.data(), n_layers, element_bits, field_bits, u_dev, n_elems, out_dev);
}

int flashe_store_layers_dev(flashe_ctx *ctx, const double *in_dev, uint64_t n, const flashe_tensor_layer *layers, int n_layers, uint64_t block,
                            double *stats_dev)
{
    CHECK_CTX(ctx);
    int rc = check_tensor_layers(ctx, n, layers, n_layers, true);
    if (rc) return rc;
    if (n && (!in_dev || (reinterpret_cast<uintptr_t>(in_dev) & 7u))) return fail(ctx, FLASHE_EINVAL, "null or misaligned in_dev");
    if (stats_dev && (block < 1 || block > 16384)) return fail(ctx, FLASHE_EINVAL, "block must be in [1, 16384], got %llu", static_cast<unsigned long long>(block));
    if (reinterpret_cast<uintptr_t>(stats_dev) & 7u) return fail(ctx, FLASHE_EINVAL, "misaligned stats_dev");
    std::vector<TensorStore> st;
    std::vector<StatLayer> sl;
    uint64_t groups = 0, blocks = 0;
    for (int l = 0; l < n_layers; l++) {
        const flashe_tensor_layer &y = layers[l];
        const uint64_t size = layer_end(layers, n_layers, l, n) - y.start;
        if (!size) continue;
        st.push_back(TensorStore{y.start, groups, size, y.ptr, y.shift, y.dtype, y.flags});
        groups += (size + 7) / 8;
        if (stats_dev) {
            sl.push_back(StatLayer{y.start, blocks, size, y.shift, y.flags, l});
            blocks += (size + block - 1) / block;
        }
    }
    if (st.empty()) return FLASHE_OK;
    if (!sl.empty()) {
        // table, then the per-buffer sums and the layer means behind it
        const size_t tab_bytes = flashe_tables::up16(sl.size() * sizeof(StatLayer));
        if ((rc = ensure(ctx, ctx->stat_ws, tab_bytes + (blocks + sl.size()) * sizeof(double))) || (rc = upload_bytes(ctx, ctx->stat_ws.p, sl.data(), sl.size() * sizeof(StatLayer)))) return rc;
        double *bsum = reinterpret_cast<double *>(static_cast<char *>(ctx->stat_ws.p) + tab_bytes);
        // (the statistics read in_dev before the store pass, which may write in place)
        HIP_TRY(ctx, launch_layer_stats(ctx->env, static_cast<const StatLayer *>(ctx->stat_ws.p), static_cast<int>(sl.size()), blocks, in_dev, block, bsum,
                                        bsum + blocks, stats_dev));
    }
    const TensorStore *tab = nullptr;
    if ((rc = upload_tab(ctx, ctx->tensor_tab, st, &tab))) return rc;
    HIP_TRY(ctx, launch_store_layers(ctx->env, tab, static_cast<int>(st.size()), groups, in_dev));
    return FLASHE_OK;
}

// ---- the aggregator's degree scaling either side of the step (jzf_aggregator.py:676, :902-907) ----
// a multiplier or divisor the reference would not have reached the kernels with
static bool usable_factor(double v) { return std::isfinite(v) && v != 0.0; }

// a non-empty row's pointer: given and aligned to its element size
static bool row_ptr_ok(const void *p, int es) { return p && reinterpret_cast<uintptr_t>(p) % static_cast<uintptr_t>(es) == 0; }

int flashe_stage_layers_dev(flashe_ctx *ctx, const flashe_stage_row *rows, int n_rows)
{
    CHECK_CTX(ctx);
    if (n_rows < 0 || (n_rows && !rows)) return fail(ctx, FLASHE_EINVAL, "stage_layers: bad row table");
    if (ctx->capturing) return fail(ctx, FLASHE_EINVAL, "stage_layers: not inside a graph capture (the row table is staged per call)");
    const int32_t known = FLASHE_STAGE_SCALE | FLASHE_STAGE_SCALE_WIDE | FLASHE_STAGE_SHIFT | FLASHE_STAGE_SHIFT_WIDE | FLASHE_STAGE_OUT_F64;
    std::vector<StageRow> st;
    uint64_t groups = 0;
    for (int r = 0; r < n_rows; r++) {
        const flashe_stage_row &y = rows[r];
        const int es = tensor_elem_bytes(y.src_dtype);
        if (!es) return fail(ctx, FLASHE_EINVAL, "row %d: unknown dtype %d", r, static_cast<int>(y.src_dtype));
        if (y.flags & ~known) return fail(ctx, FLASHE_EINVAL, "row %d: unknown flags 0x%x", r, static_cast<unsigned>(y.flags));
        const bool scale = y.flags & FLASHE_STAGE_SCALE, scale_wide = y.flags & FLASHE_STAGE_SCALE_WIDE, shift = y.flags & FLASHE_STAGE_SHIFT,
                   shift_wide = y.flags & FLASHE_STAGE_SHIFT_WIDE, out64 = y.flags & FLASHE_STAGE_OUT_F64, src64 = y.src_dtype == FLASHE_TENSOR_F64;
        if ((scale_wide && !scale) || (shift_wide && !shift)) return fail(ctx, FLASHE_EINVAL, "row %d: a WIDE flag without its operation", r);
        if ((src64 && (scale_wide || shift_wide)) || (scale_wide && shift_wide))
            return fail(ctx, FLASHE_EINVAL, "row %d: a WIDE flag on a value that is float64 already", r);
        if ((scale_wide || src64) && !out64) return fail(ctx, FLASHE_EINVAL, "row %d: a float64 value needs FLASHE_STAGE_OUT_F64", r);
        if (scale && !usable_factor(y.scale)) return fail(ctx, FLASHE_EINVAL, "row %d: the scale must be finite and not zero", r);
        if (shift && !std::isfinite(y.shift)) return fail(ctx, FLASHE_EINVAL, "row %d: the shift must be finite", r);
        if (y.size == 0) continue;
        if (!row_ptr_ok(y.src, es) || !row_ptr_ok(y.dst, out64 ? 8 : 4)) return fail(ctx, FLASHE_EINVAL, "row %d: null or misaligned src / dst", r);
        st.push_back(StageRow{groups, y.size, y.src, y.dst, y.scale, y.shift, y.src_dtype, y.flags});
        groups += (y.size + 7) / 8;
    }
    if (st.empty()) return FLASHE_OK;
    const StageRow *tab = nullptr;
    if (int rc = upload_tab(ctx, ctx->tensor_tab, st, &tab)) return rc;
    HIP_TRY(ctx, launch_stage_rows(ctx->env, tab, static_cast<int>(st.size()), groups));
    return FLASHE_OK;
}

int flashe_finish_layers_dev(flashe_ctx *ctx, const double *in_dev, uint64_t n, const flashe_finish_row *rows, int n_rows, uint64_t block,
                             double *stats_dev)
{
    CHECK_CTX(ctx);
    if (n_rows < 1 || !rows) return fail(ctx, FLASHE_EINVAL, "the row table needs at least one entry");
    if (rows[0].start != 0) return fail(ctx, FLASHE_EINVAL, "rows[0].start must be 0");
    if (ctx->capturing) return fail(ctx, FLASHE_EINVAL, "finish_layers: not inside a graph capture (the row table is staged per call)");
    if (n && (!in_dev || (reinterpret_cast<uintptr_t>(in_dev) & 7u))) return fail(ctx, FLASHE_EINVAL, "null or misaligned in_dev");
    if (stats_dev && (block < 1 || block > 16384)) return fail(ctx, FLASHE_EINVAL, "block must be in [1, 16384], got %llu", static_cast<unsigned long long>(block));
    if (reinterpret_cast<uintptr_t>(stats_dev) & 7u) return fail(ctx, FLASHE_EINVAL, "misaligned stats_dev");
    const int32_t known = FLASHE_FINISH_DIV_TOTAL | FLASHE_FINISH_SHIFT | FLASHE_FINISH_DIV_OWN | FLASHE_FINISH_ADD_LAST;
    std::vector<FinishRow> st;
    std::vector<FinishStat> sl;
    struct Span { uintptr_t lo, hi; int row; };
    std::vector<Span> dsts, lasts;
    uint64_t groups = 0, blocks = 0;
    for (int r = 0; r < n_rows; r++) {
        const flashe_finish_row &y = rows[r];
        const uint64_t end = layer_end(rows, n_rows, r, n);
        if (y.start > end || end > n) return fail(ctx, FLASHE_EINVAL, "row %d: starts must ascend and stay within n", r);
        const int es = tensor_elem_bytes(y.dst_dtype);
        if (!es) return fail(ctx, FLASHE_EINVAL, "row %d: unknown dtype %d", r, static_cast<int>(y.dst_dtype));
        if (y.flags & ~known) return fail(ctx, FLASHE_EINVAL, "row %d: unknown flags 0x%x", r, static_cast<unsigned>(y.flags));
        if (y.reserved) return fail(ctx, FLASHE_EINVAL, "row %d: reserved field must be 0", r);
        const bool add_last = y.flags & FLASHE_FINISH_ADD_LAST;
        const int ls = add_last ? tensor_elem_bytes(y.last_dtype) : 0;
        if (add_last && !ls) return fail(ctx, FLASHE_EINVAL, "row %d: unknown last_dtype %d", r, static_cast<int>(y.last_dtype));
        if (((y.flags & FLASHE_FINISH_DIV_TOTAL) && !usable_factor(y.div_total)) || ((y.flags & FLASHE_FINISH_DIV_OWN) && !usable_factor(y.div_own)))
            return fail(ctx, FLASHE_EINVAL, "row %d: a divisor must be finite and not zero", r);
        if ((y.flags & FLASHE_FINISH_SHIFT) && !std::isfinite(y.shift)) return fail(ctx, FLASHE_EINVAL, "row %d: the shift must be finite", r);
        const uint64_t size = end - y.start;
        if (!size) continue;
        if (!row_ptr_ok(y.dst, es)) return fail(ctx, FLASHE_EINVAL, "row %d: null or misaligned dst", r);
        if (add_last && !row_ptr_ok(y.last, ls)) return fail(ctx, FLASHE_EINVAL, "row %d: null or misaligned last", r);
        const uintptr_t d = reinterpret_cast<uintptr_t>(y.dst);
        dsts.push_back(Span{d, d + size * es, r});
        if (add_last) {
            const uintptr_t l = reinterpret_cast<uintptr_t>(y.last);
            lasts.push_back(Span{l, l + size * ls, r});
        }
        st.push_back(FinishRow{y.start, groups, size, y.dst, y.last, y.div_total, y.shift, y.div_own, y.dst_dtype, add_last ? y.last_dtype : 0, y.flags, 0});
        groups += (size + 7) / 8;
        if (stats_dev) {
            sl.push_back(FinishStat{y.start, blocks, size, y.div_total, y.shift, y.flags & (FLASHE_FINISH_DIV_TOTAL | FLASHE_FINISH_SHIFT), r});
            blocks += (size + block - 1) / block;
        }
    }
    // a last-round layer may be its own row's dst (same dtype: every value is read by the lane that writes it) and nothing else's
    for (const Span &l : lasts)
        for (const Span &d : dsts) {
            if (l.hi <= d.lo || d.hi <= l.lo) continue;
            const bool in_place = l.row == d.row && l.lo == d.lo && rows[l.row].last_dtype == rows[l.row].dst_dtype;
            if (!in_place) return fail(ctx, FLASHE_EINVAL, "row %d: last overlaps row %d's dst (only last == dst with equal dtypes is in place)", l.row, d.row);
        }
    if (st.empty()) return FLASHE_OK;
    int rc;
    if (!sl.empty()) {
        // table, then the per-buffer sums and the layer means behind it; the statistics read in_dev before the store pass, which may
        // write in place
        const size_t tab_bytes = flashe_tables::up16(sl.size() * sizeof(FinishStat));
        if ((rc = ensure(ctx, ctx->stat_ws, tab_bytes + (blocks + sl.size()) * sizeof(double))) || (rc = upload_bytes(ctx, ctx->stat_ws.p, sl.data(), sl.size() * sizeof(FinishStat)))) return rc;
        double *bsum = reinterpret_cast<double *>(static_cast<char *>(ctx->stat_ws.p) + tab_bytes);
        HIP_TRY(ctx, launch_finish_stats(ctx->env, static_cast<const FinishStat *>(ctx->stat_ws.p), static_cast<int>(sl.size()), blocks, in_dev, block, bsum,
                                         bsum + blocks, stats_dev));
    }
    const FinishRow *tab = nullptr;
    if ((rc = upload_tab(ctx, ctx->tensor_tab, st, &tab))) return rc;
    HIP_TRY(ctx, launch_finish_layers(ctx->env, tab, static_cast<int>(st.size()), groups, in_dev));
    return FLASHE_OK;
}

// ---- the fused client step with the ctx's precomputed masks (jzf_aggregator.py:721-741, :881-899 with next_iter_*_prepared populated,
// jzf_flashe.py:456-488, :537-582): the model-wide codec and the combine of the two calls above in one pass each, no AES ----
static int check_prepared(flashe_ctx *ctx, const flashe_ctx::Prepared &pr, uint64_t n, const char *what)
{
    if (!pr.valid) return fail(ctx, FLASHE_EINVAL, "no prepared %s masks: call flashe_prepare_%s first (they are consumed by one %s)", what, what, what);
    // (a length mismatch leaves the cache in place, as NumPy's broadcast error does in the reference, jzf_flashe.py:480)
    if (n != pr.n) return fail(ctx, FLASHE_EINVAL, "the prepared masks cover %llu elements, the vector has %llu", static_cast<unsigned long long>(pr.n),
                               static_cast<unsigned long long>(n));
    return FLASHE_OK;
}

// element `first` of a cached mask (null: a single-mask cache has no minus stream)
static const uint64_t *prepared_at(const flashe_ctx *ctx, const flashe_ctx::Buf &b, bool held, uint64_t first)
{
    return held ? static_cast<const uint64_t *>(b.p) + first * static_cast<uint64_t>(ctx->limbs) : nullptr;
}

// the prepared front end behind its argument checks (the codec-layer and the tensor form)
static int quantize_encrypt_prepared_model(flashe_ctx *ctx, uint64_t n, uint64_t first, uint64_t count, const flashe_codec_layer *layers, int n_layers,
                                           int element_bits, const double *u_dev, uint64_t *ct_dev)
{
    flashe_ctx::Prepared &pr = ctx->prep_enc;
    Codec cq{};
    if (int rc = stage_codec_layers(ctx, n, layers, n_layers, true, element_bits, 1, first, count, u_dev, nullptr, &cq)) return rc;
    if (count)
        HIP_TRY(ctx, launch_quantize_combine_model(ctx->env, count, cq, prepared_at(ctx, pr.add, true, first), prepared_at(ctx, pr.minus, pr.has_minus, first),
                                                   ct_dev));
    if (first + count == n) pr.valid = false;                           // the call that completes the vector consumes the cache (:483-486)
    return FLASHE_OK;
}

int flashe_quantize_encrypt_prepared_model_dev(flashe_ctx *ctx, uint64_t n, uint64_t first, uint64_t count, const flashe_codec_layer *layers,
                                               int n_layers, int element_bits, const double *u_dev, uint64_t *ct_dev)
{
    CHECK_CTX(ctx);
    int rc = check_prepared(ctx, ctx->prep_enc, n, "encrypt");
    if (rc || (rc = check_model_front(ctx, n, 1, first, count, element_bits, u_dev, ct_dev))) return rc;
    return quantize_encrypt_prepared_model(ctx, n, first, count, layers, n_layers, element_bits, u_dev, ct_dev);
}

int flashe_quantize_encrypt_prepared_tensors_dev(flashe_ctx *ctx, uint64_t n, uint64_t first, uint64_t count, const flashe_tensor_layer *layers,
                                                 int n_layers, int element_bits, const double *u_dev, uint64_t *ct_dev)
{
    CHECK_CTX(ctx);
    // every check that does not need the staged table, before the stage pass launches
    int rc = check_prepared(ctx, ctx->prep_enc, n, "encrypt");
    if (rc || (rc = check_model_front(ctx, n, 1, first, count, element_bits, u_dev, ct_dev)) || (rc = check_tensor_layers(ctx, n, layers, n_layers, true)))
        return rc;
    std::vector<flashe_codec_layer> cl;
    if ((rc = tensor_codec_layers(ctx, n, layers, n_layers, first, count, cl))) return rc;
    return quantize_encrypt_prepared_model(ctx, n, first, count, cl.data(), n_layers, element_bits, u_dev, ct_dev);
}

int flashe_quantize_batch_encrypt_prepared_model_dev(flashe_ctx *ctx, const flashe_batch_layer *layers, int n_layers, int element_bits, int field_bits,
                                                     const double *u_dev, uint64_t n_elems, uint64_t *ct_dev)
{
    CHECK_CTX(ctx);
    flashe_ctx::Prepared &pr = ctx->prep_enc;
    BatchTab bt;
    int rc = check_prepared(ctx, pr, n_elems, "encrypt");
    if (rc || (rc = stage_batch_layers(ctx, layers, n_layers, true, element_bits, field_bits, 1, n_elems, &bt))) return rc;
    if (n_elems && (!u_dev || !ct_dev)) return fail(ctx, FLASHE_EINVAL, "null vector");
    if ((rc = check_vec_aligned(ctx, {ct_dev})) || (rc = check_aligned(ctx, {u_dev}, 8))) return rc;
    if (n_elems)
        HIP_TRY(ctx, launch_quantize_batch_combine_model(ctx->env, bt.tab, bt.n_tab, field_bits, u_dev, n_elems, prepared_at(ctx, pr.add, true, 0),
                                                         prepared_at(ctx, pr.minus, pr.has_minus, 0), ct_dev));
    pr.valid = false;
    return FLASHE_OK;
}

int flashe_quantize_batch_encrypt_prepared_tensors_dev(flashe_ctx *ctx, const flashe_tensor_layer *layers, int n_layers, uint64_t n_values,
                                                       int element_bits, int field_bits, const double *u_dev, uint64_t n_elems, uint64_t *ct_dev)
{
    CHECK_CTX(ctx);
    int rc = check_prepared(ctx, ctx->prep_enc, n_elems, "encrypt");
    std::vector<flashe_batch_layer> bl;
    if (rc || (rc = check_tensor_layers(ctx, n_values, layers, n_layers, true)) ||
        (rc = tensor_batch_layers(ctx, layers, n_layers, n_values, element_bits, field_bits, u_dev, n_elems, ct_dev, bl)))
        return rc;
    return flashe_quantize_batch_encrypt_prepared_model_dev(ctx, bl.data(), n_layers, element_bits, field_bits, u_dev, n_elems, ct_dev);
}

// The way back.  The prefixes the precompute does not cover (dropouts) go first, into ctx scratch: the sum mod 2^b is the same in either
// order, and the codec pass then reads every cached mask once.  *src = what that pass reads (in_dev when nobody dropped out).
static int prepared_extras(flashe_ctx *ctx, uint32_t iter, const uint32_t *add_idx, int n_add, const uint32_t *minus_idx, int n_minus, uint64_t n,
                           uint32_t n_jobs, const uint64_t *in_dev, const uint64_t **src)
{
    *src = in_dev;
    if (n == 0 || (n_add == 0 && n_minus == 0)) return FLASHE_OK;
    if (int rc = ensure(ctx, ctx->stream_tmp, vec_bytes(ctx, n))) return rc;
    uint64_t *tmp = static_cast<uint64_t *>(ctx->stream_tmp.p);
    HIP_TRY(ctx, prf_lists(ctx, iter, add_idx, n_add, minus_idx, n_minus, n, n_jobs, 0, n, in_dev, ctx->limbs, tmp));
    *src = tmp;
    return FLASHE_OK;
}

int flashe_decrypt_prepared_unquantize_model_dev(flashe_ctx *ctx, uint32_t iter, const uint32_t *add_idx, int n_add, const uint32_t *minus_idx,
                                                 int n_minus, uint64_t n, uint32_t n_jobs, const uint64_t *in_dev, const flashe_codec_layer *layers,
                                                 int n_layers, int element_bits, int num_clients, double *out_dev)
{
    CHECK_CTX(ctx);
    flashe_ctx::Prepared &pr = ctx->prep_dec;
    int rc = check_prepared(ctx, pr, n, "decrypt");
    if (rc) return rc;
    if (n && (!in_dev || !out_dev)) return fail(ctx, FLASHE_EINVAL, "null vector");
    if (num_clients < 1) return fail(ctx, FLASHE_EINVAL, "num_clients must be >= 1");
    if ((rc = check_codec_bits(ctx, element_bits)) || (rc = check_prf_args(ctx, n_add, n_minus, n_jobs, in_dev, in_dev, ctx->limbs))) return rc;
    if ((rc = check_f64_aligned(ctx, out_dev, "out_dev"))) return rc;
    if ((n_add && !add_idx) || (n_minus && !minus_idx)) return fail(ctx, FLASHE_EINVAL, "null prefix list");
    Codec cq{};
    if ((rc = stage_codec_layers(ctx, n, layers, n_layers, false, element_bits, num_clients, 0, n, nullptr, out_dev, &cq))) return rc;
    if (n) {
        const uint64_t *src = nullptr;
        if ((rc = prepared_extras(ctx, iter, add_idx, n_add, minus_idx, n_minus, n, n_jobs, in_dev, &src))) return rc;
        HIP_TRY(ctx, launch_combine_unquantize_model(ctx->env, n, src, prepared_at(ctx, pr.add, true, 0), prepared_at(ctx, pr.minus, pr.has_minus, 0), cq,
                                                     out_dev));
    }
    pr.valid = false;                                                    // consumed (:573-580)
    return FLASHE_OK;
}

int flashe_decrypt_prepared_unbatch_unquantize_model_dev(flashe_ctx *ctx, uint32_t iter, const uint32_t *add_idx, int n_add, const uint32_t *minus_idx,
                                                         int n_minus, uint32_t n_jobs, const flashe_batch_layer *layers, int n_layers, int element_bits,
                                                         int field_bits, int num_clients, const uint64_t *in_dev, uint64_t n_elems, double *out_dev)
{
    CHECK_CTX(ctx);
    flashe_ctx::Prepared &pr = ctx->prep_dec;
    int rc = check_prepared(ctx, pr, n_elems, "decrypt");
    if (rc) return rc;
    if (num_clients < 1) return fail(ctx, FLASHE_EINVAL, "num_clients must be >= 1");
    if ((rc = check_prf_args(ctx, n_add, n_minus, n_jobs, in_dev, in_dev, ctx->limbs))) return rc;
    if ((n_add && !add_idx) || (n_minus && !minus_idx)) return fail(ctx, FLASHE_EINVAL, "null prefix list");
    BatchTab bt;
    if ((rc = stage_batch_layers(ctx, layers, n_layers, false, element_bits, field_bits, num_clients, n_elems, &bt))) return rc;
    if (bt.n_values && (!in_dev || !out_dev)) return fail(ctx, FLASHE_EINVAL, "null vector");
    if ((rc = check_f64_aligned(ctx, out_dev, "out_dev"))) return rc;
    if (bt.n_values) {
        const uint64_t *src = nullptr;
        if ((rc = prepared_extras(ctx, iter, add_idx, n_add, minus_idx, n_minus, n_elems, n_jobs, in_dev, &src))) return rc;
        HIP_TRY(ctx, launch_combine_unbatch_unquantize_model(ctx->env, bt.tab, bt.n_tab, field_bits, src, prepared_at(ctx, pr.add, true, 0),
                                                             prepared_at(ctx, pr.minus, pr.has_minus, 0), bt.n_values, out_dev));
    }
    pr.valid = false;
    return FLASHE_OK;
}

// Every layer of a model where its owner keeps it (include/flashe.h): the tables are built on the host in the caller's layer order, sorted
// by compute class for the launches, uploaded once.
int flashe_sparsify_tensors_dev(flashe_ctx *ctx, uint64_t n, const flashe_tensor_layer *layers, int n_layers, const uint64_t *k, void *residual_dev,
                                uint32_t *loc_dev, void *vals_dev, uint64_t *packed_dev, int bits)
{
    CHECK_CTX(ctx);
    if (n >= (1ull << 32)) return fail(ctx, FLASHE_EINVAL, "sparsify_tensors: n must be < 2^32");
    if (!k) return fail(ctx, FLASHE_EINVAL, "sparsify_tensors: null k");
    int rc = check_tensor_layers(ctx, n, layers, n_layers, true);
    if (rc) return rc;
    if (packed_dev && (bits < 1 || bits > 32 || (bits < 32 && n > (1ull << bits))))
        return fail(ctx, FLASHE_EINVAL, "sparsify_tensors: bits (%d) must be in [1, 32] and cover n (%llu)", bits, static_cast<unsigned long long>(n));
    std::vector<const void *> x(n_layers);
    std::vector<int> dt(n_layers);
    std::vector<uint64_t> nl(n_layers), start(n_layers);
    for (int l = 0; l < n_layers; l++) {
        const flashe_tensor_layer &y = layers[l];
        nl[l] = layer_end(layers, n_layers, l, n) - y.start;
        if (k[l] > nl[l]) return fail(ctx, FLASHE_EINVAL, "sparsify_tensors: layer %d: k (%llu) > n (%llu)", l, static_cast<unsigned long long>(k[l]),
                                      static_cast<unsigned long long>(nl[l]));
        x[l] = y.ptr; dt[l] = y.dtype; start[l] = y.start;
    }
    const flashe_tables::SparsifyBlock blk = flashe_tables::sparsify_block_layout(n_layers, nl.data(), k, [&](int l) { return layers[l].dtype == FLASHE_TENSOR_F64; });
    if (n == 0 || (blk.total_k == 0 && !residual_dev)) return FLASHE_OK;          // (total_k == 0 with a residual: every layer only updates it)
    if (blk.total_k && (!loc_dev || !vals_dev)) return fail(ctx, FLASHE_EINVAL, "null vector");
    std::vector<unsigned char> desc(sparsify_tensors_desc_bytes(n_layers));
    int l32 = 0;
    uint64_t nb32 = 0;
    const uint64_t blocks = sparsify_tensors_layout(n_layers, x.data(), dt.data(), nl.data(), k, blk.koff.data(), start.data(), blk.roff.data(), blk.voff.data(),
                                                    desc.data(), &l32, &nb32);
    if (blocks >= (1ull << 32)) return fail(ctx, FLASHE_EINVAL, "sparsify_tensors: too many elements");
    if (ctx->capturing) return fail(ctx, FLASHE_EINVAL, "sparsify_tensors: not inside a graph capture (the layer table is uploaded synchronously)");
    if ((rc = ensure(ctx, ctx->sp_ws, sparsify_tensors_workspace_bytes(n_layers, blocks))) || (rc = upload_bytes(ctx, ctx->sp_ws.p, desc.data(), desc.size()))) return rc;
    HIP_TRY(ctx, launch_sparsify_tensors(ctx->env, n_layers, l32, blocks, nb32, residual_dev, loc_dev, vals_dev, blk.total_k, bits, packed_dev, ctx->sp_ws.p));
    return FLASHE_OK;
}

// ---- a cohort of sparse-job clients on one device (include/flashe.h) ----
// flashe_sparsify_tensors_dev for C models of one shape: the shared table gives starts and compute classes, the C x L sources their
// pointers and storage dtypes; client c's residuals / values / locations / packed locations are block c of equal-stride buffers, laid
// out inside the block exactly as flashe_sparsify_tensors_dev lays out one model.  One set of launches whatever C is.
int flashe_sparsify_cohort_tensors_dev(flashe_ctx *ctx, int n_clients, uint64_t n, const flashe_tensor_layer *layers, int n_layers, const uint64_t *k,
                                       const void *const *src_dev, const int32_t *src_dtype, void *residual_dev, uint64_t residual_stride,
                                       uint32_t *loc_dev, uint64_t loc_stride, void *vals_dev, uint64_t vals_stride, uint64_t *packed_dev,
                                       uint64_t packed_stride, int bits)
{
    CHECK_CTX(ctx);
    if (n_clients < 1 || n_clients > 65535) return fail(ctx, FLASHE_EINVAL, "sparsify_cohort: n_clients must be in [1, 65535]");
    if (n >= (1ull << 32)) return fail(ctx, FLASHE_EINVAL, "sparsify_cohort: n must be < 2^32");
    if (!k || !src_dev || !src_dtype) return fail(ctx, FLASHE_EINVAL, "sparsify_cohort: null argument");
    int rc = check_tensor_layers(ctx, n, layers, n_layers, false);
    if (rc) return rc;
    if (packed_dev && (bits < 1 || bits > 32 || (bits < 32 && n > (1ull << bits))))
        return fail(ctx, FLASHE_EINVAL, "sparsify_cohort: bits (%d) must be in [1, 32] and cover n (%llu)", bits, static_cast<unsigned long long>(n));
    if (static_cast<uint64_t>(n_clients) * static_cast<uint64_t>(n_layers) > (1u << 24)) return fail(ctx, FLASHE_EINVAL, "sparsify_cohort: too many table rows");
    const size_t rows = static_cast<size_t>(n_clients) * n_layers;
    // one client's block: flashe_sparsify_tensors_dev's layout
    std::vector<uint64_t> nl(n_layers);
    for (int l = 0; l < n_layers; l++) {
        const flashe_tensor_layer &y = layers[l];
        if (int rc = check_compute_row(ctx, l, y.dtype)) return rc;
        nl[l] = layer_end(layers, n_layers, l, n) - y.start;
        if (k[l] > nl[l]) return fail(ctx, FLASHE_EINVAL, "sparsify_cohort: layer %d: k (%llu) > n (%llu)", l, static_cast<unsigned long long>(k[l]),
                                      static_cast<unsigned long long>(nl[l]));
    }
    const flashe_tables::SparsifyBlock blk = flashe_tables::sparsify_block_layout(n_layers, nl.data(), k, [&](int l) { return layers[l].dtype == FLASHE_TENSOR_F64; });
    if (n == 0 || (blk.total_k == 0 && !residual_dev)) return FLASHE_OK;          // (total_k == 0 with residuals: every layer only updates its own)
    if (blk.total_k && (!loc_dev || !vals_dev)) return fail(ctx, FLASHE_EINVAL, "null vector");
    if (loc_stride < blk.total_k || vals_stride < blk.v_bytes || (vals_stride & 7u) || (residual_dev && (residual_stride < blk.r_bytes || (residual_stride & 7u))))
        return fail(ctx, FLASHE_EINVAL, "sparsify_cohort: a stride is shorter than one client's block or not a multiple of 8 bytes");
    if (static_cast<uint64_t>(n_clients) * loc_stride >= (1ull << 32)) return fail(ctx, FLASHE_EINVAL, "sparsify_cohort: too many locations");
    const uint64_t n_limbs = (blk.total_k * static_cast<uint64_t>(bits > 0 ? bits : 1) + 63) / 64;
    if (packed_dev && packed_stride < n_limbs) return fail(ctx, FLASHE_EINVAL, "sparsify_cohort: packed_stride is shorter than one client's packed locations");
    std::vector<const void *> x(rows);
    std::vector<int> dt(rows);
    std::vector<uint64_t> nn(rows), kk(rows), koff(rows), start(rows), roff(rows), voff(rows);
    for (int c = 0; c < n_clients; c++)
        for (int l = 0; l < n_layers; l++) {
            const size_t at = static_cast<size_t>(c) * n_layers + l;
            if (int rc = check_cohort_source(ctx, c, l, src_dtype[at], src_dev[at], layers[l].dtype == FLASHE_TENSOR_F64, nl[l] != 0, true)) return rc;
            x[at] = src_dev[at]; dt[at] = src_dtype[at]; nn[at] = nl[l]; kk[at] = k[l]; start[at] = layers[l].start;
            koff[at] = static_cast<uint64_t>(c) * loc_stride + blk.koff[l];
            roff[at] = static_cast<uint64_t>(c) * residual_stride + blk.roff[l];
            voff[at] = static_cast<uint64_t>(c) * vals_stride + blk.voff[l];
        }
    std::vector<unsigned char> desc(sparsify_tensors_desc_bytes(static_cast<int>(rows)));
    int r32 = 0;
    uint64_t nb32 = 0;
    const uint64_t blocks = sparsify_tensors_layout(static_cast<int>(rows), x.data(), dt.data(), nn.data(), kk.data(), koff.data(), start.data(), roff.data(),
                                                    voff.data(), desc.data(), &r32, &nb32);
    if (blocks >= (1ull << 32)) return fail(ctx, FLASHE_EINVAL, "sparsify_cohort: too many elements");
    if ((rc = ensure(ctx, ctx->sp_ws, sparsify_tensors_workspace_bytes(static_cast<int>(rows), blocks))) || (rc = upload_bytes(ctx, ctx->sp_ws.p, desc.data(), desc.size()))) return rc;
    HIP_TRY(ctx, launch_sparsify_cohort(ctx->env, n_clients, static_cast<int>(rows), r32, blocks, nb32, residual_dev, loc_dev, loc_stride, vals_dev, blk.total_k, bits,
                                        packed_dev, packed_stride, ctx->sp_ws.p));
    return FLASHE_OK;
}

// The sparse job's codec front end for all clients of a cohort in one launch: shared compact layer table (start, alpha, shift, flags;
// dtype = the compute class), C x L sources, client-major draws -> C one-limb plaintext vectors + the C quantised 'zzz' values.
// (the argument checks of the two entry points that take a sparse cohort's compact layers: the one below and
// flashe_quantize_encrypt_sparse_cohort_dev; outs = the HOST array of output vectors; row_of = the non-empty layers)
static int quantize_cohort_check(flashe_ctx *ctx, int n_clients, uint64_t n, const flashe_tensor_layer *layers, int n_layers, const void *const *src_dev,
                                 const int32_t *src_dtype, int element_bits, const double *u_dev, uint64_t u_stride, const double *zzz,
                                 const void *outs, const uint64_t *zeros_dev, std::vector<int> &row_of)
{
    if (n_clients < 1 || n_clients > 65535) return fail(ctx, FLASHE_EINVAL, "quantize_cohort: n_clients must be in [1, 65535]");
    if (!src_dev || !src_dtype || !u_dev || !zzz || !outs || !zeros_dev) return fail(ctx, FLASHE_EINVAL, "quantize_cohort: null argument");
    int rc = check_element_bits(ctx, element_bits);
    if (rc || (rc = check_aligned(ctx, {u_dev, zeros_dev}, 8))) return rc;
    if (u_stride < n + 1) return fail(ctx, FLASHE_EINVAL, "quantize_cohort: u_stride must cover a client's n + 1 draws");
    if ((rc = check_tensor_layers(ctx, n, layers, n_layers, false)) || (rc = cohort_rows(ctx, n, layers, n_layers, row_of))) return rc;
    for (int c = 0; c < n_clients; c++)
        for (const int l : row_of) {
            const size_t at = static_cast<size_t>(c) * n_layers + l;
            if ((rc = check_cohort_source(ctx, c, l, src_dtype[at], src_dev[at], layers[l].dtype == FLASHE_TENSOR_F64, true, true))) return rc;
        }
    return FLASHE_OK;
}

int flashe_quantize_cohort_dev(flashe_ctx *ctx, int n_clients, uint64_t n, const flashe_tensor_layer *layers, int n_layers, const void *const *src_dev,
                               const int32_t *src_dtype, int element_bits, const double *u_dev, uint64_t u_stride, const double *zzz, int zzz_is_f64,
                               uint64_t *const *pt_dev, uint64_t *const *tail_dev, uint64_t *zeros_dev)
{
    CHECK_CTX(ctx);
    if (n >= (1ull << 32)) return fail(ctx, FLASHE_EINVAL, "quantize_cohort: n must be < 2^32");
    std::vector<int> row_of;
    int rc = quantize_cohort_check(ctx, n_clients, n, layers, n_layers, src_dev, src_dtype, element_bits, u_dev, u_stride, zzz, pt_dev, zeros_dev, row_of);
    if (rc) return rc;
    std::vector<QuantCohortRow> tab;
    for (const int l : row_of) {
        const flashe_tensor_layer &y = layers[l];
        const Codec c = codec_quantize_front(nullptr, y.dtype == FLASHE_TENSOR_F64 || (y.flags & FLASHE_TENSOR_LOOP_F64), y.alpha, element_bits, nullptr);
        tab.push_back(QuantCohortRow{y.start, c.alpha, c.scale, c.den, y.shift, c.x_is_f64, y.flags & (FLASHE_TENSOR_SHIFT | FLASHE_TENSOR_SHIFT_WIDE)});
    }
    const size_t n_tab = tab.size(), C = static_cast<size_t>(n_clients);
    std::vector<const void *> src(C * n_tab);
    std::vector<int32_t> sdt(C * n_tab);
    for (size_t c = 0; c < C; c++) {
        if (n && (!pt_dev[c] || (reinterpret_cast<uintptr_t>(pt_dev[c]) & 7u))) return fail(ctx, FLASHE_EINVAL, "client %d: null or misaligned plaintext vector", static_cast<int>(c));
        if (tail_dev && tail_dev[c] && (reinterpret_cast<uintptr_t>(tail_dev[c]) & 7u)) return fail(ctx, FLASHE_EINVAL, "client %d: misaligned tail", static_cast<int>(c));
        for (size_t rr = 0; rr < n_tab; rr++) {
            const size_t at = c * n_layers + row_of[rr];
            src[c * n_tab + rr] = src_dev[at];
            sdt[c * n_tab + rr] = src_dtype[at];
        }
    }
    // one block in ctx->codec_tab: rows | sources | plaintext pointers | tails | zzz values | source dtypes
    flashe_tables::Blob blob;
    blob.add(tab.data(), n_tab * sizeof(QuantCohortRow));
    const size_t o_src = blob.add(src.data(), src.size() * sizeof(void *)), o_pt = blob.add(pt_dev, C * sizeof(void *)),
                 o_tail = blob.add(tail_dev, C * sizeof(void *)), o_zzz = blob.add(zzz, C * sizeof(double)),
                 o_dt = blob.add(sdt.data(), sdt.size() * sizeof(int32_t));
    const char *blob_dev = nullptr;
    if ((rc = upload_tab(ctx, ctx->codec_tab, blob.bytes, &blob_dev))) return rc;
    QuantCohort qc{};
    qc.rows = reinterpret_cast<const QuantCohortRow *>(blob_dev);
    qc.src = reinterpret_cast<const void *const *>(blob_dev + o_src);
    qc.pt = reinterpret_cast<uint64_t *const *>(blob_dev + o_pt);
    qc.tail = reinterpret_cast<uint64_t *const *>(blob_dev + o_tail);
    qc.zzz = reinterpret_cast<const double *>(blob_dev + o_zzz);
    qc.src_dtype = reinterpret_cast<const int32_t *>(blob_dev + o_dt);
    qc.zeros = zeros_dev;
    qc.n_rows = static_cast<int>(n_tab); qc.n_clients = n_clients; qc.tail_limbs = ctx->limbs;
    const Codec z = codec_quantize_front(nullptr, zzz_is_f64 != 0, 1.0, element_bits, nullptr);
    qc.zrow = QuantCohortRow{n, z.alpha, z.scale, z.den, 0.0, z.x_is_f64, 0};
    HIP_TRY(ctx, launch_quantize_cohort(ctx->env, qc, n, u_dev, u_stride));
    return FLASHE_OK;
}

// The two steps of a sparse cohort's uploads -- flashe_quantize_cohort_dev, then one flashe_encrypt_dev(SINGLE) per client
// (jzf_quantize.py:433-465, jzf_aggregator.py:717-743, jzf_flashe.py:471-478) -- as ONE chained launch from the floats at int_bits
// 16 / 20 / 23 / 24 / 32 (prf_small_sparse_cohort_kernel): no plaintext vector exists in HBM.  The checks are quantize_cohort_check's, the
// table and the stage pass cohort_stage's; what the launch does not take is refused with FLASHE_ENOTSUP before anything is staged.
int flashe_quantize_encrypt_sparse_cohort_dev(flashe_ctx *ctx, uint32_t iter, int n_clients, const uint32_t *idx, uint64_t n, uint32_t n_jobs,
                                              const flashe_tensor_layer *layers, int n_layers, const void *const *src_dev, const int32_t *src_dtype,
                                              int element_bits, const double *u_dev, uint64_t u_stride, const double *zzz, int zzz_is_f64,
                                              uint64_t *const *ct_dev, uint64_t *zeros_dev)
{
    CHECK_CTX(ctx);
    static const char who[] = "flashe_quantize_encrypt_sparse_cohort_dev";
    std::vector<int> row_of;
    int rc = quantize_cohort_check(ctx, n_clients, n, layers, n_layers, src_dev, src_dtype, element_bits, u_dev, u_stride, zzz, ct_dev, zeros_dev, row_of);
    if (rc) return rc;
    if (!idx) return fail(ctx, FLASHE_EINVAL, "%s: null argument", who);
    if (n_jobs == 0) return fail(ctx, FLASHE_EINVAL, "n_jobs must be >= 1");
    for (int c = 0; c < n_clients; c++) {
        if (!ct_dev[c] || (reinterpret_cast<uintptr_t>(ct_dev[c]) & 7u)) return fail(ctx, FLASHE_EINVAL, "client %d: null or misaligned upload", c);
        if (reinterpret_cast<uint64_t *>(ct_dev[c]) == zeros_dev) return fail(ctx, FLASHE_EINVAL, "client %d: the upload aliases zeros_dev", c);
    }
    if (!small_cohort_admits(ctx->env, n_clients, n, n_jobs, false)) return cohort_declined(ctx, who, "sparse cohort");
    const Codec z = codec_quantize_front(nullptr, zzz_is_f64 != 0, 1.0, element_bits, nullptr);
    CohortCodec cc{};
    const char *zzz_dev = nullptr;
    if ((rc = cohort_stage(ctx, n_clients, n, layers, n_layers, src_dev, src_dtype, element_bits, cc, zzz, static_cast<size_t>(n_clients) * sizeof(double),
                           &zzz_dev, &row_of)))
        return rc;
    return cohort_launched(ctx, launch_small_sparse_cohort(ctx->env, iter, n_clients, idx, cc, u_dev, u_stride, ct_dev, n, n_jobs,
                                                           reinterpret_cast<const double *>(zzz_dev), z.x_is_f64 != 0, z.alpha, z.scale, z.den, zeros_dev),
                           who, "sparse cohort");
}

}  // extern "C"
