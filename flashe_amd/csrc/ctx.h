// Private to the host side of libflashe_hip.so (abi.hip, abi_layers.hip, host_twins.hip, comm.hip, mt19937.hip and, through draw_launch.h, philox.hip
// and pcg64.hip): the context object behind the opaque flashe_ctx of include/flashe.h, and the error-reporting and argument helpers the entry points share.
#pragma once
#include "flashe.h"
#include "kernels.h"
#include "blockpool.h"

#include <algorithm>
#include <initializer_list>
#include <string>
#include <vector>

struct flashe_ctx {
    int device = 0;
    int device_cus = 0;       // compute units of the device (env.num_cus is what launches may use: flashe_ctx_set_cu_limit)
    int int_bits = 0;
    int limbs = 0;
    bool own_stream = false;
    flashe::LaunchEnv env{};
    uint32_t *te0_dev = nullptr;
    uint32_t *rkw_dev = nullptr;
    uint32_t *rkp_dev = nullptr;
    std::string err;
    // scratch buffers owned by the ctx (grown on demand, reused across calls)
    struct Buf { void *p = nullptr; size_t cap = 0; };
    Buf summaries;    // packed-aggregate block summaries
    Buf stream_tmp;   // whole-vector mask stream for the sparse paths
    Buf acc_tmp[2];   // ping-pong partial sums when a packed reduce has more than kMaxOps operands
    Buf sp_ws;        // sparsifier workspace (select state, histogram, per-block counts)
    Buf bounds;       // span reduce: first entry of every client in every span
    Buf mt_ws;        // flashe_mt19937_random_dev: state in / out and the substream windows
    Buf draw_tab;     // flashe_philox_random_dev, flashe_pcg64_random_dev: the plan table of a launch of more segments than its kernel arguments hold (one for both: draw_launch.h)
    Buf codec_tab;    // layer table of the fused quantise / unquantise over a flattened model
    Buf tensor_ws;    // caller tensors: the front end's converted layers (flashe_quantize_*_tensors_dev)
    Buf tensor_tab;   // caller tensors: stage / store table
    Buf stat_ws;      // caller tensors: stat table, per-buffer sums and layer means of flashe_store_layers_dev
    hipEvent_t ev_foreign = nullptr;   // flashe_stream_wait_stream's marker on the other stream (created on first use)
    // ctx-resident mask precompute (flashe_prepare_encrypt / flashe_prepare_decrypt): the masks of the reference's next_iter_*_prepared
    // caches (jzf_flashe.py:599-666) stay in HBM inside the ctx and are consumed by the next flashe_encrypt_prepared* /
    // flashe_decrypt_prepared* call; the blocks are kept for the next round's masks
    struct Prepared { Buf add, minus; uint64_t n = 0; bool valid = false, has_minus = false; uint32_t iter = 0, add_idx = 0, minus_idx = 0; };
    Prepared prep_enc, prep_dec;
    // chain decrypt mask: the summed double-mask encrypt launch (flashe_encrypt_batch_sum_dev, the summed flashe_encrypt_batch_range_dev)
    // over clients a .. b also writes D = term(b + 1) - term(a) mod 2^int_bits of its elements [first, first + count), the mask the
    // arbiter's decrypt of the sum adds; a flashe_decrypt_range_dev with exactly that key (iter, key epoch, (add, minus) = ([b + 1], [a]),
    // n, n_jobs) on a range inside the covered one is then one combine pass.  Not consumed (D is deterministic for its key); its own
    // slot, so that an explicit flashe_prepare_decrypt survives.  Per ctx and so per stream: a decrypt on another ctx never sees it.
    struct ChainDmask { Buf d; uint64_t n = 0, first = 0, count = 0; uint32_t iter = 0, key_epoch = 0, add_idx = 0, minus_idx = 0, n_jobs = 0; bool valid = false; };
    ChainDmask chain_dmask;
    bool chain_dmask_on = true;   // FLASHE_CHAIN_DMASK=0 at ctx creation: the summed launches write no decrypt mask
    bool chain_dec_on = true;     // FLASHE_CHAIN_DEC=0 at ctx creation: flashe_encrypt_batch_sum_decrypt_dev always runs as its two calls
    // staging blocks of the host-pointer twins: hipMalloc / hipFree cost more than the kernels on LeNet-sized vectors and more than
    // the PCIe transfer on 160 MB ones, so blocks are kept and reused within a byte budget (the twins are synchronous: a block is
    // free again when its call returns)
    flashe_pool::StagingPool *staging = nullptr;   // (policy in blockpool.h, so that it can be tested on the host under sanitizers)
    bool capturing = false;   // between flashe_graph_begin and flashe_graph_end
    uint32_t key_epoch = 0;   // bumped by flashe_ctx_set_key: a graph replays the key it was captured with
    hipEvent_t ev_copy[2] = {nullptr, nullptr};   // hand-off events of the pipelined host-pointer twins (created on first use)
    uint32_t *err_flag_host = nullptr;   // host-mapped word the sparse kernels set when they skip an out-of-range location
};

namespace flashe_host {

// Records the message on ctx (or, ctx == NULL, as this thread's context-creation error) and returns `code`.
int fail(flashe_ctx *ctx, int code, const char *fmt, ...) __attribute__((format(printf, 3, 4)));

inline size_t vec_bytes(const flashe_ctx *ctx, uint64_t n) { return static_cast<size_t>(n) * ctx->limbs * 8; }

// b holds at least `bytes` (grown on demand; FLASHE_EINVAL while a graph is being captured)
int ensure(flashe_ctx *ctx, flashe_ctx::Buf &b, size_t bytes);
// FLASHE_OK outside a capture; inside one, FLASHE_EINVAL naming `what`: the first check of every entry point that waits for the ctx
// stream or copies to or from host memory on it
int refuse_in_capture(flashe_ctx *ctx, const char *what);
bool aligned16(const void *p);
bool ct_aligned(const flashe_ctx *ctx, const void *p);   // aligned like a ciphertext vector: 16 bytes for 2-limb elements, else 8

// The argument checks the entry points of abi.hip and abi_layers.hip share (abi.hip): FLASHE_OK, or FLASHE_EINVAL with the message set.
int check_scheme(flashe_ctx *ctx, int scheme);
int check_wide_aligned(flashe_ctx *ctx, std::initializer_list<const void *> vecs);
int check_sum_aligned(flashe_ctx *ctx, const void *sum_out_dev);
// ... when the double mask would need prefix idx + 1 = 2^32 for one of the n_idx entries
int check_double_idx(flashe_ctx *ctx, int scheme, const uint32_t *idx, int n_idx);
int check_field_bits(flashe_ctx *ctx, int field_bits);
int check_range(flashe_ctx *ctx, uint64_t n, uint64_t first, uint64_t count);
int check_prf_args(flashe_ctx *ctx, int n_add, int n_minus, uint32_t n_jobs, const void *out, const void *in, int in_limbs);
// out = in + sum term(add[k]) - sum term(minus[k]) over prefix lists of any length (abi.hip)
hipError_t prf_lists(flashe_ctx *ctx, uint32_t iter, const uint32_t *add, int n_add, const uint32_t *minus, int n_minus, uint64_t n, uint32_t n_jobs,
                     uint64_t first, uint64_t count, const uint64_t *in_dev, int in_limbs, uint64_t *out_dev);

// RAII temp device buffer for the host-pointer twins.  Staging blocks are kept by the ctx and reused: a hipMalloc + hipFree
// pair of a 160 MB block costs more than moving 160 MB over PCIe Gen5 on this platform (measured 7 ms against 2.9 ms,
// tests/perf/e2e_calls.py).  The blocks a ctx keeps are bounded by a byte budget (FLASHE_STAGING_POOL_MB, default 8 GiB of the
// 288 GB); beyond it the largest free block makes room, and a request that still does not fit is a plain allocation.
struct Tmp {
    void *p = nullptr;
    flashe_ctx *owner = nullptr;
    int slot = -1;
    Tmp() = default;
    Tmp(const Tmp &) = delete;
    Tmp &operator=(const Tmp &) = delete;
    ~Tmp()
    {
        if (!p) return;
        if (slot >= 0) owner->staging->give_back(slot);
        else (void)hipFree(p);
    }
    hipError_t alloc(flashe_ctx *ctx, size_t bytes);   // (abi.hip: creates the ctx's pool on first use)
    template <class T> T *as() { return static_cast<T *>(p); }
};

}  // namespace flashe_host

#define HIP_TRY(ctx, expr)                                                                           \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess)                                                                        \
            return flashe_host::fail(ctx, e_ == hipErrorOutOfMemory ? FLASHE_ENOMEM : FLASHE_EIO, "%s failed: %s", #expr, \
                                     hipGetErrorString(e_));                                         \
    } while (0)

#define CHECK_CTX(ctx)                                                        \
    do {                                                                      \
        if (!(ctx)) return FLASHE_EINVAL;                                     \
        HIP_TRY(ctx, hipSetDevice((ctx)->device));                            \
    } while (0)

namespace flashe_host {

// Host bytes to the device on the ctx stream.  (Pageable source: the copy has left `src` when the call returns; stream order keeps an
// earlier launch's table intact until it ends.)
inline int upload_bytes(flashe_ctx *ctx, void *dst, const void *src, size_t bytes)
{
    HIP_TRY(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->env.stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->env.stream));
    return FLASHE_OK;
}

// A host table into a ctx buffer (grown to hold it; an empty table uploads nothing).
template <class T> inline int upload_tab(flashe_ctx *ctx, flashe_ctx::Buf &b, const std::vector<T> &tab, const T **tab_dev, int *n_tab = nullptr)
{
    int rc = ensure(ctx, b, std::max<size_t>(tab.size(), 1) * sizeof(T));
    if (rc) return rc;
    if (!tab.empty() && (rc = upload_bytes(ctx, b.p, tab.data(), tab.size() * sizeof(T)))) return rc;
    *tab_dev = static_cast<const T *>(b.p);
    if (n_tab) *n_tab = static_cast<int>(tab.size());
    return FLASHE_OK;
}

}  // namespace flashe_host
