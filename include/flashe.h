/*
 * flashe.h -- C ABI of libflashe_hip.so, the MI355X (gfx950) FLASHE cipher engine.
 *
 * This is the drop-in boundary for ONE path of SamuelGong/FLASHE: the
 * federatedml/secureprotol FLASHE cipher (AES-256 PRF mask generation, per-element
 * modular encrypt / decrypt over big-integer vectors) plus the arbiter's ciphertext
 * mod-add reduce and the bit-packing codec either side of it.  Reference citations are
 * relative to the reference tree (federatedml/...).
 *
 * Conventions
 *   - plain C, no exceptions, no ownership transfer: the caller allocates every buffer.
 *   - every function returns 0 (FLASHE_OK) or a negative errno-style code;
 *     flashe_last_error(ctx) gives the text of the last failure on that ctx.
 *   - a ctx is bound to one HIP device and one HIP stream; it is not thread-safe, separate
 *     ctxs are independent.  *_dev functions take DEVICE pointers and are asynchronous on
 *     the ctx stream (flashe_sync to wait); the un-suffixed twins take HOST pointers and
 *     are synchronous (H2D + kernels + D2H).
 *   - element layout: an element of b = int_bits bits (1 <= b <= 128) is
 *     L = flashe_limbs(b) = ceil(b/64) little-endian uint64 limbs; vectors are [n][L].
 *     Inputs need not be reduced: everything is taken mod 2^b as the reference does
 *     (jzf_flashe.py:480-481).
 *   - there is NO CPU fallback: without a HIP device every ctx call fails with
 *     FLASHE_ENODEV.
 */
#ifndef FLASHE_H
#define FLASHE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FLASHE_OK       0
#define FLASHE_EIO     (-5)    /* a HIP runtime call failed; see flashe_last_error */
#define FLASHE_ENOMEM  (-12)
#define FLASHE_ENODEV  (-19)   /* no usable HIP device */
#define FLASHE_EINVAL  (-22)
#define FLASHE_ENOTSUP (-95)   /* the call's shape is outside what this entry point launches; nothing was launched, use the general calls */

#define FLASHE_SCHEME_SINGLE 0 /* FlasheCipher(int_bits, mask="single") */
#define FLASHE_SCHEME_DOUBLE 1 /* FlasheCipher(int_bits)  (default "double") */

typedef struct flashe_ctx flashe_ctx;

/* ---- library / device ------------------------------------------------------------- */
/* ABI version of this header; flashe_abi_version() returns the one the library was built from.  Bumped whenever an exported
 * signature or struct layout changes or entry points are added.
 *   1  rounds 1-3 (entry points and flashe_prf_job fields were added without a bump: n_in / in_stride / sum_out_dev, the *_u32_dev,
 *      *_sum_dev, sparse_double_masks, mt19937 and sparsify_batch calls -- a round-1 binding of flashe_prf_job is NOT compatible)
 *   2  round 4: flashe_codec_layer + flashe_quantize_encrypt_model_dev / flashe_decrypt_unquantize_model_dev (the fused codec over a
 *      flattened model), flashe_batch_layer + flashe_quantize_batch_model_dev / flashe_unbatch_unquantize_model_dev (batched jobs);
 *      ctx-resident mask precompute (flashe_prepare_* / flashe_*_prepared[_dev] / flashe_prepared_query / _discard); flashe_span_bounds
 *      handles (+ flashe_sparse_*_bounds_dev); flashe_dynamic_masking_cost_dev; flashe_encrypt_batch_range_dev and
 *      flashe_packed_resolve_carry_strided_dev (element-sharded multi-GPU round); flashe_aggregate_elem_u32_dev; flashe_mt19937_plan;
 *      flashe_sparse_encrypt_aggregate_dev (the clients' sparse encrypts and the aggregate of their uploads in one pass);
 *      flashe_unquantize_model_dev (the model-wide codec back end without a decrypt: the sparse job's way back);
 *      flashe_sparse_span, flashe_sparse_encrypt_aggregate_range_dev, flashe_sparse_decrypt_range_dev (the sparse round by position ranges);
 *      timing probes and tuning knobs compiled out of libflashe_hip.so (-DFLASHE_TUNING build only)
 *   3  round 5: flashe_ctx_compact_layout (does this ctx run the *_u32_dev entry points?); the double-mask encrypt entry points
 *      refuse idx = 2^32 - 1 with FLASHE_EINVAL (the reference's OverflowError, jzf_flashe.py:352-353) instead of wrapping to
 *      prefix 0; flashe_prepared_discard releases the cached mask buffers; flashe_combine_batch_sum_dev (online encrypts with
 *      precomputed masks + their sum in one pass); flashe_encrypt_batch_sum_u32_dev (the compact layout's encrypts + their sum)
 *   4  round 6: flashe_device_peer_access and flashe_rccl_version (the preflight a rank of a multi-GPU launch runs before it creates
 *      its ctx); flashe_combine_batch_sum_decrypt_dev (online encrypts + their sum + the decrypt of the sum in one pass);
 *      later additions without a bump (existing signatures unchanged; a caller checks for the symbols): flashe_ctx_stream,
 *      flashe_stream_wait_stream, flashe_event_query, flashe_tensor_layer + flashe_quantize_encrypt_tensors_dev /
 *      flashe_quantize_batch_tensors_dev / flashe_store_layers_dev (caller-owned tensors either side of the model-wide codec);
 *      flashe_quantize_encrypt_prepared_{model,tensors}_dev, flashe_quantize_batch_encrypt_prepared_{model,tensors}_dev,
 *      flashe_decrypt_prepared_unquantize_model_dev, flashe_decrypt_prepared_unbatch_unquantize_model_dev (the model-wide codec with the
 *      ctx's precomputed masks); FLASHE_ENOTSUP + flashe_quantize_encrypt_cohort_dev (a cohort of co-located clients: C float models
 *      to C ciphertexts, their sum and the decrypt mask in one chained launch) and flashe_combine_unquantize_model_dev (the codec back
 *      end over a sum and caller-held masks); flashe_quantize_encrypt_sparse_cohort_dev (a sparse cohort's quantise + encrypts in one
 *      launch at int_bits 16 - 32); flashe_sparsify_cohort_tensors_dev and flashe_quantize_cohort_dev (a cohort of sparse-job
 *      clients: C models sparsified in one set of launches, their compact layers quantised in one launch);
 *      flashe_quantize_encrypt_cohort_u32_dev (the cohort's chained launch in the compact layout, int_bits 16 / 20 / 23 / 24 / 32);
 *      flashe_quantize_batch_encrypt_cohort_dev (the cohort's chained launch for a batched job at int_bits > 64, 5 - 7 values per
 *      element) and flashe_combine_unbatch_unquantize_model_dev (the batched codec back end over a sum and caller-held masks);
 *      flashe_cohort_masks_u32_dev (a cohort's precomputed encrypt masks in the compact layout, one chain of C + 1 streams) and
 *      flashe_quantize_combine_cohort_dev / flashe_quantize_combine_cohort_u32_dev / flashe_quantize_batch_combine_cohort_dev (a
 *      precompute job's cohort online: C float models + C caller-held masks to C ciphertexts and their sum in one pass, no AES);
 *      flashe_quantize_encrypt_cohort_runs_dev / flashe_quantize_batch_encrypt_cohort_runs_dev (the cohort's chained launches for a round
 *      in which clients dropped out: any strictly ascending cipher indices) and flashe_quantize_encrypt_cohort_runs_u32_dev (the same
 *      round in the compact layout, int_bits 16 / 20 / 23 / 24 / 32); flashe_stage_row + flashe_stage_layers_dev and
 *      flashe_finish_row + flashe_finish_layers_dev (the aggregator's degree scaling either side of the fused client step: the multiply
 *      in the stage pass, the two divisions and the last round's model in the store + statistics pass);
 *      flashe_encrypt_batch_sum_decrypt_dev (a co-located round's encrypts, their sum and the decrypt of the sum: one launch at
 *      int_bits 128); flashe_cohort_cut_parts + flashe_quantize_encrypt_cohort_cut_dev / flashe_quantize_encrypt_cohort_cut_u32_dev (a
 *      cohort whose vector does not fill the chip uncut: the summed chain cut into runs of clients and one combine pass);
 *      flashe_aggregate_packed_elems_dev / flashe_aggregate_packed_elems_u32_dev (the arbiter's packed reduce computed on unpacked
 *      ciphertext vectors in one pass); flashe_cohort_cut_pieces + flashe_quantize_encrypt_cohort_cut_runs_dev /
 *      flashe_quantize_encrypt_cohort_cut_runs_u32_dev / flashe_quantize_batch_encrypt_cohort_cut_runs_dev (the cut launch for a round in
 *      which clients dropped out -- every gap is a cut -- and for a batched job); flashe_quantize_combine_cohort_philox_dev /
 *      flashe_quantize_combine_cohort_philox_u32_dev (a precompute job's cohort online with the draws of np.random.Philox streams
 *      generated inside the launch: no draw buffer) and flashe_quantize_batch_combine_cohort_philox_dev (the same for a batched job);
 *      flashe_quantize_combine_cohort_pcg64_dev / flashe_quantize_combine_cohort_pcg64_u32_dev (the un-batched form for the streams of
 *      np.random.PCG64 / PCG64DXSM, np.random.default_rng's generator) with flashe_pcg64_cohort_grid + flashe_pcg64_cohort_lane_draws;
 *      flashe_quantize_encrypt_cohort_u64_dev (the cohort's chained launch in the one-limb layout, int_bits 33 .. 64);
 *      flashe_quantize_encrypt_cohort_runs_u64_dev (the same launch for a round in which clients dropped out) */
#define FLASHE_ABI_VERSION 4
int flashe_abi_version(void);
int flashe_device_count(int *count);
/* Preflight of a multi-GPU launch (new): can `device` read and write `peer`'s memory directly (hipDeviceCanAccessPeer: what RCCL's
 * point-to-point transport over xGMI needs)?  *can_access = 1 / 0; device == peer gives 1.  Creates no ctx and no stream. */
int flashe_device_peer_access(int device, int peer, int *can_access);
int flashe_limbs(int int_bits);                 /* 1 or 2; 0 if int_bits is out of range */

/* ---- context ---------------------------------------------------------------------- */
/* Replaces FlasheCipher.__init__ + generate_prp_seed (jzf_flashe.py:230-260, :280-295):
 * key is the 32-byte AES-256 key, i.e. the low 256 bits of the PRP seed, big-endian
 * (jzf_aes.py:21-28).  stream: a hipStream_t to run on (e.g. the caller framework's
 * current stream) or NULL to let the ctx create its own non-blocking stream. */
int flashe_ctx_create(flashe_ctx **out, const uint8_t key[32], int int_bits, int device, void *stream);
int flashe_ctx_destroy(flashe_ctx *ctx);
int flashe_ctx_set_key(flashe_ctx *ctx, const uint8_t key[32]);
int flashe_ctx_int_bits(const flashe_ctx *ctx);
/* new: 1 if the compact uint32 entry points (flashe_encrypt_batch_u32_dev, flashe_aggregate_decrypt_u32_dev, ...) run on this ctx --
 * int_bits <= 32, the table PRF backend and the chained kernels (FLASHE_CHAIN != 0) -- 0 if they would answer FLASHE_EINVAL. */
int flashe_ctx_compact_layout(const flashe_ctx *ctx);
/* new: how many compute units the persistent launches of this ctx occupy (0 = the whole device; flashe_ctx_cu_count = what the
 * device has).  The PRF workgroups hold 128 KiB of LDS per CU, so a kernel from ANOTHER stream that needs more than the rest (RCCL's
 * transfer kernels do) runs beside a PRF launch only on CUs that launch leaves free: the multi-GPU schedules that hide the exchange
 * under the next chunk's encrypts set this to cu_count - 16 or so.  Results do not depend on it. */
int flashe_ctx_set_cu_limit(flashe_ctx *ctx, int cus);
int flashe_ctx_cu_count(const flashe_ctx *ctx);
/* Which implementation of the AES-256 PRF the fused kernels use (results are identical):
 * 0 = automatic, 1 = LDS T-table kernel, 2 = bit-sliced VALU kernel (b > 64, single add prefix with
 * at most one minus prefix; other shapes always use the table kernel).  Also settable at ctx creation
 * through the environment variable FLASHE_PRF_BACKEND=table|bitslice.  The bit-sliced kernels are measured
 * alternatives (2.5x the VALU work of the table kernel) and are NOT in libflashe_hip.so: they are built by
 * `make -C flashe_amd/csrc bitslice` into libflashe_hip_bitslice.so; the product library answers FLASHE_EINVAL. */
#define FLASHE_PRF_AUTO     0
#define FLASHE_PRF_TABLE    1
#define FLASHE_PRF_BITSLICE 2
int flashe_ctx_set_prf_backend(flashe_ctx *ctx, int backend);
/* Text of the last error on ctx (ctx == NULL: last flashe_ctx_create failure of this thread). */
const char *flashe_last_error(const flashe_ctx *ctx);
/* Known-answer self test on the device: FIPS-197 C.3 through the PRF kernel. */
int flashe_selftest(flashe_ctx *ctx);

/* ---- host-side logic of the path (no device needed) -------------------------------- */
/* chunks_idx(range(n), n_jobs) -- jzf_flashe.py:12-16.  begins has n_jobs + 1 entries. */
int flashe_chunks(uint64_t n, uint32_t n_jobs, uint64_t *begins);
/* set_idx_list(mode="decrypt") telescoping -- jzf_flashe.py:356-367.  raw is sorted in
 * place (as the reference sorts its argument); add_out / minus_out hold n_raw entries. */
int flashe_telescope(uint32_t *raw, int n_raw, uint32_t *add_out, uint32_t *minus_out, int *n_runs);
/* AES-256 of one 16-byte block on the HOST (key schedule check / small utilities) --
 * PsuedoRandomPermutation.get_permutation, jzf_aes_prp.py:24-30. */
int flashe_prp_block(const uint8_t key[32], const uint8_t in[16], uint8_t out[16]);

/* ---- device memory, stream, events -------------------------------------------------- */
/* Device blocks come from a per-device caching allocator (new): flashe_dev_free PARKS the block (a hipMalloc + hipFree pair of a
 * 160 MB block costs more than moving it over PCIe), flashe_dev_alloc hands a parked block of the same size class out again --
 * after a device-wide synchronisation has happened since it was parked, which keeps hipFree's guarantee that kernels of any
 * stream still reading the block finish first.  FLASHE_DEV_POOL_MB bounds the parked bytes per device (default 16384, 0 = off);
 * flashe_dev_trim gives every parked block of a device back (zeroed first). */
int flashe_dev_alloc(flashe_ctx *ctx, size_t bytes, void **dptr);
int flashe_dev_free(flashe_ctx *ctx, void *dptr);
int flashe_dev_trim(int device);
int flashe_dev_pool_stats(int device, uint64_t *parked_bytes, uint64_t *hits, uint64_t *misses);
/* new: page-locked (pinned) host memory, for callers that hand host vectors to the host-pointer calls repeatedly: DMA without
 * a staging copy, and a reused buffer spares the page faults of a fresh one.  Independent of any ctx. */
int flashe_host_alloc(size_t bytes, void **hptr);
int flashe_host_free(void *hptr);
int flashe_memcpy_h2d(flashe_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int flashe_memcpy_d2h(flashe_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);
int flashe_memcpy_d2d(flashe_ctx *ctx, void *dst_dev, const void *src_dev, size_t bytes);
int flashe_memset_dev(flashe_ctx *ctx, void *dst_dev, int byte, size_t bytes);
int flashe_sync(flashe_ctx *ctx);
int flashe_event_create(flashe_ctx *ctx, void **event);
int flashe_event_destroy(flashe_ctx *ctx, void *event);
int flashe_event_record(flashe_ctx *ctx, void *event);               /* on the ctx stream */
int flashe_event_elapsed_ms(flashe_ctx *ctx, void *start, void *stop, float *ms); /* syncs on stop */
/* Make ctx's stream wait (on the device, not the host) for an event recorded by ANOTHER ctx of the
 * same device: the fork/join primitive for running e.g. the arbiter reduce on a second stream. */
int flashe_stream_wait_event(flashe_ctx *ctx, void *event);
/* new: the ctx's hipStream_t (the caller's own stream when flashe_ctx_create was handed one) -- what a framework's DLPack export
 * (__dlpack__(stream=...)) orders its pending writes before. */
int flashe_ctx_stream(const flashe_ctx *ctx, void **stream);
/* new: ctx's stream waits, on the device, for the work queued so far on `other` (a hipStream_t of the same device; NULL = the null
 * stream): the consumer side of a __cuda_array_interface__ `stream` key.  The host never blocks. */
int flashe_stream_wait_stream(flashe_ctx *ctx, void *other);
/* new: non-blocking: *done = 1 once the work before the event's last record has finished, 0 while it is pending. */
int flashe_event_query(flashe_ctx *ctx, void *event, int *done);

/* Capture and replay (HIP graphs): the *_dev calls made on ctx between begin and end are recorded instead of
 * run; launch replays the whole sequence with one submission -- for launch-bound work such as a round over a
 * LeNet-sized model (six kernels of 10-60 us).  Pointers and scalar arguments are frozen into the graph: replay
 * with new DATA in the same buffers.  Host-pointer twins, syncs and event timing are not capturable, and
 * ctx-owned scratch must already have its size: run the sequence once normally before capturing it.
 * The synchronous calls return FLASHE_EINVAL between begin and end, before they touch the stream (the capture stays intact and can
 * still end): flashe_sync, flashe_memcpy_h2d, flashe_memcpy_d2h, flashe_mean_std_dev, flashe_selftest, flashe_ctx_set_key, every
 * host-pointer twin (flashe_mask, flashe_encrypt, ...), flashe_dynamic_masking_cost_dev, flashe_rccl_allreduce_f64 and
 * flashe_rccl_barrier; so does a call whose ctx scratch would have to grow -- it has recorded nothing.  flashe_prepared_discard marks
 * its cache invalid and frees nothing there.
 * What a frozen argument block means for the cipher:
 *   - `iter` is frozen, so flashe_graph_launch REPEATS the captured round's mask streams: never feed it new plaintexts
 *     (ct1 - ct2 would equal pt1 - pt2).  For the NEXT rounds use flashe_graph_launch_shifted: every PRF kernel adds a
 *     device-resident iter shift to its frozen iter at run time, so replaying with iter_shift = r runs the captured
 *     sequence exactly as if every call in it had been made with iter + r (what round r after the captured one needs,
 *     prepare_encrypt's iter + 1 included).
 *   - the expanded key is frozen too: after flashe_ctx_set_key a graph captured earlier refuses to launch (FLASHE_EINVAL). */
typedef struct flashe_graph flashe_graph;
int flashe_graph_begin(flashe_ctx *ctx);
int flashe_graph_end(flashe_ctx *ctx, flashe_graph **graph);
int flashe_graph_launch(flashe_ctx *ctx, flashe_graph *graph);
int flashe_graph_launch_shifted(flashe_ctx *ctx, flashe_graph *graph, uint32_t iter_shift);    /* new */
int flashe_graph_destroy(flashe_graph *graph);

/* ---- PRF mask streams -------------------------------------------------------------- */
/* out[j] = sum_k term(iter, idx[k], j) mod 2^b, chunked like chunks_idx(range(n), n_jobs).
 * n_idx == 1 is _static_prepare_encrypt_single (jzf_flashe.py:19-45), i.e. one stream of
 * prepare_encrypt / prepare_decrypt (:599-666); n_idx > 1 is one half of
 * _static_prepare_decrypt / _static_prepare_decrypt_single (:85-152). */
int flashe_mask_dev(flashe_ctx *ctx, uint32_t iter, const uint32_t *idx, int n_idx,
                    uint64_t n, uint32_t n_jobs, uint64_t *out_dev);
int flashe_mask(flashe_ctx *ctx, uint32_t iter, const uint32_t *idx, int n_idx,
                uint64_t n, uint32_t n_jobs, uint64_t *out);

/* ---- encrypt / decrypt -------------------------------------------------------------- */
/* FlasheCipher.encrypt -- jzf_flashe.py:490-504 -> _multiprocessing_encrypt (:456-488,
 * double: ct = pt + term(iter, idx) - term(iter, idx+1)) or _multiprocessing_encrypt_single
 * (:431-454, single: ct = pt + term(iter, idx)), fused with the mask generation.
 * pt has pt_limbs limbs per element (1 = uint64 plaintext, zero-extended; or L). */
int flashe_encrypt_dev(flashe_ctx *ctx, uint32_t iter, uint32_t idx, int scheme,
                       uint64_t n, uint32_t n_jobs,
                       const uint64_t *pt_dev, int pt_limbs, uint64_t *ct_dev);
int flashe_encrypt(flashe_ctx *ctx, uint32_t iter, uint32_t idx, int scheme,
                   uint64_t n, uint32_t n_jobs,
                   const uint64_t *pt, int pt_limbs, uint64_t *ct);

/* n_vec independent encrypts of equal length (e.g. the clients a simulation or a multi-tenant service hosts on one
 * GPU, or the layers of one model) in as few launches as possible: ct[v] = FlasheCipher.encrypt with cipher index
 * idx[v], exactly as n_vec calls of flashe_encrypt_dev.  pt / ct are HOST arrays of n_vec device pointers.
 * int_bits > 64, double mask: runs of CONSECUTIVE cipher indices (idx[v + 1] == idx[v] + 1) share their PRF streams --
 * client c's minus stream term(iter, c + 1) is client c + 1's add stream (jzf_flashe.py:349-353) -- so a run of C clients
 * costs C + 1 AES blocks per element instead of 2 C; the ciphertexts are bit-identical to C separate calls. */
int flashe_encrypt_batch_dev(flashe_ctx *ctx, uint32_t iter, int scheme, uint64_t n, uint32_t n_jobs, int n_vec,
                             const uint32_t *idx, const uint64_t *const *pt_dev, int pt_limbs, uint64_t *const *ct_dev);

/* ---- mask precompute, resident in the ctx (FlasheCipher.prepare_encrypt / prepare_decrypt, jzf_flashe.py:599-666) ----
 * The reference computes the next round's masks in idle time and caches them in next_iter_encrypt_prepared / next_iter_decrypt_prepared;
 * the NEXT encrypt / decrypt then only adds vectors (no AES) and deletes the cache (:457, :483-486, :557-580).  Here the cache lives in
 * HBM inside the ctx -- a C caller needs no state machine of its own:
 *   flashe_prepare_encrypt(iter_next, idx, scheme, num_params): masks term(iter_next, idx) and, double mask, term(iter_next, idx + 1)
 *       of length num_params (:599-631; the caller passes iter + 1);
 *   flashe_prepare_decrypt(iter, num_clients, num_params): term(iter, num_clients) and term(iter, 0) -- nobody dropped (:633-666);
 *   flashe_encrypt_prepared[_dev](n, pt): ct = (pt + add - minus) mod 2^b from the cache, which is CONSUMED; FLASHE_EINVAL without a
 *       cache, or -- cache kept, like NumPy's broadcast error in the reference -- when n differs from num_params;
 *   flashe_decrypt_prepared[_dev](iter, extra add / minus prefixes, n, in): out = in + add - minus from the cache plus the prefixes the
 *       precompute does not cover (dropouts: what set_idx_list leaves after skipping {num_clients} / {0}, :372-386), computed online
 *       and merged in (:557-564); consumes the cache;
 *   flashe_prepared_query(which, &n, &add_dev, &minus_dev): 1 / 0 = a cache is / is not held; its length and device vectors (valid
 *       until consumed or re-prepared); flashe_prepared_discard(which) drops it (which: FLASHE_PREPARED_ENCRYPT | _DECRYPT) AND
 *       gives the mask blocks back to the device.  (A cache that is merely consumed keeps its blocks inside the ctx for the next
 *       round's masks -- up to four vectors of num_params elements per ctx -- until flashe_prepared_discard or flashe_ctx_destroy.)
 *       flashe_prepared_discard SYNCHRONISES the ctx stream before it frees (the only call of this group that does), and what it frees
 *       is what flashe_prepared_query handed out: pointers from an earlier query, and a graph captured around flashe_*_prepared_dev
 *       (its kernel arguments are those pointers), must not be used after a discard.  Inside a capture it only marks the cache invalid.
 * prepare_* are asynchronous on the ctx stream like every *_dev call. */
#define FLASHE_PREPARED_ENCRYPT 1
#define FLASHE_PREPARED_DECRYPT 2
int flashe_prepare_encrypt(flashe_ctx *ctx, uint32_t iter_next, uint32_t idx, int scheme, uint64_t num_params, uint32_t n_jobs);
int flashe_prepare_decrypt(flashe_ctx *ctx, uint32_t iter, uint32_t num_clients, uint64_t num_params, uint32_t n_jobs);
int flashe_prepared_query(flashe_ctx *ctx, int which, uint64_t *n, const uint64_t **add_dev, const uint64_t **minus_dev);
int flashe_prepared_discard(flashe_ctx *ctx, int which);
int flashe_encrypt_prepared_dev(flashe_ctx *ctx, uint64_t n, const uint64_t *pt_dev, int pt_limbs, uint64_t *ct_dev);
int flashe_encrypt_prepared(flashe_ctx *ctx, uint64_t n, const uint64_t *pt, int pt_limbs, uint64_t *ct);
int flashe_decrypt_prepared_dev(flashe_ctx *ctx, uint32_t iter, const uint32_t *add_idx, int n_add, const uint32_t *minus_idx,
                                int n_minus, uint64_t n, uint32_t n_jobs, const uint64_t *in_dev, uint64_t *out_dev);
int flashe_decrypt_prepared(flashe_ctx *ctx, uint32_t iter, const uint32_t *add_idx, int n_add, const uint32_t *minus_idx,
                            int n_minus, uint64_t n, uint32_t n_jobs, const uint64_t *in, uint64_t *out);

/* flashe_encrypt_batch_dev on ONE element slice [first, first + count) of the n-element vectors (new): the launch of a GPU that owns
 * that slice of EVERY client's vector -- element sharding, SURVEY.md section 8e (i): mask streams are position-indexed, so the slices
 * need no exchange for the element-wise aggregate.  pt_dev[v] / ct_dev[v] / sum_out_dev address element `first`; n and n_jobs still
 * describe the whole vector (the int_bits <= 64 chunking).  sum_out_dev (may be NULL): receives the slice of sum_v ct[v] mod 2^b,
 * from the same launch when flashe_encrypt_batch_sum_dev's conditions hold for the slice, from a reduce launch otherwise. */
int flashe_encrypt_batch_range_dev(flashe_ctx *ctx, uint32_t iter, int scheme, uint64_t n, uint32_t n_jobs, uint64_t first,
                                   uint64_t count, int n_vec, const uint32_t *idx, const uint64_t *const *pt_dev, int pt_limbs,
                                   uint64_t *const *ct_dev, uint64_t *sum_out_dev);

/* flashe_encrypt_batch_dev that ALSO writes the local partial aggregate sum_out[j] = sum_v ct[v][j] mod 2^b (new): what the
 * arbiter's reduce (jzf_aggregator.py:424-430) yields for the clients this GPU hosts -- SURVEY.md section 5: "each GPU encrypts and
 * locally mod-adds its share".  int_bits > 64, double mask, one run of consecutive cipher indices, a vector long enough to fill the
 * device: ONE launch (every ciphertext of an element passes through the lane's registers, the running sum costs one extra 16-byte
 * store per element and the C ciphertexts are never re-read).  Any other shape: the encrypts followed by flashe_aggregate_elem_dev.
 * The ciphertexts are written as by flashe_encrypt_batch_dev; sum_out_dev (n x L limbs) must not be one of them nor a plaintext
 * (FLASHE_EINVAL; the same holds for the _range and _u32 forms).
 * Chain decrypt mask: when that one launch runs (and the ctx is not capturing a graph), it also writes the arbiter's decrypt mask of
 * the clients idx[0] .. idx[n_vec - 1], D = term(idx[n_vec - 1] + 1) - term(idx[0]) mod 2^b, into a block the ctx holds (16 bytes
 * per element of the launch: 160 MB at n = 1e7, kept and reused; the same for the summed flashe_encrypt_batch_range_dev on its
 * slice).  A later flashe_decrypt_range_dev on this ctx with add = {idx[n_vec - 1] + 1}, minus = {idx[0]} and the same iter, key, n
 * and n_jobs on elements inside the covered ones adds D in one memory-bound pass instead of computing the two streams again.
 * flashe_ctx_set_key, flashe_graph_begin / _end / _launch* and the next summed launch invalidate it; a decrypt on another ctx never
 * sees it; flashe_prepare_decrypt's cache is not touched.  FLASHE_CHAIN_DMASK=0 in the environment at flashe_ctx_create: no mask. */
int flashe_encrypt_batch_sum_dev(flashe_ctx *ctx, uint32_t iter, int scheme, uint64_t n, uint32_t n_jobs, int n_vec,
                                 const uint32_t *idx, const uint64_t *const *pt_dev, int pt_limbs, uint64_t *const *ct_dev,
                                 uint64_t *sum_out_dev);

/* The co-located round in one call (new): a device that plays the clients idx[0] .. idx[n_vec - 1] AND the arbiter -- a simulator, a
 * cohort host -- asks for the ciphertexts, their sum and the DECRYPTED sum together.  For every shape the bytes of ct, sum_out and
 * dec_out are those of
 *     flashe_encrypt_batch_sum_dev(ctx, iter, scheme, n, n_jobs, n_vec, idx, pt_dev, pt_limbs, ct_dev, sum_out_dev), then
 *     flashe_decrypt_dev(ctx, iter, {idx[n_vec - 1] + 1}, 1, {idx[0]}, 1, n, n_jobs, sum_out_dev, dec_out_dev)
 * (jzf_aggregator.py:424-430, then jzf_flashe.py:633-666, :570-571 with nobody dropped; n_vec = 0: the zero sum, decrypted with empty
 * lists).  int_bits = 128, double mask, one-limb plaintexts, one run of consecutive cipher indices, a vector long enough to fill the
 * device and n <= 268,435,200: ONE launch -- the lane that stores an element's sum already holds sum + D, and stores it where
 * flashe_encrypt_batch_sum_dev's launch stores the decrypt mask D, so the launch moves the same bytes and the round has no second
 * pass.  Any other shape (other widths, two-limb plaintexts, the single mask, short or longer vectors, another PRF backend), or
 * FLASHE_CHAIN_DEC=0 in the environment at flashe_ctx_create: literally those two calls.
 * dec_out_dev (n x L limbs) must be aligned like a ciphertext vector (16 bytes at int_bits > 64) and must not be sum_out_dev, a
 * ciphertext or a plaintext, and idx[n_vec - 1] + 1 must fit 32 bits: FLASHE_EINVAL, nothing written.  The one launch neither uses nor
 * touches the ctx's chain decrypt mask and keeps no state: it may be captured into a graph.  The arbiter's decrypt of a sum it RECEIVED
 * (flashe_decrypt_dev after flashe_encrypt_batch_sum_dev on another call or ctx) is unchanged. */
int flashe_encrypt_batch_sum_decrypt_dev(flashe_ctx *ctx, uint32_t iter, int scheme, uint64_t n, uint32_t n_jobs, int n_vec,
                                         const uint32_t *idx, const uint64_t *const *pt_dev, int pt_limbs, uint64_t *const *ct_dev,
                                         uint64_t *sum_out_dev, uint64_t *dec_out_dev);

/* General batched form (new): every entry is one piece of mask arithmetic on elements
 * [first, first + count) of an n-element vector,
 *     out[k] = in[k] + term(iter, add_idx, first + k) - [has_minus] term(iter, minus_idx, first + k)   mod 2^b,
 * with in = 0 when in_dev is NULL; in_dev / out_dev address element `first`.  It covers, with one
 * launch for many entries (b > 64; entry by entry otherwise):
 *   FlasheCipher.encrypt (double)     add = idx, minus = idx + 1, in = plaintext   jzf_flashe.py:349-353, :480-481
 *   FlasheCipher.encrypt (single)     add = idx, has_minus = 0                     :308-309, :450-451
 *   decrypt, nobody dropped           add = num_clients, minus = 0, in = aggregate :633-666, :570-571
 *   prepare_encrypt / prepare_decrypt the same with in_dev = NULL (the cached add - minus) :599-666
 * All entries of one call must agree on has_minus.
 * n_in > 1 fuses the arbiter's reduce (jzf_aggregator.py:424-430) into the entry: the input is
 * sum_{c < n_in} of the vectors at in_dev + c * in_stride elements (in_limbs = L required), reduced
 * mod 2^b; sum_out_dev, when not NULL, receives that sum (the ciphertext aggregate). n_in = 0 means 1. */
typedef struct flashe_prf_job {
    uint32_t add_idx;
    uint32_t minus_idx;
    int32_t has_minus;       /* 0 or 1 */
    int32_t in_limbs;        /* limbs per input element: 1 (uint64, zero-extended) or L; ignored when in_dev is NULL */
    uint64_t first, count;
    const uint64_t *in_dev;
    uint64_t *out_dev;
    uint32_t n_in;           /* number of input vectors summed (0 or 1: plain input) */
    uint32_t reserved;       /* must be 0 */
    uint64_t in_stride;      /* elements between consecutive input vectors when n_in > 1 */
    uint64_t *sum_out_dev;   /* optional, n_in > 1 only */
} flashe_prf_job;
int flashe_prf_jobs_dev(flashe_ctx *ctx, uint32_t iter, uint64_t n, uint32_t n_jobs,
                        int n_entries, const flashe_prf_job *entries);

/* FlasheCipher.decrypt -- jzf_flashe.py:584-594 -> _multiprocessing_decrypt (:537-582) /
 * _multiprocessing_decrypt_single (:506-535) with the prefix lists set_idx_list derived
 * (:356-386; single: :311-314 with n_add = 0):
 * out = in + sum_k term(iter, add_idx[k]) - sum_k term(iter, minus_idx[k])  mod 2^b.
 * The lists may have ANY length, as in the reference (single mask: one minus prefix per uploaded client; scattered
 * dropouts: one pair per run); beyond 96 entries per list the call chains launches that accumulate in place.
 * in_dev == out_dev is allowed.  The same holds for flashe_mask* and the range twins. */
int flashe_decrypt_dev(flashe_ctx *ctx, uint32_t iter,
                       const uint32_t *add_idx, int n_add, const uint32_t *minus_idx, int n_minus,
                       uint64_t n, uint32_t n_jobs, const uint64_t *in_dev, uint64_t *out_dev);
int flashe_decrypt(flashe_ctx *ctx, uint32_t iter,
                   const uint32_t *add_idx, int n_add, const uint32_t *minus_idx, int n_minus,
                   uint64_t n, uint32_t n_jobs, const uint64_t *in, uint64_t *out);

/* Range twins for element-sharded execution (one vector split over several GPUs): the call
 * covers global elements [first, first + count) of an n-element vector; the device pointers
 * address element `first` (i.e. are indexed by element - first).  n and n_jobs still describe the
 * WHOLE vector, because the PRF counters depend on chunks_idx(range(n), n_jobs)
 * (jzf_flashe.py:12-16, :34).  flashe_decrypt_range_dev (and flashe_decrypt_dev) with one add and one minus index is a combine
 * with the ctx's chain decrypt mask when that mask matches the call (see flashe_encrypt_batch_sum_dev), the PRF launch otherwise;
 * the result is the same. */
int flashe_mask_range_dev(flashe_ctx *ctx, uint32_t iter, const uint32_t *idx, int n_idx,
                          uint64_t n, uint32_t n_jobs, uint64_t first, uint64_t count, uint64_t *out_dev);
int flashe_encrypt_range_dev(flashe_ctx *ctx, uint32_t iter, uint32_t idx, int scheme,
                             uint64_t n, uint32_t n_jobs, uint64_t first, uint64_t count,
                             const uint64_t *pt_dev, int pt_limbs, uint64_t *ct_dev);
int flashe_decrypt_range_dev(flashe_ctx *ctx, uint32_t iter,
                             const uint32_t *add_idx, int n_add, const uint32_t *minus_idx, int n_minus,
                             uint64_t n, uint32_t n_jobs, uint64_t first, uint64_t count,
                             const uint64_t *in_dev, uint64_t *out_dev);

/* Pre-computed-mask arithmetic: out = in + add - minus mod 2^b (add / minus may be NULL).
 * The online half of encrypt / decrypt when next_iter_{en,de}crypt_prepared is populated
 * (jzf_flashe.py:457,480-481, :557-571) and the sparse single-mask decrypt (:531-532). */
int flashe_combine_dev(flashe_ctx *ctx, uint64_t n, const uint64_t *in_dev, int in_limbs,
                       const uint64_t *add_dev, const uint64_t *minus_dev, uint64_t *out_dev);
int flashe_combine(flashe_ctx *ctx, uint64_t n, const uint64_t *in, int in_limbs,
                   const uint64_t *add, const uint64_t *minus, uint64_t *out);
/* n_vec combines of equal length in as few launches as possible (new): the online encrypts of the clients one process hosts --
 * vector v is out[v] = in[v] + add[v] - minus[v].  in / add / minus / out are HOST arrays of n_vec device pointers; add_dev,
 * minus_dev or single entries of them may be NULL. */
int flashe_combine_batch_dev(flashe_ctx *ctx, uint64_t n, int n_vec, const uint64_t *const *in_dev, int in_limbs,
                             const uint64_t *const *add_dev, const uint64_t *const *minus_dev, uint64_t *const *out_dev);
/* The same combines AND sum_out_dev = sum_v out[v] mod 2^b written by the same pass (new): the online encrypts with precomputed masks
 * (jzf_flashe.py:457, :480-481) plus the arbiter's element-wise reduce of what they wrote (jzf_aggregator.py:424-430) -- the reduce
 * costs one more store instead of a launch that reads every ciphertext back; the twin of flashe_encrypt_batch_sum_dev for the
 * precompute path.  sum_out_dev must not be one of out_dev, in_dev, add_dev or minus_dev (FLASHE_EINVAL). */
int flashe_combine_batch_sum_dev(flashe_ctx *ctx, uint64_t n, int n_vec, const uint64_t *const *in_dev, int in_limbs,
                                 const uint64_t *const *add_dev, const uint64_t *const *minus_dev, uint64_t *const *out_dev,
                                 uint64_t *sum_out_dev);
/* ... and the DECRYPT of that sum with the decrypting party's precomputed masks from the same pass (new, ABI 4): dec_out_dev =
 * (sum_out + dec_add - dec_minus) mod 2^b, i.e. jzf_flashe.py:557-571 with next_iter_decrypt_prepared populated (:633-666) applied to
 * the reduce of jzf_aggregator.py:424-430 -- the workgroup that completes an element's sum still holds it.  dec_add_dev / dec_minus_dev
 * may be NULL; dec_out_dev must be a vector of its own (not the sum, an operand or an output: FLASHE_EINVAL). */
int flashe_combine_batch_sum_decrypt_dev(flashe_ctx *ctx, uint64_t n, int n_vec, const uint64_t *const *in_dev, int in_limbs,
                                         const uint64_t *const *add_dev, const uint64_t *const *minus_dev, uint64_t *const *out_dev,
                                         uint64_t *sum_out_dev, const uint64_t *dec_add_dev, const uint64_t *dec_minus_dev, uint64_t *dec_out_dev);

/* ---- arbiter reduce ----------------------------------------------------------------- */
/* Element-wise: out[j] = sum_c cts[c][j] mod 2^b -- jzf_aggregator.py:424-430.
 * cts is a HOST array of C pointers (device pointers for _dev).  out_dev of two-limb elements must be 16-byte aligned; every
 * operand and one-limb vectors 8-byte (16-byte aligned operands take the faster 16-byte form). */
int flashe_aggregate_elem_dev(flashe_ctx *ctx, int C, const uint64_t *const *cts_dev,
                              uint64_t n, uint64_t *out_dev);
int flashe_aggregate_elem(flashe_ctx *ctx, int C, const uint64_t *const *cts,
                          uint64_t n, uint64_t *out);
/* The element-wise reduce fused with the decrypt of its result (new): agg = sum_c cts[c] mod 2^b
 * (stored to agg_out_dev unless NULL), out = agg + sum term(add) - sum term(minus) -- exactly
 * flashe_aggregate_elem_dev followed by flashe_decrypt_range_dev on elements [first, first + count)
 * of the n-element vector, in ONE pass over the ciphertexts (one launch, the aggregate never
 * re-read) for one add and at most one minus prefix -- int_bits > 64: ciphertexts equally spaced
 * in memory; int_bits <= 64: any C <= 64 operands (n < 2^32); any other shape runs the two calls.
 * cts_dev / agg_out_dev / out_dev address element `first`. */
int flashe_aggregate_decrypt_range_dev(flashe_ctx *ctx, uint32_t iter,
                                       const uint32_t *add_idx, int n_add, const uint32_t *minus_idx, int n_minus,
                                       uint64_t n, uint32_t n_jobs, uint64_t first, uint64_t count,
                                       int C, const uint64_t *const *cts_dev, uint64_t *agg_out_dev, uint64_t *out_dev);
/* Compact layout for int_bits <= 32 (new; no reference counterpart).  The ABI stores one element per uint64 limb whatever
 * int_bits is; at the widths the reference's own jobs ship (int_bits = 20, 23: jzf configs) that is
 * 8 bytes moved for 20 useful bits, and the kernels of those widths are bound by exactly those bytes.  These entry points take
 * and produce the same VALUES as uint32 arrays, so that the hot round moves half of them:
 *   flashe_encrypt_batch_u32_dev      = flashe_encrypt_batch_dev (jzf_flashe.py:456-488 per vector) on uint32 plaintexts and ciphertexts;
 *   flashe_aggregate_decrypt_u32_dev  = flashe_aggregate_decrypt_range_dev with ONE add and at most one minus prefix (the no-dropout
 *                                       decrypt and every single telescoped run, jzf_flashe.py:356-367) on up to 64 uint32 operands;
 *                                       agg_out_dev (may be NULL) and out_dev are uint32 (out_elem_bytes = 4) or uint64 (8) arrays;
 *   flashe_widen_u32_dev / flashe_narrow_u32_dev convert to and from the one-limb layout every other call uses.
 * ct[j] here == (uint32) of what the uint64 call writes; n < 2^32; table PRF; pointers address element `first`. */
int flashe_encrypt_batch_u32_dev(flashe_ctx *ctx, uint32_t iter, int scheme, uint64_t n, uint32_t n_jobs, int n_vec,
                                 const uint32_t *idx, const uint32_t *const *pt_dev, uint32_t *const *ct_dev);
/* new (round 5): flashe_encrypt_batch_u32_dev and sum_out_dev = sum_v ct_dev[v] mod 2^b from the same launch -- the compact twin of
 * flashe_encrypt_batch_sum_dev.  One launch for consecutive clients under the double mask at int_bits 16 / 20 / 23 / 24 / 32 when the vectors are
 * long enough for the paired kernel; every other shape runs the encrypts and then the reduce of what they wrote (same results). */
int flashe_encrypt_batch_sum_u32_dev(flashe_ctx *ctx, uint32_t iter, int scheme, uint64_t n, uint32_t n_jobs, int n_vec, const uint32_t *idx,
                                     const uint32_t *const *pt_dev, uint32_t *const *ct_dev, uint32_t *sum_out_dev);
int flashe_aggregate_decrypt_u32_dev(flashe_ctx *ctx, uint32_t iter,
                                     const uint32_t *add_idx, int n_add, const uint32_t *minus_idx, int n_minus,
                                     uint64_t n, uint32_t n_jobs, uint64_t first, uint64_t count,
                                     int C, const uint32_t *const *cts_dev, void *agg_out_dev, void *out_dev, int out_elem_bytes);
/* The arbiter's element-wise reduce (jzf_aggregator.py:424-430) on uint32 vectors: out[j] = sum_c cts[c][j] mod 2^b; any C >= 1
 * (partial sums accumulate in out_dev beyond 64 operands), out_dev may be one of the operands only when C <= 64. */
int flashe_aggregate_elem_u32_dev(flashe_ctx *ctx, int C, const uint32_t *const *cts_dev, uint64_t n, uint32_t *out_dev);
int flashe_widen_u32_dev(flashe_ctx *ctx, uint64_t n, const uint32_t *in_dev, uint64_t *out_dev);
int flashe_narrow_u32_dev(flashe_ctx *ctx, uint64_t n, const uint64_t *in_dev, uint32_t *out_dev);
/* Packed: each operand is ONE integer of total_bits bits (n_limbs = ceil(total_bits/64)
 * little-endian limbs); out = sum mod 2^total_bits -- jzf_aggregator.py:406-419. */
int flashe_aggregate_packed_dev(flashe_ctx *ctx, int C, const uint64_t *const *packed_dev,
                                uint64_t n_limbs, uint64_t total_bits, uint64_t *out_dev);
int flashe_aggregate_packed(flashe_ctx *ctx, int C, const uint64_t *const *packed,
                            uint64_t n_limbs, uint64_t total_bits, uint64_t *out);
/* new: the same sum (jzf_aggregator.py:406-419) computed on UNPACKED vectors, out = unpack(sum_c pack(cts[c]) mod 2^(int_bits n)) with
 * element j at bit (n - 1 - j) int_bits, in one pass and with no packed vector: the column sums' high parts and a one-bit carry run
 * from element n - 1 towards element 0 as a scan over the elements; what leaves element 0 is dropped.  Bits of an operand above int_bits
 * are ignored, as flashe_pack_dev ignores them.  Operands and out are laid out and aligned as for flashe_aggregate_elem_dev (the _u32
 * form: as for flashe_aggregate_elem_u32_dev, int_bits <= 32), but out must NOT be one of the operands (FLASHE_EINVAL).  n = 0 is
 * FLASHE_OK with nothing launched.  More than 64 operands go in passes whose partial results ping-pong through ctx scratch.  The carry
 * is one bit only while the operands of a pass number at most 2^int_bits: beyond that (int_bits < 6) FLASHE_ENOTSUP -- nothing launched,
 * out untouched; pack, flashe_aggregate_packed_dev and unpack instead.  The first call on a ctx sizes its block summaries, so it cannot
 * be inside a graph capture.  Measured by device events against C flashe_pack_dev + flashe_aggregate_packed_dev + flashe_unpack_dev on the
 * same operands (tests/perf/packed_elems_reduce.py, profiles/r31_packed_elems_reduce.log): n = 1e7, int_bits 128, C = 10: 0.317 against
 * 0.938 ms; n = 25,557,032, int_bits 20, C = 10, uint32 operands (every pointer 16-byte aligned: four elements per lane): 0.220 against
 * 1.425 ms with the widens that sequence needs.  Other shapes: not measured. */
int flashe_aggregate_packed_elems_dev(flashe_ctx *ctx, int C, const uint64_t *const *cts_dev, uint64_t n, uint64_t *out_dev);
int flashe_aggregate_packed_elems_u32_dev(flashe_ctx *ctx, int C, const uint32_t *const *cts_dev, uint64_t n, uint32_t *out_dev);

/* Slice helpers (new; no reference counterpart): the packed reduce above cut into limb slices
 * over several GPUs ("packed variant") needs each slice's carry-out and
 * the one way a carry-in can ripple through a whole slice.
 * probe: x_dev holds n_limbs - 1 body limbs plus one carry limb (the slice was summed one limb
 * wider than it is).  info_dev[0] = x[0]; info_dev[1] = 1 iff body limbs [1, n_limbs - 1) are
 * all ones; info_dev[2] = x[n_limbs - 1].  Asynchronous; info_dev is device memory (24 bytes).
 * add_carry: x = (x + carry_in) mod 2^total_bits in place, n_limbs = ceil(total_bits / 64). */
int flashe_packed_probe_dev(flashe_ctx *ctx, uint64_t n_limbs, const uint64_t *x_dev, uint64_t *info_dev);
int flashe_packed_add_carry_dev(flashe_ctx *ctx, uint64_t n_limbs, uint64_t total_bits,
                                uint64_t carry_in, uint64_t *x_dev);
/* add_carry with the carry-in derived ON THE DEVICE from the probe triples of the n_below slices underneath (infos_dev =
 * the all-gathered 3-word infos, slice 0 first): no host round trip between the exchange of the infos and the ripple. */
int flashe_packed_resolve_carry_dev(flashe_ctx *ctx, uint64_t n_limbs, uint64_t total_bits,
                                    const uint64_t *infos_dev, int n_below, uint64_t *x_dev);
/* The same with the triples `stride_words` apart (a non-zero multiple of 3; infos_dev points at the LOWEST slice's triple): -3 walks
 * gathered triples that run from the most significant slice down -- element slices of a packed vector, whose element 0 is the most
 * significant (jzf_weights.py:59-62), gathered in rank order. */
int flashe_packed_resolve_carry_strided_dev(flashe_ctx *ctx, uint64_t n_limbs, uint64_t total_bits, const uint64_t *infos_dev,
                                            int n_below, int stride_words, uint64_t *x_dev);              /* new */

/* ---- bit-packing codec ---------------------------------------------------------------- */
/* pack: P = sum_j x[j] << (b * (n-1-j)) as ceil(n*b/64) little-endian limbs --
 * _to_bytes / _to_bytes_old + compress(), jzf_weights.py:36-84, :155-195.
 * unpack: the inverse -- _from_bytes_old + reverse(), jzf_weights.py:87-95, :197-231. */
int flashe_pack_dev(flashe_ctx *ctx, uint64_t n, const uint64_t *in_dev, uint64_t *out_dev);
int flashe_pack(flashe_ctx *ctx, uint64_t n, const uint64_t *in, uint64_t *out);
int flashe_unpack_dev(flashe_ctx *ctx, uint64_t n, const uint64_t *in_dev, uint64_t *out_dev);
int flashe_unpack(flashe_ctx *ctx, uint64_t n, const uint64_t *in, uint64_t *out);

/* ---- sparse path --------------------------------------------------------------------- */
/* Location lists live in device memory in the *_dev variants, so they cannot be validated before launch: a location
 * >= total (the reference raises IndexError there) -- or, in the "sorted" variants, an entry that is not strictly
 * increasing -- is SKIPPED by the kernels, nothing is written outside the dense vector, and the next synchronising call
 * on the ctx (flashe_sync, flashe_memcpy_d2h) returns FLASHE_EINVAL once.  The host-pointer twins validate up front. */
/* Arbiter.expand_to_dense -- jzf_aggregator.py:150-165: out[loc[q]] = vals[q], every other
 * of the `total` positions = zero (L limbs, HOST pointer in both variants). */
int flashe_expand_to_dense_dev(flashe_ctx *ctx, uint64_t total, uint64_t k, const uint32_t *loc_dev,
                               const uint64_t *vals_dev, const uint64_t *zero, uint64_t *out_dev);
int flashe_expand_to_dense(flashe_ctx *ctx, uint64_t total, uint64_t k, const uint32_t *loc,
                           const uint64_t *vals, const uint64_t *zero, uint64_t *out);
/* The sparse job's arbiter step as one operation (new): out = sum_c expand_to_dense(total, loc[c], vals[c], zero_c)
 * mod 2^b -- Arbiter.expand_to_dense (jzf_aggregator.py:150-165, :382-384) for every client followed by the
 * element-wise reduce (:424-430) -- without materialising the C dense vectors: the sum of the zero values is
 * written everywhere, then each client's (vals[q] - zero_c) is added at loc[c][q].  loc / vals are HOST arrays of
 * C device pointers, k a HOST array, zeros a HOST array of C x L limbs; locations are distinct within a client.
 * sorted != 0 promises that every loc[c] is strictly increasing -- what Client.sparsify emits (jzf_aggregator.py:598,
 * :604) -- and selects the one-pass form: spans of the dense vector are accumulated in LDS and written once. */
int flashe_sparse_aggregate_dev(flashe_ctx *ctx, uint64_t total, int C, const uint32_t *const *loc_dev, const uint64_t *k,
                                const uint64_t *const *vals_dev, const uint64_t *zeros, int sorted, uint64_t *out_dev);
/* Sparse single-mask dense minus-mask -- set_idx_list_single sparse branch,
 * jzf_flashe.py:316-343: for client c the stream over COMPACT positions 0..k[c]-1 (prefix
 * iter|c, chunks_idx(range(k[c]), n_jobs)) scattered to loc[c][q] and summed over clients.
 * loc is a HOST array of C pointers, k a HOST array. */
int flashe_sparse_minus_mask_dev(flashe_ctx *ctx, uint32_t iter, int C, const uint32_t *const *loc_dev,
                                 const uint64_t *k, uint64_t total, uint32_t n_jobs, uint64_t *out_dev);
/* The same for strictly increasing location lists (see flashe_sparse_aggregate_dev); the host-pointer twin picks it by
 * itself when the lists qualify. */
int flashe_sparse_minus_mask_sorted_dev(flashe_ctx *ctx, uint32_t iter, int C, const uint32_t *const *loc_dev,
                                        const uint64_t *k, uint64_t total, uint32_t n_jobs, uint64_t *out_dev);
/* The single-mask sparse DECRYPT in the pass that builds the mask: out = (agg - minus-mask) mod 2^b, i.e. set_idx_list_single's
 * sparse branch (jzf_flashe.py:316-343) followed by _multiprocessing_decrypt_single's `value - minus` (:531-532) without the dense
 * mask ever reaching HBM.  Same arguments as flashe_sparse_minus_mask[_sorted]_dev plus the aggregate (total x L limbs, must not be out_dev).
 * new: fusion of two reference steps. */
int flashe_sparse_decrypt_dev(flashe_ctx *ctx, uint32_t iter, int C, const uint32_t *const *loc_dev, const uint64_t *k,
                              uint64_t total, uint32_t n_jobs, int sorted, const uint64_t *agg_dev, uint64_t *out_dev);
/* Span bounds of a round's location lists, computed ONCE (new).  The LDS-staged sparse passes cut the dense vector into spans and
 * first find, for every span, where each client's (strictly increasing) list enters it -- a pass over all lists that the sparse
 * aggregate and the sparse decrypt of one round would otherwise both run on the same lists.  (The handle carries a table for both
 * span sizes in use: the one the ctx's hot passes read -- the passes with the PRF inside where the ctx has them -- is filled by create /
 * recompute, the plain reduce's by the first call that needs it, on THAT call's ctx stream; inside a graph capture that fill is part
 * of the graph.)  flashe_span_bounds_create computes the
 * table for C lists (any C) asynchronously on the ctx stream; the *_bounds_dev calls take it instead of recomputing; the handle is valid
 * for exactly these list pointers / lengths / total (checked) and until flashe_span_bounds_destroy.  The table describes the lists'
 * CONTENTS, which the check cannot see: the lists must not change while a handle built on them is in use, and after any in-place
 * rewrite (a job that reuses its upload buffers every round) flashe_span_bounds_recompute is MANDATORY before the next *_bounds_dev /
 * *_range_dev call -- a stale table stays memory-safe (slices are clamped, an entry outside its span raises the ctx's deferred error
 * flag) but the sums are wrong. */
typedef struct flashe_span_bounds flashe_span_bounds;
int flashe_span_bounds_create(flashe_ctx *ctx, uint64_t total, int C, const uint32_t *const *loc_dev, const uint64_t *k,
                              flashe_span_bounds **out);
/* the same handle for the next round's lists (same total and C): recomputed in place, asynchronously, without an allocation */
int flashe_span_bounds_recompute(flashe_ctx *ctx, flashe_span_bounds *bounds, const uint32_t *const *loc_dev, const uint64_t *k);
void flashe_span_bounds_destroy(flashe_span_bounds *bounds);
int flashe_sparse_aggregate_bounds_dev(flashe_ctx *ctx, uint64_t total, int C, const uint32_t *const *loc_dev, const uint64_t *k,
                                       const uint64_t *const *vals_dev, const uint64_t *zeros, const flashe_span_bounds *bounds,
                                       uint64_t *out_dev);
int flashe_sparse_decrypt_bounds_dev(flashe_ctx *ctx, uint32_t iter, int C, const uint32_t *const *loc_dev, const uint64_t *k,
                                     uint64_t total, uint32_t n_jobs, const flashe_span_bounds *bounds, const uint64_t *agg_dev,
                                     uint64_t *out_dev);
/* The sparse twin of flashe_encrypt_batch_sum_dev (new): the C clients this device plays encrypt their compact uploads with the single
 * mask -- ct_dev[c] = flashe_encrypt_dev(iter, idx[c], SINGLE, k[c], n_jobs) of pt_dev[c] (jzf_flashe.py:471-478) -- AND the sum of
 * their expanded uploads, flashe_sparse_aggregate_dev(loc_dev, ct_dev, zeros) (jzf_aggregator.py:150-165, :419-430), is written to
 * agg_out_dev in the same pass.  int_bits > 64 on the table PRF: ONE persistent launch per 64 clients computes every entry's mask block
 * inside the LDS-staged span reduce (the ciphertexts are stored on the way, the compact values never travel twice); int_bits <= 64 and
 * the bit-sliced backends: the two calls it stands for (measured faster at that width; the position-range form below runs the fused
 * pass at every int_bits, one block serving the up to 128 / int_bits entries of a chunk that share it).  loc_dev[c] strictly increasing; bounds: NULL or the handle of exactly these lists. */
int flashe_sparse_encrypt_aggregate_dev(flashe_ctx *ctx, uint32_t iter, uint32_t n_jobs, uint64_t total, int C, const uint32_t *idx,
                                        const uint32_t *const *loc_dev, const uint64_t *k, const uint64_t *const *pt_dev, int pt_limbs,
                                        const uint64_t *zeros, const flashe_span_bounds *bounds, uint64_t *const *ct_dev,
                                        uint64_t *agg_out_dev);
/* The sparse round sharded by POSITION ranges over several GPUs (new; SURVEY 8e (i) for the sparse path): GPU g owns the positions
 * [first, first + count) of the dense vector and runs every client's entries that fall into them -- counters and list indices stay
 * global (the full lists and their bounds handle are passed), nothing is exchanged for the aggregate.  first is a multiple of
 * flashe_sparse_span(), first + count one or the end of the vector; agg_out_dev / agg_dev / out_dev address position `first`; only the
 * ciphertexts of entries inside the range are written.  Any int_bits on the table PRF, strictly increasing lists, bounds required. */
int flashe_sparse_span(void);
int flashe_sparse_encrypt_aggregate_range_dev(flashe_ctx *ctx, uint32_t iter, uint32_t n_jobs, uint64_t total, int C, const uint32_t *idx,
                                              const uint32_t *const *loc_dev, const uint64_t *k, const uint64_t *const *pt_dev,
                                              int pt_limbs, const uint64_t *zeros, const flashe_span_bounds *bounds, uint64_t first,
                                              uint64_t count, uint64_t *const *ct_dev, uint64_t *agg_out_dev);
int flashe_sparse_decrypt_range_dev(flashe_ctx *ctx, uint32_t iter, int C, const uint32_t *const *loc_dev, const uint64_t *k,
                                    uint64_t total, uint32_t n_jobs, const flashe_span_bounds *bounds, uint64_t first, uint64_t count,
                                    const uint64_t *agg_dev, uint64_t *out_dev);
int flashe_sparse_minus_mask(flashe_ctx *ctx, uint32_t iter, int C, const uint32_t *const *loc,
                             const uint64_t *k, uint64_t total, uint32_t n_jobs, uint64_t *out);
/* Dense-position selected masks -- _static_prepare_decrypt_spar as ONE chunk
 * (jzf_flashe.py:155-225, begin = 0): out[p] = sum_i sel[i][p] * term(iter, i, p) mod 2^b,
 * sel[i] a 0/1 byte vector of length total.  sel is a HOST array of n_lists pointers. */
/* The sparse branch of set_idx_list for the DOUBLE mask as one operation (new) -- jzf_flashe.py:388-426 (per-position run analysis of
 * the clients' one-hot location vectors) + _static_prepare_decrypt_spar (:155-225, dense-position counters, one chunk, begin = 0):
 *   add_out[p]   = sum over clients c that hold p while client c + 1 does not (or c is the last) of term(iter, c + 1, p)
 *   minus_out[p] = sum over clients c that hold p while client c - 1 does not (or c is the first) of term(iter, c, p)      (mod 2^b)
 * straight from the clients' STRICTLY INCREASING location lists (what Client.sparsify emits): every list entry looks its position up
 * in the two neighbouring lists and computes at most two AES blocks, the span reduce scatters the compact values -- sum_c k_c block
 * pairs instead of (C + 1) x total blocks, no one-hot vectors of `total` bytes per list (the reference itself skips blocks without a
 * selected slot, :170, :201).  loc is a HOST array of C device pointers, k a HOST array; add_out / minus_out: total x L limbs each. */
int flashe_sparse_double_masks_dev(flashe_ctx *ctx, uint32_t iter, int C, const uint32_t *const *loc_dev, const uint64_t *k,
                                   uint64_t total, uint64_t *add_out_dev, uint64_t *minus_out_dev);
/* The arbiter's per-round choice between single and double masks for a sparse job (Arbiter.dynamic_masking,
 * jzf_flashe_block.py:92-112): single_cost = 2 sum_c len(mask_c); double_cost = 2 single_cost - 2 canceled, canceled = the positions
 * consecutive clients share (the reference ANDs one-hot vectors of `total` entries per pair).  Here every list entry of client c is
 * looked up in client c + 1's list on the device -- no one-hots, sum_c k_c binary searches.  loc_dev: HOST array of C device pointers
 * to STRICTLY INCREASING lists (what Client.sparsify emits), k: HOST array of their lengths.  The caller decides: "single" iff
 * single_cost <= double_cost (:106).  Synchronous. */
int flashe_dynamic_masking_cost_dev(flashe_ctx *ctx, int C, const uint32_t *const *loc_dev, const uint64_t *k,
                                    uint64_t *single_cost, uint64_t *double_cost);
int flashe_sparse_dense_mask_dev(flashe_ctx *ctx, uint32_t iter, int n_lists, const uint8_t *const *sel_dev,
                                 uint64_t total, uint64_t *out_dev);
int flashe_sparse_dense_mask(flashe_ctx *ctx, uint32_t iter, int n_lists, const uint8_t *const *sel,
                             uint64_t total, uint64_t *out);

/* ---- quantise / batch codec either side of the cipher ------------------ */
/* Fused forms (new): the quantiser is the step immediately before encrypt and after decrypt (QuantizingClient.quantize ->
 * JZFWeights.encrypted, decrypted -> unquantize; jzf_quantize.py:394-491, jzf_weights.py:334-338), so one launch does both and the
 * 8-byte integer never makes a round trip through HBM:
 *   quantize_encrypt: ct[j] = encrypt(_static_quantize_padding_asymmetric(x, alpha, element_bits)[j]), u_dev = the uniform draws;
 *   decrypt_unquantize: out[j] = _static_unquantize_padding_asymmetric(decrypt(in)[j], alpha, element_bits, num_clients) as float64.
 * Bit-identical to the two-call sequences.  Un-batched values only (one quantised value per ciphertext element). */
int flashe_quantize_encrypt_dev(flashe_ctx *ctx, uint32_t iter, uint32_t idx, int scheme, uint64_t n, uint32_t n_jobs,
                                const void *x_dev, int x_is_f64, double alpha, int element_bits, const double *u_dev,
                                uint64_t *ct_dev);
int flashe_decrypt_unquantize_dev(flashe_ctx *ctx, uint32_t iter, const uint32_t *add_idx, int n_add,
                                  const uint32_t *minus_idx, int n_minus, uint64_t n, uint32_t n_jobs,
                                  const uint64_t *in_dev, double alpha, int element_bits, int num_clients, double *out_dev);
/* The same for a whole FLATTENED model in one launch -- what a reference job computes (Client.secure_aggregate,
 * jzf_aggregator.py:721-741: QuantizingClient.quantize layer by layer, each layer with its own alpha, then Client.flatten_weights
 * :625-650 and ONE cipher.encrypt over the concatenation; back: cipher.decrypt of the one vector, Client.unflatten_weights :652-671,
 * unquantize layer by layer :887-899).  The PRF counters -- and for int_bits <= 64 the chunks_idx(range(n), n_jobs) chunking --
 * therefore run across the layers: n is the length of the flattened vector, the call covers its elements [first, first + count)
 * (ct_dev / in_dev / u_dev / out_dev address element `first`), and `layers` (HOST array, ascending `start`, layers[0].start == 0)
 * says which alpha -- and, quantize_encrypt, which device array -- flat element j belongs to: the last entry with start <= j.
 * x_dev of a layer points to that layer's OWN first value (the layers need not be contiguous in HBM and may mix float32 and
 * float64); decrypt_unquantize ignores x_dev / x_is_f64.  u_dev[k] = the stochastic-rounding draw of flat element first + k: the
 * reference draws np.random.random(layer.shape) layer by layer in walking order (jzf_quantize.py:61 under :417-462), i.e. one
 * stretch of NumPy's stream in flat order.  Not capturable into a graph (the table is staged per call). */
typedef struct flashe_codec_layer {
    uint64_t start;        /* flat index of the layer's first value */
    const void *x_dev;     /* quantize_encrypt: the layer's float32 / float64 values */
    double alpha;          /* the layer's clipping threshold (QuantizingClient.alpha_list; 1.0 for the sparse job's 'zzz' layer) */
    int32_t x_is_f64;
    int32_t reserved;      /* 0 */
} flashe_codec_layer;
int flashe_quantize_encrypt_model_dev(flashe_ctx *ctx, uint32_t iter, uint32_t idx, int scheme, uint64_t n, uint32_t n_jobs,
                                      uint64_t first, uint64_t count, const flashe_codec_layer *layers, int n_layers,
                                      int element_bits, const double *u_dev, uint64_t *ct_dev);
int flashe_decrypt_unquantize_model_dev(flashe_ctx *ctx, uint32_t iter, const uint32_t *add_idx, int n_add,
                                        const uint32_t *minus_idx, int n_minus, uint64_t n, uint32_t n_jobs, uint64_t first,
                                        uint64_t count, const uint64_t *in_dev, const flashe_codec_layer *layers, int n_layers,
                                        int element_bits, int num_clients, double *out_dev);
/* The same back end WITHOUT a decrypt (new): in_dev holds plaintext sums already -- the sparse job's way back, whose decrypt is the
 * sparse minus-mask pass (flashe_sparse_decrypt_dev), not a prefix list; element first + k of the flattened model -> out_dev[k]. */
int flashe_unquantize_model_dev(flashe_ctx *ctx, uint64_t n, uint64_t first, uint64_t count, const uint64_t *in_dev,
                                const flashe_codec_layer *layers, int n_layers, int element_bits, int num_clients, double *out_dev);
/* The BATCHED form of the same job (the paper's main configuration, "batch": true): QuantizingClient.quantize packs
 * batch_size = int_bits / field_bits quantised values (field_bits = element_bits + ceil(log2(num_clients))) into every ciphertext element,
 * first value most significant, EVERY LAYER padded with zeros to whole elements on its own (_static_batching_padding_asymmetric,
 * jzf_quantize.py:162-185 under :436-451); flatten_weights then concatenates the batched layers and the cipher encrypts that vector.
 * quantize_batch_model: one launch from the layers' float values (x_dev per layer) and the model's uniform draws (u_dev[j] = draw of the
 * j-th value in walking order) to the flattened batched plaintext out_dev[n_elems][L] (then flashe_encrypt_dev); unbatch_unquantize_model:
 * one launch from the decrypted flattened vector to the model's float64 values in walking order (_static_unbatching_padding_asymmetric
 * :234-251, the `[:size]` cut of QuantizingClient.unquantize :509-513, _static_unquantize_padding_asymmetric :102-107).
 * n_elems must equal sum over layers of ceil(size / batch_size).  layers is a HOST array. */
typedef struct flashe_batch_layer {
    uint64_t size;         /* values in the layer */
    const void *x_dev;     /* quantize_batch_model: the layer's float32 / float64 values; ignored on the way back */
    double alpha;
    int32_t x_is_f64;
    int32_t reserved;      /* 0 */
} flashe_batch_layer;
int flashe_quantize_batch_model_dev(flashe_ctx *ctx, const flashe_batch_layer *layers, int n_layers, int element_bits, int field_bits,
                                    const double *u_dev, uint64_t n_elems, uint64_t *out_dev);
int flashe_unbatch_unquantize_model_dev(flashe_ctx *ctx, const flashe_batch_layer *layers, int n_layers, int element_bits,
                                        int field_bits, int num_clients, const uint64_t *in_dev, uint64_t n_elems, double *out_dev);
/* QuantizingClient.normalize / unnormalize (jzf_quantize.py:542-564): x <- x + shift in place (normalize passes -mean).  wide: for
 * float32 arrays the addition runs in float64 and is rounded once -- NumPy's loop when the scalar is a float64 (np.mean / np.std
 * results), as opposed to a Python float; bit-exact either way.  mean_std: the per-layer statistics unnormalize records for the next
 * round's alpha, accumulated in float64 by a two-pass parallel reduction; NOT bit-identical to NumPy's summation order (the
 * reference sums a Python-float object array left to right): agreement is to ~1e-12 relative, tests use 1e-10.  Synchronous. */
int flashe_shift_dev(flashe_ctx *ctx, uint64_t n, void *x_dev, int x_is_f64, double shift, int wide);
int flashe_mean_std_dev(flashe_ctx *ctx, uint64_t n, const void *x_dev, int x_is_f64, double *mean, double *stddev);

/* Caller-owned tensors either side of the model-wide codec (new): a training framework's layers in HBM, handed over by pointer (DLPack /
 * __cuda_array_interface__ on the Python side), in their own dtype.  One flashe_tensor_layer per layer (HOST array, ascending start,
 * layers[0].start == 0, the last entry with start <= j holds flat element j; ptr points to the layer's own first value, C-contiguous).
 * dtype: FLASHE_TENSOR_F32 / F64 / F16 / BF16.  flags: FLASHE_TENSOR_SHIFT adds `shift` (normalize passes -mean, unnormalize +mean:
 * QuantizingClient.normalize / unnormalize, jzf_quantize.py:542-564); FLASHE_TENSOR_SHIFT_WIDE: a float32 add runs in float64 and is
 * rounded once (NumPy's loop for an np.float64 scalar, as flashe_shift_dev's `wide`); FLASHE_TENSOR_LOOP_F64: the front end quantises a
 * 32- or 16-bit layer in float64 (NumPy's loop dtype for a float32 array and an np.float64 alpha, jzf_quantize.py:55-67 under :394-491). */
#define FLASHE_TENSOR_F32 0
#define FLASHE_TENSOR_F64 1
#define FLASHE_TENSOR_F16 2
#define FLASHE_TENSOR_BF16 3
#define FLASHE_TENSOR_SHIFT 1
#define FLASHE_TENSOR_SHIFT_WIDE 2
#define FLASHE_TENSOR_LOOP_F64 4
typedef struct flashe_tensor_layer {
    uint64_t start;        /* flat index of the layer's first value */
    void *ptr;             /* the layer's values (front end: read; flashe_store_layers_dev: written) */
    double alpha;          /* front end: the clipping threshold (as flashe_codec_layer.alpha); ignored by flashe_store_layers_dev */
    double shift;          /* with FLASHE_TENSOR_SHIFT */
    int32_t dtype;         /* F32 0, F64 1, F16 2, BF16 3 */
    int32_t flags;         /* SHIFT 1, SHIFT_WIDE 2, LOOP_F64 4 */
} flashe_tensor_layer;
/* Front end, jzf_quantize.py:55-67, 542-547 (normalize): the same contract as flashe_quantize_encrypt_model_dev with tensor layers.  A
 * layer already in its compute type without SHIFT is read where it lies; every other layer touched by [first, first + count) is
 * converted by one streaming pass into ctx scratch -- a 16-bit value upcast to float32 exactly, SHIFT applied in float32 (float64 for an
 * F64 layer), then widened exactly with LOOP_F64 -- and read from there.  The table upload synchronises. */
int flashe_quantize_encrypt_tensors_dev(flashe_ctx *ctx, uint32_t iter, uint32_t idx, int scheme, uint64_t n, uint32_t n_jobs,
                                        uint64_t first, uint64_t count, const flashe_tensor_layer *layers, int n_layers,
                                        int element_bits, const double *u_dev, uint64_t *ct_dev);
/* A COHORT of n_clients consecutive clients (cipher indices first_idx .. first_idx + n_clients - 1, double mask) hosted on this GPU (new):
 * ONE chained launch quantises every client's float model (jzf_quantize.py:55-67, client c's element k with the draw
 * u_dev[c * n + k]), encrypts with the PRF streams the consecutive clients share (n_clients + 1 streams instead of 2 n_clients,
 * jzf_flashe.py:349-353), and writes ct_dev[c] (n x L limbs each, bit for bit flashe_quantize_encrypt_tensors_dev of that client),
 * sum_out_dev = sum_c ct_dev[c] mod 2^b (jzf_aggregator.py:424-430) and, when dmask_dev is not NULL, the cohort's decrypt mask
 * term(first_idx + n_clients) - term(first_idx) mod 2^b (what a decrypt of the sum adds when the cohort is the whole federation; feed it
 * to flashe_combine_unquantize_model_dev).  No integer plaintext exists in HBM.  `layers` is ONE table shared by all clients (HOST
 * array, rows as above; ptr is ignored, dtype names the row's COMPUTE type F32 / F64, LOOP_F64 makes an F32 row compute in float64,
 * SHIFT / SHIFT_WIDE / shift normalise every client's layer alike); src_dev[c * n_layers + l] is client c's layer l and
 * src_dtype[c * n_layers + l] its storage dtype (NULL: the row's dtype).  A source already in the row's compute type without SHIFT is
 * read in place; the others take one stage pass into ctx scratch first (as flashe_quantize_encrypt_tensors_dev), all clients at once.
 * A float64 source under a float32 row is FLASHE_EINVAL.
 * Returns FLASHE_ENOTSUP -- nothing launched -- for every shape outside the chained launch: int_bits <= 64, more than 128 clients, fewer
 * than two 256-element tiles per wave of the chip (2 x 16 x flashe_ctx_cu_count tiles), n > 2^32, FLASHE_CHAIN=0, another PRF backend;
 * the caller then quantises per client and uses flashe_encrypt_batch_sum_dev.  The table uploads synchronise; not capturable. */
int flashe_quantize_encrypt_cohort_dev(flashe_ctx *ctx, uint32_t iter, uint32_t first_idx, int n_clients, uint64_t n, uint32_t n_jobs,
                                       const flashe_tensor_layer *layers, int n_layers, const void *const *src_dev, const int32_t *src_dtype,
                                       int element_bits, const double *u_dev, uint64_t *const *ct_dev, uint64_t *sum_out_dev, uint64_t *dmask_dev);
/* The same cohort at the widths the reference's jobs ship, in the compact layout (new): int_bits 16 / 20 / 23 / 24 / 32, ct_dev[c] and
 * sum_out_dev are uint32 arrays of n elements (4-byte aligned, the values of flashe_quantize_encrypt_tensors_dev of client c and their
 * sum mod 2^b, as the other *_u32_dev entry points lay them out), no decrypt mask (a decrypt at these widths is 2 / m AES blocks per
 * element, m = 128 / int_bits).  ONE chained launch from the floats: per value and client it reads the float and its draw and writes
 * 4 bytes; no integer plaintext exists in HBM.  layers, src_dev, src_dtype, u_dev and the stage pass are those of
 * flashe_quantize_encrypt_cohort_dev; the counters follow the chunking of n_jobs.
 * Returns FLASHE_ENOTSUP -- nothing launched -- for every shape outside the launch: a ctx whose flashe_ctx_compact_layout is 0, another
 * int_bits, more than 128 clients, n = 0 or n >= 2^32, fewer AES blocks than 2 x 128 x 16 x flashe_ctx_cu_count (the vector has
 * r ceil((d + 1) / m) + (n_jobs - r) ceil(d / m) of them, d = n / n_jobs, r = n % n_jobs); the caller then quantises per client and uses
 * flashe_encrypt_batch_sum_u32_dev.  The table uploads synchronise; not capturable. */
int flashe_quantize_encrypt_cohort_u32_dev(flashe_ctx *ctx, uint32_t iter, uint32_t first_idx, int n_clients, uint64_t n, uint32_t n_jobs,
                                           const flashe_tensor_layer *layers, int n_layers, const void *const *src_dev, const int32_t *src_dtype,
                                           int element_bits, const double *u_dev, uint32_t *const *ct_dev, uint32_t *sum_out_dev);
/* The same cohort at int_bits 33 .. 64 in the one-limb layout (new), jzf_quantize.py:55-67, jzf_flashe.py:349-353, jzf_aggregator.py:424-430:
 * the widths of a job that quantises finer than the compact layout carries (element_bits 32 with 2 .. 10 clients: int_bits 33 .. 36).
 * ct_dev[c] and sum_out_dev are uint64 arrays of n elements (8-byte aligned: the values of flashe_quantize_encrypt_tensors_dev of client c
 * and their sum mod 2^b), no decrypt mask (a decrypt at these widths is 2 / m AES blocks per element, m = 128 / int_bits = 2 or 3).  ONE
 * chained launch from the floats: per value and client it reads the float and its draw and writes 8 bytes; no integer plaintext exists
 * in HBM.  layers, src_dev, src_dtype, u_dev and the stage pass are those of flashe_quantize_encrypt_cohort_dev; the counters follow the
 * chunking of n_jobs.
 * Returns FLASHE_ENOTSUP -- nothing launched -- for every shape outside the launch: another int_bits, more than 128 clients, n = 0 or
 * n >= 2^32, fewer AES blocks than 2 x 128 x 16 x flashe_ctx_cu_count (counted as for flashe_quantize_encrypt_cohort_u32_dev),
 * FLASHE_CHAIN=0, another PRF backend; the caller then quantises per client and uses flashe_encrypt_batch_sum_dev.  The table uploads
 * synchronise; not capturable. */
int flashe_quantize_encrypt_cohort_u64_dev(flashe_ctx *ctx, uint32_t iter, uint32_t first_idx, int n_clients, uint64_t n, uint32_t n_jobs,
                                           const flashe_tensor_layer *layers, int n_layers, const void *const *src_dev, const int32_t *src_dtype,
                                           int element_bits, const double *u_dev, uint64_t *const *ct_dev, uint64_t *sum_out_dev);
/* A SHORT cohort (new), jzf_quantize.py:394-491, jzf_flashe.py:349-353, 480-481, jzf_aggregator.py:424-430: the two cohort launches above
 * decline a vector that does not fill the chip uncut, and many clients with a small model is the shape a federation simulated on one card
 * most often has.  The three entry points below take any n >= 1: the summed chain is CUT into `parts` runs of consecutive clients,
 * piece p = clients [C p / parts, C (p + 1) / parts), each a double-mask chain of its own over the same elements (a cut costs one PRF
 * stream: C + parts streams instead of C + 1).  Every piece writes the sum of its own ciphertexts and its own decrypt mask
 * term(b_p) - term(a_p) to scratch; the sums add up and the masks telescope (b_p = a_{p+1}), so ONE short memory-bound combine pass
 * gives sum_out_dev and dmask_dev: two launches whatever C is, no integer plaintext in HBM, every output bit for bit what the uncut
 * launch (or C flashe_quantize_encrypt_tensors_dev calls and flashe_aggregate_elem_dev) writes.
 * flashe_cohort_cut_parts: *parts = the pieces the launch will use for n_clients clients and n values -- as many as fill the chip once
 * (the largest count whose items do not outnumber its 16 x flashe_ctx_cu_count waves; an item: 128 elements at int_bits > 64, 128 AES
 * blocks in the compact layout), never fewer than four clients per piece, at most 16 pieces; 1 (one launch, no combine, no scratch)
 * from half an item per wave upward.  compact != 0: the rule of the _u32 entry
 * point (n_jobs counts its AES blocks; ignored otherwise).  FLASHE_ENOTSUP (*parts = 0) where the launch itself would decline. */
int flashe_cohort_cut_parts(flashe_ctx *ctx, int n_clients, uint64_t n, uint32_t n_jobs, int compact, int *parts);
/* flashe_quantize_encrypt_cohort_dev for any n >= 1 (new), jzf_quantize.py:394-491, jzf_flashe.py:349-353, 480-481,
 * jzf_aggregator.py:424-430: its arguments, checks, stage pass and outputs, plus scratch_dev: caller-allocated, 16-byte aligned,
 * parts x n x 16 bytes for the pieces' sums and as much again when dmask_dev is given (parts from flashe_cohort_cut_parts); not
 * touched and may be NULL when parts == 1.  FLASHE_EINVAL: a scratch that is NULL with parts > 1, misaligned, or one of the outputs.
 * Returns FLASHE_ENOTSUP -- nothing launched -- for int_bits <= 64, more than 128 clients, n = 0 or n > 2^32, FLASHE_CHAIN=0, another
 * PRF backend.  The table uploads synchronise; not capturable. */
int flashe_quantize_encrypt_cohort_cut_dev(flashe_ctx *ctx, uint32_t iter, uint32_t first_idx, int n_clients, uint64_t n, uint32_t n_jobs,
                                           const flashe_tensor_layer *layers, int n_layers, const void *const *src_dev, const int32_t *src_dtype,
                                           int element_bits, const double *u_dev, uint64_t *const *ct_dev, uint64_t *sum_out_dev, uint64_t *dmask_dev,
                                           uint64_t *scratch_dev);
/* flashe_quantize_encrypt_cohort_u32_dev for any n >= 1 (new), jzf_quantize.py:394-491, jzf_flashe.py:349-353, 480-481,
 * jzf_aggregator.py:424-430: its arguments, checks, stage pass and outputs (uint32 ciphertexts and their uint32 sum at int_bits
 * 16 / 20 / 23 / 24 / 32, no decrypt mask), plus scratch_dev: caller-allocated, 16-byte aligned, parts x n x 4 bytes; not touched and
 * may be NULL when parts == 1.  FLASHE_EINVAL as above.  Returns FLASHE_ENOTSUP -- nothing launched -- for a ctx whose
 * flashe_ctx_compact_layout is 0, another int_bits, more than 128 clients, n = 0 or n >= 2^32.  Not capturable. */
int flashe_quantize_encrypt_cohort_cut_u32_dev(flashe_ctx *ctx, uint32_t iter, uint32_t first_idx, int n_clients, uint64_t n, uint32_t n_jobs,
                                               const flashe_tensor_layer *layers, int n_layers, const void *const *src_dev, const int32_t *src_dtype,
                                               int element_bits, const double *u_dev, uint32_t *const *ct_dev, uint32_t *sum_out_dev, uint32_t *scratch_dev);
/* The same cohort for a BATCHED job at int_bits > 64 (new), jzf_quantize.py:55-67, 162-185, jzf_flashe.py:349-353, jzf_aggregator.py:424-430:
 * ONE chained launch over the n_elems = sum_l ceil(size_l / bs) batched elements of the model (bs = int_bits / field_bits values per
 * element, every layer padded to whole elements on its own, the first value of an element in its most significant field).  It writes
 * ct_dev[c] (n_elems x 2 limbs: bit for bit flashe_quantize_batch_tensors_dev of client c with the draws u_dev[c * n_values ..], followed
 * by its double-mask flashe_encrypt_dev with cipher index first_idx + c), sum_out_dev = sum_c ct_dev[c] mod 2^b and, when dmask_dev is
 * not NULL, term(first_idx + n_clients) - term(first_idx) mod 2^b over the n_elems elements (feed it to
 * flashe_combine_unbatch_unquantize_model_dev).  No batched plaintext exists in HBM.  layers (sizes = the differences of consecutive
 * starts, the last one ends at n_values), src_dev, src_dtype, the stage pass and the argument checks are those of
 * flashe_quantize_encrypt_cohort_dev; FLASHE_EINVAL when n_elems is not what the layers batch into.
 * Returns FLASHE_ENOTSUP -- nothing launched -- for every shape outside the launch: int_bits <= 64, bs outside 5 .. 7 (the
 * batch sizes compiled in: what the reference's element_bits 16 jobs give at int_bits 120 / 128), more than 128 clients, fewer than two 256-element tiles per wave of the chip counted
 * in elements (2 x 16 x flashe_ctx_cu_count tiles), n_elems > 2^32, FLASHE_CHAIN=0, another PRF backend; the caller then runs
 * flashe_quantize_batch_tensors_dev per client and flashe_encrypt_batch_sum_dev.  The table uploads synchronise; not capturable. */
int flashe_quantize_batch_encrypt_cohort_dev(flashe_ctx *ctx, uint32_t iter, uint32_t first_idx, int n_clients, uint64_t n_values, uint64_t n_elems,
                                             uint32_t n_jobs, const flashe_tensor_layer *layers, int n_layers, const void *const *src_dev,
                                             const int32_t *src_dtype, int element_bits, int field_bits, const double *u_dev, uint64_t *const *ct_dev,
                                             uint64_t *sum_out_dev, uint64_t *dmask_dev);
/* The two chained launches above for a round in which clients DROPPED OUT (new), jzf_flashe.py:349-367, jzf_aggregator.py:424-430: idx =
 * the cipher indices of the n_clients clients that report, strictly ascending (P = {0,1,3,4} when client 2 of five misses the round);
 * everything indexed by client -- src_dev, src_dtype, the draws u_dev[c * n ..] and ct_dev -- counts the clients of idx, c = 0 ..
 * n_clients - 1.  The launch computes the streams S = { s : s in P or s - 1 in P }, |P| + runs of them instead of 2 |P| (a stream
 * strictly inside a dropped run of two or more clients is not computed), and writes ct_dev[c] (bit for bit
 * flashe_quantize_encrypt_tensors_dev with cipher index idx[c]), sum_out_dev = sum_c ct_dev[c] mod 2^b and, when dmask_dev is not NULL,
 * the decrypt mask of the telescoped lists, sum_r term(last index of run r + 1) - term(first index of run r) mod 2^b: what
 * flashe_decrypt_dev with flashe_telescope(idx) adds to the sum (feed it to flashe_combine_unquantize_model_dev).  One run of consecutive
 * indices launches exactly what flashe_quantize_encrypt_cohort_dev launches and writes its bytes.
 * FLASHE_EINVAL: idx NULL, not strictly ascending (unsorted, duplicates) or holding 2^32 - 1, and the argument errors of
 * flashe_quantize_encrypt_cohort_dev.  FLASHE_ENOTSUP -- nothing launched -- outside that function's admission with n_clients = |P|, and
 * when |P| + runs exceeds the 144 streams one launch holds (128 clients may form 16 runs); the caller then quantises per client and uses
 * flashe_encrypt_batch_sum_dev, which takes any indices.  The table uploads synchronise; not capturable. */
int flashe_quantize_encrypt_cohort_runs_dev(flashe_ctx *ctx, uint32_t iter, const uint32_t *idx, int n_clients, uint64_t n, uint32_t n_jobs,
                                            const flashe_tensor_layer *layers, int n_layers, const void *const *src_dev, const int32_t *src_dtype,
                                            int element_bits, const double *u_dev, uint64_t *const *ct_dev, uint64_t *sum_out_dev, uint64_t *dmask_dev);
/* The same for a BATCHED job at int_bits > 64 (new), jzf_quantize.py:162-185, jzf_flashe.py:349-367, jzf_aggregator.py:424-430:
 * flashe_quantize_batch_encrypt_cohort_dev with the cipher indices idx of the clients that report, under the rules of
 * flashe_quantize_encrypt_cohort_runs_dev (the length rule counted in the n_elems batched elements, bs = 5 .. 7; feed the mask to
 * flashe_combine_unbatch_unquantize_model_dev). */
int flashe_quantize_batch_encrypt_cohort_runs_dev(flashe_ctx *ctx, uint32_t iter, const uint32_t *idx, int n_clients, uint64_t n_values, uint64_t n_elems,
                                                  uint32_t n_jobs, const flashe_tensor_layer *layers, int n_layers, const void *const *src_dev,
                                                  const int32_t *src_dtype, int element_bits, int field_bits, const double *u_dev, uint64_t *const *ct_dev,
                                                  uint64_t *sum_out_dev, uint64_t *dmask_dev);
/* The compact cohort for a round in which clients DROPPED OUT (new), jzf_flashe.py:349-367, jzf_aggregator.py:424-430:
 * flashe_quantize_encrypt_cohort_u32_dev with the cipher indices idx of the n_clients clients that report, strictly ascending, in place
 * of first_idx; everything indexed by client counts the clients of idx, as in flashe_quantize_encrypt_cohort_runs_dev.  ONE chained launch
 * over the |P| + runs streams of S = { s : s in P or s - 1 in P } writes ct_dev[c] (uint32, n elements: the values of
 * flashe_quantize_encrypt_tensors_dev with cipher index idx[c]) and sum_out_dev = sum_c ct_dev[c] mod 2^b; no decrypt mask at these
 * widths -- decrypt the sum with flashe_telescope(idx).  One run of consecutive indices launches exactly what
 * flashe_quantize_encrypt_cohort_u32_dev launches and writes its bytes.
 * FLASHE_EINVAL: idx NULL, not strictly ascending (unsorted, duplicates) or holding 2^32 - 1, n_jobs = 0, and the argument errors of
 * flashe_quantize_encrypt_cohort_u32_dev.  FLASHE_ENOTSUP -- nothing launched, every output untouched -- outside that function's
 * admission with n_clients = |P|, and when |P| + runs exceeds the 144 streams one launch holds; the caller then quantises per client and
 * uses flashe_encrypt_batch_sum_u32_dev, which takes any indices.  The table uploads synchronise; not capturable. */
int flashe_quantize_encrypt_cohort_runs_u32_dev(flashe_ctx *ctx, uint32_t iter, const uint32_t *idx, int n_clients, uint64_t n, uint32_t n_jobs,
                                                const flashe_tensor_layer *layers, int n_layers, const void *const *src_dev, const int32_t *src_dtype,
                                                int element_bits, const double *u_dev, uint32_t *const *ct_dev, uint32_t *sum_out_dev);
/* The one-limb cohort for a round in which clients DROPPED OUT (new), jzf_flashe.py:349-367, jzf_aggregator.py:424-430:
 * flashe_quantize_encrypt_cohort_u64_dev with the cipher indices idx of the n_clients clients that report, strictly ascending, in place
 * of first_idx; everything indexed by client counts the clients of idx, as in flashe_quantize_encrypt_cohort_runs_dev.  ONE chained launch
 * over the |P| + runs streams of S = { s : s in P or s - 1 in P } writes ct_dev[c] (uint64, n elements, 8-byte aligned: the values of
 * flashe_quantize_encrypt_tensors_dev with cipher index idx[c]) and sum_out_dev = sum_c ct_dev[c] mod 2^b; no decrypt mask at these
 * widths -- decrypt the sum with flashe_telescope(idx).  One run of consecutive indices launches exactly what
 * flashe_quantize_encrypt_cohort_u64_dev launches and writes its bytes.
 * FLASHE_EINVAL: idx NULL, not strictly ascending (unsorted, duplicates) or holding 2^32 - 1, and the argument errors of
 * flashe_quantize_encrypt_cohort_u64_dev.  FLASHE_ENOTSUP -- nothing launched, every output untouched -- outside that function's
 * admission with n_clients = |P| (int_bits 33 .. 64, the length rule), and when |P| + runs exceeds the 144 streams one launch holds; the
 * caller then quantises per client and uses flashe_encrypt_batch_sum_dev, which takes any indices.  The table uploads synchronise; not
 * capturable. */
int flashe_quantize_encrypt_cohort_runs_u64_dev(flashe_ctx *ctx, uint32_t iter, const uint32_t *idx, int n_clients, uint64_t n, uint32_t n_jobs,
                                                const flashe_tensor_layer *layers, int n_layers, const void *const *src_dev, const int32_t *src_dtype,
                                                int element_bits, const double *u_dev, uint64_t *const *ct_dev, uint64_t *sum_out_dev);
/* A SHORT cohort in which clients DROPPED OUT, and a short BATCHED cohort (new), jzf_flashe.py:349-367, jzf_aggregator.py:424-430: a gap in
 * the cipher indices is a cut the round imposes -- a run of consecutive present clients a .. b is by itself a chain over streams
 * a .. b + 1 --, and the pieces' masks term(b_p + 1) - term(a_p) add up to the decrypt mask of the telescoped lists whether the cuts come
 * from gaps or from the rule of flashe_cohort_cut_parts.  So the cut launches take any strictly ascending idx in at most 16 runs.
 * flashe_cohort_cut_pieces: *parts = the pieces the launches below will use for the n_clients clients of idx and n ELEMENTS (a batched
 * job passes n_elems), and, when begins is not NULL, begins[0 .. *parts] = the position in idx of every piece's first client
 * (begins[*parts] = n_clients; room for 17 entries).  Every run starts as one piece; while they number fewer than
 * max(runs, flashe_cohort_cut_parts' count) the run with the most clients per piece takes one more, as long as its pieces keep four
 * clients; inside a run the pieces are even.  One run: flashe_cohort_cut_parts' pieces.  A gapped cohort always has parts >= 2.
 * FLASHE_EINVAL: idx NULL, not strictly ascending or holding 2^32 - 1, n_clients < 1, compact with n_jobs = 0.  FLASHE_ENOTSUP
 * (*parts = 0) where the launch would decline: flashe_cohort_cut_parts' cases and more than 16 runs. */
int flashe_cohort_cut_pieces(flashe_ctx *ctx, const uint32_t *idx, int n_clients, uint64_t n, uint32_t n_jobs, int compact, int *parts, int *begins);
/* flashe_quantize_encrypt_cohort_cut_dev with the cipher indices idx of the n_clients clients that report in place of first_idx (new),
 * jzf_quantize.py:394-491, jzf_flashe.py:349-367, jzf_aggregator.py:424-430: everything indexed by client counts the clients of idx, as
 * in flashe_quantize_encrypt_cohort_runs_dev, whose outputs it writes -- ct_dev[c], their sum and, with dmask_dev, the decrypt mask of the
 * telescoped lists -- for any n >= 1.  scratch_dev: parts x n x 16 bytes and as much again when dmask_dev is given, parts from
 * flashe_cohort_cut_pieces.  One run launches what flashe_quantize_encrypt_cohort_cut_dev launches and writes its bytes.
 * FLASHE_EINVAL: a bad idx (as above), a bad scratch, and that function's argument errors.  FLASHE_ENOTSUP -- nothing launched, every
 * output untouched -- outside its admission and for more than 16 runs.  Not capturable. */
int flashe_quantize_encrypt_cohort_cut_runs_dev(flashe_ctx *ctx, uint32_t iter, const uint32_t *idx, int n_clients, uint64_t n, uint32_t n_jobs,
                                                const flashe_tensor_layer *layers, int n_layers, const void *const *src_dev, const int32_t *src_dtype,
                                                int element_bits, const double *u_dev, uint64_t *const *ct_dev, uint64_t *sum_out_dev,
                                                uint64_t *dmask_dev, uint64_t *scratch_dev);
/* The same for the compact layout (new), jzf_quantize.py:394-491, jzf_flashe.py:349-367, jzf_aggregator.py:424-430:
 * flashe_quantize_encrypt_cohort_cut_u32_dev with idx in place of first_idx; scratch_dev: parts x n x 4 bytes, parts from
 * flashe_cohort_cut_pieces(compact = 1).  No mask is kept: decrypt the sum with flashe_telescope(idx). */
int flashe_quantize_encrypt_cohort_cut_runs_u32_dev(flashe_ctx *ctx, uint32_t iter, const uint32_t *idx, int n_clients, uint64_t n, uint32_t n_jobs,
                                                    const flashe_tensor_layer *layers, int n_layers, const void *const *src_dev,
                                                    const int32_t *src_dtype, int element_bits, const double *u_dev, uint32_t *const *ct_dev,
                                                    uint32_t *sum_out_dev, uint32_t *scratch_dev);
/* The BATCHED cohort at int_bits > 64 for any n_elems >= 1 (new), jzf_quantize.py:162-185, jzf_flashe.py:349-367, jzf_aggregator.py:424-430:
 * flashe_quantize_batch_encrypt_cohort_runs_dev's arguments, checks and outputs without its length rule (bs = 5 .. 7; one run or several,
 * at most 16), the chain cut into the pieces of flashe_cohort_cut_pieces(ctx, idx, n_clients, n_elems, ...) over the batched elements;
 * scratch_dev: parts x n_elems x 16 bytes and as much again when dmask_dev is given (feed the mask to
 * flashe_combine_unbatch_unquantize_model_dev).  FLASHE_EINVAL / FLASHE_ENOTSUP as above.  Not capturable. */
int flashe_quantize_batch_encrypt_cohort_cut_runs_dev(flashe_ctx *ctx, uint32_t iter, const uint32_t *idx, int n_clients, uint64_t n_values,
                                                      uint64_t n_elems, uint32_t n_jobs, const flashe_tensor_layer *layers, int n_layers,
                                                      const void *const *src_dev, const int32_t *src_dtype, int element_bits, int field_bits,
                                                      const double *u_dev, uint64_t *const *ct_dev, uint64_t *sum_out_dev, uint64_t *dmask_dev,
                                                      uint64_t *scratch_dev);
/* A precompute job's cohort (new), jzf_flashe.py:599-631, 456-488: every client computes its next round's encrypt mask in idle time and
 * its online step is a quantise plus a mask add.  For a cohort the masks are ONE chain of n_clients + 1 streams into vectors the caller
 * owns, mask[c][j] = term(iter, first_idx + c)[j] - term(iter, first_idx + c + 1)[j] mod 2^b: in the limb layout
 * flashe_prf_jobs_dev with n_clients linked jobs (in_dev = NULL, minus_idx[e] = add_idx[e + 1]); in the compact layout
 * flashe_cohort_masks_u32_dev (uint32 vectors of n elements, 4-byte aligned; check_u32's conditions -- FLASHE_EINVAL at int_bits > 32,
 * n >= 2^32, n_jobs = 0, another PRF backend or FLASHE_CHAIN=0 --, every int_bits <= 32, up to 128 vectors per launch).  The ctx's own
 * precompute caches (flashe_prepare_*, flashe_prepared_query / _discard) are not touched. */
int flashe_cohort_masks_u32_dev(flashe_ctx *ctx, uint32_t iter, uint32_t first_idx, int n_clients, uint64_t n, uint32_t n_jobs,
                                uint32_t *const *mask_dev);
/* The cohort's ONLINE step with those masks (new): ONE memory-bound pass, no AES, writes
 *   ct_dev[c][k] = (quantize(x_c[k], u_dev[c * n + k]) + mask_dev[c][k]) mod 2^b   and   sum_out_dev[k] = sum_c ct_dev[c][k] mod 2^b
 * for the n values of every client (n x L limbs per vector); with the chain's masks ct_dev[c] is bit for bit the double-mask
 * flashe_quantize_encrypt_tensors_dev of client c.  No integer plaintext exists in HBM.  layers, src_dev, src_dtype, LOOP_F64 / SHIFT /
 * SHIFT_WIDE, the stage pass for sources not in their row's compute type and the argument checks are those of
 * flashe_quantize_encrypt_cohort_dev (a float64 source under a float32 row, a misaligned or missing vector: FLASHE_EINVAL).  Any
 * int_bits, any n (n = 0: FLASHE_OK, nothing launched), any n_clients >= 1 in one launch (the vector pointers travel in a device
 * table).  sum_out_dev may be NULL; it must not be a mask, a ciphertext or a source (FLASHE_EINVAL).  mask_dev[c] and ct_dev[c] of
 * different clients must not overlap.  The table uploads synchronise; not capturable. */
int flashe_quantize_combine_cohort_dev(flashe_ctx *ctx, int n_clients, uint64_t n, const flashe_tensor_layer *layers, int n_layers,
                                       const void *const *src_dev, const int32_t *src_dtype, int element_bits, const double *u_dev,
                                       const uint64_t *const *mask_dev, uint64_t *const *ct_dev, uint64_t *sum_out_dev);
/* The same in the compact layout (new): uint32 masks, ciphertexts and sum (4-byte aligned) at ANY int_bits <= 32 -- there is no AES
 * here, so the widths compiled into the compact chains do not matter.  FLASHE_EINVAL at int_bits > 32; FLASHE_ENOTSUP -- nothing
 * launched -- on a ctx whose flashe_ctx_compact_layout is 0. */
int flashe_quantize_combine_cohort_u32_dev(flashe_ctx *ctx, int n_clients, uint64_t n, const flashe_tensor_layer *layers, int n_layers,
                                           const void *const *src_dev, const int32_t *src_dtype, int element_bits, const double *u_dev,
                                           const uint32_t *const *mask_dev, uint32_t *const *ct_dev, uint32_t *sum_out_dev);
/* The same for a BATCHED job (new) over its n_elems = sum_l ceil(size_l / bs) elements, bs = int_bits / field_bits >= 1 (any: the
 * 5 / 6 / 7 of the chained launch does not apply; those three read whole elements in 16-byte runs): client c's plaintext of element e
 * is flashe_quantize_batch_tensors_dev's with the draws u_dev[c * n_values + value index].  FLASHE_EINVAL when n_elems is not what the
 * layers batch into. */
int flashe_quantize_batch_combine_cohort_dev(flashe_ctx *ctx, int n_clients, uint64_t n_values, uint64_t n_elems, const flashe_tensor_layer *layers,
                                             int n_layers, const void *const *src_dev, const int32_t *src_dtype, int element_bits, int field_bits,
                                             const double *u_dev, const uint64_t *const *mask_dev, uint64_t *const *ct_dev, uint64_t *sum_out_dev);
struct flashe_philox_segment;                   /* (defined with flashe_philox_random_dev below) */
/* The un-batched online step with the draws of np.random.Philox streams generated INSIDE the launch (new): the arguments of
 * flashe_quantize_combine_cohort_dev / _u32_dev with u_dev replaced by a segment table of flashe_philox_random_dev's type and meaning
 * (declared below) -- segment s gives n draws of its generator state to the client-major draw positions [offset, offset + n), client c
 * rounding its value k with draw c * n + k.  One segment covers all clients of a shared generator, one segment per client a list of
 * generators.  No draw buffer exists: a lane's four values are one Philox4x64 block of its client's stream, so the launch moves 16 bytes
 * less per value and client than flashe_philox_random_dev + flashe_quantize_combine_cohort_dev, whose ciphertexts and sum it reproduces bit
 * for bit.  The non-empty segments must tile [0, n_clients * n) exactly, and every client's n draws must lie in one segment;
 * FLASHE_EINVAL otherwise, for everything flashe_philox_random_dev refuses in a table (a buffer_pos above 4, more than 128 segments,
 * overflowing or overlapping ranges, a graph being captured) and for everything flashe_quantize_combine_cohort_dev / _u32_dev refuse;
 * FLASHE_ENOTSUP as there.  On success every segment is advanced in place as flashe_philox_random_dev advances it; on any refusal
 * nothing is advanced, staged or launched.  n = 0 (every segment empty): FLASHE_OK, nothing launched or advanced.  The batched
 * job's form is flashe_quantize_batch_combine_cohort_philox_dev below. */
int flashe_quantize_combine_cohort_philox_dev(flashe_ctx *ctx, int n_clients, uint64_t n, const flashe_tensor_layer *layers, int n_layers,
                                              const void *const *src_dev, const int32_t *src_dtype, int element_bits,
                                              struct flashe_philox_segment *segments, int n_segments, const uint64_t *const *mask_dev,
                                              uint64_t *const *ct_dev, uint64_t *sum_out_dev);
int flashe_quantize_combine_cohort_philox_u32_dev(flashe_ctx *ctx, int n_clients, uint64_t n, const flashe_tensor_layer *layers, int n_layers,
                                                  const void *const *src_dev, const int32_t *src_dtype, int element_bits,
                                                  struct flashe_philox_segment *segments, int n_segments, const uint32_t *const *mask_dev,
                                                  uint32_t *const *ct_dev, uint32_t *sum_out_dev);
/* The BATCHED online step with the draws generated inside the launch (new): flashe_quantize_batch_combine_cohort_dev's arguments and
 * refusals with u_dev replaced by a segment table under flashe_quantize_combine_cohort_philox_dev's rules over the clients' VALUES --
 * client c rounds its flat value k (the layers' values in order; an element's pads draw nothing) with draw c * n_values + k, the
 * non-empty segments tile [0, n_clients * n_values) exactly (a table that tiles n_clients * n_elems is refused) and every client lies
 * in one segment.  A lane owns four consecutive elements of one layer and computes each Philox4x64 block their 4 bs values are words
 * of once: bs blocks where the client's stream is block-aligned at the layer's first value, bs + 1 where it is not (bs 5 / 6 / 7
 * compiled in; every other bs, a layer's last elements and elements with pads keep the current block and compute a new one when its
 * words run out).  No draw buffer exists: per element and client at bs 6 the launch moves 56 bytes where flashe_philox_random_dev +
 * flashe_quantize_batch_combine_cohort_dev move 152, and it reproduces their ciphertexts and sum bit for bit.  On success every
 * segment is advanced in place; on any refusal nothing is advanced, staged or launched.  n_values = 0: FLASHE_OK.  Not capturable. */
int flashe_quantize_batch_combine_cohort_philox_dev(flashe_ctx *ctx, int n_clients, uint64_t n_values, uint64_t n_elems,
                                                    const flashe_tensor_layer *layers, int n_layers, const void *const *src_dev,
                                                    const int32_t *src_dtype, int element_bits, int field_bits,
                                                    struct flashe_philox_segment *segments, int n_segments, const uint64_t *const *mask_dev,
                                                    uint64_t *const *ct_dev, uint64_t *sum_out_dev);
/* The codec back end over caller-held vectors (new), jzf_quantize.py:102-107: out[k] = unquantize((in[k] + add[k] - minus[k]) mod 2^b)
 * as float64 for the n elements of a flattened model, one memory-bound pass; add_dev / minus_dev may be NULL (zeros).  With in = a
 * cohort's sum and add = its decrypt mask this is the cohort's decrypt_unquantize. */
int flashe_combine_unquantize_model_dev(flashe_ctx *ctx, uint64_t n, const uint64_t *in_dev, const uint64_t *add_dev, const uint64_t *minus_dev,
                                        const flashe_codec_layer *layers, int n_layers, int element_bits, int num_clients, double *out_dev);
/* Its batched sibling (new), jzf_quantize.py:102-107, 240-246: flashe_unbatch_unquantize_model_dev over (in + add - minus) mod 2^b, one
 * memory-bound pass over the n_elems batched elements; add_dev / minus_dev may be NULL (zeros).  With in = a batched cohort's sum and
 * add = its decrypt mask this is the cohort's decrypt_unquantize. */
int flashe_combine_unbatch_unquantize_model_dev(flashe_ctx *ctx, const flashe_batch_layer *layers, int n_layers, int element_bits, int field_bits,
                                                int num_clients, const uint64_t *in_dev, const uint64_t *add_dev, const uint64_t *minus_dev,
                                                uint64_t n_elems, double *out_dev);
/* The batched job's front end, jzf_quantize.py:55-67, 162-185 (new): flashe_quantize_batch_model_dev with tensor layers; the layer
 * sizes are the differences of consecutive starts, the last one ends at n_values. */
int flashe_quantize_batch_tensors_dev(flashe_ctx *ctx, const flashe_tensor_layer *layers, int n_layers, uint64_t n_values, int element_bits,
                                      int field_bits, const double *u_dev, uint64_t n_elems, uint64_t *out_dev);
/* Back end, jzf_quantize.py:102-107, 549-564 (unnormalize): the flat float64 vector in_dev[n] (what flashe_decrypt_unquantize_model_dev /
 * flashe_unbatch_unquantize_model_dev / flashe_unquantize_model_dev write) goes into the layers' tensors: y = in (+ shift with SHIFT) in
 * float64, stored as the layer's dtype (float64 -> float32 -> 16 bits, each step round to nearest even).  ptr may be the layer's own
 * place in in_dev (in place).  stats_dev (device, 2 doubles per layer; NULL = none): (sum, sum of squared deviations) of y of every
 * non-empty layer exactly as NumPy sums a C-contiguous float64 array -- buffers of `block` values (np.getbufsize(), <= 16,384) added in
 * order to 0.0, each by NumPy's pairwise tree -- so that the caller's S / n and sqrt(S2 / n) ARE np.mean and np.std of y, bit for bit
 * (the deviations are taken from the correctly rounded S / n).  The table upload synchronises; the passes are asynchronous. */
int flashe_store_layers_dev(flashe_ctx *ctx, const double *in_dev, uint64_t n, const flashe_tensor_layer *layers, int n_layers, uint64_t block,
                            double *stats_dev);
/* The rows and flags of flashe_stage_layers_dev (new). */
#define FLASHE_STAGE_SCALE 1
#define FLASHE_STAGE_SCALE_WIDE 2
#define FLASHE_STAGE_SHIFT 4
#define FLASHE_STAGE_SHIFT_WIDE 8
#define FLASHE_STAGE_OUT_F64 16
typedef struct flashe_stage_row {
    const void *src;       /* the layer's values as stored */
    void *dst;             /* size float32 values, or float64 values with OUT_F64 */
    uint64_t size;
    double scale;          /* with SCALE: the degree */
    double shift;          /* with SHIFT: -mean */
    int32_t src_dtype;     /* F32 0, F64 1, F16 2, BF16 3 */
    int32_t flags;
} flashe_stage_row;
/* The aggregator's degree scaling in front of the step (new), jzf_aggregator.py:676 (`weights *= degree`, a client's model weighted by its
 * sample count) followed by jzf_quantize.py:542-547 (normalize): ONE streaming pass over n_rows rows (HOST array), each `size` values from
 * src (stored as src_dtype, FLASHE_TENSOR_*) to dst, a buffer of the caller's -- the rows of one model, or the C x L layers of a cohort
 * with a scale per client.  Per value, in the type NumPy gives the layer at each step: a 16-bit value is upcast to float32 exactly;
 * FLASHE_STAGE_SCALE multiplies by `scale` -- a float64 value in float64, a float32 value by (float)scale in float32 (a Python number,
 * an np.float32) or, with FLASHE_STAGE_SCALE_WIDE (an np.float64 degree), as (double)x * scale, the value being float64 from there on;
 * FLASHE_STAGE_SHIFT adds `shift` to whatever the value now is, FLASHE_STAGE_SHIFT_WIDE as FLASHE_TENSOR_SHIFT_WIDE on a float32 value;
 * the store is float32, or float64 with FLASHE_STAGE_OUT_F64 (an exact widening of a float32 value).  Nothing is contracted into an FMA.
 * Without SCALE the bytes are those of the stage pass of flashe_quantize_encrypt_tensors_dev.  dst then goes to the *_tensors_dev /
 * *_cohort_dev entry points as a plain F32 / F64 layer without SHIFT.
 * FLASHE_EINVAL before anything is launched: a null or misaligned pointer (to the element size) of a non-empty row, an unknown dtype or
 * flag, SCALE_WIDE without SCALE, SHIFT_WIDE without SHIFT, a WIDE flag on a float64 source or SHIFT_WIDE behind SCALE_WIDE (the value
 * is float64 already), SCALE_WIDE or a float64 source without OUT_F64, a scale that is zero or not finite, a shift that is not finite,
 * a call inside a graph capture.  The table upload synchronises; the pass is asynchronous. */
int flashe_stage_layers_dev(flashe_ctx *ctx, const flashe_stage_row *rows, int n_rows);
/* The rows and flags of flashe_finish_layers_dev (new). */
#define FLASHE_FINISH_DIV_TOTAL 1
#define FLASHE_FINISH_SHIFT 2
#define FLASHE_FINISH_DIV_OWN 4
#define FLASHE_FINISH_ADD_LAST 8
typedef struct flashe_finish_row {
    uint64_t start;        /* flat index of the row's first value */
    void *dst;
    const void *last;      /* with ADD_LAST */
    double div_total, shift, div_own;
    int32_t dst_dtype, last_dtype;   /* F32 0, F64 1, F16 2, BF16 3 */
    int32_t flags;
    int32_t reserved;      /* 0 */
} flashe_finish_row;
/* The aggregator's degree scaling behind the step (new), jzf_aggregator.py:902-907 around jzf_quantize.py:549-564 (unnormalize):
 * flashe_store_layers_dev with the two divisions and the last round's model.  Row r (HOST array, ascending start, the last row ends at n)
 * holds flat values [start, next start) of in_dev; per value, in float64 and under the row's flags,
 *   y1 = in / div_total   (FLASHE_FINISH_DIV_TOTAL; :902, div_total = degrees / self.degree computed by the caller as the reference does)
 *   y2 = y1 + shift       (FLASHE_FINISH_SHIFT;     :904, unnormalize's += mean)
 *   y3 = y2 / div_own     (FLASHE_FINISH_DIV_OWN;   :905)
 *   y4 = (double)last[k] + y3   (FLASHE_FINISH_ADD_LAST; :907, last stored as last_dtype and upcast exactly)
 * stored in dst as dst_dtype (float64 -> float32 -> 16 bits, round to nearest even).  Both divisions are correctly rounded divisions,
 * neither merged nor turned into a multiplication, and nothing is contracted into an FMA.  stats_dev / block: as flashe_store_layers_dev,
 * over y2 (what unnormalize records, :904) and per row index.  last == dst with equal dtypes updates the model in place.  With no
 * flag but SHIFT the bytes are flashe_store_layers_dev's.
 * FLASHE_EINVAL before anything is launched: a null or misaligned in_dev / stats_dev, a null or misaligned dst (or last with ADD_LAST)
 * of a non-empty row, an unknown dtype or flag, a non-zero reserved field, a divisor that is zero or not finite, a shift that is not
 * finite, starts that do not ascend from 0 or leave n, a `last` that overlaps any row's dst other than as its own row's dst with the
 * same dtype, a block outside [1, 16384] with stats_dev, a call inside a graph capture.  The table uploads synchronise. */
int flashe_finish_layers_dev(flashe_ctx *ctx, const double *in_dev, uint64_t n, const flashe_finish_row *rows, int n_rows, uint64_t block,
                             double *stats_dev);

/* The model-wide codec with the ctx's PRECOMPUTED masks (new): the client step of a job with precompute enabled (jzf_flashe.py:456-488,
 * :537-582 once prepare_encrypt / prepare_decrypt, :599-666, filled the caches) -- the codec of the calls above and the combine of
 * flashe_encrypt_prepared_dev / flashe_decrypt_prepared_dev in one pass, no AES:
 *   quantize_encrypt_prepared_{model,tensors}: ct[k] = (quantize(x[k], u[k]) + add[k] - minus[k]) mod 2^b for the elements
 *       [first, first + count) of the n-element flattened model (flashe_quantize_encrypt_{model,tensors}_dev's tables and pointers);
 *   quantize_batch_encrypt_prepared_{model,tensors}: ct[e] = (batched[e] + add[e] - minus[e]) mod 2^b over the whole batched vector
 *       (flashe_quantize_batch_{model,tensors}_dev's walk; n_elems elements);
 *   decrypt_prepared_unquantize_model: out[k] = unquantize((in[k] + add[k] - minus[k]) mod 2^b) as float64, k < n;
 *   decrypt_prepared_unbatch_unquantize_model: flashe_unbatch_unquantize_model_dev's walk over (in + add - minus) mod 2^b.
 * The decrypt forms take the extra add / minus prefixes of flashe_decrypt_prepared_dev (the dropouts set_idx_list leaves uncovered, merged
 * in online, :557-564): then a PRF launch writes in + extras into ctx scratch first and the codec pass reads that (two launches).
 * Cache rules (those of flashe_encrypt_prepared_dev / flashe_decrypt_prepared_dev): FLASHE_EINVAL without a valid cache of the direction,
 * and FLASHE_EINVAL with the cache left valid when the vector's length (n, n_elems) differs from the cached one; the cache is consumed once
 * per WHOLE vector -- an un-batched encrypt may come as several range calls over [first, first + count), and the call whose range ends
 * at n consumes it (a call that fails, or a range that ends before n, leaves it valid).  A decrypt never touches the encrypt cache, an
 * encrypt never the decrypt cache.  The masks' iteration is not checked (the reference uses whatever it prepared).  Not capturable
 * into a graph (the tables are staged per call). */
int flashe_quantize_encrypt_prepared_model_dev(flashe_ctx *ctx, uint64_t n, uint64_t first, uint64_t count, const flashe_codec_layer *layers,
                                               int n_layers, int element_bits, const double *u_dev, uint64_t *ct_dev);
int flashe_quantize_encrypt_prepared_tensors_dev(flashe_ctx *ctx, uint64_t n, uint64_t first, uint64_t count, const flashe_tensor_layer *layers,
                                                 int n_layers, int element_bits, const double *u_dev, uint64_t *ct_dev);
int flashe_quantize_batch_encrypt_prepared_model_dev(flashe_ctx *ctx, const flashe_batch_layer *layers, int n_layers, int element_bits, int field_bits,
                                                     const double *u_dev, uint64_t n_elems, uint64_t *ct_dev);
int flashe_quantize_batch_encrypt_prepared_tensors_dev(flashe_ctx *ctx, const flashe_tensor_layer *layers, int n_layers, uint64_t n_values,
                                                       int element_bits, int field_bits, const double *u_dev, uint64_t n_elems, uint64_t *ct_dev);
int flashe_decrypt_prepared_unquantize_model_dev(flashe_ctx *ctx, uint32_t iter, const uint32_t *add_idx, int n_add, const uint32_t *minus_idx,
                                                 int n_minus, uint64_t n, uint32_t n_jobs, const uint64_t *in_dev, const flashe_codec_layer *layers,
                                                 int n_layers, int element_bits, int num_clients, double *out_dev);
int flashe_decrypt_prepared_unbatch_unquantize_model_dev(flashe_ctx *ctx, uint32_t iter, const uint32_t *add_idx, int n_add, const uint32_t *minus_idx,
                                                         int n_minus, uint32_t n_jobs, const flashe_batch_layer *layers, int n_layers, int element_bits,
                                                         int field_bits, int num_clients, const uint64_t *in_dev, uint64_t n_elems, double *out_dev);

/* np.random.random(n) ON THE DEVICE, bit for bit (new): the stochastic-rounding draws of _static_quantize_padding_asymmetric
 * (jzf_quantize.py:61, `np.random.random(value.shape)`) come from NumPy's global MT19937 generator; this writes the same n doubles
 * to u_dev -- mt19937_next_double: a = next >> 5, b = next >> 6, (a * 2^26 + b) / 2^53 -- from the generator state the caller hands
 * in (key[624] and pos exactly as np.random.get_state() returns them, HOST memory) and advances that state in place as NumPy would,
 * so that the caller can put it back (np.random.set_state) and host draws continue the same stream.  The stream is cut into
 * substreams of 65,536 doubles whose starting states are found by jump-ahead (the recurrence is linear over GF(2)); they run in
 * parallel, one workgroup each: 1e7 doubles in 0.5 ms (np.random.random: 27-35 ms on a host core), and no 8 B/element upload.
 * Synchronous.  FLASHE_MT_PARALLEL=0 keeps the one-workgroup walk. */
int flashe_mt19937_random_dev(flashe_ctx *ctx, uint32_t key[624], uint32_t *pos, uint64_t n, double *u_dev);
/* Host only: builds the twelve jump polynomials x^(2^17 2^j) mod phi and checks the first against the generator itself. */
int flashe_mt19937_jump_selfcheck(void);
/* Host only: the pass plan of flashe_mt19937_random_dev for n draws from stream position pos -- the largest number of substreams any
 * pass is cut into, the number the jump tables can start (a pass must never exceed it), and the number of passes. */
int flashe_mt19937_plan(uint32_t pos, uint64_t n, uint32_t *max_substreams, uint32_t *substreams_available, uint32_t *passes);

/* Generator(np.random.Philox(...)).random(n) ON THE DEVICE, bit for bit (new): the stochastic-rounding draws of a caller's OWN generator
 * (rng=).  Philox4x64-10 is counter based -- block(counter[4], key[2]) -> four 64-bit words, ten rounds with the multipliers
 * 0xD2E7470EE14C6C93 / 0xCA5A826395121157 and the key bumped by 0x9E3779B97F4A7C15 / 0xBB67AE8584CAA73B before rounds 2 .. 10 -- and NumPy
 * increments the 256-bit counter (four little-endian words, wrapping at 2^256) BEFORE it generates a block: a state (counter,
 * buffer_pos = p) next returns words p .. 3 of block(counter), then all of block(counter + 1), ...; p = 4 (a fresh or exhausted buffer)
 * starts at block(counter + 1); draw = (word >> 11) * 2^-53.  A segment is one generator state (key, counter, buffer_pos exactly as
 * Generator.bit_generator.state holds them; the buffered words are recomputed from the counter, `buffer` is only written) and the n draws it
 * gives to draws [offset, offset + n) of u_dev, which need only be 8-byte aligned; bytes outside the ranges are not written.  ONE launch on
 * the ctx stream fills up to 128 segments (the clients of a cohort) and does not synchronise; every segment's state is advanced in place
 * on the host (counter, buffer_pos, buffer: what NumPy's own state is after n draws; n = 0 leaves it untouched), so the caller can put it
 * back into bit_generator.state and host draws continue the stream.  FLASHE_EINVAL: a buffer_pos above 4, more than 128 segments, an n or
 * offset + n above 2^60, overlapping output ranges, a misaligned u_dev, a graph being captured. */
typedef struct flashe_philox_segment {
    uint64_t key[2];
    uint64_t counter[4];
    uint64_t buffer[4];      /* out: the buffered words of the advanced state */
    uint32_t buffer_pos;     /* 0 .. 4 */
    uint32_t reserved;
    uint64_t n;              /* draws */
    uint64_t offset;         /* in draws into u_dev */
} flashe_philox_segment;
int flashe_philox_random_dev(flashe_ctx *ctx, flashe_philox_segment *segments, int n_segments, double *u_dev);
/* Host only (new): one Philox4x64-10 block as NumPy computes it -- words[4] = block(counter[4], key[2]). */
int flashe_philox_block(const uint64_t counter[4], const uint64_t key[2], uint64_t words[4]);
/* Host only (new): the state NumPy's Philox bit generator is in after Generator.random(n) from (counter, buffer_pos), in place: counter,
 * buffer_pos (1 .. 4) and the buffered words; n = 0 changes nothing. */
int flashe_philox_advance(const uint64_t key[2], uint64_t counter[4], uint32_t *buffer_pos, uint64_t buffer[4], uint64_t n);
/* Host only (new): the grid flashe_philox_random_dev launches for one segment of n draws from a state with that buffer_pos -- its tiles of
 * 256 blocks (1,024 draws) and its workgroups (at most 8 per compute unit the ctx may use; more tiles than that are further trips). */
int flashe_philox_grid(flashe_ctx *ctx, uint64_t n, uint32_t buffer_pos, uint32_t *workgroups, uint64_t *tiles);

/* Generator(np.random.PCG64(...)).random(n) and Generator(np.random.PCG64DXSM(...)).random(n) ON THE DEVICE, bit for bit (new): the draws
 * of the generator np.random.default_rng returns.  Both are the 128-bit LCG state' = A state + inc mod 2^128 with a 64-bit output function:
 * PCG64 (variant 0), A = 0x2360ED051FC65DA44385DF649FCCF645, steps first and outputs rotr64(hi ^ lo, state >> 122) of the NEW state;
 * PCG64DXSM (variant 1), A = 0xDA942042E4DD58B5, outputs from the OLD state (lo |= 1; hi ^= hi >> 32; hi *= A; hi ^= hi >> 48; hi *= lo)
 * and then steps; draw = (word >> 11) * 2^-53.  k steps are one affine map that does not depend on the generator, so a lane jumps once to
 * its first draw and walks a fixed stride.  A segment is one generator state (state and inc exactly as Generator.bit_generator.state holds
 * them, as two 64-bit words each, low word first; any 128-bit values, an even inc included) and the n draws it gives to draws
 * [offset, offset + n) of u_dev, which need only be 8-byte aligned; bytes outside the ranges are not written.  ONE launch per variant on
 * the ctx stream fills up to 128 segments (the clients of a cohort) and does not synchronise; every segment's state is advanced in place
 * on the host (what NumPy's own state is after n draws; has_uint32 / uinteger are no part of it: random() leaves them alone, and so must
 * the caller -- bit_generator.advance would reset them), so the caller can put it back into bit_generator.state and host draws continue the
 * stream.  FLASHE_EINVAL, and nothing advanced or written: a variant above 1, more than 128 segments, an n or offset + n above 2^60,
 * overlapping output ranges, a misaligned u_dev, a graph being captured. */
typedef struct flashe_pcg64_segment {
    uint64_t state[2];       /* in / out: low word, high word */
    uint64_t inc[2];
    uint32_t variant;        /* 0: PCG64, 1: PCG64DXSM */
    uint32_t reserved;
    uint64_t n;              /* draws */
    uint64_t offset;         /* in draws into u_dev */
} flashe_pcg64_segment;
int flashe_pcg64_random_dev(flashe_ctx *ctx, flashe_pcg64_segment *segments, int n_segments, double *u_dev);
/* Host only (new): the state (in place) of a PCG64 / PCG64DXSM bit generator n steps on -- n draws of Generator.random -- for any n below
 * 2^128 (two words, low first), by doubling: at most 128 rounds. */
int flashe_pcg64_advance(uint32_t variant, uint64_t state[2], const uint64_t inc[2], const uint64_t n[2]);
/* Host only (new): the grid flashe_pcg64_random_dev launches for one segment of n draws -- its tiles of *tile_draws (may be NULL) = 4,096
 * draws, 16 per lane at a stride of 256, and its workgroups (at most 8 per compute unit the ctx may use; more tiles than that are further
 * trips). */
int flashe_pcg64_grid(flashe_ctx *ctx, uint64_t n, uint32_t *workgroups, uint64_t *tiles, uint32_t *tile_draws);
/* A precompute cohort's un-batched online step with the draws of np.random.PCG64 / np.random.PCG64DXSM streams generated INSIDE the launch
 * (new): the arguments, results and refusals of flashe_quantize_combine_cohort_philox_dev / _u32_dev with a table of flashe_pcg64_segment
 * in place of the Philox one -- segment s gives n draws of its generator to the client-major draw positions [offset, offset + n), client c
 * rounding its value k with draw c * n + k; a stretch may start anywhere in its generator's stream.  No draw buffer exists.  A lane owns
 * runs of four values and keeps ONE jump (A^k, G_k) of the LCG for all clients -- over the 4 g steps to its run g, built once from tables
 * and composed with the grid's stride jump after every pass --; a client is a 32-byte plan (the state its first draw outputs from, and its
 * inc): two 128-bit low products apply the jump, three step on.  The ciphertexts and the sum are those of flashe_pcg64_random_dev +
 * flashe_quantize_combine_cohort_dev / _u32_dev bit for bit.  Refused with FLASHE_EINVAL, in this order: everything
 * flashe_pcg64_random_dev refuses in a table (a variant above 1, more than 128 segments, overflowing or overlapping ranges, a graph
 * being captured); non-empty segments that do not tile [0, n_clients * n) exactly, a client whose n draws lie in two segments, PCG64 and
 * PCG64DXSM segments in one table (the lane's jump is shared by the clients, so a launch has one variant); everything
 * flashe_quantize_combine_cohort_dev / _u32_dev refuse.  FLASHE_ENOTSUP as there.  On success every segment's state is advanced in
 * place on the host as flashe_pcg64_random_dev advances it -- nothing is read back, the call does not synchronise; on any refusal
 * nothing is advanced, staged or launched.  n = 0 (every segment empty): FLASHE_OK, nothing launched or advanced.  There is no batched
 * form. */
int flashe_quantize_combine_cohort_pcg64_dev(flashe_ctx *ctx, int n_clients, uint64_t n, const flashe_tensor_layer *layers, int n_layers,
                                             const void *const *src_dev, const int32_t *src_dtype, int element_bits,
                                             flashe_pcg64_segment *segments, int n_segments, const uint64_t *const *mask_dev,
                                             uint64_t *const *ct_dev, uint64_t *sum_out_dev);
int flashe_quantize_combine_cohort_pcg64_u32_dev(flashe_ctx *ctx, int n_clients, uint64_t n, const flashe_tensor_layer *layers, int n_layers,
                                                 const void *const *src_dev, const int32_t *src_dtype, int element_bits,
                                                 flashe_pcg64_segment *segments, int n_segments, const uint32_t *const *mask_dev,
                                                 uint32_t *const *ct_dev, uint32_t *sum_out_dev);
/* Host only (new): the workgroups of the grid flashe_quantize_combine_cohort_pcg64_dev / _u32_dev launch for n values per client (a lane
 * owns runs of four values; at most 8 workgroups of 256 lanes per compute unit the ctx may use: more runs than that are further passes). */
int flashe_pcg64_cohort_grid(flashe_ctx *ctx, uint64_t n, uint32_t *workgroups);
/* Host only (new): the draws the lane that owns run `run` (lane run % 256 of workgroup run / 256; run < 256 * workgroups) of that launch
 * on a grid of `workgroups` generates in its first `iterations` passes for a client whose stretch starts `first` draws into the generator
 * (variant, state, inc): out[4 p + i] = the draw of value 4 * (run + 256 * workgroups * p) + i of that client, through exactly the
 * functions the kernel compiles (the tables, the workgroup's and the lane's jump, the stride jump, apply and three steps) -- so that
 * the stride arithmetic can be compared with NumPy for grids and lengths no test launches.  out: 4 * iterations doubles. */
int flashe_pcg64_cohort_lane_draws(uint32_t variant, const uint64_t state[2], const uint64_t inc[2], uint64_t first, uint32_t workgroups,
                                   uint64_t run, uint64_t iterations, double *out);

/* _static_quantize_padding_asymmetric -- federatedml/secureprotol/jzf_quantize.py:55-67:
 * q = floor(clip(x, -alpha, alpha) + alpha) * (2^element_bits - 1) / (2 alpha) + u), with numpy's
 * dtype rules (x_is_f64 == 0: x is float32 and every step before "+ u" is a float32 operation).
 * u holds the stochastic-rounding draws in [0, 1) (the reference uses np.random.random). */
int flashe_quantize_dev(flashe_ctx *ctx, uint64_t n, const void *x_dev, int x_is_f64, double alpha,
                        int element_bits, const double *u_dev, uint64_t *q_dev);
int flashe_quantize(flashe_ctx *ctx, uint64_t n, const void *x, int x_is_f64, double alpha,
                    int element_bits, const double *u, uint64_t *q);
/* _static_unquantize_padding_asymmetric -- jzf_quantize.py:102-107:
 * out = v * (2 alpha C) / ((2^element_bits - 1) C) - alpha C in float64, v converted like a Python int
 * (correctly rounded).  v has v_limbs (1 or 2) limbs per element. */
int flashe_unquantize_dev(flashe_ctx *ctx, uint64_t n, const uint64_t *v_dev, int v_limbs, double alpha,
                          int element_bits, int num_clients, double *out_dev);
int flashe_unquantize(flashe_ctx *ctx, uint64_t n, const uint64_t *v, int v_limbs, double alpha,
                      int element_bits, int num_clients, double *out);
/* _static_batching_padding_asymmetric / _static_unbatching_padding_asymmetric -- jzf_quantize.py:162-185,
 * :234-251: batch_size = int_bits // field_bits values (uint64, zero-padded to a multiple) <-> one
 * int_bits-wide element, first value most significant; field_bits = element_bits + ceil(log2(num_clients)).
 * batch: out holds ceil(n / batch_size) elements; unbatch: out holds n_batches * batch_size values. */
int flashe_batch_dev(flashe_ctx *ctx, uint64_t n, const uint64_t *vals_dev, int field_bits, uint64_t *out_dev);
int flashe_batch(flashe_ctx *ctx, uint64_t n, const uint64_t *vals, int field_bits, uint64_t *out);
int flashe_unbatch_dev(flashe_ctx *ctx, uint64_t n_batches, const uint64_t *in_dev, int field_bits, uint64_t *out_dev);
int flashe_unbatch(flashe_ctx *ctx, uint64_t n_batches, const uint64_t *in, int field_bits, uint64_t *out);

/* ---- top-s% sparsifier of the client ------------------------------------ */
/* Client.sparsify for ONE layer -- federatedml/framework/homo/procedure/jzf_aggregator.py:578-623: the k entries
 * of largest |x| (ranked BEFORE the residual is added, as the reference does; ties at the k-th magnitude go to the
 * higher index) are emitted in ascending index order -- loc[k] and vals[k] = x + residual -- and the residual is
 * updated in place (selected positions 0, the others x + residual).  residual may be NULL (treated as zeros, not
 * written).  x / residual / vals are float32 (x_is_f64 == 0) or float64; n < 2^32; k <= n with
 * k = max(1, floor(sparsity * n)) in the reference.
 * A layer that keeps nothing (k == 0) only updates its residual: residual becomes x + residual, nothing is written to loc / vals.
 * That holds in every entry point below, whatever the other layers of the call keep -- also when NO layer keeps anything.  loc / vals
 * may be NULL exactly when the call keeps nothing in total (sum of k == 0); with no residual either, such a call does nothing. */
int flashe_sparsify_dev(flashe_ctx *ctx, uint64_t n, uint64_t k, const void *x_dev, int x_is_f64, void *residual_dev,
                        uint32_t *loc_dev, void *vals_dev);
int flashe_sparsify(flashe_ctx *ctx, uint64_t n, uint64_t k, const void *x, int x_is_f64, void *residual,
                    uint32_t *loc, void *vals);
/* Client.sparsify for EVERY layer of a model in one set of launches (new): layer l is elements [off_l, off_l + n[l]) of the flat
 * vectors x / residual (layers back to back, off_l = n[0] + ... + n[l-1]); its k[l] selected entries go to [koff_l, koff_l + k[l])
 * of the flat outputs loc / vals (koff_l = k[0] + ... + k[l-1]), locations relative to the layer, ascending -- layer by layer exactly
 * what flashe_sparsify gives (same tie rule).  n and k are HOST arrays; 12 (float32) / 20 (float64) launches per MODEL instead of per
 * layer (a ResNet-50 has 161 layers).  The _dev form synchronises the ctx stream once (layer table upload); not inside a graph capture. */
int flashe_sparsify_batch_dev(flashe_ctx *ctx, int n_layers, const uint64_t *n, const uint64_t *k, const void *x_dev, int x_is_f64,
                              void *residual_dev, uint32_t *loc_dev, void *vals_dev);
int flashe_sparsify_batch(flashe_ctx *ctx, int n_layers, const uint64_t *n, const uint64_t *k, const void *x, int x_is_f64,
                          void *residual, uint32_t *loc, void *vals);
/* Client.sparsify over a framework's own layers (new): flashe_sparsify_batch_dev's selection (same ranking and tie rule) on layers that
 * lie where their owner put them, in their own dtypes, with the outputs the sparse job sends.  layers: HOST table as for the tensor codec
 * (flashe_tensor_layer; ascending start, layers[0].start == 0, layer l holds dense elements [start_l, start_l+1), the last one ends at n;
 * ptr at any element-aligned address; alpha, shift and flags are ignored); k: HOST array of the entries each layer keeps (k_l <= n_l).
 * Compute type c_l: float64 for an F64 layer, float32 for F32, F16 and BF16 (16-bit values widened exactly); any mix in one call.
 *   residual_dev (engine-owned; NULL = zeros, not written): layer l's n_l values in c_l at byte offset R_l, R_0 = 0,
 *       R_l = align(R_{l-1} + n_{l-1} size(c_{l-1}), size(c_l)) -- for one compute type exactly flashe_sparsify_batch_dev's flat layout.
 *       Updated in place: 0 where an entry was kept, x + residual elsewhere (in c_l).
 *   vals_dev: layer l's k_l kept values x + residual (in c_l), ascending index, at byte offset V_l (the same rule on k).
 *   loc_dev: the K = sum k_l model-wide locations start_l + index, uint32, layer after layer (ascending across the model).
 *   packed_dev (NULL = none): `_to_bytes(loc, bits)` (jzf_aggregator.py:615-623) as ceil(K bits / 64) little-endian uint64 limbs -- what
 *       weights.to_big_int(loc, bits) returns; 1 <= bits <= 32, n <= 2^bits.
 * n < 2^32.  The tables are uploaded synchronously (not inside a graph capture); 14 launches for a float32-class model, 24 mixed. */
int flashe_sparsify_tensors_dev(flashe_ctx *ctx, uint64_t n, const flashe_tensor_layer *layers, int n_layers, const uint64_t *k, void *residual_dev,
                                uint32_t *loc_dev, void *vals_dev, uint64_t *packed_dev, int bits);
/* A cohort of sparse-job clients hosted on one device (new): Client.sparsify (jzf_aggregator.py:578-623) of C models of ONE shape in ONE
 * set of launches.  k_l = max(1, floor(sparsity * size_l)) depends on the shape only, so the clients share the layer table and differ in
 * where their values lie.  layers: the shared HOST table (start as above; dtype = the layer's COMPUTE class, FLASHE_TENSOR_F32 or
 * FLASHE_TENSOR_F64, the same for all clients; ptr, alpha, shift and flags ignored); src_dev / src_dtype: HOST arrays of n_clients x n_layers
 * entries, [c * n_layers + l] = client c's layer l and its storage dtype (F16 / BF16 under an F32 row are widened exactly).
 * Client c's residuals, values, locations and packed locations are block c of equal-stride buffers -- residual_dev + c residual_stride
 * bytes, vals_dev + c vals_stride bytes, loc_dev + c loc_stride entries, packed_dev + c packed_stride limbs -- each block laid out as
 * flashe_sparsify_tensors_dev lays out one model; byte strides are multiples of 8.  Results are, client by client, those of C
 * flashe_sparsify_tensors_dev calls.  The launch count does not depend on n_clients: 14 for a float32-class cohort, 24 mixed. */
int flashe_sparsify_cohort_tensors_dev(flashe_ctx *ctx, int n_clients, uint64_t n, const flashe_tensor_layer *layers, int n_layers, const uint64_t *k,
                                       const void *const *src_dev, const int32_t *src_dtype, void *residual_dev, uint64_t residual_stride,
                                       uint32_t *loc_dev, uint64_t loc_stride, void *vals_dev, uint64_t vals_stride, uint64_t *packed_dev,
                                       uint64_t packed_stride, int bits);
/* The codec front end of those clients' uploads in ONE launch (new): what QuantizingClient.quantize (jzf_quantize.py:433-465) makes of
 * the compact layers inside Client.secure_aggregate (jzf_aggregator.py:717-743), for all clients of the cohort.  layers: the shared
 * HOST table over the n compact values of one client (start, alpha, shift, flags as flashe_quantize_encrypt_tensors_dev reads them;
 * dtype = the COMPUTE class); src_dev / src_dtype as above (e.g. the values flashe_sparsify_cohort_tensors_dev left).  u_dev: the
 * draws, client c's value j takes u_dev[c * u_stride + j] and its trailing 'zzz' value the draw behind them, u_dev[c * u_stride + n]
 * (u_stride >= n + 1).  pt_dev[c] (HOST array of device pointers): client c's n plaintexts, ONE uint64 limb each -- what
 * flashe_sparse_encrypt_aggregate_dev reads with pt_limbs = 1.  zzz: HOST array of the clients' (normalised) 'zzz' values, quantised
 * with alpha 1.0 in float64 (zzz_is_f64) or float32 into zeros_dev[c] (device, uint64) and, when tail_dev (HOST array, may be NULL) names
 * one, into the flashe_limbs(int_bits) limbs at tail_dev[c] -- element n of client c's upload.  Bit for bit the values of
 * flashe_quantize_encrypt_tensors_dev's front end.  The table is uploaded synchronously (not inside a graph capture). */
int flashe_quantize_cohort_dev(flashe_ctx *ctx, int n_clients, uint64_t n, const flashe_tensor_layer *layers, int n_layers, const void *const *src_dev,
                               const int32_t *src_dtype, int element_bits, const double *u_dev, uint64_t u_stride, const double *zzz, int zzz_is_f64,
                               uint64_t *const *pt_dev, uint64_t *const *tail_dev, uint64_t *zeros_dev);
/* Those two steps of a sparse cohort's uploads in ONE launch (new): flashe_quantize_cohort_dev followed by flashe_encrypt_dev(iter, idx[c],
 * FLASHE_SCHEME_SINGLE, n, n_jobs) per client (jzf_quantize.py:433-465, jzf_aggregator.py:717-743, jzf_flashe.py:471-478), chained from
 * the floats: no plaintext vector exists in HBM and the launch count does not depend on n_clients.  layers, src_dev, src_dtype, u_dev,
 * u_stride, zzz, zzz_is_f64 and zeros_dev exactly as flashe_quantize_cohort_dev takes them; idx: HOST array of the clients' cipher
 * indices (any values).  ct_dev[c] (HOST array of device pointers, 8-byte aligned): client c's upload of n + 1 ONE-LIMB elements --
 * elements [0, n) are the single-mask ciphertexts of what flashe_quantize_cohort_dev would have written to pt_dev[c], bit for bit (the
 * chunking runs over n), element n is the plain quantised 'zzz' value that also goes to zeros_dev[c].
 * FLASHE_ENOTSUP -- nothing was launched, run the two steps -- unless int_bits is 16, 20, 23, 24 or 32, the PRF backend the table one,
 * FLASHE_CHAIN not 0, n_clients <= 128 and 0 < n < 2^32.  Sources that are not read in place (float16 / bfloat16, SHIFT, a float32 source
 * under a LOOP_F64 row) go through one stage pass for all clients.  The tables are uploaded synchronously (not inside a graph capture). */
int flashe_quantize_encrypt_sparse_cohort_dev(flashe_ctx *ctx, uint32_t iter, int n_clients, const uint32_t *idx, uint64_t n, uint32_t n_jobs,
                                              const flashe_tensor_layer *layers, int n_layers, const void *const *src_dev, const int32_t *src_dtype,
                                              int element_bits, const double *u_dev, uint64_t u_stride, const double *zzz, int zzz_is_f64,
                                              uint64_t *const *ct_dev, uint64_t *zeros_dev);

/* ---- multi-GPU exchange (RCCL over xGMI; one process per GPU) ----------------------------------------------- */
/* Replaces, inside one node, the arbiter's gather of client models + reduce in Python + broadcast of the aggregate
 * (jzf_aggregator.py:292-308, :404-430, :502-508): every GPU encrypts and locally reduces the clients it hosts, ONE
 * reduce-scatter mod 2^b combines the partial aggregates, every GPU decrypts the slice it owns (the *_range_dev twins)
 * and an all-gather returns the plaintext aggregate to all.  librccl.so is loaded on first use (dlopen), so programs
 * that never call these functions do not depend on it.  All transfers are enqueued on the ctx stream; a flashe_comm may
 * be used with any ctx of the device it was created on (e.g. a side ctx whose stream overlaps the exchange with the
 * AES-bound kernels).  Every rank must issue the same sequence of collective calls.  All "new". */
#define FLASHE_RCCL_ID_BYTES 128                      /* sizeof(ncclUniqueId) */
typedef struct flashe_comm flashe_comm;
int flashe_rccl_unique_id(uint8_t id[FLASHE_RCCL_ID_BYTES]);       /* rank 0 makes it, the launcher hands it to every rank */
int flashe_rccl_init(flashe_ctx *ctx, const uint8_t id[FLASHE_RCCL_ID_BYTES], int rank, int world, flashe_comm **out);
int flashe_rccl_destroy(flashe_comm *comm);
int flashe_rccl_rank(const flashe_comm *comm);
int flashe_rccl_world(const flashe_comm *comm);          /* as RCCL itself reports it (ncclCommCount) */
/* ncclGetVersion of the librccl.so this library loads (e.g. 22703), without creating a communicator: part of the preflight of a
 * multi-GPU launch.  FLASHE_ENODEV when librccl.so cannot be loaded. */
int flashe_rccl_version(int *version);
/* Piece p (bytes long, at send_dev + p * send_stride) goes to rank p; the piece from rank p lands at recv_dev + p * recv_stride.
 * Grouped ncclSend / ncclRecv: on xGMI every GPU pair has its own link, so the W - 1 transfers run concurrently. */
int flashe_rccl_all_to_all(flashe_ctx *ctx, flashe_comm *comm, const void *send_dev, size_t send_stride,
                           void *recv_dev, size_t recv_stride, size_t bytes);
int flashe_rccl_all_gather(flashe_ctx *ctx, flashe_comm *comm, const void *send_dev, void *recv_dev, size_t bytes);
/* The reduce-scatter mod 2^int_bits that RCCL cannot express (no 128-bit type; ncclSum does not wrap at 2^b):
 * partial_dev = world slices of slice_elems elements; after the call out_slice_dev = sum over ranks of slice [rank]
 * (+ extra_dev when given: one more local operand, e.g. the decrypt mask difference).  recv_dev = world x slice_elems
 * elements of scratch. */
int flashe_rccl_reduce_scatter_modadd(flashe_ctx *ctx, flashe_comm *comm, const uint64_t *partial_dev, uint64_t slice_elems,
                                      uint64_t *recv_dev, const uint64_t *extra_dev, uint64_t *out_slice_dev);
/* Host-value all-reduce, synchronous (timing: max over ranks; agreement: min): op 0 = max, 1 = min, 2 = sum. */
/* int_bits <= 64: buf[j] = (sum over ranks of buf[j]) mod 2^b on every rank, in place -- ncclAllReduce(ncclUint64, ncclSum) + mask
 * (the arbiter's reduce jzf_aggregator.py:424-430 across GPUs; wider moduli use flashe_rccl_reduce_scatter_modadd). */
int flashe_rccl_allreduce_modadd_u64(flashe_ctx *ctx, flashe_comm *comm, uint64_t *buf_dev, uint64_t count);
int flashe_rccl_allreduce_f64(flashe_ctx *ctx, flashe_comm *comm, double *value, int op);
int flashe_rccl_barrier(flashe_ctx *ctx, flashe_comm *comm);

#ifdef __cplusplus
}
#endif
#endif /* FLASHE_H */
