// Internal launch interface between the C ABI (abi.hip) and the gfx950 kernels (kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace flashe_philox { struct ClientPlan; }        // (philox_stream.h)
namespace flashe_pcg64 { struct ClientPlan; }         // (pcg64_stream.h)

namespace flashe {

// AES-256 expanded key, 60 big-endian words; passed to kernels by value (lands in SGPRs).
struct RoundKeys { uint32_t w[60]; };

// Optional fused codec of a SINGLE-job PRF launch (the quantiser is the step right before encrypt / after
// decrypt, jzf_quantize.py:55-67,102-107): front end = the plaintext of element k is the stochastic-rounded quantisation of a
// float instead of a stored integer; back end = the result is written as the unquantised float64 instead of the integer.
// Saves the 8-byte integer round trip through HBM on either side.  All-zero = off.
// One layer of a FLATTENED model (jzf_aggregator.py:625-650: a job quantises layer by layer, each with its own alpha, then encrypts
// the concatenation as one vector): device-resident table, sorted by start, empty layers left out.
struct CodecLayer {
    uint64_t start;            // flat index of the layer's first value
    const void *x;             // front end: the layer's own float32 / float64 values (x[0] = flat element `start`)
    double p0, p1, p2;         // front end: alpha, scale, den; back end: ac, two_a, uden
    int x_is_f64, pad_;
};
struct Codec {
    const void *x;             // front end: float32 / float64 values (null = off)
    const double *u;           //            one uniform draw in [0, 1) per value
    double alpha, scale, den;  //            q = floor((clip(x, -alpha, alpha) + alpha) * scale / den + u), computed in x's type
    int x_is_f64, n_layers;
    double *fout;              // back end: float64 output (null = off)
    double ac, two_a, uden;    //           out = float(value) * two_a / uden - ac
    // layer table (null = one layer described by the fields above): element k of the launch is flat element k0 + k of the model,
    // its parameters (and, front end, its value) come from the layer that holds it; u and fout stay indexed by k
    const CodecLayer *layers;
    uint64_t k0;
};

// Everything a launch needs that is not a per-call argument.
struct LaunchEnv {
    hipStream_t stream;
    int num_cus;
    const uint32_t *te0_dev;   // Te0 | Te1 | Te2 | Te3, 256 entries each, in device memory (4 KiB)
    const uint32_t *rkw_dev;   // the 60 expanded key words in device memory (scalar-loaded per round by the bit-sliced PRF)
    const uint32_t *rkp_dev;   // packed key planes for the 16-blocks-per-lane bit-sliced PRF: 15 x 64 words
    RoundKeys rk;
    int b;                     // int_bits
    int prf_backend;           // PRF_AUTO / PRF_TABLE / PRF_BITSLICE / PRF_HYBRID
    // PRF_HYBRID: the bit-sliced kernel takes `hybrid_bs_permille` / 1000 of the elements on a second
    // stream while the LDS-table kernel runs the rest -- they saturate different pipes (VALU vs LDS)
    hipStream_t stream2;
    hipEvent_t ev_fork, ev_join;
    int hybrid_bs_permille;
    const Codec *codec;        // host pointer, null except inside the fused quantise / unquantise entry points (single-job launches)
    uint32_t *err_flag;        // host-mapped word: set to 1 when a sparse kernel skips an out-of-range / out-of-order location
    int use_chain;             // 1 (default): jobs over the same range that share a prefix share the PRF stream (prf_chain_kernel)
    int elem32 = 0;            // 1 inside the *_u32_dev entry points (int_bits <= 32): plaintext / ciphertext vectors are uint32 arrays
};

enum { PRF_AUTO = 0, PRF_TABLE = 1, PRF_BITSLICE = 2, PRF_HYBRID = 3, PRF_BITSLICE16 = 4 };

// out = (in? + sum_{k<n_add} term(iter, add[k]) - sum_{k<n_minus} term(iter, minus[k])) mod 2^b.
// add/minus are HOST arrays (copied into the kernel argument block; at most kMaxIdx each).
constexpr int kMaxIdx = 96;
// The launch covers global elements [first, first + count) of an n-element vector; in_dev / out_dev
// are indexed by (element - first).  n and n_jobs define the chunking (b <= 64).
hipError_t launch_prf(const LaunchEnv &env, uint32_t iter,
                      const uint32_t *add, int n_add, const uint32_t *minus, int n_minus,
                      uint64_t n, uint32_t n_jobs, uint64_t first, uint64_t count,
                      const uint64_t *in_dev, int in_limbs, uint64_t *out_dev);

// Several independent encrypts of equal length in ONE launch: vector v is encrypted with prefix idx[v]
// (and idx[v] + 1 when `dbl`); at most kMaxBatch vectors per launch.
constexpr int kMaxBatch = 32;      // jobs per launch (general table)
constexpr int kMaxUniformBatch = 128;   // equal-length whole vectors per launch (compact table, b > 64)
hipError_t launch_prf_batch(const LaunchEnv &env, uint32_t iter, bool dbl, int n_vec, const uint32_t *idx,
                            const uint64_t *const *in_dev, int in_limbs, uint64_t *const *out_dev, uint64_t n,
                            uint32_t n_jobs);
// The same batch as ONE chain that also writes sum_v out[v] mod 2^b to sum_out_dev (the local partial aggregate).  Returns
// hipErrorNotSupported -- nothing launched -- unless the batch is one run of consecutive cipher indices of the double mask with
// int_bits > 64, at most kMaxUniformBatch vectors, long enough to fill the chip: the caller then encrypts and reduces separately.
// dmask_dev (optional, pointer addresses element `first`): the same launch also writes the decrypt mask of the batch,
// term(idx[n_vec - 1] + 1) - term(idx[0]) mod 2^b -- what a decrypt of the sum with add = [idx[n_vec - 1] + 1], minus = [idx[0]] adds.
// dec_out_dev (optional, instead of dmask_dev, pointer addresses element `first`): the same launch also writes that decrypt of the sum
// itself (PrfChain::dec_out_dev); hipErrorNotSupported -- nothing launched -- outside the shape of prf_dec_sum128_kernel.
hipError_t launch_prf_batch_sum(const LaunchEnv &env, uint32_t iter, int n_vec, const uint32_t *idx, const uint64_t *const *in_dev,
                                int in_limbs, uint64_t *const *out_dev, uint64_t *sum_out_dev, uint64_t n, uint32_t n_jobs, uint64_t first,
                                uint64_t count, uint64_t *dmask_dev = nullptr, uint64_t *dec_out_dev = nullptr);
// The quantising front end of a COHORT launch (prf_chain_cohort_kernel): every output of one summed double-mask chain is a client's
// own float model, all clients sharing one layer table.  layers: device table of the non-empty layers, ascending start, x unused
// (p0, p1, p2 = alpha, scale, den: codec_layer_front); src: device table, src[c * n_layers + l] = client c's values of table row l
// (float32, or float64 where the row says x_is_f64), read in place.
struct CohortCodec {
    const CodecLayer *layers;
    const void *const *src;
    int n_layers, pad_;
};
// The BATCHED cohort (prf_chain_cohort_batch_kernel): the chain runs over the model's n_elems batched elements (as BatchLayer's: every
// layer padded to whole elements on its own) and element e of table row l holds bs = int_bits / field_bits values of every client, the
// first one most significant.  cc is the table of the un-batched launch (row l: start = the layer's first VALUE among the n_values of the
// model, alpha / scale / den, the compute type; src as above); rows[2 l], rows[2 l + 1] = the row's first element and its value count.
struct CohortBatch {
    const uint64_t *rows;
    uint64_t n_values;         // values of one model: client c's draws are u_dev[c * n_values ..]
    int field_bits, pad_;
};
// The shapes the wide cohort launch takes, on the environment and the sizes alone (no HIP call; what a caller asks before it stages anything):
// the chained table PRF at int_bits > 64 without a fused codec, 1 .. kMaxLinks clients, n_elems in one 2^32 counter window and at least two
// whole 256-element tiles for each of the chip's waves; bs = 0: un-batched, else the values per element, 5, 6 or 7.
bool cohort_chain_admits(const LaunchEnv &env, int n_vec, uint64_t n_elems, int bs);
// launch_prf_batch_sum over whole n-element vectors with the cohort's front end.  cb == null: client c's plaintext k is the
// stochastic-rounded quantisation of its float k with the draw u_dev[c * n + k] (codec_quantize's arithmetic), no integer plaintext exists
// in HBM.  cb: n counts batched elements, client c's plaintext of element e = quantize_batch_model_kernel's with the draws
// u_dev[c * n_values + value index], bs = env.b / field_bits.  idx: any strictly ascending indices below 2^32 - 1 -- one run launches
// prf_chain_cohort_kernel / prf_chain_cohort_batch_kernel, several runs (clients dropped out) their _runs_ forms over the |idx| + runs streams
// of cohort_streams.h, whose decrypt mask is that of the telescoped lists.  hipErrorNotSupported -- nothing launched -- outside
// cohort_chain_admits, for idx cohort_streams refuses (not ascending, 2^32 - 1, more than kCohortMaxStreams streams), a null output or an
// empty table; dmask_dev is optional.
hipError_t launch_prf_cohort_sum(const LaunchEnv &env, uint32_t iter, int n_vec, const uint32_t *idx, const CohortCodec &cc, const CohortBatch *cb,
                                 const double *u_dev, uint64_t *const *out_dev, uint64_t *sum_out_dev, uint64_t n, uint32_t n_jobs,
                                 uint64_t *dmask_dev = nullptr);
// The shapes the two compact cohort launches below take, in the same terms: int_bits 16 / 20 / 23 / 24 / 32, the chained table PRF without
// a fused codec, 1 .. kMaxLinks clients, 0 < n < 2^32, n_jobs != 0 and, for the `summed` one, at least 2 x 128 AES blocks (of
// 128 / int_bits elements, per the chunking of n_jobs) for each of the chip's waves.
bool small_cohort_admits(const LaunchEnv &env, int n_vec, uint64_t n, uint32_t n_jobs, bool summed);
// The same cohort at int_bits <= 32 in the compact layout (prf_small_cohort_kernel): uint32 ciphertexts and their uint32 sum from the
// floats, admitted where the summed compact chain is -- small_cohort_admits(summed) and strictly ascending idx below 2^32 - 1 whose
// streams fit the table (cohort_streams.h; several runs: prf_small_cohort_runs_kernel).  hipErrorNotSupported: nothing launched.
hipError_t launch_small_cohort_sum(const LaunchEnv &env, uint32_t iter, int n_vec, const uint32_t *idx, const CohortCodec &cc, const double *u_dev,
                                   uint32_t *const *out_dev, uint32_t *sum_out_dev, uint64_t n, uint32_t n_jobs);
// The shapes the one-limb cohort launch below takes: int_bits 33 .. 64 and, at these widths, the conditions of small_cohort_admits(summed)
// (the precondition and the length rule are each stated once in kernels.hip; 0 < n < 2^32, n_jobs != 0).
bool limb_cohort_admits(const LaunchEnv &env, int n_vec, uint64_t n, uint32_t n_jobs);
// The same cohort at int_bits 33 .. 64 in the one-limb layout (prf_limb_cohort_kernel<2 | 3>): uint64 ciphertexts (8-byte aligned) and
// their uint64 sum from the floats, no decrypt mask.  Admitted where limb_cohort_admits says, for strictly ascending idx below 2^32 - 1
// whose streams fit the table (cohort_streams.h; several runs: prf_limb_cohort_runs_kernel<2 | 3>).  hipErrorNotSupported: nothing launched.
hipError_t launch_limb_cohort_sum(const LaunchEnv &env, uint32_t iter, int n_vec, const uint32_t *idx, const CohortCodec &cc, const double *u_dev,
                                  uint64_t *const *out_dev, uint64_t *sum_out_dev, uint64_t n, uint32_t n_jobs);
// The sparse job's cohort at the same widths (prf_small_sparse_cohort_kernel): out_dev[c][k] = SINGLE-mask encrypt (idx[c]; any indices) of the
// quantisation of client c's compact value k with the draw u_dev[c * u_stride + k], k < n, in the ONE-LIMB layout (uint64 elements, 8-byte
// aligned), and out_dev[c][n] = zeros_dev[c] = the client's 'zzz' value zzz_dev[c] quantised in plain with (z_alpha, z_scale, z_den) in
// float64 / float32 and the draw u_dev[c * u_stride + n].  No minimum length: short vectors are cut into runs of clients.
// hipErrorNotSupported -- nothing launched -- outside small_cohort_admits(not summed).
hipError_t launch_small_sparse_cohort(const LaunchEnv &env, uint32_t iter, int n_vec, const uint32_t *idx, const CohortCodec &cc, const double *u_dev,
                                      uint64_t u_stride, uint64_t *const *out_dev, uint64_t n, uint32_t n_jobs, const double *zzz_dev, bool zzz_f64,
                                      double z_alpha, double z_scale, double z_den, uint64_t *zeros_dev);
// The SHORT cohort (cohort_cut.h): the two summed cohort launches above without their length rules, the chain cut into runs of consecutive
// clients whose sums and decrypt masks one combine pass adds up.  cohort_cut_parts_of: the pieces the launch will use -- 0 outside the
// uncut launch's other conditions (wide: cohort_chain_admits' without the length rule and the batch size; compact:
// small_cohort_admits(not summed)) -- from the environment and the sizes alone; the caller sizes the scratch
// from it: parts x n x 16 B for the sums and as much again behind them for the masks (wide, with dmask_dev), parts x n x 4 B (compact),
// unused when parts == 1.  hipErrorNotSupported: nothing launched.
// idx: any strictly ascending indices in at most 16 runs -- every gap is a cut (cohort_cut_pieces, cohort_cut.h).  cohort_cut_pieces_of: the
// pieces of such a cohort under the same admission, begins[0 .. parts] the first present-client position of each (kCutMaxParts + 1 entries);
// one run: cohort_cut_parts_of's pieces exactly.  bs: 0, or the values per element of a BATCHED cohort (launch_prf_cohort_batch_cut: wide
// only, bs 5 .. 7, n = the batched elements, launch_prf_cohort_sum's batched arguments).
int cohort_cut_parts_of(const LaunchEnv &env, int n_vec, uint64_t n, uint32_t n_jobs, bool compact);
int cohort_cut_pieces_of(const LaunchEnv &env, int n_vec, const uint32_t *idx, uint64_t n, uint32_t n_jobs, bool compact, int bs, int *begins);
hipError_t launch_prf_cohort_batch_cut(const LaunchEnv &env, uint32_t iter, int n_vec, const uint32_t *idx, const CohortCodec &cc, const CohortBatch &cb,
                                       const double *u_dev, uint64_t *const *out_dev, uint64_t *sum_out_dev, uint64_t n, uint32_t n_jobs,
                                       uint64_t *dmask_dev, uint64_t *scratch_dev);
hipError_t launch_prf_cohort_cut(const LaunchEnv &env, uint32_t iter, int n_vec, const uint32_t *idx, const CohortCodec &cc, const double *u_dev,
                                 uint64_t *const *out_dev, uint64_t *sum_out_dev, uint64_t n, uint32_t n_jobs, uint64_t *dmask_dev, uint64_t *scratch_dev);
hipError_t launch_small_cohort_cut(const LaunchEnv &env, uint32_t iter, int n_vec, const uint32_t *idx, const CohortCodec &cc, const double *u_dev,
                                   uint32_t *const *out_dev, uint32_t *sum_out_dev, uint64_t n, uint32_t n_jobs, uint32_t *scratch_dev);
// their combine pass (stream.hip): sum_dev[k] = sum_p psum_dev[p n + k] mod 2^b and, with pmask_dev, dmask_dev[k] = sum_p pmask_dev[p n + k]
hipError_t launch_cohort_cut_combine(const LaunchEnv &env, int parts, uint64_t n, const uint64_t *psum_dev, uint64_t *sum_dev, const uint64_t *pmask_dev,
                                     uint64_t *dmask_dev);
hipError_t launch_cohort_cut_combine_u32(const LaunchEnv &env, int parts, uint64_t n, const uint32_t *psum_dev, uint32_t *sum_dev);
// launch_prf_batch on elements [first, first + count) of the n-element vectors (pointers address element `first`): what a GPU that owns
// an element slice of every client's vector runs
hipError_t launch_prf_batch_range(const LaunchEnv &env, uint32_t iter, bool dbl, int n_vec, const uint32_t *idx, const uint64_t *const *in_dev,
                                  int in_limbs, uint64_t *const *out_dev, uint64_t n, uint32_t n_jobs, uint64_t first, uint64_t count);

// General form of the batched launch: out[k] = in[k] + term(iter, add_idx, first + k)
// - [dbl] term(iter, minus_idx, first + k) for k < count; in_dev may be null (zeros); pointers address element `first`.
// n_in > 1 (in_limbs == 2 only): the input is the mod-2^b sum of n_in vectors, vector c at in_dev + c * in_stride
// limbs -- the arbiter's reduce fused into the decrypt of its result; sum_out_dev (optional) receives that sum.
struct PrfJob {
    uint32_t add_idx, minus_idx;
    uint64_t first, count;
    const uint64_t *in_dev;
    int in_limbs;
    uint64_t *out_dev;
    uint32_t n_in = 1;
    uint64_t in_stride = 0;
    uint64_t *sum_out_dev = nullptr;
};
hipError_t launch_prf_jobs(const LaunchEnv &env, uint32_t iter, bool dbl, int n_entries, const PrfJob *jobs, uint64_t n,
                           uint32_t n_jobs);

// Chained jobs (int_bits > 64): `n_out` outputs over elements [first, first + count) that share their PRF streams.
// Double mask (single == false): n_out + 1 prefixes, out[c] = in[c] + term(idx[c]) - term(idx[c + 1]) -- consecutive clients
// (idx[c + 1] = idx[c] + 1, jzf_flashe.py:349-353) cost n_out + 1 streams instead of 2 n_out; a plain (add, minus) job is a chain
// of one output.  single == true: n_out prefixes, out[c] = in[c] + term(idx[c]).  idx, in_dev, out_dev are HOST arrays; in_dev (or
// an entry of it) may be null = zeros; device pointers address element `first`.  Returns hipErrorNotSupported when a chain cannot
// take this path (a range that straddles a 2^32 counter boundary; int_bits <= 64: a vector of 2^32 elements or more, a fused codec):
// the caller then uses the job-table kernels.  n, n_jobs: the whole vector's length and chunking (int_bits <= 64 counters).
struct PrfChain {
    const uint32_t *idx;
    int n_out;
    bool single;
    uint64_t first, count;
    const uint64_t *const *in_dev;
    int in_limbs;
    uint64_t *const *out_dev;
    uint64_t *sum_out_dev = nullptr;   // optional (int_bits > 64, n_out <= kMaxLinks): receives sum_c out[c] mod 2^b, written by the same launch
    uint64_t *dmask_dev = nullptr;     // optional, with sum_out_dev, the launch's only chain: receives term(idx[n_out]) - term(idx[0]) mod 2^b
    // optional, with sum_out_dev and without dmask_dev, the launch's only chain: receives the DECRYPT of the sum, sum + term(idx[n_out]) -
    // term(idx[0]) mod 2^b (prf_dec_sum128_kernel).  Only at int_bits = 128 with one-limb inputs, every input and output present and at most
    // kSum128MaxCount elements: launch_prf_chains returns hipErrorNotSupported -- nothing launched -- for any other chain that asks for it.
    uint64_t *dec_out_dev = nullptr;
};
hipError_t launch_prf_chains(const LaunchEnv &env, uint32_t iter, int n_chains, const PrfChain *chains, uint64_t n, uint32_t n_jobs);

hipError_t launch_combine(const LaunchEnv &env, uint64_t n, const uint64_t *in_dev, int in_limbs,
                          const uint64_t *add_dev, const uint64_t *minus_dev, uint64_t *out_dev);

// n_vec combines of equal length in as few launches as possible (host arrays of device pointers; add_dev / minus_dev or single
// entries of them may be null)
hipError_t launch_combine_batch(const LaunchEnv &env, uint64_t n, int n_vec, const uint64_t *const *in_dev, int in_limbs,
                                const uint64_t *const *add_dev, const uint64_t *const *minus_dev, uint64_t *const *out_dev);
// the same and sum_out = sum_v out[v] mod 2^b in one pass (the online encrypts with precomputed masks + the reduce of what they wrote)
hipError_t launch_combine_batch_sum(const LaunchEnv &env, uint64_t n, int n_vec, const uint64_t *const *in_dev, int in_limbs,
                                    const uint64_t *const *add_dev, const uint64_t *const *minus_dev, uint64_t *const *out_dev, uint64_t *sum_out_dev,
                                    const uint64_t *dec_add_dev = nullptr, const uint64_t *dec_minus_dev = nullptr, uint64_t *dec_out_dev = nullptr);

// Operand pointers of one reduce pass travel in the kernel argument block (scalar loads).
constexpr int kMaxOps = 64;
struct PtrTable { const uint64_t *p[kMaxOps]; };

// ops: HOST array of C <= kMaxOps device pointers.  out may alias an operand.
// b <= 64: out = (sum of the C operands + term(add) - [has_minus] term(minus)) mod 2^b on elements [first, first + count) in one pass
// (pointers address element `first`; agg_out_dev may be null).  hipErrorNotSupported: reduce and decrypt in two launches instead.
// (env.elem32: the operands are uint32 arrays; out_elem_bytes = 4: so are agg_out_dev and out_dev)
hipError_t launch_small_reduce_decrypt(const LaunchEnv &env, uint32_t iter, uint32_t add_idx, bool has_minus, uint32_t minus_idx, uint64_t n,
                                       uint32_t n_jobs, uint64_t first, uint64_t count, int C, const uint64_t *const *ops, uint64_t *agg_out_dev,
                                       uint64_t *out_dev, int out_elem_bytes = 8);
// uint32 <-> uint64 element arrays (zero extension / truncation), n elements
hipError_t launch_widen_u32(const LaunchEnv &env, uint64_t n, const uint32_t *in_dev, uint64_t *out_dev);
hipError_t launch_narrow_u32(const LaunchEnv &env, uint64_t n, const uint64_t *in_dev, uint32_t *out_dev);
hipError_t launch_aggregate_elem(const LaunchEnv &env, int C, const uint64_t *const *ops,
                                 uint64_t n, uint64_t *out_dev);
// the same on uint32 element arrays (compact layout, int_bits <= 32)
hipError_t launch_aggregate_elem_u32(const LaunchEnv &env, int C, const uint32_t *const *ops, uint64_t n, uint32_t *out_dev);

// summaries_dev: scratch of at least packed_num_blocks(n_limbs) uint32 words.
// out must NOT alias an operand (blocks re-read their left neighbour's inputs).
uint64_t packed_num_blocks(uint64_t n_limbs);
hipError_t launch_aggregate_packed(const LaunchEnv &env, int C, const uint64_t *const *ops,
                                   uint64_t n_limbs, uint64_t total_bits, uint64_t *out_dev,
                                   uint32_t *summaries_dev);

// the same sum computed on UNPACKED vectors: out = unpack(sum_c pack(ops[c]) mod 2^(n b)), element j at bit (n - 1 - j) b, with no
// packed vector.  elem_bytes: 4 (uint32 elements, b <= 32), 8 (b <= 64) or 16 (b > 64; out 16-byte aligned, operands 8).  C <= kMaxOps
// and C <= 2^b (hipErrorNotSupported otherwise).  summaries_dev: at least packed_elems_num_blocks(n) uint32 words.  out must NOT alias
// an operand (lanes read their neighbours' columns).
uint64_t packed_elems_num_blocks(uint64_t n);
hipError_t launch_aggregate_packed_elems(const LaunchEnv &env, int C, const uint64_t *const *ops, uint64_t n, int elem_bytes, void *out_dev,
                                         uint32_t *summaries_dev);

// helpers for a packed reduce cut into limb slices across GPUs: (low limb, body-all-ones, carry limb) of a
// slice sum, and the in-place carry-in ripple
hipError_t launch_packed_probe(const LaunchEnv &env, uint64_t n_limbs, const uint64_t *x_dev, uint64_t *info_dev);
hipError_t launch_packed_add_carry(const LaunchEnv &env, uint64_t n_limbs, uint64_t total_bits, uint64_t cin, uint64_t *x_dev);
// the same with the carry-in derived on the device from the probe triples of the n_below slices underneath (infos_dev: 3 words each)
// (stride_words: from one slice's triple to the next more significant one's; negative = the gathered triples run from the most
// significant slice down and infos_dev points at the lowest slice's)
hipError_t launch_packed_resolve_carry(const LaunchEnv &env, uint64_t n_limbs, uint64_t total_bits, const uint64_t *infos_dev, int n_below,
                                       uint64_t *x_dev, int stride_words = 3);

hipError_t launch_pack(const LaunchEnv &env, uint64_t n, const uint64_t *in_dev, uint64_t *out_dev);
hipError_t launch_unpack(const LaunchEnv &env, uint64_t n, const uint64_t *in_dev, uint64_t *out_dev);

hipError_t launch_fill(const LaunchEnv &env, uint64_t n, uint64_t lo, uint64_t hi, uint64_t *out_dev);
// locations >= total are skipped and reported through env.err_flag (the reference raises IndexError, jzf_aggregator.py:150-165)
hipError_t launch_scatter(const LaunchEnv &env, uint64_t total, uint64_t k, const uint32_t *loc_dev,
                          const uint64_t *vals_dev, uint64_t *out_dev, bool accumulate,
                          uint64_t sub_lo = 0, uint64_t sub_hi = 0);
// Sparse reduce over strictly increasing location lists (LDS-staged, the dense output is written once):
// out[p] = from[p] +/- sum_{c, q: loc[c][q] == p} (vals[c][q] - sub[c]) mod 2^b for every p < total, where from = src_dev when it
// is given (it may be out_dev: accumulate in place) and the constant base otherwise; negate subtracts the sum (a decrypt:
// aggregate - minus-mask in the pass that builds the mask).  At most kMaxScatter clients per call;
// start_dev = (span_count(total, span) + 1) * C words of scratch.
constexpr int kMaxScatter = 64;
// positions per span: the plain reduce keeps 64 KiB of accumulators per workgroup, the passes with the PRF inside (launch_span_prf)
// what the AES tables leave of a CU's LDS.  A table of span bounds serves the kernels of ONE of the two sizes (launch_span_bounds fills both in one pass).
#ifndef FLASHE_SPAN_FUSED
#define FLASHE_SPAN_FUSED 1752
#endif
constexpr int kSpanReduce = 4096, kSpanFused = FLASHE_SPAN_FUSED;
uint64_t span_count(uint64_t total, int span);
// words of a bounds table that is large enough for either span size
inline size_t span_table_words(uint64_t total, int C) { return static_cast<size_t>(span_count(total, kSpanFused) + 1) * static_cast<size_t>(C); }
// (bounds_ready: start_dev already holds the bounds of exactly these lists -- launch_span_bounds -- and the pass that computes them is skipped)
hipError_t launch_span_reduce(const LaunchEnv &env, int C, const uint32_t *const *loc_dev, const uint64_t *const *vals_dev,
                              const uint64_t *k, const uint64_t *sub, uint64_t base_lo, uint64_t base_hi, uint64_t total,
                              uint32_t *start_dev, const uint64_t *src_dev, bool negate, uint64_t *out_dev, bool bounds_ready = false);
// the first list entry of each of the C <= kMaxScatter clients in every span, at kSpanReduce and / or kSpanFused positions per span
// (either table may be null): (span_count(total, span) + 1) * C words each, one pass over the lists
hipError_t launch_span_bounds(const LaunchEnv &env, int C, const uint32_t *const *loc_dev, const uint64_t *k, uint64_t total, uint32_t *start_reduce_dev,
                              uint32_t *start_fused_dev);
// The span reduce with the PRF inside (table PRF; one persistent launch): entry q of client c contributes its single-mask term --
// int_bits > 64: term(iter, idx[c], q); int_bits <= 64: the slot of entry q in the block of its chunk of the n_jobs-chunked list
// (stream.hip, span_prf_small_kernel).  pt_dev null: out[p] = from[p] +/- the sum of the masks at p (sparse minus-mask / decrypt);
// pt_dev given: ct_dev[c][q] = (pt_dev[c][q] + mask) mod 2^b is stored (where ct_dev[c] is not null) and out[p] = from[p] + sum (ct - sub[c]);
// pt_limbs = 1: the plaintexts are uint64 arrays; sub: L words per client.  start_dev: bounds of exactly these lists at kSpanFused.
// [first, first + count): the positions this launch covers (span-aligned, see stream.hip) -- src_dev / out_dev address position
// `first`; entries outside it are left alone (their ciphertexts are not written).
hipError_t launch_span_prf(const LaunchEnv &env, uint32_t iter, uint32_t n_jobs, int C, const uint32_t *idx, const uint32_t *const *loc_dev, const uint64_t *k,
                           const uint64_t *const *pt_dev, int pt_limbs, uint64_t *const *ct_dev, const uint64_t *sub, uint64_t base_lo, uint64_t base_hi,
                           uint64_t total, const uint32_t *start_dev, const uint64_t *src_dev, bool negate, uint64_t *out_dev, uint64_t first, uint64_t count);
#ifdef FLASHE_TUNING
hipError_t span_prf_cycles(unsigned long long *out8, bool reset);      // phase cycle sums of span_prf_kernel's workgroup 0 (FLASHE_SPAN_PROBE=9)
#endif
// Sparse + double mask (jzf_flashe.py:388-426, :155-225): compact (add, minus) mask values of a group of nc <= kMaxScatter clients
// c0 .. c0 + nc - 1 at their own sorted locations -- entry q of client c gets term(c + 1, p) unless client c + 1 holds p, and
// term(c, p) unless client c - 1 holds p (dense-position counters, one chunk).  loc / k carry nc + 2 entries: the group's lists
// framed by the neighbouring clients' (null / 0 where there is none).
hipError_t launch_sparse_edge_prf(const LaunchEnv &env, uint32_t iter, int nc, uint32_t c0, const uint32_t *const *loc_with_neighbours,
                                  const uint64_t *k_with_neighbours, uint64_t *const *va_dev, uint64_t *const *vm_dev);
// Adds to *count_dev the number of list entries of clients 0 .. nc - 1 whose position the NEXT client's (sorted) list holds too.
// loc_with_next / k_with_next carry nc + 1 entries: the group's lists followed by the client after the group (null / 0 if none).
hipError_t launch_shared_positions(const LaunchEnv &env, int nc, const uint32_t *const *loc_with_next, const uint64_t *k_with_next,
                                   unsigned long long *count_dev);
// out[p] = (out[p] + (sel[p] ? stream[p] : 0)) mod 2^b
hipError_t launch_sel_accumulate(const LaunchEnv &env, uint64_t total, const uint8_t *sel_dev,
                                 const uint64_t *stream_dev, uint64_t *out_dev);

// Quantise / batch codec
// descriptors for LaunchEnv::codec
Codec codec_quantize_front(const void *x_dev, bool is_f64, double alpha, int bits, const double *u_dev);
void codec_unquantize_back(Codec *c, double alpha, int bits, int num_clients, double *out_dev);
// the same per layer of a flattened model, as entries of the device table Codec::layers points to
CodecLayer codec_layer_front(uint64_t start, const void *x_dev, bool is_f64, double alpha, int bits);
CodecLayer codec_layer_back(uint64_t start, double alpha, int bits, int num_clients);
// x <- x + shift in place (normalize / unnormalize, jzf_quantize.py:542-564).  f32 arrays: wide = the add runs in float64 and is
// rounded once (NumPy's loop for a float64 scalar operand), otherwise in float32
hipError_t launch_shift(const LaunchEnv &env, uint64_t n, void *x_dev, bool is_f64, double shift, bool wide);
// partial sums for mean / std: part[g] = sum over block g's elements of (x - center)^pow, pow = 1 or 2, float64; returns the grid size
int moments_grid(const LaunchEnv &env, uint64_t n);
hipError_t launch_moment(const LaunchEnv &env, uint64_t n, const void *x_dev, bool is_f64, double center, int pow, double *part_dev);
hipError_t launch_quantize(const LaunchEnv &env, uint64_t n, const void *x_dev, bool is_f64, double alpha, int bits,
                           const double *u_dev, uint64_t *q_dev);
// the codec back end over a flattened model without a PRF stream: out[k] = unquantise(v[k]) with the layer table of cq (k0 = first element)
hipError_t launch_unquantize_model(const LaunchEnv &env, uint64_t count, const uint64_t *v_dev, const Codec &cq, double *out_dev);
hipError_t launch_unquantize(const LaunchEnv &env, uint64_t n, const uint64_t *v_dev, int v_limbs, double alpha, int bits,
                             int num_clients, double *out_dev);
hipError_t launch_batch(const LaunchEnv &env, uint64_t n, const uint64_t *vals_dev, int field_bits, uint64_t *out_dev);
// The BATCHED codec over a whole model (jzf_quantize.py:436-451 under :417-462, then jzf_aggregator.py:723): every layer is quantised
// with its own alpha and batched ON ITS OWN (zero padded to whole elements), the batched layers lie back to back in the flattened
// vector.  Device table, one entry per non-empty layer, ascending elem_start.
struct BatchLayer {
    uint64_t elem_start;       // first batched element of the layer in the flattened vector
    uint64_t value_start;      // index of the layer's first value among all values of the model (its draw / its float output)
    uint64_t size;             // values in the layer
    const void *x;             // front end: the layer's float32 / float64 values
    double p0, p1, p2;         // front end: alpha, scale, den; back end: ac, two_a, uden
    int x_is_f64, pad_;
};
// out[e] = sum_t quantize(value bs * e_local + t) << (field_bits * (bs - 1 - t)) for the n_elems batched elements (bs = int_bits / field_bits)
hipError_t launch_quantize_batch_model(const LaunchEnv &env, const BatchLayer *layers_dev, int n_layers, int field_bits, const double *u_dev,
                                       uint64_t n_elems, uint64_t *out_dev);
// out[value_start + j] = unquantize(field t of element elem_start + j / bs), the inverse walk, for the n_values values of the model
hipError_t launch_unbatch_unquantize_model(const LaunchEnv &env, const BatchLayer *layers_dev, int n_layers, int field_bits, const uint64_t *in_dev,
                                           uint64_t n_values, double *out_dev);
BatchLayer batch_layer_front(uint64_t elem_start, uint64_t value_start, uint64_t size, const void *x_dev, bool is_f64, double alpha, int bits);
BatchLayer batch_layer_back(uint64_t elem_start, uint64_t value_start, uint64_t size, double alpha, int bits, int num_clients);
// The same codec walks with the ctx's precomputed masks in place of the PRF streams (no AES): ct = (quantize + add - minus) mod 2^b and
// out = unquantize((in + add - minus) mod 2^b).  minus_dev may be null (a single-mask cache); the un-batched forms take cq's layer table
// (k0 = the launch's first element; add / minus / ct / in address that element)
hipError_t launch_quantize_combine_model(const LaunchEnv &env, uint64_t count, const Codec &cq, const uint64_t *add_dev, const uint64_t *minus_dev,
                                         uint64_t *ct_dev);
hipError_t launch_combine_unquantize_model(const LaunchEnv &env, uint64_t count, const uint64_t *in_dev, const uint64_t *add_dev,
                                           const uint64_t *minus_dev, const Codec &cq, double *out_dev);
hipError_t launch_quantize_batch_combine_model(const LaunchEnv &env, const BatchLayer *layers_dev, int n_layers, int field_bits, const double *u_dev,
                                               uint64_t n_elems, const uint64_t *add_dev, const uint64_t *minus_dev, uint64_t *ct_dev);
hipError_t launch_combine_unbatch_unquantize_model(const LaunchEnv &env, const BatchLayer *layers_dev, int n_layers, int field_bits, const uint64_t *in_dev,
                                                   const uint64_t *add_dev, const uint64_t *minus_dev, uint64_t n_values, double *out_dev);
// A COHORT's online step with masks the caller holds (codec.hip): ct[c][k] = (plaintext of client c's element k + mask[c][k]) mod 2^b
// for every client and sum[k] = sum_c ct[c][k] mod 2^b, in one pass with no AES.  layers / src: CohortCodec's tables (n_layers rows);
// mask / ct: DEVICE tables of the n_clients vectors, so one launch takes any number of clients; sum may be null.  Un-batched: n values,
// plaintext = the quantisation with the draw u[c * n_values + k] (n_values = n).  Batched: n elements of bs values in fields of
// field_bits, plaintext = quantize_batch_model_kernel's with the draws u[c * n_values + value index]; rows as CohortBatch's.
struct PrepCohort {
    const CodecLayer *layers;
    const void *const *src;
    const void *const *mask;
    void *const *ct;
    const uint64_t *rows;
    const double *u;
    void *sum;
    uint64_t n, n_values;
    int n_layers, n_clients, field_bits, bs;
};
// Where that launch takes its draws from.  kBuffer: pc.u.  kPhilox / kPcg64: the draws of np.random.Philox / PCG64 / PCG64DXSM streams are
// generated inside the launch and pc.u is not read; plans = a DEVICE table of one flashe_philox::ClientPlan (philox_stream.h: client c's
// draw for its flat value k = word (skip + k) % 4 of block(base + (skip + k) / 4); a batched job's pads draw nothing) or one
// flashe_pcg64::ClientPlan (pcg64_stream.h) per client, those all of the one variant (0 PCG64, 1 PCG64DXSM; never batched): a lane keeps the
// jump to its run of four values and composes it with the stride jump of the grid, which prep_pcg64_grid gives for n values.  Batched
// kPhilox: a lane owns a GROUP of four consecutive elements of one row (the row's last group may hold fewer); groups = a DEVICE table of
// every row's first group, n_groups the launch's groups.
struct PrepDraws {
    enum Kind { kBuffer, kPhilox, kPcg64 } kind; bool batched;
    const void *plans; uint32_t variant;                 // drawn forms; kPcg64
    const uint64_t *groups; uint64_t n_groups;           // batched kPhilox
};
int prep_pcg64_grid(const LaunchEnv &env, uint64_t n);
// elem_bytes = what masks, ciphertexts and sum are made of: 4 (uint32, int_bits <= 32, un-batched), 8 (one limb, int_bits <= 64) or 16
hipError_t launch_prep_cohort(const LaunchEnv &env, const PrepCohort &pc, const PrepDraws &draws, int elem_bytes);
hipError_t launch_unbatch(const LaunchEnv &env, uint64_t nb, const uint64_t *in_dev, int field_bits, uint64_t *out_dev);

// Caller-owned tensors either side of the model-wide codec (tensors.hip).  dtype / flags as in flashe_tensor_layer (include/flashe.h);
// kTensorLoopF64: the front end widens to float64 (the layer's NumPy loop dtype is float64).
constexpr int kTensorF32 = 0, kTensorF64 = 1, kTensorF16 = 2, kTensorBF16 = 3;
constexpr int kTensorShift = 1, kTensorShiftWide = 2, kTensorLoopF64 = 4;
struct TensorStage {          // front end: src (stored dtype) -> dst (compute type), value k of the layer = staged value start + k
    uint64_t start;
    const void *src;
    void *dst;
    double shift;
    int dtype, flags;
};
// dst[k] = src[k] as float32 / float64, normalised first with SHIFT; one lane per value of the concatenated staged layers
hipError_t launch_stage_layers(const LaunchEnv &env, const TensorStage *tab_dev, int n_tab, uint64_t total);
struct TensorStore {          // back end: groups of 8 values of the flat float64 vector -> the layer's tensor
    uint64_t start;           // flat index of the layer's first value
    uint64_t group_start;     // first 8-value group of the layer among all groups
    uint64_t size;
    void *dst;
    double shift;
    int dtype, flags;
};
hipError_t launch_store_layers(const LaunchEnv &env, const TensorStore *tab_dev, int n_tab, uint64_t n_groups, const double *in_dev);
struct StatLayer {            // NumPy-exact sum and sum of squared deviations of y = in (+ shift) over one layer
    uint64_t start;           // flat index of the layer's first value
    uint64_t blk_start;       // first summation buffer of the layer among all buffers
    uint64_t size;
    double shift;
    int flags, out_index;     // stats[2 * out_index] = sum, stats[2 * out_index + 1] = sum of (y - sum / size)^2
};
hipError_t launch_layer_stats(const LaunchEnv &env, const StatLayer *tab_dev, int n_tab, uint64_t n_blocks, const double *in_dev, uint64_t block,
                              double *bsum_dev, double *means_dev, double *stats_dev);

// The two passes with the aggregator's degree scaling (flashe_stage_layers_dev / flashe_finish_layers_dev; flags as in include/flashe.h).
// Front, jzf_aggregator.py:676 then jzf_quantize.py:542-547: dst[k] = src[k] (* scale) (+ shift) in the type NumPy gives the layer at
// each step, stored as float32 or -- kStageOutF64 -- float64.  Rows of one model or of a cohort's C x L layers; groups of eight values
// of one row per lane as in the store pass.
constexpr int kStageScale = 1, kStageScaleWide = 2, kStageShift = 4, kStageShiftWide = 8, kStageOutF64 = 16;
struct StageRow {
    uint64_t group_start;     // first 8-value group of the row among all groups
    uint64_t size;
    const void *src;
    void *dst;
    double scale, shift;
    int dtype, flags;         // dtype: how src is stored
};
hipError_t launch_stage_rows(const LaunchEnv &env, const StageRow *tab_dev, int n_tab, uint64_t n_groups);
// Back, jzf_aggregator.py:902-907: y1 = in / div_total, y2 = y1 + shift, y3 = y2 / div_own, y4 = last + y3, each under its flag, stored in
// the row's dtype; the statistics sum y2.  last may be dst itself (same dtype): a lane reads the eight values it writes.
constexpr int kFinishDivTotal = 1, kFinishShift = 2, kFinishDivOwn = 4, kFinishAddLast = 8;
struct FinishRow {
    uint64_t start;           // flat index of the row's first value
    uint64_t group_start;
    uint64_t size;
    void *dst;
    const void *last;
    double div_total, shift, div_own;
    int dtype, last_dtype, flags, pad_;
};
hipError_t launch_finish_layers(const LaunchEnv &env, const FinishRow *tab_dev, int n_tab, uint64_t n_groups, const double *in_dev);
struct FinishStat {           // StatLayer with the division in front of the shift
    uint64_t start, blk_start, size;
    double div_total, shift;
    int flags, out_index;     // flags: kFinishDivTotal / kFinishShift
};
hipError_t launch_finish_stats(const LaunchEnv &env, const FinishStat *tab_dev, int n_tab, uint64_t n_blocks, const double *in_dev, uint64_t block,
                               double *bsum_dev, double *means_dev, double *stats_dev);

// The sparse job's codec front end for a cohort of co-located clients (flashe_quantize_cohort_dev, tensors.hip): C clients' compact
// layers -> C one-limb plaintext vectors in ONE launch, shift + quantise in registers (no staged copy).  Row r of the shared table:
// compact values [start, next start) of every client, quantised with (alpha, scale, den) in float32 or -- loop_f64 -- float64, after
// stage_layers_kernel's normalise rule (flags: kTensorShift / kTensorShiftWide).  src[c * n_rows + r] / src_dtype[...] = where client
// c's values of row r lie and how they are stored.  Client c's value j takes the draw u[c * u_stride + j]; its trailing 'zzz' value
// zzz[c] (alpha 1.0: zrow) takes the draw u[c * u_stride + n], goes to zeros[c] and, as `tail_limbs` limbs, to tail[c].
struct QuantCohortRow {
    uint64_t start;
    double alpha, scale, den, shift;
    int32_t loop_f64, flags;
};
struct QuantCohort {
    const QuantCohortRow *rows;
    const void *const *src;
    const int32_t *src_dtype;
    uint64_t *const *pt;       // [n_clients] plaintexts of n values, one limb each
    uint64_t *const *tail;     // [n_clients] element n of client c's upload
    const double *zzz;         // [n_clients]
    uint64_t *zeros;           // [n_clients]
    int n_rows, n_clients, tail_limbs, pad_;
    QuantCohortRow zrow;
};
hipError_t launch_quantize_cohort(const LaunchEnv &env, const QuantCohort &qc, uint64_t n, const double *u_dev, uint64_t u_stride);

// Top-k of every layer of a model in one set of launches: the layers lie back to back in flat buffers.  The caller fills the host
// layer table with sparsify_batch_layout (-> number of 1024-element blocks), copies its sparsify_batch_desc_bytes(L) bytes to the START
// of a device workspace of sparsify_batch_workspace_bytes(L, blocks), then launches.
size_t sparsify_batch_workspace_bytes(int L, uint64_t n_blocks);
size_t sparsify_batch_desc_bytes(int L);
uint64_t sparsify_batch_layout(int L, const uint64_t *n, const uint64_t *k, void *desc_host);
hipError_t launch_sparsify_batch(const LaunchEnv &env, int L, uint64_t n_blocks, const void *x, bool is_f64, void *residual, uint32_t *loc, void *vals,
                                 void *ws);
// The same over caller-owned layers in their own dtypes (flashe_sparsify_tensors_dev): the caller fills the host tables with
// sparsify_tensors_layout (sorted by compute class; -> blocks), copies their sparsify_tensors_desc_bytes(L) bytes to the START of a device
// workspace of sparsify_tensors_workspace_bytes(L, blocks), then launches; packed (may be null) receives `_to_bytes(loc, bits)`.
size_t sparsify_tensors_workspace_bytes(int L, uint64_t n_blocks);
size_t sparsify_tensors_desc_bytes(int L);
uint64_t sparsify_tensors_layout(int L, const void *const *x, const int *dtype, const uint64_t *n, const uint64_t *k, const uint64_t *koff,
                                 const uint64_t *start, const uint64_t *roff, const uint64_t *voff, void *desc_host, int *n_f32_layers,
                                 uint64_t *n_f32_blocks);
hipError_t launch_sparsify_tensors(const LaunchEnv &env, int L, int L32, uint64_t n_blocks, uint64_t nb32, void *residual, uint32_t *loc, void *vals,
                                   uint64_t total_k, int bits, uint64_t *packed, void *ws);
// The same for C clients of one model at once (flashe_sparsify_cohort_tensors_dev): `rows` = C x L table rows laid out with
// sparsify_tensors_layout (row c L + l = client c's layer l; koff / roff / voff inside client c's equal-stride block), then
// `_to_bytes(loc_c, bits)` of every client's K locations in one launch (packed: C blocks of packed_stride limbs; may be null).
hipError_t launch_sparsify_cohort(const LaunchEnv &env, int C, int rows, int rows32, uint64_t n_blocks, uint64_t nb32, void *residual, uint32_t *loc,
                                  uint64_t loc_stride, void *vals, uint64_t K, int bits, uint64_t *packed, uint64_t packed_stride, void *ws);
// Top-k sparsifier; ws = device workspace of sparsify_workspace_bytes(n).
size_t sparsify_workspace_bytes(uint64_t n);
hipError_t launch_sparsify(const LaunchEnv &env, uint64_t n, uint64_t k, const void *x, bool is_f64, void *residual, uint32_t *loc,
                           void *vals, void *ws);

// Device KAT: encrypts `nblk` 16-byte blocks (big-endian words in) with the PRF core.
hipError_t launch_aes_blocks(const LaunchEnv &env, uint32_t nblk, const uint32_t *in_words_dev,
                             uint32_t *out_words_dev);

// b > 64, one add and at most one minus prefix, C <= kMaxOps operands ANYWHERE in HBM (pointers address element `first`): out = sum of the
// operands + term(add) - term(minus) on [first, first + count) in ONE launch; agg_out_dev (may be null) receives the sum.
// hipErrorNotSupported (nothing launched): b <= 64, too many operands, a range across a 2^32 counter boundary, another PRF backend.
hipError_t launch_reduce_decrypt_ptrs(const LaunchEnv &env, uint32_t iter, uint32_t add_idx, bool has_minus, uint32_t minus_idx, uint64_t first,
                                      uint64_t count, int C, const uint64_t *const *ops, uint64_t *agg_out_dev, uint64_t *out_dev);
#ifdef FLASHE_TUNING
// tuning build only: the two-workgroups-per-CU experiment on the reduce fused with the decrypt (kernels.hip); variant 0 = 1024 threads,
// full tables (correct results); 1 = 2 x 512 threads on half-size aliased tables (timing probe, wrong results); 2 = 1024 threads on them
hipError_t launch_reduce_decrypt_probe(const LaunchEnv &env, int variant, uint32_t iter, uint32_t add_idx, uint32_t minus_idx, int C,
                                       const uint64_t *const *ops, uint64_t n, uint64_t *out_dev);
#endif

}  // namespace flashe
