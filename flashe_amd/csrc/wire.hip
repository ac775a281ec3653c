// The dense client step straight to and from the packed WIRE form at int_bits 16 .. 64 (JZFTransferableWeights.compress / decompress,
// jzf_weights.py:155-231: element j of n at bits [b (n - 1 - j), b (n - j)) of one integer, element 0 most significant):
//   prf_small_pack_kernel<DBL>   float model + draws -> quantise -> encrypt -> packed limbs       (no uint64 ciphertext vector in HBM)
//   prf_small_unpack_kernel      packed limbs of the sum -> decrypt -> unquantise -> float64 model (no uint64 element vector in HBM)
//   prf_small_pack_cohort_kernel  the single-mask pack for the C clients of a SPARSE cohort, 'zzz' fields included (stated at the kernel)
//   prf_small_unpack_lists_kernel  the same with prefix LISTS of up to kMaxIdx each (a dropout, the single mask's decrypt; wire_lists.h)
// Both are siblings of prf_small_jobs_kernel (kernels.hip): a wave owns 64 consecutive AES blocks per tile, counters and chunking by
// small_block_params, prefixes through ctr_prefix / ctr_round1, the T-tables in LDS.  The structural fact they rest on: a lane's AES block
// masks m = 128 / b CONSECUTIVE elements, and consecutive elements are one CONTIGUOUS cnt * b-bit field of the packed integer with the
// slot order reversed -- so the lane that computes a block holds its whole piece of the wire integer in registers, and only neighbouring
// lanes' fields have to be stitched into 64-bit limbs.
//   pack: the lane quantises its block's values itself (plaintext slots built in wire order), adds the reversed mask slots (SWAR), writes
//   the field to its 16-byte LDS row in DESCENDING lane order (ascending LDS address = ascending bit position) and the wave emits the
//   tile's limbs lane-contiguously, one coalesced 8-byte store per lane: limb w ORs the one or two fields that overlap it.  The first and
//   the last limb of a tile are in general shared with the neighbouring tile: those go out with a 64-bit atomic OR into the output the
//   launcher zeroed on the stream beforehand.
//   unpack: the lane loads the two or three limbs its field overlaps (neighbouring lanes read neighbouring limbs: the tile is one
//   contiguous run of at most 129 limbs -- one more than the wave's rows hold, which is why they are not staged), decrypts the slots,
//   writes them to its row, and the wave walks its 64 m elements lane-contiguously as small_walk does: unquantise, coalesced float64 stores.
// RAGGED tiles -- a tile with a partial block (a chunk end with cnt < m; at most one tile per chunk) -- take a per-lane path: every valid
// lane ORs its own field into the at most three limbs it touches, atomically (pack), or stores its own cnt floats (unpack).
#include "small_blocks.h"
#include "wire_lists.h"
#include "wire_tiles.h"

namespace flashe {

namespace {

// per b-bit slot (a - c) / (a + c) mod 2^b of two 128-bit words (SWAR: borrows / carries must not cross slots); bits above the last slot: garbage
__device__ __forceinline__ u128 wire_slot_sub(u128 a, u128 c, u128 top) { return ((a | top) - (c & ~top)) ^ ((a ^ ~c) & top); }
__device__ __forceinline__ u128 wire_slot_add(u128 a, u128 c, u128 top) { return ((a & ~top) + (c & ~top)) ^ ((a ^ c) & top); }

// slots 0 .. cnt - 1 of v (slot t at bit b t) in the opposite order: slot t at bit b (cnt - 1 - t); its own inverse.  The result is cnt b bits wide.
__device__ __forceinline__ u128 wire_reverse(u128 v, int cnt, int b, uint64_t mask)
{
    u128 f = 0;
#pragma unroll 1
    for (int t = 0; t < cnt; t++) {
        f = (f << b) | (static_cast<uint64_t>(v) & mask);
        v >>= b;
    }
    return f;
}

// The M plaintexts of a WHOLE block inside one table row, for the lane that owns it (the front end the compact cohort kernels call
// CohortDirect): 4 M or 8 M bytes of the model and 8 M of draws in 16-byte accesses, quantised with the row's parameters from SGPRs,
// packed in WIRE order -- value t at bit b (M - 1 - t) -- so that nothing but one 128-bit word lives through the AES rounds.
template <int M>
__device__ __forceinline__ u128 wire_front(const void *xs, bool f64, double p0, double p1, double p2, const double *u, uint64_t r, int b, uint64_t mask)
{
    uint64_t ub[M], q[M];
    cohort_load_run<M>(reinterpret_cast<const uint64_t *>(u), ub);
    if (f64) {
        uint64_t raw[M];
        cohort_load_run<M>(static_cast<const uint64_t *>(xs) + r, raw);
#pragma unroll
        for (int t = 0; t < M; t++) q[t] = cohort_quantize_raw(raw[t], true, p0, p1, p2, __longlong_as_double(static_cast<long long>(ub[t])));
    } else {
        uint32_t raw[M];
        cohort_load_run<M>(static_cast<const uint32_t *>(xs) + r, raw);
#pragma unroll
        for (int t = 0; t < M; t++) q[t] = cohort_quantize_raw(raw[t], false, p0, p1, p2, __longlong_as_double(static_cast<long long>(ub[t])));
    }
    u128 x = 0;
#pragma unroll
    for (int t = 0; t < M; t++) x = (x << b) | (q[t] & mask);
    return x;
}

// the same with M = m at run time (2 .. 8)
__device__ __forceinline__ u128 wire_front_m(uint32_t m, const void *xs, bool f64, double p0, double p1, double p2, const double *u, uint64_t r, int b, uint64_t mask)
{
    switch (m) {
    case 2: return wire_front<2>(xs, f64, p0, p1, p2, u, r, b, mask);
    case 3: return wire_front<3>(xs, f64, p0, p1, p2, u, r, b, mask);
    case 4: return wire_front<4>(xs, f64, p0, p1, p2, u, r, b, mask);
    case 5: return wire_front<5>(xs, f64, p0, p1, p2, u, r, b, mask);
    case 6: return wire_front<6>(xs, f64, p0, p1, p2, u, r, b, mask);
    case 7: return wire_front<7>(xs, f64, p0, p1, p2, u, r, b, mask);
    default: return wire_front<8>(xs, f64, p0, p1, p2, u, r, b, mask);
    }
}

struct WireTile {
    uint64_t j0;          // the lane's block: first element, elements, counter
    int cnt;
    uint32_t ctr;
    bool valid, ragged;   // ragged: wave-uniform
    int n_valid;          // wave-uniform
    uint64_t e0;          // the tile's first element (wave-uniform)
};

struct WireChunks { uint32_t nb1, nb0, d, r; };

__device__ __forceinline__ WireChunks wire_chunks(const SmallParams &p)
{
    const uint64_t J = p.n_jobs, d = p.n / J, r = p.n % J, m = static_cast<uint64_t>(p.m);
    return WireChunks{static_cast<uint32_t>((d + 1 + m - 1) / m), static_cast<uint32_t>(d ? (d + m - 1) / m : 0), static_cast<uint32_t>(d), static_cast<uint32_t>(r)};
}

// tile t of the vector: blocks 64 t .. 64 t + 63 of its n_blocks (lane L owns block 64 t + L)
__device__ __forceinline__ WireTile wire_tile(const SmallParams &p, const WireChunks &c, uint64_t t, uint64_t n_blocks, uint32_t lane)
{
    WireTile w;
    const uint64_t B = t * 64u + lane;
    w.valid = B < n_blocks;
    small_block_params(static_cast<uint32_t>(w.valid ? B : t * 64u), c.nb1, c.nb0, c.d, c.r, static_cast<uint32_t>(p.m), p, &w.j0, &w.cnt, &w.ctr);
    w.ragged = __ballot(w.valid && w.cnt < p.m) != 0;
    w.n_valid = __popcll(__ballot(w.valid));
    const uint32_t j0_lo = static_cast<uint32_t>(w.j0), j0_hi = static_cast<uint32_t>(w.j0 >> 32);
    w.e0 = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(j0_lo)) | (static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(j0_hi))) << 32);
    return w;
}

__device__ __forceinline__ void wire_or(uint64_t *p, uint64_t v)
{
    if (v) atomicOr(reinterpret_cast<unsigned long long *>(p), static_cast<unsigned long long>(v));
}

// The stitch of a tile's fields F (the lane's block: cnt b bits, masked) into the limbs of an integer of n_fields fields, element j at bits
// [b (n_fields - 1 - j), b (n_fields - j)): the block of elements [j0, j0 + cnt) is the field at bit b (n_fields - j0 - cnt).  n_fields = n
// for the dense vector; K + 1 for a sparse upload, whose trailing 'zzz' field lifts every ciphertext field b bits.  packed: the integer's
// n_limbs limbs, the shared ones ZERO on entry.  A ragged tile: every valid lane ORs its field into the at most three limbs it touches.
// Otherwise the fields go to the wave's 16-byte rows row0 in DESCENDING lane order and lane i emits limb i (and i + 64) of the tile.
__device__ __forceinline__ void wire_stitch(const WireTile &w, u128 F, uint32_t lane, uint32_t *row0, uint32_t b, uint32_t m, uint32_t w_magic, uint64_t n_fields,
                                            uint64_t *__restrict__ packed, uint64_t n_limbs)
{
    const uint32_t W = m * b;
    if (w.ragged) {
        if (w.valid) {
            const uint64_t pos = static_cast<uint64_t>(b) * (n_fields - w.j0 - static_cast<uint64_t>(w.cnt));
            const uint64_t l = pos >> 6;
            const uint32_t sh = static_cast<uint32_t>(pos) & 63u;
            wire_or(packed + l, static_cast<uint64_t>(F) << sh);
            if (l + 1 < n_limbs) wire_or(packed + l + 1, sh ? static_cast<uint64_t>(F >> (64u - sh)) : static_cast<uint64_t>(F >> 64));
            if (l + 2 < n_limbs && sh) wire_or(packed + l + 2, static_cast<uint64_t>(F >> (128u - sh)));
        }
        return;
    }
    // 5. the fields of the n_valid whole blocks, descending lane order: row r holds bits [lo_bit + r W, + W) of the integer
    const uint32_t nv = static_cast<uint32_t>(w.n_valid);
    if (w.valid) {
        uint32_t *q = row0 + 4 * (nv - 1u - lane);
        *reinterpret_cast<uint4 *>(q) = make_uint4(static_cast<uint32_t>(F), static_cast<uint32_t>(F >> 32), static_cast<uint32_t>(F >> 64), static_cast<uint32_t>(F >> 96));
    }
    __builtin_amdgcn_wave_barrier();
    // 6. + 7. limb l0 + i covers bits [64 i - off, 64 i - off + 64) of the tile's `span` bits
    const uint64_t lo_bit = static_cast<uint64_t>(b) * (n_fields - w.e0 - static_cast<uint64_t>(nv) * m);
    const uint64_t l0 = lo_bit >> 6;
    const uint32_t off = static_cast<uint32_t>(lo_bit) & 63u, span = nv * W, tile_limbs = (off + span + 63u) >> 6;       // at most 129
    for (uint32_t i = lane; i < tile_limbs; i += 64u) {
        const int q = static_cast<int>(64u * i) - static_cast<int>(off);
        const uint32_t q_lo = q < 0 ? 0u : static_cast<uint32_t>(q), q_hi = static_cast<uint32_t>(q + 63) < span ? static_cast<uint32_t>(q + 63) : span - 1u;
        const uint32_t r_lo = static_cast<uint32_t>((static_cast<uint64_t>(q_lo) * w_magic) >> 32), r_hi = static_cast<uint32_t>((static_cast<uint64_t>(q_hi) * w_magic) >> 32);
        const uint4 a = *reinterpret_cast<const uint4 *>(row0 + 4 * r_lo);
        const u128 Fa = (static_cast<u128>((static_cast<uint64_t>(a.w) << 32) | a.z) << 64) | ((static_cast<uint64_t>(a.y) << 32) | a.x);
        const int sa = static_cast<int>(r_lo * W) - q;                    // where field r_lo starts, relative to the limb: -(W - 1) .. 63
        uint64_t val = sa >= 0 ? static_cast<uint64_t>(Fa) << sa : static_cast<uint64_t>(Fa >> -sa);
        if (r_hi != r_lo) {                                             // W >= 64: at most one more field, starting inside the limb
            const uint2 c = *reinterpret_cast<const uint2 *>(row0 + 4 * r_hi);
            val |= ((static_cast<uint64_t>(c.y) << 32) | c.x) << (static_cast<int>(r_hi * W) - q);
        }
        if (q >= 0 && static_cast<uint32_t>(q) + 64u <= span) __builtin_nontemporal_store(val, packed + l0 + i);
        else wire_or(packed + l0 + i, val);                             // shared with the neighbouring tile (or the integer's top limb)
    }
    __builtin_amdgcn_wave_barrier();
}

}  // namespace

// packed: n_limbs = ceil(n b / 64) limbs, ZERO on entry (the launcher clears them on the stream); w_magic = ceil(2^32 / (m b))
template <bool DBL>
__global__ __launch_bounds__(kSmallThreads) void prf_small_pack_kernel(const RoundKeys rk, const SmallParams p, uint32_t add_idx, uint32_t minus_idx,
                                                                       uint64_t n_blocks, uint32_t w_magic, uint64_t *__restrict__ packed, uint64_t n_limbs)
{
    const uint32_t iter = p.iter + p.te0[kIterShiftWord];
    __shared__ uint32_t tab[kTabWords];
    __shared__ uint32_t scratch[(kSmallThreads / 64) * 256 + 8];
    fill_tables(tab, p.te0);
    const LaneRegs lr = lane_regs(tab);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
    uint32_t *row0 = scratch + wave * 256;
    const u128 top = (static_cast<u128>(p.top_hi) << 64) | p.top_lo;
    const WireChunks ch = wire_chunks(p);
    const uint32_t b = static_cast<uint32_t>(p.b), m = static_cast<uint32_t>(p.m);
    const CtrPrefix pre_a = scalar_prefix(ctr_prefix(rk, lr, iter, add_idx, 0u));            // n < 2^32 (host-checked): the high counter word is 0
    CtrPrefix pre_b{};
    if (DBL) pre_b = scalar_prefix(ctr_prefix(rk, lr, iter, minus_idx, 0u));
    const uint64_t n_tiles = (n_blocks + 63) / 64, n_waves = static_cast<uint64_t>(gridDim.x) * (kSmallThreads / 64);
    for (uint64_t t = static_cast<uint64_t>(blockIdx.x) * (kSmallThreads / 64) + wave; t < n_tiles; t += n_waves) {
        const WireTile w = wire_tile(p, ch, t, n_blocks, lane);
        // 1. the plaintexts of the lane's block in wire order, before the AES rounds: only P lives through them
        const int row = w.ragged ? -1 : wire_tile_row(p.cq, w.e0, w.e0 + static_cast<uint64_t>(w.n_valid) * m, p.n);
        u128 P = 0;
        if (row >= 0) {
            const CodecLayer *L = p.cq.layers + row;
            const uint64_t ls = *FLASHE_CONSTANT(const uint64_t, &L->start);
            const void *const xs = reinterpret_cast<const void *>(*FLASHE_CONSTANT(const uintptr_t, &L->x));
            const bool f64 = *FLASHE_CONSTANT(const int, &L->x_is_f64) != 0;
            const double p0 = *FLASHE_CONSTANT(const double, &L->p0), p1 = *FLASHE_CONSTANT(const double, &L->p1), p2 = *FLASHE_CONSTANT(const double, &L->p2);
            if (w.valid) {
                const double *u = p.cq.u + w.j0;
                const uint64_t r = p.cq.k0 + w.j0 - ls;
                P = wire_front_m(m, xs, f64, p0, p1, p2, u, r, p.b, p.mask_lo);
            }
        } else if (w.valid) {
            // a partial block, or a tile that straddles a table row: value by value, the row looked up per lane
#pragma unroll 1
            for (int tt = 0; tt < w.cnt; tt++) P = (P << b) | (codec_quantize(p.cq, w.j0 + tt) & p.mask_lo);
        }
        // 2. D = S_add (- S_minus) slot-wise
        uint32_t s[DBL ? 2 : 1][4];
        const CtrVar x = ctr_var(rk, lr, w.ctr);
        ctr_round1(pre_a, x, s[0]);
        if (DBL) ctr_round1(pre_b, x, s[DBL ? 1 : 0]);
        aes256_rounds<DBL ? 2 : 1, 2>(rk, lr, s, true);
        u128 D = words_to_u128(s[0]);
        if (DBL) D = wire_slot_sub(D, words_to_u128(s[DBL ? 1 : 0]), top);
        // 3. + 4. the mask slots in wire order, added to the plaintext slots mod 2^b: the block's cnt b-bit field of the packed integer
        const uint32_t fbits = static_cast<uint32_t>(w.cnt) * b;
        u128 F = wire_slot_add(P, wire_reverse(D, w.cnt, p.b, p.mask_lo), top);
        if (fbits < 128u) F &= (static_cast<u128>(1) << fbits) - 1;
        wire_stitch(w, F, lane, row0, b, m, w_magic, p.n, packed, n_limbs);
    }
}

// ---- a sparse COHORT's uploads straight to the packed wire form (flashe_quantize_encrypt_pack_sparse_cohort_dev) ----
// prf_small_pack_kernel<false> for the C clients of a sparse cohort in ONE launch: upload c = the K single-mask ciphertexts (cipher index
// idx[c], chunking and counters over K) of client c's quantised compact values followed by its plain quantised 'zzz' value, K + 1 fields
// in the wire layout -- the 'zzz' field is bits [0, b) of limb 0 and every ciphertext field lies b bits above its place in a dense pack
// of K elements, which is all wire_stitch has to know (n_fields = K + 1).  Per value and client 4 + 8 bytes read and b / 8 written (plus
// b / 8 for the clearing), against 4 + 8 read, 8 written, 8 read and b / 8 written through the one-limb uploads and C pack launches.
//   the split: the launch deals (client, tile) ITEMS, C x ceil(blocks / 64) of them, one wave per item, the waves striding over the items
//   -- a compact vector with fewer tiles than the chip has waves still reaches every wave, as launch_small_sparse_cohort's cut does.
//   The order is CLIENT-major (item = c n_tiles + t): the 16 waves of a workgroup then take 16 consecutive tiles of ONE client -- one
//   contiguous run of its floats, of its draws and of its limbs, and the limb two neighbouring tiles share is OR-ed by waves of the same
//   workgroup, back to back -- and a wave's prefix row and source pointers change only when its client does.
//   Tile-major would share the table row among a workgroup's waves, but that row is a handful of scalar loads, and it would spread
//   every workgroup's loads and stores over C allocations' worth of DRAM pages at once.
//   the prefixes: the workgroup builds the C round-1 states once in the LDS table of wire_lists.h (the iter shift of a graph replay is
//   only known here); an item takes its row to SGPRs.  Up to 2 kMaxIdx = 192 clients, what the table holds.
//   the front end: the lane that owns a block quantises its m values of client c before the AES rounds -- a tile inside one row of the
//   shared compact-layer table takes the row's parameters and client c's source pointer from SGPRs (wire_front), a ragged tile or one that
//   straddles rows goes value by value (cohort_quantize_lane) -- in wire order, so one 128-bit word lives through the rounds.
//   the 'zzz' values: the first C lanes of workgroup 0 quantise them (SparseCohortTail's arithmetic, the draw behind the client's K),
//   store zeros[c] and OR the field into limb 0 of upload c.
// The uploads lie `stride` limbs apart in ONE allocation, so the launcher clears them with one fill whatever C is.
struct PackCohort {
    WireLists ids;             // idx[0 .. n): the clients' cipher indices (n_add = 0)
    const void *const *src;    // CohortCodec's sources: src[c * n_layers + row]
    const double *u;           // client c's K + 1 draws at u + c * u_stride, the last one its 'zzz' draw
    uint64_t u_stride;
    uint64_t *packed;          // upload c: the n_limbs limbs at packed + c * stride
    uint64_t stride, n_limbs;
    const double *zzz;         // device: the C 'zzz' values
    uint64_t *zeros;           // device: receives the C quantised values
    double z_alpha, z_scale, z_den;
    int z_f64, pad_;
};

// p: the constants of a K-vector (p.n = K), p.cq.layers / n_layers = the shared table (k0 = 0); every upload's limbs ZERO on entry
__global__ __launch_bounds__(kSmallThreads) void prf_small_pack_cohort_kernel(const RoundKeys rk, const SmallParams p, const PackCohort pc, uint64_t n_blocks,
                                                                              uint32_t w_magic)
{
    const uint32_t iter = p.iter + p.te0[kIterShiftWord];
    __shared__ uint32_t tab[kTabWords];
    __shared__ uint32_t scratch[(kSmallThreads / 64) * 256 + 8];
    __shared__ uint4 pre[2 * kMaxIdx];
    fill_tables(tab, p.te0);
    const LaneRegs lr = lane_regs(tab);
    wire_prefix_table(rk, lr, iter, pc.ids, pre);
    const uint32_t C = static_cast<uint32_t>(pc.ids.n);
    if (blockIdx.x == 0 && threadIdx.x < C) {
        const uint32_t c = threadIdx.x;
        const double v = pc.zzz[c], u = pc.u[static_cast<uint64_t>(c) * pc.u_stride + p.n];
        const uint64_t q = pc.z_f64 ? quantize_one<double>(v, pc.z_alpha, pc.z_scale, pc.z_den, u)
                                    : quantize_one<float>(static_cast<float>(v), static_cast<float>(pc.z_alpha), static_cast<float>(pc.z_scale),
                                                          static_cast<float>(pc.z_den), u);
        pc.zeros[c] = q;
        wire_or(pc.packed + static_cast<uint64_t>(c) * pc.stride, q & p.mask_lo);
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
    uint32_t *row0 = scratch + wave * 256;
    const u128 top = (static_cast<u128>(p.top_hi) << 64) | p.top_lo;
    const WireChunks ch = wire_chunks(p);
    const uint32_t b = static_cast<uint32_t>(p.b), m = static_cast<uint32_t>(p.m);
    const CohortCodec cc{p.cq.layers, pc.src, p.cq.n_layers, 0};
    // item = c n_tiles + t, walked without a division per item (n_tiles <= 2^26, the grid's waves <= 2^12)
    const uint32_t n_tiles = static_cast<uint32_t>((n_blocks + 63) / 64), n_waves = gridDim.x * (kSmallThreads / 64);
    const uint32_t first = blockIdx.x * (kSmallThreads / 64) + wave, step_c = n_waves / n_tiles, step_t = n_waves % n_tiles;
    uint32_t c = first / n_tiles, t = first % n_tiles;
    while (c < C) {
        const WireTile w = wire_tile(p, ch, t, n_blocks, lane);
        const CtrPrefix pre_c = wire_prefix_row(pre, static_cast<int>(c));
        const double *const u = pc.u + static_cast<uint64_t>(c) * pc.u_stride;
        // 1. client c's plaintexts of the lane's block in wire order, before the AES rounds
        const int row = w.ragged ? -1 : wire_tile_row(p.cq, w.e0, w.e0 + static_cast<uint64_t>(w.n_valid) * m, p.n);
        u128 P = 0;
        if (row >= 0) {
            const CodecLayer *L = p.cq.layers + row;
            const uint64_t ls = *FLASHE_CONSTANT(const uint64_t, &L->start);
            const void *const xs = reinterpret_cast<const void *>(*FLASHE_CONSTANT(const uintptr_t, pc.src + static_cast<uint64_t>(c) * cc.n_layers + row));
            const bool f64 = *FLASHE_CONSTANT(const int, &L->x_is_f64) != 0;
            const double p0 = *FLASHE_CONSTANT(const double, &L->p0), p1 = *FLASHE_CONSTANT(const double, &L->p1), p2 = *FLASHE_CONSTANT(const double, &L->p2);
            if (w.valid) P = wire_front_m(m, xs, f64, p0, p1, p2, u + w.j0, w.j0 - ls, p.b, p.mask_lo);
        } else if (w.valid) {
#pragma unroll 1
            for (int tt = 0; tt < w.cnt; tt++) P = (P << b) | (cohort_quantize_lane(cc, static_cast<int>(c), w.j0 + tt, u[w.j0 + tt]) & p.mask_lo);
        }
        // 2. the single mask of idx[c], 3. + 4. the block's field
        uint32_t s[1][4];
        ctr_round1(pre_c, ctr_var(rk, lr, w.ctr), s[0]);
        aes256_rounds<1, 2>(rk, lr, s, true);
        const uint32_t fbits = static_cast<uint32_t>(w.cnt) * b;
        u128 F = wire_slot_add(P, wire_reverse(words_to_u128(s[0]), w.cnt, p.b, p.mask_lo), top);
        if (fbits < 128u) F &= (static_cast<u128>(1) << fbits) - 1;
        wire_stitch(w, F, lane, row0, b, m, w_magic, p.n + 1, pc.packed + static_cast<uint64_t>(c) * pc.stride, pc.n_limbs);
        c += step_c; t += step_t;
        if (t >= n_tiles) { t -= n_tiles; c++; }
    }
}

// The way back, shared by the one-prefix and the lists kernel: mid(x, top) = the lane's slot-wise mask S_add - S_minus at counter part x.
template <class Mid>
__device__ __forceinline__ void small_unpack_tiles(const RoundKeys &rk, const SmallParams &p, const LaneRegs lr, uint32_t *scratch, const Mid &mid, uint64_t n_blocks,
                                                   const uint64_t *__restrict__ packed, uint64_t n_limbs)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
    uint32_t *row0 = scratch + wave * 256;
    const u128 top = (static_cast<u128>(p.top_hi) << 64) | p.top_lo;
    const WireChunks ch = wire_chunks(p);
    const uint32_t b = static_cast<uint32_t>(p.b), m = static_cast<uint32_t>(p.m);
    double *const out = p.cq.fout;
    const uint64_t n_tiles = (n_blocks + 63) / 64, n_waves = static_cast<uint64_t>(gridDim.x) * (kSmallThreads / 64);
    for (uint64_t t = static_cast<uint64_t>(blockIdx.x) * (kSmallThreads / 64) + wave; t < n_tiles; t += n_waves) {
        const WireTile w = wire_tile(p, ch, t, n_blocks, lane);
        // 1. the two or three limbs the lane's field overlaps, requested before the AES rounds
        const uint64_t pos = static_cast<uint64_t>(b) * (p.n - w.j0 - static_cast<uint64_t>(w.cnt));
        const uint64_t l = pos >> 6;
        const uint32_t sh = static_cast<uint32_t>(pos) & 63u, fbits = static_cast<uint32_t>(w.cnt) * b;
        uint64_t g0 = 0, g1 = 0, g2 = 0;
        if (w.valid) {
            g0 = __builtin_nontemporal_load(packed + l);
            if (l + 1 < n_limbs && sh + fbits > 64u) g1 = __builtin_nontemporal_load(packed + l + 1);
            if (l + 2 < n_limbs && sh + fbits > 128u) g2 = __builtin_nontemporal_load(packed + l + 2);
        }
        // 2. the prefixes the host's telescoping left
        const u128 D = mid(ctr_var(rk, lr, w.ctr), top);
        u128 F = (static_cast<u128>(g1) << 64) | g0;
        if (sh) F = (F >> sh) | (static_cast<u128>(g2) << (128u - sh));
        if (fbits < 128u) F &= (static_cast<u128>(1) << fbits) - 1;
        const u128 X = wire_slot_add(wire_reverse(F, w.cnt, p.b, p.mask_lo), D, top);        // slot t = element j0 + t, decrypted
        if (w.ragged) {
            if (w.valid)
#pragma unroll 1
                for (int tt = 0; tt < w.cnt; tt++)
                    out[w.j0 + tt] = codec_unquantize(p.cq, w.j0 + tt, static_cast<uint64_t>(X >> (p.b * tt)) & p.mask_lo);
            continue;
        }
        // 3. + 4. the decrypted slots through the lane's row; the wave walks its n_valid m elements lane-contiguously
        *reinterpret_cast<uint4 *>(row0 + 4 * lane) = make_uint4(static_cast<uint32_t>(X), static_cast<uint32_t>(X >> 32), static_cast<uint32_t>(X >> 64), static_cast<uint32_t>(X >> 96));
        __builtin_amdgcn_wave_barrier();
        const uint32_t n_elems = static_cast<uint32_t>(w.n_valid) * m;
        const int row = wire_tile_row(p.cq, w.e0, w.e0 + n_elems, p.n);
        double p0 = 0, p1 = 0, p2 = 0;
        if (row >= 0) {
            const CodecLayer *L = p.cq.layers + row;
            p0 = *FLASHE_CONSTANT(const double, &L->p0); p1 = *FLASHE_CONSTANT(const double, &L->p1); p2 = *FLASHE_CONSTANT(const double, &L->p2);
        }
        for (uint32_t e = lane; e < n_elems; e += 64u) {
            const uint32_t blk = static_cast<uint32_t>((static_cast<uint64_t>(e) * p.m_magic) >> 32);
            const uint32_t o = b * (e - blk * m);
            const uint32_t *q = row0 + 4 * blk + (o >> 5);
            const uint32_t s5 = o & 31u;
            uint64_t val = ((static_cast<uint64_t>(q[1]) << 32) | q[0]) >> s5;
            if (s5) val |= static_cast<uint64_t>(q[2]) << (64u - s5);
            val &= p.mask_lo;
            double r;
            if (row >= 0) {
#pragma clang fp contract(off)
                r = u128_to_double(val) * p1 / p2 - p0;                     // codec_unquantize's arithmetic on the row's parameters from SGPRs
            } else {
                r = codec_unquantize(p.cq, w.e0 + e, val);
            }
            __builtin_nontemporal_store(r, out + w.e0 + e);
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// out[j] = unquantise((element j of the packed sum + S_add - S_minus) mod 2^b); flags: bit 0 = an add prefix, bit 1 = a minus prefix
__global__ __launch_bounds__(kSmallThreads) void prf_small_unpack_kernel(const RoundKeys rk, const SmallParams p, uint32_t add_idx, uint32_t minus_idx, int flags,
                                                                         uint64_t n_blocks, const uint64_t *__restrict__ packed, uint64_t n_limbs)
{
    const uint32_t iter = p.iter + p.te0[kIterShiftWord];
    __shared__ uint32_t tab[kTabWords];
    __shared__ uint32_t scratch[(kSmallThreads / 64) * 256 + 8];
    fill_tables(tab, p.te0);
    const LaneRegs lr = lane_regs(tab);
    const bool has_add = (flags & 1) != 0, has_minus = (flags & 2) != 0;
    const CtrPrefix pre_a = scalar_prefix(ctr_prefix(rk, lr, iter, has_add ? add_idx : minus_idx, 0u));        // n < 2^32 (host-checked)
    const CtrPrefix pre_b = scalar_prefix(ctr_prefix(rk, lr, iter, minus_idx, 0u));
    small_unpack_tiles(rk, p, lr, scratch, [&](const CtrVar &x, u128 top) {
        if (has_add && has_minus) {
            uint32_t s[2][4];
            ctr_round1(pre_a, x, s[0]);
            ctr_round1(pre_b, x, s[1]);
            aes256_rounds<2, 2>(rk, lr, s, true);
            return wire_slot_sub(words_to_u128(s[0]), words_to_u128(s[1]), top);
        }
        uint32_t s[1][4];
        ctr_round1(pre_a, x, s[0]);
        aes256_rounds<1, 2>(rk, lr, s, true);
        const u128 D = words_to_u128(s[0]);
        return has_add ? D : wire_slot_sub(0, D, top);
    }, n_blocks, packed, n_limbs);
}

// The same with prefix LISTS (a round with a dropout, the single mask's decrypt): out[j] = unquantise((element j of the packed sum +
// sum_k S(add[k]) - sum_k S(minus[k])) mod 2^b), the prefixes' round-1 states in an LDS table the kernel builds (wire_lists.h).  The
// running mask is kept slot-wise (SWAR under `top`): no carry or borrow of one prefix's block crosses into the next slot.
__global__ __launch_bounds__(kSmallThreads) void prf_small_unpack_lists_kernel(const RoundKeys rk, const SmallParams p, const WireLists ls, uint64_t n_blocks,
                                                                               const uint64_t *__restrict__ packed, uint64_t n_limbs)
{
    const uint32_t iter = p.iter + p.te0[kIterShiftWord];
    __shared__ uint32_t tab[kTabWords];
    __shared__ uint32_t scratch[(kSmallThreads / 64) * 256 + 8];
    __shared__ uint4 pre[2 * kMaxIdx];
    fill_tables(tab, p.te0);
    const LaneRegs lr = lane_regs(tab);
    wire_prefix_table(rk, lr, iter, ls, pre);
    small_unpack_tiles(rk, p, lr, scratch, [&](const CtrVar &x, u128 top) {
        return wire_lists_mask<false>(rk, lr, pre, ls.n_add, ls.n, x,
                                      [top](u128 D, u128 S, bool add) { return add ? wire_slot_add(D, S, top) : wire_slot_sub(D, S, top); });
    }, n_blocks, packed, n_limbs);
}

bool small_wire_admits(const LaunchEnv &env, uint64_t n, uint32_t n_jobs)
{
    return env.b >= 16 && env.b <= 64 && n >= 1 && n < (1ull << 32) && n_jobs >= 1 && (env.prf_backend == PRF_AUTO || env.prf_backend == PRF_TABLE);
}

static int wire_grid(const LaunchEnv &env, uint64_t n_blocks)
{
    const uint64_t tiles = (n_blocks + 63) / 64, groups = (tiles + kSmallThreads / 64 - 1) / (kSmallThreads / 64), cus = static_cast<uint64_t>(env.num_cus);
    return static_cast<int>(groups < cus ? groups : cus);
}

hipError_t launch_small_pack(const LaunchEnv &env, uint32_t iter, uint32_t add_idx, bool dbl, uint32_t minus_idx, uint64_t n, uint32_t n_jobs, const Codec &cq,
                             uint64_t *packed_dev)
{
    if (!small_wire_admits(env, n, n_jobs) || !cq.layers || !cq.u) return hipErrorNotSupported;
    SmallParams p = small_params_of(env, iter, n, n_jobs);
    p.cq = cq;
    const uint64_t n_blocks = block_of(n - 1, n, n_jobs, p.m) + 1, n_limbs = (n * static_cast<uint64_t>(env.b) + 63) / 64;
    const uint32_t W = static_cast<uint32_t>(p.m * p.b), w_magic = static_cast<uint32_t>(((1ull << 32) + W - 1) / W);
    // the shared limbs are OR-ed into: the whole buffer is cleared first (b / 8 bytes per value more)
    hipError_t e = launch_fill(env, n_limbs, 0, 0, packed_dev);
    if (e != hipSuccess) return e;
    const dim3 grid(wire_grid(env, n_blocks)), block(kSmallThreads);
    if (dbl) hipLaunchKernelGGL(prf_small_pack_kernel<true>, grid, block, 0, env.stream, env.rk, p, add_idx, minus_idx, n_blocks, w_magic, packed_dev, n_limbs);
    else hipLaunchKernelGGL(prf_small_pack_kernel<false>, grid, block, 0, env.stream, env.rk, p, add_idx, 0u, n_blocks, w_magic, packed_dev, n_limbs);
    return hipGetLastError();
}

bool small_pack_cohort_admits(const LaunchEnv &env, int n_vec, uint64_t n, uint32_t n_jobs)
{
    return small_wire_admits(env, n, n_jobs) && n_vec >= 1 && n_vec <= kMaxPackCohort;
}

hipError_t launch_small_pack_cohort(const LaunchEnv &env, uint32_t iter, int n_vec, const uint32_t *idx, const CohortCodec &cc, const double *u_dev,
                                    uint64_t u_stride, uint64_t n, uint32_t n_jobs, uint64_t *packed_dev, uint64_t packed_stride, const double *zzz_dev,
                                    bool zzz_f64, double z_alpha, double z_scale, double z_den, uint64_t *zeros_dev)
{
    if (!small_pack_cohort_admits(env, n_vec, n, n_jobs) || !cc.layers || !cc.src || cc.n_layers < 1 || !idx || !u_dev || !packed_dev || !zzz_dev || !zeros_dev)
        return hipErrorNotSupported;
    const uint64_t n_limbs = ((n + 1) * static_cast<uint64_t>(env.b) + 63) / 64;
    if (packed_stride < n_limbs || u_stride < n + 1) return hipErrorInvalidValue;
    SmallParams p = small_params_of(env, iter, n, n_jobs);
    p.cq.layers = cc.layers; p.cq.n_layers = cc.n_layers;
    PackCohort pc{};
    for (int c = 0; c < n_vec; c++) pc.ids.idx[c] = idx[c];
    pc.ids.n = n_vec;
    pc.src = cc.src; pc.u = u_dev; pc.u_stride = u_stride;
    pc.packed = packed_dev; pc.stride = packed_stride; pc.n_limbs = n_limbs;
    pc.zzz = zzz_dev; pc.zeros = zeros_dev; pc.z_alpha = z_alpha; pc.z_scale = z_scale; pc.z_den = z_den; pc.z_f64 = zzz_f64 ? 1 : 0;
    const uint64_t n_blocks = block_of(n - 1, n, n_jobs, p.m) + 1;
    const uint32_t W = static_cast<uint32_t>(p.m * p.b), w_magic = static_cast<uint32_t>(((1ull << 32) + W - 1) / W);
    // ONE fill for all uploads, the gaps of the stride included: limbs [0, (C - 1) stride + n_limbs)
    hipError_t e = launch_fill(env, static_cast<uint64_t>(n_vec - 1) * packed_stride + n_limbs, 0, 0, packed_dev);
    if (e != hipSuccess) return e;
    const uint64_t items = (n_blocks + 63) / 64 * static_cast<uint64_t>(n_vec), groups = (items + kSmallThreads / 64 - 1) / (kSmallThreads / 64),
                   cus = static_cast<uint64_t>(env.num_cus);
    hipLaunchKernelGGL(prf_small_pack_cohort_kernel, dim3(static_cast<unsigned>(groups < cus ? groups : cus)), dim3(kSmallThreads), 0, env.stream, env.rk, p, pc,
                       n_blocks, w_magic);
    return hipGetLastError();
}

hipError_t launch_small_unpack(const LaunchEnv &env, uint32_t iter, bool has_add, uint32_t add_idx, bool has_minus, uint32_t minus_idx, uint64_t n,
                               uint32_t n_jobs, const uint64_t *packed_dev, const Codec &cq)
{
    if (!small_wire_admits(env, n, n_jobs) || !cq.layers || !cq.fout || !(has_add || has_minus)) return hipErrorNotSupported;
    SmallParams p = small_params_of(env, iter, n, n_jobs);
    p.cq = cq;
    const uint64_t n_blocks = block_of(n - 1, n, n_jobs, p.m) + 1, n_limbs = (n * static_cast<uint64_t>(env.b) + 63) / 64;
    hipLaunchKernelGGL(prf_small_unpack_kernel, dim3(wire_grid(env, n_blocks)), dim3(kSmallThreads), 0, env.stream, env.rk, p, add_idx, minus_idx,
                       (has_add ? 1 : 0) | (has_minus ? 2 : 0), n_blocks, packed_dev, n_limbs);
    return hipGetLastError();
}

hipError_t launch_small_unpack_lists(const LaunchEnv &env, uint32_t iter, const uint32_t *add, int n_add, const uint32_t *minus, int n_minus, uint64_t n,
                                     uint32_t n_jobs, const uint64_t *packed_dev, const Codec &cq)
{
    if (!small_wire_admits(env, n, n_jobs) || !wire_lists_admit(n_add, n_minus) || !cq.layers || !cq.fout) return hipErrorNotSupported;
    SmallParams p = small_params_of(env, iter, n, n_jobs);
    p.cq = cq;
    const uint64_t n_blocks = block_of(n - 1, n, n_jobs, p.m) + 1, n_limbs = (n * static_cast<uint64_t>(env.b) + 63) / 64;
    hipLaunchKernelGGL(prf_small_unpack_lists_kernel, dim3(wire_grid(env, n_blocks)), dim3(kSmallThreads), 0, env.stream, env.rk, p,
                       wire_lists_of(add, n_add, minus, n_minus), n_blocks, packed_dev, n_limbs);
    return hipGetLastError();
}

}  // namespace flashe
