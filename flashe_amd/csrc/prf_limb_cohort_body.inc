// The body of prf_limb_cohort_kernel<M> and prf_limb_cohort_runs_kernel<M> (kernels.hip), included INSIDE each kernel: the kernel defines M
// and GAPS as compile-time constants and has the arguments rk, tb, p, cc and cg in scope (included text compiles to exactly the kernel it
// was before: prf_chain_body.inc).
// GAPS (prf_limb_cohort_runs_kernel<M>): the cohort's cipher indices form SEVERAL runs -- clients dropped out.  The one chain's streams are
// the cg.n_streams of tb.idx (cohort_streams.h); the output a stream completes is cohort_stream_link(cg, c), a scalar lookup in the kernel's
// arguments at a wave-uniform index, and a stream that completes none (it only opens a run) requests no float and no draw, stores nothing
// and adds nothing to accA / accB or to the walked tiles' memory sums -- its slots become prevA / prevB for the next step.  A completing
// stream's predecessor in the list is stream s - 1, so prevA / prevB mean what they always do, and the first output completed is link 0
// (small_walk's "first link" flag).  Every branch on GAPS is a conditional on the constant: the one-run kernels compile to the code
// objects they were.
    static_assert(M == 2 || M == 3, "int_bits 43 .. 64 or 33 .. 42");
    (void)cg;
    constexpr uint32_t WAVES = kSmallThreads / 64;
    __shared__ uint32_t tab[kTabWords];
    __shared__ uint32_t scratch[WAVES * 256 + 8];
    __shared__ __attribute__((aligned(16))) uint32_t pre_lds[(kMaxLinks + kMaxChains) * 4];
    const uint32_t iter = p.iter + p.te0[kIterShiftWord];
    fill_tables(tab, p.te0);
    const LaneRegs lr = lane_regs(tab);
    const int n_streams = GAPS ? cg.n_streams : tb.len[0] + 1;
    for (int s = threadIdx.x; s < n_streams; s += kSmallThreads) {
        const CtrPrefix c = ctr_prefix(rk, lr, iter, tb.idx[s], 0u);              // n < 2^32 (host-checked): the high counter word is 0
        *reinterpret_cast<uint4 *>(pre_lds + 4 * s) = make_uint4(c.u[0], c.u[1], c.u[2], c.u[3]);
    }
    __syncthreads();
    const uint64_t n = p.n, J = p.n_jobs, d = n / J, r = n % J, blk_count = tb.blk_count[0];
    const uint32_t nb1_32 = static_cast<uint32_t>((d + 1 + M - 1) / M), nb0_32 = static_cast<uint32_t>(d ? (d + M - 1) / M : 0);
    const uint32_t d32 = static_cast<uint32_t>(d), r32 = static_cast<uint32_t>(r);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
    uint32_t *row0 = scratch + wave * 256;
    const u128 top = (static_cast<u128>(p.top_hi) << 64) | p.top_lo;
    uint64_t *const sum = tb.sum_out[0];
    // this workgroup's share of the vector's tiles, dealt to its waves in turn
    const uint64_t T = (blk_count + 127u) / 128u, G = gridDim.x, g = blockIdx.x;
    const uint64_t t_lo = T / G * g + (T % G) * g / G, t_hi = T / G * (g + 1) + (T % G) * (g + 1) / G;
    for (uint64_t q = t_lo + wave; q < t_hi; q += WAVES) {
        const uint64_t Bw = q * 128u;
        const bool vA = Bw + lane < blk_count, vB = Bw + 64u + lane < blk_count;
        uint64_t j0A = 0, j0B = 0;
        int cntA = 0, cntB = 0;
        uint32_t ctrA = 0, ctrB = 0;
        small_block_params(static_cast<uint32_t>(vA ? Bw + lane : 0), nb1_32, nb0_32, d32, r32, M, p, &j0A, &cntA, &ctrA);
        small_block_params(static_cast<uint32_t>(vB ? Bw + 64u + lane : 0), nb1_32, nb0_32, d32, r32, M, p, &j0B, &cntB, &ctrB);
        const CtrVar xA = ctr_var(rk, lr, ctrA), xB = ctr_var(rk, lr, ctrB);
        // a half tile of 64 whole blocks is one contiguous run of 64 M elements; the table row that holds all of it is found once, with
        // scalar loads (CohortDirect).  Every other half -- a chunk end with a partial block, the range end, the last partial tile, a half
        // that straddles a layer row -- walks (small_walk with CohortWalk) and keeps its sums in memory
        const uint64_t e0A = uniform64(j0A), e0B = uniform64(j0B);
        bool fastA = __ballot(vA && cntA == M) == ~0ull && e0A + 64u * M <= n;
        bool fastB = __ballot(vB && cntB == M) == ~0ull && e0B + 64u * M <= n;
        int layA = -1, layB = -1;
        if (fastA) {
            layA = cohort_layer_of(cc, e0A);
            if (layA + 1 < cc.n_layers && *FLASHE_CONSTANT(const uint64_t, &cc.layers[layA + 1].start) < e0A + 64u * M) layA = -1;
        }
        if (fastB) {
            layB = cohort_layer_of(cc, e0B);
            if (layB + 1 < cc.n_layers && *FLASHE_CONSTANT(const uint64_t, &cc.layers[layB + 1].start) < e0B + 64u * M) layB = -1;
        }
        fastA = fastA && layA >= 0;
        fastB = fastB && layB >= 0;
        const CohortDirect csrc{cc, tb.in, 0, {layA, layB}};
        u128 prevA = 0, prevB = 0;
        uint64_t accA[M], accB[M];                                 // the whole blocks' running sums, unmasked: sums mod 2^64 agree with sums mod 2^b
#pragma unroll
        for (int t = 0; t < M; t++) { accA[t] = 0ull; accB[t] = 0ull; }
        for (int c = 0; c < n_streams; c++) {
            const CtrPrefix pre = load_prefix(pre_lds, c);
            const int link = GAPS ? cohort_stream_link(cg, c) : c - 1;             // the output this stream completes
            uint64_t ptA[M], ptB[M];
#pragma unroll
            for (int t = 0; t < M; t++) { ptA[t] = 0ull; ptB[t] = 0ull; }
            if (link >= 0 && fastA) csrc.template words<M>(link, j0A, 0, ptA);
            if (link >= 0 && fastB) csrc.template words<M>(link, j0B, 1, ptB);
            uint32_t s[2][4];
            ctr_round1(pre, xA, s[0]);
            ctr_round1(pre, xB, s[1]);
            aes256_rounds<2, 2>(rk, lr, s, p.swp_prio != 0);
            const u128 SA = words_to_u128(s[0]), SB = words_to_u128(s[1]);
            if (link >= 0) {
                uint64_t *out = tb.out[link];
                const CohortWalk cw{cc, tb.in[link], link};
                if (fastA) {
                    uint64_t v[M];
#pragma unroll
                    for (int t = 0; t < M; t++) {
                        v[t] = ptA[t] + limb_slot(prevA, t, p.b) - limb_slot(SA, t, p.b);
                        accA[t] += v[t];
                    }
                    limb_put<M, true>(out + j0A, v, p.mask_lo);
                } else
                    small_walk(row0, lane, vA, cntA, j0A, slot_diff(prevA, SA, top, p.b), static_cast<const uint64_t *>(nullptr), out, 0, n, p, sum, link == 0, &cw);
                if (fastB) {
                    uint64_t v[M];
#pragma unroll
                    for (int t = 0; t < M; t++) {
                        v[t] = ptB[t] + limb_slot(prevB, t, p.b) - limb_slot(SB, t, p.b);
                        accB[t] += v[t];
                    }
                    limb_put<M, true>(out + j0B, v, p.mask_lo);
                } else
                    small_walk(row0, lane, vB, cntB, j0B, slot_diff(prevB, SB, top, p.b), static_cast<const uint64_t *>(nullptr), out, 0, n, p, sum, link == 0, &cw);
            }
            prevA = SA; prevB = SB;
        }
        if (fastA) limb_put<M, false>(sum + j0A, accA, p.mask_lo);
        if (fastB) limb_put<M, false>(sum + j0B, accB, p.mask_lo);
    }
