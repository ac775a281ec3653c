// The body of prf_small_chain_kernel<PAIR, ET, B> and prf_small_cohort_kernel<B> (kernels.hip), included INSIDE each kernel: the kernel
// defines PAIR, ET, B, COHORT and GAPS as compile-time constants and has the arguments rk, tb, n_chains, p, cc and cg in scope (included text
// compiles to exactly the kernel it was before: prf_chain_body.inc).
// COHORT (PAIR, the compact layout at a compile-time width, one summed double-mask chain over whole vectors): the plaintext of output
// `link` at element k is the quantisation of client link's float k (CohortCodec cc; tb.in[link] = that client's draws) -- whole tiles
// through CohortDirect, the tiles that walk through CohortWalk.
// COHORT with ET = uint64_t (prf_small_sparse_cohort_kernel<B>, the sparse job's cohort): the same front end on SINGLE-mask chains without a
// sum, the outputs in the one-limb layout -- a whole block's M words go out as M uint64 elements (direct32_put's uint64 form).
// GAPS (COHORT with ET = uint32_t only, prf_small_cohort_runs_kernel<B>): the cohort's cipher indices form SEVERAL runs -- clients dropped out.
// The one chain's streams are the cg.n_streams of tb.idx (cohort_streams.h); the output a stream completes is cohort_stream_link(cg, c), a
// scalar lookup in the kernel's arguments at a wave-uniform index, and a stream that completes none (it only opens a run) requests no
// float and no draw, stores nothing and adds nothing to the running sums -- its slots are kept for the next step.  A completing stream's
// predecessor in the list is stream s - 1, so prevA / prevB (psA / psB in small_chain_fast32) mean what they always do.  Every branch on
// GAPS is an `if constexpr` or a conditional on the constant: the other instantiations compile to the code objects they were.
    static_assert(!COHORT || (PAIR && B != 0 && B <= 32), "the cohort front end rides on the paired chain at a compile-time width");
    static_assert(!GAPS || (COHORT && sizeof(ET) == 4), "several runs of indices are a form of the summed compact cohort chain");
    (void)cc;
    (void)cg;
    constexpr bool LIMB_OUT = COHORT && sizeof(ET) == 8;
    static_assert(B == 0 || (PAIR && ((sizeof(ET) == 4 && B <= 32) || (sizeof(ET) == 8 && (B == 64 || LIMB_OUT)))), "compile-time widths: the paired kernel, compact layout or int_bits 64");
    constexpr uint32_t WAVES = kSmallThreads / 64, TILE = PAIR ? 128u : 64u;
    constexpr int MB = B ? 128 / B : 1;
    __shared__ uint32_t tab[kTabWords];
    __shared__ uint32_t scratch[(kSmallThreads / 64) * 256 + 8];
    __shared__ __attribute__((aligned(16))) uint32_t pre_lds[(kMaxLinks + kMaxChains) * 4];
    __shared__ uint64_t d_tlo[kMaxChains], d_cend[kMaxChains];
    const uint32_t iter = p.iter + p.te0[kIterShiftWord];
    fill_tables(tab, p.te0);
    const LaneRegs lr = lane_regs(tab);
    {
        const int last = n_chains - 1;
        const int n_streams = GAPS ? cg.n_streams : tb.sbase[last] + tb.len[last] + ((tb.flags[last] & 1) ? 0 : 1);
        for (int s = threadIdx.x; s < n_streams; s += kSmallThreads) {
            const CtrPrefix c = ctr_prefix(rk, lr, iter, tb.idx[s], 0u);          // n < 2^32 (host-checked): the high counter word is 0
            *reinterpret_cast<uint4 *>(pre_lds + 4 * s) = make_uint4(c.u[0], c.u[1], c.u[2], c.u[3]);
        }
        if (threadIdx.x < static_cast<unsigned>(n_chains)) {                          // this workgroup's tiles of every chain (see prf_chain_kernel)
            const int i = threadIdx.x;
            const uint64_t Wt = tb.wend[last], cw = i ? tb.wend[i - 1] : 0;
            const uint32_t w = GAPS ? static_cast<uint32_t>(cg.n_streams) : tb.len[i] + ((tb.flags[i] & 1) ? 0u : 1u);      // (GAPS: tiles are weighted by the streams they compute)
            uint64_t a, b, T;
            if (Wt <= 0xffffffffull && gridDim.x <= 0xffffu) {
                const uint32_t W32 = static_cast<uint32_t>(Wt), G = gridDim.x, g = blockIdx.x, c32 = static_cast<uint32_t>(cw);
                const uint32_t q = W32 / G, r = W32 % G;
                const uint32_t lo = q * g + r * g / G, hi = q * (g + 1) + r * (g + 1) / G;
                T = (static_cast<uint32_t>(tb.wend[i]) - c32) / w;
                a = lo > c32 ? (lo - c32 + w - 1) / w : 0; b = hi > c32 ? (hi - c32 + w - 1) / w : 0;
            } else {
                const uint64_t G = gridDim.x, g = blockIdx.x;
                const uint64_t lo = Wt / G * g + (Wt % G) * g / G, hi = Wt / G * (g + 1) + (Wt % G) * (g + 1) / G;
                T = (tb.wend[i] - cw) / w;
                a = lo > cw ? (lo - cw + w - 1) / w : 0; b = hi > cw ? (hi - cw + w - 1) / w : 0;
            }
            if (a > T) a = T;
            if (b > T) b = T;
            d_tlo[i] = a; d_cend[i] = b - a;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint64_t acc = 0;
            for (int i = 0; i < n_chains; i++) { acc += d_cend[i]; d_cend[i] = acc; }
        }
        __syncthreads();
    }
    const uint64_t J = p.n_jobs, d = p.n / J, r = p.n % J, m64 = static_cast<uint64_t>(p.m);
    const uint32_t nb1_32 = static_cast<uint32_t>((d + 1 + m64 - 1) / m64), nb0_32 = static_cast<uint32_t>(d ? (d + m64 - 1) / m64 : 0);
    const uint32_t d32 = static_cast<uint32_t>(d), r32 = static_cast<uint32_t>(r), m32 = static_cast<uint32_t>(p.m);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
    uint32_t *row0 = scratch + wave * 256;
    const u128 top = (static_cast<u128>(p.top_hi) << 64) | p.top_lo;
    const bool direct = p.m <= 4 && !p.no_direct;
    const bool walk32 = p.b <= 32 && !direct && p.no_direct != 2;     // (FLASHE_SMALL_DIRECT=2: A/B knob, general walk everywhere)
    const uint32_t wblk0 = lane / m32, wo0 = (lane - wblk0 * m32) * static_cast<uint32_t>(p.b);       // m >= 5 measured 35-150 % slower than the staged walk (40 .. 64-byte lane stride)      // m = 3, 4 measured: 8-byte accesses at a 24 / 32-byte lane stride lose 60-130 % against the staged walk
    const uint64_t Ng = uniform64(d_cend[n_chains - 1]);
    int cur = 0;
    uint64_t cbeg = 0;
    for (uint64_t q = wave; q < Ng; q += WAVES) {
        while (q >= uniform64(d_cend[cur])) cbeg = uniform64(d_cend[cur++]);
        const uint64_t first = tb.first[cur], range_end = first + tb.count[cur], blk_count = tb.blk_count[cur];
        const uint64_t Bw = (uniform64(d_tlo[cur]) + (q - cbeg)) * TILE;             // the tile's first block (chain-local)
        const int link0 = tb.link0[cur], sbase = tb.sbase[cur];
        const bool single = tb.flags[cur] & 1;
        const int n_streams = GAPS ? cg.n_streams : tb.len[cur] + (single ? 0 : 1);
        // per-lane block(s): chunk arithmetic and the counter-dependent quarter of round 1, once for all streams
        const bool vA = Bw + lane < blk_count, vB = PAIR && Bw + 64u + lane < blk_count;
        uint64_t j0A = 0, j0B = 0;
        int cntA = 0, cntB = 0;
        uint32_t ctrA = 0, ctrB = 0;
        small_block_params(static_cast<uint32_t>(tb.blk_first[cur] + (vA ? Bw + lane : 0)), nb1_32, nb0_32, d32, r32, m32, p, &j0A, &cntA, &ctrA);
        if (PAIR) small_block_params(static_cast<uint32_t>(tb.blk_first[cur] + (vB ? Bw + 64u + lane : 0)), nb1_32, nb0_32, d32, r32, m32, p, &j0B, &cntB, &ctrB);
        const CtrVar xA = ctr_var(rk, lr, ctrA);
        CtrVar xB{};
        if (PAIR) xB = ctr_var(rk, lr, ctrB);
        // the common tile: 64 whole blocks, all inside the range -> their 64 m elements are one contiguous run
        uint64_t e0A = 0, e0B = 0;
        bool fastA = false, fastB = false;
        if (walk32) {
            e0A = uniform64(j0A);
            fastA = __ballot(vA && cntA == p.m) == ~0ull && e0A >= first && e0A + 64u * m64 <= range_end;
            if (PAIR) {
                e0B = uniform64(j0B);
                fastB = __ballot(vB && cntB == p.m) == ~0ull && e0B >= first && e0B + 64u * m64 <= range_end;
            }
        }
        // (int_bits 64 at compile time: the lane's block is whole and inside the range -> one 16-byte access)
        const bool wholeA = B == 64 && vA && cntA == 2 && j0A >= first && j0A + 2 <= range_end;
        const bool wholeB = B == 64 && vB && cntB == 2 && j0B >= first && j0B + 2 <= range_end;
        u128 prevA = 0, prevB = 0;
        // (a summed chain, compile-time width: the blocks' running sums; irregular tiles keep theirs in memory, see small_walk)
        uint32_t accA[MB], accB[MB];
#pragma unroll
        for (int t = 0; t < MB; t++) { accA[t] = 0u; accB[t] = 0u; }
        uint32_t *const sum32 = B != 0 && B != 64 && !LIMB_OUT ? reinterpret_cast<uint32_t *>(tb.sum_out[cur]) : nullptr;
        // COHORT: the table row of each whole half tile, found once per tile with scalar loads (every link works on the same elements); a
        // half that straddles a row boundary is walked like a chunk end, its lanes look their rows up themselves (CohortWalk)
        int layA = -1, layB = -1;
        if constexpr (COHORT) {
            if (fastA) {
                layA = cohort_layer_of(cc, e0A - first);
                if (layA + 1 < cc.n_layers && *FLASHE_CONSTANT(const uint64_t, &cc.layers[layA + 1].start) < e0A - first + 64u * m64) layA = -1;
            }
            if (fastB) {
                layB = cohort_layer_of(cc, e0B - first);
                if (layB + 1 < cc.n_layers && *FLASHE_CONSTANT(const uint64_t, &cc.layers[layB + 1].start) < e0B - first + 64u * m64) layB = -1;
            }
            fastA = fastA && layA >= 0;
            fastB = fastB && layB >= 0;
        }
        if constexpr (PAIR && B != 0 && B != 64) {
            if (fastA && fastB) {                                  // (wave-uniform) both blocks of every lane whole and inside the range
                // the lanes' counters are consecutive inside a chunk; where a set of sixty-four does not cross a multiple of 256 its
                // bytes 1 .. 3 are the wave's (three sets of four in the chunks whose first counter is not a multiple of 64).  The second
                // counter shortcut only on short chains: on the ten-client chain its scalar loads at the head of every step cost more than
                // it saves (tests/perf/experiments/README.md)
                constexpr int kU2MaxStreams = 2;
                const uint32_t bA = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(ctrA)), bB = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(ctrB));
                const bool uni = !GAPS && n_streams <= kU2MaxStreams && __ballot(ctrA - bA == lane && ctrB - bB == lane) == ~0ull &&
                                 (bA & 255u) <= 192u && (bB & 255u) <= 192u;
                if constexpr (LIMB_OUT) {
                    const CohortDirect csrc{cc, tb.in + link0, link0, {layA, layB}};
                    small_chain_fast32<B, true, CohortDirect, uint64_t>(rk, lr, pre_lds, sbase, n_streams, tb.in + link0, tb.out + link0, xA, xB, j0A - first, j0B - first,
                                                                        nullptr, p.swp_prio != 0, p.te0, uni, bA ^ rk.w[3], bB ^ rk.w[3], &csrc);
                    continue;
                } else if constexpr (GAPS) {                       // (several runs never take the second counter shortcut: more than two streams)
                    const CohortDirect csrc{cc, tb.in + link0, link0, {layA, layB}};
                    small_chain_fast32<B, false, CohortDirect, uint32_t, CohortGaps>(rk, lr, pre_lds, sbase, n_streams, tb.in + link0, tb.out + link0, xA, xB, j0A - first, j0B - first,
                                                                                     sum32, p.swp_prio != 0, p.te0, false, 0u, 0u, &csrc, &cg);
                    continue;
                } else if constexpr (COHORT) {
                    const CohortDirect csrc{cc, tb.in + link0, link0, {layA, layB}};
                    small_chain_fast32<B, false>(rk, lr, pre_lds, sbase, n_streams, tb.in + link0, tb.out + link0, xA, xB, j0A - first, j0B - first, sum32, p.swp_prio != 0,
                                                 p.te0, uni, bA ^ rk.w[3], bB ^ rk.w[3], &csrc);
                    continue;
                }
                if (single) small_chain_fast32<B, true>(rk, lr, pre_lds, sbase, n_streams, tb.in + link0, tb.out + link0, xA, xB, j0A - first, j0B - first, sum32, p.swp_prio != 0,
                                                        p.te0, uni, bA ^ rk.w[3], bB ^ rk.w[3]);
                else small_chain_fast32<B, false>(rk, lr, pre_lds, sbase, n_streams, tb.in + link0, tb.out + link0, xA, xB, j0A - first, j0B - first, sum32, p.swp_prio != 0,
                                                  p.te0, uni, bA ^ rk.w[3], bB ^ rk.w[3]);
                continue;
            }
        }
        if (PAIR) {
            // two blocks per lane on the same prefix, one stream per step
            for (int c = 0; c < n_streams; c++) {
                const CtrPrefix pre = load_prefix(pre_lds, sbase + c);
                const int link = GAPS ? cohort_stream_link(cg, c) : single ? c : c - 1;      // the output this stream completes
                WalkPt ptA{}, ptB{};
                DirectPt<MB> dA{}, dB{};
                u64x2 qA = {0ull, 0ull}, qB = {0ull, 0ull};
                if (B == 64) {
                    if (link >= 0 && wholeA) qA = direct64_load(tb.in[link0 + link], j0A - first);
                    if (link >= 0 && wholeB) qB = direct64_load(tb.in[link0 + link], j0B - first);
                } else if (COHORT) {
                    if constexpr (COHORT) {
                        const CohortDirect csrc{cc, tb.in + link0, link0, {layA, layB}};
                        if (link >= 0 && fastA) dA = csrc.template block<MB>(link, j0A - first, 0);
                        if (link >= 0 && fastB) dB = csrc.template block<MB>(link, j0B - first, 1);
                    }
                } else if (B) {
                    if (link >= 0 && fastA) dA = direct32_load<MB>(reinterpret_cast<const uint32_t *>(tb.in[link0 + link]), j0A - first);
                    if (link >= 0 && fastB) dB = direct32_load<MB>(reinterpret_cast<const uint32_t *>(tb.in[link0 + link]), j0B - first);
                } else {
                    if (link >= 0 && fastA) ptA = small_walk32_load(reinterpret_cast<const ET *>(tb.in[link0 + link]), e0A, first, lane, m32);
                    if (link >= 0 && fastB) ptB = small_walk32_load(reinterpret_cast<const ET *>(tb.in[link0 + link]), e0B, first, lane, m32);
                }
                uint32_t s[2][4];
                ctr_round1(pre, xA, s[0]);
                ctr_round1(pre, xB, s[1]);
                aes256_rounds<2, 2>(rk, lr, s, p.swp_prio != 0);
                const u128 SA = words_to_u128(s[0]), SB = words_to_u128(s[1]);
                if (link >= 0) {
                    const uint64_t *in = tb.in[link0 + link];
                    uint64_t *out = tb.out[link0 + link];
                    const ET *ein = reinterpret_cast<const ET *>(in);
                    ET *eout = reinterpret_cast<ET *>(out);
                    if (B == 64) {
                        if constexpr (B == 64) {
                            if (wholeA) direct64_store(out, j0A - first, qA, single ? SA : prevA, SA, single);
                            else small_direct(vA, cntA, j0A, single ? SA : slot_diff(prevA, SA, top, 64), in, out, first, range_end, p);
                            if (wholeB) direct64_store(out, j0B - first, qB, single ? SB : prevB, SB, single);
                            else small_direct(vB, cntB, j0B, single ? SB : slot_diff(prevB, SB, top, 64), in, out, first, range_end, p);
                        }
                        prevA = SA; prevB = SB;
                        continue;
                    }
                    if (B) {
                        // compile-time width: whole tiles element by element from the two streams' slots, everything else the general walk
                        if constexpr (B != 0 && B != 64) {
                            using OT = std::conditional_t<LIMB_OUT, uint64_t, uint32_t>;
                            OT *o32 = reinterpret_cast<OT *>(out);
                            ET *const sm = reinterpret_cast<ET *>(sum32);
                            if (fastA) direct32_store<B, OT>(o32, j0A - first, dA, single ? SA : prevA, SA, single, accA);
                            else if constexpr (COHORT) {
                                const CohortWalk cw{cc, in, link0 + link};
                                small_walk(row0, lane, vA, cntA, j0A, single ? SA : slot_diff(prevA, SA, top, p.b), ein, eout, first, range_end, p, sm, link == 0, &cw);
                            }
                            else small_walk(row0, lane, vA, cntA, j0A, single ? SA : slot_diff(prevA, SA, top, p.b), ein, eout, first, range_end, p, sm, link == 0);
                            if (fastB) direct32_store<B, OT>(o32, j0B - first, dB, single ? SB : prevB, SB, single, accB);
                            else if constexpr (COHORT) {
                                const CohortWalk cw{cc, in, link0 + link};
                                small_walk(row0, lane, vB, cntB, j0B, single ? SB : slot_diff(prevB, SB, top, p.b), ein, eout, first, range_end, p, sm, link == 0, &cw);
                            }
                            else small_walk(row0, lane, vB, cntB, j0B, single ? SB : slot_diff(prevB, SB, top, p.b), ein, eout, first, range_end, p, sm, link == 0);
                        }
                        prevA = SA; prevB = SB;
                        continue;
                    }
                    // per slot (previous - current) mod 2^b: the previous stream is this client's add stream, the current its minus stream
                    const u128 DA = single ? SA : slot_diff(prevA, SA, top, p.b);
                    const u128 DB = single ? SB : slot_diff(prevB, SB, top, p.b);
                    if (direct) {                                  // (never with the compact layout: the host turns `direct` off)
                        small_direct(vA, cntA, j0A, DA, in, out, first, range_end, p);
                        small_direct(vB, cntB, j0B, DB, in, out, first, range_end, p);
                    } else {
                        if (fastA) small_walk32(row0, lane, e0A, DA, ptA, ein, eout, first, p, wblk0, wo0);
                        else small_walk(row0, lane, vA, cntA, j0A, DA, ein, eout, first, range_end, p);
                        if (fastB) small_walk32(row0, lane, e0B, DB, ptB, ein, eout, first, p, wblk0, wo0);
                        else small_walk(row0, lane, vB, cntB, j0B, DB, ein, eout, first, range_end, p);
                    }
                }
                prevA = SA; prevB = SB;
            }
            if constexpr (B != 0 && B != 64) {
                if (sum32) {                                         // the sums of the blocks that took the direct path, one store each
                    constexpr uint32_t bmask = B >= 32 ? 0xffffffffu : ((1u << (B & 31)) - 1u);
                    if (fastA) direct32_put<MB>(sum32 + (j0A - first), accA, bmask);
                    if (fastB) direct32_put<MB>(sum32 + (j0B - first), accB, bmask);
                }
            }
        } else {
            // one block per lane, TWO STREAMS per step (short launches: half the dependent AES depth per wave; an odd stream count
            // computes its last stream twice)
            for (int c = 0; c < n_streams; c += 2) {
                const bool has1 = c + 1 < n_streams;
                const CtrPrefix pre0 = load_prefix(pre_lds, sbase + c), pre1 = load_prefix(pre_lds, sbase + (has1 ? c + 1 : c));
                const int l0 = single ? c : c - 1;
                WalkPt pt0{}, pt1{};
                if (fastA && l0 >= 0) pt0 = small_walk32_load(reinterpret_cast<const ET *>(tb.in[link0 + l0]), e0A, first, lane, m32);
                if (fastA && has1) pt1 = small_walk32_load(reinterpret_cast<const ET *>(tb.in[link0 + l0 + 1]), e0A, first, lane, m32);
                uint32_t s[2][4];
                ctr_round1(pre0, xA, s[0]);
                ctr_round1(pre1, xA, s[1]);
                aes256_rounds<2, 2>(rk, lr, s, true);
                const u128 S0 = words_to_u128(s[0]), S1 = words_to_u128(s[1]);
                if (l0 >= 0) {
                    const u128 D = single ? S0 : slot_diff(prevA, S0, top, p.b);
                    const ET *ein = reinterpret_cast<const ET *>(tb.in[link0 + l0]);
                    ET *eout = reinterpret_cast<ET *>(tb.out[link0 + l0]);
                    if (direct) small_direct(vA, cntA, j0A, D, tb.in[link0 + l0], tb.out[link0 + l0], first, range_end, p);
                    else if (fastA) small_walk32(row0, lane, e0A, D, pt0, ein, eout, first, p, wblk0, wo0);
                    else small_walk(row0, lane, vA, cntA, j0A, D, ein, eout, first, range_end, p);
                }
                if (has1) {
                    const u128 D = single ? S1 : slot_diff(S0, S1, top, p.b);
                    const ET *ein = reinterpret_cast<const ET *>(tb.in[link0 + l0 + 1]);
                    ET *eout = reinterpret_cast<ET *>(tb.out[link0 + l0 + 1]);
                    if (direct) small_direct(vA, cntA, j0A, D, tb.in[link0 + l0 + 1], tb.out[link0 + l0 + 1], first, range_end, p);
                    else if (fastA) small_walk32(row0, lane, e0A, D, pt1, ein, eout, first, p, wblk0, wo0);
                    else small_walk(row0, lane, vA, cntA, j0A, D, ein, eout, first, range_end, p);
                }
                prevA = has1 ? S1 : S0;
            }
        }
    }
