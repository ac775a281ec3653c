// The body of prf_chain_kernel<THREADS, SUM, CODEC>, prf_chain_dmask_kernel<THREADS>, prf_dmask_sum128_kernel<THREADS>, prf_dec_sum128_kernel<THREADS> and
// prf_chain_cohort_kernel<THREADS>, prf_chain_cohort_cut_kernel<THREADS>, prf_chain_cohort_batch_kernel<THREADS, BS> and prf_chain_cohort_batch_cut_kernel<THREADS, BS> (kernels.hip), included INSIDE each kernel: the kernel defines
// THREADS, SUM, CODEC, DMASK, D128, COHORT, BS, GAPS, DEC and CUT as compile-time constants and has the arguments rk, tb, n_chains, all_half_arg, iter0, mask_lo,
// mask_hi, te0, cq, cc, cb, cg, dmask and cut_stride in scope.
// CUT (COHORT only, prf_chain_cohort_cut_kernel; with BS > 0 prf_chain_cohort_batch_cut_kernel, whose elements are the batched ones -- the
// front end and the mask store address a chain's clients alike, link0 + link): a SHORT cohort cut into n_chains runs of consecutive clients (cohort_cut.h), every run its
// own summed double-mask chain over the same elements.  tb.sum_out[cur] is per chain already; the decrypt mask of chain `cur` goes to
// dmask + cur * cut_stride where the other DMASK kernels have one mask for the launch's one chain.  The chains' masks telescope and
// their sums add up: one combine pass (cohort_cut_combine_kernel, stream.hip) gives what the uncut launch writes.  Every branch on CUT is
// an `if constexpr`: the other instantiations compile to the kernels they were.
// DEC (D128 only, prf_dec_sum128_kernel): where the DMASK kernels store the decrypt mask D on the last stream, the launch stores the decrypt of
// the sum it writes beside it, sum + D mod 2^b; `dmask` addresses that output.  Every branch on DEC is an `if constexpr`.
// GAPS (COHORT only, prf_chain_cohort_runs_kernel / prf_chain_cohort_batch_runs_kernel): the cohort's cipher indices form SEVERAL runs -- clients
// dropped out.  The stream loop runs over the cg.n_streams streams of tb.idx (cohort_streams.h); a stream's word of CohortGaps (a wave-uniform
// scalar read of the kernel arguments) says whether it completes an output -- the next link in turn -- and whether it opens a client.  A stream
// that completes nothing requests no float or draw, stores nothing and adds nothing to the sums; the registers that hold the first stream's
// blocks in the other DMASK kernels accumulate the decrypt mask instead: -= on a run-opening stream, += on a run-closing one, stored
// beside the sum on the last stream.  Every branch on GAPS is an `if constexpr` or a conditional on the constant, and the other instantiations
// declare nothing for it: they compile to the kernels they were.
// BS > 0 (COHORT only): the BATCHED cohort -- the chain's elements are the model's batched elements and every output's plaintext packs BS
// quantised values of its client (CohortBatch cb beside cc; tb.in[link] = that client's draws, value-indexed).  The floats and draws of an
// element are requested in runs, quantised and packed BEFORE the stream's rounds (cohort_batch_element): only the two packed plaintexts
// live through the rounds.  Every branch on BS is an `if constexpr`: the other instantiations compile to the kernels they were.
// COHORT: one summed double-mask chain whose every output has a quantising front end (CohortCodec cc; tb.in[link] = that client's draws).  D128: the launch is one summed double-mask
// chain at int_bits = 128 with one-limb inputs (launch_prf_chains), and its whole tiles run prf_chain_sum128_tile.inc.  (A __device__ function shared by both would do, but its blockDim is lowered before it
// is inlined -- the non-uniform-workgroup form -- and the headline kernel's code would change with it; included text compiles to
// exactly the kernel it was before.)
    static_assert(!DMASK || (SUM && !CODEC), "the decrypt mask is written by summed chains only");
    static_assert(!D128 || DMASK, "the int_bits = 128 specialisation is the decrypt-mask chain's");
    static_assert(!COHORT || (DMASK && !D128), "the cohort front end rides on the summed decrypt-mask chain");
    static_assert(BS == 0 || COHORT, "batching is a form of the cohort front end");
    static_assert(!GAPS || COHORT, "several runs of indices are a form of the cohort chain");
    static_assert(!DEC || D128, "the decrypted sum is written by the int_bits = 128 specialisation");
    static_assert(!CUT || (COHORT && !GAPS), "the cut is a form of the cohort chain whose every piece is one run of clients");
    (void)cg;
    (void)cut_stride;
    (void)dmask;
    (void)cc;
    (void)cb;
    const uint32_t iter = iter0 + te0[kIterShiftWord];
    constexpr uint32_t WAVES = THREADS / 64;
    __shared__ uint32_t tab[kTabWords];
    __shared__ __attribute__((aligned(16))) uint32_t pre_lds[(kMaxLinks + kMaxChains) * 4];
    __shared__ uint64_t d_tlo[kMaxChains], d_cend[kMaxChains];
    int all_half = all_half_arg;
    fill_tables(tab, te0);
#ifdef FLASHE_TUNING
    if (all_half & 0x100) return;                  // timing probes of the prologue (FLASHE_CHAIN_TUNE / FLASHE_CHAIN_PROBE only)
#endif
    const LaneRegs lr = lane_regs(tab);
    const u128 mask = D128 ? ~static_cast<u128>(0) : (static_cast<u128>(mask_hi) << 64) | mask_lo;
    {
        // round-1 prefix words of every stream (chains never straddle a 2^32 counter window: host-checked)
        const int last = n_chains - 1;
        const int n_streams = GAPS ? cg.n_streams : tb.sbase[last] + tb.len[last] + ((tb.flags[last] & 1) ? 0 : 1);
        for (int s = threadIdx.x; s < n_streams; s += THREADS) {
            int i = 0;
            while (i < last && s >= tb.sbase[i + 1]) i++;
            const CtrPrefix c = ctr_prefix(rk, lr, iter, tb.idx[s], static_cast<uint32_t>(tb.first[i] >> 32));
            *reinterpret_cast<uint4 *>(pre_lds + 4 * s) = make_uint4(c.u[0], c.u[1], c.u[2], c.u[3]);
        }
        // this workgroup's tiles of every chain: lane i works out chain i (32-bit arithmetic whenever the launch's total
        // weight fits -- a 64-bit division is ~150 dependent instructions, and a short launch is all prologue)
        if (threadIdx.x < static_cast<unsigned>(n_chains)) {
            const int i = threadIdx.x;
            const uint64_t Wt = tb.wend[last], cw = i ? tb.wend[i - 1] : 0;
            const uint32_t w = GAPS ? static_cast<uint32_t>(cg.n_streams) : tb.len[i] + ((tb.flags[i] & 1) ? 0u : 1u);      // (GAPS: tiles are weighted by the streams they compute)
            uint64_t a, b, T;
            if (Wt <= 0xffffffffull && gridDim.x <= 0xffffu) {
                const uint32_t W32 = static_cast<uint32_t>(Wt), G = gridDim.x, g = blockIdx.x, c32 = static_cast<uint32_t>(cw);
                const uint32_t q = W32 / G, r = W32 % G;
                const uint32_t lo = q * g + r * g / G, hi = q * (g + 1) + r * (g + 1) / G;
                const uint32_t T32 = (static_cast<uint32_t>(tb.wend[i]) - c32) / w;
                const uint32_t a32 = lo > c32 ? (lo - c32 + w - 1) / w : 0, b32 = hi > c32 ? (hi - c32 + w - 1) / w : 0;
                T = T32; a = a32; b = b32;
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
#ifdef FLASHE_TUNING
    if (all_half & 0x200) return;
#endif
    // (bit 2, round 6: the whole launch in QUARTER tiles -- 64 counters, one block per lane and stream, two STREAMS per step -- for
    // launches too short to give every wave a half tile: see the quarter branch below)
    const bool quarter = !CODEC && !SUM && (all_half & 4) != 0;            // (a summed chain is only launched with two whole tiles per wave: launch_prf_batch_sum)
    all_half &= 1;
    const uint32_t wave = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t Ng = uniform64(d_cend[n_chains - 1]);
    const uint64_t n_full = (all_half || quarter) ? 0 : Ng - Ng % WAVES;
    const uint64_t n_items = quarter ? 4 * Ng : n_full + 2 * (Ng - n_full);
    int cur = 0;
    uint64_t cbeg = 0;                                                     // local index of chain cur's first tile
    for (uint64_t q = wave; q < n_items; q += WAVES) {
        const bool whole = q < n_full;
        const uint64_t L = quarter ? (q >> 2) : whole ? q : n_full + ((q - n_full) >> 1);
        const uint32_t half = whole || quarter ? 0u : static_cast<uint32_t>((q - n_full) & 1u);
        while (L >= uniform64(d_cend[cur])) cbeg = uniform64(d_cend[cur++]);
        const uint64_t first = tb.first[cur], end = first + tb.count[cur];
        const uint64_t tj = (first & ~255ull) + 256u * (uniform64(d_tlo[cur]) + (L - cbeg)) + 128u * half +
                            (quarter ? 64u * static_cast<uint32_t>(q & 3u) : 0u);                             // first counter of the item
        const int link0 = tb.link0[cur], sbase = tb.sbase[cur];
        const bool single = !D128 && (tb.flags[cur] & 1), in2 = !D128 && (tb.flags[cur] & 2);
        const int n_streams = GAPS ? cg.n_streams : tb.len[cur] + (single ? 0 : 1);
        if constexpr (D128) {
            if (whole) {
#include "prf_chain_sum128_tile.inc"
                continue;
            }
        }
        if (whole) {
            // ---- 256 elements: two pairs per lane, wave-uniform part of rounds 1-2 through the scalar cache ----
            const uint32_t x3 = static_cast<uint32_t>(tj) ^ rk.w[3];
            const uint32_t jl = static_cast<uint32_t>(tj) + lane;
            uint32_t vA0 = T3(jl ^ rk.w[3], SEL_B0), vA1 = T3((jl + 64u) ^ rk.w[3], SEL_B0);
            uint32_t vB0 = T3((jl + 128u) ^ rk.w[3], SEL_B0), vB1 = T3((jl + 192u) ^ rk.w[3], SEL_B0);
            u128 pA0 = 0, pA1 = 0, pB0 = 0, pB1 = 0;
            u128 qA0 = 0, qA1 = 0, qB0 = 0, qB1 = 0;                   // SUM: running sum of the outputs of the lane's four elements
            u128 dA0 = 0, dA1 = 0, dB0 = 0, dB1 = 0;                   // DMASK: the first stream's blocks of the lane's four elements (GAPS: their running decrypt mask)
            uint64_t *const sum_out = SUM ? tb.sum_out[cur] : nullptr;
            // COHORT: the table row of each pair's first element, found once per tile (every link works on the same elements); -1 = the
            // pair straddles a layer boundary (at most one pair per layer of the model) and its lanes look their rows up themselves
            int layA = -1, layB = -1;
            if constexpr (COHORT) {
                for (int p = 0; p < 2; p++) {
                    const uint64_t jb = tj + 128u * p, kb = (jb > first ? jb : first) - first, ke = (jb + 128u < end ? jb + 128u : end) - first;
                    int l = -1;
                    if (jb < end && jb + 128u > first) {
                        if constexpr (BS > 0) {
                            l = cohort_batch_row_of(cb, cc.n_layers, kb);
                            if (l + 1 < cc.n_layers && *FLASHE_CONSTANT(const uint64_t, cb.rows + 2 * (l + 1)) < ke) l = -1;
                        } else {
                            l = cohort_layer_of(cc, kb);
                            if (l + 1 < cc.n_layers && *FLASHE_CONSTANT(const uint64_t, &cc.layers[l + 1].start) < ke) l = -1;
                        }
                    }
                    if (p == 0) layA = l; else layB = l;
                }
            }
            for (int c = 0; c < n_streams; c++) {
                const CtrPrefix pre = load_prefix(pre_lds, sbase + c);
                const CtrUniform U = ctr_uniform(rk, te0, pre, x3);
                const int link = GAPS ? cohort_stream_link(cg, c) : single ? c : c - 1;      // the output this stream completes
                const uint64_t *in = link >= 0 ? tb.in[link0 + link] : nullptr;
                uint64_t *out = link >= 0 ? tb.out[link0 + link] : nullptr;
                const bool last_stream = c == n_streams - 1;
#pragma unroll 1
                for (int p = 0; p < 2; p++) {
                    const uint64_t jb = tj + 128u * p;
                    if (jb < end && jb + 128u > first) {
                        const uint64_t j0 = jb + lane, j1 = j0 + 64u, k0 = j0 - first, k1 = j1 - first;
                        const bool a0 = j0 >= first && j0 < end, a1 = j1 >= first && j1 < end;
                        // every load is consumed on every path (the adds below are unconditional, only the stores are
                        // predicated): otherwise the compiler must assume a load may still be in flight at the loop's back
                        // edge and drains the memory queue -- stores included -- every iteration
                        // COHORT: the float's bits and the draw are requested here and quantised after the rounds with the row's
                        // parameters in SGPRs (crow < 0: already the plaintext)
                        uint64_t raw0 = 0, raw1 = 0;
                        double u0 = 0, u1 = 0, cp0 = 0, cp1 = 0, cp2 = 0;
                        bool cf64 = false;
                        const int crow = COHORT && link >= 0 ? layA : -1;
                        u128 x0 = 0, x1 = 0;
                        if constexpr (BS > 0) {
                            // (the batched front end: packed before the rounds; row crow >= 0: its parameters in SGPRs, else looked up per lane)
                            if (link >= 0) {
                                const double *const ud = reinterpret_cast<const double *>(in);
                                if (crow >= 0) {
                                    const CodecLayer *const L = cc.layers + crow;
                                    const uint64_t vs = *FLASHE_CONSTANT(const uint64_t, &L->start), es = *FLASHE_CONSTANT(const uint64_t, cb.rows + 2 * crow),
                                                   sz = *FLASHE_CONSTANT(const uint64_t, cb.rows + 2 * crow + 1);
                                    const void *const xs = reinterpret_cast<const void *>(*FLASHE_CONSTANT(const uintptr_t, cc.src + static_cast<size_t>(link0 + link) * cc.n_layers + crow));
                                    const bool bf64 = *FLASHE_CONSTANT(const int, &L->x_is_f64) != 0;
                                    const double b0 = *FLASHE_CONSTANT(const double, &L->p0), b1 = *FLASHE_CONSTANT(const double, &L->p1),
                                                 b2 = *FLASHE_CONSTANT(const double, &L->p2);
                                    if (a0) x0 = cohort_batch_element<BS>(xs, bf64, b0, b1, b2, ud + vs, (k0 - es) * static_cast<uint64_t>(BS), sz, cb.field_bits);
                                    if (a1) x1 = cohort_batch_element<BS>(xs, bf64, b0, b1, b2, ud + vs, (k1 - es) * static_cast<uint64_t>(BS), sz, cb.field_bits);
                                } else {
                                    if (a0) x0 = cohort_batch_lane<BS>(cc, cb, link0 + link, k0, ud);
                                    if (a1) x1 = cohort_batch_lane<BS>(cc, cb, link0 + link, k1, ud);
                                }
                            }
                        } else if constexpr (COHORT) {
                            if (link >= 0) {
                                const double *const ud = reinterpret_cast<const double *>(in);
                                if (a0) u0 = *FLASHE_GLOBAL(const double, ud + k0);
                                if (a1) u1 = *FLASHE_GLOBAL(const double, ud + k1);
                                if (crow >= 0) {
                                    const CodecLayer *const L = cc.layers + crow;
                                    const uint64_t ls = *FLASHE_CONSTANT(const uint64_t, &L->start);
                                    const void *const xs = reinterpret_cast<const void *>(*FLASHE_CONSTANT(const uintptr_t, cc.src + static_cast<size_t>(link0 + link) * cc.n_layers + crow));
                                    cf64 = *FLASHE_CONSTANT(const int, &L->x_is_f64) != 0;
                                    cp0 = *FLASHE_CONSTANT(const double, &L->p0); cp1 = *FLASHE_CONSTANT(const double, &L->p1);
                                    cp2 = *FLASHE_CONSTANT(const double, &L->p2);
                                    if (a0) raw0 = cohort_load(xs, cf64, k0 - ls);
                                    if (a1) raw1 = cohort_load(xs, cf64, k1 - ls);
                                } else {
                                    if (a0) raw0 = cohort_quantize_lane(cc, link0 + link, k0, u0);
                                    if (a1) raw1 = cohort_quantize_lane(cc, link0 + link, k1, u1);
                                }
                            }
                        } else if (CODEC && cq.x != nullptr && link >= 0) {
                            if (a0) x0 = codec_quantize(cq, k0);
                            if (a1) x1 = codec_quantize(cq, k1);
                        } else if (in != nullptr && in2) {
                            if (a0) x0 = ld128(in + 2 * k0);
                            if (a1) x1 = ld128(in + 2 * k1);
                        } else if (in != nullptr) {
                            if (a0) x0 = static_cast<u128>(in[k0]);
                            if (a1) x1 = static_cast<u128>(in[k1]);
                        }
                        uint32_t s[2][4];
                        ctr_round2(lr, pre.u[0], vA0, U, s[0]);
                        ctr_round2(lr, pre.u[0], vA1, U, s[1]);
                        aes256_rounds<2, 3>(rk, lr, s, true);
                        if constexpr (COHORT && BS == 0) {
                            cohort_loads_landed(raw0, raw1, u0, u1);
                            x0 = crow >= 0 ? cohort_quantize_raw(raw0, cf64, cp0, cp1, cp2, u0) : raw0;
                            x1 = crow >= 0 ? cohort_quantize_raw(raw1, cf64, cp0, cp1, cp2, u1) : raw1;
                        }
                        loads_landed(x0, x1);
                        const u128 c0 = words_to_u128(s[0]), c1 = words_to_u128(s[1]);
                        const u128 r0 = x0 + (single ? c0 : pA0 - c0), r1 = x1 + (single ? c1 : pA1 - c1);
                        if (CODEC && cq.fout != nullptr) {
                            if (a0 && link >= 0) cq.fout[k0] = codec_unquantize(cq, k0, r0 & mask);
                            if (a1 && link >= 0) cq.fout[k1] = codec_unquantize(cq, k1, r1 & mask);
                        } else {
                            if (a0 && out != nullptr) st128(out + 2 * k0, r0 & mask);
                            if (a1 && out != nullptr) st128(out + 2 * k1, r1 & mask);
                        }
                        if constexpr (SUM) {
                            // (the sums do not take part in the register rotation of the rolled pair loop: p is wave-uniform, a scalar
                            // branch around four adds is cheaper than eight more moves per pair)
                            if (link >= 0) {
                                if (p == 0) { qA0 += r0; qA1 += r1; } else { qB0 += r0; qB1 += r1; }
                            }
                            if (last_stream && sum_out != nullptr) {
                                if (p == 0) {
                                    if (a0) st128_nt(sum_out + 2 * k0, qA0 & mask);
                                    if (a1) st128_nt(sum_out + 2 * k1, qA1 & mask);
                                } else {
                                    if (a0) st128_nt(sum_out + 2 * k0, qB0 & mask);
                                    if (a1) st128_nt(sum_out + 2 * k1, qB1 & mask);
                                }
                            }
                        }
                        if constexpr (GAPS) {
                            // (the running decrypt mask: the stream's bits and p are wave-uniform)
                            const uint32_t sbits = cohort_stream_bits(cg, c);
                            if (sbits == 2u) {
                                if (p == 0) { dA0 -= c0; dA1 -= c1; } else { dB0 -= c0; dB1 -= c1; }
                            } else if (sbits == 1u) {
                                if (p == 0) { dA0 += c0; dA1 += c1; } else { dB0 += c0; dB1 += c1; }
                            }
                            if (last_stream && dmask != nullptr) {
                                if (p == 0) {
                                    if (a0) st128_nt(dmask + 2 * k0, dA0 & mask);
                                    if (a1) st128_nt(dmask + 2 * k1, dA1 & mask);
                                } else {
                                    if (a0) st128_nt(dmask + 2 * k0, dB0 & mask);
                                    if (a1) st128_nt(dmask + 2 * k1, dB1 & mask);
                                }
                            }
                        } else if constexpr (DMASK) {
                            // (p is wave-uniform: the same scalar branch as the running sums)
                            if (c == 0) {
                                if (p == 0) { dA0 = c0; dA1 = c1; } else { dB0 = c0; dB1 = c1; }
                            }
                            if constexpr (DEC) {
                                // (the decrypt of the sum stored above, sum + D mod 2^b, where the others store D)
                                if (last_stream) {
                                    if (p == 0) {
                                        if (a0) st128_nt(dmask + 2 * k0, (qA0 + (c0 - dA0)) & mask);
                                        if (a1) st128_nt(dmask + 2 * k1, (qA1 + (c1 - dA1)) & mask);
                                    } else {
                                        if (a0) st128_nt(dmask + 2 * k0, (qB0 + (c0 - dB0)) & mask);
                                        if (a1) st128_nt(dmask + 2 * k1, (qB1 + (c1 - dB1)) & mask);
                                    }
                                }
                            } else if (last_stream && (!COHORT || dmask != nullptr)) {
                                if constexpr (CUT) {
                                    uint64_t *const dm = dmask + static_cast<uint64_t>(cur) * cut_stride;     // (chain cur's own mask)
                                    if (p == 0) {
                                        if (a0) st128_nt(dm + 2 * k0, (c0 - dA0) & mask);
                                        if (a1) st128_nt(dm + 2 * k1, (c1 - dA1) & mask);
                                    } else {
                                        if (a0) st128_nt(dm + 2 * k0, (c0 - dB0) & mask);
                                        if (a1) st128_nt(dm + 2 * k1, (c1 - dB1) & mask);
                                    }
                                } else if (p == 0) {
                                    if (a0) st128_nt(dmask + 2 * k0, (c0 - dA0) & mask);
                                    if (a1) st128_nt(dmask + 2 * k1, (c1 - dA1) & mask);
                                } else {
                                    if (a0) st128_nt(dmask + 2 * k0, (c0 - dB0) & mask);
                                    if (a1) st128_nt(dmask + 2 * k1, (c1 - dB1) & mask);
                                }
                            }
                        }
                        pA0 = c0; pA1 = c1;
                    }
                    swap_regs(pA0, pB0); swap_regs(pA1, pB1); swap_regs(vA0, vB0); swap_regs(vA1, vB1);
                    if constexpr (COHORT) swap_regs(layA, layB);
                }
            }
        } else if (quarter) {
            // ---- 64 elements (round 6): ONE block per lane and stream, the software-pipelined pair is two consecutive STREAMS of the
            // chain.  For launches that cannot give every wave of the chip a half tile (config 3: a hundred LeNet-sized vectors are
            // 242 tiles): four times the items, so a chain is cut into a third as many pieces (a cut costs a stream) and every wave
            // gets ONE item of the same length instead of one or two; and 64 aligned counters share bytes 1 .. 3, so both counter-mode
            // shortcuts apply (196 lookups per block; the half tiles take only the first: 208).
            if (!CODEC && !SUM && tj < end && tj + 64u > first) {
                const uint64_t j0 = tj + lane, k0 = j0 - first;
                const bool a0 = j0 >= first && j0 < end;
                const uint32_t x3 = static_cast<uint32_t>(tj) ^ rk.w[3];
                const uint32_t v0 = T3(static_cast<uint32_t>(j0) ^ rk.w[3], SEL_B0);
                u128 pv = 0;
                for (int c = 0; c < n_streams; c += 2) {
                    const bool has1 = c + 1 < n_streams;             // (an odd stream count computes its last stream twice)
                    const CtrPrefix pre0 = load_prefix(pre_lds, sbase + c), pre1 = load_prefix(pre_lds, sbase + (has1 ? c + 1 : c));
                    const CtrUniform U0 = ctr_uniform(rk, te0, pre0, x3), U1 = ctr_uniform(rk, te0, pre1, x3);
                    const int l0 = single ? c : c - 1;               // the output stream c completes; stream c + 1 completes l0 + 1
                    const uint64_t *in0 = l0 >= 0 ? tb.in[link0 + l0] : nullptr, *in1 = has1 ? tb.in[link0 + l0 + 1] : nullptr;
                    u128 x0 = 0, x1 = 0;
                    if (in0 != nullptr && a0) x0 = in2 ? ld128(in0 + 2 * k0) : static_cast<u128>(in0[k0]);
                    if (in1 != nullptr && a0) x1 = in2 ? ld128(in1 + 2 * k0) : static_cast<u128>(in1[k0]);
                    uint32_t s[2][4];
                    ctr_round2(lr, pre0.u[0], v0, U0, s[0]);
                    ctr_round2(lr, pre1.u[0], v0, U1, s[1]);
                    aes256_rounds<2, 3>(rk, lr, s, true);
                    loads_landed(x0, x1);
                    const u128 c0 = words_to_u128(s[0]), c1 = words_to_u128(s[1]);
                    if (l0 >= 0) {
                        const u128 r0 = (x0 + (single ? c0 : pv - c0)) & mask;
                        if (a0 && tb.out[link0 + l0] != nullptr) st128(tb.out[link0 + l0] + 2 * k0, r0);
                    }
                    if (has1) {
                        const u128 r1 = (x1 + (single ? c1 : c0 - c1)) & mask;
                        if (a0 && tb.out[link0 + l0 + 1] != nullptr) st128(tb.out[link0 + l0 + 1] + 2 * k0, r1);
                    }
                    pv = has1 ? c1 : c0;
                }
            }
        } else if (tj < end && tj + 128u > first) {
            // ---- 128 elements: one pair per lane; the counter-dependent lookup of round 1 is shared by all streams ----
            const uint64_t j0 = tj + lane, j1 = j0 + 64u, k0 = j0 - first, k1 = j1 - first;
            const bool a0 = j0 >= first && j0 < end, a1 = j1 >= first && j1 < end;
            const CtrVar xv0 = ctr_var(rk, lr, static_cast<uint32_t>(j0)), xv1 = ctr_var(rk, lr, static_cast<uint32_t>(j1));
            const uint32_t x3h = static_cast<uint32_t>(tj) ^ rk.w[3];        // (a half tile is 128 aligned counters: bytes 1 .. 3 are the wave's)
            int lay = -1;                                               // COHORT: the pair's table row, as in a whole tile
            if constexpr (COHORT) {
                const uint64_t kb = (tj > first ? tj : first) - first, ke = (tj + 128u < end ? tj + 128u : end) - first;
                if constexpr (BS > 0) {
                    lay = cohort_batch_row_of(cb, cc.n_layers, kb);
                    if (lay + 1 < cc.n_layers && *FLASHE_CONSTANT(const uint64_t, cb.rows + 2 * (lay + 1)) < ke) lay = -1;
                } else {
                    lay = cohort_layer_of(cc, kb);
                    if (lay + 1 < cc.n_layers && *FLASHE_CONSTANT(const uint64_t, &cc.layers[lay + 1].start) < ke) lay = -1;
                }
            }
            u128 p0 = 0, p1 = 0, q0 = 0, q1 = 0;
            uint64_t *const sum_out = SUM ? tb.sum_out[cur] : nullptr;
            u128 d0 = 0, d1 = 0;                                        // DMASK: the first stream's blocks of the lane's two elements (GAPS: their running decrypt mask)
            for (int c = 0; c < n_streams; c++) {
                const CtrPrefix pre = load_prefix(pre_lds, sbase + c);
                const int link = GAPS ? cohort_stream_link(cg, c) : single ? c : c - 1;
                const uint64_t *in = link >= 0 ? tb.in[link0 + link] : nullptr;
                uint64_t *out = link >= 0 ? tb.out[link0 + link] : nullptr;
                u128 x0 = 0, x1 = 0;
                if constexpr (BS > 0) {
                    // (the batched front end: packed before the rounds; row lay >= 0: its parameters in SGPRs, else looked up per lane)
                    if (link >= 0) {
                        const double *const ud = reinterpret_cast<const double *>(in);
                        if (lay >= 0) {
                            const CodecLayer *const L = cc.layers + lay;
                            const uint64_t vs = *FLASHE_CONSTANT(const uint64_t, &L->start), es = *FLASHE_CONSTANT(const uint64_t, cb.rows + 2 * lay),
                                           sz = *FLASHE_CONSTANT(const uint64_t, cb.rows + 2 * lay + 1);
                            const void *const xs = reinterpret_cast<const void *>(*FLASHE_CONSTANT(const uintptr_t, cc.src + static_cast<size_t>(link0 + link) * cc.n_layers + lay));
                            const bool bf64 = *FLASHE_CONSTANT(const int, &L->x_is_f64) != 0;
                            const double b0 = *FLASHE_CONSTANT(const double, &L->p0), b1 = *FLASHE_CONSTANT(const double, &L->p1),
                                         b2 = *FLASHE_CONSTANT(const double, &L->p2);
                            if (a0) x0 = cohort_batch_element<BS>(xs, bf64, b0, b1, b2, ud + vs, (k0 - es) * static_cast<uint64_t>(BS), sz, cb.field_bits);
                            if (a1) x1 = cohort_batch_element<BS>(xs, bf64, b0, b1, b2, ud + vs, (k1 - es) * static_cast<uint64_t>(BS), sz, cb.field_bits);
                        } else {
                            if (a0) x0 = cohort_batch_lane<BS>(cc, cb, link0 + link, k0, ud);
                            if (a1) x1 = cohort_batch_lane<BS>(cc, cb, link0 + link, k1, ud);
                        }
                    }
                } else if constexpr (COHORT) {
                    // (a launch's few half tiles: quantised before the rounds)
                    if (link >= 0) {
                        const double *const ud = reinterpret_cast<const double *>(in);
                        if (lay >= 0) {
                            const CodecLayer *const L = cc.layers + lay;
                            const uint64_t ls = *FLASHE_CONSTANT(const uint64_t, &L->start);
                            const void *const xs = reinterpret_cast<const void *>(*FLASHE_CONSTANT(const uintptr_t, cc.src + static_cast<size_t>(link0 + link) * cc.n_layers + lay));
                            const bool f64 = *FLASHE_CONSTANT(const int, &L->x_is_f64) != 0;
                            const double q0 = *FLASHE_CONSTANT(const double, &L->p0), q1 = *FLASHE_CONSTANT(const double, &L->p1),
                                         q2 = *FLASHE_CONSTANT(const double, &L->p2);
                            if (a0) x0 = cohort_quantize_raw(cohort_load(xs, f64, k0 - ls), f64, q0, q1, q2, *FLASHE_GLOBAL(const double, ud + k0));
                            if (a1) x1 = cohort_quantize_raw(cohort_load(xs, f64, k1 - ls), f64, q0, q1, q2, *FLASHE_GLOBAL(const double, ud + k1));
                        } else {
                            if (a0) x0 = cohort_quantize_lane(cc, link0 + link, k0, *FLASHE_GLOBAL(const double, ud + k0));
                            if (a1) x1 = cohort_quantize_lane(cc, link0 + link, k1, *FLASHE_GLOBAL(const double, ud + k1));
                        }
                    }
                } else if (CODEC && cq.x != nullptr && link >= 0) {
                    if (a0) x0 = codec_quantize(cq, k0);
                    if (a1) x1 = codec_quantize(cq, k1);
                } else if (in != nullptr && in2) {
                    if (a0) x0 = ld128(in + 2 * k0);
                    if (a1) x1 = ld128(in + 2 * k1);
                } else if (in != nullptr) {
                    if (a0) x0 = static_cast<u128>(in[k0]);
                    if (a1) x1 = static_cast<u128>(in[k1]);
                }
                uint32_t s[2][4];
                {
                    const CtrUniform U = ctr_uniform(rk, te0, pre, x3h);
                    ctr_round2(lr, pre.u[0], xv0.v[0], U, s[0]);
                    ctr_round2(lr, pre.u[0], xv1.v[0], U, s[1]);
                }
                aes256_rounds<2, 3>(rk, lr, s, true);
                loads_landed(x0, x1);
                const u128 c0 = words_to_u128(s[0]), c1 = words_to_u128(s[1]);
                const u128 r0 = x0 + (single ? c0 : p0 - c0), r1 = x1 + (single ? c1 : p1 - c1);
                if (CODEC && cq.fout != nullptr) {
                    if (a0 && link >= 0) cq.fout[k0] = codec_unquantize(cq, k0, r0 & mask);
                    if (a1 && link >= 0) cq.fout[k1] = codec_unquantize(cq, k1, r1 & mask);
                } else {
                    if (a0 && out != nullptr) st128(out + 2 * k0, r0 & mask);
                    if (a1 && out != nullptr) st128(out + 2 * k1, r1 & mask);
                }
                if constexpr (SUM) {
                    if (link >= 0) { q0 += r0; q1 += r1; }
                    if (c == n_streams - 1 && sum_out != nullptr) {
                        if (a0) st128_nt(sum_out + 2 * k0, q0 & mask);
                        if (a1) st128_nt(sum_out + 2 * k1, q1 & mask);
                    }
                }
                if constexpr (GAPS) {
                    const uint32_t sbits = cohort_stream_bits(cg, c);
                    if (sbits == 2u) { d0 -= c0; d1 -= c1; } else if (sbits == 1u) { d0 += c0; d1 += c1; }
                    if (c == n_streams - 1 && dmask != nullptr) {
                        if (a0) st128_nt(dmask + 2 * k0, d0 & mask);
                        if (a1) st128_nt(dmask + 2 * k1, d1 & mask);
                    }
                } else if constexpr (DMASK) {
                    if (c == 0) { d0 = c0; d1 = c1; }
                    if constexpr (DEC) {
                        // (the decrypt of the sum stored above, sum + D mod 2^b, where the others store D)
                        if (c == n_streams - 1) {
                            if (a0) st128_nt(dmask + 2 * k0, (q0 + (c0 - d0)) & mask);
                            if (a1) st128_nt(dmask + 2 * k1, (q1 + (c1 - d1)) & mask);
                        }
                    } else if (c == n_streams - 1 && (!COHORT || dmask != nullptr)) {
                        if constexpr (CUT) {
                            uint64_t *const dm = dmask + static_cast<uint64_t>(cur) * cut_stride;
                            if (a0) st128_nt(dm + 2 * k0, (c0 - d0) & mask);
                            if (a1) st128_nt(dm + 2 * k1, (c1 - d1) & mask);
                        } else {
                            if (a0) st128_nt(dmask + 2 * k0, (c0 - d0) & mask);
                            if (a1) st128_nt(dmask + 2 * k1, (c1 - d1) & mask);
                        }
                    }
                }
                p0 = c0; p1 = c1;
            }
        }
    }
