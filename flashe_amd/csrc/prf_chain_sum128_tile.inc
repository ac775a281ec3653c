// The whole-tile path of prf_dmask_sum128_kernel (kernels.hip), included inside prf_chain_body.inc in place of the general whole
// tile: the summed double-mask chain at int_bits = 128 with one-limb plaintexts, every output and every input present, and the
// chain's n x 16 B below 4 GiB (launch_prf_chains checks all of it).  The general path pays, per block and stream, for what this
// shape never needs -- the SINGLE selects, the `& mask` of every stored value, a 64-bit address per access, the select that keeps
// the first stream, a 128-bit running sum and per-lane range predicates -- about 60 VALU per block beside the ~310 of the AES.
// Here (DESIGN.md 4.1):
//   - stream 0 is peeled: it only computes S_first, which stays in registers;
//   - streams 1 .. n-1 store ct = pt + S_prev - S_cur and accumulate the PLAINTEXTS only (96-bit per element: lo += x, hi += carry),
//     since sum_c ct_c telescopes to sum_c pt_c + S_first - S_last; the last stream writes D = S_last - S_first and
//     sum = sum_c pt_c - D -- the same bytes as the general path (everything mod 2^128);
//   - every access is a buffer access: one 32-bit byte offset per lane and pair serves all streams and arrays, only the SGPR
//     descriptor changes from stream to stream;
//   - DEC (prf_dec_sum128_kernel): the last stream stores dec = sum + D = sum_c pt_c where the others store D;
//   - the range predicates exist only in the chain's first and last tile (EDGE); interior tiles have all 256 counters in range.
{
    const uint32_t cnt = static_cast<uint32_t>(tb.count[cur]);
    const uint32_t k0 = static_cast<uint32_t>(tj - first) + lane;          // pair 0's first element (wraps below first: EDGE predicates it)
    const uint32_t v8 = 8u * k0, v16 = 16u * k0;                           // byte offsets into the plaintexts / the 16-byte arrays
    const uint32_t x3 = static_cast<uint32_t>(tj) ^ rk.w[3];
    const uint32_t jl = static_cast<uint32_t>(tj) + lane;
    const auto tile = [&](auto edge_tag) {
        constexpr bool EDGE = decltype(edge_tag)::value;
        // the pair loop stays rolled (one copy of the AES per stream); its per-pair state is picked by a scalar branch on the
        // wave-uniform p instead of the register rotation of the general path: two moves per pair instead of fourteen
        const uint32_t vA0 = T3(jl ^ rk.w[3], SEL_B0), vA1 = T3((jl + 64u) ^ rk.w[3], SEL_B0);
        const uint32_t vB0 = T3((jl + 128u) ^ rk.w[3], SEL_B0), vB1 = T3((jl + 192u) ^ rk.w[3], SEL_B0);
        const auto live = [&](int p) { const uint64_t jb = tj + 128u * p; return !EDGE || (jb < end && jb + 128u > first); };
        const auto blocks = [&](int p, const CtrPrefix &pre, const CtrUniform &U, u128 &c0, u128 &c1) {
            uint32_t w0, w1;
            if (p == 0) { w0 = vA0; w1 = vA1; } else { w0 = vB0; w1 = vB1; }
            uint32_t s[2][4];
            ctr_round2(lr, pre.u[0], w0, U, s[0]);
            ctr_round2(lr, pre.u[0], w1, U, s[1]);
            aes256_rounds<2, 3>(rk, lr, s, true);
            c0 = words_to_u128(s[0]); c1 = words_to_u128(s[1]);
        };
        // stream 0: S_first of the lane's four elements, kept to the end
        u128 fA0 = 0, fA1 = 0, fB0 = 0, fB1 = 0;
        {
            const CtrPrefix pre = load_prefix(pre_lds, sbase);
            const CtrUniform U = ctr_uniform(rk, te0, pre, x3);
#pragma unroll 1
            for (int p = 0; p < 2; p++) {
                if (live(p)) {
                    u128 c0, c1;
                    blocks(p, pre, U, c0, c1);
                    if (p == 0) { fA0 = c0; fA1 = c1; } else { fB0 = c0; fB1 = c1; }
                }
            }
        }
        u128 pA0 = fA0, pA1 = fA1, pB0 = fB0, pB1 = fB1;                   // the previous stream's blocks
        uint64_t sA0 = 0, sA1 = 0, sB0 = 0, sB1 = 0;                       // sum of the plaintexts: low 64 bits ...
        uint32_t hA0 = 0, hA1 = 0, hB0 = 0, hB1 = 0;                       // ... and the carries (at most kMaxLinks of them)
        const auto rsum = buf_rsrc(tb.sum_out[cur], 16u * cnt), rdm = buf_rsrc(dmask, 16u * cnt);
        for (int c = 1; c < n_streams; c++) {
            const CtrPrefix pre = load_prefix(pre_lds, sbase + c);
            const CtrUniform U = ctr_uniform(rk, te0, pre, x3);
            const auto rin = buf_rsrc(tb.in[link0 + c - 1], 8u * cnt), rout = buf_rsrc(tb.out[link0 + c - 1], 16u * cnt);
            const bool last_stream = c == n_streams - 1;
#pragma unroll 1
            for (int p = 0; p < 2; p++) {
                if (live(p)) {
                    const uint32_t o8 = v8 + 1024u * p, o16 = v16 + 2048u * p;     // the pair's byte offsets
                    bool a0 = true, a1 = true;
                    if constexpr (EDGE) { a0 = k0 + 128u * p < cnt; a1 = k0 + 128u * p + 64u < cnt; }
                    // (as in the general path: the loads are consumed on every path, their wait sits after the AES)
                    uint64_t x0 = 0, x1 = 0;
                    if (a0) x0 = buf_ld64(rin, o8);
                    if (a1) x1 = buf_ld64(rin, o8 + 512u);
                    u128 c0, c1;
                    blocks(p, pre, U, c0, c1);
                    loads_landed(x0, x1);
                    const auto finish = [&](u128 &p0, u128 &p1, uint64_t &s0, uint32_t &h0, uint64_t &s1, uint32_t &h1, const u128 &f0,
                                            const u128 &f1) {
                        if (a0) buf_st128(rout, o16, x0 + (p0 - c0));
                        if (a1) buf_st128(rout, o16 + 1024u, x1 + (p1 - c1));
                        add96(s0, h0, x0); add96(s1, h1, x1);
                        if (last_stream) {
                            const u128 d0 = c0 - f0, d1 = c1 - f1;
                            if constexpr (DEC) {
                                // the decrypt of the sum stored beside it: dec = sum + D = (join96(s, h) - D) + D mod 2^128 -- the
                                // plaintexts' sum the lane already holds -- in place of D (rdm addresses dec_out)
                                const u128 t0 = join96(s0, h0), t1 = join96(s1, h1);
                                if (a0) { buf_st128<2>(rdm, o16, t0); buf_st128<2>(rsum, o16, t0 - d0); }
                                if (a1) { buf_st128<2>(rdm, o16 + 1024u, t1); buf_st128<2>(rsum, o16 + 1024u, t1 - d1); }
                            } else {
                                if (a0) { buf_st128<2>(rdm, o16, d0); buf_st128<2>(rsum, o16, join96(s0, h0) - d0); }
                                if (a1) { buf_st128<2>(rdm, o16 + 1024u, d1); buf_st128<2>(rsum, o16 + 1024u, join96(s1, h1) - d1); }
                            }
                        }
                        p0 = c0; p1 = c1;
                    };
                    if (p == 0) finish(pA0, pA1, sA0, hA0, sA1, hA1, fA0, fA1);
                    else finish(pB0, pB1, sB0, hB0, sB1, hB1, fB0, fB1);
                }
            }
        }
    };
    if (tj < first || tj + 256u > end) tile(std::true_type{});
    else tile(std::false_type{});
}
