// The chain tables of the cohort launches: the links, the one uncut summed chain over whole vectors, the pieces of a cut cohort.  Every
// builder takes the table as a template parameter -- ChainTable and SmallChainTable (kernels.hip) go through the same text -- and there is
// no HIP header, so that tests/host_cohort_chain_table_check.cpp runs them on the host under sanitizers over stand-in tables (as
// cohort_streams.h and cohort_cut.h are).  E: the ciphertexts' element, uint64_t or the compact layout's uint32_t.
#pragma once
#include <type_traits>
#include "cohort_cut.h"
#include "cohort_streams.h"

namespace flashe_tables {

// link l: client l's draws at u_dev + l * u_stride (a batched or sparse job's u_stride exceeds the chain's elements) and its ciphertext
template <class T, class E>
inline void cohort_chain_links(T &tb, int n_vec, const double *u_dev, uint64_t u_stride, E *const *out_dev)
{
    for (int l = 0; l < n_vec; l++) {
        tb.in[l] = reinterpret_cast<const uint64_t *>(u_dev + static_cast<uint64_t>(l) * u_stride);
        tb.out[l] = reinterpret_cast<uint64_t *>(out_dev[l]);
    }
}

// the int_bits <= 64 tables: `chains` chains that each run over all the vector's AES blocks
template <class T> inline void cohort_chain_blocks(T &tb, int chains, uint64_t blocks)
{
    for (int k = 0; k < chains; k++) { tb.blk_first[k] = 0; tb.blk_count[k] = blocks; }
}

// ONE uncut summed double-mask chain over elements [0, n) of n_vec clients: chain 0 over the streams of st (cohort_streams of the clients'
// cipher indices: n_vec + runs), `tiles` tiles per stream, its sum in sum_out_dev, and the links
template <class T, class E>
inline void cohort_whole_chain(T &tb, const CohortStreams &st, int n_vec, uint64_t n, uint64_t tiles, const double *u_dev, uint64_t u_stride,
                               E *const *out_dev, E *sum_out_dev)
{
    const int n_streams = static_cast<int>(st.idx.size());
    tb.first[0] = 0; tb.count[0] = n;
    tb.len[0] = static_cast<uint8_t>(n_vec);
    for (int s = 0; s < n_streams; s++) tb.idx[s] = st.idx[s];
    tb.sum_out[0] = reinterpret_cast<uint64_t *>(sum_out_dev);
    tb.wend[0] = tiles * static_cast<uint64_t>(n_streams);
    cohort_chain_links(tb, n_vec, u_dev, u_stride, out_dev);
}

// the pieces of a cut cohort as chains of one table: piece p holds the present clients at positions [begins[p], begins[p + 1]) -- one run of
// consecutive cipher indices --, its streams are theirs and the one behind its last client (launch_prf_chains' layout: a cut costs one
// stream).  false, with nothing written past the table, for begins that are not pieces of n_vec clients (cohort_cut_pieces' always are).
template <class T>
inline bool cohort_cut_table(T &tb, int n_vec, int parts, const int *begins, const uint32_t *idx, uint64_t n, uint64_t tiles)
{
    static_assert(std::extent<decltype(T::len)>::value == kCutMaxParts && std::extent<decltype(T::in)>::value == kCutMaxClients, "cohort_cut.h states the limits of one chained launch");
    static_assert(kCutMaxStreams == kCohortMaxStreams && std::extent<decltype(T::idx)>::value == kCohortMaxStreams, "cohort_cut.h and cohort_streams.h state one table's streams");
    int streams = 0;
    uint64_t wend = 0;
    for (int p = 0; p < parts && parts <= kCutMaxParts; p++) {
        const int a = begins[p], len = begins[p + 1] - a;
        if (a < 0 || len < 1 || a + len > n_vec || streams + len + 1 > kCohortMaxStreams) return false;
        tb.first[p] = 0; tb.count[p] = n;
        tb.link0[p] = static_cast<uint16_t>(a); tb.sbase[p] = static_cast<uint16_t>(streams);
        tb.len[p] = static_cast<uint8_t>(len);
        for (int s = 0; s <= len; s++) tb.idx[streams + s] = idx[a] + static_cast<uint32_t>(s);
        wend += tiles * static_cast<uint64_t>(len + 1);
        tb.wend[p] = wend;
        streams += len + 1;
    }
    return parts >= 1 && parts <= kCutMaxParts && streams == n_vec + parts;
}

}  // namespace flashe_tables
