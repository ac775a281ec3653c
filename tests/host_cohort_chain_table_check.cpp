// Host check of flashe_amd/csrc/cohort_chain_table.h (the chain tables of the cohort launches: the links, the one uncut summed chain, the
// pieces of a cut cohort), built with -fsanitize=address,undefined by tests/test_cohort_chain_table_host.py.  The builders are templates
// over the table, so they run here over two stand-ins with the field names and array sizes of ChainTable and SmallChainTable
// (kernels.hip), pre-filled with a sentinel: every field they should write against closed forms written here on their own, and every
// byte they should not write against the sentinel.
#include "cohort_chain_table.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

using namespace flashe_tables;

#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

constexpr int kChains = 16, kLinks = 128;
struct WideTable {
    uint64_t first[kChains], count[kChains];
    uint64_t wend[kChains];
    uint16_t link0[kChains], sbase[kChains];
    uint8_t len[kChains];
    uint8_t flags[kChains];
    uint32_t idx[kLinks + kChains];
    const uint64_t *in[kLinks];
    uint64_t *out[kLinks];
    uint64_t *sum_out[kChains];
};
struct SmallTable {
    uint64_t first[kChains], count[kChains];
    uint64_t blk_first[kChains], blk_count[kChains];
    uint64_t wend[kChains];
    uint16_t link0[kChains], sbase[kChains];
    uint8_t len[kChains], flags[kChains];
    uint32_t idx[kLinks + kChains];
    const uint64_t *in[kLinks];
    uint64_t *out[kLinks];
    uint64_t *sum_out[kChains];
};

constexpr unsigned char kFill = 0xa5;
template <class T> static void fill(T &tb) { memset(static_cast<void *>(&tb), kFill, sizeof(T)); }
// entries [from, size of the array) of a field still hold the sentinel
template <class A, size_t N> static bool untouched(const A (&field)[N], int from)
{
    for (size_t i = static_cast<size_t>(from); i < N; i++) {
        const unsigned char *b = reinterpret_cast<const unsigned char *>(&field[i]);
        for (size_t k = 0; k < sizeof(A); k++) if (b[k] != kFill) return false;
    }
    return true;
}

// what the launches hand over: every client's draws `stride` apart in one buffer (stride > n, as a batched or a sparse job's) and one
// ciphertext vector per client
constexpr uint64_t kN = 1000, kStride = kN + 3;
static std::vector<double> g_u(kLinks * kStride);
template <class E> struct Outs {
    std::vector<E> mem = std::vector<E>(kLinks + 1);
    std::vector<E *> ptr;
    Outs() { for (int l = 0; l < kLinks; l++) ptr.push_back(&mem[static_cast<size_t>(kLinks - 1 - l)]); }      // (not in the order of l)
    E *sum() { return &mem[kLinks]; }
};

static long g_whole = 0, g_cut = 0;

template <class T, class E> static void check_links(const T &tb, int n_vec, Outs<E> &outs)
{
    for (int l = 0; l < n_vec; l++) {
        CHECK(tb.in[l] == reinterpret_cast<const uint64_t *>(&g_u[static_cast<size_t>(l) * kStride]));
        CHECK(tb.out[l] == reinterpret_cast<uint64_t *>(outs.ptr[static_cast<size_t>(l)]));
    }
    CHECK(untouched(tb.in, n_vec) && untouched(tb.out, n_vec));
}

// ---- the link filler on its own ----
template <class T, class E> static void check_link_filler(int n_vec)
{
    Outs<E> outs;
    T tb;
    fill(tb);
    cohort_chain_links(tb, n_vec, g_u.data(), kStride, outs.ptr.data());
    check_links(tb, n_vec, outs);
    CHECK(untouched(tb.first, 0) && untouched(tb.count, 0) && untouched(tb.wend, 0) && untouched(tb.link0, 0) && untouched(tb.sbase, 0));
    CHECK(untouched(tb.len, 0) && untouched(tb.flags, 0) && untouched(tb.idx, 0) && untouched(tb.sum_out, 0));
}

// ---- the whole chain ----
template <class T> static void check_blocks(T &, int, uint64_t) {}
static void check_blocks(SmallTable &tb, int chains, uint64_t blocks)
{
    CHECK(untouched(tb.blk_first, 0) && untouched(tb.blk_count, 0));
    cohort_chain_blocks(tb, chains, blocks);
    for (int k = 0; k < chains; k++) CHECK(tb.blk_first[k] == 0 && tb.blk_count[k] == blocks);
    CHECK(untouched(tb.blk_first, chains) && untouched(tb.blk_count, chains));
}

template <class T, class E> static void check_whole(const std::vector<uint32_t> &P, uint64_t tiles)
{
    const int n_vec = static_cast<int>(P.size());
    // the closed form of S: every index and the one behind it, once, ascending (64-bit, so that 2^32 - 1 + 1 would not wrap)
    std::set<uint64_t> S;
    for (uint32_t p : P) { S.insert(p); S.insert(static_cast<uint64_t>(p) + 1); }
    CohortStreams st;
    CHECK(cohort_streams(P.data(), n_vec, kCohortMaxStreams, st) == kCohortStreamsOk);
    Outs<E> outs;
    T tb;
    fill(tb);
    cohort_whole_chain(tb, st, n_vec, kN, tiles, g_u.data(), kStride, outs.ptr.data(), outs.sum());
    const int streams = static_cast<int>(S.size());
    CHECK(streams == n_vec + st.runs && streams <= kCohortMaxStreams);
    CHECK(tb.first[0] == 0 && tb.count[0] == kN && tb.len[0] == n_vec);
    int s = 0;
    for (uint64_t want : S) CHECK(tb.idx[s++] == want);
    CHECK(untouched(tb.idx, streams));
    CHECK(tb.wend[0] == tiles * static_cast<uint64_t>(streams));
    CHECK(tb.sum_out[0] == reinterpret_cast<uint64_t *>(outs.sum()));
    check_links(tb, n_vec, outs);
    // one chain: nothing of a second one, and the chain's place in the flat arrays is left as the launcher zeroed it
    CHECK(untouched(tb.first, 1) && untouched(tb.count, 1) && untouched(tb.wend, 1) && untouched(tb.len, 1) && untouched(tb.sum_out, 1));
    CHECK(untouched(tb.link0, 0) && untouched(tb.sbase, 0) && untouched(tb.flags, 0));
    check_blocks(tb, 1, 7 * tiles + 1);
    g_whole++;
}

static void check_whole_all(const std::vector<uint32_t> &P)
{
    check_whole<WideTable, uint64_t>(P, 4);
    check_whole<SmallTable, uint32_t>(P, (1ull << 33) + 5);       // (tiles x streams in 64 bits)
    check_whole<SmallTable, uint64_t>(P, 1);
}

// ---- the cut ----
template <class T> static void check_cut(const std::vector<uint32_t> &idx, int parts, const int *begins, uint64_t tiles)
{
    const int n_vec = static_cast<int>(idx.size());
    T tb;
    fill(tb);
    CHECK(cohort_cut_table(tb, n_vec, parts, begins, idx.data(), kN, tiles));
    int link = 0, streams = 0;
    uint64_t wend = 0;
    for (int p = 0; p < parts; p++) {
        const int len = tb.len[p];
        CHECK(tb.first[p] == 0 && tb.count[p] == kN);
        CHECK(len >= 1 && tb.link0[p] == link && tb.link0[p] == begins[p]);         // [link0, link0 + len) tile [0, n_vec) in order
        CHECK(tb.sbase[p] == streams);                                              // the running sum of len + 1
        for (int s = 0; s <= len; s++) CHECK(tb.idx[streams + s] == static_cast<uint64_t>(idx[static_cast<size_t>(link)]) + static_cast<uint64_t>(s));
        for (int s = 1; s < len; s++) CHECK(idx[static_cast<size_t>(link + s)] == idx[static_cast<size_t>(link)] + static_cast<uint32_t>(s));   // a piece is one run
        wend += tiles * static_cast<uint64_t>(len + 1);
        CHECK(tb.wend[p] == wend);
        link += len; streams += len + 1;
    }
    CHECK(link == n_vec && streams == n_vec + parts && streams <= kCohortMaxStreams);
    CHECK(untouched(tb.idx, streams) && untouched(tb.first, parts) && untouched(tb.count, parts) && untouched(tb.wend, parts));
    CHECK(untouched(tb.link0, parts) && untouched(tb.sbase, parts) && untouched(tb.len, parts));
    CHECK(untouched(tb.flags, 0) && untouched(tb.in, 0) && untouched(tb.out, 0) && untouched(tb.sum_out, 0));
    check_blocks(tb, parts, 3 * tiles);
    g_cut++;
}

static void check_cut_pieces(const std::vector<uint32_t> &P)
{
    for (uint64_t items : {1ull, 4096ull}) {
        int begins[kCutMaxParts + 1];
        const int parts = cohort_cut_pieces(P.data(), static_cast<int>(P.size()), items, 256, begins);
        CHECK(parts >= 1);
        check_cut<WideTable>(P, parts, begins, 4);
        check_cut<SmallTable>(P, parts, begins, (1ull << 33) + 5);
    }
}

static void check_cut_parts()
{
    for (int C : {1, 3, 4, 8, 127, 128})
        for (uint64_t items : {1ull, 4096ull})
            for (uint32_t first_idx : {0u, 0xffffffffu - 129u}) {            // (the last stream of 128 clients: 2^32 - 2)
                const int parts = cohort_cut_parts(C, items, 256);
                CHECK(parts >= 1 && (items != 1 || parts == (C / 4 > 16 ? 16 : C / 4 > 1 ? C / 4 : 1)) && (items != 4096 || parts == 1));
                int begins[kCutMaxParts + 1];
                for (int p = 0; p <= parts; p++) begins[p] = cohort_cut_begin(C, parts, p);
                std::vector<uint32_t> idx;
                for (int c = 0; c < C; c++) idx.push_back(first_idx + static_cast<uint32_t>(c));
                check_cut<WideTable>(idx, parts, begins, 4);
                check_cut<SmallTable>(idx, parts, begins, 1);
            }
}

// begins that are not the pieces of n_vec clients: false, and never a write past the table
static void check_cut_refusals()
{
    std::vector<uint32_t> idx;
    for (uint32_t c = 0; c < 128; c++) idx.push_back(c);
    WideTable tb;
    const int short_of[] = {0, 5}, past[] = {0, 7}, late[] = {1, 6}, back[] = {0, 4, 2, 6}, empty_piece[] = {0, 3, 3, 6};
    fill(tb);
    CHECK(!cohort_cut_table(tb, 6, 1, short_of, idx.data(), kN, 4));
    CHECK(!cohort_cut_table(tb, 6, 1, past, idx.data(), kN, 4));
    CHECK(!cohort_cut_table(tb, 6, 1, late, idx.data(), kN, 4));
    CHECK(!cohort_cut_table(tb, 6, 3, back, idx.data(), kN, 4));
    CHECK(!cohort_cut_table(tb, 6, 3, empty_piece, idx.data(), kN, 4));
    int begins[kCutMaxParts + 2];
    for (int p = 0; p <= kCutMaxParts + 1; p++) begins[p] = p * 7;
    fill(tb);
    CHECK(!cohort_cut_table(tb, 7 * (kCutMaxParts + 1), kCutMaxParts + 1, begins, idx.data(), kN, 4));
    CHECK(!cohort_cut_table(tb, 0, 0, begins, idx.data(), kN, 4));
    CHECK(untouched(tb.first, 0) && untouched(tb.idx, 0) && untouched(tb.len, 0));
}

int main()
{
    for (unsigned subset = 1; subset < 1024; subset++)
        for (uint32_t first_idx : {0u, 0xffffffffu - 11u}) {             // 2^32 - 12: the tenth client is 2^32 - 3, the last stream 2^32 - 2
            std::vector<uint32_t> P;
            for (int c = 0; c < 10; c++)
                if (subset >> c & 1u) P.push_back(first_idx + static_cast<uint32_t>(c));
            check_whole_all(P);
            check_cut_pieces(P);
        }
    // the edges of one table: 128 clients in one run (129 streams), 128 clients in 16 runs (144), and more than 129 streams from fewer
    // clients -- 100 clients in 29 runs (129), 72 singletons (144)
    std::vector<uint32_t> P;
    for (uint32_t c = 0; c < 128; c++) P.push_back(40 + c);
    check_whole_all(P);
    check_cut_pieces(P);
    P.clear();
    for (uint32_t c = 0, at = 0; c < 128; c++) {
        P.push_back(at);
        at += (c % 7 == 6 && c / 7 + 1 < 16) ? 2 : 1;                     // a gap behind every seventh client, 15 of them
    }
    check_whole_all(P);
    check_cut_pieces(P);
    P.clear();
    for (uint32_t c = 0, at = 0; c < 100; c++) {
        P.push_back(at);
        at += c < 28 ? 2 : 1;                                             // 28 singletons, then one run of 72
    }
    check_whole_all(P);
    P.clear();
    for (uint32_t c = 0; c < 72; c++) P.push_back(2 * c);
    check_whole_all(P);
    check_cut_parts();
    check_cut_refusals();
    for (int n_vec : {1, 10, 128}) {
        check_link_filler<WideTable, uint64_t>(n_vec);
        check_link_filler<SmallTable, uint32_t>(n_vec);
        check_link_filler<SmallTable, uint64_t>(n_vec);
    }
    printf("COHORT_CHAIN_TABLE_OK %ld whole chains, %ld cut tables\n", g_whole, g_cut);
    return 0;
}
