// Host check of the table arithmetic the prepared cohort launches added to flashe_amd/csrc/layer_tables.h (prepared_block, cohort_sources),
// built with -fsanitize=address,undefined by tests/test_prepared_block_host.py.  The block is built the way abi_layers.hip builds it --
// the mask pointers, the ciphertext pointers, then two words per batched row from batched_elems -- appended to a Blob behind tables of
// every size, and read back through the offsets: 1 to 130 clients, 1 to 4 layers of sizes from {0, 1, 4, 5, 6, 8, 13}, bs in {1, 2, 5, 7, 8}.
#include "layer_tables.h"

#include <cstdio>
#include <cstdlib>

using namespace flashe_tables;

#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

static const uint64_t kSizes[] = {0, 1, 4, 5, 6, 8, 13};
static const uint64_t kBs[] = {1, 2, 5, 7, 8};
static const int kClients[] = {1, 2, 3, 10, 127, 128, 129, 130};
static long g_cases = 0;

static void check_block(int n_clients, int n_layers, const uint64_t *size, uint64_t bs, size_t front_bytes)
{
    // what quantize_combine_cohort builds on the host
    std::vector<uint64_t> extra(2 * static_cast<size_t>(n_clients));
    size_t n_rows = 0;
    const uint64_t elems = batched_elems(n_layers, bs, [&](int l) { return size[l]; }, [&](int l, uint64_t elem, uint64_t) {
        extra.push_back(elem); extra.push_back(size[l]); n_rows++;
    });
    for (int c = 0; c < n_clients; c++) {
        extra[static_cast<size_t>(c)] = 0x1000u + 16u * static_cast<uint64_t>(c);
        extra[static_cast<size_t>(n_clients) + c] = 0x900000u + 16u * static_cast<uint64_t>(c);
    }
    const PreparedBlock at = prepared_block(n_clients, n_rows);
    CHECK(at.words == extra.size());
    CHECK(at.mask == 0 && at.ct == 8 * static_cast<size_t>(n_clients) && at.rows == 16 * static_cast<size_t>(n_clients));
    CHECK(at.mask % 8 == 0 && at.ct % 8 == 0 && at.rows % 8 == 0 && at.rows + 16 * n_rows == 8 * at.words);
    CHECK(prepared_block(n_clients).rows == at.rows && prepared_block(n_clients).words == 2 * static_cast<size_t>(n_clients));
    CHECK(at.groups == 8 * at.words && at.plans == 8 * at.words);                      // (no groups, no plans: both empty, at the block's end)
    // behind cohort_stage's tables in one upload: the block starts at a 16-byte boundary and every word is where the kernel reads it
    Blob blob;
    std::vector<char> front(front_bytes, 'x');
    blob.add(front.data(), front.size());
    const size_t src_at = blob.add(nullptr, cohort_sources(n_clients, n_layers) * sizeof(void *));
    const size_t extra_at = blob.add(extra.data(), extra.size() * sizeof(uint64_t));
    CHECK(extra_at % 16 == 0 && extra_at >= src_at + cohort_sources(n_clients, n_layers) * sizeof(void *));
    CHECK(blob.bytes.size() == extra_at + 8 * at.words);
    auto word = [&](size_t byte) { uint64_t v; memcpy(&v, blob.bytes.data() + extra_at + byte, 8); return v; };
    for (int c = 0; c < n_clients; c++) {
        CHECK(word(at.mask + 8 * static_cast<size_t>(c)) == 0x1000u + 16u * static_cast<uint64_t>(c));
        CHECK(word(at.ct + 8 * static_cast<size_t>(c)) == 0x900000u + 16u * static_cast<uint64_t>(c));
    }
    // the rows: the non-empty layers in order, first elements ascending from 0, the counts their sizes, the last row ends at `elems`
    uint64_t e = 0;
    size_t r = 0;
    for (int l = 0; l < n_layers; l++) {
        if (!size[l]) continue;
        CHECK(word(at.rows + 16 * r) == e && word(at.rows + 16 * r + 8) == size[l]);
        e += (size[l] + bs - 1) / bs;
        r++;
    }
    CHECK(r == n_rows && e == elems);
    g_cases++;
}

int main()
{
    CHECK(cohort_sources(1, 1) == 1 && cohort_sources(130, 7) == 910);
    CHECK(cohort_sources(1 << 20, 1 << 12) == (static_cast<size_t>(1) << 32));       // (the product is formed in size_t, not in int)
    uint64_t size[4];
    for (int n_layers = 1; n_layers <= 4; n_layers++) {
        const int combos = n_layers == 1 ? 7 : n_layers == 2 ? 49 : n_layers == 3 ? 343 : 2401;
        for (int code = 0; code < combos; code += (n_layers == 4 ? 5 : 1)) {
            int t = code;
            for (int l = 0; l < n_layers; l++) { size[l] = kSizes[t % 7]; t /= 7; }
            for (uint64_t bs : kBs)
                for (int C : kClients) check_block(C, n_layers, size, bs, static_cast<size_t>((code * 5 + C) % 41));
        }
    }
    printf("PREPARED_BLOCK_OK %ld cases\n", g_cases);
    return 0;
}
