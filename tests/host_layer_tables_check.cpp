// Host check of flashe_amd/csrc/layer_tables.h (the arithmetic of the per-layer tables behind abi_layers.hip), built with
// -fsanitize=address,undefined by tests/test_layer_tables_host.py.  Every helper is swept against a closed form written here on its own:
// layer sizes from {0, 1, 4, 5, 6, 8, 13}, 1 to 4 layers, bs in {1, 2, 5, 7, 8}, both compute sizes per layer, k from 0 to the size.
#include "layer_tables.h"

#include <cstdio>
#include <cstdlib>

using namespace flashe_tables;

#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

struct Row { uint64_t start; };

static const uint64_t kSizes[] = {0, 1, 4, 5, 6, 8, 13};
static const uint64_t kBs[] = {1, 2, 5, 7, 8};
static long g_cases = 0;

// [a, a + la) and [b, b + lb) share no byte (empty ranges share none)
static bool apart(uint64_t a, uint64_t la, uint64_t b, uint64_t lb) { return la == 0 || lb == 0 || a + la <= b || b + lb <= a; }

static void check_model(int n_layers, const uint64_t *size)
{
    // ---- layer_end over the starts the sizes give ----
    Row rows[4];
    uint64_t n = 0;
    for (int l = 0; l < n_layers; l++) { rows[l].start = n; n += size[l]; }
    for (int l = 0; l < n_layers; l++) CHECK(layer_end(rows, n_layers, l, n) == rows[l].start + size[l]);
    CHECK(layer_end(rows, n_layers, n_layers - 1, n) == n);

    // ---- batched_elems: sum of ceil(size / bs) over the non-empty layers; the rows are those layers, back to back ----
    for (uint64_t bs : kBs) {
        uint64_t want = 0;
        int nonempty = 0;
        for (int l = 0; l < n_layers; l++)
            if (size[l]) { want += size[l] / bs + (size[l] % bs ? 1 : 0); nonempty++; }
        struct Seen { int layer; uint64_t elem, value; };
        std::vector<Seen> br;
        const auto size_of = [&](int l) { return layer_end(rows, n_layers, l, n) - rows[l].start; };
        CHECK(batched_elems(n_layers, bs, size_of, [&](int l, uint64_t elem, uint64_t value) { br.push_back(Seen{l, elem, value}); }) == want);
        CHECK(static_cast<int>(br.size()) == nonempty);
        uint64_t e = 0, v = 0;
        int last = -1;
        for (const Seen &r : br) {
            CHECK(r.layer > last && size[r.layer] > 0);
            CHECK(r.elem == e && r.value == v && r.value == rows[r.layer].start);
            e += (size[r.layer] + bs - 1) / bs;
            v += size[r.layer];
            last = r.layer;
        }
        CHECK(e == want && v == n);
        g_cases++;
    }

    // ---- the stage slots of every mix of compute sizes: ascending, 16-byte aligned, apart ----
    for (int mask = 0; mask < (1 << n_layers); mask++) {
        StageSlots sl;
        uint64_t total = 0;
        for (int l = 0; l < n_layers; l++) {
            CHECK(sl.total == total);
            CHECK(sl.add(size[l], (mask >> l) & 1) == static_cast<size_t>(l));
            total += size[l];
        }
        CHECK(sl.total == n && static_cast<int>(sl.at.size()) == n_layers);
        for (int l = 0; l < n_layers; l++) {
            const uint64_t bytes = size[l] * (((mask >> l) & 1) ? 8 : 4);
            CHECK(sl.at[l] % 16 == 0 && sl.at[l] + bytes <= sl.bytes);
            if (l) CHECK(sl.at[l] >= sl.at[l - 1]);
            for (int m = 0; m < l; m++) CHECK(apart(sl.at[m], size[m] * (((mask >> m) & 1) ? 8 : 4), sl.at[l], bytes));
        }

        // ---- the sparsifier's block for every k: offsets ascend, aligned to the compute size, apart; locations back to back ----
        // (k runs over 0 .. size in models of one or two layers and in those of three layers with sizes from {0, 1, 5, 8}; in the other
        // models of three layers over the ends and the middle of that range, with four layers over its ends)
        bool full = n_layers <= 3;
        for (int l = 0; l < n_layers && n_layers == 3; l++) full = full && (size[l] <= 1 || size[l] == 5 || size[l] == 8);
        std::vector<uint64_t> ks[4];
        for (int l = 0; l < n_layers; l++)
            for (uint64_t v = 0; v <= size[l]; v++)
                if (full || v == 0 || v == size[l] || (n_layers == 3 && v == (size[l] + 1) / 2)) ks[l].push_back(v);
        size_t ki[4] = {0, 0, 0, 0};
        uint64_t k[4] = {0, 0, 0, 0};
        for (;;) {
            for (int l = 0; l < n_layers; l++) k[l] = ks[l][ki[l]];
            const SparsifyBlock b = sparsify_block_layout(n_layers, size, k, [&](int l) { return ((mask >> l) & 1) != 0; });
            uint64_t kk = 0;
            for (int l = 0; l < n_layers; l++) {
                const uint64_t cs = ((mask >> l) & 1) ? 8 : 4;
                CHECK(b.koff[l] == kk);
                CHECK(b.roff[l] % cs == 0 && b.voff[l] % cs == 0);
                CHECK(b.roff[l] + size[l] * cs <= b.r_bytes && b.voff[l] + k[l] * cs <= b.v_bytes);
                if (l) CHECK(b.roff[l] >= b.roff[l - 1] && b.voff[l] >= b.voff[l - 1]);
                for (int m = 0; m < l; m++) {
                    const uint64_t cm = ((mask >> m) & 1) ? 8 : 4;
                    CHECK(apart(b.roff[m], size[m] * cm, b.roff[l], size[l] * cs));
                    CHECK(apart(b.voff[m], k[m] * cm, b.voff[l], k[l] * cs));
                }
                kk += k[l];
            }
            CHECK(b.total_k == kk);
            // (no padding beyond the alignment: at most 4 bytes in front of every float64 layer)
            uint64_t rmin = 0, vmin = 0;
            for (int l = 0; l < n_layers; l++) { rmin += size[l] * (((mask >> l) & 1) ? 8 : 4); vmin += k[l] * (((mask >> l) & 1) ? 8 : 4); }
            CHECK(b.r_bytes >= rmin && b.r_bytes <= rmin + 4 * static_cast<uint64_t>(n_layers));
            CHECK(b.v_bytes >= vmin && b.v_bytes <= vmin + 4 * static_cast<uint64_t>(n_layers));
            g_cases++;
            int l = 0;
            while (l < n_layers && ki[l] + 1 == ks[l].size()) ki[l++] = 0;
            if (l == n_layers) break;
            ki[l]++;
        }
    }

    // ---- a blob of one block per layer: offsets ascend, 16-byte aligned, apart; the bytes are the sources', a null source is zeros ----
    Blob blob;
    std::vector<std::vector<char>> srcs;
    size_t at[4];
    for (int l = 0; l < n_layers; l++) {
        srcs.emplace_back(size[l], static_cast<char>(0x40 + l));
        at[l] = blob.add(l == 1 ? nullptr : srcs[l].data(), srcs[l].size());
        CHECK(at[l] % 16 == 0 && at[l] + size[l] == blob.bytes.size());
        if (l) CHECK(at[l] >= at[l - 1] + size[l - 1]);
    }
    for (int l = 0; l < n_layers; l++)
        for (uint64_t i = 0; i < size[l]; i++) CHECK(blob.bytes[at[l] + i] == (l == 1 ? 0 : static_cast<char>(0x40 + l)));
    g_cases++;
}

int main()
{
    for (size_t b : {size_t(0), size_t(1), size_t(15), size_t(16), size_t(17), size_t(4095)}) CHECK(up16(b) % 16 == 0 && up16(b) >= b && up16(b) < b + 16);
    uint64_t size[4];
    for (int n_layers = 1; n_layers <= 4; n_layers++) {
        int pick[4] = {0, 0, 0, 0};
        for (;;) {
            for (int l = 0; l < n_layers; l++) size[l] = kSizes[pick[l]];
            check_model(n_layers, size);
            int l = 0;
            while (l < n_layers && pick[l] == 6) pick[l++] = 0;
            if (l == n_layers) break;
            pick[l]++;
        }
    }
    printf("LAYER_TABLES_OK %ld cases\n", g_cases);
    return 0;
}
