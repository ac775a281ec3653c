// The arithmetic of the per-layer tables behind abi_layers.hip: where a layer ends, how the layers of a model batch into elements, where
// the blocks of one upload and the staged layers lie.  No HIP header, so that tests/host_layer_tables_check.cpp runs it on the host
// under sanitizers (as blockpool.h is).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace flashe_tables {

// one past the last element of layer l: the next layer's start, n behind the last layer (any table of ascending .start)
template <class Layer> inline uint64_t layer_end(const Layer *layers, int n_layers, int l, uint64_t n) { return l + 1 < n_layers ? layers[l + 1].start : n; }

inline size_t up16(size_t bytes) { return (bytes + 15) & ~static_cast<size_t>(15); }

// The elements the layers batch into, every layer padded to whole elements on its own (jzf_quantize.py:166-171): size_of(l) = the
// values of layer l; row(l, elem, value) is told the first element and the first value of every non-empty layer.
template <class SizeOf, class Row> inline uint64_t batched_elems(int n_layers, uint64_t bs, SizeOf &&size_of, Row &&row)
{
    uint64_t e = 0, v = 0;
    for (int l = 0; l < n_layers; l++) {
        const uint64_t size = size_of(l);
        if (size == 0) continue;
        row(l, e, v);
        e += (size + bs - 1) / bs;
        v += size;
    }
    return e;
}

// One client's block of the layer-wise sparsifier's outputs: layer l keeps k[l] of its size[l] values; its residuals lie at byte roff[l]
// and its kept values at byte voff[l] of their buffers, each in the layer's compute type (8 bytes where f64[l], else 4) and aligned to
// it; its locations are entries [koff[l], koff[l] + k[l]).  r_bytes / v_bytes = the block's extent.
struct SparsifyBlock { std::vector<uint64_t> koff, roff, voff; uint64_t total_k = 0, r_bytes = 0, v_bytes = 0; };
template <class IsF64> inline SparsifyBlock sparsify_block_layout(int n_layers, const uint64_t *size, const uint64_t *k, IsF64 &&f64)
{
    SparsifyBlock b;
    b.koff.resize(n_layers); b.roff.resize(n_layers); b.voff.resize(n_layers);
    for (int l = 0; l < n_layers; l++) {
        const uint64_t cs = f64(l) ? 8 : 4;
        b.r_bytes = (b.r_bytes + cs - 1) / cs * cs;
        b.v_bytes = (b.v_bytes + cs - 1) / cs * cs;
        b.koff[l] = b.total_k; b.roff[l] = b.r_bytes; b.voff[l] = b.v_bytes;
        b.r_bytes += size[l] * cs;
        b.v_bytes += k[l] * cs;
        b.total_k += k[l];
    }
    return b;
}

// Several host arrays as one upload: add() appends a copy at the next 16-byte boundary and returns its offset (p == nullptr: zeros).
struct Blob {
    std::vector<char> bytes;
    size_t add(const void *p, size_t n)
    {
        const size_t at = up16(bytes.size());
        bytes.resize(at + n, 0);
        if (p && n) memcpy(bytes.data() + at, p, n);
        return at;
    }
};

// Where the stage pass converts layers to in the workspace: every layer at a 16-byte boundary, in its loop type (double or float).
struct StageSlots {
    std::vector<size_t> at;   // byte offset of every slot
    size_t bytes = 0;         // the workspace they need
    uint64_t total = 0;       // values staged so far (a slot's first value in the pass's flat index)
    size_t add(uint64_t size, bool f64)
    {
        bytes = up16(bytes);
        at.push_back(bytes);
        bytes += static_cast<size_t>(size) * (f64 ? 8 : 4);
        total += size;
        return at.size() - 1;
    }
};

// The block the prepared cohort launches upload behind cohort_stage's tables (8-byte words): the n_clients mask pointers, the n_clients
// ciphertext pointers, two words per batched row (first element, value count), with_groups: one word per row -- the row's first GROUP of
// four elements in the launch that draws inside a batched job (a lane owns a group; a row's last group may hold fewer, batched_groups) --
// then one draw plan of plan_words words per client.  Byte offsets inside the block, and its words; a part that is absent is empty.
struct PreparedBlock { size_t mask, ct, rows, groups, plans, words; };
inline PreparedBlock prepared_block(int n_clients, size_t n_rows = 0, size_t plan_words = 0, bool with_groups = false)
{
    const size_t c = static_cast<size_t>(n_clients), groups = 2 * c + 2 * n_rows, plans = groups + (with_groups ? n_rows : 0);
    return PreparedBlock{0, c * 8, 2 * c * 8, groups * 8, plans * 8, plans + plan_words * c};
}
// rows = the (first element, value count) pairs of n_rows rows; first_group[r] = row r's first group; returns the launch's groups
inline uint64_t batched_groups(const uint64_t *rows, size_t n_rows, uint64_t bs, uint64_t *first_group)
{
    uint64_t g = 0;
    for (size_t r = 0; r < n_rows; r++) {
        first_group[r] = g;
        g += ((rows[2 * r + 1] + bs - 1) / bs + 3) / 4;
    }
    return g;
}
// entries of a cohort's n_clients x n_layers source table
inline size_t cohort_sources(int n_clients, int n_layers) { return static_cast<size_t>(n_clients) * static_cast<size_t>(n_layers); }

}  // namespace flashe_tables
