// The middle of the LISTS way back from the packed wire form (prf_small_unpack_lists_kernel, wire.hip; prf_wide_unpack_lists_kernel,
// wire_wide.hip): the rounds whose decrypt has more than one prefix per list -- a round in which a client dropped out (set_idx_list leaves
// one add and one minus prefix per run of uploaders), every round of a single-mask job (one minus prefix per uploader, repeats summed).
//   the table: the round-1 state of a prefix (CtrPrefix, 16 bytes) depends on the iter, which a kernel forms itself (the iter shift of a
//   graph replay), so the host cannot send it: lane k of the first waves computes the state of ITS prefix -- the index is a per-lane
//   operand of ctr_prefix, the twelve lookups of up to 192 prefixes cost what one costs -- and stores it at row k of an LDS table, the
//   adds first, then the minuses (2 x 96 x 16 bytes = 3 KiB beside the 128-KiB T-tables and the 16-KiB rows).
//   the loop: the lane's counter part of round 1 (ctr_var) does not depend on the prefix and is computed once; the table is walked two
//   prefixes at a time -- two wave-uniform 16-byte LDS reads (one broadcast each, no bank conflict) taken to SGPRs, two ctr_round1, one
//   software-pipelined pair of blocks -- and an odd total ends with one single block.  Row k adds while k < n_add and subtracts after.
//   The loop is not unrolled: one pair of blocks in flight is what the 128 VGPRs of a 1024-thread workgroup hold.
#pragma once
#include "device_common.h"

namespace flashe {

// the prefix lists in the kernel argument block (as launch_prf's lists travel): idx[0 .. n_add) add, idx[n_add .. n) subtract
struct WireLists {
    uint32_t idx[2 * kMaxIdx];
    int n_add, n;
};

inline bool wire_lists_admit(int n_add, int n_minus) { return n_add >= 0 && n_minus >= 0 && n_add <= kMaxIdx && n_minus <= kMaxIdx && n_add + n_minus >= 1; }

inline WireLists wire_lists_of(const uint32_t *add, int n_add, const uint32_t *minus, int n_minus)
{
    WireLists ls{};
    for (int k = 0; k < n_add; k++) ls.idx[k] = add[k];
    for (int k = 0; k < n_minus; k++) ls.idx[n_add + k] = minus[k];
    ls.n_add = n_add; ls.n = n_add + n_minus;
    return ls;
}

// pre[k] = the round-1 prefix state of idx[k] (counter high word 0: n < 2^32, host-checked); call after fill_tables, by every thread
__device__ __forceinline__ void wire_prefix_table(const RoundKeys &rk, const LaneRegs lr, uint32_t iter, const WireLists &ls, uint4 *pre)
{
    const int k = static_cast<int>(threadIdx.x);
    if (k < ls.n) {
        const CtrPrefix c = ctr_prefix(rk, lr, iter, ls.idx[k], 0u);
        pre[k] = make_uint4(c.u[0], c.u[1], c.u[2], c.u[3]);
    }
    __syncthreads();
}

// row k (wave-uniform) in SGPRs
__device__ __forceinline__ CtrPrefix wire_prefix_row(const uint4 *pre, int k)
{
    const uint4 v = pre[k];
    return scalar_prefix(CtrPrefix{{v.x, v.y, v.z, v.w}});
}

// D = acc(... acc(acc(0, S_0, 0 < n_add), S_1, 1 < n_add) ..., S_{n-1}, n - 1 < n_add), S_k = the block of prefix k at the lane's counter.
// DEEP: the single block of an odd total through aes256_rounds1_deep (the kernels of int_bits > 64) instead of aes256_rounds<1, 2>.
template <bool DEEP, class Acc>
__device__ __forceinline__ u128 wire_lists_mask(const RoundKeys &rk, const LaneRegs lr, const uint4 *pre, int n_add, int n, const CtrVar &x, const Acc &acc)
{
    u128 D = 0;
    int k = 0;
#pragma unroll 1
    for (; k + 1 < n; k += 2) {
        uint32_t s[2][4];
        ctr_round1(wire_prefix_row(pre, k), x, s[0]);
        ctr_round1(wire_prefix_row(pre, k + 1), x, s[1]);
        aes256_rounds<2, 2>(rk, lr, s, true);
        D = acc(D, words_to_u128(s[0]), k < n_add);
        D = acc(D, words_to_u128(s[1]), k + 1 < n_add);
    }
    if (k < n) {
        uint32_t s[1][4];
        ctr_round1(wire_prefix_row(pre, k), x, s[0]);
        if constexpr (DEEP) aes256_rounds1_deep<2>(rk, lr, s[0], true);
        else aes256_rounds<1, 2>(rk, lr, s, true);
        D = acc(D, words_to_u128(s[0]), k < n_add);
    }
    return D;
}

}  // namespace flashe
