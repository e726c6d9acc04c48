/*
 * lnsfaid_line_soft.hip — the line-format soft channel (include/lnsfaid.h "line-format soft channel"): a binary-input,
 * 15-level, symmetric memoryless channel from LNSFAID_LINE_HARD words to LNSFAID_LINE_LLR4 nibbles.  The host form in
 * lnsfaid_tables.c is the definition; this kernel returns the same bytes.
 *
 * Generator: the link's (lnsfaid_link.h), domain d = 3.  The table struct, the tree's nodes, the walk of one position, the unit loop
 * and the flip sums are there as well: the burst soft kernel (lnsfaid_burst_link.hip) runs the same text.
 *
 * Shape (the BSC kernel's): a workgroup owns LS_CW consecutive codewords; the first LS_CW threads compute their keys into LDS.  A unit
 * is one input word: 16 draws, 32 levels, 16 output bytes.  Units are taken with the workgroup's stride, consecutive lanes on
 * consecutive units, so a wave reads 256 consecutive bytes and writes 1 024.
 *
 * Level of one 32-bit half draw u: m = -7 + #{ i : u >= table[i] }.  The fourteen thresholds arrive by value (scalar registers); one
 * thread lays them out in LDS as the implicit binary tree over [0, table[0], .., table[13]] (node k at word k, children 2 k and 2 k + 1,
 * the leading 0 always counted, so fifteen entries make a full tree), and a position walks it in four steps: compare, node =
 * 2 * node + carry, one ds_read of the next threshold.  The walk keeps the node's byte address, which saves a shift per read, and the
 * root's threshold is compared from its scalar register.  The fifteen words lie in fifteen banks and equal addresses broadcast, so
 * the reads have no bank conflict.  After four steps node - 16 = 1 + the count, m = node - 24.
 * A naive count is 14 compares + 14 carry-adds per position; this walk compiles to 11 vector instructions and 3 ds_read_b32
 * (DESIGN.md §3.17 has the counts of the whole loop: 27.1 vector instructions per position, 40 VGPRs, 448 bytes of LDS).
 * With b the line bit, r = m - b is negative exactly where the channel's decision (level > 0) differs from b, and the level is
 * -(r ^ -b): b ? m : -m.  r and the level are shifted into a word each, nibble by nibble (v_alignbit); the flips of eight positions
 * are one popcount of the sign bits of the r word.
 *
 * Bounds.  The grid covers n_cw: cw0 < n_cw, cws = min(LS_CW, n_cw - cw0) >= 1.  A unit index is below cws * lw, and unit u of the
 * workgroup is input word cw0 * lw + u and output bytes 16 * (cw0 * lw + u) .. + 15 (a codeword's lw words follow one another in both
 * buffers).  The last, partial workgroup therefore reads up to word (cw0 + cws) * lw - 1 = n_cw * lw - 1, the last word of the
 * line, and writes up to byte 16 * n_cw * lw - 1 = n_cw * L / 2 - 1, the last byte of the output.  flips[cw0 + tid] is written for
 * tid < cws only, the highest index n_cw - 1.  sKey, sFlips: index c = u / lw < cws <= LS_CW.  sTree: node in 2 .. 15 of 16 words.
 * cws * lw < 2^32: LS_CW * lw with lw = L / 32 < 2^26.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "lnsfaid.h"
#include "lnsfaid_launch.h"
#include "lnsfaid_link.h"

#define LS_T 256   /* threads per workgroup */
#define LS_CW 32u  /* codewords per workgroup */

/* lw: words per codeword.  A16: llr4_out starts on 16 bytes (every unit's 16 bytes then do), else on 4. */
template <bool A16>
__global__ __launch_bounds__(LS_T) void lnsfaid_line_soft_kernel(const uint32_t* __restrict__ line_in, uint32_t* __restrict__ llr4_out, uint32_t n_cw,
                                                                 uint32_t lw, unsigned long long key, unsigned long long first, LnkTable tab,
                                                                 uint32_t* __restrict__ flips, unsigned long long* __restrict__ total)
{
    __shared__ uint64_t sKey[LS_CW];
    __shared__ unsigned int sFlips[LS_CW];
    __shared__ uint32_t sTree[16];
    const uint32_t tid = threadIdx.x;
    const uint32_t cw0 = blockIdx.x * LS_CW, cws = n_cw - cw0 < LS_CW ? n_cw - cw0 : LS_CW; /* the grid covers n_cw: cw0 < n_cw */
    if (tid < LS_CW) {
        sKey[tid] = lnk_cwkey(key, first + (uint64_t)cw0 + tid, 3u);
        sFlips[tid] = 0u;
    }
    if (tid == 64u) { /* a lane of the second wave, beside the keys of the first */
#pragma unroll
        for (int k = 1; k < 16; ++k) sTree[k] = lnk_node(tab, k);
    }
    __syncthreads();
    const uint32_t root = tab.t[6];
    const uint32_t units = cws * lw;
    const size_t base = (size_t)cw0 * lw;
    for (uint32_t u = tid; u < units; u += LS_T) {
        const uint32_t c = u / lw, w = u - c * lw;
        const uint32_t x = line_in[base + u];
        const uint64_t ck = sKey[c];
        const uint64_t q0 = ck + ((uint64_t)(16u * w) + 1u) * 0x9E3779B97F4A7C15ull;
        uint32_t out[4], n = 0u;
        LNK_SOFT_UNIT(x, q0, root, sTree, out, n)
        uint32_t* o = llr4_out + 4u * (base + u);
        if (A16) {
            *(uint4*)o = make_uint4(out[0], out[1], out[2], out[3]);
        } else {
            o[0] = out[0]; o[1] = out[1]; o[2] = out[2]; o[3] = out[3];
        }
        if (n) atomicAdd(&sFlips[c], n);
    }
    __syncthreads();
    lnk_flips_out(sFlips, cw0, cws, flips, total);
}

/* The caller (lnsfaid_capi.hip) has checked the rules of include/lnsfaid.h: n_cw > 0, the pointers on 4 bytes, the table non-decreasing,
 * the two ranges apart.  d_total: one counter, ADDED to. */
extern "C" hipError_t lf_launch_line_soft(const uint32_t* d_in, uint8_t* d_out, size_t n_cw, uint32_t lw, uint64_t key, uint64_t first,
                                          const uint32_t table[14], uint32_t* d_flips, unsigned long long* d_total, hipStream_t stream)
{
    const dim3 grid((unsigned)((n_cw + LS_CW - 1u) / LS_CW)), block(LS_T);
    LnkTable tab;
    for (int i = 0; i < 14; ++i) tab.t[i] = table[i];
    if (((uintptr_t)d_out & 15u) == 0u)
        hipLaunchKernelGGL(lnsfaid_line_soft_kernel<true>, grid, block, 0, stream, d_in, (uint32_t*)d_out, (uint32_t)n_cw, lw, key, first, tab, d_flips, d_total);
    else
        hipLaunchKernelGGL(lnsfaid_line_soft_kernel<false>, grid, block, 0, stream, d_in, (uint32_t*)d_out, (uint32_t)n_cw, lw, key, first, tab, d_flips, d_total);
    return hipGetLastError();
}
