/*
 * lnsfaid_burst_link.hip — the link calls on burst lines and burst payloads (include/lnsfaid.h "burst-format link"):
 * payload source, binary symmetric channel, soft channel and error counters where every codeword c is shortened by its own S_c.  The
 * host forms in lnsfaid_tables.c are the definition; these kernels return the same bytes.
 *
 * Generator: the link's (lnsfaid_link.h), indexed by MOTHER position; d = 1 payload, 2 BSC, 3 soft.  The inversion mask, the soft
 * channel's tree, walk and unit loop, the flip sums and the counter's tallies are the line kernels', from the same header.
 * Word wl of a burst codeword whose known words are [k0w, k0w + Sw) is mother word wi = wl + (wl >= k0w ? Sw : 0) and uses the draws
 * 16 wi .. 16 wi + 15 (payload: half of draw wi / 2) of the line kernels.
 *
 * Shape of the payload and channel kernels (the line kernels', plus a search).  A workgroup of BL_T threads owns BL_CW consecutive
 * codewords.  Threads 0 .. BL_CW load the descriptors: thread t < cws writes codeword t's key, its Sw and its first unit relative to
 * the workgroup's first unit into LDS; threads cws .. BL_CW write the end of the workgroup's last codeword.  The workgroup's units
 * (one unit = one word of 32 positions) are then one contiguous run [0, sOff[cws]) behind `base`, taken with the workgroup's stride,
 * consecutive lanes on consecutive units.  A thread finds the codeword of unit u by a binary search for the last c with sOff[c] <= u:
 * five steps over 32 offsets; a codeword is at least 85 units long, so a wave's 64 units lie in at most two codewords and the LDS
 * reads broadcast.  Accesses are one word wide (a codeword of a burst is only 4-byte aligned); the soft channel writes 16 bytes when
 * the output starts on 16 bytes, since every unit's 16 output bytes then do.
 * Flip sums as in the line kernels: per-codeword integer sums in LDS, plain stores by the owning workgroup, one global atomic per
 * workgroup for the total.  Nothing first-come enters any output.
 *
 * Counter kernel: one wavefront per codeword, as lnsfaid_line_count_kernel; the pointer is payload + pay_off, the length kw - Sw
 * words, and short_ones is read next to stats: failed = unsatisfied > 0 || short_ones > 0.
 *
 * Bounds.  The grid covers n_cw: cw0 = BL_CW * blockIdx.x < n_cw, cws = min(BL_CW, n_cw - cw0) >= 1; descriptors cw0 .. cw0 + cws - 1
 * are read (t >= cws reads descriptor cw0 + cws - 1 again), the highest n_cw - 1.  sOff has BL_CW + 1 entries, written at
 * t = 0 .. BL_CW; sKey, sSw, sFlips are indexed by t < BL_CW or by the search's c.  The search starts at c = 0 and adds 16, 8, 4, 2, 1
 * only while sOff[c + step] <= u, c + step <= 31; sOff[cws .. BL_CW] = units > u for every u of the loop, so c <= cws - 1 < BL_CW: the
 * search ends inside the workgroup's codewords, also in the partial last workgroup.  sOff is strictly increasing over 0 .. cws (a
 * codeword keeps L / 32 - Sw >= (L - K) / 32 + 1 > 0 units, (K - S) / 32 >= 1 payload words), so wl = u - sOff[c] < sOff[c + 1] - sOff[c],
 * the codeword's own length, and the mother word wi < L / 32 (payload: < K / 32).  The highest unit touched is base + units - 1 =
 * line_off + (words of the last codeword) - 1 of codeword cw0 + cws - 1; for the last workgroup that is the last word of the caller's
 * burst line (payload), and the soft channel's highest byte 16 * (that unit) + 15 the last byte of its LLR4 burst line.
 * flips[cw0 + t] is written for t < cws only.  sTree: node in 2 .. 15 of 16 words.  Units are below 2^26 (lnsfaid_burst.h).
 * Counter kernel: cw < n_cw; words pay_off .. pay_off + kw - Sw - 1 of the codeword, the burst payload's own; stats[cw],
 * short_ones[cw] with cw < n_cw.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "lnsfaid.h"
#include "lnsfaid_burst.h"
#include "lnsfaid_launch.h"
#include "lnsfaid_link.h"

#define BL_T 256       /* threads per workgroup of the payload and channel kernels */
#define BL_CW 32u      /* codewords per workgroup */
#define BC_WAVES 4     /* codewords in flight per workgroup of the counter kernel */
#define BC_MAX_WG 2048u

/* what a workgroup keeps of its BL_CW codewords */
struct BlFrame {
    uint64_t key[BL_CW];
    uint32_t off[BL_CW + 1u]; /* first unit of codeword t relative to the workgroup's first; [cws .. BL_CW]: the workgroup's units */
    uint32_t sw[BL_CW];       /* S_c / 32 */
    unsigned int flips[BL_CW];
};

/* Fills f (threads 0 .. BL_CW), returns the workgroup's first unit; the caller synchronises.  PAYLOAD: units are payload words
 * (pay_off, kw words per mother codeword), else line units (line_off, lw). */
template <bool PAYLOAD>
__device__ __forceinline__ uint32_t bl_frame(BlFrame& f, const LfBurstDesc* __restrict__ desc, uint32_t cw0, uint32_t cws, uint32_t words,
                                             uint64_t key, uint64_t first, uint64_t domain)
{
    const uint32_t tid = threadIdx.x;
    const LfBurstDesc d0 = desc[cw0]; /* uniform */
    const uint32_t base = PAYLOAD ? d0.pay_off : d0.line_off;
    if (tid <= BL_CW) {
        const uint32_t c = tid < cws ? tid : cws - 1u;
        const LfBurstDesc d = desc[cw0 + c];
        const uint32_t at = (PAYLOAD ? d.pay_off : d.line_off) - base;
        f.off[tid] = tid < cws ? at : at + words - d.s_words;
        if (tid < BL_CW) {
            f.key[tid] = lnk_cwkey(key, first + (uint64_t)cw0 + tid, domain);
            f.sw[tid] = tid < cws ? d.s_words : 0u;
            f.flips[tid] = 0u;
        }
    }
    return base;
}

/* the codeword of unit u < f.off[cws]: the last c with f.off[c] <= u */
__device__ __forceinline__ uint32_t bl_find(const BlFrame& f, uint32_t u)
{
    uint32_t c = 0u;
#pragma unroll
    for (uint32_t step = BL_CW / 2u; step > 0u; step >>= 1)
        if (f.off[c + step] <= u) c += step;
    return c;
}

/* unit u of codeword c -> its mother word; kw = K / 32 */
__device__ __forceinline__ uint32_t bl_mother(const BlFrame& f, uint32_t c, uint32_t u, uint32_t kw, uint32_t where)
{
    const uint32_t wl = u - f.off[c], sw = f.sw[c];
    const uint32_t k0w = where == LNSFAID_SHORTEN_HEAD ? 0u : kw - sw;
    return wl + (wl >= k0w ? sw : 0u);
}

__global__ __launch_bounds__(BL_T) void lnsfaid_burst_payload_kernel(uint32_t* __restrict__ payload, const LfBurstDesc* __restrict__ desc,
                                                                     uint32_t where, uint32_t n_cw, uint32_t kw, unsigned long long key,
                                                                     unsigned long long first)
{
    __shared__ BlFrame f;
    const uint32_t cw0 = blockIdx.x * BL_CW, cws = n_cw - cw0 < BL_CW ? n_cw - cw0 : BL_CW; /* the grid covers n_cw: cw0 < n_cw */
    const uint32_t base = bl_frame<true>(f, desc, cw0, cws, kw, key, first, 1u);
    __syncthreads();
    const uint32_t units = f.off[cws];
    for (uint32_t u = threadIdx.x; u < units; u += BL_T) {
        const uint32_t c = bl_find(f, u), wi = bl_mother(f, c, u, kw, where);
        const uint64_t h = lnk_draw(f.key[c], wi >> 1);
        payload[(size_t)base + u] = (wi & 1u) ? (uint32_t)(h >> 32) : (uint32_t)h;
    }
}

/* line_in == line_out is allowed: a thread reads a word before it writes that word, and no other thread touches it */
__global__ __launch_bounds__(BL_T) void lnsfaid_burst_bsc_kernel(const uint32_t* line_in, uint32_t* line_out, const LfBurstDesc* __restrict__ desc,
                                                                 uint32_t where, uint32_t n_cw, uint32_t lw, uint32_t kw, unsigned long long key,
                                                                 unsigned long long first, uint32_t threshold, uint32_t* __restrict__ flips,
                                                                 unsigned long long* __restrict__ total)
{
    __shared__ BlFrame f;
    const uint32_t cw0 = blockIdx.x * BL_CW, cws = n_cw - cw0 < BL_CW ? n_cw - cw0 : BL_CW;
    const uint32_t base = bl_frame<false>(f, desc, cw0, cws, lw, key, first, 2u);
    __syncthreads();
    const uint32_t units = f.off[cws];
    for (uint32_t u = threadIdx.x; u < units; u += BL_T) {
        const uint32_t c = bl_find(f, u), wi = bl_mother(f, c, u, kw, where);
        const uint32_t m = lnk_flip_mask(f.key[c], wi, threshold);
        line_out[(size_t)base + u] = line_in[(size_t)base + u] ^ m;
        if (m) atomicAdd(&f.flips[c], (unsigned int)__popc(m));
    }
    __syncthreads();
    lnk_flips_out(f.flips, cw0, cws, flips, total);
}

/* A16: llr4_out starts on 16 bytes (every unit's 16 bytes then do), else on 4 */
template <bool A16>
__global__ __launch_bounds__(BL_T) void lnsfaid_burst_soft_kernel(const uint32_t* __restrict__ line_in, uint32_t* __restrict__ llr4_out,
                                                                  const LfBurstDesc* __restrict__ desc, uint32_t where, uint32_t n_cw, uint32_t lw,
                                                                  uint32_t kw, unsigned long long key, unsigned long long first, LnkTable tab,
                                                                  uint32_t* __restrict__ flips, unsigned long long* __restrict__ total)
{
    __shared__ BlFrame f;
    __shared__ uint32_t sTree[16];
    const uint32_t tid = threadIdx.x;
    const uint32_t cw0 = blockIdx.x * BL_CW, cws = n_cw - cw0 < BL_CW ? n_cw - cw0 : BL_CW;
    const uint32_t base = bl_frame<false>(f, desc, cw0, cws, lw, key, first, 3u);
    if (tid == 64u) { /* a lane of the second wave, beside the keys of the first */
#pragma unroll
        for (int k = 1; k < 16; ++k) sTree[k] = lnk_node(tab, k);
    }
    __syncthreads();
    const uint32_t root = tab.t[6];
    const uint32_t units = f.off[cws];
    for (uint32_t u = tid; u < units; u += BL_T) {
        const uint32_t c = bl_find(f, u), wi = bl_mother(f, c, u, kw, where);
        const uint32_t x = line_in[(size_t)base + u];
        const uint64_t q0 = f.key[c] + ((uint64_t)(16u * wi) + 1u) * 0x9E3779B97F4A7C15ull;
        uint32_t out[4], n = 0u;
        LNK_SOFT_UNIT(x, q0, root, sTree, out, n)
        uint32_t* o = llr4_out + 4u * ((size_t)base + u);
        if (A16) {
            *(uint4*)o = make_uint4(out[0], out[1], out[2], out[3]);
        } else {
            o[0] = out[0]; o[1] = out[1]; o[2] = out[2]; o[3] = out[3];
        }
        if (n) atomicAdd(&f.flips[c], n);
    }
    __syncthreads();
    lnk_flips_out(f.flips, cw0, cws, flips, total);
}

/* acc: errors[4], fec[4], vs_sent[4], ADDED to.  sent, stats and short_ones may be null. */
__global__ __launch_bounds__(64 * BC_WAVES) void lnsfaid_burst_count_kernel(const uint32_t* __restrict__ payload, const uint32_t* __restrict__ sent,
                                                                            const lnsfaid_line_stats* __restrict__ stats,
                                                                            const uint32_t* __restrict__ short_ones,
                                                                            const LfBurstDesc* __restrict__ desc, uint32_t n_cw, uint32_t kw,
                                                                            unsigned long long* __restrict__ acc)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    LNK_COUNT_LOCALS()
    for (uint32_t cw = blockIdx.x * BC_WAVES + wave; cw < n_cw; cw += gridDim.x * BC_WAVES) {
        const LfBurstDesc d = desc[cw];
        const uint32_t words = kw - d.s_words;
        const uint32_t* p = payload + (size_t)d.pay_off;
        const uint32_t* s = sent ? sent + (size_t)d.pay_off : nullptr;
        uint32_t wrong = 0u;
        for (uint32_t w = lane; w < words; w += 64u) wrong += (uint32_t)__popc(p[w] ^ (s ? s[w] : 0u));
        for (int o = 32; o > 0; o >>= 1) wrong += __shfl_down(wrong, o);
        LNK_COUNT_TALLY(cw, wrong, const bool failed = unsat > 0 || (short_ones && short_ones[cw] > 0u);, failed, !failed && unsat == 0)
    }
    LNK_COUNT_TAIL(BC_WAVES)
}

/* lnsfaid_launch.h says what the caller has checked */
extern "C" hipError_t lf_launch_burst_payload(uint32_t* d_payload, const LfBurstDesc* d_desc, int where, size_t n_cw, uint32_t kw, uint64_t key,
                                              uint64_t first, hipStream_t stream)
{
    const dim3 grid((unsigned)((n_cw + BL_CW - 1u) / BL_CW)), block(BL_T);
    hipLaunchKernelGGL(lnsfaid_burst_payload_kernel, grid, block, 0, stream, d_payload, d_desc, (uint32_t)where, (uint32_t)n_cw, kw, key, first);
    return hipGetLastError();
}

extern "C" hipError_t lf_launch_burst_bsc(const uint32_t* d_in, uint32_t* d_out, const LfBurstDesc* d_desc, int where, size_t n_cw, uint32_t lw,
                                          uint32_t kw, uint64_t key, uint64_t first, uint32_t threshold, uint32_t* d_flips,
                                          unsigned long long* d_total, hipStream_t stream)
{
    const dim3 grid((unsigned)((n_cw + BL_CW - 1u) / BL_CW)), block(BL_T);
    hipLaunchKernelGGL(lnsfaid_burst_bsc_kernel, grid, block, 0, stream, d_in, d_out, d_desc, (uint32_t)where, (uint32_t)n_cw, lw, kw, key, first,
                       threshold, d_flips, d_total);
    return hipGetLastError();
}

extern "C" hipError_t lf_launch_burst_soft(const uint32_t* d_in, uint8_t* d_out, const LfBurstDesc* d_desc, int where, size_t n_cw, uint32_t lw,
                                           uint32_t kw, uint64_t key, uint64_t first, const uint32_t table[14], uint32_t* d_flips,
                                           unsigned long long* d_total, hipStream_t stream)
{
    const dim3 grid((unsigned)((n_cw + BL_CW - 1u) / BL_CW)), block(BL_T);
    LnkTable tab;
    for (int i = 0; i < 14; ++i) tab.t[i] = table[i];
    if (((uintptr_t)d_out & 15u) == 0u)
        hipLaunchKernelGGL(lnsfaid_burst_soft_kernel<true>, grid, block, 0, stream, d_in, (uint32_t*)d_out, d_desc, (uint32_t)where, (uint32_t)n_cw,
                           lw, kw, key, first, tab, d_flips, d_total);
    else
        hipLaunchKernelGGL(lnsfaid_burst_soft_kernel<false>, grid, block, 0, stream, d_in, (uint32_t*)d_out, d_desc, (uint32_t)where, (uint32_t)n_cw,
                           lw, kw, key, first, tab, d_flips, d_total);
    return hipGetLastError();
}

extern "C" hipError_t lf_launch_burst_count(const uint32_t* d_payload, const uint32_t* d_sent, const lnsfaid_line_stats* d_stats,
                                            const uint32_t* d_short_ones, const LfBurstDesc* d_desc, size_t n_cw, uint32_t kw,
                                            unsigned long long* d_acc, hipStream_t stream)
{
    const size_t wgs = (n_cw + BC_WAVES - 1u) / BC_WAVES;
    const dim3 grid((unsigned)(wgs < BC_MAX_WG ? wgs : BC_MAX_WG)), block(64 * BC_WAVES);
    hipLaunchKernelGGL(lnsfaid_burst_count_kernel, grid, block, 0, stream, d_payload, d_sent, d_stats, d_short_ones, d_desc, (uint32_t)n_cw, kw,
                       d_acc);
    return hipGetLastError();
}
