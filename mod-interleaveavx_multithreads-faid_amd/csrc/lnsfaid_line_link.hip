/*
 * lnsfaid_line_link.hip — what sits between and around the line-format encode and decode (include/lnsfaid.h "line-format link",
 * DESIGN.md §3.16): a payload source, a binary symmetric channel on LNSFAID_LINE_HARD words and the error counters on payload
 * streams.  The host forms in lnsfaid_tables.c are the definition; these kernels return the same bytes.
 *
 * Generator: the link's (lnsfaid_link.h), domain d = 1 for the payload and d = 2 for the channel.
 *
 * Payload and channel kernels: a workgroup owns LK_CW consecutive codewords.  Their LK_CW keys are computed once, by the first
 * LK_CW threads, and kept in LDS; after that a thread takes units of V output words (V = 4, 2 or 1: the widest the base addresses
 * and the words per codeword allow) with the workgroup's stride, so that a wave's loads and stores are consecutive.  A channel
 * thread makes 16 draws per word, two compares each, and one XOR of the line word; its popcounts go to a per-codeword LDS sum,
 * which the owning workgroup stores - no global atomic but one per workgroup for the total.
 *
 * Counter kernel: one wavefront per codeword, LC_WAVES codewords per workgroup pass.  The 1 824 payload bytes of a 50G-PON codeword
 * are 1.8 wave-wide 16-byte loads per stream: a wave per codeword keeps every load coalesced and needs one plain wave reduction,
 * where several codewords per wave would need a segmented one for lanes that idle a fifth of the time either way.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "lnsfaid.h"
#include "lnsfaid_launch.h"
#include "lnsfaid_link.h"

#define LK_T 256       /* threads per workgroup of the payload and channel kernels */
#define LK_CW 32u      /* codewords per workgroup */
#define LC_WAVES 4     /* codewords in flight per workgroup of the counter kernel */
#define LC_MAX_WG 2048u

template <int V> struct LkVec;
template <> struct LkVec<1> { typedef uint32_t type; };
template <> struct LkVec<2> { typedef uint2 type; };
template <> struct LkVec<4> { typedef uint4 type; };

/* lw: words per codeword (a multiple of V); line_in == line_out is allowed: a thread reads a unit before it writes that unit */
template <int V>
__global__ __launch_bounds__(LK_T) void lnsfaid_line_bsc_kernel(const uint32_t* line_in, uint32_t* line_out, uint32_t n_cw, uint32_t lw,
                                                                unsigned long long key, unsigned long long first, uint32_t threshold,
                                                                uint32_t* __restrict__ flips, unsigned long long* __restrict__ total)
{
    typedef typename LkVec<V>::type vec_t;
    __shared__ uint64_t sKey[LK_CW];
    __shared__ unsigned int sFlips[LK_CW];
    const uint32_t tid = threadIdx.x;
    const uint32_t cw0 = blockIdx.x * LK_CW, cws = n_cw - cw0 < LK_CW ? n_cw - cw0 : LK_CW; /* the grid covers n_cw: cw0 < n_cw */
    if (tid < LK_CW) {
        sKey[tid] = lnk_cwkey(key, first + (uint64_t)cw0 + tid, 2u);
        sFlips[tid] = 0u;
    }
    __syncthreads();
    const uint32_t upc = lw / (uint32_t)V, units = cws * upc;
    const size_t base = (size_t)cw0 * lw;
    for (uint32_t u = tid; u < units; u += LK_T) {
        const uint32_t c = u / upc, w = (u - c * upc) * (uint32_t)V;
        const size_t at = base + (size_t)c * lw + w;
        const vec_t in = *(const vec_t*)(line_in + at);
        uint32_t x[V], n = 0u;
        __builtin_memcpy(x, &in, sizeof(in));
        const uint64_t ck = sKey[c];
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const uint32_t m = lnk_flip_mask(ck, w + (uint32_t)i, threshold);
            x[i] ^= m;
            n += (uint32_t)__popc(m);
        }
        vec_t out;
        __builtin_memcpy(&out, x, sizeof(out));
        *(vec_t*)(line_out + at) = out;
        if (n) atomicAdd(&sFlips[c], n);
    }
    __syncthreads();
    lnk_flips_out(sFlips, cw0, cws, flips, total);
}

/* kw: words per codeword.  V = 4: kw % 4 == 0, V = 2: kw % 2 == 0 - a unit is one or two whole draws; V = 1: a word is half a draw */
template <int V>
__global__ __launch_bounds__(LK_T) void lnsfaid_line_payload_kernel(uint32_t* __restrict__ payload, uint32_t n_cw, uint32_t kw,
                                                                    unsigned long long key, unsigned long long first)
{
    typedef typename LkVec<V>::type vec_t;
    __shared__ uint64_t sKey[LK_CW];
    const uint32_t tid = threadIdx.x;
    const uint32_t cw0 = blockIdx.x * LK_CW, cws = n_cw - cw0 < LK_CW ? n_cw - cw0 : LK_CW;
    if (tid < LK_CW) sKey[tid] = lnk_cwkey(key, first + (uint64_t)cw0 + tid, 1u);
    __syncthreads();
    const uint32_t upc = kw / (uint32_t)V, units = cws * upc;
    const size_t base = (size_t)cw0 * kw;
    for (uint32_t u = tid; u < units; u += LK_T) {
        const uint32_t c = u / upc, w = (u - c * upc) * (uint32_t)V;
        const uint64_t ck = sKey[c];
        uint32_t x[V];
        if (V == 1) {
            const uint64_t h = lnk_draw(ck, w >> 1);
            x[0] = (w & 1u) ? (uint32_t)(h >> 32) : (uint32_t)h;
        } else {
#pragma unroll
            for (int i = 0; i < V; i += 2) {
                const uint64_t h = lnk_draw(ck, (w + (uint32_t)i) >> 1);
                x[i] = (uint32_t)h;
                x[(i + 1) % V] = (uint32_t)(h >> 32);
            }
        }
        vec_t out;
        __builtin_memcpy(&out, x, sizeof(out));
        *(vec_t*)(payload + base + (size_t)c * kw + w) = out;
    }
}

/* acc: errors[4], fec[4], vs_sent[4], ADDED to.  sent and stats may be null. */
template <int V>
__global__ __launch_bounds__(64 * LC_WAVES) void lnsfaid_line_count_kernel(const uint32_t* __restrict__ payload, const uint32_t* __restrict__ sent,
                                                                           const lnsfaid_line_stats* __restrict__ stats, uint32_t n_cw, uint32_t kw,
                                                                           unsigned long long* __restrict__ acc)
{
    typedef typename LkVec<V>::type vec_t;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t upc = kw / (uint32_t)V; /* in front of the tallies: behind them the instances compile to another instruction order */
    LNK_COUNT_LOCALS()
    for (uint32_t cw = blockIdx.x * LC_WAVES + wave; cw < n_cw; cw += gridDim.x * LC_WAVES) {
        const uint32_t* p = payload + (size_t)cw * kw;
        const uint32_t* s = sent ? sent + (size_t)cw * kw : nullptr;
        uint32_t wrong = 0u;
        for (uint32_t u = lane; u < upc; u += 64u) {
            const vec_t a = *(const vec_t*)(p + u * V);
            uint32_t x[V];
            __builtin_memcpy(x, &a, sizeof(a));
            if (s) {
                const vec_t b = *(const vec_t*)(s + u * V);
                uint32_t y[V];
                __builtin_memcpy(y, &b, sizeof(b));
#pragma unroll
                for (int i = 0; i < V; ++i) x[i] ^= y[i];
            }
#pragma unroll
            for (int i = 0; i < V; ++i) wrong += (uint32_t)__popc(x[i]);
        }
        for (int o = 32; o > 0; o >>= 1) wrong += __shfl_down(wrong, o);
        LNK_COUNT_TALLY(cw, wrong, /* no local */, unsat > 0, unsat == 0)
    }
    LNK_COUNT_TAIL(LC_WAVES)
}

/* words per access: 4 when every pointer given starts on 16 bytes and a codeword is a multiple of four words long (its codewords
 * then all start on 16 bytes), 2 likewise for 8 bytes, else 1.  The callers have checked 4-byte alignment. */
static int lk_width(uintptr_t align, uint32_t words)
{
    if ((align & 15u) == 0u && words % 4u == 0u) return 4;
    if ((align & 7u) == 0u && words % 2u == 0u) return 2;
    return 1;
}

/* The caller (lnsfaid_capi.hip) has checked the rules of include/lnsfaid.h; n_cw > 0 and n_cw * words fit 32 bits per workgroup by
 * construction (LK_CW codewords).  d_total: one counter, ADDED to. */
extern "C" hipError_t lf_launch_line_bsc(const uint32_t* d_in, uint32_t* d_out, size_t n_cw, uint32_t lw, uint64_t key, uint64_t first,
                                         uint32_t threshold, uint32_t* d_flips, unsigned long long* d_total, hipStream_t stream)
{
    const dim3 grid((unsigned)((n_cw + LK_CW - 1u) / LK_CW)), block(LK_T);
    switch (lk_width((uintptr_t)d_in | (uintptr_t)d_out, lw)) {
    case 4: hipLaunchKernelGGL(lnsfaid_line_bsc_kernel<4>, grid, block, 0, stream, d_in, d_out, (uint32_t)n_cw, lw, key, first, threshold, d_flips, d_total); break;
    case 2: hipLaunchKernelGGL(lnsfaid_line_bsc_kernel<2>, grid, block, 0, stream, d_in, d_out, (uint32_t)n_cw, lw, key, first, threshold, d_flips, d_total); break;
    default: hipLaunchKernelGGL(lnsfaid_line_bsc_kernel<1>, grid, block, 0, stream, d_in, d_out, (uint32_t)n_cw, lw, key, first, threshold, d_flips, d_total); break;
    }
    return hipGetLastError();
}

extern "C" hipError_t lf_launch_line_payload(uint32_t* d_payload, size_t n_cw, uint32_t kw, uint64_t key, uint64_t first, hipStream_t stream)
{
    const dim3 grid((unsigned)((n_cw + LK_CW - 1u) / LK_CW)), block(LK_T);
    switch (lk_width((uintptr_t)d_payload, kw)) {
    case 4: hipLaunchKernelGGL(lnsfaid_line_payload_kernel<4>, grid, block, 0, stream, d_payload, (uint32_t)n_cw, kw, key, first); break;
    case 2: hipLaunchKernelGGL(lnsfaid_line_payload_kernel<2>, grid, block, 0, stream, d_payload, (uint32_t)n_cw, kw, key, first); break;
    default: hipLaunchKernelGGL(lnsfaid_line_payload_kernel<1>, grid, block, 0, stream, d_payload, (uint32_t)n_cw, kw, key, first); break;
    }
    return hipGetLastError();
}

/* d_acc: twelve counters, ADDED to; d_sent and d_stats may be null */
extern "C" hipError_t lf_launch_line_count(const uint32_t* d_payload, const uint32_t* d_sent, const lnsfaid_line_stats* d_stats, size_t n_cw,
                                           uint32_t kw, unsigned long long* d_acc, hipStream_t stream)
{
    const size_t wgs = (n_cw + LC_WAVES - 1u) / LC_WAVES;
    const dim3 grid((unsigned)(wgs < LC_MAX_WG ? wgs : LC_MAX_WG)), block(64 * LC_WAVES);
    switch (lk_width((uintptr_t)d_payload | (uintptr_t)d_sent, kw)) {
    case 4: hipLaunchKernelGGL(lnsfaid_line_count_kernel<4>, grid, block, 0, stream, d_payload, d_sent, d_stats, (uint32_t)n_cw, kw, d_acc); break;
    case 2: hipLaunchKernelGGL(lnsfaid_line_count_kernel<2>, grid, block, 0, stream, d_payload, d_sent, d_stats, (uint32_t)n_cw, kw, d_acc); break;
    default: hipLaunchKernelGGL(lnsfaid_line_count_kernel<1>, grid, block, 0, stream, d_payload, d_sent, d_stats, (uint32_t)n_cw, kw, d_acc); break;
    }
    return hipGetLastError();
}
