/*
 * lnsfaid_line_link.hip — what sits between and around the line-format encode and decode (include/lnsfaid.h "line-format link",
 * DESIGN.md §3.16): a payload source, a binary symmetric channel on LNSFAID_LINE_HARD words and the error counters on payload
 * streams.  The host forms in lnsfaid_tables.c are the definition; these kernels return the same bytes.
 *
 * Generator (counter-based, stateless):  cwkey(key, C, d) = mix64(mix64(key + d) + (C + 1) * 0xD1B54A32D192ED03),
 * draw(q) = mix64(cwkey + (q + 1) * 0x9E3779B97F4A7C15), C the global codeword number, d = 1 payload, d = 2 channel.
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

#define LK_T 256       /* threads per workgroup of the payload and channel kernels */
#define LK_CW 32u      /* codewords per workgroup */
#define LC_WAVES 4     /* codewords in flight per workgroup of the counter kernel */
#define LC_MAX_WG 2048u

__device__ __forceinline__ uint64_t lk_mix64(uint64_t x)
{
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
__device__ __forceinline__ uint64_t lk_cwkey(uint64_t key, uint64_t C, uint64_t d) { return lk_mix64(lk_mix64(key + d) + (C + 1u) * 0xD1B54A32D192ED03ull); }
__device__ __forceinline__ uint64_t lk_draw(uint64_t cwkey, uint64_t q) { return lk_mix64(cwkey + (q + 1u) * 0x9E3779B97F4A7C15ull); }

template <int V> struct LkVec;
template <> struct LkVec<1> { typedef uint32_t type; };
template <> struct LkVec<2> { typedef uint2 type; };
template <> struct LkVec<4> { typedef uint4 type; };

/* the inversion mask of line word w of a codeword: bit 2 j from the low half of draw 16 w + j, bit 2 j + 1 from the high half */
__device__ __forceinline__ uint32_t lk_flip_mask(uint64_t cwkey, uint32_t w, uint32_t threshold)
{
    uint32_t mask = 0u;
    const uint64_t base = cwkey + ((uint64_t)(16u * w) + 1u) * 0x9E3779B97F4A7C15ull;
#pragma unroll
    for (uint32_t j = 0; j < 16u; ++j) {
        const uint64_t h = lk_mix64(base + (uint64_t)j * 0x9E3779B97F4A7C15ull);
        mask |= ((uint32_t)h < threshold ? 1u : 0u) << (2u * j);
        mask |= ((uint32_t)(h >> 32) < threshold ? 2u : 0u) << (2u * j);
    }
    return mask;
}

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
        sKey[tid] = lk_cwkey(key, first + (uint64_t)cw0 + tid, 2u);
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
            const uint32_t m = lk_flip_mask(ck, w + (uint32_t)i, threshold);
            x[i] ^= m;
            n += (uint32_t)__popc(m);
        }
        vec_t out;
        __builtin_memcpy(&out, x, sizeof(out));
        *(vec_t*)(line_out + at) = out;
        if (n) atomicAdd(&sFlips[c], n);
    }
    __syncthreads();
    if (tid < 64u) { /* wave 0: the codewords' sums out, their sum to the call's total */
        uint32_t n = tid < cws ? sFlips[tid] : 0u;
        if (flips && tid < cws) flips[cw0 + tid] = n;
        for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o);
        if (tid == 0u && n) atomicAdd(total, (unsigned long long)n);
    }
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
    if (tid < LK_CW) sKey[tid] = lk_cwkey(key, first + (uint64_t)cw0 + tid, 1u);
    __syncthreads();
    const uint32_t upc = kw / (uint32_t)V, units = cws * upc;
    const size_t base = (size_t)cw0 * kw;
    for (uint32_t u = tid; u < units; u += LK_T) {
        const uint32_t c = u / upc, w = (u - c * upc) * (uint32_t)V;
        const uint64_t ck = sKey[c];
        uint32_t x[V];
        if (V == 1) {
            const uint64_t h = lk_draw(ck, w >> 1);
            x[0] = (w & 1u) ? (uint32_t)(h >> 32) : (uint32_t)h;
        } else {
#pragma unroll
            for (int i = 0; i < V; i += 2) {
                const uint64_t h = lk_draw(ck, (w + (uint32_t)i) >> 1);
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
    __shared__ unsigned int sAcc[9];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid < 9u) sAcc[tid] = 0u;
    __syncthreads();
    const uint32_t upc = kw / (uint32_t)V;
    /* lane 0's tallies: error frames, error bits, frames with 1 or 2; uncorrectable, corrected codewords, corrected bits;
     * undetected, false alarms */
    uint32_t n_err = 0, n_bits = 0, n_lt3 = 0, n_unc = 0, n_cor = 0, n_cbits = 0, n_und = 0, n_fa = 0;
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
        if (lane == 0u) {
            if (wrong > 0u) { n_err += 1u; n_bits += wrong; n_lt3 += wrong < 3u ? 1u : 0u; }
            if (stats) {
                const int32_t unsat = stats[cw].unsatisfied, corr = stats[cw].corrected;
                if (unsat > 0) n_unc += 1u;
                else if (unsat == 0 && corr > 0) { n_cor += 1u; n_cbits += (uint32_t)corr; }
                if (wrong > 0u) n_und += unsat == 0 ? 1u : 0u;
                else n_fa += unsat > 0 ? 1u : 0u;
            }
        }
    }
    if (lane == 0u) {
        if (n_err) { atomicAdd(&sAcc[0], n_err); atomicAdd(&sAcc[1], n_bits); atomicAdd(&sAcc[2], n_lt3); }
        if (n_unc) atomicAdd(&sAcc[3], n_unc);
        if (n_cor) { atomicAdd(&sAcc[4], n_cor); atomicAdd(&sAcc[5], n_cbits); }
        if (n_und) atomicAdd(&sAcc[6], n_und);
        if (n_fa) atomicAdd(&sAcc[7], n_fa);
    }
    __syncthreads();
    if (tid == 0u) {
        uint32_t walked = 0; /* the codewords this workgroup walked */
        for (uint32_t cw = blockIdx.x * LC_WAVES; cw < n_cw; cw += gridDim.x * LC_WAVES) walked += n_cw - cw < LC_WAVES ? n_cw - cw : LC_WAVES;
        atomicAdd(&acc[0], (unsigned long long)walked);
        if (sAcc[0]) atomicAdd(&acc[1], (unsigned long long)sAcc[0]);
        if (sAcc[1]) atomicAdd(&acc[2], (unsigned long long)sAcc[1]);
        if (sAcc[2]) atomicAdd(&acc[3], (unsigned long long)sAcc[2]);
        if (stats) {
            atomicAdd(&acc[4], (unsigned long long)walked);
            if (sAcc[3]) atomicAdd(&acc[5], (unsigned long long)sAcc[3]);
            if (sAcc[4]) atomicAdd(&acc[6], (unsigned long long)sAcc[4]);
            if (sAcc[5]) atomicAdd(&acc[7], (unsigned long long)sAcc[5]);
            atomicAdd(&acc[8], (unsigned long long)walked);
            if (sAcc[0]) atomicAdd(&acc[9], (unsigned long long)sAcc[0]);
            if (sAcc[6]) atomicAdd(&acc[10], (unsigned long long)sAcc[6]);
            if (sAcc[7]) atomicAdd(&acc[11], (unsigned long long)sAcc[7]);
        }
    }
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
