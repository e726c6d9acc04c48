/*
 * lnsfaid_capture.hip — error-frame capture (include/lnsfaid.h "error-frame capture"): the frames with wrong
 * information bits leave the device as ordered, compact records; everything else stays where it is.  Replaces the collect-flag
 * branch of CLDPC::CalculateErrors (CLDPC.cpp:4877-4983) for device-resident buffers.
 *
 * Three kernels on one stream, no host decision between them:
 *   flag    shaped like lnsfaid_count_errors_kernel (one workgroup per group, one frame per wave pass, 16-byte loads where the
 *           pointers allow, several loads in flight before the first use): the wrong information and parity decisions of every
 *           codeword into cnt[codeword], and the four counters of lnsfaid_count_errors with one atomic set per workgroup.
 *   rank    one workgroup walks cnt in chunks of 1024 codewords with a carry: an exclusive prefix sum over the
 *           "has a wrong information bit" flags.  The rank of an error frame is the number of error frames with a smaller codeword
 *           index, so slot i of a call always holds the same frame whatever the order in which workgroups ran.
 *   gather  one workgroup per slot; a workgroup whose slot is not stored leaves at once.  Copies the record and the three payload
 *           sections (two source segments each for LLRs and sent bits) into the context's staging buffers.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "lnsfaid.h"
#include "lnsfaid_launch.h"

#define CAP_UNITS 8     /* loads a lane has in flight before the first use */
#define CAP_CHUNK 1024u /* codewords per chunk of the rank kernel = its workgroup size */

__device__ __forceinline__ uint32_t cap_nonzero_bytes(uint32_t x)
{
    return (uint32_t)__popc((((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u);
}
/* bytes that differ, per load width */
__device__ __forceinline__ uint32_t cap_diff(uint4 a, uint4 b)
{
    return cap_nonzero_bytes(a.x ^ b.x) + cap_nonzero_bytes(a.y ^ b.y) + cap_nonzero_bytes(a.z ^ b.z) + cap_nonzero_bytes(a.w ^ b.w);
}
__device__ __forceinline__ uint32_t cap_diff(uint32_t a, uint32_t b) { return cap_nonzero_bytes(a ^ b); }
__device__ __forceinline__ uint32_t cap_diff(uint8_t a, uint8_t b) { return a != b ? 1u : 0u; }
__device__ __forceinline__ void cap_clear(uint4& v) { v = make_uint4(0u, 0u, 0u, 0u); }
__device__ __forceinline__ void cap_clear(uint32_t& v) { v = 0u; }
__device__ __forceinline__ void cap_clear(uint8_t& v) { v = 0u; }

/* this lane's share of the bytes in which d[0 .. bytes) differs from s[0 .. bytes) (s == nullptr: from zero); T: the load */
template <typename T>
__device__ __forceinline__ uint32_t cap_count(const int8_t* __restrict__ d, const int8_t* __restrict__ s, uint32_t bytes, uint32_t lane)
{
    const T* dv = (const T*)d;
    const T* sv = (const T*)s;
    const uint32_t n = bytes / (uint32_t)sizeof(T);
    uint32_t cnt = 0;
    for (uint32_t j0 = 0; j0 < n; j0 += CAP_UNITS * 64u) {
        T x[CAP_UNITS], y[CAP_UNITS];
#pragma unroll
        for (uint32_t u = 0; u < CAP_UNITS; ++u) {
            const uint32_t j = j0 + u * 64u + lane;
            cap_clear(x[u]);
            cap_clear(y[u]);
            if (j < n) {
                x[u] = dv[j];
                if (s) y[u] = sv[j];
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < CAP_UNITS; ++u) cnt += cap_diff(x[u], y[u]);
    }
    return cnt;
}

/* cnt[codeword] = {wrong information decisions, wrong parity decisions}; out: TestFrame, ErrorFrame, ErrorBits, LT3ErrBitFrame */
template <typename T>
__global__ __launch_bounds__(256) void lnsfaid_capture_flag_kernel(const int8_t* __restrict__ decoded, const int8_t* __restrict__ sent,
                                                                   uint32_t N, uint32_t M, uint2* __restrict__ cnt,
                                                                   unsigned long long* __restrict__ out)
{
    __shared__ unsigned int sAcc[3];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, K = N - M;
    if (tid < 3u) sAcc[tid] = 0u;
    __syncthreads();
    const size_t g = blockIdx.x;
    const int8_t* sg = sent ? sent + g * (size_t)(32u * N) : nullptr;
    uint32_t frames_err = 0, bits_err = 0, lt3 = 0;
    for (uint32_t fr = wave; fr < LNSFAID_GROUP; fr += 4u) {
        const size_t cw = g * LNSFAID_GROUP + fr;
        const int8_t* d = decoded + cw * (size_t)N;
        uint32_t info = cap_count<T>(d, sg ? sg + (size_t)fr * K : nullptr, K, lane);
        uint32_t par = cap_count<T>(d + K, sg ? sg + (size_t)32u * K + (size_t)fr * M : nullptr, M, lane);
        for (int o = 32; o > 0; o >>= 1) { info += __shfl_down(info, o); par += __shfl_down(par, o); }
        if (lane == 0u) {
            cnt[cw] = make_uint2(info, par);
            if (info > 0u) { frames_err += 1u; bits_err += info; lt3 += info < 3u ? 1u : 0u; }
        }
    }
    if (lane == 0u) { atomicAdd(&sAcc[0], frames_err); atomicAdd(&sAcc[1], bits_err); atomicAdd(&sAcc[2], lt3); }
    __syncthreads();
    if (tid == 0u) {
        atomicAdd(&out[0], (unsigned long long)LNSFAID_GROUP);
        if (sAcc[0]) {
            atomicAdd(&out[1], (unsigned long long)sAcc[0]);
            atomicAdd(&out[2], (unsigned long long)sAcc[1]);
            if (sAcc[2]) atomicAdd(&out[3], (unsigned long long)sAcc[2]);
        }
    }
}

/* slots[r - skip] = codeword of error frame r for skip <= r < skip + cap; meta = {found, stored}.  One workgroup. */
__global__ __launch_bounds__(CAP_CHUNK) void lnsfaid_capture_rank_kernel(const uint2* __restrict__ cnt, uint32_t n_cw, uint32_t skip,
                                                                         uint32_t cap, uint32_t* __restrict__ slots,
                                                                         unsigned long long* __restrict__ meta)
{
    __shared__ uint32_t sWave[CAP_CHUNK / 64u];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t carry = 0; /* error frames in front of the chunk: every thread keeps the same value */
    for (uint32_t base = 0; base < n_cw; base += CAP_CHUNK) {
        const uint32_t cw = base + tid;
        const bool flag = cw < n_cw && cnt[cw].x > 0u;
        const unsigned long long mask = __ballot(flag);
        if (lane == 0u) sWave[wave] = (uint32_t)__popcll(mask);
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < CAP_CHUNK / 64u; ++w) {
            const uint32_t v = sWave[w];
            before += w < wave ? v : 0u;
            total += v;
        }
        const uint32_t rank = carry + before + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        if (flag && rank >= skip && rank - skip < cap) slots[rank - skip] = cw;
        carry += total;
        __syncthreads(); /* sWave is rewritten by the next chunk */
    }
    if (tid == 0u) {
        const uint32_t left = carry > skip ? carry - skip : 0u;
        meta[0] = carry;
        meta[1] = left < cap ? left : cap;
    }
}

/* n bytes from src (nullptr: zeros) to dst by the whole workgroup, with the widest access dst, src and n are all aligned to */
__device__ __forceinline__ void cap_copy(int8_t* __restrict__ dst, const int8_t* __restrict__ src, uint32_t n, uint32_t tid)
{
    const uintptr_t a = (uintptr_t)dst | (uintptr_t)src | (uintptr_t)n;
    if ((a & 15u) == 0u) {
        for (uint32_t i = tid; i < n / 16u; i += 256u) ((uint4*)dst)[i] = src ? ((const uint4*)src)[i] : make_uint4(0u, 0u, 0u, 0u);
    } else if ((a & 3u) == 0u) {
        for (uint32_t i = tid; i < n / 4u; i += 256u) ((uint32_t*)dst)[i] = src ? ((const uint32_t*)src)[i] : 0u;
    } else {
        for (uint32_t i = tid; i < n; i += 256u) dst[i] = src ? src[i] : (int8_t)0;
    }
}

/* slot i: records[i] and payload[i] = LLRs | decisions | sent bits of codeword slots[i], each n_var bytes in code-bit order */
__global__ __launch_bounds__(256) void lnsfaid_capture_gather_kernel(const int8_t* __restrict__ fix, const int8_t* __restrict__ decoded,
                                                                     const int8_t* __restrict__ sent, uint32_t N, uint32_t M,
                                                                     const uint2* __restrict__ cnt, const uint32_t* __restrict__ slots,
                                                                     const unsigned long long* __restrict__ meta,
                                                                     lnsfaid_error_record* __restrict__ records, int8_t* __restrict__ payload)
{
    const uint32_t slot = blockIdx.x, tid = threadIdx.x, K = N - M;
    if ((unsigned long long)slot >= meta[1]) return; /* the grid is sized before `stored` is known */
    const uint32_t cw = slots[slot], fr = cw % LNSFAID_GROUP;
    const size_t group = (size_t)(cw / LNSFAID_GROUP) * (size_t)(32u * N);
    if (tid == 0u) {
        const uint2 c = cnt[cw];
        lnsfaid_error_record r;
        r.codeword = cw; r.info_errors = c.x; r.parity_errors = c.y; r.reserved = 0u;
        records[slot] = r;
    }
    int8_t* p = payload + (size_t)slot * (size_t)(3u * N);
    const size_t info_at = group + (size_t)fr * K, parity_at = group + (size_t)32u * K + (size_t)fr * M;
    cap_copy(p, fix ? fix + info_at : nullptr, K, tid);
    cap_copy(p + K, fix ? fix + parity_at : nullptr, M, tid);
    cap_copy(p + N, decoded + (size_t)cw * N, N, tid);
    cap_copy(p + 2u * N, sent ? sent + info_at : nullptr, K, tid);
    cap_copy(p + 2u * N + K, sent ? sent + parity_at : nullptr, M, tid);
}

/* The caller (lnsfaid_capi.hip) has checked the rules of include/lnsfaid.h.  d_cnt: n_groups * 32 entries; d_slots, d_records,
 * d_payload: `cap` slots (d_records and d_payload 16-byte aligned); skip <= n_groups * 32; d_out: the four counters, ADDED to;
 * d_meta: {found, stored}, written. */
extern "C" hipError_t lf_launch_capture(const int8_t* d_fix, const int8_t* d_decoded, const int8_t* d_sent, size_t n_groups, int n_var,
                                        int n_check, uint32_t skip, uint32_t cap, uint2* d_cnt, uint32_t* d_slots,
                                        lnsfaid_error_record* d_records, int8_t* d_payload, unsigned long long* d_meta,
                                        unsigned long long* d_out, hipStream_t stream)
{
    const uint32_t N = (uint32_t)n_var, M = (uint32_t)n_check, K = N - M, n_cw = (uint32_t)(n_groups * LNSFAID_GROUP);
    /* every frame part starts a multiple of K, M or N bytes after its base pointer */
    const uintptr_t a = (uintptr_t)d_decoded | (uintptr_t)d_sent | (uintptr_t)K | (uintptr_t)M;
    const dim3 grid((unsigned)n_groups), block(256);
    if ((a & 15u) == 0u) hipLaunchKernelGGL(lnsfaid_capture_flag_kernel<uint4>, grid, block, 0, stream, d_decoded, d_sent, N, M, d_cnt, d_out);
    else if ((a & 3u) == 0u) hipLaunchKernelGGL(lnsfaid_capture_flag_kernel<uint32_t>, grid, block, 0, stream, d_decoded, d_sent, N, M, d_cnt, d_out);
    else hipLaunchKernelGGL(lnsfaid_capture_flag_kernel<uint8_t>, grid, block, 0, stream, d_decoded, d_sent, N, M, d_cnt, d_out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lnsfaid_capture_rank_kernel, dim3(1), dim3(CAP_CHUNK), 0, stream, d_cnt, n_cw, skip, cap, d_slots, d_meta);
    e = hipGetLastError();
    if (e != hipSuccess || cap == 0u) return e;
    hipLaunchKernelGGL(lnsfaid_capture_gather_kernel, dim3(cap), dim3(256), 0, stream, d_fix, d_decoded, d_sent, N, M, d_cnt, d_slots, d_meta,
                       d_records, d_payload);
    return hipGetLastError();
}
