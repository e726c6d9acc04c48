/*
 * lnsfaid_prefec.hip — pre-FEC error counters (include/lnsfaid.h "pre-FEC error counters"): hard decisions on the
 * demapper's levels against the sent bits, counted per bit, per channel symbol and per frame.  Replaces CModulate::ModCalErr
 * (CModulate.cpp:382-437).
 *
 * The kernel is a pure read and is organised by INPUT: the symbols are read contiguously (16 bytes per lane where the pointer
 * allows, several loads in flight before the first use), the sent bits are gathered to them - with an interleaver consecutive
 * stream positions are n_var / I code bits apart, so the sent bytes are the side that is gathered; without one they are
 * consecutive bytes of one frame part and come as dwords where the pointer allows.  One workgroup owns the 32 frames of a group,
 * one wave a frame at a time, so a frame's "any wrong bit" is known before anything is added: registers, then the wave, then
 * LDS, then four global atomics per workgroup on integers (the order of arrival does not change a sum).
 * mod_type 1 (one real float per code bit, never interleaved) has the addresses of QPSK without interleaver and runs in its
 * instances with every bit its own symbol.
 *
 * The second kernel folds the per-frame counts of the device front-end's fused counting (lnsfaid_frontend.hip, COUNT) into the
 * context's accumulator and clears them.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "lnsfaid.h"
#include "lnsfaid_launch.h"

#define PF_UNITS 4 /* loads of 16 bytes a lane has in flight before the first use */

/* c_n of the demapper's level n (n = 1 .. Q / 2 - 1): CModulate.cpp:283-356, the constants of lnsfaid_demap.hip */
template <int Q>
__device__ __forceinline__ double prefec_fold_offset(uint32_t n)
{
    return Q == 4 ? 0.6324555 : Q == 6 ? (n == 1 ? 0.6172134 : 0.3086067) : (n == 1 ? 0.613568 : n == 2 ? 0.306784 : 0.153392);
}

/* Q: bits per symbol; WIDE: two symbols (16 bytes) per load; SENT4: the sent bytes of a load's positions as whole dwords */
template <int Q, bool WIDE, bool SENT4>
__global__ __launch_bounds__(256) void lnsfaid_prefec_kernel(const float* __restrict__ rx, const int8_t* __restrict__ sent, uint32_t N,
                                                             uint32_t M, uint32_t I, uint32_t stride /* N / I */,
                                                             uint32_t k_lim /* K or N: code bits in scope */, uint32_t bit_symbols,
                                                             unsigned long long* __restrict__ out)
{
    constexpr uint32_t W = WIDE ? 2u : 1u; /* symbols of a unit = of one load */
    constexpr uint32_t B = W * (uint32_t)Q; /* its stream positions */
    constexpr bool dwords = SENT4 && B % 4u == 0u;
    constexpr uint32_t SW = dwords ? B / 4u : B; /* registers that hold a unit's sent bytes */
    __shared__ unsigned int sAcc[3];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid < 3u) sAcc[tid] = 0u;
    __syncthreads();
    const uint32_t K = N - M, S = N / (uint32_t)Q, units = S / W; /* (all positions of a group fit 32 bits: 32 n_var <= 2^21) */
    const size_t g = blockIdx.x;
    const float* in = rx + g * (size_t)(64u * S);          /* 2 S floats per frame */
    const int8_t* sg = sent ? sent + g * (size_t)(32u * N) : nullptr;
    uint32_t frames_err = 0, bits_err = 0, syms_err = 0;
    for (uint32_t fr = wave; fr < LNSFAID_GROUP; fr += 4u) {
        const float* f = in + (size_t)fr * (2u * S);
        uint32_t cnt = 0;
        for (uint32_t j0 = 0; j0 < units; j0 += PF_UNITS * 64u) {
            float v[PF_UNITS][2 * W];
            uint32_t sb[PF_UNITS][SW], scope[PF_UNITS]; /* scope: bit t set = position t of the unit takes part */
#pragma unroll
            for (uint32_t u = 0; u < PF_UNITS; ++u) {
                const uint32_t j = j0 + u * 64u + lane;
                const bool ok = j < units;
#pragma unroll
                for (uint32_t t = 0; t < 2 * W; ++t) v[u][t] = 0.0f;
#pragma unroll
                for (uint32_t t = 0; t < SW; ++t) sb[u][t] = 0u;
                scope[u] = 0u;
                if (!ok) continue;
                if constexpr (WIDE) {
                    const float4 x = ((const float4*)f)[j];
                    v[u][0] = x.x; v[u][1] = x.y; v[u][2] = x.z; v[u][3] = x.w;
                } else {
                    v[u][0] = f[2u * j]; v[u][1] = f[2u * j + 1u];
                }
                const uint32_t p0 = j * B; /* first position of the unit inside its frame */
                if constexpr (dwords) {
                    /* no interleaver, K a multiple of B: code bits p0 .. p0 + B - 1 lie in one frame part */
                    scope[u] = p0 < k_lim ? (1u << B) - 1u : 0u;
                    if (sg && scope[u]) {
                        const uint32_t* s4 = (const uint32_t*)(sg + (p0 < K ? fr * K + p0 : 32u * K + fr * M + (p0 - K)));
#pragma unroll
                        for (uint32_t t = 0; t < SW; ++t) sb[u][t] = s4[t];
                    }
                } else {
                    /* position p = I fd + fi carries code bit stride fi + fd; both kept by increments */
                    uint32_t fd = p0 / I, fi = p0 - fd * I;
#pragma unroll
                    for (uint32_t t = 0; t < B; ++t) {
                        const uint32_t k = stride * fi + fd;
                        if (k < k_lim) {
                            scope[u] |= 1u << t;
                            if (sg) sb[u][t] = (uint32_t)(int32_t)sg[k < K ? fr * K + k : 32u * K + fr * M + (k - K)];
                        }
                        if (++fi == I) { fi = 0u; ++fd; }
                    }
                }
            }
#pragma unroll
            for (uint32_t u = 0; u < PF_UNITS; ++u) {
#pragma unroll
                for (uint32_t w = 0; w < W; ++w) {
                    float l[Q];
                    l[0] = v[u][2 * w];
                    l[1] = v[u][2 * w + 1];
#pragma unroll
                    for (uint32_t n = 1; n < Q / 2; ++n) { /* in double, every level stored as float before it feeds the next */
                        l[2 * n] = (float)(fabs((double)l[2 * n - 2]) - prefec_fold_offset<Q>(n));
                        l[2 * n + 1] = (float)(fabs((double)l[2 * n - 1]) - prefec_fold_offset<Q>(n));
                    }
                    uint32_t wrong = 0;
#pragma unroll
                    for (uint32_t t = 0; t < (uint32_t)Q; ++t) {
                        const uint32_t e = w * (uint32_t)Q + t;
                        int32_t b;
                        if constexpr (dwords) b = (int32_t)(int8_t)(sb[u][e / 4u] >> (8u * (e % 4u)));
                        else b = (int32_t)sb[u][e];
                        const int32_t d = l[t] > 0.0f ? 1 : 0;
                        wrong += ((scope[u] >> e) & 1u) & (d != b ? 1u : 0u);
                    }
                    cnt += wrong;
                    syms_err += bit_symbols ? wrong : (wrong ? 1u : 0u);
                }
            }
        }
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o);
        if (lane == 0u && cnt > 0u) { frames_err += 1u; bits_err += cnt; }
    }
    for (int o = 32; o > 0; o >>= 1) syms_err += __shfl_down(syms_err, o);
    if (lane == 0u) { atomicAdd(&sAcc[0], frames_err); atomicAdd(&sAcc[1], bits_err); atomicAdd(&sAcc[2], syms_err); }
    __syncthreads();
    if (tid == 0u) {
        atomicAdd(&out[0], (unsigned long long)LNSFAID_GROUP);
        if (sAcc[0]) {
            atomicAdd(&out[1], (unsigned long long)sAcc[0]);
            atomicAdd(&out[2], (unsigned long long)sAcc[1]);
            atomicAdd(&out[3], (unsigned long long)sAcc[2]);
        }
    }
}

template <int Q>
static void prefec_launch(const float* d_rx, const int8_t* d_sent, size_t n_groups, uint32_t N, uint32_t M, uint32_t I, uint32_t k_lim,
                          uint32_t bit_symbols, unsigned long long* d_out, hipStream_t stream)
{
    const uint32_t K = N - M, S = N / (uint32_t)Q;
    /* a frame is 2 S floats: with S even every frame of every group starts on a multiple of 16 bytes when rx does */
    const bool wide = ((uintptr_t)d_rx & 15u) == 0u && S % 2u == 0u;
    const uint32_t B = (wide ? 2u : 1u) * (uint32_t)Q;
    /* all offsets of the sent bytes (32 N per group, K and M per frame, B per unit) are multiples of 4 */
    const bool sent4 = I == 1u && B % 4u == 0u && K % B == 0u && M % 4u == 0u && ((uintptr_t)d_sent & 3u) == 0u;
    const dim3 grid((unsigned)n_groups), block(256);
#define PF_GO(WIDE, SENT4)                                                                                                      \
    hipLaunchKernelGGL((lnsfaid_prefec_kernel<Q, WIDE, SENT4>), grid, block, 0, stream, d_rx, d_sent, N, M, I, N / I, k_lim,  \
                       bit_symbols, d_out)
    if (wide) { if (sent4) PF_GO(true, true); else PF_GO(true, false); }
    else { if (sent4) PF_GO(false, true); else PF_GO(false, false); }
#undef PF_GO
}

/* The caller (lnsfaid_capi.hip) has checked the rules of include/lnsfaid.h: mod_type in {1, 2, 4, 6, 8} dividing n_var (mod_type 1:
 * n_var even, which every code of a context is), interleave dividing n_var, scope 1 or 2, d_rx 4-byte aligned.  d_out: four
 * counters, ADDED to. */
extern "C" hipError_t lf_launch_prefec(const float* d_rx, const int8_t* d_sent, size_t n_groups, int mod_type, int n_var, int n_check,
                                       int interleave, int scope, unsigned long long* d_out, hipStream_t stream)
{
    const uint32_t N = (uint32_t)n_var, M = (uint32_t)n_check;
    const uint32_t k_lim = scope == LNSFAID_PREFEC_INFO ? N - M : N;
    uint32_t bit_symbols = 0u, I = (uint32_t)interleave;
    if (mod_type == 1) { mod_type = 2; I = 1u; bit_symbols = 1u; } /* the reference's BPSK branch does not interleave */
    switch (mod_type) {
    case 2: prefec_launch<2>(d_rx, d_sent, n_groups, N, M, I, k_lim, bit_symbols, d_out, stream); break;
    case 4: prefec_launch<4>(d_rx, d_sent, n_groups, N, M, I, k_lim, bit_symbols, d_out, stream); break;
    case 6: prefec_launch<6>(d_rx, d_sent, n_groups, N, M, I, k_lim, bit_symbols, d_out, stream); break;
    case 8: prefec_launch<8>(d_rx, d_sent, n_groups, N, M, I, k_lim, bit_symbols, d_out, stream); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

/* ---- fused counting of the device front-end: per-frame counts -> accumulator ------------------------------------------------
 * frame_cnt[stream * 32 + frame] = wrong bits | wrong symbols << 32 of one front-end call (atomics of the front-end's workgroups,
 * which span frame boundaries).  Adds {32 per stream, frames with a wrong bit, bits, symbols} to acc and clears the counts. */
__global__ __launch_bounds__(256) void lnsfaid_prefec_fold_kernel(unsigned long long* __restrict__ frame_cnt, uint32_t n,
                                                                  unsigned long long* __restrict__ acc)
{
    __shared__ unsigned int sAcc[3];
    const uint32_t tid = threadIdx.x;
    if (tid < 3u) sAcc[tid] = 0u;
    __syncthreads();
    uint32_t frames = 0, bits = 0, syms = 0;
    for (uint32_t i = blockIdx.x * 256u + tid; i < n; i += gridDim.x * 256u) {
        const unsigned long long c = frame_cnt[i];
        if (c) {
            frame_cnt[i] = 0ull;
            frames += (uint32_t)c ? 1u : 0u;
            bits += (uint32_t)c;
            syms += (uint32_t)(c >> 32);
        }
    }
    for (int o = 32; o > 0; o >>= 1) { frames += __shfl_down(frames, o); bits += __shfl_down(bits, o); syms += __shfl_down(syms, o); }
    if ((tid & 63u) == 0u && bits) { atomicAdd(&sAcc[0], frames); atomicAdd(&sAcc[1], bits); atomicAdd(&sAcc[2], syms); }
    __syncthreads();
    if (tid == 0u) {
        if (blockIdx.x == 0u) atomicAdd(&acc[0], (unsigned long long)n);
        if (sAcc[1]) {
            atomicAdd(&acc[1], (unsigned long long)sAcc[0]);
            atomicAdd(&acc[2], (unsigned long long)sAcc[1]);
            atomicAdd(&acc[3], (unsigned long long)sAcc[2]);
        }
    }
}

extern "C" hipError_t lf_launch_prefec_fold(unsigned long long* d_frame_cnt, size_t n_streams, unsigned long long* d_acc, hipStream_t stream)
{
    const uint32_t n = (uint32_t)(n_streams * LNSFAID_GROUP);
    /* a workgroup folds at most 2048 counts of at most n_var < 2^16 bits each: its 32-bit partial sums stay below 2^27 */
    const uint32_t blocks = (n + 2047u) / 2048u;
    hipLaunchKernelGGL(lnsfaid_prefec_fold_kernel, dim3(blocks ? blocks : 1u), dim3(256), 0, stream, d_frame_cnt, n, d_acc);
    return hipGetLastError();
}
