/*
 * lnsfaid_demap.hip — received symbols of the caller -> decoder input: the last three stages of the reference's
 * receive chain without the channel in front of them.
 *
 *   CModulate::Demodulation          CModulate.cpp:270-362   max-log: l0 = re, l1 = im, l(2n) = |l(2n-2)| - c_n, l(2n+1) = |l(2n-1)| - c_n
 *   AfterDeModulationDeInterleaver   CModulate.cpp:156-212   position p of a frame carries code bit (N / I) (p mod I) + p div I;
 *                                                            [32][K] information LLRs, then [32][M] parity LLRs
 *   CLDPC::float2LimitChar_4bit      CLDPC.cpp:4553-4573     lnsfaid_quantise.h
 *
 * The kernels are organised by OUTPUT: a thread owns a run of consecutive elements of one frame part (information or parity
 * LLRs of one frame) and writes it once, from complete data - with an interleaver the two nibbles of a packed byte come from
 * symbols that lie I positions apart, and no byte is ever read back or shared between threads.  Three mappings:
 *   DM_STREAM  no interleaver, K and N multiples of the run: the run's stream positions are consecutive, so its symbols are
 *              consecutive floats of rx (16-byte loads), and the run leaves in 16-byte stores.  One store is 16 int8 LLRs or 32
 *              nibbles; 64-QAM takes three stores per run so that a run is a whole number of symbols.
 *   DM_GATHER  any interleaver, K and N multiples of one store: consecutive code bits are I stream positions apart; every element
 *              loads its own level (4 bytes) and folds it as often as its place in the symbol asks.  Neighbouring interleaver
 *              classes read the other floats of the same lines.
 *   DM_NARROW  any code: one int8 element or one packed byte (two elements) per thread.
 * mod_type 1 (one real float per code bit, frame-major, never interleaved) has the addresses of QPSK without interleaver and
 * runs in its instances.
 * Pointer alignment only selects the load / store width (16 / 4 / 1 bytes), never the bytes.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "lnsfaid.h"
#include "lnsfaid_quantise.h"
#include "lnsfaid_launch.h"

#define DM_STREAM 0
#define DM_GATHER 1
#define DM_NARROW 2

/* elements per thread */
template <int Q, bool PACKED, int MODE>
struct DmRun {
    static constexpr uint32_t store = PACKED ? 32u : 16u; /* elements of one 16-byte store */
    static constexpr uint32_t value = MODE == DM_STREAM ? (Q == 6 ? 3u * store : store) : MODE == DM_GATHER ? store : (PACKED ? 2u : 1u);
};

/* c_n of the demapper's level n (n = 1 .. Q / 2 - 1): CModulate.cpp:283-356 */
template <int Q>
__device__ __forceinline__ double fold_offset(uint32_t n)
{
    return Q == 4 ? 0.6324555 : Q == 6 ? (n == 1 ? 0.6172134 : 0.3086067) : (n == 1 ? 0.613568 : n == 2 ? 0.306784 : 0.153392);
}

template <int Q, bool PACKED, int MODE>
__global__ __launch_bounds__(256) void lnsfaid_demap_kernel(const float* __restrict__ rx, float scale, uint32_t N, uint32_t M, uint32_t I,
                                                            uint32_t stride /* N / I */, uint8_t* __restrict__ out)
{
    constexpr uint32_t R = DmRun<Q, PACKED, MODE>::value;
    constexpr uint32_t bytes = PACKED ? R / 2 : R;       /* written by the thread */
    constexpr uint32_t WD = bytes >= 4 ? bytes / 4 : 1u; /* as dwords */
    const uint32_t K = N - M, E = 32u * N;               /* (all positions of a group fit 32 bits: 32 n_var <= 2^21) */
    const uint32_t e0 = (blockIdx.x * 256u + threadIdx.x) * R; /* first element of the run in the group's fixInput order */
    if (e0 >= E) return;
    const size_t g = blockIdx.y;
    const float* in = rx + g * (size_t)(Q == 2 ? E : 2u * (E / Q));
    uint8_t* dst = out + g * (size_t)(PACKED ? E / 2 : E) + (PACKED ? e0 / 2 : e0);
    /* frame and first code bit of the run: the only divisions of the thread */
    uint32_t m, k0;
    if (e0 < 32u * K) { m = e0 / K; k0 = e0 - m * K; }
    else { const uint32_t e1 = e0 - 32u * K; m = e1 / M; k0 = K + (e1 - m * M); }

    uint32_t w[WD];
#pragma unroll
    for (uint32_t j = 0; j < WD; ++j) w[j] = 0u;
#define DM_PUT(i, l)                                                                                                    \
    do {                                                                                                                \
        const uint32_t q_ = (uint32_t)(uint8_t)quantise_4bit((l), scale);                                               \
        if constexpr (PACKED) w[(i) / 8u] |= (q_ & 15u) << (4u * ((i) % 8u)); else w[(i) / 4u] |= q_ << (8u * ((i) % 4u));        \
    } while (0)

    if constexpr (MODE == DM_STREAM) {
        /* positions m N + k0 .. + R - 1: R / Q whole symbols (R, N and k0 are multiples of Q), F consecutive floats */
        constexpr uint32_t F = Q == 2 ? R : 2u * R / Q;
        const uint32_t pos0 = m * N + k0;
        const float* src = in + (Q == 2 ? pos0 : 2u * (pos0 / Q));
        float v[F];
        if (((uintptr_t)rx & 15u) == 0u) { /* (the group's floats and the run's offset are multiples of 4 floats) */
#pragma unroll
            for (uint32_t j = 0; j < F / 4; ++j) {
                const float4 t = ((const float4*)src)[j];
                v[4 * j] = t.x; v[4 * j + 1] = t.y; v[4 * j + 2] = t.z; v[4 * j + 3] = t.w;
            }
        } else {
#pragma unroll
            for (uint32_t j = 0; j < F; ++j) v[j] = src[j];
        }
        if constexpr (Q == 2) {
#pragma unroll
            for (uint32_t i = 0; i < R; ++i) DM_PUT(i, v[i]);
        } else {
#pragma unroll
            for (uint32_t s = 0; s < R / Q; ++s) {
                float l[Q];
                l[0] = v[2 * s];
                l[1] = v[2 * s + 1];
#pragma unroll
                for (uint32_t n = 1; n < Q / 2; ++n) { /* in double, every level stored as float before it feeds the next */
                    l[2 * n] = (float)(fabs((double)l[2 * n - 2]) - fold_offset<Q>(n));
                    l[2 * n + 1] = (float)(fabs((double)l[2 * n - 1]) - fold_offset<Q>(n));
                }
#pragma unroll
                for (uint32_t u = 0; u < Q; ++u) DM_PUT(s * Q + u, l[u]);
            }
        }
    } else {
        /* code bit k = stride kj + kd sits at position p = I kd + kj of its frame; both kept by increments */
        uint32_t kj = k0 / stride, kd = k0 - kj * stride;
        const uint32_t frame = m * N;
#pragma unroll
        for (uint32_t i = 0; i < R; ++i) {
            const uint32_t pos = frame + kd * I + kj;
            const uint32_t s = pos / Q, u = pos - s * Q; /* Q is a constant: shifts, or one multiply for 64-QAM */
            float x = in[2u * s + (u & 1u)];
#pragma unroll
            for (uint32_t n = 1; n < Q / 2; ++n)
                if (n <= (u >> 1)) x = (float)(fabs((double)x) - fold_offset<Q>(n));
            DM_PUT(i, x);
            if (++kd == stride) { kd = 0u; ++kj; }
        }
    }
#undef DM_PUT

    if constexpr (MODE == DM_NARROW) {
        dst[0] = (uint8_t)w[0];
    } else if (((uintptr_t)out & 15u) == 0u) { /* (group size and run offset are multiples of 16 bytes) */
#pragma unroll
        for (uint32_t j = 0; j < WD / 4; ++j) ((uint4*)dst)[j] = make_uint4(w[4 * j], w[4 * j + 1], w[4 * j + 2], w[4 * j + 3]);
    } else if (((uintptr_t)out & 3u) == 0u) {
#pragma unroll
        for (uint32_t j = 0; j < WD; ++j) ((uint32_t*)dst)[j] = w[j];
    } else {
#pragma unroll
        for (uint32_t j = 0; j < 4 * WD; ++j) dst[j] = (uint8_t)(w[j / 4] >> (8u * (j % 4)));
    }
}

template <int Q, bool PACKED, int MODE>
static void demap_launch(const float* d_rx, size_t n_groups, float scale, int n_var, int n_check, int interleave, uint8_t* d_out,
                         hipStream_t stream)
{
    constexpr unsigned R = DmRun<Q, PACKED, MODE>::value;
    const size_t rx_group = Q == 2 ? 32 * (size_t)n_var : 2 * (32 * (size_t)n_var / Q);
    const size_t out_group = 32 * (size_t)n_var / (PACKED ? 2 : 1);
    const unsigned runs = 32u * (unsigned)n_var / R;
    /* grid.y holds at most 65535 groups: more are launched in slices (the kernel indexes its group by blockIdx.y) */
    for (size_t g0 = 0; g0 < n_groups; g0 += 65535) {
        const size_t ng = n_groups - g0 < 65535 ? n_groups - g0 : 65535;
        hipLaunchKernelGGL((lnsfaid_demap_kernel<Q, PACKED, MODE>), dim3((runs + 255u) / 256u, (unsigned)ng), dim3(256), 0, stream,
                           d_rx + g0 * rx_group, scale, (uint32_t)n_var, (uint32_t)n_check, (uint32_t)interleave,
                           (uint32_t)(n_var / interleave), d_out + g0 * out_group);
    }
}

template <int Q, bool PACKED>
static void demap_launch_mode(const float* d_rx, size_t n_groups, float scale, int n_var, int n_check, int interleave, uint8_t* d_out,
                              hipStream_t stream)
{
    /* a run must not cross the K boundary of a frame or a frame boundary: the two parts of a frame are far apart in memory */
    const unsigned K = (unsigned)(n_var - n_check), N = (unsigned)n_var;
    constexpr unsigned rs = DmRun<Q, PACKED, DM_STREAM>::value, rg = DmRun<Q, PACKED, DM_GATHER>::value;
    if (interleave == 1 && K % rs == 0 && N % rs == 0)
        demap_launch<Q, PACKED, DM_STREAM>(d_rx, n_groups, scale, n_var, n_check, interleave, d_out, stream);
    else if (K % rg == 0 && N % rg == 0)
        demap_launch<Q, PACKED, DM_GATHER>(d_rx, n_groups, scale, n_var, n_check, interleave, d_out, stream);
    else
        demap_launch<Q, PACKED, DM_NARROW>(d_rx, n_groups, scale, n_var, n_check, interleave, d_out, stream);
}

/* The caller (lnsfaid_capi.hip) has checked the rules of include/lnsfaid.h: mod_type in {1, 2, 4, 6, 8}, interleave divides n_var,
 * 32 n_var is a multiple of mod_type, packed: n_var and K even, d_rx (and d_out when packed) 4-byte aligned. */
extern "C" hipError_t lf_launch_demap(const float* d_rx, size_t n_groups, int mod_type, float scale, int n_var, int n_check,
                                      int interleave, int packed, void* d_out, hipStream_t stream)
{
    uint8_t* o = (uint8_t*)d_out;
    if (mod_type == 1) { mod_type = 2; interleave = 1; } /* the reference's BPSK branch does not interleave (CSimulate.cpp:121-124) */
#define DM_LAUNCH(Q)                                                                                                       \
    case Q:                                                                                                                \
        if (packed) demap_launch_mode<Q, true>(d_rx, n_groups, scale, n_var, n_check, interleave, o, stream);              \
        else demap_launch_mode<Q, false>(d_rx, n_groups, scale, n_var, n_check, interleave, o, stream);                    \
        break;
    switch (mod_type) {
        DM_LAUNCH(2) DM_LAUNCH(4) DM_LAUNCH(6) DM_LAUNCH(8)
    default: return hipErrorInvalidValue;
    }
#undef DM_LAUNCH
    return hipGetLastError();
}
