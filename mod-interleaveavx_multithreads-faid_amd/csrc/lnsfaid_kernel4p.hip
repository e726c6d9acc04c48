/*
 * lnsfaid_kernel4p.hip — packed decode I/O: the four-rows-per-lane decoders reading 4-bit LLRs and writing
 * bit-packed hard decisions, plus the conversion kernels of the configurations they do not serve and the packed error counter.
 *
 * Formats (include/lnsfaid.h): llr4 is fixInput packed element by element, two's-complement nibbles, element e in byte e / 2
 * (low nibble when e is even); bits is decodedBits packed, bit b of word w = decodedBits[32 w + b], n_var / 32 words per codeword.
 *
 * The decoders are the kernels of lnsfaid_kernel4.hip (group rule) and lnsfaid_kernel4cw.hip (per-codeword rule,
 * 3.3b) with two differences:
 *   - staging reads one 16-bit word per lane and block column (four nibbles, variable nodes 4 d .. 4 d + 3), all 23 columns of
 *     a round in flight together as in the int8 staging, and widens the nibbles to the bytes the int8 staging would have loaded;
 *   - the output is the hard-decision plane itself: sHard[i] bit b is decodedBits[32 i + b], so the 552 words of a 50G-PON
 *     codeword are stored as they are, 2 208 bytes (the int8 kernels expand every word into 32 bytes, 17 664).
 * They take the int8 kernels' argument structs and reinterpret fix_input / decoded, so the int8 kernels keep their instances,
 * names and instructions.  Everything between staging and output is the same macro text: the kernel frames of
 * lnsfaid_frame4.h around the loops of lnsfaid_rows4.h.
 */
#include <hip/hip_runtime.h>

#include "lnsfaid_frame4.h"
#include "lnsfaid_launch.h"

/* ---- staging from llr4, in the shape of LF4_STAGE_INPUT including its byte path for a buffer that is not dword aligned.  The
 * host refuses such device pointers, so that path does not run; it is kept because the register allocation of the whole kernel
 * follows the shape of the code around the loops.  Without it (and with a plain copy_out for the output) the compiler laid out
 * the stage loop of the group kernel with 815 more VALU instructions per pass: 7 % slower at 3.0 dB. ---- */
#define LF4P_STAGE_INPUT() \
        const uint8_t* gi = (const uint8_t*)a.fix_input + (((size_t)g * (size_t)LNSFAID_GROUP * (size_t)N) >> 1);                        \
        const uint8_t* src_i = gi + (((size_t)lane_in_group * (size_t)K) >> 1);                                                           \
        const uint8_t* src_p = gi + (((size_t)LNSFAID_GROUP * (size_t)K + (size_t)lane_in_group * (size_t)M) >> 1);                       \
        const int first_erased = N - c->puncture_tail;                                                                                    \
        const int nbc = c->nbc;                                                                                                           \
        if ((((size_t)a.fix_input) & 3u) == 0u) {                                                                                        \
            constexpr int SB = 23;                                                                                                        \
            const uint32_t base_d = ((16u * (uint32_t)tid) & 0xffu) + ((uint32_t)tid >> 4);                                               \
            const SwLds lds = SwLds();                                                                                                    \
            for (int cb0 = 0; cb0 < nbc; cb0 += SB) {                                                                                     \
                uint32_t w[SB];                                                                                                           \
_Pragma("unroll")                                                                                                                         \
                for (int u = 0; u < SB; ++u) {                                                                                            \
                    const int cb = cb0 + u;                                                                                               \
                    if (cb < nbc) { /* uniform; a block column is 128 bytes */                                                            \
                        const uint8_t* col = cb * LF_Z < K ? src_i + ((cb * LF_Z) >> 1) : src_p + ((cb * LF_Z - K) >> 1);                 \
                        w[u] = ((const uint16_t*)col)[tid];                                                                               \
                    }                                                                                                                     \
                }                                                                                                                         \
_Pragma("unroll")                                                                                                                         \
                for (int u = 0; u < SB; ++u) {                                                                                            \
                    const int cb = cb0 + u;                                                                                               \
                    if (cb < nbc) {                                                                                                       \
                        const uint32_t h = w[u];                                                                                          \
                        uint32_t x = (h & 0xfu) | ((h & 0xf0u) << 4) | ((h & 0xf00u) << 8) | ((h & 0xf000u) << 12); /* nibble k -> byte k */ \
                        x |= (x & 0x08080808u) * 0x1eu; /* sign-extend: 0x8..0xf -> 0xf8..0xff, no carries between bytes */              \
                        const int lim = first_erased - cb * LF_Z;                                                                         \
                        if (lim < LF_Z) {                                                                                                 \
_Pragma("unroll")                                                                                                                         \
                            for (int k = 0; k < 4; ++k) if (4 * tid + k >= lim) x &= ~(0xffu << (8 * k));                                 \
                        }                                                                                                                 \
                        x = ((x & 0x7f7f7f7fu) + (uint32_t)SW_BIAS_EN * 0x01010101u) ^ (x & 0x80808080u);                                 \
                        const uint32_t ad = (uint32_t)cb * 256u + base_d;                                                                 \
                        lds.wr8(ad, x); lds.wr8(ad + 4u, x >> 8); lds.wr8(ad + 8u, x >> 16); lds.wr8(ad + 12u, x >> 24);                  \
                    }                                                                                                                     \
                }                                                                                                                         \
            }                                                                                                                             \
        } else {                                                                                                                          \
            for (int cb = 0; cb < nbc; ++cb) {                                                                                            \
                uint32_t w = 0;                                                                                                           \
_Pragma("unroll")                                                                                                                         \
                for (int k = 0; k < 4; ++k) {                                                                                             \
                    const int v = cb * LF_Z + tid + 64 * k;                                                                               \
                    const int e = v < K ? v : v - K;                                                                                      \
                    const uint8_t b = (v < K ? src_i : src_p)[e >> 1];                                                                    \
                    int x = (int)((b >> (4 * (e & 1))) & 15u);                                                                            \
                    x = x >= 8 ? x - 16 : x;                                                                                              \
                    if (v >= first_erased) x = 0;                                                                                         \
                    w |= (uint32_t)((x + SW_BIAS_EN) & 0xff) << (8 * k);                                                                  \
                }                                                                                                                         \
                lds4_wr((uint32_t)cb * 256u + 4u * (uint32_t)tid, w);                                                                     \
            }                                                                                                                             \
        }                                                                                                                                 \
    /* end of LF4P_STAGE_INPUT */

/* the plane as packed decisions, in the shape of write_decoded (lnsfaid_rows4.h; see the staging note above): 16-byte stores of
 * four plane words, the reads of nine rounds before the first store; dword stores for an output that is not 16-byte aligned */
__device__ __forceinline__ void write_bits(const uint32_t* sHard, uint32_t* g_out, int N, int tid)
{
    const int nw = N >> 5;
    if (((size_t)g_out) & 15u) {
        for (int i = tid; i < nw; i += LF_T4) g_out[i] = sHard[i];
        return;
    }
    uint4* out = (uint4*)g_out;
    const int n4 = nw >> 2;
    for (int r0 = 0; r0 * LF_T4 < n4; r0 += 9) {
        uint4 w[9];
#pragma unroll
        for (int u = 0; u < 9; ++u) { const int i = (r0 + u) * LF_T4 + tid; w[u] = i < n4 ? make_uint4(sHard[4 * i], sHard[4 * i + 1], sHard[4 * i + 2], sHard[4 * i + 3]) : make_uint4(0u, 0u, 0u, 0u); }
#pragma unroll
        for (int u = 0; u < 9; ++u) { const int i = (r0 + u) * LF_T4 + tid; if (i < n4) out[i] = w[u]; }
    }
}

/* ==== group rule: lnsfaid_kernel4.hip's frame with packed staging and output ==== */
#define LF4_RULE GROUP

template <int METHOD, bool RM, bool EF2>
__global__ __launch_bounds__(LF_T4, 2) void lnsfaid_decode4p_kernel(LfKernelArgs a)
{
    LF4_GROUP_FRAME(LF4P_STAGE_INPUT, write_bits, uint32_t, nw)
}

/* ==== per-codeword rule: lnsfaid_kernel4cw.hip's frame with packed staging and output ==== */
#undef LF4_RULE
#define LF4_RULE CW

template <int METHOD, bool RM, bool EF2>
__global__ __launch_bounds__(LF_T4, 2) void lnsfaid_decode4pcw_kernel(LfCwArgs a)
{
    LF4_LOCALS()
    const int g = cw >> 5, lane_in_group = cw & 31;
    LF4_CW_CORE(LF4P_STAGE_INPUT, a.cw_stats)
    uint32_t* g_out = (uint32_t*)a.decoded + (size_t)cw * (size_t)nw; /* packed decisions */
    write_bits(sHard, g_out, N, tid);
    LF4_CW_RECORDS()
}

/* the packed instances: the same set as lf_decode4_func / lf_decode4cw_func */
extern "C" const void* lf_decode4p_func(int method, int ef, int rm, int per_codeword)
{
    if (per_codeword) {
        LF4_INSTANCE_TABLE(lnsfaid_decode4pcw_kernel)
    }
    LF4_INSTANCE_TABLE(lnsfaid_decode4p_kernel)
}

/* ==== configurations without a packed decoder (two-rows kernel, two waves per codeword): llr4 -> int8 in front of the int8
 * decode, int8 decisions -> bits behind it ==== */

/* eight nibbles (one dword of llr4) -> eight int8 LLRs */
__global__ __launch_bounds__(256) void lnsfaid_unpack_llr4_kernel(const uint32_t* __restrict__ in, uint2* __restrict__ out, size_t n_words)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t w = in[i];
        uint32_t lo = (w & 0xfu) | ((w & 0xf0u) << 4) | ((w & 0xf00u) << 8) | ((w & 0xf000u) << 12);
        const uint32_t h = w >> 16;
        uint32_t hi = (h & 0xfu) | ((h & 0xf0u) << 4) | ((h & 0xf00u) << 8) | ((h & 0xf000u) << 12);
        lo |= (lo & 0x08080808u) * 0x1eu;
        hi |= (hi & 0x08080808u) * 0x1eu;
        out[i] = make_uint2(lo, hi);
    }
}

/* 32 int8 decisions (0 / 1) -> one word, bit b = byte b */
__device__ __forceinline__ uint32_t bytes_to_bits4(uint32_t x) { return (((x & 0x01010101u) * 0x01020408u) >> 24) & 15u; }

__global__ __launch_bounds__(256) void lnsfaid_pack_bits_kernel(const uint4* __restrict__ in, uint32_t* __restrict__ out, size_t n_words)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += (size_t)gridDim.x * blockDim.x) {
        const uint4 a = in[2 * i], b = in[2 * i + 1];
        out[i] = bytes_to_bits4(a.x) | bytes_to_bits4(a.y) << 4 | bytes_to_bits4(a.z) << 8 | bytes_to_bits4(a.w) << 12
            | bytes_to_bits4(b.x) << 16 | bytes_to_bits4(b.y) << 20 | bytes_to_bits4(b.z) << 24 | bytes_to_bits4(b.w) << 28;
    }
}

static unsigned conv_grid(size_t n) { const size_t b = (n + 255) / 256; return (unsigned)(b < 8192 ? (b ? b : 1) : 8192); }

extern "C" hipError_t lf_launch_unpack_llr4(const uint8_t* d_llr4, int8_t* d_fix, size_t n_values, hipStream_t stream)
{
    const size_t n = n_values / 8; /* n_values is a multiple of 32 * 256 */
    hipLaunchKernelGGL(lnsfaid_unpack_llr4_kernel, dim3(conv_grid(n)), dim3(256), 0, stream, (const uint32_t*)d_llr4, (uint2*)d_fix, n);
    return hipGetLastError();
}

extern "C" hipError_t lf_launch_pack_bits(const int8_t* d_decoded, uint32_t* d_bits, size_t n_values, hipStream_t stream)
{
    const size_t n = n_values / 32;
    hipLaunchKernelGGL(lnsfaid_pack_bits_kernel, dim3(conv_grid(n)), dim3(256), 0, stream, (const uint4*)d_decoded, d_bits, n);
    return hipGetLastError();
}

/* ==== CalculateErrors on packed data: lnsfaid_count_errors_kernel with XOR and popcount over the K / 32 information words of a
 * codeword; one workgroup per group of 32, one codeword per wave pass, eight loads per lane in flight ==== */
__global__ __launch_bounds__(256) void lnsfaid_count_errors_packed_kernel(const uint32_t* __restrict__ bits, const uint32_t* __restrict__ msg,
                                                                          int n_words, int k_words, unsigned long long* __restrict__ out)
{
    __shared__ unsigned int sAcc[3];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 3) sAcc[tid] = 0u;
    __syncthreads();
    unsigned int frames_err = 0, bits_err = 0, lt3 = 0;
    for (int fr = wave; fr < LNSFAID_GROUP; fr += 4) {
        const size_t cw = (size_t)blockIdx.x * LNSFAID_GROUP + (size_t)fr;
        const uint32_t* d = bits + cw * (size_t)n_words;
        const uint32_t* r = msg ? msg + cw * (size_t)k_words : nullptr;
        int cnt = 0;
        for (int j0 = 0; j0 < k_words; j0 += 8 * 64) {
            uint32_t x[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int j = j0 + u * 64 + lane;
                x[u] = j < k_words ? d[j] : 0u;
                if (r && j < k_words) x[u] ^= r[j];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) cnt += __popc(x[u]);
        }
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o);
        if (lane == 0 && cnt > 0) { frames_err += 1; bits_err += (unsigned)cnt; lt3 += (cnt < 3) ? 1u : 0u; }
    }
    if (lane == 0) { atomicAdd(&sAcc[0], frames_err); atomicAdd(&sAcc[1], bits_err); atomicAdd(&sAcc[2], lt3); }
    __syncthreads();
    if (tid == 0) {
        atomicAdd(&out[0], (unsigned long long)LNSFAID_GROUP);
        if (sAcc[0]) {
            atomicAdd(&out[1], (unsigned long long)sAcc[0]);
            atomicAdd(&out[2], (unsigned long long)sAcc[1]);
            if (sAcc[2]) atomicAdd(&out[3], (unsigned long long)sAcc[2]);
        }
    }
}

extern "C" hipError_t lf_launch_count_errors_packed(const uint32_t* d_bits, const uint32_t* d_msg, int n_var, int k_info, size_t n_cw,
                                                    unsigned long long* out, hipStream_t stream)
{
    hipLaunchKernelGGL(lnsfaid_count_errors_packed_kernel, dim3((unsigned)(n_cw / LNSFAID_GROUP)), dim3(256), 0, stream, d_bits, d_msg,
                       n_var / 32, k_info / 32, out);
    return hipGetLastError();
}
