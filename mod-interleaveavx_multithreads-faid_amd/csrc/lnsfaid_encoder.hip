/*
 * lnsfaid_encoder.hip — systematic encoder on the GPU (replaces CLDPC::Encode, reference CLDPC.cpp:68-155) and the device
 * frame source of lnsfaid_frontend_random_frames.
 *
 * With H = [A | B] (A: the first K columns, B: the last M), the parity bits of information bits u are p = B^-1 A u.  B is
 * block-circulant and so is B^-1 (derived once per context on the host, lnsfaid_code_parity_inverse): its row a z + t is the
 * first row of block row a rotated by t, so
 *     p[a z + t] = XOR over (b, c) in support(first row of block (a, b)) of s[b z + ((c + t) mod z)],   s = A u.
 * One workgroup of 256 threads encodes one group of 32 frames, bit-sliced: one 32-bit word per code bit, bit l = frame l.
 * Thread t owns row t of every circulant.
 *   1. per information block column cb: the 256 message words go to LDS (from the int8 input, or generated from the stream
 *      key), the circulants of the column are added into s (s[br z + t] ^= u[cb z + (sh + t) mod z]: thread t only ever
 *      touches its own s words), and the 32 x 256 message bytes leave as 16-byte stores;
 *   2. per block row a: p[a z + t] from the support list of B^-1 (wave-uniform: scalar loads) against s in LDS, then the
 *      32 x 256 parity bytes leave as 16-byte stores.
 * LDS: s (M words) + two 256-word staging blocks: 14 KiB for the 50G-PON code.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "lnsfaid_device.h"
#include "lnsfaid_launch.h"

#define ENC_T 256 /* threads per workgroup = circulant size */

/* the splitmix64 finaliser (include/lnsfaid.h, lnsfaid_frontend_random_frames) */
__device__ __forceinline__ unsigned long long enc_mix64(unsigned long long x)
{
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

/* 256 bit-sliced words in LDS -> bytes dst[l * stride + i] = bit l of word i, l < 32, i < 256.  Thread t writes frames
 * t / 16 and t / 16 + 16 at positions 16 (t % 16) .. + 15: sixteen lanes cover 256 contiguous bytes of one frame. */
__device__ __forceinline__ void enc_store_block(const uint32_t* w, int8_t* dst, uint32_t stride, uint32_t t, bool wide)
{
    const uint32_t q = t & 15u, l0 = t >> 4;
    uint32_t v[16];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint4 x = ((const uint4*)w)[4 * q + k];
        v[4 * k] = x.x; v[4 * k + 1] = x.y; v[4 * k + 2] = x.z; v[4 * k + 3] = x.w;
    }
#pragma unroll
    for (uint32_t r = 0; r < 2; ++r) {
        const uint32_t l = l0 + 16u * r;
        uint32_t b[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            b[k] = ((v[4 * k] >> l) & 1u) | (((v[4 * k + 1] >> l) & 1u) << 8) | (((v[4 * k + 2] >> l) & 1u) << 16) | (((v[4 * k + 3] >> l) & 1u) << 24);
        int8_t* d = dst + (size_t)l * stride + 16u * q;
        if (wide) {
            *(uint4*)d = make_uint4(b[0], b[1], b[2], b[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 16; ++k) d[k] = (int8_t)((b[k >> 2] >> (8 * (k & 3))) & 0xffu);
        }
    }
}

/* GEN = false: messages from in ([32][K] int8 per group); GEN = true: from keys[g], and also written to info ([32][K]).
 * out: per group [32][K] then [32][M].  bsup / bsup_off: support of B^-1's first rows, entries b z + c, rows [off[a], off[a + 1]). */
template <bool GEN>
__global__ __launch_bounds__(ENC_T) void lnsfaid_encode_kernel(const LfDevCode* __restrict__ code, const uint32_t* __restrict__ bsup,
                                                             const uint32_t* __restrict__ bsup_off, const int8_t* __restrict__ in,
                                                             const unsigned long long* __restrict__ keys, int8_t* __restrict__ out,
                                                             int8_t* __restrict__ info)
{
    extern __shared__ uint32_t enc_lds[];
    const uint32_t t = threadIdx.x, g = blockIdx.x;
    const uint32_t N = (uint32_t)code->n_var, M = (uint32_t)code->n_check, K = N - M;
    const uint32_t kb = K / LF_Z, mb = M / LF_Z;
    uint32_t* s = enc_lds;
    uint32_t* stage = enc_lds + M; /* two blocks of 256 words */
    int8_t* out_g = out + (size_t)g * 32u * N;
    int8_t* info_g = GEN ? info + (size_t)g * 32u * K : nullptr;
    const int8_t* in_g = GEN ? nullptr : in + (size_t)g * 32u * K;
    /* K, M, N are multiples of 256: 16-byte stores whenever the buffer starts on 16 bytes */
    const bool wide_out = ((uintptr_t)out % 16u) == 0;
    const bool wide_info = GEN && ((uintptr_t)info % 16u) == 0;
    const bool wide_in = !GEN && ((uintptr_t)in % 4u) == 0;
    const unsigned long long hk = GEN ? enc_mix64(keys[g]) : 0ull;
    for (uint32_t a = 0; a < mb; ++a) s[a * LF_Z + t] = 0u;

    /* 1. s = A u, message bytes out */
#pragma unroll 1
    for (uint32_t cb = 0; cb < kb; ++cb) {
        uint32_t* ub = stage + (cb & 1u) * LF_Z;
        if (GEN) {
            const unsigned long long j = (unsigned long long)(cb * LF_Z + t);
            ub[t] = (uint32_t)enc_mix64(hk + (j + 1ull) * 0x9E3779B97F4A7C15ull);
        } else {
            /* wave w reads frames 8 w .. 8 w + 7, lane i positions 4 i .. 4 i + 3 (one dword per frame, 256 contiguous bytes
             * per wave and frame) and writes byte w of those four words: the frame bits 8 w .. 8 w + 7 */
            const uint32_t w = t >> 6, i = t & 63u;
            uint32_t by[4] = { 0u, 0u, 0u, 0u };
#pragma unroll
            for (uint32_t f = 0; f < 8; ++f) {
                const int8_t* src = in_g + (size_t)(8u * w + f) * K + cb * LF_Z + 4u * i;
                uint32_t x;
                if (wide_in) x = *(const uint32_t*)src;
                else x = (uint32_t)(uint8_t)src[0] | ((uint32_t)(uint8_t)src[1] << 8) | ((uint32_t)(uint8_t)src[2] << 16) | ((uint32_t)(uint8_t)src[3] << 24);
#pragma unroll
                for (int k = 0; k < 4; ++k) by[k] |= ((x >> (8 * k)) & 1u) << f;
            }
            uint8_t* ubb = (uint8_t*)ub;
#pragma unroll
            for (int k = 0; k < 4; ++k) ubb[(4u * i + (uint32_t)k) * 4u + w] = (uint8_t)by[k];
        }
        __syncthreads(); /* ub complete; the other block is free again (every thread has passed the previous barrier) */
        const uint32_t cw = (uint32_t)code->col_weight[cb];
        for (uint32_t k = 0; k < cw; ++k) {
            const uint32_t c = code->colcirc[cb][k], br = c & 0xffu, sh = c >> 8;
            s[br * LF_Z + t] ^= ub[(sh + t) & (LF_Z - 1)];
        }
        enc_store_block(ub, out_g + cb * LF_Z, K, t, wide_out);
        if (GEN) enc_store_block(ub, info_g + cb * LF_Z, K, t, wide_info);
    }
    __syncthreads(); /* s complete */

    /* 2. p = B^-1 s, parity bytes out */
    int8_t* par_g = out_g + (size_t)32u * K;
#pragma unroll 1
    for (uint32_t a = 0; a < mb; ++a) {
        uint32_t acc = 0u;
        const uint32_t e1 = bsup_off[a + 1];
#pragma unroll 8
        for (uint32_t e = bsup_off[a]; e < e1; ++e) {
            const uint32_t x = bsup[e];
            acc ^= s[(x & ~(uint32_t)(LF_Z - 1)) | ((x + t) & (LF_Z - 1))];
        }
        uint32_t* pb = stage + (a & 1u) * LF_Z;
        pb[t] = acc;
        __syncthreads();
        enc_store_block(pb, par_g + a * LF_Z, M, t, wide_out);
    }
}

extern "C" size_t lf_encode_lds_bytes(int n_check) { return ((size_t)n_check + 2u * LF_Z) * sizeof(uint32_t); }

extern "C" hipError_t lf_launch_encode(const LfDevCode* d_code, int n_check, const uint32_t* d_bsup, const uint32_t* d_bsup_off,
                                       const int8_t* d_in, const unsigned long long* d_keys, size_t n_groups, int8_t* d_out,
                                       int8_t* d_info, hipStream_t stream)
{
    const size_t lds = lf_encode_lds_bytes(n_check);
    if (d_keys) hipLaunchKernelGGL(lnsfaid_encode_kernel<true>, dim3((unsigned)n_groups), dim3(ENC_T), lds, stream, d_code, d_bsup, d_bsup_off, nullptr, d_keys, d_out, d_info);
    else hipLaunchKernelGGL(lnsfaid_encode_kernel<false>, dim3((unsigned)n_groups), dim3(ENC_T), lds, stream, d_code, d_bsup, d_bsup_off, d_in, nullptr, d_out, nullptr);
    return hipGetLastError();
}
