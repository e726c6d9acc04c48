/*
 * lnsfaid_fecstatus.hip — FEC status without the sent bits (include/lnsfaid.h "FEC status"): per codeword the
 * parity checks its hard decisions leave unsatisfied and the bits in which they differ from the channel's own decisions; per call
 * the PON FEC performance counters and, when the sent frames are at hand, the split of the error frames into detected and
 * undetected ones.  A pure read of decisions that may come from anywhere; no decode kernel is involved.
 *
 * One wavefront per codeword, FS_WAVES codewords per workgroup pass, a workgroup walks the batch with the grid's stride:
 *   pass 1  streams the codeword's decisions (and its two fixInput segments, and the information part of its sent frame) with
 *           FS_UNITS loads in flight per stream before the first use, writes the codeword's bit plane into the wave's own LDS
 *           (bit b of word w = code bit 32 w + b: the layout of the decode kernels' hard plane and of the packed output) and counts
 *           `corrected` and the wrong information bytes on the way.
 *   pass 2  the syndrome from the plane: word k (rows 32 k .. 32 k + 31) of layer br is the XOR over the layer's circulants of the
 *           32 bits that start at bit (32 k + shift) mod 256 of the circulant's block column - two LDS reads and a funnel shift
 *           each.  nbr * 8 such words over the 64 lanes, a popcount, a wave reduction.
 * The layer table (block column * 256 + shift of every circulant) is staged in LDS once per workgroup.  The counters leave with
 * one set of atomics per workgroup.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "lnsfaid_device.h"
#include "lnsfaid_launch.h"

#define FS_WAVES 4   /* codewords in flight per workgroup */
#define FS_UNITS 4   /* loads a lane has in flight per stream before the first use */
#define FS_MAX_WG 2048u

/* the plane of a wave is written and read by that wave alone: an LDS fence, no s_barrier */
__device__ __forceinline__ void fs_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

/* bit 7 of every byte of x that is not zero */
__device__ __forceinline__ uint32_t fs_nonzero(uint32_t x) { return (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u; }
/* bit 7 of every byte of x that is > 0 as int8 */
__device__ __forceinline__ uint32_t fs_positive(uint32_t x) { return fs_nonzero(x) & ~x; }
/* bits 7, 15, 23, 31 -> bits 0 .. 3 */
__device__ __forceinline__ uint32_t fs_gather4(uint32_t hi) { return (((hi >> 7) * 0x01020408u) >> 24) & 0xfu; }
/* bits 0 .. 3 -> 0 / 1 in bytes 0 .. 3 */
__device__ __forceinline__ uint32_t fs_spread4(uint32_t nib) { return (nib * 0x00204081u) & 0x01010101u; }
/* the > 0 of eight two's-complement nibbles as eight bits, nibble i -> bit i */
__device__ __forceinline__ uint32_t fs_positive_nibbles(uint32_t x)
{
    uint32_t t = ((((x & 0x77777777u) + 0x77777777u) | x) & ~x & 0x88888888u) >> 3;
    t = (t | (t >> 3)) & 0x03030303u;
    t = (t | (t >> 6)) & 0x000f000fu;
    return (t | (t >> 12)) & 0xffu;
}
/* bit 7 of the first min(max(n, 0), 4) bytes */
__device__ __forceinline__ uint32_t fs_first_bytes(int n) { return n >= 4 ? 0x80808080u : n <= 0 ? 0u : (0x80808080u >> (8 * (4 - n))); }
/* the first min(max(n, 0), 32) bits */
__device__ __forceinline__ uint32_t fs_first_bits(int n) { return n >= 32 ? 0xffffffffu : n <= 0 ? 0u : ((1u << n) - 1u); }

template <bool WIDE> __device__ __forceinline__ uint32_t fs_load32(const uint8_t* p)
{
    if (WIDE) return *(const uint32_t*)p;
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}
template <bool WIDE> __device__ __forceinline__ uint4 fs_load128(const uint8_t* p)
{
    if (WIDE) return *(const uint4*)p;
    return make_uint4(fs_load32<false>(p), fs_load32<false>(p + 4), fs_load32<false>(p + 8), fs_load32<false>(p + 12));
}

struct FsCount {
    uint32_t corrected;  /* this lane's share */
    uint32_t info_wrong; /* != 0: this lane saw a wrong information byte */
};

/* pass 1, int8 decisions, 16-byte loads: lane j of a batch owns code bits 16 j .. 16 j + 15, half a plane word */
__device__ __forceinline__ FsCount fs_pass1_wide(const int8_t* __restrict__ d, const int8_t* __restrict__ fi, const int8_t* __restrict__ fp,
                                                 const int8_t* __restrict__ si, bool want_sent, uint32_t N, uint32_t K, int limit,
                                                 uint32_t* plane, uint32_t lane)
{
    FsCount c = { 0u, 0u };
    const uint32_t n_units = N / 16u;
    for (uint32_t j0 = 0; j0 < n_units; j0 += 64u * FS_UNITS) {
        uint4 dv[FS_UNITS], xv[FS_UNITS], sv[FS_UNITS];
#pragma unroll
        for (uint32_t u = 0; u < FS_UNITS; ++u) {
            const uint32_t j = j0 + u * 64u + lane, k = 16u * j;
            dv[u] = xv[u] = sv[u] = make_uint4(0u, 0u, 0u, 0u);
            if (j < n_units) {
                dv[u] = *(const uint4*)(d + k);
                if (fi) xv[u] = k < K ? *(const uint4*)(fi + k) : *(const uint4*)(fp + (k - K));
                if (si && k < K) sv[u] = *(const uint4*)(si + k);
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < FS_UNITS; ++u) {
            const uint32_t j = j0 + u * 64u + lane, k = 16u * j;
            if (j >= n_units) continue;
            const uint32_t dw[4] = { dv[u].x, dv[u].y, dv[u].z, dv[u].w }, xw[4] = { xv[u].x, xv[u].y, xv[u].z, xv[u].w };
            uint32_t half = 0;
#pragma unroll
            for (uint32_t q = 0; q < 4u; ++q) {
                const uint32_t nz = fs_nonzero(dw[q]);
                half |= fs_gather4(nz) << (4u * q);
                if (fi) c.corrected += (uint32_t)__popc((fs_positive(xw[q]) ^ nz) & fs_first_bytes(limit - (int)(k + 4u * q)));
            }
            ((uint16_t*)plane)[j] = (uint16_t)half;
            if (want_sent && k < K) c.info_wrong |= (dv[u].x ^ sv[u].x) | (dv[u].y ^ sv[u].y) | (dv[u].z ^ sv[u].z) | (dv[u].w ^ sv[u].w);
        }
    }
    return c;
}

/* pass 1, int8 decisions, byte loads for pointers of any alignment: a ballot makes two plane words of 64 lanes' bytes */
__device__ __forceinline__ FsCount fs_pass1_narrow(const int8_t* __restrict__ d, const int8_t* __restrict__ fi, const int8_t* __restrict__ fp,
                                                   const int8_t* __restrict__ si, bool want_sent, uint32_t N, uint32_t K, int limit,
                                                   uint32_t* plane, uint32_t lane)
{
    FsCount c = { 0u, 0u };
    for (uint32_t k0 = 0; k0 < N; k0 += 64u * 2u * FS_UNITS) { /* N is a multiple of 64 */
        int8_t dv[2 * FS_UNITS], xv[2 * FS_UNITS], sv[2 * FS_UNITS];
#pragma unroll
        for (uint32_t u = 0; u < 2u * FS_UNITS; ++u) {
            const uint32_t k = k0 + u * 64u + lane;
            dv[u] = xv[u] = sv[u] = 0;
            if (k < N) {
                dv[u] = d[k];
                if (fi) xv[u] = k < K ? fi[k] : fp[k - K];
                if (si && k < K) sv[u] = si[k];
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < 2u * FS_UNITS; ++u) {
            const uint32_t k = k0 + u * 64u + lane;
            const bool in = k < N, bit = in && dv[u] != 0;
            const unsigned long long m = __ballot(bit);
            if (k0 + u * 64u < N && lane == 0u) {
                plane[(k0 + u * 64u) / 32u] = (uint32_t)m;
                plane[(k0 + u * 64u) / 32u + 1u] = (uint32_t)(m >> 32);
            }
            if (fi && in && (int)k < limit) c.corrected += (xv[u] > 0) != bit ? 1u : 0u;
            if (want_sent && k < K) c.info_wrong |= dv[u] != sv[u] ? 1u : 0u;
        }
    }
    return c;
}

/* pass 1, packed decisions: lane w of a batch owns plane word w = 32 code bits = 16 bytes of llr4 = 32 sent bytes */
template <bool WIDE>
__device__ __forceinline__ FsCount fs_pass1_packed(const uint8_t* __restrict__ b, const uint8_t* __restrict__ li, const uint8_t* __restrict__ lp,
                                                   const uint8_t* __restrict__ si, bool want_sent, uint32_t N, uint32_t K, int limit,
                                                   uint32_t* plane, uint32_t lane)
{
    FsCount c = { 0u, 0u };
    const uint32_t n_words = N / 32u;
    for (uint32_t w0 = 0; w0 < n_words; w0 += 64u * FS_UNITS) {
        uint32_t bw[FS_UNITS];
        uint4 xv[FS_UNITS], s0[FS_UNITS], s1[FS_UNITS];
#pragma unroll
        for (uint32_t u = 0; u < FS_UNITS; ++u) {
            const uint32_t w = w0 + u * 64u + lane, k = 32u * w;
            bw[u] = 0u;
            xv[u] = s0[u] = s1[u] = make_uint4(0u, 0u, 0u, 0u);
            if (w < n_words) {
                bw[u] = fs_load32<WIDE>(b + 4u * w);
                if (li) xv[u] = k < K ? fs_load128<WIDE>(li + k / 2u) : fs_load128<WIDE>(lp + (k - K) / 2u);
                if (si && k < K) { s0[u] = fs_load128<WIDE>(si + k); s1[u] = fs_load128<WIDE>(si + k + 16u); }
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < FS_UNITS; ++u) {
            const uint32_t w = w0 + u * 64u + lane, k = 32u * w;
            if (w >= n_words) continue;
            plane[w] = bw[u];
            if (li) {
                const uint32_t ch = fs_positive_nibbles(xv[u].x) | fs_positive_nibbles(xv[u].y) << 8 | fs_positive_nibbles(xv[u].z) << 16 |
                                    fs_positive_nibbles(xv[u].w) << 24;
                c.corrected += (uint32_t)__popc((ch ^ bw[u]) & fs_first_bits(limit - (int)k));
            }
            if (want_sent && k < K) {
                const uint32_t sw[8] = { s0[u].x, s0[u].y, s0[u].z, s0[u].w, s1[u].x, s1[u].y, s1[u].z, s1[u].w };
#pragma unroll
                for (uint32_t q = 0; q < 8u; ++q) c.info_wrong |= fs_spread4((bw[u] >> (4u * q)) & 0xfu) ^ sw[q];
            }
        }
    }
    return c;
}

/* pass 2: this lane's share of the checks the plane leaves unsatisfied */
__device__ __forceinline__ uint32_t fs_syndrome(const uint32_t* plane, const uint32_t* sSb, const uint32_t* sDeg, uint32_t nbr, uint32_t lane)
{
    uint32_t unsat = 0;
    for (uint32_t t = lane; t < nbr * 8u; t += 64u) {
        const uint32_t br = t >> 3, k = t & 7u, deg = sDeg[br];
        uint32_t acc = 0;
        for (uint32_t j = 0; j < deg; ++j) {
            const uint32_t sb = sSb[br * LF_MAX_DEG + j], o = (32u * k + sb) & 255u, q = o >> 5;
            const uint32_t* col = plane + (sb >> 8) * 8u;
            acc ^= __funnelshift_r(col[q], col[(q + 1u) & 7u], o & 31u);
        }
        unsat += (uint32_t)__popc(acc);
    }
    return unsat;
}

struct FsArgs {
    const LfDevCode* code;
    const void* fix;      /* int8 fixInput / llr4, or null */
    const void* decided;  /* int8 decodedBits / packed bits */
    const int8_t* sent;   /* or null */
    lnsfaid_fec_record* records; /* or null */
    unsigned long long* acc;     /* out[4] then vs_sent[4], ADDED to */
    uint32_t n_cw;
    int want_sent;        /* vs_sent is asked for (sent == null: the all-zero codeword) */
};

/* MODE 0: int8, 16-byte loads; 1: int8, byte loads; 2: packed, aligned; 3: packed, byte loads */
template <int MODE> __global__ __launch_bounds__(64 * FS_WAVES) void lnsfaid_fec_status_kernel(FsArgs a)
{
    extern __shared__ uint32_t sPlanes[]; /* FS_WAVES planes of n_words words */
    __shared__ uint32_t sSb[LF_MAX_BR * LF_MAX_DEG], sDeg[LF_MAX_BR];
    __shared__ unsigned int sAcc[6];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const LfDevCode* __restrict__ code = a.code;
    const uint32_t N = (uint32_t)code->n_var, M = (uint32_t)code->n_check, K = N - M, nbr = (uint32_t)code->nbr;
    const int limit = code->n_var - code->puncture_tail;
    for (uint32_t i = tid; i < nbr * LF_MAX_DEG; i += 64u * FS_WAVES) sSb[i] = code->circ[i / LF_MAX_DEG][i % LF_MAX_DEG].sb;
    if (tid < nbr) sDeg[tid] = (uint32_t)code->deg[tid];
    if (tid < 6u) sAcc[tid] = 0u;
    __syncthreads();
    uint32_t* plane = sPlanes + wave * (N / 32u);
    const bool want_sent = a.want_sent != 0;
    /* lane 0's tallies: uncorrectable, corrected codewords, corrected bits, error frames, undetected, false alarms */
    uint32_t n_unc = 0, n_cor = 0, n_bits = 0, n_err = 0, n_und = 0, n_fa = 0;
    for (uint32_t cw = blockIdx.x * FS_WAVES + wave; cw < a.n_cw; cw += gridDim.x * FS_WAVES) {
        const size_t g = cw / LNSFAID_GROUP, m = cw % LNSFAID_GROUP;
        FsCount c;
        if (MODE < 2) {
            const int8_t* fg = a.fix ? (const int8_t*)a.fix + g * (size_t)(32u * N) : nullptr;
            const int8_t* sg = a.sent ? a.sent + g * (size_t)(32u * N) + m * K : nullptr;
            const int8_t* d = (const int8_t*)a.decided + (size_t)cw * N;
            if (MODE == 0) c = fs_pass1_wide(d, fg ? fg + m * K : nullptr, fg ? fg + (size_t)32u * K + m * M : nullptr, sg, want_sent, N, K, limit, plane, lane);
            else c = fs_pass1_narrow(d, fg ? fg + m * K : nullptr, fg ? fg + (size_t)32u * K + m * M : nullptr, sg, want_sent, N, K, limit, plane, lane);
        } else {
            const uint8_t* lg = a.fix ? (const uint8_t*)a.fix + g * (size_t)(16u * N) : nullptr;
            const uint8_t* sg = a.sent ? (const uint8_t*)a.sent + g * (size_t)(32u * N) + m * K : nullptr;
            const uint8_t* b = (const uint8_t*)a.decided + (size_t)cw * (N / 8u);
            c = fs_pass1_packed<MODE == 2>(b, lg ? lg + m * (K / 2u) : nullptr, lg ? lg + (size_t)16u * K + m * (M / 2u) : nullptr, sg, want_sent, N, K,
                                           limit, plane, lane);
        }
        fs_wave_sync();
        uint32_t unsat = fs_syndrome(plane, sSb, sDeg, nbr, lane), corr = c.corrected;
        fs_wave_sync(); /* the next codeword rewrites the plane */
        for (int o = 32; o > 0; o >>= 1) { unsat += __shfl_down(unsat, o); corr += __shfl_down(corr, o); }
        const bool wrong = __ballot(c.info_wrong != 0u) != 0ull;
        if (lane == 0u) {
            if (a.records) { a.records[cw].unsatisfied = unsat; a.records[cw].corrected = corr; }
            if (unsat > 0u) n_unc += 1u;
            else if (corr > 0u) { n_cor += 1u; n_bits += corr; }
            if (want_sent) {
                if (wrong) { n_err += 1u; n_und += unsat == 0u ? 1u : 0u; }
                else n_fa += unsat > 0u ? 1u : 0u;
            }
        }
    }
    if (lane == 0u) {
        atomicAdd(&sAcc[0], n_unc); atomicAdd(&sAcc[1], n_cor); atomicAdd(&sAcc[2], n_bits);
        atomicAdd(&sAcc[3], n_err); atomicAdd(&sAcc[4], n_und); atomicAdd(&sAcc[5], n_fa);
    }
    __syncthreads();
    if (tid == 0u) {
        uint32_t total = 0; /* the codewords this workgroup walked */
        for (uint32_t cw = blockIdx.x * FS_WAVES; cw < a.n_cw; cw += gridDim.x * FS_WAVES) total += a.n_cw - cw < FS_WAVES ? a.n_cw - cw : FS_WAVES;
        atomicAdd(&a.acc[0], (unsigned long long)total);
        if (sAcc[0]) atomicAdd(&a.acc[1], (unsigned long long)sAcc[0]);
        if (sAcc[1]) atomicAdd(&a.acc[2], (unsigned long long)sAcc[1]);
        if (sAcc[2]) atomicAdd(&a.acc[3], (unsigned long long)sAcc[2]);
        if (want_sent) {
            atomicAdd(&a.acc[4], (unsigned long long)total);
            if (sAcc[3]) atomicAdd(&a.acc[5], (unsigned long long)sAcc[3]);
            if (sAcc[4]) atomicAdd(&a.acc[6], (unsigned long long)sAcc[4]);
            if (sAcc[5]) atomicAdd(&a.acc[7], (unsigned long long)sAcc[5]);
        }
    }
}

/* The caller (lnsfaid_capi.hip) has checked the rules of include/lnsfaid.h; n_var / 32 words per plane must fit the workgroup's LDS
 * (n_var <= LF_MAX_BC * 256: 32 KiB for the four planes).  d_acc: out[4] then vs_sent[4], ADDED to. */
extern "C" hipError_t lf_launch_fec_status(const LfDevCode* d_code, int n_var, int packed, const void* d_fix, const void* d_decided,
                                           const int8_t* d_sent, size_t n_groups, lnsfaid_fec_record* d_records, int want_sent,
                                           unsigned long long* d_acc, hipStream_t stream)
{
    FsArgs a;
    a.code = d_code; a.fix = d_fix; a.decided = d_decided; a.sent = d_sent; a.records = d_records; a.acc = d_acc;
    a.n_cw = (uint32_t)(n_groups * LNSFAID_GROUP);
    a.want_sent = want_sent;
    const uint32_t wgs = (a.n_cw + FS_WAVES - 1u) / FS_WAVES;
    const dim3 grid(wgs < FS_MAX_WG ? wgs : FS_MAX_WG), block(64 * FS_WAVES);
    const size_t lds = (size_t)FS_WAVES * (size_t)(n_var / 32) * sizeof(uint32_t);
    /* every frame part starts a multiple of 128 bytes after its base pointer (n_var, K and M are multiples of 256) */
    const uintptr_t align = (uintptr_t)d_fix | (uintptr_t)d_sent | (uintptr_t)d_decided;
    if (!packed) {
        if ((align & 15u) == 0u) hipLaunchKernelGGL(lnsfaid_fec_status_kernel<0>, grid, block, lds, stream, a);
        else hipLaunchKernelGGL(lnsfaid_fec_status_kernel<1>, grid, block, lds, stream, a);
    } else {
        if ((((uintptr_t)d_fix | (uintptr_t)d_sent) & 15u) == 0u && ((uintptr_t)d_decided & 3u) == 0u)
            hipLaunchKernelGGL(lnsfaid_fec_status_kernel<2>, grid, block, lds, stream, a);
        else hipLaunchKernelGGL(lnsfaid_fec_status_kernel<3>, grid, block, lds, stream, a);
    }
    return hipGetLastError();
}
