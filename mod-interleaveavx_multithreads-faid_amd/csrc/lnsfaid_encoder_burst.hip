/*
 * lnsfaid_encoder_burst.hip — burst-format line encode (include/lnsfaid.h "burst-format line calls"): the kernel of
 * lnsfaid_encoder_line.hip on payloads and lines whose codewords are individually shortened.
 *
 * Codeword cw has a descriptor {line_off, pay_off, s_words} (lnsfaid_burst.h).  With Sw = s_words, kw = K / 32 and k0w = 0
 * (LNSFAID_SHORTEN_HEAD) or kw - Sw (LNSFAID_SHORTEN_TAIL), the information words [k0w, k0w + Sw) of the mother codeword are known
 * zeros: they enter s = A u as zero, are not in the payload and are not stored to line; information word m behind them is word
 * m - Sw of both, and the parity words follow at kw - Sw.  bits is the mother codeword at its fixed stride, zeros included.
 *
 * Everything else is lnsfaid_encode_line_kernel (see there for the phases and the LDS plan; lnsfaid_encoder_line.h has the sizes and helpers): 32 codewords per workgroup, lane
 * (l = t / 8, q = t % 8) moves the four mother words 32 r + 4 q of codeword l per round.  A kept payload length is no longer a multiple
 * of four words, so "four words inside or outside together" holds only for a quad that lies wholly in front of or wholly behind the
 * known range: such a quad moves as one 16-byte access (4-byte aligned), a quad that touches the range word by word.  With Sw = 0
 * every quad is whole.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "lnsfaid_burst.h"
#include "lnsfaid_encoder_line.h"
#include "lnsfaid_launch.h"

/* ---- the known range of a lane's codeword: mother words [k0w, k1w), sw = k1w - k0w ---- */
struct EnbRange {
    uint32_t sw, k0w, k1w;
};

/* the mother information words w0 .. w0 + 3 (w0 + 3 < kw) from the codeword's payload: zeros inside the known range.  Reads payload
 * words < k0w as they are and words >= k1w at m - sw < kw - sw: nothing outside the codeword's own kw - sw words. */
__device__ __forceinline__ enl_u32x4 enb_load_quad(const uint32_t* pay, uint32_t w0, const EnbRange& r)
{
    if (w0 + 4u <= r.k0w) return *(const enl_u32x4*)(pay + w0);
    if (w0 >= r.k1w) return *(const enl_u32x4*)(pay + (w0 - r.sw));
    uint32_t v[4];
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) {
        const uint32_t m = w0 + j;
        v[j] = 0u;
        if (m < r.k0w) v[j] = pay[m];
        else if (m >= r.k1w) v[j] = pay[m - r.sw];
    }
    return enl_u32x4{ v[0], v[1], v[2], v[3] };
}

/* the same words to the codeword's line: the known ones are not stored, the ones behind them move up by sw */
__device__ __forceinline__ void enb_store_quad(uint32_t* ln, uint32_t w0, const EnbRange& r, enl_u32x4 v)
{
    if (w0 + 4u <= r.k0w) { *(enl_u32x4*)(ln + w0) = v; return; }
    if (w0 >= r.k1w) { *(enl_u32x4*)(ln + (w0 - r.sw)) = v; return; }
    const uint32_t x[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) {
        const uint32_t m = w0 + j;
        if (m < r.k0w) ln[m] = x[j];
        else if (m >= r.k1w) ln[m - r.sw] = x[j];
    }
}

/* payload: the burst payload; line: the burst line (LNSFAID_LINE_HARD words); bits: null or [n_cw][N / 32] (uniform over the
 * launch); desc: [n_cw].  bsup / bsup_off: support of B^-1's first rows, entries b z + c, rows [off[a], off[a + 1]). */
__global__ __launch_bounds__(ENL_T) void lnsfaid_encode_burst_kernel(const LfDevCode* __restrict__ code, const uint32_t* __restrict__ bsup,
                                                                   const uint32_t* __restrict__ bsup_off,
                                                                   const uint32_t* __restrict__ payload,
                                                                   const LfBurstDesc* __restrict__ desc, uint32_t where, uint32_t n_cw,
                                                                   uint32_t* __restrict__ line, uint32_t* __restrict__ bits)
{
    extern __shared__ uint32_t enl_lds[];
    const uint32_t t = threadIdx.x, g = blockIdx.x;
    const uint32_t N = (uint32_t)code->n_var, M = (uint32_t)code->n_check, K = N - M, L = N - (uint32_t)code->puncture_tail;
    const uint32_t kw = K / 32u, nw = N / 32u, kb = K / LF_Z;
    uint32_t* s = enl_lds;
    uint32_t* raw = s + M;
    uint32_t* u = raw + ENL_RAW_WORDS;
    uint32_t* pst = u + ENL_U_WORDS;        /* two images */
    uint32_t* ctab = pst + 2 * ENL_PST_WORDS; /* two tables */
    /* codewords present in this workgroup: 1 .. 32 (the grid is ceil(n_cw / 32)) */
    const uint32_t nc = n_cw - 32u * g < 32u ? n_cw - 32u * g : 32u;
    /* this lane's codeword on the way in and on the way out, and its eighth of a round / of a block row */
    const uint32_t l = t >> 3, q = t & 7u;
    const bool present = l < nc;
    const size_t cw = (size_t)32u * g + l; /* only used under `present` */
    LfBurstDesc d = { 0u, 0u, 0u, 0u };
    if (present) d = desc[cw];
    EnbRange kr;
    kr.sw = d.s_words;
    kr.k0w = where == LNSFAID_SHORTEN_HEAD ? 0u : kw - d.s_words;
    kr.k1w = kr.k0w + d.s_words;
    const uint32_t* pay_l = payload + (size_t)d.pay_off;
    uint32_t* line_l = line + (size_t)d.line_off;
    uint32_t* bits_l = bits ? bits + cw * nw : nullptr;
    /* the transposes: half-wave hw = t / 32 (0 .. 7), lane within it */
    const uint32_t hw = t >> 5, hl = t & 31u;

    const uint32_t mb = M / LF_Z;
    for (uint32_t a = 0; a < mb; ++a) s[a * LF_Z + t] = 0u; /* thread t alone touches s[. z + t] until phase 2 */

    /* 1. s = A u, information words out.  Fetched a round ahead: this lane's four mother words, and by the first 68 threads the
     * circulants (16 slots each) and the weights of the round's four block columns, which go through LDS to every thread. */
    const uint32_t rounds = (kw + 31u) / 32u;
    enl_u32x4 next = { 0u, 0u, 0u, 0u };
    if (present && 4u * q < kw) next = enb_load_quad(pay_l, 4u * q, kr);
    const uint32_t* ct_src = t < 64u ? &code->colcirc[0][0] + t : (const uint32_t*)&code->col_weight[0] + (t - 64u);
    const uint32_t ct_step = t < 64u ? 64u : 4u, ct_col = t < 64u ? t >> 4 : t - 64u;
    uint32_t ct_next = 0u;
    if (t < 68u && ct_col < kb) ct_next = *ct_src;
#pragma unroll 1
    for (uint32_t r = 0; r < rounds; ++r) {
        const enl_u32x4 v = next;
        const uint32_t w0 = 32u * r + 4u * q; /* this lane's first mother word of the round */
        uint32_t* rw = raw + l * ENL_RAW_STRIDE + 4u * q;
        rw[0] = v.x; rw[1] = v.y; rw[2] = v.z; rw[3] = v.w;
        uint32_t* ct = ctab + (r & 1u) * ENL_CT_WORDS;
        if (t < 68u) ct[t] = ct_next;
        /* kw is a multiple of 8: a lane's four mother words are information words or not together */
        if (present && w0 < kw) {
            enb_store_quad(line_l, w0, kr, v);
            if (bits) *(enl_u32x4*)(bits_l + w0) = v;
        }
        next = enl_u32x4{ 0u, 0u, 0u, 0u };
        ct_next = 0u;
        if (present && w0 + 32u < kw) next = enb_load_quad(pay_l, w0 + 32u, kr);
        if (t < 68u && 4u * (r + 1u) + ct_col < kb) ct_next = ct_src[(r + 1u) * ct_step];
        enl_lds_barrier(); /* raw and ct complete; u is free (every thread has finished the previous round's circulants) */
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t j = 8u * k + hw;
            u[32u * j + hl] = enl_transpose32(raw[hl * ENL_RAW_STRIDE + j], hl);
        }
        enl_lds_barrier(); /* u complete; raw is free.  ct of this parity is written again two rounds on, behind two barriers */
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c) {
            const uint32_t* ub = u + c * LF_Z;
            const uint32_t wgt = (uint32_t)__builtin_amdgcn_readfirstlane((int)ct[64u + c]); /* 0 past the last block column */
            for (uint32_t k = 0; k < wgt; ++k) {
                const uint32_t cc = ct[16u * c + k], br = cc & 0xffu, sh = cc >> 8;
                s[br * LF_Z + t] ^= ub[(sh + t) & (LF_Z - 1)];
            }
        }
    }
    __syncthreads(); /* s complete */

    /* 2. p = B^-1 s for the rows that leave: the transmitted ones, or all of them with bits */
    const uint32_t n_par = bits ? M : L - K;
    const uint32_t t4 = 4u * t;
    const uint32_t lpar = kw - kr.sw; /* first parity word of the codeword's line */
#pragma unroll 1
    for (uint32_t a = 0; a * LF_Z < n_par; ++a) {
        const uint32_t rows = n_par - a * LF_Z < LF_Z ? n_par - a * LF_Z : LF_Z; /* a multiple of 32 */
        uint32_t acc = 0u;
        if ((t & ~63u) < rows) { /* wave-uniform: a wave with no row of the block row skips it */
            const uint32_t e1 = bsup_off[a + 1];
            uint32_t e = bsup_off[a];
            uint32_t cur = e + (t & 63u) < e1 ? bsup[e + (t & 63u)] << 2 : 0u;
            while (e + 64u <= e1) {
                const uint32_t en = e + 64u + (t & 63u);
                const uint32_t nxt = en < e1 ? bsup[en] << 2 : 0u;
#pragma unroll
                for (int i = 0; i < 64; ++i) acc ^= enl_s_word(s, (uint32_t)__builtin_amdgcn_readlane((int)cur, i), t4);
                cur = nxt;
                e += 64u;
            }
#pragma unroll 1
            for (uint32_t i = 0; i < e1 - e; ++i) acc ^= enl_s_word(s, (uint32_t)__builtin_amdgcn_readlane((int)cur, (int)i), t4);
        }
        if (t >= rows) acc = 0u; /* rows is a multiple of 32: whole half-waves */
        uint32_t* pb = pst + (a & 1u) * ENL_PST_WORDS;
        pb[hl * ENL_PST_STRIDE + hw] = enl_transpose32(acc, hl);
        __syncthreads(); /* the image of two block rows ago was read before the previous barrier */
        const uint32_t pw = 8u * a + q; /* parity word of codeword l */
        if (present && 32u * q < rows) {
            const uint32_t x = pb[l * ENL_PST_STRIDE + q];
            if (32u * pw < L - K) line_l[lpar + pw] = x;
            if (bits) bits_l[kw + pw] = x;
        }
    }
}

extern "C" size_t lf_encode_burst_lds_bytes(int n_check)
{
    return ((size_t)n_check + ENL_RAW_WORDS + ENL_U_WORDS + 2u * ENL_PST_WORDS + 2u * ENL_CT_WORDS) * sizeof(uint32_t);
}

extern "C" hipError_t lf_launch_encode_burst(const LfDevCode* d_code, int n_check, const uint32_t* d_bsup, const uint32_t* d_bsup_off,
                                             const uint32_t* d_payload, const LfBurstDesc* d_desc, int where, size_t n_codewords,
                                             uint32_t* d_line, uint32_t* d_bits, hipStream_t stream)
{
    const size_t groups = (n_codewords + LNSFAID_GROUP - 1) / LNSFAID_GROUP;
    hipLaunchKernelGGL(lnsfaid_encode_burst_kernel, dim3((unsigned)groups), dim3(ENL_T), lf_encode_burst_lds_bytes(n_check), stream, d_code,
                       d_bsup, d_bsup_off, d_payload, d_desc, (uint32_t)where, (uint32_t)n_codewords, d_line, d_bits);
    return hipGetLastError();
}
