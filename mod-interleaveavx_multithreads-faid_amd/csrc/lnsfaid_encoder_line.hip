/*
 * lnsfaid_encoder_line.hip — line-format encode (include/lnsfaid.h "line-format encode"): payload words in,
 * transmitted codewords out, nothing one byte per bit.
 *
 * The arithmetic is that of lnsfaid_encoder.hip: H = [A | B], p = B^-1 A u, bit-sliced over 32 codewords (one
 * 32-bit word per code bit, bit l = codeword l), thread t owns row t of every circulant.  One workgroup of 256 threads takes the
 * 32 consecutive codewords 32 g .. 32 g + 31 of the line; the last one may hold fewer: an absent codeword is neither loaded nor
 * stored and contributes zero words.
 *   way in   per round, lane (l = t / 8, q = t % 8) loads the 16 bytes at word 32 r + 4 q of codeword l's payload (eight lanes cover
 *            128 contiguous bytes = four block columns of one codeword), one round ahead of its use.  The same registers go out
 *            again as the information words of line (and bits), and into the raw image [32 codewords][32 words] in LDS.  Wave w,
 *            half-wave h then reads the columns j = 8 k + 2 w + h of the image (lane = codeword), transposes each 32 x 32 bit
 *            matrix by five exchange steps (lane ^ 16, 8, 4, 2, 1) and writes the bit-sliced words u[32 j + lane].
 *   s = A u  s[br z + t] ^= u[cb z + (sh + t) mod z] per circulant of the round's block columns.
 *   p        per block row a: p[a z + t] from the support list of B^-1 (64 entries per vector load, handed out by v_readlane)
 *            against s in LDS.  The 32
 *            lanes of a half-wave hold positions 32 w .. 32 w + 31 of the block row: the same five steps give lane l parity word
 *            8 a + w of codeword l.  Through a [32][8] image in LDS eight lanes store the 32 contiguous bytes of one codeword.
 *            Only rows below n_par are computed: L - K without bits (the punctured tail is never formed), M with bits.
 * LDS: s (M words) + raw image (32 x 33) + u (1024) + two parity images (2 x 32 x 9) + two circulant tables (2 x 68): 23 KiB for
 * the 50G-PON code.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "lnsfaid_encoder_line.h"
#include "lnsfaid_launch.h"

/* payload: [n_cw][K / 32]; line: [n_cw][L / 32]; bits: null or [n_cw][N / 32] (uniform over the launch).
 * bsup / bsup_off: support of B^-1's first rows, entries b z + c, rows [off[a], off[a + 1]). */
__global__ __launch_bounds__(ENL_T) void lnsfaid_encode_line_kernel(const LfDevCode* __restrict__ code, const uint32_t* __restrict__ bsup,
                                                                  const uint32_t* __restrict__ bsup_off,
                                                                  const uint32_t* __restrict__ payload, uint32_t n_cw,
                                                                  uint32_t* __restrict__ line, uint32_t* __restrict__ bits)
{
    extern __shared__ uint32_t enl_lds[];
    const uint32_t t = threadIdx.x, g = blockIdx.x;
    const uint32_t N = (uint32_t)code->n_var, M = (uint32_t)code->n_check, K = N - M, L = N - (uint32_t)code->puncture_tail;
    const uint32_t kw = K / 32u, lw = L / 32u, nw = N / 32u, kb = K / LF_Z;
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
    const uint32_t* pay_l = payload + cw * kw;
    uint32_t* line_l = line + cw * lw;
    uint32_t* bits_l = bits ? bits + cw * nw : nullptr;
    /* the transposes: half-wave hw = t / 32 (0 .. 7), lane within it */
    const uint32_t hw = t >> 5, hl = t & 31u;

    const uint32_t mb = M / LF_Z;
    for (uint32_t a = 0; a < mb; ++a) s[a * LF_Z + t] = 0u; /* thread t alone touches s[. z + t] until phase 2 */

    /* 1. s = A u, information words out.  Fetched a round ahead: this lane's four payload words, and by the first 68 threads the
     * circulants (16 slots each) and the weights of the round's four block columns, which go through LDS to every thread. */
    const uint32_t rounds = (kw + 31u) / 32u;
    enl_u32x4 next = { 0u, 0u, 0u, 0u };
    if (present && 4u * q < kw) next = *(const enl_u32x4*)(pay_l + 4u * q);
    /* the table entry this thread fetches: slot t of the round's 64 circulant slots (colcirc rows are LF_MAX_COLW words, so four
     * block columns are 64 consecutive words), or the weight of block column t - 64 of the round */
    const uint32_t* ct_src = t < 64u ? &code->colcirc[0][0] + t : (const uint32_t*)&code->col_weight[0] + (t - 64u);
    const uint32_t ct_step = t < 64u ? 64u : 4u, ct_col = t < 64u ? t >> 4 : t - 64u;
    uint32_t ct_next = 0u;
    if (t < 68u && ct_col < kb) ct_next = *ct_src;
#pragma unroll 1
    for (uint32_t r = 0; r < rounds; ++r) {
        const enl_u32x4 v = next;
        const uint32_t w0 = 32u * r + 4u * q; /* this lane's first word of the round */
        uint32_t* rw = raw + l * ENL_RAW_STRIDE + 4u * q;
        rw[0] = v.x; rw[1] = v.y; rw[2] = v.z; rw[3] = v.w;
        uint32_t* ct = ctab + (r & 1u) * ENL_CT_WORDS;
        if (t < 68u) ct[t] = ct_next;
        /* kw is a multiple of 8: a lane's four words are inside the payload or outside together */
        if (present && w0 < kw) {
            *(enl_u32x4*)(line_l + w0) = v;
            if (bits) *(enl_u32x4*)(bits_l + w0) = v;
        }
        next = enl_u32x4{ 0u, 0u, 0u, 0u };
        ct_next = 0u;
        if (present && w0 + 32u < kw) next = *(const enl_u32x4*)(pay_l + w0 + 32u);
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
#pragma unroll 1
    for (uint32_t a = 0; a * LF_Z < n_par; ++a) {
        const uint32_t rows = n_par - a * LF_Z < LF_Z ? n_par - a * LF_Z : LF_Z; /* a multiple of 32 */
        uint32_t acc = 0u;
        if ((t & ~63u) < rows) { /* wave-uniform: a wave with no row of the block row skips it */
            /* The list is wave-uniform, but scalar loads share their counter with the LDS reads, so a wait for the one drains the
             * other.  Instead every lane fetches one entry of the next 64, as the byte offset of its s word for t = 0, one chunk
             * ahead; v_readlane hands them out.  64 independent LDS reads per chunk. */
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
        /* half-wave hw holds positions 32 hw .. + 31 of the block row, one per lane -> lane = codeword, parity word 8 a + hw */
        uint32_t* pb = pst + (a & 1u) * ENL_PST_WORDS;
        pb[hl * ENL_PST_STRIDE + hw] = enl_transpose32(acc, hl);
        __syncthreads(); /* the image of two block rows ago was read before the previous barrier */
        const uint32_t pw = 8u * a + q; /* parity word of codeword l */
        if (present && 32u * q < rows) {
            const uint32_t x = pb[l * ENL_PST_STRIDE + q];
            if (32u * pw < L - K) line_l[kw + pw] = x;
            if (bits) bits_l[kw + pw] = x;
        }
    }
}

extern "C" size_t lf_encode_line_lds_bytes(int n_check)
{
    return ((size_t)n_check + ENL_RAW_WORDS + ENL_U_WORDS + 2u * ENL_PST_WORDS + 2u * ENL_CT_WORDS) * sizeof(uint32_t);
}

extern "C" hipError_t lf_launch_encode_line(const LfDevCode* d_code, int n_check, const uint32_t* d_bsup, const uint32_t* d_bsup_off,
                                            const uint32_t* d_payload, size_t n_codewords, uint32_t* d_line, uint32_t* d_bits,
                                            hipStream_t stream)
{
    const size_t groups = (n_codewords + LNSFAID_GROUP - 1) / LNSFAID_GROUP;
    hipLaunchKernelGGL(lnsfaid_encode_line_kernel, dim3((unsigned)groups), dim3(ENL_T), lf_encode_line_lds_bytes(n_check), stream, d_code,
                       d_bsup, d_bsup_off, d_payload, (uint32_t)n_codewords, d_line, d_bits);
    return hipGetLastError();
}
