/*
 * lnsfaid_kernel4b.hip — burst-format line decode (include/lnsfaid.h "burst-format line calls"): the line decoders of
 * lnsfaid_kernel4l.hip (lnsfaid_decode4l_kernel) on lines whose codewords are individually shortened.
 *
 * Codeword cw has a descriptor {line_off, pay_off, s_words} (lnsfaid_burst.h), the host's prefix sums.  With Sw = s_words, Kw = K / 32,
 * Lw = L / 32 and k0w = 0 (LNSFAID_SHORTEN_HEAD) or Kw - Sw (LNSFAID_SHORTEN_TAIL), the words [k0w, k0w + Sw) of the mother codeword
 * are known zeros that the line does not carry: mother word wi >= k0w + Sw is line word wi - Sw of the codeword.
 *
 * Differences from lnsfaid_decode4l_kernel:
 *   - staging walks the mother positions and classes each lane's four nodes (one class: S, k0 and L are multiples of 32) as known
 *     (staged as SW_BIAS_EN - 7 without a load), erased (>= L, as there) or transmitted (loaded from the shifted line position);
 *   - the payload is the information words without the known ones, at the codeword's own payload offset; the corrected count runs
 *     against the shifted line words and skips the known range, whose decided ones are counted on their own (short_ones);
 *   - the descriptor lives in scalar registers and is read again in the epilogue: nothing of it is carried across the decode.
 * Everything between staging and output is macro text (the per-codeword frame of lnsfaid_frame4.h, the loops of lnsfaid_rows4.h); no
 * expanded line exists anywhere.
 */
#include <hip/hip_runtime.h>

#include "lnsfaid_frame4.h"
#include "lnsfaid_burst.h"
#include "lnsfaid_launch.h"

/* the descriptor of this workgroup's codeword, uniform: through an opaque scalar copy of the address, so that the epilogue's read is
 * a read of its own and not the staging's values kept alive */
struct LbRange {
    int sw, k0w, k1w;      /* known words [k0w, k1w) of the mother codeword, sw = k1w - k0w */
    uint32_t line_off, pay_off;
};
__device__ __forceinline__ LbRange lb_range(const LfBurstArgs& a, int cw, int kw)
{
    const LfBurstDesc* dp = a.desc + cw;
    asm volatile("" : "+s"(dp));
    LbRange r;
    r.sw = __builtin_amdgcn_readfirstlane((int)dp->s_words);
    r.line_off = (uint32_t)__builtin_amdgcn_readfirstlane((int)dp->line_off);
    r.pay_off = (uint32_t)__builtin_amdgcn_readfirstlane((int)dp->pay_off);
    r.k0w = a.where == LNSFAID_SHORTEN_HEAD ? 0 : kw - r.sw;
    r.k1w = r.k0w + r.sw;
    return r;
}

/* ---- staging from a burst line.  The shape of LF4L_STAGE_ROUNDS (lnsfaid_kernel4l.hip): lane tid owns nodes 4 tid .. 4 tid + 3 of
 * every block column, the loads of a round of 23 columns are in flight together.
 *
 * Addresses.  The lane's four nodes of block column cb lie in mother word wi = 8 cb + tid / 8.
 *   known        k0w <= wi < k1w: no load.  HARD stages SW_BIAS_EN - 7; LLR4 takes the half-word 0x9999 (four nibbles -7) through
 *                the same widening as a loaded one.
 *   erased       wi >= Lw: no load, En = 0, as in every decoder of this library.
 *   transmitted  line word wl = wi - (wi >= k1w ? Sw : 0) of the codeword, 0 <= wl < Lw - Sw: inside the codeword's own
 *                (L - S) / 32 words.  HARD reads word wl and takes bits 4 (tid % 8) .. + 3; LLR4 reads the half-word at byte
 *                16 wl + 2 (tid % 8) of the codeword's (L - S) / 2 bytes, highest byte read 16 (Lw - Sw) - 1.
 * So the last codeword of a buffer is never read past the caller's allocation. ---- */
#define LF4B_STAGE_ROUNDS(KNOWN_H, LOAD, WIDEN) \
            for (int cb0 = 0; cb0 < nbc; cb0 += SB) {                                                                                     \
                uint32_t w[SB];                                                                                                           \
_Pragma("unroll")                                                                                                                         \
                for (int u = 0; u < SB; ++u) {                                                                                            \
                    const int cb = cb0 + u;                                                                                               \
                    if (cb < nbc) { /* uniform */                                                                                         \
                        const int wi = cb * (LF_Z >> 5) + (tid >> 3);                                                                     \
                        const bool known = wi >= sr.k0w && wi < sr.k1w;                                                                   \
                        const bool inside = wi < lw && !known;                                                                            \
                        const int wl = wi - (wi >= sr.k1w ? sr.sw : 0);                                                                   \
                        w[u] = known ? (KNOWN_H) : 0u;                                                                                    \
                        if (inside) w[u] = LOAD;                                                                                          \
                    }                                                                                                                     \
                }                                                                                                                         \
_Pragma("unroll")                                                                                                                         \
                for (int u = 0; u < SB; ++u) {                                                                                            \
                    const int cb = cb0 + u;                                                                                               \
                    if (cb < nbc) {                                                                                                       \
                        const int wi = cb * (LF_Z >> 5) + (tid >> 3);                                                                     \
                        const bool known = wi >= sr.k0w && wi < sr.k1w;                                                                   \
                        const bool inside = wi < lw && !known;                                                                            \
                        const uint32_t h = w[u];                                                                                          \
                        uint32_t x;                                                                                                       \
                        WIDEN                                                                                                             \
                        const uint32_t ad = (uint32_t)cb * 256u + base_d;                                                                 \
                        lds.wr8(ad, x); lds.wr8(ad + 4u, x >> 8); lds.wr8(ad + 8u, x >> 16); lds.wr8(ad + 12u, x >> 24);                  \
                    }                                                                                                                     \
                }                                                                                                                         \
            }                                                                                                                             \
    /* end of LF4B_STAGE_ROUNDS */

#define LF4B_STAGE_INPUT() \
        const int first_erased = N - c->puncture_tail; /* L */                                                                           \
        const int lw = first_erased >> 5;                                                                                                 \
        const int nbc = c->nbc;                                                                                                           \
        constexpr int SB = 23;                                                                                                            \
        const uint32_t base_d = ((16u * (uint32_t)tid) & 0xffu) + ((uint32_t)tid >> 4);                                                   \
        const SwLds lds = SwLds();                                                                                                        \
        {                                                                                                                                 \
            const LbRange sr = lb_range(a, cw, K >> 5);                                                                                   \
            if (a.format == LNSFAID_LINE_HARD) {                                                                                          \
                const uint32_t* src = (const uint32_t*)a.line + (size_t)sr.line_off;                                                      \
                const uint32_t zero4 = (uint32_t)(SW_BIAS_EN - a.magnitude) * 0x01010101u, one = 2u * (uint32_t)a.magnitude;              \
                LF4B_STAGE_ROUNDS(0u, src[wl],                                                                                            \
                    x = inside ? zero4 + ((((h >> (4 * (tid & 7))) & 15u) * 0x00204081u) & 0x01010101u) * one                             \
                               : (uint32_t)(known ? SW_BIAS_EN - 7 : SW_BIAS_EN) * 0x01010101u;)                                          \
            } else {                                                                                                                      \
                const uint8_t* src = (const uint8_t*)a.line + (size_t)sr.line_off * 16u;                                                  \
                LF4B_STAGE_ROUNDS(0x9999u, *(const uint16_t*)(src + 16 * wl + 2 * (tid & 7)),                                             \
                    x = (h & 0xfu) | ((h & 0xf0u) << 4) | ((h & 0xf00u) << 8) | ((h & 0xf000u) << 12); /* nibble k -> byte k */           \
                    x |= (x & 0x08080808u) * 0x1eu; /* sign-extend: 0x8..0xf -> 0xf8..0xff, no carries between bytes */                  \
                    (void)inside; (void)known; /* no load: h = 0, the erasure, or 0x9999, four known zeros */                             \
                    x = ((x & 0x7f7f7f7fu) + (uint32_t)SW_BIAS_EN * 0x01010101u) ^ (x & 0x80808080u);)                                    \
            }                                                                                                                             \
        }                                                                                                                                 \
    /* end of LF4B_STAGE_INPUT */

/* write_words of lnsfaid_kernel4l.hip: nw words of the plane from sHard on.  16-byte stores of four words when the output starts on
 * 16 bytes and the count is a multiple of 4; dword stores otherwise, which is the normal case inside a burst */
__device__ __forceinline__ void write_words(const uint32_t* sHard, uint32_t* g_out, int nw, int tid)
{
    if ((((size_t)g_out) & 15u) || (nw & 3)) {
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

/* eight nibbles -> eight bits, bit j = nibble j > 0 (lnsfaid_kernel4l.hip) */
__device__ __forceinline__ uint32_t nibbles_positive(uint32_t w)
{
    uint32_t p = (w | (w >> 1) | (w >> 2)) & ~(w >> 3) & 0x11111111u; /* bit 4 j: low three bits not all 0, sign clear */
    p = (p | (p >> 3)) & 0x03030303u;
    p = (p | (p >> 6)) & 0x000f000fu;
    return (p | (p >> 12)) & 0xffu;
}

/* This lane's share of the two counts over the plane's words below L: `corrected` against the codeword's own line words (mother
 * word i is line word i - Sw behind the known range; (L - S) / 32 words or (L - S) / 2 bytes, which staging has read), and the ones
 * decided inside the known range. */
__device__ __forceinline__ void burst_counts(const LfBurstArgs& a, const LbRange& r, const uint32_t* sHard, int lw, int tid, int& corrected,
                                             int& ones)
{
    const uint32_t* src = (const uint32_t*)a.line + (size_t)r.line_off * (a.format == LNSFAID_LINE_HARD ? 1u : 4u);
    int n = 0, k = 0;
    for (int i = tid; i < lw; i += LF_T4) {
        const uint32_t d = sHard[i];
        if (i >= r.k0w && i < r.k1w) {
            k += __popc(d);
            continue;
        }
        const int wl = i - (i >= r.k1w ? r.sw : 0);
        if (a.format == LNSFAID_LINE_HARD) n += __popc(d ^ src[wl]);
        else {
            const uint32_t q0 = src[4 * wl], q1 = src[4 * wl + 1], q2 = src[4 * wl + 2], q3 = src[4 * wl + 3];
            n += __popc(d ^ (nibbles_positive(q0) | nibbles_positive(q1) << 8 | nibbles_positive(q2) << 16 | nibbles_positive(q3) << 24));
        }
    }
    corrected = n;
    ones = k;
}

#define LF4_RULE CW

template <int METHOD, bool RM, bool EF2>
__global__ __launch_bounds__(LF_T4, 2) void lnsfaid_decode4b_kernel(LfBurstArgs a)
{
    LF4_LOCALS()
    LF4_CW_CORE(LF4B_STAGE_INPUT, a.stats)
    /* the lane number as the output sees it: opaque, as in lnsfaid_decode4l_kernel */
    int tid_o = tid;
    asm volatile("" : "+v"(tid_o));
    const LbRange er = lb_range(a, cw, K >> 5);
    /* the known range is the head or the tail of the information words: what is left is one run of (K - S) / 32 words */
    write_words(sHard + (er.k0w == 0 ? er.sw : 0), a.payload + (size_t)er.pay_off, (K >> 5) - er.sw, tid_o);
    if (a.bits) write_words(sHard, a.bits + (size_t)cw * (size_t)nw, nw, tid_o);
    if (a.stats || a.short_ones) {
        int corrected, ones;
        burst_counts(a, er, sHard, first_erased >> 5, tid_o, corrected, ones);
        for (int o = LF_T4 / 2; o > 0; o >>= 1) {
            corrected += __shfl_down(corrected, o);
            ones += __shfl_down(ones, o);
        }
        if (tid_o == 0) {
            if (a.stats) {
                lnsfaid_line_stats st;
                st.iterations = prog <= max_iter ? prog - 1 : max_iter;
                st.bf_iterations = prog <= max_iter ? 0 : prog - t_bf0;
                st.unsatisfied = unsat;
                st.corrected = corrected;
                a.stats[cw] = st;
            }
            if (a.short_ones) a.short_ones[cw] = (uint32_t)ones;
        }
    }
}

/* the same set of instances as lf_decode4l_func */
extern "C" const void* lf_decode4b_func(int method, int ef, int rm)
{
    LF4_INSTANCE_TABLE(lnsfaid_decode4b_kernel)
}
