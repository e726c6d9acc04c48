/*
 * lnsfaid_kernel4l.hip — line-format decode: the per-codeword four-rows-per-lane decoders of
 * lnsfaid_kernel4p.hip (lnsfaid_decode4pcw_kernel) reading a codeword where a line delivers it and writing its payload.
 *
 * Formats (include/lnsfaid.h): with L = n_var - puncture_tail and K = n_var - n_check, both multiples of 32 (the host refuses
 * other codes), codeword cw of `line` is L / 32 words of received bits (LNSFAID_LINE_HARD, bit b of word w = code bit 32 w + b)
 * or L / 2 bytes of two's-complement nibbles (LNSFAID_LINE_LLR4, code bit k in byte k / 2, low nibble for even k), codeword
 * after codeword without gaps; payload is the first K / 32 words of the hard-decision plane, bits (optional) all n_var / 32.
 *
 * Differences from lnsfaid_decode4pcw_kernel:
 *   - staging reads the codeword at line + cw * stride: no group arithmetic, no information / parity split.  A lane loads only
 *     what lies inside the codeword's own L positions (see LF4L_STAGE_INPUT): nothing of the punctured tail exists in `line`;
 *   - the format is a kernel argument, uniform over the launch, branched on in staging and in the corrected count: one set of
 *     instances serves both formats;
 *   - the output is the payload, the plane only when asked for, and a record with the corrected count; no group records.
 * Everything between staging and output is macro text: the per-codeword frame of lnsfaid_frame4.h, the loops of lnsfaid_rows4.h.
 */
#include <hip/hip_runtime.h>

#include "lnsfaid_frame4.h"
#include "lnsfaid_line.h"
#include "lnsfaid_launch.h"

/* ---- staging from a line.  As LF4P_STAGE_INPUT: lane tid owns variable nodes 4 tid .. 4 tid + 3 of every block column, the loads
 * of a round of 23 columns are in flight together, and the four values go to their bytes of the interleaved En image (node n of a
 * column: dword n mod 64, byte n div 64) as En + SW_BIAS_EN.
 *
 * Addresses.  `first_erased` is L, a multiple of 32, so the four nodes of a lane are transmitted together or not at all.
 *   HARD  a block column is 8 words; lane tid reads word wi = 8 cb + tid / 8 of the codeword and takes bits 4 (tid % 8) .. + 3.
 *         It loads only when wi < L / 32: the highest word read is L / 32 - 1, the codeword's last.
 *   LLR4  a block column is 128 bytes; lane tid reads the half-word at byte 128 cb + 2 tid, nodes v0 = 256 cb + 4 tid .. v0 + 3.
 *         It loads only when v0 < L, and then v0 + 3 < L: the highest byte read is (L - 1) / 2, the codeword's last.
 * For the 50G-PON code (L = 67.5 block columns) lanes 32 .. 63 load nothing in column 67 and no lane loads in column 68.  A lane
 * that does not load stages the erasure En = 0, which is what the tail gets in every decoder of this library. ---- */
#define LF4L_STAGE_ROUNDS(LOAD, WIDEN) \
            for (int cb0 = 0; cb0 < nbc; cb0 += SB) {                                                                                     \
                uint32_t w[SB];                                                                                                           \
_Pragma("unroll")                                                                                                                         \
                for (int u = 0; u < SB; ++u) {                                                                                            \
                    const int cb = cb0 + u;                                                                                               \
                    if (cb < nbc) { /* uniform */                                                                                         \
                        const bool inside = cb * LF_Z + 4 * tid < first_erased;                                                           \
                        w[u] = 0u;                                                                                                        \
                        if (inside) w[u] = LOAD;                                                                                          \
                    }                                                                                                                     \
                }                                                                                                                         \
_Pragma("unroll")                                                                                                                         \
                for (int u = 0; u < SB; ++u) {                                                                                            \
                    const int cb = cb0 + u;                                                                                               \
                    if (cb < nbc) {                                                                                                       \
                        const bool inside = cb * LF_Z + 4 * tid < first_erased;                                                           \
                        const uint32_t h = w[u];                                                                                          \
                        uint32_t x;                                                                                                       \
                        WIDEN                                                                                                             \
                        const uint32_t ad = (uint32_t)cb * 256u + base_d;                                                                 \
                        lds.wr8(ad, x); lds.wr8(ad + 4u, x >> 8); lds.wr8(ad + 8u, x >> 16); lds.wr8(ad + 12u, x >> 24);                  \
                    }                                                                                                                     \
                }                                                                                                                         \
            }                                                                                                                             \
    /* end of LF4L_STAGE_ROUNDS */

#define LF4L_STAGE_INPUT() \
        const int first_erased = N - c->puncture_tail; /* L */                                                                           \
        const int nbc = c->nbc;                                                                                                           \
        constexpr int SB = 23;                                                                                                            \
        const uint32_t base_d = ((16u * (uint32_t)tid) & 0xffu) + ((uint32_t)tid >> 4);                                                   \
        const SwLds lds = SwLds();                                                                                                        \
        if (a.format == LNSFAID_LINE_HARD) {                                                                                              \
            const uint32_t* src = (const uint32_t*)a.line + (size_t)cw * (size_t)(first_erased >> 5);                                     \
            /* bit k of the lane's four -> byte k: SW_BIAS_EN - magnitude, plus 2 * magnitude where the bit is set */                     \
            const uint32_t zero4 = (uint32_t)(SW_BIAS_EN - a.magnitude) * 0x01010101u, one = 2u * (uint32_t)a.magnitude;                  \
            LF4L_STAGE_ROUNDS(src[cb * (LF_Z >> 5) + (tid >> 3)],                                                                         \
                /* h * 0x204081: copies of the four bits at 0, 7, 14, 21 (disjoint, no carries); bits 0, 8, 16, 24 of it are bits 0 .. 3 */ \
                x = inside ? zero4 + ((((h >> (4 * (tid & 7))) & 15u) * 0x00204081u) & 0x01010101u) * one                                 \
                           : (uint32_t)SW_BIAS_EN * 0x01010101u;)                                                                         \
        } else {                                                                                                                          \
            const uint8_t* src = (const uint8_t*)a.line + (size_t)cw * (size_t)(first_erased >> 1);                                       \
            LF4L_STAGE_ROUNDS(((const uint16_t*)(src + ((cb * LF_Z) >> 1)))[tid],                                                         \
                x = (h & 0xfu) | ((h & 0xf0u) << 4) | ((h & 0xf00u) << 8) | ((h & 0xf000u) << 12); /* nibble k -> byte k */               \
                x |= (x & 0x08080808u) * 0x1eu; /* sign-extend: 0x8..0xf -> 0xf8..0xff, no carries between bytes */                      \
                (void)inside; /* a lane that did not load holds h = 0: the erasure */                                                     \
                x = ((x & 0x7f7f7f7fu) + (uint32_t)SW_BIAS_EN * 0x01010101u) ^ (x & 0x80808080u);)                                        \
        }                                                                                                                                 \
    /* end of LF4L_STAGE_INPUT */

/* the first nw words of the plane, in the shape of write_bits (lnsfaid_kernel4p.hip): 16-byte stores of four words, the reads of
 * nine rounds before the first store; dword stores for an output that is not 16-byte aligned or a count that is no multiple of 4 */
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

/* eight nibbles -> eight bits, bit j = nibble j > 0 (the channel decision of the FEC status: 0 and every negative value decide 0) */
__device__ __forceinline__ uint32_t nibbles_positive(uint32_t w)
{
    uint32_t p = (w | (w >> 1) | (w >> 2)) & ~(w >> 3) & 0x11111111u; /* bit 4 j: low three bits not all 0, sign clear */
    p = (p | (p >> 3)) & 0x03030303u;
    p = (p | (p >> 6)) & 0x000f000fu;
    return (p | (p >> 12)) & 0xffu;
}

/* lnsfaid_fec_record::corrected of the plane against the codeword's own line: positions below L only, which are the L / 32 words
 * (HARD) or L / 2 bytes (LLR4) staging has read - in L2 by now.  Every lane returns its share; the caller sums over the wave. */
__device__ __forceinline__ int line_corrected(const LfLineArgs& a, const uint32_t* sHard, int L, int cw, int tid)
{
    const int lw = L >> 5;
    int n = 0;
    if (a.format == LNSFAID_LINE_HARD) {
        const uint32_t* src = (const uint32_t*)a.line + (size_t)cw * (size_t)lw;
        for (int i = tid; i < lw; i += LF_T4) n += __popc(sHard[i] ^ src[i]);
    } else {
        const uint32_t* src = (const uint32_t*)a.line + (size_t)cw * (size_t)(L >> 3); /* four words of nibbles per plane word */
        for (int i = tid; i < lw; i += LF_T4) {
            const uint32_t q0 = src[4 * i], q1 = src[4 * i + 1], q2 = src[4 * i + 2], q3 = src[4 * i + 3];
            const uint32_t ch = nibbles_positive(q0) | nibbles_positive(q1) << 8 | nibbles_positive(q2) << 16 | nibbles_positive(q3) << 24;
            n += __popc(sHard[i] ^ ch);
        }
    }
    return n;
}

#define LF4_RULE CW

template <int METHOD, bool RM, bool EF2>
__global__ __launch_bounds__(LF_T4, 2) void lnsfaid_decode4l_kernel(LfLineArgs a)
{
    LF4_LOCALS()
    LF4_CW_CORE(LF4L_STAGE_INPUT, a.stats)
    /* the lane number as the output sees it: opaque, so that no address staging has computed from it (16 * tid) is kept alive -
     * spilled, with the messages in registers - through the whole decode for the stores below */
    int tid_o = tid;
    asm volatile("" : "+v"(tid_o));
    write_words(sHard, a.payload + (size_t)cw * (size_t)(K >> 5), K >> 5, tid_o);
    if (a.bits) write_words(sHard, a.bits + (size_t)cw * (size_t)nw, nw, tid_o);
    if (a.stats) {
        int corrected = line_corrected(a, sHard, first_erased, cw, tid_o);
        for (int o = LF_T4 / 2; o > 0; o >>= 1) corrected += __shfl_down(corrected, o);
        if (tid_o == 0) {
            lnsfaid_line_stats st;
            st.iterations = prog <= max_iter ? prog - 1 : max_iter;
            st.bf_iterations = prog <= max_iter ? 0 : prog - t_bf0;
            st.unsatisfied = unsat;
            st.corrected = corrected;
            a.stats[cw] = st;
        }
    }
}

/* the same set of instances as lf_decode4p_func(.., per_codeword = 1) */
extern "C" const void* lf_decode4l_func(int method, int ef, int rm)
{
    LF4_INSTANCE_TABLE(lnsfaid_decode4l_kernel)
}
