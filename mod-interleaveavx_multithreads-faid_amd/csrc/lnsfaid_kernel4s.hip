/*
 * lnsfaid_kernel4s.hip - the rotation-free decode kernel of lnsfaid_kernel4z.hip with every layer of the built-in 50G-PON code on a
 * layer step compiled for that layer.
 *
 * lnsfaid_kernel4z.hip runs the twelve layers through one loop that does not know which layer it is in: the messages in registers
 * are read and written through indexed moves, the layer's instance of the step is found by a chain of bit tests on a loaded code,
 * shifts and block columns arrive in scalar loads and enter the arithmetic as SGPR operands, and only whole leading groups of four
 * identity circulants go without rotation.  Here the layered iteration is straight-line code over the twelve layers with the layer
 * number, its degree, shifts and block columns as compile-time constants (Sw50Tab<BR>, lnsfaid_static50.h): plain register names
 * for the messages, no dispatch, no table loads, literals for the shifts, the block column in the LDS instructions' offset field,
 * and every identity circulant rotation-free.  The per-lane edge table of the arg-min look-up stays a loaded value.
 *
 * The host launches this kernel only for a code whose zero-first tables equal the compiled ones entry by entry
 * (lf_decode4s_matches); every other code stays on lnsfaid_kernel4z.hip.  Everything but the layered iteration and the decision
 * points' cheap "certainly dirty" test (dirty4s) is the text that file is made of (lnsfaid_frame4.h,
 * lnsfaid_rows4.h).  Built for DecodeMethods 1..5 like it.
 */
#include <hip/hip_runtime.h>

#define LF4_MAIN_STEP main_step4s
#define LF4_DIRTY_CHECK(c, lane) dirty4s(lane)
#include "lnsfaid_frame4.h"
#include "lnsfaid_static50.h"
#include "lnsfaid_launch.h"

static_assert(SW50_LAYERS == LF4_RM_LAYERS, "one register of every message vector per layer");

/* the context's code is the compiled one: layers, degrees and the zero-first edge tables the layer step's constants stand for */
extern "C" int lf_decode4s_matches(const LfDevCode* code)
{
    constexpr Sw50Code k = sw50_build();
    if (!code || code->nbr != SW50_LAYERS) return 0;
    for (int br = 0; br < SW50_LAYERS; ++br) {
        if (code->deg[br] != k.layer[br].deg) return 0;
        for (int j = 0; j < k.layer[br].deg; ++j) {
            if (code->zs4tab[br][j] != k.layer[br].s4[j] || code->zcbtab[br][j] != k.layer[br].cb256[j]) return 0;
            if (code->zsbplain[br][j] != ((k.layer[br].cb256[j] << 16) | k.layer[br].s4[j])) return 0;
        }
    }
    return 1;
}

/* ---- the cheap "certainly dirty" test of a decision point on the compiled tables, two stages of straight-line code (DESIGN.md
 * 3.1f): the row parity of the layer with the most identity circulants, and only where that finds nothing the parity of layer 0, the
 * layer lnsfaid_rows4.h's layer0_dirty4 asks - so whatever that test proves dirty, this one does.  The comment lines in the assembly
 * delimit what tests/test_decision_point_isa.py walks. ---- */
__device__ __forceinline__ bool dirty4s(int lane)
{
    const SwLds lds = SwLds();
    asm volatile("; lf4s check stage 1");
    const uint32_t w1 = sw50_row_parity<SW50_CHECK_LAYER>(lds, (uint32_t)lane);
    if (__ballot((w1 & 0x80808080u) != 0u) != 0ull) return true;
    asm volatile("; lf4s check stage 2");
    const uint32_t w0 = sw50_row_parity<0>(lds, (uint32_t)lane);
    return __ballot((w0 & 0x80808080u) != 0u) != 0ull;
}

/* layer BR of the iteration: main_step4z's loop body with BR a constant */
template <int METHOD, int BR>
__device__ __forceinline__ void layer4s(const uint32_t (*zsb)[32], SwRegs& R, const SwLds& lds, const SwParams& p, const SwK& K, int lane, bool fresh,
                                        const uint32_t* sP, bool have_par, bool lme, uint32_t& tabv)
{
    typedef Sw50Tab<BR> Tab;
    /* the lane number as this layer sees it: opaque, so that what two layers derive from it alike (edges of equal shift: their dword
     * address and rotate amounts) is computed in each of them, not kept alive - spilled - from one to the other */
    asm volatile("; lf4s layer %1" : "+v"(lane) : "n"(BR));
    uint32_t tabn = 0u;
    if (BR + 1 < SW50_LAYERS) tabn = zsb[BR + 1][lane & 31]; /* next layer's edge table, a layer ahead of its use */
    uint32_t rowpar = 0;
    if (have_par) { /* syndrome bits of rows lane + 64 k of this layer as byte masks */
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t wv = sP[BR * 8 + 2 * k + (lane >> 5)];
            rowpar |= ((wv >> (lane & 31)) & 1u) ? (0xffu << (8 * k)) : 0u;
        }
    }
    Tab tab;
    tab.sbv = tabv;
    const SwRow cur = regs_get(R, BR);
    SwRow st = sw_layer_step<METHOD, Tab::DEG, false, 1, 0, 0, SW_PAIRS_ALL>(lds, tab, p, K, (uint32_t)lane, Tab::DEG, cur, fresh, rowpar, lme);
    /* The record is complete HERE.  With a constant layer number regs_put is a renaming, not six moves: nothing else holds the
     * compiler from sinking the packing of the sign words to the record's next use, an iteration later, with the layer's 23 sign
     * masks alive (spilled) until then. */
    asm volatile("" : "+v"(st.x[0]), "+v"(st.x[1]), "+v"(st.x[2]), "+v"(st.cw), "+v"(st.pa[0]), "+v"(st.pa[1]));
    __builtin_amdgcn_sched_barrier(0);
    regs_put(R, BR, st);
    __builtin_amdgcn_sched_barrier(0);
    tabv = tabn;
}

/* ---- one layered iteration: main_step4z (lnsfaid_kernel4z.hip) unrolled over the twelve layers.  The comment lines in the
 * assembly ("lf4s layers begin", "lf4s layer <n>", "lf4s layers end") delimit what tests/test_static_layers_isa.py counts: the layers,
 * without the iteration's set-up in front of them, as the trips of lnsfaid_kernel4z.hip's layer loop are counted. ---- */
template <int METHOD, bool ERA, bool RM>
__device__ __forceinline__ void main_step4s(CCode c, CCfg f, const LfDevCode* gc, SwRow* __restrict__ rows, SwRegs& R, int lane, int it, const uint32_t* sP,
                                            bool have_par, bool lme, uint32_t era_plane)
{
    static_assert(RM && !ERA, "built for the messages-in-registers, non-erasing instances only");
    (void)c; (void)rows; (void)era_plane;
    it = __builtin_amdgcn_readfirstlane(it);
    const SwK K = sw_consts((uint32_t)it);
    const bool fresh = (it == 1);
    const int rem = f->max_iter - it;
    const int itx = (it >= 1 && it <= 5) ? it - 1 : 5;
    SwParams p;
    p.lut_lo = f->lut_lo[itx][0]; p.lut_hi = f->lut_hi[itx][0];
    p.ef_lo = f->lut_ef_lo[itx][0]; p.ef_hi = f->lut_ef_hi[itx][0];
    p.f1 = f->factor_1; p.f2 = f->factor_2;
    p.window = rem <= f->floor_iter_thresh;
    p.ef_tables = f->ef >= 1;
    if (LF4_OMS(METHOD)) sw_oms_tables(p);
    const SwLds lds = SwLds();
    /* the arg-min tables of all layers behind ONE base register, the layer in the loads' offset field.  The base is made per
     * iteration (an opaque zero added): as twelve loop-invariant addresses the compiler keeps twelve register pairs alive
     * through the whole loop, and the scalar registers of the decode loop are spilled around them */
    uint32_t z = 0u;
    asm volatile("" : "+s"(z));
    const uint32_t (*zsb)[32] = (const uint32_t (*)[32])((const char*)gc->zsbplain + z);
    uint32_t tabv = zsb[0][lane & 31];
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("; lf4s layers begin");
#define LF4S_LAYER(BR) layer4s<METHOD, BR>(zsb, R, lds, p, K, lane, fresh, sP, have_par, lme, tabv);
    LF4S_LAYER(0) LF4S_LAYER(1) LF4S_LAYER(2) LF4S_LAYER(3) LF4S_LAYER(4) LF4S_LAYER(5)
    LF4S_LAYER(6) LF4S_LAYER(7) LF4S_LAYER(8) LF4S_LAYER(9) LF4S_LAYER(10) LF4S_LAYER(11)
#undef LF4S_LAYER
    asm volatile("; lf4s layers end");
}

#define LF4_RULE GROUP

/* ---- the decode kernel: the frame of lnsfaid_decode4_kernel<METHOD, true, false> (LF4_GROUP_FRAME, lnsfaid_frame4.h) behind the
 * split of the two pointers the decode loop uses off the kernel arguments (LF4_SPLIT_ARGS, same file) ---- */
template <int METHOD>
__global__ __launch_bounds__(LF_T4, 2) void lnsfaid_decode4s_kernel(LfKernelArgs a_)
{
    constexpr bool RM = true, EF2 = false; /* the instances this kernel is built for (the decode loops of lnsfaid_rows4.h name them) */
    LF4_SPLIT_ARGS()
    LF4_GROUP_FRAME(LF4_STAGE_INPUT, write_decoded, int8_t, N)
}

extern "C" const void* lf_decode4s_func(int method)
{
    LF4_METHOD_TABLE(lnsfaid_decode4s_kernel)
}
