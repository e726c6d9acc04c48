/*
 * lnsfaid_kernel4w.hip - the layer-static decode kernel of lnsfaid_kernel4s.hip for configurations whose error-floor window cannot
 * open (floor_iter_thresh < 0: the shipped DecodeMethod 2), with the layered iteration in two straight-line forms: the first
 * iteration and every later one.
 *
 * lnsfaid_kernel4s.hip compiles ONE straight-line iteration that must serve every configuration and every iteration: each layer tests
 * whether the rows' syndrome bits are wanted, looks the row's magnitudes up in two tables and selects between them, and the first
 * iteration reads a record that is all zero.  Here the iteration is compiled with the window known absent (SW_FORM_NOWIN of
 * sw_layer_step, lnsfaid_swar.h: no syndrome bits, one table composed with the thermometer decode), and iteration 1 runs on a text
 * that knows the record to be zero (SW_FORM_FRESH).  (A third form for iteration max_iter, which builds a record nobody reads, does
 * not fit the register file next to these two: DESIGN.md 3.1i.)
 *
 * The host launches this kernel where it would launch lnsfaid_kernel4s.hip and the context's floor_iter_thresh is negative; the
 * decision point in front of every iteration, the resume of a parked codeword at any decision point and everything outside the
 * layered iteration are the text that file is made of (lnsfaid_frame4.h, lnsfaid_rows4.h).  Built for DecodeMethods 1..5 like it.
 */
#include <hip/hip_runtime.h>

#define LF4_MAIN_STEP main_step4w
#define LF4_DIRTY_CHECK(c, lane) dirty4w(lane)
#include "lnsfaid_frame4.h"
#include "lnsfaid_static50.h"
#include "lnsfaid_launch.h"

static_assert(SW50_LAYERS == LF4_RM_LAYERS, "one register of every message vector per layer");

/* ---- the cheap "certainly dirty" test of a decision point on the compiled tables, two stages of straight-line code (DESIGN.md
 * 3.1f): the row parity of the layer with the most identity circulants, and only where that finds nothing the parity of layer 0, the
 * layer lnsfaid_rows4.h's layer0_dirty4 asks - so whatever that test proves dirty, this one does.  The comment lines in the assembly
 * delimit what tests/test_decision_point_isa.py walks. ---- */
__device__ __forceinline__ bool dirty4w(int lane)
{
    const SwLds lds = SwLds();
    asm volatile("; lf4w check stage 1");
    const uint32_t w1 = sw50_row_parity<SW50_CHECK_LAYER>(lds, (uint32_t)lane);
    if (__ballot((w1 & 0x80808080u) != 0u) != 0ull) return true;
    asm volatile("; lf4w check stage 2");
    const uint32_t w0 = sw50_row_parity<0>(lds, (uint32_t)lane);
    return __ballot((w0 & 0x80808080u) != 0u) != 0ull;
}

/* What both forms of the iteration know (SW_FORM_NOWIN), and what the first one knows on top.  The experiment switches
 * -DLF4W_KEEP_WINDOW / -DLF4W_KEEP_FIRST (tools/gpu_variants.sh) take one part out each, for its own A/B run. */
#ifdef LF4W_KEEP_WINDOW
#define LF4W_BASE 0
#else
#define LF4W_BASE SW_FORM_NOWIN
#endif
#ifdef LF4W_KEEP_FIRST
#define LF4W_FRESH 0
#else
#define LF4W_FRESH SW_FORM_FRESH
#endif
/* How both forms are written: constants of full-rate instructions in registers instead of SGPRs (SW_FORM_VK), the single
 * left shifts as multiplies by a register (SW_FORM_MUL).  -DLF4W_KEEP_SGPR / -DLF4W_KEEP_SHIFTS take one part out each, as above. */
#ifdef LF4W_KEEP_SGPR
#define LF4W_VK 0
#else
#define LF4W_VK SW_FORM_VK
#endif
#ifdef LF4W_KEEP_SHIFTS
#define LF4W_MUL 0
#else
#define LF4W_MUL SW_FORM_MUL
#endif
#define LF4W_CLASS (LF4W_VK | LF4W_MUL)

/* layer BR of the iteration: layer4s of lnsfaid_kernel4s.hip without the rows' syndrome bits, on the step of the iteration's FORM */
template <int METHOD, int FORM, int BR>
__device__ __forceinline__ void layer4w(const uint32_t (*zsb)[32], SwRegs& R, const SwLds& lds, const SwParams& p, const SwK& K, int lane, bool fresh,
                                        uint32_t& tabv)
{
    typedef Sw50Tab<BR> Tab;
    /* the lane number as this layer sees it: opaque, so that what two layers derive from it alike (edges of equal shift: their dword
     * address and rotate amounts) is computed in each of them, not kept alive - spilled - from one to the other */
    asm volatile("; lf4w layer %1" : "+v"(lane) : "n"(BR));
    uint32_t tabn = 0u;
    /* next layer's edge table, a layer ahead of its use (SW_FORM_MUL: `lane` is 4 * lane, the table's byte offset in its bits 2 .. 6) */
    if (BR + 1 < SW50_LAYERS) tabn = (FORM & SW_FORM_MUL) ? *(const uint32_t*)((const char*)zsb[BR + 1] + (lane & 0x7c)) : zsb[BR + 1][lane & 31];
    Tab tab;
    tab.sbv = tabv;
    const SwRow zero = { { 0u, 0u, 0u }, 0u, { 0u, 0u } };
    SwRow cur = (FORM & SW_FORM_FRESH) ? zero : regs_get(R, BR); /* (iteration 1 starts from regs_clear: the same values) */
    /* the record's unpacking belongs to THIS layer: without a fixed point the compiler starts it inside the layer before */
    if (!(FORM & SW_FORM_FRESH)) asm volatile("" : "+v"(cur.cw));
    SwRow st = sw_layer_step<METHOD, Tab::DEG, false, 1, 0, 0, SW_PAIRS_ALL, FORM>(lds, tab, p, K, (uint32_t)lane, Tab::DEG, cur,
                                                                                  (FORM & SW_FORM_FRESH) ? true : fresh, 0u, false);
    /* The record is complete HERE (layer4s: without a fixed point the packing of the sign words sinks to the record's next use) */
    asm volatile("" : "+v"(st.x[0]), "+v"(st.x[1]), "+v"(st.x[2]), "+v"(st.cw), "+v"(st.pa[0]), "+v"(st.pa[1]));
    __builtin_amdgcn_sched_barrier(0);
    regs_put(R, BR, st);
    __builtin_amdgcn_sched_barrier(0);
    tabv = tabn;
}

/* the twelve layers in one form.  The comment lines in the assembly ("lf4w <form> begin", "lf4w layer <n>", "lf4w <form> end") delimit
 * what tests/test_window_free_isa.py counts */
template <int METHOD, int FORM>
__device__ __forceinline__ void layers4w(const uint32_t (*zsb)[32], SwRegs& R, const SwLds& lds, const SwParams& p, const SwK& K, int lane, bool fresh,
                                         uint32_t tabv)
{
#define LF4W_LAYER(BR) layer4w<METHOD, FORM, BR>(zsb, R, lds, p, K, lane, fresh, tabv);
    LF4W_LAYER(0) LF4W_LAYER(1) LF4W_LAYER(2) LF4W_LAYER(3) LF4W_LAYER(4) LF4W_LAYER(5)
    LF4W_LAYER(6) LF4W_LAYER(7) LF4W_LAYER(8) LF4W_LAYER(9) LF4W_LAYER(10) LF4W_LAYER(11)
#undef LF4W_LAYER
}

/* ---- one layered iteration: main_step4s (lnsfaid_kernel4s.hip) in the form of iteration `it`.  have_par and lme are what the
 * decision point found; outside the window, i.e. always here, nothing reads them. ---- */
template <int METHOD, bool ERA, bool RM>
__device__ __forceinline__ void main_step4w(CCode c, CCfg f, const LfDevCode* gc, SwRow* __restrict__ rows, SwRegs& R, int lane, int it, const uint32_t* sP,
                                            bool have_par, bool lme, uint32_t era_plane)
{
    static_assert(RM && !ERA, "built for the messages-in-registers, non-erasing instances only");
    (void)c; (void)rows; (void)era_plane; (void)sP; (void)have_par; (void)lme;
    it = __builtin_amdgcn_readfirstlane(it);
    SwK K = sw_consts((uint32_t)it);
    const bool first = (it == 1);
    const int itx = (it >= 1 && it <= 5) ? it - 1 : 5;
    SwParams p;
    p.lut_lo = f->lut_lo[itx][0]; p.lut_hi = f->lut_hi[itx][0];
    p.ef_lo = f->lut_ef_lo[itx][0]; p.ef_hi = f->lut_ef_hi[itx][0];
    p.f1 = f->factor_1; p.f2 = f->factor_2;
    p.window = false;
    p.ef_tables = f->ef >= 1;
    if (LF4_OMS(METHOD)) sw_oms_tables(p);
    {
        /* the row's one table composed with the thermometer decode: four words, built here once per iteration on the scalar unit */
        uint32_t tm[4];
        sw_therm2msg_tables(LF4_OMS(METHOD) ? p.oms_lo[0] : p.lut_lo, LF4_OMS(METHOD) ? p.oms_hi[0] : p.lut_hi, tm);
#pragma unroll
        for (int w = 0; w < 4; ++w) K.tm[w] = sw_vconst(tm[w], (uint32_t)it);
    }
    if (LF4W_MUL) K.c100 = sw_vconst(0x100u, (uint32_t)it); /* the factor of sw_shl8_mul */
    const int lane_arg = LF4W_MUL ? lane << 2 : lane; /* SW_FORM_MUL takes 4 * lane: shifted here once, not in every layer */
    const SwLds lds = SwLds();
    /* the arg-min tables of all layers behind ONE base register, the layer in the loads' offset field (main_step4s) */
    uint32_t z = 0u;
    asm volatile("" : "+s"(z));
    const uint32_t (*zsb)[32] = (const uint32_t (*)[32])((const char*)gc->zsbplain + z);
    const uint32_t tabv = zsb[0][lane & 31];
    __builtin_amdgcn_sched_barrier(0);
    if (first) { /* (regs_clear, or a codeword parked in front of iteration 1: every message is still 0) */
        asm volatile("; lf4w first begin");
        layers4w<METHOD, LF4W_BASE | LF4W_FRESH | LF4W_CLASS>(zsb, R, lds, p, K, lane_arg, true, tabv);
        asm volatile("; lf4w first end");
    } else {
        asm volatile("; lf4w middle begin");
        layers4w<METHOD, LF4W_BASE | LF4W_CLASS>(zsb, R, lds, p, K, lane_arg, false, tabv);
        asm volatile("; lf4w middle end");
    }
}

#define LF4_RULE GROUP

/* ---- the decode kernel: lnsfaid_decode4s_kernel<METHOD> of lnsfaid_kernel4s.hip - the argument split (LF4_SPLIT_ARGS) and the
 * group-rule frame (LF4_GROUP_FRAME) of lnsfaid_frame4.h ---- */
template <int METHOD>
__global__ __launch_bounds__(LF_T4, 2) void lnsfaid_decode4w_kernel(LfKernelArgs a_)
{
    constexpr bool RM = true, EF2 = false; /* the instances this kernel is built for (the decode loops of lnsfaid_rows4.h name them) */
    LF4_SPLIT_ARGS()
    LF4_GROUP_FRAME(LF4_STAGE_INPUT, write_decoded, int8_t, N)
}

extern "C" const void* lf_decode4w_func(int method)
{
    LF4_METHOD_TABLE(lnsfaid_decode4w_kernel)
}
