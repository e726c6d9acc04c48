/*
 * lnsfaid_kernel4e.hip - the window-free layer-static decode kernel of lnsfaid_kernel4w.hip with the rotating edges' dword address and
 * rotate amounts read from a table instead of computed (SW_FORM_EDGEW of sw_layer_step, lnsfaid_swar.h).
 *
 * What a lane needs of a rotating edge - the dword (lane + shift) mod 64 of the block column, the byte rotation of the read and its
 * inverse for the write-back - depends on the lane and the code alone, yet lnsfaid_kernel4w.hip computes it, four instructions per
 * edge, in every layer of every iteration of every codeword.  Here the three are fields of one word per edge and lane
 * (sw50_edge_word, lnsfaid_static50.h) in a table of 56 KB compiled into this file, the same for every codeword: two instructions per
 * edge are left (the address mask and the shift in front of the write-back rotate).  A layer's words arrive one layer ahead, a
 * 16-byte load per group of four edges, issued inside the layer before where pass 2 gives registers back (Lf4eEw::at).
 *
 * Everything else is lnsfaid_kernel4w.hip: the two forms of the iteration, the decision points, the frame.  The host launches this
 * kernel in its place unless edge words are switched off (lnsfaid_select_edge_words).  Built for DecodeMethods 1..5 like it.
 */
#include <hip/hip_runtime.h>

#define LF4_MAIN_STEP main_step4e
#define LF4_DIRTY_CHECK(c, lane) dirty4e(lane)
#include "lnsfaid_frame4.h"
#include "lnsfaid_static50.h"
#include "lnsfaid_launch.h"

static_assert(SW50_LAYERS == LF4_RM_LAYERS, "one register of every message vector per layer");

/* the edge words of all layers: [layer][group of four rotating edges][lane][4] */
__device__ const Sw50EdgeImage lf4e_edge_words = sw50_edge_image();

/* ---- the decision points' cheap "certainly dirty" test: dirty4w of lnsfaid_kernel4w.hip ---- */
__device__ __forceinline__ bool dirty4e(int lane)
{
    const SwLds lds = SwLds();
    asm volatile("; lf4e check stage 1");
    const uint32_t w1 = sw50_row_parity<SW50_CHECK_LAYER>(lds, (uint32_t)lane);
    if (__ballot((w1 & 0x80808080u) != 0u) != 0ull) return true;
    asm volatile("; lf4e check stage 2");
    const uint32_t w0 = sw50_row_parity<0>(lds, (uint32_t)lane);
    return __ballot((w0 & 0x80808080u) != 0u) != 0ull;
}

/* the forms of lnsfaid_kernel4w.hip, each with the edge words on top.  Not in the instance of DecodeMethod 3: its bit-flipping stage
 * (the plain flip, lnsfaid_rows4.h) keeps more alive across the layered loop than the others', and with the loaded register
 * quadruples next to that the allocator spills (102 registers, wherever the loads sit: DESIGN.md 3.1k).  That instance keeps the
 * step of lnsfaid_kernel4w.hip and loads no words. */
#define LF4E_EW(METHOD) ((METHOD) == 3 ? 0 : SW_FORM_EDGEW)
#define LF4E_MIDDLE(METHOD) (SW_FORM_NOWIN | SW_FORM_VK | SW_FORM_MUL | LF4E_EW(METHOD))
#define LF4E_FIRST(METHOD) (LF4E_MIDDLE(METHOD) | SW_FORM_FRESH)

#define LF4E_MAX_GROUPS 6 /* 23 rotating edges at the most */
constexpr int LF4E_GROUPS0 = sw50_edge_groups(0);

/* group g of layer BR's words for this lane (lane16: 16 * lane, the lane's byte offset inside a group) */
template <int BR>
__device__ __forceinline__ void load_words4e(uint32_t lane16, int g, uint32_t* w)
{
    constexpr int G0 = sw50_edge_group_base(BR);
    const uint4 v = *(const uint4*)((const char*)lf4e_edge_words.w + (size_t)((G0 + g) * SW50_EDGE_GROUP_WORDS * 4) + lane16);
    w[4 * g] = v.x; w[4 * g + 1] = v.y; w[4 * g + 2] = v.z; w[4 * g + 3] = v.w;
}

/* Where the next layer's groups are loaded.  Pass 2 of the step gives the registers of four edges back behind every group's
 * write-back (tb, ms, ad and the word itself), so group g of the next layer is asked for behind the write-back of this layer's
 * group g: nothing is alive longer than in lnsfaid_kernel4w.hip, and the loads have the rest of the layer to arrive. */
template <int BR>
struct Lf4eEw {
    static constexpr int NZ = Sw50Tab<BR>::NZ;
    static constexpr int NEXT = BR + 1 < SW50_LAYERS ? BR + 1 : 0;
    static constexpr int NG = BR + 1 < SW50_LAYERS ? sw50_edge_groups(NEXT) : 0; /* (layer 0's arrive in front of the iteration) */
    static constexpr int LAST = (Sw50Tab<BR>::DEG - 1) / SW_ILP * SW_ILP;          /* this layer's last group of pass 2 */
    const uint32_t* cur;
    uint32_t* next;
    uint32_t lane16;
    /* (edges of equal shift have equal words: the address and the shifted word are made from the first one's register, once, as
     * lnsfaid_kernel4w.hip makes lane + shift once for them; the read rotate takes the edge's own, or the compiler would narrow
     * the 16-byte loads around the words nobody reads) */
    static constexpr int first_of(int j)
    {
        for (int i = NZ; i < j; ++i)
            if (Sw50Tab<BR>::L.s4[i] == Sw50Tab<BR>::L.s4[j]) return i;
        return j;
    }
    __device__ __forceinline__ uint32_t w(int j) const { return cur[j - NZ]; }
    __device__ __forceinline__ uint32_t wa(int j) const { return cur[first_of(j) - NZ]; }
    __device__ __forceinline__ void at(int point) const
    {
        const int g0 = point / SW_ILP, g1 = point == LAST ? NG : (g0 + 1 < NG ? g0 + 1 : NG); /* (a short layer's last point takes what is left) */
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int g = g0; g < g1; ++g) load_words4e<NEXT>(lane16, g, next);
        __builtin_amdgcn_sched_barrier(0);
    }
};

/* layer BR of the iteration: layer4w of lnsfaid_kernel4w.hip on this layer's words `w`; leaves the next layer's there */
template <int METHOD, int FORM, int BR>
__device__ __forceinline__ void layer4e(const uint32_t (*zsb)[32], SwRegs& R, const SwLds& lds, const SwParams& p, const SwK& K, int lane, uint32_t lane16,
                                        bool fresh, uint32_t& tabv, uint32_t* w)
{
    typedef Sw50Tab<BR> Tab;
    /* the lane number as this layer sees it: opaque, so that nothing derived from it is kept alive from one layer to the other.
     * (And lane16, so that its zero extension is made in this layer, where the loads' address selection sees it: base in SGPRs plus a
     * 32-bit offset register; extended once in front of the forms it is a 64-bit addition per load.) */
    asm volatile("; lf4e layer %2" : "+v"(lane), "+v"(lane16) : "n"(BR));
    uint32_t tabn = 0u;
    /* next layer's edge table, a layer ahead of its use (`lane` is 4 * lane, the table's byte offset in its bits 2 .. 6) */
    if (BR + 1 < SW50_LAYERS) tabn = *(const uint32_t*)((const char*)zsb[BR + 1] + (lane & 0x7c));
    Tab tab;
    tab.sbv = tabv;
    uint32_t wn[4 * LF4E_MAX_GROUPS];
    const Lf4eEw<BR> ew = { w, wn, lane16 };
    const SwRow zero = { { 0u, 0u, 0u }, 0u, { 0u, 0u } };
    SwRow cur = (FORM & SW_FORM_FRESH) ? zero : regs_get(R, BR); /* (iteration 1 starts from regs_clear: the same values) */
    /* the record's unpacking belongs to THIS layer: without a fixed point the compiler starts it inside the layer before */
    if (!(FORM & SW_FORM_FRESH)) asm volatile("" : "+v"(cur.cw));
    SwRow st = sw_layer_step<METHOD, Tab::DEG, false, 1, 0, 0, SW_PAIRS_ALL, FORM>(lds, tab, p, K, (uint32_t)lane, Tab::DEG, cur,
                                                                                  (FORM & SW_FORM_FRESH) ? true : fresh, 0u, false, 0u, 0u, SwNoXch(), ew);
    /* The record is complete HERE (layer4s: without a fixed point the packing of the sign words sinks to the record's next use) */
    asm volatile("" : "+v"(st.x[0]), "+v"(st.x[1]), "+v"(st.x[2]), "+v"(st.cw), "+v"(st.pa[0]), "+v"(st.pa[1]));
    __builtin_amdgcn_sched_barrier(0);
    regs_put(R, BR, st);
    __builtin_amdgcn_sched_barrier(0);
    tabv = tabn;
#pragma unroll
    for (int i = 0; i < 4 * Lf4eEw<BR>::NG; ++i) w[i] = wn[i];
}

/* the twelve layers in one form.  The comment lines in the assembly ("lf4e <form> begin", "lf4e layer <n>", "lf4e <form> end") delimit
 * what tests/test_edge_words_isa.py counts */
template <int METHOD, int FORM>
__device__ __forceinline__ void layers4e(const uint32_t (*zsb)[32], SwRegs& R, const SwLds& lds, const SwParams& p, const SwK& K, int lane, uint32_t lane16,
                                         bool fresh, uint32_t tabv, uint32_t* w)
{
#define LF4E_LAYER(BR) layer4e<METHOD, FORM, BR>(zsb, R, lds, p, K, lane, lane16, fresh, tabv, w);
    LF4E_LAYER(0) LF4E_LAYER(1) LF4E_LAYER(2) LF4E_LAYER(3) LF4E_LAYER(4) LF4E_LAYER(5)
    LF4E_LAYER(6) LF4E_LAYER(7) LF4E_LAYER(8) LF4E_LAYER(9) LF4E_LAYER(10) LF4E_LAYER(11)
#undef LF4E_LAYER
}

/* ---- one layered iteration: main_step4w (lnsfaid_kernel4w.hip), with layer 0's words asked for first of all ---- */
template <int METHOD, bool ERA, bool RM>
__device__ __forceinline__ void main_step4e(CCode c, CCfg f, const LfDevCode* gc, SwRow* __restrict__ rows, SwRegs& R, int lane, int it, const uint32_t* sP,
                                            bool have_par, bool lme, uint32_t era_plane)
{
    static_assert(RM && !ERA, "built for the messages-in-registers, non-erasing instances only");
    (void)c; (void)rows; (void)era_plane; (void)sP; (void)have_par; (void)lme;
    it = __builtin_amdgcn_readfirstlane(it);
    const uint32_t lane16 = (uint32_t)lane << 4;
    uint32_t w[4 * LF4E_MAX_GROUPS];
#pragma unroll
    for (int g = 0; g < (LF4E_EW(METHOD) ? LF4E_GROUPS0 : 0); ++g) load_words4e<0>(lane16, g, w);
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
        for (int k = 0; k < 4; ++k) K.tm[k] = sw_vconst(tm[k], (uint32_t)it);
    }
    K.c100 = sw_vconst(0x100u, (uint32_t)it); /* the factor of sw_shl8_mul */
    const int lane_arg = lane << 2;           /* SW_FORM_MUL takes 4 * lane: shifted here once, not in every layer */
    const SwLds lds = SwLds();
    /* the arg-min tables of all layers behind ONE base register, the layer in the loads' offset field (main_step4s) */
    uint32_t z = 0u;
    asm volatile("" : "+s"(z));
    const uint32_t (*zsb)[32] = (const uint32_t (*)[32])((const char*)gc->zsbplain + z);
    const uint32_t tabv = zsb[0][lane & 31];
    __builtin_amdgcn_sched_barrier(0);
    if (first) { /* (regs_clear, or a codeword parked in front of iteration 1: every message is still 0) */
        asm volatile("; lf4e first begin");
        layers4e<METHOD, LF4E_FIRST(METHOD)>(zsb, R, lds, p, K, lane_arg, lane16, true, tabv, w);
        asm volatile("; lf4e first end");
    } else {
        asm volatile("; lf4e middle begin");
        layers4e<METHOD, LF4E_MIDDLE(METHOD)>(zsb, R, lds, p, K, lane_arg, lane16, false, tabv, w);
        asm volatile("; lf4e middle end");
    }
}

#define LF4_RULE GROUP

/* ---- the decode kernel: lnsfaid_decode4w_kernel<METHOD> of lnsfaid_kernel4w.hip ---- */
template <int METHOD>
__global__ __launch_bounds__(LF_T4, 2) void lnsfaid_decode4e_kernel(LfKernelArgs a_)
{
    constexpr bool RM = true, EF2 = false; /* the instances this kernel is built for (the decode loops of lnsfaid_rows4.h name them) */
    LF4_SPLIT_ARGS()
    LF4_GROUP_FRAME(LF4_STAGE_INPUT, write_decoded, int8_t, N)
}

extern "C" const void* lf_decode4e_func(int method)
{
    LF4_METHOD_TABLE(lnsfaid_decode4e_kernel)
}
