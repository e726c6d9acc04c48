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
 * points' cheap "certainly dirty" test (dirty4s) is the text of that file.  Built for DecodeMethods 1..5 like it.
 */
#include <hip/hip_runtime.h>

#define LF4_MAIN_STEP main_step4s
#define LF4_DIRTY_CHECK(c, lane) dirty4s(lane)
#include "lnsfaid_rows4.h"
#include "lnsfaid_static50.h"

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

/* the group rule, as in lnsfaid_kernel4.hip */
#define LF4_ON_FRONT prog >= kmax
#define LF4_CLEAN_STOPS(t) prog >= kmax && !group_passed(a.live, g, prog, t)
#define LF4_ON_STOP(t) if (RM && prog >= 2) regs_store(R, g_rows, c->nbr, t);
#define LF4_ON_PASS(t) publish_pass(a.live, cw, prog, t);

/* ---- the decode kernel: lnsfaid_decode4_kernel<METHOD, true, false> of lnsfaid_kernel4.hip, statement for statement ---- */
template <int METHOD>
__global__ __launch_bounds__(LF_T4, 2) void lnsfaid_decode4s_kernel(LfKernelArgs a_)
{
    constexpr bool RM = true, EF2 = false; /* the instances this kernel is built for (the decode loops of lnsfaid_rows4.h name them) */
    /* the two pointers the decode loop uses, split off the kernel arguments: the compiler holds those as ONE tuple of sixteen
     * registers, spilled and reloaded whole wherever a field of it is wanted (twice inside layer 0).  An opaque zero is added
     * instead of constraining the pointers themselves, which would lose their address space (flat loads in every layer). */
    LfKernelArgs a = a_;
    {
        uint32_t z = 0u;
        asm volatile("" : "+s"(z));
        a.code = (const LfDevCode*)((const char*)a_.code + z);
        a.cfg = (const LfDevCfg*)((const char*)a_.cfg + z);
    }
    extern __shared__ __align__(16) unsigned char smem[];
    CCode c = (CCode)a.code;
    CCfg f = (CCfg)a.cfg;
    const int tid = (int)threadIdx.x;
    const int cw = (int)blockIdx.x;
    const int N = c->n_var, M = c->n_check, K = c->k_info, nw = c->n_words, pw = c->p_words;
    /* (the layer step addresses En by its LDS offset: the dynamic segment must start at 0, i.e. the kernel must have no static
     * LDS - checked on the host when a context picks its kernel, lnsfaid_capi.hip kernel_check) */
    uint32_t* sHard0 = (uint32_t*)smem;      /* bit-flipping stage: hard_ch and hard2 overlay the dead En */
    uint32_t* sHard2 = (uint32_t*)smem + nw;
    uint32_t* sHard = (uint32_t*)(smem + lf_lds_off_hard(N));
    uint32_t* sP = (uint32_t*)(smem + lf_lds_off_p(N, nw));
    int* sStat = (int*)(smem + lf_lds_off_stat(N, nw, pw));
    int* sRed = sStat + LNSFAID_GROUP;

    const int max_iter = f->max_iter, max_bf = f->max_bf;
    const int t_bf0 = max_iter + 1;   /* first bit-flipping decision point */
    const int t_end = t_bf0 + max_bf; /* both loops exhausted               */

    /* snapshot of the 32 lanes of this group: one load per lane (both halves of the wave hold the same 32 words), everything
     * else in registers - no LDS round trips in front of the early exits, which most workgroups of a relaunch take */
    const int g = cw >> 5, lane_in_group = cw & 31;
    const int sv = a.status_cur ? a.status_cur[g * LNSFAID_GROUP + (tid & 31)] : 0; /* null: first launch of a batch, every codeword fresh */
    const int my_status = __builtin_amdgcn_readlane(sv, lane_in_group);
    if (my_status & LF_DONE) { /* uniform exit */
        if (tid == 0) a.status_next[cw] = my_status;
        return;
    }
    if (tid == LNSFAID_GROUP) sRed[LF_ZERO_SLOT] = 0; /* the word unused synw slots point at */
    int kmax;
    {
        int v = sv & LF_PROG_MASK; /* maximum over lanes 0..31, same DPP pattern as add_reduce32 (values are not negative) */
        v = imax(v, __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false));
        v = imax(v, __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false));
        v = imax(v, __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false));
        v = imax(v, __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false));
        v = imax(v, __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false));
        kmax = __builtin_amdgcn_readlane(v, 31);
    }
    const int all_same = __ballot(sv != my_status) == 0ull;
    LF_WG_SYNC();
    int prog = my_status & LF_PROG_MASK;

    uint32_t* g_en = (uint32_t*)(a.st_en + (size_t)cw * (size_t)N);
    SwRow* g_rows = (SwRow*)(a.st_rows + (size_t)cw * (size_t)(c->nbr * LF_T)); /* the 2-row kernel's slot: 16 B x 128 >= 24 B x 64 */
    uint32_t* g_bits = a.st_bits + (size_t)cw * (size_t)(3 * nw);
    int8_t* g_out = a.decoded + (size_t)cw * (size_t)N;

    /* parked on the group's front, not everybody there yet: nothing to do in this launch */
    if (prog != 0 && prog == kmax && !all_same) {
        if (tid == 0) { a.status_next[cw] = my_status; atomicAdd(a.remaining, 1u); }
        return;
    }

    /* all 32 lanes parked clean at the same decision point: the group stops there (the reference's break).  Every lane
     * wrote its hard decisions when it parked, so nothing is left to do but to say so. */
    if (my_status != 0 && all_same) {
        if (tid == 0) {
            a.status_next[cw] = my_status | LF_DONE;
            if (a.stats && lane_in_group == 0) {
                lnsfaid_group_stats st;
                st.iterations = prog <= max_iter ? prog - 1 : max_iter;
                st.bf_iterations = prog <= max_iter ? 0 : prog - t_bf0;
                a.stats[g] = st;
            }
        }
        return;
    }

    bool in_bf = max_bf > 0 && prog >= t_bf0 && prog != 0;
    LfLaneState ls = { 0, 0, 0, 0 };
    SwRegs R; /* RM: the codeword's compressed messages (dead in the bit-flipping stage) */
    if (RM) regs_clear(R);

    /* ---- bring the codeword's state on chip ---- */
    if (prog == 0) {
        LF4_STAGE_INPUT()
        LF_WG_SYNC();
        prog = 1;
    } else if (!in_bf) {
        copy_in<23>((uint32_t*)smem, g_en, N >> 2, tid);
        if (RM && prog >= 2) regs_load(R, g_rows, c->nbr, tid); /* parked in front of iteration 1: every Lmn is still 0 */
        LF_WG_SYNC();
    } else {
        copy_in<9>(sHard, g_bits, nw, tid);
        copy_in<9>(sHard0, g_bits + nw, nw, tid);
        copy_in<9>(sHard2, g_bits + 2 * nw, nw, tid);
        ls = a.st_lane[cw];
        LF_WG_SYNC();
    }

    bool parked = false;
    uint32_t pA = 0, pB = 0;
    /* ---- layered iterations (the syndrome stage in front of iteration prog is decision point prog) ---- */
    if (!in_bf) {
        LF4_LAYERED_LOOP()
        LF4_ENTER_BF()
    }
    /* ---- bit-flipping iterations.  Nothing of the layer step is alive here, so the lanes keep their entries of the walk
     * tables in registers for the whole stage (no table load, hence no exposed memory latency, per iteration) ---- */
    LF4_BF_LOOPS()

    const bool finished = prog >= t_end;
    if (finished) {
        if (!in_bf) build_plane4<false>(c, sHard, 0, tid);
        write_decoded(sHard, g_out, N, tid);
        if (tid == 0) {
            a.status_next[cw] = prog | LF_DONE;
            if (a.stats && lane_in_group == 0) {
                lnsfaid_group_stats st;
                st.iterations = prog <= max_iter ? prog - 1 : max_iter;
                st.bf_iterations = prog <= max_iter ? 0 : prog - t_bf0;
                a.stats[g] = st;
            }
        }
    } else {
        /* park clean at decision point prog: state back to HBM for the case that the group goes on, and the hard decisions
         * (the syndrome stage has just built the plane from this En; in the bit-flipping stage the plane is the state) as the
         * output for the case that it stops here */
        if (!in_bf) {
            copy_out<23>(g_en, (const uint32_t*)smem, N >> 2, tid); /* (RM: the messages were stored where the codeword parked) */
        } else {
            copy_out<9>(g_bits, sHard, nw, tid);
            copy_out<9>(g_bits + nw, sHard0, nw, tid);
            copy_out<9>(g_bits + 2 * nw, sHard2, nw, tid);
            if (tid == 0) a.st_lane[cw] = ls;
        }
        write_decoded(sHard, g_out, N, tid);
        if (tid == 0) { a.status_next[cw] = prog; atomicAdd(a.remaining, 1u); }
    }
}

extern "C" const void* lf_decode4s_func(int method)
{
    switch (method) {
    case 1: return (const void*)lnsfaid_decode4s_kernel<1>;
    case 2: return (const void*)lnsfaid_decode4s_kernel<2>;
    case 3: return (const void*)lnsfaid_decode4s_kernel<3>;
    case 4: return (const void*)lnsfaid_decode4s_kernel<4>;
    case 5: return (const void*)lnsfaid_decode4s_kernel<5>;
    default: return nullptr;
    }
}

extern "C" hipError_t lf_launch_decode4s(int method, const LfKernelArgs* args, size_t lds_bytes, hipStream_t stream)
{
    const void* fn = lf_decode4s_func(method);
    if (!fn) return hipErrorInvalidValue;
    void* kargs[] = { (void*)args };
    return hipLaunchKernel(fn, dim3((unsigned)args->n_cw), dim3(LF_T4), kargs, lds_bytes, stream);
}
