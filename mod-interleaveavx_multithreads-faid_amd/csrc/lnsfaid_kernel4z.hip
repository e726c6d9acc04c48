/*
 * lnsfaid_kernel4z.hip - the one-wave-per-codeword decode kernel of lnsfaid_kernel4.hip (group rule, messages in registers, int8
 * I/O) with a layer step that does not rotate on identity circulants.
 *
 * A quarter of the 50G-PON code's circulants have shift 0 (68 of 275), as is usual for quasi-cyclic base matrices.  Through such
 * an edge lane i reads dword i of the block column with its four rows already in byte order, so the five instructions the layer
 * step spends per edge on the rotation (lane + shift, the rotate amount, the rotate after the read, 4 - amount and the rotate in
 * front of the write-back) do nothing.  The host orders every layer's edges zero-shift first in tables of this kernel's own
 * (LfDevCode zsbplain / zs4tab / zcbtab; the order of a row's edges is free) and stores per layer which instance of
 * the step runs it: its degree and the number ZG of leading groups of four zero-shift edges, rounded down to a compiled instance
 * (the rotating code is correct for shift 0).  sw_layer_step<.., ZG> (lnsfaid_swar.h) drops the rotation work of those groups.
 *
 * Everything but the layered iteration is the text of lnsfaid_kernel4.hip and the macros of lnsfaid_rows4.h; the kernels of
 * lnsfaid_kernel4.hip keep their instances, names and instructions.  Built for the instances <M, RM = true, EF2 = false> of
 * DecodeMethods 1..5; every other configuration stays on lnsfaid_kernel4.hip.
 */
#include <hip/hip_runtime.h>

#define LF4_MAIN_STEP main_step4z
#include "lnsfaid_rows4.h"

/* ---- the compiled (degree, ZG) instances.  -DLF4Z_SMALL_SET (an experiment build): the two-instances-per-degree set, fewer hot
 * blocks and a shorter dispatch for fewer instructions saved (DESIGN.md 3.1d has both measured). ---- */
#ifdef LF4Z_SMALL_SET
#define LF4Z_INSTANCES(X) X(0, 23, 0) X(1, 23, 4) X(2, 22, 5) X(3, 22, 0)
#else
#define LF4Z_INSTANCES(X) X(0, 23, 0) X(1, 23, 1) X(2, 23, 2) X(3, 23, 4) X(4, 22, 5) X(5, 22, 0)
#endif

/* The instance code of a layer of degree deg with zg leading zero-shift groups (LfDevCode zinst): degree << 16 | ZG in use << 8 |
 * one bit per compiled instance.  The instance is that of the largest compiled ZG <= zg of the degree; no bit (the generic-degree
 * instance, ZG 0) for every other degree.  One bit per way and not a number: a chain of equality tests becomes a switch, which the
 * compiler lowers to a search tree in an order of its own, and the chain below is ordered by how often each way is taken. */
extern "C" int lf_decode4z_inst(int deg, int zg)
{
    int best = -1, way = -1;
#define LF4Z_ROUND(W, D, G) if (deg == (D) && (G) <= zg && (G) > best) { best = (G); way = (W); }
    LF4Z_INSTANCES(LF4Z_ROUND)
#undef LF4Z_ROUND
    return (deg << 16) | ((best < 0 ? 0 : best) << 8) | (way < 0 ? 0 : 1 << way);
}

/* the layer step's view of this kernel's edge tables (DevTab4 of lnsfaid_rows4.h reads the reference's order) */
struct DevTab4Z {
    CCode c;
    int br;
    uint32_t sbv; /* lane j < 32: zsbplain[br][j] */
    __device__ __forceinline__ uint32_t s4(int j) const { return c->zs4tab[br][j]; }
    __device__ __forceinline__ uint32_t cb256(int j) const { return c->zcbtab[br][j]; }
    __device__ __forceinline__ uint32_t sb_dyn4(uint32_t idx4) const
    {
        return (uint32_t)__builtin_amdgcn_ds_bpermute((int)idx4, (int)sbv);
    }
};

/* ---- one layered iteration: main_step4's messages-in-registers loop (lnsfaid_rows4.h) over the zero-first tables, with ONE scalar
 * per layer, the instance code, in the place of the degree.  The chain is ordered by how many layers of the 50G-PON code take
 * each way: (23, 0) runs 6 of 12. ---- */
template <int METHOD, bool ERA, bool RM>
__device__ __forceinline__ void main_step4z(CCode c, CCfg f, const LfDevCode* gc, SwRow* __restrict__ rows, SwRegs& R, int lane, int it, const uint32_t* sP,
                                            bool have_par, bool lme, uint32_t era_plane)
{
    static_assert(RM && !ERA, "built for the messages-in-registers, non-erasing instances only");
    (void)rows; (void)era_plane;
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
    const int nbr = c->nbr;
    const SwLds lds = SwLds();
    uint32_t tabv = gc->zsbplain[0][lane & 31];
#pragma nounroll
    for (int br = 0; br < nbr; ++br) {
        const int brn = br + 1 < nbr ? br + 1 : 0;
        const uint32_t tabn = gc->zsbplain[brn][lane & 31]; /* next layer's edge table, a layer ahead of its use */
        const int inst = c->zinst[br];
        uint32_t rowpar = 0;
        if (have_par) { /* syndrome bits of rows lane + 64 k of this layer as byte masks */
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t wv = sP[br * 8 + 2 * k + (lane >> 5)];
                rowpar |= ((wv >> (lane & 31)) & 1u) ? (0xffu << (8 * k)) : 0u;
            }
        }
        DevTab4Z tab;
        tab.c = c; tab.br = br; tab.sbv = tabv;
        const SwRow cur = regs_get(R, br);
        SwRow st;
#define LF4Z_WAY(W, D, G) if (inst & (1 << (W))) st = sw_layer_step<METHOD, D, false, 1, 0, G>(lds, tab, p, K, (uint32_t)lane, D, cur, fresh, rowpar, lme); else
        LF4Z_INSTANCES(LF4Z_WAY)
#undef LF4Z_WAY
            st = sw_layer_step<METHOD, 0>(lds, tab, p, K, (uint32_t)lane, inst >> 16, cur, fresh, rowpar, lme);
        /* the six indexed writes back to back (see main_step4) */
        __builtin_amdgcn_sched_barrier(0);
        regs_put(R, br, st);
        __builtin_amdgcn_sched_barrier(0);
        tabv = tabn;
    }
}

/* the group rule, as in lnsfaid_kernel4.hip */
#define LF4_ON_FRONT prog >= kmax
#define LF4_CLEAN_STOPS(t) prog >= kmax && !group_passed(a.live, g, prog, t)
#define LF4_ON_STOP(t) if (RM && prog >= 2) regs_store(R, g_rows, c->nbr, t);
#define LF4_ON_PASS(t) publish_pass(a.live, cw, prog, t);

/* ---- the decode kernel: lnsfaid_decode4_kernel<METHOD, true, false> of lnsfaid_kernel4.hip, statement for statement ---- */
template <int METHOD>
__global__ __launch_bounds__(LF_T4, 2) void lnsfaid_decode4z_kernel(LfKernelArgs a)
{
    constexpr bool RM = true, EF2 = false; /* the instances this kernel is built for (the decode loops of lnsfaid_rows4.h name them) */
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

extern "C" const void* lf_decode4z_func(int method)
{
    switch (method) {
    case 1: return (const void*)lnsfaid_decode4z_kernel<1>;
    case 2: return (const void*)lnsfaid_decode4z_kernel<2>;
    case 3: return (const void*)lnsfaid_decode4z_kernel<3>;
    case 4: return (const void*)lnsfaid_decode4z_kernel<4>;
    case 5: return (const void*)lnsfaid_decode4z_kernel<5>;
    default: return nullptr;
    }
}

extern "C" hipError_t lf_launch_decode4z(int method, const LfKernelArgs* args, size_t lds_bytes, hipStream_t stream)
{
    const void* fn = lf_decode4z_func(method);
    if (!fn) return hipErrorInvalidValue;
    void* kargs[] = { (void*)args };
    return hipLaunchKernel(fn, dim3((unsigned)args->n_cw), dim3(LF_T4), kargs, lds_bytes, stream);
}
