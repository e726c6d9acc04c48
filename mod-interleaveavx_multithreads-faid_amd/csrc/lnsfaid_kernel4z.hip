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
 * Everything but the layered iteration is the text lnsfaid_kernel4.hip is made of - the group-rule frame of lnsfaid_frame4.h, the
 * loops of lnsfaid_rows4.h; the kernels of
 * lnsfaid_kernel4.hip keep their instances, names and instructions.  Built for the instances <M, RM = true, EF2 = false> of
 * DecodeMethods 1..5; every other configuration stays on lnsfaid_kernel4.hip.
 */
#include <hip/hip_runtime.h>

#define LF4_MAIN_STEP main_step4z
#include "lnsfaid_frame4.h"
#include "lnsfaid_launch.h"

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

#define LF4_RULE GROUP

/* ---- the decode kernel: the frame of lnsfaid_decode4_kernel<METHOD, true, false> (LF4_GROUP_FRAME, lnsfaid_frame4.h) ---- */
template <int METHOD>
__global__ __launch_bounds__(LF_T4, 2) void lnsfaid_decode4z_kernel(LfKernelArgs a)
{
    constexpr bool RM = true, EF2 = false; /* the instances this kernel is built for (the decode loops of lnsfaid_rows4.h name them) */
    LF4_GROUP_FRAME(LF4_STAGE_INPUT, write_decoded, int8_t, N)
}

extern "C" const void* lf_decode4z_func(int method)
{
    LF4_METHOD_TABLE(lnsfaid_decode4z_kernel)
}
