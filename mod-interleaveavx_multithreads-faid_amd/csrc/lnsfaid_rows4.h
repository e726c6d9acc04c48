/*
 * lnsfaid_rows4.h - what the four-rows-per-lane decode kernels share outside the layer step: the code-table view the layer step
 * reads, staging copies, the hard-decision / confidence bit planes, the live-progress words, output staging, the erasure plane of
 * EF_ELIMINATION 2, and (at the end) the decode loops of the one-wave-per-codeword kernels.  Included by lnsfaid_kernel4.hip (one wave per codeword) and lnsfaid_kernel5.hip (two waves per codeword, where
 * LF_WG_SYNC() is redefined to the one-wave fence before this header is read: everything here runs on ONE wave).
 */
#ifndef LNSFAID_ROWS4_H
#define LNSFAID_ROWS4_H

#include "lnsfaid_device.h"
#include "lnsfaid_phases.h"
#include "lnsfaid_swar.h"

#define LF_T4 64

#define LF4_OMS(M) ((M) == 1 || (M) == 3 || (M) == 4)

struct DevTab4 {
    CCode c;
    int br;
    uint32_t sbv; /* lane j < 32: (block column * 256) << 16 | 4 * shift of edge j of this layer */
    __device__ __forceinline__ uint32_t sb(int j) const { return c->circ[br][j].sb; }
    /* the same split on the host (4 * shift, block column * 256): contiguous tables, so the 23 values of a layer arrive in a
     * few wide scalar loads and no scalar arithmetic is left per edge */
    __device__ __forceinline__ uint32_t s4(int j) const { return c->s4tab[br][j]; }
    __device__ __forceinline__ uint32_t cb256(int j) const { return c->cbtab[br][j]; }
    __device__ __forceinline__ uint32_t sb_dyn4(uint32_t idx4) const
    {
        return (uint32_t)__builtin_amdgcn_ds_bpermute((int)idx4, (int)sbv);
    }
};

typedef __attribute__((address_space(3))) uint32_t lds4_u32;
__device__ __forceinline__ uint32_t lds4_rd(uint32_t a) { return *(const lds4_u32*)(size_t)a; }
__device__ __forceinline__ void lds4_wr(uint32_t a, uint32_t v) { *(lds4_u32*)(size_t)a = v; }

/* n words from global memory into LDS, B loads per lane in flight at a time: with two waves per SIMD a "load, wait, store" loop
 * exposes one memory round trip per word */
template <int B>
__device__ __forceinline__ void copy_in(uint32_t* dst, const uint32_t* __restrict__ src, int n, int tid)
{
    for (int i0 = 0; i0 < n; i0 += B * LF_T4) {
        uint32_t w[B];
#pragma unroll
        for (int u = 0; u < B; ++u) { const int i = i0 + u * LF_T4 + tid; w[u] = i < n ? src[i] : 0u; }
#pragma unroll
        for (int u = 0; u < B; ++u) { const int i = i0 + u * LF_T4 + tid; if (i < n) dst[i] = w[u]; }
    }
}

/* n words from LDS to global memory (or LDS), B reads per lane in flight at a time */
template <int B>
__device__ __forceinline__ void copy_out(uint32_t* __restrict__ dst, const uint32_t* src, int n, int tid)
{
    for (int i0 = 0; i0 < n; i0 += B * LF_T4) {
        uint32_t w[B];
#pragma unroll
        for (int u = 0; u < B; ++u) { const int i = i0 + u * LF_T4 + tid; w[u] = i < n ? src[i] : 0u; }
#pragma unroll
        for (int u = 0; u < B; ++u) { const int i = i0 + u * LF_T4 + tid; if (i < n) dst[i] = w[u]; }
    }
}

__device__ __forceinline__ uint32_t hard_flags(uint32_t x) { return sw_hard_flags(x); } /* En > 0: bit 7 of every byte */

/* ---- bit plane from the interleaved En image: hard decision (CDecoder_FAID.cpp:299, :6416-6419) or, with CONF, the 2B1C
 * confidence bit |En| >= thr (CDecoder_FAID_2B1C.cpp:6132-6136).  Lane d holds variable nodes d, d + 64, d + 128, d + 192 of a
 * block column in one dword, and plane word (column, k, h) wants the flags of byte k of lanes 32 h .. 32 h + 31.  Eight columns
 * at a time: every lane collects its 8 x 4 flags in one word (bit 8 k + u: byte k of column cb0 + u), the two halves of the
 * wave transpose their 32 x 32 bit matrices in five exchange steps (lane ^ j for j = 16 .. 1: rows and columns swap bit j),
 * after which lane 8 k + u of half h holds plane word (cb0 + u, k, h).  About 60 instructions per eight columns, against
 * 32 ballots + 64 v_writelane_b32 before. */
template <int J>
__device__ __forceinline__ uint32_t plane_exchange(uint32_t x, uint32_t l5)
{
    constexpr uint32_t m_lo = J == 16 ? 0x0000ffffu : J == 8 ? 0x00ff00ffu : J == 4 ? 0x0f0f0f0fu : J == 2 ? 0x33333333u : 0x55555555u;
    uint32_t t;
    if (J == 1) t = (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0xb1, 0xf, 0xf, false);      /* quad_perm [1,0,3,2] */
    else if (J == 2) t = (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x4e, 0xf, 0xf, false); /* quad_perm [2,3,0,1] */
    else t = (uint32_t)__builtin_amdgcn_ds_swizzle((int)x, 0x1f | (J << 10));               /* lane ^ J inside 32 lanes */
    const bool up = (l5 & (uint32_t)J) != 0u;
    /* rows with bit J clear keep their low columns and take the partner's low columns as their high ones, and vice versa */
    const uint32_t r = __builtin_amdgcn_alignbit(t, t, up ? (uint32_t)J : 32u - (uint32_t)J);
    const uint32_t keep = up ? ~m_lo : m_lo;
    return (x & keep) | (r & ~keep);
}

template <bool CONF>
__device__ __forceinline__ void build_plane4(CCode c, uint32_t* plane, int thr, int lane)
{
    /* (inlined on purpose: as a function of its own the column count is no longer known to be uniform, and every column
     * becomes a masked branch with an LDS round trip of its own) */
    const int nbc = c->nbc;
    const int th = thr < 1 ? 0 : (thr > 32 ? 32 : thr); /* |En| <= 31: a threshold above 31 means "never" */
    const uint32_t th4 = (uint32_t)th * 0x01010101u;
    const uint32_t b8 = (uint32_t)(128 - SW_BIAS_EN) * 0x01010101u, b7 = (uint32_t)(127 - SW_BIAS_EN) * 0x01010101u;
    const uint32_t l5 = (uint32_t)lane & 31u;
    const int word_of_lane = (int)((l5 & 7u) * 8u + 2u * (l5 >> 3) + ((uint32_t)lane >> 5)); /* + cb0 * 8 */
    for (int cb0 = 0; cb0 < nbc; cb0 += 8) {
        uint32_t x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) /* columns beyond the last one re-read it; their words are not stored */
            x[u] = lds4_rd((uint32_t)(cb0 + u < nbc ? cb0 + u : nbc - 1) * 256u + 4u * (uint32_t)lane);
        __builtin_amdgcn_sched_barrier(0); /* the eight reads in flight together */
        uint32_t g = 0;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            uint32_t fl;
            /* En >= thr  <=>  Eb + 8 - thr >= 128;  En <= -thr  <=>  Eb + 7 + thr < 128 (no carries: Eb in [89, 151]) */
            if (CONF) fl = th == 0 ? 0x80808080u : (((x[u] + b8) - th4) | ~(x[u] + b7 + th4));
            else fl = hard_flags(x[u]);
            g |= (fl >> (7 - u)) & (0x01010101u << u); /* bit 7 of byte k -> bit 8 k + u */
        }
        g = plane_exchange<16>(g, l5);
        g = plane_exchange<8>(g, l5);
        g = plane_exchange<4>(g, l5);
        g = plane_exchange<2>(g, l5);
        g = plane_exchange<1>(g, l5);
        if (cb0 + (int)(l5 & 7u) < nbc) plane[cb0 * 8 + word_of_lane] = g;
    }
    LF_WG_SYNC();
}

/* ---- cheap "certainly dirty" test (DecodeMethod 2, see lnsfaid_kernels.hip): parity of the lane's four rows of layer 0
 * straight from En (sw_row_parity, lnsfaid_swar.h): any unsatisfied row proves the codeword dirty. */
static_assert(SW_MAX_DEG == LF_MAX_DEG, "sw_row_parity reads whole rows of LfDevCode's tables");
__device__ __forceinline__ bool layer0_dirty4(CCode c, int lane)
{
    uint32_t acc = sw_row_parity(SwLds(), c->s4tab[0], c->cbtab[0], c->deg[0], (uint32_t)lane);
    /* the word is complete HERE: without this the scalar registers of lnsfaid_kernel4z.hip's layer loop are allocated differently
     * and a byte constant is re-made inside every degree-23 layer block (one instruction above tests/test_zero_shift_isa.py) */
    asm volatile("" : "+v"(acc));
    return __ballot((acc & 0x80808080u) != 0u) != 0ull;
}
/* The same test with every table access and LDS read under `j < deg`, as all kernels had it: a basic block, a scalar load and a wait
 * per edge and table (46 dependent round trips per decision point for the 50G-PON code).  lnsfaid_kernel4.hip stays on it
 * (LF4_DIRTY_CHECK): with the straight-line text the register allocation of its layer blocks comes out two VALU instructions
 * (spill reloads) above the ratchets of tests/test_layer_trip_count.py, pinned or not. */
__device__ __forceinline__ bool layer0_dirty4_edgewise(CCode c, int lane)
{
    const int deg = c->deg[0];
    const uint32_t tid4 = (uint32_t)lane << 2;
    uint32_t x4[LF_MAX_DEG], d[LF_MAX_DEG];
    /* all addresses, then all reads, then the arithmetic: one LDS round trip instead of one per circulant */
#pragma unroll
    for (int j = 0; j < LF_MAX_DEG; ++j) x4[j] = j < deg ? tid4 + c->s4tab[0][j] : 0u;
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < LF_MAX_DEG; ++j)
        if (j < deg) d[j] = lds4_rd((x4[j] & 0xfcu) | c->cbtab[0][j]);
    __builtin_amdgcn_sched_barrier(0);
    uint32_t acc = 0;
#pragma unroll
    for (int j = 0; j < LF_MAX_DEG; ++j)
        if (j < deg) acc ^= hard_flags(__builtin_amdgcn_alignbyte(d[j], d[j], x4[j] >> 8));
    return __ballot((acc & 0x80808080u) != 0u) != 0ull;
}

/* ---- live progress of the group -----------------------------------------------------------------
 * A codeword may pass decision point t once it is PROVEN that its group does not stop there.  The snapshot of the previous
 * launch gives such proofs (a lane parked beyond t); this gives more of them while the launch runs: every codeword
 * publishes the point it is about to pass (agent-scope store, monotonic), and whoever passed t first must have been dirty
 * at t, so "some lane of my group has passed t" proves that the group goes on.  A clean codeword looks once, never waits:
 * without a proof it parks exactly as before, so results do not depend on timing, only the number of relaunches does.
 * MEASURED (profiles/r02_kernel4/live_progress.txt): bit-exact, one launch fewer, but not faster - the same iterations are
 * executed either way (SQ_INSTS_VALU 9.55 G against 9.68 G per batch at 3.6 dB) and the codewords that find no proof leave a
 * thin, long second launch (41 Gb/s against 51 Gb/s at 3.6 dB, 102 Gb/s either way at 4.2 dB).  Built only with
 * -DLF4_LIVE_PROOF; what is kept from the experiment is the speculative output of a parking codeword (below). */
__device__ __forceinline__ void publish_pass(int32_t* live, int cw, int t, int tid)
{
#ifdef LF4_LIVE_PROOF
    if (tid == 0) __hip_atomic_store(&live[cw], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
}
__device__ __forceinline__ bool group_passed(const int32_t* live, int g, int t, int tid)
{
#ifndef LF4_LIVE_PROOF
    return false;
#else
    int v = 0;
    if (tid < LNSFAID_GROUP) v = __hip_atomic_load(&live[g * LNSFAID_GROUP + tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return __ballot(v >= t) != 0ull;
#endif
}

/* decodedBits of this codeword from the hard-decision plane (CDecoder_FAID.cpp:7091-7102, CDecoder_OMS.cpp:2966-2967): one plane
 * word = 32 output bytes per lane and round, the plane words of all rounds read before the first store */
__device__ __forceinline__ void write_decoded(const uint32_t* sHard, int8_t* g_out, int N, int tid)
{
    const int nw = N >> 5;
    if (((size_t)g_out) & 15u) { /* caller's buffer not 16-byte aligned: dword stores */
        uint32_t* out32 = (uint32_t*)g_out;
        for (int i = tid; i < (N >> 2); i += LF_T4) out32[i] = (((sHard[i >> 3] >> ((i & 7) * 4)) & 15u) * 0x00204081u) & 0x01010101u;
        return;
    }
    uint4* out = (uint4*)g_out;
    for (int r0 = 0; r0 * LF_T4 < nw; r0 += 9) {
        uint32_t w[9];
#pragma unroll
        for (int u = 0; u < 9; ++u) { const int i = (r0 + u) * LF_T4 + tid; w[u] = i < nw ? sHard[i] : 0u; }
#pragma unroll
        for (int u = 0; u < 9; ++u) {
            const int i = (r0 + u) * LF_T4 + tid;
            if (i < nw) {
                uint32_t d[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) d[q] = (((w[u] >> (4 * q)) & 15u) * 0x00204081u) & 0x01010101u; /* bit k -> byte k */
                out[2 * i] = make_uint4(d[0], d[1], d[2], d[3]);
                out[2 * i + 1] = make_uint4(d[4], d[5], d[6], d[7]);
            }
        }
    }
}

/* ---- EF_ELIMINATION 2: bit plane "every check of this variable node is unsatisfied" over the block columns of weight W
 * (flip_vote[v] >= REGULAR_COL_WEIGHT, CDecoder_FAID.cpp:306-309, :675), bit-sliced like the flip decision: per (column,
 * 64-node window) the AND of the W rotated windows of the parity plane.  Written over the hard-decision plane, which is dead
 * between the syndrome stage and the next one. */
__device__ void build_erasure_plane4(CCode c, const LfDevCode* gc, uint32_t* plane, const uint32_t* sP, int W, int tid)
{
    const int units = c->n_wcols * 4;
    for (int u = tid; u < units; u += LF_T4) {
        const int cb = gc->wcol[u >> 2];
        const uint32_t win = (uint32_t)(u & 3);
        uint32_t lo = 0xffffffffu, hi = 0xffffffffu;
        for (int k = 0; k < W; ++k) {
            const uint32_t cc = gc->colcirc[cb][k];
            uint32_t a, b;
            window64(sP + (cc & 0xffu) * 8u, (64u * win - ((cc >> 8) & 0xffu)) & 255u, a, b);
            lo &= a; hi &= b;
        }
        plane[cb * 8 + 2 * (int)win] = lo;
        plane[cb * 8 + 2 * (int)win + 1] = hi;
    }
    LF_WG_SYNC();
}

/* ==== the decoder of the one-wave kernels as forced-inline pieces: the messages in registers, one layered iteration, input
 * staging, the layered loop with its syndrome stages, the entry into the bit-flipping stage and the bit-flipping loop.  Used by
 * lnsfaid_kernel4.hip (the reference's group-of-32 early stop: parking and relaunches) and lnsfaid_kernel4cw.hip
 * (every codeword stops on its own: one launch).  The two rules differ only in what a clean syndrome does; the
 * GROUP template parameter of the loops selects it. ==== */

/* ---- the compressed messages of the codeword on chip (RM instances) ------------------------------------------------
 * A lane's four rows are 6 dwords per layer (SwRow), 72 per codeword for the 12 layers of the 50G-PON code: they stay in
 * registers for the whole launch, field f of layer br in element br of vector f.  The layer number is wave-uniform, so an
 * access is one v_mov_b32 under s_set_gpr_idx_on (no scratch, no waterfall).  Codes with more than LF4_RM_LAYERS layers
 * stream the messages through HBM one layer ahead of use (the !RM instances). */
#define LF4_RM_LAYERS 12
static_assert(LF4_RM_LAYERS * 16 <= LF_SYN_ROUNDS * 64, "the RM instances assume that the syndrome walk tables fit the register cache");
typedef uint32_t lf4_vec __attribute__((ext_vector_type(LF4_RM_LAYERS)));
struct SwRegs {
    lf4_vec x0, x1, x2, cw, pa0, pa1;
};
__device__ __forceinline__ SwRow regs_get(const SwRegs& R, int br)
{
    SwRow r;
    r.x[0] = R.x0[br]; r.x[1] = R.x1[br]; r.x[2] = R.x2[br]; r.cw = R.cw[br]; r.pa[0] = R.pa0[br]; r.pa[1] = R.pa1[br];
    return r;
}
__device__ __forceinline__ void regs_put(SwRegs& R, int br, const SwRow& r)
{
    R.x0[br] = r.x[0]; R.x1[br] = r.x[1]; R.x2[br] = r.x[2]; R.cw[br] = r.cw; R.pa0[br] = r.pa[0]; R.pa1[br] = r.pa[1];
}

/* ---- one layered iteration (lnsfaid_swar.h does the rows) ---- */
template <int METHOD, bool ERA, bool RM>
__device__ __forceinline__ void main_step4(CCode c, CCfg f, const LfDevCode* gc, SwRow* __restrict__ rows, SwRegs& R, int lane, int it, const uint32_t* sP,
                           bool have_par, bool lme, uint32_t era_plane)
{
    /* register constants of the layer step: built per iteration (17 moves), outside the layer loop and the per-degree instances,
     * and dead again before the syndrome stage - kept alive across it they are spilled (they come from asm statements, which
     * the compiler cannot rematerialise) */
    it = __builtin_amdgcn_readfirstlane(it); /* uniform, and the compiler must know it: a divergent iteration number turns the
                                              * scalar branches and table loads of every layer into masked / per-lane ones */
    const SwK K = sw_consts((uint32_t)it);
    const bool fresh = (it == 1); /* no iteration has run yet: every Lmn is still 0, nothing in HBM */
    const int rem = f->max_iter - it;
    const int itx = (it >= 1 && it <= 5) ? it - 1 : 5; /* switch at CDecoder_FAID.cpp:760-779 */
    SwParams p;
    p.lut_lo = f->lut_lo[itx][0]; p.lut_hi = f->lut_hi[itx][0];
    p.ef_lo = f->lut_ef_lo[itx][0]; p.ef_hi = f->lut_ef_hi[itx][0];
    p.f1 = f->factor_1; p.f2 = f->factor_2;
    p.window = rem <= f->floor_iter_thresh;
    p.ef_tables = f->ef >= 1;
    if (LF4_OMS(METHOD)) sw_oms_tables(p); /* uniform: scalar work, once per iteration */
    if (METHOD == 0) { p.nms_t[0] = f->nms_t[0]; p.nms_t[1] = f->nms_t[1]; p.nms_t[2] = f->nms_t[2]; p.nms_t[3] = f->nms_t[3]; }
    const int nbr = c->nbr;
    const SwLds lds = SwLds();
    const SwRow zero = { { 0u, 0u, 0u }, 0u, { 0u, 0u } }; /* Lmn = 0 before the first iteration (CDecoder_FAID.cpp:211-214) */
    if (RM) {
        /* messages in registers: no vector memory operation inside the layer loop (the registers hold zeros before the first
         * iteration: the kernel clears them when it stages a fresh codeword) */
        uint32_t tabv = gc->sbplain[0][lane & 31];
#pragma nounroll
        for (int br = 0; br < nbr; ++br) {
            const int brn = br + 1 < nbr ? br + 1 : 0;
            const uint32_t tabn = gc->sbplain[brn][lane & 31]; /* next layer's edge table, a layer ahead of its use */
            const int deg = c->deg[br];
            uint32_t rowpar = 0;
            if (have_par) { /* syndrome bits of rows lane + 64 k of this layer as byte masks */
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t wv = sP[br * 8 + 2 * k + (lane >> 5)];
                    rowpar |= ((wv >> (lane & 31)) & 1u) ? (0xffu << (8 * k)) : 0u;
                }
            }
            DevTab4 tab;
            tab.c = c; tab.br = br; tab.sbv = tabv;
            const SwRow cur = regs_get(R, br);
            SwRow st;
            const uint32_t era_edges = ERA ? c->era_edges[br] : 0u;
            if (ERA) st = sw_layer_step<METHOD, 0, ERA>(lds, tab, p, K, (uint32_t)lane, deg, cur, fresh, rowpar, lme, era_edges, era_plane); /* rare: one instance */
            else if (deg == 23) st = sw_layer_step<METHOD, 23>(lds, tab, p, K, (uint32_t)lane, deg, cur, fresh, rowpar, lme);
            else if (deg == 22) st = sw_layer_step<METHOD, 22>(lds, tab, p, K, (uint32_t)lane, deg, cur, fresh, rowpar, lme);
            else st = sw_layer_step<METHOD, 0>(lds, tab, p, K, (uint32_t)lane, deg, cur, fresh, rowpar, lme);
            /* the six indexed writes back to back, nothing scheduled between them: ONE s_set_gpr_idx_on / _off pair around all of
             * them instead of one per write */
            __builtin_amdgcn_sched_barrier(0);
            regs_put(R, br, st);
            __builtin_amdgcn_sched_barrier(0);
            tabv = tabn;
        }
        return;
    }
    SwRow cur = zero;
    if (!fresh) cur = rows[lane];
    uint32_t tabv = gc->sbplain[0][lane & 31];
    /* Nothing may be in flight when the layer loop is entered: the compiler merges the counter state of this path into the
     * loop header, and with loads pending here it waits in front of every layer as if they still were - in steady state that
     * is a wait for the row store issued a few instructions earlier (a memory round trip per layer). */
    __builtin_amdgcn_s_waitcnt(0x0f70); /* vmcnt(0) */
    for (int br = 0; br < nbr; ++br) {
        /* next layer's messages and edge table: issued a whole layer ahead of their use; always a valid address (the last
         * layer re-reads layer 0, the first iteration reads what it is about to overwrite and ignores it) */
        const int brn = br + 1 < nbr ? br + 1 : 0;
        const SwRow nxt = rows[brn * LF_T4 + lane];
        const uint32_t tabn = gc->sbplain[brn][lane & 31];
        const int deg = c->deg[br]; /* (a bit mask over the layers instead of this scalar load was measured: 1 % slower) */
        uint32_t rowpar = 0;
        if (have_par) { /* syndrome bits of rows lane + 64 k of this layer as byte masks */
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t wv = sP[br * 8 + 2 * k + (lane >> 5)];
                rowpar |= ((wv >> (lane & 31)) & 1u) ? (0xffu << (8 * k)) : 0u;
            }
        }
        DevTab4 tab;
        tab.c = c; tab.br = br; tab.sbv = tabv;
        SwRow st;
        const uint32_t era_edges = ERA ? c->era_edges[br] : 0u;
        if (ERA) st = sw_layer_step<METHOD, 0, ERA>(lds, tab, p, K, (uint32_t)lane, deg, cur, fresh, rowpar, lme, era_edges, era_plane); /* rare: one instance */
        else if (deg == 23) st = sw_layer_step<METHOD, 23>(lds, tab, p, K, (uint32_t)lane, deg, cur, fresh, rowpar, lme);
        else if (deg == 22) st = sw_layer_step<METHOD, 22>(lds, tab, p, K, (uint32_t)lane, deg, cur, fresh, rowpar, lme);
        else st = sw_layer_step<METHOD, 0>(lds, tab, p, K, (uint32_t)lane, deg, cur, fresh, rowpar, lme);
        /* take the prefetched data BEFORE the store is issued: vector-memory operations retire in order, so a wait for these
         * loads placed after the store would also wait for the store's round trip, once per layer */
        cur = fresh ? zero : nxt;
        tabv = tabn;
        asm volatile("" : "+v"(cur.x[0]), "+v"(cur.x[1]), "+v"(cur.x[2]), "+v"(cur.cw), "+v"(cur.pa[0]), "+v"(cur.pa[1]), "+v"(tabv));
        __builtin_amdgcn_sched_barrier(0);
        if (rem > 0) rows[br * LF_T4 + lane] = st; /* the last layered iteration's messages are never read again */
    }
}

/* messages of a parking / resuming codeword between the registers and its slot in HBM (RM instances): every layer's transfer
 * in flight together (layers beyond the last one repeat it: no branches between the loads) */
__device__ __forceinline__ void regs_store(const SwRegs& R, SwRow* __restrict__ rows, int nbr, int lane)
{
#pragma unroll
    for (int br = 0; br < LF4_RM_LAYERS; ++br)
        if (br < nbr) rows[br * LF_T4 + lane] = regs_get(R, br);
}
__device__ __forceinline__ void regs_load(SwRegs& R, const SwRow* __restrict__ rows, int nbr, int lane)
{
    SwRow r[LF4_RM_LAYERS];
#pragma unroll
    for (int br = 0; br < LF4_RM_LAYERS; ++br) r[br] = rows[(br < nbr ? br : nbr - 1) * LF_T4 + lane];
#pragma unroll
    for (int br = 0; br < LF4_RM_LAYERS; ++br) regs_put(R, br, r[br]);
}
__device__ __forceinline__ void regs_clear(SwRegs& R)
{
    const lf4_vec z = (lf4_vec)(0u);
    R.x0 = z; R.x1 = z; R.x2 = z; R.cw = z; R.pa0 = z; R.pa1 = z;
}

/* ---- the decode loops, written once for both kernels as macros over the kernel's own locals (a forced-inline function is
 * optimised on its own before it is inlined, and the group kernel's code then comes out different; expanded in place, it is the
 * same code).  They expect in scope: a (.fix_input, .code), c, f, N, M, K, nw, tid, g, lane_in_group, g_rows, R, sHard, sHard0,
 * sHard2, sP, sRed, ls, prog, in_bf, parked, pA, pB, t_bf0, t_end, max_iter, max_bf, and the kernel's rule as four hooks:
 *   LF4_ON_FRONT          the codeword is on its group's front (only then does the syndrome stage decide anything)
 *   LF4_CLEAN_STOPS(t)    after a clean syndrome: whether the codeword stops (parks) here
 *   LF4_ON_STOP(t)        statement run when it does, in the layered stage
 *   LF4_ON_PASS(t)        statement run when it passes a decision point
 * LF4_STAGE_INPUT: the codeword's LLRs from the reference's fixInput layout into the interleaved En image (the LDS);
 * LF4_LAYERED_LOOP: the layered iterations from decision point prog on; LF4_ENTER_BF: the bit-flipping stage's entry when the
 * layered loop ran out; LF4_BF_LOOPS: the bit-flipping iterations.  parked = true when the codeword stopped clean at prog.
 * LF4_MAIN_STEP: the layered iteration the loop runs, main_step4 unless the including file names its own (lnsfaid_kernel4z.hip).
 * LF4_DIRTY_CHECK(c, lane): the cheap "certainly dirty" test in front of the syndrome stage, layer0_dirty4 unless the including
 * file names its own (lnsfaid_kernel4s.hip: on compile-time tables; lnsfaid_kernel4.hip: layer0_dirty4_edgewise). ---- */
#ifndef LF4_MAIN_STEP
#define LF4_MAIN_STEP main_step4
#endif
#ifndef LF4_DIRTY_CHECK
#define LF4_DIRTY_CHECK(c, lane) layer0_dirty4(c, lane)
#endif
#define LF4_STAGE_INPUT() \
        /* input staging (CDecoder_FAID.cpp:217-255): lane l of group g is information row l of the [32][K] block followed by                             \
         * parity row l of the [32][M] block; punctured tail erased; interleaved and biased for the layer step */                                         \
        const int8_t* gi = a.fix_input + (size_t)g * (size_t)LNSFAID_GROUP * (size_t)N;                                                                   \
        const int8_t* src_i = gi + (size_t)lane_in_group * (size_t)K;                                                                                     \
        const int8_t* src_p = gi + (size_t)LNSFAID_GROUP * (size_t)K + (size_t)lane_in_group * (size_t)M;                                                 \
        const int first_erased = N - c->puncture_tail;                                                                                                    \
        const int nbc = c->nbc;                                                                                                                           \
        if ((((size_t)a.fix_input) & 3u) == 0u) {                                                                                                         \
            /* K, M and N are multiples of Z = 256: a block column is 64 aligned dwords of one of the two rows.  Lane d loads                             \
             * dword d (variable nodes 4 d .. 4 d + 3) of LF_STAGE_COLS columns at a time, all loads in flight together, and                              \
             * scatters the four bytes to their places in the interleaved image (node n: dword n mod 64, byte n div 64). */                               \
            constexpr int SB = 23;                                                                                                                        \
            const uint32_t base_d = ((16u * (uint32_t)tid) & 0xffu) + ((uint32_t)tid >> 4);                                                               \
            const SwLds lds = SwLds();                                                                                                                    \
            for (int cb0 = 0; cb0 < nbc; cb0 += SB) {                                                                                                     \
                uint32_t w[SB];                                                                                                                           \
_Pragma("unroll")                                                                                                                                         \
                for (int u = 0; u < SB; ++u) {                                                                                                            \
                    const int cb = cb0 + u;                                                                                                               \
                    if (cb < nbc) { /* uniform */                                                                                                         \
                        const int8_t* col = cb * LF_Z < K ? src_i + cb * LF_Z : src_p + (cb * LF_Z - K);                                                  \
                        w[u] = ((const uint32_t*)col)[tid];                                                                                               \
                    }                                                                                                                                     \
                }                                                                                                                                         \
_Pragma("unroll")                                                                                                                                         \
                for (int u = 0; u < SB; ++u) {                                                                                                            \
                    const int cb = cb0 + u;                                                                                                               \
                    if (cb < nbc) {                                                                                                                       \
                        uint32_t x = w[u];                                                                                                                \
                        const int lim = first_erased - cb * LF_Z; /* nodes of this column from lim on are erased */                                       \
                        if (lim < LF_Z) {                                                                                                                 \
_Pragma("unroll")                                                                                                                                         \
                            for (int k = 0; k < 4; ++k) if (4 * tid + k >= lim) x &= ~(0xffu << (8 * k));                                                 \
                        }                                                                                                                                 \
                        x = ((x & 0x7f7f7f7fu) + (uint32_t)SW_BIAS_EN * 0x01010101u) ^ (x & 0x80808080u); /* + SW_BIAS_EN (< 128) per byte, no carries */ \
                        const uint32_t ad = (uint32_t)cb * 256u + base_d;                                                                                 \
                        lds.wr8(ad, x); lds.wr8(ad + 4u, x >> 8); lds.wr8(ad + 8u, x >> 16); lds.wr8(ad + 12u, x >> 24);                                  \
                    }                                                                                                                                     \
                }                                                                                                                                         \
            }                                                                                                                                             \
        } else {                                                                                                                                          \
            for (int cb = 0; cb < nbc; ++cb) { /* caller's buffer not dword aligned: byte loads */                                                        \
                uint32_t w = 0;                                                                                                                           \
_Pragma("unroll")                                                                                                                                         \
                for (int k = 0; k < 4; ++k) {                                                                                                             \
                    const int v = cb * LF_Z + tid + 64 * k;                                                                                               \
                    int x = v < K ? src_i[v] : src_p[v - K];                                                                                              \
                    if (v >= first_erased) x = 0;                                                                                                         \
                    w |= (uint32_t)((x + SW_BIAS_EN) & 0xff) << (8 * k);                                                                                  \
                }                                                                                                                                         \
                lds4_wr((uint32_t)cb * 256u + 4u * (uint32_t)tid, w);                                                                                     \
            }                                                                                                                                             \
        }                                                                                                                                                 \
    /* end of LF4_STAGE_INPUT */

#define LF4_LAYERED_LOOP() \
        while (prog < t_end && !(max_bf > 0 && prog >= t_bf0)) {                                                                                                                                         \
            /* the lane number as this iteration sees it: opaque, so that the per-lane addresses and masks of the syndrome stage and                                                                     \
             * the plane build are recomputed per iteration (a few dozen operations) instead of being hoisted out of the loop and                                                                        \
             * kept alive - spilled, with the messages in registers - through every layer */                                                                                                             \
            int tid_i = tid;                                                                                                                                                                             \
            asm volatile("" : "+v"(tid_i));                                                                                                                                                              \
            if (METHOD == 0) { /* CLDPC::Decode has no syndrome stage and no early stop (CLDPC.cpp:287-2283) */                                                                                          \
                LF4_MAIN_STEP<METHOD, false, RM>(c, f, a.code, g_rows, R, tid_i, prog, sP, false, false, 0u);                                                                                            \
                prog++;                                                                                                                                                                                  \
                continue;                                                                                                                                                                                \
            }                                                                                                                                                                                            \
            bool lme = false, have_par = false;                                                                                                                                                          \
            /* l_checksum_ and the unsatisfied count are consumed only inside the error-floor window                                                                                                     \
             * (nombre_iterations <= floor_iter_thresh: OMS selective offset CDecoder_OMS.cpp:388, 2B1C tables                                                                                           \
             * CDecoder_FAID.cpp:714) and never by DecodeMethod 2; elsewhere only unsat != 0 matters */                                                                                                  \
            const bool needs_checksums = max_iter - prog <= f->floor_iter_thresh; /* never for the shipped DecodeMethod 2: -1 */                                                                         \
            /* behind the group's front (the snapshot shows a lane parked beyond this point) the group is known to go on, and                                                                            \
             * outside the window nothing else reads the syndrome: a catching-up codeword skips the stage altogether */                                                                                  \
            const bool must_know = needs_checksums || LF4_ON_FRONT;                                                                                                                                      \
            if (must_know && (needs_checksums || !LF4_DIRTY_CHECK(c, tid_i))) {                                                                                                                          \
                build_plane4<false>(c, sHard, 0, tid_i);                                                                                                                                                 \
                int unsat;                                                                                                                                                                               \
                if (RM || syn_cache_fits(c->nbr)) { /* (RM: a code of up to LF4_RM_LAYERS layers always fits) all table entries of the walk loaded together: one memory round trip, not one per round */ \
                    SynCache sc;                                                                                                                                                                         \
                    syn_cache_load(a.code, c->nbr, tid_i, sc);                                                                                                                                           \
                    unsat = syndrome<LF_T4, false, true>(c, a.code, sP, tid_i, pA, pB, sRed, &sc);                                                                                                       \
                } else {                                                                                                                                                                                 \
                    unsat = syndrome<LF_T4, false>(c, a.code, sP, tid_i, pA, pB, sRed);                                                                                                                  \
                }                                                                                                                                                                                        \
                /* clean on the group's front: park, unless a group mate is known to have passed this point */                                                                                           \
                if (unsat == 0 && LF4_CLEAN_STOPS(tid_i)) {                                                                                                                                              \
                    /* the messages leave the registers here, not in the common epilogue: there the compiler would have to keep                                                                          \
                     * them alive through the whole bit-flipping stage */                                                                                                                                \
                    LF4_ON_STOP(tid_i)                                                                                                                                                                   \
                    parked = true;                                                                                                                                                                       \
                    break;                                                                                                                                                                               \
                }                                                                                                                                                                                        \
                if (LF4_OMS(METHOD)) lme = imin(unsat, 255) < (int)(uint8_t)f->floor_err_count; /* CDecoder_OMS.cpp:328 */                                                                               \
                else lme = imin(unsat, 127) < (int)(int8_t)f->floor_err_count;              /* CDecoder_FAID.cpp:619 */                                                                                  \
                have_par = true;                                                                                                                                                                         \
            }                                                                                                                                                                                            \
            LF4_ON_PASS(tid_i)                                                                                                                                                                           \
            if (EF2 && f->ef == 2 && needs_checksums && have_par && lme) {                                                                                                                               \
                /* EF_ELIMINATION 2 inside the window, few unsatisfied checks: this iteration erases (CDecoder_FAID.cpp:673-680) */                                                                      \
                build_erasure_plane4(c, a.code, sHard, sP, f->W, tid_i);                                                                                                                                 \
                LF4_MAIN_STEP<METHOD, EF2, RM>(c, f, a.code, g_rows, R, tid_i, prog, sP, true, lme, lf_lds_off_hard(N));                                                                                 \
            } else {                                                                                                                                                                                     \
                LF4_MAIN_STEP<METHOD, false, RM>(c, f, a.code, g_rows, R, tid_i, prog, sP, have_par && needs_checksums, lme, 0u);                                                                        \
            }                                                                                                                                                                                            \
            prog++;                                                                                                                                                                                      \
        }                                                                                                                                                                                                \
    /* end of LF4_LAYERED_LOOP */

#define LF4_ENTER_BF() \
        if (!parked && prog < t_end) {                                                                                          \
            /* the layered loop ran out: enter the bit-flipping stage (CDecoder_FAID.cpp:6411-6428) */                          \
            uint32_t conf[LF_MAX_BC * 8 / LF_T4]; /* this lane's share of the 2B1C confidence plane */                          \
            if (METHOD == 5) {                                                                                                  \
                build_plane4<true>(c, sHard, f->hard2_thr, tid); /* staged where the hard plane will go */                      \
_Pragma("unroll")                                                                                                               \
                for (int k = 0; k < LF_MAX_BC * 8 / LF_T4; ++k) conf[k] = (tid + k * LF_T4 < nw) ? sHard[tid + k * LF_T4] : 0u; \
                LF_WG_SYNC();                                                                                                   \
            }                                                                                                                   \
            build_plane4<false>(c, sHard, 0, tid);                                                                              \
            /* En is dead from here on: its bytes take hard_ch (= hard) and hard2 */                                            \
            copy_out<9>(sHard0, sHard, nw, tid);                                                                                \
            if (METHOD == 5) {                                                                                                  \
_Pragma("unroll")                                                                                                               \
                for (int k = 0; k < LF_MAX_BC * 8 / LF_T4; ++k) if (tid + k * LF_T4 < nw) sHard2[tid + k * LF_T4] = conf[k];    \
            }                                                                                                                   \
            ls.Th = (int8_t)f->W; ls.l0 = 0; ls.l1 = 0; ls.t = 1;                                                               \
            in_bf = true;                                                                                                       \
            LF_WG_SYNC();                                                                                                       \
        }                                                                                                                       \
    /* end of LF4_ENTER_BF */

#define LF4_BF_LOOPS() \
    if (in_bf && !parked) {                                                                                                                 \
        if (METHOD != 3 && (RM || syn_cache_fits(c->nbr)) && bf_stage_fits(c, f)) {                                                         \
            /* the stage's constants out of its iterations (lnsfaid_phases.h BfStage) */                                                    \
            BfStage bs;                                                                                                                     \
            bf_stage_load(c, f, a.code, tid, bs);                                                                                           \
            while (prog < t_end) {                                                                                                          \
                const int unsat = syndrome_staged(sP, tid, sRed, bs);                                                                       \
                if (unsat == 0 && LF4_CLEAN_STOPS(tid)) { parked = true; break; }                                                           \
                LF4_ON_PASS(tid)                                                                                                            \
                bf_step_staged<METHOD>(tid, ls, sRed, bs);                                                                                  \
                prog++;                                                                                                                     \
            }                                                                                                                               \
        } else if (METHOD == 3 && (RM || syn_cache_fits(c->nbr))) {                                                                         \
            /* the plain flip may change every column: the full walk, its table entries in registers */                                     \
            SynCache sc;                                                                                                                    \
            syn_cache_load(a.code, c->nbr, tid, sc);                                                                                        \
            while (prog < t_end) {                                                                                                          \
                const int unsat = syndrome<LF_T4, false, true>(c, a.code, sP, tid, pA, pB, sRed, &sc);                                      \
                if (unsat == 0 && LF4_CLEAN_STOPS(tid)) { parked = true; break; }                                                           \
                LF4_ON_PASS(tid)                                                                                                            \
                bf_step_plain<LF_T4>(c, f, a.code, sHard, sHard2 + nw /* 4 count planes in the dead En */, sP, tid, sRed);                  \
                prog++;                                                                                                                     \
            }                                                                                                                               \
        } else {                                                                                                                            \
            while (prog < t_end) {                                                                                                          \
                const int unsat = syndrome<LF_T4, false>(c, a.code, sP, tid, pA, pB, sRed);                                                 \
                if (unsat == 0 && LF4_CLEAN_STOPS(tid)) { parked = true; break; }                                                           \
                LF4_ON_PASS(tid)                                                                                                            \
                if (METHOD == 3) bf_step_plain<LF_T4>(c, f, a.code, sHard, sHard2 + nw /* 4 count planes in the dead En */, sP, tid, sRed); \
                else bf_step<LF_T4, METHOD>(c, f, a.code, sHard, sHard0, sHard2, sP, tid, ls, sRed);                                        \
                prog++;                                                                                                                     \
            }                                                                                                                               \
        }                                                                                                                                   \
    }                                                                                                                                       \
    /* end of LF4_BF_LOOPS */

#endif /* LNSFAID_ROWS4_H */
