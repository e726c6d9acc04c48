/*
 * lnsfaid_frame4.h - the kernel frames of the one-wave, four-rows-per-lane decoders, written once (gfx950).
 *
 * Every such decoder is the loop text of lnsfaid_rows4.h (LF4_LAYERED_LOOP, LF4_ENTER_BF, LF4_BF_LOOPS) inside one of two frames:
 *   LF4_GROUP_FRAME   the group-of-32 protocol of DESIGN.md 3.3: status snapshot, early exits, state on chip, loops, finish or park
 *                     (lnsfaid_kernel4.hip, its packed twin in lnsfaid_kernel4p.hip, lnsfaid_kernel4z / 4s / 4w.hip);
 *   LF4_CW_CORE       the per-codeword rule of DESIGN.md 3.3b: stage, loops, the hard-decision plane and the unsatisfied checks
 *                     (lnsfaid_kernel4cw.hip, its packed twin, the line decoders of lnsfaid_kernel4l / 4b.hip).
 * The frames are macro text over the kernel's own locals for the reason the loops are (lnsfaid_rows4.h: a forced-inline function is
 * optimised on its own before it is inlined, and the register allocation of a whole kernel follows the shape of the code around
 * its loops - lnsfaid_kernel4p.hip has a measured case).  A kernel is its signature, whatever it does to its arguments in front of
 * the frame, the frame, and - under the per-codeword rule - its own output and records behind it.
 *
 * The rule's four hooks of the loop text are chosen by name: the including file defines LF4_RULE as GROUP or CW in front of a
 * kernel (lnsfaid_kernel4p.hip holds one kernel of either rule and redefines it in between).
 */
#ifndef LNSFAID_FRAME4_H
#define LNSFAID_FRAME4_H

#include "lnsfaid_rows4.h"

/* ---- the hooks (lnsfaid_rows4.h says where the loops call them) ---- */
#define LF4_PASTE_(a, b) a##b
#define LF4_PASTE(a, b) LF4_PASTE_(a, b)
#define LF4_ON_FRONT LF4_PASTE(LF4_ON_FRONT_, LF4_RULE)
#define LF4_CLEAN_STOPS(t) LF4_PASTE(LF4_CLEAN_STOPS_, LF4_RULE)(t)
#define LF4_ON_STOP(t) LF4_PASTE(LF4_ON_STOP_, LF4_RULE)(t)
#define LF4_ON_PASS(t) LF4_PASTE(LF4_ON_PASS_, LF4_RULE)(t)
/* what a clean syndrome does under the group rule: a codeword on the group's front parks, unless a group mate is known to have
 * passed the point; one behind it is known to go on */
#define LF4_ON_FRONT_GROUP prog >= kmax
#define LF4_CLEAN_STOPS_GROUP(t) prog >= kmax && !group_passed(a.live, g, prog, t)
#define LF4_ON_STOP_GROUP(t) if (RM && prog >= 2) regs_store(R, g_rows, c->nbr, t); /* the messages leave the registers where it parks */
#define LF4_ON_PASS_GROUP(t) publish_pass(a.live, cw, prog, t);
/* under the per-codeword rule: the codeword stops there; a codeword is always on its own front */
#define LF4_ON_FRONT_CW true
#define LF4_CLEAN_STOPS_CW(t) true
#define LF4_ON_STOP_CW(t)
#define LF4_ON_PASS_CW(t)

/* ---- what both frames start with: the kernel's view of its arguments (a.code, a.cfg) and of the LDS ---- */
#define LF4_LOCALS()                                                                                                            \
    extern __shared__ __align__(16) unsigned char smem[];                                                                       \
    CCode c = (CCode)a.code;                                                                                                    \
    CCfg f = (CCfg)a.cfg;                                                                                                       \
    const int tid = (int)threadIdx.x;                                                                                           \
    const int cw = (int)blockIdx.x;                                                                                             \
    const int N = c->n_var, M = c->n_check, K = c->k_info, nw = c->n_words, pw = c->p_words;                                    \
    (void)M; /* (the staging of the group layout only) */                                                                       \
    /* (the layer step addresses En by its LDS offset: the dynamic segment must start at 0, i.e. the kernel must have no static \
     * LDS - checked on the host when a context picks its kernel, lnsfaid_capi.hip kernel_check) */                             \
    uint32_t* sHard0 = (uint32_t*)smem;      /* bit-flipping stage: hard_ch and hard2 overlay the dead En */                    \
    uint32_t* sHard2 = (uint32_t*)smem + nw;                                                                                    \
    uint32_t* sHard = (uint32_t*)(smem + lf_lds_off_hard(N));                                                                   \
    uint32_t* sP = (uint32_t*)(smem + lf_lds_off_p(N, nw));                                                                     \
    int* sStat = (int*)(smem + lf_lds_off_stat(N, nw, pw));                                                                     \
    int* sRed = sStat + LNSFAID_GROUP;                                                                                          \
                                                                                                                                \
    const int max_iter = f->max_iter, max_bf = f->max_bf;                                                                       \
    const int t_bf0 = max_iter + 1;   /* first bit-flipping decision point */                                                   \
    const int t_end = t_bf0 + max_bf; /* both loops exhausted               */                                                  \
    /* end of LF4_LOCALS */

/* the group's record when it stops at decision point prog */
#define LF4_GROUP_RECORD()                                              \
            if (a.stats && lane_in_group == 0) {                        \
                lnsfaid_group_stats st;                                 \
                st.iterations = prog <= max_iter ? prog - 1 : max_iter; \
                st.bf_iterations = prog <= max_iter ? 0 : prog - t_bf0; \
                a.stats[g] = st;                                        \
            }                                                           \
    /* end of LF4_GROUP_RECORD */

/* ---- the group-rule kernel, from an `a` of LfKernelArgs on: one wave per codeword.
 * STAGE: the staging text of a fresh codeword (LF4_STAGE_INPUT, LF4P_STAGE_INPUT); WRITE(sHard, g_out, N, tid): the writer of the
 * hard decisions, onto OUT_T* a.decoded with OUT_STRIDE elements per codeword (write_decoded, int8_t, N / write_bits, uint32_t, nw) */
#define LF4_GROUP_FRAME(STAGE, WRITE, OUT_T, OUT_STRIDE)                                                                                      \
    LF4_LOCALS()                                                                                                                              \
                                                                                                                                              \
    /* snapshot of the 32 lanes of this group: one load per lane (both halves of the wave hold the same 32 words), everything                 \
     * else in registers - no LDS round trips in front of the early exits, which most workgroups of a relaunch take */                        \
    const int g = cw >> 5, lane_in_group = cw & 31;                                                                                           \
    const int sv = a.status_cur ? a.status_cur[g * LNSFAID_GROUP + (tid & 31)] : 0; /* null: first launch of a batch, every codeword fresh */ \
    const int my_status = __builtin_amdgcn_readlane(sv, lane_in_group);                                                                       \
    if (my_status & LF_DONE) { /* uniform exit */                                                                                             \
        if (tid == 0) a.status_next[cw] = my_status;                                                                                          \
        return;                                                                                                                               \
    }                                                                                                                                         \
    if (tid == LNSFAID_GROUP) sRed[LF_ZERO_SLOT] = 0; /* the word unused synw slots point at */                                               \
    int kmax;                                                                                                                                 \
    {                                                                                                                                         \
        int v = sv & LF_PROG_MASK; /* maximum over lanes 0..31, same DPP pattern as add_reduce32 (values are not negative) */                 \
        v = imax(v, __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false));                                                               \
        v = imax(v, __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false));                                                               \
        v = imax(v, __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false));                                                               \
        v = imax(v, __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false));                                                               \
        v = imax(v, __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false));                                                               \
        kmax = __builtin_amdgcn_readlane(v, 31);                                                                                              \
    }                                                                                                                                         \
    const int all_same = __ballot(sv != my_status) == 0ull;                                                                                   \
    LF_WG_SYNC();                                                                                                                             \
    int prog = my_status & LF_PROG_MASK;                                                                                                      \
                                                                                                                                              \
    uint32_t* g_en = (uint32_t*)(a.st_en + (size_t)cw * (size_t)N);                                                                           \
    SwRow* g_rows = (SwRow*)(a.st_rows + (size_t)cw * (size_t)(c->nbr * LF_T)); /* the 2-row kernel's slot: 16 B x 128 >= 24 B x 64 */        \
    uint32_t* g_bits = a.st_bits + (size_t)cw * (size_t)(3 * nw);                                                                             \
    OUT_T* g_out = (OUT_T*)a.decoded + (size_t)cw * (size_t)(OUT_STRIDE);                                                                     \
                                                                                                                                              \
    /* parked on the group's front, not everybody there yet: nothing to do in this launch */                                                  \
    if (prog != 0 && prog == kmax && !all_same) {                                                                                             \
        if (tid == 0) { a.status_next[cw] = my_status; atomicAdd(a.remaining, 1u); }                                                          \
        return;                                                                                                                               \
    }                                                                                                                                         \
                                                                                                                                              \
    /* all 32 lanes parked clean at the same decision point: the group stops there (the reference's break).  Every lane                       \
     * wrote its hard decisions when it parked, so nothing is left to do but to say so. */                                                    \
    if (my_status != 0 && all_same) {                                                                                                         \
        if (tid == 0) {                                                                                                                       \
            a.status_next[cw] = my_status | LF_DONE;                                                                                          \
            LF4_GROUP_RECORD()                                                                                                                \
        }                                                                                                                                     \
        return;                                                                                                                               \
    }                                                                                                                                         \
                                                                                                                                              \
    bool in_bf = max_bf > 0 && prog >= t_bf0 && prog != 0;                                                                                    \
    LfLaneState ls = { 0, 0, 0, 0 };                                                                                                          \
    SwRegs R; /* RM: the codeword's compressed messages (dead in the bit-flipping stage) */                                                   \
    if (RM) regs_clear(R);                                                                                                                    \
                                                                                                                                              \
    /* ---- bring the codeword's state on chip ---- */                                                                                        \
    if (prog == 0) {                                                                                                                          \
        STAGE()                                                                                                                               \
        LF_WG_SYNC();                                                                                                                         \
        prog = 1;                                                                                                                             \
    } else if (!in_bf) {                                                                                                                      \
        copy_in<23>((uint32_t*)smem, g_en, N >> 2, tid);                                                                                      \
        if (RM && prog >= 2) regs_load(R, g_rows, c->nbr, tid); /* parked in front of iteration 1: every Lmn is still 0 */                    \
        LF_WG_SYNC();                                                                                                                         \
    } else {                                                                                                                                  \
        copy_in<9>(sHard, g_bits, nw, tid);                                                                                                   \
        copy_in<9>(sHard0, g_bits + nw, nw, tid);                                                                                             \
        copy_in<9>(sHard2, g_bits + 2 * nw, nw, tid);                                                                                         \
        ls = a.st_lane[cw];                                                                                                                   \
        LF_WG_SYNC();                                                                                                                         \
    }                                                                                                                                         \
                                                                                                                                              \
    bool parked = false;                                                                                                                      \
    uint32_t pA = 0, pB = 0;                                                                                                                  \
    /* ---- layered iterations (the syndrome stage in front of iteration prog is decision point prog) ---- */                                 \
    if (!in_bf) {                                                                                                                             \
        LF4_LAYERED_LOOP()                                                                                                                    \
        LF4_ENTER_BF()                                                                                                                        \
    }                                                                                                                                         \
    /* ---- bit-flipping iterations.  Nothing of the layer step is alive here, so the lanes keep their entries of the walk                    \
     * tables in registers for the whole stage (no table load, hence no exposed memory latency, per iteration) ---- */                        \
    LF4_BF_LOOPS()                                                                                                                            \
                                                                                                                                              \
    const bool finished = prog >= t_end;                                                                                                      \
    if (finished) {                                                                                                                           \
        if (!in_bf) build_plane4<false>(c, sHard, 0, tid);                                                                                    \
        WRITE(sHard, g_out, N, tid);                                                                                                          \
        if (tid == 0) {                                                                                                                       \
            a.status_next[cw] = prog | LF_DONE;                                                                                               \
            LF4_GROUP_RECORD()                                                                                                                \
        }                                                                                                                                     \
    } else {                                                                                                                                  \
        /* park clean at decision point prog: state back to HBM for the case that the group goes on, and the hard decisions                   \
         * (the syndrome stage has just built the plane from this En; in the bit-flipping stage the plane is the state) as the                \
         * output for the case that it stops here */                                                                                          \
        if (!in_bf) {                                                                                                                         \
            copy_out<23>(g_en, (const uint32_t*)smem, N >> 2, tid); /* (RM: the messages were stored where the codeword parked) */            \
        } else {                                                                                                                              \
            copy_out<9>(g_bits, sHard, nw, tid);                                                                                              \
            copy_out<9>(g_bits + nw, sHard0, nw, tid);                                                                                        \
            copy_out<9>(g_bits + 2 * nw, sHard2, nw, tid);                                                                                    \
            if (tid == 0) a.st_lane[cw] = ls;                                                                                                 \
        }                                                                                                                                     \
        WRITE(sHard, g_out, N, tid);                                                                                                          \
        if (tid == 0) { a.status_next[cw] = prog; atomicAdd(a.remaining, 1u); }                                                               \
    }                                                                                                                                         \
    /* end of LF4_GROUP_FRAME */

/* the two pointers the decode loop uses, split off the kernel arguments a_ into the frame's `a` (the layer-static kernels): the
 * compiler holds the arguments as ONE tuple of sixteen registers, spilled and reloaded whole wherever a field of it is wanted
 * (twice inside layer 0).  An opaque zero is added instead of constraining the pointers themselves, which would lose their
 * address space (flat loads in every layer). */
#define LF4_SPLIT_ARGS()                                       \
    LfKernelArgs a = a_;                                       \
    {                                                          \
        uint32_t z = 0u;                                       \
        asm volatile("" : "+s"(z));                            \
        a.code = (const LfDevCode*)((const char*)a_.code + z); \
        a.cfg = (const LfDevCfg*)((const char*)a_.cfg + z);    \
    }                                                          \
    /* end of LF4_SPLIT_ARGS */

/* ---- the per-codeword decode, behind LF4_LOCALS and whatever the kernel needs in front (the group layout's g and lane_in_group,
 * the combiner's skip): one launch, no state in HBM but the streamed messages.  Leaves behind: prog, the decision point the
 * codeword stopped at; sHard, its hard decisions - the plane the last syndrome stage checked (clean), the bit-flipping state, or
 * the plane of the final En; unsat, the unsatisfied checks of that plane where WANT_UNSAT asks for them; and the staging's locals.
 * STAGE: the staging text (LF4_STAGE_INPUT, LF4P_STAGE_INPUT, LF4L_STAGE_INPUT, LF4B_STAGE_INPUT) */
#define LF4_CW_CORE(STAGE, WANT_UNSAT)                                                                                 \
    if (tid == LNSFAID_GROUP) sRed[LF_ZERO_SLOT] = 0; /* the word unused synw slots point at */                        \
                                                                                                                       \
    SwRow* g_rows = (SwRow*)(a.st_rows + (size_t)cw * (size_t)(c->nbr * LF_T)); /* !RM: the messages between layers */ \
    LfLaneState ls = { 0, 0, 0, 0 };                                                                                   \
    SwRegs R; /* RM: the codeword's compressed messages (dead in the bit-flipping stage) */                            \
    if (RM) regs_clear(R);                                                                                             \
                                                                                                                       \
    STAGE()                                                                                                            \
    LF_WG_SYNC();                                                                                                      \
    int prog = 1;                                                                                                      \
    bool in_bf = false;                                                                                                \
    bool parked = false; /* under this rule: stopped clean at decision point prog */                                   \
    uint32_t pA = 0, pB = 0;                                                                                           \
    /* ---- layered iterations, then the bit-flipping stage ---- */                                                    \
    {                                                                                                                  \
        LF4_LAYERED_LOOP()                                                                                             \
        LF4_ENTER_BF()                                                                                                 \
    }                                                                                                                  \
    LF4_BF_LOOPS()                                                                                                     \
    const bool clean = parked;                                                                                         \
                                                                                                                       \
    if (!clean && !in_bf) build_plane4<false>(c, sHard, 0, tid);                                                       \
    int unsat = 0;                                                                                                     \
    if (!clean && (WANT_UNSAT)) { /* ran out of iterations: one syndrome pass of the output plane */                   \
        if (RM || syn_cache_fits(c->nbr)) {                                                                            \
            SynCache sc;                                                                                               \
            syn_cache_load(a.code, c->nbr, tid, sc);                                                                   \
            unsat = syndrome<LF_T4, false, true>(c, a.code, sP, tid, pA, pB, sRed, &sc);                               \
        } else {                                                                                                       \
            unsat = syndrome<LF_T4, false>(c, a.code, sP, tid, pA, pB, sRed);                                          \
        }                                                                                                              \
    }                                                                                                                  \
    /* end of LF4_CW_CORE */

/* the codeword's and the group's records under the per-codeword rule (LfCwArgs) */
#define LF4_CW_RECORDS()                                                                                               \
    if (tid == 0) {                                                                                                    \
        const int it = prog <= max_iter ? prog - 1 : max_iter;                                                         \
        const int bf = prog <= max_iter ? 0 : prog - t_bf0;                                                            \
        if (a.cw_stats) {                                                                                              \
            lnsfaid_codeword_stats st;                                                                                 \
            st.iterations = it; st.bf_iterations = bf; st.unsatisfied = unsat;                                         \
            a.cw_stats[cw] = st;                                                                                       \
        }                                                                                                              \
        if (a.stats) { /* the group's record: maxima over its codewords (zeroed by the host in front of the launch) */ \
            atomicMax(&a.stats[g].iterations, it);                                                                     \
            atomicMax(&a.stats[g].bf_iterations, bf);                                                                  \
        }                                                                                                              \
    }                                                                                                                  \
    /* end of LF4_CW_RECORDS */

/* ---- the instance a configuration runs on (for hipFuncGetAttributes / the occupancy query, and for the launch), as the body of
 * a function of (method, ef, rm).  Messages in registers (RM) for codes of up to LF4_RM_LAYERS layers, streamed through HBM
 * otherwise; the erasing layer step of EF_ELIMINATION 2 (Decode_FAID only) lives in an instance of its own, so that the common
 * ones do not carry its registers; DecodeMethod 0 has the streaming instance only (16-level search: with the messages in
 * registers too the layer step spills). ---- */
#define LF4_INSTANCE_CASE(KERNEL, M) case M: return rm ? (const void*)KERNEL<M, true, false> : (const void*)KERNEL<M, false, false>;
#define LF4_INSTANCE_TABLE(KERNEL)                                                                                                                       \
    if (method == 2 && ef == 2) return (const void*)KERNEL<2, false, true>;                                                                              \
    switch (method) {                                                                                                                                    \
    case 0: return (const void*)KERNEL<0, false, false>;                                                                                                 \
        LF4_INSTANCE_CASE(KERNEL, 1) LF4_INSTANCE_CASE(KERNEL, 2) LF4_INSTANCE_CASE(KERNEL, 3) LF4_INSTANCE_CASE(KERNEL, 4) LF4_INSTANCE_CASE(KERNEL, 5) \
    default: return nullptr;                                                                                                                             \
    }
/* the kernels built for <METHOD> alone (messages in registers, DecodeMethods 1..5), as the body of a function of (method) */
#define LF4_METHOD_TABLE(KERNEL)           \
    switch (method) {                      \
    case 1: return (const void*)KERNEL<1>; \
    case 2: return (const void*)KERNEL<2>; \
    case 3: return (const void*)KERNEL<3>; \
    case 4: return (const void*)KERNEL<4>; \
    case 5: return (const void*)KERNEL<5>; \
    default: return nullptr;               \
    }

#endif /* LNSFAID_FRAME4_H */
