/*
 * lnsfaid_kernel4cw.hip — the four-rows-per-lane decoder under the per-codeword early stop (gfx950).
 *
 * The same decoder as lnsfaid_kernel4.hip (one wave per codeword, the layer step of lnsfaid_swar.h, the loops of
 * lnsfaid_rows4.h), with the one difference of the rule: a codeword stops at the first decision point at which IT is clean,
 * whatever its 31 group mates do.  That removes everything the group rule needs between launches - no status double buffer, no
 * parking, no En / bit-plane / lane-state traffic through HBM, no relaunch: one launch per batch, and a workgroup that is done
 * writes its decisions and statistics and exits, so the grid refills its slot with the next codeword.  Decoding codeword c
 * under this rule equals the reference decoding a group of 32 copies of c (the lanes interact only through the group-wide
 * break), which is how the tests check it.
 * Instances: those lf_decode4_func serves for the group rule (DecodeMethods 0..5, messages in registers or streamed through
 * HBM, the erasing instance of EF_ELIMINATION 2).
 */
#include <hip/hip_runtime.h>

#include "lnsfaid_rows4.h"

/* what a clean syndrome does under the per-codeword rule (the decode loops of lnsfaid_rows4.h): the codeword stops there; a
 * codeword is always on its own front */
#define LF4_ON_FRONT true
#define LF4_CLEAN_STOPS(t) true
#define LF4_ON_STOP(t)
#define LF4_ON_PASS(t)

template <int METHOD, bool RM, bool EF2>
__global__ __launch_bounds__(LF_T4, 2) void lnsfaid_decode4cw_kernel(LfCwArgs a)
{
    extern __shared__ __align__(16) unsigned char smem[];
    CCode c = (CCode)a.code;
    CCfg f = (CCfg)a.cfg;
    const int tid = (int)threadIdx.x;
    const int cw = (int)blockIdx.x;
    const int N = c->n_var, M = c->n_check, K = c->k_info, nw = c->n_words, pw = c->p_words;
    /* (En at LDS offset 0: no static LDS, checked by lnsfaid_capi.hip kernel_check as for the group-rule kernel) */
    uint32_t* sHard0 = (uint32_t*)smem;      /* bit-flipping stage: hard_ch and hard2 overlay the dead En */
    uint32_t* sHard2 = (uint32_t*)smem + nw;
    uint32_t* sHard = (uint32_t*)(smem + lf_lds_off_hard(N));
    uint32_t* sP = (uint32_t*)(smem + lf_lds_off_p(N, nw));
    int* sStat = (int*)(smem + lf_lds_off_stat(N, nw, pw));
    int* sRed = sStat + LNSFAID_GROUP;

    const int max_iter = f->max_iter, max_bf = f->max_bf;
    const int t_bf0 = max_iter + 1;   /* first bit-flipping decision point */
    const int t_end = t_bf0 + max_bf; /* both loops exhausted               */
    const int g = cw >> 5, lane_in_group = cw & 31;
    if (a.skip && (a.skip[cw] & LF_DONE)) return; /* a group without a call in this batch of the call combiner (uniform exit) */
    if (tid == LNSFAID_GROUP) sRed[LF_ZERO_SLOT] = 0; /* the word unused synw slots point at */

    SwRow* g_rows = (SwRow*)(a.st_rows + (size_t)cw * (size_t)(c->nbr * LF_T)); /* !RM: the messages between layers */
    int8_t* g_out = a.decoded + (size_t)cw * (size_t)N;
    LfLaneState ls = { 0, 0, 0, 0 };
    SwRegs R; /* RM: the codeword's compressed messages (dead in the bit-flipping stage) */
    if (RM) regs_clear(R);

    LF4_STAGE_INPUT()
    LF_WG_SYNC();
    int prog = 1;
    bool in_bf = false;
    bool parked = false; /* under this rule: stopped clean at decision point prog */
    uint32_t pA = 0, pB = 0;
    /* ---- layered iterations, then the bit-flipping stage (lnsfaid_rows4.h, hooks above) ---- */
    {
        LF4_LAYERED_LOOP()
        LF4_ENTER_BF()
    }
    LF4_BF_LOOPS()
    const bool clean = parked;

    /* the hard decisions: the plane the last syndrome stage checked (clean), the bit-flipping state, or the plane of the final En */
    if (!clean && !in_bf) build_plane4<false>(c, sHard, 0, tid);
    int unsat = 0;
    if (!clean && a.cw_stats) { /* ran out of iterations: one syndrome pass of the output plane */
        if (RM || syn_cache_fits(c->nbr)) {
            SynCache sc;
            syn_cache_load(a.code, c->nbr, tid, sc);
            unsat = syndrome<LF_T4, false, true>(c, a.code, sP, tid, pA, pB, sRed, &sc);
        } else {
            unsat = syndrome<LF_T4, false>(c, a.code, sP, tid, pA, pB, sRed);
        }
    }
    write_decoded(sHard, g_out, N, tid);
    if (tid == 0) {
        const int it = prog <= max_iter ? prog - 1 : max_iter;
        const int bf = prog <= max_iter ? 0 : prog - t_bf0;
        if (a.cw_stats) {
            lnsfaid_codeword_stats st;
            st.iterations = it; st.bf_iterations = bf; st.unsatisfied = unsat;
            a.cw_stats[cw] = st;
        }
        if (a.stats) { /* the group's record: maxima over its codewords (zeroed by the host in front of the launch) */
            atomicMax(&a.stats[g].iterations, it);
            atomicMax(&a.stats[g].bf_iterations, bf);
        }
    }
}

/* the instance a configuration runs on under the per-codeword rule: the same set as lf_decode4_func */
extern "C" const void* lf_decode4cw_func(int method, int ef, int rm)
{
    if (method == 2 && ef == 2) return (const void*)lnsfaid_decode4cw_kernel<2, false, true>;
#define LF4CW_FUNC(M) case M: return rm ? (const void*)lnsfaid_decode4cw_kernel<M, true, false> : (const void*)lnsfaid_decode4cw_kernel<M, false, false>;
    switch (method) {
    case 0: return (const void*)lnsfaid_decode4cw_kernel<0, false, false>;
        LF4CW_FUNC(1) LF4CW_FUNC(2) LF4CW_FUNC(3) LF4CW_FUNC(4) LF4CW_FUNC(5)
    default: return nullptr;
    }
#undef LF4CW_FUNC
}

extern "C" hipError_t lf_launch_decode4cw(int method, int ef, int rm, const LfCwArgs* args, size_t lds_bytes, hipStream_t stream)
{
    const void* fn = lf_decode4cw_func(method, ef, rm);
    if (!fn) return hipErrorInvalidValue;
    void* kargs[] = { (void*)args };
    return hipLaunchKernel(fn, dim3((unsigned)args->n_cw), dim3(LF_T4), kargs, lds_bytes, stream);
}
