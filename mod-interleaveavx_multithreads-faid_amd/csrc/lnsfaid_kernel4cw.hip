/*
 * lnsfaid_kernel4cw.hip — the four-rows-per-lane decoder under the per-codeword early stop (gfx950).
 *
 * The same decoder as lnsfaid_kernel4.hip (one wave per codeword, the layer step of lnsfaid_swar.h, the loops of
 * lnsfaid_rows4.h inside the per-codeword frame of lnsfaid_frame4.h), with the one difference of the rule: a codeword stops at the first decision point at which IT is clean,
 * whatever its 31 group mates do.  That removes everything the group rule needs between launches - no status double buffer, no
 * parking, no En / bit-plane / lane-state traffic through HBM, no relaunch: one launch per batch, and a workgroup that is done
 * writes its decisions and statistics and exits, so the grid refills its slot with the next codeword.  Decoding codeword c
 * under this rule equals the reference decoding a group of 32 copies of c (the lanes interact only through the group-wide
 * break), which is how the tests check it.
 * Instances: those lf_decode4_func serves for the group rule (DecodeMethods 0..5, messages in registers or streamed through
 * HBM, the erasing instance of EF_ELIMINATION 2).
 */
#include <hip/hip_runtime.h>

#include "lnsfaid_frame4.h"
#include "lnsfaid_launch.h"

#define LF4_RULE CW

template <int METHOD, bool RM, bool EF2>
__global__ __launch_bounds__(LF_T4, 2) void lnsfaid_decode4cw_kernel(LfCwArgs a)
{
    LF4_LOCALS()
    const int g = cw >> 5, lane_in_group = cw & 31;
    if (a.skip && (a.skip[cw] & LF_DONE)) return; /* a group without a call in this batch of the call combiner (uniform exit) */
    LF4_CW_CORE(LF4_STAGE_INPUT, a.cw_stats)
    int8_t* g_out = a.decoded + (size_t)cw * (size_t)N;
    write_decoded(sHard, g_out, N, tid);
    LF4_CW_RECORDS()
}

/* the instance a configuration runs on under the per-codeword rule: the same set as lf_decode4_func */
extern "C" const void* lf_decode4cw_func(int method, int ef, int rm)
{
    LF4_INSTANCE_TABLE(lnsfaid_decode4cw_kernel)
}
