/*
 * lnsfaid_kernel4.hip — the decode kernel with ONE wavefront per codeword and four check rows per lane (gfx950).
 *
 * Same decoder, same group-of-32 protocol, same HBM state as lnsfaid_kernels.hip (see its header for the decision-point time
 * line and the park / relaunch rules); what differs is how a layer is computed:
 *   - lane i owns rows i, i + 64, i + 128, i + 192 of every layer; byte k of a working register belongs to row i + 64 k and
 *     the layer step is carry-free byte-parallel arithmetic on plain 32-bit operations (lnsfaid_swar.h) instead of two rows on
 *     packed 16-bit operations: 928 VALU instructions per layer of 256 rows, 70 % of them of the full-rate class, against
 *     2 x 615 with three quarters of the half-rate class;
 *   - En is kept in LDS interleaved (variable node v of a block column in dword v mod 64, byte v div 64, biased by 120), so an
 *     edge is one ds_read_b32 + one byte rotation for four rows, and a workgroup is a single wave: no barrier between layers;
 *   - the compressed messages of a lane's four rows are 24 bytes per layer (SwRow).
 * One wave per codeword means two waves per SIMD (the LDS image of a codeword allows 8 per CU), and with two waves nothing hides a
 * stall: every loop that loads keeps all its loads in flight before the first use, the walk tables of the bit-flipping stage live in
 * registers, and everything on the hot path is inlined (tests/test_kernel_isa.py holds these properties).
 * Used for DecodeMethods 1..5 whenever the FAID tables are uniform over the weight classes and non-decreasing (every shipped
 * set) and for DecodeMethod 0 with one normalisation factor >= 15; other tables / factors run on the two-rows-per-lane kernel.
 */
#include <hip/hip_runtime.h>

#define LF4_DIRTY_CHECK(c, lane) layer0_dirty4_edgewise(c, lane) /* the ratchets on this file's layer blocks hold with this text only (lnsfaid_rows4.h) */
#include "lnsfaid_rows4.h"

/* what a clean syndrome does under the group rule (the decode loops of lnsfaid_rows4.h): a codeword on the group's front parks,
 * unless a group mate is known to have passed the point; one behind it is known to go on */
#define LF4_ON_FRONT prog >= kmax
#define LF4_CLEAN_STOPS(t) prog >= kmax && !group_passed(a.live, g, prog, t)
#define LF4_ON_STOP(t) if (RM && prog >= 2) regs_store(R, g_rows, c->nbr, t); /* the messages leave the registers where it parks */
#define LF4_ON_PASS(t) publish_pass(a.live, cw, prog, t);

/* ---- the decode kernel: one wave per codeword ---------------------------------------------------------- */
template <int METHOD, bool RM, bool EF2>
__global__ __launch_bounds__(LF_T4, 2) void lnsfaid_decode4_kernel(LfKernelArgs a)
{
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

/* Instances: messages in registers (RM) for codes of up to LF4_RM_LAYERS layers, streamed through HBM otherwise; the erasing
 * layer step of EF_ELIMINATION 2 (Decode_FAID only) lives in an instance of its own, so that the common ones do not carry its
 * registers. */
extern "C" int lf_decode4_rm_layers(void) { return LF4_RM_LAYERS; }

/* the instance a configuration runs on (for hipFuncGetAttributes / the occupancy query, and for the launch) */
extern "C" const void* lf_decode4_func(int method, int ef, int rm)
{
    if (method == 2 && ef == 2) return (const void*)lnsfaid_decode4_kernel<2, false, true>;
#define LF4_FUNC(M) case M: return rm ? (const void*)lnsfaid_decode4_kernel<M, true, false> : (const void*)lnsfaid_decode4_kernel<M, false, false>;
    switch (method) {
    case 0: return (const void*)lnsfaid_decode4_kernel<0, false, false>; /* (16-level search: with the messages in registers too the layer step spills) */
        LF4_FUNC(1) LF4_FUNC(2) LF4_FUNC(3) LF4_FUNC(4) LF4_FUNC(5)
    default: return nullptr;
    }
#undef LF4_FUNC
}
extern "C" int lf_decode4_threads(void) { return LF_T4; }

extern "C" hipError_t lf_launch_decode4(int method, int ef, int rm, const LfKernelArgs* args, size_t lds_bytes, hipStream_t stream)
{
    const void* fn = lf_decode4_func(method, ef, rm);
    if (!fn) return hipErrorInvalidValue;
    void* kargs[] = { (void*)args };
    return hipLaunchKernel(fn, dim3((unsigned)args->n_cw), dim3(LF_T4), kargs, lds_bytes, stream);
}
