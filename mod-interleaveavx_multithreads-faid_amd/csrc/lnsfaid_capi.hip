/*
 * lnsfaid_capi.hip — host side of the C ABI declared in include/lnsfaid.h.
 *
 * Owns the context (device tables, per-codeword state in HBM, one HIP stream, events) and drives the
 * relaunch loop described at the top of lnsfaid_kernels.hip.  There is no CPU decode path in this
 * library: without a GPU lnsfaid_create() fails with LNSFAID_E_NODEVICE.
 */
#include <hip/hip_runtime.h>

#include <dlfcn.h>
#include <rccl/rccl.h> /* types and enums only: the library is bound at run time (lf_rccl below) */

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "lnsfaid_device.h"
#include "lnsfaid_line.h"
#include "lnsfaid_burst.h"
#include "lnsfaid_quantise.h"
#include "lnsfaid_swar.h" /* sw_nms_fits / sw_nms_tables (host side) */
#include "lnsfaid_launch.h" /* what the kernel files export */

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <thread>
struct LfCombiner;
static thread_local char g_hip_err[256] = "";
/* Contexts alive in this process.  A host thread that waits for its stream by spinning (hipStreamSynchronize) is the
 * lowest-latency choice for a few contexts, and the worst one for the reference's call shape - one context per worker thread,
 * 64 of them (reference main.cpp:31-34, :164-172): the spinning threads then fight for the cores the HIP runtime itself needs.
 * From LF_SPIN_CONTEXTS live contexts on, waits go through an event created with hipEventBlockingSync (the thread sleeps
 * until the interrupt); LNSFAID_SYNC=spin / block overrides. */
static std::atomic<int> g_live_contexts(0);
#define LF_SPIN_CONTEXTS 4
static bool sync_blocking()
{
    static const char* e = getenv("LNSFAID_SYNC");
    if (e && e[0] == 's') return false;
    if (e && e[0] == 'b') return true;
    return g_live_contexts.load(std::memory_order_relaxed) > LF_SPIN_CONTEXTS;
}

static int hip_fail(hipError_t e, const char* what)
{
    snprintf(g_hip_err, sizeof(g_hip_err), "%s: %s", what, hipGetErrorString(e));
    return LNSFAID_E_HIP;
}
#define HIP_TRY(call)                                      \
    do {                                                   \
        hipError_t e_ = (call);                            \
        if (e_ != hipSuccess) return hip_fail(e_, #call);  \
    } while (0)

#define LF_IO_CHUNKS 8 /* pieces the host-pointer path is cut into when both host buffers are pinned */
#define LF_MAX_CHAIN 6 /* decode launches queued back to back before the host looks at their "codewords left" counters */

struct lnsfaid_ctx {
    int device = 0;
    size_t max_groups = 0;
    LfDevCode hcode;
    LfDevCfg hcfg;
    int n_var = 0, n_check = 0, k_info = 0;
    size_t lds_bytes = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t ev_chain[LF_MAX_CHAIN + 1] = {}; /* time stamps around the launches of a chain */
    hipEvent_t ev_block = nullptr;              /* hipEventBlockingSync: where the host waits when many contexts are alive */
    uint32_t slot_seen[LF_MAX_CHAIN] = {};      /* last value read of each running "codewords left" counter */
    int predicted_launches = 1;                 /* launches the previous batch needed: how many this one queues at once */
    hipStream_t s_in = nullptr, s_out = nullptr; /* copy streams of the pipelined host-pointer path */
    hipEvent_t ev_in[LF_IO_CHUNKS] = {};
    LfDevCode* d_code = nullptr;
    LfDevCfg* d_cfg = nullptr;
    int8_t* d_en = nullptr;
    uint4* d_rows = nullptr;
    uint32_t* d_bits = nullptr;
    LfLaneState* d_lane = nullptr;
    int32_t* d_status[2] = { nullptr, nullptr };
    uint32_t* d_remaining = nullptr;
    int32_t* d_live = nullptr;
    unsigned long long* d_counters = nullptr;
    uint32_t* h_remaining = nullptr;          /* pinned, LF_MAX_CHAIN words */
    unsigned long long* h_counters = nullptr; /* pinned */
    /* staging for the host-pointer entry points */
    int8_t* d_io_in = nullptr;
    int8_t* d_io_out = nullptr;
    lnsfaid_group_stats* d_io_stats = nullptr;
    lnsfaid_codeword_stats* d_io_cw_stats = nullptr; /* lnsfaid_decode_codewords, allocated at its first call */
    /* staging for the packed host-pointer entry points, allocated at the first packed call */
    uint8_t* d_pk_in = nullptr;   /* llr4, 16 * n_var bytes per group */
    uint32_t* d_pk_out = nullptr; /* bits, n_var words per group */
    lnsfaid_group_stats* d_pk_stats = nullptr;
    /* staging for lnsfaid_decode_line, allocated at its first call; line and bits go through d_pk_in / d_pk_out */
    uint32_t* d_ln_payload = nullptr;       /* K words per group */
    lnsfaid_line_stats* d_ln_stats = nullptr;
    /* burst-format line calls, allocated at their first call */
    LfBurstDesc* d_burst_desc = nullptr;    /* [32 * max_groups] descriptors of the call in flight */
    LfBurstDesc* h_burst_desc = nullptr;    /* pinned: where the host forms its prefix sums */
    uint32_t* d_burst_ones = nullptr;       /* short_ones of the host-pointer decode */
    int early_stop = LNSFAID_STOP_GROUP; /* rule of lnsfaid_decode / lnsfaid_decode_device (lnsfaid_set_early_stop) */
    int rows_per_lane = 0; /* 0: pick per configuration; 2 / 4: forced (lnsfaid_select_kernel) */
    int waves_per_cw = 0;  /* 0 / 1: one wave per codeword; 2: lnsfaid_kernel5.hip where it applies (lnsfaid_select_waves) */
    int msg_store = 0;     /* 0: pick per code; 1: registers; 2: streamed through HBM (lnsfaid_select_message_store) */
    int zero_shift = 0;    /* 0: the rotation-free layer step where it applies; 1: the same, asked for; 2: off; 3: its layer loop
                            * (lnsfaid_kernel4z.hip) also where the layer-static kernel applies; 4: the layer-static kernel, asked
                            * for; 5: the same, and lnsfaid_kernel4s.hip also where its window-free twin applies
                            * (lnsfaid_select_zero_shift) */
    int edge_words = 1;    /* lnsfaid_kernel4e.hip where the window-free kernel applies; 0: lnsfaid_kernel4w.hip there (lnsfaid_select_edge_words) */
    mutable int static_code = -1; /* the code's zero-first edge tables equal the layer-static kernel's constants: -1 not compared yet */
    struct LfCombiner* comb = nullptr; /* call combiner this one-group context is a member of (see below) */
    int comb_slot = -1;
    const void* checked_fn[6] = {};           /* kernel instance kernel_check() last looked at, per entry kind (LF_ENTRY_*) */
    int resident_wg[4] = {}, lds_wg[4] = {};  /* its workgroups per CU: what the occupancy query says / what its LDS alone allows
                                               * (the four entry kinds of the decode calls) */
    void* comm = nullptr;      /* ncclComm_t for lnsfaid_allreduce_counters */
    bool comm_owned = false;
    unsigned long long* d_reduce = nullptr;
    double kernel_ms = 0.0;
    uint64_t kernel_launches = 0;
    /* device front-end scratch: seeds, draw counters, transmitted codeword */
    uint32_t* d_fe_seeds = nullptr;
    unsigned long long* d_fe_draws = nullptr;
    int8_t* d_fe_codeword = nullptr;
    int8_t* d_fe_frames = nullptr; /* per-stream sent frames (lnsfaid_frontend_set_frames), encoder output layout */
    int8_t* d_fe_input = nullptr;  /* their information bits, [stream][32][K] */
    size_t fe_frames_streams = 0;  /* 0: frames not in use */
    int fe_interleave = 1;         /* InterleaveModType of the device front-end */
    int fe_exact = 0;              /* 1: every symbol through the double-precision chain (lnsfaid_frontend_set_exact) */
    int fe_prefec = 0;             /* scope of the fused pre-FEC counting (lnsfaid_frontend_set_prefec), 0 = off */
    unsigned long long* d_fe_prefec_frames = nullptr; /* [max_groups * 32] wrong bits | symbols << 32 per frame of one call */
    unsigned long long* d_fe_prefec_acc = nullptr;    /* the four counters, read only by lnsfaid_frontend_prefec_counters */
    /* error-frame capture (lnsfaid_capture.hip), allocated at the first lnsfaid_capture_errors_device call */
    uint2* d_cap_cnt = nullptr;                /* [max_groups * 32] wrong information / parity decisions per codeword */
    unsigned long long* d_cap_meta = nullptr;  /* found, stored, then the four counters of the call: one copy brings all six back */
    unsigned long long* h_cap_meta = nullptr;  /* pinned */
    size_t cap_slots = 0;                      /* slots the three buffers below hold: grown on demand */
    uint32_t* d_cap_slots = nullptr;           /* codeword of every slot */
    lnsfaid_error_record* d_cap_records = nullptr;
    int8_t* d_cap_payload = nullptr;           /* 3 * n_var bytes per slot */
    /* FEC status (lnsfaid_fecstatus.hip), allocated at the first lnsfaid_fec_status*_device call */
    unsigned long long* d_fec_acc = nullptr; /* out[4] then vs_sent[4] of the call in flight */
    unsigned long long* h_fec_acc = nullptr; /* pinned */
    /* line-format link (lnsfaid_line_link.hip), allocated at the first lnsfaid_line_bsc_device / lnsfaid_line_count_errors_device call */
    unsigned long long* d_link_acc = nullptr; /* errors[4], fec[4], vs_sent[4] of the call in flight, then the channel's flipped bits and runs */
    unsigned long long* h_link_acc = nullptr; /* pinned */
    /* line-format failure capture (lnsfaid_line_capture.hip), allocated at the first lnsfaid_line_capture_device call */
    uint4* d_lcap_cnt = nullptr;                /* [max_groups * 32] flags, unsatisfied, wrong payload / parity bits per codeword */
    unsigned long long* d_lcap_meta = nullptr;  /* found, stored */
    unsigned long long* h_lcap_meta = nullptr;  /* pinned */
    size_t lcap_slots = 0, lcap_words = 0;      /* what the three buffers below hold: slots, payload words; grown on demand */
    uint32_t* d_lcap_slots = nullptr;           /* index of every slot's codeword */
    lnsfaid_line_failure* d_lcap_records = nullptr;
    uint32_t* d_lcap_payload = nullptr;
    /* encoder (lnsfaid_encoder.hip): support of B^-1's first rows, derived at the first encode / random-frames call */
    int enc_state = 0;                      /* 0: not derived yet, 1: on the device, LNSFAID_E_CODE: parity part singular */
    uint32_t* d_enc_sup = nullptr;          /* entries b * z + c, block row after block row */
    uint32_t* d_enc_off = nullptr;          /* [mb + 1] start of every block row's entries */
    unsigned long long* d_fe_keys = nullptr; /* stream keys of lnsfaid_frontend_random_frames */
};

/* wait until everything queued on the context's stream so far has finished */
static int stream_wait(lnsfaid_ctx* ctx)
{
    if (sync_blocking()) {
        HIP_TRY(hipEventRecord(ctx->ev_block, ctx->stream));
        HIP_TRY(hipEventSynchronize(ctx->ev_block));
    } else {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    return LNSFAID_OK;
}

/* ---- code analysis: PosNoeudsVariable -> circulants ------------------------------------------------- */
static int weight_class(int w) { return w == 3 ? 0 : (w == 6 ? 1 : (w == 11 ? 2 : 3)); } /* CDecoder_FAID.cpp:692-705 */

/* one entry of a syndrome walk table (LfDevCode::synw): word k of the 32-row words of circulant sb, hard plane at LDS offset hard0 */
static uint2 syn_entry(uint32_t hard0, uint32_t sb, int k)
{
    const uint32_t cb = sb / (uint32_t)LF_Z, sh = sb % (uint32_t)LF_Z;
    const uint32_t o = (32u * (uint32_t)k + sh) & 255u, q = o >> 5;
    uint2 e;
    e.x = (hard0 + 4u * (cb * 8u + q)) | ((hard0 + 4u * (cb * 8u + ((q + 1u) & 7u))) << 16);
    e.y = o & 31u;
    return e;
}
static uint2 syn_zero_entry(uint32_t zero)
{
    uint2 e;
    e.x = zero | (zero << 16); e.y = 0;
    return e;
}

static int build_code(const lnsfaid_code* code, LfDevCode* out)
{
    memset(out, 0, sizeof(*out));
    if (!code || !code->pos_vn || !code->deg || !code->deg_rows) return LNSFAID_E_INVAL;
    const int Z = code->z, N = code->n_var, M = code->n_check, E = code->n_edges;
    if (Z != LF_Z) return LNSFAID_E_CODE; /* kernels map the 256 rows of a circulant onto 128 threads x 2 rows */
    if (N <= 0 || M <= 0 || N % Z || M % Z || M >= N) return LNSFAID_E_CODE;
    const int nbr = M / Z, nbc = N / Z, K = N - M;
    if (nbr > LF_MAX_BR || nbc > LF_MAX_BC) return LNSFAID_E_CODE;
    if (K % 4 || M % 4 || N % LF_T) return LNSFAID_E_CODE; /* dword staging, 64-wide ballots over VNs */
    if (code->puncture_tail < 0 || code->puncture_tail > N) return LNSFAID_E_CODE;
    /* degree of each check row from the DEG_k / DEG_k_COMPUTATIONS classes */
    std::vector<int> row_deg;
    row_deg.reserve(M);
    long e_total = 0;
    for (int k = 0; k < code->nb_degres; ++k) {
        if (code->deg_rows[k] < 0 || code->deg[k] < 2 || code->deg[k] > LF_MAX_DEG) return LNSFAID_E_CODE;
        for (int i = 0; i < code->deg_rows[k]; ++i) { row_deg.push_back(code->deg[k]); e_total += code->deg[k]; }
    }
    if ((int)row_deg.size() != M || e_total != E) return LNSFAID_E_CODE;

    size_t e = 0;
    for (int br = 0; br < nbr; ++br) {
        const int deg = row_deg[(size_t)br * Z];
        out->deg[br] = deg;
        const uint16_t* row0 = code->pos_vn + e;
        for (int j = 0; j < 64; ++j) out->sbtab[br][j] = 0u;
        for (int j = 0; j < 32; ++j) out->sbplain[br][j] = 0u;
        int prev_cb = -1;
        for (int j = 0; j < deg; ++j) {
            const int cb = row0[j] / Z, sh = row0[j] % Z;
            if (row0[j] >= N || cb <= prev_cb) return LNSFAID_E_CODE; /* ascending, no block column twice */
            prev_cb = cb;
            out->circ[br][j].sb = (uint32_t)cb * (uint32_t)Z + (uint32_t)sh;
            out->sbtab[br][LF_JCODE_A(j)] = out->sbtab[br][LF_JCODE_B(j)] = out->circ[br][j].sb;
            out->sbplain[br][j] = (((uint32_t)cb * (uint32_t)Z) << 16) | (((uint32_t)sh) << 2);
            out->s4tab[br][j] = ((uint32_t)sh) << 2;
            out->cbtab[br][j] = (uint32_t)cb * (uint32_t)Z;
            if (out->col_weight[cb] >= LF_MAX_COLW) return LNSFAID_E_CODE;
            out->colcirc[cb][out->col_weight[cb]++] = (uint32_t)br | ((uint32_t)sh << 8);
        }
        for (int i = 0; i < Z; ++i) {
            if (row_deg[(size_t)br * Z + i] != deg) return LNSFAID_E_CODE;
            for (int j = 0; j < deg; ++j) {
                const uint32_t sb = out->circ[br][j].sb;
                const int want = (int)(sb / (uint32_t)Z * (uint32_t)Z + (sb % (uint32_t)Z + (uint32_t)i) % (uint32_t)Z);
                if (code->pos_vn[e + (size_t)i * deg + j] != want) return LNSFAID_E_CODE; /* not quasi-cyclic */
            }
        }
        e += (size_t)deg * Z;
        /* the rotation-free layer step's tables (lnsfaid_kernel4z.hip): the zero-shift edges first, ascending block column within
         * either class (the row is ascending, the partition is stable), and the layer's instance of the step */
        for (int j = 0; j < 32; ++j) out->zsbplain[br][j] = 0u;
        int n = 0;
        for (int zero = 1; zero >= 0; --zero)
            for (int j = 0; j < deg; ++j)
                if ((out->s4tab[br][j] == 0u) == (zero != 0)) {
                    out->zsbplain[br][n] = out->sbplain[br][j];
                    out->zs4tab[br][n] = out->s4tab[br][j];
                    out->zcbtab[br][n] = out->cbtab[br][j];
                    ++n;
                }
        int n_zero = 0;
        while (n_zero < deg && out->zs4tab[br][n_zero] == 0u) ++n_zero;
        out->zinst[br] = lf_decode4z_inst(deg, n_zero / 4);
    }
    {   /* syndrome walk table: needs the LDS layout (n_words = N / 32, p_words = M / 32) */
        const int nw = N / 32, pw = M / 32;
        const uint32_t hard0 = lf_lds_off_hard(N), zero = lf_lds_off_zero(N, nw, pw);
        if (lf_lds_bytes(N, nw, pw) > 0xffffu) return LNSFAID_E_CODE; /* 16-bit addresses */
        for (int br = 0; br < LF_MAX_BR; ++br)
            for (int j = 0; j < LF_MAX_DEG; ++j)
                for (int k = 0; k < 8; ++k)
                    out->synw[br][j][k] = (br < nbr && j < out->deg[br]) ? syn_entry(hard0, out->circ[br][j].sb, k) : syn_zero_entry(zero);
    }
    for (int br = 0; br < nbr; ++br)
        for (int j = 0; j < out->deg[br]; ++j)
            out->circ[br][j].wclass = (uint32_t)weight_class(out->col_weight[out->circ[br][j].sb / (uint32_t)Z]);
    out->n_var = N; out->n_check = M; out->k_info = K; out->nbr = nbr; out->nbc = nbc;
    out->puncture_tail = code->puncture_tail;
    out->n_words = N / 32; out->p_words = M / 32;
    return LNSFAID_OK;
}

/* block columns the bit-flipping stage may touch: column weight == REGULAR_COL_WEIGHT */
static void build_wcols(LfDevCode* code, int W)
{
    code->n_wcols = 0;
    for (int cb = 0; cb < code->nbc; ++cb)
        if (code->col_weight[cb] == W) code->wcol[code->n_wcols++] = cb;
    /* first occurrence of every weight-W block column in row order (reference era_[]: CDecoder_FAID.cpp:673-680) */
    bool seen[LF_MAX_BC] = {};
    for (int br = 0; br < LF_MAX_BR; ++br) {
        code->era_edges[br] = 0;
        for (int j = 0; br < code->nbr && j < code->deg[br]; ++j) {
            const int cb = (int)(code->circ[br][j].sb / LF_Z);
            if (code->col_weight[cb] == W && !seen[cb]) { seen[cb] = true; code->era_edges[br] |= 1u << j; }
        }
    }
    /* the syndrome walk split for the bit-flipping stage: circulants of weight-W block columns / all others, in row order */
    const uint32_t hard0 = lf_lds_off_hard(code->n_var), zero = lf_lds_off_zero(code->n_var, code->n_words, code->p_words);
    code->bfw_fits = 1;
    for (int br = 0; br < LF_MAX_BR; ++br) {
        int nw = 0, nc = 0;
        for (int j = 0; br < code->nbr && j < code->deg[br]; ++j) {
            const uint32_t sb = code->circ[br][j].sb;
            const bool w = code->col_weight[sb / LF_Z] == W;
            /* more than the table holds: synw_w stays incomplete and is not used - the stage takes the uncached walk of synw */
            if (w && nw == 2 * LF_BFW_JP) { code->bfw_fits = 0; continue; }
            for (int k = 0; k < 8; ++k) (w ? code->synw_w[br][nw] : code->synw_c[br][nc])[k] = syn_entry(hard0, sb, k);
            ++(w ? nw : nc);
        }
        for (; nw < 2 * LF_BFW_JP; ++nw)
            for (int k = 0; k < 8; ++k) code->synw_w[br][nw][k] = syn_zero_entry(zero);
        for (; nc < LF_MAX_DEG; ++nc)
            for (int k = 0; k < 8; ++k) code->synw_c[br][nc][k] = syn_zero_entry(zero);
    }
}

static int build_cfg(const lnsfaid_cfg* cfg, LfDevCfg* out)
{
    if (!cfg) return LNSFAID_E_INVAL;
    if (cfg->decode_method < 0 || cfg->decode_method > 5) return LNSFAID_E_INVAL;
    if (cfg->max_iteration < 0 || cfg->max_iteration > (1 << 20)) return LNSFAID_E_INVAL;
    if (cfg->max_bf_iter < 0 || cfg->max_bf_iter > (1 << 20)) return LNSFAID_E_INVAL;
    if (cfg->regular_col_weight < 0 || cfg->regular_col_weight > LF_MAX_COLW) return LNSFAID_E_INVAL;
    memset(out, 0, sizeof(*out));
    out->method = cfg->decode_method;
    out->max_iter = cfg->max_iteration;
    /* OMS: VECTOR_SET1 int8 lanes; NMS: VECTOR_SET2 int16 lanes (CLDPC.cpp:337, :345) */
    out->factor_1 = cfg->decode_method == 0 ? (int16_t)cfg->factor_1 : (int8_t)cfg->factor_1;
    out->factor_2 = cfg->decode_method == 0 ? (int16_t)cfg->factor_2 : (int8_t)cfg->factor_2;
    out->floor_err_count = cfg->floor_err_count;
    out->floor_iter_thresh = cfg->floor_iter_thresh;
    out->ef = cfg->ef_elimination;
    out->max_bf = (cfg->decode_method == 0 || cfg->decode_method == 1) ? 0 : cfg->max_bf_iter; /* Decode / Decode_OMS have no BF stage */
    out->L0 = cfg->bf_L0; out->L1 = cfg->bf_L1; out->alpha = cfg->bf_alpha; out->delta = cfg->bf_delta;
    out->W = cfg->regular_col_weight;
    out->hard2_thr = cfg->hard2_threshold;
    out->vote_cap = (int8_t)cfg->bf_vote_cap;
    /* OMS offsets (CDecoder_OMS.cpp:388-425) leave the 3-bit message alphabet for Factor_1 < 0 or Factor_2 < 1: the
     * minimum 0 would become -1 */
    if ((cfg->decode_method == 1 || cfg->decode_method == 3 || cfg->decode_method == 4)
        && ((int8_t)cfg->factor_1 < 0 || (int8_t)cfg->factor_2 < 1)) return LNSFAID_E_INVAL;
    if (cfg->decode_method == 5 && cfg->ef_elimination != 1) return LNSFAID_E_INVAL;
    if (cfg->decode_method == 2 && (cfg->ef_elimination < 0 || cfg->ef_elimination > 2)) return LNSFAID_E_INVAL;
    if (cfg->decode_method != 2 && cfg->decode_method != 5 && cfg->ef_elimination != 0) return LNSFAID_E_INVAL;
    out->uniform_w = 1;
    for (int it = 0; it < 6; ++it)
        for (int w = 0; w < 4; ++w) {
            for (int a = 0; a < 8; ++a) {
                const int v = cfg->v2c_map[it][w][a], ve = cfg->v2c_map_ef[it][w][a];
                if ((cfg->decode_method == 2 || cfg->decode_method == 5) && (v < 0 || v > 7)) return LNSFAID_E_INVAL; /* 3-bit message alphabet */
                if ((cfg->decode_method == 5 || cfg->ef_elimination >= 1) && (ve < 0 || ve > 7)) return LNSFAID_E_INVAL;
                uint32_t* l = a < 4 ? &out->lut_lo[it][w] : &out->lut_hi[it][w];
                uint32_t* le = a < 4 ? &out->lut_ef_lo[it][w] : &out->lut_ef_hi[it][w];
                *l |= (uint32_t)(v & 0xff) << (8 * (a & 3));
                *le |= (uint32_t)(ve & 0xff) << (8 * (a & 3));
                /* a table that is not non-decreasing cannot be applied after the minimum search */
                if (a > 0 && (v < cfg->v2c_map[it][w][a - 1] || ((cfg->decode_method == 5 || cfg->ef_elimination >= 1) && ve < cfg->v2c_map_ef[it][w][a - 1])))
                    out->uniform_w = 0;
            }
            if (out->lut_lo[it][w] != out->lut_lo[it][0] || out->lut_hi[it][w] != out->lut_hi[it][0]) out->uniform_w = 0;
            if ((cfg->decode_method == 5 || cfg->ef_elimination >= 1)
                && (out->lut_ef_lo[it][w] != out->lut_ef_lo[it][0] || out->lut_ef_hi[it][w] != out->lut_ef_hi[it][0]))
                out->uniform_w = 0;
        }
    if (cfg->decode_method == 0) {
        out->uniform_w = (out->factor_1 == out->factor_2) ? 1 : 0; /* NMS: one factor -> patch path */
        out->nms_fits = sw_nms_fits(out->factor_1, out->factor_2) ? 1 : 0;
        if (out->nms_fits) sw_nms_tables(out->factor_1, out->nms_t);
    }
    /* Decode_FAID with EF_ELIMINATION 1 / 2 exists in the four-rows-per-lane kernel only, which needs uniform tables */
    if (cfg->decode_method == 2 && cfg->ef_elimination >= 1 && !out->uniform_w) return LNSFAID_E_INVAL;
    out->bf_fast = (out->W == 3 && ((int8_t)out->alpha == 0 || (int8_t)out->alpha == 1)) ? 1 : 0;
    return LNSFAID_OK;
}

/* DecodeMethod 3 counts the votes of a variable node in four bit planes (bf_step_plain): column weight <= 15.  Checked when a
 * context is created and again when lnsfaid_set_cfg switches an existing context to DecodeMethod 3. */
static int check_code_for_method(const LfDevCode* code, int method)
{
    if (method == 3)
        for (int cb = 0; cb < code->nbc; ++cb)
            if (code->col_weight[cb] > 15) return LNSFAID_E_CODE;
    return LNSFAID_OK;
}

/* ---- context ------------------------------------------------------------------------------------------- */
extern "C" int lnsfaid_comm_destroy(lnsfaid_ctx* ctx);
static int comb_join(lnsfaid_ctx* ctx);
static void comb_leave(lnsfaid_ctx* ctx, int slot);
extern "C" void lnsfaid_destroy(lnsfaid_ctx* ctx)
{
    if (!ctx) return;
    if (ctx->comb_slot >= 0) { comb_leave(ctx, ctx->comb_slot); ctx->comb_slot = -1; }
    g_live_contexts.fetch_sub(1, std::memory_order_relaxed);
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    (void)lnsfaid_comm_destroy(ctx);
    (void)hipFree(ctx->d_reduce);
    (void)hipFree(ctx->d_code); (void)hipFree(ctx->d_cfg); (void)hipFree(ctx->d_en); (void)hipFree(ctx->d_rows);
    (void)hipFree(ctx->d_bits); (void)hipFree(ctx->d_lane); (void)hipFree(ctx->d_status[0]); (void)hipFree(ctx->d_status[1]);
    (void)hipFree(ctx->d_remaining); (void)hipFree(ctx->d_live); (void)hipFree(ctx->d_counters);
    (void)hipFree(ctx->d_io_in); (void)hipFree(ctx->d_io_out); (void)hipFree(ctx->d_io_stats);
    (void)hipFree(ctx->d_io_cw_stats);
    (void)hipFree(ctx->d_pk_in); (void)hipFree(ctx->d_pk_out); (void)hipFree(ctx->d_pk_stats);
    (void)hipFree(ctx->d_ln_payload); (void)hipFree(ctx->d_ln_stats);
    (void)hipFree(ctx->d_burst_desc); (void)hipFree(ctx->d_burst_ones);
    if (ctx->h_burst_desc) (void)hipHostFree(ctx->h_burst_desc);
    (void)hipFree(ctx->d_fe_seeds); (void)hipFree(ctx->d_fe_draws); (void)hipFree(ctx->d_fe_codeword);
    (void)hipFree(ctx->d_fe_frames); (void)hipFree(ctx->d_fe_input);
    (void)hipFree(ctx->d_enc_sup); (void)hipFree(ctx->d_enc_off); (void)hipFree(ctx->d_fe_keys);
    (void)hipFree(ctx->d_fe_prefec_frames); (void)hipFree(ctx->d_fe_prefec_acc);
    (void)hipFree(ctx->d_cap_cnt); (void)hipFree(ctx->d_cap_meta);
    if (ctx->h_cap_meta) (void)hipHostFree(ctx->h_cap_meta);
    (void)hipFree(ctx->d_cap_slots); (void)hipFree(ctx->d_cap_records); (void)hipFree(ctx->d_cap_payload);
    (void)hipFree(ctx->d_fec_acc);
    if (ctx->h_fec_acc) (void)hipHostFree(ctx->h_fec_acc);
    (void)hipFree(ctx->d_link_acc);
    if (ctx->h_link_acc) (void)hipHostFree(ctx->h_link_acc);
    (void)hipFree(ctx->d_lcap_cnt); (void)hipFree(ctx->d_lcap_meta);
    if (ctx->h_lcap_meta) (void)hipHostFree(ctx->h_lcap_meta);
    (void)hipFree(ctx->d_lcap_slots); (void)hipFree(ctx->d_lcap_records); (void)hipFree(ctx->d_lcap_payload);
    if (ctx->h_remaining) (void)hipHostFree(ctx->h_remaining);
    if (ctx->h_counters) (void)hipHostFree(ctx->h_counters);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    for (auto e : ctx->ev_chain) if (e) (void)hipEventDestroy(e);
    if (ctx->ev_block) (void)hipEventDestroy(ctx->ev_block);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    if (ctx->s_in) (void)hipStreamDestroy(ctx->s_in);
    if (ctx->s_out) (void)hipStreamDestroy(ctx->s_out);
    for (auto e : ctx->ev_in) if (e) (void)hipEventDestroy(e);
    delete ctx;
}

static int alloc_state(lnsfaid_ctx* ctx);
static int create_impl(lnsfaid_ctx* ctx, const lnsfaid_code* code, const lnsfaid_cfg* cfg)
{
    int rc = build_code(code, &ctx->hcode);
    if (rc) return rc;
    rc = build_cfg(cfg, &ctx->hcfg);
    if (rc) return rc;
    ctx->n_var = ctx->hcode.n_var; ctx->n_check = ctx->hcode.n_check; ctx->k_info = ctx->hcode.k_info;
    rc = check_code_for_method(&ctx->hcode, ctx->hcfg.method);
    if (rc) return rc;
    build_wcols(&ctx->hcode, ctx->hcfg.W);
    return alloc_state(ctx);
}

/* device state of a context whose hcode / hcfg / device / max_groups are set */
static int alloc_state(lnsfaid_ctx* ctx)
{
    ctx->n_var = ctx->hcode.n_var; ctx->n_check = ctx->hcode.n_check; ctx->k_info = ctx->hcode.k_info;
    ctx->lds_bytes = lf_lds_bytes(ctx->n_var, ctx->hcode.n_words, ctx->hcode.p_words);
    if (ctx->lds_bytes > 64 * 1024) return LNSFAID_E_CODE;

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || ctx->device < 0 || ctx->device >= ndev) {
        snprintf(g_hip_err, sizeof(g_hip_err), "no usable HIP device (count %d, asked for %d)", ndev, ctx->device);
        return LNSFAID_E_NODEVICE;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreate(&ctx->ev0));
    HIP_TRY(hipEventCreate(&ctx->ev1));
    const size_t n_cw = ctx->max_groups * LNSFAID_GROUP;
    HIP_TRY(hipMalloc(&ctx->d_code, sizeof(LfDevCode)));
    HIP_TRY(hipMalloc(&ctx->d_cfg, sizeof(LfDevCfg)));
    HIP_TRY(hipMalloc(&ctx->d_en, n_cw * (size_t)ctx->n_var));
    HIP_TRY(hipMalloc(&ctx->d_rows, n_cw * (size_t)ctx->hcode.nbr * LF_T * sizeof(uint4)));
    HIP_TRY(hipMalloc(&ctx->d_bits, n_cw * (size_t)3 * ctx->hcode.n_words * sizeof(uint32_t)));
    HIP_TRY(hipMalloc(&ctx->d_lane, n_cw * sizeof(LfLaneState)));
    HIP_TRY(hipMalloc(&ctx->d_status[0], n_cw * sizeof(int32_t)));
    HIP_TRY(hipMalloc(&ctx->d_status[1], n_cw * sizeof(int32_t)));
    HIP_TRY(hipMalloc(&ctx->d_remaining, LF_MAX_CHAIN * sizeof(uint32_t)));
    HIP_TRY(hipMemset(ctx->d_remaining, 0, LF_MAX_CHAIN * sizeof(uint32_t)));
    for (auto& e : ctx->ev_chain) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(hipEventCreateWithFlags(&ctx->ev_block, hipEventBlockingSync | hipEventDisableTiming));
    HIP_TRY(hipMalloc(&ctx->d_live, n_cw * sizeof(int32_t)));
    HIP_TRY(hipMalloc(&ctx->d_counters, 4 * sizeof(unsigned long long)));
    HIP_TRY(hipHostMalloc((void**)&ctx->h_remaining, LF_MAX_CHAIN * sizeof(uint32_t), hipHostMallocDefault));
    HIP_TRY(hipHostMalloc((void**)&ctx->h_counters, 4 * sizeof(unsigned long long), hipHostMallocDefault));
    HIP_TRY(hipMemcpy(ctx->d_code, &ctx->hcode, sizeof(LfDevCode), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ctx->d_cfg, &ctx->hcfg, sizeof(LfDevCfg), hipMemcpyHostToDevice));
    return LNSFAID_OK;
}

extern "C" int lnsfaid_create(lnsfaid_ctx** out, const lnsfaid_code* code, const lnsfaid_cfg* cfg, int32_t device,
                              size_t max_groups)
{
    if (!out || !code || !cfg || max_groups == 0 || max_groups > ((size_t)1 << 24)) return LNSFAID_E_INVAL;
    *out = nullptr;
    lnsfaid_ctx* ctx = new (std::nothrow) lnsfaid_ctx();
    if (!ctx) return LNSFAID_E_NOMEM;
    ctx->device = device;
    ctx->max_groups = max_groups;
    if (const char* e = getenv("LNSFAID_ROWS_PER_LANE")) /* test / A-B switch: force the 2-rows-per-lane kernel for a whole run */
        ctx->rows_per_lane = (e[0] == '2') ? 2 : 0;
    if (const char* e = getenv("LNSFAID_WAVES_PER_CODEWORD")) /* test / A-B switch, see lnsfaid_select_waves */
        ctx->waves_per_cw = (e[0] == '2') ? 2 : 0;
    if (const char* e = getenv("LNSFAID_FRONTEND_EXACT")) /* test / A-B switch, see lnsfaid_frontend_set_exact */
        ctx->fe_exact = (e[0] == '1') ? 1 : 0;
    if (const char* e = getenv("LNSFAID_MSG_STORE")) /* test / A-B switch, see lnsfaid_select_message_store */
        ctx->msg_store = (e[0] == 'h') ? LNSFAID_MSG_HBM : ((e[0] == 'r') ? LNSFAID_MSG_REGISTERS : 0);
    if (const char* e = getenv("LNSFAID_ZERO_SHIFT")) /* test / A-B switch, see lnsfaid_select_zero_shift: "off" / "on" */
        ctx->zero_shift = (e[0] == 'o' && e[1] == 'f') ? LNSFAID_ZERO_SHIFT_OFF /* "off" / "loop" / "windowed" */
                          : (e[0] == 'l' ? LNSFAID_ZERO_SHIFT_LOOP : (e[0] == 'w' ? LNSFAID_ZERO_SHIFT_WINDOWED : 0));
    if (const char* e = getenv("LNSFAID_EDGE_WORDS")) /* test / A-B switch, see lnsfaid_select_edge_words: "off" */
        ctx->edge_words = (e[0] == 'o' && e[1] == 'f') ? 0 : 1;
    g_live_contexts.fetch_add(1, std::memory_order_relaxed); /* (lnsfaid_destroy takes it back) */
    const int rc = create_impl(ctx, code, cfg);
    if (rc) { lnsfaid_destroy(ctx); return rc; }
    ctx->comb_slot = comb_join(ctx); /* also sets ctx->comb */
    *out = ctx;
    return LNSFAID_OK;
}

extern "C" int lnsfaid_set_cfg(lnsfaid_ctx* ctx, const lnsfaid_cfg* cfg)
{
    if (!ctx || !cfg) return LNSFAID_E_INVAL;
    LfDevCfg n;
    int rc = build_cfg(cfg, &n);
    if (rc) return rc;
    rc = check_code_for_method(&ctx->hcode, n.method);
    if (rc) return rc;
    /* the reference re-reads Profile.txt in every decode call (CDecoder_FAID.cpp:178-179), so a drop-in binding calls this once
     * per call with what is almost always the same configuration: nothing to do then (no synchronisation, no upload) */
    if (memcmp(&n, &ctx->hcfg, sizeof(n)) == 0) return LNSFAID_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (n.W != ctx->hcfg.W) { /* the bit-flipping column list depends on REGULAR_COL_WEIGHT */
        build_wcols(&ctx->hcode, n.W);
        HIP_TRY(hipMemcpy(ctx->d_code, &ctx->hcode, sizeof(LfDevCode), hipMemcpyHostToDevice));
    }
    ctx->hcfg = n;
    HIP_TRY(hipMemcpy(ctx->d_cfg, &ctx->hcfg, sizeof(LfDevCfg), hipMemcpyHostToDevice));
    return LNSFAID_OK;
}

/* the combiner's pool context takes the configuration of the batch it is about to decode (validated when the member built it) */
static void apply_devcfg(lnsfaid_ctx* ctx, const LfDevCfg& n)
{
    (void)hipStreamSynchronize(ctx->stream);
    ctx->hcfg = n; /* (same REGULAR_COL_WEIGHT as the pool's code: members are matched on the whole LfDevCode) */
    (void)hipMemcpy(ctx->d_cfg, &ctx->hcfg, sizeof(LfDevCfg), hipMemcpyHostToDevice);
}

/* ---- the hot path ------------------------------------------------------------------------------------ */
/* The four-rows-per-lane kernel (lnsfaid_kernel4.hip) covers DecodeMethods 1..5 with FAID tables that are uniform over the
 * weight classes and non-decreasing (OMS has no table), and DecodeMethod 0 with Factor_1 == Factor_2 >= 15 (sw_nms_fits); it
 * needs max degree <= 24 like the other one; everything else runs on the two-rows-per-lane kernel. */
static bool kernel4_possible(const lnsfaid_ctx* ctx)
{
    const int m = ctx->hcfg.method;
    if (m < 0 || m > 5) return false;
    if (m == 0) return ctx->hcfg.nms_fits != 0; /* one factor, at most 16 levels (the usual normalisation factors) */
    if ((m == 2 || m == 5) && !ctx->hcfg.uniform_w) return false;
    return true;
}
static bool use_kernel4(const lnsfaid_ctx* ctx)
{
    if (ctx->hcfg.method == 2 && ctx->hcfg.ef >= 1) return true; /* not built for the other kernel (build_cfg made sure it applies) */
    if (ctx->rows_per_lane == 2) return false;
    return kernel4_possible(ctx);
}

extern "C" int lnsfaid_select_kernel(lnsfaid_ctx* ctx, int32_t rows_per_lane)
{
    if (!ctx || (rows_per_lane != 0 && rows_per_lane != 2 && rows_per_lane != 4)) return LNSFAID_E_INVAL;
    if (rows_per_lane == 4 && !kernel4_possible(ctx)) return LNSFAID_E_INVAL;
    if (rows_per_lane == 2 && ctx->hcfg.method == 2 && ctx->hcfg.ef >= 1) return LNSFAID_E_INVAL;
    ctx->rows_per_lane = rows_per_lane;
    return LNSFAID_OK;
}

extern "C" int lnsfaid_kernel_rows_per_lane(const lnsfaid_ctx* ctx) { return ctx ? (use_kernel4(ctx) ? 4 : 2) : LNSFAID_E_INVAL; }

/* Two wavefronts per codeword (lnsfaid_kernel5.hip): the four-rows kernel's configurations without DecodeMethod 0 and without the
 * erasing instance of EF_ELIMINATION 2; messages streamed through HBM. */
static bool kernel5_possible(const lnsfaid_ctx* ctx)
{
    const int m = ctx->hcfg.method;
    /* (the two waves exchange 7 dwords per lane through the LDS of the hard-decision plane: n_words words) */
    return kernel4_possible(ctx) && m >= 1 && m <= 5 && !(m == 2 && ctx->hcfg.ef == 2) && ctx->hcode.n_words >= 7 * 64;
}
static bool use_kernel5(const lnsfaid_ctx* ctx) { return ctx->waves_per_cw == 2 && use_kernel4(ctx) && kernel5_possible(ctx); }

extern "C" int lnsfaid_select_waves(lnsfaid_ctx* ctx, int32_t waves_per_codeword)
{
    if (!ctx || waves_per_codeword < 0 || waves_per_codeword > 2) return LNSFAID_E_INVAL;
    if (waves_per_codeword == 2 && !(use_kernel4(ctx) && kernel5_possible(ctx))) return LNSFAID_E_INVAL;
    ctx->waves_per_cw = waves_per_codeword;
    return LNSFAID_OK;
}

extern "C" int lnsfaid_kernel_waves(const lnsfaid_ctx* ctx) { return ctx ? (use_kernel5(ctx) ? 2 : 1) : LNSFAID_E_INVAL; }

/* Where the four-rows kernel keeps the compressed check-to-variable messages between layers: in registers (codes of up to
 * lf_decode4_rm_layers() layers; not built for the erasing instance of EF_ELIMINATION 2) or streamed through HBM. */
static bool msg_registers_possible(const lnsfaid_ctx* ctx)
{
    if (ctx->hcfg.method == 0) return false; /* NMS: the 16-level minimum search leaves no room for them */
    return ctx->hcode.nbr <= lf_decode4_rm_layers() && !(ctx->hcfg.method == 2 && ctx->hcfg.ef == 2);
}
static bool use_msg_registers(const lnsfaid_ctx* ctx)
{
    if (!msg_registers_possible(ctx) || use_kernel5(ctx)) return false;
    return ctx->msg_store != LNSFAID_MSG_HBM;
}

/* The rotation-free layer step (lnsfaid_kernel4z.hip): the group rule's int8 kernel with the messages in registers, DecodeMethods
 * 1..5, on a code with at least one layer that leads with a group of four zero-shift edges its degree has an instance for. */
static int layer_zero_groups(const lnsfaid_ctx* ctx, int br) { return (ctx->hcode.zinst[br] >> 8) & 0xff; }
static bool zero_shift_possible(const lnsfaid_ctx* ctx)
{
    if (!use_kernel4(ctx) || use_kernel5(ctx) || !use_msg_registers(ctx)) return false;
    if (ctx->hcfg.method < 1 || ctx->hcfg.method > 5) return false; /* what lnsfaid_kernel4z / 4s / 4w.hip are built for */
    for (int br = 0; br < ctx->hcode.nbr; ++br)
        if (layer_zero_groups(ctx, br) >= 1) return true;
    return false;
}
static bool use_zero_shift(const lnsfaid_ctx* ctx) { return ctx->zero_shift != LNSFAID_ZERO_SHIFT_OFF && zero_shift_possible(ctx); }

/* The layer-static kernel (lnsfaid_kernel4s.hip) takes the rotation-free kernel's place where the context's code is the built-in
 * 50G-PON code, entry by entry of the zero-first edge tables (the kernel holds them as compile-time constants). */
static bool static_layers_possible(const lnsfaid_ctx* ctx)
{
    if (ctx->static_code < 0) ctx->static_code = lf_decode4s_matches(&ctx->hcode); /* (the tables never change after creation) */
    return ctx->static_code == 1 && zero_shift_possible(ctx);
}
static bool use_static_layers(const lnsfaid_ctx* ctx)
{
    return use_zero_shift(ctx) && ctx->zero_shift != LNSFAID_ZERO_SHIFT_LOOP && static_layers_possible(ctx);
}
/* The window-free kernel (lnsfaid_kernel4w.hip) takes the layer-static kernel's place where the configuration cannot open the
 * error-floor window: nombre_iterations <= floor_iter_thresh never holds for a negative threshold (the shipped DecodeMethod 2). */
static bool use_window_free(const lnsfaid_ctx* ctx)
{
    return use_static_layers(ctx) && ctx->zero_shift != LNSFAID_ZERO_SHIFT_WINDOWED && ctx->hcfg.floor_iter_thresh < 0;
}

/* The edge-word kernel (lnsfaid_kernel4e.hip) takes the window-free kernel's place unless it is switched off. */
static bool use_edge_words(const lnsfaid_ctx* ctx) { return ctx->edge_words != 0 && use_window_free(ctx); }

extern "C" int lnsfaid_select_edge_words(lnsfaid_ctx* ctx, int32_t on)
{
    if (!ctx || on < 0 || on > 1) return LNSFAID_E_INVAL;
    ctx->edge_words = on;
    return LNSFAID_OK;
}

extern "C" int lnsfaid_edge_words(const lnsfaid_ctx* ctx)
{
    if (!ctx) return LNSFAID_E_INVAL;
    return use_edge_words(ctx) ? 1 : 0;
}

extern "C" int lnsfaid_select_zero_shift(lnsfaid_ctx* ctx, int32_t mode)
{
    if (!ctx || mode < 0 || mode > LNSFAID_ZERO_SHIFT_WINDOWED) return LNSFAID_E_INVAL;
    if ((mode == LNSFAID_ZERO_SHIFT_ON || mode == LNSFAID_ZERO_SHIFT_LOOP) && !zero_shift_possible(ctx)) return LNSFAID_E_INVAL;
    if ((mode == LNSFAID_ZERO_SHIFT_STATIC || mode == LNSFAID_ZERO_SHIFT_WINDOWED) && !static_layers_possible(ctx)) return LNSFAID_E_INVAL;
    ctx->zero_shift = mode;
    return LNSFAID_OK;
}

extern "C" int lnsfaid_zero_shift_groups(const lnsfaid_ctx* ctx, int32_t* groups, int32_t n)
{
    if (!ctx || n < 0 || (n > 0 && !groups)) return LNSFAID_E_INVAL;
    const bool on = use_zero_shift(ctx);
    for (int br = 0; br < n; ++br) groups[br] = (on && br < ctx->hcode.nbr) ? layer_zero_groups(ctx, br) : 0;
    return on ? (use_static_layers(ctx) ? 2 : 1) : 0;
}

extern "C" int lnsfaid_window_free(const lnsfaid_ctx* ctx)
{
    if (!ctx) return LNSFAID_E_INVAL;
    return use_window_free(ctx) ? 1 : 0;
}

extern "C" int lnsfaid_code_zero_shift_order(const lnsfaid_code* code, int32_t* groups, int32_t* order)
{
    LfDevCode* dc = new (std::nothrow) LfDevCode;
    if (!dc) return LNSFAID_E_NOMEM;
    const int rc = build_code(code, dc);
    if (rc) { delete dc; return rc; }
    const int nbr = dc->nbr;
    for (int br = 0; br < nbr; ++br) {
        int n_zero = 0;
        while (n_zero < dc->deg[br] && dc->zs4tab[br][n_zero] == 0u) ++n_zero;
        if (groups) groups[br] = n_zero / 4;
        for (int j = 0; order && j < LF_MAX_DEG; ++j) {
            order[br * LF_MAX_DEG + j] = -1;
            for (int i = 0; j < dc->deg[br] && i < dc->deg[br]; ++i) /* a block column occurs once per layer */
                if (dc->cbtab[br][i] == dc->zcbtab[br][j] && dc->s4tab[br][i] == dc->zs4tab[br][j]) order[br * LF_MAX_DEG + j] = i;
        }
    }
    delete dc;
    return nbr;
}

extern "C" int lnsfaid_code_bf_walk(const lnsfaid_code* code, int32_t col_weight, uint32_t* full, uint32_t* flipped, uint32_t* fixed, int32_t* info)
{
    if (!full || !flipped || !fixed || !info || col_weight < 0 || col_weight > LF_MAX_COLW) return LNSFAID_E_INVAL;
    LfDevCode* dc = new (std::nothrow) LfDevCode;
    if (!dc) return LNSFAID_E_NOMEM;
    const int rc = build_code(code, dc);
    if (rc) { delete dc; return rc; }
    build_wcols(dc, col_weight);
    const int nbr = dc->nbr;
    for (int br = 0; br < nbr; ++br)
        for (int k = 0; k < 8; ++k) {
            for (int j = 0; j < LF_MAX_DEG; ++j) {
                uint32_t* o = full + ((br * LF_MAX_DEG + j) * 8 + k) * 2, *x = fixed + ((br * LF_MAX_DEG + j) * 8 + k) * 2;
                o[0] = dc->synw[br][j][k].x; o[1] = dc->synw[br][j][k].y;
                x[0] = dc->synw_c[br][j][k].x; x[1] = dc->synw_c[br][j][k].y;
            }
            for (int j = 0; j < 2 * LF_BFW_JP; ++j) {
                uint32_t* o = flipped + ((br * 2 * LF_BFW_JP + j) * 8 + k) * 2;
                o[0] = dc->synw_w[br][j][k].x; o[1] = dc->synw_w[br][j][k].y;
            }
        }
    info[0] = (int32_t)lf_lds_off_hard(dc->n_var);
    info[1] = (int32_t)lf_lds_off_zero(dc->n_var, dc->n_words, dc->p_words);
    info[2] = 2 * LF_BFW_JP;
    info[3] = dc->bfw_fits;
    info[4] = dc->n_wcols;
    delete dc;
    return nbr;
}

/* Under the per-codeword rule (lnsfaid_kernel4cw.hip) the four-rows kernel's configurations have an instance each, with the
 * same message store; the two-rows kernel and the two-waves kernel have none. */
static bool cw_possible(const lnsfaid_ctx* ctx) { return ctx->waves_per_cw != 2 && use_kernel4(ctx); }

/* The packed decoders (lnsfaid_kernel4p.hip) are twins of the one-wave four-rows kernels; the other configurations decode
 * packed I/O through conversion kernels around the int8 decode. */
static bool packed_kernel(const lnsfaid_ctx* ctx) { return use_kernel4(ctx) && !use_kernel5(ctx); }

/* ---- select, check, launch: the one path from a context to a running decode kernel ----
 * The entry kinds: the two early-stop rules of the decode calls (LNSFAID_STOP_GROUP, LNSFAID_STOP_CODEWORD), the same on packed
 * I/O, and the line formats.  An instance is what a launch needs of a kernel. */
enum { LF_ENTRY_GROUP = LNSFAID_STOP_GROUP, LF_ENTRY_CW = LNSFAID_STOP_CODEWORD, LF_ENTRY_PACKED = 2 /* + rule */, LF_ENTRY_LINE = 4, LF_ENTRY_BURST };
static int decode_entry(int rule, bool packed) { return rule + (packed ? LF_ENTRY_PACKED : 0); }
struct LfInst {
    const void* fn; /* null: the configuration has no instance of this kind */
    int threads;    /* per workgroup; one workgroup per codeword */
};

/* the instance the context runs an entry kind on: the only place that asks the kernel files */
static LfInst select_kernel(const lnsfaid_ctx* ctx, int entry)
{
    const int m = ctx->hcfg.method, ef = ctx->hcfg.ef, rm = use_msg_registers(ctx) ? 1 : 0;
    LfInst k = { nullptr, lf_decode4_threads() };
    switch (entry) {
    case LF_ENTRY_PACKED + LF_ENTRY_GROUP: k.fn = lf_decode4p_func(m, ef, rm, 0); break;
    case LF_ENTRY_PACKED + LF_ENTRY_CW: k.fn = lf_decode4p_func(m, ef, rm, 1); break;
    case LF_ENTRY_CW: if (cw_possible(ctx)) k.fn = lf_decode4cw_func(m, ef, rm); break;
    case LF_ENTRY_LINE: k.fn = lf_decode4l_func(m, ef, rm); break;
    case LF_ENTRY_BURST: k.fn = lf_decode4b_func(m, ef, rm); break;
    default: /* the group rule on int8 I/O: every kernel has it */
        if (use_kernel5(ctx)) { k.fn = lf_decode5_func(m); k.threads = lf_decode5_threads(); }
        else if (use_edge_words(ctx)) k.fn = lf_decode4e_func(m);
        else if (use_window_free(ctx)) k.fn = lf_decode4w_func(m);
        else if (use_static_layers(ctx)) k.fn = lf_decode4s_func(m);
        else if (use_zero_shift(ctx)) k.fn = lf_decode4z_func(m);
        else if (use_kernel4(ctx)) k.fn = lf_decode4_func(m, ef, rm);
        else { k.fn = lf_decode_func(m, ctx->hcfg.uniform_w); k.threads = lf_decode_threads(); }
    }
    return k;
}

extern "C" int lnsfaid_select_message_store(lnsfaid_ctx* ctx, int32_t where)
{
    if (!ctx || where < 0 || where > LNSFAID_MSG_HBM) return LNSFAID_E_INVAL;
    if (where == LNSFAID_MSG_REGISTERS && !msg_registers_possible(ctx)) return LNSFAID_E_INVAL;
    ctx->msg_store = where;
    return LNSFAID_OK;
}

extern "C" int lnsfaid_message_store(const lnsfaid_ctx* ctx)
{
    if (!ctx) return LNSFAID_E_INVAL;
    if (!use_kernel4(ctx)) return LNSFAID_MSG_HBM; /* the two-rows kernel always streams them */
    return use_msg_registers(ctx) ? LNSFAID_MSG_REGISTERS : LNSFAID_MSG_HBM;
}

/* Build-time properties of the kernel instance the context is about to launch, looked at once per instance:
 *  - it must have no static LDS: the layer steps address En by its LDS offset, so the dynamic segment has to start at 0
 *    (adding a __shared__ variable to a decode kernel would otherwise corrupt En silently);
 *  - how many of its workgroups a CU holds.  The decoders are sized so that LDS alone decides that (50G-PON: 20 424 B per
 *    codeword, 8 per CU); one more register or LDS word in the wrong place halves it, which costs ~40 % of the throughput and
 *    nothing else would show.  Recorded for lnsfaid_kernel_residency, printed under LNSFAID_TRACE.  The LDS limit is capped at
 *    the 8 workgroups per CU the kernels' launch bounds are written for: the image of a narrower code would let more of them in,
 *    but their register budget stops at 8 by design, and (8, 20) would read as residency lost to registers. */
#define LF_BUILT_RESIDENCY 8
/* Selects the instance of an entry kind into *inst and checks it: what a caller launches is what was looked at.  (The line
 * formats' kernels get the first look only: their calls have no residency to report.) */
static int kernel_check(lnsfaid_ctx* ctx, int entry, LfInst* inst)
{
    *inst = select_kernel(ctx, entry);
    const void* fn = inst->fn;
    const int threads = inst->threads;
    const bool group_rule = entry == LF_ENTRY_GROUP || entry == LF_ENTRY_PACKED + LF_ENTRY_GROUP;
    if (!fn) return group_rule ? LNSFAID_E_INTERNAL : LNSFAID_E_INVAL; /* no per-codeword instance */
    if (fn == ctx->checked_fn[entry]) return LNSFAID_OK;
    hipFuncAttributes at;
    HIP_TRY(hipFuncGetAttributes(&at, fn));
    if (at.sharedSizeBytes != 0) {
        snprintf(g_hip_err, sizeof(g_hip_err), "%sdecode kernel has %zu bytes of static LDS: its En image would not start at LDS offset 0",
                 entry == LF_ENTRY_LINE ? "line " : entry == LF_ENTRY_BURST ? "burst " : "", (size_t)at.sharedSizeBytes);
        return LNSFAID_E_INTERNAL;
    }
    if (entry >= LF_ENTRY_LINE) {
        ctx->checked_fn[entry] = fn;
        return LNSFAID_OK;
    }
    int wg = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&wg, fn, threads, ctx->lds_bytes));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, ctx->device));
    const size_t lds_cu = prop.maxSharedMemoryPerMultiProcessor ? prop.maxSharedMemoryPerMultiProcessor : 160 * 1024;
    const size_t gran = 512; /* LDS allocation granularity */
    int by_lds = (int)(lds_cu / ((ctx->lds_bytes + gran - 1) / gran * gran));
    const int by_waves = 32 / ((threads + 63) / 64); /* 32 wave slots per CU */
    if (by_lds > by_waves) by_lds = by_waves;
    if (by_lds > LF_BUILT_RESIDENCY) by_lds = LF_BUILT_RESIDENCY;
    ctx->checked_fn[entry] = fn; ctx->resident_wg[entry] = wg; ctx->lds_wg[entry] = by_lds;
    static const bool trace = getenv("LNSFAID_TRACE") != nullptr;
    if (trace)
        fprintf(stderr, "[lnsfaid] decode kernel: %d threads, %d VGPRs, %zu B LDS per workgroup, %d workgroups per CU (LDS alone: %d)%s\n",
                threads, at.numRegs, ctx->lds_bytes, wg, by_lds, wg < by_lds ? "  ** residency lost **" : "");
    return LNSFAID_OK;
}

extern "C" int lnsfaid_kernel_residency(lnsfaid_ctx* ctx, int32_t* workgroups_per_cu, int32_t* lds_limit)
{
    if (!ctx) return LNSFAID_E_INVAL;
    HIP_TRY(hipSetDevice(ctx->device));
    LfInst k;
    const int rc = kernel_check(ctx, decode_entry(ctx->early_stop, false), &k);
    if (rc) return rc;
    if (workgroups_per_cu) *workgroups_per_cu = ctx->resident_wg[ctx->early_stop];
    if (lds_limit) *lds_limit = ctx->lds_wg[ctx->early_stop];
    return LNSFAID_OK;
}

/* one workgroup per codeword on a checked instance; args: the kernel's argument struct */
static hipError_t launch_decode(const lnsfaid_ctx* ctx, const LfInst& k, const void* args, size_t n_cw)
{
    void* kargs[] = { (void*)args };
    return hipLaunchKernel(k.fn, dim3((unsigned)n_cw), dim3((unsigned)k.threads), kargs, ctx->lds_bytes, ctx->stream);
}

/* one launch, one wait: the calls without a chain (the per-codeword rule, the line formats).  what: the call's name in the trace */
static int launch_decode_timed(lnsfaid_ctx* ctx, const LfInst& k, const void* args, size_t n_cw, const char* what)
{
    static const bool trace = getenv("LNSFAID_TRACE") != nullptr;
    HIP_TRY(hipEventRecord(ctx->ev_chain[0], ctx->stream));
    HIP_TRY(launch_decode(ctx, k, args, n_cw));
    HIP_TRY(hipEventRecord(ctx->ev_chain[1], ctx->stream));
    { const int rcw = stream_wait(ctx); if (rcw) return rcw; }
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ctx->ev_chain[0], ctx->ev_chain[1]));
    ctx->kernel_ms += ms;
    ctx->kernel_launches += 1;
    if (trace) fprintf(stderr, "[lnsfaid] %s launch: %.3f ms, %zu codewords\n", what, ms, n_cw);
    return LNSFAID_OK;
}

/* status_preloaded: ctx->d_status[0] already holds the decision point of every codeword (the call combiner marks the groups
 * that take no part in a batch as finished); otherwise every codeword is fresh */
/* packed: the buffers are llr4 / bits and the packed twin of the four-rows kernel runs (packed_kernel() must hold) */
static int decode_device_impl(lnsfaid_ctx* ctx, const int8_t* d_fixInput, size_t n_groups, int8_t* d_decodedBits,
                              lnsfaid_group_stats* d_stats, bool status_preloaded, bool packed = false);
static int decode_cw_device_impl(lnsfaid_ctx* ctx, const int8_t* d_fixInput, size_t n_groups, int8_t* d_decodedBits,
                                 lnsfaid_group_stats* d_stats, lnsfaid_codeword_stats* d_cw_stats, bool status_preloaded,
                                 bool packed = false);
/* the context's rule, or the per-codeword one (lnsfaid_decode_codewords*) */
static int decode_device_rule(lnsfaid_ctx* ctx, const int8_t* d_fixInput, size_t n_groups, int8_t* d_decodedBits, lnsfaid_group_stats* d_stats,
                              lnsfaid_codeword_stats* d_cw_stats, int rule, bool status_preloaded)
{
    if (rule == LNSFAID_STOP_CODEWORD)
        return decode_cw_device_impl(ctx, d_fixInput, n_groups, d_decodedBits, d_stats, d_cw_stats, status_preloaded);
    return decode_device_impl(ctx, d_fixInput, n_groups, d_decodedBits, d_stats, status_preloaded);
}
extern "C" int lnsfaid_decode_device(lnsfaid_ctx* ctx, const int8_t* d_fixInput, size_t n_groups, int8_t* d_decodedBits,
                                     lnsfaid_group_stats* d_stats)
{
    if (!ctx) return LNSFAID_E_INVAL;
    return decode_device_rule(ctx, d_fixInput, n_groups, d_decodedBits, d_stats, nullptr, ctx->early_stop, false);
}
extern "C" int lnsfaid_decode_codewords_device(lnsfaid_ctx* ctx, const int8_t* d_fixInput, size_t n_groups, int8_t* d_decodedBits,
                                               lnsfaid_codeword_stats* d_cw_stats)
{
    return decode_cw_device_impl(ctx, d_fixInput, n_groups, d_decodedBits, nullptr, d_cw_stats, false);
}

extern "C" int lnsfaid_set_early_stop(lnsfaid_ctx* ctx, int32_t rule)
{
    if (!ctx || (rule != LNSFAID_STOP_GROUP && rule != LNSFAID_STOP_CODEWORD)) return LNSFAID_E_INVAL;
    ctx->early_stop = rule;
    return LNSFAID_OK;
}
extern "C" int lnsfaid_early_stop(const lnsfaid_ctx* ctx) { return ctx ? ctx->early_stop : LNSFAID_E_INVAL; }

/* Per-codeword rule (lnsfaid_kernel4cw.hip): every codeword runs to its own stop in ONE launch, so there is no chain, no status
 * double buffer and no "codewords left" counter - one launch, one wait.  The group records are maxima, taken with atomics over
 * zeroed words.  status_preloaded: ctx->d_status[0] marks the groups of a combiner batch that take no part (LF_DONE). */
static int decode_cw_device_impl(lnsfaid_ctx* ctx, const int8_t* d_fixInput, size_t n_groups, int8_t* d_decodedBits,
                                 lnsfaid_group_stats* d_stats, lnsfaid_codeword_stats* d_cw_stats, bool status_preloaded, bool packed)
{
    if (!ctx || (n_groups && (!d_fixInput || !d_decodedBits))) return LNSFAID_E_INVAL;
    if (n_groups > ctx->max_groups) return LNSFAID_E_INVAL;
    if (!cw_possible(ctx)) return LNSFAID_E_INVAL;
    if (n_groups == 0) return LNSFAID_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    LfInst k;
    {
        const int rc = kernel_check(ctx, decode_entry(LNSFAID_STOP_CODEWORD, packed), &k);
        if (rc) return rc;
    }
    const size_t n_cw = n_groups * LNSFAID_GROUP;
    LfCwArgs a;
    a.code = ctx->d_code; a.cfg = ctx->d_cfg;
    a.fix_input = d_fixInput; a.decoded = d_decodedBits;
    a.st_rows = ctx->d_rows;
    a.skip = status_preloaded ? ctx->d_status[0] : nullptr;
    a.stats = d_stats; a.cw_stats = d_cw_stats; a.n_cw = (int32_t)n_cw;
    if (d_stats) HIP_TRY(hipMemsetAsync(d_stats, 0, n_groups * sizeof(lnsfaid_group_stats), ctx->stream));
    return launch_decode_timed(ctx, k, &a, n_cw, "per-codeword");
}

static int decode_device_impl(lnsfaid_ctx* ctx, const int8_t* d_fixInput, size_t n_groups, int8_t* d_decodedBits,
                              lnsfaid_group_stats* d_stats, bool status_preloaded, bool packed)
{
    if (!ctx || (n_groups && (!d_fixInput || !d_decodedBits))) return LNSFAID_E_INVAL;
    if (n_groups > ctx->max_groups) return LNSFAID_E_INVAL;
    if (n_groups == 0) return LNSFAID_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    LfInst k; /* picked and checked once per call: every launch of the chain below runs it */
    {
        const int rc = kernel_check(ctx, decode_entry(LNSFAID_STOP_GROUP, packed), &k);
        if (rc) return rc;
    }
    const size_t n_cw = n_groups * LNSFAID_GROUP;
#ifdef LF4_LIVE_PROOF /* experiment build only (lnsfaid_kernel4.hip publish_pass) */
    HIP_TRY(hipMemsetAsync(ctx->d_live, 0, n_cw * sizeof(int32_t), ctx->stream));
#endif

    LfKernelArgs a;
    a.code = ctx->d_code; a.cfg = ctx->d_cfg;
    a.fix_input = d_fixInput; a.decoded = d_decodedBits;
    a.st_en = ctx->d_en; a.st_rows = ctx->d_rows; a.st_bits = ctx->d_bits; a.st_lane = ctx->d_lane;
    a.live = ctx->d_live; a.stats = d_stats; a.n_cw = (int32_t)n_cw;

    /* Every launch moves each unfinished group's front forward or finishes it; the time line has max_iter + max_bf + 1
     * points and a group needs at most two launches per point.  How many launches a batch takes is data dependent (one when
     * nothing converges, three or four with early stop) and only known from the "codewords left" counter of the previous
     * launch, so a host round trip per launch would sit between them - a quarter of the time of a one-group call.  Instead the
     * launches the PREVIOUS batch needed are queued back to back (a launch on a finished batch is a grid of immediate exits,
     * microseconds), their counters are read in one go, and only a batch that needs more continues one launch at a time.
     * No memset in front: the first launch takes "every codeword fresh" from a null status pointer, and the counters are
     * running sums of which the host remembers the last value it saw. */
    const long max_launches = 2L * ((long)ctx->hcfg.max_iter + ctx->hcfg.max_bf + 2) + 2 + LF_MAX_CHAIN;
    static const bool trace = getenv("LNSFAID_TRACE") != nullptr; /* read once: per-launch timing on stderr */
    int cur = 0;
    long launch = 0, needed = 0;
    bool done = false;
    while (!done) {
        if (launch >= max_launches) return LNSFAID_E_INTERNAL;
        int chain = launch == 0 ? ctx->predicted_launches : 1;
        if (chain < 1) chain = 1;
        if (chain > LF_MAX_CHAIN) chain = LF_MAX_CHAIN;
        for (int j = 0; j < chain; ++j) {
            a.status_cur = (launch + j == 0 && !status_preloaded) ? nullptr : ctx->d_status[cur];
            a.status_next = ctx->d_status[cur ^ 1];
            a.remaining = ctx->d_remaining + j;
            HIP_TRY(hipEventRecord(ctx->ev_chain[j], ctx->stream));
            HIP_TRY(launch_decode(ctx, k, &a, n_cw));
            cur ^= 1;
        }
        HIP_TRY(hipEventRecord(ctx->ev_chain[chain], ctx->stream));
        HIP_TRY(hipMemcpyAsync(ctx->h_remaining, ctx->d_remaining, (size_t)chain * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        { const int rcw = stream_wait(ctx); if (rcw) return rcw; }
        for (int j = 0; j < chain; ++j) {
            const uint32_t left = ctx->h_remaining[j] - ctx->slot_seen[j]; /* running counter, modulo 2^32 */
            ctx->slot_seen[j] = ctx->h_remaining[j];
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, ctx->ev_chain[j], ctx->ev_chain[j + 1]));
            ctx->kernel_ms += ms;
            ctx->kernel_launches += 1;
            if (trace) fprintf(stderr, "[lnsfaid] launch %ld: %.3f ms, %u codewords left%s\n", launch + j, ms, left, done ? " (queued ahead, batch already complete)" : "");
            if (!done && left == 0) { done = true; needed = launch + j + 1; }
        }
        launch += chain;
    }
    ctx->predicted_launches = (int)needed;
    return LNSFAID_OK;
}

static int ensure_io(lnsfaid_ctx* ctx)
{
    if (ctx->d_io_in) return LNSFAID_OK;
    const size_t bytes = ctx->max_groups * LNSFAID_GROUP * (size_t)ctx->n_var;
    HIP_TRY(hipMalloc(&ctx->d_io_in, bytes));
    HIP_TRY(hipMalloc(&ctx->d_io_out, bytes));
    HIP_TRY(hipMalloc(&ctx->d_io_stats, ctx->max_groups * sizeof(lnsfaid_group_stats)));
    return LNSFAID_OK;
}

/* ---- the call combiner: many contexts, one group per call -> few launches ------------------------------------------------
 * The reference decodes ONE group of 32 frames per call from T worker threads, each owning a CLDPC (reference
 * CSimulate.cpp:136-164, main.cpp:164-172), and the drop-in binding gives every CLDPC its own context.
 * Taken literally that is T streams with a 32-wave launch each: the runtime multiplexes the streams onto a handful of hardware
 * queues, so only a few of those launches are on the chip at a time, and every call pays its own copies, launches and waits
 * (measured, profiles/r03_dropin: 64 threads reach 1.5 Gb/s of 70).  So contexts of ONE group on the same device that decode
 * the same code share a combiner: a call copies its fixInput into a slot of a pinned staging area and sleeps; one worker thread
 * per device gathers the calls that arrive within LF_COMB_WINDOW_US (or until every member has one pending), moves their slots
 * to the device in one copy, decodes them in ONE launch sequence on a pool context of LF_COMB_SLOTS groups - groups without a
 * pending call are marked finished, their workgroups exit at once -, copies the decisions back in one copy and wakes the
 * callers, each of which copies its slot out.  Results are those of the direct path bit for bit (groups never interact).
 * A context that is alone on its device, or whose kernel / message-store selection was changed by hand, takes the direct path;
 * LNSFAID_COALESCE=0 switches the combiner off. */
#define LF_COMB_SLOTS 128
#define LF_COMB_QUIET_US 150  /* a batch is closed when no further call has arrived for this long ...                      */
#define LF_COMB_WINDOW_US 1500 /* ... or this long after its first call, or as soon as every member has a call pending       */
#define LF_COMB_DEVICES 16
#define LF_COMB_WORKERS 4     /* upper limit of the batches in flight (LNSFAID_COMB_WORKERS, default 2): the transfers of one overlap
                               * the decode of the others */
#define LF_COMB_MIN_MEMBERS 4 /* fewer one-group contexts than this on a device: each keeps to its own stream (measured faster) */
enum { LF_SLOT_FREE = 0, LF_SLOT_IDLE, LF_SLOT_PENDING, LF_SLOT_RUNNING, LF_SLOT_DONE };
struct LfSlot {
    int state = LF_SLOT_FREE;
    int rc = 0;
    LfDevCfg cfg;
    int rule = LNSFAID_STOP_GROUP; /* early-stop rule of the call: part of the batch key with cfg */
    lnsfaid_group_stats stats;
};
struct LfCombiner {
    int device = 0;
    std::mutex m;
    std::condition_variable cv_work, cv_done;
    std::thread worker[LF_COMB_WORKERS];
    bool stop = false, dead = false;
    bool gathering = false;                        /* one worker at a time collects a batch */
    int running = 0;                               /* calls claimed by a worker and not yet answered */
    lnsfaid_ctx* pool[LF_COMB_WORKERS] = {};       /* one per worker, created for its first batch */
    LfDevCode code;              /* what every member decodes (incl. the bit-flipping column list) */
    size_t group_bytes = 0;
    int8_t *h_in = nullptr, *h_out = nullptr; /* pinned, LF_COMB_SLOTS groups each; allocated when the second member joins */
    int8_t *d_in_map = nullptr, *d_out_map = nullptr; /* the same memory as the device sees it (zero copy), null if not mapped */
    int32_t* h_status = nullptr;              /* pinned, LF_COMB_WORKERS x LF_COMB_SLOTS * 32 words */
    lnsfaid_group_stats* h_stats = nullptr;   /* pinned, LF_COMB_WORKERS x LF_COMB_SLOTS */
    LfSlot slots[LF_COMB_SLOTS];
    int members = 0, pending = 0;
    char err[256] = "";              /* lnsfaid_last_hip_error text of the last failed batch (the worker's is thread-local) */
    uint64_t batches = 0, calls = 0; /* statistics (LNSFAID_TRACE at shutdown) */
    double gather_ms = 0, device_ms = 0;
};
static std::mutex g_comb_mutex;
static LfCombiner* g_comb[LF_COMB_DEVICES] = {};

static int comb_workers()
{
    static const int n = [] {
        const char* e = getenv("LNSFAID_COMB_WORKERS");
        const int v = e ? atoi(e) : 2;
        return v < 1 ? 1 : (v > LF_COMB_WORKERS ? LF_COMB_WORKERS : v);
    }();
    return n;
}

/* into how many batches the members' calls are cut (>= the number of workers; LNSFAID_COMB_BATCHES): more, smaller batches than
 * workers keep the launches out of phase - a worker that comes back from the device finds the next batch waiting */
static int comb_batches()
{
    static const int v = [] {
        const char* e = getenv("LNSFAID_COMB_BATCHES");
        const int n = e ? atoi(e) : 0;
        return n > 64 ? 64 : n;
    }();
    return v > comb_workers() ? v : comb_workers();
}

static bool comb_enabled()
{
    static const char* e = getenv("LNSFAID_COALESCE");
    return !(e && e[0] == '0');
}

static void apply_devcfg(lnsfaid_ctx* ctx, const LfDevCfg& n); /* pool only: no validation, same code */

static void comb_run_batch(LfCombiner* cb, int w, const int* batch, int nb)
{
    lnsfaid_ctx* P = cb->pool[w];
    int32_t* h_status = cb->h_status + (size_t)w * LF_COMB_SLOTS * LNSFAID_GROUP;
    lnsfaid_group_stats* h_stats = cb->h_stats + (size_t)w * LF_COMB_SLOTS;
    int rc = LNSFAID_OK;
    auto fail = [&](hipError_t e, const char* what) { if (rc == LNSFAID_OK && e != hipSuccess) rc = hip_fail(e, what); };
    int lo = LF_COMB_SLOTS, hi = -1;
    for (int i = 0; i < nb; ++i) { lo = batch[i] < lo ? batch[i] : lo; hi = batch[i] > hi ? batch[i] : hi; }
    const size_t n = (size_t)hi + 1;
    for (size_t g = 0; g < n; ++g) { /* groups without a call in this batch: finished before they start */
        bool active = false;
        for (int i = 0; i < nb; ++i) active = active || (size_t)batch[i] == g;
        for (int l = 0; l < LNSFAID_GROUP; ++l) h_status[g * LNSFAID_GROUP + l] = active ? 0 : LF_DONE;
    }
    fail(hipSetDevice(cb->device), "hipSetDevice");
    if (rc == LNSFAID_OK && memcmp(&P->hcfg, &cb->slots[batch[0]].cfg, sizeof(LfDevCfg)) != 0) apply_devcfg(P, cb->slots[batch[0]].cfg);
    const size_t gb = cb->group_bytes, span = (size_t)(hi - lo + 1);
    fail(hipMemcpyAsync(P->d_status[0], h_status, n * LNSFAID_GROUP * sizeof(int32_t), hipMemcpyHostToDevice, P->stream), "status upload");
    /* The staging area is pinned, device-mapped host memory.  zero copy: the kernel reads every LLR once (input staging) and
     * writes every decision once, so it can do both straight over PCIe - no separate copy phases in front of and behind the
     * launch, and the transfers of one batch run under the compute of the other.  LNSFAID_COMB_COPY=1: explicit copies. */
    static const bool copy_mode = getenv("LNSFAID_COMB_COPY") != nullptr;
    const int8_t* k_in = cb->d_in_map;
    int8_t* k_out = cb->d_out_map;
    if (copy_mode || !k_in || !k_out) {
        fail(hipMemcpyAsync(P->d_io_in + (size_t)lo * gb, cb->h_in + (size_t)lo * gb, span * gb, hipMemcpyHostToDevice, P->stream), "fixInput upload");
        k_in = P->d_io_in; k_out = P->d_io_out;
    }
    if (rc == LNSFAID_OK) rc = decode_device_rule(P, k_in, n, k_out, P->d_io_stats, nullptr, cb->slots[batch[0]].rule, true);
    if (rc == LNSFAID_OK) {
        if (k_out == P->d_io_out)
            fail(hipMemcpyAsync(cb->h_out + (size_t)lo * gb, P->d_io_out + (size_t)lo * gb, span * gb, hipMemcpyDeviceToHost, P->stream), "decodedBits download");
        fail(hipMemcpyAsync(h_stats + lo, P->d_io_stats + lo, span * sizeof(lnsfaid_group_stats), hipMemcpyDeviceToHost, P->stream), "stats download");
        if (rc == LNSFAID_OK) rc = stream_wait(P);
    }
    std::lock_guard<std::mutex> lk(cb->m);
    if (rc != LNSFAID_OK) snprintf(cb->err, sizeof(cb->err), "%s", g_hip_err);
    for (int i = 0; i < nb; ++i) {
        LfSlot& s = cb->slots[batch[i]];
        s.rc = rc;
        s.stats = h_stats[batch[i]];
        s.state = LF_SLOT_DONE;
    }
    cb->running -= nb;
    cb->batches += 1; cb->calls += (uint64_t)nb;
    cb->cv_done.notify_all();
    cb->cv_work.notify_all(); /* a gathering worker counts the calls in flight */
}

static void comb_worker(LfCombiner* cb, int w)
{
    std::unique_lock<std::mutex> lk(cb->m);
    for (;;) {
        cb->cv_work.wait(lk, [&] { return cb->stop || (cb->pending > 0 && !cb->gathering); });
        if (cb->stop) break;
        /* gather.  The decode time of a batch hardly depends on its size (a launch of 64 groups just fills the chip) and
         * LF_COMB_WORKERS batches are in flight at a time, so a batch should be a 1 / LF_COMB_WORKERS share of the members: wait
         * until that many calls are pending, or every member is accounted for (pending, or in flight with another worker), or no
         * further call has arrived for LF_COMB_QUIET_US, or LF_COMB_WINDOW_US have passed since the first one was seen */
        cb->gathering = true;
        const auto t_first = std::chrono::steady_clock::now();
        const auto deadline = t_first + std::chrono::microseconds(LF_COMB_WINDOW_US);
        for (;;) {
            const int share = (cb->members + comb_batches() - 1) / comb_batches();
            if (cb->stop || cb->pending >= share || cb->pending + cb->running >= cb->members) break;
            const int seen = cb->pending, seen_running = cb->running;
            auto quiet = std::chrono::steady_clock::now() + std::chrono::microseconds(LF_COMB_QUIET_US);
            if (quiet > deadline) quiet = deadline;
            cb->cv_work.wait_until(lk, quiet, [&] { return cb->pending != seen || cb->running != seen_running || cb->stop; });
            if (cb->pending == seen && cb->running == seen_running) break; /* quiet (or the window is over) */
        }
        if (cb->stop) { cb->gathering = false; break; }
        cb->gather_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_first).count();
        int batch[LF_COMB_SLOTS], nb = 0;
        const int cap = cb->members > 8 * comb_workers() ? (cb->members + comb_batches() - 1) / comb_batches() : LF_COMB_SLOTS;
        const LfDevCfg* cfg = nullptr; /* one configuration and one early-stop rule per batch: the first pending call's */
        int rule = LNSFAID_STOP_GROUP;
        for (int i = 0; i < LF_COMB_SLOTS && nb < cap; ++i) {
            LfSlot& s = cb->slots[i];
            if (s.state != LF_SLOT_PENDING) continue;
            if (!cfg) { cfg = &s.cfg; rule = s.rule; }
            if (memcmp(cfg, &s.cfg, sizeof(LfDevCfg)) != 0 || s.rule != rule) continue; /* next batch */
            s.state = LF_SLOT_RUNNING;
            batch[nb++] = i;
        }
        cb->pending -= nb;
        cb->running += nb;
        cb->gathering = false;
        cb->cv_work.notify_all(); /* the next batch may be gathered by another worker while this one is on the device */
        if (nb == 0) continue;
        if (!cb->pool[w]) { /* this worker's first batch: its pool context (device state for LF_COMB_SLOTS groups) */
            lk.unlock();
            int rc = LNSFAID_OK;
            lnsfaid_ctx* P = new (std::nothrow) lnsfaid_ctx();
            if (!P) rc = LNSFAID_E_NOMEM;
            if (!rc) {
                P->device = cb->device; P->max_groups = LF_COMB_SLOTS;
                P->hcode = cb->code; P->hcfg = cb->slots[batch[0]].cfg;
                g_live_contexts.fetch_add(1, std::memory_order_relaxed);
                rc = alloc_state(P);
                if (!rc) rc = ensure_io(P);
                if (rc) { lnsfaid_destroy(P); P = nullptr; }
            }
            lk.lock();
            if (rc) { /* the members fall back to their own contexts from now on */
                cb->dead = true;
                for (int i = 0; i < nb; ++i) { cb->slots[batch[i]].rc = rc; cb->slots[batch[i]].state = LF_SLOT_DONE; }
                cb->running -= nb;
                cb->cv_done.notify_all();
                continue;
            }
            cb->pool[w] = P;
        }
        lk.unlock();
        const auto t_dev = std::chrono::steady_clock::now();
        comb_run_batch(cb, w, batch, nb);
        lk.lock();
        cb->device_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_dev).count();
    }
}

/* a one-group context joins the combiner of its device (created on demand); -1: it stays on its own */
static int comb_join(lnsfaid_ctx* ctx)
{
    if (!comb_enabled() || ctx->max_groups != 1 || ctx->device < 0 || ctx->device >= LF_COMB_DEVICES) return -1;
    std::lock_guard<std::mutex> g(g_comb_mutex);
    LfCombiner* cb = g_comb[ctx->device];
    if (!cb) { /* the first one-group context of the device: a record only - staging area and worker come with the second */
        cb = new (std::nothrow) LfCombiner();
        if (!cb) return -1;
        cb->device = ctx->device;
        cb->code = ctx->hcode;
        cb->group_bytes = (size_t)LNSFAID_GROUP * (size_t)ctx->n_var;
        g_comb[ctx->device] = cb;
    }
    std::lock_guard<std::mutex> lk(cb->m);
    if (cb->dead || memcmp(&cb->code, &ctx->hcode, sizeof(LfDevCode)) != 0) return -1; /* another code: on its own */
    if (cb->members >= 1 && !cb->h_in) { /* there is something to combine from now on */
        const size_t bytes = (size_t)LF_COMB_SLOTS * cb->group_bytes;
        if (hipSetDevice(cb->device) != hipSuccess
            || hipHostMalloc((void**)&cb->h_in, bytes, hipHostMallocMapped) != hipSuccess
            || hipHostMalloc((void**)&cb->h_out, bytes, hipHostMallocMapped) != hipSuccess
            || hipHostMalloc((void**)&cb->h_status, (size_t)LF_COMB_WORKERS * LF_COMB_SLOTS * LNSFAID_GROUP * sizeof(int32_t), hipHostMallocDefault) != hipSuccess
            || hipHostMalloc((void**)&cb->h_stats, (size_t)LF_COMB_WORKERS * LF_COMB_SLOTS * sizeof(lnsfaid_group_stats), hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            if (cb->h_in) (void)hipHostFree(cb->h_in);
            if (cb->h_out) (void)hipHostFree(cb->h_out);
            if (cb->h_status) (void)hipHostFree(cb->h_status);
            if (cb->h_stats) (void)hipHostFree(cb->h_stats);
            cb->h_in = cb->h_out = nullptr; cb->h_status = nullptr; cb->h_stats = nullptr;
            cb->dead = true; /* everybody stays on the direct path */
            return -1;
        }
        if (hipHostGetDevicePointer((void**)&cb->d_in_map, cb->h_in, 0) != hipSuccess
            || hipHostGetDevicePointer((void**)&cb->d_out_map, cb->h_out, 0) != hipSuccess) {
            (void)hipGetLastError();
            cb->d_in_map = cb->d_out_map = nullptr; /* explicit copies then */
        }
        for (int w = 0; w < comb_workers(); ++w) cb->worker[w] = std::thread(comb_worker, cb, w);
    }
    for (int i = 0; i < LF_COMB_SLOTS; ++i)
        if (cb->slots[i].state == LF_SLOT_FREE) { cb->slots[i].state = LF_SLOT_IDLE; cb->members += 1; ctx->comb = cb; return i; }
    return -1; /* more contexts than slots */
}

static void comb_leave(lnsfaid_ctx* ctx, int slot)
{
    LfCombiner* cb = nullptr;
    {
        std::lock_guard<std::mutex> g(g_comb_mutex);
        cb = ctx->comb;
        if (!cb) return;
        bool last;
        {
            std::lock_guard<std::mutex> lk(cb->m);
            cb->slots[slot].state = LF_SLOT_FREE;
            cb->members -= 1;
            last = cb->members == 0;
            if (last) cb->stop = true;
            cb->cv_work.notify_all();
        }
        if (!last) return;
        if (g_comb[cb->device] == cb) g_comb[cb->device] = nullptr; /* a later context starts a new one */
    }
    for (auto& th : cb->worker) if (th.joinable()) th.join();
    static const bool trace = getenv("LNSFAID_TRACE") != nullptr;
    if (trace && cb->batches)
        fprintf(stderr, "[lnsfaid] call combiner of device %d: %llu calls in %llu batches (%.1f per batch); per batch %.3f ms gathering, %.3f ms copies + decode\n",
                cb->device, (unsigned long long)cb->calls, (unsigned long long)cb->batches, (double)cb->calls / (double)cb->batches,
                cb->gather_ms / (double)cb->batches, cb->device_ms / (double)cb->batches);
    for (auto P : cb->pool) if (P) lnsfaid_destroy(P);
    if (cb->h_in) { (void)hipHostFree(cb->h_in); (void)hipHostFree(cb->h_out); (void)hipHostFree(cb->h_status); (void)hipHostFree(cb->h_stats); }
    delete cb;
}

/* 1: decoded through the combiner (*rc_out = result); 0: not applicable now, take the direct path */
static int comb_decode(lnsfaid_ctx* ctx, const int8_t* fixInput, int8_t* decodedBits, lnsfaid_group_stats* stats, int rule, int* rc_out)
{
    if (ctx->comb_slot < 0 || ctx->rows_per_lane != 0 || ctx->msg_store != 0 || ctx->waves_per_cw != 0 || ctx->zero_shift != 0 || ctx->edge_words != 1) return 0;
    LfCombiner* cb = ctx->comb;
    const int slot = ctx->comb_slot;
    {
        std::lock_guard<std::mutex> lk(cb->m);
        if (cb->dead || cb->members < LF_COMB_MIN_MEMBERS || !cb->h_in) return 0; /* too few to gain from combining: direct path */
        if (memcmp(&cb->code, &ctx->hcode, sizeof(LfDevCode)) != 0) return 0; /* lnsfaid_set_cfg changed REGULAR_COL_WEIGHT */
    }
    memcpy(cb->h_in + (size_t)slot * cb->group_bytes, fixInput, cb->group_bytes); /* every caller copies its own slot, in parallel */
    int rc;
    {
        std::unique_lock<std::mutex> lk(cb->m);
        LfSlot& s = cb->slots[slot];
        s.cfg = ctx->hcfg;
        s.rule = rule;
        s.state = LF_SLOT_PENDING;
        cb->pending += 1;
        cb->cv_work.notify_all(); /* (at most LF_COMB_WORKERS waiters) */
        if (!cb->cv_done.wait_for(lk, std::chrono::seconds(120), [&] { return s.state == LF_SLOT_DONE; })) {
            snprintf(g_hip_err, sizeof(g_hip_err), "call combiner: no result after 120 s");
            *rc_out = LNSFAID_E_INTERNAL;
            return 1;
        }
        rc = s.rc;
        if (rc != LNSFAID_OK) snprintf(g_hip_err, sizeof(g_hip_err), "%s", cb->err);
        if (stats) *stats = s.stats;
        s.state = LF_SLOT_IDLE;
    }
    if (rc == LNSFAID_OK) memcpy(decodedBits, cb->h_out + (size_t)slot * cb->group_bytes, cb->group_bytes);
    *rc_out = rc;
    return 1;
}


extern "C" int lnsfaid_frontend_set_interleave(lnsfaid_ctx* ctx, int32_t interleave_mod_type)
{
    if (!ctx || interleave_mod_type < 1 || ctx->n_var % interleave_mod_type != 0) return LNSFAID_E_INVAL;
    ctx->fe_interleave = interleave_mod_type;
    return LNSFAID_OK;
}

/* the per-stream frame buffers of the device front-end (lnsfaid_frontend_set_frames / lnsfaid_frontend_random_frames) */
static int alloc_fe_frames(lnsfaid_ctx* ctx)
{
    if (!ctx->d_fe_frames) {
        HIP_TRY(hipMalloc(&ctx->d_fe_frames, ctx->max_groups * LNSFAID_GROUP * (size_t)ctx->n_var));
        HIP_TRY(hipMalloc(&ctx->d_fe_input, ctx->max_groups * LNSFAID_GROUP * (size_t)ctx->k_info));
    }
    return LNSFAID_OK;
}

extern "C" int lnsfaid_frontend_set_frames(lnsfaid_ctx* ctx, const int8_t* outputBits, const int8_t* inputBits, size_t n_streams)
{
    if (!ctx || n_streams > ctx->max_groups) return LNSFAID_E_INVAL;
    if (!outputBits || n_streams == 0) { ctx->fe_frames_streams = 0; return LNSFAID_OK; } /* back to one codeword for all */
    if (!inputBits) return LNSFAID_E_INVAL;
    HIP_TRY(hipSetDevice(ctx->device));
    { const int rc = alloc_fe_frames(ctx); if (rc) return rc; }
    HIP_TRY(hipMemcpyAsync(ctx->d_fe_frames, outputBits, n_streams * LNSFAID_GROUP * (size_t)ctx->n_var, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->d_fe_input, inputBits, n_streams * LNSFAID_GROUP * (size_t)ctx->k_info, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->fe_frames_streams = n_streams;
    return LNSFAID_OK;
}

extern "C" int lnsfaid_frontend_input_bits(lnsfaid_ctx* ctx, const int8_t** d_inputBits)
{
    if (!ctx || !d_inputBits) return LNSFAID_E_INVAL;
    *d_inputBits = ctx->fe_frames_streams ? ctx->d_fe_input : nullptr;
    return LNSFAID_OK;
}

extern "C" int lnsfaid_frontend_sent_bits(lnsfaid_ctx* ctx, const int8_t** d_outputBits)
{
    if (!ctx || !d_outputBits) return LNSFAID_E_INVAL;
    *d_outputBits = ctx->fe_frames_streams ? ctx->d_fe_frames : nullptr;
    return LNSFAID_OK;
}

extern "C" int lnsfaid_io_buffers(lnsfaid_ctx* ctx, int8_t** d_fixInput, int8_t** d_decodedBits, lnsfaid_group_stats** d_stats)
{
    if (!ctx) return LNSFAID_E_INVAL;
    HIP_TRY(hipSetDevice(ctx->device));
    const int rc = ensure_io(ctx);
    if (rc) return rc;
    if (d_fixInput) *d_fixInput = ctx->d_io_in;
    if (d_decodedBits) *d_decodedBits = ctx->d_io_out;
    if (d_stats) *d_stats = ctx->d_io_stats;
    return LNSFAID_OK;
}

extern "C" int lnsfaid_read_stats(lnsfaid_ctx* ctx, lnsfaid_group_stats* stats, size_t n_groups)
{
    if (!ctx || (n_groups && !stats) || n_groups > ctx->max_groups) return LNSFAID_E_INVAL;
    if (n_groups == 0) return LNSFAID_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const int rc = ensure_io(ctx);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(stats, ctx->d_io_stats, n_groups * sizeof(lnsfaid_group_stats), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return LNSFAID_OK;
}

static bool host_pinned(const void* p)
{
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; } /* plain malloc memory */
    return at.type == hipMemoryTypeHost;
}

/* lnsfaid_decode under the given rule; cw_stats (per-codeword rule only) optional */
static int decode_host_impl(lnsfaid_ctx* ctx, const int8_t* fixInput, size_t n_groups, int8_t* decodedBits, lnsfaid_group_stats* stats,
                            lnsfaid_codeword_stats* cw_stats, int rule)
{
    if (!ctx || (n_groups && (!fixInput || !decodedBits))) return LNSFAID_E_INVAL;
    if (n_groups > ctx->max_groups) return LNSFAID_E_INVAL;
    if (rule == LNSFAID_STOP_CODEWORD && !cw_possible(ctx)) return LNSFAID_E_INVAL;
    if (n_groups == 0) return LNSFAID_OK;
    if (!cw_stats) {   /* a one-group context among others on its device: through the call combiner */
        int rcc = 0;
        if (comb_decode(ctx, fixInput, decodedBits, stats, rule, &rcc)) return rcc;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    int rc = ensure_io(ctx);
    if (rc) return rc;
    if (cw_stats && !ctx->d_io_cw_stats)
        HIP_TRY(hipMalloc(&ctx->d_io_cw_stats, ctx->max_groups * LNSFAID_GROUP * sizeof(lnsfaid_codeword_stats)));
    lnsfaid_codeword_stats* d_cw = cw_stats ? ctx->d_io_cw_stats : nullptr;
    const size_t group_bytes = LNSFAID_GROUP * (size_t)ctx->n_var;
    const size_t bytes = n_groups * group_bytes;
    /* Pinned host buffers (hipHostMalloc / lnsfaid_host_register): cut the batch into pieces of whole groups and overlap
     * the copy-in of piece c + 1 and the copy-out of piece c - 1 with the decode of piece c (groups are independent, and
     * a piece is decoded to completion before the next one starts, so the pieces share the per-codeword state buffers).
     * Pageable buffers cannot overlap (the runtime stages them synchronously): one copy in, one decode, one copy out. */
    size_t chunk = ((n_groups + LF_IO_CHUNKS - 1) / LF_IO_CHUNKS + 63) / 64 * 64; /* >= one full wave of workgroups */
    if (chunk >= n_groups || !host_pinned(fixInput) || !host_pinned(decodedBits)) { /* (small batches: no pointer query at all) */
        HIP_TRY(hipMemcpyAsync(ctx->d_io_in, fixInput, bytes, hipMemcpyHostToDevice, ctx->stream));
        rc = decode_device_rule(ctx, ctx->d_io_in, n_groups, ctx->d_io_out, ctx->d_io_stats, d_cw, rule, false);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(decodedBits, ctx->d_io_out, bytes, hipMemcpyDeviceToHost, ctx->stream));
    } else {
        if (!ctx->s_in) {
            HIP_TRY(hipStreamCreateWithFlags(&ctx->s_in, hipStreamNonBlocking));
            HIP_TRY(hipStreamCreateWithFlags(&ctx->s_out, hipStreamNonBlocking));
            for (auto& e : ctx->ev_in) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        }
        const size_t n_chunks = (n_groups + chunk - 1) / chunk; /* <= LF_IO_CHUNKS */
        for (size_t c = 0; c < n_chunks; ++c) { /* all copies in are queued at once, one event per piece */
            const size_t g0 = c * chunk, ng = g0 + chunk <= n_groups ? chunk : n_groups - g0;
            HIP_TRY(hipMemcpyAsync(ctx->d_io_in + g0 * group_bytes, fixInput + g0 * group_bytes, ng * group_bytes, hipMemcpyHostToDevice, ctx->s_in));
            HIP_TRY(hipEventRecord(ctx->ev_in[c], ctx->s_in));
        }
        for (size_t c = 0; c < n_chunks; ++c) {
            const size_t g0 = c * chunk, ng = g0 + chunk <= n_groups ? chunk : n_groups - g0;
            HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_in[c], 0));
            rc = decode_device_rule(ctx, ctx->d_io_in + g0 * group_bytes, ng, ctx->d_io_out + g0 * group_bytes, ctx->d_io_stats + g0,
                                    d_cw ? d_cw + g0 * LNSFAID_GROUP : nullptr, rule, false);
            if (rc) { (void)hipStreamSynchronize(ctx->s_in); (void)hipStreamSynchronize(ctx->s_out); return rc; }
            /* decode_device returns with the piece finished: its copy out needs no further ordering */
            HIP_TRY(hipMemcpyAsync(decodedBits + g0 * group_bytes, ctx->d_io_out + g0 * group_bytes, ng * group_bytes, hipMemcpyDeviceToHost, ctx->s_out));
        }
        HIP_TRY(hipStreamSynchronize(ctx->s_out));
    }
    if (stats)
        HIP_TRY(hipMemcpyAsync(stats, ctx->d_io_stats, n_groups * sizeof(lnsfaid_group_stats), hipMemcpyDeviceToHost,
                               ctx->stream));
    if (cw_stats)
        HIP_TRY(hipMemcpyAsync(cw_stats, d_cw, n_groups * LNSFAID_GROUP * sizeof(lnsfaid_codeword_stats), hipMemcpyDeviceToHost,
                               ctx->stream));
    { const int rcw = stream_wait(ctx); if (rcw) return rcw; }
    return LNSFAID_OK;
}

extern "C" int lnsfaid_decode(lnsfaid_ctx* ctx, const int8_t* fixInput, size_t n_groups, int8_t* decodedBits,
                              lnsfaid_group_stats* stats)
{
    if (!ctx) return LNSFAID_E_INVAL;
    return decode_host_impl(ctx, fixInput, n_groups, decodedBits, stats, nullptr, ctx->early_stop);
}

extern "C" int lnsfaid_decode_codewords(lnsfaid_ctx* ctx, const int8_t* fixInput, size_t n_groups, int8_t* decodedBits,
                                        lnsfaid_codeword_stats* cw_stats)
{
    return decode_host_impl(ctx, fixInput, n_groups, decodedBits, nullptr, cw_stats, LNSFAID_STOP_CODEWORD);
}

/* ---- pinned host memory for callers without a HIP toolchain (the reference is plain C++) ---------------- */
extern "C" int lnsfaid_host_register(void* ptr, size_t bytes)
{
    if (!ptr || !bytes) return LNSFAID_E_INVAL;
    HIP_TRY(hipHostRegister(ptr, bytes, hipHostRegisterPortable)); /* valid on every device of the process */
    return LNSFAID_OK;
}

extern "C" int lnsfaid_host_unregister(void* ptr)
{
    if (!ptr) return LNSFAID_E_INVAL;
    HIP_TRY(hipHostUnregister(ptr));
    return LNSFAID_OK;
}

extern "C" int lnsfaid_count_errors_device(lnsfaid_ctx* ctx, const int8_t* d_decodedBits, const int8_t* d_inputBits,
                                           size_t n_groups, uint64_t out[4])
{
    if (!ctx || !out || (n_groups && !d_decodedBits)) return LNSFAID_E_INVAL;
    if (n_groups == 0) return LNSFAID_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemsetAsync(ctx->d_counters, 0, 4 * sizeof(unsigned long long), ctx->stream));
    HIP_TRY(lf_launch_count_errors(d_decodedBits, d_inputBits, ctx->n_var, ctx->k_info, n_groups * LNSFAID_GROUP,
                                   ctx->d_counters, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->h_counters, ctx->d_counters, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                           ctx->stream));
    { const int rcw = stream_wait(ctx); if (rcw) return rcw; }
    for (int i = 0; i < 4; ++i) out[i] += ctx->h_counters[i];
    return LNSFAID_OK;
}

extern "C" int lnsfaid_count_errors(lnsfaid_ctx* ctx, const int8_t* decodedBits, const int8_t* inputBits, size_t n_groups,
                                    uint64_t out[4])
{
    if (!ctx || !out || (n_groups && !decodedBits)) return LNSFAID_E_INVAL;
    if (n_groups > ctx->max_groups) return LNSFAID_E_INVAL;
    if (n_groups == 0) return LNSFAID_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    int rc = ensure_io(ctx);
    if (rc) return rc;
    const size_t n_cw = n_groups * LNSFAID_GROUP;
    HIP_TRY(hipMemcpyAsync(ctx->d_io_out, decodedBits, n_cw * (size_t)ctx->n_var, hipMemcpyHostToDevice, ctx->stream));
    const int8_t* d_in = nullptr;
    if (inputBits) {
        /* [32][K] per group packed back to back fits in the (larger) fixInput staging buffer */
        HIP_TRY(hipMemcpyAsync(ctx->d_io_in, inputBits, n_cw * (size_t)ctx->k_info, hipMemcpyHostToDevice, ctx->stream));
        d_in = ctx->d_io_in;
    }
    return lnsfaid_count_errors_device(ctx, ctx->d_io_out, d_in, n_groups, out);
}

/* ---- packed decode I/O (include/lnsfaid.h "Packed decode I/O") ------------------------------------------ */
static bool dword_aligned(const void* p) { return ((uintptr_t)p & 3u) == 0u; }

static int ensure_packed_io(lnsfaid_ctx* ctx)
{
    if (ctx->d_pk_in) return LNSFAID_OK;
    HIP_TRY(hipMalloc(&ctx->d_pk_in, ctx->max_groups * LNSFAID_GROUP * (size_t)ctx->n_var / 2));
    HIP_TRY(hipMalloc(&ctx->d_pk_out, ctx->max_groups * LNSFAID_GROUP * (size_t)ctx->n_var / 8));
    HIP_TRY(hipMalloc(&ctx->d_pk_stats, ctx->max_groups * sizeof(lnsfaid_group_stats)));
    return LNSFAID_OK;
}

/* one batch of device buffers under the given rule: the packed twin of the four-rows kernel, or (group rule only) llr4 -> int8 in
 * the context's io buffers, the int8 decode, int8 -> bits */
static int decode_packed_rule(lnsfaid_ctx* ctx, const uint8_t* d_llr4, size_t n_groups, uint32_t* d_bits, lnsfaid_group_stats* d_stats,
                              lnsfaid_codeword_stats* d_cw_stats, int rule)
{
    if (rule == LNSFAID_STOP_CODEWORD)
        return decode_cw_device_impl(ctx, (const int8_t*)d_llr4, n_groups, (int8_t*)d_bits, d_stats, d_cw_stats, false, true);
    if (packed_kernel(ctx)) return decode_device_impl(ctx, (const int8_t*)d_llr4, n_groups, (int8_t*)d_bits, d_stats, false, true);
    int rc = ensure_io(ctx);
    if (rc) return rc;
    const size_t n_values = n_groups * LNSFAID_GROUP * (size_t)ctx->n_var;
    HIP_TRY(lf_launch_unpack_llr4(d_llr4, ctx->d_io_in, n_values, ctx->stream));
    rc = decode_device_impl(ctx, ctx->d_io_in, n_groups, ctx->d_io_out, d_stats, false);
    if (rc) return rc;
    HIP_TRY(lf_launch_pack_bits(ctx->d_io_out, d_bits, n_values, ctx->stream));
    return stream_wait(ctx); /* returns with the output complete, as the decoders do */
}

static int decode_packed_device_impl(lnsfaid_ctx* ctx, const uint8_t* d_llr4, size_t n_groups, uint32_t* d_bits, lnsfaid_group_stats* d_stats,
                                     lnsfaid_codeword_stats* d_cw_stats, int rule)
{
    if (!ctx || (n_groups && (!d_llr4 || !d_bits))) return LNSFAID_E_INVAL;
    if (n_groups > ctx->max_groups) return LNSFAID_E_INVAL;
    if (rule == LNSFAID_STOP_CODEWORD && !cw_possible(ctx)) return LNSFAID_E_INVAL;
    if (n_groups == 0) return LNSFAID_OK;
    if (!dword_aligned(d_llr4) || !dword_aligned(d_bits) || !dword_aligned(d_stats) || !dword_aligned(d_cw_stats)) return LNSFAID_E_INVAL;
    HIP_TRY(hipSetDevice(ctx->device));
    return decode_packed_rule(ctx, d_llr4, n_groups, d_bits, d_stats, d_cw_stats, rule);
}

extern "C" int lnsfaid_decode_packed_device(lnsfaid_ctx* ctx, const uint8_t* d_llr4, size_t n_groups, uint32_t* d_bits,
                                            lnsfaid_group_stats* d_stats)
{
    if (!ctx) return LNSFAID_E_INVAL;
    return decode_packed_device_impl(ctx, d_llr4, n_groups, d_bits, d_stats, nullptr, ctx->early_stop);
}

extern "C" int lnsfaid_decode_codewords_packed_device(lnsfaid_ctx* ctx, const uint8_t* d_llr4, size_t n_groups, uint32_t* d_bits,
                                                      lnsfaid_codeword_stats* d_cw_stats)
{
    return decode_packed_device_impl(ctx, d_llr4, n_groups, d_bits, nullptr, d_cw_stats, LNSFAID_STOP_CODEWORD);
}

/* host buffers through the packed staging: as decode_host_impl (pieces that overlap copy-in, decode and copy-out when both buffers
 * are pinned, one copy each way otherwise), always on the context's own stream (no call combiner) */
static int decode_packed_host_impl(lnsfaid_ctx* ctx, const uint8_t* llr4, size_t n_groups, uint32_t* bits, lnsfaid_group_stats* stats,
                                   lnsfaid_codeword_stats* cw_stats, int rule)
{
    if (!ctx || (n_groups && (!llr4 || !bits))) return LNSFAID_E_INVAL;
    if (n_groups > ctx->max_groups) return LNSFAID_E_INVAL;
    if (rule == LNSFAID_STOP_CODEWORD && !cw_possible(ctx)) return LNSFAID_E_INVAL;
    if (n_groups == 0) return LNSFAID_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    int rc = ensure_packed_io(ctx);
    if (rc) return rc;
    if (cw_stats && !ctx->d_io_cw_stats)
        HIP_TRY(hipMalloc(&ctx->d_io_cw_stats, ctx->max_groups * LNSFAID_GROUP * sizeof(lnsfaid_codeword_stats)));
    lnsfaid_codeword_stats* d_cw = cw_stats ? ctx->d_io_cw_stats : nullptr;
    const size_t in_bytes = LNSFAID_GROUP * (size_t)ctx->n_var / 2, out_words = LNSFAID_GROUP * (size_t)ctx->n_var / 32;
    size_t chunk = ((n_groups + LF_IO_CHUNKS - 1) / LF_IO_CHUNKS + 63) / 64 * 64;
    if (chunk >= n_groups || !host_pinned(llr4) || !host_pinned(bits)) {
        HIP_TRY(hipMemcpyAsync(ctx->d_pk_in, llr4, n_groups * in_bytes, hipMemcpyHostToDevice, ctx->stream));
        rc = decode_packed_rule(ctx, ctx->d_pk_in, n_groups, ctx->d_pk_out, ctx->d_pk_stats, d_cw, rule);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(bits, ctx->d_pk_out, n_groups * out_words * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    } else {
        if (!ctx->s_in) {
            HIP_TRY(hipStreamCreateWithFlags(&ctx->s_in, hipStreamNonBlocking));
            HIP_TRY(hipStreamCreateWithFlags(&ctx->s_out, hipStreamNonBlocking));
            for (auto& e : ctx->ev_in) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        }
        const size_t n_chunks = (n_groups + chunk - 1) / chunk; /* <= LF_IO_CHUNKS */
        for (size_t c = 0; c < n_chunks; ++c) {
            const size_t g0 = c * chunk, ng = g0 + chunk <= n_groups ? chunk : n_groups - g0;
            HIP_TRY(hipMemcpyAsync(ctx->d_pk_in + g0 * in_bytes, llr4 + g0 * in_bytes, ng * in_bytes, hipMemcpyHostToDevice, ctx->s_in));
            HIP_TRY(hipEventRecord(ctx->ev_in[c], ctx->s_in));
        }
        for (size_t c = 0; c < n_chunks; ++c) {
            const size_t g0 = c * chunk, ng = g0 + chunk <= n_groups ? chunk : n_groups - g0;
            HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_in[c], 0));
            rc = decode_packed_rule(ctx, ctx->d_pk_in + g0 * in_bytes, ng, ctx->d_pk_out + g0 * out_words, ctx->d_pk_stats + g0,
                                    d_cw ? d_cw + g0 * LNSFAID_GROUP : nullptr, rule);
            if (rc) { (void)hipStreamSynchronize(ctx->s_in); (void)hipStreamSynchronize(ctx->s_out); return rc; }
            HIP_TRY(hipMemcpyAsync(bits + g0 * out_words, ctx->d_pk_out + g0 * out_words, ng * out_words * sizeof(uint32_t),
                                   hipMemcpyDeviceToHost, ctx->s_out));
        }
        HIP_TRY(hipStreamSynchronize(ctx->s_out));
    }
    if (stats)
        HIP_TRY(hipMemcpyAsync(stats, ctx->d_pk_stats, n_groups * sizeof(lnsfaid_group_stats), hipMemcpyDeviceToHost, ctx->stream));
    if (cw_stats)
        HIP_TRY(hipMemcpyAsync(cw_stats, d_cw, n_groups * LNSFAID_GROUP * sizeof(lnsfaid_codeword_stats), hipMemcpyDeviceToHost,
                               ctx->stream));
    { const int rcw = stream_wait(ctx); if (rcw) return rcw; }
    return LNSFAID_OK;
}

extern "C" int lnsfaid_decode_packed(lnsfaid_ctx* ctx, const uint8_t* llr4, size_t n_groups, uint32_t* bits, lnsfaid_group_stats* stats)
{
    if (!ctx) return LNSFAID_E_INVAL;
    return decode_packed_host_impl(ctx, llr4, n_groups, bits, stats, nullptr, ctx->early_stop);
}

extern "C" int lnsfaid_decode_codewords_packed(lnsfaid_ctx* ctx, const uint8_t* llr4, size_t n_groups, uint32_t* bits,
                                               lnsfaid_codeword_stats* cw_stats)
{
    return decode_packed_host_impl(ctx, llr4, n_groups, bits, nullptr, cw_stats, LNSFAID_STOP_CODEWORD);
}

extern "C" int lnsfaid_count_errors_packed_device(lnsfaid_ctx* ctx, const uint32_t* d_bits, const uint8_t* d_msg, size_t n_groups,
                                                  uint64_t out[4])
{
    if (!ctx || !out || (n_groups && !d_bits)) return LNSFAID_E_INVAL;
    if (n_groups == 0) return LNSFAID_OK;
    if (!dword_aligned(d_bits) || !dword_aligned(d_msg)) return LNSFAID_E_INVAL;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemsetAsync(ctx->d_counters, 0, 4 * sizeof(unsigned long long), ctx->stream));
    HIP_TRY(lf_launch_count_errors_packed(d_bits, (const uint32_t*)d_msg, ctx->n_var, ctx->k_info, n_groups * LNSFAID_GROUP,
                                          ctx->d_counters, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->h_counters, ctx->d_counters, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    { const int rcw = stream_wait(ctx); if (rcw) return rcw; }
    for (int i = 0; i < 4; ++i) out[i] += ctx->h_counters[i];
    return LNSFAID_OK;
}

extern "C" int lnsfaid_count_errors_packed(lnsfaid_ctx* ctx, const uint32_t* bits, const uint8_t* msg, size_t n_groups, uint64_t out[4])
{
    if (!ctx || !out || (n_groups && !bits)) return LNSFAID_E_INVAL;
    if (n_groups > ctx->max_groups) return LNSFAID_E_INVAL;
    if (n_groups == 0) return LNSFAID_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const int rc = ensure_packed_io(ctx);
    if (rc) return rc;
    const size_t n_cw = n_groups * LNSFAID_GROUP;
    HIP_TRY(hipMemcpyAsync(ctx->d_pk_out, bits, n_cw * (size_t)ctx->n_var / 8, hipMemcpyHostToDevice, ctx->stream));
    const uint8_t* d_msg = nullptr;
    if (msg) { /* K / 8 bytes per codeword fit in the (larger) llr4 staging buffer */
        HIP_TRY(hipMemcpyAsync(ctx->d_pk_in, msg, n_cw * (size_t)ctx->k_info / 8, hipMemcpyHostToDevice, ctx->stream));
        d_msg = ctx->d_pk_in;
    }
    return lnsfaid_count_errors_packed_device(ctx, ctx->d_pk_out, d_msg, n_groups, out);
}

/* ---- line-format decode (include/lnsfaid.h "line-format decode", DESIGN.md 3.14, lnsfaid_kernel4l.hip) ------------------ */
/* everything that can be refused without looking at the buffers; 1: nothing to do */
static int line_rules(const lnsfaid_ctx* ctx, int32_t format, int32_t magnitude, size_t n_codewords)
{
    if (!ctx || (format != LNSFAID_LINE_HARD && format != LNSFAID_LINE_LLR4)) return LNSFAID_E_INVAL;
    if (format == LNSFAID_LINE_HARD && (magnitude < 1 || magnitude > 7)) return LNSFAID_E_INVAL;
    const int L = ctx->n_var - ctx->hcode.puncture_tail;
    if (L <= 0 || L % 32 != 0 || ctx->k_info % 32 != 0) return LNSFAID_E_INVAL;
    if (n_codewords > ctx->max_groups * LNSFAID_GROUP) return LNSFAID_E_INVAL;
    if (!cw_possible(ctx)) return LNSFAID_E_INVAL;
    return n_codewords == 0 ? 1 : LNSFAID_OK;
}

static size_t line_bytes(const lnsfaid_ctx* ctx, int32_t format)
{
    const size_t L = (size_t)(ctx->n_var - ctx->hcode.puncture_tail);
    return format == LNSFAID_LINE_HARD ? L / 8 : L / 2;
}

/* one launch, one wait: the per-codeword rule (decode_cw_device_impl) without group records */
static int decode_line_launch(lnsfaid_ctx* ctx, const void* d_line, int32_t format, int32_t magnitude, size_t n_codewords,
                              uint32_t* d_payload, uint32_t* d_bits, lnsfaid_line_stats* d_stats)
{
    LfInst k;
    {
        const int rc = kernel_check(ctx, LF_ENTRY_LINE, &k);
        if (rc) return rc;
    }
    LfLineArgs a;
    a.code = ctx->d_code; a.cfg = ctx->d_cfg;
    a.line = d_line; a.payload = d_payload; a.bits = d_bits;
    a.st_rows = ctx->d_rows;
    a.stats = d_stats;
    a.format = format; a.magnitude = magnitude; a.n_cw = (int32_t)n_codewords;
    return launch_decode_timed(ctx, k, &a, n_codewords, "line");
}

extern "C" int lnsfaid_decode_line_device(lnsfaid_ctx* ctx, const void* d_line, int32_t format, int32_t magnitude, size_t n_codewords,
                                          uint32_t* d_payload, uint32_t* d_bits, lnsfaid_line_stats* d_stats)
{
    const int rc = line_rules(ctx, format, magnitude, n_codewords);
    if (rc) return rc < 0 ? rc : LNSFAID_OK;
    if (!d_line || !d_payload) return LNSFAID_E_INVAL;
    if (!dword_aligned(d_line) || !dword_aligned(d_payload) || !dword_aligned(d_bits) || !dword_aligned(d_stats)) return LNSFAID_E_INVAL;
    HIP_TRY(hipSetDevice(ctx->device));
    return decode_line_launch(ctx, d_line, format, magnitude, n_codewords, d_payload, d_bits, d_stats);
}

/* host buffers of any alignment: one copy each way through staging buffers of the context, on its own stream */
extern "C" int lnsfaid_decode_line(lnsfaid_ctx* ctx, const void* line, int32_t format, int32_t magnitude, size_t n_codewords,
                                   uint32_t* payload, uint32_t* bits, lnsfaid_line_stats* stats)
{
    int rc = line_rules(ctx, format, magnitude, n_codewords);
    if (rc) return rc < 0 ? rc : LNSFAID_OK;
    if (!line || !payload) return LNSFAID_E_INVAL;
    HIP_TRY(hipSetDevice(ctx->device));
    rc = ensure_packed_io(ctx); /* d_pk_in holds a line of 32 * max_groups codewords in either format, d_pk_out their bits */
    if (rc) return rc;
    if (!ctx->d_ln_payload) {
        HIP_TRY(hipMalloc(&ctx->d_ln_payload, ctx->max_groups * LNSFAID_GROUP * (size_t)ctx->k_info / 8));
        HIP_TRY(hipMalloc(&ctx->d_ln_stats, ctx->max_groups * LNSFAID_GROUP * sizeof(lnsfaid_line_stats)));
    }
    const size_t k_bytes = (size_t)ctx->k_info / 8, n_bytes = (size_t)ctx->n_var / 8;
    HIP_TRY(hipMemcpyAsync(ctx->d_pk_in, line, n_codewords * line_bytes(ctx, format), hipMemcpyHostToDevice, ctx->stream));
    rc = decode_line_launch(ctx, ctx->d_pk_in, format, magnitude, n_codewords, ctx->d_ln_payload, bits ? ctx->d_pk_out : nullptr,
                            stats ? ctx->d_ln_stats : nullptr);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(payload, ctx->d_ln_payload, n_codewords * k_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (bits) HIP_TRY(hipMemcpyAsync(bits, ctx->d_pk_out, n_codewords * n_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (stats)
        HIP_TRY(hipMemcpyAsync(stats, ctx->d_ln_stats, n_codewords * sizeof(lnsfaid_line_stats), hipMemcpyDeviceToHost, ctx->stream));
    return stream_wait(ctx);
}

/* host-only format helpers (no context, no GPU) */
extern "C" int lnsfaid_pack_llr4(const int8_t* fixInput, size_t n_values, uint8_t* llr4)
{
    if (n_values % 2 || (n_values && (!fixInput || !llr4))) return LNSFAID_E_INVAL;
    for (size_t i = 0; i < n_values; i += 2) {
        const int a = fixInput[i], b = fixInput[i + 1];
        if (a < -8 || a > 7 || b < -8 || b > 7) return LNSFAID_E_INVAL;
        llr4[i / 2] = (uint8_t)((a & 15) | ((b & 15) << 4));
    }
    return LNSFAID_OK;
}

extern "C" int lnsfaid_unpack_bits(const uint32_t* bits, size_t n_bits, int8_t* decodedBits)
{
    if (n_bits % 32 || (n_bits && (!bits || !decodedBits))) return LNSFAID_E_INVAL;
    for (size_t i = 0; i < n_bits; ++i) decodedBits[i] = (int8_t)((bits[i / 32] >> (i % 32)) & 1u);
    return LNSFAID_OK;
}

extern "C" int lnsfaid_pack_bits(const int8_t* inputBits, size_t n_bits, uint8_t* packed)
{
    if (n_bits % 8 || (n_bits && (!inputBits || !packed))) return LNSFAID_E_INVAL;
    for (size_t i = 0; i < n_bits; i += 8) {
        uint8_t v = 0;
        for (int b = 0; b < 8; ++b) {
            const int x = inputBits[i + (size_t)b];
            if (x != 0 && x != 1) return LNSFAID_E_INVAL;
            v |= (uint8_t)(x << b);
        }
        packed[i / 8] = v;
    }
    return LNSFAID_OK;
}

/* ---- front-end on the device ------------------------------------------------------------------------ */
extern "C" uint64_t lnsfaid_frontend_draws_per_group(const lnsfaid_ctx* ctx, int32_t mod_type)
{
    if (!ctx || (mod_type != 2 && mod_type != 4 && mod_type != 6 && mod_type != 8)) return 0;
    /* 32 * n_var / mod_type symbols, 2 normals per symbol, 2 uniforms per normal */
    return (uint64_t)32 * (uint64_t)ctx->n_var / (uint64_t)mod_type * 4u;
}

extern "C" int lnsfaid_frontend_device_states(lnsfaid_ctx* ctx, const uint32_t* states, const uint64_t* draws_before, size_t n_streams,
                                              int32_t mod_type, float sigma, float scale, const int8_t* codeword, int8_t* d_fixInput)
{
    if (!ctx || !states || !draws_before || !d_fixInput || (mod_type != 2 && mod_type != 4 && mod_type != 6 && mod_type != 8)) return LNSFAID_E_INVAL;
    if (n_streams == 0) return LNSFAID_OK;
    if (n_streams > ctx->max_groups || (32L * ctx->n_var) % mod_type != 0) return LNSFAID_E_INVAL;
    if (ctx->fe_prefec && ctx->n_var % mod_type != 0) return LNSFAID_E_INVAL; /* a symbol must not straddle two frames */
    HIP_TRY(hipSetDevice(ctx->device));
    if (!ctx->d_fe_seeds) {
        HIP_TRY(hipMalloc(&ctx->d_fe_seeds, ctx->max_groups * 3 * sizeof(uint32_t)));
        HIP_TRY(hipMalloc(&ctx->d_fe_draws, ctx->max_groups * sizeof(unsigned long long)));
        HIP_TRY(hipMalloc(&ctx->d_fe_codeword, (size_t)ctx->n_var));
    }
    HIP_TRY(hipMemcpyAsync(ctx->d_fe_seeds, states, n_streams * 3 * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->d_fe_draws, draws_before, n_streams * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    if (codeword) HIP_TRY(hipMemcpyAsync(ctx->d_fe_codeword, codeword, (size_t)ctx->n_var, hipMemcpyHostToDevice, ctx->stream));
    /* AWGNChannel(ModSeq, sigma / sqrt(2)): float / double -> double, narrowed to float (CSimulate.cpp:126) */
    const float sigma_ch = (float)((double)sigma / 1.4142135623730951);
    HIP_TRY(lf_launch_frontend(ctx->d_fe_seeds, ctx->d_fe_draws, (int)n_streams, mod_type, sigma_ch, scale,
                               codeword ? ctx->d_fe_codeword : nullptr,
                               (!codeword && ctx->fe_frames_streams >= n_streams) ? ctx->d_fe_frames : nullptr, ctx->n_var,
                               ctx->n_check, ctx->fe_interleave, ctx->fe_exact ? 0 : 1, d_fixInput,
                               ctx->fe_prefec == LNSFAID_PREFEC_INFO ? ctx->k_info : ctx->fe_prefec ? ctx->n_var : 0,
                               ctx->fe_prefec ? ctx->d_fe_prefec_frames : nullptr, ctx->stream));
    if (ctx->fe_prefec) HIP_TRY(lf_launch_prefec_fold(ctx->d_fe_prefec_frames, n_streams, ctx->d_fe_prefec_acc, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream)); /* states / draws_before may be reused by the caller */
    return LNSFAID_OK;
}

extern "C" int lnsfaid_frontend_set_exact(lnsfaid_ctx* ctx, int32_t exact)
{
    if (!ctx || exact < 0 || exact > 1) return LNSFAID_E_INVAL;
    ctx->fe_exact = exact;
    return LNSFAID_OK;
}

extern "C" int lnsfaid_frontend_set_prefec(lnsfaid_ctx* ctx, int32_t scope)
{
    if (!ctx || (scope != 0 && scope != LNSFAID_PREFEC_INFO && scope != LNSFAID_PREFEC_CODEWORD)) return LNSFAID_E_INVAL;
    HIP_TRY(hipSetDevice(ctx->device));
    if (scope && !ctx->d_fe_prefec_frames) {
        const size_t bytes = ctx->max_groups * LNSFAID_GROUP * sizeof(unsigned long long);
        HIP_TRY(hipMalloc(&ctx->d_fe_prefec_acc, 4 * sizeof(unsigned long long)));
        HIP_TRY(hipMalloc(&ctx->d_fe_prefec_frames, bytes));
        HIP_TRY(hipMemsetAsync(ctx->d_fe_prefec_frames, 0, bytes, ctx->stream)); /* from here on the fold kernel leaves it cleared */
    }
    if (ctx->d_fe_prefec_acc) {
        HIP_TRY(hipMemsetAsync(ctx->d_fe_prefec_acc, 0, 4 * sizeof(unsigned long long), ctx->stream));
        const int rcw = stream_wait(ctx);
        if (rcw) return rcw;
    }
    ctx->fe_prefec = scope;
    return LNSFAID_OK;
}

extern "C" int lnsfaid_frontend_prefec_counters(lnsfaid_ctx* ctx, uint64_t out[4], int32_t reset)
{
    if (!ctx || !out) return LNSFAID_E_INVAL;
    if (!ctx->d_fe_prefec_acc) return LNSFAID_OK; /* counting was never switched on: nothing to add */
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(ctx->h_counters, ctx->d_fe_prefec_acc, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    if (reset) HIP_TRY(hipMemsetAsync(ctx->d_fe_prefec_acc, 0, 4 * sizeof(unsigned long long), ctx->stream));
    { const int rcw = stream_wait(ctx); if (rcw) return rcw; }
    for (int i = 0; i < 4; ++i) out[i] += ctx->h_counters[i];
    return LNSFAID_OK;
}

extern "C" int lnsfaid_frontend_fastpath_bounds(lnsfaid_ctx* ctx, double measured[2], double assumed[2])
{
    if (!ctx || !measured || !assumed) return LNSFAID_E_INVAL;
    HIP_TRY(hipSetDevice(ctx->device));
    double* d = nullptr;
    HIP_TRY(hipMalloc(&d, 2 * sizeof(double)));
    hipError_t e = lf_frontend_fastpath_scan(d, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(measured, d, 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    (void)hipFree(d);
    HIP_TRY(e);
    lf_frontend_fastpath_assumed(assumed);
    return LNSFAID_OK;
}

extern "C" int lnsfaid_frontend_device(lnsfaid_ctx* ctx, const uint32_t* seeds, const uint64_t* draws_before, size_t n_streams,
                                       int32_t mod_type, float sigma, float scale, const int8_t* codeword, int8_t* d_fixInput)
{
    if (!ctx || !seeds || !draws_before || !d_fixInput) return LNSFAID_E_INVAL;
    if (n_streams > ctx->max_groups) return LNSFAID_E_INVAL; /* before anything is sized by it */
    if (n_streams == 0) return LNSFAID_OK;
    std::vector<uint32_t> st; /* CChannel::Initial without CONTINUE_SEED: IX = IY = IZ = seed (CChannel.cpp:121) */
    try {
        st.resize(3 * n_streams);
    } catch (...) {
        return LNSFAID_E_NOMEM; /* nothing is thrown across the C boundary */
    }
    for (size_t i = 0; i < n_streams; ++i) st[3 * i] = st[3 * i + 1] = st[3 * i + 2] = seeds[i];
    return lnsfaid_frontend_device_states(ctx, st.data(), draws_before, n_streams, mod_type, sigma, scale, codeword, d_fixInput);
}

/* ---- demapper for received symbols (lnsfaid_demap.hip) ------------------------------------- */
static int demap_rules(int n_var, int n_check, int interleave, int mod_type, bool packed)
{
    if (n_var <= 0 || n_check <= 0 || n_check >= n_var) return LNSFAID_E_INVAL;
    if (mod_type != 1 && mod_type != 2 && mod_type != 4 && mod_type != 6 && mod_type != 8) return LNSFAID_E_INVAL;
    if (interleave < 1 || n_var % interleave != 0 || (32L * n_var) % mod_type != 0) return LNSFAID_E_INVAL;
    if (packed && (n_var % 2 != 0 || (n_var - n_check) % 2 != 0)) return LNSFAID_E_INVAL;
    return LNSFAID_OK;
}

static int demap_device_impl(lnsfaid_ctx* ctx, const float* d_rx, size_t n_groups, int32_t mod_type, float scale, void* d_out, bool packed)
{
    if (!ctx) return LNSFAID_E_INVAL;
    const int rc = demap_rules(ctx->n_var, ctx->n_check, ctx->fe_interleave, mod_type, packed);
    if (rc) return rc;
    if (n_groups > ctx->max_groups) return LNSFAID_E_INVAL;
    if (n_groups == 0) return LNSFAID_OK;
    if (!d_rx || !d_out || !dword_aligned(d_rx) || (packed && !dword_aligned(d_out))) return LNSFAID_E_INVAL;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(lf_launch_demap(d_rx, n_groups, mod_type, scale, ctx->n_var, ctx->n_check, ctx->fe_interleave, packed ? 1 : 0, d_out, ctx->stream));
    return stream_wait(ctx); /* returns with the output complete, as the encoder does */
}

extern "C" int lnsfaid_demap_device(lnsfaid_ctx* ctx, const float* d_rx, size_t n_groups, int32_t mod_type, float scale, int8_t* d_fixInput)
{
    return demap_device_impl(ctx, d_rx, n_groups, mod_type, scale, d_fixInput, false);
}

extern "C" int lnsfaid_demap_packed_device(lnsfaid_ctx* ctx, const float* d_rx, size_t n_groups, int32_t mod_type, float scale, uint8_t* d_llr4)
{
    return demap_device_impl(ctx, d_rx, n_groups, mod_type, scale, d_llr4, true);
}

/* One group on the host, the formulas of include/lnsfaid.h taken literally (no HIP call) */
static void demap_group_host(int N, int M, int I, int mod_type, const float* rx, float scale, int8_t* fix)
{
    static const double c16[1] = { 0.6324555 }, c64[2] = { 0.6172134, 0.3086067 }, c256[3] = { 0.613568, 0.306784, 0.153392 };
    const int K = N - M;
    if (mod_type == 1) { /* one real float per code bit, frame-major, not interleaved */
        for (int m = 0; m < 32; ++m)
            for (int k = 0; k < N; ++k) {
                const int8_t q = quantise_4bit(rx[(size_t)m * N + k], scale);
                if (k < K) fix[(size_t)m * K + k] = q;
                else fix[(size_t)32 * K + (size_t)m * M + (k - K)] = q;
            }
        return;
    }
    const double* c = mod_type == 4 ? c16 : mod_type == 6 ? c64 : c256;
    const long symbols = 32L * N / mod_type;
    for (long s = 0; s < symbols; ++s) {
        float l[8];
        l[0] = rx[2 * s];
        l[1] = rx[2 * s + 1];
        for (int n = 1; n < mod_type / 2; ++n) { /* every level is stored as float before it feeds the next */
            l[2 * n] = (float)(fabs((double)l[2 * n - 2]) - c[n - 1]);
            l[2 * n + 1] = (float)(fabs((double)l[2 * n - 1]) - c[n - 1]);
        }
        for (int u = 0; u < mod_type; ++u) {
            const long pos = (long)mod_type * s + u;
            const int m = (int)(pos / N), p = (int)(pos % N);
            const int k = (N / I) * (p % I) + p / I;
            const int8_t q = quantise_4bit(l[u], scale);
            if (k < K) fix[(size_t)m * K + k] = q;
            else fix[(size_t)32 * K + (size_t)m * M + (k - K)] = q;
        }
    }
}

static int demap_host_impl(int32_t n_var, int32_t n_check, int32_t interleave, const float* rx, size_t n_groups, int32_t mod_type,
                           float scale, void* out, bool packed)
{
    const int rc = demap_rules(n_var, n_check, interleave, mod_type, packed);
    if (rc) return rc;
    if (n_groups == 0) return LNSFAID_OK;
    if (!rx || !out) return LNSFAID_E_INVAL;
    const size_t per = 32 * (size_t)n_var, rx_per = mod_type == 1 ? per : 2 * (per / (size_t)mod_type);
    std::vector<int8_t> group; /* the packed form quantises a group into bytes first, then packs: every output byte is written whole */
    if (packed) {
        try {
            group.resize(per);
        } catch (...) {
            return LNSFAID_E_NOMEM;
        }
    }
    for (size_t g = 0; g < n_groups; ++g) {
        int8_t* fix = packed ? group.data() : (int8_t*)out + g * per;
        demap_group_host(n_var, n_check, interleave, mod_type, rx + g * rx_per, scale, fix);
        if (packed) {
            const int prc = lnsfaid_pack_llr4(fix, per, (uint8_t*)out + g * (per / 2));
            if (prc) return prc;
        }
    }
    return LNSFAID_OK;
}

extern "C" int lnsfaid_demap_host(int32_t n_var, int32_t n_check, int32_t interleave_mod_type, const float* rx, size_t n_groups,
                                  int32_t mod_type, float scale, int8_t* fixInput)
{
    return demap_host_impl(n_var, n_check, interleave_mod_type, rx, n_groups, mod_type, scale, fixInput, false);
}

extern "C" int lnsfaid_demap_packed_host(int32_t n_var, int32_t n_check, int32_t interleave_mod_type, const float* rx, size_t n_groups,
                                         int32_t mod_type, float scale, uint8_t* llr4)
{
    return demap_host_impl(n_var, n_check, interleave_mod_type, rx, n_groups, mod_type, scale, llr4, true);
}

/* ---- pre-FEC error counters (lnsfaid_prefec.hip) ------------------------------------------- */
static int prefec_rules(int n_var, int n_check, int interleave, int mod_type, int scope)
{
    const int rc = demap_rules(n_var, n_check, interleave, mod_type, false);
    if (rc) return rc;
    if (n_var % mod_type != 0) return LNSFAID_E_INVAL; /* no symbol straddles two frames */
    if (scope != LNSFAID_PREFEC_INFO && scope != LNSFAID_PREFEC_CODEWORD) return LNSFAID_E_INVAL;
    return LNSFAID_OK;
}

extern "C" int lnsfaid_prefec_errors_device(lnsfaid_ctx* ctx, const float* d_rx, size_t n_groups, int32_t mod_type, const int8_t* d_sent,
                                            int32_t scope, uint64_t out[4])
{
    if (!ctx) return LNSFAID_E_INVAL;
    const int rc = prefec_rules(ctx->n_var, ctx->n_check, ctx->fe_interleave, mod_type, scope);
    if (rc) return rc;
    if (n_groups > ctx->max_groups) return LNSFAID_E_INVAL;
    if (n_groups == 0) return LNSFAID_OK;
    if (!d_rx || !out || !dword_aligned(d_rx)) return LNSFAID_E_INVAL;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemsetAsync(ctx->d_counters, 0, 4 * sizeof(unsigned long long), ctx->stream));
    HIP_TRY(lf_launch_prefec(d_rx, d_sent, n_groups, mod_type, ctx->n_var, ctx->n_check, ctx->fe_interleave, scope, ctx->d_counters, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->h_counters, ctx->d_counters, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    { const int rcw = stream_wait(ctx); if (rcw) return rcw; }
    for (int i = 0; i < 4; ++i) out[i] += ctx->h_counters[i];
    return LNSFAID_OK;
}

/* The definition of include/lnsfaid.h taken literally (no HIP call): the reference of the device paths */
extern "C" int lnsfaid_prefec_errors_host(int32_t n_var, int32_t n_check, int32_t interleave_mod_type, const float* rx, size_t n_groups,
                                          int32_t mod_type, const int8_t* sent, int32_t scope, uint64_t out[4])
{
    static const double c16[1] = { 0.6324555 }, c64[2] = { 0.6172134, 0.3086067 }, c256[3] = { 0.613568, 0.306784, 0.153392 };
    const int rc = prefec_rules(n_var, n_check, interleave_mod_type, mod_type, scope);
    if (rc) return rc;
    if (n_groups == 0) return LNSFAID_OK;
    if (!rx || !out) return LNSFAID_E_INVAL;
    const int N = n_var, M = n_check, K = N - M, I = mod_type == 1 ? 1 : interleave_mod_type;
    const int k_lim = scope == LNSFAID_PREFEC_INFO ? K : N;
    const size_t per = 32 * (size_t)N, rx_per = mod_type == 1 ? per : 2 * (per / (size_t)mod_type);
    const double* c = mod_type == 4 ? c16 : mod_type == 6 ? c64 : c256;
    const long symbols = (long)(per / (size_t)mod_type);
    for (size_t g = 0; g < n_groups; ++g) {
        const float* r = rx + g * rx_per;
        const int8_t* s = sent ? sent + g * per : nullptr;
        uint64_t frame_bits[32] = { 0 }, sym_err = 0;
        for (long sy = 0; sy < symbols; ++sy) {
            float l[8];
            if (mod_type == 1) {
                l[0] = r[sy];
            } else {
                l[0] = r[2 * sy];
                l[1] = r[2 * sy + 1];
                for (int n = 1; n < mod_type / 2; ++n) { /* every level is stored as float before it feeds the next */
                    l[2 * n] = (float)(fabs((double)l[2 * n - 2]) - c[n - 1]);
                    l[2 * n + 1] = (float)(fabs((double)l[2 * n - 1]) - c[n - 1]);
                }
            }
            int wrong = 0, m = 0;
            for (int u = 0; u < mod_type; ++u) {
                const long pos = (long)mod_type * sy + u;
                const int p = (int)(pos % N);
                m = (int)(pos / N); /* the same for every u: mod_type divides n_var */
                const int k = (N / I) * (p % I) + p / I;
                if (k >= k_lim) continue;
                const int b = s ? (int)s[k < K ? (size_t)m * K + k : (size_t)32 * K + (size_t)m * M + (k - K)] : 0;
                const int d = l[u] > 0.0f ? 1 : 0;
                wrong += d != b ? 1 : 0;
            }
            frame_bits[m] += (uint64_t)wrong;
            sym_err += wrong ? 1u : 0u;
        }
        out[0] += LNSFAID_GROUP;
        for (int m = 0; m < 32; ++m) { out[1] += frame_bits[m] ? 1u : 0u; out[2] += frame_bits[m]; }
        out[3] += sym_err;
    }
    return LNSFAID_OK;
}

/* ---- error-frame capture (lnsfaid_capture.hip) ---------------------------------------------- */
static int capture_rules(size_t n_groups, size_t capacity, const int8_t* decodedBits, const lnsfaid_error_record* records,
                         const int8_t* payload, const uint64_t* found, const uint64_t* stored)
{
    if (n_groups == 0) return LNSFAID_OK;
    if (!decodedBits || !found || !stored) return LNSFAID_E_INVAL;
    if (capacity > 0 && (!records || !payload)) return LNSFAID_E_INVAL;
    return LNSFAID_OK;
}

/* staging for `slots` records; what a smaller call left is kept */
static int capture_buffers(lnsfaid_ctx* ctx, size_t slots)
{
    /* each on its own: a call after a failed allocation asks again for what is still missing */
    if (!ctx->d_cap_cnt) HIP_TRY(hipMalloc(&ctx->d_cap_cnt, ctx->max_groups * LNSFAID_GROUP * sizeof(uint2)));
    if (!ctx->d_cap_meta) HIP_TRY(hipMalloc(&ctx->d_cap_meta, 6 * sizeof(unsigned long long)));
    if (!ctx->h_cap_meta) HIP_TRY(hipHostMalloc((void**)&ctx->h_cap_meta, 6 * sizeof(unsigned long long), hipHostMallocDefault));
    if (slots > ctx->cap_slots) {
        { const int rcw = stream_wait(ctx); if (rcw) return rcw; } /* nothing queued may still use the old buffers */
        (void)hipFree(ctx->d_cap_slots); (void)hipFree(ctx->d_cap_records); (void)hipFree(ctx->d_cap_payload);
        ctx->d_cap_slots = nullptr; ctx->d_cap_records = nullptr; ctx->d_cap_payload = nullptr;
        ctx->cap_slots = 0;
        HIP_TRY(hipMalloc(&ctx->d_cap_slots, slots * sizeof(uint32_t)));
        HIP_TRY(hipMalloc(&ctx->d_cap_records, slots * sizeof(lnsfaid_error_record)));
        HIP_TRY(hipMalloc(&ctx->d_cap_payload, slots * 3 * (size_t)ctx->n_var));
        ctx->cap_slots = slots;
    }
    return LNSFAID_OK;
}

extern "C" int lnsfaid_capture_errors_device(lnsfaid_ctx* ctx, const int8_t* d_fixInput, const int8_t* d_decodedBits, const int8_t* d_sent,
                                             size_t n_groups, size_t skip, size_t capacity, lnsfaid_error_record* records,
                                             int8_t* payload, uint64_t* found, uint64_t* stored, uint64_t out[4])
{
    if (!ctx || n_groups > ctx->max_groups) return LNSFAID_E_INVAL;
    { const int rc = capture_rules(n_groups, capacity, d_decodedBits, records, payload, found, stored); if (rc) return rc; }
    if (n_groups == 0) {
        if (found) *found = 0;
        if (stored) *stored = 0;
        return LNSFAID_OK;
    }
    const size_t n_cw = n_groups * LNSFAID_GROUP; /* 32 * max_groups codewords fit 32 bits: create refuses more */
    if (n_cw > 0xffffffffull) return LNSFAID_E_INVAL;
    const size_t slots = capacity < n_cw ? capacity : n_cw;
    HIP_TRY(hipSetDevice(ctx->device));
    { const int rc = capture_buffers(ctx, slots); if (rc) return rc; }
    HIP_TRY(hipMemsetAsync(ctx->d_cap_meta, 0, 6 * sizeof(unsigned long long), ctx->stream));
    /* no error frame has a rank of n_cw or more: a larger skip stores as little */
    HIP_TRY(lf_launch_capture(d_fixInput, d_decodedBits, d_sent, n_groups, ctx->n_var, ctx->n_check, (uint32_t)(skip < n_cw ? skip : n_cw),
                              (uint32_t)slots, ctx->d_cap_cnt, ctx->d_cap_slots, ctx->d_cap_records, ctx->d_cap_payload, ctx->d_cap_meta,
                              ctx->d_cap_meta + 2, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->h_cap_meta, ctx->d_cap_meta, 6 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    { const int rcw = stream_wait(ctx); if (rcw) return rcw; } /* the one wait that tells the host how much to copy */
    const size_t n_found = (size_t)ctx->h_cap_meta[0], n_stored = (size_t)ctx->h_cap_meta[1];
    if (n_stored > slots) return LNSFAID_E_INTERNAL;
    if (n_stored) {
        HIP_TRY(hipMemcpyAsync(records, ctx->d_cap_records, n_stored * sizeof(lnsfaid_error_record), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(payload, ctx->d_cap_payload, n_stored * 3 * (size_t)ctx->n_var, hipMemcpyDeviceToHost, ctx->stream));
        { const int rcw = stream_wait(ctx); if (rcw) return rcw; }
    }
    *found = n_found;
    *stored = n_stored;
    if (out) for (int i = 0; i < 4; ++i) out[i] += ctx->h_cap_meta[2 + i];
    return LNSFAID_OK;
}

/* The definition of include/lnsfaid.h taken literally (no HIP call): the reference of the device path */
extern "C" int lnsfaid_capture_errors_host(int32_t n_var, int32_t n_check, const int8_t* fixInput, const int8_t* decodedBits,
                                           const int8_t* sent, size_t n_groups, size_t skip, size_t capacity, lnsfaid_error_record* records,
                                           int8_t* payload, uint64_t* found, uint64_t* stored, uint64_t out[4])
{
    if (n_check <= 0 || n_var <= n_check) return LNSFAID_E_INVAL;
    { const int rc = capture_rules(n_groups, capacity, decodedBits, records, payload, found, stored); if (rc) return rc; }
    if (n_groups == 0) {
        if (found) *found = 0;
        if (stored) *stored = 0;
        return LNSFAID_OK;
    }
    const size_t N = (size_t)n_var, M = (size_t)n_check, K = N - M;
    uint64_t n_found = 0, n_stored = 0, add[4] = { 0, 0, 0, 0 };
    for (size_t g = 0; g < n_groups; ++g) {
        const int8_t* sg = sent ? sent + g * 32 * N : nullptr;
        const int8_t* fg = fixInput ? fixInput + g * 32 * N : nullptr;
        add[0] += LNSFAID_GROUP;
        for (size_t m = 0; m < 32; ++m) {
            const int8_t* d = decodedBits + (g * 32 + m) * N;
            const size_t info_at = m * K, parity_at = 32 * K + m * M;
            uint32_t info = 0, parity = 0;
            for (size_t k = 0; k < K; ++k) info += d[k] != (sg ? sg[info_at + k] : 0) ? 1u : 0u;
            if (info == 0) continue;
            add[1] += 1; add[2] += info; add[3] += info < 3 ? 1u : 0u;
            const uint64_t rank = n_found++;
            if (rank < skip || rank - skip >= capacity) continue;
            for (size_t k = 0; k < M; ++k) parity += d[K + k] != (sg ? sg[parity_at + k] : 0) ? 1u : 0u;
            lnsfaid_error_record& r = records[n_stored];
            r.codeword = (uint32_t)(g * 32 + m); r.info_errors = info; r.parity_errors = parity; r.reserved = 0;
            int8_t* p = payload + n_stored * 3 * N;
            for (size_t k = 0; k < N; ++k) {
                const size_t at = k < K ? info_at + k : parity_at + (k - K);
                p[k] = fg ? fg[at] : (int8_t)0;
                p[N + k] = d[k];
                p[2 * N + k] = sg ? sg[at] : (int8_t)0;
            }
            ++n_stored;
        }
    }
    *found = n_found;
    *stored = n_stored;
    if (out) for (int i = 0; i < 4; ++i) out[i] += add[i];
    return LNSFAID_OK;
}

/* ---- FEC status (lnsfaid_fecstatus.hip; the host forms are in lnsfaid_tables.c) ------------------------- */
static int fec_status_device(lnsfaid_ctx* ctx, int packed, const void* d_fix, const void* d_decided, const int8_t* d_sent, size_t n_groups,
                             lnsfaid_fec_record* d_records, uint64_t out[4], uint64_t vs_sent[4])
{
    if (!ctx || n_groups > ctx->max_groups) return LNSFAID_E_INVAL;
    if (packed && ctx->n_var % 32 != 0) return LNSFAID_E_INVAL;
    if (n_groups == 0) return LNSFAID_OK;
    if (!d_decided || n_groups * LNSFAID_GROUP > 0xffffffffull) return LNSFAID_E_INVAL;
    HIP_TRY(hipSetDevice(ctx->device));
    /* each on its own: a call after a failed allocation asks again for what is still missing */
    if (!ctx->d_fec_acc) HIP_TRY(hipMalloc(&ctx->d_fec_acc, 8 * sizeof(unsigned long long)));
    if (!ctx->h_fec_acc) HIP_TRY(hipHostMalloc((void**)&ctx->h_fec_acc, 8 * sizeof(unsigned long long), hipHostMallocDefault));
    HIP_TRY(hipMemsetAsync(ctx->d_fec_acc, 0, 8 * sizeof(unsigned long long), ctx->stream));
    HIP_TRY(lf_launch_fec_status(ctx->d_code, ctx->n_var, packed, d_fix, d_decided, vs_sent ? d_sent : nullptr, n_groups, d_records,
                                 vs_sent ? 1 : 0, ctx->d_fec_acc, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->h_fec_acc, ctx->d_fec_acc, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    { const int rcw = stream_wait(ctx); if (rcw) return rcw; }
    if (out) for (int i = 0; i < 4; ++i) out[i] += ctx->h_fec_acc[i];
    if (vs_sent) for (int i = 0; i < 4; ++i) vs_sent[i] += ctx->h_fec_acc[4 + i];
    return LNSFAID_OK;
}

extern "C" int lnsfaid_fec_status_device(lnsfaid_ctx* ctx, const int8_t* d_fixInput, const int8_t* d_decodedBits, const int8_t* d_sent,
                                         size_t n_groups, lnsfaid_fec_record* d_records, uint64_t out[4], uint64_t vs_sent[4])
{
    return fec_status_device(ctx, 0, d_fixInput, d_decodedBits, d_sent, n_groups, d_records, out, vs_sent);
}

extern "C" int lnsfaid_fec_status_packed_device(lnsfaid_ctx* ctx, const uint8_t* d_llr4, const uint32_t* d_bits, const int8_t* d_sent,
                                                size_t n_groups, lnsfaid_fec_record* d_records, uint64_t out[4], uint64_t vs_sent[4])
{
    return fec_status_device(ctx, 1, d_llr4, d_bits, d_sent, n_groups, d_records, out, vs_sent);
}

/* ---- systematic encoder (lnsfaid_encoder.hip) ----------------------------------------------
 * B = the last n_check columns of H is block-circulant, so B^-1 is too: one first row per block describes it.  Rows a z of
 * B^-1 solve B^T x = e_{a z}: one Gauss-Jordan elimination of B^T (bit-packed rows, the mb right-hand sides in one extra
 * word) gives all of them.  0.1 s for the 50G-PON code on one core. */
static int parity_inverse(const LfDevCode& code, uint8_t* circ)
{
    const int Z = LF_Z, M = code.n_check, K = code.k_info, mb = M / Z, kb = K / Z, W = M / 64 + 1; /* mb <= LF_MAX_BR <= 64 */
    std::vector<uint64_t> m;
    try {
        m.assign((size_t)M * W, 0);
    } catch (...) {
        return LNSFAID_E_NOMEM;
    }
    /* row c of B^T = column c of B: block row br, circulant of block column cb >= kb with shift sh has B[br z + i][(cb - kb) z + (sh + i) mod z] */
    for (int br = 0; br < code.nbr; ++br)
        for (int j = 0; j < code.deg[br]; ++j) {
            const int cb = (int)(code.circ[br][j].sb / (uint32_t)Z), sh = (int)(code.circ[br][j].sb % (uint32_t)Z);
            if (cb < kb) continue;
            for (int i = 0; i < Z; ++i) {
                const size_t c = (size_t)(cb - kb) * Z + (size_t)((sh + i) % Z), r = (size_t)br * Z + (size_t)i;
                m[c * W + r / 64] ^= 1ull << (r % 64);
            }
        }
    for (int a = 0; a < mb; ++a) m[(size_t)a * Z * W + (size_t)(W - 1)] |= 1ull << a;
    std::vector<uint64_t> tmp((size_t)W);
    for (int col = 0; col < M; ++col) {
        const size_t w = (size_t)col / 64;
        const uint64_t bit = 1ull << (col % 64);
        int piv = -1;
        for (int r = col; r < M; ++r)
            if (m[(size_t)r * W + w] & bit) { piv = r; break; }
        if (piv < 0) return LNSFAID_E_CODE; /* singular */
        if (piv != col) {
            memcpy(tmp.data(), &m[(size_t)col * W], sizeof(uint64_t) * W);
            memcpy(&m[(size_t)col * W], &m[(size_t)piv * W], sizeof(uint64_t) * W);
            memcpy(&m[(size_t)piv * W], tmp.data(), sizeof(uint64_t) * W);
        }
        const uint64_t* prow = &m[(size_t)col * W];
        for (int r = 0; r < M; ++r) {
            uint64_t* row = &m[(size_t)r * W];
            if (r == col || !(row[w] & bit)) continue;
            for (size_t x = w; x < (size_t)W; ++x) row[x] ^= prow[x]; /* words left of the pivot are zero in prow */
        }
    }
    /* row r now holds x_r: bit a = entry (a z, r) of B^-1 */
    memset(circ, 0, (size_t)mb * mb * (Z / 8));
    for (int a = 0; a < mb; ++a)
        for (int r = 0; r < M; ++r)
            if ((m[(size_t)r * W + (size_t)(W - 1)] >> a) & 1u) {
                const int b = r / Z, c = r % Z;
                circ[((size_t)a * mb + (size_t)b) * (Z / 8) + (size_t)(c / 8)] |= (uint8_t)(1u << (c % 8));
            }
    return LNSFAID_OK;
}

extern "C" int lnsfaid_code_parity_inverse(const lnsfaid_code* code, uint8_t* circ, size_t bytes)
{
    if (!code || !circ) return LNSFAID_E_INVAL;
    LfDevCode* c = new (std::nothrow) LfDevCode(); /* ~90 KiB: not on the caller's stack */
    if (!c) return LNSFAID_E_NOMEM;
    int rc = build_code(code, c);
    if (!rc) {
        const size_t mb = (size_t)c->nbr;
        rc = bytes < mb * mb * (LF_Z / 8) ? LNSFAID_E_INVAL : parity_inverse(*c, circ);
    }
    delete c;
    return rc;
}

/* B^-1 of the context's code on the device, derived at the first call that needs it; a singular parity part is remembered */
static int ensure_encoder(lnsfaid_ctx* ctx)
{
    if (ctx->enc_state == 1) return LNSFAID_OK;
    if (ctx->enc_state < 0) return ctx->enc_state;
    const int mb = ctx->hcode.nbr, Z = LF_Z;
    std::vector<uint8_t> circ;
    std::vector<uint32_t> sup, off;
    try {
        circ.assign((size_t)mb * mb * (Z / 8), 0);
        off.reserve((size_t)mb + 1);
        sup.reserve((size_t)mb * mb * Z / 2);
    } catch (...) {
        return LNSFAID_E_NOMEM;
    }
    const int rc = parity_inverse(ctx->hcode, circ.data());
    if (rc == LNSFAID_E_CODE) ctx->enc_state = rc;
    if (rc) return rc;
    off.push_back(0);
    for (int a = 0; a < mb; ++a) {
        for (int b = 0; b < mb; ++b)
            for (int c = 0; c < Z; ++c)
                if ((circ[((size_t)a * mb + (size_t)b) * (Z / 8) + (size_t)(c / 8)] >> (c % 8)) & 1u) sup.push_back((uint32_t)(b * Z + c));
        off.push_back((uint32_t)sup.size());
    }
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMalloc(&ctx->d_enc_sup, sup.size() * sizeof(uint32_t)));
    HIP_TRY(hipMalloc(&ctx->d_enc_off, off.size() * sizeof(uint32_t)));
    HIP_TRY(hipMemcpy(ctx->d_enc_sup, sup.data(), sup.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ctx->d_enc_off, off.data(), off.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    ctx->enc_state = 1;
    return LNSFAID_OK;
}

extern "C" int lnsfaid_encode_device(lnsfaid_ctx* ctx, const int8_t* d_inputBits, size_t n_groups, int8_t* d_outputBits)
{
    if (!ctx || (n_groups && (!d_inputBits || !d_outputBits)) || n_groups > ctx->max_groups) return LNSFAID_E_INVAL;
    if (n_groups == 0) return LNSFAID_OK;
    const int rc = ensure_encoder(ctx);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(lf_launch_encode(ctx->d_code, ctx->n_check, ctx->d_enc_sup, ctx->d_enc_off, d_inputBits, nullptr, n_groups, d_outputBits,
                             nullptr, ctx->stream));
    return stream_wait(ctx);
}

extern "C" int lnsfaid_encode(lnsfaid_ctx* ctx, const int8_t* inputBits, size_t n_groups, int8_t* outputBits)
{
    if (!ctx || (n_groups && (!inputBits || !outputBits)) || n_groups > ctx->max_groups) return LNSFAID_E_INVAL;
    if (n_groups == 0) return LNSFAID_OK;
    int rc = ensure_encoder(ctx);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    rc = ensure_io(ctx);
    if (rc) return rc;
    /* the staging buffers of the decode path: [32][K] per group fits in the fixInput buffer */
    HIP_TRY(hipMemcpyAsync(ctx->d_io_in, inputBits, n_groups * LNSFAID_GROUP * (size_t)ctx->k_info, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(lf_launch_encode(ctx->d_code, ctx->n_check, ctx->d_enc_sup, ctx->d_enc_off, ctx->d_io_in, nullptr, n_groups, ctx->d_io_out,
                             nullptr, ctx->stream));
    HIP_TRY(hipMemcpyAsync(outputBits, ctx->d_io_out, n_groups * LNSFAID_GROUP * (size_t)ctx->n_var, hipMemcpyDeviceToHost, ctx->stream));
    return stream_wait(ctx);
}

/* ---- line-format encode (include/lnsfaid.h "line-format encode", DESIGN.md 3.15, lnsfaid_encoder_line.hip) ---------------- */
/* everything that can be refused without looking at the buffers; 1: nothing to do.  Nothing of the decoder configuration. */
static int encode_line_rules(const lnsfaid_ctx* ctx, size_t n_codewords)
{
    if (!ctx) return LNSFAID_E_INVAL;
    const int L = ctx->n_var - ctx->hcode.puncture_tail;
    if (L % 32 != 0 || ctx->k_info % 32 != 0 || ctx->n_var % 32 != 0 || L < ctx->k_info) return LNSFAID_E_INVAL;
    if (n_codewords > ctx->max_groups * LNSFAID_GROUP) return LNSFAID_E_INVAL;
    return n_codewords == 0 ? 1 : LNSFAID_OK;
}

extern "C" int lnsfaid_encode_line_device(lnsfaid_ctx* ctx, const uint32_t* d_payload, size_t n_codewords, uint32_t* d_line, uint32_t* d_bits)
{
    int rc = encode_line_rules(ctx, n_codewords);
    if (rc) return rc < 0 ? rc : LNSFAID_OK;
    if (!d_payload || !d_line) return LNSFAID_E_INVAL;
    if (!dword_aligned(d_payload) || !dword_aligned(d_line) || !dword_aligned(d_bits)) return LNSFAID_E_INVAL;
    rc = ensure_encoder(ctx);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(lf_launch_encode_line(ctx->d_code, ctx->n_check, ctx->d_enc_sup, ctx->d_enc_off, d_payload, n_codewords, d_line, d_bits,
                                  ctx->stream));
    return stream_wait(ctx);
}

/* host buffers of any alignment: one copy each way through the packed staging buffers, on the context's own stream.  d_pk_in
 * (n_var / 2 bytes per codeword) holds the payload of 32 * max_groups codewords and, behind it, their line; d_pk_out their bits. */
extern "C" int lnsfaid_encode_line(lnsfaid_ctx* ctx, const uint32_t* payload, size_t n_codewords, uint32_t* line, uint32_t* bits)
{
    int rc = encode_line_rules(ctx, n_codewords);
    if (rc) return rc < 0 ? rc : LNSFAID_OK;
    if (!payload || !line) return LNSFAID_E_INVAL;
    rc = ensure_encoder(ctx);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    rc = ensure_packed_io(ctx);
    if (rc) return rc;
    const size_t k_bytes = (size_t)ctx->k_info / 8, n_bytes = (size_t)ctx->n_var / 8;
    const size_t l_bytes = (size_t)(ctx->n_var - ctx->hcode.puncture_tail) / 8;
    uint32_t* d_payload = (uint32_t*)ctx->d_pk_in;
    uint32_t* d_line = (uint32_t*)(ctx->d_pk_in + ctx->max_groups * LNSFAID_GROUP * k_bytes); /* a multiple of 128 bytes in */
    HIP_TRY(hipMemcpyAsync(d_payload, payload, n_codewords * k_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(lf_launch_encode_line(ctx->d_code, ctx->n_check, ctx->d_enc_sup, ctx->d_enc_off, d_payload, n_codewords, d_line,
                                  bits ? ctx->d_pk_out : nullptr, ctx->stream));
    HIP_TRY(hipMemcpyAsync(line, d_line, n_codewords * l_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (bits) HIP_TRY(hipMemcpyAsync(bits, ctx->d_pk_out, n_codewords * n_bytes, hipMemcpyDeviceToHost, ctx->stream));
    return stream_wait(ctx);
}

/* ---- burst-format line calls (include/lnsfaid.h "burst-format line calls", DESIGN.md 3.18, lnsfaid_kernel4b.hip,
 * lnsfaid_encoder_burst.hip; host forms in lnsfaid_tables.c) ----------------------------------------------------------------- */
static bool shorten_where_ok(int32_t where) { return where == LNSFAID_SHORTEN_TAIL || where == LNSFAID_SHORTEN_HEAD; }

/* `shortened` (a host pointer of any alignment, or NULL) by the rule of the header, and the descriptors of the call: prefix sums
 * into the context's pinned array, one copy on its stream into its device array.  The totals are in words of 32 positions. */
static int burst_descriptors(lnsfaid_ctx* ctx, const uint32_t* shortened, int32_t where, size_t n_codewords, size_t* line_units,
                             size_t* payload_words)
{
    if (!shorten_where_ok(where)) return LNSFAID_E_INVAL;
    const uint32_t K = (uint32_t)ctx->k_info, L = (uint32_t)(ctx->n_var - ctx->hcode.puncture_tail);
    if (ctx->n_var % 32 != 0 || L < K) return LNSFAID_E_INVAL;
    for (size_t c = 0; shortened && c < n_codewords; ++c) {
        uint32_t s;
        memcpy(&s, (const uint8_t*)shortened + 4 * c, 4);
        if (s % 32u != 0u || (uint64_t)s + 32u > K) return LNSFAID_E_INVAL;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    if (!ctx->d_burst_desc) {
        const size_t bytes = ctx->max_groups * LNSFAID_GROUP * sizeof(LfBurstDesc);
        HIP_TRY(hipHostMalloc((void**)&ctx->h_burst_desc, bytes, hipHostMallocDefault));
        HIP_TRY(hipMalloc(&ctx->d_burst_desc, bytes));
    }
    uint32_t lo = 0, po = 0; /* at most 65 536 codewords of L / 32 words each: below 2^26 */
    for (size_t c = 0; c < n_codewords; ++c) {
        uint32_t s = 0;
        if (shortened) memcpy(&s, (const uint8_t*)shortened + 4 * c, 4);
        ctx->h_burst_desc[c] = LfBurstDesc{ lo, po, s / 32u, 0u };
        lo += (L - s) / 32u;
        po += (K - s) / 32u;
    }
    HIP_TRY(hipMemcpyAsync(ctx->d_burst_desc, ctx->h_burst_desc, n_codewords * sizeof(LfBurstDesc), hipMemcpyHostToDevice, ctx->stream));
    *line_units = lo;
    *payload_words = po;
    return LNSFAID_OK;
}

/* decode_line_launch with the descriptors: one launch, one wait */
static int decode_burst_launch(lnsfaid_ctx* ctx, const void* d_line, int32_t format, int32_t magnitude, int32_t where, size_t n_codewords,
                               uint32_t* d_payload, uint32_t* d_bits, lnsfaid_line_stats* d_stats, uint32_t* d_short_ones)
{
    LfInst k;
    {
        const int rc = kernel_check(ctx, LF_ENTRY_BURST, &k);
        if (rc) return rc;
    }
    LfBurstArgs a;
    a.code = ctx->d_code; a.cfg = ctx->d_cfg;
    a.line = d_line; a.payload = d_payload; a.bits = d_bits;
    a.st_rows = ctx->d_rows;
    a.stats = d_stats; a.short_ones = d_short_ones;
    a.desc = ctx->d_burst_desc;
    a.format = format; a.magnitude = magnitude; a.where = where; a.n_cw = (int32_t)n_codewords;
    return launch_decode_timed(ctx, k, &a, n_codewords, "burst");
}

extern "C" int lnsfaid_decode_burst_device(lnsfaid_ctx* ctx, const void* d_line, int32_t format, int32_t magnitude, const uint32_t* shortened,
                                           int32_t where, size_t n_codewords, uint32_t* d_payload, uint32_t* d_bits,
                                           lnsfaid_line_stats* d_stats, uint32_t* d_short_ones)
{
    int rc = line_rules(ctx, format, magnitude, n_codewords);
    if (rc < 0) return rc;
    if (!shorten_where_ok(where)) return LNSFAID_E_INVAL;
    if (rc) return LNSFAID_OK;
    if (!d_line || !d_payload) return LNSFAID_E_INVAL;
    if (!dword_aligned(d_line) || !dword_aligned(d_payload) || !dword_aligned(d_bits) || !dword_aligned(d_stats) || !dword_aligned(d_short_ones))
        return LNSFAID_E_INVAL;
    size_t lu, pw;
    rc = burst_descriptors(ctx, shortened, where, n_codewords, &lu, &pw);
    if (rc) return rc;
    return decode_burst_launch(ctx, d_line, format, magnitude, where, n_codewords, d_payload, d_bits, d_stats, d_short_ones);
}

/* host buffers of any alignment: one copy each way through the staging buffers of lnsfaid_decode_line */
extern "C" int lnsfaid_decode_burst(lnsfaid_ctx* ctx, const void* line, int32_t format, int32_t magnitude, const uint32_t* shortened,
                                    int32_t where, size_t n_codewords, uint32_t* payload, uint32_t* bits, lnsfaid_line_stats* stats,
                                    uint32_t* short_ones)
{
    int rc = line_rules(ctx, format, magnitude, n_codewords);
    if (rc < 0) return rc;
    if (!shorten_where_ok(where)) return LNSFAID_E_INVAL;
    if (rc) return LNSFAID_OK;
    if (!line || !payload) return LNSFAID_E_INVAL;
    size_t lu, pw;
    rc = burst_descriptors(ctx, shortened, where, n_codewords, &lu, &pw);
    if (rc) return rc;
    rc = ensure_packed_io(ctx);
    if (rc) return rc;
    if (!ctx->d_ln_payload) {
        HIP_TRY(hipMalloc(&ctx->d_ln_payload, ctx->max_groups * LNSFAID_GROUP * (size_t)ctx->k_info / 8));
        HIP_TRY(hipMalloc(&ctx->d_ln_stats, ctx->max_groups * LNSFAID_GROUP * sizeof(lnsfaid_line_stats)));
    }
    if (!ctx->d_burst_ones) HIP_TRY(hipMalloc(&ctx->d_burst_ones, ctx->max_groups * LNSFAID_GROUP * sizeof(uint32_t)));
    const size_t n_bytes = (size_t)ctx->n_var / 8;
    HIP_TRY(hipMemcpyAsync(ctx->d_pk_in, line, lu * (format == LNSFAID_LINE_HARD ? 4u : 16u), hipMemcpyHostToDevice, ctx->stream));
    rc = decode_burst_launch(ctx, ctx->d_pk_in, format, magnitude, where, n_codewords, ctx->d_ln_payload, bits ? ctx->d_pk_out : nullptr,
                             stats ? ctx->d_ln_stats : nullptr, short_ones ? ctx->d_burst_ones : nullptr);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(payload, ctx->d_ln_payload, pw * 4u, hipMemcpyDeviceToHost, ctx->stream));
    if (bits) HIP_TRY(hipMemcpyAsync(bits, ctx->d_pk_out, n_codewords * n_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (stats)
        HIP_TRY(hipMemcpyAsync(stats, ctx->d_ln_stats, n_codewords * sizeof(lnsfaid_line_stats), hipMemcpyDeviceToHost, ctx->stream));
    if (short_ones) HIP_TRY(hipMemcpyAsync(short_ones, ctx->d_burst_ones, n_codewords * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    return stream_wait(ctx);
}

extern "C" int lnsfaid_encode_burst_device(lnsfaid_ctx* ctx, const uint32_t* d_payload, const uint32_t* shortened, int32_t where,
                                           size_t n_codewords, uint32_t* d_line, uint32_t* d_bits)
{
    int rc = encode_line_rules(ctx, n_codewords);
    if (rc < 0) return rc;
    if (!shorten_where_ok(where)) return LNSFAID_E_INVAL;
    if (rc) return LNSFAID_OK;
    if (!d_payload || !d_line) return LNSFAID_E_INVAL;
    if (!dword_aligned(d_payload) || !dword_aligned(d_line) || !dword_aligned(d_bits)) return LNSFAID_E_INVAL;
    rc = ensure_encoder(ctx);
    if (rc) return rc;
    size_t lu, pw;
    rc = burst_descriptors(ctx, shortened, where, n_codewords, &lu, &pw);
    if (rc) return rc;
    HIP_TRY(lf_launch_encode_burst(ctx->d_code, ctx->n_check, ctx->d_enc_sup, ctx->d_enc_off, d_payload, ctx->d_burst_desc, where,
                                   n_codewords, d_line, d_bits, ctx->stream));
    return stream_wait(ctx);
}

/* host buffers of any alignment, through the packed staging buffers as lnsfaid_encode_line: payload, and behind it the line */
extern "C" int lnsfaid_encode_burst(lnsfaid_ctx* ctx, const uint32_t* payload, const uint32_t* shortened, int32_t where, size_t n_codewords,
                                    uint32_t* line, uint32_t* bits)
{
    int rc = encode_line_rules(ctx, n_codewords);
    if (rc < 0) return rc;
    if (!shorten_where_ok(where)) return LNSFAID_E_INVAL;
    if (rc) return LNSFAID_OK;
    if (!payload || !line) return LNSFAID_E_INVAL;
    rc = ensure_encoder(ctx);
    if (rc) return rc;
    size_t lu, pw;
    rc = burst_descriptors(ctx, shortened, where, n_codewords, &lu, &pw);
    if (rc) return rc;
    rc = ensure_packed_io(ctx);
    if (rc) return rc;
    const size_t k_bytes = (size_t)ctx->k_info / 8, n_bytes = (size_t)ctx->n_var / 8;
    uint32_t* d_payload = (uint32_t*)ctx->d_pk_in;
    uint32_t* d_line = (uint32_t*)(ctx->d_pk_in + ctx->max_groups * LNSFAID_GROUP * k_bytes);
    HIP_TRY(hipMemcpyAsync(d_payload, payload, pw * 4u, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(lf_launch_encode_burst(ctx->d_code, ctx->n_check, ctx->d_enc_sup, ctx->d_enc_off, d_payload, ctx->d_burst_desc, where,
                                   n_codewords, d_line, bits ? ctx->d_pk_out : nullptr, ctx->stream));
    HIP_TRY(hipMemcpyAsync(line, d_line, lu * 4u, hipMemcpyDeviceToHost, ctx->stream));
    if (bits) HIP_TRY(hipMemcpyAsync(bits, ctx->d_pk_out, n_codewords * n_bytes, hipMemcpyDeviceToHost, ctx->stream));
    return stream_wait(ctx);
}

/* ---- line-format link (include/lnsfaid.h "line-format link", DESIGN.md 3.16, lnsfaid_line_link.hip; host forms in lnsfaid_tables.c) -- */
#define LF_LINK_ACC 14 /* twelve counters, the flipped bits and the runs of the error-propagation channel */
/* everything that can be refused without looking at the buffers; 1: nothing to do.  Nothing of the decoder configuration. */
static int line_link_rules(const lnsfaid_ctx* ctx, size_t n_codewords)
{
    if (!ctx) return LNSFAID_E_INVAL;
    const int L = ctx->n_var - ctx->hcode.puncture_tail;
    if (L <= 0 || L % 32 != 0 || ctx->k_info <= 0 || ctx->k_info % 32 != 0) return LNSFAID_E_INVAL;
    if (n_codewords > ctx->max_groups * LNSFAID_GROUP || n_codewords > 0x7fffffffull) return LNSFAID_E_INVAL;
    return n_codewords == 0 ? 1 : LNSFAID_OK;
}

/* each on its own: a call after a failed allocation asks again for what is still missing */
static int ensure_link_acc(lnsfaid_ctx* ctx)
{
    if (!ctx->d_link_acc) HIP_TRY(hipMalloc(&ctx->d_link_acc, LF_LINK_ACC * sizeof(unsigned long long)));
    if (!ctx->h_link_acc) HIP_TRY(hipHostMalloc((void**)&ctx->h_link_acc, LF_LINK_ACC * sizeof(unsigned long long), hipHostMallocDefault));
    return LNSFAID_OK;
}

/* the soft channels' table: non-decreasing */
static bool soft_table_ok(const uint32_t table[14])
{
    for (int i = 1; i < 14; ++i)
        if (table[i] < table[i - 1]) return false;
    return true;
}

/* A channel call's n totals (1: flips; 2: flips and runs), accumulators 12 and 13: zeroed on the stream in front of the launch ... */
static unsigned long long* link_totals(const lnsfaid_ctx* ctx) { return ctx->d_link_acc + 12; }
static int link_totals_begin(lnsfaid_ctx* ctx, int n)
{
    const int rc = ensure_link_acc(ctx);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(link_totals(ctx), 0, n * sizeof(unsigned long long), ctx->stream));
    return LNSFAID_OK;
}

/* ... and behind it copied back if one is asked for, waited for and ADDED to what the caller holds */
static int link_totals_end(lnsfaid_ctx* ctx, int n, uint64_t* total_flips, uint64_t* total_runs)
{
    if (total_flips || total_runs)
        HIP_TRY(hipMemcpyAsync(ctx->h_link_acc + 12, link_totals(ctx), n * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    const int rc = stream_wait(ctx);
    if (rc) return rc;
    if (total_flips) *total_flips += ctx->h_link_acc[12];
    if (total_runs) *total_runs += ctx->h_link_acc[13];
    return LNSFAID_OK;
}

/* The counter call of either format, the rules checked and the device set: twelve counters zeroed, counted (d_desc: the burst's
 * uploaded descriptors, null for a line), copied back, waited for and ADDED into errors / fec / vs_sent, each of which may be null. */
static int link_count_run(lnsfaid_ctx* ctx, const uint32_t* d_payload, const uint32_t* d_sent, const lnsfaid_line_stats* d_stats,
                          const uint32_t* d_short_ones, const LfBurstDesc* d_desc, size_t n_codewords, uint64_t errors[4], uint64_t fec[4],
                          uint64_t vs_sent[4])
{
    int rc = ensure_link_acc(ctx);
    if (rc) return rc;
    const uint32_t kw = (uint32_t)ctx->k_info / 32u;
    HIP_TRY(hipMemsetAsync(ctx->d_link_acc, 0, 12 * sizeof(unsigned long long), ctx->stream));
    if (d_desc)
        HIP_TRY(lf_launch_burst_count(d_payload, d_sent, d_stats, d_short_ones, d_desc, n_codewords, kw, ctx->d_link_acc, ctx->stream));
    else
        HIP_TRY(lf_launch_line_count(d_payload, d_sent, d_stats, n_codewords, kw, ctx->d_link_acc, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->h_link_acc, ctx->d_link_acc, 12 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    rc = stream_wait(ctx);
    if (rc) return rc;
    for (int i = 0; i < 4; ++i) {
        if (errors) errors[i] += ctx->h_link_acc[i];
        if (fec) fec[i] += ctx->h_link_acc[4 + i];
        if (vs_sent) vs_sent[i] += ctx->h_link_acc[8 + i];
    }
    return LNSFAID_OK;
}

extern "C" int lnsfaid_line_payload_random_device(lnsfaid_ctx* ctx, uint64_t key, uint64_t first_codeword, size_t n_codewords,
                                                  uint32_t* d_payload)
{
    const int rc = line_link_rules(ctx, n_codewords);
    if (rc) return rc < 0 ? rc : LNSFAID_OK;
    if (!d_payload || !dword_aligned(d_payload)) return LNSFAID_E_INVAL;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(lf_launch_line_payload(d_payload, n_codewords, (uint32_t)ctx->k_info / 32u, key, first_codeword, ctx->stream));
    return stream_wait(ctx);
}

extern "C" int lnsfaid_line_bsc_device(lnsfaid_ctx* ctx, const uint32_t* d_line_in, size_t n_codewords, uint64_t key, uint64_t first_codeword,
                                       uint32_t threshold, uint32_t* d_line_out, uint32_t* d_flips, uint64_t* total_flips)
{
    int rc = line_link_rules(ctx, n_codewords);
    if (rc) return rc < 0 ? rc : LNSFAID_OK;
    if (!d_line_in || !d_line_out) return LNSFAID_E_INVAL;
    if (!dword_aligned(d_line_in) || !dword_aligned(d_line_out) || !dword_aligned(d_flips)) return LNSFAID_E_INVAL;
    HIP_TRY(hipSetDevice(ctx->device));
    rc = link_totals_begin(ctx, 1);
    if (rc) return rc;
    HIP_TRY(lf_launch_line_bsc(d_line_in, d_line_out, n_codewords, (uint32_t)(ctx->n_var - ctx->hcode.puncture_tail) / 32u, key, first_codeword,
                               threshold, d_flips, link_totals(ctx), ctx->stream));
    return link_totals_end(ctx, 1, total_flips, nullptr);
}

extern "C" int lnsfaid_line_count_errors_device(lnsfaid_ctx* ctx, const uint32_t* d_payload, const uint32_t* d_sent,
                                                const lnsfaid_line_stats* d_stats, size_t n_codewords, uint64_t errors[4], uint64_t fec[4],
                                                uint64_t vs_sent[4])
{
    const int rc = line_link_rules(ctx, n_codewords);
    if (rc) return rc < 0 ? rc : LNSFAID_OK;
    if (!d_payload || ((fec || vs_sent) && !d_stats)) return LNSFAID_E_INVAL;
    if (!dword_aligned(d_payload) || !dword_aligned(d_sent) || !dword_aligned(d_stats)) return LNSFAID_E_INVAL;
    HIP_TRY(hipSetDevice(ctx->device));
    return link_count_run(ctx, d_payload, d_sent, d_stats, nullptr, nullptr, n_codewords, errors, fec, vs_sent);
}

/* ---- line-format soft channel (include/lnsfaid.h "line-format soft channel", DESIGN.md 3.17, lnsfaid_line_soft.hip) ---- */
extern "C" int lnsfaid_line_soft_device(lnsfaid_ctx* ctx, const uint32_t* d_line_in, size_t n_codewords, uint64_t key, uint64_t first_codeword,
                                        const uint32_t table[14], uint8_t* d_llr4_out, uint32_t* d_flips, uint64_t* total_flips)
{
    int rc = line_link_rules(ctx, n_codewords);
    if (rc) return rc < 0 ? rc : LNSFAID_OK;
    if (!d_line_in || !d_llr4_out || !table) return LNSFAID_E_INVAL;
    if (!dword_aligned(d_line_in) || !dword_aligned(d_llr4_out) || !dword_aligned(d_flips)) return LNSFAID_E_INVAL;
    if (!soft_table_ok(table)) return LNSFAID_E_INVAL;
    const size_t l_bits = (size_t)(ctx->n_var - ctx->hcode.puncture_tail);
    const uintptr_t a = (uintptr_t)d_line_in, b = (uintptr_t)d_llr4_out; /* four times the input: no overlap can be right */
    if (a < b + n_codewords * (l_bits / 2) && b < a + n_codewords * (l_bits / 8)) return LNSFAID_E_INVAL;
    HIP_TRY(hipSetDevice(ctx->device));
    rc = link_totals_begin(ctx, 1);
    if (rc) return rc;
    HIP_TRY(lf_launch_line_soft(d_line_in, d_llr4_out, n_codewords, (uint32_t)l_bits / 32u, key, first_codeword, table, d_flips,
                                link_totals(ctx), ctx->stream));
    return link_totals_end(ctx, 1, total_flips, nullptr);
}

/* ---- line-format error-propagation channel (include/lnsfaid.h "line-format error-propagation channel", DESIGN.md 3.20,
 * lnsfaid_line_markov.hip; the host form is in lnsfaid_tables.c) ---- */
extern "C" int lnsfaid_line_markov_device(lnsfaid_ctx* ctx, const uint32_t* d_line_in, size_t n_codewords, uint64_t key, uint64_t first_codeword,
                                          const uint32_t t[3], uint32_t* d_line_out, uint32_t* d_flips, uint32_t* d_runs,
                                          uint64_t* total_flips, uint64_t* total_runs)
{
    int rc = line_link_rules(ctx, n_codewords);
    if (rc) return rc < 0 ? rc : LNSFAID_OK;
    if (!d_line_in || !d_line_out || !t || t[0] > t[1]) return LNSFAID_E_INVAL;
    if (!dword_aligned(d_line_in) || !dword_aligned(d_line_out) || !dword_aligned(d_flips) || !dword_aligned(d_runs)) return LNSFAID_E_INVAL;
    HIP_TRY(hipSetDevice(ctx->device));
    rc = link_totals_begin(ctx, 2); /* [0] flips, [1] runs */
    if (rc) return rc;
    HIP_TRY(lf_launch_line_markov(d_line_in, d_line_out, n_codewords, (uint32_t)(ctx->n_var - ctx->hcode.puncture_tail) / 32u, key, first_codeword,
                                  t, d_flips, d_runs, link_totals(ctx), ctx->stream));
    return link_totals_end(ctx, 2, total_flips, total_runs);
}

/* ---- burst-format link (include/lnsfaid.h "burst-format link", DESIGN.md 3.22, lnsfaid_burst_link.hip; host forms in
 * lnsfaid_tables.c) ----
 * The link's rules and accumulators, the burst calls' descriptors: every refusal comes before the descriptors are uploaded or follows
 * from their totals, so a refused call has launched nothing. */
extern "C" int lnsfaid_burst_payload_random_device(lnsfaid_ctx* ctx, uint64_t key, uint64_t first_codeword, const uint32_t* shortened,
                                                   int32_t where, size_t n_codewords, uint32_t* d_payload)
{
    int rc = line_link_rules(ctx, n_codewords);
    if (rc < 0) return rc;
    if (!shorten_where_ok(where)) return LNSFAID_E_INVAL;
    if (rc) return LNSFAID_OK;
    if (!d_payload || !dword_aligned(d_payload)) return LNSFAID_E_INVAL;
    size_t lu, pw;
    rc = burst_descriptors(ctx, shortened, where, n_codewords, &lu, &pw);
    if (rc) return rc;
    HIP_TRY(lf_launch_burst_payload(d_payload, ctx->d_burst_desc, where, n_codewords, (uint32_t)ctx->k_info / 32u, key, first_codeword,
                                    ctx->stream));
    return stream_wait(ctx);
}

extern "C" int lnsfaid_burst_bsc_device(lnsfaid_ctx* ctx, const uint32_t* d_line_in, const uint32_t* shortened, int32_t where,
                                        size_t n_codewords, uint64_t key, uint64_t first_codeword, uint32_t threshold, uint32_t* d_line_out,
                                        uint32_t* d_flips, uint64_t* total_flips)
{
    int rc = line_link_rules(ctx, n_codewords);
    if (rc < 0) return rc;
    if (!shorten_where_ok(where)) return LNSFAID_E_INVAL;
    if (rc) return LNSFAID_OK;
    if (!d_line_in || !d_line_out) return LNSFAID_E_INVAL;
    if (!dword_aligned(d_line_in) || !dword_aligned(d_line_out) || !dword_aligned(d_flips)) return LNSFAID_E_INVAL;
    size_t lu, pw;
    rc = burst_descriptors(ctx, shortened, where, n_codewords, &lu, &pw);
    if (rc) return rc;
    rc = link_totals_begin(ctx, 1);
    if (rc) return rc;
    HIP_TRY(lf_launch_burst_bsc(d_line_in, d_line_out, ctx->d_burst_desc, where, n_codewords,
                                (uint32_t)(ctx->n_var - ctx->hcode.puncture_tail) / 32u, (uint32_t)ctx->k_info / 32u, key, first_codeword,
                                threshold, d_flips, link_totals(ctx), ctx->stream));
    return link_totals_end(ctx, 1, total_flips, nullptr);
}

extern "C" int lnsfaid_burst_soft_device(lnsfaid_ctx* ctx, const uint32_t* d_line_in, const uint32_t* shortened, int32_t where,
                                         size_t n_codewords, uint64_t key, uint64_t first_codeword, const uint32_t table[14],
                                         uint8_t* d_llr4_out, uint32_t* d_flips, uint64_t* total_flips)
{
    int rc = line_link_rules(ctx, n_codewords);
    if (rc < 0) return rc;
    if (!shorten_where_ok(where)) return LNSFAID_E_INVAL;
    if (rc) return LNSFAID_OK;
    if (!d_line_in || !d_llr4_out || !table) return LNSFAID_E_INVAL;
    if (!dword_aligned(d_line_in) || !dword_aligned(d_llr4_out) || !dword_aligned(d_flips)) return LNSFAID_E_INVAL;
    if (!soft_table_ok(table)) return LNSFAID_E_INVAL;
    size_t lu, pw;
    rc = burst_descriptors(ctx, shortened, where, n_codewords, &lu, &pw);
    if (rc) return rc;
    const uintptr_t a = (uintptr_t)d_line_in, b = (uintptr_t)d_llr4_out; /* four times the input: no overlap can be right */
    if (a < b + lu * 16u && b < a + lu * 4u) {
        (void)stream_wait(ctx); /* the descriptors' copy: the pinned array is free again for the next call */
        return LNSFAID_E_INVAL;
    }
    rc = link_totals_begin(ctx, 1);
    if (rc) return rc;
    HIP_TRY(lf_launch_burst_soft(d_line_in, d_llr4_out, ctx->d_burst_desc, where, n_codewords,
                                 (uint32_t)(ctx->n_var - ctx->hcode.puncture_tail) / 32u, (uint32_t)ctx->k_info / 32u, key, first_codeword,
                                 table, d_flips, link_totals(ctx), ctx->stream));
    return link_totals_end(ctx, 1, total_flips, nullptr);
}

extern "C" int lnsfaid_burst_count_errors_device(lnsfaid_ctx* ctx, const uint32_t* d_payload, const uint32_t* d_sent,
                                                 const lnsfaid_line_stats* d_stats, const uint32_t* d_short_ones, const uint32_t* shortened,
                                                 size_t n_codewords, uint64_t errors[4], uint64_t fec[4], uint64_t vs_sent[4])
{
    int rc = line_link_rules(ctx, n_codewords);
    if (rc) return rc < 0 ? rc : LNSFAID_OK;
    if (!d_payload || ((fec || vs_sent) && !d_stats)) return LNSFAID_E_INVAL;
    if (!dword_aligned(d_payload) || !dword_aligned(d_sent) || !dword_aligned(d_stats) || !dword_aligned(d_short_ones)) return LNSFAID_E_INVAL;
    size_t lu, pw;
    rc = burst_descriptors(ctx, shortened, LNSFAID_SHORTEN_TAIL, n_codewords, &lu, &pw); /* pay_off and s_words do not depend on `where` */
    if (rc) return rc;
    return link_count_run(ctx, d_payload, d_sent, d_stats, d_short_ones, ctx->d_burst_desc, n_codewords, errors, fec, vs_sent);
}

/* ---- line-format failure capture (include/lnsfaid.h "line-format failure capture", DESIGN.md 3.19, lnsfaid_line_capture.hip; the
 * host form is in lnsfaid_tables.c) ---- */
/* staging for `slots` records of `words` payload words each; what a smaller call left is kept */
static int line_capture_buffers(lnsfaid_ctx* ctx, size_t slots, size_t words)
{
    /* each on its own: a call after a failed allocation asks again for what is still missing */
    if (!ctx->d_lcap_cnt) HIP_TRY(hipMalloc(&ctx->d_lcap_cnt, ctx->max_groups * LNSFAID_GROUP * sizeof(uint4)));
    if (!ctx->d_lcap_meta) HIP_TRY(hipMalloc(&ctx->d_lcap_meta, 2 * sizeof(unsigned long long)));
    if (!ctx->h_lcap_meta) HIP_TRY(hipHostMalloc((void**)&ctx->h_lcap_meta, 2 * sizeof(unsigned long long), hipHostMallocDefault));
    if (slots > ctx->lcap_slots || slots * words > ctx->lcap_words) {
        { const int rcw = stream_wait(ctx); if (rcw) return rcw; } /* nothing queued may still use the old buffers */
        (void)hipFree(ctx->d_lcap_slots); (void)hipFree(ctx->d_lcap_records); (void)hipFree(ctx->d_lcap_payload);
        ctx->d_lcap_slots = nullptr; ctx->d_lcap_records = nullptr; ctx->d_lcap_payload = nullptr;
        ctx->lcap_slots = 0; ctx->lcap_words = 0;
        HIP_TRY(hipMalloc(&ctx->d_lcap_slots, slots * sizeof(uint32_t))); /* slots > 0 here: capacity 0 counts only and needs none */
        HIP_TRY(hipMalloc(&ctx->d_lcap_records, slots * sizeof(lnsfaid_line_failure)));
        HIP_TRY(hipMalloc(&ctx->d_lcap_payload, slots * words * sizeof(uint32_t)));
        ctx->lcap_slots = slots; ctx->lcap_words = slots * words;
    }
    return LNSFAID_OK;
}

extern "C" int lnsfaid_line_capture_device(lnsfaid_ctx* ctx, const void* d_line, int32_t format, const uint32_t* d_bits, const uint32_t* d_sent,
                                           size_t n_codewords, uint64_t first_codeword, int32_t select, size_t skip, size_t capacity,
                                           lnsfaid_line_failure* records, uint32_t* payload, uint64_t* found, uint64_t* stored)
{
    int rc = line_link_rules(ctx, n_codewords);
    if (rc < 0) return rc;
    if (ctx->n_var % 32 != 0 || (format != LNSFAID_LINE_HARD && format != LNSFAID_LINE_LLR4)) return LNSFAID_E_INVAL;
    if (select < 1 || select > 3 || (!d_sent && (select & LNSFAID_LINE_CAPTURE_WRONG))) return LNSFAID_E_INVAL;
    if (rc) { /* n_codewords == 0 */
        if (found) *found = 0;
        if (stored) *stored = 0;
        return LNSFAID_OK;
    }
    if (!d_bits || !found || !stored || (capacity > 0 && (!records || !payload))) return LNSFAID_E_INVAL;
    if (!dword_aligned(d_line) || !dword_aligned(d_bits) || !dword_aligned(d_sent)) return LNSFAID_E_INVAL;
    const size_t l_bits = (size_t)(ctx->n_var - ctx->hcode.puncture_tail);
    const size_t words = (format == LNSFAID_LINE_LLR4 ? l_bits / 8 : l_bits / 32) + 2 * (size_t)(ctx->n_var / 32) + (size_t)(ctx->n_check / 32);
    const size_t slots = capacity < n_codewords ? capacity : n_codewords;
    HIP_TRY(hipSetDevice(ctx->device));
    rc = line_capture_buffers(ctx, slots, words);
    if (rc) return rc;
    /* no failure has a rank of n_codewords or more: a larger skip stores as little */
    HIP_TRY(lf_launch_line_capture(ctx->d_code, ctx->n_var, ctx->hcode.puncture_tail, d_line, format, d_bits, d_sent, n_codewords, first_codeword,
                                   select, (uint32_t)(skip < n_codewords ? skip : n_codewords), (uint32_t)slots, ctx->d_lcap_cnt,
                                   ctx->d_lcap_slots, ctx->d_lcap_records, ctx->d_lcap_payload, ctx->d_lcap_meta, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->h_lcap_meta, ctx->d_lcap_meta, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    rc = stream_wait(ctx); /* the one wait that tells the host how much to copy */
    if (rc) return rc;
    const size_t n_found = (size_t)ctx->h_lcap_meta[0], n_stored = (size_t)ctx->h_lcap_meta[1];
    if (n_stored > slots) return LNSFAID_E_INTERNAL;
    if (n_stored) {
        HIP_TRY(hipMemcpyAsync(records, ctx->d_lcap_records, n_stored * sizeof(lnsfaid_line_failure), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(payload, ctx->d_lcap_payload, n_stored * words * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        rc = stream_wait(ctx);
        if (rc) return rc;
    }
    *found = n_found;
    *stored = n_stored;
    return LNSFAID_OK;
}

extern "C" int lnsfaid_frontend_random_frames(lnsfaid_ctx* ctx, const uint64_t* keys, size_t n_streams)
{
    if (!ctx || (n_streams && !keys) || n_streams > ctx->max_groups) return LNSFAID_E_INVAL;
    if (n_streams == 0) return LNSFAID_OK;
    int rc = ensure_encoder(ctx);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    rc = alloc_fe_frames(ctx);
    if (rc) return rc;
    if (!ctx->d_fe_keys) HIP_TRY(hipMalloc(&ctx->d_fe_keys, ctx->max_groups * sizeof(unsigned long long)));
    HIP_TRY(hipMemcpyAsync(ctx->d_fe_keys, keys, n_streams * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(lf_launch_encode(ctx->d_code, ctx->n_check, ctx->d_enc_sup, ctx->d_enc_off, nullptr, ctx->d_fe_keys, n_streams,
                             ctx->d_fe_frames, ctx->d_fe_input, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream)); /* keys may be reused by the caller */
    ctx->fe_frames_streams = n_streams;
    return LNSFAID_OK;
}

/* ---- multi-GPU: one process (or host thread) per GPU, the four counters summed over RCCL ---------------------------
 * The reference sums its workers' counters on the main thread after pthread_join (main.cpp:174-182); with one context per
 * GPU the same sum is ONE all-reduce of 4 x uint64 on the context's stream.  RCCL is bound at run time - first the copy
 * that is already in the process (a PyTorch process carries its own), then the system library - so that the decode library
 * has no link-time dependency on it and a communicator handed in by the caller belongs to the same RCCL instance. */
struct LfRccl {
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    bool ok = false;
};
static LfRccl* lf_rccl()
{
    static LfRccl r;
    static bool tried = false;
    if (tried) return r.ok ? &r : nullptr;
    tried = true;
    void* h = RTLD_DEFAULT;
    if (!dlsym(RTLD_DEFAULT, "ncclAllReduce")) {
        h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) { snprintf(g_hip_err, sizeof(g_hip_err), "RCCL not found: %s", dlerror()); return nullptr; }
    }
    r.GetUniqueId = (decltype(r.GetUniqueId))dlsym(h, "ncclGetUniqueId");
    r.CommInitRank = (decltype(r.CommInitRank))dlsym(h, "ncclCommInitRank");
    r.CommDestroy = (decltype(r.CommDestroy))dlsym(h, "ncclCommDestroy");
    r.AllReduce = (decltype(r.AllReduce))dlsym(h, "ncclAllReduce");
    r.GetErrorString = (decltype(r.GetErrorString))dlsym(h, "ncclGetErrorString");
    r.ok = r.GetUniqueId && r.CommInitRank && r.CommDestroy && r.AllReduce;
    if (!r.ok) snprintf(g_hip_err, sizeof(g_hip_err), "RCCL symbols missing");
    return r.ok ? &r : nullptr;
}
static int rccl_fail(LfRccl* r, ncclResult_t e, const char* what)
{
    snprintf(g_hip_err, sizeof(g_hip_err), "%s: %s", what, r && r->GetErrorString ? r->GetErrorString(e) : "RCCL error");
    return LNSFAID_E_HIP;
}

extern "C" int lnsfaid_comm_unique_id(uint8_t id[LNSFAID_COMM_ID_BYTES])
{
    if (!id) return LNSFAID_E_INVAL;
    static_assert(LNSFAID_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "id size");
    LfRccl* r = lf_rccl();
    if (!r) return LNSFAID_E_NODEVICE;
    ncclUniqueId u;
    const ncclResult_t e = r->GetUniqueId(&u);
    if (e != ncclSuccess) return rccl_fail(r, e, "ncclGetUniqueId");
    memcpy(id, u.internal, NCCL_UNIQUE_ID_BYTES);
    return LNSFAID_OK;
}

extern "C" int lnsfaid_comm_destroy(lnsfaid_ctx* ctx)
{
    if (!ctx) return LNSFAID_E_INVAL;
    if (ctx->comm && ctx->comm_owned) {
        LfRccl* r = lf_rccl();
        if (r) { (void)hipSetDevice(ctx->device); (void)r->CommDestroy((ncclComm_t)ctx->comm); }
    }
    ctx->comm = nullptr; ctx->comm_owned = false;
    return LNSFAID_OK;
}

extern "C" int lnsfaid_comm_init(lnsfaid_ctx* ctx, int32_t n_ranks, int32_t rank, const uint8_t id[LNSFAID_COMM_ID_BYTES])
{
    if (!ctx || !id || n_ranks < 1 || rank < 0 || rank >= n_ranks) return LNSFAID_E_INVAL;
    LfRccl* r = lf_rccl();
    if (!r) return LNSFAID_E_NODEVICE;
    (void)lnsfaid_comm_destroy(ctx);
    HIP_TRY(hipSetDevice(ctx->device));
    ncclUniqueId u;
    memcpy(u.internal, id, NCCL_UNIQUE_ID_BYTES);
    ncclComm_t c = nullptr;
    const ncclResult_t e = r->CommInitRank(&c, n_ranks, u, rank);
    if (e != ncclSuccess) return rccl_fail(r, e, "ncclCommInitRank");
    ctx->comm = (void*)c; ctx->comm_owned = true;
    return LNSFAID_OK;
}

extern "C" int lnsfaid_comm_attach(lnsfaid_ctx* ctx, void* nccl_comm)
{
    if (!ctx) return LNSFAID_E_INVAL;
    (void)lnsfaid_comm_destroy(ctx);
    ctx->comm = nccl_comm; ctx->comm_owned = false; /* the caller keeps ownership */
    return LNSFAID_OK;
}

extern "C" int lnsfaid_allreduce_counters(lnsfaid_ctx* ctx, uint64_t counters[4])
{
    if (!ctx || !counters) return LNSFAID_E_INVAL;
    if (!ctx->comm) return LNSFAID_E_INVAL; /* lnsfaid_comm_init / lnsfaid_comm_attach first */
    LfRccl* r = lf_rccl();
    if (!r) return LNSFAID_E_NODEVICE;
    HIP_TRY(hipSetDevice(ctx->device));
    if (!ctx->d_reduce) HIP_TRY(hipMalloc(&ctx->d_reduce, 4 * sizeof(unsigned long long)));
    for (int i = 0; i < 4; ++i) ctx->h_counters[i] = counters[i];
    HIP_TRY(hipMemcpyAsync(ctx->d_reduce, ctx->h_counters, 4 * sizeof(unsigned long long), hipMemcpyHostToDevice, ctx->stream));
    const ncclResult_t e = r->AllReduce(ctx->d_reduce, ctx->d_reduce, 4, ncclUint64, ncclSum, (ncclComm_t)ctx->comm, ctx->stream);
    if (e != ncclSuccess) return rccl_fail(r, e, "ncclAllReduce");
    HIP_TRY(hipMemcpyAsync(ctx->h_counters, ctx->d_reduce, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < 4; ++i) counters[i] = ctx->h_counters[i];
    return LNSFAID_OK;
}

/* ---- measurement hooks / misc ---------------------------------------------------------------------- */
extern "C" int lnsfaid_kernel_time(lnsfaid_ctx* ctx, double* out_ms, uint64_t* out_launches, int32_t reset)
{
    if (!ctx) return LNSFAID_E_INVAL;
    if (out_ms) *out_ms = ctx->kernel_ms;
    if (out_launches) *out_launches = ctx->kernel_launches;
    if (reset) { ctx->kernel_ms = 0.0; ctx->kernel_launches = 0; }
    return LNSFAID_OK;
}

extern "C" void* lnsfaid_stream(lnsfaid_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

extern "C" const char* lnsfaid_strerror(int err)
{
    switch (err) {
    case LNSFAID_OK: return "ok";
    case LNSFAID_E_INVAL: return "invalid argument or unsupported configuration";
    case LNSFAID_E_CODE: return "code table is not a supported quasi-cyclic code (Z = 256, degree 2..24, distinct block columns per block row)";
    case LNSFAID_E_NOMEM: return "out of memory";
    case LNSFAID_E_HIP: return "HIP runtime error";
    case LNSFAID_E_NODEVICE: return "no usable GPU";
    case LNSFAID_E_INTERNAL: return "internal error: relaunch loop did not converge";
    default: return "unknown error";
    }
}

extern "C" const char* lnsfaid_last_hip_error(void) { return g_hip_err; }
#ifndef LNSFAID_EXTRA_FLAGS
#define LNSFAID_EXTRA_FLAGS ""
#endif
/* the experiment switches of the build (Makefile EXTRA) are part of the version: "lnsfaid-amd 0.4 (gfx950)" is the default build */
extern "C" const char* lnsfaid_version(void)
{
    return sizeof(LNSFAID_EXTRA_FLAGS) > 1 ? "lnsfaid-amd 0.4 (gfx950) [" LNSFAID_EXTRA_FLAGS "]" : "lnsfaid-amd 0.4 (gfx950)";
}
