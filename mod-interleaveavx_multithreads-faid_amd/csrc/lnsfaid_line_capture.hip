/*
 * lnsfaid_line_capture.hip — line-format failure capture (include/lnsfaid.h "line-format failure capture"): the
 * codewords of a line call whose decisions leave checks unsatisfied, or differ from the sent word in the payload, leave the device as
 * ordered, compact records - line image, decisions, error pattern and the set of unsatisfied checks.  A pure read of decisions that
 * may come from anywhere; no decode kernel is involved.
 *
 * Three kernels on one stream, no host decision between them (the structure of lnsfaid_capture.hip, the syndrome method of
 * lnsfaid_fecstatus.hip):
 *   flag    one wavefront per codeword, LC_WAVES codewords per workgroup pass, a workgroup walks the batch with the grid's stride.
 *           Streams the codeword's packed decisions, and the sent word where given, with LC_UNITS loads in flight per stream before
 *           the first use, writes the bit plane into the wave's own LDS (bit b of word w = code bit 32 w + b) and takes XOR and
 *           popcount against the sent word on the way, split at K.  Then the syndrome from the plane: word k (rows 32 k .. 32 k + 31)
 *           of layer br is the XOR over the layer's circulants of the 32 bits that start at bit (32 k + shift) mod 256 of the
 *           circulant's block column - two LDS reads and a funnel shift each.  The layer table (block column * 256 + shift of every
 *           circulant) is staged in LDS once per workgroup.  cnt[codeword] = {flags, unsatisfied, wrong_payload, wrong_parity}.
 *   rank    one workgroup walks cnt in chunks of 1024 codewords with a carry: an exclusive prefix sum over the selected flags.  The
 *           rank of a failure is the number of failures with a smaller index, so slot i of a call always holds the same codeword
 *           whatever the order in which workgroups ran.
 *   gather  one workgroup per slot; a workgroup whose slot is not stored leaves at once.  Copies the line image and the decisions,
 *           forms the error section, recomputes the syndrome as words instead of as a count, counts the channel's own errors and
 *           writes the record.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "lnsfaid_device.h"
#include "lnsfaid_launch.h"

#define LC_WAVES 4      /* codewords in flight per workgroup of the flag kernel */
#define LC_UNITS 4      /* loads a lane has in flight per stream before the first use */
#define LC_MAX_WG 2048u
#define LC_CHUNK 1024u  /* codewords per chunk of the rank kernel = its workgroup size */
#define LC_GATHER 256u  /* threads of a gather workgroup */

/* the plane of a wave is written and read by that wave alone: an LDS fence, no s_barrier */
__device__ __forceinline__ void lc_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ void lc_clear(uint4& v) { v = make_uint4(0u, 0u, 0u, 0u); }
__device__ __forceinline__ void lc_clear(uint2& v) { v = make_uint2(0u, 0u); }
__device__ __forceinline__ void lc_clear(uint32_t& v) { v = 0u; }
__device__ __forceinline__ void lc_split(uint4 v, uint32_t* w) { w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; }
__device__ __forceinline__ void lc_split(uint2 v, uint32_t* w) { w[0] = v.x; w[1] = v.y; }
__device__ __forceinline__ void lc_split(uint32_t v, uint32_t* w) { w[0] = v; }

/* the > 0 of eight two's-complement nibbles as eight bits, nibble i -> bit i */
__device__ __forceinline__ uint32_t lc_positive_nibbles(uint32_t x)
{
    uint32_t t = ((((x & 0x77777777u) + 0x77777777u) | x) & ~x & 0x88888888u) >> 3;
    t = (t | (t >> 3)) & 0x03030303u;
    t = (t | (t >> 6)) & 0x000f000fu;
    return (t | (t >> 12)) & 0xffu;
}

/* the codeword's nw decision words into the plane; .x / .y: this lane's share of the bits that differ from the sent word in words
 * below kw / from kw on (s == nullptr: nothing is counted).  T: the load; nw is a multiple of its words. */
template <typename T>
__device__ __forceinline__ uint2 lc_pass1(const uint32_t* __restrict__ b, const uint32_t* __restrict__ s, uint32_t nw, uint32_t kw,
                                          uint32_t* plane, uint32_t lane)
{
    constexpr uint32_t C = (uint32_t)(sizeof(T) / 4u);
    const T* bv = (const T*)b;
    const T* sv = (const T*)s;
    T* pv = (T*)plane;
    const uint32_t n = nw / C;
    uint2 wrong = make_uint2(0u, 0u);
    for (uint32_t j0 = 0; j0 < n; j0 += 64u * LC_UNITS) {
        T x[LC_UNITS], y[LC_UNITS];
#pragma unroll
        for (uint32_t u = 0; u < LC_UNITS; ++u) {
            const uint32_t j = j0 + u * 64u + lane;
            lc_clear(x[u]);
            lc_clear(y[u]);
            if (j < n) {
                x[u] = bv[j];
                if (s) y[u] = sv[j];
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < LC_UNITS; ++u) {
            const uint32_t j = j0 + u * 64u + lane;
            if (j >= n) continue;
            pv[j] = x[u];
            if (s) {
                uint32_t xw[C], yw[C];
                lc_split(x[u], xw);
                lc_split(y[u], yw);
#pragma unroll
                for (uint32_t c = 0; c < C; ++c) {
                    const uint32_t d = (uint32_t)__popc(xw[c] ^ yw[c]);
                    if (j * C + c < kw) wrong.x += d;
                    else wrong.y += d;
                }
            }
        }
    }
    return wrong;
}

/* syndrome word t = br * 8 + k of the plane: bit b is row 32 t + b of pos_vn */
__device__ __forceinline__ uint32_t lc_syndrome_word(const uint32_t* plane, const uint32_t* sSb, const uint32_t* sDeg, uint32_t t)
{
    const uint32_t br = t >> 3, k = t & 7u, deg = sDeg[br];
    uint32_t acc = 0;
    for (uint32_t j = 0; j < deg; ++j) {
        const uint32_t sb = sSb[br * LF_MAX_DEG + j], o = (32u * k + sb) & 255u, q = o >> 5;
        const uint32_t* col = plane + (sb >> 8) * 8u;
        acc ^= __funnelshift_r(col[q], col[(q + 1u) & 7u], o & 31u);
    }
    return acc;
}

/* the layer table into LDS; the caller synchronises */
__device__ __forceinline__ void lc_stage_table(const LfDevCode* __restrict__ code, uint32_t nbr, uint32_t* sSb, uint32_t* sDeg, uint32_t tid,
                                               uint32_t threads)
{
    for (uint32_t i = tid; i < nbr * LF_MAX_DEG; i += threads) sSb[i] = code->circ[i / LF_MAX_DEG][i % LF_MAX_DEG].sb;
    for (uint32_t i = tid; i < nbr; i += threads) sDeg[i] = (uint32_t)code->deg[i];
}

/* cnt[codeword] = {LNSFAID_LINE_CAPTURE_* flags, unsatisfied, wrong_payload, wrong_parity} */
template <typename T>
__global__ __launch_bounds__(64 * LC_WAVES) void lnsfaid_line_capture_flag_kernel(const LfDevCode* __restrict__ code,
                                                                                  const uint32_t* __restrict__ bits,
                                                                                  const uint32_t* __restrict__ sent, uint32_t n_cw,
                                                                                  uint4* __restrict__ cnt)
{
    extern __shared__ __align__(16) uint32_t sPlanes[]; /* LC_WAVES planes of n_var / 32 words */
    __shared__ uint32_t sSb[LF_MAX_BR * LF_MAX_DEG], sDeg[LF_MAX_BR];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t N = (uint32_t)code->n_var, M = (uint32_t)code->n_check, nw = N / 32u, kw = (N - M) / 32u, nbr = (uint32_t)code->nbr;
    lc_stage_table(code, nbr, sSb, sDeg, tid, 64u * LC_WAVES);
    __syncthreads();
    uint32_t* plane = sPlanes + wave * nw;
    for (uint32_t cw = blockIdx.x * LC_WAVES + wave; cw < n_cw; cw += gridDim.x * LC_WAVES) {
        const size_t at = (size_t)cw * nw;
        const uint2 wrong = lc_pass1<T>(bits + at, sent ? sent + at : nullptr, nw, kw, plane, lane);
        lc_wave_sync();
        uint32_t unsat = 0, wp = wrong.x, wq = wrong.y;
        for (uint32_t t = lane; t < nbr * 8u; t += 64u) unsat += (uint32_t)__popc(lc_syndrome_word(plane, sSb, sDeg, t));
        lc_wave_sync(); /* the next codeword rewrites the plane */
        for (int o = 32; o > 0; o >>= 1) { unsat += __shfl_down(unsat, o); wp += __shfl_down(wp, o); wq += __shfl_down(wq, o); }
        if (lane == 0u) {
            const uint32_t flags = (unsat > 0u ? (uint32_t)LNSFAID_LINE_CAPTURE_UNCORRECTABLE : 0u) |
                                   (wp > 0u ? (uint32_t)LNSFAID_LINE_CAPTURE_WRONG : 0u);
            cnt[cw] = make_uint4(flags, unsat, wp, wq);
        }
    }
}

/* slots[r - skip] = index of failure r for skip <= r < skip + cap; meta = {found, stored}.  One workgroup.  The ordered prefix sum
 * of lnsfaid_capture_rank_kernel over the selected flags. */
__global__ __launch_bounds__(LC_CHUNK) void lnsfaid_line_capture_rank_kernel(const uint4* __restrict__ cnt, uint32_t n_cw, uint32_t select,
                                                                             uint32_t skip, uint32_t cap, uint32_t* __restrict__ slots,
                                                                             unsigned long long* __restrict__ meta)
{
    __shared__ uint32_t sWave[LC_CHUNK / 64u];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t carry = 0; /* failures in front of the chunk: every thread keeps the same value */
    const uint32_t last = n_cw > 0u ? n_cw - 1u : 0u; /* cnt holds at least one group's entries */
    uint32_t cur = cnt[tid < last ? tid : last].x;
    for (uint32_t base = 0; base < n_cw; base += LC_CHUNK) {
        const uint32_t cw = base + tid;
        /* the next chunk's flags are in flight over this chunk's two barriers: without that the walk is one load latency per chunk.
         * The index is clamped, not guarded, so that the load stands outside control flow and the wait can leave it in flight. */
        const uint32_t next = cnt[cw + LC_CHUNK < last ? cw + LC_CHUNK : last].x;
        const bool flag = cw < n_cw && (cur & select) != 0u;
        cur = next;
        const unsigned long long mask = __ballot(flag);
        if (lane == 0u) sWave[wave] = (uint32_t)__popcll(mask);
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < LC_CHUNK / 64u; ++w) {
            const uint32_t v = sWave[w];
            before += w < wave ? v : 0u;
            total += v;
        }
        const uint32_t rank = carry + before + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        if (flag && rank >= skip && rank - skip < cap) slots[rank - skip] = cw;
        carry += total;
        __syncthreads(); /* sWave is rewritten by the next chunk */
    }
    if (tid == 0u) {
        const uint32_t left = carry > skip ? carry - skip : 0u;
        meta[0] = carry;
        meta[1] = left < cap ? left : cap;
    }
}

struct LcGatherArgs {
    const LfDevCode* code;
    const uint32_t* line; /* or null */
    const uint32_t* bits;
    const uint32_t* sent; /* or null */
    const uint4* cnt;
    const uint32_t* slots;
    const unsigned long long* meta;
    lnsfaid_line_failure* records;
    uint32_t* payload;
    unsigned long long first;
    uint32_t lw; /* words of a codeword's line image */
    int llr4;
};

/* slot i: records[i] and payload[i] = line | bits | error | syndrome of codeword slots[i] */
__global__ __launch_bounds__(LC_GATHER) void lnsfaid_line_capture_gather_kernel(LcGatherArgs a)
{
    extern __shared__ __align__(16) uint32_t sPlane[]; /* n_var / 32 words */
    __shared__ uint32_t sSb[LF_MAX_BR * LF_MAX_DEG], sDeg[LF_MAX_BR], sSum[LC_GATHER / 64u];
    const uint32_t slot = blockIdx.x, tid = threadIdx.x;
    if ((unsigned long long)slot >= a.meta[1]) return; /* the grid is sized before `stored` is known */
    const LfDevCode* __restrict__ code = a.code;
    const uint32_t N = (uint32_t)code->n_var, M = (uint32_t)code->n_check, nw = N / 32u, mw = M / 32u, nbr = (uint32_t)code->nbr;
    const uint32_t cw = a.slots[slot], W = a.lw + 2u * nw + mw;
    lc_stage_table(code, nbr, sSb, sDeg, tid, LC_GATHER);
    uint32_t* __restrict__ p = a.payload + (size_t)slot * W;
    const uint32_t* __restrict__ b = a.bits + (size_t)cw * nw;
    const uint32_t* __restrict__ s = a.sent ? a.sent + (size_t)cw * nw : nullptr;
    const uint32_t* __restrict__ l = a.line ? a.line + (size_t)cw * a.lw : nullptr;
    for (uint32_t w = tid; w < nw; w += LC_GATHER) {
        const uint32_t x = b[w];
        sPlane[w] = x;
        p[a.lw + w] = x;
        p[a.lw + nw + w] = s ? x ^ s[w] : 0u;
    }
    uint32_t ch = 0; /* this thread's share of channel_errors */
    for (uint32_t w = tid; w < a.lw; w += LC_GATHER) {
        const uint32_t x = l ? l[w] : 0u;
        p[w] = x;
        if (l && s) {
            if (a.llr4) ch += (uint32_t)__popc(lc_positive_nibbles(x) ^ ((s[w >> 2] >> (8u * (w & 3u))) & 0xffu)); /* positions 8 w .. 8 w + 7 */
            else ch += (uint32_t)__popc(x ^ s[w]);
        }
    }
    for (int o = 32; o > 0; o >>= 1) ch += __shfl_down(ch, o);
    if ((tid & 63u) == 0u) sSum[tid >> 6] = ch;
    __syncthreads();
    for (uint32_t t = tid; t < nbr * 8u && t < mw; t += LC_GATHER) p[a.lw + 2u * nw + t] = lc_syndrome_word(sPlane, sSb, sDeg, t);
    if (tid == 0u) {
        const uint4 c = a.cnt[cw];
        lnsfaid_line_failure r;
        r.codeword = a.first + (unsigned long long)cw;
        r.index = cw; r.flags = c.x; r.unsatisfied = c.y; r.wrong_payload = c.z; r.wrong_parity = c.w;
        r.channel_errors = 0u;
        for (uint32_t w = 0; w < LC_GATHER / 64u; ++w) r.channel_errors += sSum[w];
        a.records[slot] = r;
    }
}

/* The caller (lnsfaid_capi.hip) has checked the rules of include/lnsfaid.h: n_var, K and L multiples of 32, n_check = nbr * 256,
 * n_var <= LF_MAX_BC * 256 (the planes fit the workgroup's LDS), every device pointer 4-byte aligned.  d_cnt: n_cw entries; d_slots,
 * d_records, d_payload: `cap` slots; skip <= n_cw; d_meta: {found, stored}, written. */
extern "C" hipError_t lf_launch_line_capture(const LfDevCode* d_code, int n_var, int puncture_tail, const void* d_line, int format,
                                             const uint32_t* d_bits, const uint32_t* d_sent, size_t n_cw, uint64_t first, int select,
                                             uint32_t skip, uint32_t cap, uint4* d_cnt, uint32_t* d_slots, lnsfaid_line_failure* d_records,
                                             uint32_t* d_payload, unsigned long long* d_meta, hipStream_t stream)
{
    const uint32_t n = (uint32_t)n_cw, nw = (uint32_t)n_var / 32u, wgs = (n + LC_WAVES - 1u) / LC_WAVES;
    const dim3 grid(wgs < LC_MAX_WG ? wgs : LC_MAX_WG), block(64 * LC_WAVES);
    const size_t lds = (size_t)LC_WAVES * nw * sizeof(uint32_t);
    /* every codeword starts a multiple of nw words after its base pointer */
    const uintptr_t a = (uintptr_t)d_bits | (uintptr_t)d_sent | (uintptr_t)(nw * 4u);
    if ((a & 15u) == 0u) hipLaunchKernelGGL(lnsfaid_line_capture_flag_kernel<uint4>, grid, block, lds, stream, d_code, d_bits, d_sent, n, d_cnt);
    else if ((a & 7u) == 0u) hipLaunchKernelGGL(lnsfaid_line_capture_flag_kernel<uint2>, grid, block, lds, stream, d_code, d_bits, d_sent, n, d_cnt);
    else hipLaunchKernelGGL(lnsfaid_line_capture_flag_kernel<uint32_t>, grid, block, lds, stream, d_code, d_bits, d_sent, n, d_cnt);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lnsfaid_line_capture_rank_kernel, dim3(1), dim3(LC_CHUNK), 0, stream, d_cnt, n, (uint32_t)select, skip, cap, d_slots,
                       d_meta);
    e = hipGetLastError();
    if (e != hipSuccess || cap == 0u) return e;
    LcGatherArgs g;
    g.code = d_code; g.line = (const uint32_t*)d_line; g.bits = d_bits; g.sent = d_sent; g.cnt = d_cnt; g.slots = d_slots; g.meta = d_meta;
    g.records = d_records; g.payload = d_payload; g.first = first;
    const uint32_t l_bits = (uint32_t)(n_var - puncture_tail);
    g.llr4 = format == LNSFAID_LINE_LLR4;
    g.lw = g.llr4 ? l_bits / 8u : l_bits / 32u;
    hipLaunchKernelGGL(lnsfaid_line_capture_gather_kernel, dim3(cap), dim3(LC_GATHER), (size_t)nw * sizeof(uint32_t), stream, g);
    return hipGetLastError();
}
