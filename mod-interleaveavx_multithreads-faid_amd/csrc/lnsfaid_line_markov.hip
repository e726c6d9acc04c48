/*
 * lnsfaid_line_markov.hip — the line-format error-propagation channel (include/lnsfaid.h "line-format error-propagation channel",
 * DESIGN.md §3.20): a hard channel with memory on LNSFAID_LINE_HARD words.  The host form in lnsfaid_tables.c is the definition; this
 * kernel returns the same bytes.
 *
 * Generator: the link's (lnsfaid_link.h), the BSC's domain d = 2.
 *
 * The chain e[k] = g[k] | (p[k] & e[k - 1]), g[k] = (u[k] < t_idle), p[k] = (u[k] < t_after), g implies p, is the carry chain of the
 * sum A + B with A the p bits and B the g bits: where both are set the adder generates, where only p is set it propagates, where
 * neither is set it kills.  The carry into bit k of A + B + c is bit k of (A + B + c) ^ A ^ B, so
 *   inside a word   e = ((A + B + c) ^ A ^ B) >> 1 on 33 bits, and bit 32 is the word's carry-out: one add and three logic operations,
 *   across words    a word generates when its carry-out with c = 0 is set and propagates when its carry-out with c = 1 is set.  Both
 *                   are balloted over the wave; the two 64-bit ballot masks are uniform, so their sum - the same identity one level
 *                   up - is scalar-unit work, and bit `lane` of (Pm + Gm + c) ^ Pm ^ Gm is the lane's carry-in.  The carry-out of
 *                   that 64-bit sum is the one bit that passes to the next 64 words.
 *
 * Shape: one wavefront per codeword, a lane per word and pass (DESIGN.md §3.20 has the reason: 540 words are 8.4 passes, 94 % of the
 * lanes busy, against 70 % with a 16-byte unit per lane, and the kernel is bound by its draws, not by its 4-byte loads).  No LDS and
 * no barrier.  A wave walks codewords with the grid's stride and keeps the call's two totals in registers: two global atomics per
 * wave.  The carry bit is re-seeded from s = the low half of draw L / 2 at each codeword.
 *
 * Bounds.  cw < n_cw and w < lw where anything is loaded or stored: word cw * lw + w < n_cw * lw of both lines, flips[cw] and
 * runs[cw] with cw <= n_cw - 1.  Lanes past the last word of a codeword hold A = B = 0 (kill) and neither load nor store.
 * line_in == line_out is allowed: a lane reads its word before it writes that word, and no other lane touches it.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "lnsfaid.h"
#include "lnsfaid_launch.h"
#include "lnsfaid_link.h"

#define LM_WAVES 4        /* codewords in flight per workgroup */
#define LM_MAX_WG 2048u   /* 8 192 waves: every SIMD of the device full once, then the waves stride */

struct LmThresholds { uint32_t idle, after, start; };

/* m = 2 m + (u < t): the compare's lane mask is the carry-in of m + m.  Two instructions per bit; written out because the compiler
 * turns the C form, m + m + (u < t), into compare, select, shift and or (three per bit and an s_nop in front of every select).  t is
 * uniform (a scalar register).  VCC written by a VALU compare and read as carry-in by the next VALU instruction needs no wait state:
 * it is the pair every 64-bit add compiles to. */
__device__ __forceinline__ void lm_shift_in(uint32_t& m, uint32_t u, uint32_t t)
{
    asm("v_cmp_gt_u32_e32 vcc, %2, %1\n\tv_addc_co_u32_e32 %0, vcc, %0, %0, vcc" : "+v"(m) : "v"(u), "s"(t) : "vcc");
}

/* the p bits (A) and g bits (B) of line word w: bit 2 j from the low half of draw 16 w + j, bit 2 j + 1 from the high half.  Built
 * from the top bit down, each compare shifted in from below. */
__device__ __forceinline__ void lm_masks(uint64_t cwkey, uint32_t w, uint32_t t_idle, uint32_t t_after, uint32_t& A, uint32_t& B)
{
    uint32_t a = 0u, b = 0u;
    const uint64_t base = cwkey + ((uint64_t)(16u * w) + 1u) * 0x9E3779B97F4A7C15ull;
#pragma unroll
    for (int j = 15; j >= 0; --j) {
        const uint64_t h = lnk_mix64(base + (uint64_t)j * 0x9E3779B97F4A7C15ull);
        const uint32_t hi = (uint32_t)(h >> 32), lo = (uint32_t)h;
        lm_shift_in(a, hi, t_after);
        lm_shift_in(b, hi, t_idle);
        lm_shift_in(a, lo, t_after);
        lm_shift_in(b, lo, t_idle);
    }
    A = a; B = b;
}

__device__ __forceinline__ uint32_t lm_wave_sum(uint32_t v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v; /* lane 0 holds the sum */
}

/* lw: words per codeword.  totals: flips and runs of the call, ADDED to. */
__global__ __launch_bounds__(64 * LM_WAVES) void lnsfaid_line_markov_kernel(const uint32_t* line_in, uint32_t* line_out, uint32_t n_cw, uint32_t lw,
                                                                            unsigned long long key, unsigned long long first, LmThresholds t,
                                                                            uint32_t* __restrict__ flips, uint32_t* __restrict__ runs,
                                                                            unsigned long long* __restrict__ totals)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned long long sum_flips = 0ull, sum_runs = 0ull; /* lane 0's */
    for (uint32_t cw = blockIdx.x * LM_WAVES + wave; cw < n_cw; cw += gridDim.x * LM_WAVES) {
        const uint64_t ck = lnk_cwkey(key, first + (uint64_t)cw, 2u);
        uint32_t carry = (uint32_t)lnk_draw(ck, (uint64_t)lw * 16u) < t.start ? 1u : 0u; /* e of position -1; uniform, as all of its kind below */
        const size_t base = (size_t)cw * lw;
        uint32_t n = 0u, r = 0u;
        for (uint32_t w0 = 0u; w0 < lw; w0 += 64u) {
            const uint32_t w = w0 + lane;
            const bool active = w < lw;
            uint32_t A = 0u, B = 0u, x = 0u;
            if (active) {
                x = line_in[base + w];
                lm_masks(ck, w, t.idle, t.after, A, B);
            }
            const uint64_t s0 = (uint64_t)A + B; /* 33 bits */
            const unsigned long long Gm = __ballot((s0 >> 32) != 0u), Pm = __ballot(((s0 + 1u) >> 32) != 0u);
            const unsigned long long s1 = Pm + Gm, s2 = s1 + carry;
            const uint32_t c_in = (uint32_t)(((s2 ^ Pm ^ Gm) >> lane) & 1ull);
            carry = (s1 < Pm || s2 < s1) ? 1u : 0u; /* the carry-out of the 64 words */
            const uint32_t e = (uint32_t)(((s0 + c_in) ^ (uint64_t)A ^ (uint64_t)B) >> 1);
            const uint32_t before = w == 0u ? 0u : c_in; /* in front of the codeword there is no inverted position */
            n += (uint32_t)__popc(e);
            r += (uint32_t)__popc(e & ~((e << 1) | before));
            if (active) line_out[base + w] = x ^ e;
        }
        n = lm_wave_sum(n);
        r = lm_wave_sum(r);
        if (lane == 0u) {
            if (flips) flips[cw] = n;
            if (runs) runs[cw] = r;
            sum_flips += n;
            sum_runs += r;
        }
    }
    if (lane == 0u) {
        if (sum_flips) atomicAdd(&totals[0], sum_flips);
        if (sum_runs) atomicAdd(&totals[1], sum_runs);
    }
}

/* The caller (lnsfaid_capi.hip) has checked the rules of include/lnsfaid.h: n_cw > 0, the pointers on 4 bytes, t_idle <= t_after.
 * d_totals: two counters, ADDED to. */
extern "C" hipError_t lf_launch_line_markov(const uint32_t* d_in, uint32_t* d_out, size_t n_cw, uint32_t lw, uint64_t key, uint64_t first,
                                            const uint32_t t[3], uint32_t* d_flips, uint32_t* d_runs, unsigned long long* d_totals,
                                            hipStream_t stream)
{
    const size_t wgs = (n_cw + LM_WAVES - 1u) / LM_WAVES;
    const dim3 grid((unsigned)(wgs < LM_MAX_WG ? wgs : LM_MAX_WG)), block(64 * LM_WAVES);
    LmThresholds th;
    th.idle = t[0]; th.after = t[1]; th.start = t[2];
    hipLaunchKernelGGL(lnsfaid_line_markov_kernel, grid, block, 0, stream, d_in, d_out, (uint32_t)n_cw, lw, key, first, th, d_flips, d_runs, d_totals);
    return hipGetLastError();
}
