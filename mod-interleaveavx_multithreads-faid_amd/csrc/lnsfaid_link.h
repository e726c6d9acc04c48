/*
 * lnsfaid_link.h - the device text that the link kernels share, written once (gfx950): lnsfaid_line_link.hip, lnsfaid_line_soft.hip,
 * lnsfaid_line_markov.hip and lnsfaid_burst_link.hip.  Internal: not part of the public boundary.
 * The host forms in lnsfaid_tables.c are the definition of every draw; this is the one device copy that is held to them.
 *
 * Generator (counter-based, stateless):
 *   cwkey(key, C, d) = mix64(mix64(key + d) + (C + 1) * 0xD1B54A32D192ED03),  draw(q) = mix64(cwkey + (q + 1) * 0x9E3779B97F4A7C15)
 * C is the global codeword number and d the domain: d = 1 payload, d = 2 binary symmetric channel and error-propagation channel,
 * d = 3 soft channel.  Line word w of a (mother) codeword uses the draws 16 w .. 16 w + 15, two positions per draw: position 2 j from
 * the low half of draw 16 w + j, position 2 j + 1 from the high half.  A payload word w is half of draw w / 2.
 *
 * The helpers are forced-inline functions where the kernels' instruction text is the same either way (tools/isa_instance_diff.py).
 * The soft channel's unit loop and the counter kernels' tallies are macro text over the kernel's own locals, as the frames of
 * lnsfaid_frame4.h are and for their reason: as functions they compile to other schedules, the tallies to scratch memory.
 */
#ifndef LNSFAID_LINK_H
#define LNSFAID_LINK_H

#include <hip/hip_runtime.h>

#include <stdint.h>

/* ---- the generator ---- */
__device__ __forceinline__ uint64_t lnk_mix64(uint64_t x)
{
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
__device__ __forceinline__ uint64_t lnk_cwkey(uint64_t key, uint64_t C, uint64_t d) { return lnk_mix64(lnk_mix64(key + d) + (C + 1u) * 0xD1B54A32D192ED03ull); }
__device__ __forceinline__ uint64_t lnk_draw(uint64_t cwkey, uint64_t q) { return lnk_mix64(cwkey + (q + 1u) * 0x9E3779B97F4A7C15ull); }

/* ---- binary symmetric channel: the inversion mask of mother word w ---- */
__device__ __forceinline__ uint32_t lnk_flip_mask(uint64_t cwkey, uint32_t w, uint32_t threshold)
{
    uint32_t mask = 0u;
    const uint64_t base = cwkey + ((uint64_t)(16u * w) + 1u) * 0x9E3779B97F4A7C15ull;
#pragma unroll
    for (uint32_t j = 0; j < 16u; ++j) {
        const uint64_t h = lnk_mix64(base + (uint64_t)j * 0x9E3779B97F4A7C15ull);
        mask |= ((uint32_t)h < threshold ? 1u : 0u) << (2u * j);
        mask |= ((uint32_t)(h >> 32) < threshold ? 2u : 0u) << (2u * j);
    }
    return mask;
}

/* ---- soft channel (lnsfaid_line_soft.hip describes the walk) ---- */
struct LnkTable { uint32_t t[14]; }; /* the fourteen thresholds, by value: scalar registers */

/* the threshold at tree node k (1 .. 15): entry (2 p + 1) * 2^(3 - d) - 1 of [0, table[0 .. 13]], d the depth of k and p its place in it */
__device__ __forceinline__ uint32_t lnk_node(const LnkTable& tab, int k)
{
    const int d = k < 2 ? 0 : k < 4 ? 1 : k < 8 ? 2 : 3, p = k - (1 << d);
    const int s = (2 * p + 1) * (8 >> d) - 1;
    return s == 0 ? 0u : tab.t[s - 1];
}

/* one position: u against the LDS threshold tree, the line bit as sb = -b.  Shifts r = m - b into rw and the level b ? m : -m into
 * lv, top nibble first. */
__device__ __forceinline__ void lnk_position(uint32_t u, uint32_t root, const uint32_t* tree, int32_t sb, uint32_t& rw, uint32_t& lv)
{
    uint32_t a = u >= root ? 12u : 8u; /* the node's byte address, 4 * node */
#pragma unroll
    for (int s = 0; s < 2; ++s) a = 2u * a + (u >= *(const uint32_t*)((const char*)tree + a) ? 4u : 0u);
    const uint32_t node = (a >> 1) + (u >= *(const uint32_t*)((const char*)tree + a) ? 1u : 0u);
    const int32_t r = (int32_t)node - 24 + sb;
    rw = __builtin_amdgcn_alignbit((uint32_t)r, rw, 4);
    lv = __builtin_amdgcn_alignbit((uint32_t)-(r ^ sb), lv, 4);
}

/* One unit: line word X, its first draw's counter Q0 = cwkey + (16 w + 1) * 0x9E37.., the root threshold and the LDS tree.  Fills the
 * unit's four output words OUT[4] and adds its flips to N.  Per output word: eight positions, four draws. */
#define LNK_SOFT_UNIT(X, Q0, ROOT, TREE, OUT, N)                                                              \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                           \
        uint32_t rw = 0u, lv = 0u;                                                                            \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                       \
            const uint64_t h = lnk_mix64((Q0) + (uint64_t)(4 * i + j) * 0x9E3779B97F4A7C15ull);               \
            const int b = 8 * i + 2 * j;                                                                      \
            lnk_position((uint32_t)h, ROOT, TREE, (int32_t)((X) << (31 - b)) >> 31, rw, lv);                  \
            lnk_position((uint32_t)(h >> 32), ROOT, TREE, (int32_t)((X) << (30 - b)) >> 31, rw, lv);          \
        }                                                                                                     \
        (OUT)[i] = lv;                                                                                        \
        (N) += (uint32_t)__popc(rw & 0x88888888u);                                                            \
    }                                                                                                         \
    /* end of LNK_SOFT_UNIT */

/* ---- flip sums of the channel kernels: wave 0 writes the codewords' sums (sFlips[t], t < cws, codewords cw0 ..) out and adds
 * their sum to the call's total, one global atomic per workgroup.  After the barrier behind the unit loop. ---- */
__device__ __forceinline__ void lnk_flips_out(const unsigned int* sFlips, uint32_t cw0, uint32_t cws, uint32_t* __restrict__ flips,
                                              unsigned long long* __restrict__ total)
{
    const uint32_t tid = threadIdx.x;
    if (tid < 64u) {
        uint32_t n = tid < cws ? sFlips[tid] : 0u;
        if (flips && tid < cws) flips[cw0 + tid] = n;
        for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o);
        if (tid == 0u && n) atomicAdd(total, (unsigned long long)n);
    }
}

/* ---- the counter kernels: one wavefront per codeword, WAVES codewords per workgroup pass.  Over the kernel's locals tid, lane,
 * stats, n_cw and acc (errors[4], fec[4], vs_sent[4], ADDED to). ---- */
/* lane 0's tallies: error frames, error bits, frames with 1 or 2; failed (uncorrectable), corrected codewords, corrected bits;
 * undetected, false alarms */
#define LNK_COUNT_LOCALS()                                                                                    \
    __shared__ unsigned int sAcc[9];                                                                          \
    if (tid < 9u) sAcc[tid] = 0u;                                                                             \
    __syncthreads();                                                                                          \
    uint32_t n_err = 0, n_bits = 0, n_lt3 = 0, n_unc = 0, n_cor = 0, n_cbits = 0, n_und = 0, n_fa = 0;        \
    /* end of LNK_COUNT_LOCALS */

/* Codeword CW with WRONG payload bits (lane 0 holds the wave's sum).  FAILED and CLEAN: the codeword's failure and "no failure is
 * reported" in terms of unsat, the record's unsatisfied checks; LOCAL: a declaration they use, or nothing.  The line counter passes
 * bare expressions: with a local of the macro's own in between, its three instances compile to another instruction order. */
#define LNK_COUNT_TALLY(CW, WRONG, LOCAL, FAILED, CLEAN)                                                      \
    if (lane == 0u) {                                                                                         \
        if ((WRONG) > 0u) { n_err += 1u; n_bits += (WRONG); n_lt3 += (WRONG) < 3u ? 1u : 0u; }                \
        if (stats) {                                                                                          \
            const int32_t unsat = stats[CW].unsatisfied, corr = stats[CW].corrected;                          \
            LOCAL                                                                                             \
            if (FAILED) n_unc += 1u;                                                                          \
            else if (unsat == 0 && corr > 0) { n_cor += 1u; n_cbits += (uint32_t)corr; }                      \
            if ((WRONG) > 0u) n_und += (CLEAN) ? 1u : 0u;                                                     \
            else n_fa += (FAILED) ? 1u : 0u;                                                                  \
        }                                                                                                     \
    }                                                                                                         \
    /* end of LNK_COUNT_TALLY */

/* behind the codeword loop: the waves' tallies into LDS, the workgroup's sums into the twelve counters */
#define LNK_COUNT_TAIL(WAVES)                                                                                 \
    if (lane == 0u) {                                                                                         \
        if (n_err) { atomicAdd(&sAcc[0], n_err); atomicAdd(&sAcc[1], n_bits); atomicAdd(&sAcc[2], n_lt3); }   \
        if (n_unc) atomicAdd(&sAcc[3], n_unc);                                                                \
        if (n_cor) { atomicAdd(&sAcc[4], n_cor); atomicAdd(&sAcc[5], n_cbits); }                              \
        if (n_und) atomicAdd(&sAcc[6], n_und);                                                                \
        if (n_fa) atomicAdd(&sAcc[7], n_fa);                                                                  \
    }                                                                                                         \
    __syncthreads();                                                                                          \
    if (tid == 0u) {                                                                                          \
        uint32_t walked = 0; /* the codewords this workgroup walked */                                        \
        for (uint32_t cw = blockIdx.x * (WAVES); cw < n_cw; cw += gridDim.x * (WAVES))                        \
            walked += n_cw - cw < (WAVES) ? n_cw - cw : (WAVES);                                              \
        atomicAdd(&acc[0], (unsigned long long)walked);                                                       \
        if (sAcc[0]) atomicAdd(&acc[1], (unsigned long long)sAcc[0]);                                         \
        if (sAcc[1]) atomicAdd(&acc[2], (unsigned long long)sAcc[1]);                                         \
        if (sAcc[2]) atomicAdd(&acc[3], (unsigned long long)sAcc[2]);                                         \
        if (stats) {                                                                                          \
            atomicAdd(&acc[4], (unsigned long long)walked);                                                   \
            if (sAcc[3]) atomicAdd(&acc[5], (unsigned long long)sAcc[3]);                                     \
            if (sAcc[4]) atomicAdd(&acc[6], (unsigned long long)sAcc[4]);                                     \
            if (sAcc[5]) atomicAdd(&acc[7], (unsigned long long)sAcc[5]);                                     \
            atomicAdd(&acc[8], (unsigned long long)walked);                                                   \
            if (sAcc[0]) atomicAdd(&acc[9], (unsigned long long)sAcc[0]);                                     \
            if (sAcc[6]) atomicAdd(&acc[10], (unsigned long long)sAcc[6]);                                    \
            if (sAcc[7]) atomicAdd(&acc[11], (unsigned long long)sAcc[7]);                                    \
        }                                                                                                     \
    }                                                                                                         \
    /* end of LNK_COUNT_TAIL */

#endif /* LNSFAID_LINK_H */
