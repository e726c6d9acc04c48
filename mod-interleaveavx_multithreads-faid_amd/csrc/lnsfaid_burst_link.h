/*
 * lnsfaid_burst_link.h — what lnsfaid_burst_link.hip exports to the host side of the C ABI (lnsfaid_capi.hip): the launch functions
 * of the burst-format link (include/lnsfaid.h "burst-format link").  Internal: not part of the public boundary.  A
 * header of its own, included by those two files only, so that no file an existing kernel is compiled from changes.
 */
#ifndef LNSFAID_BURST_LINK_H
#define LNSFAID_BURST_LINK_H

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "lnsfaid.h"
#include "lnsfaid_burst.h"

extern "C" {

/* The caller has checked the rules of include/lnsfaid.h and uploaded d_desc[n_cw] on `stream` (burst_descriptors): n_cw > 0, the
 * pointers on 4 bytes, where TAIL or HEAD.  lw = L / 32, kw = K / 32.  d_total: one counter, ADDED to; d_acc: twelve, ADDED to. */
hipError_t lf_launch_burst_payload(uint32_t* d_payload, const LfBurstDesc* d_desc, int where, size_t n_cw, uint32_t kw, uint64_t key,
                                   uint64_t first, hipStream_t stream);
hipError_t lf_launch_burst_bsc(const uint32_t* d_in, uint32_t* d_out, const LfBurstDesc* d_desc, int where, size_t n_cw, uint32_t lw,
                               uint32_t kw, uint64_t key, uint64_t first, uint32_t threshold, uint32_t* d_flips,
                               unsigned long long* d_total, hipStream_t stream);
hipError_t lf_launch_burst_soft(const uint32_t* d_in, uint8_t* d_out, const LfBurstDesc* d_desc, int where, size_t n_cw, uint32_t lw,
                                uint32_t kw, uint64_t key, uint64_t first, const uint32_t table[14], uint32_t* d_flips,
                                unsigned long long* d_total, hipStream_t stream);
hipError_t lf_launch_burst_count(const uint32_t* d_payload, const uint32_t* d_sent, const lnsfaid_line_stats* d_stats,
                                 const uint32_t* d_short_ones, const LfBurstDesc* d_desc, size_t n_cw, uint32_t kw,
                                 unsigned long long* d_acc, hipStream_t stream);

} /* extern "C" */

#endif /* LNSFAID_BURST_LINK_H */
