/*
 * lnsfaid_line.h — launch arguments of the line-format decoders (lnsfaid_kernel4l.hip), shared with the host side of the C ABI
 * (lnsfaid_capi.hip).  Internal: not part of the public boundary.  A header of its own, so that no file the other kernels are
 * compiled from changes.
 */
#ifndef LNSFAID_LINE_H
#define LNSFAID_LINE_H

#include "lnsfaid_device.h"

/* One launch per batch, one workgroup per codeword, nothing kept between launches (as LfCwArgs). */
struct LfLineArgs {
    const LfDevCode* code;
    const LfDevCfg* cfg;
    const void* line;           /* LNSFAID_LINE_HARD: [n_cw][L / 32] words; LNSFAID_LINE_LLR4: [n_cw][L / 2] bytes; 4-byte aligned */
    uint32_t* payload;          /* [n_cw][K / 32] */
    uint32_t* bits;             /* [n_cw][n_var / 32] or null */
    uint4* st_rows;             /* [n_cw][nbr][128] messages between layers (instances without messages in registers) */
    lnsfaid_line_stats* stats;  /* [n_cw] or null */
    int32_t format;             /* LNSFAID_LINE_HARD / LNSFAID_LINE_LLR4: uniform, branched on in staging and in the corrected count */
    int32_t magnitude;          /* HARD: 1 .. 7 */
    int32_t n_cw;
};

#endif
