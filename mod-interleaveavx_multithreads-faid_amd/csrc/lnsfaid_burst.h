/*
 * lnsfaid_burst.h — launch arguments of the burst-format line calls (lnsfaid_kernel4b.hip, lnsfaid_encoder_burst.hip), shared with
 * the host side of the C ABI (lnsfaid_capi.hip).  Internal: not part of the public boundary.  A header of its own, so that no file
 * the other kernels are compiled from changes.
 */
#ifndef LNSFAID_BURST_H
#define LNSFAID_BURST_H

#include "lnsfaid_device.h"

/* Where codeword c of a burst lies: the host's prefix sums over (L - S_c) / 32 and (K - S_c) / 32.  One unit of line_off is 32
 * transmitted positions - one word of a LNSFAID_LINE_HARD line, 16 bytes of a LNSFAID_LINE_LLR4 line - so 65 536 codewords of either
 * format stay below 2^26 units; the kernels widen to size_t before they scale to bytes.  16 bytes: one scalar load. */
struct LfBurstDesc {
    uint32_t line_off; /* first unit of the codeword on the line */
    uint32_t pay_off;  /* first word of the codeword's payload */
    uint32_t s_words;  /* S_c / 32 */
    uint32_t reserved;
};

/* LfLineArgs plus the descriptors: one launch per batch, one workgroup per codeword */
struct LfBurstArgs {
    const LfDevCode* code;
    const LfDevCfg* cfg;
    const void* line;           /* the burst line, 4-byte aligned */
    uint32_t* payload;          /* the burst payload */
    uint32_t* bits;             /* [n_cw][n_var / 32] or null */
    uint4* st_rows;             /* [n_cw][nbr][128] messages between layers (instances without messages in registers) */
    lnsfaid_line_stats* stats;  /* [n_cw] or null */
    uint32_t* short_ones;       /* [n_cw] or null */
    const LfBurstDesc* desc;    /* [n_cw] */
    int32_t format;             /* LNSFAID_LINE_HARD / LNSFAID_LINE_LLR4 */
    int32_t magnitude;          /* HARD: 1 .. 7 */
    int32_t where;              /* LNSFAID_SHORTEN_TAIL / LNSFAID_SHORTEN_HEAD */
    int32_t n_cw;
};

#endif
