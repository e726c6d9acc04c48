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
#include "lnsfaid_frame4.h"
#include "lnsfaid_launch.h"

#define LF4_RULE GROUP

/* ---- the decode kernel: one wave per codeword ---------------------------------------------------------- */
template <int METHOD, bool RM, bool EF2>
__global__ __launch_bounds__(LF_T4, 2) void lnsfaid_decode4_kernel(LfKernelArgs a)
{
    LF4_GROUP_FRAME(LF4_STAGE_INPUT, write_decoded, int8_t, N)
}

extern "C" int lf_decode4_rm_layers(void) { return LF4_RM_LAYERS; }

/* the instance a configuration runs on (LF4_INSTANCE_TABLE, lnsfaid_frame4.h, says which there are) */
extern "C" const void* lf_decode4_func(int method, int ef, int rm)
{
    LF4_INSTANCE_TABLE(lnsfaid_decode4_kernel)
}
extern "C" int lf_decode4_threads(void) { return LF_T4; }
