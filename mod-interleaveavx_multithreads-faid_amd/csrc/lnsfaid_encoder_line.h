/*
 * lnsfaid_encoder_line.h - what the line-format encoders share (gfx950): the sizes of the LDS plan and the helpers of
 * lnsfaid_encode_line_kernel (lnsfaid_encoder_line.hip, which describes the phases and the plan) and of its burst form
 * lnsfaid_encode_burst_kernel (lnsfaid_encoder_burst.hip).  Internal: not part of the public boundary.
 */
#ifndef LNSFAID_ENCODER_LINE_H
#define LNSFAID_ENCODER_LINE_H

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "lnsfaid_device.h"

#define ENL_T 256                     /* threads per workgroup = circulant size */
#define ENL_RAW_STRIDE 33             /* words per codeword of the raw image: column reads hit 32 banks */
#define ENL_RAW_WORDS (32 * ENL_RAW_STRIDE)
#define ENL_U_WORDS 1024              /* one round: 32 words of 32 codewords = four block columns, bit-sliced */
#define ENL_PST_STRIDE 9
#define ENL_PST_WORDS (32 * ENL_PST_STRIDE)
#define ENL_CT_WORDS 68               /* a round's circulants, LF_MAX_COLW slots for each of four block columns, and their weights */
static_assert(LF_MAX_COLW == 16 && ENL_CT_WORDS == 4 * LF_MAX_COLW + 4, "the circulant table is indexed with shifts by 4");

/* the word of lane ^ D within the 32 lanes of a half-wave (ds_swizzle bit mode: and 0x1f, or 0, xor D) */
template <int D>
__device__ __forceinline__ uint32_t enl_xor_lane(uint32_t x)
{
    return (uint32_t)__builtin_amdgcn_ds_swizzle((int)x, 0x1f | (D << 10));
}

/* One step of the 32 x 32 bit transpose over the 32 lanes of a half-wave (lane i holds row i): lanes i and i ^ D exchange the
 * off-diagonal D x D blocks.  keep: the columns c with (c & D) == 0.  Lanes with bit D clear keep those columns and take the
 * others from the partner's kept ones, shifted up; lanes with bit D set the other way round.  Branch-free: selects by mask. */
template <int D>
__device__ __forceinline__ uint32_t enl_exchange(uint32_t x, uint32_t lane, uint32_t keep)
{
    const uint32_t y = enl_xor_lane<D>(x);
    const uint32_t up = 0u - ((lane / D) & 1u); /* all ones in the lanes with bit D set */
    const uint32_t ys = ((y >> D) & up) | ((y << D) & ~up);
    const uint32_t take = ~keep ^ up; /* the columns that come from the partner: keep where bit D is set, ~keep elsewhere */
    return (x & ~take) | (ys & take);
}

/* lane i holds row i (bit c = element (i, c)) -> lane i holds column i (bit r = element (r, i)) */
__device__ __forceinline__ uint32_t enl_transpose32(uint32_t x, uint32_t lane)
{
    x = enl_exchange<16>(x, lane, 0x0000ffffu);
    x = enl_exchange<8>(x, lane, 0x00ff00ffu);
    x = enl_exchange<4>(x, lane, 0x0f0f0f0fu);
    x = enl_exchange<2>(x, lane, 0x33333333u);
    x = enl_exchange<1>(x, lane, 0x55555555u);
    return x;
}

/* four words at a 4-byte aligned address: one 16-byte access (the buffers of the calls are only promised 4-byte alignment; rows
 * that start on 16 bytes get aligned accesses) */
typedef uint32_t enl_u32x4 __attribute__((ext_vector_type(4), aligned(4)));

/* LDS writes of this wave complete, then the workgroup barrier: unlike __syncthreads() it does not wait for global loads and
 * stores in flight, so the payload words of the next round stay in flight across it */
__device__ __forceinline__ void enl_lds_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

/* the word s[b z + (c + t) mod z] from x4 = 4 (b z + c) and t4 = 4 t, z = 256 */
__device__ __forceinline__ uint32_t enl_s_word(const uint32_t* s, uint32_t x4, uint32_t t4)
{
    return *(const uint32_t*)((const char*)s + ((x4 & ~(4u * LF_Z - 1u)) | ((x4 + t4) & (4u * LF_Z - 4u))));
}

#endif /* LNSFAID_ENCODER_LINE_H */
