/*
 * lnsfaid_quantise.h — CLDPC::float2LimitChar_4bit (reference CLDPC.cpp:4553-4573), shared by the device front-end, the
 * demapper kernels and the host demapper: one float multiply, truncation toward zero as cvttps2dq does it (the "integer
 * indefinite" 0x80000000 for NaN and for every |y| >= 2^31, positive ones included), saturating packs to int8, clamp to
 * [-7, 7].  The indefinite therefore ends at -7.
 */
#ifndef LNSFAID_QUANTISE_H
#define LNSFAID_QUANTISE_H

#include <stdint.h>

__host__ __device__ __forceinline__ int8_t quantise_4bit(float x, float scale)
{
    const float y = x * scale;
    int q = (y > -2147483648.0f && y < 2147483648.0f) ? (int)y : (int)0x80000000; /* cvttps2dq */
    q = q > 127 ? 127 : (q < -128 ? -128 : q);                                      /* saturating packs */
    return (int8_t)(q > 7 ? 7 : (q < -7 ? -7 : q));
}

#endif /* LNSFAID_QUANTISE_H */
