/*
 * lnsfaid_swar.h — one layer of the layered decoder with FOUR check rows per lane, byte-parallel in 32-bit registers.
 *
 * Mapping.  One wavefront owns one codeword; lane i owns check rows i, i+64, i+128, i+192 of every
 * layer (block row) of the quasi-cyclic H.  Byte k of every working register belongs to row i + 64 k.  Inside a block
 * column the a-posteriori LLRs are stored so that the four variable nodes these rows meet on one circulant share ONE
 * LDS dword: variable node v (0..255) of the column lives in dword v mod 64, byte v div 64.  Through a circulant with
 * shift s lane i reads dword (i + s) mod 64 and rotates it right by ((i + s) div 64) mod 4 bytes: one ds_read_b32 and
 * one v_alignbyte_b32 instead of four byte reads and three packs, and all 64 lanes hit 64 consecutive dwords.
 *
 * Arithmetic is carry-free SWAR on biased bytes (every intermediate stays inside its byte, so plain 32-bit adds never
 * carry across rows) built from the instructions gfx950 issues at the full rate (two-source 32-bit ALU operations and
 * v_bitop3_b32) plus v_perm_b32 used three ways: as an 8-entry byte table (FAID look-up table, thermometer code, +-c
 * constants), as a "bit 7 of every byte -> byte mask" expander (its sign-replicating selectors 8..11), and as a packer.
 *   LDS byte        Eb = En + 120                      (En in [-31, 31])
 *   V2C             tb = t + 128,  t = En - Lold       (one add of a per-row, per-sign constant picked by v_perm)
 *   sign            bit 7 of ts = tb - b, b = "old message negative": the reference's back-tracked sign of a zero V2C
 *                   (CDecoder_FAID.cpp:682: t == 0 means En == Lold, so sign(En) is the stored sign bit)
 *   minima          thermometer code U(a), a = min(|t|, 7): bit i set iff a > i, so min = AND and
 *                   second-min' = second-min & (min | U): two boolean operations per edge for four rows; the binary
 *                   index of an edge attaining the minimum comes from five more AND accumulators (index bits 0..2: over
 *                   the edges with the bit clear, bits 3 and 4: over the fewer edges with it set) compared with the minimum
 *                   afterwards — no per-edge compare / select.
 *   update          En' = clamp(z, -31, 31 - c) + (L < 0 ? 0 : c) with z = t - (L < 0 ? c : 0): limits independent of the sign
 *                   of the new message L = +-c (sw_update)
 * Reference statements restated here: CDecoder_FAID.cpp:662-929 (FAID / 2B1C rows), CDecoder_OMS.cpp:363-471 (OMS rows),
 * CLDPC.cpp:296-375 (NMS rows).  As in the 2-rows-per-lane kernel the check-to-variable messages are kept compressed
 * (sign bit per edge, the two magnitudes of the row, the edge that carries the larger one) and only ONE edge per row
 * carries c1: every edge is processed as if it carried c2 and the arg-min edge is patched through LDS before pass 1 and
 * recomputed exactly after pass 2 (DESIGN.md 3.2 explains why this is bit-exact).
 *
 * The file compiles for the device (hipcc) and for the host (g++, -DSW_HOST): tests/ run the very same statements on the
 * CPU against the oracle, lane by lane (lanes of a layer are independent: they touch disjoint variable nodes).
 */
#ifndef LNSFAID_SWAR_H
#define LNSFAID_SWAR_H

#include <stdint.h>

#if defined(__HIPCC__) /* both passes of hipcc see the device flavour; a plain C++ compiler gets the restatements */
#define SW_DEV 1
#define SW_FN __device__ __forceinline__
#define SW_HD __host__ __device__ __forceinline__ /* table builders: also run by the host side of the C ABI */
#else
#define SW_DEV 0
#define SW_FN static inline
#define SW_HD static inline
#endif

#define SW_MAX_DEG 24
#ifndef SW_ILP
#define SW_ILP 4 /* edges whose dependency chains are interleaved in the two passes */
#endif

/* Keeps the compiler's scheduler from moving instructions across this point.  With two waves per SIMD nothing hides an LDS
 * round trip, so the layer step issues all loads of a phase back to back and only then starts consuming them; left alone the
 * scheduler interleaves "load, wait, use" per edge (one read in flight, every LDS latency exposed). */
#if SW_DEV
#define SW_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
#else
#define SW_SCHED_FENCE() ((void)0)
#endif

/* ---- the three non-trivial instructions, with host restatements of their ISA semantics -------------------------- */
/* v_perm_b32: byte i of the result = BYTE_PERMUTE({s0, s1}, sel byte i): 0..3 bytes of s1, 4..7 bytes of s0,
 * 8 / 9 / 10 / 11 bit 7 of byte 1 / 3 / 5 / 7 replicated, 12 -> 0x00, >= 13 -> 0xff */
SW_FN uint32_t sw_perm(uint32_t s0, uint32_t s1, uint32_t sel)
{
#if SW_DEV
    return __builtin_amdgcn_perm(s0, s1, sel);
#else
    const uint64_t in = ((uint64_t)s0 << 32) | s1;
    uint32_t r = 0;
    for (int i = 0; i < 4; ++i) {
        const uint32_t s = (sel >> (8 * i)) & 0xffu;
        uint32_t b;
        if (s >= 13) b = 0xff;
        else if (s == 12) b = 0;
        else if (s >= 8) b = ((in >> (8 * (2 * (s - 8) + 1) + 7)) & 1u) ? 0xffu : 0u;
        else b = (uint32_t)(in >> (8 * s)) & 0xffu;
        r |= b << (8 * i);
    }
    return r;
#endif
}
/* v_alignbyte_b32: ({s0, s1} >> (8 * s2[1:0])) & 0xffffffff (gfx950 reads two bits of s2: checked on the device by
 * tests/test_gpu_swar.py); used with s0 == s1 as a byte rotation, where 4 and 0 both mean "no rotation" */
SW_FN uint32_t sw_alignbyte(uint32_t s0, uint32_t s1, uint32_t s2)
{
#if SW_DEV
    return __builtin_amdgcn_alignbyte(s0, s1, s2);
#else
    const uint64_t in = ((uint64_t)s0 << 32) | s1;
    return (uint32_t)(in >> (8 * (s2 & 3u)));
#endif
}
/* v_bitop3_b32: bit i of the result = bit ((a_i << 2) | (b_i << 1) | c_i) of the truth table */
template <int TT>
SW_FN uint32_t sw_bitop3(uint32_t a, uint32_t b, uint32_t c)
{
#if SW_DEV
    return __builtin_amdgcn_bitop3_b32(a, b, c, TT);
#else
    uint32_t r = 0;
    for (int m = 0; m < 8; ++m)
        if ((TT >> m) & 1) r |= ((m & 4) ? a : ~a) & ((m & 2) ? b : ~b) & ((m & 1) ? c : ~c);
    return r;
#endif
}
#define SW_TT_SEL 0xca   /* a ? b : c            */
#define SW_TT_XOR3 0x96  /* a ^ b ^ c            */
#define SW_TT_AND3 0x80  /* a & b & c            */
#define SW_TT_ANDOR 0xea /* (a & b) | c          */
#define SW_TT_NANDOR 0xae /* (~a & b) | c        */
#define SW_TT_A_AND_BORC 0xe0 /* a & (b | c)     */
#define SW_TT_XORAND 0x28 /* (a ^ b) & c         */
#define SW_TT_BFI_C 0xd8 /* c ? b : a            */
#define SW_TT_ANDNOT_OR 0xf8 /* a | (b & c)      */
#define SW_TT_XNOR_AND 0x82 /* ~(a ^ b) & c        */

/* a constant that must live in a VGPR (VOP3 takes no literal, and an SGPR operand halves the issue rate) */
/* `dep`: any uniform value of the scope the constant belongs to.  The asm is not volatile, so the compiler hoists it out of every
 * loop in which its inputs do not change: out of the layer loop, as wanted - and, without `dep`, out of the iteration loop too,
 * across the syndrome stage, where the seventeen registers are then spilled (an asm result cannot be rematerialised). */
SW_FN uint32_t sw_vconst(uint32_t k, uint32_t dep = 0u)
{
#if SW_DEV
    uint32_t r;
    asm("v_mov_b32 %0, %1 ; %2" : "=v"(r) : "s"(k), "s"(dep));
    return r;
#else
    (void)dep;
    return k;
#endif
}

/* table of sw_therm2num: entries 0 / 1 / 3 / 7 = 0xfb ^ 0 / 1 / 2 / 3 */
#define SW_T2N_LO 0xf900fafbu
#define SW_T2N_HI 0xf8000000u

/* the register constants of the layer step, built ONCE per kernel: inside the layer function they would sit in a conditionally
 * executed block (the per-degree instances), out of which the compiler may not move an asm statement */
struct SwK {
    uint32_t c78, c0642, cfc, sel_sign, tt_lo, tt_hi, oh_lo, oh_hi;
    uint32_t cbit[8]; /* 0x01010101 << e; [0] = 0x01010101, [7] = 0x80808080 */
    uint32_t c7f;
    uint32_t c70;     /* NMS only: its minima keep 16 levels */
    uint32_t n_lo, n_hi; /* thermometer code -> number (sw_therm2num) */
    uint32_t c55, c33, c0f; /* merge masks of pass 2's sign words */
    uint32_t cm27;    /* -0x27272727: the last constant of sw_update2, as an addend of v_add3_u32 */
    uint32_t tm[4];   /* SW_FORM_NOWIN only, set by its caller once per iteration: thermometer code -> magnitude (sw_therm2msg_tables of
                       * the row's one table: lut_* for the FAID decoders, oms_*[0] for the min-sum ones) */
    uint32_t c100;    /* SW_FORM_MUL only: the factor of the left shifts by 8 (sw_shl8_mul) */
};
SW_FN SwK sw_consts(uint32_t dep = 0u)
{
    SwK k;
    k.c78 = sw_vconst(0x78787878u, dep); k.c0642 = sw_vconst(0x06040200u, dep); k.cfc = sw_vconst(0xfcu, dep);
    k.sel_sign = sw_vconst(0x0b090a08u, dep);
    /* thermometer code of min(|t|, 7); entry 7 equals what v_perm returns for a saturated selector */
    k.tt_lo = sw_vconst(0x07030100u, dep); k.tt_hi = sw_vconst(0xff3f1f0fu, dep);
    k.oh_lo = sw_vconst(0x08040201u, dep); k.oh_hi = sw_vconst(0x80402010u, dep);
    for (int e = 0; e < 8; ++e) k.cbit[e] = sw_vconst(0x01010101u << e, dep);
    k.c7f = sw_vconst(0x7f7f7f7fu, dep);
    k.c70 = sw_vconst(0x70707070u, dep);
    k.n_lo = sw_vconst(SW_T2N_LO, dep); k.n_hi = sw_vconst(SW_T2N_HI, dep);
    k.c55 = sw_vconst(0x55555555u, dep); k.c33 = sw_vconst(0x33333333u, dep); k.c0f = sw_vconst(0x0f0f0f0fu, dep);
    k.cm27 = sw_vconst(0u - 0x27272727u, dep);
    for (int w = 0; w < 4; ++w) k.tm[w] = 0u;
    k.c100 = 0x100u; /* (a plain value: the one caller that reads it on the device moves it to a register itself, like tm[]) */
    return k;
}

/* 0xff in every byte whose bit 7 is set, else 0x00 (two instructions: shift + v_perm with selectors 8..11) */
SW_FN uint32_t sw_mask7(uint32_t x, uint32_t sel_sign) { return sw_perm(x, x << 8, sel_sign); }
#define SW_SEL_SIGN 0x0b090a08u
/* v_lshlrev_b64 by 8 on the register pair {a (low), b (high)}: the low word is a << 8, the high word (b << 8) | (a >> 24).  Bytes 1 and
 * 3 of the high word are bytes 0 and 2 of b and only its byte 0 is foreign (a's top byte) - the byte the sign selectors 8 and 9 of
 * v_perm_b32 never read.  One shift therefore feeds the mask expansion of TWO words.
 * Device: left to itself the compiler takes a 64-bit shift of two 32-bit halves apart again (v_lshlrev_b64 of {a, 0}, v_lshlrev_b32 of b
 * and an OR; or, where only the halves of the result are read, v_lshlrev_b32 and v_alignbit_b32), so the pair and the result each pass
 * through an empty asm statement it cannot look through.  a and b come back as the halves of the pair: a caller that reads them
 * afterwards must read THESE, or the allocator keeps the old registers alive and copies them into the pair. */
SW_FN uint64_t sw_shl8x2(uint32_t& a, uint32_t& b)
{
    uint64_t p = ((uint64_t)b << 32) | a;
#if SW_DEV
    asm("" : "+v"(p));
    a = (uint32_t)p; b = (uint32_t)(p >> 32);
    uint64_t r = p << 8;
    asm("" : "+v"(r));
    return r;
#else
    return p << 8;
#endif
}
/* sw_mask7 of a and of b in three instructions instead of four: the two halves of one sw_shl8x2 under the same selector */
SW_FN uint32_t sw_mask7_lo(uint32_t a, uint64_t sh, uint32_t sel_sign) { return sw_perm(a, (uint32_t)sh, sel_sign); }
SW_FN uint32_t sw_mask7_hi(uint32_t b, uint64_t sh, uint32_t sel_sign) { return sw_perm(b, (uint32_t)(sh >> 32), sel_sign); }
SW_FN void sw_mask7x2(uint32_t a, uint32_t b, uint32_t sel_sign, uint32_t* ma, uint32_t* mb)
{
    const uint64_t sh = sw_shl8x2(a, b);
    *ma = sw_mask7_lo(a, sh, sel_sign);
    *mb = sw_mask7_hi(b, sh, sel_sign);
}

/* ---- left shifts by a constant outside the slow issue class (SW_FORM_MUL) ----
 * v_mul_u32_u24: the low 32 bits of s0[23:0] * s1[23:0].  With the factor 1 << n (n <= 23) in a register that is (x & 0xffffff) << n:
 * x << n wherever bits 24 .. 31 of x are dead - always for n >= 8, where the shift drops them anyway, and only such shifts are
 * written this way.  The factor must sit in a VGPR the compiler cannot look into (sw_vconst), or it makes the shift of it
 * again; inside the layer step's instruction mix the multiply by a register issues like a full-rate instruction, which neither
 * v_lshlrev_b32 nor the multiply by a literal does (profiles/r23_class_moves/ubench_issue_classes.txt). */
SW_FN uint32_t sw_mul_u24(uint32_t x, uint32_t k) { return (x & 0xffffffu) * (k & 0xffffffu); } /* the compiler's own v_mul_u32_u24 */
/* x << 8, every x; c100: 0x100 in a register */
SW_FN uint32_t sw_shl8_mul(uint32_t x, uint32_t c100) { return sw_mul_u24(x, c100); }
/* sw_mask7 on that shift */
SW_FN uint32_t sw_mask7_mul(uint32_t x, uint32_t sel_sign, uint32_t c100) { return sw_perm(x, sw_shl8_mul(x, c100), sel_sign); }
/* sw_mask7(x << 1) for bytes x <= 0x7f - bit 6 of every byte as a byte mask - without the shift by one: adding 0x40 carries bit 6
 * into bit 7 and nothing out of the byte (0x7f + 0x40 = 0xbf), and the expander looks at bit 7 only */
SW_FN uint32_t sw_mask6_mul(uint32_t x, uint32_t sel_sign, uint32_t c100) { return sw_mask7_mul(x + 0x40404040u, sel_sign, c100); }

/* per-byte population count of the low seven bits (thermometer code -> number) */
SW_FN uint32_t sw_popcount7(uint32_t x)
{
    x &= 0x7f7f7f7fu;
    x = x - ((x >> 1) & 0x55555555u);
    x = (x & 0x33333333u) + ((x >> 2) & 0x33333333u);
    return (x + (x >> 4)) & 0x0f0f0f0fu;
}
/* The same number for the eight codes the minimum search can hold (0x00, 0x01, 0x03, 0x07, 0x0f, 0x1f, 0x3f, 0xff) from two v_perm_b32
 * look-ups in ONE table: six instructions instead of eleven (sw_popcount7 stays as the definition the tests compare with).  The
 * table maps the nibble patterns 0 / 1 / 3 / 7 (k = 0 .. 3 bits set) to 0xfb ^ k; a full low nibble is selector 15, which saturates
 * to 0xff.  A = table[low nibble], B = table[bits 4..6]:
 *   n <= 3: A = 0xfb ^ n, B = table[0] = 0xfb          -> A ^ B = n
 *   n >= 4: A = 0xff,     B = 0xfb ^ (n - 4) = ~n      -> A ^ B = n   (0xfb = ~4, and n - 4 <= 3 only touches the low two bits) */
SW_FN uint32_t sw_therm2num(uint32_t x, uint32_t n_lo, uint32_t n_hi)
{
    const uint32_t a = sw_perm(n_hi, n_lo, x & 0x0f0f0f0fu);
    const uint32_t b = sw_perm(n_hi, n_lo, (x >> 4) & 0x07070707u);
    return a ^ b;
}
/* sw_therm2num composed with an 8-entry byte table LUT (entries 0..3 in lut_lo, 4..7 in lut_hi): the row's magnitude LUT[min] straight
 * from the thermometer code, in the six instructions of sw_therm2num - for a layer step that reads ONE table (SW_FORM_NOWIN).  The low
 * nibble's look-up A and the look-up B of bits 4..6 each get a table of their own, over the selectors 0 / 1 / 3 / 7 of sw_therm2num
 * (a full low nibble is selector 15 and still saturates to 0xff).  With C = ~LUT[4]:
 *   A[code of n] = LUT[n] ^ C (n = 0..3),   B[0] = C,   B[code of n - 4] = ~LUT[n] (n = 5..7)
 *   n <= 3: A ^ B = LUT[n] ^ C ^ C          n == 4: 0xff ^ C = LUT[4]          n >= 5: 0xff ^ ~LUT[n] = LUT[n]
 * tm[0], tm[1]: A's entries 0..3 / 4..7; tm[2], tm[3]: B's. */
SW_HD void sw_therm2msg_tables(uint32_t lut_lo, uint32_t lut_hi, uint32_t tm[4])
{
    const uint32_t c = ~lut_hi & 0xffu;                   /* C                                   */
    const uint32_t a = lut_lo ^ (c * 0x01010101u);        /* LUT[0..3] ^ C, byte n               */
    const uint32_t nb = ~lut_hi;                          /* ~LUT[4..7], byte n - 4              */
    tm[0] = (a & 0x0000ffffu) | ((a & 0x00ff0000u) << 8); /* codes 0, 1 -> n = 0, 1; code 3 -> n = 2 */
    tm[1] = a & 0xff000000u;                              /* code 7 -> n = 3                     */
    tm[2] = c | (nb & 0x0000ff00u) | ((nb & 0x00ff0000u) << 8); /* codes 0, 1 -> n = 4, 5; code 3 -> n = 6 */
    tm[3] = nb & 0xff000000u;                             /* code 7 -> n = 7                     */
}
SW_FN uint32_t sw_therm2msg(uint32_t x, const uint32_t tm[4])
{
    const uint32_t a = sw_perm(tm[1], tm[0], x & 0x0f0f0f0fu);
    const uint32_t b = sw_perm(tm[3], tm[2], (x >> 4) & 0x07070707u);
    return a ^ b;
}
/* the same with the low-nibble mask from a register (SW_FORM_VK): the compiler merges that AND into the last AND of the minimum search,
 * a v_bitop3_b32, which takes no literal - the mask would become an SGPR operand */
SW_FN uint32_t sw_therm2msg_vk(uint32_t x, const uint32_t tm[4], uint32_t c0f)
{
    const uint32_t a = sw_perm(tm[1], tm[0], x & c0f);
    const uint32_t b = sw_perm(tm[3], tm[2], (x >> 4) & 0x07070707u);
    return a ^ b;
}
/* 0xff in every byte that is zero; bytes must be <= 0x7f */
SW_FN uint32_t sw_zero_mask(uint32_t x, uint32_t sel_sign) { return ~sw_mask7(x + 0x7f7f7f7fu, sel_sign); }
/* sw_zero_mask of x and of y on one shift (sw_mask7x2) */
SW_FN void sw_zero_mask2(uint32_t x, uint32_t y, uint32_t sel_sign, uint32_t* zx, uint32_t* zy)
{
    uint32_t mx, my;
    sw_mask7x2(x + 0x7f7f7f7fu, y + 0x7f7f7f7fu, sel_sign, &mx, &my);
    *zx = ~mx;
    *zy = ~my;
}

/* four bytes read one by one (each value < 256) into one word, byte k = g_k, as two pairs and their merge: three v_lshl_or_b32 where
 * the compiler finds them (written through an asm statement they were forced - and one of the packed kernels then reserved a stack
 * slot it never touches) */
SW_FN uint32_t sw_gather4(uint32_t g0, uint32_t g1, uint32_t g2, uint32_t g3)
{
    const uint32_t lo = (g1 << 8) | g0, hi = (g3 << 8) | g2;
    return (hi << 16) | lo;
}
/* a value the compiler may not look through: keeps `x >> 16` of it a read of bits 23:16 (ds_write_b8_d16_hi) */
SW_FN uint32_t sw_opaque(uint32_t x)
{
#if SW_DEV
    asm("" : "+v"(x));
#endif
    return x;
}
/* sw_gather4 as three v_perm_b32 (SW_FORM_MUL): knowing every byte's range the compiler takes the three v_lshl_or_b32 apart, shifts g2
 * and g3 into place one by one and merges with a v_or3_b32 - four instructions of the slow class; the packer is three, with no shift */
SW_FN uint32_t sw_gather4_perm(uint32_t g0, uint32_t g1, uint32_t g2, uint32_t g3)
{
    const uint32_t lo = sw_perm(g1, g0, 0x0c0c0400u), hi = sw_perm(g3, g2, 0x0c0c0400u); /* byte 0 of either source, zeros above */
    return sw_perm(hi, lo, 0x05040100u);
}
/* LDS byte address of the variable node that row k of a lane meets through a circulant, from
 * x = 4 (lane + shift) + (k << 8) in the low half (below 0x10000, a multiple of 4) and the block column << 24:
 * byte 0 of x is the dword of the node, byte 3 its block column, bits 9:8 the byte inside the dword ((lane + shift) div 64 + k) mod 4.
 * One v_perm_b32 places the two bytes (tests/layer_trip_helpers_exhaustive.cpp holds the mask / shift / merge form it replaced). */
SW_FN uint32_t sw_node_addr(uint32_t x) { return sw_perm(x, x, 0x0c0c0300u) | ((x >> 8) & 3u); }

/* ---- small per-row statements of the layer step, as functions so that the tests run the very statements the kernel runs ---- */
/* A row's magnitude from one of two 8-entry tables, per byte: table W where the row's mask is set, table T elsewhere */
SW_FN uint32_t sw_table_pick(uint32_t rowmask, uint32_t w_hi, uint32_t w_lo, uint32_t t_hi, uint32_t t_lo, uint32_t m)
{
    return sw_bitop3<SW_TT_SEL>(rowmask, sw_perm(w_hi, w_lo, m), sw_perm(t_hi, t_lo, m));
}
/* One of the three sign words per byte by the arg-min index's bits 4 and 3, given as byte masks that are set where the bit is CLEAR
 * (nm4, nm3; bit 4 is looked at first, so nm3 need not know that bit 3 gives way to it) */
SW_FN uint32_t sw_word_pick(uint32_t nm3, uint32_t nm4, uint32_t x0, uint32_t x1, uint32_t x2)
{
    return sw_bitop3<SW_TT_SEL>(nm4, sw_bitop3<SW_TT_SEL>(nm3, x0, x1), x2);
}
/* `keep` dealt to the three words the same way: oh[g] = keep where the index is in word g */
SW_FN void sw_word_deal(uint32_t keep, uint32_t nm3, uint32_t nm4, uint32_t oh[3])
{
    oh[0] = sw_bitop3<SW_TT_AND3>(keep, nm3, nm4);
    oh[1] = sw_bitop3<0x20>(keep, nm3, nm4); /* a & ~b & c */
    oh[2] = keep & ~nm4;
}
/* v_perm selector 2 k + b of the arg-min edge: b = 1 in byte k where the picked sign word has the edge's one-hot bit set */
SW_FN uint32_t sw_argmin_selector(uint32_t w, uint32_t oh8, uint32_t c7f, uint32_t c01, uint32_t c0642)
{
    return sw_bitop3<SW_TT_ANDOR>(((w & oh8) + c7f) >> 7, c01, c0642);
}

/* ---- compressed messages of the four rows of one lane in one layer (24 bytes, streamed through HBM) ---------------
 * x[g] bit 8 k + e : the message on edge 8 g + e of row k is negative (0 for a zero message, FAID / 2B1C)
 * cw byte k        : c2 | c1 << 3 | (message on the arg-min edge negative) << 6
 * pa[h]            : LDS byte addresses of the arg-min variable nodes of rows 2 h (low half) and 2 h + 1 (high half) */
struct SwRow {
    uint32_t x[3];
    uint32_t cw;
    uint32_t pa[2];
};

/* decoder constants a layer needs (uniform over the wave) */
struct SwParams {
    uint32_t lut_lo, lut_hi;       /* V2C_map_it* as 8 bytes (entries 0..3 / 4..7) for this iteration           */
    uint32_t ef_lo, ef_hi;         /* error-floor table (DecodeMethod 5)                                        */
    int32_t f1, f2;                /* Factor_1 / Factor_2 (OMS offsets, NMS numerators)                          */
    int32_t window;                /* nombre_iterations <= floor_iter_thresh                                     */
    int32_t ef_tables;             /* EF_ELIMINATION >= 1 (always so for DecodeMethod 5; 0, 1 or 2 for DecodeMethod 2)  */
    uint32_t nms_t[4];             /* NMS with one factor: thermometer code of cste(m) = min((m * Factor) >> 5, 7) for m = 0..15 as 16
                                    * bytes (sw_nms_tables); m >= 16 saturates to 0xff, the code of 7                     */
    uint32_t oms_lo[2], oms_hi[2]; /* min-sum decoders: the selective offset + clamp as 8-entry byte tables over the minimum
                                    * (0..7), [0] the ordinary rule, [1] the rule of an unsatisfied row inside the window
                                    * (sw_oms_tables fills them from f1 / f2)                                         */
};

/* LDS seen by the layer step: byte offsets inside the codeword's En image (block column cb at cb * 256). */
#if SW_DEV
struct SwLds {
    typedef __attribute__((address_space(3))) uint32_t lds_u32;
    typedef __attribute__((address_space(3))) uint8_t lds_u8;
    /* off: a compile-time constant below 65 536, which goes into the DS instruction's offset field (0: the plain access) */
    SW_FN uint32_t rd32(uint32_t a, uint32_t off = 0u) const { return *(const lds_u32*)(size_t)(a + off); }
    SW_FN void wr32(uint32_t a, uint32_t v, uint32_t off = 0u) const { *(lds_u32*)(size_t)(a + off) = v; }
    SW_FN uint32_t rd8(uint32_t a) const { return *(const lds_u8*)(size_t)a; }
    SW_FN void wr8(uint32_t a, uint32_t v) const { *(lds_u8*)(size_t)a = (uint8_t)v; }
};
#else
struct SwLds {
    uint8_t* base;
    uint32_t rd32(uint32_t a, uint32_t off = 0u) const { a += off; return (uint32_t)base[a] | ((uint32_t)base[a + 1] << 8) | ((uint32_t)base[a + 2] << 16) | ((uint32_t)base[a + 3] << 24); }
    void wr32(uint32_t a, uint32_t v, uint32_t off = 0u) const { a += off; base[a] = (uint8_t)v; base[a + 1] = (uint8_t)(v >> 8); base[a + 2] = (uint8_t)(v >> 16); base[a + 3] = (uint8_t)(v >> 24); }
    uint32_t rd8(uint32_t a) const { return base[a]; }
    void wr8(uint32_t a, uint32_t v) const { base[a] = (uint8_t)v; }
};
#endif

#define SW_BIAS_EN 120 /* LDS byte = En + 120 */

/* LDS byte position of variable node v (index inside the code word) in the interleaved image */
SW_FN uint32_t sw_en_pos(uint32_t v) { return (v & ~255u) | ((v & 63u) << 2) | ((v >> 6) & 3u); }

/* hard decision En > 0 on the biased bytes (En + 120 >= 121): bit 7 of every byte of x + 7 */
SW_FN uint32_t sw_hard_flags(uint32_t x) { return x + 0x07070707u; }

/* ---- the decision points' cheap "certainly dirty" test on run-time tables: parity of the lane's four rows
 * (lane + 64 k in byte k) of a layer straight from En; the XOR of the hard-decision flags is bit 7 of the XOR of the flag words,
 * the other bits of the result mean nothing.  s4row / cbrow: the layer's rows of LfDevCode's s4tab / cbtab, SW_MAX_DEG entries
 * each, the ones beyond the degree 0.  ALL entries are loaded and all reads made, whatever the degree: the tables then arrive in
 * a few wide scalar loads behind one wait, and the code is straight-line (an unused entry reads the lane's own dword of block
 * column 0: a valid address); only the XOR looks at the degree.  With `j < deg` around the table accesses the compiler, which does
 * not speculate a load, gave every edge a basic block, a scalar load and a wait of its own. */
template <class Row> /* pointer to uint32_t: the device's tables sit in the constant address space */
SW_FN uint32_t sw_row_parity(const SwLds& lds, Row s4row, Row cbrow, int deg, uint32_t lane)
{
    const uint32_t tid4 = lane << 2;
    uint32_t x4[SW_MAX_DEG], ad[SW_MAX_DEG], d[SW_MAX_DEG];
    /* all addresses, then all reads, then the arithmetic: one LDS round trip instead of one per circulant */
#pragma unroll
    for (int j = 0; j < SW_MAX_DEG; ++j) { x4[j] = tid4 + s4row[j]; ad[j] = (x4[j] & 0xfcu) | cbrow[j]; }
    SW_SCHED_FENCE();
#pragma unroll
    for (int j = 0; j < SW_MAX_DEG; ++j) d[j] = lds.rd32(ad[j]);
    SW_SCHED_FENCE();
    uint32_t acc = 0;
#pragma unroll
    for (int j = SW_MAX_DEG - 1; j >= 0; --j) /* the last read first: LDS returns in order, one wait covers all */
        acc ^= j < deg ? sw_hard_flags(sw_alignbyte(d[j], d[j], x4[j] >> 8)) : 0u;
    return acc;
}

/* DecodeMethods whose rows follow Decode_OMS (1, 3, 4) / use the plain sign and no upper clamp on t (those and NMS, 0) */
#define SW_OMS(M) ((M) == 1 || (M) == 3 || (M) == 4)
#define SW_MINSUM(M) ((M) == 0 || SW_OMS(M))

/* selective offset of OMS_MODE 1 on one minimum (CDecoder_OMS.cpp:388-425) */
SW_FN int sw_oms_offset(int x, bool window, bool F, int f1, int f2)
{
    if (window && F) {
        if (x < f2) x += 1;
        if (x <= f1) x += 1;
    } else {
        if (x > f1) x -= 1;
        if (x >= f2) x -= 1;
    }
    return x;
}

/* CDecoder_OMS.cpp:388-432 as two tables: entry x = min(offset(x), SAT_POS_MSG) for both branches of the rule */
SW_FN void sw_oms_tables(SwParams& p)
{
    for (int r = 0; r < 2; ++r) {
        uint32_t lo = 0, hi = 0;
        for (int x = 0; x < 8; ++x) {
            const int a = sw_oms_offset(x, r != 0, r != 0, p.f1, p.f2);
            const uint32_t v = (uint32_t)((a > 7 ? 7 : a) & 0xff);
            if (x < 4) lo |= v << (8 * x); else hi |= v << (8 * (x - 4));
        }
        p.oms_lo[r] = lo; p.oms_hi[r] = hi;
    }
}

/* Normalised min-sum (CLDPC::Decode, CLDPC.cpp:337-352): cste(m) = min(pack_s8((uint16)(m * Factor) >> 5), 7) in 16-bit lanes
 * (VECTOR_MUL = _mm256_mullo_epi16, VECTOR_DIV32 = _mm256_srli_epi16(.., 5), VECTOR_PACK = _mm256_packs_epi16), m = 0..31. */
SW_HD int sw_nms_cste(int m, int factor)
{
    const uint16_t p = (uint16_t)((uint16_t)m * (uint16_t)(int16_t)factor);
    const int16_t q = (int16_t)(p >> 5);
    const int r = q > 127 ? 127 : q;
    return r > 7 ? 7 : r;
}
/* The byte-parallel layer step applies a row's magnitude function to the LEVELS of the minimum search: with one factor for both
 * minima cste() plays the part of the FAID table (a non-decreasing map commutes with the minimum, and edges that tie after the
 * map get the same message whichever of them is called the arg-min - DESIGN.md 3.2).  The search keeps 16 levels of |t| (two
 * v_perm_b32 tables), so cste() must be non-decreasing and have reached its end value 7 at m = 15: true for Factor >= 15 up to
 * the 16-bit wrap (Factor <= 2114), i.e. for every normalisation factor in use (24 / 32 = 0.75 ...); other factors, and two
 * different factors (a tie then gives the two minima different messages), stay on the two-rows-per-lane kernel. */
SW_HD bool sw_nms_fits(int f1, int f2)
{
    if (f1 != f2) return false;
    for (int m = 1; m < 32; ++m)
        if (sw_nms_cste(m, f1) < sw_nms_cste(m - 1, f1)) return false;
    return sw_nms_cste(15, f1) == 7;
}
SW_HD void sw_nms_tables(int factor, uint32_t nms_t[4])
{
    for (int w = 0; w < 4; ++w) nms_t[w] = 0;
    for (int m = 0; m < 16; ++m) {
        const int c = sw_nms_cste(m, factor);
        const uint32_t code = c >= 7 ? 0xffu : ((1u << c) - 1u); /* bit i set iff c > i */
        nms_t[m >> 2] |= code << (8 * (m & 3));
    }
}

/* the two-stage saturating update En' = sat31(tc + L), tc = sat31(t) (FAID, CDecoder_FAID.cpp:672, :919-920) or
 * max(t, -31) (min-sum decoders, CDecoder_OMS.cpp:371, :466), written as ONE clamp whose limits do not depend on the sign of
 * the new message L = +-c:
 *   L = +c : En' = c + clamp(t, -31, 31 - c)        L = -c : En' = clamp(t - c, -31, 31 - c)      (min-sum, L = -c: ..., 31)
 * i.e. z = t - (L < 0 ? c : 0), En' = clamp(z, -31, hi) + (L < 0 ? 0 : c): two sign-selected byte constants per edge (za, sb),
 * the rest is per row.  Working byte zb = z + 159, so that "not under" is bit 7 of zb and "over" is bit 7 of zb - oc. */
struct SwUpd {
    uint32_t za[2], sb[2]; /* [1]: chosen where the mask is 0xff, [0]: where it is 0x00 */
    uint32_t oc[2], hi[2]; /* the two entries differ for the min-sum decoders only */
};
/* c: magnitude bytes (0..7); flip: byte mask, 0xff where mask polarity is inverted (row parity F) */
/* `bias`: what the caller's tb carries on top of t + 128 per byte (FAID keeps the v_perm selector's 0 / 2 / 4 / 6 in it, see
 * pass 1): folded into the constant that meets tb */
template <bool MINSUM, bool FLIP = true>
SW_FN SwUpd sw_update_consts(uint32_t c, uint32_t flip, uint32_t bias)
{
    const uint32_t za_p = 0x1f1f1f1fu - bias, za_n = za_p - c;                  /* zb = tb + za = t + 159 - (L < 0 ? c : 0)   */
    const uint32_t sb_p = 0x27272727u - c, sb_n = 0x27272727u;                  /* En' + 120 = clamped zb - sb                */
    const uint32_t oc_p = 0x3f3f3f3fu - c, oc_n = MINSUM ? 0x3f3f3f3fu : oc_p;  /* over <=> z > hi <=> zb - oc >= 128         */
    const uint32_t hi_p = 0xbebebebeu - c, hi_n = MINSUM ? 0xbebebebeu : hi_p;  /* hi + 159                                   */
    SwUpd u;
    if (!FLIP) { /* the caller's mask already is "new message not negative" */
        u.za[1] = za_p; u.za[0] = za_n; u.sb[1] = sb_p; u.sb[0] = sb_n; u.oc[1] = oc_p; u.oc[0] = oc_n; u.hi[1] = hi_p; u.hi[0] = hi_n;
        return u;
    }
    u.za[1] = sw_bitop3<SW_TT_SEL>(flip, za_n, za_p); u.za[0] = sw_bitop3<SW_TT_SEL>(flip, za_p, za_n);
    u.sb[1] = sw_bitop3<SW_TT_SEL>(flip, sb_n, sb_p); u.sb[0] = sw_bitop3<SW_TT_SEL>(flip, sb_p, sb_n);
    if (MINSUM) {
        u.oc[1] = sw_bitop3<SW_TT_SEL>(flip, oc_n, oc_p); u.oc[0] = sw_bitop3<SW_TT_SEL>(flip, oc_p, oc_n);
        u.hi[1] = sw_bitop3<SW_TT_SEL>(flip, hi_n, hi_p); u.hi[0] = sw_bitop3<SW_TT_SEL>(flip, hi_p, hi_n);
    } else {
        u.oc[1] = u.oc[0] = oc_p; u.hi[1] = u.hi[0] = hi_p;
    }
    return u;
}
/* tb: t + 128 (+ bias) per byte; ms: byte mask picking entry [1] of the constants; c80: 0x80808080 in a register */
template <bool MINSUM>
SW_FN uint32_t sw_update(uint32_t tb, uint32_t ms, const SwUpd& u, uint32_t sel_sign, uint32_t c80)
{
    const uint32_t za = sw_bitop3<SW_TT_SEL>(ms, u.za[1], u.za[0]);
    const uint32_t sb = sw_bitop3<SW_TT_SEL>(ms, u.sb[1], u.sb[0]);
    const uint32_t oc = MINSUM ? sw_bitop3<SW_TT_SEL>(ms, u.oc[1], u.oc[0]) : u.oc[1];
    const uint32_t hi = MINSUM ? sw_bitop3<SW_TT_SEL>(ms, u.hi[1], u.hi[0]) : u.hi[1];
    const uint32_t zb = tb + za;
    const uint32_t mo = sw_mask7(zb - oc, sel_sign); /* over      */
    const uint32_t mq = sw_mask7(zb, sel_sign);      /* not under */
    return sw_bitop3<SW_TT_SEL>(mo, hi, sw_bitop3<SW_TT_SEL>(mq, zb, c80)) - sb;
}

/* The same update in fewer instructions (sw_update / sw_update_consts stay as the definition the tests compare with):
 *  - the constants that depend on the sign of the new message differ by c only: with d = (L < 0 ? 0 : c) they are za = zc + d
 *    (zc = za_p - c), sb = 0x27 - d and, for the min-sum decoders, oc = 0x3f - d, hi = 0xbe - d: ONE masked c per edge and two
 *    three-operand additions instead of a select per constant;
 *  - z can only exceed the upper limit where t > 0 and only fall below the lower one where t < 0 (the limits are at least 24
 *    away from 0 and |z - t| <= 7), so ONE "out of range" test - bit 7 of ~zb | (zb - oc) - and the limit picked by the sign of t
 *    replace the two tests with their two mask expansions and two selects.
 * ms: byte mask, 0xff where t is not negative (plain or back-tracked sign: they differ at t == 0 only); fm: the row's mask F, the
 * new message is not negative where ms ^ fm is set. */
struct SwUpd2 {
    uint32_t c, fm, zc, oc, hi;
};
template <bool MINSUM>
SW_FN SwUpd2 sw_update2_consts(uint32_t c, uint32_t fm, uint32_t bias)
{
    SwUpd2 u;
    u.c = c; u.fm = fm;
    u.zc = 0x1f1f1f1fu - bias - c;
    u.oc = MINSUM ? 0u - 0x3f3f3f3fu : 0x3f3f3f3fu - c; /* min-sum: added together with d */
    u.hi = MINSUM ? 0xbebebebeu : 0xbebebebeu - c;
    return u;
}
/* the stages of sw_update2, separately: pass 2 of the layer step runs them stage by stage over a group of edges */
SW_FN uint32_t sw_upd2_d(uint32_t ms, const SwUpd2& u) { return sw_bitop3<SW_TT_XORAND>(ms, u.fm, u.c); }
SW_FN uint32_t sw_upd2_zb(uint32_t tb, uint32_t d, const SwUpd2& u) { return tb + d + u.zc; }
template <bool MINSUM>
SW_FN uint32_t sw_upd2_out(uint32_t zb, uint32_t d, const SwUpd2& u)
{
    const uint32_t ov = MINSUM ? zb + d + u.oc : zb - u.oc;
    return sw_bitop3<0xcf>(zb, ov, ov); /* ~a | b: bit 7 set = under or over */
}
template <bool MINSUM>
SW_FN uint32_t sw_upd2_limit(uint32_t ms, uint32_t d, const SwUpd2& u, uint32_t c80)
{
    return sw_bitop3<SW_TT_ANDOR>(ms, MINSUM ? u.hi - d : u.hi, c80); /* hi where t >= 0, 0x80 (z = -31) where t < 0 */
}
SW_FN uint32_t sw_upd2_en(uint32_t mout, uint32_t lim, uint32_t zb, uint32_t d, uint32_t cm27) { return sw_bitop3<SW_TT_SEL>(mout, lim, zb) + d + cm27; }
/* tb: t + 128 (+ bias) per byte; cm27: -0x27272727 in a register */
template <bool MINSUM>
SW_FN uint32_t sw_update2(uint32_t tb, uint32_t ms, const SwUpd2& u, uint32_t sel_sign, uint32_t c80, uint32_t cm27)
{
    const uint32_t d = sw_upd2_d(ms, u);
    const uint32_t zb = sw_upd2_zb(tb, d, u);
    const uint32_t mout = sw_mask7(sw_upd2_out<MINSUM>(zb, d, u), sel_sign);
    return sw_upd2_en(mout, sw_upd2_limit<MINSUM>(ms, d, u, c80), zb, d, cm27);
}

/* sw_update2 with its mask on sw_mask7_mul (SW_FORM_MUL) */
template <bool MINSUM>
SW_FN uint32_t sw_update2_mul(uint32_t tb, uint32_t ms, const SwUpd2& u, uint32_t sel_sign, uint32_t c80, uint32_t cm27, uint32_t c100)
{
    const uint32_t d = sw_upd2_d(ms, u);
    const uint32_t zb = sw_upd2_zb(tb, d, u);
    const uint32_t mout = sw_mask7_mul(sw_upd2_out<MINSUM>(zb, d, u), sel_sign, c100);
    return sw_upd2_en(mout, sw_upd2_limit<MINSUM>(ms, d, u, c80), zb, d, cm27);
}

/* ---- minimum search over thermometer codes: running minimum t1, second minimum t2 (with multiplicity) and the five index
 * accumulators ta[] (see "binary index" in sw_layer_step) ---- */
/* one edge (index j) at a time */
SW_FN void sw_min_edge(uint32_t& t1, uint32_t& t2, uint32_t ta[5], uint32_t u, int j)
{
    t2 = sw_bitop3<SW_TT_A_AND_BORC>(t2, t1, u); /* VECTOR_MIN_2 with the old min1 */
    t1 &= u;
#pragma unroll
    for (int b = 0; b < 5; ++b)
        if (((j >> b) & 1) == (b >= 3 ? 1 : 0)) ta[b] &= u;
}
/* The four edges j0 .. j0 + 3 (j0 a multiple of 4) as one set: their minimum q, their second minimum and the partial minima the
 * index accumulators need, then ONE merge into the running pair.  Index bits 2..4 are constant over an aligned group of four, so
 * ta[2..4] take q whole; ta[1] takes the first pair, ta[0] edges 0 and 2.  Minimum and second minimum of a multiset do not depend
 * on the order in which it is merged, so every bit equals what four calls of sw_min_edge give - in fewer operations, because the
 * pairs and the quad are shared by t1 and the accumulators. */
SW_FN void sw_min_quad(uint32_t& t1, uint32_t& t2, uint32_t ta[5], uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3, int j0)
{
    const uint32_t p0 = v0 & v1, p1 = v2 & v3, q = p0 & p1;
    const uint32_t o0 = v0 | v1, o1 = v2 | v3;
    const uint32_t m2 = sw_bitop3<SW_TT_A_AND_BORC>(o0, p0, p1); /* second minimum of the four = m2 & o1: folded into the merge */
    const uint32_t y = sw_bitop3<SW_TT_A_AND_BORC>(t2, t1, q);
    t2 = sw_bitop3<SW_TT_AND3>(y, m2, o1);
    t1 &= q;
    ta[0] = sw_bitop3<SW_TT_AND3>(ta[0], v0, v2);
    ta[1] &= p0;
    if (((j0 >> 2) & 1) == 0) ta[2] &= q;
    if (((j0 >> 3) & 1) == 1) ta[3] &= q;
    if (((j0 >> 4) & 1) == 1) ta[4] &= q;
}

/* Sign words of pass 2 (bit e of byte k of ns[g]: the V2C on edge 8 g + e of row k is not negative), four edges j0 .. j0 + 3
 * (j0 a multiple of 4) at a time from their byte masks ms[]: two masks interleaved bit by bit, two pairs by bit pairs, two groups by
 * nibbles - 7 selects per 8 edges and three constants instead of 8 and eight.  Bits of edges the row does not have are copies of
 * other edges' bits: the caller masks them (`valid`). */
/* one edge at a time; cbit = 0x01010101 << (j mod 8) */
SW_FN void sw_sign_edge(uint32_t ns[3], uint32_t ms, int j, uint32_t cbit) { ns[j >> 3] = sw_bitop3<SW_TT_ANDNOT_OR>(ns[j >> 3], ms, cbit); }
template <int NJ>
SW_FN void sw_sign_quad(uint32_t ns[3], const uint32_t* ms, int j0, int deg, bool fixed, uint32_t c55, uint32_t c33, uint32_t c0f)
{
    uint32_t m[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) m[g] = (j0 + g < NJ && (fixed || j0 + g < deg)) ? ms[j0 + g < NJ ? j0 + g : 0] : 0u;
    const bool has1 = j0 + 1 < NJ, has2 = j0 + 2 < NJ, has3 = j0 + 3 < NJ;
    const uint32_t a = has1 ? sw_bitop3<SW_TT_SEL>(c55, m[0], m[1]) : m[0];
    const uint32_t b = has3 ? sw_bitop3<SW_TT_SEL>(c55, m[2], m[3]) : m[2];
    const uint32_t q = has2 ? sw_bitop3<SW_TT_SEL>(c33, a, b) : a;
    ns[j0 >> 3] = (j0 & 4) ? sw_bitop3<SW_TT_SEL>(c0f, ns[j0 >> 3], q) : q;
}

/* ERA helpers.  Plane bit of the variable node at LDS byte address a (interleaved image: block column in the high bits,
 * dword = node mod 64, byte = node div 64); returns 0 / 1. */
SW_FN uint32_t sw_plane_bit(const SwLds& lds, uint32_t era_plane, uint32_t a)
{
    const uint32_t v = (a & ~255u) | ((a >> 2) & 63u) | ((a & 3u) << 6); /* node index */
    return (lds.rd32(era_plane + ((v >> 5) << 2)) >> (v & 31u)) & 1u;
}

/* ---- one layer -----------------------------------------------------------------------------------------------------
 * Tab: tab.s4(j) = 4 * shift and tab.cb256(j) = block column * 256 of edge j (uniform), tab.sb_dyn4(4 * idx) =
 * (block column * 256) << 16 | 4 * shift for a per-lane edge index.
 * rowpar: byte mask, 0xff in byte k if the syndrome bit of row i + 64 k is set (only read by the OMS selective offset
 * and the 2B1C error-floor tables); lme: unsat < floor_err_count for this codeword.
 * DecodeMethod 0 (NMS, one factor): the minimum search keeps 16 levels of |t| and maps them through cste() (sw_nms_tables). */
/* Two waves per codeword (WAVES == 2, lnsfaid_kernel5.hip): the layer's edges are dealt to the two waves by the parity of their index,
 * every lane of either wave still works on its four rows.  Wave 0 does everything that is per row (old arg-min patch, the merge of
 * the two partial minimum searches, the new magnitudes, the arg-min edge, the row's record); wave 1 only passes 1 and 2 over its
 * edges.  They meet four times per layer (xch.barrier()) and exchange through LDS (xch.put / xch.get, one dword per lane and slot):
 *   A  wave 0 has patched the old arg-min nodes                                  -> both start pass 1
 *   B  wave 1 has published its partial minima / index accumulators / sign XOR   -> wave 0 merges, finishes the row
 *   C  wave 0 has READ the new arg-min nodes and published c2, F                  -> both start pass 2 (which overwrites the nodes)
 *   D  wave 1 has written its En and published its sign bits                     -> wave 0 writes the exact arg-min En, the record
 * SwNoXch: the single-wave build (every call compiles away). */
#if SW_DEV
#define SW_MFN __device__ __forceinline__
#else
#define SW_MFN inline
#endif
struct SwNoXch {
    SW_MFN void put(int, uint32_t) const {}
    SW_MFN uint32_t get(int) const { return 0u; }
    SW_MFN void barrier() const {}
};
/* SW_FORM_EDGEW: where the step takes its edge words from.  w(j): the packed word of rotating edge j (j >= NZ) for this lane,
 * 4 * dword | rotate amount | negated rotate amount << 8 (sw50_edge_word, lnsfaid_static50.h); the step takes the read rotate from it.
 * wa(j): a word of the same value, from which the step makes the address and the write-back rotate: a caller may hand in ONE
 * register for all edges of equal shift, whose address and shifted word are then made once.  at(point): called at fixed points of
 * the step, so that a caller can issue the NEXT layer's loads where registers come free (between scheduling fences of its own, where
 * it does): j0 behind the write-back of pass 2's group of edges j0 .. j0 + SW_ILP - 1, where that group's registers have come free.
 * SwNoEw: every other form (both calls compile away). */
struct SwNoEw {
    SW_MFN uint32_t w(int) const { return 0u; }
    SW_MFN uint32_t wa(int) const { return 0u; }
    SW_MFN void at(int) const {}
};
#define SW_OWN(j) (WAVES == 1 || (((j) & 1) == WAVE))

/* A table view whose s4(j) / cb256(j) are compile-time constants of (layer, j) specialises this (lnsfaid_static50.h): `value` and the
 * layer's exact number `nz` of leading zero-shift edges.  The layer step then takes shifts and block columns as literals, puts the
 * block column into the LDS instructions' offset fields and drops the rotation work of exactly nz edges. */
template <class Tab>
struct SwTabStatic {
    static constexpr bool value = false;
    static constexpr int nz = 0;
};

/* ZG: the layer's first SW_ILP * ZG edges are known to have shift 0 (identity circulants; the caller ordered the edge table so, and
 * the order of a row's edges is free: it only decides which of several tied edges is called the arg-min).  Lane i
 * then reads dword i of the block column and nothing is rotated: per such edge the lane-plus-shift addition, the shift for the
 * rotate amount, the rotate after the read, and the subtraction and the rotate in front of the write-back are not issued.  The
 * rotating code is correct for shift 0, so a smaller ZG than the layer has is always exact.  Per-degree instances of one wave per
 * codeword only.
 * A static table view (SwTabStatic) names the exact count instead: NZ need not be a multiple of SW_ILP then. */
/* PAIRS: byte masks that are expanded side by side share one 64-bit shift (sw_mask7x2), a bit per place: SW_PAIRS_PASS1 / _PASS2 the
 * edges' masks of a pass two by two inside a group of SW_ILP (per-degree instances of one wave per codeword: there both edges of a
 * pair exist and belong to the wave), SW_PAIRS_ROW the per-row ones, (nm3, nm4) and the two zero masks of the new magnitudes.  A
 * clear bit: every mask of that place on a shift of its own (sw_mask7).  The layer-static kernel (lnsfaid_kernel4s.hip) sets them all;
 * the other instances stay on the single form, 0: with the pairs each of them went over one of its own ceilings in tests/ (a 17th
 * s_waitcnt in the layer loop's degree-23 block, one more instruction around the rotation-free loop's blocks, 36 bytes of scratch in
 * the packed per-codeword NMS kernel - DESIGN.md 3.1h). */
#define SW_PAIRS_PASS1 1
#define SW_PAIRS_PASS2 2
#define SW_PAIRS_ROW 4
#define SW_PAIRS_ALL (SW_PAIRS_PASS1 | SW_PAIRS_PASS2 | SW_PAIRS_ROW)
/* FORM: what the caller knows about the iteration the step runs in, a bit each (0: nothing - the step as every kernel but the window-free
 * one, lnsfaid_kernel4w.hip, instantiates it).  One wave per codeword, non-erasing instances only.
 *   SW_FORM_NOWIN  the error-floor window cannot open (floor_iter_thresh < 0): rowpar, lme, p.window and the window's tables are not
 *                  looked at, and the row's magnitudes come straight from the thermometer codes through K.tm (sw_therm2msg) instead of
 *                  sw_therm2num and a look-up in one of two tables.  Not for DecodeMethod 0, whose levels are the magnitudes.
 *   SW_FORM_FRESH  the first iteration: `cur` is all zero (not looked at) and `fresh` is true, so there is no old patch, the old message
 *                  on every edge is +0 (the edges' sign bit, selector and table look-up are constants) and so is the arg-min edge's.
 * Two more bits say how the step is WRITTEN, not what it knows: its results are those of the form without them.  They move
 * instructions from the slow issue class to the full rate:
 *   SW_FORM_VK     constants that the compiler would put into SGPRs as operands of full-rate instructions (an SGPR source makes such an
 *                  instruction a slow one) come from SwK's registers: the low-nibble mask of sw_therm2msg, the record's valid mask, and the
 *                  index decode in a form that reads 0x80 alone; the addends 0x78 and -0x27 of v_add3_u32, slow wherever they sit, give
 *                  their registers up.  Per-degree FAID / min-sum instances of degree > 16.
 *   SW_FORM_MUL    the single left shifts by 8 of the mask expander go through sw_shl8_mul (K.c100 must be a register), the shift by one
 *                  in front of the old patch's mask becomes an addition (sw_mask6_mul), the byte gathers pack with v_perm_b32
 *                  (sw_gather4_perm), and `lane` is passed as 4 * lane: the caller shifts once per iteration, not the step per layer.
 * And one says where values come from that depend on the lane and the code alone:
 *   SW_FORM_EDGEW  a rotating edge's dword address and its two rotate amounts are fields of ONE word per edge and lane that the caller
 *                  hands in (`ew`: a table it loads, the same for every codeword and iteration) instead of four instructions on
 *                  lane + shift: the address is the word under 0xfc, the read rotate takes the word itself and the write-back rotate
 *                  the word >> 8 (v_alignbyte_b32 reads two bits of its amount).  Static table views only. */
#define SW_FORM_NOWIN 1
#define SW_FORM_FRESH 2
#define SW_FORM_VK 4
#define SW_FORM_MUL 8
#define SW_FORM_EDGEW 16
template <int METHOD, int DEG, bool ERA = false, int WAVES = 1, int WAVE = 0, int ZG = 0, int PAIRS = 0, int FORM = 0, class Tab, class Xch = SwNoXch, class Ew = SwNoEw>
SW_FN SwRow sw_layer_step(const SwLds& lds, const Tab& tab, const SwParams& p, const SwK& K, uint32_t lane, int deg, SwRow cur, bool fresh,
                          uint32_t rowpar, bool lme, uint32_t era_edges = 0u, uint32_t era_plane = 0u, const Xch& xch = Xch(), const Ew& ew = Ew())
{
    constexpr bool NOWIN = (FORM & SW_FORM_NOWIN) != 0, FRESH = (FORM & SW_FORM_FRESH) != 0;
    constexpr bool VK = (FORM & SW_FORM_VK) != 0, MULF = (FORM & SW_FORM_MUL) != 0;
    static_assert(FORM == 0 || (WAVES == 1 && !ERA), "iteration forms: one-wave, non-erasing instances");
    static_assert(!NOWIN || METHOD != 0, "the normalised min-sum rows read no table after the search");
    static_assert(WAVES == 1 || !ERA, "the erasing variant is built for one wave per codeword only");
    /* ERA (EF_ELIMINATION 2, CDecoder_FAID.cpp:673-680; the caller instantiates it only inside the error-floor window of a
     * codeword with few unsatisfied checks): era_edges bit j = edge j is the first edge, in row order, of a block column of
     * weight REGULAR_COL_WEIGHT; era_plane = LDS byte offset of a bit plane over the variable nodes, bit set = every check of
     * the node was unsatisfied at this iteration's syndrome stage.  On those edges the V2C becomes 0 for such nodes and its
     * sign is the sign of En itself (the back-track of :682 with vContr == 0). */
    static_assert(!ERA || METHOD == 2, "the erasure exists in Decode_FAID only");
    static_assert(ZG == 0 || (DEG > 0 && WAVES == 1 && !ERA && SW_ILP * ZG <= DEG), "rotation-free groups: per-degree, one-wave, non-erasing instances");
    constexpr bool STATIC = SwTabStatic<Tab>::value;
    static_assert(!STATIC || (ZG == 0 && DEG > 0 && WAVES == 1 && !ERA && SwTabStatic<Tab>::nz <= DEG), "static table view: per-degree, one-wave, non-erasing instances");
    constexpr int NZ = STATIC ? SwTabStatic<Tab>::nz : SW_ILP * ZG; /* edges 0 .. NZ - 1 need no rotation */
    constexpr bool EDGEW = (FORM & SW_FORM_EDGEW) != 0;
    static_assert(!EDGEW || (STATIC && WAVES == 1 && !ERA), "edge words: static table views, one-wave, non-erasing instances");
    constexpr int NJ = DEG > 0 ? DEG : SW_MAX_DEG;
    constexpr bool MINSUM = SW_MINSUM(METHOD);
    /* the minimum search merges aligned groups of four edges (pass 1); the per-degree instances only: in the generic one every
     * edge is conditional and the group's values would have to be kept under a select each */
    constexpr bool QUADS = WAVES == 1 && SW_ILP == 4 && DEG > 0;
    constexpr bool NSTREE = WAVES == 1 && SW_ILP == 4; /* pass 2 packs its sign words four edges at a time (sw_sign_quad) */
    constexpr bool EPAIRS = WAVES == 1 && DEG > 0 && SW_ILP % 2 == 0; /* edges j0 + 2 i, j0 + 2 i + 1 of a group may share a shift */
    constexpr bool EPAIRS1 = EPAIRS && (PAIRS & SW_PAIRS_PASS1), EPAIRS2 = EPAIRS && (PAIRS & SW_PAIRS_PASS2), RPAIRS = (PAIRS & SW_PAIRS_ROW) != 0;
    static_assert(!VK || DEG > 16, "the index decode of SW_FORM_VK: per-degree instances with edges in 16 .. 23");
    /* SW_FORM_VK: 0x78 and -0x27 are addends of v_add3_u32 only (FAID rows), which is of the slow class wherever its operands sit:
     * literals, i.e. SGPRs, and their two registers go to the constants that full-rate instructions read */
    const uint32_t c78 = (VK && !MINSUM) ? 0x78787878u : K.c78;
    const uint32_t c01 = K.cbit[0], c80 = K.cbit[7], c7f = K.c7f, c0642 = K.c0642, cfc = K.cfc, sel_sign = K.sel_sign;
    const uint32_t tid4 = MULF ? lane : lane << 2; /* (SW_FORM_MUL: the caller's 4 * lane) */
    /* a single mask, and a single left shift by 8, in the form of the step */
#define SW_MASK7(x) (MULF ? sw_mask7_mul((x), sel_sign, K.c100) : sw_mask7((x), sel_sign))
#define SW_SHL8(x) (MULF ? sw_shl8_mul((x), K.c100) : (x) << 8)
    /* the layer's circulants first (scalar loads share the LDS counter: in flight together with LDS reads they force full drains) */
    uint32_t s4j[NJ], cbj[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) { s4j[j] = (DEG > 0 || j < deg) ? tab.s4(j) : 0u; cbj[j] = (DEG > 0 || j < deg) ? tab.cb256(j) : 0u; }

    /* ---- the row's old messages: +-c2 on every edge (8 +- c2 as a v_perm table indexed 2 k + negative) ---- */
    const uint32_t c2o = cur.cw & 0x07070707u, c1o = (cur.cw >> 3) & 0x07070707u;
    const uint32_t kp = 0x08080808u - c2o, kn = 0x08080808u + c2o;
    /* FAID: tb = En + 120 + K + selector, with the selector's row part (0 / 2 / 4 / 6 per byte) folded into the table, so that
     * tb - selector = t + 128 - b is the back-tracked sign word in ONE subtraction; pass 2 compensates in its constants */
    const uint32_t bias = MINSUM ? 0u : 0x06040200u;
    const uint32_t kt_lo = sw_perm(kn, kp, 0x05010400u) + (MINSUM ? 0u : 0x02020000u), kt_hi = sw_perm(kn, kp, 0x07030602u) + (MINSUM ? 0u : 0x06060404u);
    const uint32_t tt_lo = K.tt_lo, tt_hi = K.tt_hi; /* thermometer code of min(|t|, 7) */
    /* FRESH: c2o == 0 and no edge's old message is negative, so every edge's selector is its row part and the look-up returns 8 + it */
    const uint32_t k_fresh = 0x08080808u + bias;

    /* ---- the old arg-min edge carries c1, not c2: move its En by the difference so that "every edge carries c2" holds ---- */
    uint32_t padd = 0, psub = 0; /* what the patch below adds to / takes from the old arg-min nodes' LDS bytes */
#ifndef SW_EXP_NO_OLDPATCH
    if (!FRESH && !fresh && WAVE == 0) {
        const uint32_t a0 = cur.pa[0] & 0xffffu, a1 = cur.pa[0] >> 16, a2 = cur.pa[1] & 0xffffu, a3 = cur.pa[1] >> 16;
        SW_SCHED_FENCE(); /* the four reads back to back: one LDS round trip, not one per read */
        const uint32_t g0 = lds.rd8(a0), g1 = lds.rd8(a1), g2 = lds.rd8(a2), g3 = lds.rd8(a3);
        const uint32_t mneg = MULF ? sw_mask6_mul(cur.cw, sel_sign, K.c100) : sw_mask7(cur.cw << 1, sel_sign); /* bit 6: the arg-min message is negative */
        /* En - L(c1) = (En - sigma (c1 - c2)) - sigma c2 */
        padd = sw_bitop3<SW_TT_SEL>(mneg, c1o, c2o); psub = sw_bitop3<SW_TT_SEL>(mneg, c2o, c1o);
        SW_SCHED_FENCE();
        const uint32_t r = (MULF ? sw_gather4_perm(g0, g1, g2, g3) : sw_gather4(g0, g1, g2, g3)) + padd - psub;
        const uint32_t rh = sw_opaque(r >> 8); /* one shift serves both odd bytes */
        lds.wr8(a0, r); lds.wr8(a1, rh); lds.wr8(a2, r >> 16); lds.wr8(a3, rh >> 16);
    }
#endif
    if (WAVES == 2) xch.barrier(); /* A */

    SW_SCHED_FENCE();
    uint32_t tb[NJ], ts[NJ], ms[NJ], ad[NJ], rq[NJ], ld[NJ];
    uint32_t t1 = 0xffffffffu, t2 = 0xffffffffu, ta[5] = { 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu };
    uint32_t sx = 0;

    /* ---- pass 1 (CDecoder_FAID.cpp:662-861, CDecoder_OMS.cpp:363-380): all addresses, then all reads, then the arithmetic ---- */
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        if (j < NZ) {
            ad[j] = STATIC ? tid4 : tid4 | cbj[j]; /* shift 0: dword `lane` of the column, rows in byte order */
        } else if (EDGEW) {
            rq[j] = ew.wa(j); /* (bits 1:0: the read rotate; bits 9:8: the write-back rotate) */
            ad[j] = rq[j] & cfc;
        } else if ((DEG > 0 || j < deg) && SW_OWN(j)) {
            const uint32_t x4 = tid4 + s4j[j];
#if SW_DEV
            uint32_t a;
            if (STATIC) a = x4 & cfc; /* (the block column is the access's offset) */
            else asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(a) : "v"(x4), "v"(cfc), "s"(cbj[j]));
#else
            const uint32_t a = STATIC ? x4 & cfc : (x4 & cfc) | cbj[j];
#endif
            ad[j] = a; rq[j] = x4 >> 8;
        }
    }
    /* static table view: ad[] is the dword inside the column, the column's base the immediate offset of every access of the edge */
#define SW_COL(j) (STATIC ? cbj[j] : 0u)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
        if ((DEG > 0 || j < deg) && SW_OWN(j)) ld[j] = lds.rd32(ad[j], SW_COL(j));
    SW_SCHED_FENCE();
    /* The arithmetic of an edge is one long dependency chain and the hardware issues a wave's instructions in order, so the
     * statements below are written stage by stage over groups of SW_ILP edges: consecutive instructions then belong to
     * different edges and do not wait for each other (two waves per SIMD cannot hide that latency). */
#pragma unroll
    for (int j0 = 0; j0 < NJ; j0 += SW_ILP) {
        uint32_t r_[SW_ILP], x_[SW_ILP], s_[SW_ILP], k_[SW_ILP], a_[SW_ILP], i_[SW_ILP], u_[SW_ILP];
#define SW_EDGES(...) _Pragma("unroll") for (int g = 0; g < SW_ILP; ++g) { const int j = j0 + g; if (j < NJ && (DEG > 0 || j < deg) && SW_OWN(j)) { __VA_ARGS__ } }
        /* A mask stage of a group, DST(g, j) = sw_mask7(SRC(g, j)) on every edge of the group, in two halves: the shifts - with EPAIRS
         * one per pair of edges, the group's odd last edge keeps a 32-bit one - and the expansions.  A reader of a 64-bit shift's
         * result within the next two instructions costs a wait state (the compiler fills it with s_nop).  So the shifts take the
         * stage in front of them along, as PRE: the statement that makes SRC(g, j), run on the two edges of a pair right in front
         * of the pair's shift.  The first pair's expansions then follow the second pair's statements, and the second pair's the
         * first pair's expansions; nothing lives longer than on the single form. */
#define SW_MASK_SHIFTS(EPAIRS, SRC, PRE)                                                                                                 \
        uint64_t sh_[SW_ILP / 2 + 1];                                                                                                    \
        if (EPAIRS) {                                                                                                                    \
            _Pragma("unroll") for (int g0 = 0; g0 < SW_ILP; g0 += 2) {                                                                   \
                _Pragma("unroll") for (int g = g0; g < g0 + 2; ++g) { const int j = j0 + g; if (j < NJ) { PRE } }                       \
                if (j0 + g0 + 1 < NJ) sh_[g0 >> 1] = sw_shl8x2(SRC(g0, j0 + g0), SRC(g0 + 1, j0 + g0 + 1));                              \
                else if (j0 + g0 < NJ) sh_[g0 >> 1] = SW_SHL8(SRC(g0, j0 + g0));                                                           \
            }                                                                                                                            \
        } else {                                                                                                                         \
            SW_EDGES(PRE)                                                                                                                \
        }
#define SW_MASK_EXPAND(EPAIRS, DST, SRC)                                                                                                 \
        if (EPAIRS) {                                                                                                                    \
            _Pragma("unroll") for (int g = 0; g < SW_ILP; ++g) {                                                                         \
                const int j = j0 + g;                                                                                                    \
                if (j < NJ) DST(g, j) = (g & 1) ? sw_mask7_hi(SRC(g, j), sh_[g >> 1], sel_sign) : sw_mask7_lo(SRC(g, j), sh_[g >> 1], sel_sign); \
            }                                                                                                                            \
        } else {                                                                                                                         \
            SW_EDGES(DST(g, j) = sw_mask7(SRC(g, j), sel_sign);)                                                                         \
        }
#define SW_P1_TS(g, j) ts[j]
#define SW_P1_MS(g, j) ms[j]
#define SW_P2_MO(g, j) mo[g]
        /* byte k = En + 120 of row k.  The group's LAST read is consumed first: LDS reads return in order, so the one s_waitcnt in
         * front of it covers the group (in ascending order every edge gets a wait of its own) */
        _Pragma("unroll") for (int g = SW_ILP - 1; g >= 0; --g) { const int j = j0 + g; if (j < NJ && (DEG > 0 || j < deg) && SW_OWN(j)) r_[g] = j < NZ ? ld[j] : sw_alignbyte(ld[j], ld[j], EDGEW ? ew.w(j) : rq[j]); }
        if (FRESH) { /* no shift, no selector build, no look-up: constants */
            SW_EDGES(x_[g] = 0u; s_[g] = c0642; k_[g] = k_fresh;)
        } else {
            SW_EDGES(x_[g] = (j & 7) ? cur.x[j >> 3] >> (j & 7) : cur.x[j >> 3];)
            SW_EDGES(s_[g] = sw_bitop3<SW_TT_ANDOR>(x_[g], c01, c0642);)
            SW_EDGES(k_[g] = sw_perm(kt_hi, kt_lo, s_[g]);)
        }
        /* t + 128, VECTOR_SUB_AND_SATURATE comes in pass 2.  (A rotation-free group has no rotate: this is the first use of its reads,
         * so it takes their descending order; a group with a rotating edge in it keeps the rotates' order) */
        if ((j0 + SW_ILP < NJ ? j0 + SW_ILP : NJ) <= NZ) { _Pragma("unroll") for (int g = SW_ILP - 1; g >= 0; --g) if (j0 + g < NJ) tb[j0 + g] = r_[g] + k_[g]; }
        else { SW_EDGES(tb[j] = r_[g] + k_[g];) }
        if (ERA) {
            SW_EDGES(x_[g] &= c01;)                               /* b: the old message on this edge is negative */
            SW_EDGES(
                if ((era_edges >> j) & 1u) {
                    uint32_t em = 0, match = 0;
                    _Pragma("unroll") for (int k = 0; k < 4; ++k) {
                        const uint32_t a = ad[j] + ((rq[j] + (uint32_t)k) & 3u); /* LDS byte of row k's node on this edge */
                        em |= sw_plane_bit(lds, era_plane, a) ? (0xffu << (8 * k)) : 0u;
                        const uint32_t pold = (k & 1) ? cur.pa[k >> 1] >> 16 : cur.pa[k >> 1] & 0xffffu;
                        match |= (!fresh && a == pold) ? (0xffu << (8 * k)) : 0u;    /* that byte carries the patch */
                    }
                    const uint32_t en_true = r_[g] - (padd & match) + (psub & match);
                    const uint32_t neg01 = ~((en_true + 0x08080808u) >> 7) & c01;      /* En < 0 */
                    tb[j] = sw_bitop3<SW_TT_SEL>(em, c80 + bias, tb[j]);               /* vContr = 0 */
                    x_[g] = sw_bitop3<SW_TT_SEL>(em, neg01, x_[g]);                    /* its sign: the sign of En */
                })
        }
        /* FAID: a zero V2C takes the sign of En (CDecoder_FAID.cpp:682); En == Lold there, so it is the stored sign b: bit 7 of
         * t + 128 - b.  k_ still holds the selector 2 k + b of the edge (the erasing variant rebuilds it from its own b) */
        { SW_MASK_SHIFTS(EPAIRS1, SW_P1_TS, ts[j] = MINSUM ? tb[j] : tb[j] - (ERA ? (x_[g] | c0642) : s_[g]);)
        /* (with pairs the XOR of the sign words comes here for the same reason: between the second pair's shift and the expansions) */
#define SW_SX_STAGE SW_EDGES(                                                                                                            \
            if (WAVES == 2) sx ^= ts[j]; /* (the neighbour edge belongs to the other wave) */                                            \
            else if (j & 1) sx = sw_bitop3<SW_TT_XOR3>(sx, ts[j - 1], ts[j]); else if (j == (DEG > 0 ? DEG : deg) - 1) sx ^= ts[j];)
        if (EPAIRS1) { SW_SX_STAGE }
        SW_MASK_EXPAND(EPAIRS1, SW_P1_MS, SW_P1_TS) }
        /* |t| -> min(|t|, 7) -> thermometer.  With m = 0xff where the (back-tracked) sign is "not negative":
         *   not negative: ts ^ 0x80 = t - b,  |t| = that + b          negative: ts ^ 0x7f = -t - 1 + b,  |t| = that + 1 - b
         * (b = 0 for the min-sum decoders); 0x78 is added on top so that |t| >= 8 reaches bit 7, which the table look-up
         * turns into the saturated code */
        SW_EDGES(a_[g] = sw_bitop3<SW_TT_XOR3>(ts[j], c7f, ms[j]);)
        if (METHOD == 0) {
            /* NMS: 16 levels.  0x70 on top so that |t| >= 16 reaches bit 7 (both look-ups then return the saturated code); bit 3
             * picks the table: entries 8..15 (nms_t[3], nms_t[2]) or 0..7 (nms_t[1], nms_t[0]) */
            uint32_t h_[SW_ILP];
            SW_EDGES(i_[g] = sw_bitop3<SW_TT_NANDOR>(ms[j], c01, K.c70);)
            SW_EDGES(a_[g] = (a_[g] + i_[g]) & 0x8f8f8f8fu;)
            SW_EDGES(h_[g] = sw_mask7(a_[g] << 4, sel_sign);)
            SW_EDGES(a_[g] &= 0x87878787u;)
            SW_EDGES(i_[g] = sw_perm(p.nms_t[3], p.nms_t[2], a_[g]);)
            SW_EDGES(u_[g] = sw_perm(p.nms_t[1], p.nms_t[0], a_[g]);)
            SW_EDGES(u_[g] = sw_bitop3<SW_TT_SEL>(h_[g], i_[g], u_[g]);)
        } else {
            if (FRESH && !MINSUM) { SW_EDGES(i_[g] = sw_bitop3<0x0a>(ms[j], ms[j], c01);) } /* ~a & c: SW_TT_XNOR_AND with x_ == 0 */
            else { SW_EDGES(i_[g] = MINSUM ? sw_bitop3<SW_TT_NANDOR>(ms[j], c01, c78) : sw_bitop3<SW_TT_XNOR_AND>(x_[g], ms[j], c01);) }
            SW_EDGES(a_[g] = (MINSUM ? a_[g] + i_[g] : a_[g] + i_[g] + c78) & 0x87878787u;)     /* v_add3_u32 */
            SW_EDGES(u_[g] = sw_perm(tt_hi, tt_lo, a_[g]);)
        }
        if (!EPAIRS1) { SW_SX_STAGE }
        if (QUADS) {
            uint32_t v_[4];
            _Pragma("unroll") for (int g = 0; g < 4; ++g) v_[g] = j0 + g < NJ ? u_[g] : 0xffffffffu; /* no such edge: "no minimum" */
            sw_min_quad(t1, t2, ta, v_[0], v_[1], v_[2], v_[3], j0);
        } else {
            SW_EDGES(sw_min_edge(t1, t2, ta, u_[g], j);)
        }
    }

    if (WAVES == 2) {
        /* index bit 0 is the wave: ta[0] (edges with the bit clear) is wave 0's own minimum */
        if (WAVE == 1) {
            xch.put(0, t1); xch.put(1, t2); xch.put(2, ta[1]); xch.put(3, ta[2]); xch.put(4, ta[3]); xch.put(5, ta[4]); xch.put(6, sx);
        }
        xch.barrier(); /* B */
        if (WAVE == 0) {
            const uint32_t o1 = xch.get(0), o2 = xch.get(1);
            ta[0] = t1;
            t2 = sw_bitop3<SW_TT_AND3>(t2, o2, t1 | o1); /* second minimum of the union: min(max(m1a, m1b), m2a, m2b) */
            t1 &= o1;
            ta[1] &= xch.get(2); ta[2] &= xch.get(3); ta[3] &= xch.get(4); ta[4] &= xch.get(5);
            sx ^= xch.get(6);
        }
    }
    uint32_t c2n_x = 0, fm_x = 0; /* what wave 1 takes over from wave 0 */
    if (WAVES == 2 && WAVE == 1) {
        xch.barrier(); /* C */
        c2n_x = xch.get(0); fm_x = xch.get(1);
    }

    /* ---- the row's new magnitudes ---- */
    const uint32_t n_lo = WAVES == 2 ? SW_T2N_LO : K.n_lo, n_hi = WAVES == 2 ? SW_T2N_HI : K.n_hi;
    const uint32_t min1 = NOWIN ? 0u : sw_therm2num(t1, n_lo, n_hi), min2 = NOWIN ? 0u : sw_therm2num(t2, n_lo, n_hi);
    uint32_t c1n, c2n;
    if (NOWIN) {
        /* one table, whatever the row's parity: composed with the thermometer decode (cste_2 from min1, cste_1 from min2) */
        c2n = VK ? sw_therm2msg_vk(t1, K.tm, K.c0f) : sw_therm2msg(t1, K.tm);
        c1n = VK ? sw_therm2msg_vk(t2, K.tm, K.c0f) : sw_therm2msg(t2, K.tm);
    } else if (METHOD == 0) {
        /* the levels of the search ARE cste() of the minima (CLDPC.cpp:337-352: cste_2 from min1, cste_1 from min2, one factor) */
        c2n = min1;
        c1n = min2;
    } else if (SW_OMS(METHOD)) {
        /* selective offset and clamp (cste_2 from min1, cste_1 from min2, CDecoder_OMS.cpp:431-432) as table look-ups; rows
         * with an unsatisfied check take the other rule inside the error-floor window of a codeword with few of them (:388) */
        /* (the choice of the second table is uniform and the same for every layer of an iteration: made on the table WORDS - two
         * scalar selects, loop-invariant, which the compiler is relied on to hoist out of the layer loop; tests/test_layer_trip_count.py
         * would show them - instead of on the rows' results.  Outside the window both look-ups read the same table) */
        const bool win = p.window && lme;
        const uint32_t w_lo = win ? p.oms_lo[1] : p.oms_lo[0], w_hi = win ? p.oms_hi[1] : p.oms_hi[0];
        c2n = sw_table_pick(rowpar, w_hi, w_lo, p.oms_hi[0], p.oms_lo[0], min1);
        c1n = sw_table_pick(rowpar, w_hi, w_lo, p.oms_hi[0], p.oms_lo[0], min2);
    } else {
        /* uniform non-decreasing table applied after the search; offset 0 (CDecoder_FAID.cpp:864-866) */
        /* mask_eef per row (CDecoder_FAID.cpp:713-720).  Whether the error-floor table applies at all is uniform and the same for
         * every layer of an iteration: the choice is made on the table WORDS (two scalar selects, loop-invariant: the compiler is
         * relied on to hoist them out of the layer loop, tests/test_layer_trip_count.py would show them), instead of on the rows'
         * results (outside the window both look-ups read the same table) */
        const bool win = (METHOD == 5 || p.ef_tables) && p.window && lme;
        const uint32_t w_lo = win ? p.ef_lo : p.lut_lo, w_hi = win ? p.ef_hi : p.lut_hi;
        c2n = sw_table_pick(rowpar, w_hi, w_lo, p.lut_hi, p.lut_lo, min1);
        c1n = sw_table_pick(rowpar, w_hi, w_lo, p.lut_hi, p.lut_lo, min2);
    }
#if SW_DEV
    /* The magnitudes are complete HERE.  Nothing but the arg-min edge, far below, reads c1n: without a fixed point the instruction
     * selector's list scheduler puts the whole second-minimum chain of pass 1 there and keeps every edge's code alive until then. */
    asm volatile("" : "+v"(c1n), "+v"(c2n));
#endif
    /* new message on edge j is negative iff s_j ^ XOR_all(s) ^ (deg odd) (the 0xC0 / 0x40 constants of
     * CDecoder_FAID.cpp:902-917); with nn_j = bit 7 of ts_j = "V2C not negative" that is: not negative iff nn_j ^ F,
     * F = bit 7 of the XOR of all ts */
    const uint32_t fm = (WAVES == 2 && WAVE == 1) ? fm_x : SW_MASK7(sx);
    if (WAVES == 2 && WAVE == 1) { c2n = c2n_x; c1n = 0u; } /* (everything per row below is wave 0's: dead code here) */

    /* ---- binary index of an edge that attains the minimum.  Bits 0..2: ta[b] runs over the edges whose index has bit b clear,
     * the bit is 1 iff none of them attains it.  Bits 3 and 4 the other way round (fewer edges have them set): ta[3] runs over
     * edges 8..15, ta[4] over edges 16..23, the bit is 1 iff one of them attains it; bit 3 gives way to bit 4.  With a unique
     * minimum that is its index; a tie leaves 16 / 8 / 0 + the AND of the tied indices' low bits, not above one of the tied
     * edges in that range, so still an edge of the row - and in a tie c1 == c2 ---- */
    uint32_t idx = 0, ne7_3 = 0, ne7_4 = 0; /* the decode words of bits 3 and 4, kept for their byte masks below */
    uint32_t idx8 = 0; /* SW_FORM_VK: idx << 3 */
    if (VK) {
        /* The same five bits collected at bit 7 and shifted DOWN into place: bit b enters at bit 7 and is moved right 4 - b times, so
         * the word ends as idx << 3 - no bit ever below bit 3 of its byte, nothing crosses into the byte below - and one more shift
         * gives idx.  Every step reads the one constant 0x80 in a register where the form above reads a one-hot constant per bit (no
         * literal in v_bitop3_b32: an SGPR each), in as many instructions; and 4 * idx, the arg-min table's index, is a RIGHT shift of it. */
        uint32_t n7[5];
#pragma unroll
        for (int b = 0; b < 5; ++b) n7[b] = sw_bitop3<SW_TT_XORAND>(ta[b], t1, c7f) + c7f; /* bit 7 of every byte: ta[b] != t1 */
        ne7_4 = n7[4]; ne7_3 = n7[3];
        const uint32_t b4 = sw_bitop3<0x0a>(n7[4], n7[4], c80); /* ~a & c */
        const uint32_t b3 = sw_bitop3<0x02>(n7[3], b4, c80);    /* ~a & ~b & c: bit 3 gives way to bit 4 */
        uint32_t acc = n7[0] & c80;
        acc = sw_bitop3<SW_TT_ANDOR>(n7[1], c80, acc >> 1);
        acc = sw_bitop3<SW_TT_ANDOR>(n7[2], c80, acc >> 1);
        acc = (acc >> 1) | b3;
        acc = (acc >> 1) | b4;
        idx8 = acc;
        idx = acc >> 3;
    }
#pragma unroll
    for (int b = 4; b >= 0 && !VK; --b) {
        const uint32_t dd = sw_bitop3<SW_TT_XORAND>(ta[b], t1, c7f);
        const uint32_t ne7 = dd + c7f;      /* bit 7 of every byte: ta[b] != t1 */
        const uint32_t ne = ne7 >> (7 - b); /* the same at bit b */
        if (b == 4) ne7_4 = ne7;
        if (b == 3) ne7_3 = ne7;
        /* (a row of the generic instance with no edge in 16..23 / 8..15 leaves that accumulator untouched: bit stays 0) */
        if (b == 4) idx = (DEG == 0 && deg <= 16) ? 0u : ~ne & (0x01010101u << 4);
        else if (b == 3) idx = (DEG == 0 && deg <= 8) ? idx : sw_bitop3<0xf2>(idx, ne | (idx >> 1), 0x01010101u << 3); /* a | (~b & c) */
        else idx = sw_bitop3<SW_TT_ANDNOT_OR>(idx, ne, 0x01010101u << b);
    }

    /* ---- the new arg-min edge: address, exact V2C, exact new En.  Its node address comes from the layer's edge table through
     * ds_bpermute_b32 and its (still old) En from LDS: two dependent round trips, which nothing else of the wave would cover
     * (two waves per SIMD).  Pass 2 does not depend on them, so its first group of edges is computed between the issue of
     * the table look-up and its use, and the rest of it between the issue of the En reads and theirs.  LDS operations of a
     * wave execute in order: the En reads are ISSUED before the first write of pass 2, so they return the old values. ---- */
    uint32_t pa[4], sbk[4], gk0 = 0, gk1 = 0, gk2 = 0, gk3 = 0, xb = 0;
    const uint32_t idx4 = VK ? idx8 >> 1 : idx << 2;
#pragma unroll
#ifdef SW_EXP_NO_ARGMIN /* timing experiment only: results are wrong */
    for (int k = 0; k < 4; ++k) sbk[k] = (cbj[k] << 16) | s4j[k];
#else
    for (int k = 0; k < 4; ++k) sbk[k] = WAVE == 0 ? tab.sb_dyn4((VK ? idx8 >> (8 * k + 1) : idx4 >> (8 * k)) & 0x7cu) : 0u;
#endif
    SW_SCHED_FENCE();

    /* ---- pass 2 (CDecoder_FAID.cpp:909-929, CDecoder_OMS.cpp:452-471): every edge as if it carried c2 ---- */
    const SwUpd2 u2 = sw_update2_consts<MINSUM>(c2n, fm, bias);
    const uint32_t cm27 = (WAVES == 2 || VK) ? 0u - 0x27272727u : K.cm27; /* (two waves per codeword: 128 registers, none to spare for constants) */
    uint32_t ns[3] = { 0u, 0u, 0u };
    uint32_t cbit[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) cbit[e] = K.cbit[e];
    /* one group of edges: the arithmetic (ARITH) and the LDS writes (STORE) separately, stage by stage over the group as in pass 1
     * (the stages of sw_update2) */
#define SW_PASS2_ARITH(J0, EN)                                                                                       \
    {                                                                                                                \
        const int j0 = (J0);                                                                                         \
        uint32_t d_[SW_ILP], zb[SW_ILP], mo[SW_ILP], lm[SW_ILP];                                                     \
        SW_EDGES(d_[g] = sw_upd2_d(ms[j], u2);)                                                                      \
        SW_EDGES(zb[g] = sw_upd2_zb(tb[j], d_[g], u2);)                                                              \
        {                                                                                                            \
            SW_MASK_SHIFTS(EPAIRS2, SW_P2_MO, mo[g] = sw_upd2_out<MINSUM>(zb[g], d_[g], u2);)                        \
            SW_MASK_EXPAND(EPAIRS2, SW_P2_MO, SW_P2_MO)  /* under or over */                                         \
        }                                                                                                            \
        SW_EDGES(lm[g] = sw_upd2_limit<MINSUM>(ms[j], d_[g], u2, c80);)                                              \
        SW_EDGES(EN[g] = sw_upd2_en(mo[g], lm[g], zb[g], d_[g], cm27);)                                              \
        SW_EDGES(if (j >= NZ) EN[g] = sw_alignbyte(EN[g], EN[g], EDGEW ? rq[j] >> 8 : 4u - rq[j]);)                  \
        if (NSTREE) sw_sign_quad<NJ>(ns, ms, j0, deg, DEG > 0, K.c55, K.c33, K.c0f);                                 \
        else SW_EDGES(sw_sign_edge(ns, ms[j], j, cbit[j & 7]);)                                                      \
    }
#define SW_PASS2_STORE(J0, EN)                                                                                       \
    {                                                                                                                \
        const int j0 = (J0);                                                                                         \
        SW_EDGES(lds.wr32(ad[j], EN[g], SW_COL(j));)                                                                 \
        if (EDGEW) ew.at(j0);                                                                                        \
    }
    uint32_t en0[SW_ILP], en1[SW_ILP];
    SW_PASS2_ARITH(0, en0)
    SW_SCHED_FENCE();
#pragma unroll
    for (int k = 0; k < 4; ++k) /* low half: 4 * (lane + shift) < 2048, with the row folded in < 2816; high half: block column * 256 */
        pa[k] = sw_node_addr(tid4 + sbk[k] + ((uint32_t)k << 8));
#ifdef SW_EXP_NO_ARGMIN
    gk0 = ld[0] & 0xffu; gk1 = ld[1] & 0xffu; gk2 = ld[2] & 0xffu; gk3 = ld[3] & 0xffu;
#else
    if (WAVE == 0) { gk0 = lds.rd8(pa[0]); gk1 = lds.rd8(pa[1]); gk2 = lds.rd8(pa[2]); gk3 = lds.rd8(pa[3]); }
#endif
    if (WAVES == 2 && WAVE == 0) { /* the barrier also waits for the reads above: wave 1 may overwrite those nodes from here on */
        xch.put(0, c2n); xch.put(1, fm);
        xch.barrier(); /* C */
    }
    SW_SCHED_FENCE();
    SW_PASS2_STORE(0, en0)
    if (SW_ILP < NJ) { SW_PASS2_ARITH(SW_ILP, en1) SW_PASS2_STORE(SW_ILP, en1) }
    SW_SCHED_FENCE();
    /* the arg-min edges as one-hot bits inside their 8-edge word (byte k: 1 << (index mod 8)) and the word they are in
     * (index div 8 = 0, 1, 2) as byte masks, all four rows at once */
    const uint32_t oh8 = sw_perm(K.oh_hi, K.oh_lo, idx & 0x07070707u);
    /* index bit 4 / bit 3 as byte masks, from the words the index was decoded from (their bit 7: the accumulator differs from the
     * minimum, i.e. the bit is CLEAR): no shifts.  nm3 ignores that bit 3 gives way to bit 4: every use below looks at nm4 first */
    uint32_t nm3, nm4;
    if (RPAIRS && (DEG == 0 || DEG > 16)) { /* (a per-degree instance up to degree 16 has one of them at the most) */
        sw_mask7x2(ne7_3, ne7_4, sel_sign, &nm3, &nm4);
        if (DEG == 0 && deg <= 16) nm4 = 0xffffffffu;
        if (DEG == 0 && deg <= 8) nm3 = 0xffffffffu;
    } else {
        nm4 = (DEG == 0 && deg <= 16) ? 0xffffffffu : sw_mask7(ne7_4, sel_sign);
        nm3 = (DEG == 0 && deg <= 8) ? 0xffffffffu : sw_mask7(ne7_3, sel_sign);
    }
    /* old message on that edge negative: bit (index mod 8) of byte k of sign word (index div 8), as 2 k + b: the v_perm selector */
    /* (FRESH: not negative on any edge, the selector is its row part) */
    const uint32_t selA = FRESH ? c0642 : sw_argmin_selector(sw_word_pick(nm3, nm4, cur.x[0], cur.x[1], cur.x[2]), oh8, c7f, c01, c0642);
    if (ERA) xb = selA & c01;
    const uint32_t gb = MULF ? sw_gather4_perm(gk0, gk1, gk2, gk3) : sw_gather4(gk0, gk1, gk2, gk3);
    uint32_t tbA = gb + (FRESH ? k_fresh : sw_perm(kt_hi, kt_lo, selA)); /* carries `bias` like tb[] */
    if (ERA) { /* the arg-min edge of a row may be an erased one (a V2C of 0 usually IS the minimum) */
        uint32_t em = 0, match = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t ik = (idx >> (8 * k)) & 31u;
            if ((era_edges >> ik) & 1u) em |= sw_plane_bit(lds, era_plane, pa[k]) ? (0xffu << (8 * k)) : 0u;
            const uint32_t pold = (k & 1) ? cur.pa[k >> 1] >> 16 : cur.pa[k >> 1] & 0xffffu;
            match |= (!fresh && pa[k] == pold) ? (0xffu << (8 * k)) : 0u;
        }
        const uint32_t en_true = gb - (padd & match) + (psub & match);
        tbA = sw_bitop3<SW_TT_SEL>(em, c80 + bias, tbA);
        xb = sw_bitop3<SW_TT_SEL>(em, ~((en_true + 0x08080808u) >> 7) & c01, xb);
    }
    const uint32_t tsA = MINSUM ? tbA : tbA - (ERA ? (xb | c0642) : selA);
    const uint32_t msA = SW_MASK7(tsA);
    const uint32_t negA = ~(msA ^ fm); /* byte mask: the new message on the arg-min edge is negative */
    const SwUpd2 u1 = sw_update2_consts<MINSUM>(c1n, fm, bias);
    const uint32_t enA = MULF ? sw_update2_mul<MINSUM>(tbA, msA, u1, sel_sign, c80, cm27, K.c100) : sw_update2<MINSUM>(tbA, msA, u1, sel_sign, c80, cm27);

#pragma unroll
    for (int jg = 2 * SW_ILP; jg < NJ; jg += SW_ILP) { /* the remaining groups of pass 2 */
        uint32_t en[SW_ILP];
        SW_PASS2_ARITH(jg, en)
        SW_PASS2_STORE(jg, en)
    }
#undef SW_EDGES
#undef SW_MASK_SHIFTS
#undef SW_SX_STAGE
#undef SW_MASK_EXPAND
#undef SW_P1_TS
#undef SW_P1_MS
#undef SW_P2_MO
#undef SW_PASS2_ARITH
#undef SW_PASS2_STORE
#undef SW_COL
#undef SW_MASK7
#undef SW_SHL8
    if (WAVES == 2) {
        if (WAVE == 1) { xch.put(0, ns[0]); xch.put(1, ns[1]); xch.put(2, ns[2]); }
        xch.barrier(); /* D: wave 1's En is in LDS */
        if (WAVE == 1) { SwRow none = { { 0u, 0u, 0u }, 0u, { 0u, 0u } }; return none; }
        ns[0] |= xch.get(0); ns[1] |= xch.get(1); ns[2] |= xch.get(2);
    }
    /* the arg-min edge carries c1: its exact En replaces the as-if value pass 2 wrote (same lane, LDS operations in order; with two
     * waves: after barrier D, behind the other wave's as-if value) */
#ifndef SW_EXP_NO_ARGMIN
    {
        const uint32_t eh = sw_opaque(enA >> 8); /* one shift serves both odd bytes */
        lds.wr8(pa[0], enA); lds.wr8(pa[1], eh); lds.wr8(pa[2], enA >> 16); lds.wr8(pa[3], eh >> 16);
    }
#endif

    /* ---- the row's new compressed messages ---- */
    SwRow out;
    const int n = DEG > 0 ? DEG : deg;
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        const int cnt = n - 8 * g < 0 ? 0 : (n - 8 * g > 8 ? 8 : n - 8 * g);
        const uint32_t valid = 0x01010101u * ((1u << cnt) - 1u);
        out.x[g] = ~(ns[g] ^ fm) & ((VK && cnt == 7) ? c7f : valid); /* negative iff not (nn ^ F) */
    }
    if (!MINSUM) {
        /* A zero message has no sign: stored as "not negative" so that the next iteration's back-track reads
         * "Lmn < 0" straight from the bit.  c2 == 0 zeroes every message of the row but the arg-min's. */
        uint32_t z2, z1;
        if (RPAIRS) sw_zero_mask2(c2n, c1n, sel_sign, &z2, &z1);
        else { z2 = sw_zero_mask(c2n, sel_sign); z1 = sw_zero_mask(c1n, sel_sign); }
        const uint32_t nz1 = ~z1;
        const uint32_t keep = oh8 & nz1; /* the arg-min edge's bit survives where its message c1 is not zero */
        uint32_t oh[3];
        sw_word_deal(keep, nm3, nm4, oh);
#pragma unroll
        for (int g = 0; g < 3; ++g) out.x[g] &= ~z2 | oh[g];
    }
    out.cw = c2n | (c1n << 3) | (negA & 0x40404040u);
    out.pa[0] = pa[0] | (pa[1] << 16);
    out.pa[1] = pa[2] | (pa[3] << 16);
    return out;
}

#endif /* LNSFAID_SWAR_H */
