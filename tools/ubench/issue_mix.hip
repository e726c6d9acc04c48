// Micro-benchmark: SIMD cycles per wave64 instruction of the byte-parallel layer step's VALU mix (70 % full-rate class: v_bitop3_b32,
// two-source add / shift; 30 % half-rate class: v_perm_b32, v_alignbyte_b32) as a function of the waves resident per SIMD.
// Unlike issue_rate.hip the loop body is long - BODY straight-line instructions per trip (template recursion, no per-instruction
// control flow) - so the loop's own scalar instructions and branch do not count; CHAINS independent dependency chains per wave,
// as in the layer step's stage-by-stage order.  Single-wave workgroups; the dynamic LDS size sets the residency.
// build: hipcc --offload-arch=gfx950 -O3 -o issue_mix issue_mix.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#define TRIPS 400
#define BODY 480

template <int I, int CHAINS>
__device__ __forceinline__ void body(uint32_t (&a)[8], uint32_t b, uint32_t c)
{
    if constexpr (I < BODY) {
        uint32_t& x = a[I % CHAINS];
        constexpr int m = I % 10; // add, shl, bitop3, perm, bitop3, add, alignbyte, bitop3, perm, bitop3
        if constexpr (m == 3 || m == 8) asm volatile("v_perm_b32 %0, %0, %1, %2" : "+v"(x) : "v"(b), "v"(c));
        else if constexpr (m == 6) asm volatile("v_alignbyte_b32 %0, %0, %1, %2" : "+v"(x) : "v"(b), "v"(c));
        else if constexpr (m == 0 || m == 5) asm volatile("v_add_u32 %0, %0, %1" : "+v"(x) : "v"(b));
        else if constexpr (m == 1) asm volatile("v_lshlrev_b32 %0, 1, %0" : "+v"(x));
        else asm volatile("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(x) : "v"(b), "v"(c));
        body<I + 1, CHAINS>(a, b, c);
    }
}

// The mask expander's shift forms, on four chains (words m[2 i], m[2 i + 1]).  A unit is
//   1 "paired":      v_lshlrev_b64, 2 v_add_u32, 2 v_perm_b32 reading the shift's halves          (two masks, 5 instructions, 3 half-rate)
//   2 "two single":  2 v_lshlrev_b32, 2 v_add_u32, 2 v_perm_b32 reading them                       (two masks, 6 instructions, 4 half-rate)
//   0 / 5 / 3 / 4:   one v_lshlrev_b64 by 8 / v_lshlrev_b32 by 8 / v_pk_lshlrev_b16 by 8 / v_mul_u32_u24 by 256 held in a VGPR
//   6 / 7:           v_mul_u32_u24 by the literal 256 / v_add_u32 (what a full-rate instruction costs in the shift's place)
//                    (the last two: one-for-one stand-ins for v_lshlrev_b32 by 8 in front of the expander's v_perm_b32)
// (the two adds stand between a shift and its readers, as other edges' instructions do in the layer step.)  MIX: the unit inside the
// layer step's 7 : 3 mix - full-rate instructions (v_bitop3_b32 / v_add_u32 alternating) behind it.  "paired" and "two single"
// get the SAME seven (4 half-rate of 13 for the form the kernel had: 31 %), so their difference per unit is what a pair saves
// in place; a lone shift gets a v_perm_b32 and four fillers (2 half-rate of 6).  Times are reported per UNIT.
#define UNITS 60
// A unit is ONE asm statement (between two statements of which the second reads what the first wrote the compiler puts a wait state
// of its own), and consecutive units work on different chains.  Inline asm cannot name the halves of a 64-bit operand, so the
// pairs of "paired" are fixed registers, v[100:101] .. v[106:107], named in the clobber list; their values mean nothing.
#define FILL_X "v_bitop3_b32 %[m0], %[m0], %[b], %[c] bitop3:0x96\n\t"
#define FILL_A "v_add_u32 %[m1], %[m1], %[b]\n\t"
#define FILL_0 ""
#define FILL_4 FILL_X FILL_A FILL_X FILL_A
#define FILL_7 FILL_X FILL_A FILL_X FILL_A FILL_X FILL_A FILL_X
#define ADDS "v_add_u32 %[m0], %[m0], %[b]\n\tv_add_u32 %[m1], %[m1], %[b]\n\t"
#define PAIRED(LO, HI, FILL) asm volatile("v_lshlrev_b64 v[" #LO ":" #HI "], 8, v[" #LO ":" #HI "]\n\t" ADDS "v_perm_b32 %[m0], %[m0], v" #LO ", %[c]\n\tv_perm_b32 %[m1], %[m1], v" #HI ", %[c]\n\t" FILL \
                                          : [m0] "+v"(m0), [m1] "+v"(m1) : [b] "v"(b), [c] "v"(c) : "v" #LO, "v" #HI)
#define SINGLES(FILL) asm volatile("v_lshlrev_b32 %[t0], 8, %[m0]\n\tv_lshlrev_b32 %[t1], 8, %[m1]\n\t" ADDS "v_perm_b32 %[m0], %[m0], %[t0], %[c]\n\tv_perm_b32 %[m1], %[m1], %[t1], %[c]\n\t" FILL \
                                   : [m0] "+v"(m0), [m1] "+v"(m1), [t0] "+v"(t0), [t1] "+v"(t1) : [b] "v"(b), [c] "v"(c))
#define LONE(SHIFT, TAIL) asm volatile(SHIFT "\n\t" TAIL : [m0] "+v"(m0), [m1] "+v"(m1) : [b] "v"(b), [c] "v"(c), [k] "v"(k256))
#define LONE_MIX "v_perm_b32 %[m1], %[m1], %[b], %[c]\n\t" FILL_4
#define LONE_B64(LO, HI, TAIL) asm volatile("v_lshlrev_b64 v[" #LO ":" #HI "], 8, v[" #LO ":" #HI "]\n\t" TAIL : [m0] "+v"(m0), [m1] "+v"(m1) : [b] "v"(b), [c] "v"(c) : "v" #LO, "v" #HI)
#define SHL_B32 "v_lshlrev_b32 %[m0], 8, %[m0]"
#define SHL_PK16 "v_pk_lshlrev_b16 %[m0], 8, %[m0] op_sel_hi:[0,1]"
#define MUL_U24 "v_mul_u32_u24 %[m0], %[m0], %[k]"
#define MUL_LIT "v_mul_u32_u24 %[m0], 0x100, %[m0]"
#define ADD_FULL "v_add_u32 %[m0], %[m0], %[k]"
template <int OP, bool MIX> constexpr int unit_len() { return OP == 1 ? (MIX ? 12 : 5) : OP == 2 ? (MIX ? 13 : 6) : MIX ? 6 : 1; }
template <int I, int OP, bool MIX>
__device__ __forceinline__ void body_pair(uint32_t (&m)[8], uint32_t b, uint32_t c, uint32_t k256, uint32_t (&t)[8])
{
    if constexpr (I < UNITS) {
        uint32_t& t0 = t[2 * (I % 4)];
        uint32_t& t1 = t[2 * (I % 4) + 1];
        uint32_t& m0 = m[2 * (I % 4)];
        uint32_t& m1 = m[2 * (I % 4) + 1];
        if constexpr (OP == 0 && I % 4 == 0) { if constexpr (MIX) LONE_B64(100, 101, LONE_MIX); else LONE_B64(100, 101, ""); }
        else if constexpr (OP == 0 && I % 4 == 1) { if constexpr (MIX) LONE_B64(102, 103, LONE_MIX); else LONE_B64(102, 103, ""); }
        else if constexpr (OP == 0 && I % 4 == 2) { if constexpr (MIX) LONE_B64(104, 105, LONE_MIX); else LONE_B64(104, 105, ""); }
        else if constexpr (OP == 0) { if constexpr (MIX) LONE_B64(106, 107, LONE_MIX); else LONE_B64(106, 107, ""); }
        else if constexpr (OP == 5 && !MIX) LONE(SHL_B32, "");
        else if constexpr (OP == 5) LONE(SHL_B32, LONE_MIX);
        else if constexpr (OP == 3 && !MIX) LONE(SHL_PK16, "");
        else if constexpr (OP == 3) LONE(SHL_PK16, LONE_MIX);
        else if constexpr (OP == 4 && !MIX) LONE(MUL_U24, "");
        else if constexpr (OP == 4) LONE(MUL_U24, LONE_MIX);
        else if constexpr (OP == 6 && !MIX) LONE(MUL_LIT, "");
        else if constexpr (OP == 6) LONE(MUL_LIT, LONE_MIX);
        else if constexpr (OP == 7 && !MIX) LONE(ADD_FULL, "");
        else if constexpr (OP == 7) LONE(ADD_FULL, LONE_MIX);
        else if constexpr (OP == 2 && !MIX) SINGLES(FILL_0);
        else if constexpr (OP == 2) SINGLES(FILL_7);
        else if constexpr (I % 4 == 0) { if constexpr (MIX) PAIRED(100, 101, FILL_7); else PAIRED(100, 101, FILL_0); }
        else if constexpr (I % 4 == 1) { if constexpr (MIX) PAIRED(102, 103, FILL_7); else PAIRED(102, 103, FILL_0); }
        else if constexpr (I % 4 == 2) { if constexpr (MIX) PAIRED(104, 105, FILL_7); else PAIRED(104, 105, FILL_0); }
        else { if constexpr (MIX) PAIRED(106, 107, FILL_7); else PAIRED(106, 107, FILL_0); }
        body_pair<I + 1, OP, MIX>(m, b, c, k256, t);
    }
}

// The 64-bit shift and its readers, a unit per asm statement on the fixed pairs of "paired", four chains:
//   6 "b64, no reader":   v_lshlrev_b64, 2 v_add_u32 that do not read it                                        (3 instructions)
//   7 "b64, reader at 2": v_lshlrev_b64, v_add_u32, the wait state the compiler puts there, v_add_u32 reading the low half  (3 + s_nop)
//   8 "two mul lit":      2 v_mul_u32_u24 by the literal 256, 2 v_add_u32 of which one reads a product          (4 instructions)
//   9 "two shl":          2 v_lshlrev_b32 by 8, 2 v_add_u32 of which one reads a shifted word                   (4 instructions)
#define B64_FREE(LO, HI) asm volatile("v_lshlrev_b64 v[" #LO ":" #HI "], 8, v[" #LO ":" #HI "]\n\t" ADDS : [m0] "+v"(m0), [m1] "+v"(m1) : [b] "v"(b) : "v" #LO, "v" #HI)
#define B64_READ(LO, HI) asm volatile("v_lshlrev_b64 v[" #LO ":" #HI "], 8, v[" #LO ":" #HI "]\n\tv_add_u32 %[m0], %[m0], %[b]\n\ts_nop 0\n\tv_add_u32 %[m1], %[m1], v" #LO "\n\t" \
                                      : [m0] "+v"(m0), [m1] "+v"(m1) : [b] "v"(b) : "v" #LO, "v" #HI)
template <int I, int OP>
__device__ __forceinline__ void body_b64(uint32_t (&m)[8], uint32_t b, uint32_t (&t)[8])
{
    if constexpr (I < UNITS) {
        uint32_t& t0 = t[2 * (I % 4)];
        uint32_t& t1 = t[2 * (I % 4) + 1];
        uint32_t& m0 = m[2 * (I % 4)];
        uint32_t& m1 = m[2 * (I % 4) + 1];
        if constexpr (OP == 6 && I % 4 == 0) B64_FREE(100, 101);
        else if constexpr (OP == 6 && I % 4 == 1) B64_FREE(102, 103);
        else if constexpr (OP == 6 && I % 4 == 2) B64_FREE(104, 105);
        else if constexpr (OP == 6) B64_FREE(106, 107);
        else if constexpr (OP == 7 && I % 4 == 0) B64_READ(100, 101);
        else if constexpr (OP == 7 && I % 4 == 1) B64_READ(102, 103);
        else if constexpr (OP == 7 && I % 4 == 2) B64_READ(104, 105);
        else if constexpr (OP == 7) B64_READ(106, 107);
        else if constexpr (OP == 8) asm volatile("v_mul_u32_u24 %[t0], 0x100, %[m0]\n\tv_mul_u32_u24 %[t1], 0x100, %[m1]\n\tv_add_u32 %[m0], %[m0], %[b]\n\tv_add_u32 %[m1], %[m1], %[t0]\n\t"
                                                 : [m0] "+v"(m0), [m1] "+v"(m1), [t0] "+v"(t0), [t1] "+v"(t1) : [b] "v"(b));
        else asm volatile("v_lshlrev_b32 %[t0], 8, %[m0]\n\tv_lshlrev_b32 %[t1], 8, %[m1]\n\tv_add_u32 %[m0], %[m0], %[b]\n\tv_add_u32 %[m1], %[m1], %[t0]\n\t"
                          : [m0] "+v"(m0), [m1] "+v"(m1), [t0] "+v"(t0), [t1] "+v"(t1) : [b] "v"(b));
        body_b64<I + 1, OP>(m, b, t);
    }
}
template <int OP>
__global__ __launch_bounds__(64) void k_b64(uint32_t* out, uint32_t seed)
{
    extern __shared__ uint32_t dyn[];
    uint32_t m[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) m[i] = seed * (2 * i + 5) + threadIdx.x;
    uint32_t b = seed * 31 + 1;
    uint32_t t[8] = { 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u };
    for (int r = 0; r < TRIPS; ++r) body_b64<0, OP>(m, b, t);
    uint32_t s = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) s ^= m[i] ^ t[i];
    if (dyn[0] == 0x12345678u) s ^= 1;
    out[blockIdx.x * 64 + threadIdx.x] = s;
}

template <int OP, bool MIX>
__global__ __launch_bounds__(64) void k_pair(uint32_t* out, uint32_t seed)
{
    extern __shared__ uint32_t dyn[];
    uint32_t m[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) m[i] = seed * (2 * i + 5) + threadIdx.x;
    uint32_t b = seed * 31 + 1, c = seed ^ 0x12345, k256 = 256u;
    uint32_t t[8] = { 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u }; // (scratch registers of "two single", a pair per chain)
    asm volatile("" : "+v"(k256));
    for (int r = 0; r < TRIPS; ++r) body_pair<0, OP, MIX>(m, b, c, k256, t);
    uint32_t s = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) s ^= m[i];
    if (dyn[0] == 0x12345678u) s ^= 1;
    out[blockIdx.x * 64 + threadIdx.x] = s;
}

// one instruction class per kernel: what each costs at the decode kernel's residency (two waves per SIMD)
// 0 v_add_u32 (two sources)  1 v_bitop3_b32  2 v_perm_b32  3 v_alignbyte_b32  4 v_add3_u32  5 v_and_or_b32  6 v_add_u32 with an SGPR source
// 7 v_and_or_b32 with an SGPR source  8 v_lshlrev_b32 (inline constant)  9 v_and_b32 with a 32-bit literal
// 10 v_mov_b32_sdwa (byte 1 of the source)  11 v_or_b32_sdwa (byte 0 of one source)  12 the same with an SGPR source  13 v_lshrrev_b32 by 8
// 14 v_lshlrev_b32 by 8  15 v_lshrrev_b32 by 1  16 / 17 the shifts by a register  18 v_sub_u32
// the candidates of DESIGN.md 3.1j: 19 v_mul_u32_u24 by the literal 256  20 v_mul_u32_u24 by 256 held in a VGPR  21 v_mul_lo_u32
// 22 v_mad_u32_u24  23 v_lshl_add_u32  24 v_lshl_or_b32  25 v_add_u32 x, x, x (a left shift by one)  26 v_bitop3_b32 with an SGPR source
// 27 v_mul_u32_u24 by 256 held in an SGPR
template <int I, int OP>
__device__ __forceinline__ void body_one(uint32_t (&a)[8], uint32_t b, uint32_t c, uint32_t sg, uint32_t k256)
{
    if constexpr (I < BODY) {
        uint32_t& x = a[I % 4];
        if constexpr (OP == 0) asm volatile("v_add_u32 %0, %0, %1" : "+v"(x) : "v"(b));
        else if constexpr (OP == 1) asm volatile("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(x) : "v"(b), "v"(c));
        else if constexpr (OP == 2) asm volatile("v_perm_b32 %0, %0, %1, %2" : "+v"(x) : "v"(b), "v"(c));
        else if constexpr (OP == 3) asm volatile("v_alignbyte_b32 %0, %0, %1, %2" : "+v"(x) : "v"(b), "v"(c));
        else if constexpr (OP == 4) asm volatile("v_add3_u32 %0, %0, %1, %2" : "+v"(x) : "v"(b), "v"(c));
        else if constexpr (OP == 5) asm volatile("v_and_or_b32 %0, %0, %1, %2" : "+v"(x) : "v"(b), "v"(c));
        else if constexpr (OP == 6) asm volatile("v_add_u32 %0, %1, %0" : "+v"(x) : "s"(sg));
        else if constexpr (OP == 7) asm volatile("v_and_or_b32 %0, %0, %1, %2" : "+v"(x) : "v"(b), "s"(sg));
        else if constexpr (OP == 8) asm volatile("v_lshlrev_b32 %0, 1, %0" : "+v"(x));
        else if constexpr (OP == 10) asm volatile("v_mov_b32_sdwa %0, %0 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_1" : "+v"(x));
        else if constexpr (OP == 11) asm volatile("v_or_b32_sdwa %0, %1, %0 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0" : "+v"(x) : "v"(b));
        else if constexpr (OP == 12) asm volatile("v_or_b32_sdwa %0, %1, %0 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0" : "+v"(x) : "s"(sg));
        else if constexpr (OP == 13) asm volatile("v_lshrrev_b32 %0, 8, %0" : "+v"(x));
        else if constexpr (OP == 14) asm volatile("v_lshlrev_b32 %0, 8, %0" : "+v"(x));
        else if constexpr (OP == 15) asm volatile("v_lshrrev_b32 %0, 1, %0" : "+v"(x));
        else if constexpr (OP == 16) asm volatile("v_lshlrev_b32 %0, %1, %0" : "+v"(x) : "v"(b));
        else if constexpr (OP == 17) asm volatile("v_lshrrev_b32 %0, %1, %0" : "+v"(x) : "v"(b));
        else if constexpr (OP == 18) asm volatile("v_sub_u32 %0, %0, %1" : "+v"(x) : "v"(b));
        else if constexpr (OP == 19) asm volatile("v_mul_u32_u24 %0, 0x100, %0" : "+v"(x));
        else if constexpr (OP == 20) asm volatile("v_mul_u32_u24 %0, %0, %1" : "+v"(x) : "v"(k256));
        else if constexpr (OP == 21) asm volatile("v_mul_lo_u32 %0, %0, %1" : "+v"(x) : "v"(k256));
        else if constexpr (OP == 22) asm volatile("v_mad_u32_u24 %0, %0, %1, %2" : "+v"(x) : "v"(k256), "v"(c));
        else if constexpr (OP == 23) asm volatile("v_lshl_add_u32 %0, %0, 8, %1" : "+v"(x) : "v"(c));
        else if constexpr (OP == 24) asm volatile("v_lshl_or_b32 %0, %0, 8, %1" : "+v"(x) : "v"(c));
        else if constexpr (OP == 25) asm volatile("v_add_u32 %0, %0, %0" : "+v"(x));
        else if constexpr (OP == 26) asm volatile("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(x) : "v"(b), "s"(sg));
        else if constexpr (OP == 27) asm volatile("v_mul_u32_u24 %0, %1, %0" : "+v"(x) : "s"(sg));
        else asm volatile("v_and_b32 %0, 0x87878787, %0" : "+v"(x));
        body_one<I + 1, OP>(a, b, c, sg, k256);
    }
}

template <int OP>
__global__ __launch_bounds__(64) void k_one(uint32_t* out, uint32_t seed)
{
    extern __shared__ uint32_t dyn[];
    uint32_t a[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = seed * (2 * i + 3) + threadIdx.x;
    uint32_t b = seed * 31 + 1, c = seed ^ 0x12345;
    const uint32_t sg = seed * 7;
    uint32_t k256 = 256u;
    asm volatile("" : "+v"(k256));
    for (int r = 0; r < TRIPS; ++r) body_one<0, OP>(a, b, c, sg, k256);
    uint32_t s = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) s ^= a[i];
    if (dyn[0] == 0x12345678u) s ^= 1;
    out[blockIdx.x * 64 + threadIdx.x] = s;
}

template <int CHAINS>
__global__ __launch_bounds__(64) void k(uint32_t* out, uint32_t seed)
{
    extern __shared__ uint32_t dyn[];
    uint32_t a[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = seed * (2 * i + 3) + threadIdx.x;
    uint32_t b = seed * 31 + 1, c = seed ^ 0x12345;
    for (int r = 0; r < TRIPS; ++r) body<0, CHAINS>(a, b, c);
    uint32_t s = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) s ^= a[i];
    if (dyn[0] == 0x12345678u) s ^= 1; // keep the LDS allocation
    out[blockIdx.x * 64 + threadIdx.x] = s;
}

// one wave ALONE on its SIMD: 64 KB of LDS per single-wave workgroup, so a CU holds two of them (on two of its four SIMDs)
template <typename K> void run_alone(K kern, const char* name, uint32_t* d, double ghz)
{
    const size_t lds = 65536 - 512;
    const int rounds = 4, blocks = 256 * 2 * rounds;
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(64), lds, 0, d, 1u);
    (void)hipDeviceSynchronize();
    (void)hipEventRecord(e0);
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(64), lds, 0, d, 2u);
    (void)hipEventRecord(e1); (void)hipEventSynchronize(e1);
    float ms;
    (void)hipEventElapsedTime(&ms, e0, e1);
    printf("%-10s  1 wave alone on its SIMD (2 per CU)      %8.3f ms  %5.2f SIMD-cycles per wave-instruction\n", name, ms,
           ms * 1e-3 * ghz * 1e9 / ((double)rounds * TRIPS * BODY));
}

template <typename K> void run(K kern, const char* name, uint32_t* d, int waves_per_simd, double ghz)
{
    // waves per CU = 4 x waves per SIMD: dynamic LDS such that exactly that many single-wave workgroups fit (160 KB per CU)
    const size_t lds = (size_t)(160 * 1024 / (4 * waves_per_simd)) - 512;
    const int rounds = 4;
    const int blocks = 256 * 4 * waves_per_simd * rounds;
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(64), lds, 0, d, 1u);
    (void)hipDeviceSynchronize();
    (void)hipEventRecord(e0);
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(64), lds, 0, d, 2u);
    (void)hipEventRecord(e1); (void)hipEventSynchronize(e1);
    float ms;
    (void)hipEventElapsedTime(&ms, e0, e1);
    const double inst_per_simd = (double)blocks / 1024.0 * TRIPS * BODY;
    printf("%-10s %2d waves/SIMD (LDS %6zu B/wave)  %8.3f ms  %5.2f SIMD-cycles per wave-instruction\n", name, waves_per_simd, lds, ms,
           ms * 1e-3 * ghz * 1e9 / inst_per_simd);
}

// the shift forms: SIMD cycles per UNIT and per issued instruction
template <typename K> void run_unit(K kern, const char* name, int len, uint32_t* d, int waves_per_simd, double ghz)
{
    const size_t lds = waves_per_simd == 1 ? 65536 - 512 : (size_t)(160 * 1024 / (4 * waves_per_simd)) - 512;
    const int rounds = 4;
    // (one wave per SIMD: 64 KB of LDS per single-wave workgroup lets a CU hold two, on two of its SIMDs: run_alone's shape)
    const int blocks = waves_per_simd == 1 ? 256 * 2 * rounds : 256 * 4 * waves_per_simd * rounds;
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(64), lds, 0, d, 1u);
    (void)hipDeviceSynchronize();
    (void)hipEventRecord(e0);
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(64), lds, 0, d, 2u);
    (void)hipEventRecord(e1); (void)hipEventSynchronize(e1);
    float ms;
    (void)hipEventElapsedTime(&ms, e0, e1);
    const double units_per_simd = (waves_per_simd == 1 ? (double)rounds : (double)blocks / 1024.0) * TRIPS * UNITS;
    const double cyc = ms * 1e-3 * ghz * 1e9 / units_per_simd;
    printf("%-34s %d waves/SIMD  %8.3f ms  %6.2f SIMD-cycles per unit of %d  = %5.2f per instruction\n", name, waves_per_simd, ms, cyc, len, cyc / len);
}
#define RUN_UNIT(OP, MIX, NAME, W) run_unit(k_pair<OP, MIX>, NAME, unit_len<OP, MIX>(), d, W, ghz)

int shift_forms(uint32_t* d, double ghz)
{
    printf("shift forms of the mask expander; 'paired' and 'two single' make two masks per unit, the lone shifts are one instruction:\n");
    for (int w : { 1, 2, 8 }) {
        RUN_UNIT(5, false, "v_lshlrev_b32 8", w);
        RUN_UNIT(0, false, "v_lshlrev_b64 8", w);
        RUN_UNIT(3, false, "v_pk_lshlrev_b16 8", w);
        RUN_UNIT(4, false, "v_mul_u32_u24 256 (VGPR)", w);
        RUN_UNIT(1, false, "paired: b64, 2 add, 2 perm", w);
        RUN_UNIT(2, false, "two single: 2 b32, 2 add, 2 perm", w);
        RUN_UNIT(5, true, "mix: v_lshlrev_b32, perm, 4 full", w);
        RUN_UNIT(0, true, "mix: v_lshlrev_b64, perm, 4 full", w);
        RUN_UNIT(3, true, "mix: v_pk_lshlrev_b16, perm, 4 full", w);
        RUN_UNIT(4, true, "mix: v_mul_u32_u24, perm, 4 full", w);
        RUN_UNIT(1, true, "mix: paired + 7 full", w);
        RUN_UNIT(2, true, "mix: two single + 7 full", w);
    }
    return 0;
}

// "classes": the table of DESIGN.md 3.1j - one class per kernel at two waves per SIMD, the 64-bit shift's units, and the lone shift forms in the mix
int issue_classes(uint32_t* d, double ghz)
{
    printf("one instruction class per kernel, four chains, two waves per SIMD:\n");
    const int w = 2;
    run(k_one<0>, "add", d, w, ghz);
    run(k_one<18>, "sub", d, w, ghz);
    run(k_one<1>, "bitop3", d, w, ghz);
    run(k_one<26>, "bitop3 sg", d, w, ghz);
    run(k_one<9>, "and lit", d, w, ghz);
    run(k_one<13>, "shr 8", d, w, ghz);
    run(k_one<14>, "shl 8", d, w, ghz);
    run(k_one<25>, "add x,x,x", d, w, ghz);
    run(k_one<6>, "add sgpr", d, w, ghz);
    run(k_one<2>, "perm", d, w, ghz);
    run(k_one<4>, "add3", d, w, ghz);
    run(k_one<19>, "mul24 lit", d, w, ghz);
    run(k_one<20>, "mul24 vgpr", d, w, ghz);
    run(k_one<27>, "mul24 sgpr", d, w, ghz);
    run(k_one<21>, "mul_lo", d, w, ghz);
    run(k_one<22>, "mad24", d, w, ghz);
    run(k_one<23>, "lshl_add", d, w, ghz);
    run(k_one<24>, "lshl_or", d, w, ghz);
    printf("the 64-bit shift and what could stand in for it, per unit:\n");
    run_unit(k_b64<6>, "b64, 2 add, no reader", 3, d, w, ghz);
    run_unit(k_b64<7>, "b64, add, s_nop, add reading it", 3, d, w, ghz);
    run_unit(k_b64<8>, "2 mul24 lit, 2 add (one reads)", 4, d, w, ghz);
    run_unit(k_b64<9>, "2 shl 8, 2 add (one reads)", 4, d, w, ghz);
    printf("a lone left shift by 8 in the layer step's mix (shift, perm, 4 full-rate):\n");
    RUN_UNIT(5, true, "mix: v_lshlrev_b32, perm, 4 full", w);
    RUN_UNIT(4, true, "mix: v_mul_u32_u24 VGPR, perm, 4 full", w);
    RUN_UNIT(6, true, "mix: v_mul_u32_u24 lit, perm, 4 full", w);
    RUN_UNIT(7, true, "mix: v_add_u32 (full), perm, 4 full", w);
    return 0;
}

int main(int argc, char** argv)
{
    hipDeviceProp_t p;
    (void)hipGetDeviceProperties(&p, 0);
    const double ghz = p.clockRate / 1e6;
    printf("%s  CUs %d  clock %.2f GHz; mix: 7 full-rate : 3 half-rate VALU, %d straight-line instructions per loop trip\n", p.name,
           p.multiProcessorCount, ghz, BODY);
    uint32_t* d;
    (void)hipMalloc(&d, (size_t)256 * 4 * 8 * 4 * 64 * 4);
    if (argc > 1 && argv[1][0] == 's') return shift_forms(d, ghz); // "shifts": only the table of DESIGN.md 3.1h
    if (argc > 1 && argv[1][0] == 'c') return issue_classes(d, ghz); // "classes": only the table of DESIGN.md 3.1j
    run_alone(k<4>, "4 chains", d, ghz);
    run_alone(k<8>, "8 chains", d, ghz);
    for (int w : { 2, 3, 4, 5, 8 }) {
        run(k<4>, "4 chains", d, w, ghz);
        run(k<8>, "8 chains", d, w, ghz);
    }
    printf("one instruction class per kernel, four chains:\n");
    for (int w : { 2, 8 }) {
        run(k_one<0>, "add", d, w, ghz);
        run(k_one<8>, "shl 1", d, w, ghz);
        run(k_one<9>, "and lit", d, w, ghz);
        run(k_one<1>, "bitop3", d, w, ghz);
        run(k_one<2>, "perm", d, w, ghz);
        run(k_one<3>, "alignbyte", d, w, ghz);
        run(k_one<4>, "add3", d, w, ghz);
        run(k_one<5>, "and_or", d, w, ghz);
        run(k_one<6>, "add sgpr", d, w, ghz);
        run(k_one<7>, "and_or sg", d, w, ghz);
        run(k_one<13>, "shr 8", d, w, ghz);
        run(k_one<14>, "shl 8", d, w, ghz);
        run(k_one<15>, "shr 1", d, w, ghz);
        run(k_one<16>, "shl vgpr", d, w, ghz);
        run(k_one<17>, "shr vgpr", d, w, ghz);
        run(k_one<18>, "sub", d, w, ghz);
        run(k_one<10>, "mov sdwa", d, w, ghz);
        run(k_one<11>, "or sdwa", d, w, ghz);
        run(k_one<12>, "or sdwa sg", d, w, ghz);
    }
    run_alone(k_one<0>, "add", d, ghz);
    run_alone(k_one<1>, "bitop3", d, ghz);
    run_alone(k_one<2>, "perm", d, ghz);
    return 0;
}
