/*
 * lnsfaid.h — C ABI of the MI355X-native batched LDPC decoder (50G-PON QC-LDPC, every value of the reference's
 * DecodeMethod switch: 0 NMS, 1 OMS, 2 LNS-FAID + DTBF, 3 OMS + BF, 4 OMS + DTBF, 5 LNS-FAID + 2B1C).
 *
 * This is the drop-in boundary for the reference's decoder member functions
 *   void CLDPC::Decode_OMS()        (reference CLDPC.h:148, CDecoder_OMS.cpp:13)
 *   void CLDPC::Decode_FAID()       (reference CLDPC.h:149, CDecoder_FAID.cpp:176)
 *   void CLDPC::Decode_FAID_2B1C()  (reference CLDPC.h:152, CDecoder_FAID_2B1C.cpp:96)
 *   void CLDPC::Decode()            (reference CLDPC.h:146, CLDPC.cpp:214; DecodeMethod 0 / default: normalised min-sum,
 *                                    Factor_1 / Factor_2 are numerators over 32, fixed iteration count, no early stop)
 *   int  CLDPC::Decode_OMSBF()      (reference CLDPC.h:150, CDecoder_OMSBF.cpp:13; DecodeMethod 3: the layered loop of
 *                                    Decode_OMS followed by plain bit flipping with threshold min(max vote, 5))
 *   int  CLDPC::Decode_OMS_DTBF()   (reference CLDPC.h:151, CDecoder_OMS_DTBF.cpp:18; DecodeMethod 4: the layered
 *                                    loop of Decode_OMS followed by the DTBF stage of Decode_FAID with other constants)
 *   Statistic CLDPC::CalculateErrors(...) (reference CLDPC.h:169, CLDPC.cpp:4819)
 * The reference has no FFI layer: inputs/outputs are the members `fixInput` /
 * `decodedBits` of `class CLDPC` (CLDPC.h:125-126) and the configuration is read
 * from Profile.txt (CTool.cpp:588-621) plus compile-time constants at the top of
 * each decoder file.  The entry points below carry exactly that information as
 * plain pointers and sizes.  INTEGRATION.md shows the CLDPC-side binding.
 *
 * Conventions: extern "C"; 0 = success, negative = error (lnsfaid_strerror);
 * no exceptions and no exit() across the boundary; the caller owns every host
 * buffer it passes, the context owns device buffers and its HIP stream.  One
 * context per (host thread, GPU): thread-compatible, not thread-safe.
 *
 * Batches are consecutive GROUPS of 32 codewords.  By default the group is part
 * of the contract: the reference decodes 32 codewords in lock-step and stops a
 * group only when all 32 lanes are clean (CDecoder_FAID.cpp:616, :6782), which
 * is observable in the hard decisions; this library reproduces it bit for bit.
 * lnsfaid_set_early_stop(ctx, LNSFAID_STOP_CODEWORD) and lnsfaid_decode_codewords
 * let every codeword stop on its own instead (still in groups of 32 in memory).
 */
#ifndef LNSFAID_H
#define LNSFAID_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LNSFAID_GROUP 32 /* codewords per group = Profile.txt noFrames = lanes of the reference's __m256i */

/* error codes */
#define LNSFAID_OK 0
#define LNSFAID_E_INVAL (-1)    /* bad argument / unsupported configuration          */
#define LNSFAID_E_CODE (-2)     /* H table is not the quasi-cyclic shape the kernels need */
#define LNSFAID_E_NOMEM (-3)    /* host or device allocation failed                  */
#define LNSFAID_E_HIP (-4)      /* a HIP runtime call failed (see lnsfaid_last_hip_error) */
#define LNSFAID_E_NODEVICE (-5) /* no usable GPU / extension built without device code */
#define LNSFAID_E_INTERNAL (-6)

/*
 * Code definition = the content of the reference's Constants_SSE.h
 * (Constants/50GPON-dc-original/Constants_SSE.h:4-19 and :29-3102).
 */
typedef struct lnsfaid_code {
    int32_t n_var;           /* _NoVar   17664 */
    int32_t n_check;         /* _NoCheck 3072  */
    int32_t n_edges;         /* _NoOnes  70400 */
    int32_t z;               /* Profile.txt Z  256 (circulant size) */
    int32_t puncture_tail;   /* number of tail VNs whose channel LLR is forced to 0
                                (CDecoder_FAID.cpp:253-255: 384) */
    int32_t nb_degres;       /* NB_DEGRES: number of consecutive row-degree classes */
    const int32_t* deg;      /* [nb_degres] DEG_k */
    const int32_t* deg_rows; /* [nb_degres] DEG_k_COMPUTATIONS */
    const uint16_t* pos_vn;  /* [n_edges] PosNoeudsVariable, row-major VN indices */
} lnsfaid_code;

/*
 * Decoder configuration = Profile.txt run-time keys + the compile-time
 * constants at the top of CDecoder_OMS.cpp / CDecoder_FAID.cpp /
 * CDecoder_FAID_2B1C.cpp.  lnsfaid_cfg_default() fills in the reference's
 * shipped values for a DecodeMethod.
 */
typedef struct lnsfaid_cfg {
    int32_t decode_method;     /* Profile.txt DecodeMethod 0..5 (README.md:13; 0 = NMS, CLDPC::Decode) */
    int32_t max_iteration;     /* Profile.txt MaxIteration (nb_iteration)           */
    int32_t factor_1;          /* Profile.txt Factor_1: OMS selective offset (>= 0), NMS numerator over 32 of min1 */
    int32_t factor_2;          /* Profile.txt Factor_2: OMS (>= 1: smaller values leave the 3-bit alphabet, E_INVAL), NMS numerator of min2 */
    int32_t floor_err_count;   /* CDecoder_OMS.cpp:28 (100) / FAID :193 (0) / 2B1C :117 (50) */
    int32_t floor_iter_thresh; /* CDecoder_OMS.cpp:29 (4)  / FAID :194 (-1) / 2B1C :118 (6) */
    int32_t ef_elimination;    /* EF_ELIMINATION 0 (FAID :6), 1 (2B1C :5) or, DecodeMethod 2 only, 2 (FAID :673-680) */
    int32_t max_bf_iter;       /* _maxBFiter 10 (CDecoder_FAID.cpp:208); 0 for OMS   */
    int32_t bf_L0;             /* _L0 50 (FAID :168) / 100 (2B1C :88)                */
    int32_t bf_L1;             /* _L1 0                                              */
    int32_t bf_alpha;          /* _alpha 1                                           */
    int32_t bf_delta;          /* _delta 1                                           */
    int32_t regular_col_weight;/* REGULAR_COL_WEIGHT 3 (CTool.h:6)                   */
    int32_t hard2_threshold;   /* 13 (CDecoder_FAID_2B1C.cpp:6130)                   */
    int32_t bf_vote_cap;       /* 5: plain BF flips votes >= min(max_vote, 5) (CDecoder_OMSBF.cpp:3332) */
    /* V2C_map_it{1..6}_[weight class 3,6,11,other][min(|t|,7)] (CDecoder_FAID.cpp:12-49) */
    int8_t v2c_map[6][4][8];
    /* V2C_map_it{1..6}_ef (CDecoder_FAID.cpp:130-165) */
    int8_t v2c_map_ef[6][4][8];
} lnsfaid_cfg;

/* per-group execution record (used for the algorithmic-byte accounting) */
typedef struct lnsfaid_group_stats {
    int32_t iterations;    /* I: layered iterations executed by the group            */
    int32_t bf_iterations; /* J: bit-flipping iterations that reached the flip step  */
} lnsfaid_group_stats;

/* per-codeword execution record (lnsfaid_decode_codewords): what the reference reports for a group of 32 copies of the codeword */
typedef struct lnsfaid_codeword_stats {
    int32_t iterations;    /* I: layered iterations the codeword executed                                          */
    int32_t bf_iterations; /* J: bit-flipping iterations that reached the flip step                                */
    int32_t unsatisfied;   /* parity checks the RETURNED decodedBits leave unsatisfied, over all n_var bits (the
                            * punctured tail included): 0 means the output is a codeword                          */
} lnsfaid_codeword_stats;

typedef struct lnsfaid_ctx lnsfaid_ctx;

/* ---- code / configuration helpers (host only, no GPU needed) ---------------- */

/* Number of edges / VNs / checks of the built-in 50G-PON mother code and its
 * expansion into the Constants_SSE.h table format.  `pos_vn` must hold 70400
 * entries.  Returns LNSFAID_OK. */
int lnsfaid_code_50gpon(lnsfaid_code* code, uint16_t* pos_vn, int32_t* deg3, int32_t* deg_rows3);

/* Fill `cfg` with the reference's shipped constants for DecodeMethod 0..5. */
int lnsfaid_cfg_default(lnsfaid_cfg* cfg, int32_t decode_method, int32_t max_iteration);

/* Replace cfg->v2c_map by one of the table sets the reference selects at compile time in CDecoder_FAID.cpp
 * (#define FAID3 - the shipped default -, FAID32 or FAID2, CDecoder_FAID.cpp:8, :12-127). */
#define LNSFAID_TABLES_FAID3 0
#define LNSFAID_TABLES_FAID32 1
#define LNSFAID_TABLES_FAID2 2
int lnsfaid_cfg_table_preset(lnsfaid_cfg* cfg, int32_t preset);

/* The reference's compile-time switch EF_ELIMINATION of Decode_FAID (CDecoder_FAID.cpp:6, :192-203) for a DecodeMethod 2
 * configuration: 0 = off (the shipped build: floor_err_count 0, floor_iter_thresh -1), 1 = error-floor tables V2C_map_it*_ef
 * on unsatisfied rows inside the window (100, 6), 2 = the same plus the erasure of CDecoder_FAID.cpp:673-680 (20, 6): inside the
 * window the V2C message of a variable node of column weight REGULAR_COL_WEIGHT all of whose checks were unsatisfied at the
 * iteration's syndrome stage is set to 0, once per iteration.  Modes 1 and 2 need tables that are uniform over the weight classes
 * and non-decreasing (lnsfaid_create / lnsfaid_set_cfg return LNSFAID_E_INVAL otherwise). */
int lnsfaid_cfg_ef_elimination(lnsfaid_cfg* cfg, int32_t mode);

/* ---- decoder context --------------------------------------------------------- */

/* Replaces CLDPC::Initial (CLDPC.cpp:4772-4817): validates the code (must be
 * quasi-cyclic with circulant size z and no repeated block column inside a
 * block row), uploads the tables and allocates device state for up to
 * `max_groups` groups on GPU `device`. */
int lnsfaid_create(lnsfaid_ctx** ctx, const lnsfaid_code* code, const lnsfaid_cfg* cfg,
                   int32_t device, size_t max_groups);
void lnsfaid_destroy(lnsfaid_ctx* ctx);

/* Change the run-time configuration (the reference re-reads Profile.txt on
 * every Decode_* call, CDecoder_FAID.cpp:178-179). */
int lnsfaid_set_cfg(lnsfaid_ctx* ctx, const lnsfaid_cfg* cfg);

/* ---- the hot path ------------------------------------------------------------ */

/*
 * Replaces Decode_OMS / Decode_FAID / Decode_FAID_2B1C for n_groups groups.
 *   fixInput    host, int8 in [-7,7], per group the reference layout
 *               [32][K] information LLRs followed by [32][M] parity LLRs
 *               (CLDPC.h:126, CDecoder_FAID.cpp:217-241); group g starts at
 *               g * 32 * n_var.
 *   decodedBits host, int8 0/1, per group [32][n_var] (CLDPC.h:125,
 *               CDecoder_FAID.cpp:7102); group g starts at g * 32 * n_var.
 *   stats       optional, [n_groups].
 */
int lnsfaid_decode(lnsfaid_ctx* ctx, const int8_t* fixInput, size_t n_groups,
                   int8_t* decodedBits, lnsfaid_group_stats* stats);
/* The reference's call shape - one group per call from T worker threads, each with its own CLDPC / context (reference
 * CSimulate.cpp:136-164, main.cpp:164-172) - is served by a call combiner: the concurrent lnsfaid_decode calls of contexts
 * created with max_groups == 1 on the same device and for the same code are decoded in common launches (from four such
 * contexts on; results bit-identical to separate launches; the call still returns only when its own group is done).
 * Environment: LNSFAID_COALESCE=0 switches it off, LNSFAID_COMB_WORKERS (1..4, default 2) sets the batches in flight,
 * LNSFAID_COMB_BATCHES (default: the number of workers) into how many batches the members' calls are cut,
 * LNSFAID_SYNC=spin|block overrides how the host waits for the GPU (default: sleep from five live contexts on). */

/* Same with device-resident buffers (pointers valid on the context's GPU).  Work is queued on the context's stream; the
 * call synchronises with it once per kernel launch (it reads back how many codewords are still open: 1 launch when
 * nothing converges, typically 3 with early stop) and returns after the batch is complete.  d_stats optional. */
int lnsfaid_decode_device(lnsfaid_ctx* ctx, const int8_t* d_fixInput, size_t n_groups,
                          int8_t* d_decodedBits, lnsfaid_group_stats* d_stats);

/* ---- early stop per codeword ----------------------------------------------------------------------
 * LNSFAID_STOP_GROUP (the default) is the reference's rule: a group stops at the first decision point at which all 32 codewords
 * are clean, and until then clean codewords keep iterating (and bit flipping).  Under LNSFAID_STOP_CODEWORD every codeword stops
 * at the first decision point at which it is itself clean (the syndrome stage in front of every layered iteration, then the one
 * in front of every bit-flipping iteration).  Decoding codeword c under that rule gives exactly what the reference gives for a
 * group of 32 copies of c (hard decisions, I and J), and the batch is decoded in one launch.  DecodeMethod 0 has no early stop:
 * both rules give the same output.  Under the per-codeword rule the group_stats of a group are the maxima of I and of J over
 * its 32 codewords.  Configurations that run on the two-rows-per-lane kernel (DecodeMethod 0 with two normalisation factors,
 * FAID tables that are not uniform over the weight classes) and contexts with lnsfaid_select_waves(ctx, 2) in effect have no
 * per-codeword decoder: their decodes under the per-codeword rule return LNSFAID_E_INVAL. */
#define LNSFAID_STOP_GROUP 0
#define LNSFAID_STOP_CODEWORD 1
/* The rule of every later lnsfaid_decode / lnsfaid_decode_device call of ctx, through the call combiner too (calls of contexts
 * with different rules never share a launch).  LNSFAID_E_INVAL for another value.  lnsfaid_early_stop returns the rule. */
int lnsfaid_set_early_stop(lnsfaid_ctx* ctx, int32_t rule);
int lnsfaid_early_stop(const lnsfaid_ctx* ctx);
/* lnsfaid_decode / lnsfaid_decode_device under the per-codeword rule whatever the context's setting, with a record per codeword:
 *   cw_stats  optional, [n_groups * 32] in decodedBits order (host pointer / device pointer on the context's GPU)
 * A one-group context that asks for cw_stats decodes on its own stream, not through the call combiner. */
int lnsfaid_decode_codewords(lnsfaid_ctx* ctx, const int8_t* fixInput, size_t n_groups, int8_t* decodedBits,
                             lnsfaid_codeword_stats* cw_stats);
int lnsfaid_decode_codewords_device(lnsfaid_ctx* ctx, const int8_t* d_fixInput, size_t n_groups, int8_t* d_decodedBits,
                                    lnsfaid_codeword_stats* d_cw_stats);

/*
 * Replaces CLDPC::CalculateErrors (CLDPC.cpp:4842-4876) for n_groups groups:
 * compares the first K bits of every decoded frame with inputBits
 * ([32][K] per group, int8 0/1) and ADDS to
 *   out[0] TestFrame, out[1] ErrorFrame, out[2] ErrorBits, out[3] LT3ErrBitFrame.
 * inputBits == NULL means the all-zero codeword (FakeEncoder with the shipped
 * CodeWord_sym, CLDPC.cpp:163 / Codeword.h:4).
 */
int lnsfaid_count_errors(lnsfaid_ctx* ctx, const int8_t* decodedBits, const int8_t* inputBits,
                         size_t n_groups, uint64_t out[4]);
int lnsfaid_count_errors_device(lnsfaid_ctx* ctx, const int8_t* d_decodedBits,
                                const int8_t* d_inputBits, size_t n_groups, uint64_t out[4]);

/* ---- packed decode I/O --------------------------------------------------------------------------------
 * The same decodes with 4-bit LLRs in and one bit per decision out: 11 040 instead of 35 328 bytes per 50G-PON codeword.
 *   llr4  packed fixInput.  Elements in the order of fixInput (per group [32][K] information LLRs, then [32][M] parity LLRs;
 *         group g starts at byte g * 16 * n_var).  Element e is a 4-bit two's-complement nibble in byte e / 2: the low nibble
 *         when e is even, the high one when e is odd.  The nibble 0x8 (-8) decodes exactly as the int8 value -8 does.
 *   bits  packed decodedBits.  Per codeword n_var / 32 little-endian 32-bit words in the order of decodedBits, codeword c of
 *         the batch at word c * n_var / 32; bit b of word w is decodedBits[32 w + b] (numpy: packbits(..., bitorder="little")).
 *         The information bits are the first K / 32 words of a codeword.
 *   msg   packed message bits for the counters: per codeword K bits in the same bit order, codeword c at byte c * K / 8; NULL
 *         means the all-zero codeword.
 * Device pointers (the _device calls) must be 4-byte aligned, LNSFAID_E_INVAL otherwise; host pointers may have any alignment
 * (they are copied through packed staging buffers of the context, allocated at its first packed host call).  n_var, K and M
 * are multiples of z = 256, so every offset above is a multiple of 128 bytes.
 * Results, stats, cw_stats and counters are those of the int8 calls for the same data.  Configurations of the four-rows kernel
 * decode in packed twins of its kernels; the others (two-rows kernel, lnsfaid_select_waves(ctx, 2)) convert on the device
 * through the buffers of lnsfaid_io_buffers (their content is overwritten) and, like the int8 calls, return LNSFAID_E_INVAL
 * under the per-codeword rule.  Host calls of one-group contexts decode on the context's own stream, not through the call
 * combiner.  NULL buffers with n_groups > 0 and n_groups > max_groups: LNSFAID_E_INVAL; n_groups 0: no-op. */
int lnsfaid_decode_packed(lnsfaid_ctx* ctx, const uint8_t* llr4, size_t n_groups, uint32_t* bits, lnsfaid_group_stats* stats);
int lnsfaid_decode_packed_device(lnsfaid_ctx* ctx, const uint8_t* d_llr4, size_t n_groups, uint32_t* d_bits,
                                 lnsfaid_group_stats* d_stats);
int lnsfaid_decode_codewords_packed(lnsfaid_ctx* ctx, const uint8_t* llr4, size_t n_groups, uint32_t* bits,
                                    lnsfaid_codeword_stats* cw_stats);
int lnsfaid_decode_codewords_packed_device(lnsfaid_ctx* ctx, const uint8_t* d_llr4, size_t n_groups, uint32_t* d_bits,
                                           lnsfaid_codeword_stats* d_cw_stats);
/* lnsfaid_count_errors on packed decisions and message bits (XOR and popcount over the K information bits of a codeword) */
int lnsfaid_count_errors_packed(lnsfaid_ctx* ctx, const uint32_t* bits, const uint8_t* msg, size_t n_groups, uint64_t out[4]);
int lnsfaid_count_errors_packed_device(lnsfaid_ctx* ctx, const uint32_t* d_bits, const uint8_t* d_msg, size_t n_groups,
                                       uint64_t out[4]);
/* Host only, no context, no GPU.  lnsfaid_pack_llr4: n_values int8 LLRs (even count, each in [-8, 7]) -> n_values / 2 bytes of
 * llr4.  lnsfaid_unpack_bits: n_bits (a multiple of 32) packed decisions -> int8 0/1.  lnsfaid_pack_bits: n_bits (a multiple
 * of 8) int8 0/1 message bits -> n_bits / 8 bytes.  LNSFAID_E_INVAL for a count or a value outside these rules (the output is
 * then incomplete). */
int lnsfaid_pack_llr4(const int8_t* fixInput, size_t n_values, uint8_t* llr4);
int lnsfaid_unpack_bits(const uint32_t* bits, size_t n_bits, int8_t* decodedBits);
int lnsfaid_pack_bits(const int8_t* inputBits, size_t n_bits, uint8_t* packed);

/* ---- line-format decode --------------------------------------------------------------------------------
 * Decode on the format a line delivers: codeword after codeword in transmission order, one bit or one 4-bit LLR per transmitted
 * code bit, any number of codewords; the K payload bits out, contiguous.  Let L = n_var - puncture_tail (50G-PON: 17 280) and
 * K = n_var - n_check (14 592).  Both must be multiples of 32, LNSFAID_E_INVAL otherwise.
 *   line, LNSFAID_LINE_HARD   L / 32 little-endian 32-bit words per codeword, codeword c at word c * L / 32.  Bit b of word w is
 *            the received bit of code-bit position 32 w + b, in the order of decodedBits: the information bits, then the
 *            transmitted parity bits.  A 1 bit enters the decoder as +magnitude, a 0 bit as -magnitude (positive means bit 1, as
 *            everywhere in this library), magnitude in 1 .. 7.
 *   line, LNSFAID_LINE_LLR4   L / 2 bytes per codeword, codeword c at byte c * L / 2.  Element k (code-bit position k) is a
 *            two's-complement nibble in byte k / 2, the low nibble when k is even: the nibble rule of llr4, -8 included.  magnitude
 *            is ignored.
 *   payload  K / 32 words per codeword, codeword c at word c * K / 32; bit b of word w is decoded bit 32 w + b: the msg format of
 *            lnsfaid_count_errors_packed, so the payloads of consecutive codewords are one contiguous bit stream
 *            (lnsfaid_unpack_bits(payload, n_codewords * K, ...) gives them as int8 0 / 1).
 *   bits     optional (NULL: not written): the packed decisions of the packed decode I/O, n_var / 32 words per codeword, so that
 *            lnsfaid_fec_status_packed_* and lnsfaid_count_errors_packed_* can follow (with the llr4 of lnsfaid_line_to_llr4).
 *   stats    optional, [n_codewords] lnsfaid_line_stats.
 * No gaps, no padding: the calls read exactly n_codewords * L / 32 words (LLR4: n_codewords * L / 2 bytes) and write exactly
 * n_codewords entries of each output, nothing outside.
 * Decoding is always under the per-codeword rule (LNSFAID_STOP_CODEWORD), whatever lnsfaid_set_early_stop says: a group rule has
 * no meaning on a line.  lnsfaid_line_to_llr4 is the definition of what is decoded: for every codeword the line calls return what
 * lnsfaid_decode_codewords_packed* returns for that llr4 - the first K / 32 words as payload, all words as bits, and iterations,
 * bf_iterations and unsatisfied.
 * n_codewords: 0 (a no-op, the buffers may be NULL) .. 32 * max_groups.  LNSFAID_E_INVAL: more codewords than that; a format
 * other than the two; LNSFAID_LINE_HARD with a magnitude outside 1 .. 7; a NULL line or payload with n_codewords > 0; a device
 * pointer that is not 4-byte aligned (more alignment only widens loads and stores; host pointers may have any alignment, they go
 * through staging buffers of the context); a configuration without a per-codeword decoder (the two-rows kernel,
 * lnsfaid_select_waves(ctx, 2)), as lnsfaid_decode_codewords.  The device call queues on the context's stream and returns when
 * the outputs are complete. */
#define LNSFAID_LINE_HARD 0
#define LNSFAID_LINE_LLR4 1
typedef struct lnsfaid_line_stats {
    int32_t iterations;    /* as lnsfaid_codeword_stats */
    int32_t bf_iterations; /* as lnsfaid_codeword_stats */
    int32_t unsatisfied;   /* as lnsfaid_codeword_stats: 0 means payload and bits are those of a codeword */
    int32_t corrected;     /* lnsfaid_fec_record::corrected: the positions k < L at which the decoded bit differs from the channel's
                            * own decision - the line bit (HARD), nibble > 0 (LLR4) */
} lnsfaid_line_stats;
int lnsfaid_decode_line(lnsfaid_ctx* ctx, const void* line, int32_t format, int32_t magnitude, size_t n_codewords,
                        uint32_t* payload, uint32_t* bits, lnsfaid_line_stats* stats);
int lnsfaid_decode_line_device(lnsfaid_ctx* ctx, const void* d_line, int32_t format, int32_t magnitude, size_t n_codewords,
                               uint32_t* d_payload, uint32_t* d_bits, lnsfaid_line_stats* d_stats);
/* Host only, no context, no GPU; of the code only n_var, n_check and puncture_tail are read.  Host pointers of any alignment.
 * lnsfaid_line_from_fixinput: the int8 group layout of lnsfaid_decode (ceil(n_codewords / 32) whole groups on the input side
 *   only) -> line of n_codewords codewords.  LLR4: a re-layout that drops the punctured tail; a transmitted value outside
 *   -8 .. 7 is LNSFAID_E_INVAL (the output is then incomplete).  HARD: the bit is x > 0.  The tail's values are never read.
 * lnsfaid_line_to_llr4: line -> the llr4 group layout of ceil(n_codewords / 32) groups; the punctured tail and the padding
 *   codewords are nibble 0.  HARD: +-magnitude (1 .. 7, else LNSFAID_E_INVAL); LLR4: magnitude is ignored.
 * Both: LNSFAID_E_INVAL for a NULL code, a bad format, L or K not a multiple of 32, a NULL buffer with n_codewords > 0;
 * n_codewords 0 is a no-op. */
int lnsfaid_line_from_fixinput(const lnsfaid_code* code, const int8_t* fixInput, size_t n_codewords, int32_t format, void* line);
int lnsfaid_line_to_llr4(const lnsfaid_code* code, const void* line, int32_t format, int32_t magnitude, size_t n_codewords,
                         uint8_t* llr4);

/* ---- line-format encode --------------------------------------------------------------------------------
 * The transmit side of the line-format decode: the payload bit stream in, codeword after codeword in transmission order out, any
 * number of codewords, nothing one byte per bit.  Let L = n_var - puncture_tail (50G-PON: 17 280), K = n_var - n_check (14 592) and
 * N = n_var (17 664).  All three must be multiples of 32 and L must not be below K (the information bits are all transmitted),
 * LNSFAID_E_INVAL otherwise.
 *   payload  exactly the payload of lnsfaid_decode_line: K / 32 little-endian 32-bit words per codeword, codeword c at word
 *            c * K / 32; bit b of word w is information bit 32 w + b.  The payloads of consecutive codewords are one contiguous bit
 *            stream.
 *   line     exactly LNSFAID_LINE_HARD: L / 32 words per codeword, codeword c at word c * L / 32; bit b of word w is code bit
 *            32 w + b in the order of decodedBits.  The first K / 32 words are the payload's own words, the next (L - K) / 32 the
 *            transmitted parity bits p = B^-1 A u (H = [A | B], see the systematic encoder below).  No gaps, no padding.
 *   bits     optional (NULL: not written, and the punctured parity rows are not computed): the whole mother codeword in the format
 *            of the packed decode I/O's bits, N / 32 words per codeword, codeword c at word c * N / 32.  Its first L / 32 words are
 *            the codeword's line words, the rest the punctured parity bits: the "sent" word of a simulator, and what
 *            lnsfaid_fec_status_packed_* and lnsfaid_count_errors_packed_* take as bits.
 * The calls read exactly n_codewords * K / 32 words and write exactly n_codewords entries of each output, nothing outside.
 * n_codewords: 0 (a no-op, the buffers may be NULL) .. 32 * max_groups.  LNSFAID_E_INVAL: a NULL context; more codewords than that;
 * a NULL payload or line with n_codewords > 0; a device pointer (payload, line or bits) that is not 4-byte aligned (more alignment
 * only widens loads and stores: 16-byte accesses when a buffer starts on 16 bytes and its codewords are a multiple of four words
 * long).  Host pointers may have any alignment: they go through the context's packed staging buffers (one copy each way), as
 * lnsfaid_decode_line's do.  A refused call writes nothing.
 * B^-1 is the one the systematic encoder below derives, lazily and once per context: a code whose parity part is singular gives
 * LNSFAID_E_CODE from these calls too, and decoding on that context is not affected.  The calls do not depend on the decoder
 * configuration: no DecodeMethod, kernel selection (two-rows kernel, lnsfaid_select_waves(ctx, 2)) or early-stop rule refuses them
 * or changes their output.  The device call queues on the context's stream and returns when the outputs are complete.
 * lnsfaid_encode_line_host: host only, no context, no GPU, host pointers of any alignment; the definition of what the two calls
 * above return, for any quasi-cyclic code lnsfaid_create accepts.  From the code it reads the dimensions (z included), deg,
 * deg_rows and pos_vn; circ is what lnsfaid_code_parity_inverse returned for that code (a NULL circ or circ_bytes below
 * mb * mb * z / 8, mb = n_check / z: LNSFAID_E_INVAL, n_codewords 0 included).  No limit on n_codewords. */
int lnsfaid_encode_line(lnsfaid_ctx* ctx, const uint32_t* payload, size_t n_codewords, uint32_t* line, uint32_t* bits);
int lnsfaid_encode_line_device(lnsfaid_ctx* ctx, const uint32_t* d_payload, size_t n_codewords, uint32_t* d_line, uint32_t* d_bits);
int lnsfaid_encode_line_host(const lnsfaid_code* code, const uint8_t* circ, size_t circ_bytes, const uint32_t* payload,
                             size_t n_codewords, uint32_t* line, uint32_t* bits);

/* ---- line-format link -----------------------------------------------------------------------------------
 * What sits between and around lnsfaid_encode_line_device and lnsfaid_decode_line_device, so that a hard-decision sweep - post-FEC
 * error rate against the pre-FEC bit error rate of a binary symmetric channel (BSC) - runs on the device in the line's own formats:
 * payload drawn on the device -> encode_line -> BSC -> decode_line (LNSFAID_LINE_HARD) -> counters; only the counters leave it.
 * L = n_var - puncture_tail (50G-PON: 17 280) and K = n_var - n_check (14 592) as in the two sections above.
 *
 * Generator (stateless, counter-based).  With mix64 as defined for lnsfaid_frontend_random_frames below and all arithmetic mod 2^64:
 *   cwkey(key, C, d)   = mix64(mix64(key + d) + (C + 1) * 0xD1B54A32D192ED03)      d = 1: payload, d = 2: BSC
 *   draw(key, C, d, q) = mix64(cwkey(key, C, d) + (q + 1) * 0x9E3779B97F4A7C15)
 * C = first_codeword + i is the global number of codeword i of the call, a uint64_t that wraps.  A run split into calls of any size,
 * or over ranks, therefore produces the bytes of the one-shot run.
 *
 * Payload source.  payload is the payload of the line calls (K / 32 words per codeword, codeword i of the call at word i * K / 32).
 * For codeword C, word 2 q is the low half of draw(key, C, 1, q) and word 2 q + 1 its high half; an odd K / 32 leaves the last high
 * half unused.  Exactly n_codewords * K / 32 words are written.
 *
 * BSC.  line_in and line_out are LNSFAID_LINE_HARD (L / 32 words per codeword).  Position 2 q of codeword C (bit (2 q) % 32 of its word
 * (2 q) / 32) is inverted iff (uint32_t)draw(key, C, 2, q) < threshold, position 2 q + 1 iff draw(key, C, 2, q) >> 32 < threshold, for
 * q < L / 2: every position flips with probability exactly threshold / 2^32, independently.  threshold 0 copies the line.
 *   line_out == line_in is allowed (in place); any other overlap of the two is undefined.
 *   flips        optional uint32_t [n_codewords] (the _device form: a device pointer): the positions inverted per codeword.
 *   total_flips  optional host uint64_t, ADDED to: the positions inverted in the call.
 * lnsfaid_line_bsc_threshold (host only): *threshold = floor(p * 2^32) for 0 <= p < 1; LNSFAID_E_INVAL otherwise (1.0, a negative p,
 * NaN) and for a NULL threshold, which is then not written.
 *
 * Counters.  payload and sent are payload streams (K / 32 words per codeword); sent == NULL means the all-zero payload.  stats is the
 * lnsfaid_line_stats [n_codewords] of the decode call, or NULL.  errors, fec and vs_sent are host uint64_t[4]; each may be NULL, each
 * is ADDED to, and each is four words so that lnsfaid_allreduce_counters sums it unchanged.  w = the bits of a codeword's payload that
 * differ from sent:
 *   errors   the words of lnsfaid_count_errors: [0] TestFrame += n_codewords, [1] ErrorFrame w > 0, [2] ErrorBits += w,
 *            [3] LT3ErrBitFrame w == 1 or w == 2.
 *   fec      the words of lnsfaid_fec_status_*'s out: [0] TotalCodewords += n_codewords, [1] UncorrectableCodewords unsatisfied > 0,
 *            [2] CorrectedCodewords unsatisfied == 0 and corrected > 0, [3] CorrectedBits the sum of corrected over unsatisfied == 0.
 *   vs_sent  as in that section: [0] TestFrame += n_codewords, [1] ErrorFrame w > 0, [2] UndetectedErrorFrame w > 0 and
 *            unsatisfied == 0, [3] FalseAlarmFrame w == 0 and unsatisfied > 0.
 * fec or vs_sent non-NULL with stats NULL is LNSFAID_E_INVAL.  iterations and bf_iterations of stats are not read.
 *
 * Rules for all of these, as for the line calls: n_codewords 0 is a no-op (every buffer may be NULL).  LNSFAID_E_INVAL: a NULL
 * context or code; L or K not a multiple of 32; more than 32 * max_groups codewords (device forms); a NULL required buffer (payload,
 * line_in, line_out); a device pointer, optional ones included, that is not 4-byte aligned (more alignment only widens loads and
 * stores: 16-byte accesses when every buffer of the call starts on 16 bytes and its codewords are a multiple of four words long,
 * 8-byte ones likewise).  A refused call writes nothing and adds nothing.
 * The device forms queue on the context's stream and return when their host outputs are complete (the device outputs are complete
 * on the stream by then); no synchronisation by the caller is needed between them and the line calls.  They do not depend on the
 * decoder configuration.  Their accumulators - the twelve counters, read back in one copy, and the flipped bits - live on the
 * context's device, are allocated at first use and freed by lnsfaid_destroy.
 * The host forms need no context and no GPU, read only n_var, n_check and puncture_tail of the code, take pointers of any alignment
 * and have no limit on n_codewords: they are the definition of what the device forms return. */
int lnsfaid_line_payload_random_device(lnsfaid_ctx* ctx, uint64_t key, uint64_t first_codeword, size_t n_codewords, uint32_t* d_payload);
int lnsfaid_line_payload_random_host(const lnsfaid_code* code, uint64_t key, uint64_t first_codeword, size_t n_codewords, uint32_t* payload);
int lnsfaid_line_bsc_threshold(double p, uint32_t* threshold);
int lnsfaid_line_bsc_device(lnsfaid_ctx* ctx, const uint32_t* d_line_in, size_t n_codewords, uint64_t key, uint64_t first_codeword,
                            uint32_t threshold, uint32_t* d_line_out, uint32_t* d_flips, uint64_t* total_flips);
int lnsfaid_line_bsc_host(const lnsfaid_code* code, const uint32_t* line_in, size_t n_codewords, uint64_t key, uint64_t first_codeword,
                          uint32_t threshold, uint32_t* line_out, uint32_t* flips, uint64_t* total_flips);
int lnsfaid_line_count_errors_device(lnsfaid_ctx* ctx, const uint32_t* d_payload, const uint32_t* d_sent, const lnsfaid_line_stats* d_stats,
                                     size_t n_codewords, uint64_t errors[4], uint64_t fec[4], uint64_t vs_sent[4]);
int lnsfaid_line_count_errors_host(const lnsfaid_code* code, const uint32_t* payload, const uint32_t* sent, const lnsfaid_line_stats* stats,
                                   size_t n_codewords, uint64_t errors[4], uint64_t fec[4], uint64_t vs_sent[4]);

/* ---- line-format soft channel ----------------------------------------------------------------------------
 * The soft-decision counterpart of the BSC above: a binary-input, 15-level, symmetric memoryless channel that reads LNSFAID_LINE_HARD
 * (what lnsfaid_encode_line_device writes) and writes LNSFAID_LINE_LLR4 (what lnsfaid_decode_line_device reads), so that
 * payload -> encode_line -> soft channel -> decode_line (LNSFAID_LINE_LLR4) -> counters runs on the device, and soft input can be
 * compared with hard decisions on the same codewords.  Integer arithmetic only: every output nibble is a pure function of (key,
 * codeword number, position, table), and the host form is the definition.
 *
 * Generator: the link's, with a third domain - cwkey(key, C, 3) and draw(key, C, 3, q) as written out above, C = first_codeword + i,
 * wrapping.  Position 2 q of a codeword uses the low 32 bits u of draw q, position 2 q + 1 the high 32 bits, for q < L / 2.
 * table: fourteen uint32_t thresholds, non-decreasing (a host pointer in both forms).  m = -7 + #{ i : u >= table[i] }, in -7 .. 7.
 * The output level is m where the line bit is 1 and -m where it is 0 (positive means bit 1, as everywhere): the channel is symmetric by
 * construction.  The level is stored as the two's-complement nibble of LNSFAID_LINE_LLR4: byte k / 2, the low nibble for even k; -8
 * never occurs.  Hence P(m = l) = (table[l + 7] - table[l + 6]) / 2^32 exactly, with table[-1] = 0 and table[14] = 2^32.
 *   flips        optional uint32_t [n_codewords] (the _device form: a device pointer): per codeword, the positions at which the
 *                channel's own decision level > 0 differs from the line bit - the rule of lnsfaid_line_stats::corrected.  A sent 1 at
 *                level 0 counts, a sent 0 at level 0 does not.
 *   total_flips  optional host uint64_t, ADDED to: their sum over the call.  The pre-FEC BER of a run is total_flips / (n * L).
 * lnsfaid_line_awgn_table (host only): the table of y = +-1 + N(0, sigma^2) behind the reference's 4-bit quantiser
 * (float2LimitChar_4bit): level = clamp(trunc(y * scale), -7, 7), truncation toward zero.  The boundaries are b_i = j_i / scale for
 * j = -7 .. -1, 1 .. 7 (level 0 is the double-width bin) and table[i] = min(floor(2^32 * Phi((b_i - 1) / sigma)), 2^32 - 1) with
 * Phi(x) = erfc(-x / sqrt 2) / 2 in double.  LNSFAID_E_INVAL for a NULL table or a sigma or scale that is not finite and positive; the
 * table is then not written.  Any other non-decreasing table is as valid an input - a receiver's measured level histogram, summed up.
 * Rules: the link's.  n_codewords 0 is a no-op.  LNSFAID_E_INVAL: a NULL context or code; L or K not a multiple of 32; more than
 * 32 * max_groups codewords (device form); a NULL line_in, llr4_out or table; a device pointer, optional ones included, that is not
 * 4-byte aligned (an output on 16 bytes is written 16 bytes at a time); a table that decreases somewhere; and, because the output is
 * four times the input and in-place use is impossible, any overlap of the byte ranges of line_in and llr4_out.  A refused call writes
 * nothing and adds nothing.  The device form queues on the context's stream and returns when total_flips is complete; its accumulator
 * is the link's.  It does not depend on the decoder configuration.  The host form needs no context and no GPU, takes pointers of any
 * alignment and has no limit on n_codewords. */
int lnsfaid_line_awgn_table(double sigma, double scale, uint32_t table[14]);
int lnsfaid_line_soft_device(lnsfaid_ctx* ctx, const uint32_t* d_line_in, size_t n_codewords, uint64_t key, uint64_t first_codeword,
                             const uint32_t table[14], uint8_t* d_llr4_out, uint32_t* d_flips, uint64_t* total_flips);
int lnsfaid_line_soft_host(const lnsfaid_code* code, const uint32_t* line_in, size_t n_codewords, uint64_t key, uint64_t first_codeword,
                           const uint32_t table[14], uint8_t* llr4_out, uint32_t* flips, uint64_t* total_flips);

/* ---- burst-format line calls ------------------------------------------------------------------------------
 * The line-format decode and encode for bursts: lines whose codewords are individually *shortened*.  A burst ends where its
 * allocation ends, so its last codeword carries fewer than K payload bits: the payload is padded with known zeros up to K, the
 * parity is computed over the padded word, and the pad is not transmitted.  These calls take such lines as they are, any mix of
 * shortenings in one call, with no expanded image in memory.  N = n_var, K = n_var - n_check, L = n_var - puncture_tail as in the
 * line sections; all three must be multiples of 32, LNSFAID_E_INVAL otherwise.
 *   shortened  const uint32_t [n_codewords]: S_c, the shortening of codeword c in bits.  A *host* pointer in every form, the device
 *            forms included (as `table` is for lnsfaid_line_soft_device); NULL means all zero.  The rule is S_c % 32 == 0 and
 *            0 <= S_c <= K - 32; anything else is LNSFAID_E_INVAL, and a refused call writes nothing.  Word granularity is
 *            deliberate: every format of the line calls is word-based, and with it every codeword of a burst stays 4-byte aligned.
 *            Bit-granular shortening is out of scope.
 *   where    uniform over the call: where the known zeros sit in the information part.  LNSFAID_SHORTEN_TAIL: positions
 *            K - S_c .. K - 1 (the reference's _ShortenBits convention); LNSFAID_SHORTEN_HEAD: positions 0 .. S_c - 1.  With
 *            k0 = K - S_c or 0 the known range is [k0, k0 + S_c) in both cases.  Any other value is LNSFAID_E_INVAL.
 *   burst line  codeword c occupies (L - S_c) / 32 words (LNSFAID_LINE_HARD) or (L - S_c) / 2 bytes (LNSFAID_LINE_LLR4), back to back
 *            with no gaps.  Inside a codeword the order is the mother codeword's positions 0 .. L - 1 with the known range removed;
 *            bit and nibble order are exactly those of the line formats.
 *   burst payload  codeword c occupies (K - S_c) / 32 words, back to back: the information bits with the known range removed.  The
 *            payloads of a burst are still one contiguous bit stream.
 *   bits     optional, decode and encode, unchanged: the whole mother codeword, N / 32 words per codeword at a fixed stride, known
 *            positions included.  On encode the known positions are 0; on decode they hold what the decoder decided, so
 *            lnsfaid_fec_status_packed_* can follow (with the llr4 of lnsfaid_burst_to_llr4).
 * A known position enters the decoder as level -7: positive means bit 1 everywhere in this library, and -7 is the strongest level a
 * line can carry.  A decoder may still decide 1 there, so the decode calls also return that count:
 *   stats    optional, lnsfaid_line_stats [n_codewords]; the struct is unchanged.  `corrected` counts transmitted positions only: the
 *            mother positions < L outside the known range at which the decision differs from the channel's own.
 *   short_ones  optional, uint32_t [n_codewords]: the known positions decided as 1.  A receiver treats short_ones > 0 like
 *            unsatisfied > 0.
 * One definition, as for the line calls: lnsfaid_burst_to_llr4 lays a burst line out as the llr4 of ceil(n_codewords / 32) whole
 * groups - known range nibble -7, punctured tail and padding codewords nibble 0, the rest as lnsfaid_line_to_llr4 - and for every
 * codeword the burst decode returns what lnsfaid_decode_codewords_packed* returns for that llr4: all words as bits, the information
 * words minus the known ones as payload, and iterations, bf_iterations and unsatisfied.  With shortened == NULL (or all zero) every
 * output is byte for byte that of lnsfaid_decode_line* / lnsfaid_encode_line*.
 * lnsfaid_encode_burst_host is the definition of the encode calls: the payload expanded with zeros in the known range,
 * lnsfaid_encode_line_host, the known words dropped from the line; circ and circ_bytes as there.
 * lnsfaid_burst_words: host only; validates `shortened` by the rule above and returns the totals of a burst as bit counts (sum of
 * L - S_c and of K - S_c; either pointer may be NULL), with which the caller sizes line and payload.
 * Every other rule is that of the corresponding line call: n_codewords 0 (a no-op) .. 32 * max_groups; device pointers 4-byte
 * aligned, host pointers of any alignment (they go through the context's staging buffers); decoding under the per-codeword rule
 * (the two-rows kernel and lnsfaid_select_waves(ctx, 2) are refused); encoding independent of the decoder configuration, with
 * LNSFAID_E_CODE for a singular parity part; the calls return when the outputs are complete.  On the GPU only the built-in code's
 * circulant size is served, as for the line calls. */
#define LNSFAID_SHORTEN_TAIL 0
#define LNSFAID_SHORTEN_HEAD 1
int lnsfaid_decode_burst(lnsfaid_ctx* ctx, const void* line, int32_t format, int32_t magnitude, const uint32_t* shortened, int32_t where,
                         size_t n_codewords, uint32_t* payload, uint32_t* bits, lnsfaid_line_stats* stats, uint32_t* short_ones);
int lnsfaid_decode_burst_device(lnsfaid_ctx* ctx, const void* d_line, int32_t format, int32_t magnitude, const uint32_t* shortened,
                                int32_t where, size_t n_codewords, uint32_t* d_payload, uint32_t* d_bits, lnsfaid_line_stats* d_stats,
                                uint32_t* d_short_ones);
int lnsfaid_encode_burst(lnsfaid_ctx* ctx, const uint32_t* payload, const uint32_t* shortened, int32_t where, size_t n_codewords,
                         uint32_t* line, uint32_t* bits);
int lnsfaid_encode_burst_device(lnsfaid_ctx* ctx, const uint32_t* d_payload, const uint32_t* shortened, int32_t where, size_t n_codewords,
                                uint32_t* d_line, uint32_t* d_bits);
int lnsfaid_encode_burst_host(const lnsfaid_code* code, const uint8_t* circ, size_t circ_bytes, const uint32_t* payload,
                              const uint32_t* shortened, int32_t where, size_t n_codewords, uint32_t* line, uint32_t* bits);
int lnsfaid_burst_to_llr4(const lnsfaid_code* code, const void* line, int32_t format, int32_t magnitude, const uint32_t* shortened,
                          int32_t where, size_t n_codewords, uint8_t* llr4);
int lnsfaid_burst_words(const lnsfaid_code* code, const uint32_t* shortened, size_t n_codewords, uint64_t* line_bits,
                        uint64_t* payload_bits);

/* ---- burst-format link ------------------------------------------------------------------------------------
 * The four link calls - payload source, BSC, soft channel, counters - on the burst formats above, so that
 * lnsfaid_burst_payload_random_device -> lnsfaid_encode_burst_device -> channel -> lnsfaid_decode_burst_device ->
 * lnsfaid_burst_count_errors_device runs on the device and only counters leave it: the frame error rate of a burst whose last
 * codeword is shortened by S, at a given input BER or Eb/N0.  `shortened` (a host pointer in every form, NULL = all zero,
 * S_c % 32 == 0, 0 <= S_c <= K - 32) and `where` follow the rules of the burst-format section; N, K, L as there.
 *
 * One definition: draws are indexed by MOTHER position.  The generator is the link's, unchanged: mix64, cwkey(key, C, d),
 * draw(key, C, d, q), d = 1 payload, 2 BSC, 3 soft; C = first_codeword + i, wrapping.  A burst codeword C with known range
 * [k0, k0 + S_c) uses, for the mother position k of each transmitted position, exactly the draw the line call uses for position k of
 * codeword C: draw q = k / 2, the low half for even k and the high half for odd k.  S_c is a multiple of 32, so a line word is always
 * 16 whole draws: with k0w = k0 / 32 and Sw = S_c / 32, word wl of the burst codeword is mother word wi = wl + (wl >= k0w ? Sw : 0), and
 * mother word wi outside the known words is burst word wl = wi - (wi >= k0w + Sw ? Sw : 0).  Exact consequences:
 *   1. Expand, run, drop.  Expand the burst line with anything in the known range, run lnsfaid_line_bsc_* / lnsfaid_line_soft_*, drop
 *      the known words: the burst channel gives the same bytes.  flips counts transmitted positions only, never the known range: it is
 *      the line call's flips minus what that call counted inside the known words.
 *   2. Payload.  The burst payload of codeword C is lnsfaid_line_payload_random_host's payload of C with the known words dropped.
 *   3. No shortening.  With shortened == NULL or all zero every output, counter and total is byte for byte that of the corresponding
 *      lnsfaid_line_* call.
 *   4. Split invariance.  A run cut into calls of any size gives the bytes of the one-shot run: first_codeword is advanced and
 *      `shortened` sliced accordingly; burst offsets restart per call, and concatenation restores the stream.  The same holds for a
 *      run dealt to ranks.
 *   5. Common random numbers.  A sweep over S on one key sees the same noise on every position that survives.
 * The error-propagation channel has no burst form: its chain has to decide what it does across the gap.
 *
 * Formats.  payload and sent are burst payloads ((K - S_c) / 32 words per codeword, back to back; sent == NULL is the all-zero
 * payload).  Lines are burst lines: (L - S_c) / 32 words (LNSFAID_LINE_HARD), (L - S_c) / 2 bytes (LNSFAID_LINE_LLR4).  Input word u of
 * the soft channel, counted over the whole burst line, is output bytes 16 u .. 16 u + 15, as on a line.
 *   lnsfaid_burst_bsc_*   LNSFAID_LINE_HARD burst lines in and out; line_out == line_in is allowed (in place), any other overlap is
 *                         undefined.  threshold as lnsfaid_line_bsc_*: 0 copies.
 *   lnsfaid_burst_soft_*  a HARD burst line in, an LLR4 burst line out; table, levels and the rule of flips as lnsfaid_line_soft_*; the
 *                         two byte ranges must not overlap.
 *   flips, total_flips    as in the line calls: optional uint32_t [n_codewords] (the _device forms: a device pointer) and an optional
 *                         host uint64_t that is ADDED to.  The pre-FEC BER of a run is total_flips over the line_bits of
 *                         lnsfaid_burst_words.
 * Counters.  errors, fec and vs_sent are the words of lnsfaid_line_count_errors_* with one change, stated by the burst-format
 * section itself: a receiver treats short_ones > 0 like unsatisfied > 0.  With w = the bits of a codeword's burst payload that differ
 * from sent and failed = unsatisfied > 0 || short_ones > 0:  fec[1] counts failed codewords, fec[2] those with !failed and
 * corrected > 0, fec[3] sums corrected over the codewords that are not failed, vs_sent[2] counts w > 0 && !failed, vs_sent[3]
 * w == 0 && failed; every other word is unchanged.  stats and short_ones are what lnsfaid_decode_burst* returned (the _device form:
 * device pointers); short_ones == NULL means zeros; fec or vs_sent with stats == NULL is LNSFAID_E_INVAL.  Each set is ADDED to and
 * is four words, so lnsfaid_allreduce_counters sums it unchanged.  The counters need no `where`: a burst payload is walked by its
 * lengths alone.  The denominators of a BER come from lnsfaid_burst_words.
 * Rules: those of the link section plus the burst-format section.  n_codewords 0 is a no-op, up to 32 * max_groups (device forms);
 * device pointers, optional ones included, 4-byte aligned; a bad `shortened` entry or a bad `where` is LNSFAID_E_INVAL, as are a NULL
 * context or code, a NULL required buffer, a table that decreases, and overlapping ranges of the soft channel.  A refused call writes
 * nothing and adds nothing.  The device forms queue on the context's stream and return when their host outputs are complete; their
 * accumulators are the link's, their descriptors the burst calls'.  They do not depend on the decoder configuration.  On the GPU only
 * the built-in code's circulant size is served, as for the burst calls.  The host forms need no context and no GPU, take pointers of
 * any alignment, have no limit on n_codewords, and are the definition of what the device forms return. */
int lnsfaid_burst_payload_random_device(lnsfaid_ctx* ctx, uint64_t key, uint64_t first_codeword, const uint32_t* shortened, int32_t where,
                                        size_t n_codewords, uint32_t* d_payload);
int lnsfaid_burst_payload_random_host(const lnsfaid_code* code, uint64_t key, uint64_t first_codeword, const uint32_t* shortened,
                                      int32_t where, size_t n_codewords, uint32_t* payload);
int lnsfaid_burst_bsc_device(lnsfaid_ctx* ctx, const uint32_t* d_line_in, const uint32_t* shortened, int32_t where, size_t n_codewords,
                             uint64_t key, uint64_t first_codeword, uint32_t threshold, uint32_t* d_line_out, uint32_t* d_flips,
                             uint64_t* total_flips);
int lnsfaid_burst_bsc_host(const lnsfaid_code* code, const uint32_t* line_in, const uint32_t* shortened, int32_t where, size_t n_codewords,
                           uint64_t key, uint64_t first_codeword, uint32_t threshold, uint32_t* line_out, uint32_t* flips,
                           uint64_t* total_flips);
int lnsfaid_burst_soft_device(lnsfaid_ctx* ctx, const uint32_t* d_line_in, const uint32_t* shortened, int32_t where, size_t n_codewords,
                              uint64_t key, uint64_t first_codeword, const uint32_t table[14], uint8_t* d_llr4_out, uint32_t* d_flips,
                              uint64_t* total_flips);
int lnsfaid_burst_soft_host(const lnsfaid_code* code, const uint32_t* line_in, const uint32_t* shortened, int32_t where, size_t n_codewords,
                            uint64_t key, uint64_t first_codeword, const uint32_t table[14], uint8_t* llr4_out, uint32_t* flips,
                            uint64_t* total_flips);
int lnsfaid_burst_count_errors_device(lnsfaid_ctx* ctx, const uint32_t* d_payload, const uint32_t* d_sent, const lnsfaid_line_stats* d_stats,
                                      const uint32_t* d_short_ones, const uint32_t* shortened, size_t n_codewords, uint64_t errors[4],
                                      uint64_t fec[4], uint64_t vs_sent[4]);
int lnsfaid_burst_count_errors_host(const lnsfaid_code* code, const uint32_t* payload, const uint32_t* sent, const lnsfaid_line_stats* stats,
                                    const uint32_t* short_ones, const uint32_t* shortened, size_t n_codewords, uint64_t errors[4],
                                    uint64_t fec[4], uint64_t vs_sent[4]);

/* ---- line-format failure capture ---------------------------------------------------------------------------
 * The codewords of a line call that fail, as ordered, compact records: what the decoder did with them.  (key, global codeword number)
 * reproduces payload, codeword and every channel draw on the host (the link's generators are counter-based); the records hold what
 * cannot be reproduced cheaply - the decisions, the error pattern and the set of unsatisfied checks.  N = n_var, K = n_var - n_check,
 * L = n_var - puncture_tail, all multiples of 32 as for the line calls.
 *   line, format  exactly the input of lnsfaid_decode_line*.  line may be NULL: the line section of every record is then zero and
 *            channel_errors is 0.
 *   bits     the optional `bits` output of lnsfaid_decode_line*, N / 32 words per codeword; REQUIRED here.  The decisions may come
 *            from anywhere, as for the FEC status calls.
 *   sent     the optional `bits` output of lnsfaid_encode_line*: the mother codeword, N / 32 words per codeword.  NULL means "no sent
 *            word is known" - a receiver's situation - and NOT the all-zero codeword of the counter calls: select must then not
 *            contain LNSFAID_LINE_CAPTURE_WRONG (LNSFAID_E_INVAL), and the error section and the three sent-derived counts are zero.
 *            A simulator that sends zeros passes a zeroed buffer.
 *   select   1 .. 3 (else LNSFAID_E_INVAL): codeword i is a failure when select & flags != 0.  UNCORRECTABLE: the syndrome of bits,
 *            recomputed here over all N bits (punctured tail included), is non-zero - the number lnsfaid_line_stats::unsatisfied
 *            gives for decisions of the line decode.  WRONG: wrong_payload > 0.
 *   order    failures are numbered 0, 1, ... in ascending index.  A call stores failures skip .. skip + capacity - 1; *found is the
 *            number of failures in the whole call, *stored = min(capacity, max(found - skip, 0)).  capacity 0 counts only.  Every
 *            output is a pure function of the inputs, and paging with skip concatenates to the one-shot result.
 *   payload  payload + i * W holds record i, W = lnsfaid_line_capture_words: 32-bit words, four sections back to back -
 *              line      L / 32 words (HARD) or L / 8 words (LLR4): the codeword's line image, verbatim
 *              bits      N / 32 words: the decisions
 *              error     N / 32 words: bits XOR sent
 *              syndrome  n_check / 32 words: bit b of word w is set when row 32 w + b of pos_vn (the code table's own row order)
 *                        is unsatisfied
 *            50G-PON: W = 1 740 (HARD) or 3 360 (LLR4).
 * Rules: the line link's.  n_codewords 0 is a no-op that sets *found and *stored to 0.  LNSFAID_E_INVAL: a NULL context or code; a
 * format other than the two; N, K or L not a multiple of 32; more than 32 * max_groups codewords (device form); a NULL bits, found
 * or stored; NULL records or payload with capacity > 0; a device pointer (line, bits, sent) that is not 4-byte aligned (more
 * alignment only widens the loads).  A refused call touches no output.  Exactly *stored records and *stored * W payload words are
 * written.  records, payload, found and stored are host pointers in both forms.
 * The device form is a pure read of its inputs; it queues on the context's stream, stages through context buffers of
 * min(capacity, n_codewords) slots (allocated at first use, grown on demand, freed by lnsfaid_destroy) and copies back only what
 * it stored.  It does not depend on the decoder configuration.  On the GPU only the built-in code's circulant size is served.
 * The host form needs no context and no GPU, reads pos_vn, deg and deg_rows row by row - so it serves any code the struct
 * describes - takes pointers of any alignment and has no limit on n_codewords: it is the definition. */
#define LNSFAID_LINE_CAPTURE_UNCORRECTABLE 1 /* the decisions leave at least one row of H unsatisfied              */
#define LNSFAID_LINE_CAPTURE_WRONG         2 /* an information bit differs from the sent word (needs sent)         */
typedef struct lnsfaid_line_failure {
    uint64_t codeword;       /* first_codeword + index (wraps): with the key of the run it reproduces payload and channel draws */
    uint32_t index;          /* index in the call                                                                   */
    uint32_t flags;          /* LNSFAID_LINE_CAPTURE_* bits that hold for this codeword (both are evaluated whatever select is;
                                WRONG only when sent is given)                                                      */
    uint32_t unsatisfied;    /* rows of H the decisions leave unsatisfied = popcount of the syndrome section        */
    uint32_t wrong_payload;  /* positions k < K where bits differ from sent (0 without sent)                        */
    uint32_t wrong_parity;   /* positions K <= k < N, punctured tail included (0 without sent)                      */
    uint32_t channel_errors; /* positions k < L where the channel's own decision (line bit; nibble > 0) differs from sent (0 without sent) */
} lnsfaid_line_failure;      /* 32 bytes */
int lnsfaid_line_capture_words(const lnsfaid_code* code, int32_t format, uint32_t* words_per_record);
int lnsfaid_line_capture_device(lnsfaid_ctx* ctx, const void* d_line, int32_t format, const uint32_t* d_bits, const uint32_t* d_sent,
                                size_t n_codewords, uint64_t first_codeword, int32_t select, size_t skip, size_t capacity,
                                lnsfaid_line_failure* records, uint32_t* payload, uint64_t* found, uint64_t* stored);
int lnsfaid_line_capture_host(const lnsfaid_code* code, const void* line, int32_t format, const uint32_t* bits, const uint32_t* sent,
                              size_t n_codewords, uint64_t first_codeword, int32_t select, size_t skip, size_t capacity,
                              lnsfaid_line_failure* records, uint32_t* payload, uint64_t* found, uint64_t* stored);

/* ---- line-format error-propagation channel ------------------------------------------------------------------
 * A hard channel with memory in the line's own format, LNSFAID_LINE_HARD in and out: a wrong decision raises the error probability of
 * the next one, as behind a decision-feedback equaliser, so the same average BER arrives in runs.  Everything downstream takes its
 * output unchanged: lnsfaid_decode_line*, lnsfaid_line_count_errors* and lnsfaid_line_capture*, whose channel_errors already counts
 * line against sent.  L, K, mix64, cwkey and draw are those of the link section above; the host form is the definition.
 *
 * Draws: the BSC's domain, d = 2, on purpose.  Position 2 q of codeword C uses u = the low 32 bits of draw(key, C, 2, q), position
 * 2 q + 1 the high 32 bits, for q < L / 2; one more draw, which the BSC never makes, gives the start: s = the low 32 bits of
 * draw(key, C, 2, L / 2).
 * t: three thresholds { t_idle, t_after, t_start }, a host pointer in both forms (as `table` is for lnsfaid_line_soft_device).  The rule
 * is t_idle <= t_after (positive correlation only).
 * Chain, one per codeword - nothing carries from a codeword to the next:
 *   e[-1] = (s < t_start),   e[k] = (u[k] < (e[k - 1] ? t_after : t_idle)) for k = 0 .. L - 1,   position k is inverted iff e[k] = 1.
 * With g[k] = (u[k] < t_idle) and p[k] = (u[k] < t_after) this is e[k] = g[k] | (p[k] & e[k - 1]), and because g implies p it is the
 * carry chain of an adder: generate, propagate, kill.
 *   line_out == line_in is allowed (in place); any other overlap of the two is undefined.
 *   flips        optional uint32_t [n_codewords] (the _device form: a device pointer): the positions inverted per codeword.
 *   total_flips  optional host uint64_t, ADDED to: the positions inverted in the call.
 *   runs         optional uint32_t [n_codewords] (the _device form: a device pointer): per codeword, the maximal runs of consecutive
 *                inverted positions inside the codeword.  A run that starts at position 0 because e[-1] = 1 is one run.
 *   total_runs   optional host uint64_t, ADDED to: the runs of the call.  total_flips / total_runs is the measured mean run length.
 * Consequences, all exact:
 *   1. With t_idle == t_after the output, flips and total_flips are byte for byte those of lnsfaid_line_bsc_* with that threshold,
 *      whatever t_start is: a sweep with and without memory on one key uses common random numbers.
 *   2. With { 0, 0xFFFFFFFF, t_start } a codeword is either returned untouched (s >= t_start) or inverted from position 0 on
 *      (s < t_start), entirely unless some u[k] equals 0xFFFFFFFF.
 *   3. { 0, 0, anything } copies the line.
 * lnsfaid_line_markov_thresholds (host only): the thresholds of a stationary chain with marginal error probability p = ber and
 * a = propagation = P(e[k] = 1 | e[k - 1] = 1), hence a mean run length of 1 / (1 - a):  t_after = floor(a * 2^32),
 * t_start = floor(p * 2^32), t_idle = floor(2^32 * p * (1 - a) / (1 - p)), evaluated in double in that order (and never above t_after);
 * when a == p all three are floor(p * 2^32), the BSC of consequence 1.  With q = p (1 - a) / (1 - p) the stationary probability
 * q / (1 - a + q) is p, so P(e[k] = 1) = p at every position and ber stays the x-axis of a sweep.  It requires 0 <= p <= a < 1, which
 * is exactly t_idle <= t_after; anything else, NaN, or a NULL t is LNSFAID_E_INVAL with t not written.
 * Rules: the BSC's.  n_codewords 0 is a no-op (every buffer may be NULL).  LNSFAID_E_INVAL: a NULL context or code; L or K not a
 * multiple of 32; more than 32 * max_groups codewords (device form); a NULL line_in, line_out or t; t_idle > t_after; a device pointer,
 * optional ones included, that is not 4-byte aligned.  A refused call writes nothing and adds nothing.  The device form queues on the
 * context's stream and returns when the totals are complete; its two accumulators live with the link's, allocated at first use and
 * freed by lnsfaid_destroy.  It does not depend on the decoder configuration.  The host form needs no context and no GPU, takes
 * pointers of any alignment and has no limit on n_codewords. */
int lnsfaid_line_markov_thresholds(double ber, double propagation, uint32_t t[3]);
int lnsfaid_line_markov_device(lnsfaid_ctx* ctx, const uint32_t* d_line_in, size_t n_codewords, uint64_t key, uint64_t first_codeword,
                               const uint32_t t[3], uint32_t* d_line_out, uint32_t* d_flips, uint32_t* d_runs,
                               uint64_t* total_flips, uint64_t* total_runs);
int lnsfaid_line_markov_host(const lnsfaid_code* code, const uint32_t* line_in, size_t n_codewords, uint64_t key, uint64_t first_codeword,
                             const uint32_t t[3], uint32_t* line_out, uint32_t* flips, uint32_t* runs,
                             uint64_t* total_flips, uint64_t* total_runs);

/* ---- front-end on the device (optional, the host generator stays the parity source) ---- */

/*
 * Generates the fixInput of n_streams groups on the GPU, one group per reference worker thread ("stream"):
 * replaces, for one pass of the loop body of CSimulate::Run (CSimulate.cpp:126-132),
 *   CChannel::AWGNChannel (CChannel.cpp:71-97, Wichmann-Hill + Box-Muller, seed table CSimulate.cpp:11-17),
 *   CModulate::Demodulation + AfterDeModulationDeInterleaver (CModulate.cpp:152-212, :273-293) and
 *   CLDPC::float2LimitChar_4bit (CLDPC.cpp:4553-4573).
 *   seeds[s]        RandomSeed of stream s (IX = IY = IZ = seed, CChannel.cpp:121)
 *   draws_before[s] uniforms stream s has consumed so far; one group consumes lnsfaid_frontend_draws_per_group()
 *   mod_type        Profile.txt modType: 2 (QPSK), 4, 6, 8 (16-, 64-, 256-QAM); InterleaveModType: lnsfaid_frontend_set_interleave
 *   sigma           CSimulate::Configure's sigma (CSimulate.cpp:69-74); the channel adds N(0, (sigma/sqrt 2)^2) per axis
 *   codeword        host, [n_var] bits 0/1 sent in every frame (FakeEncoder), NULL = all-zero
 *   d_fixInput      device, n_streams groups in the decoder's layout
 * Integer and float stages are bit-exact; Box-Muller uses the device's double log / cos (directly, or as the arbiter of the
 * single-precision fast path, see lnsfaid_frontend_set_exact), so single LLRs can differ from the host generator's (rate
 * bounded in tests/test_gpu_frontend.py).
 */
int lnsfaid_frontend_device(lnsfaid_ctx* ctx, const uint32_t* seeds, const uint64_t* draws_before, size_t n_streams,
                            int32_t mod_type, float sigma, float scale, const int8_t* codeword, int8_t* d_fixInput);
/* Same with an explicit generator state per stream: states[3 s .. 3 s + 2] = RS.IX, RS.IY, RS.IZ of stream s at
 * draws_before[s] = 0, e.g. a row of the lastSeed table the driver writes to Temp.txt (main.cpp:200-207), which the
 * reference compiles back in under CONTINUE_SEED (CChannel.cpp:4-41, :116-119). */
int lnsfaid_frontend_device_states(lnsfaid_ctx* ctx, const uint32_t* states, const uint64_t* draws_before, size_t n_streams,
                                   int32_t mod_type, float sigma, float scale, const int8_t* codeword, int8_t* d_fixInput);
uint64_t lnsfaid_frontend_draws_per_group(const lnsfaid_ctx* ctx, int32_t mod_type);

/* The front-end kernel takes a quantised LLR from a single-precision evaluation of Box-Muller whenever no quantiser threshold
 * lies within that evaluation's error bound, and recomputes the symbol in double precision otherwise (a few in ten thousand):
 * same output, about a quarter of the time.  lnsfaid_frontend_set_exact(ctx, 1) (or LNSFAID_FRONTEND_EXACT=1 at creation)
 * sends every symbol through the double-precision chain, written with the reference's own integer generator and float
 * divisions - the A/B reference of the tests.
 * lnsfaid_frontend_fastpath_bounds scans EVERY float u in [0, 1) on the device: measured[0] = max |sqrt(-2 ln(1 - u)) - fast|,
 * measured[1] = max |cos(2 pi u) - fast|; assumed[] = what the kernel's bound uses.  measured must stay below assumed (the GPU
 * test asserts a factor of two): run it once on a device whose transcendental units are not those of gfx950. */
int lnsfaid_frontend_set_exact(lnsfaid_ctx* ctx, int32_t exact);
int lnsfaid_frontend_fastpath_bounds(lnsfaid_ctx* ctx, double measured[2], double assumed[2]);

/* Profile.txt InterleaveModType for lnsfaid_frontend_device: the block interleaver of BeforeModulationInterleaver /
 * AfterDeModulationDeInterleaver (CModulate.cpp:95-212) inside every frame; 1 (the default and the shipped value) is the
 * identity.  Must divide n_var.  The value also applies to lnsfaid_demap_device / lnsfaid_demap_packed_device. */
int lnsfaid_frontend_set_interleave(lnsfaid_ctx* ctx, int32_t interleave_mod_type);

/* Frames for lnsfaid_frontend_device when every stream sends its own 32 frames (the reference with a real encoder:
 * GenMsgSeq + Encode once per 50 calls, CSimulate.cpp:106-116) instead of one codeword in every frame.
 *   outputBits  host, n_streams groups in CLDPC::Encode's output layout ([32][K] then [32][M] per group)
 *   inputBits   host, their information bits [n_streams][32][K] (what CalculateErrors compares with)
 * Both are copied to the device and used by every following lnsfaid_frontend_device call that passes codeword = NULL and
 * at most n_streams streams; outputBits = NULL switches back.  lnsfaid_frontend_input_bits returns the device copy of
 * inputBits for lnsfaid_count_errors_device (NULL while no frames are set). */
int lnsfaid_frontend_set_frames(lnsfaid_ctx* ctx, const int8_t* outputBits, const int8_t* inputBits, size_t n_streams);
int lnsfaid_frontend_input_bits(lnsfaid_ctx* ctx, const int8_t** d_inputBits);

/* ---- demapper for received symbols --------------------------------------------------------------------
 * Replaces, for n_groups groups of caller-supplied symbols, CModulate::Demodulation (CModulate.cpp:270-362),
 * AfterDeModulationDeInterleaver (:156-212) and CLDPC::float2LimitChar_4bit (CLDPC.cpp:4553-4573): the receive chain of
 * CSimulate.cpp:127-129 behind a channel of the caller's own (a capture, a channel model on the same GPU).
 *   rx    mod_type 2 / 4 / 6 / 8: the reference's MKL_Complex8 SymbolSeq of each group.  A symbol is a pair (re, im) of floats, a
 *         group has 32 * n_var / mod_type symbols, symbol s of group g starts at float index 2 * (g * 32 * n_var / mod_type + s)
 *         and carries stream positions mod_type * s .. mod_type * s + mod_type - 1.
 *         mod_type 1 (the reference's BPSK branch, CSimulate.cpp:121-124): one real float per code bit, frame-major - frame m,
 *         bit k of group g at g * 32 * n_var + m * n_var + k; the interleaver is not applied (as in that branch).  Positive
 *         means bit 1, as for every other order.  This is also the way in for LLRs computed elsewhere.
 *   levels   l0 = re, l1 = im; for n = 1 .. mod_type / 2 - 1:  l[2n]   = (float)(fabs((double)l[2n-2]) - c[n-1]),
 *                                                              l[2n+1] = (float)(fabs((double)l[2n-1]) - c[n-1]),
 *         c = {0.6324555} (16-QAM), {0.6172134, 0.3086067} (64-QAM), {0.613568, 0.306784, 0.153392} (256-QAM); every level
 *         is stored as float before it feeds the next.  Level u of symbol s is the LLR of stream position mod_type * s + u.
 *   de-interleaver   stream position pos belongs to frame m = pos / n_var, in-frame position p = pos % n_var, and carries code
 *         bit k = (n_var / I) * (p % I) + p / I, I = InterleaveModType (the device calls use the context's value,
 *         lnsfaid_frontend_set_interleave; the host calls take it as an argument).
 *   quantiser   y = l * scale (one float multiply), q = (int)y truncated toward zero and clamped to [-7, 7]; when
 *         !(y > -2^31 && y < 2^31) - NaN, +Inf, -Inf and every |y| >= 2^31, positive ones included - the conversion yields
 *         the integer indefinite, which ends at -7.
 *   output   the group's element m * K + k for k < K, else 32 * K + m * M + (k - K) (K = n_var - n_check, M = n_check): the
 *         fixInput order of lnsfaid_decode.  d_fixInput / fixInput: one int8 per element, group g at byte g * 32 * n_var.
 *         d_llr4 / llr4: the llr4 format of the packed decode I/O above (element e in byte e / 2, low nibble for even e, group g
 *         at byte 16 * g * n_var).
 * Rules: mod_type in {1, 2, 4, 6, 8}; I >= 1 dividing n_var; (32 * n_var) % mod_type == 0 (the rule of
 * lnsfaid_frontend_device, so everything it can produce these calls can consume); the packed forms also need n_var and K
 * even; a NULL buffer with n_groups > 0; the device calls: n_groups > max_groups, d_rx or d_llr4 not 4-byte aligned -
 * LNSFAID_E_INVAL.  n_groups 0 is a no-op (NULL buffers allowed).  d_fixInput may have any alignment.  Alignment beyond that
 * only selects the width of the loads and stores, never the bytes written.  The calls write exactly n_groups * 32 * n_var bytes
 * (half of that for the packed forms) and nothing outside.
 * The device calls queue on the context's stream and return when the output is complete (as lnsfaid_encode_device): a
 * following lnsfaid_decode*_device needs no synchronisation by the caller. */
int lnsfaid_demap_device(lnsfaid_ctx* ctx, const float* d_rx, size_t n_groups, int32_t mod_type, float scale, int8_t* d_fixInput);
int lnsfaid_demap_packed_device(lnsfaid_ctx* ctx, const float* d_rx, size_t n_groups, int32_t mod_type, float scale, uint8_t* d_llr4);
/* Host only, no context, no GPU (like lnsfaid_pack_llr4): the same bytes, for callers whose samples are in host memory -
 * quantise there and ship 4 bits per LLR through lnsfaid_decode_packed instead of 32. */
int lnsfaid_demap_host(int32_t n_var, int32_t n_check, int32_t interleave_mod_type, const float* rx, size_t n_groups,
                       int32_t mod_type, float scale, int8_t* fixInput);
int lnsfaid_demap_packed_host(int32_t n_var, int32_t n_check, int32_t interleave_mod_type, const float* rx, size_t n_groups,
                              int32_t mod_type, float scale, uint8_t* llr4);

/* ---- pre-FEC error counters ---------------------------------------------------------------------------
 * The counterpart of lnsfaid_count_errors on the input side of the decoder: hard decisions on the demapper's levels against
 * the sent bits.  Replaces CModulate::ModCalErr (CModulate.cpp:382-437) and feeds the ModBER / ModSER / ModFER columns of
 * demod.txt (reference main.cpp:183-185).  One definition for every entry point:
 *   levels    for a group of 32 frames and mod_type in {1, 2, 4, 6, 8} exactly the levels of the demapper section above: level
 *             u of symbol s is the LLR of stream position pos = mod_type * s + u, every level stored as float before it feeds
 *             the next; mod_type 1: one float per code bit, frame-major, no interleaver.
 *   code bit  frame m = pos / n_var, p = pos % n_var, k = (n_var / I) * (p % I) + p / I, I = InterleaveModType (mod_type 1: k = p).
 *   decision  d = level > 0 ? 1 : 0 (ModCalErr's `demodseq > 0`): +0.0, -0.0 and NaN decide 0, +Inf decides 1.  The quantiser's
 *             scale plays no part.
 *   sent bit  sent[g][m * K + k] for k < K, else sent[g][32 * K + m * M + (k - K)]: the layout of CLDPC::outputBits, of
 *             lnsfaid_encode* and of lnsfaid_frontend_set_frames (group g at byte g * 32 * n_var).  sent == NULL means the
 *             all-zero codeword.  A bit is wrong when d differs from the sent byte.
 *   scope     LNSFAID_PREFEC_INFO: only positions with k < K take part (ModCalErr's range, the denominators of demod.txt);
 *             LNSFAID_PREFEC_CODEWORD: all n_var positions take part, the punctured tail included (the simulated channel
 *             transmits it).
 *   counters  out[4], ADDED to like lnsfaid_count_errors:
 *             out[0] TestFrame       += 32 per group
 *             out[1] ModErrorFrame   frames with at least one wrong in-scope bit
 *             out[2] ModErrorBits    wrong in-scope bits
 *             out[3] ModErrorSymbol  channel symbols with at least one wrong in-scope bit (mod_type 1: equals ModErrorBits)
 *             Four words on purpose: lnsfaid_allreduce_counters sums them across ranks unchanged.
 * Rules: those of the demapper, plus n_var % mod_type == 0 (no symbol straddles two frames) and scope 1 or 2 - LNSFAID_E_INVAL
 * otherwise; a NULL rx or out with n_groups > 0 too.  n_groups 0 is a no-op (NULL buffers allowed).
 * Deviations from ModCalErr, both on purpose: the sent bit is indexed correctly for every frame (the reference's index is
 * right for frame 0 only, and its call is commented out, CSimulate.cpp:129); and a symbol is the channel's symbol, not mod_type
 * consecutive code bits - the two coincide when I = 1 and mod_type divides K. */
#define LNSFAID_PREFEC_INFO 1
#define LNSFAID_PREFEC_CODEWORD 2
/* Host only, no context, no GPU (like lnsfaid_demap_host): the reference the device paths are tested against. */
int lnsfaid_prefec_errors_host(int32_t n_var, int32_t n_check, int32_t interleave_mod_type, const float* rx, size_t n_groups,
                               int32_t mod_type, const int8_t* sent, int32_t scope, uint64_t out[4]);
/* Device-resident symbols and sent bits, the context's InterleaveModType (lnsfaid_frontend_set_interleave).  d_rx: the format and
 * the rules of lnsfaid_demap_device (4-byte aligned, n_groups <= max_groups); d_sent may have any alignment.  More alignment only
 * widens the loads, it never changes a count.  A pure read.  Queues on the context's stream and returns when out is complete;
 * no synchronisation by the caller is needed after a preceding *_device call. */
int lnsfaid_prefec_errors_device(lnsfaid_ctx* ctx, const float* d_rx, size_t n_groups, int32_t mod_type, const int8_t* d_sent,
                                 int32_t scope, uint64_t out[4]);
/* Counting inside the device front-end, which never stores a level.  scope 0 = off (the default), LNSFAID_PREFEC_INFO /
 * LNSFAID_PREFEC_CODEWORD = every later lnsfaid_frontend_device / _states call counts its own decisions against the bits it
 * sent (codeword, set_frames, random_frames or all-zero) into an accumulator on the device; TestFrame advances by 32 per stream
 * per call.  The fixInput bytes are those of a call without counting, and the counters do not depend on
 * lnsfaid_frontend_set_exact (with counting on, the fast path also sends a symbol to the double-precision chain when a level's
 * sign is not certain).  While a scope is set, front-end calls with n_var % mod_type != 0 return LNSFAID_E_INVAL.
 * lnsfaid_frontend_set_prefec clears the accumulator.  lnsfaid_frontend_prefec_counters synchronises the context's stream, ADDS
 * the accumulator to out and, with reset != 0, clears it; it is the only call that reads the accumulator back. */
int lnsfaid_frontend_set_prefec(lnsfaid_ctx* ctx, int32_t scope);
int lnsfaid_frontend_prefec_counters(lnsfaid_ctx* ctx, uint64_t out[4], int32_t reset);

/* ---- error-frame capture -------------------------------------------------------------------------------
 * The collect-flag branch of CLDPC::CalculateErrors (CLDPC.cpp:4877-4983) for buffers that stay on the device: the frames with
 * wrong information bits come back as ordered, compact records, nothing else leaves the device.  One definition for both entry
 * points:
 *   fixInput     the decoder's input, the layout of lnsfaid_decode ([32][K] then [32][M] per group, group g at byte
 *                g * 32 * n_var).  NULL is allowed: the LLR section of every payload is then zero.
 *   decodedBits  the decoder's output, the layout of lnsfaid_decode ([32][n_var] per group).
 *   sent         the sent frames in the layout of CLDPC::outputBits, of lnsfaid_encode* and of the `sent` of the pre-FEC counters:
 *                [32][K] then [32][M] per group, group g at byte g * 32 * n_var.  NULL means the all-zero codeword.
 *   error frame  a decision is wrong when its byte differs from the sent byte (the rule of lnsfaid_count_errors).  Frame m of group
 *                g - codeword 32 * g + m of the batch - is an error frame when at least one of its K information decisions is wrong
 *                (the reference's condition); wrong parity decisions alone do not make one.
 *   order        the error frames of the batch are numbered 0, 1, ... in ascending codeword index.  A call stores error frames
 *                skip .. skip + capacity - 1 of that numbering, in that order.  *found = the error frames of the whole batch,
 *                whatever skip and capacity are; *stored = min(capacity, max(found - skip, 0)).  The outputs are a pure function
 *                of the inputs: nothing depends on the order in which the device happened to run its workgroups.  A caller pages
 *                through a batch by calling again with skip advanced by *stored until skip reaches *found.
 *   records[i]   the i-th stored error frame.
 *   payload      payload + i * 3 * n_var holds three sections of n_var bytes, each in code-bit order k = 0 .. n_var - 1:
 *                [0, n_var)           the frame's LLRs: fixInput[g][m * K + k] for k < K, else fixInput[g][32 * K + m * M + (k - K)]
 *                [n_var, 2 n_var)     decodedBits[g][m * n_var + k]
 *                [2 n_var, 3 n_var)   the sent bits, indexed like the LLRs
 *                Exactly *stored records and *stored * 3 * n_var payload bytes are written and nothing outside them.
 *   out          may be NULL.  Otherwise the call ADDS exactly what lnsfaid_count_errors* adds for the same decodedBits and the
 *                information part of sent (TestFrame, ErrorFrame, ErrorBits, LT3ErrBitFrame): a caller that captures needs no
 *                separate counter pass, and *found equals the ErrorFrame it added.
 * Rules: n_groups == 0 is a no-op that sets *found = *stored = 0 (every buffer may be NULL); capacity == 0 counts only (records
 * and payload may be NULL).  LNSFAID_E_INVAL, with no output touched: a NULL ctx (device call) or a code shape outside
 * 0 < n_check < n_var (host call); with n_groups > 0 a NULL decodedBits, found or stored, and with capacity > 0 too a NULL records
 * or payload; n_groups > max_groups (device call). */
typedef struct lnsfaid_error_record {
    uint32_t codeword;      /* index in the batch: 32 * group + frame */
    uint32_t info_errors;   /* wrong information bits, always > 0 */
    uint32_t parity_errors; /* wrong parity bits */
    uint32_t reserved;      /* 0 */
} lnsfaid_error_record;
/* The three inputs are device pointers of any alignment (more alignment only widens the loads, it never changes a byte); records,
 * payload, found, stored and out are host pointers - records are rare and end in files.  The call stages through device buffers of
 * the context with min(capacity, 32 * n_groups) slots (allocated at the first call, grown on demand, freed by lnsfaid_destroy) and
 * copies back only the stored records.  A pure read of its inputs.  Queues on the context's stream and returns when the outputs
 * are complete; no synchronisation by the caller is needed after a preceding *_device call. */
int lnsfaid_capture_errors_device(lnsfaid_ctx* ctx, const int8_t* d_fixInput, const int8_t* d_decodedBits,
                                  const int8_t* d_sent, size_t n_groups, size_t skip, size_t capacity,
                                  lnsfaid_error_record* records, int8_t* payload,
                                  uint64_t* found, uint64_t* stored, uint64_t out[4]);
/* Host only, no context, no GPU (like lnsfaid_prefec_errors_host): the reference the device path is tested against. */
int lnsfaid_capture_errors_host(int32_t n_var, int32_t n_check, const int8_t* fixInput, const int8_t* decodedBits,
                                const int8_t* sent, size_t n_groups, size_t skip, size_t capacity,
                                lnsfaid_error_record* records, int8_t* payload,
                                uint64_t* found, uint64_t* stored, uint64_t out[4]);
/* The device copy of the frames lnsfaid_frontend_set_frames / lnsfaid_frontend_random_frames left for the device front-end (the
 * `sent` of the calls above and of lnsfaid_prefec_errors_device), beside lnsfaid_frontend_input_bits; NULL while no frames are
 * set (the front-end then sends its codeword argument, or the all-zero codeword).  The pointer holds the frames of the n_streams
 * streams they were set for, and lnsfaid_frontend_device sends them only in calls with codeword == NULL and at most that many
 * streams: it is the `sent` of such a call's output, for at most n_streams groups.  A front-end call with more streams, or with a
 * codeword, sent that codeword (NULL: all-zero) in every frame - pass what it was given, not this pointer. */
int lnsfaid_frontend_sent_bits(lnsfaid_ctx* ctx, const int8_t** d_outputBits);

/* ---- FEC status ------------------------------------------------------------------------------------------
 * What a receiver can say about a decoded batch WITHOUT the sent bits - which codewords are uncorrectable, how many bits were
 * corrected: the PON FEC performance counters - and, when the sent frames are at hand, which error frames were detected and which
 * are miscorrections.  The decisions may come from any decode call of this library or from elsewhere.  One definition for every
 * entry point, per codeword c = 32 g + m of the batch (frame m of group g):
 *   bit          code bit k of the codeword is 1 when decodedBits[g][m * n_var + k] != 0 (the layout of lnsfaid_decode); packed form:
 *                bit k % 32 of word c * n_var / 32 + k / 32 of bits (the layout of lnsfaid_decode_packed).
 *   unsatisfied  the rows of H with an odd number of 1-bits among the row's variable nodes, over all n_var bits, the punctured tail
 *                included: for one output the same number as lnsfaid_codeword_stats::unsatisfied.  0 means a codeword.
 *   channel decision  of code bit k: x > 0 ? 1 : 0 with x = fixInput[g][m * K + k] for k < K, else fixInput[g][32 * K + m * M + (k - K)]
 *                (the layout of lnsfaid_decode; the > 0 rule of the pre-FEC counters and of the decoder's output stage: 0 and every
 *                negative value decide 0).  Packed form: x is the two's-complement nibble of llr4, 0x8 decides 0.
 *   corrected    the k < n_var - puncture_tail at which the bit differs from the channel decision (the decoder never sees the LLRs of
 *                the punctured tail).  fixInput == NULL: 0 for every codeword.
 *   records[c]   {unsatisfied, corrected}, in batch order.  May be NULL.
 *   out          may be NULL.  ADDED to; four words, so that lnsfaid_allreduce_counters sums them unchanged:
 *                out[0] TotalCodewords          += 32 per group
 *                out[1] UncorrectableCodewords  unsatisfied > 0
 *                out[2] CorrectedCodewords      unsatisfied == 0 and corrected > 0
 *                out[3] CorrectedBits           the sum of corrected over the codewords with unsatisfied == 0
 *   vs_sent      may be NULL (sent is then not read).  ADDED to.  sent has the layout of the capture call's sent ([32][K] then [32][M]
 *                per group, group g at byte g * 32 * n_var); only the K information bytes of a frame are read, and a decision is
 *                wrong when its byte (packed form: its bit as a byte) differs from the sent byte: the rule of lnsfaid_count_errors.
 *                sent == NULL means the all-zero codeword.
 *                vs_sent[0] TestFrame             += 32 per group
 *                vs_sent[1] ErrorFrame            a wrong information bit: what lnsfaid_count_errors* adds
 *                vs_sent[2] UndetectedErrorFrame  a wrong information bit and unsatisfied == 0: a valid but wrong codeword
 *                vs_sent[3] FalseAlarmFrame       no wrong information bit and unsatisfied > 0
 * Every output is a pure function of the inputs.
 * Rules: n_groups == 0 is a no-op (every buffer may be NULL).  LNSFAID_E_INVAL, with no output touched: a NULL ctx or code; a NULL
 * decisions pointer with n_groups > 0; n_groups > max_groups (device forms); a code with n_var % 32 != 0 (packed forms); a code
 * struct whose tables are missing or do not add up (host forms: 0 < n_check < n_var, 0 <= puncture_tail <= n_var, deg_rows summing
 * to n_check, deg * deg_rows to n_edges, every pos_vn < n_var). */
typedef struct lnsfaid_fec_record {
    uint32_t unsatisfied; /* parity checks the decisions leave unsatisfied */
    uint32_t corrected;   /* transmitted bits that differ from the channel's hard decision */
} lnsfaid_fec_record;
/* Host only, no context, no GPU: row by row from code->pos_vn, deg and deg_rows, so they serve any code the struct can describe
 * (quasi-cyclic or not).  The reference the device forms are tested against.  Host pointers of any alignment. */
int lnsfaid_fec_status_host(const lnsfaid_code* code, const int8_t* fixInput, const int8_t* decodedBits, const int8_t* sent,
                            size_t n_groups, lnsfaid_fec_record* records, uint64_t out[4], uint64_t vs_sent[4]);
int lnsfaid_fec_status_packed_host(const lnsfaid_code* code, const uint8_t* llr4, const uint32_t* bits, const int8_t* sent,
                                   size_t n_groups, lnsfaid_fec_record* records, uint64_t out[4], uint64_t vs_sent[4]);
/* The three inputs are device pointers of any alignment (more alignment only widens the loads, it never changes a count); d_records is
 * a device pointer (4-byte aligned) or NULL; out and vs_sent are host pointers.  A pure read of its inputs.  Queues on the context's
 * stream and returns when out / vs_sent are complete (the records are complete on the stream by then); no synchronisation by the
 * caller is needed after a preceding *_device call.  The only read-back is one copy of the eight accumulators, which live on the
 * context's device (allocated at the first call, freed by lnsfaid_destroy). */
int lnsfaid_fec_status_device(lnsfaid_ctx* ctx, const int8_t* d_fixInput, const int8_t* d_decodedBits, const int8_t* d_sent,
                              size_t n_groups, lnsfaid_fec_record* d_records, uint64_t out[4], uint64_t vs_sent[4]);
int lnsfaid_fec_status_packed_device(lnsfaid_ctx* ctx, const uint8_t* d_llr4, const uint32_t* d_bits, const int8_t* d_sent,
                                     size_t n_groups, lnsfaid_fec_record* d_records, uint64_t out[4], uint64_t vs_sent[4]);

/* ---- systematic encoder and device frame source (replaces CLDPC::Encode, reference CLDPC.cpp:68-155) ---------------
 * H = [A | B], B = the last n_check columns.  The parity bits of information bits u are p = B^-1 A u; B^-1 is derived from the
 * code table (the reference's GenMatrix is not shipped) lazily, at the first lnsfaid_encode* / lnsfaid_frontend_random_frames
 * call of a context, and kept on its device.  For a code whose parity part is singular these three calls return
 * LNSFAID_E_CODE; decoding is not affected. */

/* Host only, no GPU: the compact inverse of the parity part of H (the last n_check columns).  B^-1 is block-circulant, so the
 * first row of each z x z block describes it:
 *   circ[(a * mb + b) * (z / 8) + c / 8] bit (c % 8) = entry (a*z, b*z + c) of B^-1, mb = n_check / z.
 * LNSFAID_E_CODE if the code is not quasi-cyclic (same rule as lnsfaid_create) or B is singular;
 * LNSFAID_E_INVAL if bytes < mb * mb * z / 8. */
int lnsfaid_code_parity_inverse(const lnsfaid_code* code, uint8_t* circ, size_t bytes);

/* Replaces CLDPC::Encode (reference CLDPC.cpp:68-155) for n_groups groups:
 *   inputBits  [32][K] per group (int8 0/1), group g at g * 32 * K
 *   outputBits [32][K] then [32][M] per group, group g at g * 32 * n_var: the layout of CLDPC::outputBits and of
 *              lnsfaid_frontend_set_frames
 * _device: device pointers on the context's GPU (any byte offset); plain: host pointers, staged through the context's
 * buffers of lnsfaid_io_buffers (their content is overwritten).  n_groups 0: no-op; more than max_groups: LNSFAID_E_INVAL.
 * Both return when the output is complete. */
int lnsfaid_encode_device(lnsfaid_ctx* ctx, const int8_t* d_inputBits, size_t n_groups, int8_t* d_outputBits);
int lnsfaid_encode(lnsfaid_ctx* ctx, const int8_t* inputBits, size_t n_groups, int8_t* outputBits);

/* lnsfaid_frontend_set_frames without host buffers: draws the message bits of n_streams groups on the device from keys[s],
 * encodes them, and leaves both where set_frames leaves its copies.  The following lnsfaid_frontend_device* calls with
 * codeword = NULL send these frames, and lnsfaid_frontend_input_bits returns the message bits for
 * lnsfaid_count_errors_device; lnsfaid_frontend_set_frames(NULL) returns to one codeword for all, set_frames with host
 * buffers replaces them.  Returns when the frames are on the device.
 * Message generator (stateless, counter-based, bit-sliced by construction):
 *   mix64(x):  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31  (splitmix64 finaliser)
 *   stream s, information position j (0 <= j < K):  h = mix64(mix64(keys[s]) + (j + 1) * 0x9E3779B97F4A7C15)  (mod 2^64)
 *   frame l (l < 32) of stream s carries information bit j = (h >> l) & 1. */
int lnsfaid_frontend_random_frames(lnsfaid_ctx* ctx, const uint64_t* keys, size_t n_streams);

/* The context's own device staging buffers (each max_groups * 32 * n_var bytes): the fixInput buffer the
 * host-pointer entry points copy into and the decodedBits buffer they copy out of.  A host driver without its own
 * device allocator (host/CLDPC.cpp) runs front-end -> decode -> counters on them with the *_device entry points. */
int lnsfaid_io_buffers(lnsfaid_ctx* ctx, int8_t** d_fixInput, int8_t** d_decodedBits, lnsfaid_group_stats** d_stats);

/* Page-lock / release a host buffer (hipHostRegister / hipHostUnregister) for callers that have no HIP toolchain of
 * their own: with fixInput and decodedBits both pinned, lnsfaid_decode overlaps its copies with the decode (pieces of
 * whole groups on separate streams); pageable buffers are copied, decoded and copied back in sequence.  Unregister before
 * the buffer is freed. */
int lnsfaid_host_register(void* ptr, size_t bytes);
int lnsfaid_host_unregister(void* ptr);

/* Copy the per-group iteration counts a *_device decode left in the context's statistics buffer (the d_stats of
 * lnsfaid_io_buffers) to the host: what Decode_OMSBF / Decode_OMS_DTBF return as BFiter (reference CLDPC.h:150-151,
 * histogrammed into iterCount.txt by CSimulate.cpp:148-178) when the decoded frames themselves stay on the device. */
int lnsfaid_read_stats(lnsfaid_ctx* ctx, lnsfaid_group_stats* stats, size_t n_groups);

/* ---- multi-GPU: counters summed over RCCL (reference main.cpp:174-182) ---------------------
 * Groups of 32 codewords are independent, so a batch shards over GPUs as contiguous ranges of whole groups with no data-path
 * traffic; the only exchange is the sum of {TestFrame, ErrorFrame, ErrorBits, LT3ErrBitFrame} the reference's main thread
 * forms after pthread_join.  One context per GPU (one process or one host thread each):
 *   rank 0:     lnsfaid_comm_unique_id(id), hand `id` to the other ranks by any means (file, pipe, MPI, torch store)
 *   every rank: lnsfaid_comm_init(ctx, n_ranks, rank, id)       (collective: returns when all ranks have called it)
 *   per round:  lnsfaid_allreduce_counters(ctx, counters)       (in place: every rank ends up with the sums;
 *                                                                one ncclAllReduce of 4 x uint64 on the context's stream)
 * lnsfaid_comm_attach takes an existing ncclComm_t of the caller (not destroyed by the library) instead of creating one.
 * RCCL is looked up at run time (the copy already loaded in the process, else librccl.so.1): LNSFAID_E_NODEVICE if absent. */
#define LNSFAID_COMM_ID_BYTES 128
int lnsfaid_comm_unique_id(uint8_t id[LNSFAID_COMM_ID_BYTES]);
int lnsfaid_comm_init(lnsfaid_ctx* ctx, int32_t n_ranks, int32_t rank, const uint8_t id[LNSFAID_COMM_ID_BYTES]);
int lnsfaid_comm_attach(lnsfaid_ctx* ctx, void* nccl_comm);
int lnsfaid_comm_destroy(lnsfaid_ctx* ctx);
int lnsfaid_allreduce_counters(lnsfaid_ctx* ctx, uint64_t counters[4]);

/* Which decode kernel the context launches.  rows_per_lane 0 (default): chosen per configuration - the byte-parallel kernel
 * with four check rows per lane and one wavefront per codeword for DecodeMethods 1..5 with FAID tables that are uniform over
 * the weight classes and non-decreasing (every set the reference ships) and for DecodeMethod 0 with Factor_1 == Factor_2 in
 * 15 .. 2114 (one normalisation factor whose scaled minimum has at most 16 levels), the two-rows-per-lane kernel otherwise
 * (NMS with two factors or a factor outside that range, other tables); 2 / 4 force one of them (4: LNSFAID_E_INVAL where it does
 * not apply).  Both produce identical results; the
 * switch exists for tests and A/B timing.  lnsfaid_kernel_rows_per_lane returns what the next decode will launch. */
int lnsfaid_select_kernel(lnsfaid_ctx* ctx, int32_t rows_per_lane);
int lnsfaid_kernel_rows_per_lane(const lnsfaid_ctx* ctx);

/* EXPERIMENTAL.  Wavefronts per codeword of the four-rows-per-lane kernel: 1 (default; 0 selects the default) or 2
 * (lnsfaid_kernel5.hip: the edges of a layer are dealt to two waves, four waves per SIMD instead of two; DecodeMethods 1..5
 * without the erasing EF_ELIMINATION 2, messages streamed through HBM).  Results are identical; LNSFAID_E_INVAL where it does
 * not apply.  Environment: LNSFAID_WAVES_PER_CODEWORD=2 forces it for every context it applies to.  lnsfaid_kernel_waves
 * returns what the next decode will launch. */
int lnsfaid_select_waves(lnsfaid_ctx* ctx, int32_t waves_per_codeword);
int lnsfaid_kernel_waves(const lnsfaid_ctx* ctx);

/* Where the four-rows-per-lane kernel keeps the check-to-variable messages (the reference's var_msgs, CLDPC.h:123,
 * lifetime CDecoder_FAID.cpp:211-214 ... :923) between the layers of a launch.  LNSFAID_MSG_REGISTERS: the compressed messages
 * of the codeword (72 dwords per lane for the 12 layers of the 50G-PON code) stay in the wavefront's registers for the whole
 * launch and reach HBM only when a codeword parks - no vector-memory operation inside the layer loop; available for codes of
 * up to 12 layers, not for EF_ELIMINATION 2 and not for DecodeMethod 0.  LNSFAID_MSG_HBM: streamed through HBM one layer ahead of use (every code).
 * 0 (default): registers where available.  Identical results either way; the switch exists for tests and A/B timing.
 * lnsfaid_message_store returns what the next decode will use. */
#define LNSFAID_MSG_REGISTERS 1
#define LNSFAID_MSG_HBM 2
int lnsfaid_select_message_store(lnsfaid_ctx* ctx, int32_t where);
int lnsfaid_message_store(const lnsfaid_ctx* ctx);

/* The layer step without byte rotations on identity circulants (lnsfaid_kernel4z.hip).  Through a circulant of shift 0 a lane's
 * four rows meet the four bytes of one dword in order, so nothing has to be rotated; the library orders every layer's edges
 * zero-shift first (the order of a row's edges is free in the four-rows kernels) and runs each layer on an instance of the step
 * that knows how many leading groups of four edges need no rotation.  Used by the group rule's int8 decode with the messages in
 * registers (DecodeMethods 1..5) on a code that has such a layer; every other configuration runs as before.  0 (default): where
 * it applies; LNSFAID_ZERO_SHIFT_ON: the same, LNSFAID_E_INVAL where it does not apply; LNSFAID_ZERO_SHIFT_OFF: the rotating
 * kernel.  Identical results either way; the switch exists for tests and A/B timing.  Environment: LNSFAID_ZERO_SHIFT=off.
 * On the built-in 50G-PON code (any code whose zero-first edge tables equal its tables entry by entry) the rotation-free kernel
 * has a layer-static twin (lnsfaid_kernel4s.hip): straight-line code over the twelve layers with degrees, shifts and block columns
 * as compile-time constants, every identity circulant rotation-free.  The default and LNSFAID_ZERO_SHIFT_ON launch it where it
 * applies; LNSFAID_ZERO_SHIFT_LOOP keeps the layer loop of lnsfaid_kernel4z.hip there too (LNSFAID_E_INVAL where the rotation-free
 * kernel does not apply); LNSFAID_ZERO_SHIFT_STATIC asks for the twin, LNSFAID_E_INVAL where it does not apply.  Environment:
 * LNSFAID_ZERO_SHIFT=loop.
 * Where the twin applies and the configuration cannot open the error-floor window (floor_iter_thresh < 0), the default, _ON and
 * _STATIC launch the twin's window-free form (lnsfaid_kernel4w.hip): the same decoder without the window's per-layer work and
 * with a text of its own for the first iteration.  LNSFAID_ZERO_SHIFT_WINDOWED keeps lnsfaid_kernel4s.hip there too
 * (LNSFAID_E_INVAL where the twin does not apply).  Environment: LNSFAID_ZERO_SHIFT=windowed.  lnsfaid_window_free returns 1 if the
 * next decode launches the window-free form, 0 if not (lnsfaid_zero_shift_groups reports 2 for either).
 * lnsfaid_zero_shift_groups returns 0 if the next decode launches the rotating kernel, 1 for the rotation-free kernel's layer loop,
 * 2 for its layer-static twin, and writes the number of whole rotation-free groups of four edges for each of the first n layers
 * (zeros when it is not in use; the twin also goes without rotation on the identity edges beyond them).
 * lnsfaid_code_zero_shift_order needs no GPU: it returns the number of layers (or an error) and writes, per layer, the number of
 * leading groups of four zero-shift edges (groups[layer], before rounding to a compiled instance) and the edge order of the
 * rotation-free tables (order[layer * 24 + j]: the edge of the code's own row that is edge j there; -1 beyond the degree). */
#define LNSFAID_ZERO_SHIFT_ON 1
#define LNSFAID_ZERO_SHIFT_OFF 2
#define LNSFAID_ZERO_SHIFT_LOOP 3
#define LNSFAID_ZERO_SHIFT_STATIC 4
#define LNSFAID_ZERO_SHIFT_WINDOWED 5
int lnsfaid_select_zero_shift(lnsfaid_ctx* ctx, int32_t mode);
int lnsfaid_zero_shift_groups(const lnsfaid_ctx* ctx, int32_t* groups, int32_t n);
int lnsfaid_window_free(const lnsfaid_ctx* ctx);
int lnsfaid_code_zero_shift_order(const lnsfaid_code* code, int32_t* groups, int32_t* order);

/* Edge words.  Where the window-free form applies (lnsfaid_window_free), its kernel has a twin that reads every
 * rotating edge's LDS address and byte rotations from a compiled-in table instead of computing them in every layer
 * (lnsfaid_kernel4e.hip).  On by default; lnsfaid_select_edge_words(ctx, 0) keeps lnsfaid_kernel4w.hip there, (ctx, 1) goes back.
 * Identical results either way; the switch exists for tests and A/B timing.  Environment: LNSFAID_EDGE_WORDS=off.
 * lnsfaid_edge_words returns 1 if the next decode launches the twin, 0 if not: never 1 where lnsfaid_window_free returns 0.
 * lnsfaid_window_free and lnsfaid_zero_shift_groups answer the same with the twin as without. */
int lnsfaid_select_edge_words(lnsfaid_ctx* ctx, int32_t on);
int lnsfaid_edge_words(const lnsfaid_ctx* ctx);

/* The syndrome walk tables of the bit-flipping stage, without a GPU (for tests).  The stage flips block columns of weight
 * col_weight (REGULAR_COL_WEIGHT) only, so the library walks their circulants in every iteration (`flipped`) and all others once
 * when a codeword enters the stage (`fixed`); `full` is the walk of the layered stage's syndrome.  Per layer, slot and 32-row word
 * k two uint32: the LDS byte addresses of the two hard-plane words (low / high 16 bits) and the bit offset; unused slots point at
 * a word that holds zero.  full and fixed: [layers][24][8][2], flipped: [layers][info[2]][8][2].  info[0]: LDS byte offset of the
 * hard plane, info[1]: of the zero word, info[2]: slots per layer of `flipped`, info[3]: 1 if every layer's circulants of such
 * columns fit them (0: the stage walks `full` without register tables, and the contents of `flipped` are undefined: it lacks the
 * circulants that did not fit), info[4]: number of such block columns.  Returns the number of layers or an error. */
int lnsfaid_code_bf_walk(const lnsfaid_code* code, int32_t col_weight, uint32_t* full, uint32_t* flipped, uint32_t* fixed, int32_t* info);

/* Workgroups (codewords) of the selected decode kernel a compute unit holds at once, from the HIP occupancy query, next to
 * what the kernel's LDS footprint alone would allow, at most the 8 per compute unit the kernels' register budget is written for
 * (50G-PON: 8 and 8; a code with a smaller LDS image: still 8; a wider one: fewer, 5 for N = 27648).  A smaller first number means
 * a build lost residency to registers - about 40 % of the throughput for the one-wave-per-codeword kernel.  Also checks that the kernel has no static LDS
 * (LNSFAID_E_INTERNAL otherwise; every decode call checks the same once per kernel instance). */
int lnsfaid_kernel_residency(lnsfaid_ctx* ctx, int32_t* workgroups_per_cu, int32_t* lds_limit);

/* ---- measurement hooks ------------------------------------------------------- */

/* Device time (HIP events on the context's stream) and launch count of the
 * decode kernel accumulated since the last reset: out_ms = total kernel
 * milliseconds, out_launches = number of kernel launches (launches queued ahead
 * on a batch that turned out to be complete already are counted too: microseconds
 * each).  Calls of a one-group context that went through the call combiner are
 * not in it (they ran in launches shared with other contexts). */
int lnsfaid_kernel_time(lnsfaid_ctx* ctx, double* out_ms, uint64_t* out_launches, int32_t reset);

/* The HIP stream of the context as an opaque pointer (hipStream_t). */
void* lnsfaid_stream(lnsfaid_ctx* ctx);

const char* lnsfaid_strerror(int err);
const char* lnsfaid_last_hip_error(void);
const char* lnsfaid_version(void);

#ifdef __cplusplus
}
#endif
#endif /* LNSFAID_H */
