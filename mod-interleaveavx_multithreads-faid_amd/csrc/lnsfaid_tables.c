/*
 * lnsfaid_tables.c — built-in code definition and the reference's shipped decoder constants.
 *
 * (1) The 50G-PON mother code as a 12 x 69 base matrix of circulant shifts (Z = 256).  The reference
 *     stores the same code expanded to 70400 VN indices in `PosNoeudsVariable`
 *     (Constants/50GPON-dc-original/Constants_SSE.h:29-3102); row br*256+i of that table is
 *     { cb*256 + ((shift + i) mod 256) } in ascending cb.  lnsfaid_code_50gpon()
 *     regenerates the table in that exact order; tests pin it by SHA-256 and, when the reference is
 *     mounted, by a text comparison with the header.
 * (2) lnsfaid_cfg_default(): the constants compiled into CDecoder_OMS.cpp / CDecoder_FAID.cpp /
 *     CDecoder_FAID_2B1C.cpp (file:line next to each value).
 */
#include "lnsfaid.h"
#include <string.h>

#include "lnsfaid_gpon_base.h" /* the base matrix itself: shared with the layer-static decode kernel's compile-time tables */

#define GPON_Z 256
#define GPON_BLOCK_ROWS LNSFAID_GPON_BLOCK_ROWS
#define GPON_BLOCK_COLS 69
#define GPON_MAX_DEG LNSFAID_GPON_MAX_DEG

typedef struct { int16_t cb; int16_t shift; } gpon_circ;

static const int gpon_row_deg[GPON_BLOCK_ROWS] = LNSFAID_GPON_ROW_DEG;

static const gpon_circ gpon_base[GPON_BLOCK_ROWS][GPON_MAX_DEG] = LNSFAID_GPON_BASE;

int lnsfaid_code_50gpon(lnsfaid_code* code, uint16_t* pos_vn, int32_t* deg3, int32_t* deg_rows3)
{
    if (!code || !pos_vn || !deg3 || !deg_rows3) return LNSFAID_E_INVAL;
    size_t e = 0;
    for (int br = 0; br < GPON_BLOCK_ROWS; ++br)
        for (int i = 0; i < GPON_Z; ++i)
            for (int j = 0; j < gpon_row_deg[br]; ++j)
                pos_vn[e++] = (uint16_t)(gpon_base[br][j].cb * GPON_Z + ((gpon_base[br][j].shift + i) % GPON_Z));
    /* DEG_1 23 x256, DEG_2 22 x256, DEG_3 23 x2560 (Constants_SSE.h:14-19) */
    deg3[0] = 23; deg_rows3[0] = 256;
    deg3[1] = 22; deg_rows3[1] = 256;
    deg3[2] = 23; deg_rows3[2] = 2560;
    code->n_var = GPON_BLOCK_COLS * GPON_Z;   /* _NoVar   17664 */
    code->n_check = GPON_BLOCK_ROWS * GPON_Z; /* _NoCheck 3072  */
    code->n_edges = (int32_t)e;               /* _NoOnes  70400 */
    code->z = GPON_Z;
    code->puncture_tail = 384;                /* CDecoder_FAID.cpp:253-255 */
    code->nb_degres = 3;
    code->deg = deg3;
    code->deg_rows = deg_rows3;
    code->pos_vn = pos_vn;
    return LNSFAID_OK;
}

static void fill_map(int8_t dst[4][8], const int8_t row[8])
{
    for (int w = 0; w < 4; ++w) memcpy(dst[w], row, 8);
}

/* The reference's other compile-time table sets of Decode_FAID (#define FAID32 / FAID2 instead of FAID3,
 * CDecoder_FAID.cpp:8, :51-127); every weight class carries the same row in all of them. */
int lnsfaid_cfg_table_preset(lnsfaid_cfg* cfg, int32_t preset)
{
    static const int8_t faid3[6][8] = { /* CDecoder_FAID.cpp:13-48 */
        { 0, 1, 1, 2, 3, 3, 3, 3 }, { 0, 1, 1, 2, 3, 3, 3, 3 }, { 0, 1, 1, 2, 4, 4, 4, 4 },
        { 0, 1, 1, 3, 3, 4, 4, 4 }, { 0, 1, 1, 3, 3, 3, 6, 6 }, { 0, 1, 1, 3, 3, 3, 7, 7 },
    };
    static const int8_t faid32[6][8] = { /* CDecoder_FAID.cpp:52-87 */
        { 0, 1, 1, 2, 3, 3, 3, 3 }, { 0, 1, 1, 2, 3, 3, 3, 3 }, { 0, 1, 1, 2, 4, 4, 4, 4 },
        { 1, 1, 1, 1, 4, 4, 4, 4 }, { 1, 1, 1, 1, 5, 5, 5, 5 }, { 1, 1, 1, 1, 6, 6, 6, 6 },
    };
    static const int8_t faid2[6][8] = { /* CDecoder_FAID.cpp:91-126 */
        { 0, 0, 2, 2, 2, 2, 2, 2 }, { 0, 0, 2, 2, 2, 2, 2, 2 }, { 1, 1, 1, 3, 3, 3, 3, 3 },
        { 1, 1, 1, 4, 4, 4, 4, 4 }, { 1, 1, 1, 5, 5, 5, 5, 5 }, { 1, 1, 1, 6, 6, 6, 6, 6 },
    };
    const int8_t (*t)[8] = preset == LNSFAID_TABLES_FAID3 ? faid3 : preset == LNSFAID_TABLES_FAID32 ? faid32
                         : preset == LNSFAID_TABLES_FAID2 ? faid2 : 0;
    if (!cfg || !t) return LNSFAID_E_INVAL;
    for (int it = 0; it < 6; ++it) fill_map(cfg->v2c_map[it], t[it]);
    return LNSFAID_OK;
}

int lnsfaid_cfg_default(lnsfaid_cfg* cfg, int32_t decode_method, int32_t max_iteration)
{
    /* every weight class (3, 6, 11, other) carries the same row in the shipped tables */
    static const int8_t faid3[6][8] = {
        /* CDecoder_FAID.cpp:13-48 (#define FAID3, :8) */
        { 0, 1, 1, 2, 3, 3, 3, 3 }, { 0, 1, 1, 2, 3, 3, 3, 3 }, { 0, 1, 1, 2, 4, 4, 4, 4 },
        { 0, 1, 1, 3, 3, 4, 4, 4 }, { 0, 1, 1, 3, 3, 3, 6, 6 }, { 0, 1, 1, 3, 3, 3, 7, 7 },
    };
    static const int8_t faid_2b1c[6][8] = {
        /* CDecoder_FAID_2B1C.cpp:12-47 */
        { 0, 0, 1, 2, 3, 3, 3, 3 }, { 0, 1, 1, 2, 3, 3, 3, 3 }, { 0, 1, 1, 2, 3, 3, 3, 3 },
        { 0, 1, 1, 3, 3, 4, 4, 4 }, { 0, 1, 1, 3, 3, 3, 6, 6 }, { 0, 1, 1, 3, 3, 3, 7, 7 },
    };
    /* CDecoder_FAID.cpp:130-165, CDecoder_FAID_2B1C.cpp:49-84: identical for it1..it6 */
    static const int8_t ef[8] = { 2, 3, 3, 4, 5, 6, 6, 7 };
    static const int8_t ident[8] = { 0, 1, 2, 3, 4, 5, 6, 7 };

    if (!cfg || max_iteration < 0) return LNSFAID_E_INVAL;
    memset(cfg, 0, sizeof(*cfg));
    cfg->decode_method = decode_method;
    cfg->max_iteration = max_iteration;
    cfg->factor_1 = 1; /* Profile.txt:11 */
    cfg->factor_2 = 6; /* Profile.txt:12 */
    cfg->bf_L1 = 0;    /* _L1    CDecoder_FAID.cpp:169 */
    cfg->bf_alpha = 1; /* _alpha CDecoder_FAID.cpp:170 */
    cfg->bf_delta = 1; /* _delta CDecoder_FAID.cpp:167 */
    cfg->regular_col_weight = 3; /* CTool.h:6 */
    cfg->hard2_threshold = 13;   /* CDecoder_FAID_2B1C.cpp:6130 */
    cfg->bf_vote_cap = 5;        /* CDecoder_OMSBF.cpp:3332 */
    for (int it = 0; it < 6; ++it) fill_map(cfg->v2c_map_ef[it], ef);
    switch (decode_method) {
    case 0: /* Decode: normalised min-sum, Factor_1 / Factor_2 are numerators over 32 (CLDPC.cpp:337-352) */
        cfg->max_bf_iter = 0;
        for (int it = 0; it < 6; ++it) fill_map(cfg->v2c_map[it], ident);
        break;
    case 1: /* Decode_OMS */
        cfg->floor_err_count = 100;  /* CDecoder_OMS.cpp:28 */
        cfg->floor_iter_thresh = 4;  /* CDecoder_OMS.cpp:29 */
        cfg->ef_elimination = 0;
        cfg->max_bf_iter = 0;        /* no bit flipping stage */
        cfg->bf_L0 = 0;
        for (int it = 0; it < 6; ++it) fill_map(cfg->v2c_map[it], ident); /* min(|t|,7), CDecoder_OMS.cpp:374 */
        break;
    case 3: /* Decode_OMSBF: the OMS layered loop followed by plain bit flipping */
        cfg->floor_err_count = 100;  /* CDecoder_OMSBF.cpp:28 */
        cfg->floor_iter_thresh = 4;  /* CDecoder_OMSBF.cpp:29 */
        cfg->ef_elimination = 0;
        cfg->max_bf_iter = 50;       /* CDecoder_OMSBF.cpp:30 */
        for (int it = 0; it < 6; ++it) fill_map(cfg->v2c_map[it], ident);
        break;
    case 4: /* Decode_OMS_DTBF: the OMS layered loop followed by the DTBF stage with its own constants */
        cfg->floor_err_count = 100;  /* CDecoder_OMS_DTBF.cpp:33 */
        cfg->floor_iter_thresh = 4;  /* CDecoder_OMS_DTBF.cpp:34 */
        cfg->ef_elimination = 0;
        cfg->max_bf_iter = 50;       /* CDecoder_OMS_DTBF.cpp:35 */
        cfg->bf_L0 = 0;              /* CDecoder_OMS_DTBF.cpp:7  */
        cfg->bf_L1 = 50;             /* CDecoder_OMS_DTBF.cpp:8  */
        for (int it = 0; it < 6; ++it) fill_map(cfg->v2c_map[it], ident);
        break;
    case 2: /* Decode_FAID */
        cfg->floor_err_count = 0;    /* CDecoder_FAID.cpp:193 */
        cfg->floor_iter_thresh = -1; /* CDecoder_FAID.cpp:194 */
        cfg->ef_elimination = 0;     /* CDecoder_FAID.cpp:6   */
        cfg->max_bf_iter = 10;       /* CDecoder_FAID.cpp:208 */
        cfg->bf_L0 = 50;             /* CDecoder_FAID.cpp:168 */
        for (int it = 0; it < 6; ++it) fill_map(cfg->v2c_map[it], faid3[it]);
        break;
    case 5: /* Decode_FAID_2B1C */
        cfg->floor_err_count = 50;   /* CDecoder_FAID_2B1C.cpp:117 */
        cfg->floor_iter_thresh = 6;  /* CDecoder_FAID_2B1C.cpp:118 */
        cfg->ef_elimination = 1;     /* CDecoder_FAID_2B1C.cpp:5   */
        cfg->max_bf_iter = 10;       /* CDecoder_FAID_2B1C.cpp:128 */
        cfg->bf_L0 = 100;            /* CDecoder_FAID_2B1C.cpp:88  */
        for (int it = 0; it < 6; ++it) fill_map(cfg->v2c_map[it], faid_2b1c[it]);
        break;
    default:
        return LNSFAID_E_INVAL;
    }
    return LNSFAID_OK;
}

/* EF_ELIMINATION of CDecoder_FAID.cpp (:6, :192-203): 0 off (the shipped build), 1 error-floor tables, 2 tables + erasure. */
int lnsfaid_cfg_ef_elimination(lnsfaid_cfg* cfg, int32_t mode)
{
    if (!cfg || cfg->decode_method != 2 || mode < 0 || mode > 2) return LNSFAID_E_INVAL;
    cfg->ef_elimination = mode;
    cfg->floor_err_count = mode == 0 ? 0 : (mode == 1 ? 100 : 20);
    cfg->floor_iter_thresh = mode == 0 ? -1 : 6;
    return LNSFAID_OK;
}

/* ---- FEC status, host forms (include/lnsfaid.h "FEC status"): the definition taken literally, row by row from pos_vn ----
 * No quasi-cyclic shortcut and no device code: the reference lnsfaid_fecstatus.hip is tested against. */
#include <stdlib.h>

static int fec_code_rules(const lnsfaid_code* c, int packed)
{
    if (!c || !c->pos_vn || !c->deg || !c->deg_rows) return LNSFAID_E_INVAL;
    if (c->n_check <= 0 || c->n_var <= c->n_check || c->puncture_tail < 0 || c->puncture_tail > c->n_var || c->nb_degres < 0 ||
        c->n_edges < 0)
        return LNSFAID_E_INVAL;
    if (packed && c->n_var % 32 != 0) return LNSFAID_E_INVAL;
    long long rows = 0, edges = 0;
    for (int d = 0; d < c->nb_degres; ++d) {
        if (c->deg[d] < 0 || c->deg_rows[d] < 0) return LNSFAID_E_INVAL;
        rows += c->deg_rows[d];
        edges += (long long)c->deg[d] * c->deg_rows[d];
    }
    if (rows != c->n_check || edges != c->n_edges) return LNSFAID_E_INVAL;
    for (long long e = 0; e < edges; ++e)
        if ((int32_t)c->pos_vn[e] >= c->n_var) return LNSFAID_E_INVAL;
    return LNSFAID_OK;
}

/* fix / dec: the int8 form's buffers, or llr4 / bits of the packed form (bytes of any alignment) */
static int fec_status_host(const lnsfaid_code* code, int packed, const uint8_t* fix, const uint8_t* dec, const int8_t* sent,
                           size_t n_groups, lnsfaid_fec_record* records, uint64_t out[4], uint64_t vs_sent[4])
{
    const int rc = fec_code_rules(code, packed);
    if (rc) return rc;
    if (n_groups == 0) return LNSFAID_OK;
    if (!dec) return LNSFAID_E_INVAL;
    const size_t N = (size_t)code->n_var, M = (size_t)code->n_check, K = N - M, limit = N - (size_t)code->puncture_tail;
    uint8_t* bit = (uint8_t*)malloc(N);
    if (!bit) return LNSFAID_E_NOMEM;
    uint64_t add[4] = { 0, 0, 0, 0 }, vs[4] = { 0, 0, 0, 0 };
    for (size_t g = 0; g < n_groups; ++g) {
        for (size_t m = 0; m < LNSFAID_GROUP; ++m) {
            const size_t c = g * LNSFAID_GROUP + m;
            uint32_t corrected = 0, wrong = 0, unsatisfied = 0;
            for (size_t k = 0; k < N; ++k) {
                const size_t e = g * 32 * N + (k < K ? m * K + k : 32 * K + m * M + (k - K)); /* the element of fixInput and of sent */
                int raw; /* the decision as lnsfaid_count_errors compares it */
                if (packed) raw = (dec[(c * N + k) / 8] >> (k % 8)) & 1; /* little-endian words: bit k % 32 of word k / 32 */
                else raw = (int8_t)dec[c * N + k];
                bit[k] = raw != 0;
                if (fix && k < limit) {
                    int x;
                    if (packed) { x = (fix[e / 2] >> (e % 2 ? 4 : 0)) & 15; x = x >= 8 ? x - 16 : x; }
                    else x = (int8_t)fix[e];
                    corrected += (uint32_t)((x > 0) != bit[k]);
                }
                if (vs_sent && k < K) wrong += (uint32_t)(raw != (sent ? (int)sent[e] : 0));
            }
            size_t e = 0;
            for (int d = 0; d < code->nb_degres; ++d)
                for (int r = 0; r < code->deg_rows[d]; ++r) {
                    unsigned parity = 0;
                    for (int j = 0; j < code->deg[d]; ++j) parity ^= bit[code->pos_vn[e++]];
                    unsatisfied += parity;
                }
            if (records) { records[c].unsatisfied = unsatisfied; records[c].corrected = corrected; }
            if (unsatisfied > 0) add[1] += 1;
            else if (corrected > 0) { add[2] += 1; add[3] += corrected; }
            if (wrong > 0) { vs[1] += 1; vs[2] += unsatisfied == 0; }
            else vs[3] += unsatisfied > 0;
        }
        add[0] += LNSFAID_GROUP;
        vs[0] += LNSFAID_GROUP;
    }
    free(bit);
    if (out) for (int i = 0; i < 4; ++i) out[i] += add[i];
    if (vs_sent) for (int i = 0; i < 4; ++i) vs_sent[i] += vs[i];
    return LNSFAID_OK;
}

int lnsfaid_fec_status_host(const lnsfaid_code* code, const int8_t* fixInput, const int8_t* decodedBits, const int8_t* sent,
                            size_t n_groups, lnsfaid_fec_record* records, uint64_t out[4], uint64_t vs_sent[4])
{
    return fec_status_host(code, 0, (const uint8_t*)fixInput, (const uint8_t*)decodedBits, sent, n_groups, records, out, vs_sent);
}

int lnsfaid_fec_status_packed_host(const lnsfaid_code* code, const uint8_t* llr4, const uint32_t* bits, const int8_t* sent,
                                   size_t n_groups, lnsfaid_fec_record* records, uint64_t out[4], uint64_t vs_sent[4])
{
    return fec_status_host(code, 1, llr4, (const uint8_t*)bits, sent, n_groups, records, out, vs_sent);
}

/* ---- line formats, host helpers (include/lnsfaid.h "line-format decode") ----
 * Byte by byte, so that host pointers of any alignment do and the little-endian word order of the formats is spelled out: bit b
 * of word w is bit b % 8 of byte 4 w + b / 8. */
static int line_code_rules(const lnsfaid_code* c, int32_t format)
{
    if (!c || (format != LNSFAID_LINE_HARD && format != LNSFAID_LINE_LLR4)) return LNSFAID_E_INVAL;
    if (c->n_check <= 0 || c->n_var <= c->n_check || c->puncture_tail < 0 || c->puncture_tail >= c->n_var) return LNSFAID_E_INVAL;
    if ((c->n_var - c->puncture_tail) % 32 != 0 || (c->n_var - c->n_check) % 32 != 0) return LNSFAID_E_INVAL;
    return LNSFAID_OK;
}

/* element of fixInput / llr4 that holds code bit k of codeword cw: [32][K] information LLRs, then [32][M] parity LLRs per group */
static size_t line_group_element(size_t cw, size_t k, size_t N, size_t K)
{
    const size_t g = cw / LNSFAID_GROUP, m = cw % LNSFAID_GROUP;
    return g * LNSFAID_GROUP * N + (k < K ? m * K + k : LNSFAID_GROUP * K + m * (N - K) + (k - K));
}

int lnsfaid_line_from_fixinput(const lnsfaid_code* code, const int8_t* fixInput, size_t n_codewords, int32_t format, void* line)
{
    const int rc = line_code_rules(code, format);
    if (rc) return rc;
    if (n_codewords == 0) return LNSFAID_OK;
    if (!fixInput || !line) return LNSFAID_E_INVAL;
    const size_t N = (size_t)code->n_var, K = N - (size_t)code->n_check, L = N - (size_t)code->puncture_tail;
    uint8_t* out = (uint8_t*)line;
    for (size_t cw = 0; cw < n_codewords; ++cw) {
        if (format == LNSFAID_LINE_LLR4) {
            uint8_t* o = out + cw * (L / 2);
            for (size_t k = 0; k < L; k += 2) {
                const int a = fixInput[line_group_element(cw, k, N, K)], b = fixInput[line_group_element(cw, k + 1, N, K)];
                if (a < -8 || a > 7 || b < -8 || b > 7) return LNSFAID_E_INVAL;
                o[k / 2] = (uint8_t)((a & 15) | ((b & 15) << 4));
            }
        } else {
            uint8_t* o = out + cw * (L / 8);
            for (size_t k = 0; k < L; k += 8) {
                unsigned v = 0;
                for (size_t b = 0; b < 8; ++b) v |= (unsigned)(fixInput[line_group_element(cw, k + b, N, K)] > 0) << b;
                o[k / 8] = (uint8_t)v;
            }
        }
    }
    return LNSFAID_OK;
}

int lnsfaid_line_to_llr4(const lnsfaid_code* code, const void* line, int32_t format, int32_t magnitude, size_t n_codewords,
                         uint8_t* llr4)
{
    const int rc = line_code_rules(code, format);
    if (rc) return rc;
    if (format == LNSFAID_LINE_HARD && (magnitude < 1 || magnitude > 7)) return LNSFAID_E_INVAL;
    if (n_codewords == 0) return LNSFAID_OK;
    if (!line || !llr4) return LNSFAID_E_INVAL;
    const size_t N = (size_t)code->n_var, K = N - (size_t)code->n_check, L = N - (size_t)code->puncture_tail;
    const size_t n_groups = (n_codewords + LNSFAID_GROUP - 1) / LNSFAID_GROUP;
    const uint8_t* in = (const uint8_t*)line;
    memset(llr4, 0, n_groups * LNSFAID_GROUP * N / 2); /* the punctured tail and the padding codewords: nibble 0 */
    for (size_t cw = 0; cw < n_codewords; ++cw)
        for (size_t k = 0; k < L; ++k) {
            unsigned nib;
            if (format == LNSFAID_LINE_LLR4) nib = (in[cw * (L / 2) + k / 2] >> (k % 2 ? 4 : 0)) & 15u;
            else nib = (unsigned)(((in[cw * (L / 8) + k / 8] >> (k % 8)) & 1) ? magnitude : -magnitude) & 15u;
            const size_t e = line_group_element(cw, k, N, K);
            llr4[e / 2] |= (uint8_t)(nib << (e % 2 ? 4 : 0));
        }
    return LNSFAID_OK;
}

/* ---- line-format encode, host form (include/lnsfaid.h "line-format encode") ----
 * The definition of what lnsfaid_encode_line* return, for any quasi-cyclic code: s = A u row by row from pos_vn (the entries below
 * K), then p[a z + t] = XOR over the set bits (b, c) of block row a of circ of s[b z + (c + t) mod z].  Nothing of the built-in code
 * is used.  Bytes in and out, so that host pointers of any alignment do: bit b of word w is bit b % 8 of byte 4 w + b / 8. */
int lnsfaid_encode_line_host(const lnsfaid_code* code, const uint8_t* circ, size_t circ_bytes, const uint32_t* payload,
                             size_t n_codewords, uint32_t* line, uint32_t* bits)
{
    int rc = line_code_rules(code, LNSFAID_LINE_HARD);
    if (rc) return rc;
    rc = fec_code_rules(code, 1);
    if (rc) return rc;
    if (code->z <= 0 || code->z % 8 != 0 || code->n_check % code->z != 0 || code->puncture_tail > code->n_check) return LNSFAID_E_INVAL;
    const size_t N = (size_t)code->n_var, M = (size_t)code->n_check, K = N - M, L = N - (size_t)code->puncture_tail;
    const size_t z = (size_t)code->z, mb = M / z;
    if (!circ || circ_bytes < mb * mb * (z / 8)) return LNSFAID_E_INVAL;
    if (n_codewords == 0) return LNSFAID_OK;
    if (!payload || !line) return LNSFAID_E_INVAL;
    const size_t n_par = bits ? M : L - K; /* parity rows that leave: without bits the punctured tail is never formed */
    /* the support of circ as offsets into s2, where every block of s is stored twice in a row so that (c + t) needs no modulo */
    size_t n_sup = 0;
    for (size_t i = 0; i < mb * mb * (z / 8); ++i)
        for (unsigned v = circ[i]; v; v &= v - 1) n_sup += 1;
    uint32_t* sup = (uint32_t*)malloc((n_sup + 1) * sizeof(uint32_t));
    size_t* sup_off = (size_t*)malloc((mb + 1) * sizeof(size_t));
    uint8_t* s2 = (uint8_t*)malloc(2 * M);
    uint8_t* p = (uint8_t*)malloc(M);
    if (!sup || !sup_off || !s2 || !p) {
        free(sup); free(sup_off); free(s2); free(p);
        return LNSFAID_E_NOMEM;
    }
    n_sup = 0;
    for (size_t a = 0; a < mb; ++a) {
        sup_off[a] = n_sup;
        for (size_t b = 0; b < mb; ++b)
            for (size_t c = 0; c < z; ++c)
                if ((circ[(a * mb + b) * (z / 8) + c / 8] >> (c % 8)) & 1u) sup[n_sup++] = (uint32_t)(b * 2 * z + c);
    }
    sup_off[mb] = n_sup;
    const uint8_t* in = (const uint8_t*)payload;
    for (size_t cw = 0; cw < n_codewords; ++cw) {
        const uint8_t* u = in + cw * (K / 8);
        size_t e = 0, r = 0;
        for (int d = 0; d < code->nb_degres; ++d)
            for (int i = 0; i < code->deg_rows[d]; ++i, ++r) {
                unsigned parity = 0;
                for (int j = 0; j < code->deg[d]; ++j) {
                    const size_t k = code->pos_vn[e++];
                    if (k < K) parity ^= (unsigned)(u[k / 8] >> (k % 8)) & 1u;
                }
                s2[(r / z) * 2 * z + r % z] = s2[(r / z) * 2 * z + z + r % z] = (uint8_t)parity;
            }
        for (size_t a = 0; a * z < n_par; ++a) {
            uint8_t* pa = p + a * z;
            memset(pa, 0, z);
            for (size_t i = sup_off[a]; i < sup_off[a + 1]; ++i) {
                const uint8_t* sr = s2 + sup[i];
                for (size_t t = 0; t < z; ++t) pa[t] ^= sr[t];
            }
        }
        uint8_t* lo = (uint8_t*)line + cw * (L / 8);
        memcpy(lo, u, K / 8);
        for (size_t k = 0; k < L - K; k += 8) {
            unsigned v = 0;
            for (size_t b = 0; b < 8; ++b) v |= (unsigned)p[k + b] << b;
            lo[(K + k) / 8] = (uint8_t)v;
        }
        if (bits) {
            uint8_t* bo = (uint8_t*)bits + cw * (N / 8);
            memcpy(bo, u, K / 8);
            for (size_t k = 0; k < M; k += 8) {
                unsigned v = 0;
                for (size_t b = 0; b < 8; ++b) v |= (unsigned)p[k + b] << b;
                bo[(K + k) / 8] = (uint8_t)v;
            }
        }
    }
    free(sup); free(sup_off); free(s2); free(p);
    return LNSFAID_OK;
}

/* ---- line-format link, host forms (include/lnsfaid.h "line-format link") ----
 * The definition of what lnsfaid_line_payload_random_device, lnsfaid_line_bsc_device and lnsfaid_line_count_errors_device return.
 * Words are read and written byte by byte (little-endian), so host pointers of any alignment do. */
static uint64_t link_mix64(uint64_t x)
{
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
static uint64_t link_cwkey(uint64_t key, uint64_t C, uint64_t d) { return link_mix64(link_mix64(key + d) + (C + 1u) * 0xD1B54A32D192ED03ull); }
static uint64_t link_draw(uint64_t cwkey, uint64_t q) { return link_mix64(cwkey + (q + 1u) * 0x9E3779B97F4A7C15ull); }
static uint32_t link_ld32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
static void link_st32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }
static uint32_t link_popcount(uint32_t v) { uint32_t n = 0; for (; v; v &= v - 1u) n += 1u; return n; }

int lnsfaid_line_bsc_threshold(double p, uint32_t* threshold)
{
    if (!threshold || !(p >= 0.0 && p < 1.0)) return LNSFAID_E_INVAL; /* NaN fails both comparisons */
    *threshold = (uint32_t)(p * 4294967296.0); /* exact product (a power of two), below 2^32, truncated: the floor */
    return LNSFAID_OK;
}

int lnsfaid_line_payload_random_host(const lnsfaid_code* code, uint64_t key, uint64_t first_codeword, size_t n_codewords, uint32_t* payload)
{
    const int rc = line_code_rules(code, LNSFAID_LINE_HARD);
    if (rc) return rc;
    if (n_codewords == 0) return LNSFAID_OK;
    if (!payload) return LNSFAID_E_INVAL;
    const size_t kw = (size_t)(code->n_var - code->n_check) / 32;
    uint8_t* out = (uint8_t*)payload;
    for (size_t i = 0; i < n_codewords; ++i) {
        const uint64_t ck = link_cwkey(key, first_codeword + (uint64_t)i, 1u);
        for (size_t w = 0; w < kw; w += 2) {
            const uint64_t h = link_draw(ck, (uint64_t)(w / 2));
            link_st32(out + 4 * (i * kw + w), (uint32_t)h);
            if (w + 1 < kw) link_st32(out + 4 * (i * kw + w + 1), (uint32_t)(h >> 32)); /* an odd K / 32 leaves the last high half unused */
        }
    }
    return LNSFAID_OK;
}

int lnsfaid_line_bsc_host(const lnsfaid_code* code, const uint32_t* line_in, size_t n_codewords, uint64_t key, uint64_t first_codeword,
                          uint32_t threshold, uint32_t* line_out, uint32_t* flips, uint64_t* total_flips)
{
    const int rc = line_code_rules(code, LNSFAID_LINE_HARD);
    if (rc) return rc;
    if (n_codewords == 0) return LNSFAID_OK;
    if (!line_in || !line_out) return LNSFAID_E_INVAL;
    const size_t lw = (size_t)(code->n_var - code->puncture_tail) / 32;
    const uint8_t* in = (const uint8_t*)line_in;
    uint8_t* out = (uint8_t*)line_out;
    uint64_t total = 0;
    for (size_t i = 0; i < n_codewords; ++i) {
        const uint64_t ck = link_cwkey(key, first_codeword + (uint64_t)i, 2u);
        uint32_t n = 0;
        for (size_t w = 0; w < lw; ++w) {
            uint32_t mask = 0;
            for (uint32_t j = 0; j < 16u; ++j) { /* position 32 w + 2 j is the low half of draw q = 16 w + j, 32 w + 2 j + 1 the high half */
                const uint64_t h = link_draw(ck, (uint64_t)(16 * w + j));
                mask |= (uint32_t)((uint32_t)h < threshold) << (2u * j);
                mask |= (uint32_t)((uint32_t)(h >> 32) < threshold) << (2u * j + 1u);
            }
            link_st32(out + 4 * (i * lw + w), link_ld32(in + 4 * (i * lw + w)) ^ mask);
            n += link_popcount(mask);
        }
        if (flips) link_st32((uint8_t*)flips + 4 * i, n);
        total += n;
    }
    if (total_flips) *total_flips += total;
    return LNSFAID_OK;
}

int lnsfaid_line_count_errors_host(const lnsfaid_code* code, const uint32_t* payload, const uint32_t* sent, const lnsfaid_line_stats* stats,
                                   size_t n_codewords, uint64_t errors[4], uint64_t fec[4], uint64_t vs_sent[4])
{
    const int rc = line_code_rules(code, LNSFAID_LINE_HARD);
    if (rc) return rc;
    if (n_codewords == 0) return LNSFAID_OK;
    if (!payload || ((fec || vs_sent) && !stats)) return LNSFAID_E_INVAL;
    const size_t kw = (size_t)(code->n_var - code->n_check) / 32;
    const uint8_t* got = (const uint8_t*)payload;
    const uint8_t* ref = (const uint8_t*)sent;
    const uint8_t* st = (const uint8_t*)stats;
    uint64_t e[4] = { 0, 0, 0, 0 }, f[4] = { 0, 0, 0, 0 }, v[4] = { 0, 0, 0, 0 };
    for (size_t i = 0; i < n_codewords; ++i) {
        uint64_t wrong = 0;
        for (size_t w = 0; w < kw; ++w)
            wrong += link_popcount(link_ld32(got + 4 * (i * kw + w)) ^ (ref ? link_ld32(ref + 4 * (i * kw + w)) : 0u));
        e[0] += 1; e[1] += wrong > 0; e[2] += wrong; e[3] += wrong == 1 || wrong == 2;
        if (st) {
            const int32_t unsatisfied = (int32_t)link_ld32(st + sizeof(lnsfaid_line_stats) * i + 8);
            const int32_t corrected = (int32_t)link_ld32(st + sizeof(lnsfaid_line_stats) * i + 12);
            f[0] += 1;
            if (unsatisfied > 0) f[1] += 1;
            else if (unsatisfied == 0 && corrected > 0) { f[2] += 1; f[3] += (uint64_t)corrected; }
            v[0] += 1;
            if (wrong > 0) { v[1] += 1; v[2] += unsatisfied == 0; }
            else v[3] += unsatisfied > 0;
        }
    }
    for (int k = 0; k < 4; ++k) {
        if (errors) errors[k] += e[k];
        if (fec) fec[k] += f[k];
        if (vs_sent) vs_sent[k] += v[k];
    }
    return LNSFAID_OK;
}

/* ---- line-format soft channel, host form and table helper (include/lnsfaid.h "line-format soft channel") ----
 * The definition of what lnsfaid_line_soft_device returns.  Bytes in, bytes out: host pointers of any alignment do. */
#include <math.h>

int lnsfaid_line_awgn_table(double sigma, double scale, uint32_t table[14])
{
    if (!table || !(sigma > 0.0 && sigma < INFINITY) || !(scale > 0.0 && scale < INFINITY)) return LNSFAID_E_INVAL; /* NaN fails the comparisons */
    for (int i = 0; i < 14; ++i) {
        const int j = i < 7 ? i - 7 : i - 6; /* -7 .. -1, 1 .. 7: level 0 is the double-width bin of a truncation toward zero */
        const double b = (double)j / scale;
        const double phi = 0.5 * erfc(-((b - 1.0) / sigma) / sqrt(2.0));
        const double t = floor(4294967296.0 * phi);
        table[i] = t >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)t;
    }
    return LNSFAID_OK;
}

/* LNSFAID_OK for fourteen non-decreasing thresholds, which it copies to t */
static int soft_table_rules(const uint32_t* table, uint32_t t[14])
{
    if (!table) return LNSFAID_E_INVAL;
    memcpy(t, table, 14 * sizeof(uint32_t));
    for (int i = 1; i < 14; ++i)
        if (t[i] < t[i - 1]) return LNSFAID_E_INVAL;
    return LNSFAID_OK;
}

int lnsfaid_line_soft_host(const lnsfaid_code* code, const uint32_t* line_in, size_t n_codewords, uint64_t key, uint64_t first_codeword,
                           const uint32_t table[14], uint8_t* llr4_out, uint32_t* flips, uint64_t* total_flips)
{
    const int rc = line_code_rules(code, LNSFAID_LINE_HARD);
    if (rc) return rc;
    if (n_codewords == 0) return LNSFAID_OK;
    uint32_t thr[14];
    if (!line_in || !llr4_out || soft_table_rules(table, thr)) return LNSFAID_E_INVAL;
    const size_t L = (size_t)(code->n_var - code->puncture_tail);
    const uint8_t* in = (const uint8_t*)line_in;
    const uintptr_t a = (uintptr_t)in, b = (uintptr_t)llr4_out; /* the output is four times the input: no overlap can be right */
    if (a < b + n_codewords * (L / 2) && b < a + n_codewords * (L / 8)) return LNSFAID_E_INVAL;
    uint64_t total = 0;
    for (size_t i = 0; i < n_codewords; ++i) {
        const uint64_t ck = link_cwkey(key, first_codeword + (uint64_t)i, 3u);
        uint32_t n = 0;
        for (size_t q = 0; q < L / 2; ++q) { /* position 2 q is the low half of draw q, 2 q + 1 the high half: one output byte */
            const uint64_t h = link_draw(ck, (uint64_t)q);
            const unsigned bits = (unsigned)(in[i * (L / 8) + q / 4] >> (2 * (q % 4))) & 3u;
            unsigned byte = 0;
            for (unsigned half = 0; half < 2u; ++half) {
                const uint32_t u = half ? (uint32_t)(h >> 32) : (uint32_t)h;
                int m = -7;
                for (int t = 0; t < 14; ++t) m += u >= thr[t];
                const int bit = (int)(bits >> half) & 1;
                const int level = bit ? m : -m;
                n += (uint32_t)((level > 0) != bit);
                byte |= ((unsigned)level & 15u) << (4u * half);
            }
            llr4_out[i * (L / 2) + q] = (uint8_t)byte;
        }
        if (flips) link_st32((uint8_t*)flips + 4 * i, n);
        total += n;
    }
    if (total_flips) *total_flips += total;
    return LNSFAID_OK;
}

/* ---- line-format error-propagation channel, host form and threshold helper (include/lnsfaid.h "line-format error-propagation
 * channel") ----
 * The definition of what lnsfaid_line_markov_device returns: the BSC's draws, walked position by position with the previous decision
 * choosing the threshold.  Words and thresholds are read and written byte by byte: host pointers of any alignment do. */
int lnsfaid_line_markov_thresholds(double ber, double propagation, uint32_t t[3])
{
    const double p = ber, a = propagation;
    if (!t || !(p >= 0.0 && p <= a && a < 1.0)) return LNSFAID_E_INVAL; /* NaN fails the comparisons */
    const uint32_t t_after = (uint32_t)(a * 4294967296.0), t_start = (uint32_t)(p * 4294967296.0); /* exact products, truncated: the floor */
    uint32_t t_idle = t_start; /* a == p: the BSC */
    if (a != p) {
        t_idle = (uint32_t)floor(4294967296.0 * p * (1.0 - a) / (1.0 - p)); /* below a * 2^32 < 2^32 up to rounding */
        if (t_idle > t_after) t_idle = t_after; /* a rounding of the quotient must not break the rule of the channel */
    }
    link_st32((uint8_t*)t, t_idle); link_st32((uint8_t*)t + 4, t_after); link_st32((uint8_t*)t + 8, t_start);
    return LNSFAID_OK;
}

int lnsfaid_line_markov_host(const lnsfaid_code* code, const uint32_t* line_in, size_t n_codewords, uint64_t key, uint64_t first_codeword,
                             const uint32_t t[3], uint32_t* line_out, uint32_t* flips, uint32_t* runs, uint64_t* total_flips,
                             uint64_t* total_runs)
{
    const int rc = line_code_rules(code, LNSFAID_LINE_HARD);
    if (rc) return rc;
    if (n_codewords == 0) return LNSFAID_OK;
    if (!line_in || !line_out || !t) return LNSFAID_E_INVAL;
    const uint32_t t_idle = link_ld32((const uint8_t*)t), t_after = link_ld32((const uint8_t*)t + 4), t_start = link_ld32((const uint8_t*)t + 8);
    if (t_idle > t_after) return LNSFAID_E_INVAL;
    const size_t lw = (size_t)(code->n_var - code->puncture_tail) / 32;
    const uint8_t* in = (const uint8_t*)line_in;
    uint8_t* out = (uint8_t*)line_out;
    uint64_t total = 0, total_r = 0;
    for (size_t i = 0; i < n_codewords; ++i) {
        const uint64_t ck = link_cwkey(key, first_codeword + (uint64_t)i, 2u);
        uint32_t e = (uint32_t)link_draw(ck, (uint64_t)(16 * lw)) < t_start; /* the draw after the BSC's last: e of position -1 */
        uint32_t before = 0, n = 0, r = 0;                                    /* before: e of the position before, 0 in front of the codeword */
        for (size_t w = 0; w < lw; ++w) {
            uint32_t mask = 0;
            for (uint32_t k = 0; k < 32u; ++k) { /* position 32 w + k: the low half of draw q = 16 w + k / 2 for even k, the high half for odd k */
                const uint64_t h = link_draw(ck, (uint64_t)(16 * w + k / 2u));
                const uint32_t u = (k & 1u) ? (uint32_t)(h >> 32) : (uint32_t)h;
                e = u < (e ? t_after : t_idle);
                mask |= e << k;
                n += e;
                r += e & ~before;
                before = e;
            }
            link_st32(out + 4 * (i * lw + w), link_ld32(in + 4 * (i * lw + w)) ^ mask);
        }
        if (flips) link_st32((uint8_t*)flips + 4 * i, n);
        if (runs) link_st32((uint8_t*)runs + 4 * i, r);
        total += n;
        total_r += r;
    }
    if (total_flips) *total_flips += total;
    if (total_runs) *total_runs += total_r;
    return LNSFAID_OK;
}

/* ---- burst-format line calls, host forms (include/lnsfaid.h "burst-format line calls") ----
 * Codeword c of a burst is shortened by S_c bits: the information positions [k0, k0 + S_c) are known zeros and are not on the line.
 * Everything is byte by byte (S_c is a multiple of 32, so every codeword starts on a byte in both formats), and `shortened` is read
 * byte by byte too: host pointers of any alignment do. */
static uint32_t burst_s(const uint32_t* shortened, size_t c) { return shortened ? link_ld32((const uint8_t*)shortened + 4 * c) : 0u; }

/* the code (N, K and L multiples of 32, K <= L) and every S_c: S_c % 32 == 0 and 0 <= S_c <= K - 32 */
static int burst_rules(const lnsfaid_code* code, const uint32_t* shortened, size_t n_codewords, uint64_t* line_bits, uint64_t* payload_bits)
{
    const int rc = line_code_rules(code, LNSFAID_LINE_HARD);
    if (rc) return rc;
    if (code->n_var % 32 != 0 || code->puncture_tail > code->n_check) return LNSFAID_E_INVAL;
    const uint64_t N = (uint64_t)code->n_var, K = N - (uint64_t)code->n_check, L = N - (uint64_t)code->puncture_tail;
    uint64_t s_sum = 0;
    for (size_t c = 0; c < n_codewords; ++c) {
        const uint32_t s = burst_s(shortened, c);
        if (s % 32u != 0u || (uint64_t)s + 32u > K) return LNSFAID_E_INVAL;
        s_sum += s;
    }
    if (line_bits) *line_bits = (uint64_t)n_codewords * L - s_sum;
    if (payload_bits) *payload_bits = (uint64_t)n_codewords * K - s_sum;
    return LNSFAID_OK;
}

static int burst_where_rules(int32_t where) { return where == LNSFAID_SHORTEN_TAIL || where == LNSFAID_SHORTEN_HEAD ? LNSFAID_OK : LNSFAID_E_INVAL; }

int lnsfaid_burst_words(const lnsfaid_code* code, const uint32_t* shortened, size_t n_codewords, uint64_t* line_bits, uint64_t* payload_bits)
{
    uint64_t lb = 0, pb = 0;
    const int rc = burst_rules(code, shortened, n_codewords, &lb, &pb);
    if (rc) return rc;
    if (line_bits) *line_bits = lb;
    if (payload_bits) *payload_bits = pb;
    return LNSFAID_OK;
}

int lnsfaid_burst_to_llr4(const lnsfaid_code* code, const void* line, int32_t format, int32_t magnitude, const uint32_t* shortened,
                          int32_t where, size_t n_codewords, uint8_t* llr4)
{
    int rc = line_code_rules(code, format);
    if (rc) return rc;
    if (format == LNSFAID_LINE_HARD && (magnitude < 1 || magnitude > 7)) return LNSFAID_E_INVAL;
    if (burst_where_rules(where)) return LNSFAID_E_INVAL;
    rc = burst_rules(code, shortened, n_codewords, NULL, NULL);
    if (rc) return rc;
    if (n_codewords == 0) return LNSFAID_OK;
    if (!line || !llr4) return LNSFAID_E_INVAL;
    const size_t N = (size_t)code->n_var, K = N - (size_t)code->n_check, L = N - (size_t)code->puncture_tail;
    const size_t n_groups = (n_codewords + LNSFAID_GROUP - 1) / LNSFAID_GROUP;
    const uint8_t* in = (const uint8_t*)line;
    memset(llr4, 0, n_groups * LNSFAID_GROUP * N / 2); /* the punctured tail and the padding codewords: nibble 0 */
    size_t first = 0; /* the codeword's first position on the line, counted over the whole burst line */
    for (size_t cw = 0; cw < n_codewords; ++cw) {
        const size_t S = burst_s(shortened, cw), k0 = where == LNSFAID_SHORTEN_HEAD ? 0 : K - S;
        for (size_t p = 0; p < L; ++p) {
            unsigned nib;
            if (p >= k0 && p < k0 + S) nib = (unsigned)-7 & 15u; /* a known zero: the strongest level a line can carry */
            else {
                const size_t q = first + p - (p >= k0 + S ? S : 0);
                if (format == LNSFAID_LINE_LLR4) nib = (in[q / 2] >> (q % 2 ? 4 : 0)) & 15u;
                else nib = (unsigned)(((in[q / 8] >> (q % 8)) & 1) ? magnitude : -magnitude) & 15u;
            }
            const size_t e = line_group_element(cw, p, N, K);
            llr4[e / 2] |= (uint8_t)(nib << (e % 2 ? 4 : 0));
        }
        first += L - S;
    }
    return LNSFAID_OK;
}

/* The definition of what lnsfaid_encode_burst* return: the payload expanded with zeros in the known range, lnsfaid_encode_line_host,
 * the known words dropped from the line.  `bits` is the mother codeword as it is.  Chunks of 64 codewords through two heap buffers. */
int lnsfaid_encode_burst_host(const lnsfaid_code* code, const uint8_t* circ, size_t circ_bytes, const uint32_t* payload,
                              const uint32_t* shortened, int32_t where, size_t n_codewords, uint32_t* line, uint32_t* bits)
{
    /* everything lnsfaid_encode_line_host refuses is refused here before anything is written */
    int rc = lnsfaid_encode_line_host(code, circ, circ_bytes, NULL, 0, NULL, NULL);
    if (rc) return rc;
    if (burst_where_rules(where)) return LNSFAID_E_INVAL;
    rc = burst_rules(code, shortened, n_codewords, NULL, NULL);
    if (rc) return rc;
    if (n_codewords == 0) return LNSFAID_OK;
    if (!payload || !line) return LNSFAID_E_INVAL;
    const size_t N = (size_t)code->n_var, K = N - (size_t)code->n_check, L = N - (size_t)code->puncture_tail;
    const size_t chunk = n_codewords < 64 ? n_codewords : 64;
    uint8_t* full_pay = (uint8_t*)malloc(chunk * (K / 8));
    uint8_t* full_line = (uint8_t*)malloc(chunk * (L / 8));
    if (!full_pay || !full_line) {
        free(full_pay); free(full_line);
        return LNSFAID_E_NOMEM;
    }
    const uint8_t* in = (const uint8_t*)payload;
    uint8_t* out = (uint8_t*)line;
    for (size_t c0 = 0; c0 < n_codewords && rc == LNSFAID_OK; c0 += chunk) {
        const size_t nc = n_codewords - c0 < chunk ? n_codewords - c0 : chunk;
        for (size_t i = 0; i < nc; ++i) { /* expand: zeros in [k0, k0 + S) */
            const size_t S = burst_s(shortened, c0 + i), k0 = where == LNSFAID_SHORTEN_HEAD ? 0 : K - S;
            uint8_t* u = full_pay + i * (K / 8);
            memcpy(u, in, k0 / 8);
            memset(u + k0 / 8, 0, S / 8);
            memcpy(u + (k0 + S) / 8, in + k0 / 8, (K - S - k0) / 8);
            in += (K - S) / 8;
        }
        rc = lnsfaid_encode_line_host(code, circ, circ_bytes, (const uint32_t*)full_pay, nc, (uint32_t*)full_line,
                                      bits ? (uint32_t*)((uint8_t*)bits + c0 * (N / 8)) : NULL);
        for (size_t i = 0; i < nc && rc == LNSFAID_OK; ++i) { /* drop the known words */
            const size_t S = burst_s(shortened, c0 + i), k0 = where == LNSFAID_SHORTEN_HEAD ? 0 : K - S;
            const uint8_t* l = full_line + i * (L / 8);
            memcpy(out, l, k0 / 8);
            memcpy(out + k0 / 8, l + (k0 + S) / 8, (L - S - k0) / 8);
            out += (L - S) / 8;
        }
    }
    free(full_pay); free(full_line);
    return rc;
}

/* ---- burst-format link, host forms (include/lnsfaid.h "burst-format link") ----
 * The definition of what the lnsfaid_burst_*_device link calls return.  Every draw is indexed by the MOTHER position: transmitted word
 * wl of a codeword with known words [k0w, k0w + Sw) is mother word wi = wl + (wl >= k0w ? Sw : 0), and uses the draws 16 wi .. 16 wi + 15
 * that lnsfaid_line_*_host uses for word wi of the same global codeword.  Own loops over the transmitted words, no expanded image;
 * words are read and written byte by byte, so host pointers of any alignment do. */
static int burst_link_rules(const lnsfaid_code* code, const uint32_t* shortened, int32_t where, size_t n_codewords, uint64_t* line_bits)
{
    const int rc = line_code_rules(code, LNSFAID_LINE_HARD);
    if (rc) return rc;
    if (burst_where_rules(where)) return LNSFAID_E_INVAL;
    return burst_rules(code, shortened, n_codewords, line_bits, NULL);
}

int lnsfaid_burst_payload_random_host(const lnsfaid_code* code, uint64_t key, uint64_t first_codeword, const uint32_t* shortened,
                                      int32_t where, size_t n_codewords, uint32_t* payload)
{
    const int rc = burst_link_rules(code, shortened, where, n_codewords, NULL);
    if (rc) return rc;
    if (n_codewords == 0) return LNSFAID_OK;
    if (!payload) return LNSFAID_E_INVAL;
    const size_t kw = (size_t)(code->n_var - code->n_check) / 32;
    uint8_t* out = (uint8_t*)payload;
    for (size_t i = 0; i < n_codewords; ++i) {
        const uint64_t ck = link_cwkey(key, first_codeword + (uint64_t)i, 1u);
        const size_t sw = burst_s(shortened, i) / 32u, k0w = where == LNSFAID_SHORTEN_HEAD ? 0 : kw - sw;
        for (size_t wl = 0; wl < kw - sw; ++wl) {
            const size_t wi = wl + (wl >= k0w ? sw : 0); /* the mother word: the low half of draw wi / 2 when even, else the high half */
            const uint64_t h = link_draw(ck, (uint64_t)(wi / 2));
            link_st32(out, (wi & 1u) ? (uint32_t)(h >> 32) : (uint32_t)h);
            out += 4;
        }
    }
    return LNSFAID_OK;
}

int lnsfaid_burst_bsc_host(const lnsfaid_code* code, const uint32_t* line_in, const uint32_t* shortened, int32_t where, size_t n_codewords,
                           uint64_t key, uint64_t first_codeword, uint32_t threshold, uint32_t* line_out, uint32_t* flips,
                           uint64_t* total_flips)
{
    const int rc = burst_link_rules(code, shortened, where, n_codewords, NULL);
    if (rc) return rc;
    if (n_codewords == 0) return LNSFAID_OK;
    if (!line_in || !line_out) return LNSFAID_E_INVAL;
    const size_t kw = (size_t)(code->n_var - code->n_check) / 32, lw = (size_t)(code->n_var - code->puncture_tail) / 32;
    const uint8_t* in = (const uint8_t*)line_in;
    uint8_t* out = (uint8_t*)line_out;
    uint64_t total = 0;
    for (size_t i = 0; i < n_codewords; ++i) {
        const uint64_t ck = link_cwkey(key, first_codeword + (uint64_t)i, 2u);
        const size_t sw = burst_s(shortened, i) / 32u, k0w = where == LNSFAID_SHORTEN_HEAD ? 0 : kw - sw;
        uint32_t n = 0;
        for (size_t wl = 0; wl < lw - sw; ++wl) {
            const size_t wi = wl + (wl >= k0w ? sw : 0);
            uint32_t mask = 0;
            for (uint32_t j = 0; j < 16u; ++j) { /* mother position 32 wi + 2 j: the low half of draw 16 wi + j, + 1: the high half */
                const uint64_t h = link_draw(ck, (uint64_t)(16 * wi + j));
                mask |= (uint32_t)((uint32_t)h < threshold) << (2u * j);
                mask |= (uint32_t)((uint32_t)(h >> 32) < threshold) << (2u * j + 1u);
            }
            link_st32(out, link_ld32(in) ^ mask);
            in += 4; out += 4;
            n += link_popcount(mask);
        }
        if (flips) link_st32((uint8_t*)flips + 4 * i, n);
        total += n;
    }
    if (total_flips) *total_flips += total;
    return LNSFAID_OK;
}

int lnsfaid_burst_soft_host(const lnsfaid_code* code, const uint32_t* line_in, const uint32_t* shortened, int32_t where, size_t n_codewords,
                            uint64_t key, uint64_t first_codeword, const uint32_t table[14], uint8_t* llr4_out, uint32_t* flips,
                            uint64_t* total_flips)
{
    uint64_t line_bits = 0;
    const int rc = burst_link_rules(code, shortened, where, n_codewords, &line_bits);
    if (rc) return rc;
    if (n_codewords == 0) return LNSFAID_OK;
    uint32_t thr[14];
    if (!line_in || !llr4_out || soft_table_rules(table, thr)) return LNSFAID_E_INVAL;
    const size_t kw = (size_t)(code->n_var - code->n_check) / 32, lw = (size_t)(code->n_var - code->puncture_tail) / 32;
    const uint8_t* in = (const uint8_t*)line_in;
    uint8_t* out = llr4_out;
    const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out; /* the output is four times the input: no overlap can be right */
    if (a < b + (size_t)(line_bits / 2) && b < a + (size_t)(line_bits / 8)) return LNSFAID_E_INVAL;
    uint64_t total = 0;
    for (size_t i = 0; i < n_codewords; ++i) {
        const uint64_t ck = link_cwkey(key, first_codeword + (uint64_t)i, 3u);
        const size_t sw = burst_s(shortened, i) / 32u, k0w = where == LNSFAID_SHORTEN_HEAD ? 0 : kw - sw;
        uint32_t n = 0;
        for (size_t wl = 0; wl < lw - sw; ++wl) {
            const size_t wi = wl + (wl >= k0w ? sw : 0);
            const uint32_t x = link_ld32(in);
            for (uint32_t j = 0; j < 16u; ++j) { /* mother positions 32 wi + 2 j and + 1: draw 16 wi + j, one output byte */
                const uint64_t h = link_draw(ck, (uint64_t)(16 * wi + j));
                unsigned byte = 0;
                for (unsigned half = 0; half < 2u; ++half) {
                    const uint32_t u = half ? (uint32_t)(h >> 32) : (uint32_t)h;
                    int m = -7;
                    for (int t = 0; t < 14; ++t) m += u >= thr[t];
                    const int bit = (int)(x >> (2u * j + half)) & 1;
                    const int level = bit ? m : -m;
                    n += (uint32_t)((level > 0) != bit);
                    byte |= ((unsigned)level & 15u) << (4u * half);
                }
                out[j] = (uint8_t)byte;
            }
            in += 4; out += 16;
        }
        if (flips) link_st32((uint8_t*)flips + 4 * i, n);
        total += n;
    }
    if (total_flips) *total_flips += total;
    return LNSFAID_OK;
}

/* the counters of lnsfaid_line_count_errors_host on payloads of (K - S_c) / 32 words, with failed = unsatisfied > 0 || short_ones > 0
 * where the line counters have unsatisfied > 0 */
int lnsfaid_burst_count_errors_host(const lnsfaid_code* code, const uint32_t* payload, const uint32_t* sent, const lnsfaid_line_stats* stats,
                                    const uint32_t* short_ones, const uint32_t* shortened, size_t n_codewords, uint64_t errors[4],
                                    uint64_t fec[4], uint64_t vs_sent[4])
{
    const int rc = burst_rules(code, shortened, n_codewords, NULL, NULL);
    if (rc) return rc;
    if (n_codewords == 0) return LNSFAID_OK;
    if (!payload || ((fec || vs_sent) && !stats)) return LNSFAID_E_INVAL;
    const size_t kw = (size_t)(code->n_var - code->n_check) / 32;
    const uint8_t* got = (const uint8_t*)payload;
    const uint8_t* ref = (const uint8_t*)sent;
    const uint8_t* st = (const uint8_t*)stats;
    uint64_t e[4] = { 0, 0, 0, 0 }, f[4] = { 0, 0, 0, 0 }, v[4] = { 0, 0, 0, 0 };
    for (size_t i = 0; i < n_codewords; ++i) {
        const size_t words = kw - burst_s(shortened, i) / 32u;
        uint64_t wrong = 0;
        for (size_t w = 0; w < words; ++w) {
            wrong += link_popcount(link_ld32(got) ^ (ref ? link_ld32(ref) : 0u));
            got += 4;
            if (ref) ref += 4;
        }
        e[0] += 1; e[1] += wrong > 0; e[2] += wrong; e[3] += wrong == 1 || wrong == 2;
        if (st) {
            const int32_t unsatisfied = (int32_t)link_ld32(st + sizeof(lnsfaid_line_stats) * i + 8);
            const int32_t corrected = (int32_t)link_ld32(st + sizeof(lnsfaid_line_stats) * i + 12);
            const int failed = unsatisfied > 0 || (short_ones && link_ld32((const uint8_t*)short_ones + 4 * i) > 0u);
            f[0] += 1;
            if (failed) f[1] += 1;
            else if (unsatisfied == 0 && corrected > 0) { f[2] += 1; f[3] += (uint64_t)corrected; }
            v[0] += 1;
            if (wrong > 0) { v[1] += 1; v[2] += !failed && unsatisfied == 0; }
            else v[3] += failed;
        }
    }
    for (int k = 0; k < 4; ++k) {
        if (errors) errors[k] += e[k];
        if (fec) fec[k] += f[k];
        if (vs_sent) vs_sent[k] += v[k];
    }
    return LNSFAID_OK;
}

/* ---- line-format failure capture, host form (include/lnsfaid.h "line-format failure capture") ----
 * The definition of what lnsfaid_line_capture_device returns: the syndrome row by row from pos_vn, no quasi-cyclic shortcut.  Bytes
 * in, bytes out (little-endian words), so host pointers of any alignment do. */
static int capture_code_rules(const lnsfaid_code* code, int32_t format)
{
    const int rc = line_code_rules(code, format);
    if (rc) return rc;
    return code->n_var % 32 != 0 ? LNSFAID_E_INVAL : LNSFAID_OK;
}

static size_t capture_line_words(const lnsfaid_code* code, int32_t format)
{
    const size_t L = (size_t)(code->n_var - code->puncture_tail);
    return format == LNSFAID_LINE_LLR4 ? L / 8 : L / 32;
}

int lnsfaid_line_capture_words(const lnsfaid_code* code, int32_t format, uint32_t* words_per_record)
{
    const int rc = capture_code_rules(code, format);
    if (rc) return rc;
    if (!words_per_record) return LNSFAID_E_INVAL;
    *words_per_record = (uint32_t)(capture_line_words(code, format) + 2 * (size_t)(code->n_var / 32) + (size_t)(code->n_check / 32));
    return LNSFAID_OK;
}

int lnsfaid_line_capture_host(const lnsfaid_code* code, const void* line, int32_t format, const uint32_t* bits, const uint32_t* sent,
                              size_t n_codewords, uint64_t first_codeword, int32_t select, size_t skip, size_t capacity,
                              lnsfaid_line_failure* records, uint32_t* payload, uint64_t* found, uint64_t* stored)
{
    int rc = capture_code_rules(code, format);
    if (rc) return rc;
    if (select < 1 || select > 3 || (!sent && (select & LNSFAID_LINE_CAPTURE_WRONG))) return LNSFAID_E_INVAL;
    if (n_codewords == 0) {
        if (found) *found = 0;
        if (stored) *stored = 0;
        return LNSFAID_OK;
    }
    if (!bits || !found || !stored || (capacity > 0 && (!records || !payload))) return LNSFAID_E_INVAL;
    rc = fec_code_rules(code, 1);
    if (rc) return rc;
    const size_t N = (size_t)code->n_var, M = (size_t)code->n_check, K = N - M, L = N - (size_t)code->puncture_tail;
    const size_t nw = N / 32, mw = M / 32, lw = capture_line_words(code, format), W = lw + 2 * nw + mw;
    const uint8_t* in = (const uint8_t*)line;
    const uint8_t* dec = (const uint8_t*)bits;
    const uint8_t* ref = (const uint8_t*)sent;
    uint8_t* out = (uint8_t*)payload;
    uint8_t* bit = (uint8_t*)malloc(N);
    uint32_t* syn = (uint32_t*)malloc(4 * (mw ? mw : 1));
    if (!bit || !syn) { free(bit); free(syn); return LNSFAID_E_NOMEM; }
    uint64_t n_found = 0, n_stored = 0;
    for (size_t i = 0; i < n_codewords; ++i) {
        const uint8_t* d = dec + i * (N / 8);
        const uint8_t* s = ref ? ref + i * (N / 8) : NULL;
        lnsfaid_line_failure r;
        memset(&r, 0, sizeof(r));
        r.codeword = first_codeword + (uint64_t)i;
        r.index = (uint32_t)i;
        for (size_t k = 0; k < N; ++k) {
            bit[k] = (uint8_t)((d[k / 8] >> (k % 8)) & 1);
            if (s && bit[k] != ((s[k / 8] >> (k % 8)) & 1)) {
                if (k < K) r.wrong_payload += 1u;
                else r.wrong_parity += 1u;
            }
        }
        memset(syn, 0, 4 * mw);
        size_t e = 0, row = 0;
        for (int dg = 0; dg < code->nb_degres; ++dg)
            for (int q = 0; q < code->deg_rows[dg]; ++q, ++row) {
                unsigned parity = 0;
                for (int j = 0; j < code->deg[dg]; ++j) parity ^= bit[code->pos_vn[e++]];
                if (parity) { syn[row / 32] |= 1u << (row % 32); r.unsatisfied += 1u; }
            }
        r.flags = (r.unsatisfied > 0 ? (uint32_t)LNSFAID_LINE_CAPTURE_UNCORRECTABLE : 0u) |
                  (r.wrong_payload > 0 ? (uint32_t)LNSFAID_LINE_CAPTURE_WRONG : 0u);
        if (!(r.flags & (uint32_t)select)) continue;
        const uint64_t rank = n_found++;
        if (rank < (uint64_t)skip || rank - (uint64_t)skip >= (uint64_t)capacity) continue;
        const uint8_t* l = in ? in + i * lw * 4 : NULL;
        if (l && s)
            for (size_t k = 0; k < L; ++k) {
                unsigned ch;
                if (format == LNSFAID_LINE_LLR4) { const unsigned nib = (l[k / 2] >> (k % 2 ? 4 : 0)) & 15u; ch = nib >= 1u && nib <= 7u; }
                else ch = (l[k / 8] >> (k % 8)) & 1u;
                r.channel_errors += ch != ((unsigned)(s[k / 8] >> (k % 8)) & 1u);
            }
        uint8_t* p = out + (size_t)n_stored * W * 4;
        if (l) memcpy(p, l, lw * 4);
        else memset(p, 0, lw * 4);
        memcpy(p + lw * 4, d, nw * 4);
        for (size_t b = 0; b < nw * 4; ++b) p[(lw + nw) * 4 + b] = s ? (uint8_t)(d[b] ^ s[b]) : (uint8_t)0;
        for (size_t w = 0; w < mw; ++w) link_st32(p + (lw + 2 * nw + w) * 4, syn[w]);
        memcpy((uint8_t*)records + (size_t)n_stored * sizeof(r), &r, sizeof(r));
        n_stored += 1;
    }
    free(bit); free(syn);
    *found = n_found;
    *stored = n_stored;
    return LNSFAID_OK;
}
