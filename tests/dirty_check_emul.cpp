/*
 * dirty_check_emul.cpp - TEST PROGRAM: the decision points' cheap "certainly dirty" test compiled for the host.
 * The per-lane row parity of the layer-static kernel (sw50_row_parity<BR>, csrc/lnsfaid_static50.h: stage 1 on the layer with the
 * most identity circulants, stage 2 on layer 0) and of every other kernel (sw_row_parity, csrc/lnsfaid_swar.h: run-time tables,
 * all 24 entries read) run over the 64 lanes of En images in the interleaved, biased LDS layout.  Bit 7 of byte k of lane l's word
 * is compared with the parity of row l + 64 k of the layer, computed node by node from the base matrix of
 * csrc/lnsfaid_gpon_base.h (row i of a circulant { cb, shift } checks node cb * 256 + (shift + i) mod 256) under the rule "hard
 * decision = En > 0".  The run-time function is also compared with the text it replaced, which is kept HERE (old_row_parity).
 *
 * No input.  Prints one line per case group and "total mismatches: n"; exit status 0 iff n == 0.
 */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "lnsfaid_static50.h"

namespace {
constexpr int Z = 256, NBC = 69;
struct Circ { int cb, shift; };
const int kDeg[SW50_LAYERS] = LNSFAID_GPON_ROW_DEG;
const Circ kBase[SW50_LAYERS][LNSFAID_GPON_MAX_DEG] = LNSFAID_GPON_BASE;

typedef std::vector<int> En; /* En of every variable node, code order */

std::vector<uint8_t> image(const En& en)
{
    std::vector<uint8_t> img(NBC * Z);
    for (uint32_t v = 0; v < (uint32_t)(NBC * Z); ++v) img[sw_en_pos(v)] = (uint8_t)(en[v] + SW_BIAS_EN);
    return img;
}

/* the reference: parity of the 256 rows of layer br */
void ref_parity(const En& en, int br, int par[Z])
{
    for (int i = 0; i < Z; ++i) {
        int p = 0;
        for (int j = 0; j < kDeg[br]; ++j) p ^= en[kBase[br][j].cb * Z + (kBase[br][j].shift + i) % Z] > 0;
        par[i] = p;
    }
}

/* the library's run-time tables of a layer, as LfDevCode holds them: 4 * shift and block column * 256 in ascending block column,
 * the entries beyond the degree 0 */
struct RunTab {
    uint32_t s4[SW_MAX_DEG], cb[SW_MAX_DEG];
    int deg;
    explicit RunTab(int br)
    {
        memset(s4, 0, sizeof(s4)); memset(cb, 0, sizeof(cb));
        deg = kDeg[br];
        for (int j = 0; j < deg; ++j) { s4[j] = (uint32_t)kBase[br][j].shift << 2; cb[j] = (uint32_t)kBase[br][j].cb << 8; }
    }
};

/* what layer0_dirty4 of csrc/lnsfaid_rows4.h was before it read its tables unconditionally: every table access and every LDS read
 * under "j < deg" */
uint32_t old_row_parity(const SwLds& lds, const uint32_t* s4row, const uint32_t* cbrow, int deg, uint32_t lane)
{
    const uint32_t tid4 = lane << 2;
    uint32_t x4[SW_MAX_DEG], d[SW_MAX_DEG];
    for (int j = 0; j < SW_MAX_DEG; ++j) x4[j] = j < deg ? tid4 + s4row[j] : 0u;
    for (int j = 0; j < SW_MAX_DEG; ++j)
        if (j < deg) d[j] = lds.rd32((x4[j] & 0xfcu) | cbrow[j]);
    uint32_t acc = 0;
    for (int j = 0; j < SW_MAX_DEG; ++j)
        if (j < deg) acc ^= sw_alignbyte(d[j], d[j], x4[j] >> 8) + 0x07070707u;
    return acc;
}

enum Which { STATIC, RUNTIME };

template <int BR>
struct Check {
    /* words of all lanes -> number of rows whose bit differs from the reference; `rows` (if given) receives the flagged rows */
    static long run(const En& en, Which w, std::vector<int>* rows = nullptr)
    {
        std::vector<uint8_t> img = image(en);
        const std::vector<uint8_t> before = img;
        SwLds lds; lds.base = img.data();
        int par[Z];
        ref_parity(en, BR, par);
        const RunTab rt(BR);
        long bad = 0;
        for (uint32_t lane = 0; lane < 64; ++lane) {
            uint32_t word;
            if (w == STATIC) word = sw50_row_parity<BR>(lds, lane);
            else {
                word = sw_row_parity(lds, rt.s4, rt.cb, rt.deg, lane);
                const uint32_t old = old_row_parity(lds, rt.s4, rt.cb, rt.deg, lane);
                if ((word ^ old) & 0x80808080u) { if (bad++ < 8) printf("layer %d lane %u: new %08x, old text %08x\n", BR, lane, word, old); }
            }
            for (int k = 0; k < 4; ++k) {
                const int got = (word >> (8 * k + 7)) & 1;
                if (got != par[lane + 64 * k]) { if (bad++ < 8) printf("layer %d row %u: parity %d, reference %d\n", BR, lane + 64 * k, got, par[lane + 64 * k]); }
                if (got && rows) rows->push_back((int)lane + 64 * k);
            }
        }
        if (img != before) { printf("layer %d: the check wrote to the image\n", BR); ++bad; }
        return bad;
    }

    static bool has_col(int cb)
    {
        for (int j = 0; j < kDeg[BR]; ++j) if (kBase[BR][j].cb == cb) return true;
        return false;
    }
    static int shift_of(int cb)
    {
        for (int j = 0; j < kDeg[BR]; ++j) if (kBase[BR][j].cb == cb) return kBase[BR][j].shift;
        return -1;
    }

    /* all cases for one function on this layer; cb_has / cb_lacks: a block column the layer has / lacks */
    static long cases(Which w, int cb_has, int cb_lacks)
    {
        long bad = 0;
        if (!has_col(cb_has) || has_col(cb_lacks)) { printf("layer %d: columns %d / %d are not a column it has / lacks\n", BR, cb_has, cb_lacks); return 1; }
        /* 200 random images, En over its whole range */
        uint32_t s = 2024u + 31u * (uint32_t)BR + (w == STATIC ? 0u : 7u);
        long dirty_rows = 0;
        for (int n = 0; n < 200; ++n) {
            En en(NBC * Z);
            for (auto& x : en) { s = s * 1664525u + 1013904223u; x = (int)((s >> 16) % 63u) - 31; }
            std::vector<int> rows;
            bad += run(en, w, &rows);
            dirty_rows += (long)rows.size();
        }
        if (dirty_rows < 200 * 64) { printf("layer %d: %ld unsatisfied rows over 200 random images: the images test nothing\n", BR, dirty_rows); ++bad; }
        /* the all-clean image (the all-zero codeword at |En| = 7): nothing */
        const En clean(NBC * Z, -7);
        {
            std::vector<int> rows;
            bad += run(clean, w, &rows);
            if (!rows.empty()) { printf("layer %d: %zu rows reported on the clean image\n", BR, rows.size()); ++bad; }
        }
        /* every single-node sign flip in a column the layer has: exactly the row that contains the node; in one it lacks: none */
        for (int i = 0; i < Z; ++i) {
            En en = clean;
            en[cb_has * Z + i] = 7;
            std::vector<int> rows;
            bad += run(en, w, &rows);
            const int want = ((i - shift_of(cb_has)) % Z + Z) % Z;
            if (rows.size() != 1 || rows[0] != want) { if (bad++ < 8) printf("layer %d: node %d of column %d flipped, %zu rows reported, row %d wanted\n", BR, i, cb_has, rows.size(), want); }
            en = clean;
            en[cb_lacks * Z + i] = 7;
            rows.clear();
            bad += run(en, w, &rows);
            if (!rows.empty()) { if (bad++ < 8) printf("layer %d: node %d of column %d flipped, %zu rows reported, none wanted\n", BR, i, cb_lacks, rows.size()); }
        }
        /* the boundary of the hard decision: En = 0 is "not positive", En = 1 is */
        for (int i = 0; i < Z; i += 37) {
            for (int val = 0; val <= 1; ++val) {
                En en = clean;
                en[cb_has * Z + i] = val;
                std::vector<int> rows;
                bad += run(en, w, &rows);
                if (rows.size() != (size_t)val) { if (bad++ < 8) printf("layer %d: En = %d at node %d of column %d: %zu rows reported\n", BR, val, i, cb_has, rows.size()); }
            }
        }
        printf("layer %d, %s tables: %ld mismatches\n", BR, w == STATIC ? "compile-time" : "run-time", bad);
        return bad;
    }
};
}

int main()
{
    long bad = 0;
    constexpr int S1 = SW50_CHECK_LAYER;
    static_assert(S1 == 1 && Sw50Tab<S1>::NZ == 22 && Sw50Tab<S1>::DEG == 22, "stage 1 asks layer 1 of the built-in code: 22 of 22 edges identities");
    printf("stage 1 layer: %d\n", S1);
    /* block column 1: layer 1 has it, layer 0 lacks it; block column 0: layer 0 has it, layer 1 lacks it */
    bad += Check<S1>::cases(STATIC, 1, 0);  /* stage 1 */
    bad += Check<0>::cases(STATIC, 0, 1);   /* stage 2 */
    bad += Check<0>::cases(RUNTIME, 0, 1);  /* every other kernel: layer 0, degree 23 of 24 entries */
    bad += Check<1>::cases(RUNTIME, 1, 0);  /* the same function on a layer of degree 22: two unused entries */
    bad += Check<7>::cases(STATIC, 12, 0);  /* a layer that mixes identity and rotating edges (column 12: an identity edge) */
    bad += Check<7>::cases(STATIC, 1, 3);   /* (column 1: a rotating one) */
    printf("total mismatches: %ld\n", bad);
    return bad == 0 ? 0 : 1;
}
