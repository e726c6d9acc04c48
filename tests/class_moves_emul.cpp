/*
 * class_moves_emul.cpp - TEST PROGRAM: the layer step written for the issue classes (SW_FORM_VK | SW_FORM_MUL of sw_layer_step,
 * csrc/lnsfaid_swar.h: what lnsfaid_kernel4w.hip instantiates) compiled for the host, against the forms without them.
 *
 *  - helpers against the expressions they replace: exhaustively over one byte lane (all 256 values, in each of the four bytes, the
 *    other bytes running through a set of fillers that includes 0xff, so bits 24 .. 31 are set in a quarter of the words and more),
 *    and on 10^6 random dwords.  sw_shl8_mul and sw_mask7_mul must be exact for EVERY dword: the 24-bit multiply drops bits 24 .. 31
 *    of its operand, which a shift by 8 drops too - and the test also shows that the same multiply by 4 is NOT x << 2 on dwords
 *    with bits 24 .. 29 set, which is why no shift below 8 is written that way.  sw_mask6_mul equals sw_mask7(x << 1) for bytes
 *    <= 0x7f, sw_gather4_perm equals sw_gather4 for bytes, sw_therm2msg_vk equals sw_therm2msg, sw_update2_mul equals sw_update2.
 *  - the step: all 64 lanes of every layer of the 50G-PON code (degrees 23 and 22) from the same En image, the forms the kernel ran
 *    before (SW_FORM_NOWIN | SW_FORM_FRESH in iteration 1, SW_FORM_NOWIN afterwards) and the same with SW_FORM_VK | SW_FORM_MUL, and
 *    each of the two bits alone: En images and the rows' records byte for byte after every layer.
 *
 * Input (text, argv[1]) as tests/window_free_emul.cpp; tests/test_class_moves_cpu.py writes it.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "lnsfaid_static50.h"

namespace {
bool same(const SwRow& a, const SwRow& b) { return memcmp(&a, &b, sizeof(SwRow)) == 0; }

struct Tally {
    long checked = 0, bad = 0;
    void expect(bool ok, const char* what, uint32_t x, uint32_t got, uint32_t want)
    {
        ++checked;
        if (!ok && bad++ < 12) printf("%s(%08x): %08x, wanted %08x\n", what, x, got, want);
    }
};

/* one dword against every helper that takes one */
void helpers_on(uint32_t x, const SwK& K, Tally& t, long& needs_condition)
{
    const uint32_t sel = K.sel_sign;
    t.expect(sw_shl8_mul(x, K.c100) == x << 8, "sw_shl8_mul", x, sw_shl8_mul(x, K.c100), x << 8);
    t.expect(sw_mask7_mul(x, sel, K.c100) == sw_mask7(x, sel), "sw_mask7_mul", x, sw_mask7_mul(x, sel, K.c100), sw_mask7(x, sel));
    for (int n = 8; n <= 23; ++n) /* every factor the 24-bit multiply can hold from 256 on */
        t.expect(sw_mul_u24(x, 1u << n) == x << n, "sw_mul_u24 by a power of two >= 256", x, sw_mul_u24(x, 1u << n), x << n);
    if (sw_mul_u24(x, 4u) != x << 2) ++needs_condition;
    const uint32_t y = x & 0x7f7f7f7fu; /* bytes <= 0x7f: a record's cw */
    t.expect(sw_mask6_mul(y, sel, K.c100) == sw_mask7(y << 1, sel), "sw_mask6_mul", y, sw_mask6_mul(y, sel, K.c100), sw_mask7(y << 1, sel));
    const uint32_t g0 = x & 0xffu, g1 = (x >> 8) & 0xffu, g2 = (x >> 16) & 0xffu, g3 = x >> 24;
    t.expect(sw_gather4_perm(g0, g1, g2, g3) == sw_gather4(g0, g1, g2, g3) && sw_gather4_perm(g0, g1, g2, g3) == x, "sw_gather4_perm", x, sw_gather4_perm(g0, g1, g2, g3), x);
}

void helper_checks(Tally& t, long n_random)
{
    const SwK K = sw_consts();
    long needs_condition = 0;
    static const uint32_t fill[6] = { 0x00u, 0xffu, 0x80u, 0x7fu, 0x01u, 0xa5u };
    for (int k = 0; k < 4; ++k)
        for (uint32_t v = 0; v < 256; ++v)
            for (int f = 0; f < 6; ++f) {
                uint32_t x = 0;
                for (int b = 0; b < 4; ++b) x |= (b == k ? v : fill[(f + b) % 6]) << (8 * b);
                helpers_on(x, K, t, needs_condition);
            }
    uint32_t s = 20261u;
    long high = 0;
    for (long i = 0; i < n_random; ++i) {
        s = s * 1664525u + 1013904223u;
        const uint32_t x = s ^ (s >> 15);
        high += (x >> 24) != 0u;
        helpers_on(x, K, t, needs_condition);
    }
    printf("random dwords with bits 24..31 set: %ld of %ld\n", high, n_random);
    printf("dwords on which a 24-bit multiply by 4 is not the shift: %ld\n", needs_condition);
    /* sw_therm2msg_vk: every thermometer code in every byte, two tables */
    static const uint32_t codes[9] = { 0x00u, 0x01u, 0x03u, 0x07u, 0x0fu, 0x1fu, 0x3fu, 0xffu, 0x7fu };
    static const uint32_t luts[2][2] = { { 0x03020100u, 0x07060504u }, { 0x04050607u, 0x00010203u } };
    for (int l = 0; l < 2; ++l) {
        uint32_t tm[4];
        sw_therm2msg_tables(luts[l][0], luts[l][1], tm);
        for (int k = 0; k < 4; ++k)
            for (int ci = 0; ci < 9; ++ci)
                for (int other = 0; other < 9; ++other) {
                    uint32_t x = 0;
                    for (int b = 0; b < 4; ++b) x |= (b == k ? codes[ci] : codes[(other + b) % 9]) << (8 * b);
                    t.expect(sw_therm2msg_vk(x, tm, K.c0f) == sw_therm2msg(x, tm), "sw_therm2msg_vk", x, sw_therm2msg_vk(x, tm, K.c0f), sw_therm2msg(x, tm));
                }
    }
    /* sw_update2_mul: every t + 128 (+ FAID's bias) in every byte, both signs' masks, every magnitude, both row masks */
    for (int minsum = 0; minsum < 2; ++minsum)
        for (uint32_t c = 0; c < 8; ++c)
            for (uint32_t fm = 0; fm < 2; ++fm)
                for (uint32_t v = 0; v < 256; ++v)
                    for (int k = 0; k < 4; ++k) {
                        const uint32_t bias = minsum ? 0u : 0x06040200u;
                        const uint32_t tb = (v << (8 * k)) | (0x80808080u & ~(0xffu << (8 * k)));
                        const uint32_t ms = sw_mask7(tb - bias, K.sel_sign); /* 0xff where t >= 0 */
                        const uint32_t cc = c * 0x01010101u, fmm = fm ? 0xffffffffu : 0u;
                        uint32_t a, b;
                        if (minsum) {
                            const SwUpd2 u = sw_update2_consts<true>(cc, fmm, bias);
                            a = sw_update2<true>(tb, ms, u, K.sel_sign, K.cbit[7], K.cm27);
                            b = sw_update2_mul<true>(tb, ms, u, K.sel_sign, K.cbit[7], K.cm27, K.c100);
                        } else {
                            const SwUpd2 u = sw_update2_consts<false>(cc, fmm, bias);
                            a = sw_update2<false>(tb, ms, u, K.sel_sign, K.cbit[7], K.cm27);
                            b = sw_update2_mul<false>(tb, ms, u, K.sel_sign, K.cbit[7], K.cm27, K.c100);
                        }
                        t.expect(a == b, "sw_update2_mul", tb, b, a);
                    }
}

struct Run {
    std::vector<uint8_t> en;
    std::vector<SwRow> rec;
};

template <int METHOD, int BR, int EXTRA>
long step_all(Run& r, const SwParams& p, const SwK& K, bool fresh)
{
    typedef Sw50Tab<BR> Tab;
    SwLds l; l.base = r.en.data();
#define LANE(lane) ((EXTRA & SW_FORM_MUL) ? (lane) << 2 : (lane)) /* SW_FORM_MUL takes 4 * lane */
    for (uint32_t lane = 0; lane < 64; ++lane) {
        Tab tab; tab.sbv = 0u;
        SwRow* rr = &r.rec[BR * 64 + lane];
        if (fresh) {
            SwRow junk;
            memset(&junk, 0xa5, sizeof(junk));
            *rr = sw_layer_step<METHOD, Tab::DEG, false, 1, 0, 0, SW_PAIRS_ALL, SW_FORM_NOWIN | SW_FORM_FRESH | EXTRA>(l, tab, p, K, LANE(lane), Tab::DEG, junk, true, 0u, false);
        } else {
            *rr = sw_layer_step<METHOD, Tab::DEG, false, 1, 0, 0, SW_PAIRS_ALL, SW_FORM_NOWIN | EXTRA>(l, tab, p, K, LANE(lane), Tab::DEG, *rr, false, 0u, false);
        }
    }
#undef LANE
    return 0;
}

template <int METHOD, int BR>
long layer(Run r[4], const SwParams& p, const SwK& K, bool fresh, int it, int degs[2])
{
    long bad = 0;
    degs[Sw50Tab<BR>::DEG == 23 ? 1 : 0] += Sw50Tab<BR>::DEG == 23 || Sw50Tab<BR>::DEG == 22;
    step_all<METHOD, BR, 0>(r[0], p, K, fresh);
    step_all<METHOD, BR, SW_FORM_VK | SW_FORM_MUL>(r[1], p, K, fresh);
    step_all<METHOD, BR, SW_FORM_VK>(r[2], p, K, fresh);
    step_all<METHOD, BR, SW_FORM_MUL>(r[3], p, K, fresh);
    static const char* name[4] = { "", "VK | MUL", "VK", "MUL" };
    for (int v = 1; v < 4; ++v) {
        for (uint32_t lane = 0; lane < 64; ++lane)
            if (!same(r[0].rec[BR * 64 + lane], r[v].rec[BR * 64 + lane])) {
                if (bad++ < 8) printf("it %d layer %d lane %u: record of form %s differs\n", it, BR, lane, name[v]);
                r[v].rec[BR * 64 + lane] = r[0].rec[BR * 64 + lane];
            }
        if (r[0].en != r[v].en) { if (bad++ < 8) printf("it %d layer %d: En image of form %s differs\n", it, BR, name[v]); r[v].en = r[0].en; }
    }
    return bad;
}

template <int METHOD>
long run(const SwParams pit[6], int n_iter, int n_seeds, long& rows_compared, int degs[2])
{
    long bad = 0;
    static const int corner[8] = { -31, -30, -8, -1, 0, 1, 7, 31 };
    for (int seed = 0; seed < n_seeds; ++seed) {
        Run r[4];
        r[0].en.resize(69 * 256);
        uint32_t s = 8765u + 1009u * (uint32_t)seed;
        const int kind = seed % 3; /* channel-like values, the whole range of En, corner values only */
        const int amp = kind == 0 ? 7 : 31;
        for (auto& x : r[0].en) {
            s = s * 1664525u + 1013904223u;
            const int v = kind == 2 ? corner[(s >> 16) & 7u] : (int)((s >> 16) % (uint32_t)(2 * amp + 1)) - amp;
            x = (uint8_t)(SW_BIAS_EN + v);
        }
        r[0].rec.resize(SW50_LAYERS * 64);
        memset(r[0].rec.data(), 0, r[0].rec.size() * sizeof(SwRow));
        r[1] = r[0]; r[2] = r[0]; r[3] = r[0];
        for (int it = 1; it <= n_iter; ++it) {
            SwParams p = pit[it <= 5 ? it - 1 : 5];
            p.window = 0;
            SwK K = sw_consts();
            sw_therm2msg_tables(SW_OMS(METHOD) ? p.oms_lo[0] : p.lut_lo, SW_OMS(METHOD) ? p.oms_hi[0] : p.lut_hi, K.tm);
#define LAYER(BR) bad += layer<METHOD, BR>(r, p, K, it == 1, it, degs); rows_compared += 256;
            LAYER(0) LAYER(1) LAYER(2) LAYER(3) LAYER(4) LAYER(5) LAYER(6) LAYER(7) LAYER(8) LAYER(9) LAYER(10) LAYER(11)
#undef LAYER
        }
    }
    return bad;
}
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    for (int br = 0; br < SW50_LAYERS; ++br) {
        int deg;
        unsigned v;
        if (fscanf(f, "%d", &deg) != 1 || deg < 2 || deg > SW_MAX_DEG) return 2;
        for (int j = 0; j < deg; ++j) if (fscanf(f, "%u", &v) != 1) return 2;
    }
    int method = 0, f1 = 0, f2 = 0, n_iter = 0, n_seeds = 0;
    if (fscanf(f, "%d %d %d", &method, &f1, &f2) != 3) return 2;
    SwParams pit[6];
    memset(pit, 0, sizeof(pit));
    for (int t = 0; t < 2; ++t)
        for (int it = 0; it < 6; ++it)
            for (int e = 0; e < 8; ++e) {
                unsigned v;
                if (fscanf(f, "%u", &v) != 1 || v > 7u) return 2;
                uint32_t& w = t == 0 ? (e < 4 ? pit[it].lut_lo : pit[it].lut_hi) : (e < 4 ? pit[it].ef_lo : pit[it].ef_hi);
                w |= v << (8 * (e & 3));
            }
    for (int it = 0; it < 6; ++it) { pit[it].f1 = f1; pit[it].f2 = f2; pit[it].window = 0; pit[it].ef_tables = 0; sw_oms_tables(pit[it]); }
    long n_random = 0;
    if (fscanf(f, "%d %d %ld", &n_iter, &n_seeds, &n_random) != 3) return 2;
    fclose(f);
    Tally t;
    helper_checks(t, n_random);
    printf("helper results compared: %ld\n", t.checked);
    printf("helper mismatches: %ld\n", t.bad);
    if (t.bad) return 1;
    long rows = 0, bad = 0;
    int degs[2] = { 0, 0 };
    if (method == 2) bad = run<2>(pit, n_iter, n_seeds, rows, degs);
    else if (method == 1) bad = run<1>(pit, n_iter, n_seeds, rows, degs);
    else if (method == 5) bad = run<5>(pit, n_iter, n_seeds, rows, degs);
    else return 2;
    printf("layer runs of degree 22 / 23: %d / %d\n", degs[0], degs[1]);
    printf("rows compared: %ld\n", rows);
    printf("total mismatches: %ld\n", bad);
    return bad == 0 ? 0 : 1;
}
