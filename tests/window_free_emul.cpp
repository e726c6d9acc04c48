/*
 * window_free_emul.cpp - TEST PROGRAM: the iteration forms of the layer step (FORM of sw_layer_step, csrc/lnsfaid_swar.h: what
 * main_step4w of lnsfaid_kernel4w.hip instantiates) compiled for the host, against the step every other kernel runs.
 *
 *  - composed tables: for every table given and every thermometer code the minimum search can hold (0x00 0x01 0x03 0x07 0x0f 0x1f
 *    0x3f 0xff and 0x7f, which decodes like the saturated one), in every byte, sw_therm2msg equals LUT[sw_therm2num];
 *  - three runs of all 64 lanes of every layer of the 50G-PON code side by side, from the same En image: the generic instance
 *    (FORM 0) called with rowpar = 0, lme = false, window = false; the SW_FORM_NOWIN instance with `fresh` a run-time value; and the
 *    forms the kernel picks (SW_FORM_NOWIN | SW_FORM_FRESH in iteration 1, which gets a record of garbage to show that it is not
 *    read, SW_FORM_NOWIN afterwards).  After every layer the three En images and the rows' records must be equal byte for byte.
 *    Random images over the channel's range and over the whole range of En, and images of corner values only.
 *
 * Input (text, argv[1]) as tests/static_layers_emul.cpp; tests/test_window_free_step_cpu.py writes it.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "lnsfaid_static50.h"

namespace {
bool same(const SwRow& a, const SwRow& b) { return memcmp(&a, &b, sizeof(SwRow)) == 0; }

const uint32_t kCodes[9] = { 0x00u, 0x01u, 0x03u, 0x07u, 0x0fu, 0x1fu, 0x3fu, 0xffu, 0x7fu };

/* every code in every byte, the other bytes running through the codes too */
long table_checks(uint32_t lut_lo, uint32_t lut_hi, long& checked)
{
    long bad = 0;
    uint32_t tm[4];
    sw_therm2msg_tables(lut_lo, lut_hi, tm);
    const uint64_t lut = ((uint64_t)lut_hi << 32) | lut_lo;
    for (int k = 0; k < 4; ++k)
        for (int ci = 0; ci < 9; ++ci)
            for (int other = 0; other < 9; ++other) {
                uint32_t x = 0;
                for (int b = 0; b < 4; ++b) x |= (b == k ? kCodes[ci] : kCodes[(other + b) % 9]) << (8 * b);
                const uint32_t n = sw_therm2num(x, SW_T2N_LO, SW_T2N_HI);
                uint32_t want = 0;
                for (int b = 0; b < 4; ++b) want |= (uint32_t)((lut >> (8 * ((n >> (8 * b)) & 0xffu))) & 0xffu) << (8 * b);
                ++checked;
                if (sw_therm2msg(x, tm) != want && bad++ < 8) printf("table %08x %08x code word %08x: %08x, wanted %08x\n", lut_lo, lut_hi, x, sw_therm2msg(x, tm), want);
            }
    return bad;
}

struct Run {
    std::vector<uint8_t> en;
    std::vector<SwRow> rec;
};

template <int METHOD, int BR>
long layer(Run& g, Run& w, Run& k, const SwParams& p, const SwK& K, const SwK& Kw, bool fresh, int it)
{
    typedef Sw50Tab<BR> Tab;
    long bad = 0;
    SwLds lg, lw, lk; lg.base = g.en.data(); lw.base = w.en.data(); lk.base = k.en.data();
    for (uint32_t lane = 0; lane < 64; ++lane) {
        Tab tab; tab.sbv = 0u;
        SwRow* rg = &g.rec[BR * 64 + lane], *rw = &w.rec[BR * 64 + lane], *rk = &k.rec[BR * 64 + lane];
        *rg = sw_layer_step<METHOD, Tab::DEG, false, 1, 0, 0, SW_PAIRS_ALL>(lg, tab, p, K, lane, Tab::DEG, *rg, fresh, 0u, false);
        *rw = sw_layer_step<METHOD, Tab::DEG, false, 1, 0, 0, SW_PAIRS_ALL, SW_FORM_NOWIN>(lw, tab, p, Kw, lane, Tab::DEG, *rw, fresh, 0xffffffffu, true);
        if (fresh) {
            SwRow junk;
            memset(&junk, 0xa5, sizeof(junk)); /* the form may not look at the record */
            *rk = sw_layer_step<METHOD, Tab::DEG, false, 1, 0, 0, SW_PAIRS_ALL, SW_FORM_NOWIN | SW_FORM_FRESH>(lk, tab, p, Kw, lane, Tab::DEG, junk, true, 0xffffffffu, true);
        } else {
            *rk = sw_layer_step<METHOD, Tab::DEG, false, 1, 0, 0, SW_PAIRS_ALL, SW_FORM_NOWIN>(lk, tab, p, Kw, lane, Tab::DEG, *rk, false, 0xffffffffu, true);
        }
        if (!same(*rg, *rw)) { if (bad++ < 8) printf("it %d layer %d lane %u: NOWIN record differs\n", it, BR, lane); *rw = *rg; }
        if (!same(*rg, *rk)) { if (bad++ < 8) printf("it %d layer %d lane %u: kernel form's record differs\n", it, BR, lane); *rk = *rg; }
    }
    if (g.en != w.en) { if (bad++ < 8) printf("it %d layer %d: NOWIN En image differs\n", it, BR); w.en = g.en; }
    if (g.en != k.en) { if (bad++ < 8) printf("it %d layer %d: kernel form's En image differs\n", it, BR); k.en = g.en; }
    return bad;
}

template <int METHOD>
long run(const SwParams pit[6], int n_iter, int n_seeds, long& rows_compared)
{
    long bad = 0;
    const SwK K = sw_consts();
    static const int corner[8] = { -31, -30, -8, -1, 0, 1, 7, 31 };
    for (int seed = 0; seed < n_seeds; ++seed) {
        Run g, w, k;
        g.en.resize(69 * 256);
        uint32_t s = 4321u + 977u * (uint32_t)seed;
        const int kind = seed % 3; /* channel-like values, the whole range of En, corner values only */
        const int amp = kind == 0 ? 7 : 31;
        for (auto& x : g.en) {
            s = s * 1664525u + 1013904223u;
            const int v = kind == 2 ? corner[(s >> 16) & 7u] : (int)((s >> 16) % (uint32_t)(2 * amp + 1)) - amp;
            x = (uint8_t)(SW_BIAS_EN + v);
        }
        g.rec.resize(SW50_LAYERS * 64);
        memset(g.rec.data(), 0, g.rec.size() * sizeof(SwRow));
        w = g; k = g;
        for (int it = 1; it <= n_iter; ++it) {
            SwParams p = pit[it <= 5 ? it - 1 : 5];
            p.window = 0;
            SwK Kw = K; /* the window-free forms' constants: the iteration's table composed with the thermometer decode */
            sw_therm2msg_tables(SW_OMS(METHOD) ? p.oms_lo[0] : p.lut_lo, SW_OMS(METHOD) ? p.oms_hi[0] : p.lut_hi, Kw.tm);
#define LAYER(BR) bad += layer<METHOD, BR>(g, w, k, p, K, Kw, it == 1, it); rows_compared += 256;
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
    for (int br = 0; br < SW50_LAYERS; ++br) { /* the edge tables: the compile-time view needs none of them (tests/test_static_layers_cpu.py compares them) */
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
    if (fscanf(f, "%d %d", &n_iter, &n_seeds) != 2) return 2;
    fclose(f);
    long bad = 0, checked = 0;
    for (int it = 0; it < 6; ++it) {
        bad += table_checks(pit[it].lut_lo, pit[it].lut_hi, checked);
        bad += table_checks(pit[it].ef_lo, pit[it].ef_hi, checked);
    }
    bad += table_checks(pit[0].oms_lo[0], pit[0].oms_hi[0], checked);
    bad += table_checks(pit[0].oms_lo[1], pit[0].oms_hi[1], checked);
    bad += table_checks(0x03020100u, 0x07060504u, checked); /* the identity: sw_therm2num itself */
    bad += table_checks(0x04050607u, 0x00010203u, checked); /* (not a decoder's table: every entry differs from its neighbours') */
    printf("table look-ups compared: %ld\n", checked);
    printf("table mismatches: %ld\n", bad);
    if (bad) return 1;
    long rows = 0;
    if (method == 2) bad = run<2>(pit, n_iter, n_seeds, rows);
    else if (method == 1) bad = run<1>(pit, n_iter, n_seeds, rows);
    else if (method == 5) bad = run<5>(pit, n_iter, n_seeds, rows);
    else return 2;
    printf("rows compared: %ld\n", rows);
    printf("total mismatches: %ld\n", bad);
    return bad == 0 ? 0 : 1;
}
