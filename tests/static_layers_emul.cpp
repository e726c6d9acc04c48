/*
 * static_layers_emul.cpp - TEST PROGRAM: the layer step of csrc/lnsfaid_swar.h compiled for the host, run over all 64 lanes of every
 * layer of the 50G-PON code twice: through the compile-time table view of the layer-static kernel (Sw50Tab<BR>,
 * csrc/lnsfaid_static50.h: what main_step4s of lnsfaid_kernel4s.hip runs) and through a run-time view of the zero-first tables the
 * library builds (LfDevCode zs4tab / zcbtab, rotating instance).  The edge order is the same on both sides, so after every layer the
 * En images and the rows' records must be equal byte for byte, arg-min addresses included.  The compile-time constants themselves
 * are compared with the library's tables entry by entry first.
 *
 * Input (text, argv[1]): 12 lines "deg" + deg entries block column * 256 + shift in the zero-first order; then "method f1 f2",
 * 6 x 8 table entries, 6 x 8 error-floor table entries; then "iterations seeds".  tests/test_static_layers_cpu.py writes it.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "lnsfaid_static50.h"

namespace {
struct HostTab {
    const uint32_t* row; /* block column * 256 + shift of the layer's edges */
    uint32_t s4(int j) const { return (row[j] & 255u) << 2; }
    uint32_t cb256(int j) const { return row[j] & ~255u; }
    uint32_t sb_dyn4(uint32_t j4) const { const uint32_t v = row[j4 >> 2]; return ((v & ~255u) << 16) | ((v & 255u) << 2); }
};

struct Layer {
    int deg;
    uint32_t zf[SW_MAX_DEG];
};

bool same(const SwRow& a, const SwRow& b) { return memcmp(&a, &b, sizeof(SwRow)) == 0; }

/* one layer, all lanes, both ways; returns the number of mismatches */
template <int METHOD, int BR>
long layer(const Layer& L, std::vector<uint8_t>& a, std::vector<uint8_t>& b, SwRow* ra, SwRow* rb, const SwParams& p, const SwK& K, bool fresh,
           uint32_t rowpar, bool lme, int it)
{
    typedef Sw50Tab<BR> Tab;
    long bad = 0;
    SwLds la, lb; la.base = a.data(); lb.base = b.data();
    for (uint32_t lane = 0; lane < 64; ++lane) {
        HostTab ht; ht.row = L.zf;
        Tab st; st.sbv = 0u;
        const uint32_t par = rowpar & (lane % 3 == 0 ? 0u : (lane & 1) ? 0x00ff00ffu : 0xffff0000u); /* some rows unsatisfied */
        ra[lane] = sw_layer_step<METHOD, Tab::DEG>(la, ht, p, K, lane, Tab::DEG, ra[lane], fresh, par, lme);
        rb[lane] = sw_layer_step<METHOD, Tab::DEG>(lb, st, p, K, lane, Tab::DEG, rb[lane], fresh, par, lme);
        if (!same(ra[lane], rb[lane])) { if (bad++ < 8) printf("it %d layer %d lane %u: records differ\n", it, BR, lane); rb[lane] = ra[lane]; }
    }
    if (a != b) { if (bad++ < 8) printf("it %d layer %d: En images differ\n", it, BR); b = a; }
    return bad;
}

template <int BR>
long constants(const Layer& L)
{
    typedef Sw50Tab<BR> Tab;
    long bad = 0;
    if (L.deg != Tab::DEG) { printf("layer %d: degree %d, compiled %d\n", BR, L.deg, Tab::DEG); return 1; }
    Tab t; t.sbv = 0u;
    int nz = 0;
    while (nz < L.deg && (L.zf[nz] & 255u) == 0u) ++nz;
    if (nz != Tab::NZ) { printf("layer %d: %d identity edges, compiled %d\n", BR, nz, Tab::NZ); ++bad; }
    for (int j = 0; j < L.deg; ++j)
        if (t.s4(j) != (L.zf[j] & 255u) << 2 || t.cb256(j) != (L.zf[j] & ~255u) || t.sb_dyn4(4u * (uint32_t)j) != (((L.zf[j] & ~255u) << 16) | ((L.zf[j] & 255u) << 2))) {
            printf("layer %d edge %d: compiled (%u, %u), library %u\n", BR, j, t.cb256(j), t.s4(j), L.zf[j]); ++bad;
        }
    return bad;
}

template <int METHOD>
long run(const std::vector<Layer>& layers, const SwParams pit[6], int n_iter, int n_seeds, long& rows_compared)
{
    long bad = 0;
    const SwK K = sw_consts();
    for (int seed = 0; seed < n_seeds; ++seed) {
        std::vector<uint8_t> a(69 * 256), b;
        uint32_t s = 4321u + 977u * (uint32_t)seed;
        const int amp = (seed & 1) ? 31 : 7; /* channel-like values and the whole range of En */
        for (auto& x : a) { s = s * 1664525u + 1013904223u; x = (uint8_t)(SW_BIAS_EN + (int)((s >> 16) % (uint32_t)(2 * amp + 1)) - amp); }
        b = a;
        std::vector<SwRow> ra(SW50_LAYERS * 64), rb(SW50_LAYERS * 64);
        memset(ra.data(), 0, ra.size() * sizeof(SwRow));
        memset(rb.data(), 0, rb.size() * sizeof(SwRow));
        for (int it = 1; it <= n_iter; ++it) {
            const bool fresh = it == 1;
            SwParams p = pit[it <= 5 ? it - 1 : 5];
            /* the last iteration inside the error-floor window with unsatisfied rows: the second tables of DecodeMethods 1 and 5 */
            const bool win = it == n_iter;
            p.window = win;
            const uint32_t rowpar = win ? 0xffffffffu : 0u;
#define LAYER(BR) bad += layer<METHOD, BR>(layers[BR], a, b, &ra[BR * 64], &rb[BR * 64], p, K, fresh, rowpar, win, it); rows_compared += 256;
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
    std::vector<Layer> layers(SW50_LAYERS);
    for (auto& L : layers) {
        if (fscanf(f, "%d", &L.deg) != 1 || L.deg < 2 || L.deg > SW_MAX_DEG) return 2;
        for (int j = 0; j < L.deg; ++j) if (fscanf(f, "%u", &L.zf[j]) != 1 || L.zf[j] >= 69u * 256u) return 2;
    }
    long bad = 0;
#define CONSTANTS(BR) bad += constants<BR>(layers[BR]);
    CONSTANTS(0) CONSTANTS(1) CONSTANTS(2) CONSTANTS(3) CONSTANTS(4) CONSTANTS(5) CONSTANTS(6) CONSTANTS(7) CONSTANTS(8) CONSTANTS(9) CONSTANTS(10) CONSTANTS(11)
#undef CONSTANTS
    printf("table mismatches: %ld\n", bad);
    if (bad) return 1;
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
    long rows = 0;
    if (method == 2) bad = run<2>(layers, pit, n_iter, n_seeds, rows);
    else if (method == 1) bad = run<1>(layers, pit, n_iter, n_seeds, rows);
    else if (method == 5) bad = run<5>(layers, pit, n_iter, n_seeds, rows);
    else return 2;
    printf("rows compared: %ld\n", rows);
    printf("total mismatches: %ld\n", bad);
    return bad == 0 ? 0 : 1;
}
