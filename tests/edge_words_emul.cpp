/*
 * edge_words_emul.cpp - TEST PROGRAM: the edge words of csrc/lnsfaid_static50.h and the layer step of csrc/lnsfaid_swar.h that takes
 * them (SW_FORM_EDGEW), compiled for the host.
 *
 *   edge_words_emul dump <words.bin> <image.bin>
 *       writes sw50_edge_word(layer, edge, lane) of every rotating edge - layer by layer, edge by edge in Sw50Tab's order, lanes 0..63 -
 *       preceded by one line per layer on stdout ("layer deg nz"), and the memory image sw50_edge_image() as the kernel loads it.
 *   edge_words_emul step <spec.txt>
 *       runs sw_layer_step over all 64 lanes of every layer twice, in the forms lnsfaid_kernel4w.hip compiles (first iteration, later
 *       ones) and in the same forms with SW_FORM_EDGEW on top, the words read from the image at the place lnsfaid_kernel4e.hip reads
 *       them; after every layer the En images and the rows' records must be equal byte for byte.  spec.txt: "method f1 f2", 6 x 8
 *       table entries, "iterations seeds" (tests/test_edge_words_cpu.py writes it).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "lnsfaid_static50.h"

namespace {
const Sw50EdgeImage g_image = sw50_edge_image();

/* the words of layer BR for one lane, where the kernel finds them: [group base + e / 4][lane][e % 4] */
template <int BR>
struct HostEw {
    uint32_t lane;
    uint32_t w(int j) const
    {
        const int e = j - Sw50Tab<BR>::NZ;
        return g_image.w[((sw50_edge_group_base(BR) + e / 4) * 64 + (int)lane) * 4 + e % 4];
    }
    uint32_t wa(int j) const { return w(j); }
    void at(int) const {}
};

constexpr int BASE = SW_FORM_NOWIN | SW_FORM_VK | SW_FORM_MUL;

template <int METHOD, int FORM, int BR>
long layer(std::vector<uint8_t>& a, std::vector<uint8_t>& b, SwRow* ra, SwRow* rb, const SwParams& p, const SwK& K, bool fresh, int it)
{
    typedef Sw50Tab<BR> Tab;
    long bad = 0;
    SwLds la, lb; la.base = a.data(); lb.base = b.data();
    for (uint32_t lane = 0; lane < 64; ++lane) {
        Tab t; t.sbv = 0u;
        const HostEw<BR> ew = { lane };
        ra[lane] = sw_layer_step<METHOD, Tab::DEG, false, 1, 0, 0, SW_PAIRS_ALL, FORM>(la, t, p, K, lane << 2, Tab::DEG, ra[lane], fresh, 0u, false);
        rb[lane] = sw_layer_step<METHOD, Tab::DEG, false, 1, 0, 0, SW_PAIRS_ALL, FORM | SW_FORM_EDGEW>(lb, t, p, K, lane << 2, Tab::DEG, rb[lane], fresh, 0u, false,
                                                                                                     0u, 0u, SwNoXch(), ew);
        if (memcmp(&ra[lane], &rb[lane], sizeof(SwRow)) != 0) { if (bad++ < 8) printf("it %d layer %d lane %u: records differ\n", it, BR, lane); rb[lane] = ra[lane]; }
    }
    if (a != b) { if (bad++ < 8) printf("it %d layer %d: En images differ\n", it, BR); b = a; }
    return bad;
}

template <int METHOD>
long run(const SwParams pit[6], int n_iter, int n_seeds, long& rows_compared)
{
    long bad = 0;
    for (int seed = 0; seed < n_seeds; ++seed) {
        std::vector<uint8_t> a(69 * 256), b;
        uint32_t s = 8765u + 991u * (uint32_t)seed;
        const int amp = (seed & 1) ? 31 : 7; /* channel-like values and the whole range of En */
        for (auto& x : a) { s = s * 1664525u + 1013904223u; x = (uint8_t)(SW_BIAS_EN + (int)((s >> 16) % (uint32_t)(2 * amp + 1)) - amp); }
        b = a;
        std::vector<SwRow> ra(SW50_LAYERS * 64), rb(SW50_LAYERS * 64);
        memset(ra.data(), 0, ra.size() * sizeof(SwRow));
        memset(rb.data(), 0, rb.size() * sizeof(SwRow));
        for (int it = 1; it <= n_iter; ++it) {
            SwParams p = pit[it <= 5 ? it - 1 : 5];
            SwK K = sw_consts();
            sw_therm2msg_tables(SW_OMS(METHOD) ? p.oms_lo[0] : p.lut_lo, SW_OMS(METHOD) ? p.oms_hi[0] : p.lut_hi, K.tm);
#define LAYER(BR)                                                                                                                 \
    bad += it == 1 ? layer<METHOD, BASE | SW_FORM_FRESH, BR>(a, b, &ra[BR * 64], &rb[BR * 64], p, K, true, it)                     \
                   : layer<METHOD, BASE, BR>(a, b, &ra[BR * 64], &rb[BR * 64], p, K, false, it);                                  \
    rows_compared += 256;
            LAYER(0) LAYER(1) LAYER(2) LAYER(3) LAYER(4) LAYER(5) LAYER(6) LAYER(7) LAYER(8) LAYER(9) LAYER(10) LAYER(11)
#undef LAYER
        }
    }
    return bad;
}

int dump(const char* words_path, const char* image_path)
{
    const Sw50Code c = sw50_build();
    FILE* fw = fopen(words_path, "wb");
    FILE* fi = fopen(image_path, "wb");
    if (!fw || !fi) return 2;
    for (int br = 0; br < SW50_LAYERS; ++br) {
        printf("%d %d %d\n", br, c.layer[br].deg, c.layer[br].nz);
        for (int j = c.layer[br].nz; j < c.layer[br].deg; ++j)
            for (int lane = 0; lane < 64; ++lane) {
                const uint32_t w = sw50_edge_word(br, j, lane);
                fwrite(&w, 4, 1, fw);
            }
    }
    fwrite(g_image.w, 4, sizeof(g_image.w) / 4, fi);
    fclose(fw); fclose(fi);
    return 0;
}
}

int main(int argc, char** argv)
{
    if (argc == 4 && !strcmp(argv[1], "dump")) return dump(argv[2], argv[3]);
    if (argc != 3 || strcmp(argv[1], "step")) return 2;
    FILE* f = fopen(argv[2], "r");
    if (!f) return 2;
    int method = 0, f1 = 0, f2 = 0, n_iter = 0, n_seeds = 0;
    if (fscanf(f, "%d %d %d", &method, &f1, &f2) != 3) return 2;
    SwParams pit[6];
    memset(pit, 0, sizeof(pit));
    for (int it = 0; it < 6; ++it)
        for (int e = 0; e < 8; ++e) {
            unsigned v;
            if (fscanf(f, "%u", &v) != 1 || v > 7u) return 2;
            (e < 4 ? pit[it].lut_lo : pit[it].lut_hi) |= v << (8 * (e & 3));
        }
    for (int it = 0; it < 6; ++it) { pit[it].f1 = f1; pit[it].f2 = f2; pit[it].window = 0; pit[it].ef_tables = 0; sw_oms_tables(pit[it]); }
    if (fscanf(f, "%d %d", &n_iter, &n_seeds) != 2) return 2;
    fclose(f);
    long rows = 0, bad;
    if (method == 2) bad = run<2>(pit, n_iter, n_seeds, rows);
    else if (method == 1) bad = run<1>(pit, n_iter, n_seeds, rows);
    else if (method == 5) bad = run<5>(pit, n_iter, n_seeds, rows);
    else return 2;
    printf("rows compared: %ld\n", rows);
    printf("total mismatches: %ld\n", bad);
    return bad == 0 ? 0 : 1;
}
