/*
 * zero_shift_emul.cpp - TEST PROGRAM: the layer step of csrc/lnsfaid_swar.h compiled for the host, run over all 64 lanes of every
 * layer of a base matrix twice: with the code's own edge order and the rotating instances (what lnsfaid_kernel4.hip runs), and
 * with the zero-shift edges first and the rotation-free instances (what lnsfaid_kernel4z.hip runs).  After every layer the En
 * images must be equal byte for byte and the rows' records equal after undoing the permutation; the arg-min address is compared
 * only where the two minima of the row differ (in a tie either of the tied edges may be called the arg-min).
 *
 * Input (text, argv[1]): nbr, then per layer "deg zg" + deg entries block column * 256 + shift in the code's order + deg entries
 * order[j] (edge j of the zero-first table is edge order[j] of the row); then "method f1 f2", 6 x 8 table entries, 6 x 8
 * error-floor table entries; then "iterations seeds".  tests/test_zero_shift_cpu.py writes it.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "lnsfaid_swar.h"

namespace {
struct HostTab {
    const uint32_t* row; /* block column * 256 + shift of the layer's edges */
    uint32_t s4(int j) const { return (row[j] & 255u) << 2; }
    uint32_t cb256(int j) const { return row[j] & ~255u; }
    uint32_t sb_dyn4(uint32_t j4) const { const uint32_t v = row[j4 >> 2]; return ((v & ~255u) << 16) | ((v & 255u) << 2); }
};

struct Layer {
    int deg, zg;
    uint32_t ref[SW_MAX_DEG], zf[SW_MAX_DEG];
    int order[SW_MAX_DEG];
};

template <int METHOD>
SwRow step_rotating(const Layer& L, const SwLds& lds, const SwParams& p, const SwK& K, uint32_t lane, SwRow cur, bool fresh)
{
    HostTab tab; tab.row = L.ref;
    if (L.deg == 23) return sw_layer_step<METHOD, 23>(lds, tab, p, K, lane, 23, cur, fresh, 0u, false);
    if (L.deg == 22) return sw_layer_step<METHOD, 22>(lds, tab, p, K, lane, 22, cur, fresh, 0u, false);
    return sw_layer_step<METHOD, 0>(lds, tab, p, K, lane, L.deg, cur, fresh, 0u, false);
}

/* the instances lnsfaid_kernel4z.hip compiles; any other (degree, ZG) is a mistake of the caller's rounding */
template <int METHOD>
bool step_rotation_free(const Layer& L, const SwLds& lds, const SwParams& p, const SwK& K, uint32_t lane, SwRow cur, bool fresh, SwRow& out)
{
    HostTab tab; tab.row = L.zf;
#define WAY(D, G) if (L.deg == D && L.zg == G) { out = sw_layer_step<METHOD, D, false, 1, 0, G>(lds, tab, p, K, lane, D, cur, fresh, 0u, false); return true; }
    WAY(23, 0) WAY(23, 1) WAY(23, 2) WAY(23, 4) WAY(22, 0) WAY(22, 5)
#undef WAY
    if (L.deg == 23 || L.deg == 22 || L.zg != 0) return false;
    out = sw_layer_step<METHOD, 0>(lds, tab, p, K, lane, L.deg, cur, fresh, 0u, false);
    return true;
}

uint32_t node_pos(uint32_t sb, uint32_t lane, int k) { return sw_en_pos((sb & ~255u) + (((sb & 255u) + lane + 64u * (uint32_t)k) & 255u)); }

/* the two minima of row (lane, k) differ: levels min(|En - Lold|, 7) over the row's edges, from the true image and the record */
bool unique_minimum(const Layer& L, const uint8_t* img, const SwRow& cur, bool fresh, uint32_t lane, int k)
{
    const int c2 = (int)((cur.cw >> (8 * k)) & 7u), c1 = (int)((cur.cw >> (8 * k + 3)) & 7u);
    const bool negA = ((cur.cw >> (8 * k + 6)) & 1u) != 0u;
    const uint32_t pold = (k & 1) ? cur.pa[k >> 1] >> 16 : cur.pa[k >> 1] & 0xffffu;
    int best = 8, count = 0;
    for (int j = 0; j < L.deg; ++j) {
        const uint32_t a = node_pos(L.ref[j], lane, k);
        int l = 0;
        if (!fresh) {
            const bool neg = ((cur.x[j >> 3] >> (8 * k + (j & 7))) & 1u) != 0u;
            l = a == pold ? (negA ? -c1 : c1) : (neg ? -c2 : c2);
        }
        int t = (int)img[a] - SW_BIAS_EN - l;
        t = t < 0 ? -t : t;
        if (t > 7) t = 7;
        if (t < best) { best = t; count = 1; } else if (t == best) ++count;
    }
    return count == 1;
}

template <int METHOD>
long run(const std::vector<Layer>& layers, const SwParams pit[6], int n_iter, int n_seeds, size_t img_bytes, long& rows_compared, long& ties)
{
    long bad = 0;
    const SwK K = sw_consts();
    for (int seed = 0; seed < n_seeds; ++seed) {
        std::vector<uint8_t> a(img_bytes), b;
        uint32_t s = 12345u + 977u * (uint32_t)seed;
        const int amp = (seed & 1) ? 31 : 7; /* channel-like values and the whole range of En */
        for (auto& x : a) { s = s * 1664525u + 1013904223u; x = (uint8_t)(SW_BIAS_EN + (int)((s >> 16) % (uint32_t)(2 * amp + 1)) - amp); }
        b = a;
        SwLds la, lb; la.base = a.data(); lb.base = b.data();
        std::vector<SwRow> ra(layers.size() * 64), rb(layers.size() * 64);
        memset(ra.data(), 0, ra.size() * sizeof(SwRow));
        memset(rb.data(), 0, rb.size() * sizeof(SwRow));
        for (int it = 1; it <= n_iter; ++it) {
            const bool fresh = it == 1;
            const SwParams& p = pit[it <= 5 ? it - 1 : 5];
            for (size_t br = 0; br < layers.size(); ++br) {
                const Layer& L = layers[br];
                const std::vector<uint8_t> before = a;
                for (uint32_t lane = 0; lane < 64; ++lane) {
                    const SwRow old = ra[br * 64 + lane];
                    ra[br * 64 + lane] = step_rotating<METHOD>(L, la, p, K, lane, old, fresh);
                    SwRow nw;
                    if (!step_rotation_free<METHOD>(L, lb, p, K, lane, rb[br * 64 + lane], fresh, nw)) { printf("no instance (%d, %d)\n", L.deg, L.zg); return -1; }
                    rb[br * 64 + lane] = nw;
                    const SwRow& x = ra[br * 64 + lane];
                    /* the record: sign bits through the permutation, magnitudes, and the arg-min where it is unique */
                    uint32_t back[3] = { 0u, 0u, 0u };
                    for (int j = 0; j < L.deg; ++j)
                        for (int k = 0; k < 4; ++k)
                            if ((nw.x[j >> 3] >> (8 * k + (j & 7))) & 1u) back[L.order[j] >> 3] |= 1u << (8 * k + (L.order[j] & 7));
                    if (back[0] != x.x[0] || back[1] != x.x[1] || back[2] != x.x[2]) { if (bad++ < 8) printf("it %d layer %zu lane %u: sign words differ\n", it, br, lane); }
                    if ((nw.cw & 0x3f3f3f3fu) != (x.cw & 0x3f3f3f3fu)) { if (bad++ < 8) printf("it %d layer %zu lane %u: magnitudes differ\n", it, br, lane); }
                    for (int k = 0; k < 4; ++k) {
                        ++rows_compared;
                        if (!unique_minimum(L, before.data(), old, fresh, lane, k)) { ++ties; continue; }
                        const uint32_t pa_a = (k & 1) ? x.pa[k >> 1] >> 16 : x.pa[k >> 1] & 0xffffu;
                        const uint32_t pa_b = (k & 1) ? nw.pa[k >> 1] >> 16 : nw.pa[k >> 1] & 0xffffu;
                        if (pa_a != pa_b || ((nw.cw ^ x.cw) >> (8 * k + 6)) & 1u) { if (bad++ < 8) printf("it %d layer %zu lane %u row %d: arg-min differs\n", it, br, lane, k); }
                    }
                }
                if (a != b) { if (bad++ < 8) printf("it %d layer %zu: En images differ\n", it, br); b = a; }
            }
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
    int nbr = 0;
    if (fscanf(f, "%d", &nbr) != 1 || nbr < 1) return 2;
    std::vector<Layer> layers((size_t)nbr);
    uint32_t max_cb = 0;
    for (auto& L : layers) {
        if (fscanf(f, "%d %d", &L.deg, &L.zg) != 2 || L.deg < 2 || L.deg > SW_MAX_DEG) return 2;
        for (int j = 0; j < L.deg; ++j) { if (fscanf(f, "%u", &L.ref[j]) != 1) return 2; if (L.ref[j] / 256u > max_cb) max_cb = L.ref[j] / 256u; }
        for (int j = 0; j < L.deg; ++j) { if (fscanf(f, "%d", &L.order[j]) != 1 || L.order[j] < 0 || L.order[j] >= L.deg) return 2; L.zf[j] = L.ref[L.order[j]]; }
        for (int j = 0; j < 4 * L.zg; ++j) if (L.zf[j] & 255u) { printf("layer claims %d rotation-free groups, edge %d has a shift\n", L.zg, j); return 1; }
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
    long rows = 0, ties = 0, bad;
    const size_t img = ((size_t)max_cb + 1) * 256;
    if (method == 2) bad = run<2>(layers, pit, n_iter, n_seeds, img, rows, ties);
    else if (method == 1) bad = run<1>(layers, pit, n_iter, n_seeds, img, rows, ties);
    else if (method == 5) bad = run<5>(layers, pit, n_iter, n_seeds, img, rows, ties);
    else return 2;
    printf("rows compared: %ld, ties: %ld\n", rows, ties);
    printf("total mismatches: %ld\n", bad);
    return bad == 0 ? 0 : 1;
}
