/*
 * swar_helpers_exhaustive.cpp — TEST INFRASTRUCTURE (compiled by tests/test_swar_helpers_exhaustive.py with g++): every helper of
 * csrc/lnsfaid_swar.h that was rewritten for a lower instruction count against the formulation it replaced, over the whole input
 * domain of a byte, in every byte position, with the other three bytes of the dword filled with other members of the domain (a
 * carry or borrow across bytes would show there).  Prints one line per check and returns non-zero on any mismatch.
 */
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "lnsfaid_swar.h"

namespace {
uint32_t rng_state = 0x2545f491u;
uint32_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5;
    return rng_state;
}
const uint32_t CODES[8] = { 0x00, 0x01, 0x03, 0x07, 0x0f, 0x1f, 0x3f, 0xff }; /* thermometer codes of 0..7 (7: the saturated selector's 0xff) */
uint32_t rnd_codes()
{
    uint32_t x = 0;
    for (int k = 0; k < 4; ++k) x |= CODES[rnd() & 7] << (8 * k);
    return x;
}

/* ---- thermometer code -> number: all 8^4 dwords ---- */
long check_therm2num()
{
    const SwK K = sw_consts();
    long bad = 0, n = 0;
    for (int i = 0; i < 8 * 8 * 8 * 8; ++i) {
        uint32_t x = 0, want = 0;
        for (int k = 0; k < 4; ++k) {
            const int v = (i >> (3 * k)) & 7;
            x |= CODES[v] << (8 * k);
            want |= (uint32_t)v << (8 * k);
        }
        if (sw_popcount7(x) != want) ++bad; /* the definition itself */
        if (sw_therm2num(x, K.n_lo, K.n_hi) != want) ++bad;
        ++n;
    }
    printf("therm2num: %ld dwords, %ld mismatches\n", n, bad);
    return bad;
}

/* ---- clamp / update of one edge ---- */
struct EdgeIn {
    int t, c, b, f; /* V2C, new magnitude, old message negative, row mask F */
};
template <bool MINSUM>
long check_update()
{
    const SwK K = sw_consts();
    const uint32_t bias = MINSUM ? 0u : 0x06040200u;
    std::vector<EdgeIn> dom;
    for (int t = -38; t <= 38; ++t)
        for (int c = 0; c < 8; ++c)
            for (int b = 0; b < 2; ++b)
                for (int f = 0; f < 2; ++f) dom.push_back(EdgeIn{ t, c, b, f });
    long bad = 0, n = 0;
    for (int pos = 0; pos < 4; ++pos)
        for (size_t i = 0; i < dom.size(); ++i)
            for (int rep = 0; rep < 24; ++rep) {
                EdgeIn e[4];
                for (int k = 0; k < 4; ++k) {
                    if (k == pos || rep == 0) e[k] = dom[i];                             /* rep 0: all four rows alike */
                    else if (rep == 1) e[k] = EdgeIn{ 38, 7, 0, dom[i].f ^ 1 };           /* neighbours at the ends of the domain */
                    else if (rep == 2) e[k] = EdgeIn{ -38, 7, 1, dom[i].f };
                    else if (rep == 3) e[k] = EdgeIn{ -38, 0, 0, 1 };
                    else e[k] = dom[rnd() % dom.size()];
                }
                uint32_t tb = 0, ms = 0, c = 0, fm = 0;
                for (int k = 0; k < 4; ++k) {
                    const uint32_t tbk = (uint32_t)(e[k].t + 128) + ((bias >> (8 * k)) & 0xffu);                 /* what pass 1 leaves: t + 128 (+ bias) */
                    const uint32_t tsk = MINSUM ? (uint32_t)(e[k].t + 128) : (uint32_t)(e[k].t + 128 - e[k].b);   /* plain / back-tracked sign */
                    tb |= tbk << (8 * k);
                    ms |= (tsk & 0x80u) ? 0xffu << (8 * k) : 0u;
                    c |= (uint32_t)e[k].c << (8 * k);
                    fm |= e[k].f ? 0xffu << (8 * k) : 0u;
                }
                const uint32_t want = sw_update<MINSUM>(tb, ms, sw_update_consts<MINSUM>(c, fm, bias), K.sel_sign, K.cbit[7]);
                const uint32_t got = sw_update2<MINSUM>(tb, ms, sw_update2_consts<MINSUM>(c, fm, bias), K.sel_sign, K.cbit[7], K.cm27);
                if (got != want) {
                    if (bad < 5) printf("  update<%d>: tb %08x ms %08x c %08x fm %08x: %08x, expected %08x\n", (int)MINSUM, tb, ms, c, fm, got, want);
                    ++bad;
                }
                /* and against the decoder's own statement for the byte under test: sat31(tc + L) + 120, tc = sat31(t) (FAID) or
                 * max(t, -31) (min-sum) */
                {
                    const EdgeIn& x = e[pos];
                    const bool positive = ((((ms >> (8 * pos)) & 0xffu) != 0) != (x.f != 0));
                    const int L = positive ? x.c : -x.c;
                    int tc = x.t < -31 ? -31 : x.t;
                    if (!MINSUM && tc > 31) tc = 31;
                    int en = tc + L;
                    en = en < -31 ? -31 : (en > 31 ? 31 : en);
                    if (((got >> (8 * pos)) & 0xffu) != (uint32_t)(en + SW_BIAS_EN)) {
                        if (bad < 5) printf("  update<%d>: t %d c %d b %d f %d: byte %02x, statement %02x\n", (int)MINSUM, x.t, x.c, x.b, x.f, (got >> (8 * pos)) & 0xffu, en + SW_BIAS_EN);
                        ++bad;
                    }
                }
                ++n;
            }
    printf("update<%s>: %ld dwords (%zu cases per byte x 4 positions x 24 neighbourhoods), %ld mismatches\n", MINSUM ? "min-sum" : "FAID", n, dom.size(), bad);
    return bad;
}

/* ---- minimum search: a group of four edges merged at once against the edge-by-edge chain ---- */
bool same_min(uint32_t a1, uint32_t a2, const uint32_t* aa, uint32_t b1, uint32_t b2, const uint32_t* ba)
{
    bool ok = a1 == b1 && a2 == b2;
    for (int b = 0; b < 5; ++b) ok = ok && aa[b] == ba[b];
    return ok;
}
long check_min_quad()
{
    long bad = 0, n = 0;
    /* byte 0: every running pair (t1 <= t2) with every four codes; bytes 1..3: other cases */
    for (int a = 0; a < 8; ++a)
        for (int b = a; b < 8; ++b)
            for (int u = 0; u < 4096; ++u)
                for (int j0 = 0; j0 < 24; j0 += 4) {
                    uint32_t t1 = rnd_codes(), t2 = 0, v[4], ta[5];
                    for (int k = 1; k < 4; ++k) { const uint32_t lo = (t1 >> (8 * k)) & 0xffu, hi = CODES[rnd() & 7]; t2 |= (lo | hi) << (8 * k); } /* t2 >= t1 */
                    t1 = (t1 & ~0xffu) | CODES[a]; t2 |= CODES[b];
                    for (int g = 0; g < 4; ++g) v[g] = (rnd_codes() & ~0xffu) | CODES[(u >> (3 * g)) & 7];
                    for (int i = 0; i < 5; ++i) ta[i] = rnd_codes();
                    uint32_t w1 = t1, w2 = t2, wa[5], g1 = t1, g2 = t2, ga[5];
                    for (int i = 0; i < 5; ++i) wa[i] = ga[i] = ta[i];
                    for (int g = 0; g < 4; ++g) sw_min_edge(w1, w2, wa, v[g], j0 + g);
                    sw_min_quad(g1, g2, ga, v[0], v[1], v[2], v[3], j0);
                    if (!same_min(w1, w2, wa, g1, g2, ga)) {
                        if (bad < 5) printf("  min: j0 %d t1 %08x t2 %08x v %08x %08x %08x %08x: (%08x, %08x), expected (%08x, %08x)\n", j0, t1, t2, v[0], v[1], v[2], v[3], g1, g2, w1, w2);
                        ++bad;
                    }
                    ++n;
                }
    printf("min_quad: %ld dwords (36 running pairs x 8^4 codes x 6 groups), %ld mismatches\n", n, bad);
    return bad;
}

/* ---- sign words of pass 2: four masks at a time against one at a time, every combination of the 23 / 22 / 24 masks of a row
 * being 0x00 or 0xff is too many, so: every combination inside each group of eight (2^8) per byte, other groups random ---- */
template <int NJ>
long check_sign_quad()
{
    const SwK K = sw_consts();
    long bad = 0, n = 0;
    for (int w = 0; w < 3; ++w)
        for (int pat = 0; pat < 256; ++pat)
            for (int pos = 0; pos < 4; ++pos) {
                uint32_t ms[24];
                for (int j = 0; j < 24; ++j) {
                    ms[j] = 0;
                    for (int k = 0; k < 4; ++k) {
                        const bool set = (k == pos && (j >> 3) == w) ? ((pat >> (j & 7)) & 1) : (rnd() & 1);
                        ms[j] |= set ? 0xffu << (8 * k) : 0u;
                    }
                }
                uint32_t want[3] = { 0, 0, 0 }, got[3] = { 0, 0, 0 };
                for (int j = 0; j < NJ; ++j) sw_sign_edge(want, ms[j], j, K.cbit[j & 7]);
                for (int j0 = 0; j0 < NJ; j0 += 4) sw_sign_quad<NJ>(got, ms, j0, NJ, true, K.c55, K.c33, K.c0f);
                for (int g = 0; g < 3; ++g) {
                    const int cnt = NJ - 8 * g < 0 ? 0 : (NJ - 8 * g > 8 ? 8 : NJ - 8 * g);
                    const uint32_t valid = 0x01010101u * ((1u << cnt) - 1u); /* the layer step masks the bits of edges the row does not have */
                    if ((want[g] & valid) != (got[g] & valid)) ++bad;
                }
                ++n;
            }
    printf("sign_quad<%d>: %ld rows, %ld mismatches\n", NJ, n, bad);
    return bad;
}
}

int main()
{
    long bad = 0;
    bad += check_therm2num();
    bad += check_update<false>();
    bad += check_update<true>();
    bad += check_min_quad();
    bad += check_sign_quad<23>();
    bad += check_sign_quad<22>();
    bad += check_sign_quad<24>();
    printf("total mismatches: %ld\n", bad);
    return bad ? 1 : 0;
}
