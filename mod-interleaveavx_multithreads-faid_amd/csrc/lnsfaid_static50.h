/*
 * lnsfaid_static50.h - the built-in 50G-PON code as a compile-time description for the layer step: per layer the
 * degree, the number of identity circulants, and 4 * shift / block column * 256 of every edge in the zero-shift-first order of
 * lnsfaid_kernel4z.hip's tables (LfDevCode zs4tab / zcbtab: zero shifts first, ascending block column within either class), all
 * derived from the base matrix of lnsfaid_gpon_base.h by a constexpr function.  Sw50Tab<BR> is the layer step's table view of layer
 * BR with these as constants.  Compiles for the device (lnsfaid_kernel4s.hip) and for the host (tests/static_layers_emul.cpp).
 */
#ifndef LNSFAID_STATIC50_H
#define LNSFAID_STATIC50_H

#include "lnsfaid_gpon_base.h"
#include "lnsfaid_swar.h"

#define SW50_LAYERS LNSFAID_GPON_BLOCK_ROWS

struct Sw50Layer {
    int deg, nz;                  /* edges; leading edges with shift 0 */
    uint32_t s4[SW_MAX_DEG];      /* 4 * shift          */
    uint32_t cb256[SW_MAX_DEG];   /* block column * 256 */
};
struct Sw50Code {
    Sw50Layer layer[SW50_LAYERS];
};

constexpr Sw50Code sw50_build()
{
    struct Circ { int cb, shift; };
    constexpr int deg[SW50_LAYERS] = LNSFAID_GPON_ROW_DEG;
    constexpr Circ base[SW50_LAYERS][LNSFAID_GPON_MAX_DEG] = LNSFAID_GPON_BASE;
    Sw50Code c = {};
    for (int br = 0; br < SW50_LAYERS; ++br) {
        int n = 0;
        for (int zero = 1; zero >= 0; --zero) /* the stable partition lnsfaid_capi.hip's build_code makes */
            for (int j = 0; j < deg[br]; ++j)
                if ((base[br][j].shift == 0) == (zero != 0)) {
                    c.layer[br].s4[n] = (uint32_t)base[br][j].shift << 2;
                    c.layer[br].cb256[n] = (uint32_t)base[br][j].cb << 8;
                    ++n;
                }
        c.layer[br].deg = n;
        int nz = 0;
        while (nz < n && c.layer[br].s4[nz] == 0u) ++nz;
        c.layer[br].nz = nz;
    }
    return c;
}

template <int BR>
struct Sw50Tab {
    static_assert(BR >= 0 && BR < SW50_LAYERS, "layer of the 50G-PON code");
    static constexpr Sw50Layer L = sw50_build().layer[BR];
    static constexpr int DEG = L.deg, NZ = L.nz;
    uint32_t sbv; /* device, lane j < 32: (block column * 256) << 16 | 4 * shift of edge j - the loaded table of the arg-min look-up */
    SW_MFN uint32_t s4(int j) const { return L.s4[j]; }
    SW_MFN uint32_t cb256(int j) const { return L.cb256[j]; }
    SW_MFN uint32_t sb_dyn4(uint32_t idx4) const
    {
#if SW_DEV
        return (uint32_t)__builtin_amdgcn_ds_bpermute((int)idx4, (int)sbv);
#else
        return (L.cb256[idx4 >> 2] << 16) | L.s4[idx4 >> 2];
#endif
    }
};
template <int BR>
struct SwTabStatic<Sw50Tab<BR>> {
    static constexpr bool value = true;
    static constexpr int nz = Sw50Tab<BR>::NZ;
};

/* ---- the edge words of SW_FORM_EDGEW: what a lane needs of a rotating edge besides its block column, in one
 * word.  With x = lane + shift: bits 7:2 the dword x mod 64 of the column (the word under 0xfc is the LDS address inside the column),
 * bits 1:0 the read's byte rotation (x div 64) mod 4, bits 9:8 the write-back's, 4 minus that mod 4.  `edge` counts in Sw50Tab's
 * order, so only edges nz <= edge < deg have words. */
constexpr uint32_t sw50_edge_word_of(uint32_t s4, int lane) /* (constexpr: host and device) */
{
    const uint32_t x = (uint32_t)lane + (s4 >> 2), rq = (x >> 6) & 3u;
    return ((x & 63u) << 2) | rq | (((4u - rq) & 3u) << 8);
}
constexpr uint32_t sw50_edge_word(int layer, int edge, int lane) { return sw50_edge_word_of(sw50_build().layer[layer].s4[edge], lane); }
/* The table a kernel loads them from: [layer][group of four rotating edges][lane][4], so that the 64 lanes' 16-byte loads of a group
 * read 1 KB contiguous; a layer's last group is padded with zero words. */
constexpr int sw50_edge_groups(int layer) { return (sw50_build().layer[layer].deg - sw50_build().layer[layer].nz + 3) / 4; }
constexpr int sw50_edge_group_base(int layer) /* groups in front of the layer's first */
{
    int n = 0;
    for (int br = 0; br < layer; ++br) n += sw50_edge_groups(br);
    return n;
}
#define SW50_EDGE_GROUPS sw50_edge_group_base(SW50_LAYERS)
#define SW50_EDGE_GROUP_WORDS 256
struct Sw50EdgeImage {
    uint32_t w[SW50_EDGE_GROUPS * SW50_EDGE_GROUP_WORDS];
};
constexpr Sw50EdgeImage sw50_edge_image()
{
    constexpr Sw50Code c = sw50_build();
    Sw50EdgeImage im = {};
    int g0 = 0;
    for (int br = 0; br < SW50_LAYERS; ++br) {
        const int rot = c.layer[br].deg - c.layer[br].nz;
        for (int e = 0; e < rot; ++e)
            for (int lane = 0; lane < 64; ++lane)
                im.w[((g0 + e / 4) * 64 + lane) * 4 + e % 4] = sw50_edge_word_of(c.layer[br].s4[c.layer[br].nz + e], lane);
        g0 += (rot + 3) / 4;
    }
    return im;
}
static_assert(SW50_EDGE_GROUPS == 56, "206 rotating edges in groups of four, layer by layer");

/* ---- the decision points' cheap "certainly dirty" test on the compile-time tables.  Any unsatisfied row proves
 * the codeword dirty, so the parity of ONE layer's rows is a sufficient condition that spares the plane build and the full
 * syndrome.  The cheapest layer to ask is the one with the most identity circulants: an identity edge is one read from the
 * lane's own dword of its block column, no address arithmetic, no rotation. */
constexpr int sw50_most_identities()
{
    constexpr Sw50Code c = sw50_build();
    int best = 0;
    for (int br = 1; br < SW50_LAYERS; ++br)
        if (c.layer[br].nz > c.layer[best].nz) best = br;
    return best;
}
#define SW50_CHECK_LAYER sw50_most_identities()

/* Parity of the lane's four rows (lane + 64 k in byte k) of layer BR straight from the En image: bit 7 of byte k of the result is
 * set when row lane + 64 k is unsatisfied under the hard decision En > 0 (bit 7 of En + 120 + 7); the other bits mean nothing.
 * Straight-line: all reads from the address register 4 * lane (identity edges) or the literal-shift address (the others), the block
 * column in the offset field; then, the last read first (LDS returns in order: one wait covers all), flags and a three-input XOR
 * per two edges. */
template <int BR>
SW_FN uint32_t sw50_row_parity(const SwLds& lds, uint32_t lane)
{
    typedef Sw50Tab<BR> Tab;
    constexpr int DEG = Tab::DEG, NZ = Tab::NZ;
    const Tab tab = Tab();
    const uint32_t tid4 = lane << 2;
    uint32_t ad[DEG], rq[DEG], ld[DEG];
#pragma unroll
    for (int j = 0; j < DEG; ++j) {
        const uint32_t x4 = tid4 + tab.s4(j);
        ad[j] = j < NZ ? tid4 : x4 & 0xfcu;
        rq[j] = j < NZ ? 0u : x4 >> 8;
    }
    SW_SCHED_FENCE();
#pragma unroll
    for (int j = 0; j < DEG; ++j) ld[j] = lds.rd32(ad[j], tab.cb256(j));
    SW_SCHED_FENCE();
    uint32_t acc = 0;
#pragma unroll
    for (int j = DEG - 1; j >= 0; j -= 2) {
        const uint32_t fa = sw_hard_flags(j < NZ ? ld[j] : sw_alignbyte(ld[j], ld[j], rq[j]));
        if (j == 0) { acc ^= fa; break; }
        const uint32_t fb = sw_hard_flags(j - 1 < NZ ? ld[j - 1] : sw_alignbyte(ld[j - 1], ld[j - 1], rq[j - 1]));
        acc = sw_bitop3<SW_TT_XOR3>(acc, fa, fb);
    }
    return acc;
}

/* every layer's immediate offset fits the DS instructions' 16-bit field, and the identity edges are the 69 the matrix has */
constexpr bool sw50_check()
{
    constexpr Sw50Code c = sw50_build();
    int zeros = 0, edges = 0;
    for (int br = 0; br < SW50_LAYERS; ++br) {
        for (int j = 0; j < c.layer[br].deg; ++j)
            if (c.layer[br].cb256[j] + 255u > 0xffffu) return false;
        zeros += c.layer[br].nz; edges += c.layer[br].deg;
    }
    return zeros == 69 && edges == 275;
}
static_assert(sw50_check(), "50G-PON base matrix: 275 circulants, 69 of them identities, block columns inside the offset field");

#endif /* LNSFAID_STATIC50_H */
