/* Exhaustive comparison of the helpers of csrc/lnsfaid_swar.h that shortened the layer trip with the statements they replaced,
 * each over its whole input domain (tests/test_layer_trip_helpers_exhaustive.py builds and runs this; no GPU):
 *   node_addr   LDS byte address of the new arg-min node: every lane, shift, block column and row
 *   gather4     four separately read bytes into one word: every byte value in every position
 *   scatter4    the bytes a word is scattered as, with one shared shift for the odd bytes: every byte value in every position
 *   selector    the v_perm selector 2 k + b of the arg-min edge from its sign word: every one-hot bit against every byte
 *   index masks index bit 4 / bit 3 as byte masks from the decode words instead of from the shifted index: every combination
 *               of "accumulator differs from the minimum" in every byte
 *   table pick  the error-floor / selective-offset table chosen on the table words against the select on the rows' results */
#include <stdio.h>
#include "lnsfaid_swar.h"

/* the mask / shift / merge form of the node address that sw_node_addr replaced */
static uint32_t node_addr_ref(uint32_t tid4, uint32_t sb, uint32_t k)
{
    const uint32_t x = tid4 + sb;
    return ((x & 0xfcu) | (x >> 16)) | ((((x >> 8) & 3u) + k) & 3u);
}

static long total = 0;
static void report(const char* name, long n, long bad) { printf("%s: %ld cases, %ld mismatches\n", name, n, bad); total += bad; }

int main()
{
    {
        long n = 0, bad = 0;
        for (uint32_t lane = 0; lane < 64; ++lane)
            for (uint32_t shift = 0; shift < 256; ++shift)
                for (uint32_t cb = 0; cb < 256; ++cb)
                    for (uint32_t k = 0; k < 4; ++k) {
                        const uint32_t tid4 = lane << 2, sb = ((cb * 256u) << 16) | (4u * shift);
                        const uint32_t x = tid4 + sb + (k << 8);
                        bad += sw_node_addr(x) != node_addr_ref(tid4, sb, k);
                        ++n;
                    }
        report("node_addr", n, bad);
    }
    {
        long n = 0, bad = 0;
        for (uint32_t pos = 0; pos < 4; ++pos)
            for (uint32_t v = 0; v < 256; ++v)
                for (uint32_t other = 0; other < 256; other += 85) {
                    uint32_t g[4] = { other, other, other, other };
                    g[pos] = v;
                    bad += sw_gather4(g[0], g[1], g[2], g[3]) != (g[0] | (g[1] << 8) | (g[2] << 16) | (g[3] << 24));
                    const uint32_t r = sw_gather4(g[0], g[1], g[2], g[3]), rh = sw_opaque(r >> 8);
                    /* what wr8 stores: the low byte of its operand */
                    bad += (uint8_t)r != (uint8_t)g[0] || (uint8_t)rh != (uint8_t)(r >> 8) || (uint8_t)(r >> 16) != (uint8_t)g[2] || (uint8_t)(rh >> 16) != (uint8_t)(r >> 24);
                    n += 2;
                }
        report("gather4 / scatter4", n, bad);
    }
    {
        long n = 0, bad = 0;
        const uint32_t c7f = 0x7f7f7f7fu, c80 = 0x80808080u, c01 = 0x01010101u, c0642 = 0x06040200u;
        for (uint32_t pos = 0; pos < 4; ++pos)
            for (uint32_t e = 0; e < 8; ++e)
                for (uint32_t w = 0; w < 256; ++w)
                    for (uint32_t fill = 0; fill < 2; ++fill) {
                        const uint32_t bg = fill ? 0xffffffffu : 0u;
                        const uint32_t oh8 = (0x01010101u << 3) ^ ((0x08u ^ (1u << e)) << (8 * pos)); /* one-hot in every byte */
                        const uint32_t wA = (bg & ~(0xffu << (8 * pos))) | (w << (8 * pos));
                        const uint32_t xb = (((wA & oh8) + c7f) & c80) >> 7;
                        bad += sw_argmin_selector(wA, oh8, c7f, c01, c0642) != (xb | c0642);
                        ++n;
                    }
        report("selector", n, bad);
    }
    {
        long n = 0, bad = 0;
        const uint32_t c7f = 0x7f7f7f7fu;
        /* per byte: d4 / d3 = the decode word of bit 4 / 3 before c7f is added (0: equal to the minimum, else 1 .. 0x7f) */
        const uint32_t dv[3] = { 0u, 1u, 0x7fu };
        for (uint32_t c = 0; c < 6561; ++c) { /* 3^8: both words, four bytes */
            uint32_t d4 = 0, d3 = 0, t = c;
            for (int k = 0; k < 4; ++k) { d4 |= dv[t % 3] << (8 * k); t /= 3; d3 |= dv[t % 3] << (8 * k); t /= 3; }
            const uint32_t e4 = d4 + c7f, e3 = d3 + c7f;
            /* the index bits as sw_layer_step decodes them */
            uint32_t idx = ~(e4 >> 3) & (0x01010101u << 4);
            idx = sw_bitop3<0xf2>(idx, (e3 >> 4) | (idx >> 1), 0x01010101u << 3);
            const uint32_t in1 = sw_mask7(idx << 4, SW_SEL_SIGN), in2 = sw_mask7(idx << 3, SW_SEL_SIGN);
            const uint32_t nm4 = sw_mask7(e4, SW_SEL_SIGN), nm3 = sw_mask7(e3, SW_SEL_SIGN);
            for (uint32_t v = 0; v < 3; ++v) {
                const uint32_t x0 = 0x11111111u * (v + 1), x1 = 0x22222222u * (v + 1), x2 = 0x0f0f0f0fu * (v + 5), keep = 0x55aa33ccu * (v + 1);
                uint32_t oh[3];
                sw_word_deal(keep, nm3, nm4, oh);
                bad += sw_word_pick(nm3, nm4, x0, x1, x2) != sw_bitop3<SW_TT_SEL>(in2, x2, sw_bitop3<SW_TT_SEL>(in1, x1, x0));
                bad += oh[0] != (keep & ~(in1 | in2));
                bad += oh[1] != (keep & in1);
                bad += oh[2] != (keep & in2);
                n += 4;
            }
        }
        report("index masks", n, bad);
    }
    {
        long n = 0, bad = 0;
        /* [0]: a FAID table and its error-floor table; [1]: the two selective-offset tables of Factor_1 = 1, Factor_2 = 6 (sw_oms_tables);
         * [2]: two arbitrary tables */
        SwParams po;
        po.f1 = 1; po.f2 = 6;
        sw_oms_tables(po);
        const uint32_t tabs[3][4] = { { 0x03020100u, 0x07060504u, 0x02010000u, 0x07050403u },
                                      { po.oms_lo[0], po.oms_hi[0], po.oms_lo[1], po.oms_hi[1] },
                                      { 0x05030001u, 0x07070706u, 0x01040207u, 0x00030605u } };
        for (int t = 0; t < 3; ++t)
            for (int win = 0; win < 2; ++win)
                for (uint32_t rp = 0; rp < 16; ++rp)
                    for (uint32_t m = 0; m < 4096; ++m) {
                        const uint32_t t_lo = tabs[t][0], t_hi = tabs[t][1], e_lo = tabs[t][2], e_hi = tabs[t][3];
                        const uint32_t rowpar = ((rp & 1) ? 0xffu : 0u) | ((rp & 2) ? 0xff00u : 0u) | ((rp & 4) ? 0xff0000u : 0u) | ((rp & 8) ? 0xff000000u : 0u);
                        const uint32_t mn = (m & 7u) | (((m >> 3) & 7u) << 8) | (((m >> 6) & 7u) << 16) | (((m >> 9) & 7u) << 24);
                        uint32_t was = sw_perm(t_hi, t_lo, mn); /* the statements replaced: the second table under the condition */
                        if (win) was = sw_bitop3<SW_TT_SEL>(rowpar, sw_perm(e_hi, e_lo, mn), was);
                        const uint32_t w_lo = win ? e_lo : t_lo, w_hi = win ? e_hi : t_hi;
                        bad += sw_table_pick(rowpar, w_hi, w_lo, t_hi, t_lo, mn) != was;
                        ++n;
                    }
        report("table pick", n, bad);
    }
    printf("total mismatches: %ld\n", total);
    return total != 0;
}
