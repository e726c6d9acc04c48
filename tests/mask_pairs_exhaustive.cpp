/*
 * mask_pairs_exhaustive.cpp — TEST INFRASTRUCTURE (compiled by tests/test_mask_pairs_exhaustive.py with g++): the paired mask
 * expanders of csrc/lnsfaid_swar.h, sw_mask7x2 and sw_zero_mask2 (one 64-bit shift for two words), against two calls
 * of the definitions they stand for, sw_mask7 and sw_zero_mask.  The host form restates the instruction: the high word of the
 * shifted pair is (b << 8) | (a >> 24), so the top byte of a sits in byte 0 of what the expander of b reads - the byte the sign
 * selectors must never look at.  Prints one line per check and returns non-zero on any mismatch.
 */
#include <stdint.h>
#include <stdio.h>

#include "lnsfaid_swar.h"

namespace {
uint32_t rng_state = 0x9e3779b9u;
uint32_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5;
    return rng_state;
}

/* both argument orders of one pair of words */
long pair_bad(uint32_t a, uint32_t b)
{
    long bad = 0;
    for (int order = 0; order < 2; ++order) {
        const uint32_t x = order ? b : a, y = order ? a : b;
        uint32_t mx = ~0u / 3, my = ~0u / 5;
        sw_mask7x2(x, y, SW_SEL_SIGN, &mx, &my);
        if (mx != sw_mask7(x, SW_SEL_SIGN)) ++bad;
        if (my != sw_mask7(y, SW_SEL_SIGN)) ++bad;
    }
    return bad;
}
long zero_pair_bad(uint32_t a, uint32_t b)
{
    long bad = 0;
    for (int order = 0; order < 2; ++order) {
        const uint32_t x = order ? b : a, y = order ? a : b;
        uint32_t zx = ~0u / 3, zy = ~0u / 5;
        sw_zero_mask2(x, y, SW_SEL_SIGN, &zx, &zy);
        if (zx != sw_zero_mask(x, SW_SEL_SIGN)) ++bad;
        if (zy != sw_zero_mask(y, SW_SEL_SIGN)) ++bad;
    }
    return bad;
}

/* the definition itself: 0xff where bit 7 of the byte is set */
long check_definition()
{
    long bad = 0, n = 0;
    for (int rep = 0; rep < 4096; ++rep) {
        const uint32_t x = rnd();
        uint32_t want = 0;
        for (int k = 0; k < 4; ++k)
            if ((x >> (8 * k + 7)) & 1u) want |= 0xffu << (8 * k);
        if (sw_mask7(x, SW_SEL_SIGN) != want) ++bad;
        ++n;
    }
    printf("mask7 definition: %ld words, %ld mismatches\n", n, bad);
    return bad;
}

/* every byte value in every byte position of a and of b, the other bytes from the generator */
long check_every_byte()
{
    long bad = 0, n = 0;
    for (int word = 0; word < 2; ++word)
        for (int pos = 0; pos < 4; ++pos)
            for (uint32_t v = 0; v < 256; ++v)
                for (int rep = 0; rep < 64; ++rep) {
                    uint32_t w[2] = { rnd(), rnd() };
                    w[word] = (w[word] & ~(0xffu << (8 * pos))) | (v << (8 * pos));
                    bad += pair_bad(w[0], w[1]);
                    ++n;
                }
    printf("mask7x2 every byte: %ld pairs, %ld mismatches\n", n, bad);
    return bad;
}

/* the foreign byte: all 256 values of a's top byte against the four sign patterns of b's bytes 0 and 2 (the bytes whose signs are read
 * from the shifted word, next to the foreign byte), with b's other bits all clear, all set and random */
long check_foreign_byte()
{
    long bad = 0, n = 0;
    for (uint32_t top = 0; top < 256; ++top)
        for (uint32_t pat = 0; pat < 4; ++pat)
            for (int fill = 0; fill < 18; ++fill) {
                const uint32_t a = (fill == 0 ? 0u : fill == 1 ? 0x00ffffffu : rnd() & 0x00ffffffu) | (top << 24);
                uint32_t b = fill == 0 ? 0u : fill == 1 ? 0xffffffffu : rnd();
                b = (b & ~0x00800080u) | ((pat & 1u) ? 0x00000080u : 0u) | ((pat & 2u) ? 0x00800000u : 0u);
                bad += pair_bad(a, b);
                ++n;
            }
    printf("mask7x2 foreign byte: %ld pairs, %ld mismatches\n", n, bad);
    return bad;
}

/* sw_zero_mask2 on its domain (bytes <= 0x7f): every value in every position of either word */
long check_zero_mask2()
{
    long bad = 0, n = 0;
    for (int word = 0; word < 2; ++word)
        for (int pos = 0; pos < 4; ++pos)
            for (uint32_t v = 0; v < 128; ++v)
                for (int rep = 0; rep < 64; ++rep) {
                    /* neighbours: mostly small numbers (the magnitudes 0..7 the layer step passes), zero often */
                    uint32_t w[2];
                    for (int i = 0; i < 2; ++i) {
                        const uint32_t r = rnd();
                        w[i] = (rep & 1) ? r & 0x07070707u & (rnd() | rnd()) : r & 0x7f7f7f7fu;
                    }
                    w[word] = (w[word] & ~(0xffu << (8 * pos))) | (v << (8 * pos));
                    bad += zero_pair_bad(w[0], w[1]);
                    ++n;
                }
    /* and all pairs of magnitude words with one value per word */
    for (uint32_t x = 0; x < 8; ++x)
        for (uint32_t y = 0; y < 8; ++y) {
            bad += zero_pair_bad(x * 0x01010101u, y * 0x01010101u);
            ++n;
        }
    printf("zero_mask2: %ld pairs, %ld mismatches\n", n, bad);
    return bad;
}

/* the halves on their own, as the layer step's stages use them */
long check_halves()
{
    long bad = 0, n = 0;
    for (int rep = 0; rep < 65536; ++rep) {
        uint32_t a = rnd(), b = rnd();
        const uint32_t a0 = a, b0 = b;
        const uint64_t sh = sw_shl8x2(a, b);
        if (a != a0 || b != b0) ++bad; /* the words come back unchanged */
        if (sh != ((((uint64_t)b0 << 32) | a0) << 8)) ++bad;
        if (sw_mask7_lo(a, sh, SW_SEL_SIGN) != sw_mask7(a0, SW_SEL_SIGN)) ++bad;
        if (sw_mask7_hi(b, sh, SW_SEL_SIGN) != sw_mask7(b0, SW_SEL_SIGN)) ++bad;
        ++n;
    }
    printf("shl8x2 halves: %ld pairs, %ld mismatches\n", n, bad);
    return bad;
}
} // namespace

int main()
{
    long bad = 0;
    bad += check_definition();
    bad += check_every_byte();
    bad += check_foreign_byte();
    bad += check_zero_mask2();
    bad += check_halves();
    printf("total mismatches: %ld\n", bad);
    return bad ? 1 : 0;
}
