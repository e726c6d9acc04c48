/* Self-test of lnsfaid_line_from_fixinput / lnsfaid_line_to_llr4 on the host (no GPU, no liblnsfaid.so: it links
 * ../csrc/lnsfaid_tables.c alone).  33 codewords of the built-in code - one whole group and one codeword of a second - in heap
 * buffers of exactly the sizes the header states, so that a build with -fsanitize=address,undefined (make line_selftest) sees
 * every access outside them:
 *   - both formats against a restatement of the layouts, element by element,
 *   - the round trip through llr4: +-magnitude / the identity below L, nibble 0 in the punctured tail and in the padding codewords,
 *   - buffers at odd addresses,
 *   - refused calls and n_codewords == 0 touch nothing. */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "lnsfaid.h"

static unsigned long long g_state = 0x9E3779B97F4A7C15ull;
static unsigned rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(g_state >> 33); }

static int nibble_at(const uint8_t* p, size_t e)
{
    const int x = (p[e / 2] >> (e % 2 ? 4 : 0)) & 15;
    return x >= 8 ? x - 16 : x;
}

int main()
{
    std::unique_ptr<uint16_t[]> pos(new uint16_t[70400]);
    int32_t deg[3], rows[3];
    lnsfaid_code code;
    if (lnsfaid_code_50gpon(&code, pos.get(), deg, rows)) return 2;
    const size_t N = (size_t)code.n_var, M = (size_t)code.n_check, K = N - M, L = N - (size_t)code.puncture_tail;
    const size_t n_cw = 33, groups = 2, per = 32 * N;
    int bad = 0;
    std::unique_ptr<int8_t[]> fix(new int8_t[groups * per]);
    for (size_t i = 0; i < groups * per; ++i) fix[i] = (int8_t)((int)(rnd() % 16) - 8);
    auto element = [&](size_t cw, size_t k) { /* the group layout: [32][K] information LLRs, then [32][M] parity LLRs */
        const size_t g = cw / 32, m = cw % 32;
        return g * per + (k < K ? m * K + k : 32 * K + m * M + (k - K));
    };
    /* +1: the same calls once more on buffers at odd addresses */
    std::unique_ptr<uint8_t[]> hard(new uint8_t[n_cw * L / 8]), soft(new uint8_t[n_cw * L / 2]), odd(new uint8_t[n_cw * L / 2 + 1]);
    std::unique_ptr<uint8_t[]> llr4(new uint8_t[groups * per / 2]), llr4_odd(new uint8_t[groups * per / 2 + 1]);
    bad += lnsfaid_line_from_fixinput(&code, fix.get(), n_cw, LNSFAID_LINE_HARD, hard.get()) != 0;
    bad += lnsfaid_line_from_fixinput(&code, fix.get(), n_cw, LNSFAID_LINE_LLR4, soft.get()) != 0;
    size_t wrong = 0;
    for (size_t cw = 0; cw < n_cw; ++cw)
        for (size_t k = 0; k < L; ++k) {
            const int x = fix[element(cw, k)];
            wrong += ((hard[cw * (L / 8) + k / 8] >> (k % 8)) & 1) != (x > 0);
            wrong += nibble_at(soft.get() + cw * (L / 2), k) != x;
        }
    bad += wrong != 0;
    bad += lnsfaid_line_from_fixinput(&code, fix.get(), n_cw, LNSFAID_LINE_LLR4, odd.get() + 1) != 0;
    bad += memcmp(odd.get() + 1, soft.get(), n_cw * L / 2) != 0;
    bad += lnsfaid_line_from_fixinput(&code, fix.get(), n_cw, LNSFAID_LINE_HARD, odd.get() + 1) != 0;
    bad += memcmp(odd.get() + 1, hard.get(), n_cw * L / 8) != 0;

    /* the round trips */
    for (int magnitude = 1; magnitude <= 7; magnitude += 3) {
        memset(llr4.get(), 0x5a, groups * per / 2);
        bad += lnsfaid_line_to_llr4(&code, hard.get(), LNSFAID_LINE_HARD, magnitude, n_cw, llr4.get()) != 0;
        wrong = 0;
        for (size_t cw = 0; cw < groups * 32; ++cw)
            for (size_t k = 0; k < N; ++k) {
                const int want = cw >= n_cw || k >= L ? 0 : (fix[element(cw, k)] > 0 ? magnitude : -magnitude);
                wrong += nibble_at(llr4.get(), element(cw, k)) != want;
            }
        bad += wrong != 0;
    }
    memset(llr4.get(), 0x5a, groups * per / 2);
    bad += lnsfaid_line_to_llr4(&code, soft.get(), LNSFAID_LINE_LLR4, 0 /* ignored */, n_cw, llr4.get()) != 0;
    wrong = 0;
    for (size_t cw = 0; cw < groups * 32; ++cw)
        for (size_t k = 0; k < N; ++k) {
            const int want = cw >= n_cw || k >= L ? 0 : fix[element(cw, k)];
            wrong += nibble_at(llr4.get(), element(cw, k)) != want;
        }
    bad += wrong != 0;
    memcpy(odd.get() + 1, soft.get(), n_cw * L / 2);
    bad += lnsfaid_line_to_llr4(&code, odd.get() + 1, LNSFAID_LINE_LLR4, 0, n_cw, llr4_odd.get() + 1) != 0;
    bad += memcmp(llr4_odd.get() + 1, llr4.get(), groups * per / 2) != 0;
    /* one codeword: exactly L / 8 bytes in, one group out */
    {
        std::unique_ptr<uint8_t[]> one(new uint8_t[L / 8]), g1(new uint8_t[per / 2]);
        bad += lnsfaid_line_from_fixinput(&code, fix.get(), 1, LNSFAID_LINE_HARD, one.get()) != 0;
        bad += memcmp(one.get(), hard.get(), L / 8) != 0;
        bad += lnsfaid_line_to_llr4(&code, one.get(), LNSFAID_LINE_HARD, 4, 1, g1.get()) != 0;
        bad += nibble_at(g1.get(), 0) != (fix[0] > 0 ? 4 : -4) || nibble_at(g1.get(), K) != 0 /* codeword 1: padding */;
    }

    /* refusals and the no-op touch nothing */
    std::unique_ptr<uint8_t[]> keep(new uint8_t[n_cw * L / 2]);
    memcpy(keep.get(), soft.get(), n_cw * L / 2);
    bad += lnsfaid_line_from_fixinput(&code, fix.get(), n_cw, 2, soft.get()) != LNSFAID_E_INVAL;
    bad += lnsfaid_line_from_fixinput(nullptr, fix.get(), n_cw, LNSFAID_LINE_LLR4, soft.get()) != LNSFAID_E_INVAL;
    bad += lnsfaid_line_from_fixinput(&code, nullptr, n_cw, LNSFAID_LINE_LLR4, soft.get()) != LNSFAID_E_INVAL;
    bad += lnsfaid_line_from_fixinput(&code, nullptr, 0, LNSFAID_LINE_LLR4, nullptr) != 0;
    bad += lnsfaid_line_to_llr4(&code, hard.get(), LNSFAID_LINE_HARD, 0, n_cw, llr4.get()) != LNSFAID_E_INVAL;
    bad += lnsfaid_line_to_llr4(&code, hard.get(), LNSFAID_LINE_HARD, 8, n_cw, llr4.get()) != LNSFAID_E_INVAL;
    bad += lnsfaid_line_to_llr4(&code, nullptr, LNSFAID_LINE_HARD, 4, 0, nullptr) != 0;
    lnsfaid_code shifted = code;
    shifted.puncture_tail -= 8; /* L no multiple of 32 */
    bad += lnsfaid_line_from_fixinput(&shifted, fix.get(), n_cw, LNSFAID_LINE_LLR4, soft.get()) != LNSFAID_E_INVAL;
    bad += memcmp(keep.get(), soft.get(), n_cw * L / 2) != 0;
    fix[element(32, L - 1)] = 8; /* out of range in the last transmitted position of the last codeword */
    bad += lnsfaid_line_from_fixinput(&code, fix.get(), n_cw, LNSFAID_LINE_LLR4, soft.get()) != LNSFAID_E_INVAL;
    fix[element(32, L - 1)] = 0;
    fix[element(32, L)] = 100; /* the tail is never read */
    bad += lnsfaid_line_from_fixinput(&code, fix.get(), n_cw, LNSFAID_LINE_LLR4, soft.get()) != 0;
    printf("L %zu K %zu, %zu codewords\nline_selftest: %s\n", L, K, n_cw, bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
