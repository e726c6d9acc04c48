/* Self-test of lnsfaid_line_soft_host and lnsfaid_line_awgn_table on the host (no GPU, no liblnsfaid.so: it links
 * ../csrc/lnsfaid_tables.c alone).  Every buffer is a heap block of exactly the size the header states, used at an odd address, so
 * that a build with -fsanitize=address,undefined (make line_soft_selftest) sees every access outside it and every misaligned
 * word access:
 *   - the built-in code (33 codewords) and a made-up shape L = 96, K = 32,
 *   - paging: two calls concatenate to the one-shot run; the flips are those recounted from the output and sum to the total,
 *   - the all-zero table gives +-7 and no flips, the all-ones table -+7 and a flip at (nearly) every position,
 *   - the table helper: non-decreasing, symmetric bins of a symmetric setting, refusals leave the table alone,
 *   - refusals (NULL, a decreasing table, overlapping ranges, L no multiple of 32) and n_codewords == 0 touch nothing. */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "lnsfaid.h"

/* a heap block of exactly n bytes behind one leading byte: data() is odd (operator new returns even addresses) */
struct Odd {
    std::unique_ptr<uint8_t[]> mem;
    size_t n;
    explicit Odd(size_t bytes, int fill = 0x5a) : mem(new uint8_t[bytes + 1]), n(bytes) { memset(mem.get(), fill, bytes + 1); }
    uint8_t* data() { return mem.get() + 1; }
    uint32_t* words() { return (uint32_t*)(void*)data(); }
};

static uint32_t word_at(const uint8_t* p, size_t w)
{
    uint32_t v;
    memcpy(&v, p + 4 * w, 4);
    return v;
}

static int level_at(const uint8_t* llr4, size_t k)
{
    const int nib = (llr4[k / 2] >> (4 * (k % 2))) & 15;
    return nib >= 8 ? nib - 16 : nib;
}

static int run(const lnsfaid_code& code, size_t n_cw, const uint32_t* table)
{
    const size_t L = (size_t)(code.n_var - code.puncture_tail);
    const size_t lb = L / 8, ob = L / 2;
    const uint64_t key = 0x0123456789abcdefull, first = (1ull << 32) + 5;
    int bad = 0;

    Odd line(n_cw * lb), out(n_cw * ob), out2(n_cw * ob), fl(n_cw * 4), fl2(n_cw * 4);
    for (size_t i = 0; i < n_cw * lb; ++i) line.data()[i] = (uint8_t)(i * 37u + (i >> 8));
    uint64_t total = 1000, total2 = 0;
    bad += lnsfaid_line_soft_host(&code, line.words(), n_cw, key, first, table, out.data(), fl.words(), &total) != 0;
    uint64_t sum = 0;
    for (size_t i = 0; i < n_cw; ++i) {
        uint32_t n = 0;
        for (size_t k = 0; k < L; ++k) {
            const int bit = (line.data()[i * lb + k / 8] >> (k % 8)) & 1, level = level_at(out.data() + i * ob, k);
            n += (uint32_t)((level > 0) != bit);
            bad += level == -8;
        }
        bad += word_at(fl.data(), i) != n;
        sum += n;
    }
    bad += total != 1000 + sum;
    const size_t m = n_cw / 2;
    bad += lnsfaid_line_soft_host(&code, line.words(), m, key, first, table, out2.data(), fl2.words(), &total2) != 0;
    bad += lnsfaid_line_soft_host(&code, (const uint32_t*)(const void*)(line.data() + m * lb), n_cw - m, key, first + m, table,
                                  out2.data() + m * ob, (uint32_t*)(void*)(fl2.data() + m * 4), &total2) != 0;
    bad += memcmp(out.data(), out2.data(), n_cw * ob) != 0 || memcmp(fl.data(), fl2.data(), n_cw * 4) != 0 || total2 != sum;
    /* without the optional outputs */
    memset(out2.data(), 0x5a, n_cw * ob);
    bad += lnsfaid_line_soft_host(&code, line.words(), n_cw, key, first, table, out2.data(), nullptr, nullptr) != 0;
    bad += memcmp(out.data(), out2.data(), n_cw * ob) != 0;

    /* all zero: u >= 0 always, m = 7, no flips; all ones: m = -7 unless u is 0xffffffff */
    uint32_t flat[14];
    memset(flat, 0, sizeof(flat));
    total2 = 0;
    bad += lnsfaid_line_soft_host(&code, line.words(), n_cw, key, first, flat, out2.data(), fl2.words(), &total2) != 0;
    bad += total2 != 0;
    for (size_t k = 0; k < n_cw * L; ++k) {
        const int bit = (line.data()[k / 8] >> (k % 8)) & 1;
        bad += level_at(out2.data(), k) != (bit ? 7 : -7);
    }
    memset(flat, 0xff, sizeof(flat));
    total2 = 0;
    bad += lnsfaid_line_soft_host(&code, line.words(), n_cw, key, first, flat, out2.data(), nullptr, &total2) != 0;
    bad += total2 + 16 < n_cw * L || total2 > n_cw * L;

    /* refusals and the no-op touch nothing */
    Odd keep(n_cw * ob);
    memcpy(keep.data(), out.data(), n_cw * ob);
    total2 = 7;
    uint32_t down[14];
    memcpy(down, table, sizeof(down));
    down[9] = down[8] > 0 ? down[8] - 1 : 0;
    down[8] = down[8] > 0 ? down[8] : 1;
    bad += lnsfaid_line_soft_host(&code, line.words(), n_cw, key, first, down, out.data(), fl.words(), &total2) != LNSFAID_E_INVAL;
    bad += lnsfaid_line_soft_host(&code, nullptr, n_cw, key, first, table, out.data(), nullptr, &total2) != LNSFAID_E_INVAL;
    bad += lnsfaid_line_soft_host(&code, line.words(), n_cw, key, first, table, nullptr, nullptr, &total2) != LNSFAID_E_INVAL;
    bad += lnsfaid_line_soft_host(&code, line.words(), n_cw, key, first, nullptr, out.data(), nullptr, &total2) != LNSFAID_E_INVAL;
    bad += lnsfaid_line_soft_host(nullptr, line.words(), n_cw, key, first, table, out.data(), nullptr, &total2) != LNSFAID_E_INVAL;
    /* overlap: the input inside the output, at its first and at its last byte */
    bad += lnsfaid_line_soft_host(&code, out.words(), n_cw, key, first, table, out.data(), nullptr, &total2) != LNSFAID_E_INVAL;
    bad += lnsfaid_line_soft_host(&code, (const uint32_t*)(const void*)(out.data() + n_cw * ob - 1), n_cw, key, first, table, out.data(), nullptr,
                                  &total2) != LNSFAID_E_INVAL;
    bad += lnsfaid_line_soft_host(&code, nullptr, 0, key, first, nullptr, nullptr, nullptr, &total2) != 0;
    lnsfaid_code shifted = code;
    shifted.puncture_tail -= 8; /* L no multiple of 32 */
    bad += lnsfaid_line_soft_host(&shifted, line.words(), n_cw, key, first, table, out.data(), nullptr, &total2) != LNSFAID_E_INVAL;
    bad += total2 != 7 || memcmp(keep.data(), out.data(), n_cw * ob) != 0;
    printf("L %zu, %zu codewords, %llu flips: %s\n", L, n_cw, (unsigned long long)sum, bad ? "FAILED" : "ok");
    return bad;
}

int main()
{
    std::unique_ptr<uint16_t[]> pos(new uint16_t[70400]);
    int32_t deg[3], rows[3];
    lnsfaid_code code;
    if (lnsfaid_code_50gpon(&code, pos.get(), deg, rows)) return 2;
    int bad = 0;
    uint32_t table[14], t2[14];
    const double scale = 13.0 / sqrt(2.0);
    bad += lnsfaid_line_awgn_table(0.474, scale, table) != 0;
    for (int i = 1; i < 14; ++i) bad += table[i] < table[i - 1];
    bad += table[0] == 0 || table[13] == 0xffffffffu || table[6] >= table[7];
    /* a wide, coarse setting: far tails on both sides */
    bad += lnsfaid_line_awgn_table(0.05, scale, t2) != 0;
    for (int i = 1; i < 14; ++i) bad += t2[i] < t2[i - 1];
    memcpy(t2, table, sizeof(t2));
    const double nan = strtod("nan", nullptr), inf = strtod("inf", nullptr);
    bad += lnsfaid_line_awgn_table(0.0, scale, t2) != LNSFAID_E_INVAL || lnsfaid_line_awgn_table(-1.0, scale, t2) != LNSFAID_E_INVAL;
    bad += lnsfaid_line_awgn_table(nan, scale, t2) != LNSFAID_E_INVAL || lnsfaid_line_awgn_table(inf, scale, t2) != LNSFAID_E_INVAL;
    bad += lnsfaid_line_awgn_table(0.5, 0.0, t2) != LNSFAID_E_INVAL || lnsfaid_line_awgn_table(0.5, nan, t2) != LNSFAID_E_INVAL;
    bad += lnsfaid_line_awgn_table(0.5, inf, t2) != LNSFAID_E_INVAL || lnsfaid_line_awgn_table(0.5, scale, nullptr) != LNSFAID_E_INVAL;
    bad += memcmp(t2, table, sizeof(t2)) != 0;

    bad += run(code, 33, table);
    lnsfaid_code small; /* the host form reads only these three */
    memset(&small, 0, sizeof(small));
    small.n_var = 128; small.n_check = 96; small.puncture_tail = 32; /* L = 96, K = 32 */
    bad += run(small, 5, table);
    bad += run(small, 1, table);
    printf("line_soft_selftest: %s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
