/* Self-test of lnsfaid_line_markov_host and lnsfaid_line_markov_thresholds on the host (no GPU, no liblnsfaid.so: it links
 * ../csrc/lnsfaid_tables.c alone).  Every buffer, the three thresholds included, is a heap block of exactly the size the header
 * states, used at an odd address, so that a build with -fsanitize=address,undefined (make line_markov_selftest) sees every access
 * outside it and every misaligned word access:
 *   - the built-in code (33 codewords) and a made-up shape L = 96, K = 32,
 *   - flips and runs are those recounted from line_out ^ line_in and sum to the totals; paging: two calls concatenate to the one-shot
 *     run; in place gives the same bytes,
 *   - t_idle == t_after is lnsfaid_line_bsc_host whatever t_start is; { 0, 0xffffffff, t_start } leaves a codeword alone or inverts
 *     it from position 0 on; { 0, 0, anything } copies the line,
 *   - the threshold helper: the values of (0.01, 0.5), a == p, refusals leave t alone,
 *   - refusals (NULL, t_idle > t_after, L no multiple of 32) and n_codewords == 0 touch nothing. */
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

/* twelve bytes at an odd address holding { idle, after, start } */
struct Thresholds {
    Odd mem;
    Thresholds(uint32_t idle, uint32_t after, uint32_t start) : mem(12)
    {
        const uint32_t v[3] = { idle, after, start };
        memcpy(mem.data(), v, 12);
    }
    const uint32_t* t() { return mem.words(); }
};

static int run(const lnsfaid_code& code, size_t n_cw, uint32_t idle, uint32_t after, uint32_t start)
{
    const size_t L = (size_t)(code.n_var - code.puncture_tail), lb = L / 8;
    const uint64_t key = 0x0123456789abcdefull, first = (1ull << 32) + 5;
    int bad = 0;
    Thresholds th(idle, after, start);

    Odd line(n_cw * lb), out(n_cw * lb), out2(n_cw * lb), fl(n_cw * 4), fl2(n_cw * 4), rn(n_cw * 4), rn2(n_cw * 4);
    for (size_t i = 0; i < n_cw * lb; ++i) line.data()[i] = (uint8_t)(i * 37u + (i >> 8));
    uint64_t total = 1000, total_r = 500, total2 = 0, total_r2 = 0;
    bad += lnsfaid_line_markov_host(&code, line.words(), n_cw, key, first, th.t(), out.words(), fl.words(), rn.words(), &total, &total_r) != 0;
    uint64_t sum = 0, sum_r = 0;
    for (size_t i = 0; i < n_cw; ++i) {
        uint32_t n = 0, r = 0;
        int before = 0;
        for (size_t k = 0; k < L; ++k) {
            const int e = ((line.data()[i * lb + k / 8] ^ out.data()[i * lb + k / 8]) >> (k % 8)) & 1;
            n += (uint32_t)e;
            r += (uint32_t)(e && !before);
            before = e;
        }
        bad += word_at(fl.data(), i) != n || word_at(rn.data(), i) != r;
        sum += n;
        sum_r += r;
    }
    bad += total != 1000 + sum || total_r != 500 + sum_r;
    /* paging */
    const size_t m = n_cw / 2;
    bad += lnsfaid_line_markov_host(&code, line.words(), m, key, first, th.t(), out2.words(), fl2.words(), rn2.words(), &total2, &total_r2) != 0;
    bad += lnsfaid_line_markov_host(&code, (const uint32_t*)(const void*)(line.data() + m * lb), n_cw - m, key, first + m, th.t(),
                                    (uint32_t*)(void*)(out2.data() + m * lb), (uint32_t*)(void*)(fl2.data() + m * 4),
                                    (uint32_t*)(void*)(rn2.data() + m * 4), &total2, &total_r2) != 0;
    bad += memcmp(out.data(), out2.data(), n_cw * lb) != 0 || memcmp(fl.data(), fl2.data(), n_cw * 4) != 0 ||
           memcmp(rn.data(), rn2.data(), n_cw * 4) != 0 || total2 != sum || total_r2 != sum_r;
    /* in place, without the optional outputs */
    memcpy(out2.data(), line.data(), n_cw * lb);
    bad += lnsfaid_line_markov_host(&code, out2.words(), n_cw, key, first, th.t(), out2.words(), nullptr, nullptr, nullptr, nullptr) != 0;
    bad += memcmp(out.data(), out2.data(), n_cw * lb) != 0;

    /* t_idle == t_after: the BSC with that threshold, whatever t_start is */
    const uint32_t starts[3] = { 0u, 0x80000000u, 0xffffffffu };
    uint64_t bsc_total = 0;
    bad += lnsfaid_line_bsc_host(&code, line.words(), n_cw, key, first, after, out.words(), fl.words(), &bsc_total) != 0;
    for (int s = 0; s < 3; ++s) {
        Thresholds flat(after, after, starts[s]);
        total2 = 0;
        bad += lnsfaid_line_markov_host(&code, line.words(), n_cw, key, first, flat.t(), out2.words(), fl2.words(), nullptr, &total2, nullptr) != 0;
        bad += memcmp(out.data(), out2.data(), n_cw * lb) != 0 || memcmp(fl.data(), fl2.data(), n_cw * 4) != 0 || total2 != bsc_total;
    }
    /* { 0, 0xffffffff, 2^31 }: a codeword comes back untouched or inverted from position 0 on (entirely, unless a u is 0xffffffff) */
    {
        Thresholds all(0u, 0xffffffffu, 0x80000000u);
        total2 = total_r2 = 0;
        bad += lnsfaid_line_markov_host(&code, line.words(), n_cw, key, first, all.t(), out2.words(), fl2.words(), rn2.words(), &total2, &total_r2) != 0;
        for (size_t i = 0; i < n_cw; ++i) {
            const uint32_t n = word_at(fl2.data(), i), r = word_at(rn2.data(), i);
            bad += !((n == 0 && r == 0) || (n > 0 && n <= L && r == 1));
            for (size_t k = 0; k < (size_t)n; ++k) bad += (((line.data()[i * lb + k / 8] ^ out2.data()[i * lb + k / 8]) >> (k % 8)) & 1) != 1;
        }
    }
    /* { 0, 0, anything }: a copy */
    {
        Thresholds none(0u, 0u, 0xffffffffu);
        total2 = total_r2 = 0;
        bad += lnsfaid_line_markov_host(&code, line.words(), n_cw, key, first, none.t(), out2.words(), nullptr, nullptr, &total2, &total_r2) != 0;
        bad += memcmp(line.data(), out2.data(), n_cw * lb) != 0 || total2 != 0 || total_r2 != 0;
    }

    /* refusals and the no-op touch nothing */
    Odd keep(n_cw * lb);
    memcpy(keep.data(), out.data(), n_cw * lb);
    total2 = 7; total_r2 = 9;
    Thresholds down(after > 0 ? after : 1u, after > 0 ? after - 1u : 0u, start);
    bad += lnsfaid_line_markov_host(&code, line.words(), n_cw, key, first, down.t(), out.words(), fl.words(), rn.words(), &total2, &total_r2) != LNSFAID_E_INVAL;
    bad += lnsfaid_line_markov_host(&code, nullptr, n_cw, key, first, th.t(), out.words(), nullptr, nullptr, &total2, &total_r2) != LNSFAID_E_INVAL;
    bad += lnsfaid_line_markov_host(&code, line.words(), n_cw, key, first, th.t(), nullptr, nullptr, nullptr, &total2, &total_r2) != LNSFAID_E_INVAL;
    bad += lnsfaid_line_markov_host(&code, line.words(), n_cw, key, first, nullptr, out.words(), nullptr, nullptr, &total2, &total_r2) != LNSFAID_E_INVAL;
    bad += lnsfaid_line_markov_host(nullptr, line.words(), n_cw, key, first, th.t(), out.words(), nullptr, nullptr, &total2, &total_r2) != LNSFAID_E_INVAL;
    bad += lnsfaid_line_markov_host(&code, nullptr, 0, key, first, nullptr, nullptr, nullptr, nullptr, &total2, &total_r2) != 0;
    lnsfaid_code shifted = code;
    shifted.puncture_tail -= 8; /* L no multiple of 32 */
    bad += lnsfaid_line_markov_host(&shifted, line.words(), n_cw, key, first, th.t(), out.words(), nullptr, nullptr, &total2, &total_r2) != LNSFAID_E_INVAL;
    bad += total2 != 7 || total_r2 != 9 || memcmp(keep.data(), out.data(), n_cw * lb) != 0;
    printf("L %zu, %zu codewords, { %u, %u, %u }: %llu flips in %llu runs: %s\n", L, n_cw, idle, after, start, (unsigned long long)sum,
           (unsigned long long)sum_r, bad ? "FAILED" : "ok");
    return bad;
}

int main()
{
    std::unique_ptr<uint16_t[]> pos(new uint16_t[70400]);
    int32_t deg[3], rows[3];
    lnsfaid_code code;
    if (lnsfaid_code_50gpon(&code, pos.get(), deg, rows)) return 2;
    int bad = 0;
    Odd t(12), keep(12);
    bad += lnsfaid_line_markov_thresholds(0.01, 0.5, t.words()) != 0;
    const uint32_t idle = word_at(t.data(), 0), after = word_at(t.data(), 1), start = word_at(t.data(), 2);
    bad += idle != 21691754u || after != 2147483648u || start != 42949672u;
    bad += lnsfaid_line_markov_thresholds(0.01, 0.01, t.words()) != 0;
    bad += word_at(t.data(), 0) != 42949672u || word_at(t.data(), 1) != 42949672u || word_at(t.data(), 2) != 42949672u;
    bad += lnsfaid_line_markov_thresholds(0.0, 0.0, t.words()) != 0;
    bad += word_at(t.data(), 0) != 0u || word_at(t.data(), 1) != 0u || word_at(t.data(), 2) != 0u;
    memcpy(keep.data(), t.data(), 12);
    const double nan = strtod("nan", nullptr);
    bad += lnsfaid_line_markov_thresholds(0.5, 0.01, t.words()) != LNSFAID_E_INVAL || lnsfaid_line_markov_thresholds(-0.1, 0.5, t.words()) != LNSFAID_E_INVAL;
    bad += lnsfaid_line_markov_thresholds(0.01, 1.0, t.words()) != LNSFAID_E_INVAL || lnsfaid_line_markov_thresholds(nan, 0.5, t.words()) != LNSFAID_E_INVAL;
    bad += lnsfaid_line_markov_thresholds(0.01, nan, t.words()) != LNSFAID_E_INVAL || lnsfaid_line_markov_thresholds(0.01, 0.5, nullptr) != LNSFAID_E_INVAL;
    bad += memcmp(t.data(), keep.data(), 12) != 0;

    bad += run(code, 33, idle, after, start);
    bad += run(code, 3, 0xffffffffu / 500u, 4252017623u, 0u); /* the long-run set: a = 0.99 */
    lnsfaid_code small; /* the host form reads only these three */
    memset(&small, 0, sizeof(small));
    small.n_var = 128; small.n_check = 96; small.puncture_tail = 32; /* L = 96, K = 32 */
    bad += run(small, 5, idle, after, start);
    bad += run(small, 1, idle, after, 0xffffffffu);
    printf("line_markov_selftest: %s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
