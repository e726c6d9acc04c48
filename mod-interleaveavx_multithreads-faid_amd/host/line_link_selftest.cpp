/* Self-test of the host forms of the line-format link - lnsfaid_line_payload_random_host, lnsfaid_line_bsc_host,
 * lnsfaid_line_count_errors_host, lnsfaid_line_bsc_threshold - on the host (no GPU, no liblnsfaid.so: it links
 * ../csrc/lnsfaid_tables.c alone).  Every buffer is a heap block of exactly the size the header states, used at an odd address, so
 * that a build with -fsanitize=address,undefined (make line_link_selftest) sees every access outside it and every misaligned
 * word access:
 *   - the built-in code (33 codewords) and a made-up shape L = 96, K = 32 with an odd K / 32,
 *   - paging: two calls concatenate to the one-shot run, payload and channel,
 *   - threshold 0 copies, in place equals out of place, flips sum to the total, the total is added to,
 *   - the counters on planted errors and stats, added to; NULL sent; refusals and n_codewords == 0 touch nothing. */
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

static int popcount_bytes(const uint8_t* a, const uint8_t* b, size_t n)
{
    int c = 0;
    for (size_t i = 0; i < n; ++i) c += __builtin_popcount((unsigned)(a[i] ^ (b ? b[i] : 0)));
    return c;
}

static int run(const lnsfaid_code& code, size_t n_cw)
{
    const size_t L = (size_t)(code.n_var - code.puncture_tail), K = (size_t)(code.n_var - code.n_check);
    const size_t lb = L / 8, kb = K / 8;
    const uint64_t key = 0x0123456789abcdefull, first = (1ull << 32) + 5;
    int bad = 0;

    /* payload: one shot against two pages */
    Odd pay(n_cw * kb), page(n_cw * kb);
    bad += lnsfaid_line_payload_random_host(&code, key, first, n_cw, pay.words()) != 0;
    const size_t m = n_cw / 2;
    bad += lnsfaid_line_payload_random_host(&code, key, first, m, page.words()) != 0;
    bad += lnsfaid_line_payload_random_host(&code, key, first + m, n_cw - m, (uint32_t*)(void*)(page.data() + m * kb)) != 0;
    bad += memcmp(pay.data(), page.data(), n_cw * kb) != 0;
    Odd one(kb);
    bad += lnsfaid_line_payload_random_host(&code, key, first + n_cw - 1, 1, one.words()) != 0;
    bad += memcmp(one.data(), pay.data() + (n_cw - 1) * kb, kb) != 0;

    /* channel: a line of payload-like words (the content does not matter to the channel) */
    Odd line(n_cw * lb), out(n_cw * lb), out2(n_cw * lb), fl(n_cw * 4), fl2(n_cw * 4);
    for (size_t i = 0; i < n_cw * lb; ++i) line.data()[i] = (uint8_t)(i * 37u + (i >> 8));
    uint32_t thr = 0;
    bad += lnsfaid_line_bsc_threshold(0.01, &thr) != 0 || thr != 42949672u;
    uint64_t total = 1000, total2 = 0;
    bad += lnsfaid_line_bsc_host(&code, line.words(), n_cw, key, first, thr, out.words(), fl.words(), &total) != 0;
    uint64_t sum = 0;
    for (size_t i = 0; i < n_cw; ++i) {
        sum += word_at(fl.data(), i);
        bad += (int)word_at(fl.data(), i) != popcount_bytes(line.data() + i * lb, out.data() + i * lb, lb);
    }
    bad += total != 1000 + sum || (n_cw * L > 100000 && sum == 0);
    bad += lnsfaid_line_bsc_host(&code, line.words(), m, key, first, thr, out2.words(), fl2.words(), &total2) != 0;
    bad += lnsfaid_line_bsc_host(&code, (const uint32_t*)(const void*)(line.data() + m * lb), n_cw - m, key, first + m, thr,
                                 (uint32_t*)(void*)(out2.data() + m * lb), (uint32_t*)(void*)(fl2.data() + m * 4), &total2) != 0;
    bad += memcmp(out.data(), out2.data(), n_cw * lb) != 0 || memcmp(fl.data(), fl2.data(), n_cw * 4) != 0 || total2 != sum;
    /* in place, without the optional outputs */
    memcpy(out2.data(), line.data(), n_cw * lb);
    bad += lnsfaid_line_bsc_host(&code, out2.words(), n_cw, key, first, thr, out2.words(), nullptr, nullptr) != 0;
    bad += memcmp(out.data(), out2.data(), n_cw * lb) != 0;
    /* threshold 0 copies; the largest threshold inverts nearly everything */
    total2 = 0;
    bad += lnsfaid_line_bsc_host(&code, line.words(), n_cw, key, first, 0u, out2.words(), fl2.words(), &total2) != 0;
    bad += memcmp(line.data(), out2.data(), n_cw * lb) != 0 || total2 != 0;
    for (size_t i = 0; i < n_cw; ++i) bad += word_at(fl2.data(), i) != 0;
    total2 = 0;
    bad += lnsfaid_line_bsc_host(&code, line.words(), n_cw, key, first, 0xffffffffu, out2.words(), nullptr, &total2) != 0;
    bad += total2 + 16 < n_cw * L || total2 > n_cw * L;

    /* counters: planted errors against the drawn payload; codeword 0 clean, the last one with 3 wrong bits in its last word */
    Odd got(n_cw * kb), st(n_cw * sizeof(lnsfaid_line_stats), 0);
    memcpy(got.data(), pay.data(), n_cw * kb);
    got.data()[(n_cw - 1) * kb + kb - 1] ^= 0xe0;
    if (n_cw > 2) got.data()[1 * kb] ^= 0x01; /* one wrong bit, first word */
    for (size_t i = 0; i < n_cw; ++i) {
        lnsfaid_line_stats s = { 3, 0, i == n_cw - 1 ? 5 : 0, (int32_t)(i % 3) };
        memcpy(st.data() + i * sizeof(s), &s, sizeof(s));
    }
    uint64_t e[4] = { 10, 20, 30, 40 }, f[4] = { 0, 0, 0, 0 }, v[4] = { 0, 0, 0, 0 };
    bad += lnsfaid_line_count_errors_host(&code, got.words(), pay.words(), (const lnsfaid_line_stats*)(const void*)st.data(), n_cw, e, f, v) != 0;
    const uint64_t frames = n_cw > 2 ? 2 : 1, bits = n_cw > 2 ? 4 : 3, lt3 = n_cw > 2 ? 1 : 0;
    bad += e[0] != 10 + n_cw || e[1] != 20 + frames || e[2] != 30 + bits || e[3] != 40 + lt3;
    uint64_t cw_corr = 0, b_corr = 0;
    for (size_t i = 0; i + 1 < n_cw; ++i) { cw_corr += i % 3 > 0; b_corr += i % 3; }
    bad += f[0] != n_cw || f[1] != 1 || f[2] != cw_corr || f[3] != b_corr;
    bad += v[0] != n_cw || v[1] != frames || v[2] != frames - 1 || v[3] != 0;
    uint64_t z[4] = { 0, 0, 0, 0 };
    bad += lnsfaid_line_count_errors_host(&code, got.words(), nullptr, nullptr, n_cw, z, nullptr, nullptr) != 0;
    bad += z[0] != n_cw || z[2] != (uint64_t)popcount_bytes(got.data(), nullptr, n_cw * kb);

    /* refusals and the no-op touch nothing */
    const uint64_t e0[4] = { e[0], e[1], e[2], e[3] };
    bad += lnsfaid_line_count_errors_host(&code, got.words(), pay.words(), nullptr, n_cw, e, f, nullptr) != LNSFAID_E_INVAL;
    bad += lnsfaid_line_count_errors_host(&code, got.words(), pay.words(), nullptr, n_cw, e, nullptr, v) != LNSFAID_E_INVAL;
    bad += lnsfaid_line_count_errors_host(&code, nullptr, pay.words(), nullptr, n_cw, e, nullptr, nullptr) != LNSFAID_E_INVAL;
    bad += lnsfaid_line_count_errors_host(nullptr, got.words(), pay.words(), nullptr, n_cw, e, nullptr, nullptr) != LNSFAID_E_INVAL;
    bad += lnsfaid_line_count_errors_host(&code, nullptr, nullptr, nullptr, 0, e, nullptr, nullptr) != 0;
    bad += memcmp(e, e0, sizeof(e)) != 0;
    Odd keep(n_cw * lb);
    memcpy(keep.data(), out.data(), n_cw * lb);
    total2 = 7;
    bad += lnsfaid_line_bsc_host(&code, nullptr, n_cw, key, first, thr, out.words(), nullptr, &total2) != LNSFAID_E_INVAL;
    bad += lnsfaid_line_bsc_host(&code, line.words(), n_cw, key, first, thr, nullptr, nullptr, &total2) != LNSFAID_E_INVAL;
    bad += lnsfaid_line_bsc_host(nullptr, line.words(), n_cw, key, first, thr, out.words(), nullptr, &total2) != LNSFAID_E_INVAL;
    bad += lnsfaid_line_bsc_host(&code, nullptr, 0, key, first, thr, nullptr, nullptr, &total2) != 0;
    bad += lnsfaid_line_payload_random_host(&code, key, first, n_cw, nullptr) != LNSFAID_E_INVAL;
    bad += lnsfaid_line_payload_random_host(&code, key, first, 0, nullptr) != 0;
    lnsfaid_code shifted = code;
    shifted.puncture_tail -= 8; /* L no multiple of 32 */
    bad += lnsfaid_line_bsc_host(&shifted, line.words(), n_cw, key, first, thr, out.words(), nullptr, &total2) != LNSFAID_E_INVAL;
    bad += lnsfaid_line_payload_random_host(&shifted, key, first, n_cw, pay.words()) != LNSFAID_E_INVAL;
    bad += total2 != 7 || memcmp(keep.data(), out.data(), n_cw * lb) != 0 || memcmp(pay.data(), page.data(), n_cw * kb) != 0;
    printf("L %zu K %zu, %zu codewords, %llu flips: %s\n", L, K, n_cw, (unsigned long long)sum, bad ? "FAILED" : "ok");
    return bad;
}

int main()
{
    std::unique_ptr<uint16_t[]> pos(new uint16_t[70400]);
    int32_t deg[3], rows[3];
    lnsfaid_code code;
    if (lnsfaid_code_50gpon(&code, pos.get(), deg, rows)) return 2;
    int bad = run(code, 33);
    lnsfaid_code small; /* the host forms read only these three */
    memset(&small, 0, sizeof(small));
    small.n_var = 128; small.n_check = 96; small.puncture_tail = 32; /* L = 96, K = 32: an odd K / 32 */
    bad += run(small, 5);
    bad += run(small, 1);
    uint32_t t = 123;
    bad += lnsfaid_line_bsc_threshold(0.0, &t) != 0 || t != 0;
    bad += lnsfaid_line_bsc_threshold(1.0 - 1.0 / 4294967296.0, &t) != 0 || t != 0xffffffffu;
    bad += lnsfaid_line_bsc_threshold(1.0, &t) != LNSFAID_E_INVAL || lnsfaid_line_bsc_threshold(-0.0001, &t) != LNSFAID_E_INVAL;
    bad += lnsfaid_line_bsc_threshold(strtod("nan", nullptr), &t) != LNSFAID_E_INVAL || t != 0xffffffffu;
    printf("line_link_selftest: %s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
