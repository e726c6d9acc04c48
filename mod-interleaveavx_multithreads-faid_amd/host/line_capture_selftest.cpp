/* Self-test of lnsfaid_line_capture_host and lnsfaid_line_capture_words on the host (no GPU, no liblnsfaid.so: it links
 * ../csrc/lnsfaid_tables.c alone).  Every buffer is a heap block of exactly the size the header states, used at an odd address, so
 * that a build with -fsanitize=address,undefined (make line_capture_selftest) sees every access outside it and every misaligned
 * word access:
 *   - the built-in code (33 codewords) and a made-up code that is not quasi-cyclic (N = 128, M = 96, two row degrees), both formats,
 *   - the sent word is the all-zero codeword in a zeroed buffer; decisions with planted flips in payload, parity and punctured tail,
 *   - every stored record is recounted here from pos_vn: syndrome words, unsatisfied, the error section and its split at K, the
 *     channel's own errors, the flags; records come in ascending index and codeword = first_codeword + index, wrapping,
 *   - paging: capacity 2 concatenates to the one-shot result; a skip beyond found stores nothing; capacity 0 counts only,
 *   - without sent and without line the sections and counts that need them are zero,
 *   - refusals and n_codewords == 0 touch no output. */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "lnsfaid.h"

/* a heap block of exactly n bytes behind one leading byte: data() is odd (operator new returns even addresses) */
struct Odd {
    std::unique_ptr<uint8_t[]> mem;
    size_t n;
    explicit Odd(size_t bytes, int fill = 0x5a) : mem(new uint8_t[bytes + 1]), n(bytes) { memset(mem.get(), fill, bytes + 1); }
    uint8_t* data() { return mem.get() + 1; }
    uint32_t* words() { return (uint32_t*)(void*)data(); }
};

static int bit_at(const uint8_t* p, size_t k) { return (p[k / 8] >> (k % 8)) & 1; }
static void flip(uint8_t* p, size_t k) { p[k / 8] ^= (uint8_t)(1u << (k % 8)); }

static int run(const lnsfaid_code& code, size_t n_cw, int32_t format)
{
    const size_t N = (size_t)code.n_var, M = (size_t)code.n_check, K = N - M, L = N - (size_t)code.puncture_tail;
    const size_t nb = N / 8, lb = format == LNSFAID_LINE_LLR4 ? L / 2 : L / 8;
    const uint64_t first = ~0ull - 1; /* the codeword number wraps inside the call */
    int bad = 0;
    uint32_t W = 0;
    bad += lnsfaid_line_capture_words(&code, format, &W) != 0;
    bad += W != lb / 4 + 2 * (N / 32) + M / 32;

    Odd line(n_cw * lb), bits(n_cw * nb, 0), sent(n_cw * nb, 0);
    for (size_t i = 0; i < n_cw * lb; ++i) line.data()[i] = (uint8_t)(i * 37u + (i >> 8) + (i >> 3));
    /* codeword i: i % 4 == 0 clean, 1 payload flips, 2 parity flips, 3 payload and tail flips */
    size_t planted = 0;
    for (size_t i = 0; i < n_cw; ++i) {
        uint8_t* b = bits.data() + i * nb;
        if (i % 4 == 1) { flip(b, 0); flip(b, K - 1); flip(b, (7 * i) % K == 0 ? 1 : (7 * i) % K == K - 1 ? 2 : (7 * i) % K); }
        if (i % 4 == 2) { flip(b, K); flip(b, L - 1); }
        if (i % 4 == 3) { flip(b, i % K); flip(b, L); flip(b, N - 1); }
        planted += i % 4 != 0;
    }

    std::vector<lnsfaid_line_failure> rec_store(n_cw + 1);
    Odd records(n_cw * sizeof(lnsfaid_line_failure)), payload(n_cw * (size_t)W * 4);
    uint64_t found = 99, stored = 99;
    bad += lnsfaid_line_capture_host(&code, line.data(), format, bits.words(), sent.words(), n_cw, first, 3, 0, n_cw,
                                     (lnsfaid_line_failure*)(void*)records.data(), payload.words(), &found, &stored) != 0;
    bad += found != stored || found > n_cw || found < planted / 2;
    std::vector<uint8_t> bit(N);
    uint64_t prev = 0;
    for (size_t s = 0; s < stored; ++s) {
        lnsfaid_line_failure r;
        memcpy(&r, records.data() + s * sizeof(r), sizeof(r));
        const uint8_t* p = payload.data() + s * (size_t)W * 4;
        const size_t i = r.index;
        bad += i >= n_cw || (s > 0 && i <= prev) || r.codeword != first + (uint64_t)i;
        prev = i;
        if (i >= n_cw) break;
        const uint8_t* b = bits.data() + i * nb;
        bad += memcmp(p, line.data() + i * lb, lb) != 0 || memcmp(p + lb, b, nb) != 0;
        uint32_t wp = 0, wq = 0, ch = 0, unsat = 0;
        for (size_t k = 0; k < N; ++k) {
            bit[k] = (uint8_t)bit_at(b, k);
            bad += bit_at(p + lb + nb, k) != bit[k]; /* sent is zero: the error section is the decisions */
            if (k < K) wp += bit[k];
            else wq += bit[k];
        }
        for (size_t k = 0; k < L; ++k) {
            const uint8_t* l = line.data() + i * lb;
            const int nib = format == LNSFAID_LINE_LLR4 ? (l[k / 2] >> (4 * (k % 2))) & 15 : 0;
            ch += (uint32_t)(format == LNSFAID_LINE_LLR4 ? nib >= 1 && nib <= 7 : bit_at(l, k));
        }
        size_t e = 0, row = 0;
        for (int d = 0; d < code.nb_degres; ++d)
            for (int q = 0; q < code.deg_rows[d]; ++q, ++row) {
                int parity = 0;
                for (int j = 0; j < code.deg[d]; ++j) parity ^= bit[code.pos_vn[e++]];
                bad += bit_at(p + lb + 2 * nb, row) != parity;
                unsat += (uint32_t)parity;
            }
        bad += r.unsatisfied != unsat || r.wrong_payload != wp || r.wrong_parity != wq || r.channel_errors != ch;
        bad += r.flags != ((unsat ? 1u : 0u) | (wp ? 2u : 0u)) || r.flags == 0;
    }

    /* paging */
    Odd rec2(n_cw * sizeof(lnsfaid_line_failure)), pay2(n_cw * (size_t)W * 4);
    uint64_t at = 0, f2 = 0, s2 = 0;
    for (size_t skip = 0; skip < found + 2; skip += 2) {
        bad += lnsfaid_line_capture_host(&code, line.data(), format, bits.words(), sent.words(), n_cw, first, 3, skip, 2,
                                         (lnsfaid_line_failure*)(void*)(rec2.data() + at * sizeof(lnsfaid_line_failure)),
                                         (uint32_t*)(void*)(pay2.data() + at * (size_t)W * 4), &f2, &s2) != 0;
        bad += f2 != found || s2 != (skip >= found ? 0 : found - skip < 2 ? found - skip : 2);
        at += s2;
    }
    bad += at != stored || memcmp(rec2.data(), records.data(), stored * sizeof(lnsfaid_line_failure)) != 0;
    bad += memcmp(pay2.data(), payload.data(), stored * (size_t)W * 4) != 0;
    bad += memcmp(rec2.data() + stored * sizeof(lnsfaid_line_failure), records.data() + stored * sizeof(lnsfaid_line_failure),
                  (n_cw - stored) * sizeof(lnsfaid_line_failure)) != 0; /* nothing past `stored` was written: still the fill */
    /* capacity 0 counts only, NULL records and payload allowed */
    f2 = s2 = 99;
    bad += lnsfaid_line_capture_host(&code, line.data(), format, bits.words(), sent.words(), n_cw, first, 3, 0, 0, nullptr, nullptr, &f2, &s2) != 0;
    bad += f2 != found || s2 != 0;
    /* select 1 and 2 partition by their flag */
    uint64_t f_unc = 0, f_wrong = 0;
    bad += lnsfaid_line_capture_host(&code, nullptr, format, bits.words(), sent.words(), n_cw, first, 1, 0, 0, nullptr, nullptr, &f_unc, &s2) != 0;
    bad += lnsfaid_line_capture_host(&code, nullptr, format, bits.words(), sent.words(), n_cw, first, 2, 0, 0, nullptr, nullptr, &f_wrong, &s2) != 0;
    bad += f_unc > found || f_wrong > found || f_unc + f_wrong < found;

    /* a receiver: no sent word, no line */
    memset(pay2.data(), 0x5a, n_cw * (size_t)W * 4);
    bad += lnsfaid_line_capture_host(&code, nullptr, format, bits.words(), nullptr, n_cw, first, 1, 0, n_cw,
                                     (lnsfaid_line_failure*)(void*)rec2.data(), pay2.words(), &f2, &s2) != 0;
    bad += f2 != f_unc || s2 != f_unc;
    for (size_t s = 0; s < s2; ++s) {
        lnsfaid_line_failure r;
        memcpy(&r, rec2.data() + s * sizeof(r), sizeof(r));
        const uint8_t* p = pay2.data() + s * (size_t)W * 4;
        bad += r.flags != 1u || r.wrong_payload != 0 || r.wrong_parity != 0 || r.channel_errors != 0 || r.unsatisfied == 0;
        for (size_t k = 0; k < lb; ++k) bad += p[k] != 0;
        for (size_t k = 0; k < nb; ++k) bad += p[lb + nb + k] != 0;
        uint32_t pop = 0;
        for (size_t k = 0; k < M; ++k) pop += (uint32_t)bit_at(p + lb + 2 * nb, k);
        bad += pop != r.unsatisfied;
    }

    /* refusals and the no-op touch nothing */
    Odd keep_r(n_cw * sizeof(lnsfaid_line_failure)), keep_p(n_cw * (size_t)W * 4);
    memcpy(keep_r.data(), records.data(), keep_r.n);
    memcpy(keep_p.data(), payload.data(), keep_p.n);
    f2 = s2 = 7;
    lnsfaid_line_failure* R = (lnsfaid_line_failure*)(void*)records.data();
    uint32_t* P = payload.words();
    const int inval = LNSFAID_E_INVAL;
    bad += lnsfaid_line_capture_host(nullptr, line.data(), format, bits.words(), sent.words(), n_cw, first, 3, 0, n_cw, R, P, &f2, &s2) != inval;
    bad += lnsfaid_line_capture_host(&code, line.data(), 2, bits.words(), sent.words(), n_cw, first, 3, 0, n_cw, R, P, &f2, &s2) != inval;
    bad += lnsfaid_line_capture_host(&code, line.data(), format, nullptr, sent.words(), n_cw, first, 3, 0, n_cw, R, P, &f2, &s2) != inval;
    bad += lnsfaid_line_capture_host(&code, line.data(), format, bits.words(), sent.words(), n_cw, first, 0, 0, n_cw, R, P, &f2, &s2) != inval;
    bad += lnsfaid_line_capture_host(&code, line.data(), format, bits.words(), sent.words(), n_cw, first, 4, 0, n_cw, R, P, &f2, &s2) != inval;
    bad += lnsfaid_line_capture_host(&code, line.data(), format, bits.words(), nullptr, n_cw, first, 2, 0, n_cw, R, P, &f2, &s2) != inval;
    bad += lnsfaid_line_capture_host(&code, line.data(), format, bits.words(), nullptr, n_cw, first, 3, 0, n_cw, R, P, &f2, &s2) != inval;
    bad += lnsfaid_line_capture_host(&code, line.data(), format, bits.words(), sent.words(), n_cw, first, 3, 0, n_cw, nullptr, P, &f2, &s2) != inval;
    bad += lnsfaid_line_capture_host(&code, line.data(), format, bits.words(), sent.words(), n_cw, first, 3, 0, n_cw, R, nullptr, &f2, &s2) != inval;
    bad += lnsfaid_line_capture_host(&code, line.data(), format, bits.words(), sent.words(), n_cw, first, 3, 0, n_cw, R, P, nullptr, &s2) != inval;
    bad += lnsfaid_line_capture_host(&code, line.data(), format, bits.words(), sent.words(), n_cw, first, 3, 0, n_cw, R, P, &f2, nullptr) != inval;
    lnsfaid_code shifted = code;
    shifted.puncture_tail -= 8; /* L no multiple of 32 */
    bad += lnsfaid_line_capture_host(&shifted, line.data(), format, bits.words(), sent.words(), n_cw, first, 3, 0, n_cw, R, P, &f2, &s2) != inval;
    uint32_t w2 = 77;
    bad += lnsfaid_line_capture_words(&shifted, format, &w2) != inval || lnsfaid_line_capture_words(&code, 2, &w2) != inval || w2 != 77;
    bad += lnsfaid_line_capture_words(&code, format, nullptr) != inval;
    bad += f2 != 7 || s2 != 7;
    bad += lnsfaid_line_capture_host(&code, nullptr, format, nullptr, nullptr, 0, first, 1, 0, n_cw, R, P, &f2, &s2) != 0;
    bad += f2 != 0 || s2 != 0;
    bad += memcmp(keep_r.data(), records.data(), keep_r.n) != 0 || memcmp(keep_p.data(), payload.data(), keep_p.n) != 0;
    printf("N %zu, %s, %zu codewords, %llu failures of %zu planted: %s\n", N, format == LNSFAID_LINE_LLR4 ? "LLR4" : "HARD", n_cw,
           (unsigned long long)found, planted, bad ? "FAILED" : "ok");
    return bad;
}

int main()
{
    std::unique_ptr<uint16_t[]> pos(new uint16_t[70400]);
    int32_t deg[3], rows[3];
    lnsfaid_code code;
    if (lnsfaid_code_50gpon(&code, pos.get(), deg, rows)) return 2;
    int bad = 0;
    uint32_t W = 0;
    bad += lnsfaid_line_capture_words(&code, LNSFAID_LINE_HARD, &W) != 0 || W != 1740;
    bad += lnsfaid_line_capture_words(&code, LNSFAID_LINE_LLR4, &W) != 0 || W != 3360;
    bad += run(code, 33, LNSFAID_LINE_HARD);
    bad += run(code, 33, LNSFAID_LINE_LLR4);

    /* not quasi-cyclic: 64 rows of degree 3, then 32 rows of degree 5, over 128 variable nodes; every node is in some row */
    const int32_t sdeg[2] = { 3, 5 }, srows[2] = { 64, 32 };
    std::vector<uint16_t> spos;
    uint32_t x = 12345u;
    for (int r = 0; r < 96; ++r)
        for (int j = 0; j < (r < 64 ? 3 : 5); ++j) {
            x = x * 1664525u + 1013904223u;
            spos.push_back(j == 0 ? (uint16_t)((r * 4) % 128 + (r / 32)) : (uint16_t)((x >> 16) % 128u));
        }
    lnsfaid_code small;
    memset(&small, 0, sizeof(small));
    small.n_var = 128; small.n_check = 96; small.puncture_tail = 32; /* L = 96, K = 32 */
    small.n_edges = (int32_t)spos.size(); small.z = 32; small.nb_degres = 2;
    small.deg = sdeg; small.deg_rows = srows; small.pos_vn = spos.data();
    bad += run(small, 9, LNSFAID_LINE_HARD);
    bad += run(small, 9, LNSFAID_LINE_LLR4);
    bad += run(small, 1, LNSFAID_LINE_HARD);
    printf("line_capture_selftest: %s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
