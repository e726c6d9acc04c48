/* Self-test of the host forms of the burst-format line calls (no GPU, no liblnsfaid.so: it links ../csrc/lnsfaid_tables.c alone).
 *   burst_selftest CIRC_FILE
 * CIRC_FILE holds what lnsfaid_code_parity_inverse returns for the built-in code (tests/test_burst_cpu.py writes it).
 * lnsfaid_burst_words, lnsfaid_encode_burst_host and lnsfaid_burst_to_llr4 run on heap buffers of exactly the sizes
 * lnsfaid_burst_words reports, every one of them (shortened included) at an odd address, so that a build with
 * -fsanitize=address,undefined (make burst_selftest) sees every access outside them and every misaligned word access:
 *   - bits satisfies every row of H, holds zeros in the known range, and line is its first L bits without that range,
 *   - without bits the line is the same,
 *   - the llr4 of the encoded line (HARD, magnitude 3) holds -7 in the known range, +-3 by the codeword's bit elsewhere, 0 in the tail,
 *     and the llr4 of an LLR4 line of the same size holds that line's nibbles,
 *   - refused calls touch nothing. */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "lnsfaid.h"

static unsigned long long g_state = 0x9E3779B97F4A7C15ull;
static unsigned rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(g_state >> 33); }

static int bit_at(const uint8_t* p, size_t k) { return (p[k / 8] >> (k % 8)) & 1; }
static int nib_at(const uint8_t* p, size_t e) { const int v = (p[e / 2] >> (e % 2 ? 4 : 0)) & 15; return v >= 8 ? v - 16 : v; }

/* a heap buffer of exactly n bytes that starts at an odd address */
struct Odd {
    std::unique_ptr<uint8_t[]> mem;
    uint8_t* p;
    explicit Odd(size_t n) : mem(new uint8_t[n + 1]), p(mem.get() + 1) {}
};

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: burst_selftest CIRC_FILE\n"); return 2; }
    std::unique_ptr<uint16_t[]> pos(new uint16_t[70400]);
    int32_t deg[3], rows[3];
    lnsfaid_code code;
    if (lnsfaid_code_50gpon(&code, pos.get(), deg, rows)) return 2;
    const size_t N = (size_t)code.n_var, M = (size_t)code.n_check, K = N - M, L = N - (size_t)code.puncture_tail;
    const size_t z = (size_t)code.z, mb = M / z, circ_bytes = mb * mb * z / 8;
    std::unique_ptr<uint8_t[]> circ(new uint8_t[circ_bytes]);
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(circ.get(), 1, circ_bytes, f) != circ_bytes || fgetc(f) != EOF) { fprintf(stderr, "cannot read %zu bytes of circ\n", circ_bytes); return 2; }
    fclose(f);
    static const uint32_t short_set[8] = { 0, 32, 224, 256, 288, 5760, 8288, 14560 };
    int bad = 0;
    const size_t counts[2] = { 1, 33 };
    for (size_t n : counts)
        for (int32_t where : { LNSFAID_SHORTEN_TAIL, LNSFAID_SHORTEN_HEAD }) {
            Odd sh(4 * n);
            std::unique_ptr<uint32_t[]> S(new uint32_t[n]);
            for (size_t c = 0; c < n; ++c) S[c] = n == 1 ? 14560u : short_set[c % 8];
            memcpy(sh.p, S.get(), 4 * n);
            const uint32_t* shortened = (const uint32_t*)sh.p;
            uint64_t line_bits = 0, payload_bits = 0;
            bad += lnsfaid_burst_words(&code, shortened, n, &line_bits, &payload_bits) != 0;
            uint64_t s_sum = 0;
            for (size_t c = 0; c < n; ++c) s_sum += S[c];
            bad += line_bits != n * L - s_sum || payload_bits != n * K - s_sum;
            Odd payload(payload_bits / 8), line(line_bits / 8), line_only(line_bits / 8), bits(n * N / 8);
            for (size_t i = 0; i < payload_bits / 8; ++i) payload.p[i] = (uint8_t)rnd();
            memset(line.p, 0x5a, line_bits / 8);
            memset(line_only.p, 0x5a, line_bits / 8);
            memset(bits.p, 0x5a, n * N / 8);
            bad += lnsfaid_encode_burst_host(&code, circ.get(), circ_bytes, (const uint32_t*)payload.p, shortened, where, n,
                                             (uint32_t*)line.p, (uint32_t*)bits.p) != 0;
            bad += lnsfaid_encode_burst_host(&code, circ.get(), circ_bytes, (const uint32_t*)payload.p, shortened, where, n,
                                             (uint32_t*)line_only.p, nullptr) != 0;
            bad += memcmp(line.p, line_only.p, line_bits / 8) != 0;
            size_t unsatisfied = 0, known_ones = 0, mismatches = 0, at_line = 0, at_pay = 0;
            for (size_t c = 0; c < n; ++c) {
                const uint8_t* cwb = bits.p + c * (N / 8);
                const size_t k0 = where == LNSFAID_SHORTEN_HEAD ? 0 : K - S[c], k1 = k0 + S[c];
                size_t e = 0;
                for (int d = 0; d < code.nb_degres; ++d)
                    for (int r = 0; r < code.deg_rows[d]; ++r) {
                        int parity = 0;
                        for (int j = 0; j < code.deg[d]; ++j) parity ^= bit_at(cwb, code.pos_vn[e++]);
                        unsatisfied += (size_t)parity;
                    }
                for (size_t p = 0; p < L; ++p) {
                    if (p >= k0 && p < k1) { known_ones += (size_t)bit_at(cwb, p); continue; }
                    mismatches += (size_t)(bit_at(line.p, at_line++) != bit_at(cwb, p));
                    if (p < K) mismatches += (size_t)(bit_at(payload.p, at_pay++) != bit_at(cwb, p));
                }
            }
            bad += unsatisfied != 0 || known_ones != 0 || mismatches != 0 || at_line != line_bits || at_pay != payload_bits;
            /* the definition of the decode: HARD at magnitude 3, then an LLR4 line of random nibbles */
            const size_t groups = (n + 31) / 32;
            Odd llr4(groups * 32 * N / 2), soft(line_bits / 2);
            bad += lnsfaid_burst_to_llr4(&code, line.p, LNSFAID_LINE_HARD, 3, shortened, where, n, llr4.p) != 0;
            for (size_t i = 0; i < line_bits / 2; ++i) soft.p[i] = (uint8_t)rnd();
            Odd llr4s(groups * 32 * N / 2);
            bad += lnsfaid_burst_to_llr4(&code, soft.p, LNSFAID_LINE_LLR4, 0, shortened, where, n, llr4s.p) != 0;
            size_t wrong = 0, at = 0;
            for (size_t c = 0; c < groups * 32; ++c) {
                const size_t g = c / 32, m = c % 32;
                const size_t s_c = c < n ? S[c] : 0, k0 = where == LNSFAID_SHORTEN_HEAD ? 0 : K - s_c, k1 = k0 + s_c;
                const uint8_t* cwb = c < n ? bits.p + c * (N / 8) : nullptr;
                for (size_t p = 0; p < N; ++p) {
                    const size_t e = g * 32 * N + (p < K ? m * K + p : 32 * K + m * M + (p - K));
                    int want = 0, want_soft = 0;
                    if (c < n && p < L) {
                        if (p >= k0 && p < k1) want = want_soft = -7;
                        else { want = bit_at(cwb, p) ? 3 : -3; want_soft = nib_at(soft.p, at++); }
                    }
                    wrong += (size_t)(nib_at(llr4.p, e) != want) + (size_t)(nib_at(llr4s.p, e) != want_soft);
                }
            }
            bad += wrong != 0 || at != line_bits;
            /* refusals touch nothing */
            Odd keep_l(line_bits / 8), keep_b(n * N / 8), keep_4(groups * 32 * N / 2);
            memcpy(keep_l.p, line.p, line_bits / 8);
            memcpy(keep_b.p, bits.p, n * N / 8);
            memcpy(keep_4.p, llr4.p, groups * 32 * N / 2);
            Odd bad_sh(4 * n);
            memcpy(bad_sh.p, S.get(), 4 * n);
            const uint32_t bad_values[4] = { 31u, (uint32_t)K, (uint32_t)K + 32u, 0xffffffe0u };
            for (uint32_t v : bad_values) {
                memcpy(bad_sh.p + 4 * (n - 1), &v, 4);
                const uint32_t* bs = (const uint32_t*)bad_sh.p;
                uint64_t a = 7, b = 9;
                bad += lnsfaid_burst_words(&code, bs, n, &a, &b) != LNSFAID_E_INVAL || a != 7 || b != 9;
                bad += lnsfaid_encode_burst_host(&code, circ.get(), circ_bytes, (const uint32_t*)payload.p, bs, where, n, (uint32_t*)line.p,
                                                 (uint32_t*)bits.p) != LNSFAID_E_INVAL;
                bad += lnsfaid_burst_to_llr4(&code, line.p, LNSFAID_LINE_HARD, 3, bs, where, n, llr4.p) != LNSFAID_E_INVAL;
            }
            bad += lnsfaid_encode_burst_host(&code, circ.get(), circ_bytes, (const uint32_t*)payload.p, shortened, 2, n, (uint32_t*)line.p,
                                             (uint32_t*)bits.p) != LNSFAID_E_INVAL;
            bad += lnsfaid_burst_to_llr4(&code, line.p, LNSFAID_LINE_HARD, 3, shortened, -1, n, llr4.p) != LNSFAID_E_INVAL;
            bad += lnsfaid_encode_burst_host(&code, circ.get(), circ_bytes, nullptr, shortened, where, n, (uint32_t*)line.p,
                                             (uint32_t*)bits.p) != LNSFAID_E_INVAL;
            bad += lnsfaid_burst_to_llr4(&code, nullptr, LNSFAID_LINE_HARD, 3, shortened, where, n, llr4.p) != LNSFAID_E_INVAL;
            bad += lnsfaid_encode_burst_host(&code, circ.get(), circ_bytes, nullptr, nullptr, where, 0, nullptr, nullptr) != 0;
            bad += memcmp(keep_l.p, line.p, line_bits / 8) != 0 || memcmp(keep_b.p, bits.p, n * N / 8) != 0 ||
                   memcmp(keep_4.p, llr4.p, groups * 32 * N / 2) != 0;
            printf("%zu codewords, where %d: line %llu bits, payload %llu bits, %zu unsatisfied checks, %zu wrong levels\n", n, (int)where,
                   (unsigned long long)line_bits, (unsigned long long)payload_bits, unsatisfied, wrong);
        }
    printf("L %zu K %zu N %zu\nburst_selftest: %s\n", L, K, N, bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
