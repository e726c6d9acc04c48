/* Self-test of lnsfaid_encode_line_host on the host (no GPU, no liblnsfaid.so: it links ../csrc/lnsfaid_tables.c alone).
 *   encode_line_selftest CIRC_FILE
 * CIRC_FILE holds what lnsfaid_code_parity_inverse returns for the built-in code (mb * mb * z / 8 bytes; tests/test_encode_line_cpu.py
 * writes it).  1 and 33 codewords of random payload are encoded into heap buffers of exactly the sizes the header states, so that a
 * build with -fsanitize=address,undefined (make encode_line_selftest) sees every access outside them:
 *   - every row of H, taken from pos_vn, is satisfied by every codeword of `bits`, and the information words are the payload's,
 *   - `line` is the first L bits of `bits`, with and without `bits`,
 *   - buffers at odd addresses give the same words,
 *   - refused calls and n_codewords == 0 touch nothing. */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "lnsfaid.h"

static unsigned long long g_state = 0x9E3779B97F4A7C15ull;
static unsigned rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(g_state >> 33); }

static int bit_at(const uint8_t* p, size_t k) { return (p[k / 8] >> (k % 8)) & 1; }

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: encode_line_selftest CIRC_FILE\n"); return 2; }
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
    int bad = 0;
    const size_t counts[2] = { 1, 33 };
    for (size_t n : counts) {
        std::unique_ptr<uint8_t[]> payload(new uint8_t[n * K / 8]), line(new uint8_t[n * L / 8]), bits(new uint8_t[n * N / 8]);
        std::unique_ptr<uint8_t[]> line_only(new uint8_t[n * L / 8]);
        for (size_t i = 0; i < n * K / 8; ++i) payload[i] = (uint8_t)rnd();
        memset(line.get(), 0x5a, n * L / 8);
        memset(bits.get(), 0x5a, n * N / 8);
        memset(line_only.get(), 0x5a, n * L / 8);
        bad += lnsfaid_encode_line_host(&code, circ.get(), circ_bytes, (const uint32_t*)payload.get(), n, (uint32_t*)line.get(),
                                        (uint32_t*)bits.get()) != 0;
        bad += lnsfaid_encode_line_host(&code, circ.get(), circ_bytes, (const uint32_t*)payload.get(), n, (uint32_t*)line_only.get(),
                                        nullptr) != 0;
        size_t unsatisfied = 0, parity_ones = 0;
        for (size_t c = 0; c < n; ++c) {
            const uint8_t* cwb = bits.get() + c * (N / 8);
            bad += memcmp(cwb, payload.get() + c * (K / 8), K / 8) != 0;           /* systematic */
            bad += memcmp(line.get() + c * (L / 8), cwb, L / 8) != 0;               /* line = the first L bits */
            bad += memcmp(line_only.get() + c * (L / 8), cwb, L / 8) != 0;
            size_t e = 0;
            for (int d = 0; d < code.nb_degres; ++d)
                for (int r = 0; r < code.deg_rows[d]; ++r) {
                    int parity = 0;
                    for (int j = 0; j < code.deg[d]; ++j) parity ^= bit_at(cwb, code.pos_vn[e++]);
                    unsatisfied += (size_t)parity;
                }
            for (size_t k = K; k < N; ++k) parity_ones += (size_t)bit_at(cwb, k);
        }
        bad += unsatisfied != 0;
        bad += parity_ones < n * M / 4 || parity_ones > n * M * 3 / 4; /* random payloads: about half the parity bits are set */
        /* every buffer at an odd address */
        std::unique_ptr<uint8_t[]> op(new uint8_t[n * K / 8 + 1]), ol(new uint8_t[n * L / 8 + 1]), ob(new uint8_t[n * N / 8 + 1]);
        memcpy(op.get() + 1, payload.get(), n * K / 8);
        bad += lnsfaid_encode_line_host(&code, circ.get(), circ_bytes, (const uint32_t*)(op.get() + 1), n, (uint32_t*)(ol.get() + 1),
                                        (uint32_t*)(ob.get() + 1)) != 0;
        bad += memcmp(ol.get() + 1, line.get(), n * L / 8) != 0 || memcmp(ob.get() + 1, bits.get(), n * N / 8) != 0;
        /* refusals and the no-op touch nothing */
        std::unique_ptr<uint8_t[]> keep_l(new uint8_t[n * L / 8]), keep_b(new uint8_t[n * N / 8]);
        memcpy(keep_l.get(), line.get(), n * L / 8);
        memcpy(keep_b.get(), bits.get(), n * N / 8);
        const uint32_t* pp = (const uint32_t*)payload.get();
        uint32_t *lp = (uint32_t*)line.get(), *bp = (uint32_t*)bits.get();
        bad += lnsfaid_encode_line_host(nullptr, circ.get(), circ_bytes, pp, n, lp, bp) != LNSFAID_E_INVAL;
        bad += lnsfaid_encode_line_host(&code, nullptr, circ_bytes, pp, n, lp, bp) != LNSFAID_E_INVAL;
        bad += lnsfaid_encode_line_host(&code, circ.get(), circ_bytes - 1, pp, n, lp, bp) != LNSFAID_E_INVAL;
        bad += lnsfaid_encode_line_host(&code, circ.get(), circ_bytes, nullptr, n, lp, bp) != LNSFAID_E_INVAL;
        bad += lnsfaid_encode_line_host(&code, circ.get(), circ_bytes, pp, n, nullptr, bp) != LNSFAID_E_INVAL;
        bad += lnsfaid_encode_line_host(&code, circ.get(), circ_bytes, nullptr, 0, nullptr, nullptr) != 0;
        lnsfaid_code shifted = code;
        shifted.puncture_tail -= 8; /* L no multiple of 32 */
        bad += lnsfaid_encode_line_host(&shifted, circ.get(), circ_bytes, pp, n, lp, bp) != LNSFAID_E_INVAL;
        bad += memcmp(keep_l.get(), line.get(), n * L / 8) != 0 || memcmp(keep_b.get(), bits.get(), n * N / 8) != 0;
        printf("%zu codewords: %zu unsatisfied checks, %zu parity ones\n", n, unsatisfied, parity_ones);
    }
    printf("L %zu K %zu N %zu\nencode_line_selftest: %s\n", L, K, N, bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
