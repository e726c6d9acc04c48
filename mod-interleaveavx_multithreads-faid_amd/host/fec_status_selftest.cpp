/* Self-test of lnsfaid_fec_status_host / lnsfaid_fec_status_packed_host on the host (no GPU, no liblnsfaid.so: it links
 * ../csrc/lnsfaid_tables.c alone).  A random group of the built-in code in buffers of the exact sizes the header states, so that a
 * build with -fsanitize=address,undefined (make fec_status_selftest) sees every access outside them:
 *   - the int8 and the packed form give the same records and counters for the same decisions and LLRs,
 *   - the all-zero word and single flips give 0 and the flipped column's weight,
 *   - a refused call and n_groups == 0 touch nothing. */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "lnsfaid.h"

static unsigned long long g_state = 0x9E3779B97F4A7C15ull;
static unsigned rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(g_state >> 33); }

int main()
{
    std::unique_ptr<uint16_t[]> pos(new uint16_t[70400]);
    int32_t deg[3], rows[3];
    lnsfaid_code code;
    if (lnsfaid_code_50gpon(&code, pos.get(), deg, rows)) return 2;
    const size_t N = (size_t)code.n_var, M = (size_t)code.n_check, K = N - M, per = 32 * N;
    std::unique_ptr<int8_t[]> fix(new int8_t[per]), dec(new int8_t[per]), sent(new int8_t[per]);
    std::unique_ptr<uint8_t[]> llr4(new uint8_t[per / 2]);
    std::unique_ptr<uint32_t[]> bits(new uint32_t[per / 32]);
    std::unique_ptr<lnsfaid_fec_record[]> ra(new lnsfaid_fec_record[32]), rb(new lnsfaid_fec_record[32]);
    memset(sent.get(), 0, per);
    for (size_t i = 0; i < per; ++i) fix[i] = (int8_t)((int)(rnd() % 16) - 8);
    /* frames 0 .. 7: the all-zero word with m single flips at random places; the others: random decisions */
    memset(dec.get(), 0, per);
    unsigned weight_sum[32] = { 0 };
    for (size_t m = 0; m < 32; ++m) {
        if (m >= 8) { for (size_t k = 0; k < N; ++k) dec[m * N + k] = (int8_t)(rnd() & 1); continue; }
        if (m == 0) continue;
        const size_t k = rnd() % N; /* one flip: every check of the column is unsatisfied */
        dec[m * N + k] = 1;
        for (size_t e = 0; e < (size_t)code.n_edges; ++e) weight_sum[m] += pos[e] == k;
    }
    for (size_t i = 0; i < per; i += 2) llr4[i / 2] = (uint8_t)((fix[i] & 15) | (fix[i + 1] & 15) << 4); /* element e: nibble e % 2 of byte e / 2 */
    memset(bits.get(), 0, per / 8);
    for (size_t i = 0; i < per; ++i) bits[i / 32] |= (uint32_t)(dec[i] != 0) << (i % 32);
    uint64_t oa[4] = { 0, 0, 0, 0 }, ob[4] = { 0, 0, 0, 0 }, va[4] = { 0, 0, 0, 0 }, vb[4] = { 0, 0, 0, 0 };
    int bad = 0;
    bad += lnsfaid_fec_status_host(&code, fix.get(), dec.get(), sent.get(), 1, ra.get(), oa, va) != 0;
    bad += lnsfaid_fec_status_packed_host(&code, llr4.get(), bits.get(), sent.get(), 1, rb.get(), ob, vb) != 0;
    bad += memcmp(ra.get(), rb.get(), 32 * sizeof(lnsfaid_fec_record)) != 0;
    bad += memcmp(oa, ob, sizeof(oa)) != 0 || memcmp(va, vb, sizeof(va)) != 0;
    for (size_t m = 0; m < 8; ++m) bad += ra[m].unsatisfied != weight_sum[m];
    for (size_t m = 8; m < 32; ++m) bad += ra[m].unsatisfied < 1200 || ra[m].unsatisfied > 1900;
    bad += oa[0] != 32 || oa[1] != 31 || va[0] != 32 || va[1] + va[3] != 31;
    /* optional arguments, NULL sent, and the calls that must touch nothing */
    uint64_t keep[4];
    memcpy(keep, oa, sizeof(keep));
    bad += lnsfaid_fec_status_host(&code, nullptr, dec.get(), nullptr, 1, nullptr, nullptr, vb) != 0;
    bad += lnsfaid_fec_status_host(&code, fix.get(), nullptr, sent.get(), 1, ra.get(), oa, va) != LNSFAID_E_INVAL;
    bad += lnsfaid_fec_status_host(nullptr, fix.get(), dec.get(), sent.get(), 1, ra.get(), oa, va) != LNSFAID_E_INVAL;
    bad += lnsfaid_fec_status_packed_host(&code, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr) != 0;
    bad += memcmp(keep, oa, sizeof(keep)) != 0;
    printf("unsatisfied of frames 0..9:");
    for (size_t m = 0; m < 10; ++m) printf(" %u", ra[m].unsatisfied);
    printf("\ncorrected of frames 0..3: %u %u %u %u\n", ra[0].corrected, ra[1].corrected, ra[2].corrected, ra[3].corrected);
    printf("out %llu %llu %llu %llu  vs_sent %llu %llu %llu %llu  K %zu\n", (unsigned long long)oa[0], (unsigned long long)oa[1],
           (unsigned long long)oa[2], (unsigned long long)oa[3], (unsigned long long)va[0], (unsigned long long)va[1], (unsigned long long)va[2],
           (unsigned long long)va[3], K);
    printf("fec_status_selftest: %s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
