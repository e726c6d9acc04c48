/* Self-test of the host forms of the burst-format link (no GPU, no liblnsfaid.so: it links ../csrc/lnsfaid_tables.c alone).
 *   burst_link_selftest
 * lnsfaid_burst_payload_random_host, lnsfaid_burst_bsc_host, lnsfaid_burst_soft_host and lnsfaid_burst_count_errors_host run on heap
 * buffers of exactly the sizes lnsfaid_burst_words reports, every one of them (shortened, stats and short_ones included) at an odd
 * address, so that a build with -fsanitize=address,undefined (make burst_link_selftest) sees every access outside them and every
 * misaligned word access.  Checked, for 1, 33 and 65 codewords, TAIL and HEAD:
 *   - payload: lnsfaid_line_payload_random_host's payload with the known words dropped,
 *   - BSC and soft channel: expand with a pattern in the known range, lnsfaid_line_*_host, drop the known words - the same bytes; flips
 *     is the line call's minus what it counted inside the known words,
 *   - shortened == NULL: the line calls' bytes, flips and totals,
 *   - a run cut in two gives the bytes and totals of the one-shot run,
 *   - the counters against a bit loop here, with short_ones > 0 counted as failed,
 *   - refused calls touch nothing. */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "lnsfaid.h"

static unsigned long long g_state = 0x9E3779B97F4A7C15ull;
static unsigned rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(g_state >> 33); }

/* a heap buffer of exactly n bytes that starts at an odd address */
struct Odd {
    std::unique_ptr<uint8_t[]> mem;
    uint8_t* p;
    size_t n;
    explicit Odd(size_t n_) : mem(new uint8_t[n_ + 1]), p(mem.get() + 1), n(n_) {}
    uint32_t* w() const { return (uint32_t*)p; }
};

static unsigned popcount8(const uint8_t* p, size_t n)
{
    unsigned c = 0;
    for (size_t i = 0; i < n; ++i)
        for (unsigned v = p[i]; v; v &= v - 1u) c += 1u;
    return c;
}

int main()
{
    std::unique_ptr<uint16_t[]> pos(new uint16_t[70400]);
    int32_t deg[3], rows[3];
    lnsfaid_code code;
    if (lnsfaid_code_50gpon(&code, pos.get(), deg, rows)) return 2;
    const size_t N = (size_t)code.n_var, K = N - (size_t)code.n_check, L = N - (size_t)code.puncture_tail;
    static const uint32_t short_set[8] = { 0, 32, 224, 256, 288, 5760, 8288, 14560 };
    const uint64_t key = 0x0DDBA11C0FFEEull, first = 0xFFFFFFFFFFFFFFF0ull; /* the codeword number wraps inside the run */
    uint32_t threshold = 0, table[14];
    if (lnsfaid_line_bsc_threshold(0.01, &threshold) || lnsfaid_line_awgn_table(0.66, 9.19, table)) return 2;
    int bad = 0;
    const size_t counts[3] = { 1, 33, 65 };
    for (size_t n : counts)
        for (int32_t where : { LNSFAID_SHORTEN_TAIL, LNSFAID_SHORTEN_HEAD }) {
            Odd sh(4 * n);
            std::unique_ptr<uint32_t[]> S(new uint32_t[n]);
            for (size_t c = 0; c < n; ++c) S[c] = n == 1 ? 14560u : short_set[c % 8];
            memcpy(sh.p, S.get(), 4 * n);
            const uint32_t* shortened = (const uint32_t*)sh.p;
            uint64_t line_bits = 0, payload_bits = 0;
            bad += lnsfaid_burst_words(&code, shortened, n, &line_bits, &payload_bits) != 0;
            const size_t lb = (size_t)line_bits / 8, pb = (size_t)payload_bits / 8;

            /* payload: the line payload without the known words */
            Odd pay(pb), full_pay(n * K / 8);
            bad += lnsfaid_burst_payload_random_host(&code, key, first, shortened, where, n, pay.w()) != 0;
            bad += lnsfaid_line_payload_random_host(&code, key, first, n, full_pay.w()) != 0;
            size_t at = 0, mism = 0;
            for (size_t c = 0; c < n; ++c) {
                const size_t k0 = where == LNSFAID_SHORTEN_HEAD ? 0 : K - S[c], k1 = k0 + S[c];
                for (size_t b = 0; b < K / 8; ++b)
                    if (8 * b < k0 || 8 * b >= k1) mism += pay.p[at++] != full_pay.p[c * (K / 8) + b];
            }
            bad += mism != 0 || at != pb;

            /* channels: expand, run the line call, drop */
            Odd line(lb), full(n * L / 8), out(lb), full_out(n * L / 8), fl(4 * n), full_fl(4 * n);
            Odd soft(4 * lb), full_soft(n * L / 2), sfl(4 * n), full_sfl(4 * n);
            for (size_t i = 0; i < lb; ++i) line.p[i] = (uint8_t)rnd();
            at = 0;
            for (size_t c = 0; c < n; ++c) {
                const size_t k0 = where == LNSFAID_SHORTEN_HEAD ? 0 : K - S[c], k1 = k0 + S[c];
                for (size_t b = 0; b < L / 8; ++b) full.p[c * (L / 8) + b] = (8 * b < k0 || 8 * b >= k1) ? line.p[at++] : (uint8_t)0xC3;
            }
            uint64_t total = 100, full_total = 0, stotal = 200, full_stotal = 0;
            bad += lnsfaid_burst_bsc_host(&code, line.w(), shortened, where, n, key, first, threshold, out.w(), fl.w(), &total) != 0;
            bad += lnsfaid_line_bsc_host(&code, full.w(), n, key, first, threshold, full_out.w(), full_fl.w(), &full_total) != 0;
            bad += lnsfaid_burst_soft_host(&code, line.w(), shortened, where, n, key, first, table, soft.p, sfl.w(), &stotal) != 0;
            bad += lnsfaid_line_soft_host(&code, full.w(), n, key, first, table, full_soft.p, full_sfl.w(), &full_stotal) != 0;
            at = 0;
            mism = 0;
            uint64_t sum = 0, ssum = 0;
            for (size_t c = 0; c < n; ++c) {
                const size_t k0 = where == LNSFAID_SHORTEN_HEAD ? 0 : K - S[c], k1 = k0 + S[c];
                unsigned inside = 0, sinside = 0;
                for (size_t b = 0; b < L / 8; ++b) {
                    const size_t fb = c * (L / 8) + b;
                    if (8 * b < k0 || 8 * b >= k1) {
                        mism += out.p[at] != full_out.p[fb];
                        mism += memcmp(soft.p + 4 * at, full_soft.p + 4 * fb, 4) != 0;
                        at += 1;
                    } else {
                        const uint8_t m = (uint8_t)(full_out.p[fb] ^ full.p[fb]);
                        inside += popcount8(&m, 1);
                        for (unsigned j = 0; j < 8; ++j) { /* the soft channel's flips inside the known range: level > 0 differs from the bit */
                            const int v = (full_soft.p[4 * fb + j / 2] >> (j % 2 ? 4 : 0)) & 15, level = v >= 8 ? v - 16 : v;
                            sinside += (unsigned)((level > 0) != (int)((full.p[fb] >> j) & 1));
                        }
                    }
                }
                uint32_t f, ff, sf, sff;
                memcpy(&f, fl.p + 4 * c, 4); memcpy(&ff, full_fl.p + 4 * c, 4); memcpy(&sf, sfl.p + 4 * c, 4); memcpy(&sff, full_sfl.p + 4 * c, 4);
                mism += f != ff - inside || sf != sff - sinside;
                sum += f; ssum += sf;
            }
            bad += mism != 0 || at != lb || total != 100 + sum || stotal != 200 + ssum || sum == 0 || ssum == 0;

            /* in place */
            Odd work(lb);
            memcpy(work.p, line.p, lb);
            bad += lnsfaid_burst_bsc_host(&code, work.w(), shortened, where, n, key, first, threshold, work.w(), nullptr, nullptr) != 0;
            bad += memcmp(work.p, out.p, lb) != 0;

            /* shortened == NULL: the line calls */
            {
                Odd a(n * L / 8), a4(n * L / 2), p0(n * K / 8), f0(4 * n), f1(4 * n);
                uint64_t t0 = 0, t1 = 0;
                bad += lnsfaid_burst_payload_random_host(&code, key, first, nullptr, where, n, p0.w()) != 0 || memcmp(p0.p, full_pay.p, n * K / 8) != 0;
                bad += lnsfaid_burst_bsc_host(&code, full.w(), nullptr, where, n, key, first, threshold, a.w(), f0.w(), &t0) != 0;
                bad += memcmp(a.p, full_out.p, n * L / 8) != 0 || memcmp(f0.p, full_fl.p, 4 * n) != 0 || t0 != full_total;
                bad += lnsfaid_burst_soft_host(&code, full.w(), nullptr, where, n, key, first, table, a4.p, f1.w(), &t1) != 0;
                bad += memcmp(a4.p, full_soft.p, n * L / 2) != 0 || memcmp(f1.p, full_sfl.p, 4 * n) != 0 || t1 != full_stotal;
            }

            /* counters: got = the payload with planted errors, against a bit loop */
            Odd got(pb), st(sizeof(lnsfaid_line_stats) * n), ones(4 * n);
            memcpy(got.p, pay.p, pb);
            uint64_t want_e[4] = { 0, 0, 0, 0 }, want_f[4] = { 0, 0, 0, 0 }, want_v[4] = { 0, 0, 0, 0 };
            at = 0;
            for (size_t c = 0; c < n; ++c) {
                const size_t bytes = (K - S[c]) / 8;
                const unsigned plan = (unsigned)(c % 5);
                unsigned w = 0;
                for (unsigned e = 0; e < (plan == 4 ? 20u : plan); ++e) { /* distinct bits of the codeword's last payload word */
                    got.p[at + bytes - 4 + e / 8] ^= (uint8_t)(1u << (e % 8));
                    w += 1;
                }
                lnsfaid_line_stats s;
                memset(&s, 0, sizeof(s));
                s.unsatisfied = (c % 4 == 1) ? 7 : (c % 4 == 3) ? 2 : 0;
                s.corrected = (c % 4 == 2) ? 5 : (c % 4 == 3) ? 9 : 0;
                const uint32_t o = c % 3 == 2 ? 2u : 0u;
                memcpy(st.p + sizeof(s) * c, &s, sizeof(s));
                memcpy(ones.p + 4 * c, &o, 4);
                const bool failed = s.unsatisfied > 0 || o > 0;
                want_e[0] += 1; want_e[1] += w > 0; want_e[2] += w; want_e[3] += w == 1 || w == 2;
                want_f[0] += 1; want_f[1] += failed; want_f[2] += !failed && s.corrected > 0; want_f[3] += failed ? 0 : (uint64_t)s.corrected;
                want_v[0] += 1; want_v[1] += w > 0; want_v[2] += w > 0 && !failed; want_v[3] += w == 0 && failed;
                at += bytes;
            }
            uint64_t e[4] = { 1, 2, 3, 4 }, f[4] = { 5, 6, 7, 8 }, v[4] = { 9, 10, 11, 12 };
            bad += lnsfaid_burst_count_errors_host(&code, got.w(), pay.w(), (const lnsfaid_line_stats*)st.p, ones.w(), shortened, n, e, f, v) != 0;
            for (int k = 0; k < 4; ++k) bad += e[k] != 1u + k + want_e[k] || f[k] != 5u + k + want_f[k] || v[k] != 9u + k + want_v[k];

            /* a run cut in two */
            if (n > 20) {
                const size_t cut = 20;
                uint64_t lb1 = 0, pb1 = 0;
                bad += lnsfaid_burst_words(&code, shortened, cut, &lb1, &pb1) != 0;
                lb1 /= 8; pb1 /= 8;
                const uint32_t* sh2 = (const uint32_t*)(sh.p + 4 * cut);
                Odd o1(lb1), o2(lb - lb1), s1(4 * lb1), s2(4 * (lb - lb1)), p1(pb1), p2(pb - pb1);
                uint64_t t = 100, ts = 200;
                bad += lnsfaid_burst_payload_random_host(&code, key, first, shortened, where, cut, p1.w()) != 0;
                bad += lnsfaid_burst_payload_random_host(&code, key, first + cut, sh2, where, n - cut, p2.w()) != 0;
                bad += memcmp(p1.p, pay.p, pb1) != 0 || memcmp(p2.p, pay.p + pb1, pb - pb1) != 0;
                bad += lnsfaid_burst_bsc_host(&code, line.w(), shortened, where, cut, key, first, threshold, o1.w(), nullptr, &t) != 0;
                bad += lnsfaid_burst_bsc_host(&code, (const uint32_t*)(line.p + lb1), sh2, where, n - cut, key, first + cut, threshold, o2.w(), nullptr, &t) != 0;
                bad += memcmp(o1.p, out.p, lb1) != 0 || memcmp(o2.p, out.p + lb1, lb - lb1) != 0 || t != total;
                bad += lnsfaid_burst_soft_host(&code, line.w(), shortened, where, cut, key, first, table, s1.p, nullptr, &ts) != 0;
                bad += lnsfaid_burst_soft_host(&code, (const uint32_t*)(line.p + lb1), sh2, where, n - cut, key, first + cut, table, s2.p, nullptr, &ts) != 0;
                bad += memcmp(s1.p, soft.p, 4 * lb1) != 0 || memcmp(s2.p, soft.p + 4 * lb1, 4 * (lb - lb1)) != 0 || ts != stotal;
                uint64_t e2[4] = { 1, 2, 3, 4 }, f2[4] = { 5, 6, 7, 8 }, v2[4] = { 9, 10, 11, 12 };
                bad += lnsfaid_burst_count_errors_host(&code, got.w(), pay.w(), (const lnsfaid_line_stats*)st.p, ones.w(), shortened, cut, e2, f2, v2) != 0;
                bad += lnsfaid_burst_count_errors_host(&code, (const uint32_t*)(got.p + pb1), (const uint32_t*)(pay.p + pb1),
                                                       (const lnsfaid_line_stats*)(st.p + sizeof(lnsfaid_line_stats) * cut),
                                                       (const uint32_t*)(ones.p + 4 * cut), sh2, n - cut, e2, f2, v2) != 0;
                bad += memcmp(e, e2, sizeof(e)) != 0 || memcmp(f, f2, sizeof(f)) != 0 || memcmp(v, v2, sizeof(v)) != 0;
            }

            /* refusals touch nothing */
            Odd keep_o(lb), keep_s(4 * lb), keep_p(pb);
            memcpy(keep_o.p, out.p, lb); memcpy(keep_s.p, soft.p, 4 * lb); memcpy(keep_p.p, pay.p, pb);
            Odd bad_sh(4 * n);
            memcpy(bad_sh.p, S.get(), 4 * n);
            const uint32_t bad_values[4] = { 31u, (uint32_t)K, (uint32_t)K + 32u, 0xffffffe0u };
            uint64_t t = 7;
            for (uint32_t val : bad_values) {
                memcpy(bad_sh.p + 4 * (n - 1), &val, 4);
                const uint32_t* bs = (const uint32_t*)bad_sh.p;
                bad += lnsfaid_burst_payload_random_host(&code, key, first, bs, where, n, pay.w()) != LNSFAID_E_INVAL;
                bad += lnsfaid_burst_bsc_host(&code, line.w(), bs, where, n, key, first, threshold, out.w(), fl.w(), &t) != LNSFAID_E_INVAL;
                bad += lnsfaid_burst_soft_host(&code, line.w(), bs, where, n, key, first, table, soft.p, sfl.w(), &t) != LNSFAID_E_INVAL;
                bad += lnsfaid_burst_count_errors_host(&code, got.w(), pay.w(), (const lnsfaid_line_stats*)st.p, ones.w(), bs, n, e, f, v) != LNSFAID_E_INVAL;
            }
            bad += lnsfaid_burst_payload_random_host(&code, key, first, shortened, 2, n, pay.w()) != LNSFAID_E_INVAL;
            bad += lnsfaid_burst_bsc_host(&code, line.w(), shortened, -1, n, key, first, threshold, out.w(), fl.w(), &t) != LNSFAID_E_INVAL;
            bad += lnsfaid_burst_soft_host(&code, line.w(), shortened, 7, n, key, first, table, soft.p, sfl.w(), &t) != LNSFAID_E_INVAL;
            bad += lnsfaid_burst_soft_host(&code, (const uint32_t*)soft.p, shortened, where, n, key, first, table, soft.p, sfl.w(), &t) != LNSFAID_E_INVAL;
            bad += lnsfaid_burst_count_errors_host(&code, got.w(), pay.w(), nullptr, ones.w(), shortened, n, e, f, nullptr) != LNSFAID_E_INVAL;
            bad += memcmp(keep_o.p, out.p, lb) != 0 || memcmp(keep_s.p, soft.p, 4 * lb) != 0 || memcmp(keep_p.p, pay.p, pb) != 0 || t != 7;
            for (int k = 0; k < 4; ++k) bad += e[k] != 1u + k + want_e[k] || f[k] != 5u + k + want_f[k] || v[k] != 9u + k + want_v[k];
            printf("%zu codewords, where %d: line %llu bits, payload %llu bits, %llu + %llu flips, %d bad so far\n", n, (int)where,
                   (unsigned long long)line_bits, (unsigned long long)payload_bits, (unsigned long long)sum, (unsigned long long)ssum, bad);
        }
    printf("L %zu K %zu N %zu\nburst_link_selftest: %s\n", L, K, N, bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
