/* lnsfaid_line_sim - hard-decision sweep of the 50G-PON code on the line's own formats, on one GPU (include/lnsfaid.h "line-format
 * link"): per input bit error rate and call
 *   lnsfaid_line_payload_random_device -> lnsfaid_encode_line_device -> lnsfaid_line_bsc_device (in place) ->
 *   lnsfaid_decode_line_device (LNSFAID_LINE_HARD) -> lnsfaid_line_count_errors_device
 * or, with --ebn0 in place of --ber, the soft-decision sweep (include/lnsfaid.h "line-format soft channel"): per Eb/N0
 *   ... -> lnsfaid_encode_line_device -> lnsfaid_line_soft_device (table of lnsfaid_line_awgn_table) ->
 *   lnsfaid_decode_line_device (LNSFAID_LINE_LLR4) -> lnsfaid_line_count_errors_device
 * or, with --ber and --propagation A, the hard sweep through the channel with memory (include/lnsfaid.h "line-format error-propagation
 * channel"): lnsfaid_line_markov_device with lnsfaid_line_markov_thresholds(p, max(A, p)) in place of the BSC call,
 * on the device buffers of one context (lnsfaid_io_buffers, carved up below): no bit crosses to the host, only the counters do.
 * first_codeword continues across calls and points, so a run is one stream of codewords of the key.  A point stops at --min-errors
 * error frames or after --max-calls calls.  One row per point goes to LineResult.txt (in the working directory) and to the console.
 * With --capture-failures CAPACITY (include/lnsfaid.h "line-format failure capture") the encode and decode calls also
 * write their `bits`, and after the counters of every call lnsfaid_line_capture_device pages through the codewords that are
 * uncorrectable or wrong, CAPACITY records at a time; one text row per failure is appended to --capture-file (LineFailures.txt).
 * With --burst-length B --shorten S[,S...] [--where tail|head] (include/lnsfaid.h "burst-format link") the run is bursts
 * of B codewords: the last codeword of burst j is shortened by S[j % len] bits and all others by 0 - a function of the global codeword
 * number alone, so a run cut into calls is the same run - and every call is the burst form:
 *   lnsfaid_burst_payload_random_device -> lnsfaid_encode_burst_device -> lnsfaid_burst_bsc_device | lnsfaid_burst_soft_device ->
 *   lnsfaid_decode_burst_device -> lnsfaid_burst_count_errors_device
 * The input BER is then taken over transmitted bits and the output BER over payload bits, and three columns are appended to a row:
 * transmitted bits, payload bits, codewords with short_ones > 0.  Not with --propagation or --capture-failures. */
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "lnsfaid.h"

static const char* kUsage =
    "usage: %s --ber P[,P...] [--magnitude 4] [--propagation A] | --ebn0 D[,D...] [--scale 9.19238816] --codewords N --max-calls C --min-errors E [--method 2] [--iterations 10] [--key K] [--device D] [--capture-failures CAPACITY [--capture-file LineFailures.txt]] [--burst-length B --shorten S[,S...] [--where tail|head]]\n";

static bool parse_u64(const char* s, uint64_t* v)
{
    if (!*s || *s == '-') return false;
    char* end = nullptr;
    *v = strtoull(s, &end, 0);
    return end && *end == '\0';
}

static bool parse_ber(const char* s, std::vector<double>* out)
{
    const char* p = s;
    while (true) {
        char* end = nullptr;
        const double v = strtod(p, &end);
        uint32_t t;
        if (end == p || lnsfaid_line_bsc_threshold(v, &t) != LNSFAID_OK) return false;
        out->push_back(v);
        if (*end == '\0') return true;
        if (*end != ',') return false;
        p = end + 1;
    }
}

static bool parse_ebn0(const char* s, std::vector<double>* out)
{
    const char* p = s;
    while (true) {
        char* end = nullptr;
        const double v = strtod(p, &end);
        if (end == p || !std::isfinite(v)) return false;
        out->push_back(v);
        if (*end == '\0') return true;
        if (*end != ',') return false;
        p = end + 1;
    }
}

static bool parse_shorten(const char* s, std::vector<uint32_t>* out)
{
    const char* p = s;
    while (true) {
        char* end = nullptr;
        if (*p < '0' || *p > '9') return false;
        const unsigned long long v = strtoull(p, &end, 10);
        if (end == p || v > 0xffffffffull) return false; /* the rule S % 32 == 0, S <= K - 32 is the library's: checked below */
        out->push_back((uint32_t)v);
        if (*end == '\0') return true;
        if (*end != ',') return false;
        p = end + 1;
    }
}

static bool parse_scale(const char* s, double* v)
{
    char* end = nullptr;
    *v = strtod(s, &end);
    return end != s && *end == '\0' && std::isfinite(*v) && *v > 0.0;
}

static bool parse_propagation(const char* s, double* v)
{
    char* end = nullptr;
    *v = strtod(s, &end);
    return end != s && *end == '\0' && *v >= 0.0 && *v < 1.0; /* NaN fails the comparisons */
}

static size_t align256(size_t x) { return (x + 255u) & ~(size_t)255u; }

/* " ; " and the ascending indices of the set bits of a record section */
static void print_set_bits(FILE* f, const uint32_t* words, size_t n_words)
{
    fputs(" ;", f);
    for (size_t w = 0; w < n_words; ++w)
        for (uint32_t v = words[w]; v; v &= v - 1u) fprintf(f, " %zu", 32 * w + (size_t)__builtin_ctz(v));
}

int main(int argc, char** argv)
{
    std::vector<double> ber, ebn0;
    double scale = 13.0 / std::sqrt(2.0); /* the QPSK operating scale 13 on a unit-amplitude axis */
    double propagation = 0.0;
    bool have_magnitude = false, have_scale = false, markov = false;
    uint64_t codewords = 0, max_calls = 0, min_errors = 0, method = 2, iterations = 10, magnitude = 4, key = 1, device = 0;
    uint64_t capture = 0; /* --capture-failures: records per page, 0 = off */
    const char* capture_file = nullptr;
    uint64_t burst_length = 0; /* --burst-length: codewords per burst, 0 = the line formats */
    std::vector<uint32_t> shorten;
    int32_t where = LNSFAID_SHORTEN_TAIL;
    bool have_where = false;
    bool have[4] = { false, false, false, false }, ok = true;
    for (int i = 1; i < argc && ok; ++i) {
        const char* a = argv[i];
        const char* v = i + 1 < argc ? argv[i + 1] : nullptr;
        if (!v) ok = false;
        else if (!strcmp(a, "--ber")) have[0] = ok = parse_ber(v, &ber);
        else if (!strcmp(a, "--ebn0")) ok = parse_ebn0(v, &ebn0);
        else if (!strcmp(a, "--scale")) have_scale = ok = parse_scale(v, &scale);
        else if (!strcmp(a, "--propagation")) markov = ok = parse_propagation(v, &propagation);
        else if (!strcmp(a, "--codewords")) have[1] = ok = parse_u64(v, &codewords) && codewords > 0 && codewords <= 0x7fffffffull;
        else if (!strcmp(a, "--max-calls")) have[2] = ok = parse_u64(v, &max_calls) && max_calls > 0;
        else if (!strcmp(a, "--min-errors")) have[3] = ok = parse_u64(v, &min_errors);
        else if (!strcmp(a, "--method")) ok = parse_u64(v, &method) && method <= 5;
        else if (!strcmp(a, "--iterations")) ok = parse_u64(v, &iterations) && iterations > 0 && iterations <= 1000;
        else if (!strcmp(a, "--magnitude")) have_magnitude = ok = parse_u64(v, &magnitude) && magnitude >= 1 && magnitude <= 7;
        else if (!strcmp(a, "--key")) ok = parse_u64(v, &key);
        else if (!strcmp(a, "--device")) ok = parse_u64(v, &device) && device < 1024;
        else if (!strcmp(a, "--capture-failures")) ok = parse_u64(v, &capture) && capture > 0 && capture <= 0x7fffffffull;
        else if (!strcmp(a, "--capture-file")) ok = *(capture_file = v) != '\0';
        else if (!strcmp(a, "--burst-length")) ok = parse_u64(v, &burst_length) && burst_length > 0;
        else if (!strcmp(a, "--shorten")) ok = shorten.empty() && parse_shorten(v, &shorten);
        else if (!strcmp(a, "--where")) {
            have_where = ok = !strcmp(v, "tail") || !strcmp(v, "head");
            where = !strcmp(v, "head") ? LNSFAID_SHORTEN_HEAD : LNSFAID_SHORTEN_TAIL;
        }
        else ok = false;
        ++i;
    }
    const bool soft = !ebn0.empty();
    if (soft) have[0] = ber.empty() && !have_magnitude && !markov; /* exactly one of --ber and --ebn0; --magnitude and --propagation belong to --ber */
    else if (have_scale) ok = false;                    /* and --scale to --ebn0 */
    if (capture_file && !capture) ok = false;           /* and --capture-file to --capture-failures */
    if (capture && !capture_file) capture_file = "LineFailures.txt";
    const bool burst = burst_length > 0;
    if (burst ? (shorten.empty() || markov || capture) : (!shorten.empty() || have_where)) ok = false; /* the three belong together */
    if (!ok || !have[0] || !have[1] || !have[2] || !have[3]) {
        fprintf(stderr, kUsage, argv[0]);
        return 2;
    }

    std::unique_ptr<uint16_t[]> pos(new uint16_t[70400]);
    int32_t deg[3], rows[3];
    lnsfaid_code code;
    lnsfaid_cfg cfg;
    lnsfaid_ctx* ctx = nullptr;
    int rc = lnsfaid_code_50gpon(&code, pos.get(), deg, rows);
    if (!rc) rc = lnsfaid_cfg_default(&cfg, (int32_t)method, (int32_t)iterations);
    const size_t n = (size_t)codewords, groups = (n + LNSFAID_GROUP - 1) / LNSFAID_GROUP;
    if (!rc && burst && lnsfaid_burst_words(&code, shorten.data(), shorten.size(), nullptr, nullptr)) { /* S % 32 == 0, S <= K - 32 */
        fprintf(stderr, kUsage, argv[0]);
        return 2;
    }
    if (!rc) rc = lnsfaid_create(&ctx, &code, &cfg, (int32_t)device, groups);
    int8_t *d_a = nullptr, *d_b = nullptr;
    if (!rc) rc = lnsfaid_io_buffers(ctx, &d_a, &d_b, nullptr);
    if (rc) {
        fprintf(stderr, "lnsfaid_line_sim: set-up failed: %s (%s)\n", lnsfaid_strerror(rc), lnsfaid_last_hip_error());
        lnsfaid_destroy(ctx);
        return 1;
    }
    /* each of the two buffers holds 32 * n_var bytes per group; the five streams need (2 K + L) / 8 + 20 bytes per codeword, the
     * LLR4 line of the soft sweep L / 2 more, behind the hard line; with --capture-failures the sent words and the decisions, N / 8
     * each, come last in either buffer; with --propagation the runs per codeword lie behind the flips */
    const size_t K = (size_t)(code.n_var - code.n_check), L = (size_t)(code.n_var - code.puncture_tail), N = (size_t)code.n_var;
    const size_t room = groups * LNSFAID_GROUP * N;
    const size_t o_line = align256(n * K / 8), o_llr4 = o_line + align256(n * L / 8), o_flips = o_llr4 + (soft ? align256(n * L / 2) : 0),
                 o_stats = align256(n * K / 8);
    const size_t o_runs = o_flips + align256(4 * n);
    const size_t o_sent = o_runs + (markov ? align256(4 * n) : 0), o_bits = o_stats + align256(sizeof(lnsfaid_line_stats) * n);
    const size_t o_ones = o_bits; /* --burst-length: short_ones behind the stats (no --capture-failures then) */
    if (o_flips + 4 * n > room || (markov && o_runs + 4 * n > room) || o_stats + sizeof(lnsfaid_line_stats) * n > room ||
        (capture && (o_sent + n * N / 8 > room || o_bits + n * N / 8 > room)) || (burst && o_ones + 4 * n > room)) {
        fprintf(stderr, "lnsfaid_line_sim: the context's buffers are too small for this code\n");
        lnsfaid_destroy(ctx);
        return 1;
    }
    uint32_t* d_payload = (uint32_t*)d_a;
    uint32_t* d_line = (uint32_t*)(d_a + o_line);
    uint8_t* d_llr4 = (uint8_t*)(d_a + o_llr4);
    uint32_t* d_flips = (uint32_t*)(d_a + o_flips);
    uint32_t* d_runs = markov ? (uint32_t*)(d_a + o_runs) : nullptr;
    uint32_t* d_decoded = (uint32_t*)d_b;
    lnsfaid_line_stats* d_stats = (lnsfaid_line_stats*)(d_b + o_stats);
    uint32_t* d_sent = capture ? (uint32_t*)(d_a + o_sent) : nullptr;  /* the encode call's bits */
    uint32_t* d_bits = capture ? (uint32_t*)(d_b + o_bits) : nullptr;  /* the decode call's bits */
    uint32_t* d_ones = burst ? (uint32_t*)(d_b + o_ones) : nullptr;    /* the burst decode's short_ones */
    /* the call's S_c, and S = K - 32 for all: with it short_ones [n] reads as a burst payload of one word per codeword, and
     * ErrorFrame of the counters against the all-zero payload is the number of codewords with short_ones > 0 */
    std::vector<uint32_t> shortened(burst ? n : 0), one_word(burst ? n : 0, (uint32_t)K - 32u);
    const int32_t format = soft ? LNSFAID_LINE_LLR4 : LNSFAID_LINE_HARD;
    const size_t page = capture < n ? (size_t)capture : n;
    uint32_t W = 0;
    std::vector<lnsfaid_line_failure> records;
    std::vector<uint32_t> sections;
    FILE* ff = nullptr;
    if (capture) {
        rc = lnsfaid_line_capture_words(&code, format, &W);
        if (!rc) {
            records.resize(page);
            sections.resize(page * (size_t)W);
            ff = fopen(capture_file, "w");
        }
        if (!ff) {
            fprintf(stderr, "lnsfaid_line_sim: cannot write %s\n", capture_file);
            lnsfaid_destroy(ctx);
            return 1;
        }
        fprintf(ff, "# %s codeword index flags unsatisfied wrong_payload wrong_parity channel_errors ; wrong positions ; unsatisfied rows\n",
                soft ? "ebn0_db" : "p");
    }

    FILE* f = fopen("LineResult.txt", "w");
    if (!f) {
        fprintf(stderr, "lnsfaid_line_sim: cannot write LineResult.txt\n");
        if (ff) fclose(ff);
        lnsfaid_destroy(ctx);
        return 1;
    }
    const char* head = "# p threshold codewords flipped_bits ber_in TestFrame ErrorFrame ErrorBits LT3ErrBitFrame FER ber_out "
                       "TotalCodewords UncorrectableCodewords CorrectedCodewords CorrectedBits "
                       "vsTestFrame vsErrorFrame UndetectedErrorFrame FalseAlarmFrame seconds\n";
    const char* soft_head = "# ebn0_db table7 codewords flipped_bits ber_in TestFrame ErrorFrame ErrorBits LT3ErrBitFrame FER ber_out "
                            "TotalCodewords UncorrectableCodewords CorrectedCodewords CorrectedBits "
                            "vsTestFrame vsErrorFrame UndetectedErrorFrame FalseAlarmFrame seconds sigma scale\n";
    const char* markov_head = "# p threshold codewords flipped_bits ber_in TestFrame ErrorFrame ErrorBits LT3ErrBitFrame FER ber_out "
                              "TotalCodewords UncorrectableCodewords CorrectedCodewords CorrectedBits "
                              "vsTestFrame vsErrorFrame UndetectedErrorFrame FalseAlarmFrame seconds propagation t_idle t_after runs mean_run\n";
    if (markov) head = markov_head;
    std::string burst_head;
    if (burst) {
        burst_head = std::string(soft ? soft_head : head);
        burst_head.replace(burst_head.size() - 1, 1, " transmitted_bits payload_bits ShortOnesCodewords\n");
        fprintf(f, "# lnsfaid_line_sim: bursts of %llu codewords, the last shortened by", (unsigned long long)burst_length);
        for (size_t i = 0; i < shorten.size(); ++i) fprintf(f, "%s%u", i ? "," : " ", shorten[i]);
        fprintf(f, " bits at the %s\n", where == LNSFAID_SHORTEN_HEAD ? "head" : "tail");
    }
    if (soft) {
        head = soft_head;
        if (burst) head = burst_head.c_str();
        fprintf(f, "# lnsfaid_line_sim: soft, DecodeMethod %llu, %llu iterations, scale %.9g, key %llu, %zu codewords per call\n%s",
                (unsigned long long)method, (unsigned long long)iterations, scale, (unsigned long long)key, n, head);
    } else {
        if (burst) head = burst_head.c_str();
        fprintf(f, "# lnsfaid_line_sim: DecodeMethod %llu, %llu iterations, magnitude %llu, key %llu, %zu codewords per call\n%s",
                (unsigned long long)method, (unsigned long long)iterations, (unsigned long long)magnitude, (unsigned long long)key, n, head);
    }
    printf("%s", head);
    uint64_t first = 0;
    for (const double x : soft ? ebn0 : ber) { /* x: Eb/N0 in dB, or the BSC's p */
        uint32_t threshold = 0, table[14], mt[3] = { 0, 0, 0 };
        /* Eb/N0 of the information bit on a unit-amplitude axis: sigma^2 = 1 / (2 R Eb/N0), R = K / L the rate on the line */
        const double sigma = soft ? 1.0 / std::sqrt(2.0 * ((double)K / (double)L) * std::pow(10.0, x / 10.0)) : 0.0;
        if (soft) rc = lnsfaid_line_awgn_table(sigma, scale, table);
        else lnsfaid_line_bsc_threshold(x, &threshold); /* checked with the arguments */
        const double a = propagation > x ? propagation : x; /* positive correlation only: below p the channel is the BSC */
        if (markov) rc = lnsfaid_line_markov_thresholds(x, a, mt); /* mt[2], the threshold of the marginal BER, is `threshold` */
        uint64_t errors[4] = { 0, 0, 0, 0 }, fec[4] = { 0, 0, 0, 0 }, vs[4] = { 0, 0, 0, 0 }, flips = 0, runs = 0;
        uint64_t sent_bits = 0, payload_bits = 0, ones[4] = { 0, 0, 0, 0 }; /* --burst-length: the denominators, short_ones > 0 in ones[1] */
        const auto t0 = std::chrono::steady_clock::now();
        for (uint64_t call = 0; burst && call < max_calls && !rc && errors[1] < min_errors; ++call, first += n) {
            for (size_t i = 0; i < n; ++i) { /* the last codeword of burst j = C / B is shortened by S[j % len] */
                const uint64_t C = first + i;
                shortened[i] = C % burst_length == burst_length - 1 ? shorten[(size_t)((C / burst_length) % shorten.size())] : 0u;
            }
            const uint32_t* sh = shortened.data();
            uint64_t lb = 0, pb = 0;
            rc = lnsfaid_burst_words(&code, sh, n, &lb, &pb);
            if (!rc) rc = lnsfaid_burst_payload_random_device(ctx, key, first, sh, where, n, d_payload);
            if (!rc) rc = lnsfaid_encode_burst_device(ctx, d_payload, sh, where, n, d_line, nullptr);
            if (soft) {
                if (!rc) rc = lnsfaid_burst_soft_device(ctx, d_line, sh, where, n, key, first, table, d_llr4, d_flips, &flips);
                if (!rc) rc = lnsfaid_decode_burst_device(ctx, d_llr4, LNSFAID_LINE_LLR4, 0, sh, where, n, d_decoded, nullptr, d_stats, d_ones);
            } else {
                if (!rc) rc = lnsfaid_burst_bsc_device(ctx, d_line, sh, where, n, key, first, threshold, d_line, d_flips, &flips);
                if (!rc) rc = lnsfaid_decode_burst_device(ctx, d_line, LNSFAID_LINE_HARD, (int32_t)magnitude, sh, where, n, d_decoded, nullptr,
                                                          d_stats, d_ones);
            }
            if (!rc) rc = lnsfaid_burst_count_errors_device(ctx, d_decoded, d_payload, d_stats, d_ones, sh, n, errors, fec, vs);
            if (!rc) rc = lnsfaid_burst_count_errors_device(ctx, d_ones, nullptr, nullptr, nullptr, one_word.data(), n, ones, nullptr, nullptr);
            sent_bits += lb;
            payload_bits += pb;
        }
        for (uint64_t call = 0; !burst && call < max_calls && !rc && errors[1] < min_errors; ++call, first += n) {
            rc = lnsfaid_line_payload_random_device(ctx, key, first, n, d_payload);
            if (!rc) rc = lnsfaid_encode_line_device(ctx, d_payload, n, d_line, d_sent);
            if (soft) {
                if (!rc) rc = lnsfaid_line_soft_device(ctx, d_line, n, key, first, table, d_llr4, d_flips, &flips);
                if (!rc) rc = lnsfaid_decode_line_device(ctx, d_llr4, LNSFAID_LINE_LLR4, 0, n, d_decoded, d_bits, d_stats);
            } else {
                if (!rc && markov) rc = lnsfaid_line_markov_device(ctx, d_line, n, key, first, mt, d_line, d_flips, d_runs, &flips, &runs);
                else if (!rc) rc = lnsfaid_line_bsc_device(ctx, d_line, n, key, first, threshold, d_line, d_flips, &flips);
                if (!rc) rc = lnsfaid_decode_line_device(ctx, d_line, LNSFAID_LINE_HARD, (int32_t)magnitude, n, d_decoded, d_bits, d_stats);
            }
            if (!rc) rc = lnsfaid_line_count_errors_device(ctx, d_decoded, d_payload, d_stats, n, errors, fec, vs);
            uint64_t found = 0, stored = 0;
            for (size_t skip = 0; capture && !rc && (skip == 0 || skip < found); skip += page) {
                rc = lnsfaid_line_capture_device(ctx, soft ? (const void*)d_llr4 : (const void*)d_line, format, d_bits, d_sent, n, first,
                                                 LNSFAID_LINE_CAPTURE_UNCORRECTABLE | LNSFAID_LINE_CAPTURE_WRONG, skip, page, records.data(),
                                                 sections.data(), &found, &stored);
                for (size_t s = 0; !rc && s < stored; ++s) {
                    const lnsfaid_line_failure& r = records[s];
                    const uint32_t* error = sections.data() + s * (size_t)W + (W - 2 * N / 32 - (N - K) / 32) + N / 32;
                    fprintf(ff, "%.9g %llu %u %u %u %u %u %u", x, (unsigned long long)r.codeword, r.index, r.flags, r.unsatisfied, r.wrong_payload,
                            r.wrong_parity, r.channel_errors);
                    print_set_bits(ff, error, N / 32);
                    print_set_bits(ff, error + N / 32, (N - K) / 32);
                    fputc('\n', ff);
                }
            }
            if (ff) fflush(ff);
        }
        if (rc) break;
        const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        const double cw = (double)errors[0];
        char row[704];
        int len = snprintf(row, sizeof(row), "%.9g %u %llu %llu %.6e %llu %llu %llu %llu %.6e %.6e %llu %llu %llu %llu %llu %llu %llu %llu %.3f", x,
                           soft ? table[7] : threshold, (unsigned long long)errors[0], (unsigned long long)flips,
                           burst ? (sent_bits ? (double)flips / (double)sent_bits : 0.0) : cw > 0 ? (double)flips / (cw * (double)L) : 0.0,
                           (unsigned long long)errors[0], (unsigned long long)errors[1], (unsigned long long)errors[2], (unsigned long long)errors[3],
                           cw > 0 ? (double)errors[1] / cw : 0.0, burst ? (payload_bits ? (double)errors[2] / (double)payload_bits : 0.0) : cw > 0 ? (double)errors[2] / (cw * (double)K) : 0.0,
                           (unsigned long long)fec[0], (unsigned long long)fec[1], (unsigned long long)fec[2], (unsigned long long)fec[3],
                           (unsigned long long)vs[0], (unsigned long long)vs[1], (unsigned long long)vs[2], (unsigned long long)vs[3], seconds);
        if (soft) len += snprintf(row + len, sizeof(row) - (size_t)len, " %.9g %.9g", sigma, scale);
        if (markov)
            len += snprintf(row + len, sizeof(row) - (size_t)len, " %.9g %u %u %llu %.6f", a, mt[0], mt[1], (unsigned long long)runs,
                            runs ? (double)flips / (double)runs : 0.0);
        if (burst)
            len += snprintf(row + len, sizeof(row) - (size_t)len, " %llu %llu %llu", (unsigned long long)sent_bits, (unsigned long long)payload_bits,
                            (unsigned long long)ones[1]);
        snprintf(row + len, sizeof(row) - (size_t)len, "\n");
        fputs(row, f);
        fflush(f);
        fputs(row, stdout);
        fflush(stdout);
    }
    fclose(f);
    if (ff) fclose(ff);
    if (rc) fprintf(stderr, "lnsfaid_line_sim: a call failed: %s (%s)\n", lnsfaid_strerror(rc), lnsfaid_last_hip_error());
    lnsfaid_destroy(ctx);
    return rc ? 1 : 0;
}
