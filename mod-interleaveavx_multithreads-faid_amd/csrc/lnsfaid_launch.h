/*
 * lnsfaid_launch.h - what the kernel files export to the host side of the C ABI (lnsfaid_capi.hip): the decode kernels' instance
 * tables and the launch functions of everything else.  Internal: not part of the public boundary.
 *
 * The symbols have C linkage, so nothing at link time compares a definition with a declaration written elsewhere.  Included by
 * lnsfaid_capi.hip AND by every file that defines one of these functions: the compiler then refuses a definition that disagrees.
 * The decode kernels are launched by lnsfaid_capi.hip itself, on the instance an lf_decode*_func returns with lf_decode*_threads
 * threads per workgroup and one workgroup per codeword.
 */
#ifndef LNSFAID_LAUNCH_H
#define LNSFAID_LAUNCH_H

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "lnsfaid.h"

struct LfDevCode;   /* lnsfaid_device.h */
struct LfBurstDesc; /* lnsfaid_burst.h */

extern "C" {

/* lnsfaid_kernels.hip */
const void* lf_decode_func(int method, int uniform_w);
int lf_decode_threads(void);
hipError_t lf_launch_count_errors(const int8_t* decoded, const int8_t* input_bits, int n_var, int k_info, size_t n_cw,
                                  unsigned long long* out, hipStream_t stream);
/* lnsfaid_kernel4.hip */
const void* lf_decode4_func(int method, int ef, int rm);
int lf_decode4_threads(void);
int lf_decode4_rm_layers(void);
/* lnsfaid_kernel4cw.hip */
const void* lf_decode4cw_func(int method, int ef, int rm);
/* lnsfaid_kernel4p.hip */
const void* lf_decode4p_func(int method, int ef, int rm, int per_codeword);
hipError_t lf_launch_unpack_llr4(const uint8_t* d_llr4, int8_t* d_fix, size_t n_values, hipStream_t stream);
hipError_t lf_launch_pack_bits(const int8_t* d_decoded, uint32_t* d_bits, size_t n_values, hipStream_t stream);
hipError_t lf_launch_count_errors_packed(const uint32_t* d_bits, const uint32_t* d_msg, int n_var, int k_info, size_t n_cw,
                                         unsigned long long* out, hipStream_t stream);
/* lnsfaid_kernel4l.hip, lnsfaid_kernel4b.hip */
const void* lf_decode4l_func(int method, int ef, int rm);
const void* lf_decode4b_func(int method, int ef, int rm);
/* lnsfaid_kernel4z.hip, lnsfaid_kernel4s.hip, lnsfaid_kernel4w.hip, lnsfaid_kernel4e.hip */
int lf_decode4z_inst(int deg, int zg);
const void* lf_decode4z_func(int method);
int lf_decode4s_matches(const LfDevCode* code);
const void* lf_decode4s_func(int method);
const void* lf_decode4w_func(int method);
const void* lf_decode4e_func(int method);
/* lnsfaid_kernel5.hip */
const void* lf_decode5_func(int method);
int lf_decode5_threads(void);

/* lnsfaid_frontend.hip */
hipError_t lf_launch_frontend(const uint32_t* d_seeds, const unsigned long long* d_draws, int n_streams, int mod_type, float sigma_ch,
                              float scale, const int8_t* d_codeword, const int8_t* d_frames, int n_var, int n_check, int interleave,
                              int fast, int8_t* d_fix, int count_limit, unsigned long long* d_frame_cnt, hipStream_t stream);
hipError_t lf_frontend_fastpath_scan(double* d_out2, hipStream_t stream);
void lf_frontend_fastpath_assumed(double* eps2);
/* lnsfaid_prefec.hip */
hipError_t lf_launch_prefec(const float* d_rx, const int8_t* d_sent, size_t n_groups, int mod_type, int n_var, int n_check,
                            int interleave, int scope, unsigned long long* d_out, hipStream_t stream);
hipError_t lf_launch_prefec_fold(unsigned long long* d_frame_cnt, size_t n_streams, unsigned long long* d_acc, hipStream_t stream);
/* lnsfaid_capture.hip */
hipError_t lf_launch_capture(const int8_t* d_fix, const int8_t* d_decoded, const int8_t* d_sent, size_t n_groups, int n_var, int n_check,
                             uint32_t skip, uint32_t cap, uint2* d_cnt, uint32_t* d_slots, lnsfaid_error_record* d_records,
                             int8_t* d_payload, unsigned long long* d_meta, unsigned long long* d_out, hipStream_t stream);
/* lnsfaid_fecstatus.hip */
hipError_t lf_launch_fec_status(const LfDevCode* d_code, int n_var, int packed, const void* d_fix, const void* d_decided,
                                const int8_t* d_sent, size_t n_groups, lnsfaid_fec_record* d_records, int want_sent,
                                unsigned long long* d_acc, hipStream_t stream);
/* lnsfaid_demap.hip */
hipError_t lf_launch_demap(const float* d_rx, size_t n_groups, int mod_type, float scale, int n_var, int n_check, int interleave,
                           int packed, void* d_out, hipStream_t stream);
/* lnsfaid_encoder.hip, lnsfaid_encoder_line.hip, lnsfaid_encoder_burst.hip */
hipError_t lf_launch_encode(const LfDevCode* d_code, int n_check, const uint32_t* d_bsup, const uint32_t* d_bsup_off, const int8_t* d_in,
                            const unsigned long long* d_keys, size_t n_groups, int8_t* d_out, int8_t* d_info, hipStream_t stream);
hipError_t lf_launch_encode_line(const LfDevCode* d_code, int n_check, const uint32_t* d_bsup, const uint32_t* d_bsup_off,
                                 const uint32_t* d_payload, size_t n_codewords, uint32_t* d_line, uint32_t* d_bits, hipStream_t stream);
hipError_t lf_launch_encode_burst(const LfDevCode* d_code, int n_check, const uint32_t* d_bsup, const uint32_t* d_bsup_off,
                                  const uint32_t* d_payload, const LfBurstDesc* d_desc, int where, size_t n_codewords, uint32_t* d_line,
                                  uint32_t* d_bits, hipStream_t stream);
/* lnsfaid_line_link.hip */
hipError_t lf_launch_line_bsc(const uint32_t* d_in, uint32_t* d_out, size_t n_cw, uint32_t lw, uint64_t key, uint64_t first,
                              uint32_t threshold, uint32_t* d_flips, unsigned long long* d_total, hipStream_t stream);
hipError_t lf_launch_line_payload(uint32_t* d_payload, size_t n_cw, uint32_t kw, uint64_t key, uint64_t first, hipStream_t stream);
hipError_t lf_launch_line_count(const uint32_t* d_payload, const uint32_t* d_sent, const lnsfaid_line_stats* d_stats, size_t n_cw,
                                uint32_t kw, unsigned long long* d_acc, hipStream_t stream);
/* lnsfaid_line_soft.hip, lnsfaid_line_markov.hip */
hipError_t lf_launch_line_soft(const uint32_t* d_in, uint8_t* d_out, size_t n_cw, uint32_t lw, uint64_t key, uint64_t first,
                               const uint32_t table[14], uint32_t* d_flips, unsigned long long* d_total, hipStream_t stream);
hipError_t lf_launch_line_markov(const uint32_t* d_in, uint32_t* d_out, size_t n_cw, uint32_t lw, uint64_t key, uint64_t first,
                                 const uint32_t t[3], uint32_t* d_flips, uint32_t* d_runs, unsigned long long* d_totals,
                                 hipStream_t stream);
/* lnsfaid_burst_link.hip.  The caller has checked the rules of include/lnsfaid.h and uploaded d_desc[n_cw] on `stream`
 * (burst_descriptors): n_cw > 0, the pointers on 4 bytes, where TAIL or HEAD.  lw = L / 32, kw = K / 32.  d_total: one counter, ADDED
 * to; d_acc: twelve, ADDED to. */
hipError_t lf_launch_burst_payload(uint32_t* d_payload, const LfBurstDesc* d_desc, int where, size_t n_cw, uint32_t kw, uint64_t key,
                                   uint64_t first, hipStream_t stream);
hipError_t lf_launch_burst_bsc(const uint32_t* d_in, uint32_t* d_out, const LfBurstDesc* d_desc, int where, size_t n_cw, uint32_t lw,
                               uint32_t kw, uint64_t key, uint64_t first, uint32_t threshold, uint32_t* d_flips,
                               unsigned long long* d_total, hipStream_t stream);
hipError_t lf_launch_burst_soft(const uint32_t* d_in, uint8_t* d_out, const LfBurstDesc* d_desc, int where, size_t n_cw, uint32_t lw,
                                uint32_t kw, uint64_t key, uint64_t first, const uint32_t table[14], uint32_t* d_flips,
                                unsigned long long* d_total, hipStream_t stream);
hipError_t lf_launch_burst_count(const uint32_t* d_payload, const uint32_t* d_sent, const lnsfaid_line_stats* d_stats,
                                 const uint32_t* d_short_ones, const LfBurstDesc* d_desc, size_t n_cw, uint32_t kw,
                                 unsigned long long* d_acc, hipStream_t stream);
/* lnsfaid_line_capture.hip */
hipError_t lf_launch_line_capture(const LfDevCode* d_code, int n_var, int puncture_tail, const void* d_line, int format,
                                  const uint32_t* d_bits, const uint32_t* d_sent, size_t n_cw, uint64_t first, int select, uint32_t skip,
                                  uint32_t cap, uint4* d_cnt, uint32_t* d_slots, lnsfaid_line_failure* d_records, uint32_t* d_payload,
                                  unsigned long long* d_meta, hipStream_t stream);

} /* extern "C" */

#endif /* LNSFAID_LAUNCH_H */
