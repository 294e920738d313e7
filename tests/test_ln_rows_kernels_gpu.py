"""The stand-alone LayerNorm family and the row helpers of csrc/a4r_rows.hip against the fp64 reference of tests/ln_rows_ref.py at their launch
edges, on the cases tests/test_ln_rows_ref_cpu.py proves sound: every tensor with a leading dimension a view into a wider buffer (ld = H + 8, or
H + 64 starting 32 columns in), junk in gap columns and pad rows, every output pre-filled with a sentinel that must survive outside rows < M and
columns < H, column sums started from 0.5 inside an arena of sentinels.  Bounds: ln_rows_ref.judge (its header states them).  References are
computed on the device in fp64, once per case.

WHICH KERNEL (the third column of every line: ln_rows_ref.branch, the dispatch conditions of a4r_ln_fwd / a4r_ln_bwd restated).
    ln_fwd_lean_kernel      w_fwd_lean_*, r_fwd_lean_*, c_fwd_*                 ln_bwd_lean_kernel   w_bwd_lean_*
    ln_fwd_kernel           w_fwd_gen_*, r_fwd_gen_*, f_fwd_*, w_fp8_*, f_fp8_* ln_bwd_pg_kernel     r_bwd_pg_* at M >= 2048
    ln_fwd_sum_kernel       w_sum_*, f_sum_*, c_sum_*                           ln_bwd_kernel<T, WGB, WDB>: f_bwd_*_sums_* (all four), w_bwd_gen_*,
    quant_rows_fp8_kernel   w_quant_*                                                                r_bwd_gen_*, r_bwd_pg_*_2047_* (one row short of pg)
G = the CU count: the pg kernel's grid is min(ceil(M / 8), G) workgroups of 8 waves, so 8 G + 1 and 16 G + 5 rows give some waves a second and
a third row; the lean kernels' grid is at most 8 workgroups per CU x 4 rows = 8192 rows at 256 CUs; the general backward's 1024 x 4.

HELPERS.  a4r_gather_rows / a4r_scatter_rows / a4r_scatter_rows_fill / a4r_rows_idx_copy: bit-equal with torch indexing on strided views, sentinels
intact, one case each past the grid cap (2048 or 4096 blocks of 256 threads, one 16-byte piece per thread and round).  a4r_dropout_apply: bit-equal
with x * keep * ks of the host mask (one fp32 product, rounded once to the element type).  a4r_act_bwd_f32 against fp64 act'(pre) dy at
n = 524 288 + 5 (a second round of the 2048-block grid, a ragged last block): |dx - ref| <= |dy| (E_act + 2^-23 |act'|).  2^-23 |act'| is the
product's own rounding (2^-24) and that of the constant 0.01f (below 2^-25).  E_1 = E_4 = 0 (act' is a constant chosen by a comparison);
E_3 = 2^-20 (a dozen fp32 roundings of intermediates of unit size, tanhf within 2 ulp); E_2 = 2^-20 + 1.5e-7 (the erf of csrc/a4r_common.h is
Abramowitz & Stegun 7.1.26, whose published maximum error is 1.5e-7).

REJECTIONS.  Every launch guard of the C entry points has a call that trips it; the entry point returns A4R_EINVAL before anything is launched.

MEASURED on an MI355X (G = 256; the KERNEL lines the tests print).  Per case: M; the kernel; then per output its worst error over its bound and, in
brackets, bf16 tensors: maximum error kernel / model (the figure in front is the tile RMS over twice the model's: 0.50 = the model's own); fp32
tensors: the maximum error; column sums: the worst error in units u = 2^-24 (0.5 + sum |term|) (bound 16 u); keep / keep2: elements whose
zero / non-zero state differs from the host mask.
Wall time of the whole file: 3.7 s (412 tests; the slowest, the first launch of the process aside, 0.24 s: the host mask of 8200 x 1032 elements).
Within 20 % of a bound (marked NEAR): y8 alone, at 0.89 .. 0.94 in every case that has one -- by construction: its bound is the e4m3 format's own
worst-case rounding (half an ulp of 3 mantissa bits), which some element of every row comes close to.  Nothing else: no bf16 tensor (every tile RMS
is the model's own, 0.50 of its bound, every maximum error equals the model's), no fp32 tensor (worst: mean 0.58 at r_fwd_lean_f32_H72_M5, where five
rows set the yardstick; rstd 0.37, y 0.37, dv 0.29, dv2 0.30, sum / sum32 0.24, y32 0.31, ys 0.42), no column sum (worst 2.58 u of 16: dbias of
r_bwd_gen_bf16_H72_M4), no mask element (0 differ everywhere), and act_bwd_f32 at 0.68 at most (act 4: the fp32 constant 0.01f against 0.01).

Hand mutations of a scratch copy of csrc/a4r_rows.hip (never committed), each run through this file: one-pass variance in row_stats -- 35 cases fail
(c_fwd_*_offset_*, c_sum_*_offset_*, w_fwd_lean_f32_H8, w_sum_*_H8, ...); dres added before dbias is taken in ln_bwd_kernel -- 28 fail (every w_bwd_gen_* and
f_bwd_*_sums_{v,gv,bv,gbv} with dres); the dropout index built with the leading dimension -- 26 fail (every w_fwd_gen_*, f_fwd_*_drop*, f_bwd_*_drop*);
sv assigned instead of accumulated (a wave's earlier rows lost from dbias) -- exactly the four r_bwd_gen_*_M4101 cases fail, nothing at fewer rows.

    case                                             M kernel           | per output: worst error / bound (figures)
    w_fwd_lean_bf16_H8                              37 fwd_lean         | y 0.50 (7.2e-03 / 7.2e-03) mean 0.00 (0.0e+00) rstd 0.19 (9.9e-08)
    w_fwd_gen_bf16_H8                               37 fwd_general      | y 0.50 (7.7e-03 / 7.7e-03) mean 0.29 (1.3e-07) rstd 0.15 (7.3e-08) keep 0 differ
    w_bwd_lean_bf16_H8                              37 bwd_lean         | dv 0.50 (8.4e-03 / 8.4e-03)
    w_bwd_gen_bf16_H8                               37 bwd_general<1,1> | dv 0.50 (6.6e-03 / 6.6e-03) dgamma 0.04 (0.67 u) dbeta 0.00 (0.00 u) dbias 0.04 (0.60 u)
    w_sum_bf16_H8                                   37 sum              | y 0.50 (7.8e-03 / 7.8e-03) sum 0.50 (1.3e-02 / 1.3e-02) sum32 0.21 (2.4e-07) y32 0.31 (3.4e-07) mean 0.37 (2.8e-07) rstd 0.25 (1.0e-07)
    w_fp8_bf16_H8                                   37 fwd_general      | y 0.50 (7.8e-03 / 7.8e-03) mean 0.00 (0.0e+00) rstd 0.24 (1.4e-07) ys 0.26 (7.5e-10) y8 0.89 (8.8e-02)   NEAR ['y8']
    w_fwd_lean_bf16_H64                             37 fwd_lean         | y 0.50 (1.3e-02 / 1.3e-02) mean 0.00 (0.0e+00) rstd 0.15 (5.9e-08)
    w_fwd_gen_bf16_H64                              37 fwd_general      | y 0.50 (1.0e-02 / 1.0e-02) mean 0.35 (1.5e-07) rstd 0.24 (5.7e-08) keep 0 differ
    w_bwd_lean_bf16_H64                             37 bwd_lean         | dv 0.50 (7.6e-03 / 7.6e-03)
    w_bwd_gen_bf16_H64                              37 bwd_general<1,1> | dv 0.50 (1.6e-02 / 1.6e-02) dgamma 0.08 (1.21 u) dbeta 0.00 (0.00 u) dbias 0.07 (1.05 u)
    w_sum_bf16_H64                                  37 sum              | y 0.50 (7.8e-03 / 7.8e-03) sum 0.50 (1.6e-02 / 1.6e-02) sum32 0.00 (0.0e+00) y32 0.19 (3.6e-07) mean 0.07 (3.0e-08) rstd 0.24 (6.8e-08)
    w_fp8_bf16_H64                                  37 fwd_general      | mean 0.00 (0.0e+00) rstd 0.31 (9.8e-08) ys 0.18 (6.8e-10) y8 0.94 (1.2e-01)   NEAR ['y8']
    w_fwd_lean_bf16_H504                            37 fwd_lean         | y 0.50 (1.5e-02 / 1.5e-02) mean 0.06 (5.3e-08) rstd 0.21 (9.9e-08)
    w_fwd_gen_bf16_H504                             37 fwd_general      | y 0.50 (1.5e-02 / 1.5e-02) mean 0.16 (1.4e-07) rstd 0.21 (6.2e-08) keep 0 differ
    w_bwd_lean_bf16_H504                            37 bwd_lean         | dv 0.50 (1.5e-02 / 1.5e-02)
    w_bwd_gen_bf16_H504                             37 bwd_general<1,1> | dv 0.50 (1.3e-02 / 1.3e-02) dgamma 0.08 (1.22 u) dbeta 0.00 (0.00 u) dbias 0.09 (1.37 u)
    w_sum_bf16_H504                                 37 sum              | y 0.50 (1.2e-02 / 1.2e-02) sum 0.50 (1.6e-02 / 1.6e-02) sum32 0.14 (2.4e-07) y32 0.17 (5.8e-07) mean 0.16 (1.4e-07) rstd 0.17 (5.6e-08)
    w_fp8_bf16_H504                                 37 fwd_general      | y 0.50 (1.4e-02 / 1.4e-02) mean 0.19 (1.5e-07) rstd 0.25 (8.3e-08) ys 0.16 (1.2e-09) y8 0.94 (1.8e-01)   NEAR ['y8']
    w_fwd_lean_bf16_H512                            37 fwd_lean         | y 0.50 (1.2e-02 / 1.2e-02) mean 0.21 (1.2e-07) rstd 0.29 (9.5e-08)
    w_fwd_gen_bf16_H512                             37 fwd_general      | y 0.50 (1.5e-02 / 1.5e-02) mean 0.18 (7.3e-08) rstd 0.18 (4.9e-08) keep 0 differ
    w_bwd_lean_bf16_H512                            37 bwd_lean         | dv 0.50 (7.8e-03 / 7.8e-03)
    w_bwd_gen_bf16_H512                             37 bwd_general<1,1> | dv 0.50 (1.5e-02 / 1.5e-02) dgamma 0.10 (1.54 u) dbeta 0.00 (0.00 u) dbias 0.06 (0.93 u)
    w_sum_bf16_H512                                 37 sum              | y 0.50 (1.6e-02 / 1.6e-02) sum 0.50 (1.6e-02 / 1.6e-02) sum32 0.00 (0.0e+00) y32 0.24 (5.5e-07) mean 0.22 (9.7e-08) rstd 0.13 (4.7e-08)
    w_fp8_bf16_H512                                 37 fwd_general      | mean 0.11 (6.0e-08) rstd 0.20 (8.1e-08) ys 0.18 (1.1e-09) y8 0.94 (1.6e-01)   NEAR ['y8']
    w_fwd_lean_bf16_H520                            37 fwd_lean         | y 0.50 (1.5e-02 / 1.5e-02) mean 0.24 (9.9e-08) rstd 0.21 (9.0e-08)
    w_fwd_gen_bf16_H520                             37 fwd_general      | y 0.50 (1.6e-02 / 1.6e-02) mean 0.23 (1.3e-07) rstd 0.25 (7.6e-08) keep 0 differ
    w_bwd_lean_bf16_H520                            37 bwd_lean         | dv 0.50 (1.6e-02 / 1.6e-02)
    w_bwd_gen_bf16_H520                             37 bwd_general<1,1> | dv 0.50 (1.3e-02 / 1.3e-02) dgamma 0.08 (1.31 u) dbeta 0.02 (0.28 u) dbias 0.08 (1.25 u)
    w_sum_bf16_H520                                 37 sum              | y 0.50 (1.4e-02 / 1.4e-02) sum 0.50 (1.6e-02 / 1.6e-02) sum32 0.24 (4.8e-07) y32 0.24 (5.2e-07) mean 0.22 (1.4e-07) rstd 0.21 (4.9e-08)
    w_fp8_bf16_H520                                 37 fwd_general      | y 0.50 (1.5e-02 / 1.5e-02) mean 0.18 (1.1e-07) rstd 0.27 (9.5e-08) ys 0.18 (1.4e-09) y8 0.94 (1.6e-01)   NEAR ['y8']
    w_fwd_lean_bf16_H768                            37 fwd_lean         | y 0.50 (1.5e-02 / 1.5e-02) mean 0.16 (1.2e-07) rstd 0.16 (5.9e-08)
    w_fwd_gen_bf16_H768                             37 fwd_general      | y 0.50 (1.6e-02 / 1.6e-02) mean 0.12 (9.2e-08) rstd 0.24 (6.5e-08) keep 0 differ
    w_bwd_lean_bf16_H768                            37 bwd_lean         | dv 0.50 (8.7e-03 / 8.7e-03)
    w_bwd_gen_bf16_H768                             37 bwd_general<1,1> | dv 0.50 (1.6e-02 / 1.6e-02) dgamma 0.10 (1.62 u) dbeta 0.01 (0.15 u) dbias 0.08 (1.28 u)
    w_sum_bf16_H768                                 37 sum              | y 0.50 (1.5e-02 / 1.5e-02) sum 0.50 (1.6e-02 / 1.6e-02) sum32 0.02 (3.0e-08) y32 0.14 (4.7e-07) mean 0.13 (1.3e-07) rstd 0.17 (4.9e-08)
    w_fp8_bf16_H768                                 37 fwd_general      | mean 0.18 (1.2e-07) rstd 0.24 (1.0e-07) ys 0.19 (1.8e-09) y8 0.94 (1.7e-01)   NEAR ['y8']
    w_fwd_lean_bf16_H1016                           37 fwd_lean         | y 0.50 (1.5e-02 / 1.5e-02) mean 0.16 (5.9e-08) rstd 0.27 (9.4e-08)
    w_fwd_gen_bf16_H1016                            37 fwd_general      | y 0.50 (1.5e-02 / 1.5e-02) mean 0.19 (1.6e-07) rstd 0.18 (5.2e-08) keep 0 differ
    w_bwd_lean_bf16_H1016                           37 bwd_lean         | dv 0.50 (1.6e-02 / 1.6e-02)
    w_bwd_gen_bf16_H1016                            37 bwd_general<1,1> | dv 0.50 (7.8e-03 / 7.8e-03) dgamma 0.09 (1.45 u) dbeta 0.03 (0.45 u) dbias 0.09 (1.43 u)
    w_sum_bf16_H1016                                37 sum              | y 0.50 (1.5e-02 / 1.5e-02) sum 0.50 (1.6e-02 / 1.6e-02) sum32 0.14 (2.4e-07) y32 0.18 (6.3e-07) mean 0.16 (1.7e-07) rstd 0.26 (6.6e-08)
    w_fp8_bf16_H1016                                37 fwd_general      | y 0.50 (1.4e-02 / 1.4e-02) mean 0.25 (1.3e-07) rstd 0.25 (9.6e-08) ys 0.17 (1.1e-09) y8 0.94 (1.6e-01)   NEAR ['y8']
    w_fwd_lean_bf16_H1024                           37 fwd_lean         | y 0.50 (1.6e-02 / 1.6e-02) mean 0.16 (9.2e-08) rstd 0.26 (9.3e-08)
    w_fwd_gen_bf16_H1024                            37 fwd_general      | y 0.50 (1.6e-02 / 1.6e-02) mean 0.17 (1.1e-07) rstd 0.18 (4.9e-08) keep 0 differ
    w_bwd_lean_bf16_H1024                           37 bwd_lean         | dv 0.50 (1.4e-02 / 1.4e-02)
    w_bwd_gen_bf16_H1024                            37 bwd_general<1,1> | dv 0.50 (1.5e-02 / 1.5e-02) dgamma 0.09 (1.45 u) dbeta 0.01 (0.11 u) dbias 0.12 (1.84 u)
    w_sum_bf16_H1024                                37 sum              | y 0.50 (1.5e-02 / 1.5e-02) sum 0.50 (1.6e-02 / 1.6e-02) sum32 0.00 (0.0e+00) y32 0.18 (4.8e-07) mean 0.14 (7.5e-08) rstd 0.19 (4.8e-08)
    w_fp8_bf16_H1024                                37 fwd_general      | mean 0.13 (8.9e-08) rstd 0.17 (8.3e-08) ys 0.22 (1.6e-09) y8 0.94 (2.0e-01)   NEAR ['y8']
    w_quant_bf16_H8                                 37 quant            | ys 0.41 (2.0e-10) y8 0.93 (1.1e-01)   NEAR ['y8']
    w_quant_bf16_H512                               37 quant            | ys 0.42 (4.0e-10) y8 0.94 (2.1e-01)   NEAR ['y8']
    w_quant_bf16_H520                               37 quant            | ys 0.41 (4.0e-10) y8 0.94 (2.1e-01)   NEAR ['y8']
    w_quant_bf16_H4088                              37 quant            | ys 0.41 (4.0e-10) y8 0.94 (1.9e-01)   NEAR ['y8']
    w_quant_bf16_H4096                              37 quant            | ys 0.42 (4.0e-10) y8 0.94 (2.1e-01)   NEAR ['y8']
    w_fwd_lean_f32_H8                               37 fwd_lean         | y 0.34 (2.7e-07) mean 0.09 (6.7e-08) rstd 0.27 (1.7e-07)
    w_fwd_gen_f32_H8                                37 fwd_general      | y 0.18 (3.1e-07) mean 0.38 (2.0e-07) rstd 0.11 (6.4e-08) keep 0 differ
    w_bwd_lean_f32_H8                               37 bwd_lean         | dv 0.25 (3.6e-07)
    w_bwd_gen_f32_H8                                37 bwd_general<1,1> | dv 0.25 (2.2e-07) dgamma 0.04 (0.57 u) dbeta 0.07 (1.13 u) dbias 0.07 (1.09 u)
    w_sum_f32_H8                                    37 sum              | y 0.21 (3.4e-07) sum 0.18 (2.4e-07) sum32 0.18 (2.4e-07) y32 0.21 (3.4e-07) mean 0.23 (2.0e-07) rstd 0.27 (1.4e-07)
    w_fp8_f32_H8                                    37 fwd_general      | y 0.14 (2.5e-07) mean 0.22 (1.4e-07) rstd 0.22 (1.4e-07) ys 0.13 (6.3e-10) y8 0.92 (7.8e-02)   NEAR ['y8']
    w_fwd_lean_f32_H64                              37 fwd_lean         | y 0.22 (4.2e-07) mean 0.25 (1.4e-07) rstd 0.23 (9.2e-08)
    w_fwd_gen_f32_H64                               37 fwd_general      | y 0.16 (4.4e-07) mean 0.17 (9.2e-08) rstd 0.13 (3.8e-08) keep 0 differ
    w_bwd_lean_f32_H64                              37 bwd_lean         | dv 0.20 (2.9e-07)
    w_bwd_gen_f32_H64                               37 bwd_general<1,1> | dv 0.23 (3.5e-07) dgamma 0.06 (0.91 u) dbeta 0.04 (0.59 u) dbias 0.12 (1.97 u)
    w_sum_f32_H64                                   37 sum              | y 0.15 (3.7e-07) sum 0.15 (2.4e-07) sum32 0.15 (2.4e-07) y32 0.15 (3.7e-07) mean 0.30 (2.4e-07) rstd 0.33 (8.0e-08)
    w_fp8_f32_H64                                   37 fwd_general      | mean 0.25 (1.4e-07) rstd 0.34 (1.2e-07) ys 0.17 (1.0e-09) y8 0.94 (1.3e-01)   NEAR ['y8']
    w_fwd_lean_f32_H504                             37 fwd_lean         | y 0.21 (6.2e-07) mean 0.16 (1.3e-07) rstd 0.15 (7.6e-08)
    w_fwd_gen_f32_H504                              37 fwd_general      | y 0.21 (7.2e-07) mean 0.09 (1.0e-07) rstd 0.17 (7.0e-08) keep 0 differ
    w_bwd_lean_f32_H504                             37 bwd_lean         | dv 0.20 (3.9e-07)
    w_bwd_gen_f32_H504                              37 bwd_general<1,1> | dv 0.25 (3.9e-07) dgamma 0.12 (1.86 u) dbeta 0.08 (1.21 u) dbias 0.08 (1.21 u)
    w_sum_f32_H504                                  37 sum              | y 0.21 (5.9e-07) sum 0.15 (2.4e-07) sum32 0.15 (2.4e-07) y32 0.21 (5.9e-07) mean 0.09 (1.2e-07) rstd 0.22 (7.9e-08)
    w_fp8_f32_H504                                  37 fwd_general      | y 0.20 (5.8e-07) mean 0.09 (9.1e-08) rstd 0.14 (7.8e-08) ys 0.17 (1.3e-09) y8 0.94 (1.5e-01)   NEAR ['y8']
    w_fwd_lean_f32_H512                             37 fwd_lean         | y 0.18 (4.7e-07) mean 0.16 (7.8e-08) rstd 0.19 (7.9e-08)
    w_fwd_gen_f32_H512                              37 fwd_general      | y 0.23 (7.2e-07) mean 0.22 (1.5e-07) rstd 0.25 (5.6e-08) keep 0 differ
    w_bwd_lean_f32_H512                             37 bwd_lean         | dv 0.23 (3.9e-07)
    w_bwd_gen_f32_H512                              37 bwd_general<1,1> | dv 0.25 (3.6e-07) dgamma 0.08 (1.31 u) dbeta 0.07 (1.19 u) dbias 0.07 (1.15 u)
    w_sum_f32_H512                                  37 sum              | y 0.17 (5.0e-07) sum 0.14 (2.4e-07) sum32 0.14 (2.4e-07) y32 0.17 (5.0e-07) mean 0.22 (1.4e-07) rstd 0.17 (5.5e-08)
    w_fp8_f32_H512                                  37 fwd_general      | mean 0.16 (8.6e-08) rstd 0.22 (9.7e-08) ys 0.18 (1.3e-09) y8 0.94 (1.6e-01)   NEAR ['y8']
    w_fwd_lean_f32_H520                             37 fwd_lean         | y 0.24 (6.4e-07) mean 0.27 (1.5e-07) rstd 0.22 (1.0e-07)
    w_fwd_gen_f32_H520                              37 fwd_general      | y 0.21 (7.0e-07) mean 0.26 (1.5e-07) rstd 0.24 (5.3e-08) keep 0 differ
    w_bwd_lean_f32_H520                             37 bwd_lean         | dv 0.24 (5.6e-07)
    w_bwd_gen_f32_H520                              37 bwd_general<1,1> | dv 0.25 (4.0e-07) dgamma 0.09 (1.37 u) dbeta 0.05 (0.84 u) dbias 0.12 (1.91 u)
    w_sum_f32_H520                                  37 sum              | y 0.19 (4.9e-07) sum 0.16 (2.4e-07) sum32 0.16 (2.4e-07) y32 0.19 (4.9e-07) mean 0.11 (1.0e-07) rstd 0.22 (6.3e-08)
    w_fp8_f32_H520                                  37 fwd_general      | y 0.27 (6.2e-07) mean 0.22 (1.2e-07) rstd 0.15 (8.6e-08) ys 0.16 (9.8e-10) y8 0.94 (1.7e-01)   NEAR ['y8']
    w_fwd_lean_f32_H768                             37 fwd_lean         | y 0.19 (5.0e-07) mean 0.23 (1.5e-07) rstd 0.17 (7.5e-08)
    w_fwd_gen_f32_H768                              37 fwd_general      | y 0.21 (7.3e-07) mean 0.15 (1.6e-07) rstd 0.17 (5.0e-08) keep 0 differ
    w_bwd_lean_f32_H768                             37 bwd_lean         | dv 0.22 (3.5e-07)
    w_bwd_gen_f32_H768                              37 bwd_general<1,1> | dv 0.25 (5.2e-07) dgamma 0.09 (1.49 u) dbeta 0.06 (0.95 u) dbias 0.07 (1.16 u)
    w_sum_f32_H768                                  37 sum              | y 0.22 (6.9e-07) sum 0.14 (2.4e-07) sum32 0.14 (2.4e-07) y32 0.22 (6.9e-07) mean 0.27 (1.3e-07) rstd 0.14 (4.9e-08)
    w_fp8_f32_H768                                  37 fwd_general      | mean 0.16 (1.2e-07) rstd 0.22 (1.0e-07) ys 0.16 (1.2e-09) y8 0.94 (1.7e-01)   NEAR ['y8']
    w_fwd_lean_f32_H1016                            37 fwd_lean         | y 0.23 (6.8e-07) mean 0.21 (1.9e-07) rstd 0.19 (8.0e-08)
    w_fwd_gen_f32_H1016                             37 fwd_general      | y 0.27 (9.1e-07) mean 0.18 (1.3e-07) rstd 0.25 (7.2e-08) keep 0 differ
    w_bwd_lean_f32_H1016                            37 bwd_lean         | dv 0.19 (4.1e-07)
    w_bwd_gen_f32_H1016                             37 bwd_general<1,1> | dv 0.25 (4.4e-07) dgamma 0.09 (1.39 u) dbeta 0.09 (1.38 u) dbias 0.11 (1.80 u)
    w_sum_f32_H1016                                 37 sum              | y 0.23 (8.2e-07) sum 0.15 (2.4e-07) sum32 0.15 (2.4e-07) y32 0.23 (8.2e-07) mean 0.31 (2.0e-07) rstd 0.20 (5.9e-08)
    w_fp8_f32_H1016                                 37 fwd_general      | y 0.21 (5.6e-07) mean 0.20 (1.4e-07) rstd 0.19 (7.7e-08) ys 0.21 (1.5e-09) y8 0.94 (1.7e-01)   NEAR ['y8']
    w_fwd_lean_f32_H1024                            37 fwd_lean         | y 0.21 (5.1e-07) mean 0.19 (1.3e-07) rstd 0.17 (6.4e-08)
    w_fwd_gen_f32_H1024                             37 fwd_general      | y 0.23 (7.5e-07) mean 0.25 (2.1e-07) rstd 0.34 (7.7e-08) keep 0 differ
    w_bwd_lean_f32_H1024                            37 bwd_lean         | dv 0.25 (6.0e-07)
    w_bwd_gen_f32_H1024                             37 bwd_general<1,1> | dv 0.25 (5.1e-07) dgamma 0.10 (1.61 u) dbeta 0.06 (0.96 u) dbias 0.07 (1.04 u)
    w_sum_f32_H1024                                 37 sum              | y 0.21 (6.8e-07) sum 0.23 (4.8e-07) sum32 0.23 (4.8e-07) y32 0.21 (6.8e-07) mean 0.19 (1.1e-07) rstd 0.25 (6.6e-08)
    w_fp8_f32_H1024                                 37 fwd_general      | mean 0.17 (9.8e-08) rstd 0.19 (7.9e-08) ys 0.18 (1.1e-09) y8 0.94 (1.7e-01)   NEAR ['y8']
    w_quant_f32_H8                                  37 quant            | ys 0.41 (2.7e-10) y8 0.90 (1.2e-01)   NEAR ['y8']
    w_quant_f32_H512                                37 quant            | ys 0.41 (4.0e-10) y8 0.94 (2.1e-01)   NEAR ['y8']
    w_quant_f32_H520                                37 quant            | ys 0.42 (4.0e-10) y8 0.94 (2.1e-01)   NEAR ['y8']
    w_quant_f32_H4088                               37 quant            | ys 0.42 (4.0e-10) y8 0.94 (2.2e-01)   NEAR ['y8']
    w_quant_f32_H4096                               37 quant            | ys 0.41 (4.0e-10) y8 0.94 (2.3e-01)   NEAR ['y8']
    f_bwd_bf16_sums_none                            37 bwd_general<0,0> | dv 0.50 (7.7e-03 / 7.7e-03)
    f_bwd_bf16_sums_g                               37 bwd_general<1,0> | dv 0.50 (1.3e-02 / 1.3e-02) dgamma 0.08 (1.22 u)
    f_bwd_bf16_sums_b                               37 bwd_general<1,0> | dv 0.50 (1.2e-02 / 1.2e-02) dbeta 0.00 (0.00 u)
    f_bwd_bf16_sums_gb                              37 bwd_general<1,0> | dv 0.50 (7.7e-03 / 7.7e-03) dgamma 0.07 (1.12 u) dbeta 0.00 (0.00 u)
    f_bwd_bf16_sums_v                               37 bwd_general<0,1> | dv 0.50 (1.5e-02 / 1.5e-02) dbias 0.06 (0.99 u)
    f_bwd_bf16_sums_gv                              37 bwd_general<1,1> | dv 0.50 (7.6e-03 / 7.6e-03) dgamma 0.06 (0.97 u) dbias 0.05 (0.87 u)
    f_bwd_bf16_sums_bv                              37 bwd_general<1,1> | dv 0.50 (6.7e-03 / 6.7e-03) dbeta 0.00 (0.00 u) dbias 0.04 (0.59 u)
    f_bwd_bf16_sums_gbv                             37 bwd_general<1,1> | dv 0.50 (1.0e-02 / 1.0e-02) dgamma 0.06 (0.93 u) dbeta 0.00 (0.00 u) dbias 0.05 (0.76 u)
    f_fwd_bf16_add1                                 37 fwd_general      | y 0.50 (7.7e-03 / 7.7e-03) mean 0.13 (9.8e-08) rstd 0.28 (7.8e-08)
    f_bwd_bf16_add1                                 37 bwd_general<1,1> | dv 0.50 (7.5e-03 / 7.5e-03) dgamma 0.05 (0.82 u) dbeta 0.00 (0.00 u) dbias 0.06 (0.93 u)
    f_fwd_bf16_add20                                37 fwd_general      | y 0.50 (1.4e-02 / 1.4e-02) mean 0.25 (2.1e-07) rstd 0.19 (6.8e-08)
    f_bwd_bf16_add20                                37 bwd_general<1,1> | dv 0.50 (7.7e-03 / 7.7e-03) dgamma 0.06 (0.94 u) dbeta 0.00 (0.00 u) dbias 0.06 (1.01 u)
    f_fwd_bf16_add37                                37 fwd_general      | y 0.50 (1.1e-02 / 1.1e-02) mean 0.17 (1.4e-07) rstd 0.17 (6.3e-08)
    f_bwd_bf16_add37                                37 bwd_general<1,1> | dv 0.50 (7.7e-03 / 7.7e-03) dgamma 0.06 (0.91 u) dbeta 0.00 (0.00 u) dbias 0.07 (1.12 u)
    f_fwd_bf16_add40                                37 fwd_general      | y 0.50 (1.3e-02 / 1.3e-02) mean 0.19 (1.2e-07) rstd 0.22 (5.2e-08)
    f_bwd_bf16_add40                                37 bwd_general<1,1> | dv 0.50 (7.4e-03 / 7.4e-03) dgamma 0.06 (0.94 u) dbeta 0.00 (0.00 u) dbias 0.04 (0.64 u)
    f_fwd_bf16_drop0.1                              37 fwd_general      | y 0.50 (1.5e-02 / 1.5e-02) mean 0.23 (1.0e-07) rstd 0.16 (7.2e-08) keep 0 differ
    f_bwd_bf16_drop0.1                              37 bwd_general<1,1> | dv 0.50 (1.4e-02 / 1.4e-02) dgamma 0.07 (1.16 u) dbeta 0.08 (1.25 u) dbias 0.07 (1.16 u)
    f_fwd_bf16_drop0.5                              37 fwd_general      | y 0.50 (2.8e-02 / 2.8e-02) mean 0.17 (1.2e-07) rstd 0.23 (9.0e-08) keep 0 differ
    f_bwd_bf16_drop0.5                              37 bwd_general<1,1> | dv 0.50 (2.6e-02 / 2.6e-02) dgamma 0.09 (1.52 u) dbeta 0.02 (0.37 u) dbias 0.09 (1.45 u)
    f_bwd_bf16_dv2                                  37 bwd_general<0,0> | dv 0.50 (1.5e-02 / 1.5e-02) dv2 0.50 (1.4e-02 / 1.4e-02) keep2 0 differ
    f_bwd_bf16_dv2_p0                               37 bwd_general<0,1> | dv 0.50 (7.8e-03 / 7.8e-03) dv2 0.50 (7.8e-03 / 7.8e-03) dbias 0.05 (0.85 u)
    f_bwd_bf16_dv2_both                             37 bwd_general<1,0> | dv 0.50 (1.5e-02 / 1.5e-02) dv2 0.50 (1.6e-02 / 1.6e-02) dgamma 0.11 (1.79 u) dbeta 0.07 (1.06 u) keep2 0 differ
    f_sum_bf16_none                                 37 sum              | y 0.50 (1.1e-02 / 1.1e-02) mean 0.29 (1.6e-07) rstd 0.13 (6.0e-08)
    f_sum_bf16_sum                                  37 sum              | y 0.50 (9.3e-03 / 9.3e-03) sum 0.50 (1.6e-02 / 1.6e-02) mean 0.17 (1.1e-07) rstd 0.23 (6.6e-08)
    f_sum_bf16_sum32                                37 sum              | y 0.50 (1.6e-02 / 1.6e-02) sum32 0.14 (2.4e-07) mean 0.27 (1.5e-07) rstd 0.17 (6.1e-08)
    f_sum_bf16_y32                                  37 sum              | y 0.50 (7.8e-03 / 7.8e-03) y32 0.25 (4.5e-07) mean 0.09 (5.3e-08) rstd 0.22 (5.8e-08)
    f_sum_bf16_sum_sum32_y32                        37 sum              | y 0.50 (7.8e-03 / 7.8e-03) sum 0.50 (1.3e-02 / 1.3e-02) sum32 0.17 (2.4e-07) y32 0.25 (4.8e-07) mean 0.26 (1.4e-07) rstd 0.20 (5.6e-08)
    f_sum_bf16_res_all                              37 sum              | y 0.50 (7.8e-03 / 7.8e-03) sum 0.50 (1.6e-02 / 1.6e-02) sum32 0.00 (0.0e+00) y32 0.20 (4.0e-07) mean 0.14 (1.1e-07) rstd 0.29 (8.0e-08)
    f_sum_bf16_res32_all                            37 sum              | y 0.50 (7.7e-03 / 7.7e-03) sum 0.50 (1.6e-02 / 1.6e-02) sum32 0.15 (2.4e-07) y32 0.23 (6.2e-07) mean 0.25 (2.4e-07) rstd 0.20 (6.1e-08)
    f_fp8_bf16_y0                                   37 fwd_general      | mean 0.19 (1.1e-07) rstd 0.33 (1.1e-07) ys 0.17 (7.7e-10) y8 0.94 (1.3e-01)   NEAR ['y8']
    f_fp8_bf16_y1                                   37 fwd_general      | y 0.50 (1.3e-02 / 1.3e-02) mean 0.35 (2.2e-07) rstd 0.25 (6.7e-08) ys 0.22 (1.1e-09) y8 0.94 (1.4e-01)   NEAR ['y8']
    f_bwd_f32_sums_none                             37 bwd_general<0,0> | dv 0.25 (2.7e-07)
    f_bwd_f32_sums_g                                37 bwd_general<1,0> | dv 0.23 (2.5e-07) dgamma 0.05 (0.86 u)
    f_bwd_f32_sums_b                                37 bwd_general<1,0> | dv 0.22 (2.4e-07) dbeta 0.03 (0.55 u)
    f_bwd_f32_sums_gb                               37 bwd_general<1,0> | dv 0.25 (2.1e-07) dgamma 0.07 (1.11 u) dbeta 0.06 (0.98 u)
    f_bwd_f32_sums_v                                37 bwd_general<0,1> | dv 0.25 (3.1e-07) dbias 0.06 (0.88 u)
    f_bwd_f32_sums_gv                               37 bwd_general<1,1> | dv 0.25 (2.4e-07) dgamma 0.06 (0.91 u) dbias 0.05 (0.76 u)
    f_bwd_f32_sums_bv                               37 bwd_general<1,1> | dv 0.25 (2.5e-07) dbeta 0.05 (0.85 u) dbias 0.06 (0.88 u)
    f_bwd_f32_sums_gbv                              37 bwd_general<1,1> | dv 0.26 (3.0e-07) dgamma 0.06 (0.88 u) dbeta 0.05 (0.79 u) dbias 0.05 (0.78 u)
    f_fwd_f32_add1                                  37 fwd_general      | y 0.23 (4.0e-07) mean 0.16 (1.1e-07) rstd 0.20 (5.2e-08)
    f_bwd_f32_add1                                  37 bwd_general<1,1> | dv 0.25 (2.6e-07) dgamma 0.09 (1.51 u) dbeta 0.05 (0.87 u) dbias 0.08 (1.24 u)
    f_fwd_f32_add20                                 37 fwd_general      | y 0.29 (4.9e-07) mean 0.30 (1.9e-07) rstd 0.26 (6.6e-08)
    f_bwd_f32_add20                                 37 bwd_general<1,1> | dv 0.25 (2.9e-07) dgamma 0.12 (1.85 u) dbeta 0.04 (0.71 u) dbias 0.04 (0.67 u)
    f_fwd_f32_add37                                 37 fwd_general      | y 0.17 (4.4e-07) mean 0.37 (1.8e-07) rstd 0.32 (1.0e-07)
    f_bwd_f32_add37                                 37 bwd_general<1,1> | dv 0.21 (2.2e-07) dgamma 0.07 (1.09 u) dbeta 0.05 (0.81 u) dbias 0.05 (0.86 u)
    f_fwd_f32_add40                                 37 fwd_general      | y 0.37 (7.2e-07) mean 0.24 (1.3e-07) rstd 0.20 (6.4e-08)
    f_bwd_f32_add40                                 37 bwd_general<1,1> | dv 0.25 (2.5e-07) dgamma 0.06 (0.96 u) dbeta 0.06 (0.96 u) dbias 0.06 (0.92 u)
    f_fwd_f32_drop0.1                               37 fwd_general      | y 0.20 (5.9e-07) mean 0.25 (1.3e-07) rstd 0.32 (1.0e-07) keep 0 differ
    f_bwd_f32_drop0.1                               37 bwd_general<1,1> | dv 0.25 (6.5e-07) dgamma 0.10 (1.53 u) dbeta 0.07 (1.05 u) dbias 0.10 (1.61 u)
    f_fwd_f32_drop0.5                               37 fwd_general      | y 0.17 (9.5e-07) mean 0.35 (1.9e-07) rstd 0.25 (8.9e-08) keep 0 differ
    f_bwd_f32_drop0.5                               37 bwd_general<1,1> | dv 0.25 (9.0e-07) dgamma 0.13 (2.03 u) dbeta 0.09 (1.37 u) dbias 0.09 (1.51 u)
    f_bwd_f32_dv2                                   37 bwd_general<0,0> | dv 0.29 (4.5e-07) dv2 0.30 (5.5e-07) keep2 0 differ
    f_bwd_f32_dv2_p0                                37 bwd_general<0,1> | dv 0.25 (3.5e-07) dv2 0.25 (3.5e-07) dbias 0.09 (1.40 u)
    f_bwd_f32_dv2_both                              37 bwd_general<1,0> | dv 0.25 (7.1e-07) dv2 0.25 (7.6e-07) dgamma 0.09 (1.49 u) dbeta 0.06 (1.03 u) keep2 0 differ
    f_sum_f32_none                                  37 sum              | y 0.18 (3.9e-07) mean 0.18 (1.1e-07) rstd 0.23 (6.8e-08)
    f_sum_f32_sum                                   37 sum              | y 0.34 (7.0e-07) sum 0.15 (2.4e-07) mean 0.25 (1.8e-07) rstd 0.37 (9.5e-08)
    f_sum_f32_sum32                                 37 sum              | y 0.12 (4.1e-07) sum32 0.16 (2.4e-07) mean 0.24 (1.4e-07) rstd 0.21 (6.2e-08)
    f_sum_f32_y32                                   37 sum              | y 0.29 (4.5e-07) y32 0.29 (4.5e-07) mean 0.32 (2.5e-07) rstd 0.24 (7.3e-08)
    f_sum_f32_sum_sum32_y32                         37 sum              | y 0.20 (4.1e-07) sum 0.16 (2.4e-07) sum32 0.16 (2.4e-07) y32 0.20 (4.1e-07) mean 0.25 (1.8e-07) rstd 0.15 (5.4e-08)
    f_sum_f32_res_all                               37 sum              | y 0.16 (4.2e-07) sum 0.15 (2.4e-07) sum32 0.15 (2.4e-07) y32 0.16 (4.2e-07) mean 0.23 (1.4e-07) rstd 0.23 (5.6e-08)
    f_sum_f32_res32_all                             37 sum              | y 0.28 (4.9e-07) sum 0.19 (2.4e-07) sum32 0.19 (2.4e-07) y32 0.28 (4.9e-07) mean 0.28 (1.7e-07) rstd 0.25 (6.3e-08)
    f_fp8_f32_y0                                    37 fwd_general      | mean 0.26 (1.7e-07) rstd 0.21 (9.9e-08) ys 0.16 (9.0e-10) y8 0.94 (1.2e-01)   NEAR ['y8']
    f_fp8_f32_y1                                    37 fwd_general      | y 0.31 (7.1e-07) mean 0.24 (1.6e-07) rstd 0.29 (6.3e-08) ys 0.25 (1.6e-09) y8 0.94 (1.3e-01)   NEAR ['y8']
    c_fwd_bf16_offset_1e-06                         37 fwd_lean         | y 0.50 (1.5e-02 / 1.5e-02) mean 0.12 (2.5e-06) rstd 0.19 (9.1e-08)
    c_fwd_gen_bf16_offset_1e-06                     37 fwd_general      | y 0.50 (1.5e-02 / 1.5e-02) mean 0.37 (8.0e-06) rstd 0.23 (1.1e-07)
    c_sum_bf16_offset_1e-06                         37 sum              | y 0.50 (1.5e-02 / 1.5e-02) sum 0.50 (2.5e-01 / 2.5e-01) sum32 0.22 (3.8e-06) y32 0.22 (9.7e-06) mean 0.22 (6.3e-06) rstd 0.31 (8.5e-08)
    c_bwd_bf16_offset_1e-06                         37 bwd_general<1,1> | dv 0.50 (1.5e-02 / 1.5e-02) dgamma 0.10 (1.58 u) dbeta 0.01 (0.17 u) dbias 0.08 (1.23 u)
    c_fwd_bf16_const_1e-06                          37 fwd_lean         | y 0.50 (1.5e-02 / 1.5e-02) mean 0.16 (1.0e-07) rstd 0.00 (8.5e-08)
    c_bwd_bf16_const_1e-06                          37 bwd_general<1,0> | dv 0.50 (8.0e+00 / 8.0e+00) dgamma 0.08 (1.23 u) dbeta 0.01 (0.13 u)
    c_fp8_bf16_zero_1e-06                           37 fwd_general      | y 0.50 (1.6e-02 / 1.6e-02) mean 0.12 (7.9e-08) rstd 0.00 (9.8e-08) ys 0.16 (1.3e-09) y8 0.94 (1.5e-01)   NEAR ['y8']
    c_fwd_bf16_offset_1e-12                         37 fwd_lean         | y 0.50 (1.6e-02 / 1.6e-02) mean 0.12 (2.5e-06) rstd 0.25 (9.9e-08)
    c_fwd_gen_bf16_offset_1e-12                     37 fwd_general      | y 0.50 (1.6e-02 / 1.6e-02) mean 0.34 (9.6e-06) rstd 0.25 (8.8e-08)
    c_sum_bf16_offset_1e-12                         37 sum              | y 0.50 (1.5e-02 / 1.5e-02) sum 0.50 (2.5e-01 / 2.5e-01) sum32 0.23 (3.8e-06) y32 0.23 (1.1e-05) mean 0.20 (7.4e-06) rstd 0.24 (1.3e-07)
    c_bwd_bf16_offset_1e-12                         37 bwd_general<1,1> | dv 0.50 (1.5e-02 / 1.5e-02) dgamma 0.08 (1.29 u) dbeta 0.02 (0.31 u) dbias 0.07 (1.17 u)
    c_fwd_bf16_const_1e-12                          37 fwd_lean         | y 0.50 (1.5e-02 / 1.5e-02) mean 0.12 (7.9e-08) rstd 0.00 (8.5e-08)
    c_bwd_bf16_const_1e-12                          37 bwd_general<1,0> | dv 0.50 (8.0e+03 / 8.0e+03) dgamma 0.11 (1.78 u) dbeta 0.01 (0.11 u)
    c_fp8_bf16_zero_1e-12                           37 fwd_general      | y 0.50 (7.8e-03 / 7.8e-03) mean 0.12 (7.9e-08) rstd 0.00 (8.1e-08) ys 0.20 (1.1e-09) y8 0.94 (1.4e-01)   NEAR ['y8']
    c_fwd_f32_offset_1e-06                          37 fwd_lean         | y 0.17 (1.3e-04) mean 0.17 (7.9e-05) rstd 0.15 (8.6e-08)
    c_fwd_gen_f32_offset_1e-06                      37 fwd_general      | y 0.20 (1.3e-04) mean 0.20 (1.0e-04) rstd 0.25 (5.6e-07)
    c_sum_f32_offset_1e-06                          37 sum              | y 0.20 (1.1e-04) sum 0.13 (3.1e-05) sum32 0.13 (3.1e-05) y32 0.20 (1.1e-04) mean 0.18 (7.9e-05) rstd 0.25 (8.3e-07)
    c_bwd_f32_offset_1e-06                          37 bwd_general<1,1> | dv 0.25 (4.5e-07) dgamma 0.09 (1.44 u) dbeta 0.08 (1.23 u) dbias 0.09 (1.46 u)
    c_fwd_f32_const_1e-06                           37 fwd_lean         | y 0.25 (6.6e-07) mean 0.16 (1.0e-07) rstd 0.00 (8.2e-08)
    c_bwd_f32_const_1e-06                           37 bwd_general<1,0> | dv 0.25 (3.0e-04) dgamma 0.08 (1.33 u) dbeta 0.07 (1.14 u)
    c_fp8_f32_zero_1e-06                            37 fwd_general      | y 0.25 (5.4e-07) mean 0.25 (1.5e-07) rstd 0.00 (1.1e-07) ys 0.21 (1.2e-09) y8 0.94 (1.5e-01)   NEAR ['y8']
    c_fwd_f32_offset_1e-12                          37 fwd_lean         | y 0.17 (1.3e-04) mean 0.18 (8.9e-05) rstd 0.25 (1.0e-07)
    c_fwd_gen_f32_offset_1e-12                      37 fwd_general      | y 0.24 (1.2e-04) mean 0.27 (1.0e-04) rstd 0.25 (8.6e-07)
    c_sum_f32_offset_1e-12                          37 sum              | y 0.17 (1.1e-04) sum 0.13 (3.1e-05) sum32 0.13 (3.1e-05) y32 0.17 (1.1e-04) mean 0.15 (7.8e-05) rstd 0.25 (9.5e-07)
    c_bwd_f32_offset_1e-12                          37 bwd_general<1,1> | dv 0.25 (4.0e-07) dgamma 0.08 (1.36 u) dbeta 0.06 (1.00 u) dbias 0.08 (1.22 u)
    c_fwd_f32_const_1e-12                           37 fwd_lean         | y 0.28 (7.7e-07) mean 0.29 (1.8e-07) rstd 0.00 (9.2e-08)
    c_bwd_f32_const_1e-12                           37 bwd_general<1,0> | dv 0.25 (2.8e-01) dgamma 0.09 (1.44 u) dbeta 0.07 (1.11 u)
    c_fp8_f32_zero_1e-12                            37 fwd_general      | y 0.30 (6.6e-07) mean 0.19 (9.0e-08) rstd 0.00 (9.9e-08) ys 0.25 (1.5e-09) y8 0.94 (1.5e-01)   NEAR ['y8']
    r_fwd_lean_bf16_H72_M1                           1 fwd_lean         | y 0.50 (6.0e-03 / 6.0e-03) mean 0.04 (3.3e-09) rstd 0.29 (6.5e-08)
    r_bwd_gen_bf16_H72_M1                            1 bwd_general<1,1> | dv 0.50 (7.8e-03 / 7.8e-03) dgamma 0.09 (1.49 u) dbeta 0.00 (0.00 u) dbias 0.09 (1.38 u)
    r_fwd_lean_bf16_H72_M3                           3 fwd_lean         | y 0.50 (6.5e-03 / 6.5e-03) mean 0.13 (5.3e-08) rstd 0.24 (5.7e-08)
    r_bwd_gen_bf16_H72_M3                            3 bwd_general<1,1> | dv 0.50 (9.2e-03 / 9.2e-03) dgamma 0.11 (1.69 u) dbeta 0.00 (0.00 u) dbias 0.11 (1.78 u)
    r_fwd_lean_bf16_H72_M4                           4 fwd_lean         | y 0.50 (7.8e-03 / 7.8e-03) mean 0.16 (5.3e-08) rstd 0.23 (6.4e-08)
    r_bwd_gen_bf16_H72_M4                            4 bwd_general<1,1> | dv 0.50 (7.6e-03 / 7.6e-03) dgamma 0.07 (1.11 u) dbeta 0.00 (0.00 u) dbias 0.16 (2.58 u)
    r_fwd_lean_bf16_H72_M5                           5 fwd_lean         | y 0.50 (6.4e-03 / 6.4e-03) mean 0.11 (5.3e-08) rstd 0.24 (6.8e-08)
    r_bwd_gen_bf16_H72_M5                            5 bwd_general<1,1> | dv 0.50 (7.7e-03 / 7.7e-03) dgamma 0.10 (1.67 u) dbeta 0.00 (0.00 u) dbias 0.10 (1.65 u)
    r_bwd_gen_bf16_H72_M4101                      4101 bwd_general<1,1> | dv 0.50 (1.6e-02 / 1.6e-02) dgamma 0.05 (0.82 u) dbeta 0.00 (0.08 u) dbias 0.03 (0.50 u)
    r_fwd_lean_bf16_H72_M8195                     8195 fwd_lean         | y 0.50 (1.6e-02 / 1.6e-02) mean 0.21 (2.1e-07) rstd 0.24 (1.7e-07)
    r_fwd_gen_bf16_H72_M8195                      8195 fwd_general      | y 0.50 (1.6e-02 / 1.6e-02) mean 0.24 (3.6e-07) rstd 0.23 (1.1e-07)
    r_fwd_lean_bf16_H72_M24593                   24593 fwd_lean         | y 0.50 (1.6e-02 / 1.6e-02) mean 0.18 (1.9e-07) rstd 0.22 (1.5e-07)
    r_fwd_gen_bf16_H72_M24593                    24593 fwd_general      | y 0.50 (1.6e-02 / 1.6e-02) mean 0.25 (3.8e-07) rstd 0.22 (1.0e-07)
    r_bwd_pg_bf16_H72_2047_plain                  2047 bwd_general<1,0> | dv 0.50 (1.5e-02 / 1.5e-02) dgamma 0.04 (0.70 u) dbeta 0.00 (0.06 u)
    r_bwd_pg_bf16_H72_2047_dres                   2047 bwd_general<1,0> | dv 0.50 (1.6e-02 / 1.6e-02) dgamma 0.05 (0.81 u)
    r_bwd_pg_bf16_H72_2047_dv2p0                  2047 bwd_general<1,0> | dv 0.50 (1.5e-02 / 1.5e-02) dv2 0.50 (1.5e-02 / 1.5e-02) dbeta 0.00 (0.08 u)
    r_bwd_pg_bf16_H72_2047_dres_dv2               2047 bwd_general<1,0> | dv 0.50 (1.6e-02 / 1.6e-02) dv2 0.50 (2.9e-02 / 2.9e-02) dgamma 0.06 (0.96 u) dbeta 0.00 (0.06 u) keep2 0 differ
    r_bwd_pg_bf16_H72_2048_plain                  2048 bwd_pg           | dv 0.50 (1.5e-02 / 1.5e-02) dgamma 0.03 (0.55 u)
    r_bwd_pg_bf16_H72_2048_dres                   2048 bwd_pg           | dv 0.50 (1.6e-02 / 1.6e-02) dbeta 0.00 (0.08 u)
    r_bwd_pg_bf16_H72_2048_dv2p0                  2048 bwd_pg           | dv 0.50 (1.5e-02 / 1.5e-02) dv2 0.50 (1.5e-02 / 1.5e-02) dgamma 0.06 (1.03 u) dbeta 0.01 (0.08 u)
    r_bwd_pg_bf16_H72_2048_dres_dv2               2048 bwd_pg           | dv 0.50 (1.6e-02 / 1.6e-02) dv2 0.50 (1.6e-02 / 1.6e-02) dgamma 0.03 (0.42 u) dbeta 0.01 (0.10 u) keep2 0 differ
    r_bwd_pg_bf16_H72_2049_plain                  2049 bwd_pg           | dv 0.50 (1.6e-02 / 1.6e-02) dbeta 0.00 (0.04 u)
    r_bwd_pg_bf16_H72_2049_dres                   2049 bwd_pg           | dv 0.50 (1.6e-02 / 1.6e-02) dgamma 0.05 (0.80 u) dbeta 0.00 (0.08 u)
    r_bwd_pg_bf16_H72_2049_dv2p0                  2049 bwd_pg           | dv 0.50 (1.5e-02 / 1.5e-02) dv2 0.50 (1.5e-02 / 1.5e-02) dgamma 0.03 (0.50 u) dbeta 0.00 (0.06 u)
    r_bwd_pg_bf16_H72_2049_dres_dv2               2049 bwd_pg           | dv 0.50 (1.6e-02 / 1.6e-02) dv2 0.50 (1.6e-02 / 1.6e-02) dgamma 0.05 (0.74 u) keep2 0 differ
    r_bwd_pg_bf16_H72_8G+1_plain                  2049 bwd_pg           | dv 0.50 (1.6e-02 / 1.6e-02) dgamma 0.07 (1.15 u) dbeta 0.00 (0.06 u)
    r_bwd_pg_bf16_H72_8G+1_dres                   2049 bwd_pg           | dv 0.50 (1.6e-02 / 1.6e-02) dgamma 0.05 (0.75 u) dbeta 0.00 (0.04 u)
    r_bwd_pg_bf16_H72_8G+1_dv2p0                  2049 bwd_pg           | dv 0.50 (1.5e-02 / 1.5e-02) dv2 0.50 (1.5e-02 / 1.5e-02) dgamma 0.03 (0.53 u)
    r_bwd_pg_bf16_H72_8G+1_dres_dv2               2049 bwd_pg           | dv 0.50 (1.6e-02 / 1.6e-02) dv2 0.50 (1.6e-02 / 1.6e-02) dbeta 0.01 (0.12 u) keep2 0 differ
    r_bwd_pg_bf16_H72_16G+5_plain                 4101 bwd_pg           | dv 0.50 (1.5e-02 / 1.5e-02) dgamma 0.02 (0.36 u) dbeta 0.01 (0.10 u)
    r_bwd_pg_bf16_H72_16G+5_dres                  4101 bwd_pg           | dv 0.50 (1.6e-02 / 1.6e-02) dgamma 0.03 (0.47 u)
    r_bwd_pg_bf16_H72_16G+5_dv2p0                 4101 bwd_pg           | dv 0.50 (1.6e-02 / 1.6e-02) dv2 0.50 (1.6e-02 / 1.6e-02) dbeta 0.01 (0.09 u)
    r_bwd_pg_bf16_H72_16G+5_dres_dv2              4101 bwd_pg           | dv 0.50 (1.6e-02 / 1.6e-02) dv2 0.50 (1.6e-02 / 1.6e-02) dgamma 0.02 (0.32 u) dbeta 0.00 (0.06 u) keep2 0 differ
    r_fwd_lean_bf16_H1024_M1                         1 fwd_lean         | y 0.50 (7.8e-03 / 7.8e-03) mean 0.12 (6.0e-08) rstd 0.29 (7.0e-08)
    r_bwd_gen_bf16_H1024_M1                          1 bwd_general<1,1> | dv 0.50 (1.0e-02 / 1.0e-02) dgamma 0.12 (1.93 u) dbeta 0.00 (0.00 u) dbias 0.15 (2.38 u)
    r_fwd_lean_bf16_H1024_M3                         3 fwd_lean         | y 0.50 (1.4e-02 / 1.4e-02) mean 0.13 (6.0e-08) rstd 0.15 (3.6e-08)
    r_bwd_gen_bf16_H1024_M3                          3 bwd_general<1,1> | dv 0.50 (1.4e-02 / 1.4e-02) dgamma 0.12 (1.87 u) dbeta 0.00 (0.00 u) dbias 0.12 (1.98 u)
    r_fwd_lean_bf16_H1024_M4                         4 fwd_lean         | y 0.50 (1.1e-02 / 1.1e-02) mean 0.25 (1.5e-07) rstd 0.15 (5.1e-08)
    r_bwd_gen_bf16_H1024_M4                          4 bwd_general<1,1> | dv 0.50 (1.5e-02 / 1.5e-02) dgamma 0.13 (2.04 u) dbeta 0.00 (0.00 u) dbias 0.14 (2.23 u)
    r_fwd_lean_bf16_H1024_M5                         5 fwd_lean         | y 0.50 (8.7e-03 / 8.7e-03) mean 0.26 (8.9e-08) rstd 0.17 (5.6e-08)
    r_bwd_gen_bf16_H1024_M5                          5 bwd_general<1,1> | dv 0.50 (1.6e-02 / 1.6e-02) dgamma 0.15 (2.38 u) dbeta 0.00 (0.00 u) dbias 0.13 (2.07 u)
    r_bwd_gen_bf16_H1024_M4101                    4101 bwd_general<1,1> | dv 0.50 (1.6e-02 / 1.6e-02) dgamma 0.08 (1.21 u) dbeta 0.01 (0.10 u) dbias 0.06 (0.92 u)
    r_fwd_lean_bf16_H1024_M8195                   8195 fwd_lean         | y 0.50 (1.6e-02 / 1.6e-02) mean 0.20 (1.9e-07) rstd 0.22 (1.2e-07)
    r_fwd_gen_bf16_H1024_M8195                    8195 fwd_general      | y 0.50 (1.6e-02 / 1.6e-02) mean 0.27 (3.0e-07) rstd 0.21 (8.2e-08)
    r_fwd_lean_bf16_H1024_M24593                 24593 fwd_lean         | y 0.50 (1.6e-02 / 1.6e-02) mean 0.20 (2.2e-07) rstd 0.22 (1.3e-07)
    r_fwd_gen_bf16_H1024_M24593                  24593 fwd_general      | y 0.50 (1.6e-02 / 1.6e-02) mean 0.24 (3.2e-07) rstd 0.27 (1.0e-07)
    r_bwd_pg_bf16_H1024_2047_plain                2047 bwd_general<1,0> | dv 0.50 (1.6e-02 / 1.6e-02) dgamma 0.07 (1.08 u) dbeta 0.01 (0.10 u)
    r_bwd_pg_bf16_H1024_2047_dres                 2047 bwd_general<1,0> | dv 0.50 (1.6e-02 / 1.6e-02) dgamma 0.09 (1.40 u)
    r_bwd_pg_bf16_H1024_2047_dv2p0                2047 bwd_general<1,0> | dv 0.50 (1.6e-02 / 1.6e-02) dv2 0.50 (1.6e-02 / 1.6e-02) dbeta 0.00 (0.08 u)
    r_bwd_pg_bf16_H1024_2047_dres_dv2             2047 bwd_general<1,0> | dv 0.50 (1.6e-02 / 1.6e-02) dv2 0.50 (2.2e-02 / 2.2e-02) dgamma 0.07 (1.20 u) dbeta 0.01 (0.20 u) keep2 0 differ
    r_bwd_pg_bf16_H1024_2048_plain                2048 bwd_pg           | dv 0.50 (1.6e-02 / 1.6e-02) dgamma 0.05 (0.87 u)
    r_bwd_pg_bf16_H1024_2048_dres                 2048 bwd_pg           | dv 0.50 (1.6e-02 / 1.6e-02) dbeta 0.01 (0.18 u)
    r_bwd_pg_bf16_H1024_2048_dv2p0                2048 bwd_pg           | dv 0.50 (1.6e-02 / 1.6e-02) dv2 0.50 (1.6e-02 / 1.6e-02) dgamma 0.06 (0.90 u) dbeta 0.01 (0.12 u)
    r_bwd_pg_bf16_H1024_2048_dres_dv2             2048 bwd_pg           | dv 0.50 (1.6e-02 / 1.6e-02) dv2 0.50 (2.9e-02 / 2.9e-02) dgamma 0.05 (0.86 u) dbeta 0.01 (0.16 u) keep2 0 differ
    r_bwd_pg_bf16_H1024_2049_plain                2049 bwd_pg           | dv 0.50 (1.6e-02 / 1.6e-02) dbeta 0.01 (0.12 u)
    r_bwd_pg_bf16_H1024_2049_dres                 2049 bwd_pg           | dv 0.50 (1.6e-02 / 1.6e-02) dgamma 0.06 (0.93 u) dbeta 0.01 (0.10 u)
    r_bwd_pg_bf16_H1024_2049_dv2p0                2049 bwd_pg           | dv 0.50 (1.6e-02 / 1.6e-02) dv2 0.50 (1.6e-02 / 1.6e-02) dgamma 0.06 (1.00 u) dbeta 0.00 (0.08 u)
    r_bwd_pg_bf16_H1024_2049_dres_dv2             2049 bwd_pg           | dv 0.50 (1.6e-02 / 1.6e-02) dv2 0.50 (2.4e-02 / 2.4e-02) dgamma 0.05 (0.84 u) keep2 0 differ
    r_bwd_pg_bf16_H1024_8G+1_plain                2049 bwd_pg           | dv 0.50 (1.6e-02 / 1.6e-02) dgamma 0.05 (0.81 u) dbeta 0.01 (0.11 u)
    r_bwd_pg_bf16_H1024_8G+1_dres                 2049 bwd_pg           | dv 0.50 (1.6e-02 / 1.6e-02) dgamma 0.06 (0.93 u) dbeta 0.01 (0.10 u)
    r_bwd_pg_bf16_H1024_8G+1_dv2p0                2049 bwd_pg           | dv 0.50 (1.6e-02 / 1.6e-02) dv2 0.50 (1.6e-02 / 1.6e-02) dgamma 0.05 (0.85 u)
    r_bwd_pg_bf16_H1024_8G+1_dres_dv2             2049 bwd_pg           | dv 0.50 (1.6e-02 / 1.6e-02) dv2 0.50 (1.6e-02 / 1.6e-02) dbeta 0.01 (0.22 u) keep2 0 differ
    r_bwd_pg_bf16_H1024_16G+5_plain               4101 bwd_pg           | dv 0.50 (1.6e-02 / 1.6e-02) dgamma 0.03 (0.49 u) dbeta 0.01 (0.24 u)
    r_bwd_pg_bf16_H1024_16G+5_dres                4101 bwd_pg           | dv 0.50 (1.6e-02 / 1.6e-02) dgamma 0.05 (0.76 u)
    r_bwd_pg_bf16_H1024_16G+5_dv2p0               4101 bwd_pg           | dv 0.50 (1.6e-02 / 1.6e-02) dv2 0.50 (1.6e-02 / 1.6e-02) dbeta 0.01 (0.14 u)
    r_bwd_pg_bf16_H1024_16G+5_dres_dv2            4101 bwd_pg           | dv 0.50 (1.6e-02 / 1.6e-02) dv2 0.50 (2.7e-02 / 2.7e-02) dgamma 0.04 (0.60 u) dbeta 0.01 (0.16 u) keep2 0 differ
    r_fwd_lean_f32_H72_M1                            1 fwd_lean         | y 0.14 (1.5e-07) mean 0.09 (3.2e-08) rstd 0.01 (3.2e-09)
    r_bwd_gen_f32_H72_M1                             1 bwd_general<1,1> | dv 0.22 (1.4e-07) dgamma 0.08 (1.21 u) dbeta 0.06 (0.99 u) dbias 0.09 (1.40 u)
    r_fwd_lean_f32_H72_M3                            3 fwd_lean         | y 0.14 (2.4e-07) mean 0.31 (5.5e-08) rstd 0.09 (2.9e-08)
    r_bwd_gen_f32_H72_M3                             3 bwd_general<1,1> | dv 0.25 (2.7e-07) dgamma 0.11 (1.70 u) dbeta 0.08 (1.29 u) dbias 0.11 (1.69 u)
    r_fwd_lean_f32_H72_M4                            4 fwd_lean         | y 0.17 (2.2e-07) mean 0.11 (8.1e-08) rstd 0.09 (2.4e-08)
    r_bwd_gen_f32_H72_M4                             4 bwd_general<1,1> | dv 0.25 (2.8e-07) dgamma 0.11 (1.82 u) dbeta 0.07 (1.08 u) dbias 0.13 (2.00 u)
    r_fwd_lean_f32_H72_M5                            5 fwd_lean         | y 0.19 (2.9e-07) mean 0.58 (1.4e-07) rstd 0.17 (4.5e-08)
    r_bwd_gen_f32_H72_M5                             5 bwd_general<1,1> | dv 0.25 (5.0e-07) dgamma 0.09 (1.40 u) dbeta 0.07 (1.10 u) dbias 0.10 (1.54 u)
    r_bwd_gen_f32_H72_M4101                       4101 bwd_general<1,1> | dv 0.25 (6.9e-07) dgamma 0.05 (0.82 u) dbeta 0.05 (0.73 u) dbias 0.04 (0.64 u)
    r_fwd_lean_f32_H72_M8195                      8195 fwd_lean         | y 0.31 (9.2e-07) mean 0.25 (3.9e-07) rstd 0.23 (1.4e-07)
    r_fwd_gen_f32_H72_M8195                       8195 fwd_general      | y 0.18 (7.6e-07) mean 0.23 (3.3e-07) rstd 0.17 (9.6e-08)
    r_fwd_lean_f32_H72_M24593                    24593 fwd_lean         | y 0.21 (8.3e-07) mean 0.30 (5.2e-07) rstd 0.24 (1.5e-07)
    r_fwd_gen_f32_H72_M24593                     24593 fwd_general      | y 0.24 (8.5e-07) mean 0.25 (3.7e-07) rstd 0.21 (1.0e-07)
    r_bwd_pg_f32_H72_2047_plain                   2047 bwd_general<1,0> | dv 0.25 (5.5e-07) dgamma 0.07 (1.14 u) dbeta 0.04 (0.69 u)
    r_bwd_pg_f32_H72_2047_dres                    2047 bwd_general<1,0> | dv 0.25 (5.5e-07) dgamma 0.08 (1.21 u)
    r_bwd_pg_f32_H72_2047_dv2p0                   2047 bwd_general<1,0> | dv 0.25 (6.6e-07) dv2 0.25 (6.6e-07) dbeta 0.04 (0.67 u)
    r_bwd_pg_f32_H72_2047_dres_dv2                2047 bwd_general<1,0> | dv 0.25 (7.2e-07) dv2 0.25 (9.5e-07) dgamma 0.06 (1.00 u) dbeta 0.03 (0.47 u) keep2 0 differ
    r_bwd_pg_f32_H72_2048_plain                   2048 bwd_pg           | dv 0.25 (5.6e-07) dgamma 0.03 (0.48 u)
    r_bwd_pg_f32_H72_2048_dres                    2048 bwd_pg           | dv 0.22 (5.8e-07) dbeta 0.04 (0.62 u)
    r_bwd_pg_f32_H72_2048_dv2p0                   2048 bwd_pg           | dv 0.19 (4.9e-07) dv2 0.19 (4.9e-07) dgamma 0.04 (0.65 u) dbeta 0.02 (0.40 u)
    r_bwd_pg_f32_H72_2048_dres_dv2                2048 bwd_pg           | dv 0.12 (4.3e-07) dv2 0.13 (6.3e-07) dgamma 0.04 (0.68 u) dbeta 0.04 (0.61 u) keep2 0 differ
    r_bwd_pg_f32_H72_2049_plain                   2049 bwd_pg           | dv 0.25 (6.6e-07) dbeta 0.03 (0.45 u)
    r_bwd_pg_f32_H72_2049_dres                    2049 bwd_pg           | dv 0.18 (4.8e-07) dgamma 0.03 (0.41 u) dbeta 0.03 (0.42 u)
    r_bwd_pg_f32_H72_2049_dv2p0                   2049 bwd_pg           | dv 0.25 (6.5e-07) dv2 0.25 (6.5e-07) dgamma 0.03 (0.49 u) dbeta 0.03 (0.56 u)
    r_bwd_pg_f32_H72_2049_dres_dv2                2049 bwd_pg           | dv 0.19 (4.7e-07) dv2 0.23 (7.0e-07) dgamma 0.03 (0.46 u) keep2 0 differ
    r_bwd_pg_f32_H72_8G+1_plain                   2049 bwd_pg           | dv 0.25 (5.2e-07) dgamma 0.06 (0.94 u) dbeta 0.01 (0.24 u)
    r_bwd_pg_f32_H72_8G+1_dres                    2049 bwd_pg           | dv 0.15 (5.1e-07) dgamma 0.04 (0.58 u) dbeta 0.02 (0.29 u)
    r_bwd_pg_f32_H72_8G+1_dv2p0                   2049 bwd_pg           | dv 0.21 (5.6e-07) dv2 0.21 (5.6e-07) dgamma 0.06 (0.98 u)
    r_bwd_pg_f32_H72_8G+1_dres_dv2                2049 bwd_pg           | dv 0.14 (5.0e-07) dv2 0.16 (7.1e-07) dbeta 0.05 (0.87 u) keep2 0 differ
    r_bwd_pg_f32_H72_16G+5_plain                  4101 bwd_pg           | dv 0.23 (6.0e-07) dgamma 0.03 (0.52 u) dbeta 0.02 (0.28 u)
    r_bwd_pg_f32_H72_16G+5_dres                   4101 bwd_pg           | dv 0.18 (5.0e-07) dgamma 0.02 (0.34 u)
    r_bwd_pg_f32_H72_16G+5_dv2p0                  4101 bwd_pg           | dv 0.21 (5.6e-07) dv2 0.21 (5.6e-07) dbeta 0.02 (0.39 u)
    r_bwd_pg_f32_H72_16G+5_dres_dv2               4101 bwd_pg           | dv 0.20 (5.3e-07) dv2 0.23 (7.7e-07) dgamma 0.02 (0.30 u) dbeta 0.03 (0.45 u) keep2 0 differ
    r_fwd_lean_f32_H1024_M1                          1 fwd_lean         | y 0.24 (2.7e-07) mean 0.03 (5.9e-10) rstd 0.05 (1.1e-08)
    r_bwd_gen_f32_H1024_M1                           1 bwd_general<1,1> | dv 0.23 (3.0e-07) dgamma 0.12 (1.91 u) dbeta 0.06 (1.00 u) dbias 0.14 (2.21 u)
    r_fwd_lean_f32_H1024_M3                          3 fwd_lean         | y 0.18 (4.6e-07) mean 0.25 (4.2e-08) rstd 0.08 (2.8e-08)
    r_bwd_gen_f32_H1024_M3                           3 bwd_general<1,1> | dv 0.25 (5.5e-07) dgamma 0.14 (2.26 u) dbeta 0.09 (1.49 u) dbias 0.13 (2.09 u)
    r_fwd_lean_f32_H1024_M4                          4 fwd_lean         | y 0.25 (4.1e-07) mean 0.11 (2.8e-08) rstd 0.31 (7.6e-08)
    r_bwd_gen_f32_H1024_M4                           4 bwd_general<1,1> | dv 0.24 (3.7e-07) dgamma 0.13 (2.06 u) dbeta 0.11 (1.83 u) dbias 0.13 (2.12 u)
    r_fwd_lean_f32_H1024_M5                          5 fwd_lean         | y 0.30 (6.1e-07) mean 0.09 (1.1e-08) rstd 0.25 (8.5e-08)
    r_bwd_gen_f32_H1024_M5                           5 bwd_general<1,1> | dv 0.25 (4.8e-07) dgamma 0.13 (2.14 u) dbeta 0.11 (1.72 u) dbias 0.12 (1.90 u)
    r_bwd_gen_f32_H1024_M4101                     4101 bwd_general<1,1> | dv 0.25 (8.1e-07) dgamma 0.07 (1.20 u) dbeta 0.05 (0.85 u) dbias 0.06 (1.01 u)
    r_fwd_lean_f32_H1024_M8195                    8195 fwd_lean         | y 0.23 (9.4e-07) mean 0.22 (4.3e-07) rstd 0.23 (1.4e-07)
    r_fwd_gen_f32_H1024_M8195                     8195 fwd_general      | y 0.23 (1.0e-06) mean 0.28 (3.0e-07) rstd 0.23 (8.6e-08)
    r_fwd_lean_f32_H1024_M24593                  24593 fwd_lean         | y 0.21 (1.0e-06) mean 0.26 (3.2e-07) rstd 0.25 (1.4e-07)
    r_fwd_gen_f32_H1024_M24593                   24593 fwd_general      | y 0.24 (1.2e-06) mean 0.25 (3.2e-07) rstd 0.24 (9.9e-08)
    r_bwd_pg_f32_H1024_2047_plain                 2047 bwd_general<1,0> | dv 0.25 (8.8e-07) dgamma 0.06 (1.00 u) dbeta 0.06 (0.93 u)
    r_bwd_pg_f32_H1024_2047_dres                  2047 bwd_general<1,0> | dv 0.25 (1.0e-06) dgamma 0.12 (1.86 u)
    r_bwd_pg_f32_H1024_2047_dv2p0                 2047 bwd_general<1,0> | dv 0.25 (7.6e-07) dv2 0.25 (7.6e-07) dbeta 0.06 (0.97 u)
    r_bwd_pg_f32_H1024_2047_dres_dv2              2047 bwd_general<1,0> | dv 0.25 (9.5e-07) dv2 0.25 (1.1e-06) dgamma 0.09 (1.42 u) dbeta 0.06 (0.97 u) keep2 0 differ
    r_bwd_pg_f32_H1024_2048_plain                 2048 bwd_pg           | dv 0.19 (6.5e-07) dgamma 0.05 (0.82 u)
    r_bwd_pg_f32_H1024_2048_dres                  2048 bwd_pg           | dv 0.18 (6.5e-07) dbeta 0.05 (0.79 u)
    r_bwd_pg_f32_H1024_2048_dv2p0                 2048 bwd_pg           | dv 0.19 (6.4e-07) dv2 0.19 (6.4e-07) dgamma 0.05 (0.88 u) dbeta 0.04 (0.68 u)
    r_bwd_pg_f32_H1024_2048_dres_dv2              2048 bwd_pg           | dv 0.19 (6.5e-07) dv2 0.25 (9.1e-07) dgamma 0.05 (0.87 u) dbeta 0.04 (0.72 u) keep2 0 differ
    r_bwd_pg_f32_H1024_2049_plain                 2049 bwd_pg           | dv 0.20 (6.5e-07) dbeta 0.04 (0.62 u)
    r_bwd_pg_f32_H1024_2049_dres                  2049 bwd_pg           | dv 0.19 (6.5e-07) dgamma 0.06 (0.90 u) dbeta 0.04 (0.67 u)
    r_bwd_pg_f32_H1024_2049_dv2p0                 2049 bwd_pg           | dv 0.18 (6.2e-07) dv2 0.18 (6.2e-07) dgamma 0.06 (0.98 u) dbeta 0.05 (0.76 u)
    r_bwd_pg_f32_H1024_2049_dres_dv2              2049 bwd_pg           | dv 0.21 (7.8e-07) dv2 0.19 (9.3e-07) dgamma 0.06 (0.89 u) keep2 0 differ
    r_bwd_pg_f32_H1024_8G+1_plain                 2049 bwd_pg           | dv 0.24 (6.5e-07) dgamma 0.05 (0.85 u) dbeta 0.04 (0.62 u)
    r_bwd_pg_f32_H1024_8G+1_dres                  2049 bwd_pg           | dv 0.19 (6.0e-07) dgamma 0.06 (1.03 u) dbeta 0.04 (0.64 u)
    r_bwd_pg_f32_H1024_8G+1_dv2p0                 2049 bwd_pg           | dv 0.20 (6.4e-07) dv2 0.20 (6.4e-07) dgamma 0.07 (1.18 u)
    r_bwd_pg_f32_H1024_8G+1_dres_dv2              2049 bwd_pg           | dv 0.20 (6.6e-07) dv2 0.23 (8.5e-07) dbeta 0.04 (0.63 u) keep2 0 differ
    r_bwd_pg_f32_H1024_16G+5_plain                4101 bwd_pg           | dv 0.20 (6.6e-07) dgamma 0.04 (0.66 u) dbeta 0.02 (0.39 u)
    r_bwd_pg_f32_H1024_16G+5_dres                 4101 bwd_pg           | dv 0.20 (7.4e-07) dgamma 0.05 (0.73 u)
    r_bwd_pg_f32_H1024_16G+5_dv2p0                4101 bwd_pg           | dv 0.20 (6.2e-07) dv2 0.20 (6.2e-07) dbeta 0.03 (0.48 u)
    r_bwd_pg_f32_H1024_16G+5_dres_dv2             4101 bwd_pg           | dv 0.22 (7.8e-07) dv2 0.24 (1.1e-06) dgamma 0.06 (1.03 u) dbeta 0.03 (0.44 u) keep2 0 differ
    gather_rows / scatter_rows bf16 n=5 step=3 H=72: bit-equal, sentinels intact
    gather_rows / scatter_rows bf16 n=4100 step=2 H=1024: bit-equal, sentinels intact
    gather_rows / scatter_rows f32 n=5 step=3 H=72: bit-equal, sentinels intact
    gather_rows / scatter_rows f32 n=2100 step=2 H=1024: bit-equal, sentinels intact
    scatter_rows_fill bf16 n=5 step=3 H=72 fill_rows=13: bit-equal, sentinels intact
    scatter_rows_fill bf16 n=2100 step=4 H=1024 fill_rows=8400: bit-equal, sentinels intact
    scatter_rows_fill f32 n=5 step=3 H=72 fill_rows=17: bit-equal, sentinels intact
    scatter_rows_fill f32 n=1400 step=3 H=1024 fill_rows=4200: bit-equal, sentinels intact
    rows_idx_copy bf16 n=5 H=72 scatter=False: bit-equal, sentinels intact
    rows_idx_copy bf16 n=5 H=72 scatter=True: bit-equal, sentinels intact
    rows_idx_copy bf16 n=4100 H=1024 scatter=False: bit-equal, sentinels intact
    rows_idx_copy bf16 n=4100 H=1024 scatter=True: bit-equal, sentinels intact
    rows_idx_copy f32 n=5 H=72 scatter=False: bit-equal, sentinels intact
    rows_idx_copy f32 n=5 H=72 scatter=True: bit-equal, sentinels intact
    rows_idx_copy f32 n=2100 H=1024 scatter=False: bit-equal, sentinels intact
    rows_idx_copy f32 n=2100 H=1024 scatter=True: bit-equal, sentinels intact
    dropout_apply bf16 M=37 N=72 p=0.1: mask equals the host mask, values bit-equal, sentinels intact
    dropout_apply bf16 M=37 N=520 p=0.5: mask equals the host mask, values bit-equal, sentinels intact
    dropout_apply bf16 M=8200 N=1032 p=0.1: mask equals the host mask, values bit-equal, sentinels intact
    dropout_apply f32 M=37 N=72 p=0.1: mask equals the host mask, values bit-equal, sentinels intact
    dropout_apply f32 M=37 N=520 p=0.5: mask equals the host mask, values bit-equal, sentinels intact
    dropout_apply f32 M=8200 N=1032 p=0.1: mask equals the host mask, values bit-equal, sentinels intact
    act_bwd_f32 act=1 n=524293: max error 0.00e+00, worst error / bound 0.00
    act_bwd_f32 act=2 n=524293: max error 6.74e-07, worst error / bound 0.25
    act_bwd_f32 act=3 n=524293: max error 1.61e-06, worst error / bound 0.57
    act_bwd_f32 act=4 n=524293: max error 2.68e-09, worst error / bound 0.68
"""
import functools

import pytest
import torch

import adapter_ln_ref as A
import ln_rows_ref as R
from attn_ref import JUNK, SENTINEL

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@functools.lru_cache(maxsize=None)
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def walk():
    return {s['name']: s for s in R.walk_specs(cus())}


WALK_NAMES = [s['name'] for s in R.walk_specs(256)]             # (the names do not depend on G, the row counts of '8G+1' / '16G+5' do)
TABLE = {s['name']: s for s in R.width_specs() + R.form_specs() + R.cond_specs()}


def check(spec):
    from adapter4rec_amd import _lib as L
    c = R.build(spec, DEV)
    got = R.run(c, L)
    figures, fails = R.judge(c, got, c.ref, c.fig)
    near = R.near_bound(figures)
    print('KERNEL ' + R.table_row(c, figures) + (f'   NEAR {near}' if near else ''))
    assert not fails, (c.name, fails)


@pytest.mark.parametrize('name', [n for n in TABLE if n.startswith('w_')])
def test_width_sweep(name):
    """ng = H / 8 at 1, 63 / 64 / 65 (the lane map's second group absent, exactly empty, live in one lane: H = 520 is where the clamped gamma index of
    the lean and pg kernels would show), 127 / 128; the quantiser's own layout at ng = 1, 64, 65, 511, 512.  M = 37: ten workgroups, the last with one
    live wave."""
    check(TABLE[name])


@pytest.mark.parametrize('name', [n for n in TABLE if n.startswith('f_')])
def test_forms(name):
    """every <WGB, WDB> instantiation with one-sided sums; add_rows 1, 20, M, M + 3; dropout 0.1 / 0.5 forward and the backward through the same
    mask; dv2 through a second mask; every optional output of ln_fwd_sum with res and with res32; ln_fwd_fp8 with and without y"""
    check(TABLE[name])


@pytest.mark.parametrize('name', [n for n in TABLE if n.startswith('c_')])
def test_conditioning(name):
    """rows of mean 1000 (fp32) / 64 (bf16) and unit spread; a constant row (variance 0) and a row of zeros; rows of zeros into the quantiser of
    ln_fwd_fp8; eps 1e-6 and 1e-12"""
    check(TABLE[name])


@pytest.mark.parametrize('name', WALK_NAMES)
def test_row_count_walk(name):
    """M = 1, 3, 4, 5 around a workgroup's four waves; 4096 + 5 rows under the general backward's 1024-block cap (some waves sum two rows);
    8192 + 3 and 3 x 8192 + 17 rows through both forward kernels (a second and a third row per wave, the lean kernel's prefetch); the pg kernel at
    2047 (still the general kernel), 2048, 2049, 8 G + 1 and 16 G + 5 rows, with and without dres and dv2"""
    check(walk()[name])


# ------------------------------------------------------------------ copy helpers
def _strided(rows, W, dtype, wide, fill, data=None):
    ld, c0 = R._layout(W, wide)
    buf = torch.full((rows, ld), fill, dtype=dtype, device=DEV)
    vw = buf[:, c0:c0 + W]
    if data is not None:
        vw[:data.shape[0]] = data
    return buf, vw, c0


def _rows(n, W, dtype, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(n, W, generator=g, device=DEV).to(dtype)


def _outside_intact(buf, c0, W, rows_written, what):
    keep = torch.ones(buf.shape[0], dtype=torch.bool, device=DEV)
    keep[rows_written] = False
    assert bool((buf[keep] == SENTINEL).all()), f'{what}: a row outside the copy was written'
    assert bool((buf[:, :c0] == SENTINEL).all()) and bool((buf[:, c0 + W:] == SENTINEL).all()), f'{what}: a gap column was written'


# (n, row_step, H): small and odd; then pieces = n * H * esz / 16 past 2048 blocks x 256 threads (4096 x 256 for the fill)
COPY_SHAPES = {'f32': [(5, 3, 72), (2100, 2, 1024)], 'bf16': [(5, 3, 72), (4100, 2, 1024)]}
FILL_SHAPES = {'f32': [(5, 3, 72, 17), (1400, 3, 1024, 4200)], 'bf16': [(5, 3, 72, 13), (2100, 4, 1024, 8400)]}


@pytest.mark.parametrize('big', [0, 1])
@pytest.mark.parametrize('dt', R.DTYPES)
def test_gather_scatter_rows(dt, big):
    from adapter4rec_amd import _lib as L
    n, step, H = COPY_SHAPES[dt][big]
    T, wide = R.DT[dt], (8, 64)[big]
    assert not big or n * (H * T.itemsize // 16) > 2048 * 256
    data = _rows(n * step + 2, H, T, 11 + big)
    sbuf, src, _ = _strided(n * step + 2 + R.PAD_ROWS, H, T, wide, JUNK, data)
    dbuf, dst, c0 = _strided(n + R.PAD_ROWS, H, T, 72 - wide, SENTINEL)
    before = sbuf.clone()
    L.gather_rows(src, dst, n, step)
    torch.cuda.synchronize()
    assert torch.equal(dst[:n], data[0:n * step:step]) and torch.equal(sbuf, before)
    _outside_intact(dbuf, c0, H, slice(0, n), 'gather_rows')
    small = _rows(n, H, T, 13 + big)
    sbuf, src, _ = _strided(n + R.PAD_ROWS, H, T, 72 - wide, JUNK, small)
    dbuf, dst, c0 = _strided(n * step + R.PAD_ROWS, H, T, wide, SENTINEL)
    L.scatter_rows(src, dst, n, step)
    torch.cuda.synchronize()
    assert torch.equal(dst[0:n * step:step][:n], small)
    _outside_intact(dbuf, c0, H, slice(0, (n - 1) * step + 1, step), 'scatter_rows')
    print(f'KERNEL gather_rows / scatter_rows {dt} n={n} step={step} H={H}: bit-equal, sentinels intact')


@pytest.mark.parametrize('big', [0, 1])
@pytest.mark.parametrize('dt', R.DTYPES)
def test_scatter_rows_fill(dt, big):
    from adapter4rec_amd import _lib as L
    n, step, H, fill_rows = FILL_SHAPES[dt][big]
    T, wide = R.DT[dt], (64, 8)[big]
    assert not big or fill_rows * (H * T.itemsize // 16) > 4096 * 256
    small = _rows(n, H, T, 17 + big)
    sbuf, src, _ = _strided(n + R.PAD_ROWS, H, T, wide, JUNK, small)
    dbuf, dst, c0 = _strided(fill_rows + R.PAD_ROWS, H, T, 72 - wide, SENTINEL)
    L.scatter_rows_fill(src, dst, n, step, fill_rows)
    torch.cuda.synchronize()
    want = torch.zeros(fill_rows, H, dtype=T, device=DEV)
    want[0:n * step:step] = small
    assert torch.equal(dst[:fill_rows], want)
    _outside_intact(dbuf, c0, H, slice(0, fill_rows), 'scatter_rows_fill')
    print(f'KERNEL scatter_rows_fill {dt} n={n} step={step} H={H} fill_rows={fill_rows}: bit-equal, sentinels intact')


@pytest.mark.parametrize('scatter', [False, True])
@pytest.mark.parametrize('big', [0, 1])
@pytest.mark.parametrize('dt', R.DTYPES)
def test_rows_idx_copy(dt, big, scatter):
    from adapter4rec_amd import _lib as L
    n, _, H = COPY_SHAPES[dt][big]
    T, wide = R.DT[dt], (8, 64)[big]
    pool = n + 7                                                       # rows on the indexed side: more than are used, none twice
    idx = torch.randperm(pool, generator=torch.Generator().manual_seed(23 + big))[:n].to(torch.int32).to(DEV)
    data = _rows(n if scatter else pool, H, T, 19 + big)
    sbuf, src, _ = _strided(data.shape[0] + R.PAD_ROWS, H, T, wide, JUNK, data)
    dbuf, dst, c0 = _strided((pool if scatter else n) + R.PAD_ROWS, H, T, 72 - wide, SENTINEL)
    before = sbuf.clone()
    L.rows_idx_copy(src, dst, idx, n, scatter=scatter)
    torch.cuda.synchronize()
    assert torch.equal(sbuf, before)
    if scatter:
        assert torch.equal(dst[idx.long()], data)
        written = idx.long()
    else:
        assert torch.equal(dst[:n], data[idx.long()])
        written = slice(0, n)
    _outside_intact(dbuf, c0, H, written, 'rows_idx_copy')
    print(f'KERNEL rows_idx_copy {dt} n={n} H={H} scatter={scatter}: bit-equal, sentinels intact')


# ------------------------------------------------------------------ dropout_apply, act_bwd_f32
@functools.lru_cache(maxsize=None)
def _apply_mask(M, N, p):
    return R.host_mask(0x77 * 1000003 + N, 5, M, N, p).to(DEV)


@pytest.mark.parametrize('M,N,p', [(37, 72, 0.1), (37, 520, 0.5), (8200, 1032, 0.1)])
@pytest.mark.parametrize('dt', R.DTYPES)
def test_dropout_apply_against_host_mask(dt, M, N, p):
    """the last shape: M N / 8 = 1 057 800 > 4096 blocks x 256 threads, the grid-stride loop's second round"""
    from adapter4rec_amd import _lib as L
    T = R.DT[dt]
    data = _rows(M, N, T, 29)
    data = torch.where(data == 0, torch.ones_like(data), data)
    xbuf, x, _ = _strided(M + R.PAD_ROWS, N, T, 8, JUNK, data)
    ybuf, y, c0 = _strided(M + R.PAD_ROWS, N, T, 64, SENTINEL)
    before = xbuf.clone()
    L.dropout_apply(x, y, p, 5, 0x77 * 1000003 + N, M=M)
    torch.cuda.synchronize()
    km = _apply_mask(M, N, p)
    diff = int(((y[:M] == 0) != (km == 0)).sum())
    assert diff == 0, f'{diff} elements zeroed where the host mask keeps them, or the reverse'
    assert 0.8 * p < float((km == 0).double().mean()) < 1.2 * p
    assert torch.equal(y[:M], (data.float() * km.float()).to(T)) and torch.equal(xbuf, before)
    _outside_intact(ybuf, c0, N, slice(0, M), 'dropout_apply')
    print(f'KERNEL dropout_apply {dt} M={M} N={N} p={p}: mask equals the host mask, values bit-equal, sentinels intact')


E_ACT = {1: 0.0, 2: 2.0 ** -20 + 1.5e-7, 3: 2.0 ** -20, 4: 0.0}


@pytest.mark.parametrize('act', [1, 2, 3, 4])
def test_act_bwd_f32(act):
    from adapter4rec_amd import _lib as L
    n = 524288 + 5
    buf = torch.full((3, n + 16), SENTINEL, dtype=torch.float32, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(31 + act)
    buf[0, 4:4 + n] = torch.randn(n, generator=g, device=DEV)
    buf[1, 4:4 + n] = torch.randn(n, generator=g, device=DEV) * 2
    dy, pre, dx = (buf[i, 4:4 + n] for i in range(3))
    before = buf[:2].clone()
    L.act_bwd_f32(dy, pre, dx, act)
    torch.cuda.synchronize()
    da = A.dact64(pre.double(), act)
    err = (dx.double() - dy.double() * da).abs()
    lim = dy.double().abs() * (E_ACT[act] + 2.0 ** -23 * da.abs())
    worst = float((err / lim.clamp(min=1e-300)).max())
    print(f'KERNEL act_bwd_f32 act={act} n={n}: max error {float(err.max()):.2e}, worst error / bound {worst:.2f}' + ('   NEAR' if worst > 0.8 else ''))
    assert bool((err <= lim).all()), worst
    assert torch.equal(buf[:2], before) and bool((buf[2, :4] == SENTINEL).all()) and bool((buf[2, 4 + n:] == SENTINEL).all())


# ------------------------------------------------------------------ rejections: argument checks, nothing is launched
def _t(rows, W, dt=torch.float32, fill=0.0):
    return torch.full((rows, W), fill, dtype=dt, device=DEV)


def _overlap(rows, W, ld, dt=torch.float32):
    """a [rows, W] view whose rows lie ld < W elements apart (inside a buffer of rows x W elements)"""
    return torch.as_strided(_t(rows, W, dt), (rows, W), (ld, 1))


def _off(rows, W, by, dt=torch.float32):
    """a [rows, W] view that starts `by` elements into a row of a wider buffer: a base that is not 16-byte aligned"""
    return _t(rows, W + 16, dt)[:, by:by + W]


def _ln_args(H=64, M=8, dt=torch.float32):
    return dict(v=_t(M, H, dt), gamma=_t(1, H).view(-1), beta=_t(1, H).view(-1), y=_t(M, H, dt), stats=_t(M, 2), dy=_t(M, H, dt), dv=_t(M, H, dt))


def _fwd(L, a, **kw):
    L.ln_fwd(kw.pop('v', a['v']), a['gamma'], a['beta'], 1e-12, kw.pop('y', a['y']), a['stats'], **kw)


def _bwd(L, a, **kw):
    L.ln_bwd(kw.pop('dy', a['dy']), kw.pop('v', a['v']), a['stats'], a['gamma'], kw.pop('dv', a['dv']), **kw)


def _sum(L, a, **kw):
    L.ln_fwd_sum(kw.pop('h', a['v']), kw.pop('res', a['dy']), a['gamma'], a['beta'], 1e-12, kw.pop('y', a['y']), a['stats'], **kw)


def _raw_add_rows(L, a, bwd):
    """add given with add_rows = 0: the wrapper cannot say that (it passes add.shape[0]), the C entry point is called as the wrapper calls it"""
    add, H, M = _t(4, 64), 64, 8
    p = lambda t: t.data_ptr()
    if bwd:
        rc = L.lib().a4r_ln_bwd(L._stream(), p(a['dy']), H, p(a['v']), H, p(add), 0, p(a['stats']), p(a['gamma']), None, 0, p(a['dv']), H, None, None, None,
                                M, H, L.F32, 0.0, 0, 0, None, 0, 0.0, 0, 0)
    else:
        rc = L.lib().a4r_ln_fwd(L._stream(), p(a['v']), H, p(add), 0, p(a['gamma']), p(a['beta']), 1e-12, p(a['y']), H, p(a['stats']), M, H, L.F32, 0.0, 0, 0)
    L._check(rc, 'a4r_ln_' + ('bwd' if bwd else 'fwd'))


REJECTIONS = {
    'fwd_H_not_8': lambda L: _fwd(L, _ln_args(H=12)),
    'fwd_H_above_1024': lambda L: _fwd(L, _ln_args(H=1032)),
    'fwd_ldv_below_H': lambda L: _fwd(L, _ln_args(), v=_overlap(8, 64, 32)),
    'fwd_ldy_below_H': lambda L: _fwd(L, _ln_args(), y=_overlap(8, 64, 32)),
    'fwd_v_misaligned': lambda L: _fwd(L, _ln_args(), v=_off(8, 64, 1)),
    'fwd_y_misaligned': lambda L: _fwd(L, _ln_args(), y=_off(8, 64, 2)),
    'fwd_bf16_ld_not_16_bytes': lambda L: _fwd(L, _ln_args(dt=torch.bfloat16), v=_t(8, 68, torch.bfloat16)[:, :64]),
    'fwd_add_rows_0': lambda L: _raw_add_rows(L, _ln_args(), False),
    'fwd_add_misaligned': lambda L: _fwd(L, _ln_args(), add=_t(5, 64).view(-1)[2:2 + 4 * 64].view(4, 64)),
    'fwd_drop_p_1': lambda L: _fwd(L, _ln_args(), drop_p=1.0),
    'fwd_drop_p_negative': lambda L: _fwd(L, _ln_args(), drop_p=-0.1),
    'fp8_ld8_below_H': lambda L: _fwd(L, _ln_args(), y8=_overlap(8, 64, 32, torch.uint8), ys=_t(1, 8).view(-1)),
    'fp8_y8_misaligned': lambda L: _fwd(L, _ln_args(), y8=_off(8, 64, 4, torch.uint8), ys=_t(1, 8).view(-1)),
    'fp8_ld8_not_8': lambda L: _fwd(L, _ln_args(), y8=_t(8, 68, torch.uint8)[:, :64], ys=_t(1, 8).view(-1)),
    'sum_H_not_8': lambda L: _sum(L, _ln_args(H=12)),
    'sum_H_above_1024': lambda L: _sum(L, _ln_args(H=1032)),
    'sum_ldh_below_H': lambda L: _sum(L, _ln_args(), h=_overlap(8, 64, 32)),
    'sum_res_misaligned': lambda L: _sum(L, _ln_args(), res=_off(8, 64, 1)),
    'sum_ld_res32_below_H': lambda L: _sum(L, _ln_args(), res=None, res32=_overlap(8, 64, 32)),
    'sum_sum_out_misaligned': lambda L: _sum(L, _ln_args(), sum_out=_off(8, 64, 1)),
    'sum_ld_sum32_below_H': lambda L: _sum(L, _ln_args(), sum32=_overlap(8, 64, 32)),
    'sum_y32_misaligned': lambda L: _sum(L, _ln_args(), y32=_off(8, 64, 3)),
    'bwd_H_not_8': lambda L: _bwd(L, _ln_args(H=12)),
    'bwd_H_above_1024': lambda L: _bwd(L, _ln_args(H=1032)),
    'bwd_lddy_below_H': lambda L: _bwd(L, _ln_args(), dy=_overlap(8, 64, 32)),
    'bwd_lddv_below_H': lambda L: _bwd(L, _ln_args(), dv=_overlap(8, 64, 32)),
    'bwd_v_misaligned': lambda L: _bwd(L, _ln_args(), v=_off(8, 64, 1)),
    'bwd_dres_misaligned': lambda L: _bwd(L, _ln_args(), dres=_off(8, 64, 1)),
    'bwd_lddres_below_H': lambda L: _bwd(L, _ln_args(), dres=_overlap(8, 64, 32)),
    'bwd_lddv2_below_H': lambda L: _bwd(L, _ln_args(), dv2=_overlap(8, 64, 32)),
    'bwd_dv2_misaligned': lambda L: _bwd(L, _ln_args(), dv2=_off(8, 64, 2)),
    'bwd_add_rows_0': lambda L: _raw_add_rows(L, _ln_args(), True),
    'bwd_drop_p_1': lambda L: _bwd(L, _ln_args(), drop_p=1.0),
    'bwd_drop2_p_1': lambda L: _bwd(L, _ln_args(), dv2=_t(8, 64), drop2_p=1.0),
    'bwd_drop2_p_negative': lambda L: _bwd(L, _ln_args(), dv2=_t(8, 64), drop2_p=-0.5),
    'quant_H_not_8': lambda L: L.quant_rows_fp8(_t(8, 12), _t(8, 16, torch.uint8), _t(1, 8).view(-1)),
    'quant_H_above_4096': lambda L: L.quant_rows_fp8(_t(8, 4104), _t(8, 4104, torch.uint8), _t(1, 8).view(-1)),
    'quant_ldx_below_H': lambda L: L.quant_rows_fp8(_overlap(8, 64, 32), _t(8, 64, torch.uint8), _t(1, 8).view(-1)),
    'quant_ldq_below_H': lambda L: L.quant_rows_fp8(_t(8, 64), _overlap(8, 64, 32, torch.uint8), _t(1, 8).view(-1)),
    'quant_x_misaligned': lambda L: L.quant_rows_fp8(_off(8, 64, 1), _t(8, 64, torch.uint8), _t(1, 8).view(-1)),
    'quant_q_misaligned': lambda L: L.quant_rows_fp8(_t(8, 64), _off(8, 64, 4, torch.uint8), _t(1, 8).view(-1)),
    'gather_ldi_below_H': lambda L: L.gather_rows(_overlap(8, 64, 32), _t(4, 64), 4, 2),
    'gather_ldo_below_H': lambda L: L.gather_rows(_t(8, 64), _overlap(4, 64, 32), 4, 2),
    'scatter_ldi_below_H': lambda L: L.scatter_rows(_overlap(4, 64, 32), _t(8, 64), 4, 2),
    'scatter_ldo_below_H': lambda L: L.scatter_rows(_t(4, 64), _overlap(8, 64, 32), 4, 2),
    'gather_src_misaligned': lambda L: L.gather_rows(_off(8, 64, 1), _t(4, 64), 4, 2),
    'gather_H_not_16_bytes': lambda L: L.gather_rows(_t(8, 8, torch.bfloat16)[:, :4], _t(4, 8, torch.bfloat16)[:, :4], 4, 2),
    'fill_rows_too_few': lambda L: L.scatter_rows_fill(_t(4, 64), _t(8, 64), 4, 2, 6),
    'fill_dst_misaligned': lambda L: L.scatter_rows_fill(_t(4, 64), _off(8, 64, 1), 4, 2, 8),
    'idx_copy_ld_below_row': lambda L: L.rows_idx_copy(_overlap(8, 64, 32), _t(4, 64), torch.zeros(4, dtype=torch.int32, device=DEV), 4),
    'idx_copy_dst_misaligned': lambda L: L.rows_idx_copy(_t(8, 64), _off(4, 64, 1), torch.zeros(4, dtype=torch.int32, device=DEV), 4),
    'dropout_apply_N_not_8': lambda L: L.dropout_apply(_t(8, 12), _t(8, 12), 0.1, 1, 2),
    'dropout_apply_ldx_below_N': lambda L: L.dropout_apply(_overlap(8, 64, 32), _t(8, 64), 0.1, 1, 2),
    'dropout_apply_y_misaligned': lambda L: L.dropout_apply(_t(8, 64), _off(8, 64, 1), 0.1, 1, 2),
    'dropout_apply_p_1': lambda L: L.dropout_apply(_t(8, 64), _t(8, 64), 1.0, 1, 2),
    'dropout_apply_p_negative': lambda L: L.dropout_apply(_t(8, 64), _t(8, 64), -0.1, 1, 2),
}


@pytest.mark.parametrize('name', list(REJECTIONS))
def test_launch_guard_rejects(name):
    from adapter4rec_amd import _lib as L
    with pytest.raises(RuntimeError, match='invalid argument'):
        REJECTIONS[name](L)
    torch.cuda.synchronize()
