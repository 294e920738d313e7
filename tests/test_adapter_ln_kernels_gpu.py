"""The fused adapter + LayerNorm kernels (a4r_adapter_ln_fwd / a4r_adapter_ln_bwd: csrc/a4r_adapter_fused.hip) against the fp64 reference of
tests/adapter_ln_ref.py at their form and launch edges, on the cases tests/test_adapter_ln_ref_cpu.py proves sound: every tensor with a leading
dimension a view into a wider buffer, junk in gap columns and pad rows, every output pre-filled with a sentinel that must survive outside rows < M
and columns < H, column sums started from 0.5 inside an arena of sentinels.  Bounds: adapter_ln_ref.judge (its header derives them).

G = the CU count rounded down to a multiple of 8 = the grid of both persistent kernels once M / 16 >= G.  References are computed on the device in
fp64, once per case.

INSTANTIATIONS.  Forward adapter_ln_fwd_kernel<CW, NW, RM>: RM = 0 (bf16 residual), 1 (res32 fp32), 2 (byte plane), 3 (nibble plane) at every width
128 .. 1024: the cases fwd_*_H<width>_{bf16, f32, lo8, lo4}_* of the form sweep.  Backward adapter_ln_bwd_kernel<CW, NW, WGB, WDB, DRES, FY>, the ten
that launch_bwd_d can pick, at every width 128 .. 768 (adapter_ln_ref.BWD_FORMS; the CPU file asserts the table is complete):
    WGB WDB DRES FY    forms of the sweep (bwd_*_H<width>_<form>)
    0   0   0    0     plain
    0   1   0    0     bias, bias_tot
    1   0   0    0     ln, g_only (dbeta null), b_only (dgamma null)
    1   1   0    0     all
    0   0   1    0     res
    0   1   1    0     res_bias (dbias before dres), res_biastot (after)
    1   0   1    0     res_ln
    1   1   1    0     res_all (before), vit (after: the image tower's call), res_b_only (dgamma null)
    0   0   0    1     from_y
    0   1   0    1     from_y_bias
Schedules: DEEP (rows two tiles ahead) at CW < 96 always and at H = 768 without WGB and DRES; the launch walk runs H = 256 and both schedules of 768.

MEASURED on an MI355X (G = 256; the KERNEL lines the tests print).  Per case: M; the bf16 tensor nearest its tile bound, its maximum error kernel / model and the relative RMS error kernel / model on that tile (bound: twice the
model's); then every other figure, in brackets its worst error / bound: mean, rstd, y32 / y24 / y20 / y8 with their maximum error; the column sums with
their worst error in units u = 2^-24 (0.5 + sum |term|) and, in brackets, the share in use of what the bound adds to the model's error (16 u, for dbd
plus the rounding-flip term).
Within 20 % of a bound (marked NEAR): no bf16 tensor -- the worst tile RMS is 1.01 x the model's, i.e. 0.51 of its bound, every maximum error equals
the model's --, no column sum (worst 1.84 u of 16; dbd 0.14 of its remainder), not rstd (0.51) and not y32 (0.32).  NEAR by construction: y20 (0.99),
y24 (0.97) and y8 (0.94), whose bounds are the formats' own worst-case rounding, which some element of every case comes close to; and mean (up to
0.99) in rows where an element of z did round the other way in fp32 than in fp64: the error then IS the allowance computed for that row.

    case                                       M  bf16: max error k / m, tile RMS k / m       | the rest
    fwd_m48_H128_bf16_houlsby_vy              48  y   1.5e-02 / 1.5e-02  1.71e-03 / 1.71e-03 | mean 2.4e-08 (0.08) rstd 6.5e-08 (0.34)
    fwd_m48_H128_f32_houlsby_gelu_y           48  zp  3.9e-03 / 3.9e-03  1.62e-03 / 1.62e-03 | mean 2.9e-08 (0.07) rstd 6.8e-08 (0.32) y32 4.3e-07 (0.24)
    fwd_m48_H128_lo8_compacter_vy8            48  zp  7.5e-03 / 7.5e-03  1.69e-03 / 1.69e-03 | mean 1.9e-08 (0.07) rstd 1.1e-07 (0.23) y24 9.8e-05 (0.93) y8 1.5e-01 (0.94)   NEAR ['y24', 'y8']
    fwd_m48_H128_lo4_pfeiffer_vy8             48  zp  5.6e-03 / 5.6e-03  1.59e-03 / 1.59e-03 | mean 8.0e-06 (0.97) rstd 7.8e-07 (0.46) y20 1.5e-03 (0.98) y8 1.4e-01 (0.94)   NEAR ['mean', 'y20', 'y8']
    fwd_m48_H256_bf16_parallel_y              48  zp  7.5e-03 / 7.5e-03  1.69e-03 / 1.69e-03 | mean 2.3e-08 (0.06) rstd 4.9e-08 (0.23)
    fwd_m48_H256_f32_identity_v8              48  zp  7.3e-03 / 7.3e-03  1.68e-03 / 1.68e-03 | mean 2.3e-08 (0.08) rstd 5.2e-08 (0.18) y32 9.7e-07 (0.17) y8 1.5e-01 (0.94)   NEAR ['y8']
    fwd_m48_H256_lo8_leaky_vy8                48  zp  7.7e-03 / 7.7e-03  1.61e-03 / 1.61e-03 | mean 2.1e-08 (0.02) rstd 4.7e-08 (0.00) y24 9.7e-05 (0.24) y8 1.5e-01 (0.94)   NEAR ['y8']
    fwd_m48_H256_lo4_houlsby_vy               48  v   1.6e-02 / 1.6e-02  1.68e-03 / 1.68e-03 | mean 2.3e-08 (0.07) rstd 7.0e-08 (0.32) y20 1.8e-03 (0.93)   NEAR ['y20']
    fwd_m48_H512_bf16_houlsby_gelu_v8         48  zp  7.7e-03 / 7.7e-03  1.63e-03 / 1.63e-03 | mean 1.8e-08 (0.03) rstd 5.0e-08 (0.04) y8 1.7e-01 (0.94)   NEAR ['y8']
    fwd_m48_H512_f32_compacter_vy8            48  zp  7.8e-03 / 7.8e-03  1.60e-03 / 1.60e-03 | mean 1.3e-08 (0.02) rstd 7.0e-08 (0.02) y32 4.9e-07 (0.01) y8 1.7e-01 (0.93)   NEAR ['y8']
    fwd_m48_H512_lo8_pfeiffer_vy              48  zp  7.8e-03 / 7.8e-03  1.65e-03 / 1.65e-03 | mean 1.1e-08 (0.05) rstd 1.1e-07 (0.48) y24 1.2e-04 (0.95)   NEAR ['y24']
    fwd_m48_H512_lo4_parallel_y               48  zp  9.2e-03 / 9.2e-03  1.68e-03 / 1.68e-03 | mean 3.1e-08 (0.10) rstd 6.8e-08 (0.25) y20 9.6e-04 (0.96)   NEAR ['y20']
    fwd_m48_H768_bf16_identity_vy8            48  zp  1.4e-02 / 1.4e-02  1.63e-03 / 1.63e-03 | mean 2.4e-08 (0.04) rstd 6.3e-08 (0.18) y8 1.6e-01 (0.94)   NEAR ['y8']
    fwd_m48_H768_f32_leaky_vy                 48  v   1.6e-02 / 1.6e-02  1.72e-03 / 1.72e-03 | mean 1.6e-08 (0.01) rstd 7.9e-08 (0.00) y32 7.4e-07 (0.00)
    fwd_m48_H768_lo8_houlsby_y                48  zp  1.4e-02 / 1.4e-02  1.62e-03 / 1.62e-03 | mean 2.1e-08 (0.07) rstd 6.6e-08 (0.24) y24 1.2e-04 (0.93)   NEAR ['y24']
    fwd_m48_H768_lo4_houlsby_gelu_vy8         48  v   1.7e-02 / 1.7e-02  1.71e-03 / 1.71e-03 | mean 2.0e-08 (0.05) rstd 7.1e-08 (0.05) y20 1.4e-03 (0.92) y8 1.7e-01 (0.94)   NEAR ['y20', 'y8']
    fwd_m48_H1024_bf16_compacter_vy           48  y   1.6e-02 / 1.6e-02  1.74e-03 / 1.74e-03 | mean 1.4e-08 (0.01) rstd 6.4e-08 (0.00)
    fwd_m48_H1024_f32_pfeiffer_y              48  zp  1.5e-02 / 1.5e-02  1.63e-03 / 1.63e-03 | mean 1.3e-08 (0.06) rstd 6.6e-08 (0.25) y32 5.3e-07 (0.19)
    fwd_m48_H1024_lo8_parallel_vy8            48  y   1.6e-02 / 1.6e-02  1.70e-03 / 1.70e-03 | mean 1.5e-08 (0.05) rstd 5.9e-08 (0.24) y24 1.2e-04 (0.95) y8 1.8e-01 (0.94)   NEAR ['y24', 'y8']
    fwd_m48_H1024_lo4_identity_vy8            48  zp  1.6e-02 / 1.6e-02  1.70e-03 / 1.70e-03 | mean 2.0e-08 (0.05) rstd 4.6e-08 (0.17) y20 9.7e-04 (0.98) y8 1.9e-01 (0.94)   NEAR ['y20', 'y8']
    fwd_mG1_H128_bf16_houlsby_vy            4112  v   1.6e-02 / 1.6e-02  1.68e-03 / 1.68e-03 | mean 2.5e-07 (0.42) rstd 3.4e-07 (0.27)
    fwd_mG1_H128_f32_houlsby_gelu_y         4112  y   1.6e-02 / 1.6e-02  1.67e-03 / 1.67e-03 | mean 8.1e-06 (0.87) rstd 4.5e-06 (0.23) y32 5.2e-04 (0.32)   NEAR ['mean']
    fwd_mG1_H128_lo8_compacter_vy8          4112  v   1.5e-02 / 1.5e-02  1.70e-03 / 1.70e-03 | mean 8.9e-06 (0.97) rstd 6.6e-06 (0.36) y24 2.9e-04 (0.97) y8 1.7e-01 (0.94)   NEAR ['mean', 'y24', 'y8']
    fwd_mG1_H128_lo4_pfeiffer_vy8           4112  y   1.6e-02 / 1.6e-02  1.70e-03 / 1.70e-03 | mean 1.6e-06 (0.87) rstd 3.2e-06 (0.34) y20 1.9e-03 (0.99) y8 1.7e-01 (0.94)   NEAR ['mean', 'y20', 'y8']
    fwd_mG1_H256_bf16_parallel_y            4112  y   1.6e-02 / 1.6e-02  1.66e-03 / 1.66e-03 | mean 3.5e-05 (0.99) rstd 1.1e-05 (0.29)   NEAR ['mean']
    fwd_mG1_H256_f32_identity_v8            4112  v   1.7e-02 / 1.7e-02  1.67e-03 / 1.67e-03 | mean 4.4e-06 (0.92) rstd 2.2e-07 (0.27) y32 9.1e-05 (0.25) y8 2.1e-01 (0.94)   NEAR ['mean', 'y8']
    fwd_mG1_H256_lo8_leaky_vy8              4112  v   1.7e-02 / 1.7e-02  1.67e-03 / 1.67e-03 | mean 3.7e-06 (0.83) rstd 1.2e-05 (0.04) y24 3.8e-04 (0.51) y8 1.9e-01 (0.94)   NEAR ['mean', 'y8']
    fwd_mG1_H256_lo4_houlsby_vy             4112  v   1.7e-02 / 1.7e-02  1.69e-03 / 1.69e-03 | mean 8.3e-06 (0.96) rstd 2.3e-06 (0.30) y20 1.9e-03 (0.99)   NEAR ['mean', 'y20']
    fwd_mG1_H512_bf16_houlsby_gelu_v8       4112  v   1.7e-02 / 1.7e-02  1.70e-03 / 1.70e-03 | mean 3.3e-06 (0.89) rstd 1.4e-06 (0.20) y8 1.9e-01 (0.94)   NEAR ['mean', 'y8']
    fwd_mG1_H512_f32_compacter_vy8          4112  y   1.7e-02 / 1.7e-02  1.70e-03 / 1.70e-03 | mean 6.8e-06 (0.95) rstd 6.6e-06 (0.22) y32 6.4e-04 (0.18) y8 2.2e-01 (0.94)   NEAR ['mean', 'y8']
    fwd_mG1_H512_lo8_pfeiffer_vy            4112  v   1.6e-02 / 1.6e-02  1.73e-03 / 1.73e-03 | mean 1.1e-05 (0.98) rstd 5.1e-05 (0.32) y24 1.4e-03 (0.96)   NEAR ['mean', 'y24']
    fwd_mG1_H512_lo4_parallel_y             4112  y   1.7e-02 / 1.7e-02  1.69e-03 / 1.69e-03 | mean 9.0e-07 (0.16) rstd 1.5e-07 (0.28) y20 1.9e-03 (0.99)   NEAR ['y20']
    fwd_mG1_H768_bf16_identity_vy8          4112  v   2.6e-02 / 2.6e-02  1.78e-03 / 1.77e-03 | mean 9.5e-06 (0.89) rstd 1.6e-05 (0.30) y8 2.2e-01 (0.94)   NEAR ['mean', 'y8']
    fwd_mG1_H768_f32_leaky_vy               4112  y   1.6e-02 / 1.6e-02  1.72e-03 / 1.72e-03 | mean 1.2e-06 (0.48) rstd 1.1e-06 (0.01) y32 1.0e-04 (0.07)
    fwd_mG1_H768_lo8_houlsby_y              4112  y   1.7e-02 / 1.7e-02  1.74e-03 / 1.74e-03 | mean 1.8e-05 (0.98) rstd 1.0e-05 (0.31) y24 7.6e-04 (0.96)   NEAR ['mean', 'y24']
    fwd_mG1_H768_lo4_houlsby_gelu_vy8       4112  y   1.7e-02 / 1.7e-02  1.72e-03 / 1.72e-03 | mean 2.7e-06 (0.81) rstd 1.2e-06 (0.19) y20 1.9e-03 (0.98) y8 2.1e-01 (0.94)   NEAR ['mean', 'y20', 'y8']
    fwd_mG1_H1024_bf16_compacter_vy         4112  v   1.7e-02 / 1.7e-02  1.80e-03 / 1.80e-03 | mean 5.5e-07 (0.13) rstd 1.1e-06 (0.05)
    fwd_mG1_H1024_f32_pfeiffer_y            4112  y   1.8e-02 / 1.8e-02  1.77e-03 / 1.77e-03 | mean 1.6e-05 (0.98) rstd 7.7e-06 (0.31) y32 1.2e-03 (0.21)   NEAR ['mean']
    fwd_mG1_H1024_lo8_parallel_vy8          4112  y   1.7e-02 / 1.7e-02  1.73e-03 / 1.73e-03 | mean 3.6e-07 (0.49) rstd 3.1e-07 (0.32) y24 1.2e-04 (0.97) y8 2.2e-01 (0.94)   NEAR ['y24', 'y8']
    fwd_mG1_H1024_lo4_identity_vy8          4112  y   1.8e-02 / 1.8e-02  1.77e-03 / 1.77e-03 | mean 8.3e-06 (0.96) rstd 1.9e-06 (0.30) y20 1.9e-03 (0.99) y8 2.1e-01 (0.94)   NEAR ['mean', 'y20', 'y8']
    bwd_m48_H128_plain                        48  dv  7.5e-03 / 7.5e-03  1.67e-03 / 1.67e-03 |
    bwd_m48_H256_plain                        48  dv  7.8e-03 / 7.8e-03  1.66e-03 / 1.66e-03 |
    bwd_m48_H512_plain                        48  dv  7.8e-03 / 7.8e-03  1.65e-03 / 1.65e-03 |
    bwd_m48_H768_plain                        48  dh  1.4e-02 / 1.4e-02  2.45e-03 / 2.45e-03 |
    bwd_m48_H128_bias                         48  dzp 4.1e-03 / 4.1e-03  2.29e-03 / 2.29e-03 | dbias 0.85 u (0.05) dbd 1418.28 u (0.00)
    bwd_m48_H256_bias                         48  dzp 6.5e-03 / 6.5e-03  2.27e-03 / 2.27e-03 | dbias 0.92 u (0.06) dbd 1104.59 u (0.05)
    bwd_m48_H512_bias                         48  dv  7.6e-03 / 7.6e-03  1.65e-03 / 1.65e-03 | dbias 0.84 u (0.05) dbd 780.40 u (0.00)
    bwd_m48_H768_bias                         48  dzp 1.0e-02 / 1.0e-02  2.11e-03 / 2.11e-03 | dbias 0.82 u (0.05) dbd 680.27 u (0.00)
    bwd_m48_H128_bias_tot                     48  dv  1.1e-02 / 1.1e-02  1.66e-03 / 1.66e-03 | dbias 0.73 u (0.05)
    bwd_m48_H256_bias_tot                     48  dh  3.6e-03 / 3.6e-03  2.96e-03 / 2.96e-03 | dbias 1.08 u (0.07)
    bwd_m48_H512_bias_tot                     48  dv  7.8e-03 / 7.8e-03  1.65e-03 / 1.65e-03 | dbias 0.94 u (0.06)
    bwd_m48_H768_bias_tot                     48  dh  5.6e-03 / 5.6e-03  2.76e-03 / 2.76e-03 | dbias 0.89 u (0.06)
    bwd_m48_H128_ln                           48  dv  1.1e-02 / 1.1e-02  1.64e-03 / 1.64e-03 | dgamma 1.11 u (0.07) dbeta 0.00 u (0.00)
    bwd_m48_H256_ln                           48  dv  9.1e-03 / 9.1e-03  1.65e-03 / 1.65e-03 | dgamma 0.97 u (0.06) dbeta 0.00 u (0.00)
    bwd_m48_H512_ln                           48  dv  1.4e-02 / 1.4e-02  1.66e-03 / 1.66e-03 | dgamma 1.01 u (0.06) dbeta 0.04 u (0.00)
    bwd_m48_H768_ln                           48  dh  6.3e-03 / 6.3e-03  2.72e-03 / 2.72e-03 | dgamma 1.21 u (0.08) dbeta 0.00 u (0.00)
    bwd_m48_H128_all                          48  dv  1.5e-02 / 1.5e-02  1.66e-03 / 1.66e-03 | dgamma 0.80 u (0.05) dbeta 0.00 u (0.00) dbias 0.92 u (0.06) dbd 2132.00 u (0.00)
    bwd_m48_H256_all                          48  dh  4.3e-03 / 4.3e-03  2.93e-03 / 2.93e-03 | dgamma 0.90 u (0.06) dbeta 0.00 u (0.00) dbias 0.81 u (0.05) dbd 1227.55 u (0.00)
    bwd_m48_H512_all                          48  dh  6.8e-03 / 6.8e-03  2.87e-03 / 2.87e-03 | dgamma 1.84 u (0.11) dbeta 0.19 u (0.01) dbias 0.83 u (0.05) dbd 923.48 u (0.00)
    bwd_m48_H768_all                          48  dzp 1.6e-02 / 1.6e-02  2.50e-03 / 2.48e-03 | dgamma 1.09 u (0.07) dbeta 0.12 u (0.01) dbias 0.87 u (0.05) dbd 933.53 u (0.14)
    bwd_m48_H128_g_only                       48  dv  7.7e-03 / 7.7e-03  1.62e-03 / 1.62e-03 | dgamma 0.96 u (0.06) dbd 1356.97 u (0.00)
    bwd_m48_H256_g_only                       48  dv  7.7e-03 / 7.7e-03  1.63e-03 / 1.63e-03 | dgamma 1.22 u (0.08) dbd 1259.52 u (0.00)
    bwd_m48_H512_g_only                       48  dv  7.8e-03 / 7.8e-03  1.65e-03 / 1.65e-03 | dgamma 0.95 u (0.06) dbd 781.57 u (0.00)
    bwd_m48_H768_g_only                       48  dv  7.7e-03 / 7.7e-03  1.64e-03 / 1.64e-03 | dgamma 1.08 u (0.07) dbd 582.74 u (0.00)
    bwd_m48_H128_b_only                       48  dv  7.7e-03 / 7.7e-03  1.71e-03 / 1.71e-03 | dbeta 0.00 u (0.00)
    bwd_m48_H256_b_only                       48  dh  1.5e-02 / 1.5e-02  2.38e-03 / 2.38e-03 | dbeta 0.00 u (0.00)
    bwd_m48_H512_b_only                       48  dv  7.7e-03 / 7.7e-03  1.67e-03 / 1.67e-03 | dbeta 0.11 u (0.01)
    bwd_m48_H768_b_only                       48  dv  7.8e-03 / 7.8e-03  1.65e-03 / 1.65e-03 | dbeta 0.11 u (0.01)
    bwd_m48_H128_res                          48  dzp 1.1e-02 / 1.1e-02  2.45e-03 / 2.45e-03 | dbd 1841.19 u (0.00)
    bwd_m48_H256_res                          48  dv  1.1e-02 / 1.1e-02  1.64e-03 / 1.64e-03 | dbd 857.96 u (0.00)
    bwd_m48_H512_res                          48  dh  2.7e-02 / 2.7e-02  2.35e-03 / 2.35e-03 | dbd 770.41 u (0.00)
    bwd_m48_H768_res                          48  dh  2.2e-02 / 2.2e-02  2.44e-03 / 2.44e-03 | dbd 704.54 u (0.02)
    bwd_m48_H128_res_bias                     48  dzp 8.6e-03 / 8.6e-03  2.36e-03 / 2.35e-03 | dbias 0.83 u (0.05)
    bwd_m48_H256_res_bias                     48  dv  1.5e-02 / 1.5e-02  1.68e-03 / 1.68e-03 | dbias 0.67 u (0.04)
    bwd_m48_H512_res_bias                     48  dv  1.5e-02 / 1.5e-02  1.67e-03 / 1.67e-03 | dbias 1.14 u (0.07)
    bwd_m48_H768_res_bias                     48  dh  1.2e-02 / 1.2e-02  2.94e-03 / 2.94e-03 | dbias 0.82 u (0.05)
    bwd_m48_H128_res_biastot                  48  dv  1.5e-02 / 1.5e-02  1.62e-03 / 1.62e-03 | dbias 0.52 u (0.03) dbd 1890.46 u (0.00)
    bwd_m48_H256_res_biastot                  48  dv  1.5e-02 / 1.5e-02  1.72e-03 / 1.72e-03 | dbias 1.18 u (0.07) dbd 1604.84 u (0.00)
    bwd_m48_H512_res_biastot                  48  dv  1.5e-02 / 1.5e-02  1.65e-03 / 1.65e-03 | dbias 0.72 u (0.05) dbd 1223.15 u (0.00)
    bwd_m48_H768_res_biastot                  48  dh  2.6e-02 / 2.6e-02  2.44e-03 / 2.44e-03 | dbias 0.78 u (0.05) dbd 835.20 u (0.00)
    bwd_m48_H128_res_ln                       48  dv  1.5e-02 / 1.5e-02  1.63e-03 / 1.63e-03 | dgamma 0.80 u (0.05) dbeta 0.00 u (0.00)
    bwd_m48_H256_res_ln                       48  dv  1.4e-02 / 1.4e-02  1.65e-03 / 1.65e-03 | dgamma 0.89 u (0.06) dbeta 0.12 u (0.01)
    bwd_m48_H512_res_ln                       48  dv  1.5e-02 / 1.5e-02  1.64e-03 / 1.64e-03 | dgamma 0.91 u (0.06) dbeta 0.00 u (0.00)
    bwd_m48_H768_res_ln                       48  dh  2.5e-02 / 2.5e-02  2.45e-03 / 2.45e-03 | dgamma 1.20 u (0.07) dbeta 0.26 u (0.02)
    bwd_m48_H128_res_all                      48  dv  1.2e-02 / 1.2e-02  1.62e-03 / 1.62e-03 | dgamma 0.75 u (0.05) dbeta 0.00 u (0.00) dbias 0.65 u (0.04) dbd 1878.43 u (0.00)
    bwd_m48_H256_res_all                      48  dh  2.2e-02 / 2.2e-02  2.36e-03 / 2.36e-03 | dgamma 0.92 u (0.06) dbeta 0.00 u (0.00) dbias 1.35 u (0.08) dbd 1310.64 u (0.00)
    bwd_m48_H512_res_all                      48  dv  1.4e-02 / 1.4e-02  1.65e-03 / 1.65e-03 | dgamma 1.00 u (0.06) dbeta 0.20 u (0.01) dbias 0.64 u (0.04) dbd 809.62 u (0.00)
    bwd_m48_H768_res_all                      48  dv  1.6e-02 / 1.6e-02  1.69e-03 / 1.69e-03 | dgamma 1.04 u (0.07) dbeta 0.00 u (0.00) dbias 0.90 u (0.06) dbd 618.31 u (0.00)
    bwd_m48_H128_vit                          48  dh  1.7e-02 / 1.7e-02  2.28e-03 / 2.28e-03 | dgamma 0.90 u (0.06) dbeta 0.00 u (0.00) dbias 0.61 u (0.04) dbd 2057.03 u (0.00)
    bwd_m48_H256_vit                          48  dv  1.5e-02 / 1.5e-02  1.65e-03 / 1.65e-03 | dgamma 0.78 u (0.05) dbeta 0.19 u (0.01) dbias 0.80 u (0.05) dbd 1069.73 u (0.01)
    bwd_m48_H512_vit                          48  dv  1.6e-02 / 1.6e-02  1.67e-03 / 1.67e-03 | dgamma 0.97 u (0.06) dbeta 0.10 u (0.01) dbias 0.64 u (0.04) dbd 973.42 u (0.00)
    bwd_m48_H768_vit                          48  dh  2.2e-02 / 2.2e-02  2.37e-03 / 2.37e-03 | dgamma 1.33 u (0.08) dbeta 0.12 u (0.01) dbias 1.19 u (0.07) dbd 728.09 u (0.00)
    bwd_m48_H128_res_b_only                   48  dv  1.5e-02 / 1.5e-02  1.62e-03 / 1.62e-03 | dbeta 0.09 u (0.01) dbias 0.75 u (0.05)
    bwd_m48_H256_res_b_only                   48  dh  5.3e-03 / 5.3e-03  2.80e-03 / 2.80e-03 | dbeta 0.04 u (0.00) dbias 0.83 u (0.05)
    bwd_m48_H512_res_b_only                   48  dh  1.0e-02 / 1.0e-02  2.94e-03 / 2.94e-03 | dbeta 0.11 u (0.01) dbias 0.71 u (0.04)
    bwd_m48_H768_res_b_only                   48  dzp 2.2e-02 / 2.2e-02  2.26e-03 / 2.25e-03 | dbeta 0.00 u (0.00) dbias 0.85 u (0.05)
    bwd_m48_H128_from_y                       48  dv  7.6e-03 / 7.6e-03  1.67e-03 / 1.67e-03 |
    bwd_m48_H256_from_y                       48  dv  7.8e-03 / 7.8e-03  1.69e-03 / 1.69e-03 |
    bwd_m48_H512_from_y                       48  dv  7.8e-03 / 7.8e-03  1.68e-03 / 1.68e-03 |
    bwd_m48_H768_from_y                       48  dv  7.8e-03 / 7.8e-03  1.65e-03 / 1.65e-03 |
    bwd_m48_H128_from_y_bias                  48  dv  7.6e-03 / 7.6e-03  1.58e-03 / 1.58e-03 | dbias 0.83 u (0.05) dbd 1514.03 u (0.00)
    bwd_m48_H256_from_y_bias                  48  dv  7.7e-03 / 7.7e-03  1.67e-03 / 1.67e-03 | dbias 0.70 u (0.04) dbd 1173.03 u (0.00)
    bwd_m48_H512_from_y_bias                  48  dzp 7.7e-03 / 7.7e-03  2.32e-03 / 2.31e-03 | dbias 0.86 u (0.05) dbd 1110.07 u (0.00)
    bwd_m48_H768_from_y_bias                  48  dv  7.8e-03 / 7.8e-03  1.65e-03 / 1.65e-03 | dbias 0.80 u (0.05) dbd 671.43 u (0.00)
    bwd_mG1_H128_plain                      4112  dh  1.6e-02 / 1.6e-02  2.34e-03 / 2.33e-03 |
    bwd_mG1_H256_plain                      4112  dh  1.6e-02 / 1.6e-02  2.28e-03 / 2.27e-03 |
    bwd_mG1_H512_plain                      4112  dzp 1.1e-02 / 1.1e-02  2.35e-03 / 2.33e-03 |
    bwd_mG1_H768_plain                      4112  dzp 1.4e-02 / 1.4e-02  2.45e-03 / 2.44e-03 |
    bwd_mG1_H128_bias                       4112  dzp 6.7e-03 / 6.7e-03  2.41e-03 / 2.38e-03 | dbias 0.45 u (0.03) dbd 193.21 u (0.03)
    bwd_mG1_H256_bias                       4112  dzp 1.0e-02 / 1.0e-02  2.36e-03 / 2.34e-03 | dbias 0.32 u (0.02) dbd 143.17 u (0.02)
    bwd_mG1_H512_bias                       4112  dzp 1.1e-02 / 1.1e-02  2.34e-03 / 2.33e-03 | dbias 0.51 u (0.03) dbd 88.36 u (0.01)
    bwd_mG1_H768_bias                       4112  dzp 1.4e-02 / 1.4e-02  2.37e-03 / 2.36e-03 | dbias 0.55 u (0.03) dbd 106.11 u (0.01)
    bwd_mG1_H128_bias_tot                   4112  dh  3.6e-03 / 3.6e-03  2.97e-03 / 2.97e-03 | dbias 0.44 u (0.03)
    bwd_mG1_H256_bias_tot                   4112  dzp 1.3e-02 / 1.3e-02  2.41e-03 / 2.38e-03 | dbias 0.42 u (0.03)
    bwd_mG1_H512_bias_tot                   4112  dzp 1.7e-02 / 1.7e-02  2.37e-03 / 2.36e-03 | dbias 0.65 u (0.04)
    bwd_mG1_H768_bias_tot                   4112  dzp 1.8e-02 / 1.8e-02  2.20e-03 / 2.19e-03 | dbias 0.46 u (0.03)
    bwd_mG1_H128_ln                         4112  dh  3.4e-03 / 3.4e-03  2.72e-03 / 2.70e-03 | dgamma 0.48 u (0.03) dbeta 0.13 u (0.01)
    bwd_mG1_H256_ln                         4112  dh  4.3e-03 / 4.3e-03  2.96e-03 / 2.94e-03 | dgamma 0.61 u (0.04) dbeta 0.14 u (0.01)
    bwd_mG1_H512_ln                         4112  dzp 1.6e-02 / 1.6e-02  2.24e-03 / 2.23e-03 | dgamma 0.53 u (0.03) dbeta 0.12 u (0.01)
    bwd_mG1_H768_ln                         4112  dh  7.7e-03 / 7.7e-03  2.93e-03 / 2.93e-03 | dgamma 0.64 u (0.04) dbeta 0.08 u (0.00)
    bwd_mG1_H128_all                        4112  dh  5.3e-03 / 5.3e-03  2.87e-03 / 2.85e-03 | dgamma 0.44 u (0.03) dbeta 0.12 u (0.01) dbias 0.26 u (0.02) dbd 190.94 u (0.03)
    bwd_mG1_H256_all                        4112  dzp 1.2e-02 / 1.2e-02  2.39e-03 / 2.38e-03 | dgamma 0.63 u (0.04) dbeta 0.10 u (0.01) dbias 0.53 u (0.03) dbd 167.50 u (0.01)
    bwd_mG1_H512_all                        4112  dzp 1.6e-02 / 1.6e-02  2.39e-03 / 2.38e-03 | dgamma 0.43 u (0.03) dbeta 0.14 u (0.01) dbias 0.61 u (0.04) dbd 117.97 u (0.01)
    bwd_mG1_H768_all                        4112  dzp 2.1e-02 / 2.1e-02  2.45e-03 / 2.44e-03 | dgamma 0.70 u (0.04) dbeta 0.10 u (0.01) dbias 0.56 u (0.03) dbd 92.15 u (0.01)
    bwd_mG1_H128_g_only                     4112  dzp 5.8e-03 / 5.8e-03  2.43e-03 / 2.42e-03 | dgamma 0.47 u (0.03) dbd 135.10 u (0.02)
    bwd_mG1_H256_g_only                     4112  dh  1.6e-02 / 1.6e-02  2.38e-03 / 2.37e-03 | dgamma 0.45 u (0.03) dbd 166.13 u (0.03)
    bwd_mG1_H512_g_only                     4112  dzp 1.0e-02 / 1.0e-02  2.35e-03 / 2.33e-03 | dgamma 0.51 u (0.03) dbd 75.05 u (0.01)
    bwd_mG1_H768_g_only                     4112  dh  1.6e-02 / 1.6e-02  2.48e-03 / 2.46e-03 | dgamma 0.64 u (0.04) dbd 64.30 u (0.01)
    bwd_mG1_H128_b_only                     4112  dzp 5.9e-03 / 5.9e-03  2.30e-03 / 2.28e-03 | dbeta 0.12 u (0.01)
    bwd_mG1_H256_b_only                     4112  dzp 9.3e-03 / 9.3e-03  2.29e-03 / 2.29e-03 | dbeta 0.09 u (0.01)
    bwd_mG1_H512_b_only                     4112  dzp 1.2e-02 / 1.2e-02  2.39e-03 / 2.37e-03 | dbeta 0.13 u (0.01)
    bwd_mG1_H768_b_only                     4112  dzp 1.5e-02 / 1.5e-02  2.25e-03 / 2.24e-03 | dbeta 0.09 u (0.01)
    bwd_mG1_H128_res                        4112  dh  3.0e-02 / 3.0e-02  2.42e-03 / 2.40e-03 | dbd 122.51 u (0.02)
    bwd_mG1_H256_res                        4112  dh  3.1e-02 / 3.1e-02  2.32e-03 / 2.32e-03 | dbd 144.76 u (0.01)
    bwd_mG1_H512_res                        4112  dzp 2.3e-02 / 2.3e-02  2.24e-03 / 2.23e-03 | dbd 92.03 u (0.02)
    bwd_mG1_H768_res                        4112  dzp 2.4e-02 / 2.4e-02  2.41e-03 / 2.38e-03 | dbd 67.35 u (0.00)
    bwd_mG1_H128_res_bias                   4112  dh  6.9e-03 / 6.9e-03  3.01e-03 / 2.99e-03 | dbias 0.40 u (0.02)
    bwd_mG1_H256_res_bias                   4112  dh  1.0e-02 / 1.0e-02  3.03e-03 / 3.01e-03 | dbias 0.31 u (0.02)
    bwd_mG1_H512_res_bias                   4112  dh  1.4e-02 / 1.4e-02  2.87e-03 / 2.85e-03 | dbias 0.39 u (0.02)
    bwd_mG1_H768_res_bias                   4112  dh  1.6e-02 / 1.6e-02  2.76e-03 / 2.74e-03 | dbias 0.51 u (0.03)
    bwd_mG1_H128_res_biastot                4112  dzp 1.0e-02 / 1.0e-02  2.45e-03 / 2.44e-03 | dbias 0.39 u (0.02) dbd 301.52 u (0.01)
    bwd_mG1_H256_res_biastot                4112  dzp 1.8e-02 / 1.8e-02  2.33e-03 / 2.33e-03 | dbias 0.47 u (0.03) dbd 178.85 u (0.01)
    bwd_mG1_H512_res_biastot                4112  dzp 2.1e-02 / 2.1e-02  2.51e-03 / 2.50e-03 | dbias 0.60 u (0.04) dbd 113.60 u (0.01)
    bwd_mG1_H768_res_biastot                4112  dzp 2.3e-02 / 2.3e-02  2.39e-03 / 2.38e-03 | dbias 0.49 u (0.03) dbd 111.45 u (0.01)
    bwd_mG1_H128_res_ln                     4112  dh  2.9e-02 / 2.9e-02  2.38e-03 / 2.38e-03 | dgamma 0.75 u (0.05) dbeta 0.08 u (0.00)
    bwd_mG1_H256_res_ln                     4112  dzp 1.7e-02 / 1.7e-02  2.17e-03 / 2.16e-03 | dgamma 0.51 u (0.03) dbeta 0.09 u (0.01)
    bwd_mG1_H512_res_ln                     4112  dzp 2.1e-02 / 2.1e-02  2.25e-03 / 2.25e-03 | dgamma 0.62 u (0.04) dbeta 0.09 u (0.01)
    bwd_mG1_H768_res_ln                     4112  dzp 3.0e-02 / 3.0e-02  2.37e-03 / 2.36e-03 | dgamma 1.06 u (0.07) dbeta 0.13 u (0.01)
    bwd_mG1_H128_res_all                    4112  dzp 1.1e-02 / 1.1e-02  2.33e-03 / 2.32e-03 | dgamma 0.57 u (0.04) dbeta 0.09 u (0.01) dbias 0.41 u (0.03) dbd 204.12 u (0.02)
    bwd_mG1_H256_res_all                    4112  dzp 1.5e-02 / 1.5e-02  2.23e-03 / 2.23e-03 | dgamma 0.69 u (0.04) dbeta 0.07 u (0.00) dbias 0.56 u (0.04) dbd 118.81 u (0.01)
    bwd_mG1_H512_res_all                    4112  dzp 2.2e-02 / 2.2e-02  2.47e-03 / 2.46e-03 | dgamma 0.72 u (0.05) dbeta 0.15 u (0.01) dbias 0.60 u (0.04) dbd 87.64 u (0.01)
    bwd_mG1_H768_res_all                    4112  dzp 2.3e-02 / 2.3e-02  2.28e-03 / 2.27e-03 | dgamma 0.62 u (0.04) dbeta 0.14 u (0.01) dbias 0.47 u (0.03) dbd 67.37 u (0.00)
    bwd_mG1_H128_vit                        4112  dzp 1.0e-02 / 1.0e-02  2.16e-03 / 2.16e-03 | dgamma 0.57 u (0.04) dbeta 0.09 u (0.01) dbias 0.42 u (0.03) dbd 174.33 u (0.04)
    bwd_mG1_H256_vit                        4112  dzp 1.6e-02 / 1.6e-02  2.43e-03 / 2.42e-03 | dgamma 0.51 u (0.03) dbeta 0.08 u (0.00) dbias 0.34 u (0.02) dbd 189.04 u (0.02)
    bwd_mG1_H512_vit                        4112  dh  3.0e-02 / 3.0e-02  2.36e-03 / 2.35e-03 | dgamma 0.50 u (0.03) dbeta 0.10 u (0.01) dbias 0.40 u (0.03) dbd 92.90 u (0.01)
    bwd_mG1_H768_vit                        4112  dh  3.1e-02 / 3.1e-02  2.42e-03 / 2.42e-03 | dgamma 0.60 u (0.04) dbeta 0.10 u (0.01) dbias 0.57 u (0.04) dbd 99.09 u (0.00)
    bwd_mG1_H128_res_b_only                 4112  dh  6.9e-03 / 6.9e-03  2.89e-03 / 2.87e-03 | dbeta 0.08 u (0.00) dbias 0.51 u (0.03)
    bwd_mG1_H256_res_b_only                 4112  dh  1.2e-02 / 1.2e-02  2.91e-03 / 2.91e-03 | dbeta 0.08 u (0.00) dbias 0.29 u (0.02)
    bwd_mG1_H512_res_b_only                 4112  dh  1.4e-02 / 1.4e-02  2.93e-03 / 2.92e-03 | dbeta 0.08 u (0.00) dbias 0.32 u (0.02)
    bwd_mG1_H768_res_b_only                 4112  dh  1.5e-02 / 1.5e-02  2.87e-03 / 2.85e-03 | dbeta 0.11 u (0.01) dbias 0.40 u (0.02)
    bwd_mG1_H128_from_y                     4112  dh  1.5e-02 / 1.5e-02  2.33e-03 / 2.32e-03 |
    bwd_mG1_H256_from_y                     4112  dzp 1.0e-02 / 1.0e-02  2.32e-03 / 2.29e-03 |
    bwd_mG1_H512_from_y                     4112  dzp 1.1e-02 / 1.1e-02  2.31e-03 / 2.29e-03 |
    bwd_mG1_H768_from_y                     4112  dzp 1.4e-02 / 1.4e-02  2.22e-03 / 2.21e-03 |
    bwd_mG1_H128_from_y_bias                4112  dzp 6.1e-03 / 6.1e-03  2.25e-03 / 2.24e-03 | dbias 0.59 u (0.04) dbd 147.88 u (0.02)
    bwd_mG1_H256_from_y_bias                4112  dzp 8.3e-03 / 8.3e-03  2.40e-03 / 2.40e-03 | dbias 0.42 u (0.03) dbd 114.26 u (0.02)
    bwd_mG1_H512_from_y_bias                4112  dzp 1.6e-02 / 1.6e-02  2.35e-03 / 2.34e-03 | dbias 0.51 u (0.03) dbd 110.90 u (0.01)
    bwd_mG1_H768_from_y_bias                4112  dzp 1.3e-02 / 1.3e-02  2.37e-03 / 2.34e-03 | dbias 0.48 u (0.03) dbd 99.64 u (0.01)
    walk_fwd_H256_bf16_1                      16  zp  7.2e-03 / 7.2e-03  1.67e-03 / 1.67e-03 | mean 1.3e-08 (0.04) rstd 5.3e-08 (0.25)
    walk_fwd_H256_bf16_2                      32  zp  7.6e-03 / 7.6e-03  1.71e-03 / 1.71e-03 | mean 2.0e-08 (0.07) rstd 5.8e-08 (0.24)
    walk_fwd_H256_bf16_3                      48  zp  7.7e-03 / 7.7e-03  1.72e-03 / 1.72e-03 | mean 4.2e-08 (0.13) rstd 7.6e-08 (0.30)
    walk_fwd_H256_bf16_G-1                  4080  v   1.7e-02 / 1.7e-02  1.69e-03 / 1.69e-03 | mean 5.2e-05 (0.97) rstd 1.5e-05 (0.29)   NEAR ['mean']
    walk_fwd_H256_bf16_G                    4096  v   1.7e-02 / 1.7e-02  1.66e-03 / 1.66e-03 | mean 1.0e-05 (0.97) rstd 3.3e-06 (0.30)   NEAR ['mean']
    walk_fwd_H256_bf16_G+1                  4112  y   1.6e-02 / 1.6e-02  1.65e-03 / 1.65e-03 | mean 5.2e-06 (0.94) rstd 2.5e-06 (0.31)   NEAR ['mean']
    walk_fwd_H256_bf16_2G                   8192  v   1.7e-02 / 1.7e-02  1.67e-03 / 1.67e-03 | mean 9.5e-06 (0.97) rstd 2.0e-06 (0.29)   NEAR ['mean']
    walk_fwd_H256_bf16_2G+1                 8208  v   1.7e-02 / 1.7e-02  1.65e-03 / 1.65e-03 | mean 1.6e-05 (0.98) rstd 3.4e-06 (0.29)   NEAR ['mean']
    walk_fwd_H256_bf16_3G+1                12304  y   1.6e-02 / 1.6e-02  1.66e-03 / 1.66e-03 | mean 1.3e-05 (0.98) rstd 1.6e-06 (0.28)   NEAR ['mean']
    walk_fwd_H256_lo4_1                       16  zp  6.8e-03 / 6.8e-03  1.59e-03 / 1.59e-03 | mean 1.7e-08 (0.05) rstd 5.7e-08 (0.29) y20 9.1e-04 (0.97)   NEAR ['y20']
    walk_fwd_H256_lo4_2                       32  v   1.5e-02 / 1.5e-02  1.70e-03 / 1.70e-03 | mean 1.9e-08 (0.04) rstd 5.8e-08 (0.22) y20 9.7e-04 (0.95)   NEAR ['y20']
    walk_fwd_H256_lo4_3                       48  zp  7.0e-03 / 7.0e-03  1.66e-03 / 1.66e-03 | mean 2.2e-08 (0.06) rstd 4.6e-08 (0.24) y20 9.8e-04 (0.99)   NEAR ['y20']
    walk_fwd_H256_lo4_G-1                   4080  y   1.6e-02 / 1.6e-02  1.68e-03 / 1.68e-03 | mean 1.8e-05 (0.98) rstd 8.6e-06 (0.30) y20 1.9e-03 (0.99)   NEAR ['mean', 'y20']
    walk_fwd_H256_lo4_G                     4096  y   1.6e-02 / 1.6e-02  1.64e-03 / 1.64e-03 | mean 6.7e-06 (0.95) rstd 3.2e-06 (0.29) y20 1.9e-03 (0.99)   NEAR ['mean', 'y20']
    walk_fwd_H256_lo4_G+1                   4112  y   1.6e-02 / 1.6e-02  1.69e-03 / 1.69e-03 | mean 6.5e-08 (0.17) rstd 8.5e-08 (0.30) y20 1.7e-03 (0.99)   NEAR ['y20']
    walk_fwd_H256_lo4_2G                    8192  v   1.7e-02 / 1.7e-02  1.64e-03 / 1.64e-03 | mean 1.6e-05 (0.98) rstd 1.4e-05 (0.31) y20 2.0e-03 (0.99)   NEAR ['mean', 'y20']
    walk_fwd_H256_lo4_2G+1                  8208  y   1.6e-02 / 1.6e-02  1.67e-03 / 1.67e-03 | mean 7.4e-06 (0.96) rstd 5.8e-06 (0.30) y20 1.9e-03 (0.99)   NEAR ['mean', 'y20']
    walk_fwd_H256_lo4_3G+1                 12304  y   1.6e-02 / 1.6e-02  1.70e-03 / 1.69e-03 | mean 2.4e-05 (0.94) rstd 6.5e-06 (0.27) y20 1.9e-03 (0.99)   NEAR ['mean', 'y20']
    walk_fwd_H768_bf16_1                      16  v   1.6e-02 / 1.6e-02  1.70e-03 / 1.70e-03 | mean 1.1e-08 (0.04) rstd 5.1e-08 (0.21)
    walk_fwd_H768_bf16_2                      32  zp  1.1e-02 / 1.1e-02  1.51e-03 / 1.51e-03 | mean 2.3e-08 (0.07) rstd 8.1e-08 (0.39)
    walk_fwd_H768_bf16_3                      48  v   1.6e-02 / 1.6e-02  1.70e-03 / 1.70e-03 | mean 1.6e-08 (0.05) rstd 6.7e-08 (0.25)
    walk_fwd_H768_bf16_G-1                  4080  y   1.7e-02 / 1.7e-02  1.71e-03 / 1.71e-03 | mean 1.3e-06 (0.80) rstd 1.7e-06 (0.32)   NEAR ['mean']
    walk_fwd_H768_bf16_G                    4096  y   1.7e-02 / 1.7e-02  1.71e-03 / 1.71e-03 | mean 3.5e-08 (0.10) rstd 1.1e-07 (0.33)
    walk_fwd_H768_bf16_G+1                  4112  v   1.9e-02 / 1.9e-02  1.76e-03 / 1.76e-03 | mean 6.3e-06 (0.95) rstd 5.3e-06 (0.29)   NEAR ['mean']
    walk_fwd_H768_bf16_2G                   8192  y   1.7e-02 / 1.7e-02  1.72e-03 / 1.72e-03 | mean 2.5e-06 (0.89) rstd 1.3e-05 (0.33)   NEAR ['mean']
    walk_fwd_H768_bf16_2G+1                 8208  y   1.7e-02 / 1.7e-02  1.72e-03 / 1.72e-03 | mean 1.2e-05 (0.98) rstd 8.3e-06 (0.33)   NEAR ['mean']
    walk_fwd_H768_bf16_3G+1                12304  y   1.7e-02 / 1.7e-02  1.72e-03 / 1.72e-03 | mean 1.8e-05 (0.98) rstd 3.1e-05 (0.35)   NEAR ['mean']
    walk_fwd_H768_lo4_1                       16  y   1.5e-02 / 1.5e-02  1.72e-03 / 1.72e-03 | mean 9.3e-09 (0.03) rstd 7.4e-08 (0.40) y20 1.0e-03 (0.92)   NEAR ['y20']
    walk_fwd_H768_lo4_2                       32  v   1.6e-02 / 1.6e-02  1.72e-03 / 1.72e-03 | mean 1.4e-08 (0.04) rstd 6.8e-08 (0.26) y20 9.6e-04 (0.98)   NEAR ['y20']
    walk_fwd_H768_lo4_3                       48  y   1.4e-02 / 1.4e-02  1.74e-03 / 1.74e-03 | mean 1.3e-08 (0.04) rstd 7.8e-08 (0.43) y20 9.7e-04 (0.96)   NEAR ['y20']
    walk_fwd_H768_lo4_G-1                   4080  y   1.7e-02 / 1.7e-02  1.68e-03 / 1.68e-03 | mean 9.9e-06 (0.97) rstd 2.5e-05 (0.30) y20 1.9e-03 (0.99)   NEAR ['mean', 'y20']
    walk_fwd_H768_lo4_G                     4096  y   1.7e-02 / 1.7e-02  1.70e-03 / 1.70e-03 | mean 2.0e-06 (0.87) rstd 9.8e-07 (0.33) y20 1.9e-03 (0.99)   NEAR ['mean', 'y20']
    walk_fwd_H768_lo4_G+1                   4112  v   1.8e-02 / 1.8e-02  1.70e-03 / 1.70e-03 | mean 4.0e-06 (0.85) rstd 2.2e-06 (0.34) y20 1.9e-03 (0.99)   NEAR ['mean', 'y20']
    walk_fwd_H768_lo4_2G                    8192  v   1.8e-02 / 1.8e-02  1.70e-03 / 1.70e-03 | mean 9.1e-06 (0.97) rstd 1.8e-05 (0.35) y20 1.9e-03 (0.99)   NEAR ['mean', 'y20']
    walk_fwd_H768_lo4_2G+1                  8208  y   1.7e-02 / 1.7e-02  1.69e-03 / 1.69e-03 | mean 2.9e-05 (0.99) rstd 1.3e-05 (0.32) y20 1.9e-03 (0.99)   NEAR ['mean', 'y20']
    walk_fwd_H768_lo4_3G+1                 12304  y   1.7e-02 / 1.7e-02  1.71e-03 / 1.71e-03 | mean 1.1e-05 (0.97) rstd 1.0e-05 (0.31) y20 2.0e-03 (0.99)   NEAR ['mean', 'y20']
    walk_bwd_H256_vit_1                       16  dv  1.4e-02 / 1.4e-02  1.66e-03 / 1.66e-03 | dgamma 1.77 u (0.11) dbeta 0.00 u (0.00) dbias 1.11 u (0.07) dbd 2381.17 u (0.00)
    walk_bwd_H256_vit_2                       32  dv  1.4e-02 / 1.4e-02  1.65e-03 / 1.65e-03 | dgamma 1.11 u (0.07) dbeta 0.00 u (0.00) dbias 1.09 u (0.07) dbd 1928.38 u (0.00)
    walk_bwd_H256_vit_3                       48  dv  1.4e-02 / 1.4e-02  1.66e-03 / 1.66e-03 | dgamma 0.86 u (0.05) dbeta 0.00 u (0.00) dbias 0.80 u (0.05) dbd 1393.30 u (0.03)
    walk_bwd_H256_vit_G-1                   4080  dzp 1.5e-02 / 1.5e-02  2.40e-03 / 2.39e-03 | dgamma 0.47 u (0.03) dbeta 0.09 u (0.01) dbias 0.45 u (0.03) dbd 145.57 u (0.01)
    walk_bwd_H256_vit_G                     4096  dzp 1.4e-02 / 1.4e-02  2.38e-03 / 2.37e-03 | dgamma 0.41 u (0.03) dbeta 0.12 u (0.01) dbias 0.37 u (0.02) dbd 160.59 u (0.01)
    walk_bwd_H256_vit_G+1                   4112  dh  3.1e-02 / 3.1e-02  2.45e-03 / 2.44e-03 | dgamma 0.62 u (0.04) dbeta 0.08 u (0.01) dbias 0.47 u (0.03) dbd 134.01 u (0.01)
    walk_bwd_H256_vit_2G                    8192  dh  3.1e-02 / 3.1e-02  2.37e-03 / 2.37e-03 | dgamma 0.43 u (0.03) dbeta 0.08 u (0.01) dbias 0.30 u (0.02) dbd 104.93 u (0.00)
    walk_bwd_H256_vit_2G+1                  8208  dzp 1.5e-02 / 1.5e-02  2.45e-03 / 2.44e-03 | dgamma 0.41 u (0.03) dbeta 0.12 u (0.01) dbias 0.30 u (0.02) dbd 94.61 u (0.01)
    walk_bwd_H256_vit_3G+1                 12304  dzp 1.7e-02 / 1.7e-02  2.45e-03 / 2.43e-03 | dgamma 0.33 u (0.02) dbeta 0.09 u (0.01) dbias 0.31 u (0.02) dbd 90.21 u (0.00)
    walk_bwd_H768_vit_1                       16  dh  2.4e-02 / 2.4e-02  2.39e-03 / 2.39e-03 | dgamma 1.53 u (0.10) dbeta 0.00 u (0.00) dbias 1.60 u (0.10) dbd 1114.54 u (0.00)
    walk_bwd_H768_vit_2                       32  dv  1.3e-02 / 1.3e-02  1.66e-03 / 1.66e-03 | dgamma 1.63 u (0.10) dbeta 0.00 u (0.00) dbias 0.96 u (0.06) dbd 1301.91 u (0.00)
    walk_bwd_H768_vit_3                       48  dh  2.9e-02 / 2.9e-02  2.43e-03 / 2.43e-03 | dgamma 1.55 u (0.10) dbeta 0.05 u (0.00) dbias 1.11 u (0.07) dbd 583.45 u (0.00)
    walk_bwd_H768_vit_G-1                   4080  dzp 2.3e-02 / 2.3e-02  2.43e-03 / 2.42e-03 | dgamma 0.56 u (0.04) dbeta 0.09 u (0.01) dbias 0.64 u (0.04) dbd 86.23 u (0.01)
    walk_bwd_H768_vit_G                     4096  dzp 2.3e-02 / 2.3e-02  2.43e-03 / 2.41e-03 | dgamma 0.76 u (0.05) dbeta 0.09 u (0.01) dbias 0.51 u (0.03) dbd 68.87 u (0.01)
    walk_bwd_H768_vit_G+1                   4112  dzp 3.1e-02 / 3.1e-02  2.24e-03 / 2.23e-03 | dgamma 0.58 u (0.04) dbeta 0.12 u (0.01) dbias 0.53 u (0.03) dbd 68.97 u (0.01)
    walk_bwd_H768_vit_2G                    8192  dzp 2.6e-02 / 2.6e-02  2.48e-03 / 2.46e-03 | dgamma 0.43 u (0.03) dbeta 0.14 u (0.01) dbias 0.35 u (0.02) dbd 47.51 u (0.01)
    walk_bwd_H768_vit_2G+1                  8208  dh  3.2e-02 / 3.2e-02  2.39e-03 / 2.39e-03 | dgamma 0.39 u (0.02) dbeta 0.11 u (0.01) dbias 0.49 u (0.03) dbd 54.53 u (0.01)
    walk_bwd_H768_vit_3G+1                 12304  dzp 2.5e-02 / 2.5e-02  2.26e-03 / 2.25e-03 | dgamma 0.49 u (0.03) dbeta 0.08 u (0.00) dbias 0.30 u (0.02) dbd 41.29 u (0.00)
    walk_bwd_H768_bias_1                      16  dh  1.4e-02 / 1.4e-02  2.44e-03 / 2.44e-03 | dbias 1.27 u (0.08) dbd 1253.78 u (0.00)
    walk_bwd_H768_bias_2                      32  dzp 8.1e-03 / 8.1e-03  2.45e-03 / 2.45e-03 | dbias 1.34 u (0.08) dbd 920.36 u (0.00)
    walk_bwd_H768_bias_3                      48  dh  1.5e-02 / 1.5e-02  2.39e-03 / 2.39e-03 | dbias 1.29 u (0.08) dbd 636.47 u (0.00)
    walk_bwd_H768_bias_G-1                  4080  dzp 1.5e-02 / 1.5e-02  2.42e-03 / 2.39e-03 | dbias 0.49 u (0.03) dbd 99.44 u (0.01)
    walk_bwd_H768_bias_G                    4096  dzp 1.4e-02 / 1.4e-02  2.34e-03 / 2.31e-03 | dbias 0.44 u (0.03) dbd 80.71 u (0.01)
    walk_bwd_H768_bias_G+1                  4112  dzp 1.3e-02 / 1.3e-02  2.30e-03 / 2.28e-03 | dbias 0.51 u (0.03) dbd 75.85 u (0.01)
    walk_bwd_H768_bias_2G                   8192  dzp 1.8e-02 / 1.8e-02  2.39e-03 / 2.38e-03 | dbias 0.31 u (0.02) dbd 77.61 u (0.01)
    walk_bwd_H768_bias_2G+1                 8208  dzp 1.5e-02 / 1.5e-02  2.37e-03 / 2.36e-03 | dbias 0.36 u (0.02) dbd 71.11 u (0.01)
    walk_bwd_H768_bias_3G+1                12304  dzp 1.4e-02 / 1.4e-02  2.26e-03 / 2.26e-03 | dbias 0.29 u (0.02) dbd 40.00 u (0.00)
    fwd_tight_H256                            48  zp  7.6e-03 / 7.6e-03  1.67e-03 / 1.67e-03 | mean 2.4e-08 (0.08) rstd 5.9e-08 (0.31)
    bwd_tight_H256                            48  dzp 9.2e-03 / 9.2e-03  2.37e-03 / 2.37e-03 | dgamma 0.75 u (0.05) dbeta 0.03 u (0.00) dbias 0.56 u (0.04) dbd 1158.19 u (0.02)
    fwd_shared_H512                           80  v   1.8e-02 / 1.8e-02  1.68e-03 / 1.68e-03 | mean 1.6e-06 (0.85) rstd 2.1e-06 (0.29)   NEAR ['mean']
    fwd_offset_H768                           80  y   1.6e-02 / 1.6e-02  1.76e-03 / 1.76e-03 | mean 3.2e-06 (0.24) rstd 2.1e-07 (0.51) y32 5.0e-06 (0.21)
    fwd_mG1_H768_lo4_houlsby_gelu_vy8       4112  y   1.7e-02 / 1.7e-02  1.72e-03 / 1.72e-03 | mean 2.7e-06 (0.81) rstd 1.2e-06 (0.19) y20 1.9e-03 (0.98) y8 2.1e-01 (0.94)   NEAR ['mean', 'y20', 'y8']
    bwd_mG1_H768_vit                        4112  dh  3.1e-02 / 3.1e-02  2.42e-03 / 2.42e-03 | dgamma 0.60 u (0.04) dbeta 0.10 u (0.01) dbias 0.57 u (0.04) dbd 99.07 u (0.00)
    bwd_m48_H128_from_y_bias                  48  dv  7.6e-03 / 7.6e-03  1.58e-03 / 1.58e-03 | dbias 0.83 u (0.05) dbd 1514.03 u (0.00)
"""
import functools

import pytest
import torch

import adapter_ln_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
WALK_TILES = ('1', '2', '3', 'G-1', 'G', 'G+1', '2G', '2G+1', '3G+1')


@functools.lru_cache(maxsize=None)
def grid():
    return max(8, torch.cuda.get_device_properties(0).multi_processor_count & ~7)


def tiles(sym):
    G = grid()
    return {'1': 1, '2': 2, '3': 3, 'G-1': G - 1, 'G': G, 'G+1': G + 1, '2G': 2 * G, '2G+1': 2 * G + 1, '3G+1': 3 * G + 1}[sym]


@functools.lru_cache(maxsize=None)
def sweep():
    return {s['name']: s for s in R.sweep_specs(grid())}


def check(c, frag=None):
    from adapter4rec_amd import _lib as L
    got = R.run(c, L, frag=frag)
    figures, fails = R.judge(c, got, c.ref, c.fig)
    near = R.near_bound(figures)
    print('KERNEL ' + R.table_row(c, figures) + (f'   NEAR {near}' if near else ''))
    assert not fails, (c.name, fails)


# ------------------------------------------------------------------ form sweep
@pytest.mark.parametrize('name', R.names('fwd_m'))
def test_forward_forms(name):
    check(R.build(sweep()[name], DEV))


@pytest.mark.parametrize('name', R.names('bwd_m'))
def test_backward_forms(name):
    check(R.build(sweep()[name], DEV))


# ------------------------------------------------------------------ launch walk
@pytest.mark.parametrize('nt', WALK_TILES)
@pytest.mark.parametrize('res', ['bf16', 'lo4'])
@pytest.mark.parametrize('H', [256, 768])
def test_forward_launch_walk(H, res, nt):
    """min(M / 16, G) persistent workgroups, rows requested one tile ahead, the last tile re-requesting itself: one tile in the whole launch, fewer tiles
    than workgroups, exactly one / two / three / four tiles for some workgroup.  Every row has its own random data and the bound is per 16-row tile:
    a tile computed from another tile's rows misses it (the stale-tile mutation of the CPU file)."""
    M = 16 * tiles(nt)
    check(R.build(dict(name=f'walk_fwd_H{H}_{res}_{nt}', H=H, M=M, dirn='fwd', mode='houlsby', res=res, out='vy', G=grid()), DEV))


@pytest.mark.parametrize('nt', WALK_TILES)
@pytest.mark.parametrize('H,form', [(256, 'vit'), (768, 'vit'), (768, 'bias')])
def test_backward_launch_walk(H, form, nt):
    """the image tower's form (dres, bias_total, all sums): H = 256 requests two tiles ahead (cur <- nxt <- nn), H = 768 one (cur <- nn); H = 768 without
    dres and dgamma: two again.  The column sums cross every workgroup's tiles and the atomics of up to G workgroups."""
    M = 16 * tiles(nt)
    check(R.build(dict(R.bwd_spec(form, H, M, drop=0.0), name=f'walk_bwd_H{H}_{form}_{nt}', G=grid()), DEV))


# ------------------------------------------------------------------ strides, offset rows
@pytest.mark.parametrize('name', ['fwd_tight_H256', 'bwd_tight_H256', 'fwd_shared_H512', 'fwd_offset_H768'])
def test_strides_and_offset_rows(name):
    """ld == H in both directions; A and the other residual as column slices of one [rows, 2 H + 16] buffer; rows of mean 30 and unit variance, where
    only stats and y32 carry the tight fp32 bound."""
    check(R.build(R.CASES[name], DEV))


# ------------------------------------------------------------------ fragment-ordered weights
def _fragments(c):
    """Wd, Wu, Wu^T, Wd^T of the case in fragment order, from a4r_pack_matrices (layout 1 for the [64, H] matrices, 2 for the [H, 64] ones)"""
    from adapter4rec_amd import _lib as L
    H, t = c.H, torch.bfloat16
    flat = torch.cat([c.Wd.float().reshape(-1), c.Wu.float().reshape(-1)])
    mk = lambda r, k: torch.zeros(r, k, dtype=t, device=DEV)
    f_wd, f_wu, f_wuT, f_wdT = mk(64, H), mk(H, 64), mk(64, H), mk(H, 64)
    ents = [(0, f_wd, 64, H, 2), (64 * H, f_wu, H, 64, 4), (64 * H, f_wuT, H, 64, 2 | 1), (0, f_wdT, 64, H, 4 | 1)]
    arr = (L.PackDesc * len(ents))()
    for i, (off, dst, rows, cols, code) in enumerate(ents):
        arr[i] = L.PackDesc(off, dst.data_ptr(), rows, cols, dst.shape[0], dst.shape[1], code, 0)
    tab = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
    L.pack_matrices(flat, tab, len(ents), 64 * H, L.BF16)
    torch.cuda.synchronize()
    assert sorted(f_wd.view(-1).tolist()) == sorted(c.Wd.view(-1).tolist()) and not torch.equal(f_wd, c.Wd)
    return (f_wd, f_wu), (f_wuT, f_wdT)


@pytest.mark.parametrize('name', ['fwd_mG1_H768_lo4_houlsby_gelu_vy8', 'bwd_mG1_H768_vit', 'bwd_m48_H128_from_y_bias'])
def test_fragment_ordered_weights(name):
    """frag=: the same case through the fragment-ordered copies passes judge and is bit-equal to the row-major launch"""
    from adapter4rec_amd import _lib as L
    c = R.build(sweep()[name], DEV)
    frag = _fragments(c)[0 if c.dirn == 'fwd' else 1]
    check(c, frag=frag)
    a, b = R.run(c, L, raw=True), R.run(c, L, frag=frag, raw=True)
    for k in a:
        assert torch.equal(a[k], b[k]), f'{name}: {k} differs between the row-major and the fragment-ordered launch'
