"""The attention kernels (a4r_attn_fwd / _bwd, a4r_attn_long_fwd / _bwd) against the fp64 reference of tests/attn_ref.py at their shape and launch
edges, on the cases tests/test_attn_ref_cpu.py proves sound: qkv with gap columns and the block order v, q, k, out / dout wider than the heads,
every output buffer pre-filled with a sentinel that must survive outside the rows and columns a kernel owns.  Bounds: attn_ref.judge (fp32: 1e-4
forward, 2e-4 gradients, 1e-3 lse; bf16: the elementwise bounds of tests/test_kernels_gpu.py and the relative RMS error per (item, head) and per
16-row block of one, at most twice the bf16 model's).

Measured maximum errors against the fp64 reference on an MI355X ("kernel"; grad = the worst of dQ, dK, dV), next to the error of the same formula
evaluated in fp32 on the CPU ("fp32 CPU", printed by tests/test_attn_ref_cpu.py) and, for bf16 cases, the worst (item, head) relative RMS error of
the kernel and of the bf16 model (bound: twice the model's; the per-16-row-block figures are printed by both files).  No case exceeded a bound.
(nan: the reference of dQ / dK is all zero at S = 1, so there is no relative figure.)

    case                            kernel out  grad     lse     | fp32 CPU out  grad    | bf16 RMS kernel / model: out        grad
    short_f32_dh8_S1                0.0e+00     0.0e+00  -       | 0.0e+00       0.0e+00 |
    short_f32_dh8_S2                2.2e-07     2.1e-07  -       | 2.2e-07       2.3e-07 |
    short_f32_dh8_S15               2.5e-07     5.2e-07  -       | 4.2e-07       5.2e-07 |
    short_f32_dh8_S16               3.8e-07     8.2e-07  -       | 6.2e-07       8.2e-07 |
    short_f32_dh8_S17               2.4e-07     7.8e-07  -       | 5.2e-07       7.8e-07 |
    short_f32_dh8_S31               6.1e-07     3.4e-06  -       | 5.2e-07       3.4e-06 |
    short_f32_dh8_S32               3.3e-07     1.1e-06  -       | 4.1e-07       1.1e-06 |
    short_bf16_dh8_S1               0.0e+00     0.0e+00  -       | 0.0e+00       0.0e+00 | 0.00e+00 / 0.00e+00   nan / nan
    short_bf16_dh8_S2               5.2e-03     1.6e-02  -       | 2.7e-07       3.2e-07 | 1.85e-03 / 1.85e-03   3.08e-03 / 3.08e-03
    short_bf16_dh8_S15              3.9e-03     1.2e-02  -       | 3.7e-07       5.0e-07 | 1.77e-03 / 1.77e-03   2.06e-03 / 2.06e-03
    short_bf16_dh8_S16              7.6e-03     1.2e-02  -       | 2.9e-07       8.3e-07 | 1.93e-03 / 1.93e-03   2.07e-03 / 2.07e-03
    short_bf16_dh8_S17              3.8e-03     1.4e-02  -       | 4.2e-07       4.5e-07 | 1.82e-03 / 1.82e-03   2.28e-03 / 2.28e-03
    short_bf16_dh8_S31              1.0e-02     2.3e-02  -       | 3.2e-07       1.3e-06 | 2.15e-03 / 2.15e-03   2.17e-03 / 2.17e-03
    short_bf16_dh8_S32              3.8e-03     3.1e-02  -       | 4.4e-07       4.8e-07 | 1.87e-03 / 1.87e-03   2.56e-03 / 2.56e-03
    short_f32_dh16_S1               1.6e-07     1.6e-07  -       | 1.6e-07       1.6e-07 |
    short_f32_dh16_S2               2.0e-07     2.1e-07  -       | 2.3e-07       1.7e-07 |
    short_f32_dh16_S15              4.5e-07     8.2e-07  -       | 4.9e-07       6.3e-07 |
    short_f32_dh16_S16              4.6e-07     9.7e-07  -       | 6.8e-07       9.7e-07 |
    short_f32_dh16_S17              5.1e-07     1.0e-06  -       | 9.9e-07       1.1e-06 |
    short_f32_dh16_S31              7.1e-07     8.5e-07  -       | 5.9e-07       1.1e-06 |
    short_f32_dh16_S32              4.2e-07     8.3e-07  -       | 4.7e-07       1.1e-06 |
    short_bf16_dh16_S1              1.0e-02     5.2e-03  -       | 3.2e-07       1.6e-07 | 1.96e-03 / 1.96e-03   nan / nan
    short_bf16_dh16_S2              3.9e-03     7.8e-03  -       | 1.3e-07       1.8e-07 | 1.87e-03 / 1.87e-03   2.63e-03 / 2.63e-03
    short_bf16_dh16_S15             5.2e-03     1.2e-02  -       | 4.3e-07       6.5e-07 | 1.78e-03 / 1.78e-03   2.03e-03 / 2.03e-03
    short_bf16_dh16_S16             6.0e-03     2.7e-02  -       | 4.5e-07       4.6e-07 | 2.34e-03 / 2.34e-03   1.98e-03 / 1.98e-03
    short_bf16_dh16_S17             1.0e-02     3.0e-02  -       | 7.3e-07       9.2e-07 | 1.97e-03 / 1.97e-03   2.40e-03 / 2.40e-03
    short_bf16_dh16_S31             3.5e-03     2.3e-02  -       | 4.6e-07       4.5e-07 | 1.70e-03 / 1.70e-03   1.79e-03 / 1.79e-03
    short_bf16_dh16_S32             7.7e-03     7.6e-03  -       | 7.1e-07       8.2e-07 | 1.83e-03 / 1.83e-03   1.81e-03 / 1.81e-03
    short_f32_dh32_S1               1.6e-07     1.6e-07  -       | 1.6e-07       1.6e-07 |
    short_f32_dh32_S2               2.3e-07     3.2e-07  -       | 3.9e-07       3.4e-07 |
    short_f32_dh32_S15              4.7e-07     1.0e-06  -       | 6.2e-07       1.3e-06 |
    short_f32_dh32_S16              5.2e-07     9.2e-07  -       | 6.2e-07       1.4e-06 |
    short_f32_dh32_S17              4.7e-07     8.7e-07  -       | 5.1e-07       9.8e-07 |
    short_f32_dh32_S31              4.2e-07     1.2e-06  -       | 4.9e-07       1.2e-06 |
    short_f32_dh32_S32              4.8e-07     2.0e-06  -       | 6.7e-07       2.0e-06 |
    short_bf16_dh32_S1              1.0e-02     1.0e-02  -       | 1.6e-07       1.6e-07 | 2.88e-03 / 2.88e-03   nan / nan
    short_bf16_dh32_S2              1.3e-02     9.1e-03  -       | 2.1e-07       6.0e-07 | 2.23e-03 / 2.23e-03   3.08e-03 / 2.46e-03
    short_bf16_dh32_S15             1.7e-02     4.4e-02  -       | 6.1e-07       9.5e-07 | 2.78e-03 / 2.78e-03   3.30e-03 / 2.93e-03
    short_bf16_dh32_S16             1.2e-02     2.2e-02  -       | 3.6e-07       7.1e-07 | 2.33e-03 / 2.33e-03   2.78e-03 / 2.96e-03
    short_bf16_dh32_S17             1.0e-02     2.3e-02  -       | 4.3e-07       8.9e-07 | 2.72e-03 / 2.72e-03   2.97e-03 / 2.97e-03
    short_bf16_dh32_S31             7.4e-03     1.3e-02  -       | 3.9e-07       7.5e-07 | 2.47e-03 / 2.47e-03   2.74e-03 / 2.61e-03
    short_bf16_dh32_S32             1.0e-02     5.6e-02  -       | 6.3e-07       1.6e-06 | 2.62e-03 / 2.62e-03   3.21e-03 / 3.21e-03
    short_f32_dh64_S1               0.0e+00     0.0e+00  -       | 0.0e+00       0.0e+00 |
    short_f32_dh64_S2               4.8e-07     8.1e-07  -       | 4.9e-07       7.5e-07 |
    short_f32_dh64_S15              8.4e-07     1.1e-06  -       | 7.3e-07       9.5e-07 |
    short_f32_dh64_S16              6.5e-07     1.9e-06  -       | 6.5e-07       1.2e-06 |
    short_f32_dh64_S17              4.0e-07     7.0e-07  -       | 6.8e-07       8.0e-07 |
    short_f32_dh64_S31              9.2e-07     2.0e-06  -       | 1.0e-06       2.6e-06 |
    short_f32_dh64_S32              7.0e-07     1.4e-06  -       | 9.5e-07       1.8e-06 |
    short_bf16_dh64_S1              0.0e+00     0.0e+00  -       | 0.0e+00       0.0e+00 | 0.00e+00 / 0.00e+00   nan / nan
    short_bf16_dh64_S2              1.0e-02     2.1e-02  -       | 4.5e-07       5.4e-07 | 2.91e-03 / 2.91e-03   2.70e-03 / 2.70e-03
    short_bf16_dh64_S15             1.2e-02     1.7e-02  -       | 5.1e-07       1.3e-06 | 3.83e-03 / 3.83e-03   4.19e-03 / 4.19e-03
    short_bf16_dh64_S16             9.4e-03     2.7e-02  -       | 4.1e-07       9.5e-07 | 2.54e-03 / 2.54e-03   2.72e-03 / 2.72e-03
    short_bf16_dh64_S17             8.3e-03     1.8e-02  -       | 4.3e-07       6.0e-07 | 2.28e-03 / 2.28e-03   2.54e-03 / 2.54e-03
    short_bf16_dh64_S31             1.0e-02     7.7e-02  -       | 5.4e-07       2.6e-06 | 2.73e-03 / 2.73e-03   2.73e-03 / 2.73e-03
    short_bf16_dh64_S32             1.0e-02     2.9e-02  -       | 6.4e-07       2.2e-06 | 2.35e-03 / 2.35e-03   2.67e-03 / 2.67e-03
    short_f32_dh128_S1              0.0e+00     0.0e+00  -       | 0.0e+00       0.0e+00 |
    short_f32_dh128_S2              5.2e-07     8.1e-07  -       | 3.2e-07       5.6e-07 |
    short_f32_dh128_S15             5.1e-07     1.6e-06  -       | 7.4e-07       1.3e-06 |
    short_f32_dh128_S16             1.0e-06     1.0e-06  -       | 1.3e-06       1.5e-06 |
    short_f32_dh128_S17             9.3e-07     1.3e-06  -       | 8.5e-07       2.1e-06 |
    short_f32_dh128_S31             2.5e-06     1.8e-06  -       | 1.7e-06       2.5e-06 |
    short_f32_dh128_S32             8.0e-07     2.4e-06  -       | 6.2e-07       2.5e-06 |
    short_f32_dh256_S1              0.0e+00     0.0e+00  -       | 0.0e+00       0.0e+00 |
    short_f32_dh256_S2              1.6e-06     1.3e-06  -       | 3.7e-07       5.0e-07 |
    short_f32_dh256_S15             1.0e-06     1.1e-06  -       | 1.2e-06       1.6e-06 |
    short_f32_dh256_S16             1.9e-06     2.0e-06  -       | 1.9e-06       2.0e-06 |
    short_f32_dh256_S17             1.6e-06     1.7e-06  -       | 1.5e-06       1.8e-06 |
    short_f32_dh256_S31             1.3e-06     2.7e-06  -       | 1.5e-06       2.7e-06 |
    short_f32_dh256_S32             1.0e-06     1.9e-06  -       | 1.0e-06       2.5e-06 |
    packed_f32_dh32                 4.4e-07     5.3e-07  -       | 5.9e-07       7.7e-07 |
    packed_bf16_dh32                1.2e-02     1.0e-02  -       | 4.0e-07       1.3e-06 | 2.67e-03 / 2.67e-03   3.27e-03 / 3.38e-03
    packed_f32_dh64                 8.6e-07     9.3e-07  -       | 8.6e-07       1.3e-06 |
    packed_bf16_dh64                7.7e-03     8.3e-03  -       | 5.6e-07       5.8e-07 | 2.68e-03 / 2.68e-03   2.73e-03 / 2.73e-03
    long_f32_dh64_S1                1.2e-07     1.4e-06  4.0e-07 | 0.0e+00       0.0e+00 |
    long_f32_dh64_S1_key            1.2e-07     5.4e-07  5.7e-07 | 0.0e+00       0.0e+00 |
    long_f32_dh64_S1_causal         0.0e+00     1.9e-06  2.3e-07 | 0.0e+00       0.0e+00 |
    long_bf16_dh64_S1               0.0e+00     3.3e-07  2.1e-07 | 0.0e+00       0.0e+00 | 0.00e+00 / 0.00e+00   nan / nan
    long_bf16_dh64_S1_key           0.0e+00     3.1e-07  1.8e-07 | 0.0e+00       0.0e+00 | 0.00e+00 / 0.00e+00   nan / nan
    long_bf16_dh64_S1_causal        0.0e+00     2.0e-07  2.3e-07 | 0.0e+00       0.0e+00 | 0.00e+00 / 0.00e+00   nan / nan
    long_f32_dh32_S1                0.0e+00     1.7e-07  1.3e-07 | 0.0e+00       0.0e+00 |
    long_f32_dh32_S1_key            0.0e+00     3.1e-07  2.6e-07 | 0.0e+00       0.0e+00 |
    long_f32_dh32_S1_causal         0.0e+00     2.9e-07  2.7e-07 | 0.0e+00       0.0e+00 |
    long_bf16_dh32_S1               0.0e+00     7.5e-08  1.8e-07 | 0.0e+00       0.0e+00 | 0.00e+00 / 0.00e+00   nan / nan
    long_bf16_dh32_S1_key           0.0e+00     1.1e-07  1.8e-07 | 0.0e+00       0.0e+00 | 0.00e+00 / 0.00e+00   nan / nan
    long_bf16_dh32_S1_causal        0.0e+00     2.2e-07  4.3e-08 | 0.0e+00       0.0e+00 | 0.00e+00 / 0.00e+00   nan / nan
    long_f32_dh64_S32               1.1e-06     7.9e-07  1.0e-06 | 6.8e-07       8.2e-07 |
    long_f32_dh64_S32_key           6.0e-07     3.1e-06  5.6e-07 | 7.6e-07       2.5e-06 |
    long_f32_dh64_S32_causal        6.8e-07     3.0e-06  6.3e-07 | 7.5e-07       1.3e-06 |
    long_bf16_dh64_S32              3.3e-03     5.4e-03  3.9e-07 | 6.2e-07       4.8e-07 | 2.15e-03 / 2.39e-03   2.58e-03 / 2.61e-03
    long_bf16_dh64_S32_key          4.5e-03     3.1e-02  3.5e-07 | 4.4e-07       5.7e-07 | 2.10e-03 / 2.42e-03   2.81e-03 / 2.91e-03
    long_bf16_dh64_S32_causal       7.6e-03     2.5e-02  3.0e-07 | 4.2e-07       1.1e-06 | 1.72e-03 / 2.18e-03   3.71e-03 / 3.37e-03
    long_f32_dh32_S32               5.8e-07     1.5e-06  6.3e-07 | 5.6e-07       9.3e-07 |
    long_f32_dh32_S32_key           4.9e-07     2.4e-06  7.1e-07 | 5.0e-07       2.4e-06 |
    long_f32_dh32_S32_causal        5.6e-07     1.5e-06  5.2e-07 | 4.9e-07       1.7e-06 |
    long_bf16_dh32_S32              4.0e-03     9.4e-03  5.4e-07 | 8.0e-07       7.3e-07 | 2.19e-03 / 2.64e-03   2.84e-03 / 2.76e-03
    long_bf16_dh32_S32_key          4.5e-03     2.8e-02  5.1e-07 | 4.6e-07       6.3e-07 | 2.16e-03 / 2.55e-03   3.16e-03 / 3.10e-03
    long_bf16_dh32_S32_causal       7.0e-03     3.0e-02  4.5e-07 | 5.1e-07       1.3e-06 | 1.90e-03 / 2.27e-03   3.19e-03 / 3.46e-03
    long_f32_dh64_S33               5.2e-07     8.1e-07  5.1e-07 | 5.4e-07       1.1e-06 |
    long_f32_dh64_S33_key           5.6e-07     2.6e-06  5.5e-07 | 5.0e-07       1.4e-06 |
    long_f32_dh64_S33_causal        5.0e-07     2.5e-06  8.5e-07 | 6.8e-07       1.3e-06 |
    long_bf16_dh64_S33              3.4e-03     6.2e-03  4.6e-07 | 4.4e-07       4.6e-07 | 2.20e-03 / 2.55e-03   2.76e-03 / 2.64e-03
    long_bf16_dh64_S33_key          5.0e-03     3.1e-02  3.8e-07 | 5.1e-07       6.0e-07 | 2.11e-03 / 2.48e-03   2.71e-03 / 2.78e-03
    long_bf16_dh64_S33_causal       7.4e-03     3.0e-02  3.5e-07 | 5.5e-07       1.3e-06 | 1.84e-03 / 2.33e-03   2.96e-03 / 4.26e-03
    long_f32_dh32_S33               4.5e-07     6.9e-07  7.0e-07 | 5.9e-07       1.1e-06 |
    long_f32_dh32_S33_key           5.5e-07     1.7e-06  5.1e-07 | 8.8e-07       2.1e-06 |
    long_f32_dh32_S33_causal        4.9e-07     1.8e-06  6.2e-07 | 5.3e-07       1.3e-06 |
    long_bf16_dh32_S33              3.7e-03     6.8e-03  5.9e-07 | 4.6e-07       7.2e-07 | 2.12e-03 / 2.33e-03   2.81e-03 / 2.89e-03
    long_bf16_dh32_S33_key          7.7e-03     2.7e-02  4.3e-07 | 6.7e-07       8.6e-07 | 2.43e-03 / 2.48e-03   3.79e-03 / 3.55e-03
    long_bf16_dh32_S33_causal       6.3e-03     3.1e-02  4.4e-07 | 3.7e-07       7.7e-07 | 1.83e-03 / 2.35e-03   3.99e-03 / 3.33e-03
    long_f32_dh64_S64               4.4e-07     5.7e-07  6.2e-07 | 5.0e-07       5.6e-07 |
    long_f32_dh64_S64_key           6.0e-07     4.5e-06  7.9e-07 | 6.6e-07       5.1e-06 |
    long_f32_dh64_S64_causal        8.7e-07     4.1e-06  7.2e-07 | 9.6e-07       4.2e-06 |
    long_bf16_dh64_S64              2.9e-03     6.2e-03  6.5e-07 | 5.3e-07       6.0e-07 | 2.17e-03 / 2.45e-03   2.60e-03 / 2.66e-03
    long_bf16_dh64_S64_key          4.6e-03     6.1e-02  5.3e-07 | 5.9e-07       8.4e-07 | 2.18e-03 / 2.47e-03   2.71e-03 / 3.00e-03
    long_bf16_dh64_S64_causal       7.5e-03     3.9e-02  5.0e-07 | 7.2e-07       2.0e-06 | 1.92e-03 / 2.34e-03   3.00e-03 / 3.12e-03
    long_f32_dh32_S64               3.3e-07     6.6e-07  6.9e-07 | 4.5e-07       5.8e-07 |
    long_f32_dh32_S64_key           4.7e-07     2.9e-06  6.4e-07 | 6.6e-07       2.9e-06 |
    long_f32_dh32_S64_causal        3.5e-07     2.7e-06  6.7e-07 | 5.2e-07       2.7e-06 |
    long_bf16_dh32_S64              3.8e-03     6.5e-03  7.6e-07 | 5.0e-07       4.6e-07 | 2.19e-03 / 2.40e-03   2.60e-03 / 2.67e-03
    long_bf16_dh32_S64_key          4.6e-03     2.9e-02  6.7e-07 | 8.2e-07       1.2e-06 | 2.21e-03 / 2.51e-03   2.63e-03 / 2.82e-03
    long_bf16_dh32_S64_causal       7.6e-03     3.0e-02  7.1e-07 | 4.2e-07       1.3e-06 | 1.95e-03 / 2.34e-03   3.22e-03 / 3.19e-03
    long_f32_dh64_S65               4.8e-07     7.7e-07  5.9e-07 | 7.3e-07       7.7e-07 |
    long_f32_dh64_S65_key           7.7e-07     6.0e-06  6.4e-07 | 7.7e-07       6.0e-06 |
    long_f32_dh64_S65_causal        6.4e-07     4.6e-06  9.7e-07 | 9.3e-07       3.7e-06 |
    long_bf16_dh64_S65              2.5e-03     4.7e-03  7.4e-07 | 5.8e-07       5.6e-07 | 2.13e-03 / 2.44e-03   2.49e-03 / 2.55e-03
    long_bf16_dh64_S65_key          3.9e-03     4.6e-02  4.9e-07 | 4.6e-07       7.9e-07 | 2.19e-03 / 2.50e-03   2.52e-03 / 2.57e-03
    long_bf16_dh64_S65_causal       7.7e-03     3.3e-02  4.5e-07 | 3.8e-07       2.0e-06 | 1.87e-03 / 2.39e-03   2.96e-03 / 3.37e-03
    long_f32_dh32_S65               5.2e-07     1.1e-06  7.3e-07 | 5.0e-07       9.4e-07 |
    long_f32_dh32_S65_key           4.5e-07     8.4e-06  6.8e-07 | 6.6e-07       8.4e-06 |
    long_f32_dh32_S65_causal        4.4e-07     2.5e-06  6.0e-07 | 6.6e-07       3.1e-06 |
    long_bf16_dh32_S65              3.8e-03     5.1e-03  7.6e-07 | 3.8e-07       6.2e-07 | 2.23e-03 / 2.58e-03   2.63e-03 / 2.70e-03
    long_bf16_dh32_S65_key          4.2e-03     5.7e-02  7.3e-07 | 4.8e-07       6.7e-07 | 2.22e-03 / 2.59e-03   2.89e-03 / 2.94e-03
    long_bf16_dh32_S65_causal       7.5e-03     5.5e-02  7.0e-07 | 5.6e-07       1.9e-06 | 1.90e-03 / 2.32e-03   2.99e-03 / 3.63e-03
    long_f32_dh64_S128              6.1e-07     1.4e-06  6.3e-07 | 5.9e-07       8.2e-07 |
    long_f32_dh64_S128_key          7.8e-07     8.5e-06  7.3e-07 | 8.0e-07       6.6e-06 |
    long_f32_dh64_S128_causal       8.0e-07     6.2e-06  6.5e-07 | 6.9e-07       4.4e-06 |
    long_bf16_dh64_S128             2.2e-03     4.4e-03  6.8e-07 | 3.7e-07       6.7e-07 | 2.18e-03 / 2.35e-03   2.46e-03 / 2.52e-03
    long_bf16_dh64_S128_key         3.4e-03     6.1e-02  6.7e-07 | 4.1e-07       8.8e-07 | 2.18e-03 / 2.43e-03   2.46e-03 / 2.50e-03
    long_bf16_dh64_S128_causal      8.3e-03     6.1e-02  5.8e-07 | 4.6e-07       3.6e-06 | 2.05e-03 / 2.24e-03   2.79e-03 / 2.94e-03
    long_f32_dh32_S128              4.5e-07     7.9e-07  8.9e-07 | 6.0e-07       6.8e-07 |
    long_f32_dh32_S128_key          7.8e-07     1.0e-05  9.0e-07 | 9.3e-07       8.3e-06 |
    long_f32_dh32_S128_causal       6.3e-07     4.6e-06  7.7e-07 | 6.4e-07       4.4e-06 |
    long_bf16_dh32_S128             2.3e-03     5.9e-03  8.0e-07 | 4.6e-07       8.3e-07 | 2.27e-03 / 2.48e-03   2.59e-03 / 2.68e-03
    long_bf16_dh32_S128_key         4.0e-03     5.9e-02  7.6e-07 | 3.8e-07       5.9e-07 | 2.15e-03 / 2.41e-03   2.67e-03 / 2.59e-03
    long_bf16_dh32_S128_causal      6.0e-03     3.8e-02  6.6e-07 | 5.1e-07       1.5e-06 | 1.90e-03 / 2.33e-03   2.95e-03 / 2.86e-03
    long_f32_dh64_S129              4.8e-07     8.6e-07  7.1e-07 | 4.5e-07       6.8e-07 |
    long_f32_dh64_S129_key          5.5e-07     8.5e-06  6.9e-07 | 8.8e-07       8.4e-06 |
    long_f32_dh64_S129_causal       7.8e-07     4.0e-06  7.1e-07 | 8.9e-07       5.7e-06 |
    long_bf16_dh64_S129             2.4e-03     4.8e-03  6.3e-07 | 5.7e-07       1.1e-06 | 2.22e-03 / 2.39e-03   2.52e-03 / 2.50e-03
    long_bf16_dh64_S129_key         2.9e-03     1.2e-01  7.5e-07 | 5.7e-07       9.5e-07 | 2.24e-03 / 2.42e-03   2.46e-03 / 2.49e-03
    long_bf16_dh64_S129_causal      7.8e-03     5.0e-02  6.6e-07 | 7.3e-07       4.2e-06 | 1.97e-03 / 2.29e-03   2.70e-03 / 3.10e-03
    long_f32_dh32_S129              5.9e-07     1.2e-06  7.3e-07 | 4.7e-07       5.1e-07 |
    long_f32_dh32_S129_key          6.7e-07     6.0e-06  6.6e-07 | 5.0e-07       5.4e-06 |
    long_f32_dh32_S129_causal       4.3e-07     5.8e-06  6.7e-07 | 7.7e-07       4.7e-06 |
    long_bf16_dh32_S129             2.2e-03     5.1e-03  8.9e-07 | 3.9e-07       5.5e-07 | 2.25e-03 / 2.46e-03   2.50e-03 / 2.50e-03
    long_bf16_dh32_S129_key         3.5e-03     5.9e-02  7.5e-07 | 4.1e-07       9.3e-07 | 2.17e-03 / 2.39e-03   2.55e-03 / 2.61e-03
    long_bf16_dh32_S129_causal      4.7e-03     6.0e-02  7.2e-07 | 4.3e-07       2.3e-06 | 1.91e-03 / 2.32e-03   3.06e-03 / 3.12e-03
    long_f32_dh64_S224              6.0e-07     9.2e-07  8.7e-07 | 7.2e-07       9.1e-07 |
    long_f32_dh64_S224_key          8.9e-07     3.3e-05  8.7e-07 | 7.8e-07       2.9e-05 |
    long_f32_dh64_S224_causal       7.9e-07     8.9e-06  1.1e-06 | 7.1e-07       9.5e-06 |
    long_bf16_dh64_S224             2.0e-03     3.7e-03  7.7e-07 | 3.8e-07       7.7e-07 | 2.21e-03 / 2.36e-03   2.44e-03 / 2.46e-03
    long_bf16_dh64_S224_key         3.3e-03     1.2e-01  7.1e-07 | 6.9e-07       9.5e-07 | 2.19e-03 / 2.39e-03   2.43e-03 / 2.44e-03
    long_bf16_dh64_S224_causal      7.0e-03     1.2e-01  6.8e-07 | 5.0e-07       8.0e-06 | 1.98e-03 / 2.42e-03   2.85e-03 / 2.85e-03
    long_f32_dh32_S224              6.6e-07     6.5e-07  9.2e-07 | 5.3e-07       5.5e-07 |
    long_f32_dh32_S224_key          5.5e-07     2.0e-05  9.5e-07 | 8.3e-07       2.0e-05 |
    long_f32_dh32_S224_causal       7.4e-07     1.0e-05  8.1e-07 | 7.7e-07       1.4e-05 |
    long_bf16_dh32_S224             2.6e-03     6.3e-03  9.6e-07 | 4.9e-07       7.6e-07 | 2.30e-03 / 2.49e-03   2.52e-03 / 2.58e-03
    long_bf16_dh32_S224_key         2.4e-03     6.1e-02  9.8e-07 | 5.2e-07       9.9e-07 | 2.27e-03 / 2.45e-03   3.12e-03 / 3.12e-03
    long_bf16_dh32_S224_causal      7.9e-03     6.2e-02  8.7e-07 | 5.5e-07       4.2e-06 | 2.01e-03 / 2.59e-03   3.20e-03 / 3.20e-03
    long_f32_dh64_S225              6.9e-07     1.5e-06  7.1e-07 | 6.1e-07       8.5e-07 |
    long_f32_dh64_S225_key          8.5e-07     1.2e-05  7.7e-07 | 7.7e-07       1.5e-05 |
    long_f32_dh64_S225_causal       8.1e-07     6.9e-06  8.8e-07 | 5.5e-07       7.0e-06 |
    long_bf16_dh64_S225             2.1e-03     3.4e-03  7.4e-07 | 4.9e-07       8.5e-07 | 2.30e-03 / 2.45e-03   2.46e-03 / 2.49e-03
    long_bf16_dh64_S225_key         3.5e-03     1.1e-01  7.1e-07 | 4.1e-07       1.9e-06 | 2.32e-03 / 2.89e-03   2.90e-03 / 2.90e-03
    long_bf16_dh64_S225_causal      8.3e-03     6.2e-02  8.1e-07 | 8.1e-07       4.6e-06 | 1.96e-03 / 3.41e-03   3.26e-03 / 3.26e-03
    long_f32_dh32_S225              4.7e-07     1.3e-06  9.2e-07 | 6.3e-07       1.1e-06 |
    long_f32_dh32_S225_key          6.1e-07     1.5e-05  8.8e-07 | 7.2e-07       1.6e-05 |
    long_f32_dh32_S225_causal       1.0e-06     1.0e-05  9.2e-07 | 1.0e-06       1.0e-05 |
    long_bf16_dh32_S225             2.0e-03     3.1e-03  8.6e-07 | 3.4e-07       5.1e-07 | 2.28e-03 / 2.44e-03   2.54e-03 / 2.52e-03
    long_bf16_dh32_S225_key         3.8e-03     8.9e-02  8.3e-07 | 4.8e-07       7.3e-07 | 2.32e-03 / 3.94e-03   3.24e-03 / 3.24e-03
    long_bf16_dh32_S225_causal      7.8e-03     8.9e-02  7.7e-07 | 4.1e-07       2.6e-06 | 1.92e-03 / 2.85e-03   3.17e-03 / 3.17e-03
    long_f32_dh64_S256              4.3e-07     6.2e-07  7.6e-07 | 4.2e-07       5.3e-07 |
    long_f32_dh64_S256_key          5.7e-07     1.4e-05  8.0e-07 | 7.9e-07       1.5e-05 |
    long_f32_dh64_S256_causal       6.0e-07     1.2e-05  7.2e-07 | 8.4e-07       1.2e-05 |
    long_bf16_dh64_S256             1.9e-03     3.4e-03  7.8e-07 | 5.9e-07       8.7e-07 | 2.23e-03 / 2.42e-03   2.43e-03 / 2.44e-03
    long_bf16_dh64_S256_key         3.8e-03     1.1e-01  7.6e-07 | 5.7e-07       9.9e-07 | 2.25e-03 / 2.45e-03   2.49e-03 / 2.50e-03
    long_bf16_dh64_S256_causal      7.5e-03     1.1e-01  7.1e-07 | 7.9e-07       4.4e-06 | 2.02e-03 / 2.34e-03   2.76e-03 / 2.94e-03
    long_f32_dh32_S256              5.5e-07     9.0e-07  9.5e-07 | 4.8e-07       7.6e-07 |
    long_f32_dh32_S256_key          3.9e-07     1.5e-05  8.3e-07 | 4.6e-07       1.5e-05 |
    long_f32_dh32_S256_causal       5.2e-07     8.6e-06  8.0e-07 | 5.8e-07       6.4e-06 |
    long_bf16_dh32_S256             1.6e-03     3.9e-03  8.7e-07 | 4.0e-07       6.8e-07 | 2.31e-03 / 2.47e-03   2.58e-03 / 2.57e-03
    long_bf16_dh32_S256_key         2.6e-03     1.0e-01  9.3e-07 | 4.0e-07       1.1e-06 | 2.26e-03 / 2.47e-03   2.49e-03 / 2.52e-03
    long_bf16_dh32_S256_causal      7.8e-03     9.0e-02  7.7e-07 | 6.7e-07       4.1e-06 | 2.00e-03 / 2.33e-03   2.72e-03 / 2.78e-03
    long_f32_dh64_S16               6.9e-07     9.8e-07  5.7e-07 | 6.9e-07       9.9e-07 |
    long_bf16_dh32_S16              4.2e-03     7.1e-03  3.7e-07 | 5.0e-07       4.9e-07 | 2.16e-03 / 2.69e-03   2.71e-03 / 2.85e-03
    long_f32_dh32_S17               4.0e-07     1.1e-06  6.3e-07 | 4.7e-07       5.0e-07 |
    long_bf16_dh64_S17              4.4e-03     1.0e-02  4.1e-07 | 8.1e-07       4.6e-07 | 2.17e-03 / 2.52e-03   2.80e-03 / 2.86e-03
    long_f32_dh64_S144              6.0e-07     8.9e-07  6.5e-07 | 7.1e-07       8.4e-07 |
    long_bf16_dh32_S144             2.4e-03     4.6e-03  8.5e-07 | 4.2e-07       5.9e-07 | 2.26e-03 / 2.49e-03   2.58e-03 / 2.70e-03
    long_f32_dh32_S145              6.4e-07     8.2e-07  8.8e-07 | 5.2e-07       5.4e-07 |
    long_bf16_dh64_S145             2.0e-03     4.0e-03  7.7e-07 | 3.8e-07       5.9e-07 | 2.26e-03 / 2.44e-03   2.45e-03 / 2.47e-03
    long_f32_dh64_S161              8.0e-07     1.9e-06  7.0e-07 | 9.6e-07       1.5e-06 |
    long_bf16_dh32_S161             3.5e-03     4.6e-03  9.3e-07 | 5.5e-07       8.2e-07 | 2.30e-03 / 2.41e-03   2.58e-03 / 2.58e-03
    long_f32_dh32_S193              6.0e-07     1.1e-06  8.5e-07 | 7.7e-07       9.9e-07 |
    long_bf16_dh64_S193             1.9e-03     5.5e-03  7.2e-07 | 6.7e-07       1.2e-06 | 2.25e-03 / 2.42e-03   2.57e-03 / 2.57e-03
    long_f32_dh64_S209              8.1e-07     9.8e-07  7.9e-07 | 8.0e-07       7.1e-07 |
    long_bf16_dh32_S209             2.2e-03     5.4e-03  8.9e-07 | 4.9e-07       5.7e-07 | 2.24e-03 / 2.42e-03   2.55e-03 / 2.59e-03
    long_f32_dh32_S241              5.7e-07     9.4e-07  8.9e-07 | 5.6e-07       7.9e-07 |
    long_bf16_dh64_S241             2.0e-03     4.1e-03  7.8e-07 | 6.4e-07       7.0e-07 | 2.28e-03 / 2.40e-03   2.45e-03 / 2.44e-03
    long_bf16_dh64_S129_drop        3.6e-03     7.0e-03  7.6e-07 | 6.8e-07       1.0e-06 | 2.26e-03 / 2.41e-03   2.46e-03 / 2.51e-03
    long_bf16_dh64_S144             2.4e-03     6.7e-03  7.1e-07 | 6.2e-07       7.7e-07 | 2.20e-03 / 2.37e-03   2.55e-03 / 2.52e-03
    long_bf16_dh64_S144_drop        2.5e-03     7.3e-03  8.4e-07 | 8.2e-07       8.1e-07 | 2.20e-03 / 2.41e-03   2.60e-03 / 2.58e-03
    long_bf16_dh64_S145_drop        2.8e-03     7.1e-03  7.0e-07 | 7.0e-07       1.0e-06 | 2.23e-03 / 2.43e-03   2.54e-03 / 2.62e-03
    long_bf16_dh64_S161             2.2e-03     3.9e-03  7.8e-07 | 8.4e-07       7.5e-07 | 2.24e-03 / 2.42e-03   2.48e-03 / 2.52e-03
    long_bf16_dh64_S161_drop        3.1e-03     4.6e-03  7.4e-07 | 5.8e-07       8.5e-07 | 2.25e-03 / 2.45e-03   2.43e-03 / 2.46e-03
    long_bf16_dh64_S193_drop        2.9e-03     6.5e-03  7.3e-07 | 6.2e-07       9.2e-07 | 2.28e-03 / 2.43e-03   2.57e-03 / 2.60e-03
    long_bf16_dh64_S209             1.8e-03     3.3e-03  7.0e-07 | 4.3e-07       5.6e-07 | 2.24e-03 / 2.42e-03   2.44e-03 / 2.45e-03
    long_bf16_dh64_S209_drop        2.2e-03     5.8e-03  8.0e-07 | 5.9e-07       9.9e-07 | 2.26e-03 / 2.40e-03   2.48e-03 / 2.48e-03
    long_bf16_dh64_S224_drop        2.5e-03     8.2e-03  7.6e-07 | 4.1e-07       1.4e-06 | 2.26e-03 / 2.43e-03   2.50e-03 / 2.74e-03
    long_f32_dh128_S17              7.6e-07     9.0e-07  5.2e-07 | 1.1e-06       9.2e-07 |
    long_f32_dh128_S17_causal       7.0e-07     2.6e-06  5.4e-07 | 7.9e-07       1.5e-06 |
    long_f32_dh128_S33              8.6e-07     1.6e-06  8.4e-07 | 8.0e-07       1.2e-06 |
    long_f32_dh128_S33_causal       1.6e-06     3.0e-06  9.0e-07 | 1.1e-06       1.7e-06 |
    long_f32_dh128_S65              9.1e-07     1.2e-06  7.9e-07 | 6.7e-07       8.8e-07 |
    long_f32_dh128_S65_causal       1.0e-06     4.4e-06  7.2e-07 | 1.0e-06       3.4e-06 |
    long_f32_dh128_S128             1.0e-06     1.0e-06  8.0e-07 | 1.2e-06       1.4e-06 |
    long_f32_dh128_S128_causal      9.3e-07     1.2e-05  1.1e-06 | 9.6e-07       7.1e-06 |
    long_f32_dh64_S17_drop          6.1e-07     1.3e-06  3.9e-07 | 7.3e-07       1.2e-06 |
    long_bf16_dh64_S17_drop         5.5e-03     1.1e-02  3.5e-07 | 3.9e-07       5.5e-07 | 2.19e-03 / 2.38e-03   2.91e-03 / 3.09e-03
    long_f32_dh32_S17_drop          5.5e-07     9.6e-07  3.9e-07 | 7.3e-07       8.1e-07 |
    long_bf16_dh32_S17_drop         5.1e-03     6.2e-03  5.0e-07 | 5.7e-07       5.8e-07 | 2.08e-03 / 2.59e-03   3.07e-03 / 3.74e-03
    long_f32_dh128_S17_drop         7.5e-07     1.0e-06  6.2e-07 | 8.7e-07       7.8e-07 |
    long_f32_dh64_S33_drop          1.0e-06     1.7e-06  5.2e-07 | 6.4e-07       8.2e-07 |
    long_bf16_dh64_S33_drop         4.4e-03     8.9e-03  4.8e-07 | 7.8e-07       8.3e-07 | 2.22e-03 / 2.54e-03   2.57e-03 / 2.62e-03
    long_f32_dh32_S33_drop          5.5e-07     1.1e-06  5.5e-07 | 5.3e-07       7.8e-07 |
    long_bf16_dh32_S33_drop         4.4e-03     7.4e-03  5.8e-07 | 6.4e-07       6.4e-07 | 2.18e-03 / 2.62e-03   2.69e-03 / 3.83e-03
    long_f32_dh128_S33_drop         8.0e-07     1.3e-06  6.9e-07 | 9.3e-07       9.3e-07 |
    long_f32_dh64_S65_drop          8.0e-07     9.0e-07  5.8e-07 | 5.2e-07       7.7e-07 |
    long_bf16_dh64_S65_drop         3.7e-03     5.9e-03  7.5e-07 | 5.8e-07       7.1e-07 | 2.16e-03 / 2.43e-03   2.66e-03 / 2.67e-03
    long_f32_dh32_S65_drop          6.7e-07     9.7e-07  6.0e-07 | 5.4e-07       6.0e-07 |
    long_bf16_dh32_S65_drop         3.7e-03     9.4e-03  7.1e-07 | 4.1e-07       9.4e-07 | 2.15e-03 / 2.39e-03   2.78e-03 / 2.77e-03
    long_f32_dh128_S65_drop         6.7e-07     1.4e-06  7.2e-07 | 1.3e-06       1.4e-06 |
    long_f32_dh64_S145_drop         7.8e-07     1.3e-06  7.0e-07 | 6.3e-07       7.7e-07 |
    long_f32_dh32_S145_drop         5.1e-07     7.6e-07  8.4e-07 | 5.5e-07       9.6e-07 |
    long_bf16_dh32_S145_drop        3.9e-03     5.4e-03  8.8e-07 | 5.8e-07       7.8e-07 | 2.22e-03 / 2.48e-03   2.60e-03 / 2.58e-03
    long_f32_dh64_S241_drop         4.5e-07     8.9e-07  8.0e-07 | 4.8e-07       9.1e-07 |
    long_bf16_dh64_S241_drop        2.4e-03     5.5e-03  7.5e-07 | 5.3e-07       5.7e-07 | 2.24e-03 / 2.38e-03   2.50e-03 / 2.52e-03
    long_f32_dh32_S241_drop         4.3e-07     8.8e-07  9.8e-07 | 8.1e-07       9.7e-07 |
    long_bf16_dh32_S241_drop        3.7e-03     5.7e-03  8.8e-07 | 5.6e-07       9.5e-07 | 2.30e-03 / 2.44e-03   2.51e-03 / 2.52e-03
    walk_cu256_S197_drop0           4.0e-03     9.2e-03  8.8e-07 | (GPU reference)        | 2.31e-03 / 2.49e-03   2.66e-03 / 2.72e-03
    walk_cu256_S129_drop0           4.1e-03     8.4e-03  7.8e-07 | (GPU reference)        | 2.29e-03 / 2.51e-03   2.63e-03 / 2.83e-03
    walk_cu256_S197_drop1           4.1e-03     1.0e-02  8.8e-07 | (GPU reference)        | 2.26e-03 / 2.51e-03   2.60e-03 / 2.61e-03
    walk_cu256_S129_drop1           4.1e-03     1.1e-02  7.8e-07 | (GPU reference)        | 2.28e-03 / 2.53e-03   2.68e-03 / 2.87e-03
"""
import math
import os
import subprocess
import sys

import pytest
import torch

import attn_ref as R

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda:0')


def _gaps(c):
    Hd = c.Hd
    return [(Hd, Hd + 8), (2 * Hd + 8, 2 * Hd + 16), (3 * Hd + 16, c.ld)]


def run_kernels(c):
    """forward + backward of the case on the device; returns out, dq, dk, dv as fp64 [n, nh, S, dh] and lse [n, nh, S] (long kernels), after the
    sentinel checks: rows >= n_items * S, the gap columns of dqkv, the columns of out beyond Hd and the tail of lse are bit-identical to the pre-fill,
    and the inputs are untouched."""
    from adapter4rec_amd import _lib as L
    d = dev()
    qkv, dout = c.qkv.to(d), c.dout.to(d)
    out = torch.full((c.Mp, c.ldo), R.SENTINEL, dtype=c.t, device=d)
    dqkv = torch.full((c.Mp, c.ld), R.SENTINEL, dtype=c.t, device=d)
    km = c.key_mask.to(d) if c.key_mask is not None else None
    offs = (c.off['q'], c.off['k'], c.off['v'])
    kw = dict(drop_p=c.drop, drop_site=c.drop_site, drop_seed=c.drop_seed)
    n_stat = c.n_items * c.nh * c.S
    lse = None
    if c.family == 'short':
        o = c.offsets.to(d) if c.offsets is not None else None
        L.attn_fwd(qkv, out, km, c.n_items, c.S, c.nh, c.dh, *offs, c.causal, c.scale, c.neg, offsets=o, **kw)
        L.attn_bwd(qkv, dout, dqkv, km, c.n_items, c.S, c.nh, c.dh, *offs, c.causal, c.scale, c.neg, offsets=o, **kw)
    else:
        lse = torch.full((n_stat + 64,), R.SENTINEL, device=d)
        ws = torch.zeros(n_stat, device=d)
        L.attn_long_fwd(qkv, out, lse, c.n_items, c.S, c.nh, c.dh, *offs, c.scale, key_mask=km, causal=c.causal, **kw)
        L.attn_long_bwd(qkv, out, dout, dqkv, lse, ws, c.n_items, c.S, c.nh, c.dh, *offs, c.scale, key_mask=km, causal=c.causal, **kw)
    torch.cuda.synchronize()
    sent = lambda t: bool((t == R.SENTINEL).all())
    assert sent(out[c.n_rows:]) and sent(out[:, c.Hd:]), f'{c.name}: out written outside its rows / columns'
    assert sent(dqkv[c.n_rows:]), f'{c.name}: dqkv written behind the last row'
    for a, b in _gaps(c):
        assert sent(dqkv[:, a:b]), f'{c.name}: dqkv gap columns {a}..{b} written'
    assert torch.equal(qkv, c.qkv.to(d)) and torch.equal(dout, c.dout.to(d)), f'{c.name}: an input was written'
    got = dict(out=R.gather(c, out, 0), dq=R.gather(c, dqkv, c.off['q']), dk=R.gather(c, dqkv, c.off['k']), dv=R.gather(c, dqkv, c.off['v']))
    if lse is not None:
        assert sent(lse[n_stat:]), f'{c.name}: lse written behind its end'
        got['lse'] = lse[:n_stat].view(c.n_items, c.nh, c.S).double()
    return got


def check_case(c, got, ref, fig):
    figures, fails = R.judge(c, got, ref, fig)
    line = f'KERNEL {c.name} ' + ' '.join(f'{x}={figures[x][0]:.1e}' for x in R.TENSORS)
    if 'lse' in got:
        lse, rl = got['lse'], ref.lse.to(got['lse'].device)
        assert bool(torch.isfinite(lse).all()), f'{c.name}: lse not finite'
        has_key = (c.valid & c.any_key).to(lse.device)[:, None, :].expand_as(lse)
        err = ((lse - rl).abs() * has_key)
        atol, rtol = (1e-3, 1e-3) if c.t == torch.float32 else (2e-2, 1e-3)
        line += f' lse={float(err.max()):.1e}'
        if bool((err > atol + rtol * rl.abs()).any()):
            fails.append(f'lse: max err {float(err.max()):.3e}')
    if c.t == torch.bfloat16:
        line += ' RMS ' + ' '.join(f'{x}={figures[x][2]:.2e}' for x in R.TENSORS)
    print(line)
    assert not fails, (c.name, fails)


def _run(name):
    c = R.case(name)
    got = {k: v.cpu() for k, v in run_kernels(c).items()}
    check_case(c, got, c.ref, c.fig)


@pytest.mark.parametrize('name', R.names('short_'))
def test_short_kernels(name):
    _run(name)


@pytest.mark.parametrize('name', R.names('packed_'))
def test_short_kernels_packed_items(name):
    """a4r_attn_t.offsets: items of 32, 1, 17, 16, 15, 31 and 2 tokens back to back, each against the reference evaluated on its own tokens"""
    _run(name)


@pytest.mark.parametrize('name', R.names('long_'))
def test_long_kernels(name):
    _run(name)


def test_wide_heads_refuse_bf16():
    """head widths 128 / 256 are fp32 instantiations only: a bf16 launch is refused, not run by something else"""
    from adapter4rec_amd import _lib as L
    d = dev()
    for dh in (128, 256):
        qkv = torch.zeros(128, 3 * dh, dtype=torch.bfloat16, device=d)
        out = torch.zeros(128, dh, dtype=torch.bfloat16, device=d)
        km = torch.ones(3, 17, device=d)
        with pytest.raises(RuntimeError):
            L.attn_fwd(qkv, out, km, 3, 17, 1, dh, 0, dh, 2 * dh, False, 0.1, -1e9)
        with pytest.raises(RuntimeError):
            L.attn_bwd(qkv, out, torch.zeros_like(qkv), km, 3, 17, 1, dh, 0, dh, 2 * dh, False, 0.1, -1e9)
    qkv = torch.zeros(256, 384, dtype=torch.bfloat16, device=d)
    out = torch.zeros(256, 128, dtype=torch.bfloat16, device=d)
    lse = torch.zeros(256, device=d)
    with pytest.raises(RuntimeError):
        L.attn_long_fwd(qkv, out, lse, 3, 33, 1, 128, 0, 128, 256, 0.1)
    with pytest.raises(RuntimeError):
        L.attn_long_bwd(qkv, out, out, torch.zeros_like(qkv), lse, torch.zeros_like(lse), 3, 33, 1, 128, 0, 128, 256, 0.1)
    with pytest.raises(RuntimeError):                                   # ... and fp32 up to 128 tokens
        L.attn_long_fwd(qkv.float(), out.float(), lse, 1, 129, 1, 128, 0, 128, 256, 0.1)


@pytest.mark.parametrize('S', [197, 129])
@pytest.mark.parametrize('drop', [0.0, 0.25])
def test_onepass_persistent_walk(S, drop):
    """a4r_attn_long_bwd1_launch starts min(pairs, CU count) persistent workgroups that walk the (item, head) pairs with stride = the grid.  With
    2.5 pairs per CU every workgroup serves two or three: the image-set switch, the LDS-DMA prefetch of the next pair under the current one, the
    O / K / V prefetch and the reuse of region R across pairs all run.  Every item has its own random data, so a pair served from the wrong image
    set misses the per-(item, head) bound (tests/test_attn_ref_cpu.py: the pair-swap mutation).  Reference and bf16 model are computed on the GPU."""
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    c = R.make_case(**R.walk_spec(cu, S, drop), device=dev())
    n_pairs = c.n_items * c.nh
    assert n_pairs > cu and 2 * cu < n_pairs < 3 * cu, (n_pairs, cu)
    ref = R.reference(c)
    fig = R.model_figures(c, ref)
    print(f'BF16MODEL {c.name} ' + ' '.join(f'{x}={fig[x][0]:.2e}/{fig[x][1]:.2e}' for x in R.TENSORS))
    check_case(c, run_kernels(c), ref, fig)


@pytest.mark.parametrize('fused', ['0', '1'])
def test_launch_form(fused):
    """A4R_ATTN_BWD_ONEPASS=0 with A4R_ATTN_BWD_FUSED=0 / 1: the two-launch / one-launch backward for EVERY length, the one-pass kernel off (the switches
    are read once per process, hence a child process): every long-kernel case of this file passes in both forms."""
    env = dict(os.environ, A4R_ATTN_BWD_ONEPASS='0', A4R_ATTN_BWD_FUSED=fused)
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-p', 'no:cacheprovider', '-k', 'test_long_kernels'],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert ' passed' in r.stdout and 'failed' not in r.stdout, r.stdout[-500:]
