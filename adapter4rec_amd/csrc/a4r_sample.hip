// a4r_id_sample: the ID tower's training batch drawn on the device (include/a4r.h; data_utils.DeviceIdSampler, --device_sampler 1).
//
// One wave per batch row.  The user's sequence (L <= 256 ids) goes into LDS, is sorted by rank counting (at most 4 elements per lane, every
// lane reads the whole sequence as LDS broadcasts), and each lane then draws the negatives of positions lane, lane + 64, ...: one counter
// hash, one 64 x 64-bit high product onto 0 .. m-1, and a walk up the sorted distinct ids that steps over the user's own items.  No
// rejection loop, no float work, no scratch memory; the only atomic is the integer add on *err.
#include "a4r_common.h"
#include "../../include/a4r.h"

namespace {

constexpr int SAMPLE_MAX_L = 256;

A4R_DEV int wave_sum_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(64) void id_sample_kernel(const int32_t* __restrict__ seqs, int n_users, int L, const int32_t* __restrict__ rows,
                                                       int item_num, uint64_t seed, uint64_t draw, int negatives,
                                                       int64_t* __restrict__ ids, float* __restrict__ log_mask, int32_t* __restrict__ err) {
    __shared__ int32_t s_seq[SAMPLE_MAX_L], s_sorted[SAMPLE_MAX_L];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int u = rows[b];
    const bool in_range = u >= 0 && u < n_users;                   // an out-of-range row reads nothing: it is a row of pads
    const int32_t* row = seqs + (size_t)(in_range ? u : 0) * L;
    for (int l = lane; l < L; l += 64) s_seq[l] = in_range ? row[l] : 0;
    __syncthreads();
    int64_t m = 0;
    if (negatives && in_range) {                                   // (uniform over the wave)
        // rank of element i among the L ids: smaller ones, and equal ones in front of it -- a permutation, so every slot is written once
        for (int i = lane; i < L; i += 64) {
            const int32_t v = s_seq[i];
            int rank = 0;
            for (int j = 0; j < L; ++j) {
                const int32_t w = s_seq[j];
                rank += (w < v || (w == v && j < i)) ? 1 : 0;
            }
            s_sorted[rank] = v;
        }
        __syncthreads();
        int d = 0;                                                 // d = |D|: the first of every run of equal non-zero ids
        for (int k = lane; k < L; k += 64) {
            const int32_t s = s_sorted[k];
            d += (s != 0 && (k == 0 || s != s_sorted[k - 1])) ? 1 : 0;
        }
        d = wave_sum_i32(d);
        m = (int64_t)item_num - d;
    }
    const bool bad = !in_range || (negatives && m < 1);
    if (bad && lane == 0) atomicAdd(err, 1);
    const bool drawing = negatives && !bad;
    int64_t* out = ids + (size_t)b * L * 2;
    float* lm = log_mask + (size_t)b * (L - 1);
    for (int l = lane; l < L; l += 64) {
        const int32_t pos = s_seq[l];
        int64_t x = 0;
        if (drawing && l < L - 1 && pos != 0) {
            const uint64_t h = a4r_hash64(seed, A4R_SAMPLE_SITE, (draw << 40) | ((uint64_t)(uint32_t)u << 8) | (uint64_t)l);
            x = (int64_t)__umul64hi(h, (uint64_t)m) + 1;           // uniform over 1 .. m: the x-th item that is not the user's
            for (int k = 0; k < L; ++k) {
                const int32_t s = s_sorted[k];
                if (s == 0 || (k > 0 && s == s_sorted[k - 1])) continue;
                if (x >= (int64_t)s) ++x;
            }
        }
        out[2 * l] = pos;
        out[2 * l + 1] = x;
        if (l < L - 1) lm[l] = pos != 0 ? 1.0f : 0.0f;
    }
}

}  // namespace

extern "C" int a4r_id_sample(void* stream, const int32_t* seqs, int n_users, int L, const int32_t* rows, int B, int item_num,
                             uint64_t seed, uint64_t draw, int negatives, int64_t* ids, float* log_mask, int32_t* err) {
    if (!seqs || !rows || !ids || !log_mask || !err || L < 2 || L > SAMPLE_MAX_L || B < 1 || n_users < 1 || item_num < 1 || draw >= (1ull << 24))
        return A4R_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (hipMemsetAsync(err, 0, sizeof(int32_t), s) != hipSuccess) return A4R_ELAUNCH;
    hipLaunchKernelGGL(id_sample_kernel, dim3(B), dim3(64), 0, s, seqs, n_users, L, rows, item_num, seed, draw, negatives ? 1 : 0, ids, log_mask, err);
    return a4r_launch_status();
}
