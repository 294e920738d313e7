// The learned item-ID table of the IDRec baseline (Downstream/CV/model/model.py: nn.Embedding(item_num + 1, E, padding_idx=0)):
// a4r_id_index builds, once per step, the row each slot reads and the inverted index (for every distinct id its slots, in ascending
// slot order); a4r_id_grad_sum sums the slots' gradient rows through that index into the table's gradient.  Integer work only in the
// index and a fixed summation order in the gradient: the table gradient is a function of the batch alone, bit for bit (no float atomics).
//
// Index = a stable LSD radix sort of the slots by id, 8 bits per pass, over ceil(bits(item_num) / 8) passes.  Each pass is three launches
// over tiles of TILE slots: a 256-bin histogram per tile, one exclusive scan of the digit-major [256, tiles] histogram, and a scatter that
// ranks equal digits inside a tile in slot order (wave ballots per 256-slot round, wave counts through LDS).  Out-of-range ids and id 0 sort
// under key 0, in front of every list; the CSR is then the sorted slot array with one head per run of equal non-zero keys.  Every grid is
// sized from n alone and every count the later launches need stays on the device.
#include "a4r_common.h"
#include "../../include/a4r.h"

namespace {

constexpr int NT = 256;                    // threads per workgroup of the tile kernels
constexpr int ROUNDS = 16;                 // slots per thread per tile
constexpr int TILE = NT * ROUNDS;          // 4096 slots per tile
constexpr int SCAN_NT = 1024;              // the single-workgroup scan
constexpr int MAX_N = 1 << 20;

A4R_DEV int tiles_of(int n) { return (n + TILE - 1) / TILE; }

// exclusive scan of one int per thread over the workgroup; *total = the sum.  lds: NTH ints.
template <int NTH>
A4R_DEV int block_excl_scan(int v, int* lds, int* total) {
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int off = 1; off < NTH; off <<= 1) {
        const int a = t >= off ? lds[t - off] : 0;
        __syncthreads();
        lds[t] += a;
        __syncthreads();
    }
    const int incl = lds[t];
    *total = lds[NTH - 1];
    __syncthreads();
    return incl - v;
}

// rows[i] = id in [0, item_num] else 0 (counted in *err); key[i] = id for ids 1..item_num, else 0; val[i] = i
__global__ void __launch_bounds__(NT) id_keys_kernel(const int64_t* __restrict__ ids, int n, int item_num, int32_t* __restrict__ rows,
                                                     uint32_t* __restrict__ key, int32_t* __restrict__ val, int32_t* __restrict__ err) {
    for (int i = blockIdx.x * NT + threadIdx.x; i < n; i += gridDim.x * NT) {
        const int64_t id = ids[i];
        const bool ok = id >= 0 && id <= (int64_t)item_num;
        if (!ok) atomicAdd(err, 1);
        rows[i] = ok ? (int32_t)id : 0;
        key[i] = ok ? (uint32_t)id : 0u;
        val[i] = i;
    }
}

// ghist[d * tiles + tile] = slots of the tile whose digit (key >> shift) & 255 is d
__global__ void __launch_bounds__(NT) radix_hist_kernel(const uint32_t* __restrict__ key, int n, int shift, int32_t* __restrict__ ghist) {
    __shared__ int h[256];
    const int tiles = tiles_of(n);
    h[threadIdx.x] = 0;
    __syncthreads();
    const int i0 = blockIdx.x * TILE;
    for (int r = 0; r < ROUNDS; ++r) {
        const int i = i0 + r * NT + threadIdx.x;
        if (i < n) atomicAdd(&h[(key[i] >> shift) & 255u], 1);
    }
    __syncthreads();
    ghist[threadIdx.x * tiles + blockIdx.x] = h[threadIdx.x];
}

// in-place exclusive scan of a[0 .. m) by one workgroup.  total / ptr (optional): *total = the sum, ptr[sum] = n_end.
__global__ void __launch_bounds__(SCAN_NT) scan_excl_kernel(int32_t* __restrict__ a, int m, int32_t* __restrict__ total,
                                                            int32_t* __restrict__ ptr, int n_end) {
    __shared__ int lds[SCAN_NT];
    const int per = (m + SCAN_NT - 1) / SCAN_NT;
    const int b = threadIdx.x * per, e = min(b + per, m);
    int s = 0;
    for (int i = b; i < e; ++i) s += a[i];
    int tot;
    int run = block_excl_scan<SCAN_NT>(s, lds, &tot);
    for (int i = b; i < e; ++i) { const int v = a[i]; a[i] = run; run += v; }
    if (threadIdx.x == 0) {
        if (total) *total = tot;
        if (ptr) ptr[tot] = n_end;
    }
}

// stable scatter of one pass: slot i of the tile goes to ghist[d, tile] + (earlier slots of the tile with digit d)
__global__ void __launch_bounds__(NT) radix_scatter_kernel(const uint32_t* __restrict__ kin, const int32_t* __restrict__ vin, int n, int shift,
                                                           const int32_t* __restrict__ ghist, uint32_t* __restrict__ kout, int32_t* __restrict__ vout) {
    __shared__ int base[256], run[256], wcnt[NT / 64][256];
    const int tiles = tiles_of(n);
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    base[t] = ghist[t * tiles + blockIdx.x];
    run[t] = 0;
    for (int k = 0; k < NT / 64; ++k) wcnt[k][t] = 0;
    __syncthreads();
    const uint64_t lt_mask = lane ? (~0ull >> (64 - lane)) : 0ull;
    const int i0 = blockIdx.x * TILE;
    for (int r = 0; r < ROUNDS; ++r) {
        const int i = i0 + r * NT + t;
        const bool ok = i < n;
        uint32_t k = 0; int32_t v = 0;
        if (ok) { k = kin[i]; v = vin[i]; }
        const int d = (int)((k >> shift) & 255u);
        uint64_t peers = __ballot(ok);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const uint64_t bal = __ballot(ok && ((d >> bit) & 1));
            peers &= ((d >> bit) & 1) ? bal : ~bal;
        }
        const int rank = __popcll(peers & lt_mask);
        if (ok && rank == 0) wcnt[w][d] = __popcll(peers);
        __syncthreads();
        if (ok) {
            int off = base[d] + run[d] + rank;
            for (int k2 = 0; k2 < w; ++k2) off += wcnt[k2][d];
            kout[off] = k;
            vout[off] = v;
        }
        __syncthreads();
        int add = 0;
        for (int k2 = 0; k2 < NT / 64; ++k2) { add += wcnt[k2][t]; wcnt[k2][t] = 0; }
        run[t] += add;
        __syncthreads();
    }
}

A4R_DEV bool is_head(const uint32_t* key, int i) { return key[i] != 0u && (i == 0 || key[i - 1] != key[i]); }

// tsum[tile] = heads (first slot of a run of equal non-zero keys) in the tile; thread t owns slots t*ROUNDS .. of the tile
__global__ void __launch_bounds__(NT) heads_count_kernel(const uint32_t* __restrict__ key, int n, int32_t* __restrict__ tsum) {
    __shared__ int lds[NT];
    const int b = blockIdx.x * TILE + threadIdx.x * ROUNDS, e = min(b + ROUNDS, n);
    int c = 0;
    for (int i = b; i < e; ++i) c += is_head(key, i);
    int tot;
    block_excl_scan<NT>(c, lds, &tot);
    if (threadIdx.x == 0) tsum[blockIdx.x] = tot;
}

// list u (u-th head in slot order): uniq[u] = its id, ptr[u] = its first position in the sorted slot array
__global__ void __launch_bounds__(NT) heads_write_kernel(const uint32_t* __restrict__ key, int n, const int32_t* __restrict__ tsum,
                                                         int32_t* __restrict__ uniq, int32_t* __restrict__ ptr) {
    __shared__ int lds[NT];
    const int b = blockIdx.x * TILE + threadIdx.x * ROUNDS, e = min(b + ROUNDS, n);
    int c = 0;
    for (int i = b; i < e; ++i) c += is_head(key, i);
    int tot;
    int u = tsum[blockIdx.x] + block_excl_scan<NT>(c, lds, &tot);
    for (int i = b; i < e; ++i) {
        if (is_head(key, i)) { uniq[u] = (int32_t)key[i]; ptr[u] = i; ++u; }
    }
}

// grad[uniq[u]] += S_u for every list u < *n_uniq.  One wave per list (grid-stride over lists); the wave's lanes form 64 / G groups of G lanes,
// a group covers one E-wide row in float4 pieces.  Group g sums chunks g, g + NG, ... of the list (CHUNK rows each, sequential from 0.0f, loads
// issued ahead of the adds); after each round of NG chunks every lane adds the round's chunk sums into S in chunk order.
template <int G, int V>
__global__ void __launch_bounds__(256) id_grad_sum_kernel(const float* __restrict__ src, int ld_src, const int32_t* __restrict__ slots,
                                                          const int32_t* __restrict__ ptr, const int32_t* __restrict__ uniq,
                                                          const int32_t* __restrict__ n_uniq, float* __restrict__ grad, int ldg, int E) {
    constexpr int NG = 64 / G, CH = A4R_ID_SUM_CHUNK;
    const int lane = threadIdx.x & 63, g = lane / G, gl = lane % G;
    const int nu = *n_uniq;
    const int waves = gridDim.x * 4;
    const int pieces = E / 4;
    for (int u = blockIdx.x * 4 + (threadIdx.x >> 6); u < nu; u += waves) {
        const int p0 = ptr[u], p1 = ptr[u + 1];
        const int nch = (p1 - p0 + CH - 1) / CH;
        float4 S[V];
#pragma unroll
        for (int v = 0; v < V; ++v) S[v] = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int c0 = 0; c0 < nch; c0 += NG) {
            const int c = c0 + g;
            float4 acc[V];
#pragma unroll
            for (int v = 0; v < V; ++v) acc[v] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c < nch) {
                const int q0 = p0 + c * CH, q1 = min(q0 + CH, p1);
                int sl[CH];
#pragma unroll
                for (int j = 0; j < CH; ++j) sl[j] = q0 + j < q1 ? slots[q0 + j] : -1;
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    const int pc = gl + v * G;
                    if (pc < pieces) {
                        float4 x[CH];
#pragma unroll
                        for (int j = 0; j < CH; ++j)
                            x[j] = sl[j] >= 0 ? *reinterpret_cast<const float4*>(src + (size_t)sl[j] * ld_src + pc * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                        for (int j = 0; j < CH; ++j) {
                            if (sl[j] >= 0) { acc[v].x += x[j].x; acc[v].y += x[j].y; acc[v].z += x[j].z; acc[v].w += x[j].w; }
                        }
                    }
                }
            }
            // S += chunk c0, c0 + 1, ... in order (every group's lane gl reads group k's lane gl)
            for (int k = 0; k < NG && c0 + k < nch; ++k) {
                const int srcl = k * G + gl;
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    const float a = __shfl(acc[v].x, srcl), b = __shfl(acc[v].y, srcl), cc = __shfl(acc[v].z, srcl), d = __shfl(acc[v].w, srcl);
                    S[v].x += a; S[v].y += b; S[v].z += cc; S[v].w += d;
                }
            }
        }
        if (g == 0) {
            float* row = grad + (size_t)uniq[u] * ldg;
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const int pc = gl + v * G;
                if (pc < pieces) {
                    float4 o = *reinterpret_cast<float4*>(row + pc * 4);
                    o.x += S[v].x; o.y += S[v].y; o.z += S[v].z; o.w += S[v].w;
                    *reinterpret_cast<float4*>(row + pc * 4) = o;
                }
            }
        }
    }
}

bool misaligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }

int64_t ws_ints_of(int n) {            // keys + values of the ping-pong buffer, the [256, tiles] histogram, the per-tile head counts
    const int64_t tiles = (n + TILE - 1) / TILE;
    return 3 * (int64_t)n + 256 * tiles + tiles + 16;
}

}  // namespace

extern "C" int a4r_id_index_ws_ints(int n, int item_num) {
    if (n <= 0 || n > MAX_N || item_num <= 0 || item_num >= 0x7fffffff) return A4R_EINVAL;
    return (int)ws_ints_of(n);
}

extern "C" int a4r_id_index(void* stream, const int64_t* ids, int n, int item_num, int32_t* rows, int32_t* slots, int32_t* ptr, int32_t* uniq,
                            int32_t* n_uniq, int32_t* err, int32_t* ws, int64_t ws_ints) {
    if (!ids || !rows || !slots || !ptr || !uniq || !n_uniq || !err || !ws || n <= 0 || n > MAX_N || item_num <= 0 || item_num >= 0x7fffffff ||
        ws_ints < ws_ints_of(n))
        return A4R_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int tiles = (n + TILE - 1) / TILE;
    // workspace: key ping-pong (2 n), the value buffer the passes alternate with `slots` (n), histogram [256, tiles], tile head counts [tiles]
    uint32_t* ka = reinterpret_cast<uint32_t*>(ws);
    uint32_t* kb = ka + n;
    int32_t* vtmp = ws + 2 * (int64_t)n;
    int32_t* ghist = vtmp + n;
    int32_t* tsum = ghist + 256 * (int64_t)tiles;
    int bits = 0;
    while (bits < 31 && (item_num >> bits) != 0) ++bits;
    const int passes = (bits + 7) / 8;
    // the values alternate between vtmp and slots so that the LAST pass writes `slots`
    int32_t* va = (passes % 2) ? vtmp : slots;
    int32_t* vb = (passes % 2) ? slots : vtmp;
    if (hipMemsetAsync(err, 0, sizeof(int32_t), s) != hipSuccess) return A4R_ELAUNCH;
    int grid = (n + NT - 1) / NT; if (grid > 2048) grid = 2048;
    hipLaunchKernelGGL(id_keys_kernel, dim3(grid), dim3(NT), 0, s, ids, n, item_num, rows, ka, va, err);
    for (int p = 0; p < passes; ++p) {
        hipLaunchKernelGGL(radix_hist_kernel, dim3(tiles), dim3(NT), 0, s, (const uint32_t*)ka, n, 8 * p, ghist);
        hipLaunchKernelGGL(scan_excl_kernel, dim3(1), dim3(SCAN_NT), 0, s, ghist, 256 * tiles, (int32_t*)nullptr, (int32_t*)nullptr, 0);
        hipLaunchKernelGGL(radix_scatter_kernel, dim3(tiles), dim3(NT), 0, s, (const uint32_t*)ka, (const int32_t*)va, n, 8 * p, (const int32_t*)ghist, kb, vb);
        uint32_t* tk = ka; ka = kb; kb = tk;
        int32_t* tv = va; va = vb; vb = tv;
    }
    hipLaunchKernelGGL(heads_count_kernel, dim3(tiles), dim3(NT), 0, s, (const uint32_t*)ka, n, tsum);
    hipLaunchKernelGGL(scan_excl_kernel, dim3(1), dim3(SCAN_NT), 0, s, tsum, tiles, n_uniq, ptr, n);
    hipLaunchKernelGGL(heads_write_kernel, dim3(tiles), dim3(NT), 0, s, (const uint32_t*)ka, n, (const int32_t*)tsum, uniq, ptr);
    return a4r_launch_status();
}

extern "C" int a4r_id_grad_sum(void* stream, const float* src, int ld_src, const int32_t* slots, const int32_t* ptr, const int32_t* uniq,
                               const int32_t* n_uniq, int n, float* grad, int ldg, int E) {
    if (!src || !slots || !ptr || !uniq || !n_uniq || !grad || n <= 0 || n > MAX_N || E <= 0 || E % 4 || E > 1024 || ld_src < E || ldg < E ||
        ld_src % 4 || ldg % 4 || misaligned16(src) || misaligned16(grad))
        return A4R_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int grid = (n + 3) / 4; if (grid > 2048) grid = 2048;          // one wave per list, at most n lists (the count stays on the device)
    if (E <= 64)
        hipLaunchKernelGGL((id_grad_sum_kernel<16, 1>), dim3(grid), dim3(256), 0, s, src, ld_src, slots, ptr, uniq, n_uniq, grad, ldg, E);
    else if (E <= 128)
        hipLaunchKernelGGL((id_grad_sum_kernel<32, 1>), dim3(grid), dim3(256), 0, s, src, ld_src, slots, ptr, uniq, n_uniq, grad, ldg, E);
    else
        hipLaunchKernelGGL((id_grad_sum_kernel<64, 4>), dim3(grid), dim3(256), 0, s, src, ld_src, slots, ptr, uniq, n_uniq, grad, ldg, E);
    return a4r_launch_status();
}
