// dph_pq_train.hip -- one Lloyd iteration of the M sub-space quantisers of a product quantiser, in HBM: the inner step of what
// index.train does behind IndexPreTransform(OPQMatrix) -> IndexIVFPQ (build_phrase_index.py:96-142: OPQ alternation, then the PQ of the
// residuals).  gfx950 only.  The alternation around it is densephrases_amd/pq_train.py.
//
//   bias, wmax = fp32(-||w_mj||^2 / 2), max_j ||w_mj|| (up)   pqt_bias_kernel: what dph_pq_set_params computes on the host, for the CURRENT codebooks
//   code[r][m] = arg-min_j ||w_mj||^2 - 2 <x_rm, w_mj>        dph_launch_pq_codes (dph_pq_encode.hip) with by_residual = 0, as it is: the float64
//                                                             arg-min, ties to the lowest j
//   e[r]       = sum_t (x[r][t] - w[code][t])^2               pqt_row_err_kernel: float64, t ascending, one thread per row
//   w_mj       = fp32(sum_{r: code[r][m] = j} x_rm / count)   pqt_keys_kernel + radix sort of ((m 256 + j) << 32 | r) + pqt_update_kernel: the
//                                                             float64 sum of the members IN ASCENDING ROW ORDER, one thread per (m, j, t) chain
//   y[r]       = concat_m w[m][code[r][m]]                    pqt_decode_kernel
//
// Every output is a pure function of the inputs: no float atomics, no order left to the scheduler (the counts are integer atomics).
#include <math.h>

#include <algorithm>

#include "dph_internal.h"

// ---------------------------------------------------------------------------------------------- the encoder's view of the codebooks
// One workgroup per m, thread j: ||w_mj||^2 in float64, sequential in t (products of two fp32 values are exact in float64: only the sums
// round, fused or not); wmax[m] rounded up like the host's (it bounds an error).
__global__ __launch_bounds__(256) void pqt_bias_kernel(const float* __restrict__ pqc, int dsub, float* __restrict__ bias, float* __restrict__ wmax) {
    __shared__ double red[256];
    const int m = blockIdx.x, j = threadIdx.x;
    const float* w = pqc + ((size_t)m * 256 + j) * dsub;
    double nw = 0.0;
    for (int t = 0; t < dsub; ++t) nw += (double)w[t] * (double)w[t];
    bias[(size_t)m * 256 + j] = (float)(-0.5 * nw);
    red[j] = nw;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (j < o) red[j] = fmax(red[j], red[j + o]);
        __syncthreads();
    }
    if (j == 0) wmax[m] = nextafterf((float)(sqrt(red[0]) * (1.0 + 1e-6)), INFINITY);
}

// ---------------------------------------------------------------------------------------------- row error
// e[r] = sum over t = 0 .. 767 of (x - y)^2, every operation a float64 operation of its own (no fused multiply-add: the restatement has none)
__global__ __launch_bounds__(256) void pqt_row_err_kernel(const float* __restrict__ x, int64_t n, const uint8_t* __restrict__ codes, int M, int dsub,
                                                          const float* __restrict__ pqc, double* __restrict__ err) {
#pragma clang fp contract(off)
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const float2* xr = (const float2*)(x + r * DPH_DIM);
    double e = 0.0;
    for (int m = 0; m < M; ++m) {
        const float2* w = (const float2*)(pqc + ((size_t)m * 256 + codes[r * M + m]) * dsub);
        const float2* xm = xr + m * (dsub / 2);
        for (int t2 = 0; t2 < dsub / 2; ++t2) {                         // (dsub is even)
            const float2 xv = xm[t2], wv = w[t2];
            const double d0 = (double)xv.x - (double)wv.x, d1 = (double)xv.y - (double)wv.y;
            e = e + d0 * d0;
            e = e + d1 * d1;
        }
    }
    err[r] = e;
}

// ---------------------------------------------------------------------------------------------- update
// keys ((m 256 + j) << 32 | r), the row again as the sort's value, and the size of every (m, j)
__global__ __launch_bounds__(256) void pqt_keys_kernel(const uint8_t* __restrict__ codes, int64_t n, int M, int64_t* __restrict__ keys,
                                                       unsigned* __restrict__ vals, unsigned* __restrict__ counts, int want_keys) {
    const int64_t total = n * M;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t r = e / M;
        const int cell = (int)(e - r * M) * 256 + codes[e];
        if (want_keys) {
            keys[e] = ((int64_t)cell << 32) | r;
            vals[e] = (unsigned)r;
        }
        atomicAdd(&counts[cell], 1u);
    }
}
// One thread per (m, j, t): its segment of the sorted order starts at the first key >= (m 256 + j) << 32 and holds counts[m][j] rows,
// ascending.  An empty codeword keeps its value.
__global__ __launch_bounds__(256) void pqt_update_kernel(const float* __restrict__ x, const int64_t* __restrict__ keys, const unsigned* __restrict__ rows,
                                                         int64_t total, const unsigned* __restrict__ counts, int dsub, float* __restrict__ pqc) {
    const int g = blockIdx.x * 256 + threadIdx.x;                       // [M][256][dsub] = 256 * 768 threads
    if (g >= 256 * DPH_DIM) return;
    const int cell = g / dsub, t = g - cell * dsub, m = cell >> 8;
    const unsigned cnt = counts[cell];
    if (cnt == 0) return;
    const int64_t first = (int64_t)cell << 32;
    int64_t lo = 0, hi = total;
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (keys[mid] < first) lo = mid + 1; else hi = mid; }
    const float* col = x + m * dsub + t;
    double s = 0.0;
    for (unsigned i = 0; i < cnt; ++i) s += (double)col[(int64_t)rows[lo + i] * DPH_DIM];
    pqc[g] = (float)(s / (double)cnt);
}

// ---------------------------------------------------------------------------------------------- decode
// two floats per thread (dsub is even: a pair never straddles two codewords)
__global__ __launch_bounds__(256) void pqt_decode_kernel(const uint8_t* __restrict__ codes, int64_t n, int M, int dsub, const float* __restrict__ pqc,
                                                         float* __restrict__ y) {
    const int64_t total = n * (DPH_DIM / 2);
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t r = e / (DPH_DIM / 2);
        const int c = 2 * (int)(e - r * (DPH_DIM / 2)), m = c / dsub, t = c - m * dsub;
        ((float2*)y)[e] = *(const float2*)(pqc + ((size_t)m * 256 + codes[r * M + m]) * dsub + t);
    }
}

// ---------------------------------------------------------------------------------------------- entry points
static bool pqt_m_ok(int M) { return M > 0 && DPH_DIM % M == 0 && M % 16 == 0 && M <= 128; }          // what dph_pq_alloc admits

int dph_pq_train_step_dev(int device, const float* x_dev, int64_t n, int M, float* pq_centroids_dev, uint8_t* codes_dev, uint32_t* counts_dev,
                          double* row_err_dev, int update, void* stream) {
    if (!x_dev || !pq_centroids_dev || !codes_dev || !counts_dev) return fail(DPH_E_ARG, "dph_pq_train_step_dev: null pointer");
    if (n <= 0 || n >= ((int64_t)1 << 31)) return fail(DPH_E_ARG, "dph_pq_train_step_dev: need 0 < n < 2^31 rows");
    if (!pqt_m_ok(M)) return fail(DPH_E_ARG, "dph_pq_train_step_dev: M must be a multiple of 16 that divides 768, M <= 128");
    if (((uintptr_t)x_dev & 15u) || ((uintptr_t)codes_dev & 15u) || ((uintptr_t)pq_centroids_dev & 15u))
        return fail(DPH_E_ARG, "dph_pq_train_step_dev: x, the codebooks and codes must be 16-byte aligned");
    HIPCHK(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    const int dsub = DPH_DIM / M;
    const int64_t total = n * M;
    dev_buf<float> bias, wmax;
    dev_buf<int32_t> list;                                              // all zero: every row is a row (dph_launch_pq_codes reads -1 as "none")
    HIPCHK(bias.alloc((size_t)M * 256)); HIPCHK(wmax.alloc((size_t)M)); HIPCHK(list.alloc((size_t)n));
    HIPCHK(hipMemsetAsync(list, 0, (size_t)n * 4, st));
    HIPCHK(hipMemsetAsync(counts_dev, 0, (size_t)M * 256 * 4, st));
    hipLaunchKernelGGL(pqt_bias_kernel, dim3(M), dim3(256), 0, st, pq_centroids_dev, dsub, bias, wmax);
    if (dph_launch_pq_codes(x_dev, n, list, nullptr, 0, pq_centroids_dev, bias, wmax, M, codes_dev, device, st))
        return fail(DPH_E_ARG, "dph_pq_train_step_dev: no kernel for this M");
    if (row_err_dev)
        hipLaunchKernelGGL(pqt_row_err_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x_dev, n, codes_dev, M, dsub, pq_centroids_dev, row_err_dev);
    dev_buf<int64_t> keys, keys_sorted;
    dev_buf<unsigned> vals, vals_sorted;
    if (update) {
        HIPCHK(keys.alloc((size_t)total)); HIPCHK(keys_sorted.alloc((size_t)total));
        HIPCHK(vals.alloc((size_t)total)); HIPCHK(vals_sorted.alloc((size_t)total));
    }
    hipLaunchKernelGGL(pqt_keys_kernel, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 1 << 16)), dim3(256), 0, st, codes_dev, n, M, keys, vals,
                       counts_dev, update ? 1 : 0);
    HIPCHK(hipGetLastError());
    if (update) {
        if (dph_sort_pairs_i64_u32(keys, vals, keys_sorted, vals_sorted, total, st)) return fail(DPH_E_HIP, "dph_pq_train_step_dev: sorting by (m, code, row) failed");
        hipLaunchKernelGGL(pqt_update_kernel, dim3(DPH_DIM), dim3(256), 0, st, x_dev, keys_sorted, vals_sorted, total, counts_dev, dsub, pq_centroids_dev);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(st));                                   // the scratch dies with this call
    return DPH_OK;
}

int dph_pq_decode_dev(int device, const uint8_t* codes_dev, int64_t n, int M, const float* pq_centroids_dev, float* y_dev, void* stream) {
    if (!codes_dev || !pq_centroids_dev || !y_dev) return fail(DPH_E_ARG, "dph_pq_decode_dev: null pointer");
    if (n <= 0 || n >= ((int64_t)1 << 31)) return fail(DPH_E_ARG, "dph_pq_decode_dev: need 0 < n < 2^31 rows");
    if (!pqt_m_ok(M)) return fail(DPH_E_ARG, "dph_pq_decode_dev: M must be a multiple of 16 that divides 768, M <= 128");
    if (((uintptr_t)y_dev & 7u) || ((uintptr_t)pq_centroids_dev & 7u)) return fail(DPH_E_ARG, "dph_pq_decode_dev: y and the codebooks must be 8-byte aligned");
    HIPCHK(hipSetDevice(device));
    const int64_t blocks = (n * (DPH_DIM / 2) + 255) / 256;
    hipLaunchKernelGGL(pqt_decode_kernel, dim3((unsigned)std::min<int64_t>(blocks, 1 << 20)), dim3(256), 0, (hipStream_t)stream, codes_dev, n, M,
                       DPH_DIM / M, pq_centroids_dev, y_dev);
    HIPCHK(hipGetLastError());
    return DPH_OK;
}
