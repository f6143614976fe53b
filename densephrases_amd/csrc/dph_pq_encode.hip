// dph_pq_encode.hip -- the ADD step of the reference's index in HBM: what index.add_with_ids does behind a trained
// IndexPreTransform(OPQMatrix) -> IndexIVFPQ (build_phrase_index.py:145-153; add_to_index :156-279 feeds it dump rows).  gfx950 only.
//
//   x'       = A x (+ b)                                   pq_transform_kernel (dph_pq.hip), reused as it is
//   list     = arg-max_l <x', c_l>, float64 order          dph_launch_assign (fused MFMA estimate + gap) + pqe_relist_kernel (rows inside the
//                                                          fp32 error band, exact ties and all-zero rows: float64 over every list)
//   r        = fp32(x' - c_list)  (by_residual)            one fp32 subtraction while the rows are staged (pqe_codes_kernel)
//   code[m]  = arg-min_j ||w_mj||^2 - 2 <r_m, w_mj>        pqe_codes_kernel: fp32 MFMA estimate, best + runner-up per (row, m); a cell whose gap is
//                                                          inside the error bound of its dot is re-decided in float64 by the wave that holds it
//   lists    = stable order by (list, input position)      pqe_fill_keys_kernel + radix sort (dph_sort_pairs_i64_u32) + pqe_fill_gather_kernel
//
// The host half (scratch, chunking, the handle's state) is in dph_pq.hip: dph_pq_encode / dph_pq_fill.
#include <float.h>
#include <math.h>

#include <algorithm>

#include "dph_internal.h"

typedef float v16f __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------------------------- list of a row
// One workgroup per row.  A row the transform flagged non-finite gets list -1.  A row whose fp32 gap is above the band keeps the list of
// the MFMA estimate; every other row -- `!(gap > band)`, so gap 0 (exact ties, the all-zero row) and a NaN gap are inside -- is scored
// against ALL lists in float64, products and sums sequential in t, the largest score winning, ties to the lowest list.
//   band = 4 * 1.5 * 768 * 2^-24 * ||x'|| * max||c||: each fp32 score is off by at most 768 * 2^-24 * ||x'|| ||c|| (a chain of 768 fmaf), a gap
//   compares two of them, and the remaining factor 3 is the slack ivf.assign_lists_resident carries (same constant, 5.97e-8 for 2^-24).
#define PQE_BAND_COEF (4.0 * 1.5 * 768.0 * 5.97e-8)
__global__ __launch_bounds__(256) void pqe_relist_kernel(const float* __restrict__ xp, int64_t n, const float* __restrict__ cent, int nlist,
                                                         const int32_t* __restrict__ nonfinite, const float* __restrict__ gap, double cnorm_max,
                                                         int32_t* __restrict__ list) {
    __shared__ double xs[DPH_DIM];
    __shared__ double red_v[256];
    __shared__ int red_i[256];
    const int tid = threadIdx.x;
    for (int64_t r = blockIdx.x; r < n; r += gridDim.x) {
        __syncthreads();                                    // xs / red_* of the previous row are done with
        if (nonfinite[r]) {                                 // (block-uniform)
            if (tid == 0) list[r] = -1;
            continue;
        }
        double ss = 0.0;
        for (int t = tid; t < DPH_DIM; t += 256) {
            const double v = (double)xp[r * DPH_DIM + t];
            xs[t] = v;
            ss += v * v;
        }
        red_v[tid] = ss;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) red_v[tid] += red_v[tid + o];
            __syncthreads();
        }
        const double band = PQE_BAND_COEF * cnorm_max * sqrt(red_v[0]);
        __syncthreads();                                    // everyone has read red_v[0]
        if ((double)gap[r] > band) continue;                // (block-uniform) the estimate stands
        double best = -DBL_MAX;
        int bl = 0x7fffffff;
        for (int l = tid; l < nlist; l += 256) {
            const float4* c = (const float4*)(cent + (int64_t)l * DPH_DIM);
            double acc = 0.0;
            for (int t4 = 0; t4 < DPH_DIM / 4; ++t4) {
                const float4 cv = c[t4];
                acc += (double)cv.x * xs[4 * t4];           // (a product of two fp32 values is exact in float64: only the sums round)
                acc += (double)cv.y * xs[4 * t4 + 1];
                acc += (double)cv.z * xs[4 * t4 + 2];
                acc += (double)cv.w * xs[4 * t4 + 3];
            }
            if (acc > best || bl == 0x7fffffff) { best = acc; bl = l; }      // l ascends: a tie keeps the lower list
        }
        red_v[tid] = best;
        red_i[tid] = bl;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) {
                const double ov = red_v[tid + o];
                const int oi = red_i[tid + o];
                const int mi = red_i[tid];
                if (oi != 0x7fffffff && (mi == 0x7fffffff || ov > red_v[tid] || (ov == red_v[tid] && oi < mi))) { red_v[tid] = ov; red_i[tid] = oi; }
            }
            __syncthreads();
        }
        if (tid == 0) list[r] = red_i[0];
    }
}

void dph_launch_pq_relist(const float* xp, int64_t n, const float* cent, int nlist, const int32_t* nonfinite, const float* gap, double cnorm_max,
                          int32_t* list, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(pqe_relist_kernel, dim3((unsigned)std::min<int64_t>(n, 1 << 20)), dim3(256), 0, st, xp, n, cent, nlist, nonfinite, gap, cnorm_max,
                       list);
}

// ---------------------------------------------------------------------------------------------- codes
// A workgroup of 4 waves owns 128 rows (wave w rows 32 w .. 32 w + 31) and walks the sub-quantisers in steps of G: a step stages the G
// codebooks [256][dsub] and their biases, and columns [m0 dsub, (m0 + G) dsub) of the 128 residual rows (the subtraction x' - c_list happens
// here: the residual is never written), through LDS.  Per sub-quantiser a wave computes s[j][row] = bias[j] + <w_j, r_m> for its 32 rows and
// the 256 codewords in 8 tiles of v_mfma_f32_32x32x2_f32 -- A = codewords (i), B = rows (j = lane & 31), the accumulator starts at the bias
// bias[j] = fp32(-||w_j||^2 / 2), so arg-max s = arg-min ||w||^2 - 2 <r, w>.  The MFMA's k is 2 and every dsub (6, 8, 12, 16, 24, 48) is
// even: no k-step is padded.  Row strides in LDS are odd, so the 32 lanes of a ds_read_b32 group hit 32 different banks.
//
// Error bound of a score.  The MFMA result is the fp32 chain s^_0 = fl(b), s^_k = fma(w_k, r_k, s^_{k-1}), k = 1 .. dsub: dsub + 1 roundings
// (the bias once, one per fma), each relative 2^-24 to a partial sum that never exceeds |b| + sum |w_k r_k| (1 + o(1)).  Hence
//   | s^ - s | <= gamma_{dsub+1} (||w||^2 / 2 + sum_k |w_k| |r_k|) <= gamma_{dsub+1} (||w||^2 / 2 + ||r_m|| ||w||),   gamma_k = k 2^-24 / (1 - k 2^-24),
// and with W = max_j ||w_mj|| (rounded up on the host) one bound serves all 256 codewords of m:
//   E(row, m) = PQE_SLACK (dsub + 1) 2^-24 (||r_m|| W + W^2 / 2);
// PQE_SLACK = 1.5 pays for gamma's denominator and for ||r_m|| being an fp32 sum itself.  If s^_1 - s^_2 > 2 E then s_1 - E > s_2 + E and every
// third codeword lies below the runner-up: the estimate's winner is the float64 winner.  Every other cell -- `!(gap > 2 E)`: exact ties
// between duplicate codewords, E = inf of an overflowing norm, a NaN gap -- is re-decided where it is: the wave's 64 lanes take 4 codewords
// each, d_j = ||w_j||^2 - 2 <r_m, w_j> in float64 with products and sums sequential in t, arg-min over the wave, ties to the lowest j.
// No list of such cells is kept: however many there are (a fifth of all cells on an index with duplicated codewords), each costs its wave
// 4 dsub float64 multiply-adds per lane and nothing can overflow.
#define PQE_ROWS 128
#define PQE_SLACK 1.5f
template <int DSUB> struct pqe_geo {
    static constexpr int GW = DSUB <= 12 ? 24 : DSUB;       // floats of a row staged per step
    static constexpr int G = GW / DSUB;                     // sub-quantisers per step: 4, 3, 2, 1, 1, 1
    static constexpr int CLD = DSUB + 1;                    // LDS stride of a codeword (odd)
    static constexpr int RLD = GW + 1;                      // LDS stride of a row (odd)
    static constexpr size_t cw_floats = (size_t)G * 256 * CLD;
    static constexpr size_t lds(int M) { return (cw_floats + (size_t)G * 256 + (size_t)PQE_ROWS * RLD + PQE_ROWS) * 4 + (size_t)PQE_ROWS * M; }
};

template <int DSUB>
__global__ __launch_bounds__(256) void pqe_codes_kernel(const float* __restrict__ xp, int64_t n, const int32_t* __restrict__ list,
                                                        const float* __restrict__ cent, int by_residual, const float* __restrict__ pqc,
                                                        const float* __restrict__ bias, const float* __restrict__ wmax, int M,
                                                        uint8_t* __restrict__ codes) {
    using geo = pqe_geo<DSUB>;
    constexpr int G = geo::G, GW = geo::GW, CLD = geo::CLD, RLD = geo::RLD;
    extern __shared__ __attribute__((aligned(16))) unsigned char pqe_smem[];
    float* cw_s = (float*)pqe_smem;                                     // [G][256][CLD]
    float* bias_s = cw_s + geo::cw_floats;                              // [G][256]
    float* r_s = bias_s + G * 256;                                      // [128][RLD]
    int* list_s = (int*)(r_s + PQE_ROWS * RLD);                         // [128] list of the row, -1 = no row here / non-finite
    uint8_t* code_s = (uint8_t*)(list_s + PQE_ROWS);                    // [128][M]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, col = lane & 31;
    const int64_t r0 = (int64_t)blockIdx.x * PQE_ROWS;
    if (tid < PQE_ROWS) list_s[tid] = r0 + tid < n ? list[r0 + tid] : -1;
    for (int m0 = 0; m0 < M; m0 += G) {
        __syncthreads();                                                // the previous step's readers are done (and list_s is written)
        {
            const float2* src = (const float2*)(pqc + (size_t)m0 * 256 * DSUB);
            for (int e = tid; e < G * 256 * DSUB / 2; e += 256) {
                const float2 v = src[e];
                const int cw = (2 * e) / DSUB, t = (2 * e) % DSUB;      // (DSUB is even: a pair never straddles two codewords)
                cw_s[cw * CLD + t] = v.x;
                cw_s[cw * CLD + t + 1] = v.y;
            }
            for (int e = tid; e < G * 256; e += 256) bias_s[e] = bias[(size_t)m0 * 256 + e];
            for (int e = tid; e < PQE_ROWS * GW / 2; e += 256) {
                const int row = e / (GW / 2), c2 = e % (GW / 2);
                const int l = list_s[row];
                float2 v = make_float2(0.f, 0.f);
                if (l >= 0) {
                    v = *(const float2*)(xp + (r0 + row) * DPH_DIM + m0 * DSUB + 2 * c2);
                    if (by_residual) {
                        const float2 c = *(const float2*)(cent + (int64_t)l * DPH_DIM + m0 * DSUB + 2 * c2);
                        v.x = __fsub_rn(v.x, c.x);
                        v.y = __fsub_rn(v.y, c.y);
                    }
                }
                r_s[row * RLD + 2 * c2] = v.x;
                r_s[row * RLD + 2 * c2 + 1] = v.y;
            }
        }
        __syncthreads();
#pragma unroll 1
        for (int g = 0; g < G; ++g) {
            const float* rrow = r_s + (wave * 32 + col) * RLD + g * DSUB;
            float bq[DSUB / 2];
            float rn2 = 0.f;
#pragma unroll
            for (int k = 0; k < DSUB / 2; ++k) { bq[k] = rrow[2 * k + half]; rn2 = fmaf(bq[k], bq[k], rn2); }
            rn2 += __shfl_xor(rn2, 32);
            float b1 = -FLT_MAX, b2 = -FLT_MAX;
            int i1 = 0;
            const float* cwg = cw_s + (size_t)g * 256 * CLD + col * CLD + half;
            const float* bg = bias_s + g * 256 + 4 * half;
#pragma unroll 2
            for (int T = 0; T < 8; ++T) {
                v16f acc;
                // C[i = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)][j = lane & 31]: i = codeword inside the tile, j = row
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 bv = *(const float4*)(bg + T * 32 + 8 * q);
                    acc[4 * q] = bv.x; acc[4 * q + 1] = bv.y; acc[4 * q + 2] = bv.z; acc[4 * q + 3] = bv.w;
                }
                const float* ap = cwg + T * 32 * CLD;
#pragma unroll
                for (int k = 0; k < DSUB / 2; ++k) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * k], bq[k], acc, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int j = T * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                    const float v = acc[r];
                    if (v > b1) { b2 = b1; b1 = v; i1 = j; }
                    else b2 = fmaxf(b2, v);
                }
            }
            {   // the other lane half holds the same row's other codewords
                const float ob1 = __shfl_xor(b1, 32), ob2 = __shfl_xor(b2, 32);
                const int oi1 = __shfl_xor(i1, 32);
                if (ob1 > b1 || (ob1 == b1 && oi1 < i1)) { b2 = fmaxf(b1, ob2); b1 = ob1; i1 = oi1; }
                else b2 = fmaxf(b2, ob1);
            }
            const float W = wmax[m0 + g];
            const float E = PQE_SLACK * (float)(DSUB + 1) * 5.9604645e-8f * (sqrtf(rn2) * W + 0.5f * W * W);
            const bool redo = !(b1 - b2 > 2.f * E);
            int code = i1;
            unsigned long long todo = __ballot(redo && half == 0);
            while (todo) {                                              // (wave-uniform)
                const int rr = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const float* rv = r_s + (wave * 32 + rr) * RLD + g * DSUB;
                double bd = 0.0;
                int bj = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int j = lane + 64 * q;
                    const float* w = cw_s + ((size_t)g * 256 + j) * CLD;
                    double nw = 0.0, dot = 0.0;
                    for (int t = 0; t < DSUB; ++t) {
                        const double wt = (double)w[t];
                        nw += wt * wt;                                  // (exact products: see pqe_relist_kernel)
                        dot += (double)rv[t] * wt;
                    }
                    const double d = nw - 2.0 * dot;
                    if (q == 0 || d < bd) { bd = d; bj = j; }           // j ascends: a tie keeps the lower codeword
                }
                for (int o = 32; o > 0; o >>= 1) {
                    const double od = __shfl_xor(bd, o);
                    const int oj = __shfl_xor(bj, o);
                    if (od < bd || (od == bd && oj < bj)) { bd = od; bj = oj; }
                }
                if (col == rr) code = bj;
            }
            if (half == 0) code_s[(wave * 32 + col) * M + m0 + g] = (uint8_t)code;
        }
    }
    __syncthreads();
    // 128 x M code bytes out, 4 at a time (M is a multiple of 16); a row without a list (non-finite) gets zero codes
    const int wpr = M / 4;
    for (int e = tid; e < PQE_ROWS * wpr; e += 256) {
        const int row = e / wpr;
        if (r0 + row < n) ((unsigned*)(codes + (r0 + row) * M))[e % wpr] = list_s[row] >= 0 ? ((const unsigned*)code_s)[e] : 0u;
    }
}

template <int DSUB>
static void pqe_launch_codes(const float* xp, int64_t n, const int32_t* list, const float* cent, int by_residual, const float* pqc, const float* bias,
                             const float* wmax, int M, uint8_t* codes, int device, hipStream_t st) {
    const size_t lds = pqe_geo<DSUB>::lds(M);
    static_assert(pqe_geo<DSUB>::lds(128) <= 160 * 1024, "a step's codebooks, rows and the code bytes must fit the LDS of a CU");
    DPH_ALLOW_LDS(pqe_codes_kernel<DSUB>, pqe_geo<DSUB>::lds(128), device);
    hipLaunchKernelGGL(pqe_codes_kernel<DSUB>, dim3((unsigned)((n + PQE_ROWS - 1) / PQE_ROWS)), dim3(256), lds, st, xp, n, list, cent, by_residual, pqc, bias,
                       wmax, M, codes);
}

int dph_launch_pq_codes(const float* xp, int64_t n, const int32_t* list, const float* cent, int by_residual, const float* pqc, const float* bias,
                        const float* wmax, int M, uint8_t* codes, int device, hipStream_t st) {
    if (n <= 0) return 0;
    switch (DPH_DIM / M) {
        case 6: pqe_launch_codes<6>(xp, n, list, cent, by_residual, pqc, bias, wmax, M, codes, device, st); return 0;
        case 8: pqe_launch_codes<8>(xp, n, list, cent, by_residual, pqc, bias, wmax, M, codes, device, st); return 0;
        case 12: pqe_launch_codes<12>(xp, n, list, cent, by_residual, pqc, bias, wmax, M, codes, device, st); return 0;
        case 16: pqe_launch_codes<16>(xp, n, list, cent, by_residual, pqc, bias, wmax, M, codes, device, st); return 0;
        case 24: pqe_launch_codes<24>(xp, n, list, cent, by_residual, pqc, bias, wmax, M, codes, device, st); return 0;
        case 48: pqe_launch_codes<48>(xp, n, list, cent, by_residual, pqc, bias, wmax, M, codes, device, st); return 0;
    }
    return 1;                                                           // (dph_pq_alloc admits no other M)
}

// ---------------------------------------------------------------------------------------------- the list builder
// keys (list << 32 | input position) and the identity permutation, the size of every list, and a flag for a list outside [0, nlist)
__global__ __launch_bounds__(256) void pqe_fill_keys_kernel(const int32_t* __restrict__ list, int64_t n, int nlist, int64_t* __restrict__ keys,
                                                            unsigned* __restrict__ vals, unsigned* __restrict__ counts, int* __restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int l = list[i];
    vals[i] = (unsigned)i;
    if (l < 0 || l >= nlist) { *bad = 1; keys[i] = (int64_t)i; return; }
    keys[i] = ((int64_t)l << 32) | i;
    atomicAdd(&counts[l], 1u);
}
// position p of the list-major order takes the codes (16 bytes per thread) and the id of input row src[p]
__global__ __launch_bounds__(256) void pqe_fill_gather_kernel(const unsigned* __restrict__ src, int64_t n, int M, const uint8_t* __restrict__ codes_in,
                                                              const int64_t* __restrict__ ids_in, uint8_t* __restrict__ codes_out,
                                                              int64_t* __restrict__ ids_out) {
    const int per = M / 16;
    const int64_t total = n * per;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t p = e / per;
        const int c = (int)(e % per);
        const int64_t s = src[p];
        ((uint4*)(codes_out + p * M))[c] = ((const uint4*)(codes_in + s * M))[c];
        if (c == 0) ids_out[p] = ids_in[s];
    }
}

void dph_launch_pq_fill_keys(const int32_t* list, int64_t n, int nlist, int64_t* keys, unsigned* vals, unsigned* counts, int* bad, hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(pqe_fill_keys_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, list, n, nlist, keys, vals, counts, bad);
}
void dph_launch_pq_fill_gather(const unsigned* src, int64_t n, int M, const uint8_t* codes_in, const int64_t* ids_in, uint8_t* codes_out, int64_t* ids_out,
                               hipStream_t st) {
    if (n <= 0) return;
    const int64_t blocks = (n * (M / 16) + 255) / 256;
    hipLaunchKernelGGL(pqe_fill_gather_kernel, dim3((unsigned)std::min<int64_t>(blocks, 1 << 20)), dim3(256), 0, st, src, n, M, codes_in, ids_in, codes_out,
                       ids_out);
}
