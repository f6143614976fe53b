// dph_pq.hip -- the reference's OWN index type served from HBM: IndexPreTransform(OPQMatrix) -> IndexIVFPQ (inner product,
// by_residual, 8-bit codes) as build_phrase_index.py:108-116 trains it and index.py:30-33,200,286 uses it (SURVEY.md 8 row
// a3 / f2, BASELINE.json north_star "(or PQ-compressed)").  gfx950 only.
//
//   x'          = A x (+ b)                                   pq_transform_kernel      (float64 accumulation, one rounding)
//   coarse      = top-nprobe lists by <x', c_l>               dph_launch_coarse        (f32 MFMA GEMM + radix select + float64 band re-rank)
//   LUT[m][j]   = <x'_m, codeword[m][j]>                      pq_lut_kernel            (float64 accumulation, one rounding)
//   score(code) = <x', c_list> + sum_m LUT[m][code[m]]        pq_adc_kernel            (fp32, summed SEQUENTIALLY in m like FAISS' scalar scan)
//   top-k       = k largest, (score desc, id asc)             pq_adc_kernel + pq_final_kernel
//   reconstruct = c_list + concat_m codeword[m][code[m]]      pq_reconstruct_kernel / window_kernel<PqCodes> (dph_window.hip)
//   windows over the dump's raw int8 rows (HDF5 branch)       window_kernel<DocRows>   (dph_index_attach_doc_rows)
//
// ADC scan.  Work = (query row, probed list) pairs from the coarse probe masks, taken from a work queue by workgroups of
// 1024 threads.  A workgroup keeps the row's LUT in LDS (M x 256 fp32 = 96 KiB at OPQ96) and walks the list in segments of
// PQ_SEG codes: every thread sums its codes (16-byte loads of the code bytes, one LDS gather per sub-quantiser), the
// segment's scores go to LDS as order-preserving uint32 keys, a 4-pass radix select finds the segment's k-th largest, and
// only keys >= max(that, the row's running bound) are appended to the row's candidate list in HBM; the row's bound is
// raised with atomicMax.  The bound is always the k-th largest of SOME subset of the row's scores, i.e. a lower bound of
// the true k-th best, so no member of the true top-k is ever dropped.  pq_final_kernel selects the k best candidates of a
// row exactly (radix select over its candidate list, then a sort of the survivors by (score desc, id asc)).
// LDS gathers with random codes hit ~4-way bank conflicts: the kernel is LDS-gather-bound, the roofline DESIGN.md prices
// it against is M gathers per code at 64 lanes x 1 gather / (conflict factor) per clock per CU.
#include <float.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "dph_internal.h"
#include "dph_plan.h"

// (PQ_THREADS, PQ_SEG, PQ_FINAL_CAP, PQ_LM_CHUNK, PQ_GROUP: dph_geometry.h -- the capacity rules of dph_plan.h are made of them)

__device__ __forceinline__ unsigned pq_key(float s) {
    const unsigned b = __float_as_uint(s);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);          // larger float <=> larger key; key 0 is below every score
}
__device__ __forceinline__ float pq_unkey(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// ---------------------------------------------------------------------------------------------- x' = A x (+ b)
// At = A transposed ([d_in][d_out]): lane j walks column j, coalesced over the lanes, t ascending
// out_hi / out_pk (optional): the row once more as bf16 and as packed bf16 hi << 16 | lo -- the operands of the coarse quantizer's
// filter and of its bf16x3 fail-over chain (dph_ivf.hip), written here instead of by two more launches
__device__ __forceinline__ unsigned short pq_bf16_rne(float v) {
    const unsigned u = __float_as_uint(v);
    return (unsigned short)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
// grid (ceil(rows / 8), DPH_DIM / 64) x 256 threads: a workgroup owns 8 rows x 64 output columns -- wave w rows 2w, 2w + 1, lane =
// column.  The 64 x 64 block of A^T of a step is loaded ONCE per workgroup (16 values per thread, coalesced), converted to float64
// once and shared through LDS (two buffers, one barrier per step); the blocks of the next three steps are in flight in registers.
// One column of one row per thread (rounds 1-4) read all of A per row -- 302 MB through the L2 for 128 rows, 28-38 us however
// the loads were batched -- and converted both factors of every term.  Same arithmetic: fma(double(A_jt), double(x_t), acc), t
// ascending, one rounding to float at the end.
#define PQT_ROWS 8
#define PQT_COLS 64
#define PQT_TB 64
__global__ __launch_bounds__(256) void pq_transform_kernel(const float* __restrict__ x, const float* __restrict__ At, int64_t n_rows,
                                                           const float* __restrict__ b, float* __restrict__ out,
                                                           unsigned short* __restrict__ out_hi = nullptr, unsigned* __restrict__ out_pk = nullptr,
                                                           int32_t* __restrict__ nonfinite = nullptr) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pqt_smem[];
    __shared__ int pqt_bad[PQT_ROWS];
    double (*xs)[DPH_DIM] = (double (*)[DPH_DIM])pqt_smem;                                       // [PQT_ROWS][768]
    double (*as_)[PQT_TB][PQT_COLS] = (double (*)[PQT_TB][PQT_COLS])(pqt_smem + sizeof(double) * PQT_ROWS * DPH_DIM);   // [2][64][64]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * PQT_ROWS;
    const int j = blockIdx.y * PQT_COLS + lane;
    constexpr int NST = DPH_DIM / PQT_TB, RING = 4, PER = PQT_TB / 4;          // 12 steps; a thread loads PER = 16 values of a step's block
    float ring[RING][PER];
    auto issue = [&](int st, float (&dst)[PER]) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < PER; ++i) dst[i] = At[(int64_t)(st * PQT_TB + wave * PER + i) * DPH_DIM + j];
    };
    auto stage = [&](int st, const float (&src)[PER]) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < PER; ++i) as_[st & 1][wave * PER + i][lane] = (double)src[i];
    };
    if (At) {
#pragma unroll
        for (int st = 0; st < RING - 1; ++st) issue(st, ring[st]);
    }
    {
        float xr[PQT_ROWS][DPH_DIM / 256];                 // the 8 rows, all 24 loads of a thread in flight together
#pragma unroll
        for (int rr = 0; rr < PQT_ROWS; ++rr)
#pragma unroll
            for (int q = 0; q < DPH_DIM / 256; ++q) xr[rr][q] = x[(r0 + rr < n_rows ? r0 + rr : n_rows - 1) * DPH_DIM + tid + 256 * q];      // (a row past the end: the last row again, never stored)
        if (nonfinite) {
            // a row with a NaN / Inf element (search only: `nonfinite` set): flagged, searched as a bounded stand-in pattern so that the
            // coarse filter and the ADC scan see ordinary numbers (a NaN estimate fails the filter and sends the WHOLE pass down the
            // bf16x3 chain), answered with -1 / -FLT_MAX / status DPH_ROW_NONFINITE by pq_final_kernel -- what FAISS returns for it
            if (tid < PQT_ROWS) pqt_bad[tid] = 0;
            __syncthreads();
#pragma unroll
            for (int rr = 0; rr < PQT_ROWS; ++rr) {
                bool ok = true;
#pragma unroll
                for (int q = 0; q < DPH_DIM / 256; ++q) ok = ok && isfinite(xr[rr][q]);
                if (!ok) pqt_bad[rr] = 1;
            }
            __syncthreads();
#pragma unroll
            for (int rr = 0; rr < PQT_ROWS; ++rr) {
                if (pqt_bad[rr]) {
#pragma unroll
                    for (int q = 0; q < DPH_DIM / 256; ++q) xr[rr][q] = (float)(((tid + 256 * q) * 37) % 64) * (1.0f / 64.0f) - 0.4921875f;
                }
                if (blockIdx.y == 0 && tid == 0 && r0 + rr < n_rows) nonfinite[r0 + rr] = pqt_bad[rr];
            }
        }
#pragma unroll
        for (int rr = 0; rr < PQT_ROWS; ++rr)
#pragma unroll
            for (int q = 0; q < DPH_DIM / 256; ++q) xs[rr][tid + 256 * q] = (double)xr[rr][q];
    }
    double acc[2] = {0.0, 0.0};
    if (At) {
        stage(0, ring[0]);
        __syncthreads();
        // Rolled: three trips of four steps (the ring index must be a constant inside a trip), the two halves of a step a loop too.
        // Fully unrolled this was 29 KB of straight-line code run once per wave -- instruction fetch, not arithmetic or loads, was what
        // every earlier form of this kernel waited for (28-38 us whatever else changed).
#pragma unroll 1
        for (int st0 = 0; st0 < NST; st0 += RING) {
#pragma unroll
            for (int sr = 0; sr < RING; ++sr) {
                const int st = st0 + sr;
                // (always issued -- past the last step the last block once more, unused: a conditional load makes the compiler wait for
                // the count of the path without it)
                issue(st + RING - 1 < NST ? st + RING - 1 : NST - 1, ring[(sr + RING - 1) % RING]);
#pragma unroll 1
                for (int h = 0; h < PQT_TB; h += 32) {
                    double av[32];
                    double2 xv[2][16];
#pragma unroll
                    for (int u = 0; u < 32; ++u) av[u] = as_[sr & 1][h + u][lane];
#pragma unroll
                    for (int rr = 0; rr < 2; ++rr)
#pragma unroll
                        for (int u = 0; u < 16; ++u) xv[rr][u] = *(const double2*)&xs[2 * wave + rr][st * PQT_TB + h + 2 * u];
                    __builtin_amdgcn_sched_barrier(0);    // (left alone, the scheduler sinks every LDS read next to its use and waits for each)
#pragma unroll
                    for (int u = 0; u < 16; ++u)
#pragma unroll
                        for (int rr = 0; rr < 2; ++rr) {
                            acc[rr] = fma(av[2 * u], xv[rr][u].x, acc[rr]);
                            acc[rr] = fma(av[2 * u + 1], xv[rr][u].y, acc[rr]);
                        }
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (st + 1 < NST) {                       // the other buffer: its readers left at the barrier that ended step st - 1
#pragma unroll
                    for (int i = 0; i < PER; ++i) as_[(sr + 1) & 1][wave * PER + i][lane] = (double)ring[(sr + 1) % RING][i];
                }
                __syncthreads();
            }
        }
    } else {
        __syncthreads();
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) acc[rr] = xs[2 * wave + rr][j];
    }
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
        const int64_t r = r0 + 2 * wave + rr;
        if (r >= n_rows) break;
        double s_ = acc[rr];
        if (b) s_ += (double)b[j];
        const float v = (float)s_;
        out[r * DPH_DIM + j] = v;
        if (out_hi) {
            const unsigned short hi = pq_bf16_rne(v);
            out_hi[r * DPH_DIM + j] = hi;
            if (out_pk) out_pk[r * DPH_DIM + j] = ((unsigned)hi << 16) | (unsigned)pq_bf16_rne(v - __uint_as_float((unsigned)hi << 16));
        }
    }
}
static constexpr size_t PQT_LDS = sizeof(double) * (PQT_ROWS * DPH_DIM + 2 * PQT_TB * PQT_COLS);       // 48 KiB + 64 KiB
static void pq_launch_transform(const float* x, const float* At, int64_t n_rows, const float* b, float* out, unsigned short* out_hi, unsigned* out_pk,
                                int device, hipStream_t st, int32_t* nonfinite = nullptr) {
    DPH_ALLOW_LDS(pq_transform_kernel, PQT_LDS, device);
    hipLaunchKernelGGL(pq_transform_kernel, dim3((unsigned)((n_rows + PQT_ROWS - 1) / PQT_ROWS), DPH_DIM / PQT_COLS), dim3(256), PQT_LDS, st, x, At, n_rows, b, out,
                       out_hi, out_pk, nonfinite);
}

// ---------------------------------------------------------------------------------------------- LUT[r][m][j]
// grid (rows, M / 8): a workgroup fills eight sub-quantisers' tables of a row (one workgroup per table was 12288 launches of
// 2 K multiply-adds at the released shape: 50 us of launch overhead).  DSUB > 0 (a multiple of 4): the thread's eight centroid
// vectors are loaded as float4 BEFORE the first sum starts -- with dsub a run-time value the loop issued one scalar load per
// component and waited for each (64 exposed L2 round trips per thread: 48 us for 64 rows); the sums themselves are unchanged
// (float64, t ascending)
template <int DSUB>
__global__ __launch_bounds__(256) void pq_lut_kernel(const float* __restrict__ xp, const float* __restrict__ pqc, int M, int dsub,
                                                     float* __restrict__ lut) {
    const int64_t r = blockIdx.x;
    const int j = threadIdx.x;
    if constexpr (DSUB > 0) {
        const int m0 = blockIdx.y * 8;
        float4 c[8][DSUB / 4];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int m = m0 + u < M ? m0 + u : M - 1;
            const float4* cp = (const float4*)(pqc + ((int64_t)m * 256 + j) * DSUB);
#pragma unroll
            for (int v = 0; v < DSUB / 4; ++v) c[u][v] = cp[v];
        }
        __builtin_amdgcn_sched_barrier(0);                // (no branch and no scheduling across: the loads would be sunk next to their uses)
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int m = m0 + u < M ? m0 + u : M - 1;     // (a clamped table is computed again and stored again: same value)
            const float* q = xp + r * DPH_DIM + m * DSUB;
            double acc = 0.0;
#pragma unroll
            for (int v = 0; v < DSUB / 4; ++v) {
                acc += (double)q[4 * v] * (double)c[u][v].x;
                acc += (double)q[4 * v + 1] * (double)c[u][v].y;
                acc += (double)q[4 * v + 2] * (double)c[u][v].z;
                acc += (double)q[4 * v + 3] * (double)c[u][v].w;
            }
            lut[(r * M + m) * 256 + j] = (float)acc;
        }
    } else {
        for (int m = blockIdx.y * 8; m < M && m < blockIdx.y * 8 + 8; ++m) {
            const float* c = pqc + ((int64_t)m * 256 + j) * dsub;
            const float* q = xp + r * DPH_DIM + m * dsub;
            double acc = 0.0;
            for (int t = 0; t < dsub; ++t) acc += (double)q[t] * (double)c[t];
            lut[(r * M + m) * 256 + j] = (float)acc;
        }
    }
}

// ---------------------------------------------------------------------------------------------- (list, row) pairs
// one thread per list: every query row of the pass whose bit is set in the list's probe mask becomes a pair -- one pair per CHUNK of
// PQ_LM_CHUNK segments of the list (round 6: work cut by code count; a list of millions of codes among lists of thousands is many
// units of many workgroups, not one workgroup's).  Record: (list, row | chunk << 10); the rows of a pass fit 10 bits (DPH_PASS_MAX).
static_assert(DPH_PASS_MAX <= 1024, "pair records keep the row in 10 bits");
__global__ __launch_bounds__(256) void pq_pairs_kernel(const unsigned* __restrict__ listmask, int mask_words, int nlist,
                                                       const int64_t* __restrict__ list_off, int seg, int2* __restrict__ pairs,
                                                       int* __restrict__ n_pairs, int cap, unsigned* __restrict__ overflow) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= nlist) return;
    const long long len = list_off[l + 1] - list_off[l];
    if (len == 0) return;                                       // empty list: nothing to scan
    const int nch = (int)((len + (long long)seg * PQ_LM_CHUNK - 1) / ((long long)seg * PQ_LM_CHUNK));
    for (int w = 0; w < mask_words; ++w) {
        unsigned m = listmask[(int64_t)l * mask_words + w];
        while (m) {
            const int bit = __builtin_ctz(m);
            m &= m - 1u;
            const int slot = atomicAdd(n_pairs, nch);
            for (int c = 0; c < nch; ++c) {
                if (slot + c < cap) pairs[slot + c] = make_int2(l, (32 * w + bit) | (c << 10));
                else overflow[32 * w + bit] = 1u;               // (cannot happen: the capacity is sized from the longest lists)
            }
        }
    }
}

// k-th largest of the n keys key_at(0 .. n-1), n >= k >= 1, by four 8-bit radix passes.  All PQ_THREADS threads call it; hist = 256 + 4
// words of LDS.  The bin of each pass comes from suffix sums over one wave (lane l owns bins 4l .. 4l+3).
template <class F>
__device__ __forceinline__ unsigned pq_select_kth(F key_at, int n, int k, unsigned* hist) {
    unsigned prefix = 0;
    int left = k;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int i = threadIdx.x; i < 256; i += PQ_THREADS) hist[i] = 0;
        __syncthreads();
        const unsigned hi_mask = shift == 24 ? 0u : (0xFFFFFFFFu << (shift + 8));
        for (int i = threadIdx.x; i < n; i += PQ_THREADS) {
            const unsigned key = key_at(i);
            if ((key & hi_mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (threadIdx.x < 64) {
            const int l = threadIdx.x;
            const unsigned h0 = hist[4 * l], h1 = hist[4 * l + 1], h2 = hist[4 * l + 2], h3 = hist[4 * l + 3];
            const unsigned mine = h0 + h1 + h2 + h3;
            unsigned incl = mine;                                // sum over lanes >= l
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned v = __shfl_down(incl, o);
                if (l + o < 64) incl += v;
            }
            const unsigned above = incl - mine;                  // keys in bins of higher lanes
            if (above < (unsigned)left && (unsigned)left <= incl) {
                unsigned need = (unsigned)left - above;          // rank inside this lane's four bins, from the top
                int bin;
                if (need <= h3) { bin = 4 * l + 3; }
                else if (need <= h3 + h2) { bin = 4 * l + 2; need -= h3; }
                else if (need <= h3 + h2 + h1) { bin = 4 * l + 1; need -= h3 + h2; }
                else { bin = 4 * l; need -= h3 + h2 + h1; }
                hist[256] = (unsigned)bin;
                hist[257] = need;
            }
        }
        __syncthreads();
        prefix |= hist[256] << shift;
        left = (int)hist[257];
        __syncthreads();
    }
    return prefix;
}
__device__ unsigned pq_select_kth_lds(const unsigned* keys, int n, int k, unsigned* hist) {
    return pq_select_kth([&](int i) { return keys[i]; }, n, k, hist);
}

// ---------------------------------------------------------------------------------------------- ADC scan
struct pq_scan_args {
    const float* xp; const float* cent; const float* lut; const uint8_t* codes; const int64_t* list_off;
    const int2* pairs; const int* n_pairs; int* next; int pair_cap;
    int M; int seg; int k; int by_residual;
    unsigned* bound; unsigned* cand_count; uint2* cand; int cand_cap; unsigned* overflow;
    const int2* units; const int* n_units; int unit_cap;      // row-major scan: (row * units_per_row + group, segment) records of pq_units_kernel
    unsigned long long* prof;       // debugging (dph_debug_pq_phases): 8 words per workgroup of the row-major scan, null otherwise
};

// What happens to a segment's scores once they sit in LDS as keys: how many reach the row's running bound?  Fewer than k: the
// segment cannot raise it, only those are appended.  Otherwise the segment's k-th largest (radix select) raises the bound
// (atomicMax) and keys >= max(old bound, k-th) are appended.  pos_of(i) = position of key i in the code array.
template <bool SAMPLE, class P>
__device__ __forceinline__ void pq_segment_finish(const pq_scan_args& a, int r, const unsigned* keys_s, int n, unsigned* hist, P pos_of) {
    // SAMPLE (the row-major scan, segments of ~10 k codes): the bound comes from a strided SAMPLE of PQ_THREADS keys -- its k-th largest is
    // the k-th largest of a subset of the row's scores like every other bound here, just a lower one: the segment appends ~k n / 1024
    // keys instead of ~k (pq_final_kernel selects among a few hundred per row instead of a few dozen), and the four radix passes walk
    // one key per thread instead of twelve: 14 us per unit -> 4 (a sixth of the kernel).  The list-major scan keeps the exact k-th: its
    // rows meet thousands of segments, whose appended keys must stay ~k each.
    const int tid = threadIdx.x, lane = tid & 63;
    const unsigned bound0 = __hip_atomic_load(&a.bound[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int ns = SAMPLE && n > 2 * PQ_THREADS && a.k <= PQ_THREADS / 8 ? PQ_THREADS : n;     // (a large k wants more than a sample holds: exact)
    // sample key i sits at floor(i n / 1024): the positions span the WHOLE segment.  (i * floor(n / 1024), rounds 5-6, left up to 1023
    // keys at the end of the segment unsampled -- a segment is a sequence of LISTS, each with its own <x', centroid> term, and when the
    // row's best list lay in that tail every code of it beat the sample's k-th: hundreds of candidates from one segment, a row with
    // status 1 once in a few hundred random index shapes, tests/test_fuzz_gpu.py.)
    static_assert(PQ_THREADS == 1024, "the sample positions shift by 10");
    const bool sampled = ns < n;
    auto skey = [&](int i) { return keys_s[sampled ? (int)(((unsigned)i * (unsigned)n) >> 10) : i]; };
    int mine = 0;
    for (int i = tid; i < ns; i += PQ_THREADS) mine += skey(i) >= bound0 ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    __syncthreads();
    if (tid == 0) hist[258] = 0;
    __syncthreads();
    if (lane == 0 && mine) atomicAdd(&hist[258], (unsigned)mine);
    __syncthreads();
    const int n_ge = (int)hist[258];                                          // sample keys at or above the row's bound
    unsigned T = bound0;
    if (n_ge >= a.k) {
        const unsigned kth = pq_select_kth(skey, ns, a.k, hist);
        if (kth > T) T = kth;
        if (tid == 0 && kth > bound0) atomicMax(&a.bound[r], kth);
    }
    if (n_ge > 0 || ns < n) {                                                 // (a sample without a key at the bound says nothing about the rest)
        for (int i = tid; i < n; i += PQ_THREADS) {
            const unsigned key = keys_s[i];
            if (key >= T) {
                const unsigned slot = atomicAdd(&a.cand_count[r], 1u);
                if (slot < (unsigned)a.cand_cap) a.cand[(size_t)r * a.cand_cap + slot] = make_uint2(key, (unsigned)pos_of(i));
                else a.overflow[r] = 1u;
            }
        }
    }
}

// Two codes at a time: all code bytes of both (up to 2 x 8 uint4) are loaded BEFORE the look-up chains start, and the two chains --
// each the same sequential fp32 sum as pq_adc_sum -- are interleaved.  pq_adc_sum loads 16 code bytes, walks 16 dependent LDS gathers,
// loads the next 16: six exposed memory latencies per code of an OPQ96 index, and one gather chain per thread in flight; the
// row-major scan of the released shape spent 300 us per batch of 64 that way.
// NG = uint4 per code the kernel is compiled for (6: M <= 96, the released OPQ96; 8: up to M = 128), ng = M / 16 <= NG.
template <int NG>
__device__ __forceinline__ void pq_load_code(const uint8_t* __restrict__ codes, int64_t pos, int M, int ng, uint4 (&c)[NG]) {
    const uint4* cp = (const uint4*)(codes + (size_t)pos * M);
#pragma unroll
    for (int g = 0; g < NG; ++g) c[g] = g < ng ? cp[g] : make_uint4(0u, 0u, 0u, 0u);
}
template <int NG>
__device__ __forceinline__ void pq_adc_sum2(const uint4 (&c0)[NG], const uint4 (&c1)[NG], int ng, const float* lut_s, float& acc0, float& acc1) {
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        if (g < ng) {
            const unsigned w0[4] = {c0[g].x, c0[g].y, c0[g].z, c0[g].w}, w1[4] = {c1[g].x, c1[g].y, c1[g].z, c1[g].w};
#pragma unroll
            for (int w = 0; w < 4; ++w)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int m = g * 16 + w * 4 + b;
                    acc0 = __fadd_rn(acc0, lut_s[m * 256 + ((w0[w] >> (8 * b)) & 255u)]);
                    acc1 = __fadd_rn(acc1, lut_s[m * 256 + ((w1[w] >> (8 * b)) & 255u)]);
                }
        }
    }
}

// One code: the sixteen table entries of a uint4 of code bytes are read TOGETHER, then added in order (the same sequential fp32 sum).
// Left to the scheduler every ds_read was followed by s_waitcnt lgkmcnt(0) and its add -- 96 exposed LDS latencies per code.
template <int NG>
__device__ __forceinline__ float pq_adc_sum1(const uint4 (&c)[NG], int ng, const float* lut_s, float acc) {
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        if (g < ng) {
            const unsigned w[4] = {c[g].x, c[g].y, c[g].z, c[g].w};
            float v[16];
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int b = 0; b < 4; ++b) v[q * 4 + b] = lut_s[(g * 16 + q * 4 + b) * 256 + ((w[q] >> (8 * b)) & 255u)];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 16; ++i) acc = __fadd_rn(acc, v[i]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    return acc;
}

// LIST-MAJOR work (long lists): (list, row) pairs in list order -- the rows probing a list scan it one after the other
// while its codes are hot in L2 / MALL.
template <int NG>
__global__ __launch_bounds__(PQ_THREADS, 1) void pq_adc_kernel(pq_scan_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pq_smem[];
    const int M = a.M;
    float* const lut_s = (float*)pq_smem;                                  // [M][256]
    unsigned* const keys_s = (unsigned*)(lut_s + (size_t)M * 256);          // [seg]
    unsigned* const hist = keys_s + a.seg;                                 // [256 + 8]
    double* const red = (double*)(hist + 264);                             // [16] wave partials
    int* const cur = (int*)(red + 16);                                     // [2] the pair taken from the queue
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_pairs = min(*a.n_pairs, a.pair_cap);
    for (;;) {
        __syncthreads();
        if (tid == 0) cur[0] = atomicAdd(a.next, 1);
        __syncthreads();
        const int p = cur[0];
        if (p >= n_pairs) break;
        const int2 pr = a.pairs[p];
        const int l = pr.x, r = pr.y & 1023, chunk = pr.y >> 10;
        // the row's table into LDS, and dis0 = fl32(<x'_r, c_l>) in float64 (IVFPQ by_residual with METRIC_INNER_PRODUCT)
        const float4* src = (const float4*)(a.lut + (size_t)r * M * 256);
        for (int i = tid; i < M * 64; i += PQ_THREADS) ((float4*)lut_s)[i] = src[i];
        double part = 0.0;
        if (a.by_residual && tid < DPH_DIM) part = (double)a.xp[(size_t)r * DPH_DIM + tid] * (double)a.cent[(size_t)l * DPH_DIM + tid];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
        if (lane == 0) red[wave] = part;
        __syncthreads();
        double d0 = 0.0;
        for (int w = 0; w < DPH_DIM / 64; ++w) d0 += red[w];
        const float dis0 = (float)d0;
        const int64_t begin = a.list_off[l], len = min(a.list_off[l + 1] - begin, (int64_t)(chunk + 1) * a.seg * PQ_LM_CHUNK);
        for (int64_t s0 = (int64_t)chunk * a.seg * PQ_LM_CHUNK; s0 < len; s0 += a.seg) {
            const int n = (int)min((int64_t)a.seg, len - s0);
            __syncthreads();                                               // keys_s / hist of the previous segment are done with
            for (int i = tid; i < n; i += 2 * PQ_THREADS) {
                const int i1 = i + PQ_THREADS < n ? i + PQ_THREADS : i;         // (a lone code is summed twice)
                uint4 c0[NG], c1[NG];
                pq_load_code(a.codes, begin + s0 + i, M, M / 16, c0);
                pq_load_code(a.codes, begin + s0 + i1, M, M / 16, c1);
                float acc0 = dis0, acc1 = dis0;
                pq_adc_sum2(c0, c1, M / 16, lut_s, acc0, acc1);
                keys_s[i] = pq_key(acc0);
                keys_s[i1] = pq_key(acc1);
            }
            __syncthreads();
            pq_segment_finish<false>(a, r, keys_s, n, hist, [&](int i) { return begin + s0 + i; });
        }
    }
}

// ROW-MAJOR work (many short lists -- the reference's 2^20): a group = (query row, PQ_GROUP of its probed lists).  The lists'
// codes are ONE virtual sequence (prefix sums of their lengths in LDS, a binary search per code), so a segment of 12288 codes
// spans dozens of lists and the bound / select step runs once per segment, not once per 160-code list.
// The work is cut by CODE COUNT (round 6): a unit = one segment of <= seg codes of a group's sequence.  A k-means quantizer over
// token vectors (build_phrase_index.py:113-116,156-279) leaves lists hundreds of times the mean, and they are the most probed:
// with one workgroup per group a 600 k-code list kept ONE workgroup busy for 3 ms while 255 idled
// (profiles/r05_pq_ivf1M_b256_one_giant_list_phases.json).  pq_units_kernel writes the (group, segment) records once the probe
// lists are known; a workgroup of the scan pops a record, loads the row's table, rebuilds the group's prefix sums (64 offsets)
// and scores its segment only -- dis0 of just the lists that segment touches.  A uniform index gives one unit per group: the
// same work as before.
// one wave per (row, group): total codes of the group's lists -> ceil(total / seg) unit records (none for an empty group)
__global__ __launch_bounds__(256) void pq_units_kernel(const int* __restrict__ probe, int probe_stride, int units_per_row, int n_groups,
                                                       const int64_t* __restrict__ list_off, int seg, int2* __restrict__ units,
                                                       int* __restrict__ n_units, int unit_cap, unsigned* __restrict__ overflow) {
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= n_groups) return;
    const int r = p / units_per_row, g0 = (p - r * units_per_row) * PQ_GROUP;
    const int l = g0 + lane < probe_stride ? probe[(size_t)r * probe_stride + g0 + lane] : -1;
    long long tot = l >= 0 ? (long long)(list_off[l + 1] - list_off[l]) : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o);
    const int nseg = (int)((tot + seg - 1) / seg);
    if (nseg == 0) return;
    int base = 0;
    if (lane == 0) base = atomicAdd(n_units, nseg);
    base = __shfl(base, 0);
    for (int s_ = lane; s_ < nseg; s_ += 64) {
        if (base + s_ < unit_cap) units[base + s_] = make_int2(p, s_);
        else overflow[r] = 1u;                                     // (cannot happen: the capacity is sized from the longest lists)
    }
}
template <int NG>
__global__ __launch_bounds__(PQ_THREADS, 1) void pq_adc_rows_kernel(pq_scan_args a, const int* __restrict__ probe, int probe_stride,
                                                                    int units_per_row) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pq_smem[];
    const int M = a.M;
    float* const lut_s = (float*)pq_smem;
    unsigned* const keys_s = (unsigned*)(lut_s + (size_t)M * 256);
    unsigned* const hist = keys_s + a.seg;
    double* const red = (double*)(hist + 264);                             // (unused here; keeps the layout of pq_adc_kernel)
    int* const cur = (int*)(red + 16);
    __shared__ int g_list[PQ_GROUP];
    __shared__ long long g_beg[PQ_GROUP];
    __shared__ int g_pre[PQ_GROUP + 1];
    __shared__ float g_dis0[PQ_GROUP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // phase clock of thread 0 (100 MHz wall clock), only when a.prof is set: [start, end, table + lists, dis0, sums, select + append, units, codes]
    const bool prof = a.prof != nullptr && tid == 0;
    __shared__ unsigned long long pt[9];                                   // ([8]: the last stamp)
    if (prof) { for (int i = 1; i < 8; ++i) pt[i] = 0; pt[0] = pt[8] = wall_clock64(); }
    auto lap = [&](int slot) __attribute__((always_inline)) { if (prof) { const unsigned long long t = wall_clock64(); pt[slot] += t - pt[8]; pt[8] = t; } };
    const int n_units = min(*a.n_units, a.unit_cap);
    for (;;) {
        __syncthreads();
        if (tid == 0) cur[0] = atomicAdd(a.next, 1);
        __syncthreads();
        const int u = cur[0];
        if (u >= n_units) break;
        if (prof) pt[8] = wall_clock64();
        const int2 urec = a.units[u];
        const int r = urec.x / units_per_row, g0 = (urec.x - r * units_per_row) * PQ_GROUP;
        const float4* src = (const float4*)(a.lut + (size_t)r * M * 256);
        for (int i = tid; i < M * 64; i += PQ_THREADS) ((float4*)lut_s)[i] = src[i];
        if (tid < PQ_GROUP) {
            const int l = g0 + tid < probe_stride ? probe[(size_t)r * probe_stride + g0 + tid] : -1;
            g_list[tid] = l;
            const long long beg = l >= 0 ? (long long)a.list_off[l] : 0;
            g_beg[tid] = beg;
            // the lists' lengths by 64 threads at once (one thread walking them paid 64 global round trips: ~30 us per unit), then
            // their exclusive prefix sums over the wave
            const int len = l >= 0 ? (int)((long long)a.list_off[l + 1] - beg) : 0;
            int incl = len;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(incl, o); if (tid >= o) incl += v; }
            g_pre[tid] = incl - len;
            if (tid == PQ_GROUP - 1) g_pre[PQ_GROUP] = incl;
        }
        __syncthreads();                                                   // g_list is read by every wave below
        lap(2);
        const int total = g_pre[PQ_GROUP];
        const int s0 = urec.y * a.seg, n = min(a.seg, total - s0);       // this unit's segment of the group's sequence (n >= 1: pq_units_kernel)
        // dis0 of the lists this segment touches, float64: a wave takes two lists per trip and has their 2 x 12 centroid values in
        // flight together (one list after the other, each load waited for: 22 us per unit, a sixth of the kernel); sums as before --
        // t ascending per lane, then the butterfly
        {
            float xv[DPH_DIM / 64];
#pragma unroll
            for (int i = 0; i < DPH_DIM / 64; ++i) xv[i] = a.xp[(size_t)r * DPH_DIM + lane + 64 * i];
            for (int j0 = wave * 2; j0 < PQ_GROUP; j0 += (PQ_THREADS / 64) * 2) {
                // (wave-uniform: LDS values) lists j0, j0 + 1 hold virtual codes [pre[j0], pre[j0 + 2]) -- skip the pair when the segment lies elsewhere
                if (g_pre[j0] >= s0 + n || g_pre[j0 + 2 < PQ_GROUP ? j0 + 2 : PQ_GROUP] <= s0) continue;
                float cv[2][DPH_DIM / 64];
                bool on[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int l = __builtin_amdgcn_readfirstlane(j0 + u < PQ_GROUP ? g_list[j0 + u] : -1);      // (wave-uniform: a scalar row base)
                    const float* crow = a.cent + (size_t)(l >= 0 ? l : 0) * DPH_DIM;          // (an empty slot reads list 0 and is zeroed below: no branch around the loads)
#pragma unroll
                    for (int i = 0; i < DPH_DIM / 64; ++i) cv[u][i] = crow[lane + 64 * i];
                    on[u] = a.by_residual && l >= 0;
                }
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    double part = 0.0;
#pragma unroll
                    for (int i = 0; i < DPH_DIM / 64; ++i) part += (double)xv[i] * (double)cv[u][i];
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
                    if (lane == 0 && j0 + u < PQ_GROUP) g_dis0[j0 + u] = on[u] ? (float)part : 0.f;
                }
            }
        }
        __syncthreads();
        lap(3);
        if (prof) { pt[6] += 1; pt[7] += (unsigned long long)n; }
        auto locate = [&](int v, int& j) {                                 // list of virtual code v: last j with pre[j] <= v
            int lo = 0, hi = PQ_GROUP - 1;
            while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (g_pre[mid] <= v) lo = mid; else hi = mid - 1; }
            j = lo;
            return (int64_t)g_beg[lo] + (v - g_pre[lo]);
        };
        {
            {
                // one code per thread and trip, the NEXT trip's code bytes already on their way while this one's look-ups run (two codes
                // per trip, loaded and then summed: every trip began with an exposed HBM round trip -- random 96-byte reads)
                int i = tid, jn = 0;
                uint4 cn[NG];
                if (i < n) pq_load_code(a.codes, locate(s0 + i, jn), M, M / 16, cn);
                for (; i < n; i += PQ_THREADS) {
                    uint4 cc[NG];
#pragma unroll
                    for (int g = 0; g < NG; ++g) cc[g] = cn[g];
                    const int jc = jn;
                    if (i + PQ_THREADS < n) pq_load_code(a.codes, locate(s0 + i + PQ_THREADS, jn), M, M / 16, cn);
                    __builtin_amdgcn_sched_barrier(0);
                    keys_s[i] = pq_key(pq_adc_sum1<NG>(cc, M / 16, lut_s, g_dis0[jc]));
                }
            }
            __syncthreads();
            lap(4);
            pq_segment_finish<true>(a, r, keys_s, n, hist, [&](int i) { int j; return locate(s0 + i, j); });
            if (a.prof) { __syncthreads(); lap(5); }
        }
    }
    if (prof) {
        pt[1] = wall_clock64();
#pragma unroll
        for (int i = 0; i < 8; ++i) a.prof[(size_t)blockIdx.x * 8 + i] = pt[i];
    }
}

// ---------------------------------------------------------------------------------------------- exact top-k of a row's candidates
__global__ __launch_bounds__(PQ_THREADS) void pq_final_kernel(const uint2* __restrict__ cand, const unsigned* __restrict__ cand_count,
                                                              int cand_cap, const unsigned* __restrict__ overflow,
                                                              const int64_t* __restrict__ ids, int q0, int k, float* __restrict__ D,
                                                              int64_t* __restrict__ I, int32_t* __restrict__ status,
                                                              const int32_t* __restrict__ nonfinite) {
    __shared__ unsigned hist[264];
    __shared__ unsigned skey[PQ_FINAL_CAP];
    __shared__ long long sid[PQ_FINAL_CAP];
    __shared__ unsigned n_keep;
    const int r = blockIdx.x, tid = threadIdx.x;
    if (nonfinite && nonfinite[r]) {                 // (block-uniform) the stand-in of a NaN / Inf row was searched; its answer is FAISS'
        for (int j = tid; j < k; j += PQ_THREADS) { D[(int64_t)(q0 + r) * k + j] = -FLT_MAX; I[(int64_t)(q0 + r) * k + j] = -1; }
        if (tid == 0) status[q0 + r] = DPH_ROW_NONFINITE;
        return;
    }
    const uint2* c = cand + (size_t)r * cand_cap;
    const int n = (int)min(cand_count[r], (unsigned)cand_cap);
    bool bad = overflow[r] != 0u;
    // k-th largest key of the candidates (all of them when fewer than k).  (One thread walking the 256 bins of each of the four
    // passes was 40 of this kernel's 48 us.)
    unsigned T = 0;
    if (n >= k) T = pq_select_kth([&](int i) { return c[i].x; }, n, k, hist);
    if (tid == 0) n_keep = 0;
    __syncthreads();
    for (int i = tid; i < n; i += PQ_THREADS) {
        const uint2 e = c[i];
        if (e.x >= T) {
            const unsigned slot = atomicAdd(&n_keep, 1u);
            if (slot < PQ_FINAL_CAP) { skey[slot] = e.x; sid[slot] = ids[e.y]; }
        }
    }
    __syncthreads();
    int m = (int)n_keep;
    if (m > PQ_FINAL_CAP) { bad = true; m = PQ_FINAL_CAP; }
    int pow2 = 1;
    while (pow2 < m) pow2 <<= 1;
    for (int i = m + tid; i < pow2; i += PQ_THREADS) { skey[i] = 0u; sid[i] = 0x7FFFFFFFFFFFFFFFll; }
    __syncthreads();
    // bitonic sort, (key desc, id asc)
    for (int size = 2; size <= pow2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < pow2 / 2; i += PQ_THREADS) {
                const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                const bool up = (lo & size) == 0;
                const unsigned ka = skey[lo], kb = skey[hi];
                const long long ia = sid[lo], ib = sid[hi];
                const bool a_first = ka > kb || (ka == kb && ia < ib);
                if (a_first != up) { skey[lo] = kb; skey[hi] = ka; sid[lo] = ib; sid[hi] = ia; }
            }
            __syncthreads();
        }
    for (int j = tid; j < k; j += PQ_THREADS) {
        const int64_t o = (int64_t)(q0 + r) * k + j;
        if (j < m) { D[o] = pq_unkey(skey[j]); I[o] = sid[j]; }
        else { D[o] = -FLT_MAX; I[o] = -1; }
    }
    if (tid == 0) status[q0 + r] = bad ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------- direct map, reconstruct
// (pq_store, pq_pos_of_id, pq_list_of_pos, pq_component: dph_internal.h, shared with the window kernel of dph_window.hip)
__global__ __launch_bounds__(256) void pq_reconstruct_kernel(pq_store s, const int64_t* __restrict__ ids, int64_t n,
                                                             float* __restrict__ out, int32_t* __restrict__ found) {
    const int64_t c = blockIdx.x;
    const int64_t pos = pq_pos_of_id(s.dm_ids, s.dm_pos, s.ntotal, ids[c]);
    if (threadIdx.x == 0 && found) found[c] = pos >= 0 ? 1 : 0;
    const int list = pos >= 0 ? pq_list_of_pos(s.list_off, s.nlist, pos) : 0;
    for (int j = threadIdx.x; j < DPH_DIM; j += 256) out[c * DPH_DIM + j] = pos >= 0 ? pq_component(s, pos, list, j) : 0.f;
}

// ---------------------------------------------------------------------------------------------- window re-score: dph_window.hip (PqCodes, DocRows)
// out[v, :] = in[v, :] @ R, R = A [768,768] row-major (index.py:340 `end.matmul(self.R)`, :381-389 `.dot(self.R)`), float64
// accumulation; `twice[v & 1]` vectors get it applied a second time (the reference's pred_*_vecs are taken from the already
// un-rotated window tensor and then multiplied by R again, :345,370 then :381-389 -- replicated as is)
__global__ __launch_bounds__(256) void pq_unrotate_kernel(float* __restrict__ vecs, const float* __restrict__ A, int64_t n_vecs) {
    __shared__ float v[DPH_DIM];
    const int64_t c = blockIdx.x;
    const int reps = (c & 1) ? 2 : 1;
    for (int rep = 0; rep < reps; ++rep) {
        __syncthreads();
        for (int j = threadIdx.x; j < DPH_DIM; j += 256) v[j] = vecs[c * DPH_DIM + j];
        __syncthreads();
        for (int j = threadIdx.x; j < DPH_DIM; j += 256) {
            double acc = 0.0;
            for (int t = 0; t < DPH_DIM; ++t) acc += (double)v[t] * (double)A[(int64_t)t * DPH_DIM + j];
            vecs[c * DPH_DIM + j] = (float)acc;
        }
    }
}

__global__ __launch_bounds__(256) void pq_iota_kernel(unsigned* p, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = (unsigned)i;
}
__global__ __launch_bounds__(256) void pq_dup_kernel(const int64_t* sorted_ids, int64_t n, int* dup) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i + 1 < n && sorted_ids[i] == sorted_ids[i + 1]) *dup = 1;
}

// ============================================================================================== host side
// head of the counters of a pass: the kernels get the addresses of its fields
struct pq_pass_head {
    int n_pairs;                                           // list-major scan: pair records written (pq_pairs_kernel)
    int next;                                              // head of the work queue the scan workgroups pop (pairs or units)
    int n_units;                                           // row-major scan: unit records written (pq_units_kernel)
    int pad[13];
};
static_assert(sizeof(pq_pass_head) == 64 && offsetof(pq_pass_head, n_pairs) == 0 && offsetof(pq_pass_head, next) == 4 && offsetof(pq_pass_head, n_units) == 8,
              "dph_pq_debug_pass hands the head's first words to Python as info[0..3] = pairs, items taken, units, -");

// the per-pass scratch, sized by pq_ensure from (rows, k, nprobe) and the list lengths; released as a whole (`p->s = pq_scratch()`),
// its description with it
struct pq_scratch {
    int cap_rows = 0, cap_k = 0, cap_nprobe = 0;           // what it was sized for
    int cand_cap = 0, pair_cap = 0, unit_cap = 0;          // candidates per row; pair and unit records per pass
    dev_buf<float> xp, lut, scores;
    dev_buf<unsigned> xp_pk;                               // bf16 hi << 16 | lo of the rotated query rows of a pass
    dev_buf<unsigned short> xp_hi;                         // ... and as plain bf16
    dev_buf<unsigned> listmask;
    dev_buf<int2> pairs; dev_buf<uint2> cand;
    // the counters of a pass, ONE allocation: pq_pass_head | bound | cand_count | overflow | nf, the four arrays [cap_rows] words each
    dev_buf<int> counters;
    pq_pass_head* head() const { return (pq_pass_head*)counters.p; }
    unsigned* row_words(int which) const { return (unsigned*)(counters.p + sizeof(pq_pass_head) / 4) + (size_t)which * cap_rows; }
    unsigned* bound() const { return row_words(0); }
    unsigned* cand_count() const { return row_words(1); }
    unsigned* overflow() const { return row_words(2); }
    int32_t* nf() const { return (int32_t*)row_words(3); } // query rows with a NaN / Inf element (pq_transform_kernel writes every row's)
    // bytes of the head and the first `arrays` of them.  All four are allocated; one memset in front of every pass clears three (the
    // coarse quantizer flags a row whose error band overflows in `overflow` too) -- not nf, which the transform has written by then
    static size_t counter_bytes(int rows, int arrays) { return sizeof(pq_pass_head) + (size_t)arrays * rows * 4; }
    dev_buf<int> probe;                                    // [rows][nprobe] probed lists of every row (row-major scan)
    dev_buf<int2> units;                                   // ... and its work queue: (group, segment) records (pq_units_kernel)
};

struct dph_pq {
    int device = 0, nlist = 0, M = 0, dsub = 0, by_residual = 1;
    int64_t ntotal = 0;
    dev_buf<float> A, At, b, cent, pqc;
    dev_buf<float> pqc_bias, pqc_wmax;                     // the encoder's view of the codebooks: fp32(-||w_mj||^2 / 2) [M][256] and max_j ||w_mj|| [M] (rounded up)
    dev_buf<unsigned> cent_pk;                             // bf16 hi << 16 | lo of the centroids (long quantizers: the bf16x3 coarse GEMM)
    dev_buf<unsigned short> cent_hi;                       // the centroids as plain bf16, chunk-major: the sample GEMM of the coarse quantizer's filter
    dev_buf<unsigned short> cent_pieces;                   // ... and as 24 KiB pieces with the byte layout of an int8 tile: the filter scan
    int coarse_filter = 1;                                 // tuning key "coarse_filter": 1 (default) = the filter scan in front of the bf16x3 chain -- bf16 centroid pieces
                                                           // through the flat scan's feed (dph_scan.hip MODE 3) --, 0 = the chain alone
    int coarse_teams = 1;                                  // tuning key "coarse_teams": passes of more than 128 rows run the filter scan as ONE launch of workgroup teams
    dph_profiler prof;
    dph_event_pairs prof_events;                           // around the launches of the coarse filter's dominant kernel
    dph_event_pairs enc_events;                            // around the four launches of every chunk of dph_pq_encode: transform, assign, re-decide, codes
    dph_event_pairs win_events;                            // around the window kernel of every dph_pq_window (the rotation and un-rotation launches outside)
    bool prof_windows = false;                             // ... only when dph_profile_enable was given bit 1 (on = 3): a serving loop that profiles its scans re-scores thousands of windows nobody reads
    std::vector<float> h_A;
    dev_buf<uint8_t> codes; dev_buf<int64_t> ids, list_off;
    std::vector<int64_t> h_list_off;
    dev_buf<int64_t> dm_ids; dev_buf<unsigned> dm_pos;
    double cnorm_max = 0.0, cnorm_cap = 0.0;               // longest centroid; the length above which a list is HEAVY for the coarse filter (dph_coarse_select_kernel)
    dev_buf<float> cnorm;                                  // [nlist] ||c_l||_2
    int64_t max_list = 0;
    bool lists_set = false, params_set = false, finalized = false;
    // scratch, grown on demand
    pq_scratch s;
    std::vector<int64_t> h_top_prefix;                     // [i] = codes in the i longest lists: what a row can meet at most with nprobe = i
    // what lives until the index is freed
    dev_buf<float> qrot; int64_t qrot_rows = 0;            // rotated query halves of dph_pq_window
    dph_coarse_scratch coarse;                             // of the coarse quantizer (dph_launch_coarse / dph_launch_coarse_filter allocate what they need)
    struct { dev_buf<float> xp, gap; dev_buf<int32_t> nf; int64_t rows = 0; } enc;    // scratch of dph_pq_encode: one chunk of rotated rows, gaps, flags
    dev_buf<unsigned long long> phase_prof;                // dph_debug_pq_phases: [workgroups][8], allocated by the first call
    int phase_wgs = 0;
};

int dph_pq_alloc(dph_pq** out, int device, int64_t ntotal, int nlist, int M) {
    if (!out || ntotal < 0 || nlist <= 0 || nlist > (1 << 20) || M <= 0 || DPH_DIM % M || M % 16 || M > 128)
        return fail(DPH_E_ARG, "PQ index: need 0 < nlist <= 2^20 and M a multiple of 16 that divides 768, M <= 128");
    if (ntotal >= (int64_t)0xFFFFFFF0ll) return fail(DPH_E_ARG, "PQ index: at most 2^32-16 codes per GPU");
    HIPCHK(hipSetDevice(device));
    dph_pq* p = new dph_pq();
    p->device = device; p->ntotal = ntotal; p->nlist = nlist; p->M = M; p->dsub = DPH_DIM / M;
    const size_t nt = (size_t)(ntotal > 0 ? ntotal : 1);
    if (p->cent.alloc((size_t)nlist * DPH_DIM) != hipSuccess || p->pqc.alloc((size_t)256 * DPH_DIM) != hipSuccess ||
        p->codes.alloc(nt * M + 16) != hipSuccess || p->ids.alloc(nt) != hipSuccess ||
        p->list_off.alloc((size_t)nlist + 1) != hipSuccess || p->dm_ids.alloc(nt) != hipSuccess ||
        p->dm_pos.alloc(nt) != hipSuccess) {
        dph_pq_free(p);
        return fail(DPH_E_NOMEM, "PQ index: hipMalloc failed");
    }
    *out = p;
    return DPH_OK;
}

void dph_pq_set_coarse_filter(dph_pq* p, int on) { if (p) p->coarse_filter = on ? 1 : 0; }
void dph_pq_set_coarse_teams(dph_pq* p, int on) { if (p) p->coarse_teams = on ? 1 : 0; }
int dph_pq_coarse_debug(dph_pq* p, unsigned out[2]) {
    if (!p) return fail(DPH_E_ARG, "null");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipDeviceSynchronize());
    return dph_coarse_filter_debug(p->coarse, out) ? fail(DPH_E_HIP, "coarse debug: copy failed") : DPH_OK;
}
// what the LAST pass left in the scan's bookkeeping: info[8] = {counters[0..3] (pairs, next, units, -), cand_cap, unit_cap, pair_cap, rows of
// the scratch}, per_row[n][3] = {appended candidates, overflow flag, bound key} of the first n rows.  (tests/test_fuzz_gpu.py prints it
// for a round that comes back uncertified.)
int dph_pq_debug_pass(dph_pq* p, int* info, unsigned* per_row, int n) {
    if (!p || !info || n < 0) return fail(DPH_E_ARG, "null");
    if (!p->s.counters) return fail(DPH_E_STATE, "PQ debug: no search yet");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipDeviceSynchronize());
    pq_pass_head head;
    HIPCHK(hipMemcpy(&head, p->s.head(), sizeof head, hipMemcpyDeviceToHost));
    info[0] = head.n_pairs; info[1] = head.next; info[2] = head.n_units; info[3] = head.pad[0];
    info[4] = p->s.cand_cap; info[5] = p->s.unit_cap; info[6] = p->s.pair_cap; info[7] = p->s.cap_rows;
    n = std::min(n, p->s.cap_rows);
    const unsigned* const cols[3] = {p->s.cand_count(), p->s.overflow(), p->s.bound()};
    std::vector<unsigned> col((size_t)n);
    for (int c = 0; c < 3 && n > 0 && per_row; ++c) {
        HIPCHK(hipMemcpy(col.data(), cols[c], (size_t)n * 4, hipMemcpyDeviceToHost));
        for (int r = 0; r < n; ++r) per_row[3 * r + c] = col[(size_t)r];
    }
    return DPH_OK;
}
// phase clock of the row-major ADC scan: the first call (out = null) arms it, later calls copy the last launch's [workgroups][8]
// 100 MHz ticks: start, end, table + lists, dis0, sums, select + append, units, codes.  Returns the number of workgroups.
// which = 1: dph_coarse_select_kernel's stamps instead (dph_ivf.hip).
int dph_pq_debug_phases(dph_pq* p, int which, unsigned long long* out, int cap_wgs) {
    if (!p) return -1;
    if (hipSetDevice(p->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return -1;
    if (which == 1) return dph_coarse_select_clock(out, cap_wgs);        // the probe selection's stamps, one record per query row
    if (!p->phase_prof) {
        const int cus = dph_scan_grid(p->device);
        if (p->phase_prof.alloc((size_t)cus * 8) != hipSuccess) return -1;
        (void)hipMemset(p->phase_prof, 0, (size_t)cus * 64);
        p->phase_wgs = cus;
    }
    const int n = cap_wgs < p->phase_wgs ? cap_wgs : p->phase_wgs;
    if (out && n > 0 && hipMemcpy(out, p->phase_prof, (size_t)n * 64, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return p->phase_wgs;
}
int dph_pq_profile(dph_pq* p, int on) {
    if (!p) return fail(DPH_E_ARG, "null");
    HIPCHK(hipSetDevice(p->device));
    p->prof.on = on != 0;
    p->prof_windows = (on & 2) != 0;
    if (on) HIPCHK(p->prof.warm(64));
    return DPH_OK;
}
int dph_pq_profile_read(dph_pq* p, double* ms_total, int* launches) {
    if (!p || !ms_total || !launches) return fail(DPH_E_ARG, "null");
    HIPCHK(hipSetDevice(p->device));
    return p->prof.drain(p->prof_events, ms_total, launches);
}
int dph_pq_profile_read_each(dph_pq* p, int which, double* ms_out, int cap, int* n_out) {
    if (!p || !n_out) return fail(DPH_E_ARG, "null");
    HIPCHK(hipSetDevice(p->device));
    return p->prof.drain(which == 3 ? p->win_events : which == 2 ? p->enc_events : p->prof_events, nullptr, n_out, ms_out, cap);
}

void dph_pq_free(dph_pq* p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    delete p;
}

int dph_pq_set_params(dph_pq* p, const float* A, const float* b, const float* centroids, const float* pq_centroids, int by_residual) {
    if (!p || !centroids || !pq_centroids) return fail(DPH_E_ARG, "PQ index: null parameter");
    HIPCHK(hipSetDevice(p->device));
    p->A.reset(); p->At.reset(); p->b.reset();
    p->h_A.assign((size_t)DPH_DIM * DPH_DIM, 0.f);
    if (A) {
        p->h_A.assign(A, A + (size_t)DPH_DIM * DPH_DIM);
        std::vector<float> At((size_t)DPH_DIM * DPH_DIM);
        for (int i = 0; i < DPH_DIM; ++i) for (int j = 0; j < DPH_DIM; ++j) At[(size_t)j * DPH_DIM + i] = A[(size_t)i * DPH_DIM + j];
        HIPCHK(p->A.alloc(At.size()));
        HIPCHK(p->At.alloc(At.size()));
        HIPCHK(hipMemcpy(p->A, A, At.size() * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(p->At, At.data(), At.size() * 4, hipMemcpyHostToDevice));
    } else {
        for (int i = 0; i < DPH_DIM; ++i) p->h_A[(size_t)i * DPH_DIM + i] = 1.f;
    }
    if (b) {
        HIPCHK(p->b.alloc(DPH_DIM));
        HIPCHK(hipMemcpy(p->b, b, DPH_DIM * 4, hipMemcpyHostToDevice));
    }
    HIPCHK(hipMemcpy(p->cent, centroids, (size_t)p->nlist * DPH_DIM * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(p->pqc, pq_centroids, (size_t)256 * DPH_DIM * 4, hipMemcpyHostToDevice));
    if (p->nlist >= (1 << 16)) {                    // CG_BF16X3_MIN of dph_ivf.hip: the coarse GEMM of long quantizers runs on bf16 hi / lo parts
        if (!p->cent_pk) HIPCHK(p->cent_pk.alloc((size_t)p->nlist * DPH_DIM));
        dph_launch_bf16_split(p->cent, (int64_t)p->nlist * DPH_DIM, p->cent_pk, nullptr);
        if (!p->cent_hi) HIPCHK(p->cent_hi.alloc((size_t)dph_bf16_hi_rows(p->nlist) * DPH_DIM));
        dph_launch_bf16_hi(p->cent, p->nlist, p->cent_hi, nullptr);
        if (!p->cent_pieces) HIPCHK(p->cent_pieces.alloc((size_t)dph_bf16_piece_rows(p->nlist) * DPH_DIM));
        dph_launch_bf16_pieces(p->cent, p->nlist, p->cent_pieces, nullptr);
        HIPCHK(hipDeviceSynchronize());
    }
    double mx = 0.0;
    std::vector<float> cn((size_t)p->nlist);
    for (int l = 0; l < p->nlist; ++l) {
        double s = 0.0;
        for (int j = 0; j < DPH_DIM; ++j) s += (double)centroids[(size_t)l * DPH_DIM + j] * (double)centroids[(size_t)l * DPH_DIM + j];
        mx = std::max(mx, s);
        cn[(size_t)l] = (float)(sqrt(s) * (1.0 + 1e-6));          // (rounded up: it bounds an error)
    }
    p->cnorm_max = sqrt(mx);
    {
        // heavy lists: centroids longer than 1.1 x the 99-th percentile (none when the lengths are alike: the cap is then the maximum)
        std::vector<float> srt(cn);
        const size_t q99 = (size_t)((double)(p->nlist - 1) * 0.99);
        std::nth_element(srt.begin(), srt.begin() + (std::ptrdiff_t)q99, srt.end());
        p->cnorm_cap = std::min(p->cnorm_max, 1.1 * (double)srt[q99]);
        if (!p->cnorm) HIPCHK(p->cnorm.alloc((size_t)p->nlist));
        HIPCHK(hipMemcpy(p->cnorm, cn.data(), (size_t)p->nlist * 4, hipMemcpyHostToDevice));
    }
    {
        // the encoder's bias and bound constant of every codebook: ||w||^2 in float64, sequential in t
        const int dsub = p->dsub;
        std::vector<float> bias((size_t)p->M * 256), wmax((size_t)p->M);
        for (int m = 0; m < p->M; ++m) {
            double mx2 = 0.0;
            for (int j = 0; j < 256; ++j) {
                const float* w = pq_centroids + ((size_t)m * 256 + j) * dsub;
                double nw = 0.0;
                for (int t = 0; t < dsub; ++t) nw += (double)w[t] * (double)w[t];
                bias[(size_t)m * 256 + j] = (float)(-0.5 * nw);
                mx2 = std::max(mx2, nw);
            }
            wmax[(size_t)m] = nextafterf((float)(sqrt(mx2) * (1.0 + 1e-6)), INFINITY);       // (rounded up: it bounds an error)
        }
        if (!p->pqc_bias) HIPCHK(p->pqc_bias.alloc(bias.size()));
        if (!p->pqc_wmax) HIPCHK(p->pqc_wmax.alloc(wmax.size()));
        HIPCHK(hipMemcpy(p->pqc_bias, bias.data(), bias.size() * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(p->pqc_wmax, wmax.data(), wmax.size() * 4, hipMemcpyHostToDevice));
    }
    p->by_residual = by_residual ? 1 : 0;
    p->params_set = true;
    return DPH_OK;
}

int dph_pq_set_list_sizes(dph_pq* p, const int64_t* sizes) {
    if (!p || !sizes) return fail(DPH_E_ARG, "PQ index: null list sizes");
    HIPCHK(hipSetDevice(p->device));
    p->h_list_off.assign((size_t)p->nlist + 1, 0);
    p->max_list = 0;
    for (int l = 0; l < p->nlist; ++l) {
        if (sizes[l] < 0) return fail(DPH_E_ARG, "PQ index: negative list size");
        p->h_list_off[(size_t)l + 1] = p->h_list_off[(size_t)l] + sizes[l];
        p->max_list = std::max(p->max_list, sizes[l]);
    }
    if (p->h_list_off[(size_t)p->nlist] != p->ntotal) return fail(DPH_E_ARG, "PQ index: list sizes do not add up to ntotal");
    HIPCHK(hipMemcpy(p->list_off, p->h_list_off.data(), ((size_t)p->nlist + 1) * 8, hipMemcpyHostToDevice));
    plan_pq_top_prefix(sizes, p->nlist, p->h_top_prefix);
    p->s = pq_scratch();                                   // (the scratch is sized from the list lengths)
    p->lists_set = true;
    p->finalized = false;
    return DPH_OK;
}

int dph_pq_upload(dph_pq* p, int64_t pos0, int64_t n, const uint8_t* codes, const int64_t* ids) {
    if (!p || n < 0 || pos0 < 0 || pos0 + n > p->ntotal || (n > 0 && (!codes || !ids))) return fail(DPH_E_ARG, "PQ index: bad code range");
    HIPCHK(hipSetDevice(p->device));
    if (n > 0) {
        HIPCHK(hipMemcpy(p->codes + (size_t)pos0 * p->M, codes, (size_t)n * p->M, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(p->ids + pos0, ids, (size_t)n * 8, hipMemcpyHostToDevice));
    }
    p->finalized = false;
    return DPH_OK;
}

int dph_pq_finalize(dph_pq* p, hipStream_t st) {
    if (!p || !p->params_set || !p->lists_set) return fail(DPH_E_STATE, "PQ index: parameters / list sizes not set");
    HIPCHK(hipSetDevice(p->device));
    if (p->ntotal > 0) {
        dev_buf<unsigned> iota;
        dev_buf<int> dup;
        HIPCHK(iota.alloc((size_t)p->ntotal));
        if (dup.alloc(1) != hipSuccess) return fail(DPH_E_NOMEM, "PQ index: hipMalloc");
        (void)hipMemsetAsync(dup, 0, 4, st);
        hipLaunchKernelGGL(pq_iota_kernel, dim3((unsigned)((p->ntotal + 255) / 256)), dim3(256), 0, st, iota, p->ntotal);
        int rc = dph_sort_pairs_i64_u32(p->ids, iota, p->dm_ids, p->dm_pos, p->ntotal, st);
        int dup_h = 0;
        if (rc == 0) {
            hipLaunchKernelGGL(pq_dup_kernel, dim3((unsigned)((p->ntotal + 255) / 256)), dim3(256), 0, st, p->dm_ids, p->ntotal, dup);
            if (hipMemcpyAsync(&dup_h, dup, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) rc = 1;
        }
        if (rc) return fail(DPH_E_HIP, "PQ index: building the direct map failed");
        if (dup_h) return fail(DPH_E_ARG, "PQ index: duplicate ids in the inverted lists");
    }
    p->finalized = true;
    return DPH_OK;
}

// ---------------------------------------------------------------------------------------------- the add step (kernels: dph_pq_encode.hip)
// x [n,768] fp32 (device) -> list[n], codes[n,M]: a pure function of the parameters, in chunks of PQ_ENC_CHUNK rows through a scratch of
// one chunk (192 MiB of rotated rows).  A non-finite row comes back with list -1 and zero codes.
#define PQ_ENC_CHUNK 65536
int dph_pq_encode(dph_pq* p, const float* x_dev, int64_t n, int32_t* list_dev, uint8_t* codes_dev, hipStream_t st) {
    if (!p || !x_dev || n <= 0 || !list_dev || !codes_dev) return fail(DPH_E_ARG, "PQ encode: null pointer or no rows");
    if (((uintptr_t)codes_dev & 15u) || ((uintptr_t)x_dev & 15u)) return fail(DPH_E_ARG, "PQ encode: x and codes must be 16-byte aligned");
    if (!p->params_set) return fail(DPH_E_STATE, "PQ encode: parameters not set (dph_index_set_pq)");
    HIPCHK(hipSetDevice(p->device));
    const int64_t chunk = std::min<int64_t>(n, PQ_ENC_CHUNK);
    if (p->enc.rows < chunk) {
        p->enc.rows = 0;
        HIPCHK(p->enc.xp.alloc((size_t)chunk * DPH_DIM));
        HIPCHK(p->enc.gap.alloc((size_t)chunk));
        HIPCHK(p->enc.nf.alloc((size_t)chunk));
        p->enc.rows = chunk;
    }
    dph_event_pairs* ev = p->prof.on ? &p->enc_events : nullptr;
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t m = std::min(chunk, n - r0);
        const float* x = x_dev + r0 * DPH_DIM;
        int32_t* list = list_dev + r0;
        p->prof.bracket(ev, st, [&] { pq_launch_transform(x, p->At, m, p->b, p->enc.xp, nullptr, nullptr, p->device, st, p->enc.nf); });
        p->prof.bracket(ev, st, [&] { dph_launch_assign(p->enc.xp, false, nullptr, m, p->cent, p->nlist, nullptr, list, p->enc.gap, st); });
        p->prof.bracket(ev, st, [&] { dph_launch_pq_relist(p->enc.xp, m, p->cent, p->nlist, p->enc.nf, p->enc.gap, p->cnorm_max, list, st); });
        int rc = 0;
        p->prof.bracket(ev, st, [&] {
            rc = dph_launch_pq_codes(p->enc.xp, m, list, p->cent, p->by_residual, p->pqc, p->pqc_bias, p->pqc_wmax, p->M, codes_dev + r0 * p->M, p->device, st);
        });
        if (rc) return fail(DPH_E_ARG, "PQ encode: no kernel for this M");
    }
    HIPCHK(hipGetLastError());
    return DPH_OK;
}

// list[n], codes[n,M], ids[n] of ALL ntotal codes (device) -> the handle's list-major codes / ids / list_off: stable order by (list, input
// position), FAISS' append order.  A list outside [0, nlist) -- the -1 of a non-finite row -- fails the call before anything is written.
int dph_pq_fill(dph_pq* p, int64_t n, const int32_t* list_dev, const uint8_t* codes_dev, const int64_t* ids_dev, hipStream_t st) {
    if (!p || n <= 0 || !list_dev || !codes_dev || !ids_dev) return fail(DPH_E_ARG, "PQ fill: null pointer or no codes");
    if ((uintptr_t)codes_dev & 15u) return fail(DPH_E_ARG, "PQ fill: codes must be 16-byte aligned");
    if (!p->params_set) return fail(DPH_E_STATE, "PQ fill: parameters not set (dph_index_set_pq)");
    if (n != p->ntotal) return fail(DPH_E_ARG, "PQ fill: takes all ntotal codes of the handle at once");
    HIPCHK(hipSetDevice(p->device));
    p->finalized = false;
    dev_buf<int64_t> keys, keys_sorted;
    dev_buf<unsigned> vals, vals_sorted, counts;
    dev_buf<int> bad;
    HIPCHK(keys.alloc((size_t)n)); HIPCHK(keys_sorted.alloc((size_t)n));
    HIPCHK(vals.alloc((size_t)n)); HIPCHK(vals_sorted.alloc((size_t)n));
    HIPCHK(counts.alloc((size_t)p->nlist)); HIPCHK(bad.alloc(1));
    HIPCHK(hipMemsetAsync(counts, 0, (size_t)p->nlist * 4, st));
    HIPCHK(hipMemsetAsync(bad, 0, 4, st));
    dph_launch_pq_fill_keys(list_dev, n, p->nlist, keys, vals, counts, bad, st);
    int bad_h = 0;
    std::vector<unsigned> cnt((size_t)p->nlist);
    HIPCHK(hipMemcpyAsync(&bad_h, bad, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(cnt.data(), counts, (size_t)p->nlist * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (bad_h) return fail(DPH_E_ARG, "PQ fill: a row's list is outside [0, nlist) (-1 marks a non-finite row)");
    if (dph_sort_pairs_i64_u32(keys, vals, keys_sorted, vals_sorted, n, st)) return fail(DPH_E_HIP, "PQ fill: sorting by (list, position) failed");
    dph_launch_pq_fill_gather(vals_sorted, n, p->M, codes_dev, ids_dev, p->codes, p->ids, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    std::vector<int64_t> sizes(cnt.begin(), cnt.end());
    return dph_pq_set_list_sizes(p, sizes.data());         // list_off, the host copies, the search scratch dropped
}

int dph_pq_get_list_sizes(dph_pq* p, int64_t* sizes) {
    if (!p || !sizes) return fail(DPH_E_ARG, "PQ list sizes: null");
    if (!p->params_set || !p->lists_set) return fail(DPH_E_STATE, "PQ list sizes: parameters / lists not set");
    for (int l = 0; l < p->nlist; ++l) sizes[l] = p->h_list_off[(size_t)l + 1] - p->h_list_off[(size_t)l];
    return DPH_OK;
}

int dph_pq_download(dph_pq* p, int64_t pos0, int64_t n, uint8_t* codes, int64_t* ids) {
    if (!p || n <= 0 || pos0 < 0 || !codes || !ids) return fail(DPH_E_ARG, "PQ download: null pointer or no codes");
    if (!p->params_set || !p->lists_set) return fail(DPH_E_STATE, "PQ download: parameters / lists not set");
    if (pos0 + n > p->ntotal) return fail(DPH_E_ARG, "PQ download: bad code range");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(codes, p->codes + (size_t)pos0 * p->M, (size_t)n * p->M, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ids, p->ids + pos0, (size_t)n * 8, hipMemcpyDeviceToHost));
    return DPH_OK;
}

bool dph_pq_ready(const dph_pq* p) { return p && p->finalized; }
int64_t dph_pq_ntotal(const dph_pq* p) { return p ? p->ntotal : 0; }
int dph_pq_nlist(const dph_pq* p) { return p ? p->nlist : 0; }
const float* dph_pq_A_host(const dph_pq* p) { return p ? p->h_A.data() : nullptr; }

// the scan's plan (dph_plan.h: segment length, row-major or list-major work, LDS, capacities) from this index's lists
static plan_pq_facts pq_facts(const dph_pq* p) { return plan_pq_facts{p->M, p->ntotal, p->nlist, p->max_list, p->h_top_prefix.data()}; }
static bool pq_by_rows(const dph_pq* p) { return pq_by_rows(pq_facts(p)); }
// (one workgroup per CU either way: __launch_bounds__(PQ_THREADS, 1); the launches pass pq_lds_bytes(p->M))
static void pq_allow_lds(int device) {
    DPH_ALLOW_LDS(pq_adc_kernel<6>, pq_lds_bytes_max(), device);
    DPH_ALLOW_LDS(pq_adc_kernel<8>, pq_lds_bytes_max(), device);
    DPH_ALLOW_LDS(pq_adc_rows_kernel<6>, pq_lds_bytes_max(), device);
    DPH_ALLOW_LDS(pq_adc_rows_kernel<8>, pq_lds_bytes_max(), device);
}

static int pq_ensure(dph_pq* p, int rows, int k, int nprobe) {
    if (rows <= p->s.cap_rows && k <= p->s.cap_k && nprobe <= p->s.cap_nprobe) return DPH_OK;
    rows = std::max(rows, p->s.cap_rows); k = std::max(k, p->s.cap_k); nprobe = std::max(nprobe, p->s.cap_nprobe);
    p->s = pq_scratch();
    pq_scratch& s = p->s;
    const plan_pq_caps caps = plan_pq_scan(pq_facts(p), rows, k, nprobe);
    s.cand_cap = caps.cand_cap; s.pair_cap = caps.pair_cap; s.unit_cap = caps.unit_cap;
    if (s.xp.alloc((size_t)rows * DPH_DIM) != hipSuccess || s.lut.alloc((size_t)rows * p->M * 256) != hipSuccess ||
        s.scores.alloc((size_t)rows * p->nlist) != hipSuccess || s.listmask.alloc((size_t)p->nlist * DPH_UNIT_WORDS) != hipSuccess ||
        s.counters.alloc(pq_scratch::counter_bytes(rows, 4) / 4) != hipSuccess ||
        s.pairs.alloc((size_t)s.pair_cap) != hipSuccess ||
        s.cand.alloc((size_t)rows * s.cand_cap) != hipSuccess ||
        s.probe.alloc((size_t)rows * nprobe) != hipSuccess ||
        (s.unit_cap > 0 && s.units.alloc((size_t)s.unit_cap) != hipSuccess) ||
        s.xp_pk.alloc((size_t)rows * DPH_DIM) != hipSuccess ||
        s.xp_hi.alloc((size_t)rows * DPH_DIM) != hipSuccess) {
        p->s = pq_scratch();
        return fail(DPH_E_NOMEM, "PQ search: scratch allocation failed");
    }
    s.cap_rows = rows; s.cap_k = k; s.cap_nprobe = nprobe;
    return DPH_OK;
}

// ---- a pass of up to DPH_PASS_MAX query rows in four stages, all asynchronous on st
// Stage 1: the rows rotated, x' = A x + b (a long quantizer: with their bf16 images), and their inner-product tables.
static void pq_pass_tables(dph_pq* p, const float* x, int nq, hipStream_t st) {
    pq_launch_transform(x, p->At, nq, p->b, p->s.xp, p->cent_pk ? p->s.xp_hi : (unsigned short*)nullptr, p->cent_pk ? p->s.xp_pk : (unsigned*)nullptr, p->device, st, p->s.nf());
    const dim3 lg(nq, (p->M + 7) / 8);
    if (p->dsub == 8) hipLaunchKernelGGL(pq_lut_kernel<8>, lg, dim3(256), 0, st, p->s.xp, p->pqc, p->M, p->dsub, p->s.lut);             // M = 96 (the released OPQ96)
    else if (p->dsub == 12) hipLaunchKernelGGL(pq_lut_kernel<12>, lg, dim3(256), 0, st, p->s.xp, p->pqc, p->M, p->dsub, p->s.lut);       // M = 64
    else if (p->dsub == 16) hipLaunchKernelGGL(pq_lut_kernel<16>, lg, dim3(256), 0, st, p->s.xp, p->pqc, p->M, p->dsub, p->s.lut);       // M = 48
    else hipLaunchKernelGGL(pq_lut_kernel<0>, lg, dim3(256), 0, st, p->s.xp, p->pqc, p->M, p->dsub, p->s.lut);
}

// what the coarse quantizer is asked for a pass: probe masks per list (list-major scan) or a probe list per row -- the row-major scan
// walks the probe lists, not the masks (134 MB to clear at 2^20 lists)
static dph_coarse_filter_args pq_coarse_args(dph_pq* p, int nq, int nprobe, bool by_rows) {
    dph_coarse_filter_args c;
    c.x = p->s.xp; c.n_q = nq;
    c.centroids = p->cent; c.nlist = p->nlist; c.nprobe = nprobe; c.cnorm_max = p->cnorm_max;
    c.scores = p->s.scores;
    c.listmask = by_rows ? nullptr : p->s.listmask.p; c.mask_words = DPH_UNIT_WORDS;
    c.probe_out = by_rows ? p->s.probe.p : nullptr; c.probe_stride = nprobe;
    c.c_pk = p->cent_pk; c.x_pk = p->cent_pk ? p->s.xp_pk.p : nullptr;
    c.row_fail = p->s.overflow();
    // the filter's part
    c.c_hi = p->cent_hi; c.x_hi = p->s.xp_hi; c.c_pieces = p->cent_pieces;
    c.cnorm = p->cnorm; c.cnorm_cap = p->cnorm_cap;
    c.teams = p->coarse_teams;
    if (p->prof.on) { c.prof = &p->prof; c.prof_list = &p->prof_events; }
    return c;
}
// Stage 2: the counters of the pass cleared, then the coarse probe -- a long quantizer through the filter, otherwise the chain.
static int pq_pass_probe(dph_pq* p, int nq, int nprobe, bool by_rows, hipStream_t st) {
    HIPCHK(hipMemsetAsync(p->s.counters, 0, pq_scratch::counter_bytes(p->s.cap_rows, 3), st));
    const dph_coarse_filter_args c = pq_coarse_args(p, nq, nprobe, by_rows);
    if (p->cent_hi && p->coarse_filter) dph_launch_coarse_filter(c, p->coarse, st);
    else dph_launch_coarse(c, p->coarse, st);
    return DPH_OK;
}

template <int NG> static void pq_launch_adc(const dph_pq* p, const pq_scan_args& a, bool by_rows, int grid, int nprobe, int units_per_row, hipStream_t st) {
    if (by_rows) hipLaunchKernelGGL(pq_adc_rows_kernel<NG>, dim3(grid), dim3(PQ_THREADS), pq_lds_bytes(p->M), st, a, p->s.probe, nprobe, units_per_row);
    else hipLaunchKernelGGL(pq_adc_kernel<NG>, dim3(grid), dim3(PQ_THREADS), pq_lds_bytes(p->M), st, a);
}
// Stage 3: the work queue from what the probe left (units of a row's groups, or (list, row) pairs), then the ADC scan, one workgroup per CU.
static void pq_pass_scan(dph_pq* p, int nq, int k, int nprobe, bool by_rows, int grid, hipStream_t st) {
    const pq_scratch& s = p->s;
    pq_pass_head* const head = s.head();           // (addresses of device memory: nothing is read here)
    pq_scan_args a;
    a.xp = s.xp; a.cent = p->cent; a.lut = s.lut; a.codes = p->codes; a.list_off = p->list_off;
    a.pairs = s.pairs; a.n_pairs = &head->n_pairs; a.next = &head->next; a.pair_cap = s.pair_cap;
    a.M = p->M; a.seg = pq_seg(p->M); a.k = k; a.by_residual = p->by_residual;
    a.bound = s.bound(); a.cand_count = s.cand_count(); a.cand = s.cand; a.cand_cap = s.cand_cap; a.overflow = s.overflow();
    a.prof = p->phase_prof && p->phase_wgs >= grid ? p->phase_prof : nullptr;
    a.units = s.units; a.n_units = &head->n_units; a.unit_cap = s.unit_cap;
    const int upr = (nprobe + PQ_GROUP - 1) / PQ_GROUP;
    // many short lists on average: group the work by query row, cut by code count (pq_units_kernel)
    if (by_rows)
        hipLaunchKernelGGL(pq_units_kernel, dim3((nq * upr + 3) / 4), dim3(256), 0, st, s.probe, nprobe, upr, nq * upr, p->list_off, a.seg, s.units,
                           &head->n_units, s.unit_cap, s.overflow());
    else
        hipLaunchKernelGGL(pq_pairs_kernel, dim3((p->nlist + 255) / 256), dim3(256), 0, st, s.listmask, DPH_UNIT_WORDS, p->nlist,
                           p->list_off, a.seg, s.pairs, &head->n_pairs, s.pair_cap, s.overflow());
    if (p->M <= 96) pq_launch_adc<6>(p, a, by_rows, grid, nprobe, upr, st);
    else pq_launch_adc<8>(p, a, by_rows, grid, nprobe, upr, st);
}

// Stage 4: every row's k best candidates, their ids and the row's status.
static void pq_pass_final(dph_pq* p, int q0, int nq, int k, float* D, int64_t* I, int32_t* status, hipStream_t st) {
    hipLaunchKernelGGL(pq_final_kernel, dim3(nq), dim3(PQ_THREADS), 0, st, p->s.cand, p->s.cand_count(), p->s.cand_cap, p->s.overflow(), p->ids,
                       q0, k, D, I, status, (const int32_t*)p->s.nf());
}

// x_dev [n,768] -> D/I [n,k], status [n] (0 = exact top-k of the probed lists, 1 = candidate buffers overflowed); asynchronous on st
int dph_pq_search_dev(dph_pq* p, const float* x_dev, int64_t n, int k, int nprobe, float* D, int64_t* I, int32_t* status, hipStream_t st) {
    if (!p || !p->finalized) return fail(DPH_E_STATE, "PQ search: index not finalized");
    HIPCHK(hipSetDevice(p->device));
    nprobe = std::max(1, std::min(nprobe, p->nlist));
    int rc = pq_ensure(p, (int)std::min<int64_t>(n, DPH_PASS_MAX), k, nprobe);
    if (rc) return rc;
    pq_allow_lds(p->device);
    const int grid = dph_scan_grid(p->device);
    const bool by_rows = pq_by_rows(p);
    for (int64_t q0 = 0; q0 < n; q0 += DPH_PASS_MAX) {
        const int nq = (int)std::min<int64_t>(n - q0, DPH_PASS_MAX);
        pq_pass_tables(p, x_dev + q0 * DPH_DIM, nq, st);
        rc = pq_pass_probe(p, nq, nprobe, by_rows, st);
        if (rc) return rc;
        pq_pass_scan(p, nq, k, nprobe, by_rows, grid, st);
        pq_pass_final(p, (int)q0, nq, k, D, I, status, st);
    }
    HIPCHK(hipGetLastError());
    return DPH_OK;
}

// the stored index as the reconstruct / window kernels read it
static pq_store pq_store_of(const dph_pq* p) {
    return pq_store{p->cent, p->pqc, p->codes, p->list_off, p->dm_ids, p->dm_pos, p->ntotal, p->nlist, p->M, p->dsub, p->by_residual};
}

int dph_pq_reconstruct_dev(dph_pq* p, const int64_t* ids_dev, int64_t n, float* out_dev, int32_t* found_dev, hipStream_t st) {
    if (!p || !p->finalized) return fail(DPH_E_STATE, "PQ reconstruct: index not finalized");
    HIPCHK(hipSetDevice(p->device));
    if (n <= 0) return DPH_OK;
    hipLaunchKernelGGL(pq_reconstruct_kernel, dim3((unsigned)n), dim3(256), 0, st, pq_store_of(p), ids_dev, n, out_dev, found_dev);
    HIPCHK(hipGetLastError());
    return DPH_OK;
}

// qrot = A q (no bias) of the n_q query halves of a window pass: what both PQ row sources take their dots with
static int pq_rotate_query_halves(dph_pq* p, const float* qhalf, int64_t n_q, hipStream_t st) {
    if (n_q > p->qrot_rows) {
        p->qrot_rows = 0;
        HIPCHK(p->qrot.alloc((size_t)n_q * DPH_DIM));
        p->qrot_rows = n_q;
    }
    pq_launch_transform(qhalf, p->At, n_q, nullptr, p->qrot, nullptr, nullptr, p->device, st);
    return DPH_OK;
}

// doc_rows = NULL: windows of reconstructions; otherwise over the raw int8 rows of whole documents (doc_rows [n_doc_rows,768] in
// f2o-CSR order, doc_lut = the single-rounding codec table)
int dph_pq_window(dph_pq* p, dph_window_args a, const int8_t* doc_rows, int64_t n_doc_rows, const float* doc_lut, hipStream_t st) {
    if (!p || !p->finalized) return fail(DPH_E_STATE, "PQ window: index not finalized");
    if (doc_rows && !doc_lut) return fail(DPH_E_STATE, "PQ window: no document rows attached");
    HIPCHK(hipSetDevice(p->device));
    if (a.n_cand <= 0) return DPH_OK;
    const int rc = pq_rotate_query_halves(p, a.qhalf, a.n_cand / a.k, st);
    if (rc) return rc;
    a.qhalf = p->qrot;
    const pq_store store = pq_store_of(p);
    p->prof.bracket(p->prof.on && p->prof_windows ? &p->win_events : nullptr, st,
                    [&] { dph_launch_window(a, &store, doc_rows, n_doc_rows, doc_lut, nullptr, st); });
    if (a.vecs && p->A) hipLaunchKernelGGL(pq_unrotate_kernel, dim3((unsigned)(2 * a.n_cand)), dim3(256), 0, st, a.vecs, p->A, 2 * a.n_cand);
    HIPCHK(hipGetLastError());
    return DPH_OK;
}
