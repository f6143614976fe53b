// dph_ivf.hip -- the coarse quantizer of the IVF path (BASELINE.json configs[3]: IVF-4096 + in-list exact IP).
// Replaces the IndexFlatIP coarse search inside faiss IndexIVF that the reference offloads to the GPU
// (/root/reference/densephrases/index.py:52-56, nprobe 256 at :53/:62; nlist up to 2^20: model.py:18): scores =
// q . centroid^T, the nprobe best lists per query row in (score desc, list id asc) order, emitted as a list-major bit
// mask for the scan.
//   dph_coarse_gemm_kernel   scores[q][l] = <x_q, c_l> on the matrix cores: v_mfma_f32_32x32x2_f32 (exact fp32 products,
//                            fp32 accumulation -- the f32-in MFMA runs at the fp32 vector rate, which is plenty: 412 GFLOP
//                            for 256 query rows x 2^20 lists), LDS-tiled 128 lists x 128 query rows per workgroup
//   dph_coarse_select_kernel one workgroup per query row: the nprobe-th largest fp32 score by a 3-pass radix select;
//                            lists clearly above it are probed, the lists within the fp32 error band around it are
//                            re-scored in fp64 and ranked (score desc, list id asc) -- so the probed SET is the one the
//                            float64 oracle (and FAISS up to its own rounding) picks, not merely a similar one
//   dph_tilemask_kernel      tilemask[tile] = listmask[list of tile] (32 B per 24 KiB tile: what the scan reads)
#include <stdio.h>
#include <algorithm>
#include "dph_internal.h"

typedef float v16f __attribute__((ext_vector_type(16)));

#define CG_LISTS 128        // lists per workgroup tile (4 waves x 32)
#define CG_QROWS 128        // query rows per workgroup tile (4 MFMA column blocks)
#define CG_KCHUNK 32        // k per LDS stage
#define CG_LD (CG_KCHUNK + 1)   // padded row stride (floats): lane&31 walks rows, so an odd stride is conflict-free

__global__ __launch_bounds__(256) void dph_coarse_gemm_kernel(const float* __restrict__ x, int q0, int n_q_host,
                                                              const int* __restrict__ gate, int gate_base,
                                                              const float* __restrict__ centroids, int nlist,
                                                              float* __restrict__ scores) {
    __shared__ float a_lds[CG_LISTS * CG_LD];
    __shared__ float b_lds[CG_QROWS * CG_LD];
    const int n_q = dph_gated_rows(gate, gate_base, n_q_host);
    const int qb0 = blockIdx.y * CG_QROWS;
    if (qb0 >= n_q) return;
    const int l0 = blockIdx.x * CG_LISTS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    v16f acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    for (int k0 = 0; k0 < DPH_DIM; k0 += CG_KCHUNK) {
        // stage: 128 rows x 32 floats each for centroids and queries: thread t loads float4 #(t&7) of rows t>>3 + 32*i
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = (tid >> 3) + 32 * i, c4 = (tid & 7) * 4;
            const int l = l0 + row, q = qb0 + row;
            const float4 av = l < nlist ? *(const float4*)(centroids + (int64_t)l * DPH_DIM + k0 + c4) : make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 bv = q < n_q ? *(const float4*)(x + (int64_t)(q0 + q) * DPH_DIM + k0 + c4) : make_float4(0.f, 0.f, 0.f, 0.f);
            float* ap = a_lds + row * CG_LD + c4;
            float* bp = b_lds + row * CG_LD + c4;
            ap[0] = av.x; ap[1] = av.y; ap[2] = av.z; ap[3] = av.w;
            bp[0] = bv.x; bp[1] = bv.y; bp[2] = bv.z; bp[3] = bv.w;
        }
        __syncthreads();
        // A[i = lane&31][k = lane>>5] = centroid row, B[k = lane>>5][j = lane&31] = query row (cdna_hip_programming.md section 3)
        const float* ap = a_lds + (wave * 32 + (lane & 31)) * CG_LD + (lane >> 5);
        const float* bp = b_lds + (lane & 31) * CG_LD + (lane >> 5);
#pragma unroll
        for (int kk = 0; kk < CG_KCHUNK; kk += 2) {
            const float a = ap[kk];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bp[j * 32 * CG_LD + kk], acc[j], 0, 0, 0);
        }
        __syncthreads();
    }
    // C[row i = (r&3) + 8*(r>>2) + 4*(lane>>5)][col j = lane&31]: i = list inside the wave's 32, j = query row of block jb
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int q = qb0 + j * 32 + (lane & 31);
        if (q >= n_q) continue;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int l = l0 + wave * 32 + 8 * g + 4 * (lane >> 5);
            float* o = scores + (int64_t)q * nlist + l;
            if (l + 3 < nlist && (nlist & 3) == 0) {
                *(float4*)o = make_float4(acc[j][4 * g], acc[j][4 * g + 1], acc[j][4 * g + 2], acc[j][4 * g + 3]);
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) if (l + r < nlist) o[r] = acc[j][4 * g + r];
            }
        }
    }
}

// ---- the same scores through the bf16 matrix cores, for the long coarse quantizers (the reference's 2^20 lists: 2*10^11 flop per
// 128 query rows is 2 ms at the f32 MFMA rate).  Every fp32 operand is split into two bf16 numbers, v = hi + lo + O(2^-16 |v|),
// and <x, c> is taken as hi*hi + hi*lo + lo*hi with three v_mfma_f32_32x32x16_bf16 per tile step (16x the f32-in rate each) into
// ONE fp32 accumulator: the dropped lo*lo and rounding residues are <= 3.1 * 2^-16 * ||x|| * ||c||, the accumulation of 2304
// products <= 2304 * 2^-24 * ||x|| * ||c|| -- the select kernel widens its float64 re-rank band by exactly that
// (CG_BF16X3_ERR), so the probed set stays the float64 oracle's.
typedef short v8s __attribute__((ext_vector_type(8)));
#define CG3_LD 40                    // bf16 per LDS row: 32 of the k-chunk + 8 of padding (80 B: 16-byte aligned, conflict-free)
#define CG_BF16X3_MIN (1 << 16)      // lists from which the bf16x3 kernel is used
#define CG_F32_ERR (768.0 * 5.97e-8)
#define CG_BF16X3_ERR (2304.0 * 5.97e-8 + 3.1 / 65536.0)

__device__ __forceinline__ unsigned short bf16_rne(float v) {
    const unsigned u = __float_as_uint(v);
    return (unsigned short)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
__device__ __forceinline__ void bf16_split(float v, unsigned short& hi, unsigned short& lo) {
    hi = bf16_rne(v);
    lo = bf16_rne(v - __uint_as_float((unsigned)hi << 16));        // exact difference, then rounded
}

// split of a whole fp32 matrix [n, 768] into its bf16 hi / lo parts (the centroids once per index, the rotated queries once per
// pass): with both operands pre-split the GEMM's staging is plain copies -- in-kernel splitting (~10 VALU ops per element and
// stage) kept the VALU busier than the matrix pipe
// (packed as hi << 16 | lo in one 32-bit word per element: the same 128-byte runs per row and k-chunk as the fp32 matrix, and
// two v_perm per pair of elements unpack them -- separate hi / lo arrays halved the run length and ran slower than splitting in
// the kernel)
__global__ __launch_bounds__(256) void dph_bf16_split_kernel(const float* __restrict__ v, int64_t n_elems, unsigned* __restrict__ packed) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_elems; i += (int64_t)gridDim.x * 256) {
        unsigned short hi, lo;
        bf16_split(v[i], hi, lo);
        packed[i] = ((unsigned)hi << 16) | (unsigned)lo;
    }
}
void dph_launch_bf16_split(const float* v, int64_t n_elems, unsigned* packed, hipStream_t st) {
    if (n_elems > 0)
        hipLaunchKernelGGL(dph_bf16_split_kernel, dim3((unsigned)std::min<int64_t>((n_elems + 255) / 256, 1 << 16)), dim3(256), 0, st, v, n_elems, packed);
}

__global__ __launch_bounds__(256) void dph_coarse_gemm_bf16x3_kernel(const float* __restrict__ x, int q0, int n_q_host,
                                                                     const int* __restrict__ gate, int gate_base,
                                                                     const float* __restrict__ centroids, int nlist,
                                                                     float* __restrict__ scores) {
    __shared__ __attribute__((aligned(16))) unsigned short a_hi[CG_LISTS * CG3_LD], a_lo[CG_LISTS * CG3_LD];
    __shared__ __attribute__((aligned(16))) unsigned short b_hi[CG_QROWS * CG3_LD], b_lo[CG_QROWS * CG3_LD];
    const int n_q = dph_gated_rows(gate, gate_base, n_q_host);
    const int qb0 = blockIdx.y * CG_QROWS;
    if (qb0 >= n_q) return;
    const int l0 = blockIdx.x * CG_LISTS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    v16f acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    for (int k0 = 0; k0 < DPH_DIM; k0 += CG_KCHUNK) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = (tid >> 3) + 32 * i, c4 = (tid & 7) * 4;
            const int l = l0 + row, q = qb0 + row;
            const float4 av = l < nlist ? *(const float4*)(centroids + (int64_t)l * DPH_DIM + k0 + c4) : make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 bv = q < n_q ? *(const float4*)(x + (int64_t)(q0 + q) * DPH_DIM + k0 + c4) : make_float4(0.f, 0.f, 0.f, 0.f);
            unsigned short h[4], lw[4];
            bf16_split(av.x, h[0], lw[0]); bf16_split(av.y, h[1], lw[1]); bf16_split(av.z, h[2], lw[2]); bf16_split(av.w, h[3], lw[3]);
            *(uint2*)(a_hi + row * CG3_LD + c4) = make_uint2((unsigned)h[0] | ((unsigned)h[1] << 16), (unsigned)h[2] | ((unsigned)h[3] << 16));
            *(uint2*)(a_lo + row * CG3_LD + c4) = make_uint2((unsigned)lw[0] | ((unsigned)lw[1] << 16), (unsigned)lw[2] | ((unsigned)lw[3] << 16));
            bf16_split(bv.x, h[0], lw[0]); bf16_split(bv.y, h[1], lw[1]); bf16_split(bv.z, h[2], lw[2]); bf16_split(bv.w, h[3], lw[3]);
            *(uint2*)(b_hi + row * CG3_LD + c4) = make_uint2((unsigned)h[0] | ((unsigned)h[1] << 16), (unsigned)h[2] | ((unsigned)h[3] << 16));
            *(uint2*)(b_lo + row * CG3_LD + c4) = make_uint2((unsigned)lw[0] | ((unsigned)lw[1] << 16), (unsigned)lw[2] | ((unsigned)lw[3] << 16));
        }
        __syncthreads();
        // A[i = lane&31][k = 8*(lane>>5) .. +7] = centroid row, B[k = 8*(lane>>5) .. +7][j = lane&31] = query row
        const int ko = 8 * (lane >> 5);
        const unsigned short* ap_h = a_hi + (wave * 32 + (lane & 31)) * CG3_LD + ko;
        const unsigned short* ap_l = a_lo + (wave * 32 + (lane & 31)) * CG3_LD + ko;
#pragma unroll
        for (int kk = 0; kk < CG_KCHUNK; kk += 16) {
            const v8s ah = *(const v8s*)(ap_h + kk), al = *(const v8s*)(ap_l + kk);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const v8s bh = *(const v8s*)(b_hi + (j * 32 + (lane & 31)) * CG3_LD + ko + kk);
                const v8s bl = *(const v8s*)(b_lo + (j * 32 + (lane & 31)) * CG3_LD + ko + kk);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[j], 0, 0, 0);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int q = qb0 + j * 32 + (lane & 31);
        if (q >= n_q) continue;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int l = l0 + wave * 32 + 8 * g + 4 * (lane >> 5);
            float* o = scores + (int64_t)q * nlist + l;
            if (l + 3 < nlist && (nlist & 3) == 0) {
                *(float4*)o = make_float4(acc[j][4 * g], acc[j][4 * g + 1], acc[j][4 * g + 2], acc[j][4 * g + 3]);
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) if (l + r < nlist) o[r] = acc[j][4 * g + r];
            }
        }
    }
}

// The pre-split form, software-pipelined: k-chunks of 64 (each MFMA step is fed from LDS twice as long per barrier), the NEXT
// chunk's global loads are issued into registers before the current chunk is multiplied, so HBM latency overlaps the matrix work
// inside a workgroup instead of relying on two co-resident workgroups (the plain form above: 16 % matrix-pipe utilisation).
#define CG3P_K 64
#define CG3P_LD 72                   // bf16 per LDS row: 64 + 8 of padding (144 B: 16-byte aligned, conflict-free for ds_read_b128)
__global__ __launch_bounds__(256, 2) void dph_coarse_gemm_bf16x3_pipe_kernel(int q0, int n_q_host, const int* __restrict__ gate, int gate_base,
                                                                             int nlist, float* __restrict__ scores,
                                                                             const unsigned* __restrict__ c_pk,
                                                                             const unsigned* __restrict__ x_pk) {
    extern __shared__ __attribute__((aligned(16))) unsigned short cg_lds[];       // a_hi | a_lo | b_hi | b_lo, each [128][CG3P_LD]
    unsigned short* const a_hi = cg_lds;
    unsigned short* const a_lo = a_hi + CG_LISTS * CG3P_LD;
    unsigned short* const b_hi = a_lo + CG_LISTS * CG3P_LD;
    unsigned short* const b_lo = b_hi + CG_QROWS * CG3P_LD;
    const int n_q = dph_gated_rows(gate, gate_base, n_q_host);
    const int qb0 = blockIdx.y * CG_QROWS;
    if (qb0 >= n_q) return;
    const int l0 = blockIdx.x * CG_LISTS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = tid & 15, row0 = tid >> 4;                    // 16 uint4 (64 packed elements) per row, rows row0 + 16 i
    v16f acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    uint4 ra[8], rb[8];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int row = row0 + 16 * i, l = l0 + row, q = qb0 + row;
            ra[i] = l < nlist ? *(const uint4*)(c_pk + (int64_t)l * DPH_DIM + k0 + 4 * col) : make_uint4(0u, 0u, 0u, 0u);
            rb[i] = q < n_q ? *(const uint4*)(x_pk + (int64_t)(q0 + q) * DPH_DIM + k0 + 4 * col) : make_uint4(0u, 0u, 0u, 0u);
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < DPH_DIM; k0 += CG3P_K) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int o = (row0 + 16 * i) * CG3P_LD + 4 * col;
            *(uint2*)(a_hi + o) = make_uint2(__builtin_amdgcn_perm(ra[i].y, ra[i].x, 0x07060302u), __builtin_amdgcn_perm(ra[i].w, ra[i].z, 0x07060302u));
            *(uint2*)(a_lo + o) = make_uint2(__builtin_amdgcn_perm(ra[i].y, ra[i].x, 0x05040100u), __builtin_amdgcn_perm(ra[i].w, ra[i].z, 0x05040100u));
            *(uint2*)(b_hi + o) = make_uint2(__builtin_amdgcn_perm(rb[i].y, rb[i].x, 0x07060302u), __builtin_amdgcn_perm(rb[i].w, rb[i].z, 0x07060302u));
            *(uint2*)(b_lo + o) = make_uint2(__builtin_amdgcn_perm(rb[i].y, rb[i].x, 0x05040100u), __builtin_amdgcn_perm(rb[i].w, rb[i].z, 0x05040100u));
        }
        __syncthreads();
        if (k0 + CG3P_K < DPH_DIM) fetch(k0 + CG3P_K);            // in flight while this chunk is multiplied
        const int ko = 8 * (lane >> 5);
        const unsigned short* ap_h = a_hi + (wave * 32 + (lane & 31)) * CG3P_LD + ko;
        const unsigned short* ap_l = a_lo + (wave * 32 + (lane & 31)) * CG3P_LD + ko;
#pragma unroll
        for (int kk = 0; kk < CG3P_K; kk += 16) {
            const v8s ah = *(const v8s*)(ap_h + kk), al = *(const v8s*)(ap_l + kk);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const v8s bh = *(const v8s*)(b_hi + (j * 32 + (lane & 31)) * CG3P_LD + ko + kk);
                const v8s bl = *(const v8s*)(b_lo + (j * 32 + (lane & 31)) * CG3P_LD + ko + kk);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[j], 0, 0, 0);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int q = qb0 + j * 32 + (lane & 31);
        if (q >= n_q) continue;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int l = l0 + wave * 32 + 8 * g + 4 * (lane >> 5);
            float* o = scores + (int64_t)q * nlist + l;
            if (l + 3 < nlist && (nlist & 3) == 0) {
                *(float4*)o = make_float4(acc[j][4 * g], acc[j][4 * g + 1], acc[j][4 * g + 2], acc[j][4 * g + 3]);
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) if (l + r < nlist) o[r] = acc[j][4 * g + r];
            }
        }
    }
}

__device__ __forceinline__ unsigned f32_key(float v) {          // order-preserving map to unsigned
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_f32(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

#define CS_THREADS 1024
#define CS_BPT (2048 / CS_THREADS)     // histogram bins per thread
#define CS_BAND_CAP 2048
#define CS_BROWS 6                   // band lists whose rows a wave has in flight together (float64 re-rank)
#define CS_SAMPLE 8192               // scores sampled for the threshold estimate of the one-pass path
#define CS_CAND 8192                 // candidates that path keeps in LDS (the filter form's wider band wants ~4 x nprobe + noise)
#define CS_FAST_MIN 8192             // lists from which the one-pass path is tried
// np-th largest of n order-preserving keys in three passes of 11 / 11 / 10 bits (2048-bin histogram in LDS).  `key_at(i)` reads
// key i; all CS_THREADS threads call it.  Keys fall into few distinct bins in the first pass (sign, exponent, two mantissa
// bits), so a wave first merges equal bins with ballots and issues ONE LDS atomic per distinct bin instead of 64 colliding ones.
template <class F>
__device__ __forceinline__ unsigned cs_select_kth(F key_at, int n, int want, unsigned* hist, unsigned* sh) {
    const int tid = threadIdx.x;
    unsigned prefix = 0, pmask = 0;
    const int shifts[3] = {21, 10, 0}, widths[3] = {11, 11, 10};
    for (int p = 0; p < 3; ++p) {
        for (int i = tid; i < 2048; i += CS_THREADS) hist[i] = 0;
        __syncthreads();
        const unsigned dm = (1u << widths[p]) - 1u;
        for (int i0 = 0; i0 < n; i0 += CS_THREADS) {
            const int i = i0 + tid;
            unsigned bin = 0xFFFFFFFFu;                  // not a member
            if (i < n) { const unsigned k = key_at(i); if ((k & pmask) == prefix) bin = (k >> shifts[p]) & dm; }
            // at most four merge rounds: keys spread over many bins (the later passes, a sample of a whole score row) are counted
            // one atomic per key after that -- 64 rounds of ballots per wave and trip otherwise (2 us per trip of 1024 keys)
            unsigned long long todo = __builtin_amdgcn_ballot_w64(bin != 0xFFFFFFFFu);
            for (int round = 0; round < 4 && todo; ++round) {
                const int leader = __builtin_ctzll(todo);
                const unsigned b = (unsigned)__builtin_amdgcn_readlane((int)bin, leader);
                const unsigned long long same = __builtin_amdgcn_ballot_w64(bin == b);
                if ((tid & 63) == leader) atomicAdd(&hist[b], (unsigned)__builtin_popcountll(same));
                todo &= ~same;
            }
            if ((todo >> (tid & 63)) & 1ull) atomicAdd(&hist[bin], 1u);
        }
        __syncthreads();
        {
            // the bin holding the want-th largest key: thread t owns bins CS_BPT t .. CS_BPT t + CS_BPT - 1, suffix sums from the
            // top bin down over the lanes (shuffles) and the waves (LDS) -- one thread walking 2048 bins cost 25 us per pass
            const int lane = tid & 63, wv = tid >> 6;
            unsigned h[CS_BPT];
            unsigned mine = 0;
#pragma unroll
            for (int u = 0; u < CS_BPT; ++u) { h[u] = hist[CS_BPT * tid + u]; mine += h[u]; }
            unsigned incl = mine;                                  // sum over this wave's lanes >= lane
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const unsigned v = __shfl_down(incl, o); if (lane + o < 64) incl += v; }
            if (lane == 0) sh[8 + wv] = incl;                      // the wave's total
            if (tid == 0) { sh[0] = 0; sh[1] = (unsigned)want; }   // (no bin reaches the rank: bin 0 takes it, as before)
            __syncthreads();
            unsigned above = incl - mine;
            for (int w = wv + 1; w < CS_THREADS / 64; ++w) above += sh[8 + w];
            if (above < (unsigned)want && (unsigned)want <= above + mine) {
                unsigned need = (unsigned)want - above;            // rank inside this thread's bins, counted from its top bin down
                int bin = CS_BPT * tid;
                unsigned acc = 0;
                bool found = false;
#pragma unroll
                for (int u = CS_BPT - 1; u >= 1; --u) {
                    if (!found && need <= acc + h[u]) { bin = CS_BPT * tid + u; need -= acc; found = true; }
                    acc += h[u];
                }
                if (!found) need -= acc;                           // the thread's lowest bin
                if (bin > 0) { sh[0] = (unsigned)bin; sh[1] = need; }
                else { sh[0] = 0; sh[1] = (unsigned)want - (above + acc); }
            }
        }
        __syncthreads();
        prefix |= sh[0] << shifts[p];
        pmask |= dm << shifts[p];
        want = (int)sh[1];
        __syncthreads();
    }
    return prefix;
}


// ---------------------------------------------------------------------------------------------------------------------
// Long quantizers, the filter in front of the chain.  The bf16x3 GEMM above reads 4 bytes per centroid component and writes a
// [rows, nlist] score matrix that two more passes read back (estimate + collect): at 2^20 lists that is 3.2 GB + 2 x 0.5 GB
// per batch of 64.  The probe set only needs the scores NEAR the nprobe-th one exactly, so the first pass is a FILTER:
//   * the centroids once more as plain bf16 (the hi parts: 2 bytes per component, 1.6 GB at 2^20 lists), the rotated queries
//     likewise; <x~, c~> with ONE v_mfma_f32_32x32x16_bf16 per tile step.  |<x~,c~> - <x,c>| <= (2^-8 + 2^-18) sum|x_j c_j|
//     (two roundings to 8 significant bits) + the fp32 accumulation <= CF_HI_ERR * ||x|| * ||c||;
//   * a threshold estimate per query row from the scores of every (nlist/8192)-th list (dph_coarse_sample_gemm_kernel reads
//     12.6 MB of the chunk-major image, dph_coarse_estimate_sample_kernel takes the order statistic), chosen so that
//     ~4-5 x nprobe lists beat it;
//   * the filter itself is a SCAN of the piece-major image (dph_scan.hip MODE 3, MODE 4 for teams): every score at or above its
//     row's estimate leaves as a (list | query row << 20, key) pair in a chunk of the pair pool -- the score matrix is never
//     written;
//   * dph_coarse_bucket_chunks_kernel deals the chunks into per-row candidate lists, dph_coarse_select_kernel selects the
//     nprobe-th candidate, marks what is clearly above the error band and re-ranks the band in float64 exactly as before -- the
//     band is wider (the 2^-8 error: a few hundred lists around the 256-th of 2^20), which is what the float64 re-rank is for.
// A row whose estimate was too high (fewer than nprobe candidates, or the band reaching below it), whose candidates or band
// overflow, fails the whole pass over to the bf16x3 chain (gated on the device: no host round trip; empty launches otherwise).
// (Rounds 4-5 also had four GEMM forms of the filter, the threshold test in their epilogue: measured and removed, DESIGN_HISTORY.md.)
#define CF_K 128                     // k-chunk of the sample GEMM = one run of the chunk-major centroid image
#define CF_HI_ERR (1.0 / 256.0 + 1.0 / 262144.0 + 800.0 * 5.97e-8)
#define CF_SAMPLE 8192               // lists of the threshold sample

// The bf16 image of the centroids [n, 768] the sample GEMM reads (the query rows of a pass are plain row-major bf16).
// CHUNK-MAJOR -- [k-chunk of 128][tile of 128 rows][row][k]: the 32 KiB of a tile and k-chunk are one contiguous run, and the runs of
// the tiles w, w+1, ... of one k-chunk follow each other.  (The layout was chosen for the GEMM form of the filter, which streamed all
// of it: row-major, a step gathered 128 pieces of 256 B at a stride of 1536 B; tile-major, [tile][k-chunk]..., was three times slower
// than that.)  Rows past n in the last tile are written as zeros (the allocation holds whole tiles).
__host__ __device__ inline int64_t dph_cf_tiled_index(int64_t row, int k, int64_t n_tiles) {
    return ((int64_t)(k / CF_K) * n_tiles + row / CG_LISTS) * (int64_t)(CG_LISTS * CF_K) + (row % CG_LISTS) * CF_K + k % CF_K;
}
__global__ __launch_bounds__(256) void dph_bf16_hi_kernel(const float* __restrict__ v, int64_t n_rows, int64_t n_rows_padded,
                                                          unsigned short* __restrict__ hi) {
    const int64_t n_elems = n_rows_padded * DPH_DIM;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_elems; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / DPH_DIM;
        const int k = (int)(i % DPH_DIM);
        hi[dph_cf_tiled_index(row, k, n_rows_padded / CG_LISTS)] = row < n_rows ? bf16_rne(v[i]) : (unsigned short)0;
    }
}
int64_t dph_bf16_hi_rows(int64_t n_rows) { return (n_rows + CG_LISTS - 1) / CG_LISTS * CG_LISTS; }
void dph_launch_bf16_hi(const float* v, int64_t n_rows, unsigned short* hi, hipStream_t st) {
    const int64_t n_elems = dph_bf16_hi_rows(n_rows) * DPH_DIM;
    if (n_elems > 0)
        hipLaunchKernelGGL(dph_bf16_hi_kernel, dim3((unsigned)std::min<int64_t>((n_elems + 255) / 256, 1 << 16)), dim3(256), 0, st, v, n_rows,
                           dph_bf16_hi_rows(n_rows), hi);
}

// The sample GEMM: sample_scores[q][i] = <x~_q, c~_l> for the lists l = i * list_stride, i < n_lists.
// Persistent workgroups (two per CU: grid.x = 2 x CUs, or fewer tiles): workgroup w multiplies the tiles of 128 sampled lists w,
// w + grid.x, ... as ONE stream of k-chunks of 128 -- the centroid chunk two steps ahead and the query chunk one step ahead are in
// flight in registers while the current chunk is multiplied out of LDS, across tile boundaries (the epilogue of a tile runs under the
// next tile's loads).
typedef unsigned cf_v4u __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256, 2) void dph_coarse_sample_gemm_kernel(int n_q, int n_lists, int list_stride, int64_t image_tiles,
                                                                        const unsigned short* __restrict__ c_hi,
                                                                        const unsigned short* __restrict__ x_hi,
                                                                        float* __restrict__ sample_scores) {
    constexpr int CK = CF_K;
    constexpr int LD = CK + 8;                                    // bf16 per LDS row (CK + 8 of padding: 16-byte aligned rows, conflict-free ds_read_b128)
    constexpr int NF = CK / 16;                                   // uint4 per thread and operand per chunk (256 threads, 128 rows of CK bf16)
    constexpr int CPR = CK / 8;                                   // uint4 per row
    constexpr int NCH = DPH_DIM / CK;                             // chunks per tile
    extern __shared__ __attribute__((aligned(16))) unsigned short cf_lds[];       // a | b, each [128][LD]
    unsigned short* const a_s = cf_lds;
    unsigned short* const b_s = a_s + CG_LISTS * LD;
    const int qb0 = blockIdx.y * CG_QROWS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = tid % CPR, row0 = tid / CPR;                  // rows row0 + (256 / CPR) i
    constexpr int RSTEP = 256 / CPR;
    const int n_tiles = (n_lists + CG_LISTS - 1) / CG_LISTS;
    const int my_tiles = (int)blockIdx.x < n_tiles ? (n_tiles - 1 - (int)blockIdx.x) / (int)gridDim.x + 1 : 0;
    const int n_chunks = my_tiles * NCH;                          // of this workgroup's stream
    v16f acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    // staging registers: the centroid chunks two steps ahead (RA0 / RA1 alternate) and the query chunk one step ahead.  Plain named
    // arrays touched through MACROS with constant indices: behind a reference parameter of a lambda hipcc left them in scratch
    // memory (256 bytes per thread, every chunk through it: the GEMM took 1.19 ms instead of 0.4)
    cf_v4u ra0[NF], ra1[NF], rb[NF];        // (native vectors: arrays of HIP's uint4 struct were not always split into registers either)
#define CF_FETCH_A(RA, C)                                                                                                        \
    do {                                                                                                                         \
        const int c_ = (C);                                                                                                      \
        const int l0_ = ((int)blockIdx.x + (c_ / NCH) * (int)gridDim.x) * CG_LISTS, k0_ = (c_ % NCH) * CK;                        \
        /* the sample's lists are every list_stride-th list of the index: 256-byte pieces of the chunk-major image */            \
        _Pragma("unroll") for (int i = 0; i < NF; ++i) {                                                                         \
            const int l = l0_ + row0 + RSTEP * i;                                                                                \
            RA[i] = l < n_lists ? *(const cf_v4u*)(c_hi + dph_cf_tiled_index((int64_t)l * list_stride, k0_ + 8 * col, image_tiles))\
                                : cf_v4u{0u, 0u, 0u, 0u};                                                                        \
        }                                                                                                                        \
    } while (0)
    auto fetch_b = [&](int c) __attribute__((always_inline)) {
        const int k0 = (c % NCH) * CK;
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            const int q = qb0 + row0 + RSTEP * i;
            rb[i] = q < n_q ? *(const cf_v4u*)(x_hi + (int64_t)q * DPH_DIM + k0 + 8 * col) : cf_v4u{0u, 0u, 0u, 0u};
        }
    };
    // (always_inline: as an out-of-line call the lambda takes the accumulators by reference, i.e. through scratch memory -- 3x the kernel time)
    auto epilogue = [&](int tile) __attribute__((always_inline)) {
        const int l0 = tile * CG_LISTS;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int q = qb0 + j * 32 + (lane & 31);
            if (q >= n_q) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int l = l0 + wave * 32 + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
                if (l < n_lists) sample_scores[(int64_t)q * n_lists + l] = acc[j][r];
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    };
    // one chunk: stage it (the centroid registers first, re-loaded at once), multiply, and at a tile's last chunk run its epilogue
#define CF_STEP(RA, C)                                                                                                           \
    do {                                                                                                                         \
        const int cc_ = (C);                                                                                                     \
        _Pragma("unroll") for (int i = 0; i < NF; ++i) *(cf_v4u*)(a_s + (row0 + RSTEP * i) * LD + 8 * col) = RA[i];                \
        if (cc_ + 2 < n_chunks) CF_FETCH_A(RA, cc_ + 2);                                                                         \
        _Pragma("unroll") for (int i = 0; i < NF; ++i) *(cf_v4u*)(b_s + (row0 + RSTEP * i) * LD + 8 * col) = rb[i];                \
        if (cc_ + 1 < n_chunks) fetch_b(cc_ + 1);                                                                                \
        __syncthreads();                                                                                                         \
        const int ko = 8 * (lane >> 5);                                                                                          \
        const unsigned short* ap = a_s + (wave * 32 + (lane & 31)) * LD + ko;                                                    \
        _Pragma("unroll") for (int kk = 0; kk < CK; kk += 16) {                                                                  \
            const v8s a = *(const v8s*)(ap + kk);                                                                                \
            _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                                      \
                const v8s b = *(const v8s*)(b_s + (j * 32 + (lane & 31)) * LD + ko + kk);                                        \
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[j], 0, 0, 0);                                         \
            }                                                                                                                    \
        }                                                                                                                        \
        __syncthreads();                                                                                                         \
        if (cc_ % NCH == NCH - 1) epilogue((int)blockIdx.x + (cc_ / NCH) * (int)gridDim.x);                                      \
    } while (0)
    if (n_chunks == 0) return;
    CF_FETCH_A(ra0, 0);
    CF_FETCH_A(ra1, 1);                                              // (NCH >= 2: chunk 1 exists)
    fetch_b(0);
    for (int c = 0; c < n_chunks; c += 2) {                          // NCH is even: the stream has an even number of chunks
        CF_STEP(ra0, c);
        CF_STEP(ra1, c + 1);
    }
#undef CF_STEP
#undef CF_FETCH_A
}

// ---- the filter as a SCAN (dph_scan.hip MODE 3): the centroids as 24 KiB pieces with the byte layout
// of an int8 tile -- [tile of 32 lists][half of k][32 rows][384 bf16] -- streamed by the flat scan's feed at the flat scan's rate.
__global__ __launch_bounds__(256) void dph_bf16_pieces_kernel(const float* __restrict__ v, int64_t n_rows, int64_t n_rows_padded,
                                                              unsigned short* __restrict__ out) {
    const int64_t n_elems = n_rows_padded * DPH_DIM;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_elems; i += (int64_t)gridDim.x * 256) {
        // out index i = ((tile * 2 + half) * 32 + r) * 384 + kk
        const int kk = (int)(i % 384), r = (int)((i / 384) % 32), half = (int)((i / (384 * 32)) % 2);
        const int64_t tile = i / (384 * 32 * 2), row = tile * 32 + r;
        out[i] = row < n_rows ? bf16_rne(v[row * DPH_DIM + 384 * half + kk]) : (unsigned short)0;
    }
}
int64_t dph_bf16_piece_rows(int64_t n_rows) { return (n_rows + 31) / 32 * 32; }
void dph_launch_bf16_pieces(const float* v, int64_t n_rows, unsigned short* out, hipStream_t st) {
    const int64_t n_elems = dph_bf16_piece_rows(n_rows) * DPH_DIM;
    if (n_elems > 0)
        hipLaunchKernelGGL(dph_bf16_pieces_kernel, dim3((unsigned)std::min<int64_t>((n_elems + 255) / 256, 1 << 16)), dim3(256), 0, st, v, n_rows,
                           dph_bf16_piece_rows(n_rows), out);
}
// query fragments of a pass of <= 128 rows for that scan: [group of 32 rows][half][k-step of 16][lane][8 bf16], lane l = query row
// 32 g + (l & 31), k = 384 half + 16 ks + 8 (l >> 5) .. +7 -- the B operand of v_mfma_f32_32x32x16_bf16 as the wave loads it.
// (Round 6 tried v_mfma_f32_16x16x32_bf16 here as well -- the shape that took 8 % off the int8 256-row pass: bit-identical pools, and no
// faster: coarse stage 0.306 / 1.045 / 1.993 ms at batch 64 / 256 / 512 against 0.289 / 1.004 / 1.86-1.97.  Not kept.)
// (n_groups > 1, the teams form: the blocks of all groups of 128 rows one after the other, g counts on through them)
__global__ __launch_bounds__(256) void dph_cf_qfrag_kernel(const unsigned short* __restrict__ x_hi, int n_q, uint4* __restrict__ qfrag, int n_groups = 1) {
    const int i = blockIdx.x * 256 + threadIdx.x;              // one 16-byte fragment each: 4 * 2 * 24 * 64 of them per group of 128 rows
    if (i >= n_groups * 4 * 2 * 24 * 64) return;
    const int lane = i % 64, ks = (i / 64) % 24, half = (i / (64 * 24)) % 2, g = i / (64 * 24 * 2);
    const int q = 32 * g + (lane & 31), k = 384 * half + 16 * ks + 8 * (lane >> 5);
    qfrag[i] = q < n_q ? *(const uint4*)(x_hi + (int64_t)q * DPH_DIM + k) : make_uint4(0u, 0u, 0u, 0u);
}

#define CB_THREADS 512
// The chunks the filter scan claimed from its pair pool -> per-row candidate lists [row][cand_cap] (list, key) + counts.  A workgroup
// takes a contiguous range of chunks, a wave a chunk at a time; it counts its rows in LDS, reserves each row's run with one global
// atomic and scatters: n_wg x rows atomics instead of one per pair.  pool_count only keeps the statistic (dph_debug_pq_coarse).
__global__ __launch_bounds__(CB_THREADS) void dph_coarse_bucket_chunks_kernel(const uint2* __restrict__ pairs, const unsigned* __restrict__ chunk_fill,
                                                                              const int* __restrict__ counters, int n_q_total, unsigned q_base,
                                                                              uint2* __restrict__ cand_glob, unsigned* __restrict__ cand_cnt, int cand_cap,
                                                                              unsigned* __restrict__ pool_count, unsigned* __restrict__ fail) {
    __shared__ unsigned cnt[DPH_PASS_MAX];
    __shared__ unsigned base[DPH_PASS_MAX];
    __shared__ unsigned total;
    const int tid = threadIdx.x;
    const unsigned lane = tid & 63u, wave = (unsigned)tid >> 6, n_waves = CB_THREADS / 64;
    const unsigned claimed = (unsigned)counters[1];
    const unsigned used = claimed < (unsigned)DPH_POOL_CHUNKS ? claimed : (unsigned)DPH_POOL_CHUNKS;
    if (blockIdx.x == 0 && tid == 0 && (claimed > (unsigned)DPH_POOL_CHUNKS || counters[2] != 0)) atomicOr(fail, 1u);
    const unsigned per = (used + gridDim.x - 1) / gridDim.x;
    const unsigned lo = blockIdx.x * per, hi = lo + per < used ? lo + per : used;
    for (int i = tid; i < n_q_total; i += CB_THREADS) cnt[i] = 0;
    if (tid == 0) total = 0;
    __syncthreads();
    unsigned mine = 0;
    for (unsigned ch = lo + wave; ch < hi; ch += n_waves) {
        const unsigned raw = chunk_fill[ch];
        const unsigned n = raw < (unsigned)DPH_CHUNK_PAIRS ? raw : (unsigned)DPH_CHUNK_PAIRS;
        mine += n;
#pragma unroll
        for (unsigned i0 = 0; i0 < (unsigned)DPH_CHUNK_PAIRS; i0 += 64u)
            if (i0 + lane < n) atomicAdd(&cnt[q_base + (pairs[(size_t)ch * DPH_CHUNK_PAIRS + i0 + lane].x >> 20)], 1u);
    }
    if (lane == 0 && mine) atomicAdd(&total, mine);
    __syncthreads();
    for (int i = tid; i < n_q_total; i += CB_THREADS) { base[i] = cnt[i] ? atomicAdd(&cand_cnt[i], cnt[i]) : 0u; cnt[i] = 0; }
    if (tid == 0 && total) atomicAdd(pool_count, total);
    __syncthreads();
    for (unsigned ch = lo + wave; ch < hi; ch += n_waves) {
        const unsigned raw = chunk_fill[ch];
        const unsigned n = raw < (unsigned)DPH_CHUNK_PAIRS ? raw : (unsigned)DPH_CHUNK_PAIRS;
#pragma unroll
        for (unsigned i0 = 0; i0 < (unsigned)DPH_CHUNK_PAIRS; i0 += 64u)
            if (i0 + lane < n) {
                const uint2 pr = pairs[(size_t)ch * DPH_CHUNK_PAIRS + i0 + lane];
                const unsigned q = q_base + (pr.x >> 20);
                const unsigned slot = base[q] + atomicAdd(&cnt[q], 1u);
                if (slot < (unsigned)cand_cap) cand_glob[(int64_t)q * cand_cap + slot] = make_uint2(pr.x & 0xFFFFFu, pr.y);
            }
    }
}

// threshold estimate of every row from its sample scores [n_q][m] (lists i * stride): the smallest sample rank r whose population count
// r * stride is >= target at -3 sigma
__global__ __launch_bounds__(CS_THREADS) void dph_coarse_estimate_sample_kernel(const float* __restrict__ sample_scores, int n_q, int m, int stride,
                                                                                int target, unsigned* __restrict__ est_out) {
    __shared__ unsigned hist[2048];
    __shared__ unsigned sh[32];
    __shared__ unsigned smp[CF_SAMPLE];
    const int qi = blockIdx.x;
    if (qi >= n_q) return;
    const int tid = threadIdx.x;
    for (int i = tid; i < m; i += CS_THREADS) smp[i] = f32_key(sample_scores[(int64_t)qi * m + i]);
    __syncthreads();
    int r = 1;
    while (((double)r - 3.0 * sqrt((double)r)) * (double)stride < (double)target && r < m) ++r;
    const unsigned est = cs_select_kth([&](int i) { return smp[i]; }, m, r, hist, sh);
    if (tid == 0) est_out[qi] = est;
}

// gate of the fail-over chain: all rows of the pass when any row (or the pool) failed, none otherwise
__global__ void dph_coarse_gate_kernel(const unsigned* __restrict__ fail, int n_q, int* __restrict__ gate_out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) gate_out[0] = fail[0] ? n_q : 0;
}

// Long score rows, first half of the one-pass path: dph_coarse_estimate_kernel takes the threshold estimate of every row from a
// strided sample, dph_coarse_collect_kernel spreads the pass over the row across several workgroups (one workgroup streams its
// 4 MiB row at HBM latency: 0.6 ms for 128 rows x 2^20 lists) that append the scores at or above the estimate to the row's
// candidate list in global memory; dph_coarse_select_kernel then works on the candidates only.
__global__ __launch_bounds__(CS_THREADS) void dph_coarse_estimate_kernel(const float* __restrict__ scores, int n_q_host,
                                                                         const int* __restrict__ gate, int gate_base, int nlist, int nprobe,
                                                                         unsigned* __restrict__ est_out) {
    __shared__ unsigned hist[2048];
    __shared__ unsigned sh[32];
    __shared__ unsigned smp[CS_SAMPLE];
    const int n_q = dph_gated_rows(gate, gate_base, n_q_host);
    const int qi = blockIdx.x;
    if (qi >= n_q) return;
    const int tid = threadIdx.x;
    const float* s = scores + (int64_t)qi * nlist;
    const int np = nprobe < nlist ? nprobe : nlist;
    const int stride = nlist / CS_SAMPLE > 0 ? nlist / CS_SAMPLE : 1;
    const int m = nlist / stride < CS_SAMPLE ? nlist / stride : CS_SAMPLE;
    for (int i = tid; i < m; i += CS_THREADS) smp[i] = f32_key(s[(int64_t)i * stride]);
    __syncthreads();
    int r = 1;                                       // smallest sample rank whose population count is >= np at -3 sigma
    while (((double)r - 3.0 * sqrt((double)r)) * (double)stride < (double)np && r < m) ++r;
    const unsigned est = cs_select_kth([&](int i) { return smp[i]; }, m, r, hist, sh);
    if (tid == 0) est_out[qi] = est;
}

__global__ __launch_bounds__(CS_THREADS) void dph_coarse_collect_kernel(const float* __restrict__ scores, int n_q_host,
                                                                        const int* __restrict__ gate, int gate_base, int nlist,
                                                                        uint2* __restrict__ cand_glob, unsigned* __restrict__ cand_cnt,
                                                                        const unsigned* __restrict__ est_in) {
    __shared__ unsigned sh[32];
    __shared__ unsigned smp[CS_SAMPLE];             // this workgroup's candidates (CS_SAMPLE / 2 pairs)
    const int n_q = dph_gated_rows(gate, gate_base, n_q_host);
    const int qi = blockIdx.x, slice = blockIdx.y, n_slices = gridDim.y;
    if (qi >= n_q) return;
    const int tid = threadIdx.x;
    const float* s = scores + (int64_t)qi * nlist;
    const unsigned est = est_in[qi];
    // candidates go to LDS first and to the row's global list with ONE atomic per workgroup: thousands of returning atomics on
    // counters that share cache lines serialise in the L2 (measured: 0.9 ms for 128 rows)
    uint2* const loc = (uint2*)smp;
    constexpr unsigned LOC_CAP = CS_SAMPLE / 2;
    if (tid == 0) sh[4] = 0;
    __syncthreads();                                 // (also: everybody is done reading the sample)
    auto take = [&](float v, int i) {
        const unsigned k = f32_key(v);
        if (k >= est) { const unsigned slot = atomicAdd(&sh[4], 1u); if (slot < LOC_CAP) loc[slot] = make_uint2((unsigned)i, k); }
    };
    const int per = ((nlist + n_slices - 1) / n_slices + 3) & ~3;
    const int i_lo = slice * per, i_hi = min(nlist, i_lo + per);
    if ((nlist & 3) == 0 && (((uintptr_t)s) & 15) == 0) {
        const float4* s4 = (const float4*)s;
        const int a4 = i_lo / 4, b4 = (i_hi > i_lo ? i_hi : i_lo) / 4;        // i_lo is a multiple of 4, i_hi too (nlist and per are)
        for (int i0 = a4; i0 < b4; i0 += 4 * CS_THREADS) {
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { const int i = i0 + u * CS_THREADS + tid; v[u] = i < b4 ? s4[i] : make_float4(-3.4e38f, -3.4e38f, -3.4e38f, -3.4e38f); }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = i0 + u * CS_THREADS + tid;
                if (i < b4) { take(v[u].x, 4 * i); take(v[u].y, 4 * i + 1); take(v[u].z, 4 * i + 2); take(v[u].w, 4 * i + 3); }
            }
        }
    } else {
        for (int i = i_lo + tid; i < i_hi; i += CS_THREADS) take(s[i], i);
    }
    __syncthreads();
    const unsigned n_loc = sh[4];
    if (tid == 0) sh[5] = atomicAdd(&cand_cnt[qi], n_loc > LOC_CAP ? (unsigned)(2 * CS_CAND) : n_loc);      // too many here: the row falls back
    __syncthreads();
    const unsigned base = sh[5];
    if (n_loc <= LOC_CAP)
        for (unsigned i = tid; i < n_loc; i += CS_THREADS) if (base + i < CS_CAND) cand_glob[(int64_t)qi * CS_CAND + base + i] = loc[i];
}

// debugging (dph_debug_pq_phases, which = 1): 100 MHz stamps of dph_coarse_select_kernel per query row of its last launch with rows --
// start, query norm, candidates in LDS, nprobe-th candidate, marking, float64 band dots, band ranks; [7] = band | candidates << 16 | need << 40
__device__ unsigned long long dph_cs_clock[DPH_PASS_MAX * 8];
__device__ int dph_cs_clock_on;
int dph_coarse_select_clock(unsigned long long* out, int cap_rows) {
    const int on = 1;                                    // (armed by every call, read or not)
    if (hipMemcpyToSymbol(HIP_SYMBOL(dph_cs_clock_on), &on, sizeof on) != hipSuccess) return -1;
    const int n = cap_rows < DPH_PASS_MAX ? cap_rows : DPH_PASS_MAX;
    if (out && n > 0 && hipMemcpyFromSymbol(out, HIP_SYMBOL(dph_cs_clock), (size_t)n * 64) != hipSuccess) return -1;
    return DPH_PASS_MAX;
}

// The nprobe lists of a query row.  Short lists of scores (nlist < CS_FAST_MIN): radix select over the whole score row
// (three passes) + one marking pass.  Long ones (the reference's 2^20 lists): ONE pass -- a strided sample of CS_SAMPLE
// scores gives a threshold estimate that ~8 x nprobe scores beat (an order statistic of the sample: the count above it is
// nprobe .. CS_CAND with overwhelming probability), one pass collects those candidates into LDS, and select + marking run on
// the candidates; whenever the estimate turns out too high, too low, or closer to the nprobe-th score than the fp32 error
// band, the row falls back to the full passes.  Either way the lists inside the band are re-ranked in float64.
__global__ __launch_bounds__(CS_THREADS) void dph_coarse_select_kernel(
    const float* __restrict__ x, int q0, int n_q_host, const int* __restrict__ gate, int gate_base,
    const float* __restrict__ centroids, const float* __restrict__ scores, int nlist, int nprobe, double cnorm_max,
    unsigned* __restrict__ listmask, int mask_words, int* __restrict__ probe_out, int probe_stride, double err_rel,
    const uint2* __restrict__ cand_glob, const unsigned* __restrict__ cand_cnt, const unsigned* __restrict__ est_in,
    unsigned* __restrict__ fail_out, unsigned* __restrict__ row_fail, const float* __restrict__ cnorm = nullptr, double cnorm_cap = 0.0) {
    __shared__ unsigned hist[2048];
    __shared__ float q_lds[DPH_DIM];
    __shared__ int band_id[CS_BAND_CAP];
    __shared__ double band_s[CS_BAND_CAP];
    __shared__ unsigned sh[32];
    __shared__ double qn_sh[CS_THREADS / 64];
    extern __shared__ unsigned cs_dyn[];             // [CS_CAND] candidate ids | [CS_CAND] keys
    const int n_q = dph_gated_rows(gate, gate_base, n_q_host);
    const int qi = blockIdx.x;
    if (qi >= n_q) return;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const bool clk = tid == 0 && dph_cs_clock_on != 0;
    auto stamp = [&](int slot) __attribute__((always_inline)) { if (clk) dph_cs_clock[qi * 8 + slot] = wall_clock64(); };
    stamp(0);
    const float* s = scores + (int64_t)qi * nlist;
    const int np = nprobe < nlist ? nprobe : nlist;
    double qn = 0.0;
    for (int j = tid; j < DPH_DIM; j += CS_THREADS) { const float v = x[(int64_t)(q0 + qi) * DPH_DIM + j]; q_lds[j] = v; qn += (double)v * v; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) qn += __shfl_xor(qn, o);
    if (lane == 0) qn_sh[wv] = qn;
    __syncthreads();
    double qnorm = 0.0;
    for (int w = 0; w < CS_THREADS / 64; ++w) qnorm += qn_sh[w];
    // |MFMA dot - exact| <= err_rel * ||x|| * max||c|| (f32-in: 768 * 2^-24 * sum|x_j c_j|; bf16x3 and the one-product filter: see
    // the kernels; the callers fold their slack into err_rel)
    // HEAVY lists (round 6).  The bound is per list: err_rel * ||x|| * ||c_l||.  A quantizer trained on token vectors has a few
    // centroids several times longer than the rest -- and under inner product exactly those crowd the top of every score row.  With
    // max||c|| for every list the band grew with the ONE longest centroid (x 2.4: the band overflowed and every pass failed over to
    // the bf16x3 chain, 1.3 ms per 128 rows).  So: lists with ||c_l|| > cnorm_cap (the caller's choice, ~1.1 x the 99-th percentile)
    // are heavy; a heavy CANDIDATE gets its exact float64 score at once (a few dozen 3 KiB rows per query row) in place of its
    // estimate -- error ~0 <= delta -- and the band logic below runs with delta from cnorm_cap.  Heavy lists OUTSIDE the candidate
    // set are covered by the pool test: est + delta_max must stay below the band (`fast`).
    const bool heavy_on = cnorm != nullptr && cnorm_cap > 0.0 && cnorm_cap < cnorm_max;
    const float delta = (float)(err_rel * sqrt(qnorm) * (heavy_on ? cnorm_cap : cnorm_max)) + 1e-30f;
    const float delta_max = (float)(err_rel * sqrt(qnorm) * cnorm_max) + 1e-30f;
    stamp(1);
    const unsigned word = (unsigned)qi >> 5, bitv = 1u << (qi & 31);
    int* const cand_id = (int*)cs_dyn;
    unsigned* const cand_key = cs_dyn + CS_CAND;
    bool fast = false;
    float t = 0.f;
    int n_cand = 0;
    if (nlist >= CS_FAST_MIN && cand_glob) {
        // ---- candidates collected by dph_coarse_collect_kernel (every score at or above its sampled estimate)
        const unsigned est = est_in[qi];
        n_cand = (int)cand_cnt[qi];
        if (n_cand <= CS_CAND)
            for (int i = tid; i < n_cand; i += CS_THREADS) { const uint2 c = cand_glob[(int64_t)qi * CS_CAND + i]; cand_id[i] = (int)c.x; cand_key[i] = c.y; }
        __syncthreads();
        bool heavy_ok = true;
        if (heavy_on && n_cand <= CS_CAND) {
            // exact scores for the heavy candidates (their positions collected in band_id, CS_BROWS rows per wave in flight)
            if (tid == 0) sh[6] = 0;
            __syncthreads();
            for (int i = tid; i < n_cand; i += CS_THREADS)
                if (cnorm[cand_id[i]] > (float)cnorm_cap) { const unsigned b = atomicAdd(&sh[6], 1u); if (b < CS_BAND_CAP) band_id[b] = i; }
            __syncthreads();
            const int nh = (int)sh[6];
            heavy_ok = nh <= CS_BAND_CAP;
            for (int b0 = wv * CS_BROWS; heavy_ok && b0 < nh; b0 += (CS_THREADS / 64) * CS_BROWS) {
                float cv[CS_BROWS][12];
#pragma unroll
                for (int u = 0; u < CS_BROWS; ++u) {
                    const int b = b0 + u < nh ? b0 + u : nh - 1;
                    const float4* cp = (const float4*)(centroids + (int64_t)cand_id[band_id[b]] * DPH_DIM + lane * 12);
                    const float4 c0 = cp[0], c1 = cp[1], c2 = cp[2];
                    cv[u][0] = c0.x; cv[u][1] = c0.y; cv[u][2] = c0.z; cv[u][3] = c0.w; cv[u][4] = c1.x; cv[u][5] = c1.y; cv[u][6] = c1.z; cv[u][7] = c1.w;
                    cv[u][8] = c2.x; cv[u][9] = c2.y; cv[u][10] = c2.z; cv[u][11] = c2.w;
                }
#pragma unroll
                for (int u = 0; u < CS_BROWS; ++u) {
                    double acc = 0.0;
#pragma unroll
                    for (int j = 0; j < 12; ++j) acc += (double)q_lds[lane * 12 + j] * (double)cv[u][j];
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
                    if (lane == 0 && b0 + u < nh) cand_key[band_id[b0 + u]] = f32_key((float)acc);
                }
            }
            __syncthreads();
        }
        stamp(2);
        if (heavy_ok && n_cand >= np && n_cand <= CS_CAND) {
            const unsigned kth = cs_select_kth([&](int i) { return cand_key[i]; }, n_cand, np, hist, sh);
            t = key_f32(kth);
            // the whole error band lies inside the candidate set: a list outside it has estimate < est, hence score < est + delta_max,
            // and the true nprobe-th score is >= t - delta
            fast = (t - delta - delta_max) >= key_f32(est);
        }
    }
    if (!fast && !scores) {                          // filter form: there is no score matrix to fall back on -- the pass fails over
        if (tid == 0 && fail_out) atomicOr(fail_out, 1u);
        return;
    }
    if (!fast) t = key_f32(cs_select_kth([&](int i) { return f32_key(s[i]); }, nlist, np, hist, sh));
    const float hi = t + 2.f * delta, lo = t - 2.f * delta;
    stamp(3);
    // ---- lists clearly above the band are probed; the band is collected for the fp64 re-rank
    if (tid == 0) { sh[2] = 0; sh[3] = 0; sh[5] = 0; }
    __syncthreads();
    if (probe_out) {
        for (int i = tid; i < probe_stride; i += CS_THREADS) probe_out[(int64_t)qi * probe_stride + i] = -1;
        __syncthreads();                              // (block-uniform branch) the fills land before any real entry
    }
    unsigned n_in = 0;
    const int n_mark = fast ? n_cand : nlist;
    for (int i = tid; i < n_mark; i += CS_THREADS) {
        const int l = fast ? cand_id[i] : i;
        const float v = fast ? key_f32(cand_key[i]) : s[i];
        if (v > hi) {
            if (listmask) atomicOr(&listmask[(int64_t)l * mask_words + word], bitv);
            ++n_in;
            if (probe_out) { const unsigned o = atomicAdd(&sh[5], 1u); if ((int)o < probe_stride) probe_out[(int64_t)qi * probe_stride + o] = l; }
        }
        else if (v >= lo) { const unsigned b = atomicAdd(&sh[3], 1u); if (b < CS_BAND_CAP) band_id[b] = l; }
    }
    atomicAdd(&sh[2], n_in);
    __syncthreads();
    const int nb = (int)(sh[3] < (unsigned)CS_BAND_CAP ? sh[3] : (unsigned)CS_BAND_CAP);
    if (sh[3] > (unsigned)CS_BAND_CAP) {        // more lists inside the error band than the re-rank holds
        // filter form: the pass fails over to the chain with the narrow band.  There (thousands of centroids within 10^-4 of the
        // nprobe-th score: copies of one vector) the row is flagged -- the caller reports it like an overflowed candidate buffer --
        // instead of being answered from a truncated band; without a flag array (flat-IVF callers) the band is cut as before
        if (fail_out) { if (tid == 0) atomicOr(fail_out, 1u); return; }
        if (row_fail && tid == 0) row_fail[qi] = 1u;
    }
    int need = np - (int)sh[2];                  // band lists still to probe
    stamp(4);
    if (clk) dph_cs_clock[qi * 8 + 7] = (unsigned long long)nb | ((unsigned long long)n_cand << 16) | ((unsigned long long)(need > 0 ? need : 0) << 40);
    if (need <= 0 || nb == 0) return;
    // float64 dot of every band list: CS_BROWS lists per wave and trip, their 3 KiB rows in flight together (the one-product filter
    // leaves a few hundred lists in the band; one row at a time was 2 us of latency each)
    for (int b0 = wv * CS_BROWS; b0 < nb; b0 += (CS_THREADS / 64) * CS_BROWS) {
        float cv[CS_BROWS][12];
#pragma unroll
        for (int u = 0; u < CS_BROWS; ++u) {
            const int b = b0 + u < nb ? b0 + u : nb - 1;
            const float4* cp = (const float4*)(centroids + (int64_t)band_id[b] * DPH_DIM + lane * 12);
            const float4 c0 = cp[0], c1 = cp[1], c2 = cp[2];
            cv[u][0] = c0.x; cv[u][1] = c0.y; cv[u][2] = c0.z; cv[u][3] = c0.w; cv[u][4] = c1.x; cv[u][5] = c1.y; cv[u][6] = c1.z; cv[u][7] = c1.w;
            cv[u][8] = c2.x; cv[u][9] = c2.y; cv[u][10] = c2.z; cv[u][11] = c2.w;
        }
#pragma unroll
        for (int u = 0; u < CS_BROWS; ++u) {
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < 12; ++j) acc += (double)q_lds[lane * 12 + j] * (double)cv[u][j];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
            if (lane == 0 && b0 + u < nb) band_s[b0 + u] = acc;
        }
    }
    __syncthreads();
    stamp(5);
    // the `need` best of the band: bitonic sort of (score desc, list id asc) in LDS -- 55 barrier steps for a band of 535 .. 1024.
    // (Counting, for every list, the lists ahead of it was 535 x 535 float64 compares per row: 23-40 us.)
    int pow2 = 1;
    while (pow2 < nb) pow2 <<= 1;                    // <= CS_BAND_CAP
    for (int i = nb + tid; i < pow2; i += CS_THREADS) { band_s[i] = -__builtin_huge_val(); band_id[i] = 0x7FFFFFFF; }
    __syncthreads();
    for (int size = 2; size <= pow2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < pow2 / 2; i += CS_THREADS) {
                const int lo_ = 2 * i - (i & (stride - 1)), hi_ = lo_ + stride;
                const bool up = (lo_ & size) == 0;
                const double sa = band_s[lo_], sb = band_s[hi_];
                const int ia = band_id[lo_], ib = band_id[hi_];
                const bool a_first = (sa > sb) | ((sa == sb) & (ia < ib));
                if (a_first != up) { band_s[lo_] = sb; band_s[hi_] = sa; band_id[lo_] = ib; band_id[hi_] = ia; }
            }
            __syncthreads();
        }
    const int take = need < nb ? need : nb;
    for (int b = tid; b < take; b += CS_THREADS) {
        const int id = band_id[b];
        if (listmask) atomicOr(&listmask[(int64_t)id * mask_words + word], bitv);
        if (probe_out) { const unsigned o = atomicAdd(&sh[5], 1u); if ((int)o < probe_stride) probe_out[(int64_t)qi * probe_stride + o] = id; }
    }
    if (dph_cs_clock_on) { __syncthreads(); stamp(6); }
}

__global__ __launch_bounds__(256) void dph_tilemask_kernel(const int32_t* __restrict__ tile_list, int64_t n_tiles,
                                                           const uint4* __restrict__ listmask, uint4* __restrict__ tilemask,
                                                           const int* __restrict__ gate, int gate_base) {
    if (dph_gated_rows(gate, gate_base, 1) <= 0) return;          // gated retry pass with nothing to do
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < n_tiles) {
        const int64_t l = tile_list[t];
        tilemask[2 * t] = listmask[2 * l];
        tilemask[2 * t + 1] = listmask[2 * l + 1];
    }
}

#define CS_LDS ((size_t)2 * CS_CAND * 4)        // dynamic LDS of the select kernel (static + dynamic exceed 64 KiB)

static void cs_select_allow_lds(int dev) { DPH_ALLOW_LDS(dph_coarse_select_kernel, CS_LDS, dev); }

// the parts of the scratch (dph_internal.h): all of a part or nothing; a failed hipMalloc is not the caller's error
static bool ensure_chain(dph_coarse_scratch::chain_part& c) {
    if (c.est) return true;                         // (allocated last)
    const size_t rows = DPH_PASS_MAX;
    const bool ok = c.cand.alloc(rows * CS_CAND) == hipSuccess && c.cand_cnt.alloc(rows) == hipSuccess && c.est.alloc(rows) == hipSuccess;
    if (!ok) { c = dph_coarse_scratch::chain_part{}; (void)hipGetLastError(); }
    return ok;
}
static bool ensure_filter(dph_coarse_scratch::filter_part& f) {
    if (f.qfrag) return true;                       // (allocated last)
    const size_t rows = DPH_PASS_MAX;
    // (wave statistics for 256 CUs; the fragments of a whole pass: the teams form)
    const bool ok = f.sample.alloc(rows * CF_SAMPLE) == hipSuccess && f.cand.alloc(rows * CS_CAND) == hipSuccess && f.cnt.alloc(1) == hipSuccess &&
                    f.pairs.alloc((size_t)DPH_POOL_CHUNKS * DPH_CHUNK_PAIRS) == hipSuccess && f.chunk_fill.alloc(DPH_POOL_CHUNKS) == hipSuccess &&
                    f.wave_counts.alloc(256 * 4 * 2) == hipSuccess && f.counters.alloc(64) == hipSuccess &&
                    f.qfrag.alloc((size_t)(DPH_PASS_MAX / DPH_QROWS) * 4 * 2 * DPH_QGROUP_FRAG_BYTES / sizeof(uint4)) == hipSuccess;
    if (!ok) { f = dph_coarse_scratch::filter_part{}; (void)hipGetLastError(); }
    return ok;
}

// the chain: score GEMM (f32, or bf16x3 from CG_BF16X3_MIN lists on), probe selection, tile masks
void dph_launch_coarse(const dph_coarse_args& a, dph_coarse_scratch& s, hipStream_t st) {
    if (a.clear_mask && a.listmask) (void)hipMemsetAsync(a.listmask, 0, (size_t)a.nlist * a.mask_words * 4, st);
    const int dev = dph_current_device();
    const bool bf16x3 = a.nlist >= CG_BF16X3_MIN;
    const dim3 gg((a.nlist + CG_LISTS - 1) / CG_LISTS, (a.n_q + CG_QROWS - 1) / CG_QROWS);
    if (bf16x3 && a.c_pk && a.x_pk) {
        const size_t lds3 = (size_t)4 * CG_LISTS * CG3P_LD * 2;
        DPH_ALLOW_LDS(dph_coarse_gemm_bf16x3_pipe_kernel, lds3, dev);
        hipLaunchKernelGGL(dph_coarse_gemm_bf16x3_pipe_kernel, gg, dim3(256), lds3, st, a.q0, a.n_q, a.gate, a.gate_base, a.nlist, a.scores, a.c_pk, a.x_pk);
    }
    else if (bf16x3)
        hipLaunchKernelGGL(dph_coarse_gemm_bf16x3_kernel, gg, dim3(256), 0, st, a.x, a.q0, a.n_q, a.gate, a.gate_base, a.centroids, a.nlist, a.scores);
    else
        hipLaunchKernelGGL(dph_coarse_gemm_kernel, gg, dim3(256), 0, st, a.x, a.q0, a.n_q, a.gate, a.gate_base, a.centroids, a.nlist, a.scores);
    // long score rows: candidates collected by several workgroups per row first; without the scratch they take the full three-pass selection
    uint2* cand = nullptr; unsigned* cand_cnt = nullptr; unsigned* est = nullptr;
    if (a.nlist >= CS_FAST_MIN && a.n_q <= DPH_PASS_MAX && ensure_chain(s.chain)) {
        cand = s.chain.cand; cand_cnt = s.chain.cand_cnt; est = s.chain.est;
        (void)hipMemsetAsync(cand_cnt, 0, (size_t)a.n_q * 4, st);
        int slices = 2048 / (a.n_q > 0 ? a.n_q : 1);
        slices = slices < 1 ? 1 : (slices > 16 ? 16 : slices);
        hipLaunchKernelGGL(dph_coarse_estimate_kernel, dim3(a.n_q), dim3(CS_THREADS), 0, st, a.scores, a.n_q, a.gate, a.gate_base, a.nlist, a.nprobe, est);
        hipLaunchKernelGGL(dph_coarse_collect_kernel, dim3(a.n_q, slices), dim3(CS_THREADS), 0, st, a.scores, a.n_q, a.gate, a.gate_base, a.nlist,
                           cand, cand_cnt, est);
    }
    cs_select_allow_lds(dev);
    hipLaunchKernelGGL(dph_coarse_select_kernel, dim3(a.n_q), dim3(CS_THREADS), CS_LDS, st, a.x, a.q0, a.n_q, a.gate, a.gate_base, a.centroids,
                       a.scores, a.nlist, a.nprobe, a.cnorm_max, a.listmask, a.mask_words, a.probe_out, a.probe_stride,
                       1.5 * (bf16x3 ? CG_BF16X3_ERR : CG_F32_ERR), cand, cand_cnt, est, (unsigned*)nullptr, a.row_fail);
    if (a.tilemask && a.mask_words == 8)
        hipLaunchKernelGGL(dph_tilemask_kernel, dim3((unsigned)((a.n_tiles + 255) / 256)), dim3(256), 0, st, a.tile_list, a.n_tiles,
                           (const uint4*)a.listmask, (uint4*)a.tilemask, a.gate, a.gate_base);
}

// The filter in front of the chain for long quantizers (comment above dph_coarse_sample_gemm_kernel).  a.x: the (rotated) query rows of
// the pass [n_q][768] fp32, x_hi their bf16 image, c_hi / c_pieces the centroids' (chunk-major for the sample GEMM, piece-major for the
// scan), x_pk / c_pk the packed hi|lo images the fail-over chain multiplies.
void dph_launch_coarse_filter(const dph_coarse_filter_args& a, dph_coarse_scratch& s, hipStream_t st) {
    dph_coarse_args chain = a;                      // what the bf16x3 chain serves: the pass as it stands, or its fail-over
    const int n_q = a.n_q, nlist = a.nlist;
    if (!a.c_pieces || !ensure_filter(s.filter) || n_q > DPH_PASS_MAX) {      // no image or no scratch: the bf16x3 chain alone
        dph_launch_coarse(chain, s, st);
        return;
    }
    const dph_coarse_scratch::filter_part& f = s.filter;
    dph_coarse_counters* const cnt = f.cnt;
    unsigned* const cand_cnt = cnt->cand_cnt;       // (addresses of device memory: nothing is read here)
    unsigned* const est = cnt->est;
    unsigned* const pool_count = &cnt->pool_count;
    unsigned* const fail = &cnt->fail;
    const int m = nlist < CF_SAMPLE ? nlist : CF_SAMPLE;
    const int stride = nlist / m;
    if (a.listmask) (void)hipMemsetAsync(a.listmask, 0, (size_t)nlist * a.mask_words * 4, st);       // (NULL: the caller walks probe_out only)
    (void)hipMemsetAsync(cnt, 0, sizeof *cnt, st);
    const int dev = dph_current_device();
    const int cus = dph_scan_grid(dev);             // (at most 256: what the wave statistics hold)
    const size_t lds128 = (size_t)2 * CG_LISTS * (CF_K + 8) * 2;
    DPH_ALLOW_LDS(dph_coarse_sample_gemm_kernel, lds128, dev);
    cs_select_allow_lds(dev);
    const int qt = (n_q + CG_QROWS - 1) / CG_QROWS;
    const int np = a.nprobe < nlist ? a.nprobe : nlist;
    // enough candidates for the nprobe lists, the error band below them and the sampling noise; never more than the lists there are
    int target = 4 * np + 64;
    if (target > nlist) target = nlist;
    const int tiles_s = (m + CG_LISTS - 1) / CG_LISTS, tiles_f = (nlist + CG_LISTS - 1) / CG_LISTS;
    // persistent: two workgroups per CU share the list tiles (fewer when the pass has several query tiles: grid.y)
    const int wg = std::max(1, 2 * cus / qt);
    hipLaunchKernelGGL(dph_coarse_sample_gemm_kernel, dim3(std::min(tiles_s, wg), qt), dim3(256), lds128, st, n_q, m, stride, (int64_t)tiles_f, a.c_hi, a.x_hi,
                       f.sample.p);
    hipLaunchKernelGGL(dph_coarse_estimate_sample_kernel, dim3(n_q), dim3(CS_THREADS), 0, st, f.sample.p, n_q, m, stride, target, est);
    auto profiled = [&](auto launch) { if (a.prof) a.prof->bracket(a.prof_list, st, launch); else launch(); };
    // 128 query rows per read of the centroid image (one group of 32 per scan wave); a pass of more rows reads it once per 128.
    // More than 128 rows: ONE launch of teams (dph_scan.hip MODE 4) -- the groups of 128 rows share every tile through the XCDs' L2
    // instead of each reading the image from HBM.  Groups rounded up to a power of two that divides the 32 workgroups of an XCD.
    int n_groups = 1;
    while (n_groups * (int)DPH_QROWS < n_q) n_groups *= 2;
    const bool teams = a.teams != 0 && n_groups >= 2 && n_groups <= 8 && cus % (8 * n_groups) == 0;
    if (teams) {
        hipLaunchKernelGGL(dph_cf_qfrag_kernel, dim3((n_groups * 4 * 2 * 24 * 64 + 255) / 256), dim3(256), 0, st, a.x_hi, n_q, f.qfrag.p, n_groups);
        profiled([&] { dph_launch_coarse_scan_teams(a.c_pieces, nlist, f.qfrag, n_q, n_groups, est, f.pairs, f.chunk_fill, f.wave_counts, f.counters, cus, st); });
        hipLaunchKernelGGL(dph_coarse_bucket_chunks_kernel, dim3(64), dim3(CB_THREADS), 0, st, (const uint2*)f.pairs, (const unsigned*)f.chunk_fill, (const int*)f.counters,
                           n_q, 0u, f.cand.p, cand_cnt, (int)CS_CAND, pool_count, fail);
    }
    for (int q0 = 0; !teams && q0 < n_q; q0 += DPH_QROWS) {
        const int nq = std::min(n_q - q0, (int)DPH_QROWS);
        hipLaunchKernelGGL(dph_cf_qfrag_kernel, dim3((4 * 2 * 24 * 64 + 255) / 256), dim3(256), 0, st, a.x_hi + (int64_t)q0 * DPH_DIM, nq, f.qfrag.p);
        profiled([&] { dph_launch_coarse_scan(a.c_pieces, nlist, f.qfrag, nq, est + q0, f.pairs, f.chunk_fill, f.wave_counts, f.counters, cus, st); });
        hipLaunchKernelGGL(dph_coarse_bucket_chunks_kernel, dim3(64), dim3(CB_THREADS), 0, st, (const uint2*)f.pairs, (const unsigned*)f.chunk_fill, (const int*)f.counters,
                           n_q, (unsigned)q0, f.cand.p, cand_cnt, (int)CS_CAND, pool_count, fail);
    }
    hipLaunchKernelGGL(dph_coarse_select_kernel, dim3(n_q), dim3(CS_THREADS), CS_LDS, st, a.x, 0, n_q, (const int*)nullptr, 0, a.centroids,
                       (const float*)nullptr, nlist, a.nprobe, a.cnorm_max, a.listmask, a.mask_words, a.probe_out, a.probe_stride, 1.02 * CF_HI_ERR,
                       (const uint2*)f.cand, (const unsigned*)cand_cnt, (const unsigned*)est, fail, (unsigned*)nullptr, a.cnorm, a.cnorm_cap);
    hipLaunchKernelGGL(dph_coarse_gate_kernel, dim3(1), dim3(64), 0, st, fail, n_q, &cnt->gate);
    // fail-over: the whole pass again through the bf16x3 chain, gated on the device (empty launches when nothing failed); it ORs into
    // the masks the filter form has set (a row that succeeded marks the same lists again) and rewrites the probe lists it covers
    chain.gate = &cnt->gate;
    chain.clear_mask = false;
    dph_launch_coarse(chain, s, st);
}

// what the filter form did in the last pass over this scratch: out[0] = 1 when the pass failed over to the bf16x3 chain, out[1] = pairs
// its scan put into the pair pool (synchronises the device)
int dph_coarse_filter_debug(const dph_coarse_scratch& s, unsigned out[2]) {
    const dph_coarse_counters* const cnt = s.filter.cnt;
    if (!cnt) { out[0] = out[1] = 0xFFFFFFFFu; return 0; }
    return hipMemcpy(&out[0], &cnt->fail, 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(&out[1], &cnt->pool_count, 4, hipMemcpyDeviceToHost) != hipSuccess;
}

// ---- work queue of the unit scan (dph_internal.h: DPH_PASS_MAX).  One wave per inverted list: the probing query rows
// of the list (set bits of its DPH_UNIT_WORDS mask words, ascending) are dealt into chunks of 128 slots; every chunk
// gets a slot table, its gathered high-digit fragments (written by the kernel below) and one unit record per segment
// of DPH_UNIT_TILES tiles.  Chunks and units are numbered in list order (dph_units_offsets_kernel: an exclusive scan
// over the lists), i.e. in address order: consecutive pops of the scan's work queue stream neighbouring segments.
#define UO_THREADS 1024
__global__ __launch_bounds__(UO_THREADS) void dph_units_offsets_kernel(const unsigned* __restrict__ listmask, int nlist,
                                                                      const int* __restrict__ list_tile0,
                                                                      int2* __restrict__ offsets, int* __restrict__ counts) {
    __shared__ int2 wsum[UO_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int per = (nlist + UO_THREADS - 1) / UO_THREADS;
    const int l0 = tid * per, l1 = min(nlist, l0 + per);
    int2 mine = make_int2(0, 0);                      // chunks, units of this thread's lists
    for (int l = l0; l < l1; ++l) {
        const uint4* m = (const uint4*)(listmask + (int64_t)l * DPH_UNIT_WORDS);
        int cnt = 0;
#pragma unroll
        for (int i = 0; i < DPH_UNIT_WORDS / 4; ++i) {
            const uint4 v = m[i];
            cnt += __builtin_popcount(v.x) + __builtin_popcount(v.y) + __builtin_popcount(v.z) + __builtin_popcount(v.w);
        }
        const int ntiles = list_tile0[l + 1] - list_tile0[l];
        const int chunks = (cnt > 0 && ntiles > 0) ? (cnt + DPH_UNIT_SLOTS - 1) / DPH_UNIT_SLOTS : 0;
        mine.x += chunks;
        mine.y += chunks * ((ntiles + DPH_UNIT_TILES - 1) / DPH_UNIT_TILES);
    }
    int2 incl = mine;                                 // inclusive scan over the workgroup
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int vx = __shfl_up(incl.x, o), vy = __shfl_up(incl.y, o);
        if (lane >= o) { incl.x += vx; incl.y += vy; }
    }
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    int2 base = make_int2(0, 0);
    for (int w = 0; w < wv; ++w) { base.x += wsum[w].x; base.y += wsum[w].y; }
    int2 run = make_int2(base.x + incl.x - mine.x, base.y + incl.y - mine.y);       // exclusive prefix of this thread
    for (int l = l0; l < l1; ++l) {
        // (recomputed: cheaper than keeping `per` values in registers)
        const uint4* m = (const uint4*)(listmask + (int64_t)l * DPH_UNIT_WORDS);
        int cnt = 0;
#pragma unroll
        for (int i = 0; i < DPH_UNIT_WORDS / 4; ++i) {
            const uint4 v = m[i];
            cnt += __builtin_popcount(v.x) + __builtin_popcount(v.y) + __builtin_popcount(v.z) + __builtin_popcount(v.w);
        }
        const int ntiles = list_tile0[l + 1] - list_tile0[l];
        const int chunks = (cnt > 0 && ntiles > 0) ? (cnt + DPH_UNIT_SLOTS - 1) / DPH_UNIT_SLOTS : 0;
        offsets[l] = run;
        run.x += chunks;
        run.y += chunks * ((ntiles + DPH_UNIT_TILES - 1) / DPH_UNIT_TILES);
    }
    if (tid == UO_THREADS - 1) { counts[0] = run.x; counts[1] = run.y; }
}

__global__ __launch_bounds__(256) void dph_units_build_kernel(const unsigned* __restrict__ listmask, int nlist,
                                                              const int* __restrict__ list_tile0, int chunk_cap, int unit_cap,
                                                              const int2* __restrict__ offsets, int* __restrict__ counts,
                                                              int* __restrict__ slot_q, int4* __restrict__ unit_recs,
                                                              int4* __restrict__ list_recs, int spread) {
    const int l = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (l >= nlist) return;
    const unsigned w = lane < DPH_UNIT_WORDS ? listmask[(int64_t)l * DPH_UNIT_WORDS + lane] : 0u;
    const int pc = __builtin_popcount(w);
    int incl = pc;                                   // inclusive prefix sum over the lanes
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(incl, o); if (lane >= o) incl += v; }
    const int cnt = __shfl(incl, 63);
    const int t0 = list_tile0[l], ntiles = list_tile0[l + 1] - t0;
    if (cnt == 0 || ntiles <= 0) return;
    const int chunks = (cnt + DPH_UNIT_SLOTS - 1) / DPH_UNIT_SLOTS;
    const int segs = (ntiles + DPH_UNIT_TILES - 1) / DPH_UNIT_TILES;
    const int c0 = offsets[l].x, u0 = offsets[l].y;
    if (c0 + chunks > chunk_cap || u0 + chunks * segs > unit_cap) { if (lane == 0) atomicOr(&counts[2], 1); return; }   // cannot happen: caps are worst case
    // slot tables: the i-th probing row (ascending) goes to chunk i / 128
    int i = incl - pc;
    unsigned bits = w;
    while (bits) {
        const int j = __builtin_ctz(bits);
        bits &= bits - 1u;
        // dealt over the four column groups (= scan waves) first, so that a half-empty chunk still loads all four waves
        // with pairs: their pair regions fill evenly and so do the refine workgroups behind them
        const int within = i % DPH_UNIT_SLOTS;
        const int col = spread ? (within & 3) * DPH_QGROUP + (within >> 2) : within;
        slot_q[(int64_t)c0 * DPH_UNIT_SLOTS + (i - within) + col] = 32 * lane + j;
        ++i;
    }
    for (int e = cnt + lane; e < chunks * DPH_UNIT_SLOTS; e += 64) {
        const int within = e % DPH_UNIT_SLOTS;
        const int col = spread ? (within & 3) * DPH_QGROUP + (within >> 2) : within;
        slot_q[(int64_t)c0 * DPH_UNIT_SLOTS + (e - within) + col] = -1;
    }
    for (int c = lane; c < chunks; c += 64) list_recs[c0 + c] = make_int4(t0, t0, t0 + ntiles, c0 + c);
    for (int e = lane; e < chunks * segs; e += 64) {
        const int c = e / segs, sg = e % segs;
        const int first = t0 + sg * DPH_UNIT_TILES;
        const int end = min(t0 + ntiles, first + DPH_UNIT_TILES);
        unit_recs[u0 + e] = make_int4(t0, first, end, c0 + c);
    }
}

// fragment image of chunk c, group g (dph_quantize_kernel's order: [kstep][lane][16 B], lane = 32*half + column):
// the 16 bytes of lane (half, column) at k-step ks are bytes 32 ks + 16 half .. + 15 of the column's query row
__global__ __launch_bounds__(256) void dph_units_gather_kernel(const int* __restrict__ counts, const int* __restrict__ slot_q,
                                                               const int8_t* __restrict__ q1, int q0,
                                                               int8_t* __restrict__ frags, bool x16) {
    const int c = blockIdx.x, g = blockIdx.y;
    if (c >= counts[0]) return;
    const int lane = threadIdx.x & 63, kq = threadIdx.x >> 6;
    uint4* out = (uint4*)(frags + ((int64_t)c * 4 + g) * DPH_QGROUP_FRAG_BYTES);
    if (x16) {
        // the 16 x 16 x 64 order (dph_internal.h): entry 2 s + h, lane = 16 (k-chunk) + column of the query half h
#pragma unroll
        for (int i = 0; i < DPH_KSTEPS / 4; ++i) {
            const int e = kq + 4 * i, s_ = e >> 1, hq = e & 1;
            const int qrow = slot_q[(int64_t)c * DPH_UNIT_SLOTS + g * DPH_QGROUP + 16 * hq + (lane & 15)];
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (qrow >= 0) v = *(const uint4*)(q1 + (int64_t)(q0 + qrow) * DPH_DIM + 64 * s_ + 16 * (lane >> 4));
            out[e * 64 + lane] = v;
        }
        return;
    }
    const int qrow = slot_q[(int64_t)c * DPH_UNIT_SLOTS + g * DPH_QGROUP + (lane & 31)];
    const int8_t* src = q1 + (int64_t)(q0 + (qrow < 0 ? 0 : qrow)) * DPH_DIM + 16 * (lane >> 5);
#pragma unroll
    for (int i = 0; i < DPH_KSTEPS / 4; ++i) {
        const int ks = kq + 4 * i;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (qrow >= 0) v = *(const uint4*)(src + 32 * ks);
        out[ks * 64 + lane] = v;
    }
}

void dph_launch_units_build(const dph_ivf_pass& ivf, const dph_unit_queue& uq, int nlist, const int* list_tile0, const int8_t* q1, int q0,
                            int spread, bool x16, hipStream_t st) {
    int* const counts = &ivf.unit_cnt.p->chunks;          // the kernels' view: [0] chunks, [1] units, [2] error (dph_unit_counters)
    (void)hipMemsetAsync(ivf.unit_cnt.p, 0, sizeof(dph_unit_counters), st);
    hipLaunchKernelGGL(dph_units_offsets_kernel, dim3(1), dim3(UO_THREADS), 0, st, ivf.listmask_u.p, nlist, list_tile0, ivf.unit_offsets.p,
                       counts);
    hipLaunchKernelGGL(dph_units_build_kernel, dim3((nlist + 3) / 4), dim3(256), 0, st, ivf.listmask_u.p, nlist, list_tile0, uq.chunk_cap,
                       uq.unit_cap, ivf.unit_offsets.p, counts, uq.slot_q.p, uq.unit_recs.p, uq.unit_list_recs.p, spread);
    hipLaunchKernelGGL(dph_units_gather_kernel, dim3(uq.chunk_cap, 4), dim3(256), 0, st, counts, uq.slot_q.p, q1, q0, uq.unit_frags.p, x16);
}

// ---- list assignment of database rows for the list builder (replaces the add-to-index step of
// build_phrase_index.py:145-153 for the exact in-list variant): best[r] = arg-max_l <x_r, c_l> (+ an optional per-list
// bias: -||c||^2/2 turns it into the L2 assignment of a k-means step), ties to the lowest list id, plus the gap to the
// runner-up so the caller can re-check near-ties in float64.  FUSED: a workgroup owns 128 rows and walks all list tiles,
// keeping the running best two scores per row in registers -- the [n, nlist] score matrix (2.8 TB for 170 M rows x 4096
// lists) is never written.  Same MFMA tile as dph_coarse_gemm_kernel (v_mfma_f32_32x32x2_f32: exact fp32 products), the
// centroids are the streamed operand (L2-resident: 12.6 MB at 4096 lists).  ROWS_INT8: the rows are int8 rows of the
// resident shard, de-quantised through the shard's LUT while they are staged (the reference's fp32 values exactly).
template <bool ROWS_INT8>
__global__ __launch_bounds__(256) void dph_assign_fused_kernel(const void* __restrict__ rows, int64_t n,
                                                               const float* __restrict__ lut,
                                                               const float* __restrict__ centroids, int nlist,
                                                               const float* __restrict__ bias, int32_t* __restrict__ best,
                                                               float* __restrict__ gap) {
    __shared__ float a_lds[CG_LISTS * CG_LD];
    __shared__ float b_lds[CG_QROWS * CG_LD];
    __shared__ float red_s1[4][CG_QROWS], red_s2[4][CG_QROWS];
    __shared__ int red_i1[4][CG_QROWS];
    const int64_t r0 = (int64_t)blockIdx.x * CG_QROWS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float b1[4], b2[4];
    int i1[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { b1[j] = -3.4e38f; b2[j] = -3.4e38f; i1[j] = 0x7fffffff; }
    for (int l0 = 0; l0 < nlist; l0 += CG_LISTS) {
        v16f acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
        for (int k0 = 0; k0 < DPH_DIM; k0 += CG_KCHUNK) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = (tid >> 3) + 32 * i, c4 = (tid & 7) * 4;
                const int l = l0 + row;
                const int64_t q = r0 + row;
                const float4 av = l < nlist ? *(const float4*)(centroids + (int64_t)l * DPH_DIM + k0 + c4) : make_float4(0.f, 0.f, 0.f, 0.f);
                float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
                if (q < n) {
                    if constexpr (ROWS_INT8) {
                        const unsigned w = *(const unsigned*)((const int8_t*)rows + q * DPH_DIM + k0 + c4);
                        bv = make_float4(lut[(int)(int8_t)(w) + 128], lut[(int)(int8_t)(w >> 8) + 128],
                                         lut[(int)(int8_t)(w >> 16) + 128], lut[(int)(int8_t)(w >> 24) + 128]);
                    } else {
                        bv = *(const float4*)((const float*)rows + q * DPH_DIM + k0 + c4);
                    }
                }
                float* ap = a_lds + row * CG_LD + c4;
                float* bp = b_lds + row * CG_LD + c4;
                ap[0] = av.x; ap[1] = av.y; ap[2] = av.z; ap[3] = av.w;
                bp[0] = bv.x; bp[1] = bv.y; bp[2] = bv.z; bp[3] = bv.w;
            }
            __syncthreads();
            const float* ap = a_lds + (wave * 32 + (lane & 31)) * CG_LD + (lane >> 5);
            const float* bp = b_lds + (lane & 31) * CG_LD + (lane >> 5);
#pragma unroll
            for (int kk = 0; kk < CG_KCHUNK; kk += 2) {
                const float a = ap[kk];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bp[j * 32 * CG_LD + kk], acc[j], 0, 0, 0);
            }
            __syncthreads();
        }
        // C[i = (r&3) + 8*(r>>2) + 4*(lane>>5)][j = lane&31]: i = list inside the wave's 32 (ascending in r), j = row
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int l = l0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (l < nlist) {
                    const float v = acc[j][r] + (bias ? bias[l] : 0.f);
                    if (v > b1[j] || (v == b1[j] && l < i1[j])) { b2[j] = b1[j]; b1[j] = v; i1[j] = l; }
                    else if (v > b2[j]) b2[j] = v;
                }
            }
    }
    // merge the two lane halves (same row, other lists), then the four waves through LDS
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float ob1 = __shfl_xor(b1[j], 32), ob2 = __shfl_xor(b2[j], 32);
        const int oi1 = __shfl_xor(i1[j], 32);
        if (ob1 > b1[j] || (ob1 == b1[j] && oi1 < i1[j])) { b2[j] = fmaxf(b1[j], ob2); b1[j] = ob1; i1[j] = oi1; }
        else b2[j] = fmaxf(b2[j], ob1);
        if (lane < 32) { red_s1[wave][j * 32 + lane] = b1[j]; red_s2[wave][j * 32 + lane] = b2[j]; red_i1[wave][j * 32 + lane] = i1[j]; }
    }
    __syncthreads();
    if (tid < CG_QROWS) {
        float s1 = red_s1[0][tid], s2 = red_s2[0][tid];
        int i = red_i1[0][tid];
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            const float o1 = red_s1[w][tid], o2 = red_s2[w][tid];
            const int oi = red_i1[w][tid];
            if (o1 > s1 || (o1 == s1 && oi < i)) { s2 = fmaxf(s1, o2); s1 = o1; i = oi; }
            else s2 = fmaxf(s2, o1);
        }
        const int64_t q = r0 + tid;
        if (q < n) { best[q] = i; gap[q] = s1 - s2; }
    }
}

void dph_launch_assign(const void* rows, bool rows_int8, const float* lut, int64_t n, const float* centroids, int nlist,
                       const float* bias, int32_t* best, float* gap, hipStream_t st) {
    const dim3 grid((unsigned)((n + CG_QROWS - 1) / CG_QROWS));
    if (rows_int8)
        hipLaunchKernelGGL(dph_assign_fused_kernel<true>, grid, dim3(256), 0, st, rows, n, lut, centroids, nlist, bias, best, gap);
    else
        hipLaunchKernelGGL(dph_assign_fused_kernel<false>, grid, dim3(256), 0, st, rows, n, lut, centroids, nlist, bias, best, gap);
}
