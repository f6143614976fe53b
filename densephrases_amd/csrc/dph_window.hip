// dph_window.hip -- start/end window re-scoring (replaces /root/reference/densephrases/index.py:276-370: the
// 2*B*k*L python-level faiss.reconstruct calls, the zeros[B*k, L, 768] fill, end @ R, the (q * end).sum(2)
// and the valid_phrase mask) with one gather + de-quantise + dot + mask + arg-max kernel over the resident shard.
// One wavefront per candidate; rows are read exactly once (768 B each), scores accumulate in fp64.
#include "dph_internal.h"

// The candidate of a wavefront as the row sources see it.
struct win_cand {
    int64_t id; bool in_idmap;                       // in_idmap: the id map knows the id (before the get_idxs clip)
    int w; int64_t fbase, flen; bool own_in;         // word, the document's span of the f2o CSR; own_in: the word lies inside its document
    int direction, L, lane;
    __device__ int64_t delta(int i) const { return direction == 0 ? (int64_t)i : -(int64_t)i; }     // slot i is id + delta / word + delta
};
// 12 int8 codes of a lane, as three words
struct win_codes {
    unsigned wv[3];
    __device__ void load(const int8_t* rows, int64_t row, int lane) {
        const unsigned* p = (const unsigned*)(rows + row * DPH_DIM + lane * 12);
        wv[0] = p[0]; wv[1] = p[1]; wv[2] = p[2];
    }
    __device__ int code(int j) const { return (int)(int8_t)(wv[j >> 2] >> (8 * (j & 3))); }
    __device__ void dequant(const float* lut, float v[12]) const {
#pragma unroll
        for (int j = 0; j < 12; ++j) v[j] = lut[code(j) + 128];
    }
};

// ---- the three row sources: where the vector of a window slot comes from.  stage(base slot) runs wave-uniformly before every
// 64th slot; fetch gives this lane's 12 components of slot sl (i-th neighbour), false = the zero vector, wave-uniform; owns says
// whether this shard may speak in `vecs`; fetch_vec gives the output vectors t = 0 (the candidate's own) and 1 (the arg-max slot's).

// Raw int8 rows of a flat / grouped / list-major shard: the stored row of id +- i, consecutive GLOBAL ids like the reference's
// reconstruct loop (index.py:282-300); an id this shard does not hold counts as a zero vector (:285-288).  List-major (IVF)
// shards go through inv_row.
struct FlatRows {
    static constexpr bool has_lut = true;
    const int8_t* db; int64_t n_rows; const float* lut; const int32_t* inv_row; dph_idmap idmap;
    __device__ int64_t row_of(int64_t id) const {
        const int64_t l = dph_local_of_id(idmap, id);
        const int64_t row = (l < 0) ? -1 : (inv_row ? (int64_t)inv_row[l] : l);
        return row < n_rows ? row : -1;
    }
    __device__ void stage(const win_cand&, int) {}
    __device__ bool fetch(const win_cand& c, int, int i, const float* lut_lds, float v[12]) const { return fetch_vec(c, 1, i, lut_lds, v); }
    // false for an id this shard does not hold.  Range-sharded: a candidate of another rank -- its vectors come back zero here and the
    // SUM all-reduce fills them in.  Single rank: only FAISS' -1 padding (fewer than k rows) gets here, and zero is what the reference's
    // RAM branch returns for it too: reconst_fn(-1) raises and index.py:285-288 substitutes np.zeros (the HDF5 branch, which would read
    // the row of the CLIPPED id, is not the one this path follows: DESIGN.md section 2 "reference quirks").
    __device__ bool owns(const win_cand& c) { return c.in_idmap; }
    __device__ bool fetch_vec(const win_cand& c, int, int i, const float* lut_lds, float v[12]) const {
        const int64_t row = row_of(c.id + c.delta(i));
        if (row < 0) return false;
        win_codes r;
        r.load(db, row, c.lane);
        r.dequant(lut_lds, v);
        return true;
    }
};

// RECONSTRUCTED vectors of an OPQ + IVFPQ index (index.py:276-370, PQ branch): slot vector = reconstruct(id +- i) in the rotated
// space, zero when the id is unknown (index.py:285-288); the reference un-rotates it (`end.matmul(self.R)`, :340) and takes the
// fp32 dot with the query half -- <q, v' R> = <R q, v'> = <A q, v'>, so the dot is taken with the ROTATED query half qrot = A q
// (pq_transform_kernel without the bias) in float64 and rounded once, no un-rotation of 2*B*k*L vectors.  `vecs` leaves here in
// the rotated space: pq_unrotate_kernel finishes them.
struct PqCodes {
    static constexpr bool has_lut = false;
    pq_store s;
    int64_t my_pos = -1; int my_list = 0;            // of slot (base + lane) of the staged 64
    int64_t own_pos = -1;                            // of the candidate itself (owns)
    // Where the window's codes lie: lane sl resolves slot base + sl -- the binary search of its id in the direct map (28 dependent
    // loads at 170 M codes) and of its position in the list offsets (20) -- for up to 64 slots AT ONCE; walking the slots one after
    // the other, 2 * B * k * L searches in series per wave, was 127 us per direction at B = 64, k = 10, L = 10
    // (profiles/r05_kernel_trace_pq_e2e_b64.csv)
    __device__ void stage(const win_cand& c, int base) {
        const int mine_sl = base + c.lane;
        my_pos = -1;
        my_list = 0;
        if (mine_sl < c.L) {
            const int i = c.direction == 0 ? mine_sl : (c.L - 1 - mine_sl);
            my_pos = pq_pos_of_id(s.dm_ids, s.dm_pos, s.ntotal, c.id + c.delta(i));
            if (my_pos >= 0) my_list = pq_list_of_pos(s.list_off, s.nlist, my_pos);
        }
    }
    __device__ bool components(const win_cand& c, int64_t pos, int list, float v[12]) const {
        if (pos < 0) return false;
#pragma unroll
        for (int j = 0; j < 12; ++j) v[j] = pq_component(s, pos, list, c.lane * 12 + j);
        return true;
    }
    __device__ bool fetch(const win_cand& c, int sl, int, const float*, float v[12]) const {
        const int64_t pos = __shfl(my_pos, sl & 63);
        const int list = __shfl(my_list, sl & 63);
        return components(c, pos, list, v);
    }
    // The shard holds a candidate when its DIRECT MAP does (what dph_reconstruct answers), whatever the id map says: ids of a PQ
    // shard without id groups are sparse or offset (n_ids = ntotal, id_base = 0), and dph_local_of_id knows none of them.
    __device__ bool owns(const win_cand& c) { own_pos = pq_pos_of_id(s.dm_ids, s.dm_pos, s.ntotal, c.id); return own_pos >= 0; }
    __device__ bool fetch_vec(const win_cand& c, int t, int i, const float*, float v[12]) const {
        const int64_t pos = t == 0 ? own_pos : pq_pos_of_id(s.dm_ids, s.dm_pos, s.ntotal, c.id + c.delta(i));
        return components(c, pos, pos >= 0 ? pq_list_of_pos(s.list_off, s.nlist, pos) : 0, v);
    }
};

// The dump's RAW int8 rows of whole documents next to a PQ index (index.py:246-273, the HDF5 branch; dph_index_attach_doc_rows):
// what the reference reads when meta_compressed.pkl is absent.  A slot's row is addressed by (document of the candidate,
// word +- i), row = f2o_off[doc slot] + word in the doc-row store, and a word outside [0, len) of the document is a zero vector
// (:265, :270 clip the range, :333-336 / :358-361 fill the rest of the np.zeros window); a candidate outside its document has no
// window at all.  No direct-map search per slot: the only one left is the candidate's own, for `vecs`.  The dot is
// <A q, dequant(row)> like PqCodes', with lut[n + 128] = fp32(n / scale + offset) rounded ONCE from float64 (int8_to_float,
// :158-162, on an int8 array gives float64; the assignment into the fp32 window rounds it).  vecs [c,0,:] is the candidate's own
// row as RAW int8 values (:383, :388 take groups_*[...] before any dequant), [c,1,:] the de-quantised arg-max row;
// pq_unrotate_kernel multiplies them by R once / twice.
struct DocRows {
    static constexpr bool has_lut = true;
    const int8_t* rows; int64_t n_doc_rows; const float* lut; pq_store s;
    __device__ void stage(const win_cand&, int) {}
    __device__ bool load(const win_cand& c, int i, win_codes& r) const {
        const int64_t ww = (int64_t)c.w + c.delta(i), row = c.fbase + ww;
        if (!c.own_in || ww < 0 || ww >= c.flen || row >= n_doc_rows) return false;
        r.load(rows, row, c.lane);
        return true;
    }
    __device__ bool fetch(const win_cand& c, int, int i, const float* lut_lds, float v[12]) const { return fetch_vec(c, 1, i, lut_lds, v); }
    // a candidate the DIRECT MAP does not hold (another rank's, FAISS' -1 padding) gives zero vectors: see PqCodes
    __device__ bool owns(const win_cand& c) { return pq_pos_of_id(s.dm_ids, s.dm_pos, s.ntotal, c.id) >= 0; }
    __device__ bool fetch_vec(const win_cand& c, int t, int i, const float* lut_lds, float v[12]) const {
        win_codes r;
        if (!load(c, i, r)) return false;
        if (t == 0) {
#pragma unroll
            for (int j = 0; j < 12; ++j) v[j] = (float)r.code(j);
        } else {
            r.dequant(lut_lds, v);
        }
        return true;
    }
};

template <class Source>
__global__ __launch_bounds__(256) void window_kernel(dph_window_args a, Source src) {
    const int tid = threadIdx.x, lane = tid & 63;
    const float* lut_lds = nullptr;
    if constexpr (Source::has_lut) {
        __shared__ float lut_sh[256];
        lut_sh[tid] = src.lut[tid];
        __syncthreads();
        lut_lds = lut_sh;
    }
    const int64_t c = (int64_t)blockIdx.x * 4 + (tid >> 6);
    if (c >= a.n_cand) return;

    win_cand cd;
    cd.id = a.ids[c]; cd.direction = a.direction; cd.L = a.L; cd.lane = lane;
    // (doc, word) of the candidate when the caller did not pass them: idx2id is indexed by local id (= stored row on
    // flat and grouped shards); ids outside the shard are clipped like get_idxs (index.py:128-133)
    int64_t lc = dph_local_of_id(a.idmap, cd.id);
    cd.in_idmap = lc >= 0;
    if (lc < 0) {
        const int64_t first_id = a.idmap.n_groups ? a.idmap.id_offsets[0] : a.idmap.id_base;
        lc = cd.id < first_id ? 0 : a.idmap.n_ids - 1;
        if (lc < 0) lc = 0;
    }
    const int d = a.doc_in ? a.doc_in[c] : a.row2doc[lc];
    const int w = cd.w = a.word_in ? a.word_in[c] : a.row2word[lc];

    // document -> f2o CSR slot (binary search over the sorted doc ids)
    int64_t lo = 0, hi = a.n_docs;
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (a.doc_ids[mid] < d) lo = mid + 1; else hi = mid; }
    const bool have_doc = d >= 0 && lo < a.n_docs && a.doc_ids[lo] == d;
    const int64_t fbase = cd.fbase = have_doc ? a.f2o_off[lo] : 0;
    const int64_t flen = cd.flen = have_doc ? a.f2o_off[lo + 1] - fbase : 0;
    cd.own_in = have_doc && w >= 0 && w < flen;

    float q[12];
    const float* qp = a.qhalf + (c / a.k) * DPH_DIM + lane * 12;
#pragma unroll
    for (int j = 0; j < 12; ++j) q[j] = qp[j];

    double best_s = 0.0;
    int best_slot = -1, best_word = -1;
    const float f0 = a.first[c];
    for (int sl = 0; sl < a.L; ++sl) {
        if ((sl & 63) == 0) src.stage(cd, sl);
        const int i = a.direction == 0 ? sl : (a.L - 1 - sl);
        const int64_t ww = (int64_t)w + cd.delta(i);
        bool valid = cd.own_in && ww >= 0 && ww < flen;                                // index.py:305-321
        if (valid) {
            const int64_t gap = a.direction == 0 ? (int64_t)a.f2o[fbase + ww] - (int64_t)a.f2o[fbase + w]
                                                 : (int64_t)a.f2o[fbase + w] - (int64_t)a.f2o[fbase + ww];
            valid = gap >= 0 && gap <= a.L;
        }
        double dot = 0.0;
        float v[12];
        if (src.fetch(cd, sl, i, lut_lds, v)) {       // wave-uniform: the shuffles sit under it
#pragma unroll
            for (int j = 0; j < 12; ++j) dot += (double)q[j] * (double)v[j];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) dot += __shfl_xor(dot, o);
        }
        // fp32 + fp32 in fp32, then the float64 mask: np.expand_dims(start_scores, 1) + new_end_scores + end_mask (:343 / :368)
        const double sc = (double)(f0 + (float)dot) + (valid ? 0.0 : -1e9);
        if (best_slot < 0 || sc > best_s) { best_s = sc; best_slot = sl; best_word = valid ? (int)ww : -1; }
    }
    if (lane == 0) {
        a.pred_word[c] = best_word;
        a.best[c] = best_s;
        a.argslot[c] = best_slot;
    }
    if (a.vecs) {
        // [c,0,:] the candidate's own vector, [c,1,:] the arg-max slot's (index.py:345,370,381-389)
        const int iv[2] = {0, a.direction == 0 ? best_slot : (a.L - 1 - best_slot)};
        // A candidate this shard does not hold contributes ZERO vectors, also for a window slot that happens to lie in this shard's
        // range (the first rows of the next rank's range): the ranks' vectors are SUMMED (index.py _window_vectors), exactly one
        // rank -- the candidate's own -- may speak
        const bool mine = src.owns(cd);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            float* o = a.vecs + (c * 2 + t) * DPH_DIM + lane * 12;
            float v[12];
            const bool have = mine && src.fetch_vec(cd, t, iv[t], lut_lds, v);
#pragma unroll
            for (int j = 0; j < 12; ++j) o[j] = have ? v[j] : 0.f;
        }
    }
}

void dph_launch_window(const dph_window_args& a, const pq_store* pq, const int8_t* rows, int64_t n_rows, const float* lut,
                       const int32_t* inv_row, hipStream_t st) {
    if (a.n_cand <= 0) return;
    const dim3 grid((unsigned)((a.n_cand + 3) / 4)), block(256);
    if (!pq) hipLaunchKernelGGL(window_kernel<FlatRows>, grid, block, 0, st, a, FlatRows{rows, n_rows, lut, inv_row, a.idmap});
    else if (!rows) hipLaunchKernelGGL(window_kernel<PqCodes>, grid, block, 0, st, a, PqCodes{*pq});
    else hipLaunchKernelGGL(window_kernel<DocRows>, grid, block, 0, st, a, DocRows{rows, n_rows, lut, *pq});
}

// ------------------------------------------------------------------------------------------ encoder.py scoring
// The start/end-vector scoring of /root/reference/densephrases/encoder.py:
//   train_query (:383-386)  start_logits = query_start.matmul(start_vecs.transpose(1, 2)).squeeze(1)   [B,1,768]x[B,768,M]
//   forward     (:206-208)  start_logits = start.matmul(query_start.transpose(1, 2)).squeeze(-1)        [bs,T,768]x[bs,768,1]
//                           dense_logits = start_logits.unsqueeze(2) + end_logits.unsqueeze(1)
// Both contractions are out[b, m] = <q[b, :], vecs[b, m, :]> -- the dot of the window kernel without the gather: one
// wavefront per (b, m), 12 contiguous floats per lane, fp32 FMA chain in a fixed order, butterfly.  HBM-bound
// (3 KiB read per output); the vectors are the [B, 2k, 768] arrays MIPS.search(return_idxs=True) returns.
__global__ __launch_bounds__(256) void dph_score_vecs_kernel(const float* __restrict__ q, const float* __restrict__ vecs,
                                                             int64_t n_b, int64_t m, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= n_b * m) return;
    const int64_t b = c / m;
    const float4* qp = (const float4*)(q + b * DPH_DIM + lane * 12);
    const float4* vp = (const float4*)(vecs + c * DPH_DIM + lane * 12);
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float4 a = qp[i], v = vp[i];
        acc = fmaf(a.x, v.x, acc); acc = fmaf(a.y, v.y, acc); acc = fmaf(a.z, v.z, acc); acc = fmaf(a.w, v.w, acc);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) out[c] = acc;
}
// gradient of the above w.r.t. q (what query-side fine-tuning back-propagates into the query encoder,
// train_query.py:208-275): grad_q[b, j] = sum_m grad[b, m] * vecs[b, m, j]; one workgroup per b, 3 columns per thread
__global__ __launch_bounds__(256) void dph_score_vecs_bwd_kernel(const float* __restrict__ grad, const float* __restrict__ vecs,
                                                                 int64_t m, float* __restrict__ grad_q) {
    const int64_t b = blockIdx.x;
    float acc[3] = {0.f, 0.f, 0.f};
    for (int64_t i = 0; i < m; ++i) {
        const float g = grad[b * m + i];
        const float* v = vecs + (b * m + i) * DPH_DIM;
#pragma unroll
        for (int t = 0; t < 3; ++t) acc[t] = fmaf(g, v[threadIdx.x + 256 * t], acc[t]);
    }
#pragma unroll
    for (int t = 0; t < 3; ++t) grad_q[b * DPH_DIM + threadIdx.x + 256 * t] = acc[t];
}
// dense_logits[b, i, j] = start_logits[b, i] + end_logits[b, j]   (encoder.py:208)
__global__ __launch_bounds__(256) void dph_dense_logits_kernel(const float* __restrict__ s, const float* __restrict__ e,
                                                               int64_t n_b, int64_t T, float* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n_b * T * T) return;
    const int64_t b = idx / (T * T), r = idx % (T * T);
    out[idx] = s[b * T + r / T] + e[b * T + r % T];
}

void dph_launch_score_vecs(const float* q, const float* vecs, int64_t n_b, int64_t m, float* out, hipStream_t st) {
    if (n_b * m <= 0) return;
    hipLaunchKernelGGL(dph_score_vecs_kernel, dim3((unsigned)((n_b * m + 3) / 4)), dim3(256), 0, st, q, vecs, n_b, m, out);
}
void dph_launch_score_vecs_bwd(const float* grad, const float* vecs, int64_t n_b, int64_t m, float* grad_q, hipStream_t st) {
    if (n_b <= 0) return;
    hipLaunchKernelGGL(dph_score_vecs_bwd_kernel, dim3((unsigned)n_b), dim3(256), 0, st, grad, vecs, m, grad_q);
}
void dph_launch_dense_logits(const float* s, const float* e, int64_t n_b, int64_t T, float* out, hipStream_t st) {
    if (n_b * T * T <= 0) return;
    hipLaunchKernelGGL(dph_dense_logits_kernel, dim3((unsigned)((n_b * T * T + 255) / 256)), dim3(256), 0, st, s, e, n_b, T, out);
}
