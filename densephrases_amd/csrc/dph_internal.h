// dph_internal.h -- shared constants / device structs of libdph (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <atomic>
#include <string>
#include <utility>
#include <vector>
#include "../../include/dph_debug.h"      // (includes dph.h: the contract + the tuning / profiling / debug entry points)
#include "dph_geometry.h"                 // the constants the kernels share with the host planning rules (dph_plan.h)

// ---------------------------------------------------------------- errors and ownership (host side)
// The one error channel: fail() stores the message dph_last_error() returns (thread-local, dph_api.hip) and hands the code back.
int fail(int code, const std::string& msg);
#define HIPCHK(expr)                                                                                 \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess)                                                                        \
            return fail(e_ == hipErrorOutOfMemory ? DPH_E_NOMEM : DPH_E_HIP,                         \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                          \
    } while (0)

// Owner of one hipMalloc allocation of `n` elements.  Move-only; the destructor frees, so the struct a dev_buf is a member of releases
// it wherever that struct dies (with its device current: dph_index_destroy / dph_pq_free).  Reads as a plain T* at the call sites.
template <typename T> struct dev_buf {
    T* p = nullptr;
    size_t n = 0;
    dev_buf() = default;
    dev_buf(const dev_buf&) = delete;
    dev_buf& operator=(const dev_buf&) = delete;
    dev_buf(dev_buf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    dev_buf& operator=(dev_buf&& o) noexcept { if (this != &o) { reset(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; } return *this; }
    ~dev_buf() { reset(); }
    hipError_t alloc(size_t count) {     // frees what it held; on failure it holds nothing
        reset();
        const hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
        if (e == hipSuccess) n = count; else p = nullptr;
        return e;
    }
    void reset() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
    operator T*() const { return p; }
};

// Owner of the (start, stop) event pairs that bracket profiled launches.
struct dph_event_pairs {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> v;
    dph_event_pairs() = default;
    dph_event_pairs(const dph_event_pairs&) = delete;
    dph_event_pairs& operator=(const dph_event_pairs&) = delete;
    ~dph_event_pairs() { for (auto& ev : v) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); } }
    std::pair<hipEvent_t, hipEvent_t> take() {           // a pair of this (free) list, or a new one when it is empty
        std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
        if (!v.empty()) { ev = v.back(); v.pop_back(); }
        else { (void)hipEventCreate(&ev.first); (void)hipEventCreate(&ev.second); }
        return ev;
    }
};
// The profiler of a handle: while `on`, chosen launches run between an event pair of their own -- what a rocprofv3 kernel trace
// reports per dispatch, so the two can be held against each other.  A bracketed launch leaves its pair in a list of the handle until
// drain() reads that list and hands the pairs back to `idle`.
struct dph_profiler {
    bool on = false;
    dph_event_pairs idle;
    // create the events now: the first hipEventCreate of a process can take ~100 ms, and it must not land in a timed region
    hipError_t warm(size_t n) {
        while (idle.v.size() < n) {
            std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
            hipError_t e = hipEventCreate(&ev.first);
            if (e == hipSuccess) e = hipEventCreate(&ev.second);
            if (e != hipSuccess) return e;
            idle.v.push_back(ev);
        }
        return hipSuccess;
    }
    // `launch` between a (start, stop) pair that goes to `list`; list == NULL: the launch alone
    template <typename Launch> void bracket(dph_event_pairs* list, hipStream_t st, Launch launch) {
        std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
        if (list) { ev = idle.take(); (void)hipEventRecord(ev.first, st); }
        launch();
        if (list) { (void)hipEventRecord(ev.second, st); list->v.push_back(ev); }
    }
    // every bracketed launch of `list` since the last read: total and count, each duration to each_out[0 .. cap) when asked
    int drain(dph_event_pairs& list, double* total_out, int* cnt_out, double* each_out = nullptr, int cap = 0) {
        std::vector<std::pair<hipEvent_t, hipEvent_t>> evs;
        evs.swap(list.v);               // back to `idle` first: a read that fails below leaves every pair with ONE owner
        idle.v.insert(idle.v.end(), evs.begin(), evs.end());
        double total = 0.0;
        int cnt = 0;
        for (auto& ev : evs) {
            HIPCHK(hipEventSynchronize(ev.second));
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, ev.first, ev.second));
            total += ms;
            if (each_out && cnt < cap) each_out[cnt] = ms;
            ++cnt;
        }
        if (total_out) *total_out = total;
        if (cnt_out) *cnt_out = cnt;
        return DPH_OK;
    }
};

// Dynamic LDS beyond the default limit is granted per kernel and device: asked for once (`done`: a static of the call site -- zero-
// initialised; handles are searched from several threads), asked again by the next call when it was refused.
static inline void dph_allow_lds(const void* kernel, const char* name, size_t bytes, int dev, std::atomic<bool> (&done)[64]) {
    if (dev >= 0 && dev < 64 && done[dev]) return;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) fprintf(stderr, "libdph: hipFuncSetAttribute(%s, %zu B of LDS): %s\n", name, bytes, hipGetErrorString(e));
    if (dev >= 0 && dev < 64) done[dev] = e == hipSuccess;
}
static inline int dph_current_device() { int dev = 0; (void)hipGetDevice(&dev); return dev; }
#define DPH_ALLOW_LDS(KERNEL, BYTES, DEV)                                           \
    do {                                                                            \
        static std::atomic<bool> done_[64];                                         \
        dph_allow_lds((const void*)KERNEL, #KERNEL, (BYTES), (DEV), done_);         \
    } while (0)

// The small device counters of a pass, each ONE allocation of one struct (dph_api.hip): host code hands the kernels field addresses.
// Cleared in front of every scan launch (dph_clear_pass_counters): the scan counts and flags, the outlier / refine kernels behind it
// fill the buckets, threshold / select read all of it.
struct dph_pass_counters {
    int queue_head;                             // work-queue head of the flat / masked scan
    unsigned chunks_claimed;                    // chunks claimed from the pair pool: the scan kernels find it one word behind queue_head
    unsigned pad[2];
    unsigned bucket_counts[DPH_PASS_MAX];       // keys in every query row's bucket
    unsigned overflow[DPH_PASS_MAX];            // row lost pairs (the pair pool ran dry)
};
static_assert(offsetof(dph_pass_counters, chunks_claimed) == offsetof(dph_pass_counters, queue_head) + sizeof(int) &&
              offsetof(dph_pass_counters, bucket_counts) == 16 && sizeof(dph_pass_counters) == 16 + 2 * DPH_PASS_MAX * sizeof(unsigned),
              "dph_scan_kernel derives chunks_claimed from queue_head; the accumulating scan clears the 16 bytes in front of the bucket counts");
// ... and of a unit-scan pass: cleared and written by dph_launch_units_build, the heads popped by the scan launches
struct dph_unit_counters {
    int chunks, units, error, spare;            // chunks and units of the pass (dph_units_offsets_kernel); error: a table would have overflowed
    int next[DPH_UNIT_LAUNCHES];                // work-queue heads, one per scan launch
};
static_assert(offsetof(dph_unit_counters, units) == 4 && offsetof(dph_unit_counters, error) == 8 && offsetof(dph_unit_counters, next) == 16,
              "dph_units_offsets_kernel / dph_units_build_kernel write counts[0..2]");

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

// per query row scalars produced by the quantiser, consumed by the select/certify kernel (all float64)
struct dph_qinfo {
    double sc;        // q_j ~= sc * (128*q1_j + q2_j)
    double e_norm2;   // || e ||_2,  e_j = q_j - sc*(128*q1_j+q2_j)
    double e_mu;      // <e, mu>  (mu = the shard's per-dimension mean code)
    double q_sum;     // sum_j q_j
    double q_l1;      // sum_j |q_j|
};

// 64-bit candidate key: high word = score biased to unsigned, low word = ~local_row, so that unsigned
// descending order is (score desc, row asc).  0 is the "empty" sentinel.
__host__ __device__ static inline uint64_t dph_make_key(int32_t score, uint32_t row) {
    return ((uint64_t)((uint32_t)score ^ 0x80000000u) << 32) | (uint64_t)(0xFFFFFFFFu - row);
}
__host__ __device__ static inline int32_t dph_key_score(uint64_t key) {
    return (int32_t)((uint32_t)(key >> 32) ^ 0x80000000u);
}
__host__ __device__ static inline uint32_t dph_key_row(uint64_t key) {
    return 0xFFFFFFFFu - (uint32_t)key;
}

// id <-> stored-row translation of a shard built from several sub-indexes (the reference merges per-dump indexes whose
// ids are offset + local, offsets spaced max_idx apart: scripts/parallel/add_to_index.py:42-51, index.py:135-140):
// group g holds stored rows [row_starts[g], row_starts[g+1]) with ids id_offsets[g] + (row - row_starts[g]).
// n_groups = 0: ids are id_base + row.
struct dph_idmap {
    const int64_t* id_offsets; const int64_t* row_starts; int n_groups; int64_t id_base; int64_t n_ids;
};
__device__ __forceinline__ int64_t dph_id_of_row(const dph_idmap& m, int64_t row) {
    if (m.n_groups == 0) return m.id_base + row;
    int lo = 0, hi = m.n_groups - 1;                    // last group whose first row is <= row
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (m.row_starts[mid] <= row) lo = mid; else hi = mid - 1; }
    return m.id_offsets[lo] + (row - m.row_starts[lo]);
}
// stored row (flat / grouped shards) or local id (list-major shards: the caller maps it through inv_row), -1 = not here
__device__ __forceinline__ int64_t dph_local_of_id(const dph_idmap& m, int64_t id) {
    if (m.n_groups == 0) { const int64_t l = id - m.id_base; return (l < 0 || l >= m.n_ids) ? -1 : l; }
    if (id < m.id_offsets[0]) return -1;
    int lo = 0, hi = m.n_groups - 1;                    // last group whose offset is <= id
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (m.id_offsets[mid] <= id) lo = mid; else hi = mid - 1; }
    const int64_t r = id - m.id_offsets[lo];
    return r < m.row_starts[lo + 1] - m.row_starts[lo] ? m.row_starts[lo] + r : -1;
}

// ---- the stored OPQ + IVFPQ index as the reconstruct / window kernels read it (dph_pq.hip fills it, pq_store_of)
struct pq_store {
    const float* cent; const float* pqc; const uint8_t* codes; const int64_t* list_off; const int64_t* dm_ids; const unsigned* dm_pos;
    int64_t ntotal; int nlist; int M; int dsub; int by_residual;
};
// the direct map: position of the code of `id` in the list-major store, -1 = not in the index
__device__ __forceinline__ int64_t pq_pos_of_id(const int64_t* dm_ids, const unsigned* dm_pos, int64_t n, int64_t id) {
    int64_t lo = 0, hi = n;
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (dm_ids[mid] < id) lo = mid + 1; else hi = mid; }
    return (lo < n && dm_ids[lo] == id) ? (int64_t)dm_pos[lo] : -1;
}
__device__ __forceinline__ int pq_list_of_pos(const int64_t* list_off, int nlist, int64_t pos) {
    int lo = 0, hi = nlist - 1;                                  // last list whose offset is <= pos and that is not empty there
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (list_off[mid] <= pos) lo = mid; else hi = mid - 1; }
    return lo;
}
// component j of the reconstruction of the code at `pos` (rotated space, fp32: decode, then one add of the centroid)
__device__ __forceinline__ float pq_component(const pq_store& s, int64_t pos, int list, int j) {
    const int m = j / s.dsub, t = j - m * s.dsub;
    float v = s.pqc[((int64_t)m * 256 + s.codes[pos * s.M + m]) * s.dsub + t];
    if (s.by_residual) v = __fadd_rn(v, s.cent[(int64_t)list * DPH_DIM + j]);
    return v;
}

// ---- window re-score (dph_window.hip): what one launch is asked for, whatever serves the slot vectors.  Filled once per call by
// dph_rescore_dev (make_window_args); n_cand = n_q * k candidates, query half c / k for candidate c.
struct dph_window_args {
    int direction;                                              // 0: slots id + i (end windows), 1: id - i (start windows)
    dph_idmap idmap;
    const float* qhalf;                                         // [n_cand / k, 768]
    int64_t n_cand; int k; int L;
    const int64_t* ids; const int32_t* doc_in; const int32_t* word_in; const float* first;     // [n_cand]; doc_in / word_in NULL: idx2id
    const int32_t* row2doc; const int32_t* row2word;            // idx2id by local id
    const int32_t* doc_ids; int64_t n_docs; const int64_t* f2o_off; const int32_t* f2o;        // the f2o CSR
    int32_t* pred_word; double* best; int32_t* argslot; float* vecs;                           // [n_cand] x 3, [n_cand,2,768] or NULL
};
// The one launch.  pq = NULL: the raw int8 rows of a flat / grouped / list-major shard (rows [n_rows,768], lut, inv_row or NULL);
// pq, rows = NULL: reconstructions of the PQ index; pq and rows: the doc-row store [n_rows,768] in f2o-CSR order with its lut.
void dph_launch_window(const dph_window_args& a, const pq_store* pq, const int8_t* rows, int64_t n_rows, const float* lut,
                       const int32_t* inv_row, hipStream_t st);

// device-side gate of the retry launches: a kernel whose `gate` pointer is non-NULL serves rows
// [gate_base, min(*gate, gate_base + rows of the pass)) and exits at once when that range is empty, so the retry chain
// can be enqueued without a host round trip (it costs a few empty launches when every row certified).
__device__ __forceinline__ int dph_gated_rows(const int* gate, int gate_base, int n_q) {
    if (!gate) return n_q;
    const int left = *gate - gate_base;
    return left < 0 ? 0 : (left < n_q ? left : n_q);
}

// Work queue of the flat / masked scan (dph_scan.hip): segment `u` of `n_tiles` visited tiles for a grid of `grid`
// workgroups -- guided self-scheduling in phases of 2*grid segments, every phase dealing out half of what is left, so
// the segment length halves from n_tiles/(4*grid) down to `seg_min`.  Returns the segment's first tile (>= n_tiles: the
// queue is empty, and so it is for every later u) and its length in *len.  Shared by the kernel and, through
// dph_debug_guided_segment, by the CPU tests.
__host__ __device__ static inline int64_t dph_guided_segment(int64_t u, int64_t n_tiles, int grid, int seg_min, int64_t* len) {
    const int64_t per_phase = 2 * (int64_t)grid;
    int64_t first = 0, l = seg_min;
    for (int64_t k = u / per_phase;; --k) {
        const int64_t left = n_tiles - first;
        l = left / (2 * per_phase);
        l = l > (int64_t)seg_min ? l : (int64_t)seg_min;
        if (k == 0 || left <= 0) break;
        first += per_phase * l;
    }
    first += (u % per_phase) * l;
    *len = (first < n_tiles && n_tiles - first < l) ? n_tiles - first : l;
    return first;
}

// everything a pass of the search pipeline shares (filled by dph_api.hip, consumed by the launchers)
struct dph_pass {
    // shard
    const int8_t* db; int64_t n_rows; const int64_t* row_ids; dph_idmap idmap;
    int grid;                           // scan workgroups (= CUs)
    // the pass
    int qb;                             // 1 or 2: 128*qb query rows
    int q0;                             // first query row of the pass inside the call
    int n_q;                            // rows of the pass (host view; the gate may shrink it)
    const int* gate; int gate_base;     // device-side row count (retry passes), or NULL
    // query images (whole call)
    const float* x; const int8_t* qfrag_hi; const int8_t* q1; const int8_t* q2; const dph_qinfo* qinfo; const int* lmax;
    // the aux k-step: the shard's aux rows (NULL = none), their layout, the query rows' aux digits [row of the call][DPH_AUX_SLOTS]
    const int8_t* aux; dph_aux_layout aux_lay; const int8_t* qaux;
    // IVF
    const unsigned* tilemask;           // [n_tiles][8] words or NULL
    // IVF unit scan (unit_recs != NULL): work queue + gathered query fragments (dph_geometry.h: DPH_PASS_MAX)
    const int4* unit_recs;              // {first tile of the list, first tile of the segment, end tile, chunk}
    const int4* unit_list_recs;         // the same per chunk for the whole list (what the ladder levels walk)
    dph_unit_counters* unit_cnt;        // chunks, units (device side, written by dph_launch_units_build) and the work-queue heads
    int unit_launch;                    // which head the next scan launch uses
    const int* slot_q;                  // [chunk][128] query row of the pass in that MFMA column, -1 = empty
    const int8_t* unit_frags;           // [chunk][4][DPH_QGROUP_FRAG_BYTES] high digits in fragment order
    const unsigned* listmask;           // [nlist][mask_words]
    const int32_t* tile_list;           // [n_tiles]
    int mask_words;
    // outlier rows of the shard (sorted stored-row indices): scored against every query row, never bounded
    const unsigned* outliers; int n_out;
    // scratch
    uint2* pairs; unsigned* chunk_fill;         // [DPH_POOL_CHUNKS][DPH_CHUNK_PAIRS] pair pool, pairs in every claimed chunk
    unsigned* wave_counts;                      // [grid*4][2] (pairs, emit-path triggers) of every scan wave: statistics
    uint64_t* buckets;                          // [DPH_PASS_MAX][DPH_BUCKET_CAP]
    dph_pass_counters* cnt;                     // queue head, claimed chunks, bucket counts, overflow flags: zeroed by every scan launch
    int seg_tiles;                              // shortest queue segment in tiles (full scans; sampled levels: fewer)
    int sched;                                  // hand-over schedule of the flat full scan (dph_scan.hip hand_pos): 0 lock step, 1 wave after wave, 2 interleaved
    // the full scan behind a FUSED finest ladder level of stride S: skip_m = ceil(2^29 / (S - 1)) makes the scan skip the tiles
    // that level visited (0 = visit every tile), accumulate = keep the buckets / flags that level's refine filled
    unsigned skip_m; bool accumulate;
};

// launchers (defined in the .hip files, called from dph_api.hip)
struct dph_index;
// mu: the shard's per-dimension mean codes [768] (device); lay / norm_unit: its aux layout (stride 0: lmax carries the shard-wide norm
// bound ||q2|| rmax + <q2, mu>; otherwise lmax = <q2, mu> and the norm part rides in the aux digits qaux [row][DPH_AUX_SLOTS])
void dph_launch_quantize(const float* x_dev, int64_t n_rows, const int* gate, int8_t* qfrag_hi, int8_t* q1, int8_t* q2,
                         dph_qinfo* qinfo_dev, double rmax, int* lmax_dev, int8_t* qaux, const int* mu_dev, const dph_aux_layout& lay,
                         int norm_unit, hipStream_t st, float* xc = nullptr, int32_t* nonfinite = nullptr);
void dph_launch_nonfinite_fix(const int32_t* flag, int64_t n, int k, float* D, int64_t* I, int32_t* status, double* bound, int* count,
                              hipStream_t st);
// per-dimension sums of the stored rows (row_ids != NULL: padding rows skipped): sums[0..767] = sum n_j, sums[768..1535] = sum n_j^2
void dph_launch_colstats(const int8_t* db, int64_t n_rows, const int64_t* row_ids, long long* sums, hipStream_t st);
// aux rows of a shard: [n_tiles * 32][lay.stride] (padding rows zero)
void dph_launch_aux_build(const int8_t* db, int64_t n_rows, int64_t n_rows_padded, const int64_t* row_ids, const int* mu_dev,
                          const dph_aux_layout& lay, int norm_unit, int8_t* aux, hipStream_t st);
// filter scan of every `tile_stride`-th tile (n_tiles_visit of them) under the per-row bounds tau (NULL = none: every
// row of the visited tiles is emitted -- cold start of the ladder / tiny shards)
void dph_launch_scan(const dph_pass& p, bool sample, int64_t n_tiles_visit, int tile_stride, const int* tau, hipStream_t st);
// unit scan: every unit visits the tiles of its segment whose index inside the list is a multiple of `tile_stride`;
// `rowmask` (bit r = accumulator register r of a lane, 2 rows each) restricts what a visited tile may emit (cold level)
void dph_launch_scan_units(const dph_pass& p, bool sample, int tile_stride, unsigned rowmask, const int* tau, hipStream_t st);
void dph_clear_pass_counters(const dph_pass& p, hipStream_t st);     // issued by every scan launch
void dph_launch_refine(const dph_pass& p, hipStream_t st);
void dph_launch_threshold(const dph_pass& p, int kp, const int* floor_tau, int* tau_out, int* top_out, hipStream_t st);
void dph_launch_union_bounds(const int* top_parts, int n_parts, int64_t n, int* tau_out, hipStream_t st);
int  dph_scan_grid(int device);
struct dph_select_args {
    const float* lut; int k; int C; double rmax; double rmax_all; double delta_max; float offset; float scale;
    const int* tau;                     // bound the pass was scanned under (NULL = none)
    const int* rowmap;                  // retry passes: slot -> row of the call (outputs go to rowmap[slot]); NULL = identity
    float* D; int64_t* I; int32_t* status; double* bound_out; int32_t* ik_out; int32_t* fail_out;
    const int32_t* only_failed;         // != NULL: a second look at the same buckets -- only rows whose flag is set (and whose pairs are all there)
    int* reselect_count;                // ... counting the rows it certifies
};
void dph_launch_select(const dph_pass& p, const dph_select_args& a, hipStream_t st);
// ---- the coarse quantizer (dph_ivf.hip)
// Its scratch, one per index handle (two handles searched from two threads never share it): allocated by the launchers on first use (they
// know the sizes), never shrunk, freed with the handle.  Each part is held whole or not at all -- a part that cannot be allocated is
// tried again by the next call, which meanwhile takes the path that does without it.
struct dph_coarse_counters {            // cleared by one memset per filter pass
    unsigned cand_cnt[DPH_PASS_MAX];    // candidates of every row
    unsigned est[DPH_PASS_MAX];         // threshold estimate (score key) of every row
    unsigned pool_count, fail;          // pairs the scan emitted (a statistic); 1 = the pass fails over to the chain
    int gate;                           // rows the fail-over chain serves: all of the pass or none
    unsigned spare[13];                 // (pads the struct to a whole number of 16-byte units)
};
struct dph_coarse_scratch {
    struct chain_part {                 // one-pass probe selection over long score rows
        dev_buf<uint2> cand; dev_buf<unsigned> cand_cnt, est;      // [DPH_PASS_MAX][CS_CAND] (list, key), [DPH_PASS_MAX], [DPH_PASS_MAX]
    } chain;
    struct filter_part {                // the filter; its candidate lists are its own (the fail-over chain runs behind it)
        dev_buf<float> sample;                                      // [DPH_PASS_MAX][CF_SAMPLE] scores of the sampled lists
        dev_buf<uint2> cand;                                        // [DPH_PASS_MAX][CS_CAND]
        dev_buf<dph_coarse_counters> cnt;                           // [1]
        // the filter scan: pair pool and its chunk fills, per-wave statistics, queue counters, query fragments of a whole pass
        dev_buf<uint2> pairs; dev_buf<unsigned> chunk_fill, wave_counts; dev_buf<int> counters; dev_buf<uint4> qfrag;
    } filter;
};
// One coarse search: the nprobe best lists of query rows [q0, q0 + n_q) of x [.., 768], as bits of listmask [nlist][mask_words] (bit = row
// of the pass; NULL: none), per tile in tilemask (8 words per tile, mask_words == 8 only; NULL: none) and / or as a list per row in
// probe_out [n_q][probe_stride] (-1 padded, order unspecified: what a scan that groups its work by query row walks; NULL: none).
struct dph_coarse_args {
    const float* x = nullptr; int q0 = 0; int n_q = 0;
    const int* gate = nullptr; int gate_base = 0;
    const float* centroids = nullptr; int nlist = 0; int nprobe = 0; double cnorm_max = 0.0;
    float* scores = nullptr;                                    // [n_q][nlist] scratch
    unsigned* listmask = nullptr; int mask_words = 0;
    const int32_t* tile_list = nullptr; int64_t n_tiles = 0; unsigned* tilemask = nullptr;
    int* probe_out = nullptr; int probe_stride = 0;
    // packed bf16 hi / lo images (dph_launch_bf16_split) of the centroids [nlist,768] and of the query rows [>= q0 + n_q, 768] when the
    // caller keeps them (dph_pq.hip): the long-quantizer GEMM then unpacks instead of splitting
    const unsigned* c_pk = nullptr; const unsigned* x_pk = nullptr;
    unsigned* row_fail = nullptr;                               // [n_q] set for a row whose error band overflows the re-rank (NULL: the band is cut)
    bool clear_mask = true;                                     // false: OR into the listmask as it is
};
void dph_launch_coarse(const dph_coarse_args& a, dph_coarse_scratch& s, hipStream_t st);
// The int8 scans multiply with v_mfma_i32_16x16x64_i8 (dph_scan.hip, round 6), and the high-digit query fragments are written in
// that instruction's operand order: entry [2 s + h][lane] (16 bytes) of a group of 32 query rows = bytes 64 s + 16 (lane >> 4) .. + 15
// of query row 16 h + (lane & 15).  (DPH_SCAN_X16 = 0 builds the 32 x 32 x 32 kernels of rounds 1-5 for A/B timing: entry [ks][lane] =
// bytes 32 ks + 16 (lane >> 5) .. + 15 of query row lane & 31.)  Both are [24][64][16 B] per group.
#ifndef DPH_SCAN_X16
#define DPH_SCAN_X16 1
#endif
__host__ __device__ static inline bool dph_frag_x16(int aux_stride) { (void)aux_stride; return DPH_SCAN_X16 != 0; }
// long quantizers, the filter in front of the chain: a one-product bf16 scan under a sampled threshold (dph_ivf.hip).  A whole pass from
// row 0 (q0 = 0, no gate, no tiles); c_pk / x_pk feed its fail-over chain.
struct dph_coarse_filter_args : dph_coarse_args {
    const unsigned short* c_hi = nullptr; const unsigned short* x_hi = nullptr;       // bf16 images of the centroids (chunk-major) and of the query rows
    const unsigned short* c_pieces = nullptr;                                         // the centroids piece-major (NULL: the chain alone)
    const float* cnorm = nullptr;       // [nlist] ||c_l||_2 (device)
    double cnorm_cap = 0.0;             // lists longer than this get exact scores
    int teams = 1;                      // more than 128 rows: one launch of workgroup teams sharing tiles through L2 (dph_scan.hip MODE 4)
    // profiling: an event pair of its own around EVERY launch of the filter's dominant kernel (the scan), appended to prof_list.
    // Both NULL: none
    dph_profiler* prof = nullptr; dph_event_pairs* prof_list = nullptr;
};
void dph_launch_coarse_filter(const dph_coarse_filter_args& a, dph_coarse_scratch& s, hipStream_t st);
void dph_launch_coarse_scan_teams(const void* img, int64_t n_lists, const void* qfrag, int n_q, int n_groups, const unsigned* est_keys, uint2* pairs,
                                  unsigned* chunk_fill, unsigned* wave_counts, int* counters, int grid, hipStream_t st);
// the coarse quantizer's filter as a SCAN (dph_scan.hip MODE 3) over the piece-major bf16 image
// [tile of 32 lists][half of k][32 rows][384 bf16] (dph_launch_bf16_pieces; dph_bf16_piece_rows(n) rows allocated); hits land in
// chunks of the pair pool as (list | query row << 20, score key)
void dph_launch_bf16_pieces(const float* v, int64_t n_rows, unsigned short* out, hipStream_t st);
int64_t dph_bf16_piece_rows(int64_t n_rows);
void dph_launch_coarse_scan(const void* img, int64_t n_lists, const void* qfrag, int n_q, const unsigned* est_keys, uint2* pairs,
                            unsigned* chunk_fill, unsigned* wave_counts, int* counters, int grid, hipStream_t st);
int dph_coarse_filter_debug(const dph_coarse_scratch& s, unsigned out[2]);
// chunk-major bf16 image of a [n_rows, 768] fp32 matrix, what the sample GEMM reads (dph_bf16_hi_rows(n) rows allocated)
void dph_launch_bf16_hi(const float* v, int64_t n_rows, unsigned short* hi, hipStream_t st);
int64_t dph_bf16_hi_rows(int64_t n_rows);
void dph_launch_bf16_split(const float* v, int64_t n_elems, unsigned* packed, hipStream_t st);
// IVF scratch of a handle: what a pass writes (dph_index_set_ivf sizes it from the lists) ...
struct dph_ivf_pass {
    dev_buf<float> coarse_scores;       // [coarse_rows, nlist] fp32: query x centroid scores of the current pass
    int coarse_rows = 0;
    dev_buf<unsigned> listmask;         // [nlist][8]   bit j of word w: query row 32w+j of the pass probes the list
    dev_buf<unsigned> tilemask;         // [n_tiles][8] the same per tile (what the scan reads)
    dev_buf<int2> unit_offsets;         // [nlist] first chunk / first unit of every list in the current pass
    dev_buf<unsigned> listmask_u;       // [nlist][DPH_UNIT_WORDS]
    dev_buf<dph_unit_counters> unit_cnt;    // [1]
};
// ... and the work queue of a unit-scan pass of up to DPH_PASS_MAX query rows (sized from nprobe)
struct dph_unit_queue {
    dev_buf<int> slot_q; dev_buf<int4> unit_recs, unit_list_recs; dev_buf<int8_t> unit_frags;
    int chunk_cap = 0, unit_cap = 0;
};
// work queue of a unit-scan pass from the probe masks ivf.listmask_u: chunks, slot tables, unit records, gathered fragments
void dph_launch_units_build(const dph_ivf_pass& ivf, const dph_unit_queue& uq, int nlist, const int* list_tile0, const int8_t* q1, int q0,
                            int spread, bool x16, hipStream_t st);
// list assignment (arg-max over the centroids, fused: no score matrix); rows = fp32 [n,768] or int8 rows + the shard's LUT
void dph_launch_assign(const void* rows, bool rows_int8, const float* lut, int64_t n, const float* centroids, int nlist,
                       const float* bias, int32_t* best, float* gap, hipStream_t st);
// k-means centroid update over int8 rows (dph_kmeans.hip): sums [nlist,768] int64 and counts [nlist] are scratch + output
void dph_launch_kmeans_update(const int8_t* rows, const int32_t* assign, int64_t m, int nlist, float offset, float scale,
                              int spherical, long long* sums, unsigned* counts, float* centroids, hipStream_t st);
void dph_launch_gather_sample(const int8_t* db, int64_t n_rows, const int64_t* idx, int64_t m, int8_t* out, hipStream_t st);
// retry plumbing: compact the failing rows of a call (fail flags -> rows[], *count), gather their query vectors
void dph_launch_compact_failing(const int32_t* fail, int64_t n, int match, const float* x, int32_t* rows_out, int* count_out,
                                float* x_out, int max_rows, hipStream_t st);
void dph_launch_gather_rows(const float* x, const int32_t* rows, const int* count, float* x_out, int max_rows, hipStream_t st);
void dph_launch_count_status(const int32_t* status, int64_t n, int* out, hipStream_t st);
void dph_launch_retry_tau(const int* gate, int64_t n_max, const int32_t* rows, const int32_t* ik, const dph_qinfo* qinfo,
                          double rmax, double delta_max, float scale, int* tau_out, hipStream_t st);

void dph_launch_exact(const int8_t* db, int64_t n_rows, dph_idmap idmap, const float* x_dev, const float* lut_dev,
                      const int32_t* rows_dev, const int* n_fail_dev, int n_fail_max, int k, const int64_t* row_ids,
                      const unsigned* tilemask, float* D, int64_t* I, int32_t* status, void* scratch,
                      size_t scratch_bytes, hipStream_t st, int tighten_rounds = 1);
// device-side list builder (dph_build.hip): rows sorted by (list, row) + the first sorted position of every list
int dph_list_major_sort(const int32_t* assign_dev, int64_t n, int nlist, uint64_t** keys_out, int64_t* starts_host, hipStream_t st);
void dph_launch_list_major_gather(const int8_t* src, const uint64_t* keys, int64_t n, const int64_t* src_start_dev,
                                  const int64_t* dst_start_dev, int64_t id_base, int8_t* dst, int64_t* row_ids,
                                  int32_t* inv_row, hipStream_t st);
// (id, position) pairs sorted by id: the direct map of a PQ index
int dph_sort_pairs_i64_u32(const int64_t* keys_in, const unsigned* vals_in, int64_t* keys_out, unsigned* vals_out, int64_t n, hipStream_t st);
void dph_launch_fill(int8_t* db, int64_t n_rows, int64_t id_base, uint64_t seed, int kind, hipStream_t st);
void dph_launch_rownorm(const int8_t* db, int64_t n_rows, const int64_t* row_ids, const int* mu_dev, unsigned long long* max_out,
                        unsigned* hist, unsigned long long cut2, unsigned* out_rows, unsigned* out_count, unsigned out_cap,
                        hipStream_t st);
void dph_launch_merge(const float* D_parts, const int64_t* I_parts, const double* best_parts, const int32_t* pred_parts,
                      const int32_t* status_parts, const double* bound_parts, int n_parts, int64_t stride_bytes, int64_t n,
                      int k, float* D_out, int64_t* I_out, int32_t* src_out, double* best_out, int32_t* pred_out,
                      int32_t* status_out, hipStream_t st);
void dph_launch_score_vecs(const float* q, const float* vecs, int64_t n_b, int64_t m, float* out, hipStream_t st);
void dph_launch_score_vecs_bwd(const float* grad, const float* vecs, int64_t n_b, int64_t m, float* grad_q, hipStream_t st);
void dph_launch_dense_logits(const float* s, const float* e, int64_t n_b, int64_t T, float* out, hipStream_t st);

// ---- the reference's own index type, IndexPreTransform(OPQMatrix) -> IndexIVFPQ, resident in HBM (dph_pq.hip)
struct dph_pq;
int dph_pq_alloc(dph_pq** out, int device, int64_t ntotal, int nlist, int M);
void dph_pq_free(dph_pq* p);
int dph_pq_set_params(dph_pq* p, const float* A, const float* b, const float* centroids, const float* pq_centroids, int by_residual);
int dph_pq_set_list_sizes(dph_pq* p, const int64_t* sizes);
int dph_pq_upload(dph_pq* p, int64_t pos0, int64_t n, const uint8_t* codes, const int64_t* ids);
int dph_pq_finalize(dph_pq* p, hipStream_t st);
// the add step (build_phrase_index.py:145-153): rows -> (list, codes) behind the handle's parameters, and all codes -> the handle's lists
int dph_pq_encode(dph_pq* p, const float* x_dev, int64_t n, int32_t* list_dev, uint8_t* codes_dev, hipStream_t st);
int dph_pq_fill(dph_pq* p, int64_t n, const int32_t* list_dev, const uint8_t* codes_dev, const int64_t* ids_dev, hipStream_t st);
int dph_pq_get_list_sizes(dph_pq* p, int64_t* sizes);
int dph_pq_download(dph_pq* p, int64_t pos0, int64_t n, uint8_t* codes, int64_t* ids);
// ... its kernels (dph_pq_encode.hip)
void dph_launch_pq_relist(const float* xp, int64_t n, const float* cent, int nlist, const int32_t* nonfinite, const float* gap, double cnorm_max,
                          int32_t* list, hipStream_t st);
int dph_launch_pq_codes(const float* xp, int64_t n, const int32_t* list, const float* cent, int by_residual, const float* pqc, const float* bias,
                        const float* wmax, int M, uint8_t* codes, int device, hipStream_t st);
void dph_launch_pq_fill_keys(const int32_t* list, int64_t n, int nlist, int64_t* keys, unsigned* vals, unsigned* counts, int* bad, hipStream_t st);
void dph_launch_pq_fill_gather(const unsigned* src, int64_t n, int M, const uint8_t* codes_in, const int64_t* ids_in, uint8_t* codes_out, int64_t* ids_out,
                               hipStream_t st);
bool dph_pq_ready(const dph_pq* p);
int64_t dph_pq_ntotal(const dph_pq* p);
int dph_pq_nlist(const dph_pq* p);
const float* dph_pq_A_host(const dph_pq* p);
void dph_pq_set_coarse_teams(dph_pq* p, int on);               // tuning key "coarse_teams"
void dph_pq_set_coarse_filter(dph_pq* p, int on);              // tuning key "coarse_filter"
int dph_pq_coarse_debug(dph_pq* p, unsigned out[2]);
int dph_pq_debug_phases(dph_pq* p, int which, unsigned long long* out, int cap);
int dph_pq_debug_pass(dph_pq* p, int* info, unsigned* per_row, int n);
int dph_coarse_select_clock(unsigned long long* out, int cap_rows);
// measurement hook: HIP events around the launches of the coarse quantizer's dominant kernel, the filter scan, in every pass (dph_profile_enable / _read on a PQ index)
int dph_pq_profile(dph_pq* p, int on);
int dph_pq_profile_read(dph_pq* p, double* ms_total, int* launches);
int dph_pq_profile_read_each(dph_pq* p, int which, double* ms_out, int cap, int* n_out);
int dph_pq_search_dev(dph_pq* p, const float* x_dev, int64_t n, int k, int nprobe, float* D, int64_t* I, int32_t* status, hipStream_t st);
int dph_pq_reconstruct_dev(dph_pq* p, const int64_t* ids_dev, int64_t n, float* out_dev, int32_t* found_dev, hipStream_t st);
// window re-score of a PQ shard: doc_rows = NULL re-scores reconstructions, otherwise the raw int8 rows of whole documents (the
// reference's HDF5 branch, dph_index_attach_doc_rows; doc_lut = the single-rounding codec table).  a.qhalf is rotated here.
int dph_pq_window(dph_pq* p, dph_window_args a, const int8_t* doc_rows, int64_t n_doc_rows, const float* doc_lut, hipStream_t st);
