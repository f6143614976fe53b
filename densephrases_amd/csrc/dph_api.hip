// dph_api.hip -- the C ABI of libdph (include/dph.h): handle management, host<->HBM plumbing, and the
// search driver (quantise -> sampled bounds -> int8 filter scan -> refine -> select/certify -> on-device retry ->
// fp64 fallback).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "dph_internal.h"
#include "dph_plan.h"

static thread_local std::string g_err;
// (a HIP call that failed leaves its code as the thread's "last error" until somebody reads it: rocPRIM checks hipGetLastError() after its
// launches and would report the stale code of a REFUSED call -- dph_index_create on a device that does not exist -- as the failure of the
// next index's finalize.  An error that has been turned into a return code is consumed here.)
int fail(int code, const std::string& msg) {
    g_err = msg;
    if (code == DPH_E_HIP || code == DPH_E_NOMEM) (void)hipGetLastError();
    return code;
}
// A handle is three things with three lifetimes, each a plain struct whose destructor is the only place its memory is released
// (dev_buf members; dph_index_destroy makes the device current and deletes):
//   dph_shard    the rows, metadata and shard constants -- owned by the handle dph_index_create made, shared by its twins;
//   dph_scratch  what a search (or a measurement hook) allocates on demand -- every handle its own;
//   dph_tuning   the values dph_index_set_tuning sets -- every handle its own, a twin starts from a copy.
struct dph_shard {
    int64_t n_rows = 0, n_tiles = 0, id_base = 0;   // n_rows = stored rows (incl. list padding on IVF shards)
    int64_t n_ids = 0;                   // ids the shard answers for: [id_base, id_base + n_ids)
    dev_buf<int8_t> db;                  // [n_tiles*32, 768] int8, padding rows zero
    // list-major (IVF) shards: row <-> id maps, per-tile list ids, centroids
    dev_buf<int64_t> row_ids;            // [n_rows] global id of a stored row, -1 = padding
    dev_buf<int32_t> inv_row;            // [n_ids]  stored row of local id
    // shards merged from several sub-indexes: ids = id_offsets[g] + (row - row_starts[g])
    std::vector<int64_t> h_id_offsets, h_row_starts;
    dev_buf<int64_t> id_offsets, row_starts;
    std::vector<int32_t> h_inv;
    int nlist = 0;
    dev_buf<float> centroids;            // [nlist, 768] fp32
    double cnorm_max = 0.0;              // max_l || c_l ||_2 (error band of the fp32 coarse scores)
    dev_buf<int32_t> tile_list;          // [n_tiles]
    dev_buf<unsigned> onesmask;          // [n_tiles][8] all ones: exact (flat) search over a list-major shard
    // unit scan (lists stored as contiguous runs of tiles)
    bool lists_contiguous = false;
    dev_buf<int> list_tile0;             // [nlist+1] first tile of every list
    int max_list_tiles = 0; int64_t total_segs = 0;
    float offset = -2.f, scale = 20.f;
    float lut_host[256];
    dev_buf<float> lut_dev;
    double delta_max = 0.0;              // max_n | x32(n) - (n/scale + offset) |
    double rmax = 0.0;                   // max over NON-outlier rows of || n - mu ||_2: the certificate's shard constant
    double rmax_all = 0.0;               // the same over every row
    double rmed = 0.0;                   // median of the same
    // per-dimension mean codes of the stored rows (integers): the centre of every Cauchy-Schwarz bound of the search
    int mu_host[DPH_DIM] = {0};
    double sd_host[DPH_DIM] = {0};       // per-dimension spread (what the rogue dimensions are told from)
    dev_buf<int> mu_dev; dev_buf<long long> colsum_dev;
    dev_buf<unsigned long long> norm_dev; dev_buf<unsigned> hist_dev;    // dph_index_finalize: largest squared row norm | outlier count, histogram
    // aux rows (dph_scan.hip "the aux k-step"): per-row norm codes + raw codes of the rogue dimensions
    dev_buf<int8_t> aux;
    dph_aux_layout aux_lay{};            // stride 0: the shard has none (its rows are alike: one norm bound serves them all)
    int norm_unit = 1;                   // a norm code counts this many units of || n - mu ||
    int aux_mode = -1;                   // tuning key "aux": -1 = decided by dph_index_finalize, 0 = never, 4 = norm codes, 16 / 32 = norm codes + 12 / 24 replica slots
    bool aux_lay_forced = false;         // the layout was set by dph_index_set_aux_layout (a sharded job: every rank the same digits)
    dev_buf<unsigned> outliers;          // sorted stored-row indices of the rows above the cut (always candidates)
    int n_out = 0;
    int n_out_found = 0; double rmax_cut = 0.0;   // what finalize found; in force only on a shard WITHOUT aux rows (derive_aux_units)
    bool finalized = false;
    // idx2id + f2o CSR
    dev_buf<int32_t> row2doc, row2word;
    std::vector<int32_t> h_row2doc, h_row2word;
    dev_buf<int32_t> doc_ids; dev_buf<int64_t> f2o_off; dev_buf<int32_t> f2o; int64_t n_docs = 0;
    int64_t f2o_total = 0;               // f2o_off[n_docs]: the words of all documents of the CSR
    // PQ index with the dump's raw rows next to its codes (dph_index_attach_doc_rows): the int8 `start` rows of WHOLE documents in the
    // order of the f2o CSR, row of (document slot d, word w) = f2o_off[d] + w -- what the reference's HDF5 branch reads (index.py:246-273)
    dev_buf<int8_t> doc_rows; int64_t n_doc_rows = 0;
    std::map<int64_t, int64_t> doc_rows_have;       // uploaded runs [first, second), merged: finalize wants exactly [0, n_doc_rows)
    float doc_lut_host[256];             // that branch's de-quantisation: fp32(n / scale + offset), float64 rounded ONCE (index.py:158-162, 334)
    dev_buf<float> doc_lut;
    // the reference's own index type (IndexPreTransform + IndexIVFPQ) instead of raw int8 rows: dph_pq.hip
    dph_pq* pq = nullptr;
    ~dph_shard() { if (pq) dph_pq_free(pq); }
};

struct dph_tuning {
    std::vector<int> ladder;             // explicit pre-pass strides, coarse -> fine; empty = derived from the shard size
    int fine_stride = 0;                 // 0 = default (32 on shards >= 100 M rows, 16 below)
    int sample_kp = 16;                  // the bound of a level = its kp-th best sampled score
    int max_qb = DPH_MAX_QB;
    int default_nprobe = 0;              // > 0: entry points without an nprobe argument search IVF (tuning key "nprobe")
    int ivf_spread = 1;                  // tuning key "ivf_spread": deal a chunk's query rows over the four scan waves first
    int ivf_units = -1;                  // tuning key "ivf_units": -1 = when the lists are long enough, 0 = never, 1 = always
    int grid = 256;                      // tuning key "scan_grid": scan workgroups (= CUs)
    int seg_tiles = 64;                  // tuning key "scan_seg": shortest work-queue segment of the flat scan, in tiles
    int ladder_fuse = 1;                 // tuning key "ladder_fuse": the full scan skips the tiles the finest ladder level scanned
    int retry_chain = 1;                 // tuning key "retry_chain": 0 = the first attempt only (rows it cannot certify come back with status 1)
    int scan_sched[2] = {1, 1};          // tuning key "scan_sched" (qb 1, qb 2): hand-over schedule of the flat full scan (dph_scan.hip); 1 = wave after
                                         // wave: 20.25 vs 20.47 ms (128 rows) and 29.4 vs 30.1 ms (256 rows) per 170 M-row launch (profiles/r04_scan_scheds_170M.json)
    int side_grid = 0;                   // tuning key "side_grid": scan workgroups of the prepare stage's sampled levels (0 = grid)
};

// The device counters of a search call, in the order the chain fills them.  A PQ index counts its rows' statuses into words of its own.
struct dph_search_counters {
    int fail_first;                      // rows failing the first attempt (the gate of the retry passes)
    int fail_retry;                      // rows failing the retry = rows of the fp64 fallback (its gate)
    int unsettled;                       // rows still flagged 1 at the end of the chain
    int reselect;                        // rows the in-pass wide re-select certified (no re-scan)
    int nonfinite;                       // non-finite query rows of the call
    struct { int uncertified, nonfinite; } pq;       // PQ index: what dph_launch_count_status counts (out[0], out[1])
    int spare;
};
static_assert(sizeof(dph_search_counters) == 32 && offsetof(dph_search_counters, nonfinite) == offsetof(dph_search_counters, reselect) + sizeof(int),
              "search_core clears reselect and nonfinite with one memset");
// the bound a pass's full scan runs under, and the stride of the last ladder level that ran under a bound itself (0 = none: nothing to fuse)
struct pass_bound { const int* tau = nullptr; int fuse_stride = 0; };

struct dph_scratch {
    int64_t cap_rows = 0;                // query rows the per-call scratch is sized for
    struct qimg { dev_buf<float> x; dev_buf<int8_t> frag, q1, q2; dev_buf<dph_qinfo> qinfo; dev_buf<int> lmax; dev_buf<int8_t> qaux;
                  dev_buf<int32_t> nf; };
    qimg q_main, q_retry;                // q_main.x: the query rows as every stage after the quantiser reads them (non-finite rows replaced by
                                         // their stand-in, q_main.nf flags them: dph_quantize_kernel); also the staging copy of the host entry points
    dev_buf<float> D_dev; dev_buf<int64_t> I_dev; dev_buf<int32_t> status_dev;   // host-pointer entry points
    int cap_k = 0;
    dev_buf<int32_t> ik_dev, fail_dev, fail2_dev, retry_rows, exact_rows;
    dev_buf<int> retry_tau;
    dev_buf<dph_search_counters> counters;       // [1]
    dev_buf<float> exact_x;
    dev_buf<char> exact_scratch;         // hit buffers of the fp64 fallback (its .n: their size in bytes)
    // per-pass scratch (fixed size)
    dev_buf<uint2> pairs; dev_buf<unsigned> chunk_fill, wave_counts; dev_buf<uint64_t> buckets;
    dev_buf<dph_pass_counters> pass_cnt; // [1] work-queue head | bucket counts | overflow flags of the current pass
    dev_buf<int> tau_dev;                // [2][DPH_PASS_MAX] per-row bounds of the current pass (ladder ping-pong)
    dph_ivf_pass ivf;                    // IVF: what a pass writes (dph_index_set_ivf sizes it from the lists) ...
    dph_unit_queue uq;                   // ... and the work queue of a unit-scan pass (ensure_units sizes it from nprobe)
    dph_coarse_scratch coarse;           // of the coarse quantizer (dph_launch_coarse allocates what it needs on first use)
    dev_buf<long long> kmeans_sums; int kmeans_nlist = 0;        // [nlist,768] integer sums of a k-means update
    dph_search_stats stats{};
    bool stats_pending = false;          // device counters of the last device-pointer call not read back yet
    // measurement hook: event pairs around scan launches
    dph_profiler prof;
    dph_event_pairs prof_events;         // around the full-scan launches
    dph_event_pairs prof_events_ladder;  // around the scan launches of the ladder levels
    // the two-stage form of a search (dph_search_prepare_dev / dph_search_finish_dev): what the prepare stage left behind
    struct prepared { bool valid = false; int64_t n = 0; int k = 0; pass_bound bound; } prep;
};

struct dph_index {
    int device = 0;
    dph_shard* sh = nullptr;             // the handle's own, or -- a twin -- the one of `twin_of`
    dph_tuning tune;
    dph_scratch sc;
    // a TWIN (dph_index_create_twin): a second handle over the shard of `twin_of` with search scratch of its own, so that two batches
    // can be in flight on the same shard (the pipelined search below).  Sharing is sound because rows, metadata and constants are
    // frozen while twins exist (DPH_NOT_TWINNED).
    dph_index* twin_of = nullptr;
    int n_twins = 0;                     // twins alive over this handle (it must outlive them and stay as it is)
    ~dph_index() { if (!twin_of) delete sh; }
};

static void build_lut(dph_shard* s) {
    // the reference's fp32 de-quantisation, two roundings: fl(fl(n)/scale) + offset  (embed_utils.py:148-149)
    double dm = 0.0;
    for (int n = -128; n < 128; ++n) {
        volatile float a = (float)n / s->scale;
        volatile float b = a + s->offset;
        s->lut_host[n + 128] = b;
        const double exact = (double)n / (double)s->scale + (double)s->offset;
        dm = fmax(dm, fabs((double)b - exact));
        s->doc_lut_host[n + 128] = (float)exact;
    }
    s->delta_max = dm;
}

// the rows, metadata and shard constants of an index that has twins (or is one) are shared and stay as they are
#define DPH_NOT_TWINNED(h, who) \
    do { if ((h) && ((h)->twin_of || (h)->n_twins > 0)) return fail(DPH_E_STATE, std::string(who) + ": not on an index that has twins or is one"); } while (0)

extern "C" {

int dph_abi_version(void) { return DPH_ABI_VERSION; }
const char* dph_last_error(void) { return g_err.c_str(); }
int dph_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int dph_index_create(int device, int64_t n_rows, int64_t id_base, dph_index** out) {
    if (!out || n_rows < 0) return fail(DPH_E_ARG, "dph_index_create: bad arguments");
    if (n_rows >= (int64_t)0xFFFFFFF0ll) return fail(DPH_E_ARG, "dph_index_create: shard limited to 2^32-16 rows");
    HIPCHK(hipSetDevice(device));
    dph_index* h = new dph_index();
    h->sh = new dph_shard();
    h->device = device;
    h->sh->n_rows = n_rows;
    h->sh->n_ids = n_rows;
    h->sh->id_base = id_base;
    h->sh->n_tiles = (n_rows + DPH_TILE_ROWS - 1) / DPH_TILE_ROWS;
    h->tune.grid = dph_scan_grid(device);
    const size_t bytes = (size_t)(h->sh->n_tiles > 0 ? h->sh->n_tiles : 1) * DPH_TILE_BYTES;
    hipError_t e = h->sh->db.alloc(bytes);
    if (e != hipSuccess) { delete h; return fail(DPH_E_NOMEM, std::string("hipMalloc shard: ") + hipGetErrorString(e)); }
    // zero the padding rows of the last tile (they are excluded from the candidates by row index as well)
    if (h->sh->n_tiles > 0) {
        const size_t used = (size_t)n_rows * DPH_DIM;
        if (bytes > used) (void)hipMemset(h->sh->db + used, 0, bytes - used);
    }
    build_lut(h->sh);
    if (h->sh->lut_dev.alloc(256) != hipSuccess ||
        h->sh->norm_dev.alloc(2) != hipSuccess ||
        h->sh->hist_dev.alloc(DPH_NORM_BINS) != hipSuccess ||
        h->sh->outliers.alloc(DPH_OUTLIER_MAX) != hipSuccess ||
        h->sh->mu_dev.alloc(DPH_DIM) != hipSuccess ||
        h->sh->colsum_dev.alloc(2 * DPH_DIM) != hipSuccess) {
        dph_index_destroy(h);
        return fail(DPH_E_NOMEM, "hipMalloc lut");
    }
    (void)hipMemset(h->sh->mu_dev, 0, DPH_DIM * sizeof(int));
    h->sh->aux_lay.q2max = 64;
    (void)hipMemcpy(h->sh->lut_dev, h->sh->lut_host, sizeof(h->sh->lut_host), hipMemcpyHostToDevice);
    *out = h;
    return DPH_OK;
}

int dph_index_destroy(dph_index* h) {
    if (!h) return DPH_OK;
    (void)hipSetDevice(h->device);
    if (!h->twin_of && h->n_twins > 0) return fail(DPH_E_STATE, "dph_index_destroy: destroy the twins of this index first");
    if (h->twin_of) h->twin_of->n_twins--;
    delete h;
    return DPH_OK;
}

int dph_index_create_twin(dph_index* src, dph_index** out) {
    if (!src || !out) return fail(DPH_E_ARG, "dph_index_create_twin: null");
    if (src->twin_of) return fail(DPH_E_ARG, "dph_index_create_twin: make twins of the index itself, not of a twin");
    if (!src->sh->finalized) return fail(DPH_E_STATE, "dph_index_create_twin: call dph_index_finalize first");
    if (src->sh->pq || src->sh->row_ids) return fail(DPH_E_STATE, "dph_index_create_twin: flat shards only (no PQ index, no list-major shard)");
    dph_index* t = new dph_index();      // the shard is shared, the search scratch is the twin's own (allocated by its first search)
    t->device = src->device;
    t->sh = src->sh;
    t->tune = src->tune;
    t->twin_of = src;
    src->n_twins++;
    *out = t;
    return DPH_OK;
}

int dph_index_set_codec(dph_index* h, float offset, float scale) {
    DPH_NOT_TWINNED(h, "dph_index_set_codec");
    if (!h || !(scale > 0.f)) return fail(DPH_E_ARG, "dph_index_set_codec: scale must be > 0");
    HIPCHK(hipSetDevice(h->device));
    h->sh->offset = offset; h->sh->scale = scale;
    build_lut(h->sh);
    HIPCHK(hipMemcpy(h->sh->lut_dev, h->sh->lut_host, sizeof(h->sh->lut_host), hipMemcpyHostToDevice));
    if (h->sh->doc_lut) HIPCHK(hipMemcpy(h->sh->doc_lut, h->sh->doc_lut_host, sizeof(h->sh->doc_lut_host), hipMemcpyHostToDevice));
    return DPH_OK;
}

// where dph_index_upload_rows(_async) writes: the shard's rows, or -- a PQ index with document rows attached -- that store
static int8_t* upload_target(dph_shard* s, int64_t* cap) {
    const bool doc = s->pq && s->doc_rows;
    *cap = doc ? s->n_doc_rows : s->n_rows;
    return doc ? s->doc_rows.p : s->db.p;
}
static void note_doc_rows(dph_shard* s, int64_t row0, int64_t n) {
    if (!(s->pq && s->doc_rows) || n <= 0) return;
    int64_t a = row0, b = row0 + n;
    auto it = s->doc_rows_have.upper_bound(a);
    if (it != s->doc_rows_have.begin() && std::prev(it)->second >= a) --it;
    while (it != s->doc_rows_have.end() && it->first <= b) {
        a = std::min(a, it->first); b = std::max(b, it->second);
        it = s->doc_rows_have.erase(it);
    }
    s->doc_rows_have[a] = b;
}

int dph_index_attach_doc_rows(dph_index* h, int64_t n_doc_rows) {
    DPH_NOT_TWINNED(h, "dph_index_attach_doc_rows");
    if (!h || n_doc_rows <= 0) return fail(DPH_E_ARG, "dph_index_attach_doc_rows: need a handle and n_doc_rows > 0");
    dph_shard* const s = h->sh;
    if (!s->pq) return fail(DPH_E_STATE, "dph_index_attach_doc_rows: not a PQ index (dph_index_create_pq)");
    if (s->doc_rows) return fail(DPH_E_STATE, "dph_index_attach_doc_rows: document rows are attached already");
    if (s->finalized) return fail(DPH_E_STATE, "dph_index_attach_doc_rows: attach before dph_index_finalize");
    HIPCHK(hipSetDevice(h->device));
    hipError_t e = s->doc_lut.alloc(256);
    if (e == hipSuccess) e = s->doc_rows.alloc((size_t)n_doc_rows * DPH_DIM);
    if (e != hipSuccess) {
        s->doc_rows.reset(); s->doc_lut.reset();
        return fail(DPH_E_NOMEM, std::string("dph_index_attach_doc_rows: hipMalloc: ") + hipGetErrorString(e));
    }
    HIPCHK(hipMemcpy(s->doc_lut, s->doc_lut_host, sizeof(s->doc_lut_host), hipMemcpyHostToDevice));
    s->n_doc_rows = n_doc_rows;
    s->doc_rows_have.clear();
    return DPH_OK;
}

int dph_index_upload_rows(dph_index* h, int64_t row0, int64_t n, const int8_t* host_rows) {
    DPH_NOT_TWINNED(h, "dph_index_upload_rows");
    int64_t cap = 0;
    int8_t* const dst = h ? upload_target(h->sh, &cap) : nullptr;
    if (!h || !host_rows || row0 < 0 || n < 0 || row0 + n > cap) return fail(DPH_E_ARG, "dph_index_upload_rows: range");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpy(dst + row0 * DPH_DIM, host_rows, (size_t)n * DPH_DIM, hipMemcpyHostToDevice));
    note_doc_rows(h->sh, row0, n);
    h->sh->finalized = false;
    return DPH_OK;
}

int dph_index_upload_rows_async(dph_index* h, int64_t row0, int64_t n, const int8_t* pinned_rows, void* stream) {
    DPH_NOT_TWINNED(h, "dph_index_upload_rows_async");
    int64_t cap = 0;
    int8_t* const dst = h ? upload_target(h->sh, &cap) : nullptr;
    if (!h || !pinned_rows || row0 < 0 || n < 0 || row0 + n > cap) return fail(DPH_E_ARG, "dph_index_upload_rows_async: range");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(dst + row0 * DPH_DIM, pinned_rows, (size_t)n * DPH_DIM, hipMemcpyHostToDevice, (hipStream_t)stream));
    note_doc_rows(h->sh, row0, n);
    h->sh->finalized = false;
    return DPH_OK;
}

int dph_host_alloc_pinned(size_t bytes, void** out) {
    if (!out) return fail(DPH_E_ARG, "dph_host_alloc_pinned: null");
    HIPCHK(hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
    return DPH_OK;
}
int dph_host_free_pinned(void* p) {
    if (p) HIPCHK(hipHostFree(p));
    return DPH_OK;
}
int dph_stream_synchronize(int device, void* stream) {
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    return DPH_OK;
}

int dph_index_fill_synthetic(dph_index* h, uint64_t seed, void* stream) {
    DPH_NOT_TWINNED(h, "dph_index_fill_synthetic");
    if (!h) return fail(DPH_E_ARG, "null handle");
    HIPCHK(hipSetDevice(h->device));
    if (h->sh->n_rows > 0) dph_launch_fill(h->sh->db, h->sh->n_rows, h->sh->id_base, seed, 0, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    h->sh->finalized = false;
    return DPH_OK;
}

int dph_index_fill_synthetic_kind(dph_index* h, uint64_t seed, int kind, void* stream) {
    DPH_NOT_TWINNED(h, "dph_index_fill_synthetic_kind");
    if (!h || kind < 0 || kind > 4)
        return fail(DPH_E_ARG, "dph_index_fill_synthetic_kind: kind is 0 (i.i.d.), 1 (mixture + outliers), 2 (document-ordered runs), 3 (mixture) or 4 (anisotropic)");
    HIPCHK(hipSetDevice(h->device));
    if (h->sh->n_rows > 0) dph_launch_fill(h->sh->db, h->sh->n_rows, h->sh->id_base, seed, kind, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    h->sh->finalized = false;
    return DPH_OK;
}

int dph_index_set_idx2id(dph_index* h, const int32_t* doc, const int32_t* word) {
    DPH_NOT_TWINNED(h, "dph_index_set_idx2id");
    if (!h || !doc || !word) return fail(DPH_E_ARG, "dph_index_set_idx2id: null");
    HIPCHK(hipSetDevice(h->device));
    // indexed by local id (= stored row on a flat shard)
    const size_t count = (size_t)(h->sh->n_ids > 0 ? h->sh->n_ids : 1);
    h->sh->row2doc.reset(); h->sh->row2word.reset();
    HIPCHK(h->sh->row2doc.alloc(count));
    HIPCHK(h->sh->row2word.alloc(count));
    HIPCHK(hipMemcpy(h->sh->row2doc, doc, (size_t)h->sh->n_ids * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->sh->row2word, word, (size_t)h->sh->n_ids * 4, hipMemcpyHostToDevice));
    h->sh->h_row2doc.assign(doc, doc + h->sh->n_ids);
    h->sh->h_row2word.assign(word, word + h->sh->n_ids);
    return DPH_OK;
}

int dph_index_set_f2o(dph_index* h, int64_t n_docs, const int32_t* doc_ids, const int64_t* f2o_off, const int32_t* f2o) {
    DPH_NOT_TWINNED(h, "dph_index_set_f2o");
    if (!h || n_docs < 0 || (n_docs > 0 && (!doc_ids || !f2o_off || !f2o))) return fail(DPH_E_ARG, "dph_index_set_f2o: null");
    for (int64_t i = 1; i < n_docs; ++i)
        if (doc_ids[i] <= doc_ids[i - 1]) return fail(DPH_E_ARG, "dph_index_set_f2o: doc_ids must be strictly ascending");
    HIPCHK(hipSetDevice(h->device));
    h->sh->doc_ids.reset(); h->sh->f2o_off.reset(); h->sh->f2o.reset(); h->sh->n_docs = 0;
    const int64_t total = n_docs > 0 ? f2o_off[n_docs] : 0;
    HIPCHK(h->sh->doc_ids.alloc((size_t)(n_docs > 0 ? n_docs : 1)));
    HIPCHK(h->sh->f2o_off.alloc((size_t)(n_docs + 1)));
    HIPCHK(h->sh->f2o.alloc((size_t)(total > 0 ? total : 1)));
    if (n_docs > 0) {
        HIPCHK(hipMemcpy(h->sh->doc_ids, doc_ids, (size_t)n_docs * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(h->sh->f2o_off, f2o_off, (size_t)(n_docs + 1) * 8, hipMemcpyHostToDevice));
        if (total > 0) HIPCHK(hipMemcpy(h->sh->f2o, f2o, (size_t)total * 4, hipMemcpyHostToDevice));
    } else {
        const int64_t zero = 0;
        HIPCHK(hipMemcpy(h->sh->f2o_off, &zero, 8, hipMemcpyHostToDevice));
    }
    h->sh->n_docs = n_docs;
    h->sh->f2o_total = total;
    if (h->sh->doc_rows) h->sh->finalized = false;      // the document rows are addressed through this table: finalize checks them against it
    return DPH_OK;
}

// ---- shard statistics: what the bounds of the search are made of ------------------------------------------------------
// Every bound (the low-digit bound of the filter, the score bound of the rows that were not re-scored) is a Cauchy-Schwarz
// bound around the per-dimension mean code mu of the stored rows.  dph_index_finalize measures, in three passes over the rows:
//   1. per-dimension sums -> mu_j (rounded mean), spread sd_j (plan_col_stats);
//   2. the squared centred norms || n - mu ||^2: maximum, histogram -> median, and the outlier cut (plan_norm_stats): ONE extreme row (a
//      saturated code vector) would loosen a shard-wide bound for every query, so the DPH_OUTLIER_MAX largest-norm rows are taken out of
//      it when that tightens it by more than 10 %: "outlier rows", scored exactly against every query (dph_outlier_kernel), never bounded;
//   3. whether the rows are ALIKE (choose_aux_layout); a shard whose rows are not gets AUX ROWS (dph_scan.hip "the aux k-step").
// The rules themselves stand in dph_plan.h; here the shard's state goes in and the plan comes back.
static plan_aux_facts aux_facts(const dph_shard* s) {
    return plan_aux_facts{s->n_rows, s->aux_mode, s->mu_host, s->sd_host, s->rmed, s->rmax_cut, s->rmax_all, s->n_out_found};
}
static void set_aux_plan(dph_shard* s, const plan_aux& a) {
    s->aux_lay = a.lay; s->aux_lay_forced = a.forced; s->norm_unit = a.norm_unit; s->n_out = a.n_out; s->rmax = a.rmax;
}
static plan_list_facts list_facts(const dph_shard* s) {
    return plan_list_facts{s->n_rows, s->n_tiles, s->nlist, s->lists_contiguous, s->max_list_tiles, s->total_segs};
}

static int build_aux_rows(dph_shard* s, hipStream_t st) {
    if (s->aux_lay.stride <= 0) return DPH_OK;
    const int64_t padded = s->n_tiles * DPH_TILE_ROWS;
    const size_t bytes = (size_t)padded * s->aux_lay.stride + 256;      // + the over-read of the last lanes (stride 4: 16-byte loads)
    if (bytes > s->aux.n) HIPCHK(s->aux.alloc(bytes));
    HIPCHK(hipMemsetAsync(s->aux, 0, s->aux.n, st));
    dph_launch_aux_build(s->db, s->n_rows, padded, s->row_ids, s->mu_dev, s->aux_lay, s->norm_unit, s->aux, st);
    HIPCHK(hipGetLastError());
    return DPH_OK;
}

int dph_index_finalize(dph_index* h, void* stream) {
    DPH_NOT_TWINNED(h, "dph_index_finalize");
    if (!h) return fail(DPH_E_ARG, "null handle");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    dph_shard* const s = h->sh;
    if (s->pq) {                         // a PQ index has no row statistics: its finalize builds the direct map
        if (s->doc_rows) {
            if (s->n_doc_rows != s->f2o_total)
                return fail(DPH_E_STATE, "dph_index_finalize: " + std::to_string(s->n_doc_rows) + " document rows attached, the f2o table (dph_index_set_f2o) counts " +
                                             std::to_string(s->f2o_total) + " words");
            if (s->doc_rows_have.size() != 1 || s->doc_rows_have.begin()->first != 0 || s->doc_rows_have.begin()->second != s->n_doc_rows)
                return fail(DPH_E_STATE, "dph_index_finalize: not every attached document row was uploaded (dph_index_upload_rows)");
        }
        const int rc = dph_pq_finalize(s->pq, st);
        if (rc) return rc;
        s->finalized = true;
        return DPH_OK;
    }
    // ---- 1. per-dimension mean codes
    int64_t n_real = s->row_ids ? s->n_ids : s->n_rows;
    std::vector<long long> sums(2 * DPH_DIM, 0);
    HIPCHK(hipMemsetAsync(s->colsum_dev, 0, 2 * DPH_DIM * sizeof(long long), st));
    if (s->n_rows > 0) dph_launch_colstats(s->db, s->n_rows, s->row_ids, s->colsum_dev, st);
    HIPCHK(hipMemcpyAsync(sums.data(), s->colsum_dev, 2 * DPH_DIM * sizeof(long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    plan_col_stats(sums.data(), n_real, s->mu_host, s->sd_host);
    HIPCHK(hipMemcpyAsync(s->mu_dev, s->mu_host, DPH_DIM * sizeof(int), hipMemcpyHostToDevice, st));
    // ---- 2. centred row norms
    HIPCHK(hipMemsetAsync(s->norm_dev, 0, 2 * sizeof(unsigned long long), st));
    HIPCHK(hipMemsetAsync(s->hist_dev, 0, DPH_NORM_BINS * sizeof(unsigned), st));
    if (s->n_rows > 0) dph_launch_rownorm(s->db, s->n_rows, s->row_ids, s->mu_dev, s->norm_dev, s->hist_dev, 0, nullptr, nullptr, 0, st);
    unsigned long long m = 0;
    std::vector<unsigned> hist(DPH_NORM_BINS);
    HIPCHK(hipMemcpyAsync(&m, s->norm_dev, sizeof(m), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hist.data(), s->hist_dev, DPH_NORM_BINS * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    s->rmax_all = sqrt((double)m);
    s->rmax = s->rmax_all;
    s->rmax_cut = s->rmax_all;
    s->n_out = 0;
    s->n_out_found = 0;
    const plan_norms nrm = plan_norm_stats(hist.data(), m);
    s->rmed = nrm.rmed;
    const unsigned long long cut2 = nrm.cut2;
    if (nrm.take_cut) {
        unsigned* cnt = (unsigned*)(s->norm_dev + 1);
        dph_launch_rownorm(s->db, s->n_rows, s->row_ids, s->mu_dev, nullptr, nullptr, cut2 - 1, s->outliers, cnt, DPH_OUTLIER_MAX, st);
        unsigned n_out = 0;
        HIPCHK(hipMemcpyAsync(&n_out, cnt, sizeof(n_out), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (n_out > 0 && n_out <= (unsigned)DPH_OUTLIER_MAX) {
            std::vector<unsigned> rows(n_out);
            HIPCHK(hipMemcpy(rows.data(), s->outliers, n_out * sizeof(unsigned), hipMemcpyDeviceToHost));
            std::sort(rows.begin(), rows.end());
            HIPCHK(hipMemcpy(s->outliers, rows.data(), n_out * sizeof(unsigned), hipMemcpyHostToDevice));
            s->n_out_found = (int)n_out;
            s->rmax_cut = sqrt((double)cut2);
        }
    }
    // ---- 3. aux rows: the layout is chosen unless a forced one still serves these rows (plan_aux_rows)
    set_aux_plan(s, plan_aux_rows(aux_facts(s), s->aux_lay, s->aux_lay_forced));
    const int rc = build_aux_rows(s, st);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(st));
    s->finalized = true;
    return DPH_OK;
}

// The digits of a query row depend on the aux layout (which dimensions have replica digits, the clamp of the low digit), and the
// ranks of a range-sharded job compare INTEGER scores (dph_search_sample_dev / dph_union_bounds_dev / dph_search_bounded_dev): every
// rank must cut its queries into the same digits.  A sharded caller therefore reads the layout of every finalized shard, agrees on
// one (densephrases_amd/dist.py: the widest stride, the replica table of the lowest rank that has one, the smallest clamp) and
// sets it everywhere; the aux rows are rebuilt to it (one pass over the rows).  out / in: [0] stride, [1] n_norm, [2] n_rep,
// [3] q2max, [4 .. 4 + DPH_AUX_REP_MAX) rep_dim.
int dph_index_get_aux_layout(dph_index* h, int32_t* out) {
    if (!h || !out) return fail(DPH_E_ARG, "dph_index_get_aux_layout: null");
    if (!h->sh->finalized) return fail(DPH_E_STATE, "dph_index_get_aux_layout: call dph_index_finalize first");
    const dph_shard* src = h->sh;
    plan_pack_layout(src->aux_lay, out);
    // no aux rows here, but another rank of the job may force some on this shard: report the clamp THIS shard's row norms would allow
    // with the fewest norm slots a layout has (4), so that the minimum over the ranks is one every rank can set
    if (src->aux_lay.stride <= 0) out[3] = plan_q2max(plan_norm_unit(src->rmax_all, 4));
    return DPH_OK;
}
int dph_index_set_aux_layout(dph_index* h, const int32_t* in) {
    DPH_NOT_TWINNED(h, "dph_index_set_aux_layout");
    if (!h || !in) return fail(DPH_E_ARG, "dph_index_set_aux_layout: null");
    if (h->sh->pq) return DPH_OK;        // a PQ index has no digits
    if (!h->sh->finalized) return fail(DPH_E_STATE, "dph_index_set_aux_layout: call dph_index_finalize first");
    plan_aux a{};
    a.forced = true;
    const int bad = plan_unpack_layout(in, &a.lay);
    if (bad == 1) return fail(DPH_E_ARG, "dph_index_set_aux_layout: not a layout dph_index_get_aux_layout returns");
    if (bad) return fail(DPH_E_ARG, "dph_index_set_aux_layout: replica dimension out of range");
    HIPCHK(hipSetDevice(h->device));
    derive_aux_units(aux_facts(h->sh), &a);
    set_aux_plan(h->sh, a);
    // the forced clamp must serve this shard's norm unit (see derive_aux_units)
    if (a.lay.stride > 0 && a.lay.q2max > plan_q2_limit(a.norm_unit))
        return fail(DPH_E_ARG, "dph_index_set_aux_layout: q2max too large for this shard's row norms (take the minimum over the ranks)");
    const int rc = build_aux_rows(h->sh, nullptr);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(nullptr));
    return DPH_OK;
}

int64_t dph_index_ntotal(const dph_index* h) { return h ? h->sh->n_ids : 0; }

int dph_index_set_row_ids(dph_index* h, const int64_t* row_ids, int64_t n_ids) {
    DPH_NOT_TWINNED(h, "dph_index_set_row_ids");
    if (!h || !row_ids || n_ids < 0 || n_ids > h->sh->n_rows) return fail(DPH_E_ARG, "dph_index_set_row_ids: bad arguments");
    std::vector<int32_t> inv((size_t)n_ids, -1);
    for (int64_t r = 0; r < h->sh->n_rows; ++r) {
        const int64_t id = row_ids[r];
        if (id < 0) continue;
        const int64_t l = id - h->sh->id_base;
        if (l < 0 || l >= n_ids || inv[(size_t)l] != -1) return fail(DPH_E_ARG, "dph_index_set_row_ids: ids must be a permutation of [id_base, id_base+n_ids)");
        inv[(size_t)l] = (int32_t)r;
    }
    for (int64_t l = 0; l < n_ids; ++l) if (inv[(size_t)l] < 0) return fail(DPH_E_ARG, "dph_index_set_row_ids: an id has no row");
    HIPCHK(hipSetDevice(h->device));
    h->sh->row_ids.reset(); h->sh->inv_row.reset(); h->sh->onesmask.reset();
    HIPCHK(h->sh->row_ids.alloc((size_t)(h->sh->n_tiles > 0 ? h->sh->n_tiles : 1) * DPH_TILE_ROWS));
    HIPCHK(hipMemset(h->sh->row_ids, 0xFF, (size_t)(h->sh->n_tiles > 0 ? h->sh->n_tiles : 1) * DPH_TILE_ROWS * 8));   // padding = -1
    HIPCHK(hipMemcpy(h->sh->row_ids, row_ids, (size_t)h->sh->n_rows * 8, hipMemcpyHostToDevice));
    HIPCHK(h->sh->inv_row.alloc((size_t)(n_ids > 0 ? n_ids : 1)));
    HIPCHK(hipMemcpy(h->sh->inv_row, inv.data(), (size_t)n_ids * 4, hipMemcpyHostToDevice));
    HIPCHK(h->sh->onesmask.alloc((size_t)(h->sh->n_tiles > 0 ? h->sh->n_tiles : 1) * 8));
    HIPCHK(hipMemset(h->sh->onesmask, 0xFF, (size_t)(h->sh->n_tiles > 0 ? h->sh->n_tiles : 1) * 32));
    h->sh->h_inv.swap(inv);
    h->sh->n_ids = n_ids;
    h->sh->finalized = false;
    return DPH_OK;
}

int dph_index_set_id_groups(dph_index* h, int n_groups, const int64_t* id_offsets, const int64_t* row_starts) {
    DPH_NOT_TWINNED(h, "dph_index_set_id_groups");
    if (!h || n_groups < 0 || (n_groups > 0 && (!id_offsets || !row_starts))) return fail(DPH_E_ARG, "dph_index_set_id_groups: bad arguments");
    if (h->sh->row_ids) return fail(DPH_E_STATE, "dph_index_set_id_groups: not on a list-major shard (its row_ids already carry the ids)");
    if (n_groups > 0) {
        if (row_starts[0] != 0 || row_starts[n_groups] != (h->sh->pq ? h->sh->n_ids : h->sh->n_rows)) return fail(DPH_E_ARG, "dph_index_set_id_groups: row_starts must run from 0 to n_rows");
        for (int g = 0; g < n_groups; ++g) {
            const int64_t len = row_starts[g + 1] - row_starts[g];
            if (len < 0 || id_offsets[g] < 0) return fail(DPH_E_ARG, "dph_index_set_id_groups: negative group");
            if (g + 1 < n_groups && id_offsets[g] + len > id_offsets[g + 1]) return fail(DPH_E_ARG, "dph_index_set_id_groups: id ranges must ascend without overlap");
        }
    }
    HIPCHK(hipSetDevice(h->device));
    h->sh->id_offsets.reset(); h->sh->row_starts.reset();
    h->sh->h_id_offsets.assign(id_offsets, id_offsets + n_groups);
    h->sh->h_row_starts.assign(row_starts, row_starts + (n_groups > 0 ? n_groups + 1 : 0));
    if (n_groups > 0) {
        HIPCHK(h->sh->id_offsets.alloc((size_t)n_groups));
        HIPCHK(h->sh->row_starts.alloc((size_t)(n_groups + 1)));
        HIPCHK(hipMemcpy(h->sh->id_offsets, id_offsets, (size_t)n_groups * 8, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(h->sh->row_starts, row_starts, (size_t)(n_groups + 1) * 8, hipMemcpyHostToDevice));
    }
    return DPH_OK;
}

// host twin of dph_local_of_id (flat / grouped shards: the stored row; list-major shards: the local id)
static int64_t host_local_of_id(const dph_shard* s, int64_t id) {
    const int ng = (int)s->h_id_offsets.size();
    if (ng == 0) { const int64_t l = id - s->id_base; return (l < 0 || l >= s->n_ids) ? -1 : l; }
    if (id < s->h_id_offsets[0]) return -1;
    int g = (int)(std::upper_bound(s->h_id_offsets.begin(), s->h_id_offsets.end(), id) - s->h_id_offsets.begin()) - 1;
    const int64_t r = id - s->h_id_offsets[(size_t)g];
    return r < s->h_row_starts[(size_t)g + 1] - s->h_row_starts[(size_t)g] ? s->h_row_starts[(size_t)g] + r : -1;
}

int dph_index_set_ivf(dph_index* h, int nlist, const float* centroids, const int32_t* tile_list) {
    DPH_NOT_TWINNED(h, "dph_index_set_ivf");
    if (!h || nlist <= 0 || nlist > (1 << 20) || !centroids || !tile_list) return fail(DPH_E_ARG, "dph_index_set_ivf: bad arguments");
    if (!h->sh->row_ids) return fail(DPH_E_STATE, "dph_index_set_ivf: call dph_index_set_row_ids first (list-major shard)");
    for (int64_t t = 0; t < h->sh->n_tiles; ++t)
        if (tile_list[t] < 0 || tile_list[t] >= nlist) return fail(DPH_E_ARG, "dph_index_set_ivf: tile_list out of range");
    HIPCHK(hipSetDevice(h->device));
    h->sh->centroids.reset(); h->sh->tile_list.reset(); h->sh->list_tile0.reset();
    h->sc.ivf = dph_ivf_pass(); h->sc.uq = dph_unit_queue();
    // the unit scan needs every list to be one contiguous run of tiles (what ivf.build_list_major writes)
    std::vector<int> tile0;
    const plan_list_facts geo = plan_list_geometry(tile_list, h->sh->n_rows, h->sh->n_tiles, nlist, tile0);
    h->sh->lists_contiguous = geo.lists_contiguous; h->sh->max_list_tiles = geo.max_list_tiles; h->sh->total_segs = geo.total_segs;
    double cmax = 0.0;
    for (int l = 0; l < nlist; ++l) {
        double a = 0.0;
        for (int j = 0; j < DPH_DIM; ++j) a += (double)centroids[(size_t)l * DPH_DIM + j] * centroids[(size_t)l * DPH_DIM + j];
        cmax = fmax(cmax, a);
    }
    h->sh->cnorm_max = sqrt(cmax);
    h->sc.ivf.coarse_rows = h->sh->lists_contiguous ? DPH_PASS_MAX : DPH_QROWS * DPH_MAX_QB;
    HIPCHK(h->sc.ivf.coarse_scores.alloc((size_t)h->sc.ivf.coarse_rows * nlist));
    if (h->sh->lists_contiguous) {
        HIPCHK(h->sh->list_tile0.alloc((size_t)nlist + 1));
        HIPCHK(hipMemcpy(h->sh->list_tile0, tile0.data(), ((size_t)nlist + 1) * 4, hipMemcpyHostToDevice));
        HIPCHK(h->sc.ivf.listmask_u.alloc((size_t)nlist * DPH_UNIT_WORDS));
        HIPCHK(h->sc.ivf.unit_offsets.alloc((size_t)nlist));
        HIPCHK(h->sc.ivf.unit_cnt.alloc(1));
    }
    HIPCHK(h->sh->centroids.alloc((size_t)nlist * DPH_DIM));
    HIPCHK(hipMemcpy(h->sh->centroids, centroids, (size_t)nlist * DPH_DIM * 4, hipMemcpyHostToDevice));
    HIPCHK(h->sh->tile_list.alloc((size_t)(h->sh->n_tiles > 0 ? h->sh->n_tiles : 1)));
    HIPCHK(hipMemcpy(h->sh->tile_list, tile_list, (size_t)h->sh->n_tiles * 4, hipMemcpyHostToDevice));
    HIPCHK(h->sc.ivf.listmask.alloc((size_t)nlist * 8));
    HIPCHK(h->sc.ivf.tilemask.alloc((size_t)(h->sh->n_tiles > 0 ? h->sh->n_tiles : 1) * 8));
    h->sh->nlist = nlist;
    return DPH_OK;
}
// A flat shard resident in HBM -> list-major shard + IVF data, on the device (dph_build.hip): the rows are permuted into a
// second buffer (the dump is in HBM twice for the duration: 2 x 131 GB of the 288), ids stay what they were.
int dph_index_make_list_major(dph_index* h, const int32_t* assign_dev, int nlist, const float* centroids, void* stream) {
    DPH_NOT_TWINNED(h, "dph_index_make_list_major");
    if (!h || !assign_dev || !centroids || nlist <= 0 || nlist > (1 << 20)) return fail(DPH_E_ARG, "dph_index_make_list_major: bad arguments");
    if (h->sh->row_ids) return fail(DPH_E_STATE, "dph_index_make_list_major: the shard is list-major already");
    if (!h->sh->h_id_offsets.empty()) return fail(DPH_E_STATE, "dph_index_make_list_major: not on a shard merged from several sub-indexes");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = h->sh->n_rows;
    std::vector<int64_t> src_start((size_t)nlist + 1, 0);
    dev_buf<uint64_t> keys;              // (allocated by the sort, owned here)
    const int src_rc = dph_list_major_sort(assign_dev, n, nlist, &keys.p, src_start.data(), st);
    if (src_rc == 2) return fail(DPH_E_ARG, "dph_index_make_list_major: a list number is out of range");
    if (src_rc != 0) return fail(DPH_E_NOMEM, "dph_index_make_list_major: sort scratch");
    // every list padded to whole tiles; the tile -> list table the scans read
    std::vector<int64_t> dst_start((size_t)nlist, 0);
    int64_t n_store = 0;
    for (int l = 0; l < nlist; ++l) {
        dst_start[(size_t)l] = n_store;
        const int64_t cnt = src_start[(size_t)l + 1] - src_start[(size_t)l];
        n_store += (cnt + DPH_TILE_ROWS - 1) / DPH_TILE_ROWS * DPH_TILE_ROWS;
    }
    if (n_store >= (int64_t)0xFFFFFFF0ll) return fail(DPH_E_ARG, "dph_index_make_list_major: padded shard exceeds 2^32-16 rows");
    const int64_t n_tiles = n_store / DPH_TILE_ROWS;
    std::vector<int32_t> tile_list((size_t)n_tiles);
    for (int l = 0; l < nlist; ++l) {
        const int64_t t0 = dst_start[(size_t)l] / DPH_TILE_ROWS;
        const int64_t t1 = (l + 1 < nlist ? dst_start[(size_t)l + 1] : n_store) / DPH_TILE_ROWS;
        for (int64_t t = t0; t < t1; ++t) tile_list[(size_t)t] = l;
    }
    dev_buf<int8_t> db_new; dev_buf<int64_t> row_ids; dev_buf<int32_t> inv_row; dev_buf<unsigned> ones;
    dev_buf<int64_t> src_dev, dst_dev;
    const size_t tiles_alloc = (size_t)(n_tiles > 0 ? n_tiles : 1);
    if (db_new.alloc(tiles_alloc * DPH_TILE_BYTES) != hipSuccess || row_ids.alloc(tiles_alloc * DPH_TILE_ROWS) != hipSuccess ||
        inv_row.alloc((size_t)(n > 0 ? n : 1)) != hipSuccess || ones.alloc(tiles_alloc * 8) != hipSuccess ||
        src_dev.alloc((size_t)nlist + 1) != hipSuccess || dst_dev.alloc((size_t)nlist) != hipSuccess)
        return fail(DPH_E_NOMEM, "dph_index_make_list_major: the permuted copy does not fit next to the shard");
    (void)hipMemsetAsync(db_new, 0, tiles_alloc * DPH_TILE_BYTES, st);                    // padding rows are zero
    (void)hipMemsetAsync(row_ids, 0xFF, tiles_alloc * DPH_TILE_ROWS * 8, st);             // ... and carry id -1
    (void)hipMemsetAsync(ones, 0xFF, tiles_alloc * 32, st);
    (void)hipMemsetAsync(inv_row, 0xFF, (size_t)(n > 0 ? n : 1) * 4, st);                 // every id must get a row: checked below
    (void)hipMemcpyAsync(src_dev, src_start.data(), ((size_t)nlist + 1) * 8, hipMemcpyHostToDevice, st);
    (void)hipMemcpyAsync(dst_dev, dst_start.data(), (size_t)nlist * 8, hipMemcpyHostToDevice, st);
    dph_launch_list_major_gather(h->sh->db, keys, n, src_dev, dst_dev, h->sh->id_base, db_new, row_ids, inv_row, st);
    std::vector<int32_t> inv((size_t)n);
    hipError_t e = hipMemcpyAsync(inv.data(), inv_row, (size_t)n * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return fail(DPH_E_HIP, std::string("dph_index_make_list_major: ") + hipGetErrorString(e));
    for (int64_t r = 0; r < n; ++r)
        if (inv[(size_t)r] < 0) return fail(DPH_E_HIP, "dph_index_make_list_major: the gather left row " + std::to_string(r) + " without a place");
    keys.reset(); src_dev.reset(); dst_dev.reset();
    h->sh->db = std::move(db_new); h->sh->row_ids = std::move(row_ids); h->sh->inv_row = std::move(inv_row); h->sh->onesmask = std::move(ones);
    h->sh->h_inv.swap(inv);
    h->sh->n_ids = n;
    h->sh->n_rows = n_store;
    h->sh->n_tiles = n_tiles;
    h->sh->finalized = false;
    return dph_index_set_ivf(h, nlist, centroids, tile_list.data());
}

int dph_index_rehome_rows(dph_index* h, void* stream) {
    DPH_NOT_TWINNED(h, "dph_index_rehome_rows");
    if (!h) return fail(DPH_E_ARG, "null handle");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const size_t bytes = (size_t)(h->sh->n_tiles > 0 ? h->sh->n_tiles : 1) * DPH_TILE_BYTES;
    dev_buf<int8_t> fresh;
    if (fresh.alloc(bytes) != hipSuccess) return fail(DPH_E_NOMEM, "dph_index_rehome_rows: no room for a second copy of the rows");
    hipError_t e = hipMemcpyAsync(fresh, h->sh->db, bytes, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(DPH_E_HIP, std::string("dph_index_rehome_rows: ") + hipGetErrorString(e));
    h->sh->db = std::move(fresh);
    return DPH_OK;
}

// ---- the reference's own index: IndexPreTransform(OPQMatrix) + IndexIVFPQ (index.py:30-33; densephrases_amd/faiss_io.py reads the file)
int dph_index_create_pq(int device, int64_t ntotal, int nlist, int M, dph_index** out) {
    if (!out || ntotal < 0) return fail(DPH_E_ARG, "dph_index_create_pq: bad arguments");
    dph_index* h = nullptr;
    int rc = dph_index_create(device, 0, 0, &h);
    if (rc) return rc;
    rc = dph_pq_alloc(&h->sh->pq, device, ntotal, nlist, M);
    if (rc) { dph_index_destroy(h); return fail(rc, std::string("dph_index_create_pq: ") + dph_last_error()); }
    h->sh->n_ids = ntotal;                   // idx2id / id groups are indexed by local id
    h->tune.default_nprobe = 256;             // index.py:53,62
    *out = h;
    return DPH_OK;
}
int dph_index_set_pq(dph_index* h, const float* A, const float* b, const float* centroids, const float* pq_centroids, int by_residual) {
    DPH_NOT_TWINNED(h, "dph_index_set_pq");
    if (!h || !h->sh->pq) return fail(DPH_E_STATE, "dph_index_set_pq: not a PQ index (dph_index_create_pq)");
    const int rc = dph_pq_set_params(h->sh->pq, A, b, centroids, pq_centroids, by_residual);
    h->sh->finalized = false;
    return rc;
}
int dph_index_set_pq_list_sizes(dph_index* h, const int64_t* sizes) {
    DPH_NOT_TWINNED(h, "dph_index_set_pq_list_sizes");
    if (!h || !h->sh->pq) return fail(DPH_E_STATE, "dph_index_set_pq_list_sizes: not a PQ index");
    const int rc = dph_pq_set_list_sizes(h->sh->pq, sizes);
    h->sh->finalized = false;
    return rc;
}
int dph_index_upload_pq_codes(dph_index* h, int64_t pos0, int64_t n, const uint8_t* codes, const int64_t* ids) {
    DPH_NOT_TWINNED(h, "dph_index_upload_pq_codes");
    if (!h || !h->sh->pq) return fail(DPH_E_STATE, "dph_index_upload_pq_codes: not a PQ index");
    const int rc = dph_pq_upload(h->sh->pq, pos0, n, codes, ids);
    h->sh->finalized = false;
    return rc;
}
// the add step: index.add_with_ids behind a trained index (build_phrase_index.py:145-153; add_to_index :156-279 feeds it the dump)
int dph_pq_encode_dev(dph_index* h, const float* x_dev, int64_t n, int32_t* list_dev, uint8_t* codes_dev, void* stream) {
    if (!h || !x_dev || n <= 0 || !list_dev || !codes_dev) return fail(DPH_E_ARG, "dph_pq_encode_dev: bad arguments");
    if (!h->sh->pq) return fail(DPH_E_STATE, "dph_pq_encode_dev: not a PQ index (dph_index_create_pq)");
    return dph_pq_encode(h->sh->pq, x_dev, n, list_dev, codes_dev, (hipStream_t)stream);
}
int dph_index_fill_pq_dev(dph_index* h, int64_t n, const int32_t* list_dev, const uint8_t* codes_dev, const int64_t* ids_dev, void* stream) {
    DPH_NOT_TWINNED(h, "dph_index_fill_pq_dev");
    if (!h || n <= 0 || !list_dev || !codes_dev || !ids_dev) return fail(DPH_E_ARG, "dph_index_fill_pq_dev: bad arguments");
    if (!h->sh->pq) return fail(DPH_E_STATE, "dph_index_fill_pq_dev: not a PQ index");
    h->sh->finalized = false;
    return dph_pq_fill(h->sh->pq, n, list_dev, codes_dev, ids_dev, (hipStream_t)stream);
}
int dph_index_get_pq_list_sizes(dph_index* h, int64_t* sizes) {
    if (!h || !sizes) return fail(DPH_E_ARG, "dph_index_get_pq_list_sizes: bad arguments");
    if (!h->sh->pq) return fail(DPH_E_STATE, "dph_index_get_pq_list_sizes: not a PQ index");
    return dph_pq_get_list_sizes(h->sh->pq, sizes);
}
int dph_index_download_pq_codes(dph_index* h, int64_t pos0, int64_t n, uint8_t* codes, int64_t* ids) {
    if (!h || n <= 0 || pos0 < 0 || !codes || !ids) return fail(DPH_E_ARG, "dph_index_download_pq_codes: bad arguments");
    if (!h->sh->pq) return fail(DPH_E_STATE, "dph_index_download_pq_codes: not a PQ index");
    return dph_pq_download(h->sh->pq, pos0, n, codes, ids);
}
int dph_index_get_transform(dph_index* h, float* A_out) {
    if (!h || !A_out) return fail(DPH_E_ARG, "dph_index_get_transform: null");
    if (h->sh->pq) { memcpy(A_out, dph_pq_A_host(h->sh->pq), (size_t)DPH_DIM * DPH_DIM * 4); return DPH_OK; }
    memset(A_out, 0, (size_t)DPH_DIM * DPH_DIM * 4);
    for (int i = 0; i < DPH_DIM; ++i) A_out[(size_t)i * DPH_DIM + i] = 1.f;
    return DPH_OK;
}

int dph_index_dim(const dph_index* h) { (void)h; return DPH_DIM; }
int dph_index_device(const dph_index* h) { return h ? h->device : -1; }
void* dph_index_rows_dev(dph_index* h) { if (h) h->sh->finalized = false; return h ? h->sh->db : nullptr; }

int dph_index_set_tuning(dph_index* h, const char* key, const int32_t* values, int n_values) {
    if (!h || !key || n_values < 0 || (n_values > 0 && !values)) return fail(DPH_E_ARG, "dph_index_set_tuning: bad arguments");
    const std::string k(key);
    if (h->twin_of && (k == "nprobe" || k == "ivf_units" || k == "ivf_spread" || k == "coarse_filter" || k == "coarse_teams"))
        return fail(DPH_E_STATE, "dph_index_set_tuning: " + k + ": not on a twin (flat shards only; set it on the index itself)");
    auto one = [&](int lo, int hi, int* dst) {
        if (n_values != 1 || values[0] < lo || values[0] > hi) return fail(DPH_E_ARG, "dph_index_set_tuning: " + k + ": value out of range");
        *dst = values[0];
        return DPH_OK;
    };
    if (k == "ladder") {                 // explicit pre-pass strides, coarse -> fine; {0} = no pre-pass; empty = default
        for (int i = 0; i < n_values; ++i) if (values[i] < 0) return fail(DPH_E_ARG, "dph_index_set_tuning: ladder strides must be >= 0");
        h->tune.ladder.assign(values, values + n_values);
        return DPH_OK;
    }
    if (k == "fine_stride") return one(0, 1 << 20, &h->tune.fine_stride);
    if (k == "sample_kp") return one(1, 1024, &h->tune.sample_kp);
    if (k == "max_qb") return one(1, DPH_MAX_QB, &h->tune.max_qb);
    if (k == "nprobe") return one(0, 1 << 20, &h->tune.default_nprobe);
    if (k == "ivf_units") return one(-1, 1, &h->tune.ivf_units);
    if (k == "ivf_spread") return one(0, 1, &h->tune.ivf_spread);
    if (k == "scan_seg") return one(1, 1 << 16, &h->tune.seg_tiles);
    if (k == "ladder_fuse") return one(0, 1, &h->tune.ladder_fuse);
    if (k == "coarse_teams") {           // PQ index, filter scan: passes of more than 128 rows as ONE launch of workgroup teams (default 1)
        if (!h->sh->pq) return fail(DPH_E_STATE, "coarse_teams: not a PQ index");
        if (n_values != 1 || values[0] < 0 || values[0] > 1) return fail(DPH_E_ARG, "coarse_teams: 0 or 1");
        dph_pq_set_coarse_teams(h->sh->pq, values[0]);
        return DPH_OK;
    }
    if (k == "coarse_filter") {          // PQ index: 1 = the one-product filter scan in front of the coarse quantizer's chain (default), 0 = the bf16x3 chain alone
        if (!h->sh->pq) return fail(DPH_E_STATE, "coarse_filter: not a PQ index");
        // (5: how the filter scan was selected while the GEMM forms 1 .. 4 existed; a request for one of those fails rather than be served by the scan)
        if (n_values != 1 || (values[0] != 0 && values[0] != 1 && values[0] != 5))
            return fail(DPH_E_ARG, "coarse_filter: 0 (the chain alone), 1 (the filter scan in front of it) or 5 (the old spelling of 1)");
        dph_pq_set_coarse_filter(h->sh->pq, values[0]);
        return DPH_OK;
    }
    if (k == "retry_chain") return one(0, 1, &h->tune.retry_chain);
    if (k == "aux") {                    // aux rows: -1 = dph_index_finalize decides (default), 0 = never, 4 = norm codes, 32 = norm codes + rogue replicas
        DPH_NOT_TWINNED(h, "dph_index_set_tuning(aux)");
        if (h->sh->pq) return fail(DPH_E_STATE, "aux: not on a PQ index");
        if (n_values != 1 || (values[0] != -1 && values[0] != 0 && values[0] != 4 && values[0] != 16 && values[0] != 32)) return fail(DPH_E_ARG, "aux: -1, 0, 4, 16 or 32");
        h->sh->aux_mode = values[0];
        h->sh->aux_lay_forced = false;
        if (h->sh->finalized) {              // the statistics stand: only the layout and the aux rows follow
            HIPCHK(hipSetDevice(h->device));
            set_aux_plan(h->sh, plan_aux_rows(aux_facts(h->sh), h->sh->aux_lay, false));
            const int rc = build_aux_rows(h->sh, nullptr);
            if (rc) return rc;
            HIPCHK(hipStreamSynchronize(nullptr));
        }
        return DPH_OK;
    }
    if (k == "side_grid") return one(0, 256, &h->tune.side_grid);
    if (k == "scan_grid") {              // persistent scan workgroups (one per CU): fewer than the CU count leaves CUs to other streams
        const int cus = dph_scan_grid(h->device);
        if (n_values != 1 || values[0] < 0 || values[0] > cus) return fail(DPH_E_ARG, "scan_grid: 0 (= the CU count) .. CU count");
        if (h->sc.wave_counts) return fail(DPH_E_STATE, "scan_grid: set it before the first search (scratch is sized by it)");
        h->tune.grid = values[0] ? values[0] : cus;
        return DPH_OK;
    }
    if (k == "scan_sched") {             // one value: both kernels; two: the 128-row and the 256-row kernel
        if (n_values < 1 || n_values > 2) return fail(DPH_E_ARG, "scan_sched: one or two values");
        for (int i = 0; i < n_values; ++i) if (values[i] < 0 || values[i] > 2) return fail(DPH_E_ARG, "scan_sched: 0, 1 or 2");
        h->tune.scan_sched[0] = values[0];
        h->tune.scan_sched[1] = values[n_values - 1];
        return DPH_OK;
    }
    return fail(DPH_E_ARG, "dph_index_set_tuning: unknown key " + k);
}

// ------------------------------------------------------------------------------------------ search driver
static int alloc_qimg(dph_scratch::qimg& q, int64_t padded, bool with_x) {
    q = dph_scratch::qimg();
    if (with_x) HIPCHK(q.x.alloc((size_t)padded * DPH_DIM));
    HIPCHK(q.frag.alloc((size_t)(padded / DPH_QGROUP) * DPH_QGROUP_FRAG_BYTES));
    HIPCHK(q.q1.alloc((size_t)padded * DPH_DIM));
    HIPCHK(q.q2.alloc((size_t)padded * DPH_DIM));
    HIPCHK(q.qinfo.alloc((size_t)padded));
    HIPCHK(q.lmax.alloc((size_t)padded));
    HIPCHK(q.qaux.alloc((size_t)padded * DPH_AUX_SLOTS));
    HIPCHK(hipMemset(q.qaux, 0, (size_t)padded * DPH_AUX_SLOTS));
    HIPCHK(q.nf.alloc((size_t)padded));
    HIPCHK(hipMemset(q.nf, 0, (size_t)padded * 4));
    return DPH_OK;
}

static int ensure_scratch(dph_index* h, int64_t n, int k_host) {
    // padded to whole passes of the widest kernel, plus one pass of slack for the quantiser's padding groups
    const int64_t pass = DPH_QROWS * DPH_MAX_QB;
    const int64_t padded = (n + pass - 1) / pass * pass;
    if (padded > h->sc.cap_rows) {
        h->sc.cap_rows = 0;              // (a growth that fails half-way leaves no capacity behind: the next call starts over)
        int rc = alloc_qimg(h->sc.q_main, padded, true);
        if (rc) return rc;
        rc = alloc_qimg(h->sc.q_retry, padded, true);
        if (rc) return rc;
        h->sc.D_dev.reset(); h->sc.I_dev.reset();       // sized by rows x k: allocated again below, when a host entry point asks
        HIPCHK(h->sc.status_dev.alloc((size_t)padded));
        HIPCHK(h->sc.ik_dev.alloc((size_t)padded));
        HIPCHK(h->sc.fail_dev.alloc((size_t)padded));
        HIPCHK(h->sc.fail2_dev.alloc((size_t)padded));
        HIPCHK(h->sc.retry_rows.alloc((size_t)padded));
        HIPCHK(h->sc.exact_rows.alloc((size_t)padded));
        HIPCHK(h->sc.retry_tau.alloc((size_t)padded));
        h->sc.cap_rows = padded;
        h->sc.cap_k = 0;
    }
    if (k_host > h->sc.cap_k) {
        HIPCHK(h->sc.D_dev.alloc((size_t)h->sc.cap_rows * k_host));
        HIPCHK(h->sc.I_dev.alloc((size_t)h->sc.cap_rows * k_host));
        h->sc.cap_k = k_host;
    }
    if (!h->sc.exact_x) {                // (the last of the block: a call that failed half-way allocates it again)
        HIPCHK(h->sc.pairs.alloc((size_t)DPH_POOL_CHUNKS * DPH_CHUNK_PAIRS));
        HIPCHK(h->sc.chunk_fill.alloc((size_t)DPH_POOL_CHUNKS));
        // two images: [0] the passes of the first attempt (what dph_scan_counters reports), [1] the retry passes
        HIPCHK(h->sc.wave_counts.alloc((size_t)2 * h->tune.grid * 4 * 2));
        HIPCHK(h->sc.buckets.alloc((size_t)DPH_PASS_MAX * DPH_BUCKET_CAP));
        HIPCHK(h->sc.pass_cnt.alloc(1));
        HIPCHK(hipMemset(h->sc.pass_cnt, 0, sizeof(dph_pass_counters)));
        HIPCHK(h->sc.tau_dev.alloc((size_t)2 * DPH_PASS_MAX));
        HIPCHK(h->sc.counters.alloc(1));
        HIPCHK(hipMemset(h->sc.counters, 0, sizeof(dph_search_counters)));
        HIPCHK(h->sc.exact_x.alloc((size_t)DPH_EXACT_ROWS_DEV * DPH_DIM));
    }
    if (!h->sc.exact_scratch) {
        // DPH_EXACT_HITS boundary hits per row the on-device fp64 fallback serves -- never more than the shard has rows (a twin, or a
        // small shard, does not need the 512 MiB the full size takes)
        const size_t hits = (size_t)std::max<int64_t>(1024, std::min<int64_t>((int64_t)DPH_EXACT_HITS, h->sh->n_rows + 64));
        const size_t want = (size_t)DPH_EXACT_HEAD + (size_t)DPH_EXACT_ROWS_DEV * hits * 16;
        HIPCHK(h->sc.exact_scratch.alloc(want));
    }
    return DPH_OK;
}

static plan_ladder_facts ladder_facts(const dph_index* h) {
    return plan_ladder_facts{h->sh->n_tiles, h->sh->n_rows, h->tune.grid, h->tune.fine_stride, h->tune.ladder.data(), (int)h->tune.ladder.size()};
}
// unit scan of a list-major shard, or the masked scan (dph_plan.h: use_units)
static bool use_units(const dph_index* h, int nprobe) { return use_units(list_facts(h->sh), h->sh->row_ids != nullptr, h->tune.ivf_units, nprobe); }

static int ensure_units(dph_index* h, int nprobe) {
    const plan_unit_caps c = plan_unit_queue(list_facts(h->sh), nprobe);
    if (c.chunk_cap <= h->sc.uq.chunk_cap && c.unit_cap <= h->sc.uq.unit_cap) return DPH_OK;
    h->sc.uq = dph_unit_queue();
    if (c.too_large) return fail(DPH_E_ARG, "unit scan: work queue too large for this nprobe");
    HIPCHK(h->sc.uq.slot_q.alloc((size_t)c.chunk_cap * DPH_UNIT_SLOTS));
    HIPCHK(h->sc.uq.unit_recs.alloc((size_t)c.unit_cap));
    HIPCHK(h->sc.uq.unit_list_recs.alloc((size_t)c.chunk_cap));
    HIPCHK(h->sc.uq.unit_frags.alloc((size_t)c.chunk_cap * 4 * DPH_QGROUP_FRAG_BYTES));
    h->sc.uq.chunk_cap = (int)c.chunk_cap; h->sc.uq.unit_cap = (int)c.unit_cap;
    return DPH_OK;
}

// clean = true: the rows are also written to q.x with non-finite rows replaced by their stand-in, q.nf flags them
static void quantize(dph_index* h, dph_scratch::qimg& q, const float* x, int64_t n, const int* gate, hipStream_t st, bool clean = false) {
    dph_launch_quantize(x, n, gate, q.frag, q.q1, q.q2, q.qinfo, h->sh->rmax, q.lmax, q.qaux, h->sh->mu_dev, h->sh->aux_lay, h->sh->norm_unit, st,
                        clean ? q.x : nullptr, clean ? q.nf : nullptr);
}

static dph_idmap make_idmap(const dph_shard* s) {
    dph_idmap m{};
    m.id_offsets = s->id_offsets; m.row_starts = s->row_starts; m.n_groups = (int)s->h_id_offsets.size();
    m.id_base = s->id_base; m.n_ids = s->n_ids;
    return m;
}

// what a window re-score launch is asked for (dph_rescore_dev): the caller's arrays and the shard's idx2id / f2o metadata
static dph_window_args make_window_args(const dph_index* h, int direction, const float* qhalf, int64_t n_q, int k, int L, const int64_t* ids,
                                        const int32_t* doc, const int32_t* word, const float* first, int32_t* pred_word, double* best,
                                        int32_t* argslot, float* vecs) {
    const dph_shard* s = h->sh;
    dph_window_args a{};
    a.direction = direction; a.idmap = make_idmap(s); a.qhalf = qhalf; a.n_cand = n_q * k; a.k = k; a.L = L;
    a.ids = ids; a.doc_in = doc; a.word_in = word; a.first = first;
    a.row2doc = s->row2doc; a.row2word = s->row2word; a.doc_ids = s->doc_ids; a.n_docs = s->n_docs; a.f2o_off = s->f2o_off; a.f2o = s->f2o;
    a.pred_word = pred_word; a.best = best; a.argslot = argslot; a.vecs = vecs;
    return a;
}

static dph_pass make_pass(dph_index* h, const dph_scratch::qimg& q, const float* x, int q0, int n_q, int qb) {
    dph_pass p{};
    p.db = h->sh->db; p.n_rows = h->sh->n_rows; p.row_ids = h->sh->row_ids;
    p.idmap = make_idmap(h->sh);
    p.grid = h->tune.grid;
    p.qb = qb; p.q0 = q0; p.n_q = n_q; p.gate = nullptr; p.gate_base = 0;
    p.x = x; p.qfrag_hi = q.frag; p.q1 = q.q1; p.q2 = q.q2; p.qinfo = q.qinfo; p.lmax = q.lmax;
    p.aux = h->sh->aux_lay.stride > 0 ? h->sh->aux : nullptr; p.aux_lay = h->sh->aux_lay; p.qaux = q.qaux;
    p.tilemask = nullptr;
    p.outliers = h->sh->outliers; p.n_out = h->sh->n_out;
    p.pairs = h->sc.pairs; p.chunk_fill = h->sc.chunk_fill; p.wave_counts = h->sc.wave_counts; p.buckets = h->sc.buckets; p.cnt = h->sc.pass_cnt;
    p.seg_tiles = h->tune.seg_tiles;
    p.sched = h->tune.scan_sched[qb == 2 ? 1 : 0];
    return p;
}

// What a pass is asked for and where its results go: filled once per call (the entry points, search_core) and adjusted per pass.
// The sharded two-phase form (dph_search_sample_dev / dph_search_bounded_dev): `top_out` != NULL stops after the ladder and returns
// the DPH_SAMPLE_KEEP best sampled scores per row; `tau_ext` != NULL skips the ladder and scans under the caller's bounds,
// `bound_out` then receives the upper bound of the score of any row this shard did not return.
struct pass_args {
    int k = 1, nprobe = 0;
    int32_t* top_out = nullptr;          // [rows][DPH_SAMPLE_KEEP]
    const int32_t* tau_ext = nullptr;    // [rows]: the kernels read entries < n_q only
    const int* rowmap = nullptr;         // != NULL marks a retry pass: outputs scattered to rowmap[slot], larger C, failures go to fail2
    float* D = nullptr; int64_t* I = nullptr; int32_t* status = nullptr; double* bound_out = nullptr;
    int32_t* ik_out = nullptr; int32_t* fail_out = nullptr;
    bool retry() const { return rowmap != nullptr; }
    int C() const { return plan_select_C(k, retry()); }          // candidates the select step re-scores
};
// the two-stage form cuts a first-attempt pass behind its ladder (dph_search_prepare_dev / dph_search_finish_dev)
enum search_stage { SEARCH_WHOLE, SEARCH_PREPARE, SEARCH_FINISH };

// what every coarse search of a shard shares: its quantizer, the query rows, the score scratch (the caller adds masks and gate)
static dph_coarse_args coarse_args(const dph_shard& sh, const float* x, int q0, int n_q, int nprobe, float* scores) {
    dph_coarse_args c;
    c.x = x; c.q0 = q0; c.n_q = n_q;
    c.centroids = sh.centroids; c.nlist = sh.nlist; c.nprobe = nprobe; c.cnorm_max = sh.cnorm_max;
    c.scores = scores;
    c.tile_list = sh.tile_list; c.n_tiles = sh.n_tiles;
    return c;
}

// One pass = 128*qb query rows (unit scan: up to DPH_PASS_MAX), three stages: pass_probe [probe masks] -> pass_ladder (sampled bounds)
// -> pass_scan_select (full filter scan -> refine -> select).  search_core says which of them a pass runs.
// Stage 1, the probe set-up of a pass over a list-major shard: coarse search -> probe masks, or -> the work queue of a unit scan.
static int pass_probe(dph_index* h, dph_pass& p, const pass_args& a, hipStream_t st) {
    const dph_shard& sh = *h->sh;
    dph_ivf_pass& ivf = h->sc.ivf;
    if (!a.retry() && !p.gate && use_units(h, a.nprobe)) {
        int rc = ensure_units(h, a.nprobe);
        if (rc) return rc;
        const dph_unit_queue& uq = h->sc.uq;
        dph_coarse_args c = coarse_args(sh, p.x, p.q0, p.n_q, a.nprobe, ivf.coarse_scores);
        c.listmask = ivf.listmask_u; c.mask_words = DPH_UNIT_WORDS;
        dph_launch_coarse(c, h->sc.coarse, st);
        dph_launch_units_build(ivf, uq, sh.nlist, sh.list_tile0, p.q1, p.q0, h->tune.ivf_spread, dph_frag_x16(sh.aux_lay.stride), st);
        p.unit_recs = uq.unit_recs; p.unit_list_recs = uq.unit_list_recs; p.unit_cnt = ivf.unit_cnt; p.unit_launch = 0;
        p.slot_q = uq.slot_q; p.unit_frags = uq.unit_frags; p.listmask = ivf.listmask_u; p.tile_list = sh.tile_list;
        p.mask_words = DPH_UNIT_WORDS;
    } else if (sh.row_ids) {
        if (a.nprobe > 0) {
            dph_coarse_args c = coarse_args(sh, p.x, p.q0, p.n_q, a.nprobe, ivf.coarse_scores);
            c.gate = p.gate; c.gate_base = p.gate_base;
            c.listmask = ivf.listmask; c.mask_words = 8; c.tilemask = ivf.tilemask;
            dph_launch_coarse(c, h->sc.coarse, st);
            p.tilemask = ivf.tilemask;
        } else {
            p.tilemask = sh.onesmask;
        }
    }
    return DPH_OK;
}

// Stage 2, the ladder of sampled bounds (`p` by value: the unit work-queue head moves with the levels).  The sample form
// (a.top_out) gets the best sampled scores of the last level.
static int pass_ladder(dph_index* h, dph_pass p, const pass_args& a, hipStream_t st, pass_bound* b) {
    const bool units = p.unit_recs != nullptr;
    std::vector<ladder_level> levels;
    double last_ratio = 1.0;             // rows of the shard (of the probed lists) per row of the last level's sample
    if (units) {
        build_ladder_units(list_facts(h->sh), h->tune.fine_stride, p.n_q, a.nprobe, levels, &last_ratio);
    } else {
        std::vector<int> strides;
        build_ladder(ladder_facts(h), p.qb, strides);
        for (int v : strides) levels.push_back({v, 0xFFFFu});
        if (!strides.empty()) last_ratio = strides.back();
    }
    const int kp = plan_kp(h->tune.sample_kp, !levels.empty(), a.C(), last_ratio);
    if (!plan_ladder_fits(levels.size())) return fail(DPH_E_STATE, "ladder deeper than the unit work-queue heads");
    *b = pass_bound();
    for (size_t i = 0; i < levels.size(); ++i) {
        const int stride = levels[i].stride;
        const int* tau = b->tau;
        h->sc.prof.bracket(h->sc.prof.on && !a.retry() ? &h->sc.prof_events_ladder : nullptr, st, [&] {
            if (units) { p.unit_launch = (int)i; dph_launch_scan_units(p, true, stride, levels[i].rowmask, tau, st); }
            else dph_launch_scan(p, true, (h->sh->n_tiles + stride - 1) / stride, stride, tau, st);
        });
        dph_launch_refine(p, st);
        int* out = h->sc.tau_dev + (i & 1) * DPH_PASS_MAX;
        dph_launch_threshold(p, kp, tau, out, i + 1 == levels.size() ? a.top_out : nullptr, st);
        // a level that ran under a bound leaves a small bucket the full scan can build on; a COLD level (no bound: every
        // sampled row is in its bucket, more than the select step sorts) cannot be fused
        b->fuse_stride = tau ? stride : 0;
        b->tau = out;
    }
    // a shard too small for any ladder level shares nothing (INT_MIN everywhere)
    if (a.top_out && levels.empty()) HIPCHK(hipMemsetD32Async((hipDeviceptr_t)a.top_out, (int)0x80000000, (size_t)p.n_q * DPH_SAMPLE_KEEP, st));
    return DPH_OK;
}

// Stage 3: the full scan under b.tau, refine, select (+ the in-pass re-select).
static int pass_scan_select(dph_index* h, dph_pass p, const pass_args& a, const pass_bound& b, hipStream_t st) {
    const bool units = p.unit_recs != nullptr, retry = a.retry();
    // Fused finest level (flat shards): the last ladder level scanned every S-th tile under the previous level's bound, and its
    // refine left those tiles' candidates -- a superset of what the final bound admits -- in the buckets.  The full scan therefore
    // visits only the OTHER tiles and accumulates: the dump is read once per batch instead of 1 + 1/S times.  Every un-emitted row
    // still has I <= tau: the fused tiles were filtered under a bound <= tau.  (A pass that skipped the ladder brings stride 0.)
    int64_t full_tiles = h->sh->n_tiles;
    if (!units && !h->sh->row_ids && h->tune.ladder_fuse) {
        unsigned m = 0;
        const int64_t visit = fused_scan_plan(h->sh->n_tiles, b.fuse_stride, &m);
        if (visit > 0) { p.skip_m = m; p.accumulate = true; full_tiles = visit; }
    }
    if (!retry) h->sc.stats.fused_stride = p.skip_m ? b.fuse_stride : 0;
    h->sc.prof.bracket(h->sc.prof.on && !retry ? &h->sc.prof_events : nullptr, st, [&] {
        if (units) { p.unit_launch = DPH_UNIT_LAUNCHES - 1; dph_launch_scan_units(p, false, 1, 0xFFFFu, b.tau, st); }
        else dph_launch_scan(p, false, full_tiles, 1, b.tau, st);
    });
    dph_launch_refine(p, st);
    dph_select_args s{};
    s.lut = h->sh->lut_dev; s.k = a.k; s.C = a.C(); s.rmax = h->sh->rmax; s.rmax_all = h->sh->rmax_all; s.delta_max = h->sh->delta_max;
    s.offset = h->sh->offset; s.scale = h->sh->scale; s.tau = b.tau; s.rowmap = a.rowmap;
    s.D = a.D; s.I = a.I; s.status = a.status; s.bound_out = a.bound_out; s.ik_out = a.ik_out; s.fail_out = a.fail_out;
    dph_launch_select(p, s, st);
    // A row whose certificate did not close although every pair is in its bucket (near-ties at the k-th place: a run of near-duplicate
    // rows) does not need another scan of the shard -- the wider re-score of the retry pass can run on the bucket it already has.
    // Second look, same buckets, C = DPH_SELECT_C_MAX, flagged rows only (the others leave at once: ~5 us when nothing failed); only
    // rows that lost pairs or still fail go on to the re-scan.  (Document-ordered dump, batch 64: one such row in every fourth batch
    // used to cost a whole extra 18.5 ms scan of the 170 M-row shard.)
    if (!retry && s.fail_out && s.C < DPH_SELECT_C_MAX) {
        dph_select_args w = s;
        w.C = DPH_SELECT_C_MAX;
        w.only_failed = s.fail_out;
        w.reselect_count = &h->sc.counters.p->reselect;
        dph_launch_select(p, w, st);
    }
    if (!retry) h->sc.stats.scan_launches++;
    return DPH_OK;
}

static int check_search_args(dph_index* h, const void* x, int64_t n, int k, int nprobe, const void* D, const void* I,
                             const char* who) {
    if (!h || !x || !D || !I || n < 0 || k <= 0 || nprobe < 0) return fail(DPH_E_ARG, std::string(who) + ": bad arguments");
    if (k > 1024) return fail(DPH_E_ARG, std::string(who) + ": k <= 1024");
    if (n > (1 << 20)) return fail(DPH_E_ARG, std::string(who) + ": at most 2^20 query rows per call");
    if (!h->sh->finalized) return fail(DPH_E_STATE, std::string(who) + ": call dph_index_finalize first");
    if (nprobe > 0 && (!h->sh->centroids || !h->sh->row_ids)) return fail(DPH_E_STATE, std::string(who) + ": IVF data not set (dph_index_set_ivf)");
    return DPH_OK;
}

// The fp64 full scan of the (up to DPH_EXACT_ROWS_DEV) rows in exact_rows / exact_x, their count in counters.fail_retry: the probe masks of those
// rows on an IVF search, then the exact scan with `rounds` tightening rounds.
static void launch_exact_fallback(dph_index* h, int k, int nprobe, float* D, int64_t* I, int32_t* status, int rounds, hipStream_t st) {
    const unsigned* mask = nullptr;
    const int* n_rows = &h->sc.counters.p->fail_retry;
    if (h->sh->row_ids && nprobe > 0) {
        dph_coarse_args c = coarse_args(*h->sh, h->sc.exact_x, 0, DPH_EXACT_ROWS_DEV, nprobe, h->sc.ivf.coarse_scores);
        c.gate = n_rows;
        c.listmask = h->sc.ivf.listmask; c.mask_words = 8; c.tilemask = h->sc.ivf.tilemask;
        dph_launch_coarse(c, h->sc.coarse, st);
        mask = h->sc.ivf.tilemask;
    }
    dph_launch_exact(h->sh->db, h->sh->n_rows, make_idmap(h->sh), h->sc.exact_x, h->sh->lut_dev, h->sc.exact_rows, n_rows, DPH_EXACT_ROWS_DEV,
                     k, h->sh->row_ids, mask, D, I, status, h->sc.exact_scratch, h->sc.exact_scratch.n, st, rounds);
}

// The whole search of n query rows, enqueued on `st` without a host round trip:
//   1. quantise, then pass by pass (256 rows while at least 129 are left, else 128): ladder, scan, refine, select;
//   2. rows the first attempt could not certify are compacted on the device and searched again (passes of 128 rows,
//      gated by the device-side count) under a bound derived from their own k-th best integer score, with up to
//      DPH_SELECT_C_MAX re-scored candidates;
//   3. up to DPH_EXACT_ROWS_DEV rows that still fail go through the fp64 full scan.
// Afterwards status[r] = 0 for every row except the ones neither step could settle (counted by dph_search_get_stats).
static int search_core(dph_index* h, const float* x_dev, int64_t n, const pass_args& call, hipStream_t st, search_stage stage = SEARCH_WHOLE) {
    dph_search_counters* const cnt = h->sc.counters;
    if (stage != SEARCH_FINISH) {
        quantize(h, h->sc.q_main, x_dev, n, nullptr, st, true);
        // rows the in-pass wide re-select certifies (pass_scan_select); non-finite rows
        HIPCHK(hipMemsetAsync(&cnt->reselect, 0, offsetof(dph_search_counters, nonfinite) + sizeof(int) - offsetof(dph_search_counters, reselect), st));
    }
    // from here on the rows are read from the quantiser's clean copy (finish: the one the prepare stage left), never from the caller's buffer
    x_dev = h->sc.q_main.x;
    for (int64_t q0 = 0; q0 < n;) {
        const int64_t left = n - q0;
        const bool units = use_units(h, call.nprobe);               // a unit pass serves up to DPH_PASS_MAX rows
        int qb = 1;
        const int nq = plan_pass_rows(left, units, h->tune.max_qb, &qb);
        dph_pass p = make_pass(h, h->sc.q_main, x_dev, (int)q0, nq, qb);
        pass_args a = call;
        if (a.tau_ext) a.tau_ext += q0;
        if (a.top_out) a.top_out += q0 * DPH_SAMPLE_KEEP;
        a.ik_out = h->sc.ik_dev; a.fail_out = h->sc.fail_dev;
        int rc;
        if (stage == SEARCH_FINISH) {
            // (flat shards: no probe set-up) the prepare stage's last bound; its finest level's candidates wait in the buckets
            rc = pass_scan_select(h, p, a, h->sc.prep.bound, st);
        } else {
            rc = pass_probe(h, p, a, st);
            pass_bound b{a.tau_ext, 0};                              // the bounded form brings its bounds and skips the ladder
            if (!rc && !a.tau_ext) {
                // (prepare: the sampled levels run on the few CUs of a side stream -- as many workgroups as those, not one per CU of the chip)
                dph_pass lp = p;
                if (stage == SEARCH_PREPARE && h->tune.side_grid > 0) lp.grid = std::min(h->tune.side_grid, h->tune.grid);
                rc = pass_ladder(h, lp, a, st, &b);
            }
            if (rc) return rc;
            if (stage == SEARCH_PREPARE) h->sc.prep.bound = b;
            else if (!a.top_out) rc = pass_scan_select(h, p, a, b, st);   // (the sample form stops after the ladder)
        }
        if (rc) return rc;
        q0 += nq;
    }
    if (call.top_out || stage == SEARCH_PREPARE) { HIPCHK(hipGetLastError()); return DPH_OK; }
    if (!h->tune.retry_chain) {
        // measurements / diagnostics: no re-scan, no fp64 fallback -- the counters say how many rows the first attempt left open, their
        // status stays 1 (and the buckets of the last pass stay readable: dph_debug_bucket_counts)
        dph_launch_compact_failing(h->sc.fail_dev, n, 0, nullptr, h->sc.retry_rows, &cnt->fail_first, nullptr, 0, st);
        HIPCHK(hipMemcpyAsync(&cnt->fail_retry, &cnt->fail_first, sizeof(int), hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(&cnt->unsettled, &cnt->fail_first, sizeof(int), hipMemcpyDeviceToDevice, st));
        dph_launch_nonfinite_fix(h->sc.q_main.nf, n, call.k, call.D, call.I, call.status, call.bound_out, &cnt->nonfinite, st);
        HIPCHK(hipGetLastError());
        return DPH_OK;
    }

    // ---- 2. on-device retry of the rows that failed
    dph_launch_compact_failing(h->sc.fail_dev, n, 0, x_dev, h->sc.retry_rows, &cnt->fail_first, h->sc.q_retry.x, (int)n, st);
    quantize(h, h->sc.q_retry, h->sc.q_retry.x, n, &cnt->fail_first, st);
    dph_launch_retry_tau(&cnt->fail_first, n, h->sc.retry_rows, h->sc.ik_dev, h->sc.q_retry.qinfo, h->sh->rmax, h->sh->delta_max, h->sh->scale,
                         h->sc.retry_tau, st);
    HIPCHK(hipMemsetAsync(h->sc.fail2_dev, 0, (size_t)n * 4, st));
    for (int64_t q0 = 0; q0 < n; q0 += DPH_QROWS) {
        const int nq = (int)std::min<int64_t>(n - q0, DPH_QROWS);
        dph_pass p = make_pass(h, h->sc.q_retry, h->sc.q_retry.x, (int)q0, nq, 1);
        p.gate = &cnt->fail_first;
        p.gate_base = (int)q0;
        p.wave_counts = h->sc.wave_counts + (size_t)h->tune.grid * 8;
        pass_args a = call;                                          // (never the sample form: that returned above)
        a.tau_ext = h->sc.retry_tau + q0; a.rowmap = h->sc.retry_rows; a.fail_out = h->sc.fail2_dev;
        int rc = pass_probe(h, p, a, st);
        if (!rc) rc = pass_scan_select(h, p, a, pass_bound{a.tau_ext, 0}, st);
        if (rc) return rc;
    }
    // ---- 3. fp64 full scan for (up to DPH_EXACT_ROWS_DEV of) the rows the retry could not settle
    dph_launch_compact_failing(h->sc.fail2_dev, n, 0, x_dev, h->sc.exact_rows, &cnt->fail_retry, h->sc.exact_x, DPH_EXACT_ROWS_DEV, st);
    launch_exact_fallback(h, call.k, call.nprobe, call.D, call.I, call.status, 1, st);
    // the result of a non-finite query row: ids -1, scores -FLT_MAX, status DPH_ROW_NONFINITE (its stand-in was searched like any row)
    dph_launch_nonfinite_fix(h->sc.q_main.nf, n, call.k, call.D, call.I, call.status, call.bound_out, &cnt->nonfinite, st);
    // rows still flagged 1 (more than DPH_EXACT_ROWS_DEV failures, or boundary ties beyond the fp64 scan's buffer)
    dph_launch_compact_failing(call.status, n, 1, nullptr, h->sc.retry_rows, &cnt->unsettled, nullptr, 0, st);
    HIPCHK(hipGetLastError());
    return DPH_OK;
}

static int read_counters(dph_index* h, hipStream_t st, dph_search_counters* out) {
    HIPCHK(hipMemcpyAsync(out, h->sc.counters, sizeof(*out), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return DPH_OK;
}

// The one rule from the counters of a call to its statistics (s.rows set by the entry point); `unsettled`: rows still open at the end.
// (A non-finite row's stand-in is searched and certified like any row; the row is counted once, as non-finite.)
static void fill_stats(dph_search_stats& s, const dph_search_counters& c, int unsettled) {
    s.nonfinite = c.nonfinite;
    s.certified_fast = s.rows - c.fail_first - c.reselect - c.nonfinite;
    s.certified_wide = c.fail_first - c.fail_retry + c.reselect;
    s.certified_reselect = c.reselect;        // the first look could not certify, the wider look at the same bucket could (no re-scan)
    s.exact_fallback = c.fail_retry - unsettled;
    s.uncertified = unsettled;
}

// a call starts its statistics; pending = its device counters are read back only when dph_search_get_stats asks
static void begin_stats(dph_index* h, int64_t n, bool pending) {
    h->sc.stats = dph_search_stats{};
    h->sc.stats.rows = (int32_t)n;
    h->sc.stats_pending = pending;
}
static int pq_nprobe(const dph_index* h, int nprobe) { return nprobe > 0 ? nprobe : (h->tune.default_nprobe > 0 ? h->tune.default_nprobe : 256); }

static int search_dev_impl(dph_index* h, const float* x_dev, int64_t n, int k, int nprobe, float* D_dev, int64_t* I_dev,
                           int32_t* status_dev, void* stream, const char* who, pass_args opt = pass_args()) {
    if (h && h->sh->pq) {
        if (!x_dev || !D_dev || !I_dev || !status_dev || n < 0 || k <= 0 || k > 1024) return fail(DPH_E_ARG, std::string(who) + ": bad arguments");
        if (opt.top_out || opt.tau_ext) return fail(DPH_E_STATE, std::string(who) + ": the sharded two-phase entry points do not serve PQ indexes");
        if (!h->sh->finalized) return fail(DPH_E_STATE, std::string(who) + ": call dph_index_finalize first");
        if (n == 0) return DPH_OK;
        HIPCHK(hipSetDevice(h->device));
        if (!h->sc.counters) HIPCHK(h->sc.counters.alloc(1));
        begin_stats(h, n, false);
        const int rc = dph_pq_search_dev(h->sh->pq, x_dev, n, k, pq_nprobe(h, nprobe), D_dev, I_dev, status_dev, (hipStream_t)stream);
        if (rc) return fail(rc, std::string(who) + ": " + dph_last_error());
        // the rows' statuses, counted on the device: uncertified, non-finite (read back when dph_search_get_stats asks)
        static_assert(offsetof(dph_search_counters, pq.nonfinite) == offsetof(dph_search_counters, pq.uncertified) + sizeof(int), "out[0], out[1]");
        dph_launch_count_status(status_dev, n, &h->sc.counters.p->pq.uncertified, (hipStream_t)stream);
        HIPCHK(hipGetLastError());
        h->sc.stats_pending = true;
        return DPH_OK;
    }
    int rc = check_search_args(h, x_dev, n, k, nprobe, D_dev, I_dev, who);
    if (rc) return rc;
    if (!status_dev) return fail(DPH_E_ARG, std::string(who) + ": status buffer is NULL");
    if (n == 0) return DPH_OK;
    HIPCHK(hipSetDevice(h->device));
    rc = ensure_scratch(h, n, 0);
    if (rc) return rc;
    begin_stats(h, n, true);
    opt.k = k; opt.nprobe = nprobe; opt.D = D_dev; opt.I = I_dev; opt.status = status_dev;
    return search_core(h, x_dev, n, opt, (hipStream_t)stream);
}

static int search_host_impl(dph_index* h, const float* x, int64_t n, int k, int nprobe, float* D, int64_t* I, const char* who) {
    if (h && h->sh->pq) {
        if (!x || !D || !I || n < 0 || k <= 0 || k > 1024) return fail(DPH_E_ARG, std::string(who) + ": bad arguments");
        if (n == 0) return DPH_OK;
        HIPCHK(hipSetDevice(h->device));
        dev_buf<char> blob;
        const size_t b_x = ((size_t)n * DPH_DIM * 4 + 255) / 256 * 256, b_d = ((size_t)n * k * 4 + 255) / 256 * 256, b_i = ((size_t)n * k * 8 + 255) / 256 * 256;
        HIPCHK(blob.alloc(b_x + b_d + b_i + (size_t)n * 4));
        int rc = DPH_OK;
        std::vector<int32_t> status((size_t)n);
        if (hipMemcpy(blob, x, (size_t)n * DPH_DIM * 4, hipMemcpyHostToDevice) != hipSuccess) rc = fail(DPH_E_HIP, std::string(who) + ": copy failed");
        if (!rc) rc = search_dev_impl(h, (const float*)blob.p, n, k, nprobe, (float*)(blob + b_x), (int64_t*)(blob + b_x + b_d),
                                      (int32_t*)(blob + b_x + b_d + b_i), nullptr, who);
        if (!rc && (hipMemcpy(D, blob + b_x, (size_t)n * k * 4, hipMemcpyDeviceToHost) != hipSuccess ||
                    hipMemcpy(I, blob + b_x + b_d, (size_t)n * k * 8, hipMemcpyDeviceToHost) != hipSuccess ||
                    hipMemcpy(status.data(), blob + b_x + b_d + b_i, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess))
            rc = fail(DPH_E_HIP, std::string(who) + ": copy failed");
        if (rc) return rc;
        int bad = 0, nf = 0;
        for (int32_t v : status) { bad += v == 1; nf += v == DPH_ROW_NONFINITE; }
        h->sc.stats_pending = false;        // (counted here from the copied statuses)
        h->sc.stats.uncertified = bad;
        h->sc.stats.nonfinite = nf;
        h->sc.stats.certified_fast = (int32_t)n - bad - nf;
        if (bad) return fail(DPH_E_UNCERTIFIED, std::string(who) + ": candidate buffers of the PQ scan overflowed (boundary ties)");
        return DPH_OK;
    }
    int rc = check_search_args(h, x, n, k, nprobe, D, I, who);
    if (rc) return rc;
    if (n == 0) return DPH_OK;
    HIPCHK(hipSetDevice(h->device));
    rc = ensure_scratch(h, n, k);
    if (rc) return rc;
    hipStream_t st = nullptr;
    begin_stats(h, n, false);
    HIPCHK(hipMemcpyAsync(h->sc.q_main.x, x, (size_t)n * DPH_DIM * 4, hipMemcpyHostToDevice, st));
    pass_args call;
    call.k = k; call.nprobe = nprobe; call.D = h->sc.D_dev; call.I = h->sc.I_dev; call.status = h->sc.status_dev;
    rc = search_core(h, h->sc.q_main.x, n, call, st);
    if (rc) return rc;
    dph_search_counters c{};
    rc = read_counters(h, st, &c);
    if (rc) return rc;
    int left = c.unsettled;
    if (left > 0) {
        // more failures than the on-device fallback serves per call: feed it the rest, DPH_EXACT_ROWS_DEV at a time
        std::vector<int32_t> status((size_t)n);
        HIPCHK(hipMemcpy(status.data(), h->sc.status_dev, (size_t)n * 4, hipMemcpyDeviceToHost));
        std::vector<int32_t> todo;
        for (int64_t r = 0; r < n; ++r) if (status[r] == 1) todo.push_back((int32_t)r);
        // (the rows the device pass already tried -- one tightening round -- get the three rounds of this loop as well)
        std::vector<int32_t> rest(todo);
        for (size_t i0 = 0; i0 < rest.size(); i0 += DPH_EXACT_ROWS_DEV) {
            const int m = (int)std::min<size_t>(DPH_EXACT_ROWS_DEV, rest.size() - i0);
            HIPCHK(hipMemcpyAsync(h->sc.exact_rows, rest.data() + i0, (size_t)m * 4, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(&h->sc.counters.p->fail_retry, &m, sizeof(int), hipMemcpyHostToDevice, st));
            dph_launch_gather_rows(h->sc.q_main.x, h->sc.exact_rows, &h->sc.counters.p->fail_retry, h->sc.exact_x, DPH_EXACT_ROWS_DEV, st);
            launch_exact_fallback(h, k, nprobe, h->sc.D_dev, h->sc.I_dev, h->sc.status_dev, 3, st);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(st));
        }
        HIPCHK(hipMemcpy(status.data(), h->sc.status_dev, (size_t)n * 4, hipMemcpyDeviceToHost));
        left = 0;
        for (int64_t r = 0; r < n; ++r) left += status[r] == 1;
    }
    fill_stats(h->sc.stats, c, left);
    HIPCHK(hipMemcpy(D, h->sc.D_dev, (size_t)n * k * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(I, h->sc.I_dev, (size_t)n * k * 8, hipMemcpyDeviceToHost));
    if (left > 0) return fail(DPH_E_UNCERTIFIED, std::string(who) + ": boundary ties exceed the exact-scan buffer");
    return DPH_OK;
}

static int default_nprobe(const dph_index* h) { return (h && ((h->sh->centroids && h->sh->row_ids) || h->sh->pq)) ? h->tune.default_nprobe : 0; }

int dph_search_dev(dph_index* h, const float* x_dev, int64_t n, int k, float* D_dev, int64_t* I_dev,
                   int32_t* status_dev, void* stream) {
    return search_dev_impl(h, x_dev, n, k, default_nprobe(h), D_dev, I_dev, status_dev, stream, "dph_search_dev");
}
int dph_search(dph_index* h, const float* x, int64_t n, int k, float* D, int64_t* I) {
    return search_host_impl(h, x, n, k, default_nprobe(h), D, I, "dph_search");
}
int dph_search_ivf_dev(dph_index* h, const float* x_dev, int64_t n, int k, int nprobe, float* D_dev, int64_t* I_dev,
                       int32_t* status_dev, void* stream) {
    if (nprobe <= 0) return fail(DPH_E_ARG, "dph_search_ivf_dev: nprobe must be > 0");
    return search_dev_impl(h, x_dev, n, k, nprobe, D_dev, I_dev, status_dev, stream, "dph_search_ivf_dev");
}
int dph_search_ivf(dph_index* h, const float* x, int64_t n, int k, int nprobe, float* D, int64_t* I) {
    if (nprobe <= 0) return fail(DPH_E_ARG, "dph_search_ivf: nprobe must be > 0");
    return search_host_impl(h, x, n, k, nprobe, D, I, "dph_search_ivf");
}

// ---- two-phase search of a range-sharded dump under a bound taken over the union of all shards' samples
int dph_search_sample_dev(dph_index* h, const float* x_dev, int64_t n, int32_t* top_dev, void* stream) {
    if (!h || !x_dev || !top_dev || n < 0 || n > (1 << 20)) return fail(DPH_E_ARG, "dph_search_sample_dev: bad arguments");
    if (!h->sh->finalized) return fail(DPH_E_STATE, "dph_search_sample_dev: call dph_index_finalize first");
    if (n == 0) return DPH_OK;
    HIPCHK(hipSetDevice(h->device));
    int rc = ensure_scratch(h, n, 0);
    if (rc) return rc;
    pass_args call;
    call.nprobe = default_nprobe(h); call.top_out = top_dev;
    return search_core(h, x_dev, n, call, (hipStream_t)stream);
}

int dph_union_bounds_dev(int device, const int32_t* top_parts, int n_parts, int64_t n, int32_t* tau_dev, void* stream) {
    if (!top_parts || !tau_dev || n_parts <= 0 || n < 0) return fail(DPH_E_ARG, "dph_union_bounds_dev: bad arguments");
    HIPCHK(hipSetDevice(device));
    if (n > 0) dph_launch_union_bounds(top_parts, n_parts, n, tau_dev, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return DPH_OK;
}

int dph_search_bounded_dev(dph_index* h, const float* x_dev, int64_t n, int k, const int32_t* tau_dev, float* D_dev,
                           int64_t* I_dev, int32_t* status_dev, double* bound_dev, void* stream) {
    if (!tau_dev || !bound_dev) return fail(DPH_E_ARG, "dph_search_bounded_dev: null buffer");
    pass_args opt;
    opt.tau_ext = tau_dev;
    opt.bound_out = bound_dev;
    return search_dev_impl(h, x_dev, n, k, default_nprobe(h), D_dev, I_dev, status_dev, stream, "dph_search_bounded_dev", opt);
}

// ---- the search in two stages, for two batches in flight on one shard (dph_index_create_twin; one handle per batch in flight).
// prepare: quantise + the sampled levels (every scan launch of them with `side_grid` workgroups) -- leaves the bound and the finest
// level's candidates in the handle; finish: the full scan (fused with that level), refine, select, retry chain.  Together they enqueue
// exactly the launches of dph_search_dev, with the same arguments: the same result.  One pass only (n <= 256 rows), flat shards.
static int two_stage_check(dph_index* h, const float* x_dev, int64_t n, int k, const char* who) {
    if (!h || !x_dev || n <= 0 || k <= 0 || k > 1024) return fail(DPH_E_ARG, std::string(who) + ": bad arguments");
    if (!h->sh->finalized) return fail(DPH_E_STATE, std::string(who) + ": call dph_index_finalize first");
    if (h->sh->pq || h->sh->row_ids) return fail(DPH_E_STATE, std::string(who) + ": flat shards only");
    if (n > (int64_t)DPH_QROWS * std::min(h->tune.max_qb, DPH_MAX_QB)) return fail(DPH_E_ARG, std::string(who) + ": one pass per call (at most 128 x max_qb query rows)");
    return DPH_OK;
}

int dph_search_prepare_dev(dph_index* h, const float* x_dev, int64_t n, int k, void* stream) {
    int rc = two_stage_check(h, x_dev, n, k, "dph_search_prepare_dev");
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    rc = ensure_scratch(h, n, 0);
    if (rc) return rc;
    h->sc.prep = dph_scratch::prepared();
    pass_args call;
    call.k = k;
    rc = search_core(h, x_dev, n, call, (hipStream_t)stream, SEARCH_PREPARE);
    if (rc) return rc;
    h->sc.prep.valid = true; h->sc.prep.n = n; h->sc.prep.k = k;
    return DPH_OK;
}

int dph_search_finish_dev(dph_index* h, const float* x_dev, int64_t n, int k, float* D_dev, int64_t* I_dev, int32_t* status_dev, void* stream) {
    int rc = two_stage_check(h, x_dev, n, k, "dph_search_finish_dev");
    if (rc) return rc;
    if (!D_dev || !I_dev || !status_dev) return fail(DPH_E_ARG, "dph_search_finish_dev: null buffer");
    if (!h->sc.prep.valid || h->sc.prep.n != n || h->sc.prep.k != k)
        return fail(DPH_E_STATE, "dph_search_finish_dev: no matching dph_search_prepare_dev on this handle (same n, same k)");
    HIPCHK(hipSetDevice(h->device));
    h->sc.prep.valid = false;
    begin_stats(h, n, true);
    pass_args call;
    call.k = k; call.D = D_dev; call.I = I_dev; call.status = status_dev;
    return search_core(h, x_dev, n, call, (hipStream_t)stream, SEARCH_FINISH);
}

// A stream whose kernels run on the CUs [first_cu, first_cu + n_cus) of the device's CU-mask bit order only (MI355X: bit i is a CU of
// XCD i % 8, so any run of 8 k bits takes k CUs from every XCD -- profiles/r04_cu_mask_probe.txt).  Two such streams over disjoint
// ranges run their kernels side by side whatever either of them occupies.
int dph_stream_create_cu_range(int device, int first_cu, int n_cus, void** stream_out) {
    if (!stream_out || first_cu < 0 || n_cus <= 0) return fail(DPH_E_ARG, "dph_stream_create_cu_range: bad arguments");
    HIPCHK(hipSetDevice(device));
    int cus = 0;
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    if (first_cu + n_cus > cus) return fail(DPH_E_ARG, "dph_stream_create_cu_range: range beyond the device's CUs");
    std::vector<uint32_t> mask((size_t)(cus + 31) / 32, 0u);
    for (int i = first_cu; i < first_cu + n_cus; ++i) mask[(size_t)i / 32] |= 1u << (i % 32);
    hipStream_t st = nullptr;
    HIPCHK(hipExtStreamCreateWithCUMask(&st, (uint32_t)mask.size(), mask.data()));
    *stream_out = (void*)st;
    return DPH_OK;
}
int dph_stream_destroy(void* stream) {
    if (stream) HIPCHK(hipStreamDestroy((hipStream_t)stream));
    return DPH_OK;
}

int dph_search_get_stats(dph_index* h, dph_search_stats* out) {
    if (!h || !out) return fail(DPH_E_ARG, "null");
    if (h->sc.stats_pending) {
        // device-pointer call: the counters live on the device until somebody asks (this synchronises the device)
        HIPCHK(hipSetDevice(h->device));
        dph_search_counters c{};
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpy(&c, h->sc.counters, sizeof(c), hipMemcpyDeviceToHost));
        h->sc.stats_pending = false;
        if (h->sh->pq) {                     // (search_dev_impl: the statuses the PQ search wrote, counted)
            h->sc.stats.uncertified = c.pq.uncertified;
            h->sc.stats.nonfinite = c.pq.nonfinite;
            h->sc.stats.certified_fast = h->sc.stats.rows - c.pq.uncertified - c.pq.nonfinite;
        } else {
            fill_stats(h->sc.stats, c, c.unsettled);
        }
    }
    *out = h->sc.stats;
    return DPH_OK;
}

// pairs the scan kernels emitted / emit-path triggers (wave level) in the LAST scan launch on this handle
int dph_scan_counters(dph_index* h, int64_t* pairs_out, int64_t* triggers_out) {
    if (!h || !pairs_out || !triggers_out) return fail(DPH_E_ARG, "null");
    if (!h->sc.wave_counts) return fail(DPH_E_STATE, "dph_scan_counters: no search yet");
    HIPCHK(hipSetDevice(h->device));
    std::vector<unsigned> wc((size_t)h->tune.grid * 8);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(wc.data(), h->sc.wave_counts, wc.size() * 4, hipMemcpyDeviceToHost));
    int64_t a = 0, b = 0;
    for (size_t i = 0; i < wc.size(); i += 2) { a += wc[i]; b += wc[i + 1]; }
    *pairs_out = a; *triggers_out = b;
    return DPH_OK;
}

int dph_debug_wave_pairs(dph_index* h, int image, uint32_t* pairs_out, int out_cap, int* n_waves) {
    if (!h || !pairs_out || !n_waves || (image != 0 && image != 1)) return fail(DPH_E_ARG, "dph_debug_wave_pairs: bad arguments");
    if (!h->sc.wave_counts) return fail(DPH_E_STATE, "dph_debug_wave_pairs: no search yet");
    const int nw = h->tune.grid * 4;
    if (out_cap < nw) return fail(DPH_E_ARG, "dph_debug_wave_pairs: buffer too small");
    HIPCHK(hipSetDevice(h->device));
    std::vector<unsigned> wc((size_t)nw * 2);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(wc.data(), h->sc.wave_counts + (size_t)image * nw * 2, wc.size() * 4, hipMemcpyDeviceToHost));
    for (int w = 0; w < nw; ++w) pairs_out[w] = wc[(size_t)2 * w];
    *n_waves = nw;
    return DPH_OK;
}

int dph_reconstruct(dph_index* h, int64_t id, float* out768) {
    if (!h || !out768) return fail(DPH_E_ARG, "null");
    if (h->sh->pq) {
        // IndexIVFPQ::reconstruct through the direct map: centroid + decoded residual, in the ROTATED space (index.py:31,286)
        HIPCHK(hipSetDevice(h->device));
        dev_buf<char> blob;
        HIPCHK(blob.alloc(16 + DPH_DIM * 4));
        int32_t found = 0;
        int rc = DPH_OK;
        if (hipMemcpy(blob, &id, 8, hipMemcpyHostToDevice) != hipSuccess) rc = fail(DPH_E_HIP, "dph_reconstruct: copy failed");
        if (!rc) rc = dph_pq_reconstruct_dev(h->sh->pq, (const int64_t*)blob.p, 1, (float*)(blob + 16), (int32_t*)(blob + 8), nullptr);
        if (!rc && (hipMemcpy(&found, blob + 8, 4, hipMemcpyDeviceToHost) != hipSuccess ||
                    hipMemcpy(out768, blob + 16, DPH_DIM * 4, hipMemcpyDeviceToHost) != hipSuccess)) rc = fail(DPH_E_HIP, "dph_reconstruct: copy failed");
        if (rc) return rc;
        return found ? DPH_OK : fail(DPH_E_NOTFOUND, "dph_reconstruct: id not in the index");
    }
    const int64_t local = host_local_of_id(h->sh, id);
    if (local < 0) return fail(DPH_E_NOTFOUND, "dph_reconstruct: id not in this shard");
    HIPCHK(hipSetDevice(h->device));
    const int64_t srow = h->sh->h_inv.empty() ? local : (int64_t)h->sh->h_inv[(size_t)local];
    int8_t row[DPH_DIM];
    HIPCHK(hipMemcpy(row, h->sh->db + srow * DPH_DIM, DPH_DIM, hipMemcpyDeviceToHost));
    for (int j = 0; j < DPH_DIM; ++j) out768[j] = h->sh->lut_host[(int)row[j] + 128];
    return DPH_OK;
}

int dph_id2docword(dph_index* h, const int64_t* I, int64_t n, int32_t* doc, int32_t* word) {
    if (!h || !I || !doc || !word || n < 0) return fail(DPH_E_ARG, "null");
    if (h->sh->h_row2doc.empty() && h->sh->n_ids > 0) return fail(DPH_E_STATE, "dph_id2docword: idx2id not set");
    const int64_t first = h->sh->h_id_offsets.empty() ? h->sh->id_base : h->sh->h_id_offsets[0];
    for (int64_t i = 0; i < n; ++i) {
        if (h->sh->n_ids == 0) { doc[i] = -1; word[i] = -1; continue; }      // empty shard: nothing to clip to
        int64_t local = host_local_of_id(h->sh, I[i]);
        if (local < 0) local = I[i] < first ? 0 : h->sh->n_ids - 1;          // np.clip (index.py:133); a hole between sub-indexes clips up
        doc[i] = h->sh->h_row2doc[(size_t)local];
        word[i] = h->sh->h_row2word[(size_t)local];
    }
    return DPH_OK;
}

int dph_rescore_dev(dph_index* h, int direction, const float* qhalf_dev, int64_t n_q, int k, int L,
                    const int64_t* ids_dev, const int32_t* doc_dev, const int32_t* word_dev, const float* first_dev,
                    int32_t* pred_word_dev, double* best_dev, int32_t* argslot_dev, float* vecs_dev, void* stream) {
    if (!h || !qhalf_dev || !ids_dev || !first_dev || !pred_word_dev || !best_dev || !argslot_dev || n_q < 0 || k <= 0 || L <= 0)
        return fail(DPH_E_ARG, "dph_rescore_dev: bad arguments");
    if (direction != 0 && direction != 1) return fail(DPH_E_ARG, "dph_rescore_dev: direction is 0 or 1");
    if (!h->sh->doc_ids || !h->sh->f2o_off || !h->sh->f2o) return fail(DPH_E_STATE, "dph_rescore_dev: f2o metadata not set");
    if ((!doc_dev || !word_dev) && !h->sh->row2doc) return fail(DPH_E_STATE, "dph_rescore_dev: idx2id not set");
    HIPCHK(hipSetDevice(h->device));
    const dph_shard* sh = h->sh;
    const dph_window_args a = make_window_args(h, direction, qhalf_dev, n_q, k, L, ids_dev, doc_dev, word_dev, first_dev, pred_word_dev, best_dev,
                                               argslot_dev, vecs_dev);
    if (sh->pq) {
        // the raw rows are resident: the HDF5 branch of the reference (index.py:246-273); otherwise windows of reconstructions
        if (sh->doc_rows && !sh->finalized) return fail(DPH_E_STATE, "dph_rescore_dev: call dph_index_finalize after attaching document rows");
        const int rc = dph_pq_window(sh->pq, a, sh->doc_rows, sh->n_doc_rows, sh->doc_lut, (hipStream_t)stream);
        return rc ? fail(rc, std::string("dph_rescore_dev: ") + dph_last_error()) : DPH_OK;
    }
    dph_launch_window(a, nullptr, sh->db, sh->n_rows, sh->lut_dev, sh->inv_row, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return DPH_OK;
}

int dph_rescore(dph_index* h, int direction, const float* qhalf, int64_t n_q, int k, int L, const int64_t* ids,
                const int32_t* doc, const int32_t* word, const float* first, int32_t* pred_word, double* best,
                int32_t* argslot, float* vecs) {
    if (!h || !qhalf || !ids || !doc || !word || !first || !pred_word || !best || !argslot)
        return fail(DPH_E_ARG, "dph_rescore: null argument");
    HIPCHK(hipSetDevice(h->device));
    const int64_t nc = n_q * k;
    if (nc == 0) return DPH_OK;
    dev_buf<char> blob;
    const size_t b_q = (size_t)n_q * DPH_DIM * 4, b_ids = (size_t)nc * 8, b_i32 = (size_t)nc * 4, b_f64 = (size_t)nc * 8;
    const size_t b_vec = vecs ? (size_t)nc * 2 * DPH_DIM * 4 : 0;
    size_t off = 0;
    auto take = [&](size_t b) { size_t o = off; off += (b + 255) / 256 * 256; return o; };
    const size_t o_q = take(b_q), o_ids = take(b_ids), o_doc = take(b_i32), o_word = take(b_i32), o_first = take(b_i32),
                 o_pw = take(b_i32), o_best = take(b_f64), o_arg = take(b_i32), o_vec = take(b_vec);
    HIPCHK(blob.alloc(off));
    int rc = DPH_OK;
    auto up = [&](size_t o, const void* p, size_t b) { if (hipMemcpy(blob + o, p, b, hipMemcpyHostToDevice) != hipSuccess) rc = DPH_E_HIP; };
    up(o_q, qhalf, b_q); up(o_ids, ids, b_ids); up(o_doc, doc, b_i32); up(o_word, word, b_i32); up(o_first, first, b_i32);
    if (!rc)
        rc = dph_rescore_dev(h, direction, (const float*)(blob + o_q), n_q, k, L, (const int64_t*)(blob + o_ids),
                             (const int32_t*)(blob + o_doc), (const int32_t*)(blob + o_word), (const float*)(blob + o_first),
                             (int32_t*)(blob + o_pw), (double*)(blob + o_best), (int32_t*)(blob + o_arg),
                             vecs ? (float*)(blob + o_vec) : nullptr, nullptr);
    auto down = [&](void* p, size_t o, size_t b) { if (hipMemcpy(p, blob + o, b, hipMemcpyDeviceToHost) != hipSuccess) rc = DPH_E_HIP; };
    if (!rc) { down(pred_word, o_pw, b_i32); down(best, o_best, b_f64); down(argslot, o_arg, b_i32); if (vecs) down(vecs, o_vec, b_vec); }
    if (rc == DPH_E_HIP) return fail(DPH_E_HIP, "dph_rescore: copy failed");
    return rc;
}

int dph_ivf_assign_dev(int device, const float* x_dev, int64_t n, const float* centroids_dev, int nlist, const float* bias_dev,
                       float* scores_dev, int32_t* best_dev, float* gap_dev, void* stream) {
    (void)scores_dev;                    // ABI 2 took a [n, nlist] scratch here; the fused kernel writes no scores
    if (!x_dev || !centroids_dev || !best_dev || !gap_dev || n < 0 || nlist <= 0)
        return fail(DPH_E_ARG, "dph_ivf_assign_dev: bad arguments");
    HIPCHK(hipSetDevice(device));
    if (n > 0) dph_launch_assign(x_dev, false, nullptr, n, centroids_dev, nlist, bias_dev, best_dev, gap_dev, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return DPH_OK;
}

int dph_index_assign_dev(dph_index* h, int64_t row0, int64_t n, const float* centroids_dev, int nlist, const float* bias_dev,
                         int32_t* best_dev, float* gap_dev, void* stream) {
    if (!h || !centroids_dev || !best_dev || !gap_dev || row0 < 0 || n < 0 || row0 + n > h->sh->n_rows || nlist <= 0)
        return fail(DPH_E_ARG, "dph_index_assign_dev: bad arguments");
    HIPCHK(hipSetDevice(h->device));
    if (n > 0)
        dph_launch_assign(h->sh->db + row0 * DPH_DIM, true, h->sh->lut_dev, n, centroids_dev, nlist, bias_dev, best_dev, gap_dev,
                          (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return DPH_OK;
}

int dph_index_gather_rows_dev(dph_index* h, const int64_t* rows_idx_dev, int64_t m, int8_t* sample_dev, void* stream) {
    if (!h || !rows_idx_dev || !sample_dev || m < 0) return fail(DPH_E_ARG, "dph_index_gather_rows_dev: bad arguments");
    HIPCHK(hipSetDevice(h->device));
    dph_launch_gather_sample(h->sh->db, h->sh->n_rows, rows_idx_dev, m, sample_dev, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return DPH_OK;
}

int dph_kmeans_step_dev(dph_index* h, const int8_t* rows_dev, int64_t m, float* centroids_dev, int nlist, const float* bias_dev,
                        int spherical, int32_t* assign_dev, float* gap_dev, uint32_t* counts_dev, void* stream) {
    if (!h || !rows_dev || !centroids_dev || !assign_dev || !gap_dev || !counts_dev || m < 0 || nlist <= 0 || nlist > (1 << 20))
        return fail(DPH_E_ARG, "dph_kmeans_step_dev: bad arguments");
    DPH_NOT_TWINNED(h, "dph_kmeans_step_dev");           // (refused as before the scratch became the handle's own)
    HIPCHK(hipSetDevice(h->device));
    if (h->sc.kmeans_nlist < nlist) {
        h->sc.kmeans_nlist = 0;
        HIPCHK(h->sc.kmeans_sums.alloc((size_t)nlist * DPH_DIM));
        h->sc.kmeans_nlist = nlist;
    }
    hipStream_t st = (hipStream_t)stream;
    if (m > 0) dph_launch_assign(rows_dev, true, h->sh->lut_dev, m, centroids_dev, nlist, bias_dev, assign_dev, gap_dev, st);
    dph_launch_kmeans_update(rows_dev, assign_dev, m, nlist, h->sh->offset, h->sh->scale, spherical, h->sc.kmeans_sums, counts_dev, centroids_dev, st);
    HIPCHK(hipGetLastError());
    return DPH_OK;
}

int64_t dph_index_stored_rows(const dph_index* h) { return h ? h->sh->n_rows : 0; }

int dph_score_vecs_dev(int device, const float* q_dev, const float* vecs_dev, int64_t n_b, int64_t m, float* out_dev, void* stream) {
    if (!q_dev || !vecs_dev || !out_dev || n_b < 0 || m < 0) return fail(DPH_E_ARG, "dph_score_vecs_dev: bad arguments");
    HIPCHK(hipSetDevice(device));
    dph_launch_score_vecs(q_dev, vecs_dev, n_b, m, out_dev, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return DPH_OK;
}
int dph_score_vecs_bwd_dev(int device, const float* grad_dev, const float* vecs_dev, int64_t n_b, int64_t m, float* grad_q_dev,
                           void* stream) {
    if (!grad_dev || !vecs_dev || !grad_q_dev || n_b < 0 || m < 0) return fail(DPH_E_ARG, "dph_score_vecs_bwd_dev: bad arguments");
    HIPCHK(hipSetDevice(device));
    dph_launch_score_vecs_bwd(grad_dev, vecs_dev, n_b, m, grad_q_dev, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return DPH_OK;
}
int dph_dense_logits_dev(int device, const float* start_logits_dev, const float* end_logits_dev, int64_t n_b, int64_t T,
                         float* out_dev, void* stream) {
    if (!start_logits_dev || !end_logits_dev || !out_dev || n_b < 0 || T < 0) return fail(DPH_E_ARG, "dph_dense_logits_dev: bad arguments");
    HIPCHK(hipSetDevice(device));
    dph_launch_dense_logits(start_logits_dev, end_logits_dev, n_b, T, out_dev, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return DPH_OK;
}

int dph_merge_topk_dev(int device, const float* D_parts, const int64_t* I_parts, int n_parts, int64_t part_stride_bytes,
                       int64_t n, int k, float* D_out, int64_t* I_out, int32_t* src_out, void* stream) {
    if (!D_parts || !I_parts || !D_out || !I_out || n_parts <= 0 || n < 0 || k <= 0) return fail(DPH_E_ARG, "dph_merge_topk_dev: bad arguments");
    HIPCHK(hipSetDevice(device));
    if (part_stride_bytes < 0 || (part_stride_bytes % 8) != 0) return fail(DPH_E_ARG, "dph_merge_topk_dev: stride must be a multiple of 8");
    if (n > 0) dph_launch_merge(D_parts, I_parts, nullptr, nullptr, nullptr, nullptr, n_parts, part_stride_bytes, n, k, D_out,
                                I_out, src_out, nullptr, nullptr, nullptr, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return DPH_OK;
}

int dph_merge_records_dev(int device, const float* D_parts, const int64_t* I_parts, const double* best_parts,
                          const int32_t* pred_parts, const int32_t* status_parts, const double* bound_parts, int n_parts,
                          int64_t part_stride_bytes,
                          int64_t n, int k, float* D_out, int64_t* I_out, double* best_out, int32_t* pred_out,
                          int32_t* status_out, void* stream) {
    if (!D_parts || !I_parts || !best_parts || !pred_parts || !status_parts || !D_out || !I_out || !best_out || !pred_out ||
        !status_out || n_parts <= 0 || n < 0 || k <= 0)
        return fail(DPH_E_ARG, "dph_merge_records_dev: bad arguments");
    if (part_stride_bytes < 0 || (part_stride_bytes % 8) != 0) return fail(DPH_E_ARG, "dph_merge_records_dev: stride must be a multiple of 8");
    HIPCHK(hipSetDevice(device));
    if (n > 0) dph_launch_merge(D_parts, I_parts, best_parts, pred_parts, status_parts, bound_parts, n_parts, part_stride_bytes,
                                n, k, D_out, I_out, nullptr, best_out, pred_out, status_out, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return DPH_OK;
}

int dph_profile_enable(dph_index* h, int on) {
    if (!h) return fail(DPH_E_ARG, "null");
    if (h->sh->pq) return dph_pq_profile(h->sh->pq, on);
    HIPCHK(hipSetDevice(h->device));
    h->sc.prof.on = on != 0;
    if (on) HIPCHK(h->sc.prof.warm(256));
    return DPH_OK;
}

int dph_profile_read(dph_index* h, double* scan_ms_total, int* scan_launches) {
    if (!h || !scan_ms_total || !scan_launches) return fail(DPH_E_ARG, "null");
    if (h->sh->pq) return dph_pq_profile_read(h->sh->pq, scan_ms_total, scan_launches);
    HIPCHK(hipSetDevice(h->device));
    int rc = h->sc.prof.drain(h->sc.prof_events_ladder, nullptr, nullptr);
    if (rc) return rc;
    return h->sc.prof.drain(h->sc.prof_events, scan_ms_total, scan_launches);
}

// every bracketed launch since the last read on its own: which = 0 the full scans (PQ index: the coarse filter scans), 1 the ladder levels'
int dph_profile_read_each(dph_index* h, int which, double* ms_out, int cap, int* n_out) {
    if (!h || !n_out || cap < 0 || (cap > 0 && !ms_out)) return fail(DPH_E_ARG, "dph_profile_read_each: bad arguments");
    if (h->sh->pq) return dph_pq_profile_read_each(h->sh->pq, which, ms_out, cap, n_out);
    HIPCHK(hipSetDevice(h->device));
    return h->sc.prof.drain(which ? h->sc.prof_events_ladder : h->sc.prof_events, nullptr, n_out, ms_out, cap);
}

int dph_profile_read_all(dph_index* h, double* scan_ms_total, int* scan_launches, double* ladder_ms_total, int* ladder_launches) {
    if (!h || !scan_ms_total || !scan_launches || !ladder_ms_total || !ladder_launches) return fail(DPH_E_ARG, "null");
    HIPCHK(hipSetDevice(h->device));
    int rc = h->sc.prof.drain(h->sc.prof_events_ladder, ladder_ms_total, ladder_launches);
    if (rc) return rc;
    return h->sc.prof.drain(h->sc.prof_events, scan_ms_total, scan_launches);
}

// what the two scan hooks below share: the query rows copied and quantised, one pass over them (a list-major shard: every tile)
static int debug_scan_pass(dph_index* h, const float* x, int64_t n, hipStream_t st, dph_pass* p) {
    HIPCHK(hipSetDevice(h->device));
    int rc = ensure_scratch(h, n, 0);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(h->sc.q_main.x, x, (size_t)n * DPH_DIM * 4, hipMemcpyHostToDevice, st));
    quantize(h, h->sc.q_main, h->sc.q_main.x, n, nullptr, st);
    *p = make_pass(h, h->sc.q_main, h->sc.q_main.x, 0, (int)n, n > DPH_QROWS ? 2 : 1);
    if (h->sh->row_ids) p->tilemask = h->sh->onesmask;
    return DPH_OK;
}

int dph_debug_scan_buckets(dph_index* h, const float* x, int64_t n, const int32_t* tau_host, int tile_stride,
                           uint64_t* keys_host, uint32_t* counts_host) {
    if (!h || !x || !keys_host || !counts_host || n <= 0 || n > DPH_QROWS * DPH_MAX_QB || tile_stride < 1)
        return fail(DPH_E_ARG, "dph_debug_scan_buckets: bad arguments");
    if (!h->sh->finalized) return fail(DPH_E_STATE, "dph_debug_scan_buckets: call dph_index_finalize first");
    hipStream_t st = nullptr;
    dph_pass p;
    int rc = debug_scan_pass(h, x, n, st, &p);
    if (rc) return rc;
    const int* tau = nullptr;
    if (tau_host) {
        HIPCHK(hipMemcpyAsync(h->sc.tau_dev, tau_host, (size_t)n * 4, hipMemcpyHostToDevice, st));
        tau = h->sc.tau_dev;
    }
    const int64_t tiles = (h->sh->n_tiles + tile_stride - 1) / tile_stride;
    dph_launch_scan(p, tile_stride > 1, tiles, tile_stride, tau, st);
    dph_launch_refine(p, st);
    HIPCHK(hipGetLastError());
    std::vector<dph_pass_counters> cnt(1);
    HIPCHK(hipMemcpyAsync(cnt.data(), p.cnt, sizeof(dph_pass_counters), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int64_t q = 0; q < n; ++q) {
        // bit 31 of the count reports lost pairs (the pair pool ran dry) for that row
        const unsigned c = std::min(cnt[0].bucket_counts[q], (unsigned)DPH_BUCKET_CAP);
        counts_host[q] = c | (cnt[0].overflow[q] ? 0x80000000u : 0u);
        HIPCHK(hipMemcpy(keys_host + q * DPH_BUCKET_CAP, h->sc.buckets + q * DPH_BUCKET_CAP, (size_t)c * 8, hipMemcpyDeviceToHost));
    }
    return DPH_OK;
}

int dph_debug_scan_time(dph_index* h, const float* x, int64_t n, int iters, float* ms_out) {
    if (!h || !x || !ms_out || n <= 0 || n > DPH_QROWS * DPH_MAX_QB || iters <= 0 || iters > 64)
        return fail(DPH_E_ARG, "dph_debug_scan_time: bad arguments");
    if (!h->sh->finalized) return fail(DPH_E_STATE, "dph_debug_scan_time: call dph_index_finalize first");
    if (h->sh->pq) return fail(DPH_E_STATE, "dph_debug_scan_time: a PQ index has no filter scan");
    hipStream_t st = nullptr;
    dph_pass p;
    int rc = debug_scan_pass(h, x, n, st, &p);
    if (rc) return rc;
    // a bound no high-digit score reaches (|H| <= 127 * 128 * 768 < 2^24 = (2^31 - 1 - lmax) >> 7 for any lmax < 2^24): the
    // launch streams and multiplies everything and emits nothing
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)h->sc.tau_dev, 0x7fffffff, (size_t)n, st));
    dph_profiler prof;                  // (of this call alone: one event pair, read back after every launch)
    dph_event_pairs one;
    for (int i = 0; i < iters; ++i) {
        prof.bracket(&one, st, [&] { dph_launch_scan(p, false, h->sh->n_tiles, 1, h->sc.tau_dev, st); });
        double ms = 0.0;
        rc = prof.drain(one, &ms, nullptr);
        if (rc) return rc;
        ms_out[i] = (float)ms;
    }
    HIPCHK(hipGetLastError());
    return DPH_OK;
}

int dph_debug_bucket_counts(dph_index* h, int64_t n, uint32_t* raw_out, uint32_t* overflow_out) {
    if (!h || !raw_out || !overflow_out || n <= 0 || n > DPH_PASS_MAX) return fail(DPH_E_ARG, "dph_debug_bucket_counts: bad arguments");
    if (!h->sc.pass_cnt) return fail(DPH_E_STATE, "dph_debug_bucket_counts: no search yet");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(raw_out, h->sc.pass_cnt.p->bucket_counts, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(overflow_out, h->sc.pass_cnt.p->overflow, (size_t)n * 4, hipMemcpyDeviceToHost));
    return DPH_OK;
}

int dph_debug_pq_coarse(dph_index* h, uint32_t out[2]) {
    if (!h || !out) return fail(DPH_E_ARG, "null");
    if (!h->sh->pq) return fail(DPH_E_STATE, "dph_debug_pq_coarse: not a PQ index");
    return dph_pq_coarse_debug(h->sh->pq, out);
}

int dph_debug_pq_pass(dph_index* h, int32_t info[8], uint32_t* per_row, int n_rows) {
    if (!h || !info || n_rows < 0 || (n_rows > 0 && !per_row)) return fail(DPH_E_ARG, "dph_debug_pq_pass: bad arguments");
    if (!h->sh->pq) return fail(DPH_E_STATE, "dph_debug_pq_pass: not a PQ index");
    return dph_pq_debug_pass(h->sh->pq, info, per_row, n_rows);
}

int dph_debug_pq_phases(dph_index* h, int which, uint64_t* out, int cap_wgs, int* n_wgs) {
    if (!h || !n_wgs || cap_wgs < 0 || which < 0 || which > 1) return fail(DPH_E_ARG, "dph_debug_pq_phases: bad arguments");
    if (!h->sh->pq) return fail(DPH_E_STATE, "dph_debug_pq_phases: not a PQ index");
    const int n = dph_pq_debug_phases(h->sh->pq, which, (unsigned long long*)out, cap_wgs);
    if (n < 0) return fail(DPH_E_HIP, "dph_debug_pq_phases: allocation or copy failed");
    *n_wgs = n;
    return DPH_OK;
}

int dph_debug_lmax(dph_index* h, int64_t n, int32_t* lmax_host) {
    if (!h || !lmax_host || n <= 0 || n > h->sc.cap_rows) return fail(DPH_E_ARG, "dph_debug_lmax: bad arguments");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpy(lmax_host, h->sc.q_main.lmax, (size_t)n * 4, hipMemcpyDeviceToHost));
    return DPH_OK;
}

int dph_debug_aux(dph_index* h, int64_t row0, int64_t n_rows, int8_t* aux_host, int64_t n_q, int8_t* qaux_host, int32_t* info) {
    if (!h || row0 < 0 || n_rows < 0 || n_q < 0) return fail(DPH_E_ARG, "dph_debug_aux: bad arguments");
    const dph_shard* src = h->sh;
    if (!src->finalized) return fail(DPH_E_STATE, "dph_debug_aux: call dph_index_finalize first");
    HIPCHK(hipSetDevice(h->device));
    if (info) { info[0] = src->aux_lay.stride; info[1] = src->norm_unit; info[2] = src->aux_lay.q2max; info[3] = src->aux_lay.n_rep; }
    if (aux_host && n_rows > 0) {
        if (src->aux_lay.stride <= 0 || row0 + n_rows > src->n_tiles * DPH_TILE_ROWS) return fail(DPH_E_ARG, "dph_debug_aux: no aux rows there");
        HIPCHK(hipMemcpy(aux_host, src->aux + row0 * src->aux_lay.stride, (size_t)n_rows * src->aux_lay.stride, hipMemcpyDeviceToHost));
    }
    if (qaux_host && n_q > 0) {
        if (n_q > h->sc.cap_rows) return fail(DPH_E_ARG, "dph_debug_aux: more query rows than the last call quantised");
        HIPCHK(hipMemcpy(qaux_host, h->sc.q_main.qaux, (size_t)n_q * DPH_AUX_SLOTS, hipMemcpyDeviceToHost));
    }
    return DPH_OK;
}
int dph_debug_mu(dph_index* h, int32_t* mu_out) {
    if (!h || !mu_out) return fail(DPH_E_ARG, "dph_debug_mu: null");
    for (int j = 0; j < DPH_DIM; ++j) mu_out[j] = h->sh->mu_host[j];
    return DPH_OK;
}

int64_t dph_debug_fused_tile(int64_t n_tiles, int stride, int64_t v, int64_t* visit_out) {
    unsigned m = 0;
    const int64_t visit = fused_scan_plan(n_tiles, stride, &m);
    if (visit_out) *visit_out = visit;
    if (visit <= 0 || v < 0 || v >= visit) return -1;
    return v + (int64_t)(((uint64_t)v * m) >> 29) + 1;              // dph_scan.hip: tile_of
}

int64_t dph_debug_guided_segment(int64_t u, int64_t n_tiles, int grid, int seg_min, int64_t* len) {
    int64_t l = 0;
    if (u < 0 || n_tiles < 0 || grid <= 0 || seg_min <= 0) { if (len) *len = 0; return -1; }
    const int64_t first = dph_guided_segment(u, n_tiles, grid, seg_min, &l);
    if (len) *len = l;
    return first;
}

int dph_debug_units(dph_index* h, int32_t out[4]) {
    if (!h || !out) return fail(DPH_E_ARG, "dph_debug_units: null");
    if (!h->sc.ivf.unit_cnt) return fail(DPH_E_STATE, "dph_debug_units: no unit scan on this shard");
    HIPCHK(hipSetDevice(h->device));
    dph_unit_counters c;
    HIPCHK(hipMemcpy(&c, h->sc.ivf.unit_cnt, sizeof(c), hipMemcpyDeviceToHost));
    out[0] = c.chunks; out[1] = c.units; out[2] = c.error; out[3] = c.next[DPH_UNIT_LAUNCHES - 1];
    return DPH_OK;
}

int dph_index_shard_stats(dph_index* h, double* rmax, double* rmax_all, int* n_outliers) {
    if (!h || !rmax || !rmax_all || !n_outliers) return fail(DPH_E_ARG, "null");
    *rmax = h->sh->rmax; *rmax_all = h->sh->rmax_all; *n_outliers = h->sh->n_out;
    return DPH_OK;
}

}  // extern "C"
