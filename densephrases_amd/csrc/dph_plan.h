// dph_plan.h -- the host planning rules of libdph: everything that decides how a shard is laid out and how a search is cut into launches
// BEFORE a kernel runs.  Plain host arithmetic, each rule a function from a small struct of facts to a plain result: dph_api.hip and
// dph_pq.hip fill the facts from their handles and act on the result; tests/test_plan.py calls the same functions through
// tests/_plan_shim.cpp.  No HIP header, no handle type: the file compiles with a host compiler alone, and every rule stands here once.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "dph_geometry.h"

// ---------------------------------------------------------------- shard statistics (dph_index_finalize, steps 1 and 2)
// per-dimension mean code mu_j (rounded, clipped to int8) and spread sd_j from sums[0..767] = sum n_j, sums[768..1535] = sum n_j^2
static inline void plan_col_stats(const long long* sums, int64_t n_real, int* mu, double* sd) {
    for (int j = 0; j < DPH_DIM; ++j) {
        const double mean = n_real > 0 ? (double)sums[j] / (double)n_real : 0.0;
        const double var = n_real > 0 ? (double)sums[DPH_DIM + j] / (double)n_real - mean * mean : 0.0;
        int m = (int)lrint(mean);
        mu[j] = m < -128 ? -128 : (m > 127 ? 127 : m);
        sd[j] = var > 0.0 ? sqrt(var) : 0.0;
    }
}

// From the histogram of squared centred row norms (DPH_NORM_BINS bins of DPH_NORM_BIN_W) and the largest one: the median norm, and the
// outlier cut -- the lowest bin edge with at most DPH_OUTLIER_MAX rows at or above it, taken when that tightens the shard-wide norm
// bound by more than 10 % (1.21 = 1.1^2: the histogram holds squares).
struct plan_norms {
    double rmed;                    // median of || n - mu ||_2 (centre of the bin that holds the median row)
    int cut_bin;                    // rows in bins >= cut_bin are above the cut (DPH_NORM_BINS: none)
    unsigned long long cut2;        // norm^2 < cut2 for the rest
    uint64_t above;                 // rows in those bins
    bool take_cut;
};
static inline plan_norms plan_norm_stats(const unsigned* hist, unsigned long long max2) {
    plan_norms r{};
    {
        uint64_t total = 0, run = 0;
        for (int b = 0; b < DPH_NORM_BINS; ++b) total += hist[b];
        r.rmed = 0.0;
        for (int b = 0; b < DPH_NORM_BINS && total > 0; ++b) {
            run += hist[b];
            if (2 * run >= total) { r.rmed = sqrt(((double)b + 0.5) * DPH_NORM_BIN_W); break; }
        }
    }
    r.above = 0;
    r.cut_bin = DPH_NORM_BINS;
    for (int b = DPH_NORM_BINS - 1; b >= 0; --b) {
        if (r.above + hist[b] > (uint64_t)DPH_OUTLIER_MAX) break;
        r.above += hist[b];
        r.cut_bin = b;
    }
    r.cut2 = (unsigned long long)r.cut_bin * DPH_NORM_BIN_W;
    r.take_cut = r.above > 0 && r.cut_bin > 0 && (double)r.cut2 * 1.21 < (double)max2;
    return r;
}

// ---------------------------------------------------------------- aux rows: norm unit, low-digit clamp, layout
// The norm codes of a row sum to ceil(norm / unit) <= 127 n_norm, and the digit they meet, ceil(unit ||q2|| / 128), must fit int8:
// q2max <= 126 * 128 / (unit * sqrt(768)).  A clamp larger than that gives "wrong rows filtered, result still certified".
#define DPH_PLAN_SQRT_DIM 27.7129   // sqrt(768) as the rule has always spelled it: the clamp of every unit depends on these digits
static inline int plan_norm_unit(double rmax_all, int n_norm) {
    const double cap = 127.0 * n_norm;
    const int unit = (int)ceil(rmax_all / cap);
    return unit < 1 ? 1 : unit;
}
static inline int plan_q2_limit(int norm_unit) { return (int)floor(126.0 * 128.0 / ((double)norm_unit * DPH_PLAN_SQRT_DIM)); }
static inline int plan_q2max(int norm_unit) {
    const int q2 = plan_q2_limit(norm_unit);
    return q2 > 64 ? 64 : (q2 < 1 ? 1 : q2);
}

// what the layout of a shard is chosen from: the statistics dph_index_finalize measured and the tuning key "aux"
struct plan_aux_facts {
    int64_t n_rows;
    int aux_mode;                   // -1 = decided here, 0 = never, 4 = norm codes, 16 / 32 = norm codes + 12 / 24 replica slots
    const int* mu; const double* sd;        // [DPH_DIM]
    double rmed, rmax_cut, rmax_all;
    int n_out_found;                // outlier rows finalize found above the cut
};
// Whether the rows are ALIKE.  They are not when (a) some dimensions sit far from the others for every row -- "rogue" dimensions:
// | mu_j - median mu | beyond 3.5 spreads of a typical dimension; a query of the same encoder carries them too and they would eat the
// range of its high digit -- or (b) the norms are heavy-tailed (largest non-outlier norm > 1.3 x the median): then the shard gets AUX
// ROWS (dph_scan.hip "the aux k-step") and the filter bounds every row by its own norm.
static inline dph_aux_layout choose_aux_layout(const plan_aux_facts& s) {
    dph_aux_layout lay{};
    lay.q2max = 64;
    // (a shard the select step sorts whole is scanned cold -- no bound, nothing for aux rows to tighten -- and its handful of rows says
    // little about dimensions)
    if (s.n_rows <= 0 || s.aux_mode == 0 || (s.n_rows <= DPH_POOL_MAX && s.aux_mode < 0)) return lay;
    // rogue dimensions: mean far outside the spread the typical dimension has around the typical mean
    std::vector<double> sds(s.sd, s.sd + DPH_DIM), mus(DPH_DIM);
    for (int j = 0; j < DPH_DIM; ++j) mus[j] = (double)s.mu[j];
    std::nth_element(sds.begin(), sds.begin() + DPH_DIM / 2, sds.end());
    std::nth_element(mus.begin(), mus.begin() + DPH_DIM / 2, mus.end());
    const double sd_med = std::max(1.0, sds[DPH_DIM / 2]), mu_med = mus[DPH_DIM / 2];
    std::vector<std::pair<double, int>> rogue;          // (ratio, dimension): how many times the bulk's range a query needs there
    for (int j = 0; j < DPH_DIM; ++j) {
        const double ratio = fabs((double)s.mu[j] - mu_med) / (3.5 * sd_med);
        if (ratio >= 1.2) rogue.push_back({ratio, j});
    }
    std::sort(rogue.begin(), rogue.end(), [](const std::pair<double, int>& x, const std::pair<double, int>& y) {
        return x.first > y.first || (x.first == y.first && x.second < y.second); });
    if (rogue.size() > 12) rogue.resize(12);            // at least two replica slots each
    const bool heavy = s.rmed > 0.0 && s.rmax_cut > 1.3 * s.rmed;
    // replica slots a query that looks like a row needs: its digit in a rogue dimension is `ratio` times the bulk's range.  Twelve fit the
    // 16-byte aux row (4 norm slots), twenty-four the 32-byte one (8 norm slots); with fewer than it needs a query only loses a little
    // resolution in its bulk (the scale is max_j |q_j| / (1 + R_j)), so the narrow row -- half the extra HBM bytes -- is taken when it suffices
    int need = 0;
    for (auto& r : rogue) need += std::max(1, (int)ceil(r.first) - 1);
    int stride = s.aux_mode > 0 ? s.aux_mode : (!rogue.empty() ? (need <= 12 ? 16 : 32) : (heavy ? 4 : 0));
    if (stride >= 16 && rogue.empty()) stride = 4;
    if (stride == 0) return lay;
    lay.stride = stride;
    lay.n_norm = stride == 32 ? 8 : 4;
    if (stride >= 16) {
        // the replica slots are dealt out in proportion to the ratios (largest remainder), every rogue dimension >= 1
        const int n_slots = stride == 32 ? DPH_AUX_REP_MAX : 12;
        double total = 0;
        for (auto& r : rogue) total += r.first;
        std::vector<int> cnt(rogue.size(), 1);
        int left = n_slots - (int)rogue.size();
        std::vector<double> want(rogue.size());
        for (size_t i = 0; i < rogue.size(); ++i) want[i] = rogue[i].first / total * n_slots;
        while (left > 0) {
            size_t best = 0; double gap = -1e300;
            for (size_t i = 0; i < rogue.size(); ++i) if (want[i] - cnt[i] > gap) { gap = want[i] - cnt[i]; best = i; }
            cnt[best]++; left--;
        }
        int sl = 0;
        for (size_t i = 0; i < rogue.size(); ++i)
            for (int c = 0; c < cnt[i]; ++c) lay.rep_dim[sl++] = (short)rogue[i].second;
        lay.n_rep = sl;
    }
    return lay;
}

// The layout in force on a shard and what follows from it on THAT shard's rows.
struct plan_aux {
    dph_aux_layout lay;
    bool forced;                    // the layout was set from outside (dph_index_set_aux_layout): its clamp is the caller's
    int norm_unit;                  // a norm code counts this many units of || n - mu ||
    int n_out; double rmax;         // outlier rows in force and the largest norm of the others
};
// norm unit and low-digit clamp of a.lay: outlier rows serve the shard-wide norm bound; with aux rows every row is bounded by its own
// norm and none is set aside
static inline void derive_aux_units(const plan_aux_facts& s, plan_aux* a) {
    if (a->lay.stride <= 0) { a->norm_unit = 1; a->n_out = s.n_out_found; a->rmax = s.n_out_found > 0 ? s.rmax_cut : s.rmax_all; return; }
    a->n_out = 0;
    a->rmax = s.rmax_all;
    a->norm_unit = plan_norm_unit(s.rmax_all, a->lay.n_norm);
    if (!a->forced) a->lay.q2max = plan_q2max(a->norm_unit);
}
// Choose unless forced, then derive.  A forced layout (`cur`) survives only while its low-digit clamp still serves THESE rows (new rows
// with larger norms -> a larger norm unit -> the query's norm digit would not fit int8 and the per-row bound would be too small).
// Otherwise the shard chooses afresh and the ranks of a sharded job agree again (densephrases_amd: Shard.finalize resets the sync mark).
static inline plan_aux plan_aux_rows(const plan_aux_facts& s, const dph_aux_layout& cur, bool forced) {
    plan_aux a{};
    a.forced = forced;
    a.lay = forced ? cur : choose_aux_layout(s);
    derive_aux_units(s, &a);
    if (a.forced && a.lay.stride > 0 && a.lay.q2max > plan_q2_limit(a.norm_unit)) {
        a.forced = false;
        a.lay = choose_aux_layout(s);
        derive_aux_units(s, &a);
    }
    return a;
}

// The layout as int32[4 + DPH_AUX_REP_MAX], what the ranks of a sharded job exchange: [0] stride, [1] n_norm, [2] n_rep, [3] q2max,
// [4 .. 4 + DPH_AUX_REP_MAX) rep_dim (-1 behind n_rep).
#define DPH_AUX_LAYOUT_WORDS (4 + DPH_AUX_REP_MAX)
static inline void plan_pack_layout(const dph_aux_layout& lay, int32_t* out) {
    out[0] = lay.stride; out[1] = lay.n_norm; out[2] = lay.n_rep; out[3] = lay.q2max;
    for (int i = 0; i < DPH_AUX_REP_MAX; ++i) out[4 + i] = i < lay.n_rep ? lay.rep_dim[i] : -1;
}
// 0 = a layout plan_pack_layout writes, 1 = not one (shape or clamp), 2 = a replica dimension out of range
static inline int plan_unpack_layout(const int32_t* in, dph_aux_layout* out) {
    dph_aux_layout lay{};
    lay.stride = in[0]; lay.n_norm = in[1]; lay.n_rep = in[2]; lay.q2max = in[3];
    const bool ok_shape = (lay.stride == 0 && lay.n_norm == 0 && lay.n_rep == 0) || (lay.stride == 4 && lay.n_norm == 4 && lay.n_rep == 0) ||
                          (lay.stride == 16 && lay.n_norm == 4 && lay.n_rep >= 0 && lay.n_rep <= 12) ||
                          (lay.stride == 32 && lay.n_norm == 8 && lay.n_rep >= 0 && lay.n_rep <= DPH_AUX_REP_MAX);
    if (!ok_shape || lay.q2max < 1 || lay.q2max > 64) return 1;
    for (int i = 0; i < lay.n_rep; ++i) {
        if (in[4 + i] < 0 || in[4 + i] >= DPH_DIM) return 2;
        lay.rep_dim[i] = (short)in[4 + i];
    }
    *out = lay;
    return 0;
}

// ---------------------------------------------------------------- the pre-pass ladder
struct plan_ladder_facts {
    int64_t n_tiles, n_rows;
    int grid;                       // scan workgroups
    int fine_stride;                // tuning key: 0 = default
    const int* ladder; int n_ladder;        // tuning key "ladder": explicit strides, coarse -> fine (n_ladder = 0: derived)
};
// The pre-pass ladder: strides of the sampled levels, coarse -> fine.  Every level scans each `stride`-th tile under
// the bound of the previous one; the first runs cold (no bound: every sampled row is emitted), so it must be small
// enough for the pair pool (the scan waves' fair share of it) and the buckets -- and a shard small enough for ITS full
// scan to run cold needs no ladder at all.  The bound of the last level is what the full scan runs under: ~ kp * stride
// rows per query row beat it whatever the shard size (plus ~2x as many that only pass the high-digit test).
static inline void build_ladder(const plan_ladder_facts& h, int qb, std::vector<int>& out) {
    out.clear();
    const int64_t nt = h.n_tiles;
    if (h.n_ladder > 0) {
        for (int i = 0; i < h.n_ladder; ++i) { const int v = h.ladder[i]; if (v > 1 && (nt + v - 1) / v >= 1) out.push_back(v); }
        return;
    }
    if (nt * DPH_TILE_ROWS <= DPH_POOL_MAX) return;             // every row fits the select pool: scan cold
    // tiles a cold level may visit: the pair regions of the scan waves and the buckets must hold every sampled row.  The
    // aim is ONE tile per scan workgroup: balanced, and the refine step of that level scores every (row, query) pair
    const int64_t wave_share = (int64_t)DPH_POOL_CHUNKS * DPH_CHUNK_PAIRS / ((int64_t)h.grid * 4);
    const int64_t per_wg = wave_share / (DPH_TILE_ROWS * DPH_QGROUP * qb);
    const int64_t cold_max = std::min<int64_t>((int64_t)h.grid * per_wg / 2, DPH_BUCKET_CAP / DPH_TILE_ROWS - 64);
    const int64_t cold_aim = std::min<int64_t>(h.grid, cold_max);
    const bool big = h.n_rows >= 100000000ll;
    const int fine = h.fine_stride > 0 ? h.fine_stride : (big ? 32 : 16);
    const int ratio = big ? 16 : 8;
    const int64_t s0 = std::max<int64_t>(2, (nt + cold_aim - 1) / cold_aim);          // stride that visits ~cold_aim tiles
    std::vector<int64_t> up;             // fine -> coarse
    int64_t s = std::max<int64_t>(2, fine);
    while ((nt + s - 1) / s > cold_max) {
        up.push_back(s);
        int64_t next = s * ratio;
        if ((nt + next - 1) / next < cold_aim) next = std::max<int64_t>(s0, s + 1);   // do not overshoot the cold level
        s = next;
    }
    // s can run cold; the top level visits ~cold_aim tiles (if that sits too close above the level below, it replaces it)
    if ((nt + s - 1) / s > cold_aim && s0 > s) { if (s0 >= s * 4) up.push_back(s); s = s0; }
    if (!up.empty() && s < up.back() * 4) up.back() = s;
    else up.push_back(s);
    for (size_t i = up.size(); i-- > 0;) out.push_back((int)std::min<int64_t>(up[i], 1 << 30));
}

// One ladder level of a pass: flat / masked scans visit every stride-th tile of the shard; the unit scan visits the
// tiles of every probed list whose index INSIDE the list is a multiple of the stride, and its cold level (stride =
// longest list: tile 0 of every probed list) emits only the rows `rowmask` names, so that the cold sample of
// DPH_PASS_MAX rows x nprobe lists fits the pair regions.
struct ladder_level { int stride; unsigned rowmask; };

// the lists of a list-major shard as the unit scan sees them
struct plan_list_facts {
    int64_t n_rows, n_tiles;        // stored rows (list padding included) and their tiles
    int nlist;
    bool lists_contiguous;          // every list is one contiguous run of tiles
    int max_list_tiles; int64_t total_segs;         // longest list in tiles; segments of DPH_UNIT_TILES tiles over all lists
};
static inline void build_ladder_units(const plan_list_facts& h, int fine_stride, int n_q, int nprobe, std::vector<ladder_level>& out,
                                      double* last_ratio) {
    out.clear();
    const int64_t np = std::min<int64_t>(nprobe, h.nlist);
    const int64_t probed = np * (h.n_rows / std::max(1, h.nlist));        // rows a query row scores (average)
    *last_ratio = 1.0;
    // small enough to run cold (every row of every probed list is emitted): a scan wave emits 1024 pairs per tile of a
    // unit with full slot groups, so only shards of one- or two-tile lists qualify
    if (h.max_list_tiles <= 2 && (int64_t)n_q * probed <= (1 << 19) && probed <= DPH_POOL_MAX / 2) return;
    int r = 32;                                                               // rows of a tile the cold level samples
    while (r > 2 && (int64_t)n_q * np * r > (1 << 19)) r >>= 1;            // ~0.2 us of refine per 1000 pairs
    const int64_t s0 = np * r;
    const int fine = fine_stride > 0 ? fine_stride : 32;
    std::vector<int> up;                                                      // fine -> coarse
    for (int64_t s = std::max(2, fine); s < h.max_list_tiles && probed / s >= 4 * s0; s *= 16) up.push_back((int)s);
    out.push_back({std::max(1, h.max_list_tiles), (1u << (r / 2)) - 1u});
    for (size_t i = up.size(); i-- > 0;) out.push_back({up[i], 0xFFFFu});
    *last_ratio = up.empty() ? std::max(1.0, (double)probed / (double)s0) : (double)up[0];
}

// candidates the select step re-scores: max(k + 32, 2 k) on the first attempt, all it can hold on a retry pass
static inline int plan_select_C(int k, bool retry) { return retry ? DPH_SELECT_C_MAX : std::min(std::max(k + 32, 2 * k), DPH_SELECT_C_MAX); }
// the bound of a level is its kp-th best sampled score: ~kp * last_ratio rows beat it in the full scan (last_ratio: rows of the shard --
// of the probed lists -- per row of the last level's sample), and that must cover the C candidates the select step wants to re-score
static inline int plan_kp(int sample_kp, bool has_levels, int C, double last_ratio) {
    int kp = sample_kp;
    if (has_levels) kp = std::max(kp, (int)((double)C * 1.5 / last_ratio) + 8);
    return kp;
}
// every scan launch of a pass (the ladder levels + the full scan) pops a work-queue head of its own
static inline bool plan_ladder_fits(size_t n_levels) { return (int)n_levels + 1 <= DPH_UNIT_LAUNCHES; }

// The full scan behind a FUSED finest ladder level of stride S (pass_scan_select): that level scanned tiles 0, S, 2S, ...; the full scan
// visits the other `visit` tiles, visited index v -> tile v + v / (S - 1) + 1, and the kernel takes the quotient as
// (v * m) >> 29 with m = ceil(2^29 / (S - 1)) (dph_scan.hip, tile_of).  With err = m (S - 1) - 2^29 that is exact as long as
// v * err < 2^29 (the fraction the multiply adds stays below 1 / (S - 1)).  Returns the number of tiles to visit and the
// multiplier, or 0 when the scan is not to be fused (no bounded level, a shard of a few tiles, a multiply that would not be
// exact or would overflow).
static inline int64_t fused_scan_plan(int64_t n_tiles, int stride, unsigned* m_out) {
    if (stride < 2 || n_tiles <= 4 * (int64_t)stride) return 0;
    const unsigned d = (unsigned)stride - 1u;
    const unsigned m = (unsigned)(((1ull << 29) + d - 1) / d);
    const uint64_t err = (uint64_t)m * d - (1ull << 29);
    const int64_t visit = n_tiles - (n_tiles + stride - 1) / stride;
    if ((uint64_t)visit * (err ? err : 1) >= (1ull << 29) || (uint64_t)visit * m >= (1ull << 62)) return 0;
    *m_out = m;
    return visit;
}

// the next pass of a call with `left` rows to go: 256 rows (qb = 2) while at least 129 are left, else 128; a unit pass serves up to
// DPH_PASS_MAX.  Returns its rows.
static inline int plan_pass_rows(int64_t left, bool units, int max_qb, int* qb_out) {
    const int qb = units ? 1 : ((left > DPH_QROWS && max_qb >= 2) ? 2 : 1);
    *qb_out = qb;
    return (int)std::min<int64_t>(left, units ? (int64_t)DPH_PASS_MAX : (int64_t)DPH_QROWS * qb);
}

// ---------------------------------------------------------------- unit scan of a list-major shard (dph_geometry.h: DPH_PASS_MAX)
// list geometry from the tile -> list table: the unit scan needs every list to be one contiguous run of tiles (what
// ivf.build_list_major writes); tile0 [nlist + 1] = first tile of every list (zeros when the lists are not contiguous)
static inline plan_list_facts plan_list_geometry(const int32_t* tile_list, int64_t n_rows, int64_t n_tiles, int nlist, std::vector<int>& tile0) {
    plan_list_facts g{};
    g.n_rows = n_rows; g.n_tiles = n_tiles; g.nlist = nlist;
    tile0.assign((size_t)nlist + 1, 0);
    g.lists_contiguous = nlist <= 65536 && n_tiles < (int64_t)0x7fffffff;
    for (int64_t t = 1; t < n_tiles && g.lists_contiguous; ++t) if (tile_list[t] < tile_list[t - 1]) g.lists_contiguous = false;
    g.max_list_tiles = 0; g.total_segs = 0;
    if (g.lists_contiguous) {
        std::vector<int> cnt((size_t)nlist, 0);
        for (int64_t t = 0; t < n_tiles; ++t) cnt[(size_t)tile_list[t]]++;
        for (int l = 0; l < nlist; ++l) {
            tile0[(size_t)l + 1] = tile0[(size_t)l] + cnt[(size_t)l];
            g.max_list_tiles = std::max(g.max_list_tiles, cnt[(size_t)l]);
            g.total_segs += (cnt[(size_t)l] + DPH_UNIT_TILES - 1) / DPH_UNIT_TILES;
        }
    }
    return g;
}
// Worth it when the lists are long: a unit pays a few microseconds of start-up (pop the queue, load its query fragments,
// fill the pipeline) against ~1 us per 10 tiles of streaming.  Shards with many short lists (the reference's 2^20 lists)
// keep the masked scan.  (list_major: the shard has row ids; ivf_units: the tuning key, -1 = decided here.)
static inline bool use_units(const plan_list_facts& h, bool list_major, int ivf_units, int nprobe) {
    if (!list_major || nprobe <= 0 || !h.lists_contiguous || ivf_units == 0) return false;
    return ivf_units == 1 || h.n_tiles / std::max(1, h.nlist) >= 64;
}
// capacity of the work queue of a pass: DPH_PASS_MAX rows x nprobe lists give at most that many (row, list) probes; a list probed by
// r rows is ceil(r / DPH_UNIT_SLOTS) chunks -- one per probed list plus one per DPH_UNIT_SLOTS probes -- and every chunk one unit per
// segment of its list
struct plan_unit_caps { int64_t chunk_cap, unit_cap; bool too_large; };
static inline plan_unit_caps plan_unit_queue(const plan_list_facts& h, int nprobe) {
    const int64_t np = std::min<int64_t>(nprobe, h.nlist);
    const int64_t probes = (int64_t)DPH_PASS_MAX * np;                       // (query row, list) pairs of a pass
    const int64_t extra = probes / DPH_UNIT_SLOTS + 1;                       // chunks beyond the first of a list
    const int64_t segs_max = (h.max_list_tiles + DPH_UNIT_TILES - 1) / DPH_UNIT_TILES;
    plan_unit_caps c{};
    c.chunk_cap = std::min<int64_t>(h.nlist, probes) + extra;
    c.unit_cap = h.total_segs + extra * std::max<int64_t>(1, segs_max);
    c.too_large = c.chunk_cap > (1 << 22) || c.unit_cap > (1 << 26);
    return c;
}

// ---------------------------------------------------------------- the ADC scans of the PQ index (dph_pq.hip)
struct plan_pq_facts {
    int M; int64_t ntotal; int nlist;
    int64_t max_list;               // codes of the longest list
    const int64_t* top_prefix;      // [nlist + 1], plan_pq_top_prefix
};
// [i] = codes in the i longest lists: what a row can meet at most with nprobe = i
static inline void plan_pq_top_prefix(const int64_t* sizes, int nlist, std::vector<int64_t>& out) {
    std::vector<int64_t> srt(sizes, sizes + nlist);
    std::sort(srt.begin(), srt.end(), [](int64_t x, int64_t y) { return x > y; });
    out.assign((size_t)nlist + 1, 0);
    for (int l = 0; l < nlist; ++l) out[(size_t)l + 1] = out[(size_t)l] + srt[(size_t)l];
}
static constexpr int pq_seg(int M) { return M <= 96 ? PQ_SEG : PQ_SEG / 2; }
// many short lists ON AVERAGE: the work is grouped by query row (pq_adc_rows_kernel) and cut by code count, so a list hundreds of times
// the mean is several units of several workgroups.  (A group's 64 lists are one sequence indexed with 32-bit ints: 2^24 codes per list.)
static inline bool pq_by_rows(const plan_pq_facts& p) { return p.ntotal / p.nlist < 2048 && p.max_list < ((int64_t)1 << 24); }
// codes a query row can meet at most: those of its nprobe LONGEST lists, not nprobe x the longest (dph_pq_set_list_sizes fills the
// prefix sums, and no index is searched without it)
static inline int64_t pq_row_codes_max(const plan_pq_facts& p, int nprobe) { return p.top_prefix[(size_t)std::min(nprobe, p.nlist)]; }
// units / segments a query row can meet at most: one (partial) segment per group + the codes of its nprobe longest lists cut into segments
static inline int64_t pq_row_units_max(const plan_pq_facts& p, int nprobe) {
    return (nprobe + PQ_GROUP - 1) / PQ_GROUP + pq_row_codes_max(p, nprobe) / pq_seg(p.M) + 1;
}
// dynamic LDS of the ADC scans: the row's tables [M][256], the keys of a segment, histogram, wave partials, the queue item
static constexpr size_t pq_lds_bytes(int M) { return (size_t)M * 1024 + (size_t)pq_seg(M) * 4 + 264 * 4 + 16 * 8 + 16; }
// ... and the most any M that dph_pq_alloc accepts asks for: the allowance is granted once per kernel and device, whatever the handle
static constexpr size_t pq_lds_bytes_max() {
    size_t mx = 0;
    for (int M = 16; M <= 128; M += 16) if (DPH_DIM % M == 0 && pq_lds_bytes(M) > mx) mx = pq_lds_bytes(M);
    return mx;
}
static_assert(pq_lds_bytes_max() <= 160 * 1024, "the ADC scans' tables and keys must fit the 160 KiB of LDS of a CU");
// candidates a segment may append: its k best -- or, in the row-major scan (pq_segment_finish<true>: the bound of a long segment is the
// k-th of a 1024-key sample), about k * seg / 1024 keys: twice that is reserved.  (The scratch serves every later call with k' <= k
// without a new allocation: the sampled rule's share for min(k, 128) counts even when THIS k is beyond it.)
static inline int64_t pq_per_seg(bool by_rows, int M, int k) {
    return by_rows ? std::max<int64_t>(k, (int64_t)std::min(k, PQ_THREADS / 8) * (pq_seg(M) / PQ_THREADS) * 2) : k;
}
// + the count above the k-th of a 1-in-12 sample has a geometric tail -- for k = 1, P(more than m) = (11/12)^m: m = 64 was crossed once
// in 4000 cold segments, 512 once in 10^19
#define PQ_SAMPLE_TAIL 512
// capacities of a pass of `rows` query rows: candidates per row; pair records (list-major scan) and unit records (row-major scan) per pass
struct plan_pq_caps { int cand_cap, pair_cap, unit_cap; };
static inline plan_pq_caps plan_pq_scan(const plan_pq_facts& p, int rows, int k, int nprobe) {
    const bool by_rows = pq_by_rows(p);
    const int64_t per_seg = pq_per_seg(by_rows, p.M, k);
    // segments a row can meet: row-major, (partial) segments of its groups; list-major, every probed list on its own
    const int64_t codes_row = pq_row_codes_max(p, nprobe);
    const int64_t segs_row = by_rows ? pq_row_units_max(p, nprobe) : (int64_t)nprobe + codes_row / pq_seg(p.M);
    int64_t cap = segs_row * per_seg + PQ_SAMPLE_TAIL;
    const int64_t budget = ((int64_t)2 << 30) / 8 / rows;                // at most 2 GiB of candidates per pass
    cap = std::max<int64_t>(std::min(cap, budget), 4 * (int64_t)k + 64);
    plan_pq_caps c{};
    c.cand_cap = (int)std::min<int64_t>(cap, 1 << 30);
    // list-major pairs: one per chunk of PQ_LM_CHUNK segments of a probed list -- at most nprobe + (codes of the nprobe longest lists) / chunk per row
    c.pair_cap = (int)std::min<int64_t>((int64_t)rows * (nprobe + (by_rows ? 0 : codes_row / ((int64_t)pq_seg(p.M) * PQ_LM_CHUNK))), 1 << 28);
    c.unit_cap = by_rows ? (int)std::min<int64_t>((int64_t)rows * pq_row_units_max(p, nprobe), 1 << 28) : 0;
    return c;
}
