// tests/_plan_shim.cpp -- extern "C" wrappers over densephrases_amd/csrc/dph_plan.h, flat arrays in and out: what tests/_plan.py
// compiles with a plain host compiler and loads with ctypes.  (That it compiles that way is the proof that the header needs no HIP.)
// With -DPLAN_SHIM_MAIN it is a stand-alone program that sweeps the rules over a fixed grid: the form a sanitizer build runs.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../densephrases_amd/csrc/dph_plan.h"

static plan_list_facts list_facts_of(const int64_t* f) { return plan_list_facts{f[0], f[1], (int)f[2], f[3] != 0, (int)f[4], f[5]}; }
static plan_aux_facts aux_facts_of(int64_t n_rows, int aux_mode, const int* mu, const double* sd, const double* norms, int n_out_found) {
    return plan_aux_facts{n_rows, aux_mode, mu, sd, norms[0], norms[1], norms[2], n_out_found};
}

extern "C" {

// the constants the properties are stated from, in the order tests/_plan.py names them
int shim_constants(int64_t* out, int cap) {
    const int64_t v[] = {DPH_DIM, DPH_TILE_ROWS, DPH_QGROUP, DPH_QROWS, DPH_MAX_QB, DPH_CHUNK_PAIRS, DPH_POOL_CHUNKS, DPH_BUCKET_CAP, DPH_POOL_MAX,
                         DPH_SELECT_C_MAX, DPH_PASS_MAX, DPH_UNIT_TILES, DPH_UNIT_SLOTS, DPH_UNIT_LAUNCHES, DPH_NORM_BINS, DPH_NORM_BIN_W,
                         DPH_OUTLIER_MAX, DPH_AUX_REP_MAX, DPH_AUX_LAYOUT_WORDS, PQ_THREADS, PQ_SEG, PQ_GROUP, PQ_LM_CHUNK, PQ_FINAL_CAP,
                         PQ_SAMPLE_TAIL};
    const int n = (int)(sizeof(v) / sizeof(v[0]));
    for (int i = 0; i < n && i < cap; ++i) out[i] = v[i];
    return n;
}

void shim_col_stats(const long long* sums, int64_t n_real, int* mu, double* sd) { plan_col_stats(sums, n_real, mu, sd); }

// out: cut_bin, cut2, above, take_cut
void shim_norm_stats(const unsigned* hist, unsigned long long max2, double* rmed, int64_t* out) {
    const plan_norms r = plan_norm_stats(hist, max2);
    *rmed = r.rmed;
    out[0] = r.cut_bin; out[1] = (int64_t)r.cut2; out[2] = (int64_t)r.above; out[3] = r.take_cut;
}

int shim_norm_unit(double rmax_all, int n_norm) { return plan_norm_unit(rmax_all, n_norm); }
int shim_q2_limit(int unit) { return plan_q2_limit(unit); }
int shim_q2max(int unit) { return plan_q2max(unit); }

// norms = {rmed, rmax_cut, rmax_all}
void shim_choose_layout(int64_t n_rows, int aux_mode, const int* mu, const double* sd, const double* norms, int32_t* lay_out) {
    plan_pack_layout(choose_aux_layout(aux_facts_of(n_rows, aux_mode, mu, sd, norms, 0)), lay_out);
}
// cur: the layout in force (NULL: none), forced: it was set from outside.  info: forced, norm_unit, n_out; rmax
int shim_aux_rows(int64_t n_rows, int aux_mode, const int* mu, const double* sd, const double* norms, int n_out_found, const int32_t* cur,
                  int forced, int32_t* lay_out, int* info, double* rmax) {
    dph_aux_layout lay{};
    lay.q2max = 64;
    if (cur) { const int bad = plan_unpack_layout(cur, &lay); if (bad) return bad; }
    const plan_aux a = plan_aux_rows(aux_facts_of(n_rows, aux_mode, mu, sd, norms, n_out_found), lay, forced != 0);
    plan_pack_layout(a.lay, lay_out);
    info[0] = a.forced; info[1] = a.norm_unit; info[2] = a.n_out;
    *rmax = a.rmax;
    return 0;
}
// unpack, then pack again: the validator's verdict, and -- when it is 0 -- the same words in `out`
int shim_layout_roundtrip(const int32_t* in, int32_t* out) {
    dph_aux_layout lay{};
    const int bad = plan_unpack_layout(in, &lay);
    if (!bad) plan_pack_layout(lay, out);
    return bad;
}

int shim_ladder(int64_t n_tiles, int64_t n_rows, int grid, int fine_stride, const int* ladder, int n_ladder, int qb, int* out, int cap) {
    std::vector<int> v;
    build_ladder(plan_ladder_facts{n_tiles, n_rows, grid, fine_stride, ladder, n_ladder}, qb, v);
    for (size_t i = 0; i < v.size() && (int)i < cap; ++i) out[i] = v[i];
    return (int)v.size();
}
// lists = {n_rows, n_tiles, nlist, lists_contiguous, max_list_tiles, total_segs}
int shim_ladder_units(const int64_t* lists, int fine_stride, int n_q, int nprobe, int* strides, unsigned* rowmasks, int cap, double* last_ratio) {
    std::vector<ladder_level> v;
    build_ladder_units(list_facts_of(lists), fine_stride, n_q, nprobe, v, last_ratio);
    for (size_t i = 0; i < v.size() && (int)i < cap; ++i) { strides[i] = v[i].stride; rowmasks[i] = v[i].rowmask; }
    return (int)v.size();
}
int shim_select_C(int k, int retry) { return plan_select_C(k, retry != 0); }
int shim_kp(int sample_kp, int has_levels, int C, double last_ratio) { return plan_kp(sample_kp, has_levels != 0, C, last_ratio); }
int shim_ladder_fits(int n_levels) { return plan_ladder_fits((size_t)n_levels); }
int64_t shim_fused_scan(int64_t n_tiles, int stride, unsigned* m_out) { *m_out = 0; return fused_scan_plan(n_tiles, stride, m_out); }
int shim_pass_rows(int64_t left, int units, int max_qb, int* qb_out) { return plan_pass_rows(left, units != 0, max_qb, qb_out); }

// tile0: [nlist + 1]; lists_out as above
void shim_list_geometry(const int32_t* tile_list, int64_t n_rows, int64_t n_tiles, int nlist, int* tile0, int64_t* lists_out) {
    std::vector<int> t0;
    const plan_list_facts g = plan_list_geometry(tile_list, n_rows, n_tiles, nlist, t0);
    for (size_t i = 0; i < t0.size(); ++i) tile0[i] = t0[i];
    lists_out[0] = g.n_rows; lists_out[1] = g.n_tiles; lists_out[2] = g.nlist; lists_out[3] = g.lists_contiguous; lists_out[4] = g.max_list_tiles;
    lists_out[5] = g.total_segs;
}
int shim_use_units(const int64_t* lists, int list_major, int ivf_units, int nprobe) { return use_units(list_facts_of(lists), list_major != 0, ivf_units, nprobe); }
// out: chunk_cap, unit_cap, too_large
void shim_unit_queue(const int64_t* lists, int nprobe, int64_t* out) {
    const plan_unit_caps c = plan_unit_queue(list_facts_of(lists), nprobe);
    out[0] = c.chunk_cap; out[1] = c.unit_cap; out[2] = c.too_large;
}

void shim_pq_top_prefix(const int64_t* sizes, int nlist, int64_t* out) {
    std::vector<int64_t> v;
    plan_pq_top_prefix(sizes, nlist, v);
    for (size_t i = 0; i < v.size(); ++i) out[i] = v[i];
}
// out: seg, by_rows, row_codes_max, row_units_max, lds_bytes, lds_bytes_max, per_seg, cand_cap, pair_cap, unit_cap
void shim_pq_scan(int M, int64_t ntotal, int nlist, int64_t max_list, const int64_t* top_prefix, int rows, int k, int nprobe, int64_t* out) {
    const plan_pq_facts f{M, ntotal, nlist, max_list, top_prefix};
    const plan_pq_caps c = plan_pq_scan(f, rows, k, nprobe);
    out[0] = pq_seg(M); out[1] = pq_by_rows(f); out[2] = pq_row_codes_max(f, nprobe); out[3] = pq_row_units_max(f, nprobe);
    out[4] = (int64_t)pq_lds_bytes(M); out[5] = (int64_t)pq_lds_bytes_max(); out[6] = pq_per_seg(pq_by_rows(f), M, k);
    out[7] = c.cand_cap; out[8] = c.pair_cap; out[9] = c.unit_cap;
}

}  // extern "C"

#ifdef PLAN_SHIM_MAIN
// The grid of tests/golden/plan_rules.json (tools/make_golden_plan.py), with synthetic statistics where that one reads shards: every rule
// runs, a checksum of what it returned is printed.  Built with -fsanitize=address,undefined this is the one-off check of the header.
static uint64_t g_sum = 0, g_calls = 0;
static void note(int64_t v) { g_sum = g_sum * 1099511628211ull + (uint64_t)v; ++g_calls; }
static uint64_t g_rng = 88172645463325252ull;
static uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }

int main() {
    const int64_t rows[] = {8192, 8224, 300000, 2000000, 170000000, 375000000};
    const int grids[] = {64, 256, 304}, fines[] = {0, 16, 64}, ks[] = {1, 10, 100, 1024}, nprobes[] = {1, 16, 64, 256};
    const int explicit_ladder[] = {4096, 256, 16};
    int buf[64]; unsigned masks[64];
    for (int64_t n : rows) for (int grid : grids) for (int qb = 1; qb <= 2; ++qb) for (int fine : fines) for (int ex = 0; ex < 2; ++ex) {
        const int64_t nt = (n + DPH_TILE_ROWS - 1) / DPH_TILE_ROWS;
        const int nl = shim_ladder(nt, n, grid, fine, explicit_ladder, ex ? 3 : 0, qb, buf, 64);
        note(nl);
        for (int i = 0; i < nl; ++i) { note(buf[i]); unsigned m = 0; note(shim_fused_scan(nt, buf[i], &m)); note(m); }
        for (int k : ks) for (int retry = 0; retry < 2; ++retry)
            note(shim_kp(16, nl > 0, shim_select_C(k, retry), nl ? (double)buf[nl - 1] : 1.0));
        note(shim_ladder_fits(nl));
    }
    for (int64_t left : {1, 64, 128, 129, 200, 256, 300, 700, 1024, 5000}) for (int u = 0; u < 2; ++u) for (int mq = 1; mq <= 2; ++mq) {
        int qb = 0; note(shim_pass_rows(left, u, mq, &qb)); note(qb);
    }
    for (int unit = 1; unit <= 64; ++unit) { note(shim_q2_limit(unit)); note(shim_q2max(unit)); }
    for (double r = 0.0; r < 7100.0; r += 37.5) { note(shim_norm_unit(r, 4)); note(shim_norm_unit(r, 8)); }
    // statistics: random sums and histograms, every aux mode, forced layouts that stop serving the rows
    std::vector<long long> sums(2 * DPH_DIM);
    std::vector<int> mu(DPH_DIM); std::vector<double> sd(DPH_DIM);
    std::vector<unsigned> hist(DPH_NORM_BINS);
    for (int trial = 0; trial < 40; ++trial) {
        const int64_t n = 20000;
        for (int j = 0; j < DPH_DIM; ++j) {
            const long long mean = (long long)(rnd() % 60) + 10 + ((trial & 1) && j % 97 == 0 ? (long long)(rnd() % 80) : 0);
            const long long spread = 4 + (long long)(rnd() % 12);
            sums[j] = mean * n; sums[DPH_DIM + j] = (mean * mean + spread * spread) * n;
        }
        shim_col_stats(sums.data(), n, mu.data(), sd.data());
        for (int j = 0; j < DPH_DIM; ++j) { note(mu[j]); note((int64_t)(sd[j] * 1024)); }
        for (auto& h : hist) h = 0;
        const int centre = 20 + (int)(rnd() % 60);
        for (int64_t i = 0; i < n; ++i) hist[(size_t)(centre + rnd() % 16 + (rnd() % 64 == 0 ? rnd() % 900 : 0))]++;
        int top = DPH_NORM_BINS - 1;
        while (top > 0 && !hist[(size_t)top]) --top;
        const unsigned long long max2 = (unsigned long long)(top + 1) * DPH_NORM_BIN_W - 1;
        double rmed = 0; int64_t o[4];
        shim_norm_stats(hist.data(), max2, &rmed, o);
        for (int64_t v : o) note(v);
        const double norms[3] = {rmed, o[3] ? sqrt((double)o[1]) : sqrt((double)max2), sqrt((double)max2)};
        for (int mode : {-1, 0, 4, 16, 32}) {
            int32_t lay[DPH_AUX_LAYOUT_WORDS], lay2[DPH_AUX_LAYOUT_WORDS]; int info[3]; double rmax = 0;
            shim_aux_rows(n, mode, mu.data(), sd.data(), norms, o[3] ? (int)o[2] : 0, nullptr, 0, lay, info, &rmax);
            for (int32_t v : lay) note(v);
            note(shim_layout_roundtrip(lay, lay2));
            lay[3] = 64;                                     // forced with the widest clamp, and rows whose norms outgrew it
            const double big[3] = {norms[0], norms[1] * 40, norms[2] * 40};
            note(shim_aux_rows(n, mode, mu.data(), sd.data(), big, 0, lay, 1, lay2, info, &rmax));
            note(info[0]); note(info[1]);
        }
    }
    // lists: uniform, zipf, one giant list
    for (int nlist : {64, 4096, 65536}) for (int shape = 0; shape < 3; ++shape) {
        std::vector<int64_t> sizes((size_t)nlist);
        for (int l = 0; l < nlist; ++l) sizes[(size_t)l] = shape == 0 ? 1000 : shape == 1 ? 4000000 / (l + 1) : (l == nlist / 3 ? 600000 : 100);
        std::vector<int32_t> tiles;
        int64_t total = 0, mx = 0;
        for (int l = 0; l < nlist; ++l) {
            total += sizes[(size_t)l]; mx = std::max(mx, sizes[(size_t)l]);
            tiles.insert(tiles.end(), (size_t)((sizes[(size_t)l] + DPH_TILE_ROWS - 1) / DPH_TILE_ROWS), l);
        }
        std::vector<int> tile0((size_t)nlist + 1);
        int64_t lists[6];
        shim_list_geometry(tiles.data(), (int64_t)tiles.size() * DPH_TILE_ROWS, (int64_t)tiles.size(), nlist, tile0.data(), lists);
        for (int64_t v : lists) note(v);
        std::vector<int64_t> prefix((size_t)nlist + 1);
        shim_pq_top_prefix(sizes.data(), nlist, prefix.data());
        for (int np : nprobes) {
            int64_t o[10];
            note(shim_use_units(lists, 1, -1, np));
            shim_unit_queue(lists, np, o); note(o[0]); note(o[1]); note(o[2]);
            double lr = 0;
            for (int nq : {64, 700, 1024}) { const int nl = shim_ladder_units(lists, 0, nq, np, buf, masks, 64, &lr); note(nl); for (int i = 0; i < nl; ++i) { note(buf[i]); note(masks[i]); } }
            for (int M : {48, 64, 96, 128}) for (int k : ks) { shim_pq_scan(M, total, nlist, mx, prefix.data(), 1024, k, np, o); for (int64_t v : o) note(v); }
        }
    }
    printf("plan shim sweep: %llu values, checksum %016llx\n", (unsigned long long)g_calls, (unsigned long long)g_sum);
    return 0;
}
#endif
