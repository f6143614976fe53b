"""CPU-only: the host planning rules of densephrases_amd/csrc/dph_plan.h, called through tests/_plan_shim.cpp (tests/_plan.py builds it
with a plain g++: the header needs no HIP).  A recorded table holds every rule over a fixed grid exactly; the properties below say what
the kernels rely on without restating the rules."""
import json

import numpy as np

from tests import _plan as P

K = P.constants()


# ------------------------------------------------------------------------------------------------------------------ 4.1 the table
def test_every_rule_matches_the_recorded_table():
    """tests/golden/plan_rules.json (tools/make_golden_plan.py) against the rules as they stand: exact, section by section."""
    with open(P.GOLDEN) as f:
        want = json.load(f)
    got = json.loads(json.dumps(P.table()))
    assert sorted(got) == sorted(want)
    for section in want:
        if isinstance(want[section], list) and len(want[section]) == len(got[section]):
            for a, b in zip(want[section], got[section]):
                assert a == b, (section, a, b)
        assert got[section] == want[section], section


# ------------------------------------------------------------------------------------------------------------------ 4.2 ladder
def _flat_points():
    for n in P.ROWS + (8193, 40_000, 1_000_003, 21_000_000, 99_999_999, 100_000_000):
        for grid in P.GRIDS:
            for qb in (1, 2):
                for fine in P.FINES:
                    yield n, (n + K["TILE_ROWS"] - 1) // K["TILE_ROWS"], grid, qb, fine


def test_ladder_strides_fall_and_the_cold_level_fits_the_pool_and_the_buckets():
    pool_pairs = K["POOL_CHUNKS"] * K["CHUNK_PAIRS"]
    for n, nt, grid, qb, fine in _flat_points():
        st = P.ladder(nt, n, grid, fine, (), qb)
        assert bool(st) == (nt * K["TILE_ROWS"] > K["POOL_MAX"]), (n, grid, qb, fine)
        if not st:
            continue
        assert all(s >= 2 for s in st) and all(a > b for a, b in zip(st, st[1:])), (n, grid, qb, fine, st)
        # the first level runs cold: EVERY row of every visited tile is a pair for every query row of the pass, and a key in each bucket
        visited = (nt + st[0] - 1) // st[0]
        assert visited * K["TILE_ROWS"] * K["QROWS"] * qb <= pool_pairs, (n, grid, qb, fine, st)
        assert visited * K["TILE_ROWS"] <= K["BUCKET_CAP"], (n, grid, qb, fine, st)
        assert P.ladder_fits(len(st))


def test_a_shard_the_select_step_sorts_whole_gets_no_ladder():
    for n in (0, 1, 31, 32, 33, 5000, K["POOL_MAX"] - 1, K["POOL_MAX"]):
        for grid in P.GRIDS:
            for fine in P.FINES:
                assert P.ladder((n + 31) // 32, n, grid, fine, (), 1) == [], n
    assert P.ladder((K["POOL_MAX"] + 32) // 32, K["POOL_MAX"] + 1, 256) != []


def test_ladder_of_the_full_size_shard_is_the_documented_one():
    n = 170_000_000
    assert P.ladder((n + 31) // 32, n, 256) == [20752, 512, 32]


def test_explicit_ladder_keeps_the_strides_that_sample():
    assert P.ladder(1000, 32000, 256, 0, (4096, 0, 1, 256, 16), 1) == [4096, 256, 16]
    assert P.ladder(1000, 32000, 256, 0, (0,), 1) == []


def test_kp_covers_the_candidates_the_select_step_wants():
    """~kp * last_ratio rows beat the last level's bound in the full scan: at least 1.5 C of them, on every ladder of the grid"""
    for n, nt, grid, qb, fine in _flat_points():
        st = P.ladder(nt, n, grid, fine, (), qb)
        for k in P.KS if st else ():
            for retry in (False, True):
                c = P.select_C(k, retry)
                assert max(k + 32, 2 * k) <= c or c == K["SELECT_C_MAX"]
                for sample_kp in (1, 16, 1024):
                    kp = P.kp(sample_kp, True, c, st[-1])
                    assert kp >= sample_kp and kp * st[-1] >= 1.5 * c, (n, grid, qb, fine, k, retry, kp)
    for nlist in P.NLISTS:
        for shape in P.SHAPES:
            lists, _ = P.list_geometry(P.tile_list_of(P.list_sizes(shape, nlist)), nlist)
            for nprobe in P.NPROBES:
                for nq in (1, 64, 700, 1024):
                    for fine in P.FINES:
                        lv, lr = P.ladder_units(lists, fine, nq, nprobe)
                        assert P.ladder_fits(len(lv))
                        assert all(a[0] > b[0] for a, b in zip(lv, lv[1:])) and all(s >= 2 for s, _ in lv[1:]), lv
                        for k in P.KS:
                            c = P.select_C(k)
                            if lv:
                                assert P.kp(16, True, c, lr) * lr >= 1.5 * c, (nlist, shape, nprobe, nq, fine, k)
    assert P.kp(16, False, 2048, 1.0) == 16                               # no level, no bound: the tuning value stands
    assert P.ladder_fits(K["UNIT_LAUNCHES"] - 1) and not P.ladder_fits(K["UNIT_LAUNCHES"])


def test_pass_rows_split_a_call_into_whole_passes():
    for n in (1, 127, 128, 129, 255, 256, 257, 700, 1024, 1025, 3000):
        for units in (False, True):
            for max_qb in (1, 2):
                left, got = n, []
                while left > 0:
                    nq, qb = P.pass_rows(left, units, max_qb)
                    assert 1 <= nq <= left and 1 <= qb <= max_qb and (qb == 1 or not units)
                    assert nq <= (K["PASS_MAX"] if units else K["QROWS"] * qb)
                    got.append(nq)
                    left -= nq
                assert sum(got) == n and all(g in (K["PASS_MAX"], K["QROWS"], 2 * K["QROWS"]) for g in got[:-1])


# ------------------------------------------------------------------------------------------------------------------ 4.2 clamp
def test_low_digit_clamp_falls_with_the_unit_and_keeps_the_norm_digit_in_int8():
    """dph_quantize_kernel: the digit the norm codes meet is ceil(unit ||q2|| / 128) with ||q2|| <= q2max sqrt(768): at most 126"""
    prev = None
    for unit in range(1, 600):
        q = P.q2max(unit)
        assert 1 <= q <= 64 and q == min(64, max(1, P.q2_limit(unit)))
        assert prev is None or q <= prev
        if P.q2_limit(unit) >= 1:
            assert unit * q * np.sqrt(768.0) / 128.0 <= 126.0, unit
        prev = q
    assert P.q2max(1) == 64 and P.q2_limit(600) == 0
    # the norm unit: the codes of the largest norm, ceil(rmax / unit), fit 127 per norm slot
    for n_norm in (4, 8):
        for r in np.concatenate([[0.0, 0.5, 507.9, 508.0, 508.1, 1016.0, 7067.0], np.random.default_rng(1).uniform(0, 7100, 300)]):
            u = P.norm_unit(r, n_norm)
            assert u >= 1 and np.ceil(r / u) <= 127 * n_norm and (u == 1 or np.ceil(r / (u - 1)) > 127 * n_norm), (r, n_norm, u)


# ------------------------------------------------------------------------------------------------------------------ 4.2 norm statistics
def test_norm_statistics_on_random_histograms():
    rng = np.random.default_rng(7)
    taken = 0
    for trial in range(200):
        hist = np.zeros(K["NORM_BINS"], np.uint32)
        lo, width = int(rng.integers(0, 400)), int(rng.integers(1, 60))
        body = rng.integers(lo, lo + width, int(rng.integers(1, 30000)))
        n_tail = 0 if trial % 4 == 0 else int(rng.integers(0, 3000 if trial % 3 else 40))          # (every fourth: a body alone, nothing to cut)
        tail = rng.integers(lo + width, lo + width + int(rng.integers(1, 4000)), n_tail)
        np.add.at(hist, np.concatenate([body, tail]), 1)
        if trial % 7 == 0 and trial % 4:
            hist[int(rng.integers(6000, 8192))] += 1                       # one extreme row
        top = int(np.nonzero(hist)[0].max())
        max2 = top * K["NORM_BIN_W"] + int(rng.integers(0, K["NORM_BIN_W"]))
        r = P.norm_stats(hist, max2)
        total = int(hist.sum())
        assert int(hist[r["cut_bin"]:].sum()) == r["above"] <= K["OUTLIER_MAX"]
        assert r["cut_bin"] == 0 or int(hist[r["cut_bin"] - 1:].sum()) > K["OUTLIER_MAX"]
        assert r["cut2"] == r["cut_bin"] * K["NORM_BIN_W"]
        if r["take_cut"]:                                                   # only when it tightens the norm bound by more than 10 %
            assert r["above"] > 0 and np.sqrt(r["cut2"]) * 1.1 < np.sqrt(max2)
            taken += 1
        else:
            assert r["above"] == 0 or r["cut_bin"] == 0 or r["cut2"] * 1.21 >= max2
        median_bin = int(np.repeat(np.arange(K["NORM_BINS"]), hist)[(total + 1) // 2 - 1])
        assert median_bin * K["NORM_BIN_W"] <= r["rmed"] ** 2 < (median_bin + 1) * K["NORM_BIN_W"]
    assert 20 <= taken <= 180                                               # both verdicts were exercised
    assert P.norm_stats(np.zeros(K["NORM_BINS"], np.uint32), 0) == dict(rmed=0.0, cut_bin=0, cut2=0, above=0, take_cut=False)


def test_column_statistics_round_and_clip_the_mean():
    n = 1000
    means = np.linspace(-140.0, 140.0, 768)
    sums = np.concatenate([np.rint(means * n), np.rint((means ** 2 + 9.0) * n)]).astype(np.int64)
    mu, sd = P.col_stats(sums, n)
    np.testing.assert_array_equal(mu, np.clip(np.rint(sums[:768] / n), -128, 127))
    assert (sd >= 0).all() and np.abs(sd - 3.0).max() < 0.3
    mu, sd = P.col_stats(sums, 0)
    assert not mu.any() and not sd.any()


# ------------------------------------------------------------------------------------------------------------------ 4.2 layout
class _Facts:
    """statistics of a shard that was never built: what choose_aux_layout reads"""

    def __init__(self, rng, n_rogue, tail):
        self.n_rows, self.n_out_found = 100_000, 0
        self.mu = rng.integers(30, 50, 768).astype(np.int32)
        self.sd = rng.uniform(6.0, 14.0, 768)
        for j in rng.choice(768, n_rogue, replace=False):
            self.mu[j] = int(rng.choice([-1, 1])) * int(rng.integers(60, 128))
        self.rmed = 300.0
        self.rmax_cut = self.rmax_all = 300.0 * tail

    def facts(self, scale=1.0):
        return np.array([self.rmed, self.rmax_cut * scale, self.rmax_all * scale], np.float64)


def _check_layout(lay, mode, st):
    rc, back = P.layout_roundtrip(lay)
    assert rc == 0 and np.array_equal(back, lay), lay                      # the validator accepts it; pack(unpack) is the identity
    stride, n_norm, n_rep = int(lay[0]), int(lay[1]), int(lay[2])
    assert (stride, n_norm) in ((0, 0), (4, 4), (16, 4), (32, 8)) and (mode <= 0 or stride in (mode, 4))
    mu_med, sd_med = np.sort(st.mu)[384], max(1.0, np.sort(st.sd)[384])
    rogue = set(np.nonzero(np.abs(st.mu - mu_med) / (3.5 * sd_med) >= 1.2)[0].tolist())
    slots = [int(d) for d in lay[4:4 + n_rep]]
    assert (lay[4 + n_rep:] == -1).all() and set(slots) <= rogue
    if stride >= 16:
        assert rogue and n_rep == (12 if stride == 16 else 24)             # every replica slot is dealt out ...
        assert len(set(slots)) == min(len(rogue), 12)                      # ... and every rogue dimension (the 12 worst) has at least one
    else:
        assert n_rep == 0 and (mode != -1 or stride == 0 or not rogue)


def test_every_chosen_layout_is_valid_and_serves_every_rogue_dimension():
    rng = np.random.default_rng(11)
    cases = [(name, st) for name, st in P.stat_shards().items()]
    cases += [("random", _Facts(rng, int(rng.integers(0, 20)), float(rng.choice([1.0, 1.2, 1.5, 3.0])))) for _ in range(60)]
    seen = set()
    for name, st in cases:
        for mode in P.AUX_MODES:
            lay = P.choose_layout(st, mode)
            _check_layout(lay, mode, st)
            seen.add(int(lay[0]))
            rc, lay2, forced, unit, n_out, rmax = P.aux_rows(st, mode)
            assert rc == 0 and not forced and np.array_equal(lay2[:3], lay[:3]) and np.array_equal(lay2[4:], lay[4:])
            if lay2[0] > 0:                                                 # aux rows: no row is set aside, the clamp follows the unit
                assert n_out == 0 and rmax == st.facts()[2] and unit == P.norm_unit(rmax, int(lay2[1])) and lay2[3] == P.q2max(unit)
            else:
                assert unit == 1 and lay2[3] == 64 and n_out == st.n_out_found
            # forced: it stays while its clamp serves the rows, and is dropped for a fresh choice when the norms outgrow it
            rc, lay3, forced3, _, _, _ = P.aux_rows(st, mode, lay2, True)
            assert rc == 0 and forced3 and np.array_equal(lay3, lay2)
            rc, lay4, forced4, unit4, _, _ = P.aux_rows(st, mode, lay2, True, scale=40.0)
            assert rc == 0 and (forced4 or lay2[0] > 0) and (forced4 or lay4[3] == P.q2max(unit4) < lay2[3])
    assert seen == {0, 4, 16, 32}
    for bad in ([8, 4, 0, 64], [4, 4, 1, 64], [16, 4, 13, 64], [32, 8, 25, 64], [4, 4, 0, 0], [4, 4, 0, 65], [0, 4, 0, 64]):
        assert P.layout_roundtrip(np.array(bad + [-1] * 24, np.int32))[0] == 1, bad
    for dim in (-1, 768):
        assert P.layout_roundtrip(np.array([16, 4, 2, 64, 5, dim] + [-1] * 22, np.int32))[0] == 2


def test_the_restated_layout_of_the_certificate_sets_is_the_real_one():
    """tests/_certificate_sets.py::choose_layout (numpy, what the certificate's restatement is built on) against choose_aux_layout"""
    from tests import _certificate_sets as S
    for name, sh in sorted(S.build()[0].items()):
        st = P.stat_shards()["cert_" + name]
        for mode in (4, 16):
            np.testing.assert_array_equal(P.choose_layout(st, mode), S.choose_layout(sh.xb, mode), err_msg=f"{name} mode {mode}")


# ------------------------------------------------------------------------------------------------------------------ 4.2 unit-scan capacities
def test_unit_queue_holds_every_probe_pattern():
    """chunks = sum over the lists of ceil(rows probing it / 128), units = chunks x segments of the list, counted by brute force"""
    rng = np.random.default_rng(13)
    for trial in range(120):
        nlist = int(rng.integers(1, 400))
        tiles = rng.integers(1, int(rng.choice([4, 300, 3000])), nlist)
        if trial % 4 == 0:
            tiles[int(rng.integers(0, nlist))] = int(rng.integers(3000, 60000))
        lists, tile0 = P.list_geometry(np.repeat(np.arange(nlist, dtype=np.int32), tiles), nlist)
        assert lists[3] == 1 and lists[4] == tiles.max() and np.array_equal(np.diff(tile0), tiles)
        segs = (tiles + K["UNIT_TILES"] - 1) // K["UNIT_TILES"]
        assert lists[5] == segs.sum()
        nprobe = int(rng.integers(1, 300))
        chunk_cap, unit_cap, too_large = P.unit_queue(lists, nprobe)
        assert not too_large
        n_q, np_eff = int(rng.integers(1, K["PASS_MAX"] + 1)), min(nprobe, nlist)
        for pattern in range(3):
            if pattern == 0:          # every row the same lists, the longest first
                probes = np.tile(np.argsort(-tiles)[:np_eff], (n_q, 1))
            elif pattern == 1:        # spread out: as many distinct lists as there are
                probes = np.stack([(r * np_eff + np.arange(np_eff)) % nlist for r in range(n_q)])
            else:
                probes = np.stack([rng.choice(nlist, np_eff, replace=False) for _ in range(n_q)])
            per_list = np.bincount(probes.ravel(), minlength=nlist)
            chunks = (per_list + K["UNIT_SLOTS"] - 1) // K["UNIT_SLOTS"]
            assert chunks.sum() <= chunk_cap and (chunks * segs).sum() <= unit_cap, (trial, pattern, nlist, nprobe, n_q)
    # lists that are not contiguous runs of tiles, too many lists: no unit scan
    assert P.list_geometry(np.array([0, 1, 0], np.int32), 2)[0][3] == 0
    lists, _ = P.list_geometry(np.repeat(np.arange(8, dtype=np.int32), 100), 8)
    assert P.use_units(lists, 4) and not P.use_units(lists, 0) and not P.use_units(lists, 4, list_major=False) and not P.use_units(lists, 4, ivf_units=0)
    short, _ = P.list_geometry(np.repeat(np.arange(8, dtype=np.int32), 63), 8)
    assert not P.use_units(short, 4) and P.use_units(short, 4, ivf_units=1)


# ------------------------------------------------------------------------------------------------------------------ 4.2 PQ capacities
def test_pq_scan_capacities_hold_every_choice_of_lists():
    rng = np.random.default_rng(17)
    rows = K["PASS_MAX"]
    for nlist in P.NLISTS:
        for shape in P.SHAPES:
            sizes = P.list_sizes(shape, nlist)
            prefix = P.pq_top_prefix(sizes)
            assert prefix[0] == 0 and np.array_equal(np.diff(prefix), np.sort(sizes)[::-1])
            order = np.argsort(-sizes, kind="stable")
            for nprobe in P.NPROBES:
                np_eff = min(nprobe, nlist)
                for M in P.MS:
                    r = P.pq_scan(M, sizes, prefix, rows, 10, nprobe)
                    seg = r["seg"]
                    assert seg == (K["PQ_SEG"] if M <= 96 else K["PQ_SEG"] // 2) and r["lds_bytes"] <= r["lds_bytes_max"] <= 160 * 1024
                    picks = [order[:np_eff], order[:np_eff][::-1], rng.permutation(order[:np_eff]), rng.choice(nlist, np_eff, replace=False)]
                    for pick in picks:
                        codes = sizes[pick]
                        assert codes.sum() <= r["row_codes_max"]
                        padded = np.concatenate([codes, np.zeros(-len(codes) % K["PQ_GROUP"], np.int64)]).reshape(-1, K["PQ_GROUP"])
                        units = int(((padded.sum(1) + seg - 1) // seg).sum())          # row-major: segments of every group of 64 lists
                        assert units <= r["row_units_max"]
                        pairs = int(((codes + seg * K["PQ_LM_CHUNK"] - 1) // (seg * K["PQ_LM_CHUNK"])).sum())    # list-major: chunks of every list
                        if r["by_rows"]:
                            assert rows * units <= r["unit_cap"]
                        else:
                            assert r["unit_cap"] == 0 and rows * pairs <= r["pair_cap"]
                    for k in P.KS:
                        c = P.pq_scan(M, sizes, prefix, rows, k, nprobe)
                        assert c["cand_cap"] >= 4 * k + 64 and c["per_seg"] >= k
