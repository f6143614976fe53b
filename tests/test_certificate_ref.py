"""The certificate's inequality, on the restatement alone (no GPU): tests/_certificate_ref.py over the input sets of
tests/_certificate_sets.py.
  a. wherever the restated status is 0 the restated answer is the oracle's top-k;
  b. the sets have teeth: the unmutated bound holds for every (query row, row that was not re-scored) pair, and each of seven
     mutations of the bound is broken by at least one such pair;
  c. the rows whose k-th score sits inside the bound's tolerance -- the status comparisons the GPU test has to leave out -- are at most
     2 % of every set."""
import numpy as np
import pytest

from oracle import mips_oracle as O
from tests import _certificate_ref as R
from tests import _certificate_sets as S

MUTATIONS = {
    "drop ||e|| rmax": {"drop": ("e_r",)},
    "drop <e, mu>": {"drop": ("e_mu",)},
    "drop ||q||_1 dmax": {"drop": ("lut",)},
    "rmax_all -> rmax on the outlier path": {"outlier_rmax": True},
    "rmax -> 0.98 rmax": {"rmax_scale": 0.98},
    "lmax -> lmax - 128 in the emission rule": {"lmax_shift": -128},
    "a_cut ignored": {"ignore_a_cut": True},
}


@pytest.fixture(scope="module")
def built():
    shards, sets = S.build()
    return shards, sets, {s.name: s.certify() for s in sets}


def _worst_unscored(c):
    """(largest S64 among the rows that were not re-scored, that row)"""
    s = c["S64"].copy()
    s[c["rescored"]] = -np.inf
    row = int(np.argmax(s))
    return float(s[row]), row


def test_shard_constants_of_the_sets():
    shards, _ = S.build()
    for name in ("plain", "codec"):
        assert shards[name].outliers.size == 0 and shards[name].rmax == shards[name].rmax_all
    o = shards["outlier"]
    assert 50 <= o.outliers.size <= R.OUTLIER_MAX
    assert np.array_equal(o.outliers, np.nonzero(o.n2 >= round(o.rmax ** 2))[0]) and o.rmax_all ** 2 == pytest.approx(o.n2.max(), rel=1e-15)
    for mode in (4, 16):
        a = shards["aux%d" % mode]
        assert int(a.layout[0]) == mode and a.rmax == a.rmax_all and a.outliers.size == 0
    for s in shards.values():
        assert 12000 <= s.xb.shape[0] <= 20000


def test_restated_status_zero_means_the_oracle_top_k(built):
    _, sets, res = built
    seen = {0: 0, 2: 0}
    for s in sets:
        Dr, Ir, D64 = O.flat_ip_search(s.x, s.shard.xb, s.k, offset=s.shard.codec[0], factor=s.shard.codec[1])
        for r, c in enumerate(res[s.name]):
            seen[c["status"]] += 1
            if c["status"] != 0:
                continue
            D = np.where(c["I"] >= 0, c["D64"], -np.float64(O.FLT_MAX)).astype(np.float32)
            ok, msg = O.topk_equivalent(D[None, :], c["I"][None, :], D64[r:r + 1], Ir[r:r + 1])
            assert ok, (s.name, r, msg)
    assert seen[0] >= 40 and seen[2] >= 20, seen


def test_planted_rows_sit_where_the_sets_say(built):
    _, sets, res = built
    by = {s.name: s for s in sets}
    for name in ("q2_filtered", "q2_filtered_aux4", "q2_filtered_aux16"):
        for r, row in by[name].planted.items():
            c = res[name][r]
            assert not c["emitted"][row] and c["a_rest"] == int(by[name].tau[r]) and c["n_emitted"] <= 8 and c["status"] == 2, (name, r)
    for name in ("e_aligned", "one_signed", "lut_default", "lut_wide_codec", "outlier_in_pool", "under_the_cut"):
        for r, row in by[name].planted.items():           # n* is the best key left in the pool: a_rest = I(n*); the rows re-scored in
            c = res[name][r]                              # its place tie with it and obey its bound: the row stays uncertified
            assert row not in set(c["rescored"].tolist()) and c["a_rest"] == int(c["key"][row]) and c["status"] == 2, (name, r)
            assert (c["key"][c["rescored"]] >= c["key"][row]).all() and _worst_unscored(c)[1] == row, (name, r)
    o = by["outlier_in_pool"].shard
    assert all(row in set(o.outliers.tolist()) for row in by["outlier_in_pool"].planted.values())
    c = res["radix_cut"][0]
    row = by["radix_cut"].planted[0]
    assert c["a_cut"] is not None and 9000 <= c["n_emitted"] <= 30000 and c["key"][row] <= c["a_cut"] and row in set(o.outliers.tolist())
    assert all(9000 <= c["n_emitted"] <= 30000 and c["a_cut"] is not None for c in res["radix_cut"])
    for c in res["fewer_than_k"]:
        assert c["n_cand"] == by["fewer_than_k"].k - 3 and c["status"] == 2 and (c["I"][-3:] == -1).all()
    assert by["random_130"].x.shape[0] == 130
    assert sorted({s.k for s in sets}) == [1, 10, 33, 100]


def test_the_unmutated_bound_holds_and_every_mutation_is_broken_by_some_pair(built, capsys):
    _, sets, res = built
    tight = {}
    for s in sets:
        for r, c in enumerate(res[s.name]):
            worst, row = _worst_unscored(c)
            # float64 summation error of the two sides only (the inequality itself is exact arithmetic)
            assert worst <= c["bound_cert"] + 2 * R.sum_error(c["terms"]), (s.name, r, row, worst, c["bound_cert"])
            kept = np.ones(s.shard.xb.shape[0], bool)
            kept[c["I"][c["I"] >= 0]] = False
            assert c["S64"][kept].max() <= c["bound"] + 2 * R.sum_error(c["terms"]), (s.name, r)      # what is handed out: every row not returned
            tight[s.name] = min(tight.get(s.name, np.inf), c["bound_cert"] - worst)
    broken = {}
    for name, mut in MUTATIONS.items():
        broken[name] = []
        for s in sets:
            for r, c in enumerate(s.certify(mutate=mut)):
                worst, row = _worst_unscored(c)
                if worst > c["bound_cert"] + 2 * R.sum_error(c["terms"]):
                    broken[name].append((s.name, r, row, worst - c["bound_cert"]))
    with capsys.disabled():
        print()
        for name, hits in broken.items():
            print(f"  mutation {name!r}: broken by {len(hits)} pairs, e.g. {max(hits, key=lambda h: h[3]) if hits else None}")
        for name, v in tight.items():
            print(f"  set {name}: smallest bound - max S64(not re-scored) = {v:.3e}")
    for name, hits in broken.items():
        assert hits, f"no input pair breaks the mutation {name!r}: the sets are too soft"


def test_exempt_status_comparisons_stay_rare(built, capsys):
    _, sets, res = built
    for s in sets:
        n = 0
        for c in res[s.name]:
            if c["terms"] is None or c["n_cand"] < s.k:
                continue
            n += abs(c["D64"][s.k - 1] - c["bound_cert"]) <= R.bound_tol(c["terms"], c["bound_cert"]) + R.sum_error(c["terms"])
        with capsys.disabled():
            print(f"  set {s.name}: {n} of {len(res[s.name])} status comparisons exempt")
        assert n <= 0.02 * len(res[s.name]), (s.name, n)
