"""The sharded search's sample, union bound, merge and merge verdict on the restatement alone (no GPU): tests/_shard_merge_ref.py over the
input sets of tests/_shard_merge_sets.py.
  a. the verdict sets have teeth: each mutation of merged_status changes the verdict on some row of a named set;
  b. the rule is sound from first principles: hidden rows scoring up to every part's bound (up to its own k-th where it closed its top-k)
     never belong in the exact float64 top-k of a row the rule certifies -- also where the true k-th score rounds UP to fp32 across the
     bound, which the margin refuses and the "no margin" mutation accepts;
  c. union_bounds: at least every part's own bound, 16 entries above it, invariant under permutations of parts and slots;
  d. the sample sets are what they claim (ties at the 16-th place, all-negative scores, outliers on top, fewer than 16 sampled rows, no
     level at all, a ladder that does not nest) and stay inside the buckets and the pair pool;
  e. the protocol sets: no near-tie among the oracle's top-(k+1), every finite row of the k <= 16 sets certifies, the k = 32 set leaves rows
     at status 1, the non-finite row is 3, and status 0 means the oracle's top-k."""
import numpy as np
import pytest

from oracle import mips_oracle as O
from tests import _certificate_ref as R
from tests import _shard_merge_ref as M
from tests import _shard_merge_sets as S

GRID = 256                  # scan workgroups of an MI355X (one per CU): what the derived ladder is planned with


# ---------------------------------------------------------------------------------------------------------------- a, b: the verdict
def test_every_mutation_of_the_verdict_is_caught_by_a_named_set(capsys):
    sets = S.verdict_sets()
    caught = {m: {} for m in M.MUTATIONS}
    for name, s in sets.items():
        want = s.verdict()
        assert set(np.unique(want)) <= {0, 1, 3}
        for m in M.MUTATIONS:
            n = int((s.verdict(mutate=m) != want).sum())
            if n:
                caught[m][name] = n
    with capsys.disabled():
        print()
        for m, hits in caught.items():
            print(f"  mutation {m!r}: changes the verdict in {hits}")
    for m, hits in caught.items():
        assert hits, f"no set notices the mutation {m!r}"
    assert "rounds_up" in caught["no_margin"] and "kth_zero" in caught["ge"]
    # without bounds a deferred part is never certified; a part that reports 1 or 3 decides the row whatever the bounds say
    for s in sets.values():
        nb = s.verdict(bounds=False)
        any3, any12 = (s.status == 3).any(0), ((s.status == 1) | (s.status == 2)).any(0)
        np.testing.assert_array_equal(nb, np.where(any3, 3, any12.astype(np.int32)))
        wb = s.verdict()
        assert (wb[any3] == 3).all() and (wb[(s.status == 1).any(0) & ~any3] == 1).all() and (wb <= nb).all()
        assert (wb == 0).sum() > 0 and (wb == 1).sum() > 0


def _exact_topk_ids(s, r):
    """ids of the exact float64 top-k of row r over the returned candidates AND hidden rows: one per part scoring what the part's verdict
    allows at most -- its bound where it deferred (2), its own k-th true score where it closed a full top-k (0) -- with the largest ids"""
    cand = [(-float(s.S64[p, r, c]), int(s.I[p, r, c])) for p in range(S.VERDICT_P) for c in range(s.k) if s.I[p, r, c] >= 0]
    hidden = []
    for p in range(S.VERDICT_P):
        st = int(s.status[p, r])
        if st == 2 and s.bound[p, r] > -1.0e300:
            hidden.append((-float(s.bound[p, r]), 2 ** 62 + p))
        elif st == 0 and s.I[p, r, s.k - 1] >= 0:
            hidden.append((-float(s.S64[p, r, s.k - 1]), 2 ** 62 + p))
    return [i for _, i in sorted(cand + hidden)[:s.k]], [i for _, i in hidden]


def test_the_verdict_is_sound_against_hidden_rows_and_the_margin_is_what_makes_it_so():
    unsound_without_margin = 0
    for name, s in S.verdict_sets().items():
        assert np.array_equal(s.S64.astype(np.float32)[s.I >= 0], s.D[s.I >= 0])
        want, loose = s.verdict(), s.verdict(mutate="no_margin")
        for r in range(want.size):
            if not set(s.status[:, r].tolist()) <= {0, 2}:
                continue                                    # (1 / 3: nothing is claimed about such a part's hidden rows, and the verdict is never 0)
            top, hidden = _exact_topk_ids(s, r)
            if want[r] == 0:
                assert not set(top) & set(hidden), (name, r, s.row_info[r])
            elif loose[r] == 0 and set(top) & set(hidden):
                unsound_without_margin += 1
                assert name == "rounds_up"
    assert unsound_without_margin >= 6
    s = S.verdict_sets()["rounds_up"]
    want, loose = s.verdict(), s.verdict(mutate="no_margin")
    for r, info in enumerate(s.row_info):
        f = info["focus"]
        Sk, Dk = s.S64[0, r, s.k - 1], float(s.D[0, r, s.k - 1])
        assert Sk < s.bound[f, r] < Dk and s.kth[r] < s.bound[f, r]
        if s.status[f, r] == 2:
            assert want[r] == 1 and loose[r] == 0, (r, info)


def test_no_bound_of_the_table_comes_closer_to_the_kth_score_than_the_gpu_test_allows():
    for name, s in S.verdict_sets().items():
        for r in range(s.kth.size):
            k = s.kth[r]
            for p in range(S.VERDICT_P):
                b = s.bound[p, r]
                exact = (k == 0.0 or k == M.NO_KTH)         # (no product to contract: the device computes these bit for bit)
                assert (b == k and exact) or abs(b - k) >= abs(k) * S.NEAR * 0.5, (name, r, p, b, k)


def test_merge_restatement_on_its_own_sets():
    for P, n, k in S.MERGE_SHAPES + [(3, 0, 4)]:
        c = S.merge_case(P, n, k)
        m = M.merge(c["D"], c["I"], k, c["best"], c["pred"])
        for r in range(n):
            nv = int(m["nvalid"][r])
            assert nv == int((c["I"][:, r] >= 0).sum())
            w = min(nv, k)
            assert (m["I"][r, w:] == -1).all() and (m["src"][r, w:] == -1).all() and (m["best"][r, w:] == -1e9).all()
            p, col = m["src"][r, :w] // k, m["src"][r, :w] % k
            assert np.array_equal(m["I"][r, :w], c["I"][p, r, col]) and np.array_equal(m["D"][r, :w].view(np.uint32), c["D"][p, r, col].view(np.uint32))
            d = m["D"][r, :w].astype(np.float64)
            assert (np.diff(d) <= 0).all() and all(m["I"][r, j] < m["I"][r, j + 1] for j in range(w - 1) if d[j] == d[j + 1])
    c = S.merge_case(3, 257, 100)
    assert set(c["kinds"]) == set(S.MERGE_KINDS) and (c["I"] > 2 ** 32).any()


# ---------------------------------------------------------------------------------------------------------------- c: the union bound
def test_union_bounds_properties():
    rng = np.random.default_rng(9)
    seen = set()
    for P in S.UNION_PARTS:
        for n in S.UNION_ROWS:
            top, kinds = S.union_case(P, n)
            seen |= set(kinds)
            tau = M.union_bounds(top)
            own = np.stack([M.union_bounds(top[p:p + 1]) for p in range(P)])
            assert (tau[None, :] >= own).all()
            valid = top.astype(np.int64) != M.INT_MIN
            above = ((top.astype(np.int64) > tau[None, :, None]) & valid).sum((0, 2))
            total = valid.sum((0, 2))
            assert ((tau == M.INT_MIN) == (total < 16)).all() or "extremes" in kinds
            assert (above[tau != M.INT_MIN] >= 16).all()
            # exactly the 16-th: fewer than 16 entries are strictly above tau + 1
            strictly = ((top.astype(np.int64) > (tau + 1)[None, :, None]) & valid).sum((0, 2))
            assert (strictly[tau != M.INT_MIN] < 16).all()
            perm = top[rng.permutation(P)]
            flat = np.transpose(top, (1, 0, 2)).reshape(n, P * 16)
            shuffled = np.stack([flat[r, rng.permutation(P * 16)] for r in range(n)]).reshape(n, P, 16).transpose(1, 0, 2)
            assert np.array_equal(M.union_bounds(perm), tau) and np.array_equal(M.union_bounds(shuffled), tau)
            for r, kind in enumerate(kinds):
                if kind == "exactly_15" or kind == "all_int_min":
                    assert tau[r] == M.INT_MIN
                if kind in ("exactly_16", "exactly_17") and P > 1:
                    assert tau[r] != M.INT_MIN
    assert seen == set(S.UNION_KINDS)


# ---------------------------------------------------------------------------------------------------------------- d: the sample
def test_sample_sets_are_what_they_claim_and_fit_the_buckets(capsys):
    shards = S.sample_shards()
    for s in shards.values():
        assert s.xb.shape[0] % 32 != 0 or s.name == "outlier"
    assert shards["main"].shard.outliers.size == 0 and shards["large"].shard.outliers.size == 0 and shards["outlier"].shard.outliers.size >= 50
    assert 12000 <= shards["main"].xb.shape[0] and shards["large"].xb.shape[0] <= 40000
    lines = []
    for name, explicit, n_q in S.SAMPLE_CASES:
        s = shards[name]
        top, log = s.sample(n_q, GRID, explicit)
        assert (np.diff(top, axis=1) <= 0).all()
        for q0, nq, strides, kp, info in log:
            assert kp >= 16
            for lv in info:
                assert lv["bucket"].max() <= R.BUCKET_CAP, (name, explicit, lv["stride"])        # (lost pairs are out of scope)
                assert lv["bucket"].sum() <= 2 ** 21, "a quarter of the pair pool"
            if strides and M.nests(strides):
                key, _, _ = s.keys()
                np.testing.assert_array_equal(top[q0:q0 + nq], M.sample_top_closed_form(key[q0:q0 + nq], s.shard.outliers, strides[-1]))
        lines.append(f"  {name} ladder {explicit or 'default'} x {n_q} rows: passes " +
                     ", ".join(f"{nq} rows strides {st} kp {kp} largest bucket {max(int(lv['bucket'].max()) for lv in info) if info else 0}"
                               for _, nq, st, kp, info in log))
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    # kp of the intermediate levels: planned with k = 1
    assert M.sample_plan(S.MAIN_ROWS, GRID, 1, (16, 2))[1] == 32 and M.sample_plan(S.MAIN_ROWS, GRID, 1, (32, 4))[1] == 20
    assert M.sample_plan(S.MAIN_ROWS, GRID, 1, (8,)) == ([8], 16)
    # main: ten rows above a block of forty exact ties; the block holds the 16-th place under every explicit ladder
    m = shards["main"]
    key, _, _ = m.keys()
    for explicit in ((8,), (16, 2), (32, 4), (7, 2)):
        top, _ = m.sample(3, GRID, explicit)
        t = top[S.Q_TIES]
        assert (np.diff(t[:S.N_HIGHER + 1]) < 0).all() and (t[S.N_HIGHER:] == t[15]).all()
        assert t[15] == key[S.Q_TIES, m.notes["tie_slots"][0]] and (key[S.Q_TIES, m.notes["tie_slots"]] == t[15]).all()
        assert (top[S.Q_NEGATIVE] < 0).all() and (top[S.Q_NEGATIVE] != M.INT_MIN).all() and (top[S.Q_POSITIVE] > 0).all()
    assert (key[S.Q_NEGATIVE] < 0).all()                    # ... so the zero rows that pad the last tile would lead the sample
    assert 448 % 8 == 0 and 448 % 32 == 0 and 448 % 7 == 0 and (S.MAIN_ROWS - 1) // 32 == 448
    # outlier: the best rows of query rows 0..3 are outlier rows and stay out of the sample
    o = shards["outlier"]
    key, _, _ = o.keys()
    top, _ = o.sample(7, GRID, (16, 2))
    outl = set(o.shard.outliers.tolist())
    for q in range(4):
        assert int(np.argmax(key[q])) in outl and int(o.notes["sat"][q]) in outl and key[q].max() > top[q, 0]
    # few / small
    top, log = shards["few"].sample(7, GRID, (2,))
    assert ((top != M.INT_MIN).sum(1) == 13).all() and log[0][2] == [2]
    top, log = shards["small"].sample(7, GRID)
    assert (top == M.INT_MIN).all() and log[0][2] == []
    assert not M.nests([7, 2]) and M.nests([16, 2]) and M.nests([8])
    # both pass widths and a second pass
    assert [p[1:] for p in M.passes(300)] == [(256, 2), (44, 1)] and [p[1:] for p in M.passes(130)] == [(130, 2)] and M.passes(128)[0][2] == 1


# ---------------------------------------------------------------------------------------------------------------- e: the protocol
@pytest.fixture(scope="module")
def dump():
    return S.dump()


@pytest.mark.parametrize("name,P,k", S.PROTOCOL_SETS)
def test_protocol_sets(dump, name, P, k, capsys):
    run = dump.run(P, k, GRID)
    x, nf = dump.x, run["nonfinite"]
    fin = np.nonzero(~nf)[0]
    assert nf.sum() == 1 and nf[S.Q_NONFINITE] and dump.xb.shape[0] <= 100000
    # the oracle over the whole dump; no near-tie among its top-(k+1): equal bits (byte-identical rows) or more than two fp32 ulps apart
    _, Ir, D64 = O.flat_ip_search(x[fin], dump.xb, k + 1)
    gap = -np.diff(D64, axis=1)
    ulp = np.spacing(np.abs(D64[:, :-1]).astype(np.float32)).astype(np.float64)
    assert ((gap == 0) | (gap > 2 * ulp)).all()
    for q in S.Q_TIE:                                        # the cross-shard tie: ranks k-1 and k of the k = 10 sets, rows of two shards
        j = list(fin).index(q)
        if k + 1 > S.TIE_K:
            assert gap[j, S.TIE_K - 2] == 0 and sorted(Ir[j, S.TIE_K - 2:S.TIE_K].tolist()) == [3000 + S.Q_TIE.index(q), 45000 + S.Q_TIE.index(q)]
    # what the restatement says
    st = run["status"]
    assert st[S.Q_NONFINITE] == 3 and (run["merged"]["I"][S.Q_NONFINITE] == -1).all() and (st[fin] != 3).all()
    ex = M.status_exemptions(run, k)
    assert ex.sum() <= 0.02 * st.size
    if k <= 16:
        assert (st[fin] == 0).all(), st
    else:
        assert (st[fin] == 1).sum() >= 1 and (st[list(S.Q_HOME)] == 1).all()
        for q in S.Q_HOME:                                   # fewer than k rows of the whole dump beat the union bound
            assert sum(int((s.keys(x[q:q + 1])[0][0] > run["tau"][q]).sum()) for s in dump.shards(P)) == 16 < k
    for j, r in enumerate(fin):
        if st[r] == 0:
            np.testing.assert_array_equal(run["merged"]["I"][r], Ir[j, :k], err_msg=f"{name} q{r}")
    # the home rows: sampled (local tile 0), so the union bound sits just under the 16-th of them and the other shards return padding
    cuts = S.CUTS[P]
    if P > 2:
        assert len(dump.shards(P)[0].sample(x[:1], GRID)[1][0][2]) == 0                      # the shard too small for a ladder
        assert (run["top"][0][fin] == M.INT_MIN).all()
    for q, row0 in zip(S.Q_HOME, S.HOME_ROWS):
        home = [p for p in range(P) if cuts[p] <= row0 < cuts[p + 1]][0]
        if cuts[home] != row0:
            continue
        for p in range(P):                                   # (outlier rows are candidates of every query row: a shard that has some returns those)
            if p != home:
                ids = run["I_parts"][p, q][run["I_parts"][p, q] >= 0] - cuts[p]
                assert set(ids.tolist()) <= set(dump.shards(P)[p].outliers.tolist()) and run["status_parts"][p, q] == 2, (name, q, p)
        assert sum((run["I_parts"][p, q] == -1).all() for p in range(P)) >= P - 2
        assert (run["I_parts"][home, q, :min(k, 16)] >= 0).all()                                # (the 16 rows above the bound at least)
    assert any(s.outliers.size >= 50 for s in dump.shards(P))
    with capsys.disabled():
        print(f"\n  {name}: restated status {st.tolist()}, part statuses {run['status_parts'].tolist()}, exempt {int(ex.sum())}")
