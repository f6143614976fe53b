"""CPU-only: the float64 restatement of the train step (tests/_pq_train_ref.py) is what tests/test_pq_train_gpu.py may be held to -- its exempt
sets stay under the cap on every input the GPU tests use, its OPQ alternation behaves like one (the error falls, A stays orthogonal) -- and
the host-side ends of the feature: the trained index through the FAISS file format, the argument checks of MIPS(pq={"train": ...}).

Seed-to-seed spread.  The restated trainer over TRAINER_CASE from the seeds 0 .. 4 ended its OPQ stage at the mean errors
    17.369707781360432, 17.396789935424295, 17.420620219914856, 17.346513573009904, 17.364643929591765
(spread max - min = 0.0741) after first iterations at 21.50 +- 0.03: OPQ_SEED_SPREAD below."""
import numpy as np
import pytest

from tests import _pq_train_ref as R

OPQ_SEED_FINALS = (17.369707781360432, 17.396789935424295, 17.420620219914856, 17.346513573009904, 17.364643929591765)
OPQ_SEED_SPREAD = max(OPQ_SEED_FINALS) - min(OPQ_SEED_FINALS)


@pytest.mark.parametrize("name", R.STEP_CASES)
def test_exempt_share_of_the_step_cases_is_within_the_cap(name):
    x, pqc, ref = R.step_case(name)
    share = ref["exempt"].mean()
    print(f"{name}: {int(ref['exempt'].sum())} exempt cells of {ref['exempt'].size} ({share:.2e})")
    assert share <= R.EXEMPT_CAP
    assert int(ref["counts"].sum()) == ref["codes"].size
    if name == "duplicates":                                # exact ties are decided, never exempt: the lowest j
        assert not (ref["codes"] == 9).any() and not (ref["codes"] == 200).any() and (ref["codes"] == 5).any()


def test_exempt_share_of_the_opq_case_and_of_the_trainer_case_is_within_the_cap():
    x, A0, pqc0 = R.opq_case_inputs()
    o = R.opq_iteration(x, A0, pqc0, R.OPQ_CASE["steps"])
    print("one OPQ iteration:", o["exempt_share"], "whole trainer:", R.trainer_restatement()["exempt_share"])
    assert o["exempt_share"] <= R.EXEMPT_CAP and R.trainer_restatement()["exempt_share"] <= R.EXEMPT_CAP
    # x' of int8 rows and of int8 residual codebooks: the step test of the restatement's own parts
    assert o["codes"].shape == (R.OPQ_CASE["n"], R.OPQ_CASE["M"]) and o["pqc"].dtype == np.float32 and o["A_new"].dtype == np.float32


def test_update_is_the_ascending_row_order_sum_and_keeps_empty_codewords():
    rng = np.random.default_rng(0)
    x = rng.normal(0, 1, (40, 768)).astype(np.float32)
    pqc = rng.normal(0, 1, (16, 256, 48)).astype(np.float32)
    codes = rng.integers(0, 3, (40, 16)).astype(np.uint8)
    new, counts = R.update(x, codes, pqc)
    for m in (0, 7, 15):
        for j in range(3):
            acc = np.zeros(48, np.float64)
            for r in range(40):
                if codes[r, m] == j:
                    acc = acc + x[r, m * 48:(m + 1) * 48].astype(np.float64)
            np.testing.assert_array_equal(new[m, j], (acc / counts[m, j]).astype(np.float32))
    np.testing.assert_array_equal(new[:, 3:], pqc[:, 3:])
    assert (counts[:, 3:] == 0).all() and (counts.sum(1) == 40).all()


def test_split_takes_the_largest_donors_in_stable_order():
    pqc = np.arange(2 * 256 * 4, dtype=np.float32).reshape(2, 256, 4) + 1
    counts = np.full((2, 256), 2, np.int64)
    counts[0, [3, 10]] = 0
    counts[0, [7, 20, 30]] = 9                              # a three-way tie for the largest: 7, then 20
    counts[1, 5] = 0
    counts[1, :5] = 1
    counts[1, 6:] = 1                                       # no donor with more than one member: codeword 5 stays
    before = pqc.copy()
    assert R.split_empty(pqc, counts) == 2
    up, down = np.float32(1 + 1 / 1024), np.float32(1 - 1 / 1024)
    np.testing.assert_array_equal(pqc[0, 3], before[0, 7] * np.array([up, down, up, down], np.float32))
    np.testing.assert_array_equal(pqc[0, 7], before[0, 7] * np.array([down, up, down, up], np.float32))
    np.testing.assert_array_equal(pqc[0, 10], before[0, 20] * np.array([up, down, up, down], np.float32))
    np.testing.assert_array_equal(pqc[0, 30], before[0, 30])
    np.testing.assert_array_equal(pqc[1], before[1])


def test_restated_opq_error_falls_and_a_stays_orthogonal():
    r = R.trainer_restatement()
    print("OPQ error per iteration:", r["opq_err"], "residual PQ:", r["pq_err"], r["final_err"])
    assert all(b <= a for a, b in zip(r["opq_err"], r["opq_err"][1:]))
    trace = r["pq_err"] + [r["final_err"]]
    assert all(b <= a for a, b in zip(trace, trace[1:]))
    A = r["A"].astype(np.float64)
    assert r["A"].dtype == np.float32 and np.abs(A @ A.T - np.eye(768)).max() <= 2.0 ** -22
    # the alternation buys more than a change of seed does
    assert r["opq_err"][0] - r["opq_err"][-1] > OPQ_SEED_SPREAD
    assert abs(r["opq_err"][-1] - OPQ_SEED_FINALS[0]) <= 1e-6 * OPQ_SEED_FINALS[0]
    x, cent = R.trainer_case_inputs()
    assert R.training_error(x, r["A"], cent, r["pqc"]) == r["final_err"]


def test_the_device_draws_the_seeds_the_restatement_draws():
    from densephrases_amd.pq_train import draw_seeds
    s = draw_seeds(3, 1000, 48)
    A0, init_opq, init_pq = R.draw_seeds(3, 1000, 48)
    np.testing.assert_array_equal(s["A0"], A0)
    np.testing.assert_array_equal(s["init_opq"], init_opq)
    np.testing.assert_array_equal(s["init_pq"], init_pq)
    assert all(len(set(row)) == 256 for row in init_opq.tolist())
    with pytest.raises(ValueError):
        draw_seeds(0, 255, 96)


def test_trained_index_round_trips_through_the_faiss_file(tmp_path):
    from densephrases_amd import faiss_io as F
    r = R.trainer_restatement()
    _, cent = R.trainer_case_inputs()
    nlist, M = R.TRAINER_CASE["nlist"], R.TRAINER_CASE["M"]
    ivf = F.IVFPQIndex(768, nlist, M, 8, np.asarray(cent), r["pqc"], [np.zeros((0, M), np.uint8) for _ in range(nlist)],
                       [np.zeros(0, np.int64) for _ in range(nlist)], True, F.METRIC_INNER_PRODUCT, 1, 2)
    ix = F.PreTransformIndex([F.LinearTransform(r["A"])], ivf, 768, True)
    p = str(tmp_path / "trained.faiss")
    F.write_index(ix, p)
    back = F.read_index(p)
    assert isinstance(back, F.PreTransformIndex) and back.ntotal == 0 and back.is_trained and back.chain[0].is_trained
    b = back.index
    assert (b.nlist, b.M, b.nbits, b.by_residual, b.nprobe, b.direct_map_type, b.metric) == (nlist, M, 8, True, 1, 2, F.METRIC_INNER_PRODUCT)
    assert back.chain[0].A.shape == (768, 768) and b.centroids.shape == (nlist, 768) and b.pq_centroids.shape == (M, 256, 768 // M)
    np.testing.assert_array_equal(back.chain[0].A, r["A"])
    np.testing.assert_array_equal(b.centroids, cent)
    np.testing.assert_array_equal(b.pq_centroids, r["pqc"])
    assert all(len(i) == 0 for i in b.list_ids)


def test_mips_argument_conflicts_raise_value_error():
    from densephrases_amd import DocMeta, DocStore, MIPS
    from tests._golden import load_toy_docs
    store = DocStore([DocMeta(m.doc_idx, m.title, m.context, m.f2o_start, m.word2char_start, m.word2char_end, m.start) for m in load_toy_docs()])
    train = {"nlist": 4, "M": 96}
    with pytest.raises(ValueError, match="trained"):
        MIPS.from_store(store, pq={"train": train, "trained": "trained.faiss"})
    with pytest.raises(ValueError, match="ivf"):
        MIPS.from_store(store, pq={"train": train}, ivf={"nlist": 4, "nprobe": 2})
    with pytest.raises(ValueError, match="world"):
        MIPS(None, "in-memory", None, _store=store, pq={"train": train}, rank=0, world=2, dist=object())
    with pytest.raises(ValueError):
        MIPS.from_store(store, pq={})


def test_exported_entry_points_refuse_bad_arguments_without_a_gpu():
    from densephrases_amd import _lib
    lib = _lib.lib
    assert lib.dph_pq_train_step_dev(0, None, 8, 96, None, None, None, None, 1, None) == -1 and b"dph_pq_train_step_dev" in lib.dph_last_error()
    assert lib.dph_pq_decode_dev(0, None, 8, 96, None, None, None) == -1 and b"dph_pq_decode_dev" in lib.dph_last_error()
    assert {"dph_pq_train_step_dev", "dph_pq_decode_dev"} <= set(_lib.EXPORTED)
