"""GPU: the train step of the reference's index on the device (csrc/dph_pq_train.hip, densephrases_amd/pq_train.py, MIPS(pq={"train": ...}))
against the float64 restatement tests/_pq_train_ref.py.  The step is demanded EQUAL to the restatement -- codes, counts, the new codebooks bit
for bit -- outside the exempt set, which tests/test_pq_train_ref.py holds under its cap on these very inputs.

The whole-trainer margin.  The restatement of the trainer at the shape of TRAINER_CASE (4096 rows, nlist 16 given, M 96, 3 OPQ iterations,
8 / 2 / 5 Lloyd steps) run on the CPU from the seeds 0 .. 4 ended at the mean training errors
    31.590373900856324, 31.647364867570353, 31.680679316576068, 31.616480144170538, 31.63217241856148
so margin = 3 (max - min) / min = 3 * 0.090305 / 31.590374 = 8.576e-3 (TRAINER_MARGIN below)."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import _pq_train_ref as R

pytestmark = pytest.mark.gpu
DPH_E_ARG = -1
TRAINER_SEED_ERRORS = (31.590373900856324, 31.647364867570353, 31.680679316576068, 31.616480144170538, 31.63217241856148)
TRAINER_MARGIN = 3.0 * (max(TRAINER_SEED_ERRORS) - min(TRAINER_SEED_ERRORS)) / min(TRAINER_SEED_ERRORS)
ORTHO_BOUND = 2.0 ** -22


def _dev():
    import torch
    return torch.device("cuda", 0)


def _step(x, pqc, update=True, want_err=True):
    """dph_pq_train_step_dev over host arrays -> (codes, counts, row_err, codebooks after the call), host arrays"""
    import torch
    from densephrases_amd.pq_train import train_step_dev
    xt = torch.from_numpy(np.array(x, dtype=np.float32)).to(_dev())
    pt = torch.from_numpy(np.array(pqc, dtype=np.float32)).to(_dev())
    codes, counts, err = train_step_dev(xt, pt, update=update, want_err=want_err)
    torch.cuda.synchronize()
    return codes.cpu().numpy(), counts.cpu().numpy(), None if err is None else err.cpu().numpy(), pt.cpu().numpy()


def _comparable_codewords(ref, codes):
    """[M,256] bool: no member of the codeword under either assignment is an exempt cell"""
    M = codes.shape[1]
    bad = np.zeros((M, 256), bool)
    r, m = np.nonzero(ref["exempt"])
    bad[m, ref["codes"][r, m]] = True
    bad[m, codes[r, m]] = True
    return ~bad


def _assert_step_equals(ref, codes, counts, err, new_pqc, what):
    keep = ~ref["exempt"]
    diff = np.argwhere((codes != ref["codes"]) & keep)
    print(f"{what}: {int(ref['exempt'].sum())} exempt cells of {codes.size}, {len(diff)} other cells differ")
    assert len(diff) == 0, (what, diff[:10])
    ok = _comparable_codewords(ref, codes)
    np.testing.assert_array_equal(counts[ok], ref["counts"][ok], err_msg=what)
    assert int(counts.sum()) == codes.size
    if new_pqc is not None:
        np.testing.assert_array_equal(new_pqc.view(np.uint32)[ok], ref["pqc"].view(np.uint32)[ok], err_msg=what)
    if err is not None:
        rows = keep.all(1)
        ulp = np.spacing(ref["row_err"][rows])
        worst = np.abs(err[rows] - ref["row_err"][rows]) / np.where(ulp > 0, ulp, 1.0)
        print(f"{what}: row_err off by at most {worst.max() if worst.size else 0.0} ulp")
        assert (worst <= 1.0).all(), (what, worst.max())


# ------------------------------------------------------------------------------------------------- 1. the step, direct
@pytest.mark.parametrize("name", R.STEP_CASES)
def test_step_equals_the_restatement(name):
    x, pqc, ref = R.step_case(name)
    codes, counts, err, new = _step(x, pqc)
    _assert_step_equals(ref, codes, counts, err, new, name)
    if name in ("n255", "identical"):
        empty = ref["counts"] == 0
        assert empty.any(1).all()                                       # empty codewords in every sub-space ...
        np.testing.assert_array_equal(new[empty].view(np.uint32), np.asarray(pqc)[empty].view(np.uint32))          # ... keep their value
    if name == "identical":
        assert ((ref["counts"] == 0).sum(1) == 255).all()
    if name == "duplicates":
        assert not (codes == 9).any() and not (codes == 200).any()      # the copies of codeword 5 never win: a tie goes to the lowest j
        assert not (codes[:, ::2] == 255).any()
        np.testing.assert_array_equal(codes[100:200], codes[:100])


def test_step_without_update_leaves_the_codebooks_and_two_calls_give_the_same_bytes():
    x, pqc, ref = R.step_case("n4097")
    codes, counts, err, after = _step(x, pqc, update=False)
    np.testing.assert_array_equal(after.view(np.uint32), np.asarray(pqc).view(np.uint32))
    _assert_step_equals(ref, codes, counts, err, None, "update = 0")
    a, b = _step(x, pqc), _step(x, pqc)
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u.view(np.uint8), v.view(np.uint8))
    c2, n2, e2, _ = _step(x, pqc, update=False, want_err=False)         # row_err = NULL
    assert e2 is None
    np.testing.assert_array_equal(c2, codes)
    np.testing.assert_array_equal(n2, counts)


# ------------------------------------------------------------------------------------------------- 2. decode
@pytest.mark.parametrize("n", [1, 129, 4097])
def test_decode_equals_the_gather(n):
    import torch
    from densephrases_amd.pq_train import decode_dev
    rng = np.random.default_rng(n)
    for M in (96, 16):
        pqc = rng.normal(0, 0.3, (M, 256, 768 // M)).astype(np.float32)
        codes = rng.integers(0, 256, (n, M), dtype=np.uint8)
        codes[0], codes[-1, -1] = 255, 0
        y = decode_dev(torch.from_numpy(codes).to(_dev()), torch.from_numpy(pqc).to(_dev())).cpu().numpy()
        np.testing.assert_array_equal(y.view(np.uint32), R.decode(codes, pqc).view(np.uint32))


# ------------------------------------------------------------------------------------------------- 3. one OPQ iteration
def test_one_opq_iteration_equals_the_restatement():
    import torch
    from densephrases_amd.pq_train import opq_iteration_dev
    x, A0, pqc0 = R.opq_case_inputs()
    xt, At = torch.from_numpy(np.array(x)).to(_dev()), torch.from_numpy(A0).to(_dev())
    pt = torch.from_numpy(np.array(pqc0)).to(_dev())
    out = opq_iteration_dev(xt, At, pt, R.OPQ_CASE["steps"])
    xp = out["xp"].cpu().numpy()
    # the rotation: fp32 of a float64 product -- the product's own error (768 2^-53 sum |x||a|) can move the rounding by one ulp, no more
    want = R.rotate(x, A0)
    assert (np.abs(xp.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))).all()
    print("rotation: fp32 values that differ from numpy's:", int((xp != want).sum()), "of", xp.size)
    ref = R.opq_iteration(x, A0, pqc0, R.OPQ_CASE["steps"], xp=xp)      # everything behind the rotation from the SAME rotated rows
    codes = out["codes"].cpu().numpy()
    diff = np.argwhere((codes != ref["codes"]) & ~ref["exempt"])
    print(f"one OPQ iteration: exempt share {ref['exempt_share']:.2e}, {len(diff)} non-exempt cells differ")
    assert ref["exempt_share"] <= R.EXEMPT_CAP and len(diff) == 0, diff[:10]
    if ref["exempt_share"] == 0.0:
        np.testing.assert_array_equal(pt.cpu().numpy().view(np.uint32), ref["pqc"].view(np.uint32))
    Cm = out["C"].cpu().numpy()
    y = R.decode(codes, pt.cpu().numpy()).astype(np.float64)
    bound = len(x) * 768 * 2.0 ** -53 * (np.abs(y).T @ np.abs(np.asarray(x, np.float64)))
    exact = y.T @ np.asarray(x, np.float64)
    assert (np.abs(Cm - exact) <= bound).all()
    A = out["A_new"].astype(np.float64)
    dev_orth = np.abs(A @ A.T - np.eye(768)).max()
    print("orthogonality of A:", dev_orth)
    assert out["A_new"].dtype == np.float32 and dev_orth <= ORTHO_BOUND
    assert abs(out["err"] - ref["err"]) <= 1e-12 * ref["err"]


# ------------------------------------------------------------------------------------------------- 4. the whole trainer
@functools.lru_cache(maxsize=None)
def _trainer_run(which):
    from densephrases_amd.pq_train import train_index_resident
    T = R.TRAINER_CASE
    x, cent = R.trainer_case_inputs()
    return train_index_resident(np.asarray(x), T["nlist"], M=T["M"], opq_iters=T["opq_iters"], pq_iters_first=T["pq_iters_first"],
                                pq_iters=T["pq_iters"], final_pq_iters=T["final_pq_iters"], train_rows=T["n"], centroids=np.asarray(cent),
                                seed=T["seed"], return_info=True)


def test_whole_trainer_is_deterministic_monotone_and_as_good_as_the_restatement():
    T = R.TRAINER_CASE
    x, cent = R.trainer_case_inputs()
    (ix, info), (ix2, _) = _trainer_run(0), _trainer_run(1)
    ivf = ix.index
    assert ix.is_trained and ix.ntotal == 0 and ivf.by_residual and ivf.nprobe == 1 and ivf.direct_map_type == 2 and ivf.metric == 0
    assert ix.chain[0].A.shape == (768, 768) and ivf.centroids.shape == (16, 768) and ivf.pq_centroids.shape == (96, 256, 8)
    for a, b in ((ix.chain[0].A, ix2.chain[0].A), (ivf.centroids, ix2.index.centroids), (ivf.pq_centroids, ix2.index.pq_centroids)):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    np.testing.assert_array_equal(ivf.centroids, cent)
    print("OPQ error per iteration:", info["opq_err"], "residual PQ per step:", info["pq_err"], "final:", info["final_err"])
    assert len(info["opq_err"]) == T["opq_iters"] and all(b <= a for a, b in zip(info["opq_err"], info["opq_err"][1:]))
    trace = info["pq_err"] + [info["final_err"]]
    assert len(trace) == T["final_pq_iters"] + 1 and all(b <= a for a, b in zip(trace, trace[1:]))
    A = ix.chain[0].A.astype(np.float64)
    assert np.abs(A @ A.T - np.eye(768)).max() <= ORTHO_BOUND
    got = R.training_error(x, ix.chain[0].A, ivf.centroids, ivf.pq_centroids)
    want = R.trainer_restatement()["final_err"]
    print(f"final training error: device {got!r}, restatement {want!r}, margin {TRAINER_MARGIN:.3e}")
    assert abs(got - info["final_err"]) <= 1e-9 * got
    assert got <= (1.0 + TRAINER_MARGIN) * want


# ------------------------------------------------------------------------------------------------- 5. through MIPS
def test_mips_trains_builds_saves_and_answers_like_its_own_files(tmp_path):
    import os
    from densephrases_amd import DocMeta, DocStore, MIPS, faiss_io as F
    from densephrases_amd.ivf import dequant
    from oracle import ivfpq_oracle as P
    from tests._golden import load_toy_docs
    from tests._pq_encode_ref import empty_copy
    from tests.test_pq import INDEX_NAME, _pq_cases, _write_pq_layout
    from tests.test_pq_encode_gpu import _same
    nlist, M = 64, 96
    store = DocStore([DocMeta(m.doc_idx, m.title, m.context, m.f2o_start, m.word2char_start, m.word2char_end, m.start) for m in load_toy_docs()])
    root = _write_pq_layout(str(tmp_path / "dump"))
    idx_dir = os.path.join(root, "start", INDEX_NAME)
    p1, p2 = str(tmp_path / "built" / "trained.faiss"), os.path.join(idx_dir, "index.faiss")
    os.remove(p2)                                                       # (the fixture's own index: this test writes its own there)
    first = MIPS.from_store(store, pq={"train": {"nlist": nlist, "M": M, "opq_iters": 2, "pq_iters_first": 6, "pq_iters": 2, "final_pq_iters": 6},
                                       "save_trained": p1, "save": p2})
    trained = F.read_index(p1)
    assert trained.ntotal == 0 and trained.is_trained and trained.index.nlist == nlist and trained.index.M == M
    second = MIPS.from_store(store, pq={"trained": p1})
    third = MIPS(phrase_dump_dir=os.path.join(root, "phrase"), index_path=p2, idx2id_path=os.path.join(idx_dir, "idx2id.hdf5"), cuda=True)
    assert first.index.ntotal == second.index.ntotal == third.index.ntotal == store.n_rows and first.pq == second.pq == third.pq
    cases, _ = _pq_cases()
    for c in cases:
        kw = dict(q_texts=[f"q{i}" for i in range(c["B"])], top_k=c["top_k"], aggregate=c["aggregate"], return_idxs=c["return_idxs"],
                  max_answer_length=c["L"], agg_strat=c["agg_strat"], return_sent=c["return_sent"])
        q = c["query_arr"].astype(np.float64)
        want = first.search(q, **kw)
        _same(second.search(q, **kw), want)
        _same(third.search(q, **kw), want)
    # recall@10 at nprobe = nlist against the exact flat search: at least the oracle's stand-in training (random rotation, 4-step k-means)
    xb = dequant(store.rows, store.offset, store.scale)
    flat = MIPS.from_store(store)
    oracle = MIPS.from_store(store, pq={"trained": empty_copy(P.train(xb, nlist=nlist, M=M, seed=5))})
    rng = np.random.default_rng(17)
    q = (xb[rng.choice(len(xb), 64, replace=False)] + rng.normal(0, 0.1, (64, 768))).astype(np.float32)
    _, I_true = flat.index.search(q, 10)

    def recall(m):
        prev = m._set_nprobe(nlist)
        try:
            _, I = m.index.search(q, 10)
        finally:
            m._set_nprobe(prev)
        return np.mean([len(set(a) & set(b)) / 10.0 for a, b in zip(I.tolist(), I_true.tolist())])
    r_trained, r_oracle = recall(first), recall(oracle)
    print(f"recall@10 at nprobe = nlist: trained on the device {r_trained:.4f}, oracle stand-in {r_oracle:.4f}")
    assert r_trained >= r_oracle
    for m in (first, second, third, flat, oracle):
        m.close()


# ------------------------------------------------------------------------------------------------- 6. a resident shard as the input
def test_resident_int8_shard_gives_what_its_dequantised_rows_give():
    from densephrases_amd import Shard
    from densephrases_amd.pq_train import train_index_resident
    x, cent = R.trainer_case_inputs()
    n = 1024
    rows = R.quantise(np.asarray(x[:n], np.float64))
    np.testing.assert_array_equal(R.dequant(rows), x[:n])               # the set IS de-quantised int8 rows
    flat = Shard(n, device=0)
    flat.upload(rows)
    flat.finalize()
    kw = dict(nlist=16, M=96, opq_iters=2, pq_iters_first=3, pq_iters=1, final_pq_iters=2, train_rows=n, centroids=np.asarray(cent), seed=4)
    a = train_index_resident(flat, **kw)
    b = train_index_resident(np.asarray(x[:n]), **kw)
    flat.close()
    np.testing.assert_array_equal(a.chain[0].A.view(np.uint32), b.chain[0].A.view(np.uint32))
    np.testing.assert_array_equal(a.index.centroids.view(np.uint32), b.index.centroids.view(np.uint32))
    np.testing.assert_array_equal(a.index.pq_centroids.view(np.uint32), b.index.pq_centroids.view(np.uint32))


# ------------------------------------------------------------------------------------------------- 7. misuse
def test_misuse_is_refused_with_a_code_and_a_message_and_a_nan_row_raises():
    import torch
    from densephrases_amd import _lib
    from densephrases_amd.pq_train import train_index_resident
    lib, vp = _lib.lib, C.c_void_p
    dev = _dev()
    x = torch.zeros((8, 768), dtype=torch.float32, device=dev)
    pqc = torch.zeros((96, 256, 8), dtype=torch.float32, device=dev)
    codes = torch.zeros((8, 96), dtype=torch.uint8, device=dev)
    counts = torch.zeros((96, 256), dtype=torch.int32, device=dev)
    y = torch.zeros((8, 768), dtype=torch.float32, device=dev)
    for M in (0, 7, 24, 100, 192, 256, -96):
        assert lib.dph_pq_train_step_dev(0, vp(x.data_ptr()), 8, M, vp(pqc.data_ptr()), vp(codes.data_ptr()), vp(counts.data_ptr()), None, 1, None) == DPH_E_ARG
        assert b"M must be" in lib.dph_last_error()
        assert lib.dph_pq_decode_dev(0, vp(codes.data_ptr()), 8, M, vp(pqc.data_ptr()), vp(y.data_ptr()), None) == DPH_E_ARG
        assert b"M must be" in lib.dph_last_error()
    for n in (0, -1, 1 << 31):
        assert lib.dph_pq_train_step_dev(0, vp(x.data_ptr()), n, 96, vp(pqc.data_ptr()), vp(codes.data_ptr()), vp(counts.data_ptr()), None, 1, None) == DPH_E_ARG
        assert b"rows" in lib.dph_last_error()
        assert lib.dph_pq_decode_dev(0, vp(codes.data_ptr()), n, 96, vp(pqc.data_ptr()), vp(y.data_ptr()), None) == DPH_E_ARG
        assert b"rows" in lib.dph_last_error()
    assert lib.dph_pq_train_step_dev(0, None, 8, 96, vp(pqc.data_ptr()), vp(codes.data_ptr()), vp(counts.data_ptr()), None, 1, None) == DPH_E_ARG
    assert b"null" in lib.dph_last_error()
    torch.cuda.synchronize()
    rows, cent = R.trainer_case_inputs()
    bad = np.array(rows[:600])
    bad[321, 5] = np.nan
    torch.cuda.empty_cache()
    before = torch.cuda.memory_allocated(dev)
    with pytest.raises(ValueError, match="row 321 "):
        train_index_resident(bad, 16, M=96, train_rows=600, centroids=np.asarray(cent))
    assert torch.cuda.memory_allocated(dev) == before
    with pytest.raises(ValueError):
        train_index_resident(np.asarray(rows[:600]), 16, M=100, centroids=np.asarray(cent))
    with pytest.raises(ValueError):
        train_index_resident(np.asarray(rows[:600]), 16, M=96)            # fp32 rows without centroids
