"""GPU: the add step of the reference's index on the device (csrc/dph_pq_encode.hip, densephrases_amd/pq_build.py, MIPS(pq=...)) against
the float64 restatement tests/_pq_encode_ref.py -- pinned on the CPU to oracle.ivfpq_oracle.add_with_ids, exempt set EMPTY on the four
input sets -- so lists and codes are demanded EQUAL, exact ties between duplicated codewords / centroids included (lowest index)."""
import copy
import ctypes as C
import functools
import os

import numpy as np
import pytest

from densephrases_amd import faiss_io as F
from oracle import ivfpq_oracle as P
from tests import _pq_encode_ref as R

pytestmark = pytest.mark.gpu
DPH_E_ARG, DPH_E_STATE = -1, -4


def _encode(shard, x, chunks=None):
    """pq_encode_dev over x [n,768] (host) in the given chunk sizes (default: one call) -> (lists int32 [n], codes uint8 [n,M]) on the host"""
    import torch
    dev = torch.device("cuda", shard.device)
    n, M = x.shape[0], shard.pq["M"]
    xt = torch.from_numpy(np.array(x, dtype=np.float32)).to(dev)
    lists = torch.full((n,), -7, dtype=torch.int32, device=dev)
    codes = torch.full((n, M), 0xEE, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    r0 = 0
    for m in (chunks or [n]):
        shard.pq_encode_dev(xt[r0:].data_ptr(), m, lists[r0:].data_ptr(), codes[r0:].data_ptr(), stream=st)
        r0 += m
    assert r0 == n
    torch.cuda.synchronize(dev)
    return lists.cpu().numpy(), codes.cpu().numpy()


def _trained_shard(trained, ntotal=1):
    from densephrases_amd import Shard
    return Shard.pq_from_trained(trained, ntotal, device=0)


def _finalize(s):
    n = s.ntotal
    s.set_idx2id(np.zeros(n, np.int32), np.arange(n, dtype=np.int32))
    s.set_f2o(np.zeros(1, np.int32), np.asarray([0, n], np.int64), np.arange(n, dtype=np.int32))
    s.finalize()
    return s


def _assert_equal_to_ref(lists, codes, ref, what):
    bad_rows = np.nonzero(lists != ref["lists"])[0]
    bad_cells = np.argwhere(codes != ref["codes"])
    print(f"{what}: {len(bad_rows)} of {len(lists)} lists differ, {len(bad_cells)} of {codes.size} cells differ")
    assert len(bad_rows) == 0, (what, bad_rows[:10], lists[bad_rows[:10]], ref["lists"][bad_rows[:10]])
    assert len(bad_cells) == 0, (what, bad_cells[:10])


# ------------------------------------------------------------------------------------------------- 1. pq_encode_dev
@pytest.mark.parametrize("i", range(len(R.SETS)))
def test_encode_equals_the_restatement_on_the_four_sets(i):
    _, trained, xb, ref = R.input_set(i)
    s = _trained_shard(trained)
    _assert_equal_to_ref(*_encode(s, xb), ref, f"set {i + 1}")
    s.close()


@functools.lru_cache(maxsize=None)
def _variant(name):
    """(trained index, rows, restatement) of a variant of one of the sets, 300 rows each"""
    base = {"no_residual": 3, "bias": 0, "not_a_rotation": 2, "no_transform": 1}[name]
    _, trained, xb, _ = R.input_set(base)
    t = copy.copy(trained)
    t.index = copy.copy(trained.index)
    rng = np.random.default_rng(11)
    if name == "no_residual":
        t.index.by_residual = False
    elif name == "bias":
        t.chain = [F.LinearTransform(trained.chain[0].A, rng.normal(0, 0.2, 768).astype(np.float32))]
    elif name == "not_a_rotation":
        A = trained.chain[0].A.astype(np.float64) * rng.uniform(0.5, 1.5, (768, 1)) + rng.normal(0, 0.01, (768, 768))
        t.chain = [F.LinearTransform(A.astype(np.float32))]
    elif name == "no_transform":
        t = t.index                                         # a bare IndexIVFPQ: no A at all
    x = np.array(xb[:300])
    return t, x, R.encode(t, x)


@pytest.mark.parametrize("name", ["no_residual", "bias", "not_a_rotation", "no_transform"])
def test_encode_variants_no_residual_bias_general_matrix_no_transform(name):
    t, x, ref = _variant(name)
    s = _trained_shard(t)
    _assert_equal_to_ref(*_encode(s, x), ref, name)
    s.close()


@pytest.mark.parametrize("M", [32, 16])
def test_encode_the_wide_sub_quantisers(M):
    """dsub = 24 and 48: the two kernel instances the four sets (dsub 8, 16, 6, 12) do not reach"""
    from tests._pq_build import _random_index
    ix, xb, _ = _random_index(20 + M, 400, 5, M=M)
    trained = R.empty_copy(ix)
    ref = R.encode(trained, xb)
    codes, ids = R.build_lists(ref["lists"], ref["codes"], np.arange(400), 5)
    for l in range(5):                                      # (the restatement against the oracle for these two as well)
        np.testing.assert_array_equal(codes[l], np.asarray(ix.index.list_codes[l]))
        np.testing.assert_array_equal(ids[l], np.asarray(ix.index.list_ids[l]))
    assert not ref["exempt_rows"].any() and not ref["exempt_cells"].any()
    s = _trained_shard(trained)
    _assert_equal_to_ref(*_encode(s, xb), ref, f"M = {M}")
    s.close()


def test_encode_row_counts_around_the_block_chunks_and_a_filled_handle():
    ix, trained, xb, ref = R.input_set(0)
    s = _trained_shard(trained)
    for n in (1, 127, 128, 129):
        sub = {k: v[:n] for k, v in ref.items()}
        _assert_equal_to_ref(*_encode(s, xb[:n]), sub, f"n = {n}")
    _assert_equal_to_ref(*_encode(s, xb, chunks=[517, 1, 782]), ref, "three uneven chunks")
    s.close()
    from tests._pq_build import _shard
    full = _shard(ix)                                       # a handle that already holds codes: encoding is a pure function of the parameters
    q = np.array(xb[:16])
    before = full.search_ivf(q, 10, 4)
    _assert_equal_to_ref(*_encode(full, xb), ref, "filled handle")
    after = full.search_ivf(q, 10, 4)
    np.testing.assert_array_equal(before[0], after[0])
    np.testing.assert_array_equal(before[1], after[1])
    full.close()


# ------------------------------------------------------------------------------------------------- 2. non-finite rows
def test_nan_and_inf_rows_get_list_minus_one_zero_codes_and_are_refused_downstream():
    import torch
    from densephrases_amd._lib import DphError
    from densephrases_amd.pq_build import add_with_ids_resident
    _, trained, xb, ref = R.input_set(2)
    n = 300
    x = np.array(xb[:n])
    x[7, 100] = np.nan
    x[130, 767] = np.inf
    x[131, 0] = -np.inf
    bad = np.asarray([7, 130, 131])
    s = _trained_shard(trained, ntotal=n)
    lists, codes = _encode(s, x)
    assert (lists[bad] == -1).all() and not codes[bad].any()
    keep = np.setdiff1d(np.arange(n), bad)
    np.testing.assert_array_equal(lists[keep], ref["lists"][keep])
    np.testing.assert_array_equal(codes[keep], ref["codes"][keep])
    dev = torch.device("cuda", 0)
    lt, ct, it = torch.from_numpy(lists).to(dev), torch.from_numpy(codes).to(dev), torch.arange(n, dtype=torch.int64, device=dev)
    with pytest.raises(DphError) as e:
        s.pq_fill_dev(n, lt.data_ptr(), ct.data_ptr(), it.data_ptr())
    assert e.value.code == DPH_E_ARG
    with pytest.raises(DphError):                           # ... and the handle stays unfinalized
        _finalize(s)
    s.close()
    with pytest.raises(ValueError, match="row 7 "):
        add_with_ids_resident(trained, x)


# ------------------------------------------------------------------------------------------------- 3. add_with_ids_resident
def _lists_of(shard):
    sizes = shard.pq_list_sizes()
    codes, ids = shard.pq_download(0, int(sizes.sum()))
    off = np.concatenate([[0], np.cumsum(sizes)])
    return sizes, [codes[off[l]:off[l + 1]] for l in range(len(sizes))], [ids[off[l]:off[l + 1]] for l in range(len(sizes))]


def _assert_lists_equal_index(shard, ix):
    ivf = ix.index
    sizes, codes, ids = _lists_of(shard)
    np.testing.assert_array_equal(sizes, [len(i) for i in ivf.list_ids])
    for l in range(ivf.nlist):
        np.testing.assert_array_equal(ids[l], np.asarray(ivf.list_ids[l]), err_msg=f"list {l}")
        np.testing.assert_array_equal(codes[l], np.asarray(ivf.list_codes[l]), err_msg=f"list {l}")


@pytest.mark.parametrize("i", range(len(R.SETS)))
def test_built_index_equals_the_oracle_index_and_answers_bit_identically(i):
    from densephrases_amd.pq_build import add_with_ids_resident
    from tests._pq_build import _shard
    ix, trained, xb, _ = R.input_set(i)
    nlist = R.SETS[i]["nlist"]
    built = add_with_ids_resident(trained, xb, device=0, block=512)        # (several blocks, the last one partial)
    _assert_lists_equal_index(built, ix)
    _finalize(built)
    want = _shard(ix)
    rng = np.random.default_rng(100 + i)
    q = np.concatenate([xb[rng.choice(len(xb), 24, replace=False)], rng.normal(0, 0.5, (8, 768)).astype(np.float32)])
    for k in (1, 10, 100):
        for nprobe in (1, 4, nlist):
            Dg, Ig = built.search_ivf(q, k, nprobe)
            Dw, Iw = want.search_ivf(q, k, nprobe)
            np.testing.assert_array_equal(Ig, Iw, err_msg=f"k {k} nprobe {nprobe}")
            np.testing.assert_array_equal(Dg.view(np.uint32), Dw.view(np.uint32), err_msg=f"k {k} nprobe {nprobe}")
    for j in rng.choice(len(xb), 20, replace=False):
        np.testing.assert_array_equal(built.reconstruct(int(j)).view(np.uint32), want.reconstruct(int(j)).view(np.uint32))
    D, I = want.search_ivf(q, 10, nlist)
    ids = np.where(I < 0, 0, I)
    for direction in (0, 1):
        args = (direction, q, 10, 7, ids, np.zeros_like(ids, dtype=np.int32), ids.astype(np.int32), D)
        for a, b in zip(built.rescore(*args, want_vecs=True), want.rescore(*args, want_vecs=True)):
            np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))
    built.close()
    want.close()


def test_sparse_and_offset_ids_and_a_duplicate_id_is_refused_at_finalize():
    from densephrases_amd._lib import DphError
    from densephrases_amd.pq_build import add_with_ids_resident
    from tests._pq_build import _shard
    _, trained, xb, _ = R.input_set(3)
    n = len(xb)
    ids = (np.arange(n, dtype=np.int64) * 7 + (1 << 33) + 5)[np.random.default_rng(5).permutation(n)]
    ix = P.add_with_ids(R.empty_copy(trained), xb, ids)
    built = add_with_ids_resident(trained, xb, ids=ids)
    _assert_lists_equal_index(built, ix)
    _finalize(built)
    want = _shard(ix)
    q = np.array(xb[:32])
    for a, b in zip(built.search_ivf(q, 10, 4), want.search_ivf(q, 10, 4)):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))
    for j in (0, 17, n - 1):
        np.testing.assert_array_equal(built.reconstruct(int(ids[j])), want.reconstruct(int(ids[j])))
    built.close()
    want.close()
    dup = ids.copy()
    dup[3] = dup[900]
    s = add_with_ids_resident(trained, xb, ids=dup)
    with pytest.raises(DphError) as e:
        _finalize(s)
    assert e.value.code == DPH_E_ARG and "duplicate" in str(e.value)
    s.close()


# ------------------------------------------------------------------------------------------------- 4. from a resident int8 shard
@pytest.mark.parametrize("kind", [0, 4])
def test_from_a_resident_int8_shard_of_5000_synthetic_rows(kind):
    """the rows are de-quantised on the device through the exact table (ivf._lut_dev); the index is set 4's without its rotation, which
    keeps the float64 restatement of 5000 rows to a few seconds (the rotation is covered above)"""
    from densephrases_amd import Shard
    from densephrases_amd.ivf import dequant
    from densephrases_amd.pq_build import add_with_ids_resident
    from densephrases_amd.synth import synthetic_rows
    _, trained, _, _ = R.input_set(3)
    bare = trained.index
    n = 5000
    flat = Shard(n, device=0)
    flat.fill_synthetic(seed=9, kind=kind)
    rows = synthetic_rows(0, n, seed=9, kind=kind)
    ref = R.encode(bare, dequant(rows))
    assert not ref["exempt_rows"].any() and not ref["exempt_cells"].any()
    built = add_with_ids_resident(bare, flat, block=2048)
    sizes, codes, ids = _lists_of(built)
    want_c, want_i = R.build_lists(ref["lists"], ref["codes"], np.arange(n), bare.nlist)
    for l in range(bare.nlist):
        np.testing.assert_array_equal(ids[l], want_i[l], err_msg=f"list {l}")
        np.testing.assert_array_equal(codes[l], want_c[l], err_msg=f"list {l}")
    built.close()
    flat.close()


# ------------------------------------------------------------------------------------------------- 5. back to a file
def test_built_index_written_to_a_faiss_file_reads_back_and_answers_the_same(tmp_path):
    from densephrases_amd import Shard
    from densephrases_amd.pq_build import add_with_ids_resident
    ix, trained, xb, _ = R.input_set(1)
    built = add_with_ids_resident(trained, xb)
    parsed = built.to_faiss_index(trained)
    assert trained.ntotal == 0 and parsed.ntotal == len(xb)             # the template is left alone
    path = str(tmp_path / "index.faiss")
    F.write_index(parsed, path)
    back = F.read_index(path)
    for l in range(ix.index.nlist):
        np.testing.assert_array_equal(np.asarray(back.index.list_ids[l]), np.asarray(ix.index.list_ids[l]))
        np.testing.assert_array_equal(np.asarray(back.index.list_codes[l]), np.asarray(ix.index.list_codes[l]))
    again = _finalize(Shard.from_faiss_index(back, device=0))
    _finalize(built)
    q = np.array(xb[:40])
    for a, b in zip(built.search_ivf(q, 10, 8), again.search_ivf(q, 10, 8)):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))
    built.close()
    again.close()


# ------------------------------------------------------------------------------------------------- 6. MIPS(pq=...)
def _same(a, b, path="result"):
    if isinstance(a, dict):
        assert isinstance(b, dict) and a.keys() == b.keys(), path
        for k in a:
            _same(a[k], b[k], f"{path}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert isinstance(b, (list, tuple)) and len(a) == len(b), path
        for j, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{path}[{j}]")
    elif isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b), err_msg=path)
    elif isinstance(a, float) and isinstance(b, float) and a != a:
        assert b != b, path
    else:
        assert a == b, (path, a, b)


def test_mips_compressing_the_toy_dump_equals_mips_over_the_file_the_oracle_wrote(tmp_path):
    from densephrases_amd import DocMeta, DocStore, MIPS
    from densephrases_amd.ivf import dequant
    from tests._golden import load_toy_docs
    from tests.test_pq import INDEX_NAME, _pq_cases, _write_pq_layout
    store = DocStore([DocMeta(m.doc_idx, m.title, m.context, m.f2o_start, m.word2char_start, m.word2char_end, m.start)
                      for m in load_toy_docs()])
    xb = dequant(store.rows, store.offset, store.scale)
    trained = P.train(xb, nlist=6, M=96, seed=5)
    filled = P.add_with_ids(R.empty_copy(trained), xb, np.arange(len(xb), dtype=np.int64))
    root = _write_pq_layout(str(tmp_path / "dump"))
    idx_dir = os.path.join(root, "start", INDEX_NAME)
    F.write_index(filled, os.path.join(idx_dir, "index.faiss"))          # in place of the fixture's: the oracle's add over the same rows
    want = MIPS(phrase_dump_dir=os.path.join(root, "phrase"), index_path=os.path.join(idx_dir, "index.faiss"),
                idx2id_path=os.path.join(idx_dir, "idx2id.hdf5"), cuda=True)
    saved = str(tmp_path / "built" / "index.faiss")
    got = MIPS.from_store(store, pq={"trained": trained, "save": saved})
    assert got.index.ntotal == want.index.ntotal == len(xb) and got.pq == want.pq
    np.testing.assert_array_equal(got.R, want.R)
    back = F.read_index(saved)
    for l in range(6):
        np.testing.assert_array_equal(np.asarray(back.index.list_ids[l]), np.asarray(filled.index.list_ids[l]))
        np.testing.assert_array_equal(np.asarray(back.index.list_codes[l]), np.asarray(filled.index.list_codes[l]))
    cases, _ = _pq_cases()
    assert any(c["return_idxs"] for c in cases)
    for c in cases:
        kw = dict(q_texts=[f"q{i}" for i in range(c["B"])], top_k=c["top_k"], aggregate=c["aggregate"], return_idxs=c["return_idxs"],
                  max_answer_length=c["L"], agg_strat=c["agg_strat"], return_sent=c["return_sent"])
        q = c["query_arr"].astype(np.float64)
        _same(got.search(q, **kw), want.search(q, **kw))
    with pytest.raises(ValueError):
        MIPS.from_store(store, pq={"trained": trained}, ivf={"nlist": 4, "nprobe": 2})
    with pytest.raises(ValueError):
        MIPS.from_store(store, pq={"trained": filled})                  # not an empty index
    got.close()
    want.close()


# ------------------------------------------------------------------------------------------------- 7. misuse through the raw ABI
def test_misuse_through_the_raw_abi_is_refused_with_a_code_and_a_message():
    import torch
    from densephrases_amd import Shard, _lib
    lib = _lib.lib
    _, trained, xb, _ = R.input_set(2)
    dev = torch.device("cuda", 0)
    M = trained.index.M
    x = torch.from_numpy(np.array(xb[:8])).to(dev)
    lists = torch.zeros(8, dtype=torch.int32, device=dev)
    codes = torch.zeros((8, M), dtype=torch.uint8, device=dev)
    ids = torch.arange(8, dtype=torch.int64, device=dev)
    vp = C.c_void_p
    sizes = np.zeros(trained.index.nlist, np.int64)
    out_c, out_i = np.zeros((8, M), np.uint8), np.zeros(8, np.int64)

    def calls(h):
        return [lib.dph_pq_encode_dev(h, vp(x.data_ptr()), 8, vp(lists.data_ptr()), vp(codes.data_ptr()), None),
                lib.dph_index_fill_pq_dev(h, 8, vp(lists.data_ptr()), vp(codes.data_ptr()), vp(ids.data_ptr()), None),
                lib.dph_index_get_pq_list_sizes(h, _lib._p(sizes)),
                lib.dph_index_download_pq_codes(h, 0, 8, _lib._p(out_c), _lib._p(out_i))]

    flat = Shard(16, device=0)                                          # a flat handle
    for rc in calls(flat.handle):
        assert rc == DPH_E_STATE and b"not a PQ index" in lib.dph_last_error()
    flat.close()
    h = vp()                                                            # a PQ handle without parameters
    assert lib.dph_index_create_pq(0, 8, trained.index.nlist, M, C.byref(h)) == 0
    for rc in calls(h):
        assert rc == DPH_E_STATE and b"not set" in lib.dph_last_error()
    assert lib.dph_index_destroy(h) == 0
    s = _trained_shard(trained, ntotal=9)                               # n != ntotal
    assert lib.dph_pq_encode_dev(s.handle, vp(x.data_ptr()), 8, vp(lists.data_ptr()), vp(codes.data_ptr()), None) == 0
    rc = lib.dph_index_fill_pq_dev(s.handle, 8, vp(lists.data_ptr()), vp(codes.data_ptr()), vp(ids.data_ptr()), None)
    assert rc == DPH_E_ARG and b"ntotal" in lib.dph_last_error()
    assert lib.dph_index_get_pq_list_sizes(s.handle, _lib._p(sizes)) == DPH_E_STATE       # parameters, but no lists yet
    torch.cuda.synchronize(dev)
    s.close()
