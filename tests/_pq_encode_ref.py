"""Float64 restatement of the ADD step of IndexPreTransform(OPQMatrix) -> IndexIVFPQ (build_phrase_index.py:145-153) with every sum taken
SEQUENTIALLY in t -- the definition densephrases_amd/csrc/dph_pq_encode.hip is held to -- sharing no code with oracle/ivfpq_oracle.py, and
the four input sets both test files use (built once per process).

    x'      = fp32(sum_t A[j,t] x[t] + b[j])                 float64, t ascending, one rounding
    list    = arg-max_l sum_t x'[t] c_l[t]                   float64, t ascending, ties to the lowest list
    r       = fp32(x' - c_list)  (by_residual) else x'       one fp32 subtraction
    code[m] = arg-min_j (sum_t w_mj[t]^2 - 2 sum_t r_m[t] w_mj[t])   float64, t ascending, ties to the lowest j

The EXEMPT set: a row whose two best list scores differ by a NONZERO amount below 2^-40 |best|, a cell whose two best distances differ by
a nonzero amount below 2^-40 (||r_m||^2 + |d_best|) -- float64 summation orders may disagree there, an implementation may too.  Exact
ties are never exempt: the lowest index wins."""
import copy
import functools

import numpy as np

SETS = [dict(seed=1, n=1300, nlist=12, M=96, dup=0), dict(seed=2, n=700, nlist=300, M=48, dup=5),
        dict(seed=3, n=900, nlist=7, M=128, dup=0), dict(seed=4, n=1000, nlist=33, M=64, dup=3)]
EXEMPT_REL = 2.0 ** -40
EXEMPT_CAP = 1e-3                       # of the rows and of the cells of a set


def _parts(index):
    ivf = getattr(index, "index", index)
    A = b = None
    chain = getattr(index, "chain", None)
    if chain:
        assert len(chain) == 1
        A, b = chain[0].A, chain[0].b
    return ivf, A, b


def empty_copy(index):
    """the TRAINED index: same parameters, no vectors"""
    ivf = copy.copy(getattr(index, "index", index))
    ivf.list_codes = [np.zeros((0, ivf.M), np.uint8) for _ in range(ivf.nlist)]
    ivf.list_ids = [np.zeros(0, np.int64) for _ in range(ivf.nlist)]
    if not hasattr(index, "index"):
        return ivf
    out = copy.copy(index)
    out.index = ivf
    return out


def _seq_matmul_t(x64, w64):
    """[n, k] . [j, k]^T with the sum over k taken sequentially, in float64"""
    acc = np.zeros((x64.shape[0], w64.shape[0]), np.float64)
    for t in range(x64.shape[1]):
        acc += x64[:, t, None] * w64[None, :, t]
    return acc


def transform(index, x):
    ivf, A, b = _parts(index)
    x = np.asarray(x, np.float32)
    if A is None:
        return x.copy()
    y = _seq_matmul_t(x.astype(np.float64), np.asarray(A, np.float32).astype(np.float64))
    if b is not None:
        y = y + np.asarray(b, np.float32).astype(np.float64)[None, :]
    return y.astype(np.float32)


def _two_best(v, largest):
    """(index of the best of every row -- ties to the lowest --, best value, runner-up value)"""
    n = v.shape[0]
    s = -v if largest else v
    i1 = np.argmin(s, 1)
    best = s[np.arange(n), i1]
    s2 = s.copy()
    s2[np.arange(n), i1] = np.inf
    second = s2.min(1) if s.shape[1] > 1 else np.full(n, np.inf)
    return i1, (-best if largest else best), (-second if largest else second)


def encode(index, x):
    """-> dict(lists int64 [n] (-1: non-finite row), codes uint8 [n, M], exempt_rows bool [n], exempt_cells bool [n, M])"""
    ivf, A, b = _parts(index)
    x = np.asarray(x, np.float32)
    n, M, dsub = x.shape[0], ivf.M, ivf.d // ivf.M
    finite = np.isfinite(x).all(1)
    xs = np.where(finite[:, None], x, np.float32(0))
    with np.errstate(all="ignore"):
        xp = transform(index, xs)
        cent = np.asarray(ivf.centroids, np.float32)
        sc = _seq_matmul_t(xp.astype(np.float64), cent.astype(np.float64))
        lists, s1, s2 = _two_best(sc, largest=True)
        gap = s1 - s2
        exempt_rows = (gap != 0) & (gap < EXEMPT_REL * np.abs(s1))
        res = (xp - cent[lists]).astype(np.float32) if ivf.by_residual else xp
        codes = np.zeros((n, M), np.uint8)
        exempt_cells = np.zeros((n, M), bool)
        for m in range(M):
            w = np.asarray(ivf.pq_centroids[m], np.float32).astype(np.float64)            # [256, dsub]
            nw = np.zeros(w.shape[0], np.float64)
            for t in range(dsub):
                nw += w[:, t] * w[:, t]
            rm = res[:, m * dsub:(m + 1) * dsub].astype(np.float64)
            d = nw[None, :] - 2.0 * _seq_matmul_t(rm, w)
            j1, d1, d2 = _two_best(d, largest=False)
            codes[:, m] = j1
            g = d2 - d1
            exempt_cells[:, m] = (g != 0) & (g < EXEMPT_REL * ((rm * rm).sum(1) + np.abs(d1)))
    lists = np.where(finite, lists, -1).astype(np.int64)
    codes[~finite] = 0
    exempt_rows &= finite
    exempt_cells &= finite[:, None]
    return dict(lists=lists, codes=codes, exempt_rows=exempt_rows, exempt_cells=exempt_cells)


def build_lists(lists, codes, ids, nlist):
    """per-list (codes, ids) in input order: FAISS' append order"""
    lists, ids = np.asarray(lists), np.asarray(ids, np.int64)
    out_c, out_i = [], []
    for l in range(nlist):
        sel = np.nonzero(lists == l)[0]
        out_c.append(codes[sel])
        out_i.append(ids[sel])
    return out_c, out_i


@functools.lru_cache(maxsize=None)
def input_set(i):
    """(oracle-filled index, trained empty index, rows xb [n,768] fp32, restatement of the rows) of SETS[i]; built once per process and
    never modified by the tests"""
    from tests._pq_build import _random_index
    s = SETS[i]
    ix, xb, _ = _random_index(s["seed"], s["n"], s["nlist"], M=s["M"], dup=s["dup"])
    trained = empty_copy(ix)
    ref = encode(trained, xb)
    xb.setflags(write=False)
    return ix, trained, xb, ref
