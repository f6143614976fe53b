"""Float64 restatement of the TRAIN step of IndexPreTransform(OPQMatrix) -> IndexIVFPQ as densephrases_amd/pq_train.py and
csrc/dph_pq_train.hip define it, in numpy, sharing no code with them, and the input sets tests/test_pq_train_ref.py and
tests/test_pq_train_gpu.py use (built once per process, never modified).

    code[r][m] = arg-min_j (sum_t w_mj[t]^2 - 2 sum_t x_rm[t] w_mj[t])     float64, t ascending, ties to the lowest j
    e[r]       = sum_t (x[r][t] - w[code][t])^2                            float64, t ascending
    w_mj       = fp32(sum_{r ascending: code[r][m] = j} x_rm / count)      float64; a codeword without members keeps its value
    split      per sub-space: the k-th empty codeword (ascending j) takes the k-th largest one (stable: ties to the lowest j) while that one
               has more than one member; the copies are base * (1 +- 1/1024) on alternating components, in fp32
    OPQ        x' = fp32(x A^T); Lloyd steps; Y = decode; C = Y^T X; U S V^T = svd(C); A = fp32(U V^T)

The arg-min: the distances of a sub-space come from one float64 BLAS product first; every cell whose two best of those differ by less than
NEAR_REL (||x_m||^2 + |d_best|) is decided again from the sequential-t distances of tests/_pq_encode_ref.py, from which the EXEMPT set is
taken with that module's rule (a NONZERO gap below EXEMPT_REL (||x_m||^2 + |d_best|); exact ties are never exempt).  A BLAS distance is off
its sequential value by at most ~dsub 2^-52 (||w||^2 + 2 ||x_m|| ||w||) -- twenty binary orders below the NEAR band -- so outside the band
the two agree on the winner and no exempt cell can lie there."""
import functools

import numpy as np

from tests._pq_encode_ref import EXEMPT_CAP, EXEMPT_REL, _seq_matmul_t, _two_best        # noqa: F401 (re-exported)

try:                                    # (the sub-spaces go to threads of this module's own: a BLAS that threads every small product only gets in their way)
    from threadpoolctl import threadpool_limits as _limits
except ImportError:
    _limits = None


def _one_blas_thread():
    import contextlib
    return _limits(1) if _limits is not None else contextlib.nullcontext()


D = 768
NEAR_REL = 2.0 ** -26
EPS = 1.0 / 1024.0


# ------------------------------------------------------------------------------------------------- the step
def assign(x, pqc):
    """-> (codes uint8 [n,M], exempt bool [n,M]); the sub-spaces are independent and go to a few threads"""
    from concurrent.futures import ThreadPoolExecutor
    x = np.asarray(x, np.float32)
    n, M, dsub = x.shape[0], pqc.shape[0], pqc.shape[2]
    codes = np.zeros((n, M), np.uint8)
    exempt = np.zeros((n, M), bool)

    def one(m):
        w = pqc[m].astype(np.float64)
        rm = x[:, m * dsub:(m + 1) * dsub].astype(np.float64)
        nw = np.zeros(256, np.float64)
        for t in range(dsub):
            nw += w[:, t] * w[:, t]
        scale = (rm * rm).sum(1)
        d = nw[None, :] - 2.0 * (rm @ w.T)
        j1, d1, d2 = _two_best(d, largest=False)
        near = np.nonzero(~(d2 - d1 > NEAR_REL * (scale + np.abs(d1))))[0]
        if near.size:
            ds = nw[None, :] - 2.0 * _seq_matmul_t(rm[near], w)
            k1, e1, e2 = _two_best(ds, largest=False)
            j1[near] = k1
            g = e2 - e1
            exempt[near, m] = (g != 0) & (g < EXEMPT_REL * (scale[near] + np.abs(e1)))
        codes[:, m] = j1

    with _one_blas_thread(), ThreadPoolExecutor(max_workers=8) as ex:
        list(ex.map(one, range(M)))
    return codes, exempt


def decode(codes, pqc):
    n, M = codes.shape
    return np.concatenate([pqc[m][codes[:, m]] for m in range(M)], axis=1).astype(np.float32)


def row_err(x, codes, pqc):
    d = np.asarray(x, np.float32).astype(np.float64) - decode(codes, pqc).astype(np.float64)
    e = np.zeros(d.shape[0], np.float64)
    for t in range(d.shape[1]):
        e += d[:, t] * d[:, t]
    return e


def update(x, codes, pqc):
    """-> (new codebooks fp32 [M,256,dsub], counts int64 [M,256]); the member sums run over the rows in ascending order, one add each"""
    x = np.asarray(x, np.float32)
    n, M = codes.shape
    dsub = pqc.shape[2]
    cell = (np.arange(M, dtype=np.int64)[None, :] * 256 + codes).T.reshape(-1)              # m-major: entry m n + r
    row = np.tile(np.arange(n, dtype=np.int64), M)
    order = np.argsort(cell, kind="stable")                                                 # by cell, rows ascending inside
    counts = np.bincount(cell, minlength=M * 256)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    vals = x.reshape(n, M, dsub).astype(np.float64)[row[order], cell[order] // 256]         # [n M, dsub]
    acc = np.zeros((M * 256, dsub), np.float64)
    for k in range(int(counts.max())):
        live = np.nonzero(counts > k)[0]
        acc[live] += vals[starts[live] + k]
    new = pqc.reshape(M * 256, dsub).copy()
    has = counts > 0
    new[has] = (acc[has] / counts[has, None].astype(np.float64)).astype(np.float32)
    return new.reshape(M, 256, dsub), counts.reshape(M, 256)


def step(x, pqc, do_update=True):
    """dph_pq_train_step_dev restated -> dict(codes, exempt, counts, row_err, pqc (new codebooks, or the input with do_update False))"""
    pqc = np.asarray(pqc, np.float32)
    codes, exempt = assign(x, pqc)
    err = row_err(x, codes, pqc)
    new, counts = update(x, codes, pqc)
    return dict(codes=codes, exempt=exempt, counts=counts, row_err=err, pqc=new if do_update else pqc.copy())


def split_empty(pqc, counts):
    """in place; -> codewords split"""
    M, _, dsub = pqc.shape
    sign = np.ones(dsub, np.float32)
    sign[1::2] = -1.0
    up, down = np.float32(1.0) + np.float32(EPS) * sign, np.float32(1.0) - np.float32(EPS) * sign
    done = 0
    for m in range(M):
        empties = np.nonzero(counts[m] == 0)[0]
        if not empties.size:
            continue
        donors = np.argsort(-counts[m].astype(np.int64), kind="stable")
        for k, j in enumerate(empties):
            d = donors[k]
            if counts[m, d] > 1:
                base = pqc[m, d].copy()
                pqc[m, j] = base * up
                pqc[m, d] = base * down
                done += 1
    return done


def lloyd(x, pqc, steps):
    """-> (codes, exempt of the closing assignment, mean error of it, per-step errors, new codebooks, share of exempt cells over all assignments)"""
    pqc = np.array(pqc, np.float32)
    errs, n_ex, n_cells = [], 0, 0
    for _ in range(int(steps)):
        s = step(x, pqc)
        errs.append(float(s["row_err"].sum()) / len(x))
        n_ex, n_cells = n_ex + int(s["exempt"].sum()), n_cells + s["exempt"].size
        pqc = s["pqc"]
        split_empty(pqc, s["counts"])
    codes, exempt = assign(x, pqc)
    n_ex, n_cells = n_ex + int(exempt.sum()), n_cells + exempt.size
    return codes, exempt, float(row_err(x, codes, pqc).sum()) / len(x), errs, pqc, n_ex / n_cells


def rotate(x, A):
    return (np.asarray(x, np.float32).astype(np.float64) @ np.asarray(A, np.float32).astype(np.float64).T).astype(np.float32)


def init_codebooks(x, init):
    M = init.shape[0]
    dsub = D // M
    xs = np.asarray(x, np.float32).reshape(len(x), M, dsub)
    return np.stack([xs[init[m], m] for m in range(M)])


def opq_iteration(x, A, pqc, steps, xp=None):
    """one iteration of the alternation; ``xp``: the rotated rows to use instead of ``rotate(x, A)`` (a device run's, so that everything
    behind the rotation can be compared bit for bit)"""
    xp = rotate(x, A) if xp is None else np.asarray(xp, np.float32)
    codes, exempt, err, _, pqc, share = lloyd(xp, pqc, steps)
    y = decode(codes, pqc)
    Cm = y.astype(np.float64).T @ np.asarray(x, np.float32).astype(np.float64)
    U, _, Vt = np.linalg.svd(Cm)
    return dict(xp=xp, codes=codes, exempt=exempt, err=err, pqc=pqc, C=Cm, A_new=(U @ Vt).astype(np.float32), exempt_share=share)


def random_orthonormal(rng):
    q, r = np.linalg.qr(rng.normal(size=(D, D)))
    return (q * np.sign(np.diag(r))[None, :]).astype(np.float32)


def opq(x, M, A0, init, iters, steps_first, steps):
    """-> (A, codebooks, per-iteration errors, largest exempt share of an iteration)"""
    A, pqc, errs, share = A0, None, [], 0.0
    for it in range(iters):
        if pqc is None:
            pqc = init_codebooks(rotate(x, A), init)
        o = opq_iteration(x, A, pqc, steps_first if it == 0 else steps)
        A, pqc = o["A_new"], o["pqc"]
        errs.append(o["err"])
        share = max(share, o["exempt_share"])
    return A, pqc, errs, share


def train(x, centroids, M, A0, init_opq, init_pq, opq_iters, pq_iters_first, pq_iters, final_pq_iters):
    """the whole trainer over the set x with the coarse centroids given -> dict(A, pqc, opq_err, pq_err, final_err, exempt_share)"""
    A, _, opq_err, share = opq(x, M, A0, init_opq, opq_iters, pq_iters_first, pq_iters)
    xp = rotate(x, A)
    cent = np.asarray(centroids, np.float32)
    lists = np.argmax(xp.astype(np.float64) @ cent.astype(np.float64).T, axis=1)
    res = (xp - cent[lists]).astype(np.float32)
    _, _, final_err, pq_err, pqc, share2 = lloyd(res, init_codebooks(res, init_pq), final_pq_iters)
    return dict(A=A, pqc=pqc, opq_err=opq_err, pq_err=pq_err, final_err=final_err, exempt_share=max(share, share2))


def training_error(x, A, centroids, pqc):
    """mean over the rows of ||r - decode(encode(r))||^2, r = fp32(fp32(x A^T) - c_list): float64 from the parts of a trained index"""
    xp = rotate(x, A)
    cent = np.asarray(centroids, np.float32)
    lists = np.argmax(xp.astype(np.float64) @ cent.astype(np.float64).T, axis=1)
    res = (xp - cent[lists]).astype(np.float32)
    codes, _ = assign(res, np.asarray(pqc, np.float32))
    return float(row_err(res, codes, np.asarray(pqc, np.float32)).sum()) / len(x)


# ------------------------------------------------------------------------------------------------- input sets
def quantise(x, offset=-2.0, scale=20.0):
    return np.clip(np.rint((x - offset) * scale), -128, 127).astype(np.int8)


def dequant(rows, offset=-2.0, scale=20.0):
    return rows.astype(np.float32) / np.float32(scale) + np.float32(offset)


@functools.lru_cache(maxsize=None)
def anisotropic_rows(n, seed=7):
    """de-quantised int8 rows of the dump's codec: decaying axis variances under a fixed orthogonal mix (what OPQ is for)"""
    rng = np.random.default_rng(seed)
    mix = random_orthonormal(np.random.default_rng(1234)).astype(np.float64)
    sigma = 0.15 + 1.2 * np.exp(-np.arange(D) / 60.0)
    x = dequant(quantise((rng.normal(size=(n, D)) * sigma[None, :]) @ mix))
    x.setflags(write=False)
    return x


def _codebooks_from_rows(x, M, rng):
    n = len(x)
    return init_codebooks(x, np.stack([rng.choice(n, 256, replace=n < 256) for _ in range(M)]))


STEP_CASES = ["n1", "n129", "n255", "n4097", "identical", "duplicates", "M128", "M16"]


@functools.lru_cache(maxsize=None)
def step_case(name):
    """(x [n,768] fp32, codebooks [M,256,dsub] fp32, restatement of the step with update) of a case of the direct step test"""
    rng = np.random.default_rng(STEP_CASES.index(name) + 50)
    pool = anisotropic_rows(4097)
    M = {"M128": 128, "M16": 16}.get(name, 96)
    n = {"n1": 1, "n129": 129, "n255": 255, "n4097": 4097, "identical": 300, "duplicates": 600, "M128": 700, "M16": 300}[name]
    x = np.array(pool[:n])
    pqc = _codebooks_from_rows(pool, M, rng)
    if name == "identical":
        x[:] = x[0]
    if name == "duplicates":
        x[100:200] = x[:100]                                # duplicated rows ...
        x[599] = x[0]
        pqc[:, 9] = pqc[:, 5]                               # ... and duplicated codewords: exact ties, the lowest j wins
        pqc[:, 200] = pqc[:, 5]
        pqc[::2, 0] = pqc[::2, 255]
    x.setflags(write=False)
    pqc.setflags(write=False)
    return x, pqc, step(x, pqc)


OPQ_CASE = dict(n=4096, M=96, steps=3, seed=3)


@functools.lru_cache(maxsize=None)
def opq_case_inputs():
    """(x, A_0, start codebooks) of the one-iteration test"""
    x = anisotropic_rows(4097)[:OPQ_CASE["n"]]
    rng = np.random.default_rng(OPQ_CASE["seed"])
    A0 = random_orthonormal(rng)
    init = np.stack([rng.choice(len(x), 256, replace=False) for _ in range(OPQ_CASE["M"])])
    return x, A0, init_codebooks(rotate(x, A0), init)


TRAINER_CASE = dict(n=4096, nlist=16, M=96, opq_iters=3, pq_iters_first=8, pq_iters=2, final_pq_iters=5, seed=0)


@functools.lru_cache(maxsize=None)
def trainer_case_inputs():
    """(rows fp32 [4096,768], centroids [16,768]: 16 of the rows) of the whole-trainer test"""
    x = anisotropic_rows(4097)[:TRAINER_CASE["n"]]
    cent = np.array(x[np.random.default_rng(99).choice(len(x), TRAINER_CASE["nlist"], replace=False)])
    cent.setflags(write=False)
    return x, cent


def draw_seeds(seed, n_set, M):
    """the trainer's draws (densephrases_amd.pq_train.draw_seeds restated: one generator, A_0, then the two sets of start rows)"""
    rng = np.random.default_rng(seed)
    A0 = random_orthonormal(rng)
    init_opq = np.stack([rng.choice(n_set, 256, replace=False) for _ in range(M)])
    init_pq = np.stack([rng.choice(n_set, 256, replace=False) for _ in range(M)])
    return A0, init_opq, init_pq


@functools.lru_cache(maxsize=None)
def trainer_restatement(seed=None):
    """the restated trainer over TRAINER_CASE from ``seed`` (default: the case's own), once per process"""
    T = TRAINER_CASE
    x, cent = trainer_case_inputs()
    A0, init_opq, init_pq = draw_seeds(T["seed"] if seed is None else seed, len(x), T["M"])
    return train(x, cent, T["M"], A0, init_opq, init_pq, T["opq_iters"], T["pq_iters_first"], T["pq_iters"], T["final_pq_iters"])
