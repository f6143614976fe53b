"""The input sets of the direct window re-score tests (tests/test_window_direct.py on the GPU, tests/test_window_ref.py
without one): shard contents, documents, candidate batches.  numpy and the oracle only, so that the restatement can be
run over every set on a machine without a GPU.  Everything is a pure function of its arguments (fixed seeds)."""
import functools
from types import SimpleNamespace

import numpy as np

from oracle import ivfpq_oracle as P
from oracle import mips_oracle as O
from tests._window_ref import DIM, window_ref

FLT_MAX = np.float32(3.4028234663852886e38)

# ------------------------------------------------------------------------------------------------- raw-dump shard
N_ROWS, ID_BASE = 700, 1000                       # 700: not a multiple of the 32-row tile
DOC_IDS = [3, 4, 10, 500, 2_000_000]
DOC_LEN = [1, 40, 60, 50, 549]                    # one token | constant f2o | steps of L and L + 1 | decreasing steps | plain
DOC_ROW0 = np.concatenate([[0], np.cumsum(DOC_LEN)]).tolist()
RUNS = [(200, 4), (347, 5), (696, 3)]             # (first row, length) of byte-identical rows; 347..351 straddles the cut at 350
SATURATED = (10, 11)                              # +127 / -128 in every component
CUT = 350
GROUP_OFFSETS = [0, 10 ** 9, 3 * 10 ** 9]
GROUP_ROWS = [0, 200, 350, 700]                   # unequal sizes 200 / 150 / 350
N_LISTS, EMPTY_LIST = 7, 3

# (n_q, k), L: every L with a partial last workgroup (n_q * k not a multiple of 4), every shape with L = 10; L = 65 passes the
# staging point of the window kernel at every 64th slot
RAW_SHAPES = [((1, 1), 1), ((1, 1), 10), ((1, 3), 2), ((1, 3), 10), ((1, 3), 33), ((3, 4), 10), ((5, 7), 1), ((5, 7), 10),
              ((5, 7), 20), ((5, 7), 33), ((5, 7), 65), ((64, 10), 10), ((64, 10), 33)]
L_ALL = (1, 2, 10, 20, 33)


@functools.lru_cache(maxsize=None)
def raw_rows():
    rng = np.random.default_rng(2024)
    rows = rng.integers(-128, 128, (N_ROWS, DIM)).astype(np.int8)
    for r0, n in RUNS:
        rows[r0:r0 + n] = rows[r0]
    rows[SATURATED[0]] = 127
    rows[SATURATED[1]] = -128
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def raw_vectors():
    v = O.int8_to_float(raw_rows())
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def raw_meta(L):
    """idx2id and the f2o CSR of the five documents; the steps of document 10 depend on the L under test"""
    rng = np.random.default_rng(77)
    pattern = [L, 0, 1, L + 1, 0, 0, 1, 1, max(L - 1, 0), 2]
    f2o = [np.asarray([7]),
           np.full(40, 5),
           np.concatenate([[0], np.cumsum([pattern[i % len(pattern)] for i in range(59)])]),
           100 + np.concatenate([[0], np.cumsum(rng.choice([1, 1, 2, 0, -1, -3], 49))]),
           np.concatenate([[0], np.cumsum(rng.choice([0, 1, 1, 2], 548))])]
    assert [len(a) for a in f2o] == DOC_LEN and (np.diff(f2o[3]) < 0).any()
    return SimpleNamespace(doc_ids=np.asarray(DOC_IDS, np.int32), f2o_off=np.asarray(DOC_ROW0, np.int64),
                           f2o=np.concatenate(f2o).astype(np.int32),
                           row2doc=np.repeat(np.asarray(DOC_IDS, np.int32), DOC_LEN),
                           row2word=np.concatenate([np.arange(n, dtype=np.int32) for n in DOC_LEN]))


def clip_docword(meta, local, n=N_ROWS):
    """what get_idxs / dph_id2docword answer: idx2id of the local id clipped into the shard"""
    l = np.clip(np.asarray(local, np.int64), 0, n - 1)
    return meta.row2doc[l].astype(np.int32), meta.row2word[l].astype(np.int32)


def raw_edges(meta, rng, undecidable):
    """(id, doc, word, first or None): ids around both ends of the shard and far away, words around both ends of
    every document, documents around and between the CSR's entries, FAISS padding, saturated rows, every phase of
    the L / L + 1 steps and the decreasing steps; (doc, word) mostly NOT those of the id"""
    def dw(i):
        d, w = clip_docword(meta, i - ID_BASE)
        return int(d), int(w)
    E = []
    for i in (-1, ID_BASE - 1, ID_BASE, ID_BASE + N_ROWS - 1, ID_BASE + N_ROWS, 2 ** 40):
        E.append((i, *dw(i), None))
        E.append((i, 2_000_000, 17, None))
    E.append((-1, -1, -1, -FLT_MAX))
    if undecidable:
        # padding as MIPS.search sends it: (doc, word) of the clipped id.  -FLT_MAX absorbs dot and mask alike, every slot scores
        # the same while their validity differs: the one kind of candidate the acceptance rule leaves out (batches of >= 200 only)
        E.append((-1, *dw(-1), -FLT_MAX))
    inside = lambda: ID_BASE + int(rng.integers(0, N_ROWS))
    for d, flen in zip(DOC_IDS, DOC_LEN):
        for w in (-1, 0, flen - 1, flen):
            E.append((inside(), d, w, None))
    for d in (-1, 1, 7, 3_000_000, 3, 2_000_000):
        E.append((inside(), d, 0, None))
    for r in SATURATED:
        E.append((ID_BASE + r, *dw(ID_BASE + r), None))
    for w in range(12):
        E.append((ID_BASE + DOC_ROW0[2] + w, 10, w, None))
    for w in range(3, 50, 6):
        E.append((inside(), 500, w, None))
    return E


def _plant_ties(rng, q, ids, doc, word, k, direction, meta, id_of_row):
    """query rows 1 and 2 point along a run of identical rows; their first two candidates start a window on it, once with
    the (doc, word) of the id and once in the constant-f2o document (every slot valid): the first of the run must win"""
    vec = raw_vectors()
    for r, (r0, n) in zip((1, 2), RUNS):
        if r >= q.shape[0]:
            break
        q[r] = (0.02 * vec[r0] + rng.normal(0, 0.05, DIM)).astype(np.float32)
        row = r0 if direction == 0 else r0 + n - 1
        for j, dw in enumerate(((int(meta.row2doc[row]), int(meta.row2word[row])), (4, 10))[:k]):
            c = r * k + j
            ids[c], doc[c], word[c] = id_of_row(row), dw[0], dw[1]


def raw_batch(n_q, k, L, direction, seed=0):
    rng = np.random.default_rng([seed, n_q, k, L, direction])
    meta = raw_meta(L)
    n = n_q * k
    local = rng.integers(0, N_ROWS, n)
    ids = (ID_BASE + local).astype(np.int64)
    doc, word = meta.row2doc[local].copy(), meta.row2word[local].copy()
    first = rng.normal(50, 5, n).astype(np.float32)
    q = rng.normal(0, 0.5, (n_q, DIM)).astype(np.float32)
    E = raw_edges(meta, rng, undecidable=n >= 200)
    where = rng.permutation(n)[:min(len(E), 2 * n // 3)]
    for c, e in zip(where, rng.permutation(len(E))):
        ids[c], doc[c], word[c] = E[e][:3]
        if E[e][3] is not None:
            first[c] = E[e][3]
    _plant_ties(rng, q, ids, doc, word, k, direction, meta, lambda row: ID_BASE + row)
    return SimpleNamespace(n_q=n_q, k=k, L=L, direction=direction, q=q, ids=ids, doc=doc, word=word, first=first, meta=meta)


def gap_batch(L, direction):
    """35 candidates, one at each of the first 35 words of document 10 (steps L, 0, 1, L + 1, ...): windows whose last
    valid slot is exactly L away, whose first invalid slot L + 1; and 7 words of the document with decreasing steps"""
    b = raw_batch(5, 7, L, direction, seed=5)
    n = 35
    b.doc[:] = 10
    b.word[:] = np.arange(n)
    b.ids[:] = ID_BASE + DOC_ROW0[2] + np.arange(n)
    b.doc[28:], b.word[28:] = 500, np.arange(10, 45, 5)
    b.first[:] = np.random.default_rng(L).normal(50, 5, n).astype(np.float32)
    return b


def invalid_batch(L, direction):
    """no slot of any candidate is valid: unknown / negative documents, words outside the document"""
    b = raw_batch(5, 7, L, direction, seed=6)
    docs = [-1, 1, 7, 3_000_000, 4, 10, 2_000_000]
    for c in range(35):
        b.ids[c] = ID_BASE + (c * 53) % N_ROWS if c % 5 else ID_BASE + N_ROWS + c      # a few outside the shard: zero vectors
        b.doc[c] = docs[c % 7]
        b.word[c] = 0 if c % 7 < 4 else (-1 - c % 3 if c % 2 else DOC_LEN[DOC_IDS.index(docs[c % 7])] + c % 3)
    b.first[:] = np.random.default_rng(L + 100).normal(50, 5, 35).astype(np.float32)
    return b


def flat_lookup(lo=0, hi=N_ROWS, id_base=ID_BASE):
    """vec_of / held of the shard that stores rows [lo, hi) under ids id_base + row"""
    vec = raw_vectors()

    def vec_of(i):
        return vec[i - id_base] if lo <= i - id_base < hi else None
    return vec_of, lambda i: lo <= i - id_base < hi


def group_of(i):
    for g, off in enumerate(GROUP_OFFSETS):
        if off <= i < off + GROUP_ROWS[g + 1] - GROUP_ROWS[g]:
            return GROUP_ROWS[g] + i - off
    return -1


def group_lookup():
    vec = raw_vectors()
    return (lambda i: vec[group_of(i)] if group_of(i) >= 0 else None), (lambda i: group_of(i) >= 0)


def group_batch(L, direction):
    """three id groups with 64-bit offsets: windows that leave a group into the hole behind (or before) it, candidates
    in the holes, below the first offset and beyond the last group"""
    rng = np.random.default_rng([9, L, direction])
    meta = raw_meta(L)
    n_q, k = 5, 7
    ids = []
    for g, off in enumerate(GROUP_OFFSETS):
        size = GROUP_ROWS[g + 1] - GROUP_ROWS[g]
        ids += [off, off + 1, off + size - 2, off + size - 1, off + size, off + size + 3, off - 1, off - 2]
    ids += [-7, 2 * 10 ** 9, 2 ** 40, 10 ** 9 + 149, 3 * 10 ** 9 + 349]
    while len(ids) < n_q * k:
        g = int(rng.integers(0, 3))
        ids.append(GROUP_OFFSETS[g] + int(rng.integers(0, GROUP_ROWS[g + 1] - GROUP_ROWS[g])))
    ids = np.asarray(ids[:n_q * k], np.int64)
    rows = np.asarray([group_of(int(i)) for i in ids])
    doc, word = clip_docword(meta, np.where(rows >= 0, rows, rng.integers(0, N_ROWS, len(ids))))
    first = rng.normal(50, 5, len(ids)).astype(np.float32)
    q = rng.normal(0, 0.5, (n_q, DIM)).astype(np.float32)
    return SimpleNamespace(n_q=n_q, k=k, L=L, direction=direction, q=q, ids=ids, doc=doc, word=word, first=first, meta=meta)


@functools.lru_cache(maxsize=None)
def list_assignment():
    """a random list for every row, list EMPTY_LIST gets none: neighbouring ids lie in different lists, every list ends in padding"""
    a = np.random.default_rng(31).integers(0, N_LISTS - 1, N_ROWS).astype(np.int32)
    a[a >= EMPTY_LIST] += 1
    assert set(a.tolist()) == set(range(N_LISTS)) - {EMPTY_LIST}
    return a


def list_batch(L, direction):
    """the first and the last id of every list (the rows next to another list's padding), then the mixed batch"""
    b = raw_batch(5, 7, L, direction, seed=7)
    a = list_assignment()
    c = 14                                           # (the planted ties of query rows 1 and 2 stay)
    for l in sorted(set(a.tolist())):
        for row in (int(np.nonzero(a == l)[0][0]), int(np.nonzero(a == l)[0][-1])):
            b.ids[c], b.doc[c], b.word[c], b.first[c] = ID_BASE + row, b.meta.row2doc[row], b.meta.row2word[row], 50 + l
            c += 1
    return b


def cut_batch(L, direction):
    """candidates within L of the cut between the shards [0, CUT) and [CUT, N_ROWS), on both sides"""
    b = raw_batch(5, 7, L, direction, seed=8)
    rows = np.clip(CUT + np.asarray([(-1) ** c * ((c * L) // 34 + c % 2) for c in range(35)]), 0, N_ROWS - 1)
    rows[:6] = [CUT - 1, CUT, CUT - L, CUT + L - 1, RUNS[1][0], RUNS[1][0] + RUNS[1][1] - 1]
    rows = np.clip(rows, 0, N_ROWS - 1)
    b.ids[:] = ID_BASE + rows
    b.doc[:], b.word[:] = b.meta.row2doc[rows], b.meta.row2word[rows]
    b.first[:] = np.random.default_rng(L + 200).normal(50, 5, 35).astype(np.float32)
    return b


NULL_SHAPES = (((5, 7), 10), ((1, 3), 2), ((64, 10), 33))


def null_batch(n_q, k, L, direction, base=None):
    """for dph_rescore_dev(doc = NULL, word = NULL): (doc, word) are idx2id of the id clipped into the shard"""
    b = raw_batch(n_q, k, L, direction, seed=11) if base is None else base
    b.doc, b.word = clip_docword(b.meta, b.ids - ID_BASE)
    if n_q * k < 200:
        b.first[b.first < -1e30] = 47.0              # (padding with the clipped id's (doc, word) is the undecidable candidate of raw_edges)
    return b


def not_held_batch(direction, L=10):
    """candidates next to the shard whose window lies inside it, and one the shard holds; every slot valid (constant f2o)"""
    b = raw_batch(1, 3, L, direction, seed=12)
    out_id = ID_BASE - 1 if direction == 0 else ID_BASE + N_ROWS
    b.ids[:] = [out_id, out_id - 3 if direction == 0 else out_id + 3, ID_BASE + 5]
    b.doc[:], b.word[:] = 4, 20
    b.first[:] = 50, 51, 52
    return b


def run_ref(b, vec_of, held, A=None):
    m = b.meta
    return window_ref(vec_of, held, m.doc_ids, m.f2o_off, m.f2o, b.q, b.ids, b.doc, b.word, b.first, b.k, b.L, b.direction, A=A)


def raw_sets():
    """(name, batch, vec_of, held) of every raw-dump input set the GPU tests use"""
    flat = flat_lookup()
    for direction in (0, 1):
        for (n_q, k), L in RAW_SHAPES:
            yield (f"flat {n_q}x{k} L{L} d{direction}", raw_batch(n_q, k, L, direction), *flat)
        for L in L_ALL:
            yield (f"gap L{L} d{direction}", gap_batch(L, direction), *flat)
            yield (f"invalid L{L} d{direction}", invalid_batch(L, direction), *flat)
        for (n_q, k), L in NULL_SHAPES:
            yield (f"flat NULL doc/word {n_q}x{k} L{L} d{direction}", null_batch(n_q, k, L, direction), *flat)
        yield (f"not held d{direction}", not_held_batch(direction), *flat)
        for L in (2, 10, 33):
            yield (f"lists NULL doc/word L{L} d{direction}", null_batch(5, 7, L, direction, list_batch(L, direction)), *flat)
            yield (f"groups L{L} d{direction}", group_batch(L, direction), *group_lookup())
            yield (f"lists L{L} d{direction}", list_batch(L, direction), *flat)
            for lo, hi in ((0, CUT), (CUT, N_ROWS)):
                yield (f"cut [{lo},{hi}) L{L} d{direction}", cut_batch(L, direction), *flat_lookup(lo, hi))


# ------------------------------------------------------------------------------------------------- PQ shards
PQ_N, PQ_NLIST = 1500, 8
PQ_VARIANTS = ("m96", "m96_bare", "m48_sparse", "m128_plain", "m64_offset")
PQ_L = (1, 10, 64, 65, 70)
PQ_SHAPES = ((1, 3), (5, 7))
PQ_OFFSET = 5 * 10 ** 9


@functools.lru_cache(maxsize=None)
def pq_variant(name):
    """the index, its stored ids (ascending), every reconstruction (rotated space) by id, and the documents"""
    M = {"m96": 96, "m96_bare": 96, "m48_sparse": 48, "m128_plain": 128, "m64_offset": 64}[name]
    rng = np.random.default_rng(1000 + M)
    centres = rng.normal(0, 0.5, (4, DIM)).astype(np.float32)
    xb = (centres[rng.integers(0, 4, PQ_N)] + rng.normal(0, 0.3, (PQ_N, DIM))).astype(np.float32)
    ix = P.train(xb, nlist=PQ_NLIST, M=M, seed=M)
    ids = np.arange(PQ_N, dtype=np.int64)
    if name == "m48_sparse":
        ids = ids * 3 + 7
    if name == "m64_offset":
        ids = ids + PQ_OFFSET
    if name == "m128_plain":
        # codes of the vectors themselves, a bias (the search uses it, the window must not) and a transform that is no
        # rotation: A, its transpose and its inverse all differ
        ix.index.by_residual = False
        ix.chain[0].b = rng.normal(0, 0.05, DIM).astype(np.float32)
        ix.chain[0].A = (ix.chain[0].A * np.linspace(0.5, 2.0, DIM, dtype=np.float32)[None, :]).astype(np.float32)
    P.add_with_ids(ix, xb, ids)
    if name == "m48_sparse":
        for l in (0, 4, PQ_NLIST - 1):                  # first, one in the middle, last: runs of equal list offsets
            ix.index.list_codes[l] = np.zeros((0, M), np.uint8)
            ix.index.list_ids[l] = np.zeros(0, np.int64)
    dm = P.DirectMap(ix.index)
    recon = {int(i): P.reconstruct(ix, dm, int(i)) for i in dm.map}
    n = ix.ntotal
    drng = np.random.default_rng(5)
    lens = [1, 200, 37, n - 1 - 200 - 37 - 300, 300]
    doc_ids = [2, 5, 9, 40, 1000]
    steps = [[0, 1], [0, 1, 1, 2], [0, 0, 1], [0, 1, 1, 2, 3, 40], [0, 1]]
    f2o = [np.concatenate([[3], 3 + np.cumsum(drng.choice(st, ln - 1))]) for st, ln in zip(steps, lens)]
    meta = SimpleNamespace(doc_ids=np.asarray(doc_ids, np.int32), f2o_off=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64),
                           f2o=np.concatenate(f2o).astype(np.int32), row2doc=np.repeat(np.asarray(doc_ids, np.int32), lens),
                           row2word=np.concatenate([np.arange(ln, dtype=np.int32) for ln in lens]), lens=lens)
    # m96_bare: the IndexIVFPQ of m96 without its pre-transform -- the vectors come back as reconstructed, bit for bit
    bare = name == "m96_bare"
    return SimpleNamespace(name=name, ix=ix.index if bare else ix, ivf=ix.index, ids=np.sort(np.asarray(list(dm.map), np.int64)),
                           recon=recon, meta=meta, A=None if bare else np.ascontiguousarray(ix.chain[0].A, np.float32))


def pq_lookup(v):
    return (lambda i: v.recon.get(int(i))), (lambda i: int(i) in v.recon)


def pq_batch(v, n_q, k, L, direction):
    """stored ids (the first and the last code of every list among them: the codes next to an empty list), ids the
    index does not hold before, between and behind them, FAISS padding; (doc, word) drawn independently of the id"""
    rng = np.random.default_rng([v.ivf.M, n_q, k, L, direction])
    n = n_q * k
    meta = v.meta
    ids = v.ids[rng.integers(0, len(v.ids), n)].copy()
    special = [int(l[j]) for l in v.ivf.list_ids if len(l) for j in (0, -1)]
    special += [int(v.ids[0]) - 1, int(v.ids[-1]) + 1, int(v.ids[0]) + 1, int(v.ids[0]), int(v.ids[-1]), int(v.ids[len(v.ids) // 2]) + 1]
    where = rng.permutation(n)[:min(len(special), 2 * n // 3)]
    for c, e in zip(where, rng.permutation(len(special))):
        ids[c] = special[e]
    d = rng.integers(0, len(meta.doc_ids), n)
    d[rng.random(n) < 0.7] = [1, 4][int(rng.integers(0, 2))]       # mostly the documents with small steps: late slots stay valid
    doc = meta.doc_ids[d].astype(np.int32)
    lens = np.asarray(meta.lens)[d]
    word = (rng.integers(0, 1 << 30, n) % lens).astype(np.int32)
    near_end = rng.random(n) < 0.25
    word[near_end] = np.where(rng.random(int(near_end.sum())) < 0.5, rng.integers(0, 4, int(near_end.sum())),
                              lens[near_end] - 1 - rng.integers(0, 4, int(near_end.sum()))).clip(0).astype(np.int32)
    first = rng.normal(50, 5, n).astype(np.float32)
    if n > 3:
        # FAISS padding; towards larger ids an unknown id far below the stored ones instead: behind -FLT_MAX every slot scores the
        # same, and the restatement decides such a candidate only when all its slots hold the same (zero) vector
        ids[n - 1], doc[n - 1], word[n - 1], first[n - 1] = (-1 if direction == 1 else -100), -1, -1, -FLT_MAX
        doc[n - 2], word[n - 2] = 7, 0                              # a document the CSR does not hold
    q = rng.normal(0, 0.5, (n_q, DIM)).astype(np.float32)
    return SimpleNamespace(n_q=n_q, k=k, L=L, direction=direction, q=q, ids=ids, doc=doc, word=word, first=first, meta=meta)


def pq_null_batch(v, L, direction):
    """for the NULL doc / word path: idx2id is indexed by the local id, which is the id on a PQ shard without id groups"""
    b = pq_batch(v, 5, 7, L, direction)
    b.ids[:3] = -1 if direction == 1 else -100, len(v.ids), len(v.ids) + 5          # clipped to the first / last local id
    b.first[:3] = 40, 41, 42
    b.first[-1] = 45
    b.doc, b.word = clip_docword(v.meta, b.ids, n=len(v.ids))
    return b


def pq_sets(name):
    v = pq_variant(name)
    look = pq_lookup(v)
    for direction in (0, 1):
        for L in PQ_L:
            for n_q, k in PQ_SHAPES:
                yield (f"pq {name} {n_q}x{k} L{L} d{direction}", pq_batch(v, n_q, k, L, direction), *look)
        if name == "m96":
            for L in (10, 65):
                yield (f"pq m96 NULL doc/word L{L} d{direction}", pq_null_batch(v, L, direction), *look)
