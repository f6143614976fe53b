"""The input sets of the direct tests of the doc-addressed window re-score (tests/test_window_doc_direct.py on the GPU,
tests/test_window_doc_ref.py without one): a dump of whole documents, a FILTERED OPQ + IVFPQ index over it, candidate
batches.  numpy only; every set is a pure function of its arguments (fixed seeds).

The dump (per window length L under test): documents of 1, 2, L - 1, L, L + 1 rows for every L in `L_ALL` (one of them empty:
L - 1 = 0) and documents of ~70 rows, 303 rows in all; the f2o steps of the 70-row document walk through gaps of L, L - 1 and
L + 1.  The index keeps every word that is NOT a multiple of 3 (an `_ftN`-style filter), so ids and dump rows diverge: id i is
word row2word[i] of document row2doc[i], and a window of L words reads dump rows the index has no code for."""
import functools
from types import SimpleNamespace

import numpy as np

from densephrases_amd import faiss_io as F
from tests._window_doc_ref import window_doc_ref
from tests._window_ref import DIM

FLT_MAX = np.float32(3.4028234663852886e38)
L_ALL = (1, 10, 20, 70)
DOC_LEN = [1, 2, 0, 9, 10, 11, 19, 20, 21, 69, 70, 71]
DOC_IDS = [2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 1000, 2_000_000]
STEP_DOC = 10                                     # the 70-row document: its f2o steps depend on L
N_DOC_ROWS = int(sum(DOC_LEN))                    # 303
NLIST, M = 4, 96
ID_OFFSET = 5 * 10 ** 9
# (n_q, k): 1, 3, 5 candidates, 20 = whole workgroups, 21 and 35 = a partly empty last workgroup over several of them
SHAPES = ((1, 1), (1, 3), (5, 1), (4, 5), (3, 7), (5, 7))
VARIANTS = ("house", "plain_codec", "house_offset")


@functools.lru_cache(maxsize=None)
def doc_rows():
    rng = np.random.default_rng(31)
    rows = rng.integers(-128, 128, (N_DOC_ROWS, DIM)).astype(np.int8)
    rows[0] = 127                                 # the one-row document is saturated
    rows[5] = -128
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def meta(L):
    """the f2o CSR of the documents and idx2id of the filtered index (words that are no multiple of 3)"""
    rng = np.random.default_rng(41)
    pattern = [L, 0, 1, L + 1, 0, max(L - 1, 0), 1, 1, 2]
    f2o = []
    for d, n in enumerate(DOC_LEN):
        if d == STEP_DOC:
            f2o.append(np.concatenate([[4], 4 + np.cumsum([pattern[i % len(pattern)] for i in range(n - 1)])]))
        else:
            f2o.append(3 + np.cumsum(rng.choice([0, 1, 1, 2], n)))
    off = np.concatenate([[0], np.cumsum(DOC_LEN)]).astype(np.int64)
    keep = [np.asarray([w for w in range(n) if w % 3], np.int32) for n in DOC_LEN]
    row2doc = np.concatenate([np.full(len(kw), d, np.int32) for d, kw in zip(DOC_IDS, keep)])
    row2word = np.concatenate(keep)
    return SimpleNamespace(doc_ids=np.asarray(DOC_IDS, np.int32), f2o_off=off, f2o=np.concatenate(f2o).astype(np.int32),
                           row2doc=row2doc, row2word=row2word, lens=np.asarray(DOC_LEN))


N_IDS = int(sum(len([w for w in range(n) if w % 3]) for n in DOC_LEN))


def householder_permutation(rng):
    """an orthogonal matrix: rows of I - 2 v v^T / <v, v> permuted"""
    v = rng.normal(0, 1, DIM)
    H = np.eye(DIM) - 2.0 * np.outer(v, v) / float(v @ v)
    return np.ascontiguousarray(H[rng.permutation(DIM)].astype(np.float32))


@functools.lru_cache(maxsize=None)
def variant(name):
    """house: R = Householder x permutation, the default codec | plain_codec: a transform that is no rotation (A, its transpose and
    its inverse all differ) and the codec (-1.7, 23) | house_offset: ids from 5e9 behind one id group.  The codes are random: the
    doc-addressed re-score reads none of them (the control test, which re-scores reconstructions, does)."""
    rng = np.random.default_rng({"house": 1, "plain_codec": 2, "house_offset": 3}[name])
    A = householder_permutation(rng)
    offset, scale = -2.0, 20.0
    if name == "plain_codec":
        A = (A * np.linspace(0.5, 2.0, DIM, dtype=np.float32)[None, :] + rng.normal(0, 0.01, (DIM, DIM))).astype(np.float32)
        offset, scale = -1.7, 23.0
    ids = np.arange(N_IDS, dtype=np.int64) + (ID_OFFSET if name == "house_offset" else 0)
    lists = rng.integers(0, NLIST, N_IDS)
    codes = rng.integers(0, 256, (N_IDS, M), dtype=np.uint8)
    ivf = F.IVFPQIndex(DIM, NLIST, M, 8, rng.normal(0, 0.5, (NLIST, DIM)).astype(np.float32),
                       rng.normal(0, 0.3, (M, 256, DIM // M)).astype(np.float32), [codes[lists == l] for l in range(NLIST)],
                       [ids[lists == l] for l in range(NLIST)], True, 0, 1, 2)
    ix = F.PreTransformIndex([F.LinearTransform(A)], ivf, DIM, True)
    return SimpleNamespace(name=name, ix=ix, A=A, ids=ids, offset=offset, scale=scale, groups=name == "house_offset")


def id_of(m, d, w):
    """local id of (document index d, word w) in the filtered index, or None"""
    hit = np.nonzero((m.row2doc == DOC_IDS[d]) & (m.row2word == w))[0]
    return int(hit[0]) if len(hit) else None


def batch(v, n_q, k, L, direction, null_docword=False):
    """Candidates: the first and the last word of documents (the last document of the store among them), words whose windows run
    past either end, the phases of the L / L - 1 / L + 1 steps, ids the direct map does not hold (they must give zero vectors),
    FAISS padding, a document the CSR does not hold, a word outside its document.  (doc, word) are those of the id unless the
    candidate is one of the edges; `null_docword`: every (doc, word) is what idx2id answers for the id, clipped."""
    rng = np.random.default_rng([len(v.name), n_q, k, L, direction, int(null_docword)])
    m = meta(L)
    n = n_q * k
    base = int(v.ids[0])
    local = rng.integers(0, N_IDS, n)
    E = []                                           # (local id or None, doc index, word)
    for d in (len(DOC_LEN) - 1, STEP_DOC, 9, 4, 0, 1):
        for w in (0, DOC_LEN[d] - 1, 1, DOC_LEN[d] - 2):
            if 0 <= w < DOC_LEN[d]:
                E.append((id_of(m, d, w), d, w))
    for w in range(2, 20, 2):
        E.append((id_of(m, STEP_DOC, w), STEP_DOC, w))
    order = rng.permutation(len(E))
    ids = base + local
    doc = m.row2doc[local].astype(np.int32)
    word = m.row2word[local].astype(np.int32)
    for c, e in zip(rng.permutation(n)[:max(1, 3 * n // 4)], order):
        l, d, w = E[e]
        # a word the filter dropped has no id of its own: the candidate keeps a held id, its (doc, word) are the edge's
        ids[c] = base + (l if l is not None else int(local[c]))
        doc[c], word[c] = DOC_IDS[d], w
    first = rng.normal(50, 5, n).astype(np.float32)
    if n >= 20 and not null_docword:
        ids[n - 1], doc[n - 1], word[n - 1], first[n - 1] = -1, -1, -1, -FLT_MAX          # FAISS padding
        doc[n - 2], word[n - 2] = 7, 0                                                    # a document the CSR does not hold
        ids[n - 3] = base + N_IDS                                                         # behind the last id: not held, window scored
        ids[n - 4] = base - 1 if base else 2 ** 40
        word[n - 5] = DOC_LEN[STEP_DOC]                                                   # a word outside its document
        doc[n - 5] = DOC_IDS[STEP_DOC]
        doc[n - 6], word[n - 6] = DOC_IDS[2], 0                                           # the empty document
    if null_docword:
        if n >= 20:
            ids[:3] = -1, base + N_IDS, base + N_IDS + 5                                  # clipped to the first / last local id
        l = np.clip(ids - base, 0, N_IDS - 1)
        doc, word = m.row2doc[l].astype(np.int32), m.row2word[l].astype(np.int32)
    q = rng.normal(0, 0.5, (n_q, DIM)).astype(np.float32)
    return SimpleNamespace(n_q=n_q, k=k, L=L, direction=direction, q=q, ids=ids, doc=doc, word=word, first=first, meta=m)


def held(v):
    lo, hi = int(v.ids[0]), int(v.ids[-1])
    return lambda i: lo <= int(i) <= hi


def run_ref(v, b):
    m = b.meta
    return window_doc_ref(doc_rows(), m.doc_ids, m.f2o_off, m.f2o, b.q, b.ids, b.doc, b.word, b.first, b.k, b.L, b.direction,
                          held(v), A=v.A, offset=v.offset, scale=v.scale)


def sets(name):
    v = variant(name)
    for direction in (0, 1):
        for L in L_ALL:
            for n_q, k in SHAPES:
                yield f"doc {name} {n_q}x{k} L{L} d{direction}", v, batch(v, n_q, k, L, direction)
            yield f"doc {name} NULL doc/word L{L} d{direction}", v, batch(v, 5, 7, L, direction, null_docword=True)
