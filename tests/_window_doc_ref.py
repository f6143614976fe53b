"""Float64 restatement of the window re-score over the dump's RAW int8 rows: the HDF5 branch of the reference's
search_phrase (index.py:246-273, 323-389) behind an OPQ matrix R = A, as dph_rescore serves it on a PQ handle with document
rows attached (include/dph.h, dph_index_attach_doc_rows).  numpy only; in the style of tests/_window_ref.py, whose acceptance
rule (`check`) and tie handling (`WindowRef`) it shares.

A candidate c has an id, a (doc, word), a first-stage score and the query half q[c // k].  Slot s of its window is i = s
(direction 0) or i = L - 1 - s (direction 1, right-aligned) words away IN ITS DOCUMENT: word +- i, whatever the ids are.

    row[c, s]   = doc_rows[f2o_off[j] + word +- i], j the CSR slot of doc[c]; the ZERO vector when the document is unknown,
                  when word[c] itself or word +- i lies outside [0, len) (index.py:265, 270, 333-336, 358-361)
    dequant     = fp32(n / scale + offset), the float64 value rounded once (index.py:158-162 on an int8 array)
    dot[c, s]   = <qrot, dequant(row)> in float64, qrot = fp32(A q) accumulated in float64 (q itself when A is None)
    valid       = as in tests/_window_ref.py (index.py:305-321)
    score[c, s] = float64(fp32(first + fp32(dot))) + (valid ? 0 : -1e9); argslot = the FIRST maximum
    vecs[c, 0]  = fp32(raw A): the candidate's own row as raw int8 values, NOT de-quantised (index.py:383, 388)
    vecs[c, 1]  = fp32(fp32(dequant(arg-max row) A) A)   (index.py:345, 370, then 381-389); both zero unless held(id)

Tolerances, all computed from the inputs (U = 2^-24, the fp32 unit round-off):
    best      tol = 2 U sum_j |qrot_j v_j|            qrot_j is an fp32 rounding of a float64 sum: two summation orders land at most
                  + 2 U (|dot| + |first + dot|)       one ulp = 2 U |qrot_j| apart; one rounding of the dot, one of the sum, each
                                                      again at most one ulp apart
    vecs      per product out = fp32(v A): 2 U |out| + 2 U U sum_t |v_t A_tj| (one rounding of a float64 sum of 768 terms whose
              own error is far below the second term); the twice-rotated vector carries the tolerance of its first product
              through the second: tol_1 |A| + the second product's own.  (`vec_tol`: kernel against restatement.)
    vec_tol_ref   the same vectors against the REFERENCE's arithmetic, which accumulates in fp32 (torch matmul, numpy dot): the
              standard bound of an n-term fp32 inner product, gamma_n sum_t |v_t A_tj| with gamma_n = n U / (1 - n U), n = 768,
              per product, plus the rounding of the result, propagated through the second product like above."""
import numpy as np

from tests._window_ref import DIM, MASK, U, WindowRef


class WindowDocRef(WindowRef):
    def slot_vector(self, c, s):
        if not self.is_held[c]:
            return np.zeros(DIM, np.float32), np.zeros(DIM)
        v, tol, _ = self._twice(self._slot_rows[c][s])
        return v, tol

    def slot_vector_ref_tol(self, c, s):
        if not self.is_held[c]:
            return np.zeros(DIM)
        return self._twice(self._slot_rows[c][s])[2]


def codec_lut(offset, scale):
    """fp32(n / scale + offset) for n = -128 .. 127 with the codec as the fp32 numbers the C ABI takes"""
    o, s = float(np.float32(offset)), float(np.float32(scale))
    return (np.arange(-128, 128, dtype=np.float64) / s + o).astype(np.float32)


def window_doc_ref(doc_rows, doc_ids, f2o_off, f2o, q, ids, doc, word, first, k, L, direction, held, A=None, offset=-2.0, scale=20.0):
    doc_rows = np.asarray(doc_rows, np.int8)
    q = np.asarray(q, np.float32)
    ids = np.asarray(ids, np.int64).reshape(-1)
    doc = np.asarray(doc, np.int64).reshape(-1)
    word = np.asarray(word, np.int64).reshape(-1)
    first = np.asarray(first, np.float32).reshape(-1)
    n = ids.size
    assert q.shape == (n // k, DIM) and n == q.shape[0] * k and direction in (0, 1)
    A64 = None if A is None else np.asarray(A, np.float32).astype(np.float64)
    absA = None if A64 is None else np.abs(A64)
    qd = (q if A64 is None else (q.astype(np.float64) @ A64.T).astype(np.float32)).astype(np.float64)
    csr = {int(d): j for j, d in enumerate(np.asarray(doc_ids).tolist())}
    f2o_off = np.asarray(f2o_off, np.int64)
    f2o = np.asarray(f2o, np.int64)
    assert doc_rows.shape == (int(f2o_off[-1]), DIM)
    lut = codec_lut(offset, scale)
    gamma = DIM * U / (1 - DIM * U)

    def product(v, tol_in, ref_in):
        """fp32(v A) with its tolerance against another float64 implementation / against fp32 accumulation"""
        if A64 is None:
            return v, tol_in, ref_in
        v64 = v.astype(np.float64)
        out = (v64 @ A64).astype(np.float32)
        l1 = np.abs(v64) @ absA
        tol = tol_in @ absA + 2 * U * np.abs(out.astype(np.float64)) + 2 * U * U * l1
        ref = ref_in @ absA + 2 * U * np.abs(out.astype(np.float64)) + gamma * l1
        return out, tol, ref

    zero, ztol = np.zeros(DIM, np.float32), np.zeros(DIM)
    memo = {}

    def twice(row):
        """dequant(row) A A for a row of the store (-1: the zero vector)"""
        if row < 0:
            return zero, ztol, ztol
        if row not in memo:
            v = lut[doc_rows[row].astype(np.int64) + 128]
            memo[row] = product(*product(v, ztol, ztol))
        return memo[row]

    r = WindowDocRef()
    r._twice = twice
    r.slot_ids = np.zeros((n, L), np.int64)            # (the ids play no part in the addressing: kept for the messages of `check`)
    r.slot_words = np.zeros((n, L), np.int64)
    r.valid = np.zeros((n, L), bool)
    r.dots = np.zeros((n, L))
    r.scores = np.zeros((n, L))
    r.tol = np.zeros((n, L))
    r.vec_key = np.zeros((n, L), np.int64)
    r._slot_rows = np.full((n, L), -1, np.int64)
    keys = {zero.tobytes(): 0}
    step = 1 if direction == 0 else -1
    away = np.arange(L) if direction == 0 else np.arange(L - 1, -1, -1)
    own_row = np.full(n, -1, np.int64)
    with np.errstate(over="ignore"):
        for c in range(n):
            r.slot_ids[c] = int(ids[c]) + step * away
            r.slot_words[c] = int(word[c]) + step * away
            j = csr.get(int(doc[c])) if doc[c] >= 0 else None
            base = int(f2o_off[j]) if j is not None else 0
            flen = int(f2o_off[j + 1]) - base if j is not None else 0
            tok = f2o[base:base + flen]
            w = int(word[c])
            own_in = 0 <= w < flen
            if own_in:
                own_row[c] = base + w
            V = np.zeros((L, DIM))
            for s in range(L):
                ww = int(r.slot_words[c, s])
                ok = own_in and 0 <= ww < flen
                if ok:
                    r._slot_rows[c, s] = base + ww
                    V[s] = lut[doc_rows[base + ww].astype(np.int64) + 128]
                    r.vec_key[c, s] = keys.setdefault(doc_rows[base + ww].tobytes(), len(keys))
                    gap = int(tok[ww]) - int(tok[w]) if direction == 0 else int(tok[w]) - int(tok[ww])
                    ok = 0 <= gap <= L
                r.valid[c, s] = ok
            prod = V * qd[c // k][None, :]
            r.dots[c] = prod.sum(1)
            l1 = np.abs(prod).sum(1)
            dot32 = r.dots[c].astype(np.float32)
            sum32 = (first[c] + dot32).astype(np.float32)
            r.scores[c] = sum32.astype(np.float64) + np.where(r.valid[c], 0.0, MASK)
            r.tol[c] = 2 * U * (np.abs(r.dots[c]) + np.abs(np.float64(first[c]) + r.dots[c]))
            if A64 is not None:
                r.tol[c] += 2 * U * l1
    r.argslot = np.argmax(r.scores, 1)                     # the first maximum
    at = np.arange(n)
    r.pred_word = np.where(r.valid[at, r.argslot], r.slot_words[at, r.argslot], -1)
    r.best = r.scores[at, r.argslot]
    r.is_held = np.asarray([bool(held(int(i))) for i in ids])
    r.vecs = np.zeros((n, 2, DIM), np.float32)
    r.vec_tol = np.zeros((n, 2, DIM))
    r.vec_tol_ref = np.zeros((n, 2, DIM))
    for c in range(n):
        if r.is_held[c]:
            if own_row[c] >= 0:
                raw = doc_rows[own_row[c]].astype(np.float32)                       # the raw int8 values, exact in fp32
                r.vecs[c, 0], r.vec_tol[c, 0], r.vec_tol_ref[c, 0] = product(raw, ztol, ztol)
            r.vecs[c, 1], r.vec_tol[c, 1], r.vec_tol_ref[c, 1] = twice(int(r._slot_rows[c, r.argslot[c]]))
    return r
