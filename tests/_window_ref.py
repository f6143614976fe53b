"""Float64 restatement of the start/end window re-score (dph_rescore, include/dph.h; the reference's index.py:276-370)
with the tolerances its roundings allow, and the acceptance rule the direct tests hold the kernels to.  numpy only: no
GPU, no torch, and no code shared with oracle.mips_oracle.window_rescore (tests/test_window_ref.py pins the two to each
other on the toy dump).

A candidate c has a global id, a (doc, word), a first-stage score and the query half q[c // k].  Slot s of its window is
i = s (direction 0) or i = L - 1 - s (direction 1, right-aligned) steps away: id +- i, word +- i.

    dot[c, s]   = <q, v(id +- i)> in float64, v = vec_of(id +- i) or the zero vector when the shard does not store it
    valid[c, s] = the document is in the CSR, word and word +- i lie in it and 0 <= f2o[later] - f2o[earlier] <= L
    score[c, s] = float64(fp32(first + fp32(dot))) + (valid ? 0 : -1e9)
    argslot     = FIRST maximum of score[c, :], pred_word = its word or -1 when it is invalid, best = its score
    vecs[c, 0]  = the candidate's own vector, vecs[c, 1] = the arg-max slot's, both zero unless held(id)

With a pre-transform A (PQ shards: vec_of returns ROTATED reconstructions) the dot is taken with qrot = fp32(A q) and
vecs[c, 0] = fp32(v' A), vecs[c, 1] = fp32(fp32(v' A) A), every product accumulated in float64.

Tolerances (derived from those roundings, U = 2^-24 the fp32 unit round-off; none of them is measured):
    flat   tol = 2 U (|dot| + |first + dot|)        one fp32 rounding of the dot and one of the sum, each at most
                                                    one ulp = 2 U apart between two float64 summation orders
    PQ     + U sum_j |qrot_j v'_j|                  qrot itself is an fp32 rounding of a float64 sum
    (the float64 add of the mask is the same operation on both sides and rounds far below either term)
    PQ vectors, per element: 2 U |value| + 2 U U sum_t |v_t A_tj| (v = the fp32 input of that product); flat vectors
    are table reads and PQ reconstructions one fp32 add: bit for bit."""
import numpy as np

MASK = -1e9
U = 2.0 ** -24
DIM = 768


class WindowRef:
    """Arrays over the n candidates of one batch: slot_ids / slot_words / valid / dots / scores / tol [n, L], argslot /
    pred_word / best [n], vecs / vec_tol [n, 2, DIM]; vec_key [n, L] numbers the distinct slot vectors (byte-wise)."""

    def slot_vector(self, c, s):
        """(vector fp32 [DIM], tolerance [DIM]) of what vecs[c, 1] must hold if slot s were the arg-max"""
        if not self.is_held[c]:
            return np.zeros(DIM, np.float32), np.zeros(DIM)
        return self._finish(self._vec(int(self.slot_ids[c, s])), 2)

    def tied(self, c):
        """T: the slots whose score is within 2 tol of the maximum"""
        m = int(self.argslot[c])
        band = 2.0 * np.maximum(self.tol[c], self.tol[c, m])
        return np.nonzero(self.scores[c] >= self.scores[c, m] - band)[0]

    def planted(self, c, T):
        """every slot of T holds the same bytes with the same validity: the kernel's scores there are equal too"""
        return len(set(self.vec_key[c, T].tolist())) == 1 and len(set(self.valid[c, T].tolist())) == 1

    def left_out(self):
        """candidates whose arg-max the restatement cannot decide: |T| > 1 and not a planted tie"""
        out = []
        for c in range(len(self.argslot)):
            T = self.tied(c)
            if len(T) > 1 and not self.planted(c, T):
                out.append(c)
        return out


def window_ref(vec_of, held, doc_ids, f2o_off, f2o, q, ids, doc, word, first, k, L, direction, A=None):
    q = np.asarray(q, np.float32)
    ids = np.asarray(ids, np.int64).reshape(-1)
    doc = np.asarray(doc, np.int64).reshape(-1)
    word = np.asarray(word, np.int64).reshape(-1)
    first = np.asarray(first, np.float32).reshape(-1)
    n = ids.size
    assert q.shape == (n // k, DIM) and n == q.shape[0] * k and direction in (0, 1)
    A64 = None if A is None else np.asarray(A, np.float32).astype(np.float64)
    qd = q if A64 is None else (q.astype(np.float64) @ A64.T).astype(np.float32)         # qrot = fp32(A q)
    qd = qd.astype(np.float64)
    csr = {int(d): j for j, d in enumerate(np.asarray(doc_ids).tolist())}
    f2o_off = np.asarray(f2o_off, np.int64)
    f2o = np.asarray(f2o, np.int64)
    zero = np.zeros(DIM, np.float32)
    memo, keys = {}, {zero.tobytes(): 0}

    def vec(i):
        if i not in memo:
            v = vec_of(i)
            v = zero if v is None else np.ascontiguousarray(v, np.float32)
            memo[i] = (v, keys.setdefault(v.tobytes(), len(keys)))
        return memo[i][0]

    def finish(v, reps):
        """v (A = None) or v A applied `reps` times, one fp32 rounding per product; and the element tolerance"""
        tol = np.zeros(DIM)
        if A64 is None:
            return v, tol
        for _ in range(reps):
            v64 = v.astype(np.float64)
            out = (v64 @ A64).astype(np.float32)
            tol = 2 * U * np.abs(out.astype(np.float64)) + 2 * U * U * (np.abs(v64) @ np.abs(A64))
            v = out
        return v, tol

    r = WindowRef()
    r._vec, r._finish = vec, finish
    r.slot_ids = np.zeros((n, L), np.int64)
    r.slot_words = np.zeros((n, L), np.int64)
    r.valid = np.zeros((n, L), bool)
    r.dots = np.zeros((n, L))
    r.scores = np.zeros((n, L))
    r.tol = np.zeros((n, L))
    r.vec_key = np.zeros((n, L), np.int64)
    step = 1 if direction == 0 else -1
    away = np.arange(L) if direction == 0 else np.arange(L - 1, -1, -1)
    with np.errstate(over="ignore"):
        for c in range(n):
            r.slot_ids[c] = int(ids[c]) + step * away
            r.slot_words[c] = int(word[c]) + step * away
            j = csr.get(int(doc[c])) if doc[c] >= 0 else None
            tok = f2o[f2o_off[j]:f2o_off[j + 1]] if j is not None else f2o[:0]
            w = int(word[c])
            V = np.stack([vec(int(i)) for i in r.slot_ids[c]]).astype(np.float64)
            r.vec_key[c] = [memo[int(i)][1] for i in r.slot_ids[c]]
            prod = V * qd[c // k][None, :]
            r.dots[c] = prod.sum(1)
            l1 = np.abs(prod).sum(1)
            for s in range(L):
                ww = int(r.slot_words[c, s])
                ok = 0 <= w < len(tok) and 0 <= ww < len(tok)
                if ok:
                    gap = int(tok[ww]) - int(tok[w]) if direction == 0 else int(tok[w]) - int(tok[ww])
                    ok = 0 <= gap <= L
                r.valid[c, s] = ok
            dot32 = r.dots[c].astype(np.float32)
            sum32 = (first[c] + dot32).astype(np.float32)
            r.scores[c] = sum32.astype(np.float64) + np.where(r.valid[c], 0.0, MASK)
            r.tol[c] = 2 * U * (np.abs(r.dots[c]) + np.abs(np.float64(first[c]) + r.dots[c]))
            if A64 is not None:
                r.tol[c] += U * l1
    r.argslot = np.argmax(r.scores, 1)                     # the first maximum
    at = np.arange(n)
    r.pred_word = np.where(r.valid[at, r.argslot], r.slot_words[at, r.argslot], -1)
    r.best = r.scores[at, r.argslot]
    r.is_held = np.asarray([bool(held(int(i))) for i in ids])
    r.vecs = np.zeros((n, 2, DIM), np.float32)
    r.vec_tol = np.zeros((n, 2, DIM))
    for c in range(n):
        if r.is_held[c]:
            r.vecs[c, 0], r.vec_tol[c, 0] = finish(vec(int(ids[c])), 1)
            r.vecs[c, 1], r.vec_tol[c, 1] = r.slot_vector(c, r.argslot[c])
    return r


def check(r, pred, best, arg, vecs=None, what=""):
    """The acceptance rule: holds the outputs of dph_rescore to the restatement `r`; returns the candidates left out
    (arg-max undecided within the tolerance), which the caller caps."""
    n = len(r.argslot)
    pred, best, arg = np.asarray(pred).reshape(-1), np.asarray(best).reshape(-1), np.asarray(arg).reshape(-1)
    assert pred.shape == best.shape == arg.shape == (n,)
    left = []
    for c in range(n):
        tag = f"{what} candidate {c} id {int(r.slot_ids[c, 0])}..{int(r.slot_ids[c, -1])}"
        a = int(arg[c])
        T = r.tied(c)
        if len(T) == 1:
            assert a == int(T[0]), f"{tag}: argslot {a}, restatement {int(T[0])} (scores {r.scores[c]})"
        elif r.planted(c, T):
            assert a == int(T.min()), f"{tag}: argslot {a}, first of the planted tie {T}"
        else:
            assert a in T.tolist(), f"{tag}: argslot {a} is not among the near-maxima {T}"
            left.append(c)
        want_word = int(r.slot_words[c, a]) if r.valid[c, a] else -1
        assert int(pred[c]) == want_word, f"{tag}: pred_word {int(pred[c])}, slot {a} says {want_word}"
        err = abs(float(best[c]) - float(r.scores[c, a]))
        assert err <= r.tol[c, a], f"{tag}: best {float(best[c])!r} vs {float(r.scores[c, a])!r}: {err} > tol {r.tol[c, a]}"
        if vecs is not None:
            v1, t1 = (r.vecs[c, 1], r.vec_tol[c, 1]) if a == int(r.argslot[c]) else r.slot_vector(c, a)
            for t, (v, tol) in enumerate(((r.vecs[c, 0], r.vec_tol[c, 0]), (v1, t1))):
                got = np.asarray(vecs[c, t], np.float32)
                if not tol.any():
                    assert np.array_equal(got, v), f"{tag}: vecs[{c},{t}] is not bit for bit the stored vector (held {bool(r.is_held[c])})"
                else:
                    bad = np.abs(got.astype(np.float64) - v.astype(np.float64)) > tol
                    assert not bad.any(), f"{tag}: vecs[{c},{t}] off at {np.nonzero(bad)[0][:5]}: {got[bad][:5]} vs {v[bad][:5]}"
    return left
