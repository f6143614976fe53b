"""The range-sharded, two-phase search restated in numpy / plain Python -- float64 and exact integers, no code shared with oracle/ (include/dph.h:
"two-phase search of a range-sharded dump", "multi-GPU merge"):

  sample_top     what dph_search_sample_dev shares: the ladder of one pass walked as pass_ladder (csrc/dph_api.hip) walks it, the 16 best
                 non-outlier keys of the last level's bucket;
  union_bounds   dph_union_bounds_dev: the 16-th best of the union, minus one;
  merge          dph_merge_topk_dev / dph_merge_records_dev: (fp32 score desc, id asc) over the candidates with id >= 0;
  merged_status  the verdict of the merge over rows whose shards deferred it (dph.h, dph_merge_records_dev), with a `mutate` switch that
                 breaks single pieces -- tests/test_shard_merge_ref.py shows that the input sets notice each of them;
  protocol       sample -> union -> tests/_certificate_ref.certify per shard -> merge -> merged_status over range shards of one dump.

What the tests had to learn beyond dph.h:
  * The sample call plans its INTERMEDIATE levels with k = 1 (pass_args' default: dph_search_sample_dev sets no k), so
    kp = plan_kp(16, true, plan_select_C(1) = 33, last stride) -- 32 behind a last stride of 2, 20 behind 4, 16 from 7 on.  The LAST level is
    always cut at 16 (dph_launch_threshold: top_out != NULL), whatever the tuning key "sample_kp" says.
  * The derived ladder depends on the width of the pass (qb): a call of 300 rows is a pass of 256 and a pass of 44 that may walk different
    strides.  An explicit ladder (tuning key "ladder") is the same for every pass; strides <= 1 are dropped.
  * A ladder whose strides do not nest -- (7, 2) -- shares only the tiles t % lcm == 0 between two levels.  The bound of the coarser level is
    still the score of real rows, so it stays a valid lower bound, but nothing guarantees that 16 rows of the finer level beat it: `top` may
    then hold fewer than 16 scores (INT_MIN padded).  For nesting ladders every level's kp >= 16 best rows are visited again by the next
    level and `top` is simply the 16 best non-outlier keys of the tiles t % last_stride == 0.
  * Outlier rows sit in every level's bucket in full, but neither the bounds nor `top` count them.
  * The padding rows of a shard's last, partial tile (all-zero codes: key 0) are never candidates -- a query row whose real rows all score
    negative must not see a 0 in its sample.
  * The margin of the verdict, kth = D_k - |D_k| 1.2e-7, covers the rounding of a float64 score to a NORMAL fp32 number (relative error
    <= 2^-24 = 5.96e-8).  Scores in fp32's denormal range are not covered by it; the search never gets there, because the bound of
    dph_search_bounded_dev carries an absolute slack of 1e-9 that no such score beats."""
import numpy as np

from tests import _certificate_ref as R

KEEP = 16                   # DPH_SAMPLE_KEEP
INT_MIN = -2 ** 31
INT_MAX = 2 ** 31 - 1
TILE = 32
FLT_MAX = np.float32(3.4028234663852886e38)
SAMPLE_PLAN_K = 1           # the k dph_search_sample_dev plans its intermediate kp with (pass_args::k's default)
MARGIN = 1.2e-7
NO_KTH = -1.0e300
PAD_BEST, PAD_PRED = -1.0e9, -1
MUTATIONS = ("no_margin", "two_as_zero", "ignore_nvalid", "ge", "ignore_one", "wrong_part")


# ---------------------------------------------------------------------------------------------------------------- phase 1: the sample
def passes(n, max_qb=2):
    """[(q0, rows, qb)] of a call of n query rows on a flat shard: 256 rows while more than 128 are left, else up to 128"""
    out, q0 = [], 0
    while q0 < n:
        left = n - q0
        qb = 2 if (left > 128 and max_qb >= 2) else 1
        nq = min(left, 128 * qb)
        out.append((q0, nq, qb))
        q0 += nq
    return out


def sample_plan(n_rows, grid, qb, explicit=(), fine_stride=0):
    """(strides, kp) of one pass: tests/_plan.py's ladder and kp, with the k the sample call plans with"""
    from tests import _plan as P
    strides = P.ladder((n_rows + TILE - 1) // TILE, n_rows, grid, fine_stride, tuple(explicit), qb)
    kp = P.kp(KEEP, bool(strides), P.select_C(SAMPLE_PLAN_K), float(strides[-1]) if strides else 1.0)
    return strides, kp


def sample_top(key, Hp, lmax, outliers, strides, kp):
    """key, Hp [n_q, n_rows]: exact integer scores 128 (q1 + X).n + q2.n and high-digit filter scores of every (query row, real row); lmax [n_q].
    -> (top [n_q, 16] int64, sorted descending, INT_MIN padded; info = per level: stride, bucket sizes [n_q], tau [n_q])"""
    n_q, n_rows = key.shape
    is_out = np.zeros(n_rows, bool)
    is_out[np.asarray(outliers, np.int64)] = True
    n_out = int(is_out.sum())
    tile = np.arange(n_rows) // TILE
    top = np.full((n_q, KEEP), INT_MIN, np.int64)
    info = []
    tau = None                                              # the first level runs cold
    for li, stride in enumerate(strides):
        last = li + 1 == len(strides)
        visited = (tile % stride == 0) & ~is_out
        new_tau = np.full(n_q, INT_MIN, np.int64)
        sizes = np.zeros(n_q, np.int64)
        for r in range(n_q):
            if tau is None or tau[r] == INT_MIN:
                emitted = visited
            else:
                emitted = visited & (128 * Hp[r] + int(lmax[r]) > int(tau[r]))
            ks = np.sort(key[r, emitted])[::-1]
            sizes[r] = ks.size + n_out                      # every outlier row is in the bucket as well
            cut = KEEP if last else kp
            t = int(ks[cut - 1]) - 1 if ks.size >= cut else INT_MIN
            new_tau[r] = max(t, INT_MIN if tau is None else int(tau[r]))
            if last:
                top[r, :min(KEEP, ks.size)] = ks[:KEEP]
        info.append({"stride": stride, "bucket": sizes, "tau": new_tau})
        tau = new_tau
    return top, info


def sample_top_closed_form(key, outliers, last_stride):
    """nesting ladders: the 16 best non-outlier keys of the rows in tiles t % last_stride == 0 (no kp, no filter)"""
    n_q, n_rows = key.shape
    keep = (np.arange(n_rows) // TILE) % last_stride == 0
    keep[np.asarray(outliers, np.int64)] = False
    top = np.full((n_q, KEEP), INT_MIN, np.int64)
    for r in range(n_q):
        ks = np.sort(key[r, keep])[::-1][:KEEP]
        top[r, :ks.size] = ks
    return top


def nests(strides):
    return all(a % b == 0 for a, b in zip(strides, strides[1:]))


# ---------------------------------------------------------------------------------------------------------------- the union bound
def union_bounds(top_parts):
    """top_parts [P, n, 16] -> tau [n]: the 16-th largest of the entries that are not INT_MIN, minus one; INT_MIN when fewer than 16"""
    top_parts = np.asarray(top_parts, np.int64)
    P, n, w = top_parts.shape
    tau = np.full(n, INT_MIN, np.int64)
    for r in range(n):
        u = top_parts[:, r, :].reshape(-1)
        u = np.sort(u[u != INT_MIN])[::-1]
        if u.size >= KEEP:
            tau[r] = int(u[KEEP - 1]) - 1
    return tau


# ---------------------------------------------------------------------------------------------------------------- the merge
def merge(D_parts, I_parts, k, best_parts=None, pred_parts=None):
    """D_parts [P, n, k] fp32, I_parts [P, n, k] int64 -> dict D, I, src (part * k + col), nvalid, and best / pred when given.
    Ids within a row are unique (anything else is undefined input for the kernel)."""
    D_parts = np.asarray(D_parts, np.float32)
    I_parts = np.asarray(I_parts, np.int64)
    P, n, kk = I_parts.shape
    assert kk == k
    D = np.full((n, k), -FLT_MAX, np.float32)
    I = np.full((n, k), -1, np.int64)
    src = np.full((n, k), -1, np.int32)
    best = None if best_parts is None else np.full((n, k), PAD_BEST, np.float64)
    pred = None if pred_parts is None else np.full((n, k), PAD_PRED, np.int32)
    nvalid = np.zeros(n, np.int64)
    for r in range(n):
        cand = [(-float(D_parts[p, r, c]), int(I_parts[p, r, c]), p, c) for p in range(P) for c in range(k) if I_parts[p, r, c] >= 0]
        cand.sort(key=lambda t: (t[0], t[1]))               # (-0.0 == +0.0: such scores tie and the id decides, as in the kernel)
        nvalid[r] = len(cand)
        for j, (_, i, p, c) in enumerate(cand[:k]):
            D[r, j] = D_parts[p, r, c]                      # the copied float, sign of zero included
            I[r, j] = i
            src[r, j] = p * k + c
            if best is not None:
                best[r, j] = best_parts[p, r, c]
            if pred is not None:
                pred[r, j] = pred_parts[p, r, c]
    return {"D": D, "I": I, "src": src, "best": best, "pred": pred, "nvalid": nvalid}


def kth_of(D_k, nvalid, k):
    """the merged k-th score with its margin, float64 [n]: D_k - |D_k| 1.2e-7 where k rows came back, else -1e300"""
    d = np.asarray(D_k, np.float32).astype(np.float64)
    return np.where(np.asarray(nvalid) >= k, d - np.abs(d) * MARGIN, NO_KTH)


def merged_status(D_k, nvalid, k, status_parts, bound_parts=None, mutate=None):
    """D_k [n] fp32 (column k-1 of the merged D), nvalid [n], status_parts [P, n], bound_parts [P, n] float64 or None -> status [n]:
    3 if any part says 3; else 0 iff every part has status 0, or status 2 with bounds given and kth > bound_p; else 1."""
    assert mutate is None or mutate in MUTATIONS
    status_parts = np.asarray(status_parts)
    P, n = status_parts.shape
    d = np.asarray(D_k, np.float32).astype(np.float64)
    nv = np.asarray(nvalid)
    out = np.zeros(n, np.int32)
    for r in range(n):
        have_k = nv[r] >= k or mutate == "ignore_nvalid"
        kth = (d[r] if mutate == "no_margin" else d[r] - abs(d[r]) * MARGIN) if have_k else NO_KTH
        worst, nonfinite = 0, False
        for p in range(P):
            v = int(status_parts[p, r])
            if v == 0:
                continue
            if v == 3:
                nonfinite = True
                continue
            if v == 2 and mutate == "two_as_zero":
                continue
            if v == 1 and mutate == "ignore_one":
                continue
            if v == 2 and bound_parts is not None:
                b = float(bound_parts[(p + 1) % P if mutate == "wrong_part" else p, r])
                if (kth >= b) if mutate == "ge" else (kth > b):
                    continue
            worst = 1
        out[r] = 3 if nonfinite else worst
    return out


# ---------------------------------------------------------------------------------------------------------------- the whole protocol
class RangeShard:
    """rows [id_base, id_base + n) of a dump, with what dph_index_finalize measures on them (no aux rows)"""

    def __init__(self, xb, id_base):
        self.xb, self.id_base = np.ascontiguousarray(xb, np.int8), int(id_base)
        c = R.shard_constants(self.xb)
        self.mu, self.n2, self.rmax, self.rmax_all, self.outliers = c["mu"], c["n2"], c["rmax"], c["rmax_all"], c["outliers"]

    def keys(self, x):
        qs = R.query_scalars(x, self.mu, None, 1, self.rmax)
        xf = self.xb.astype(np.float64)                     # (integer products below 2^53: exact in float64)
        key = np.rint(qs["m"].astype(np.float64) @ xf.T).astype(np.int64)
        Hp = np.rint(qs["hi"].astype(np.float64) @ xf.T).astype(np.int64)
        return key, Hp, qs["lmax"]

    def sample(self, x, grid, explicit=(), fine_stride=0):
        """`top` of a whole call [n_q, 16] and the per-pass (q0, rows, strides, kp, info)"""
        key, Hp, lmax = self.keys(x)
        top = np.full((x.shape[0], KEEP), INT_MIN, np.int64)
        log = []
        for q0, nq, qb in passes(x.shape[0]):
            strides, kp = sample_plan(self.xb.shape[0], grid, qb, explicit, fine_stride)
            t, info = sample_top(key[q0:q0 + nq], Hp[q0:q0 + nq], lmax[q0:q0 + nq], self.outliers, strides, kp)
            top[q0:q0 + nq] = t
            log.append((q0, nq, strides, kp, info))
        return top, log

    def certify(self, x, tau, k, codec=(-2.0, 20.0)):
        return R.certify(self.xb, x, codec, tau, k, None, 1, self.mu, self.rmax, self.rmax_all, self.outliers, id_base=self.id_base)


def nonfinite_rows(x):
    return ~np.isfinite(np.asarray(x, np.float32)).all(1)


def protocol(shards, x, k, grid, explicit=()):
    """sample -> union -> certify per shard -> merge -> merged_status.  -> dict: top [P, n, 16], tau [n], parts (certify's output per shard),
    D_parts / I_parts / status_parts / bound_parts, merged (merge's output), status [n].  A non-finite query row is 3 on every shard (ids -1)
    and searched as nothing here."""
    x = np.ascontiguousarray(x, np.float32)
    n = x.shape[0]
    nf = nonfinite_rows(x)
    xs = np.where(nf[:, None], np.float32(0), x)            # (stand-in: the row's results are overwritten below)
    P = len(shards)
    top = np.stack([s.sample(xs, grid, explicit)[0] for s in shards])
    tau = union_bounds(top)
    D_parts = np.full((P, n, k), -FLT_MAX, np.float32)
    I_parts = np.full((P, n, k), -1, np.int64)
    status_parts = np.zeros((P, n), np.int32)
    bound_parts = np.zeros((P, n), np.float64)
    parts = []
    for p, s in enumerate(shards):
        res = s.certify(xs, tau, k)
        parts.append(res)
        for r, c in enumerate(res):
            if nf[r]:
                status_parts[p, r] = 3
                continue
            got = c["I"] >= 0
            I_parts[p, r] = c["I"]
            D_parts[p, r, got] = c["D64"][got].astype(np.float32)
            status_parts[p, r] = c["status"]
            bound_parts[p, r] = c["bound"]
    m = merge(D_parts, I_parts, k)
    status = merged_status(m["D"][:, k - 1], m["nvalid"], k, status_parts, bound_parts)
    return {"top": top, "tau": tau, "parts": parts, "D_parts": D_parts, "I_parts": I_parts, "status_parts": status_parts,
            "bound_parts": bound_parts, "merged": m, "status": status, "nonfinite": nf}


def status_exemptions(run, k):
    """rows whose status the GPU may report differently: a comparison against a shard's bound -- the shard's own k-th, or the merged k-th
    with its margin -- falls inside the tolerance of that bound (tests/test_certificate_direct.py, `status`)"""
    n = run["status"].size
    kth = kth_of(run["merged"]["D"][:, k - 1], run["merged"]["nvalid"], k)
    out = np.zeros(n, bool)
    for part in run["parts"]:
        for r, c in enumerate(part):
            if c["terms"] is None or run["nonfinite"][r]:
                continue
            tol = R.bound_tol(c["terms"], c["bound_cert"]) + 2 * R.sum_error(c["terms"])
            if c["n_cand"] >= k and abs(c["D64"][k - 1] - c["bound_cert"]) <= tol:
                out[r] = True
            if kth[r] != NO_KTH and abs(kth[r] - c["bound"]) <= tol + 2 * float(np.spacing(np.float32(abs(kth[r])))):
                out[r] = True
    return out
