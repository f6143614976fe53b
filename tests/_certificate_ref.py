"""The certificate of dph_select_kernel restated in numpy / float64 (no code shared with oracle/).

A pass of dph_search_bounded_dev over a flat shard, for one batch of query rows under the caller's per-row bounds tau:
  digits      q_j = sc (128 Q1_j + q2_j) + e_j (tests/_digits.py), sum(q), ||q||_1, ||e||_2, <e, mu>, lmax;
  emitted     non-outlier rows with  (q1 + X).n + bq * code(n) > floor((tau - lmax) / 128)  plus EVERY outlier row;
  keys        exact integer scores I = 128 (q1 + X).n + q2.n, ordered (I desc, row asc); more than POOL_MAX of them: the POOL_MAX
              best stay, a_cut = the POOL_MAX-th best score;
  re-score    the C = min(max(2k, k + 32), 2048) best keys, S64 = sum_j q_j x32(n_j) with x32 the two-rounding fp32 table;
  answer      (S desc, id asc), FAISS padding;
  bound       rows that were not re-scored have I <= a_rest = max(tau, best key left in the pool, a_cut), hence
              S <= (sc a_rest + ||e|| rmax + <e, mu>) / scale + offset sum(q) + ||q||_1 dmax  =: the sum of `terms`
              (+ 1e-9 (|b| + 1)); outlier rows among them take rmax_all instead of rmax;
  status      0 iff k rows came back and the k-th beats the bound, else 2.  A row of status 0 also has re-scored rows it did not
              return: what the shard hands out as its bound covers the best of them as well (include/dph.h).
`mutate` switches single pieces off -- what tests/test_certificate_ref.py uses to show that the input sets have teeth."""
import numpy as np

from tests._digits import host_aux_rows, host_digits

POOL_MAX = 8192          # keys the select kernel sorts
BUCKET_CAP = 32768       # keys a bucket holds: more are "lost pairs" (out of scope here)
C_MAX = 2048
NORM_BIN_W = 4096        # histogram of squared centred norms (finalize)
NORM_BINS = 8192
OUTLIER_MAX = 1024
INT_MIN = -2 ** 31
TERMS = ("int", "e_r", "e_mu", "off", "lut")


def lut32(offset, scale):
    """x32[n + 128]: fl(fl(n) / scale) + offset in fp32, as float64"""
    n = np.arange(-128, 128).astype(np.float32)
    return ((n / np.float32(scale)).astype(np.float32) + np.float32(offset)).astype(np.float32).astype(np.float64)


def delta_max(offset, scale):
    exact = np.arange(-128, 128, dtype=np.float64) / float(np.float32(scale)) + float(np.float32(offset))
    return float(np.abs(lut32(offset, scale) - exact).max())


def shard_constants(xb):
    """What dph_index_finalize measures on a shard WITHOUT aux rows: mu = round-half-even(mean code), the squared centred norms, rmax_all,
    the outlier rows (squared norm >= the lowest histogram bin edge with at most OUTLIER_MAX rows above it, taken only when the
    largest squared norm exceeds 1.21 x that edge) and rmax = sqrt(edge), or rmax_all when no row is set aside."""
    xi = xb.astype(np.int64)
    mu = np.clip(np.rint(xi.sum(0) / float(xi.shape[0])), -128, 127).astype(np.int64)
    n2 = ((xi - mu[None, :]) ** 2).sum(1)
    m = int(n2.max())
    hist = np.bincount(np.minimum(n2 // NORM_BIN_W, NORM_BINS - 1), minlength=NORM_BINS)
    above, cut_bin = 0, NORM_BINS
    for b in range(NORM_BINS - 1, -1, -1):
        if above + hist[b] > OUTLIER_MAX:
            break
        above += int(hist[b])
        cut_bin = b
    cut2 = cut_bin * NORM_BIN_W
    outliers = np.empty(0, np.int64)
    rmax = float(np.sqrt(m))
    if above > 0 and cut_bin > 0 and cut2 * 1.21 < m:
        outliers = np.nonzero(n2 >= cut2)[0]
        rmax = float(np.sqrt(cut2))
    return {"mu": mu, "n2": n2, "rmax": rmax, "rmax_all": float(np.sqrt(m)), "outliers": outliers}


def aux_constants(xb, layout):
    """... and on a shard WITH aux rows (layout = int32[28] as dph_index_get_aux_layout returns it): no row is set aside, rmax = rmax_all,
    norm unit = ceil(rmax_all / (127 n_norm))."""
    c = shard_constants(xb)
    c["rmax"] = c["rmax_all"]
    c["outliers"] = np.empty(0, np.int64)
    c["unit"] = max(1, int(np.ceil(c["rmax_all"] / (127.0 * int(layout[1])))))
    return c


def query_scalars(x, mu, layout, unit, rmax):
    """digits and the per-row scalars of dph_quantize_kernel"""
    x64 = x.astype(np.float32).astype(np.float64)
    aux = layout is not None and int(layout[0]) > 0
    q1, q2, X, sc = host_digits(x, layout if aux else None)
    m = 128 * (q1 + X) + q2
    e = x64 - sc[:, None] * m.astype(np.float64)
    q2n = np.sqrt((q2 * q2).sum(1).astype(np.float64))
    q2mu = q2 @ mu
    if aux:
        lmax = q2mu.astype(np.int64)
        bq = np.minimum(np.ceil(unit * q2n / 128.0 * (1 + 1e-9)).astype(np.int64), 127)
    else:
        lmax = (np.ceil(q2n * rmax * (1 + 1e-9) + q2mu) + 1.0).astype(np.int64)
        bq = np.zeros(x.shape[0], np.int64)
    return {"x64": x64, "hi": q1 + X, "q2": q2, "m": m, "sc": sc, "e": e, "e_norm": np.sqrt((e * e).sum(1)), "e_mu": e @ mu.astype(np.float64),
            "q_sum": x64.sum(1), "q_l1": np.abs(x64).sum(1), "lmax": lmax, "bq": bq}


def bound_of(terms, drop=()):
    """the bound from its terms, the kernel's 1e-9 slack included; `drop` leaves terms out"""
    b = sum(v for name, v in terms.items() if name not in drop)
    return b + 1e-9 * (abs(b) + 1.0)


def certify(xb, x, codec, tau, k, layout, unit, mu, rmax, rmax_all, outliers, id_base=0, mutate=None, cache=None):
    """-> list (one dict per query row): I, D64 (the answer, padded with -1 / -inf), status, bound (what the shard hands out),
    bound_cert (what decides the status), terms (of the branch that sets bound_cert), a_rest, a_cut, n_emitted, n_cand,
    rescored (rows), S64 (every row of the shard), emitted (bool per row), key (exact integer score of every row)."""
    mu = np.asarray(mu, np.int64)
    mut = dict(mutate or {})
    drop = tuple(mut.get("drop", ()))
    offset, scale = float(np.float32(codec[0])), float(np.float32(codec[1]))
    lut = lut32(*codec)
    dmax = delta_max(*codec)
    n_rows = xb.shape[0]
    aux = layout is not None and int(layout[0]) > 0
    if cache is None or "qs" not in cache:                  # (what no mutation touches: computed once per input set)
        qs = query_scalars(x, mu, layout, unit, rmax)
        code = host_aux_rows(xb, mu, layout, unit)[:, :int(layout[1])].sum(1) if aux else np.zeros(n_rows, np.int64)
        xf = xb.astype(np.float64)                          # (integer products below 2^53: exact in float64, and BLAS does them)
        store = {"qs": qs, "S_all": qs["x64"] @ lut[xb.astype(np.int64) + 128].T,
                 "key_all": np.rint(qs["m"].astype(np.float64) @ xf.T).astype(np.int64),
                 "Hp_all": np.rint(qs["hi"].astype(np.float64) @ xf.T).astype(np.int64) + qs["bq"][:, None] * code[None, :]}
        if cache is not None:
            cache.update(store)
    else:
        store = cache
    qs, S_all, key_all, Hp_all = store["qs"], store["S_all"], store["key_all"], store["Hp_all"]
    is_out = np.zeros(n_rows, bool)
    is_out[np.asarray(outliers, np.int64)] = True
    n_out = int(is_out.sum())
    C = min(max(2 * k, k + 32), C_MAX)
    rm_bound = rmax * float(mut.get("rmax_scale", 1.0))
    rm_out = rm_bound if mut.get("outlier_rmax") else rmax_all
    out = []
    for r in range(x.shape[0]):
        key, Hp = key_all[r], Hp_all[r]
        t = int(tau[r])
        if t == INT_MIN:
            emitted = np.ones(n_rows, bool)
        else:
            emitted = (Hp > (t - (int(qs["lmax"][r]) + int(mut.get("lmax_shift", 0)))) // 128) & ~is_out
            emitted |= is_out
        rows = np.nonzero(emitted)[0]
        assert rows.size <= BUCKET_CAP, "lost pairs are out of scope"
        order = rows[np.lexsort((rows, -key[rows]))]
        a_cut = None
        if order.size > POOL_MAX:
            a_cut = int(key[order[POOL_MAX - 1]])
            order = order[:POOL_MAX]
        nc = min(order.size, C)
        cand = order[:nc]
        rest = order[nc:]
        top = cand[np.lexsort((cand, -S_all[r, cand]))]
        I = np.full(k, -1, np.int64)
        D = np.full(k, -np.inf)
        I[:min(k, nc)] = top[:k] + id_base
        D[:min(k, nc)] = S_all[r, top[:k]]

        def terms_of(a, rm):
            return {"int": qs["sc"][r] * a / scale, "e_r": qs["e_norm"][r] * rm / scale, "e_mu": qs["e_mu"][r] / scale,
                    "off": offset * qs["q_sum"][r], "lut": qs["q_l1"][r] * dmax}

        a_rest = t if t != INT_MIN else None
        if rest.size:
            a_rest = int(key[rest[0]]) if a_rest is None else max(a_rest, int(key[rest[0]]))
        if a_cut is not None and not mut.get("ignore_a_cut"):
            a_rest = a_cut if a_rest is None else max(a_rest, a_cut)
        terms = None
        bound = -1.0e300
        status = 0
        if a_rest is not None:
            branches = [terms_of(a_rest, rm_bound)]
            o_rest = rest[is_out[rest]]
            if o_rest.size:                                  # outlier rows left in the pool: their best key, the shard's true maximum norm
                branches.append(terms_of(int(key[o_rest].max()), rm_out))
            if a_cut is not None and n_out > 0 and not mut.get("ignore_a_cut"):
                branches.append(terms_of(a_cut, rm_out))    # ... and outlier rows the radix cut left out of the pool
            terms = max(branches, key=lambda t: bound_of(t, drop))
            bound = bound_of(terms, drop)
            status = 2 if (nc < k or not D[k - 1] > bound) else 0
        handed = bound
        if status == 0 and nc > k:
            handed = max(bound, float(S_all[r, top[k]]))
        out.append({"I": I, "D64": D, "status": status, "bound": handed, "bound_cert": bound, "terms": terms, "a_rest": a_rest,
                    "a_cut": a_cut, "n_emitted": int(rows.size), "n_cand": nc, "rescored": cand, "S64": S_all[r], "emitted": emitted,
                    "key": key, "q": {n: v[r] for n, v in qs.items()}})
    return out


def sum_error(terms):
    """float64 summation error of the bound's terms: each is a reduction over at most 768 products, 768 * 2^-53 * sum |term|"""
    return 768.0 * 2.0 ** -53 * sum(abs(v) for v in terms.values())


def bound_tol(terms, bound):
    """|kernel bound - restated bound| <= 4 x (the terms' summation error: the kernel reduces per thread, per wave and over four
    waves, numpy pairwise -- different orders, each within the bound above) + the kernel's own slack 1e-9 (|b| + 1)"""
    return 4.0 * sum_error(terms) + 1e-9 * (abs(bound) + 1.0)
