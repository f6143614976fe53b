"""Input sets that press the certificate's bound against each of its terms (tests/test_certificate_ref.py on the restatement alone,
tests/test_certificate_direct.py on the GPU).  Everything here is numpy on the host: shards of 14 000 - 20 000 rows (above the 8192 rows
the select step sorts whole) made of synth.py rows with planted rows, crafted query rows, per-row bounds tau.

Crafted query rows are x_j = 2^-14 (m_j + eps_j) with ONE pin element m = 16256, eps = 0: max |x| = 127 * 2^-7, so sc = 2^-14 exactly,
the digits are m = 128 Q1 + q2 and the residual is e_j = sc eps_j, chosen freely in (-0.5, 0.5) sc.  The pin dimension carries most of the
integer score: a planted row is moved up and down the ranking by its code there, and rows planted for OTHER query rows (other pins)
look like background to this one."""
import functools

import numpy as np

from tests import _certificate_ref as R

SC = 2.0 ** -14
PIN_M = 16256
E45, E49 = 115.0 / 256.0, 125.0 / 256.0     # residual sizes (dyadic: the crafted rows stay exact in fp32)
CODEC_DEFAULT = (-2.0, 20.0)
CODEC_WIDE = (-300.3, 7.0)          # offset far from the codes' range: x32 rounds at 2^-15, dmax ~ 30 x the default codec's


def craft(m, eps):
    x = (SC * (m.astype(np.float64) + eps)).astype(np.float32)
    assert np.array_equal(x.astype(np.float64), SC * (m.astype(np.float64) + eps)), "not representable in fp32"
    return x


def _m_of(q1, q2):
    assert (np.abs(q2) <= 63).all() and (np.abs(q1) <= 127).all()
    return 128 * q1 + q2


def _rand_m(rng, pin, amp):
    """digits of a crafted row: the pin, |m| <= amp elsewhere"""
    m = rng.integers(-amp, amp + 1, 768)
    q1 = np.rint(m / 128.0).astype(np.int64)
    q2 = np.clip(m - 128 * q1, -63, 63)
    m = _m_of(q1, q2)
    m[pin] = PIN_M
    a, b, c = _adjust_dims(pin)
    m[a] = m[b] = 128                                     # (two steps of 128 and one of 1: _tie_rows reaches every integer score with them)
    m[c] = 1
    return m


def _adjust_dims(pin):
    return pin + 100, pin + 101, pin + 102


def _tie_rows(m, rows, target, pin):
    """copies of `rows` whose integer score m.n is EXACTLY `target`: the pin code takes the bulk (steps of 16256), two dimensions with
    digit 128 the next 8128 either way, one with digit 1 the rest.  Rows that tie with a planted row n* and have smaller row ids rank
    before it and are re-scored in its place -- and every one of them obeys the bound n* presses against, so the row stays uncertified
    (status 2) and the bound that is handed out is the certificate's own."""
    a, b, c = _adjust_dims(pin)
    assert m[a] == 128 and m[b] == 128 and m[c] == 1 and m[pin] == PIN_M
    out = np.atleast_2d(np.asarray(rows, np.int64)).copy()
    for r in out:
        r[[a, b, c]] = 40
        r[pin] = 0
        r[pin] = int(np.rint((target - int(m @ r)) / PIN_M))
        q = int(np.rint((target - int(m @ r)) / 128.0))
        qa = int(np.clip(q, -40, 40))
        r[a] += qa
        r[b] += q - qa
        r[c] += target - int(m @ r)
        assert int(m @ r) == target and -128 <= r.min() and r.max() <= 127
    return out


def _fill_to_cap(sign, dims, fixed2, cap2):
    """d = sign * g on `dims` with integer magnitudes g as equal as possible and fixed2 + |d|^2 <= cap2, as large as that allows"""
    D = len(dims)
    g = int(np.sqrt(max(cap2 - fixed2, 0) / D))
    mag = np.full(D, g, np.int64)
    room = cap2 - fixed2 - D * g * g
    bump = min(D, int(room // (2 * g + 1)))
    mag[:bump] += 1
    d = np.zeros(768, np.int64)
    d[dims] = sign[dims] * mag
    return d


def _aligned_row(mu, sign, dims, cap2, pin, pin_code):
    """mu + (sign * magnitudes on `dims`, filled up to the squared norm cap2) with the pin code pin_code(row) wants; the pin's share of the
    norm is what the fill leaves room for (a few rounds: the pin code depends on the rest of the row)"""
    fixed2 = 0
    for _ in range(6):
        row = mu + _fill_to_cap(sign, dims, fixed2, cap2)
        row[pin] = 0
        row[pin] = int(np.clip(pin_code(row), -128, 127))
        need = int(row[pin] - mu[pin]) ** 2
        if need <= fixed2:
            break
        fixed2 = need
    return np.clip(row, -128, 127)


def choose_layout(xb, mode):
    """choose_aux_layout (csrc/dph_plan.h) for a forced stride `mode` (4 or 16), restated: rogue dimensions = mean code further than
    1.2 x 3.5 median spreads from the median mean; the 12 replica slots of stride 16 are dealt out by largest remainder of the ratios.
    Held against the real rule on the CPU, on every shard of this module (tests/test_plan.py)."""
    xi = xb.astype(np.float64)
    mean = xi.mean(0)
    sd = np.sqrt(np.maximum((xi * xi).mean(0) - mean * mean, 0.0))
    mu = np.clip(np.rint(mean), -128, 127)
    sd_med, mu_med = max(1.0, np.sort(sd)[384]), np.sort(mu)[384]
    ratio = np.abs(mu - mu_med) / (3.5 * sd_med)
    rogue = sorted([(-ratio[j], j) for j in range(768) if ratio[j] >= 1.2])[:12]
    lay = np.full(28, -1, np.int32)
    stride = mode if (mode < 16 or rogue) else 4
    lay[:4] = [stride, 4, 0, 64]
    if stride >= 16:
        total = sum(-r for r, _ in rogue)
        want = [-r / total * 12 for r, _ in rogue]
        cnt = [1] * len(rogue)
        for _ in range(12 - len(rogue)):
            gaps = [w - c for w, c in zip(want, cnt)]
            cnt[int(np.argmax(gaps))] += 1
        slots = [j for (_, j), c in zip(rogue, cnt) for _ in range(c)]
        lay[2] = len(slots)
        lay[4:4 + len(slots)] = slots
    return lay


class Shard:
    def __init__(self, name, xb, codec=CODEC_DEFAULT, aux=0):
        self.name, self.xb, self.codec, self.aux = name, np.ascontiguousarray(xb, np.int8), codec, aux
        if aux:
            self.layout = choose_layout(self.xb, aux)
            c = R.aux_constants(self.xb, self.layout)
            self.unit = c["unit"]
        else:
            self.layout, self.unit = None, 1
            c = R.shard_constants(self.xb)
        self.mu, self.n2, self.rmax, self.rmax_all, self.outliers = c["mu"], c["n2"], c["rmax"], c["rmax_all"], c["outliers"]

    def certify(self, x, tau, k, mutate=None, cache=None):
        return R.certify(self.xb, x, self.codec, tau, k, self.layout, self.unit, self.mu, self.rmax, self.rmax_all, self.outliers,
                         mutate=mutate, cache=cache)

    def keys(self, x):
        """exact integer scores [n_q, n_rows], high-digit filter scores, lmax"""
        qs = R.query_scalars(x, self.mu, self.layout, self.unit, self.rmax)
        xf = self.xb.astype(np.float64)
        key = np.rint(qs["m"].astype(np.float64) @ xf.T).astype(np.int64)
        code = (R.host_aux_rows(self.xb, self.mu, self.layout, self.unit)[:, :int(self.layout[1])].sum(1)
                if self.aux else np.zeros(self.xb.shape[0], np.int64))
        Hp = np.rint(qs["hi"].astype(np.float64) @ xf.T).astype(np.int64) + qs["bq"][:, None] * code[None, :]
        return key, Hp, qs["lmax"]


class Set:
    def __init__(self, name, shard, x, tau, k, term, planted=None):
        self.name, self.shard, self.k, self.term = name, shard, k, term
        self.x = np.ascontiguousarray(x, np.float32)
        self.tau = np.ascontiguousarray(tau, np.int32)
        self.planted = planted or {}          # query row -> planted row n*
        self._cache = {}

    def certify(self, mutate=None):
        return self.shard.certify(self.x, self.tau, self.k, mutate=mutate, cache=self._cache)


def _tau_rank(key_row, rank):
    return int(np.sort(key_row)[-rank])


def random_fill(shard, rng, n, rank=40):
    x = rng.normal(0, 0.5, (n, 768)).astype(np.float32)
    key, _, _ = shard.keys(x)
    return x, np.array([_tau_rank(key[r], rank) for r in range(n)], np.int64)


def _pin_code_above(m, row, others_key_max, pin):
    """code of `row` in the pin dimension that lifts its integer score just above `others_key_max`"""
    rest = int(m @ row) - PIN_M * int(row[pin])
    return int(np.floor((others_key_max - rest) / PIN_M)) + 1


# ------------------------------------------------------------------------------------------------------------------ the shards
@functools.lru_cache(maxsize=None)
def build():
    """-> (shards: dict, sets: list)"""
    from densephrases_amd.synth import synthetic_rows
    rng = np.random.default_rng(2024)
    sets = []

    # ================= plain shard: 16 000 kind-0 rows, no outliers, no aux rows
    n_p = 16000
    xb = synthetic_rows(0, n_p, seed=11, kind=0).copy()
    c0 = R.shard_constants(xb)
    assert c0["outliers"].size == 0
    free = list(np.argsort(c0["n2"])[:1200])              # low-norm rows: the slots planted rows take (decoys keep a modest norm)
    hist_edge = (np.sort(c0["n2"])[-R.OUTLIER_MAX] // R.NORM_BIN_W) * R.NORM_BIN_W
    cap2_plain = int(1.18 * hist_edge)                    # a planted row's squared norm: below 1.21 x the cut (no row is set aside)

    def take(n):
        out = [free.pop() for _ in range(n)]
        return np.array(out, np.int64)

    def take_tied(n):
        """slots of n rows that will tie with a planted row, and that row's slot: the LAST of them by row id"""
        got = np.sort(take(n + 1))
        return got[:-1], int(got[-1])

    xb0 = xb.copy()

    # ---- e-aligned, pool rest (k = 10, C = 42): four variants
    ea = []
    for v in range(4):
        pin = 10 + v
        m = _rand_m(rng, pin, 300)
        eps = E45 * rng.choice([-1.0, 1.0], 768)
        eps[pin] = 0.0
        slots, slot = take_tied(42)
        ea.append((pin, m, eps, slot, slots))
    # ---- one-signed residual (k = 1, C = 33)
    os_ = []
    for v in range(4):
        pin = 20 + v
        m = _rand_m(rng, pin, 300)
        eps = np.full(768, E45)
        eps[pin] = 0.0
        slots, slot = take_tied(33)
        os_.append((pin, m, eps, slot, slots))
    # ---- LUT rounding (k = 33, C = 66), one planted row per codec
    lu = []
    for v in range(4):
        pin = 30 + v
        m = _rand_m(rng, pin, 300)
        slots, slot = take_tied(66)
        lu.append((pin, m, slot, slots))
    # ---- q2-aligned, filtered (k = 10): pin, 96 low digits +-1, 8 high digits +-1
    qf = []
    for v in range(4):
        pin = 40 + v
        dims = rng.permutation(np.delete(np.arange(768), pin))
        q1, q2 = np.zeros(768, np.int64), np.zeros(768, np.int64)
        q2[dims[:96]] = rng.choice([-1, 1], 96)
        q1[dims[96:104]] = rng.choice([-1, 1], 8)
        q1[pin] = 127
        qf.append((pin, q1, q2, dims, take(1)[0], take(1)[0]))

    wide_rows = {}

    def plant_plain(mu, xb):
        planted = {}
        for i, (pin, m, eps, slot, slots) in enumerate(ea):
            bg = np.delete(np.arange(n_p), np.append(slots, slot))
            top = int((xb[bg].astype(np.int64) @ m).max())
            xb[slot] = _aligned_row(mu, np.sign(eps).astype(np.int64), np.delete(np.arange(768), pin), cap2_plain, pin,
                                    lambda row: _pin_code_above(m, row, top, pin))
            xb[slots] = _tie_rows(m, xb0[slots], int(m @ xb[slot].astype(np.int64)), pin)
            planted[("ea", i)] = slot
        for i, (pin, m, eps, slot, slots) in enumerate(os_):
            bg = np.delete(np.arange(n_p), np.append(slots, slot))
            target = int((xb[bg].astype(np.int64) @ m).max()) + 30000
            xb[np.append(slots, slot)] = _tie_rows(m, xb0[np.append(slots, slot)], target, pin)
            planted[("os", i)] = slot
        for i, (pin, m, slot, slots) in enumerate(lu):
            bg = np.delete(np.arange(n_p), np.append(slots, slot))
            target = int((xb[bg].astype(np.int64) @ m).max()) + 30000
            xb[slots] = _tie_rows(m, xb0[slots], target, pin)
            for codec in (CODEC_DEFAULT, CODEC_WIDE):
                lut = R.lut32(*codec)
                delta = lut - (np.arange(-128, 128) / float(np.float32(codec[1])) + float(np.float32(codec[0])))
                row = mu.copy()
                for j in range(768):
                    if j == pin or m[j] == 0:
                        continue
                    cand = np.arange(mu[j] - 6, mu[j] + 7)
                    row[j] = cand[np.argmax(np.sign(m[j]) * delta[cand + 128])]      # x32 errs towards the query element's sign
                row = _tie_rows(m, row, target, pin)[0]
                if codec is CODEC_DEFAULT:
                    xb[slot] = row
                else:                                     # the other codec's shard holds this one in the same slot
                    wide_rows[i] = row
            planted[("lu", i)] = slot
        for i, (pin, q1, q2, dims, s1, s2) in enumerate(qf):
            others = np.delete(np.arange(n_p), [s1, s2])
            H = xb[others].astype(np.int64) @ q1
            h4 = int(np.sort(H)[-4])                      # three rows keep a larger H
            row = _aligned_row(mu, q2, dims[:96], cap2_plain, pin, lambda row: np.ceil((h4 - int(q1 @ row)) / 127.0))
            xb[s1] = row
            j = dims[96]                                  # n**: one step along a high digit +-1 -> H + 1, same low-digit sum
            row2 = row.copy()
            row2[j] += q1[j]
            xb[s2] = row2
            planted[("qf", i)] = (s1, s2)
        return planted

    mu = R.shard_constants(xb)["mu"]
    for _ in range(6):
        planted = plant_plain(mu, xb)
        mu2 = R.shard_constants(xb)["mu"]
        if np.array_equal(mu, mu2):
            break
        mu = mu2
    else:
        raise AssertionError("the mean codes did not settle")
    # (each codec's shard holds its own LUT rows only: the other codec's row would sit at the same place in the ranking)
    xb2 = xb.copy()
    for i in range(4):
        xb2[planted[("lu", i)]] = wide_rows[i]
    P = Shard("plain", xb)
    assert P.outliers.size == 0 and P.rmax == P.rmax_all
    P2 = Shard("codec", xb2, codec=CODEC_WIDE)

    def tau_set(shard, x, rank):
        key, _, _ = shard.keys(x)
        return key, np.array([_tau_rank(key[r], rank) for r in range(x.shape[0])], np.int64)

    # e-aligned
    xs = np.stack([craft(m, eps) for _, m, eps, _, _ in ea])
    fx, ft = random_fill(P, rng, 4)
    key, tau = tau_set(P, xs, 80)
    sets.append(Set("e_aligned", P, np.concatenate([xs, fx]), np.concatenate([tau, ft]), 10, "e_r",
                    {i: planted[("ea", i)] for i in range(4)}))
    # one-signed
    xs = np.stack([craft(m, eps) for _, m, eps, _, _ in os_])
    fx, ft = random_fill(P, rng, 4)
    key, tau = tau_set(P, xs, 60)
    sets.append(Set("one_signed", P, np.concatenate([xs, fx]), np.concatenate([tau, ft]), 1, "e_mu",
                    {i: planted[("os", i)] for i in range(4)}))
    # LUT rounding, both codecs
    xs = np.stack([craft(m, np.zeros(768)) for _, m, _, _ in lu])
    for shard, name in ((P, "lut_default"), (P2, "lut_wide_codec")):
        fx, ft = random_fill(shard, rng, 4)
        key, tau = tau_set(shard, xs, 120)
        sets.append(Set(name, shard, np.concatenate([xs, fx]), np.concatenate([tau, ft]), 33, "lut",
                        {i: planted[("lu", i)] for i in range(4)}))
    # q2-aligned, filtered: tau = 128 H(n*) + lmax exactly
    xs = np.stack([craft(_m_of(q1, q2), np.zeros(768)) for _, q1, q2, _, _, _ in qf])
    key, Hp, lmax = P.keys(xs)
    tau = np.array([128 * Hp[i, planted[("qf", i)][0]] + lmax[i] for i in range(4)], np.int64)
    fx, ft = random_fill(P, rng, 4)
    sets.append(Set("q2_filtered", P, np.concatenate([xs, fx]), np.concatenate([tau, ft]), 10, "lmax",
                    {i: planted[("qf", i)][0] for i in range(4)}))
    # fewer than k: tau admits exactly k - 3 rows (k = 100)
    fx, _ = random_fill(P, rng, 8)
    key, Hp, lmax = P.keys(fx)
    tau = np.array([128 * int(np.sort(Hp[r])[-98]) + int(lmax[r]) + 5 for r in range(8)], np.int64)
    sets.append(Set("fewer_than_k", P, fx, tau, 100, "int"))
    # 130 random rows: the 256-row scan kernel
    fx, ft = random_fill(P, rng, 130)
    sets.append(Set("random_130", P, fx, ft, 10, "int"))

    # ================= outlier shard: 10 900 kind-0 rows, a cluster of 9 000 near-copies, 50 saturated rows
    n_o, n_cl, n_sat = 20000, 9000, 50
    xo = synthetic_rows(0, n_o, seed=12, kind=0).copy()
    pins_o = list(range(50, 60))
    pin_cut = 50
    cl_rows = np.arange(1000, 1000 + n_cl)
    cl = np.full((n_cl, 768), 40, np.int64) + rng.choice([-1, 0, 0, 1], (n_cl, 768))
    cl[:, pin_cut] = 127
    xo[cl_rows] = cl
    sat_rows = np.arange(12000, 12000 + n_sat)
    sat = np.where(rng.random((n_sat, 768)) < 0.5, 127, -128)
    sat[:, pins_o] = -128                                  # the crafted rows' pins: saturated rows rank last for them
    xo[sat_rows] = sat
    free = [r for r in np.argsort(R.shard_constants(xo)["n2"]) if r >= 12100][:700]
    # radix cut + a cut-away outlier (k = 33): tiny digits, a one-signed negative residual; o* = -128 everywhere but the pin
    m_cut = np.zeros(768, np.int64)
    dd = rng.permutation(np.delete(np.arange(768), pin_cut))
    m_cut[dd[:200]] = rng.choice([-3, -2, -1, 1, 2, 3], 200)
    m_cut[dd[200]] += 2 - int(m_cut.sum())                # sum of the small digits = 2: o* sits 336 below the cluster's centre
    assert abs(m_cut[dd[200]]) <= 63
    m_cut[pin_cut] = PIN_M
    eps_cut = np.full(768, -E49)
    eps_cut[pin_cut] = 0.0
    xo0 = xo.copy()
    o_star = take(1)[0]
    row = np.full(768, -128, np.int64)
    row[pin_cut] = 127
    xo[o_star] = row
    # outlier in the pool's rest (k = 10, C = 42) and a non-outlier e-aligned row just under the cut (k = 100, C = 200)
    op, uc = [], []
    for v in range(4):
        pin = 51 + v
        m = _rand_m(rng, pin, 60)
        eps = E45 * rng.choice([-1.0, 1.0], 768)
        eps[pin] = 0.0
        slots, slot = take_tied(42)
        op.append((pin, m, eps, slot, slots))
    for v in range(2):
        pin = 56 + v
        m = _rand_m(rng, pin, 300)
        eps = E45 * rng.choice([-1.0, 1.0], 768)
        eps[pin] = 0.0
        slots, slot = take_tied(200)
        uc.append((pin, m, eps, slot, slots))

    def plant_out(mu, cut2, xo):
        planted = {}
        for i, (pin, m, eps, slot, slots) in enumerate(op):
            bg = np.delete(np.arange(n_o), np.append(slots, slot))
            row = np.where(eps > 0, 127, -128).astype(np.int64)
            row[pins_o] = -128                            # (last in the ranking of the other crafted rows, like every saturated row)
            row[pin] = 0
            row[pin] = _pin_code_above(m, row, int((xo[bg].astype(np.int64) @ m).max()), pin)
            assert -128 <= row[pin] < 127
            xo[slot] = row
            xo[slots] = _tie_rows(m, xo0[slots], int(m @ row), pin)
            planted[("op", i)] = slot
        for i, (pin, m, eps, slot, slots) in enumerate(uc):
            bg = np.delete(np.arange(n_o), np.append(slots, slot))
            top = int((xo[bg].astype(np.int64) @ m).max())
            xo[slot] = _aligned_row(mu, np.sign(eps).astype(np.int64), np.delete(np.arange(768), pin), cut2 - 1, pin,
                                    lambda row: _pin_code_above(m, row, top, pin))
            xo[slots] = _tie_rows(m, xo0[slots], int(m @ xo[slot].astype(np.int64)), pin)
            planted[("uc", i)] = slot
        return planted

    c = R.shard_constants(xo)
    for _ in range(6):
        planted_o = plant_out(c["mu"], int(round(c["rmax"] ** 2)), xo)
        c2 = R.shard_constants(xo)
        if np.array_equal(c["mu"], c2["mu"]) and c["rmax"] == c2["rmax"]:
            break
        c = c2
    else:
        raise AssertionError("the mean codes did not settle")
    O = Shard("outlier", xo)
    assert 0 < O.outliers.size <= R.OUTLIER_MAX and O.rmax < O.rmax_all

    xs = np.stack([craft(m, eps) for _, m, eps, _, _ in op])
    fx, ft = random_fill(O, rng, 4)
    key, tau = tau_set(O, xs, 80)
    sets.append(Set("outlier_in_pool", O, np.concatenate([xs, fx]), np.concatenate([tau, ft]), 10, "rmax_all",
                    {i: planted_o[("op", i)] for i in range(4)}))
    xs = np.stack([craft(m, eps) for _, m, eps, _, _ in uc])
    fx, ft = random_fill(O, rng, 6)
    key, tau = tau_set(O, xs, 300)
    sets.append(Set("under_the_cut", O, np.concatenate([xs, fx]), np.concatenate([tau, ft]), 100, "e_r",
                    {i: planted_o[("uc", i)] for i in range(2)}))
    xs = craft(m_cut, eps_cut)[None, :]
    fx, _ = random_fill(O, rng, 7)
    xs = np.concatenate([xs, fx])
    key, _, _ = O.keys(xs)
    tau = np.array([_tau_rank(key[0], 12000)] + [_tau_rank(key[r], 9500 + 1500 * r) for r in range(1, 8)], np.int64)
    sets.append(Set("radix_cut", O, xs, tau, 33, "a_cut", {0: o_star}))

    # ================= kind-4 shards with forced aux rows: the per-row norm code (and the replica digits) carry the filter
    shards = {"plain": P, "codec": P2, "outlier": O}
    for mode in (4, 16):
        n_a = 14000
        xa = synthetic_rows(0, n_a, seed=13 + mode, kind=4).copy()
        A0 = Shard("aux%d" % mode, xa, aux=mode)
        slots = [int(s) for s in np.argsort(A0.n2)[:8]]
        rogue = set(int(d) for d in A0.layout[4:4 + int(A0.layout[2])])
        qa = []
        for v in range(4):
            pin = 200 + v
            ok = np.array([j for j in range(768) if j != pin and j not in rogue])
            dims = rng.permutation(ok)
            # ||q2|| just under 128 b / unit: the norm digit ceil(unit ||q2|| / 128) = b loses as little as the grid allows
            lim2 = (128.0 / A0.unit) ** 2
            g = 2
            D2 = int(lim2 / (1 + 1e-6) // (g * g))
            assert 16 <= D2 <= 600, D2
            q1, q2 = np.zeros(768, np.int64), np.zeros(768, np.int64)
            q2[dims[:D2]] = g * rng.choice([-1, 1], D2)
            q1[dims[D2:D2 + 8]] = rng.choice([-1, 1], 8)
            q1[pin] = 127
            qa.append((pin, q1, q2, dims[:D2], slots[2 * v], slots[2 * v + 1]))
        for _ in range(6):
            A = Shard("aux%d" % mode, xa, aux=mode)
            cap2 = int(A.rmax_all ** 2)
            for pin, q1, q2, d2, s1, s2 in qa:
                others = np.delete(np.arange(n_a), [s1, s2])
                code = R.host_aux_rows(xa[others], A.mu, A.layout, A.unit)[:, :4].sum(1)
                bq = int(np.ceil(A.unit * np.sqrt(float(q2 @ q2)) / 128.0 * (1 + 1e-9)))
                Hp = xa[others].astype(np.int64) @ q1 + bq * code
                h4 = int(np.sort(Hp)[-4])
                own = bq * int(np.ceil(np.sqrt(cap2) / A.unit))      # (the planted row's own norm code, at the cap)
                xa[s1] = _aligned_row(A.mu, np.sign(q2), d2, cap2, pin, lambda row: np.ceil((h4 - own - int(q1 @ row)) / 127.0))
                xa[s2] = xa[others[np.argmax(Hp)]]           # (a copy of the best row: an exact tie in the answer, id order)
            A2 = Shard("aux%d" % mode, xa, aux=mode)
            if np.array_equal(A.mu, A2.mu) and A.rmax_all == A2.rmax_all and np.array_equal(A.layout, A2.layout):
                break
        else:
            raise AssertionError("the aux shard did not settle")
        A = A2
        assert int(A.layout[0]) == mode
        xs = np.stack([craft(_m_of(q1, q2), np.zeros(768)) for _, q1, q2, _, _, _ in qa])
        key, Hp, lmax = A.keys(xs)
        tau = np.array([128 * Hp[i, qa[i][4]] + lmax[i] for i in range(4)], np.int64)
        fx, ft = random_fill(A, rng, 4)
        sets.append(Set("q2_filtered_aux%d" % mode, A, np.concatenate([xs, fx]), np.concatenate([tau, ft]), 10, "lmax",
                        {i: qa[i][4] for i in range(4)}))
        shards[A.name] = A
    for s in sets:
        assert 8 <= s.x.shape[0] <= 16 or s.name == "random_130"
        assert (np.abs(s.tau.astype(np.int64)) < 2 ** 31 - 1).all()
    return shards, sets
