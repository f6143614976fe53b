"""numpy replicas of the query quantiser's digits and of the aux rows (csrc/dph_quant.hip): shared by the aux-row tests and the
certificate restatement (tests/_certificate_ref.py)."""
import numpy as np


def host_digits(x, layout=None):
    """numpy replica of dph_quantize_kernel: q ~= sc * (128 * (q1 + replica digits) + q2).  Returns (q1 [n,768], q2 [n,768],
    X [n,768] = the sum of a dimension's replica digits, sc)."""
    x = x.astype(np.float32).astype(np.float64)
    reps = np.zeros(768, np.int64)
    q2max = 64
    if layout is not None:
        for d in layout[4:4 + int(layout[2])]:
            reps[int(d)] += 1
        q2max = int(layout[3])
    cap = 127.0 * (1 + reps)
    am = (np.abs(x) / (1 + reps)[None, :]).max(1)
    s = np.where(am > 0, am / 127.0, 1.0)
    u = x / s[:, None]
    Q1 = np.clip(np.rint(u), -cap[None, :], cap[None, :])
    q2 = np.clip(np.rint((u - Q1) * 128.0), -q2max, q2max)
    q1 = np.clip(Q1, -127, 127)
    return q1.astype(np.int64), q2.astype(np.int64), (Q1 - q1).astype(np.int64), s / 128.0


def host_aux_rows(xb, mu, layout, unit):
    """numpy replica of dph_aux_build_kernel"""
    stride, n_norm, n_rep = int(layout[0]), int(layout[1]), int(layout[2])
    d = xb.astype(np.int64) - mu[None, :].astype(np.int64)
    n2 = (d * d).sum(1)
    code = np.ceil(np.sqrt(n2.astype(np.float64)) / unit).astype(np.int64)
    code = np.where((code * unit) ** 2 < n2, code + 1, code)
    code = np.where(((code - 1) * unit) ** 2 >= n2, np.maximum(code - 1, 0), code)
    out = np.zeros((xb.shape[0], stride), np.int64)
    for s in range(n_norm):
        out[:, s] = np.clip(code - 127 * s, 0, 127)
    for s in range(n_rep):
        out[:, n_norm + s] = xb[:, int(layout[4 + s])]
    return out
