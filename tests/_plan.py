"""The host planning rules (densephrases_amd/csrc/dph_plan.h) on the CPU: tests/_plan_shim.cpp compiled with a plain g++ -- no HIP, no
sanitizer (it is loaded into this process) -- and bound with ctypes.  A missing compiler is an error: build.py needs g++ as well.

`table()` runs every rule over the fixed grid of tests/golden/plan_rules.json (tools/make_golden_plan.py writes it, tests/test_plan.py
recomputes and compares it): integers and short lists only, doubles as their IEEE bit patterns."""
import ctypes as C
import functools
import os
import struct
import subprocess
import tempfile
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "_plan_shim.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_rules.json")
_CONSTANTS = ("DIM TILE_ROWS QGROUP QROWS MAX_QB CHUNK_PAIRS POOL_CHUNKS BUCKET_CAP POOL_MAX SELECT_C_MAX PASS_MAX UNIT_TILES UNIT_SLOTS "
              "UNIT_LAUNCHES NORM_BINS NORM_BIN_W OUTLIER_MAX AUX_REP_MAX AUX_LAYOUT_WORDS PQ_THREADS PQ_SEG PQ_GROUP PQ_LM_CHUNK PQ_FINAL_CAP "
              "PQ_SAMPLE_TAIL").split()
_tmp = None

i32, i64, u32, u64, f64 = C.c_int, C.c_int64, C.c_uint, C.c_uint64, C.c_double
_P = C.c_void_p


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_P)


@functools.lru_cache(maxsize=None)
def lib():
    global _tmp
    _tmp = tempfile.TemporaryDirectory(prefix="dph_plan_shim_")
    so = os.path.join(_tmp.name, "plan_shim.so")
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-Wall", "-Wextra", "-shared", "-fPIC", SHIM, "-o", so], check=True)
    L = C.CDLL(so)
    sig = {
        "shim_constants": (i32, [_P, i32]), "shim_col_stats": (None, [_P, i64, _P, _P]), "shim_norm_stats": (None, [_P, u64, _P, _P]),
        "shim_norm_unit": (i32, [f64, i32]), "shim_q2_limit": (i32, [i32]), "shim_q2max": (i32, [i32]),
        "shim_choose_layout": (None, [i64, i32, _P, _P, _P, _P]), "shim_aux_rows": (i32, [i64, i32, _P, _P, _P, i32, _P, i32, _P, _P, _P]),
        "shim_layout_roundtrip": (i32, [_P, _P]), "shim_ladder": (i32, [i64, i64, i32, i32, _P, i32, i32, _P, i32]),
        "shim_ladder_units": (i32, [_P, i32, i32, i32, _P, _P, i32, _P]), "shim_select_C": (i32, [i32, i32]), "shim_kp": (i32, [i32, i32, i32, f64]),
        "shim_ladder_fits": (i32, [i32]), "shim_fused_scan": (i64, [i64, i32, _P]), "shim_pass_rows": (i32, [i64, i32, i32, _P]),
        "shim_list_geometry": (None, [_P, i64, i64, i32, _P, _P]), "shim_use_units": (i32, [_P, i32, i32, i32]), "shim_unit_queue": (None, [_P, i32, _P]),
        "shim_pq_top_prefix": (None, [_P, i32, _P]), "shim_pq_scan": (None, [i32, i64, i32, i64, _P, i32, i32, i32, _P]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    return L


@functools.lru_cache(maxsize=None)
def constants():
    out = np.zeros(64, np.int64)
    n = lib().shim_constants(_ptr(out), 64)
    assert n == len(_CONSTANTS)
    return dict(zip(_CONSTANTS, (int(v) for v in out[:n])))


def bits(x):
    """a double as the integer of its bit pattern (the golden table holds integers only)"""
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]


# ------------------------------------------------------------------------------------------------------------------ the rules
def col_stats(sums, n_real):
    sums = np.ascontiguousarray(sums, np.int64)
    mu, sd = np.zeros(768, np.int32), np.zeros(768, np.float64)
    lib().shim_col_stats(_ptr(sums), n_real, _ptr(mu), _ptr(sd))
    return mu, sd


def norm_stats(hist, max2):
    hist = np.ascontiguousarray(hist, np.uint32)
    rmed, out = np.zeros(1), np.zeros(4, np.int64)
    lib().shim_norm_stats(_ptr(hist), int(max2), _ptr(rmed), _ptr(out))
    return dict(rmed=float(rmed[0]), cut_bin=int(out[0]), cut2=int(out[1]), above=int(out[2]), take_cut=bool(out[3]))


def norm_unit(rmax_all, n_norm):
    return lib().shim_norm_unit(float(rmax_all), n_norm)


def q2_limit(unit):
    return lib().shim_q2_limit(unit)


def q2max(unit):
    return lib().shim_q2max(unit)


class Stats:
    """what dph_index_finalize measures on a shard, steps 1 and 2, from the rows on the host"""

    def __init__(self, xb):
        K = constants()
        xi = np.asarray(xb).astype(np.int64)
        self.n_rows = int(xi.shape[0])
        self.mu, self.sd = col_stats(np.concatenate([xi.sum(0), (xi * xi).sum(0)]), self.n_rows)
        n2 = ((xi - self.mu.astype(np.int64)) ** 2).sum(1)
        self.hist = np.bincount(np.minimum(n2 // K["NORM_BIN_W"], K["NORM_BINS"] - 1), minlength=K["NORM_BINS"]).astype(np.uint32)
        self.max2 = int(n2.max())
        self.norms = norm_stats(self.hist, self.max2)
        self.rmax_all = float(np.sqrt(np.float64(self.max2)))
        cut = self.norms["take_cut"] and 0 < self.norms["above"] <= K["OUTLIER_MAX"]
        self.n_out_found = self.norms["above"] if cut else 0
        self.rmax_cut = float(np.sqrt(np.float64(self.norms["cut2"]))) if cut else self.rmax_all

    def facts(self, scale=1.0):
        return np.array([self.norms["rmed"], self.rmax_cut * scale, self.rmax_all * scale], np.float64)


def choose_layout(st, mode):
    lay, norms = np.zeros(28, np.int32), st.facts()
    lib().shim_choose_layout(st.n_rows, mode, _ptr(st.mu), _ptr(st.sd), _ptr(norms), _ptr(lay))
    return lay


def aux_rows(st, mode, cur=None, forced=False, scale=1.0):
    """-> (rc, layout[28], forced, norm_unit, n_out, rmax)"""
    lay, info, rmax, norms = np.zeros(28, np.int32), np.zeros(3, np.int32), np.zeros(1), st.facts(scale)
    cur = None if cur is None else np.ascontiguousarray(cur, np.int32)
    rc = lib().shim_aux_rows(st.n_rows, mode, _ptr(st.mu), _ptr(st.sd), _ptr(norms), st.n_out_found, _ptr(cur), int(forced), _ptr(lay), _ptr(info),
                             _ptr(rmax))
    return rc, lay, bool(info[0]), int(info[1]), int(info[2]), float(rmax[0])


def layout_roundtrip(lay):
    lay, out = np.ascontiguousarray(lay, np.int32), np.zeros(28, np.int32)
    return lib().shim_layout_roundtrip(_ptr(lay), _ptr(out)), out


def ladder(n_tiles, n_rows, grid, fine_stride=0, explicit=(), qb=1):
    ex, out = np.ascontiguousarray(explicit, np.int32), np.zeros(64, np.int32)
    n = lib().shim_ladder(n_tiles, n_rows, grid, fine_stride, _ptr(ex), len(ex), qb, _ptr(out), 64)
    return [int(v) for v in out[:n]]


def ladder_units(lists, fine_stride, n_q, nprobe):
    """-> ([(stride, rowmask)], last_ratio)"""
    s, m, lr = np.zeros(64, np.int32), np.zeros(64, np.uint32), np.zeros(1)
    n = lib().shim_ladder_units(_ptr(lists), fine_stride, n_q, nprobe, _ptr(s), _ptr(m), 64, _ptr(lr))
    return [(int(a), int(b)) for a, b in zip(s[:n], m[:n])], float(lr[0])


def select_C(k, retry=False):
    return lib().shim_select_C(k, int(retry))


def kp(sample_kp, has_levels, c, last_ratio):
    return lib().shim_kp(sample_kp, int(has_levels), c, float(last_ratio))


def ladder_fits(n_levels):
    return bool(lib().shim_ladder_fits(n_levels))


def fused_scan(n_tiles, stride):
    m = np.zeros(1, np.uint32)
    return int(lib().shim_fused_scan(n_tiles, stride, _ptr(m))), int(m[0])


def pass_rows(left, units, max_qb):
    qb = np.zeros(1, np.int32)
    return lib().shim_pass_rows(left, int(units), max_qb, _ptr(qb)), int(qb[0])


def list_geometry(tile_list, nlist):
    """-> (lists facts int64[6] = n_rows, n_tiles, nlist, contiguous, max_list_tiles, total_segs; tile0[nlist + 1])"""
    tl = np.ascontiguousarray(tile_list, np.int32)
    tile0, lists = np.zeros(nlist + 1, np.int32), np.zeros(6, np.int64)
    lib().shim_list_geometry(_ptr(tl), len(tl) * constants()["TILE_ROWS"], len(tl), nlist, _ptr(tile0), _ptr(lists))
    return lists, tile0


def use_units(lists, nprobe, list_major=True, ivf_units=-1):
    return bool(lib().shim_use_units(_ptr(lists), int(list_major), ivf_units, nprobe))


def unit_queue(lists, nprobe):
    out = np.zeros(3, np.int64)
    lib().shim_unit_queue(_ptr(lists), nprobe, _ptr(out))
    return int(out[0]), int(out[1]), bool(out[2])


def pq_top_prefix(sizes):
    sizes = np.ascontiguousarray(sizes, np.int64)
    out = np.zeros(len(sizes) + 1, np.int64)
    lib().shim_pq_top_prefix(_ptr(sizes), len(sizes), _ptr(out))
    return out


PQ_FIELDS = ("seg", "by_rows", "row_codes_max", "row_units_max", "lds_bytes", "lds_bytes_max", "per_seg", "cand_cap", "pair_cap", "unit_cap")


def pq_scan(M, sizes, prefix, rows, k, nprobe):
    out = np.zeros(10, np.int64)
    lib().shim_pq_scan(M, int(sizes.sum()), len(sizes), int(sizes.max()), _ptr(prefix), rows, k, nprobe, _ptr(out))
    return dict(zip(PQ_FIELDS, (int(v) for v in out)))


# ------------------------------------------------------------------------------------------------------------------ the grid
ROWS = (8192, 8224, 300_000, 2_000_000, 170_000_000, 375_000_000)
GRIDS, FINES, KS, NPROBES, MS, NLISTS = (64, 256, 304), (0, 16, 64), (1, 10, 100, 1024), (1, 16, 64, 256), (48, 64, 96, 128), (64, 4096, 65536)
EXPLICIT = (4096, 256, 16)
AUX_MODES = (-1, 0, 4, 16, 32)
SHAPES = ("uniform", "zipf", "giant")


def list_sizes(shape, nlist):
    """rows of every list, without a random number: all alike, 1 / rank, one list of 600 000 among lists of 100"""
    if shape == "uniform":
        return np.full(nlist, 1000, np.int64)
    if shape == "zipf":
        return (4_000_000 // np.arange(1, nlist + 1)).astype(np.int64)
    s = np.full(nlist, 100, np.int64)
    s[nlist // 3] = 600_000
    return s


def tile_list_of(sizes):
    tiles = (np.asarray(sizes) + 31) // 32
    return np.repeat(np.arange(len(sizes), dtype=np.int32), tiles)


@functools.lru_cache(maxsize=None)
def stat_shards():
    """name -> Stats of every shard of tests/_certificate_sets.py and of synth.py kinds 0 to 4 at 20 000 rows"""
    from densephrases_amd.synth import synthetic_rows
    from tests import _certificate_sets as S
    out = {"cert_" + name: Stats(sh.xb) for name, sh in sorted(S.build()[0].items())}
    for kind in range(5):
        out["synth_kind%d" % kind] = Stats(synthetic_rows(0, 20000, seed=5, kind=kind))
    return out


def table():
    T = {"constants": constants()}
    rec = []
    for n in ROWS:
        nt = (n + 31) // 32
        for grid in GRIDS:
            for qb in (1, 2):
                for fine in FINES:
                    for ex in ((), EXPLICIT):
                        st = ladder(nt, n, grid, fine, ex, qb)
                        fused = [list(fused_scan(nt, s)) for s in st]
                        kps = [kp(16, bool(st), select_C(k, r), st[-1] if st else 1.0) for k in KS for r in (False, True)]
                        rec.append([n, grid, qb, fine, len(ex), st, fused, kps, int(ladder_fits(len(st)))])
    T["ladder"] = rec
    T["select_C"] = [[k, select_C(k, False), select_C(k, True)] for k in KS]
    T["pass_rows"] = [[left, u, mq, *pass_rows(left, u, mq)] for left in (1, 64, 128, 129, 200, 256, 300, 700, 900, 1024, 5000) for u in (0, 1) for mq in (1, 2)]
    T["clamp"] = [[u, q2_limit(u), q2max(u)] for u in range(1, 65)]
    T["norm_unit"] = [[r, norm_unit(r / 8.0, 4), norm_unit(r / 8.0, 8)] for r in range(0, 57000, 333)]
    rec = []
    for name, st in stat_shards().items():
        row = {"n_rows": st.n_rows, "mu_crc": zlib.crc32(st.mu.tobytes()), "sd_crc": zlib.crc32(st.sd.tobytes()), "max2": st.max2,
               "norms": [bits(st.norms["rmed"]), st.norms["cut_bin"], st.norms["cut2"], st.norms["above"], int(st.norms["take_cut"])], "modes": []}
        for mode in AUX_MODES:
            rc, lay, forced, unit, n_out, rmax = aux_rows(st, mode)
            assert rc == 0
            # the same layout forced: on these rows it stays; on rows whose norms grew 12-fold its clamp no longer serves
            _, lay_f, f1, u1, _, _ = aux_rows(st, mode, lay, True)
            _, lay_g, f2, u2, _, _ = aux_rows(st, mode, lay, True, scale=12.0)
            row["modes"].append([mode, [int(v) for v in lay], unit, n_out, bits(rmax), [int(f1), u1, int(lay_f[3])], [int(f2), u2, int(lay_g[3])]])
        rec.append([name, row])
    T["aux"] = rec
    rec_l, rec_p = [], []
    for nlist in NLISTS:
        for shape in SHAPES:
            sizes = list_sizes(shape, nlist)
            lists, tile0 = list_geometry(tile_list_of(sizes), nlist)
            prefix = pq_top_prefix(sizes)
            row = {"lists": [int(v) for v in lists], "tile0_crc": zlib.crc32(tile0.tobytes()), "prefix_crc": zlib.crc32(prefix.tobytes()), "nprobe": []}
            for np_ in NPROBES:
                lad = []
                for fine in FINES:
                    for nq in (64, 700, 1024):
                        lv, lr = ladder_units(lists, fine, nq, np_)
                        lad.append([fine, nq, [list(x) for x in lv], bits(lr), [kp(16, bool(lv), select_C(k), lr) for k in KS]])
                row["nprobe"].append([np_, [int(use_units(lists, np_, ivf_units=u)) for u in (-1, 0, 1)], list(map(int, unit_queue(lists, np_))), lad])
                for M in MS:
                    for k in KS:
                        rec_p.append([nlist, shape, np_, M, k, *pq_scan(M, sizes, prefix, 1024, k, np_).values()])
            rec_l.append([nlist, shape, row])
    T["lists"] = rec_l
    T["pq_fields"] = list(PQ_FIELDS)
    T["pq"] = rec_p
    return T
