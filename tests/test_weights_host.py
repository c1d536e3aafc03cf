"""The weight row and the weighted reductions without a GPU: the header, the ctypes mirror, the Fortran binding and the library's
symbols agree, NULL arguments are refused, the exponential the weights are formed with stays within 1 ulp of expl on [-690, 0]
(samsim_pow.h compiled for the host), the numpy restatement (tests/weights_reference.py) agrees with np.average and np.histogram on
random data, and the two host-side helpers give the numbers written out below on hand-made cases."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import samsim_amd
from samsim_amd import capi
from samsim_amd.capi import HistBins, WeightInfo, WeightSpec, WSTAT_DTYPE
from tests import weights_reference as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("samsim_set_weights", "samsim_get_weights", "samsim_get_weighted_stats", "samsim_get_weighted_histogram")


def code_of_header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "samsim.h")).read(), flags=re.S)


def fields_of(code, name):
    body = code[code.index("typedef struct %s {" % name):code.index("} %s;" % name)]
    ctypes_of = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}
    out = []
    for ctype, decl in re.findall(r"(int32_t|int64_t|double)\s+([^;]+);", body):
        out += [(n.strip(), ctypes_of[ctype]) for n in decl.split(",")]
    return out


def test_header_declares_the_functions_and_constants():
    code = " ".join(code_of_header().split())
    for decl in ("int samsim_set_weights(samsim_handle *h, const samsim_weight_spec *spec, samsim_weight_info *info );",
                 "int samsim_get_weights(samsim_handle *h, int64_t col0, int64_t ncols, double *out );",
                 "int samsim_get_weighted_stats(samsim_handle *h, int32_t nslots, const int32_t *slots, int32_t group, samsim_wstat *out );",
                 "int samsim_get_weighted_histogram(samsim_handle *h, int32_t slot, const samsim_hist_bins *vb, int32_t group, double *wsum );"):
        assert decl in code, decl
    assert re.search(r"#define SAMSIM_WEIGHT_SLOT 0x40000\b", code)
    assert "#define SAMSIM_WEIGHT_SCRATCH_BYTES (4ull << 20)" in code
    assert "enum samsim_weight_kind { SAMSIM_WEIGHT_DIRECT = 0, SAMSIM_WEIGHT_GAUSS = 1 };" in code
    assert capi.WEIGHT_KINDS == {"direct": 0, "gauss": 1}
    assert "#define SAMSIM_ABI_VERSION 6" in code and capi.ABI_VERSION == 6


def test_the_weight_slot_lies_above_the_score_slots():
    assert capi.weight_slot() == 0x40000 > capi.score_slot(capi.NSF - 1)
    assert capi._slot(capi.weight_slot()) == 0x40000


def test_struct_layouts_match_the_ctypes_mirrors():
    code = code_of_header()
    assert fields_of(code, "samsim_weight_spec") == list(WeightSpec._fields_) and C.sizeof(WeightSpec) == 32
    assert fields_of(code, "samsim_weight_info") == list(WeightInfo._fields_) and C.sizeof(WeightInfo) == 40
    wstat = fields_of(code, "samsim_wstat")
    assert [n for n, _ in wstat] == ["count", "sum_w", "sum_w2", "mean", "var", "min", "max"] == list(WSTAT_DTYPE.names)
    assert WSTAT_DTYPE.itemsize == 56 and [WSTAT_DTYPE.fields[n][1] for n in WSTAT_DTYPE.names] == list(range(0, 56, 8))
    assert WSTAT_DTYPE["count"] == np.int64 and all(WSTAT_DTYPE[n] == np.float64 for n in WSTAT_DTYPE.names[1:])
    s = WeightSpec.make(capi.score_slot("J_SUM"), scale=4.0, group=2)
    assert (s.struct_size, s.kind, s.slot, s.group, s.scale, s.reserved) == (32, 1, 0x30005, 2, 4.0, 0.0)
    s = WeightSpec.make("N_active", "direct")
    assert (s.kind, s.slot, s.group, s.scale) == (0, -1, -1, 0.0)


def test_fortran_binding_names_every_symbol():
    binding = open(os.path.join(ROOT, "host", "capi_binding.f90")).read()
    for name in FUNCTIONS:
        assert re.search(r"BIND\(C,\s*NAME\s*=\s*['\"]%s['\"]\)" % name, binding, re.I), name
    for name in ("samsim_weight_spec", "samsim_weight_info", "samsim_wstat"):
        assert re.search(r"TYPE,\s*BIND\(C\)\s*::\s*%s\b" % name, binding, re.I), name
    for name in ("SAMSIM_WEIGHT_SLOT", "SAMSIM_WEIGHT_DIRECT", "SAMSIM_WEIGHT_GAUSS"):
        assert re.search(r"\b%s\b" % name, binding), name


def test_library_exports_and_refuses_null_arguments():
    lib = samsim_amd.load()
    assert lib.samsim_abi_version() == 6
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    sig = {"samsim_set_weights": [vp, C.POINTER(WeightSpec), C.POINTER(WeightInfo)], "samsim_get_weights": [vp, i64, i64, vp],
           "samsim_get_weighted_stats": [vp, i32, vp, i32, vp], "samsim_get_weighted_histogram": [vp, i32, C.POINTER(HistBins), i32, vp]}
    assert sorted(sig) == sorted(FUNCTIONS)
    f = {}
    for name, args in sig.items():
        f[name] = getattr(lib, name)
        f[name].argtypes, f[name].restype = args, C.c_int
    spec, info = WeightSpec.make("thickness"), WeightInfo(-7, -7, -77.0, -77.0, -77.0)
    assert f["samsim_set_weights"](None, C.byref(spec), C.byref(info)) == -1
    assert f["samsim_set_weights"](None, None, None) == -1
    assert (info.n_in, info.n_pos, info.x_min, info.sum_w, info.sum_w2) == (-7, -7, -77.0, -77.0, -77.0)
    out = np.full(8, -77.0)
    slots = (C.c_int32 * 1)(0)
    vb = capi.hist_bins(4, 0.0, 1.0)
    assert f["samsim_get_weights"](None, 0, 4, out.ctypes.data) == -1
    assert f["samsim_get_weighted_stats"](None, 1, slots, -1, out.ctypes.data) == -1
    assert f["samsim_get_weighted_histogram"](None, 0, C.byref(vb), -1, out.ctypes.data) == -1
    assert (out == -77.0).all()


def test_the_exponential_of_the_weights_on_its_range():
    """sp_exp of samsim_pow.h, compiled by gcc, against expl over 4e6 random arguments in [-690, 0], a quarter of them in
    [-0.69, 0]: under 1 ulp of the result (0.888 ulp on this sample when the feature was written); sp_exp(-0.0) is exactly 1.0"""
    lib = wr.exp_helper()
    assert lib is not None, "needs gcc, as tests/test_host_logic.py does"
    worst = lib.helper_worst_ulp(4_000_000, 12345)
    print("worst error of sp_exp on [-690, 0]: %.4f ulp" % worst)
    assert 0.0 < worst < 1.0, worst
    assert lib.helper_exp(-0.0) == 1.0 and lib.helper_exp(0.0) == 1.0
    assert 0.0 < lib.helper_exp(-689.999) < 1e-299


# ------------------------------------------------------------------------------------------------------------ the reference
def test_reference_weights():
    nan, inf = float("nan"), float("inf")
    x = np.array([3.0, 1.0, nan, 1.0, 5.0, -2.0, inf, 2000.0])
    status = np.array([0, 0, 0, 0, 0, 7, 0, 0])
    inn = wr.in_columns(status)
    assert wr.direct_weights(x, inn).tolist() == [3.0, 1.0, 0.0, 1.0, 5.0, 0.0, 0.0, 2000.0]
    assert wr.direct_weights(np.array([-1.0, 0.0, -0.0, 2.0]), np.ones(4, bool)).tolist() == [0.0, 0.0, 0.0, 2.0]
    for exact in (True, False):
        w, x_min, how = wr.gauss_weights(x, inn, 1.0, exact)
        assert x_min == 1.0 and how in ("header", "np.exp")              # the stopped column's -2 does not count
        assert w[1] == 1.0 and w[3] == 1.0 and w[2] == 0.0 and w[5] == 0.0 and w[6] == 0.0 and w[7] == 0.0   # t = 999.5 >= 690
        assert abs(w[0] - np.exp(-1.0)) <= 2 * np.spacing(np.exp(-1.0)) and abs(w[4] - np.exp(-2.0)) <= 2 * np.spacing(np.exp(-2.0))
    w, x_min, _ = wr.gauss_weights(x, wr.in_columns(status, np.array([0, 1, 1, 0, 0, 0, 0, 0]), 1), 0.25)
    assert x_min == 1.0 and w.tolist() == [0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    w, x_min, _ = wr.gauss_weights(np.full(3, nan), np.ones(3, bool), 1.0)
    assert x_min == 0.0 and w.tolist() == [0.0, 0.0, 0.0]
    info = wr.info_of(np.array([0.5, 0.0, 0.25, 0.0]), np.array([True, True, True, False]))
    assert info == dict(n_in=3, n_pos=2, sum_w=0.75, sum_w2=0.3125)


def test_reference_moments_and_histogram_against_numpy():
    rng = np.random.default_rng(11)
    n = 5000
    rows = [rng.normal(3.0, 2.0, n), 1.0e6 + rng.uniform(0.0, 1.0, n), rng.integers(1, 9, n).astype(np.float64)]
    w = np.where(rng.uniform(size=n) < 0.3, 0.0, rng.exponential(1.0, n))
    ok = rng.uniform(size=n) < 0.9
    use = ok & (w > 0.0)
    q = wr.weighted_moments(rows, w, ok)
    for i, r in enumerate(rows):
        mean = np.average(r[use], weights=w[use])
        var = np.average((r[use] - mean) ** 2, weights=w[use])
        assert q["count"][i] == use.sum() and q["min"][i] == r[use].min() and q["max"][i] == r[use].max()
        assert abs(q["mean"][i] - mean) <= 1e-13 * max(1.0, abs(mean)) and abs(q["var"][i] - var) <= 1e-11 * var
        assert abs(q["sum_w"][i] - w[use].sum()) <= 1e-13 * w[use].sum() and abs(q["sum_w2"][i] - (w[use] ** 2).sum()) <= 1e-12 * (w[use] ** 2).sum()
    # equal values: their mean, and no variance; no counting column: zeros
    q = wr.weighted_moments([np.full(n, 0.1)], w, ok)
    assert q["mean"][0] == 0.1 and q["var"][0] == 0.0
    q = wr.weighted_moments(rows, np.zeros(n), ok)
    assert q.tobytes() == np.zeros(3, dtype=WSTAT_DTYPE).tobytes()
    nv, v0, dv = 12, -2.0, 0.75
    got = wr.weighted_histogram(rows[0], w, ok, nv, v0, dv)
    edges = np.concatenate([[-np.inf], capi.hist_edges(nv, v0, dv), [np.inf]])
    want = np.histogram(rows[0][use], bins=edges, weights=w[use])[0]
    assert got.shape == (nv + 2,) and (np.abs(got - want) <= 1e-12 * np.maximum(1.0, want)).all() and got[0] > 0 and got[-1] > 0
    v = rows[0].copy()
    v[use.nonzero()[0][:5]] = np.nan                                     # a NaN lands in entry 0
    assert wr.weighted_histogram(v, w, ok, nv, v0, dv)[0] > got[0]
    for qq in (0.05, 0.5, 0.95):
        x = wr.weighted_quantile(rows[0], w, ok, qq)
        below = w[use & (rows[0] < x)].sum() / w[use].sum()
        at = w[use & (rows[0] <= x)].sum() / w[use].sum()
        assert below < qq <= at + 1e-15


# ------------------------------------------------------------------------------------------------------------ the two helpers
def test_weighted_quantile_bracket_on_hand_made_sums():
    wsum = np.array([0.0, 1.0, 0.0, 2.0, 1.0, 0.0])                       # nvbins = 4, edges 10, 11, 12, 13, 14
    b = lambda q: capi.weighted_quantile_bracket(wsum, 10.0, 1.0, q)      # noqa: E731
    assert b(0.0) == (10.0, 11.0)                                         # the first entry that holds weight
    assert b(0.25) == (10.0, 11.0)                                        # the cumulative 1.0 reaches 0.25 * 4
    assert b(0.26) == (12.0, 13.0) and b(0.5) == (12.0, 13.0) and b(0.75) == (12.0, 13.0)
    assert b(0.76) == (13.0, 14.0) and b(1.0) == (13.0, 14.0)
    assert capi.weighted_quantile_bracket([2.0, 0.0, 0.0, 1.0], 0.0, 1.0, 0.5) == (-np.inf, 0.0)
    assert capi.weighted_quantile_bracket([1.0, 0.0, 0.0, 3.0], 0.0, 1.0, 0.5) == (2.0, np.inf)
    for bad, q in (([0.0, 0.0, 0.0], 0.5), ([1.0, -1.0, 1.0], 0.5), ([1.0, float("nan"), 1.0], 0.5), ([1.0, 1.0], 0.5), ([1.0, 1.0, 1.0], 1.5)):
        with pytest.raises(ValueError):
            capi.weighted_quantile_bracket(bad, 0.0, 1.0, q)
    # integer weights: the bracket of the unweighted rule
    counts = np.array([3, 0, 5, 2, 0, 1])
    for q in (0.0, 0.1, 0.5, 0.9, 1.0):
        assert capi.weighted_quantile_bracket(counts.astype(np.float64), -1.0, 0.5, q) == capi.quantile_bracket(counts, -1.0, 0.5, q), q


def test_weighted_profile_mean_on_a_hand_made_bin():
    """three columns in a bin with weights 1, 3, 0 and values 2, 4, 100: sum w y / sum w = 14 / 4; from the moments the regression
    returns with the weight as predictor: mean_x = 4/3, mean_y = 106/3, cov = mean(w y) - mean_x mean_y"""
    w, y = np.array([1.0, 3.0, 0.0]), np.array([2.0, 4.0, 100.0])
    q = np.zeros(3, dtype=capi.PAIR_STAT_DTYPE)
    q[0] = (3, w.mean(), y.mean(), w.var(), y.var(), (w * y).mean() - w.mean() * y.mean())
    q[1] = (2, 0.0, 5.0, 0.0, 1.0, 0.0)                                    # no weight in the bin
    q[2] = (0, 0.0, 0.0, 0.0, 0.0, 0.0)                                    # no column in the bin
    got = capi.weighted_profile_mean(q)
    assert abs(got[0] - 3.5) <= 1e-14 and got[1] == 0.0 and got[2] == 0.0
