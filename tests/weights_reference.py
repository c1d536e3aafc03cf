"""TEST INFRASTRUCTURE: numpy restatement of samsim_set_weights, samsim_get_weighted_stats and samsim_get_weighted_histogram
(include/samsim.h).

The weights follow the header's rule operation by operation; the exponential of SAMSIM_WEIGHT_GAUSS is the library's own sequence,
samsim_amd/csrc/samsim_pow.h compiled for the host by gcc (exp_helper), or np.exp where there is no gcc -- the caller is told which.
The moments are West's weighted update in np.longdouble, one column after the other; a histogram entry is math.fsum of the weights
that land in it, the entries being those of tests/hist_reference.py."""
import ctypes as C
import functools
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np

from samsim_amd.capi import WSTAT_DTYPE
from tests import hist_reference as hr

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POW_H = os.path.join(ROOT, "samsim_amd", "csrc", "samsim_pow.h")

HELPER_C = r'''#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include "%s"
double helper_exp(double y) { return sp_exp(y); }
/* the GAUSS rule of samsim.h for n values: t = (x - x_min) * c, w = t < 690 ? sp_exp(-t) : 0 */
void helper_gauss(const double *x, long n, double x_min, double c, double *w) {
  for (long i = 0; i < n; ++i) {
    const double t = (x[i] - x_min) * c;
    w[i] = t < 690.0 ? sp_exp(-t) : 0.0;
  }
}
/* the worst error of sp_exp against expl in ulp of the result over n random arguments in [-690, 0], a quarter of them in [-0.69, 0] */
double helper_worst_ulp(long n, unsigned seed) {
  double worst = 0.0;
  srand(seed);
  for (long i = 0; i < n; ++i) {
    const double u = (rand() + rand() / (RAND_MAX + 1.0)) / (RAND_MAX + 1.0);
    const double y = (i %% 4 == 0 ? -0.69 : -690.0) * u;
    const double got = sp_exp(y);
    const long double want = expl((long double)y);
    int e;
    (void)frexp((double)want, &e);
    const double err = (double)fabsl(((long double)got - want) / ldexpl(1.0L, e - 53));
    if (err > worst) worst = err;
  }
  return worst;
}
'''


@functools.lru_cache(maxsize=None)
def exp_helper():
    """samsim_pow.h compiled for the host as a small shared library (helper_exp, helper_gauss, helper_worst_ulp), or None where
    there is no gcc.  -ffp-contract=off as the library is built: t is a difference and a product, each rounded."""
    if shutil.which("gcc") is None:
        return None
    d = tempfile.mkdtemp(prefix="samsim_weights_")
    src, so = os.path.join(d, "helper.c"), os.path.join(d, "libhelper.so")
    with open(src, "w") as f:
        f.write(HELPER_C % POW_H)
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", so, "-lm"])
    lib = C.CDLL(so)
    lib.helper_exp.argtypes, lib.helper_exp.restype = [C.c_double], C.c_double
    lib.helper_gauss.argtypes, lib.helper_gauss.restype = [C.c_void_p, C.c_long, C.c_double, C.c_double, C.c_void_p], None
    lib.helper_worst_ulp.argtypes, lib.helper_worst_ulp.restype = [C.c_long, C.c_uint], C.c_double
    return lib


def in_columns(status, labels=None, group=None):
    """the columns that are IN: status 0 and, with a group, that label"""
    ok = np.asarray(status) == 0
    if group is not None and group >= 0:
        ok = ok & (np.asarray(labels) == group)
    return ok


def direct_weights(x, inn):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(inn & (x > 0.0) & (x < np.inf), x, 0.0)


def gauss_weights(x, inn, scale, exact=True):
    """(w, x_min, how): the GAUSS row.  exact: through the host-compiled header where gcc is there (how == "header"), else -- and
    with exact=False -- through np.exp (how == "np.exp")"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    valid = inn & ~np.isnan(x)
    x_min = float(x[valid].min()) if valid.any() else 0.0
    c = np.float64(0.5) / np.float64(scale)
    lib = exp_helper() if exact else None
    if lib is not None:
        w = np.zeros(x.size)
        lib.helper_gauss(x.ctypes.data, x.size, x_min, float(c), w.ctypes.data)
        how = "header"
    else:
        with np.errstate(invalid="ignore", over="ignore"):
            t = (x - x_min) * c
            w = np.where(t < 690.0, np.exp(-np.where(t < 690.0, t, 0.0)), 0.0)
        how = "np.exp"
    return np.where(inn, w, 0.0), x_min, how


def info_of(w, inn):
    """what samsim_weight_info reports of a row: n_in, n_pos and the two sums (math.fsum: correctly rounded)"""
    pos = w[w > 0.0]
    return dict(n_in=int(inn.sum()), n_pos=int(pos.size), sum_w=math.fsum(pos), sum_w2=math.fsum(pos * pos))


def weighted_moments(rows, w, ok):
    """WSTAT_DTYPE [k] of the k rows over the columns with ok and w > 0: West's update in extended precision, column by column in
    ascending order, the k rows side by side"""
    X = np.stack([np.asarray(r, dtype=np.float64) for r in rows]).astype(LD)
    cols = np.flatnonzero(ok & (w > 0.0))
    out = np.zeros(X.shape[0], dtype=WSTAT_DTYPE)
    if cols.size == 0:
        return out
    W, W2 = LD(0), LD(0)
    mean, m2 = np.zeros(X.shape[0], dtype=LD), np.zeros(X.shape[0], dtype=LD)
    for c in cols:
        wc, x = LD(w[c]), X[:, c]
        W = W + wc
        W2 = W2 + wc * wc
        d = x - mean
        mean = mean + d * (wc / W)
        m2 = m2 + wc * d * (x - mean)
    out["count"] = cols.size
    out["sum_w"], out["sum_w2"] = float(W), float(W2)
    out["mean"], out["var"] = mean.astype(np.float64), (m2 / W).astype(np.float64)
    out["min"], out["max"] = X[:, cols].min(1).astype(np.float64), X[:, cols].max(1).astype(np.float64)
    return out


def weighted_histogram(values, w, ok, nvbins, v0, dv):
    """float64 [nvbins + 2]: math.fsum of the weights of the columns with ok and w > 0 per entry of tests/hist_reference.py"""
    use = ok & (w > 0.0)
    idx = hr.entries(np.asarray(values, dtype=np.float64)[use], nvbins, v0, dv)
    ww = w[use]
    return np.array([math.fsum(ww[idx == i]) for i in range(nvbins + 2)])


def weighted_quantile(values, w, ok, q):
    """the smallest value whose cumulative weight (in ascending order of the values) reaches q times the total"""
    use = ok & (w > 0.0)
    v, ww = np.asarray(values, dtype=np.float64)[use], w[use]
    order = np.argsort(v, kind="stable")
    cum = np.cumsum(ww[order].astype(LD))
    i = min(int(np.searchsorted(cum, LD(q) * cum[-1], side="left")), v.size - 1)
    return float(v[order][i])
