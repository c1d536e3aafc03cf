"""TEST INFRASTRUCTURE: numpy restatement of samsim_get_covariance and samsim_get_profile_regression (include/samsim.h) in extended
precision (np.longdouble, two passes: the means first, then the products of deviations) over a host State.

Scalars: over the rows of get_state() of the columns with status 0 and the right label.  Profiles: over the per-column bin values
that tests/profile_reference.py forms -- its own loops, taken as they hand their values to its _stats()."""
import contextlib

import numpy as np

from samsim_amd.capi import A, PAIR_STAT_DTYPE
from tests import profile_reference as pr

LD = np.longdouble


def pair_moments(x, y):
    """(count, mean_x, mean_y, var_x, var_y, cov) of two equally long samples: population moments, extended precision"""
    x, y = np.asarray(x, dtype=LD), np.asarray(y, dtype=LD)
    assert x.shape == y.shape and x.ndim == 1
    n = x.size
    if n == 0:
        return 0, LD(0), LD(0), LD(0), LD(0), LD(0)
    mx, my = x.sum() / n, y.sum() / n
    dx, dy = x - mx, y - my
    return n, mx, my, (dx * dx).sum() / n, (dy * dy).sum() / n, (dx * dy).sum() / n


def covariance_matrix(rows):
    """(count, mean [k], cov [k, k]) of k equally long samples, extended precision throughout"""
    rows = [np.asarray(r, dtype=LD) for r in rows]
    k, n = len(rows), rows[0].size
    mean, cov = np.zeros(k, dtype=LD), np.zeros((k, k), dtype=LD)
    if n == 0:
        return 0, mean, cov
    dev = []
    for i, r in enumerate(rows):
        mean[i] = r.sum() / n
        dev.append(r - mean[i])
    for i in range(k):
        for j in range(i, k):
            cov[i, j] = cov[j, i] = (dev[i] * dev[j]).sum() / n
    return n, mean, cov


def counting(status, labels=None, group=None):
    """the columns that count: status 0 and, with a group, that label"""
    ok = np.asarray(status) == 0
    if group is not None and group >= 0:
        ok = ok & (np.asarray(labels) == group)
    return ok


def scalar_row(s, name):
    return s.n_active.astype(np.float64) if name == "N_active" else s.sc(name)


def covariance_reference(s, status, names, labels=None, group=None):
    ok = counting(status, labels, group)
    return covariance_matrix([scalar_row(s, n)[ok] for n in names])


@contextlib.contextmanager
def _captured():
    """what profile_reference hands to its _stats(): per call the list of the bins' value arrays"""
    calls, orig = [], pr._stats

    def capture(values_per_bin):
        calls.append([np.array(v) for v in values_per_bin])
        return orig(values_per_bin)
    pr._stats = capture
    try:
        yield calls
    finally:
        pr._stats = orig


def bin_values(st, status, names, **kw):
    """{name: per bin (columns, values)}: the contributing columns of every bin in ascending order and their values, from
    profile_reference itself.  The columns come from a second call with the column index written into every layer of T (a column's
    bin value is then its index, to within a rounding of the depth average): the state is put back afterwards."""
    names = list(names)
    with _captured() as calls:
        pr.profile_reference(st, status, names, **kw)
    values = dict(zip(names, calls))
    keep = st.lay[A["T"]].copy()
    try:
        st.lay[A["T"]][:] = np.arange(st.ncol, dtype=np.float64)[None, :]
        with _captured() as calls:
            pr.profile_reference(st, status, ["T"], **kw)
    finally:
        st.lay[A["T"]][:] = keep
    cols = [np.rint(c).astype(np.int64) for c in calls[0]]
    for n in names:
        assert [v.size for v in values[n]] == [c.size for c in cols]
    return {n: list(zip(cols, values[n])) for n in names}


def profile_regression_reference(st, status, names, predictor, labels=None, group=None, **kw):
    """{name: PAIR_STAT_DTYPE [nbins]} (rounded from extended precision)"""
    status = np.where(counting(status, labels, group), 0, 1).astype(np.int32)
    x = scalar_row(st, predictor)
    res = {}
    for n, bins in bin_values(st, status, names, **kw).items():
        out = np.zeros(len(bins), dtype=PAIR_STAT_DTYPE)
        for b, (cols, v) in enumerate(bins):
            out[b] = tuple(float(q) if i else q for i, q in enumerate(pair_moments(x[cols], v)))
        res[n] = out
    return res
