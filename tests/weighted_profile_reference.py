"""TEST INFRASTRUCTURE: numpy restatement of samsim_get_weighted_profile_stats and samsim_get_weighted_covariance
(include/samsim.h) over a host State and a weight row.

Profiles: built on tests/sens_reference.bin_values, which returns every bin's contributing columns and their values v from
tests/profile_reference.py itself.  A column COUNTS if its status is 0, its label passes the group and its weight is positive; per
bin, over the counting contributors, the weighted mean and variance in two passes in np.longdouble (the mean first, then the
weighted squared deviations), sum_w and sum_w2 by math.fsum (correctly rounded), min and max exact.  Covariances likewise: the
weighted means first, then the weighted products of deviations."""
import math

import numpy as np

from samsim_amd.capi import WSTAT_DTYPE
from tests import sens_reference as cr

LD = np.longdouble


def counting(status, w, labels=None, group=None):
    """the columns that count: status 0, the right label with a group, and w > 0 (a NaN weight does not count)"""
    with np.errstate(invalid="ignore"):
        return cr.counting(status, labels, group) & (np.asarray(w) > 0.0)


def wstat_of(v, w):
    """one WSTAT_DTYPE record of the values v with the positive weights w (equally long, possibly empty)"""
    out = np.zeros((), dtype=WSTAT_DTYPE)
    v, w = np.asarray(v, dtype=np.float64), np.asarray(w, dtype=np.float64)
    assert v.shape == w.shape and v.ndim == 1
    if v.size == 0:
        return out
    assert (w > 0.0).all()
    wl, vl = w.astype(LD), v.astype(LD)
    W = wl.sum()
    mean = (wl * vl).sum() / W
    d = vl - mean
    var = (wl * d * d).sum() / W
    out["count"] = v.size
    out["sum_w"], out["sum_w2"] = math.fsum(w), math.fsum(w * w)
    out["mean"], out["var"], out["min"], out["max"] = float(mean), float(var), v.min(), v.max()
    return out


def from_bins(bins, w, ok):
    """(WSTAT_DTYPE [nbins], per bin the counting contributors) from one array's list of sens_reference.bin_values -- per bin the
    contributing columns among those with status 0 and their values -- and the columns that count: a column's bin value does not
    depend on the other columns, so the counting contributors are the contributors that count"""
    w = np.asarray(w, dtype=np.float64)
    out, who = np.zeros(len(bins), dtype=WSTAT_DTYPE), []
    for b, (cols, v) in enumerate(bins):
        keep = ok[cols]
        out[b] = wstat_of(v[keep], w[cols[keep]])
        who.append(cols[keep])
    return out, who


def weighted_profile_reference(st, status, w, names, labels=None, group=None, **kw):
    """({name: WSTAT_DTYPE [nbins]}, {name: per bin the counting contributors}); st must be writable (bin_values borrows T)"""
    ok = counting(status, w, labels, group)
    res, who = {}, {}
    for n, bins in cr.bin_values(st, status, names, **kw).items():
        res[n], who[n] = from_bins(bins, w, ok)
    return res, who


def weighted_covariance_reference(rows, w, ok):
    """(count, sum_w, sum_w2, mean [k], cov [k, k]) of the k rows over the columns with ok and w > 0; mean and cov in np.longdouble"""
    w = np.asarray(w, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        use = np.asarray(ok) & (w > 0.0)
    k = len(rows)
    mean, cov = np.zeros(k, dtype=LD), np.zeros((k, k), dtype=LD)
    if not use.any():
        return 0, 0.0, 0.0, mean, cov
    ww = w[use]
    wl = ww.astype(LD)
    W = wl.sum()
    dev = []
    for i, r in enumerate(rows):
        x = np.asarray(r, dtype=np.float64)[use].astype(LD)
        mean[i] = (wl * x).sum() / W
        dev.append(x - mean[i])
    for i in range(k):
        for j in range(i, k):
            cov[i, j] = cov[j, i] = (wl * dev[i] * dev[j]).sum() / W
    return int(use.sum()), math.fsum(ww), math.fsum(ww * ww), mean, cov
