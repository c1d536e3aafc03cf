"""TEST INFRASTRUCTURE: numpy restatement of samsim_get_weighted_profile_histogram (include/samsim.h) over a host State and a weight
row.

The per-column bin values and the condition under which a column contributes to a bin are those of
tests/hist_reference.profile_values, the entry of a value is tests/hist_reference.entries, and a column COUNTS as
tests/weighted_profile_reference.counting says (status 0, the right label with a group, w > 0).  Per (bin, entry) the sum of the
weights is math.fsum of them: correctly rounded, whatever the order."""
import math

import numpy as np

from tests import hist_reference as hr


def entries_of_bins(v, has, nvbins, v0, dv):
    """int [nbins, ncol]: the entry of every contributing column's bin value, -1 where the column does not contribute; the columns
    are not yet restricted to those that count, so one table serves every group and weight row"""
    en = np.full(v.shape, -1, dtype=np.int64)
    for b in range(v.shape[0]):
        cols = np.flatnonzero(has[b])
        if cols.size:
            en[b, cols] = hr.entries(v[b, cols], nvbins, v0, dv)
    return en


def table_from_entries(en, w, ok, nvbins):
    """wsum [nbins, nvbins + 2]: per (bin, entry) math.fsum of w over the counting columns (ok) that land there; +0.0 elsewhere"""
    w = np.asarray(w, dtype=np.float64)
    out = np.zeros((en.shape[0], nvbins + 2))
    for b in range(en.shape[0]):
        cols = np.flatnonzero((en[b] >= 0) & ok)
        if not cols.size:
            continue
        e = en[b, cols]
        order = np.argsort(e, kind="stable")
        e, ww = e[order], w[cols[order]]
        cuts = np.flatnonzero(np.diff(e)) + 1
        for i, part in zip(e[np.concatenate(([0], cuts))], np.split(ww, cuts)):
            out[b, i] = math.fsum(part)
    return out


def weighted_joint_histogram(v, has, w, ok, nvbins, v0, dv):
    """wsum [nbins, nvbins + 2] of the values hist_reference.profile_values returned, over the columns `ok`
    (weighted_profile_reference.counting)"""
    return table_from_entries(entries_of_bins(v, has, nvbins, v0, dv), w, ok, nvbins)
