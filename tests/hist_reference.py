"""TEST INFRASTRUCTURE: plain numpy restatement of samsim_get_histogram / samsim_get_profile_histogram (include/samsim.h) over a
host State, in the header's operation order.

The edges are v0 + j*dv (product rounded, then the sum); the entry of a value is the number of edges that are <= the value, so a
NaN lands in entry 0.  The per-column bin values are those of tests/profile_reference.py -- the layers k in ascending order, the
depth coordinate by sequential additions, overlaps summed over ascending k, one IEEE division per (column, bin) -- returned per
column instead of as statistics."""
import numpy as np

from tests.profile_reference import column_thickness, layer_values


def edges(nvbins, v0, dv):
    return np.float64(v0) + np.arange(nvbins + 1, dtype=np.float64) * np.float64(dv)


def entries(v, nvbins, v0, dv):
    """idx(v) of the header for every value"""
    E = edges(nvbins, v0, dv)
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (E[None, :] <= v[:, None]).sum(1)


def histogram_reference(v, nvbins, v0, dv):
    """counts [nvbins + 2] of the values v"""
    return np.bincount(entries(v, nvbins, v0, dv), minlength=nvbins + 2).astype(np.int64)


def scalar_histogram_reference(values, status, nvbins, v0, dv, labels=None, ngroups=None):
    """samsim_get_histogram: counts [nvbins+2] over the columns with status == 0, or [ngroups, nvbins+2] per label"""
    ok = np.asarray(status) == 0
    if labels is None:
        return histogram_reference(values[ok], nvbins, v0, dv)
    return np.stack([histogram_reference(values[ok & (labels == g)], nvbins, v0, dv) for g in range(ngroups)])


def profile_values(st, status, name, axis="layer", origin="top", nbins=None, z0=0.0, dz=None):
    """(v [nbins, ncol], contributes [nbins, ncol]): the value of every column in every bin and whether the column contributes to
    the bin, as samsim_get_profile_stats defines both"""
    ok = np.asarray(status) == 0
    na = st.n_active.astype(np.int64)
    cols = np.arange(st.ncol)
    nbins = st.nlayer if nbins is None else nbins
    a = layer_values(st, name)
    v = np.zeros((nbins, st.ncol))
    has = np.zeros((nbins, st.ncol), dtype=bool)
    if axis == "layer":
        for b in range(nbins):
            k = np.full(st.ncol, b + 1) if origin == "top" else na - b        # 1-based layer of bin b
            sel = ok & (k >= 1) & (k <= na)
            v[b, sel] = a[k[sel] - 1, cols[sel]]
            has[b] = sel
        return v, has
    assert axis == "depth" and dz is not None
    thick = st.arr("thick")
    e = z0 + np.arange(nbins + 1, dtype=np.float64) * dz
    e0, e1 = e[:-1, None], e[1:, None]
    H = column_thickness(st)
    L = np.zeros((nbins, st.ncol))
    W = np.zeros((nbins, st.ncol))
    Z = np.zeros(st.ncol)
    for k in range(1, int(na[ok].max()) + 1 if ok.any() else 1):
        act = ok & (k <= na)
        Zn = np.where(k <= na, Z + thick[k - 1], Z)
        lo, hi = (Z, Zn) if origin == "top" else (H - Zn, H - Z)
        o = np.maximum(0.0, np.minimum(hi[None, :], e1) - np.maximum(lo[None, :], e0))
        o = np.where(act[None, :], o, 0.0)
        L += o
        W += np.where(act[None, :], o * a[k - 1][None, :], 0.0)
        Z = Zn
    has = ok[None, :] & (L > 0.0)
    v[has] = W[has] / L[has]
    return v, has


def joint_histogram(v, has, nvbins, v0, dv, select=None):
    """counts [nbins, nvbins+2] of the values profile_values returned; select: a column mask (a group)"""
    if select is not None:
        has = has & select[None, :]
    return np.stack([histogram_reference(v[b, has[b]], nvbins, v0, dv) for b in range(v.shape[0])])
