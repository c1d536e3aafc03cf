"""TEST INFRASTRUCTURE: plain numpy restatement of samsim_get_profile_stats (include/samsim.h) over a host State.

Written from the formulas of the header, in their operation order: a loop over the layers k in ascending order, the depth
coordinate by sequential additions, the bin edges as z0 + b*dz (product rounded, then the sum), overlaps summed over
ascending k, one IEEE division per (column, bin)."""
import numpy as np

from samsim_amd.capi import A, STAT_DTYPE


def layer_values(st, name):
    """a_k of the header for every (layer, column): the stored array; S_abs/m where m != 0 for the bulk salinity"""
    if name != "S_bu":
        return st.arr(name)
    s, m = st.arr("S_abs"), st.arr("m")
    stored = st.arr("S_bu") if st.lay.shape[0] > A["S_bu"] else np.zeros_like(m)   # (a prognostic-only State holds no S_bu)
    return np.where(m != 0.0, s / np.where(m != 0.0, m, 1.0), stored)


def _stats(values_per_bin):
    out = np.zeros(len(values_per_bin), dtype=STAT_DTYPE)
    for b, v in enumerate(values_per_bin):
        if v.size:
            out[b] = (v.size, v.mean(), v.min(), v.max(), v.std())
    return out


def column_thickness(st):
    """H = Z_Na of every column, Z_k = Z_{k-1} + thick(k)"""
    thick, na = st.arr("thick"), st.n_active
    Z = np.zeros(st.ncol)
    for k in range(1, int(na.max()) + 1):
        Z = np.where(k <= na, Z + thick[k - 1], Z)
    return Z


def profile_reference(st, status, names, axis="layer", origin="top", nbins=None, z0=0.0, dz=None):
    """{name: structured array [nbins] (count, mean, min, max, std)} over the columns with status == 0"""
    names = list(names)
    ok = np.asarray(status) == 0
    na = st.n_active.astype(np.int64)
    cols = np.arange(st.ncol)
    nbins = st.nlayer if nbins is None else nbins
    vals = {n: layer_values(st, n) for n in names}
    if axis == "layer":
        res = {}
        for n in names:
            per_bin = []
            for b in range(nbins):
                k = np.full(st.ncol, b + 1) if origin == "top" else na - b        # 1-based layer of bin b
                sel = ok & (k >= 1) & (k <= na)
                per_bin.append(vals[n][k[sel] - 1, cols[sel]])
            res[n] = _stats(per_bin)
        return res
    assert axis == "depth" and dz is not None
    thick = st.arr("thick")
    e = z0 + np.arange(nbins + 1, dtype=np.float64) * dz
    e0, e1 = e[:-1, None], e[1:, None]
    H = column_thickness(st)
    L = np.zeros((nbins, st.ncol))
    W = {n: np.zeros((nbins, st.ncol)) for n in names}
    Z = np.zeros(st.ncol)
    for k in range(1, int(na[ok].max()) + 1 if ok.any() else 1):
        act = ok & (k <= na)
        Zn = np.where(k <= na, Z + thick[k - 1], Z)
        lo, hi = (Z, Zn) if origin == "top" else (H - Zn, H - Z)
        o = np.maximum(0.0, np.minimum(hi[None, :], e1) - np.maximum(lo[None, :], e0))
        o = np.where(act[None, :], o, 0.0)
        L += o
        for n in names:
            W[n] += np.where(act[None, :], o * vals[n][k - 1][None, :], 0.0)
        Z = Zn
    res = {}
    for n in names:
        per_bin = []
        for b in range(nbins):
            sel = ok & (L[b] > 0.0)
            per_bin.append(W[n][b, sel] / L[b, sel])
        res[n] = _stats(per_bin)
    return res
