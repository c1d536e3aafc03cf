"""TEST INFRASTRUCTURE: plain numpy restatement of the column functionals (samsim_set_functionals, include/samsim.h) on a host
State: the layer value as samsim_get_state returns it, the depth coordinate by sequential additions, and every kind's sequence of
IEEE operations in ascending k, vectorised over the columns (numpy rounds every elementwise operation on its own: no fused
multiply-add, and never np.sum).  The oracle of tests/test_gpu_functionals.py."""
import numpy as np

from samsim_amd.capi import A, FN, PROFILE_ORIGINS

TOP = PROFILE_ORIGINS["top"]


def layer_values(spec, st, status=None, uploaded=False, stepped=True):
    """a_k [nlayer, ncol] of the spec's array as samsim_get_state returns it.  With a State that came from get_state() the rule is
    the identity; with the State that was uploaded it restates that function: once the handle has stepped (`stepped`), in a column
    with status 0, S_abs is clamped at 0 unless the column was uploaded since the last step (`uploaded`: a bool or a bool [ncol]),
    and S_bu is S_abs / m where m != 0"""
    ncol = st.ncol
    status = np.zeros(ncol, dtype=np.int32) if status is None else np.asarray(status)
    adjust = (status == 0) & bool(stepped)
    clamp = adjust & ~np.broadcast_to(np.asarray(uploaded, dtype=bool), (ncol,))
    if spec.array not in (A["S_abs"], A["S_bu"]):
        return st.lay[spec.array]
    s_abs = np.where(clamp[None, :] & (st.lay[A["S_abs"]] < 0.0), 0.0, st.lay[A["S_abs"]])
    if spec.array == A["S_abs"]:
        return s_abs
    m = st.lay[A["m"]]
    quot = adjust[None, :] & (m != 0.0)
    with np.errstate(all="ignore"):
        return np.where(quot, s_abs / np.where(quot, m, 1.0), st.lay[A["S_bu"]])


def evaluate(spec, st, status=None, uploaded=False, stepped=True):
    """float64 [ncol]: the value of one FunctionalSpec in every column"""
    ncol, N = st.ncol, st.nlayer
    na = np.clip(st.n_active.astype(np.int64), 0, N)
    a_all = layer_values(spec, st, status, uploaded, stepped)
    thick = st.lay[A["thick"]]
    kmax = int(na.max()) if ncol else 0
    H = np.zeros(ncol)
    for k in range(1, kmax + 1):                          # Z_k = Z_{k-1} + thick(k), k ascending
        H = np.where(k <= na, H + thick[k - 1], H)
    top = spec.origin == TOP
    z_lo, z_hi, thr = np.float64(spec.z_lo), np.float64(spec.z_hi), np.float64(spec.threshold)
    kind = spec.kind
    Z = np.zeros(ncol)
    r0, r1, found = np.zeros(ncol), np.zeros(ncol), np.zeros(ncol, dtype=bool)
    with np.errstate(all="ignore"):
        for k in range(1, kmax + 1):
            have = k <= na
            Zn = Z + thick[k - 1]
            lo, hi = (Z, Zn) if top else (H - Zn, H - Z)
            e1 = np.where(hi < z_hi, hi, z_hi)
            e0 = np.where(lo > z_lo, lo, z_lo)
            o = e1 - e0
            inw = have & (o > 0.0)
            a = a_all[k - 1]
            cond = (a >= thr) if spec.sense > 0 else (a < thr) if spec.sense < 0 else np.zeros(ncol, dtype=bool)
            if kind in (FN["integral"], FN["mean"]):
                r0 = np.where(inw, r0 + o * a, r0)
                r1 = np.where(inw, r1 + o, r1)
                found = found | inw
            elif kind in (FN["min"], FN["depth_of_min"], FN["max"], FN["depth_of_max"]):
                better = (a < r0) if kind in (FN["min"], FN["depth_of_min"]) else (a > r0)
                take = inw & np.where(found, better, a == a)
                r0 = np.where(take, a, r0)
                r1 = np.where(take, 0.5 * (lo + hi), r1)
                found = found | take
            elif kind == FN["crossing_depth"]:
                take = inw & cond & ~(found & top)      # from the top the first is kept, from the bottom the last
                r1 = np.where(take, e0, r1)
                found = found | take
            else:
                assert kind == FN["thickness_where"]
                r0 = np.where(inw & cond, r0 + o, r0)
            Z = np.where(have, Zn, Z)
        missing = np.float64(spec.missing)
        if kind in (FN["integral"], FN["thickness_where"]):
            return r0
        if kind == FN["mean"]:
            return np.where(found, r0 / np.where(found, r1, 1.0), missing)
        if kind in (FN["min"], FN["max"]):
            return np.where(found, r0, missing)
        return np.where(found, r1, missing)


def evaluate_all(specs, st, status=None, uploaded=False, stepped=True):
    return [evaluate(s, st, status, uploaded, stepped) for s in specs]


def same_bytes(got, want):
    """compared as uint64, so that -0.0 and NaNs compare"""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    return got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64))
