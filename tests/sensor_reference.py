"""TEST INFRASTRUCTURE: plain numpy restatement of the sensors and the per-column misfit (samsim_set_sensors, samsim_score,
include/samsim.h) on a host State: the layer value as samsim_get_state returns it, the depth coordinate by sequential additions,
the containing layer, the interpolation between layer midpoints and the score update as the header's sequence of IEEE operations,
vectorised over the columns (numpy rounds every elementwise operation on its own: no fused multiply-add, and never np.sum).  The
oracle of tests/test_gpu_sensors.py."""
from types import SimpleNamespace

import numpy as np

from samsim_amd.capi import A, NSF, PROFILE_ORIGINS, SCORE_FIELDS, SENSOR_INTERPS, SF, SK
from tests.functional_reference import layer_values, same_bytes  # noqa: F401  (same_bytes is re-exported)

TOP = PROFILE_ORIGINS["top"]


def evaluate(spec, st, status=None, uploaded=False, stepped=True, info=None):
    """(y, in_ice): float64 [ncol] the value of one SensorSpec in every column, bool [ncol] whether the sensor is in the ice there.
    info: a dict that receives `extrapolated` (LINEAR without a neighbour on the side of z) and `zero_neighbour` (LINEAR with a
    neighbour of zero thickness), bool [ncol]"""
    ncol, N = st.ncol, st.nlayer
    na = np.clip(st.n_active.astype(np.int64), 0, N)
    thick = st.lay[A["thick"]]
    kmax = int(na.max()) if ncol else 0
    H = np.zeros(ncol)
    for k in range(1, kmax + 1):                          # Z_k = Z_{k-1} + thick(k), k ascending
        H = np.where(k <= na, H + thick[k - 1], H)
    extrapolated, zero_neighbour = np.zeros(ncol, dtype=bool), np.zeros(ncol, dtype=bool)
    if info is not None:
        info.update(extrapolated=extrapolated, zero_neighbour=zero_neighbour)
    if spec.kind == SK["scalar"]:
        return st.scal[spec.id].copy(), np.ones(ncol, dtype=bool)
    if spec.kind == SK["ice_thickness"]:
        return H, np.ones(ncol, dtype=bool)
    assert spec.kind == SK["profile"]
    a_all = layer_values(SimpleNamespace(array=spec.id), st, status, uploaded, stepped)
    top, linear = spec.origin == TOP, spec.interp == SENSOR_INTERPS["linear"]
    z = np.float64(spec.z)
    # lo, hi and the midpoint of every layer, k ascending
    lo, hi, mid = np.zeros((kmax + 2, ncol)), np.zeros((kmax + 2, ncol)), np.zeros((kmax + 2, ncol))
    Z = np.zeros(ncol)
    with np.errstate(all="ignore"):
        for k in range(1, kmax + 1):
            Zn = Z + thick[k - 1]
            lo[k], hi[k] = (Z, Zn) if top else (H - Zn, H - Z)
            mid[k] = 0.5 * (lo[k] + hi[k])
            Z = np.where(k <= na, Zn, Z)
        y = np.full(ncol, np.float64(spec.missing))
        found = np.zeros(ncol, dtype=bool)
        for k in range(1, kmax + 1):
            take = (k <= na) & ~found & (lo[k] <= z) & (z < hi[k])   # the smallest such k
            found |= take
            ak = a_all[k - 1]
            if not linear:
                y = np.where(take, ak, y)
                continue
            up = z >= mid[k]                              # the neighbour has the larger coordinate
            nxt = up if top else ~up                      # ... and is layer k + 1; else layer k - 1
            for j, side in ((k + 1, nxt), (k - 1, ~nxt)):
                sel = take & side
                if not sel.any():
                    continue
                inside = (j >= 1) & (j <= na)
                extrapolated |= sel & ~inside
                if j < 1 or j > kmax:
                    y = np.where(sel, ak, y)
                    continue
                aj = a_all[j - 1]
                zero_neighbour |= sel & inside & (lo[j] == hi[j])
                # (c_a, a_a): the smaller coordinate -- from the top the smaller index, from the bottom the larger
                k_is_a = (k < j) == top
                ca, aa, cb, ab = (mid[k], ak, mid[j], aj) if k_is_a else (mid[j], aj, mid[k], ak)
                t = (z - ca) / (cb - ca)
                prod = t * (ab - aa)
                y = np.where(sel, np.where(inside, aa + prod, ak), y)
    return y, found


def evaluate_all(specs, st, status=None, uploaded=False, stepped=True):
    """(y [n, ncol], in_ice [n, ncol])"""
    out = [evaluate(s, st, status, uploaded, stepped) for s in specs]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def zero_rows(ncol):
    return {f: np.zeros(ncol) for f in SCORE_FIELDS}


def score_update(rows, y, in_ice, obs, weight=None, scored=None):
    """one samsim_score on the nine rows {field: float64 [ncol]} (a new dict; the argument is left alone): y, in_ice [n, ncol] as
    evaluate_all gives them, obs [n], weight [n] or None, scored bool [ncol] (status 0, and the label where a group is given)"""
    n, ncol = y.shape
    obs = np.asarray(obs, dtype=np.float64)
    w = np.ones(n) if weight is None else np.asarray(weight, dtype=np.float64)
    scored = np.ones(ncol, dtype=bool) if scored is None else np.asarray(scored, dtype=bool)
    N, J, B, W = np.zeros(ncol), np.zeros(ncol), np.zeros(ncol), np.zeros(ncol)
    with np.errstate(all="ignore"):
        for i in range(n):                                # ascending i
            if np.isnan(obs[i]):
                continue
            valid = in_ice[i]
            d = y[i] - obs[i]
            dd = d * d
            N = np.where(valid, N + 1.0, N)
            J = np.where(valid, J + w[i] * dd, J)
            B = np.where(valid, B + w[i] * d, B)
            W = np.where(valid, W + w[i], W)
        out = {f: r.copy() for f, r in rows.items()}
        for f, v in (("N_LAST", N), ("J_LAST", J), ("B_LAST", B), ("W_LAST", W)):
            out[f] = np.where(scored, v, out[f])
        add = scored & (N > 0.0)
        for f, v in (("N_SUM", N), ("J_SUM", J), ("B_SUM", B), ("W_SUM", W), ("CALLS", np.ones(ncol))):
            out[f] = np.where(add, out[f] + v, out[f])
    assert len(out) == NSF and list(out) == SCORE_FIELDS and SF["CALLS"] == NSF - 1
    return out
