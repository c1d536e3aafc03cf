"""TEST INFRASTRUCTURE: plain numpy restatement of the time-domain diagnostics (samsim_set_tracks, include/samsim.h): the
observable of every kind from a host State as get_state() returns it, and the update rule of the eleven fields -- the header's
sequence of IEEE operations, vectorised over the columns (numpy rounds every elementwise operation on its own: no fused
multiply-add) -- applied to a list of (step, State, status) taken at the sample points."""
import numpy as np

from samsim_amd.capi import OBS, TRACK_FIELDS, TRACK_INITIAL


def initial(ncol):
    """the rows of one track before the first sample"""
    return {f: np.full(ncol, TRACK_INITIAL[f], dtype=np.float64) for f in TRACK_FIELDS}


def observable(spec, st):
    """(x [ncol], exists [ncol]): the observable of a TrackSpec in every column of a State, and whether the column has it (a LAYER
    track: whether the column has the layer)"""
    na = st.n_active.astype(np.int64)
    ncol = st.ncol
    every = np.ones(ncol, dtype=bool)
    if spec.kind == OBS["scalar"]:
        return st.scal[spec.id].copy(), every
    if spec.kind == OBS["n_active"]:
        return st.n_active.astype(np.float64), every
    if spec.kind == OBS["ice_thickness"]:
        thick, Z = st.lay[3], np.zeros(ncol)
        for k in range(1, int(na.max()) + 1):                 # Z_k = Z_{k-1} + thick(k), k ascending
            Z = np.where(k <= na, Z + thick[k - 1], Z)
        return Z, every
    if spec.kind == OBS["bulk_salinity"]:
        s_abs, m, ssum, msum = st.lay[1], st.lay[2], np.zeros(ncol), np.zeros(ncol)
        for k in range(1, int(na.max()) + 1):
            ssum = np.where(k <= na, ssum + s_abs[k - 1], ssum)
            msum = np.where(k <= na, msum + m[k - 1], msum)
        with np.errstate(all="ignore"):
            return ssum / msum, every
    assert spec.kind == OBS["layer"]
    k = np.full(ncol, spec.layer, dtype=np.int64) if spec.layer > 0 else na + 1 + spec.layer
    exists = (k >= 1) & (k <= na)
    x = st.lay[spec.id][np.where(exists, k - 1, 0), np.arange(ncol)]
    return np.where(exists, x, 0.0), exists


def update(fields, spec, x, sampled, s):
    """one sample with the values x at time s in the columns `sampled`; the other columns keep every field"""
    f = fields
    s = np.float64(s)
    with np.errstate(all="ignore"):
        n = f["N"] + 1.0
        d = x - f["MEAN"]
        mean = f["MEAN"] + d / n
        m2 = f["M2"] + d * (x - mean)
        lower, higher = sampled & (x < f["MIN"]), sampled & (x > f["MAX"])
        hold = sampled & ((x >= spec.threshold) if spec.sense > 0 else (x < spec.threshold) if spec.sense < 0 else np.zeros_like(sampled))
    f["N"] = np.where(sampled, n, f["N"])
    f["LAST"] = np.where(sampled, x, f["LAST"])
    f["MEAN"] = np.where(sampled, mean, f["MEAN"])
    f["M2"] = np.where(sampled, m2, f["M2"])
    f["MIN"], f["STEP_MIN"] = np.where(lower, x, f["MIN"]), np.where(lower, s, f["STEP_MIN"])
    f["MAX"], f["STEP_MAX"] = np.where(higher, x, f["MAX"]), np.where(higher, s, f["STEP_MAX"])
    f["N_HOLD"] = np.where(hold, f["N_HOLD"] + 1.0, f["N_HOLD"])
    f["STEP_FIRST"] = np.where(hold & (f["STEP_FIRST"] < 0.0), s, f["STEP_FIRST"])
    f["STEP_LAST"] = np.where(hold, s, f["STEP_LAST"])


def apply(specs, samples, start=None):
    """the rows of every track -- a list of {field: [ncol]} -- after the samples [(step, State, status), ...], from the initial
    values or from `start`"""
    samples = list(samples)
    ncol = samples[0][1].ncol if samples else start[0]["N"].size
    rows = [initial(ncol) for _ in specs] if start is None else [{k: v.copy() for k, v in r.items()} for r in start]
    for step, st, status in samples:
        alive = np.asarray(status) == 0
        for spec, fields in zip(specs, rows):
            x, exists = observable(spec, st)
            update(fields, spec, x, alive & exists, step)
    return rows


def same_bytes(got, want):
    """the fields in which two sets of rows differ, [(track, field), ...]: bytes, so that -0.0 and the payload of a NaN count"""
    assert len(got) == len(want)
    return [(t, f) for t in range(len(want)) for f in TRACK_FIELDS if got[t][f].tobytes() != want[t][f].tobytes()]
