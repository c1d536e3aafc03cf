"""numpy restatement of samsim_select_columns (include/samsim.h): the mask over the columns from get_state(), get_status(), the
labels and -- for track slots -- tracks(), and the matching indices np.nonzero(mask)[0]."""
import numpy as np

from samsim_amd import capi

TRACK_SLOT0 = capi.track_slot(0, 0)


def slot_values(slot, state, tracks=None):
    """float64 [ncol]: the value x of a slot -- a name from SCALARS, "N_active", or an int (an enum samsim_scalar, -1, or a
    track_slot; tracks: {track: {field: row}} as Solver.tracks returns them)"""
    slot = capi._slot(slot)
    if slot == -1:
        return state.n_active.astype(np.float64)
    if slot < capi.NSCAL:
        return state.scal[slot]
    o = slot - TRACK_SLOT0
    return tracks[o // 32][capi.TRACK_FIELDS[o % 32]]


def select_mask(state, status, terms=(), group=None, labels=None, mode="running", tracks=None):
    """bool [ncol].  terms: (slot, lo, hi), a term holds when lo <= x and x < hi (two IEEE comparisons: a NaN x satisfies none);
    mode "running" (status == 0), "stopped" (status != 0), "any", or an integer code (status == code); group: None or -1 any
    column, else only the columns with that label"""
    status = np.asarray(status)
    if mode == "running":
        mask = status == 0
    elif mode == "stopped":
        mask = status != 0
    elif mode == "any":
        mask = np.ones(status.shape, dtype=bool)
    else:
        mask = status == int(mode)
    if group is not None and group >= 0:
        mask = mask & (np.asarray(labels) == group)
    for slot, lo, hi in terms:
        x = slot_values(slot, state, tracks)
        with np.errstate(invalid="ignore"):
            mask = mask & (np.float64(lo) <= x) & (x < np.float64(hi))
    return mask


def select_reference(state, status, terms=(), group=None, labels=None, mode="running", tracks=None, max_out=None):
    """(int64 indices, n_match): np.nonzero(mask)[0][:max_out] and the exact number of matches"""
    idx = np.nonzero(select_mask(state, status, terms, group, labels, mode, tracks))[0].astype(np.int64)
    return (idx if max_out is None else idx[:max_out]), int(idx.size)
