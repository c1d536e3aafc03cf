"""ctypes view of the C-ABI declared in include/samsim.h.

The struct layouts and call signatures are those of the product library
(``samsim_amd/csrc/libsamsim_hip.so``, symbol prefix ``samsim_``).  ``Solver`` is parameterised by the library
object and the symbol prefix so that the test-suite can drive a checker library that exports the same interface
under another prefix; this module itself only ever describes the interface (``samsim_amd.load()`` loads the HIP
library and fails loudly when it is missing -- there is no CPU fallback).
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

ABI_VERSION = 6

_CFG_INT_FIELDS = [
    "struct_size", "testcase", "nlayer", "n_top", "n_middle", "n_bottom",
    "atmoflux_flag", "grav_flag", "prescribe_flag", "grav_heat_flag", "flush_heat_flag", "turb_flag",
    "salt_flag", "boundflux_flag", "flush_flag", "flood_flag", "bottom_flag", "debug_flag", "precip_flag",
    "harmonic_flag", "tank_flag", "albedo_flag", "lab_snow_flag", "freeboard_snow_flag", "snow_flush_flag",
    "snow_precip_flag", "bgc_flag", "i_time_out",
]
_CFG_DBL_FIELDS = [
    "dt", "thick_0", "thick_min", "T_bottom", "S_bu_bottom", "k_snow_flush", "max_flux_plate", "time_out",
    "time_total", "alpha_flux_instable", "alpha_flux_stable", "m_total", "S_total",
]


class Config(C.Structure):
    """samsim_config (include/samsim.h); flags of mo_data.f90:136-155."""
    _fields_ = [(n, C.c_int32) for n in _CFG_INT_FIELDS] + [(n, C.c_double) for n in _CFG_DBL_FIELDS]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class StateSoA(C.Structure):
    _fields_ = [("ncol", C.c_int64), ("nlayer", C.c_int32), ("narr", C.c_int32),
                ("lay", C.POINTER(C.c_double)), ("scal", C.POINTER(C.c_double)),
                ("n_active", C.POINTER(C.c_int32))]


class Clock(C.Structure):
    _fields_ = [("time", C.c_double), ("step", C.c_int64), ("n_time_out", C.c_int32),
                ("time_counter", C.c_int32), ("n_outputs", C.c_int64)]


class Stat(C.Structure):
    """samsim_stat"""
    _fields_ = [("count", C.c_int64), ("mean", C.c_double), ("min", C.c_double), ("max", C.c_double), ("std", C.c_double)]


PROFILE_MAX_BINS = 1024
PROFILE_MAX_ARRAYS = 8
PROFILE_AXES = {"layer": 0, "depth": 1}
PROFILE_ORIGINS = {"top": 0, "bottom": 1}
MAX_GROUPS = 1024           # SAMSIM_MAX_GROUPS


class ProfileRequest(C.Structure):
    """samsim_profile_request"""
    _fields_ = [("struct_size", C.c_int32), ("axis", C.c_int32), ("origin", C.c_int32), ("nbins", C.c_int32),
                ("narrays", C.c_int32), ("arrays", C.c_int32 * PROFILE_MAX_ARRAYS), ("z0", C.c_double), ("dz", C.c_double)]


HIST_MAX_VBINS = 254        # SAMSIM_HIST_MAX_VBINS


class HistBins(C.Structure):
    """samsim_hist_bins: edges E_j = v0 + j*dv, j = 0..nvbins"""
    _fields_ = [("struct_size", C.c_int32), ("nvbins", C.c_int32), ("v0", C.c_double), ("dv", C.c_double)]


def hist_bins(nvbins, v0, dv) -> "HistBins":
    return HistBins(C.sizeof(HistBins), int(nvbins), float(v0), float(dv))


def hist_edges(nvbins, v0, dv) -> np.ndarray:
    """the nvbins + 1 edges as the library forms them: the product is rounded, then the sum"""
    return np.float64(v0) + np.arange(int(nvbins) + 1, dtype=np.float64) * np.float64(dv)


def quantile_bracket(counts, v0, dv, q):
    """(lo, hi) with the r-th smallest value of the data in [lo, hi), from one row of counts of Solver.histogram /
    Solver.profile_histogram (nvbins + 2 entries): n = sum of the row, rank r = max(1, ceil(q n)), i = the first entry whose
    cumulative count reaches r, lo = E_{i-1} and hi = E_i, with -inf and +inf for the two outer entries"""
    counts = np.asarray(counts, dtype=np.int64)
    if counts.ndim != 1 or counts.size < 3:
        raise ValueError("one row of nvbins + 2 counts is needed")
    n = int(counts.sum())
    if n == 0:
        raise ValueError("an empty row has no quantiles")
    if not 0.0 <= q <= 1.0:
        raise ValueError("q outside [0, 1]")
    r = max(1, int(np.ceil(q * n)))
    i = int(np.searchsorted(np.cumsum(counts), r, side="left"))
    e = hist_edges(counts.size - 2, v0, dv)
    return (-np.inf if i == 0 else float(e[i - 1])), (np.inf if i == counts.size - 1 else float(e[i]))


SENS_MAX_SLOTS = 8          # SAMSIM_SENS_MAX_SLOTS


class PairStat(C.Structure):
    """samsim_pair_stat: joint population moments of a predictor x and a bin value y over the contributing columns"""
    _fields_ = [("count", C.c_int64), ("mean_x", C.c_double), ("mean_y", C.c_double), ("var_x", C.c_double), ("var_y", C.c_double),
                ("cov", C.c_double)]


PAIR_STAT_DTYPE = np.dtype([("count", np.int64), ("mean_x", np.float64), ("mean_y", np.float64), ("var_x", np.float64),
                            ("var_y", np.float64), ("cov", np.float64)])


def correlation(cov) -> np.ndarray:
    """the correlation matrix of a covariance matrix (Solver.covariance): cov[i][j] / sqrt(cov[i][i] cov[j][j]), 0.0 where a
    variance is 0"""
    cov = np.asarray(cov, dtype=np.float64)
    if cov.ndim != 2 or cov.shape[0] != cov.shape[1]:
        raise ValueError("a square covariance matrix is needed")
    var = np.diag(cov)
    scale = np.sqrt(var[:, None] * var[None, :])
    ok = scale > 0.0
    return np.where(ok, cov / np.where(ok, scale, 1.0), 0.0)


def slope_and_correlation(pair_stats):
    """(slope, correlation) of y on x from an array of PAIR_STAT_DTYPE (Solver.profile_regression): cov / var_x and
    cov / sqrt(var_x var_y), each 0.0 where a variance it divides by is 0"""
    q = np.asarray(pair_stats)
    vx, vy, c = q["var_x"], q["var_y"], q["cov"]
    okx = vx > 0.0
    slope = np.where(okx, c / np.where(okx, vx, 1.0), 0.0)
    scale = np.sqrt(vx * vy)
    ok = scale > 0.0
    return slope, np.where(ok, c / np.where(ok, scale, 1.0), 0.0)


MAX_TRACKS = 8              # SAMSIM_MAX_TRACKS
# enum samsim_observable_kind
OBSERVABLES = ["scalar", "n_active", "ice_thickness", "bulk_salinity", "layer"]
OBS = {n: i for i, n in enumerate(OBSERVABLES)}
# enum samsim_track_field: one double[ncol] row per track and field
TRACK_FIELDS = ["N", "LAST", "MEAN", "M2", "MIN", "STEP_MIN", "MAX", "STEP_MAX", "N_HOLD", "STEP_FIRST", "STEP_LAST"]
TF = {n: i for i, n in enumerate(TRACK_FIELDS)}
NTF = len(TRACK_FIELDS)
TRACK_INITIAL = {"N": 0.0, "LAST": 0.0, "MEAN": 0.0, "M2": 0.0, "MIN": np.inf, "STEP_MIN": -1.0, "MAX": -np.inf, "STEP_MAX": -1.0,
                 "N_HOLD": 0.0, "STEP_FIRST": -1.0, "STEP_LAST": -1.0}


class TrackSpec(C.Structure):
    """samsim_track_spec: one observable followed through the run, with an optional condition x >= threshold (sense +1) or
    x < threshold (sense -1)"""
    _fields_ = [("struct_size", C.c_int32), ("kind", C.c_int32), ("id", C.c_int32), ("layer", C.c_int32), ("sense", C.c_int32),
                ("reserved", C.c_int32), ("threshold", C.c_double)]

    @staticmethod
    def make(kind, name=None, layer=0, sense=0, threshold=0.0) -> "TrackSpec":
        """kind from OBSERVABLES; name from SCALARS ("scalar") or ARRAYS ("layer"); layer k >= 1 from the top, k <= -1 from the
        bottom ("layer" only)"""
        ident = S[name] if kind == "scalar" else A[name] if kind == "layer" else 0
        return TrackSpec(C.sizeof(TrackSpec), OBS[kind], ident, int(layer), int(sense), 0, float(threshold))


def track_slot(track, field) -> int:
    """SAMSIM_TRACK_SLOT(track, field): the row of a track as a slot of ensemble_stats, group_stats, histogram, covariance and
    profile_regression; field a name from TRACK_FIELDS or its number"""
    return 0x10000 + int(track) * 32 + (TF[field] if isinstance(field, str) else int(field))


MAX_FUNCTIONALS = 8         # SAMSIM_MAX_FUNCTIONALS
# enum samsim_functional_kind
FUNCTIONAL_KINDS = ["integral", "mean", "min", "max", "depth_of_min", "depth_of_max", "crossing_depth", "thickness_where"]
FN = {n: i for i, n in enumerate(FUNCTIONAL_KINDS)}


class FunctionalSpec(C.Structure):
    """samsim_functional_spec: one functional of a column's layer profile over the depth window [z_lo, z_hi), with the condition
    a_k >= threshold (sense +1) or a_k < threshold (sense -1) for "crossing_depth" and "thickness_where" """
    _fields_ = [("struct_size", C.c_int32), ("kind", C.c_int32), ("array", C.c_int32), ("origin", C.c_int32), ("sense", C.c_int32),
                ("reserved", C.c_int32), ("z_lo", C.c_double), ("z_hi", C.c_double), ("threshold", C.c_double), ("missing", C.c_double)]

    @staticmethod
    def make(kind, array, origin="top", z_lo=0.0, z_hi=np.inf, sense=0, threshold=0.0, missing=np.nan) -> "FunctionalSpec":
        """kind from FUNCTIONAL_KINDS, array from ARRAYS, origin from PROFILE_ORIGINS (names or their numbers)"""
        k = FN[kind] if isinstance(kind, str) else int(kind)
        a = A[array] if isinstance(array, str) else int(array)
        o = PROFILE_ORIGINS[origin] if isinstance(origin, str) else int(origin)
        return FunctionalSpec(C.sizeof(FunctionalSpec), k, a, o, int(sense), 0, float(z_lo), float(z_hi), float(threshold), float(missing))


def func_slot(i) -> int:
    """SAMSIM_FUNC_SLOT(i): the row of functional i as a slot of ensemble_stats, group_stats, histogram, covariance,
    profile_regression and select"""
    return 0x20000 + int(i)


MAX_SENSORS = 32            # SAMSIM_MAX_SENSORS
# enum samsim_sensor_kind, enum samsim_sensor_interp, enum samsim_score_field
SENSOR_KINDS = ["profile", "scalar", "ice_thickness"]
SK = {n: i for i, n in enumerate(SENSOR_KINDS)}
SENSOR_INTERPS = {"step": 0, "linear": 1}
SCORE_FIELDS = ["N_LAST", "J_LAST", "B_LAST", "W_LAST", "N_SUM", "J_SUM", "B_SUM", "W_SUM", "CALLS"]
SF = {n: i for i, n in enumerate(SCORE_FIELDS)}
NSF = len(SCORE_FIELDS)


class SensorSpec(C.Structure):
    """samsim_sensor_spec: the model's equivalent of one sensor, per column: a layer array at depth z from `origin` ("profile", by
    "step" or "linear" between layer midpoints), a stored column scalar ("scalar"), or the current ice thickness ("ice_thickness");
    `missing` is the value of a profile sensor that is not in the ice"""
    _fields_ = [("struct_size", C.c_int32), ("kind", C.c_int32), ("id", C.c_int32), ("origin", C.c_int32), ("interp", C.c_int32),
                ("reserved", C.c_int32), ("z", C.c_double), ("missing", C.c_double)]

    @staticmethod
    def make(kind, name=None, z=0.0, origin="top", interp="step", missing=np.nan) -> "SensorSpec":
        """kind from SENSOR_KINDS; name from ARRAYS ("profile") or SCALARS ("scalar"), or its number; origin from PROFILE_ORIGINS,
        interp from SENSOR_INTERPS (names or their numbers)"""
        k = SK[kind] if isinstance(kind, str) else int(kind)
        if name is None:
            i = 0
        elif isinstance(name, str):
            i = S[name] if k == SK["scalar"] else A[name]
        else:
            i = int(name)
        o = PROFILE_ORIGINS[origin] if isinstance(origin, str) else int(origin)
        p = SENSOR_INTERPS[interp] if isinstance(interp, str) else int(interp)
        return SensorSpec(C.sizeof(SensorSpec), k, i, o, p, 0, float(z), float(missing))


def score_slot(field) -> int:
    """SAMSIM_SCORE_SLOT(field): a row of the per-column misfit (field from SCORE_FIELDS or its number) as a slot of ensemble_stats,
    group_stats, histogram, covariance, profile_regression and select, while sensors are set"""
    return 0x30000 + (SF[field] if isinstance(field, str) else int(field))


# enum samsim_weight_kind
WEIGHT_KINDS = {"direct": 0, "gauss": 1}


class WeightSpec(C.Structure):
    """samsim_weight_spec: how the weight row is formed from the slot's value x of the columns that are IN (status 0, label `group` or
    -1 for any): "direct" w = x where 0 < x < inf, "gauss" w = exp(-(x - x_min) * (0.5 / scale))"""
    _fields_ = [("struct_size", C.c_int32), ("kind", C.c_int32), ("slot", C.c_int32), ("group", C.c_int32), ("scale", C.c_double),
                ("reserved", C.c_double)]

    @staticmethod
    def make(slot, kind="gauss", scale=1.0, group=None) -> "WeightSpec":
        """slot a name from SCALARS, "N_active", or an int of track_slot, func_slot or score_slot; kind from WEIGHT_KINDS or its
        number; scale belongs to "gauss" ("direct" takes none: its field is 0)"""
        k = WEIGHT_KINDS[kind] if isinstance(kind, str) else int(kind)
        return WeightSpec(C.sizeof(WeightSpec), k, _slot(slot), -1 if group is None else int(group),
                          float(scale) if k == WEIGHT_KINDS["gauss"] else 0.0, 0.0)


class WeightInfo(C.Structure):
    """samsim_weight_info"""
    _fields_ = [("n_in", C.c_int64), ("n_pos", C.c_int64), ("x_min", C.c_double), ("sum_w", C.c_double), ("sum_w2", C.c_double)]


WSTAT_DTYPE = np.dtype([("count", np.int64), ("sum_w", np.float64), ("sum_w2", np.float64), ("mean", np.float64), ("var", np.float64),
                        ("min", np.float64), ("max", np.float64)])


def weight_slot() -> int:
    """SAMSIM_WEIGHT_SLOT: the weight row of set_weights as a slot of ensemble_stats, group_stats, histogram, covariance,
    profile_regression and select, while the row exists"""
    return 0x40000


# enum samsim_resample_kind
RESAMPLE_KINDS = {"systematic": 0, "stratified": 1}
RESAMPLE_MAX_DRAWS = 4194304    # SAMSIM_RESAMPLE_MAX_DRAWS


class ResampleSpec(C.Structure):
    """samsim_resample_spec: m draws over the columns that count (status 0, label `group` or -1 for any, w > 0), "systematic" with
    the offset u0 in [0, 1) or "stratified" with the seed of the per-draw offsets"""
    _fields_ = [("struct_size", C.c_int32), ("kind", C.c_int32), ("group", C.c_int32), ("reserved", C.c_int32), ("m", C.c_int64),
                ("u0", C.c_double), ("seed", C.c_uint64)]

    @staticmethod
    def make(m, kind="systematic", u0=0.0, seed=0, group=None) -> "ResampleSpec":
        """kind from RESAMPLE_KINDS or its number; u0 belongs to "systematic", seed to "stratified" (the other's field is 0)"""
        k = RESAMPLE_KINDS[kind] if isinstance(kind, str) else int(kind)
        return ResampleSpec(C.sizeof(ResampleSpec), k, -1 if group is None else int(group), 0, int(m), float(u0), int(seed))


class ResampleInfo(C.Structure):
    """samsim_resample_info"""
    _fields_ = [("n_pos", C.c_int64), ("m_drawn", C.c_int64), ("n_survivors", C.c_int64), ("max_offspring", C.c_int64),
                ("argmax_offspring", C.c_int64), ("sum_w", C.c_double)]


# what samsim_copy_columns and samsim_apply_resample copy beside the state (SAMSIM_COPY_*)
COPY_FORCING, COPY_TRACKS, COPY_SCORES = 1, 2, 4
COPY_SCRATCH_BYTES = 64 << 10   # SAMSIM_COPY_SCRATCH_BYTES


class ApplyInfo(C.Structure):
    """struct samsim_apply_info"""
    _fields_ = [("n_pool", C.c_int64), ("n_free", C.c_int64), ("n_copies", C.c_int64), ("n_sources", C.c_int64)]


def copy_what(forcing=False, tracks=False, scores=False) -> int:
    """the `what` of samsim_copy_columns and samsim_apply_resample"""
    return (COPY_FORCING if forcing else 0) | (COPY_TRACKS if tracks else 0) | (COPY_SCORES if scores else 0)


def offspring_slot() -> int:
    """SAMSIM_OFFSPRING_SLOT: the offspring row of resample as a slot of ensemble_stats, group_stats, histogram, covariance and
    select, while the row exists"""
    return 0x50000


# the rejuvenation of the resampled ensemble (samsim_jitter)
JITTER_MAX_TERMS = 4                # SAMSIM_JITTER_MAX_TERMS
JITTER_MAX_ATTEMPTS = 32            # SAMSIM_JITTER_MAX_ATTEMPTS
JITTER_SCRATCH_BYTES = 320 << 10    # SAMSIM_JITTER_SCRATCH_BYTES
# enum samsim_jitter_target: the two perturbation slots of the forcing, then the two rows of set_ocean
JITTER_TARGETS = ["dT2m", "precip_scale", "dfl_q_bottom", "S_bu_bottom"]
JT = {n: i for i, n in enumerate(JITTER_TARGETS)}
# enum samsim_jitter_which
JITTER_WHICH = {"pool": 0, "copies": 1}
OCEAN_ROWS = ["dfl_q_bottom", "S_bu_bottom"]


class JitterTerm(C.Structure):
    """samsim_jitter_term: the row `target` becomes centre + shrink * (row - centre) + sigma * eps, kept within [lo, hi]"""
    _fields_ = [("target", C.c_int32), ("reserved", C.c_int32), ("centre", C.c_double), ("shrink", C.c_double), ("sigma", C.c_double),
                ("lo", C.c_double), ("hi", C.c_double)]

    @staticmethod
    def make(target, centre=0.0, shrink=1.0, sigma=0.0, lo=-np.inf, hi=np.inf) -> "JitterTerm":
        """target from JITTER_TARGETS or its number"""
        t = JT[target] if isinstance(target, str) else int(target)
        return JitterTerm(t, 0, float(centre), float(shrink), float(sigma), float(lo), float(hi))


class JitterSpec(C.Structure):
    """samsim_jitter_spec: up to JITTER_MAX_TERMS terms over the pool (status 0, label `group` or -1 for any) or over the copies of the
    last apply_resample, the deviates keyed by (seed, column, target)"""
    _fields_ = [("struct_size", C.c_int32), ("which", C.c_int32), ("group", C.c_int32), ("nterms", C.c_int32), ("seed", C.c_uint64),
                ("term", JitterTerm * JITTER_MAX_TERMS)]

    @staticmethod
    def make(terms, which="pool", seed=0, group=None) -> "JitterSpec":
        """terms JitterTerm's (at most JITTER_MAX_TERMS are stored; nterms is their number as given); which from JITTER_WHICH or its
        number"""
        terms = list(terms)
        w = JITTER_WHICH[which] if isinstance(which, str) else int(which)
        spec = JitterSpec(C.sizeof(JitterSpec), w, -1 if group is None else int(group), len(terms), int(seed) & (2 ** 64 - 1))
        for i, t in enumerate(terms[:JITTER_MAX_TERMS]):
            spec.term[i] = t
        return spec


class JitterInfo(C.Structure):
    """samsim_jitter_info"""
    _fields_ = [("n_written", C.c_int64), ("n_lo", C.c_int64 * JITTER_MAX_TERMS), ("n_hi", C.c_int64 * JITTER_MAX_TERMS)]

    def as_dict(self, nterms=JITTER_MAX_TERMS):
        return {"n_written": int(self.n_written), "n_lo": [int(x) for x in self.n_lo[:nterms]], "n_hi": [int(x) for x in self.n_hi[:nterms]]}


def ocean_slot(name) -> int:
    """SAMSIM_OCEAN_SLOT(i): a row of set_ocean ("dfl_q_bottom" or "S_bu_bottom", or its number) as a slot of ensemble_stats,
    group_stats, histogram, covariance, select and the weighted reductions, while that row exists"""
    return 0x60000 + (OCEAN_ROWS.index(name) if isinstance(name, str) else int(name))


def jitter_slot(target) -> int:
    """the slot that reads the row of a jitter target: the scalar of that name, or ocean_slot"""
    t = JITTER_TARGETS[target] if isinstance(target, (int, np.integer)) else target
    return ocean_slot(t) if t in OCEAN_ROWS else S[t]


def liu_west(delta):
    """(a, h) of Liu and West's kernel shrinkage for the discount factor delta in (0, 1]: a = (3 delta - 1) / (2 delta) the shrinkage
    of each value towards the mean, h = sqrt(1 - a^2) the width of the kernel in standard deviations; mean and variance of the
    ensemble are kept"""
    delta = float(delta)
    if not 1.0 / 3.0 <= delta <= 1.0:
        raise ValueError("delta outside [1/3, 1]")
    a = (3.0 * delta - 1.0) / (2.0 * delta)
    return a, float(np.sqrt(1.0 - a * a))


_M64 = (1 << 64) - 1


def mix64(seed, k) -> int:
    """rs_mix of samsim_resample.h: the splitmix64 finaliser of seed + (k + 1) * 0x9E3779B97F4A7C15 in wrapping 64-bit arithmetic, the
    mixer of the stratified draw and of the jitter's deviates"""
    z = (int(seed) + (int(k) + 1) * 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def rs_offset(seed, k) -> float:
    """rs_offset of samsim_resample.h: the upper 53 bits of mix64(seed, k) as a double in [0, 1)"""
    return float(mix64(seed, k) >> 11) * 2.0 ** -53


def weighted_quantile_bracket(wsum, v0, dv, q):
    """(lo, hi) with the weighted q-quantile of the data in [lo, hi), from the sums of Solver.weighted_histogram (nvbins + 2
    entries): the quantile is the smallest value whose cumulative weight reaches q times the total; i = the first entry of positive
    weight whose cumulative sum reaches that, lo = E_{i-1} and hi = E_i, with -inf and +inf for the two outer entries"""
    wsum = np.asarray(wsum, dtype=np.float64)
    if wsum.ndim != 1 or wsum.size < 3:
        raise ValueError("one row of nvbins + 2 sums is needed")
    if not (wsum >= 0.0).all():
        raise ValueError("a sum of weights is negative or a NaN")
    cum = np.cumsum(wsum)
    if not cum[-1] > 0.0:
        raise ValueError("an empty row has no quantiles")
    if not 0.0 <= q <= 1.0:
        raise ValueError("q outside [0, 1]")
    i = min(int(np.searchsorted(cum, q * cum[-1], side="left")), wsum.size - 1)
    while wsum[i] == 0.0:       # q == 0, or a target met exactly at an entry's end: the next entry that holds weight
        i += 1
    e = hist_edges(wsum.size - 2, v0, dv)
    return (-np.inf if i == 0 else float(e[i - 1])), (np.inf if i == wsum.size - 1 else float(e[i]))


WPHIST_SCRATCH_BYTES = 32 << 20     # SAMSIM_WPHIST_SCRATCH_BYTES
WPHIST_GRID = 512                   # DEV_WPHIST_GRID (samsim_pass_plan.h): the waves of a pass, which decide the merge order
WPHIST_LDS_BYTES = 64 << 10         # DEV_WPHIST_LDS_BYTES


def wphist_chunk(nvbins) -> int:
    """dev_wphist_chunk (samsim_pass_plan.h): the depth bins one pass of Solver.weighted_profile_histogram serves -- the tile rows
    [65] and the table rows [(nvbins + 2) | 1] of doubles that fit 64 KiB of LDS beside the lanes' masks and the block's weights,
    at most 64"""
    per_bin = (65 + ((int(nvbins) + 2) | 1)) * 8
    return min(64, (WPHIST_LDS_BYTES - 1024) // per_bin)


def weighted_profile_quantiles(wsum, v0, dv, qs):
    """(lo, hi), each float64 [len(qs), nbins], from the table [nbins, nvbins + 2] of Solver.weighted_profile_histogram:
    weighted_quantile_bracket of every row for every q of qs, so the weighted q-quantile of depth bin b lies in
    [lo[k, b], hi[k, b]); NaN in both for a row without weight.  qs = (0.05, 0.5, 0.95) gives the posterior median and the 5-95 %
    band of a profile"""
    wsum = np.asarray(wsum, dtype=np.float64)
    if wsum.ndim != 2 or wsum.shape[1] < 3:
        raise ValueError("a table [nbins, nvbins + 2] of sums is needed")
    if not (wsum >= 0.0).all():
        raise ValueError("a sum of weights is negative or a NaN")
    qs = [float(q) for q in qs]
    if not all(0.0 <= q <= 1.0 for q in qs):
        raise ValueError("q outside [0, 1]")
    lo = np.full((len(qs), wsum.shape[0]), np.nan)
    hi = np.full((len(qs), wsum.shape[0]), np.nan)
    for b, row in enumerate(wsum):
        if not (row > 0.0).any():
            continue
        for k, q in enumerate(qs):
            lo[k, b], hi[k, b] = weighted_quantile_bracket(row, v0, dv, q)
    return lo, hi


def weighted_profile_mean(pair_stats) -> np.ndarray:
    """the weighted mean of the bin value y per bin, sum w y / sum w over the bin's contributing columns, from an array of
    PAIR_STAT_DTYPE that Solver.profile_regression returned with predictor=weight_slot(): mean_y + cov / mean_x (cov = mean(w y) -
    mean_w mean_y and mean_x = mean_w over the same columns); 0.0 where mean_x == 0 (no weight in the bin)"""
    q = np.asarray(pair_stats)
    mx = q["mean_x"]
    ok = mx != 0.0
    return np.where(ok, q["mean_y"] + q["cov"] / np.where(ok, mx, 1.0), 0.0)


def _slot(name) -> int:
    """the slot of a name from SCALARS, of "N_active", or of an int as track_slot, func_slot, score_slot, weight_slot or offspring_slot
    gives it"""
    if isinstance(name, (int, np.integer)):
        return int(name)
    return -1 if name == "N_active" else S[name]


SELECT_MAX_TERMS = 4        # SAMSIM_SELECT_MAX_TERMS
SELECT_MAX_OUT = 262144     # SAMSIM_SELECT_MAX_OUT: indices per select, and columns per get_columns
# enum samsim_select_status
SELECT_STATUS = {"running": 0, "stopped": 1, "code": 2, "any": 3}


class SelectTerm(C.Structure):
    """samsim_select_term: holds when lo <= x && x < hi for the column's value x of the slot"""
    _fields_ = [("slot", C.c_int32), ("reserved", C.c_int32), ("lo", C.c_double), ("hi", C.c_double)]


class Selection(C.Structure):
    """samsim_selection: the ANDed terms, the label and the status mode a column must pass"""
    _fields_ = [("struct_size", C.c_int32), ("nterms", C.c_int32), ("group", C.c_int32), ("status_mode", C.c_int32),
                ("code", C.c_int32), ("reserved", C.c_int32), ("terms", SelectTerm * SELECT_MAX_TERMS)]

    @staticmethod
    def make(terms=(), group=None, status="running") -> "Selection":
        """terms: (name_or_slot, lo, hi) with names from SCALARS, "N_active", or ints of track_slot; status "running", "stopped",
        "any" or an integer STOP code"""
        sel = Selection()
        sel.struct_size = C.sizeof(Selection)
        terms = list(terms)
        sel.nterms = len(terms)
        for i, (name, lo, hi) in enumerate(terms[:SELECT_MAX_TERMS]):
            sel.terms[i] = SelectTerm(_slot(name), 0, float(lo), float(hi))
        sel.group = -1 if group is None else int(group)
        if isinstance(status, str):
            sel.status_mode, sel.code = SELECT_STATUS[status], 0
        else:
            sel.status_mode, sel.code = SELECT_STATUS["code"], int(status)
        return sel


STAT_DTYPE = np.dtype([("count", np.int64), ("mean", np.float64), ("min", np.float64), ("max", np.float64), ("std", np.float64)])


class OutputSoA(C.Structure):
    _fields_ = [("ncols", C.c_int64), ("nlayer", C.c_int32), ("reserved", C.c_int32),
                ("lay", C.POINTER(C.c_double)), ("scal", C.POINTER(C.c_double)),
                ("n_active", C.POINTER(C.c_int32)), ("time", C.c_double), ("step", C.c_int64)]


# enum samsim_scalar
SCALARS = [
    "m_snow", "H_abs_snow", "S_abs_snow", "thick_snow", "psi_s_snow", "psi_l_snow", "psi_g_snow", "T_snow",
    "phi_s", "T_top", "melt_thick", "T2m", "liquid_precip", "solid_precip", "fl_q_bottom",
    "grav_drain", "grav_salt", "grav_temp", "melt_out1", "melt_out2", "melt_out3", "melt_err",
    "freeboard", "T_freeze", "albedo", "fl_sw", "fl_lw", "melt_thick_snow", "fl_Q_snow",
    "energy_stored", "freshwater", "total_resist", "thickness", "bulk_salin", "fl_rest", "S_bu_bottom", "dT2m", "precip_scale",
]
S = {n: i for i, n in enumerate(SCALARS)}
NSCAL = len(SCALARS)
# enum samsim_layer_array
ARRAYS = ["H_abs", "S_abs", "m", "thick", "T", "phi", "psi_s", "psi_l", "psi_g", "S_bu", "S_br", "ray", "perm",
          "flush_v", "flush_h"]
A = {n: i for i, n in enumerate(ARRAYS)}
NARR = len(ARRAYS)
NPROG = 4

ERRORS = {0: "ok", -1: "bad argument", -2: "unsupported flag value", -3: "HIP error", -4: "no HIP device",
          -5: "no output snapshot", -6: "ABI mismatch", -7: "out of memory"}


class SamsimError(RuntimeError):
    def __init__(self, code, what):
        super().__init__(f"{what}: error {code} ({ERRORS.get(code, '?')})")
        self.code = code


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


@dataclass
class State:
    """Host copy of the SoA column state: lay[narr, nlayer, ncol], scal[NSCAL, ncol], n_active[ncol]."""
    lay: np.ndarray
    scal: np.ndarray
    n_active: np.ndarray

    @property
    def ncol(self):
        return self.lay.shape[2]

    @property
    def nlayer(self):
        return self.lay.shape[1]

    def arr(self, name):
        return self.lay[A[name]]

    def sc(self, name):
        return self.scal[S[name]]

    def copy(self):
        return State(self.lay.copy(), self.scal.copy(), self.n_active.copy())

    def replicate(self, ncol):
        """state of column 0 repeated ncol times"""
        return State(np.ascontiguousarray(np.repeat(self.lay[:, :, :1], ncol, axis=2)),
                     np.ascontiguousarray(np.repeat(self.scal[:, :1], ncol, axis=1)),
                     np.ascontiguousarray(np.repeat(self.n_active[:1], ncol)))

    def window(self, c0, n):
        return State(np.ascontiguousarray(self.lay[:, :, c0:c0 + n]), np.ascontiguousarray(self.scal[:, c0:c0 + n]),
                     np.ascontiguousarray(self.n_active[c0:c0 + n]))

    def _c(self):
        assert self.lay.dtype == np.float64 and self.lay.flags.c_contiguous
        assert self.scal.dtype == np.float64 and self.scal.flags.c_contiguous and self.scal.shape == (NSCAL, self.ncol)
        assert self.n_active.dtype == np.int32 and self.n_active.flags.c_contiguous
        return StateSoA(self.ncol, self.nlayer, self.lay.shape[0], _dp(self.lay), _dp(self.scal), _ip(self.n_active))

    @staticmethod
    def empty(ncol, nlayer, narr=NARR):
        return State(np.zeros((narr, nlayer, ncol)), np.zeros((NSCAL, ncol)), np.ones(ncol, dtype=np.int32))


@dataclass
class Output:
    lay: np.ndarray
    scal: np.ndarray
    n_active: np.ndarray
    time: float
    step: int

    def arr(self, name):
        return self.lay[A[name]]

    def sc(self, name):
        return self.scal[S[name]]


class Solver:
    """One handle of the C-ABI of include/samsim.h."""

    def __init__(self, lib: C.CDLL, prefix: str, cfg: Config, ncol: int, device: int = 0):
        self._lib = lib
        self._p = prefix
        self.cfg = cfg
        self.ncol = int(ncol)
        self.nlayer = int(cfg.nlayer)
        self._h = C.c_void_p()
        self._bind()
        self._chk(self._create(device), "create")
        self._out_window = (0, 1)
        self.ngroups = 0            # groups of set_groups; 0: no labels
        self.ntracks = 0            # tracks of set_tracks; 0: no tracking

    def _create(self, device):
        f = self._f("create")
        f.argtypes, f.restype = [C.POINTER(Config), C.c_int64, C.c_int32, C.POINTER(C.c_void_p)], C.c_int
        return f(C.byref(self.cfg), C.c_int64(self.ncol), C.c_int32(device), C.byref(self._h))

    # -- plumbing
    def _f(self, name):
        return getattr(self._lib, self._p + name)

    def _chk(self, rc, what):
        if rc != 0:
            raise SamsimError(rc, self._p + what)

    def _bind(self):
        vp, i64, i32, dp = C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_double)
        sig = {
            "set_forcing": [vp, i32, dp, dp, dp, dp, dp, dp],
            "set_forcing_sites": [vp, i32, i32, dp, dp, dp, dp, C.POINTER(C.c_int32), dp, dp],
            "set_ocean": [vp, dp, dp],
            "set_state": [vp, C.POINTER(StateSoA), i64], "get_state": [vp, C.POINTER(StateSoA), i64],
            "set_clock": [vp, C.POINTER(Clock)], "get_clock": [vp, C.POINTER(Clock)],
            "step": [vp, i64], "set_output_window": [vp, i64, i64], "get_output": [vp, C.POINTER(OutputSoA)],
            "get_status": [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int32)],
            "set_status": [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int32), i64, i64],
            "get_work": [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)],
            "get_ensemble_stats": [vp, i32, C.POINTER(C.c_int32), C.POINTER(Stat)],
            "set_tracers": [vp, i32, dp, dp], "set_tracer_state": [vp, dp, i64, i64], "set_tracer_bottom": [vp, dp, i64, i64],
            "get_tracer_state": [vp, dp, dp, i64, i64], "get_tracer_output": [vp, dp, dp],
        }
        for n, a in sig.items():
            f = self._f(n)
            f.argtypes, f.restype = a, C.c_int
        f = self._f("steps_to_output")
        f.argtypes, f.restype = [vp], C.c_int64
        f = self._f("destroy")
        f.argtypes, f.restype = [vp], None
        self._bind_extra()

    def _bind_extra(self):
        vp, i64 = C.c_void_p, C.c_int64
        f = self._f("step_timed")
        f.argtypes, f.restype = [vp, i64, C.POINTER(C.c_double)], C.c_int
        f = self._f("steps_timed")
        f.argtypes, f.restype = [vp, i64, C.c_int32, C.POINTER(C.c_double)], C.c_int
        f = self._f("synchronize")
        f.argtypes, f.restype = [vp], C.c_int
        f = self._f("get_device")
        f.argtypes, f.restype = [vp, C.POINTER(C.c_int32), C.c_char_p, C.c_int32], C.c_int
        f = self._f("set_launch_split")
        f.argtypes, f.restype = [vp, i64, C.c_int32], C.c_int
        f = self._f("get_profile_stats")
        f.argtypes, f.restype = [vp, C.POINTER(ProfileRequest), C.c_void_p], C.c_int
        # the per-group statistics came as new symbols under ABI 6: a library of ABI 6 built before them (an A/B build of an older
        # commit) still loads, and a call of one of them fails with the missing symbol's name
        group_sig = {"set_groups": [vp, C.c_int32, C.POINTER(C.c_int32)],
                     "get_group_stats": [vp, C.c_int32, C.POINTER(C.c_int32), C.c_void_p],
                     "get_group_profile_stats": [vp, C.POINTER(ProfileRequest), C.c_int32, C.c_void_p]}
        for n, a in group_sig.items():
            if hasattr(self._lib, self._p + n):
                f = self._f(n)
                f.argtypes, f.restype = a, C.c_int
        # the histograms came the same way
        hist_sig = {"get_histogram": [vp, C.c_int32, C.POINTER(HistBins), C.c_int32, C.c_void_p],
                    "get_profile_histogram": [vp, C.POINTER(ProfileRequest), C.POINTER(HistBins), C.c_int32, C.c_void_p]}
        for n, a in hist_sig.items():
            if hasattr(self._lib, self._p + n):
                f = self._f(n)
                f.argtypes, f.restype = a, C.c_int
        # and the sensitivities
        sens_sig = {"get_covariance": [vp, C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p],
                    "get_profile_regression": [vp, C.POINTER(ProfileRequest), C.c_int32, C.c_int32, C.c_void_p]}
        for n, a in sens_sig.items():
            if hasattr(self._lib, self._p + n):
                f = self._f(n)
                f.argtypes, f.restype = a, C.c_int
        # and the time-domain diagnostics
        track_sig = {"set_tracks": [vp, C.c_int32, C.POINTER(TrackSpec), i64], "reset_tracks": [vp],
                     "get_tracks": [vp, C.c_int32, i64, i64, C.c_void_p], "set_track_state": [vp, C.c_int32, i64, i64, C.c_void_p]}
        for n, a in track_sig.items():
            if hasattr(self._lib, self._p + n):
                f = self._f(n)
                f.argtypes, f.restype = a, C.c_int
        # and the selection of columns and the gather of scattered ones
        select_sig = {"select_columns": [vp, C.POINTER(Selection), i64, C.c_void_p, C.POINTER(C.c_int64)],
                      "get_columns": [vp, i64, C.c_void_p, C.POINTER(StateSoA), C.c_void_p, C.c_void_p, C.c_void_p]}
        for n, a in select_sig.items():
            if hasattr(self._lib, self._p + n):
                f = self._f(n)
                f.argtypes, f.restype = a, C.c_int
        # and the column functionals
        func_sig = {"set_functionals": [vp, C.c_int32, C.POINTER(FunctionalSpec)], "get_functionals": [vp, C.c_int32, i64, i64, C.c_void_p]}
        for n, a in func_sig.items():
            if hasattr(self._lib, self._p + n):
                f = self._f(n)
                f.argtypes, f.restype = a, C.c_int
        # and the sensors and scores
        sensor_sig = {"set_sensors": [vp, C.c_int32, C.POINTER(SensorSpec)], "get_sensor_values": [vp, i64, C.c_void_p, C.c_void_p],
                      "score": [vp, C.c_void_p, C.c_void_p, C.c_int32], "get_scores": [vp, i64, i64, C.c_void_p],
                      "set_score_state": [vp, i64, i64, C.c_void_p], "reset_scores": [vp]}
        for n, a in sensor_sig.items():
            if hasattr(self._lib, self._p + n):
                f = self._f(n)
                f.argtypes, f.restype = a, C.c_int
        # and the weight row and the weighted reductions
        weight_sig = {"set_weights": [vp, C.POINTER(WeightSpec), C.POINTER(WeightInfo)], "get_weights": [vp, i64, i64, C.c_void_p],
                      "get_weighted_stats": [vp, C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_void_p],
                      "get_weighted_histogram": [vp, C.c_int32, C.POINTER(HistBins), C.c_int32, C.c_void_p]}
        for n, a in weight_sig.items():
            if hasattr(self._lib, self._p + n):
                f = self._f(n)
                f.argtypes, f.restype = a, C.c_int
        # and the weighted profile statistics and the weighted covariances
        wprof_sig = {"get_weighted_profile_stats": [vp, C.POINTER(ProfileRequest), C.c_int32, C.c_void_p],
                     "get_weighted_covariance": [vp, C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int64),
                                                 C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p, C.c_void_p]}
        for n, a in wprof_sig.items():
            if hasattr(self._lib, self._p + n):
                f = self._f(n)
                f.argtypes, f.restype = a, C.c_int
        # and the weighted joint histogram of a profile
        wphist_sig = {"get_weighted_profile_histogram": [vp, C.POINTER(ProfileRequest), C.POINTER(HistBins), C.c_int32, C.c_void_p]}
        for n, a in wphist_sig.items():
            if hasattr(self._lib, self._p + n):
                f = self._f(n)
                f.argtypes, f.restype = a, C.c_int
        # and the posterior draw
        resample_sig = {"resample": [vp, C.POINTER(ResampleSpec), C.POINTER(ResampleInfo)], "get_offspring": [vp, i64, i64, C.c_void_p],
                        "get_ancestors": [vp, i64, i64, C.c_void_p]}
        for n, a in resample_sig.items():
            if hasattr(self._lib, self._p + n):
                f = self._f(n)
                f.argtypes, f.restype = a, C.c_int

        # and the copy of whole columns on the device
        copy_sig = {"copy_columns": [vp, i64, C.c_void_p, C.c_void_p, C.c_int32], "apply_resample": [vp, C.c_int32, C.POINTER(ApplyInfo)],
                    "get_copy_plan": [vp, i64, i64, C.c_void_p, C.c_void_p]}
        for n, a in copy_sig.items():
            if hasattr(self._lib, self._p + n):
                f = self._f(n)
                f.argtypes, f.restype = a, C.c_int
        # and the jitter of the per-column parameters, with the getter of the ocean rows
        jitter_sig = {"jitter": [vp, C.POINTER(JitterSpec), C.POINTER(JitterInfo)], "get_ocean": [vp, i64, i64, C.c_void_p, C.c_void_p]}
        for n, a in jitter_sig.items():
            if hasattr(self._lib, self._p + n):
                f = self._f(n)
                f.argtypes, f.restype = a, C.c_int

    # -- API
    def set_forcing(self, fl_sw, fl_lw, T2m, precip, dT2m=None, precip_scale=None):
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (fl_sw, fl_lw, T2m, precip)]
        n = len(arrs[0])
        assert all(len(a) == n for a in arrs)
        d = None if dT2m is None else np.ascontiguousarray(dT2m, dtype=np.float64)
        p = None if precip_scale is None else np.ascontiguousarray(precip_scale, dtype=np.float64)
        assert d is None or d.shape == (self.ncol,)
        assert p is None or p.shape == (self.ncol,)
        self._chk(self._f("set_forcing")(self._h, n, *[_dp(a) for a in arrs],
                                         _dp(d) if d is not None else None, _dp(p) if p is not None else None),
                  "set_forcing")

    def set_forcing_sites(self, fl_sw, fl_lw, T2m, precip, site_of_column, dT2m=None, precip_scale=None):
        """tables [nsites][len] (samsim_set_forcing_sites): column c reads set site_of_column[c]"""
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (fl_sw, fl_lw, T2m, precip)]
        nsites, n = arrs[0].shape
        assert all(a.shape == (nsites, n) for a in arrs)
        site = np.ascontiguousarray(site_of_column, dtype=np.int32)
        assert site.shape == (self.ncol,)
        d = None if dT2m is None else np.ascontiguousarray(dT2m, dtype=np.float64)
        p = None if precip_scale is None else np.ascontiguousarray(precip_scale, dtype=np.float64)
        self._chk(self._f("set_forcing_sites")(self._h, nsites, n, *[_dp(a) for a in arrs], _ip(site),
                                               _dp(d) if d is not None else None, _dp(p) if p is not None else None),
                  "set_forcing_sites")

    def set_ocean(self, dfl_q_bottom=None, S_bu_bottom=None):
        """the water below a grid of columns (samsim_set_ocean): per-column offset on the oceanic heat flux sub_test4 sets every
        step, per-column salinity of the water below (tank_flag 1); None switches a part off"""
        d = None if dfl_q_bottom is None else np.ascontiguousarray(dfl_q_bottom, dtype=np.float64)
        s = None if S_bu_bottom is None else np.ascontiguousarray(S_bu_bottom, dtype=np.float64)
        assert d is None or d.shape == (self.ncol,)
        assert s is None or s.shape == (self.ncol,)
        self._chk(self._f("set_ocean")(self._h, _dp(d) if d is not None else None, _dp(s) if s is not None else None), "set_ocean")

    def set_state(self, st: State, col0: int = 0):
        s = st._c()
        self._chk(self._f("set_state")(self._h, C.byref(s), col0), "set_state")

    def get_state(self, col0: int = 0, ncols: int | None = None, narr: int = NARR) -> State:
        n = self.ncol - col0 if ncols is None else ncols
        st = State.empty(n, self.nlayer, narr)
        s = st._c()
        self._chk(self._f("get_state")(self._h, C.byref(s), col0), "get_state")
        return st

    def set_clock(self, time=0.0, step=0, n_time_out=0, time_counter=1, n_outputs=0):
        c = Clock(time, step, n_time_out, time_counter, n_outputs)
        self._chk(self._f("set_clock")(self._h, C.byref(c)), "set_clock")

    def get_clock(self) -> Clock:
        c = Clock()
        self._chk(self._f("get_clock")(self._h, C.byref(c)), "get_clock")
        return c

    def step(self, nsteps: int = 1):
        self._chk(self._f("step")(self._h, nsteps), "step")

    def step_timed(self, nsteps: int) -> float:
        ms = C.c_double()
        self._chk(self._f("step_timed")(self._h, nsteps, C.byref(ms)), "step_timed")
        return ms.value

    def steps_timed(self, nsteps: int, nlaunches: int) -> float:
        """nlaunches launches of nsteps steps each, enqueued back to back; device time of the whole sequence [ms]"""
        ms = C.c_double()
        self._chk(self._f("steps_timed")(self._h, nsteps, nlaunches, C.byref(ms)), "steps_timed")
        return ms.value

    def synchronize(self):
        self._chk(self._f("synchronize")(self._h), "synchronize")

    def get_device(self):
        """(HIP device ordinal, PCI bus id) of the GPU this handle lives on"""
        dev, buf = C.c_int32(-1), C.create_string_buffer(32)
        self._chk(self._f("get_device")(self._h, C.byref(dev), buf, 32), "get_device")
        return int(dev.value), buf.value.decode()

    def set_launch_split(self, min_blocks: int = 8192, first_part_eighths: int = 4):
        """from how many 64-column blocks a step runs as two concurrent launches (0 = never), and the first part's share"""
        self._chk(self._f("set_launch_split")(self._h, min_blocks, first_part_eighths), "set_launch_split")

    def steps_to_output(self) -> int:
        return int(self._f("steps_to_output")(self._h))

    def set_output_window(self, col0: int, ncols: int):
        self._chk(self._f("set_output_window")(self._h, col0, ncols), "set_output_window")
        self._out_window = (col0, ncols)

    def get_output(self) -> Output:
        n = self._out_window[1]
        lay = np.zeros((NARR, self.nlayer, n))
        scal = np.zeros((NSCAL, n))
        na = np.zeros(n, dtype=np.int32)
        o = OutputSoA(n, self.nlayer, 0, _dp(lay), _dp(scal), _ip(na), 0.0, 0)
        self._chk(self._f("get_output")(self._h, C.byref(o)), "get_output")
        return Output(lay, scal, na, o.time, o.step)

    def get_status(self):
        st = np.zeros(self.ncol, dtype=np.int32)
        sp = np.zeros(self.ncol, dtype=np.int64)
        ly = np.zeros(self.ncol, dtype=np.int32)
        self._chk(self._f("get_status")(self._h, _ip(st), sp.ctypes.data_as(C.POINTER(C.c_int64)), _ip(ly)), "get_status")
        return st, sp, ly

    def set_status(self, status, step=None, layer=None, col0: int = 0):
        """restart: put back the STOP codes (and the step / layer of the failure) samsim_get_status returned"""
        st = np.ascontiguousarray(status, dtype=np.int32)
        sp = None if step is None else np.ascontiguousarray(step, dtype=np.int64)
        ly = None if layer is None else np.ascontiguousarray(layer, dtype=np.int32)
        self._chk(self._f("set_status")(self._h, _ip(st), sp.ctypes.data_as(C.POINTER(C.c_int64)) if sp is not None else None,
                                        _ip(ly) if ly is not None else None, col0, len(st)), "set_status")

    def get_work(self):
        a, b = C.c_int64(), C.c_int64()
        self._chk(self._f("get_work")(self._h, C.byref(a), C.byref(b)), "get_work")
        return a.value, b.value

    # -- passive tracers (bgc_flag 2)
    def set_tracers(self, bgc_bottom, bgc_total=None):
        """number of tracers = len(bgc_bottom); concentrations below the ice; tank totals for tank_flag 2"""
        b = np.ascontiguousarray(bgc_bottom, dtype=np.float64)
        t = None if bgc_total is None else np.ascontiguousarray(bgc_total, dtype=np.float64)
        self.n_bgc = len(b)
        self._chk(self._f("set_tracers")(self._h, self.n_bgc, _dp(b), _dp(t) if t is not None else None), "set_tracers")

    def set_tracer_state(self, bgc_abs, col0: int = 0):
        """bgc_abs[n_bgc][nlayer][ncols]"""
        a = np.ascontiguousarray(bgc_abs, dtype=np.float64)
        assert a.shape[:2] == (self.n_bgc, self.nlayer)
        self._chk(self._f("set_tracer_state")(self._h, _dp(a), col0, a.shape[2]), "set_tracer_state")

    def set_tracer_bottom(self, bgc_bottom, col0: int = 0):
        """bgc_bottom[n_bgc][ncols]: per-column concentration below the ice, as get_tracer_state returned it (restart)"""
        b = np.ascontiguousarray(bgc_bottom, dtype=np.float64)
        assert b.shape[0] == self.n_bgc
        self._chk(self._f("set_tracer_bottom")(self._h, _dp(b), col0, b.shape[1]), "set_tracer_bottom")

    def get_tracer_state(self, col0: int = 0, ncols: int | None = None):
        n = self.ncol - col0 if ncols is None else ncols
        a, b = np.zeros((self.n_bgc, self.nlayer, n)), np.zeros((self.n_bgc, n))
        self._chk(self._f("get_tracer_state")(self._h, _dp(a), _dp(b), col0, n), "get_tracer_state")
        return a, b

    def get_tracer_output(self):
        """tracer snapshot of the output window at the reference's output point: (bgc_abs, bgc_bottom)"""
        w = self._out_window[1]
        a, b = np.zeros((self.n_bgc, self.nlayer, w)), np.zeros((self.n_bgc, w))
        self._chk(self._f("get_tracer_output")(self._h, _dp(a), _dp(b)), "get_tracer_output")
        return a, b

    def ensemble_stats(self, names):
        """{name: Stat} over the columns without a STOP code; names from SCALARS, "N_active" or ints of track_slot
        (samsim_get_ensemble_stats)"""
        names = list(names)
        slots = (C.c_int32 * len(names))(*[_slot(n) for n in names])
        out = (Stat * len(names))()
        self._chk(self._f("get_ensemble_stats")(self._h, len(names), slots, out), "get_ensemble_stats")
        return {n: out[i] for i, n in enumerate(names)}

    def set_groups_raw(self, ngroups, labels):
        """samsim_set_groups with the arguments as given (no checks on this side): labels an int32 array [ncol] or None"""
        self._chk(self._f("set_groups")(self._h, ngroups, _ip(labels) if labels is not None else None), "set_groups")
        self.ngroups = int(ngroups) if labels is not None else 0

    def set_groups(self, labels, ngroups=None):
        """a group label per column, -1 = in no group (samsim_set_groups); ngroups defaults to max(label) + 1; set_groups(None)
        removes the labels"""
        if labels is None:
            return self.set_groups_raw(0, None)
        lab = np.ascontiguousarray(labels, dtype=np.int32)
        assert lab.shape == (self.ncol,)
        if ngroups is None:
            ngroups = int(lab.max()) + 1
            if ngroups < 1:
                raise ValueError("every label is -1: no group to count; pass ngroups, or set_groups(None) to remove the labels")
        self.set_groups_raw(int(ngroups), lab)

    def group_stats(self, names):
        """{name: structured array [ngroups] with fields count, mean, min, max, std} over the columns without a STOP code, per
        group of set_groups; names from SCALARS, "N_active" or ints of track_slot (samsim_get_group_stats)"""
        names = list(names)
        ng = self.ngroups
        slots = (C.c_int32 * len(names))(*[_slot(n) for n in names])
        out = np.zeros((len(names), max(1, ng)), dtype=STAT_DTYPE)
        self._chk(self._f("get_group_stats")(self._h, len(names), slots, out.ctypes.data), "get_group_stats")
        return {n: out[i] for i, n in enumerate(names)}

    def profile_stats_raw(self, rq: ProfileRequest, group=None) -> np.ndarray:
        """samsim_get_profile_stats -- with group: samsim_get_group_profile_stats -- with the request as given (no checks on this
        side): structured array [narrays][nbins]"""
        out = np.zeros((max(0, min(rq.narrays, PROFILE_MAX_ARRAYS)), max(0, min(rq.nbins, PROFILE_MAX_BINS))), dtype=STAT_DTYPE)
        buf = np.zeros(max(1, out.size), dtype=STAT_DTYPE)
        if group is None:
            self._chk(self._f("get_profile_stats")(self._h, C.byref(rq), buf.ctypes.data), "get_profile_stats")
        else:
            self._chk(self._f("get_group_profile_stats")(self._h, C.byref(rq), int(group), buf.ctypes.data), "get_group_profile_stats")
        out.ravel()[:] = buf[:out.size]
        return out

    def profile_stats(self, names, axis="layer", origin="top", nbins=None, z0=0.0, dz=None, group=None):
        """{name: structured array [nbins] with fields count, mean, min, max, std} over the columns without a STOP code
        (samsim_get_profile_stats): names from ARRAYS; axis "layer" (bin b = layer b+1 from the top, or N_active-b from the
        bottom; nbins defaults to nlayer) or "depth" (bins [z0 + b dz, z0 + (b+1) dz) in metres below the ice surface or above
        the ice bottom; nbins and dz are required); group: only the columns with that label of set_groups
        (samsim_get_group_profile_stats)"""
        names = list(names)
        if axis == "depth" and (nbins is None or dz is None):
            raise ValueError("axis='depth' needs nbins and dz")
        rq = self._profile_request(names, axis, origin, nbins, z0, dz)
        out = self.profile_stats_raw(rq) if group is None else self.profile_stats_raw(rq, group)
        return {n: out[i] for i, n in enumerate(names)}

    def _profile_request(self, names, axis, origin, nbins, z0, dz) -> ProfileRequest:
        rq = ProfileRequest()
        rq.struct_size = C.sizeof(ProfileRequest)
        rq.axis, rq.origin = PROFILE_AXES[axis], PROFILE_ORIGINS[origin]
        rq.nbins = self.nlayer if nbins is None else int(nbins)
        rq.narrays = len(names)
        for i, n in enumerate(names[:PROFILE_MAX_ARRAYS]):
            rq.arrays[i] = A[n]
        rq.z0, rq.dz = float(z0), float(0.0 if dz is None else dz)
        return rq

    def histogram_raw(self, slot, vb: HistBins, by_group=0) -> np.ndarray:
        """samsim_get_histogram with the arguments as given (no checks on this side): int64 [nvbins+2], with by_group
        [ngroups, nvbins+2]"""
        w = max(0, min(vb.nvbins, HIST_MAX_VBINS)) + 2
        rows = max(1, self.ngroups) if by_group == 1 else 1
        buf = np.zeros((rows, w), dtype=np.int64)
        self._chk(self._f("get_histogram")(self._h, int(slot), C.byref(vb), int(by_group), buf.ctypes.data), "get_histogram")
        return buf if by_group == 1 else buf[0]

    def histogram(self, name, nvbins, v0, dv, by_group=False) -> np.ndarray:
        """fixed-edge histogram of a scalar from SCALARS, of "N_active" or of a track row (an int of track_slot) over the columns without a STOP code
        (samsim_get_histogram): edges v0 + j dv, j = 0..nvbins; entry 0 counts the values below the first edge, entry j+1 those
        in [E_j, E_{j+1}), entry nvbins+1 those at or above the last edge.  int64 [nvbins+2]; by_group: [ngroups, nvbins+2] per
        group of set_groups"""
        return self.histogram_raw(_slot(name), hist_bins(nvbins, v0, dv), 1 if by_group else 0)

    def profile_histogram_raw(self, rq: ProfileRequest, vb: HistBins, group=-1) -> np.ndarray:
        """samsim_get_profile_histogram with the arguments as given (no checks on this side): int64 [nbins, nvbins+2]"""
        buf = np.zeros((max(1, min(rq.nbins, PROFILE_MAX_BINS)), max(0, min(vb.nvbins, HIST_MAX_VBINS)) + 2), dtype=np.int64)
        self._chk(self._f("get_profile_histogram")(self._h, C.byref(rq), C.byref(vb), int(group), buf.ctypes.data),
                  "get_profile_histogram")
        return buf

    def profile_histogram(self, name, nvbins, v0, dv, axis="layer", origin="top", nbins=None, z0=0.0, dz=None, group=None) -> np.ndarray:
        """joint histogram over depth bin x value bin of one array from ARRAYS (samsim_get_profile_histogram): the bins and the
        per-column bin values of profile_stats, the value entries of histogram.  int64 [nbins, nvbins+2]; group: only the
        columns with that label of set_groups"""
        if axis == "depth" and (nbins is None or dz is None):
            raise ValueError("axis='depth' needs nbins and dz")
        rq = self._profile_request([name], axis, origin, nbins, z0, dz)
        return self.profile_histogram_raw(rq, hist_bins(nvbins, v0, dv), -1 if group is None else int(group))

    def covariance_raw(self, slots, group=-1):
        """samsim_get_covariance with the arguments as given (no checks on this side): (count, mean [nslots], cov [nslots, nslots])"""
        slots = [int(x) for x in slots]
        n = len(slots)
        arr = (C.c_int32 * max(1, n))(*slots)
        count = C.c_int64(0)
        m = max(1, min(n, SENS_MAX_SLOTS))
        mean, cov = np.zeros(m), np.zeros((m, m))
        self._chk(self._f("get_covariance")(self._h, n, arr, int(group), C.byref(count), mean.ctypes.data, cov.ctypes.data), "get_covariance")
        return int(count.value), mean, cov

    def covariance(self, names, group=None):
        """(count, mean [n], cov [n, n]) of the scalars `names` (from SCALARS, "N_active", or ints of track_slot) over the columns without a STOP code --
        with group: over those with that label of set_groups -- (samsim_get_covariance): population covariances, the diagonal the
        variances; capi.correlation(cov) gives the correlations"""
        return self.covariance_raw([_slot(n) for n in names], -1 if group is None else int(group))

    def profile_regression_raw(self, rq: ProfileRequest, predictor_slot, group=-1) -> np.ndarray:
        """samsim_get_profile_regression with the arguments as given (no checks on this side): PAIR_STAT_DTYPE [narrays][nbins]"""
        out = np.zeros((max(0, min(rq.narrays, PROFILE_MAX_ARRAYS)), max(0, min(rq.nbins, PROFILE_MAX_BINS))), dtype=PAIR_STAT_DTYPE)
        buf = np.zeros(max(1, out.size), dtype=PAIR_STAT_DTYPE)
        self._chk(self._f("get_profile_regression")(self._h, C.byref(rq), int(predictor_slot), int(group), buf.ctypes.data),
                  "get_profile_regression")
        out.ravel()[:] = buf[:out.size]
        return out

    def profile_regression(self, names, predictor, axis="layer", origin="top", nbins=None, z0=0.0, dz=None, group=None):
        """{name: PAIR_STAT_DTYPE array [nbins]}: per bin of profile_stats the joint moments of the bin value y of the array and the
        column's scalar `predictor` x (from SCALARS, "N_active", or an int of track_slot) over the columns that contribute to the bin
        (samsim_get_profile_regression); capi.slope_and_correlation gives dy/dx and the correlation per bin"""
        names = list(names)
        if axis == "depth" and (nbins is None or dz is None):
            raise ValueError("axis='depth' needs nbins and dz")
        rq = self._profile_request(names, axis, origin, nbins, z0, dz)
        out = self.profile_regression_raw(rq, _slot(predictor), -1 if group is None else int(group))
        return {n: out[i] for i, n in enumerate(names)}

    # -- time-domain diagnostics
    def set_tracks_raw(self, ntracks, specs, every):
        """samsim_set_tracks with the arguments as given (no checks on this side): specs a ctypes array of TrackSpec or None"""
        self._chk(self._f("set_tracks")(self._h, int(ntracks), specs, int(every)), "set_tracks")
        self.ntracks = int(ntracks) if specs is not None else 0

    def set_tracks(self, specs, every=1):
        """follow the observables `specs` (TrackSpec, at most MAX_TRACKS) through the run: from now on every column without a
        STOP code is sampled after each step that brings clock.step to a multiple of `every` (samsim_set_tracks).  The rows start
        from TRACK_INITIAL.  set_tracks(None) removes tracking"""
        if specs is None:
            return self.set_tracks_raw(0, None, 0)
        specs = list(specs)
        self.set_tracks_raw(len(specs), (TrackSpec * max(1, len(specs)))(*specs), every)

    def reset_tracks(self):
        """the rows of every track back to TRACK_INITIAL (samsim_reset_tracks)"""
        self._chk(self._f("reset_tracks")(self._h), "reset_tracks")

    def tracks(self, track, col0: int = 0, ncols: int | None = None):
        """{field: float64 [ncols]} of one track, fields from TRACK_FIELDS (samsim_get_tracks)"""
        n = self.ncol - col0 if ncols is None else ncols
        buf = np.zeros((NTF, max(0, n)))
        self._chk(self._f("get_tracks")(self._h, int(track), col0, n, buf.ctypes.data), "get_tracks")
        return {f: buf[i] for i, f in enumerate(TRACK_FIELDS)}

    def set_track_state(self, track, fields, col0: int = 0):
        """restart: put back what tracks() returned for the columns [col0, col0 + ncols) of one track (samsim_set_track_state);
        set_tracks comes first"""
        buf = np.ascontiguousarray(np.stack([np.asarray(fields[f], dtype=np.float64) for f in TRACK_FIELDS]))
        self._chk(self._f("set_track_state")(self._h, int(track), col0, buf.shape[1], buf.ctypes.data), "set_track_state")

    # -- which columns, and what they look like
    def select_raw(self, sel: Selection, max_out, out=None):
        """samsim_select_columns with the arguments as given (no checks on this side): (int64 array of the first min(n_match,
        max_out) matching column indices in ascending order, n_match).  max_out == 0 only counts (cols_out NULL).  out: an int64
        array of at least max_out entries to receive the indices in place (entries beyond them are left alone)"""
        n = C.c_int64(-1)
        if out is None:
            out = np.zeros(max(0, min(int(max_out), SELECT_MAX_OUT)), dtype=np.int64)
        assert out.dtype == np.int64 and out.flags.c_contiguous
        self._chk(self._f("select_columns")(self._h, C.byref(sel), int(max_out), out.ctypes.data if int(max_out) != 0 else None,
                                            C.byref(n)), "select_columns")
        return out[:max(0, min(int(n.value), int(max_out)))], int(n.value)

    def select(self, terms=(), group=None, status="running", max_out=SELECT_MAX_OUT):
        """(indices, n_match): the columns for which every term (name_or_slot, lo, hi) holds -- lo <= x < hi, names from SCALARS,
        "N_active" or ints of track_slot --, with label `group` of set_groups (None: any) and status "running" (the columns the
        statistics count), "stopped", "any" or an integer STOP code (samsim_select_columns).  indices: int64, ascending, the first
        min(n_match, max_out); n_match is exact whatever max_out is"""
        return self.select_raw(Selection.make(terms, group, status), max_out)

    def get_columns(self, cols, narr: int = NARR, with_status=False):
        """State of the columns `cols` (any order, duplicates allowed, at most SELECT_MAX_OUT), position j holding column cols[j]:
        the bytes get_state returns for those columns (samsim_get_columns).  with_status: (State, (status, step, layer)), the
        entries of get_status for those columns"""
        cols = np.ascontiguousarray(cols, dtype=np.int64)
        assert cols.ndim == 1
        n = cols.size
        st = State.empty(max(1, n), self.nlayer, narr)
        s = st._c()
        s.ncol = n
        if not with_status:
            self._chk(self._f("get_columns")(self._h, n, cols.ctypes.data, C.byref(s), None, None, None), "get_columns")
            return st
        status, step, layer = np.zeros(max(1, n), dtype=np.int32), np.zeros(max(1, n), dtype=np.int64), np.zeros(max(1, n), dtype=np.int32)
        self._chk(self._f("get_columns")(self._h, n, cols.ctypes.data, C.byref(s), status.ctypes.data, step.ctypes.data, layer.ctypes.data),
                  "get_columns")
        return st, (status, step, layer)

    # -- column functionals
    def set_functionals_raw(self, n, specs):
        """samsim_set_functionals with the arguments as given (no checks on this side): specs a ctypes array of FunctionalSpec or None"""
        self._chk(self._f("set_functionals")(self._h, int(n), specs), "set_functionals")
        self.nfunctionals = int(n) if specs is not None else 0

    def set_functionals(self, specs):
        """evaluate the functionals `specs` (FunctionalSpec, at most MAX_FUNCTIONALS) of every column's layer profile on the device
        (samsim_set_functionals): func_slot(i) is then the row of specs[i] wherever a slot is accepted, always current.
        set_functionals(None) removes them"""
        if specs is None:
            return self.set_functionals_raw(0, None)
        specs = list(specs)
        self.set_functionals_raw(len(specs), (FunctionalSpec * max(1, len(specs)))(*specs))

    def functionals(self, index, col0: int = 0, ncols: int | None = None) -> np.ndarray:
        """float64 [ncols]: the value of functional `index` in the columns [col0, col0 + ncols), stopped ones included
        (samsim_get_functionals)"""
        n = self.ncol - col0 if ncols is None else ncols
        buf = np.zeros(max(0, n))
        self._chk(self._f("get_functionals")(self._h, int(index), col0, n, buf.ctypes.data), "get_functionals")
        return buf

    # -- sensors and the per-column misfit
    def set_sensors_raw(self, n, specs):
        """samsim_set_sensors with the arguments as given (no checks on this side): specs a ctypes array of SensorSpec or None"""
        self._chk(self._f("set_sensors")(self._h, int(n), specs), "set_sensors")
        self.nsensors = int(n) if specs is not None else 0

    def set_sensors(self, specs):
        """name the sensors `specs` (SensorSpec, at most MAX_SENSORS) and allocate the score rows, all zero (samsim_set_sensors):
        score_slot(field) is then a row wherever a slot is accepted.  set_sensors(None) removes sensors and rows"""
        if specs is None:
            return self.set_sensors_raw(0, None)
        specs = list(specs)
        self.set_sensors_raw(len(specs), (SensorSpec * max(1, len(specs)))(*specs))

    def sensor_values(self, cols) -> np.ndarray:
        """float64 [nsensors, len(cols)]: the model's equivalent of every sensor for the columns `cols` (any order, duplicates
        allowed, at most SELECT_MAX_OUT), stopped ones included (samsim_get_sensor_values)"""
        cols = np.ascontiguousarray(cols, dtype=np.int64)
        assert cols.ndim == 1
        y = np.zeros((getattr(self, "nsensors", 0), cols.size))
        self._chk(self._f("get_sensor_values")(self._h, cols.size, cols.ctypes.data, y.ctypes.data), "get_sensor_values")
        return y

    def score(self, obs, weight=None, group=None):
        """add the weighted squared differences between the sensors and the observations `obs` [nsensors] (NaN: no observation) to
        the score rows of the running columns -- with group: of those with that label of set_groups -- (samsim_score)"""
        obs = np.ascontiguousarray(obs, dtype=np.float64)
        w = None if weight is None else np.ascontiguousarray(weight, dtype=np.float64)
        assert obs.shape == (self.nsensors,) and (w is None or w.shape == obs.shape)
        self._chk(self._f("score")(self._h, obs.ctypes.data, None if w is None else w.ctypes.data, -1 if group is None else int(group)),
                  "score")

    def scores(self, col0: int = 0, ncols: int | None = None):
        """{field: float64 [ncols]} of the score rows, fields from SCORE_FIELDS (samsim_get_scores)"""
        n = self.ncol - col0 if ncols is None else ncols
        buf = np.zeros((NSF, max(0, n)))
        self._chk(self._f("get_scores")(self._h, col0, n, buf.ctypes.data), "get_scores")
        return {f: buf[i] for i, f in enumerate(SCORE_FIELDS)}

    def set_score_state(self, fields, col0: int = 0):
        """restart: put back what scores() returned for the columns [col0, col0 + ncols) (samsim_set_score_state); set_sensors
        comes first"""
        buf = np.ascontiguousarray(np.stack([np.asarray(fields[f], dtype=np.float64) for f in SCORE_FIELDS]))
        self._chk(self._f("set_score_state")(self._h, col0, buf.shape[1], buf.ctypes.data), "set_score_state")

    def reset_scores(self):
        """every score row back to 0.0 (samsim_reset_scores)"""
        self._chk(self._f("reset_scores")(self._h), "reset_scores")

    # -- the weight row and the weighted (posterior) reductions
    def set_weights_raw(self, spec, info=None):
        """samsim_set_weights with the arguments as given (no checks on this side): spec a WeightSpec or None, info a WeightInfo or
        None"""
        self._chk(self._f("set_weights")(self._h, None if spec is None else C.byref(spec), None if info is None else C.byref(info)),
                  "set_weights")

    def set_weights(self, slot, kind="gauss", scale=1.0, group=None):
        """form the weight row on the device from the slot's values of the running columns -- with group: of those with that label
        of set_groups; every other column gets 0 -- (samsim_set_weights): "gauss" w = exp(-(x - x_min) / (2 scale)), with
        slot=score_slot("J_SUM") the likelihood of the accumulated misfit relative to the best member; "direct" w = x where
        0 < x < inf.  weight_slot() is then the row wherever a slot is accepted.  Returns {"n_in", "n_pos", "x_min", "sum_w",
        "sum_w2", "ess"}, ess = sum_w^2 / sum_w2 the effective sample size (0.0 without a positive weight)"""
        info = WeightInfo()
        self.set_weights_raw(WeightSpec.make(slot, kind, scale, group), info)
        ess = info.sum_w * info.sum_w / info.sum_w2 if info.sum_w2 > 0.0 else 0.0
        return {"n_in": int(info.n_in), "n_pos": int(info.n_pos), "x_min": info.x_min, "sum_w": info.sum_w, "sum_w2": info.sum_w2,
                "ess": ess}

    def clear_weights(self):
        """remove the weight row (samsim_set_weights with NULL), also when none was set"""
        self.set_weights_raw(None)

    def weights(self, col0: int = 0, ncols: int | None = None) -> np.ndarray:
        """float64 [ncols]: the weights of the columns [col0, col0 + ncols) (samsim_get_weights)"""
        n = self.ncol - col0 if ncols is None else ncols
        buf = np.zeros(max(0, n))
        self._chk(self._f("get_weights")(self._h, col0, n, buf.ctypes.data), "get_weights")
        return buf

    def weighted_stats_raw(self, slots, group=-1) -> np.ndarray:
        """samsim_get_weighted_stats with the arguments as given (no checks on this side): WSTAT_DTYPE [nslots]"""
        slots = [int(x) for x in slots]
        n = len(slots)
        arr = (C.c_int32 * max(1, n))(*slots)
        out = np.zeros(max(1, min(n, SENS_MAX_SLOTS)), dtype=WSTAT_DTYPE)
        self._chk(self._f("get_weighted_stats")(self._h, n, arr, int(group), out.ctypes.data), "get_weighted_stats")
        return out[:max(0, min(n, SENS_MAX_SLOTS))]

    def weighted_stats(self, names, group=None):
        """{name: WSTAT_DTYPE record} of the slots `names` (from SCALARS, "N_active", or ints of track_slot, func_slot, score_slot)
        over the running columns with a positive weight -- with group: of those with that label -- (samsim_get_weighted_stats):
        count, sum_w, sum_w2, the weighted mean, the weighted population variance sum w (x - mean)^2 / sum w, min and max"""
        names = list(names)
        out = self.weighted_stats_raw([_slot(n) for n in names], -1 if group is None else int(group))
        return {n: out[i] for i, n in enumerate(names)}

    def weighted_histogram_raw(self, slot, vb: HistBins, group=-1) -> np.ndarray:
        """samsim_get_weighted_histogram with the arguments as given (no checks on this side): float64 [nvbins+2]"""
        buf = np.zeros(max(0, min(vb.nvbins, HIST_MAX_VBINS)) + 2)
        self._chk(self._f("get_weighted_histogram")(self._h, int(slot), C.byref(vb), int(group), buf.ctypes.data), "get_weighted_histogram")
        return buf

    def weighted_histogram(self, name, nvbins, v0, dv, group=None) -> np.ndarray:
        """the sum of the weights per entry of histogram() over the running columns with a positive weight -- with group: of those
        with that label -- (samsim_get_weighted_histogram): float64 [nvbins+2]; capi.weighted_quantile_bracket reads quantiles off
        it"""
        return self.weighted_histogram_raw(_slot(name), hist_bins(nvbins, v0, dv), -1 if group is None else int(group))

    def weighted_profile_stats_raw(self, rq: ProfileRequest, group=-1) -> np.ndarray:
        """samsim_get_weighted_profile_stats with the arguments as given (no checks on this side): WSTAT_DTYPE [narrays][nbins]"""
        out = np.zeros((max(0, min(rq.narrays, PROFILE_MAX_ARRAYS)), max(0, min(rq.nbins, PROFILE_MAX_BINS))), dtype=WSTAT_DTYPE)
        buf = np.zeros(max(1, out.size), dtype=WSTAT_DTYPE)
        self._chk(self._f("get_weighted_profile_stats")(self._h, C.byref(rq), int(group), buf.ctypes.data), "get_weighted_profile_stats")
        out.ravel()[:] = buf[:out.size]
        return out

    def weighted_profile_stats(self, names, axis="layer", origin="top", nbins=None, z0=0.0, dz=None, group=None):
        """{name: WSTAT_DTYPE array [nbins]}: per bin of profile_stats the count, sum_w, sum_w2, the weighted mean, the weighted
        population variance, min and max of the bin value over the running columns with a positive weight that contribute to the
        bin -- with group: of those with that label -- (samsim_get_weighted_profile_stats): the posterior profile with its spread;
        sum_w^2 / sum_w2 is the effective sample size of a bin"""
        names = list(names)
        if axis == "depth" and (nbins is None or dz is None):
            raise ValueError("axis='depth' needs nbins and dz")
        rq = self._profile_request(names, axis, origin, nbins, z0, dz)
        out = self.weighted_profile_stats_raw(rq, -1 if group is None else int(group))
        return {n: out[i] for i, n in enumerate(names)}

    def weighted_profile_histogram_raw(self, rq: ProfileRequest, vb: HistBins, group=-1) -> np.ndarray:
        """samsim_get_weighted_profile_histogram with the arguments as given (no checks on this side): float64 [nbins, nvbins+2]"""
        buf = np.zeros((max(1, min(rq.nbins, PROFILE_MAX_BINS)), max(0, min(vb.nvbins, HIST_MAX_VBINS)) + 2))
        self._chk(self._f("get_weighted_profile_histogram")(self._h, C.byref(rq), C.byref(vb), int(group), buf.ctypes.data),
                  "get_weighted_profile_histogram")
        return buf

    def weighted_profile_histogram(self, name, nvbins, v0, dv, axis="layer", origin="top", nbins=None, z0=0.0, dz=None,
                                   group=None) -> np.ndarray:
        """the sum of the weights per depth bin x value entry of profile_histogram() over the running columns with a positive weight
        -- with group: of those with that label -- (samsim_get_weighted_profile_histogram): float64 [nbins, nvbins+2];
        capi.weighted_profile_quantiles reads the posterior median and band of the profile off it"""
        if axis == "depth" and (nbins is None or dz is None):
            raise ValueError("axis='depth' needs nbins and dz")
        rq = self._profile_request([name], axis, origin, nbins, z0, dz)
        return self.weighted_profile_histogram_raw(rq, hist_bins(nvbins, v0, dv), -1 if group is None else int(group))

    def weighted_covariance_raw(self, slots, group=-1):
        """samsim_get_weighted_covariance with the arguments as given (no checks on this side): (count, sum_w, sum_w2, mean [nslots],
        cov [nslots, nslots])"""
        slots = [int(x) for x in slots]
        n = len(slots)
        arr = (C.c_int32 * max(1, n))(*slots)
        count, sum_w, sum_w2 = C.c_int64(0), C.c_double(0.0), C.c_double(0.0)
        m = max(1, min(n, SENS_MAX_SLOTS))
        mean, cov = np.zeros(m), np.zeros((m, m))
        self._chk(self._f("get_weighted_covariance")(self._h, n, arr, int(group), C.byref(count), C.byref(sum_w), C.byref(sum_w2),
                                                     mean.ctypes.data, cov.ctypes.data), "get_weighted_covariance")
        return int(count.value), float(sum_w.value), float(sum_w2.value), mean, cov

    def weighted_covariance(self, names, group=None):
        """(count, sum_w, sum_w2, mean [n], cov [n, n]) of the slots `names` (from SCALARS, "N_active", or ints of track_slot,
        func_slot, score_slot, weight_slot) over the running columns with a positive weight -- with group: of those with that label
        -- (samsim_get_weighted_covariance): weighted means and weighted population covariances, the diagonal the variances of
        weighted_stats; capi.correlation(cov) gives the correlations"""
        return self.weighted_covariance_raw([_slot(n) for n in names], -1 if group is None else int(group))

    # -- the posterior draw: which members to continue from, and how many copies of each
    def resample_raw(self, spec, info=None):
        """samsim_resample with the arguments as given (no checks on this side): spec a ResampleSpec or None, info a ResampleInfo or
        None"""
        self._chk(self._f("resample")(self._h, None if spec is None else C.byref(spec), None if info is None else C.byref(info)),
                  "resample")
        if spec is None:
            self.m_drawn = 0
        elif info is not None:
            self.m_drawn = int(info.m_drawn)

    def resample(self, m, kind="systematic", u0=0.0, seed=0, group=None):
        """draw m members by the weight row over the running columns with a positive weight -- with group: of those with that label
        -- on the device (samsim_resample): "systematic" with the offset u0 in [0, 1), or "stratified" with per-draw offsets from
        `seed`.  offspring() then holds the copies of every column, ancestors() the ascending list of the m ancestors, and
        offspring_slot() is the offspring row wherever a slot is accepted.  Nothing of the ensemble is written.  Returns {"n_pos",
        "m_drawn", "n_survivors", "max_offspring", "argmax_offspring", "sum_w"}; m_drawn is 0 when no weight is positive and finite"""
        info = ResampleInfo()
        self.resample_raw(ResampleSpec.make(m, kind, u0, seed, group), info)
        return {"n_pos": int(info.n_pos), "m_drawn": int(info.m_drawn), "n_survivors": int(info.n_survivors),
                "max_offspring": int(info.max_offspring), "argmax_offspring": int(info.argmax_offspring), "sum_w": info.sum_w}

    def clear_resample(self):
        """remove the offspring row and the ancestor list (samsim_resample with NULL), also when there are none"""
        self.resample_raw(None)

    def offspring(self, col0: int = 0, ncols: int | None = None) -> np.ndarray:
        """float64 [ncols]: the number of offspring of the columns [col0, col0 + ncols) (samsim_get_offspring)"""
        n = self.ncol - col0 if ncols is None else ncols
        buf = np.zeros(max(0, n))
        self._chk(self._f("get_offspring")(self._h, col0, n, buf.ctypes.data), "get_offspring")
        return buf

    def ancestors(self, k0: int = 0, nk: int | None = None) -> np.ndarray:
        """int64 [nk]: the ancestors of the draws [k0, k0 + nk), ascending (samsim_get_ancestors); nk None: up to the last draw of
        the last resample() of this Solver"""
        n = getattr(self, "m_drawn", 0) - k0 if nk is None else nk
        buf = np.zeros(max(1, n), dtype=np.int64)
        self._chk(self._f("get_ancestors")(self._h, k0, n, buf.ctypes.data), "get_ancestors")
        return buf[:max(0, n)]

    def resampled_columns(self, k0, nk, narr: int = NARR, with_status=False):
        """the state of the ancestors of the draws [k0, k0 + nk), nk at most SELECT_MAX_OUT, position j holding the ancestor of draw
        k0 + j: get_columns of that window of the ancestor list, ready for set_state of this or another Solver"""
        assert 0 <= nk <= SELECT_MAX_OUT
        return self.get_columns(self.ancestors(k0, nk), narr, with_status)

    # -- applying a resample: whole columns copied in place on the device
    def copy_columns_raw(self, n, src, dst, what):
        """samsim_copy_columns with the arguments as given (no checks on this side): src and dst int64 arrays or None"""
        self._chk(self._f("copy_columns")(self._h, int(n), None if src is None else src.ctypes.data, None if dst is None else dst.ctypes.data,
                                          int(what)), "copy_columns")

    def copy_columns(self, src, dst, forcing=False, tracks=False, scores=False):
        """overwrite column dst[k] with column src[k] on the device (samsim_copy_columns): afterwards every getter returns for dst[k]
        what it would after get_columns(src) -> set_state(dst) -> set_status with the source's status, with the tracer amounts, and --
        tracks, scores -- the track and score rows; forcing: also the perturbation slots, the forcing set and the ocean rows.  A dst
        may be listed once and may not be a src; a src may feed many.  The copies take their next step through the restart path"""
        src, dst = np.ascontiguousarray(src, dtype=np.int64), np.ascontiguousarray(dst, dtype=np.int64)
        assert src.ndim == 1 and src.shape == dst.shape
        self.copy_columns_raw(src.size, src, dst, copy_what(forcing, tracks, scores))

    def apply_resample_raw(self, what, info=None):
        """samsim_apply_resample with the arguments as given: info an ApplyInfo or None"""
        self._chk(self._f("apply_resample")(self._h, int(what), None if info is None else C.byref(info)), "apply_resample")
        if info is not None:
            self.n_plan = int(info.n_copies)

    def apply_resample(self, forcing=False, tracks=False, scores=False):
        """put the copies of the last resample() where the dropped members were, on the device (samsim_apply_resample): the columns
        of the pool nobody drew take, in ascending order, the surplus copies of the columns drawn more than once; survivors keep
        their slot.  Needs a draw with m equal to the pool size, and every drawn column still running: else SamsimError -2, and
        nothing is written.  Returns {"n_pool", "n_free", "n_copies", "n_sources"}; copy_plan() then holds the pairs"""
        info = ApplyInfo()
        self.apply_resample_raw(copy_what(forcing, tracks, scores), info)
        return {"n_pool": int(info.n_pool), "n_free": int(info.n_free), "n_copies": int(info.n_copies), "n_sources": int(info.n_sources)}

    def copy_plan(self, k0: int = 0, nk: int | None = None):
        """(src, dst), int64 [nk] each: the entries [k0, k0 + nk) of the plan of the last apply_resample (samsim_get_copy_plan);
        nk None: up to the last entry of the last apply_resample() of this Solver"""
        n = getattr(self, "n_plan", 0) - k0 if nk is None else nk
        src, dst = np.zeros(max(1, n), dtype=np.int64), np.zeros(max(1, n), dtype=np.int64)
        self._chk(self._f("get_copy_plan")(self._h, k0, n, src.ctypes.data, dst.ctypes.data), "get_copy_plan")
        return src[:max(0, n)], dst[:max(0, n)]

    # -- rejuvenation: the per-column parameters jittered on the device, and one assimilation cycle from end to end
    def get_ocean(self, col0: int = 0, ncols: int | None = None, dfl_q_bottom=True, S_bu_bottom=True):
        """(dfl_q_bottom, S_bu_bottom), float64 [ncols] each or None where not asked for: the window of the rows of set_ocean
        (samsim_get_ocean); a row that is asked for and not set is SamsimError -1"""
        n = self.ncol - col0 if ncols is None else ncols
        d = np.zeros(max(0, n)) if dfl_q_bottom else None
        s = np.zeros(max(0, n)) if S_bu_bottom else None
        self._chk(self._f("get_ocean")(self._h, col0, n, None if d is None else d.ctypes.data, None if s is None else s.ctypes.data),
                  "get_ocean")
        return d, s

    def jitter_raw(self, spec, info=None):
        """samsim_jitter with the arguments as given (no checks on this side): spec a JitterSpec or None, info a JitterInfo or None"""
        self._chk(self._f("jitter")(self._h, None if spec is None else C.byref(spec), None if info is None else C.byref(info)), "jitter")

    def jitter(self, terms, which="pool", seed=0, group=None):
        """shrink and jitter the parameter rows the terms (JitterTerm.make) name, on the device (samsim_jitter): row = centre +
        shrink * (row - centre) + sigma * eps within [lo, hi], eps the normal deviate of (seed, column, target).  which="pool": the
        running columns -- with group: of that label --; "copies": the destinations of the last apply_resample that still run.
        Returns {"n_written", "n_lo" [nterms], "n_hi" [nterms]}"""
        terms = list(terms)
        info = JitterInfo()
        self.jitter_raw(JitterSpec.make(terms, which, seed, group), info)
        return info.as_dict(len(terms))

    def rejuvenate(self, targets, delta=0.98, seed=0, which="pool", group=None, bounds=None):
        """Liu and West's kernel shrinkage of the parameter rows `targets` (names from JITTER_TARGETS): mean and variance of each
        row over the pool (one covariance call on their slots), then one jitter with centre = mean, shrink = a and sigma = h *
        sqrt(var), (a, h) = liu_west(delta), so the pool keeps its mean and variance while equal members part.  bounds: {target:
        (lo, hi)}.  Returns the jitter's info with the moments used: "count", "mean" and "var" [ntargets], "a" and "h" """
        targets = [JITTER_TARGETS[t] if isinstance(t, (int, np.integer)) else t for t in targets]
        a, h = liu_west(delta)
        count, mean, cov = self.covariance_raw([jitter_slot(t) for t in targets], -1 if group is None else int(group))
        var = np.diag(cov)[:len(targets)].copy()
        bounds = bounds or {}
        free = {t: ((0.0 if t == "S_bu_bottom" else -np.inf), np.inf) for t in targets}     # a salinity below is never negative
        terms = [JitterTerm.make(t, mean[i], a, h * float(np.sqrt(max(var[i], 0.0))), *bounds.get(t, free[t]))
                 for i, t in enumerate(targets)]
        info = self.jitter(terms, which, seed, group)
        info.update(count=count, mean=mean[:len(targets)].copy(), var=var, a=a, h=h)
        return info

    def assimilate(self, obs, weight=None, scale=1.0, ess_frac=0.5, seed=0, targets=("dT2m",), delta=0.98, tracks=False):
        """one assimilation cycle of the whole handle: score the sensors against `obs`, weight the members by the accumulated misfit
        (Gauss, `scale`), and when the effective sample size falls below ess_frac * n_in: a systematic resample of n_in draws, the
        copies put in place with their forcing (and tracks), the targets rejuvenated (rejuvenate with delta) and the scores reset.
        Offset and jitter seed follow from `seed` and the clock's step, so two handles given the same calls hold the same bytes.
        Returns {"ess", "n_in", "resampled", "n_copies", "n_survivors", "jitter"}"""
        self.score(obs, weight)
        w = self.set_weights(score_slot("J_SUM"), "gauss", scale)
        out = {"ess": w["ess"], "n_in": w["n_in"], "resampled": False, "n_copies": 0, "n_survivors": w["n_in"], "jitter": None}
        if w["ess"] < ess_frac * w["n_in"]:
            step = int(self.get_clock().step)
            r = self.resample(w["n_in"], "systematic", u0=rs_offset(seed, 2 * step))
            p = self.apply_resample(forcing=True, tracks=tracks)
            out["jitter"] = self.rejuvenate(list(targets), delta, mix64(seed, 2 * step + 1))
            self.reset_scores()
            out.update(resampled=True, n_copies=p["n_copies"], n_survivors=r["n_survivors"])
        return out

    def run_to_output(self) -> Output:
        """advance to (and through) the next output point of mo_grotz.f90:340 and return its snapshot"""
        self.step(self.steps_to_output())
        return self.get_output()

    def close(self):
        if self._h:
            self._f("destroy")(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


HIP_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libsamsim_hip.so")
