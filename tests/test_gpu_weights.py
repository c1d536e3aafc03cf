"""The weight row and the weighted reductions on the GPU (samsim_set_weights, samsim_get_weights, samsim_get_weighted_stats,
samsim_get_weighted_histogram, SAMSIM_WEIGHT_SLOT): the ensemble weighted by its misfit, w ~ exp(-J / 2), and its posterior
statistics reduced on the device.  The oracle is tests/weights_reference.py applied to get_state(), get_status(), the downloaded
score rows and -- for the reductions -- the downloaded weight row of the same handle.

Bars.  The GAUSS row: within 2 ulp of np.exp (the library's exponential is within 1 ulp of exp, numpy's libm within 1 ulp), and bit
for bit the host-compiled header's where gcc is there.  Weighted moments: count, min and max exact, mean at 1e-12 max(1, |mean|), var
at 1e-10 max(1e-3, sd)^2 -- the project's bars for the unweighted moments.  A weighted histogram entry: 1e-12 max(1, entry) against
math.fsum: a wave adds at most 70 x 64 = 4 480 positive terms and the merge 1 024 partials, (4 480 + 1 024) 2^-53 = 6e-13 relative.
Small integer weights (DIRECT on N_active) make every sum exact: those are compared bit for bit."""
import ctypes as C
import math

import numpy as np
import pytest

import samsim_amd
from samsim_amd import capi, testcases as tcs
from samsim_amd.capi import (S, FunctionalSpec, SamsimError, SensorSpec, State, TrackSpec, WeightInfo, WeightSpec, WSTAT_DTYPE, func_slot,
                             score_slot, weight_slot)
from tests import hist_reference as hr
from tests import sens_reference as cr
from tests import weights_reference as wr
from tests.profile_reference import column_thickness
from tests.test_gpu_group_stats import labels_of_test_1
from tests.test_gpu_profile_stats import ensemble, pick_dz

pytestmark = pytest.mark.gpu
LD = np.longdouble
INF, NAN = float("inf"), float("nan")
CORRUPT = (5, 40000, 70000)
MEMBER = 12345                                # the member whose own values are the observations
SLOTS = ["thickness", "T_top", "m_snow", "thick_snow", "bulk_salin", "N_active", "dT2m", "precip_scale"]
mk = SensorSpec.make
# what a buoy carries: a temperature string from the top, two salinity sections, the ice thickness and the snow depth
BUOY = ([mk("profile", "T", 0.1 * i, interp="linear", missing=NAN) for i in range(8)]
        + [mk("profile", "S_bu", z, "bottom", missing=NAN) for z in (0.02, 0.1)] + [mk("ice_thickness"), mk("scalar", "thick_snow")])
J_SUM = score_slot("J_SUM")


def snapshot(g):
    """everything the four calls must leave alone, as bytes"""
    s, (status, step, layer), k = g.get_state(), g.get_status(), g.get_clock()
    try:
        o = g.get_output()
        out = (o.lay.tobytes(), o.scal.tobytes(), o.n_active.tobytes(), o.time, o.step)
    except SamsimError as e:
        assert e.code == -5                   # no output point passed yet: nothing to compare
        out = None
    return dict(lay=s.lay.view(np.uint64).tobytes(), scal=s.scal.view(np.uint64).tobytes(), n_active=s.n_active.tobytes(),
                status=status.tobytes(), err_step=step.tobytes(), err_layer=layer.tobytes(),
                clock=(k.time, k.step, k.n_time_out, k.time_counter, k.n_outputs), work=g.get_work(), output=out,
                tracks={f: r.view(np.uint64).tobytes() for f, r in g.tracks(0).items()},
                functionals=g.functionals(0).view(np.uint64).tobytes(),
                scores={f: r.view(np.uint64).tobytes() for f, r in g.scores().items()})


def scored_ensemble(ncol, corrupt, lab, ngroups, member):
    """the day-200 ensemble tiled over ncol columns, three steps on, with labels, one track, one functional and the buoy's sensors,
    scored once against the values of `member`: a twin experiment"""
    g = ensemble("sheba_ensemble_80.npz", ncol, 0, corrupt=corrupt)
    g.set_output_window(0, 8)
    g.set_tracks([TrackSpec.make("ice_thickness")], 1)
    g.step(3)
    g.set_functionals([FunctionalSpec.make("thickness_where", "psi_l", sense=1, threshold=0.05)])
    g.set_groups(lab, ngroups=ngroups)
    g.set_sensors(BUOY)
    status = g.get_status()[0]
    assert sorted(np.flatnonzero(status)) == list(corrupt) and status[member] == 0
    g.score(g.sensor_values([member])[:, 0])
    return g, status


@pytest.fixture(scope="module")
def big():
    """70 001 columns: 1 094 blocks of 64, more than the grid has waves (1 024), and a ragged tail of 49; three columns stopped;
    the labels of the group statistics' tests (nine groups, -1s, one group of one column, one empty).  The tests set the weight
    row and read reductions; nobody steps it or changes its labels, sensors or score rows."""
    ncol = 70001
    assert (ncol + 63) // 64 > 1024 and ncol % 64 != 0
    lab = labels_of_test_1(ncol)
    g, status = scored_ensemble(ncol, CORRUPT, lab, 11, MEMBER)
    s, rows = g.get_state(), g.scores()
    J = rows["J_SUM"]
    ok = status == 0
    # the tempering of the reduction tests: the median member keeps exp(-1) of the best member's weight
    scale = float(np.median(J[ok & (J > 0.0)])) / 2.0
    assert np.isfinite(scale) and scale > 0.0
    for a in (s.lay, s.scal, s.n_active, status, lab, *rows.values()):
        a.setflags(write=False)
    return dict(g=g, s=s, status=status, lab=lab, rows=rows, scale=scale)


@pytest.fixture(scope="module")
def small():
    """4 197 columns (65 blocks + 37 columns), two of them stopped, labels 0..2 with -1s; one running column's melt_err is a NaN,
    and melt_err is a sensor: that column's J is a NaN"""
    ncol = 4197
    lab = (np.arange(ncol) % 3).astype(np.int32)
    lab[::7] = -1
    g = ensemble("sheba_ensemble_80.npz", ncol, 0, corrupt=(5, 3000))
    g.set_output_window(0, 8)
    g.set_tracks([TrackSpec.make("ice_thickness")], 1)
    g.step(3)
    g.set_functionals([FunctionalSpec.make("thickness_where", "psi_l", sense=1, threshold=0.05)])
    g.set_groups(lab, ngroups=3)
    status = g.get_status()[0]
    assert sorted(np.flatnonzero(status)) == [5, 3000]
    c_nan = 1000
    one = g.get_state(c_nan, 1)
    one.scal[S["melt_err"]] = NAN
    g.set_state(one, c_nan)
    sensors = BUOY + [mk("scalar", "melt_err")]
    g.set_sensors(sensors)
    g.score(g.sensor_values([77])[:, 0])
    s, rows = g.get_state(), g.scores()
    assert np.array_equal(g.get_status()[0], status)
    assert np.isnan(rows["J_SUM"][c_nan]) and np.isnan(rows["J_SUM"]).sum() == 1
    s_rw = State(s.lay.copy(), s.scal.copy(), s.n_active.copy())         # for the profile reference, which borrows an array
    for a in (s.lay, s.scal, s.n_active, status, lab):
        a.setflags(write=False)
    return dict(g=g, s=s, s_rw=s_rw, status=status, lab=lab, rows=rows, c_nan=c_nan)


@pytest.fixture(scope="module")
def same():
    """256 copies of one column (testcase 1: no forcing, so dT2m = 0 and precip_scale = 1 everywhere)"""
    ncol = 256
    cfg, st = tcs.testcase1(ncol)
    g = samsim_amd.hip_solver(cfg, ncol)
    g.set_state(st)
    g.set_clock()
    g.step(4000)
    assert not g.get_status()[0].any()
    return g, g.get_state()


def row_of(s, name):
    return s.n_active.astype(np.float64) if name == "N_active" else s.sc(name)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check_info(info, w, inn, what):
    want = wr.info_of(w, inn)
    print(what, "n_in", info["n_in"], "n_pos", info["n_pos"], "sum_w", info["sum_w"], "ess", info["ess"],
          "| sum errors", abs(info["sum_w"] - want["sum_w"]) / max(want["sum_w"], 1e-300),
          abs(info["sum_w2"] - want["sum_w2"]) / max(want["sum_w2"], 1e-300))
    assert info["n_in"] == want["n_in"] and info["n_pos"] == want["n_pos"] == int((w > 0.0).sum()), what
    assert abs(info["sum_w"] - want["sum_w"]) <= 1e-12 * want["sum_w"] and abs(info["sum_w2"] - want["sum_w2"]) <= 1e-12 * want["sum_w2"], what
    if want["sum_w2"] > 0.0:
        assert info["ess"] == info["sum_w"] * info["sum_w"] / info["sum_w2"]


def check_gauss_row(g, x, status, lab, group, scale, what):
    """the row of GAUSS on the values x against the header's rule; returns (w, info, t)"""
    info = g.set_weights(J_SUM, "gauss", scale, group)
    w = g.weights()
    inn = wr.in_columns(status, lab, group)
    valid = inn & ~np.isnan(x)
    x_min = float(x[valid].min())
    assert info["x_min"] == x_min, what
    assert (w[~inn] == 0.0).all() and (w[inn & np.isnan(x)] == 0.0).all(), what
    c = np.float64(0.5) / np.float64(scale)
    with np.errstate(invalid="ignore"):
        t = (x - x_min) * c
    assert (w[valid & (x == x_min)] == 1.0).all() and (w[valid & (t >= 690.0)] == 0.0).all() and (w[valid & (t < 690.0)] > 0.0).all(), what
    # x_i <= x_j => w_i >= w_j
    order = np.argsort(x[valid], kind="stable")
    assert (np.diff(w[valid][order]) <= 0.0).all(), what
    live = valid & (t < 690.0)
    ref = np.exp(-t[live])
    ulp = np.abs(w[live] - ref) / np.spacing(ref)
    wh, xh, how = wr.gauss_weights(x, inn, scale)
    print(what, "| x_min", x_min, "| worst distance to np.exp", float(ulp.max()), "ulp | compared bit for bit with:", how)
    assert ulp.max() <= 2.0, what
    assert xh == x_min
    if how == "header":
        bad = np.flatnonzero(bits(w) != bits(wh))
        assert bad.size == 0, (what, bad[:8].tolist(), w[bad[:8]].tolist(), wh[bad[:8]].tolist())
    check_info(info, w, inn, what)
    return w, info, t


def check_wstats(got, want, what):
    sd = np.sqrt(want["var"])
    print(what, "count", want["count"].tolist()[:1], "| mean err", float(np.max(np.abs(got["mean"] - want["mean"]) / np.maximum(1.0, np.abs(want["mean"])))),
          "| var err / max(1e-3, sd)^2", float(np.max(np.abs(got["var"] - want["var"]) / np.maximum(1e-3, sd) ** 2)),
          "| sum_w err", float(np.max(np.abs(got["sum_w"] - want["sum_w"]) / np.maximum(want["sum_w"], 1e-300))))
    assert np.array_equal(got["count"], want["count"]), what
    assert bits(got["min"]).tolist() == bits(want["min"]).tolist() and bits(got["max"]).tolist() == bits(want["max"]).tolist(), what
    assert (np.abs(got["mean"] - want["mean"]) <= 1e-12 * np.maximum(1.0, np.abs(want["mean"]))).all(), what
    assert (np.abs(got["var"] - want["var"]) <= 1e-10 * np.maximum(1e-3, sd) ** 2).all(), what
    assert (np.abs(got["sum_w"] - want["sum_w"]) <= 1e-12 * want["sum_w"]).all(), what
    assert (np.abs(got["sum_w2"] - want["sum_w2"]) <= 1e-12 * want["sum_w2"]).all(), what


def as_array(q, names):
    return np.array([tuple(q[n]) for n in names], dtype=WSTAT_DTYPE)


# ------------------------------------------------------------------------------------------------------------ 1: the row
def test_gauss_on_the_misfit_of_a_twin_experiment(big):
    g, status, lab, x, scale = big["g"], big["status"], big["lab"], big["rows"]["J_SUM"], big["scale"]
    copies = np.array([c for c in range(MEMBER % 256, g.ncol, 256) if status[c] == 0])
    assert MEMBER in copies and copies.size > 200 and (x[copies] == 0.0).all()
    assert len(set(x[status == 0].tolist())) > 100                       # the members differ
    for sc in (1.0, scale, 8.0 * scale):
        w, info, _ = check_gauss_row(g, x, status, lab, None, sc, f"every column, scale {sc:g}")
        assert info["x_min"] == 0.0 and (w[copies] == 1.0).all() and (w[list(CORRUPT)] == 0.0).all()
        assert info["n_in"] == g.ncol - 3
    k = int(lab[MEMBER + 256])                                           # a group that holds a copy of the observed member
    assert k >= 0
    w, info, _ = check_gauss_row(g, x, status, lab, k, scale, f"group {k}")
    assert info["x_min"] == 0.0 and (w[lab != k] == 0.0).all() and w[MEMBER + 256] == 1.0 and 0 < info["n_pos"] <= (lab == k).sum()
    w, info, _ = check_gauss_row(g, x, status, lab, 9, scale, "the group of one column")
    assert info["n_in"] == info["n_pos"] == 1 and info["sum_w"] == 1.0 and w[MEMBER] == 1.0 and w.sum() == 1.0
    info = g.set_weights(J_SUM, "gauss", scale, 10)                      # the empty group
    assert (info["n_in"], info["n_pos"], info["x_min"], info["sum_w"], info["sum_w2"], info["ess"]) == (0, 0, 0.0, 0.0, 0.0, 0.0)
    assert not g.weights().any()
    # a window of the row
    g.set_weights(J_SUM, "gauss", scale)
    w = g.weights()
    assert bits(g.weights(60, 200)).tolist() == bits(w[60:260]).tolist() and g.weights(g.ncol, 0).size == 0


def test_gauss_with_a_nan_and_beyond_the_cutoff(small):
    g, status, lab, c_nan = small["g"], small["status"], small["lab"], small["c_nan"]
    x = small["rows"]["J_SUM"]
    ok = status == 0
    finite = x[ok & ~np.isnan(x)]
    scale = float(finite.max() - finite.min()) / (4.0 * 690.0)           # t reaches 2 x 690 at the worst member
    for group in (None, int(lab[c_nan])):
        w, info, t = check_gauss_row(g, x, status, lab, group, scale, f"cutoff, group {group}")
        inn = wr.in_columns(status, lab, group)
        assert w[c_nan] == 0.0 and inn[c_nan]
        with np.errstate(invalid="ignore"):
            gone = inn & (t >= 690.0)
        assert gone.sum() >= 2 and (w[gone] == 0.0).all() and info["n_pos"] == (inn & (t < 690.0)).sum() >= 2


def test_direct(big):
    g, s, status, lab = big["g"], big["s"], big["status"], big["lab"]
    for name in ("N_active", "dT2m", func_slot(0)):
        x = g.functionals(0) if name == func_slot(0) else row_of(s, name)
        for group in (None, 3):
            inn = wr.in_columns(status, lab, group)
            info = g.set_weights(name, "direct", group=group)
            w = g.weights()
            assert bits(w).tolist() == bits(wr.direct_weights(x, inn)).tolist(), (name, group)
            assert info["x_min"] == 0.0 and 0 < info["n_pos"] and info["n_in"] == inn.sum()
            check_info(info, w, inn, f"direct {name}, group {group}")
    assert (row_of(s, "dT2m")[status == 0] <= 0.0).any()                 # DIRECT had something to refuse


def test_direct_with_integer_weights_is_exact(big):
    """N_active as the weight: every partial sum is a small integer, so whatever the order the sums are exact"""
    g, s, status, lab = big["g"], big["s"], big["status"], big["lab"]
    thick = row_of(s, "thickness")
    lo, hi = float(thick[status == 0].min()), float(thick[status == 0].max())
    nv, v0 = 254, lo + 0.02 * (hi - lo)
    dv = 0.9 * (hi - lo) / nv                                            # both outer entries hold columns
    for group in (None, 3):
        inn = wr.in_columns(status, lab, group)
        info = g.set_weights("N_active", "direct", group=group)
        w = g.weights()
        assert info["sum_w"] == float(w.sum()) and info["sum_w2"] == float((w * w).sum()) and float(w.sum()) == float(s.n_active[inn].sum())
        for name, bins in (("thickness", (nv, v0, dv)), ("N_active", (40, 0.5, 1.0)), ("thickness", (1, v0, dv))):
            use = inn & (w > 0.0)
            idx = hr.entries(row_of(s, name)[use], *bins)
            want = np.bincount(idx, weights=w[use], minlength=bins[0] + 2)
            got = g.weighted_histogram(name, *bins, group=group)
            assert bits(got).tolist() == bits(want).tolist(), (name, bins, group)
            assert want[0] > 0 or name == "N_active"
        q = g.weighted_stats(["thickness"], group=group)["thickness"]
        assert q["sum_w"] == info["sum_w"] and q["sum_w2"] == info["sum_w2"] and q["count"] == info["n_pos"]


def test_unit_weights_on_identical_columns(same):
    g, s = same
    info = g.set_weights("precip_scale", "direct")
    assert (g.weights() == 1.0).all() and info["n_pos"] == 256 and info["sum_w"] == 256.0 and info["ess"] == 256.0
    q = g.weighted_stats(SLOTS)
    plain = g.ensemble_stats(SLOTS)
    for name in SLOTS:
        x = float(row_of(s, name)[0])
        assert (row_of(s, name) == x).all()
        assert q[name]["count"] == plain[name].count == 256 and q[name]["sum_w"] == 256.0 and q[name]["sum_w2"] == 256.0
        assert q[name]["mean"] == x and q[name]["var"] == 0.0 and q[name]["min"] == x and q[name]["max"] == x, name
        bins = (16, x - 0.8, 0.1) if name != "N_active" else (40, 0.5, 1.0)
        counts = g.histogram(name, *bins)
        assert counts.sum() == 256 and bits(g.weighted_histogram(name, *bins)).tolist() == bits(counts.astype(np.float64)).tolist(), name
    # a GAUSS row on equal values: every weight is exactly 1
    info = g.set_weights("thickness", "gauss", 0.5)
    assert (g.weights() == 1.0).all() and info["x_min"] == float(row_of(s, "thickness")[0])


# ------------------------------------------------------------------------------------------------------------ 2: the moments
def test_weighted_stats_against_the_reference(big):
    g, s, status, lab, x, scale = big["g"], big["s"], big["status"], big["lab"], big["rows"]["J_SUM"], big["scale"]
    info = g.set_weights(J_SUM, "gauss", scale)
    w = g.weights()
    print("posterior of the twin experiment: n_pos", info["n_pos"], "ess", info["ess"])
    assert info["n_pos"] >= 2
    k = int(lab[MEMBER + 256])
    for group in (None, k, 9, 10):
        inn = wr.in_columns(status, lab, group)
        want = wr.weighted_moments([row_of(s, n) for n in SLOTS], w, inn)
        got = as_array(g.weighted_stats(SLOTS, group=group), SLOTS)
        if group == 10:                                                  # nothing counts: all zeros
            assert got.tobytes() == np.zeros(len(SLOTS), dtype=WSTAT_DTYPE).tobytes()
            continue
        check_wstats(got, want, f"8 slots, group {group}")
        if group in (None, k):
            assert want["count"][0] >= 2 and want["var"][0] > 0.0        # the thickness has a posterior spread
        if group == 9:                                                   # one column: its values, and no variance
            assert got["count"].tolist() == [1] * 8 and (got["var"] == 0.0).all()
            assert bits(got["mean"]).tolist() == bits(np.array([row_of(s, n)[MEMBER] for n in SLOTS])).tolist()
    # the weighting matters: the posterior mean is not the prior's
    assert g.weighted_stats(["thickness"])["thickness"]["mean"] != g.ensemble_stats(["thickness"])["thickness"].mean
    # rows of other kinds as slots: a functional, a score row, the weight row itself
    names = [func_slot(0), J_SUM, weight_slot(), "thickness"]
    rows = [g.functionals(0), x, w, row_of(s, "thickness")]
    inn = wr.in_columns(status)
    check_wstats(as_array(g.weighted_stats(names), names), wr.weighted_moments(rows, w, inn), "functional, score and weight rows")
    # two calls, the same bytes; one slot alone, the bytes it had among eight
    a, b = as_array(g.weighted_stats(SLOTS, group=k), SLOTS), as_array(g.weighted_stats(SLOTS, group=k), SLOTS)
    assert a.tobytes() == b.tobytes()
    assert as_array(g.weighted_stats(["bulk_salin"], group=k), ["bulk_salin"]).tobytes() == a[4:5].tobytes()


def test_zero_one_weights_count_what_select_counts(small):
    """after a score restricted to one group CALLS is 1 in the scored columns and 0 elsewhere: DIRECT on it is a 0/1 row, and the
    weighted count is the selection's n_match"""
    g, s, status, lab = small["g"], small["s"], small["status"], small["lab"]
    keep = g.scores()
    try:
        g.reset_scores()
        g.score(g.sensor_values([77])[:, 0], group=1)
        info = g.set_weights(score_slot("CALLS"), "direct")
        w = g.weights()
        member = (status == 0) & (lab == 1)
        assert bits(w).tolist() == bits(member.astype(np.float64)).tolist() and info["n_pos"] == member.sum() > 1000
        idx, n_match = g.select([(score_slot("CALLS"), 0.5, INF)])
        assert n_match == member.sum() and np.array_equal(idx, np.flatnonzero(member))
        got = as_array(g.weighted_stats(SLOTS), SLOTS)
        assert (got["count"] == n_match).all() and (got["sum_w"] == float(n_match)).all()
        # with unit weights the moments are the unweighted ones of that group
        cnt, mean, cov = g.covariance(SLOTS, group=1)
        assert cnt == n_match and (np.abs(got["mean"] - mean) <= 1e-12 * np.maximum(1.0, np.abs(mean))).all()
        assert (np.abs(got["var"] - np.diag(cov)) <= 1e-10 * np.maximum(1e-3, np.sqrt(np.diag(cov))) ** 2).all()
    finally:
        g.set_score_state(keep)
    assert all(bits(a).tolist() == bits(b).tolist() for a, b in zip(g.scores().values(), keep.values()))


# ------------------------------------------------------------------------------------------------------------ 3: the histogram
def test_weighted_histogram_against_fsum(big):
    g, s, status, lab, scale = big["g"], big["s"], big["status"], big["lab"], big["scale"]
    k = int(lab[MEMBER + 256])
    for group in (None, k):
        info = g.set_weights(J_SUM, "gauss", scale, group)
        w = g.weights()
        inn = wr.in_columns(status, lab, group)
        for name in ("thickness", "T_top", "N_active"):
            v = row_of(s, name)
            lo, hi = float(v[inn].min()), float(v[inn].max())
            bins = (40, 0.5, 1.0) if name == "N_active" else (37, lo + 0.03 * (hi - lo), 0.9 * (hi - lo) / 37)
            want = wr.weighted_histogram(v, w, inn, *bins)
            got = g.weighted_histogram(name, *bins, group=group)
            print(name, "group", group, "| worst entry error / bar", float(np.max(np.abs(got - want) / (1e-12 * np.maximum(1.0, want)))),
                  "| entries with weight", int((want > 0).sum()))
            assert (np.abs(got - want) <= 1e-12 * np.maximum(1.0, want)).all(), (name, group)
            assert (got[want == 0.0] == 0.0).all() and ((want > 0).sum() >= 3 or name == "N_active")
            total = math.fsum(got)
            assert abs(total - info["sum_w"]) <= 1e-12 * max(1.0, info["sum_w"]), (name, group)
            assert bits(g.weighted_histogram(name, *bins, group=group)).tolist() == bits(got).tolist()
            if name == "N_active":
                continue
            # the posterior median and the 5-95 % bracket
            for q in (0.05, 0.5, 0.95):
                blo, bhi = capi.weighted_quantile_bracket(got, bins[1], bins[2], q)
                x = wr.weighted_quantile(v, w, inn, q)
                assert blo <= x < bhi, (name, group, q, blo, x, bhi)


# ------------------------------------------------------------------------------------------------------------ 4: the slot
def test_the_weight_row_as_a_slot(small):
    g, s, status, lab = small["g"], small["s"], small["status"], small["lab"]
    x = small["rows"]["J_SUM"]
    ok = status == 0
    finite = x[ok & ~np.isnan(x)]
    scale = float(np.median(finite[finite > 0.0])) / 2.0
    info = g.set_weights(J_SUM, "gauss", scale)
    w = g.weights()
    ws = weight_slot()
    # the histogram of the weights
    want = hr.scalar_histogram_reference(w, status, 20, 0.0, 0.05)
    assert np.array_equal(g.histogram(ws, 20, 0.0, 0.05), want) and (want > 0).sum() >= 3
    assert np.array_equal(g.histogram(ws, 20, 0.0, 0.05, by_group=True), hr.scalar_histogram_reference(w, status, 20, 0.0, 0.05, lab, 3))
    # the members that carry the posterior
    idx, n = g.select([(ws, 0.01, INF)])
    assert np.array_equal(idx, np.nonzero(ok & (w >= 0.01))[0]) and 0 < n < ok.sum()
    st = g.ensemble_stats([ws])[ws]
    assert st.count == ok.sum() and st.max == 1.0 and st.min == 0.0
    # the posterior mean of a depth bin from the regression on the weight
    nbins = 12
    dz = pick_dz(column_thickness(s)[ok], (0.07, 0.05, 0.09, 0.11), nbins, (0.0,))
    assert dz is not None
    kw = dict(axis="depth", origin="top", nbins=nbins, z0=0.0, dz=dz)
    names = ["T", "S_bu"]
    q = g.profile_regression(names, ws, **kw)
    bins = cr.bin_values(small["s_rw"], status, names, **kw)
    checked = 0
    for name in names:
        got = capi.weighted_profile_mean(q[name])
        for b, (cols, v) in enumerate(bins[name]):
            assert q[name]["count"][b] == cols.size
            wb = w[cols].astype(LD)
            if not cols.size or not float(wb.sum()) > 0.0:                # no column, or no weight, in the bin
                assert got[b] == 0.0
                continue
            want = float((wb * v.astype(LD)).sum() / wb.sum())
            _, mx, my, vx, vy, _ = cr.pair_moments(w[cols], v)
            bar = 1e-12 * max(1.0, abs(float(my))) + 1e-10 * max(1e-3, math.sqrt(float(vx))) * max(1e-3, math.sqrt(float(vy))) / float(mx)
            print(name, "bin", b, "posterior mean", want, "err / bar", abs(got[b] - want) / bar)
            assert abs(got[b] - want) <= bar, (name, b, got[b], want, bar)
            checked += 1
    assert checked >= 8
    assert info["n_pos"] >= 2


# ------------------------------------------------------------------------------------------------------------ 5: isolation
def test_the_calls_are_deterministic_and_write_nothing_else(small):
    g, s, status, lab = small["g"], small["s"], small["status"], small["lab"]
    x = small["rows"]["J_SUM"]
    ok = status == 0
    finite = x[ok & ~np.isnan(x)]
    scale = float(np.median(finite[finite > 0.0])) / 2.0
    g.clear_weights()
    before = snapshot(g)

    def everything(group):
        info = g.set_weights(J_SUM, "gauss", scale, group)
        names = SLOTS[:7] + [func_slot(0)]
        return (tuple(sorted(info.items())), g.weights().tobytes(), as_array(g.weighted_stats(names, group=group), names).tobytes(),
                g.weighted_histogram("thickness", 30, 0.5, 0.1, group=group).tobytes())
    first = {group: everything(group) for group in (None, 1)}
    assert snapshot(g) == before
    assert {group: everything(group) for group in (None, 1)} == first
    # relabelling the columns outside group 1 changes nothing of group 1's results
    other = lab.copy()
    other[lab != 1] = np.where(lab[lab != 1] == 0, 2, -1)
    try:
        g.set_groups(other, ngroups=3)
        assert everything(1) == first[1]
    finally:
        g.set_groups(lab, ngroups=3)
    # a second call replaces the row
    g.set_weights("N_active", "direct")
    assert bits(g.weights()).tolist() == bits(wr.direct_weights(row_of(s, "N_active"), ok)).tolist()
    # clearing frees the slot: a consumer then answers SAMSIM_ERR_ARG, and so do the calls that need the row
    g.clear_weights()
    g.clear_weights()                                                    # also when none is set
    for call in (lambda: g.histogram(weight_slot(), 4, 0.0, 0.25), lambda: g.select([(weight_slot(), 0.5, INF)]),
                 lambda: g.ensemble_stats([weight_slot()]), lambda: g.weights(), lambda: g.weighted_stats(["thickness"]),
                 lambda: g.weighted_histogram("thickness", 4, 0.0, 1.0)):
        with pytest.raises(SamsimError) as e:
            call()
        assert e.value.code == -1
    assert snapshot(g) == before


def test_every_number_of_slots_gives_the_leading_block_of_eight(small):
    """Every instantiation of the two walks over a list of slots, 1 to 8 slots: the first k slots alone return the records of
    weighted_stats and count, sums, mean[:k] and cov[:k, :k] of weighted_covariance of the call with all eight, byte for byte.
    4 197 columns are 66 waves, so a lane of the merge takes two waves and the lanes 33 to 63 none; the last block has 37 columns."""
    g, x, ok = small["g"], small["rows"]["J_SUM"], small["status"] == 0
    finite = x[ok & ~np.isnan(x)]
    g.set_weights(J_SUM, "gauss", float(np.median(finite[finite > 0.0])) / 2.0)
    try:
        for group in (None, 1):
            st8 = as_array(g.weighted_stats(SLOTS, group=group), SLOTS)
            n8, sw8, sw28, mean8, cov8 = g.weighted_covariance(SLOTS, group=group)
            assert n8 > 100 and st8["count"].min() == n8 and (np.diag(cov8)[:5] > 0.0).all()
            for k in range(1, 9):
                st = as_array(g.weighted_stats(SLOTS[:k], group=group), SLOTS[:k])
                assert all(st[i].tobytes() == st8[i].tobytes() for i in range(k)), (group, k)
                n, sw, sw2, mean, cov = g.weighted_covariance(SLOTS[:k], group=group)
                assert (n, sw, sw2) == (n8, sw8, sw28) and mean.tobytes() == mean8[:k].tobytes(), (group, k)
                assert cov.tobytes() == np.ascontiguousarray(cov8[:k, :k]).tobytes(), (group, k)
    finally:
        g.clear_weights()


def test_a_second_trip_and_sixteen_waves_a_lane_are_deterministic(big):
    """70 001 columns are 1 094 blocks on a grid of 1 024 waves: 70 waves take a second block, and a lane of every merge takes 16
    waves.  Two consecutive calls over all columns return the same bytes (the group statistics and the covariances assert theirs
    on such a handle in tests/test_gpu_group_stats.py and tests/test_gpu_sens.py)."""
    g, scale = big["g"], big["scale"]

    def everything():
        info = g.set_weights(J_SUM, "gauss", scale)
        n, sw, sw2, mean, cov = g.weighted_covariance(SLOTS)
        return (tuple(sorted(info.items())), g.weights().tobytes(), as_array(g.weighted_stats(SLOTS), SLOTS).tobytes(),
                g.weighted_histogram("thickness", 254, 0.5, 0.01).tobytes(), n, sw, sw2, mean.tobytes(), cov.tobytes(),
                g.histogram("thickness", 254, 0.5, 0.01).tobytes(), g.histogram("T_top", 40, -30.0, 1.0, by_group=True).tobytes())
    first = everything()
    assert first[0] and dict(first[0])["n_pos"] > 1000 and first[4] > 1000
    assert everything() == first


def test_the_row_outlives_steps_and_uploads():
    """stepping, set_state, set_status and set_clock leave the row alone"""
    ncol = 300
    cfg, st = tcs.testcase1(ncol)
    g = samsim_amd.hip_solver(cfg, ncol)
    g.set_state(st)
    g.set_clock()
    g.step(50)
    g.set_weights("N_active", "direct")
    w = g.weights()
    assert (w > 0.0).all()
    g.step(50)
    g.set_state(g.get_state(0, 10), 0)
    g.set_status(np.array([7], dtype=np.int32), col0=3)
    g.set_clock()
    assert g.weights().tobytes() == w.tobytes()
    info = g.set_weights("N_active", "direct")                           # the stopped column is no longer IN
    assert info["n_in"] == ncol - 1 and g.weights()[3] == 0.0
    g.close()


# ------------------------------------------------------------------------------------------------------------ 6: refusals
def test_refusals_in_the_documented_order(small):
    g, s, status, lab = small["g"], small["s"], small["status"], small["lab"]
    g.set_weights("N_active", "direct")
    row = g.weights()

    def refused(code, call):
        with pytest.raises(SamsimError) as e:
            call()
        assert e.value.code == code, (e.value.code, code)
        assert g.weights().tobytes() == row.tobytes()                    # the previous row is still in force

    def spec(**kw):
        sp = WeightSpec.make(J_SUM, "gauss", 2.0, 1)
        for k, v in kw.items():
            setattr(sp, k, v)
        return sp
    info = WeightInfo(-7, -7, -77.0, -77.0, -77.0)
    refused(-1, lambda: g.set_weights_raw(None, info))                   # NULL spec asks for removal: no info then
    refused(-6, lambda: g.set_weights_raw(spec(struct_size=28, kind=5), info))   # the size comes before the kind
    refused(-1, lambda: g.set_weights_raw(spec(kind=2), info))
    refused(-1, lambda: g.set_weights_raw(spec(kind=-1), info))
    for slot in (0x50000, weight_slot(), capi.NSCAL, -2, func_slot(1), score_slot(capi.NSF), capi.track_slot(1, 0)):
        refused(-1, lambda: g.set_weights_raw(spec(slot=slot), info))
    for group in (3, -2, 99):
        refused(-1, lambda: g.set_weights_raw(spec(group=group), info))
    refused(-1, lambda: g.set_weights_raw(spec(kind=0, scale=2.0), info))        # DIRECT takes no scale
    for scale in (0.0, -1.0, INF, NAN):
        refused(-1, lambda: g.set_weights_raw(spec(scale=scale), info))
    refused(-1, lambda: g.set_weights_raw(spec(reserved=1.0), info))
    assert (info.n_in, info.n_pos, info.x_min, info.sum_w, info.sum_w2) == (-7, -7, -77.0, -77.0, -77.0)
    g.set_weights_raw(spec(), None)                                      # the spec itself is good; info may be NULL
    row = g.weights()
    assert (row[lab != 1] == 0.0).all() and (row > 0.0).any()
    # samsim_get_weights
    buf = np.full(8, -77.0)
    raw = g._f("get_weights")
    assert raw(g._h, 0, 8, None) == -1
    for col0, n in ((-1, 4), (0, -1), (g.ncol - 3, 4), (g.ncol + 1, 0), (0, g.ncol + 1)):
        assert raw(g._h, col0, n, buf.ctypes.data) == -1, (col0, n)
    assert (buf == -77.0).all()
    # samsim_get_weighted_stats
    out = np.full(9 * 7, -77.0)
    raw = g._f("get_weighted_stats")
    one = (C.c_int32 * 9)(*([S["thickness"]] * 9))
    assert raw(g._h, 1, None, -1, out.ctypes.data) == -1 and raw(g._h, 1, one, -1, None) == -1
    assert raw(g._h, 0, one, -1, out.ctypes.data) == -1 and raw(g._h, 9, one, -1, out.ctypes.data) == -1
    bad = (C.c_int32 * 2)(S["thickness"], 0x50000)
    assert raw(g._h, 2, bad, -1, out.ctypes.data) == -1
    for group in (3, -2):
        assert raw(g._h, 1, one, group, out.ctypes.data) == -1
    assert (out == -77.0).all()
    assert raw(g._h, 8, one, 2, out.ctypes.data) == 0 and (out[:56] != -77.0).any() and (out[56:] == -77.0).all()
    # samsim_get_weighted_histogram: the checks of samsim_get_histogram first
    out = np.full(260, -77.0)
    raw = g._f("get_weighted_histogram")
    vb = capi.hist_bins(8, 0.0, 0.5)
    assert raw(g._h, 0, None, -1, out.ctypes.data) == -1 and raw(g._h, 0, C.byref(vb), -1, None) == -1
    wrong = capi.hist_bins(0, 0.0, 0.5)
    wrong.struct_size = 20
    assert raw(g._h, 0x50000, C.byref(wrong), -1, out.ctypes.data) == -6        # the size comes before the bins and the slot
    for nv, v0, dv in ((0, 0.0, 0.5), (255, 0.0, 0.5), (8, NAN, 0.5), (8, 0.0, INF), (8, 0.0, 0.0), (8, 0.0, -1.0), (8, 1e300, 1e-300)):
        assert raw(g._h, 0, C.byref(capi.hist_bins(nv, v0, dv)), -1, out.ctypes.data) == -1, (nv, v0, dv)
    assert raw(g._h, 0x50000, C.byref(vb), -1, out.ctypes.data) == -1
    for group in (3, -2):
        assert raw(g._h, 0, C.byref(vb), group, out.ctypes.data) == -1
    assert (out == -77.0).all()
    assert raw(g._h, 0, C.byref(capi.hist_bins(254, 0.0, 0.5)), 2, out.ctypes.data) == 0 and (out[256:] == -77.0).all()
    assert g.weights().tobytes() == row.tobytes()
    # without labels a group is refused, -1 is not
    g.set_groups(None)
    try:
        refused(-1, lambda: g.set_weights(J_SUM, "gauss", 2.0, 0))
        refused(-1, lambda: g.weighted_stats(["thickness"], group=0))
        refused(-1, lambda: g.weighted_histogram("thickness", 8, 0.0, 0.5, group=0))
        assert g.weighted_stats(["thickness"])["thickness"]["count"] == (row > 0.0).sum()
    finally:
        g.set_groups(lab, ngroups=3)
