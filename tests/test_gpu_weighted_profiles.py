"""Weighted profile statistics and weighted covariances on the GPU (samsim_get_weighted_profile_stats,
samsim_get_weighted_covariance): the posterior profile with its spread and the posterior sensitivities, reduced on the device with
the weight row of samsim_set_weights.  The oracle is tests/weighted_profile_reference.py applied to get_state(), get_status(), the
labels and the downloaded weight row of the same handle.

Bars, the project's own.  count, min and max exact (by depth a bin value is one IEEE division per column of sums the reference forms
in the device's order); mean at 1e-12 max(1, |mean|); var at 1e-10 max(1e-3, sd)^2; sum_w and sum_w2 at 1e-12 relative against
math.fsum -- a bin's sum passes through at most 64 additions in a block, 69 merges in a wave and 1 024 across the waves, all of
positive terms: 1 157 x 2^-53 = 1.3e-13 relative --; covariances at 1e-10 sx sy with sx = max(1e-3, sd_x).  With unit weights the
results are compared with the unweighted calls bit for bit."""
import ctypes as C
import math

import numpy as np
import pytest

import samsim_amd
from samsim_amd import capi, testcases as tcs
from samsim_amd.capi import S, SamsimError, SensorSpec, State, WSTAT_DTYPE, func_slot, score_slot, weight_slot
from tests import sens_reference as cr
from tests import weighted_profile_reference as wpr
from tests.profile_reference import column_thickness
from tests.test_gpu_group_stats import labels_of_test_1
from tests.test_gpu_profile_stats import ensemble, pick_dz
from tests.test_gpu_weights import BUOY, CORRUPT, J_SUM, MEMBER, SLOTS, bits, row_of, scored_ensemble, snapshot

pytestmark = pytest.mark.gpu
INF, NAN = float("inf"), float("nan")
NAMES = ["T", "S_bu", "psi_l", "thick"]
ZERO = np.zeros((), dtype=WSTAT_DTYPE).tobytes()


@pytest.fixture(scope="module")
def big():
    """70 001 columns x 80 layers: 1 094 blocks of 64, more than the grid has waves (1 024), and a ragged tail of 49; three columns
    stopped; eleven labels with -1s, one group of one column, one empty; GAUSS weights on the accumulated misfit of a twin
    experiment, tempered so that the median member keeps exp(-1) of the best member's weight.  The tests read reductions; a test
    that sets another weight row puts this one back."""
    ncol = 70001
    assert (ncol + 63) // 64 > 1024 and ncol % 64 == 49
    lab = labels_of_test_1(ncol)
    g, status = scored_ensemble(ncol, CORRUPT, lab, 11, MEMBER)
    s, rows = g.get_state(), g.scores()
    J = rows["J_SUM"]
    ok = status == 0
    scale = float(np.median(J[ok & (J > 0.0)])) / 2.0
    assert np.isfinite(scale) and scale > 0.0
    info = g.set_weights(J_SUM, "gauss", scale)
    w = g.weights()
    print("posterior of the twin experiment: n_in", info["n_in"], "n_pos", info["n_pos"], "ess", info["ess"])
    assert info["n_in"] == ncol - 3 and info["ess"] >= info["n_in"] / 10.0      # not three members
    assert len(set(w[ok].tolist())) > 100                                        # the weights differ
    H = column_thickness(s)
    for a in (s.lay, s.scal, s.n_active, status, lab, w, H):
        a.setflags(write=False)
    s_rw = State(s.lay.copy(), s.scal.copy(), s.n_active.copy())                 # for bin_values, which borrows an array
    return dict(g=g, s=s, s_rw=s_rw, status=status, lab=lab, w=w, scale=scale, H=H, rows=rows)


@pytest.fixture(scope="module")
def small():
    """4 197 columns (65 blocks + 37 columns), two of them stopped, labels 0..2 with -1s; one running column's misfit is a NaN, so
    its weight is 0"""
    ncol = 4197
    lab = (np.arange(ncol) % 3).astype(np.int32)
    lab[::7] = -1
    g = ensemble("sheba_ensemble_80.npz", ncol, 0, corrupt=(5, 3000))
    g.set_output_window(0, 8)
    g.set_tracks([capi.TrackSpec.make("ice_thickness")], 1)
    g.step(3)
    g.set_functionals([capi.FunctionalSpec.make("thickness_where", "psi_l", sense=1, threshold=0.05)])
    g.set_groups(lab, ngroups=3)
    status = g.get_status()[0]
    assert sorted(np.flatnonzero(status)) == [5, 3000]
    c_nan = 1000
    one = g.get_state(c_nan, 1)
    one.scal[S["melt_err"]] = NAN
    g.set_state(one, c_nan)
    g.set_sensors(BUOY + [SensorSpec.make("scalar", "melt_err")])
    g.score(g.sensor_values([77])[:, 0])
    s, J = g.get_state(), g.scores()["J_SUM"]
    assert np.isnan(J[c_nan]) and np.isnan(J).sum() == 1
    finite = J[(status == 0) & ~np.isnan(J)]
    scale = float(np.median(finite[finite > 0.0])) / 2.0
    info = g.set_weights(J_SUM, "gauss", scale)
    w = g.weights()
    assert w[c_nan] == 0.0 and status[c_nan] == 0 and info["n_pos"] >= 100
    s_rw = State(s.lay.copy(), s.scal.copy(), s.n_active.copy())
    for a in (s.lay, s.scal, s.n_active, status, lab, w):
        a.setflags(write=False)
    return dict(g=g, s=s, s_rw=s_rw, status=status, lab=lab, w=w, scale=scale, c_nan=c_nan)


@pytest.fixture(scope="module")
def same():
    """256 copies of one column (testcase 1), with weights that differ: the columns with label 1 are scored twice, the others
    once, and DIRECT on CALLS makes the row 2.0 and 1.0"""
    ncol = 256
    cfg, st = tcs.testcase1(ncol)
    g = samsim_amd.hip_solver(cfg, ncol)
    g.set_state(st)
    g.set_clock()
    g.step(4000)
    assert not g.get_status()[0].any()
    lab = (np.arange(ncol) % 5 == 1).astype(np.int32)
    g.set_groups(lab, ngroups=2)
    g.set_sensors([SensorSpec.make("ice_thickness")])
    obs = g.sensor_values([0])[:, 0]
    g.score(obs)
    g.score(obs, group=1)
    g.set_weights(score_slot("CALLS"), "direct")
    w = g.weights()
    assert bits(w).tolist() == bits(np.where(lab == 1, 2.0, 1.0)).tolist()
    return g, g.get_state(), lab, w


def depth_request(H_ok, nbins=70):
    """nbins depth bins of which the last four lie below (above) every column: nbins - 4 bins reach the thickest one"""
    base = float(H_ok.max()) / (nbins - 4)
    dz = pick_dz(H_ok, (base, 1.01 * base, 0.99 * base, 1.02 * base), nbins, (0.0,))
    assert dz is not None and nbins * dz > H_ok.max()
    return dict(axis="depth", nbins=nbins, z0=0.0, dz=dz)


def check_profile(got, want, what):
    """every bin of the request; an empty bin is all zeros"""
    sd = np.sqrt(want["var"])
    full = want["count"] > 0
    rel = lambda a, b: np.abs(a - b) / np.maximum(np.abs(b), 1e-300)
    print(what, "count", int(want["count"].min()), "..", int(want["count"].max()), "| empty bins", int((~full).sum()),
          "| mean err", float(np.max(np.abs(got["mean"] - want["mean"]) / np.maximum(1.0, np.abs(want["mean"])))),
          "| var err / max(1e-3, sd)^2", float(np.max(np.abs(got["var"] - want["var"]) / np.maximum(1e-3, sd) ** 2)),
          "| sum_w, sum_w2 err", float(np.max(rel(got["sum_w"], want["sum_w"])[full], initial=0.0)),
          float(np.max(rel(got["sum_w2"], want["sum_w2"])[full], initial=0.0)),
          "| min/max err", float(np.max(np.abs(got["min"] - want["min"]))), float(np.max(np.abs(got["max"] - want["max"]))))
    assert got.shape == want.shape
    assert np.array_equal(got["count"], want["count"]), what
    for b in np.flatnonzero(~full):
        assert got[b].tobytes() == ZERO, (what, b)
    assert np.array_equal(got["min"], want["min"]) and np.array_equal(got["max"], want["max"]), what
    assert (np.abs(got["mean"] - want["mean"]) <= 1e-12 * np.maximum(1.0, np.abs(want["mean"]))).all(), what
    assert (np.abs(got["var"] - want["var"]) <= 1e-10 * np.maximum(1e-3, sd) ** 2).all(), what
    assert (np.abs(got["sum_w"] - want["sum_w"]) <= 1e-12 * want["sum_w"]).all(), what
    assert (np.abs(got["sum_w2"] - want["sum_w2"]) <= 1e-12 * want["sum_w2"]).all(), what


def against_reference(f, requests):
    """every (request, arrays, groups) against the reference, every bin of it; returns how many bins were empty and how many held a
    strict subset of the counting columns"""
    g, status, lab, w = f["g"], f["status"], f["lab"], f["w"]
    empty = subset = 0
    for kw, names, groups in requests:
        bins = cr.bin_values(f["s_rw"], status, names, **kw)
        for group in groups:
            ok = wpr.counting(status, w, lab, group)
            got = g.weighted_profile_stats(names, group=group, **kw)
            for name in names:
                want, who = wpr.from_bins(bins[name], w, ok)
                check_profile(got[name], want, f"{kw['axis']}/{kw['origin']}/{kw['nbins']}/{name}/group {group}")
                empty += int((want["count"] == 0).sum())
                subset += int(((want["count"] > 0) & (want["count"] < ok.sum())).sum())
                if kw["axis"] == "depth":
                    cnt = want["count"]
                    assert (cnt == 0).any() and ((cnt > 0) & (cnt < ok.sum())).any() and cnt.max() == ok.sum(), (kw, name, group)
                    assert kw["nbins"] <= 64 or (cnt[:64].max() > 0 and cnt[64:].max() > 0)     # both chunks hold ice
    return empty, subset


# ------------------------------------------------------------------------------------------------- 1: against the reference
def test_weighted_profile_stats_by_layer_against_the_reference(big):
    """80 layer bins are two chunks of the reduction, 64 + 16; 1 094 blocks are more than the grid's waves"""
    g, lab, w = big["g"], big["lab"], big["w"]
    k = int(lab[MEMBER + 256])
    assert k >= 0
    against_reference(big, [(dict(axis="layer", origin="top", nbins=80), NAMES, (None, k)),
                            (dict(axis="layer", origin="bottom", nbins=80), ["psi_l", "thick"], (k,))])
    # the weighting matters: the posterior profile is not the prior's
    post = g.weighted_profile_stats(["T"], axis="layer", origin="top", nbins=80)["T"]
    prior = g.profile_stats(["T"], axis="layer", origin="top", nbins=80)["T"]
    assert (post["mean"] != prior["mean"]).any() and np.array_equal(post["count"], prior["count"])
    # the group of one column: its values, and no variance; the empty group: all zeros
    one = g.weighted_profile_stats(["T"], axis="layer", origin="top", nbins=80, group=9)["T"]
    assert w[MEMBER] == 1.0 and (one["count"] == 1).all() and (one["var"] == 0.0).all() and (one["sum_w"] == 1.0).all()
    assert bits(one["mean"]).tolist() == bits(big["s"].arr("T")[:, MEMBER]).tolist()
    none = g.weighted_profile_stats(NAMES, group=10, axis="depth", origin="top", nbins=70, dz=0.03)
    assert all(none[n].tobytes() == np.zeros(70, dtype=WSTAT_DTYPE).tobytes() for n in NAMES)


def test_weighted_profile_stats_by_depth_against_the_reference(big):
    """the depth axis on the large ensemble, few bins (the reference forms a [bins, columns] table per layer); more than 64 depth
    bins are compared on the small one below"""
    lab, status = big["lab"], big["status"]
    k = int(lab[MEMBER + 256])
    dq = depth_request(big["H"][status == 0], nbins=16)
    empty, subset = against_reference(big, [(dict(origin="top", **dq), ["S_bu"], (None,)), (dict(origin="bottom", **dq), ["T"], (k,))])
    assert empty > 0 and subset > 0


def test_weighted_profile_stats_with_a_nan_misfit_and_more_than_64_depth_bins(small):
    H = column_thickness(small["s"])[small["status"] == 0]
    dq = depth_request(H)
    assert dq["nbins"] > 64
    groups = (None, int(small["lab"][small["c_nan"]]), 2)
    empty, subset = against_reference(small, [(dict(axis="layer", origin="top", nbins=80), NAMES, groups),
                                              (dict(axis="layer", origin="bottom", nbins=80), NAMES, groups),
                                              (dict(origin="top", **dq), NAMES, groups), (dict(origin="bottom", **dq), NAMES, groups)])
    assert empty > 0 and subset > 0


def test_weighted_covariance_against_the_reference(big):
    g, s, status, lab, w = big["g"], big["s"], big["status"], big["lab"], big["w"]
    k = int(lab[MEMBER + 256])
    names = SLOTS[:6] + [func_slot(0), weight_slot()]
    rows = [row_of(s, n) for n in SLOTS[:6]] + [g.functionals(0), w]
    for group in (None, k, 9, 10):
        ok = cr.counting(status, lab, group)
        rn, rsw, rsw2, rmean, rcov = wpr.weighted_covariance_reference(rows, w, ok)
        n, sw, sw2, mean, cov = g.weighted_covariance(names, group=group)
        if group == 10:                                                          # nothing counts: all zeros
            assert (n, sw, sw2) == (0, 0.0, 0.0) and not mean.any() and not cov.any() and rn == 0
            continue
        rmean, rcov = rmean.astype(np.float64), rcov.astype(np.float64)
        sd = np.maximum(1e-3, np.sqrt(np.diag(rcov)))
        print("group", group, "count", n, "| mean err", float(np.max(np.abs(mean - rmean) / np.maximum(1.0, np.abs(rmean)))),
              "| cov err / (sx sy)", float(np.max(np.abs(cov - rcov) / np.outer(sd, sd))), "| sum errs", abs(sw - rsw) / rsw, abs(sw2 - rsw2) / rsw2)
        assert n == rn == (ok & (w > 0.0)).sum()
        assert abs(sw - rsw) <= 1e-12 * rsw and abs(sw2 - rsw2) <= 1e-12 * rsw2
        assert (np.abs(mean - rmean) <= 1e-12 * np.maximum(1.0, np.abs(rmean))).all(), group
        assert (np.abs(cov - rcov) <= 1e-10 * np.outer(sd, sd)).all(), group
        assert bits(cov).tolist() == bits(cov.T).tolist()
        if group == 9:
            assert n == 1 and not cov.any() and bits(mean).tolist() == bits(np.array([r[MEMBER] for r in rows])).tolist()
    # the weighting matters: the posterior covariance of thickness and dT2m is not the prior's
    _, _, _, _, post = g.weighted_covariance(["thickness", "dT2m"])
    _, _, prior = g.covariance(["thickness", "dT2m"])
    assert post[0, 1] != prior[0, 1] and post[0, 0] > 0.0
    r = capi.correlation(post)
    assert r[0, 0] == 1.0 and abs(r[0, 1]) <= 1.0


# ------------------------------------------------------------------------------------------------- 2: unit weights, byte for byte
def test_unit_weights_are_the_unweighted_call_byte_for_byte(big):
    g, status, lab, scale = big["g"], big["status"], big["lab"], big["scale"]
    dq = depth_request(big["H"][status == 0])
    requests = [dict(axis="layer", origin=o, nbins=80) for o in ("top", "bottom")] + [dict(origin=o, **dq) for o in ("top", "bottom")]
    k = int(lab[MEMBER + 256])
    try:
        for row_group in (None, k):
            info = g.set_weights(score_slot("CALLS"), "direct", group=row_group)
            w = g.weights()
            member = (status == 0) & ((lab == row_group) if row_group is not None else True)
            assert bits(w).tolist() == bits(member.astype(np.float64)).tolist() and info["n_pos"] == member.sum()
            for kw in requests:
                got = g.weighted_profile_stats(NAMES, **kw)                      # group -1: the row alone restricts the columns
                plain = g.profile_stats(NAMES, group=row_group, **kw)
                for n in NAMES:
                    q, p = got[n], plain[n]
                    assert p["count"].max() == member.sum() and (p["count"] == 0).any() or kw["axis"] == "layer"
                    assert np.array_equal(q["count"], p["count"]), (kw, n, row_group)
                    for f in ("mean", "min", "max"):
                        assert bits(q[f]).tolist() == bits(p[f]).tolist(), (kw, n, row_group, f)
                    bad = np.flatnonzero(bits(np.sqrt(q["var"])) != bits(p["std"]))
                    assert bad.size == 0, (kw, n, row_group, bad[:4].tolist(), np.sqrt(q["var"][bad[:4]]).tolist(), p["std"][bad[:4]].tolist())
                    assert bits(q["sum_w"]).tolist() == bits(p["count"].astype(np.float64)).tolist()
                    assert bits(q["sum_w2"]).tolist() == bits(p["count"].astype(np.float64)).tolist()
                if row_group is None:                                            # with labels on top of unit weights: the group call's bytes
                    got = g.weighted_profile_stats(["T", "S_bu"], group=k, **kw)
                    plain = g.profile_stats(["T", "S_bu"], group=k, **kw)
                    for n in ("T", "S_bu"):
                        for f in ("count", "mean", "min", "max"):
                            assert got[n][f].tobytes() == plain[n][f].tobytes(), (kw, n, f)
                        assert bits(np.sqrt(got[n]["var"])).tolist() == bits(plain[n]["std"]).tolist()
    finally:
        g.set_weights(J_SUM, "gauss", scale)
    assert g.weights().tobytes() == big["w"].tobytes()


# ------------------------------------------------------------------------------------------------- 3: the diagonal
def test_the_diagonal_is_the_weighted_moments(big):
    g, lab = big["g"], big["lab"]
    k = int(lab[MEMBER + 256])
    for names in (SLOTS, SLOTS[:5] + [func_slot(0), J_SUM, weight_slot()]):
        for group in (None, k, 9):
            st = g.weighted_stats(names, group=group)
            n, sw, sw2, mean, cov = g.weighted_covariance(names, group=group)
            for i, name in enumerate(names):
                q = st[name]
                assert n == q["count"] and bits(sw) == bits(q["sum_w"]) and bits(sw2) == bits(q["sum_w2"]), (name, group)
                assert bits(mean[i]) == bits(q["mean"]) and bits(cov[i, i]) == bits(q["var"]), (name, group, mean[i], q["mean"], cov[i, i], q["var"])
            # each slot asked for alone keeps its bytes
            for i in (0, 4, 7):
                n1, sw1, sw21, mean1, cov1 = g.weighted_covariance([names[i]], group=group)
                assert (n1, bits(sw1), bits(sw21)) == (n, bits(sw), bits(sw2))
                assert bits(mean1[0]) == bits(mean[i]) and bits(cov1[0, 0]) == bits(cov[i, i])
    # a slot listed twice gives identical rows and columns
    twice = ["thickness", "dT2m", "thickness", "T_top", "dT2m"]
    n, sw, sw2, mean, cov = g.weighted_covariance(twice, group=k)
    assert bits(cov[0, 2]) == bits(cov[0, 0]) == bits(cov[2, 2]) and bits(cov[1, 4]) == bits(cov[1, 1]) == bits(cov[4, 4])
    assert bits(cov[0]).tolist() == bits(cov[2]).tolist() and bits(cov[:, 1]).tolist() == bits(cov[:, 4]).tolist()
    assert bits(mean[0]) == bits(mean[2]) and cov[0, 0] > 0.0 and cov[0, 1] != 0.0
    assert bits(cov).tolist() == bits(cov.T).tolist()


# ------------------------------------------------------------------------------------------------- 4: the regression identity
def test_the_mean_agrees_with_the_regression_on_the_weight(small):
    g, s, status, w = small["g"], small["s"], small["status"], small["w"]
    nbins = 12
    dz = pick_dz(column_thickness(s)[status == 0], (0.07, 0.05, 0.09, 0.11), nbins, (0.0,))
    assert dz is not None
    kw = dict(axis="depth", origin="top", nbins=nbins, z0=0.0, dz=dz)
    names = ["T", "S_bu"]
    reg = g.profile_regression(names, weight_slot(), **kw)
    got = g.weighted_profile_stats(names, **kw)
    bins = cr.bin_values(small["s_rw"], status, names, **kw)
    checked = 0
    for name in names:
        via = capi.weighted_profile_mean(reg[name])
        for b, (cols, v) in enumerate(bins[name]):
            if not cols.size or not float(w[cols].sum()) > 0.0:
                assert via[b] == 0.0 and got[name][b].tobytes() == ZERO
                continue
            _, mx, my, vx, vy, _ = cr.pair_moments(w[cols], v)
            bar = 1e-12 * max(1.0, abs(float(my))) + 1e-10 * max(1e-3, math.sqrt(float(vx))) * max(1e-3, math.sqrt(float(vy))) / float(mx)
            print(name, "bin", b, "posterior mean", got[name]["mean"][b], "difference / bar", abs(got[name]["mean"][b] - via[b]) / bar)
            assert abs(got[name]["mean"][b] - via[b]) <= bar, (name, b, got[name]["mean"][b], via[b], bar)
            assert got[name]["count"][b] == (w[cols] > 0.0).sum() <= reg[name]["count"][b]
            checked += 1
    assert checked >= 8


# ------------------------------------------------------------------------------------------------- 5: identical columns
def test_identical_columns_with_weights_that_differ(same):
    g, s, lab, w = same
    assert set(w.tolist()) == {1.0, 2.0}
    na = int(s.n_active[0])
    H = float(column_thickness(s)[0])
    for kw in (dict(axis="layer", origin="top"), dict(axis="layer", origin="bottom"),
               dict(axis="depth", origin="top", nbins=70, z0=0.0, dz=H / 66.3), dict(axis="depth", origin="bottom", nbins=70, z0=0.0, dz=H / 66.3)):
        for group in (None, 1):
            q = g.weighted_profile_stats(NAMES, group=group, **kw)
            cnt = 256 if group is None else int((lab == 1).sum())
            sw = float(w.sum()) if group is None else 2.0 * cnt
            for n in NAMES:
                full = q[n]["count"] > 0
                assert full.any() and set(q[n]["count"][full].tolist()) == {cnt} and ((~full).any() or kw["axis"] == "layer")
                assert bits(q[n]["mean"]).tolist() == bits(q[n]["min"]).tolist() == bits(q[n]["max"]).tolist(), (kw, n)
                assert (q[n]["var"] == 0.0).all() and (q[n]["sum_w"][full] == sw).all(), (kw, n)
                assert all(q[n][b].tobytes() == ZERO for b in np.flatnonzero(~full))
                if kw["axis"] == "layer":
                    col = s.arr(n)[:na, 0]                                       # the stored values themselves, bit for bit
                    assert bits(q[n]["mean"][:na]).tolist() == bits(col if kw["origin"] == "top" else col[::-1]).tolist() and full.sum() == na
    names = SLOTS + []
    for group in (None, 1):
        n, sw, sw2, mean, cov = g.weighted_covariance(names, group=group)
        assert n == (256 if group is None else (lab == 1).sum()) and not cov.any()
        assert bits(mean).tolist() == bits(np.array([row_of(s, x)[0] for x in names])).tolist()
        assert sw == (float(w.sum()) if group is None else 2.0 * n)


# ------------------------------------------------------------------------------------------------- 6: determinism and purity
def test_the_calls_are_deterministic_and_write_nothing(small):
    g, s, status, lab, w = small["g"], small["s"], small["status"], small["lab"], small["w"]
    dq = depth_request(column_thickness(s)[status == 0])
    before = snapshot(g)
    names = SLOTS[:6] + [func_slot(0), weight_slot()]

    def everything(group):
        out = []
        for kw in (dict(axis="layer", origin="bottom", nbins=80), dict(origin="top", **dq), dict(origin="bottom", **dq)):
            q = g.weighted_profile_stats(NAMES, group=group, **kw)
            out += [q[n].tobytes() for n in NAMES]
        n, sw, sw2, mean, cov = g.weighted_covariance(names, group=group)
        return tuple(out) + (n, sw, sw2, mean.tobytes(), cov.tobytes())
    first = {group: everything(group) for group in (None, 1)}
    assert snapshot(g) == before and g.weights().tobytes() == w.tobytes()
    assert {group: everything(group) for group in (None, 1)} == first
    # relabelling the columns outside group 1 changes nothing of group 1's results
    other = lab.copy()
    other[lab != 1] = np.where(lab[lab != 1] == 0, 2, -1)
    try:
        g.set_groups(other, ngroups=3)
        assert everything(1) == first[1]
    finally:
        g.set_groups(lab, ngroups=3)
    # re-weighting the columns outside group 1 changes nothing of group 1's results: DIRECT on the thickness gives group 1 the
    # same weights with and without the restriction of the row to the group, and the other columns 0.0 or their thickness
    try:
        g.set_weights("thickness", "direct", group=1)
        only = g.weights()
        a = g.weighted_profile_stats(["T", "S_bu"], group=1, origin="top", **dq)
        g.set_weights("thickness", "direct")
        every = g.weights()
        assert bits(every[lab == 1]).tolist() == bits(only[lab == 1]).tolist() and (only[lab != 1] == 0.0).all() and (every[lab != 1] > 0.0).any()
        b = g.weighted_profile_stats(["T", "S_bu"], group=1, origin="top", **dq)
        assert all(a[n].tobytes() == b[n].tobytes() for n in a)
        ca = g.weighted_covariance(SLOTS, group=1)
        g.set_weights("thickness", "direct", group=1)
        cb = g.weighted_covariance(SLOTS, group=1)
        assert ca[:3] == cb[:3] and ca[3].tobytes() == cb[3].tobytes() and ca[4].tobytes() == cb[4].tobytes()
    finally:
        g.set_weights(J_SUM, "gauss", small["scale"])
    assert g.weights().tobytes() == w.tobytes() and snapshot(g) == before


# ------------------------------------------------------------------------------------------------- 7: refusals
def test_refusals_in_the_documented_order(small):
    g, lab, w = small["g"], small["lab"], small["w"]
    PAT = -77.0

    def request(**kw):
        rq = g._profile_request(["T", "S_bu"], "depth", "top", 8, 0.0, 0.1)
        for k, v in kw.items():
            setattr(rq, k, v)
        return rq
    prof, covf = g._f("get_weighted_profile_stats"), g._f("get_weighted_covariance")
    out = np.full(2 * 8 * 7 + 7, PAT)

    def prof_refused(code, rq, group=-1):
        assert prof(g._h, None if rq is None else C.byref(rq), group, out.ctypes.data) == code, (code, group)
        assert (out == PAT).all()
    # -- the profile call: NULLs; every check of samsim_get_profile_stats in its order; no weight row; the group
    prof_refused(-1, None)
    assert prof(g._h, C.byref(request()), -1, None) == -1 and prof(None, C.byref(request()), -1, out.ctypes.data) == -1
    prof_refused(-6, request(struct_size=8, axis=7, nbins=0), 99)                # the size comes before everything else
    prof_refused(-1, request(axis=2, origin=5))
    prof_refused(-1, request(origin=2, nbins=0))
    for nbins in (0, -1, capi.PROFILE_MAX_BINS + 1):
        prof_refused(-1, request(nbins=nbins, narrays=0))
    prof_refused(-1, request(axis=0, nbins=g.nlayer + 1))
    for narrays in (0, capi.PROFILE_MAX_ARRAYS + 1):
        prof_refused(-1, request(narrays=narrays))
    bad = request()
    bad.arrays[1] = capi.NARR
    prof_refused(-1, bad)
    for z0, dz in ((NAN, 0.1), (0.0, INF), (-0.1, 0.1), (0.0, 0.0), (0.0, -1.0)):
        prof_refused(-1, request(z0=z0, dz=dz), 99)
    for group in (3, -2, 99):
        prof_refused(-1, request(), group)
    # -- the covariance call: NULLs; nslots; a bad slot; no weight row; the group
    cnt, sw, sw2 = C.c_int64(-7), C.c_double(PAT), C.c_double(PAT)
    mean, cov = np.full(9, PAT), np.full(82, PAT)
    one = (C.c_int32 * 9)(*([S["thickness"]] * 9))
    args = lambda: [C.byref(cnt), C.byref(sw), C.byref(sw2), mean.ctypes.data, cov.ctypes.data]

    def cov_untouched():
        assert (cnt.value, sw.value, sw2.value) == (-7, PAT, PAT) and (mean == PAT).all() and (cov == PAT).all()
    assert covf(None, 1, one, -1, *args()) == -1 and covf(g._h, 1, None, -1, *args()) == -1
    for i in range(5):
        a = args()
        a[i] = None
        assert covf(g._h, 1, one, -1, *a) == -1, i
    assert covf(g._h, 0, one, -1, *args()) == -1 and covf(g._h, 9, one, -1, *args()) == -1 and covf(g._h, -1, one, -1, *args()) == -1
    for slot in (0x50000, capi.NSCAL, -2, func_slot(1), score_slot(capi.NSF), capi.track_slot(1, 0)):
        assert covf(g._h, 2, (C.c_int32 * 2)(S["thickness"], slot), 99, *args()) == -1, slot    # the slot comes before the group
    for group in (3, -2, 99):
        assert covf(g._h, 1, one, group, *args()) == -1
    cov_untouched()
    # -- a good call writes exactly its share
    assert prof(g._h, C.byref(request()), 2, out.ctypes.data) == 0 and (out[:112] != PAT).any() and (out[112:] == PAT).all()
    out[:] = PAT
    assert covf(g._h, 8, one, 2, *args()) == 0 and cnt.value > 0 and (mean[:8] != PAT).all() and mean[8] == PAT
    assert (cov[:64] != PAT).all() and (cov[64:] == PAT).all()
    cnt.value, sw.value, sw2.value = -7, PAT, PAT
    mean[:], cov[:] = PAT, PAT
    # -- without a weight row both calls are refused: after the request's (the slots') checks, before the group's
    try:
        g.clear_weights()
        prof_refused(-1, request())
        prof_refused(-6, request(struct_size=8))
        assert covf(g._h, 1, one, -1, *args()) == -1
        assert covf(g._h, 1, (C.c_int32 * 1)(weight_slot()), -1, *args()) == -1           # and the weight slot is then a bad slot
        cov_untouched()
        for call in (lambda: g.weighted_profile_stats(["T"]), lambda: g.weighted_covariance(["thickness"])):
            with pytest.raises(SamsimError) as e:
                call()
            assert e.value.code == -1
    finally:
        g.set_weights(J_SUM, "gauss", small["scale"])
    assert g.weights().tobytes() == w.tobytes()
    # -- without labels a group is refused, -1 is not
    g.set_groups(None)
    try:
        prof_refused(-1, request(), 0)
        assert covf(g._h, 1, one, 0, *args()) == -1
        cov_untouched()
        assert g.weighted_covariance(["thickness"])[0] == (w > 0.0).sum()
        assert g.weighted_profile_stats(["T"], axis="layer", origin="top")["T"]["count"].max() == (w > 0.0).sum()
    finally:
        g.set_groups(lab, ngroups=3)
