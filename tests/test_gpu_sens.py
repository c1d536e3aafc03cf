"""Ensemble sensitivities on the GPU (samsim_get_covariance, samsim_get_profile_regression): joint second moments of the column
scalars and, per depth bin, of a layer profile and a per-column predictor, reduced on the device.  Everything is checked against
the extended-precision reference of tests/sens_reference.py applied to get_state() / get_status() of the same handle.

Tolerances are the bars of tests/test_gpu_profile_stats.py::check carried over to second moments: count exact, means at 1e-12
relative, var_x, var_y and cov within 1e-10 * sx * sy with sx = max(1e-3, std_x), sy = max(1e-3, std_y) -- with x = y the std bar
squared; the bar scales with the spreads, not with |cov|, because a covariance near zero has no relative accuracy."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import samsim_amd
from samsim_amd import capi, testcases as tcs
from samsim_amd.capi import A, NSCAL, PAIR_STAT_DTYPE, ProfileRequest, S
from tests import sens_reference as sr
from tests.helpers import golden, ROOT
from tests.profile_reference import column_thickness
from tests.test_gpu_group_stats import labels_of_test_1
from tests.test_gpu_profile_stats import close, ensemble, pick_dz

pytestmark = pytest.mark.gpu
HOST = os.path.join(ROOT, "host", "samsim_host.x")
CORRUPT = (5, 40000, 70000)
SLOTS = ["thickness", "T_top", "m_snow", "thick_snow", "bulk_salin", "N_active", "dT2m", "precip_scale"]
ARRAYS = ["T", "S_bu", "psi_l"]


@pytest.fixture(scope="module")
def big():
    """the 256 members of the day-200 ensemble tiled over 70 001 columns: 1 094 blocks of 64, more than the grid has waves (1 024),
    and a ragged tail of 49; three columns stopped.  The tests only label it and read reductions, so they share it."""
    ncol = 70001
    assert (ncol + 63) // 64 > 1024 and ncol % 64 != 0
    g = ensemble("sheba_ensemble_80.npz", ncol, 3, corrupt=CORRUPT)
    status = g.get_status()[0]
    assert sorted(np.flatnonzero(status)) == list(CORRUPT)
    return g, g.get_state(), status


@pytest.fixture(scope="module")
def small():
    """the same ensemble over 4 197 columns (65 blocks + 37 columns), two of them stopped: the depth-axis reference is a loop over
    layers x bins x columns"""
    ncol = 4197
    g = ensemble("sheba_ensemble_80.npz", ncol, 3, corrupt=(5, 3000))
    status = g.get_status()[0]
    assert (status != 0).sum() == 2
    lab = (np.arange(ncol) % 3).astype(np.int32)
    lab[::7] = -1
    g.set_groups(lab, ngroups=3)
    return g, g.get_state(), status, lab


@pytest.fixture(scope="module")
def same():
    """256 copies of one column (testcase 1: no forcing, so dT2m = 0 and precip_scale = 1 everywhere), default output window"""
    ncol = 256
    cfg, st = tcs.testcase1(ncol)
    g = samsim_amd.hip_solver(cfg, ncol)
    g.set_state(st)
    g.set_clock()
    g.step(4000)                                    # past the output point at step 3602: the vital signs are set
    assert not g.get_status()[0].any()
    return g, g.get_state(), cfg


def check_cov(got, want, what):
    (n, mean, cov), (rn, rmean, rcov) = got, want
    rmean, rcov = rmean.astype(np.float64), rcov.astype(np.float64)
    sd = np.maximum(1e-3, np.sqrt(np.diag(rcov)))
    print(what, "count", n, rn, "| mean err", float(np.max(np.abs(mean - rmean) / np.maximum(1.0, np.abs(rmean)))) if rn else 0.0,
          "| cov err / (sx sy)", float(np.max(np.abs(cov - rcov) / np.outer(sd, sd))))
    assert n == rn, what
    assert close(mean, rmean, 1e-12).all(), what
    assert (np.abs(cov - rcov) <= 1e-10 * np.outer(sd, sd)).all(), what


def check_pairs(q, r, what):
    for name in r:
        g, w = q[name], r[name]
        sx, sy = np.maximum(1e-3, np.sqrt(w["var_x"])), np.maximum(1e-3, np.sqrt(w["var_y"]))
        print(what, name, "count", int(w["count"].min()), "..", int(w["count"].max()),
              "| mean err", float(np.max(np.abs(g["mean_y"] - w["mean_y"]) / np.maximum(1.0, np.abs(w["mean_y"])))),
              float(np.max(np.abs(g["mean_x"] - w["mean_x"]) / np.maximum(1.0, np.abs(w["mean_x"])))),
              "| var_x, var_y, cov err / bar", float(np.max(np.abs(g["var_x"] - w["var_x"]) / (sx * sx))),
              float(np.max(np.abs(g["var_y"] - w["var_y"]) / (sy * sy))), float(np.max(np.abs(g["cov"] - w["cov"]) / (sx * sy))))
        assert np.array_equal(g["count"], w["count"]), (what, name)
        assert close(g["mean_x"], w["mean_x"], 1e-12).all() and close(g["mean_y"], w["mean_y"], 1e-12).all(), (what, name)
        assert (np.abs(g["var_x"] - w["var_x"]) <= 1e-10 * sx * sx).all(), (what, name)
        assert (np.abs(g["var_y"] - w["var_y"]) <= 1e-10 * sy * sy).all(), (what, name)
        assert (np.abs(g["cov"] - w["cov"]) <= 1e-10 * sx * sy).all(), (what, name)


def check_against_statistics(q, stats, what):
    """count and mean_y are the bytes of the statistics call, sqrt(var_y) those of its std"""
    for name in stats:
        assert q[name]["count"].tobytes() == stats[name]["count"].tobytes(), (what, name)
        assert q[name]["mean_y"].tobytes() == stats[name]["mean"].tobytes(), (what, name)
        assert np.sqrt(q[name]["var_y"]).tobytes() == stats[name]["std"].tobytes(), (what, name)


def test_scalars_against_the_reference(big):
    g, s, status = big
    want = sr.covariance_reference(s, status, SLOTS)
    rho = capi.correlation(want[2].astype(np.float64))
    assert abs(rho[0, 7]) > 0.9 and abs(rho[3, 7]) > 0.9                 # a kernel that returned zero covariances could not pass
    got = g.covariance(SLOTS)
    check_cov(got, want, "8 slots, every column")
    assert got[0] == g.ncol - 3                                          # the three stopped columns are missing
    lab, ng = labels_of_test_1(g.ncol), 11
    assert status[12345] == 0 and min(lab[c] for c in CORRUPT) >= 0
    g.set_groups(lab, ngroups=ng)
    for k in sorted({3} | {int(lab[c]) for c in CORRUPT}):
        got = g.covariance(SLOTS, group=k)
        check_cov(got, sr.covariance_reference(s, status, SLOTS, lab, k), f"group {k}")
        assert got[0] == (lab == k).sum() - sum(1 for c in CORRUPT if lab[c] == k)
    n, mean, cov = g.covariance(SLOTS, group=9)                          # one column: its values, and zeros
    one = np.array([s.n_active[12345] if name == "N_active" else s.sc(name)[12345] for name in SLOTS], dtype=np.float64)
    assert n == 1 and np.array_equal(mean, one) and cov.tobytes() == np.zeros((8, 8)).tobytes()
    n, mean, cov = g.covariance(SLOTS, group=10)                         # the empty group: all zeros
    assert n == 0 and mean.tobytes() == np.zeros(8).tobytes() and cov.tobytes() == np.zeros((8, 8)).tobytes()
    # fewer slots take another instantiation of the kernel: every size once
    for k in range(1, 8):
        check_cov(g.covariance(SLOTS[-k:], group=3), sr.covariance_reference(s, status, SLOTS[-k:], lab, 3), f"{k} slots, group 3")


def test_a_slot_listed_twice(big):
    g, s, status = big
    names = ["thickness", "precip_scale", "thickness", "dT2m", "precip_scale", "T_top"]
    n, mean, cov = g.covariance(names)
    check_cov((n, mean, cov), sr.covariance_reference(s, status, names), "a slot twice")
    assert cov.tobytes() == np.ascontiguousarray(cov.T).tobytes()
    for i, j in ((0, 2), (1, 4)):
        assert cov[i, i] > 0.0 and mean[i].tobytes() == mean[j].tobytes()
        assert cov[i, j].tobytes() == cov[i, i].tobytes() == cov[j, j].tobytes(), (i, j)
        assert cov[i].tobytes() == cov[j].tobytes() and np.ascontiguousarray(cov[:, i]).tobytes() == np.ascontiguousarray(cov[:, j]).tobytes()


def test_every_number_of_slots_gives_the_leading_block_of_eight(small):
    """Every instantiation of the walk, 1 to 8 slots: the first k slots alone return count, mean[:k] and cov[:k, :k] of the call
    with all eight, byte for byte -- a pair's chain of operations does not depend on how many slots ride along.  4 197 columns are
    66 waves, so a lane of the merge takes two waves and the lanes 33 to 63 none, and the last block has 37 columns."""
    g = small[0]
    for group in (None, 1):
        n8, mean8, cov8 = g.covariance(SLOTS, group=group)
        assert n8 > 1000 and (np.diag(cov8)[:5] > 0.0).all()
        for k in range(1, 9):
            n, mean, cov = g.covariance(SLOTS[:k], group=group)
            assert n == n8 and mean.tobytes() == mean8[:k].tobytes(), (group, k)
            assert cov.tobytes() == np.ascontiguousarray(cov8[:k, :k]).tobytes(), (group, k)


def test_profiles_by_layer_against_the_reference(big):
    """80 layer bins: two passes; 1 094 blocks: every wave strides"""
    g, s, status = big
    lab = labels_of_test_1(g.ncol)
    g.set_groups(lab, ngroups=11)
    for origin in ("top", "bottom"):
        kw = dict(axis="layer", origin=origin)
        for group in (None, 3):
            r = sr.profile_regression_reference(s, status, ARRAYS, "precip_scale", lab, group, **kw)
            q = g.profile_regression(ARRAYS, "precip_scale", group=group, **kw)
            assert r["S_bu"]["count"].max() == (sr.counting(status, lab, group)).sum() and r["S_bu"].shape == (80,)
            assert np.abs(capi.slope_and_correlation(r["S_bu"])[1]).max() > 0.9
            check_pairs(q, r, f"layer/{origin}/group {group}")
            check_against_statistics(q, g.profile_stats(ARRAYS, group=group, **kw), f"layer/{origin}/group {group}")


def test_profiles_by_depth_against_the_reference(small):
    g, s, status, lab = small
    H = column_thickness(s)[status == 0]
    dz = pick_dz(H, (0.07, 0.05, 0.09, 0.11), 32, (0.0, 0.035))
    dz100 = pick_dz(H, (0.02, 0.021, 0.019, 0.022), 100, (0.0,))
    assert dz is not None and dz100 is not None
    requests = [(dict(axis="depth", origin="top", nbins=32, dz=dz), None), (dict(axis="depth", origin="bottom", nbins=32, z0=0.035, dz=dz), None),
                (dict(axis="depth", origin="top", nbins=32, z0=0.035, dz=dz), 1), (dict(axis="depth", origin="bottom", nbins=32, dz=dz), 2),
                (dict(axis="depth", origin="top", nbins=100, dz=dz100), None), (dict(axis="depth", origin="bottom", nbins=100, dz=dz100), 0)]
    for kw, group in requests:
        r = sr.profile_regression_reference(s, status, ARRAYS, "precip_scale", lab, group, **kw)
        cnt = r["T"]["count"]
        assert cnt.max() == sr.counting(status, lab, group).sum() and ((cnt > 0) & (cnt < cnt.max())).any() and (cnt == 0).any()
        if kw["nbins"] > 64:
            assert cnt[:64].max() > 0 and cnt[64:].max() > 0                   # both passes hold ice
        q = g.profile_regression(ARRAYS, "precip_scale", group=group, **kw)
        check_pairs(q, r, f"{kw}/group {group}")
        check_against_statistics(q, g.profile_stats(ARRAYS, group=group, **kw), f"{kw}/group {group}")
    # another predictor, and the layer axis on this handle
    kw = dict(axis="layer", origin="bottom")
    for predictor in ("dT2m", "N_active"):
        check_pairs(g.profile_regression(ARRAYS, predictor, **kw), sr.profile_regression_reference(s, status, ARRAYS, predictor, **kw),
                    f"layer/bottom on {predictor}")


def test_identical_columns(same):
    g, s, cfg = same
    names = ["thickness", "bulk_salin", "energy_stored", "T_top", "N_active", "dT2m", "precip_scale"]
    n, mean, cov = g.covariance(names)
    one = np.array([s.n_active[0] if name == "N_active" else s.sc(name)[0] for name in names], dtype=np.float64)
    assert n == g.ncol and one[0] > 0.0 and one[2] != 0.0 and one[6] == 1.0
    assert np.array_equal(mean, one) and cov.tobytes() == np.zeros((7, 7)).tobytes()
    na = int(s.n_active[0])
    arrays = ["T", "S_bu", "psi_l", "thick"]
    for kw in (dict(axis="layer", origin="top"), dict(axis="layer", origin="bottom"),
               dict(axis="depth", origin="top", nbins=40, dz=0.0015), dict(axis="depth", origin="bottom", nbins=40, z0=0.001, dz=0.0015)):
        q, stats = g.profile_regression(arrays, "T_top", **kw), g.profile_stats(arrays, **kw)
        for name in arrays:
            x, occ = q[name], q[name]["count"] > 0
            assert occ.any() and (x["count"][occ] == g.ncol).all(), (kw, name)
            assert (x["mean_x"][occ] == s.sc("T_top")[0]).all() and np.array_equal(x["mean_y"][occ], stats[name]["min"][occ]), (kw, name)
            for field in ("var_x", "var_y", "cov"):
                assert x[field].tobytes() == np.zeros(x.size).tobytes(), (kw, name, field)
            assert x[~occ].tobytes() == np.zeros((~occ).sum(), dtype=PAIR_STAT_DTYPE).tobytes(), (kw, name)
            if kw["axis"] == "layer":               # the stored values themselves, bit for bit
                col = s.arr(name)[:na, 0]
                assert occ.sum() == na and np.array_equal(x["mean_y"][:na], col if kw["origin"] == "top" else col[::-1]), (kw, name)


def test_deterministic_and_blind_to_labels_outside_the_group(big):
    g, s, status = big
    lab, ng = labels_of_test_1(g.ncol), 11
    kw = dict(axis="layer", origin="bottom")
    g.set_groups(lab, ngroups=ng)

    def everything(group):
        n, mean, cov = g.covariance(SLOTS, group=group)
        q = g.profile_regression(ARRAYS, "precip_scale", group=group, **kw)
        return np.int64(n).tobytes() + mean.tobytes() + cov.tobytes() + b"".join(q[name].tobytes() for name in ARRAYS)
    first = {k: everything(k) for k in (None, 3, 4)}
    assert all(everything(k) == first[k] for k in first)
    # every column outside group 3 gets another label: the other groups' labels permuted, every fifth of them unlabelled
    perm = np.array([1, 2, 4, 3, 5, 6, 7, 8, 0, 10, 9, -1], dtype=np.int32)      # (the last entry: -1 stays -1)
    lab2 = perm[lab]
    outside = np.flatnonzero(lab != 3)
    lab2[outside[::5]] = -1
    assert np.array_equal(lab2 == 3, lab == 3) and (lab2[outside] != lab[outside]).mean() > 0.8
    g.set_groups(lab2, ngroups=ng)
    assert everything(3) == first[3] and everything(None) == first[None] and everything(4) != first[4]
    check_cov(g.covariance(SLOTS, group=4), sr.covariance_reference(s, status, SLOTS, lab2, 4), "relabelled, group 4")


def test_the_calls_change_nothing(small, same):
    g, s, status, lab = small
    clock = g.get_clock()
    groups_before = g.group_stats(["thickness", "N_active"])
    g.covariance(SLOTS)
    g.covariance(SLOTS, group=1)
    g.profile_regression(ARRAYS, "precip_scale", axis="layer", origin="top")
    g.profile_regression(ARRAYS, "dT2m", axis="depth", origin="bottom", nbins=100, dz=0.02, group=2)
    after, t = g.get_clock(), g.get_state()
    assert (clock.time, clock.step, clock.n_time_out, clock.time_counter, clock.n_outputs) == \
        (after.time, after.step, after.n_time_out, after.time_counter, after.n_outputs)
    assert np.array_equal(t.lay, s.lay, equal_nan=True) and np.array_equal(t.scal, s.scal, equal_nan=True) and np.array_equal(t.n_active, s.n_active)
    assert np.array_equal(g.get_status()[0], status)
    groups_after = g.group_stats(["thickness", "N_active"])                # the labels are those of before
    assert all(groups_after[n].tobytes() == groups_before[n].tobytes() and groups_after[n]["count"].sum() > 0 for n in groups_before)
    # the output snapshot
    h = same[0]
    o = h.get_output()
    h.covariance(["thickness", "T_top"])
    h.profile_regression(["T"], "T_top", axis="depth", origin="top", nbins=8, dz=0.01)
    p = h.get_output()
    assert (o.time, o.step) == (p.time, p.step) and o.step == 3602
    assert np.array_equal(o.lay, p.lay) and np.array_equal(o.scal, p.scal) and np.array_equal(o.n_active, p.n_active)


def test_argument_errors(same):
    g, s, cfg = same
    g.set_groups(None)

    def request(**kw):
        rq = ProfileRequest()
        rq.struct_size, rq.axis, rq.origin, rq.nbins, rq.narrays = C.sizeof(ProfileRequest), 1, 0, 8, 1
        rq.arrays[0] = A["T"]
        rq.z0, rq.dz = 0.0, 0.01
        for k, v in kw.items():
            if k == "array0":
                rq.arrays[0] = v
            else:
                setattr(rq, k, v)
        return rq

    def refused(code, call, *args):
        with pytest.raises(samsim_amd.SamsimError) as e:
            call(*args)
        assert e.value.code == code, (call.__name__, args)

    def good():
        assert g.covariance_raw([S["thickness"], -1], -1)[0] == g.ncol
        assert g.profile_regression_raw(request(), S["precip_scale"], -1).shape == (1, 8)
    good()
    # samsim_get_covariance: null pointers, nslots, slots, group
    f = g._f("get_covariance")
    slots, count, mean, cov = (C.c_int32 * 2)(0, 1), C.c_int64(0), np.zeros(8), np.zeros(64)
    full = [g._h, 2, slots, -1, C.byref(count), mean.ctypes.data, cov.ctypes.data]
    assert f(*full) == 0
    for k in (0, 2, 4, 5, 6):
        assert f(*[None if i == k else a for i, a in enumerate(full)]) == -1, k
    for bad in ([], list(range(9))):
        refused(-1, g.covariance_raw, bad, -1)
    for bad in (NSCAL, -2):
        refused(-1, g.covariance_raw, [0, bad], -1)
    assert g.covariance_raw([NSCAL - 1, -1], -1)[0] == g.ncol
    refused(-1, g.covariance_raw, [0, 1], -2)
    refused(-1, g.covariance_raw, [0, 1], 0)                               # a group without labels
    good()
    # samsim_get_profile_regression: the request as samsim_get_profile_stats checks it, and first
    h = g._f("get_profile_regression")
    out = np.zeros(64, dtype=PAIR_STAT_DTYPE)
    rq = request()
    assert h(g._h, C.byref(rq), 0, -1, out.ctypes.data) == 0
    assert h(None, C.byref(rq), 0, -1, out.ctypes.data) == -1 and h(g._h, None, 0, -1, out.ctypes.data) == -1
    assert h(g._h, C.byref(rq), 0, -1, None) == -1
    cases = [(dict(struct_size=C.sizeof(ProfileRequest) - 8), -6), (dict(nbins=0), -1), (dict(nbins=1025), -1), (dict(narrays=9), -1),
             (dict(narrays=0), -1), (dict(array0=15), -1), (dict(array0=-1), -1), (dict(dz=0.0), -1), (dict(dz=float("nan")), -1),
             (dict(z0=-0.01), -1), (dict(z0=float("inf")), -1), (dict(axis=2), -1), (dict(origin=2), -1), (dict(axis=0, nbins=cfg.nlayer + 1), -1)]
    for kw, code in cases:
        refused(code, g.profile_regression_raw, request(**kw), S["precip_scale"], -1)
    for bad in (NSCAL, -2):
        refused(-1, g.profile_regression_raw, request(), bad, -1)
    assert g.profile_regression_raw(request(), -1, -1).shape == (1, 8)     # N_active as the predictor
    refused(-1, g.profile_regression_raw, request(), 0, -2)
    refused(-1, g.profile_regression_raw, request(), 0, 0)                 # a group without labels
    # the order: a bad request is reported before a bad predictor, a bad predictor before a bad group (both -1: the request's -6 tells)
    refused(-6, g.profile_regression_raw, request(struct_size=C.sizeof(ProfileRequest) - 8), NSCAL, -2)
    good()
    # with labels: the group must lie below ngroups
    g.set_groups((np.arange(g.ncol) % 3).astype(np.int32))
    assert g.covariance_raw([0, 1], 2)[0] > 0 and g.profile_regression_raw(request(), 0, 2)["count"].max() > 0
    refused(-1, g.covariance_raw, [0, 1], 3)
    refused(-1, g.profile_regression_raw, request(), 0, 3)
    refused(-6, g.profile_regression_raw, request(struct_size=C.sizeof(ProfileRequest) - 8), 0, 3)
    good()
    g.set_groups(None)


@pytest.mark.skipif(not os.path.exists(HOST), reason="Fortran host not built (no flang)")
def test_fortran_host_sensitivity_files(tmp_path):
    """sens in &samsim_run: one row per output point in dat_ens_sens.dat and, with profile_bins > 0, in
    dat_ens_sens_profile_{T,S_bu,psi_l}.dat, equal at the printed precision (ES16.8: nine digits, coarser than the bars above) to
    what the Python mirror gets from an identically driven handle; without the key no new file appears"""
    sheba = golden("sheba_forcing.npz")
    keys = (("fl_sw", "flux_sw"), ("fl_lw", "flux_lw"), ("T2m", "T2m"), ("precip", "precip"))

    def run(d, extra):
        (d / "output").mkdir(parents=True)
        for key, name in keys:
            np.savetxt(d / f"{name}.txt.input", sheba[key], fmt="%.17e")
        (d / "samsim.nml").write_text(f"&samsim_run testcase=4, ncol={ncol}, perturb=.true., max_steps={total}, "
                                      f"profile_bins={nbins}, profile_dz={dz}{extra} /\n")
        r = subprocess.run([HOST], cwd=d, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return d / "output"
    ncol, nbins, dz, total = 96, 8, 0.01, 18000
    with_sens = run(tmp_path / "sens", ", sens=.true.")
    plain = run(tmp_path / "plain", "")
    assert sorted(set(os.listdir(with_sens)) - set(os.listdir(plain))) == \
        sorted(["dat_ens_sens.dat"] + [f"dat_ens_sens_profile_{n}.dat" for n in ARRAYS])
    assert not set(os.listdir(plain)) - set(os.listdir(with_sens))
    assert (plain / "dat_ensemble.dat").read_bytes() == (with_sens / "dat_ensemble.dat").read_bytes()
    # the same run through the Python mirror
    cfg, st = tcs.testcase4(ncol)
    g = samsim_amd.hip_solver(cfg, ncol)
    g.set_forcing(*[sheba[k] for k, _ in keys], *tcs.ensemble_perturbation(ncol))
    g.set_state(st)
    g.set_clock()
    slots, rows, done = ["thickness", "thick_snow", "bulk_salin", "freeboard", "T_top", "N_active", "dT2m", "precip_scale"], [], 0
    while done < total:
        n = min(g.steps_to_output(), total - done)
        g.step(n)
        done += n
        if g.steps_to_output() == cfg.i_time_out + 1 or done == 1:
            rows.append((g.covariance(slots), g.profile_regression(ARRAYS, "precip_scale", axis="depth", origin="top", nbins=nbins, dz=dz)))
    assert len(rows) == 3                                          # outputs at steps 1, 8642, 17283

    def printed(got, want):
        """ES16.8 prints nine digits: half a unit of the ninth"""
        tol = np.array([0.5e-8 * 10.0 ** math.floor(math.log10(abs(x))) if x != 0.0 else 0.0 for x in np.ravel(want)]) * (1.0 + 1e-6)
        return (np.abs(np.ravel(got) - np.ravel(want)) <= tol).all()
    f = np.loadtxt(with_sens / "dat_ens_sens.dat")
    ens = np.loadtxt(with_sens / "dat_ensemble.dat")
    assert f.shape == (len(rows), 1 + 6 * 5)
    moved = False
    for i, ((n, mean, cov), prof) in enumerate(rows):
        x = f[i, 1:].reshape(6, 5)
        assert f[i, 0] == ens[i, 0] and (x[:, 0] == n).all() and n == ens[i, 1] == ncol, i
        rho = capi.correlation(cov)
        var = np.diag(cov)
        want = np.array([[cov[j, 6] / var[6], cov[j, 7] / var[7], rho[j, 6], rho[j, 7]] for j in range(6)])
        print("output", i, "slopes and correlations of thickness, thick_snow, bulk_salin, freeboard, T_top, N_active\n", want)
        assert var[6] > 1.0 and var[7] > 0.02 and printed(x[:, 1:], want), i
        moved = moved or bool(np.any(want != 0.0))
        for name in ARRAYS:
            p = np.loadtxt(with_sens / f"dat_ens_sens_profile_{name}.dat")
            stats = np.loadtxt(with_sens / f"dat_ens_profile_{name}.dat")
            assert p.shape == (len(rows), 1 + 3 * nbins) and p[i, 0] == ens[i, 0], name
            y, w = p[i, 1:].reshape(nbins, 3), prof[name]
            assert np.array_equal(y[:, 0], w["count"]) and np.array_equal(y[:, 0], stats[i, 1:].reshape(nbins, 5)[:, 0]), (name, i)
            assert w["count"][0] == ncol, (name, i)
            assert printed(y[:, 1:], np.stack(capi.slope_and_correlation(w), axis=1)), (name, i)
    assert moved                                                   # the ensemble responds to its perturbation
