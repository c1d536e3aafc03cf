"""Per-group ensemble statistics on the GPU (samsim_set_groups, samsim_get_group_stats, samsim_get_group_profile_stats): the
scalars against numpy over get_state() / get_status() of the same handle, the profiles against the numpy restatement of the
header's semantics (tests/profile_reference.py) with every column outside the group marked as stopped.  Tolerances are those of
tests/test_gpu_profile_stats.py::check: count, min and max exact, mean at 1e-12, std at 1e-10."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import samsim_amd
from samsim_amd import capi, testcases as tcs
from samsim_amd.capi import A, NSCAL, ProfileRequest, STAT_DTYPE
from tests.helpers import golden, load_checkpoint, sheba_forcing, ROOT
from tests.profile_reference import column_thickness, profile_reference
from tests.test_gpu_profile_stats import check, ensemble, pick_dz

pytestmark = pytest.mark.gpu
HOST = os.path.join(ROOT, "host", "samsim_host.x")
SCALARS = ["thickness", "thick_snow", "bulk_salin", "freeboard", "T_top", "T2m", "m_snow"]
CORRUPT = (5, 40000, 70000)


def spunup(ncol, corrupt=()):
    """tc4_spunup_state.npz replicated over ncol columns with the counter-based perturbation, run to the next output point"""
    st1, clock = load_checkpoint("tc4_spunup_state.npz")
    cfg, _ = tcs.testcase4(1)
    st = st1.replicate(ncol)
    for c in corrupt:
        st.arr("H_abs")[0, c] = -1.0e15            # getT cannot converge -> STOP 99
    g = samsim_amd.hip_solver(cfg, ncol)
    g.set_forcing(*sheba_forcing(), *tcs.ensemble_perturbation(ncol))
    g.set_state(st)
    g.set_clock(**clock)
    g.run_to_output()
    return g


@pytest.fixture(scope="module")
def big():
    """70 001 columns: 1 094 blocks of 64, more than the grid has waves (at most 1 024), and a ragged tail of 49; three columns
    stopped.  The tests only label it and read statistics, so they share it."""
    ncol = 70001
    assert (ncol + 63) // 64 > 1024 and ncol % 64 != 0
    g = spunup(ncol, CORRUPT)
    status = g.get_status()[0]
    assert sorted(np.flatnonzero(status)) == list(CORRUPT)
    return g, g.get_state(), status


def scalar_reference(s, status, labels, ngroups, names):
    """numpy over the columns with status 0 and label g, per name and group"""
    ok = np.flatnonzero((status == 0) & (labels >= 0))
    order = ok[np.argsort(labels[ok], kind="stable")]
    bounds = np.searchsorted(labels[order], np.arange(ngroups + 1))
    res = {}
    for n in names:
        row = s.n_active.astype(np.float64) if n == "N_active" else s.sc(n)
        out = np.zeros(ngroups, dtype=STAT_DTYPE)
        for g in range(ngroups):
            v = row[order[bounds[g]:bounds[g + 1]]]
            if v.size:
                out[g] = (v.size, v.mean(), v.min(), v.max(), v.std())
        res[n] = out
    return res


def labels_of_test_1(ncol):
    c = np.arange(ncol, dtype=np.int64)
    lab = ((c * 7919) % 9).astype(np.int32)
    lab[::11] = -1
    lab[12345] = 9                                  # group 9 holds exactly one column; group 10 stays empty
    return lab


def test_scalars_per_group_against_numpy(big):
    g, s, status = big
    lab, ng = labels_of_test_1(g.ncol), 11
    assert len({int(lab[c]) for c in CORRUPT}) == 3 and min(lab[c] for c in CORRUPT) >= 0 and status[12345] == 0
    assert (lab == 9).sum() == 1 and (lab == 10).sum() == 0 and (lab == -1).sum() > 6000
    g.set_groups(lab, ngroups=ng)
    names = SCALARS + ["N_active"]
    q, r = g.group_stats(names), scalar_reference(s, status, lab, ng, names)
    assert all(q[n].shape == (ng,) for n in names)
    check(q, r, "11 groups", exact_extremes=True)
    for c in CORRUPT:                               # a stopped column is missing from its group's count
        assert q["thickness"]["count"][lab[c]] == (lab == lab[c]).sum() - 1
    for n in names:
        assert q[n][10].tobytes() == np.zeros(1, dtype=STAT_DTYPE).tobytes(), n          # the empty group: all zeros
        one = s.n_active[12345] if n == "N_active" else s.sc(n)[12345]
        assert q[n][9]["count"] == 1 and q[n][9]["mean"] == q[n][9]["min"] == q[n][9]["max"] == one and q[n][9]["std"] == 0.0, n
    assert q["thickness"]["mean"][:9].min() > 1.0 and q["T2m"]["std"][:9].min() > 1.0 and q["thick_snow"]["std"][:9].min() > 0.0


def test_1024_groups(big):
    """the wave's table at full size (40 KiB of LDS)"""
    g, s, status = big
    lab = (np.arange(g.ncol) % 1024).astype(np.int32)
    g.set_groups(lab)
    assert g.ngroups == capi.MAX_GROUPS == 1024
    names = SCALARS + ["N_active"]
    q, r = g.group_stats(names), scalar_reference(s, status, lab, 1024, names)
    assert r["thickness"]["count"].min() >= 67 and r["thickness"]["count"].sum() == g.ncol - 3
    check(q, r, "1024 groups", exact_extremes=True)


def test_deterministic_and_blind_to_labels_outside_the_group(big):
    g, s, status = big
    lab, ng = labels_of_test_1(g.ncol), 11
    names = SCALARS + ["N_active"]
    g.set_groups(lab, ngroups=ng)
    q1, q2 = g.group_stats(names), g.group_stats(names)
    for n in names:
        assert q1[n].tobytes() == q2[n].tobytes(), n
    # every column outside group 3 gets another label: the other groups' labels permuted, every fifth of them unlabelled
    perm = np.array([1, 2, 4, 3, 5, 6, 7, 8, 0, 10, 9, -1], dtype=np.int32)      # (the last entry: -1 stays -1)
    lab2 = perm[lab]
    outside = np.flatnonzero(lab != 3)
    lab2[outside[::5]] = -1
    assert np.array_equal(lab2 == 3, lab == 3) and (lab2[outside] != lab[outside]).mean() > 0.8
    g.set_groups(lab2, ngroups=ng)
    q3 = g.group_stats(names)
    check(q3, scalar_reference(s, status, lab2, ng, names), "relabelled", exact_extremes=True)
    for n in names:
        assert q3[n][3].tobytes() == q1[n][3].tobytes(), n
        for k in list(range(3)) + list(range(4, 11)):
            assert q3[n][k].tobytes() != q1[n][k].tobytes(), (n, k)


def test_one_group_of_all_columns(big):
    g, s, status = big
    g.set_groups(np.zeros(g.ncol, dtype=np.int32), ngroups=1)
    names = SCALARS + ["N_active"]
    q, e = g.group_stats(names), g.ensemble_stats(names)
    for n in names:
        x = q[n][0]
        print(n, "mean", x["mean"], e[n].mean, "std", x["std"], e[n].std)
        assert x["count"] == e[n].count == g.ncol - 3 and x["min"] == e[n].min and x["max"] == e[n].max, n
        assert abs(x["mean"] - e[n].mean) <= 1e-12 * max(1.0, abs(e[n].mean)), n
        assert abs(x["std"] - e[n].std) <= 1e-10 * max(1e-3, e[n].std), n
    arrays = ["T", "S_bu", "psi_l"]
    for kw in (dict(axis="layer", origin="top"), dict(axis="layer", origin="bottom"),
               dict(axis="depth", origin="top", nbins=32, dz=0.07), dict(axis="depth", origin="bottom", nbins=32, z0=0.035, dz=0.07)):
        whole, grouped = g.profile_stats(arrays, **kw), g.profile_stats(arrays, group=0, **kw)
        for n in arrays:
            assert whole[n]["count"].max() == g.ncol - 3 and whole[n].tobytes() == grouped[n].tobytes(), (kw, n)


def test_profiles_per_group():
    ncol, nbins = 4197, 32                          # 65 blocks + 37 columns
    g = spunup(ncol, corrupt=(5, 3000))
    status = g.get_status()[0]
    assert (status != 0).sum() == 2
    s = g.get_state()
    lab = (np.arange(ncol) % 3).astype(np.int32)
    lab[::7] = -1
    assert lab[5] >= 0 and lab[3000] >= 0 and lab[5] != lab[3000]
    g.set_groups(lab, ngroups=3)
    arrays = ["T", "S_bu", "psi_l"]
    dz = pick_dz(column_thickness(s)[status == 0], (0.07, 0.05, 0.09, 0.11), nbins, (0.0, 0.035))
    assert dz is not None
    requests = [(dict(axis="layer", origin="top"), True), (dict(axis="layer", origin="bottom"), True),
                (dict(axis="depth", origin="top", nbins=nbins, dz=dz), False),
                (dict(axis="depth", origin="bottom", nbins=nbins, z0=0.035, dz=dz), False)]
    for kw, exact in requests:
        whole = g.profile_stats(arrays, **kw)
        unlabelled = profile_reference(s, np.where(lab == -1, status, 1).astype(np.int32), arrays, **kw)
        total = {n: np.zeros_like(whole[n]["count"]) for n in arrays}
        for k in range(3):
            r = profile_reference(s, np.where(lab == k, status, 1).astype(np.int32), arrays, **kw)
            q = g.profile_stats(arrays, group=k, **kw)
            cnt = r["T"]["count"]
            assert cnt.max() == ((lab == k) & (status == 0)).sum(), (kw, k)
            if kw["axis"] == "depth":               # (every layer of this ensemble is active: only depth bins lie below the ice)
                assert (cnt == 0).any() and r["T"]["std"].max() > 0.0, (kw, k)
            check(q, r, f"group {k} {kw}", exact_extremes=exact)
            for n in arrays:
                total[n] += q[n]["count"]
        for n in arrays:
            assert whole[n]["count"].max() == ncol - 2
            assert np.array_equal(total[n], whole[n]["count"] - unlabelled[n]["count"]), (kw, n)


def test_identical_columns():
    ncol = 256
    cfg, st = tcs.testcase1(ncol)
    g = samsim_amd.hip_solver(cfg, ncol)
    g.set_state(st)
    g.set_clock()
    g.step(4000)                                    # past the output point at step 3602: the vital signs are set
    assert not g.get_status()[0].any()
    s = g.get_state()
    g.set_groups((np.arange(ncol) % 4).astype(np.int32))
    names = ["thickness", "bulk_salin", "energy_stored", "freshwater", "T_top", "fl_q_bottom", "N_active"]
    q = g.group_stats(names)
    assert s.sc("thickness")[0] > 0.0 and s.sc("energy_stored")[0] != 0.0
    for n in names:
        x = q[n]
        one = s.n_active[0] if n == "N_active" else s.sc(n)[0]
        assert x.shape == (4,) and (x["count"] == 64).all(), n
        assert (x["mean"] == one).all() and (x["min"] == one).all() and (x["max"] == one).all() and (x["std"] == 0.0).all(), n


def test_leaves_the_run_alone_and_set_state_keeps_the_labels():
    """labels and statistics between two launches of a handle whose every step is two concurrent launches change nothing of the
    run; samsim_set_state of a window leaves the labels in force"""
    ncol = 1000

    def fresh():
        g = ensemble("sheba_ensemble_80_day75.npz", ncol, 0)
        g.set_launch_split(min_blocks=2)
        return g
    a, b = fresh(), fresh()
    lab = (np.arange(ncol) % 5).astype(np.int32)
    a.step(500)
    a.set_groups(lab)
    clock = a.get_clock()
    q = a.group_stats(["thickness", "T_top", "N_active"])
    assert q["T_top"]["count"].tolist() == [200] * 5 and q["T_top"]["std"].min() > 0.0
    assert a.profile_stats(["T"], group=4)["T"]["count"].max() == 200
    after = a.get_clock()
    assert (clock.time, clock.step, clock.n_time_out, clock.n_outputs) == (after.time, after.step, after.n_time_out, after.n_outputs)
    a.step(500)
    b.step(1000)
    sa, sb = a.get_state(), b.get_state()
    assert np.array_equal(sa.n_active, sb.n_active)
    assert np.array_equal(sa.lay[:4], sb.lay[:4]) and np.array_equal(sa.scal, sb.scal)
    names = ["thickness", "T_top", "m_snow", "N_active"]
    before = a.group_stats(names)
    a.set_state(sa.window(100, 300), 100)            # the same values again: only lost labels could change the statistics
    again = a.group_stats(names)
    for n in names:
        assert before[n]["count"].tolist() == [200] * 5 and again[n].tobytes() == before[n].tobytes(), n


def test_argument_errors():
    ncol = 64
    cfg, st = tcs.testcase1(ncol)
    g = samsim_amd.hip_solver(cfg, ncol)
    g.set_state(st)

    def request(**kw):
        rq = ProfileRequest()
        rq.struct_size, rq.axis, rq.origin, rq.nbins, rq.narrays = C.sizeof(ProfileRequest), 1, 0, 8, 1
        rq.arrays[0] = A["T"]
        rq.z0, rq.dz = 0.0, 0.01
        for k, v in kw.items():
            setattr(rq, k, v)
        return rq

    def refused(code, call, *args):
        with pytest.raises(samsim_amd.SamsimError) as e:
            call(*args)
        assert e.value.code == code, (call.__name__, args)

    def raw_group_stats(slot):
        slots, out = (C.c_int32 * 1)(slot), np.zeros(8, dtype=STAT_DTYPE)
        return g._f("get_group_stats")(g._h, 1, slots, out.ctypes.data)

    # no labels yet
    refused(-1, g.group_stats, ["T_top"])
    refused(-1, g.profile_stats_raw, request(), 0)
    lab = (np.arange(ncol) % 3).astype(np.int32)
    lab[7] = -1
    g.set_groups(lab)
    assert g.ngroups == 3
    good = g.group_stats(["T_top", "N_active"])
    assert good["T_top"]["count"].tolist() == [22, 20, 21]          # 64 columns mod 3, column 7 (label 1) unlabelled
    assert g.profile_stats_raw(request(), 2).shape == (1, 8)
    # refused labels leave the earlier ones in force
    for bad_value in (3, -2):
        bad = lab.copy()
        bad[ncol - 1] = bad_value
        refused(-1, g.set_groups_raw, 3, bad)
    refused(-1, g.set_groups_raw, 1025, np.zeros(ncol, dtype=np.int32))
    refused(-1, g.set_groups_raw, 0, np.zeros(ncol, dtype=np.int32))
    refused(-1, g.set_groups_raw, 3, None)
    assert g.ngroups == 3
    again = g.group_stats(["T_top", "N_active"])
    assert all(again[n].tobytes() == good[n].tobytes() for n in good)
    # the slots and the group
    assert raw_group_stats(NSCAL) == -1 and raw_group_stats(-2) == -1 and raw_group_stats(-1) == 0 and raw_group_stats(NSCAL - 1) == 0
    refused(-1, g.profile_stats_raw, request(), 3)
    refused(-1, g.profile_stats_raw, request(), -1)
    # the request is checked as samsim_get_profile_stats checks it, and first
    refused(-6, g.profile_stats_raw, request(struct_size=C.sizeof(ProfileRequest) - 8), 0)
    refused(-6, g.profile_stats_raw, request(struct_size=C.sizeof(ProfileRequest) - 8), 3)
    refused(-1, g.profile_stats_raw, request(nbins=0), 0)
    refused(-1, g.profile_stats_raw, request(dz=0.0), 0)
    refused(-1, g.profile_stats_raw, request(axis=0, nbins=cfg.nlayer + 1), 0)
    # labels removed
    g.set_groups(None)
    refused(-1, g.group_stats, ["T_top"])
    refused(-1, g.profile_stats_raw, request(), 0)
    assert g.profile_stats_raw(request()).shape == (1, 8)


@pytest.mark.skipif(not os.path.exists(HOST), reason="Fortran host not built (no flang)")
def test_fortran_host_statistics_by_site(tmp_path):
    """stats_by_site in &samsim_run with two sites: one row per output point and site in dat_ens_site.dat and in the per-site
    profile files, equal at the printed precision to what the Python mirror gets from an identically driven handle; without the
    key no new file appears and dat_ensemble.dat is the same bytes"""
    z, sheba = golden("era_sites_forcing.npz"), golden("sheba_forcing.npz")
    keys = (("fl_sw", "flux_sw"), ("fl_lw", "flux_lw"), ("T2m", "T2m"), ("precip", "precip"))

    def run(d, extra):
        (d / "output").mkdir(parents=True)
        (d / "np").mkdir()
        for key, name in keys:
            np.savetxt(d / f"{name}.txt.input", sheba[key], fmt="%.17e")
            np.savetxt(d / "np" / f"{name}.txt.input", z["NorthPole_" + key], fmt="%.17e")
        (d / "samsim.nml").write_text(f"&samsim_run testcase=4, ncol={ncol}, perturb=.true., max_steps={total}, sites='.', 'np', "
                                      f"profile_bins={nbins}, profile_dz={dz}{extra} /\n")
        r = subprocess.run([HOST], cwd=d, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return d / "output"
    ncol, nbins, dz, total = 9, 8, 0.01, 18000                    # five columns of the first site, four of the second
    members = (5, 4)
    by_site = run(tmp_path / "by_site", ", stats_by_site=.true.")
    plain = run(tmp_path / "plain", "")
    new = sorted(set(os.listdir(by_site)) - set(os.listdir(plain)))
    arrays = ["T", "S_bu", "psi_l"]
    assert new == sorted(["dat_ens_site.dat"] + [f"dat_ens_profile_{n}_site{k:02d}.dat" for n in arrays for k in (1, 2)])
    assert (plain / "dat_ensemble.dat").read_bytes() == (by_site / "dat_ensemble.dat").read_bytes()
    # the same run through the Python mirror
    cfg, st = tcs.testcase4(ncol)
    g = samsim_amd.hip_solver(cfg, ncol)
    site = (np.arange(ncol) % 2).astype(np.int32)
    g.set_forcing_sites(*[np.stack([sheba[k], z["NorthPole_" + k]]) for k, _ in keys], site, *tcs.ensemble_perturbation(ncol))
    g.set_state(st)
    g.set_clock()
    g.set_groups(site, ngroups=2)
    slots, rows, done = ["thickness", "thick_snow", "bulk_salin", "freeboard", "T_top", "N_active"], [], 0
    while done < total:
        n = min(g.steps_to_output(), total - done)
        g.step(n)
        done += n
        if g.steps_to_output() == cfg.i_time_out + 1 or done == 1:
            rows.append((g.group_stats(slots), [g.profile_stats(arrays, axis="depth", origin="top", nbins=nbins, dz=dz, group=k) for k in (0, 1)]))
    assert len(rows) == 3                                          # outputs at steps 1, 8642, 17283

    def printed(got, want):
        """ES16.8 prints nine digits: half a unit of the ninth"""
        tol = np.array([0.5e-8 * 10.0 ** math.floor(math.log10(abs(x))) if x != 0.0 else 0.0 for x in np.ravel(want)]) * (1.0 + 1e-6)
        return (np.abs(np.ravel(got) - np.ravel(want)) <= tol).all()
    f = np.loadtxt(by_site / "dat_ens_site.dat")
    assert f.shape == (2 * len(rows), 3 + 24)
    ens = np.loadtxt(by_site / "dat_ensemble.dat")
    for i, (q, prof) in enumerate(rows):
        for k in (0, 1):
            row = f[2 * i + k]
            assert row[0] == ens[i, 0] and row[1] == k + 1 and row[2] == q["thickness"]["count"][k] == members[k], (i, k)
            want = np.array([[q[n][k][fld] for fld in ("mean", "min", "max", "std")] for n in slots])
            assert printed(row[3:], want), (i, k)
            for name in arrays:
                p = np.loadtxt(by_site / f"dat_ens_profile_{name}_site{k + 1:02d}.dat")
                assert p.shape == (len(rows), 1 + 5 * nbins), name
                x, w = p[i, 1:].reshape(nbins, 5), prof[k][name]
                assert np.array_equal(x[:, 0], w["count"]) and w["count"][0] == members[k], (name, i, k)
                assert printed(x[:, 1:], np.stack([w[fld] for fld in ("mean", "min", "max", "std")], axis=1)), (name, i, k)
    # (two days from open water the columns of a site still agree to the last digits: what tells the sites apart in the files
    # is their number of columns)
