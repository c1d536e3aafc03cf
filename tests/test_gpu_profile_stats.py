"""samsim_get_profile_stats on the GPU: ensemble statistics of the layer profiles by layer and by depth, reduced on the device.
Everything is checked against the numpy restatement of the header's semantics (tests/profile_reference.py) applied to
get_state() of the same handle."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import bench
import samsim_amd
from samsim_amd import testcases as tcs
from samsim_amd.capi import A, ProfileRequest, State
from tests.helpers import ROOT
from tests.profile_reference import column_thickness, profile_reference

pytestmark = pytest.mark.gpu
HOST = os.path.join(ROOT, "host", "samsim_host.x")


def ensemble(fixture, ncol, nsteps, corrupt=()):
    """the perturbed SHEBA ensemble of a stage fixture, its members tiled over ncol columns, stepped nsteps steps"""
    z, st, clock, pert = bench.load_ensemble(fixture)
    cfg, _ = tcs.testcase4(1, nlayer=int(z["nlayer"]), n_top=int(z["n_top"]), n_bottom=int(z["n_bottom"]))
    full = State(bench.tile(st.lay, ncol), bench.tile(st.scal, ncol), bench.tile(st.n_active, ncol).astype(np.int32))
    for c in corrupt:
        full.arr("H_abs")[0, c] = -1.0e15            # getT cannot converge -> STOP 99
    g = samsim_amd.hip_solver(cfg, ncol)
    g.set_forcing(*bench.sheba_forcing(), bench.tile(pert[0], ncol), bench.tile(pert[1], ncol))
    g.set_state(full)
    g.set_clock(**clock)
    g.set_output_window(0, 0)
    if nsteps:
        g.step(nsteps)
    return g


def close(got, want, rel):
    return np.abs(got - want) <= rel * np.maximum(1.0, np.abs(want))


def check(q, r, what, exact_extremes):
    """count exact; min and max exact (stored values, or one IEEE division) or at 1e-12; mean at 1e-12 and std at 1e-10: the
    bars of the scalar statistics (tests/test_gpu_ensemble_io.py)"""
    for name in r:
        g, w = q[name], r[name]
        print(what, name, "count", int(w["count"].min()), "..", int(w["count"].max()),
              "| mean err", float(np.max(np.abs(g["mean"] - w["mean"]) / np.maximum(1.0, np.abs(w["mean"])))),
              "| std err", float(np.max(np.abs(g["std"] - w["std"]) / np.maximum(1e-3, w["std"]))),
              "| min/max err", float(np.max(np.abs(g["min"] - w["min"]))), float(np.max(np.abs(g["max"] - w["max"]))))
        assert np.array_equal(g["count"], w["count"]), (what, name)
        if exact_extremes:
            assert np.array_equal(g["min"], w["min"]) and np.array_equal(g["max"], w["max"]), (what, name)
        else:
            assert close(g["min"], w["min"], 1e-12).all() and close(g["max"], w["max"], 1e-12).all(), (what, name)
        assert close(g["mean"], w["mean"], 1e-12).all(), (what, name)
        assert (np.abs(g["std"] - w["std"]) <= 1e-10 * np.maximum(1e-3, w["std"])).all(), (what, name)


def pick_dz(H, candidates, nbins, z0s):
    """the first bin width for which no column's thickness lies within 1e-9 m of a bin edge: which columns reach into a bin is
    then beyond rounding (a condition on the data, not a tolerance)"""
    for dz in candidates:
        edges = np.concatenate([z0 + np.arange(nbins + 1) * dz for z0 in z0s])
        if np.abs(H[:, None] - edges[None, :]).min() > 1e-9:
            return dz
    return None


def test_by_layer_both_origins_with_stopped_columns():
    ncol = 70001
    g = ensemble("sheba_ensemble_80_day75.npz", ncol, 300, corrupt=(5, 40000, 70000))
    status = g.get_status()[0]
    assert (status != 0).sum() == 3
    s = g.get_state()
    names = ["T", "S_bu", "psi_l", "thick", "H_abs"]
    for origin in ("top", "bottom"):
        r = profile_reference(s, status, names, axis="layer", origin=origin)
        cnt, na_max = r["T"]["count"], int(s.n_active[status == 0].max())
        assert ((cnt > 0) & (cnt < ncol - 3)).any() and (cnt == ncol - 3).any()     # else the test proves nothing
        assert na_max < g.nlayer and (cnt[na_max:] == 0).all() and cnt[na_max - 1] > 0
        check(g.profile_stats(names, axis="layer", origin=origin), r, f"layer/{origin}", exact_extremes=True)


def test_by_depth_both_origins():
    ncol, nbins = 70001, 32
    g = ensemble("sheba_ensemble_80_day345.npz", ncol, 200)
    status = g.get_status()[0]
    s = g.get_state()
    dz = pick_dz(column_thickness(s)[status == 0], (0.07, 0.05, 0.09, 0.11), nbins, (0.0, 0.035))
    assert dz is not None
    names = ["T", "S_bu", "psi_l", "thick"]
    for origin, z0 in (("top", 0.0), ("bottom", 0.0), ("top", 0.035), ("bottom", 0.035)):
        r = profile_reference(s, status, names, axis="depth", origin=origin, nbins=nbins, z0=z0, dz=dz)
        cnt = r["T"]["count"]
        assert ((cnt > 0) & (cnt < cnt.max())).any() and (cnt == 0).any() and cnt.max() == (status == 0).sum()
        check(g.profile_stats(names, axis="depth", origin=origin, nbins=nbins, z0=z0, dz=dz), r, f"depth/{origin}/z0={z0}/dz={dz}",
              exact_extremes=False)


def test_by_depth_more_bins_than_one_pass_holds():
    """100 depth bins are served in two chunks of the reduction: from the top the second chunk begins 1.28 m below the surface,
    from the bottom the first chunk ends in the middle of the columns"""
    ncol, nbins = 5003, 100
    g = ensemble("sheba_ensemble_80_day345.npz", ncol, 200)
    status = g.get_status()[0]
    s = g.get_state()
    dz = pick_dz(column_thickness(s)[status == 0], (0.02, 0.021, 0.019, 0.022), nbins, (0.0, 0.01))
    assert dz is not None
    names = ["T", "S_bu", "thick"]
    for origin, z0 in (("top", 0.0), ("bottom", 0.0), ("top", 0.01), ("bottom", 0.01)):
        r = profile_reference(s, status, names, axis="depth", origin=origin, nbins=nbins, z0=z0, dz=dz)
        cnt = r["T"]["count"]
        assert cnt[:64].max() > 0 and cnt[64:].max() > 0 and (cnt[64:] == 0).any()      # both chunks hold ice, the second ends in water
        assert ((cnt[64:] > 0) & (cnt[64:] < cnt.max())).any()
        check(g.profile_stats(names, axis="depth", origin=origin, nbins=nbins, z0=z0, dz=dz), r, f"depth100/{origin}/z0={z0}/dz={dz}",
              exact_extremes=False)


def test_identical_columns():
    ncol = 256
    cfg, st = tcs.testcase1(ncol)
    g = samsim_amd.hip_solver(cfg, ncol)
    g.set_state(st)
    g.set_clock()
    g.step(2000)
    s = g.get_state()
    na = int(s.n_active[0])
    assert na > 3 and not g.get_status()[0].any()
    names = ["T", "S_bu", "psi_l", "thick"]
    requests = [dict(axis="layer", origin="top"), dict(axis="layer", origin="bottom"),
                dict(axis="depth", origin="top", nbins=40, dz=0.0015), dict(axis="depth", origin="bottom", nbins=40, z0=0.001, dz=0.0015)]
    for kw in requests:
        q = g.profile_stats(names, **kw)
        for n in names:
            x = q[n]
            occ = x["count"] > 0
            assert occ.any() and (x["count"][occ] == ncol).all(), (kw, n)
            assert np.array_equal(x["min"][occ], x["max"][occ]), (kw, n)
            assert (np.abs(x["mean"][occ] - x["min"][occ]) <= 1e-15 * np.abs(x["min"][occ])).all(), (kw, n)
            assert (x["std"][occ] <= 1e-15 * np.abs(x["mean"][occ])).all(), (kw, n)
            if kw["axis"] == "layer":           # the stored values themselves, bit for bit
                col = s.arr(n)[:na, 0]
                assert occ.sum() == na and np.array_equal(x["min"][:na], col if kw["origin"] == "top" else col[::-1]), (kw, n)


def test_deterministic_and_leaves_the_run_alone():
    """two calls return the same bytes; a call between two launches of a handle whose every step is two concurrent launches
    changes nothing of the run"""
    ncol = 1000

    def fresh():
        g = ensemble("sheba_ensemble_80_day75.npz", ncol, 0)
        g.set_launch_split(min_blocks=2)
        return g
    a, b = fresh(), fresh()
    a.step(500)
    names = ["T", "S_bu", "psi_l"]
    for kw in (dict(axis="layer", origin="bottom"), dict(axis="depth", origin="top", nbins=64, dz=0.005)):
        q1, q2 = a.profile_stats(names, **kw), a.profile_stats(names, **kw)
        for n in names:
            assert q1[n].tobytes() == q2[n].tobytes() and q1[n]["count"].max() == ncol, (kw, n)
            assert q1[n]["std"].max() > 0.0
    a.step(500)
    b.step(1000)
    sa, sb = a.get_state(), b.get_state()
    assert np.array_equal(sa.n_active, sb.n_active)
    assert np.array_equal(sa.lay[:4], sb.lay[:4]) and np.array_equal(sa.scal, sb.scal)


def test_full_size_ensemble_beyond_32_bit_offsets():
    """1 048 576 columns of 80 layers (a 10.7 GB layer block), members repeating with period 256 as bench.py uploads them, not
    stepped: every bin holds each member's value 4 096 times"""
    ncol, nbins = 1 << 20, 64
    z, st, clock, pert = bench.load_ensemble("sheba_ensemble_80.npz")
    assert st.ncol == 256 and ncol % st.ncol == 0
    cfg, _ = tcs.testcase4(1, nlayer=int(z["nlayer"]), n_top=int(z["n_top"]), n_bottom=int(z["n_bottom"]))
    g = samsim_amd.hip_solver(cfg, ncol)
    bench.upload_tiled(g, st, ncol, 0)
    members = State.empty(st.ncol, st.nlayer)
    members.lay[:4] = st.lay
    members.n_active[:] = st.n_active
    members.arr("S_bu")[:] = np.nan          # a prognostic-only upload: the bulk salinity must come from S_abs / m
    status = np.zeros(st.ncol, dtype=np.int32)
    dz = pick_dz(column_thickness(members), (0.03, 0.029, 0.031, 0.033), nbins, (0.0,))
    assert dz is not None
    names = ["thick", "S_bu"]
    for kw in (dict(axis="layer", origin="top"), dict(axis="layer", origin="bottom"),
               dict(axis="depth", origin="top", nbins=nbins, dz=dz), dict(axis="depth", origin="bottom", nbins=nbins, dz=dz)):
        r = profile_reference(members, status, names, **kw)
        q = g.profile_stats(names, **kw)
        for n in names:
            assert r[n]["count"].max() == st.ncol and np.array_equal(q[n]["count"], r[n]["count"] * (ncol // st.ncol)), (kw, n)
            print(kw, n, "min/max differ in", int((q[n]["min"] != r[n]["min"]).sum()), int((q[n]["max"] != r[n]["max"]).sum()), "bins")
            # exact on both axes: stored values, or one IEEE division of sums formed in the header's order
            assert np.array_equal(q[n]["min"], r[n]["min"]) and np.array_equal(q[n]["max"], r[n]["max"]), (kw, n)
            assert close(q[n]["mean"], r[n]["mean"], 1e-12).all(), (kw, n)
            assert (np.abs(q[n]["std"] - r[n]["std"]) <= 1e-10 * np.maximum(1e-3, r[n]["std"])).all(), (kw, n)


def test_argument_errors():
    cfg, st = tcs.testcase1(64)
    g = samsim_amd.hip_solver(cfg, 64)
    g.set_state(st)

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
    assert g.profile_stats_raw(request()).shape == (1, 8)
    cases = [(dict(struct_size=C.sizeof(ProfileRequest) - 8), -6), (dict(nbins=0), -1), (dict(nbins=1025), -1), (dict(narrays=9), -1),
             (dict(array0=15), -1), (dict(array0=-1), -1), (dict(dz=0.0), -1), (dict(dz=float("nan")), -1), (dict(z0=-0.01), -1),
             (dict(z0=float("inf")), -1), (dict(axis=2), -1), (dict(origin=2), -1), (dict(axis=0, nbins=cfg.nlayer + 1), -1)]
    for kw, code in cases:
        with pytest.raises(samsim_amd.SamsimError) as e:
            g.profile_stats_raw(request(**kw))
        assert e.value.code == code, kw
    # the layer axis ignores z0 / dz, and takes every layer
    assert g.profile_stats_raw(request(axis=0, nbins=cfg.nlayer, dz=0.0)).shape == (1, cfg.nlayer)


@pytest.mark.skipif(not os.path.exists(HOST), reason="Fortran host not built (no flang)")
def test_fortran_host_profile_files(tmp_path):
    """profile_bins / profile_dz in &samsim_run: one row per output point in dat_ens_profile_{T,S_bu,psi_l}.dat, equal to what the
    Python mirror gets from an identically driven handle; without the keys no such file appears"""
    def run(d, nml):
        d.mkdir()
        (d / "output").mkdir()
        (d / "samsim.nml").write_text(nml)
        r = subprocess.run([HOST], cwd=d, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout
    ncol, nbins, dz, total = 96, 24, 0.05, 12000
    out = run(tmp_path / "prof", f"&samsim_run testcase=1, ncol={ncol}, max_steps={total}, profile_bins={nbins}, profile_dz={dz} /\n")
    assert "on HIP device 0, PCI" in out
    run(tmp_path / "plain", f"&samsim_run testcase=1, ncol={ncol}, max_steps=3700 /\n")
    assert not [f for f in os.listdir(tmp_path / "plain" / "output") if f.startswith("dat_ens_profile")]
    assert np.loadtxt(tmp_path / "prof" / "output" / "dat_ensemble.dat").shape == (4, 26)
    # the same run through the Python mirror (the host's two passive tracers do not act on the ice)
    cfg, st = tcs.testcase1(ncol)
    g = samsim_amd.hip_solver(cfg, ncol)
    g.set_state(st)
    g.set_clock()
    names, rows, done = ["T", "S_bu", "psi_l"], [], 0
    while done < total:
        n = min(g.steps_to_output(), total - done)
        g.step(n)
        done += n
        if g.steps_to_output() == cfg.i_time_out + 1 or done == 1:
            rows.append(g.profile_stats(names, axis="depth", origin="top", nbins=nbins, dz=dz))
    assert len(rows) == 4                                          # outputs at steps 1, 3602, 7203, 10804
    for name in names:
        f = np.loadtxt(tmp_path / "prof" / "output" / f"dat_ens_profile_{name}.dat")
        assert f.shape == (len(rows), 1 + 5 * nbins), name
        f = f[:, 1:].reshape(len(rows), nbins, 5)
        for i, row in enumerate(rows):
            q = row[name]
            assert np.array_equal(f[i, :, 0], q["count"]) and q["count"][0] == ncol and (q["count"][-1] == 0), name
            occ = q["count"] > 0
            assert np.array_equal(f[i, occ, 2], f[i, occ, 3]), name          # identical columns: min == max
            # ES16.8 prints nine digits: half a unit of the ninth
            tol = np.array([0.5e-8 * 10.0 ** math.floor(math.log10(abs(x))) if x != 0.0 else 0.0 for x in q["mean"]]) * (1.0 + 1e-6)
            assert (np.abs(f[i, :, 1] - q["mean"]) <= tol).all(), (name, i)
