"""Parity tests proper: the HIP path (through the C-ABI of include/samsim.h) against the CPU oracle on the same
seeded inputs, against committed golden fixtures, and -- at BASELINE.json's full sizes -- through size-independent
properties.  Bar (BASELINE.json north_star): per-layer T / phi / S within 1e-6 relative; integers (N_active, STOP
codes, step indices) exact."""
import os

import numpy as np
import pytest

import samsim_amd
from samsim_amd import testcases as tcs
from samsim_amd.capi import SCALARS
from tests.helpers import ROOT, RTOL, assert_state_close, golden, load_checkpoint, rel_err, sheba_forcing
from tests.oracle_lib import oracle_solver

pytestmark = pytest.mark.gpu

NTHREADS = min(16, len(os.sched_getaffinity(0)))


def pair(cfg, ncol, st, clock=None, forcing=None, perturb=True, col0=0):
    """a HIP solver and an oracle solver with identical inputs"""
    g = samsim_amd.hip_solver(cfg, ncol)
    o = oracle_solver(cfg, ncol)
    o.set_threads(NTHREADS)
    for s in (g, o):
        if forcing is not None:
            dT, ps = tcs.ensemble_perturbation(ncol, col0) if perturb else (None, None)
            s.set_forcing(*forcing, dT, ps)
        s.set_state(st)
        s.set_clock(**(clock or {}))
    return g, o


def check(g, o, what, rtol=RTOL):
    sg, so = g.get_state(), o.get_state()
    stg, sto = g.get_status()[0], o.get_status()[0]
    assert np.array_equal(stg, sto), f"{what}: STOP codes differ {np.unique(stg)} vs {np.unique(sto)}"
    assert_state_close(sg, so, rtol, what=what)
    return sg, so


def test_tc1_from_open_water_identical_columns():
    """cfg2 in small: testcase-1 forcing replicated to identical columns; every column must stay bitwise equal to
    column 0 and column 0 must follow the oracle (freezing from a single water layer, first regrids)"""
    ncol = 192
    cfg, st = tcs.testcase1(ncol)
    g, o = pair(cfg, ncol, st)
    done = 0
    for upto in (1, 2, 50, 3601, 3602, 20000):
        g.step(upto - done)
        o.step(upto - done)
        done = upto
        sg, so = check(g, o, f"tc1 step {upto}")
        assert (sg.lay == sg.lay[:, :, :1]).all() and (sg.scal == sg.scal[:, :1]).all(), "identical columns diverged"
    assert int(sg.n_active[0]) > 5
    assert g.get_clock().time == o.get_clock().time == 20000.0


def test_tc1_output_snapshots_match_golden_and_oracle():
    """the `output` snapshot (mo_output.f90:129-144) at the first output points: vs oracle and vs the flang reference dump"""
    cfg, st = tcs.testcase1(4)
    g, o = pair(cfg, 4, st)
    g.set_output_window(0, 4)
    o.set_output_window(0, 4)
    ref = golden("tc1_ref_fullprec.npz")
    for i in range(4):
        assert g.steps_to_output() == o.steps_to_output()
        og, oo = g.run_to_output(), o.run_to_output()
        assert og.step == oo.step == ref["step"][i]
        assert np.array_equal(og.n_active, oo.n_active) and og.n_active[0] == ref["N_active"][i]
        na = int(oo.n_active[0])
        for n in ["T", "psi_s", "psi_l", "psi_g", "S_bu", "thick", "ray", "H_abs", "S_abs", "m"]:
            k = na - 1 if n == "ray" else na
            assert rel_err(og.arr(n)[:k], oo.arr(n)[:k]) <= RTOL, f"output {i}: {n} vs oracle"
            assert rel_err(og.arr(n)[:k, 0], ref["a_" + n][i, :k]) <= RTOL, f"output {i}: {n} vs reference dump"
        for n in ["freeboard", "energy_stored", "freshwater", "total_resist", "thickness", "bulk_salin", "grav_drain",
                  "grav_salt", "grav_temp", "T_top"]:
            assert rel_err(og.sc(n), oo.sc(n)) <= RTOL, f"output {i}: scalar {n}"
            assert rel_err(og.sc(n)[0], ref["s_" + n][i]) <= RTOL, f"output {i}: scalar {n} vs reference dump"


def test_tc1_spun_up_state():
    """75 active layers, gravity drainage active in most layers"""
    st1, clock = load_checkpoint("tc1_spunup_state.npz")
    cfg, _ = tcs.testcase1(1)
    ncol = 64
    g, o = pair(cfg, ncol, st1.replicate(ncol), clock)
    g.step(5000)
    o.step(5000)
    sg, so = check(g, o, "tc1 spun-up +5000")
    assert int(so.n_active[0]) >= 60


def test_sheba_from_open_water_perturbed_ensemble():
    """cfg3 in small: SHEBA forcing, perturbed T2m / precipitation per column, first three days (open water, rain and
    snow into water, first ice layers, surface energy balance)"""
    ncol = 64
    cfg, st = tcs.testcase4(ncol)
    g, o = pair(cfg, ncol, st, forcing=sheba_forcing())
    for upto, n in ((1, 1), (8642, 8641), (26000, 17358)):
        g.step(n)
        o.step(n)
        sg, so = check(g, o, f"sheba step {upto}")
    assert len(np.unique(sg.arr("H_abs")[0])) > ncol // 2, "perturbation did not spread the ensemble"


def test_sheba_spun_up_winter():
    """day 200: full-depth ice (N_active = Nlayer region, elastic middle layers), snow cover, bottom growth"""
    st1, clock = load_checkpoint("tc4_spunup_state.npz")
    cfg, _ = tcs.testcase4(1)
    ncol = 64
    g, o = pair(cfg, ncol, st1.replicate(ncol), clock, forcing=sheba_forcing())
    g.step(4000)
    o.step(4000)
    sg, so = check(g, o, "sheba day 200 +4000")
    assert so.sc("thick_snow").min() > 0.0


def test_sheba_melt_season_one_day():
    """day 340 (melt onset): flushing (flush3), snow melt water, melt ponds, flooding checks, top melt regrids;
    one full output interval so that the snapshot path is covered too"""
    st1, clock = load_checkpoint("tc4_melt_state.npz")
    cfg, _ = tcs.testcase4(1)
    ncol = 48
    g, o = pair(cfg, ncol, st1.replicate(ncol), clock, forcing=sheba_forcing())
    g.set_output_window(0, ncol)
    o.set_output_window(0, ncol)
    n = g.steps_to_output()
    assert n == o.steps_to_output()
    og, oo = g.run_to_output(), o.run_to_output()
    assert og.step == oo.step
    for name in ["T", "psi_s", "psi_l", "S_bu", "thick", "perm", "flush_v", "flush_h"]:
        assert rel_err(og.arr(name), oo.arr(name), 1e-7 if name != "perm" else 1e-30) <= RTOL, name
    for name in ["freeboard", "thick_snow", "T_snow", "thickness", "bulk_salin", "melt_out1", "melt_out2"]:
        assert rel_err(og.sc(name), oo.sc(name), 1e-7) <= RTOL, name
    check(g, o, "sheba melt season")
    g.step(3000)
    o.step(3000)
    check(g, o, "sheba melt season +3000")


def test_launch_granularity_does_not_change_results():
    """1000 steps in one launch == 10 launches of 100 == 143 launches of 7 == samsim_steps_timed(50, 20) (bitwise): the uniform
    clock carried by the host and the state carried in HBM are the whole state"""
    st1, clock = load_checkpoint("tc4_spunup_state.npz")
    cfg, _ = tcs.testcase4(1)
    ncol = 128
    res = []
    for chunk in (1000, 100, 7, -50):
        g = samsim_amd.hip_solver(cfg, ncol)
        dT, ps = tcs.ensemble_perturbation(ncol)
        g.set_forcing(*sheba_forcing(), dT, ps)
        g.set_state(st1.replicate(ncol))
        g.set_clock(**clock)
        if chunk < 0:      # samsim_steps_timed: 20 launches of 50 steps enqueued back to back and timed as one region
            assert g.steps_timed(-chunk, 1000 // -chunk) > 0.0
        else:
            done = 0
            while done < 1000:
                n = min(chunk, 1000 - done)
                g.step(n)
                done += n
        res.append((g.get_state(), g.get_clock()))
        g.close()
    for st, clk in res[1:]:
        assert np.array_equal(st.lay, res[0][0].lay) and np.array_equal(st.scal, res[0][0].scal)
        assert np.array_equal(st.n_active, res[0][0].n_active)
        assert (clk.time, clk.step, clk.n_time_out, clk.time_counter) == (
            res[0][1].time, res[0][1].step, res[0][1].n_time_out, res[0][1].time_counter)


def test_state_roundtrip_and_column_windows():
    cfg, st = tcs.testcase4(10)
    rng = np.random.default_rng(7)
    st.lay[:] = rng.random(st.lay.shape)
    st.scal[:] = rng.random(st.scal.shape)
    st.n_active[:] = rng.integers(1, cfg.nlayer + 1, size=10)
    g = samsim_amd.hip_solver(cfg, 10)
    g.set_state(st)
    back = g.get_state()
    nown = len(SCALARS) - 2  # the two perturbation slots are owned by set_forcing
    assert np.array_equal(back.lay, st.lay) and np.array_equal(back.n_active, st.n_active)
    assert np.array_equal(back.scal[:nown], st.scal[:nown])
    assert (back.sc("dT2m") == 0.0).all() and (back.sc("precip_scale") == 1.0).all()
    w = st.window(3, 4)
    w.lay[:] = -1.0
    g.set_state(w, col0=3)
    back = g.get_state()
    assert (back.lay[:, :, 3:7] == -1.0).all() and np.array_equal(back.lay[:, :, :3], st.lay[:, :, :3])
    part = g.get_state(col0=6, ncols=3)
    assert np.array_equal(part.lay, back.lay[:, :, 6:9])
    with pytest.raises(samsim_amd.SamsimError):
        g.set_state(st, col0=5)  # does not fit


def test_failed_columns_are_frozen_and_reported():
    """the reference aborts the whole program with STOP n; here the column records n and freezes while its
    neighbours keep running.  Codes, first failing step and healthy columns must match the oracle."""
    st1, clock = load_checkpoint("tc1_spunup_state.npz")
    cfg, _ = tcs.testcase1(1)
    ncol = 8
    st = st1.replicate(ncol)
    # What the oracle does with each corruption (tests/stop_seeds.py has the seeds that do stop, site by site):
    st.arr("S_abs")[3, 2] = -5.0e3      # strongly negative salt: NO stop -- S_bu < 0 sends getT down its fresh-ice branch, and the first
    #                                     mass_transfer of the expelled brine clamps its transfer to -S_abs, which brings S_abs(4) to 0
    #                                     before gravity drainage tests MINVAL(S_abs); the column runs on with a salt-free layer 4
    st.arr("H_abs")[0, 5] = -1.0e15     # absurd enthalpy: getT of layer 1 cannot converge, STOP 99 in the first step, layer 1
    st.arr("m")[10, 6] = -st.arr("m")[10, 6]  # negative mass: NO stop -- H = H_abs/m > 0 makes the layer liquid (phi = 0), so psi_s(11) is
    #                                     -0.0, which MINVAL(psi_s) < 0 does not catch; the column runs on with its negative mass
    g, o = pair(cfg, ncol, st, clock)
    g.step(300)
    o.step(300)
    (sg, stepg, layg), (so, stepo, layo) = g.get_status(), o.get_status()
    assert np.array_equal(sg, so), (sg, so)
    assert np.array_equal(stepg, stepo), (stepg, stepo)
    assert np.array_equal(layg, layo), (layg, layo)
    assert set(np.nonzero(so)[0]) == {5} and so[5] == 99 and stepo[5] == clock["step"] + 1 and layo[5] == 1, (so, stepo, layo)
    healthy = np.array([0, 1, 3, 4, 7])  # untouched columns next to the corrupted ones
    assert not so[healthy].any()
    a, b = g.get_state(), o.get_state()
    for n in ["H_abs", "S_abs", "T"]:
        assert rel_err(a.arr(n)[:, healthy], b.arr(n)[:, healthy]) <= RTOL
    # a checkpoint carries the STOP codes: after save / load the frozen columns are still frozen and still reported, and the
    # healthy ones continue bit for bit
    import tempfile
    from samsim_amd import checkpoint
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "frozen.chk")
        checkpoint.save(g, path)
        g2 = samsim_amd.hip_solver(cfg, ncol)
        checkpoint.load(g2, path)
    s2, step2, lay2 = g2.get_status()
    assert np.array_equal(s2, sg) and np.array_equal(step2, stepg) and np.array_equal(lay2, layg)
    g.step(100)
    g2.step(100)
    a, b = g.get_state(), g2.get_state()
    frozen = np.nonzero(sg)[0]
    for n in ["H_abs", "S_abs", "m", "thick", "T"]:
        assert np.array_equal(a.arr(n)[:, healthy], b.arr(n)[:, healthy]), n
        assert np.array_equal(a.arr(n)[:, frozen], b.arr(n)[:, frozen]), n
    assert np.array_equal(g2.get_status()[0], sg)


def test_launch_without_forcing_tables_is_refused():
    """atmoflux_flag 2 reads T2m and precipitation from the tables in every step, whatever boundflux_flag says: a step before
    samsim_set_forcing must come back as SAMSIM_ERR_ARG (the kernel is never launched on a null table)"""
    for bf in (1, 2, 3):
        cfg, st = tcs.testcase4(4)
        cfg.boundflux_flag = bf
        g = samsim_amd.hip_solver(cfg, 4)
        g.set_state(st)
        with pytest.raises(samsim_amd.SamsimError) as e:
            g.step(1)
        assert e.value.code == -1, bf


def test_division_and_power_sequences_stay_within_an_ulp_or_four():
    """samsim_div.h forms 1/x and a/b of the sweeps by the arithmetic core of the compiler's division sequence (no operand
    scaling, no special-case fix-up, one Newton step less); samsim_pow.h forms x**3.1 through a hardware-seeded tenth root.
    tools/div_probe (built by __graft_entry__.build()) measures them on the GPU against 1.0/x, a/b and pow(x, 3.1) on 2^26
    operands each: the quotients within ONE ulp (observed: none differs), the two forms of the power within 2.5e-15 of each other"""
    import re
    import subprocess
    exe = os.path.join(ROOT, "tools", "div_probe")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "samsim_amd", "csrc"), "div_probe"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=180)
    assert out.returncode == 0, out.stdout + out.stderr
    print(out.stdout)
    m = re.search(r"recip != 1.0/x: (\d+) \(max (\d+) ulp\)  quot != a/b: (\d+) \(max (\d+) ulp\)", out.stdout)
    assert m, out.stdout
    assert int(m.group(2)) <= 1 and int(m.group(4)) <= 1, out.stdout
    m = re.search(r"max rel err ([0-9.e+-]+) \(plain form ([0-9.e+-]+)\); tenth-root form vs plain form: ([0-9.e+-]+); (\d+) arguments "
                  r"below 2\^-100 \(plain form\): ([0-9.e+-]+)", out.stdout)
    assert m, out.stdout
    # the plain form is pinned on the CPU against the exact power (tests/test_host_logic.py: 7e-16); the tenth-root form against it here
    assert float(m.group(3)) <= 2.5e-15, out.stdout     # (each form is within ~4 ulp of the exact power: observed 1.8e-15 apart)
    assert float(m.group(1)) <= 2e-14 and float(m.group(2)) <= 2e-14, out.stdout     # (the device's own pow() is good to ~7e-15)
    assert int(m.group(4)) > 1000 and float(m.group(5)) <= 1e-13, out.stdout         # liquid fractions below 1e-33: |log x| up to 200


def test_unsupported_flags_are_rejected():
    for flag, value in (("prescribe_flag", 3), ("flush_flag", 3), ("lab_snow_flag", 1)):
        cfg, _ = tcs.testcase2(1) if flag == "lab_snow_flag" else tcs.testcase1(1)
        setattr(cfg, flag, value)
        with pytest.raises(samsim_amd.SamsimError) as e:
            samsim_amd.hip_solver(cfg, 4)
        assert e.value.code == -2, flag
    cfg, st = tcs.testcase1(4)
    cfg.bgc_flag = 2                     # tracers on, but samsim_set_tracers not called: the step is refused
    g = samsim_amd.hip_solver(cfg, 4)
    g.set_state(st)
    with pytest.raises(samsim_amd.SamsimError) as e:
        g.step(1)
    assert e.value.code == -1
    cfg, _ = tcs.testcase1(1)
    cfg.struct_size = 8
    with pytest.raises(samsim_amd.SamsimError) as e:
        samsim_amd.hip_solver(cfg, 4)
    assert e.value.code == -6


def test_full_size_cfg2_replicas_stay_identical():
    """BASELINE cfg2 size: 65 536 identical testcase-1 columns.  Property: every column equals column 0 bitwise after
    2 000 steps (no cross-column interference at full occupancy), and column 0 equals the oracle."""
    st1, clock = load_checkpoint("tc1_spunup_state.npz")
    cfg, _ = tcs.testcase1(1)
    ncol = 65536
    g = samsim_amd.hip_solver(cfg, ncol)
    rep = st1.replicate(8192)
    for c0 in range(0, ncol, 8192):
        g.set_state(rep, c0)
    g.set_clock(**clock)
    g.step(2000)
    sg = g.get_state()
    assert not g.get_status()[0].any()
    assert (sg.lay == sg.lay[:, :, :1]).all() and (sg.n_active == sg.n_active[0]).all()
    o = oracle_solver(cfg, 1)
    o.set_state(st1)
    o.set_clock(**clock)
    o.step(2000)
    assert_state_close(sg.window(0, 1), o.get_state(), what="cfg2 column 0")
    cells, colsteps = g.get_work()
    assert colsteps == (clock["step"] + 2000) * ncol and cells == 2000 * int(sg.n_active[0]) * ncol


def test_full_size_cfg3_million_columns_properties():
    """BASELINE cfg3 size: 1 048 576 SHEBA columns.  The perturbation is made periodic with period 4096, so column c and
    c + 4096 must agree bitwise wherever they run on the chip; column 0..63 are checked against the oracle; no column may
    trip the per-step energy-conservation assert (mo_heat_fluxes.f90:265-310, STOP 431) or any other STOP."""
    st1, clock = load_checkpoint("tc4_spunup_state.npz")
    cfg, _ = tcs.testcase4(1)
    ncol, period, nsteps = 1 << 20, 4096, 300
    dT, ps = tcs.ensemble_perturbation(period)
    dT, ps = np.tile(dT, ncol // period), np.tile(ps, ncol // period)
    g = samsim_amd.hip_solver(cfg, ncol)
    g.set_forcing(*sheba_forcing(), dT, ps)
    rep = st1.replicate(16384)
    for c0 in range(0, ncol, 16384):
        g.set_state(rep, c0)
    g.set_clock(**clock)
    g.step(nsteps)
    assert not g.get_status()[0].any()
    first = g.get_state(0, period, narr=4)
    for c0 in (period, 37 * period, ncol - period):
        other = g.get_state(c0, period, narr=4)
        assert np.array_equal(other.lay, first.lay) and np.array_equal(other.n_active, first.n_active)
    o = oracle_solver(cfg, 64)
    o.set_threads(NTHREADS)
    o.set_forcing(*sheba_forcing(), dT[:64], ps[:64])
    o.set_state(st1.replicate(64))
    o.set_clock(**clock)
    o.step(nsteps)
    assert_state_close(g.get_state(0, 64), o.get_state(), what="cfg3 columns 0..63")


def test_headline_workload_at_full_size_against_the_oracle():
    """The configuration bench.py times, as bench.py builds it (its own `workload` / `upload_tiled`): 1 048 576 columns x 80 layers
    (20 + 40 + 20), the 256-member spun-up SHEBA ensemble tiled over the columns, one bench step of 500 time steps with the two
    concurrent launches of a large handle.  Every member against the oracle (256 columns x 500 steps on the CPU), and the copies of
    a member bitwise equal wherever they ran -- first, middle and last block of the handle, both launch halves."""
    import argparse
    import bench
    a = argparse.Namespace(workload="sheba", nlayer=80)
    cfg, st, pert, clock, forcing, _, _ = bench.workload(a)
    ncol, nmem, nsteps = 1 << 20, st.ncol, 500
    assert cfg.nlayer == 80 and nmem == 256
    g = samsim_amd.hip_solver(cfg, ncol)
    g.set_forcing(*forcing, bench.tile(pert[0], ncol), bench.tile(pert[1], ncol))
    bench.upload_tiled(g, st, ncol, 0)
    g.set_clock(**clock)
    g.set_output_window(0, 0)
    g.step(nsteps)
    assert not g.get_status()[0].any()
    first = g.get_state(0, nmem)
    for c0 in (nmem, ncol // 2 - nmem, ncol // 2, ncol - nmem):
        other = g.get_state(c0, nmem)
        assert np.array_equal(other.lay, first.lay) and np.array_equal(other.scal, first.scal) and np.array_equal(other.n_active, first.n_active), c0
    o = oracle_solver(cfg, nmem)
    o.set_threads(NTHREADS)
    o.set_forcing(*forcing, pert[0], pert[1])
    from samsim_amd.capi import State
    o.set_state(State(st.lay, st.scal, st.n_active.astype(np.int32)))
    o.set_clock(**clock)
    o.step(nsteps)
    assert_state_close(first, o.get_state(), what="headline workload, members 0..255")


def _ensemble(nlayer, n):
    """first n members of the spun-up perturbed SHEBA ensemble fixture (prognostic arrays only)"""
    from samsim_amd.capi import State
    z = golden(f"sheba_ensemble_{nlayer}.npz")
    cfg, _ = tcs.testcase4(1, nlayer=int(z["nlayer"]), n_top=int(z["n_top"]), n_bottom=int(z["n_bottom"]))
    st = State(np.ascontiguousarray(z["lay"][:, :, :n]), np.ascontiguousarray(z["scal"][:, :n]),
               np.ascontiguousarray(z["n_active"][:n]))
    clock = dict(time=float(z["time"]), step=int(z["step"]), n_time_out=int(z["n_time_out"]),
                 time_counter=int(z["time_counter"]), n_outputs=int(z["n_outputs"]))
    return cfg, st, clock, z["dT2m"][:n], z["precip_scale"][:n]


@pytest.mark.parametrize("nlayer", [100, 80])
def test_spun_up_ensemble_members(nlayer):
    """the bench workload in small: genuinely different columns (1.4-1.6 m of ice, 9-16 cm of snow) restarted from their
    prognostic arrays only (the carried diagnostics are rebuilt by the first sweep), Nlayer 100 and the 80-layer
    headline geometry (20 + 40 + 20)"""
    n = 64
    cfg, st, clock, dT, ps = _ensemble(nlayer, n)
    g = samsim_amd.hip_solver(cfg, n)
    o = oracle_solver(cfg, n)
    o.set_threads(NTHREADS)
    for s in (g, o):
        s.set_forcing(*sheba_forcing(), dT, ps)
        s.set_state(st)
        s.set_clock(**clock)
    g.step(3000)
    o.step(3000)
    sg, so = check(g, o, f"ensemble Nlayer {nlayer}")
    assert len(np.unique(so.arr("H_abs")[cfg.n_top + 5])) == n   # members really differ


def test_cfg5_nlayer500_all_brine_processes():
    """BASELINE cfg5 in small: Nlayer 500 (20 + 460 + 20), dt 2 s, every layer active, heavy snow (flooding), a
    temperature gradient (gravity drainage), SHEBA forcing in the melt season"""
    n = 32
    cfg, st, clock = tcs.config5(n, nlayer=500)
    g, o = pair(cfg, n, st, clock, forcing=sheba_forcing())
    g.step(1500)
    o.step(1500)
    sg, so = check(g, o, "cfg5 Nlayer 500")
    assert so.sc("grav_drain").min() > 0.0 and so.arr("thick")[0].min() > cfg.thick_0   # drainage and flooding fired


def test_full_size_cfg5_quarter_million_columns():
    """BASELINE cfg5 size: 262 144 columns x 500 layers (20 GB of state).  Periodic perturbation (period 1024): column c
    and c + 1024 must agree bitwise; no STOP code; columns 0..15 against the oracle."""
    ncol, period, nsteps = 262144, 1024, 30
    cfg, st1, clock = tcs.config5(1, nlayer=500)
    dT, ps = tcs.ensemble_perturbation(period)
    dT, ps = np.tile(dT, ncol // period), np.tile(ps, ncol // period)
    g = samsim_amd.hip_solver(cfg, ncol)
    g.set_forcing(*sheba_forcing(), dT, ps)
    rep = st1.replicate(4096)
    for c0 in range(0, ncol, 4096):
        g.set_state(rep, c0)
    g.set_clock(**clock)
    g.step(nsteps)
    assert not g.get_status()[0].any()
    first = g.get_state(0, period, narr=4)
    for c0 in (period, 100 * period, ncol - period):
        other = g.get_state(c0, period, narr=4)
        assert np.array_equal(other.lay, first.lay)
    o = oracle_solver(cfg, 16)
    o.set_threads(NTHREADS)
    o.set_forcing(*sheba_forcing(), dT[:16], ps[:16])
    o.set_state(st1.replicate(16))
    o.set_clock(**clock)
    o.step(nsteps)
    assert_state_close(g.get_state(0, 16), o.get_state(), what="cfg5 columns 0..15")


def test_sheba_melt_season_teacher_forced_windows():
    """the melt season is chaotic in a free run (a 1e-15 difference is amplified to 1e-4 within a
    few hundred steps once thin snow couples to a surface layer sitting at the psi_s = 0.4 melt threshold), so parity is
    asserted teacher-forced: the HIP path is restarted from the oracle's state and must agree 1 000 steps later.
    Every 3rd day of days 340..440 of the SHEBA run: melt onset, snow melt, flushing, melt ponds, top and bottom melt
    regrids (N_active 100 -> below 45), first refreezing; 16 perturbed columns."""
    st1, clock = load_checkpoint("tc4_melt_state.npz")   # oracle checkpoint at day 340
    cfg, _ = tcs.testcase4(1)
    n, window = 16, 1000
    dT, ps = tcs.ensemble_perturbation(n)
    o = oracle_solver(cfg, n)
    o.set_threads(NTHREADS)
    o.set_forcing(*sheba_forcing(), dT, ps)
    o.set_state(st1.replicate(n))
    o.set_clock(**clock)
    g = samsim_amd.hip_solver(cfg, n)
    g.set_forcing(*sheba_forcing(), dT, ps)
    na_seen = set()
    for day in range(340, 440):
        if (day - 340) % 3 == 0:
            k = o.get_clock()
            g.set_state(o.get_state())
            g.set_clock(time=k.time, step=k.step, n_time_out=k.n_time_out, time_counter=k.time_counter, n_outputs=k.n_outputs)
            g.step(window)
            o.step(window)
            sg, so = check(g, o, f"teacher-forced day {day}", rtol=1e-6)
            na_seen.update(int(v) for v in so.n_active)
            o.step(8640 - window)
        else:
            o.step(8640)
    assert min(na_seen) < 50 and max(na_seen) == 100, na_seen   # the regrids really happened inside the tested span


def test_per_column_ocean_grid_of_columns():
    """samsim_set_ocean: a grid of 64 columns over oceans of different heat flux and salinity (KShebaSites instantiation), from
    open water through freeze-up against the oracle; column 0 (no offset, cfg.S_bu_bottom) equals the single-ocean run bitwise"""
    ncol = 64
    cfg, st = tcs.testcase4(ncol)
    rng = np.random.default_rng(11)
    dq = rng.uniform(-4.0, 8.0, ncol)
    sb = rng.uniform(28.0, 36.0, ncol)
    dq[0], sb[0] = 0.0, cfg.S_bu_bottom
    g, o = pair(cfg, ncol, st, forcing=sheba_forcing())
    for s in (g, o):
        s.set_ocean(dq, sb)
    # Free run through open water to the first ice (day 64), then windows restarted from the checker's state.  Why windows: two
    # events of the freeze-up amplify round-off -- the first ice layer (day 64-65) and the first snow growing through thick_min on
    # three to five layers of ice (day 66-67: the thin-snow coupling's fixed-size enthalpy steps, then the switch of the surface
    # balance at thick_min).  profiles/r3_freeze_up_*.json shows it without any GPU: the checker against its own
    # -ffp-contract=fast build, same 64 columns, parts by up to 3e-4 in 10 columns exactly there in a free run (which is what round
    # 2's free run to day 75 had met: 4e-5); a window of only 1 500 steps started at day 67, when the snow of several columns is
    # within a few per cent of thick_min, already shows 2e-3 (profiles/r3_freeze_up_windows_days64_68.json; the HIP path: 3e-4),
    # the 1 500-step windows of days 64, 65, 66 and 68 stay below 1e-13, and so does every ONE-DAY window from day 68 on
    # (profiles/r3_freeze_up_windows_1day.json: 3e-13).  So: 1 500-step windows at days 64, 65, 66 at the parity bar, the one at
    # day 67 held to the size of that event (4e-3: twice the 2e-3 of the two CPU builds, thirteen times the HIP path's 3e-4), and
    # from day 68 one-day windows every second day at 1e-9, like the main path's windows from the reference's records.  The parity
    # bar THROUGH day 67 -- every step of it, in 864 ten-step windows in which nothing is amplified -- is held by
    # tests/test_gpu_event_windows.py::test_ocean_grid_day_67_first_snow_through_thick_min.
    n = 8641 * 64
    g.step(n)
    o.step(n)
    sg, so = check(g, o, "ocean grid, day 64")
    assert np.array_equal(sg.sc("S_bu_bottom"), sb)
    spread = set()
    worst_late = 0.0
    day = 64
    while day < 100:
        k = o.get_clock()
        assert k.step == 8641 * day
        window = 1500 if day < 68 else 8641
        g.set_state(o.get_state())
        g.set_clock(time=k.time, step=k.step, n_time_out=k.n_time_out, time_counter=k.time_counter, n_outputs=k.n_outputs)
        g.step(window)
        o.step(window)
        sg, so = check(g, o, f"ocean grid, {window} steps from day {day}", rtol=4e-3 if day == 67 else 1e-6)
        spread.update(int(v) for v in so.n_active)
        if day >= 68:
            kk = np.arange(sg.nlayer)[:, None] < so.n_active[None, :]
            for name in ("H_abs", "S_abs", "m", "thick", "T"):
                floor = 1e-3 if name == "H_abs" else 1e-9
                worst_late = max(worst_late, rel_err(sg.arr(name)[kk], so.arr(name)[kk], floor))
        step_to = 1 if day < 68 else 2
        o.step(8641 * step_to - window)
        day += step_to
    print(f"ocean grid: worst one-day window from day 68 on {worst_late:.2e}")
    assert worst_late <= 1e-9
    assert len(spread) > 8                                                  # the oceans spread the ensemble
    assert abs(float(sg.sc("fl_q_bottom")[5] - sg.sc("fl_q_bottom")[0]) - dq[5]) < 1e-12
    # column 0 (no offset, cfg.S_bu_bottom) is the single-ocean column, bit for bit
    n = 8641 * 64
    g2 = samsim_amd.hip_solver(cfg, ncol)
    dT, ps = tcs.ensemble_perturbation(ncol)
    g2.set_forcing(*sheba_forcing(), dT, ps)
    g2.set_ocean(dq, sb)
    g2.set_state(st)
    g2.set_clock()
    g2.step(n)
    sg = g2.get_state()
    plain = samsim_amd.hip_solver(cfg, ncol)
    plain.set_forcing(*sheba_forcing(), dT, ps)
    plain.set_state(st)
    plain.set_clock()
    plain.step(n)
    sp = plain.get_state()
    for name in ("H_abs", "S_abs", "m", "thick", "T"):
        assert np.array_equal(sp.arr(name)[:, 0], sg.arr(name)[:, 0]), name
    with pytest.raises(samsim_amd.SamsimError) as e:
        cfg2, _ = tcs.testcase2(4)
        samsim_amd.hip_solver(cfg2, 4).set_ocean(None, np.full(4, 30.0))
    assert e.value.code == -2
