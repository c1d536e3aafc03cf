"""The Beer-law pass (sweep_beer, samsim_sweeps_fused.h) walks a column that follows the grid rule by stretches -- layer 1, top block,
elastic block, bottom block -- with the factor exp(-extinc * thick) formed once per stretch and the multiply alone inside; with a
scalar layer count where the lanes of a wave agree on N_active and up to the wave's maximum where they do not; not at all where no
lane of the wave has short-wave radiation to absorb (polar night, or a snow cover that lets nothing through).  None of these
choices may show in a column's bits, and the flux must be the reference's.

Five waves of 64 brine-saturated slabs at Nlayer 80 = 20+40+20 on bare ice or under thin snow, with thick(1), thick_0 and the
elastic thickness all different (so that a factor taken from the wrong stretch shows):
  wave 0  N_active over {80, 2, 3, 20, 21, 22, 60, 61, 79}: a column ends on each stretch boundary, one layer past it and inside
          each stretch; bare ice (the pass in front of the fused down sweep)
  wave 1  every lane N_active 80 (the scalar count), bare ice
  wave 2  wave 0 with one hand-made column (a layer off the grid rule): the whole wave takes the unfused order, whose gravity
          drainage carries a Beer loop of its own (sweep_grav_drain, untouched) -- a check that the two forms agree, not a run of
          sweep_beer's per-layer branch, which a hand-made column only reaches in a configuration without gravity drainage
  wave 3  wave 0 under 3 mm of snow: the coupling of a thin snow cover moves the pass into the down sweep
  wave 4  every lane N_active 60 under thin snow
run on the SHEBA forcing at a daylight clock (day 300) and with the short-wave table set to zero (the same clock, dark)."""
import os

import numpy as np
import pytest

import samsim_amd
from samsim_amd import testcases as tcs
from samsim_amd.capi import SCALARS, State
from tests.helpers import RTOL, assert_state_close, load_checkpoint, sheba_forcing
from tests.oracle_lib import oracle_solver

pytestmark = pytest.mark.gpu

NTHREADS = min(16, len(os.sched_getaffinity(0)))
WAVE = 64
NLAYER, N_TOP, N_BOTTOM = 80, 20, 20
NSTEPS = 24
NA_SET = [80, 2, 3, 20, 21, 22, 60, 61, 79]
EXTINC, PENETR = 2.0, 0.30          # mo_parameters.f90
SC = {n: i for i, n in enumerate(SCALARS)}
ARRS = ["H_abs", "S_abs", "m", "thick", "T", "phi", "psi_s", "psi_l", "psi_g", "S_bu"]


def slab(cfg, n, th1, th_mid, S_bu):
    """n layers on the grid rule: H_abs, S_abs, m, thick of a saturated slab, -15 C at the top to -1.9 C at the bottom, and a
    bottom layer with a solid fraction of 0.03 (between the two thresholds of layer_dynamics: the grid neither grows nor melts a
    layer in the first steps)"""
    k = np.arange(1, n + 1)
    th = np.where(k == 1, th1, np.where((k > N_TOP) & (k <= NLAYER - N_BOTTOM), th_mid, cfg.thick_0))
    T = -15.0 + (15.0 - 1.9) * (k - 0.5) / n
    Tb = -0.3
    for _ in range(50):   # S_br(Tb) = S_bu / (1 - 0.03), Newton on the sea-salt liquidus, mo_thermo_functions.f90:324-326
        Tb = Tb - (-18.7 * Tb - 0.519 * Tb ** 2 - 0.00535 * Tb ** 3 - S_bu / 0.97) / (-18.7 - 1.038 * Tb - 0.01605 * Tb ** 2)
    T[-1] = Tb
    S_br = -18.7 * T - 0.519 * T ** 2 - 0.00535 * T ** 3
    phi = 1.0 - S_bu / S_br
    H = -tcs.LATENT_HEAT + tcs.LATENT_HEAT * S_bu / S_br + 2020.0 * T + 7.6973 * T * T / 2.0
    m = th / (phi / 920.0 + (1.0 - phi) / tcs.RHO_L)
    return H * m, S_bu * m, m, th


def five_waves():
    cfg, _ = tcs.testcase4(1, nlayer=NLAYER, n_top=N_TOP, n_bottom=N_BOTTOM)
    _, clock = load_checkpoint("sheba_ensemble_80_day300.npz")
    ncol = 5 * WAVE
    lay = np.zeros((4, NLAYER, ncol))
    scal = np.zeros((len(SCALARS), ncol))
    na = np.zeros(ncol, dtype=np.int32)
    for c in range(ncol):
        w, i = divmod(c, WAVE)
        n = 80 if w == 1 else (60 if w == 4 else NA_SET[i % len(NA_SET)])
        th1, th_mid, S_bu = 0.009 + 0.006 * (i % 7) / 7.0, 0.012 + 0.02 * (i % 5) / 5.0, 4.0 + 2.0 * i / (WAVE - 1)
        cols = slab(cfg, n, th1, th_mid, S_bu)
        for a in range(4):
            lay[a, :n, c] = cols[a]
        na[c] = n
        if w >= 3:      # 3 mm of dry snow at -12 C
            ms = 330.0 * 0.003
            for name, v in dict(m_snow=ms, thick_snow=0.003, H_abs_snow=ms * (2020.0 * -12.0 - tcs.LATENT_HEAT), T_snow=-12.0,
                                phi_s=1.0, psi_s_snow=330.0 / 920.0, psi_g_snow=1.0 - 330.0 / 920.0).items():
                scal[SC[name], c] = v
    # the hand-made column of wave 2: a lane with N_active 80, its fifth layer a fifth thicker than the rule says
    odd = 2 * WAVE + NA_SET.index(80) + len(NA_SET)
    assert na[odd] == 80
    for a in (0, 1, 2, 3):
        lay[a, 4, odd] *= 1.2
    return cfg, State(lay, scal, na), clock


def run(make, cfg, st, clock, nsteps, fl_sw_scale=1.0, sites=None):
    s = make(cfg, st.ncol)
    if hasattr(s, "set_threads"):
        s.set_threads(NTHREADS)
    sw, lw, t2, pr = sheba_forcing()
    if sites is None:
        s.set_forcing(sw * fl_sw_scale, lw, t2, pr, None, None)
    else:       # set 0 dark, set 1 daylight
        s.set_forcing_sites(np.stack([sw * 0.0, sw]), np.stack([lw, lw]), np.stack([t2, t2]), np.stack([pr, pr]), sites, None, None)
    s.set_state(st)
    s.set_clock(**clock)
    s.set_output_window(0, 0)
    assert s.steps_to_output() > nsteps        # (an output step takes the unfused order)
    s.step(nsteps)
    out, status = s.get_state(), s.get_status()[0]
    s.close()
    return out, status


@pytest.fixture(scope="module")
def waves():
    return five_waves()


@pytest.fixture(scope="module")
def gpu_runs(waves):
    """the five waves after NSTEPS steps and after one step, in daylight and in the dark"""
    cfg, st, clock = waves
    return {(n, d): run(samsim_amd.hip_solver, cfg, st, clock, n, d) for n in (NSTEPS, 1) for d in (1.0, 0.0)}


@pytest.mark.parametrize("daylight", [1.0, 0.0], ids=["daylight", "dark"])
def test_the_waves_match_the_oracle(waves, gpu_runs, daylight):
    cfg, st, clock = waves
    got, status = gpu_runs[(NSTEPS, daylight)]
    want, ostatus = run(oracle_solver, cfg, st, clock, NSTEPS, daylight)
    assert not status.any() and np.array_equal(status, ostatus)
    sw = got.sc("fl_sw")
    assert (sw > 100.0).all() if daylight else (sw == 0.0).all()
    assert_state_close(got, want, RTOL, what="Beer pass, five waves vs oracle")


def test_the_flux_is_the_sequential_product(waves, gpu_runs):
    """One step in daylight against one step in the dark from the same state: the short-wave flux reaches the layers below the
    first through fl_rad(N_active) alone (the surface balance it also enters feeds layer 1), which the conductive update adds to
    every layer as fl_rad * dt.  So H_abs(k) of the two runs differs by fl_rad * dt for k >= 2, and fl_rad is
    beer0 * prod_{k < Na} e_k * (1 - e_Na), e_k = exp(-extinc * thick(k)), beer0 = penetr * (1 - albedo) * fl_sw.
    The difference of two H_abs (|H_abs| < 1e7 J/m2, one ulp 2e-9) divided by dt = 10 s carries an absolute error below 1e-9
    W/m2 on a flux of 1e-2 .. 1 W/m2; the bar is the project's 1e-6 relative.  A pass that stops one layer early or takes the factor
    of the neighbouring stretch is off by 2 % or more."""
    cfg, st, _ = waves
    (day, sd), (dark, sk) = gpu_runs[(1, 1.0)], gpu_runs[(1, 0.0)]
    assert not sd.any() and not sk.any()
    assert np.array_equal(day.n_active, st.n_active) and np.array_equal(dark.n_active, st.n_active)
    beer0 = PENETR * (1.0 - day.sc("albedo")) * day.sc("fl_sw")
    assert (beer0 > 1.0).all()
    worst = 0.0
    for c in range(st.ncol):
        n = int(st.n_active[c])
        e = np.exp(-EXTINC * st.arr("thick")[:n, c])
        t = beer0[c]
        for k in range(n - 1):
            t = t * e[k]
        want = t - t * e[n - 1]
        got = (day.arr("H_abs")[1:n, c] - dark.arr("H_abs")[1:n, c]) / cfg.dt
        err = np.max(np.abs(got - want)) / want
        worst = max(worst, err)
        assert err <= RTOL, f"column {c} (wave {c // WAVE}, N_active {n}): fl_rad {got} W/m2, expected {want}"
    print(f"fl_rad against the sequential product: worst relative error {worst:.2e}")


def test_a_lane_does_not_depend_on_how_its_wave_counts_layers(waves, gpu_runs):
    """Every column of waves 0 and 3 (mixed N_active: the wave runs to its maximum) again in a wave of 64 copies of itself (one
    N_active: the scalar count): the same bits."""
    cfg, st, clock = waves
    mixed, _ = gpu_runs[(NSTEPS, 1.0)]
    reps = [w * WAVE + i for w in (0, 3) for i in range(len(NA_SET))]
    rep = State(np.ascontiguousarray(np.repeat(st.lay[:, :, reps], WAVE, axis=2)),
                np.ascontiguousarray(np.repeat(st.scal[:, reps], WAVE, axis=1)), np.ascontiguousarray(np.repeat(st.n_active[reps], WAVE)))
    solo, status = run(samsim_amd.hip_solver, cfg, rep, clock, NSTEPS)
    assert not status.any()
    assert np.array_equal(solo.n_active, np.repeat(mixed.n_active[reps], WAVE))
    assert np.array_equal(solo.scal, np.repeat(mixed.scal[:, reps], WAVE, axis=1)), "scalars depend on the wave-mates"
    act = np.arange(NLAYER)[:, None] < mixed.n_active[reps][None, :]
    for name in ARRS:
        a = np.where(act, mixed.arr(name)[:, reps], 0.0)
        b = np.where(np.repeat(act, WAVE, axis=1), solo.arr(name), 0.0)
        assert np.array_equal(b, np.repeat(a, WAVE, axis=1)), f"{name} depends on the wave-mates"


def test_the_dark_wave_skips_the_pass_with_the_bits_of_the_walk(waves):
    """Two forcing sets, one with the short-wave table at zero: all columns on the dark set (no lane has anything to absorb: the
    pass returns at once) against the same with the last lane of every wave in daylight (the wave walks its columns).  The dark
    lanes must not notice."""
    cfg, st, clock = waves
    all_dark = np.zeros(st.ncol, dtype=np.int32)
    one_lit = all_dark.copy()
    one_lit[WAVE - 1::WAVE] = 1
    a, sa = run(samsim_amd.hip_solver, cfg, st, clock, NSTEPS, sites=all_dark)
    b, sb = run(samsim_amd.hip_solver, cfg, st, clock, NSTEPS, sites=one_lit)
    assert not sa.any() and not sb.any()
    keep = one_lit == 0
    assert (a.sc("fl_sw") == 0.0).all() and (b.sc("fl_sw")[~keep] > 100.0).all()
    assert np.array_equal(a.n_active, b.n_active)
    assert np.array_equal(a.scal[:, keep], b.scal[:, keep])
    act = (np.arange(NLAYER)[:, None] < a.n_active[None, :])[:, keep]
    for name in ARRS:
        assert np.array_equal(np.where(act, a.arr(name)[:, keep], 0.0), np.where(act, b.arr(name)[:, keep], 0.0)), name
    lit = ~keep
    assert not np.array_equal(a.arr("H_abs")[:2, lit], b.arr("H_abs")[:2, lit])      # (the lit lanes did absorb something)


def test_short_columns(waves):
    """N_active 1 and 2: a column of one layer has no gravity drainage, so its lanes take the stand-alone pass inside the unfused
    order while their wave-mates take the one fused with the drainage; a wave of one-layer columns takes it with the scalar count."""
    cfg, _, clock = waves
    ncol = 2 * WAVE
    lay = np.zeros((4, NLAYER, ncol))
    na = np.zeros(ncol, dtype=np.int32)
    for c in range(ncol):
        w, i = divmod(c, WAVE)
        n = 1 if w == 1 else 1 + (i % 3 != 0)
        cols = slab(cfg, n, 0.009 + 0.006 * (i % 7) / 7.0, 0.0, 4.0 + 2.0 * i / (WAVE - 1))
        for a in range(4):
            lay[a, :n, c] = cols[a]
        na[c] = n
    st = State(lay, np.zeros((len(SCALARS), ncol)), na)
    got, status = run(samsim_amd.hip_solver, cfg, st, clock, NSTEPS)
    want, ostatus = run(oracle_solver, cfg, st, clock, NSTEPS)
    assert not status.any() and np.array_equal(status, ostatus)
    assert (got.sc("fl_sw") > 100.0).all()
    assert_state_close(got, want, RTOL, what="short columns vs oracle")
