"""Melt onset: the steps in which the fused down sweep's stored-row decision changes its answer.

The fixed-flag SHEBA kernels store psi_s / psi_l / psi_g of layers >= 3 only where the finished top layer says that something will
read them later in the step (sweep_down_fused, samsim_sweeps_fused.h).  The in-step readers are func_freeboard and flush3, and what
lets them run is, on the state a step leaves behind, the LATE-READER CONDITION

    psi_s(1) < psi_s_top_min (0.4)  ||  T_top >= T_freeze  ||  melt_thick_snow > 0  ||  melt_thick > 1e-12

(`late_reader_terms`).  An ONSET is a step after which the condition holds in a column in which it did not hold before the step.

This module holds what the CPU test (tests/test_melt_onset_host.py) and the GPU test (tests/test_gpu_melt_onset.py) share:

  * the committed wave tests/golden/melt_onset_wave_80.npz (tests/golden/make_melt_onset_fixtures.py): 70 columns, each a state of
    one ensemble member a few steps before an onset, all under one clock, so that the columns of a wave disagree about the decision
    in most of the 24 steps;
  * crafted LEADERS: one column per term of the condition in which that term alone holds in the onset step, and a TWIN on the
    other side of the threshold in which no reader fires -- or, in NO_LEADER, the reason the oracle gives why no finite state
    isolates the term.

Rules of a mutation, as in tests/stop_seeds.py: finite values only; only H_abs, S_abs, m, thick of ACTIVE layers and the snow scalars
(m_snow, H_abs_snow, S_abs_snow, thick_snow); n_active is never touched.
"""
from dataclasses import dataclass
from typing import Callable

import numpy as np

from samsim_amd import testcases as tcs
from samsim_amd.capi import S, State
from tests.helpers import assert_state_close, golden, sheba_forcing

NCOL = 70               # one full 64-column block and a partial block of 6 (stop_seeds.NCOL)
NSTEPS = 24
MIN_LEAD, MAX_LEAD = 2, 17      # never below 2: the first step after samsim_set_state takes the full first sweep
# two waves with two clocks: no clock gives both onsets spread over steps 2..17 and melt water in the onset step
# (tests/golden/make_melt_onset_fixtures.py)
# `melt_bare` is the melt wave with its snow taken away (the snow scalars set to 0, by the rules of a mutation): every column of
# `melt` carries 0 < thick_snow < thick_min, under which the sweep stores the rows whatever the other terms say; on bare ice the
# T_top term alone decides, in the step in which flush3 reads the rows
WAVES = {"spread": "melt_onset_wave_80.npz", "melt": "melt_onset_wave_80_melt.npz", "melt_bare": "melt_onset_wave_80_melt.npz"}
WAVE = WAVES["spread"]
TERMS = ("psi_s_top", "T_top", "melt_thick_snow", "melt_thick")
PSI_S_TOP_MIN = 0.4
PERTURBATIONS = (1.0e-13, -1.0e-13, 3.0e-13)    # H_abs * (1 + p): the robustness filter
ROBUST_TOL = 1.0e-7
PROGNOSTIC = ("H_abs", "S_abs", "m", "thick")
SNOW = ("m_snow", "H_abs_snow", "S_abs_snow", "thick_snow")
VARIANTS = ("plain", "sites", "bgc")


def config(z=None):
    z = golden(WAVE) if z is None else z
    return tcs.testcase4(1, nlayer=int(z["nlayer"]), n_top=int(z["n_top"]), n_bottom=int(z["n_bottom"]))[0]


def late_reader_terms(st):
    """bool[4, ncol]: the four terms of the late-reader condition, in the order of TERMS, on a state as get_state returns it"""
    return np.stack([st.arr("psi_s")[0] < PSI_S_TOP_MIN, st.sc("T_top") >= st.sc("T_freeze"), st.sc("melt_thick_snow") > 0.0,
                     st.sc("melt_thick") > 1.0e-12])


def melt_out(st):
    return st.sc("melt_out1") + st.sc("melt_out2")


def load_wave(which="spread"):
    """(cfg, State, clock, dT2m, precip_scale, onset step of each column counted from the clock)"""
    z = golden(WAVES[which])
    st = State(np.ascontiguousarray(z["lay"]), np.ascontiguousarray(z["scal"]), np.ascontiguousarray(z["n_active"]))
    if which.endswith("_bare"):
        for n in SNOW:
            st.sc(n)[:] = 0.0
    clock = dict(time=float(z["time"]), step=int(z["step"]), n_time_out=int(z["n_time_out"]),
                 time_counter=int(z["time_counter"]), n_outputs=int(z["n_outputs"]))
    return config(z), st, clock, np.ascontiguousarray(z["dT2m"]), np.ascontiguousarray(z["precip_scale"]), z["onset"].copy()


def columns(st, idx):
    return State(np.ascontiguousarray(st.lay[:, :, idx]), np.ascontiguousarray(st.scal[:, idx]), np.ascontiguousarray(st.n_active[idx]))


def variant_config(cfg0, variant):
    cfg = type(cfg0).from_buffer_copy(cfg0)
    if variant == "bgc":
        cfg.bgc_flag = 2
    return cfg


def prepare(solver, cfg, st, clock, dT2m, precip_scale, variant="plain"):
    """same inputs for the HIP solver and the oracle (as stop_seeds.prepare, with the wave's own perturbations)"""
    ncol = st.ncol
    solver.set_forcing(*sheba_forcing(), dT2m, precip_scale)
    if variant == "sites":
        solver.set_ocean(np.zeros(ncol), np.full(ncol, cfg.S_bu_bottom))
    if variant == "bgc":
        solver.set_tracers(np.array([385.0]), None)
    solver.set_state(st)
    if variant == "bgc":
        solver.set_tracer_state(385.0 * st.arr("m")[None, :, :] * np.linspace(0.2, 1.0, cfg.nlayer)[None, :, None])
    solver.set_clock(**clock)
    solver.set_output_window(0, ncol)


def oracle_trajectory(cfg0, st, clock, dT2m, precip_scale, nsteps=NSTEPS, variant="plain", threads=1, want_output=False):
    """the oracle's state after each of nsteps single steps (a list of nsteps States), its status, and -- on request -- the output
    snapshot of the run (None when no output point fell into it)"""
    import samsim_amd
    from tests.oracle_lib import oracle_solver
    cfg = variant_config(cfg0, variant)
    o = oracle_solver(cfg, st.ncol)
    o.set_threads(threads)
    prepare(o, cfg, st, clock, dT2m, precip_scale, variant)
    traj = []
    for _ in range(nsteps):
        o.step(1)
        traj.append(o.get_state())
    status = o.get_status()[0]
    out = None
    if want_output:
        try:
            out = o.get_output()
        except samsim_amd.SamsimError:
            out = None
    o.close()
    return (traj, status, out) if want_output else (traj, status)


def onsets(st0, traj):
    """(onset[ncol], leaders[4, ncol], grew[ncol]): the first step i >= 2 (1-based) after which the late-reader condition holds and
    before which it did not (the states after steps i-1 and i: what a snapshot's own diagnostics say is not used), 0 where there is
    none; the terms that hold after that step; whether melt_out1 + melt_out2 grew in that very step"""
    ncol = st0.ncol
    onset, leaders, grew = np.zeros(ncol, dtype=np.int64), np.zeros((4, ncol), dtype=bool), np.zeros(ncol, dtype=bool)
    done = np.zeros(ncol, dtype=bool)
    for i in range(2, len(traj) + 1):
        t = late_reader_terms(traj[i - 1])
        new = t.any(0) & ~late_reader_terms(traj[i - 2]).any(0) & ~done
        onset[new], leaders[:, new], grew[new] = i, t[:, new], (melt_out(traj[i - 1]) > melt_out(traj[i - 2]))[new]
        done |= new
    return onset, leaders, grew


def scaled(st, p):
    s = st.copy()
    s.arr("H_abs")[:] *= (1.0 + p)
    return s


def within(a, b, c, tol=ROBUST_TOL):
    """column c of state a against state b in the measure of helpers.assert_state_close"""
    try:
        assert_state_close(columns(a, [c]), columns(b, [c]), tol)
    except AssertionError:
        return False
    return True


def robust(cfg, st, clock, dT2m, precip_scale, base_traj, threads=1):
    """bool[ncol]: under H_abs * (1 + p), p of PERTURBATIONS, the column has the same on/off pattern of the late-reader condition in
    every step as the unscaled run and ends within ROBUST_TOL of it"""
    ok = np.ones(st.ncol, dtype=bool)
    pattern = np.stack([late_reader_terms(s).any(0) for s in base_traj])
    for p in PERTURBATIONS:
        traj, status = oracle_trajectory(cfg, scaled(st, p), clock, dT2m, precip_scale, len(base_traj), threads=threads)
        ok &= (np.stack([late_reader_terms(s).any(0) for s in traj]) == pattern).all(0) & (status == 0)
        for c in np.nonzero(ok)[0]:
            ok[c] = within(traj[-1], base_traj[-1], c)
    return ok


# ------------------------------------------------------------------ crafted leaders and their twins
WINTER = "sheba_ensemble_80_day300.npz"     # 0.15-0.28 m of snow at -14 C, surface at -12 C: no reader for weeks
COLUMNS = (0, 63, 69)                       # lane 0, lane 63, and a column of the partial block (stop_seeds.COLUMNS)
LATENT_HEAT = 333500.0


@dataclass(frozen=True)
class Seed:
    terms: tuple                # the terms of the late-reader condition that hold in the leaders' onset step, and no others
    base: Callable              # () -> (cfg, State of NCOL columns, clock, dT2m, precip_scale): the wave before the mutations
    roles: dict                 # column -> ("leader" | "twin", mutation(st, c, cfg))
    what: str
    quiet_mates: bool = True    # no reader fires in the other 67 columns


def winter_wave():
    """members 0..69 of the winter stage under its own clock and their own perturbations; the three seeded columns hold member 0"""
    z = golden(WINTER)
    idx = np.arange(NCOL)
    idx[list(COLUMNS)] = 0
    st = State(np.ascontiguousarray(z["lay"][:, :, idx]), np.ascontiguousarray(z["scal"][:, idx]), np.ascontiguousarray(z["n_active"][idx]))
    clock = dict(time=float(z["time"]), step=int(z["step"]), n_time_out=int(z["n_time_out"]),
                 time_counter=int(z["time_counter"]), n_outputs=int(z["n_outputs"]))
    return config(z), st, clock, np.ascontiguousarray(z["dT2m"][idx]), np.ascontiguousarray(z["precip_scale"][idx])


def warm_top(h1):
    """Layer 1 at the specific enthalpy h1 [J/kg], a little on the solid side of psi_s(1) = 0.4, between layers 2..4 close to melting
    (-15 kJ/kg) and a snow cover at -0.1 C (H_abs_snow / m_snow = -333.7 kJ/kg: dry).  The surface stays at -12 C under the winter
    forcing, so T_top < T_freeze, the snow releases nothing, and the heat layer 2 conducts upwards takes psi_s(1) through 0.4 a few
    steps later (h1 = -134.5 kJ/kg: step 4; -134.8 kJ/kg: step 12; -135.0 kJ/kg: step 18, too late; -140 kJ/kg: psi_s(1) = 0.414 after 24 steps, the twin).
    func_freeboard then reads the rows; the melt water sub_melt_thick finds is taken up by the snow (sub_melt_snow), so melt_thick
    stays 0 and flush3 does not run: psi_s(1) < 0.4 alone"""
    def f(st, c, cfg):
        assert int(st.n_active[c]) >= 4
        m = st.arr("m")
        st.arr("H_abs")[0, c] = h1 * m[0, c]
        for k in (1, 2, 3):
            st.arr("H_abs")[k, c] = -1.5e4 * m[k, c]
        st.sc("H_abs_snow")[c] = -(LATENT_HEAT + 200.0) * st.sc("m_snow")[c]
    return f


def melt_wave():
    return load_wave("melt")[:5]


def no_snow(st, c, cfg):
    """the column's 0.04 mm of snow taken away: thick_snow = 0 skips the sweep's snow terms, T_top >= T_freeze alone stores the rows in
    the onset step, and on bare ice sub_melt_thick finds melt water at once (1e-9 m, above flush3's 1e-12), so flush3 reads them"""
    for n in SNOW:
        st.sc(n)[c] = 0.0


def winter_snow(st, c, cfg):
    """the other side: 0.2 m of snow at -14 C (the cover of the winter stage's first member) keeps the surface below T_freeze"""
    st.sc("m_snow")[c], st.sc("H_abs_snow")[c], st.sc("S_abs_snow")[c], st.sc("thick_snow")[c] = 70.957, -2.5718e7, 0.0, 0.2150


SEEDS = {
    # the kernel's T_top term deciding ahead of flush3; its wave-mates are the melt wave's own columns, which have their onset too
    "T_top_bare": Seed(("T_top", "melt_thick"), melt_wave, {0: ("leader", no_snow), 63: ("twin", winter_snow), 69: ("leader", no_snow)},
                       "bare ice whose surface reaches T_freeze: melt water in the onset step", quiet_mates=False),
    "psi_s_top": Seed(("psi_s_top",), winter_wave, {0: ("leader", warm_top(-1.345e5)), 63: ("twin", warm_top(-1.40e5)),
                                                  69: ("leader", warm_top(-1.348e5))},
                      "top-layer enthalpy raised so that psi_s(1) crosses 0.4 under a cold surface"),
}

# the term that leads alone on the natural trajectories, and why it has no crafted column
NATURAL_LEADER = {
    "T_top":
        "leads alone in all 70 columns of the `spread` wave (a surface that reaches T_freeze(S_bu(1)) under 5-9 mm of snow, around thick_min: "
        "func_freeboard runs, nothing melts yet); their twins are in the same wave, the columns whose surface is still below it in the "
        "same step.  No crafted column beside the winter wave-mates: layer 1 is on its liquidus, T(1) = T_freeze(S_br) <= "
        "T_freeze(S_bu(1)) wherever phi(1) > 0, and under the winter forcing (T2m = -11 C) the surface is the coldest point of the "
        "column, so T_top >= T_freeze(S_bu(1)) needs phi(1) -> 0 and psi_s(1) < 0.4 holds first; only warmer air takes the surface "
        "there, and under the clock of the waves the winter columns all have their onset within 24 steps themselves.",
}

# terms of the condition for which the oracle shows that no finite state makes them hold alone in an onset step
NO_LEADER = {
    "melt_thick_snow":
        "never alone: mo_grotz.f90:670 adds melt_thick_snow to melt_thick in the same step, so melt_thick_snow > 1e-12 makes the fourth "
        "term true as well; alone it holds only for 0 < melt_thick_snow <= 1e-12 m.  Nor does it lead under a cold surface: snow_thermo "
        "releases melt water once the liquid mass fraction of the snow exceeds 0.057 (1 - psi_s_snow) / psi_s_snow + 0.017 (0.12 for "
        "the winter cover), and a cover at 0 C under a surface with T_top < T_freeze <= 0 C over ice at or below 0 C loses heat at "
        "both faces.  Tried on the winter column: H_abs_snow = -latent_heat * m_snow * f, f = 1.2 .. 0.99 -- T_top rises from -12.3 C "
        "to -5.3 C, no melt water within 24 steps; with f < 0.88 the first snow_block of step 1 (the full first sweep after "
        "set_state, not the deciding sweep) releases it.  In the wave the term appears with T_top, never before it.",
    "melt_thick":
        "never alone: sub_melt_thick runs only under psi_s(1) < psi_s_top_min or T_top >= T_freeze (mo_grotz.f90:637) and melt_thick is "
        "otherwise the sum 0 + melt_thick_snow, so the term needs the first, the second or the third one in the same step.",
}


def build_seed_wave(seed, mutated=True):
    """(cfg, State, clock, dT2m, precip_scale, {column: role}) of a seed's wave; mutated=False: the wave before the mutations"""
    cfg, st, clock, dT2m, precip_scale = seed.base()
    if mutated:
        for c, (_, mutate) in seed.roles.items():
            mutate(st, c, cfg)
    return cfg, st, clock, dT2m, precip_scale, {c: role for c, (role, _) in seed.roles.items()}
