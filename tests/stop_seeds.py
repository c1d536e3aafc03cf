"""STOP seeds: committed fixture states with one deterministically corrupted column, each aimed at one STOPC site of the step kernel.

A physics failure never aborts the process: the column records the reference's `STOP n` with the step and the layer of the
failure (include/samsim.h, samsim_get_status) and freezes.  Those three integers are the library's only error channel, so every
STOPC site of samsim_amd/csrc gets either a seed here -- a fixture, a configuration and a mutation of ONE column that brings the
CPU oracle to that site within 64 steps -- or a line in SITES saying what was tried and why a finite state does not get there.

Rules of a mutation: finite values only; only H_abs, S_abs, m, thick of ACTIVE layers and the snow scalars (m_snow, H_abs_snow,
S_abs_snow, thick_snow); n_active is never touched.  tests/test_stop_seeds_host.py checks these rules and that the oracle really
stops with the aimed-at code; tests/test_gpu_stop_codes.py runs the seeds with `gpu=True` on the device.

A seed is kept away from the GPU (`gpu=False`) when its outcome is decided by round-off (the two paths sum in different orders)
or when its trajectory passes close to states on which the reference's own Newton loops do not terminate.
"""
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np

from samsim_amd import testcases as tcs
from samsim_amd.capi import State
from tests.helpers import golden, load_checkpoint, sheba_forcing

NCOL = 70           # one full 64-column block and a partial block of 6
COLUMNS = (0, 63, 69)   # lane 0, lane 63, and a column of the partial block
MAX_STEPS = 64
PROGNOSTIC = ("H_abs", "S_abs", "m", "thick")
SNOW = ("m_snow", "H_abs_snow", "S_abs_snow", "thick_snow")

WINTER, MELT, PLATE, GROWTH = "tc4_spunup_state.npz", "tc4_melt_state.npz", "tc1_spunup_state.npz", "growth_wave_12.npz"
GROWTH_COLUMN = 8   # N_active 7 of Nlayer 12


# ------------------------------------------------------------------ configurations
def _tc4():
    return tcs.testcase4(1)[0]


def _tc4_harmonic1():
    c = _tc4()
    c.harmonic_flag = 1     # not the flag set the fixed-flag kernels are built for: the run-time-flag kernel
    return c


def _tc4_flush6():
    c = _tc4()
    c.flush_flag = 6
    return c


def _tc1():
    return tcs.testcase1(1)[0]


def _tc4_nlayer12():
    z = golden(GROWTH)
    return tcs.testcase4(1, nlayer=int(z["nlayer"]), n_top=int(z["n_top"]), n_bottom=int(z["n_bottom"]))[0]


CONFIGS = {"tc4": _tc4, "tc4_harmonic1": _tc4_harmonic1, "tc4_flush6": _tc4_flush6, "tc1": _tc1, "tc4_nlayer12": _tc4_nlayer12}

# instantiations of the step kernel a seed is run under: the configuration's own, per-column ocean (zero offsets: the same
# physics), one passive tracer, and the run-time-flag kernel
VARIANTS = ("plain", "sites", "bgc", "generic")


def fixture(name):
    """(one-column State, clock) of a committed fixture"""
    if name == GROWTH:
        z = golden(name)
        i = GROWTH_COLUMN
        st = State(np.ascontiguousarray(z["lay"][:, :, i:i + 1]), np.ascontiguousarray(z["scal"][:, i:i + 1]),
                   np.ascontiguousarray(z["n_active"][i:i + 1]))
        c = golden("sheba_ensemble_80_day75.npz")
        clock = dict(time=float(c["time"]), step=int(c["step"]), n_time_out=int(c["n_time_out"]),
                     time_counter=int(c["time_counter"]), n_outputs=int(c["n_outputs"]))
        return st, clock
    return load_checkpoint(name)


# ------------------------------------------------------------------ mutations (st: State of the ensemble, c: the column)
def _lay(st, name, k, c):
    """layer k (1-based) of column c"""
    assert 1 <= k <= int(st.n_active[c]), "a mutation never touches an inactive layer"
    return st.arr(name), k - 1, c


def set_layer(name, k, value):
    def f(st, c, cfg):
        a, i, j = _lay(st, name, k, c)
        a[i, j] = value
    return f


def set_snow(**values):
    def f(st, c, cfg):
        for n, v in values.items():
            assert n in SNOW
            st.sc(n)[c] = v(st, c, cfg) if callable(v) else v
    return f


def chain(*fs):
    def f(st, c, cfg):
        for g in fs:
            g(st, c, cfg)
    return f


def scale_layer(k, factor, names=("m", "H_abs", "S_abs")):
    """layer k times `factor` in the named arrays (all three extensive ones: H and S_bu keep their values)"""
    def f(st, c, cfg):
        for n in names:
            a, i, j = _lay(st, n, k, c)
            a[i, j] *= factor(st, c, cfg) if callable(factor) else factor
    return f


def thin_snow(h_abs_snow=None, h_factor=None, dense=False):
    """a snow cover of half thick_min (the thin-snow coupling of mo_snow.f90:61-104 runs in every step), its enthalpy set or scaled"""
    def f(st, c, cfg):
        st.sc("thick_snow")[c] = cfg.thick_min / 2.0
        if dense:
            st.sc("m_snow")[c] = 330.0 * cfg.thick_min / 2.0
        if h_abs_snow is not None:
            st.sc("H_abs_snow")[c] = h_abs_snow
        if h_factor is not None:
            st.sc("H_abs_snow")[c] *= h_factor
    return f


def light_top_layer_under_heavy_thin_snow(st, c, cfg):
    """layer 1 scaled to 0.3 kg/m2 (H and S_bu unchanged) under 0.9 thick_min of snow five times as heavy: each exchange of the
    thin-snow coupling moves sg*c_s*m_snow of enthalpy, which changes T(1) by m_snow/m(1) = 5 times what it changes T_snow by, so the
    temperature difference grows by (1 - (1+5)/2) = -2 per iteration instead of shrinking: 201 iterations, STOP 16"""
    f = 0.3 / st.arr("m")[0, c]
    for n in ("m", "H_abs", "S_abs"):
        st.arr(n)[0, c] *= f
    th = 0.9 * cfg.thick_min
    st.sc("thick_snow")[c] = th
    st.sc("m_snow")[c] = 330.0 * th
    st.sc("H_abs_snow")[c] = -333500.0 * 330.0 * th * 1.1


def thin_top_fat_third_layer(st, c, cfg):
    """7889.  thick(1) = 0.4 thick_0 (below the 0.5 thick_0 that calls top_melt) and thick(3) = 1.6 thick_0, m, H_abs and S_abs of both
    scaled with them (densities, H and S_bu unchanged).  top_melt merges layer 2 into layer 1, shifts the rest up by one and drops
    the last active layer; the thicknesses then sum to (N_active + 0.4 + 0.6) thick_0 = (N_active' + 2.0) thick_0 >= (N_active' +
    0.501) thick_0 with N_active' = N_active - 1 < Nlayer.

    Why every layer index of layer_dynamics (samsim_regrid.h) stays within 1..Nlayer for this input: no index there is computed from
    a thickness.  layer_dynamics reads phi at N_active, max(N_active-1, 1), Nlayer-1, Nlayer and thick at N_top+1 and 1; top_melt
    (N_active = 68 > N_top = 5, thick(N_top+1)/thick_0 < 1.00001, N_active < Nlayer = 90) reads and writes layers 1, 2, then k and
    k+1 for k = 2..N_top-1 and for k = N_top..N_active-1 (k+1 <= N_active <= Nlayer), zeroes layer N_active, and sums thick over
    1..Nlayer.  The perturbed thicknesses enter as divisors (rho = m/thick, both finite and positive) and as terms of that sum, and in
    the branch conditions `thick(1) < 0.5 thick_0` and `thick(N_top+1)/thick_0 < 1.00001`, which select among loops whose bounds are
    N_top, N_middle, N_active and Nlayer.  The first sweep finds the column off the grid rule after samsim_set_state (COLF_REGULAR is
    checked against the array there) and the wave takes the sweeps that load thick per layer."""
    f = 0.4 * cfg.thick_0 / st.arr("thick")[0, c]
    for n in PROGNOSTIC:
        st.arr(n)[0, c] *= f
        st.arr(n)[2, c] *= 1.6


def negate_top_layer(st, c, cfg):
    """m(1), H_abs(1), S_abs(1) negated: H and S_bu keep their values, so getT returns the same phi > 0, and psi_s(1) = m phi / rho_s /
    thick < 0.  S_abs(1) is 0 in the melt state (-0.0 < 0 is false), so gravity drainage's MINVAL(S_abs) does not fire: the column
    reaches the health check at the end of the step"""
    for n in ("m", "H_abs", "S_abs"):
        st.arr(n)[0, c] *= -1.0


# ------------------------------------------------------------------ the seeds
@dataclass(frozen=True)
class Seed:
    name: str
    site: str                   # the STOPC site (SITES) the oracle's route corresponds to
    code: int
    fixture: str
    config: str
    mutate: Callable
    gpu: bool = True
    min_step: int = 1           # the stop must come this many steps after set_state or later (late seeds: inside the fused sweeps)
    layer: Optional[int] = None  # the layer the contract of include/samsim.h defines, where it does not depend on dynamics
    variants: tuple = ("plain",)
    why_cpu_only: str = ""


SEEDS = [
    # --- 99 in the first sweep after set_state (full first sweep, samsim_sweeps_unfused.h)
    Seed("first_sweep_99_winter", "unfused:first_sweep", 99, WINTER, "tc4", set_layer("H_abs", 40, -1.0e15), layer=40),
    Seed("first_sweep_99_plate", "unfused:first_sweep", 99, PLATE, "tc1", set_layer("H_abs", 40, -1.0e15), layer=40),
    Seed("first_sweep_99_two_layers", "unfused:first_sweep", 99, WINTER, "tc4",
         chain(set_layer("H_abs", 3, -1.0e15), set_layer("H_abs", 40, -1.0e15)), layer=40),   # double fault: the sweep meets 40 first
    Seed("first_sweep_99_short_column", "unfused:first_sweep", 99, GROWTH, "tc4_nlayer12", set_layer("H_abs", 2, -1.0e15), layer=2),
    # --- 99 of the snow: snow_thermo's own getT (salty snow, so that getT iterates at all), and the thin-snow coupling
    Seed("snow_99", "surface:snow_getT", 99, WINTER, "tc4",
         set_snow(S_abs_snow=lambda st, c, cfg: 5.0 * st.sc("m_snow")[c], H_abs_snow=-1.0e15), layer=0),
    Seed("coupling_99", "surface:coupling", 99, WINTER, "tc4", thin_snow(h_abs_snow=-1.0e9), layer=1),
    Seed("coupling_16", "surface:coupling", 16, MELT, "tc4", light_top_layer_under_heavy_thin_snow, layer=1),
    # --- 99 many steps after set_state: the cold wave of an absurdly cold thin snow cover travels down, inside the fused sweeps
    Seed("late_99_cold_snow_x40", "fused:up_sweep_rc", 99, MELT, "tc4", thin_snow(h_factor=40.0), min_step=10,
         variants=VARIANTS),
    Seed("late_99_dense_cold_snow", "fused:up_sweep_rc", 99, MELT, "tc4", thin_snow(h_abs_snow=-1.0e9, dense=True), min_step=10),
    # --- 431.  The balance of sub_heat_fluxes is violated only through round-off: an enthalpy so large that one ulp of it is far above
    # the 1e-5 W * dt of the test.  The reference compares two column sums that are both quantised to that ulp and agree in
    # roughly every second step -- on the issue's own H_abs_snow = -1e15 the oracle stops in step 1, 3 or 5 or runs on to a 99
    # depending on the column's forcing perturbation -- while the kernel's sum of per-layer differences keeps the rounding error of the
    # update itself (uniform in +-ulp/2: below 1e-4 J with probability 3e-3 at ulp = 0.06 J).  The GPU seeds are the magnitudes at which
    # the oracle stops in step 1 in all three columns and under every variant, found by scanning on the CPU; their neighbours in
    # the scan (4.75e14; 2.5e14 .. 6e14) behave the same.  The issue's literal values stay as CPU seeds of column 0.
    Seed("energy_431_snow_melt", "fused:up_sweep_431", 431, MELT, "tc4", set_snow(H_abs_snow=-4.5e14), layer=0, variants=VARIANTS),
    Seed("energy_431_top_plate", "fused:up_sweep_431", 431, PLATE, "tc1", set_layer("H_abs", 1, 4.0e14), layer=0),
    # double fault: on the winter state the same snow also cools layer 1 so far within the step that the second getT sweep fails
    # (with the oracle's 431 made non-fatal: 431, then 99 of layer 1, both in step 1, in all three columns); the reference evaluates
    # the heat fluxes (431, mo_grotz.f90:584) before that sweep (:598)
    Seed("energy_431_then_99_same_step", "fused:up_sweep_431", 431, WINTER, "tc4", set_snow(H_abs_snow=-4.25e15), layer=0),
    Seed("energy_431_snow_1e15", "fused:up_sweep_431", 431, MELT, "tc4", set_snow(H_abs_snow=-1.0e15), gpu=False, layer=0,
         why_cpu_only="round-off decides the step: the oracle stops column 0 in step 1, column 69 in step 3, and column 63 never (99 in step 6)"),
    Seed("energy_431_top_1e12", "fused:up_sweep_431", 431, PLATE, "tc1", set_layer("H_abs", 1, 1.0e12), gpu=False, layer=0,
         why_cpu_only="ulp(1e12) = 1.2e-4 J against a bound of 1e-5 J (dt = 1 s): a step passes the test with probability ~0.1 in either "
                      "summation order, so the two may stop one step apart"),
    Seed("late_431_round_off", "fused:up_sweep_431", 431, WINTER, "tc4", set_layer("H_abs", 40, 1.0e11), gpu=False, min_step=10, layer=0,
         why_cpu_only="|H_abs| = 1e11 puts one ulp of the column sum at 1.5e-5 J: whether |balance|/dt passes 1e-5 W in a given step is "
                      "decided by the order of summation (the reference: two sums of Nlayer terms; the kernel: one sum of per-layer "
                      "differences), so the two legitimately stop in different steps"),
    # --- 1337 after gravity drainage (MINVAL(S_abs) < 0): the melt state does not expel brine, so nothing heals the negative salt
    Seed("drain_1337_top", "unfused:drain_1337", 1337, MELT, "tc4", set_layer("S_abs", 1, -1.0), layer=0),
    Seed("drain_1337_layer4", "unfused:drain_1337", 1337, MELT, "tc4", set_layer("S_abs", 4, -5.0e3), layer=0, variants=VARIANTS),
    # --- 1337 of the health check at the end of the step (MINVAL(psi_s) < 0)
    Seed("health_1337", "kernels:health_1337", 1337, MELT, "tc4", negate_top_layer, layer=0),
    # --- 7889: the grid after top_melt is thicker than its layer count allows
    Seed("regrid_7889", "regrid:7889", 7889, PLATE, "tc1", thin_top_fat_third_layer, layer=0),
]
BY_NAME = {s.name: s for s in SEEDS}
GPU_SEEDS = [s for s in SEEDS if s.gpu]

# ------------------------------------------------------------------ the site table: every STOPC of samsim_amd/csrc
# (file, code as written, what the site is, seeds or the reason there is none).  tests/test_stop_seeds_host.py holds this
# table against the source: a STOPC added or removed there fails until the table follows.
SITES = [
    ("samsim_surface.h", "rc", "thin-snow coupling: 99 of either getT, 16 of the exchange loop", ["coupling_99", "coupling_16"]),
    ("samsim_surface.h", "99", "snow_thermo's getT of the snow", ["snow_99"]),
    ("samsim_surface.h", "345", "snow_thermo: psi_s_snow + psi_l_snow != 1 after the cover was shrunk to its water equivalent",
     "unreachable from a finite state: the branch sets thick_snow = m_snow*(phi/rho_s + (1-phi)/rho_l) and forms psi_s_snow + psi_l_snow "
     "= m_snow*(phi/rho_s + (1-phi)/rho_l)/thick_snow from the same numbers, which is 1 to a few ulp whatever m_snow, phi are (the branch "
     "is entered with m_snow*(..) > thick_snow > 0, so the new thickness is positive).  Tried: m_snow x3, x30 with thick_snow /3, /30 on "
     "both SHEBA states, H_abs_snow x30: the branch runs, the sum stays 1 (no stop, or 431 from the heavier cover)."),
    ("samsim_surface.h", "9876", "snow_thermo: psi_g_snow < 0 at its end",
     "unreachable: psi_g_snow = 1 - psi_s_snow - psi_l_snow can be negative by round-off after the branch above, but every path to the "
     "end either takes |psi_g_snow| (melting cover), sets it to 0 (psi_s_snow < 1e-6), needs psi_g_snow > 0 (wet snow), or -- for "
     "psi_g_snow <= 0 -- merges the cover into layer 1 and sets it to 0.  Tried with the denser covers of the line above."),
    ("samsim_sweeps_fused.h", "rc", "prologue_top_layer: getT of layer 1 at the head of a fused step",
     "shares its cause with the up sweep's rc: layer 1's prognostic values change between the up sweep of step n and the prologue of "
     "step n+1 only through snow melt water, flushing and regrids, none of which produced a non-converging getT in the searches "
     "(melt state, layer 1 warmed to H_abs x0.2 / x0.05, with and without snow)"),
    ("samsim_sweeps_fused.h", "rcc", "fused down sweep: the step's first thin-snow coupling (mo_grotz.f90:418-420), written without the macro",
     "not reached late: between the second coupling of step n (up sweep) and the first of step n+1 only snow fall and snow_thermo touch "
     "the snow and layer 1, and a coupling that has just converged leaves T(1) and T_snow within 0.1 K of each other, so the next one "
     "starts at its own fixed point.  A coupling that fails therefore fails in the first step after set_state, which takes the unfused "
     "order (coupling_99, coupling_16); the late seeds with thin snow run this site in every step without a stop"),
    ("samsim_sweeps_fused.h", "21234", "fused down sweep: S_abs(k) < 0 after the drainage loss",
     "not reached: the flux is clamped to psi_l*rho_l*thick = m(1-phi) - V_ex*rho_l and S_br = S_bu/(1-phi), so flux*S_br <= S_abs "
     "after expulsion up to round-off; a clamped flux needs a Rayleigh number of order 1e3 above critical.  Tried: S_abs x3, x10, x30 "
     "in layer 5 and in all layers but the bottom one, with H_abs(5) x1.3, on the three states and with harmonic_flag 1: no stop up to "
     "x10, 99 of the first sweep (or a reference Newton loop that does not end) at x30"),
    ("samsim_sweeps_fused.h", "1337", "fused down sweep: MINVAL(S_abs) < 0 after gravity drainage",
     "no late seed: mass_transfer clamps every transfer to the salt present and the health check clamps S_abs >= 0 at the end of every "
     "step, so a negative S_abs exists only in the first step after set_state, which takes the unfused order (drain_1337_*)"),
    ("samsim_sweeps_fused.h", "rc", "fused up sweep: 99 of the second getT sweep", ["late_99_cold_snow_x40", "late_99_dense_cold_snow"]),
    ("samsim_sweeps_fused.h", "431", "fused up sweep: energy balance of sub_heat_fluxes",
     ["energy_431_snow_melt", "energy_431_top_plate", "energy_431_then_99_same_step", "energy_431_snow_1e15", "energy_431_top_1e12",
      "late_431_round_off"]),
    ("samsim_sweeps_unfused.h", "rc", "full first sweep: 99 of getT",
     ["first_sweep_99_winter", "first_sweep_99_plate", "first_sweep_99_two_layers", "first_sweep_99_short_column"]),
    ("samsim_sweeps_unfused.h", "21234", "unfused drainage: S_abs(k) < 0 after the drainage loss", "as the fused site: not reached"),
    ("samsim_sweeps_unfused.h", "1337", "unfused drainage: MINVAL(S_abs) < 0", ["drain_1337_top", "drain_1337_layer4"]),
    ("samsim_melt.h", "9876", "flush3: |m(1)| < 1e-6 after the flushed melt water left layer 1",
     "not reached: needs m(1) equal to the flushed mass to 1e-6 kg/m2.  Tried on the melt state: layer 1 scaled to 1e-7, 1e-5, 1e-3 "
     "kg/m2, warmed (H_abs x0.2), with and without snow: 16 (coupling), 99 in the bottom layer one step later, or no stop"),
    ("samsim_melt.h", "9876", "flush4 (flush_flag 6): MINVAL(S_abs) < 0",
     "unreachable with gravity drainage on: flush4 clamps S_abs(1) and multiplies the other layers by para_flush_gamma > 0, so it needs "
     "a negative S_abs(k >= 2) on entry, which drainage's own MINVAL(S_abs) test (1337) has caught earlier in the same step and the "
     "health check has clamped in every later one.  Tried: flush_flag 6 on the melt state without snow, layer 1 warmed so that melt "
     "water forms at once: flush4 runs, no stop"),
    ("samsim_regrid.h", "7889", "top_melt: SUM(thick) too large for N_active", ["regrid_7889"]),
    ("samsim_kernels.hip", "1337", "health check at the end of the step: MINVAL(psi_s) < 0", ["health_1337"]),
]
# 431 and 99 in ONE step: found (energy_431_then_99_same_step).  With the oracle's 431 made non-fatal, the winter state with
# H_abs_snow = -4.25e15 reports 431 and then 99 of layer 1 in step 1; the reference order gives 431.


# ------------------------------------------------------------------ building and running an ensemble
def build(seed, col=0, mutated=True, ncol=NCOL, variant="plain"):
    """(cfg, State of ncol replicas with column `col` mutated, clock)"""
    cfg = CONFIGS["tc4_harmonic1" if variant == "generic" else seed.config]()
    if variant == "generic":
        assert seed.config == "tc4"
    if variant == "bgc":
        cfg.bgc_flag = 2
    st1, clock = fixture(seed.fixture)
    st = st1.replicate(ncol)
    if mutated:
        seed.mutate(st, col, cfg)
    return cfg, st, dict(clock)


def prepare(solver, cfg, st, clock, variant="plain"):
    """same inputs for the HIP solver and the oracle: forcing with the project's ensemble perturbation where the configuration reads
    forcing, the variant's extras, state, clock"""
    ncol = st.ncol
    if cfg.atmoflux_flag == 2:
        dT, ps = tcs.ensemble_perturbation(ncol)
        solver.set_forcing(*sheba_forcing(), dT, ps)
    if variant == "sites":
        solver.set_ocean(np.zeros(ncol), np.full(ncol, cfg.S_bu_bottom))
    if variant == "bgc":
        solver.set_tracers(np.array([385.0]), None)
    solver.set_state(st)
    if variant == "bgc":
        solver.set_tracer_state(385.0 * st.arr("m")[None, :, :] * np.linspace(0.2, 1.0, cfg.nlayer)[None, :, None])
    solver.set_clock(**clock)
    solver.set_output_window(0, ncol)


def run_oracle(seed, col=0, mutated=True, variant="plain", nsteps=MAX_STEPS, clock_override=None, ncol=NCOL):
    """the oracle on the seed's ensemble: (solver after nsteps, cfg, initial state, clock)"""
    from tests.oracle_lib import oracle_solver
    cfg, st, clock = build(seed, col, mutated, ncol, variant)
    clock.update(clock_override or {})
    o = oracle_solver(cfg, ncol)
    o.set_threads(1)        # 70 columns x 64 steps: a team of threads costs more than it saves, most of all beside other work
    prepare(o, cfg, st, clock, variant)
    o.step(nsteps)
    return o, cfg, st, clock
