"""The wave-level votes of the fused up sweep (tests/wave_votes.py) held against the CPU oracle, on the CPU.

The oracle runs every committed SHEBA stage ensemble (sheba_ensemble_80*.npz) and the melt-season checkpoint tc4_melt_state.npz for
200 steps; after every step the first sweep of the next step is restated in numpy from the state the oracle returns, and
  * no row the division-free bound calls "below" holds a lane whose Rayleigh number exceeds ray_crit (nor any single lane);
  * no layer the shortcut calls "above" has S_br_clamped(H/c_l, S_bu) <= S_bu.
The decided shares are printed per fixture (a record, not a threshold).  The bound is also held against 10**6 random operand sets
whose exact quotient lies within 1 +- 2**-18 of ray_crit, and the liquidus cubics against the two facts the shortcut rests on."""
import functools
import glob
import os

import numpy as np
import pytest

from samsim_amd import testcases as tcs
from samsim_amd.capi import State
from tests import wave_votes as wv
from tests.helpers import GOLDEN, golden, load_checkpoint, sheba_forcing
from tests.oracle_lib import oracle_solver

NSTEPS = 200
NTHREADS = min(16, len(os.sched_getaffinity(0)))
FIXTURES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "sheba_ensemble_80*.npz"))) + ["tc4_melt_state.npz"]
EPS = 2.0 ** -52


def setup(name):
    """(cfg, State, clock, dT2m, precip_scale)"""
    if name.startswith("sheba_ensemble"):
        z = golden(name)
        cfg, _ = tcs.testcase4(1, nlayer=int(z["nlayer"]), n_top=int(z["n_top"]), n_bottom=int(z["n_bottom"]))
        st = State(np.ascontiguousarray(z["lay"][:4]), np.ascontiguousarray(z["scal"]), np.ascontiguousarray(z["n_active"]))
        clock = dict(time=float(z["time"]), step=int(z["step"]), n_time_out=int(z["n_time_out"]),
                     time_counter=int(z["time_counter"]), n_outputs=int(z["n_outputs"]))
        return cfg, st, clock, np.ascontiguousarray(z["dT2m"]), np.ascontiguousarray(z["precip_scale"])
    st, clock = load_checkpoint(name)
    cfg, _ = tcs.testcase4(1, nlayer=st.nlayer)
    return cfg, st, clock, None, None


@functools.lru_cache(maxsize=None)
def tally(name):
    """the oracle's 200 steps, restated after each: counts of rows and lanes, and the violations"""
    cfg, st, clock, dT2m, precip_scale = setup(name)
    assert cfg.harmonic_flag == 2 and cfg.salt_flag == 1
    o = oracle_solver(cfg, st.ncol)
    o.set_threads(NTHREADS)
    o.set_forcing(*sheba_forcing(), dT2m, precip_scale)
    o.set_state(st)
    o.set_clock(**clock)
    o.set_output_window(0, 0)
    t = dict(rows=0, rows_bound=0, rows_with_a_lane_above=0, rows_bad=0, lanes=0, lanes_below=0, lanes_bad=0, lanes_near=0,
             layers=0, layers_short=0, layer_rows=0, layer_rows_short=0, layers_bad=0)
    for _ in range(NSTEPS):
        o.step(1)
        f = wv.first_sweep(o.get_state())
        up = f["inner"].copy()
        up[0] = False                                       # the up sweep runs layers N_active .. 2; layer 1 always stores its row
        below = wv.bound_below(f["d_S_br"], f["height"], f["h_sum"], f["h_den"], f["minp"])
        above = f["ray"] > wv.RAY_CRIT
        decided, has = wv.rows(below, up)
        row_above = wv.row_any(above & up)
        t["rows"] += int(has.sum()); t["rows_bound"] += int(decided.sum()); t["rows_with_a_lane_above"] += int(row_above.sum())
        t["rows_bad"] += int((decided & row_above).sum())
        t["lanes"] += int(up.sum()); t["lanes_below"] += int((below & up).sum()); t["lanes_bad"] += int((below & above & up).sum())
        t["lanes_near"] += int((up & (np.abs(f["ray"] / wv.RAY_CRIT - 1.0) < 0.01)).sum())
        lay = f["active"].copy()
        lay[0] = False
        short = wv.shortcut_lane(f["Tl"], f["S_bu"])
        really = np.maximum(wv.S_br_poly(f["Tl"]), f["S_bu"]) > f["S_bu"]
        srow, shas = wv.rows(short, lay)
        t["layers"] += int(lay.sum()); t["layers_short"] += int((short & lay).sum()); t["layers_bad"] += int((short & ~really & lay).sum())
        t["layer_rows"] += int(shas.sum()); t["layer_rows_short"] += int(srow.sum())
    status = o.get_status()[0]
    o.close()
    t["stopped"] = int((status != 0).sum())
    return t


@pytest.mark.parametrize("name", FIXTURES)
def test_the_votes_agree_with_the_numbers(name, capsys):
    t = tally(name)
    with capsys.disabled():
        print("\n%s: rows %d, decided by the bound %.1f %%, with a lane above ray_crit %.1f %%; lanes within 1 %% of ray_crit %.2f %%; "
              "getT rows %d, decided by the shortcut %.1f %% (lanes %.1f %%); stopped columns %d"
              % (name, t["rows"], 100.0 * t["rows_bound"] / max(t["rows"], 1), 100.0 * t["rows_with_a_lane_above"] / max(t["rows"], 1),
                 100.0 * t["lanes_near"] / max(t["lanes"], 1), t["layer_rows"], 100.0 * t["layer_rows_short"] / max(t["layer_rows"], 1),
                 100.0 * t["layers_short"] / max(t["layers"], 1), t["stopped"]))
    if name == "sheba_ensemble_80.npz":      # the headline ensemble holds rows on both sides (day 25 is open water: no row at all)
        assert 0 < t["rows_bound"] < t["rows"] and t["rows_with_a_lane_above"] > 0 and 0 < t["layer_rows_short"] < t["layer_rows"]
    assert t["rows_bad"] == 0, "a row the bound calls below holds a lane above ray_crit"
    assert t["lanes_bad"] == 0, "a lane the bound calls below is above ray_crit"
    assert t["layers_bad"] == 0, "a layer the shortcut calls above is pure brine"


def test_the_bound_on_random_operands_at_the_threshold():
    """operand sets whose exact quotient c * d * height * h_sum / h_den is ray_crit * (1 + delta), delta uniform in +- 2**-18: a lane
    the bound calls below stays below ray_crit with eight ulp to spare (the device's quotient is within two ulp of the division,
    samsim_div.h), and the bound decides every lane more than 2**-19 below the threshold"""
    rng = np.random.default_rng(13)
    n = 10 ** 6
    d = rng.uniform(0.5, 150.0, n)                   # S_br - S_br_bot, g/kg
    height = rng.uniform(0.01, 3.0, n)               # m
    h_sum = height + rng.uniform(0.001, 0.05, n)
    delta = rng.uniform(-1.0, 1.0, n) * 2.0 ** -18
    h_den = (wv.C_RAY * d * height * h_sum) / (wv.RAY_CRIT * (1.0 + delta))
    minp = np.full(n, 1.0e-10)
    ray = wv.ray_of(d, height, h_sum, h_den, minp)
    below = wv.bound_below(d, height, h_sum, h_den, minp)
    assert 0.2 < below.mean() < 0.5, below.mean()    # (the margin is a quarter of the interval's half width)
    assert (ray[below] * (1.0 + 8.0 * EPS) < wv.RAY_CRIT).all()
    assert below[delta < -2.0 ** -19].all()
    assert not below[delta > 0.0].any()
    # without the margin the compare sits on the threshold itself, where a rounding decides
    loose = wv.bound_below(d, height, h_sum, h_den, minp, margin=0.0)
    assert loose[delta < -2.0 ** -40].all()
    # a NaN operand is never below; a column whose smallest permeability is under 1e-14 always is (hp = 0)
    nan = np.full(4, np.nan)
    one = np.ones(4)
    assert not wv.bound_below(nan, one, one, one, one).any() and not wv.bound_below(one, one, one, nan, one).any()
    assert wv.bound_below(one * 1e6, one, one, one * 1e-30, one * 1e-15).all()
    assert (wv.ray_of(one * 1e6, one, one, one * 1e-30, one * 1e-15) == 0.0).all()


@pytest.mark.parametrize("salt", [1, 2])
def test_the_liquidus_falls_and_is_above_40_at_minus_3(salt):
    c2, c3, c4 = wv.SALTS[salt]
    assert (2.0 * c3) ** 2 < 4.0 * (3.0 * c4) * c2            # the derivative c2 + 2 c3 T + 3 c4 T**2 has no real root
    assert c2 < 0.0                                            # ... and is negative at 0: negative everywhere
    assert wv.S_br_poly(wv.T_SHORT, salt) > wv.S_SHORT + 9.0
    T = -np.geomspace(3.0, 1.0e6, 200001)
    S = wv.S_br_poly(T, salt)
    assert (np.diff(S) > 0.0).all() and S[0] > wv.S_SHORT + 9.0   # computed values: rising as T falls
    assert wv.S_br_poly(-np.inf, salt) == np.inf and not wv.shortcut_lane(np.nan, 1.0) and not wv.shortcut_lane(-5.0, np.nan)
