"""TEST INFRASTRUCTURE: ten-step windows tiled end to end across the events that amplify round-off.

The freeze-up of the ocean grid (first snow growing through thick_min), the SHEBA melt onset of days 346..349 and the melting back
of 80N90E's young ice are the three spans in which a difference of one ulp grows past the parity bar within a few hundred steps,
so the windows of 1 000 and more steps of the older tests are held to the size of the event there, not to the bar.  Within TEN steps
nothing is amplified (the checker against its own -ffp-contract=fast build stays below 1e-11 in every ten-step window of every span,
profiles/r25_event_windows.json), so windows of ten steps restarted from the checker's state and laid end to end check every step
of an event at the bar.  `tile` is that protocol; the three spans' solvers and their start states (tests/golden/event_*.npz, written
by tests/golden/make_event_fixtures.py) are set up here so that the generator, the host replay test, the CPU measurement
(tools/event_window_sensitivity.py) and the GPU test all run the very same thing.

`g` in `tile` is any Solver: the HIP path in the GPU tests, the checker's FMA build in the CPU measurement."""
import os

import numpy as np

from samsim_amd import testcases as tcs
from samsim_amd.capi import State
from tests.helpers import RTOL, assert_state_close, golden, sheba_forcing

CLOCK_KEYS = ("time", "step", "n_time_out", "time_counter", "n_outputs")
DAY = 8641                       # steps from one output point of testcase 4 to the next
NTHREADS = min(16, len(os.sched_getaffinity(0)))

# the spans: start step and length (tests/golden/make_event_fixtures.py lists what each fixture holds)
OCEAN_STEP0, OCEAN_STEPS = 67 * DAY, 8640
SHEBA_DAYS = (346, 347, 348)
SITES_STEP0, SITES_STEPS = 59 * DAY, 4 * DAY
SITES_LATE_DAYS = (70, 100, 130)
FIXTURES = {"ocean": "event_ocean_grid_day67.npz", "sites": "event_sites_day59.npz",
            **{f"sheba{d}": f"event_sheba_day{d}.npz" for d in SHEBA_DAYS}}


def clock_of(s):
    k = s.get_clock()
    return {n: getattr(k, n) for n in CLOCK_KEYS}


def restart(second, o):
    """copy the checker's state and clock into `second`"""
    second.set_state(o.get_state())
    second.set_clock(**clock_of(o))


def deviation(a, b):
    """worst relative deviation over H_abs, S_abs, m, thick and T on the active layers (the measure of tools/freeze_up_sensitivity.py)"""
    k = np.arange(a.nlayer)[:, None] < b.n_active[None, :]
    worst = 0.0
    for n in ("H_abs", "S_abs", "m", "thick", "T"):
        floor = 1e-3 if n == "H_abs" else 1e-9
        x, y = a.arr(n)[k], b.arr(n)[k]
        if x.size:
            worst = max(worst, float(np.max(np.abs(x - y) / np.maximum(np.abs(y), floor))))
    return worst


def tile(g, o, total_steps, window, what, rtol=RTOL, seen=None):
    """windows of `window` steps end to end over `total_steps` (the last one shorter where it does not divide): each starts from the
    checker's state and clock, ends with equal STOP codes, equal N_active and every array and scalar of helpers.assert_state_close
    within `rtol`.  Returns the worst relative deviation of each window (`deviation`); `seen` collects the N_active met."""
    worst = []
    done = 0
    while done < total_steps:
        n = min(window, total_steps - done)
        step0 = o.get_clock().step
        restart(g, o)
        g.step(n)
        o.step(n)
        done += n
        stg, sto = g.get_status()[0], o.get_status()[0]
        assert np.array_equal(stg, sto), f"{what}: {n} steps from step {step0}: STOP codes differ {np.unique(stg)} vs {np.unique(sto)}"
        sg, so = g.get_state(), o.get_state()
        assert np.array_equal(sg.n_active, so.n_active), f"{what}: {n} steps from step {step0}: N_active differs"
        assert_state_close(sg, so, rtol, what=f"{what}: {n} steps from step {step0}")
        worst.append(deviation(sg, so))
        if seen is not None:
            seen.update(int(v) for v in so.n_active)
    return worst


# ---- the three spans: the same set-up for any solver (make(cfg, ncol) -> Solver) ----

def ocean_grid():
    """the 64 oceans of tests/test_gpu_parity.py::test_per_column_ocean_grid_of_columns"""
    ncol = 64
    cfg, st = tcs.testcase4(ncol)
    rng = np.random.default_rng(11)
    dq = rng.uniform(-4.0, 8.0, ncol)
    sb = rng.uniform(28.0, 36.0, ncol)
    dq[0], sb[0] = 0.0, cfg.S_bu_bottom
    return cfg, st, dq, sb


def ocean_solver(make):
    cfg, st, dq, sb = ocean_grid()
    s = make(cfg, 64)
    s.set_forcing(*sheba_forcing(), *tcs.ensemble_perturbation(64))
    s.set_ocean(dq, sb)
    return cfg, st, s


def sheba_solver(make, ncol=16):
    """the perturbed SHEBA columns of test_sheba_melt_season_teacher_forced_windows (ncol=1: the unperturbed column)"""
    cfg, _ = tcs.testcase4(1)
    s = make(cfg, ncol)
    if ncol == 1:
        s.set_forcing(*sheba_forcing())
    else:
        s.set_forcing(*sheba_forcing(), *tcs.ensemble_perturbation(ncol))
    return cfg, s


def sites_solver(make):
    """the five later ERA-interim sites of tests/background_runs.py in one handle, one unperturbed column each"""
    from tests.background_runs import SITES
    zm = golden("era_sites_forcing_more.npz")
    tables = [np.stack([zm[f"{s}_{n}"] for s in SITES]) for n in ("fl_sw", "fl_lw", "T2m", "precip")]
    ncol = len(SITES)
    cfg, st = tcs.testcase4(ncol)
    s = make(cfg, ncol)
    s.set_forcing_sites(*tables, np.arange(ncol, dtype=np.int32), None, None)
    return cfg, st, s


def make_oracle(cfg, ncol):
    from tests.oracle_lib import oracle_solver
    o = oracle_solver(cfg, ncol)
    o.set_threads(NTHREADS)
    return o


def make_hip(cfg, ncol):
    import samsim_amd
    return samsim_amd.hip_solver(cfg, ncol)


# ---- fixtures: the start state in the layout helpers.load_checkpoint reads, later states under a label ----

def pack(start, clock, later):
    """`later`: label -> (State, clock dict)"""
    d = dict(lay=start.lay, scal=start.scal, n_active=start.n_active, **clock)
    for label, (st, k) in later.items():
        d.update({f"{label}_lay": st.lay, f"{label}_scal": st.scal, f"{label}_n_active": st.n_active,
                  f"{label}_clock": np.array([k[n] for n in CLOCK_KEYS], dtype=np.float64)})
    return d


def later_state(z, label):
    st = State(np.ascontiguousarray(z[f"{label}_lay"]), np.ascontiguousarray(z[f"{label}_scal"]), np.ascontiguousarray(z[f"{label}_n_active"]))
    k = {n: (float(v) if n == "time" else int(v)) for n, v in zip(CLOCK_KEYS, z[f"{label}_clock"])}
    return st, k


def load(o, st, clock):
    o.set_state(st)
    o.set_clock(**clock)


def same_bytes(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in ((a.lay, b.lay), (a.scal, b.scal), (a.n_active, b.n_active)))
