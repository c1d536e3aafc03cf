"""The fused down sweep walks a wave's columns three layers per trip, stretch by stretch (top block, elastic block, bottom block),
with single-layer steps for a column whose interior layers end inside a trip and for the 0-2 layers a stretch has left over.  Its
request buffers go round once per trip, and the layer's own row is handed from the request buffer to `raw` and on to `prev`, which
waits for the return flow of the layer below.  Which copy of the layer body a layer of a column meets depends on the layer count,
on the grid's blocks and on the longest column of the wave -- and must not matter.

The synthetic slabs of tests/test_gpu_up_sweep_trips.py never drain (grav_drain stays 0 in every column), so the down sweep's
drainage (B), its return flow (C) and the changed-row stores never run there.  The waves here do: each column is a snapshot of one
testcase-4 column growing from open water, taken the first time it had that many active layers
(tests/golden/make_growth_wave_fixtures.py), so the wave holds 64 different N_active (at least nine in 17 columns at Nlayer 12) and every
column is above the critical Rayleigh number somewhere.  Nlayer 80 = 20+40+20, 81 = 22+39+20, 83 = 22+40+21 give, with the
geometries of the up-sweep test, every remainder 0, 1, 2 of a trip in each stretch; 12 = 4+4+4 has stretches shorter than a trip.
50 steps under the clock of the day-75 ensemble fixture,
  * against the CPU oracle at the project's bar (1e-6 relative, status and integers exact), where grav_drain must have grown in
    at least three quarters of the columns, and
  * bitwise against each of those columns run in a wave of copies of itself: what a lane gets must not depend on its wave-mates."""
import os

import numpy as np
import pytest

import samsim_amd
from samsim_amd import testcases as tcs
from samsim_amd.capi import State
from tests.helpers import RTOL, assert_state_close, golden, sheba_forcing
from tests.oracle_lib import oracle_solver

pytestmark = pytest.mark.gpu

NTHREADS = min(16, len(os.sched_getaffinity(0)))
NSTEPS = 50
WAVE = 64


def growth_wave(nlayer):
    z = golden(f"growth_wave_{nlayer}.npz")
    cfg, _ = tcs.testcase4(1, nlayer=int(z["nlayer"]), n_top=int(z["n_top"]), n_bottom=int(z["n_bottom"]))
    st = State(np.ascontiguousarray(z["lay"]), np.ascontiguousarray(z["scal"]), np.ascontiguousarray(z["n_active"]))
    c = golden("sheba_ensemble_80_day75.npz")
    clock = dict(time=float(c["time"]), step=int(c["step"]), n_time_out=int(c["n_time_out"]),
                 time_counter=int(c["time_counter"]), n_outputs=int(c["n_outputs"]))
    return cfg, st, clock


def advance(solver, st, clock):
    solver.set_forcing(*sheba_forcing(), None, None)
    solver.set_state(st)
    solver.set_clock(**clock)
    solver.set_output_window(0, 0)
    solver.step(NSTEPS)
    return solver.get_state(), solver.get_status()[0]


@pytest.mark.parametrize("nlayer,ncol,distinct", [(80, 64, 64), (81, 64, 64), (83, 64, 64), (12, 17, 9)])
def test_draining_wave_matches_oracle_and_solo_waves(nlayer, ncol, distinct):
    cfg, st, clock = growth_wave(nlayer)
    assert st.ncol == ncol and cfg.nlayer == nlayer
    assert len(np.unique(st.n_active)) >= distinct and st.n_active.min() >= 2 and st.n_active.max() == nlayer

    g = samsim_amd.hip_solver(cfg, ncol)
    mixed, status = advance(g, st, clock)
    g.close()

    o = oracle_solver(cfg, ncol)
    o.set_threads(NTHREADS)
    want, ostatus = advance(o, st, clock)
    o.close()
    grew = want.sc("grav_drain") > st.sc("grav_drain")
    print(f"Nlayer {nlayer}: oracle status {np.unique(ostatus)}, grav_drain grew in {int(grew.sum())} of {ncol} columns")
    assert 4 * int(grew.sum()) >= 3 * ncol, "the wave does not drain: the test would not reach the down sweep's B / C paths"
    assert np.array_equal(status, ostatus)
    assert not status.any(), f"STOP codes {np.unique(status)} in the mixed wave"
    assert_state_close(mixed, want, RTOL, what=f"Nlayer {nlayer}, draining wave vs oracle")

    # wave b of the second handle = 64 copies of column b
    rep = State(np.ascontiguousarray(np.repeat(st.lay, WAVE, axis=2)), np.ascontiguousarray(np.repeat(st.scal, WAVE, axis=1)),
                np.ascontiguousarray(np.repeat(st.n_active, WAVE)))
    g = samsim_amd.hip_solver(cfg, ncol * WAVE)
    solo, sstatus = advance(g, rep, clock)
    g.close()
    assert not sstatus.any()
    assert np.array_equal(solo.n_active, np.repeat(mixed.n_active, WAVE))
    assert np.array_equal(solo.scal, np.repeat(mixed.scal, WAVE, axis=1)), "scalars depend on the wave-mates"
    act = np.arange(nlayer)[:, None] < mixed.n_active[None, :]
    for name in ["H_abs", "S_abs", "m", "thick", "T", "phi", "psi_s", "psi_l", "psi_g", "S_bu"]:
        a = np.where(act, mixed.arr(name), 0.0)
        b = np.where(np.repeat(act, WAVE, axis=1), solo.arr(name), 0.0)
        assert np.array_equal(b, np.repeat(a, WAVE, axis=1)), f"{name} depends on the wave-mates"
