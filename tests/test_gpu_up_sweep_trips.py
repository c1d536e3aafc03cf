"""The fused up sweep walks a wave's columns three layers per trip, stretch by stretch (bottom block, elastic block, top block),
with a single-layer step for the 0-2 layers a stretch has left over and with every lane sitting out the layers below its own
bottom (`k > N_active`).  Which copy of the layer body a given layer of a given column meets therefore depends on the layer
count, on the grid's blocks and on the longest column of the wave -- and must not matter.

One wave of 64 columns whose N_active values are spread over 2..Nlayer (every remainder of every stretch and the sit-out occur
inside the one wave), at Nlayer 80 = 20+40+20 (stretches of 20, 40 and 19 layers below layer 1) and at Nlayer 82 = 21+41+20
(20, 41 and 20): SHEBA winter physics and forcing, 50 steps,
  * against the CPU oracle at the project's bar (1e-6 relative, integers exact), as tests/test_gpu_parity.py does, and
  * bitwise against each of those columns run in a wave of 64 copies of itself (where every lane has the same N_active, so no
    lane sits out and the remainders fall elsewhere): what a lane gets must not depend on its wave-mates."""
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


def spread_columns(nlayer, n_top, n_bottom):
    """64 brine-saturated slabs on the regular grid (every layer thick_0), column i with N_active[i] layers, 2..nlayer: a linear
    temperature profile from -15 C at the top to -1.9 C at the bottom, S_bu 5 g/kg (in the manner of testcases.config5), under
    the snow cover, surface state and clock of the first member of the day-200 SHEBA ensemble fixture."""
    z = golden("sheba_ensemble_80.npz")
    cfg, _ = tcs.testcase4(1, nlayer=nlayer, n_top=n_top, n_bottom=n_bottom)
    na = np.rint(np.linspace(2, nlayer, WAVE)).astype(np.int32)
    assert na[0] == 2 and na[-1] == nlayer and len(np.unique(na)) == WAVE
    lay = np.zeros((4, nlayer, WAVE))
    for i, n in enumerate(na):
        k = (np.arange(n) + 0.5) / n
        T = -15.0 + (15.0 - 1.9) * k
        S_br = -18.7 * T - 0.519 * T ** 2 - 0.00535 * T ** 3      # sea-salt liquidus, mo_thermo_functions.f90:324-326
        S_bu = 5.0
        phi = 1.0 - S_bu / S_br
        H = -tcs.LATENT_HEAT + tcs.LATENT_HEAT * S_bu / S_br + 2020.0 * T + 7.6973 * T * T / 2.0
        m = cfg.thick_0 / (phi / 920.0 + (1.0 - phi) / tcs.RHO_L)
        lay[0, :n, i], lay[1, :n, i], lay[2, :n, i], lay[3, :n, i] = H * m, S_bu * m, m, cfg.thick_0
    scal = np.ascontiguousarray(np.repeat(z["scal"][:, :1], WAVE, axis=1))
    clock = dict(time=float(z["time"]), step=int(z["step"]), n_time_out=int(z["n_time_out"]),
                 time_counter=int(z["time_counter"]), n_outputs=int(z["n_outputs"]))
    return cfg, State(np.ascontiguousarray(lay), scal, na), clock


def advance(solver, st, clock):
    solver.set_forcing(*sheba_forcing(), None, None)
    solver.set_state(st)
    solver.set_clock(**clock)
    solver.set_output_window(0, 0)
    solver.step(NSTEPS)
    return solver.get_state(), solver.get_status()[0]


@pytest.mark.parametrize("nlayer,n_top,n_bottom", [(80, 20, 20), (82, 21, 20)])
def test_mixed_wave_matches_oracle_and_solo_waves(nlayer, n_top, n_bottom):
    cfg, st, clock = spread_columns(nlayer, n_top, n_bottom)

    g = samsim_amd.hip_solver(cfg, WAVE)
    mixed, status = advance(g, st, clock)
    g.close()
    assert not status.any(), f"STOP codes {np.unique(status)} in the mixed wave"

    o = oracle_solver(cfg, WAVE)
    o.set_threads(NTHREADS)
    want, ostatus = advance(o, st, clock)
    assert np.array_equal(status, ostatus)
    assert_state_close(mixed, want, RTOL, what=f"Nlayer {nlayer}, mixed wave vs oracle")

    # wave b of the second handle = 64 copies of column b
    rep = State(np.ascontiguousarray(np.repeat(st.lay, WAVE, axis=2)), np.ascontiguousarray(np.repeat(st.scal, WAVE, axis=1)),
                np.ascontiguousarray(np.repeat(st.n_active, WAVE)))
    g = samsim_amd.hip_solver(cfg, WAVE * WAVE)
    solo, sstatus = advance(g, rep, clock)
    g.close()
    assert not sstatus.any()
    first = slice(0, WAVE * WAVE, WAVE)
    assert np.array_equal(solo.n_active[first], mixed.n_active)
    assert np.array_equal(solo.n_active, np.repeat(mixed.n_active, WAVE))
    assert np.array_equal(solo.scal, np.repeat(mixed.scal, WAVE, axis=1)), "scalars depend on the wave-mates"
    act = np.arange(nlayer)[:, None] < mixed.n_active[None, :]
    for name in ["H_abs", "S_abs", "m", "thick", "T", "phi", "psi_s", "psi_l", "psi_g", "S_bu"]:
        a = np.where(act, mixed.arr(name), 0.0)
        b = np.where(np.repeat(act, WAVE, axis=1), solo.arr(name), 0.0)
        assert np.array_equal(b, np.repeat(a, WAVE, axis=1)), f"{name} depends on the wave-mates"
