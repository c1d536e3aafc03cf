#!/usr/bin/env python3
"""TEST INFRASTRUCTURE / fixture generator: one wave of columns that DRAIN, with every N_active in it.

One column of testcase 4 (SHEBA forcing, unperturbed) is integrated from open water with the CPU oracle for 1.5 million steps;
the first time each N_active >= 2 is met (looked at every CHUNK steps) its prognostic state -- H_abs, S_abs, m, thick, the
scalars -- is kept.  WAVE of those snapshots, evenly picked, are written as the columns of one wave:

    tests/golden/growth_wave_<nlayer>.npz      lay[4, nlayer, ncol], scal[NSCAL, ncol], n_active[ncol], nlayer, n_top, n_bottom

Growing ice is what the synthetic slabs of tests/test_gpu_up_sweep_trips.py are not: its lower layers are above the critical
Rayleigh number, so the down sweep's drainage, return flow and changed-row stores run in every column
(tests/test_gpu_down_sweep_trips.py).  The geometries give, with 80 = 20+40+20 and 82 = 21+41+20 of the up-sweep test, every
remainder 0, 1, 2 of a three-layer trip in each of the three stretches; 12 = 4+4+4 has stretches shorter than a trip and a wave
that is not full.  The script ends by running each wave for 50 steps under the clock of sheba_ensemble_80_day75.npz and
reporting what the test relies on (status 0, N_active kept, grav_drain grown).

Run in the build container:  python tests/golden/make_growth_wave_fixtures.py
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from samsim_amd import testcases as tcs  # noqa: E402
from samsim_amd.capi import State  # noqa: E402
from tests.oracle_lib import oracle_solver  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
NSTEPS_TOTAL = 1_500_000
CHUNK = 100
# nlayer, n_top, n_bottom, columns of the wave
GEOMETRIES = [(80, 20, 20, 64), (81, 22, 20, 64), (83, 22, 21, 64), (12, 4, 4, 17)]


def forcing():
    z = np.load(os.path.join(GOLDEN, "sheba_forcing.npz"))
    return z["fl_sw"], z["fl_lw"], z["T2m"], z["precip"]


def spin_up(nlayer, n_top, n_bottom):
    """{N_active: (lay[4, nlayer], scal[NSCAL])} of one column grown from open water"""
    cfg, st = tcs.testcase4(1, nlayer=nlayer, n_top=n_top, n_bottom=n_bottom)
    o = oracle_solver(cfg, 1)
    o.set_threads(1)
    o.set_forcing(*forcing(), None, None)
    o.set_state(st)
    o.set_clock()
    snaps = {}
    for _ in range(NSTEPS_TOTAL // CHUNK):
        o.step(CHUNK)
        s = o.get_state()
        na = int(s.n_active[0])
        if na >= 2 and na not in snaps:
            assert o.get_status()[0][0] == 0
            snaps[na] = (s.lay[:4, :, 0].copy(), s.scal[:, 0].copy())
    o.close()
    return cfg, snaps


def check(cfg, st):
    """what tests/test_gpu_down_sweep_trips.py relies on, on the oracle"""
    z = np.load(os.path.join(GOLDEN, "sheba_ensemble_80_day75.npz"))
    o = oracle_solver(cfg, st.ncol)
    o.set_threads(1)
    o.set_forcing(*forcing(), None, None)
    o.set_state(st)
    o.set_clock(time=float(z["time"]), step=int(z["step"]), n_time_out=int(z["n_time_out"]),
                time_counter=int(z["time_counter"]), n_outputs=int(z["n_outputs"]))
    o.set_output_window(0, 0)
    o.step(50)
    after, status = o.get_state(), o.get_status()[0]
    o.close()
    grew = after.sc("grav_drain") > st.sc("grav_drain")
    thin = (st.sc("thick_snow") >= cfg.thick_min / 100.0) & (st.sc("thick_snow") < cfg.thick_min)
    return (f"status 0 in {int((status == 0).sum())}/{st.ncol}, N_active kept in {int((after.n_active == st.n_active).sum())}, "
            f"grav_drain grew in {int(grew.sum())}, thin snow in {int(thin.sum())}")


def main():
    for nlayer, n_top, n_bottom, ncol in GEOMETRIES:
        t0 = time.time()
        cfg, snaps = spin_up(nlayer, n_top, n_bottom)
        have = sorted(snaps)
        pick = [have[i] for i in np.rint(np.linspace(0, len(have) - 1, ncol)).astype(int)]
        lay = np.ascontiguousarray(np.stack([snaps[n][0] for n in pick], axis=2))
        scal = np.ascontiguousarray(np.stack([snaps[n][1] for n in pick], axis=1))
        na = np.array(pick, dtype=np.int32)
        out = os.path.join(GOLDEN, f"growth_wave_{nlayer}.npz")
        np.savez_compressed(out, lay=lay, scal=scal, n_active=na, nlayer=nlayer, n_top=n_top, n_bottom=n_bottom)
        print(f"Nlayer {nlayer} = {n_top}+{cfg.n_middle}+{n_bottom}: {time.time() - t0:.0f} s, N_active {have[0]}..{have[-1]} "
              f"({len(have)} values met, {len(set(pick))} in the wave of {ncol}), {os.path.getsize(out) // 1024} KB; "
              + check(cfg, State(lay, scal, na)), flush=True)


if __name__ == "__main__":
    main()
