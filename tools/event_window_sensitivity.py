#!/usr/bin/env python3
"""How much does round-off grow inside the windows tests/test_gpu_event_windows.py tiles?  (CPU only; TEST INFRASTRUCTURE.)

The checker as built (-ffp-contract=off) against the same source with every a*b+c contracted (build_fma of
tools/freeze_up_sensitivity.py), through tests/event_windows.tile: the FMA build takes the place the HIP path has in the GPU tests,
from the committed start states, same windows.  Prints one JSON line per span: window length, number of windows, worst window.

  python tools/event_window_sensitivity.py [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import event_windows as ew  # noqa: E402
from tests.helpers import golden, load_checkpoint  # noqa: E402
from tests.oracle_lib import OracleSolver  # noqa: E402
from tools.freeze_up_sensitivity import build_fma  # noqa: E402

_fma = None


def make_fma(cfg, ncol):
    global _fma
    if _fma is None:
        _fma = C.CDLL(build_fma())
    s = OracleSolver(_fma, "oracle_", cfg, ncol)
    s.set_threads(ew.NTHREADS)
    return s


def span(name, f, o, st, clock, steps, window, recs):
    ew.load(o, st, clock)
    w = ew.tile(f, o, steps, window, name)
    rec = {"span": name, "step0": clock["step"], "steps": steps, "window": window, "windows": len(w), "checker_vs_fma_worst": max(w),
           "windows_above_1e-9": sum(x > 1e-9 for x in w)}
    recs.append(rec)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    recs = []
    _, _, o = ew.ocean_solver(ew.make_oracle)
    _, _, f = ew.ocean_solver(make_fma)
    span("ocean grid, day 67", f, o, *load_checkpoint(ew.FIXTURES["ocean"]), ew.OCEAN_STEPS, 10, recs)
    _, o = ew.sheba_solver(ew.make_oracle)
    _, f = ew.sheba_solver(make_fma)
    for day in ew.SHEBA_DAYS:
        span(f"SHEBA, day {day}", f, o, *load_checkpoint(ew.FIXTURES[f"sheba{day}"]), ew.DAY, 10, recs)
    _, _, o = ew.sites_solver(ew.make_oracle)
    _, _, f = ew.sites_solver(make_fma)
    span("five sites, days 59 to 63", f, o, *load_checkpoint(ew.FIXTURES["sites"]), ew.SITES_STEPS, 100, recs)
    z = golden(ew.FIXTURES["sites"])
    for day in ew.SITES_LATE_DAYS:
        span(f"five sites, day {day}", f, o, *ew.later_state(z, f"day{day}"), ew.DAY, ew.DAY, recs)
    # the tank experiments: the output intervals tests/test_gpu_event_windows.py::test_tank_budget_in_ten_step_windows tiles
    from samsim_amd import testcases as tcs
    for tc, output in ((2, 99), (9, 54), (33, 31)):
        cfg, st = getattr(tcs, f"testcase{tc}")(1)
        o, f = ew.make_oracle(cfg, 1), make_fma(cfg, 1)
        ew.load(o, st, dict(time=0.0, step=0, n_time_out=0, time_counter=1, n_outputs=0))
        o.set_output_window(0, 1)
        for _ in range(output):
            o.run_to_output()
        span(f"tank testcase {tc}, interval to output {output}", f, o, o.get_state(), ew.clock_of(o), o.steps_to_output(), 10, recs)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(recs, fh, indent=1)


if __name__ == "__main__":
    sys.exit(main())
