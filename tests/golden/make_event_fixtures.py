#!/usr/bin/env python3
"""TEST INFRASTRUCTURE / fixture generator: checker states at the start of the three spans tests/event_windows.py tiles.

    tests/golden/event_ocean_grid_day67.npz   64 columns over the ocean grid of test_per_column_ocean_grid_of_columns, free from open
                                              water to step 578 947 (day 67); `end`: 8 640 steps later
    tests/golden/event_sheba_day346.npz       16 perturbed SHEBA columns, tc4_melt_state.npz replicated and run on to step 2 989 786
                                              (day 346); `end`: one output interval (8 641 steps) later
    tests/golden/event_sheba_day347.npz       the same run at day 347 (the `end` of the file before, byte for byte) and 348
    tests/golden/event_sheba_day348.npz       ... at day 348 and 349
    tests/golden/event_sites_day59.npz        the five later ERA-interim sites in one handle, free from open water to step 509 819
                                              (day 59); `end`: day 63; `day70`, `day100`, `day130` and, one output interval after
                                              each, `day71`, `day101`, `day131`

    each: lay, scal, n_active and the clock as helpers.load_checkpoint reads them; a later state under its label as
    <label>_lay, <label>_scal, <label>_n_active, <label>_clock (tests/event_windows.later_state)

The CPU oracle alone does all of it (the reference tree is not read).  tests/test_event_fixtures_host.py replays the short spans
between the stored states and requires equal bytes; the long runs that lead to the start states are here only.

Run in the build container:  python tests/golden/make_event_fixtures.py [ocean] [sheba] [sites]   (about a minute on 8 cores)
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import event_windows as ew  # noqa: E402
from tests.helpers import load_checkpoint  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def advance(o, to_step, what, t0):
    n = to_step - o.get_clock().step
    assert n >= 0
    o.step(n)
    assert not o.get_status()[0].any(), f"{what}: STOP codes on the way to step {to_step}"
    print(f"  {what}: step {to_step} ({time.time() - t0:.0f} s)", flush=True)
    return o.get_state(), ew.clock_of(o)


def write(name, start, clock, later):
    out = os.path.join(GOLDEN, name)
    np.savez_compressed(out, **ew.pack(start, clock, later))
    print(f"{out}: {os.path.getsize(out) // 1024} KB, N_active {int(start.n_active.min())}..{int(start.n_active.max())} at the start, "
          + ", ".join(f"{int(s.n_active.min())}..{int(s.n_active.max())} at {k}" for k, (s, _) in later.items()), flush=True)


def ocean():
    t0 = time.time()
    cfg, st, o = ew.ocean_solver(ew.make_oracle)
    o.set_state(st)
    o.set_clock()
    start, clock = advance(o, ew.OCEAN_STEP0, "ocean grid", t0)
    end = advance(o, ew.OCEAN_STEP0 + ew.OCEAN_STEPS, "ocean grid", t0)
    ts0, ts1 = start.sc("thick_snow"), end[0].sc("thick_snow")
    print(f"  thick_snow below thick_min = {cfg.thick_min} in {int(((ts0 > 0) & (ts0 < cfg.thick_min)).sum())} columns at the start, "
          f"of which above it at the end: {int(((ts0 > 0) & (ts0 < cfg.thick_min) & (ts1 > cfg.thick_min)).sum())}")
    write(ew.FIXTURES["ocean"], start, clock, {"end": end})


def sheba():
    t0 = time.time()
    cfg, o = ew.sheba_solver(ew.make_oracle)
    st1, clock = load_checkpoint("tc4_melt_state.npz")          # the checker at day 340
    ew.load(o, st1.replicate(16), clock)
    start, clock = advance(o, ew.SHEBA_DAYS[0] * ew.DAY, "SHEBA", t0)
    for day in ew.SHEBA_DAYS:
        end = advance(o, (day + 1) * ew.DAY, "SHEBA", t0)
        for d, s in ((day, start), (day + 1, end[0])):
            ts = s.sc("thick_snow")
            print(f"  day {d}: N_active {sorted(set(s.n_active.tolist()))}, snow on {int((ts > 0).sum())} of 16 columns, thick_snow up to {ts.max():.3e}, "
                  f"T_top {s.sc('T_top').min():.3f}..{s.sc('T_top').max():.3f}")
        write(ew.FIXTURES[f"sheba{day}"], start, clock, {"end": end})
        start, clock = end


def sites():
    t0 = time.time()
    cfg, st, o = ew.sites_solver(ew.make_oracle)
    o.set_state(st)
    o.set_clock()
    start, clock = advance(o, ew.SITES_STEP0, "five sites", t0)
    later = {"end": advance(o, ew.SITES_STEP0 + ew.SITES_STEPS, "five sites", t0)}
    for day in ew.SITES_LATE_DAYS:
        later[f"day{day}"] = advance(o, day * ew.DAY, "five sites", t0)
        later[f"day{day + 1}"] = advance(o, (day + 1) * ew.DAY, "five sites", t0)
    write(ew.FIXTURES["sites"], start, clock, later)


if __name__ == "__main__":
    which = sys.argv[1:] or ["ocean", "sheba", "sites"]
    for w in which:
        {"ocean": ocean, "sheba": sheba, "sites": sites}[w]()
