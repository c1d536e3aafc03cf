#!/usr/bin/env python3
"""Cost of the rejuvenation on the device, on the headline ensemble (1 048 576 columns x 80 layers, SHEBA day-200 fixture tiled as
bench.py tiles it, both ocean rows set, --warmup-steps steps on, the twin-experiment GAUSS row of tools/copy_bench.py).  Host wall
clock around the blocking call (the launches and the synchronisation included), medians of --repeats calls with min and max:

  jitter_pool_4       samsim_jitter of four terms over the pool: the map reads and writes four rows of ncol doubles and reads the
                      status row; row_gb_s counts those bytes
  jitter_pool_1       ... of one term
  jitter_copies_4     ... of four terms over the copies of a balanced systematic draw at an effective sample size of --ess of the pool
  rejuvenate_1        Solver.rejuvenate of dT2m: one covariance call for the moments, then the jitter
  assimilate          one whole cycle of Solver.assimilate with ess_frac 1.0 (score, weights, resample, apply with the forcing,
                      rejuvenate, reset of the scores), after --cycle-steps steps
  host_get_state      samsim_get_state of the whole handle with the four prognostic arrays, the cheapest call that returns the scalar
                      rows, and host_set_forcing the upload of new perturbation rows with the tables: the route through the host
                      the jitter of the two forcing rows replaces (for the ocean rows there was none)

    python tools/jitter_bench.py > profiles/rN_jitter.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from tools.functional_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncol", type=int, default=1 << 20)
    ap.add_argument("--warmup-steps", type=int, default=500)
    ap.add_argument("--cycle-steps", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--ess", type=float, default=0.7, help="effective sample size of the weight row, as a share of the pool")
    a = ap.parse_args()

    import samsim_amd
    from samsim_amd import capi, testcases as tcs
    from samsim_amd.capi import JitterTerm, SensorSpec, score_slot
    mk = SensorSpec.make
    z, st, clock, pert = bench.load_ensemble("sheba_ensemble_80.npz")
    cfg, _ = tcs.testcase4(1, nlayer=int(z["nlayer"]), n_top=int(z["n_top"]), n_bottom=int(z["n_bottom"]))
    forcing = bench.sheba_forcing()
    g = samsim_amd.hip_solver(cfg, a.ncol)
    g.set_forcing(*forcing, bench.tile(pert[0], a.ncol), bench.tile(pert[1], a.ncol))
    rng = np.random.default_rng(24)
    g.set_ocean(rng.normal(0.0, 0.5, a.ncol), cfg.S_bu_bottom + rng.uniform(-0.5, 0.5, a.ncol))
    bench.upload_tiled(g, st, a.ncol, 0)
    g.set_clock(**clock)
    g.set_output_window(0, 0)
    g.step(a.warmup_steps)
    g.synchronize()
    status = g.get_status()[0]
    n_pool = int((status == 0).sum())
    out = {"what": "cost of samsim_jitter, Solver.rejuvenate and Solver.assimilate beside the route through the host; host wall clock "
                   "around the blocking calls", "ncol": a.ncol, "nlayer": int(cfg.nlayer), "warmup_steps": a.warmup_steps,
           "repeats": a.repeats, "device": g.get_device()[1], "lib_md5": bench.lib_md5(), "failed_columns": a.ncol - n_pool}

    def note(label, t, **more):
        t.update(more)
        out[label] = t
        print(label, t["median_ms"], "ms", file=sys.stderr, flush=True)

    def row_gb_s(t, nterms, n):
        return (16.0 * nterms + 4.0) * n / (t["median_ms"] * 1e-3) / 1e9

    # shrink 1 and a small sigma: the rows keep their spread however often the call is repeated
    terms = [JitterTerm.make("dT2m", 0.0, 1.0, 1e-3), JitterTerm.make("precip_scale", 1.0, 1.0, 1e-4, 0.0, 10.0),
             JitterTerm.make("dfl_q_bottom", 0.0, 1.0, 1e-3), JitterTerm.make("S_bu_bottom", 34.0, 1.0, 1e-3, 0.0, 100.0)]
    seeds = iter(range(1, 1 << 20))
    t, info = timed(lambda: g.jitter(terms, "pool", next(seeds)), a.repeats)
    note("jitter_pool_4", t, info=info, row_gb_s=row_gb_s(t, 4, a.ncol))
    t, info = timed(lambda: g.jitter(terms[:1], "pool", next(seeds)), a.repeats)
    note("jitter_pool_1", t, info=info, row_gb_s=row_gb_s(t, 1, a.ncol))
    t, info = timed(lambda: g.rejuvenate(["dT2m"], 0.98, next(seeds)), a.repeats)
    note("rejuvenate_1", t, info={k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in info.items()})

    # the twin experiment of tools/copy_bench.py, the tempering chosen by bisection for the effective sample size asked for
    buoy = [mk("profile", "T", 0.1 * i, interp="linear") for i in range(16)] + [mk("ice_thickness"), mk("scalar", "thick_snow")]
    member = int(np.flatnonzero(status == 0)[a.ncol // 3 % max(1, n_pool)])
    g.set_sensors(buoy)
    g.score(g.sensor_values([member])[:, 0])
    J = score_slot("J_SUM")
    lo, hi = 1e-6, 1e12
    for _ in range(40):
        scale = float(np.sqrt(lo * hi))
        winfo = g.set_weights(J, "gauss", scale)
        if winfo["ess"] < a.ess * n_pool:
            lo = scale
        else:
            hi = scale
    out["weights"] = dict(winfo, scale=scale, ess_share=winfo["ess"] / n_pool)
    g.resample(n_pool, "systematic", u0=0.37)
    plan = g.apply_resample(forcing=True)
    t, info = timed(lambda: g.jitter(terms, "copies", next(seeds)), a.repeats)
    note("jitter_copies_4", t, plan=plan, info=info, row_gb_s=row_gb_s(t, 4, plan["n_copies"]))

    # one whole cycle, every round resampling
    def advance():
        g.step(a.cycle_steps)
        g.synchronize()
    obs_of = lambda: g.sensor_values([member])[:, 0]                      # noqa: E731
    cycles = []

    def cycle():
        r = g.assimilate(obs_of(), scale=scale, ess_frac=1.0, seed=next(seeds), targets=("dT2m", "precip_scale"))
        cycles.append({"ess": r["ess"], "n_survivors": r["n_survivors"], "n_copies": r["n_copies"]})
        return r
    t, _ = timed(cycle, min(a.repeats, 5), before=advance)
    note("assimilate", t, cycle_steps=a.cycle_steps, cycles=cycles, includes="the download of one member's sensor values")

    # the route through the host for the two forcing rows
    t, s = timed(lambda: g.get_state(narr=capi.NPROG), 3)
    note("host_get_state", t, bytes_returned=int(s.lay.nbytes + s.scal.nbytes + s.n_active.nbytes))
    d, p = s.sc("dT2m").copy(), s.sc("precip_scale").copy()
    del s
    t, _ = timed(lambda: g.set_forcing(*forcing, d, p), 3)
    note("host_set_forcing", t)
    out["host_route_ms"] = out["host_get_state"]["median_ms"] + t["median_ms"]
    out["host_route_over_jitter_pool_4"] = out["host_route_ms"] / out["jitter_pool_4"]["median_ms"]
    g.close()
    print(json.dumps(out, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
