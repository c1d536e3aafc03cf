#!/usr/bin/env python3
"""Cost of scoring the headline ensemble against observations (1 048 576 columns x 80 layers, SHEBA day-200 fixture tiled as
bench.py tiles it, 500 warm-up steps).  Nothing here is a bar; the record says what the calls cost, host wall clock around the
blocking call (the launch and the synchronisation included), medians of --repeats calls:

  score_buoy           one samsim_score with what a mass-balance buoy carries: a 16-sensor temperature string (LINEAR from the
                       top, every 0.1 m), the ice thickness and the snow depth: a thick-only pre-pass and one walk over thick and T
  score_buoy_group     the same restricted to one of four groups
  score_full           32 sensors over T, S_bu (S_abs and m), psi_l and ray: the pre-pass and two walks
  values_4096          samsim_get_sensor_values of the buoy for 4 096 scattered members (one piece of the device scratch)
  evaluate_eight       beside them, one evaluation of eight functionals over four arrays, as tools/functional_bench.py times it
  evaluate_mean_T      ... and of one functional that reads the rows the buoy's score reads (MEAN of T over the whole column)
  histogram_score      samsim_get_histogram of J_SUM: what a consumer of the slot costs (the rows are never stale)
  get_state            the whole handle, beside them

Beside each score the bytes its walks must read at the least and the bandwidth that makes.

    python tools/score_bench.py > profiles/rN_score.json
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
    ap.add_argument("--repeats", type=int, default=9)
    a = ap.parse_args()

    import samsim_amd
    from samsim_amd import testcases as tcs
    from samsim_amd.capi import FunctionalSpec, SensorSpec, func_slot, score_slot
    mk, fn = SensorSpec.make, FunctionalSpec.make
    z, st, clock, pert = bench.load_ensemble("sheba_ensemble_80.npz")
    cfg, _ = tcs.testcase4(1, nlayer=int(z["nlayer"]), n_top=int(z["n_top"]), n_bottom=int(z["n_bottom"]))
    g = samsim_amd.hip_solver(cfg, a.ncol)
    g.set_forcing(*bench.sheba_forcing(), bench.tile(pert[0], a.ncol), bench.tile(pert[1], a.ncol))
    bench.upload_tiled(g, st, a.ncol, 0)
    g.set_clock(**clock)
    g.set_output_window(0, 0)
    g.step(a.warmup_steps)
    g.synchronize()
    N = int(cfg.nlayer)
    status = g.get_status()[0]
    out = {"what": "cost of scoring the ensemble against observations on one handle; host wall clock around the blocking calls",
           "ncol": a.ncol, "nlayer": N, "warmup_steps": a.warmup_steps, "repeats": a.repeats, "device": g.get_device()[1],
           "lib_md5": bench.lib_md5(), "failed_columns": int((status != 0).sum())}
    na = g.ensemble_stats(["N_active"])["N_active"]
    out["n_active"] = {"mean": na.mean, "min": na.min, "max": na.max}
    # a wave reads whole 512-byte rows up to its largest n_active; the mean over the columns is the lower bound quoted here
    row_bytes = 8.0 * a.ncol * na.mean
    g.set_groups((np.arange(a.ncol, dtype=np.int64) % 4).astype(np.int32), ngroups=4)

    buoy = [mk("profile", "T", 0.1 * i, interp="linear") for i in range(16)] + [mk("ice_thickness"), mk("scalar", "thick_snow")]
    full = ([mk("profile", "T", 0.1 * i, interp="linear") for i in range(16)]
            + [mk("profile", "S_bu", 0.05 + 0.1 * i, "bottom") for i in range(8)]
            + [mk("profile", "psi_l", 0.1 * i, "bottom", "linear") for i in range(4)] + [mk("profile", "ray", 0.1 * i, "bottom") for i in range(2)]
            + [mk("ice_thickness"), mk("scalar", "thick_snow")])
    member = int(np.flatnonzero(status == 0)[a.ncol // 3 % max(1, int((status == 0).sum()))])
    # rows per layer: the pre-pass over thick, a walk over thick and T; and the pre-pass, a walk over thick, T, S_abs, m and psi_l,
    # a walk over thick and ray
    for label, specs, rows, group in (("score_buoy", buoy, 3, None), ("score_buoy_group", buoy, 3, 1), ("score_full", full, 1 + 5 + 2, None)):
        g.set_sensors(specs)
        obs = g.sensor_values([member])[:, 0]              # a twin experiment: the observations are one member's values
        t, _ = timed(lambda: g.score(obs, group=group), a.repeats)
        share = 0.25 if group is not None else 1.0
        t.update(sensors=len(specs), layer_rows_read=rows, bytes_read=rows * row_bytes * share,
                 TBps=rows * row_bytes * share / (t["median_ms"] * 1e-3) / 1e12, in_the_ice_for_the_member=int((~np.isnan(obs)).sum()))
        out[label] = t
        print(label, t["median_ms"], "ms", file=sys.stderr, flush=True)
    g.set_sensors(buoy)
    obs = g.sensor_values([member])[:, 0]
    g.score(obs)
    r = g.scores()
    assert r["J_LAST"][member] == 0.0 and r["CALLS"][member] == 1.0
    q = g.ensemble_stats([score_slot("J_SUM")])[score_slot("J_SUM")]
    out["J_SUM"] = {"count": q.count, "mean": q.mean, "min": q.min, "max": q.max, "std": q.std}
    del r
    cols = (np.arange(4096, dtype=np.int64) * 7919) % a.ncol
    out["values_4096"], _ = timed(lambda: g.sensor_values(cols), a.repeats)
    nv, v0, dv = 50, 0.0, max(q.max, 1e-3) / 49.0
    out["histogram_score"], h = timed(lambda: g.histogram(score_slot("J_SUM"), nv, v0, dv), a.repeats)
    assert int(h.sum()) == q.count
    out["histogram_counts"] = [int(x) for x in h]

    eight = [fn("thickness_where", "psi_l", sense=1, threshold=0.05),
             fn("crossing_depth", "psi_l", sense=1, threshold=0.05, missing=-1.0),
             fn("crossing_depth", "T", sense=1, threshold=-5.0, missing=-1.0),
             fn("min", "T", missing=0.0),
             fn("mean", "S_bu", z_hi=0.5, missing=-1.0),
             fn("integral", "psi_l"),
             fn("max", "ray", missing=-1.0),
             fn("depth_of_max", "ray", "bottom", missing=-1.0)]
    for label, specs, rows in (("evaluate_eight", eight, 1 + 5 + 2), ("evaluate_mean_T", [fn("mean", "T", missing=0.0)], 2)):
        t, _ = timed(lambda: g.functionals(0, 0, 1), a.repeats, before=lambda: g.set_functionals(specs))
        t.update(functionals=len(specs), layer_rows_read=rows, bytes_read=rows * row_bytes,
                 TBps=rows * row_bytes / (t["median_ms"] * 1e-3) / 1e12)
        out[label] = t
        print(label, t["median_ms"], "ms", file=sys.stderr, flush=True)
    assert func_slot(0) == 0x20000
    whole_t, whole = timed(lambda: g.get_state(), 2)
    whole_t.update(columns=a.ncol, bytes_returned=whole.lay.nbytes + whole.scal.nbytes + whole.n_active.nbytes)
    del whole
    out["get_state_whole_handle"] = whole_t
    out["score_buoy_over_evaluate_mean_T"] = out["score_buoy"]["median_ms"] / out["evaluate_mean_T"]["median_ms"]
    out["score_full_over_evaluate_eight"] = out["score_full"]["median_ms"] / out["evaluate_eight"]["median_ms"]
    out["get_state_over_score_buoy"] = whole_t["median_ms"] / out["score_buoy"]["median_ms"]
    g.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
