#!/usr/bin/env python3
"""Time the device-side sensitivities on the headline ensemble (1 048 576 columns x 80 layers, SHEBA day-200 fixture tiled as
bench.py tiles it, 500 warm-up steps), one handle, one job:

  1. samsim_get_covariance of 8 slots (thickness, T_top, m_snow, thick_snow, bulk_salin, N_active and the two perturbations),
     beside samsim_get_ensemble_stats of the same 8 slots -- the marginal moments of the same rows -- and samsim_get_state, the
     only route to a covariance before;
  2. samsim_get_profile_regression of T, S_bu and psi_l in 64 depth bins of 3 cm on precip_scale, beside
     samsim_get_profile_stats of the same request -- it walks the same rows, so it is the yardstick: the ratio is reported.

Host clock around the calls (each ends in a stream synchronise inside the library); ten calls after two warm-ups, median and
spread.  The covariance is checked against numpy over the state that get_state returned; count and mean_y of the regression
against the bytes of the statistics.

    python tools/sens_bench.py > profiles/rN_sens.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from tools.group_stats_bench import header_define, timed  # noqa: E402

SLOTS = ["thickness", "T_top", "m_snow", "thick_snow", "bulk_salin", "N_active", "dT2m", "precip_scale"]
ARRAYS = ["T", "S_bu", "psi_l"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncol", type=int, default=1 << 20)
    ap.add_argument("--warmup-steps", type=int, default=500)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--get-state-calls", type=int, default=3)
    a = ap.parse_args()

    import samsim_amd
    from samsim_amd import capi, testcases as tcs
    z, st, clock, pert = bench.load_ensemble("sheba_ensemble_80.npz")
    cfg, _ = tcs.testcase4(1, nlayer=int(z["nlayer"]), n_top=int(z["n_top"]), n_bottom=int(z["n_bottom"]))
    g = samsim_amd.hip_solver(cfg, a.ncol)
    g.set_forcing(*bench.sheba_forcing(), bench.tile(pert[0], a.ncol), bench.tile(pert[1], a.ncol))
    bench.upload_tiled(g, st, a.ncol, 0)
    g.set_clock(**clock)
    g.set_output_window(0, 0)
    g.step(a.warmup_steps)
    g.synchronize()
    ok = g.get_status()[0] == 0
    state = {}

    def get_state():
        state["s"] = None                                  # one host copy at a time
        state["s"] = g.get_state()

    out = {"what": "samsim_get_covariance against samsim_get_ensemble_stats and samsim_get_state, samsim_get_profile_regression against "
                   "samsim_get_profile_stats, on one handle; host clock around the synchronising calls", "ncol": a.ncol,
           "nlayer": int(cfg.nlayer), "warmup_steps": a.warmup_steps, "failed_columns": int((~ok).sum()), "device": g.get_device()[1],
           "lib_md5": bench.lib_md5(), "scratch_bytes_bound": header_define("SAMSIM_SENS_SCRATCH_BYTES")}
    t = timed(get_state, a.get_state_calls, 1)
    t.update(bytes_to_host=15.0 * cfg.nlayer * a.ncol * 8)
    out["get_state"] = t
    s = state["s"]
    rows = np.stack([s.n_active.astype(np.float64) if n == "N_active" else s.sc(n) for n in SLOTS])[:, ok]
    want = np.cov(rows, bias=True)
    state["s"] = s = None

    t = timed(lambda: g.covariance(SLOTS), a.calls, a.warmups)
    n, mean, cov = g.covariance(SLOTS)
    sd = np.maximum(1e-3, np.sqrt(np.diag(want)))
    rho = capi.correlation(cov)
    t.update(slots=SLOTS, count=n, worst_error_over_sx_sy_against_numpy=float(np.max(np.abs(cov - want) / np.outer(sd, sd))),
             correlation_thickness_precip_scale=float(rho[0, 7]), correlation_thick_snow_precip_scale=float(rho[3, 7]),
             correlation_thickness_dT2m=float(rho[0, 6]))
    out["covariance_8_slots"] = t
    out["ensemble_stats_same_8_slots"] = timed(lambda: g.ensemble_stats(SLOTS), a.calls, a.warmups)
    out["covariance_1_slot"] = timed(lambda: g.covariance(["thickness"]), a.calls, a.warmups)

    kw = dict(axis="depth", origin="top", nbins=64, dz=0.03)
    t = timed(lambda: g.profile_regression(ARRAYS, "precip_scale", **kw), a.calls, a.warmups)
    q = g.profile_regression(ARRAYS, "precip_scale", **kw)
    out["profile_stats_same_request"] = timed(lambda: g.profile_stats(ARRAYS, **kw), a.calls, a.warmups)
    ps = g.profile_stats(ARRAYS, **kw)
    same = all(q[n]["count"].tobytes() == ps[n]["count"].tobytes() and q[n]["mean_y"].tobytes() == ps[n]["mean"].tobytes()
               and np.sqrt(q[n]["var_y"]).tobytes() == ps[n]["std"].tobytes() for n in ARRAYS)
    corr = capi.slope_and_correlation(q["S_bu"])[1]
    t.update(arrays=ARRAYS, predictor="precip_scale", nbins=64, dz=0.03, passes=3, count_mean_std_are_the_bytes_of_profile_stats=bool(same),
             correlation_S_bu_precip_scale_min_max=[float(corr.min()), float(corr.max())])
    out["profile_regression_T_S_bu_psi_l_64_bins"] = t
    out["covariance_over_ensemble_stats"] = out["covariance_8_slots"]["median_ms"] / out["ensemble_stats_same_8_slots"]["median_ms"]
    out["profile_regression_over_profile_stats"] = (out["profile_regression_T_S_bu_psi_l_64_bins"]["median_ms"]
                                                     / out["profile_stats_same_request"]["median_ms"])
    out["get_state_over_covariance"] = out["get_state"]["median_ms"] / out["covariance_8_slots"]["median_ms"]
    out["get_state_over_profile_regression"] = out["get_state"]["median_ms"] / out["profile_regression_T_S_bu_psi_l_64_bins"]["median_ms"]
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
