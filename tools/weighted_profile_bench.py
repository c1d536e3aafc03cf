#!/usr/bin/env python3
"""Cost of the weighted profile statistics and the weighted covariances on the headline ensemble (1 048 576 columns x 80 layers,
SHEBA day-200 fixture tiled as bench.py tiles it, 500 warm-up steps, a twin experiment scored once, GAUSS weights).  Nothing here
is a bar; the record says what the two calls cost beside what the library offered for the same questions before, host wall clock
around the blocking call (the launches and the synchronisation included), medians of --repeats calls with min and max:

  weighted_profile_stats   samsim_get_weighted_profile_stats, one array (T), BY_DEPTH from the top, 64 bins
  profile_regression       samsim_get_profile_regression of the same request with the weight slot as predictor: the posterior mean
                           sideways, no spread
  profile_stats            samsim_get_profile_stats of the same request: the unweighted counterpart
  weighted_covariance      samsim_get_weighted_covariance of one slot and of the eight slots of tools/sens_bench.py
  covariance               samsim_get_covariance of the same slots: the unweighted counterpart
  weighted_stats           samsim_get_weighted_stats of the same slots: the diagonal alone
  get_state                the whole handle, once: what the posterior spread of a depth bin cost before

    python tools/weighted_profile_bench.py > profiles/rN_weighted_profiles.json
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

SLOTS = ["thickness", "T_top", "m_snow", "thick_snow", "bulk_salin", "N_active", "dT2m", "precip_scale"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncol", type=int, default=1 << 20)
    ap.add_argument("--warmup-steps", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=9)
    a = ap.parse_args()

    import samsim_amd
    from samsim_amd import capi, testcases as tcs
    from samsim_amd.capi import SensorSpec, score_slot, weight_slot
    mk = SensorSpec.make
    z, st, clock, pert = bench.load_ensemble("sheba_ensemble_80.npz")
    cfg, _ = tcs.testcase4(1, nlayer=int(z["nlayer"]), n_top=int(z["n_top"]), n_bottom=int(z["n_bottom"]))
    g = samsim_amd.hip_solver(cfg, a.ncol)
    g.set_forcing(*bench.sheba_forcing(), bench.tile(pert[0], a.ncol), bench.tile(pert[1], a.ncol))
    bench.upload_tiled(g, st, a.ncol, 0)
    g.set_clock(**clock)
    g.set_output_window(0, 0)
    g.step(a.warmup_steps)
    g.synchronize()
    status = g.get_status()[0]
    out = {"what": "cost of the weighted profile statistics and the weighted covariances beside their counterparts on one handle; "
                   "host wall clock around the blocking calls",
           "ncol": a.ncol, "nlayer": int(cfg.nlayer), "warmup_steps": a.warmup_steps, "repeats": a.repeats, "device": g.get_device()[1],
           "lib_md5": bench.lib_md5(), "failed_columns": int((status != 0).sum())}

    # a twin experiment: the observations are one member's values
    buoy = [mk("profile", "T", 0.1 * i, interp="linear") for i in range(16)] + [mk("ice_thickness"), mk("scalar", "thick_snow")]
    member = int(np.flatnonzero(status == 0)[a.ncol // 3 % max(1, int((status == 0).sum()))])
    g.set_sensors(buoy)
    g.score(g.sensor_values([member])[:, 0])
    J = score_slot("J_SUM")
    q = g.ensemble_stats([J])[J]
    scale = max(q.mean, 1e-3) / 2.0                         # tempered: the mean member keeps exp(-1) of the best member's weight
    info = g.set_weights(J, "gauss", scale)
    assert info["n_pos"] >= 2 and info["x_min"] == 0.0
    out["weights"] = dict(info, scale=scale, ess_over_n_in=info["ess"] / max(1, info["n_in"]))

    def note(label, t, **more):
        t.update(more)
        out[label] = t
        print(label, t["median_ms"], "ms", file=sys.stderr, flush=True)

    def ratio(label, num, den):
        n, d = out[num], out[den]
        out[label] = {"of_medians": n["median_ms"] / d["median_ms"], "lowest": n["min_ms"] / d["max_ms"], "highest": n["max_ms"] / d["min_ms"]}

    # ---- the posterior profile: one array by depth, 64 bins that reach below the thickest column
    th = g.ensemble_stats(["thickness"])["thickness"]
    kw = dict(axis="depth", origin="top", nbins=64, z0=0.0, dz=th.max * 1.05 / 64)
    t, wp = timed(lambda: g.weighted_profile_stats(["T"], **kw), a.repeats)
    wp = wp["T"]
    full = wp["count"] > 0
    note("weighted_profile_stats", t, request=kw, bins_with_columns=int(full.sum()),
         bin_0={k: float(wp[k][0]) for k in wp.dtype.names},
         ess_of_the_bins={"min": float((wp["sum_w"][full] ** 2 / wp["sum_w2"][full]).min()),
                          "max": float((wp["sum_w"][full] ** 2 / wp["sum_w2"][full]).max())})
    t, reg = timed(lambda: g.profile_regression(["T"], weight_slot(), **kw), a.repeats)
    via = capi.weighted_profile_mean(reg["T"])
    note("profile_regression_on_the_weight", t,
         worst_difference_of_the_means=float(np.max(np.abs(via[full] - wp["mean"][full]) / np.maximum(1.0, np.abs(wp["mean"][full])))))
    t, ps = timed(lambda: g.profile_stats(["T"], **kw), a.repeats)
    assert np.array_equal(ps["T"]["count"], wp["count"])     # every weight is positive here
    note("profile_stats", t)

    # ---- the posterior covariance
    for n in (1, 8):
        t, (cnt, sw, sw2, mean, cov) = timed(lambda: g.weighted_covariance(SLOTS[:n]), a.repeats)
        more = {"correlation_thickness_dT2m": float(capi.correlation(cov)[0, 6])} if n == 8 else {}
        note(f"weighted_covariance_{n}", t, count=cnt, sum_w=sw, thickness={"mean": float(mean[0]), "var": float(cov[0, 0])}, **more)
        t, (cnt, mean, cov) = timed(lambda: g.covariance(SLOTS[:n]), a.repeats)
        more = {"correlation_thickness_dT2m": float(capi.correlation(cov)[0, 6])} if n == 8 else {}
        note(f"covariance_{n}", t, count=cnt, thickness={"mean": float(mean[0]), "var": float(cov[0, 0])}, **more)
        t, ws = timed(lambda: g.weighted_stats(SLOTS[:n]), a.repeats)
        assert ws["thickness"]["var"] == out[f"weighted_covariance_{n}"]["thickness"]["var"]       # the diagonal, byte for byte
        note(f"weighted_stats_{n}", t)

    whole_t, whole = timed(lambda: g.get_state(), 1)
    whole_t.update(columns=a.ncol, bytes_returned=whole.lay.nbytes + whole.scal.nbytes + whole.n_active.nbytes)
    del whole
    out["get_state_whole_handle"] = whole_t

    ratio("weighted_profile_stats_over_profile_regression", "weighted_profile_stats", "profile_regression_on_the_weight")
    ratio("weighted_profile_stats_over_profile_stats", "weighted_profile_stats", "profile_stats")
    for n in (1, 8):
        ratio(f"weighted_covariance_{n}_over_covariance_{n}", f"weighted_covariance_{n}", f"covariance_{n}")
        ratio(f"weighted_covariance_{n}_over_weighted_stats_{n}", f"weighted_covariance_{n}", f"weighted_stats_{n}")
    out["get_state_over_weighted_profile_stats"] = whole_t["median_ms"] / out["weighted_profile_stats"]["median_ms"]
    g.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
