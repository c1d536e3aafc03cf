#!/usr/bin/env python3
"""Cost of the weight row and the weighted reductions on the headline ensemble (1 048 576 columns x 80 layers, SHEBA day-200
fixture tiled as bench.py tiles it, 500 warm-up steps, a twin experiment scored once).  Nothing here is a bar; the record says
what the calls cost beside their unweighted counterparts, host wall clock around the blocking call (the launches and the
synchronisation included), medians of --repeats calls:

  set_weights_gauss        samsim_set_weights, GAUSS on J_SUM: the minimum, the row, its sums
  set_weights_direct       ... DIRECT on N_active: no minimum pass
  weighted_stats_8_slots   samsim_get_weighted_stats of the eight slots of tools/sens_bench.py, and of one slot
  covariance_8_slots       samsim_get_covariance of the same slots, and of one: the unweighted counterpart
  weighted_histogram       samsim_get_weighted_histogram of the thickness, 64 and 254 value bins
  histogram                samsim_get_histogram of the same requests: the unweighted counterpart
  get_weights              the whole row to the host
  get_state                the whole handle: what the posterior cost before

    python tools/weights_bench.py > profiles/rN_weights.json
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
    out = {"what": "cost of the weight row and the weighted reductions beside their unweighted counterparts on one handle; host wall "
                   "clock around the blocking calls",
           "ncol": a.ncol, "nlayer": int(cfg.nlayer), "warmup_steps": a.warmup_steps, "repeats": a.repeats, "device": g.get_device()[1],
           "lib_md5": bench.lib_md5(), "failed_columns": int((status != 0).sum())}

    # a twin experiment: the observations are one member's values
    buoy = [mk("profile", "T", 0.1 * i, interp="linear") for i in range(16)] + [mk("ice_thickness"), mk("scalar", "thick_snow")]
    member = int(np.flatnonzero(status == 0)[a.ncol // 3 % max(1, int((status == 0).sum()))])
    g.set_sensors(buoy)
    g.score(g.sensor_values([member])[:, 0])
    J = score_slot("J_SUM")
    q = g.ensemble_stats([J])[J]
    out["J_SUM"] = {"count": q.count, "mean": q.mean, "min": q.min, "max": q.max, "std": q.std}
    scale = max(q.mean, 1e-3) / 2.0                         # tempered: the mean member keeps exp(-1) of the best member's weight

    def note(label, t, **more):
        t.update(more)
        out[label] = t
        print(label, t["median_ms"], "ms", file=sys.stderr, flush=True)

    t, info = timed(lambda: g.set_weights(J, "gauss", scale), a.repeats)
    note("set_weights_gauss", t, scale=scale, info=info)
    t, _ = timed(lambda: g.set_weights("N_active", "direct"), a.repeats)
    note("set_weights_direct", t)
    info = g.set_weights(J, "gauss", scale)
    assert info["n_pos"] >= 2 and info["x_min"] == 0.0

    t, ws = timed(lambda: g.weighted_stats(SLOTS), a.repeats)
    note("weighted_stats_8_slots", t, thickness={k: float(ws["thickness"][k]) for k in ws["thickness"].dtype.names})
    t, _ = timed(lambda: g.weighted_stats(SLOTS[:1]), a.repeats)
    note("weighted_stats_1_slot", t)
    t, (cnt, mean, cov) = timed(lambda: g.covariance(SLOTS), a.repeats)
    note("covariance_8_slots", t, count=cnt, thickness={"mean": float(mean[0]), "var": float(cov[0, 0])})
    t, _ = timed(lambda: g.covariance(SLOTS[:1]), a.repeats)
    note("covariance_1_slot", t)

    th = g.ensemble_stats(["thickness"])["thickness"]
    for nv in (64, 254):
        v0, dv = th.min, (th.max - th.min) * 1.001 / nv
        t, wh = timed(lambda: g.weighted_histogram("thickness", nv, v0, dv), a.repeats)
        lo, hi = capi.weighted_quantile_bracket(wh, v0, dv, 0.05)[0], capi.weighted_quantile_bracket(wh, v0, dv, 0.95)[1]
        note(f"weighted_histogram_{nv}", t, sum=float(wh.sum()), sum_w=info["sum_w"], median_bracket=capi.weighted_quantile_bracket(wh, v0, dv, 0.5),
             bracket_5_95=(lo, hi))
        t, h = timed(lambda: g.histogram("thickness", nv, v0, dv), a.repeats)
        assert int(h.sum()) == th.count
        note(f"histogram_{nv}", t)
    t, _ = timed(lambda: g.histogram(weight_slot(), 50, 0.0, 0.02), a.repeats)
    note("histogram_of_the_weights", t)

    t, w = timed(lambda: g.weights(), 3)
    note("get_weights", t, bytes_returned=int(w.nbytes))
    del w
    whole_t, whole = timed(lambda: g.get_state(), 2)
    whole_t.update(columns=a.ncol, bytes_returned=whole.lay.nbytes + whole.scal.nbytes + whole.n_active.nbytes)
    del whole
    out["get_state_whole_handle"] = whole_t
    out["weighted_stats_8_over_covariance_8"] = out["weighted_stats_8_slots"]["median_ms"] / out["covariance_8_slots"]["median_ms"]
    out["weighted_stats_1_over_covariance_1"] = out["weighted_stats_1_slot"]["median_ms"] / out["covariance_1_slot"]["median_ms"]
    for nv in (64, 254):
        out[f"weighted_histogram_{nv}_over_histogram_{nv}"] = out[f"weighted_histogram_{nv}"]["median_ms"] / out[f"histogram_{nv}"]["median_ms"]
    out["get_state_over_weighted_stats_8"] = whole_t["median_ms"] / out["weighted_stats_8_slots"]["median_ms"]
    g.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
