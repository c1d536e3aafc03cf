#!/usr/bin/env python3
"""Cost of the weighted joint histogram of a profile on the headline ensemble (1 048 576 columns x 80 layers, SHEBA day-200 fixture
tiled as bench.py tiles it, 500 warm-up steps, a twin experiment scored once, GAUSS weights).  Nothing here is a bar; the record
says what the call costs beside what the library offered for the same request before, host wall clock around the blocking call (the
launches and the synchronisation included), medians of --repeats calls with min and max.  The request is T by depth from the top,
64 bins, with 64 and with 254 value bins, over all columns and over one group of eight:

  weighted_profile_histogram   samsim_get_weighted_profile_histogram
  profile_histogram            samsim_get_profile_histogram of the same request: the unweighted counterpart
  weighted_profile_stats       samsim_get_weighted_profile_stats of the same request: the posterior moments
  get_state                    the whole handle, once: what the posterior band of a depth bin cost before

    python tools/weighted_profile_hist_bench.py > profiles/rN_weighted_profile_hist.json

SAMSIM_HIP_LIB selects a measuring build of the library (make variant EXTRA=-DDEV_WPHIST_GRID=...; a cap above the product's also
needs a larger SAMSIM_WPHIST_SCRATCH_BYTES, as the static_assert of samsim_wphist.h says): --label names it in the record.
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
    ap.add_argument("--label", default="product")
    ap.add_argument("--new-call-only", action="store_true", help="time the new call alone (a grid-cap variant)")
    a = ap.parse_args()

    import samsim_amd
    from samsim_amd import capi, testcases as tcs
    from samsim_amd.capi import SensorSpec, score_slot
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
    out = {"what": "cost of the weighted joint histogram of a profile beside its counterparts on one handle; host wall clock around "
                   "the blocking calls",
           "label": a.label, "library": os.environ.get("SAMSIM_HIP_LIB", "product"),
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
    g.set_groups((np.arange(a.ncol) % 8).astype(np.int32), ngroups=8)

    def note(label, t, **more):
        t.update(more)
        out[label] = t
        print(label, t["median_ms"], "ms", file=sys.stderr, flush=True)

    def ratio(label, num, den):
        n, d = out[num], out[den]
        out[label] = {"of_medians": n["median_ms"] / d["median_ms"], "lowest": n["min_ms"] / d["max_ms"], "highest": n["max_ms"] / d["min_ms"]}

    # T by depth from the top, 64 bins that reach below the thickest column; the value bins span the ensemble's temperatures
    th = g.ensemble_stats(["thickness"])["thickness"]
    kw = dict(axis="depth", origin="top", nbins=64, z0=0.0, dz=th.max * 1.05 / 64)
    prior = g.profile_stats(["T"], **kw)["T"]
    full = prior["count"] > 0
    t_lo, t_hi = float(prior["min"][full].min()), float(prior["max"][full].max())
    out["request"] = dict(kw, array="T", value_range=[t_lo, t_hi])
    for nvbins in (64, 254):
        v0, dv = t_lo, (t_hi - t_lo) * 1.001 / nvbins
        passes = {"weighted": -(-64 // capi.wphist_chunk(nvbins)), "unweighted": -(-64 // min(64, 65024 // (520 + 4 * ((nvbins + 2) | 1))))}
        for group, tag in ((None, "all"), (3, "group")):
            key = f"{nvbins}_{tag}"
            t, ws = timed(lambda: g.weighted_profile_histogram("T", nvbins, v0, dv, group=group, **kw), a.repeats)
            lo, hi = capi.weighted_profile_quantiles(ws, v0, dv, (0.05, 0.5, 0.95))
            note(f"weighted_profile_histogram_{key}", t, passes=passes["weighted"], entries_with_weight=int((ws > 0.0).sum()),
                 bin_0_band=[[float(lo[k, 0]), float(hi[k, 0])] for k in range(3)])
            if a.new_call_only:
                continue
            t, cnt = timed(lambda: g.profile_histogram("T", nvbins, v0, dv, group=group, **kw), a.repeats)
            assert np.array_equal(cnt > 0, ws > 0.0)        # every weight is positive here
            note(f"profile_histogram_{key}", t, passes=passes["unweighted"])
            t, wp = timed(lambda: g.weighted_profile_stats(["T"], group=group, **kw), a.repeats)
            rows, held = ws.sum(1), wp["T"]["count"] > 0
            note(f"weighted_profile_stats_{key}", t,
                 worst_row_sum_difference=float(np.max(np.abs(rows - wp["T"]["sum_w"])[held] / wp["T"]["sum_w"][held])))
            ratio(f"weighted_profile_histogram_over_profile_histogram_{key}", f"weighted_profile_histogram_{key}", f"profile_histogram_{key}")
            ratio(f"weighted_profile_histogram_over_weighted_profile_stats_{key}", f"weighted_profile_histogram_{key}",
                  f"weighted_profile_stats_{key}")
            out[f"weighted_over_unweighted_per_pass_{key}"] = (out[f"weighted_profile_histogram_{key}"]["median_ms"] / passes["weighted"]) / (
                out[f"profile_histogram_{key}"]["median_ms"] / passes["unweighted"])

    if not a.new_call_only:
        whole_t, whole = timed(lambda: g.get_state(), 1)
        whole_t.update(columns=a.ncol, bytes_returned=whole.lay.nbytes + whole.scal.nbytes + whole.n_active.nbytes)
        del whole
        out["get_state_whole_handle"] = whole_t
        for key in ("64_all", "254_all"):
            out[f"get_state_over_weighted_profile_histogram_{key}"] = whole_t["median_ms"] / out[f"weighted_profile_histogram_{key}"]["median_ms"]
    g.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
