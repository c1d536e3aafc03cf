#!/usr/bin/env python3
"""Time the device-side histograms on the headline ensemble (1 048 576 columns x 80 layers, SHEBA day-200 fixture tiled as bench.py
tiles it, 500 warm-up steps):

  1. samsim_get_histogram of the ice thickness, ungrouped, 64 value bins;
  2. the same with 9 groups (label = column mod 9; a wave's table in LDS) and with 1 024 groups and 254 value bins (the adds go
     straight into the result table in device memory);
  3. samsim_get_profile_histogram: a 64 x 64 BY_DEPTH joint histogram of T;
  4. beside it, on the same handle, samsim_get_profile_stats of the same request -- it reads the same rows, so it is the yardstick:
     the ratio is reported -- and samsim_get_state, the only route to a distribution before.

Host clock around the calls (each ends in a stream synchronise inside the library); ten calls after two warm-ups, median and
spread.  The ungrouped histogram, the 9-group one and the joint histogram are checked against numpy over the state that get_state
returned (rows against the counts of the statistics for the joint one).

    python tools/histogram_bench.py > profiles/rN_histogram.json
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


def entries(v, nvbins, v0, dv):
    e = np.float64(v0) + np.arange(nvbins + 1, dtype=np.float64) * np.float64(dv)
    return np.searchsorted(e, v, side="right")          # the number of edges <= v (no NaN in a state without failed columns)


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
    status = g.get_status()[0]
    ok = status == 0
    cols = np.arange(a.ncol)
    state = {}

    def get_state():
        state["s"] = None                                  # one host copy at a time
        state["s"] = g.get_state()

    out = {"what": "samsim_get_histogram and samsim_get_profile_histogram against samsim_get_profile_stats and samsim_get_state on one "
                   "handle; host clock around the synchronising calls", "ncol": a.ncol, "nlayer": int(cfg.nlayer),
           "warmup_steps": a.warmup_steps, "failed_columns": int((~ok).sum()), "device": g.get_device()[1], "lib_md5": bench.lib_md5(),
           "scratch_bytes_bound": header_define("SAMSIM_HIST_SCRATCH_BYTES")}
    t = timed(get_state, a.get_state_calls, 1)
    t.update(bytes_to_host=15.0 * cfg.nlayer * a.ncol * 8)
    out["get_state"] = t
    s = state["s"]
    thick = s.sc("thickness")
    lo, hi = np.quantile(thick[ok], [0.02, 0.98])
    v0, dv = float(lo), float((hi - lo) / 64)

    t = timed(lambda: g.histogram("thickness", 64, v0, dv), a.calls, a.warmups)
    q = g.histogram("thickness", 64, v0, dv)
    t.update(nvbins=64, equal_to_numpy=bool(np.array_equal(q, np.bincount(entries(thick[ok], 64, v0, dv), minlength=66))),
             median_bracket=capi.quantile_bracket(q, v0, dv, 0.5))
    out["histogram_ungrouped"] = t
    out["ensemble_stats_one_slot"] = timed(lambda: g.ensemble_stats(["thickness"]), a.calls, a.warmups)

    labels = (cols % 9).astype(np.int32)
    g.set_groups(labels, ngroups=9)
    t = timed(lambda: g.histogram("thickness", 64, v0, dv, by_group=True), a.calls, a.warmups)
    q = g.histogram("thickness", 64, v0, dv, by_group=True)
    want = np.stack([np.bincount(entries(thick[ok & (labels == k)], 64, v0, dv), minlength=66) for k in range(9)])
    t.update(ngroups=9, nvbins=64, path="LDS table per wave", equal_to_numpy=bool(np.array_equal(q, want)))
    out["histogram_9_groups"] = t
    out["group_stats_one_slot_9_groups"] = timed(lambda: g.group_stats(["thickness"]), a.calls, a.warmups)
    g.set_groups((cols % capi.MAX_GROUPS).astype(np.int32), ngroups=capi.MAX_GROUPS)
    v0w, dvw = float(lo), float((hi - lo) / 254)
    t = timed(lambda: g.histogram("thickness", 254, v0w, dvw, by_group=True), a.calls, a.warmups)
    q = g.histogram("thickness", 254, v0w, dvw, by_group=True)
    t.update(ngroups=capi.MAX_GROUPS, nvbins=254, path="integer atomics into the result table", rows_sum_to_count=int(q.sum()) == int(ok.sum()))
    out[f"histogram_{capi.MAX_GROUPS}_groups"] = t
    g.set_groups(None)
    state["s"] = s = None

    kw = dict(axis="depth", origin="top", nbins=64, dz=0.03)
    t = timed(lambda: g.profile_histogram("T", 64, -20.0, 0.3125, **kw), a.calls, a.warmups)
    q = g.profile_histogram("T", 64, -20.0, 0.3125, **kw)
    out["profile_stats_same_request"] = timed(lambda: g.profile_stats(["T"], **kw), a.calls, a.warmups)
    ps = g.profile_stats(["T"], **kw)["T"]
    t.update(nbins=64, nvbins=64, dz=0.03, v0=-20.0, dv=0.3125, rows_sum_to_the_counts_of_profile_stats=bool(np.array_equal(q.sum(1), ps["count"])),
             entries_occupied=int((q > 0).sum()))
    out["profile_histogram_64x64_T_by_depth"] = t
    t = timed(lambda: g.profile_histogram("T", 254, -20.0, 0.08, **kw), a.calls, a.warmups)
    t.update(nbins=64, nvbins=254, passes=2)
    out["profile_histogram_64x254_T_by_depth"] = t
    out["profile_histogram_over_profile_stats"] = out["profile_histogram_64x64_T_by_depth"]["median_ms"] / out["profile_stats_same_request"]["median_ms"]
    out["get_state_over_profile_histogram"] = out["get_state"]["median_ms"] / out["profile_histogram_64x64_T_by_depth"]["median_ms"]
    out["get_state_over_histogram_ungrouped"] = out["get_state"]["median_ms"] / out["histogram_ungrouped"]["median_ms"]
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
