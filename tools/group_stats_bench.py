#!/usr/bin/env python3
"""Time samsim_get_group_stats on the headline ensemble (1 048 576 columns x 80 layers, SHEBA day-200 fixture tiled as bench.py
tiles it, 500 warm-up steps): the Fortran host's six slots with 9 groups (columns interleaved over nine sites, label = column
mod 9) and with 1 024 groups, beside -- on the same handle -- samsim_get_ensemble_stats of the same six slots (the ungrouped
reduction) and samsim_get_state (the only route to per-group numbers before the labels existed).  One
samsim_get_group_profile_stats call for one of the nine groups is timed as well: a request for G groups is G such calls.

Host clock around the calls (each ends in a stream synchronise inside the library); ten calls after two warm-ups, median and
spread.  The first grouped result is checked against numpy over the state that get_state returned.

    python tools/group_stats_bench.py > profiles/rN_group_stats.json
"""
import argparse
import json
import os
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

SLOTS = ["thickness", "thick_snow", "bulk_salin", "freeboard", "T_top", "N_active"]     # output_ensemble of host/host_driver.f90


def header_define(name):
    text = open(os.path.join(ROOT, "include", "samsim.h")).read()
    return re.search(rf"^#define {name}\s+(.+)$", text, re.M).group(1).strip()


def timed(fn, calls, warmups):
    for _ in range(warmups):
        fn()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "calls": calls, "warmups": warmups}


def worst_error(q, s, status, labels, ngroups):
    """largest deviations of the grouped statistics from numpy over the host copy of the state (mean relative to max(1, |mean|),
    std relative to max(1e-3, std)); counts and extremes must be equal"""
    ok = np.flatnonzero((status == 0) & (labels >= 0))
    order = ok[np.argsort(labels[ok], kind="stable")]
    bounds = np.searchsorted(labels[order], np.arange(ngroups + 1))
    mean_err = std_err = 0.0
    exact = True
    for n in SLOTS:
        row = s.n_active.astype(np.float64) if n == "N_active" else s.sc(n)
        for g in range(ngroups):
            v = row[order[bounds[g]:bounds[g + 1]]]
            x = q[n][g]
            exact = exact and x["count"] == v.size and x["min"] == v.min() and x["max"] == v.max()
            mean_err = max(mean_err, abs(x["mean"] - v.mean()) / max(1.0, abs(v.mean())))
            std_err = max(std_err, abs(x["std"] - v.std()) / max(1e-3, v.std()))
    return {"count_min_max_exact": bool(exact), "mean_err": float(mean_err), "std_err": float(std_err)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncol", type=int, default=1 << 20)
    ap.add_argument("--warmup-steps", type=int, default=500)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--get-state-calls", type=int, default=None, help="default: --calls")
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
    cols = np.arange(a.ncol)
    state = {}

    def get_state():
        state["s"] = None                                  # one host copy at a time
        state["s"] = g.get_state()

    out = {"what": "samsim_get_group_stats against samsim_get_ensemble_stats and samsim_get_state on one handle; host clock around "
                   "the synchronising calls", "ncol": a.ncol, "nlayer": int(cfg.nlayer), "warmup_steps": a.warmup_steps,
           "failed_columns": int((status != 0).sum()), "slots": SLOTS, "device": g.get_device()[1], "lib_md5": bench.lib_md5(),
           "scratch_bytes_bound": header_define("SAMSIM_GROUP_SCRATCH_BYTES"), "max_groups": capi.MAX_GROUPS}
    t = timed(get_state, a.calls if a.get_state_calls is None else a.get_state_calls, a.warmups)
    t.update(bytes_to_host=15.0 * cfg.nlayer * a.ncol * 8)
    out["get_state"] = t
    for ngroups in (9, capi.MAX_GROUPS):
        labels = (cols % ngroups).astype(np.int32)
        g.set_groups(labels, ngroups=ngroups)
        t = timed(lambda: g.group_stats(SLOTS), a.calls, a.warmups)
        t.update(ngroups=ngroups, ms_per_slot=t["median_ms"] / len(SLOTS))
        t["against_numpy"] = worst_error(g.group_stats(SLOTS), state["s"], status, labels, ngroups)
        out[f"group_stats_{ngroups}_groups"] = t
    out["ensemble_stats"] = timed(lambda: g.ensemble_stats(SLOTS), a.calls, a.warmups)
    g.set_groups((cols % 9).astype(np.int32), ngroups=9)
    t = timed(lambda: g.profile_stats(["T", "S_bu", "psi_l"], axis="depth", origin="top", nbins=64, dz=0.03, group=4), a.calls, a.warmups)
    t.update(ngroups=9, group=4, nbins=64, dz=0.03, arrays=["T", "S_bu", "psi_l"])
    out["group_profile_stats_one_of_9_groups"] = t
    state["s"] = None
    for k in ("group_stats_9_groups", f"group_stats_{capi.MAX_GROUPS}_groups"):
        out[f"get_state_over_{k}"] = out["get_state"]["median_ms"] / out[k]["median_ms"]
        out[f"{k}_over_ensemble_stats"] = out[k]["median_ms"] / out["ensemble_stats"]["median_ms"]
    out["grouped_faster_than_get_state"] = bool(max(out["group_stats_9_groups"]["max_ms"],
                                                    out[f"group_stats_{capi.MAX_GROUPS}_groups"]["max_ms"]) < out["get_state"]["min_ms"])
    print(json.dumps(out, indent=1))
    if not out["grouped_faster_than_get_state"]:
        sys.exit("the grouped reduction did not beat samsim_get_state")


if __name__ == "__main__":
    main()
