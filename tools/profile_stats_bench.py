#!/usr/bin/env python3
"""Time samsim_get_profile_stats on the headline ensemble (1 048 576 columns x 80 layers, SHEBA day-200 fixture tiled as
bench.py tiles it, 500 warm-up steps) beside samsim_get_state of the same handle -- the only route to the layer profiles of an
ensemble before the device reduction existed.

Host clock around the calls (each ends in a stream synchronise inside the library); ten calls after two warm-ups, median and
spread.  The bytes a request must read are computed from shapes: distinct rows needed x sum(N_active) x 8; the reduction serves a
request in passes of one array, so the depth axis reads `thick` once per array (bytes_read_by_passes).

    python tools/profile_stats_bench.py > profiles/rN_profile_stats.json
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

HBM_ACHIEVABLE_TBS = 6.3    # measured copy bandwidth of the MI355X (8.0 TB/s spec)


def header_define(name):
    text = open(os.path.join(ROOT, "include", "samsim.h")).read()
    return re.search(rf"^#define {name}\s+(.+)$", text, re.M).group(1).strip()


def resource_usage(path):
    """compiler remarks (-Rpass-analysis=kernel-resource-usage) of the profile kernels as `make resource-usage` prints them, from a
    file whose first line names the sources they were taken from (`# src_md5 <bench.source_md5()>`): remarks of other sources
    are not quoted"""
    if not path or not os.path.exists(path):
        return None
    lines = open(path).read().splitlines()
    m = re.match(r"# src_md5 (\w+)", lines[0]) if lines else None
    if not m or m.group(1) != bench.source_md5():
        return {"not_quoted": f"{os.path.basename(path)} does not name the sources of the library being timed"}
    out, cur = {"src_md5": m.group(1)}, None
    for line in lines[1:]:
        m = re.search(r"Function Name: \S*?(profile_\w+?_kernel)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill|"
                      r"LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    return out


def timed(fn, calls, warmups):
    for _ in range(warmups):
        fn()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "calls": calls, "warmups": warmups}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncol", type=int, default=1 << 20)
    ap.add_argument("--warmup-steps", type=int, default=500)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--dz", type=float, default=0.03)
    ap.add_argument("--get-state-calls", type=int, default=None, help="default: --calls")
    ap.add_argument("--resource-usage", default=None,
                    help="file with the compiler's remarks of samsim_profile.hip, first line `# src_md5 <md5 of the sources>`")
    a = ap.parse_args()

    import samsim_amd
    from samsim_amd import testcases as tcs
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
    names = ["T", "S_bu", "psi_l"]
    na = g.ensemble_stats(["N_active"])["N_active"]
    layer_cells = float(na.mean) * int(na.count)          # sum of N_active over the columns that count
    row = layer_cells * 8.0

    def depth():
        return g.profile_stats(names, axis="depth", origin="top", nbins=a.bins, dz=a.dz)

    def layer():
        return g.profile_stats(names, axis="layer", origin="top")

    state = {}

    def get_state():
        state["s"] = None                                  # one host copy at a time
        state["s"] = g.get_state()

    q = depth()
    out = {"what": "samsim_get_profile_stats against samsim_get_state on one handle; host clock around the synchronising calls",
           "ncol": a.ncol, "nlayer": int(cfg.nlayer), "warmup_steps": a.warmup_steps, "failed_columns": int((status != 0).sum()),
           "sum_n_active": layer_cells, "arrays": names, "device": g.get_device()[1], "lib_md5": bench.lib_md5(),
           "hbm_achievable_TBps": HBM_ACHIEVABLE_TBS,
           "scratch_bytes_bound": header_define("SAMSIM_PROFILE_SCRATCH_BYTES"),
           "occupied_depth_bins": int((q["T"]["count"] > 0).sum())}
    t = timed(depth, a.calls, a.warmups)
    # distinct rows: T, psi_l, S_abs, m, thick; by passes: thick with each of the three arrays
    t.update(nbins=a.bins, dz=a.dz, bytes_needed=5 * row, bytes_read_by_passes=7 * row)
    t["TBps_needed_bytes"] = t["bytes_needed"] / (t["median_ms"] * 1e-3) / 1e12
    t["TBps_read_by_passes"] = t["bytes_read_by_passes"] / (t["median_ms"] * 1e-3) / 1e12
    out["by_depth"] = t
    t = timed(layer, a.calls, a.warmups)
    t.update(nbins=int(cfg.nlayer), bytes_needed=4 * row, bytes_read_by_passes=4 * row)      # T, psi_l, S_abs, m
    t["TBps_needed_bytes"] = t["bytes_needed"] / (t["median_ms"] * 1e-3) / 1e12
    out["by_layer"] = t
    t = timed(get_state, a.calls if a.get_state_calls is None else a.get_state_calls, a.warmups)
    t.update(bytes_to_host=15.0 * cfg.nlayer * a.ncol * 8)
    out["get_state"] = t
    out["get_state_over_by_depth"] = out["get_state"]["median_ms"] / out["by_depth"]["median_ms"]
    out["get_state_over_by_layer"] = out["get_state"]["median_ms"] / out["by_layer"]["median_ms"]
    out["reduction_faster_than_get_state"] = bool(out["by_depth"]["max_ms"] < out["get_state"]["min_ms"]
                                                  and out["by_layer"]["max_ms"] < out["get_state"]["min_ms"])
    ru = resource_usage(a.resource_usage)
    if ru:
        out["kernel_resource_usage"] = ru
    print(json.dumps(out, indent=1))
    if not out["reduction_faster_than_get_state"]:
        sys.exit("the device reduction did not beat samsim_get_state")


if __name__ == "__main__":
    main()
