#!/usr/bin/env python3
"""Cost of applying a resample on the device, on the headline ensemble (1 048 576 columns x 80 layers, SHEBA day-200 fixture tiled as
bench.py tiles it, 500 warm-up steps, the twin-experiment GAUSS row of tools/resample_bench.py).  Host wall clock around the blocking
call (the launches and the synchronisation included), medians of --repeats calls with min and max:

  apply_spread        samsim_apply_resample after a systematic draw of m = n_pool members on a GAUSS row tempered until the effective
                      sample size is about --ess of the pool; payload_gb_s counts the bytes of a column once read and once written
  apply_degenerate    ... on a row that leaves one member at 1.0: one source, every other running column a destination
  copy_262144         samsim_copy_columns of the first 262 144 pairs of the spread plan
  get_columns_262144  samsim_get_columns of the same sources, and set_state_262144 the upload of what it returned: the route the copy
                      replaces.  THE BAR: copy_262144 takes less time than get_columns_262144 alone (exit status 1 otherwise)
  step_after_apply    the first 500-step launch after an apply -- every wave that holds a copy runs the full first sweep once --
                      beside step_without, the next one
  step                with --parent-lib: `bench.py --gpus 1` for the parent commit's library and this one, alternating in one job
                      (step_ab of tools/select_bench.py; the step kernel is the parent's, so the two must agree within the parent's
                      own spread); written to --bench-out

    python tools/copy_bench.py --parent-lib samsim_amd/csrc/variants/libsamsim_hip_parent.so --bench-out profiles/rN_bench.json \\
        > profiles/rN_copy.json
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
from tools.select_bench import step_ab  # noqa: E402

PAIRS = 262144


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncol", type=int, default=1 << 20)
    ap.add_argument("--warmup-steps", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--ess", type=float, default=0.7, help="effective sample size of the spread row, as a share of the pool")
    ap.add_argument("--parent-lib", default=None, help="library of the parent commit for the comparison of the step")
    ap.add_argument("--bench-out", default=None, help="where the comparison of the step is written")
    ap.add_argument("--bench-steps", type=int, default=10)
    ap.add_argument("--bench-warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3, help="parent / new alternations of the comparison of the step")
    a = ap.parse_args()

    # the step against the parent: first, each run in a process of its own, before this process opens the GPU
    if a.parent_lib:
        ab = step_ab(a)
        if a.bench_out:
            with open(a.bench_out, "w") as f:
                json.dump(ab, f, indent=1)
        print("step: ratio of medians", ab["ratio_of_medians"], file=sys.stderr, flush=True)

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
    n_pool = int((status == 0).sum())
    nlayer = int(cfg.nlayer)
    # what a copy moves of one column: the fifteen layer arrays, the scalars below dT2m, N_active and the status triple
    column_bytes = capi.NARR * nlayer * 8 + capi.S["dT2m"] * 8 + 4 + 4 + 4 + 8
    out = {"what": "cost of samsim_apply_resample and samsim_copy_columns beside the route through the host; host wall clock around the "
                   "blocking calls", "ncol": a.ncol, "nlayer": nlayer, "warmup_steps": a.warmup_steps, "repeats": a.repeats,
           "device": g.get_device()[1], "lib_md5": bench.lib_md5(), "failed_columns": a.ncol - n_pool, "column_bytes": column_bytes}

    def note(label, t, **more):
        t.update(more)
        out[label] = t
        print(label, t["median_ms"], "ms", file=sys.stderr, flush=True)

    def payload(t, n):
        return 2.0 * n * column_bytes / (t["median_ms"] * 1e-3) / 1e9

    # the twin experiment of tools/resample_bench.py, the tempering chosen by bisection for the effective sample size asked for
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

    def draw():
        info = g.resample(n_pool, "systematic", u0=0.37)
        assert info["m_drawn"] == n_pool
        return info

    rinfo = draw()
    t, ainfo = timed(g.apply_resample, a.repeats, before=draw)            # the weights stay with the slots: every repeat has the same plan
    note("apply_spread", t, resample=rinfo, plan=ainfo, payload_gb_s=payload(t, ainfo["n_copies"]))
    src, dst = g.copy_plan()
    assert src.size == ainfo["n_copies"] and (np.diff(dst) > 0).all() and (np.diff(src) >= 0).all()
    kt, _ = timed(lambda: g.step_timed(a.warmup_steps), 1)
    note("step_after_apply", kt, steps=a.warmup_steps)
    kt, _ = timed(lambda: g.step_timed(a.warmup_steps), 1)
    note("step_without", kt, steps=a.warmup_steps)
    out["step_after_apply_over_without"] = out["step_after_apply"]["median_ms"] / out["step_without"]["median_ms"]

    # the bar: the copy of 262 144 pairs against the download it replaces
    n = min(PAIRS, src.size)
    s1, d1 = np.ascontiguousarray(src[:n]), np.ascontiguousarray(dst[:n])
    t, _ = timed(lambda: g.copy_columns(s1, d1), a.repeats)
    note(f"copy_{PAIRS}", t, pairs=n, payload_gb_s=payload(t, n))
    t, got = timed(lambda: g.get_columns(s1), 3)
    note(f"get_columns_{PAIRS}", t, columns=n, bytes_returned=int(got.lay.nbytes + got.scal.nbytes + got.n_active.nbytes))
    out["copy_over_get_columns"] = out[f"copy_{PAIRS}"]["median_ms"] / t["median_ms"]
    out["bar_copy_faster_than_get_columns"] = bool(out[f"copy_{PAIRS}"]["median_ms"] < t["median_ms"])

    # the degenerate posterior, as tools/resample_bench.py forms it: one column's melt_err far below the others'
    one = g.get_state(member, 1)
    one.scal[capi.S["melt_err"]] = -1.0e30
    g.set_state(one, member)
    dinfo = g.set_weights("melt_err", "gauss", 1.0)
    assert dinfo["n_pos"] == 1 and dinfo["sum_w"] == 1.0
    draw()
    t, ainfo = timed(g.apply_resample, a.repeats, before=draw)
    assert ainfo["n_sources"] == 1 and ainfo["n_copies"] == n_pool - 1
    note("apply_degenerate", t, plan=ainfo, payload_gb_s=payload(t, ainfo["n_copies"]))

    # last, because it overwrites the first columns of the handle: the upload half of the route through the host
    t, _ = timed(lambda: g.set_state(got, 0), 3)
    note(f"set_state_{PAIRS}", t, columns=n)
    out["host_route_ms"] = out[f"get_columns_{PAIRS}"]["median_ms"] + t["median_ms"]
    g.close()
    print(json.dumps(out, indent=1))
    return 0 if out["bar_copy_faster_than_get_columns"] else 1


if __name__ == "__main__":
    sys.exit(main())
